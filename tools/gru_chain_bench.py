"""Times vmmt_gru_chain_fwd / vmmt_gru_chain_bwd alone on the chip next to vmmt_lstm_chain_fwd / vmmt_lstm_chain_bwd at the benchmark's two
recurrence shapes: bf16, device events around `--iters` back-to-back chains after a warm-up, `--reps` windows per entry with the entries
alternating.  A chain is `steps` launches of the per-step kernel; both cells get random operands of the same shapes, no `lens` (every
position valid), no per-sentence addend.
    python tools/gru_chain_bench.py [--out FILE]"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from variational_mmt_amd import _lib as L  # noqa: E402

SHAPES = [(256, 512, 20, 1), (256, 256, 20, 2)]          # (B, H, steps, directions): the decoder's and the encoder's recurrence in bench.py


def _chains(B, H, S, dirs, G):
    """step descriptors of a forward and a backward chain of a cell with G gate blocks (4: LSTM, 3: GRU); returns (fwd, bwd, keep-alive)"""
    g = torch.Generator().manual_seed(G)
    bf = lambda r, c, s: (torch.randn(r, c, generator=g) * s).to(torch.bfloat16).cuda()
    f32 = lambda r, c, s=0.0: (torch.randn(r, c, generator=g) * s).cuda()
    P = lambda t, row=0: t.data_ptr() + row * t.stride(0) * t.element_size()
    FT, BT = (L.LstmDirFwd, L.LstmDirBwd) if G == 4 else (L.GruDirFwd, L.GruDirBwd)
    fwd, bwd, keep = (FT * (S * dirs))(), (BT * (S * dirs))(), []
    for k in range(dirs):
        w = bf(G * H, H, H ** -0.5)
        b = dict(w=w, wt=w.t().contiguous(), gx=f32(S * B, G * H, 1.0), h0=bf(B, H, .5), out=bf(S * B, H, 0), sv=bf(S * B, 4 * H, 0),
                 dha=bf(S * B, H, .1), dg=bf(S * B, G * H, 0), dgx=bf(S * B, G * H, 0), carry=f32(B, H), c=f32((S + 1) * B, H), bhn=f32(1, H, .3))
        keep.append(b)
        for i in range(S):
            t, tp = (i, i - 1) if k == 0 else (S - 1 - i, S - i)
            a = fwd[i * dirs + k]
            a.h_prev, a.ld_hprev = (P(b["h0"]), H) if i == 0 else (P(b["out"], tp * B), H)
            a.w_hh, a.ld_w, a.gx, a.ld_gx, a.h_out, a.ld_h, a.t = P(b["w"]), H, P(b["gx"], t * B), G * H, P(b["out"], t * B), H, t
            if G == 4:                                       # cell state: row block i + 1 of `c` after step i, block 0 = c0
                a.c_prev, a.ld_cprev, a.c_out, a.ld_c, a.gates, a.ld_gates = P(b["c"], i * B), H, P(b["c"], (i + 1) * B), H, P(b["sv"], t * B), 4 * H
            else:
                a.b_hn, a.saved, a.ld_saved = P(b["bhn"]), P(b["sv"], t * B), 4 * H
            t, tn = (S - 1 - i, S - i) if k == 0 else (i, i - 1)
            a = bwd[i * dirs + k]
            a.w_hh_t, a.ld_wt, a.dh_above, a.ld_dha, a.t = P(b["wt"]), G * H, P(b["dha"], t * B), H, t
            if G == 4:
                j = S - 1 - i                                # forward step index of this time position
                if i > 0:
                    a.dgates_next, a.ld_dgn = P(b["dg"], tn * B), 4 * H
                a.gates, a.ld_gates, a.c_t, a.ld_ct, a.c_prev, a.ld_cp = P(b["sv"], t * B), 4 * H, P(b["c"], (j + 1) * B), H, P(b["c"], j * B), H
                a.dc_carry, a.ld_dcc, a.dgates_out, a.ld_dgo = P(b["carry"]), H, P(b["dg"], t * B), 4 * H
            else:
                if i > 0:
                    a.dgh_next, a.ld_dgn = P(b["dg"], tn * B), 3 * H
                first = t == (0 if k == 0 else S - 1)
                a.h_prev, a.ld_hp = (P(b["h0"]), H) if first else (P(b["out"], (t - 1 if k == 0 else t + 1) * B), H)
                a.saved, a.ld_saved, a.dh_carry, a.ld_dhc = P(b["sv"], t * B), 4 * H, P(b["carry"]), H
                a.dgx_out, a.ld_dgx, a.dgh_out, a.ld_dgh = P(b["dgx"], t * B), 3 * H, P(b["dg"], t * B), 3 * H
    return fwd, bwd, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3000)        # ~0.3 s of device time per window
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    lib = L.lib()
    lines = ["%s, bf16, us per chain and per step: median (min - max of the per-step figure) of %d windows of %d chains"
             % (torch.cuda.get_device_name(0), a.reps, a.iters)]
    for B, H, S, dirs in SHAPES:
        lf, lb, keep4 = _chains(B, H, S, dirs, 4)
        gf, gb, keep3 = _chains(B, H, S, dirs, 3)
        entries = {
            "vmmt_lstm_chain_fwd": lambda: lib.vmmt_lstm_chain_fwd(L.BF16, dirs, S, lf, None, B, H, None),
            "vmmt_gru_chain_fwd": lambda: lib.vmmt_gru_chain_fwd(L.BF16, dirs, S, gf, None, B, H, None),
            "vmmt_lstm_chain_bwd": lambda: lib.vmmt_lstm_chain_bwd(L.BF16, dirs, S, lb, None, B, H, 0, None),
            "vmmt_gru_chain_bwd": lambda: lib.vmmt_gru_chain_bwd(L.BF16, dirs, S, gb, None, B, H, 0, None),
        }
        times = {k: [] for k in entries}
        for k, fn in entries.items():                        # warm-up: code objects, LDS attributes; the forwards leave valid saved values
            for _ in range(10):
                L.check(fn(), k)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in entries.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        lines.append("(B, H, steps, directions) = (%d, %d, %d, %d)" % (B, H, S, dirs))
        for k, t in times.items():
            t = sorted(t)
            lines.append("  %-22s %8.1f per chain  %6.2f per step  (%.2f - %.2f)" % (k, t[len(t) // 2], t[len(t) // 2] / S, t[0] / S, t[-1] / S))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
