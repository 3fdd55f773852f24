"""Times vmmt_attn_mlp_fwd / vmmt_attn_mlp_bwd alone on the chip, next to vmmt_attn_fwd / vmmt_attn_bwd ("general") at the same shapes:
bf16, device events around `--iters` back-to-back launches after a warm-up, `--reps` windows per kernel with the kernels alternating.
    python tools/attn_mlp_bench.py [--long] [--out FILE]
--long: the backward beyond the per-sentence kernels, vmmt_attn_mlp_bwd_long next to vmmt_attn_bwd_long ("general") at LONG_SHAPES; where a
shape still fits the short kernels (S, T' <= 64) they are timed too -- that comparison is why the engine keeps them below 65.
The score of the mlp attention is H tanh per (t, s) pair where "general" does H FMAs on the matrix pipe; the table says what that costs."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from variational_mmt_amd import _lib as L  # noqa: E402

SHAPES = [(20, 20, 512, 256), (64, 64, 1024, 128)]          # (T', S, H, B): BASELINE config 2 / config 5 at half its batch
LONG_SHAPES = [(64, 64, 512, 64), (100, 100, 512, 64), (100, 100, 512, 8), (256, 256, 1024, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    lines = ["%s, bf16, us per launch: median (min - max) of %d windows of %d launches" % (torch.cuda.get_device_name(0), a.reps, a.iters)]
    for Tp, S, H, B in (LONG_SHAPES if a.long else SHAPES):
        g = torch.Generator().manual_seed(1)
        M, MS = Tp * B, S * B
        rnd = lambda r, c, s: (torch.randn(r, c, generator=g) * s).to(torch.bfloat16).cuda()
        lens = torch.randint(S // 2, S + 1, (B,), generator=g).sort(descending=True)[0].cuda()
        Q, UH, CTX, CAT, DCAT = rnd(M, H, .5), rnd(MS, H, .5), rnd(MS, H, .3), rnd(M, 2 * H, .1), rnd(M, 2 * H, .1)
        DQ, DUH, DCTX = torch.zeros_like(Q), torch.zeros_like(UH), torch.zeros_like(CTX)
        bq, v = (torch.randn(H, generator=g) * .1).cuda(), (torch.randn(H, generator=g) * .3).cuda()
        probs = torch.zeros(M * S, device="cuda")
        dvp = torch.zeros(lib.vmmt_attn_mlp_dv_parts(B, H), H, device="cuda")
        kernels = {
            "vmmt_attn_mlp_fwd": lambda: lib.vmmt_attn_mlp_fwd(L.BF16, P(Q), H, P(bq), P(UH), H, P(v), P(CTX), H, P(lens), P(CAT), 2 * H,
                                                               P(probs), Tp, B, S, H, None),
            "vmmt_attn_mlp_bwd": lambda: lib.vmmt_attn_mlp_bwd(L.BF16, P(DCAT), 2 * H, P(probs), P(Q), H, P(bq), P(UH), H, P(v), P(CTX), H,
                                                               P(lens), P(DQ), H, P(DUH), H, P(DCTX), H, P(dvp), Tp, B, S, H, None),
            "vmmt_attn_fwd": lambda: lib.vmmt_attn_fwd(L.BF16, P(Q), H, P(CTX), H, P(lens), P(CAT), 2 * H, P(probs), Tp, B, S, H, None),
            "vmmt_attn_bwd": lambda: lib.vmmt_attn_bwd(L.BF16, P(DCAT), 2 * H, P(probs), P(Q), H, P(CTX), H, P(lens), P(DQ), H, P(DCTX), H,
                                                       Tp, B, S, H, None),
        }
        if a.long:
            short = {k: f for k, f in kernels.items() if k.endswith("_bwd") and S <= 64 and Tp <= 64}
            dvl = torch.zeros(lib.vmmt_attn_mlp_bwd_long_dv_parts(Tp, B, H), H, device="cuda")
            scr = torch.zeros(lib.vmmt_attn_mlp_bwd_long_scratch(Tp, B, S, H), device="cuda")
            dots = torch.zeros(M, device="cuda")
            L.check(kernels["vmmt_attn_mlp_fwd"](), "vmmt_attn_mlp_fwd")          # valid probs for the backward kernels
            kernels = dict(short)
            kernels["vmmt_attn_mlp_bwd_long"] = lambda: lib.vmmt_attn_mlp_bwd_long(
                L.BF16, P(DCAT), 2 * H, P(probs), P(Q), H, P(bq), P(UH), H, P(v), P(CTX), H, P(lens), P(DQ), H, P(DUH), H, P(DCTX), H, P(dvl),
                Tp, B, S, H, P(scr), None)
            kernels["vmmt_attn_bwd_long"] = lambda: lib.vmmt_attn_bwd_long(L.BF16, P(DCAT), 2 * H, P(probs), P(Q), H, P(CTX), H, P(lens), P(DQ),
                                                                           H, P(DCTX), H, Tp, B, S, H, P(dots), None)
        times = {k: [] for k in kernels}
        for k, fn in kernels.items():                        # warm-up: code objects, LDS attributes; the forward leaves valid probs
            for _ in range(10):
                L.check(fn(), k)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        tanh = Tp * S * H * B                                # upper bound (full-length sentences) of tanh evaluations per forward
        lines.append("(T', S, H, B) = (%d, %d, %d, %d): %.1f M tanh per forward, as many again in the backward" % (Tp, S, H, B, tanh / 1e6))
        for k, t in times.items():
            t = sorted(t)
            lines.append("  %-24s %8.1f  (%.1f - %.1f)" % (k, t[len(t) // 2], t[0], t[-1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
