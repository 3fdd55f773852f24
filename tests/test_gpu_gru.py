"""GPU: vmmt_gru_chain_fwd / vmmt_gru_chain_bwd / vmmt_gru_step_bwd (mode 1) against the recurrence restated as a plain loop in fp64 on
the same (bf16-rounded) operands.  Reference arithmetic: torch nn.GRU as the reference model builds it (onmt/Models.py:124-129,140-147,
onmt/VI_Model1.py:137-152), packed-sequence masking via `lens`.

Bounds are measured, not invented: `_loop` in fp32 on the CPU against `_loop` in fp64 at the five shapes below, for the bf16 case with
everything the kernels store in bf16 rounded to bf16 (h handed from step to step, the gate gradients, the recurrent-side gradients on
their way into the next step's product); error = max |x - ref| / max(1e-3, max |ref|), largest over the shapes; the bound is 4 x that
(summation order, hardware exp / rcp).  Order: h_out, h_n, dgx, dgh, carry, dh0.
    bf16: measured  4.47e-03  4.94e-03  2.92e-03  3.67e-03  9.65e-04  1.21e-03
          bound     1.79e-02  1.98e-02  1.17e-02  1.47e-02  3.86e-03  4.84e-03
    f32:  measured  4.25e-07  4.27e-07  3.85e-07  2.75e-07  2.17e-07  2.09e-07
          bound     1.70e-06  1.71e-06  1.54e-06  1.10e-06  8.68e-07  8.36e-07"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUNDS = {"bf16": (1.79e-02, 1.98e-02, 1.17e-02, 1.47e-02, 3.86e-03, 4.84e-03),
          "f32": (1.70e-06, 1.71e-06, 1.54e-06, 1.10e-06, 8.68e-07, 8.36e-07)}
CASES = [(3, 64, 5, 1, False), (33, 512, 3, 1, False), (5, 96, 4, 2, True), (2, 40, 6, 1, True), (17, 1024, 2, 1, False)]


def _operands(B, H, S, dirs, ragged, dtype):
    T = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(B * 1000 + H + S)
    lens = torch.full((B,), S, dtype=torch.int64)
    if ragged:
        lens = torch.sort(torch.randint(1, S + 1, (B,), generator=g), descending=True)[0]
        lens[0], lens[-1] = S, 1
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    ops = []
    for k in range(dirs):
        ops.append(dict(w=rn(3 * H, H, sc=H ** -0.5).to(T), gx=rn(S, B, 3 * H), gx2=rn(B, 3 * H, sc=0.3), bhn=rn(H, sc=0.3),
                        h0=(rn(B, H, sc=0.5) if k == 0 else torch.zeros(B, H)).to(T), dha=rn(S, B, H, sc=0.1).to(T), dhn=rn(B, H, sc=0.1)))
    return ops, lens


def _loop(o, lens, reverse, dt, rnd):
    """one direction in precision `dt`; `rnd` rounds what the kernels store in T.  Returns h_out, h_n, dgx, dgh, carry, dh0"""
    w, gx, gx2, bhn, dha, dhn = (o[k].to(dt) for k in ("w", "gx", "gx2", "bhn", "dha", "dhn"))
    S, B, H = dha.shape
    ste = lambda x: x + (rnd(x) - x).detach()
    h0 = o["h0"].to(dt).requires_grad_()
    gx.requires_grad_()
    ah = torch.zeros(S, B, 3 * H, dtype=dt, requires_grad=True)                # its gradient is the recurrent-side gate gradient
    h, outs, cap = h0, [None] * S, torch.zeros(B, H, dtype=dt)
    order = range(S - 1, -1, -1) if reverse else range(S)
    for t in order:
        rec = h @ w.T
        rec.register_hook(rnd)                                                # dgh is stored in T before the next step multiplies it
        a, g = rec + ah[t], gx[t] + gx2
        r, z = torch.sigmoid(g[:, :H] + a[:, :H]), torch.sigmoid(g[:, H:2 * H] + a[:, H:2 * H])
        n = torch.tanh(g[:, 2 * H:] + r * (a[:, 2 * H:] + bhn))
        hnew = n + z * (h - n)
        cap = torch.where((lens - 1 == t if not reverse else torch.full((B,), t == 0)).view(B, 1), hnew, cap)
        h = outs[t] = ste(torch.where((lens > t).view(B, 1), hnew, torch.zeros_like(hnew)))
    ((torch.stack(outs) * dha).sum() + (cap * dhn).sum()).backward()
    dgh = rnd(ah.grad)
    last = 0 if not reverse else S - 1                                        # the step the backward processes last
    return torch.stack(outs).detach(), rnd(cap.detach()), rnd(gx.grad), dgh, h0.grad - dgh[last] @ w, h0.grad


def _err(got, ref):
    return (got.double() - ref).abs().max().item() / max(1e-3, ref.abs().max().item())


def measure(dtype):
    """the numbers in the docstring: python -c 'import tests.test_gpu_gru as t; print(t.measure("bf16"), t.measure("f32"))'"""
    rnd = (lambda x: x.bfloat16().to(x.dtype)) if dtype == "bf16" else (lambda x: x)
    worst = [0.0] * 6
    for B, H, S, dirs, ragged in CASES:
        ops, lens = _operands(B, H, S, dirs, ragged, dtype)
        for k in range(dirs):
            ref = _loop(ops[k], lens, k == 1, torch.double, lambda x: x)
            worst = [max(w_, _err(x, r)) for w_, x, r in zip(worst, _loop(ops[k], lens, k == 1, torch.float32, rnd), ref)]
    return worst


def _run(L, lib, ops, lens, B, H, S, dirs, ragged, dtype):
    T, code = (torch.bfloat16, L.BF16) if dtype == "bf16" else (torch.float32, L.F32)
    dev = lambda x, dt=None: x.to(device="cuda", dtype=dt or x.dtype).contiguous()
    z = lambda r, c, dt, fill=0.0: torch.full((r, c), fill, dtype=dt, device="cuda")
    P = lambda t_, row=0: t_.data_ptr() + row * t_.stride(0) * t_.element_size()
    lens_d = dev(lens) if ragged else None
    lp = C.c_void_p(lens_d.data_ptr()) if ragged else None
    bufs = []
    for o in ops:
        w = dev(o["w"])
        bufs.append(dict(w=w, wt=w.t().contiguous(), gx=dev(o["gx"].reshape(S * B, 3 * H)), gx2=dev(o["gx2"]), bhn=dev(o["bhn"]), h0=dev(o["h0"]),
                         dha=dev(o["dha"].reshape(S * B, H)), dhn=dev(o["dhn"]), out=z(S * B, H, T, 7.0), saved=z(S * B, 4 * H, T), hn=z(B, H, T),
                         dgx=z(S * B, 3 * H, T, 7.0), dgh=z(S * B, 3 * H, T, 7.0), carry=z(B, H, torch.float32), dh0=z(B, H, torch.float32, 7.0)))
    fwd, bwd = (L.GruDirFwd * (S * dirs))(), (L.GruDirBwd * (S * dirs + dirs))()
    for i in range(S):
        for k, b in enumerate(bufs):
            t, tp = (i, i - 1) if k == 0 else (S - 1 - i, S - i)               # forward: step i of direction k works on time t, after tp
            a = fwd[i * dirs + k]
            a.h_prev, a.ld_hprev = (P(b["h0"]), H) if i == 0 else (P(b["out"], tp * B), H)
            a.w_hh, a.ld_w, a.gx, a.ld_gx, a.gx2, a.ld_gx2, a.b_hn = P(b["w"]), H, P(b["gx"], t * B), 3 * H, P(b["gx2"]), 3 * H, P(b["bhn"])
            a.saved, a.ld_saved, a.h_out, a.ld_h, a.h_n, a.ld_hn, a.t = P(b["saved"], t * B), 4 * H, P(b["out"], t * B), H, P(b["hn"]), H, t
            a.capture = (1 if k == 0 else 2) if ragged else (3 if i == S - 1 else 0)
            t, tn = (S - 1 - i, S - i) if k == 0 else (i, i - 1)               # backward: the other way round, after tn
            a = bwd[i * dirs + k]
            if i > 0:
                a.dgh_next, a.ld_dgn = P(b["dgh"], tn * B), 3 * H
            a.w_hh_t, a.ld_wt, a.dh_above, a.ld_dha, a.saved, a.ld_saved = P(b["wt"]), 3 * H, P(b["dha"], t * B), H, P(b["saved"], t * B), 4 * H
            first = t == (0 if k == 0 else S - 1)                              # the step that h0 entered
            a.h_prev, a.ld_hp = (P(b["h0"]), H) if first else (P(b["out"], (t - 1 if k == 0 else t + 1) * B), H)
            a.dh_carry, a.ld_dhc, a.dgx_out, a.ld_dgx, a.dgh_out, a.ld_dgh = P(b["carry"]), H, P(b["dgx"], t * B), 3 * H, P(b["dgh"], t * B), 3 * H
            a.dh_n, a.ld_dhn, a.t = P(b["dhn"]), H, t
            a.inject = (1 if k == 0 else 2) if ragged else (3 if i == 0 else 0)
    for k, b in enumerate(bufs):                                               # mode 1: gradient of the initial state
        a = bwd[S * dirs + k]
        a.dgh_next, a.ld_dgn, a.w_hh_t, a.ld_wt = P(b["dgh"], (0 if k == 0 else S - 1) * B), 3 * H, P(b["wt"]), 3 * H
        a.dh_carry, a.ld_dhc, a.dh0_out, a.ld_dh0 = P(b["carry"]), H, P(b["dh0"]), H
    L.check(lib.vmmt_gru_chain_fwd(code, dirs, S, fwd, lp, B, H, None), "vmmt_gru_chain_fwd")
    L.check(lib.vmmt_gru_chain_bwd(code, dirs, S, bwd, lp, B, H, 0, None), "vmmt_gru_chain_bwd")
    last = C.cast(C.byref(bwd, S * dirs * C.sizeof(L.GruDirBwd)), C.POINTER(L.GruDirBwd))
    L.check(lib.vmmt_gru_step_bwd(code, dirs, last, lp, B, H, 1, None), "vmmt_gru_step_bwd")
    torch.cuda.synchronize()
    return [[b[n].float().cpu().view(*s) for n, s in (("out", (S, B, H)), ("hn", (B, H)), ("dgx", (S, B, 3 * H)), ("dgh", (S, B, 3 * H)),
                                                       ("carry", (B, H)), ("dh0", (B, H)))] for b in bufs]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("B,H,S,dirs,ragged", CASES)
def test_gru_chain_forward_backward(B, H, S, dirs, ragged, dtype):
    from variational_mmt_amd import _lib as L
    lib = L.lib()
    ops, lens = _operands(B, H, S, dirs, ragged, dtype)
    got = _run(L, lib, ops, lens, B, H, S, dirs, ragged, dtype)
    pad = (torch.arange(S).view(S, 1, 1) >= lens.view(1, B, 1))
    for k in range(dirs):
        ref = _loop(ops[k], lens, k == 1, torch.double, lambda x: x)
        errs = [_err(x, r) for x, r in zip(got[k], ref)]
        print(dtype, (B, H, S, dirs, ragged), "dir", k, " ".join("%.3g" % e for e in errs))
        for e, bound in zip(errs, BOUNDS[dtype]):
            assert e <= bound
        out, _, dgx, dgh = got[k][:4]
        assert (out[pad.expand(S, B, H)] == 0).all()
        assert (dgx[pad.expand(S, B, 3 * H)] == 0).all() and (dgh[pad.expand(S, B, 3 * H)] == 0).all()
        assert (dgx != 7.0).all() and (dgh != 7.0).all() and (out != 7.0).all()            # every row written
    again = _run(L, lib, ops, lens, B, H, S, dirs, ragged, dtype)                          # no atomics: the same bits
    assert all(torch.equal(a, b) for ga, gb in zip(got, again) for a, b in zip(ga, gb))
