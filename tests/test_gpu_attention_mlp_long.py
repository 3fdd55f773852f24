"""GPU: vmmt_attn_mlp_bwd_long (the mlp attention's backward for sources of 65 - 256 positions and targets beyond 64) against fp64 math on
the same (bf16-rounded) operands, and one engine step whose batch is padded from the short kernel's range into the long one's.
Reference arithmetic: onmt/modules/GlobalAttention.py:114-127 (score), :171-184 (mask, softmax, context).

Bounds of test 1, measured as tests/test_gpu_attention_mlp.py describes, at the seven shapes below (one sentence of the B = 3 cases has
length 1): `_math` in fp32 on the CPU (dwq / duh rounded to bf16 for the bf16 case; dv is an f32 output in both) against `_math` in fp64,
error = max |x - ref| / max(1e-3, max |ref|), largest over the shapes; the bound is 4 x that (summation order, hardware exp / rcp):
            bf16: measured  dwq 3.21e-3  duh 2.98e-3  dv 1.28e-6    bound  dwq 1.28e-2  duh 1.19e-2  dv 5.1e-6
            f32:  measured  dwq 1.29e-6  duh 8.02e-7  dv 8.24e-7    bound  dwq 5.2e-6   duh 3.2e-6   dv 3.3e-6
dctx keeps that file's tol_g (3e-2 / 2e-5).

Bounds of test 2, measured on a pinned path: the identical comparison with attn = "general" (attn_bwd at S = 7, T' = 5 against
vmmt_attn_bwd_long at S = 70, T' = 69), largest per-tensor max |delta| / max |g| and relative ELBO / KL difference:
            general  bi64   grad 1.14e-7   elbo, kl 0 (equal bits)      uni40  grad 1.15e-7   elbo, kl 0 (equal bits)
            mlp      bi64   grad 8.40e-8   elbo, kl 0                   uni40  grad 1.15e-7   elbo, kl 8.8e-8
the bound is twice the larger `general` figure, and not below the project's f32 step tolerances (2e-4 of a tensor's largest gradient, 2e-5
for the statistics): 2e-4 and 2e-5."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_attention_mlp import _buf, _err, _forward, _math, _operands

pytestmark = pytest.mark.gpu

BOUNDS = {"bf16": (1.28e-2, 1.19e-2, 5.1e-6), "f32": (5.2e-6, 3.2e-6, 3.3e-6)}          # dwq, duh, dv
SHAPES = [(65, 5, 64, 2), (5, 65, 64, 2), (65, 65, 96, 3), (130, 200, 128, 2), (3, 256, 1024, 2), (70, 70, 72, 2), (20, 20, 512, 3)]
GENERAL = dict(grad=1.15e-7, stat=0.0)          # measured with attn = "general" (docstring)
TOL_GRAD, TOL_STAT = max(2 * GENERAL["grad"], 2e-4), max(2 * GENERAL["stat"], 2e-5)


def _ops(Tp, S, H, B, dtype):
    ops = _operands(Tp, S, H, B, dtype)
    if B == 3:                                     # one sentence of length 1
        uh, ctx, lens = ops[2], ops[4], ops[6]
        lens[2] = 1
        uh[1:, 2] = 0
        ctx[1:, 2] = 0
    return ops


def _backward_long(L, lib, d, dc, Tp, S, H, B, dtype):
    T = torch.bfloat16 if dtype == "bf16" else torch.float32
    M, MS = Tp * B, S * B
    DCAT = _buf(M, 2 * H, T)
    DCAT[:M, :H] = dc.reshape(M, H).cuda()
    DWQ, DUH, DCTX = _buf(M, H, T), _buf(MS, H, T), _buf(MS, H, T)
    DCTX.fill_(7.0)                                # every valid row must be overwritten, nothing beyond
    nparts, nscr = lib.vmmt_attn_mlp_bwd_long_dv_parts(Tp, B, H), lib.vmmt_attn_mlp_bwd_long_scratch(Tp, B, S, H)
    assert nparts > 0 and nscr > 0
    dvp = torch.full((nparts, H), 7.0, dtype=torch.float32, device="cuda")
    scr = torch.full((nscr,), float("nan"), dtype=torch.float32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.vmmt_attn_mlp_bwd_long(d["code"], P(DCAT), DCAT.shape[1], P(d["probs"]), P(d["WQ"]), d["WQ"].shape[1], P(d["bq"]), P(d["UH"]),
                                       d["UH"].shape[1], P(d["v"]), P(d["CTX"]), d["CTX"].shape[1], P(d["lens"]), P(DWQ), DWQ.shape[1],
                                       P(DUH), DUH.shape[1], P(DCTX), DCTX.shape[1], P(dvp), Tp, B, S, H, P(scr), None), "attn mlp bwd long")
    dv = torch.zeros(H, dtype=torch.float32, device="cuda")      # the caller's fold: the existing column-sum kernel
    L.check(lib.vmmt_colsum(L.F32, P(dvp), H, nparts, H, 0, 0, P(dv), None, None), "colsum")
    torch.cuda.synchronize()
    return DWQ, DUH, DCTX, dv


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("Tp,S,H,B", SHAPES)
def test_mlp_attention_backward_long(Tp, S, H, B, dtype):
    from variational_mmt_amd import _lib as L
    lib = L.lib()
    ops = _ops(Tp, S, H, B, dtype)
    lens = ops[6]
    _, _, dwq_ref, duh_ref, dctx_ref, dv_ref = _math(*ops, torch.double)
    M, MS = Tp * B, S * B
    d = _forward(L, lib, ops, Tp, S, H, B, dtype)
    out = _backward_long(L, lib, d, ops[5], Tp, S, H, B, dtype)
    DWQ, DUH, DCTX, dv = out
    got = (DWQ[:M, :H].float().cpu().view(Tp, B, H), DUH[:MS, :H].float().cpu().view(S, B, H), dv.cpu())
    got_dc = DCTX[:MS, :H].float().cpu().view(S, B, H)
    errs = [_err(x, r) for x, r in zip(got, (dwq_ref, duh_ref, dv_ref))] + [_err(got_dc, dctx_ref)]
    print("errors dwq, duh, dv, dctx:", " ".join("%.3g" % e for e in errs))
    for e, bound in zip(errs, BOUNDS[dtype] + (3e-2 if dtype == "bf16" else 2e-5,)):
        assert e <= bound, errs
    pad = (torch.arange(S).view(S, 1, 1) >= lens.view(1, B, 1)).expand(S, B, H)
    assert (got_dc[pad] == 0).all() and (got[1][pad] == 0).all()
    assert (DCTX[:MS, :H] != 7.0).all()
    assert (DWQ[M:] == 0).all() and (DUH[MS:] == 0).all() and (DCTX[MS:] == 7.0).all()
    # a second call returns the same bits (no atomics anywhere)
    out2 = _backward_long(L, lib, d, ops[5], Tp, S, H, B, dtype)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))


def _step(attn, cfg, pad_to):
    """(statistics, gradients) of one f32 training step; pad_to: rows of PAD appended to src and tgt up to that many"""
    from tests.test_gpu_attention_variants import CONFIGS
    from variational_mmt_amd.engine import Dims, Engine
    from variational_mmt_amd.engine.layout import PAD
    c = CONFIGS[cfg]
    e = Engine(Dims(40, 50, 32, c["hid"], 16, 64, 1, c["brnn"], 0.0, attn=attn), dtype="f32", device="cuda", seed=3, param_init=0.1)
    g = torch.Generator().manual_seed(0)
    B, S, T = 3, 7, 6
    lens = torch.tensor([7, 5, 2])
    src = torch.randint(4, 40, (S, B), generator=g)
    for b in range(B):
        src[lens[b]:, b] = PAD
    tgt = torch.randint(4, 50, (T, B), generator=g)
    e.set_image_table(torch.randn(B, 64, generator=g))
    eps = torch.randn(B, 16, generator=g)
    if pad_to:
        src = torch.cat([src, torch.full((pad_to - S, B), PAD)])
        tgt = torch.cat([tgt, torch.full((pad_to - T, B), PAD)])
    ws = e.forward(src, lens, tgt, torch.arange(B), training=True, eps=eps)
    e.loss_backward(ws, normalization=B)
    torch.cuda.synchronize()
    return e.read_stats(ws), {k: v.detach().double().cpu() for k, v in e.grads.items()}


def _padding_changes(attn, cfg):
    """(largest per-tensor max |delta| / max |g|, largest relative difference of ELBO and KL) between the natural and the padded batch"""
    (s0, g0), (s1, g1) = _step(attn, cfg, 0), _step(attn, cfg, 70)
    assert g0.keys() == g1.keys()
    dg = max((g1[k] - g0[k]).abs().max().item() / max(g0[k].abs().max().item(), 1e-12) for k in g0)
    ds = max(abs(s1[k] - s0[k]) / abs(s0[k]) for k in ("elbo", "td_kl_before"))
    return dg, ds


@pytest.mark.parametrize("cfg", ["bi64", "uni40"])
def test_padding_into_the_long_kernels_does_not_change_a_step(cfg):
    dg, ds = _padding_changes("mlp", cfg)
    print("padding changes the step by: gradients %.3g, statistics %.3g" % (dg, ds))
    assert dg <= TOL_GRAD and ds <= TOL_STAT, (dg, ds)
