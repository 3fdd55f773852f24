"""GPU: vmmt_attn_mlp_fwd / vmmt_attn_mlp_bwd (Bahdanau attention, score = v . tanh(W_q r + b_q + W_c Hs)) against fp64 math on the
same (bf16-rounded) operands.  Reference arithmetic: onmt/modules/GlobalAttention.py:114-127 (score), :171-184 (mask, softmax, context).

Bounds.  probs, cat and dctx: test_gpu_attention.py's values for the same quantity and dtype.  dwq, duh and dv were measured: `_math` below
in fp32 on the CPU (dwq / duh rounded to bf16 for the bf16 case; dv is an f32 output in both) against `_math` in fp64 at the seven shapes of
test 1, error = max |x - ref| / max(1e-3, max |ref|), largest over the shapes; the bound is 4 x that (summation order, hardware exp / rcp):
            bf16: measured  dwq 3.03e-3  duh 3.75e-3  dv 1.34e-6    bound  dwq 1.21e-2  duh 1.50e-2  dv 5.3e-6
            f32:  measured  dwq 1.55e-6  duh 9.76e-7  dv 9.55e-7    bound  dwq 6.2e-6   duh 3.9e-6   dv 3.8e-6"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUNDS = {"bf16": (1.21e-2, 1.50e-2, 5.3e-6), "f32": (6.2e-6, 3.9e-6, 3.8e-6)}          # dwq, duh, dv


def _ru(x, m):
    return (x + m - 1) // m * m


def _buf(rows, cols, dtype, fill=None):
    t = torch.zeros(_ru(rows, 64) + 64, _ru(cols, 64), dtype=dtype, device="cuda")
    if fill is not None:
        t[:rows, :cols] = fill.to(device="cuda", dtype=dtype)
    return t


def _operands(Tp, S, H, B, dtype):
    T = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(Tp * 1000 + S * 10 + B)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    lens, _ = torch.sort(lens, descending=True)
    wq = (torch.randn(Tp, B, H, generator=g) * 0.5).to(T)
    uh = (torch.randn(S, B, H, generator=g) * 0.5).to(T)
    ctx = (torch.randn(S, B, H, generator=g) * 0.3).to(T)
    for b in range(B):
        ctx[lens[b]:, b] = 0                       # encoder memory is zero at pads (packed sequence), and so is W_c Hs
        uh[lens[b]:, b] = 0
    dc = (torch.randn(Tp, B, H, generator=g) * 0.1).to(T)
    bq = torch.randn(H, generator=g) * 0.1
    v = torch.randn(H, generator=g) * 0.3
    return wq, bq, uh, v, ctx, dc, lens


def _math(wq, bq, uh, v, ctx, dc, lens, dt):
    """the formulas, in precision `dt`: probs, context, dwq, duh, dctx (direct path), dv"""
    wq, bq, uh, v, ctx, dc = (x.to(dt) for x in (wq, bq, uh, v, ctx, dc))
    S, B = ctx.shape[:2]
    th = torch.tanh(wq[:, :, None, :] + bq + uh.permute(1, 0, 2)[None])             # [Tp][B][S][H]
    mask = torch.arange(S).view(1, 1, S) >= lens.view(1, B, 1)
    pr = torch.softmax((th @ v).masked_fill(mask, float("-inf")), dim=2)
    c = torch.einsum("tbs,sbh->tbh", pr, ctx)
    dp = torch.einsum("tbh,sbh->tbs", dc, ctx)
    ds = pr * (dp - (pr * dp).sum(2, keepdim=True))
    g = ds[..., None] * v * (1 - th * th)
    return pr, c, g.sum(2), g.sum(0).permute(1, 0, 2), torch.einsum("tbs,tbh->sbh", pr, dc), (ds[..., None] * th).sum((0, 1, 2))


def _err(got, ref):
    return (got.double() - ref).abs().max().item() / max(1e-3, ref.abs().max().item())


def _forward(L, lib, ops, Tp, S, H, B, dtype):
    wq, bq, uh, v, ctx, dc, lens = ops
    T = torch.bfloat16 if dtype == "bf16" else torch.float32
    M, MS = Tp * B, S * B
    d = dict(code=L.BF16 if dtype == "bf16" else L.F32, WQ=_buf(M, H, T, wq.reshape(M, H)), UH=_buf(MS, H, T, uh.reshape(MS, H)),
             CTX=_buf(MS, H, T, ctx.reshape(MS, H)), CAT=_buf(M, 2 * H, T), bq=bq.cuda(), v=v.cuda(), lens=lens.cuda(),
             probs=torch.zeros(M * S, dtype=torch.float32, device="cuda"))
    P = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.vmmt_attn_mlp_fwd(d["code"], P(d["WQ"]), d["WQ"].shape[1], P(d["bq"]), P(d["UH"]), d["UH"].shape[1], P(d["v"]), P(d["CTX"]),
                                  d["CTX"].shape[1], P(d["lens"]), P(d["CAT"]), d["CAT"].shape[1], P(d["probs"]), Tp, B, S, H, None), "attn mlp fwd")
    torch.cuda.synchronize()
    return d


def _backward(L, lib, d, dc, Tp, S, H, B, dtype):
    T = torch.bfloat16 if dtype == "bf16" else torch.float32
    M, MS = Tp * B, S * B
    DCAT = _buf(M, 2 * H, T)
    DCAT[:M, :H] = dc.reshape(M, H).cuda()
    DWQ, DUH, DCTX = _buf(M, H, T), _buf(MS, H, T), _buf(MS, H, T)
    DCTX.fill_(7.0)                                # every valid row must be overwritten
    nparts = lib.vmmt_attn_mlp_dv_parts(B, H)
    dvp = torch.full((max(nparts, 1), H), 7.0, dtype=torch.float32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.vmmt_attn_mlp_bwd(d["code"], P(DCAT), DCAT.shape[1], P(d["probs"]), P(d["WQ"]), d["WQ"].shape[1], P(d["bq"]), P(d["UH"]),
                               d["UH"].shape[1], P(d["v"]), P(d["CTX"]), d["CTX"].shape[1], P(d["lens"]), P(DWQ), DWQ.shape[1], P(DUH),
                               DUH.shape[1], P(DCTX), DCTX.shape[1], P(dvp), Tp, B, S, H, None)
    if rc != 0:
        return rc, None
    dv = torch.zeros(H, dtype=torch.float32, device="cuda")      # the caller's fold: the existing column-sum kernel
    L.check(lib.vmmt_colsum(L.F32, P(dvp), H, nparts, H, 0, 0, P(dv), None, None), "colsum")
    torch.cuda.synchronize()
    return 0, (DWQ, DUH, DCTX, dv)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("Tp,S,H,B", [(3, 5, 64, 2), (20, 20, 512, 3), (64, 64, 1024, 2), (7, 64, 96, 3), (64, 9, 512, 2), (1, 64, 1024, 2),
                                     (5, 12, 72, 2)])       # H % 32 != 0: bf16 takes the plain kernels too
def test_mlp_attention_forward_backward(Tp, S, H, B, dtype):
    from variational_mmt_amd import _lib as L
    lib = L.lib()
    ops = _operands(Tp, S, H, B, dtype)
    lens = ops[6]
    pr, cvec, dwq_ref, duh_ref, dctx_ref, dv_ref = _math(*ops, torch.double)
    M, MS = Tp * B, S * B
    d = _forward(L, lib, ops, Tp, S, H, B, dtype)
    got_p = d["probs"].view(Tp, B, S).cpu().double()
    tol_p, tol_c, tol_g = (2e-2, 2e-2, 3e-2) if dtype == "bf16" else (1e-5, 1e-5, 2e-5)
    mask = torch.arange(S).view(1, 1, S) >= lens.view(1, B, 1)
    assert (got_p - pr).abs().max().item() <= tol_p
    assert (got_p.sum(2) - 1).abs().max().item() <= 1e-5
    assert (got_p[mask.expand(Tp, B, S)] == 0).all()
    got_c = d["CAT"][:M, :H].float().cpu().double().view(Tp, B, H)
    assert (got_c - cvec).abs().max().item() <= tol_c * max(1.0, cvec.abs().max().item())
    assert (d["CAT"][:M, H:] == 0).all() and (d["CAT"][M:] == 0).all()    # only the left half of [c ; r], only valid rows
    rc, out = _backward(L, lib, d, ops[5], Tp, S, H, B, dtype)
    assert rc == 0
    DWQ, DUH, DCTX, dv = out
    got = (DWQ[:M, :H].float().cpu().view(Tp, B, H), DUH[:MS, :H].float().cpu().view(S, B, H), dv.cpu())
    errs = [_err(x, r) for x, r in zip(got, (dwq_ref, duh_ref, dv_ref))]
    got_dc = DCTX[:MS, :H].float().cpu().view(S, B, H)
    for e, bound in zip(errs, BOUNDS[dtype]):
        assert e <= bound
    assert _err(got_dc, dctx_ref) <= tol_g
    pad = torch.arange(S).view(S, 1, 1) >= lens.view(1, B, 1)
    assert (got_dc[pad.expand(S, B, H)] == 0).all() and (got[1][pad.expand(S, B, H)] == 0).all()
    assert (DCTX[:MS, :H] != 7.0).all()
    assert (DWQ[M:] == 0).all() and (DUH[MS:] == 0).all()
    # a second call returns the same bits (no atomics anywhere)
    d2 = _forward(L, lib, ops, Tp, S, H, B, dtype)
    _, out2 = _backward(L, lib, d2, ops[5], Tp, S, H, B, dtype)
    assert torch.equal(d2["probs"], d["probs"]) and torch.equal(d2["CAT"], d["CAT"])
    assert all(torch.equal(a, b) for a, b in zip(out, out2))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("Tp,S,H,B", [(1, 200, 512, 2), (5, 65, 96, 3)])
def test_mlp_attention_forward_long_sources(Tp, S, H, B, dtype):
    from variational_mmt_amd import _lib as L
    lib = L.lib()
    ops = _operands(Tp, S, H, B, dtype)
    pr, cvec = _math(*ops, torch.double)[:2]
    d = _forward(L, lib, ops, Tp, S, H, B, dtype)
    got_p = d["probs"].view(Tp, B, S).cpu().double()
    tol_p, tol_c = (2e-2, 2e-2) if dtype == "bf16" else (1e-5, 1e-5)
    assert (got_p - pr).abs().max().item() <= tol_p
    assert (got_p[(torch.arange(S).view(1, 1, S) >= ops[6].view(1, B, 1)).expand(Tp, B, S)] == 0).all()
    got_c = d["CAT"][:Tp * B, :H].float().cpu().double().view(Tp, B, H)
    assert (got_c - cvec).abs().max().item() <= tol_c * max(1.0, cvec.abs().max().item())
    if S == 65:                                    # a long-source backward does not exist: refused, not served wrongly
        assert _backward(L, lib, d, ops[5], Tp, S, H, B, dtype)[0] == 1
