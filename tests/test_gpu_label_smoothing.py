"""GPU: the three -label_smoothing entries (csrc/label_smoothing.hip) through the C-ABI against torch.nn.KLDivLoss(reduction="sum") on
log_softmax(O Wg^T + b) in float64, the target distribution built as onmt/Loss.py:156-166 / onmt/VILoss.py:232-240 build it, gradients from
autograd, operands first rounded to the tested dtype.  dO, dWg and db are pre-filled with the plain (eps = 0) float64 result cast to f32, the
entries add their corrections, and the totals and the loss sum are compared with the smoothed float64 result.
Bound (the convention of tests/test_gpu_optim_methods.py and the mlp-attention tests): 4 x the error of the same torch computation in float32
on the same rounded operands against float64, plus 1 ulp of the f32 result (eps_f32 x the largest magnitude of the output); error = max |x - ref|.
The measured ratios are printed (LABNOTES.md holds a run).  On the commit before this feature the test fails at `lib.vmmt_ls_ws_floats`
(AttributeError: the library has no such symbol)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
PAD = 1
SHAPES = [(8, 67, 64),        # V not a multiple of 32, fewer rows than one workgroup takes
          (37, 515, 96),      # odd M, H not a multiple of 64
          (264, 130, 256)]    # more tokens than vocabulary entries: every target repeats
ULP = torch.finfo(torch.float32).eps


def _loss_and_grads(O, W, b, y, eps, inv_norm, dtype):
    O, W, b = (t.to(dtype).clone().requires_grad_(True) for t in (O, W, b))
    logits = O @ W.t() + b
    logp, V = torch.log_softmax(logits, 1), W.shape[0]
    if eps > 0:
        q = torch.full((1, V), eps / (V - 2), dtype=dtype)
        q[0, PAD] = 0
        q = q.repeat(y.numel(), 1).scatter_(1, y.unsqueeze(1), 1.0 - eps)
        q[y == PAD] = 0
        loss = torch.nn.KLDivLoss(reduction="sum")(logp, q)
    else:
        w = torch.ones(V, dtype=dtype)
        w[PAD] = 0
        loss = torch.nn.NLLLoss(w, reduction="sum")(logp, y)
    (loss * inv_norm).backward()
    nll = -logp.detach().gather(1, y.unsqueeze(1)).squeeze(1) * (y != PAD)
    return dict(loss=loss.detach(), dO=O.grad, dW=W.grad, db=b.grad, lse=torch.logsumexp(logits.detach(), 1), nll=nll)


@functools.lru_cache(maxsize=None)
def _case(M, V, H, dtype, eps):
    g = torch.Generator().manual_seed(M * 1000 + V)
    T = torch.bfloat16 if dtype == "bf16" else torch.float32
    O, W, b = (t.to(T).double() for t in (torch.randn(M, H, generator=g) * 0.5, torch.randn(V, H, generator=g) * 0.2, torch.randn(V, generator=g) * 0.1))
    y = torch.randint(2, V, (M,), generator=g)
    y[torch.randperm(M, generator=g)[:M // 4]] = PAD          # a quarter of the targets are pads
    y[0], y[2] = 0, V - 1
    inv_norm = 1.0 / 3.0
    plain, ref = (_loss_and_grads(O, W, b, y, e_, inv_norm, torch.float64) for e_ in (0.0, eps))
    f32 = _loss_and_grads(O, W, b, y, eps, inv_norm, torch.float32)
    return T, O, W, b, y, inv_norm, plain, ref, f32


@pytest.mark.parametrize("eps", (0.1, 0.3))
@pytest.mark.parametrize("compact", (False, True))
@pytest.mark.parametrize("dtype", ("bf16", "f32"))
@pytest.mark.parametrize("M,V,H", SHAPES)
def test_entries_against_fp64(M, V, H, dtype, compact, eps):
    from variational_mmt_amd import _lib as L
    lib, dev, st = L.lib(), torch.device("cuda"), torch.cuda.current_stream().cuda_stream
    T, O, W, b, y, inv_norm, plain, ref, f32 = _case(M, V, H, dtype, eps)
    ld, code = (H + 63) // 64 * 64, L.BF16 if dtype == "bf16" else L.F32

    def padded(x, t):               # [rows][ld] with zeros in the padding, as the engine's buffers
        out = torch.zeros(x.shape[0], ld, dtype=t, device=dev)
        out[:, :H] = x.to(t)
        return out
    Od, Wd, bd, yd = padded(O, T), padded(W, T), b.float().to(dev), y.to(dev)
    lse, nll = plain["lse"].float().to(dev), plain["nll"].float().to(dev)
    rows = None
    if compact:                     # the combine's list: the rows that carry a token, in order, then -1 up to a rounded count
        idx = torch.nonzero(y != PAD).squeeze(1)
        rows = torch.cat([idx, torch.full((5,), -1)]).to(torch.int32).to(dev)
    Mk, rp = (rows.numel(), rows.data_ptr()) if compact else (M, None)
    scratch = torch.zeros(int(lib.vmmt_ls_ws_floats(M, V, H)), device=dev)

    def run():
        wbar, bbar, obar, sums = torch.zeros(H, device=dev), torch.zeros(1, device=dev), torch.zeros(H, device=dev), torch.zeros(2, device=dev)
        dO, dW, db = padded(plain["dO"], torch.float32), plain["dW"].float().to(dev).contiguous(), plain["db"].float().to(dev)
        L.check(lib.vmmt_ls_colsum(code, Wd.data_ptr(), ld, bd.data_ptr(), V, H, PAD, wbar.data_ptr(), bbar.data_ptr(), scratch.data_ptr(), st), "colsum")
        L.check(lib.vmmt_ls_rows(code, Od.data_ptr(), ld, Wd.data_ptr(), ld, yd.data_ptr(), rp, Mk, V, H, PAD, eps, inv_norm, lse.data_ptr(),
                                 nll.data_ptr(), wbar.data_ptr(), bbar.data_ptr(), dO.data_ptr(), ld, obar.data_ptr(), sums.data_ptr(),
                                 scratch.data_ptr(), st), "rows")
        only = torch.zeros(2, device=dev)       # the loss-only mode: the same sum, nothing else touched
        L.check(lib.vmmt_ls_rows(code, Od.data_ptr(), ld, None, 0, yd.data_ptr(), rp, Mk, V, H, PAD, eps, 0.0, lse.data_ptr(), nll.data_ptr(),
                                 wbar.data_ptr(), bbar.data_ptr(), None, 0, None, only.data_ptr(), scratch.data_ptr(), st), "rows, loss only")
        L.check(lib.vmmt_ls_dW(code, Od.data_ptr(), ld, yd.data_ptr(), rp, Mk, V, H, PAD, eps, inv_norm, obar.data_ptr(), sums.data_ptr(),
                               dW.data_ptr(), H, db.data_ptr(), st), "dW")
        torch.cuda.synchronize()
        assert torch.equal(only[:1], sums[:1])
        return dict(loss=sums[0].cpu(), dO=dO.cpu(), dW=dW.cpu(), db=db.cpu(), wbar=wbar.cpu())
    got, again = run(), run()
    assert all(torch.equal(got[k], again[k]) for k in ("loss", "wbar", "dO"))          # fixed partitions, fixed fold order: equal bits
    assert torch.equal(got["dO"][:, H:], torch.zeros(M, ld - H))                        # the padding keeps its zeros
    for k in ("loss", "dO", "dW", "db"):
        x = got[k][:, :H] if k == "dO" else got[k]
        err, yard = (x.double() - ref[k]).abs().max().item(), (f32[k].double() - ref[k]).abs().max().item()
        bound = 4 * yard + ULP * ref[k].abs().max().item()
        print("%s M=%d V=%d H=%d %s compact=%s eps=%g: err %.3g, fp32 torch %.3g, err / bound %.3f" % (k, M, V, H, dtype, compact, eps, err, yard, err / bound))
        assert err <= bound, (k, err, bound)
