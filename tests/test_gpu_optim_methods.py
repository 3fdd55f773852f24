"""GPU: -optim sgd | adagrad | adadelta as fused HIP updates (csrc/optim_methods.hip), through the C-ABI, against torch.optim.SGD / Adagrad /
Adadelta behind clip_grad_norm_ in fp64 on the CPU (the reference's onmt/Optim.py:56-67,94-96: only lr is passed, Adagrad's `sum` starts at
adagrad_accum), over consecutive updates with fresh gradients.
Bound: 4 x the error of torch's own fp32 optimisers against the fp64 ones at these same cases (the convention of tests/test_gpu_gru.py), error =
max |x - ref| / max(1e-3, max |ref|) per output, largest over a method's cases.  Measured on the CPU with torch 2.10 (FP32_ERR), reproduced by
`python -c "import tests.test_gpu_optim_methods as t; print(t.fp32_error())"`: sgd p 9.66e-08; adagrad p 9.74e-08, sum 4.03e-07; adadelta p
9.45e-08, square_avg 4.00e-07, acc_delta 2.49e-09 (`sum` / `square_avg` carry twice the error of the fp32 norm's clip coefficient; acc_delta stays
below 1e-3, so its error is in units of 1e-3).  The kernels' results play no part in it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
CLS = {"sgd": torch.optim.SGD, "adagrad": torch.optim.Adagrad, "adadelta": torch.optim.Adadelta}
KEYS = {"sgd": (), "adagrad": ("sum",), "adadelta": ("square_avg", "acc_delta")}
LR = {"sgd": 1.0, "adagrad": 0.1, "adadelta": 1.0}
MAX_NORM = 5.0
# span, (hole_lo, hole_n), (shadow_lo, shadow_n), max_blocks: the smallest shapes at which the dense kernel takes another path
GEOS = {"tail": (4 * 37 + 3, (0, 0), (0, 0), 0),                       # n = 4k + 3 below one grid stride
        "strides": (2 * 2048 + 4 * 5 + 3, (0, 0), (0, 0), 2),          # above two grid strides (2 x 256 x 4) of a grid forced to two workgroups
        "hole": (731, (200, 128), (0, 0), 0),                          # a hole in the middle, 603 = 4 * 150 + 3 elements around it
        "shadow": (1024, (0, 0), (256, 512), 0)}                       # a bf16 shadow over an inner sub-range
PARAMS = [(m, geo, clip, acc) for m in CLS for geo in GEOS for clip in (False, True) for acc in ((0.0, 0.1) if m == "adagrad" else (0.0,))]
FP32_ERR = {("sgd", "p"): 9.66e-8, ("adagrad", "p"): 9.74e-8, ("adagrad", "sum"): 4.03e-7,
            ("adadelta", "p"): 9.45e-8, ("adadelta", "square_avg"): 4.00e-7, ("adadelta", "acc_delta"): 2.49e-9}


def _err(x, ref):
    return ((x.double() - ref.double()).abs().max() / max(1e-3, ref.double().abs().max().item())).item()


def _data(n, clip, seed, steps=3):
    """fp32 parameters and `steps` gradients whose norm is clearly below (0.05 sqrt(n) <= 3.2) or above (2 sqrt(n) >= 24) MAX_NORM"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) * (2.0 if clip else 0.05) for _ in range(steps)]


def _torch_opt(method, p0, acc, dtype):
    q = torch.nn.Parameter(p0.to(dtype).clone())
    opt = CLS[method]([q], lr=LR[method])
    if method == "adagrad":
        opt.state[q]["sum"].fill_(acc)
    return q, opt


def _torch_run(method, p0, grads, acc, dtype):
    """the reference's Optim on the CPU: clip_grad_norm_ + torch's optimiser; returns {"p": ..., state key: ...}"""
    q, opt = _torch_opt(method, p0, acc, dtype)
    for g in grads:
        q.grad = g.to(dtype).clone()
        torch.nn.utils.clip_grad_norm_([q], MAX_NORM)
        opt.step()
    return dict({"p": q.detach()}, **{k: opt.state[q][k] for k in KEYS[method]})


def fp32_error():
    """torch's fp32 optimisers against its fp64 ones at the cases of this file: {(method, output): largest error}"""
    out = {}
    for m, geo, clip, acc in PARAMS:
        p0, grads = _data(GEOS[geo][0] - GEOS[geo][1][1], clip, GEOS[geo][0])
        a, b = _torch_run(m, p0, grads, acc, torch.float32), _torch_run(m, p0, grads, acc, torch.float64)
        for k in a:
            out[(m, k)] = max(out.get((m, k), 0.0), _err(a[k], b[k]))
    return out


@pytest.mark.parametrize("method,geo,clip,acc", PARAMS)
def test_dense_kernel_against_torch_fp64(method, geo, clip, acc):
    from variational_mmt_amd import _lib as L
    lib, dev, st = L.lib(), torch.device("cuda"), torch.cuda.current_stream().cuda_stream
    span, (h_lo, h_n), (s_lo, s_n), blocks = GEOS[geo]
    keep = torch.ones(span, dtype=torch.bool)
    keep[h_lo:h_lo + h_n] = False
    p0, grads = _data(span - h_n, clip, span)
    ref = _torch_run(method, p0, grads, acc, torch.float64)
    p, g = torch.full((span,), 7.0), torch.full((span,), 77.0)      # (the hole belongs to the row-wise kernel: never read or written here)
    p[keep] = p0
    p, g = p.to(dev), g.to(dev)
    s1, s2 = torch.full((span,), acc if method == "adagrad" else 0.0, device=dev), torch.zeros(span, device=dev)
    before = [t.clone() for t in (p, s1, s2)]
    shadow = torch.zeros(max(s_n, 4), dtype=torch.bfloat16, device=dev)
    sq = torch.zeros(L.SUMSQ_SCRATCH, dtype=torch.float32, device=dev)
    skip = torch.zeros(2, dtype=torch.int32, device=dev)

    def launch():
        L.check(lib.vmmt_optim_step_ranges(L.OPTIM_METHODS[method], p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), span, h_lo, h_n,
                                           LR[method], MAX_NORM, sq.data_ptr(), 1.0, blocks, shadow.data_ptr() if s_n else None, s_lo, s_n,
                                           skip.data_ptr(), st), "optim_step_ranges")
        torch.cuda.synchronize()
    for g0 in grads:
        g[keep.to(dev)] = g0.to(dev)
        sq[:L.SUMSQ_SLOTS].zero_()
        L.check(lib.vmmt_sumsq(g.data_ptr(), h_lo if h_n else span, sq.data_ptr(), 0, st), "sumsq")
        if h_n:
            L.check(lib.vmmt_sumsq(g.data_ptr() + 4 * (h_lo + h_n), span - h_lo - h_n, sq.data_ptr(), 1, st), "sumsq")
        launch()
    for k, r in ref.items():
        e = _err(dict(p=p, **dict(zip(KEYS[method], (s1, s2))))[k].cpu()[keep], r)
        print("%s %s clip=%s acc=%g %s: %.3g (bound %.3g)" % (method, geo, clip, acc, k, e, 4 * FP32_ERR[(method, k)]))
        assert e <= 4 * FP32_ERR[(method, k)], (k, e)
    # the hole, and the state arrays a method does not use, are never written
    assert all(torch.equal(t.cpu()[~keep], b.cpu()[~keep]) for t, b in zip((p, s1, s2), before))
    assert (torch.equal(s2, before[2]) or method == "adadelta") and (torch.equal(s1, before[1]) or method != "sgd")
    if s_n:                                                 # the shadow is the bf16 rounding of the kernel's own fp32 result, bit for bit
        assert torch.equal(shadow.view(torch.int16), p[s_lo:s_lo + s_n].to(torch.bfloat16).view(torch.int16))
    # guard word set: the step is not applied -- parameters, state and shadow keep their bits, skip[1] counts the launch
    now = [t.clone() for t in (p, s1, s2, shadow)]
    assert skip.tolist() == [0, 0]
    skip[0] = 1
    launch()
    assert all(torch.equal(a, b) for a, b in zip((p, s1, s2, shadow), now)) and skip.tolist() == [1, 1]


@pytest.mark.parametrize("method", ("sgd", "adagrad"))
@pytest.mark.parametrize("Cc", (4, 260, 516))               # inside the first 256-column chunk, across both, into a second pass
def test_rows_kernel(method, Cc):
    """R = 130: two full 64-row blocks and a tail; a third of the rows flagged, roll = 4, stale gradient in the unflagged rows"""
    from variational_mmt_amd import _lib as L
    lib, dev, st = L.lib(), torch.device("cuda"), torch.cuda.current_stream().cuda_stream
    R, roll, code, acc = 130, 4, L.OPTIM_METHODS[method], 0.1
    gen = torch.Generator().manual_seed(Cc)
    p0 = torch.randn(R, Cc, generator=gen)
    p, g = p0.to(dev), torch.randn(R, Cc, generator=gen).to(dev)         # g: stale, non-zero everywhere
    s1, v = torch.full((R, Cc), acc if method == "adagrad" else 0.0, device=dev), torch.zeros(R, Cc, device=dev)
    dp, ds1 = p.clone(), s1.clone()                                     # the dense kernel's twin, fed zeros outside the flagged rows
    q, opt = _torch_opt(method, p0, acc, torch.float64)                 # fp64 reference: torch on the whole table, zero gradient elsewhere
    flags, last = torch.zeros(2 * R, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
    hist = torch.zeros(L.LAZY_HIST_WORDS, dtype=torch.int32, device=dev)
    rowsq, sq = torch.zeros(R, dtype=torch.float32, device=dev), torch.zeros(L.SUMSQ_SCRATCH, dtype=torch.float32, device=dev)
    ptrs, book = (p.data_ptr(), g.data_ptr(), s1.data_ptr(), v.data_ptr()), (flags.data_ptr(), last.data_ptr(), hist.data_ptr())
    for step, scale in ((1, 0.01), (2, 1.0)):                           # clip inactive (norm <= 1.5), then active (norm >= 13)
        rows = torch.randperm(R, generator=gen)[:R // 3].sort().values
        ids = rows.to(dev)
        L.check(lib.vmmt_rows_mark(ids.data_ptr(), ids.numel(), flags.data_ptr(), R, hist.data_ptr(), st), "mark")
        L.check(lib.vmmt_rows_catchup(*ptrs, R, Cc, *book, 0.9, 0.999, 1e-9, 0, st), "catchup 0")
        g_dense = torch.zeros(R, Cc)
        g_dense[rows] = torch.randn(rows.numel(), Cc, generator=gen) * scale
        gd = g_dense.to(dev)
        g[ids] = gd[ids]
        before = (p.clone(), s1.clone(), last.clone())
        sq[:L.SUMSQ_SLOTS].zero_()
        L.check(lib.vmmt_sumsq_rows(g.data_ptr(), R, Cc, flags.data_ptr(), hist.data_ptr(), rowsq.data_ptr(), sq.data_ptr(), 3, st), "sumsq_rows")
        L.check(lib.vmmt_optim_rows_step(code, *ptrs[:3], R, Cc, *book, LR[method], step, roll, MAX_NORM, sq.data_ptr(), 1.0, None, st), "rows_step")
        L.check(lib.vmmt_optim_step_ranges(code, dp.data_ptr(), gd.data_ptr(), ds1.data_ptr(), None, R * Cc, 0, 0, LR[method], MAX_NORM, sq.data_ptr(),
                                           1.0, 0, None, 0, 0, None, st), "dense twin")
        torch.cuda.synchronize()
        q.grad = g_dense.double()
        torch.nn.utils.clip_grad_norm_([q], MAX_NORM)
        opt.step()
        un = torch.ones(R, dtype=torch.bool)
        un[rows] = False
        assert torch.equal(p.cpu()[un], before[0].cpu()[un]) and torch.equal(s1.cpu()[un], before[1].cpu()[un])      # unflagged: untouched
        assert torch.equal(p[ids], dp[ids]) and torch.equal(s1[ids], ds1[ids])                                        # flagged: the dense kernel's bits
        for k, x, r in (("p", p, q.detach()),) + ((("sum", s1, opt.state[q]["sum"]),) if method == "adagrad" else ()):
            e = _err(x.cpu()[rows], r[rows])
            print("%s C=%d step %d %s: %.3g" % (method, Cc, step, k, e))
            assert e <= 4 * FP32_ERR[(method, k)], (k, e)
        moved = ~un | (torch.arange(R) % roll == step % roll)
        assert torch.equal(last.cpu(), torch.where(moved, torch.tensor(step, dtype=torch.int32), before[2].cpu()))
        entry = hist[4 + 4 * step:8 + 4 * step]                         # the ring: (lr, 0, applied = 0, step) -- nothing to replay
        assert int(hist[0]) == step and entry[:3].view(torch.float32).tolist() == [torch.tensor(LR[method]).item(), 0.0, 0.0] and int(entry[3]) == step
    # a flush finds nothing to replay: parameters and state keep their bits, every row is current, no ring error
    now = (p.clone(), s1.clone(), v.clone())
    L.check(lib.vmmt_rows_catchup(ptrs[0], None, ptrs[2], ptrs[3], R, Cc, None, *book[1:], 0.9, 0.999, 1e-9, 1, st), "catchup 1")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, s1, v), now)) and (last == 2).all() and int(hist[1]) == 0
