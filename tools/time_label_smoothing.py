"""What -label_smoothing costs at BASELINE config 2 (bench.py's shape and batches, bf16, dropout 0.5): the training step with
label_smoothing 0 against 0.1 on the same build, one engine per process, the arms taking turns (`--reps` rounds, each child timing `--steps`
steps behind `--warmup`; host clock around a device synchronise), and the three entries of csrc/label_smoothing.hip alone at the same shape
(`--entries`: device events around `--entry-iters` back-to-back launches on an otherwise idle GPU, median of `--reps` windows, in us).
Prints one JSON line for the step and one for the entries.

    python tools/time_label_smoothing.py [--steps 50] [--reps 3] [--warmup 10]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from variational_mmt_amd import _lib as L  # noqa: E402
from variational_mmt_amd.engine import Dims, Engine  # noqa: E402

B, PAD = 256, 1


def step_arm(eps, steps, warmup):
    cf, dev = bench.CONFIGS["2"], torch.device("cuda")
    d = Dims(vs=cf["vs"], vt=cf["vt"], emb=cf["emb"], hid=cf["hid"], z=cf["z"], img=cf["img"], layers=cf["layers"], brnn=cf["brnn"], dropout=0.5)
    eng = Engine(d, dtype="bf16", device=dev, seed=0)
    eng.set_image_table(torch.rand(cf["n_img"], d.img, generator=torch.Generator().manual_seed(11)))
    batches = bench.make_batches(d, B, cf["S"], cf["T"], cf["n_img"], 8, dev, 1234, ragged=False)
    eng.hold_back = True

    def window(first, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(first, first + n):
            src, sl, tgt, idx, tlen, n_tok = batches[i % len(batches)]
            ws = eng.forward(src, sl, tgt, idx, training=True, n_tgt_tokens=n_tok)
            eng.loss_backward(ws, normalization=B, batch_global=B, label_smoothing=eps)
            eng.optim_step(lr=0.002, max_grad_norm=5.0)
        eng.wait_background()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    window(0, warmup)
    ms = window(warmup, steps)
    eng.check_async_errors()
    return dict(ms=ms)


def entries(iters, reps, eps=0.1):
    """the three entries alone: M = 256 x 20 token rows, V = 30000, H = 512, bf16; every token a target (config 2 has no pads)"""
    cf, dev, lib = bench.CONFIGS["2"], torch.device("cuda"), L.lib()
    M, V, H = B * (cf["T"] - 1), cf["vt"], cf["hid"]
    g = torch.Generator(device=dev).manual_seed(3)
    O, W = (torch.randn(r, H, device=dev, generator=g).mul_(s).to(torch.bfloat16) for r, s in ((M, 0.5), (V, 0.1)))
    bias, y = torch.zeros(V, device=dev), torch.randint(4, V, (M,), device=dev, generator=g)
    lse, nll = torch.full((M,), 10.3, device=dev), torch.full((M,), 10.3, device=dev)
    dO, dW, db = torch.zeros(M, H, device=dev), torch.zeros(V, H, device=dev), torch.zeros(V, device=dev)
    wbar, bbar, obar, sums = torch.zeros(H, device=dev), torch.zeros(1, device=dev), torch.zeros(H, device=dev), torch.zeros(2, device=dev)
    scratch = torch.zeros(int(lib.vmmt_ls_ws_floats(M, V, H)), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    calls = {
        "colsum": lambda: lib.vmmt_ls_colsum(L.BF16, W.data_ptr(), H, bias.data_ptr(), V, H, PAD, wbar.data_ptr(), bbar.data_ptr(), scratch.data_ptr(), st),
        "rows": lambda: lib.vmmt_ls_rows(L.BF16, O.data_ptr(), H, W.data_ptr(), H, y.data_ptr(), None, M, V, H, PAD, eps, 1.0 / B, lse.data_ptr(),
                                         nll.data_ptr(), wbar.data_ptr(), bbar.data_ptr(), dO.data_ptr(), H, obar.data_ptr(), sums.data_ptr(),
                                         scratch.data_ptr(), st),
        "rows_loss_only": lambda: lib.vmmt_ls_rows(L.BF16, O.data_ptr(), H, None, 0, y.data_ptr(), None, M, V, H, PAD, eps, 0.0, lse.data_ptr(),
                                                   nll.data_ptr(), wbar.data_ptr(), bbar.data_ptr(), None, 0, None, sums.data_ptr(), scratch.data_ptr(), st),
        "dW": lambda: lib.vmmt_ls_dW(L.BF16, O.data_ptr(), H, y.data_ptr(), None, M, V, H, PAD, eps, 1.0 / B, obar.data_ptr(), sums.data_ptr(),
                                     dW.data_ptr(), H, db.data_ptr(), st),
    }
    out = {}
    for name, fn in calls.items():
        us = []
        for _ in range(reps + 1):                   # (the first window warms up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                L.check(fn(), name)
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / iters)
        out[name] = round(statistics.median(us[1:]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--entry-iters", type=int, default=50)
    ap.add_argument("--arm", default=None, help="(child) the label_smoothing value to time in this process, or `entries`")
    a = ap.parse_args()
    if a.arm is not None:
        if not torch.cuda.is_available():
            raise SystemExit("time_label_smoothing.py: no GPU; nothing is measured without one")
        print(json.dumps(entries(a.entry_iters, a.reps) if a.arm == "entries" else step_arm(float(a.arm), a.steps, a.warmup)), flush=True)
        return

    def child(arm):                 # (a child that fails ends the run: nothing more is started on the device behind it)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--steps", str(a.steps), "--warmup", str(a.warmup), "--reps",
                              str(a.reps), "--entry-iters", str(a.entry_iters)], capture_output=True, text=True, timeout=300, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])
    arms = ("0", "0.1")
    got = {k: [] for k in arms}
    for _ in range(a.reps):
        for k in arms:
            got[k].append(round(child(k)["ms"], 4))
    print(json.dumps(dict(config=2, steps=a.steps, reps=a.reps, ms_per_step={k: statistics.median(v) for k, v in got.items()}, ms_per_step_all=got)), flush=True)
    print(json.dumps(dict(entries_us=child("entries"), iters=a.entry_iters)), flush=True)


if __name__ == "__main__":
    main()
