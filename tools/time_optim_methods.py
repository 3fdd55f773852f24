"""A/B of `-optim sgd | adagrad | adadelta` at BASELINE config 2 (bench.py's shape and batches): the fused HIP update
(csrc/optim_methods.hip on Adam's schedule) against `Optim.torch_dense = True` (torch.optim on the arena views), with `-optim adam` beside
them.  The model comes from make_vi_model_mmt and the update goes through onmt.Optim.step(); forward / backward are the engine's, held back
as in TrainerMultimodal._train_loop.  ONE model per process: a second model built in the same process runs 0.3-0.4 ms per step slower or
faster than the first whatever its method (LABNOTES, "-optim sgd|adagrad|adadelta"), so every arm is a fresh child process, and the arms
take turns: `--reps` rounds over (method, arm), each child timing `--steps` steps behind `--warmup` (host clock around a device
synchronise).  Prints one JSON line per method: median ms / step of each arm over the rounds and the HIP update's launch count.

    python tools/time_optim_methods.py [--steps 20] [--reps 3] [--warmup 10]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import variational_mmt_amd  # noqa: E402

LR = {"adam": 0.002, "sgd": 1.0, "adagrad": 0.1, "adadelta": 1.0}


class _Vocab(object):
    def __init__(self, n, tgt):
        sp = ["<unk>", "<blank>"] + (["<s>", "</s>"] if tgt else [])
        self.itos = sp + ["w%d" % i for i in range(n - len(sp))]
        self.stoi = {w: i for i, w in enumerate(self.itos)}

    def __len__(self):
        return len(self.itos)


def arm(onmt, cf, method, torch_dense, dev):
    """(step function, engine) of one model + Optim at config 2"""
    opt = argparse.Namespace(model_type="text", multimodal_model_type="vi-model1", use_posterior_image_features=False,
                             use_global_image_features=True, path_to_train_img_feats="resnet50.hdf5", rnn_type="LSTM", global_attention="general",
                             copy_attn=False, coverage_attn=False, context_gate=None, share_embeddings=False, share_decoder_embeddings=False,
                             word_dropout=0.0, enc_layers=cf["layers"], dec_layers=cf["layers"], src_word_vec_size=cf["emb"],
                             tgt_word_vec_size=cf["emb"], brnn=cf["brnn"], encoder_type="brnn" if cf["brnn"] else "rnn", rnn_size=cf["hid"],
                             z_latent_dim=cf["z"], dropout=0.0, param_init=0.1, conditional=False, image_loss="logprob", compute_dtype="bf16",
                             gpuid=[0], seed=-1, early_stopping_criteria="perplexity", evaluate_every_n_model_updates=500, save_model="unused")
    fields = {"src": types.SimpleNamespace(vocab=_Vocab(cf["vs"], False)), "tgt": types.SimpleNamespace(vocab=_Vocab(cf["vt"], True))}
    model = onmt.ModelConstructor.make_vi_model_mmt(opt, fields, True, None)
    eng = model.engine
    n_img = cf["n_img"]
    eng.set_image_table(torch.rand(n_img, eng.d.img, generator=torch.Generator().manual_seed(11)))
    B = 256
    batches = bench.make_batches(eng.d, B, cf["S"], cf["T"], n_img, 8, dev, 1234, ragged=False)
    optim = onmt.Optim(method, LR[method], 5.0)
    optim.torch_dense = torch_dense
    optim.set_parameters(model.parameters())
    eng.hold_back = True

    def step(i):
        src, sl, tgt, idx, tlen, n_tok = batches[i % len(batches)]
        ws = eng.forward(src, sl, tgt, idx, training=True, n_tgt_tokens=n_tok)
        eng.loss_backward(ws, normalization=B, batch_global=B)
        optim.step()
    return step, eng


def window(step, eng, first, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(first, first + n):
        step(i)
    eng.wait_background()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--methods", default="adam,sgd,adagrad,adadelta")
    ap.add_argument("--arm", default=None, help="(child) METHOD:hip or METHOD:torch_dense -- time this one arm in this process")
    a = ap.parse_args()
    if a.arm is not None:
        if not torch.cuda.is_available():
            raise SystemExit("time_optim_methods.py: no GPU; nothing is measured without one")
        method, kind = a.arm.split(":")
        step, eng = arm(variational_mmt_amd.install_as_onmt(), bench.CONFIGS["2"], method, kind == "torch_dense", torch.device("cuda"))
        window(step, eng, 0, a.warmup)
        ms = window(step, eng, a.warmup, a.steps)
        eng.check_async_errors()
        print(json.dumps(dict(ms=ms, update_launches=eng._adam_launches if kind == "hip" else None, rows_active=eng.rows_active())), flush=True)
        return
    methods = a.methods.split(",")
    arms = [(m, k) for m in methods for k in (("hip",) if m == "adam" else ("hip", "torch_dense"))]
    got = {mk: [] for mk in arms}
    for r in range(a.reps):
        for m, k in arms:           # (a child that fails ends the run: nothing more is started on the device behind it)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", "%s:%s" % (m, k), "--steps", str(a.steps), "--warmup",
                                  str(a.warmup)], capture_output=True, text=True, timeout=300, check=True).stdout
            got[(m, k)].append(json.loads(out.strip().splitlines()[-1]))
    for m in methods:
        mine = {k: [round(x["ms"], 4) for x in got[(mm, k)]] for mm, k in arms if mm == m}
        print(json.dumps(dict(method=method_lr(m), steps=a.steps, reps=a.reps, update_launches=got[(m, "hip")][0]["update_launches"],
                              rows_active=got[(m, "hip")][0]["rows_active"], ms_per_step={k: round(statistics.median(v), 4) for k, v in mine.items()},
                              ms_per_step_all=mine)), flush=True)


def method_lr(m):
    return "%s (lr %g)" % (m, LR[m])


if __name__ == "__main__":
    main()
