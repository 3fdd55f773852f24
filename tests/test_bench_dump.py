"""`bench.py --dump-outputs DIR` (CPU: an engine stand-in holding CPU tensors): one float32 / float64 .npy per array -- the step's
statistics, the per-token NLL, every gradient, every parameter -- a tensor above the cap as a sample whose indices depend on the seed alone, the same
files from the same state, and a plain run's options (`--full`, `--dump-outputs`) in the parser's help."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


class _Engine:
    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.params = {"b.big": torch.randn(700, 300, generator=g),            # 210 000 elements: above the cap
                       "a.edge": torch.randn(bench.DUMP_SAMPLE, generator=g),  # exactly the cap: written whole
                       "c.small": torch.randn(3, 5, generator=g)}
        self.grads = {n: torch.randn(v.shape, generator=g) for n, v in self.params.items() if n != "c.small"}    # (one without gradient)

    def state_dict(self):
        return {n: v.clone() for n, v in self.params.items()}

    def read_stats(self, ws, batch_global=None):
        return dict(nmt=1.5, td_kl_before=0.25, td_kl_after=0.25, td_kl_multiplier=1.0, img_feats_loss=-2.0, img_feats_cos=0.5, elbo=3.75,
                    n_words=40, n_correct=7)


def _ws():
    return types.SimpleNamespace(Tp=4, B=3, tok_nll=torch.arange(12, dtype=torch.float32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_array_once(tmp_path):
    e = _Engine(0)
    total = bench.dump_outputs(str(tmp_path / "a"), e, _ws(), 3)
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == ["grad.a.edge", "grad.b.big", "param.a.edge", "param.b.big", "param.c.small", "stats", "tok_nll"]
    assert total == sum(x.nbytes for x in got.values()) <= 64 * 2 ** 20
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert got["stats"].tolist() == [1.5, 0.25, 0.25, -2.0, 0.5, 3.75, 40.0, 7.0] and len(bench.STAT_KEYS) == 8
    assert got["tok_nll"].shape == (4, 3) and got["tok_nll"][1, 0] == 3.0
    assert np.array_equal(got["param.c.small"], e.params["c.small"].numpy())
    assert np.array_equal(got["param.a.edge"], e.params["a.edge"].numpy())
    idx = bench.sample_indices({n: v.numel() for n, v in e.params.items()})
    assert list(idx) == ["b.big"] and idx["b.big"].shape == (bench.DUMP_SAMPLE,)
    assert int(idx["b.big"].min()) >= 0 and int(idx["b.big"].max()) < 210000
    assert np.array_equal(got["param.b.big"], e.params["b.big"].reshape(-1)[idx["b.big"]].numpy())
    assert np.array_equal(got["grad.b.big"], e.grads["b.big"].reshape(-1)[idx["b.big"]].numpy())            # the same elements as the parameter's
    assert np.array_equal(got["grad.a.edge"], e.grads["a.edge"].numpy())


def test_dump_is_the_same_for_the_same_state_and_follows_the_values(tmp_path):
    bench.dump_outputs(str(tmp_path / "a"), _Engine(0), _ws(), 3)
    bench.dump_outputs(str(tmp_path / "b"), _Engine(0), _ws(), 3)
    bench.dump_outputs(str(tmp_path / "c"), _Engine(1), _ws(), 3)
    a, b, c = (_load(str(tmp_path / x)) for x in "abc")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["param.b.big"].shape == c["param.b.big"].shape and not np.array_equal(a["param.b.big"], c["param.b.big"])


def test_sample_does_not_depend_on_the_order_of_the_names():
    x = bench.sample_indices({"p": 10 ** 6, "q": 2 * 10 ** 6, "r": 5})
    y = bench.sample_indices({"q": 2 * 10 ** 6, "r": 5, "p": 10 ** 6})
    assert sorted(x) == ["p", "q"] and all(torch.equal(x[k], y[k]) for k in x)


def test_options_are_there():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
