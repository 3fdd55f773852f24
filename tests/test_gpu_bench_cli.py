"""`bench.py` from the command line on the GPU: a plain run prints the headline line without the blocks that moved behind `--full`, `--full`
still prints them, `--steps` sets the timed steps, and `--dump-outputs` writes the same arrays in every run.

The bound on two dumps: the inputs are seeded to the bit and the dumped step starts from the seeded state, so what is left between two runs is
the order of the float atomics inside one step -- f32 rounding, which can move a bf16 activation across ONE rounding step (2^-8 relative).
Every array of a second run must therefore lie within 2^-8 of the first one's largest value; the state a training loop is left in behind a
few updates does not (profiles/dump_outputs_run_to_run.txt)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BF16_STEP = 2.0 ** -8


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"] + list(args),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines                      # ONE line on stdout
    return json.loads(lines[0]), r.stderr


def _load(d):
    return {f[:-4]: np.load(os.path.join(str(d), f)) for f in sorted(os.listdir(str(d)))}


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        d, top = float(np.abs(a[k].astype(np.float64) - b[k]).max()), float(np.abs(a[k]).max())
        print("%-70s max|a| %.3e  max|a-b| %.3e" % (k, top, d))
        assert d <= BF16_STEP * top, (k, d, top)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return d, _bench("--dump-outputs", str(d / "a")), _bench("--dump-outputs", str(d / "b"))


def test_plain_run_prints_the_headline_only_and_dumps_the_same_arrays_twice(plain):
    d, (line, err), (line_b, _) = plain
    assert line["metric"] == line["unit"] == "triplets/sec" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == 3 and len(line["step_ms"]["list"]) == 3                    # --steps IS the number of timed steps
    assert abs(line["value"] - 256 * 1e3 / line["ms_per_step"]) <= 2e-3 * line["value"]  # value and ms_per_step say the same
    assert not {"roofline", "parity", "cpu_baseline"} & set(line) and line["stream_overlap"] is None and len(line["repeats_ms"]) == 1
    assert "only shape a --full run" not in err
    a, b = _load(d / "a"), _load(d / "b")
    assert {"stats", "tok_nll", "param.generator.0.weight", "grad.generator.0.weight"} <= set(a)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert line["outputs_dumped"]["bytes"] == sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    assert a["tok_nll"].shape == (20, 256) and np.isfinite(a["stats"]).all() and a["stats"][6] == 20 * 256      # n_words of the step
    assert all(np.abs(a[k]).max() > 0 for k in a if k.startswith("grad."))             # a backward pass has run behind the restore
    _same(a, b)


def test_full_run_still_prints_what_moved_and_dumps_what_a_plain_run_dumps(plain, tmp_path):
    d = plain[0]
    line, err = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "f"))
    assert {"roofline", "parity"} <= set(line) and "cpu_baseline" not in line and "error" not in line["parity"]
    assert line["roofline"]["achieved"] > 0 and line["stream_overlap"]["ratio"] > 0 and len(line["repeats_ms"]) == 3
    assert line["steps"] == 3 and len(line["step_ms"]["list"]) == 3
    _same(_load(d / "a"), _load(tmp_path / "f"))


def test_a_full_run_s_switch_on_a_plain_run_is_answered_on_stderr():
    line, err = _bench("--repeats", "2")
    assert len(line["repeats_ms"]) == 1 and "only shape a --full run" in err
