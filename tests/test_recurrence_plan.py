"""CPU: the step descriptors engine/recurrence.py builds, checked against the kernels' contract (csrc/lstm.hip, csrc/gru.hip; vmmt.h) at the
smallest shape where every rule shows: 3 steps (first, middle, last), 2 directions, 2 rows per step, width 32, both cells.  Buffers are
layout.Buf on the CPU device; nothing is launched."""
import ctypes as C

import pytest
import torch

from variational_mmt_amd import _lib as L
from variational_mmt_amd.engine import recurrence as R
from variational_mmt_amd.engine.layout import Buf

T, F32 = torch.bfloat16, torch.float32
CELLS = ("LSTM", "GRU")


def _site(kind, steps=3, dirs=2, rows=2, W=32, given=False, capture=False, gx2=False, inject=False, dh0=False, same_dg=None):
    """a site on fresh buffers (every role its own buffer, so that a pointer names its role) + the buffers by role"""
    G = 4 if kind == "LSTM" else 3
    nb = lambda r, c, dt=T: Buf(r, c, dt, "cpu")
    b = dict(out=nb(steps * rows, 64 + dirs * W), saved=nb(steps * rows, dirs * 4 * W), c=nb(steps * rows, dirs * W, F32),
             gx=nb(steps * rows, dirs * G * W, F32), gx2=nb(rows, G * W, F32), zero=nb(rows, dirs * W), h0=nb(rows, 32 + dirs * W),
             c0=nb(rows, dirs * W, F32), hn=nb(rows, dirs * W), cn=nb(rows, dirs * W, F32), w_hh=[nb(G * W, W) for _ in range(dirs)],
             w_hh_t=[nb(W, G * W) for _ in range(dirs)], b_hn=[nb(1, W, F32) for _ in range(dirs)], dh_above=nb(steps * rows, dirs * W),
             dgx=nb(steps * rows, dirs * G * W), dgh=nb(steps * rows, dirs * G * W), carry=nb(rows, dirs * W, F32),
             dh_n=nb(rows, dirs * W, F32), dc_n=nb(rows, dirs * W, F32), dh0=nb(rows, dirs * W, F32))
    if same_dg if same_dg is not None else kind == "LSTM":
        b["dgh"] = b["dgx"]
    init = dict(h0=b["h0"], h0col=32, c0=b["c0"]) if given else dict(zero=b["zero"])
    s = R.Site(steps, dirs, rows, W, G, b["out"], b["saved"], ocol=64, c=b["c"], lens=None, gx=b["gx"], gx2=b["gx2"] if gx2 else None,
               w_hh=b["w_hh"], b_hn=b["b_hn"], hn=b["hn"] if capture else None, cn=b["cn"] if capture else None,
               dh_above=b["dh_above"], dgx=b["dgx"], dgh=b["dgh"], carry=b["carry"], w_hh_t=b["w_hh_t"],
               dh_n=b["dh_n"] if inject else None, dc_n=b["dc_n"] if inject else None, dh0=b["dh0"] if dh0 else None, **init)
    return s, b


@pytest.mark.parametrize("given", (False, True))
@pytest.mark.parametrize("kind", CELLS)
def test_forward_descriptors(kind, given):
    lstm, G, W, R_ = kind == "LSTM", (4 if kind == "LSTM" else 3), 32, 2
    s, b = _site(kind, given=given, capture=not given, gx2=given)
    arr = R.forward_array(R.CELLS[kind], s)
    assert len(arr) == 6 and isinstance(arr[0], L.LstmDirFwd if lstm else L.GruDirFwd)
    for k in range(2):
        seq = [arr[step * 2 + k] for step in range(3)]
        assert [a.t for a in seq] == ([0, 1, 2] if k == 0 else [2, 1, 0])          # direction 1 walks time downwards
        for i, a in enumerate(seq):
            assert (a.h_out, a.ld_h) == (b["out"].p(a.t * R_, 64 + k * W), b["out"].ld)
            assert (a.w_hh, a.ld_w) == (b["w_hh"][k].p(), b["w_hh"][k].ld)
            assert (a.gx, a.ld_gx) == (b["gx"].p(a.t * R_, k * G * W), b["gx"].ld)
            assert (a.gx2, a.ld_gx2) == ((b["gx2"].p(), b["gx2"].ld) if given else (None, 0))      # set only when given
            saved = (a.gates, a.ld_gates) if lstm else (a.saved, a.ld_saved)
            assert saved == (b["saved"].p(a.t * R_, k * 4 * W), b["saved"].ld)       # four blocks per direction, the three-gate GRU too
            if lstm:
                assert (a.c_out, a.ld_c) == (b["c"].p(a.t * R_, k * W), b["c"].ld)
            else:
                assert a.b_hn == b["b_hn"][k].p()
            if i > 0:                                   # the predecessor's outputs
                assert (a.h_prev, a.ld_hprev) == (seq[i - 1].h_out, seq[i - 1].ld_h)
                if lstm:
                    assert (a.c_prev, a.ld_cprev) == (seq[i - 1].c_out, seq[i - 1].ld_c)
            elif given:
                assert (a.h_prev, a.ld_hprev) == (b["h0"].p(0, 32 + k * W), b["h0"].ld)
                if lstm:
                    assert (a.c_prev, a.ld_cprev) == (b["c0"].p(0, k * W), b["c0"].ld)
            else:                                       # the zero buffer, no cell state
                assert (a.h_prev, a.ld_hprev) == (b["zero"].p(0, k * W), b["zero"].ld)
                if lstm:
                    assert a.c_prev is None
            if not given:                               # (this case captures the final state)
                assert a.capture == (1 if k == 0 else 2) and (a.h_n, a.ld_hn) == (b["hn"].p(0, k * W), b["hn"].ld)
                if lstm:
                    assert (a.c_n, a.ld_cn) == (b["cn"].p(0, k * W), b["cn"].ld)
            else:
                assert a.capture == 0 and a.h_n is None and (not lstm or a.c_n is None)


def test_forward_time_label_of_a_decoding_step():
    for kind in CELLS:
        s, _ = _site(kind, steps=1, dirs=1, given=True)
        assert [a.t for a in R.forward_array(R.CELLS[kind], s, t0=7)] == [7]


@pytest.mark.parametrize("given", (False, True))
@pytest.mark.parametrize("kind", CELLS)
def test_backward_descriptors(kind, given):
    lstm, G, W, R_ = kind == "LSTM", (4 if kind == "LSTM" else 3), 32, 2
    s, b = _site(kind, given=given, inject=not given)
    arr = R.backward_array(R.CELLS[kind], s)
    assert len(arr) == 6 and isinstance(arr[0], L.LstmDirBwd if lstm else L.GruDirBwd)
    for k in range(2):
        seq = [arr[step * 2 + k] for step in range(3)]
        assert [a.t for a in seq] == ([2, 1, 0] if k == 0 else [0, 1, 2])          # the reverse of the forward order
        for i, a in enumerate(seq):
            nxt = a.dgates_next if lstm else a.dgh_next
            if i == 0:
                assert nxt is None
            elif lstm:
                assert (nxt, a.ld_dgn) == (seq[i - 1].dgates_out, seq[i - 1].ld_dgo)
            else:                                       # the recurrent-side matrix [dr, dz, dn r], not the input-side one
                assert (nxt, a.ld_dgn) == (seq[i - 1].dgh_out, seq[i - 1].ld_dgh) and nxt != seq[i - 1].dgx_out
            assert (a.w_hh_t, a.ld_wt) == (b["w_hh_t"][k].p(), b["w_hh_t"][k].ld)
            assert (a.dh_above, a.ld_dha) == (b["dh_above"].p(a.t * R_, k * W), b["dh_above"].ld)
            saved = (a.gates, a.ld_gates) if lstm else (a.saved, a.ld_saved)
            assert saved == (b["saved"].p(a.t * R_, k * 4 * W), b["saved"].ld)
            carry = (a.dc_carry, a.ld_dcc) if lstm else (a.dh_carry, a.ld_dhc)
            assert carry == (b["carry"].p(0, k * W), b["carry"].ld)
            if lstm:
                assert (a.dgates_out, a.ld_dgo) == (b["dgx"].p(a.t * R_, k * G * W), b["dgx"].ld)
                assert (a.c_t, a.ld_ct) == (b["c"].p(a.t * R_, k * W), b["c"].ld)
            else:
                assert (a.dgx_out, a.ld_dgx) == (b["dgx"].p(a.t * R_, k * G * W), b["dgx"].ld)
                assert (a.dgh_out, a.ld_dgh) == (b["dgh"].p(a.t * R_, k * G * W), b["dgh"].ld)
            # the state that ENTERED step t in the forward: the predecessor's, outside the sequence the given one or none (zero)
            tp = a.t - 1 if k == 0 else a.t + 1
            prev = (a.c_prev, a.ld_cp) if lstm else (a.h_prev, a.ld_hp)
            if 0 <= tp < 3:
                assert prev == ((b["c"].p(tp * R_, k * W), b["c"].ld) if lstm else (b["out"].p(tp * R_, 64 + k * W), b["out"].ld))
            elif given:
                assert prev == ((b["c0"].p(0, k * W), b["c0"].ld) if lstm else (b["h0"].p(0, 32 + k * W), b["h0"].ld))
            else:
                assert prev[0] is None
            if given:                                   # (this case injects nothing)
                assert a.inject == 0 and a.dh_n is None and (not lstm or a.dc_n is None)
            else:                                       # inject codes mirror the capture codes
                assert a.inject == (1 if k == 0 else 2) and (a.dh_n, a.ld_dhn) == (b["dh_n"].p(0, k * W), b["dh_n"].ld)
                if lstm:
                    assert (a.dc_n, a.ld_dcn) == (b["dc_n"].p(0, k * W), b["dc_n"].ld)
            assert a.dh0_out is None


def test_lstm_gate_gradients_are_one_buffer():
    s, _ = _site("LSTM", same_dg=False)
    with pytest.raises(AssertionError):
        R.backward_array(R.LSTM, s)


@pytest.mark.parametrize("kind", CELLS)
def test_trailing_dh0_descriptor(kind):
    lstm = kind == "LSTM"
    s, b = _site(kind, dirs=1, given=True, dh0=True)
    arr = R.backward_array(R.CELLS[kind], s)
    assert len(arr) == 3 + 1
    a, first = arr[3], arr[2]                           # mode 1: dh0 = (gate gradients of the forward's first step) W_hh
    assert first.t == 0
    if lstm:
        assert (a.dgates_next, a.ld_dgn) == (first.dgates_out, first.ld_dgo) and a.dc_carry is None
    else:                                               # ... + the direct path left in the carry
        assert (a.dgh_next, a.ld_dgn) == (first.dgh_out, first.ld_dgh)
        assert (a.dh_carry, a.ld_dhc) == (b["carry"].p(), b["carry"].ld)
    assert (a.w_hh_t, a.ld_wt) == (b["w_hh_t"][0].p(), b["w_hh_t"][0].ld)
    assert (a.dh0_out, a.ld_dh0) == (b["dh0"].p(), b["dh0"].ld)
    assert all(x.dh0_out is None for x in arr[:3])


# the batch-walking pointers of each descriptor: pointer -> (its leading dimension, bytes per element: 4 = f32, None = the storage type);
# FIXED: per-direction parameters, the same for every sentence (the structs of csrc/lstm.hip / csrc/gru.hip say which is which)
WALK = {
    L.LstmDirFwd: dict(h_prev=("ld_hprev", None), c_prev=("ld_cprev", 4), gx=("ld_gx", 4), gx2=("ld_gx2", 4), gates=("ld_gates", None),
                       c_out=("ld_c", 4), h_out=("ld_h", None), h_n=("ld_hn", None), c_n=("ld_cn", 4)),
    L.LstmDirBwd: dict(dgates_next=("ld_dgn", None), dh_above=("ld_dha", None), gates=("ld_gates", None), c_t=("ld_ct", 4), c_prev=("ld_cp", 4),
                       dc_carry=("ld_dcc", 4), dgates_out=("ld_dgo", None), dh_n=("ld_dhn", 4), dc_n=("ld_dcn", 4), dh0_out=("ld_dh0", 4)),
    L.GruDirFwd: dict(h_prev=("ld_hprev", None), gx=("ld_gx", 4), gx2=("ld_gx2", 4), saved=("ld_saved", None), h_out=("ld_h", None),
                      h_n=("ld_hn", None)),
    L.GruDirBwd: dict(dgh_next=("ld_dgn", None), dh_above=("ld_dha", None), saved=("ld_saved", None), h_prev=("ld_hp", None),
                      dh_carry=("ld_dhc", 4), dgx_out=("ld_dgx", None), dgh_out=("ld_dgh", None), dh_n=("ld_dhn", 4), dh0_out=("ld_dh0", 4)),
}
FIXED = ("w_hh", "w_hh_t", "b_hn")


@pytest.mark.parametrize("bwd", (False, True))
@pytest.mark.parametrize("kind", CELLS)
def test_row_chunks_at_width_1024(kind, bwd):
    cell = R.CELLS[kind]
    s, _ = _site(kind, steps=2, dirs=1, rows=144, W=1024, given=True, capture=True, gx2=True, inject=True, dh0=True)
    arr = R.backward_array(cell, s) if bwd else R.forward_array(cell, s)
    walk = WALK[type(arr[0])]
    ptrs = [n for n, t in type(arr[0])._fields_ if t is C.c_void_p]
    assert sorted(ptrs) == sorted(list(walk) + [n for n in FIXED if n in ptrs])       # every pointer is classified
    chunks = R.row_chunks(arr, cell.WALK_B if bwd else cell.WALK_F, 2, 1, 144, 1024)
    # 1024 / 32 = 32 unit slices: 256 / 32 = 8 row groups of 16 sentences per launch
    assert [(r0, rows) for _, r0, rows in chunks] == [(0, 128), (128, 16)]
    seen = set()
    for sub, r0, _rows in chunks:
        assert len(sub) == len(arr) and sub is not arr
        for a, o in zip(sub, arr):
            for n in ptrs:
                p, q = getattr(a, n), getattr(o, n)
                if q is None:
                    assert p is None
                elif n in FIXED:
                    assert p == q
                else:
                    ld, esz = walk[n]
                    assert getattr(a, ld) == getattr(o, ld) and p == q + r0 * getattr(o, ld) * (esz or 2)
                    seen.add(n)
            assert (a.t, a.inject if bwd else a.capture) == (o.t, o.inject if bwd else o.capture)
    assert seen == set(walk)                            # the site set every walking pointer somewhere
    assert R.row_chunks(arr, cell.WALK_F, 2, 1, 16, 64)[0][0] is arr               # a batch that fits: the array itself
    assert R.row_chunks(arr, cell.WALK_F, 2, 1, 144, 96) is None                   # a width the persistent kernel does not take
