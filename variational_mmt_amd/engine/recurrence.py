"""The step descriptors of every recurrence (LSTM and GRU), built in ONE place, and the plan entries that run them.

A caller describes a `Site` -- one recurrence of one layer: its buffers, sizes and initial state -- and a cell kind (LSTM / GRU) turns
it into the descriptor array the step kernels read (csrc/lstm.hip, csrc/gru.hip; include/vmmt.h).  What makes a recurrence correct is
written here once: the time order of each direction, which step is whose predecessor, what the first step reads, the capture / inject
codes of the final state, how a backward step finds the gate gradients of the step processed before it, and the trailing mode-1 step
that turns the first step's gate gradients into the gradient of the initial state.  A cell adds only the fields its own kernels have.

Imports without a GPU: descriptors are ctypes structures, buffers are anything with `.p(row, col)` and `.ld` (layout.Buf)."""
import ctypes as C

from .. import _lib as L


class Site(object):
    """One recurrence of one layer.  Buffers are [steps * rows][...] with step t at row t * rows; direction k owns columns k * width
    of the states and k * gates * width of the gate pre-activations / gradients -- but k * 4 * width of the SAVED gates, whose buffer is
    laid out for four blocks per direction whatever the cell (the GRU saves r, z, n and hn).

    forward and backward: steps, dirs, rows (B; encoder_tgt: Tn), width (per direction, as computed), gates (G), out / ocol (the
      outputs h_t and their first column: the decoder's top layer writes into `cat` at Hp), saved, c (f32 cell states, LSTM), lens,
      and the initial state -- `zero` (a buffer of zeros: the state is zero) or `h0` / `h0col` / `c0` (given; `c0` LSTM only)
    forward: gx, gx2 (per-sentence addend or None), w_hh / b_hn (one per direction; b_hn GRU only), hn / cn (final-state capture or None)
    backward: dh_above, dgx / dgh (input-side / recurrent-side gate gradients: ONE buffer for the LSTM), carry (f32), w_hh_t (one per
      direction), dh_n / dc_n (injected gradients of the final state or None), dh0 (or None: the gradient of the initial hidden state,
      written by one more step in mode 1)"""

    def __init__(self, steps, dirs, rows, width, gates, out, saved, ocol=0, c=None, lens=None, zero=None, h0=None, h0col=0, c0=None,
                 gx=None, gx2=None, w_hh=(), b_hn=(), hn=None, cn=None,
                 dh_above=None, dgx=None, dgh=None, carry=None, w_hh_t=(), dh_n=None, dc_n=None, dh0=None):
        assert (zero is None) != (h0 is None), "the initial state is the zero buffer or given"
        self.steps, self.dirs, self.rows, self.width, self.gates = steps, dirs, rows, width, gates
        self.out, self.ocol, self.saved, self.c, self.lens = out, ocol, saved, c, lens
        self.zero, self.h0, self.h0col, self.c0 = zero, h0, h0col, c0
        self.gx, self.gx2, self.w_hh, self.b_hn, self.hn, self.cn = gx, gx2, w_hh, b_hn, hn, cn
        self.dh_above, self.dgx, self.dgh, self.carry, self.w_hh_t = dh_above, dgx, dgh, carry, w_hh_t
        self.dh_n, self.dc_n, self.dh0 = dh_n, dc_n, dh0


def _time(s, fstep, k):
    """(t, tp): the time index the `fstep`-th FORWARD step of direction k computes and that of its predecessor (outside [0, steps): the
    initial state).  Direction 1 walks time downwards.  The backward visits the forward steps last to first."""
    return (fstep, fstep - 1) if k == 0 else (s.steps - 1 - fstep, s.steps - fstep)


def _final_code(buf, k):
    """capture (forward) / inject (backward) code of the final state: 1 = where t == len - 1 (direction 0), 2 = where t == 0"""
    return 0 if buf is None else (1 if k == 0 else 2)


class _Lstm(object):
    name, persistent = "lstm", True              # persistent: csrc/lstm_seq.hip runs a whole recurrence in one launch
    Fwd, Bwd = L.LstmDirFwd, L.LstmDirBwd
    # pointer fields that walk the batch: (pointer, leading dimension, element size; None = the storage type T)
    WALK_F = (("h_prev", "ld_hprev", None), ("c_prev", "ld_cprev", 4), ("gx", "ld_gx", 4), ("gx2", "ld_gx2", 4), ("gates", "ld_gates", None),
              ("c_out", "ld_c", 4), ("h_out", "ld_h", None), ("h_n", "ld_hn", None), ("c_n", "ld_cn", 4))
    WALK_B = (("dgates_next", "ld_dgn", None), ("dh_above", "ld_dha", None), ("gates", "ld_gates", None), ("c_t", "ld_ct", 4), ("c_prev", "ld_cp", 4),
              ("dc_carry", "ld_dcc", 4), ("dgates_out", "ld_dgo", None), ("dh_n", "ld_dhn", 4), ("dc_n", "ld_dcn", 4), ("dh0_out", "ld_dh0", 4))
    NEXT = "dgates_next"

    @staticmethod
    def fwd(a, s, t, tp, k, first):
        R, W = s.rows, s.width
        if first:
            a.c_prev, a.ld_cprev = (None, s.c.ld) if s.c0 is None else (s.c0.p(0, k * W), s.c0.ld)
        else:
            a.c_prev, a.ld_cprev = s.c.p(tp * R, k * W), s.c.ld
        a.gates, a.ld_gates = s.saved.p(t * R, k * 4 * W), s.saved.ld
        a.c_out, a.ld_c = s.c.p(t * R, k * W), s.c.ld
        if s.cn is not None:
            a.c_n, a.ld_cn = s.cn.p(0, k * W), s.cn.ld

    @staticmethod
    def bwd(a, s, t, tp, k):
        R, W = s.rows, s.width
        assert s.dgh is s.dgx                      # one gate-gradient matrix serves dW_ih and the next step's recurrent product
        a.gates, a.ld_gates = s.saved.p(t * R, k * 4 * W), s.saved.ld
        a.c_t, a.ld_ct = s.c.p(t * R, k * W), s.c.ld
        if 0 <= tp < s.steps:
            a.c_prev, a.ld_cp = s.c.p(tp * R, k * W), s.c.ld
        elif s.c0 is not None:
            a.c_prev, a.ld_cp = s.c0.p(0, k * W), s.c0.ld
        a.dc_carry, a.ld_dcc = s.carry.p(0, k * W), s.carry.ld
        a.dgates_out, a.ld_dgo = s.dgx.p(t * R, k * s.gates * W), s.dgx.ld
        if s.dc_n is not None:
            a.dc_n, a.ld_dcn = s.dc_n.p(0, k * W), s.dc_n.ld

    @staticmethod
    def bwd_dh0(a, s, k):
        pass


class _Gru(object):
    name, persistent = "gru", False              # one launch per step (csrc/gru.hip)
    Fwd, Bwd = L.GruDirFwd, L.GruDirBwd
    WALK_F = (("h_prev", "ld_hprev", None), ("gx", "ld_gx", 4), ("gx2", "ld_gx2", 4), ("saved", "ld_saved", None), ("h_out", "ld_h", None),
              ("h_n", "ld_hn", None))
    WALK_B = (("dgh_next", "ld_dgn", None), ("dh_above", "ld_dha", None), ("saved", "ld_saved", None), ("h_prev", "ld_hp", None),
              ("dh_carry", "ld_dhc", 4), ("dgx_out", "ld_dgx", None), ("dgh_out", "ld_dgh", None), ("dh_n", "ld_dhn", 4), ("dh0_out", "ld_dh0", 4))
    NEXT = "dgh_next"

    @staticmethod
    def fwd(a, s, t, tp, k, first):              # no cell state: the state is the output row; b_hn sits inside r * (.), an operand of the step
        a.b_hn = s.b_hn[k].p()
        a.saved, a.ld_saved = s.saved.p(t * s.rows, k * 4 * s.width), s.saved.ld

    @staticmethod
    def bwd(a, s, t, tp, k):
        R, W = s.rows, s.width
        a.saved, a.ld_saved = s.saved.p(t * R, k * 4 * W), s.saved.ld
        if 0 <= tp < s.steps:
            a.h_prev, a.ld_hp = s.out.p(tp * R, s.ocol + k * W), s.out.ld
        elif s.h0 is not None:
            a.h_prev, a.ld_hp = s.h0.p(0, s.h0col + k * W), s.h0.ld
        a.dh_carry, a.ld_dhc = s.carry.p(0, k * W), s.carry.ld           # the f32 direct path dh z
        a.dgx_out, a.ld_dgx = s.dgx.p(t * R, k * s.gates * W), s.dgx.ld
        a.dgh_out, a.ld_dgh = s.dgh.p(t * R, k * s.gates * W), s.dgh.ld

    @staticmethod
    def bwd_dh0(a, s, k):                        # dh0 = dgh_0 W_hh + the direct path left in the carry
        a.dh_carry, a.ld_dhc = s.carry.p(0, k * s.width), s.carry.ld


LSTM, GRU = _Lstm, _Gru
CELLS = {"LSTM": LSTM, "GRU": GRU}               # by Dims.rnn


def forward_array(cell, s, t0=0):
    """the forward descriptors of site `s`, step-major then direction; `t0`: the time index of the site's first row (a decoding step)"""
    R, W, nd = s.rows, s.width, s.dirs
    arr = (cell.Fwd * (s.steps * nd))()
    init = s.zero if s.zero is not None else s.h0
    for step in range(s.steps):
        for k in range(nd):
            t, tp = _time(s, step, k)
            a = arr[step * nd + k]
            if step == 0:
                a.h_prev, a.ld_hprev = init.p(0, s.h0col + k * W), init.ld
            else:
                a.h_prev, a.ld_hprev = s.out.p(tp * R, s.ocol + k * W), s.out.ld
            a.w_hh, a.ld_w = s.w_hh[k].p(), s.w_hh[k].ld
            a.gx, a.ld_gx = s.gx.p(t * R, k * s.gates * W), s.gx.ld
            if s.gx2 is not None:
                a.gx2, a.ld_gx2 = s.gx2.p(), s.gx2.ld
            a.h_out, a.ld_h = s.out.p(t * R, s.ocol + k * W), s.out.ld
            if s.hn is not None:
                a.h_n, a.ld_hn = s.hn.p(0, k * W), s.hn.ld
            a.t, a.capture = t0 + t, _final_code(s.hn, k)
            cell.fwd(a, s, t, tp, k, step == 0)
    return arr


def backward_array(cell, s):
    """the backward descriptors of site `s`: the forward steps last to first; with `s.dh0` one more step (mode 1) behind them"""
    R, W, nd, G = s.rows, s.width, s.dirs, s.gates
    arr = (cell.Bwd * ((s.steps + (s.dh0 is not None)) * nd))()
    for step in range(s.steps + (s.dh0 is not None)):
        for k in range(nd):
            a = arr[step * nd + k]
            if step > 0:                         # the step processed just before (the forward successor) left its recurrent-side gate gradients
                tn = _time(s, s.steps - step, k)[0]
                setattr(a, cell.NEXT, s.dgh.p(tn * R, k * G * W))
                a.ld_dgn = s.dgh.ld
            a.w_hh_t, a.ld_wt = s.w_hh_t[k].p(), s.w_hh_t[k].ld
            if step == s.steps:                  # mode 1: nothing but the product with W_hh
                a.dh0_out, a.ld_dh0 = s.dh0.p(0, k * W), s.dh0.ld
                cell.bwd_dh0(a, s, k)
                continue
            t, tp = _time(s, s.steps - 1 - step, k)
            a.dh_above, a.ld_dha = s.dh_above.p(t * R, k * W), s.dh_above.ld
            if s.dh_n is not None:
                a.dh_n, a.ld_dhn = s.dh_n.p(0, k * W), s.dh_n.ld
            a.t, a.inject = t, _final_code(s.dh_n, k)
            cell.bwd(a, s, t, tp, k)
    return arr


def row_chunks(arr, walk, tsz, ndir, B, H):
    """A persistent recurrence needs all of its workgroups resident at once: (B / 16 row groups) x (H / 32 unit slices) x directions
    <= 256.  Sentences are independent in a recurrence, so a batch that does not fit is cut into ROW chunks, one persistent launch
    each, one after the other (BASELINE config 5: H = 1024 -> 32 slices -> 128 sentences per launch; the per-step kernels it
    replaces re-read their W_hh slice from L2 at every step: 35 us per backward step against 8).  `walk`: the cell's WALK_F / WALK_B,
    `tsz`: bytes of the storage type.  -> [(descriptors, row offset, rows)], or None when the persistent kernel does not serve this
    size at all."""
    if H not in (64, 128, 256, 512, 1024):
        return None
    groups = 256 // ((H // 32) * ndir)
    if groups < 1:
        return None
    rows = 16 * groups
    if B <= rows:
        return [(arr, 0, B)]
    out = []
    for r0 in range(0, B, rows):
        chunk = type(arr)()
        C.memmove(chunk, arr, C.sizeof(arr))
        for a in chunk:
            for ptr, ld, esz in walk:
                p0 = getattr(a, ptr)
                if p0:
                    setattr(a, ptr, p0 + r0 * getattr(a, ld) * (esz if esz is not None else tsz))
        out.append((chunk, r0, min(rows, B - r0)))
    return out


def _emit(e, plan, cell, s, arr, bwd):
    """plan entries of a whole recurrence.  A cell with a persistent kernel (Engine.persistent_lstm): ONE launch per row chunk (W_hh
    resident in registers, in-launch hand-off of h_t: csrc/lstm_seq.hip), which falls back by itself to the per-step kernels where it
    does not apply; otherwise the per-step kernels issued from one host call (and the mode-1 step by a call of its own)."""
    lib, nd, n, B, H = e.lib, s.dirs, s.steps, s.rows, s.width
    which = "bwd" if bwd else "fwd"
    mode = ((1 if s.dh0 is not None else 0),) if bwd else ()
    if cell.persistent and e.persistent_lstm:
        import torch
        chunks = row_chunks(arr, cell.WALK_B if bwd else cell.WALK_F, e.tsz, nd, B, H) if e.dt == L.BF16 else None
        name = "vmmt_%s_seq_%s" % (cell.name, which)
        xchg_bytes = lib.vmmt_lstm_seq_xchg_bytes_bwd if bwd else lib.vmmt_lstm_seq_xchg_bytes
        for sub, r0, rows in (chunks or [(arr, 0, B)]):
            lens = (s.lens + 8 * r0) if s.lens else None
            dev = torch.frombuffer(bytearray(bytes(sub)), dtype=torch.uint8).to(e.dev)
            sync = e._seq_sync()
            xchg = torch.zeros(max(16, xchg_bytes(nd, rows, H)), dtype=torch.uint8, device=e.dev)
            plan.append((getattr(lib, name), (e.dt, nd, n, sub, dev.data_ptr(), lens, rows, H) + mode + (sync.data_ptr(), xchg.data_ptr()),
                         name, (sub, dev, sync, xchg), e._sid))
            e.seq_syncs.append(sync)
        return
    name = "vmmt_%s_chain_%s" % (cell.name, which)
    plan.append((getattr(lib, name), (e.dt, nd, n, arr, s.lens, B, H) + ((0,) if bwd else ()), name, arr, e._sid))
    if bwd and s.dh0 is not None:
        last = C.cast(C.byref(arr, n * nd * C.sizeof(cell.Bwd)), C.POINTER(cell.Bwd))
        name = "vmmt_%s_step_bwd" % cell.name
        plan.append((getattr(lib, name), (e.dt, nd, last, s.lens, B, H, 1), name, arr, e._sid))


def emit_forward(e, plan, cell, s):
    _emit(e, plan, cell, s, forward_array(cell, s), False)


def emit_backward(e, plan, cell, s):
    _emit(e, plan, cell, s, backward_array(cell, s), True)


def step_forward(lib, cell, dt, s, t, stream):
    """one time step right away (decoding): `s` is a site of one step with a given initial state, `t` its time index"""
    name = "vmmt_%s_step_fwd" % cell.name
    L.check(getattr(lib, name)(dt, s.dirs, forward_array(cell, s, t0=t), s.lens, s.rows, s.width, stream), name)
