"""psk_soft_process_device_resampled on a real MI355X: packets resampled on the GPU (psk_resample.hip) in front of the
demodulator.  Every checked stream is, bit for bit, what a fresh handle gives when it is fed the contract's CF32 packets --
tests/resample_model.py on (tests/tune_model.py on) the packet's samples -- contiguously through psk_soft_process_device, and what
the oracle gives on those packets; counts and SRI fields are those of a control-plane-only handle fed packets of n_out samples
with the scaled sample period; the history behind every call is the model's; the launch trace (PSK_SOFT_TRACE_LAUNCHES=2) says
which pre-pass kernels ran, and the source buffers come back byte for byte.

The calls go through tests.test_gpu_strided.strided_run (layout, poison, download, the source check) behind a handle proxy that
adds the tunes, the resamples and the sample periods and sizes the output rows for n_out.  P = psk_soft_resample_piece(): lengths stay around three
pieces."""
import numpy as np
import pytest

import tests.test_gpu_cs8 as t_cs8
import tests.test_gpu_strided as t_strided
from tests import resample_model as rm
from tests import tune_model as tm
from tests.test_gpu_cs16_schedules import H_CS16, assert_same, check_parity, screened, untraced_then_traced
from tests.test_gpu_strided import contiguous, gathers, strided_run
from tests.test_gpu_tune import DT, F16, NEG, _pieces, _signals, tunes_of
from tests.test_strided_control import OUT_FIELDS

pytestmark = pytest.mark.gpu

ONE = 1 << 32
S = 8
STEP_837 = int(8.37 / 8 * 2.0 ** 32)
STEPS = (1 << 31, ONE, 1 << 33, STEP_837)


@pytest.fixture(autouse=True)
def _half_packets_in_the_shared_helpers(monkeypatch):
    """the shared helpers take a packet's format from its dtype: teach them float16 (as tests/test_gpu_tune.py does)"""
    from psk_soft_amd import lib as pl

    fmt8, fmts, poison = t_cs8._fmt, t_strided._fmt, t_strided._poison
    monkeypatch.setattr(t_cs8, "_fmt", lambda x: pl.FORMAT_CF16 if x.dtype == F16 else fmt8(x))
    monkeypatch.setattr(t_strided, "_fmt", lambda p, dt: p.FORMAT_CF16 if np.dtype(dt) == F16 else fmts(p, dt))
    monkeypatch.setattr(t_strided, "_poison", lambda dt: np.uint16(0x7E55).view(np.float16) if np.dtype(dt) == F16 else poison(dt))


def _props(C, numAvg=(10, 16, 25)):
    return [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=numAvg[c % 3], phaseAvg=(5, 20, 50)[(c // 3) % 3],
                 differentialDecoding=int(c % 5 == 3)) for c in range(C)]


def _period_in(step):
    """The sample period a resampled packet comes with, chosen so that the period the demodulator sees behind the resampler,
    sri_xdelta * (step * 2^-32), is exactly the 0.01 the shared helpers and the oracle run the model's packets with (the phase
    estimator's fit does float arithmetic on the period: another period, other bits)."""
    if not step:
        return 0.01
    scale = step * 2.0 ** -32
    lo = hi = 0.01 / scale
    for _ in range(16):
        for x in (lo, hi):
            if x * scale == 0.01:
                return float(x)
        lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, 1.0)
    raise AssertionError("no sample period brings step %#x to 0.01" % step)


def _live(x):
    """a packet the call resamples or tunes: there, and at least one sample"""
    return x is not None and x.size >= 2


class Plan:
    """The arguments and the model of a sequence of calls.  data[k][c]: the packet of channel c in call k (or None); steps[c]:
    the resampler's step (0: not resampled); pos0[c]; restart[k][c]; tsteps[c]: the NCO's step (None: untuned), phase0[c];
    hist0[c]: six floats set with set_resample_history in front of the first call (None: the handle's zeros)."""

    def __init__(self, data, steps, pos0=None, restart=None, tsteps=None, phase0=None, hist0=None):
        from psk_soft_amd import lib as pl

        K, C = len(data), len(data[0])
        self.data, self.steps, self.hist0 = data, steps, hist0 or [None] * C
        tsteps = tsteps or [None] * C
        pos = list(pos0 or [0] * C)
        ph = list(phase0 or [0] * C)
        streams = [rm.Stream(steps[c] or ONE, pos[c], self.hist0[c]) for c in range(C)]
        self.rss, self.tunes, self.model, self.hist, self.n_out = [], [], [], [], []
        for k in range(K):
            rs_row, tn_row, m_row, n_row = [], [], [], []
            for c in range(C):
                x = data[k][c]
                re = bool(restart and restart[k][c])
                rs_row.append(pl.Resample(pos[c], steps[c], pl.RS_RESTART if re else 0, 0))
                tn_row.append((0, 0) if tsteps[c] is None else (ph[c], tsteps[c]))
                if not _live(x):
                    m_row.append(x)
                    n_row.append(0)
                    continue
                s = x if tsteps[c] is None else tm.apply(ph[c], tsteps[c], x)
                if tsteps[c] is not None:
                    ph[c] = pl.tune_advance(ph[c], tsteps[c], x.size // 2)
                if steps[c]:
                    assert streams[c].pos == pos[c]
                    s = streams[c].push(s, restart=re)  # (the library's helper moves pos, the model's own arithmetic checks it)
                    pos[c] = pl.resample_advance(rs_row[-1], x.size // 2)
                    assert pos[c] == streams[c].pos
                m_row.append(s)
                n_row.append(s.size // 2)
            self.rss.append(rs_row)
            self.tunes.append(tn_row)
            self.model.append(m_row)
            self.n_out.append(n_row)
            self.hist.append([streams[c].history.copy() for c in range(C)])
        self.any_tune = any(t is not None for t in tsteps)
        self.xd = [_period_in(steps[c]) for c in range(C)]


class Resampled:
    """a Handle whose process_device_strided is process_device_resampled with the plan's tunes and resamples of the k-th call
    made through it, and whose output_capacity sizes a row for the model's packet.  short: {(k, c): symbols}: rows of that capacity;
    refused: {k: status} calls expected to fail.  After every call it keeps the SRI fields and the channels' histories."""

    def __init__(self, h, plan, short=None, refused=None, no_tunes=False, histories=True):
        self._h, self._plan, self._k, self._short, self._refused = h, plan, 0, short or {}, refused or {}
        self._order = iter([(k, c) for k in range(len(plan.data)) for c in range(len(plan.data[0])) if plan.data[k][c] is not None])
        self._no_tunes, self._histories = no_tunes, histories
        self.fields, self.hist = [], []
        for c, h0 in enumerate(plan.hist0):
            if h0 is not None:
                h.set_resample_history(c, h0)

    def __getattr__(self, name):
        return getattr(self._h, name)

    def output_capacity(self, c, n):
        k, cc = next(self._order)
        assert cc == c
        x = self._plan.model[k][c]
        return self._short[k, c] if (k, c) in self._short else self._h.output_capacity(c, x.size // 2)

    def process_device_strided(self, ch0, pk, strides, outs, stream=None):
        from psk_soft_amd import lib as pl

        k = self._k
        self._k += 1
        tunes = None if self._no_tunes or not self._plan.any_tune else self._plan.tunes[k]
        for i in range(len(pk)):
            pk[i].sri_xdelta = self._plan.xd[ch0 + i]
        try:
            self._h.process_device_resampled(ch0, pk, strides, tunes, self._plan.rss[k], outs, stream)
            assert k not in self._refused, k
        except pl.PskSoftError as e:
            assert self._refused.get(k) == e.status, (k, e)
            for o in outs:
                o.n_symbols = o.n_bits = o.n_sampleIndex = 0
        self.fields.append([tuple(getattr(o, f) for f in OUT_FIELDS) for o in outs])
        if self._histories:
            self.hist.append([self._h.resample_history(c) for c in range(len(pk))])


def _planned_fields(props, plan, skip=()):
    """(ret, counts, SRI fields, warnings) per call and channel of a control-plane-only handle fed the contract's packets: CF32,
    n_out samples, sri_xdelta scaled by the step"""
    from psk_soft_amd import lib as pl

    C = len(props)
    h = pl.Handle(C, device=pl.DEVICE_NONE)
    h.configure(0, props)
    out_all = []
    for k, row in enumerate(plan.model):
        if k in skip:
            out_all.append(None)
            continue
        pk, out = (pl.Packet * C)(), (pl.Output * C)()
        for c, x in enumerate(row):
            if x is None:
                continue
            live = _live(plan.data[k][c])
            step = plan.steps[c] if live else 0
            pk[c].n_floats = x.size if live else plan.data[k][c].size
            # (a packet without samples is not resampled: it keeps the period it came with)
            pk[c].sri_xdelta = plan.xd[c] * (step * 2.0 ** -32) if step else plan.xd[c]
            assert pk[c].sri_xdelta == 0.01 or not live
            pk[c].sri_mode, pk[c].sriChanged, pk[c].present = 1, int(k == 0), 1
            pk[c].format = pl.FORMAT_CF32 if step else t_strided._fmt(pl, x.dtype)
            out[c].cap_symbols = 1 << 62
        h.process_device(0, pk, out)
        out_all.append([tuple(getattr(o, f) for f in OUT_FIELDS) for o in out])
    h.close()
    return out_all


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(oracle_mod, plan, props, res, proxies, ctx, skip=()):
    """the outputs against a fresh handle on the model's packets and against the oracle; the counts and SRI fields against the
    control plane; the histories against the model.  skip: calls left out of the comparison (refused ones)."""
    C = len(props)
    keep = [k for k in range(len(plan.data)) if k not in skip]
    got = {c: [res[0][0][c][k] for k in keep] for c in res[0][0]}
    model = [plan.model[k] for k in keep]
    assert_same(got, contiguous(C, props, model), "%s: against the model's packets" % ctx)
    check_parity(oracle_mod, got, lambda c: props[c], model, ctx)
    want = _planned_fields(props, plan, skip)
    for p in proxies:
        for k in keep:
            assert p.fields[k] == want[k], (ctx, k, [(c, a, b) for c, (a, b) in enumerate(zip(p.fields[k], want[k])) if a != b][:3])
            for c in range(C):
                assert _same_bits(p.hist[k][c], plan.hist[k][c]), (ctx, "history", k, c, p.hist[k][c], plan.hist[k][c])


def resamples_of(lines):
    return [t["cnt"] for t in lines if t["what"] == "resample"]


def _length_for(n_out, step):
    """(n, pos): a packet length and a position below 2^33 with exactly n_out outputs"""
    for pos in (step // 3, step // 3 + (1 << 31), 5, (1 << 32) + 7, (1 << 33) - 9, 1 << 33):
        for n in range(max(1, n_out * step // ONE - 3), n_out * step // ONE + 6):
            if rm.count(pos, step, n) == n_out:
                return n, pos
    raise AssertionError((n_out, step))


# ---- 1. the edges of a piece ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", STEPS)
def test_piece_edges_in_the_four_formats(oracle_mod, monkeypatch, capfd, step):
    """n_out = 1, P-1, P, P+1 and 2P+3 in each of the four formats, every channel restarted: one call, one resample launch"""
    from psk_soft_amd import lib as pl

    P = pl.resample_piece()
    targets = (1, P - 1, P, P + 1, 2 * P + 3)
    C = 4 * len(targets)
    props = _props(C)
    dts = [DT[c % 4] for c in range(C)]
    np_ = [_length_for(targets[c // 4], step) for c in range(C)]
    data = _pieces(_signals(96000 + step % 97, props, [n for n, _ in np_], dts), [[n for n, _ in np_]])
    plan = Plan(data, [step] * C, [p for _, p in np_], [[True] * C])
    assert [plan.n_out[0][c] for c in range(C)] == [targets[c // 4] for c in range(C)]
    proxies = []

    def run(h, cf):
        h.configure(0, props)
        proxies.append(Resampled(h, plan))
        return strided_run(proxies[-1], data, [None] * C, {}, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    lines = res[1][1][0]
    assert resamples_of(lines) == [C] and lines[0]["what"] == "resample" and not tunes_of(lines) and gathers(lines) == (0, 0, 0, 0), lines
    _check(oracle_mod, plan, props, res, proxies, "piece edges, step %#x" % step)


# ---- 2. the history carried from call to call ---------------------------------------------------------------------------------------

def test_history_carried_over_six_calls(oracle_mod, monkeypatch, capfd):
    """packets of 0, 1, 2, 3, P+5 and 4 samples, channel 2 absent in call 3; pos moved on by psk_soft_resample_advance.  Even
    channels restart (calls 0 and 1: the empty packet of call 0 is not resampled, so its restart is not looked at) on top of a
    history that must not show; odd channels start from a history set with psk_soft_resample_set_history."""
    from psk_soft_amd import lib as pl

    P = pl.resample_piece()
    C, lens1 = 8, [0, 1, 2, 3, P + 5, 4]
    props = _props(C)
    dts = [DT[c % 4] for c in range(C)]
    lens = [[n] * C for n in lens1]
    data = _pieces(_signals(96100, props, [sum(lens1)] * C, dts), lens)
    data[3][2] = None
    steps = [STEPS[(c // 2) % 4] for c in range(C)]
    hist0 = [np.array([3.5, -1.25, 1e-3, 40.0, -7.0, 0.5], np.float32) * (c + 1) for c in range(C)]
    restart = [[k < 2 and c % 2 == 0 for c in range(C)] for k in range(len(lens1))]
    plan = Plan(data, steps, [(c * 0x3243F6A9) % steps[c] for c in range(C)], restart, hist0=hist0)
    proxies = []

    def run(h, cf):
        h.configure(0, props)
        proxies.append(Resampled(h, plan))
        return strided_run(proxies[-1], data, [None] * C, {}, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert resamples_of(lines) == ([] if k == 0 else [C - 1] if k == 3 else [C]), (k, lines)
    for c in range(C):  # (the empty packets of call 0 left the histories as they were set)
        assert _same_bits(proxies[0].hist[0][c], hist0[c])
    _check(oracle_mod, plan, props, res, proxies, "carried history")


# ---- 3. where the samples lie ---------------------------------------------------------------------------------------------------------

def test_contiguous_strided_singles_and_a_run_of_columns(oracle_mod, monkeypatch, capfd):
    """channels 0 .. 7: columns 1 .. 8 of an int16 matrix 10 wide, unequal lengths (the tile gather, then the resample kernel on
    its rows); 8 .. 11: single columns of matrices 7 wide in the four formats (read where they lie); 12 .. 15: contiguous packets
    in the four formats.  Two calls, so every source also follows a carried history."""
    from psk_soft_amd import lib as pl

    P = pl.resample_piece()
    C, calls = 16, 2
    props = _props(C)
    dts = [np.int16] * 8 + list(DT) + list(DT)
    place = [(0, 1 + c) for c in range(8)] + [(1 + j, 2 + j) for j in range(4)] + [None] * 4
    widths = {0: 10, 1: 7, 2: 7, 3: 7, 4: 7}
    lens = [[P + 300 + 37 * ((5 * c + 3 * k) % 11) + (c % 2) for c in range(C)] for k in range(calls)]
    data = _pieces(_signals(96200, props, [sum(lens[k][c] for k in range(calls)) for c in range(C)], dts), lens)
    steps = [STEPS[c % 4] for c in range(C)]
    plan = Plan(data, steps, [(c * 0x9E3779B1) % steps[c] for c in range(C)], [[k == 0] * C for k in range(calls)])
    proxies = []

    def run(h, cf):
        h.configure(0, props)
        proxies.append(Resampled(h, plan))
        return strided_run(proxies[-1], data, place, widths, cf)  # (asserts that the sources come back as they were)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (1, 1, 0, 0), (k, lines)
        assert [t["what"] for t in lines[:2]] == ["gather_tiles", "resample"], (k, lines[:2])
        assert resamples_of(lines) == [C] and not tunes_of(lines), (k, lines)
    _check(oracle_mod, plan, props, res, proxies, "sources")


# ---- 4. tuned and resampled in one pass --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tuned_only", [0, 4])
def test_tuned_and_resampled_in_one_pass(oracle_mod, monkeypatch, capfd, tuned_only):
    """12 channels, every one tuned: resampled too, but for the last `tuned_only` of them.  Against tune_model.apply followed by
    the resampler's model.  Channels 0 .. 7 are a run of columns, the others contiguous; two calls carry phase, pos and history."""
    from psk_soft_amd import lib as pl

    P = pl.resample_piece()
    C, calls = 12, 2
    props = _props(C)
    dts = [np.int8] * 8 + list(DT)
    place = [(0, c) for c in range(8)] + [None] * 4
    lens = [[P + 100 + 53 * ((3 * c + k) % 7) for c in range(C)] for k in range(calls)]
    data = _pieces(_signals(96300, props, [sum(lens[k][c] for k in range(calls)) for c in range(C)], dts), lens)
    steps = [STEPS[c % 4] if c < C - tuned_only else 0 for c in range(C)]
    tsteps = [(tm.step_word(0.003), tm.step_word(-0.01), 1, NEG)[c % 4] for c in range(C)]
    plan = Plan(data, steps, [(c * 0x9E3779B1) % (steps[c] or ONE) for c in range(C)], [[k == 0] * C for k in range(calls)], tsteps,
                [(0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64) for c in range(C)])
    proxies = []

    def run(h, cf):
        h.configure(0, props)
        proxies.append(Resampled(h, plan))
        return strided_run(proxies[-1], data, place, {0: 9}, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert resamples_of(lines) == [C - tuned_only] and tunes_of(lines) == ([tuned_only] if tuned_only else []), (k, lines)
        assert [t["what"] for t in lines[: 2 + bool(tuned_only)]] == ["gather_tiles"] + ["tune"] * bool(tuned_only) + ["resample"], (k, lines[:3])
    _check(oracle_mod, plan, props, res, proxies, "tuned and resampled, %d tuned only" % tuned_only)


# ---- 5. a mixed batch; a batch without a resampled packet ------------------------------------------------------------------------------

def test_packets_with_step_zero_take_the_tuned_entrys_path(oracle_mod, monkeypatch, capfd):
    """every second packet has step 0 (and junk in pos, flags and pad, which are not looked at): it gives what the tuned entry
    gives for it -- its own contract's CF32 packet if tuned, itself in its own format if not, the in-place builds included.  A
    second sequence has no resampled packet at all: no resample launch."""
    from psk_soft_amd import lib as pl
    from tests.test_gpu_tune import Tuned

    C = 12
    props = _props(C, numAvg=(100, 64, 25))
    dts = [DT[(c // 2) % 4] for c in range(C)]
    lens = [[3000 + 41 * c for c in range(C)]]
    data = _pieces(_signals(96400, props, lens[0], dts), lens)
    steps = [STEP_837 if c % 2 else 0 for c in range(C)]
    tsteps = [None if c in (2, 4, 9) else tm.step_word(0.002 * (c - 5)) for c in range(C)]
    plan = Plan(data, steps, [7 * c for c in range(C)], [[True] * C], tsteps, [c << 50 for c in range(C)])
    for c in range(0, C, 2):
        plan.rss[0][c] = pl.Resample(1 << 60, 0, 0xFFFFFFFF, 77)
    proxies = []

    def run(h, cf):
        h.configure(0, props)
        proxies.append(Resampled(h, plan))
        return strided_run(proxies[-1], data, [None] * C, {}, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    lines = res[1][1][0]
    n_tuned_only = sum(1 for c in range(0, C, 2) if tsteps[c] is not None)
    assert resamples_of(lines) == [C // 2] and tunes_of(lines) == [n_tuned_only], lines
    assert (S, H_CS16) in screened(lines), screened(lines)  # (channel 2: int16, step 0, untuned -- read in place as ever)
    _check(oracle_mod, plan, props, res, proxies, "mixed batch")
    # ... and the step-0 packets are, stream for stream, the tuned entry's
    h = pl.Handle(C, device=0)
    try:
        h.configure(0, props)
        tuned_got = strided_run(Tuned(h, plan.tunes), data, [None] * C, {})[0]
    finally:
        h.close()
    assert_same({c: res[0][0][c] for c in range(0, C, 2)}, {c: tuned_got[c] for c in range(0, C, 2)}, "step 0 against the tuned entry")

    none = Plan(data, [0] * C, tsteps=tsteps, phase0=[c << 50 for c in range(C)])
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    h = pl.Handle(C, device=0)
    try:
        h.configure(0, props)
        got, traces, _ = strided_run(Resampled(h, none, histories=False), data, [None] * C, {}, capfd)
    finally:
        h.close()
        monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES")
    assert not resamples_of(traces[0]) and tunes_of(traces[0]) == [sum(t is not None for t in tsteps)], traces[0]
    assert_same(got, tuned_got, "no resampled packet against the tuned entry")


# ---- 6. a refused call ------------------------------------------------------------------------------------------------------------------

def test_a_refused_call_changes_nothing(oracle_mod, monkeypatch, capfd):
    """three calls, the second with the packets, positions and flags of the third but one output row a symbol short of what
    the packet of n_out samples emits: PSK_SOFT_ERR_CAPACITY.  The third call's outputs and histories are those of a run without the second."""
    from psk_soft_amd import lib as pl

    P = pl.resample_piece()
    C = 6
    props = _props(C)
    dts = [DT[c % 4] for c in range(C)]
    lens = [[P + 200 + 8 * c for c in range(C)], [2 * P + 77 - 8 * c for c in range(C)]]
    two = _pieces(_signals(96500, props, [lens[0][c] + lens[1][c] for c in range(C)], dts), lens)
    steps = [STEPS[c % 4] for c in range(C)]
    pos0 = [(c * 0x3243F6A9) % steps[c] for c in range(C)]
    good = Plan(two, steps, pos0, [[k == 0] * C for k in range(2)])
    # the plan with the refused call in the middle: the same arguments twice (its model rows are only used to size the rows)
    data = [two[0], two[1], two[1]]
    plan = Plan(data, steps, pos0, [[k == 0] * C for k in range(3)])
    for attr in ("rss", "tunes", "model", "n_out", "hist"):
        rows = getattr(good, attr)
        setattr(plan, attr, [rows[0], rows[1], rows[1]])
    proxies = []
    emits = _planned_fields(props, good)[1][3][OUT_FIELDS.index("n_symbols")]
    assert emits > 100

    def run(h, cf):
        h.configure(0, props)
        proxies.append(Resampled(h, plan, short={(1, 3): emits - 1}, refused={1: 6}))
        return strided_run(proxies[-1], data, [None] * C, {}, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for p in proxies:  # (behind the refused call the histories are still those behind call 0)
        for c in range(C):
            assert _same_bits(p.hist[1][c], good.hist[0][c]), c
    _check(oracle_mod, plan, props, res, proxies, "refused call", skip=(1,))


# ---- 7. a call of 1100 packets: workgroups that walk several pieces -------------------------------------------------------------------------

def test_1100_packets_in_one_call_and_their_histories_carried(oracle_mod, monkeypatch, capfd):
    """1100 resampled packets in one call: launch_resample gives a packet two workgroups, so the ten packets of 2P+1 .. 5P+3
    outputs are walked by workgroups that take several pieces each, and the history behind them is written by workgroup 0 for
    some and by workgroup 1 for others.  Those ten sit on channels with samplesPerBaud 1 and numAvg 0: every row sample is a
    symbol.  The other packets have 1 .. 40 samples; every 50th has pos 2^33 and 1 or 2 samples -- no output, but its history
    moves.  A second call reads the histories back and carries them.  What tests/test_gpu_prepass_probe.py cannot see is
    checked here: the descriptor offsets, row offsets and history slots front_layout and front_describe compute for a call of this size."""
    from psk_soft_amd import lib as pl

    P = pl.resample_piece()
    C, calls = 1100, 2
    targets = (2 * P + 1, 3 * P, 4 * P + 2, 5 * P + 3, 2 * P + 1, 3 * P, 4 * P + 2, 5 * P + 3, 5 * P + 1, 2 * P + 2)
    big = {3 + 110 * j: t for j, t in enumerate(targets)}
    quiet = [c for c in range(C) if c % 50 == 10]
    props = _props(C)
    for c in big:
        props[c] = dict(props[c], samplesPerBaud=1, numAvg=0)
    dts = [DT[c % 4] for c in range(C)]
    steps = [STEPS[(c + c // 4) % 4] for c in range(C)]
    pos0 = [(c * 0x3243F6A9) % steps[c] for c in range(C)]
    lens = [[1 + (13 * c) % 40 for c in range(C)], [1 + (7 * c + 3) % 40 for c in range(C)]]
    for c, t in big.items():
        lens[0][c], pos0[c] = _length_for(t, steps[c])
        lens[1][c] = 300 + c % 7
    for c in quiet:
        lens[0][c], pos0[c] = 1 + (c // 50) % 2, 1 << 33
    assert {1, 2, 3, 40} <= set(lens[0]) and not set(quiet) & set(big)
    # every eighth channel is a single column of a matrix 7 wide: read where it lies, at its stride
    place = [(c, 2) if c % 8 == 5 else None for c in range(C)]
    widths = {c: 7 for c in range(C) if c % 8 == 5}
    assert any(place[c] is not None for c in big) and any(place[c] is None for c in big)
    data = _pieces(_signals(96700, props, [lens[0][c] + lens[1][c] for c in range(C)], dts), lens)
    tsteps = [None if c % 3 == 0 else (tm.step_word(0.003), tm.step_word(-0.01), 1, NEG)[c % 4] for c in range(C)]
    # even channels restart in call 0; odd ones, and every second packet without output, start from a history set in front of it
    carried = [c % 2 == 1 or c % 100 == 10 for c in range(C)]
    hist0 = [np.array([3.5, -1.25, 1e-3, 40.0, -7.0, 0.5], np.float32) * (c % 9 + 1) if carried[c] else None for c in range(C)]
    restart = [[not carried[c] for c in range(C)], [c % 11 == 5 for c in range(C)]]
    plan = Plan(data, steps, pos0, restart, tsteps, [(0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64) for c in range(C)], hist0)
    assert all(plan.n_out[0][c] == t for c, t in big.items()) and all(plan.n_out[0][c] == 0 for c in quiet)
    assert any(plan.hist[0][c].any() for c in quiet), "a packet without output moved its history"
    assert max(plan.n_out[0]) == 5 * P + 3 and sorted(plan.n_out[0])[-11] <= 80
    proxies = []

    def run(h, cf):
        h.configure(0, props)
        proxies.append(Resampled(h, plan))
        return strided_run(proxies[-1], data, place, widths, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert resamples_of(lines) == [C] and lines[0]["what"] == "resample" and not tunes_of(lines) and gathers(lines) == (0, 0, 0, 0), (k, lines[:3])
    _check(oracle_mod, plan, props, res, proxies, "1100 packets")


# ---- 8. schedules and quality records ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["time_tiled", "deferred_join", "quality"])
def test_schedules_and_quality_records(oracle_mod, monkeypatch, capfd, schedule):
    from psk_soft_amd import lib as pl

    C, calls, n = 12, 2, 4200
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(25, 100, 200, 400)[(c // 3) % 4] if schedule == "deferred_join" else 64,
                  phaseAvg=(10, 50)[c % 2]) for c in range(C)]
    dts = [DT[c % 4] for c in range(C)]
    lens = [[n + 33 * c + 500 * k for c in range(C)] for k in range(calls)]
    data = _pieces(_signals(96600, props, [sum(lens[k][c] for k in range(calls)) for c in range(C)], dts), lens)
    steps = [STEPS[c % 4] for c in range(C)]
    tsteps = [None if c % 2 else tm.step_word(0.001 * (c + 1)) for c in range(C)]
    plan = Plan(data, steps, [(c * 0x9E3779B1) % steps[c] for c in range(C)], [[k == 0] * C for k in range(calls)], tsteps, [c << 40 for c in range(C)])
    proxies, recs, stats = [], [], []

    def options(h):
        h.configure(0, props)
        if schedule == "time_tiled":
            h.set_option(pl.Handle.OPT_TIME_TILED, 2)
        elif schedule == "deferred_join":
            h.set_option(pl.Handle.OPT_DEFERRED_JOIN, 1)
        else:
            h.set_option(pl.Handle.OPT_QUALITY, 1)

    def run(h, cf):
        options(h)
        # (no look at the histories between deferred calls: that would wait for the device)
        proxies.append(Resampled(h, plan, histories=schedule != "deferred_join"))
        got = strided_run(proxies[-1], data, [None] * C, {}, cf, sync_each=schedule != "deferred_join")
        stats.append(h.stats())
        if schedule == "quality":
            recs.append(bytes(h.quality_records()))
        if schedule == "deferred_join":
            proxies[-1].hist = [plan.hist[0], [h.resample_history(c) for c in range(C)]]
        return got

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    if schedule == "time_tiled":
        assert stats[0]["channels_tiled"] > 0, stats[0]
    if schedule == "quality":
        h = pl.Handle(C, device=0)
        try:
            options(h)
            t_cs8.device_run(h, plan.model)
            want = bytes(h.quality_records())
        finally:
            h.close()
        assert recs[0] == want and recs[1] == want
    _check(oracle_mod, plan, props, res, proxies, schedule)
