"""psk_soft_process_device_tuned on a real MI355X: packets shifted in frequency on the GPU (psk_tune.hip) in front of the
demodulator.  Every checked stream is, bit for bit, what the oracle gives on the packet tests/tune_model.py computes -- the
contract's CF32 packet of the shifted samples -- and what a fresh handle gives when it is fed those CF32 packets contiguously;
the launch trace (PSK_SOFT_TRACE_LAUNCHES=2) says which pre-pass kernels ran, and the source buffers come back byte for byte.

The calls go through tests.test_gpu_strided.strided_run (layout, poison, download) behind a handle proxy that adds the tunes."""
import ctypes

import numpy as np
import pytest

import tests.test_gpu_cs8 as t_cs8
import tests.test_gpu_strided as t_strided
from tests import tune_model as tm
from tests.test_gpu_cs16_schedules import H_CS16, _synth, assert_same, check_parity, screened, untraced_then_traced, whats
from tests.test_gpu_cs8 import H_CS8, SCALE8, device_run, q8
from tests.test_gpu_strided import contiguous, gathers, strided_run

pytestmark = pytest.mark.gpu

F16 = np.dtype(np.float16)
DT = (np.float32, np.int16, np.int8, np.float16)
NEG = (1 << 63) + 12345


@pytest.fixture(autouse=True)
def _half_packets_in_the_shared_helpers(monkeypatch):
    """the shared helpers take a packet's format from its dtype: teach them float16 (as tests/test_gpu_cf16.py does)"""
    from psk_soft_amd import lib as pl

    fmt8, fmts, poison = t_cs8._fmt, t_strided._fmt, t_strided._poison
    monkeypatch.setattr(t_cs8, "_fmt", lambda x: pl.FORMAT_CF16 if x.dtype == F16 else fmt8(x))
    monkeypatch.setattr(t_strided, "_fmt", lambda p, dt: p.FORMAT_CF16 if np.dtype(dt) == F16 else fmts(p, dt))
    monkeypatch.setattr(t_strided, "_poison", lambda dt: np.uint16(0x7E55).view(np.float16) if np.dtype(dt) == F16 else poison(dt))


class Tuned:
    """a Handle whose process_device_strided is process_device_tuned with tunes[k] ([(phase, step)] per channel, or None) in the
    k-th call made through it"""

    def __init__(self, h, tunes):
        self._h, self._tunes, self._k = h, tunes, 0

    def __getattr__(self, name):
        return getattr(self._h, name)

    def process_device_strided(self, ch0, pk, strides, outs, stream=None):
        t = self._tunes[self._k]
        self._k += 1
        self._h.process_device_tuned(ch0, pk, strides, t, outs, stream)


def _signals(seed, props, lens, dts):
    """one stream per channel in its dtype: int8 values for the integer and half formats, floats with every mantissa bit in use
    (40 x the synthetic channel) for float32"""
    Ms = [p["constelationSize"] for p in props]
    raw = _synth(seed, Ms, props[0]["samplesPerBaud"], list(lens))
    return [(np.asarray(x, np.float32) * np.float32(SCALE8)) if np.dtype(dt) == np.float32 else q8(x).astype(dt) for x, dt in zip(raw, dts)]


def _pieces(streams, lens):
    """data[k][c] = lens[k][c] complex samples of channel c, one call after the other"""
    K, C = len(lens), len(streams)
    at = [0] * C
    data = []
    for k in range(K):
        row = []
        for c in range(C):
            row.append(streams[c][2 * at[c] : 2 * (at[c] + lens[k][c])])
            at[c] += lens[k][c]
        data.append(row)
    return data


def _tunes(data, phase0, steps):
    """tunes[k][c] of a continuous stream per channel: the phase word advanced by psk_soft_tune_advance from call to call"""
    from psk_soft_amd import lib as pl

    ph, out = list(phase0), []
    for row in data:
        out.append([(0, 0) if steps[c] is None else (ph[c], steps[c]) for c in range(len(row))])
        for c, x in enumerate(row):
            if x is not None and steps[c] is not None:
                ph[c] = pl.tune_advance(ph[c], steps[c], x.size // 2)
    return out


def _model(data, tunes):
    """the packets of the contract: float32 tune_model.apply of every tuned packet, the others as they are"""
    return [[x if x is None or t is None or t[c] == (0, 0) or x.size < 2 else tm.apply(t[c][0], t[c][1], x) for c, x in enumerate(row)]
            for row, t in zip(data, tunes)]


def tunes_of(lines):
    return [t["cnt"] for t in lines if t["what"] == "tune"]


# ---- 1. contiguous packets of the four formats, state and phase carried over three calls ------------------------------------------

def test_contiguous_mixed_formats_over_three_calls(oracle_mod, monkeypatch, capfd):
    """12 channels, M 2 / 4 / 8, some differential, the four formats; steps up, down (>= 2^63), 1 and 2^63 + 12345.  Channel 5
    brings 70 001 samples in call 0 (nine pieces, nine workgroups on one packet); channels 8 .. 11 bring 0, 1, 2 and 3 samples in
    call 1; channel 2 counts an odd element more than it has."""
    S, C, calls = 8, 12, 3
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 64, 25)[c % 3], phaseAvg=(50, 10, 200)[(c // 3) % 3],
                  differentialDecoding=int(c % 5 == 3)) for c in range(C)]
    dts = [DT[c % 4] for c in range(C)]
    lens = [[3000 + 167 * ((5 * c + 3 * k) % 13) for c in range(C)] for k in range(calls)]
    lens[0][5] = 70001
    for j in range(4):
        lens[1][8 + j] = j
    data = _pieces(_signals(92000, props, [sum(lens[k][c] for k in range(calls)) for c in range(C)], dts), lens)
    steps = [(tm.step_word(0.003), tm.step_word(-0.01), 1, NEG)[(c // 2) % 4] for c in range(C)]
    assert steps[2] >= 1 << 63
    tunes = _tunes(data, [(0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64) for c in range(C)], steps)
    model = _model(data, tunes)

    def run(h, cf):
        h.configure(0, props)
        return strided_run(Tuned(h, tunes), data, [None] * C, {}, cf, odd=(2,))

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (0, 0, 0, 0), (k, lines)
        assert tunes_of(lines) == [C - (1 if k == 1 else 0)], (k, lines)  # (the packet of 0 samples is not tuned: nothing to read)
        assert lines[0]["what"] == "tune", (k, lines[0])
        assert not whats(lines) & {"cs16_convert", "cs8_convert", "cf16_convert"}, (k, whats(lines))
    assert_same(res[0][0], contiguous(C, props, model), "tuned against the model's packets")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], model, "tuned contiguous")


# ---- 2. strided, contiguous, tuned and untuned packets in one call ---------------------------------------------------------------

def _mix():
    """channels 0 .. 23: columns 5 .. 28 of an int16 matrix 40 wide, tuned (tile kernel, then tune); 24 .. 26: tuned single
    columns of a float32, an int8 and a half matrix; 27, 28: contiguous int16 and int8 packets with tune {0, 0}; 29, 30: columns
    0 and 2 of an int16 matrix 4 wide with tune {0, 0} (plain strided gather)."""
    S, C, calls = 8, 31, 2
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 64)[c % 2], phaseAvg=(50, 10, 200)[(c // 3) % 3],
                  differentialDecoding=int(c % 7 == 3)) for c in range(C)]
    dts = [np.int16] * 24 + [np.float32, np.int8, np.float16, np.int16, np.int8, np.int16, np.int16]
    place = [(0, 5 + c) for c in range(24)] + [(1, 1), (2, 0), (3, 3), None, None, (4, 0), (4, 2)]
    widths = {0: 40, 1: 3, 2: 2, 3: 7, 4: 4}
    lens = [[3100 + 37 * ((7 * c + 5 * k) % 23) + (c % 2) for c in range(C)] for k in range(calls)]
    data = _pieces(_signals(93000, props, [sum(lens[k][c] for k in range(calls)) for c in range(C)], dts), lens)
    steps = [(tm.step_word(0.004), tm.step_word(-0.02), NEG, 1, (1 << 64) - 1)[c % 5] if c < 27 else None for c in range(C)]
    tunes = _tunes(data, [(0xD1B54A32D192ED03 * (c + 3)) % (1 << 64) for c in range(C)], steps)
    return S, C, props, place, widths, data, tunes


def test_strided_mix_in_one_call(oracle_mod, monkeypatch, capfd):
    S, C, props, place, widths, data, tunes = _mix()
    model = _model(data, tunes)

    def run(h, cf):
        h.configure(0, props)
        return strided_run(Tuned(h, tunes), data, place, widths, cf)  # (asserts that the source comes back as it was)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (1, 1, 1, 2), (k, lines)
        assert tunes_of(lines) == [27], (k, lines)
        assert [t["what"] for t in lines[:3]] == ["gather_tiles", "gather_singles", "tune"], (k, lines[:3])
        # the packets with tune {0, 0} are not tuned at all: the integer ones still reach their in-place builds
        assert (S, H_CS16) in screened(lines) and (S, H_CS8) in screened(lines), (k, screened(lines))
    assert_same(res[0][0], contiguous(C, props, model), "tuned against the model's packets")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], model, "tuned mix")


# ---- 3. tune == NULL and tunes of {0, 0} are the strided entry --------------------------------------------------------------------

def test_null_and_all_zero_tunes_are_the_strided_call(oracle_mod, monkeypatch, capfd):
    from psk_soft_amd import lib as pl

    S, C, props, place, widths, data, _ = _mix()
    runs = []
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    for tunes in ("strided", None, [(0, 0)] * C):
        h = pl.Handle(C, device=0)
        try:
            h.configure(0, props)
            hh = h if tunes == "strided" else Tuned(h, [tunes] * len(data))
            got, traces, _ = strided_run(hh, data, place, widths, capfd)
            runs.append((got, [[{k: v for k, v in t.items() if k != "stream"} for t in lines] for lines in traces], h.channel_stats()))
        finally:
            h.close()
    monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES")
    for got, traces, stats in runs[1:]:
        assert traces == runs[0][1]
        assert stats == runs[0][2]
        assert_same(got, runs[0][0], "untuned against strided")
    assert all(not tunes_of(lines) for lines in runs[0][1])
    assert all(gathers(lines) == (1, 1, 3, 5) for lines in runs[0][1]), runs[0][1]


# ---- 4. back-to-back calls ----------------------------------------------------------------------------------------------------------

def test_back_to_back_calls_deferred_join_and_a_second_stream(oracle_mod, monkeypatch, capfd):
    """PSK_SOFT_OPT_DEFERRED_JOIN, four window classes, four tuned calls issued without a host wait on the handle's stream (every
    call gathers and tunes into the scratch a class of the call before may still be reading: the entry joins first), then two
    more on a second stream, which takes a scratch of its own."""
    from psk_soft_amd import lib as pl

    S, C, calls, n = 8, 48, 6, 4000
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(25, 100, 200, 400)[(c // 3) % 4], phaseAvg=(10, 50, 200)[(c // 12) % 3])
             for c in range(C)]
    dts = [np.int16] * 24 + [DT[c % 4] for c in range(24)]
    place = [(0, 2 + c) for c in range(24)] + [None] * 24
    lens = [[n - 301 * (k % 3) + (c % 3) for c in range(C)] for k in range(calls)]
    data = _pieces(_signals(94000, props, [sum(lens[k][c] for k in range(calls)) for c in range(C)], dts), lens)
    steps = [(tm.step_word(0.002), tm.step_word(-0.006), None, NEG)[c % 4] for c in range(C)]
    tunes = _tunes(data, [(0xA0761D6478BD642F * (c + 1)) % (1 << 64) for c in range(C)], steps)
    model = _model(data, tunes)
    n_tuned = sum(s is not None for s in steps)
    L = pl.load()
    second = ctypes.c_void_p()
    assert L.hipStreamCreateWithFlags(ctypes.byref(second), 1) == 0  # (non-blocking)

    def run(h, cf):
        h.configure(0, props)
        h.set_option(pl.Handle.OPT_DEFERRED_JOIN, 1)
        a, tr_a, _ = strided_run(Tuned(h, tunes[:4]), data[:4], place, {0: 28}, cf, sync_each=False)
        b, tr_b, _ = strided_run(Tuned(h, tunes[4:]), data[4:], place, {0: 28}, cf, sync_each=False, k0=4, stream=second.value)
        return {c: a[c] + b[c] for c in a}, tr_a + tr_b

    try:
        res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    finally:
        L.hipStreamDestroy(second)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines)[:2] == (1, 1) and tunes_of(lines) == [n_tuned], (k, lines)
        assert len(screened(lines)) >= 3, (k, screened(lines))
    assert len({lines[0]["stream"] for lines in res[1][1]}) == 2
    assert_same(res[0][0], contiguous(C, props, model), "deferred tuned calls against joined calls on the model's packets")
    check_parity(oracle_mod, {c: res[0][0][c] for c in (0, 1, 2, 3, 23, 24, 25, 27, C - 1)}, lambda c: props[c], model, "back to back")


# ---- 5. quality records ----------------------------------------------------------------------------------------------------------------

def test_quality_records_and_the_lock_of_a_channel_off_its_centre(oracle_mod, monkeypatch, capfd):
    """PSK_SOFT_OPT_QUALITY: the records of tuned calls are byte for byte those of the calls on the model's packets.  Channels 0
    and 1 carry the same 8-PSK signal 0.05 cycles per symbol off its centre: tuned back it locks, left alone it does not."""
    from psk_soft_amd import lib as pl
    from ref_stimulus import gen_psk

    S, C, n_sym, offset = 8, 10, 600, 0.05
    props = [dict(samplesPerBaud=S, constelationSize=8 if c < 2 else (2, 4, 8)[c % 3], numAvg=100, phaseAvg=50, differentialDecoding=int(c == 7))
             for c in range(C)]
    iq, _ = gen_psk(n_sym, S, 8)
    x = (iq[0::2].astype(np.float64) + 1j * iq[1::2]) * np.exp(2j * np.pi * (offset / S) * np.arange(n_sym * S))
    off = np.empty(2 * x.size, np.float32)
    off[0::2], off[1::2] = x.real, x.imag
    dts = [np.float32, np.float32] + [np.int16] * 4 + [DT[c % 4] for c in range(6, C)]
    data = [[off, off] + _signals(95000, props[2:], [n_sym * S + c for c in range(2, C)], dts[2:])]
    place = [None, None] + [(0, c) for c in range(2, 6)] + [None] * (C - 6)  # (four columns of an int16 matrix 8 wide)
    steps = [pl.tune_step(-offset / S), None] + [(tm.step_word(0.001), NEG, tm.step_word(-0.004))[c % 3] for c in range(2, C)]
    tunes = _tunes(data, [0] + [(0xE7037ED1A0B428DB * (c + 1)) % (1 << 64) for c in range(1, C)], steps)
    model = _model(data, tunes)
    recs = []

    def run(h, cf):
        h.configure(0, props)
        h.set_option(pl.Handle.OPT_QUALITY, 1)
        got, traces, _ = strided_run(Tuned(h, tunes), data, place, {0: 8}, cf)
        recs.append((bytes(h.quality_records()), h.quality()))
        return got, traces

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    lines = res[1][1][0]
    assert tunes_of(lines) == [C - 1] and gathers(lines) == (0, 0, 0, 0), lines  # (the four columns are read where they lie)
    assert [t["what"] for t in lines[-2:]] == ["quality_fold", "quality_join"], lines
    h = pl.Handle(C, device=0)
    try:
        h.configure(0, props)
        h.set_option(pl.Handle.OPT_QUALITY, 1)
        got_m = device_run(h, model)[0]
        want = bytes(h.quality_records())
    finally:
        h.close()
    assert_same(res[0][0], got_m, "tuned against the model's packets")
    assert recs[0][0] == want and recs[1][0] == want
    q = recs[0][1]
    print("lock tuned %.4f untuned %.4f" % (q[0]["lock"], q[1]["lock"]))
    assert q[0]["lock"] > 0.99
    assert q[1]["lock"] < 0.5
    check_parity(oracle_mod, res[0][0], lambda c: props[c], model, "quality")
