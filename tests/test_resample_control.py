"""Resampled packets without a GPU: the host-side helpers (psk_soft_resample_step / _count / _advance / _apply) against
tests/resample_model.py, the entry on control-plane-only handles (PSK_SOFT_DEVICE_NONE) -- it checks, then plans and counts on
n_out samples and the scaled sample period --, and what the resampler is for: a symbol rate that does not divide the sample
rate, which the integer samplesPerBaud of the reference cannot follow, brought to 8 samples a symbol in front of it (through the
oracle)."""
import ctypes
import math

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests import resample_model as rm
from tests.test_strided_control import _handle, _packets, _peeks, _queries, _results, _table

U32 = np.uint32
ONE = 1 << 32
NEW = ("psk_soft_process_device_resampled", "psk_soft_resample_get_history", "psk_soft_resample_set_history", "psk_soft_resample_step",
       "psk_soft_resample_count", "psk_soft_resample_advance", "psk_soft_resample_apply", "psk_soft_resample_piece")


def test_the_symbols_are_exported_and_the_abi_version_stays():
    L = pl.load()
    for name in NEW:
        assert name in pl.EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    R = pl.Resample
    assert ctypes.sizeof(R) == 24 and (R.pos.offset, R.step.offset, R.flags.offset, R.pad.offset) == (0, 8, 16, 20)
    assert ctypes.sizeof(pl.Packet) == 32 and ctypes.sizeof(pl.Output) == 104 and ctypes.sizeof(pl.Stats) == 96
    assert pl.resample_piece() >= 2 and pl.resample_piece() % 2 == 0


# ---- the definition ----------------------------------------------------------------------------------------------------------

def _samples(rng, n):
    """finite samples: amplitudes 1e-3 / 1 / 300, both zeros, denormals"""
    x = (rng.standard_normal(2 * n) * rng.choice([1e-3, 1.0, 300.0], 2 * n)).astype(np.float32)
    if n >= 8:
        x[:8] = [0.0, -0.0, -0.0, 0.0, 1.0, 0.0, 0.0, -1.0]
        x[8:12] = np.array([1, 0x00400000, 0x807FFFFF, 0x00800000], U32).view(np.float32)  # denormals are kept
        x[12:16] = np.array([0x00000003, 0x80000001, 0x007FFFFF, 0x80000100], U32).view(np.float32)
    return x


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.size == b.size and np.array_equal(a.view(U32), b.view(U32))


STEPS = [1 << 31, ONE, 1 << 33, ONE + 1, ONE - 1, "8.37/8", "random", "random", "random"]


@pytest.mark.parametrize("case", range(len(STEPS)))
def test_resample_apply_equals_the_model_bit_for_bit(case):
    rng = np.random.default_rng(2000 + case)
    step = STEPS[case]
    if step == "8.37/8":
        step = pl.resample_step(8.37 / 8)
        assert step == int(8.37 / 8 * 2.0 ** 32)
    elif step == "random":
        step = int(rng.integers(1 << 31, (1 << 33) + 1, dtype=np.uint64))
    n = 6000
    x = _samples(rng, n)
    hist = _samples(rng, 3)
    for pos in (0, step - 1, 1, int(rng.integers(0, step, dtype=np.uint64))):
        for history, restart in ((None, False), (hist, False), (hist, True)):
            got, gh = pl.resample_apply((pos, step, int(restart)), x, history)
            want, wh = rm.apply(pos, step, x, history, restart)
            assert got.size == 2 * rm.count(pos, step, n) == 2 * pl.resample_count((pos, step), n)
            assert _same(got, want), (pos, np.flatnonzero(got.view(U32) != want.view(U32))[:5])
            assert _same(gh, wh) and _same(gh, x[-6:])
    # an odd last element is dropped; nothing is a null call that leaves the history as it was
    assert _same(pl.resample_apply((0, step), x[:15], hist)[0], rm.apply(0, step, x[:14], hist)[0])
    y, h = pl.resample_apply((5, step), x[:1], hist)
    assert y.size == 0 and _same(h, hist)


def test_unit_step_is_a_delay_of_two_samples():
    rng = np.random.default_rng(5)
    n = 4097
    x = _samples(rng, n)
    y, h = pl.resample_apply((0, ONE, pl.RS_RESTART), x)
    assert y.size == 2 * n
    assert y[:4].view(U32).tolist() == [0, 0, 0, 0]  # (+0: the first two outputs after a restart)
    # every further output is s[i-2] itself, denormals included: the weights are (-0, 1, +0, -0), and x + (+-0) keeps x -- but
    # for the sign of a zero, which depends on its neighbours' signs
    pz = lambda v: np.where(v == 0, np.float32(0), v).astype(np.float32)  # noqa: E731
    assert _same(pz(y[4:]), pz(x[: 2 * (n - 2)]))
    assert np.count_nonzero(y[4:]) == np.count_nonzero(x[: 2 * (n - 2)]) > 2 * n - 20
    assert _same(h, x[-6:])
    # ... and with a history the delay line runs on across the packets' seam
    y2, _ = pl.resample_apply((0, ONE), x[:400], x[-6:])
    assert _same(pz(y2[:4]), pz(x[-4:])) and _same(pz(y2[4:]), pz(x[:396]))


@pytest.mark.parametrize("step", [1 << 31, ONE, 1 << 33, int(8.37 / 8 * 2.0 ** 32), 0x123456789])
def test_a_stream_cut_into_packets_gives_the_bytes_of_the_whole(step):
    rng = np.random.default_rng(11)
    n = 7001 + 10 + 2500
    x = _samples(rng, n)
    pos0 = step // 3
    whole, _ = pl.resample_apply((pos0, step, pl.RS_RESTART), x)
    m = rm.Stream(step, pos0)
    pos, hist, at, parts = pos0, None, 0, []
    cuts = [0, 1, 2, 3, 4, 7001]
    for k, ln in enumerate(cuts + [n - sum(cuts)]):
        part = x[2 * at : 2 * (at + ln)]
        y, hist = pl.resample_apply((pos, step, pl.RS_RESTART if k == 0 else 0), part, hist)
        want = m.push(part, restart=(k == 0))
        assert _same(y, want), (k, ln)
        assert _same(hist, m.history), (k, ln)
        pos = pl.resample_advance((pos, step), ln)
        assert pos == m.pos and pos < step
        parts.append(y)
        at += ln
    assert at == n
    assert _same(np.concatenate(parts), whole)


def test_count_and_advance_against_big_integers():
    rng = np.random.default_rng(3)
    cases = [(0, ONE, 0), (5, ONE, 0), (0, ONE, 1), (ONE, ONE, 1), (ONE - 1, ONE, 1), (3 * ONE + 7, 1 << 33, 2), (1 << 33, 1 << 31, 1),
             (1 << 33, 1 << 33, 2), (1 << 33, 1 << 33, 3), (0, 1 << 31, (1 << 30) - 1), ((1 << 33) - 1, (1 << 33), (1 << 30) - 1)]
    for _ in range(300):
        step = int(rng.integers(1 << 31, (1 << 33) + 1, dtype=np.uint64))
        cases.append((int(rng.integers(0, (1 << 33) + 1, dtype=np.uint64)), step, int(rng.integers(0, 1 << int(rng.integers(1, 31))))))
    for pos, step, n in cases:
        n_out = 0 if pos >= n * ONE else -(-(n * ONE - pos) // step)
        assert all(pos + m * step < n * ONE for m in ((n_out - 1,) if n_out else ())) and pos + n_out * step >= n * ONE
        assert pl.resample_count((pos, step), n) == n_out == rm.count(pos, step, n), (pos, step, n)
        nxt = pos + n_out * step - n * ONE
        assert pl.resample_advance((pos, step), n) == nxt == rm.advance(pos, step, n), (pos, step, n)
        if pos >= n * ONE:  # no output: the position is only reduced
            assert n_out == 0 and nxt == pos - n * ONE
        elif pos < step:
            assert 0 <= nxt < step
    # step 0: the packet is not resampled
    assert pl.resample_count((7, 0), 1234) == 1234 and pl.resample_advance((7, 0), 1234) == 7


def test_resample_step_against_its_restatement():
    for r in (0.5, 1.0, 2.0, 8.37 / 8, 7.2 / 8, 9.3 / 8, 0.4999999, 2.0000001, 0.0, -1.0, 3.0, 1e300, float("nan"), float("inf"), float("-inf")):
        assert pl.resample_step(r) == rm.step_word(r), r
    assert pl.resample_step(0.5) == 1 << 31 and pl.resample_step(1.0) == ONE and pl.resample_step(2.0) == 1 << 33
    assert pl.resample_step(8.37 / 8) == int(8.37 / 8 * 2.0 ** 32)
    for r in (0.4999999, 2.0000001, 0.0, -1.0, float("nan"), float("inf")):
        assert pl.resample_step(r) == 0, r


def test_resample_apply_refuses_what_the_entry_refuses():
    L = pl.load()
    x, y, h = np.zeros(64, np.float32), np.zeros(256, np.float32), np.zeros(6, np.float32)
    ok = pl.Resample(0, ONE, 0, 0)
    assert L.psk_soft_resample_apply(ctypes.byref(ok), None, x.ctypes.data, 32, y.ctypes.data, None) == 0
    assert L.psk_soft_resample_apply(ctypes.byref(ok), None, None, 0, None, h.ctypes.data) == 0
    assert L.psk_soft_resample_apply(None, None, x.ctypes.data, 32, y.ctypes.data, None) == 1
    assert L.psk_soft_resample_apply(ctypes.byref(ok), None, None, 32, y.ctypes.data, None) == 1
    assert L.psk_soft_resample_apply(ctypes.byref(ok), None, x.ctypes.data, 32, None, None) == 1
    for bad in (pl.Resample(0, 0, 0, 0), pl.Resample(0, (1 << 31) - 1, 0, 0), pl.Resample(0, (1 << 33) + 1, 0, 0),
                pl.Resample((1 << 33) + 1, ONE, 0, 0), pl.Resample(0, ONE, 0, 1), pl.Resample(0, ONE, 2, 0)):
        assert L.psk_soft_resample_apply(ctypes.byref(bad), None, x.ctypes.data, 32, y.ctypes.data, None) == 1
    assert L.psk_soft_resample_apply(ctypes.byref(ok), None, x.ctypes.data, 1 << 30, y.ctypes.data, None) == 1


# ---- the entry on a control-plane-only handle ----------------------------------------------------------------------------------

def _resamples(n, k):
    """every fourth packet not resampled; the others at steps across the range, positions below the step"""
    out = []
    for i in range(n):
        step = (0, 1 << 31, int(8.37 / 8 * 2.0 ** 32), 1 << 33)[i % 4] if i % 8 < 4 else (0, ONE + 1, ONE - 1, int(1.3 * 2.0 ** 32))[i % 4]
        out.append(pl.Resample((i * 0x9E3779B1 + k) % step if step else 12345, step, pl.RS_RESTART if (i + k) % 3 == 0 else 0, 0))
    return out


@pytest.mark.parametrize("fmt", (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8, pl.FORMAT_CF16))
def test_counts_sri_warnings_stats_and_peek_equal_the_call_on_n_out_samples(fmt):
    cfgs = _table()
    C = len(cfgs)
    ref, got, null, tuned = _handle(cfgs), _handle(cfgs), _handle(cfgs), _handle(cfgs)
    for h in (ref, got, null, tuned):
        h.set_option(pl.Handle.OPT_QUALITY, 1)
    tunes = [(0, 0) if i % 3 == 0 else (i * 0x9E3779B97F4A7C15 % (1 << 64), 977 * i) for i in range(C)]
    for k in range(2):
        pk, out_g = _packets(cfgs, fmt, k, odd=True)
        _, out_r = _packets(cfgs, fmt, k, odd=True)
        _, out_n = _packets(cfgs, fmt, k, odd=True)
        _, out_t = _packets(cfgs, fmt, k, odd=True)
        if k == 1:
            pk[3].present = 0
            pk[4].sri_mode = 0
            pk[5].n_floats = 1  # (no samples)
        rs = _resamples(C, k)
        # the contract's packets: CF32, n_out samples, the sample period scaled; absent, mode-0 and empty packets as they are
        want = (pl.Packet * C)()
        for i in range(C):
            ctypes.memmove(ctypes.byref(want[i]), ctypes.byref(pk[i]), ctypes.sizeof(pl.Packet))
            if rs[i].step and pk[i].present and pk[i].sri_mode == 1 and pk[i].n_floats >= 2:
                want[i].n_floats = 2 * rm.count(rs[i].pos, rs[i].step, int(pk[i].n_floats) // 2)
                want[i].sri_xdelta = pk[i].sri_xdelta * (rs[i].step * 2.0 ** -32)
                want[i].format = pl.FORMAT_CF32
        assert any(want[i].n_floats != pk[i].n_floats for i in range(C))
        ref.process_device(0, want, out_r)
        strides = [1 if i % 2 else 7 for i in range(C)]
        got.process_device_resampled(0, pk, strides, tunes, rs, out_g)
        assert _results(out_g) == _results(out_r), k
        assert got.stats() == ref.stats() and _peeks(got) == _peeks(ref)
        # resample == NULL is the tuned entry
        null.process_device_resampled(0, pk, strides, tunes, None, out_n)
        tuned.process_device_tuned(0, pk, strides, tunes, out_t)
        assert _results(out_n) == _results(out_t) and null.stats() == tuned.stats() and _peeks(null) == _peeks(tuned)
    assert got.channel_stats() == ref.channel_stats()
    assert bytes(got.quality_records()) == bytes(ref.quality_records())
    assert bytes(null.quality_records()) == bytes(tuned.quality_records())
    # a control-plane-only handle keeps zeros
    got.set_resample_history(1, [1, 2, 3, 4, 5, 6])
    assert got.resample_history(1).tolist() == [0.0] * 6
    for h in (ref, got, null, tuned):
        h.close()


def test_each_refusal_returns_invalid_arg_and_changes_nothing():
    cfgs = _table()[::5]
    C = len(cfgs)
    h, fresh = _handle(cfgs), _handle(cfgs)
    L = pl.load()
    good = pl.Resample(17, int(1.05 * 2.0 ** 32), 0, 0)
    bad = {
        "step": [pl.Resample(0, (1 << 31) - 1, 0, 0), pl.Resample(0, (1 << 33) + 1, 0, 0), pl.Resample(0, 1, 0, 0), pl.Resample(0, (1 << 64) - 1, 0, 0)],
        "position": [pl.Resample((1 << 33) + 1, ONE, 0, 0)],
        "pad": [pl.Resample(0, ONE, 0, 1)],
        "flag": [pl.Resample(0, ONE, 2, 0), pl.Resample(0, ONE, pl.RS_RESTART | 0x80000000, 0)],
    }
    for k in range(2):
        pk, out = _packets(cfgs, pl.FORMAT_CS16, k)
        before = (_peeks(h), _queries(h), h.stats())

        def refused(pkts, strides, rs, word):
            arr = (pl.Resample * C)(*rs)
            st = None if strides is None else (ctypes.c_uint64 * C)(*strides)
            assert L.psk_soft_process_device_resampled(h._h, 0, C, pkts, st, None, arr, out, None) == 1, word
            assert word.encode() in L.psk_soft_last_error(), (word, L.psk_soft_last_error())
            with pytest.raises(pl.PskSoftError) as ei:
                h.process_device_resampled(0, pkts, strides, None, rs, out)
            assert ei.value.status == 1
            assert (_peeks(h), _queries(h), h.stats()) == before, word

        for word, rss in bad.items():
            for r in rss:
                refused(pk, None, [good] * 4 + [r] + [good] * (C - 5), word)
        # 2^30 samples or more
        long_pk, _ = _packets(cfgs, pl.FORMAT_CS16, k)
        long_pk[2].n_floats = 2 << 30
        refused(long_pk, None, [good] * C, "samples")
        # the strided entry's own: a stride of 0
        refused(pk, [1] * 4 + [0] + [1] * (C - 5), [good] * C, "stride")
        # the limits themselves pass, an absent packet or one with step 0 is not looked at, and the sequence goes on as a fresh one
        edge = [pl.Resample(1 << 33, 1 << 33, pl.RS_RESTART, 0), pl.Resample(0, 1 << 31, 0, 0), pl.Resample(1 << 33, 0, 77, 5)] + [good] * (C - 3)
        pk[3].present = 0
        edge[3] = pl.Resample(1 << 40, 5, 9, 9)
        h.process_device_resampled(0, pk, [5] * C, None, edge, out)
        want = (pl.Packet * C)()
        for i in range(C):
            ctypes.memmove(ctypes.byref(want[i]), ctypes.byref(pk[i]), ctypes.sizeof(pl.Packet))
            if edge[i].step and pk[i].present:
                want[i].n_floats = 2 * rm.count(edge[i].pos, edge[i].step, int(pk[i].n_floats) // 2)
                want[i].sri_xdelta = pk[i].sri_xdelta * (edge[i].step * 2.0 ** -32)
                want[i].format = pl.FORMAT_CF32
        _, out_f = _packets(cfgs, pl.FORMAT_CS16, k)
        fresh.process_device(0, want, out_f)
        assert _results(out) == _results(out_f) and _peeks(h) == _peeks(fresh) and h.stats() == fresh.stats()
    with pytest.raises(ValueError):
        h.process_device_resampled(0, pk, None, None, [good] * (C - 1), out)
    h.close()
    fresh.close()


# ---- what it is for ------------------------------------------------------------------------------------------------------------

def _signal(M, sps, n_sym=3000, seed=1):
    """n_sym symbols at sps samples a symbol: sample k lies f = frac(k / sps) into symbol floor(k / sps); the pulse of
    stimulus.pulse_shape evaluated at the fractional instant f * sps, phase offset 0.3, sigma 0.01"""
    g = np.random.default_rng(seed)
    sym = g.integers(0, M, n_sym)
    n = int(math.floor(n_sym * sps))
    u = np.arange(n, dtype=np.float64) / sps
    j = np.floor(u).astype(np.int64)
    f = u - j
    amp = 0.2 + 0.8 * np.sin(np.pi * (f * sps + 0.9) / (sps + 1.3))
    x = amp * np.exp(1j * (2 * np.pi * sym[j] / M + 0.3)) + 0.01 * (g.standard_normal(n) + 1j * g.standard_normal(n))
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = x.real, x.imag
    return sym, iq


def _decision_errors(soft, sym, M, lag):
    """(wrong, compared): differential decisions of consecutive soft symbols, the first 200 skipped, against the transmitted
    differential symbols `lag` further on"""
    z = soft[0::2].astype(np.float64) + 1j * soft[1::2]
    d = np.rint(np.angle(z[1:] * np.conj(z[:-1])) * M / (2 * np.pi)).astype(np.int64) % M
    tx = (sym[1:] - sym[:-1]) % M
    idx = np.arange(200, d.size)
    ok = (idx + lag >= 0) & (idx + lag < tx.size)
    return int(np.sum(d[idx[ok]] != tx[idx[ok] + lag])), int(ok.sum())


@pytest.mark.parametrize("sps", [8.37, 7.2, 9.3])
@pytest.mark.parametrize("M", [4, 8])
def test_a_symbol_rate_that_does_not_divide_the_sample_rate(oracle_mod, M, sps):
    """3000 symbols at 8.37 / 7.2 / 9.3 samples a symbol, samplesPerBaud 8: the oracle on the raw packet emits a symbol count
    far from 2901 and gets more than 1000 differential decisions wrong at its best alignment; behind psk_soft_resample_apply
    with resample_step(sps / 8) it emits exactly 2901 symbols with no wrong decision in 2700."""
    sym, iq = _signal(M, sps)

    def soft(data):
        o = oracle_mod.OracleComponent()
        o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = 8, M, 100, 50
        return o.service(data, 0.01, sriChanged=True).soft

    raw = soft(iq)
    best = min(_decision_errors(raw, sym, M, lag)[0] for lag in range(-5, 141))
    y, _ = pl.resample_apply((0, pl.resample_step(sps / 8), pl.RS_RESTART), iq)
    res = soft(y)
    wrong, compared = _decision_errors(res, sym, M, 0)
    print("M %d sps %.2f: raw %d symbols, %d wrong at the best lag; resampled %d symbols, %d wrong of %d" %
          (M, sps, raw.size // 2, best, res.size // 2, wrong, compared))
    assert abs(raw.size // 2 - 2901) > 100
    assert best > 1000
    assert res.size // 2 == 2901
    assert compared == 2700 and wrong == 0
