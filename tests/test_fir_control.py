"""Filtered packets without a GPU: the host-side helpers (psk_soft_fir_count / _advance / _apply) against tests/fir_model.py, the
entry on control-plane-only handles (PSK_SOFT_DEVICE_NONE) -- it checks, then plans and counts on n_out samples and the scaled
sample period --, and what the filter is for: the demodulator picks one sample per symbol, and a matched filter in front puts
the whole symbol's energy into it (through the oracle)."""
import ctypes

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests import fir_model as fm
from tests import resample_model as rm
from tests.test_resample_control import _decision_errors, _same, _samples
from tests.test_strided_control import _handle, _packets, _peeks, _queries, _results, _table

U32 = np.uint32
ONE = 1 << 32
NEW = ("psk_soft_fir_define", "psk_soft_process_device_filtered", "psk_soft_fir_get_history", "psk_soft_fir_set_history",
       "psk_soft_fir_count", "psk_soft_fir_advance", "psk_soft_fir_apply", "psk_soft_fir_piece")


def test_the_symbols_are_exported_and_the_abi_version_stays():
    L = pl.load()
    for name in NEW:
        assert name in pl.EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    F = pl.Fir
    assert ctypes.sizeof(F) == 16 and (F.filter.offset, F.decim.offset, F.pos.offset, F.flags.offset) == (0, 4, 8, 12)
    assert (pl.FIR_MAX_TAPS, pl.FIR_SLOTS, pl.FIR_MAX_DECIM, pl.FIR_RESTART) == (128, 64, 16, 1)
    assert ctypes.sizeof(pl.Packet) == 32 and ctypes.sizeof(pl.Output) == 104 and ctypes.sizeof(pl.Resample) == 24
    for D in range(1, 17):  # a piece: as many outputs as fit a window of 4096 inputs behind the longest filter's reach; even
        P = pl.fir_piece(D)
        assert P == fm.piece(D) and P % 2 == 0 and (P - 1) * D + 128 <= 4096 < (P + 2) * D + 128, D
    assert pl.fir_piece(0) == 0 and pl.fir_piece(17) == 0


# ---- the definition ----------------------------------------------------------------------------------------------------------

def _taps(rng, T):
    """finite taps around 1 / T, both signs, a zero and a denormal among them"""
    h = (rng.standard_normal(T) * (2.0 / T)).astype(np.float32)
    if T >= 8:
        h[3], h[5] = 0.0, np.array([0x00000011], U32).view(np.float32)[0]
    return h


DP = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (5, 0), (5, 4), (16, 0), (16, 15), (16, 7)]


@pytest.mark.parametrize("T", [1, 2, 3, 8, 33, 127, 128])
def test_fir_apply_equals_the_model_bit_for_bit(T):
    rng = np.random.default_rng(3000 + T)
    h = _taps(rng, T)
    x = _samples(rng, 1000)
    hist = _samples(rng, fm.HIST)
    for D, pos in DP:
        for n in sorted({1, 2, T - 1, T, T + 1, 1000} - {0}):
            for history, restart in ((None, False), (hist, False), (hist, True)):
                got, gh = pl.fir_apply((1, D, pos, int(restart)), h, x[: 2 * n], history)
                want, wh = fm.apply(h, D, pos, x[: 2 * n], history, restart)
                assert got.size == 2 * fm.count(pos, D, n) == 2 * pl.fir_count((1, D, pos), n)
                assert _same(got, want), (D, pos, n, np.flatnonzero(got.view(U32) != want.view(U32))[:5])
                assert _same(gh, wh)
                # the new history: the last 127 of (old history || the packet)
                old = np.zeros(2 * fm.HIST, np.float32) if history is None or restart else history
                assert _same(gh, np.concatenate([old, x[: 2 * n]])[-2 * fm.HIST:])
    # an odd last element is dropped; no sample is a null call that leaves the history as it was
    assert _same(pl.fir_apply((1, 2, 1), h, x[:15], hist)[0], fm.apply(h, 2, 1, x[:14], hist)[0])
    y, gh = pl.fir_apply((1, 3, 2), h, x[:0], hist)
    assert y.size == 0 and _same(gh, hist)
    # a packet with samples but no output (pos >= n) still moves the history
    y, gh = pl.fir_apply((1, 16, 9), h, x[:10], hist)
    assert y.size == 0 and _same(gh, np.concatenate([hist, x[:10]])[-2 * fm.HIST:])


@pytest.mark.parametrize("D", [1, 2, 3, 5, 16])
def test_a_stream_cut_into_packets_gives_the_bytes_of_the_whole(D):
    """packets of random lengths, 1-sample packets and packets shorter than the filter among them; pos carried by
    psk_soft_fir_advance, the history by hist_out"""
    rng = np.random.default_rng(40 + D)
    T = (33, 128, 8, 127, 2)[D % 5]
    h = _taps(rng, T)
    cuts = [1, 1, 2, T - 1, 1, T, T + 1, 700, 0, 3, 1] + [int(v) for v in rng.integers(1, 400, 12)]
    n = sum(cuts)
    x = _samples(rng, n)
    pos0 = D - 1
    whole, whole_h = pl.fir_apply((1, D, pos0, pl.FIR_RESTART), h, x)
    m = fm.Stream(pos0)
    pos, hist, at, parts = pos0, None, 0, []
    for k, ln in enumerate(cuts):
        part = x[2 * at: 2 * (at + ln)]
        y, hist = pl.fir_apply((1, D, pos, pl.FIR_RESTART if k == 0 else 0), h, part, hist)
        want = m.push(h, D, part, restart=(k == 0))
        assert _same(y, want) and _same(hist, m.history), (k, ln)
        pos = pl.fir_advance((1, D, pos), ln)
        assert pos == m.pos and pos < D
        parts.append(y)
        at += ln
    assert at == n and _same(np.concatenate(parts), whole) and _same(hist, whole_h)


def test_a_filter_changed_in_mid_stream():
    """the history holds 127 samples whatever the filter's length: 8 taps, then 128, then 3 at another decimation give, packet
    for packet, what each filter gives on the whole stream up to there"""
    rng = np.random.default_rng(77)
    x = _samples(rng, 900)
    legs = [(_taps(rng, 8), 2, 300), (_taps(rng, 128), 1, 1), (_taps(rng, 128), 1, 299), (_taps(rng, 3), 3, 300)]
    m = fm.Stream(1)
    pos, hist, at = 1, None, 0
    for h, D, ln in legs:
        pos = min(pos, D - 1)  # (a new decimation: the caller picks its phase anew)
        m.pos = pos
        part = x[2 * at: 2 * (at + ln)]
        y, hist = pl.fir_apply((1, D, pos), h, part, hist)
        assert _same(y, m.push(h, D, part)) and _same(hist, m.history)
        # ... and that is the filter run over everything so far (at least 127 samples of it, once the stream is that long)
        full, _ = pl.fir_apply((1, 1, 0, pl.FIR_RESTART), h, x[: 2 * (at + ln)])
        assert _same(y, full.reshape(-1, 2)[at + pos: at + ln: D].reshape(-1)), (D, ln)
        pos = pl.fir_advance((1, D, pos), ln)
        at += ln


def test_count_and_advance_against_big_integers():
    rng = np.random.default_rng(3)
    cases = [(0, 1, 0), (0, 1, 1), (0, 16, 1), (15, 16, 1), (15, 16, 15), (15, 16, 16), (15, 16, 17), (2, 3, 2), (2, 3, 3),
             (0, 1, (1 << 30) - 1), (15, 16, (1 << 30) - 1), (4, 5, 1 << 40), (0, 7, (1 << 63) + 12345)]
    for _ in range(400):
        D = int(rng.integers(1, 17))
        cases.append((int(rng.integers(0, D)), D, int(rng.integers(0, 1 << int(rng.integers(1, 62))))))
    for pos, D, n in cases:
        n_out = 0 if pos >= n else -(-(n - pos) // D)
        assert (not n_out or pos + (n_out - 1) * D < n) and pos + n_out * D >= n
        assert pl.fir_count((1, D, pos), n) == n_out == fm.count(pos, D, n), (pos, D, n)
        nxt = pos + n_out * D - n
        assert pl.fir_advance((1, D, pos), n) == nxt == fm.advance(pos, D, n), (pos, D, n)
        if pos >= n:  # no output: the position is only reduced
            assert n_out == 0 and nxt == pos - n
        assert 0 <= nxt < D
    # filter 0: the packet is not filtered
    assert pl.fir_count((0, 4, 3), 1234) == 1234 and pl.fir_advance((0, 4, 3), 1234) == 3


def test_the_two_identities():
    rng = np.random.default_rng(5)
    n = 4097
    x = _samples(rng, n)
    hist = _samples(rng, fm.HIST)
    # {1.0f}, D = 1: the packet itself, bit for bit, denormals and the sign of zero included
    y, gh = pl.fir_apply((1, 1, 0), [1.0], x, hist)
    assert _same(y, x) and _same(gh, x[-2 * fm.HIST:])
    assert np.count_nonzero(np.signbit(y) & (y == 0)) >= 2
    # {0, 0, 1}: the stream delayed by two samples, but for the sign of a zero sample
    pz = lambda v: np.where(v == 0, np.float32(0), v).astype(np.float32)  # noqa: E731
    y, _ = pl.fir_apply((1, 1, 0, pl.FIR_RESTART), [0.0, 0.0, 1.0], x)
    assert y.size == 2 * n and not y[:4].any() and _same(pz(y[4:]), pz(x[: 2 * (n - 2)]))
    assert np.count_nonzero(y[4:]) == np.count_nonzero(x[: 2 * (n - 2)]) > 2 * n - 20
    # ... and with a history the delay line runs on across the packets' seam
    y2, _ = pl.fir_apply((1, 1, 0), [0.0, 0.0, 1.0], x[:400], hist)
    assert _same(pz(y2[:4]), pz(hist[-4:])) and _same(pz(y2[4:]), pz(x[:396]))
    # decimated: every D-th of them
    y3, _ = pl.fir_apply((1, 3, 2), [1.0], x, hist)
    assert _same(y3, x.reshape(-1, 2)[2::3].reshape(-1))


def test_fir_apply_refuses_what_the_entry_refuses():
    L = pl.load()
    x, y, h = np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros(254, np.float32)
    t = np.ones(128, np.float32)
    ok = pl.Fir(1, 2, 1, 0)

    def call(f, taps, nt, hin, xin, n, out, hout):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.psk_soft_fir_apply(None if f is None else ctypes.byref(f), p(taps), nt, p(hin), p(xin), n, p(out), p(hout))

    assert call(ok, t, 128, None, x, 32, y, None) == 0
    assert call(ok, t, 1, h, None, 0, None, h) == 0
    assert call(pl.Fir(0, 16, 15, 1), t, 8, None, x, 32, y, None) == 0  # (f->filter is not looked at)
    assert call(None, t, 8, None, x, 32, y, None) == 1
    assert call(ok, None, 8, None, x, 32, y, None) == 1
    assert call(ok, t, 8, None, None, 32, y, None) == 1
    assert call(ok, t, 8, None, x, 32, None, None) == 1
    assert call(ok, t, 0, None, x, 32, y, None) == 1
    assert call(ok, t, 129, None, x, 32, y, None) == 1
    for bad in (pl.Fir(1, 0, 0, 0), pl.Fir(1, 17, 0, 0), pl.Fir(1, 2, 2, 0), pl.Fir(1, 1, 1, 0), pl.Fir(1, 2, 1, 2)):
        assert call(bad, t, 8, None, x, 32, y, None) == 1
    assert call(ok, t, 8, None, x, 1 << 30, y, None) == 1


# ---- the entry on a control-plane-only handle ----------------------------------------------------------------------------------

SLOT_TAPS = {0: 8, 1: 128, 5: 1, 63: 33}


def _define(h):
    for slot, T in SLOT_TAPS.items():
        h.fir_define(slot, np.full(T, 1.0 / T, np.float32))


def _firs(n, k):
    """every fourth packet not filtered (junk in the other fields); the others across the slots and decimations"""
    out = []
    slots = sorted(SLOT_TAPS)
    for i in range(n):
        if i % 4 == 0:
            out.append(pl.Fir(0, 99, 1234, 0xFFFF))
            continue
        D = (1, 2, 3, 5, 16, 8)[(i // 4 + i) % 6]
        out.append(pl.Fir(1 + slots[i % 4], D, (i * 7 + k) % D, pl.FIR_RESTART if (i + k) % 3 == 0 else 0))
    return out


def _resamples(n, k):
    """every third packet resampled: 8.37 / 8, and the limits of the step"""
    out = []
    for i in range(n):
        step = (int(8.37 / 8 * 2.0 ** 32), 1 << 31, 1 << 33, ONE + 1)[(i // 3) % 4] if i % 3 == 1 else 0
        out.append(pl.Resample((i * 0x9E3779B1 + k) % step if step else 5, step, 0, 0))
    return out


def _contract_packets(pk, firs, rs):
    """the contract's packets, for the resampled entry: CF32, the filter's n_out samples, the sample period times D; absent,
    mode-0 and empty packets as they are"""
    C = len(firs)
    want = (pl.Packet * C)()
    for i in range(C):
        ctypes.memmove(ctypes.byref(want[i]), ctypes.byref(pk[i]), ctypes.sizeof(pl.Packet))
        if firs[i].filter and pk[i].present and pk[i].sri_mode == 1 and pk[i].n_floats >= 2:
            want[i].n_floats = 2 * fm.count(firs[i].pos, firs[i].decim, int(pk[i].n_floats) // 2)
            want[i].sri_xdelta = pk[i].sri_xdelta * float(firs[i].decim)
            want[i].format = pl.FORMAT_CF32
    return want


@pytest.mark.parametrize("fmt", (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8, pl.FORMAT_CF16))
def test_counts_sri_warnings_stats_and_peek_equal_the_resampled_call_on_n_out_samples(fmt):
    cfgs = _table()
    C = len(cfgs)
    ref, got, null, rsd = _handle(cfgs), _handle(cfgs), _handle(cfgs), _handle(cfgs)
    for h in (ref, got, null, rsd):
        h.set_option(pl.Handle.OPT_QUALITY, 1)
    _define(got)
    tunes = [(0, 0) if i % 3 == 0 else (i * 0x9E3779B97F4A7C15 % (1 << 64), 977 * i) for i in range(C)]
    for k in range(2):
        pk, out_g = _packets(cfgs, fmt, k, odd=True)
        _, out_r = _packets(cfgs, fmt, k, odd=True)
        _, out_n = _packets(cfgs, fmt, k, odd=True)
        _, out_t = _packets(cfgs, fmt, k, odd=True)
        if k == 1:
            pk[3].present = 0
            pk[5].sri_mode = 0
            pk[6].n_floats = 1  # (no samples)
            pk[7].n_floats = 2  # (one sample at D = 16 and pos 15: no output)
        firs, rs = _firs(C, k), _resamples(C, k)
        if k == 1:
            firs[7] = pl.Fir(2, 16, 15, 0)
        want = _contract_packets(pk, firs, rs)
        assert any(want[i].n_floats != pk[i].n_floats for i in range(C))
        assert any(firs[i].filter and rs[i].step for i in range(C)) and any(firs[i].filter and not rs[i].step for i in range(C))
        ref.process_device_resampled(0, want, None, None, rs, out_r)
        strides = [1 if i % 2 else 7 for i in range(C)]
        got.process_device_filtered(0, pk, strides, tunes, firs, rs, out_g)
        assert _results(out_g) == _results(out_r), k
        assert got.stats() == ref.stats() and _peeks(got) == _peeks(ref)
        # the sample period: times D, and D x step with a resampler
        for i in range(C):
            if firs[i].filter and out_g[i].sri_pushed and pk[i].present and pk[i].sri_mode == 1 and want[i].n_floats >= 2:
                S = cfgs[i][0]
                x = 0.01 * float(firs[i].decim)
                x = x * (rs[i].step * 2.0 ** -32) if rs[i].step else x
                assert out_g[i].sri_soft_xdelta == x * S, (i, out_g[i].sri_soft_xdelta, x, S)
        # fir == NULL is the resampled entry
        null.process_device_filtered(0, pk, strides, tunes, None, rs, out_n)
        rsd.process_device_resampled(0, pk, strides, tunes, rs, out_t)
        assert _results(out_n) == _results(out_t) and null.stats() == rsd.stats() and _peeks(null) == _peeks(rsd)
    assert got.channel_stats() == ref.channel_stats()
    assert bytes(got.quality_records()) == bytes(ref.quality_records())
    assert bytes(null.quality_records()) == bytes(rsd.quality_records())
    # a control-plane-only handle keeps zeros
    got.set_fir_history(1, np.arange(254))
    assert not got.fir_history(1).any()
    for h in (ref, got, null, rsd):
        h.close()


def test_each_refusal_returns_invalid_arg_and_changes_nothing():
    cfgs = _table()[::5]
    C = len(cfgs)
    h, fresh = _handle(cfgs), _handle(cfgs)
    L = pl.load()
    # the refusals of psk_soft_fir_define
    t = np.ones(129, np.float32)
    assert L.psk_soft_fir_define(h._h, 0, t.ctypes.data, 0) == 1
    assert L.psk_soft_fir_define(h._h, 0, t.ctypes.data, 129) == 1
    assert L.psk_soft_fir_define(h._h, 0, None, 8) == 1
    assert L.psk_soft_fir_define(h._h, 64, t.ctypes.data, 8) == 1
    assert L.psk_soft_fir_define(None, 0, t.ctypes.data, 8) == 1
    with pytest.raises(pl.PskSoftError):
        h.fir_define(0, [])
    good = pl.Fir(1, 2, 1, 0)
    for k in range(2):
        pk, out = _packets(cfgs, pl.FORMAT_CS16, k)
        before = (_peeks(h), _queries(h), h.stats())

        def refused(pkts, strides, firs, rs, word):
            arr = (pl.Fir * C)(*firs)
            st = None if strides is None else (ctypes.c_uint64 * C)(*strides)
            ra = None if rs is None else (pl.Resample * C)(*rs)
            assert L.psk_soft_process_device_filtered(h._h, 0, C, pkts, st, None, arr, ra, out, None) == 1, word
            assert word.encode() in L.psk_soft_last_error(), (word, L.psk_soft_last_error())
            with pytest.raises(pl.PskSoftError) as ei:
                h.process_device_filtered(0, pkts, strides, None, firs, rs, out)
            assert ei.value.status == 1
            assert (_peeks(h), _queries(h), h.stats()) == before, word

        if k == 0:  # no slot is defined yet: every filter is refused
            refused(pk, None, [good] * C, None, "slot")
            _define(h)
        bad = {
            "slot": [pl.Fir(65, 1, 0, 0), pl.Fir(3, 1, 0, 0), pl.Fir(0xFFFFFFFF, 1, 0, 0)],
            "decimation": [pl.Fir(1, 0, 0, 0), pl.Fir(1, 17, 0, 0), pl.Fir(1, 0xFFFFFFFF, 0, 0)],
            "position": [pl.Fir(1, 1, 1, 0), pl.Fir(1, 16, 16, 0)],
            "flag": [pl.Fir(1, 2, 0, 2), pl.Fir(1, 2, 0, pl.FIR_RESTART | 0x80000000)],
        }
        for word, fs in bad.items():
            for f in fs:
                refused(pk, None, [good] * 4 + [f] + [good] * (C - 5), None, word)
        # 2^30 samples or more
        long_pk, _ = _packets(cfgs, pl.FORMAT_CS16, k)
        long_pk[2].n_floats = 2 << 30
        refused(long_pk, None, [good] * C, None, "samples")
        # what the resampled entry refuses: a step outside its range, a stride of 0
        refused(pk, None, [good] * C, [pl.Resample(0, 0, 0, 0)] * 4 + [pl.Resample(0, 5, 0, 0)] + [pl.Resample(0, 0, 0, 0)] * (C - 5), "step")
        refused(pk, [1] * 4 + [0] + [1] * (C - 5), [good] * C, None, "stride")
        # the limits themselves pass, an absent packet or one with filter 0 is not looked at, and the sequence goes on as a fresh one
        edge = [pl.Fir(64, 16, 15, pl.FIR_RESTART), pl.Fir(2, 1, 0, 0), pl.Fir(0, 77, 99, 5)] + [good] * (C - 3)
        pk[3].present = 0
        edge[3] = pl.Fir(99, 0, 9, 9)
        h.process_device_filtered(0, pk, [5] * C, None, edge, None, out)
        want = _contract_packets(pk, edge, None)
        _, out_f = _packets(cfgs, pl.FORMAT_CS16, k)
        fresh.process_device(0, want, out_f)
        assert _results(out) == _results(out_f) and _peeks(h) == _peeks(fresh) and h.stats() == fresh.stats()
    with pytest.raises(ValueError):
        h.process_device_filtered(0, pk, None, None, [good] * (C - 1), None, out)
    h.close()
    fresh.close()


# ---- what it is for ------------------------------------------------------------------------------------------------------------

def _signal(M, sigma):
    """6000 symbols, each repeated 8 times at unit amplitude (a rectangular pulse), phase offset 0.3, white noise of `sigma` a
    component"""
    g = np.random.default_rng(3)
    sym = g.integers(0, M, 6000)
    s = np.repeat(np.exp(1j * (2 * np.pi * sym / M + 0.3)), 8)
    n = s.size
    x = s + sigma * (g.standard_normal(n) + 1j * g.standard_normal(n))
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = x.real, x.imag
    return sym, iq


def _wrong(oracle_mod, data, S, sym, M):
    """wrong differential decisions of 5700, at the best lag of -3 .. 3, of the oracle's soft symbols of `data`"""
    o = oracle_mod.OracleComponent()
    o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = S, M, 100, 50
    soft = o.service(data, 0.01, sriChanged=True).soft
    res = [_decision_errors(soft, sym, M, lag) for lag in range(-3, 4)]
    wrong, compared = min(res)
    assert compared == 5700, res
    return wrong


def test_a_matched_filter_in_front_of_the_demodulator(oracle_mod):
    """QPSK and 8-PSK at 8 samples a symbol in noise of sigma 0.3: the demodulator picks one sample of eight per symbol and gets
    hundreds of differential decisions wrong; behind eight taps of 1/8 it gets none (QPSK).  Decimated by 2 to samplesPerBaud
    4 the phase decides: pos 1 keeps the triangle's peak, pos 0 puts two equal samples either side of it and the timing pick
    flips between them."""
    box = np.full(8, 0.125, np.float32)
    sym, iq = _signal(4, 0.3)
    raw = _wrong(oracle_mod, iq, 8, sym, 4)
    y, _ = pl.fir_apply((1, 1, 0, pl.FIR_RESTART), box, iq)
    mf = _wrong(oracle_mod, y, 8, sym, 4)
    y1, _ = pl.fir_apply((1, 2, 1, pl.FIR_RESTART), box, iq)
    d1 = _wrong(oracle_mod, y1, 4, sym, 4)
    y0, _ = pl.fir_apply((1, 2, 0, pl.FIR_RESTART), box, iq)
    d0 = _wrong(oracle_mod, y0, 4, sym, 4)
    sym8, iq8 = _signal(8, 0.3)
    raw8 = _wrong(oracle_mod, iq8, 8, sym8, 8)
    y8, _ = pl.fir_apply((1, 1, 0, pl.FIR_RESTART), box, iq8)
    mf8 = _wrong(oracle_mod, y8, 8, sym8, 8)
    print("QPSK: raw %d, filtered %d, D = 2 pos 1 %d, pos 0 %d; 8-PSK: raw %d, filtered %d (of 5700)" % (raw, mf, d1, d0, raw8, mf8))
    assert raw > 300
    assert mf == 0
    assert d1 == 0
    assert d0 > 1000
    assert raw8 > 1500 and mf8 < 100
