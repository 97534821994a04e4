"""Tuned packets without a GPU: the host-side helpers (psk_soft_tune_step / _advance / _apply) against tests/tune_model.py, the
entry on control-plane-only handles (PSK_SOFT_DEVICE_NONE) -- it checks, then plans and counts like the strided entry --, and what
the shift is for: a carrier offset the phase tracker of the reference cannot follow, taken out in front of it (through the oracle)."""
import ctypes
import math

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests import tune_model as tm
from tests.test_strided_control import _handle, _packets, _peeks, _queries, _results, _table

U32 = np.uint32


def test_the_symbols_are_exported_and_the_abi_version_stays():
    L = pl.load()
    for name in ("psk_soft_process_device_tuned", "psk_soft_tune_step", "psk_soft_tune_advance", "psk_soft_tune_apply"):
        assert name in pl.EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    assert ctypes.sizeof(pl.Tune) == 16 and pl.Tune.phase.offset == 0 and pl.Tune.step.offset == 8
    assert ctypes.sizeof(pl.Packet) == 32 and ctypes.sizeof(pl.Output) == 104 and ctypes.sizeof(pl.Stats) == 96


# ---- the definition ----------------------------------------------------------------------------------------------------------

def test_the_phasor_tables_of_the_model():
    C, F = tm.tables()
    assert C[0].tolist() == [1.0, 0.0] and F[0].tolist() == [1.0, 0.0]
    wr, wi = tm.phasors(0, 0, 3)
    assert wr.tolist() == [1.0] * 3 and wi.tolist() == [0.0] * 3  # W(0) = (1, 0) exactly
    # | |W| - 1 | <= 1.4e-7 and the angle within 3.3e-7 rad of the truncated phase, over random phase words
    rng = np.random.default_rng(7)
    p = rng.integers(0, 1 << 64, 20000, dtype=np.uint64)
    w = np.array([tm.phasors(int(x), 0, 1) for x in p[:4000]], np.float64).reshape(-1, 2)
    assert np.max(np.abs(np.hypot(w[:, 0], w[:, 1]) - 1.0)) <= 1.4e-7
    want = 2.0 * math.pi * (p[:4000] >> np.uint64(44)).astype(np.float64) / 2.0 ** 20
    err = np.angle((w[:, 0] + 1j * w[:, 1]) * np.exp(-1j * want))
    assert np.max(np.abs(err)) <= 3.3e-7


APPLY_CASES = [
    (0x0123456789ABCDEF, 1),
    (0, (1 << 63) + 12345),
    ((1 << 64) - 1, (1 << 64) - 1),
    ((1 << 64) - 1, 1),
    (0, 0),
    (12345, tm.step_word(-0.025)),
    (0xFFFFF00000000000, 1 << 44),  # every sample another fine entry, across the wrap of the phase word
    (0, 1 << 54),                   # every sample another coarse entry
]


@pytest.mark.parametrize("case", range(len(APPLY_CASES) + 6))
def test_tune_apply_equals_the_model_bit_for_bit(case):
    rng = np.random.default_rng(1000 + case)
    if case < len(APPLY_CASES):
        phase, step = APPLY_CASES[case]
    else:
        phase, step = (int(v) for v in rng.integers(0, 1 << 64, 2, dtype=np.uint64))
    n = 20000
    x = (rng.standard_normal(2 * n) * rng.choice([1e-3, 1.0, 300.0], 2 * n)).astype(np.float32)
    x[:8] = [0.0, -0.0, -0.0, 0.0, 1.0, 0.0, 0.0, -1.0]
    x[8:12] = np.array([1, 0x00400000, 0x807FFFFF, 0x00800000], U32).view(np.float32)  # denormals are kept
    got = pl.tune_apply(phase, step, x)
    want = tm.apply(phase, step, x)
    assert got.dtype == np.float32 and got.size == 2 * n
    assert np.array_equal(got.view(U32), want.view(U32)), np.flatnonzero(got.view(U32) != want.view(U32))[:5]
    # an odd last element is dropped; nothing is a null call
    assert np.array_equal(pl.tune_apply(phase, step, x[:7]).view(U32), want[:6].view(U32))
    assert pl.tune_apply(phase, step, x[:1]).size == 0
    # continuing a stream: the second half from the advanced phase word
    half = n // 2 + 1
    p2 = pl.tune_advance(phase, step, half)
    assert p2 == tm.advance(phase, step, half)
    assert np.array_equal(pl.tune_apply(p2, step, x[2 * half :]).view(U32), want[2 * half :].view(U32))


def test_tune_apply_in_place_and_bad_arguments():
    L = pl.load()
    x = np.arange(64, dtype=np.float32)
    want = tm.apply(5 << 50, 3 << 45, x)
    t = pl.Tune(5 << 50, 3 << 45)
    assert L.psk_soft_tune_apply(ctypes.byref(t), x.ctypes.data, 32, x.ctypes.data) == 0
    assert np.array_equal(x.view(U32), want.view(U32))
    assert L.psk_soft_tune_apply(None, x.ctypes.data, 32, x.ctypes.data) == 1
    assert L.psk_soft_tune_apply(ctypes.byref(t), None, 32, x.ctypes.data) == 1
    assert L.psk_soft_tune_apply(ctypes.byref(t), x.ctypes.data, 32, None) == 1
    assert L.psk_soft_tune_apply(ctypes.byref(t), None, 0, None) == 0


def test_tune_step_against_its_restatement():
    for f in (0.025, -0.025, 0.0, -0.0, 1.0, -1e-30, 1e-30, 0.5, -0.5, 123456.75, -3.125, 2.0 ** -64, 1 - 2.0 ** -53, float("nan"),
              float("inf"), float("-inf")):
        assert pl.tune_step(f) == tm.step_word(f), f
    assert pl.tune_step(0.0) == 0 and pl.tune_step(1.0) == 0 and pl.tune_step(float("nan")) == 0
    assert pl.tune_step(-1e-30) == 0  # (r rounds to 1: wraps)
    assert pl.tune_step(0.5) == 1 << 63 and pl.tune_step(-0.25) == 3 << 62
    assert pl.tune_step(0.025) == int(0.025 * 2.0 ** 64)
    # a shift and its inverse cancel to the rounding of 1 - 0.025 in a double: 2^-53 turns, 2^11 units of the step word
    assert min((pl.tune_step(0.025) + pl.tune_step(-0.025)) % (1 << 64), -(pl.tune_step(0.025) + pl.tune_step(-0.025)) % (1 << 64)) <= 2048


def test_tune_advance_wraps():
    M = 1 << 64
    assert pl.tune_advance(0, 0, 12345) == 0
    assert pl.tune_advance(M - 1, 1, 1) == 0
    assert pl.tune_advance(M - 1, M - 1, M - 1) == (M - 1 + (M - 1) * (M - 1)) % M
    assert pl.tune_advance(7, (1 << 63) + 12345, 3) == (7 + 3 * ((1 << 63) + 12345)) % M
    assert pl.tune_advance(1 << 63, 1 << 63, 1) == 0
    assert pl.tune_advance(5, 9, 0) == 5


# ---- the entry on a control-plane-only handle ----------------------------------------------------------------------------------

def _tunes(n, k):
    return [(0, 0) if i % 4 == 0 else ((i * 0x9E3779B97F4A7C15 + k) % (1 << 64), (1 << 64) - 1 - 977 * i) for i in range(n)]


@pytest.mark.parametrize("fmt", (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8, pl.FORMAT_CF16))
def test_counts_sri_warnings_stats_and_peek_equal_the_strided_call(fmt):
    cfgs = _table()
    ref, got, null = _handle(cfgs), _handle(cfgs), _handle(cfgs)
    for h in (ref, got, null):
        h.set_option(pl.Handle.OPT_QUALITY, 1)
    for k in range(2):
        pk, out_r = _packets(cfgs, fmt, k, odd=True)
        _, out_g = _packets(cfgs, fmt, k, odd=True)
        _, out_n = _packets(cfgs, fmt, k, odd=True)
        if k == 1:
            pk[3].present = 0
            pk[4].sri_mode = 0
        strides = [1 if i % 2 else 7 for i in range(len(cfgs))]
        ref.process_device_strided(0, pk, strides, out_r)
        got.process_device_tuned(0, pk, strides, _tunes(len(cfgs), k), out_g)
        null.process_device_tuned(0, pk, None, None, out_n)
        assert _results(out_g) == _results(out_r) and _results(out_n) == _results(out_r), k
        assert got.stats() == ref.stats() and null.stats() == ref.stats()
        assert _peeks(got) == _peeks(ref) and _peeks(null) == _peeks(ref)
    assert got.channel_stats() == ref.channel_stats()
    assert bytes(got.quality_records()) == bytes(ref.quality_records())
    for h in (ref, got, null):
        h.close()


def test_a_stride_of_zero_is_refused_and_changes_nothing():
    cfgs = _table()[::5]
    C = len(cfgs)
    h, fresh = _handle(cfgs), _handle(cfgs)
    L = pl.load()
    for k in range(2):
        pk, out = _packets(cfgs, pl.FORMAT_CS16, k)
        before = (_peeks(h), _queries(h), h.stats())
        for tunes in (None, _tunes(C, k)):
            arr = (ctypes.c_uint64 * C)(*([1] * 4 + [0] + [1] * (C - 5)))
            tn = None if tunes is None else (pl.Tune * C)(*[pl.Tune(p, s) for p, s in tunes])
            assert L.psk_soft_process_device_tuned(h._h, 0, C, pk, arr, tn, out, None) == 1
            assert b"stride" in L.psk_soft_last_error()
            with pytest.raises(pl.PskSoftError):
                h.process_device_tuned(0, pk, [3] * (C - 1) + [(1 << 64) - 1], tunes, out)
            assert (_peeks(h), _queries(h), h.stats()) == before
        h.process_device_tuned(0, pk, [5] * C, _tunes(C, k), out)
        _, out_f = _packets(cfgs, pl.FORMAT_CS16, k)
        fresh.process_device(0, pk, out_f)
        assert _results(out) == _results(out_f) and _peeks(h) == _peeks(fresh) and h.stats() == fresh.stats()
    with pytest.raises(ValueError):
        h.process_device_tuned(0, pk, None, [(1, 1)] * (C - 1), out)
    h.close()
    fresh.close()


# ---- what it is for ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M, offset", [(8, 0.05), (4, 0.1)])
def test_an_offset_the_tracker_cannot_follow_is_taken_out(oracle_mod, M, offset):
    """gen_psk, 8 samples per baud, 600 symbols, a carrier offset of `offset` cycles per symbol: the oracle loses the signal
    (lock < 0.5); after psk_soft_tune_apply with the negated step it holds it (lock > 0.99)."""
    from ref_stimulus import gen_psk

    S, n_sym = 8, 600
    iq, _ = gen_psk(n_sym, S, M)
    x = iq[0::2].astype(np.float64) + 1j * iq[1::2]
    x = x * np.exp(2j * math.pi * (offset / S) * np.arange(x.size))
    off = np.empty(2 * x.size, np.float32)
    off[0::2], off[1::2] = x.real, x.imag

    def lock(data):
        o = oracle_mod.OracleComponent()
        o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = S, M, 100, 50
        r = o.service(data, 0.01, sriChanged=True)
        assert r.soft.size >= 2 * 400
        return tm.lock_of(r.soft, M)

    untuned, tuned = lock(off), lock(pl.tune_apply(0, pl.tune_step(-offset / S), off))
    print("M %d offset %.2f: lock untuned %.4f tuned %.4f" % (M, offset, untuned, tuned))
    assert untuned < 0.5
    assert tuned > 0.99
