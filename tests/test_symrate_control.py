"""psk_soft_symrate_device without a GPU: the exports and the record's layout, the host-side definition (psk_soft_symrate_host) and
derivation (psk_soft_symrate_derive) against tests/symrate_model.py, the entry on control-plane-only handles (PSK_SOFT_DEVICE_NONE)
-- it checks, then leaves planned records and nothing else --, how well the estimate does on the pulses it is meant for, and what
the look is for: a symbol rate that does not divide the sample rate, estimated from the samples and taken out by the resampler in
front of the oracle."""
import ctypes
import math

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import symrate_model as sm
from tests import tune_model as tm
from tests.test_resample_control import _decision_errors, _signal

F32 = np.float32
NEW = ("psk_soft_symrate_device", "psk_soft_get_symrate", "psk_soft_symrate_derive", "psk_soft_symrate_host", "psk_soft_symrate_bytes",
       "psk_soft_symrate_piece")


def test_the_symbols_are_exported_and_the_record_has_its_layout():
    L = pl.load()
    for name in NEW:
        assert name in pl.EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    R = pl.Symrate
    assert ctypes.sizeof(R) == 392 == sm.RECORD_BYTES and L.psk_soft_symrate_bytes() == 392
    names = ("n_samples", "n_used", "n_blocks", "n_valid", "n_pairs", "sum_re", "sum_im", "sum_pow", "sum_lvl", "samplesPerBaud", "flags", "pad")
    assert [getattr(R, k).offset for k in names] == [0, 8, 16, 24, 32, 96, 224, 352, 368, 384, 386, 387]
    D = pl.SymrateDerived
    assert ctypes.sizeof(D) == 40
    assert [getattr(D, k).offset for k in ("samples_per_symbol", "step_ratio", "coherence", "mean_level", "detector", "lags_used")] == [0, 8, 16, 24, 32, 36]
    assert (pl.SR_DATA, pl.SR_TUNED, pl.SR_PLANNED) == (1, 2, 128)
    # the piece is a constant of the library, whole turns of the fold's lanes, and the model's
    assert pl.symrate_piece() == sm.PIECE and sm.PIECE % sm.THREADS == 0 and sm.HALO == max(sm.LAGS)


# ---- the definition ----------------------------------------------------------------------------------------------------------

_TUNE = (0x0123456789ABCDEF, tm.step_word(-0.0137))
# (S, samples): two blocks and one sample more; blocks that are no power of two wide; more than one piece, the halo, a ragged end
# (24, 200 and 257: four, 32 and 64 lanes a block in the device's fold, the last with a ragged last turn -- the model restates them)
SHAPES = ((4, 8), (4, 9), (5, 5 * 131 + 4), (8, 8 * 700 + 7), (33, 33 * 515), (100, 100 * 300 + 99), (1024, 1024 * 3 + 5),
          (24, 24 * 530 + 23), (200, 200 * 140 + 199), (257, 257 * 130 + 3))
KINDS = ("signal", "nonfinite", "huge", "zeros")


def _samples(S, n, kind, seed):
    """interleaved float32: noisy QPSK at 1.04 S samples a symbol with a shaped pulse; `nonfinite` puts +-inf and NaN samples into
    it, `huge` (3e19) overflows every e (no block is valid), `zeros` is all zeros (every block valid, every sum zero)"""
    rng = np.random.default_rng(seed)
    u = np.arange(n) / (1.04 * S)
    amp = 0.2 + 0.8 * np.sin(np.pi * (u - np.floor(u)))
    z = amp * np.exp(2j * math.pi * (rng.integers(0, 4, n)[np.floor(u).astype(int)] / 4 + 0.002 * np.arange(n))) + 0.05 * (
        rng.standard_normal(n) + 1j * rng.standard_normal(n))
    z = z * {"signal": 1.0, "nonfinite": 1.0, "huge": 3e19, "zeros": 0.0}[kind]
    x = np.empty(2 * n, F32)
    x[0::2], x[1::2] = z.real, z.imag
    if kind == "nonfinite":
        for pos, v in ((n // 2, np.inf), (n // 2 + 3, -np.inf), (n // 3, np.nan), (n - 1, np.nan), (S - 1, np.inf)):
            x[2 * (pos % n) + (pos & 1)] = v
    return x


_host_records = {}


def _host_record(S, n, kind, tuned):
    key = (S, n, kind, tuned)
    if key not in _host_records:
        x = _samples(S, n, kind, 31 * n + S)
        tune = _TUNE if tuned else None
        _host_records[key] = (pl.symrate_host(S, x, tune), sm.model_record(x, S, tune), x)
    return _host_records[key]


@pytest.mark.parametrize("tuned", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_symrate_host_against_the_model(kind, tuned):
    for S, n in SHAPES:
        rec, model, _ = _host_record(S, n, kind, tuned)
        ctx = "S %d n %d %s tuned %d" % (S, n, kind, tuned)
        sm.assert_close(rec, model, ctx)
        nb = min(n // S, 4096)
        assert rec.flags == pl.SR_DATA | (pl.SR_TUNED if tuned else 0) and (rec.n_samples, rec.n_blocks, rec.n_used) == (n, nb, nb * S), ctx
        if kind == "huge":
            assert rec.n_valid == 0 and not any(rec.n_pairs) and bytes(rec)[96:384] == bytes(288), ctx
        elif kind in ("signal", "zeros"):
            assert rec.n_valid == nb and list(rec.n_pairs) == [max(0, nb - L) for L in sm.LAGS], ctx
        else:
            assert 0 < rec.n_valid < nb or nb <= 3, ctx
        if kind == "zeros":
            assert bytes(rec)[96:384] == bytes(288), ctx


def test_the_bound_of_the_comparison_sees_one_float32_rounding():
    """a record whose terms were off by one float32 rounding in one block misses assert_close: the bound is the order of additions'"""
    S, n = 8, 8 * 700 + 7
    rec, model, x = _host_record(S, n, "signal", False)
    y = x.copy()
    y[2 * (S * 300 + 3)] = np.nextafter(y[2 * (S * 300 + 3)], F32(4))
    with pytest.raises(AssertionError):
        sm.assert_close(pl.symrate_host(S, y), model, "one ulp")


def test_the_cap_of_4096_blocks():
    S = 4
    x = _samples(S, 4096 * S + S + 3, "signal", 9)
    rec = pl.symrate_host(S, x)
    assert (rec.n_samples, rec.n_used, rec.n_blocks) == (4096 * S + S + 3, 4096 * S, 4096)
    capped = pl.symrate_host(S, x[: 2 * 4096 * S])
    capped.n_samples = rec.n_samples
    assert bytes(capped) == bytes(rec)
    sm.assert_close(rec, sm.model_record(x, S), "cap")


def test_symrate_host_null_tune_zero_tune_and_bad_arguments():
    L = pl.load()
    x = _samples(8, 300, "signal", 5)
    a, b = pl.symrate_host(8, x), pl.symrate_host(8, x, (0, 0))
    assert bytes(a) == bytes(b) and a.flags == pl.SR_DATA
    # an odd last element is dropped; fewer than two blocks is the zero record
    assert bytes(pl.symrate_host(8, x[:-1])) == bytes(pl.symrate_host(8, x[:-2]))
    assert bytes(pl.symrate_host(8, x[: 2 * 15])) == bytes(392) and pl.symrate_host(8, x[: 2 * 16]).n_blocks == 2
    rec = pl.Symrate()
    for S in (0, 1, 3, 1025, 65535):
        assert L.psk_soft_symrate_host(S, None, x.ctypes.data, 100, ctypes.byref(rec)) == 1
    assert L.psk_soft_symrate_host(8, None, None, 100, ctypes.byref(rec)) == 1
    assert L.psk_soft_symrate_host(8, None, x.ctypes.data, 100, None) == 1
    assert L.psk_soft_symrate_derive(None, None) == 1


def _derive_both(rec, ctx):
    got, want = pl.symrate_derive(rec), sm.derive(rec)
    sm.assert_derived(got, want, ctx)
    return got


def _nothing(d):
    return d["lags_used"] == 0 and d["detector"] == -1 and all(math.isnan(d[k]) for k in ("samples_per_symbol", "step_ratio", "coherence", "mean_level"))


def test_symrate_derive_against_the_model_on_the_host_records():
    for kind in KINDS:
        for tuned in (False, True):
            for S, n in SHAPES:
                rec, _, _ = _host_record(S, n, kind, tuned)
                d = _derive_both(rec, "S %d n %d %s tuned %d" % (S, n, kind, tuned))
                if kind in ("huge", "zeros"):
                    assert _nothing(d)
    rec, _, _ = _host_record(8, 8 * 700 + 7, "signal", False)
    d = pl.symrate_derive(rec)
    assert d["detector"] == 0 and d["lags_used"] >= 4 and abs(d["samples_per_symbol"] / (1.04 * 8) - 1) < 5e-4 and d["coherence"] > 0.5
    assert d["step_ratio"] == d["samples_per_symbol"] / 8 or abs(d["step_ratio"] - d["samples_per_symbol"] / 8) < 1e-15


def _hand_made(S=8, f=0.04, nb=1000, c=((1.0,) * 8, (0.0,) * 8), f_g=None):
    """a record whose detector z has coherence c[z][j] at lag j and turns by f (detector g: f_g) cycles a block"""
    r = pl.Symrate()
    r.n_samples = r.n_used = nb * S
    r.n_blocks = r.n_valid = nb
    r.samplesPerBaud, r.flags = S, pl.SR_DATA
    for z in range(2):
        r.sum_pow[z], r.sum_lvl[z] = 4.0 * nb, (2.5 + z) * nb * S  # (mean power of a block sum: 4)
        fz = f if z == 0 or f_g is None else f_g
        for j, L in enumerate(sm.LAGS):
            r.sum_re[z][j] = c[z][j] * 4.0 * (nb - L) * math.cos(2 * math.pi * L * fz)
            r.sum_im[z][j] = c[z][j] * 4.0 * (nb - L) * math.sin(2 * math.pi * L * fz)
    for j, L in enumerate(sm.LAGS):
        r.n_pairs[j] = nb - L
    return r


def test_symrate_derive_on_hand_made_records():
    d = _derive_both(_hand_made(), "clean")
    assert d["lags_used"] == 8 and d["detector"] == 0 and abs(d["samples_per_symbol"] - 8 / 1.04) < 1e-11 and abs(d["step_ratio"] - 1 / 1.04) < 1e-12
    assert abs(d["coherence"] - 1.0) < 1e-12 and abs(d["mean_level"] - 2.5) < 1e-12
    # the detector of the larger lag-1 coherence answers; a tie goes to e
    half = (0.5,) * 8
    d = _derive_both(_hand_made(c=(half, (0.5 * (1 + 1e-9),) * 8), f_g=-0.1), "g")
    assert d["detector"] == 1 and abs(d["samples_per_symbol"] - 8 / 0.9) < 1e-11 and abs(d["mean_level"] - 3.5) < 1e-12
    d = _derive_both(_hand_made(c=(half, half), f_g=-0.1), "tie")
    assert d["detector"] == 0 and abs(d["samples_per_symbol"] - 8 / 1.04) < 1e-11
    # (g answers through its lag 1 alone, however e does further on)
    d = _derive_both(_hand_made(c=((0.5,) + (1.0,) * 7, (0.6,) + (0.0,) * 7), f_g=0.1), "lag 1 decides")
    assert d["detector"] == 1 and d["lags_used"] == 1
    # a lag whose coherence is just under / just over half of lag 1's: the walk stops in front of it / goes on
    under = _derive_both(_hand_made(c=((0.8, 0.8, 0.8, 0.4 * (1 - 1e-9), 0.8, 0.8, 0.8, 0.8), (0.0,) * 8)), "under")
    over = _derive_both(_hand_made(c=((0.8, 0.8, 0.8, 0.4 * (1 + 1e-9), 0.8, 0.8, 0.8, 0.8), (0.0,) * 8)), "over")
    assert under["lags_used"] == 3 and over["lags_used"] == 8
    # the later lags are never looked at once one is refused, however coherent
    assert _derive_both(_hand_made(c=((0.8, 0.1) + (1.0,) * 6, (0.0,) * 8)), "second")["lags_used"] == 1
    # a lag with fewer than 8 pairs ends the walk; 8 pairs do not
    r = _hand_made()
    r.n_pairs[5] = 7
    for z in range(2):
        r.sum_re[z][5] *= 7.0 / (1000 - 32)
        r.sum_im[z][5] *= 7.0 / (1000 - 32)
    assert _derive_both(r, "7 pairs at lag 32")["lags_used"] == 5
    r = _hand_made(nb=136)  # (lag 128: 8 pairs)
    assert _derive_both(r, "8 pairs at lag 128")["lags_used"] == 8
    r = _hand_made(nb=135)
    assert _derive_both(r, "7 pairs at lag 128")["lags_used"] == 7
    # the unwrap at each lag: an f whose angle at lag L_j has wrapped j times over is still refined, not replaced -- every f
    # inside the range comes back, from either side of it
    for f in (0.49, -0.49, 0.26, -0.37, 0.124, 1.0 / 3.0):
        for used in range(1, 9):
            c = tuple(1.0 if j < used else 0.0 for j in range(8))
            d = _derive_both(_hand_made(f=f, c=(c, (0.0,) * 8)), "f %r, %d lags" % (f, used))
            assert d["lags_used"] == used and abs(d["samples_per_symbol"] - 8 / (1 + f)) < 1e-10, (f, used)
    # ... and a lag-1 angle that is off by less than half a turn of the next lag is corrected by it
    r = _hand_made(f=0.1)
    r.sum_re[0][0], r.sum_im[0][0] = 4.0 * 999 * math.cos(2 * math.pi * 0.3), 4.0 * 999 * math.sin(2 * math.pi * 0.3)
    assert abs(_derive_both(r, "coarse lag 1")["samples_per_symbol"] - 8 / 1.1) < 1e-10
    # nothing to derive from: no lag-1 pairs, zero lag-1 sums of both detectors, no DATA flag
    for what in ("pairs", "sums", "flag", "planned"):
        r = _hand_made()
        if what == "pairs":
            r.n_pairs[0] = 0
        elif what == "sums":
            r.sum_re[0][0] = r.sum_im[0][0] = 0.0
        elif what == "flag":
            r.flags = 0
        else:
            r.flags = pl.SR_PLANNED
        assert _nothing(_derive_both(r, what)), what
    # zero lag-1 sums of one detector: the other answers
    r = _hand_made(c=((1.0,) * 8, (0.1,) * 8), f_g=0.2)
    r.sum_re[0][0] = r.sum_im[0][0] = 0.0
    assert _derive_both(r, "e silent")["detector"] == 1
    # the zero record of a covered channel without a look
    assert _nothing(pl.symrate_derive(pl.Symrate()))


# ---- the entry on a control-plane-only handle ----------------------------------------------------------------------------------

C = 12
_S = [8, 4, 8, 1024, 8, 8, 5, 3, 1025, 33, 16, 2000]
_LENGTHS = [2 * (100 + 37 * i) + (i % 2) for i in range(C)]  # ragged, some with an odd last element
_LENGTHS[3] = 2 * 2048   # exactly two blocks of 1024
_LENGTHS[9] = 2 * 65     # one sample short of two blocks of 33
_LENGTHS[10] = 2 * (4096 * 16 + 100)  # beyond the cap
_NO_LOOK = (2, 4, 5, 7, 8, 9, 11)  # no packet, real data, a sample short, S below 4, S above 1024, a sample short, S above 1024


def _handle():
    h = pl.Handle(C, device=pl.DEVICE_NONE)
    h.configure(0, [dict(constelationSize=(2, 4, 8)[i % 3], samplesPerBaud=_S[i], numAvg=8) for i in range(C)])
    return h


def _packets(fmt=pl.FORMAT_CF32):
    pk = (pl.Packet * C)()
    for i in range(C):
        pk[i].n_floats, pk[i].sri_xdelta, pk[i].sri_mode, pk[i].present, pk[i].format = _LENGTHS[i], 0.01, 1, 1, fmt
    pk[2].present = 0      # no packet
    pk[4].sri_mode = 0     # real data
    pk[5].n_floats = 2 * 15  # fewer than two blocks
    pk[6].sriChanged = pk[6].inputQueueFlushed = 1  # (ignored)
    return pk


def _snapshot(h):
    return ([h.peek(c) for c in range(C)], [tuple(getattr(h.query(c), k) for k in pl.PROP_NAMES) for c in range(C)],
            [h.export_state(c) for c in range(C)], h.stats(), h.channel_stats(), bytes(h.quality_records()), bytes(h.acquire_records()),
            [h.resample_history(c).tobytes() for c in range(C)], [h.fir_history(c).tobytes() for c in range(C)])


def _planned(i):
    r = pl.Symrate()
    if i not in _NO_LOOK:
        n = _LENGTHS[i] // 2
        nb = min(n // _S[i], 4096)
        r.n_samples, r.n_used, r.n_blocks, r.samplesPerBaud, r.flags = n, nb * _S[i], nb, _S[i], pl.SR_PLANNED
    return bytes(r)


@pytest.mark.parametrize("fmt", (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8, pl.FORMAT_CF16))
def test_planned_records_of_a_control_plane_handle(fmt):
    h = _handle()
    assert bytes(h.symrate_records()) == bytes(392 * C)
    before = _snapshot(h)
    h.symrate_device(0, _packets(fmt), [1 if i % 2 else 9 for i in range(C)], [(i, 3 * i) for i in range(C)])
    recs = h.symrate_records()
    for i in range(C):
        assert bytes(recs[i]) == _planned(i), i
    assert recs[10].n_blocks == 4096 and recs[3].n_blocks == 2
    assert _snapshot(h) == before
    # uncovered channels keep theirs; covered ones are rewritten (channel 3 now without a packet)
    pk = _packets(fmt)
    pk[3].present = 0
    h.symrate_device(3, (pl.Packet * 2)(pk[3], pk[4]), None, None)
    recs = h.symrate_records()
    for i in range(C):
        assert bytes(recs[i]) == (bytes(392) if i == 3 else _planned(i)), i
    assert bytes(h.symrate_records(8, 2)) == _planned(8) + _planned(9)
    d = h.symrate(0, _packets(fmt))
    assert len(d) == C and all(_nothing(x) for x in d)
    assert _snapshot(h) == before
    h.close()


def test_every_refusal_changes_nothing():
    h = _handle()
    L = pl.load()
    h.symrate_device(0, _packets(), None, None)
    want = bytes(h.symrate_records())
    before = _snapshot(h)
    ones = [1] * C

    def refused(pk, strides, ch0=0, nch=C, word=None):
        arr = None if strides is None else (ctypes.c_uint64 * len(strides))(*strides)
        assert L.psk_soft_symrate_device(h._h, ch0, nch, pk, arr, None, None) == 1
        if word:
            assert word in L.psk_soft_last_error() and b"psk_soft_symrate_device" in L.psk_soft_last_error(), L.psk_soft_last_error()
        assert bytes(h.symrate_records()) == want and _snapshot(h) == before

    pk = _packets()
    pk[0].n_floats = 2 * 5000  # (would change record 0 if anything were written)
    refused(pk, ones[:4] + [0] + ones[5:], word=b"stride")                   # a stride of 0 (on a present packet, even a real one)
    refused(pk, ones[:6] + [(1 << 64) - 1] + ones[7:], word=b"64 bits")      # stride x 8 bytes overflows
    refused(pk, ones[:6] + [1 << 56] + ones[7:], word=b"64 bits")            # ... and stride x 8 bytes x samples
    bad = _packets()
    bad[0].n_floats = 2 * 5000
    bad[9].format = 2
    refused(bad, None, word=b"format")                                       # an unknown format on a present packet
    bad = _packets()
    bad[0].n_floats = 2 * 5000
    bad[1].data = 0x10004
    refused(bad, None, word=b"aligned")                                      # data that does not start on a whole sample
    refused(pk, None, ch0=1, nch=C)                                          # bad channel ranges
    refused(pk, None, ch0=C, nch=1)
    refused(pk, None, ch0=0, nch=0)
    assert L.psk_soft_symrate_device(h._h, 0, C, None, None, None, None) == 1
    assert L.psk_soft_symrate_device(None, 0, C, pk, None, None, None) == 1
    rec = (pl.Symrate * 2)()
    assert L.psk_soft_get_symrate(h._h, C - 1, 2, rec) == 1 and L.psk_soft_get_symrate(h._h, 0, 1, None) == 1
    with pytest.raises(ValueError):
        h.symrate_device(0, pk, [1] * (C - 1), None)
    # an absent packet's stride and format are not looked at; data that is misaligned under a packet the call would not read is not either
    ok = _packets()
    ok[2].format = 2
    ok[7].data = 0x10004
    h.symrate_device(0, ok, ones[:2] + [0] + ones[3:], None)
    assert bytes(h.symrate_records()) == want and _snapshot(h) == before
    h.close()


def test_looks_between_process_calls_move_nothing_on_a_control_plane_handle():
    """two handles go through the same process calls, one with looks (the symbol-rate look, and the carrier look among them) in
    between: peek, query, the state blobs, the statistics, the quality records and both histories are the same after every call"""
    a, b = _handle(), _handle()
    pk = _packets()

    def call(h, k):
        outs = (pl.Output * C)()
        pkk = _packets()
        for i in range(C):
            pkk[i].sriChanged = int(k == 0)
        h.process_device_resampled(0, pkk, None, [(i, 5 * i) for i in range(C)], [(0, pl.resample_step(1.04), pl.RS_RESTART if k == 0 else 0)] * C, outs)
        return [int(o.n_symbols) for o in outs]

    for k in range(3):
        b.symrate_device(0, pk, None, [(i, 7 * i) for i in range(C)])
        if k == 1:
            b.acquire_device(0, pk, None, None)
            a.acquire_device(0, pk, None, None)
        assert call(a, k) == call(b, k)
        b.symrate_device(2, (pl.Packet * 3)(pk[2], pk[3], pk[4]), [3, 3, 3], None)
        assert _snapshot(a) == _snapshot(b), k
    assert bytes(a.symrate_records()) == bytes(392 * C) and bytes(b.symrate_records()) != bytes(392 * C)
    a.close()
    b.close()


# ---- how well it does ----------------------------------------------------------------------------------------------------------

PAIRS = ((8.37, 8), (7.2, 8), (9.3, 8), (8.0, 8), (6.5, 8), (4.13, 4), (16.9, 16))
N_LOOK = 4096


def _pulse_signal(pulse, M, sps, seed, n=N_LOOK, sigma=0.01, offset=0.003):
    """n samples of M-PSK at sps samples a symbol, a carrier offset of `offset` cycles a sample, noise of sigma: the project's
    pulse (stimulus.pulse_shape at the fractional instant, as _signal of tests/test_resample_control.py) or a rectangular one"""
    g = np.random.default_rng(1000 * seed + M)
    u = np.arange(n, dtype=np.float64) / sps
    j = np.floor(u).astype(np.int64)
    f = u - j
    sym = g.integers(0, M, int(j[-1]) + 1)
    amp = 0.2 + 0.8 * np.sin(np.pi * (f * sps + 0.9) / (sps + 1.3)) if pulse == "project" else np.ones(n)
    x = amp * np.exp(1j * (2 * np.pi * sym[j] / M + 0.3 + 2 * np.pi * offset * np.arange(n))) + sigma * (g.standard_normal(n) + 1j * g.standard_normal(n))
    iq = np.empty(2 * n, F32)
    iq[0::2], iq[1::2] = x.real, x.imag
    return iq


@pytest.mark.parametrize("pulse, detector", (("project", 0), ("rect", 1)))
def test_the_estimate_on_the_pulses_it_is_meant_for(pulse, detector):
    """M in 2, 4, 8, seven (sps, S) pairs, 4096 samples, sigma 0.01, a carrier offset of 0.003 cycles a sample, 8 seeds, through
    psk_soft_symrate_host: |samples_per_symbol / sps - 1| <= 5e-4 -- three times the worst of the float64 rehearsal of the
    definition (1.6e-4, the rectangular pulse at 9.3 / 8), and what keeps a resampled packet of 25 000 samples within two
    symbols of its true count -- and the detector that answers is e for the project's pulse, g for the rectangular one.
    Measured, worst case of each pulse: DESIGN.md 2.12."""
    worst = (0.0, None)
    for M in (2, 4, 8):
        for sps, S in PAIRS:
            for seed in range(8):
                d = pl.symrate_derive(pl.symrate_host(S, _pulse_signal(pulse, M, sps, seed)))
                err = abs(d["samples_per_symbol"] / sps - 1)
                worst = max(worst, (err, (M, sps, S, seed, d["coherence"], d["lags_used"])))
                assert d["detector"] == detector, (M, sps, S, seed, d)
                assert err <= 5e-4, (M, sps, S, seed, d)
    print("pulse %s: worst relative error %.3g at (M, sps, S, seed, coherence, lags) = %r" % (pulse, worst[0], worst[1]))


def test_noise_alone_has_no_coherence():
    """sigma 1 and no signal: coherence stays below 4 / sqrt(n_blocks) over 8 seeds"""
    worst = 0.0
    for S in (4, 8, 16):
        for seed in range(8):
            g = np.random.default_rng(77 + seed)
            rec = pl.symrate_host(S, g.standard_normal(2 * N_LOOK).astype(F32))
            d = pl.symrate_derive(rec)
            worst = max(worst, d["coherence"] * math.sqrt(rec.n_blocks))
            assert d["coherence"] < 4.0 / math.sqrt(rec.n_blocks), (S, seed, d)
    print("noise: the largest coherence x sqrt(n_blocks) is %.3g" % worst)


# ---- what it is for ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sps", [8.37, 7.2, 9.3])
def test_look_step_resample_demodulate(oracle_mod, sps):
    """the packets of tests/test_resample_control.py (QPSK, 3000 symbols at 8.37 / 7.2 / 9.3 samples a symbol, samplesPerBaud 8): a
    look at the first 4096 samples, resample_step(step_ratio), resample_apply, the oracle -- the symbol count within 2 of the
    count at the true step, and at most a tenth of the raw packet's wrong differential decisions, each at its best lag"""
    M, S = 4, 8
    sym, iq = _signal(M, sps)

    def soft(data):
        o = oracle_mod.OracleComponent()
        o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = S, M, 100, 50
        return o.service(data, 0.01, sriChanged=True).soft

    d = pl.symrate_derive(pl.symrate_host(S, iq[: 2 * N_LOOK]))
    raw = soft(iq)
    true = soft(pl.resample_apply((0, pl.resample_step(sps / S), pl.RS_RESTART), iq)[0])
    est = soft(pl.resample_apply((0, pl.resample_step(d["step_ratio"]), pl.RS_RESTART), iq)[0])
    wrong = {k: min(_decision_errors(v, sym, M, lag)[0] for lag in lags)
             for k, v, lags in (("raw", raw, range(-5, 141)), ("true", true, range(-2, 3)), ("est", est, range(-2, 3)))}
    print("sps %.2f: estimated %.5f (coherence %.3f, %d lags); symbols raw %d, true step %d, estimated step %d; wrong decisions raw %d, true step %d, estimated step %d"
          % (sps, d["samples_per_symbol"], d["coherence"], d["lags_used"], raw.size // 2, true.size // 2, est.size // 2, wrong["raw"], wrong["true"], wrong["est"]))
    assert abs(est.size // 2 - true.size // 2) <= 2
    assert wrong["est"] <= wrong["raw"] / 10.0
