"""psk_soft_acquire_device without a GPU: the exports and the record's layout, the host-side definition (psk_soft_acquire_host) and
derivation (psk_soft_acquire_derive) against tests/acquire_model.py, the entry on control-plane-only handles (PSK_SOFT_DEVICE_NONE)
-- it checks, then leaves planned records and nothing else --, and what the look is for: a carrier offset no search that watches
`lock` can find, estimated from the samples and taken out in front of the oracle."""
import ctypes
import math

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from psk_soft_amd.stimulus import synth_channel
from tests import acquire_model as am
from tests import tune_model as tm

F32 = np.float32


def test_the_symbols_are_exported_and_the_record_has_its_layout():
    L = pl.load()
    for name in ("psk_soft_acquire_device", "psk_soft_get_acquire", "psk_soft_acquire_derive", "psk_soft_acquire_host",
                 "psk_soft_acquire_bytes", "psk_soft_acquire_piece"):
        assert name in pl.EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    A = pl.Acquire
    assert ctypes.sizeof(A) == 224 and L.psk_soft_acquire_bytes() == 224
    assert [getattr(A, k).offset for k in ("n_samples", "n_valid", "n_pairs", "sum_re", "sum_im", "sum_e", "constelationSize", "flags", "pad")] == [
        0, 8, 16, 80, 144, 208, 216, 218, 219]
    D = pl.AcquireDerived
    assert ctypes.sizeof(D) == 32 and [getattr(D, k).offset for k in ("offset_cycles_per_sample", "coherence", "mean_energy", "lags_used")] == [
        0, 8, 16, 24]
    assert (pl.A_DATA, pl.A_TUNED, pl.A_PLANNED) == (1, 2, 128)
    assert ctypes.sizeof(pl.Packet) == 32 and ctypes.sizeof(pl.Tune) == 16
    assert pl.acquire_piece() >= 256 and pl.acquire_piece() % 128 == 0


# ---- the definition ----------------------------------------------------------------------------------------------------------

LENGTHS = (1, 2, 3, 128, 129, 130, 1000)
KINDS = ("signal", "nonfinite", "tiny", "huge", "large")
_TUNE = (0x0123456789ABCDEF, tm.step_word(-0.0137))


def _samples(M, n, kind, seed):
    """interleaved float32: a noisy M-PSK carrier at 0.011 cycles per sample; `nonfinite` puts +-inf and NaN samples in the
    middle, `tiny` (1e-24) makes every sample invalid by underflow (a < FLT_MIN), `huge` (3e19) by overflow (q = e*e is inf), `large`
    (1e9) leaves e and q finite and overflows a = q*q of M = 8 only"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    z = np.exp(2j * math.pi * (rng.integers(0, M, n) / M + 0.011 * k)) * rng.uniform(0.5, 2.0, n) + 0.05 * (
        rng.standard_normal(n) + 1j * rng.standard_normal(n))
    z = z * {"signal": 1.0, "nonfinite": 1.0, "tiny": 1e-24, "huge": 3e19, "large": 1e9}[kind]
    x = np.empty(2 * n, F32)
    x[0::2], x[1::2] = z.real, z.imag
    if kind == "nonfinite":
        for pos, v in ((n // 2, np.inf), (n // 2 + 3, -np.inf), (n // 3, np.nan), (n - 1, np.nan), (0, np.inf)):
            x[2 * (pos % n) + (pos & 1)] = v
    return x


_host_records = {}


def _host_record(M, n, kind, tuned):
    key = (M, n, kind, tuned)
    if key not in _host_records:
        x = _samples(M, n, kind, 31 * n + M)
        tune = _TUNE if tuned else None
        _host_records[key] = (pl.acquire_host(M, x, tune), am.model_record(x, M, tune))
    return _host_records[key]


@pytest.mark.parametrize("tuned", (False, True))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", (2, 4, 8))
def test_acquire_host_against_the_model(M, kind, tuned):
    for n in LENGTHS:
        rec, model = _host_record(M, n, kind, tuned)
        am.assert_record(rec, model, "M %d n %d %s tuned %d" % (M, n, kind, tuned))
        assert rec.flags == pl.A_DATA | (pl.A_TUNED if tuned else 0) and rec.n_samples == n
        if kind in ("tiny", "huge") or (kind == "large" and M == 8):
            assert rec.n_valid == 0 and not any(rec.n_pairs) and rec.sum_e == 0.0
        elif kind in ("signal", "large"):
            assert rec.n_valid == n and list(rec.n_pairs) == [max(0, n - L) for L in am.LAGS]
        if kind == "nonfinite":
            assert rec.n_valid < n


def test_acquire_host_null_tune_zero_tune_and_bad_arguments():
    L = pl.load()
    x = _samples(4, 300, "signal", 5)
    a, b = pl.acquire_host(4, x), pl.acquire_host(4, x, (0, 0))
    assert bytes(a) == bytes(b) and a.flags == pl.A_DATA
    # an odd last element is dropped; no sample is the zero record
    assert bytes(pl.acquire_host(4, x[:-1])) == bytes(pl.acquire_host(4, x[:-2]))
    assert bytes(pl.acquire_host(4, x[:1])) == bytes(224)
    rec = pl.Acquire()
    for M in (0, 1, 3, 16):
        assert L.psk_soft_acquire_host(M, None, x.ctypes.data, 10, ctypes.byref(rec)) == 1
    assert L.psk_soft_acquire_host(4, None, None, 10, ctypes.byref(rec)) == 1
    assert L.psk_soft_acquire_host(4, None, x.ctypes.data, 10, None) == 1
    assert L.psk_soft_acquire_derive(None, None) == 1


def _derive_both(rec, ctx):
    got, want = pl.acquire_derive(rec), am.derive(rec)
    am.assert_derived(got, want, ctx)
    return got


@pytest.mark.parametrize("M", (2, 4, 8))
def test_acquire_derive_against_the_model_on_the_host_records(M):
    for kind in KINDS:
        for tuned in (False, True):
            for n in LENGTHS:
                rec, _ = _host_record(M, n, kind, tuned)
                d = _derive_both(rec, "M %d n %d %s tuned %d" % (M, n, kind, tuned))
                if kind in ("tiny", "huge") or n == 1:
                    assert d["lags_used"] == 0 and math.isnan(d["offset_cycles_per_sample"]) and math.isnan(d["coherence"])
    rec, _ = _host_record(M, 1000, "signal", False)
    d = pl.acquire_derive(rec)
    assert d["lags_used"] >= 4 and abs(d["offset_cycles_per_sample"] - 0.011) < 2e-4 and d["coherence"] > 0.5
    rec, _ = _host_record(M, 1000, "signal", True)  # (the residual under the tune)
    assert abs(pl.acquire_derive(rec)["offset_cycles_per_sample"] - (0.011 - 0.0137)) < 2e-4


def _hand_made(M=4, f=0.01, n=1000, c=(1.0,) * 8):
    r = pl.Acquire()
    r.n_samples, r.n_valid, r.sum_e, r.constelationSize, r.flags = n, n, 2.5 * n, M, pl.A_DATA
    for j, L in enumerate(am.LAGS):
        r.n_pairs[j] = n - L
        r.sum_re[j] = c[j] * (n - L) * math.cos(2 * math.pi * M * L * f)
        r.sum_im[j] = c[j] * (n - L) * math.sin(2 * math.pi * M * L * f)
    return r


def test_acquire_derive_on_hand_made_records():
    d = _derive_both(_hand_made(), "clean")
    assert d["lags_used"] == 8 and abs(d["offset_cycles_per_sample"] - 0.01) < 1e-12 and abs(d["mean_energy"] - 2.5) < 1e-12
    # a lag whose coherence is just under / just over half of lag 1's: the walk stops in front of it / goes on
    under = _derive_both(_hand_made(c=(0.8, 0.8, 0.8, 0.4 * (1 - 1e-9), 0.8, 0.8, 0.8, 0.8)), "under")
    over = _derive_both(_hand_made(c=(0.8, 0.8, 0.8, 0.4 * (1 + 1e-9), 0.8, 0.8, 0.8, 0.8)), "over")
    assert under["lags_used"] == 3 and over["lags_used"] == 8
    # the later lags are never looked at once one is refused, however coherent
    r = _hand_made(c=(0.8, 0.1, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0))
    assert _derive_both(r, "second")["lags_used"] == 1
    # a lag without pairs ends the walk
    r = _hand_made()
    r.n_pairs[5] = 0
    assert _derive_both(r, "no pairs at lag 32")["lags_used"] == 5
    # nothing to derive from: no lag-1 pairs, zero lag-1 sums, no DATA flag
    for what in ("pairs", "sums", "flag", "planned"):
        r = _hand_made()
        if what == "pairs":
            r.n_pairs[0] = 0
        elif what == "sums":
            r.sum_re[0] = r.sum_im[0] = 0.0
        elif what == "flag":
            r.flags = 0
        else:
            r.flags = pl.A_PLANNED
        d = _derive_both(r, what)
        assert d["lags_used"] == 0 and all(math.isnan(d[k]) for k in ("offset_cycles_per_sample", "coherence", "mean_energy")), what
    # a negative offset near the edge of the range, M = 8: |f| < 1 / 16
    d = _derive_both(_hand_made(M=8, f=-0.06), "edge")
    assert abs(d["offset_cycles_per_sample"] + 0.06) < 1e-12
    # the zero record of a covered channel without a look
    assert pl.acquire_derive(pl.Acquire())["lags_used"] == 0


# ---- the entry on a control-plane-only handle ----------------------------------------------------------------------------------

C = 12
_LENGTHS = [2 * (100 + 37 * i) + (i % 2) for i in range(C)]  # ragged, some with an odd last element


def _handle():
    h = pl.Handle(C, device=pl.DEVICE_NONE)
    h.configure(0, [dict(constelationSize=(2, 4, 8)[i % 3], samplesPerBaud=4 + i) for i in range(C)])
    h.configure(7, [dict(constelationSize=16)])
    return h


def _packets(fmt=pl.FORMAT_CF32):
    pk = (pl.Packet * C)()
    for i in range(C):
        pk[i].n_floats, pk[i].sri_xdelta, pk[i].sri_mode, pk[i].present, pk[i].format = _LENGTHS[i], 0.01, 1, 1, fmt
    pk[2].present = 0      # no packet
    pk[4].sri_mode = 0     # real data
    pk[5].n_floats = 1     # not one whole sample
    pk[6].sriChanged = pk[6].inputQueueFlushed = 1  # (ignored)
    return pk


def _snapshot(h):
    return ([h.peek(c) for c in range(C)], [tuple(getattr(h.query(c), k) for k in pl.PROP_NAMES) for c in range(C)],
            [h.export_state(c) for c in range(C)], h.stats(), h.channel_stats(), bytes(h.quality_records()))


def _planned(i):
    r = pl.Acquire()
    if i not in (2, 4, 5, 7):
        r.n_samples, r.constelationSize, r.flags = _LENGTHS[i] // 2, (2, 4, 8)[i % 3], pl.A_PLANNED
    return bytes(r)


@pytest.mark.parametrize("fmt", (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8, pl.FORMAT_CF16))
def test_planned_records_of_a_control_plane_handle(fmt):
    h = _handle()
    assert bytes(h.acquire_records()) == bytes(224 * C)
    before = _snapshot(h)
    h.acquire_device(0, _packets(fmt), [1 if i % 2 else 9 for i in range(C)], [(i, 3 * i) for i in range(C)])
    recs = h.acquire_records()
    for i in range(C):
        assert bytes(recs[i]) == _planned(i), i
    assert _snapshot(h) == before
    # uncovered channels keep theirs; covered ones are rewritten (channel 3 now without a packet)
    pk = _packets(fmt)
    pk[3].present = 0
    h.acquire_device(3, (pl.Packet * 2)(pk[3], pk[4]), None, None)
    recs = h.acquire_records()
    for i in range(C):
        assert bytes(recs[i]) == (bytes(224) if i == 3 else _planned(i)), i
    assert bytes(h.acquire_records(8, 2)) == _planned(8) + _planned(9)
    d = h.acquire(0, _packets(fmt))
    assert len(d) == C and all(x["lags_used"] == 0 and math.isnan(x["offset_cycles_per_sample"]) for x in d)
    assert _snapshot(h) == before
    h.close()


def test_every_refusal_changes_nothing():
    h = _handle()
    L = pl.load()
    h.acquire_device(0, _packets(), None, None)
    want = bytes(h.acquire_records())
    before = _snapshot(h)
    ones = [1] * C

    def refused(pk, strides, ch0=0, nch=C, word=None):
        arr = None if strides is None else (ctypes.c_uint64 * len(strides))(*strides)
        assert L.psk_soft_acquire_device(h._h, ch0, nch, pk, arr, None, None) == 1
        if word:
            assert word in L.psk_soft_last_error(), L.psk_soft_last_error()
        assert bytes(h.acquire_records()) == want and _snapshot(h) == before

    pk = _packets()
    pk[0].n_floats = 2 * 5000  # (would change record 0 if anything were written)
    refused(pk, ones[:4] + [0] + ones[5:], word=b"stride")                   # a stride of 0 (on a present packet, even a real one)
    refused(pk, ones[:8] + [(1 << 64) - 1] + ones[9:], word=b"64 bits")      # stride x 8 bytes overflows
    refused(pk, ones[:8] + [1 << 56] + ones[9:], word=b"64 bits")            # ... and stride x 8 bytes x samples
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
    assert L.psk_soft_acquire_device(h._h, 0, C, None, None, None, None) == 1
    assert L.psk_soft_acquire_device(None, 0, C, pk, None, None, None) == 1
    rec = (pl.Acquire * 2)()
    assert L.psk_soft_get_acquire(h._h, C - 1, 2, rec) == 1 and L.psk_soft_get_acquire(h._h, 0, 1, None) == 1
    with pytest.raises(ValueError):
        h.acquire_device(0, pk, [1] * (C - 1), None)
    # an absent packet's stride and format are not looked at
    ok = _packets()
    ok[2].format = 2
    h.acquire_device(0, ok, ones[:2] + [0] + ones[3:], None)
    assert bytes(h.acquire_records()) == want and _snapshot(h) == before
    h.close()


# ---- what it is for ------------------------------------------------------------------------------------------------------------

N_LOOK = 4096


def _oracle_lock(oracle_mod, data, M):
    o = oracle_mod.OracleComponent()
    o.samplesPerBaud, o.constelationSize = 8, M
    r = o.service(data, 0.01, sriChanged=True)
    assert r.soft.size >= 2 * 2000
    return tm.lock_of(r.soft, M)


@pytest.mark.parametrize("M, r, after", [(4, 0.10, 0.95), (8, 0.20, 0.85)])
@pytest.mark.parametrize("ch", (1, 2, 3))
def test_an_offset_the_tracker_cannot_follow_is_found_and_taken_out(oracle_mod, ch, M, r, after):
    """synth_channel at 8 samples per baud with a carrier offset of r cycles per symbol: the estimate from the first 4096 samples
    is within 2e-4 cycles per symbol; the oracle loses the untuned signal (lock < 0.2) and holds the one tuned by the estimate."""
    x = synth_channel(ch, M, 8, 24000, sigma=0.05, cfo=2 * math.pi * M * r)
    d = pl.acquire_derive(pl.acquire_host(M, x[: 2 * N_LOOK]))
    est = d["offset_cycles_per_sample"] * 8
    tuned = pl.tune_apply(0, pl.tune_step(-d["offset_cycles_per_sample"]), x)
    before, behind = _oracle_lock(oracle_mod, x, M), _oracle_lock(oracle_mod, tuned, M)
    print("ch %d M %d r %.2f: estimate %.6f (error %.2g), coherence %.3f, lags %d, lock untuned %.4f tuned %.4f"
          % (ch, M, r, est, est - r, d["coherence"], d["lags_used"], before, behind))
    assert abs(est - r) <= 2e-4
    assert before < 0.2
    assert behind > after


@pytest.mark.parametrize("ch", (1, 2, 3))
def test_the_alias_no_search_over_lock_can_tell_apart(oracle_mod, ch):
    """QPSK at 0.30 cycles per symbol: to the tracker that is 0.30 - 1/4 = 0.05, which it follows -- the whole-call lock is above
    0.9 with the constellation turning a quarter turn every symbol.  The samples tell: the estimate is 0.30."""
    M, r = 4, 0.30
    x = synth_channel(ch, M, 8, 24000, sigma=0.05, cfo=2 * math.pi * M * r)
    d = pl.acquire_derive(pl.acquire_host(M, x[: 2 * N_LOOK]))
    est = d["offset_cycles_per_sample"] * 8
    lock = _oracle_lock(oracle_mod, x, M)
    print("ch %d: estimate %.6f (error %.2g), lock untuned %.4f" % (ch, est, est - r, lock))
    assert abs(est - r) <= 2e-4
    assert lock > 0.9
