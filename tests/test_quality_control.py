"""PSK_SOFT_OPT_QUALITY on the control plane, without a GPU: the record's layout, the option, what a control-plane-only handle
puts into the records (the counts of the call's psk_soft_output_t, the property snapshot, PSK_SOFT_Q_PLANNED), which records a
call leaves alone, the refusals, and psk_soft_quality_derive against the same formulas in Python (tests/quality_model.py)."""
import ctypes
import math

import pytest

from psk_soft_amd import lib as pl
from tests import quality_model as qm

SUM_FIELDS = ("n_finite", "n_lock", "index_changes", "sum_e", "sum_e2", "sum_lock_re", "sum_lock_im", "phase_first", "phase_last",
              "index_first", "index_last")


def _is_zero(q):
    return bytes(q) == bytes(ctypes.sizeof(pl.Quality))


def test_record_layout():
    L = pl.load()
    assert L.psk_soft_quality_bytes() == ctypes.sizeof(pl.Quality) == 88
    assert L.psk_soft_quality_bytes() % 8 == 0
    assert ctypes.sizeof(pl.QualityDerived) == 32
    assert L.psk_soft_abi_version() == 2
    assert (pl.Q_SOFT, pl.Q_PHASE, pl.Q_INDEX, pl.Q_LOCK, pl.Q_PLANNED) == (1, 2, 4, 8, 128)
    assert pl.Handle.OPT_QUALITY == 6
    for name in ("psk_soft_quality_bytes", "psk_soft_get_quality", "psk_soft_quality_derive"):
        assert name in pl.EXPORTS and hasattr(L, name)


def test_option_values_and_off_by_default():
    h = pl.Handle(3, device=pl.DEVICE_NONE)
    # off: a call writes no record
    h.plan_only(0, [dict(n_floats=20000, xdelta=0.01, sriChanged=True)] * 3)
    assert all(_is_zero(q) for q in h.quality_records())
    for bad in (2, -1, 7):
        with pytest.raises(pl.PskSoftError) as e:
            h.set_option(pl.Handle.OPT_QUALITY, bad)
        assert e.value.status == 1
    h.set_option(pl.Handle.OPT_QUALITY, 1)
    h.plan_only(0, [dict(n_floats=20000, xdelta=0.01)] * 3)
    assert all(q.flags == pl.Q_PLANNED and q.n_symbols > 0 for q in h.quality_records())
    # off again: the records stay as they are and calls leave them alone
    h.set_option(pl.Handle.OPT_QUALITY, 0)
    before = [bytes(q) for q in h.quality_records()]
    h.plan_only(0, [dict(n_floats=4000, xdelta=0.01)] * 3)
    assert [bytes(q) for q in h.quality_records()] == before
    # switched on: all records zeroed
    h.set_option(pl.Handle.OPT_QUALITY, 1)
    assert all(_is_zero(q) for q in h.quality_records())
    h.close()


def test_planned_records_of_ragged_calls():
    """Channels of different properties through three calls: cold start, a window still filling, no packet, sri_mode 0,
    samplesPerBaud 1, a call beyond 2^20 symbols.  Every covered channel's record holds the n_symbols of the call's
    psk_soft_output_t, the properties the call ran with and Q_PLANNED, everything else zero."""
    props = [dict(samplesPerBaud=8, constelationSize=4, numAvg=100, phaseAvg=50, differentialDecoding=0),
             dict(samplesPerBaud=4, constelationSize=2, numAvg=25, phaseAvg=10, differentialDecoding=1),
             dict(samplesPerBaud=1, constelationSize=8, numAvg=0, phaseAvg=20, differentialDecoding=0),
             dict(samplesPerBaud=2, constelationSize=16, numAvg=100, phaseAvg=50, differentialDecoding=1),
             dict(samplesPerBaud=30, constelationSize=8, numAvg=400, phaseAvg=200, differentialDecoding=0),
             dict(samplesPerBaud=8, constelationSize=4, numAvg=100, phaseAvg=50, differentialDecoding=0)]
    C = len(props)
    h = pl.Handle(C, device=pl.DEVICE_NONE, max_packet_complex=1 << 23)
    h.configure(0, props)
    h.set_option(pl.Handle.OPT_QUALITY, 1)
    long_floats = 2 * 2 * ((1 << 20) + 12345)
    calls = [
        # cold start; channel 4's window (30 x 400 samples) is still filling; channel 5 has no packet
        [dict(n_floats=2 * 8000, xdelta=0.01, sriChanged=True), dict(n_floats=2 * 8000 + 1, xdelta=0.01, sriChanged=True),
         dict(n_floats=2 * 777, xdelta=0.01, sriChanged=True), dict(n_floats=2 * 9000, xdelta=0.01, sriChanged=True),
         dict(n_floats=2 * 5000, xdelta=0.01, sriChanged=True), None],
        # steady; channel 1's packet is real data (dropped); channel 3: beyond 2^20 symbols
        [dict(n_floats=2 * 8001, xdelta=0.01), dict(n_floats=2 * 8000, xdelta=0.01, mode=0), dict(n_floats=2 * 5, xdelta=0.01),
         dict(n_floats=long_floats, xdelta=0.01), dict(n_floats=2 * 20000, xdelta=0.01), dict(n_floats=2 * 3000, xdelta=0.01, sriChanged=True)],
    ]
    for k, pk in enumerate(calls):
        res = h.plan_only(0, pk)
        recs = h.quality_records()
        for c in range(C):
            q = recs[c]
            assert q.n_symbols == res[c]["n_symbols"], (k, c)
            assert (q.constelationSize, q.samplesPerBaud, q.differentialDecoding) == \
                   (props[c]["constelationSize"], props[c]["samplesPerBaud"], props[c]["differentialDecoding"]), (k, c)
            assert q.flags == pl.Q_PLANNED, (k, c)
            assert all(getattr(q, f) == 0 for f in SUM_FIELDS) and bytes(q.pad) == bytes(6), (k, c)
        if k == 0:
            assert recs[0].n_symbols > 0 and recs[4].n_symbols == 0 and recs[2].n_symbols == 777
        else:
            assert recs[1].n_symbols == 0 and recs[3].n_symbols > (1 << 20) and recs[2].n_symbols == 5
    h.close()


def test_no_packet_is_a_planned_record_of_zero_symbols():
    h = pl.Handle(2, device=pl.DEVICE_NONE)
    h.configure(0, [dict(samplesPerBaud=5, constelationSize=2)] * 2)
    h.set_option(pl.Handle.OPT_QUALITY, 1)
    h.plan_only(0, [None, dict(n_floats=2000, xdelta=0.01, sriChanged=True)])
    a, b = h.quality_records()
    assert (a.n_symbols, a.flags, a.samplesPerBaud, a.constelationSize) == (0, pl.Q_PLANNED, 5, 2)
    assert b.n_symbols > 0 and b.flags == pl.Q_PLANNED
    h.close()


def test_uncovered_channels_keep_their_records():
    h = pl.Handle(40, device=pl.DEVICE_NONE)
    h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=100)
    h.set_option(pl.Handle.OPT_QUALITY, 1)
    h.plan_only(0, [dict(n_floats=2 * 9000, xdelta=0.01, sriChanged=True)] * 40)   # (a uniform batch: the stamped path)
    first = [bytes(q) for q in h.quality_records()]
    assert len(set(first)) == 1 and h.quality_records()[0].n_symbols > 0
    h.configure(10, [dict(constelationSize=8, differentialDecoding=1)] * 5)
    r = h.plan_only(10, [dict(n_floats=2 * 4000, xdelta=0.01)] * 5)
    now = h.quality_records()
    for c in range(40):
        if 10 <= c < 15:
            assert (now[c].n_symbols, now[c].constelationSize, now[c].differentialDecoding) == (r[c - 10]["n_symbols"], 8, 1)
        else:
            assert bytes(now[c]) == first[c]
    # the properties a call runs with are those configured BEFORE it
    h.plan_only(0, [dict(n_floats=2 * 9000, xdelta=0.01)] * 40)
    assert [q.constelationSize for q in h.quality_records(8, 8)] == [4, 4, 8, 8, 8, 8, 8, 4]
    # ranges of the getter
    assert [bytes(q) for q in h.quality_records(12, 3)] == [bytes(q) for q in h.quality_records()][12:15]
    assert len(h.quality(38)) == 2 and set(h.quality(0, 1)[0]) >= {"lock", "snr_db", "mean_energy", "index_change_rate", "n_symbols"}
    h.close()


def test_bad_arguments_are_refused():
    L = pl.load()
    h = pl.Handle(4, device=pl.DEVICE_NONE)
    arr = (pl.Quality * 8)()
    assert L.psk_soft_get_quality(h._h, 0, 4, arr) == 0
    assert L.psk_soft_get_quality(h._h, 0, 5, arr) == 1
    assert L.psk_soft_get_quality(h._h, 4, 1, arr) == 1
    assert L.psk_soft_get_quality(h._h, 0xFFFFFFFF, 2, arr) == 1
    assert L.psk_soft_get_quality(h._h, 0, 4, None) == 1
    assert L.psk_soft_get_quality(None, 0, 4, arr) == 1
    d = pl.QualityDerived()
    assert L.psk_soft_quality_derive(None, ctypes.byref(d)) == 1
    assert L.psk_soft_quality_derive(ctypes.byref(arr[0]), None) == 1
    assert L.psk_soft_set_option(None, pl.Handle.OPT_QUALITY, 1) == 1
    h.close()


def _rec(**kw):
    q = pl.Quality()
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _same(a, b):
    if math.isnan(b):
        return math.isnan(a)
    return not math.isnan(a) and abs(a - b) <= 1e-12 * abs(b)


DERIVE_CASES = {
    "clean qpsk": dict(n_symbols=4900, n_finite=4900, n_lock=4900, index_changes=3, sum_e=4903.25, sum_e2=4910.5, sum_lock_re=-1200.5,
                       sum_lock_im=4740.125, flags=15, constelationSize=4, samplesPerBaud=8),
    "noisy": dict(n_symbols=1000, n_finite=998, n_lock=990, index_changes=400, sum_e=1100.0, sum_e2=1500.0, sum_lock_re=30.0,
                  sum_lock_im=-12.0, flags=15, constelationSize=8, samplesPerBaud=8),
    "differential: no snr": dict(n_symbols=500, n_finite=499, n_lock=499, index_changes=0, sum_e=510.0, sum_e2=530.0, sum_lock_re=400.0,
                                 sum_lock_im=1.0, flags=15, differentialDecoding=1),
    "d <= 0 (heavier than gaussian)": dict(n_symbols=100, n_finite=100, n_lock=100, sum_e=100.0, sum_e2=250.0, sum_lock_re=1.0, flags=9),
    "d == 0": dict(n_symbols=100, n_finite=100, n_lock=100, sum_e=100.0, sum_e2=200.0, sum_lock_re=1.0, flags=9),
    "m2 - s <= 0 (no noise at all)": dict(n_symbols=64, n_finite=64, n_lock=64, sum_e=64.0, sum_e2=64.0, sum_lock_re=64.0, flags=15, index_changes=0),
    "no Q_LOCK": dict(n_symbols=100, n_finite=100, n_lock=0, sum_e=120.0, sum_e2=150.0, flags=7, constelationSize=16, index_changes=7),
    "Q_LOCK but n_lock 0": dict(n_symbols=100, n_finite=100, n_lock=0, sum_e=1e-80, sum_e2=0.0, flags=15),
    "n_finite 0": dict(n_symbols=1, n_finite=0, n_lock=0, flags=15),
    "no Q_INDEX": dict(n_symbols=777, n_finite=777, n_lock=777, sum_e=800.0, sum_e2=830.0, sum_lock_re=-700.0, sum_lock_im=-90.0,
                       flags=11, index_changes=5),
    "one symbol": dict(n_symbols=1, n_finite=1, n_lock=1, sum_e=1.02, sum_e2=1.0404, sum_lock_re=0.6, sum_lock_im=0.8, flags=15),
    "two symbols": dict(n_symbols=2, n_finite=2, n_lock=2, index_changes=1, sum_e=2.1, sum_e2=2.3, sum_lock_re=1.9, sum_lock_im=0.1, flags=15),
    "planned": dict(n_symbols=5000, flags=128, constelationSize=4, samplesPerBaud=8),
    "zero record": dict(),
}


@pytest.mark.parametrize("name", sorted(DERIVE_CASES))
def test_derive_against_the_formulas(name):
    q = _rec(**DERIVE_CASES[name])
    got, want = pl.quality_derive(q), qm.derive(q)
    for k in ("lock", "snr_db", "mean_energy", "index_change_rate"):
        assert _same(got[k], want[k]), (name, k, got[k], want[k])


def test_derive_nan_conditions_and_values():
    """the formulas' own results on the hand-made records, so that model and library cannot be wrong together"""
    d = {k: pl.quality_derive(_rec(**v)) for k, v in DERIVE_CASES.items()}
    c = d["clean qpsk"]
    assert _same(c["lock"], math.hypot(-1200.5, 4740.125) / 4900) and _same(c["mean_energy"], 4903.25 / 4900)
    assert _same(c["index_change_rate"], 3 / 4899)
    m2, m4 = 4903.25 / 4900, 4910.5 / 4900
    s = math.sqrt(2 * m2 * m2 - m4)
    assert _same(c["snr_db"], 10 * math.log10(s / (m2 - s))) and 20 < c["snr_db"] < 40
    assert math.isnan(d["differential: no snr"]["snr_db"]) and _same(d["differential: no snr"]["lock"], math.hypot(400.0, 1.0) / 499)
    assert math.isnan(d["d <= 0 (heavier than gaussian)"]["snr_db"]) and math.isnan(d["d == 0"]["snr_db"])
    assert math.isnan(d["m2 - s <= 0 (no noise at all)"]["snr_db"]) and d["m2 - s <= 0 (no noise at all)"]["lock"] == 1.0
    assert d["m2 - s <= 0 (no noise at all)"]["index_change_rate"] == 0.0
    assert math.isnan(d["no Q_LOCK"]["lock"]) and _same(d["no Q_LOCK"]["index_change_rate"], 7 / 99)
    assert math.isnan(d["Q_LOCK but n_lock 0"]["lock"])
    assert all(math.isnan(d["n_finite 0"][k]) for k in ("lock", "snr_db", "mean_energy", "index_change_rate"))
    assert math.isnan(d["no Q_INDEX"]["index_change_rate"]) and not math.isnan(d["no Q_INDEX"]["snr_db"])
    assert math.isnan(d["one symbol"]["index_change_rate"]) and _same(d["one symbol"]["lock"], 1.0)
    assert d["two symbols"]["index_change_rate"] == 1.0
    assert all(math.isnan(v) for v in d["planned"].values()) and all(math.isnan(v) for v in d["zero record"].values())
