"""samplesPerBaud above 1024 (the property is a ushort: up to 65535) on the control plane, without a GPU: configure accepts it
within the window limit, the plans follow the oracle's counters call by call, wide-symbol channels are planned for the
time-tiled kernels behind the wide front stage (psk_wide.hip) unless phaseAvg is beyond what those hold, and the state of
such a channel survives export and import."""
import math

import numpy as np
import pytest

from psk_soft_amd import lib as pl


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("S", [1025, 2048, 4097, 32768, 65535])
def test_configure_accepts_wide_symbols_within_the_window_limit(S):
    h = pl.Handle(2, device=pl.DEVICE_NONE, max_window_samples=4 * 65535, max_phase_avg=512)
    h.configure(0, [dict(samplesPerBaud=S, numAvg=4), dict(samplesPerBaud=S, numAvg=1)])
    assert h.query(0).samplesPerBaud == S and h.query(1).numAvg == 1
    # samplesPerBaud * numAvg above max_window_samples: still refused, nothing changed
    with pytest.raises(pl.PskSoftError) as e:
        h.configure(0, [dict(samplesPerBaud=S, numAvg=4 * 65535 // S + 1)])
    assert e.value.status == 4  # PSK_SOFT_ERR_LIMIT
    assert h.query(0).numAvg == 4
    h.close()


def _check_call(h, o, ch, rg, ro, ctx):
    assert rg["ret"] == ro.ret, ctx
    assert rg["n_symbols"] == ro.phase.size, ctx
    assert rg["n_bits"] == ro.bits.size, ctx
    assert rg["n_sampleIndex"] == ro.index.size, ctx
    assert rg["sri_pushed"] == ro.sri_pushed, ctx
    if ro.sri_pushed:
        assert _same(rg["sri_soft_xdelta"], ro.sri_soft_xdelta), ctx
        assert _same(rg["sri_bits_xdelta"], ro.sri_bits_xdelta), ctx
    assert rg["n_warn"] == ro.n_warn, ctx
    pk = h.peek(ch)
    assert pk["ring_len"] == o.ring_size, ctx
    assert pk["index"] == o.index, ctx
    assert pk["fit_len"] == o.fit_history().size, ctx


@pytest.mark.parametrize("S,A,n", [(1025, 3, 50), (2048, 4, 50), (4097, 2, 20), (32768, 1, 10), (65535, 2, 5), (2048, 3, 40000)])
def test_plans_follow_the_oracle_over_ragged_calls(oracle_mod, S, A, n):
    rng = np.random.default_rng(S + A)
    h = pl.Handle(1, device=pl.DEVICE_NONE, max_window_samples=max(S * A, 1 << 16), max_phase_avg=max(n + 1, 512))
    o = oracle_mod.OracleComponent()
    props = dict(samplesPerBaud=S, numAvg=A, phaseAvg=n, constelationSize=4)
    h.configure(0, [props])
    for k, v in props.items():
        setattr(o, k, v)
    fast = seq = 0
    for call in range(6):
        n_complex = int(S * rng.uniform(0.3, 5.0)) + int(rng.integers(0, 7))  # (not a multiple of samplesPerBaud)
        data = rng.standard_normal(2 * n_complex).astype(np.float32)
        ro = o.service(data, 0.01, sriChanged=(call == 0))
        rg = h.plan_only(0, [dict(n_floats=2 * n_complex, xdelta=0.01, sriChanged=(call == 0))])[0]
        _check_call(h, o, 0, rg, ro, "S %d call %d" % (S, call))
        st = h.stats()
        if rg["n_symbols"]:
            fast += st["channels_fast"]
            seq += st["channels_sequential"]
    assert fast + seq > 0
    if n <= 32640:
        assert seq == 0 and fast > 0, (fast, seq)
    else:
        assert fast == 0 and seq > 0, (fast, seq)
    h.close()


def test_emitting_wide_symbol_calls_are_planned_fast():
    h = pl.Handle(3, device=pl.DEVICE_NONE, max_window_samples=1 << 17, max_phase_avg=40001)
    h.configure(0, [dict(samplesPerBaud=2048, numAvg=4), dict(samplesPerBaud=3000, numAvg=2, phaseAvg=40000),
                    dict(samplesPerBaud=65535, numAvg=1)])
    h.plan_only(0, [dict(n_floats=2 * 70000, xdelta=0.01, sriChanged=True)] * 3)
    st = h.stats()
    assert st["channels_fast"] == 2 and st["channels_sequential"] == 1, st
    # force_sequential: the reference-order kernel for every channel
    h.set_force_sequential(1)
    h.plan_only(0, [dict(n_floats=2 * 70000, xdelta=0.01)] * 3)
    st = h.stats()
    assert st["channels_fast"] == 0 and st["channels_sequential"] == 3, st
    h.close()


def test_property_changes_mid_stream(oracle_mod):
    """samplesPerBaud 8 -> 3000 -> 8 and numAvg changes between calls: counts, SRI and state as the oracle's"""
    rng = np.random.default_rng(7)
    h = pl.Handle(1, device=pl.DEVICE_NONE, max_window_samples=1 << 19, max_phase_avg=512)
    o = oracle_mod.OracleComponent()
    steps = [dict(samplesPerBaud=8, numAvg=100), None, dict(samplesPerBaud=3000), None, dict(numAvg=5), None,
             dict(numAvg=2), dict(samplesPerBaud=8), None, dict(numAvg=50), None]
    for call, step in enumerate(steps):
        if step:
            h.configure(0, [step])
            for k, v in step.items():
                setattr(o, k, v)
        n_complex = int(rng.integers(100, 20000))
        data = rng.standard_normal(2 * n_complex).astype(np.float32)
        ro = o.service(data, 0.01, sriChanged=(call == 0))
        rg = h.plan_only(0, [dict(n_floats=2 * n_complex, xdelta=0.01, sriChanged=(call == 0))])[0]
        _check_call(h, o, 0, rg, ro, "call %d" % call)
    h.close()


def test_state_round_trip_of_a_wide_symbol_channel(oracle_mod):
    a = pl.Handle(2, device=pl.DEVICE_NONE, max_window_samples=1 << 16, max_phase_avg=512)
    b = pl.Handle(2, device=pl.DEVICE_NONE, max_window_samples=1 << 16, max_phase_avg=512)
    props = dict(samplesPerBaud=5000, numAvg=3, phaseAvg=30)
    a.configure(0, [props, props])
    a.plan_only(0, [dict(n_floats=2 * 23456, xdelta=0.01, sriChanged=True)] * 2)
    blob = a.export_state(1)
    b.import_state(0, blob)
    assert b.peek(0) == a.peek(1) and b.query(0).samplesPerBaud == 5000
    assert b.export_state(0) == blob
    pk = [dict(n_floats=2 * 7777, xdelta=0.01)]
    assert b.plan_only(0, pk) == a.plan_only(1, pk)
    assert b.peek(0) == a.peek(1)
    a.close()
    b.close()
