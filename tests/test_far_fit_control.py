"""PSK_SOFT_OPT_FAR_FIT on the control plane, without a GPU: phaseAvg 32641 .. 65535 ("far" fit windows) is planned for the
reference-order kernel by default and for the fast path (time-tiled kernels, fit window in device memory) with the option on,
whatever the window class; counters, SRI and state follow the oracle either way; the option is not part of a channel's state."""
import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests.test_wide_symbols_control import _check_call

OPT_FAR_FIT = 7


def _handle(n=1, window=1 << 16):
    return pl.Handle(n, device=pl.DEVICE_NONE, max_window_samples=window, max_phase_avg=65535)


def _emitting_call(h, S, A, n, first=True):
    """one call long enough to emit (samplesPerBaud 1 emits with numAvg 0 only); returns (n_symbols, stats)"""
    r = h.plan_only(0, [dict(n_floats=2 * S * (A + 300), xdelta=0.01, sriChanged=first)])[0]
    return r["n_symbols"], h.stats()


def test_default_handles_plan_far_windows_sequential():
    h = _handle()
    h.configure(0, [dict(samplesPerBaud=8, numAvg=10, phaseAvg=40000)])
    n_sym, st = _emitting_call(h, 8, 10, 40000)
    assert n_sym > 0 and st["channels_sequential"] == 1 and st["channels_fast"] == 0, st
    h.close()


@pytest.mark.parametrize("S", [1, 2, 8, 33, 2048])
@pytest.mark.parametrize("n", [32641, 32768, 65535])
def test_option_plans_far_windows_fast(S, n):
    A = 0 if S == 1 else 10
    h = _handle(window=max(1 << 16, S * 16))
    h.set_option(OPT_FAR_FIT, 1)
    h.configure(0, [dict(samplesPerBaud=S, numAvg=A, phaseAvg=n)])
    for call in range(2):
        n_sym, st = _emitting_call(h, S, A, n, first=(call == 0))
        assert n_sym > 0 and st["channels_fast"] == 1 and st["channels_sequential"] == 0, (call, st)
    # ... takes effect at the next call, both ways
    h.set_option(OPT_FAR_FIT, 0)
    n_sym, st = _emitting_call(h, S, A, n, first=False)
    assert n_sym > 0 and st["channels_fast"] == 0 and st["channels_sequential"] == 1, st
    h.close()


@pytest.mark.parametrize("opt", [0, 1])
def test_the_largest_lds_window_is_unchanged_either_way(opt):
    h = _handle()
    h.set_option(OPT_FAR_FIT, opt)
    h.configure(0, [dict(samplesPerBaud=8, numAvg=10, phaseAvg=32640)])
    n_sym, st = _emitting_call(h, 8, 10, 32640)
    assert n_sym > 0 and st["channels_fast"] == 1 and st["channels_sequential"] == 0, st
    h.close()


def test_other_values_are_refused_and_force_sequential_wins():
    h = _handle()
    h.configure(0, [dict(samplesPerBaud=8, numAvg=10, phaseAvg=40000)])
    h.set_option(OPT_FAR_FIT, 1)
    for bad in (2, -1):
        with pytest.raises(pl.PskSoftError) as e:
            h.set_option(OPT_FAR_FIT, bad)
        assert e.value.status == 1  # PSK_SOFT_ERR_INVALID_ARG
    n_sym, st = _emitting_call(h, 8, 10, 40000)
    assert n_sym > 0 and st["channels_fast"] == 1, st  # (the setting was kept)
    h.set_option(OPT_FAR_FIT, 0)
    for bad in (2, -1):
        with pytest.raises(pl.PskSoftError):
            h.set_option(OPT_FAR_FIT, bad)
    n_sym, st = _emitting_call(h, 8, 10, 40000, first=False)
    assert n_sym > 0 and st["channels_sequential"] == 1, st
    h.set_option(OPT_FAR_FIT, 1)
    h.set_force_sequential(1)
    n_sym, st = _emitting_call(h, 8, 10, 40000, first=False)
    assert n_sym > 0 and st["channels_fast"] == 0 and st["channels_sequential"] == 1, st
    h.close()


def test_environment_sets_the_default_of_new_handles(monkeypatch):
    monkeypatch.setenv("PSK_SOFT_FAR_FIT", "1")
    h = _handle()
    monkeypatch.setenv("PSK_SOFT_FAR_FIT", "0")
    h0 = _handle()
    monkeypatch.delenv("PSK_SOFT_FAR_FIT")
    for hh, fast in ((h, 1), (h0, 0)):
        hh.configure(0, [dict(samplesPerBaud=8, numAvg=10, phaseAvg=40000)])
        n_sym, st = _emitting_call(hh, 8, 10, 40000)
        assert n_sym > 0 and st["channels_fast"] == fast and st["channels_sequential"] == 1 - fast, st
        hh.close()


# (1, 1, 32641): one sample per symbol emits with numAvg 0 only -- that configuration emits nothing, the one behind it does
@pytest.mark.parametrize("S,A,n", [(8, 100, 65535), (2048, 3, 40000), (1, 1, 32641), (1, 0, 32641)])
def test_plans_follow_the_oracle_over_ragged_calls(oracle_mod, S, A, n):
    rng = np.random.default_rng(S + A + n)
    h = _handle(window=max(S * A, 1 << 16))
    h.set_option(OPT_FAR_FIT, 1)
    o = oracle_mod.OracleComponent()
    props = dict(samplesPerBaud=S, numAvg=A, phaseAvg=n, constelationSize=4)
    h.configure(0, [props])
    for k, v in props.items():
        setattr(o, k, v)
    fast = seq = emitted = 0
    for call in range(6):
        n_complex = int(S * max(A, 1) * rng.uniform(0.3, 2.5)) + int(rng.integers(0, 7))  # (not a multiple of samplesPerBaud)
        data = rng.standard_normal(2 * n_complex).astype(np.float32)
        ro = o.service(data, 0.01, sriChanged=(call == 0))
        rg = h.plan_only(0, [dict(n_floats=2 * n_complex, xdelta=0.01, sriChanged=(call == 0))])[0]
        _check_call(h, o, 0, rg, ro, "S %d call %d" % (S, call))
        st = h.stats()
        if rg["n_symbols"]:
            emitted += 1
            fast += st["channels_fast"]
            seq += st["channels_sequential"]
    assert seq == 0 and fast == emitted, (fast, seq, emitted)
    assert emitted > 0 or (S == 1 and A != 0)
    h.close()


def test_a_call_longer_than_2_to_the_20_symbols_is_cut_into_continuations():
    h = _handle()
    h.set_option(OPT_FAR_FIT, 1)
    h.configure(0, [dict(samplesPerBaud=1, numAvg=0, phaseAvg=40000)])
    n_sym = (1 << 20) + 5000
    r = h.plan_only(0, [dict(n_floats=2 * n_sym, xdelta=0.01, sriChanged=True)])[0]
    st = h.stats()
    assert r["n_symbols"] == n_sym and st["channels_sequential"] == 0 and st["channels_fast"] == 1, (r, st)
    # ... as for a window the LDS holds; with the option off the far window stays one sequential call
    h.set_option(OPT_FAR_FIT, 0)
    r = h.plan_only(0, [dict(n_floats=2 * n_sym, xdelta=0.01)])[0]
    st = h.stats()
    assert r["n_symbols"] == n_sym and st["channels_sequential"] == 1, (r, st)
    h.close()


def test_the_option_is_not_part_of_a_channels_state():
    on, off = _handle(), _handle()
    on.set_option(OPT_FAR_FIT, 1)
    props = dict(samplesPerBaud=8, numAvg=10, phaseAvg=50000)
    for h in (on, off):
        h.configure(0, [props])
    lens = (8 * 700 + 3, 8 * 1300 + 5, 8 * 41 + 1)
    for k, n in enumerate(lens):
        for h in (on, off):
            h.plan_only(0, [dict(n_floats=2 * n, xdelta=0.01, sriChanged=(k == 0))])
    blob_on, blob_off = on.export_state(0), off.export_state(0)
    assert blob_on == blob_off
    off.import_state(0, blob_on)  # option-on -> option-off
    on.import_state(0, blob_off)  # ... and back
    assert on.export_state(0) == off.export_state(0) == blob_on
    pk = dict(n_floats=2 * (8 * 500 + 7), xdelta=0.01)
    r_on, r_off = on.plan_only(0, [pk])[0], off.plan_only(0, [pk])[0]
    assert r_on == r_off and r_on["n_symbols"] > 0
    assert on.peek(0) == off.peek(0)
    s_on, s_off = on.stats(), off.stats()
    assert s_on["channels_fast"] == 1 and s_on["channels_sequential"] == 0, s_on
    assert s_off["channels_fast"] == 0 and s_off["channels_sequential"] == 1, s_off
    assert on.export_state(0) == off.export_state(0)
    on.close()
    off.close()
