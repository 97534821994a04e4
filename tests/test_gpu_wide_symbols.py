"""samplesPerBaud 1025 .. 65535 on a real MI355X: the wide front stage (psk_wide.hip) behind the time-tiled kernels, and the
reference-order kernel's wide build for what those hand over, bit for bit (uint32 patterns) against the oracle, call by call."""
import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

KEYS = ("soft", "bits", "phase", "index")


def psk_signal(rng, S, n_sym, M, offset=None, noise=0.05, freq=3e-5):
    """n_sym M-PSK symbols, rectangular pulses of S samples with a raised middle (the timing peak), a carrier offset and
    noise: complex64 interleaved as float32 I/Q"""
    sym = np.exp(1j * (2 * np.pi * rng.integers(0, M, n_sym) / M + np.pi / 4))
    k = np.arange(S)
    off = rng.integers(0, S) if offset is None else offset
    shape = 1.0 + 0.5 * np.exp(-(((k - off + S // 2) % S - S // 2) / (0.15 * S)) ** 2)
    x = (sym[:, None] * shape[None, :]).ravel()
    x = x * np.exp(1j * freq * np.arange(x.size)) + noise * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    out = np.empty(2 * x.size, np.float32)
    out[0::2], out[1::2] = x.real, x.imag
    return out


def cuts_of(rng, n_complex, k):
    c = sorted(set([0, n_complex] + [int(v) for v in rng.integers(1, n_complex, k - 1)]))
    return list(zip(c[:-1], c[1:]))


def run_both(oracle_mod, h, chans, xdelta=0.01, fmt=None):
    """chans: list of (props, data, cuts) -- the same number of calls each; every channel of handle h, one call per piece.
    Returns the handle's stats after each call."""
    orc = []
    for props, _, _ in chans:
        o = oracle_mod.OracleComponent()
        for k, v in props.items():
            setattr(o, k, v)
        orc.append(o)
    h.configure(0, [p for p, _, _ in chans])
    stats = []
    for call in range(len(chans[0][2])):
        pk = []
        for c, (props, data, cuts) in enumerate(chans):
            a, b = cuts[call]
            seg = data[2 * a : 2 * b]
            pk.append(dict(data=seg if fmt is None else fmt(seg), xdelta=xdelta, sriChanged=(call == 0)))
        got = h.process_host(0, pk)
        stats.append(h.stats())
        for c, (props, data, cuts) in enumerate(chans):
            seg = pk[c]["data"].astype(np.float32)
            r = orc[c].service(seg, xdelta, sriChanged=(call == 0))
            ref = dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index)
            assert_parity({k: got[c][k] for k in KEYS}, ref, "channel %d call %d %s" % (c, call, props))
    return stats


def _handle(n, window, phase_avg=512):
    return pl.Handle(n, device=0, max_window_samples=window, max_phase_avg=phase_avg, max_packet_complex=1 << 23)


CASES = [(S, M, diff) for S in (1025, 1100, 2048, 4097, 32768, 40000, 65535) for M in (2, 4, 8) for diff in (0, 1)
         if S <= 4097 or diff == (M == 4)]


@pytest.mark.parametrize("S,M,diff", CASES)
def test_wide_symbols_match_the_oracle(oracle_mod, S, M, diff):
    rng = np.random.default_rng(S * 16 + M * 2 + diff)
    A = 3 if S <= 4097 else 2
    n_sym = 300 if S <= 4097 else 60
    data = psk_signal(rng, S, n_sym, M)
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=20, differentialDecoding=diff)
    h = _handle(1, S * A)
    stats = run_both(oracle_mod, h, [(props, data, cuts_of(rng, data.size // 2, 4))])
    assert all(st["channels_sequential"] == 0 and st["channels_guard"] == 0 for st in stats), stats
    assert any(st["channels_tiled"] == 1 for st in stats), stats
    h.close()


def _tie_signal(rng, S, n_sym, levels):
    """integer samples: every symbol a QPSK point times an integer amplitude per phase (levels: phase -> amplitude, 1 elsewhere),
    so that every window sum is exact and equal sums are exact ties"""
    amp = np.ones(S)
    for k, v in levels.items():
        amp[k] = v
    sym = np.array([1, 1j, -1, -1j])[rng.integers(0, 4, n_sym)]
    x = (sym[:, None] * amp[None, :]).ravel()
    out = np.empty(2 * x.size, np.float32)
    out[0::2], out[1::2] = x.real, x.imag
    return out


@pytest.mark.parametrize("S,levels", [
    (2048, {1023: 2, 1024: 2}),          # a tie across the first chunk boundary: the first phase wins
    (2048, {1023: 2, 1024: 3}),
    (3000, {5: 2, 1024: 2, 2047: 2, 2048: 2}),
    (32768, {16383: 3, 16384: 3}),       # across the 16th chunk boundary
    (40000, {35000: 2, 39999: 2}),       # picks above 32767: negative sampleIndex values
    (65535, {65534: 2}),
])
def test_exact_ties_and_picks_across_chunks(oracle_mod, S, levels):
    rng = np.random.default_rng(S + len(levels))
    n_sym = 200 if S <= 4096 else 40
    data = _tie_signal(rng, S, n_sym, levels)
    h = _handle(1, 2 * S)
    stats = run_both(oracle_mod, h, [(dict(samplesPerBaud=S, constelationSize=4, numAvg=2, phaseAvg=10), data,
                                      cuts_of(rng, data.size // 2, 3))])
    assert all(st["channels_guard"] == 0 for st in stats), stats
    h.close()


def test_nonfinite_sample_goes_to_the_reference_order_kernel(oracle_mod):
    rng = np.random.default_rng(5)
    S = 2048
    data = psk_signal(rng, S, 300, 4)
    data[2 * (S * 100 + 77)] = np.nan
    data[2 * (S * 200 + 3) + 1] = np.inf
    h = _handle(1, 4 * S)
    stats = run_both(oracle_mod, h, [(dict(samplesPerBaud=S, numAvg=3, phaseAvg=20), data, cuts_of(rng, data.size // 2, 3))])
    assert sum(st["channels_guard"] for st in stats) >= 1, stats
    h.close()


def test_force_sequential_and_long_fit_windows(oracle_mod):
    rng = np.random.default_rng(6)
    h = _handle(1, 4 * 5000)
    h.set_force_sequential(1)
    data = psk_signal(rng, 5000, 200, 8)
    stats = run_both(oracle_mod, h, [(dict(samplesPerBaud=5000, constelationSize=8, numAvg=2, phaseAvg=30), data,
                                      cuts_of(rng, data.size // 2, 3))])
    assert all(st["channels_fast"] == 0 for st in stats), stats
    h.close()
    # phaseAvg beyond what the time-tiled kernels hold: the reference-order kernel, wide build
    h = _handle(1, 4 * 2048, phase_avg=40001)
    data = psk_signal(rng, 2048, 300, 4)
    stats = run_both(oracle_mod, h, [(dict(samplesPerBaud=2048, numAvg=3, phaseAvg=40000), data, cuts_of(rng, data.size // 2, 3))])
    assert any(st["channels_sequential"] == 1 for st in stats), stats
    h.close()


def test_one_call_mixes_narrow_and_wide_symbols(oracle_mod):
    rng = np.random.default_rng(8)
    chans = []
    for S, A in ((8, 100), (40, 20), (2048, 3), (1500, 2)):
        n_sym = 150000 // S + 200
        data = psk_signal(rng, S, n_sym, 4)
        n = data.size // 2
        chans.append((dict(samplesPerBaud=S, numAvg=A, phaseAvg=20), data, [(0, n // 3), (n // 3, n // 2), (n // 2, n)]))
    h = _handle(len(chans), 4 * 2048)
    run_both(oracle_mod, h, chans)
    h.close()


def test_cs16_packets_of_wide_symbols(oracle_mod):
    rng = np.random.default_rng(9)
    S = 4097
    data = psk_signal(rng, S, 200, 4)
    q = np.clip(np.rint(data.astype(np.float64) * 8192), -32768, 32767).astype(np.int16)
    h = _handle(1, 3 * S)
    run_both(oracle_mod, h, [(dict(samplesPerBaud=S, numAvg=3, phaseAvg=20), q, cuts_of(rng, q.size // 2, 3))])
    h.close()


@pytest.mark.parametrize("n_ch", [1, 64])
def test_many_channels_and_the_parallel_fit(oracle_mod, n_ch):
    rng = np.random.default_rng(10 + n_ch)
    S = 2048
    chans = []
    for c in range(n_ch):
        data = psk_signal(rng, S, 400, 4, noise=0.02)
        chans.append((dict(samplesPerBaud=S, numAvg=4, phaseAvg=8), data, [(0, 100 * S + 5), (100 * S + 5, 250 * S), (250 * S, 400 * S)]))
    h = _handle(n_ch, 4 * S)
    stats = run_both(oracle_mod, h, chans)
    assert stats[-1]["channels_parallel_fit"] > 0, stats
    assert all(st["channels_guard"] == 0 and st["channels_sequential"] == 0 for st in stats), stats
    h.close()


def test_launch_trace_names_the_wide_kernels(oracle_mod, capfd, monkeypatch):
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    rng = np.random.default_rng(11)
    data = psk_signal(rng, 3000, 200, 4)
    h = _handle(1, 3 * 3000)
    stats = run_both(oracle_mod, h, [(dict(samplesPerBaud=3000, numAvg=3, phaseAvg=20), data, cuts_of(rng, data.size // 2, 2))])
    h.close()
    err = capfd.readouterr().err
    assert "next: wide_front" in err and "next: tile_fit (wide)" in err, err[-2000:]
    assert "next: tile_front_any" not in err
    assert all(st["channels_guard"] == 0 and st["channels_sequential"] == 0 for st in stats), stats


def test_host_class_configured_by_property(oracle_mod):
    from psk_soft_amd import sandbox

    rng = np.random.default_rng(12)
    S = 2000
    data = psk_signal(rng, S, 200, 2)
    comp = sandbox.Component(device=0)
    comp.numAvg = 4  # (first: the default numAvg of 100 at 2000 samples a symbol is beyond the component's window of 65536 samples)
    comp.samplesPerBaud = S
    comp.constelationSize = 2
    comp.phaseAvg = 20
    o = oracle_mod.OracleComponent()
    o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = S, 2, 4, 20
    n = data.size // 2
    for k, (a, b) in enumerate([(0, n // 2), (n // 2, n)]):
        seg = data[2 * a : 2 * b]
        comp.push(seg, xdelta=0.01, sriChanged=(k == 0))
        comp.service()
        r = o.service(seg, 0.01, sriChanged=(k == 0))
        got = dict(soft=comp.getData("softDecision_dataFloat_out"), bits=comp.getData("bits_dataShort_out"),
                   phase=comp.getData("phase_dataFloat_out"), index=comp.getData("sampleIndex_dataShort_out"))
        assert_parity(got, dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index), "host class call %d" % k)
    comp.close()
