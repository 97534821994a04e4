"""Complex binary16 packets (PSK_SOFT_FORMAT_CF16: interleaved IEEE half I/Q, torch.complex32) on a real MI355X: every stream bit
for bit what the oracle gives on x.astype(np.float32) of the same halves -- the widening is exact --, through every entry point,
kernel family and schedule: the host-buffer path, device-resident packets from a torch.complex32 tensor, zero-copy from
page-locked memory at 4-byte alignment, calls the library cuts, the deferred join, pipelined ranges, the strided entry, the
quality records.  What only half precision brings is tested on purpose: subnormal halves (never flushed), every finite encoding,
amplitudes up to 65504, infinities and quiet NaNs.  Signalling-NaN encodings are outside the contract and never used."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tests.test_gpu_cs8 as t_cs8
import tests.test_gpu_quality as t_quality
import tests.test_gpu_strided as t_strided
from tests.test_gpu_cs16 import _cut, _tie_streams, _window_class_cfgs
from tests.test_gpu_cs16_schedules import (KEYS, H_CS16, _mixed_cut_batch, _synth, assert_same, check_parity, host_run, oracle_calls,
                                           parse_trace, rounds, screened, untraced_then_traced, whats)
from tests.test_gpu_cs8 import H_CS8, device_run, q8
from tests.test_gpu_parity import assert_parity
from tests.test_gpu_strided import contiguous, gathers, strided_run

pytestmark = pytest.mark.gpu

H_CF16 = 6  # the window class of CF16 packets read in place (psk_ctl.h: kPktFormats)
F16 = np.dtype(np.float16)


def h16(x):
    """float I/Q -> half I/Q, round to nearest even"""
    return np.asarray(x, np.float32).astype(np.float16)


def bits16(u):
    """half values from their encodings"""
    return np.asarray(u, np.uint16).view(np.float16)


@pytest.fixture(autouse=True)
def _half_packets_in_the_shared_helpers(monkeypatch):
    """the helpers of the sc8, strided and quality files take a packet's format from its dtype: teach them float16"""
    from psk_soft_amd import lib as pl

    fmt8, fmts, fmtq, poison = t_cs8._fmt, t_strided._fmt, t_quality._fmt, t_strided._poison
    monkeypatch.setattr(t_cs8, "_fmt", lambda x: pl.FORMAT_CF16 if x.dtype == F16 else fmt8(x))
    monkeypatch.setattr(t_quality, "_fmt", lambda x: pl.FORMAT_CF16 if x.dtype == F16 else fmtq(x))
    monkeypatch.setattr(t_strided, "_fmt", lambda p, dt: p.FORMAT_CF16 if np.dtype(dt) == F16 else fmts(p, dt))
    monkeypatch.setattr(t_strided, "_poison", lambda dt: bits16(0x7E55)[()] if np.dtype(dt) == F16 else poison(dt))


def _joined(got):
    return {k: np.concatenate([g[k] for g in got]) for k in KEYS}


def _oracle(oracle_mod, props, pieces):
    return _joined(oracle_calls(oracle_mod, props, pieces)[0])


@pytest.mark.parametrize("name", ["testDiffDecode8PSK", "testDiffDecodeBPSK", "testDiffDecodeQPSK",
                                  "testNonDiffDecode8PSK", "testNonDiffDecodeBPSK", "testNonDiffDecodeQPSK"])
def test_reference_component_scenarios_rounded_to_half(oracle_mod, name):
    from psk_soft_amd import lib as pl
    from tests.test_oracle_reference_kat import reference_stimuli

    M, diff, data, _ = reference_stimuli()[name]
    iq = h16(data)
    props = dict(samplesPerBaud=8, constelationSize=M, numAvg=100, differentialDecoding=int(diff))
    h = pl.Handle(1, device=0)
    h.configure(0, [props])
    n = iq.size // 2
    pieces = _cut(iq, [0, n // 3, n // 3 + 1001, n])
    got, _ = host_run(h, [[p] for p in pieces])
    assert h.stats()["channels_fast"] == 1
    h.close()
    assert_parity(_joined(got[0]), _oracle(oracle_mod, props, pieces), name)


def _torch_batch_child(path):
    """(a fresh process, torch initialised before the library) 4096 channels x 2^16 samples of one torch.complex32 tensor
    through psk_soft_process_device, two calls, as CF16 (the tensor as it lies: torch.view_as_real) and as CF32 of the widened
    values, then CF16 again on a handle with the launch trace on; saves the stimulus and outputs of a few channels, the stats
    and the comparisons to `path`"""
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    C, N, S, M = 4096, 1 << 16, 8, 4
    dev = torch.device("cuda", 0)
    z = torch.view_as_complex(synth_channels_torch(C, M, S, 2 * N, dev).to(torch.float16).view(C, 2 * N, 2).contiguous())
    assert z.dtype == torch.complex32 and z.shape == (C, 2 * N)
    iq16 = torch.view_as_real(z).view(C, 4 * N)  # (the recipe of INTEGRATION.md: interleaved half I/Q, no copy)
    assert iq16.dtype == torch.float16 and iq16.data_ptr() == z.data_ptr()
    forms = {pl.FORMAT_CF16: iq16, pl.FORMAT_CF32: iq16.to(torch.float32).contiguous()}
    cap = (N // S + 2 + 63) // 64 * 64
    check = [0, 1, 777, 2048, C - 1]
    save = {"check": np.array(check), "iq": iq16[check].cpu().numpy()}

    def run(fmt, trace):
        src = forms[fmt]
        esz = src.element_size()
        out_t = [torch.empty((2, C, 2 * cap), dtype=torch.float32, device=dev), torch.empty((2, C, cap), dtype=torch.float32, device=dev),
                 torch.empty((2, C, cap), dtype=torch.int16, device=dev), torch.empty((2, C, 2 * cap), dtype=torch.int16, device=dev)]
        for t in out_t:
            t.zero_()
        torch.cuda.synchronize()
        if trace:
            os.environ["PSK_SOFT_TRACE_LAUNCHES"] = "2"
        h = pl.Handle(C, device=0)
        os.environ.pop("PSK_SOFT_TRACE_LAUNCHES", None)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)
        stats = []
        ns = []
        for k in range(2):
            pk = (pl.Packet * C)()
            out = (pl.Output * C)()
            for c in range(C):
                pk[c].data = src[c].data_ptr() + k * 2 * N * esz
                pk[c].n_floats = 2 * N
                pk[c].sri_xdelta = 0.01
                pk[c].sri_mode = 1
                pk[c].sriChanged = int(k == 0)
                pk[c].present = 1
                pk[c].format = fmt
                out[c].soft = out_t[0][k, c].data_ptr()
                out[c].phase = out_t[1][k, c].data_ptr()
                out[c].sampleIndex = out_t[2][k, c].data_ptr()
                out[c].bits = out_t[3][k, c].data_ptr()
                out[c].cap_symbols = cap
            if trace:
                sys.stderr.write("[cf16-test] call %d\n" % k)
                sys.stderr.flush()
            h.process_device(0, pk, out)
            h.synchronize()
            stats.append(h.stats())
            ns.append([int(out[c].n_symbols) for c in range(C)])
        h.close()
        return out_t, stats, ns

    res = {fmt: run(fmt, False) for fmt in (pl.FORMAT_CF16, pl.FORMAT_CF32)}
    res["trace"] = run(pl.FORMAT_CF16, True)
    base, sth, nsh = res[pl.FORMAT_CF16]
    same = {}
    for key, (outs, st, ns) in res.items():
        same[str(key)] = bool(ns == nsh and all(torch.equal(a.view(torch.int16 if a.dtype == torch.int16 else torch.int32),
                                                            b.view(torch.int16 if b.dtype == torch.int16 else torch.int32))
                                                for a, b in zip(outs, base)))
    save["same"] = np.array([same[str(pl.FORMAT_CF32)], same["trace"]])
    save["seq"] = np.array([s["channels_sequential"] for s in sth])
    save["fast"] = np.array([s["channels_fast"] for s in sth])
    for c in check:
        for k in range(2):
            n = nsh[k][c]
            save["soft_%d_%d" % (c, k)] = base[0][k, c, : 2 * n].cpu().numpy()
            save["phase_%d_%d" % (c, k)] = base[1][k, c, :n].cpu().numpy()
            save["index_%d_%d" % (c, k)] = base[2][k, c, :n].cpu().numpy()
            save["bits_%d_%d" % (c, k)] = base[3][k, c, : 2 * n].cpu().numpy()
    np.savez(path, **save)


def test_device_batch_from_a_torch_complex32_tensor(oracle_mod, tmp_path):
    """4096 channels x 2^16 samples, QPSK, S = 8, numAvg 100: the complex32 tensor as it lies and the CF32 tensor of the widened
    values give identical bits, no channel leaves the wave-scan kernels, and the launch trace shows the CF16 in-place class
    (H=6) in both tiers and no pre-pass.  (In a child process of its own: torch initialises its HIP runtime first there.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "batch.npz")
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_cf16 as t; t._torch_batch_child(%r)" % path], cwd=root,
                       capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = np.load(path)
    assert d["same"].tolist() == [True, True]
    assert d["seq"].tolist() == [0, 0] and d["fast"].tolist() == [4096, 4096]
    err = r.stderr.decode()
    calls = err.split("[cf16-test] call ")[1:]
    assert len(calls) == 2
    for text in calls:
        lines = parse_trace(text)
        w = whats(lines)
        assert not w & {"cf16_convert", "cs8_convert", "cs16_convert", "tile_front"}, w
        assert screened(lines) == {(8, H_CF16): 1}, lines
        assert all(t["H"] == H_CF16 for t in lines if t["what"].startswith("fast (")), lines
    props = dict(samplesPerBaud=8, constelationSize=4, numAvg=100, phaseAvg=50)
    N = 1 << 16
    assert d["iq"].dtype == np.float16
    for i, c in enumerate(d["check"].tolist()):
        got = {key: np.concatenate([d["%s_%d_%d" % (key, c, k)] for k in range(2)]) for key in KEYS}
        assert_parity(got, _oracle(oracle_mod, props, [d["iq"][i, : 2 * N], d["iq"][i, 2 * N :]]), "channel %d" % c)


def test_every_window_class_in_one_mixed_cf16_batch(oracle_mod, monkeypatch, capfd):
    """samplesPerBaud 2 .. 32, 33 and 100, numAvg 1 .. 1025, phaseAvg 50 / 4000: one batch, three calls with ragged cuts and
    odd element counts, time tiling off.  The launch trace says which classes ran where: numAvg <= 128 with samplesPerBaud
    2 .. 16 and phaseAvg 50 in place (H=6), every other class behind the pre-pass (cf16_convert) on the float kernels."""
    from psk_soft_amd.stimulus import synth_channel

    cfgs = _window_class_cfgs()
    C = len(cfgs)
    rng = np.random.default_rng(14)
    pieces = []
    for c, p in enumerate(cfgs):
        S, A = p["samplesPerBaud"], p["numAvg"]
        n = S * (A + 300) + int(rng.integers(0, 4000))
        iq = h16(synth_channel(71000 + c, p["constelationSize"], S, n))
        a, b = sorted(rng.choice(np.arange(1, n), 2, replace=False))
        segs = _cut(iq, [0, a, b, n])
        segs[0] = np.concatenate([segs[0], np.float16([12.5])])  # an odd element: ignored
        segs[2] = np.concatenate([segs[2], np.float16([-5])])
        pieces.append(segs)
    data = [[pieces[c][k] for c in range(C)] for k in range(3)]

    def run(h, cf):
        h.configure(0, cfgs)
        got, traces = host_run(h, data, cf)
        assert h.stats()["channels_sequential"] == 0
        return got, traces

    res = untraced_then_traced(monkeypatch, capfd, dict(PSK_SOFT_TIME_TILED=0), C, run, max_window_samples=65536 + 64, max_phase_avg=4096)
    in_place = {p["samplesPerBaud"] for p in cfgs if p["samplesPerBaud"] <= 16 and p["numAvg"] <= 128 and p["phaseAvg"] == 50}
    seen = set()
    for k, lines in enumerate(res[1][1]):
        assert "cf16_convert" in whats(lines) and not whats(lines) & {"cs16_convert", "cs8_convert"}, (k, whats(lines))
        fast = {(t["S"], t["H"]) for t in lines if t["what"].startswith("fast (")}
        assert not any(H in (H_CS16, H_CS8) for _, H in fast), (k, fast)
        assert all(S in in_place for S, H in fast if H == H_CF16), (k, fast)
        seen |= {S for S, H in fast if H == H_CF16}
        # the classes the in-place builds do not cover ran on the float kernels: deeper histories, wider symbols, deep fits
        assert {H for _, H in fast} >= {2, 4, 8}, (k, fast)
        assert any(S > 16 and H == 1 for S, H in fast), (k, fast)
    assert seen == in_place, (seen, in_place)
    for c, p in enumerate(cfgs):
        assert_parity(_joined(res[0][0][c]), _oracle(oracle_mod, p, pieces[c]), "cfg %s" % p)


@pytest.mark.parametrize("ties_in_place", [1, 0])
@pytest.mark.parametrize("numAvg", [100, 400])
def test_exact_energy_ties_of_small_integers_in_half(oracle_mod, monkeypatch, ties_in_place, numAvg):
    """The tie streams of the integer formats cast to half: small integers are exact in half, the window sums of their
    squares are exact and tie all the time.  The exact tier runs, and decides them as the reference does."""
    from psk_soft_amd import lib as pl

    monkeypatch.setenv("PSK_SOFT_TIES_IN_PLACE", str(ties_in_place))
    S, N = 8, 20000
    streams = [x.astype(np.float16) for x in _tie_streams(N, S)]
    assert all(np.isfinite(x).all() for x in streams)
    props = dict(samplesPerBaud=S, constelationSize=4, numAvg=numAvg)
    h = pl.Handle(len(streams), device=0)
    h.configure(0, [props] * len(streams))
    pieces = [_cut(x, [0, 7001, N]) for x in streams]
    got = {c: [] for c in range(len(streams))}
    exact = 0
    for k in range(2):
        g, _ = host_run(h, [[pieces[c][k] for c in range(len(streams))]], k0=k)
        for c in got:
            got[c] += g[c]
        st = h.stats()
        exact += st["timing_exact_blocks"] + st["channels_exact_timing"]
    assert exact > 0
    h.close()
    for c in range(len(streams)):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, props, pieces[c]), "tie stream %d" % c)


def _run_three_ways(oracle_mod, monkeypatch, capfd, x, S, M, cuts, ctx):
    """one stream three ways -- read in place (numAvg 100, time tiling off), through the pre-pass (numAvg 300) and time-tiled
    (numAvg 100) --, each against the oracle; the launch traces say that each path ran"""
    from psk_soft_amd import lib as pl

    pieces = _cut(x, cuts)
    data = [[p] for p in pieces]
    out = {}
    for way, A, tiled in (("in place", 100, 0), ("pre-pass", 300, 0), ("time-tiled", 100, 2)):
        props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=50)

        def run(h, cf):
            h.configure(0, [props])
            h.set_option(pl.Handle.OPT_TIME_TILED, tiled)
            return device_run(h, data, cf)

        res = untraced_then_traced(monkeypatch, capfd, {}, 1, run)
        lines = [t for tr in res[1][1] for t in tr]
        if way == "in place":
            assert (S, H_CF16) in screened(lines) and not whats(lines) & {"cf16_convert", "tile_front"}, lines
        elif way == "pre-pass":
            assert (S, 4) in screened(lines) and "cf16_convert" in whats(lines), lines
        else:
            assert {"cf16_convert", "tile_front"} <= whats(lines) and not any(t["H"] == H_CF16 for t in lines), lines
        ref = _oracle(oracle_mod, props, pieces)
        assert_parity(_joined(res[0][0][0]), ref, "%s, %s" % (ctx, way))
        out[way] = ref
    return out


def test_a_stream_of_subnormal_halves(oracle_mod, monkeypatch, capfd):
    """Every sample a subnormal half (+-1 .. 1023 x 2^-24): QPSK pulses in that range with noise.  Widened they are normal
    floats; a kernel that flushed them would see silence.  The outputs are the oracle's, and not those of a zero stream."""
    from psk_soft_amd.stimulus import synth_channel

    S, M, N = 8, 4, 24000
    x = synth_channel(72000, M, S, N)
    k = np.clip(np.rint(x / np.abs(x).max() * 1000.0), -1023, 1023).astype(np.int32)
    k[k == 0] = 1
    enc = (np.abs(k) | np.where(k < 0, 0x8000, 0)).astype(np.uint16)
    xh = bits16(enc)
    assert ((enc & 0x7C00) == 0).all() and ((enc & 0x3FF) != 0).all()
    assert np.array_equal(xh.astype(np.float64), k * 2.0 ** -24)
    refs = _run_three_ways(oracle_mod, monkeypatch, capfd, xh, S, M, [0, 9001, N], "subnormal halves")
    for way, ref in refs.items():
        assert np.abs(ref["soft"]).max() > 0, way


def test_every_finite_half_encoding_once(oracle_mod, monkeypatch, capfd):
    """One stream that uses each of the 63 488 finite encodings (both zeros, all subnormals, up to +-65504) exactly once, in a
    random order, at samplesPerBaud 2: in place, through the pre-pass and time-tiled."""
    u = np.arange(65536, dtype=np.uint32)
    enc = u[(u & 0x7C00) != 0x7C00].astype(np.uint16)
    assert enc.size == 63488
    np.random.default_rng(15).shuffle(enc)
    x = bits16(enc)
    assert np.isfinite(x).all()
    _run_three_ways(oracle_mod, monkeypatch, capfd, x, 2, 4, [0, 10001, enc.size // 2], "every finite encoding")


def test_full_range_amplitudes_with_8psk(oracle_mod):
    """8-PSK at amplitudes up to the largest half, 65504 (energies of 4e9, window sums of 1e12, |z|^8 beyond float range),
    in place and through the pre-pass; two calls."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    S, M, N = 8, 8, 30000
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=50, differentialDecoding=d) for A, d in ((100, 0), (400, 1), (64, 1))]
    streams = []
    for c in range(len(props)):
        x = synth_channel(73000 + c, M, S, N)
        xh = h16(np.clip(x * (65504.0 / np.abs(x).max()), -65504.0, 65504.0))
        assert np.isfinite(xh).all() and np.abs(xh.astype(np.float32)).max() == 65504.0
        streams.append(xh)
    pieces = [_cut(x, [0, 11003, N]) for x in streams]
    h = pl.Handle(len(props), device=0)
    h.configure(0, props)
    got, _ = host_run(h, [[pieces[c][k] for c in range(len(props))] for k in range(2)])
    assert h.stats()["channels_sequential"] == 0
    h.close()
    for c, p in enumerate(props):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, p, pieces[c]), "full range %s" % p)


def test_infinities_and_quiet_nans(oracle_mod):
    """+-inf and the quiet NaNs 0x7e00, 0xfe00, 0x7e01 inside otherwise clean channels, as runs of I (or Q) samples and as
    single samples, in place and through the pre-pass; device-resident and host-buffer entry."""
    from psk_soft_amd import lib as pl

    S, n = 8, 16000
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=50, differentialDecoding=d)
             for M, d, A in ((2, 0, 100), (4, 0, 100), (8, 1, 100), (4, 1, 300), (8, 0, 300))]
    C = len(props)
    host = [h16(x).copy() for x in _synth(74000, [p["constelationSize"] for p in props], S, 2 * n)]
    bad = bits16([0x7E00, 0x7C00, 0xFE00, 0xFC00, 0x7E01])
    rng = np.random.default_rng(8)
    for c in range(C):
        for j, v in enumerate(bad):
            at = 2 * (3000 + 2500 * j) + c % 2
            host[c][at:at + 2 * S * 3:2] = v
            host[c][int(rng.integers(34000, 60000))] = v
    calls = [[host[c][:2 * n] for c in range(C)], [host[c][2 * n:] for c in range(C)]]
    for entry in ("device", "host"):
        h = pl.Handle(C, device=0)
        try:
            h.configure(0, props)
            got = device_run(h, calls)[0] if entry == "device" else host_run(h, calls)[0]
            assert h.stats()["channels_sequential"] == 0
        finally:
            h.close()
        check_parity(oracle_mod, got, lambda c: props[c], calls, "non-finite halves, %s entry" % entry)
        assert any(not np.isfinite(g["soft"]).all() for c in got for g in got[c])


@pytest.mark.parametrize("n_ch", [1, 64])
def test_time_tiled_and_parallel_fit(oracle_mod, n_ch):
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    N, S, M = 1 << 18, 8, 4
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)
    streams = [h16(synth_channel(75000 + c, M, S, N)) for c in range(n_ch)]
    h = pl.Handle(n_ch, device=0)
    h.configure(0, [props] * n_ch)
    h.set_option(pl.Handle.OPT_TIME_TILED, 2)
    pieces = [_cut(x, [0, 5000, N]) for x in streams]
    got, _ = host_run(h, [[pieces[c][k] for c in range(n_ch)] for k in range(2)])
    st = h.stats()
    assert st["channels_tiled"] == n_ch and st["channels_parallel_fit"] > 0, st
    h.close()
    for c in sorted({0, n_ch // 2, n_ch - 1}):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, props, pieces[c]), "ch %d" % c)


def test_wide_symbols(oracle_mod):
    """samplesPerBaud 2048 (the wide-symbol front stage, through the pre-pass), two channels, three calls."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    S, M, A = 2048, 4, 4
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=20), dict(samplesPerBaud=S, constelationSize=2, numAvg=1)]
    N = S * 700
    streams = [h16(synth_channel(76000 + c, p["constelationSize"], S, N)) for c, p in enumerate(props)]
    pieces = [_cut(x, [0, S * 100 + 77, S * 400, N]) for x in streams]
    h = pl.Handle(2, device=0, max_window_samples=S * A + 64, max_packet_complex=N)
    h.configure(0, props)
    got, _ = host_run(h, [[pieces[c][k] for c in range(2)] for k in range(3)])
    h.close()
    for c in range(2):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, props[c], pieces[c]), "wide ch %d" % c)


def test_reference_order_kernel(oracle_mod):
    """A forced-sequential handle: every CF16 channel through the reference-order kernel (the pre-pass in front of it)."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    cfgs = [(8, 4, 0), (10, 8, 1), (5, 2, 0), (1, 4, 0)]
    streams = [h16(synth_channel(77000 + c, M, S, 6000)) for c, (S, M, d) in enumerate(cfgs)]
    props = [dict(samplesPerBaud=S, constelationSize=M, differentialDecoding=d, numAvg=(0 if S == 1 else 100)) for S, M, d in cfgs]
    h = pl.Handle(len(cfgs), device=0)
    h.set_force_sequential(1)
    h.configure(0, props)
    pieces = [_cut(x, [0, 2500, 6000]) for x in streams]
    got, _ = host_run(h, [[pieces[c][k] for c in range(len(cfgs))] for k in range(2)])
    assert h.stats()["channels_sequential"] == len(cfgs)
    h.close()
    for c in range(len(cfgs)):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, props[c], pieces[c]), "cfg %s" % (cfgs[c],))


def _zero_copy(h, bufs, offs, n_elems, k, cap):
    """psk_soft_process_device on CF16 packets in page-locked memory: channel c's packet at bufs[c] + offs[c] bytes, n_elems[c]
    half elements; outputs in page-locked memory too"""
    from psk_soft_amd import lib as pl

    n_ch = len(bufs)
    soft = pl.host_alloc(n_ch * 2 * cap, np.float32).reshape(n_ch, 2 * cap)
    phase = pl.host_alloc(n_ch * cap, np.float32).reshape(n_ch, cap)
    sidx = pl.host_alloc(n_ch * cap, np.int16).reshape(n_ch, cap)
    bits = pl.host_alloc(n_ch * 3 * cap, np.int16).reshape(n_ch, 3 * cap)
    pk = (pl.Packet * n_ch)()
    out = (pl.Output * n_ch)()
    for c in range(n_ch):
        pk[c].data = bufs[c].ctypes.data + offs[c]
        pk[c].n_floats = n_elems[c]
        pk[c].sri_xdelta = 0.01
        pk[c].sri_mode = 1
        pk[c].sriChanged = int(k == 0)
        pk[c].present = 1
        pk[c].format = pl.FORMAT_CF16
        out[c].soft = soft[c].ctypes.data
        out[c].bits = bits[c].ctypes.data
        out[c].phase = phase[c].ctypes.data
        out[c].sampleIndex = sidx[c].ctypes.data
        out[c].cap_symbols = cap
    h.process_device(0, pk, out)
    h.synchronize()
    res = []
    for c in range(n_ch):
        n = int(out[c].n_symbols)
        res.append(dict(soft=soft[c, : 2 * n].copy(), phase=phase[c, :n].copy(), bits=bits[c, : int(out[c].n_bits)].copy(),
                        index=sidx[c, : int(out[c].n_sampleIndex)].copy()))
    for a in (soft, phase, sidx, bits):
        pl.host_free(a.reshape(-1))
    return res


@pytest.mark.parametrize("tiled", [0, 1])
def test_zero_copy_half_at_4_byte_alignment_and_long_calls(oracle_mod, monkeypatch, tiled):
    """CF16 packets in psk_soft_host_alloc memory handed to psk_soft_process_device, every one at an address 4 bytes past an
    8-byte boundary, odd element counts, three calls; the last channel's third call has more than 2^20 symbols (samplesPerBaud
    2) and ends in an odd element: the library cuts it on whole samples.  tiled=0: time tiling off, the in-place kernels read
    the packets at that alignment; tiled=1: default options.  A 2-byte aligned CF16 packet is refused, nothing committed."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    if not tiled:
        monkeypatch.setenv("PSK_SOFT_TIME_TILED", "0")
    cfgs = [(8, 4), (10, 8), (7, 2), (16, 4), (2, 4)]
    n_ch, N = len(cfgs), 30000
    n_long = (1 << 20) + 12345
    lens = [N, N, N, N, 2 * n_long + 4000]
    streams = [h16(synth_channel(78000 + c, M, S, lens[c])) for c, (S, M) in enumerate(cfgs)]
    bufs = [pl.host_alloc(2 * lens[c] + 64, np.float16) for c in range(n_ch)]
    h = pl.Handle(n_ch, device=0, max_packet_complex=n_long + 16)
    h.configure(0, [dict(samplesPerBaud=S, constelationSize=M) for S, M in cfgs])
    cuts = [[0, 13001, 20000, N]] * 4 + [[0, 2000, 4000, lens[4]]]
    cap = (n_long + 127) // 64 * 64  # (a multiple of 64: every channel's output rows stay aligned)
    got = [dict(soft=[], bits=[], phase=[], index=[]) for _ in range(n_ch)]
    for k in range(3):
        elems = []
        for c in range(n_ch):
            seg = streams[c][2 * cuts[c][k] : 2 * cuts[c][k + 1]]
            odd = 1 if (c == 4 and k == 2) else (k + c) % 2
            bufs[c][2 : 2 + seg.size] = seg
            bufs[c][2 + seg.size] = 99  # the odd element, ignored
            elems.append(seg.size + odd)
            assert (bufs[c].ctypes.data + 4) % 8 == 4
        if k == 1:  # a 2-byte aligned packet: refused before anything runs
            before = [h.peek(c) for c in range(n_ch)]
            pk = (pl.Packet * 1)()
            out = (pl.Output * 1)()
            pk[0].data, pk[0].n_floats, pk[0].sri_xdelta, pk[0].sri_mode, pk[0].present = bufs[0].ctypes.data + 2, 1000, 0.01, 1, 1
            pk[0].format = pl.FORMAT_CF16
            out[0].cap_symbols = 0
            assert pl.load().psk_soft_process_device(h._h, 0, 1, pk, out, None) == 1
            msg = pl.load().psk_soft_last_error()
            assert b"aligned (CS16: 4)" in msg and b"(CF16: 4)" in msg, msg
            assert [h.peek(c) for c in range(n_ch)] == before
        res = _zero_copy(h, bufs, [4] * n_ch, elems, k, cap)
        st = h.stats()
        assert st["channels_sequential"] == 0, st
        for c in range(n_ch):
            for key in got[c]:
                got[c][key].append(res[c][key])
    assert got[4]["phase"][2].size > (1 << 20)
    h.close()
    for b in bufs:
        pl.host_free(b)
    for c, (S, M) in enumerate(cfgs):
        assert_parity({k: np.concatenate(v) for k, v in got[c].items()},
                      _oracle(oracle_mod, dict(samplesPerBaud=S, constelationSize=M), _cut(streams[c], cuts[c])), "S=%d M=%d" % (S, M))


@pytest.mark.parametrize("variant", ["in_place", "tiled", "pre_pass"])
def test_long_cf16_calls_in_pieces(oracle_mod, monkeypatch, capfd, variant):
    """A CF16 call of more than 2^20 symbols at samplesPerBaud 2 between a short call and a call after it, through
    process_device and process_host; the long packet ends in an odd element (ignored), so a piece boundary computed in
    elements instead of whole samples would show.  in_place: numAvg 100 read in place (time tiling off); tiled: default
    options (widened per piece, time tiled); pre_pass: numAvg 400, widened once per piece."""
    S, M = 2, 4
    A = 100 if variant in ("in_place", "tiled") else 400
    n_sym = (1 << 20) + 12345
    lens = [5000 * S, n_sym * S, 7000 * S]
    iq = h16(_synth(79000, [M], S, [sum(lens)])[0])
    cuts = np.cumsum([0] + lens)
    seq = [[iq[2 * cuts[k] : 2 * cuts[k + 1]]] for k in range(3)]
    seq[1][0] = np.concatenate([seq[1][0], np.float16([5])])
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=50)
    env = dict(PSK_SOFT_TIME_TILED=0) if variant == "in_place" else {}
    lim = dict(max_packet_complex=n_sym * S + 16)
    ref, _ = oracle_calls(oracle_mod, props, [p[0] for p in seq])
    assert ref[1]["phase"].size > (1 << 20)
    for entry in ("device", "host"):
        def body(h, cf):
            h.configure(0, [props])
            g = {0: []}
            tr = []
            for k in range(3):
                gk, tk = device_run(h, [seq[k]], cf, k0=k)[:2] if entry == "device" else host_run(h, [seq[k]], cf, k0=k)
                g[0] += gk[0]
                tr += tk
                st = h.stats()
                assert st["channels_sequential"] == 0 and st["channels_fast"] == 1, (entry, k, st)
            return g, tr
        res = untraced_then_traced(monkeypatch, capfd, env, 1, body, **lim)
        got, traces = res[0][0], res[1][1]
        long = traces[1]
        assert rounds(long) >= 2, (entry, long)
        if variant == "in_place":
            assert screened(long) == {(S, H_CF16): rounds(long)} and "cf16_convert" not in whats(long), (entry, long)
        elif variant == "tiled":
            assert sum(t["what"] == "tile_front" and t["H"] == 1 for t in long) == rounds(long), (entry, long)
            assert sum(t["what"] == "cf16_convert" for t in long) == rounds(long), (entry, long)
        else:
            assert screened(long) == {(S, 4): rounds(long)}, (entry, long)
            assert sum(t["what"] == "cf16_convert" for t in long) == rounds(long), (entry, long)
        for k in range(3):
            assert_parity(got[0][k], ref[k], "%s %s call %d" % (variant, entry, k))


def test_a_channel_that_alternates_the_four_formats(oracle_mod, monkeypatch, capfd):
    """24 channels whose packets rotate through CF32, CS16, CS8 and CF16 call by call (each channel at its own phase), six
    calls, against one continuous oracle run per channel: the carried window holds float samples, channel state has no format.
    The values are int8 ones, exact in all four.  The traced run shows the three in-place classes and the float class side by
    side."""
    from psk_soft_amd.stimulus import synth_channel

    C, calls = 24, 6
    props = [dict(samplesPerBaud=(8, 10, 4, 16)[c % 4], constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 200, 600)[c % 3])
             for c in range(C)]
    N = 48000
    streams = [q8(synth_channel(80000 + c, p["constelationSize"], p["samplesPerBaud"], N)) for c, p in enumerate(props)]
    cuts = [0, 3000, 11111, 20000, 20001, 33000, N]
    conv = (lambda x: x.astype(np.float32), lambda x: x.astype(np.int16), lambda x: x, lambda x: x.astype(np.float16))
    data = [[conv[(c // 3 + k) % 4](_cut(streams[c], cuts)[k]) for c in range(C)] for k in range(calls)]

    def run(h, cf):
        h.configure(0, props)
        return device_run(h, data, cf)

    res = untraced_then_traced(monkeypatch, capfd, dict(PSK_SOFT_TIME_TILED=0), C, run)
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "alternating formats")
    for k, lines in enumerate(res[1][1]):
        if k == 3:  # (a packet of one sample: nothing emits, no wave-scan launch)
            continue
        hs = {t["H"] for t in lines if t["what"].startswith("fast (")}
        assert {1, H_CS16, H_CS8, H_CF16} <= hs, (k, hs)
        assert {"cs16_convert", "cs8_convert", "cf16_convert"} <= whats(lines), (k, whats(lines))  # (numAvg 200, 600)


def test_the_in_place_formats_hand_over_in_one_call(oracle_mod, monkeypatch, capfd):
    """Eight channels, two each of CF32, CS16, CS8 and CF16 (interleaved), PSK_SOFT_TIES_IN_PLACE=0, three calls, time tiling
    off.  The first of each pair is an int8-valued tie stream.  The second of the CF32, CS16 and CF16 pairs is a stream that
    trips the exactness guard in every call -- a few LSB of noise around a burst of +-32767 (CF16: +-32768, exact in half), the
    stream of channel 16 of test_deferred_join_with_a_cs16_class -- so the joined tail's reference-order kernels really redo a
    channel of the float build, of the CS16 build and of the CF16 build in one call, each from its own part of the channel
    list: the CF16 part lies behind the CS16 and the CS8 parts.  An int8 packet cannot trip that guard at numAvg <= 128 (its
    sample energies span 1 .. 2^15, and 24 + 15 + log2(numAvg + 256) stays below 53: the double sums are always exact), so
    the second CS8 channel is a tie stream too and the CS8 build's launch finds nothing handed over.  Every channel bit for bit
    the oracle's, call by call."""
    S, N = 4, 10000
    cuts = [0, 3001, 7000, N]
    ts = _tie_streams(N, S)
    rng = np.random.default_rng(21)

    def guard_stream(full):  # (numpy int16 values; full = the burst's amplitude)
        x = rng.integers(-2, 3, 2 * N).astype(np.int32)
        for a in cuts[:-1]:
            i0 = a + 1000
            x[2 * i0 : 2 * (i0 + 256)] = rng.choice(np.int32([-full, full]), 512)
        return x

    k = rng.integers(0, 4, N // S + 1)
    pulses = (np.repeat(np.stack([(1, 1), (-1, 1), (-1, -1), (1, -1)])[k], S, axis=0)[:N] * 2).reshape(-1)  # (QPSK pulses, no noise)
    streams = [ts[0], ts[1], ts[2], ts[6], guard_stream(32767), guard_stream(32767), pulses, guard_stream(32768)]
    conv = (np.float32, np.int16, np.int8, np.float16)
    C = len(streams)
    assert C == 8 and all(np.abs(streams[c]).max() <= 127 for c in (0, 1, 2, 3, 6))
    streams = [np.asarray(x).astype(conv[c % 4]) for c, x in enumerate(streams)]
    assert all(np.array_equal(x.astype(np.float64), np.asarray(y, np.float64)) for x, y in zip(streams, [ts[0], ts[1], ts[2], ts[6]]))
    guarded = [4, 5, 7]  # (CF32, CS16, CF16)
    props = dict(samplesPerBaud=S, constelationSize=4, numAvg=100, phaseAvg=50)
    data = [[_cut(streams[c], cuts)[k] for c in range(C)] for k in range(3)]

    def run(h, cf):
        h.configure(0, [props] * C)
        got, traces, nsym = {c: [] for c in range(C)}, [], []
        for k in range(3):
            g, t, n = device_run(h, [data[k]], cf, k0=k)
            for c in range(C):
                got[c] += g[c]
            traces += t
            nsym += n
            st = h.stats()
            per = [h.channel_stats(c, 1)[0]["channels_guard"] for c in range(C)]
            assert [c for c in range(C) if per[c]] == guarded, (k, per)
            assert st["channels_sequential"] >= 3 and st["channels_guard"] == 3, (k, st)
        return got, traces, nsym

    res = untraced_then_traced(monkeypatch, capfd, dict(PSK_SOFT_TIES_IN_PLACE=0, PSK_SOFT_TIME_TILED=0), C, run)
    check_parity(oracle_mod, res[0][0], lambda c: props, data, "hand-over of four formats")
    for k, lines in enumerate(res[1][1]):
        hs = {t["H"] for t in lines if t["what"].startswith("fast (")}
        assert {1, H_CS16, H_CS8, H_CF16} <= hs, (k, hs)
        assert "seq (reference order)" in whats(lines), (k, whats(lines))


def test_stamp_key_tells_cf16_from_the_other_formats(oracle_mod):
    """A uniform 256-channel CF16 batch (the stamped path plans it once) in which one channel sends CS16 -- the same bytes per
    sample --, one CF32 and one CS8 of the same values: the odd channels and their neighbours all match.  Then the same with a
    CS16 batch and one CF16 channel."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    C, N, odd16, odd32, odd8 = 256, 12000, 137, 200, 31
    props = dict(samplesPerBaud=8, constelationSize=4, numAvg=100)
    streams = [q8(synth_channel(81000 + c, 4, 8, N)) for c in range(C)]
    pieces = [_cut(x, [0, 4000, 8000, N]) for x in streams]
    calls = []
    for k in range(3):
        base = np.int16 if k == 2 else np.float16
        row = [pieces[c][k].astype(base) for c in range(C)]
        if k == 1:
            row[odd16] = pieces[odd16][k].astype(np.int16)
            row[odd32] = pieces[odd32][k].astype(np.float32)
            row[odd8] = pieces[odd8][k]
        if k == 2:
            row[odd16] = pieces[odd16][k].astype(np.float16)
        calls.append(row)
    h = pl.Handle(C, device=0)
    h.configure_all(**props)
    got, _ = host_run(h, calls)
    h.close()
    for c in (0, odd8, odd16 - 1, odd16, odd16 + 1, odd32, C - 1):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, props, pieces[c]), "ch %d" % c)


def test_deferred_join_with_a_cf16_class(oracle_mod, monkeypatch, capfd):
    """PSK_SOFT_OPT_DEFERRED_JOIN with CF16 packets read in place: 384 channels of four window classes, CF16 at numAvg <= 100,
    six calls issued without a host wait.  The CF16 class (H=6) ends its calls on a side stream; outputs and channel states
    are the ones the same calls give joined, and the oracle's."""
    from psk_soft_amd import lib as pl

    S, C, calls, n = 8, 384, 6, 6000
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    As = [(25, 100, 200, 400)[(c // 3) % 4] for c in range(C)]
    props = [dict(samplesPerBaud=S, constelationSize=Ms[c], numAvg=As[c], phaseAvg=(10, 50, 200)[(c // 12) % 3]) for c in range(C)]
    host = [h16(x) for x in _synth(82000, Ms, S, calls * n)]
    data = [[host[c][2 * k * n : 2 * (k + 1) * n] if (As[c] <= 100 and c % 2 == 0)
             else host[c][2 * k * n : 2 * (k + 1) * n].astype(np.float32) for c in range(C)] for k in range(calls)]
    check = sorted({0, 1, 2, 4, 5, 100, 101, 203, C - 2, C - 1})

    def run(h, cf):
        h.configure(0, props)
        h.set_option(pl.Handle.OPT_DEFERRED_JOIN, 1)
        got, traces, _ = device_run(h, data, cf, check, sync_each=False)
        return got, traces, [h.export_state(c) for c in check]

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    joined = pl.Handle(C, device=0)
    try:
        joined.configure(0, props)
        got_j, _, _ = device_run(joined, data, None, check)
        blobs_j = [joined.export_state(c) for c in check]
    finally:
        joined.close()
    assert_same(res[0][0], got_j, "deferred against joined")
    assert res[0][2] == blobs_j
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "deferred join")
    for k, lines in enumerate(res[1][1]):
        sc = screened(lines)
        assert sc[(S, H_CF16)] == 1 and lines[0]["H"] != H_CF16, (k, sc)
        assert not whats(lines) & {"cf16_convert", "seq (reference order)"}, (k, whats(lines))
        side = {t["stream"] for t in lines if t["H"] == H_CF16}
        assert len(side) == 1 and side.isdisjoint({t["stream"] for t in lines if t["H"] != H_CF16}), (k, lines)


@pytest.mark.parametrize("S,M,diff,n_ph", [(8, 4, 1, 50), (4, 2, 0, 200)])
def test_pipelined_ranges_with_cf16(oracle_mod, monkeypatch, capfd, S, M, diff, n_ph):
    """PSK_SOFT_PIPELINED=2: channels of ragged lengths whose packets alternate CF16 / CF32 from call to call (the CF16 ones
    widened by the pre-pass, whose scratch the pipeline streams read), three calls."""
    from psk_soft_amd.stimulus import synth_channel

    C, calls = 7, 3
    lens = [40000, 40000, 1000 * S, 23456, 40000, 17 * 128 * S + 5 * S, 40000]
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=n_ph, differentialDecoding=diff)
    iqs = [h16(synth_channel(83000 + 7 * S + c, M, S, calls * lens[c], sigma=(0.35 if c == 4 else 0.01))) for c in range(C)]
    data = [[iqs[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]] if (c + k) % 2 == 0
             else iqs[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]].astype(np.float32) for c in range(C)] for k in range(calls)]

    def run(h, cf):
        h.configure(0, [props] * C)
        return device_run(h, data, cf)

    res = untraced_then_traced(monkeypatch, capfd, dict(PSK_SOFT_PIPELINED=2, PSK_SOFT_TIME_TILED=2), C, run)
    for k, lines in enumerate(res[1][1]):
        w = whats(lines)
        assert "cf16_convert" in w, (k, w)
        assert sum(t["what"] == "pipe_front" and t["H"] == 1 for t in lines) >= 2, (k, lines)
        assert not any(t["H"] == H_CF16 for t in lines), (k, lines)
    check_parity(oracle_mod, res[0][0], lambda c: props, data, "pipelined S%d" % S)


@pytest.mark.parametrize("pieces", [2, 3, 5])
def test_a_mixed_batch_of_the_four_formats_cut_in_time(oracle_mod, monkeypatch, capfd, pieces):
    """The mixed batch of the sc16 schedule tests (four window classes; its numAvg <= 128 "kind 1" channels sent int16 there)
    with those channels in turn as CF16, CS16 and CS8 -- so five classes, three of them read in place -- cut into
    PSK_SOFT_SPLIT_CLASSES pieces: each piece of a half packet starts whole samples further on.  Channel 9 (CF16) keeps its odd
    last element."""
    S, calls, C = 4, 2, 28
    env = dict(PSK_SOFT_SPLIT_CLASSES=pieces, PSK_SOFT_TIME_TILED=0)
    props, data16, kind = _mixed_cut_batch(C, S, calls, prepass=False)
    as_fmt = {}
    for c in range(C):
        if kind[c] == 1:
            as_fmt[c] = (np.float16, np.int16, np.int8)[(c // 4 + 1) % 3]
    assert as_fmt[9] == np.float16 and {np.float16, np.int16, np.int8} == set(as_fmt.values())
    # (int16 values scaled down into int8 range, exact in all three formats)
    data = [[(np.clip(x.astype(np.int32) >> 8, -128, 127).astype(as_fmt[c]) if c in as_fmt else x) for c, x in enumerate(row)] for row in data16]
    check = sorted({0, 1, 2, 3, 5, 6, 9, 10, 13, 17, 21, C - 2, C - 1})
    res = untraced_then_traced(monkeypatch, capfd, env, C, lambda h, cf: (h.configure(0, props), device_run(h, data, cf, check))[1])
    got, _, nsym = res[0]
    _, traces, _ = res[1]
    check_parity(oracle_mod, got, lambda c: props[c], data, "four formats cut in %d" % pieces)
    assert any(n % 2 for row in nsym for n in row), "no call emitted an odd number of symbols"
    h_of = {np.float16: H_CF16, np.int16: H_CS16, np.int8: H_CS8}
    classes = {(S, {0: 1, 2: 2, 3: 4}[kind[c]] if kind[c] != 1 else h_of[as_fmt[c]]) for c in range(C)}
    assert len(classes) == 6
    for k, lines in enumerate(traces):
        assert rounds(lines) == pieces, (k, lines)
        assert screened(lines) == {cl: pieces for cl in classes}, (k, screened(lines))
        assert not whats(lines) & {"cf16_convert", "cs16_convert", "cs8_convert", "tile_front"}, (k, whats(lines))


def test_strided_entry_with_a_frame_major_half_matrix(oracle_mod, monkeypatch, capfd):
    """A frame-major matrix of halves 128 samples wide: columns 5 .. 64 as one frame group (the tile kernel, 4-byte columns),
    columns 70, 73, 76 as singles, next to two contiguous CF16 packets; ragged lengths, three calls carrying state.  The rows
    land as halves and still reach the in-place kernels; everything equals the contiguous call and the oracle."""
    S, G, calls = 8, 60, 3
    place = [(0, 5 + c) for c in range(G)] + [(0, 70), (0, 73), (0, 76), None, None]
    C = len(place)
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 64, 25)[c % 3], phaseAvg=(50, 10, 200)[(c // 3) % 3],
                  differentialDecoding=int(c % 7 == 3)) for c in range(C)]
    lens = [[9000 + 131 * ((7 * c + 3 * k) % 61) + (c % 2) for c in range(C)] for k in range(calls)]
    Ms = [p["constelationSize"] for p in props]
    streams = [h16(x) for x in _synth(84000, Ms, S, [sum(lens[k][c] for k in range(calls)) for c in range(C)])]
    data = [[streams[c][2 * sum(lens[j][c] for j in range(k)) : 2 * sum(lens[j][c] for j in range(k + 1))] for c in range(C)]
            for k in range(calls)]

    def run(h, cf):
        h.configure(0, props)
        got, traces, nsym = strided_run(h, data, place, {0: 128}, cf, odd=(0, 7, G + 1))
        st = h.stats()
        assert st["channels_sequential"] == 0 and st["channels_fast"] == C, st
        return got, traces, nsym

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (1, 1, 1, 3), (k, lines)
        assert all(t["S"] == 4 for t in lines if t["what"].startswith("gather_")), (k, lines)  # (bytes per sample)
        assert (S, H_CF16) in screened(lines), (k, screened(lines))
        assert not whats(lines) & {"cf16_convert", "cs16_convert", "cs8_convert"}, (k, whats(lines))
    assert_same(res[0][0], contiguous(C, props, data), "strided against contiguous")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "frame-major half matrix")


def test_quality_records_equal_the_float_runs(oracle_mod, monkeypatch, capfd):
    """CF32, CS16, CS8 and CF16 packets of the same int8-valued stimulus, and a CF16 / CF32 pair of a half-rounded one at
    numAvg 300 (the pre-pass): identical records, byte for byte, call by call."""
    S, M = 8, 4
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)] * 4 + [dict(samplesPerBaud=S, constelationSize=M, numAvg=300)] * 2
    lens = [8000, 8003]
    x8 = q8(_synth(85000, [M], S, sum(lens))[0])
    xh = h16(_synth(85001, [M], S, sum(lens))[0])
    calls = [[x8[2 * a:2 * b].astype(np.float32), x8[2 * a:2 * b].astype(np.int16), x8[2 * a:2 * b], x8[2 * a:2 * b].astype(np.float16),
              xh[2 * a:2 * b], xh[2 * a:2 * b].astype(np.float32)] for a, b in ((0, lens[0]), (lens[0], sum(lens)))]
    C = len(props)
    runs = t_quality.three_runs(monkeypatch, capfd, {}, C,
                                lambda h, cf, q: (h.configure(0, props), t_quality.device_calls(h, calls, None, cf, q))[1])
    t_quality.check_case(oracle_mod, runs, lambda c: props[c], calls, C, "formats")
    for k in range(2):
        r = runs[1].recs[k]
        assert r[0] == r[1] == r[2] == r[3] != bytes(88), k
        assert r[4] == r[5] != bytes(88), k
