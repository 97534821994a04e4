"""Complex int8 packets (PSK_SOFT_FORMAT_CS8) on a real MI355X: every stream bit for bit what the oracle gives on the float32
cast of the same int8 values (the cast is exact), through every entry point, kernel family and schedule -- the host-buffer
path, device-resident packets from torch int8 tensors, zero-copy from page-locked memory at 2-byte alignment, calls the
library cuts, the deferred join, pipelined ranges, the host class with a char input port.  Small int8 amplitudes make exact
energy ties the normal case, so the exact tier is checked on purpose."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_cs16 import _cut, _tie_streams, _window_class_cfgs
from tests.test_gpu_cs16_schedules import (KEYS, assert_same, check_parity, host_run, oracle_calls, parse_trace, screened,
                                           untraced_then_traced, whats, _synth)
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

SCALE8 = 40.0
H_CS8 = 5  # the window class of CS8 packets read in place (psk_ctl.h: kPktFormats)


def q8(x, scale=SCALE8):
    """float I/Q -> int8 I/Q: round(x * scale), clipped"""
    return np.clip(np.rint(np.asarray(x, np.float64) * scale), -128, 127).astype(np.int8)


def _fmt(x):
    from psk_soft_amd import lib as pl

    return {np.dtype(np.int8): pl.FORMAT_CS8, np.dtype(np.int16): pl.FORMAT_CS16}.get(x.dtype, pl.FORMAT_CF32)


def device_run(h, calls, capfd=None, check=None, sync_each=True, before=None, k0=0):
    """tests.test_gpu_cs16_schedules.device_run with the format taken from each packet's dtype: int8 CS8, int16 CS16, float32
    CF32.  Returns ({c: [per-call dicts]}, [launch lines of call k], [n_symbols[k][c]])."""
    from psk_soft_amd import lib as pl

    K, C = len(calls), len(calls[0])
    check = list(range(C)) if check is None else list(check)
    al = lambda n: (n + 127) // 128 * 128  # noqa: E731
    lay, tot = {}, [0, 0, 0, 0, 0]
    for k in range(K):
        for c in range(C):
            x = calls[k][c]
            if x is None:
                continue
            cap = h.output_capacity(c, x.size // 2)
            sizes = (x.nbytes, 8 * cap, 4 * cap, 6 * cap, 2 * cap)
            lay[k, c] = (cap, tuple(tot))
            for i, s in enumerate(sizes):
                tot[i] += al(s)
    bufs = [h.device_alloc(max(t, 128)) for t in tot]
    d_in, d_soft, d_phase, d_bits, d_sidx = bufs
    traces, nsym, outs = [], [], []
    try:
        for (k, c), (cap, o) in lay.items():
            h.upload(d_in + o[0], calls[k][c])
        h.synchronize()
        for k in range(K):
            if before:
                before(h, k)
            pk, out = (pl.Packet * C)(), (pl.Output * C)()
            for c in range(C):
                x = calls[k][c]
                if x is None:
                    continue
                cap, o = lay[k, c]
                pk[c].data, pk[c].n_floats, pk[c].sri_xdelta, pk[c].sri_mode = d_in + o[0], x.size, 0.01, 1
                pk[c].sriChanged, pk[c].present, pk[c].format = int(k + k0 == 0), 1, _fmt(x)
                out[c].soft, out[c].phase, out[c].bits, out[c].sampleIndex = d_soft + o[1], d_phase + o[2], d_bits + o[3], d_sidx + o[4]
                out[c].cap_symbols = cap
            if capfd:
                capfd.readouterr()
            h.process_device(0, pk, out)
            if capfd:
                traces.append(parse_trace(capfd.readouterr().err))
            if sync_each:
                h.synchronize()
            outs.append(out)
            nsym.append([int(out[c].n_symbols) for c in range(C)])
        if not sync_each:
            h.join()
        h.synchronize()
        got = {c: [] for c in check}
        for c in check:
            for k in range(K):
                if calls[k][c] is None:
                    got[c].append(None)
                    continue
                o, (cap, off) = outs[k][c], lay[k, c]
                ns = int(o.n_symbols)
                assert int(o.n_sampleIndex) in (0, ns), (k, c, int(o.n_sampleIndex), ns)
                got[c].append(dict(soft=h.download(d_soft + off[1], (2 * ns,), np.float32),
                                   phase=h.download(d_phase + off[2], (ns,), np.float32),
                                   bits=h.download(d_bits + off[3], (int(o.n_bits),), np.int16),
                                   # (n_sampleIndex is n_symbols, or 0 at samplesPerBaud 1: that row is not written)
                                   index=h.download(d_sidx + off[4], (int(o.n_sampleIndex),), np.int16)))
    finally:
        for b in bufs:
            h.device_free(b)
    return got, traces, nsym


def _joined(got):
    return {k: np.concatenate([g[k] for g in got]) for k in KEYS}


def _oracle(oracle_mod, props, pieces):
    return _joined(oracle_calls(oracle_mod, props, pieces)[0])


@pytest.mark.parametrize("name", ["testDiffDecode8PSK", "testDiffDecodeBPSK", "testDiffDecodeQPSK",
                                  "testNonDiffDecode8PSK", "testNonDiffDecodeBPSK", "testNonDiffDecodeQPSK"])
def test_reference_component_scenarios_quantised(oracle_mod, name):
    from psk_soft_amd import lib as pl
    from tests.test_oracle_reference_kat import reference_stimuli

    M, diff, data, _ = reference_stimuli()[name]
    iq = q8(data)
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
    """(a fresh process, torch initialised before the library) 4096 channels x 2^16 samples from torch int8 device tensors
    through psk_soft_process_device, two calls, as CS8, as CS16 and as CF32 of the same values, then CS8 again on a handle
    with the launch trace on; saves the stimulus and outputs of a few channels, the stats and the comparisons to `path`"""
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    C, N, S, M = 4096, 1 << 16, 8, 4
    dev = torch.device("cuda", 0)
    iq8 = torch.clamp(torch.round(synth_channels_torch(C, M, S, 2 * N, dev) * SCALE8), -128, 127).to(torch.int8).contiguous()
    forms = {pl.FORMAT_CS8: iq8, pl.FORMAT_CS16: iq8.to(torch.int16).contiguous(), pl.FORMAT_CF32: iq8.to(torch.float32).contiguous()}
    cap = (N // S + 2 + 63) // 64 * 64
    check = [0, 1, 777, 2048, C - 1]
    save = {"check": np.array(check), "iq": iq8[check].cpu().numpy()}

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
                sys.stderr.write("[cs8-test] call %d\n" % k)
                sys.stderr.flush()
            h.process_device(0, pk, out)
            h.synchronize()
            stats.append(h.stats())
            ns.append([int(out[c].n_symbols) for c in range(C)])
        h.close()
        return out_t, stats, ns

    res = {fmt: run(fmt, False) for fmt in (pl.FORMAT_CS8, pl.FORMAT_CS16, pl.FORMAT_CF32)}
    res["trace"] = run(pl.FORMAT_CS8, True)
    base, st8, ns8 = res[pl.FORMAT_CS8]
    same = {}
    for key, (outs, st, ns) in res.items():
        same[str(key)] = bool(ns == ns8 and all(torch.equal(a.view(torch.int16 if a.dtype == torch.int16 else torch.int32),
                                                            b.view(torch.int16 if b.dtype == torch.int16 else torch.int32))
                                                for a, b in zip(outs, base)))
    save["same"] = np.array([same[str(f)] for f in (pl.FORMAT_CS16, pl.FORMAT_CF32)] + [same["trace"]])
    save["seq"] = np.array([s["channels_sequential"] for s in st8])
    save["fast"] = np.array([s["channels_fast"] for s in st8])
    for c in check:
        for k in range(2):
            n = ns8[k][c]
            save["soft_%d_%d" % (c, k)] = base[0][k, c, : 2 * n].cpu().numpy()
            save["phase_%d_%d" % (c, k)] = base[1][k, c, :n].cpu().numpy()
            save["index_%d_%d" % (c, k)] = base[2][k, c, :n].cpu().numpy()
            save["bits_%d_%d" % (c, k)] = base[3][k, c, : 2 * n].cpu().numpy()
    np.savez(path, **save)


def test_device_batch_from_torch_int8_tensors(oracle_mod, tmp_path):
    """4096 channels x 2^16 samples, QPSK, S = 8, numAvg 100: CS8, CS16 and CF32 of the same values give identical bits, no
    channel leaves the wave-scan kernels, and the launch trace shows the CS8 in-place class (H=5) in both tiers and no
    pre-pass.  (In a child process of its own: torch initialises its HIP runtime first there.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "batch.npz")
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_cs8 as t; t._torch_batch_child(%r)" % path], cwd=root,
                       capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = np.load(path)
    assert d["same"].tolist() == [True, True, True]
    assert d["seq"].tolist() == [0, 0] and d["fast"].tolist() == [4096, 4096]
    err = r.stderr.decode()
    calls = err.split("[cs8-test] call ")[1:]
    assert len(calls) == 2
    for text in calls:
        lines = parse_trace(text)
        w = whats(lines)
        assert "cs8_convert" not in w and "cs16_convert" not in w and "tile_front" not in w, w
        assert screened(lines) == {(8, H_CS8): 1}, lines
        assert all(t["H"] == H_CS8 for t in lines if t["what"].startswith("fast (")), lines
    props = dict(samplesPerBaud=8, constelationSize=4, numAvg=100, phaseAvg=50)
    N = 1 << 16
    for i, c in enumerate(d["check"].tolist()):
        got = {key: np.concatenate([d["%s_%d_%d" % (key, c, k)] for k in range(2)]) for key in KEYS}
        assert_parity(got, _oracle(oracle_mod, props, [d["iq"][i, : 2 * N], d["iq"][i, 2 * N :]]), "channel %d" % c)


def test_every_window_class_in_one_mixed_cs8_batch(oracle_mod):
    """samplesPerBaud 2 .. 32, 33 and 100, numAvg 1 .. 1025, phaseAvg 50 / 4000: one batch, three calls with ragged cuts and
    odd element counts -- every class but the in-place one through the conversion pre-pass."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    cfgs = _window_class_cfgs()
    rng = np.random.default_rng(13)
    pieces = []
    for c, p in enumerate(cfgs):
        S, A = p["samplesPerBaud"], p["numAvg"]
        n = S * (A + 300) + int(rng.integers(0, 4000))
        iq = q8(synth_channel(61000 + c, p["constelationSize"], S, n))
        a, b = sorted(rng.choice(np.arange(1, n), 2, replace=False))
        segs = _cut(iq, [0, a, b, n])
        segs[0] = np.concatenate([segs[0], np.int8([12])])  # an odd element: ignored
        segs[2] = np.concatenate([segs[2], np.int8([-5])])
        pieces.append(segs)
    h = pl.Handle(len(cfgs), device=0, max_window_samples=65536 + 64, max_phase_avg=4096)
    h.configure(0, cfgs)
    got, _ = host_run(h, [[pieces[c][k] for c in range(len(cfgs))] for k in range(3)])
    assert h.stats()["channels_sequential"] == 0
    h.close()
    for c, p in enumerate(cfgs):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, p, pieces[c]), "cfg %s" % p)


@pytest.mark.parametrize("ties_in_place", [1, 0])
@pytest.mark.parametrize("numAvg", [100, 400])
def test_exact_energy_ties_of_int8_samples(oracle_mod, monkeypatch, ties_in_place, numAvg):
    """Rectangular pulses of +-1 ... 3 LSB, constant and full-scale square streams: the window sums of integer squares are
    exact and tie all the time.  The exact tier runs, and decides them as the reference does."""
    from psk_soft_amd import lib as pl

    monkeypatch.setenv("PSK_SOFT_TIES_IN_PLACE", str(ties_in_place))
    S, N = 8, 20000
    streams = [np.clip(x, -128, 127).astype(np.int8) for x in _tie_streams(N, S)]
    rng = np.random.default_rng(7)
    for lsb in (1, 2, 3):  # rectangular QPSK pulses of `lsb`, no noise
        k = rng.integers(0, 4, N // S + 1)
        streams.append((np.repeat(np.stack([(1, 1), (-1, 1), (-1, -1), (1, -1)])[k], S, axis=0)[:N] * lsb).reshape(-1).astype(np.int8))
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


@pytest.mark.parametrize("n_ch", [1, 64])
def test_time_tiled_and_parallel_fit(oracle_mod, n_ch):
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    N, S, M = 1 << 18, 8, 4
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)
    streams = [q8(synth_channel(62000 + c, M, S, N)) for c in range(n_ch)]
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
    streams = [q8(synth_channel(63000 + c, p["constelationSize"], S, N)) for c, p in enumerate(props)]
    pieces = [_cut(x, [0, S * 100 + 77, S * 400, N]) for x in streams]
    h = pl.Handle(2, device=0, max_window_samples=S * A + 64, max_packet_complex=N)
    h.configure(0, props)
    got, _ = host_run(h, [[pieces[c][k] for c in range(2)] for k in range(3)])
    h.close()
    for c in range(2):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, props[c], pieces[c]), "wide ch %d" % c)


def test_reference_order_kernel(oracle_mod):
    """A forced-sequential handle: every CS8 channel through the reference-order kernel (the pre-pass in front of it)."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    cfgs = [(8, 4, 0), (10, 8, 1), (5, 2, 0), (1, 4, 0)]
    streams = [q8(synth_channel(64000 + c, M, S, 6000)) for c, (S, M, d) in enumerate(cfgs)]
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
    """psk_soft_process_device on packets in page-locked memory: channel c's packet at bufs[c] + offs[c] bytes, n_elems[c]
    int8 elements; outputs in page-locked memory too"""
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
        pk[c].format = pl.FORMAT_CS8
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
def test_zero_copy_int8_at_2_byte_alignment(oracle_mod, monkeypatch, tiled):
    """CS8 packets in psk_soft_host_alloc memory handed to psk_soft_process_device, every one at an address 2 bytes past a
    4-byte boundary, odd element counts, two calls; then a call of more than 2^20 symbols (samplesPerBaud 2) that the library
    cuts on whole samples.  tiled=0: time tiling off, the in-place kernels read the packets at that alignment; tiled=1:
    default options.  An odd-address CS8 packet is refused, nothing committed."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    if not tiled:
        monkeypatch.setenv("PSK_SOFT_TIME_TILED", "0")
    cfgs = [(8, 4), (10, 8), (7, 2), (16, 4), (2, 4)]
    n_ch, N = len(cfgs), 30000
    n_long = (1 << 20) + 12345
    lens = [N, N, N, N, 2 * n_long + 4000]
    streams = [q8(synth_channel(65000 + c, M, S, lens[c])) for c, (S, M) in enumerate(cfgs)]
    bufs = [pl.host_alloc(2 * lens[c] + 64, np.int8) for c in range(n_ch)]
    h = pl.Handle(n_ch, device=0, max_packet_complex=n_long + 16)
    h.configure(0, [dict(samplesPerBaud=S, constelationSize=M) for S, M in cfgs])
    cuts = [[0, 13001, 20000, N]] * 4 + [[0, 2000, 4000, lens[4]]]
    cap = (n_long + 127) // 64 * 64  # (a multiple of 64: every channel's output rows stay aligned)
    got = [dict(soft=[], bits=[], phase=[], index=[]) for _ in range(n_ch)]
    for k in range(3):
        elems = []
        for c in range(n_ch):
            seg = streams[c][2 * cuts[c][k] : 2 * cuts[c][k + 1]]
            odd = (k + c) % 2
            bufs[c][2 : 2 + seg.size] = seg
            bufs[c][2 + seg.size] = 99  # the odd element, ignored
            elems.append(seg.size + odd)
            assert (bufs[c].ctypes.data + 2) % 4 == 2
        if k == 1:  # an odd-address packet: refused before anything runs
            before = [h.peek(c) for c in range(n_ch)]
            pk = (pl.Packet * 1)()
            out = (pl.Output * 1)()
            pk[0].data, pk[0].n_floats, pk[0].sri_xdelta, pk[0].sri_mode, pk[0].present = bufs[0].ctypes.data + 3, 1000, 0.01, 1, 1
            pk[0].format = pl.FORMAT_CS8
            out[0].cap_symbols = 0
            assert pl.load().psk_soft_process_device(h._h, 0, 1, pk, out, None) == 1
            msg = pl.load().psk_soft_last_error()
            assert b"aligned (CS16: 4)" in msg and b"(CS8: 2)" in msg, msg
            assert [h.peek(c) for c in range(n_ch)] == before
        res = _zero_copy(h, bufs, [2] * n_ch, elems, k, cap)
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


def test_a_channel_that_alternates_cf32_cs16_cs8(oracle_mod, monkeypatch, capfd):
    """24 channels whose packets rotate through CF32, CS16 and CS8 call by call (each channel at its own phase), five calls,
    against one continuous oracle run per channel: the carried window holds float samples, channel state has no format.
    The traced run shows both in-place classes and the float class side by side."""
    C, calls = 24, 5
    props = [dict(samplesPerBaud=(8, 10, 4, 16)[c % 4], constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 200, 600)[c % 3])
             for c in range(C)]
    N = 40000
    from psk_soft_amd.stimulus import synth_channel

    streams = [q8(synth_channel(66000 + c, p["constelationSize"], p["samplesPerBaud"], N)) for c, p in enumerate(props)]
    cuts = [0, 3000, 11111, 20000, 20001, N]
    conv = (lambda x: x.astype(np.float32), lambda x: x.astype(np.int16), lambda x: x)
    data = [[conv[(c // 3 + k) % 3](_cut(streams[c], cuts)[k]) for c in range(C)] for k in range(calls)]

    def run(h, cf):
        h.configure(0, props)
        return device_run(h, data, cf)

    res = untraced_then_traced(monkeypatch, capfd, dict(PSK_SOFT_TIME_TILED=0), C, run)
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "alternating formats")
    for k, lines in enumerate(res[1][1]):
        if k == 3:  # (a packet of one sample: nothing emits, no wave-scan launch)
            continue
        hs = {t["H"] for t in lines if t["what"].startswith("fast (")}
        assert {1, 3, H_CS8} <= hs, (k, hs)


def test_stamp_key_tells_cs8_from_cs16_and_cf32(oracle_mod):
    """A uniform 256-channel CS8 batch (the stamped path plans it once) in which one channel sends CS16 and another CF32 of the
    same values: the odd channels and their neighbours all match."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    C, N, odd16, odd32 = 256, 12000, 137, 200
    props = dict(samplesPerBaud=8, constelationSize=4, numAvg=100)
    streams = [q8(synth_channel(67000 + c, 4, 8, N)) for c in range(C)]
    pieces = [_cut(x, [0, 6000, N]) for x in streams]
    calls = []
    for k in range(2):
        row = [pieces[c][k] for c in range(C)]
        if k == 1:
            row[odd16] = row[odd16].astype(np.int16)
            row[odd32] = row[odd32].astype(np.float32)
        calls.append(row)
    h = pl.Handle(C, device=0)
    h.configure_all(**props)
    got, _ = host_run(h, calls)
    h.close()
    for c in (0, odd16 - 1, odd16, odd16 + 1, odd32, C - 1):
        assert_parity(_joined(got[c]), _oracle(oracle_mod, props, pieces[c]), "ch %d" % c)


def test_deferred_join_with_a_cs8_class(oracle_mod, monkeypatch, capfd):
    """PSK_SOFT_OPT_DEFERRED_JOIN with CS8 packets read in place: 384 channels of four window classes, CS8 at numAvg <= 100,
    six calls issued without a host wait.  The CS8 class (H=5) ends its calls on a side stream; outputs and channel states
    are the ones the same calls give joined, and the oracle's."""
    from psk_soft_amd import lib as pl

    S, C, calls, n = 8, 384, 6, 6000
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    As = [(25, 100, 200, 400)[(c // 3) % 4] for c in range(C)]
    props = [dict(samplesPerBaud=S, constelationSize=Ms[c], numAvg=As[c], phaseAvg=(10, 50, 200)[(c // 12) % 3]) for c in range(C)]
    host = [q8(x) for x in _synth(68000, Ms, S, calls * n)]
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
        assert sc[(S, H_CS8)] == 1 and lines[0]["H"] != H_CS8, (k, sc)
        assert not whats(lines) & {"cs8_convert", "seq (reference order)"}, (k, whats(lines))


@pytest.mark.parametrize("S,M,diff,n_ph", [(8, 4, 1, 50), (4, 2, 0, 200)])
def test_pipelined_ranges_with_cs8(oracle_mod, monkeypatch, capfd, S, M, diff, n_ph):
    """PSK_SOFT_PIPELINED=2: channels of ragged lengths whose packets alternate CS8 / CF32 from call to call (the CS8 ones
    converted by the pre-pass, whose scratch the pipeline streams read), three calls."""
    from psk_soft_amd.stimulus import synth_channel

    C, calls = 7, 3
    lens = [40000, 40000, 1000 * S, 23456, 40000, 17 * 128 * S + 5 * S, 40000]
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=n_ph, differentialDecoding=diff)
    iqs = [q8(synth_channel(69000 + 7 * S + c, M, S, calls * lens[c], sigma=(0.35 if c == 4 else 0.01))) for c in range(C)]
    data = [[iqs[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]] if (c + k) % 2 == 0
             else iqs[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]].astype(np.float32) for c in range(C)] for k in range(calls)]

    def run(h, cf):
        h.configure(0, [props] * C)
        return device_run(h, data, cf)

    res = untraced_then_traced(monkeypatch, capfd, dict(PSK_SOFT_PIPELINED=2, PSK_SOFT_TIME_TILED=2), C, run)
    for k, lines in enumerate(res[1][1]):
        w = whats(lines)
        assert "cs8_convert" in w, (k, w)
        assert sum(t["what"] == "pipe_front" and t["H"] == 1 for t in lines) >= 2, (k, lines)
        assert not any(t["H"] == H_CS8 for t in lines), (k, lines)
    check_parity(oracle_mod, res[0][0], lambda c: props, data, "pipelined S%d" % S)


def test_host_class_with_a_char_input_port(oracle_mod):
    from psk_soft_amd import sandbox
    from psk_soft_amd.stimulus import synth_channel

    comp = sandbox.Component(device=0, input="char")
    comp.samplesPerBaud = 8
    comp.constelationSize = 8
    comp.numAvg = 100
    iq = q8(synth_channel(70000, 8, 8, 20000))
    pieces = _cut(iq, [0, 9000, 20000])
    for k, seg in enumerate(pieces):
        comp.push(seg, sampleRate=100, sriChanged=(k == 0))
        assert comp.service() == 1
    got = dict(soft=comp.getData("softDecision_dataFloat_out"), bits=comp.getData("bits_dataShort_out"),
               phase=comp.getData("phase_dataFloat_out"), index=comp.getData("sampleIndex_dataShort_out"))
    comp.close()
    assert_parity(got, _oracle(oracle_mod, dict(samplesPerBaud=8, constelationSize=8, numAvg=100), pieces), "host class")
