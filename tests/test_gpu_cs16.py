"""Complex int16 packets (PSK_SOFT_FORMAT_CS16) on a real MI355X: every stream bit for bit what the oracle gives on the
float32 cast of the same int16 values (the cast is exact), through every entry point and kernel family -- device-resident
packets, zero-copy from page-locked memory, the host-buffer path, the host class with a short input port."""

import numpy as np
import pytest

from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

SCALE = 8192.0


def q16(x, scale=SCALE):
    """float I/Q -> int16 I/Q: round(x * scale), clipped"""
    return np.clip(np.rint(np.asarray(x, np.float64) * scale), -32768, 32767).astype(np.int16)


def _oracle_calls(oracle_mod, props, pieces, xdelta=0.01):
    """the oracle on the float cast of each piece (one call each)"""
    o = oracle_mod.OracleComponent()
    for k, v in props.items():
        setattr(o, k, v)
    ref = dict(soft=[], bits=[], phase=[], index=[])
    for k, seg in enumerate(pieces):
        r = o.service(np.asarray(seg).astype(np.float32), xdelta, sriChanged=(k == 0))
        ref["soft"].append(r.soft); ref["bits"].append(r.bits); ref["phase"].append(r.phase); ref["index"].append(r.index)
    return {k: np.concatenate(v) for k, v in ref.items()}


def _host_calls(h, pieces_per_channel, fmt_of=lambda c, k: 1, xdelta=0.01):
    """process_host, one call per piece index; fmt_of(c, k) = 1: the piece goes as int16, 0: as its float32 cast"""
    n_ch = len(pieces_per_channel)
    got = [dict(soft=[], bits=[], phase=[], index=[]) for _ in range(n_ch)]
    for k in range(len(pieces_per_channel[0])):
        pk = []
        for c in range(n_ch):
            seg = pieces_per_channel[c][k]
            pk.append(dict(data=seg if fmt_of(c, k) else seg.astype(np.float32), xdelta=xdelta, sriChanged=(k == 0)))
        res = h.process_host(0, pk)
        for c in range(n_ch):
            for key in got[c]:
                got[c][key].append(res[c][key])
    return [{k: np.concatenate(v) for k, v in g.items()} for g in got]


def _cut(x, cuts):
    return [x[2 * a : 2 * b] for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("name", ["testDiffDecode8PSK", "testDiffDecodeBPSK", "testDiffDecodeQPSK",
                                  "testNonDiffDecode8PSK", "testNonDiffDecodeBPSK", "testNonDiffDecodeQPSK"])
def test_reference_component_scenarios_quantised(oracle_mod, name):
    from psk_soft_amd import lib as pl
    from tests.test_oracle_reference_kat import reference_stimuli

    M, diff, data, _ = reference_stimuli()[name]
    iq = q16(data)
    props = dict(samplesPerBaud=8, constelationSize=M, numAvg=100, differentialDecoding=int(diff))
    h = pl.Handle(1, device=0)
    h.configure(0, [props])
    n = iq.size // 2
    cuts = [0, n // 3, n // 3 + 1001, n]
    got = _host_calls(h, [_cut(iq, cuts)])[0]
    assert_parity(got, _oracle_calls(oracle_mod, props, _cut(iq, cuts), 0.01), name)
    assert h.stats()["channels_fast"] == 1
    h.close()


def _torch_batch_child(path):
    """(runs in a fresh process, torch initialised before the library) 2048 channels x 2^16 samples from torch int16 device
    tensors through psk_soft_process_device, two calls; saves the stimulus and the outputs of a few channels to `path`"""
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    C, N, S, M = 2048, 1 << 16, 8, 4
    dev = torch.device("cuda", 0)
    iq = torch.clamp(torch.round(synth_channels_torch(C, M, S, 2 * N, dev) * SCALE), -32768, 32767).to(torch.int16).contiguous()
    cap = (N // S + 2 + 63) // 64 * 64
    soft = torch.empty((C, 2 * cap), dtype=torch.float32, device=dev)
    phase = torch.empty((C, cap), dtype=torch.float32, device=dev)
    sidx = torch.empty((C, cap), dtype=torch.int16, device=dev)
    bits = torch.empty((C, 2 * cap), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    h = pl.Handle(C, device=0)
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)
    check = [0, 1, 777, 1500, C - 1]
    save = {"check": np.array(check), "iq": iq[check].cpu().numpy()}
    for k in range(2):
        pk = (pl.Packet * C)()
        out = (pl.Output * C)()
        for c in range(C):
            pk[c].data = iq[c].data_ptr() + k * 2 * N * 2
            pk[c].n_floats = 2 * N
            pk[c].sri_xdelta = 0.01
            pk[c].sri_mode = 1
            pk[c].sriChanged = int(k == 0)
            pk[c].present = 1
            pk[c].format = pl.FORMAT_CS16
            out[c].soft = soft[c].data_ptr()
            out[c].bits = bits[c].data_ptr()
            out[c].phase = phase[c].data_ptr()
            out[c].sampleIndex = sidx[c].data_ptr()
            out[c].cap_symbols = cap
        h.process_device(0, pk, out)
        h.synchronize()
        st = h.stats()
        assert st["channels_fast"] == C and st["channels_sequential"] == 0, st
        for c in check:
            ns = int(out[c].n_symbols)
            save["soft_%d_%d" % (c, k)] = soft[c, : 2 * ns].cpu().numpy()
            save["phase_%d_%d" % (c, k)] = phase[c, :ns].cpu().numpy()
            save["index_%d_%d" % (c, k)] = sidx[c, :ns].cpu().numpy()
            save["bits_%d_%d" % (c, k)] = bits[c, : 2 * ns].cpu().numpy()
    h.close()
    np.savez(path, **save)


def test_machine_filling_batch_from_torch_int16_tensors(oracle_mod, tmp_path):
    """2048 channels x 2^16 samples, QPSK, S = 8, from torch int16 device tensors through psk_soft_process_device, two calls
    (cold start, then carried state).  (In a child process of its own: torch initialises its HIP runtime first there.)"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "batch.npz")
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_cs16 as t; t._torch_batch_child(%r)" % path], cwd=root,
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = np.load(path)
    props = dict(samplesPerBaud=8, constelationSize=4, numAvg=100, phaseAvg=50)
    N = 1 << 16
    for i, c in enumerate(d["check"].tolist()):
        got = {key: np.concatenate([d["%s_%d_%d" % (key, c, k)] for k in range(2)]) for key in ("soft", "bits", "phase", "index")}
        ref = _oracle_calls(oracle_mod, props, [d["iq"][i, : 2 * N], d["iq"][i, 2 * N :]])
        assert_parity(got, ref, "channel %d" % c)


def _window_class_cfgs():
    cfgs = []
    Ss = list(range(2, 33)) + [33, 100]
    As = (1, 100, 129, 257, 513, 1025)
    for i, S in enumerate(Ss):
        for j, A in enumerate(As):
            if S * A > 65536:
                continue
            cfgs.append(dict(samplesPerBaud=S, numAvg=A, constelationSize=(2, 4, 8)[(i + j) % 3],
                             phaseAvg=(50, 4000)[(i * 7 + j) % 5 == 0], differentialDecoding=(i + j) % 2))
    return cfgs


def test_every_window_class_in_one_mixed_cs16_batch(oracle_mod):
    """samplesPerBaud 2 .. 32 and run-time-front ones (33, 100), numAvg 1 / 100 / 129 / 257 / 513 / 1025, phaseAvg 50 and
    4000, M 2 / 4 / 8, differential on and off: one batch, three calls with ragged cuts and odd element counts."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    cfgs = _window_class_cfgs()
    rng = np.random.default_rng(12)
    n_ch = len(cfgs)
    pieces = []
    for c, p in enumerate(cfgs):
        S, A = p["samplesPerBaud"], p["numAvg"]
        n = S * (A + 300) + int(rng.integers(0, 4000))
        iq = q16(synth_channel(31000 + c, p["constelationSize"], S, n))
        a, b = sorted(rng.choice(np.arange(1, n), 2, replace=False))
        segs = _cut(iq, [0, a, b, n])
        segs[0] = np.concatenate([segs[0], np.int16([123])])  # an odd element: ignored
        segs[2] = np.concatenate([segs[2], np.int16([-5])])
        pieces.append(segs)
    h = pl.Handle(n_ch, device=0, max_window_samples=65536 + 64, max_phase_avg=4096)
    h.configure(0, cfgs)
    got = _host_calls(h, pieces)
    assert h.stats()["channels_sequential"] == 0
    h.close()
    for c, p in enumerate(cfgs):
        assert_parity(got[c], _oracle_calls(oracle_mod, p, pieces[c]), "cfg %s" % p)


def _tie_streams(N, S):
    rng = np.random.default_rng(99)
    out = []
    for lsb in (1, 2, 3):
        out.append(rng.integers(-lsb, lsb + 1, 2 * N).astype(np.int16))
    out.append(np.zeros(2 * N, np.int16))
    out.append(np.full(2 * N, 3, np.int16))
    sq = np.where((np.arange(N) // S) % 2 == 0, 32767, -32768).astype(np.int16)
    iq = np.empty(2 * N, np.int16)
    iq[0::2] = sq
    iq[1::2] = sq[::-1]
    out.append(iq)
    # rectangular QPSK pulses of a few LSB with +-1 LSB noise: exact integer energy ties inside every symbol
    k = rng.integers(0, 4, N // S + 1)
    base = np.repeat(np.stack([(2, 2), (-2, 2), (-2, -2), (2, -2)])[k], S, axis=0)[:N]
    base = base + rng.integers(-1, 2, (N, 2))
    out.append(base.reshape(-1).astype(np.int16))
    return out


@pytest.mark.parametrize("ties_in_place", [1, 0])
@pytest.mark.parametrize("numAvg", [100, 400])
def test_exact_energy_ties_of_integer_samples(oracle_mod, monkeypatch, ties_in_place, numAvg):
    """A few LSBs of amplitude: the window sums of integer squares are exact and tie all the time.  The first-maximum rule
    and the exact-timing paths decide them, as the reference does."""
    from psk_soft_amd import lib as pl

    monkeypatch.setenv("PSK_SOFT_TIES_IN_PLACE", str(ties_in_place))
    S, N = 8, 20000
    streams = _tie_streams(N, S)
    props = dict(samplesPerBaud=S, constelationSize=4, numAvg=numAvg)
    h = pl.Handle(len(streams), device=0)
    h.configure(0, [props] * len(streams))
    cuts = [0, 7001, N]
    pieces = [_cut(x, cuts) for x in streams]
    got = []
    exact = 0
    for k in range(2):
        res = h.process_host(0, [dict(data=pieces[c][k], xdelta=0.01, sriChanged=(k == 0)) for c in range(len(streams))])
        got.append(res)
        st = h.stats()
        exact += st["timing_exact_blocks"] + st["channels_exact_timing"]
    assert exact > 0
    h.close()
    for c in range(len(streams)):
        g = {key: np.concatenate([got[k][c][key] for k in range(2)]) for key in ("soft", "bits", "phase", "index")}
        assert_parity(g, _oracle_calls(oracle_mod, props, pieces[c]), "tie stream %d" % c)


@pytest.mark.parametrize("n_ch", [1, 64])
def test_time_tiled_and_parallel_fit(oracle_mod, n_ch):
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    N, S, M = 1 << 18, 8, 4
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)
    streams = [q16(synth_channel(41000 + c, M, S, N)) for c in range(n_ch)]
    h = pl.Handle(n_ch, device=0)
    h.configure(0, [props] * n_ch)
    h.set_option(pl.Handle.OPT_TIME_TILED, 2)
    cuts = [0, 5000, N]
    pieces = [_cut(x, cuts) for x in streams]
    got = [dict(soft=[], bits=[], phase=[], index=[]) for _ in range(n_ch)]
    for k in range(2):
        res = h.process_host(0, [dict(data=pieces[c][k], xdelta=0.01, sriChanged=(k == 0)) for c in range(n_ch)])
        for c in range(n_ch):
            for key in got[c]:
                got[c][key].append(res[c][key])
    st = h.stats()
    assert st["channels_tiled"] == n_ch and st["channels_parallel_fit"] > 0, st
    h.close()
    for c in sorted({0, n_ch // 2, n_ch - 1}):
        assert_parity({k: np.concatenate(v) for k, v in got[c].items()}, _oracle_calls(oracle_mod, props, pieces[c]), "ch %d" % c)


def test_reference_order_kernel(oracle_mod):
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    cfgs = [(8, 4, 0), (10, 8, 1), (5, 2, 0), (1, 4, 0)]
    streams = [q16(synth_channel(42000 + c, M, S, 6000)) for c, (S, M, d) in enumerate(cfgs)]
    props = [dict(samplesPerBaud=S, constelationSize=M, differentialDecoding=d, numAvg=(0 if S == 1 else 100)) for S, M, d in cfgs]
    h = pl.Handle(len(cfgs), device=0)
    h.set_force_sequential(1)
    h.configure(0, props)
    pieces = [_cut(x, [0, 2500, 6000]) for x in streams]
    got = _host_calls(h, pieces)
    assert h.stats()["channels_sequential"] == len(cfgs)
    h.close()
    for c in range(len(cfgs)):
        assert_parity(got[c], _oracle_calls(oracle_mod, props[c], pieces[c]), "cfg %s" % (cfgs[c],))


def test_mixed_formats_and_a_channel_that_alternates(oracle_mod):
    """One call mixes CF32 and CS16 packets; channel 0 alternates CF32 / CS16 over five calls against ONE continuous oracle
    run: the carried window holds converted samples, channel state has no format."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    n_ch, N = 24, 40000
    props = [dict(samplesPerBaud=(8, 10, 4, 16)[c % 4], constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 200, 600)[c % 3])
             for c in range(n_ch)]
    streams = [q16(synth_channel(43000 + c, p["constelationSize"], p["samplesPerBaud"], N)) for c, p in enumerate(props)]
    cuts = [0, 3000, 11111, 20000, 20001, N]
    pieces = [_cut(x, cuts) for x in streams]
    h = pl.Handle(n_ch, device=0)
    h.configure(0, props)
    got = _host_calls(h, pieces, fmt_of=lambda c, k: (c + k) % 2 if c else k % 2)
    h.close()
    for c in range(n_ch):
        assert_parity(got[c], _oracle_calls(oracle_mod, props[c], pieces[c]), "ch %d" % c)


def _zero_copy(h, n_ch, pk_ptr, n_elems, fmt, cap, k):
    from psk_soft_amd import lib as pl

    soft = pl.host_alloc(n_ch * 2 * cap, np.float32).reshape(n_ch, 2 * cap)
    phase = pl.host_alloc(n_ch * cap, np.float32).reshape(n_ch, cap)
    sidx = pl.host_alloc(n_ch * cap, np.int16).reshape(n_ch, cap)
    bits = pl.host_alloc(n_ch * 3 * cap, np.int16).reshape(n_ch, 3 * cap)
    pk = (pl.Packet * n_ch)()
    out = (pl.Output * n_ch)()
    for c in range(n_ch):
        pk[c].data = pk_ptr(c)
        pk[c].n_floats = n_elems(c)
        pk[c].sri_xdelta = 0.01
        pk[c].sri_mode = 1
        pk[c].sriChanged = int(k == 0)
        pk[c].present = 1
        pk[c].format = fmt
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


def test_zero_copy_int16_from_page_locked_memory_and_alignment(oracle_mod):
    """CS16 packets in psk_soft_host_alloc memory handed to psk_soft_process_device, every one at an address 4 bytes past an
    8-byte boundary (the minimum for CS16); two calls.  A 2-byte aligned CS16 packet is refused, nothing committed."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    cfgs = [(8, 4), (10, 8), (7, 2), (16, 4)]
    n_ch, N = len(cfgs), 30000
    streams = [q16(synth_channel(44000 + c, M, S, N)) for c, (S, M) in enumerate(cfgs)]
    buf = pl.host_alloc(n_ch * (2 * N + 8), np.int16).reshape(n_ch, 2 * N + 8)
    h = pl.Handle(n_ch, device=0)
    h.configure(0, [dict(samplesPerBaud=S, constelationSize=M) for S, M in cfgs])
    cuts = [0, 13001, N]
    cap = N // 2 + 8
    got = [dict(soft=[], bits=[], phase=[], index=[]) for _ in range(n_ch)]
    for k in range(2):
        for c in range(n_ch):
            seg = streams[c][2 * cuts[k] : 2 * cuts[k + 1]]
            buf[c, 2 : 2 + seg.size] = seg
            assert (buf[c].ctypes.data + 4) % 8 == 4
        if k == 1:  # a 2-byte aligned packet: refused before anything runs
            before = [h.peek(c) for c in range(n_ch)]
            pk = (pl.Packet * 1)()
            out = (pl.Output * 1)()
            pk[0].data, pk[0].n_floats, pk[0].sri_xdelta, pk[0].sri_mode, pk[0].present = buf[0].ctypes.data + 2, 1000, 0.01, 1, 1
            pk[0].format = pl.FORMAT_CS16
            out[0].cap_symbols = 0
            assert pl.load().psk_soft_process_device(h._h, 0, 1, pk, out, None) == 1
            assert b"aligned (CS16: 4)" in pl.load().psk_soft_last_error()
            assert [h.peek(c) for c in range(n_ch)] == before
        res = _zero_copy(h, n_ch, lambda c: buf[c].ctypes.data + 4, lambda c: 2 * (cuts[k + 1] - cuts[k]), pl.FORMAT_CS16, cap, k)
        for c in range(n_ch):
            for key in got[c]:
                got[c][key].append(res[c][key])
    assert h.stats()["channels_sequential"] == 0
    h.close()
    pl.host_free(buf.reshape(-1))
    for c, (S, M) in enumerate(cfgs):
        assert_parity({k: np.concatenate(v) for k, v in got[c].items()},
                      _oracle_calls(oracle_mod, dict(samplesPerBaud=S, constelationSize=M), _cut(streams[c], cuts)), "S=%d M=%d" % (S, M))


def test_stamp_key_tells_the_formats_apart(oracle_mod):
    """A uniform 256-channel batch (the stamped path plans it once) in which one channel differs only in its format: the
    odd channel and its neighbours all match."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    C, N, odd = 256, 12000, 137
    props = dict(samplesPerBaud=8, constelationSize=4, numAvg=100)
    streams = [q16(synth_channel(45000 + c, 4, 8, N)) for c in range(C)]
    h = pl.Handle(C, device=0)
    h.configure_all(**props)
    pieces = [_cut(x, [0, 6000, N]) for x in streams]
    got = _host_calls(h, pieces, fmt_of=lambda c, k: 0 if (c == odd and k == 1) else 1)
    h.close()
    for c in (0, odd - 1, odd, odd + 1, C - 1):
        assert_parity(got[c], _oracle_calls(oracle_mod, props, pieces[c]), "ch %d" % c)


def test_host_class_with_a_short_input_port(oracle_mod):
    from psk_soft_amd import sandbox
    from psk_soft_amd.stimulus import synth_channel

    comp = sandbox.Component(device=0, input="short")
    comp.samplesPerBaud = 8
    comp.constelationSize = 8
    comp.numAvg = 100
    iq = q16(synth_channel(46000, 8, 8, 20000))
    pieces = _cut(iq, [0, 9000, 20000])
    for k, seg in enumerate(pieces):
        comp.push(seg, sampleRate=100, sriChanged=(k == 0))
        assert comp.service() == 1
    got = dict(soft=comp.getData("softDecision_dataFloat_out"), bits=comp.getData("bits_dataShort_out"),
               phase=comp.getData("phase_dataFloat_out"), index=comp.getData("sampleIndex_dataShort_out"))
    comp.close()
    assert_parity(got, _oracle_calls(oracle_mod, dict(samplesPerBaud=8, constelationSize=8, numAvg=100), pieces), "host class")
