"""psk_soft_process_device_strided on a real MI355X: packets that are columns of frame-major matrices (a channelizer's output,
[frame][channel]) are gathered on the GPU (psk_gather.hip) and then run like contiguous packets.  Every checked stream is,
bit for bit, what the oracle gives on the column's samples and what a handle of the same kind gives when it is fed the same
samples contiguously, under every schedule the library chooses; the launch trace (PSK_SOFT_TRACE_LAUNCHES=2) says which gather
kernel ran, and the source buffer comes back byte for byte as it was uploaded.

Everything around the channels' samples -- the other columns of a matrix, the frames behind a ragged channel's end -- holds
poison (NaN patterns for float32, 0x8000 / 0x80 for the integer formats): a gather that read one sample too many would show.
The samples are int8 values (round(40 x), clipped) cast to the packet's format, so exact energy ties are common."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_cs16 import _cut
from tests.test_gpu_cs16_schedules import (KEYS, assert_same, check_parity, oracle_calls, parse_trace, rounds, screened,
                                           untraced_then_traced, whats, _synth)
from tests.test_gpu_cs8 import H_CS8, SCALE8, device_run, q8
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

H_CS16 = 3
DTYPES = {"cf32": np.float32, "sc16": np.int16, "sc8": np.int8}
H_OF = {"cf32": 1, "sc16": H_CS16, "sc8": H_CS8}


def _poison(dtype):
    return {np.dtype(np.float32): np.uint32(0x7FC00ABC).view(np.float32), np.dtype(np.int16): np.int16(-32768),
            np.dtype(np.int8): np.int8(-128), np.dtype(np.float16): np.uint16(0x7E55).view(np.float16)}[np.dtype(dtype)]


def _fmt(pl, dtype):
    return {np.dtype(np.int8): pl.FORMAT_CS8, np.dtype(np.int16): pl.FORMAT_CS16,
            np.dtype(np.float16): pl.FORMAT_CF16}.get(np.dtype(dtype), pl.FORMAT_CF32)


def gathers(lines):
    """(tile launches, frame groups they cover, single launches, singles they cover) of one call's launch lines"""
    t = [x for x in lines if x["what"] == "gather_tiles"]
    s = [x for x in lines if x["what"] == "gather_singles"]
    return len(t), sum(x["cnt"] for x in t), len(s), sum(x["cnt"] for x in s)


def strided_run(h, calls, place, widths, capfd=None, check=None, sync_each=True, k0=0, odd=(), host_mem=False, stream=None, spans=None):
    """psk_soft_process_device_strided with the packets of call k laid out as `place` says: place[c] = None -- channel c's
    packet is contiguous (stride 1) -- or (m, col): it is column `col` of matrix m, widths[m] complex samples wide, as many frames
    as its longest channel of that call, everything else in it poison.  calls[k][c]: interleaved I/Q (float32 / int16 / int8) or
    None (no packet); the channels of one matrix share a format within a call.  odd: channels whose n_floats counts one element
    more than the packet has (an odd last element is ignored: nothing is there to read).  host_mem: the source lies in
    psk_soft_host_alloc memory instead of device memory.  All sources are uploaded in front of the first call and compared with
    what is there after the last.  stream: a raw hipStream_t, or a list of them, one per call (None: the handle's own).
    spans[k] = (ch0, nch): the channels call k covers (default: all of them; calls[k][c] is None outside).
    Returns ({c: [per-call dicts]} for c in check, [launch lines of call k], [n_symbols[k][c]])."""
    from psk_soft_amd import lib as pl

    K, C = len(calls), len(calls[0])
    check = list(range(C)) if check is None else list(check)
    al = lambda n: (n + 127) // 128 * 128  # noqa: E731
    src_parts, src_off = [], 0
    where = {}  # (k, c) -> (byte offset of sample 0, stride)
    for k in range(K):
        mats = {}
        for c in range(C):
            x = calls[k][c]
            if x is None:
                continue
            if place[c] is None:
                where[k, c] = (src_off, 1)
                part = np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8)
                src_parts.append(np.concatenate([part, np.full(al(part.size) - part.size, 0xEE, np.uint8)]))
                src_off += al(part.size)
            else:
                mats.setdefault(place[c][0], []).append(c)
        for m, chans in mats.items():
            dt = calls[k][chans[0]].dtype
            assert all(calls[k][c].dtype == dt for c in chans)
            frames = max(calls[k][c].size // 2 for c in chans)
            mat = np.full((frames, widths[m], 2), _poison(dt), dt)
            for c in chans:
                n = calls[k][c].size // 2
                mat[:n, place[c][1], :] = calls[k][c][: 2 * n].reshape(n, 2)
                where[k, c] = (src_off + place[c][1] * 2 * dt.itemsize, widths[m])
            part = np.frombuffer(mat.tobytes(), np.uint8)
            src_parts.append(np.concatenate([part, np.full(al(part.size) - part.size, 0xEE, np.uint8)]))
            src_off += al(part.size)
    src = np.concatenate(src_parts) if src_parts else np.zeros(128, np.uint8)
    lay, tot = {}, [0, 0, 0, 0]
    for k in range(K):
        for c in range(C):
            x = calls[k][c]
            if x is None:
                continue
            cap = h.output_capacity(c, x.size // 2)
            lay[k, c] = (cap, tuple(tot))
            for i, s in enumerate((8 * cap, 4 * cap, 6 * cap, 2 * cap)):
                tot[i] += al(s)
    bufs = [h.device_alloc(max(t, 128)) for t in tot]
    d_soft, d_phase, d_bits, d_sidx = bufs
    if host_mem:
        h_src = pl.host_alloc(src.size, np.uint8)
        h_src[:] = src
        base = h_src.ctypes.data
    else:
        base = h.device_alloc(src.size)
        h.upload(base, src)
    traces, nsym, outs = [], [], []
    try:
        h.synchronize()
        for k in range(K):
            lo, n = spans[k] if spans else (0, C)
            assert all(calls[k][c] is None for c in range(C) if not lo <= c < lo + n)
            pk, out = (pl.Packet * n)(), (pl.Output * n)()
            strides = [1] * n
            for c in range(lo, lo + n):
                x = calls[k][c]
                if x is None:
                    strides[c - lo] = widths[place[c][0]] if place[c] is not None else 1
                    continue
                cap, o = lay[k, c]
                p, q = pk[c - lo], out[c - lo]
                off, strides[c - lo] = where[k, c]
                p.data, p.n_floats, p.sri_xdelta, p.sri_mode = base + off, x.size + (1 if c in odd else 0), 0.01, 1
                p.sriChanged, p.present, p.format = int(k + k0 == 0), 1, _fmt(pl, x.dtype)
                q.soft, q.phase, q.bits, q.sampleIndex = d_soft + o[0], d_phase + o[1], d_bits + o[2], d_sidx + o[3]
                q.cap_symbols = cap
            if capfd:
                capfd.readouterr()
            h.process_device_strided(lo, pk, strides, out, stream[k] if isinstance(stream, list) else stream)
            if capfd:
                traces.append(parse_trace(capfd.readouterr().err))
            if sync_each:
                h.synchronize()
            outs.append({c: out[c - lo] for c in range(lo, lo + n)})
            nsym.append([int(out[c - lo].n_symbols) if lo <= c < lo + n else 0 for c in range(C)])
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
                got[c].append(dict(soft=h.download(d_soft + off[0], (2 * ns,), np.float32),
                                   phase=h.download(d_phase + off[1], (ns,), np.float32),
                                   bits=h.download(d_bits + off[2], (int(o.n_bits),), np.int16),
                                   # (n_sampleIndex is n_symbols, or 0 at samplesPerBaud 1: that row is not written)
                                   index=h.download(d_sidx + off[3], (int(o.n_sampleIndex),), np.int16)))
        after = np.array(h_src) if host_mem else h.download(base, (src.size,), np.uint8)
        assert np.array_equal(after, src), "the source buffer changed"
    finally:
        for b in bufs:
            h.device_free(b)
        if host_mem:
            pl.host_free(h_src)
        else:
            h.device_free(base)
    return got, traces, nsym


def contiguous(n_ch, props, calls, check=None, **limits):
    """the same calls through psk_soft_process_device on a fresh handle, contiguous packets"""
    from psk_soft_amd import lib as pl

    h = pl.Handle(n_ch, device=0, **limits)
    try:
        h.configure(0, props)
        return device_run(h, calls, None, check)[0]
    finally:
        h.close()


def _streams(seed, props, lens, dtype):
    """one int8-valued stream per channel in `dtype`, lens[c] complex samples"""
    Ms = [p["constelationSize"] for p in props]
    S = props[0]["samplesPerBaud"]
    return [q8(x).astype(dtype) for x in _synth(seed, Ms, S, list(lens))]


# ---- 1. a frame-major batch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cf32", "sc16", "sc8"])
def test_frame_major_batch(oracle_mod, monkeypatch, capfd, fmt):
    """96 channels -- columns 5 .. 100 of a matrix 128 wide --, ragged lengths, three calls carrying state: one frame group,
    the tile kernel, no singles; the integer formats still reach the in-place builds of the wave-scan kernels."""
    S, C, calls = 8, 96, 3
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 64, 25)[c % 3], phaseAvg=(50, 10, 200)[(c // 3) % 3],
                  differentialDecoding=int(c % 7 == 3)) for c in range(C)]
    lens = [[9000 + 131 * ((7 * c + 3 * k) % 61) + (c % 2) for c in range(C)] for k in range(calls)]
    streams = _streams(81000, props, [sum(lens[k][c] for k in range(calls)) for c in range(C)], DTYPES[fmt])
    data = [[streams[c][2 * sum(lens[j][c] for j in range(k)) : 2 * sum(lens[j][c] for j in range(k + 1))] for c in range(C)]
            for k in range(calls)]
    place = [(0, 5 + c) for c in range(C)]

    def run(h, cf):
        h.configure(0, props)
        got, traces, nsym = strided_run(h, data, place, {0: 128}, cf, odd=(0, 7, 95))
        st = h.stats()
        assert st["channels_sequential"] == 0 and st["channels_fast"] == C, st
        return got, traces, nsym

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (1, 1, 0, 0), (k, lines)
        assert lines[0]["what"] == "gather_tiles" and lines[0]["S"] == 2 * DTYPES[fmt]().itemsize, (k, lines[0])
        assert (S, H_OF[fmt]) in screened(lines), (k, screened(lines))
        assert not whats(lines) & {"cs16_convert", "cs8_convert"}, (k, whats(lines))
    assert_same(res[0][0], contiguous(C, props, data), "strided against contiguous")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "frame-major %s" % fmt)


# ---- 2. other shapes ----------------------------------------------------------------------------------------------------

def test_group_widths_and_tile_edges(oracle_mod, monkeypatch, capfd):
    """Frame groups 1, 3, 31, 33 and 65 columns wide, each in a matrix of its own (two columns wider, starting at column 1), the
    three formats in turn; calls of 63, 64, 65, 127 and 129 frames (the tile is 64 x 64) with ragged ends inside a group.
    The groups of 1 and 3 are gathered as singles, the others by the tile kernel."""
    S = 2
    gw = [1, 3, 31, 33, 65]
    frames = [63, 64, 65, 127, 129]
    fm = ["sc8", "sc16", "cf32", "sc8", "sc16"]
    place, props, dts = [], [], []
    for m, g in enumerate(gw):
        for j in range(g):
            place.append((m, 1 + j))
            dts.append(DTYPES[fm[m]])
            props.append(dict(samplesPerBaud=S, constelationSize=(4, 2, 8)[(m + j) % 3], numAvg=(10, 4, 25)[j % 3], phaseAvg=(5, 20)[j % 2]))
    C = len(place)
    lens = [[frames[k] - (j % 3 if k in (1, 4) else 0) for j in range(C)] for k in range(len(frames))]
    base = _streams(82000, props, [sum(lens[k][c] for k in range(len(frames))) for c in range(C)], np.int8)
    data = [[base[c][2 * sum(lens[j][c] for j in range(k)) : 2 * sum(lens[j][c] for j in range(k + 1))].astype(dts[c]) for c in range(C)]
            for k in range(len(frames))]

    def run(h, cf):
        h.configure(0, props)
        return strided_run(h, data, place, {m: g + 2 for m, g in enumerate(gw)}, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        # sc8: groups of 33 (tiles) and 1 (single); sc16: 65 (tiles) and 3 (singles); cf32: 31 (tiles)
        assert gathers(lines) == (3, 3, 2, 4), (k, lines)
        assert sorted((t["S"], t["cnt"]) for t in lines if t["what"] == "gather_singles") == [(2, 1), (4, 3)], (k, lines)
    assert_same(res[0][0], contiguous(C, props, data), "strided against contiguous")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "group widths")


@pytest.mark.parametrize("fmt", ["cf32", "sc8"])
def test_every_third_column_is_gathered_as_singles(oracle_mod, monkeypatch, capfd, fmt):
    S, C, calls, n = 4, 20, 2, 3001
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(30, 100)[c % 2]) for c in range(C)]
    streams = _streams(83000, props, [calls * n + c for c in range(C)], DTYPES[fmt])
    data = [[(streams[c][: 2 * n], streams[c][2 * n :])[k] for c in range(C)] for k in range(calls)]
    place = [(0, 3 * c) for c in range(C)]

    def run(h, cf):
        h.configure(0, props)
        return strided_run(h, data, place, {0: 3 * C}, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (0, 0, 1, C), (k, lines)
    assert_same(res[0][0], contiguous(C, props, data), "strided against contiguous")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "singles %s" % fmt)


def test_strided_and_contiguous_packets_formats_and_holes_in_one_call(oracle_mod, monkeypatch, capfd):
    """Channels 0 .. 19: columns of a float32 matrix; 20 .. 29: contiguous packets (a stride of 1) of the three formats;
    30 .. 41: columns of an int8 matrix; 42 .. 53: columns of an int16 matrix.  Call 1 has no packet for channels 9 and 35: the
    float group splits in two (9 and 10 columns wide), the int8 one into 5 + 6 columns, gathered as singles.  Call 2 brings
    packets for the contiguous channels only: no gather is launched."""
    S, C, n = 8, 54, 4100
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 200, 400, 50)[c % 4], phaseAvg=(50, 10)[c % 2])
             for c in range(C)]
    dt = [np.float32] * 20 + [(np.float32, np.int16, np.int8)[c % 3] for c in range(10)] + [np.int8] * 12 + [np.int16] * 12
    place = [(0, 2 + c) for c in range(20)] + [None] * 10 + [(1, c) for c in range(12)] + [(2, 20 + c) for c in range(12)]
    base = _streams(84000, props, [3 * n + 17 * c for c in range(C)], np.int8)
    cuts = lambda c: [0, n + c, 2 * n + 5 * c, 3 * n + 17 * c]  # noqa: E731
    data = [[_cut(base[c], cuts(c))[k].astype(dt[c]) for c in range(C)] for k in range(3)]
    for c in (9, 35):
        data[1][c] = None
    for c in list(range(20)) + list(range(30, C)):
        data[2][c] = None

    def run(h, cf):
        h.configure(0, props)
        return strided_run(h, data, place, {0: 24, 1: 12, 2: 40}, cf)

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    tr = res[1][1]
    assert gathers(tr[0]) == (3, 3, 0, 0), tr[0]
    assert gathers(tr[1]) == (2, 3, 1, 11), tr[1]
    assert sorted((t["S"], t["cnt"]) for t in tr[1] if t["what"] == "gather_tiles") == [(4, 1), (8, 2)], tr[1]
    assert gathers(tr[2]) == (0, 0, 0, 0), tr[2]
    assert_same(res[0][0], contiguous(C, props, data), "strided against contiguous")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "mixed call")


# ---- 3. schedules --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cf32", "sc16"])
def test_few_channels_with_long_calls_are_time_tiled(oracle_mod, monkeypatch, capfd, fmt):
    """12 channels, calls of 20 blocks and more, default options: the class goes to the time-tiled kernels (channels_tiled), which
    read the gathered rows (the int16 ones through the conversion pre-pass)."""
    S, C, calls = 8, 12, 2
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=100, phaseAvg=(10, 50, 200)[c % 3]) for c in range(C)]
    lens = [20 * 128 * S + 8 * (97 * c % 900) for c in range(C)]
    streams = _streams(85000, props, [calls * x for x in lens], DTYPES[fmt])
    data = [[streams[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]] for c in range(C)] for k in range(calls)]
    place = [(0, c) for c in range(C)]

    def run(h, cf):
        h.configure(0, props)
        got, traces, _ = strided_run(h, data, place, {0: C}, cf)
        return got, traces, h.stats()

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    assert res[0][2]["channels_tiled"] == C and res[0][2]["channels_sequential"] == 0, res[0][2]
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (1, 1, 0, 0) and lines[0]["what"] == "gather_tiles", (k, lines)
        assert any(t["what"] == "tile_front" for t in lines), (k, whats(lines))
        assert ("cs16_convert" in whats(lines)) == (fmt == "sc16"), (k, whats(lines))
    assert_same(res[0][0], contiguous(C, props, data), "strided against contiguous")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "time-tiled %s" % fmt)


def test_pipelined_ranges(oracle_mod, monkeypatch, capfd):
    """320 channels of one window class, calls of 260 blocks, default options: the pipelined mode of the time-tiled path
    (pipe_front lines), its three streams reading the gathered rows.  int8 columns of one matrix."""
    S, C, calls, n = 2, 320, 2, 260 * 128 * 2
    props = [dict(samplesPerBaud=S, constelationSize=4, numAvg=100, phaseAvg=50)] * C
    few = _streams(86000, props[:16], [calls * n + 64] * 16, np.int8)
    data = [[few[c % 16][2 * (k * n + c // 16) : 2 * ((k + 1) * n + c // 16)] for c in range(C)] for k in range(calls)]
    place = [(0, c) for c in range(C)]
    check = [0, 1, 15, 16, 100, 255, C - 1]

    def run(h, cf):
        h.configure(0, props)
        got, traces, _ = strided_run(h, data, place, {0: C}, cf, check)
        return got, traces, h.stats()

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    assert res[0][2]["channels_tiled"] == C and res[0][2]["channels_sequential"] == 0, res[0][2]
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (1, 1, 0, 0), (k, lines)
        assert sum(t["what"] == "pipe_front" for t in lines) >= 2, (k, whats(lines))
    assert_same(res[0][0], contiguous(C, props, data, check), "strided against contiguous")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "pipelined")


def test_a_mixed_batch_cut_in_time(oracle_mod, monkeypatch, capfd):
    """Four window classes side by side (float numAvg 100, int16 numAvg 100 read in place, float 200, float 400), calls of 130
    blocks and more: the library cuts every channel's call into PSK_SOFT_SPLIT_CLASSES pieces, each piece of a gathered row
    starting further along it."""
    S, C, calls, pieces = 4, 28, 2, 3
    kind = [c % 4 for c in range(C)]
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 100, 200, 400)[kind[c]], phaseAvg=(10, 50, 200)[(c // 4) % 3])
             for c in range(C)]
    lens = [S * (16640 + (211 * c) % 6300 + (c % 2)) for c in range(C)]
    base = _streams(87000, props, [calls * x for x in lens], np.int8)
    data = [[base[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]].astype(np.int16 if kind[c] == 1 else np.float32) for c in range(C)]
            for k in range(calls)]
    # (every class in a matrix of its own: no two neighbours of the call share one, so every packet is gathered as a single)
    place = [(kind[c], c // 4) for c in range(C)]
    env = dict(PSK_SOFT_SPLIT_CLASSES=pieces, PSK_SOFT_TIME_TILED=0)

    def run(h, cf):
        h.configure(0, props)
        return strided_run(h, data, place, {0: 7, 1: 7, 2: 7, 3: 7}, cf)

    res = untraced_then_traced(monkeypatch, capfd, env, C, run)
    classes = {(S, {0: 1, 1: H_CS16, 2: 2, 3: 4}[kind[c]]) for c in range(C)}
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (0, 0, 2, C), (k, lines)
        rest = [t for t in lines if not t["what"].startswith("gather_")]
        assert rounds(rest) == pieces, (k, rest)
        assert screened(lines) == {cl: pieces for cl in classes}, (k, screened(lines))
    monkeypatch.setenv("PSK_SOFT_SPLIT_CLASSES", str(pieces))
    monkeypatch.setenv("PSK_SOFT_TIME_TILED", "0")
    assert_same(res[0][0], contiguous(C, props, data), "strided against contiguous")
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "cut in time")


@pytest.mark.parametrize("fmt", ["cf32", "sc8"])
def test_one_channel_through_a_call_of_more_than_2_to_the_20_symbols(oracle_mod, monkeypatch, capfd, fmt):
    """samplesPerBaud 2, a call of 2^20 + 12345 symbols between two short ones, the channel in column 1 of a matrix 3 wide (a
    single): the library cuts the call, the pieces walk along the gathered row."""
    S, M = 2, 4
    n_sym = (1 << 20) + 12345
    lens = [5000 * S, n_sym * S, 7000 * S]
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)]
    iq = _streams(88000, props, [sum(lens)], DTYPES[fmt])[0]
    cuts = np.cumsum([0] + lens)
    data = [[iq[2 * cuts[k] : 2 * cuts[k + 1]]] for k in range(3)]
    lim = dict(max_packet_complex=n_sym * S + 16)
    env = dict(PSK_SOFT_TIME_TILED=0)

    def run(h, cf):
        h.configure(0, props)
        got, traces, nsym = strided_run(h, data, [(0, 1)], {0: 3}, cf, odd=(0,))
        st = h.stats()
        assert st["channels_sequential"] == 0 and st["channels_fast"] == 1, st
        return got, traces, nsym

    res = untraced_then_traced(monkeypatch, capfd, env, 1, run, **lim)
    assert res[0][2][1][0] > (1 << 20)
    long = res[1][1][1]
    assert gathers(long) == (0, 0, 1, 1) and long[0]["what"] == "gather_singles", long
    assert rounds(long[1:]) >= 2, long
    ref, _ = oracle_calls(oracle_mod, props[0], [d[0] for d in data])
    for k in range(3):
        assert_parity(res[0][0][0][k], ref[k], "long call %s, call %d" % (fmt, k))


def test_deferred_join_with_back_to_back_strided_calls(oracle_mod, monkeypatch, capfd):
    """PSK_SOFT_OPT_DEFERRED_JOIN, 96 channels of four window classes, six strided calls issued without a host wait on one
    stream, then join: every call gathers into the same scratch, which a class of the call before may still be reading on a
    side stream -- the entry joins before it gathers.  Outputs are those of the same calls made contiguously and joined."""
    from psk_soft_amd import lib as pl

    S, C, calls, n = 8, 96, 6, 6000
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    As = [(25, 100, 200, 400)[(c // 3) % 4] for c in range(C)]
    props = [dict(samplesPerBaud=S, constelationSize=Ms[c], numAvg=As[c], phaseAvg=(10, 50, 200)[(c // 12) % 3]) for c in range(C)]
    base = _streams(89000, props, [calls * n] * C, np.int8)
    # (a different length from call to call: the rows of consecutive calls do not coincide in the scratch)
    lens = [n - 501 * (k % 3) for k in range(calls)]
    data = [[base[c][2 * k * n : 2 * (k * n + lens[k])].astype(np.float32) for c in range(C)] for k in range(calls)]
    place = [(0, 3 + c) for c in range(C)]

    def run(h, cf):
        h.configure(0, props)
        h.set_option(pl.Handle.OPT_DEFERRED_JOIN, 1)
        got, traces, _ = strided_run(h, data, place, {0: 100}, cf, sync_each=False)
        return got, traces

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (1, 1, 0, 0), (k, lines)
        # (a deferred call: its classes end on their own streams; a joined call ends with the reference-order launch over the
        # whole batch, as the run without the option below shows)
        assert "seq (reference order)" not in whats(lines), (k, whats(lines))
        assert len(screened(lines)) >= 3, (k, screened(lines))
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    joined = pl.Handle(C, device=0)
    monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES")
    try:
        joined.configure(0, props)
        got_j, traces_j, _ = strided_run(joined, data, place, {0: 100}, capfd)
    finally:
        joined.close()
    assert all("seq (reference order)" in whats(lines) for lines in traces_j), [whats(lines) for lines in traces_j]
    assert_same(res[0][0], got_j, "deferred against joined")
    assert_same(res[0][0], contiguous(C, props, data), "deferred strided against joined contiguous")
    check_parity(oracle_mod, {c: res[0][0][c] for c in (0, 1, 2, 3, 9, 50, C - 1)}, lambda c: props[c], data, "deferred join")


def test_quality_records_equal_the_contiguous_run(oracle_mod, monkeypatch, capfd):
    """PSK_SOFT_OPT_QUALITY: the records of strided calls are byte for byte those of the contiguous calls."""
    from psk_soft_amd import lib as pl

    S, C, calls, n = 8, 40, 2, 5000
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 200)[c % 2], differentialDecoding=int(c % 5 == 0))
             for c in range(C)]
    base = _streams(90000, props, [calls * n + c for c in range(C)], np.int8)
    data = [[_cut(base[c], [0, n, calls * n + c])[k].astype((np.int16, np.float32, np.int8)[c // 14]) for c in range(C)] for k in range(calls)]
    place = [(c // 14, c % 14) for c in range(C)]
    recs = []

    def run(h, cf):
        h.configure(0, props)
        h.set_option(pl.Handle.OPT_QUALITY, 1)
        got, traces, _ = strided_run(h, data, place, {0: 14, 1: 16, 2: 14}, cf)
        recs.append(bytes(h.quality_records()))
        return got, traces

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (3, 3, 0, 0), (k, lines)
        assert [t["what"] for t in lines[-2:]] == ["quality_fold", "quality_join"], (k, lines)
    h = pl.Handle(C, device=0)
    try:
        h.configure(0, props)
        h.set_option(pl.Handle.OPT_QUALITY, 1)
        got_c = device_run(h, data)[0]
        want = bytes(h.quality_records())
    finally:
        h.close()
    assert_same(res[0][0], got_c, "strided against contiguous")
    assert recs[0] == want and recs[1] == want
    assert any(q.n_lock for q in (pl.Quality * C).from_buffer_copy(want))
    check_parity(oracle_mod, {c: res[0][0][c] for c in (0, 13, 14, 29, C - 1)}, lambda c: props[c], data, "quality")


def test_zero_copy_from_page_locked_memory(oracle_mod, monkeypatch, capfd):
    """The frame-major matrix lies in psk_soft_host_alloc memory: the gather reads it over the link, once."""
    S, C, calls, n = 8, 16, 2, 7000
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=100) for c in range(C)]
    streams = _streams(91000, props, [calls * n - c for c in range(C)], np.int16)
    data = [[_cut(streams[c], [0, n, calls * n - c])[k] for c in range(C)] for k in range(calls)]
    place = [(0, 1 + c) for c in range(C)]

    def run(h, cf):
        h.configure(0, props)
        return strided_run(h, data, place, {0: 19}, cf, host_mem=True)

    res = untraced_then_traced(monkeypatch, capfd, dict(PSK_SOFT_TIME_TILED=0), C, run)
    for k, lines in enumerate(res[1][1]):
        assert gathers(lines) == (1, 1, 0, 0), (k, lines)
        assert (S, H_CS16) in screened(lines), (k, lines)
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "zero copy")


# ---- 4. the machine-filling batch ------------------------------------------------------------------------------------------

# ---- the descriptor ring wraps with calls in flight ----------------------------------------------------------------------

@pytest.mark.parametrize("cover", ["six of eight", "all eight"])
def test_descriptor_ring_wraps_with_calls_in_flight_on_two_streams(oracle_mod, cover):
    """The nine calls of test_gpu_quality.wrapping_calls, their packets columns of a frame-major matrix 8 wide, issued back to back
    on the handle's stream and a second one in turn, one wait at the end: more calls than the gather descriptor ring has slots,
    each stream with a gather scratch of its own, the channel ranges overlapping across the streams.  Bit for bit the oracle.
    "six of eight": calls over channels [0, 6) and [2, 8) in turn, runs of six columns (below kGatherMinGroup: the plain strided
    gather); "all eight": every call over all eight columns (the tile kernel)."""
    from psk_soft_amd import lib as pl
    from tests.test_gpu_acquire import _second_stream
    from tests.test_gpu_quality import wrapping_calls

    props, calls, spans = wrapping_calls(92000, np.int16, None if cover == "six of eight" else [(0, 8)] * 9)
    C, K = 8, len(calls)
    second = _second_stream()
    h = pl.Handle(C, device=0)
    try:
        h.configure(0, props)
        got, _, nsym = strided_run(h, calls, [(0, c) for c in range(C)], {0: 8}, sync_each=False,
                                   stream=[None if k % 2 == 0 else second.value for k in range(K)], spans=spans)
        assert all(nsym[k][c] > 250 for k, (lo, n) in enumerate(spans) for c in range(lo, lo + n))
        check_parity(oracle_mod, got, lambda c: props[c], calls, "descriptor ring wrap, " + cover)
    finally:
        h.close()
        pl.load().hipStreamDestroy(second)


def _machine_child(path):
    """(a fresh process, torch initialised before the library) 4096 channels x 2^16 samples, frame-major and device-resident,
    two calls; saves the stimulus and the outputs of the checked channels, and the statistics, to `path`"""
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    C, N, S, M, W = 4096, 1 << 16, 8, 4, 4100
    dev = torch.device("cuda", 0)
    iq = torch.clamp(torch.round(synth_channels_torch(C, M, S, 2 * N, dev) * SCALE8), -128, 127)  # (C, 4N) floats: int8 values
    check = sorted(set(range(0, C, 32)) | {1, C - 1})
    save = {"check": np.array(check), "iq": iq[check].cpu().numpy().astype(np.int8)}
    cap = (N // S + 2 + 63) // 64 * 64
    for name, tdt, fmt in (("cf32", torch.float32, pl.FORMAT_CF32), ("sc8", torch.int8, pl.FORMAT_CS8)):
        poison = float("nan") if tdt == torch.float32 else -128
        mats = []
        for k in range(2):  # [frame][column][I, Q], the channels in columns 2 .. 4097
            m = torch.full((N, W, 2), poison, dtype=tdt, device=dev)
            m[:, 2 : 2 + C, :] = iq[:, 2 * k * N : 2 * (k + 1) * N].reshape(C, N, 2).permute(1, 0, 2).to(tdt)
            mats.append(m)
        as_int = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)  # noqa: E731  (NaNs compare as bits)
        copies = [m.clone() for m in mats]
        out_t = [torch.zeros((2, C, 2 * cap), dtype=torch.float32, device=dev), torch.zeros((2, C, cap), dtype=torch.float32, device=dev),
                 torch.zeros((2, C, cap), dtype=torch.int16, device=dev), torch.zeros((2, C, 2 * cap), dtype=torch.int16, device=dev)]
        torch.cuda.synchronize()
        os.environ["PSK_SOFT_TRACE_LAUNCHES"] = "2"
        h = pl.Handle(C, device=0)
        os.environ.pop("PSK_SOFT_TRACE_LAUNCHES", None)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)
        fast, seq, ns = [], [], []
        for k in range(2):
            pk, strides = pl.frame_major_packets(mats[k].data_ptr(), N, W, 2, C, fmt, xdelta=0.01, sriChanged=(k == 0))
            out = (pl.Output * C)()
            for c in range(C):
                out[c].soft, out[c].phase = out_t[0][k, c].data_ptr(), out_t[1][k, c].data_ptr()
                out[c].sampleIndex, out[c].bits = out_t[2][k, c].data_ptr(), out_t[3][k, c].data_ptr()
                out[c].cap_symbols = cap
            sys.stderr.write("[strided-test] %s call %d\n" % (name, k))
            sys.stderr.flush()
            h.process_device_strided(0, pk, strides, out)
            h.synchronize()
            st = h.stats()
            fast.append(st["channels_fast"])
            seq.append(st["channels_sequential"])
            ns.append([int(out[c].n_symbols) for c in range(C)])
        h.close()
        save[name + "_fast"], save[name + "_seq"] = np.array(fast), np.array(seq)
        save[name + "_src_same"] = np.array([bool(torch.equal(as_int(m), as_int(x))) for m, x in zip(mats, copies)])
        for c in check:
            for k in range(2):
                n = ns[k][c]
                save["%s_soft_%d_%d" % (name, c, k)] = out_t[0][k, c, : 2 * n].cpu().numpy()
                save["%s_phase_%d_%d" % (name, c, k)] = out_t[1][k, c, :n].cpu().numpy()
                save["%s_index_%d_%d" % (name, c, k)] = out_t[2][k, c, :n].cpu().numpy()
                save["%s_bits_%d_%d" % (name, c, k)] = out_t[3][k, c, : 2 * n].cpu().numpy()
        del mats, copies, out_t
        torch.cuda.empty_cache()
    np.savez(path, **save)


def test_machine_filling_frame_major_batch(oracle_mod, tmp_path):
    """4096 channels x 2^16 samples, QPSK, samplesPerBaud 8, frame-major in device memory (a matrix 4100 wide), float32 and int8,
    two calls: one frame group through the tile kernel, every channel on the wave-scan kernels (the int8 rows read in place),
    130 channels spread over the batch against the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "machine.npz")
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_strided as t; t._machine_child(%r)" % path], cwd=root,
                       capture_output=True, timeout=1200)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = np.load(path)
    err = r.stderr.decode()
    props = dict(samplesPerBaud=8, constelationSize=4, numAvg=100, phaseAvg=50)
    N = 1 << 16
    assert len(d["check"]) == 130
    for name, H in (("cf32", 1), ("sc8", H_CS8)):
        assert d[name + "_fast"].tolist() == [4096, 4096] and d[name + "_seq"].tolist() == [0, 0]
        assert d[name + "_src_same"].tolist() == [True, True]
        for k in range(2):
            lines = parse_trace(err.split("[strided-test] %s call %d\n" % (name, k))[1].split("[strided-test]")[0])
            assert gathers(lines) == (1, 1, 0, 0), lines
            assert screened(lines) == {(8, H): 1}, lines
            assert not whats(lines) & {"cs8_convert", "tile_front"}, whats(lines)
    for i, c in enumerate(d["check"].tolist()):
        ref, _ = oracle_calls(oracle_mod, props, [d["iq"][i, : 2 * N], d["iq"][i, 2 * N :]])
        for name in ("cf32", "sc8"):
            for k in range(2):
                got = {key: d["%s_%s_%d_%d" % (name, key, c, k)] for key in KEYS}
                assert_parity(got, ref[k], "%s channel %d call %d" % (name, c, k))
