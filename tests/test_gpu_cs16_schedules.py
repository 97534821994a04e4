"""Complex int16 (CS16) packets under the schedules other than the joined one: a mixed batch cut in time, long calls cut by the
library, the deferred join, automatic time tiling (also on the stamped path), pipelined ranges, and the conversion scratch
shared by more caller streams than it has buffers.  Every output stream of every checked channel bit for bit what the oracle
gives on the float32 cast of the same int16 values, over two or more consecutive calls.

Each test also shows that the schedule it is named for ran.  A second handle, created with PSK_SOFT_TRACE_LAUNCHES=2, is fed
the same input: its launch lines (one per launch, on stderr) say which kernels ran in which pieces, and its outputs must be the
untraced run's.  The parity run itself is untraced: a traced run waits for the device in front of every launch, which would
hide a missing stream wait."""

import os
import re
import subprocess
import sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.test_gpu_cs16 import q16
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

KEYS = ("soft", "bits", "phase", "index")
H_CS16 = 3  # the window class of CS16 packets read in place (psk_ctl.h: kPktFormats)
_LINE = re.compile(r"\[psk_soft\] ok; next: (?P<what>.+?) S=(?P<S>-?\d+) H=(?P<H>-?\d+) ch0=\d+ cnt=(?P<cnt>\d+) .*?"
                   r"slot=(?P<slot>\d+) stream=(?P<stream>\S+)")


def parse_trace(text):
    """the launch lines of PSK_SOFT_TRACE_LAUNCHES=2: [dict(what, S, H, cnt, slot, stream)] in launch order"""
    out = []
    for line in text.splitlines():
        m = _LINE.search(line)
        if m:
            out.append(dict(what=m["what"], S=int(m["S"]), H=int(m["H"]), cnt=int(m["cnt"]), slot=int(m["slot"]), stream=m["stream"]))
    return out


def screened(lines):
    """(S, H) -> launches of the screened tier: one per piece of the call that has channels of the class"""
    return Counter((t["S"], t["H"]) for t in lines if t["what"] == "fast (screened tier)")


def rounds(lines):
    """pieces the call ran in: every piece takes the next plan slot"""
    return sum(1 for i, t in enumerate(lines) if i == 0 or t["slot"] != lines[i - 1]["slot"])


def whats(lines):
    return {t["what"] for t in lines}


def _env(monkeypatch, env, trace):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    if trace:
        monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    else:
        monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES", raising=False)


def untraced_then_traced(monkeypatch, capfd, env, n_ch, body, **limits):
    """body(handle, capfd or None) on a handle created under `env`, then on one created under `env` with the launch trace on;
    the two must give the same outputs (body's first result, {channel: [per-call dicts]}).  Returns both results."""
    from psk_soft_amd import lib as pl

    res = []
    for trace in (False, True):
        _env(monkeypatch, env, trace)
        h = pl.Handle(n_ch, device=0, **limits)
        try:
            capfd.readouterr()
            res.append(body(h, capfd if trace else None))
        finally:
            h.close()
    monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES", raising=False)
    assert_same(res[0][0], res[1][0], "traced run")
    return res


def assert_same(a, b, ctx):
    """{channel: [per-call dicts]} equal as bit patterns"""
    assert a.keys() == b.keys(), ctx
    for c in a:
        assert len(a[c]) == len(b[c]), ctx
        for k, (x, y) in enumerate(zip(a[c], b[c])):
            if x is None or y is None:
                assert x is None and y is None, ctx
                continue
            for key in KEYS:
                assert x[key].dtype == y[key].dtype and np.array_equal(x[key].view(np.uint8), y[key].view(np.uint8)), \
                    "%s: channel %d call %d, %s differs" % (ctx, c, k, key)


def device_run(h, calls, capfd=None, check=None, sync_each=True, stream=None, before=None, k0=0):
    """psk_soft_process_device with device-resident packets: calls[k][c] = interleaved I/Q of channel c in call k, int16 (CS16)
    or float32 (CF32), or None (no packet).  Every (call, channel) has input and output rows of its own, all inputs uploaded in
    front of the first call.  sync_each=False: the calls are issued back to back, then joined and synchronised.  k0: the
    number of the first call in the channels' streams (sriChanged on call 0 only).
    Returns ({c: [dict(soft, bits, phase, index) per call]} for c in `check`, [launch lines of call k], [n_symbols[k][c]])."""
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
            sizes = (x.nbytes, 8 * cap, 4 * cap, 6 * cap, 2 * cap)  # input, soft, phase, bits (3 a symbol at most), sampleIndex
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
                pk[c].sriChanged, pk[c].present = int(k + k0 == 0), 1
                pk[c].format = pl.FORMAT_CS16 if x.dtype == np.int16 else pl.FORMAT_CF32
                out[c].soft, out[c].phase, out[c].bits, out[c].sampleIndex = d_soft + o[1], d_phase + o[2], d_bits + o[3], d_sidx + o[4]
                out[c].cap_symbols = cap
            if capfd:
                capfd.readouterr()
            h.process_device(0, pk, out, stream)
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
                assert int(o.n_sampleIndex) == ns
                got[c].append(dict(soft=h.download(d_soft + off[1], (2 * ns,), np.float32),
                                   phase=h.download(d_phase + off[2], (ns,), np.float32),
                                   bits=h.download(d_bits + off[3], (int(o.n_bits),), np.int16),
                                   index=h.download(d_sidx + off[4], (ns,), np.int16)))
    finally:
        for b in bufs:
            h.device_free(b)
    return got, traces, nsym


def host_run(h, calls, capfd=None, check=None, k0=0):
    """the same through psk_soft_process_host"""
    K, C = len(calls), len(calls[0])
    check = list(range(C)) if check is None else list(check)
    got, traces = {c: [] for c in check}, []
    for k in range(K):
        if capfd:
            capfd.readouterr()
        res = h.process_host(0, [None if x is None else dict(data=x, xdelta=0.01, sriChanged=(k + k0 == 0)) for x in calls[k]])
        if capfd:
            traces.append(parse_trace(capfd.readouterr().err))
        for c in check:
            got[c].append(None if calls[k][c] is None else {key: res[c][key] for key in KEYS})
    return got, traces


def oracle_calls(oracle_mod, props, pieces, sri_first=True, o=None):
    """the oracle, one service() call per piece (None: no packet), on the float32 cast; returns per-call dicts (and the
    component, to be continued)"""
    if o is None:
        o = oracle_mod.OracleComponent()
        for k, v in props.items():
            setattr(o, k, v)
    out = []
    for k, seg in enumerate(pieces):
        if seg is None:
            out.append(None)
            continue
        r = o.service(np.asarray(seg).astype(np.float32), 0.01, sriChanged=(sri_first and k == 0))
        out.append(dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index))
    return out, o


def check_parity(oracle_mod, got, props_of, calls, ctx):
    """every checked channel, call by call, against the oracle"""
    for c, per_call in got.items():
        ref, _ = oracle_calls(oracle_mod, props_of(c), [calls[k][c] for k in range(len(calls))])
        for k, (g, r) in enumerate(zip(per_call, ref)):
            if r is None:
                assert g is None
                continue
            assert_parity(g, r, "%s, channel %d call %d (%s)" % (ctx, c, k, props_of(c)))


def _synth(seeds, Ms, S, n):
    from psk_soft_amd.stimulus import synth_channel

    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda c: synth_channel(seeds + c, Ms[c], S, n[c] if isinstance(n, list) else n), range(len(Ms))))


# ---- 1. a mixed batch with CS16 read in place, cut in time ------------------------------------------------------------------

def _mixed_cut_batch(C, S, calls, prepass):
    """four window classes in turn: float numAvg <= 128 (H=1), CS16 numAvg <= 128 (read in place, H=3), float 200 (H=2),
    float 400 (H=4); calls of 130 ... 180 blocks, ragged.  Channel 5: too short to cut; channel 6: fewer blocks than pieces x
    128; channels 9 (CS16) and 10 (CF32): packets with an odd element at the end; odd channels one symbol longer.  prepass: channel 7 is a
    CS16 channel at numAvg 400 (converted in front of the call)."""
    kind = [c % 4 for c in range(C)]
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    props = [dict(samplesPerBaud=S, constelationSize=Ms[c], numAvg=((25, 100)[c % 8 // 4], (64, 128, 100)[c % 3], 200, 400)[kind[c]],
                  phaseAvg=(10, 50, 200)[(c // 4) % 3], differentialDecoding=int(c % 5 == 1)) for c in range(C)]
    lens = [S * (16640 + (211 * c) % 6300 + (c % 2)) for c in range(C)]
    lens[5], lens[6] = 9000, S * 70 * 128
    cs16 = [kind[c] == 1 for c in range(C)]
    if prepass:
        cs16[7] = True  # (kind 3: numAvg 400)
    host = _synth(52000, Ms, S, [calls * n for n in lens])
    pieces = []
    for k in range(calls):
        row = []
        for c in range(C):
            x = host[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]]
            if cs16[c]:
                x = q16(x)
                if c == 9:
                    x = np.concatenate([x, np.int16([-77])])
            elif c == 10:
                x = np.concatenate([x, np.float32([0.5])])
            row.append(x)
        pieces.append(row)
    return props, pieces, kind


@pytest.mark.parametrize("pieces", [2, 3, 5])
@pytest.mark.parametrize("variant", ["untiled", "default"])
def test_cs16_in_place_inside_a_mixed_batch_cut_in_time(oracle_mod, monkeypatch, capfd, pieces, variant):
    """The CS16 class read in place (H=3) inside a mixed batch that the library cuts into PSK_SOFT_SPLIT_CLASSES pieces:
    each piece of an int16 packet starts elem_bytes(CS16) x the elements before it further on, and the pieces carry the call's
    rounding bounds (PLAN_CARRY_DRIFT).  "untiled": 28 channels with PSK_SOFT_TIME_TILED=0; "default": default options, every
    class of more than 64 channels and under 192 blocks, so that nothing goes to the time-tiled kernels by itself."""
    S, calls = 4, 2
    C = 28 if variant == "untiled" else 264
    env = dict(PSK_SOFT_SPLIT_CLASSES=pieces)
    if variant == "untiled":
        env["PSK_SOFT_TIME_TILED"] = 0
    props, data, kind = _mixed_cut_batch(C, S, calls, prepass=False)
    check = sorted({0, 1, 2, 3, 5, 6, 9, 10, 13, C - 2, C - 1})
    res = untraced_then_traced(monkeypatch, capfd, env, C, lambda h, cf: (h.configure(0, props), device_run(h, data, cf, check))[1])
    got, _, nsym = res[0]
    _, traces, _ = res[1]
    check_parity(oracle_mod, got, lambda c: props[c], data, "cut in %d (%s)" % (pieces, variant))
    assert any(n % 2 for row in nsym for n in row), "no call emitted an odd number of symbols"
    classes = {(S, {0: 1, 1: H_CS16, 2: 2, 3: 4}[kind[c]]) for c in range(C)}
    for k, lines in enumerate(traces):
        assert rounds(lines) == pieces, (k, lines)
        assert screened(lines) == {cl: pieces for cl in classes}, (k, screened(lines))
        assert not whats(lines) & {"cs16_convert", "tile_front"}, (k, whats(lines))


def test_cs16_pre_pass_channel_keeps_the_mixed_batch_whole(oracle_mod, monkeypatch, capfd):
    """The same batch with one CS16 channel at numAvg 400: its packets are converted in front of the call (the conversion
    scratch is one per stream), and such a call is not cut -- one launch per class, a cs16_convert line."""
    S, C, calls = 4, 28, 2
    props, data, kind = _mixed_cut_batch(C, S, calls, prepass=True)
    check = [0, 1, 3, 7, 9, C - 1]
    env = dict(PSK_SOFT_SPLIT_CLASSES=3, PSK_SOFT_TIME_TILED=0)
    res = untraced_then_traced(monkeypatch, capfd, env, C, lambda h, cf: (h.configure(0, props), device_run(h, data, cf, check))[1])
    got, traces = res[0][0], res[1][1]
    check_parity(oracle_mod, got, lambda c: props[c], data, "pre-pass channel in a mixed batch")
    for k, lines in enumerate(traces):
        assert rounds(lines) == 1, (k, lines)
        sc = screened(lines)
        assert sc[(S, H_CS16)] == 1 and set(sc.values()) == {1}, (k, sc)
        assert "cs16_convert" in whats(lines), (k, whats(lines))


# ---- 3. calls longer than 2^20 symbols, cut by the library --------------------------------------------------------------

@pytest.mark.parametrize("variant", ["in_place", "tiled", "pre_pass", "pre_pass_grows"])
def test_long_cs16_calls_in_pieces(oracle_mod, monkeypatch, capfd, variant):
    """A CS16 call of more than 2^20 symbols at samplesPerBaud 2 between a short call and a call after it, through
    process_device and process_host.  in_place: numAvg 100 read in place (time tiling off: one channel of a long call would go
    to the tiled kernels and with them to the conversion); tiled: the same with default options (converted per piece, time
    tiled); pre_pass: numAvg 400, converted once per piece, after a first call of 900 000 symbols (on the caller's stream it
    leaves the conversion scratch large enough for the pieces); pre_pass_grows: the same after a short first call -- the
    scratch grows at the long call's first piece.  The long
    packet ends in an odd element (ignored)."""
    S, M = 2, 4
    A = 100 if variant in ("in_place", "tiled") else 400
    n0 = 900000 if variant == "pre_pass" else 5000
    n_sym = (1 << 20) + 12345
    lens = [n0 * S, n_sym * S, 7000 * S]
    iq = q16(_synth(53000, [M], S, [sum(lens)])[0])
    cuts = np.cumsum([0] + lens)
    seq = [[iq[2 * cuts[k] : 2 * cuts[k + 1]]] for k in range(3)]
    seq[1][0] = np.concatenate([seq[1][0], np.int16([5])])
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
            assert screened(long) == {(S, H_CS16): rounds(long)} and "cs16_convert" not in whats(long), (entry, long)
        elif variant == "tiled":
            assert sum(t["what"] == "tile_front" and t["H"] == 1 for t in long) == rounds(long), (entry, long)
            assert sum(t["what"] == "cs16_convert" for t in long) == rounds(long), (entry, long)
        else:
            assert screened(long) == {(S, 4): rounds(long)}, (entry, long)
            assert sum(t["what"] == "cs16_convert" for t in long) == rounds(long), (entry, long)
        for k in range(3):
            assert_parity(got[0][k], ref[k], "%s %s call %d" % (variant, entry, k))


# ---- 4. the deferred join with a CS16 class ---------------------------------------------------------------------------------

# ChanState (psk_plan.h) field by field, for naming what differs between two state blobs
_STATE_FIELDS = [("lf_ySum", 8), ("lf_xySum", 8), ("last_re", 4), ("last_im", 4), ("phaseEstimate", 4), ("lf_den", 4), ("lf_xavg", 4),
                 ("lf_m", 4), ("lf_b", 4), ("guard", 4), ("stat_blocks", 4), ("stat_extra", 4), ("last_k", 4), ("stat_exact", 4),
                 ("stat_chain", 4), ("emax_hint", 4), ("pad_state", 4), ("stat_pfit", 4)]


def blob_diff(a, b):
    """the parts of two psk_soft_export_state blobs that differ: header, ctl, ChanState fields by name, ring, yvals"""
    assert len(a) == len(b)
    ctl_b, st_b = np.frombuffer(a[16:24], np.uint32)
    parts = [("header", 24), ("ctl", int(ctl_b))]
    assert sum(n for _, n in _STATE_FIELDS) == st_b
    parts += [("state." + f, n) for f, n in _STATE_FIELDS]
    ring_cap = int(np.frombuffer(a[8:12], np.uint32)[0])
    parts += [("ring", 8 * ring_cap), ("yvals", len(a) - 24 - int(ctl_b) - int(st_b) - 8 * ring_cap)]
    out, off = [], 0
    for name, n in parts:
        if a[off : off + n] != b[off : off + n]:
            out.append(name)
        off += n
    return out


def test_deferred_join_with_a_cs16_class(oracle_mod, monkeypatch, capfd):
    """PSK_SOFT_OPT_DEFERRED_JOIN with CS16 packets read in place: their class (H=3) ends its calls on a side stream, and the
    calls the exactness guard hands over are redone there (launch_seq_cs16).  384 channels, eight calls issued without a host
    wait, every call into buffers of its own.  Channels 4 and 5 (same window class, numAvg 100) swap formats CS16 <-> CF32 from
    call 3 on: the class counts stay, the channel lists differ, the library has to join first.  In call 5 channel 9 (numAvg 400)
    sends CS16: a pre-pass call, which runs joined.  Channel 16 trips the exactness guard.  The channel states afterwards are
    the ones the same calls leave joined; imported into a fresh handle they go on as the oracle does."""
    from psk_soft_amd import lib as pl

    S, C, calls, n = 8, 384, 8, 6000
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    As = [(25, 100, 200, 400)[(c // 3) % 4] for c in range(C)]
    props = [dict(samplesPerBaud=S, constelationSize=Ms[c], numAvg=As[c], phaseAvg=(10, 50, 200)[(c // 12) % 3]) for c in range(C)]
    a, b, p, g = 4, 5, 9, 16
    assert As[a] == As[b] == 100 and As[p] == 400 and As[g] == 100 and a % 2 == 0 and g % 2 == 0
    props[g]["constelationSize"] = Ms[g] = 4
    host = [q16(x) for x in _synth(54000, Ms, S, (calls + 2) * n)]
    rng = np.random.default_rng(16)
    host[g] = rng.integers(-2, 3, 2 * (calls + 2) * n).astype(np.int16)
    for k in range(calls + 2):  # a QPSK burst at full scale in the middle of every call
        i0 = k * n + 2000
        host[g][2 * i0 : 2 * (i0 + 256)] = rng.choice(np.int16([-32768, 32767]), 512)

    def cs16(c, k):
        if c in (a, b) and k >= 3:
            return c == b
        if c == p:
            return k == 5
        return As[c] <= 100 and c % 2 == 0

    data = [[host[c][2 * k * n : 2 * (k + 1) * n] if cs16(c, k) else host[c][2 * k * n : 2 * (k + 1) * n].astype(np.float32)
             for c in range(C)] for k in range(calls)]
    check = sorted({0, 1, 2, a, b, p, g, 100, 101, 203, C - 2, C - 1})
    exp = [0, a, b, p, g, C - 1]

    def body(deferred):
        def run(h, cf):
            h.configure(0, props)
            if deferred:
                h.set_option(pl.Handle.OPT_DEFERRED_JOIN, 1)
            got, traces, _ = device_run(h, data, cf, check, sync_each=not deferred)
            st = h.stats()  # (of the last call: the guard has handed channel g over, nothing else left the wave-scan kernels)
            assert st["channels_sequential"] == st["channels_guard"] == h.channel_stats(g, 1)[0]["channels_guard"] == 1, st
            return got, traces, [h.export_state(c) for c in exp]
        return run

    res = untraced_then_traced(monkeypatch, capfd, {}, C, body(True))
    got, blobs = res[0][0], res[0][2]
    joined = pl.Handle(C, device=0)
    try:
        joined.configure(0, props)
        got_j, _, _ = device_run(joined, data, None, check)
        blobs_j = [joined.export_state(c) for c in exp]
    finally:
        joined.close()
    assert_same(got, got_j, "deferred against joined")
    for c, x, y in zip(exp, blobs, blobs_j):
        assert x == y, "channel %d: the state blobs differ in %s" % (c, blob_diff(x, y))
    # the states go on in a fresh handle: two more calls, CS16
    fresh = pl.Handle(len(exp), device=0)
    try:
        for i, blob in enumerate(blobs):
            fresh.import_state(i, blob)
        more = [[host[c][2 * k * n : 2 * (k + 1) * n] for c in exp] for k in (calls, calls + 1)]
        got_f, _ = host_run(fresh, more, k0=calls)
    finally:
        fresh.close()
    for c in check:
        K = calls + 2 if c in exp else calls
        ref, _ = oracle_calls(oracle_mod, props[c], [host[c][2 * k * n : 2 * (k + 1) * n] for k in range(K)])
        for k in range(K):
            g_k = got[c][k] if k < calls else got_f[exp.index(c)][k - calls]
            assert_parity(g_k, ref[k], "deferred join, channel %d call %d" % (c, k))
    # the schedule: H=3 is not the first class launched (the caller's stream) but on a side stream; every call but 5 deferred
    # (a joined call ends with the reference-order launch over the whole batch), call 5 joined
    for k, lines in enumerate(res[1][1]):
        sc = screened(lines)
        assert sc[(S, H_CS16)] == 1 and lines[0]["H"] != H_CS16, (k, sc)
        if k == 5:
            assert {"cs16_convert", "seq (reference order)"} <= whats(lines), (k, whats(lines))
        else:
            assert not whats(lines) & {"cs16_convert", "seq (reference order)"}, (k, whats(lines))


# ---- 5. automatic time tiling with CS16 channels --------------------------------------------------------------------------

def _tiled_check(lines, k):
    w = whats(lines)
    assert "cs16_convert" in w and any(t["what"] == "tile_front" and t["H"] == 1 for t in lines), (k, w)
    assert not any(t["H"] == H_CS16 for t in lines), (k, lines)


def test_automatic_tiling_of_a_mixed_format_class(oracle_mod, monkeypatch, capfd):
    """48 channels at samplesPerBaud 8, numAvg 100, CF32 and CS16 alternating, calls of 16 blocks and more, default options:
    the class goes to the time-tiled kernels by itself, and its CS16 channels with it -- folded back into the float class and
    converted in front of the call, not read in place."""
    S, C, calls = 8, 48, 2
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=100, phaseAvg=(10, 50, 200)[c % 3],
                  differentialDecoding=int(c % 5 == 2)) for c in range(C)]
    lens = [16 * 128 * S + 8 * (97 * c % 900) + (3 if c == 7 else 0) * S for c in range(C)]
    host = _synth(55000, [p["constelationSize"] for p in props], S, [calls * x for x in lens])
    data = [[q16(host[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]]) if c % 2 == 0
             else q16(host[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]]).astype(np.float32) for c in range(C)] for k in range(calls)]

    def run(h, cf):
        h.configure(0, props)
        got, traces, _ = device_run(h, data, cf, [0, 1, 2, 7, 24, C - 1], before=None)
        return got, traces, h.stats()

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    assert res[0][2]["channels_tiled"] == C and res[0][2]["channels_sequential"] == 0, res[0][2]
    for k, lines in enumerate(res[1][1]):
        _tiled_check(lines, k)
    check_parity(oracle_mod, res[0][0], lambda c: props[c], data, "tiled mixed formats")


def test_automatic_tiling_of_a_uniform_cs16_batch_stamped_and_not(oracle_mod, monkeypatch, capfd):
    """A uniform CS16 batch (configure_all, one length, one format): the stamped path plans it once, and its CS16 class, time
    tiled, is folded back all the same.  PSK_SOFT_STAMP=0 (every channel planned on its own) gives the same outputs."""
    from psk_soft_amd import lib as pl

    S, C, calls, n = 8, 48, 3, 2600 * 8
    props = dict(samplesPerBaud=S, constelationSize=4, numAvg=100, phaseAvg=50)
    host = _synth(56000, [4] * C, S, calls * n)
    data = [[q16(host[c][2 * k * n : 2 * (k + 1) * n]) for c in range(C)] for k in range(calls)]
    check = [0, 1, 23, C - 1]

    def run(h, cf):
        h.configure_all(**props)
        got, traces, _ = device_run(h, data, cf, check)
        return got, traces, h.stats()

    res = untraced_then_traced(monkeypatch, capfd, {}, C, run)
    assert res[0][2]["channels_tiled"] == C, res[0][2]
    for k, lines in enumerate(res[1][1]):
        _tiled_check(lines, k)
    monkeypatch.setenv("PSK_SOFT_STAMP", "0")
    h = pl.Handle(C, device=0)
    try:
        unstamped = run(h, None)
    finally:
        h.close()
    assert unstamped[2]["channels_tiled"] == C, unstamped[2]
    assert_same(res[0][0], unstamped[0], "PSK_SOFT_STAMP=0")
    check_parity(oracle_mod, res[0][0], lambda c: props, data, "uniform CS16 batch")


# ---- 6. pipelined ranges ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,M,diff,n_ph", [(8, 4, 1, 50), (4, 2, 0, 200)])
def test_pipelined_ranges_with_cs16(oracle_mod, monkeypatch, capfd, S, M, diff, n_ph):
    """PSK_SOFT_PIPELINED=2 (front / fit / back of ranges of three tiles on three streams): channels of ragged lengths whose
    packets alternate CS16 / CF32 from call to call (the CS16 ones converted by the pre-pass, whose scratch the two pipeline
    streams read), differential decoding, a noisy channel that is handed over, three calls."""
    C, calls = 7, 3
    lens = [40000, 40000, 1000 * S, 23456, 40000, 17 * 128 * S + 5 * S, 40000]
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=n_ph, differentialDecoding=diff)
    from psk_soft_amd.stimulus import synth_channel

    iqs = [q16(synth_channel(57000 + 7 * S + c, M, S, calls * lens[c], sigma=(0.35 if c == 4 else 0.01))) for c in range(C)]
    data = [[iqs[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]] if (c + k) % 2 == 0
             else iqs[c][2 * k * lens[c] : 2 * (k + 1) * lens[c]].astype(np.float32) for c in range(C)] for k in range(calls)]

    def run(h, cf):
        h.configure(0, [props] * C)
        tiled = []

        def before(hh, k):
            if k:
                st = hh.stats()
                assert st["channels_sequential"] == 0 and st["channels_parallel_fit"] == 0, st
                tiled.append(st["channels_tiled"])
        got, traces, _ = device_run(h, data, cf, before=before)
        before(h, calls)
        return got, traces, tiled

    res = untraced_then_traced(monkeypatch, capfd, dict(PSK_SOFT_PIPELINED=2, PSK_SOFT_TIME_TILED=2), C, run)
    assert all(t >= C - 1 for t in res[0][2]), res[0][2]  # (the noisy channel may be handed over)
    for k, lines in enumerate(res[1][1]):
        w = whats(lines)
        assert "cs16_convert" in w and "tile_front" not in w, (k, w)
        assert sum(t["what"] == "pipe_front" and t["H"] == 1 for t in lines) >= 2, (k, lines)
        assert not any(t["H"] == H_CS16 for t in lines), (k, lines)
    check_parity(oracle_mod, res[0][0], lambda c: props, data, "pipelined S%d" % S)


# ---- 7. the conversion scratch taken over across caller streams --------------------------------------------------------

_SCR = dict(S=8, M=4, A=400, C=48, groups=6, calls=12, n=12000, big=9, n_big=48000)


def _scratch_child(path, trace):
    """(a fresh process: torch initialises HIP first) twelve process_device calls on six torch streams in turn, no host wait;
    call k on stream k % 6 for the channels of group k % 6, CS16 at numAvg 400 (the pre-pass: four conversion buffers for six
    streams).  Call 9 is larger than any before it.  Saves inputs and outputs."""
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    p = _SCR
    S, C, G, K = p["S"], p["C"], p["groups"], p["calls"]
    per = C // G
    lens = [p["n_big"] if k == p["big"] else p["n"] + 8 * S * k for k in range(K)]
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(G)]
    host = [q16(synth_channel(58000 + c, p["M"], S, sum(lens))) for c in range(C)]
    pos = [0] * G
    save = {}
    ins, outs = [], []
    for k in range(K):
        gi = k % G
        n = lens[k]
        x = np.stack([host[gi * per + j][2 * pos[gi] : 2 * (pos[gi] + n)] for j in range(per)])
        pos[gi] += n
        save["in_%d" % k] = x
        cap = n // S + 2
        ins.append(torch.from_numpy(x).to(dev))
        outs.append(dict(soft=torch.empty((per, 2 * cap), dtype=torch.float32, device=dev),
                         phase=torch.empty((per, cap), dtype=torch.float32, device=dev),
                         index=torch.empty((per, cap), dtype=torch.int16, device=dev),
                         bits=torch.empty((per, 2 * cap), dtype=torch.int16, device=dev), cap=cap))
    torch.cuda.synchronize()
    if trace:
        os.environ["PSK_SOFT_TRACE_LAUNCHES"] = "2"
    h = pl.Handle(C, device=0)
    h.configure_all(samplesPerBaud=S, constelationSize=p["M"], numAvg=p["A"], phaseAvg=50)
    first = [True] * G
    res = []
    for k in range(K):
        gi, o = k % G, outs[k]
        pk, out = (pl.Packet * per)(), (pl.Output * per)()
        for j in range(per):
            pk[j].data, pk[j].n_floats, pk[j].sri_xdelta, pk[j].sri_mode = ins[k][j].data_ptr(), ins[k].shape[1], 0.01, 1
            pk[j].sriChanged, pk[j].present, pk[j].format = int(first[gi]), 1, pl.FORMAT_CS16
            out[j].soft, out[j].phase = o["soft"][j].data_ptr(), o["phase"][j].data_ptr()
            out[j].sampleIndex, out[j].bits, out[j].cap_symbols = o["index"][j].data_ptr(), o["bits"][j].data_ptr(), o["cap"]
        first[gi] = False
        h.process_device(gi * per, pk, out, streams[gi].cuda_stream)
        res.append(out)
    torch.cuda.synchronize()
    h.synchronize()
    st = h.stats()
    assert st["channels_sequential"] == 0, st
    for k in range(K):
        for j in range(per):
            ns = int(res[k][j].n_symbols)
            for key in ("soft", "phase", "index", "bits"):
                m = {"soft": 2 * ns, "bits": int(res[k][j].n_bits)}.get(key, ns)
                save["%s_%d_%d" % (key, k, j)] = outs[k][key][j, :m].cpu().numpy()
    h.close()
    np.savez(path, **save)


def test_conversion_scratch_taken_over_across_caller_streams(oracle_mod, tmp_path):
    """Twelve process_device calls rotating over six torch streams without a host wait, each with CS16 channels that the
    pre-pass converts: the library keeps four conversion buffers, so streams take buffers over from one another and must wait
    for their last use; call 9, larger than any before, grows a buffer while others are in flight.  Every call against the
    oracle; a traced run (in a second child) gives the same outputs and shows the pre-pass on six streams."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [str(tmp_path / ("scratch_%d.npz" % t)) for t in (0, 1)]
    errs = []
    for t in (0, 1):
        r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_cs16_schedules as t; t._scratch_child(%r, %d)" % (paths[t], t)],
                           cwd=root, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        errs.append(r.stderr.decode())
    lines = parse_trace(errs[1])
    conv = [t for t in lines if t["what"] == "cs16_convert"]
    assert len(conv) == _SCR["calls"] and len({t["stream"] for t in conv}) == _SCR["groups"], conv
    d0, d1 = np.load(paths[0]), np.load(paths[1])
    for key in d0.files:
        assert np.array_equal(d0[key].view(np.uint8), d1[key].view(np.uint8)), "traced run: %s differs" % key
    p = _SCR
    per = p["C"] // p["groups"]
    props = dict(samplesPerBaud=p["S"], constelationSize=p["M"], numAvg=p["A"], phaseAvg=50)
    for gi in range(p["groups"]):
        ks = [k for k in range(p["calls"]) if k % p["groups"] == gi]
        for j in sorted({0, per - 1}):
            ref, _ = oracle_calls(oracle_mod, props, [d0["in_%d" % k][j] for k in ks])
            for k, r in zip(ks, ref):
                got = {key: d0["%s_%d_%d" % (key, k, j)] for key in KEYS}
                assert_parity(got, r, "stream %d, call %d, channel %d" % (gi, k, gi * per + j))
