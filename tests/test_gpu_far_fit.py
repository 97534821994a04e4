"""PSK_SOFT_OPT_FAR_FIT on a real MI355X: phaseAvg 32641 .. 65535 on the time-tiled kernels, the fit window in a ring in device
memory (psk_farfit.hip), bit for bit (uint32 patterns) against the oracle, call by call."""
import ctypes

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from psk_soft_amd.stimulus import synth_channel
from tests.test_gpu_parity import _handle, assert_parity
from tests.test_gpu_wide_symbols import KEYS, cuts_of, psk_signal, run_both

pytestmark = pytest.mark.gpu

OPT_FAR_FIT = 7
OPT_QUALITY = 6


def _far_handle(n=1, window=16384, opt=1):
    h = _handle(n, max_window_samples=window, max_phase_avg=65535, max_packet_complex=1 << 21)
    h.set_option(OPT_FAR_FIT, opt)  # (without the feature: refused here)
    return h


def _cuts_by_symbols(S, A, sym_counts, tail):
    """call boundaries in complex samples: call k emits sym_counts[k] symbols, the last call brings `tail` samples (< S)"""
    ends, total = [], 0
    for k, ns in enumerate(sym_counts):
        total += S * (ns + (A - 1 if k == 0 else 0))
        ends.append(total)
    ends.append(total + tail)
    return list(zip([0] + ends[:-1], ends))


# ---- 1. the window filling, becoming steady in the middle of a block, steady; a call shorter than a block; one that emits nothing

@pytest.mark.parametrize("S,M,n,diff", [(2, 2, 32641, 0), (2, 4, 32768, 1), (2, 8, 65535, 0), (8, 4, 40000, 0)])
def test_filling_crossing_steady(oracle_mod, S, M, n, diff):
    A = 10
    c0 = int(0.6 * n) | 1
    while (n - c0) % 128 == 0:  # (the window becomes steady in the middle of a block of call 2)
        c0 += 2
    counts = [c0, c0, int(1.1 * n) | 1, 100]  # (odd or 100: no multiple of 128)
    assert all(c % 128 for c in counts) and counts[0] < n < counts[0] + counts[1] and (n - counts[0]) % 128
    cuts = _cuts_by_symbols(S, A, counts, S - 1)
    data = synth_channel(4100 + S + M, M, S, cuts[-1][1])
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n, differentialDecoding=diff)
    h = _far_handle()
    stats = run_both(oracle_mod, h, [(props, data, cuts)])
    for k, st in enumerate(stats[:4]):
        assert st["channels_fast"] == 1 and st["channels_sequential"] == 0 and st["channels_guard"] == 0, (k, st)
        assert st["channels_tiled"] == 1, (k, st)
    assert stats[4]["channels_sequential"] == 0, stats[4]
    h.close()


# ---- 2. the end-of-call wrap over a far window

def test_end_of_call_wrap(oracle_mod):
    S, M, n, A, ns = 2, 2, 40000, 10, 30000
    cuts = _cuts_by_symbols(S, A, [ns] * 4, 0)[:4]
    data = synth_channel(4200, M, S, cuts[-1][1], cfo=2e-3)
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n)
    # the oracle first: the estimate passes 2 pi M inside every call, so the wrap fires at the end of the calls
    o = oracle_mod.OracleComponent()
    for k, v in props.items():
        setattr(o, k, v)
    ph = [o.service(data[2 * a : 2 * b], 0.01, sriChanged=(k == 0)).phase for k, (a, b) in enumerate(cuts)]
    wrap, fired = 2 * np.pi * M, 0
    for k in range(3):
        drop = float(ph[k][-1]) - float(ph[k + 1][0])
        turns = round(drop / wrap)
        if turns >= 1 and abs(drop - turns * wrap) < 0.5:
            fired += 1
    assert fired >= 2, [(float(p[0]), float(p[-1])) for p in ph]
    h = _far_handle()
    stats = run_both(oracle_mod, h, [(props, data, cuts)])
    assert all(st["channels_fast"] == 1 and st["channels_sequential"] == 0 for st in stats), stats
    h.close()


# ---- 3. a mixed batch

def _mixed_batch():
    rng = np.random.default_rng(43)
    cfg = [(8, 100, 50), (10, 64, 200), (8, 25, 3000),                                      # ordinary and deep windows
           (8, 10, 32641), (40, 5, 50000), (1, 0, 65535), (2048, 2, 32641), (8, 10, 65535), (40, 3, 50000), (8, 100, 50000)]
    chans = []
    for c, (S, A, n) in enumerate(cfg):
        M = (2, 4, 8)[c % 3]
        n_sym = {1: 70000, 2048: 90}.get(S, 36000 if n > 32640 else 9000)
        data = psk_signal(rng, S, n_sym + A, M) if S != 1 else synth_channel(4300, M, 1, n_sym)
        props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n, differentialDecoding=int(c == 4))
        chans.append((props, data, cuts_of(rng, data.size // 2, 3)))
    return chans, sum(1 for _, _, n in cfg if n > 32640)


def test_mixed_batch(oracle_mod):
    chans, n_far = _mixed_batch()
    outs = []
    for opt in (1, 0):
        h = _far_handle(len(chans), window=4 * 2048, opt=opt)
        h.configure(0, [p for p, _, _ in chans])
        per_call = []
        for call in range(3):
            pk = [dict(data=d[2 * cuts[call][0] : 2 * cuts[call][1]], xdelta=0.01, sriChanged=(call == 0)) for _, d, cuts in chans]
            got = h.process_host(0, pk)
            st = h.stats()
            emitting_far = sum(1 for c, (p, _, _) in enumerate(chans) if p["phaseAvg"] > 32640 and got[c]["phase"].size)
            if opt:
                assert st["channels_sequential"] - st["channels_guard"] == 0, (call, st)
            else:
                assert st["channels_sequential"] == emitting_far, (call, st)
            per_call.append([{k: got[c][k].copy() for k in KEYS} for c in range(len(chans))])
        outs.append(per_call)
        h.close()
    assert sum(1 for p, _, _ in chans if p["phaseAvg"] > 32640) == n_far
    for call in range(3):
        for c in range(len(chans)):
            for k in KEYS:
                assert outs[0][call][c][k].tobytes() == outs[1][call][c][k].tobytes(), (call, c, k)
    # ... and every channel against the oracle
    for c, (props, data, cuts) in enumerate(chans):
        o = oracle_mod.OracleComponent()
        for k, v in props.items():
            setattr(o, k, v)
        for call, (a, b) in enumerate(cuts):
            r = o.service(data[2 * a : 2 * b], 0.01, sriChanged=(call == 0))
            assert_parity(outs[0][call][c], dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index), "channel %d call %d %s" % (c, call, props))


# ---- 4. changing paths mid-stream

def test_changing_paths_mid_stream(oracle_mod):
    S, M, A, n = 2, 4, 10, 65535
    steps = [("opt", 1), ("opt", 0), ("opt", 1), ("cfg", dict(phaseAvg=33000)), ("cfg", dict(phaseAvg=50)), ("cfg", dict(phaseAvg=65535)),
             ("cfg", dict(resetState=1)), (None, None)]
    lens = [40001, 30003, 20005, 9001, 9003, 40001, 9005, 30001]
    data = synth_channel(4400, M, S, S * (sum(lens) + A))
    h = _far_handle()
    o = oracle_mod.OracleComponent()
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n)
    h.configure(0, [props])
    for k, v in props.items():
        setattr(o, k, v)
    pos = 0
    far_fast = 0
    for call, ((what, arg), ns) in enumerate(zip(steps, lens)):
        if what == "opt":
            h.set_option(OPT_FAR_FIT, arg)
        elif what == "cfg":
            props = dict(props, **arg)
            h.configure(0, [props])
            for k, v in arg.items():
                setattr(o, k, v)
            props.pop("resetState", None)
        cnt = S * (ns + (A - 1 if call == 0 else 0))
        seg = data[2 * pos : 2 * (pos + cnt)]
        pos += cnt
        got = h.process_host(0, [dict(data=seg, xdelta=0.01, sriChanged=(call == 0))])[0]
        r = o.service(seg, 0.01, sriChanged=(call == 0))
        assert_parity({k: got[k] for k in KEYS}, dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index), "call %d (%s %s)" % (call, what, arg))
        st = h.stats()
        if call == 1:
            assert st["channels_sequential"] == 1, st
        else:
            assert st["channels_fast"] == 1 and st["channels_sequential"] == 0, (call, st)
            far_fast += props["phaseAvg"] > 32640
    assert far_fast == 6
    h.close()


# ---- 5. hand-over

def test_non_finite_samples_are_handed_over(oracle_mod):
    S, M, A, n = 2, 4, 10, 40000
    cuts = _cuts_by_symbols(S, A, [25001, 25003, 25005, 25007], 0)[:4]
    data = synth_channel(4500, M, S, cuts[-1][1]).copy()
    data[2 * (cuts[1][0] + 20001)] = np.nan
    data[2 * (cuts[2][0] + 777) + 1] = np.inf
    h = _far_handle()
    stats = run_both(oracle_mod, h, [(dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n), data, cuts)])
    assert all(st["channels_sequential"] == st["channels_guard"] for st in stats), stats
    assert stats[0]["channels_fast"] == 1 and stats[1]["channels_guard"] == 1 and stats[2]["channels_guard"] == 1, stats
    h.close()


# ---- 6. formats and strides

def test_formats_and_strides_give_the_same_bytes(oracle_mod):
    from tests.test_gpu_cs8 import q8
    from tests.test_gpu_strided import strided_run

    S, M, A, n, ns = 2, 4, 10, 32641, 40000
    cuts = _cuts_by_symbols(S, A, [ns, ns], 0)[:2]
    base = q8(synth_channel(4600, M, S, cuts[-1][1]))  # (int8 values: every format holds them exactly)
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n)
    outs = {}
    for name, dt in (("cf32", np.float32), ("cs16", np.int16), ("cs8", np.int8), ("cf16", np.float16)):
        h = _far_handle()
        h.configure(0, [props])
        outs[name] = []
        for k, (a, b) in enumerate(cuts):
            got = h.process_host(0, [dict(data=base[2 * a : 2 * b].astype(dt), xdelta=0.01, sriChanged=(k == 0))])[0]
            outs[name].append({key: got[key].copy() for key in KEYS})
            st = h.stats()
            assert st["channels_fast"] == 1 and st["channels_sequential"] == 0, (name, k, st)
        h.close()
    h = _far_handle()
    h.configure(0, [props])
    calls = [[base[2 * a : 2 * b]] for a, b in cuts]
    got, _, _ = strided_run(h, calls, [(0, 3)], {0: 7})
    st = h.stats()
    assert st["channels_fast"] == 1 and st["channels_sequential"] == 0, st
    outs["strided"] = got[0]
    h.close()
    for name in ("cs16", "cs8", "cf16", "strided"):
        for k in range(2):
            for key in KEYS:
                assert outs[name][k][key].tobytes() == outs["cf32"][k][key].tobytes(), (name, k, key)
    o = oracle_mod.OracleComponent()
    for k, v in props.items():
        setattr(o, k, v)
    for k, (a, b) in enumerate(cuts):
        r = o.service(base[2 * a : 2 * b].astype(np.float32), 0.01, sriChanged=(k == 0))
        assert_parity(outs["cf32"][k], dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index), "call %d" % k)


# ---- 7. quality records

def test_quality_records_equal_those_of_the_reference_order_path(oracle_mod):
    S, M, A, n = 8, 4, 10, 40000
    cuts = _cuts_by_symbols(S, A, [30001, 20003], 0)[:2]
    data = synth_channel(4700, M, S, cuts[-1][1])
    recs = []
    for opt in (1, 0):
        h = _far_handle(opt=opt)
        h.set_option(OPT_QUALITY, 1)
        h.configure(0, [dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n)])
        mine = []
        for k, (a, b) in enumerate(cuts):
            h.process_host(0, [dict(data=data[2 * a : 2 * b], xdelta=0.01, sriChanged=(k == 0))])
            mine.append(bytes(h.quality_records()[0]))
            st = h.stats()
            assert st["channels_fast"] == opt and st["channels_sequential"] == 1 - opt, (opt, k, st)
        recs.append(mine)
        h.close()
    assert recs[0] == recs[1]


# ---- 8. the scratch across calls and streams

def _device_calls(h, L, plan):
    """plan: list of (ch0, [segments of the channels from ch0], stream, first); all inputs uploaded first, the calls issued back to
    back without a host wait; returns per call the per-channel output dicts"""
    al = lambda v: (v + 127) // 128 * 128  # noqa: E731
    bufs, jobs = [], []
    for ch0, segs, stream, first in plan:
        C = len(segs)
        pk, out = (pl.Packet * C)(), (pl.Output * C)()
        rows = []
        for j, seg in enumerate(segs):
            cap = h.output_capacity(ch0 + j, seg.size // 2)
            d_in = h.device_alloc(al(seg.nbytes))
            h.upload(d_in, seg)
            d = [h.device_alloc(al(b * cap)) for b in (8, 4, 6, 2)]
            bufs += [d_in] + d
            pk[j].data, pk[j].n_floats, pk[j].sri_xdelta, pk[j].sri_mode = d_in, seg.size, 0.01, 1
            pk[j].sriChanged, pk[j].present, pk[j].format = int(first), 1, pl.FORMAT_CF32
            out[j].soft, out[j].phase, out[j].bits, out[j].sampleIndex, out[j].cap_symbols = d[0], d[1], d[2], d[3], cap
            rows.append(d)
        jobs.append((ch0, pk, out, rows, stream))
    h.synchronize()
    for ch0, pk, out, rows, stream in jobs:
        h.process_device(ch0, pk, out, stream)
    for s in {j[4] for j in jobs if j[4]}:
        assert L.hipStreamSynchronize(ctypes.c_void_p(s)) == 0
    h.synchronize()
    res = []
    for ch0, pk, out, rows, stream in jobs:
        per = []
        for j, d in enumerate(rows):
            ns = int(out[j].n_symbols)
            per.append(dict(soft=h.download(d[0], (2 * ns,), np.float32), phase=h.download(d[1], (ns,), np.float32),
                            bits=h.download(d[2], (int(out[j].n_bits),), np.int16), index=h.download(d[3], (ns,), np.int16)))
        res.append(per)
    for b in bufs:
        h.device_free(b)
    return res


def test_scratch_across_calls_and_streams(oracle_mod):
    """Two calls in a row on one stream without a host wait between them (the second reads the rows the first leaves), then two
    disjoint channel ranges, each holding a far channel, on two streams at once: the rows belong to channels, not to calls."""
    L = pl.load()
    S, A = 8, 10
    props = [dict(samplesPerBaud=S, constelationSize=4, numAvg=A, phaseAvg=40000), dict(samplesPerBaud=S, constelationSize=4, numAvg=A, phaseAvg=50),
             dict(samplesPerBaud=S, constelationSize=2, numAvg=A, phaseAvg=200), dict(samplesPerBaud=S, constelationSize=8, numAvg=A, phaseAvg=65535)]
    cuts = _cuts_by_symbols(S, A, [30001, 15003, 20005], 0)[:3]
    data = [synth_channel(4800 + c, p["constelationSize"], S, cuts[-1][1]) for c, p in enumerate(props)]
    seg = lambda c, k: data[c][2 * cuts[k][0] : 2 * cuts[k][1]]  # noqa: E731
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        assert L.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0  # (non-blocking)
    h = _far_handle(4)
    try:
        h.configure(0, props)
        a = _device_calls(h, L, [(0, [seg(c, 0) for c in range(4)], streams[0].value, True),
                                 (0, [seg(c, 1) for c in range(4)], streams[0].value, False)])
        b = _device_calls(h, L, [(0, [seg(0, 2), seg(1, 2)], streams[0].value, False), (2, [seg(2, 2), seg(3, 2)], streams[1].value, False)])
        st = h.stats()
        assert st["channels_sequential"] == 0 and st["channels_fast"] == 4, st
        got = {c: [a[0][c], a[1][c], b[c // 2][c % 2]] for c in range(4)}
        for c in range(4):
            o = oracle_mod.OracleComponent()
            for k, v in props[c].items():
                setattr(o, k, v)
            for k in range(3):
                r = o.service(seg(c, k), 0.01, sriChanged=(k == 0))
                assert_parity(got[c][k], dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index), "channel %d call %d" % (c, k))
    finally:
        h.close()
        for s in streams:
            L.hipStreamDestroy(s)
