"""PSK_SOFT_OPT_QUALITY on the GPU: the reduction pass behind a call (psk_quality.hip) and its records.

Every case runs its calls three times on fresh handles under PSK_SOFT_TRACE_LAUNCHES=2 -- option off, on, on again:
  * the four output streams are byte-identical between off and on, and bit for bit the oracle's, as in the other suites;
  * the launch lines of the off run hold no quality_*; those of the on run are, compared by (what, S, H, cnt), the off run's
    plus exactly one quality_fold and one quality_join per psk_soft_process_device call, last;
  * every checked record equals the model (tests/quality_model.py) applied to the rows downloaded from the device: counts,
    copied values, snapshot and flags equal, the four sums within n * 2^-53 * sum|t_i| of the exact sum;
  * the second on-handle gives byte-identical records."""

import math
from collections import namedtuple

import numpy as np
import pytest

from tests import quality_model as qm
from tests.test_gpu_cs16_schedules import KEYS, _mixed_cut_batch, _synth, assert_same, check_parity, parse_trace
from tests.test_gpu_cs8 import q8

pytestmark = pytest.mark.gpu

Run = namedtuple("Run", "got traces recs nsym")
STREAM_OF = dict(soft="soft", phase="phase", bits="bits", index="sampleIndex")


def _fmt(x):
    from psk_soft_amd import lib as pl

    return {np.dtype(np.int8): pl.FORMAT_CS8, np.dtype(np.int16): pl.FORMAT_CS16}.get(x.dtype, pl.FORMAT_CF32)


def device_calls(h, calls, check=None, capfd=None, quality=False, nulls=None, skew=(), k0=0, sync_each=True, streams=None, spans=None):
    """psk_soft_process_device, one call per calls[k] (calls[k][c]: interleaved I/Q of channel c -- int8, int16 or float32 -- or
    None: no packet), device-resident packets, every (call, channel) with rows of its own on 128-byte boundaries (channels in
    `skew`: 8 bytes further on for soft, 4 for the others -- the alignment the ABI asks for and no more).  nulls: {channel:
    streams handed over as null pointers}.  After every call the host waits and, with `quality`, reads all records.
    sync_each=False: the calls are issued back to back, the host waits once behind the last and reads the records once.
    streams[k]: the raw hipStream_t of call k (None: the handle's own).  spans[k] = (ch0, nch): the channels call k covers
    (default: all of them; calls[k][c] is None outside).
    Returns Run(got = {c: [dict of the four rows, or None without a packet]}, traces[k], recs[k][c] as bytes, nsym[k][c])."""
    from psk_soft_amd import lib as pl

    K, C = len(calls), len(calls[0])
    check = list(range(C)) if check is None else list(check)
    nulls = nulls or {}
    al = lambda n: (n + 127) // 128 * 128 + 128  # noqa: E731
    lay, tot = {}, [0, 0, 0, 0, 0]
    for k in range(K):
        for c in range(C):
            x = calls[k][c]
            if x is None:
                continue
            cap = h.output_capacity(c, x.size // 2)
            lay[k, c] = (cap, tuple(tot))
            for i, s in enumerate((x.nbytes, 8 * cap, 4 * cap, 6 * cap, 2 * cap)):
                tot[i] += al(s)
    d_in = h.device_alloc(max(tot[0], 128))
    bufs = [h.device_alloc(max(t, 128)) for t in tot[1:]]
    d_soft, d_phase, d_bits, d_sidx = bufs
    traces, nsym, outs, recs = [], [], [], []
    try:
        for (k, c), (cap, o) in lay.items():
            h.upload(d_in + o[0], calls[k][c])
        h.synchronize()
        for k in range(K):
            lo, n = spans[k] if spans else (0, C)
            assert all(calls[k][c] is None for c in range(C) if not lo <= c < lo + n)
            pk, out = (pl.Packet * n)(), (pl.Output * n)()
            for c in range(lo, lo + n):
                x = calls[k][c]
                if x is None:
                    continue
                cap, o = lay[k, c]
                s8, s4 = (8, 4) if c in skew else (0, 0)
                p, q = pk[c - lo], out[c - lo]
                p.data, p.n_floats, p.sri_xdelta, p.sri_mode = d_in + o[0], x.size, 0.01, 1
                p.sriChanged, p.present, p.format = int(k + k0 == 0), 1, _fmt(x)
                q.soft, q.phase, q.bits, q.sampleIndex = d_soft + o[1] + s8, d_phase + o[2] + s4, d_bits + o[3] + s4, d_sidx + o[4] + s4
                for name in nulls.get(c, ()):
                    setattr(q, STREAM_OF[name], None)
                q.cap_symbols = cap
            if capfd:
                capfd.readouterr()
            h.process_device(lo, pk, out, streams[k] if streams else None)
            if capfd:
                traces.append(parse_trace(capfd.readouterr().err))
            if sync_each:
                h.synchronize()
                if quality:
                    recs.append([bytes(q) for q in h.quality_records()])
            outs.append({c: out[c - lo] for c in range(lo, lo + n)})
            nsym.append([int(out[c - lo].n_symbols) if lo <= c < lo + n else 0 for c in range(C)])
        if not sync_each:
            h.synchronize()
            if quality:
                recs.append([bytes(q) for q in h.quality_records()])
        got = {c: [] for c in check}

        def fetch(ptr, n, dt):
            if not ptr:
                return None
            return h.download(ptr, (n,), dt) if n else np.zeros(0, dt)

        for c in check:
            for k in range(K):
                if calls[k][c] is None:
                    got[c].append(None)
                    continue
                o = outs[k][c]
                ns = int(o.n_symbols)
                got[c].append(dict(soft=fetch(o.soft, 2 * ns, np.float32), phase=fetch(o.phase, ns, np.float32),
                                   bits=fetch(o.bits, int(o.n_bits), np.int16), index=fetch(o.sampleIndex, int(o.n_sampleIndex), np.int16)))
    finally:
        for b in [d_in] + bufs:
            h.device_free(b)
    return Run(got, traces, recs, nsym)


def three_runs(monkeypatch, capfd, env, n_ch, body, **limits):
    """body(handle, capfd, quality) -> Run on three fresh handles under `env` and the launch trace: option off, on, on"""
    from psk_soft_amd import lib as pl

    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    runs = []
    for quality in (False, True, True):
        h = pl.Handle(n_ch, device=0, **limits)
        try:
            if quality:
                h.set_option(pl.Handle.OPT_QUALITY, 1)
                assert all(bytes(q) == bytes(88) for q in h.quality_records())
            capfd.readouterr()
            runs.append(body(h, capfd, quality))
        finally:
            h.close()
    return runs


def _key(t):
    return (t["what"], t["S"], t["H"], t["cnt"])


def check_traces(off, on, n_ch, ctx, device_calls_per_call=1, pair_only=False):
    """the launch lines of one public call, option off and on"""
    assert off and not any(t["what"].startswith("quality_") for t in off), (ctx, off)
    rest = [_key(t) for t in on if not t["what"].startswith("quality_")]
    if not pair_only:
        assert rest == [_key(t) for t in off], (ctx, rest, [_key(t) for t in off])
    fold = [i for i, t in enumerate(on) if t["what"] == "quality_fold"]
    join = [i for i, t in enumerate(on) if t["what"] == "quality_join"]
    assert len(fold) + len(join) == len(on) - len(rest), ctx
    assert fold and [i + 1 for i in fold] == join and join[-1] == len(on) - 1, (ctx, fold, join, len(on))
    for i in fold + join:
        assert on[i]["S"] == 0 and on[i]["H"] == 0, (ctx, on[i])
    if device_calls_per_call == 1:
        assert len(fold) == 1 and on[fold[0]]["cnt"] == on[join[0]]["cnt"] == n_ch, (ctx, on[-2:])
    else:  # (psk_soft_process_host: one psk_soft_process_device call per chunk of channels)
        assert len(fold) == device_calls_per_call, (ctx, len(fold))
        assert sum(on[i]["cnt"] for i in fold) == sum(on[i]["cnt"] for i in join) == n_ch, ctx


def model_of(g, p):
    return qm.model_record(g["soft"], g["phase"], g["index"], p["constelationSize"], p["samplesPerBaud"], p.get("differentialDecoding", 0))


def check_records(run, props_of, ctx):
    """every checked channel's record of every call against the model on the rows the call wrote"""
    from psk_soft_amd import lib as pl

    for c, per_call in run.got.items():
        for k, g in enumerate(per_call):
            q = pl.Quality.from_buffer_copy(run.recs[k][c])
            if g is None:
                assert run.recs[k][c] == bytes(88), "%s: channel %d call %d had no packet, its record is not zero" % (ctx, c, k)
                continue
            qm.assert_record(q, model_of(g, props_of(c)), "%s, channel %d call %d" % (ctx, c, k))
            if run.nsym[k][c] == 0:
                assert run.recs[k][c] == bytes(88), (ctx, c, k)


def check_case(oracle_mod, runs, props_of, calls, n_ch, ctx, parity=True, pair_only=False):
    off, on, on2 = runs
    assert_same(off.got, on.got, ctx + ": option on against off")
    if parity:
        check_parity(oracle_mod, on.got, props_of, calls, ctx)
    for k in range(len(calls)):
        check_traces(off.traces[k], on.traces[k], n_ch, "%s call %d" % (ctx, k), pair_only=pair_only)
    check_records(on, props_of, ctx)
    assert on.recs == on2.recs, ctx + ": a second handle gives other bytes"
    assert on.nsym == off.nsym == on2.nsym


# ---- 1. every constellation, differential decoding off and on --------------------------------------------------------------

def test_records_of_every_constellation(oracle_mod, monkeypatch, capfd):
    """M 2 / 4 / 8 x differential off / on, samplesPerBaud 8, numAvg 100: cold start, steady, a one-sample call that emits
    nothing.  The first symbol of a differentially decoded stream is not finite and is left out: n_finite = n - 1.  Odd
    channels have rows at the ABI's alignment only (the 8-byte loads of the fold)."""
    from psk_soft_amd import lib as pl

    S = 8
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50, differentialDecoding=d) for M in (2, 4, 8) for d in (0, 1)]
    C = len(props)
    lens = [9000, 12001, 1]
    host = _synth(61000, [p["constelationSize"] for p in props], S, sum(lens))
    cuts = np.cumsum([0] + lens)
    calls = [[host[c][2 * cuts[k]:2 * cuts[k + 1]] for c in range(C)] for k in range(3)]
    runs = three_runs(monkeypatch, capfd, {}, C,
                      lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, None, cf, q, skew=(1, 3, 5)))[1])
    check_case(oracle_mod, runs, lambda c: props[c], calls, C, "constellations")
    on = runs[1]
    assert all(n > 1000 for n in on.nsym[0] + on.nsym[1]) and on.nsym[2] == [0] * C
    for c in range(C):
        q0, q1, q2 = (pl.Quality.from_buffer_copy(on.recs[k][c]) for k in range(3))
        assert q0.flags == q1.flags == 15 and q2.flags == 0 and q2.n_symbols == 0
        assert q0.n_finite == q0.n_symbols - props[c]["differentialDecoding"], (c, q0.n_finite, q0.n_symbols)
        assert q1.n_finite == q1.n_symbols == q1.n_lock
        assert pl.quality_derive(q1)["lock"] > 0.9


# ---- 2. the three packet formats -------------------------------------------------------------------------------------------

def test_three_formats_one_record(oracle_mod, monkeypatch, capfd):
    """CF32, CS16 and CS8 packets of the same quantised stimulus: three identical records, call by call."""
    S, M = 8, 4
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)] * 3
    lens = [8000, 8003]
    x8 = q8(_synth(62000, [M], S, sum(lens))[0])
    calls = [[x8[2 * a:2 * b].astype(np.float32), x8[2 * a:2 * b].astype(np.int16), x8[2 * a:2 * b]] for a, b in ((0, lens[0]), (lens[0], sum(lens)))]
    runs = three_runs(monkeypatch, capfd, {}, 3, lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, None, cf, q))[1])
    check_case(oracle_mod, runs, lambda c: props[c], calls, 3, "formats")
    for k in range(2):
        assert runs[1].recs[k][0] == runs[1].recs[k][1] == runs[1].recs[k][2] != bytes(88), k


# ---- 3. the flags ----------------------------------------------------------------------------------------------------------

def test_flags_and_zeros_where_a_flag_is_off(oracle_mod, monkeypatch, capfd):
    """samplesPerBaud 1 (no sampleIndex stream), constelationSize 16 (no lock sums), a null phase, sampleIndex and soft
    pointer: the flags, and zeros where a flag is off.  (Short calls of few channels: the wave-scan and reference-order
    kernels, which take null pointers.)"""
    from psk_soft_amd import lib as pl

    base = dict(samplesPerBaud=8, constelationSize=4, numAvg=100, phaseAvg=50)
    props = [dict(base, samplesPerBaud=1, numAvg=0), dict(base, constelationSize=16), dict(base), dict(base), dict(base, differentialDecoding=1), dict(base)]
    nulls = {2: ("phase",), 3: ("index",), 4: ("soft",)}
    C = len(props)
    host = [_synth(63000 + c, [4], props[c]["samplesPerBaud"], 1500 * props[c]["samplesPerBaud"] * 2 + 13)[0] for c in range(C)]
    calls = [[host[c][:host[c].size // 2 // 2 * 2] for c in range(C)], [host[c][host[c].size // 2 // 2 * 2:] for c in range(C)]]
    runs = three_runs(monkeypatch, capfd, dict(PSK_SOFT_TIME_TILED=0), C,
                      lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, None, cf, q, nulls=nulls))[1])
    off, on, on2 = runs
    # the streams that were asked for: off == on == the oracle
    from tests.test_gpu_cs16_schedules import oracle_calls
    for c in range(C):
        ref, _ = oracle_calls(oracle_mod, props[c], [calls[k][c] for k in range(2)])
        for k in range(2):
            for key in KEYS:
                a, b = off.got[c][k][key], on.got[c][k][key]
                if key in nulls.get(c, ()):
                    assert a is None and b is None
                    continue
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (c, k, key)
                r = np.ascontiguousarray(ref[k][key], a.dtype)
                assert np.array_equal(a.view(np.uint8), r.view(np.uint8)), (c, k, key)
    for k in range(2):
        check_traces(off.traces[k], on.traces[k], C, "flags call %d" % k)
    check_records(on, lambda c: props[c], "flags")
    assert on.recs == on2.recs
    want = {0: pl.Q_SOFT | pl.Q_PHASE | pl.Q_LOCK, 1: pl.Q_SOFT | pl.Q_PHASE | pl.Q_INDEX, 2: pl.Q_SOFT | pl.Q_INDEX | pl.Q_LOCK,
            3: pl.Q_SOFT | pl.Q_PHASE | pl.Q_LOCK, 4: pl.Q_PHASE | pl.Q_INDEX, 5: 15}
    for k in range(2):
        for c in range(C):
            q = pl.Quality.from_buffer_copy(on.recs[k][c])
            assert q.flags == want[c] and q.n_symbols == on.nsym[k][c] > 100, (k, c, q.flags)
            if not q.flags & pl.Q_SOFT:
                assert (q.n_finite, q.n_lock, q.sum_e, q.sum_e2, q.sum_lock_re, q.sum_lock_im) == (0, 0, 0.0, 0.0, 0.0, 0.0)
            if not q.flags & pl.Q_LOCK:
                assert (q.n_lock, q.sum_lock_re, q.sum_lock_im) == (0, 0.0, 0.0)
            if not q.flags & pl.Q_PHASE:
                assert (q.phase_first, q.phase_last) == (0.0, 0.0)
            if not q.flags & pl.Q_INDEX:
                assert (q.index_first, q.index_last, q.index_changes) == (0, 0, 0)
            d = pl.quality_derive(q)
            assert math.isnan(d["lock"]) == (not q.flags & pl.Q_LOCK) and math.isnan(d["index_change_rate"]) == (not q.flags & pl.Q_INDEX)


# ---- 4. every way a call is scheduled --------------------------------------------------------------------------------------

def test_one_channel_time_tiled(oracle_mod, monkeypatch, capfd):
    """one channel x 2^20 samples: the time-tiled kernels; the fold spreads over 32 segments"""
    S, M = 8, 4
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)]
    n = 1 << 20
    x = _synth(64000, [M], S, n + 9000)[0]
    calls = [[x[:2 * n]], [x[2 * n:]]]
    runs = three_runs(monkeypatch, capfd, {}, 1, lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, None, cf, q))[1])
    check_case(oracle_mod, runs, lambda c: props[c], calls, 1, "one channel, 2^20 samples")
    assert any(t["what"] == "tile_front" for t in runs[1].traces[0])
    assert runs[1].nsym[0][0] > 130000


def test_automatic_tiling_of_48_channels(oracle_mod, monkeypatch, capfd):
    """48 channels x 16 blocks and a little: the automatic choice of the time-tiled kernels, the stamped control plane"""
    S, C = 8, 48
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    props = [dict(samplesPerBaud=S, constelationSize=Ms[c], numAvg=100, phaseAvg=50, differentialDecoding=c % 2) for c in range(C)]
    n = S * (16 * 128 + 100 + 37)
    host = _synth(65000, Ms, S, 2 * n)
    calls = [[host[c][:2 * n] for c in range(C)], [host[c][2 * n:] for c in range(C)]]
    check = [0, 1, 2, 17, 46, 47]
    runs = three_runs(monkeypatch, capfd, {}, C, lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, check, cf, q))[1])
    check_case(oracle_mod, runs, lambda c: props[c], calls, C, "48 channels tiled")
    assert any(t["what"] == "tile_front" for t in runs[1].traces[1])


@pytest.mark.parametrize("deferred", [False, True])
def test_mixed_batch_cut_in_time(oracle_mod, monkeypatch, capfd, deferred):
    """A mixed batch of four window classes, calls of 130 blocks and more, PSK_SOFT_SPLIT_CLASSES=3, PSK_SOFT_TIME_TILED=0: the
    library cuts every call into three pieces; one record per public call over the whole rows, one fold / join pair behind the
    last piece.  With the deferred join on, the call joins its side streams before the pass (only the pair is asserted of
    the launch lines: the option changes where that call joins)."""
    from psk_soft_amd import lib as pl

    S, C = 4, 28
    props, data, kind = _mixed_cut_batch(C, S, 2, prepass=False)
    check = [0, 1, 2, 3, 5, 6, 9, 10, C - 1]

    def body(h, cf, q):
        h.configure(0, props)
        if deferred:
            h.set_option(pl.Handle.OPT_DEFERRED_JOIN, 1)
        return device_calls(h, data, check, cf, q)

    runs = three_runs(monkeypatch, capfd, dict(PSK_SOFT_SPLIT_CLASSES=3, PSK_SOFT_TIME_TILED=0), C, body)
    check_case(oracle_mod, runs, lambda c: props[c], data, C, "mixed batch%s" % (", deferred join" if deferred else ""), pair_only=deferred)
    if not deferred:
        for lines in runs[1].traces:
            assert len({t["slot"] for t in lines if not t["what"].startswith("quality_")}) == 3, lines
            assert lines[-1]["slot"] == lines[-3]["slot"], lines[-3:]  # (the number of the call's last plan slot)


def test_call_beyond_2_20_symbols(oracle_mod, monkeypatch, capfd):
    """a call of 2^20 + 12345 symbols at samplesPerBaud 2 between two short ones: cut by the library, one record"""
    S, M = 2, 4
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50, differentialDecoding=1)]
    n_sym = (1 << 20) + 12345
    lens = [5000 * S, n_sym * S, 7000 * S]
    x = _synth(66000, [M], S, [sum(lens)])[0]
    cuts = np.cumsum([0] + lens)
    calls = [[x[2 * cuts[k]:2 * cuts[k + 1]]] for k in range(3)]
    runs = three_runs(monkeypatch, capfd, {}, 1, lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, None, cf, q))[1],
                      max_packet_complex=n_sym * S + 16)
    check_case(oracle_mod, runs, lambda c: props[c], calls, 1, "2^20 + 12345 symbols")
    assert runs[1].nsym[1][0] > (1 << 20)
    assert len({t["slot"] for t in runs[1].traces[1]}) > 1  # (pieces)


# ---- 5. the host-buffer path -----------------------------------------------------------------------------------------------

def test_process_host_in_chunks(oracle_mod, monkeypatch, capfd):
    """psk_soft_process_host with pageable packets and PSK_SOFT_STAGE_MB=1: several chunks, each a psk_soft_process_device call
    on the chunk's stream, the pass over the staging rows before they are downloaded.  The records are those of the device
    path on the same data, byte for byte."""
    from psk_soft_amd import lib as pl

    S, C = 8, 10
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    props = [dict(samplesPerBaud=S, constelationSize=Ms[c], numAvg=100, phaseAvg=50, differentialDecoding=int(c % 4 == 1)) for c in range(C)]
    lens = [40000 + 8 * c for c in range(C)]  # 320 KB a packet: three to a chunk
    host = _synth(67000, Ms, S, [2 * n for n in lens])
    calls = [[host[c][:2 * lens[c]] for c in range(C)], [host[c][2 * lens[c]:] for c in range(C)]]
    calls[1][4] = None

    def host_body(h, cf, q):
        h.configure(0, props)
        got, traces, recs, nsym = {c: [] for c in range(C)}, [], [], []
        for k in range(2):
            cf.readouterr()
            res = h.process_host(0, [None if x is None else dict(data=x, xdelta=0.01, sriChanged=(k == 0)) for x in calls[k]])
            traces.append(parse_trace(cf.readouterr().err))
            if q:
                recs.append([bytes(r) for r in h.quality_records()])
            for c in range(C):
                got[c].append(None if calls[k][c] is None else {key: res[c][key] for key in KEYS})
            nsym.append([0 if calls[k][c] is None else res[c]["phase"].size for c in range(C)])
        return Run(got, traces, recs, nsym)

    runs = three_runs(monkeypatch, capfd, dict(PSK_SOFT_STAGE_MB=1), C, host_body)
    off, on, on2 = runs
    assert_same(off.got, on.got, "host path: option on against off")
    check_parity(oracle_mod, on.got, lambda c: props[c], calls, "host path")
    for k in range(2):
        chunks = sum(1 for t in on.traces[k] if t["what"] == "quality_fold")
        assert chunks > 1, on.traces[k]
        check_traces(off.traces[k], on.traces[k], C, "host path call %d" % k, device_calls_per_call=chunks)
    check_records(on, lambda c: props[c], "host path")
    assert on.recs == on2.recs
    dev = three_runs(monkeypatch, capfd, {}, C, lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, None, cf, q))[1])[1]
    assert dev.recs == on.recs, "the device path gives other records"


# ---- 6. samples that are not finite, huge, tiny ----------------------------------------------------------------------------

def test_non_finite_and_extreme_samples(oracle_mod, monkeypatch, capfd):
    """NaN, inf, 3e19 and 1e-24 samples in otherwise clean channels: what the conditions `finite` and `lock` are for.  Counts
    and sums per the model; the streams bit for bit the oracle's."""
    from psk_soft_amd import lib as pl

    S = 8
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50, differentialDecoding=d) for M, d in ((2, 0), (4, 0), (8, 0), (4, 1), (8, 1))]
    C = len(props)
    n = 16000
    host = [x.copy() for x in _synth(68000, [p["constelationSize"] for p in props], S, 2 * n)]
    bad = (np.float32(np.nan), np.float32(np.inf), np.float32(3e19), np.float32(1e-24), np.float32(-np.inf), np.float32(-3e19), np.float32(1e-20))
    rng = np.random.default_rng(6)
    for c in range(C):
        for j, v in enumerate(bad):
            at = 2 * (3000 + 1500 * j) + c % 2
            host[c][at:at + 2 * S * 3:2] = v        # three symbols' worth of I (or Q) samples
            host[c][int(rng.integers(30000, 60000))] = v
        host[c][2 * 20000:2 * 20400] *= np.float32(1e-12)   # energies that are denormal floats
        host[c][2 * 24000:2 * 24400] *= np.float32(3e9)     # |z|^8 overflows where |z|^2 does not
    calls = [[host[c][:2 * n] for c in range(C)], [host[c][2 * n:] for c in range(C)]]
    runs = three_runs(monkeypatch, capfd, {}, C, lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, None, cf, q))[1])
    check_case(oracle_mod, runs, lambda c: props[c], calls, C, "extreme samples")
    seen_not_finite = seen_not_lock = 0
    for k in range(2):
        for c in range(C):
            q = pl.Quality.from_buffer_copy(runs[1].recs[k][c])
            seen_not_finite += q.n_symbols - q.n_finite
            seen_not_lock += q.n_finite - q.n_lock
    assert seen_not_finite > 10 and seen_not_lock > 10, (seen_not_finite, seen_not_lock)


# ---- 7. the machine-filling shape ------------------------------------------------------------------------------------------

def test_machine_filling_batch(oracle_mod, monkeypatch, capfd):
    """4096 channels x 32768 samples, QPSK, samplesPerBaud 8, device pointers, rows on 128-byte boundaries: 130 channels
    compared (every 32nd, the first and the last two)."""
    S, M, C, n = 8, 4, 4096, 32768
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50)
    base = _synth(69000, [M] * 64, S, n)
    rng = np.random.default_rng(7)
    rot = np.exp(2j * np.pi * rng.random(C)).astype(np.complex64)
    calls = [[None] * C]
    for c in range(C):  # (64 stimuli, every channel its own rotation of one of them)
        calls[0][c] = (base[c % 64].view(np.complex64) * rot[c]).view(np.float32)
    check = sorted(set(range(0, C, 32)) | {C - 2, C - 1})
    assert len(check) == 130
    runs = three_runs(monkeypatch, capfd, {}, C,
                      lambda h, cf, q: (h.configure_all(**props), device_calls(h, calls, check, cf, q))[1])
    check_case(oracle_mod, runs, lambda c: props, calls, C, "machine-filling batch")
    assert len({r for r in runs[1].recs[0]}) > 4000  # (every channel a record of its own)


# ---- 8. what the numbers are for -------------------------------------------------------------------------------------------

def test_lock_and_snr_order_channels_by_their_signal(oracle_mod, monkeypatch, capfd):
    """Per (M, differential) three channels: the stimulus at sigma 0.01, at sigma 0.2, and Gaussian noise without a signal.  `lock`
    strictly decreases in that order, `snr_db` likewise where it is not NaN.  No threshold is asserted."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    S, n = 8, 8 * 5000
    combos = [(M, d) for M in (2, 4, 8) for d in (0, 1)]
    props, data = [], []
    for i, (M, d) in enumerate(combos):
        for j, sigma in enumerate((0.01, 0.2, None)):
            props.append(dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50, differentialDecoding=d))
            if sigma is None:
                g = np.random.default_rng(7000 + i)
                data.append((0.7 * g.standard_normal(2 * n)).astype(np.float32))
            else:
                data.append(synth_channel(70000 + i, M, S, n, sigma=sigma))
    C = len(props)
    calls = [data]
    runs = three_runs(monkeypatch, capfd, {}, C, lambda h, cf, q: (h.configure(0, props), device_calls(h, calls, None, cf, q))[1])
    check_case(oracle_mod, runs, lambda c: props[c], calls, C, "signal and noise")
    for i, (M, d) in enumerate(combos):
        q = [pl.Quality.from_buffer_copy(runs[1].recs[0][3 * i + j]) for j in range(3)]
        der = [pl.quality_derive(x) for x in q]
        print("M=%d differential=%d: lock %.4f %.4f %.4f, snr_db %.2f %.2f %.2f" % ((M, d) + tuple(x["lock"] for x in der) + tuple(x["snr_db"] for x in der)))
        assert der[0]["lock"] > der[1]["lock"] > der[2]["lock"], (M, d, der)
        snr = [x["snr_db"] for x in der if not math.isnan(x["snr_db"])]
        assert all(a > b for a, b in zip(snr, snr[1:])), (M, d, snr)
        assert (len(snr) == 0) if d else (len(snr) >= 2), (M, d, snr)


# ---- 9. the slot ring wraps with calls in flight ---------------------------------------------------------------------------

def wrapping_calls(seed, dtype=np.float32, spans=None):
    """Nine calls of about 300 symbols a channel (QPSK, samplesPerBaud 8, numAvg 25, phaseAvg 50: less than three blocks, the
    last one partial) on a handle of 8 channels -- one more than two turns of every four-slot ring.  The first, third, ...
    cover channels [0, 6), the others [2, 8); they alternate between the handle's stream and a second one.
    (spans: other channel ranges, one (ch0, nch) per call.)  dtype other than float32: int8 values cast to it.
    Returns (props, calls, spans): calls[k][c] = the next samples of channel c's stream, None outside the call's span."""
    S, C, K = 8, 8, 9
    props = [dict(samplesPerBaud=S, constelationSize=4, numAvg=25, phaseAvg=50)] * C
    spans = spans or [(0, 6) if k % 2 == 0 else (2, 6) for k in range(K)]
    lens = [[S * 300 + 8 * c + k if lo <= c < lo + n else 0 for c in range(C)] for k, (lo, n) in enumerate(spans)]
    raw = _synth(seed, [4] * C, S, [sum(lens[k][c] for k in range(K)) for c in range(C)])
    if dtype != np.float32:
        raw = [q8(x).astype(dtype) for x in raw]
    calls, at = [], [0] * C
    for k in range(K):
        calls.append([raw[c][2 * at[c]:2 * (at[c] + lens[k][c])] if lens[k][c] else None for c in range(C)])
        at = [at[c] + lens[k][c] for c in range(C)]
    return props, calls, spans


def test_slot_ring_wraps_with_calls_in_flight_on_two_streams(oracle_mod, monkeypatch, capfd):
    """wrapping_calls back to back, no host wait between them, one psk_soft_synchronize at the end: the four streams of all nine
    calls are the oracle's; the final record of every channel is that of the same calls with a wait after each; under the launch
    trace nine quality_fold and nine quality_join lines are written."""
    from psk_soft_amd import lib as pl
    from tests.test_gpu_acquire import _second_stream

    props, calls, spans = wrapping_calls(71000)
    C, K = 8, len(calls)
    second = _second_stream()
    streams = [None if k % 2 == 0 else second.value for k in range(K)]

    def run(sync_each, cf=None):
        h = pl.Handle(C, device=0)
        try:
            h.configure(0, props)
            h.set_option(pl.Handle.OPT_QUALITY, 1)
            return device_calls(h, calls, None, cf, True, sync_each=sync_each, streams=streams, spans=spans)
        finally:
            h.close()

    try:
        monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES", raising=False)
        flight = run(False)
        check_parity(oracle_mod, flight.got, lambda c: props[c], calls, "ring wrap in flight")
        waited = run(True)
        assert_same(flight.got, waited.got, "in flight against a wait after each call")
        assert len(flight.recs) == 1 and len(waited.recs) == K
        assert flight.recs[0] == waited.recs[-1], "final records differ from those of the run that waits after each call"
        assert all(r != bytes(88) for r in flight.recs[0])
        monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
        traced = run(False, capfd)
        lines = [t for per_call in traced.traces for t in per_call]
        assert sum(t["what"] == "quality_fold" for t in lines) == K and sum(t["what"] == "quality_join" for t in lines) == K, lines
        assert len({t["stream"] for t in lines if t["what"] == "quality_fold"}) == 2
    finally:
        monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES", raising=False)
        pl.load().hipStreamDestroy(second)
