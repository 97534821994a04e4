"""psk_soft_acquire_device on a real MI355X (psk_acquire.hip): the records of the device against tests/acquire_model.py at the
edges of the kernel's pieces, their independence of the batch, the stream, the format, the stride and the tune (byte for byte),
the absence of side effects on the demodulator (streams against the oracle, statistics and quality records against a run without
the looks), and the loop the call is for: look, derive, tune, demodulate."""
import ctypes
import math

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from psk_soft_amd.stimulus import synth_channel
from tests import acquire_model as am
from tests import tune_model as tm

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
FMT = {np.dtype(F32): pl.FORMAT_CF32, np.dtype(np.int16): pl.FORMAT_CS16, np.dtype(np.int8): pl.FORMAT_CS8, np.dtype(F16): pl.FORMAT_CF16}
POISON = {np.dtype(F32): np.uint32(0x7FC00ABC).view(F32), np.dtype(np.int16): np.int16(-32768), np.dtype(np.int8): np.int8(-128),
          np.dtype(F16): np.uint16(0x7E55).view(F16)}
P = None             # samples of one piece of the fold, read from the binding ...
EDGE_LENGTHS = None  # ... and the lengths at its edges: both set when the first test runs (collecting the module loads no library)
A_BYTES = 224


@pytest.fixture(autouse=True, scope="module")
def _piece_of_the_binding():
    global P, EDGE_LENGTHS
    P = pl.acquire_piece()
    EDGE_LENGTHS = (1, 2, 127, 128, 129, P - 1, P, P + 1, P + 127, P + 129, 2 * P + 5, 3 * P + 1)


def look(h, items, ch0=0, place=None, widths=None, tunes=None, stream=None, real=(), capfd=None, keep=None, skew=0):
    """One psk_soft_acquire_device call over channels ch0 .. ch0 + len(items) - 1.  items[i]: the packet's interleaved I/Q
    (float32 / int16 / int8 / float16) or None (no packet).  place[i]: None -- contiguous -- or (m, col): column `col` of matrix
    m, widths[m] complex samples wide, as many frames as its longest column, everything else in it poison.  real: packets handed
    over as real data (sri_mode 0).  skew: poison samples in front of every contiguous packet (a packet that starts `skew`
    samples behind a 128-byte boundary).  The source is uploaded in front of the call and compared with what is there behind it.
    Returns ([bytes of record i], the ctypes records, the launch lines of the call).  keep: a list -- the call is only enqueued,
    nothing is waited for or read back, and the source buffer is appended to the list for the caller to free."""
    from tests.test_gpu_cs16_schedules import parse_trace

    n = len(items)
    place = place or [None] * n
    al = lambda b: (b + 127) // 128 * 128  # noqa: E731
    parts, off, where, mats = [], 0, {}, {}
    for i, x in enumerate(items):
        if x is None:
            continue
        if place[i] is None:
            where[i] = (off + skew * 2 * x.dtype.itemsize, 1)
            part = np.frombuffer(np.full(2 * skew, POISON[x.dtype], x.dtype).tobytes() + np.ascontiguousarray(x).tobytes(), np.uint8)
            parts.append(np.concatenate([part, np.full(al(part.size + 1) - part.size, 0xEE, np.uint8)]))
            off += parts[-1].size
        else:
            mats.setdefault(place[i][0], []).append(i)
    for m, chans in mats.items():
        dt = items[chans[0]].dtype
        assert all(items[i].dtype == dt for i in chans)
        frames = max(items[i].size // 2 for i in chans)
        mat = np.full((frames, widths[m], 2), POISON[dt], dt)
        for i in chans:
            k = items[i].size // 2
            mat[:k, place[i][1], :] = items[i][: 2 * k].reshape(k, 2)
            where[i] = (off + place[i][1] * 2 * dt.itemsize, widths[m])
        part = np.frombuffer(mat.tobytes(), np.uint8)
        parts.append(np.concatenate([part, np.full(al(part.size + 1) - part.size, 0xEE, np.uint8)]))
        off += parts[-1].size
    src = np.concatenate(parts) if parts else np.zeros(128, np.uint8)
    base = h.device_alloc(src.size)
    try:
        h.upload(base, src)
        pk, strides = (pl.Packet * n)(), [1] * n
        for i, x in enumerate(items):
            if x is None:
                continue
            o, strides[i] = where[i]
            pk[i].data, pk[i].n_floats, pk[i].sri_xdelta, pk[i].sri_mode = base + o, x.size, 0.01, 0 if i in real else 1
            pk[i].present, pk[i].format = 1, FMT[x.dtype]
            pk[i].sriChanged = pk[i].inputQueueFlushed = i % 2  # (ignored)
        if capfd:
            capfd.readouterr()
        h.acquire_device(ch0, pk, strides if any(p is not None for p in place) else None, tunes, stream)
        lines = parse_trace(capfd.readouterr().err) if capfd else []
        if keep is not None:
            keep.append(base)
            base = None
            return None, None, lines
        recs = h.acquire_records(ch0, n)
        assert np.array_equal(h.download(base, (src.size,), np.uint8), src), "the source buffer changed"
        return [bytes(r) for r in recs], recs, lines
    finally:
        if base is not None:
            h.device_free(base)


def _carrier(seed, M, n, scale=1.0):
    """a noisy M-PSK carrier at 0.007 cycles per sample, 4 samples per symbol, interleaved float32"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    z = np.exp(2j * math.pi * (np.repeat(rng.integers(0, M, n // 4 + 1), 4)[:n] / M + 0.007 * k)) * rng.uniform(0.8, 1.25) + 0.08 * (
        rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.empty(2 * n, F32)
    x[0::2], x[1::2] = z.real * scale, z.imag * scale
    return x


def _edge_packets(M):
    """the packets of EDGE_LENGTHS; in some of them an inf, a NaN and a run of 200 zeros lie across the piece boundary"""
    out = []
    for i, n in enumerate(EDGE_LENGTHS):
        x = _carrier(7000 + 13 * i + M, M, n)
        if n > P and i % 2 == 1:
            x[2 * (P - 1)] = np.inf          # the last sample of piece 0
            x[2 * P + 1] = np.nan            # the first of piece 1
        if n >= P + 127 and i % 3 == 0:
            x[2 * (P - 100) : 2 * min(n, P + 100)] = 0.0
        if n >= 2 * P + 5:
            x[2 * (2 * P - 64) + 1] = -np.inf  # reaches over the next boundary through the longer lags
        out.append(x)
    return out


_edge_cache = {}


def _edge_models(M):
    """the packets and their model records, computed once"""
    if M not in _edge_cache:
        xs = _edge_packets(M)
        _edge_cache[M] = (xs, [am.model_record(x, M) for x in xs])
    return _edge_cache[M]


def _handle(Ms, **kw):
    h = pl.Handle(len(Ms), device=0, **kw)
    h.configure(0, [dict(constelationSize=M, samplesPerBaud=8) for M in Ms])
    return h


def _second_stream():
    s = ctypes.c_void_p()
    assert pl.load().hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0  # (non-blocking)
    return s


# ---- 1. lengths at the edges of the kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", (2, 4, 8))
def test_lengths_at_the_edges_of_a_piece_against_the_model(M):
    xs, models = _edge_models(M)
    h = _handle([M] * len(xs))
    try:
        _, recs, _ = look(h, xs)
        for i, (r, model) in enumerate(zip(recs, models)):
            ctx = "M %d n %d" % (M, EDGE_LENGTHS[i])
            am.assert_record(r, model, ctx)
            assert r.flags == pl.A_DATA and r.n_samples == EDGE_LENGTHS[i]
            am.assert_derived(pl.acquire_derive(r), am.derive(r), ctx)
        d = pl.acquire_derive(recs[-1])
        assert d["lags_used"] == 8 and abs(d["offset_cycles_per_sample"] - 0.007) < 1e-4, d
        assert models[1]["n_pairs"] == [1, 0, 0, 0, 0, 0, 0, 0] and models[5]["n_valid"] == P - 1
        assert any(m["n_valid"] < m["n_samples"] for m in models)
    finally:
        h.close()


def test_a_packet_of_66_pieces_among_short_ones():
    """65 P + 131 samples of CS16: the join's lanes 0 and 1 take two partials each, and the handle's scratch grows to 66 partials
    and more.  At this length assert_record's bound is two orders wider than one float32 rounding of a term, so the record is
    held to acquire_model.device_record -- the device's order of additions restated -- byte for byte as well; the short packets
    around it, the edge packets of M = 4, keep their model records."""
    n, M = 65 * P + 131, 8
    long = np.round(_carrier(8100, M, n, 40.0)).astype(np.int16)
    long[2 * (64 * P - 1) : 2 * (64 * P + 90)] = 0  # (91 invalid samples across the boundary of piece 64)
    xs, models = _edge_models(4)
    items = xs[:5] + [long] + xs[5:]
    h = _handle([4] * 5 + [M] + [4] * (len(xs) - 5))
    try:
        got, recs, _ = look(h, items)
        assert got[5] == am.device_record(long, M), "65 P + 131 samples: the record is not the restated order's"
        model = am.model_record(long, M)
        am.assert_record(recs[5], model, "65 P + 131 samples")
        assert recs[5].n_samples == n and recs[5].n_valid == n - 91 and recs[5].flags == pl.A_DATA
        am.assert_derived(pl.acquire_derive(recs[5]), am.derive(recs[5]), "65 P + 131 samples")
        for i, r in enumerate(recs[:5] + recs[6:]):
            am.assert_record(r, models[i], "beside the long packet, n %d" % EDGE_LENGTHS[i])
        # alone on a fresh handle, whose scratch grows from nothing: the same bytes
        g = _handle([M])
        try:
            assert look(g, [long])[0][0] == got[5]
        finally:
            g.close()
    finally:
        h.close()


# ---- 2. independence of the batch --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rot", (0, 1, 2))
def test_a_record_does_not_depend_on_the_batch_the_handle_or_the_stream(rot):
    """the twelve edge packets alone (one call each), among 58 packets of other lengths and formats in one call, and in that
    batch on a second fresh handle on a non-default stream: byte-identical records; `rot` turns M over the lengths, so that
    every length meets every M"""
    C = 70
    Ms = [(2, 4, 8)[(c + rot) % 3] for c in range(C)]
    at = [3 + 5 * i for i in range(len(EDGE_LENGTHS))]  # where the edge packets sit in the batch
    dts = (F32, np.int16, np.int8, F16)
    items = []
    for c in range(C):
        if c in at:
            items.append(_edge_models(Ms[c])[0][at.index(c)])
        else:
            n = (1, 300, P + 17, 2 * P - 1, 5 * P + 3, 777)[c % 6] + c
            items.append(np.round(_carrier(9000 + c, Ms[c], n, 40.0)).astype(dts[c % 4]))
    h = _handle(Ms)
    second = _second_stream()
    try:
        batch, recs, _ = look(h, items)
        for i, c in enumerate(at):
            am.assert_record(recs[c], _edge_models(Ms[c])[1][i], "in the batch, n %d" % EDGE_LENGTHS[i])
        alone = [look(h, [items[c]], ch0=c)[0][0] for c in at]
        assert alone == [batch[c] for c in at]
        assert [bytes(r) for r in h.acquire_records()] == batch  # (the calls on one channel left the others alone)
        g = _handle(Ms)
        try:
            other, _, _ = look(g, items, stream=second.value)
        finally:
            g.close()
        assert other == batch
    finally:
        pl.load().hipStreamDestroy(second)
        h.close()


# ---- 3. formats ----------------------------------------------------------------------------------------------------------------------

def test_the_integer_and_half_formats_give_the_records_of_their_float_packets():
    lens = (1, 2, 129, P - 1, P + 1, 2 * P + 5)
    Ms = [(2, 4, 8)[i % 3] for i in range(len(lens))]
    vals = [np.clip(np.round(_carrier(11000 + i, Ms[i], n, 40.0)), -128, 127).astype(np.int8) for i, n in enumerate(lens)]
    h = _handle(Ms)
    try:
        want, recs, _ = look(h, [v.astype(F32) for v in vals])
        for i, r in enumerate(recs):
            am.assert_record(r, am.model_record(vals[i], Ms[i]), "int8 values, n %d" % lens[i])
        for dt in (np.int16, np.int8, F16):
            got, _, _ = look(h, [v.astype(dt) for v in vals])
            assert got == want, dt
        # packets that start one and three samples behind a 128-byte boundary: the pairs are no longer aligned to their size
        for dt in (F32, np.int16, np.int8, F16):
            for skew in (1, 3):
                assert look(h, [v.astype(dt) for v in vals], skew=skew)[0] == want, (dt, skew)
    finally:
        h.close()


# ---- 4. strides ----------------------------------------------------------------------------------------------------------------------

def _columns(seed, dt, C, Ms, base_len):
    return [np.clip(np.round(_carrier(seed + c, Ms[c], base_len + 61 * ((5 * c) % 7) + c, 40.0)), -128, 127).astype(dt) for c in range(C)]


@pytest.mark.parametrize("dt", (F32, np.int16, np.int8, F16))
def test_columns_of_a_frame_major_matrix(monkeypatch, capfd, dt):
    """twelve adjacent columns of a matrix 20 wide, ragged lengths around one piece, which the tile gather takes; then every third
    of them, which are no neighbours and are read where they lie: byte-identical to the contiguous packets of the same samples,
    the matrix unchanged (look() compares it)"""
    C = 12
    Ms = [(4, 8, 2)[c % 3] for c in range(C)]
    cols = _columns(13000, dt, C, Ms, P - 200)
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    h = _handle(Ms)
    try:
        want, recs, _ = look(h, cols)
        assert all(r.flags == pl.A_DATA for r in recs)
        got, _, lines = look(h, cols, place=[(0, 3 + c) for c in range(C)], widths={0: 20}, capfd=capfd)
        assert got == want
        assert [t["what"] for t in lines] == ["gather_tiles", "acquire_fold", "acquire_join"], lines  # (one group, one sample size)
        third = list(range(0, C, 3))
        g = _handle([Ms[c] for c in third])
        try:
            got3, _, lines = look(g, [cols[c] for c in third], place=[(0, 3 + c) for c in third], widths={0: 20}, capfd=capfd)
        finally:
            g.close()
        assert got3 == [want[c] for c in third]
        assert [t["what"] for t in lines] == ["acquire_fold", "acquire_join"], lines  # (read where they lie: no gather)
    finally:
        monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES")
        h.close()


# ---- 5. tunes ------------------------------------------------------------------------------------------------------------------------

def _untuned(b):
    """a record's bytes with PSK_SOFT_A_TUNED cleared: a tuned look says so in its flags, everything else is the model packet's"""
    r = pl.Acquire.from_buffer_copy(b)
    r.flags &= ~pl.A_TUNED
    return bytes(r)


def test_tuned_packets_give_the_records_of_their_model_packets():
    """a tuned packet of each format, contiguous, as a single column and as one of nine adjacent columns (gathered): its record is that of
    the untuned CF32 packet holding tune_model.apply of it, but for the TUNED flag; {0, 0} and tune == NULL are the untuned call"""
    dts = (F32, np.int16, np.int8, F16)
    C = 4 + 4 + 9
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    items = [np.clip(np.round(_carrier(15000 + c, Ms[c], (P + 300, 2 * P + 1, 555, P - 1)[c % 4] + c, 40.0)), -128, 127).astype(
        dts[c % 4] if c < 8 else np.int16) for c in range(C)]
    place = [None] * 4 + [(1 + c, 1) for c in range(4)] + [(0, 2 + c) for c in range(9)]
    widths = {0: 12, 1: 3, 2: 2, 3: 5, 4: 4}
    tunes = [((0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64), (tm.step_word(0.0031), tm.step_word(-0.012), (1 << 63) + 12345, 1)[c % 4])
             for c in range(C)]
    tunes[2] = tunes[6] = tunes[12] = (0, 0)
    model = [x.astype(F32) if t == (0, 0) else tm.apply(t[0], t[1], x) for x, t in zip(items, tunes)]
    h = _handle(Ms)
    try:
        want, _, _ = look(h, model)
        got, recs, _ = look(h, items, place=place, widths=widths, tunes=tunes)
        for c in range(C):
            assert recs[c].flags == pl.A_DATA | (0 if tunes[c] == (0, 0) else pl.A_TUNED), c
            assert _untuned(got[c]) == want[c], c
            am.assert_record(recs[c], am.model_record(items[c], Ms[c], tunes[c]), "tuned, channel %d" % c)
        plain, _, _ = look(h, items, place=place, widths=widths)
        zeros, _, _ = look(h, items, place=place, widths=widths, tunes=[(0, 0)] * C)
        assert plain == zeros and plain == look(h, [x.astype(F32) for x in items])[0]
    finally:
        h.close()


# ---- 6. no side effects ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", (0, 1))
def test_looks_between_process_calls_change_nothing(oracle_mod, monkeypatch, capfd, deferred):
    """three process calls with PSK_SOFT_OPT_QUALITY, a look in front of the second and one in front of the third (tuned, with a
    frame group and single columns, over the same channels): all four streams are bit for bit the oracle's, statistics and quality
    records byte for byte those of the run without the looks, and the looks launch the gather of their frame group, acquire_fold
    and acquire_join only"""
    from tests.test_gpu_cs16_schedules import _synth, assert_same, check_parity, device_run

    S, C, calls = 8, 12, 3
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 200)[c % 2], phaseAvg=(50, 10)[(c // 3) % 2],
                  differentialDecoding=int(c % 5 == 3)) for c in range(C)]
    lens = [[3000 + 160 * ((5 * c + 3 * k) % 7) for c in range(C)] for k in range(calls)]
    raw = _synth(17000, [p["constelationSize"] for p in props], S, [sum(lens[k][c] for k in range(calls)) for c in range(C)])
    streams = [x if c % 2 else np.clip(np.round(40.0 * x), -32768, 32767).astype(np.int16) for c, x in enumerate(raw)]
    data, at = [], [0] * C
    for k in range(calls):
        data.append([streams[c][2 * at[c] : 2 * (at[c] + lens[k][c])] for c in range(C)])
        at = [at[c] + lens[k][c] for c in range(C)]
    looked = [np.clip(np.round(_carrier(17500 + c, props[c]["constelationSize"], P + 50 * c, 40.0)), -128, 127).astype(np.int16)
              for c in range(C)]
    place = [(0, 1 + c) for c in range(9)] + [(1, 0), (1, 2), None]
    tunes = [(c << 40, tm.step_word(0.001 * (c - 4))) for c in range(C)]
    look_lines, keep = [], []

    def run(with_looks, trace):
        if trace:
            monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
        h = pl.Handle(C, device=0)
        try:
            h.configure(0, props)
            h.set_option(pl.Handle.OPT_QUALITY, 1)
            h.set_option(pl.Handle.OPT_DEFERRED_JOIN, deferred)

            def before(hh, k):
                if with_looks and k >= 1:
                    look_lines.append(look(hh, looked, place=place, widths={0: 11, 1: 3}, tunes=tunes, capfd=capfd if trace else None,
                                           keep=keep)[2])

            got = device_run(h, data, capfd if trace else None, before=before, sync_each=not deferred)[0]
            acq = bytes(h.acquire_records())
            for b in keep:
                h.device_free(b)
            del keep[:]
            return got, h.stats(), h.channel_stats(), bytes(h.quality_records()), acq
        finally:
            monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES", raising=False)
            h.close()

    ref = run(False, False)
    got = run(True, False)
    traced = run(True, True)
    for r in (got, traced):
        assert_same(r[0], ref[0], "with looks against without")
        assert r[1:4] == ref[1:4]
    assert ref[4] == bytes(A_BYTES * C) and got[4] == traced[4] and got[4] != ref[4]
    assert len(look_lines) == 4 and not any(look_lines[:2])
    for lines in look_lines[2:]:
        assert [t["what"] for t in lines] == ["gather_tiles", "acquire_fold", "acquire_join"], lines
    check_parity(oracle_mod, got[0], lambda c: props[c], data, "looks between the calls")


# ---- 7. zero records and kept records ----------------------------------------------------------------------------------------------------

def test_zero_records_and_kept_records():
    Ms = [4, 2, 8, 16, 4, 4, 2, 8]
    xs = [_carrier(19000 + c, 4, 500 + c) for c in range(8)]
    h = _handle(Ms)
    try:
        first, recs, _ = look(h, xs)
        assert [r.flags for r in recs] == [1, 1, 1, 0, 1, 1, 1, 1] and first[3] == bytes(A_BYTES)  # (constelationSize 16)
        # channels 1 .. 5: no packet, real data, (16 again), one float only, a packet
        items = [None, xs[2], xs[3], xs[4][:1], xs[5][:400]]
        got, recs, _ = look(h, items, ch0=1, real=(1,))
        assert got[:4] == [bytes(A_BYTES)] * 4 and recs[4].flags == pl.A_DATA and recs[4].n_samples == 200
        now = [bytes(r) for r in h.acquire_records()]
        assert now[0] == first[0] and now[6:] == first[6:] and now[1:6] == got
        am.assert_record(recs[4], am.model_record(xs[5][:400], 4), "the rewritten record")
    finally:
        h.close()


# ---- 7b. the slot ring wraps with looks in flight -----------------------------------------------------------------------------------------

def test_slot_ring_wraps_with_looks_in_flight_on_two_streams():
    """Nine looks back to back -- one more than two turns of the four-slot ring -- over channels [0, 6) and [2, 8) in turn, on the
    handle's stream and a second one in turn, nothing waited for until the records are read: every channel's record is the
    model's for the last look that covered it, and byte for byte that of the same looks with a wait after each."""
    C, K, M = 8, 9, 4
    spans = [(0, 6) if k % 2 == 0 else (2, 6) for k in range(K)]
    items = [[_carrier(21000 + 16 * k + c, M, 2400 + 8 * c + k) for c in range(lo, lo + n)] for k, (lo, n) in enumerate(spans)]
    last = {c: max(k for k, (lo, n) in enumerate(spans) if lo <= c < lo + n) for c in range(C)}
    second = _second_stream()

    def run(in_flight):
        h, keep = _handle([M] * C), []
        try:
            for k, (lo, n) in enumerate(spans):
                look(h, items[k], ch0=lo, stream=None if k % 2 == 0 else second.value, keep=keep if in_flight else None)
            return h.acquire_records()
        finally:
            for b in keep:
                h.device_free(b)
            h.close()

    try:
        flight, waited = run(True), run(False)
        for c in range(C):
            am.assert_record(flight[c], am.model_record(items[last[c]][c - spans[last[c]][0]], M), "channel %d, look %d" % (c, last[c]))
        assert bytes(flight) == bytes(waited)
    finally:
        pl.load().hipStreamDestroy(second)


# ---- 8. look, derive, tune, demodulate -------------------------------------------------------------------------------------------------

def test_the_loop_the_look_is_for(oracle_mod):
    """QPSK 0.10 and 8-PSK 0.20 cycles per symbol off centre, channels 1 .. 3 each: acquire_device on the first 4096 samples, the
    derived step into process_device_tuned on the whole packet; the streams are bit for bit the oracle's on tune_model.apply of
    that step, and the quality record's lock is above 0.95 / 0.85"""
    from tests.test_gpu_cs16_schedules import check_parity
    from tests.test_gpu_strided import strided_run
    from tests.test_gpu_tune import Tuned

    cases = [(4, 0.10, 0.95, ch) for ch in (1, 2, 3)] + [(8, 0.20, 0.85, ch) for ch in (1, 2, 3)]
    C = len(cases)
    xs = [synth_channel(ch, M, 8, 24000, sigma=0.05, cfo=2 * math.pi * M * r) for M, r, _, ch in cases]
    h = _handle([M for M, _, _, _ in cases])
    try:
        h.set_option(pl.Handle.OPT_QUALITY, 1)
        _, recs, _ = look(h, [x[: 2 * 4096] for x in xs])
        ds = [pl.acquire_derive(r) for r in recs]
        for (M, r, _, ch), d, x in zip(cases, ds, xs):
            print("M %d ch %d: estimate %.6f cycles per symbol (error %.2g), coherence %.3f" % (
                M, ch, 8 * d["offset_cycles_per_sample"], 8 * d["offset_cycles_per_sample"] - r, d["coherence"]))
            assert abs(8 * d["offset_cycles_per_sample"] - r) <= 2e-4
            am.assert_derived(d, am.derive(pl.acquire_host(M, x[: 2 * 4096])), "device against host record")
        tunes = [(0, pl.tune_step(-d["offset_cycles_per_sample"])) for d in ds]
        got = strided_run(Tuned(h, [tunes]), [xs], [None] * C, {})[0]
        q = h.quality()
        model = [[tm.apply(t[0], t[1], x) for t, x in zip(tunes, xs)]]
        check_parity(oracle_mod, got, lambda c: dict(samplesPerBaud=8, constelationSize=cases[c][0]), model, "acquire, tune, process")
        for (M, r, floor, ch), qc in zip(cases, q):
            print("M %d ch %d: lock %.4f" % (M, ch, qc["lock"]))
            assert qc["lock"] > floor
    finally:
        h.close()
