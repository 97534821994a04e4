"""psk_soft_symrate_device on a real MI355X (psk_symrate.hip): the records of the device against tests/symrate_model.py, byte for
byte, at the edges of the kernel's pieces and of its halo; their independence of the batch, the handle, the stream, the format, the
stride and the tune; the blocks a non-finite sample invalidates; the absence of side effects on the demodulator; and the loop the
call is for: look, step, resample, demodulate."""
import math

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests import symrate_model as sm
from tests import tune_model as tm
from tests.test_gpu_acquire import _second_stream
from tests.test_gpu_acquire import look as _acquire_look
from tests.test_symrate_control import _samples

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
R_BYTES = 392
P, H = sm.PIECE, sm.HALO  # (tests/test_symrate_control.py holds the binding's piece to the model's)


class _Symrate:
    """a Handle whose acquire_device / acquire_records are symrate_device / symrate_records: tests/test_gpu_acquire.py's look()
    -- the layout of the sources, the poison around them, the comparison of the source buffer behind the call -- makes the
    symbol-rate look through it"""

    def __init__(self, h):
        self._h = h

    def __getattr__(self, name):
        return getattr(self._h, name)

    def acquire_device(self, *a):
        return self._h.symrate_device(*a)

    def acquire_records(self, *a):
        return self._h.symrate_records(*a)


def look(h, items, **kw):
    return _acquire_look(_Symrate(h), items, **kw)


def _handle(Ss, **kw):
    h = pl.Handle(len(Ss), device=0, **kw)
    h.configure(0, [dict(constelationSize=4, samplesPerBaud=S, numAvg=8) for S in Ss])
    return h


def _edge_blocks(S):
    """block counts at the edges: two blocks, either side of the piece boundaries and of the halo behind the first, 129, the cap"""
    every = [k * P for k in range(1, 8)] if S in (4, 5, 8, 33) else [P]  # (every piece edge up to the cap at four block lengths)
    return [2] + sorted({b + e for b in every for e in (-1, 0, 1)} | {P + H - 1, P + H, P + H + 1, 129, 4096})


def _edge_lengths(S):
    """(n, blocks the look uses); some lengths with a ragged tail, 2S + 1, and one that reaches beyond the cap"""
    out = [(2 * S, 2), (2 * S + 1, 2)]
    for i, b in enumerate(_edge_blocks(S)[1:]):
        out.append((b * S + (0, S - 1, 3)[i % 3] if b < 4096 else b * S, b))
    return out + [(4096 * S + S + 3, 4096)]


_edge_cache = {}


def _edge_models(S):
    """the edge packets of S and their model records, computed once"""
    if S not in _edge_cache:
        lens = _edge_lengths(S)
        xs = [_samples(S, n, "signal", 500 * S + i) for i, (n, _) in enumerate(lens[:-1])]
        models = [sm.model_record(x, S) for x in xs]
        # the packet beyond the cap: the one of 4096 blocks and S + 3 samples more, which the look does not use -- by the
        # definition its record is that packet's but for n_samples (the model is computed once for the two)
        assert lens[-2] == (4096 * S, 4096) and lens[-1][0] == 4096 * S + S + 3
        xs.append(np.concatenate([xs[-1], _samples(S, S + 3, "signal", 77)]))
        models.append(dict(models[-1], n_samples=lens[-1][0]))
        _edge_cache[S] = (xs, models)
    return _edge_cache[S]


# ---- 1. lengths at the edges of the kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", (4, 5, 8, 17, 33, 200, 257, 1024))
def test_lengths_at_the_edges_of_a_piece_against_the_model(S):
    xs, models = _edge_models(S)
    lens = _edge_lengths(S)
    h = _handle([S] * (len(xs) + 1))
    try:
        got, recs, _ = look(h, xs + [xs[0][: 2 * (2 * S - 1)]])
        for i, (r, model) in enumerate(zip(recs, models)):
            ctx = "S %d n %d" % (S, lens[i][0])
            sm.assert_bytes(r, model, ctx)
            assert r.flags == pl.SR_DATA and (r.n_samples, r.n_blocks, r.n_used, r.n_valid) == (lens[i][0], lens[i][1], lens[i][1] * S, lens[i][1]), ctx
            assert list(r.n_pairs) == [max(0, lens[i][1] - L) for L in sm.LAGS], ctx
            sm.assert_derived(pl.symrate_derive(r), sm.derive(r), ctx)
            sm.assert_close(pl.symrate_host(S, xs[i]), model, ctx)
        assert got[-1] == bytes(R_BYTES)  # (2S - 1 samples: the zero record)
        d = pl.symrate_derive(recs[-2])
        assert d["lags_used"] == 8 and d["detector"] == 0 and abs(d["samples_per_symbol"] / (1.04 * S) - 1) < 5e-4, d
    finally:
        h.close()


# ---- 2. independence of the batch --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rot", (0, 1, 2))
def test_a_record_does_not_depend_on_the_batch_the_handle_or_the_stream(rot):
    """edge packets of S = 8 and S = 5 alone (one call each), among 70 packets of other lengths, block lengths and formats in one
    call, and in that batch on a second fresh handle on a non-default stream: byte-identical records, the model's; `rot` moves
    them through the batch"""
    C = 70
    picks = [(8, i) for i in (0, 1, 3, 4, 5, 14, 26)] + [(5, i) for i in (2, 9, 25, 27)]
    at = [(3 + 6 * i + 23 * rot) % C for i in range(len(picks))]
    assert len(set(at)) == len(at)
    dts = (F32, np.int16, np.int8, F16)
    Ss, items = [], []
    for c in range(C):
        if c in at:
            S, i = picks[at.index(c)]
            Ss.append(S)
            items.append(_edge_models(S)[0][i])
        else:
            Ss.append((4, 5, 8, 33, 100, 16)[c % 6])
            n = Ss[-1] * (2, 40, P + 17, 2 * P - 1, 700, 130)[(c // 6) % 6] + c
            items.append(np.clip(np.round(40.0 * _samples(Ss[-1], n, "signal", 9000 + c)), -128, 127).astype(dts[c % 4]))
    h = _handle(Ss)
    second = _second_stream()
    try:
        batch, recs, _ = look(h, items)
        for k, c in enumerate(at):
            S, i = picks[k]
            sm.assert_bytes(recs[c], _edge_models(S)[1][i], "in the batch, S %d packet %d" % (S, i))
        assert all(r.flags == pl.SR_DATA for r in recs)
        alone = [look(h, [items[c]], ch0=c)[0][0] for c in at]
        assert alone == [batch[c] for c in at]
        assert [bytes(r) for r in h.symrate_records()] == batch  # (the calls on one channel left the others alone)
        g = _handle(Ss)
        try:
            other, _, _ = look(g, items, stream=second.value)
        finally:
            g.close()
        assert other == batch
    finally:
        pl.load().hipStreamDestroy(second)
        h.close()


# ---- 3. formats ----------------------------------------------------------------------------------------------------------------------

def _int8_packets(seed, Ss, blocks, extra=0):
    return [np.clip(np.round(40.0 * _samples(S, S * b + extra, "signal", seed + i)), -128, 127).astype(np.int8) for i, (S, b) in enumerate(zip(Ss, blocks))]


def test_the_integer_and_half_formats_give_the_records_of_their_float_packets():
    Ss = (4, 5, 8, 33, 1024, 16, 100, 9)  # (1, 1, 1, 8, 64, 2, 16 and 2 lanes a block)
    vals = _int8_packets(11000, Ss, (2, 129, P + 1, P + H + 1, 3, 2 * P + 5, P + 3, 700), extra=1)
    h = _handle(Ss)
    try:
        want, recs, _ = look(h, [v.astype(F32) for v in vals])
        for i, r in enumerate(recs):
            sm.assert_bytes(r, sm.model_record(vals[i], Ss[i]), "int8 values, S %d" % Ss[i])
        for dt in (np.int16, np.int8, F16):
            got, _, _ = look(h, [v.astype(dt) for v in vals])
            assert got == want, dt
        # packets that start one and three samples behind a 128-byte boundary
        for dt in (F32, np.int16, np.int8, F16):
            for skew in (1, 3):
                assert look(h, [v.astype(dt) for v in vals], skew=skew)[0] == want, (dt, skew)
    finally:
        h.close()


# ---- 4. strides ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", (F32, np.int16, np.int8, F16))
def test_columns_of_a_frame_major_matrix(monkeypatch, capfd, dt):
    """twelve adjacent columns of a matrix 20 wide, ragged lengths around one piece, which the tile gather takes; then every third
    of them, which are no neighbours and are read where they lie: byte-identical to the contiguous packets of the same samples,
    the matrix unchanged (look() compares it)"""
    C = 12
    Ss = [(8, 5, 33)[c % 3] for c in range(C)]
    cols = [v.astype(dt) for v in _int8_packets(13000, Ss, [(P - 3, P + 2, 140, 2)[c % 4] + c for c in range(C)], extra=2)]
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    h = _handle(Ss)
    try:
        want, recs, _ = look(h, cols)
        assert all(r.flags == pl.SR_DATA for r in recs)
        got, _, lines = look(h, cols, place=[(0, 3 + c) for c in range(C)], widths={0: 20}, capfd=capfd)
        assert got == want
        assert [t["what"] for t in lines] == ["gather_tiles", "symrate_fold", "symrate_join"], lines  # (one group, one sample size)
        third = list(range(0, C, 3))
        g = _handle([Ss[c] for c in third])
        try:
            got3, _, lines = look(g, [cols[c] for c in third], place=[(0, 3 + c) for c in third], widths={0: 20}, capfd=capfd)
        finally:
            g.close()
        assert got3 == [want[c] for c in third]
        assert [t["what"] for t in lines] == ["symrate_fold", "symrate_join"], lines  # (read where they lie: no gather)
    finally:
        monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES")
        h.close()


# ---- 5. tunes ------------------------------------------------------------------------------------------------------------------------

def _untuned(b):
    """a record's bytes with PSK_SOFT_SR_TUNED cleared: a tuned look says so in its flags, everything else is the model packet's"""
    r = pl.Symrate.from_buffer_copy(b)
    r.flags &= ~pl.SR_TUNED
    return bytes(r)


def test_tuned_packets_give_the_records_of_their_model_packets():
    """a tuned packet of each format, contiguous, as a single column and as one of nine adjacent columns (gathered): its record is that of
    the untuned CF32 packet holding tune_model.apply of it, but for the TUNED flag; {0, 0} and tune == NULL are the untuned call"""
    dts = (F32, np.int16, np.int8, F16)
    C = 4 + 4 + 9
    Ss = [(8, 5, 33, 4)[c % 4] for c in range(C)]
    items = [v.astype(dts[c % 4] if c < 8 else np.int16)
             for c, v in enumerate(_int8_packets(15000, Ss, [(P + 30, 2 * P + 1, 55, P - 1)[c % 4] + c for c in range(C)], extra=1))]
    place = [None] * 4 + [(1 + c, 1) for c in range(4)] + [(0, 2 + c) for c in range(9)]
    widths = {0: 12, 1: 3, 2: 2, 3: 5, 4: 4}
    tunes = [((0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64), (tm.step_word(0.0031), tm.step_word(-0.012), (1 << 63) + 12345, 1)[c % 4])
             for c in range(C)]
    tunes[2] = tunes[6] = tunes[12] = (0, 0)
    model = [x.astype(F32) if t == (0, 0) else tm.apply(t[0], t[1], x) for x, t in zip(items, tunes)]
    h = _handle(Ss)
    try:
        want, _, _ = look(h, model)
        got, recs, _ = look(h, items, place=place, widths=widths, tunes=tunes)
        for c in range(C):
            assert recs[c].flags == pl.SR_DATA | (0 if tunes[c] == (0, 0) else pl.SR_TUNED), c
            assert _untuned(got[c]) == want[c], c
            sm.assert_bytes(recs[c], sm.model_record(items[c], Ss[c], tunes[c]), "tuned, channel %d" % c)
        plain, _, _ = look(h, items, place=place, widths=widths)
        zeros, _, _ = look(h, items, place=place, widths=widths, tunes=[(0, 0)] * C)
        assert plain == zeros and plain == look(h, [x.astype(F32) for x in items])[0]
    finally:
        h.close()


# ---- 6. non-finite samples -----------------------------------------------------------------------------------------------------------

def test_a_non_finite_sample_invalidates_the_blocks_the_definition_says():
    """S = 8, 16, 24, 33, 100, 200 and 1000 (1, 2, 4, 8, 16, 32 and 64 lanes a block), 40 blocks: a NaN or an inf in the first, a middle or the last sample of block 17 (its real or its
    imaginary part) takes block 17 out, in the last sample block 18 too (its first g reaches back); every block's last sample NaN:
    no block is valid, n_pairs all zero, a NaN derive.  Every record is the model's, byte for byte."""
    cases = []
    for S in (8, 16, 24, 33, 100, 200, 1000):
        for v in (np.nan, np.inf, -np.inf):
            for where, part, bad in (("first", 0, {17}), ("middle", 1, {17}), ("last", 0, {17, 18})):
                x = _samples(S, 40 * S + 3, "signal", 23000 + S)
                x[2 * (17 * S + dict(first=0, middle=S // 2, last=S - 1)[where]) + part] = v
                cases.append((S, x, bad, "%s %r" % (where, v)))
        x = _samples(S, 40 * S + 3, "signal", 23100 + S)
        x[2 * (S - 1) :: 2 * S] = np.nan
        cases.append((S, x, set(range(40)), "every block"))
        x = _samples(S, 40 * S + 3, "signal", 23200 + S)
        x[0], x[2 * (40 * S) + 1] = np.inf, np.nan  # (the packet's first sample; one behind the last block: not looked at)
        cases.append((S, x, {0}, "sample 0, and the tail"))
    h = _handle([S for S, _, _, _ in cases])
    try:
        _, recs, _ = look(h, [x for _, x, _, _ in cases])
        for r, (S, x, bad, what) in zip(recs, cases):
            ctx = "S %d, %s" % (S, what)
            ok = [m not in bad for m in range(40)]
            assert r.n_blocks == 40 and r.n_valid == 40 - len(bad), ctx
            assert list(r.n_pairs) == [sum(ok[m] and ok[m - L] for m in range(L, 40)) for L in sm.LAGS], ctx
            sm.assert_bytes(r, sm.model_record(x, S), ctx)
            sm.assert_close(pl.symrate_host(S, x), sm.model_record(x, S), ctx)
            d = pl.symrate_derive(r)
            sm.assert_derived(d, sm.derive(r), ctx)
            if len(bad) == 40:
                assert not any(r.n_pairs) and bytes(r)[96:384] == bytes(288) and d["lags_used"] == 0 and math.isnan(d["samples_per_symbol"]), ctx
            else:
                assert d["lags_used"] >= 1 and abs(d["samples_per_symbol"] / (1.04 * S) - 1) < 0.02, (ctx, d)
    finally:
        h.close()


# ---- 7. no side effects ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", (0, 1))
def test_looks_between_process_calls_change_nothing(oracle_mod, monkeypatch, capfd, deferred):
    """three process calls with PSK_SOFT_OPT_QUALITY and a carrier look in front of the third; a symbol-rate look in front of the
    second and one in front of the third (tuned, with a frame group and single columns, over the same channels): all four streams
    are bit for bit the oracle's; statistics, quality records, carrier-look records and state blobs byte for byte those of the run
    without the symbol-rate looks; and those looks launch the gather of their frame group, symrate_fold and symrate_join only"""
    from tests.test_gpu_cs16_schedules import _synth, assert_same, check_parity, device_run

    S, C, calls = 8, 12, 3
    props = [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=(100, 200)[c % 2], phaseAvg=(50, 10)[(c // 3) % 2],
                  differentialDecoding=int(c % 5 == 3)) for c in range(C)]
    lens = [[3000 + 160 * ((5 * c + 3 * k) % 7) for c in range(C)] for k in range(calls)]
    raw = _synth(27000, [p["constelationSize"] for p in props], S, [sum(lens[k][c] for k in range(calls)) for c in range(C)])
    streams = [x if c % 2 else np.clip(np.round(40.0 * x), -32768, 32767).astype(np.int16) for c, x in enumerate(raw)]
    data, at = [], [0] * C
    for k in range(calls):
        data.append([streams[c][2 * at[c] : 2 * (at[c] + lens[k][c])] for c in range(C)])
        at = [at[c] + lens[k][c] for c in range(C)]
    looked = [v.astype(np.int16) for v in _int8_packets(27500, [S] * C, [P + 5 * c for c in range(C)], extra=3)]
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
                if k == 2:
                    _acquire_look(hh, looked, place=place, widths={0: 11, 1: 3}, keep=keep)

            got = device_run(h, data, capfd if trace else None, before=before, sync_each=not deferred)[0]
            sr = bytes(h.symrate_records())
            for b in keep:
                h.device_free(b)
            del keep[:]
            return got, h.stats(), h.channel_stats(), bytes(h.quality_records()), bytes(h.acquire_records()), [h.export_state(c) for c in range(C)], sr
        finally:
            monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES", raising=False)
            h.close()

    ref = run(False, False)
    got = run(True, False)
    traced = run(True, True)
    for r in (got, traced):
        assert_same(r[0], ref[0], "with looks against without")
        assert r[1:6] == ref[1:6]
    assert ref[4] != bytes(224 * C)  # (the carrier look did leave its records)
    assert ref[6] == bytes(R_BYTES * C) and got[6] == traced[6] and got[6] != ref[6]
    want = b"".join(sm.record_bytes(sm.model_record(looked[c], S, tunes[c])) for c in range(C))
    assert got[6] == want
    assert len(look_lines) == 4 and not any(look_lines[:2])
    for lines in look_lines[2:]:
        assert [t["what"] for t in lines] == ["gather_tiles", "symrate_fold", "symrate_join"], lines
    check_parity(oracle_mod, got[0], lambda c: props[c], data, "looks between the calls")


# ---- 8. zero records and kept records ----------------------------------------------------------------------------------------------------

def test_zero_records_and_kept_records():
    Ss = [8, 4, 8, 3, 8, 8, 1024, 1025]
    xs = [_samples(8, 500 + c, "signal", 19000 + c) for c in range(8)]
    h = _handle(Ss)
    try:
        first, recs, _ = look(h, xs)
        # (samplesPerBaud 3 and 1025: outside the look's range; 1024: fewer than two blocks)
        assert [r.flags for r in recs] == [1, 1, 1, 0, 1, 1, 0, 0] and first[3] == first[6] == first[7] == bytes(R_BYTES)
        # channels 1 .. 5: no packet, real data, (3 again), fewer than two blocks, a packet
        items = [None, xs[2], xs[3], xs[4][: 2 * 15], xs[5][:400]]
        got, recs, _ = look(h, items, ch0=1, real=(1,))
        assert got[:4] == [bytes(R_BYTES)] * 4 and recs[4].flags == pl.SR_DATA and (recs[4].n_samples, recs[4].n_blocks) == (200, 25)
        now = [bytes(r) for r in h.symrate_records()]
        assert now[0] == first[0] and now[6:] == first[6:] and now[1:6] == got
        sm.assert_bytes(recs[4], sm.model_record(xs[5][:400], 8), "the rewritten record")
    finally:
        h.close()


def test_slot_ring_wraps_with_looks_in_flight_on_two_streams():
    """Nine looks back to back -- one more than two turns of the four-slot ring -- over channels [0, 6) and [2, 8) in turn, on the
    handle's stream and a second one in turn, nothing waited for until the records are read: every channel's record is the
    model's for the last look that covered it, and byte for byte that of the same looks with a wait after each."""
    C, K, S = 8, 9, 8
    spans = [(0, 6) if k % 2 == 0 else (2, 6) for k in range(K)]
    items = [[_samples(S, 2400 + 8 * c + k, "signal", 21000 + 16 * k + c) for c in range(lo, lo + n)] for k, (lo, n) in enumerate(spans)]
    last = {c: max(k for k, (lo, n) in enumerate(spans) if lo <= c < lo + n) for c in range(C)}
    second = _second_stream()

    def run(in_flight):
        h, keep = _handle([S] * C), []
        try:
            for k, (lo, n) in enumerate(spans):
                look(h, items[k], ch0=lo, stream=None if k % 2 == 0 else second.value, keep=keep if in_flight else None)
            return h.symrate_records()
        finally:
            for b in keep:
                h.device_free(b)
            h.close()

    try:
        flight, waited = run(True), run(False)
        for c in range(C):
            sm.assert_bytes(flight[c], sm.model_record(items[last[c]][c - spans[last[c]][0]], S), "channel %d, look %d" % (c, last[c]))
        assert bytes(flight) == bytes(waited)
    finally:
        pl.load().hipStreamDestroy(second)


# ---- 9. look, step, resample, demodulate -----------------------------------------------------------------------------------------------

def test_the_loop_the_look_is_for(oracle_mod):
    """QPSK and 8-PSK at 8.37 samples a symbol, samplesPerBaud 8 (the packets of tests/test_resample_control.py): symrate_device on
    the first 4096 samples, resample_step(step_ratio) into process_device_resampled on the whole packet; the streams are bit for
    bit the oracle's on psk_soft_resample_apply with that step, and the symbol count is within 2 of the count at the true step"""
    from tests.test_gpu_cs16_schedules import check_parity
    from tests.test_gpu_resample import Plan, Resampled
    from tests.test_gpu_strided import strided_run
    from tests.test_resample_control import _signal

    Ms, S, sps = (4, 8), 8, 8.37
    xs = [_signal(M, sps)[1] for M in Ms]
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=100, phaseAvg=50) for M in Ms]
    h = pl.Handle(len(Ms), device=0)
    try:
        h.configure(0, props)
        _, recs, _ = look(h, [x[: 2 * 4096] for x in xs])
        steps = []
        for M, r, x in zip(Ms, recs, xs):
            sm.assert_bytes(r, sm.model_record(x[: 2 * 4096], S), "M %d" % M)
            d = pl.symrate_derive(r)
            print("M %d: estimate %.6f samples a symbol (relative error %.2g), coherence %.3f, detector %d, %d lags" % (
                M, d["samples_per_symbol"], d["samples_per_symbol"] / sps - 1, d["coherence"], d["detector"], d["lags_used"]))
            assert abs(d["samples_per_symbol"] / sps - 1) <= 5e-4 and d["detector"] == 0
            steps.append(pl.resample_step(d["step_ratio"]))
        data = [xs]
        plan = Plan(data, steps, restart=[[True] * len(Ms)])
        got = strided_run(Resampled(h, plan), data, [None] * len(Ms), {})[0]
        for c, x in enumerate(xs):
            y, _ = pl.resample_apply((0, steps[c], pl.RS_RESTART), x)
            assert np.array_equal(y.view(np.uint32), plan.model[0][c].view(np.uint32))
            o = oracle_mod.OracleComponent()
            o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = S, Ms[c], 100, 50
            true = o.service(pl.resample_apply((0, pl.resample_step(sps / S), pl.RS_RESTART), x)[0], 0.01, sriChanged=True).soft.size // 2
            assert abs(got[c][0]["soft"].size // 2 - true) <= 2, (c, got[c][0]["soft"].size // 2, true)
        check_parity(oracle_mod, got, lambda c: props[c], plan.model, "look, step, resample, process")
    finally:
        h.close()
