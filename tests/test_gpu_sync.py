"""psk_soft_sync_device on the GPU: the fold and the join of psk_sync.hip and the records they leave.

Every record is held byte for byte to tests/sync_model.py AND to psk_soft_sync_host: window counts at the edges of the kernel's
lanes, waves and pieces at every word length, hits and bests spread over waves and pieces, non-finite symbols at the lane and piece
edges; the records' independence of the batch, the handle and the stream, with guard bytes around every row; the history across
calls, behind a refused call and through get / set; no side effect on the demodulator; and process_device followed by sync_device
on one stream with nothing between, on the stimulus of tests/test_sync_control.py, against the oracle."""
import ctypes
import time

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import sync_model as sm
from tests.test_sync_control import ORACLE_CASES, WORD_LENGTHS, _row, _word, oracle_run

pytestmark = pytest.mark.gpu

F32 = np.float32
P = sm.PIECE
GUARD, GUARD_BYTE = 1024, 0xA5
THR = 0.9


def _second_stream():
    s = ctypes.c_void_p()
    assert pl.load().hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0  # (non-blocking)
    return s


class Case:
    """one row of a call: its symbols, the slot of its word, threshold, flags, the history in front (None: as the handle has it)"""

    def __init__(self, name, x, slot, thr=THR, flags=0, hist=None):
        self.name, self.x, self.slot, self.thr, self.flags, self.hist = name, np.ascontiguousarray(x, F32), slot, thr, flags, hist


WORDS = {k: _word(L, 500 + L) for k, L in enumerate(WORD_LENGTHS)}  # slot k holds the word of WORD_LENGTHS[k]
SLOT_OF = {L: k for k, L in enumerate(WORD_LENGTHS)}
# a word of two points a quarter turn apart, for rows of one repeated symbol: the window at a planted word has m = 1, the one in
# front of it 1/2, the one behind it 0 -- hits exactly where the test puts them, as close as two symbols apart
COMB_SLOT = 6
WORDS[COMB_SLOT] = np.array([1, 0, 0, 1], F32)


def _handle(nch, **limits):
    h = pl.Handle(nch, device=0, **limits)
    for k, w in WORDS.items():
        h.sync_define(k, w)
    return h


def search(h, cases, ch0=0, stream=None, set_hist=True):
    """one sync_device call over `cases` (channel ch0 + i <- cases[i]; None: word 0, not searched).  Every row lies between GUARD
    bytes of GUARD_BYTE in one arena, odd rows 8 bytes past a 128-byte boundary; the arena must come back as it went up.
    Returns the records of the covered channels."""
    off, size = [], 0
    for i, c in enumerate(cases):
        start = -(-(size + GUARD) // 128) * 128 + (8 if i % 2 else 0)
        off.append(start)
        size = start + (c.x.nbytes if c is not None else 0)
    size += GUARD
    arena = np.full(size, GUARD_BYTE, np.uint8)
    ins = (pl.SyncIn * len(cases))()
    d = h.device_alloc(size)
    try:
        for i, c in enumerate(cases):
            if c is None:
                continue
            arena[off[i]: off[i] + c.x.nbytes] = c.x.view(np.uint8)
            ins[i] = pl.SyncIn(d + off[i], c.x.size // 2, c.slot + 1, c.flags, c.thr, 0)
            if set_hist and c.hist is not None:
                h.set_sync_history(ch0 + i, c.hist)
        h.upload(d, arena)
        h.sync_device(ch0, ins, stream)
        recs = h.sync_records(ch0, len(cases))
        back = h.download(d, (size,), np.uint8)
        assert back.tobytes() == arena.tobytes(), "the call wrote into a row or a guard"
    finally:
        h.device_free(d)
    return recs


_models = {}


def model_of(c):
    """(record, history behind) of a case by the model, held to the host definition -- computed once"""
    if c.name not in _models:
        rec, hist = sm.model_record(WORDS[c.slot], c.thr, c.x, c.flags, c.hist)
        host, hh = pl.sync_host(WORDS[c.slot], c.thr, c.x, c.flags, c.hist)
        sm.assert_same(host, rec, "host, " + c.name)
        assert hh.tobytes() == hist.tobytes()
        _models[c.name] = (rec, hist)
    return _models[c.name]


def check(h, cases, recs, ch0=0, history=True):
    for i, c in enumerate(cases):
        if c is None:
            assert bytes(recs[i]) == bytes(sm.RECORD_BYTES)
            continue
        rec, hist = model_of(c)
        sm.assert_same(recs[i], rec, c.name)
        if history:
            assert h.sync_history(ch0 + i).tobytes() == hist.tobytes(), c.name + ": history"


def _planted(n, L, seed, every=97, **kw):
    """a row of n symbols with the word of length L every `every` symbols from 11 on (the first possibly cut by the row's end)"""
    return _row(n, seed, WORDS[SLOT_OF[L]], at=tuple(range(11, max(n - L + 1, 12), max(every, L + 3))), **kw)


# ---- 1. window counts at the edges of the kernel ---------------------------------------------------------------------------------

COUNTS = (1, 63, 64, 65, P - 1, P, P + 1, 2 * P - 1, 2 * P + 1, 3 * P + 5)


def edge_cases(L):
    hist = _row(127, 40 + L, WORDS[SLOT_OF[L]], at=(127 - L // 2,))  # (the word straddles the row's start where the row goes on with it)
    out = []
    for w in COUNTS:
        # a continuing row has as many windows as symbols; a restarted one L - 1 fewer
        out.append(Case("edge L%d w%d cont" % (L, w), _planted(w, L, 1000 * L + w), SLOT_OF[L], hist=hist))
        out.append(Case("edge L%d w%d restart" % (L, w), _planted(w + L - 1, L, 2000 * L + w), SLOT_OF[L], flags=pl.SYNC_RESTART, hist=hist))
    if L > 1:
        # rows shorter than the word: windows only through the history; restarted: none at all (the history still moves)
        for n in sorted({1, L // 2, L - 1} - {0}):
            out.append(Case("short L%d n%d cont" % (L, n), _row(n, 3000 * L + n), SLOT_OF[L], thr=0.2, hist=hist))
            out.append(Case("short L%d n%d restart" % (L, n), _row(n, 4000 * L + n), SLOT_OF[L], flags=pl.SYNC_RESTART, hist=hist))
    return out


@pytest.mark.parametrize("L", WORD_LENGTHS)
def test_window_counts_at_the_edges_of_lanes_waves_and_pieces(L):
    cases = edge_cases(L)
    h = _handle(len(cases))
    try:
        recs = search(h, cases)
        check(h, cases, recs)
        for c, r in zip(cases, recs):
            n = c.x.size // 2
            assert r.n_windows == (max(0, n - L + 1) if c.flags else n) and r.flags == pl.SYNC_DATA and r.word_len == L, c.name
        assert sorted({int(r.n_windows) for r in recs} & set(COUNTS)) == sorted(COUNTS)
    finally:
        h.close()


# ---- 2. hits and bests over waves and pieces, non-finite symbols -----------------------------------------------------------------

def spread_cases():
    out = []
    w31 = WORDS[SLOT_OF[31]]
    run = P // 4  # (windows of a piece one wave owns)

    def hits_row(name, n, at, L=2):
        if L == 2:
            z = np.full(n, 0.8 - 0.3j)
            z[np.asarray(at) + 1] *= 1j
            x = np.empty(2 * n, F32)
            x[0::2], x[1::2] = z.real, z.imag
            out.append(Case(name, x, COMB_SLOT, thr=0.999, flags=pl.SYNC_RESTART))
            return
        x = _row(n, len(out) + 77, WORDS[SLOT_OF[L]], at=tuple(at), sigma=0.0)
        out.append(Case(name, x, SLOT_OF[L], thr=0.999, flags=pl.SYNC_RESTART))

    # more than 16 hits over three pieces: 6, 7 and 10
    hits_row("hits over three pieces", 3 * P + 50, [100 + 9 * i for i in range(6)] + [P + 5 + 9 * i for i in range(7)] + [2 * P + 1 + 9 * i for i in range(10)])
    # ... over the waves of one piece, the second wave with more than are left; in one turn of one wave; in the last wave only
    hits_row("hits over the waves", P + 10, [3, 60, 64, 200, run + 1] + [run + 70 + 5 * i for i in range(14)] + [3 * run + 7, 3 * run + 250])
    hits_row("hits in one turn", 400, [64 + 3 * i for i in range(21)])
    hits_row("hits in the last wave", P, [3 * run + 64 + 4 * i for i in range(18)])
    hits_row("exactly sixteen", 2 * P, [50 * i + 7 for i in range(16)], L=31)
    # equal bests: in two pieces, in two waves of a piece, in two lanes of a turn
    for name, half in (("two pieces", P + 100), ("two waves", run + 30), ("two lanes", 40)):
        x = _row(half, 90 + half, w31, at=(4,), sigma=0.1)
        out.append(Case("equal bests in " + name, np.concatenate([x, x, x[:62]]), SLOT_OF[31], thr=0.7, flags=pl.SYNC_RESTART))
    # a non-finite symbol at lane 0 / 63 of a turn, at the wave and piece edges, and in the part of the stage behind the windows
    for k, s in enumerate((0, 63, 64, 127, run - 1, run, P - 1, P, P + 63, 2 * P - 1, 2 * P, 2 * P + 29)):
        x = _planted(2 * P + 30, 31, 600 + k)
        x[2 * s + (k & 1)] = (np.nan, np.inf, -np.inf)[k % 3]
        out.append(Case("non-finite at %d" % s, x, SLOT_OF[31], flags=pl.SYNC_RESTART))
        hist = _row(127, 700 + k)
        hist[2 * (126 - k) + 1] = np.nan
        out.append(Case("non-finite in the history %d" % k, x[: 2 * (P + 5)], SLOT_OF[31], hist=hist))
    out.append(Case("all zeros", np.zeros(2 * (P + 40), F32), SLOT_OF[64], flags=pl.SYNC_RESTART))
    out.append(Case("huge", _planted(P + 40, 64, 5) * F32(3e19), SLOT_OF[64], flags=pl.SYNC_RESTART))
    out.append(Case("denormal energies", _planted(300, 64, 6) * F32(1e-22), SLOT_OF[64]))
    out.append(Case("threshold one", _planted(300, 64, 7, sigma=0.0), SLOT_OF[64], thr=1.0))
    return out


def test_hits_and_bests_over_waves_and_pieces_and_non_finite_symbols():
    cases = spread_cases()
    h = _handle(len(cases))
    try:
        recs = search(h, cases)
        check(h, cases, recs)
        by = {c.name: r for c, r in zip(cases, recs)}
        assert [by[k].n_hits for k in ("hits over three pieces", "hits over the waves", "hits in one turn", "hits in the last wave")] == [23, 21, 21, 18]
        assert [x.pos for x in by["hits over the waves"].hits] == [3, 60, 64, 200, P // 4 + 1] + [P // 4 + 70 + 5 * i for i in range(11)]
        assert by["exactly sixteen"].n_hits == 16 and by["exactly sixteen"].hits[15].pos == 757
        for name, half in (("two pieces", P + 100), ("two waves", P // 4 + 30), ("two lanes", 40)):
            r = by["equal bests in " + name]
            assert r.best.pos == 4 and [x.pos for x in r.hits[:2]] == [4, 4 + half] and bytes(r.hits[0])[8:] == bytes(r.hits[1])[8:], name
        assert by["all zeros"].n_valid == 0 and by["huge"].n_valid == 0 and bytes(by["huge"].best) == bytes(24)
        assert by["non-finite at 0"].n_valid == by["non-finite at 0"].n_windows - 1
        assert by["non-finite at %d" % P].n_valid == by["non-finite at %d" % P].n_windows - 31
    finally:
        h.close()


# ---- 3. ordering and independence -----------------------------------------------------------------------------------------------

def test_a_record_does_not_depend_on_the_batch_the_handle_or_the_stream():
    """six rows alone, in one call; then among 70 rows of other lengths, words and thresholds (and channels that are not
    searched), on a second fresh handle on a non-default stream: byte-identical records, the model's"""
    mine = [c for L in (2, 31, 128) for c in edge_cases(L) if " w%d " % (2 * P + 1) in c.name or " w65 " in c.name][:6]
    assert len(mine) == 6
    others = [Case("other %d" % k, _planted(17 + 53 * k, WORD_LENGTHS[k % 6], 9000 + k), k % 6, thr=(0.3, 0.9, 0.6)[k % 3],
                   flags=(0, pl.SYNC_RESTART)[k % 2]) for k in range(70)]
    h = _handle(6)
    try:
        alone = search(h, mine)
        check(h, mine, alone)
    finally:
        h.close()
    batch, where = [], []
    for k, c in enumerate(others):
        batch.append(c if k % 9 else None)
        if k % 12 == 5 and len(where) < 6:
            where.append(len(batch))
            batch.append(mine[len(where) - 1])
    assert len(where) == 6
    second = _second_stream()
    g = _handle(len(batch) + 3)
    try:
        recs = search(g, batch, ch0=3, stream=second.value)
        for k, i in enumerate(where):
            assert bytes(recs[i]) == bytes(alone[k]), mine[k].name
        check(g, batch, recs, ch0=3)
        assert bytes(g.sync_records(0, 3)) == bytes(3 * sm.RECORD_BYTES)  # (not covered: untouched)
    finally:
        g.close()
        pl.load().hipStreamDestroy(second)


def test_slot_ring_wraps_with_sync_calls_in_flight_on_two_streams():
    """Nine calls back to back -- one more than two turns of the four-slot ring -- over channels [0, 6) and [2, 8) in turn, on the
    handle's stream and a second one in turn, nothing waited for until the records are read: every channel's record and history
    are the model's for the whole sequence of calls that covered it, and byte for byte those of the same calls with a wait after
    each.  Rows of 1100 .. 1200 symbols are two pieces each (a row that continues has as many windows as symbols), so the rows of
    channels 1 and 6 have 1000 .. 1024 symbols: one piece."""
    C, K, L, slot = 8, 9, 16, 7
    word = _word(L, 516)
    spans = [(0, 6) if k % 2 == 0 else (2, 6) for k in range(K)]
    n_of = lambda k, c: 1000 + (5 * k + c) % 25 if c in (1, 6) else 1100 + (37 * k + 11 * c) % 101  # noqa: E731
    rows = [[_row(n_of(k, c), 31000 + 16 * k + c, word, at=(40 + 3 * c, n_of(k, c) - 5 - c)) for c in range(lo, lo + n)]
            for k, (lo, n) in enumerate(spans)]
    sizes = sorted({x.size // 2 for r in rows for x in r})
    assert sizes[0] <= P < 1100 <= sizes[-1] <= 1200
    off, size = [], 0
    for r in rows:
        off.append([])
        for x in r:
            off[-1].append(-(-size // 128) * 128)
            size = off[-1][-1] + x.nbytes
    arena = np.zeros(size, np.uint8)
    for r, o in zip(rows, off):
        for x, at in zip(r, o):
            arena[at: at + x.nbytes] = x.view(np.uint8)
    # the model: each channel's calls in order, the history carried from one to the next
    want, hist = [None] * C, [None] * C
    for k, (lo, n) in enumerate(spans):
        for i in range(n):
            want[lo + i], hist[lo + i] = sm.model_record(word, THR, rows[k][i], 0, hist[lo + i])
    second = _second_stream()

    def run(in_flight):
        h = _handle(C)
        d = h.device_alloc(size)
        try:
            h.sync_define(slot, word)
            h.upload(d, arena)
            for k, (lo, n) in enumerate(spans):
                ins = [pl.SyncIn(d + off[k][i], rows[k][i].size // 2, slot + 1, 0, THR, 0) for i in range(n)]
                h.sync_device(lo, ins, None if k % 2 == 0 else second.value)
                if not in_flight:
                    h.synchronize()
                    assert pl.load().hipStreamSynchronize(second) == 0
            recs = h.sync_records()
            return recs, [h.sync_history(c).tobytes() for c in range(C)]
        finally:
            h.device_free(d)
            h.close()

    try:
        (flight, flight_hist), (waited, waited_hist) = run(True), run(False)
        for c in range(C):
            sm.assert_same(flight[c], want[c], "channel %d" % c)
        assert bytes(flight) == bytes(waited)
        assert flight_hist == waited_hist and flight_hist == [x.tobytes() for x in hist]
    finally:
        pl.load().hipStreamDestroy(second)


# ---- 4. the history ---------------------------------------------------------------------------------------------------------------

def _abs_hits(rec, shift):
    assert rec.n_hits <= 16
    return [(p + shift, cr, ci, e, m) for p, cr, ci, e, m in sm.hits_of(rec) if p + shift >= 0]


def test_cuts_the_history_a_refused_call_and_set_history():
    L = 31
    slot = SLOT_OF[L]
    n = 2 * P + 300
    x = _row(n, 31, WORDS[slot], at=(60, 500, P - 10, P + 400, 2 * P + 100, n - L), sigma=0.1)
    whole = Case("whole", x, slot, thr=0.8, flags=pl.SYNC_RESTART)
    cuts2, cuts3 = (P - 3,), (20, P + 5)  # (a word lies across the first; the second's first row is shorter than the word)
    h = _handle(4)
    try:
        sym = lambda a, b: x[2 * a: 2 * b]  # noqa: E731
        rows = {1: [sym(0, cuts2[0]), sym(cuts2[0], n)], 2: [sym(0, cuts3[0]), sym(cuts3[0], cuts3[1]), sym(cuts3[1], n)]}
        starts = {1: [0, cuts2[0]], 2: [0, cuts3[0], cuts3[1]]}
        got = {1: [], 2: []}
        for k in range(3):
            cases = [whole if k == 0 else None]
            for ch in (1, 2):
                cases.append(Case("cut %d %d" % (ch, k), rows[ch][k], slot, thr=0.8, flags=pl.SYNC_RESTART if k == 0 else 0)
                             if k < len(rows[ch]) else None)
            recs = search(h, cases, set_hist=False)
            for ch in (1, 2):
                if cases[ch] is not None:
                    got[ch] += _abs_hits(recs[ch], starts[ch][k])
                    # the record is the model's on the history the calls before have left
                    at = starts[ch][k]
                    hist_in = None if k == 0 else np.concatenate([np.zeros(2 * 127, F32), x[: 2 * at]])[-254:]
                    sm.assert_same(recs[ch], sm.model_record(WORDS[slot], 0.8, rows[ch][k], cases[ch].flags, hist_in)[0], cases[ch].name)
            if k == 0:
                want = sm.hits_of(recs[0])
                sm.assert_same(recs[0], model_of(whole)[0], "whole")
                assert [p for p, *_ in want] == [60, 500, P - 10, P + 400, 2 * P + 100, n - L]
        assert got[1] == want and got[2] == want
        last = x[2 * (n - 127):]
        for ch in (0, 1, 2):
            assert h.sync_history(ch).tobytes() == last.tobytes(), ch
        assert h.sync_history(3).tobytes() == bytes(4 * 254)
        # a refused call -- a bad threshold on the last channel -- leaves records and histories as they were
        before = bytes(h.sync_records())
        d = h.device_alloc(8 * 400)
        try:
            h.upload(d, _row(400, 1))
            ins = [pl.SyncIn(d, 400, slot + 1, 0, 0.5, 0) for _ in range(4)]
            ins[3].threshold = 1.5
            with pytest.raises(pl.PskSoftError) as e:
                h.sync_device(0, ins)
            assert e.value.status == 1
            assert bytes(h.sync_records()) == before
            for ch in (0, 1, 2):
                assert h.sync_history(ch).tobytes() == last.tobytes(), ch
            # ... and the same call with the threshold mended goes through and moves all four
            ins[3].threshold = 0.5
            h.sync_device(0, ins)
            assert bytes(h.sync_records()) != before
            assert all(h.sync_history(ch).tobytes() == _row(400, 1)[2 * (400 - 127):].tobytes() for ch in range(4))
        finally:
            h.device_free(d)
        # set_history round trip: what is set is what is read, and what the next call searches
        hist = _row(127, 2, WORDS[slot], at=(127 - 12,))
        h.set_sync_history(3, hist)
        assert h.sync_history(3).tobytes() == hist.tobytes()
        c = Case("after set_history", _row(200, 3, WORDS[slot], at=(-12,)), slot, hist=hist)
        recs = search(h, [c], ch0=3, set_hist=False)
        check(h, [c], recs, ch0=3)
        assert recs[0].n_hits == 1 and recs[0].hits[0].pos == -12
    finally:
        h.close()


# ---- 5. the demodulator is left alone; process then sync on one stream -----------------------------------------------------------

class Rows:
    """device rows for process_device on `n` channels, kept for the life of the object"""

    def __init__(self, h, n, max_complex):
        self.h, self.n = h, n
        self.cap = -(-max(h.output_capacity(c, max_complex) for c in range(n)) // 16) * 16
        self.sizes = (8 * max_complex, 8 * self.cap, 6 * self.cap, 4 * self.cap, 2 * self.cap)
        self.bufs = [h.device_alloc(n * s + 256) for s in self.sizes]

    def call(self, packets, first, stream=None):
        """process_device over interleaved float32 packets (one per channel); nothing is waited for"""
        pk, out = (pl.Packet * self.n)(), (pl.Output * self.n)()
        for c, x in enumerate(packets):
            assert x.size // 2 <= self.sizes[0] // 8
            self.h.upload(self.bufs[0] + c * self.sizes[0], x)
            p, q = pk[c], out[c]
            p.data, p.n_floats, p.sri_xdelta, p.sri_mode, p.sriChanged, p.present, p.format = self.bufs[0] + c * self.sizes[0], x.size, 0.01, 1, int(first), 1, 0
            q.soft, q.bits, q.phase, q.sampleIndex = (self.bufs[k] + c * self.sizes[k] for k in (1, 2, 3, 4))
            q.cap_symbols = self.cap
        self.h.process_device(0, pk, out, stream)
        return out

    def fetch(self, out):
        self.h.synchronize()
        return [dict(soft=self.h.download(o.soft, (2 * int(o.n_symbols),), F32) if o.n_symbols else np.zeros(0, F32),
                     phase=self.h.download(o.phase, (int(o.n_symbols),), F32) if o.n_symbols else np.zeros(0, F32),
                     bits=self.h.download(o.bits, (int(o.n_bits),), np.int16) if o.n_bits else np.zeros(0, np.int16),
                     index=self.h.download(o.sampleIndex, (int(o.n_sampleIndex),), np.int16) if o.n_sampleIndex else np.zeros(0, np.int16))
                for o in out]

    def free(self):
        for b in self.bufs:
            self.h.device_free(b)


def _sync_after(h, out, thr, flags, stream=None):
    h.sync_device(0, [pl.SyncIn(o.soft, o.n_symbols, 1, flags, thr, 0) for o in out], stream)


def test_sync_calls_between_process_calls_change_nothing(oracle_mod):
    soft, w, starts, iq = oracle_run(oracle_mod, ORACLE_CASES[0])
    C, cuts = 3, (0, 8192, 20000, 30000)

    def run(with_sync):
        h = pl.Handle(C, device=0)
        rows = None
        try:
            h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=50, phaseAvg=50)
            h.sync_define(0, w)
            rows = Rows(h, C, 12000)
            got = []
            for k in range(3):
                out = rows.call([iq[2 * cuts[k]: 2 * cuts[k + 1]]] * C, k == 0)
                if with_sync:
                    _sync_after(h, out, 0.7, pl.SYNC_RESTART if k == 0 else 0)
                got.append([{key: v.tobytes() for key, v in r.items()} for r in rows.fetch(out)])
            return got, h.stats(), h.channel_stats(), [h.export_state(c) for c in range(C)], bytes(h.sync_records())
        finally:
            if rows:
                rows.free()
            h.close()

    ref, got = run(False), run(True)
    assert got[:4] == ref[:4]
    assert ref[4] == bytes(C * sm.RECORD_BYTES) and got[4] != ref[4]


@pytest.mark.parametrize("deferred", (0, 1))
def test_process_then_sync_on_one_stream_finds_every_frame(oracle_mod, deferred):
    """the QPSK sigma 0.1 stimulus in packets of 8192 samples: process_device, then sync_device on the same stream with nothing
    between; the hits, by absolute symbol count, are the frames the oracle's soft stream holds, with one rotation.  deferred: with
    PSK_SOFT_OPT_DEFERRED_JOIN, on a batch that mixes window classes (numAvg 50 and 200)."""
    case = ORACLE_CASES[0]
    M, WL = case[0], case[1]
    soft, w, starts, iq = oracle_run(oracle_mod, case)
    navg = (50, 200, 50, 200) if deferred else (50, 50)
    C = len(navg)
    want = {}
    for na in set(navg):
        if na == 50:
            ref_soft = soft
        else:
            o = oracle_mod.OracleComponent()
            o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = 8, M, na, 50
            ref_soft = oracle_mod.run_stream(o, iq, 0.01, packet_complex=8192)["soft"]
        rec, _ = pl.sync_host(w, 0.7, ref_soft, pl.SYNC_RESTART)
        assert rec.n_hits <= 16
        want[na] = (ref_soft, [h.pos for h in rec.hits[: rec.n_hits]], {pl.sync_derive(h, M, WL, pl.sync_word_energy(w))["rotation"] for h in rec.hits[: rec.n_hits]})
    assert want[50][1] == starts and len(want[50][2]) == 1
    stream = _second_stream() if deferred else None
    h = pl.Handle(C, device=0)
    rows = None
    try:
        h.configure(0, [dict(samplesPerBaud=8, constelationSize=M, numAvg=na, phaseAvg=50) for na in navg])
        h.set_option(pl.Handle.OPT_DEFERRED_JOIN, deferred)
        h.sync_define(0, w)
        rows = Rows(h, C, 8192)
        found, rots, softs, count = [[] for _ in range(C)], [set() for _ in range(C)], [[] for _ in range(C)], [0] * C
        n = iq.size // 2
        for k, at in enumerate(range(0, n, 8192)):
            out = rows.call([iq[2 * at: 2 * min(at + 8192, n)]] * C, k == 0, stream.value if stream else None)
            _sync_after(h, out, 0.7, pl.SYNC_RESTART if k == 0 else 0, stream.value if stream else None)
            recs = h.sync_records()
            got = rows.fetch(out)
            for c in range(C):
                assert recs[c].n_symbols == out[c].n_symbols and recs[c].n_hits <= 16
                for hit in recs[c].hits[: recs[c].n_hits]:
                    found[c].append(count[c] + hit.pos)
                    rots[c].add(pl.sync_derive(hit, M, WL, pl.sync_word_energy(w))["rotation"])
                count[c] += int(out[c].n_symbols)
                softs[c].append(got[c]["soft"])
        for c in range(C):
            ref_soft, frames, rot = want[navg[c]]
            assert np.concatenate(softs[c]).tobytes() == ref_soft.tobytes(), c  # (the rows searched are the oracle's, bit for bit)
            assert found[c] == frames and rots[c] == rot, c
    finally:
        if rows:
            rows.free()
        h.close()
        if stream:
            pl.load().hipStreamDestroy(stream)


# ---- 5a. workgroups that walk several pieces; rows of more than 64 pieces -----------------------------------------------------------

def _comb_row(n, at):
    """n copies of one symbol, turned by a quarter from at + 1 on for one symbol: the comb word hits at `at` and nowhere else"""
    z = np.full(n, 0.8 - 0.3j)
    z[np.asarray(at) + 1] *= 1j
    x = np.empty(2 * n, F32)
    x[0::2], x[1::2] = z.real, z.imag
    return x


def search_shared(h, rows, pick, set_hist=True):
    """one sync_device call over len(pick) channels that share the device rows of `rows`: channel i searches rows[pick[i]] (None:
    not searched).  The rows lie between guard bytes in one arena, as in search()."""
    off, size = [], 0
    for i, c in enumerate(rows):
        start = -(-(size + GUARD) // 128) * 128 + (8 if i % 2 else 0)
        off.append(start)
        size = start + c.x.nbytes
    size += GUARD
    arena = np.full(size, GUARD_BYTE, np.uint8)
    for o, c in zip(off, rows):
        arena[o: o + c.x.nbytes] = c.x.view(np.uint8)
    ins = (pl.SyncIn * len(pick))()
    d = h.device_alloc(size)
    try:
        for i, k in enumerate(pick):
            if k is None:
                continue
            c = rows[k]
            ins[i] = pl.SyncIn(d + off[k], c.x.size // 2, c.slot + 1, c.flags, c.thr, 0)
            if set_hist and c.hist is not None:
                h.set_sync_history(i, c.hist)
        h.upload(d, arena)
        h.sync_device(0, ins)
        recs = sm.as_np(h.sync_records(0, len(pick)))
        back = h.download(d, (size,), np.uint8)
        assert back.tobytes() == arena.tobytes(), "the call wrote into a row or a guard"
    finally:
        h.device_free(d)
    return recs


def test_two_thousand_channels_share_rows_of_one_to_five_pieces():
    """700 channels, then 2100 on the same handle -- three workgroups a channel, then one that walks all five pieces; the
    host's part0 runs over some 5000 partials and the scratch grows between the calls -- over six device rows of 1 .. 5 pieces,
    continued and restarted; every ninth channel is not searched.  Records and histories are the model's and the host's."""
    hist = _row(127, 77, WORDS[SLOT_OF[31]], at=(127 - 15,))
    hits4 = [-1, 5, 900, P + 1] + [2 * P + 40 + 2 * i for i in range(20)] + [3 * P + 3, 3 * P + 9]
    rows = [Case("shared comb 1", _comb_row(300, [7, 100]), COMB_SLOT, thr=0.999, flags=pl.SYNC_RESTART),
            Case("shared L31 2", _planted(P + 400, 31, 8101), SLOT_OF[31], hist=hist),
            Case("shared L128 3", _planted(2 * P + 127 + 60, 128, 8102), SLOT_OF[128], flags=pl.SYNC_RESTART),
            Case("shared comb 4", _comb_row(3 * P + 500, hits4), COMB_SLOT, thr=0.999, hist=np.tile(np.array([0.8, -0.3], F32), 127)),
            Case("shared L31 5", _planted(4 * P + 30 + 7, 31, 8104), SLOT_OF[31], flags=pl.SYNC_RESTART),
            Case("shared L128 2", _planted(P + 9, 128, 8105), SLOT_OF[128], hist=_row(127, 78, WORDS[SLOT_OF[128]], at=(127 - 64,)))]
    pieces = [len(sm.partials(WORDS[c.slot], c.thr, c.x, c.flags, c.hist)) for c in rows]
    assert pieces == [1, 2, 3, 4, 5, 2]
    models = [model_of(c) for c in rows]
    assert int(models[3][0]["n_hits"]) == 26 and models[3][0]["hits"]["pos"][0] == -1  # (the history's last symbol starts a word)
    h = _handle(2100, max_window_samples=16, max_phase_avg=1, max_packet_complex=64)
    try:
        for n in (700, 2100):
            pick = [None if i % 9 == 4 else (i * 5 + i // 6) % 6 for i in range(n)]
            assert {k for k in pick if k is not None} == set(range(6))
            before = [h.sync_history(i).tobytes() for i in range(n) if pick[i] is None]
            recs = search_shared(h, rows, pick)
            for i, k in enumerate(pick):
                if k is None:
                    assert recs[i].tobytes() == bytes(sm.RECORD_BYTES), i
                else:
                    assert recs[i].tobytes() == models[k][0].tobytes(), (n, i, rows[k].name)
                    assert h.sync_history(i).tobytes() == models[k][1].tobytes(), (n, i, rows[k].name)
            assert before == [h.sync_history(i).tobytes() for i in range(n) if pick[i] is None], "a channel that is not searched keeps its history"
    finally:
        h.close()


def test_a_row_of_131_pieces_alone_and_among_short_rows():
    """130 P + 5 windows -- the join takes three trips over the partials -- with ten hits in front of piece 64 and ten from it
    on: the 16th stored hit lies in the second trip.  Alone, then as channel 7 among 20 short rows: the same bytes."""
    at = [p * P + 33 for p in (0, 5, 11, 20, 31, 40, 47, 55, 60, 63)] + [64 * P + 2 * i for i in range(6)] + [p * P + 1 for p in (65, 100, 128, 130)]
    big = Case("131 pieces", _comb_row(130 * P + 6, at), COMB_SLOT, thr=0.999, flags=pl.SYNC_RESTART)
    rec, _ = model_of(big)
    assert int(rec["n_windows"]) == 130 * P + 5 and int(rec["n_hits"]) == 20 and [int(x) for x in rec["hits"]["pos"]] == at[:16]
    assert at[9] < 64 * P <= at[10] and int(rec["best"]["pos"]) == at[0]
    # (channel 0 goes on from the history the first call leaves there; the other channels of the fresh handle from zeros)
    short = [Case("short beside 131 %d" % k, _planted(40 + 31 * k, WORD_LENGTHS[k % 6], 8200 + k), k % 6, flags=(0, pl.SYNC_RESTART)[k % 2],
                  hist=model_of(big)[1] if k == 0 else None) for k in range(20)]
    h = _handle(21)
    try:
        alone = search(h, [big])
        check(h, [big], alone)
        batch = short[:7] + [big] + short[7:]
        recs = search(h, batch, set_hist=False)
        assert bytes(recs[7]) == bytes(alone[0])
        sm.assert_same(recs[7], rec, big.name)
        assert h.sync_history(7).tobytes() == model_of(big)[1].tobytes()
        check(h, batch, recs)
    finally:
        h.close()


# ---- 6. more channels than a grid dimension holds ---------------------------------------------------------------------------------

def test_sixty_six_thousand_channels_in_one_call():
    """one call of 66000 channels, rows of 40 symbols, L = 8: the second trip of the fold's and the join's channel loops"""
    C, n, L = 66000, 40, 8
    word = _word(L, 66)
    distinct = [_row(n, 6600 + k, word, at=(3 + k,)) for k in range(8)]
    t0 = time.time()
    h = pl.Handle(C, device=0, max_window_samples=16, max_phase_avg=1, max_packet_complex=64)
    print("creating the handle took %.2f s" % (time.time() - t0))
    try:
        h.sync_define(9, word)
        d = h.device_alloc(8 * 8 * n)
        try:
            h.upload(d, np.concatenate(distinct))
            ins = (pl.SyncIn * C)()
            for c in range(C):
                ins[c] = pl.SyncIn(d + 8 * n * (c % 8), n, 10, pl.SYNC_RESTART if c % 3 else 0, 0.8, 0)
            h.sync_device(0, ins)
            got = sm.as_np(h.sync_records())
        finally:
            h.device_free(d)
        assert len(got) == C
        ch = np.arange(C)
        for k in range(8):
            for restart in (0, 1):
                rec, _ = sm.model_record(word, 0.8, distinct[k], pl.SYNC_RESTART if restart else 0)
                sel = got[(ch % 8 == k) & ((ch % 3 != 0) == bool(restart))]
                assert len(sel) > 2000 and sel.tobytes() == rec.tobytes() * len(sel), (k, restart)
                assert 3 + k in [p for p, *_ in sm.hits_of(rec)]
    finally:
        h.close()
