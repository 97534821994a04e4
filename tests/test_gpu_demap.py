"""psk_soft_demap_device on the GPU: the fold and the join of psk_demap.hip, the values they write and the records they leave.

Every output is held byte for byte, every record member for member, to tests/demap_model.py AND to psk_soft_demap_host: both
output forms at every count around the kernel's lanes, waves and pieces and at every byte offset of an int8 output; frames across
two rows behind a process call and a sync call, with PSK_SOFT_DEMAP_FRONT for a frame found in front of a row; 70000 segments in
one call; segments of 130 pieces; non-finite symbols at the lane edges; the same bytes whatever the batch; two calls back to back;
PSK_SOFT_OPT_DEFERRED_JOIN; no side effect on the demodulator.  Every output buffer lies between 64 guard bytes of a poison
pattern, which must come back unchanged, as must the rows."""
import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import demap_model as dm
from tests import sync_model as sm
from tests.test_gpu_sync import Rows, _second_stream

pytestmark = pytest.mark.gpu

F32 = np.float32
P = dm.PIECE
GUARD, POISON = 64, 0xC3
GAIN = (0.9, 0.5)  # (what dm.noisy_row divides by)
SLOT = {2: 3, 4: 0, 8: 15}  # the slot of dm.odd_map(M)
GRAY_SLOT = {2: 4, 4: 5, 8: 6}  # ... and of the Gray map on sync_model.psk_points(M)


def gray_map(M):
    z = sm.psk_points(M, np.arange(M))
    p = np.empty(2 * M, F32)
    p[0::2], p[1::2] = z.real, z.imag
    return p, dm.gray_labels(M)


MAPS = {SLOT[M]: dm.odd_map(M) for M in (2, 4, 8)}
MAPS.update({GRAY_SLOT[M]: gray_map(M) for M in (2, 4, 8)})


def _handle(nch=1, **limits):
    h = pl.Handle(nch, device=0, **limits)
    for slot, (p, lab) in MAPS.items():
        h.demap_define(slot, p, lab)
    return h


class Seg:
    """one segment of a call: symbols [pos, pos + count) of row `row` against the map of `slot`, written `at` values into the
    output buffer `buf` (None: a buffer of its own) that starts `mis` bytes past a 16-byte boundary.  skip: None, or which of
    count / map / soft is zeroed.  front: the 254 floats in front of the row (with DEMAP_FRONT)."""

    def __init__(self, row, pos, count, slot, flags=0, gain=GAIN, scale=8.0, buf=None, at=0, mis=0, skip=None, channel=0, front=None):
        self.row, self.pos, self.count, self.slot, self.flags, self.gain, self.scale = row, pos, count, slot, flags, gain, scale
        self.buf, self.at, self.mis, self.skip, self.channel, self.front = buf, at, mis, skip, channel, front
        self.B = dm.bits_of(len(MAPS[slot][1]))
        self.item = 1 if flags & pl.DEMAP_I8 else 4

    def expect(self, rows):
        """(the bytes of its values, its record) by the model, held to the host definition"""
        p, lab = MAPS[self.slot]
        args = (p, lab, rows[self.row], self.pos, self.count, self.gain, self.scale, self.flags, self.front)
        out, rec = dm.model_segment(*args)
        hout, hrec = pl.demap_host(*args)
        assert hout.tobytes() == out.tobytes(), "host values"
        dm.assert_same(hrec, rec, "host record")
        return out.tobytes(), rec


def _arena(sizes, align, shift):
    """offsets of regions of `sizes` bytes, each between GUARD bytes, region i starting shift[i] bytes past an `align` boundary"""
    off, size = [], 0
    for n, s in zip(sizes, shift):
        start = -(-(size + GUARD) // align) * align + s
        off.append(start)
        size = start + n
    return off, size + GUARD


def demap(h, rows, segs, stream=None, expect=None, dev_rows=None, records=True):
    """One demap_device call.  rows: the host copies of the rows (interleaved float32); dev_rows: their device pointers if they are
    on the device already, else they go up in an arena of their own between guard bytes.  The output buffers lie between GUARD
    bytes of POISON; outputs, guards and rows must come back as the model says.  expect: [(bytes, record)] per segment that is not
    skipped, else Seg.expect.  Returns the records as numpy."""
    row_dev = None
    if dev_rows is None:
        roff, rsize = _arena([r.nbytes for r in rows], 128, [8 if i % 2 else 0 for i in range(len(rows))])
        row_arena = np.full(rsize, POISON, np.uint8)
        for o, r in zip(roff, rows):
            row_arena[o: o + r.nbytes] = r.view(np.uint8)
        row_dev = h.device_alloc(rsize)
        h.upload(row_dev, row_arena)
        dev_rows = [row_dev + o for o in roff]
    # the output buffers: one per name, as long as its segments reach
    bufs = {}
    for i, s in enumerate(segs):
        key = ("own", i) if s.buf is None else s.buf
        end = (s.at + s.count * s.B) * s.item
        mis, size = bufs.get(key, (s.mis, 0))
        assert mis == s.mis
        bufs[key] = (mis, max(size, end))
    keys = list(bufs)
    ooff, osize = _arena([bufs[k][1] for k in keys], 16, [bufs[k][0] for k in keys])
    where = dict(zip(keys, ooff))
    out_arena = np.full(osize, POISON, np.uint8)
    out_dev = h.device_alloc(osize)
    try:
        h.upload(out_dev, out_arena)
        ins = (pl.DemapIn * len(segs))()
        want_out, want_rec = out_arena.copy(), np.zeros(len(segs), dm.RECORD_DTYPE)
        k = 0
        for i, s in enumerate(segs):
            o = where[("own", i) if s.buf is None else s.buf] + s.at * s.item
            ins[i] = pl.DemapIn(dev_rows[s.row], rows[s.row].size // 2, s.pos, out_dev + o, s.count, s.channel, s.slot + 1, s.flags,
                                s.gain[0], s.gain[1], s.scale, 0)
            if s.skip:
                setattr(ins[i], s.skip, 0)
                continue
            b, rec = expect[k] if expect is not None else s.expect(rows)
            k += 1
            assert len(b) == s.count * s.B * s.item
            want_out[o: o + len(b)] = np.frombuffer(b, np.uint8)
            want_rec[i] = rec
        h.demap_device(ins, stream)
        recs = dm.as_np(h.demap_records(0, len(segs))) if records else None
        back = h.download(out_dev, (osize,), np.uint8)
        bad = np.flatnonzero(back != want_out)
        assert bad.size == 0, "outputs or their guards differ from byte %d on (%d bytes)" % (bad[0], bad.size)
        if row_dev is not None:
            assert h.download(row_dev, (rsize,), np.uint8).tobytes() == row_arena.tobytes(), "the call wrote into a row or its guard"
        if records:
            for i in np.flatnonzero([recs[i].tobytes() != want_rec[i].tobytes() for i in range(len(segs))]):
                dm.assert_same(recs[i: i + 1].tobytes(), want_rec[i], "segment %d" % i)
    finally:
        h.device_free(out_dev)
        if row_dev is not None:
            h.device_free(row_dev)
    return recs


# ---- 1. both output forms at every count and byte offset ---------------------------------------------------------------------------

COUNTS = (1, 63, 64, 65, 257, P - 1, P, P + 1, 3 * P + 5)


@pytest.mark.parametrize("M", (2, 4, 8))
def test_every_count_output_form_and_byte_offset(M):
    rows = [dm.noisy_row(M, 3 * P + 40, 900 + M)]
    segs = []
    for k, count in enumerate(COUNTS):
        segs.append(Seg(0, k % 3, count, SLOT[M], 0, scale=3.25))
        for mis in (0, 1, 2, 3):
            segs.append(Seg(0, (k + mis) % 5, count, SLOT[M], pl.DEMAP_I8, scale=40.0, mis=mis))
    h = _handle()
    try:
        recs = demap(h, rows, segs)
        assert [int(r["n_symbols"]) for r in recs[::5]] == list(COUNTS) and (recs["n_finite"] == recs["n_symbols"]).all()
        assert (recs["bits"] == dm.bits_of(M)).all() and set(recs["flags"].tolist()) == {pl.DEMAP_DATA, pl.DEMAP_DATA | pl.DEMAP_REC_I8}
        assert recs["n_clip"][1::5].sum() > 0 and (recs["n_clip"][0::5] == 0).all()
    finally:
        h.close()


# ---- 2. frames across rows, behind a process call and a sync call -----------------------------------------------------------------

def test_frames_across_two_rows_and_in_front_of_a_row():
    """8 channels, two process calls of 24000 samples (about 3000 symbols of 8-PSK) each into rows of their own, a sync call behind
    each, all on one stream -- the first row ends at symbol 2951, inside the word that starts at 2930 + 2 c --; then ONE demap call: every frame of 700 symbols behind a hit, as one segment, as two abutting
    segments where it ends in the second row, with PSK_SOFT_DEMAP_FRONT where the second sync call found it in front of its row"""
    M, WL, S, C, FRAME, NS = 8, 48, 8, 8, 700, 3000
    streams = [sm.framed_stream(M, S, WL, 500, 2 * NS + 10, 430 + 2 * c, 0.05, 50 + c) for c in range(C)]
    points, labels = MAPS[GRAY_SLOT[M]]
    stream = _second_stream()
    h = _handle(C)
    ra = rb = None
    try:
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=50, phaseAvg=50)
        for c in range(C):
            h.sync_define(c, streams[c][1])
        ra, rb = Rows(h, C, NS * S), Rows(h, C, NS * S)
        out_a = ra.call([iq[: 2 * NS * S] for iq, _, _ in streams], True, stream.value)
        h.sync_device(0, [pl.SyncIn(o.soft, o.n_symbols, c + 1, pl.SYNC_RESTART, 0.7, 0) for c, o in enumerate(out_a)], stream.value)
        hits_a = [list(r.hits[: r.n_hits]) for r in h.sync_records()]
        out_b = rb.call([iq[2 * NS * S: 4 * NS * S] for iq, _, _ in streams], False, stream.value)
        h.sync_device(0, [pl.SyncIn(o.soft, o.n_symbols, c + 1, 0, 0.7, 0) for c, o in enumerate(out_b)], stream.value)
        hits_b = [list(r.hits[: r.n_hits]) for r in h.sync_records()]
        soft_a, soft_b = [g["soft"] for g in ra.fetch(out_a)], [g["soft"] for g in rb.fetch(out_b)]
        rows, dev_rows, segs, frames = [], [], [], []
        kinds = set()
        for c in range(C):
            na, nb = soft_a[c].size // 2, soft_b[c].size // 2
            rows += [soft_a[c], soft_b[c]]
            dev_rows += [out_a[c].soft, out_b[c].soft]
            front = soft_a[c][2 * (na - 127):]
            assert h.sync_history(c).tobytes() == soft_b[c][2 * (nb - 127):].tobytes()
            Ew = pl.sync_word_energy(streams[c][1])
            for row, hits in ((0, hits_a[c]), (1, hits_b[c])):
                for k, hit in enumerate(hits):
                    start = hit.pos + (na if row else 0)  # in the concatenated stream
                    if start + FRAME > na + nb:
                        continue
                    gain = tuple(pl.demap_gain(pl.sync_derive(hit, M, WL, Ew), M))
                    flags = pl.DEMAP_I8 if (k + c) % 2 else 0
                    kw = dict(flags=flags, gain=gain, scale=12.0, buf=("frame", c, start), mis=(c + k) % 4 if flags else 0, channel=c)
                    if row == 0 and hit.pos + FRAME > na:
                        first = na - hit.pos
                        segs.append(Seg(2 * c, hit.pos, first, GRAY_SLOT[M], **kw))
                        segs.append(Seg(2 * c + 1, 0, FRAME - first, GRAY_SLOT[M], at=3 * first, **kw))
                        kinds.add("two rows")
                    elif hit.pos < 0:
                        kw["flags"] |= pl.DEMAP_FRONT
                        segs.append(Seg(2 * c + 1, hit.pos, FRAME, GRAY_SLOT[M], front=front, **kw))
                        kinds.add("front")
                    else:
                        segs.append(Seg(2 * c + row, hit.pos, FRAME, GRAY_SLOT[M], **kw))
                        kinds.add("one row")
                    whole = np.concatenate([soft_a[c], soft_b[c]])
                    frames.append((len(segs) - 1, dm.model_segment(points, labels, whole, start, FRAME, gain, 12.0, flags)[0].tobytes(), c, start))
        assert kinds == {"two rows", "front", "one row"} and len(frames) >= 9 * C
        # (demap() holds every segment to the model of its row; the frames below to the model of the concatenated stream)
        demap(h, rows, segs, stream.value, dev_rows=dev_rows)
        for last, want, c, start in frames:
            s = segs[last]
            got = Seg(s.row, s.pos, s.count, s.slot, s.flags, s.gain, s.scale, front=s.front).expect(rows)[0]
            if s.at:
                p = segs[last - 1]
                got = Seg(p.row, p.pos, p.count, p.slot, p.flags, p.gain, p.scale).expect(rows)[0] + got
            assert got == want, (c, start)
        # the signs are the bits that were sent
        data = sm.framed_symbols(M, WL, 500, 2 * NS + 10, 430, 50)[0]
        last, want, c, start = frames[0]
        v = np.frombuffer(want, np.int8 if segs[last].flags & pl.DEMAP_I8 else F32).reshape(-1, 3)
        sent = np.array([[(int(g) >> (2 - j)) & 1 for j in range(3)] for g in labels[data[start: start + FRAME]]])
        assert c == 0 and ((v < 0).astype(int) == sent).all()
    finally:
        for r in (ra, rb):
            if r:
                r.free()
        h.close()
        pl.load().hipStreamDestroy(stream)


def test_front_reads_zeros_behind_a_restart_and_the_history_otherwise():
    M = 4
    hist, row = dm.noisy_row(M, 127, 61), dm.noisy_row(M, 900, 62)
    h = _handle(3)
    d = None
    try:
        h.sync_define(0, row[:16])
        d = h.device_alloc(row.nbytes)
        h.upload(d, row)
        for flags, front in ((0, hist), (pl.SYNC_RESTART, None)):
            h.set_sync_history(2, hist)
            h.sync_device(2, [pl.SyncIn(d, 900, 1, flags, 0.9, 0)])
            segs = [Seg(0, pos, count, SLOT[M], fl | pl.DEMAP_FRONT, front=front, channel=2, mis=1 if fl else 0)
                    for pos, count in ((-127, 127), (-127, 600), (-1, 1), (-40, 900), (3, 50)) for fl in (0, pl.DEMAP_I8)]
            demap(h, [row], segs, dev_rows=[d])
        # FRONT on a channel the last sync call did not search is refused
        with pytest.raises(pl.PskSoftError):
            demap(h, [row], [Seg(0, -5, 10, SLOT[M], pl.DEMAP_FRONT, channel=1)], dev_rows=[d])
    finally:
        if d:
            h.device_free(d)
        h.close()


# ---- 3. many segments; long segments ----------------------------------------------------------------------------------------------

def test_seventy_thousand_segments_in_one_call():
    """the second trip of the segment loop: 70000 segments of 3 .. 40 symbols over 64 rows in a shuffled order, every seventh
    skipped (count 0: its out stays poison, its record zero); the model is vectorised here -- a segment of at most 64 symbols is
    lanes 0 .. 63 of one wave of one piece -- and held to Seg.expect on a sample"""
    M, N, NROW, RLEN = 8, 70000, 64, 2000
    rng = np.random.default_rng(11)
    rows = [dm.noisy_row(M, RLEN, 300 + r) for r in range(NROW)]
    points, labels = MAPS[SLOT[M]]
    terms = [dm.symbol_terms(points, labels, r.reshape(-1, 2), GAIN, 40.0) for r in rows]
    assert all(t[3].all() for t in terms)
    E, D, V = (np.stack([t[k] for t in terms]) for k in (0, 1, 2))
    I8 = np.stack([dm.to_i8(t[2].reshape(-1))[0].reshape(-1, 3) for t in terms])
    CL = (np.abs(np.rint(V)) > 127).sum(axis=2)
    count = rng.integers(3, 41, N)
    row = rng.integers(0, NROW, N)
    pos = (rng.random(N) * (RLEN - count)).astype(np.int64)
    form = rng.integers(0, 2, N)
    # lane l of segment i holds its symbol l, or 0.0; the tree over all segments at once
    lanes = np.arange(64)
    live_lane = lanes[None, :] < count[:, None]
    at = np.minimum(pos[:, None] + lanes[None, :], RLEN - 1)
    sums = []
    for T in (E, D):
        w = np.where(live_lane, T[row[:, None], at], F32(0)).astype(np.float64)
        off = 32
        while off:
            w = w + w[:, lanes ^ off]
            off //= 2
        sums.append(((w[:, 0] + 0.0) + 0.0) + 0.0)  # (the three waves without a symbol)
    clips = np.where(live_lane, CL[row[:, None], at], 0).sum(axis=1)
    segs, expect = [], []
    for i in range(N):
        flags = pl.DEMAP_I8 if form[i] else 0
        s = Seg(int(row[i]), int(pos[i]), int(count[i]), SLOT[M], flags, scale=40.0, mis=i % 4 if flags else 0, skip="count" if i % 7 == 3 else None)
        segs.append(s)
        if s.skip:
            continue
        rec = np.zeros((), dm.RECORD_DTYPE)
        rec["n_symbols"] = rec["n_finite"] = s.count
        rec["sum_e"], rec["sum_err"] = sums[0][i], sums[1][i]
        rec["n_clip"] = clips[i] if flags else 0
        rec["bits"], rec["flags"] = 3, pl.DEMAP_DATA | (pl.DEMAP_REC_I8 if flags else 0)
        out = (I8 if flags else V)[s.row, s.pos: s.pos + s.count]
        expect.append((np.ascontiguousarray(out).tobytes(), rec))
    live = [s for s in segs if not s.skip]
    for k in range(0, len(live), 997):
        b, rec = live[k].expect(rows)
        assert b == expect[k][0] and rec.tobytes() == expect[k][1].tobytes(), k
    h = _handle()
    try:
        recs = demap(h, rows, segs, expect=expect)
        assert (recs["n_symbols"][3::7] == 0).all() and recs[3::7].tobytes() == bytes(64 * len(recs[3::7]))
        with pytest.raises(pl.PskSoftError):
            h.demap_records(N - 1, 2)
    finally:
        h.close()


def test_two_segments_of_130_pieces():
    """the join's trips of 64 partials and workgroups that walk several pieces"""
    M, n = 4, 130 * P + 7
    rows = [dm.noisy_row(M, n + 9, 71)]
    segs = [Seg(0, 2, n, SLOT[M], 0, scale=2.0), Seg(0, 9, n, SLOT[M], pl.DEMAP_I8, scale=50.0, mis=3)]
    h = _handle()
    try:
        recs = demap(h, rows, segs)
        assert (recs["n_finite"] == n).all() and recs["n_clip"][1] > 0
    finally:
        h.close()


# ---- 4. non-finite symbols; the batch; back to back ---------------------------------------------------------------------------------

def test_non_finite_symbols_at_the_lane_edges():
    M, n = 8, P + 70  # (the last piece is short: 70 symbols, its last lane 69)
    x = dm.noisy_row(M, n, 81)
    where = (0, 63, 64, 255, 256, P - 1, P, P + 63, P + 64, n - 1)
    for k, s in enumerate(where):
        x[2 * s + (k & 1)] = (np.nan, np.inf, -np.inf)[k % 3]
    h = _handle()
    try:
        recs = demap(h, [x], [Seg(0, 0, n, SLOT[M], 0), Seg(0, 0, n, SLOT[M], pl.DEMAP_I8, mis=1, scale=30.0)])
        assert (recs["n_finite"] == n - len(where)).all() and (recs["n_nan"] == 3 * len(where)).all()
        assert np.isfinite(recs["sum_e"]).all() and np.isfinite(recs["sum_err"]).all()
    finally:
        h.close()


def test_the_same_bytes_alone_and_as_one_of_five_thousand():
    M = 8
    rows = [dm.noisy_row(M, 2 * P + 300, 91), dm.noisy_row(M, 700, 92)]
    mine = Seg(0, 11, 2 * P + 201, SLOT[M], pl.DEMAP_I8, scale=25.0, mis=3)
    rng = np.random.default_rng(5)
    others = [Seg(1, int(rng.integers(0, 300)), int(rng.integers(1, 400)), SLOT[(2, 4, 8)[k % 3]], pl.DEMAP_I8 * (k % 2), mis=k % 4 if k % 2 else 0)
              for k in range(4999)]
    cache = {}

    def expect(s):
        key = (s.row, s.pos, s.count, s.slot, s.flags)
        if key not in cache:
            cache[key] = s.expect(rows)
        return cache[key]

    h = _handle()
    try:
        alone = demap(h, rows, [mine])
        batch = others + [mine]
        recs = demap(h, rows, batch, expect=[expect(s) for s in batch])
        assert recs[4999].tobytes() == alone[0].tobytes()
    finally:
        h.close()


class Guarded:
    """regions of device memory for tests that enqueue their calls themselves: each of sizes[i] bytes between GUARD bytes of POISON,
    shift[i] bytes past a 16-byte boundary, in one arena; `fill` gives a region's first content (else POISON)"""

    def __init__(self, h, sizes, shift=None, fill=None):
        self.h = h
        self.off, self.size = _arena(sizes, 16, shift or [0] * len(sizes))
        self.arena = np.full(self.size, POISON, np.uint8)
        for i, content in (fill or {}).items():
            self.arena[self.off[i]: self.off[i] + content.nbytes] = content.view(np.uint8)
        self.dev = h.device_alloc(self.size)
        h.upload(self.dev, self.arena)

    def ptr(self, i, byte=0):
        return self.dev + self.off[i] + byte

    def check(self, written, what):
        """the whole arena is what went up but for `written`: {(region, byte offset): bytes}"""
        want = self.arena.copy()
        for (i, byte), b in written.items():
            want[self.off[i] + byte: self.off[i] + byte + len(b)] = np.frombuffer(b, np.uint8)
        back = self.h.download(self.dev, (self.size,), np.uint8)
        bad = np.flatnonzero(back != want)
        assert bad.size == 0, "%s: differs from byte %d on (%d bytes)" % (what, bad[0], bad.size)

    def free(self):
        self.h.device_free(self.dev)


def test_two_calls_back_to_back_on_one_stream():
    """no wait lies between the two calls: the second's records replace the first's, both calls' outputs are whole, every byte
    around them and the row are as they went up"""
    M = 4
    row = dm.noisy_row(M, 3000, 95)
    first = [Seg(0, 10 * k, 500 + k, SLOT[M], pl.DEMAP_I8 * (k % 2), mis=k % 4 if k % 2 else 0) for k in range(6)]
    second = [Seg(0, 7, 1500, SLOT[M], 0, scale=1.5), Seg(0, 900, 33, SLOT[M], pl.DEMAP_I8, mis=1)]
    stream = _second_stream()
    h = _handle()
    rows = outs = None
    try:
        rows = Guarded(h, [row.nbytes], fill={0: row})
        both = first + second
        outs = Guarded(h, [s.count * s.B * s.item for s in both], [s.mis for s in both])

        def ins_of(segs, k0):
            arr = (pl.DemapIn * len(segs))()
            for i, s in enumerate(segs):
                arr[i] = pl.DemapIn(rows.ptr(0), 3000, s.pos, outs.ptr(k0 + i), s.count, 0, s.slot + 1, s.flags, s.gain[0], s.gain[1], s.scale, 0)
            return arr

        h.demap_device(ins_of(first, 0), stream.value)
        h.demap_device(ins_of(second, len(first)), stream.value)
        recs = dm.as_np(h.demap_records(0, 2))
        with pytest.raises(pl.PskSoftError):
            h.demap_records(0, 3)
        want = [s.expect([row]) for s in both]
        outs.check({(k, 0): b for k, (b, _) in enumerate(want)}, "the outputs of the two calls and their guards")
        rows.check({}, "the row and its guards")
        for i in range(len(second)):
            dm.assert_same(recs[i: i + 1].tobytes(), want[len(first) + i][1], "second call, segment %d" % i)
    finally:
        for g in (rows, outs):
            if g:
                g.free()
        h.close()
        pl.load().hipStreamDestroy(stream)


def test_three_calls_on_two_streams_with_the_descriptors_growing():
    """3, 700 and 2 segments on stream A, stream B, stream A, no wait between them: the first call's slot holds 3 + 0 + 256
    descriptors, the second makes a slot and the handle's records grow, the third reuses a grown slot.  Segments of 1 .. 1500
    symbols (one or two pieces).  All three calls' outputs and guards are whole, the records are the third call's, and outputs and
    records are those of the same calls with a wait after each."""
    M = 4
    row = dm.noisy_row(M, 3000, 96)
    counts = [1, 1023, 1024, 1025, 1500] + [1 + (37 * k) % 90 for k in range(690)] + [P + 1 + 9 * k for k in range(5)]
    calls = [[Seg(0, 5 * k, 900 + 300 * k, SLOT[M], pl.DEMAP_I8 * (k % 2), mis=k % 4 if k % 2 else 0) for k in range(3)],
             [Seg(0, (11 * k) % 1400, n, SLOT[M], pl.DEMAP_I8 * (k % 2), mis=k % 4 if k % 2 else 0, scale=2.0 + k % 3) for k, n in enumerate(counts)],
             [Seg(0, 3, 1400, SLOT[M], 0, scale=1.5), Seg(0, 2000, 77, SLOT[M], pl.DEMAP_I8, mis=3)]]
    assert [len(c) for c in calls] == [3, 700, 2] and min(counts) == 1 and max(counts) == 1500
    every = [s for c in calls for s in c]
    want = [s.expect([row]) for s in every]
    a, b = _second_stream(), _second_stream()

    def run(in_flight):
        h = _handle()
        rows = outs = None
        try:
            rows = Guarded(h, [row.nbytes], fill={0: row})
            outs = Guarded(h, [s.count * s.B * s.item for s in every], [s.mis for s in every])
            k0 = 0
            for segs, stream in zip(calls, (a, b, a)):
                arr = (pl.DemapIn * len(segs))()
                for i, s in enumerate(segs):
                    arr[i] = pl.DemapIn(rows.ptr(0), 3000, s.pos, outs.ptr(k0 + i), s.count, 0, s.slot + 1, s.flags, s.gain[0], s.gain[1], s.scale, 0)
                h.demap_device(arr, stream.value)
                if not in_flight:
                    h.synchronize()
                    assert pl.load().hipStreamSynchronize(stream) == 0
                k0 += len(segs)
            recs = bytes(h.demap_records(0, 2))
            with pytest.raises(pl.PskSoftError):
                h.demap_records(0, 3)
            outs.check({(k, 0): b_ for k, (b_, _) in enumerate(want)}, "the outputs of the three calls and their guards")
            rows.check({}, "the row and its guards")
            return recs, h.download(outs.dev, (outs.size,), np.uint8).tobytes()
        finally:
            for g in (rows, outs):
                if g:
                    g.free()
            h.close()

    try:
        flight, waited = run(True), run(False)
        for i in range(2):
            dm.assert_same(flight[0][64 * i: 64 * (i + 1)], want[703 + i][1], "third call, segment %d" % i)
        assert flight == waited
    finally:
        for s in (a, b):
            pl.load().hipStreamDestroy(s)


# ---- 5. deferred join; the demodulator is left alone ------------------------------------------------------------------------------

def _process_then_demap(deferred, stream, with_demap=True):
    """a process call over a batch that mixes window classes, directly followed by a demap call over its rows, its outputs between
    guard bytes; returns the soft rows and the LLRs (with_demap False: the process call alone, the rows)"""
    M, S, C, N = 4, 8, 4, 8192
    navg = (50, 200, 50, 200)
    iq = [sm.framed_stream(M, S, 32, 500, N // S + 8, 100, 0.1, 20 + c)[0][: 2 * N] for c in range(C)]
    h = _handle(C)
    rows = outs = None
    try:
        h.configure(0, [dict(samplesPerBaud=S, constelationSize=M, numAvg=na, phaseAvg=50) for na in navg])
        h.set_option(pl.Handle.OPT_DEFERRED_JOIN, deferred)
        rows = Rows(h, C, N)
        out = rows.call(iq, True, stream)
        if not with_demap:
            return [g["soft"].tobytes() for g in rows.fetch(out)], None
        outs = Guarded(h, [8 * int(o.n_symbols) for o in out])
        h.demap_device([pl.DemapIn(o.soft, o.n_symbols, 0, outs.ptr(c), int(o.n_symbols), 0, GRAY_SLOT[M] + 1, 0, 0.8, -0.6, 4.0, 0)
                        for c, o in enumerate(out)], stream)
        recs = h.demap_records(0, C)
        soft = [g["soft"] for g in rows.fetch(out)]
        llr = {}
        for c in range(C):
            want, rec = dm.model_segment(*MAPS[GRAY_SLOT[M]], soft[c], 0, soft[c].size // 2, (0.8, -0.6), 4.0, 0)
            llr[(c, 0)] = want.tobytes()
            dm.assert_same(recs[c], rec, "channel %d" % c)
        outs.check(llr, "the LLRs and their guards")
        return [s.tobytes() for s in soft], [llr[(c, 0)] for c in range(C)]
    finally:
        if outs:
            outs.free()
        if rows:
            rows.free()
        h.close()


def test_a_demap_call_directly_behind_a_deferred_process_call():
    stream = _second_stream()
    try:
        plain = _process_then_demap(0, stream.value)
        assert _process_then_demap(1, stream.value) == plain
        # the rows are what the process call leaves without a demap call behind it
        assert _process_then_demap(1, stream.value, with_demap=False)[0] == plain[0]
    finally:
        pl.load().hipStreamDestroy(stream)


def test_a_demap_call_touches_no_demodulator_state():
    M, S, C, N = 4, 8, 3, 8192
    iq = [sm.framed_stream(M, S, 32, 500, N // S + 8, 100, 0.1, 30 + c) for c in range(C)]
    h = _handle(C)
    rows = None
    try:
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=50, phaseAvg=50)
        h.sync_define(0, iq[0][1])
        rows = Rows(h, C, N)
        out = rows.call([x[0][: 2 * N] for x in iq], True)
        h.sync_device(0, [pl.SyncIn(o.soft, o.n_symbols, 1, 0, 0.7, 0) for o in out])

        def state():
            return ([h.peek(c) for c in range(C)], h.stats(), h.channel_stats(), [h.export_state(c) for c in range(C)], bytes(h.sync_records()),
                    [h.sync_history(c).tobytes() for c in range(C)])

        before = state()
        soft = [g["soft"] for g in rows.fetch(out)]
        segs = [Seg(c, -20 if c else 0, 400, GRAY_SLOT[M], pl.DEMAP_FRONT | (pl.DEMAP_I8 if c else 0), channel=c, front=np.zeros(254, F32))
                for c in range(C)]
        # (the channels' first sync call: the history it read is zeros)
        demap(h, soft, segs, dev_rows=[o.soft for o in out])
        assert state() == before
    finally:
        if rows:
            rows.free()
        h.close()
