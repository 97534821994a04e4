"""psk_soft_frame_search_device and psk_soft_frame_cut_device on the GPU (include/psk_soft_frame.h): the device against the host
definition and the numpy model of tests/frame_model.py byte for byte, records included.  Every buffer lies between guard bytes in
its arena; an arena is read back whole, so a byte written outside an output, or inside an input, fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import frame_cases as fc
from tests import frame_model as fm
from tests.test_gpu_sync import _second_stream

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xC3


class Arena:
    """regions of bytes in one device allocation, each between GUARD bytes of POISON, region i starting mis[i] bytes past a 16-byte
    boundary; `image` is what the arena must hold (the tests write the expected outputs into it).  tight: no guard behind the last
    region, which ends on the allocation's last byte."""

    def __init__(self):
        self.off, self.size, self.parts = [], 0, []

    def add(self, nbytes, mis=0, data=None):
        start = -(-(self.size + GUARD) // 16) * 16 + mis
        self.off.append(start)
        self.parts.append(None if data is None else np.ascontiguousarray(data, np.uint8))
        self.size = start + nbytes
        return len(self.off) - 1

    def up(self, h, tight=False):
        self.h = h
        self.image = np.full(self.size + (0 if tight else GUARD), POISON, np.uint8)
        for o, d in zip(self.off, self.parts):
            if d is not None:
                self.image[o : o + d.size] = d
        self.dev = h.device_alloc(self.image.size)
        h.upload(self.dev, self.image)
        return self

    def at(self, i):
        return self.dev + self.off[i]

    def expect(self, i, data):
        self.image[self.off[i] : self.off[i] + len(data)] = data

    def check(self, what=""):
        got = self.h.download(self.dev, (self.image.size,), np.uint8)
        bad = np.flatnonzero(got != self.image)
        assert not bad.size, "%s: %d bytes differ, the first at arena offset %d" % (what, bad.size, bad[0])

    def free(self):
        self.h.device_free(self.dev)


def _handle():
    return pl.Handle(1, device=0)


def _words(h, cases):
    """a slot per distinct word of the cases (at most 16 a handle): {(length, word, care): slot}"""
    slots = {}
    for c in cases:
        key = (c.length, c.word, c.care)
        if key not in slots:
            assert len(slots) < pl.FRAME_SLOTS
            slots[key] = len(slots)
            h.frame_word_define(slots[key], *key)
    return slots


def _search_in(c, addr, slot):
    return pl.FrameSearchIn(addr, c.bit0, c.n_bits, slot + 1, c.max_diff, c.period, 0, (ctypes.c_uint32 * 3)(0, 0, 0))


def _run_search(cases, mis_of, tight=False, check_model=True):
    """the cases in calls of at most 16 distinct words each, stream i of a call mis_of(i) bytes past a 16-byte boundary"""
    rng = np.random.default_rng(20)
    groups, cur, keys = [], [], set()
    for c in cases:
        k = (c.length, c.word, c.care)
        if k not in keys and len(keys) == pl.FRAME_SLOTS:
            groups.append(cur)
            cur, keys = [], set()
        keys.add(k)
        cur.append(c)
    groups.append(cur)
    for group in groups:
        h = _handle()
        arena = None
        try:
            slots = _words(h, group)
            arena = Arena()
            bufs = [c.packed(rng) for c in group]
            for i, b in enumerate(bufs):
                arena.add(b.size, mis_of(i), b)
            arena.up(h, tight)
            h.frame_search_device([_search_in(c, arena.at(i), slots[(c.length, c.word, c.care)]) for i, c in enumerate(group)])
            recs = h.frame_search_records(0, len(group))
            for i, c in enumerate(group):
                host = bytes(pl.frame_search_host(c.length, c.word, c.care, bufs[i], c.n_bits, c.bit0, c.max_diff, c.period))
                assert bytes(recs[i]) == host, "%s (stream %d, %d bytes past a boundary): the device against the host" % (c.label, i, mis_of(i))
                if check_model:
                    assert host == c.want.tobytes(), c.label
            arena.check("the streams are not written")
        finally:
            if arena:
                arena.free()
            h.close()


# ---- 1. the search ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mis", (0, 1, 2, 3))
def test_search_directed_cases_at_every_alignment(mis):
    """the directed list (every length class, care with holes, every bit0 mod 8, the ends of a stream, the periods, the ties, 0 / 16 / 17
    hits; windows of 33 .. 64 bits at a bit offset straddle three dwords) with every stream `mis` bytes past a 16-byte boundary"""
    _run_search(fc.search_cases(), lambda i: mis)


def test_search_across_tile_edges():
    tile = pl.load().psk_soft_frame_tile()
    _run_search(fc.tile_edge_cases(tile), lambda i: (i + 1) % 4)


def test_search_a_stream_that_ends_on_the_last_byte_of_its_allocation():
    rng = np.random.default_rng(21)
    for L, tail_bits in ((64, 0), (32, 0), (8, 0), (64, 3)):
        for nbytes in (4096 - 1, 4096, 4096 + 1, 4096 + 2):
            bit0 = 5
            bits = rng.integers(0, 2, 8 * nbytes - bit0 - tail_bits).astype(np.uint8)
            word = 0x0123456789ABCDEF & fc.full(L)
            fc.plant(bits, len(bits) - L, L, word)
            fc.plant(bits, 0, L, word, inverted=True)
            c = fc.SearchCase("ends on the last byte: L=%d, %d bytes" % (L, nbytes), L, word, fc.full(L), bits, bit0, 0, 0)
            assert c.packed().size == nbytes
            _run_search([c], lambda i: 0, tight=True)


def test_search_more_streams_than_workgroups_and_skipped_streams():
    """66000 streams (the join has 65535 workgroups) over a few dozen small buffers; every seventh is skipped, by its word or by its
    pointer, and gets the zero record"""
    rng = np.random.default_rng(22)
    cases = [c for c in fc.search_cases() if c.n_bits <= 1000][:40]
    n = 66000
    h = _handle()
    arena = None
    try:
        keys = []
        for c in cases:
            k = (c.length, c.word, c.care)
            if k not in keys:
                keys.append(k)
        keys = keys[: pl.FRAME_SLOTS]
        cases = [c for c in cases if (c.length, c.word, c.care) in keys]
        slots = _words(h, cases)
        arena = Arena()
        bufs = [c.packed(rng) for c in cases]
        for i, b in enumerate(bufs):
            arena.add(b.size, i % 4, b)
        arena.up(h)
        want = [bytes(host_search_buf(c, b)) for c, b in zip(cases, bufs)]
        ins = (pl.FrameSearchIn * n)()
        expect = []
        for i in range(n):
            j = (i * 7 + i // 64) % len(cases)
            c = cases[j]
            ins[i] = _search_in(c, arena.at(j), slots[(c.length, c.word, c.care)])
            if i % 7 == 3:
                if i % 2:
                    ins[i].word = 0
                else:
                    ins[i].bits = 0
                expect.append(bytes(192))
            else:
                expect.append(want[j])
        h.frame_search_device(ins)
        got = bytes(h.frame_search_records(0, n))
        assert len(got) == 192 * n
        if got != b"".join(expect):
            bad = [i for i in range(n) if got[192 * i : 192 * i + 192] != expect[i]]
            raise AssertionError("%d records differ, the first of stream %d" % (len(bad), bad[0]))
        # a range of the records
        assert bytes(h.frame_search_records(65530, 10)) == b"".join(expect[65530:65540])
        arena.check("the streams are not written")
    finally:
        if arena:
            arena.free()
        h.close()


def host_search_buf(c, buf):
    return pl.frame_search_host(c.length, c.word, c.care, buf, c.n_bits, c.bit0, c.max_diff, c.period)


# ---- 2. the cut ------------------------------------------------------------------------------------------------------------------------------

class CutCall:
    """frames of one handle: a format slot per distinct (branches, cell, table), an arena of streams and one of outputs"""

    def __init__(self, h, cases, in_mis, out_mis, abut=False, seed=30):
        rng = np.random.default_rng(seed)
        self.h, self.cases = h, cases
        self.slot = {}
        for c in cases:
            key = (c.branches, c.cell, None if c.table is None else c.table.tobytes())
            if key not in self.slot and key != (1, 0, None):
                assert len(self.slot) < pl.FRAME_SLOTS
                self.slot[key] = len(self.slot)
                h.frame_format_define(self.slot[key], c.branches, c.cell, c.table)
        self.bufs = [c.packed(rng) for c in cases]
        self.ins_arena, self.outs = Arena(), Arena()
        for i, (c, b) in enumerate(zip(cases, self.bufs)):
            self.ins_arena.add(b.size, in_mis(i), b)
        if abut:  # every output starts where the one before it ends
            self.out_off = np.concatenate([[0], np.cumsum([c.n_bytes for c in cases])])
            self.outs.add(int(self.out_off[-1]), out_mis(0))
        else:
            for i, c in enumerate(cases):
                self.outs.add(c.n_bytes, out_mis(i))
        self.ins_arena.up(h)
        self.outs.up(h)
        self.abut = abut

    def out_at(self, i):
        return self.outs.at(0) + int(self.out_off[i]) if self.abut else self.outs.at(i)

    def frame(self, i):
        c = self.cases[i]
        key = (c.branches, c.cell, None if c.table is None else c.table.tobytes())
        return pl.FrameCutIn(self.ins_arena.at(i), c.bit, self.out_at(i), c.n_bytes, 0 if key == (1, 0, None) else self.slot[key] + 1,
                             c.branch0, c.flags, (ctypes.c_uint32 * 2)(0, 0))

    def enqueue(self, lo=0, hi=None, stream=None):
        hi = len(self.cases) if hi is None else hi
        self.h.frame_cut_device((pl.FrameCutIn * (hi - lo))(*[self.frame(i) for i in range(lo, hi)]), stream)
        self.want_rec = []
        for i in range(lo, hi):
            out, rec = host_cut_buf(self.cases[i], self.bufs[i])
            if self.abut:
                self.outs.image[self.outs.off[0] + int(self.out_off[i]) : self.outs.off[0] + int(self.out_off[i + 1])] = out
            else:
                self.outs.expect(i, out)
            self.want_rec.append(bytes(rec))

    def check(self, what=""):
        n = len(self.want_rec)
        got = bytes(self.h.frame_cut_records(0, n))
        if got != b"".join(self.want_rec):
            bad = [i for i in range(n) if got[32 * i : 32 * i + 32] != self.want_rec[i]]
            raise AssertionError("%s: %d records differ, the first of frame %d" % (what, len(bad), bad[0]))
        self.outs.check(what + ": the outputs and their guards")
        self.ins_arena.check(what + ": the streams are not written")

    def free(self):
        self.ins_arena.free()
        self.outs.free()


def host_cut_buf(c, buf):
    return pl.frame_cut_host(c.branches, c.cell, buf, c.bit, c.n_bytes, c.branch0, c.table, c.flags)


def _cut(cases, in_mis, out_mis, abut=False, model=True, what=""):
    h = _handle()
    call = None
    try:
        call = CutCall(h, cases, in_mis, out_mis, abut)
        call.enqueue()
        call.check(what)
        if model:
            for i, c in enumerate(cases):
                out, rec = host_cut_buf(c, call.bufs[i])
                assert out.tobytes() == c.want[0].tobytes() and bytes(rec) == c.want[1].tobytes(), c.label
    finally:
        if call:
            call.free()
        h.close()


def _small_cut_cases():
    """every bit offset x every output alignment x n_bytes 1 .. 9 and 204; the alignment of the stream turns with them"""
    table = np.random.default_rng(31).permutation(256).astype(np.uint8)
    cases, mis = [], []
    seed = 1000
    for bit in range(8):
        for out_mis in range(4):
            for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 204):
                seed += 1
                cases.append(fc.CutCase("bit=%d out+%d n=%d" % (bit, out_mis, n), 1, 0, n, bit + 8 * (n % 2), table=table if seed % 3 == 0 else None,
                                        flags=seed % 2, seed=seed))
                mis.append(out_mis)
    return cases, mis


def test_cut_every_bit_offset_output_alignment_and_small_length():
    cases, mis = _small_cut_cases()
    assert len(cases) == 320
    _cut(cases, lambda i: (i // 3) % 4, lambda i: mis[i], what="bit offsets x alignments x lengths")


def test_cut_frames_that_abut():
    cases, _ = _small_cut_cases()
    for first in range(4):
        _cut(cases[first::7], lambda i: i % 4, lambda i: first, abut=True, model=False, what="abutting outputs from +%d" % first)


def test_cut_the_directed_cases_with_every_interleaver_shape():
    cases = list(fc.cut_cases())
    _cut(cases, lambda i: i % 4, lambda i: (i // 4) % 4, what="the directed cases")
    _cut(cases[::-1], lambda i: (i + 1) % 4, lambda i: 3 - i % 4, abut=True, what="the directed cases, abutting")


def test_cut_more_frames_than_workgroups_and_skipped_frames():
    """66000 frames (the launch has 65535 workgroups) cut from a few dozen streams into one run of abutting outputs; every ninth is
    skipped and leaves its bytes as they were"""
    base = [c for c in fc.cut_cases() if c.n_bytes <= 40]
    n = 66000
    h = _handle()
    call = None
    try:
        call = CutCall(h, base, lambda i: i % 4, lambda i: 1)
        want = [host_cut_buf(c, b) for c, b in zip(base, call.bufs)]
        pick = [(5 * i + i // 100) % len(base) for i in range(n)]
        off = np.concatenate([[0], np.cumsum([base[j].n_bytes for j in pick])])
        outs = Arena()
        outs.add(int(off[-1]), 3)
        outs.up(h)
        ins = (pl.FrameCutIn * n)()
        recs = []
        for i, j in enumerate(pick):
            k = call.frame(j)
            k.out = outs.at(0) + int(off[i])
            if i % 9 == 4:
                k.bits = 0
                recs.append(bytes(32))
            else:
                outs.image[outs.off[0] + int(off[i]) : outs.off[0] + int(off[i + 1])] = want[j][0]
                recs.append(bytes(want[j][1]))
            ins[i] = k
        h.frame_cut_device(ins)
        got = bytes(h.frame_cut_records(0, n))
        if got != b"".join(recs):
            bad = [i for i in range(n) if got[32 * i : 32 * i + 32] != recs[i]]
            raise AssertionError("%d records differ, the first of frame %d" % (len(bad), bad[0]))
        outs.check("66000 frames")
        outs.free()
    finally:
        if call:
            call.free()
        h.close()


# ---- 3. calls in flight on two streams; a slot redefined between calls --------------------------------------------------------------------

def test_calls_in_flight_on_two_streams():
    """five search calls and five cut calls alternating between two streams with nothing waited for between them leave what the
    same calls leave one after the other"""
    scases = [c for c in fc.search_cases() if c.length in (32, 64) and c.care == fc.full(c.length)]
    ccases = list(fc.cut_cases())
    ssizes, csizes = (9, 1, 14, 3, 6), (30, 7, 20, 1, 13)
    assert len(scases) >= sum(ssizes) and len(ccases) >= sum(csizes)
    a, b = _second_stream(), _second_stream()

    def go(in_flight):
        rng = np.random.default_rng(40)
        h = _handle()
        arena = call = None
        try:
            slots = _words(h, scases)
            arena = Arena()
            bufs = [c.packed(rng) for c in scases]
            for i, buf in enumerate(bufs):
                arena.add(buf.size, i % 4, buf)
            arena.up(h)
            call = CutCall(h, ccases, lambda i: i % 4, lambda i: (i + 2) % 4)
            slo = clo = 0
            for sn, cn, stream in zip(ssizes, csizes, (a, b, a, b, a)):
                h.frame_search_device([_search_in(c, arena.at(slo + i), slots[(c.length, c.word, c.care)])
                                       for i, c in enumerate(scases[slo : slo + sn])], stream.value)
                call.enqueue(clo, clo + cn, stream.value)
                if not in_flight:
                    h.synchronize()
                    assert pl.load().hipStreamSynchronize(stream) == 0
                slo, clo = slo + sn, clo + cn
            srec = bytes(h.frame_search_records(0, ssizes[-1]))
            want = b"".join(bytes(host_search_buf(c, buf)) for c, buf in zip(scases[slo - ssizes[-1] : slo], bufs[slo - ssizes[-1] : slo]))
            assert srec == want, "the last search call's records"
            call.check("five calls")  # (the outputs of all five, the records of the last)
            return srec, bytes(h.frame_cut_records(0, csizes[-1])), h.download(call.outs.dev, (call.outs.image.size,), np.uint8).tobytes()
        finally:
            if arena:
                arena.free()
            if call:
                call.free()
            h.close()

    try:
        assert go(True) == go(False)
    finally:
        for s in (a, b):
            pl.load().hipStreamDestroy(s)


def test_a_slot_redefined_between_two_calls():
    rng = np.random.default_rng(41)
    stream = _second_stream()
    h = _handle()
    arena = first = second = None
    try:
        # the search: slot 0 is one word, then another
        old = [c for c in fc.search_cases() if c.label.startswith("bit0=") and c.length == 64]
        new = [c for c in fc.search_cases() if c.label.startswith("bit0=") and c.length == 32]
        arena = Arena()
        bufs = [c.packed(rng) for c in old + new]
        for i, buf in enumerate(bufs):
            arena.add(buf.size, i % 4, buf)
        arena.up(h)
        h.frame_word_define(0, old[0].length, old[0].word, old[0].care)
        h.frame_search_device([_search_in(c, arena.at(i), 0) for i, c in enumerate(old)], stream.value)
        h.frame_word_define(0, new[0].length, new[0].word, new[0].care)  # (waits for the launch in front)
        h.frame_search_device([_search_in(c, arena.at(len(old) + i), 0) for i, c in enumerate(new)], stream.value)
        got = bytes(h.frame_search_records(0, len(new)))
        assert got == b"".join(c.want.tobytes() for c in new)
        # the cut: slot 0 is one table, then another interleaver and another table
        t1, t2 = rng.permutation(256).astype(np.uint8), rng.permutation(256).astype(np.uint8)
        before = [fc.CutCase("before %d" % i, 3, 5, 50 + i, i % 8, i % 3, t1, i % 2, seed=2000 + i) for i in range(12)]
        after = [fc.CutCase("after %d" % i, 2, 1, 50 + i, i % 8, i % 2, t2, i % 2, seed=2100 + i) for i in range(12)]
        first = CutCall(h, before, lambda i: i % 4, lambda i: 3 - i % 4)
        first.enqueue(stream=stream.value)
        second = CutCall(h, after, lambda i: i % 4, lambda i: i % 4)  # (defines slot 0 again: waits for the launch that reads it)
        assert first.slot == {(3, 5, t1.tobytes()): 0} and second.slot == {(2, 1, t2.tobytes()): 0}
        second.enqueue(stream=stream.value)
        second.check("behind the redefinition")
        first.outs.check("the call in front of the redefinition")
    finally:
        for c in (arena, first, second):
            if c:
                c.free()
        h.close()
        pl.load().hipStreamDestroy(stream)


# ---- 4. the chain: viterbi -> search -> (the only wait) -> cut -> rs on one stream -------------------------------------------------------

def test_viterbi_search_cut_rs_on_one_stream():
    """rs_encode_host (DVB) -> the model's interleaver -> 13 junk bits -> viterbi_encode -> LLRs +-16 with a fixed set of signs flipped;
    then viterbi_device (PACKED), frame_search_device and the only wait, for the search record; then frame_cut_device and rs_device with
    no wait between them.  The bytes are the data that was encoded and the rs records show the corrections.
    (tests/test_frame_control.py holds the stream to its premise: the decoder returns the sent bits outside the unterminated tail.)"""
    ch = fc.chain()
    F, T = fc.CHAIN_PACKETS, ch["n_steps"]
    good = T - 8 * fc.CHAIN_TAIL_BYTES
    stream = _second_stream()
    h = _handle()
    h.viterbi_define(0, ch["K"], ch["g"])
    h.frame_word_define(0, 8, 0x47)
    h.frame_format_define(0, fm.DVB_B, fm.DVB_M)
    h.rs_define(0, *pl.RS_DVB, depth=1)
    llrs = mid = pkts = outs = None
    try:
        llrs, mid, pkts, outs = Arena(), Arena(), Arena(), Arena()
        llrs.add(ch["llr"].size, 1, ch["llr"].view(np.uint8))
        mid.add((T + 7) // 8, 3)
        for q in range(F):
            pkts.add(204, q % 4)
            outs.add(188, (q + 1) % 4)
        for a in (llrs, mid, pkts, outs):
            a.up(h)
        h.viterbi_device([pl.ViterbiIn(llrs.at(0), mid.at(0), T, 1, pl.VITERBI_PACKED, 0)], stream.value)
        h.frame_search_device([(mid.at(0), 0, good, 1, 0, fm.DVB_PERIOD)], stream.value)
        rec = h.frame_search_records(0, 1)[0]  # the only wait
        assert (rec.best_phase, rec.best_score, rec.best_inv) == (fc.CHAIN_JUNK_BITS, F, F // 8)
        assert rec.listed == [(13 + fm.DVB_PERIOD * k, 0, 1 if k % 8 == 0 else 0) for k in range(16)]
        h.frame_cut_device([(mid.at(0), rec.best_phase + fm.DVB_PERIOD * q, pkts.at(q), 204, 1, 0) for q in range(F)], stream.value)
        h.rs_device([(pkts.at(q), outs.at(q), 1, 0) for q in range(F)], stream.value)
        rs = h.get_rs(0, F)
        cuts = h.frame_cut_records(0, F)
        for q in range(F):
            assert rs[q].n_err[0] == ch["errors"][q] and rs[q].failed == 0, "packet %d" % q
            assert cuts[q].n_ones == int(np.unpackbits(ch["packets"][q]).sum()) and cuts[q].span == fm.span(fm.DVB_B, fm.DVB_M, 0, 204)
            pkts.expect(q, ch["packets"][q])
            outs.expect(q, ch["data"][q])
        pkts.check("the packets")
        outs.check("the data")
        llrs.check("the LLRs are not written")
        packed = h.download(mid.at(0), ((T + 7) // 8,), np.uint8)
        assert np.array_equal(np.unpackbits(packed)[:good], ch["sent"][:good])
        assert bytes(rec) == bytes(pl.frame_search_host(8, 0x47, 0xFF, packed, good, 0, 0, fm.DVB_PERIOD))
    finally:
        for a in (llrs, mid, pkts, outs):
            if a is not None and hasattr(a, "dev"):
                a.free()
        h.close()
        pl.load().hipStreamDestroy(stream)
