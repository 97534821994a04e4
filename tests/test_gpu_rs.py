"""psk_soft_rs_device on the GPU: every input and every output lies between guard bytes; outputs, records, guards and inputs are
compared byte for byte with the host definition (psk_soft_rs_host), which tests/test_rs_control.py holds to tests/rs_model.py.
The shapes are the smallest at which the kernel can go wrong: codewords around the 64 lanes of a wave (n = nroots + 1, 63, 64, 65,
128, 129, 192, 193, 255), nroots 2, 3, 16, 32, 33 and 64, every depth, frames and outputs at every byte offset, every directed
error case of the control test, clean, corrected and failed codewords in one frame and in one call, two codes in one call, a slot
redefined between calls, skipped frames, more frames than the grid holds, calls in flight on two streams, and the chain
viterbi -> rs on one stream."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import rs_model as rm
from tests import viterbi_model as vm
from tests.test_gpu_sync import _second_stream

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xC3
IN_DTYPE = np.dtype([("in", "<u8"), ("out", "<u8"), ("code", "<u4"), ("flags", "<u4"), ("pad", "<u4", 2)])


def _handle(codes):
    """a handle with codes[i] (rm.Code) in slot i"""
    assert len(codes) <= pl.RS_SLOTS
    h = pl.Handle(1, device=0)
    for slot, c in enumerate(codes):
        h.rs_define(slot, *c.args, mask=c.mask)
    return h


def _arena(sizes, shift):
    """offsets of regions of `sizes` bytes, each between GUARD bytes, region i starting shift[i] bytes past a 16-byte boundary"""
    off, size = [], 0
    for n, s in zip(sizes, shift):
        start = -(-(size + GUARD) // 16) * 16 + s
        off.append(start)
        size = start + n
    return off, size + GUARD


class Frame:
    """one frame of a call: its code (rm.Code), its n * depth bytes and flags; the frame starts in_mis bytes and the output out_mis
    bytes past a 16-byte boundary.  skip: None, or which of code / in_ is zeroed."""

    def __init__(self, code, data, flags=0, in_mis=0, out_mis=0, skip=None, label=""):
        self.code, self.data, self.flags = code, np.ascontiguousarray(data, np.uint8), flags
        self.in_mis, self.out_mis, self.skip, self.label = in_mis, out_mis, skip, label
        assert self.data.size == code.n * code.depth
        self.out_bytes = (code.n if flags & rm.WITH_PARITY else code.k) * code.depth

    def expect(self):
        out, rec = pl.rs_host(*self.code.args, self.data, self.code.mask, self.flags)
        assert out.size == self.out_bytes
        return out, bytes(rec)


class Call:
    """the frames of one or more calls in device memory: one arena of frames and one of outputs, every region between GUARD bytes
    of POISON.  enqueue() sends a range of the frames as one rs_device call; check() holds both arenas to what the host definition
    says of every frame enqueued so far."""

    def __init__(self, h, codes, frames):
        self.h, self.frames = h, frames
        self.slot = {id(c): i for i, c in enumerate(codes)}
        self.ioff, isize = _arena([f.data.size for f in frames], [f.in_mis for f in frames])
        self.in_arena = np.full(isize, POISON, np.uint8)
        for o, f in zip(self.ioff, frames):
            self.in_arena[o: o + f.data.size] = f.data
        self.ooff, osize = _arena([f.out_bytes for f in frames], [f.out_mis for f in frames])
        self.want_out = np.full(osize, POISON, np.uint8)
        self.in_dev, self.out_dev = h.device_alloc(isize), h.device_alloc(osize)
        h.upload(self.in_dev, self.in_arena)
        h.upload(self.out_dev, self.want_out)
        self.want_rec = {}

    def enqueue(self, lo=0, hi=None, stream=None):
        hi = len(self.frames) if hi is None else hi
        ins = (pl.RsIn * (hi - lo))()
        for i in range(lo, hi):
            f = self.frames[i]
            k = ins[i - lo]
            k.in_, k.out, k.code, k.flags = self.in_dev + self.ioff[i], self.out_dev + self.ooff[i], self.slot[id(f.code)] + 1, f.flags
            if f.skip:
                setattr(k, f.skip, 0)
                self.want_rec[i] = bytes(64)
                continue
            out, rec = f.expect()
            self.want_out[self.ooff[i]: self.ooff[i] + out.size] = out
            self.want_rec[i] = rec
        self.h.rs_device(ins, stream)

    def check(self, lo=0, hi=None, what="the call"):
        """the records are those of the frames [lo, hi) -- the last call's --, the arenas those of every call so far"""
        hi = len(self.frames) if hi is None else hi
        recs = bytes(self.h.get_rs(0, hi - lo))
        with pytest.raises(pl.PskSoftError):
            self.h.get_rs(0, hi - lo + 1)
        back = self.h.download(self.out_dev, (self.want_out.size,), np.uint8)
        bad = np.flatnonzero(back != self.want_out)
        if bad.size:
            i = max(k for k in range(len(self.frames)) if self.ooff[k] - GUARD <= bad[0])
            f = self.frames[i]
            raise AssertionError("%s: outputs or their guards differ from byte %d on (%d bytes): frame %d (%s) at %d, %d bytes, code %s flags %d"
                                 % (what, bad[0], bad.size, i, f.label, self.ooff[i], f.out_bytes, f.code.args, f.flags))
        assert self.h.download(self.in_dev, (self.in_arena.size,), np.uint8).tobytes() == self.in_arena.tobytes(), what + ": the call wrote into frames or their guards"
        for i in range(lo, hi):
            got = recs[64 * (i - lo): 64 * (i - lo + 1)]
            if got != self.want_rec[i]:
                f = self.frames[i]
                raise AssertionError("%s: frame %d (%s, code %s flags %d): record %s, want %s"
                                     % (what, i, f.label, f.code.args, f.flags, np.frombuffer(got, rm.RECORD_DTYPE)[0], np.frombuffer(self.want_rec[i], rm.RECORD_DTYPE)[0]))

    def outcomes(self, lo=0, hi=None):
        """the kinds of codeword the frames [lo, hi) hold by the host definition: a set of 'clean', 'corrected', 'failed'"""
        hi = len(self.frames) if hi is None else hi
        kinds = set()
        for i in range(lo, hi):
            if self.frames[i].skip:
                continue
            r = np.frombuffer(self.want_rec[i], rm.RECORD_DTYPE)[0]
            for e in r["n_err"][: int(r["depth"])]:
                kinds.add("clean" if e == 0 else "failed" if e == rm.FAILED else "corrected")
        return kinds

    def free(self):
        self.h.device_free(self.in_dev)
        self.h.device_free(self.out_dev)


def run(codes, frames, what="the call"):
    h = _handle(codes)
    call = None
    try:
        call = Call(h, codes, frames)
        call.enqueue()
        call.check(what=what)
        return call.outcomes()
    finally:
        if call:
            call.free()
        h.close()


def mask_of(rng, n, depth, kind):
    """a mask of length 0, 1, n I - 1, n I or anything between"""
    size = (0, 1, n * depth - 1, n * depth, int(rng.integers(0, n * depth + 1)))[kind % 5]
    return rng.integers(0, 256, size).astype(np.uint8) if size else None


def enc(code, data):
    """the frame of the data by the library's host encoder (tests/test_rs_control.py holds it to the model's)"""
    return pl.rs_encode_host(*code.args, data, code.mask)


def directed_frames(rng, code, start=0):
    """the directed cases of tests/rs_model.py as frames, both flag values and the byte offsets 0 .. 3 (and 4 .. 7) going round"""
    frames = []
    for q, (label, data) in enumerate(rm.directed_cases(rng, code, lambda d: enc(code, d))):
        i = start + q
        frames.append(Frame(code, data, i % 2, in_mis=i % 8, out_mis=(i // 2 + i // 8) % 8, label=label))
    return frames


# ---- 1. every n and nroots, the directed cases, every byte offset ------------------------------------------------------------------------

LENGTHS = (None, 63, 64, 65, 128, 129, 192, 193, 255)  # None: nroots + 1 (k = 1)


def codes_of_nroots(nroots):
    rng = np.random.default_rng(nroots)
    codes = []
    for q, n in enumerate(LENGTHS):
        n = nroots + 1 if n is None else n
        if n <= nroots or any(c.n == n for c in codes):
            continue
        gfpoly = rm.PRIMITIVE_POLYS[(q + nroots) % len(rm.PRIMITIVE_POLYS)]
        prim = (1, 11, 2, 7, 254, 13, 4, 19, 8)[q]
        depth = 1 + (q + nroots) % 8
        codes.append(rm.Code(gfpoly, int(rng.integers(0, 255)), prim, nroots, n, depth, mask_of(rng, n, depth, q)))
    return rng, codes


@pytest.mark.parametrize("nroots", (2, 3, 16, 32, 33, 64))
def test_every_length_directed_case_and_byte_offset(nroots):
    """one call: codes of this nroots at every length around the wave's 64 lanes, depths going round 1 .. 8, masks of every kind of
    length, every directed error case on each, with and without parity, frames and outputs at every byte offset, a skipped frame
    of each kind between decoded ones"""
    rng, codes = codes_of_nroots(nroots)
    frames = []
    for c in codes:
        frames += directed_frames(rng, c, len(frames))
        frames.append(Frame(c, frames[-1].data, 1, in_mis=1, out_mis=3, skip=("code", "in_")[len(frames) % 2], label="skipped"))
    assert {f.in_mis for f in frames} == set(range(8)) == {f.out_mis for f in frames}
    kinds = run(codes, frames, "nroots %d" % nroots)
    assert kinds == {"clean", "corrected", "failed"}


@pytest.mark.parametrize("depth", range(1, 9))
def test_every_depth_of_the_two_standard_codes(depth):
    """CCSDS (255,223) and DVB (204,188) at this depth in one call -- two codes in one call --: the directed cases, then frames whose
    codewords are clean, corrected and failed side by side"""
    rng = np.random.default_rng(40 + depth)
    codes = [rm.Code(*rm.CCSDS, depth=depth, mask=mask_of(rng, 255, depth, depth)), rm.Code(*rm.DVB, depth=depth, mask=mask_of(rng, 204, depth, depth + 2))]
    frames = []
    for c in codes:
        frames += directed_frames(rng, c, len(frames))
    for q in range(6):
        c = codes[q % 2]
        data = enc(c, rng.integers(0, 256, c.k * depth).astype(np.uint8))
        for j in range(depth):
            rm.corrupt(rng, data, c, j, (0, c.t, c.t + 2, 1, c.t + 1, c.t - 1)[(q + j) % 6])
        frames.append(Frame(c, data, q % 2, in_mis=q % 4, out_mis=(q + 1) % 4, label="mixed"))
    kinds = run(codes, frames, "depth %d" % depth)
    assert kinds == {"clean", "corrected", "failed"}


def test_frames_that_abut_at_every_alignment():
    """frames of an odd length packed with no byte between them, and their outputs likewise: only the ends have guards; one call per
    alignment 0 .. 3 of the first frame and of the first output"""
    rng = np.random.default_rng(50)
    code = rm.Code(0x11D, 1, 1, 6, 37, 3, mask_of(rng, 37, 3, 2))  # 111 bytes in, 93 out
    F = 24
    datas = []
    for q in range(F):
        d = enc(code, rng.integers(0, 256, code.k * code.depth).astype(np.uint8))
        for j in range(code.depth):
            rm.corrupt(rng, d, code, j, (0, 1, 3, 4, 2)[(q + j) % 5])
        datas.append(d)
    exp = [pl.rs_host(*code.args, d, code.mask, 0) for d in datas]
    nin, nout = code.n * code.depth, code.k * code.depth
    h = _handle([code])
    bufs = []
    try:
        for mis in range(4):
            in_arena = np.full(GUARD + 16 + F * nin + GUARD, POISON, np.uint8)
            out_want = np.full(GUARD + 16 + F * nout + GUARD, POISON, np.uint8)
            i0, o0 = GUARD + mis, GUARD + (mis + 1) % 4
            for q in range(F):
                in_arena[i0 + q * nin: i0 + (q + 1) * nin] = datas[q]
            in_dev, out_dev = h.device_alloc(in_arena.size), h.device_alloc(out_want.size)
            bufs += [in_dev, out_dev]
            h.upload(in_dev, in_arena)
            h.upload(out_dev, out_want)
            for q in range(F):
                out_want[o0 + q * nout: o0 + (q + 1) * nout] = exp[q][0]
            h.rs_device([(in_dev + i0 + q * nin, out_dev + o0 + q * nout, 1, 0) for q in range(F)])
            recs = h.get_rs(0, F)
            assert h.download(out_dev, (out_want.size,), np.uint8).tobytes() == out_want.tobytes(), "alignment %d: outputs or guards" % mis
            assert h.download(in_dev, (in_arena.size,), np.uint8).tobytes() == in_arena.tobytes(), "alignment %d: inputs" % mis
            assert bytes(recs) == b"".join(bytes(e[1]) for e in exp), "alignment %d: records" % mis
    finally:
        for p in bufs:
            h.device_free(p)
        h.close()


# ---- 2. more frames than the grid holds ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nframe,code_args", ((70000, (0x11D, 0, 1, 2, 5, 1)), (9000, (0x187, 112, 11, 4, 21, 8))))
def test_more_frames_than_workgroups(nframe, code_args):
    """70 000 frames of a (5,3) code, and 9000 frames of depth 8 (72 000 codewords): 251 distinct frames -- clean, corrected, failed --
    go round, abutting; the host definition is computed once for each"""
    rng = np.random.default_rng(nframe)
    code = rm.Code(*code_args)
    D = 251
    nin, nout = code.n * code.depth, code.k * code.depth
    datas = np.zeros((D, nin), np.uint8)
    outs = np.zeros((D, nout), np.uint8)
    recs = np.zeros(D, rm.RECORD_DTYPE)
    for q in range(D):
        d = enc(code, rng.integers(0, 256, nout).astype(np.uint8))
        for j in range(code.depth):
            rm.corrupt(rng, d, code, j, (q + j) % (code.t + 2))
        datas[q] = d
        o, r = pl.rs_host(*code.args, d, None, 0)
        outs[q], recs[q] = o, np.frombuffer(bytes(r), rm.RECORD_DTYPE)[0]
    assert {0, 1, rm.FAILED} <= set(recs["n_err"][:, : code.depth].reshape(-1).tolist())
    idx = np.arange(nframe) % D
    in_arena = np.full(GUARD + nframe * nin + GUARD, POISON, np.uint8)
    in_arena[GUARD: GUARD + nframe * nin] = datas[idx].reshape(-1)
    out_want = np.full(GUARD + nframe * nout + GUARD, POISON, np.uint8)
    h = _handle([code])
    bufs = []
    try:
        in_dev, out_dev = h.device_alloc(in_arena.size), h.device_alloc(out_want.size)
        bufs += [in_dev, out_dev]
        h.upload(in_dev, in_arena)
        h.upload(out_dev, out_want)
        out_want[GUARD: GUARD + nframe * nout] = outs[idx].reshape(-1)
        ins = (pl.RsIn * nframe)()
        a = np.frombuffer(ins, IN_DTYPE)
        a["in"] = in_dev + GUARD + np.arange(nframe, dtype=np.uint64) * np.uint64(nin)
        a["out"] = out_dev + GUARD + np.arange(nframe, dtype=np.uint64) * np.uint64(nout)
        a["code"] = 1
        h.rs_device(ins)
        got = np.frombuffer(bytes(h.get_rs(0, nframe)), rm.RECORD_DTYPE)
        assert h.download(out_dev, (out_want.size,), np.uint8).tobytes() == out_want.tobytes()
        assert h.download(in_dev, (in_arena.size,), np.uint8).tobytes() == in_arena.tobytes()
        assert got.tobytes() == recs[idx].tobytes()
    finally:
        for p in bufs:
            h.device_free(p)
        h.close()


# ---- 3. calls in flight on two streams; a slot redefined between calls ------------------------------------------------------------------

def test_calls_in_flight_on_two_streams():
    """five calls alternating between two streams with nothing waited for between them leave what the same calls leave one after
    the other"""
    rng = np.random.default_rng(60)
    codes = [rm.Code(*rm.DVB, depth=2), rm.Code(0x12B, 7, 13, 9, 77, 5, mask_of(rng, 77, 5, 3))]
    sizes = (40, 7, 90, 1, 33)
    frames = []
    for i in range(sum(sizes)):
        c = codes[i % 2]
        d = enc(c, rng.integers(0, 256, c.k * c.depth).astype(np.uint8))
        for j in range(c.depth):
            rm.corrupt(rng, d, c, j, (0, c.t, 2, c.t + 1)[(i + j) % 4])
        frames.append(Frame(c, d, i % 2, in_mis=i % 8, out_mis=(i // 2) % 8))
    a, b = _second_stream(), _second_stream()

    def go(in_flight):
        h = _handle(codes)
        call = None
        try:
            call = Call(h, codes, frames)
            lo = 0
            for n, stream in zip(sizes, (a, b, a, b, a)):
                call.enqueue(lo, lo + n, stream.value)
                if not in_flight:
                    h.synchronize()
                    assert pl.load().hipStreamSynchronize(stream) == 0
                lo += n
            call.check(lo - sizes[-1], lo, "five calls")
            return bytes(h.get_rs(0, sizes[-1])), h.download(call.out_dev, (call.want_out.size,), np.uint8).tobytes()
        finally:
            if call:
                call.free()
            h.close()

    try:
        assert go(True) == go(False)
    finally:
        for s in (a, b):
            pl.load().hipStreamDestroy(s)


def test_a_slot_redefined_between_two_calls():
    rng = np.random.default_rng(61)
    old, new = rm.Code(*rm.CCSDS, depth=4, mask=mask_of(rng, 255, 4, 3)), rm.Code(0x11D, 0, 1, 16, 204, 4, mask_of(rng, 204, 4, 2))
    stream = _second_stream()
    h = _handle([old])
    first = second = None
    try:
        def frames_of(c):
            out = []
            for i in range(12):
                d = enc(c, rng.integers(0, 256, c.k * c.depth).astype(np.uint8))
                for j in range(c.depth):
                    rm.corrupt(rng, d, c, j, (0, c.t, 1, c.t + 1)[(i + j) % 4])
                out.append(Frame(c, d, i % 2, in_mis=i % 4, out_mis=3 - i % 4))
            return out

        first, second = Call(h, [old], frames_of(old)), Call(h, [new], frames_of(new))
        first.enqueue(stream=stream.value)
        h.rs_define(0, *new.args, mask=new.mask)  # (waits for the launch that reads the slot)
        second.enqueue(stream=stream.value)
        second.check(what="behind the redefinition")
        back = h.download(first.out_dev, (first.want_out.size,), np.uint8)
        assert back.tobytes() == first.want_out.tobytes(), "the call in front of the redefinition"
    finally:
        for c in (first, second):
            if c:
                c.free()
        h.close()
        pl.load().hipStreamDestroy(stream)


# ---- 4. the chain: viterbi -> rs on one stream -----------------------------------------------------------------------------------------

def test_viterbi_then_rs_on_one_stream():
    """psk_soft_rs_encode_host -> psk_soft_viterbi_encode_host -> int8 LLRs with a few flipped -> viterbi_device (PACKED, TERMINATED)
    -> rs_device on the same stream with no host wait between: the output is the original data, and n_err what the model says of
    the Viterbi output read back afterwards.  Some codewords carry byte errors put in front of the convolutional encoder, so that
    the outer code has work whatever the inner one repairs."""
    rng = np.random.default_rng(62)
    K, g = 7, vm.CODES[(7, 2)]
    code = rm.Code(*rm.CCSDS, depth=2, mask=rng.integers(0, 256, 510).astype(np.uint8))
    F = 6
    nin, nout = code.n * code.depth, code.k * code.depth
    T = 8 * nin + (K - 1)
    datas, llrs = [], []
    for q in range(F):
        data = rng.integers(0, 256, nout).astype(np.uint8)
        frame = pl.rs_encode_host(*code.args, data, code.mask)
        assert frame.tobytes() == code.encode(data).tobytes()
        for j in range(code.depth):
            rm.corrupt(rng, frame, code, j, (0, 3, code.t - 1)[(q + j) % 3])
        bits = np.concatenate([np.unpackbits(frame), np.zeros(K - 1, np.uint8)])
        cb = pl.viterbi_encode(K, g, 1, 3, bits)
        llr = np.where(cb == 0, 20, -20).astype(np.int8)
        flip = rng.choice(llr.size, 12, replace=False)
        llr[flip] = -llr[flip]
        datas.append(data)
        llrs.append(llr)
    stream = _second_stream()
    h = _handle([code])
    h.viterbi_define(0, K, g)
    bufs = []
    try:
        loff, lsize = _arena([x.size for x in llrs], [q % 4 for q in range(F)])
        moff, msize = _arena([nin] * F, [(q + 1) % 4 for q in range(F)])
        ooff, osize = _arena([nout] * F, [(q + 2) % 4 for q in range(F)])
        larena, marena, out_want = (np.full(s, POISON, np.uint8) for s in (lsize, msize, osize))
        for q in range(F):
            larena[loff[q]: loff[q] + llrs[q].size] = llrs[q].view(np.uint8)
        ldev, mdev, odev = (h.device_alloc(s) for s in (lsize, msize, osize))
        bufs += [ldev, mdev, odev]
        for dev, arena in ((ldev, larena), (mdev, marena), (odev, out_want)):
            h.upload(dev, arena)
        # the two calls, nothing between them
        h.viterbi_device([pl.ViterbiIn(ldev + loff[q], mdev + moff[q], T, 1, pl.VITERBI_PACKED | pl.VITERBI_TERMINATED, 0) for q in range(F)], stream.value)
        h.rs_device([(mdev + moff[q], odev + ooff[q], 1, 0) for q in range(F)], stream.value)
        recs = h.get_rs(0, F)
        mid = h.download(mdev, (msize,), np.uint8)
        got = h.download(odev, (osize,), np.uint8)
        for q in range(F):
            out_want[ooff[q]: ooff[q] + nout] = datas[q]
            mout, mrec = code.decode(mid[moff[q]: moff[q] + nin], 0)
            assert mout.tobytes() == datas[q].tobytes(), "frame %d: the model does not get the data back" % q
            rm.assert_same(recs[q], mrec, "frame %d" % q)
            assert recs[q].failed == 0
        assert got.tobytes() == out_want.tobytes(), "the data and their guards"
        assert sum(r.corrected_bytes for r in recs) > 0
    finally:
        for p in bufs:
            h.device_free(p)
        h.close()
        pl.load().hipStreamDestroy(stream)
