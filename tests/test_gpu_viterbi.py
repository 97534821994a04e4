"""psk_soft_viterbi_device on the GPU: every input and every output lies between guard bytes; outputs, records, guards and
inputs are compared byte for byte with the host definition (psk_soft_viterbi_host), which tests/test_viterbi_control.py holds to
tests/viterbi_model.py.  The shapes are the smallest at which the kernel can go wrong: frames around the 64-step chunks of its
decision words and the 256-byte window of its LLR reads, LLRs and outputs at every byte offset, every K (idle lanes), every n,
punctured frames that end at every phase, ties, the extreme LLRs at 65536 steps, more frames than the grid holds, more decisions
than the scratch bound holds, calls in flight on two streams."""
import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import demap_model as dm
from tests import sync_model as sm
from tests import viterbi_model as vm
from tests.test_gpu_sync import Rows, _second_stream

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xC3
G7 = vm.CODES[(7, 2)]
UNPUNCTURED = {(K, n): (K, g, 1, (1 << n) - 1) for (K, n), g in vm.CODES.items()}
RATES = {rate: (7, G7, P, keep) for rate, (P, keep) in vm.PUNCTURED.items()}


def _handle(codes, nch=1):
    """a handle with codes[i] = (K, g, P, keep) in slot i"""
    assert len(codes) <= pl.VITERBI_SLOTS
    h = pl.Handle(nch, device=0)
    for slot, (K, g, P, keep) in enumerate(codes):
        h.viterbi_define(slot, K, g, P, keep)
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
    """one frame of a call: the code (K, g, P, keep), its int8 LLRs, steps and flags; the LLRs start in_mis bytes and the output
    out_mis bytes past a 16-byte boundary.  skip: None, or which of n_steps / code / llr is zeroed.  shared: frames with the same
    value read the same LLR buffer (the first one's)."""

    def __init__(self, code, llr, n_steps, flags=0, in_mis=0, out_mis=0, skip=None, shared=None):
        self.code, self.llr, self.n_steps, self.flags = code, np.ascontiguousarray(llr, np.int8), n_steps, flags
        self.in_mis, self.out_mis, self.skip, self.shared = in_mis, out_mis, skip, shared
        K = code[0]
        n_bits = n_steps - (K - 1) if flags & vm.TERMINATED else n_steps
        self.out_bytes = (n_bits + 7) // 8 if flags & vm.PACKED else n_bits

    def expect(self, cache):
        """(the output bytes, the record's bytes) by the host definition; frames that share their LLRs share the result"""
        key = (self.shared, self.code, self.n_steps, self.flags) if self.shared is not None else None
        if key is None or key not in cache:
            K, g, P, keep = self.code
            out, rec = pl.viterbi_host(K, g, P, keep, self.llr, self.n_steps, self.flags)
            assert out.size == self.out_bytes
            if key is None:
                return out.tobytes(), bytes(rec)
            cache[key] = (out.tobytes(), bytes(rec))
        return cache[key]


class Call:
    """the frames of one or more calls in device memory: one arena of LLRs and one of outputs, every region between GUARD bytes of
    POISON.  enqueue() sends a range of the frames as one viterbi_device call; check() holds both arenas to what the host
    definition says of every frame enqueued so far."""

    def __init__(self, h, codes, frames):
        self.h, self.frames = h, frames
        self.slot = {c: i for i, c in enumerate(codes)}
        owners, self.in_of = [], []
        first = {}
        for i, f in enumerate(frames):
            if f.shared is not None and f.shared in first:
                self.in_of.append(first[f.shared])
                continue
            if f.shared is not None:
                first[f.shared] = len(owners)
            self.in_of.append(len(owners))
            owners.append(i)
        self.ioff, isize = _arena([max(frames[i].llr.size, 1) for i in owners], [frames[i].in_mis for i in owners])
        self.in_arena = np.full(isize, POISON, np.uint8)
        for o, i in zip(self.ioff, owners):
            self.in_arena[o: o + frames[i].llr.size] = frames[i].llr.view(np.uint8)
        self.ooff, osize = _arena([f.out_bytes for f in frames], [f.out_mis for f in frames])
        self.want_out = np.full(osize, POISON, np.uint8)
        self.in_dev, self.out_dev = h.device_alloc(isize), h.device_alloc(osize)
        h.upload(self.in_dev, self.in_arena)
        h.upload(self.out_dev, self.want_out)
        self.want_rec, self.cache = {}, {}

    def enqueue(self, lo=0, hi=None, stream=None):
        hi = len(self.frames) if hi is None else hi
        ins = (pl.ViterbiIn * (hi - lo))()
        for i in range(lo, hi):
            f = self.frames[i]
            ins[i - lo] = pl.ViterbiIn(self.in_dev + self.ioff[self.in_of[i]], self.out_dev + self.ooff[i], f.n_steps, self.slot[f.code] + 1, f.flags, 0)
            if f.skip:
                setattr(ins[i - lo], f.skip, 0)
                self.want_rec[i] = bytes(64)
                continue
            out, rec = f.expect(self.cache)
            self.want_out[self.ooff[i]: self.ooff[i] + len(out)] = np.frombuffer(out, np.uint8)
            self.want_rec[i] = rec
        self.h.viterbi_device(ins, stream)

    def check(self, lo=0, hi=None, what="the call"):
        """the records are those of the frames [lo, hi) -- the last call's --, the arenas those of every call so far"""
        hi = len(self.frames) if hi is None else hi
        recs = bytes(self.h.viterbi_records(0, hi - lo))
        with pytest.raises(pl.PskSoftError):
            self.h.viterbi_records(0, hi - lo + 1)
        back = self.h.download(self.out_dev, (self.want_out.size,), np.uint8)
        bad = np.flatnonzero(back != self.want_out)
        if bad.size:
            i = max(k for k in range(len(self.frames)) if self.ooff[k] - GUARD <= bad[0])
            f = self.frames[i]
            raise AssertionError("%s: outputs or their guards differ from byte %d on (%d bytes): frame %d at %d, %d bytes, K %d n %d P %d steps %d flags %d"
                                 % (what, bad[0], bad.size, i, self.ooff[i], f.out_bytes, f.code[0], len(f.code[1]), f.code[2], f.n_steps, f.flags))
        assert self.h.download(self.in_dev, (self.in_arena.size,), np.uint8).tobytes() == self.in_arena.tobytes(), what + ": the call wrote into LLRs or their guards"
        for i in range(lo, hi):
            got = recs[64 * (i - lo): 64 * (i - lo + 1)]
            if got != self.want_rec[i]:
                f = self.frames[i]
                vm.assert_same(got, np.frombuffer(self.want_rec[i], vm.RECORD_DTYPE)[0],
                               "%s: frame %d (K %d n %d P %d steps %d flags %d)" % (what, i, f.code[0], len(f.code[1]), f.code[2], f.n_steps, f.flags))

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
    finally:
        if call:
            call.free()
        h.close()


def llrs_of(rng, code, n_steps, kind, terminated=False):
    """the LLRs of a frame: 0 noisy code bits of random data, 1 ties (-2 .. 2), 2 all zero, 3 anything (-128 .. 127)"""
    K, g, P, keep = code
    n_llr = vm.count(len(g), P, keep, n_steps)
    if kind == 1:
        return vm.tie_llrs(rng, n_llr)
    if kind == 2:
        return np.zeros(n_llr, np.int8)
    if kind == 3:
        return rng.integers(-128, 128, n_llr).astype(np.int8)
    u = rng.integers(0, 2, n_steps).astype(np.uint8)
    if terminated and n_steps >= K - 1:
        u[n_steps - (K - 1):] = 0
    c = pl.viterbi_encode(K, g, P, keep, u)
    return np.clip(np.rint(((1.0 - 2.0 * c) + 0.7 * rng.standard_normal(c.size)) * 30.0), -127, 127).astype(np.int8)


# ---- 1. every K and n, both output forms, every flag, at every length and byte offset ----------------------------------------------

@pytest.mark.parametrize("K", (3, 4, 5, 6, 7))
def test_every_length_flag_and_byte_offset(K):
    """one call of frames of all three n, mixed: steps around the chunks of 64 and the LLR window (4097 steps of n = 4 are 65 windows),
    all eight flag combinations, LLRs and outputs at byte offsets 0 .. 7, noisy / tied / all-zero / arbitrary LLRs, and a skipped
    frame of each kind between decoded ones"""
    codes, frames = frames_of_K(K)
    run(codes, frames, "K %d" % K)


def frames_of_K(K):
    rng = np.random.default_rng(K)
    codes = [UNPUNCTURED[(K, n)] for n in (2, 3, 4)]
    steps = sorted({1, max(K - 2, 1), K - 1, K, 63, 64, 65, 127, 128, 129, 4095, 4097})
    frames, i = [], 0
    for T in steps:
        for n in (2, 3, 4):
            for flags in range(8):
                if flags & vm.TERMINATED and T < K - 1:
                    continue
                code = codes[n - 2]
                frames.append(Frame(code, llrs_of(rng, code, T, i % 4, flags & vm.TERMINATED), T, flags, in_mis=i % 8, out_mis=(i // 8 + i // 3) % 8))
                if i % 29 == 0:
                    frames.append(Frame(code, llrs_of(rng, code, 9, 3), 9, flags, in_mis=1, out_mis=3, skip=("n_steps", "code", "llr")[(i // 29) % 3]))
                i += 1
    # both output forms meet every byte offset, with bit counts that are no multiple of 8 or 64
    for packed in (0, 1):
        seen = {f.out_mis for f in frames if (f.flags & 1) == packed and not f.skip and f.n_steps > 64 and (f.n_steps - (K - 1 if f.flags & 2 else 0)) % 8}
        assert seen == set(range(8))
    assert {f.in_mis for f in frames} == set(range(8))
    return codes, frames


# ---- 2. the punctured rates: frames that end at every phase of the period ------------------------------------------------------------

def test_the_punctured_rates_at_every_phase():
    rng = np.random.default_rng(70)
    codes = list(RATES.values()) + [(7, G7, 3, 0b110000), (5, vm.CODES[(5, 3)], 2, 0b101110)]
    frames, i = [], 0
    for code in codes:
        P = code[2]
        for T in [6 + k for k in range(P)] + [60 + k for k in range(P)] + [250 + k for k in range(P)] + [1, 2, 4097]:
            for flags in (i % 8, (i + 3) % 8):
                if flags & vm.TERMINATED and T < code[0] - 1:
                    flags &= ~vm.TERMINATED
                frames.append(Frame(code, llrs_of(rng, code, T, (i // 2) % 3, flags & vm.TERMINATED), T, flags, in_mis=(i * 5) % 8, out_mis=(i * 3) % 8))
                i += 1
    run(codes, frames, "punctured")


# ---- 3. 65536 steps: the longest frame, the extreme LLRs -----------------------------------------------------------------------------

def test_frames_of_65536_steps_and_the_extreme_llrs():
    rng = np.random.default_rng(71)
    T = 65536
    c4, c2 = UNPUNCTURED[(7, 4)], UNPUNCTURED[(7, 2)]
    frames = [Frame(c4, np.full(4 * T, v, np.int8), T, flags, in_mis=k + 1, out_mis=7 - k)
              for k, (v, flags) in enumerate(((127, 0), (-127, vm.PACKED), (-128, 0), (-128, vm.PACKED | vm.ANY_START)))]
    frames.append(Frame(c2, llrs_of(rng, c2, T, 0, True), T, vm.TERMINATED | vm.PACKED, in_mis=3, out_mis=5))
    frames.append(Frame(c2, llrs_of(rng, c2, T - 1, 3), T - 1, 0, in_mis=6, out_mis=1))
    h = _handle([c4, c2])
    call = None
    try:
        call = Call(h, [c4, c2], frames)
        call.enqueue()
        call.check(what="65536 steps")
        r = h.viterbi_records(0, 4)
        assert r[0].metric == r[0].sum_abs == 127 * 4 * T and r[0].n_flip == 0
        assert all(abs(x.metric) < 1 << 26 and x.sum_abs == abs(v) * 4 * T for x, v in zip(r, (127, -127, -128, -128)))
    finally:
        if call:
            call.free()
        h.close()


# ---- 4. more frames than the grid holds; more decisions than the scratch bound holds -------------------------------------------------

def test_sixty_six_thousand_short_frames_in_one_call():
    """66 000 frames of one to eight steps of two codes, a skipped one every 97: beyond 65535 workgroups the frames are the second
    trip of the frame loop.  Every output has 16 bytes of the arena, 4 of them in front of it; the whole arena is compared."""
    rng = np.random.default_rng(72)
    codes = [UNPUNCTURED[(7, 2)], UNPUNCTURED[(3, 3)]]
    N, CELL = 66000, 16
    kinds = []  # 64 distinct frames: (code, steps, flags, LLRs, output, record)
    for k in range(64):
        code, T, flags = codes[k % 2], 1 + k % 8, (k // 8) % 8
        if flags & vm.TERMINATED and T < code[0] - 1:
            flags &= ~vm.TERMINATED
        llr = llrs_of(rng, code, T, 3 if k % 3 else 1)
        out, rec = pl.viterbi_host(*code, llr, T, flags)
        kinds.append((code, T, flags, llr, out, bytes(rec)))
    in_arena = np.full(64 * 64 + 2 * GUARD, POISON, np.uint8)
    for k, kind in enumerate(kinds):
        in_arena[GUARD + 64 * k + k % 5: GUARD + 64 * k + k % 5 + kind[3].size] = kind[3].view(np.uint8)
    want = np.full(N * CELL + 2 * GUARD, POISON, np.uint8)
    which = (np.arange(N) * 37 + np.arange(N) // 64) % 64
    skipped = np.arange(N) % 97 == 96
    for k, kind in enumerate(kinds):
        at = GUARD + CELL * np.flatnonzero((which == k) & ~skipped) + 4
        for b, v in enumerate(kind[4]):
            want[at + b] = v
    h = _handle(codes)
    in_dev = out_dev = None
    try:
        in_dev, out_dev = h.device_alloc(in_arena.size), h.device_alloc(want.size)
        h.upload(in_dev, in_arena)
        h.upload(out_dev, np.full(want.size, POISON, np.uint8))
        ins = np.zeros(N, np.dtype([("llr", "<u8"), ("out", "<u8"), ("n_steps", "<u4"), ("code", "<u4"), ("flags", "<u4"), ("pad", "<u4")]))
        ins["llr"] = in_dev + GUARD + 64 * which + which % 5
        ins["out"] = out_dev + GUARD + CELL * np.arange(N) + 4
        ins["n_steps"] = np.array([k[1] for k in kinds])[which]
        ins["code"] = np.where(skipped, 0, 1 + which % 2)
        ins["flags"] = np.array([k[2] for k in kinds])[which]
        h.viterbi_device((pl.ViterbiIn * N).from_buffer_copy(ins.tobytes()))
        recs = np.frombuffer(bytes(h.viterbi_records(0, N)), np.uint8).reshape(N, 64)
        want_rec = np.array([np.frombuffer(k[5], np.uint8) for k in kinds])[which]
        want_rec[skipped] = 0
        bad = np.flatnonzero((recs != want_rec).any(axis=1))
        assert bad.size == 0, "records differ from frame %d on (%d frames)" % (bad[0], bad.size)
        back = h.download(out_dev, (want.size,), np.uint8)
        bad = np.flatnonzero(back != want)
        assert bad.size == 0, "outputs differ from byte %d on (%d bytes): frame %d" % (bad[0], bad.size, (bad[0] - GUARD) // CELL)
        assert h.download(in_dev, (in_arena.size,), np.uint8).tobytes() == in_arena.tobytes()
    finally:
        for p in (in_dev, out_dev):
            if p:
                h.device_free(p)
        h.close()


def test_more_long_frames_than_the_scratch_bound_holds():
    """decisions are 8 bytes a step: PSK_SOFT_VITERBI_SCRATCH_BYTES hold 512 frames of 65536 steps, so a call of 520 such frames
    (and shorter ones between them) takes a second trip of its workgroups.  The frames read four LLR buffers between them."""
    rng = np.random.default_rng(73)
    T = 65536
    in_flight = pl.VITERBI_SCRATCH_BYTES // (8 * T)
    assert in_flight == 512
    code = UNPUNCTURED[(7, 2)]
    llr = [llrs_of(rng, code, T, kind) for kind in (0, 1, 3, 0)]
    frames = []
    for i in range(in_flight + 8):
        k = i % 4
        steps = T if i % 8 else T - 1 - 64 * (i % 5)  # (every eighth is a little shorter, a prefix of the same LLRs)
        frames.append(Frame(code, llr[k], steps, vm.PACKED | (vm.ANY_START if k == 3 else 0), in_mis=k, out_mis=i % 8, shared=k))
    assert sum(f.n_steps for f in frames) * 8 > pl.VITERBI_SCRATCH_BYTES
    run([code], frames, "beyond the scratch bound")


# ---- 5. calls in flight: two streams until the ring wraps, a redefinition between two calls ------------------------------------------

def test_calls_on_two_streams_in_turn_until_the_ring_wraps():
    """five calls on streams A, B, A, B, A with no wait between them: the ring of two slots wraps twice, the records grow with the
    second call (300 frames after 3).  All outputs and guards are whole, the records are the fifth call's, and everything equals
    the same calls with a wait after each."""
    rng = np.random.default_rng(74)
    codes = [UNPUNCTURED[(7, 2)], UNPUNCTURED[(4, 3)], RATES["3/4"]]
    sizes = (3, 300, 2, 40, 5)
    frames = []
    for i in range(sum(sizes)):
        code, T, flags = codes[i % 3], (700, 65, 1, 129, 2000)[i % 5] + i % 7, i % 8
        if T < code[0] - 1:
            flags &= ~vm.TERMINATED
        frames.append(Frame(code, llrs_of(rng, code, T, i % 3, flags & vm.TERMINATED), T, flags, in_mis=i % 8, out_mis=(i // 2) % 8))
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
            return bytes(h.viterbi_records(0, sizes[-1])), h.download(call.out_dev, (call.want_out.size,), np.uint8).tobytes()
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
    rng = np.random.default_rng(75)
    old, new = UNPUNCTURED[(7, 2)], UNPUNCTURED[(5, 3)]
    stream = _second_stream()
    h = _handle([old])
    first = second = None
    try:
        f1 = [Frame(old, llrs_of(rng, old, T, 0), T, i % 8, in_mis=i, out_mis=7 - i) for i, T in enumerate((3000, 64, 4097, 130))]
        f2 = [Frame(new, llrs_of(rng, new, T, 0), T, i % 8, in_mis=i, out_mis=7 - i) for i, T in enumerate((3000, 64, 4097, 130))]
        first, second = Call(h, [old], f1), Call(h, [new], f2)
        first.enqueue(stream=stream.value)
        h.viterbi_define(0, *new)  # (waits for the launch that reads the slot)
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


# ---- 6. the demodulator is left alone; the whole chain on one stream -----------------------------------------------------------------

def test_a_viterbi_call_touches_no_demodulator_state_and_no_other_record():
    M, S, C, N = 4, 8, 3, 8192
    rng = np.random.default_rng(76)
    iq = [sm.framed_stream(M, S, 32, 500, N // S + 8, 100, 0.1, 30 + c) for c in range(C)]
    code = UNPUNCTURED[(7, 2)]
    h = _handle([code], C)
    rows = call = llr_dev = None
    try:
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=50, phaseAvg=50)
        h.sync_define(0, iq[0][1])
        pz = sm.psk_points(M, np.arange(M))
        points = np.empty(2 * M, np.float32)
        points[0::2], points[1::2] = pz.real, pz.imag
        h.demap_define(0, points, dm.gray_labels(M))
        rows = Rows(h, C, N)
        out = rows.call([x[0][: 2 * N] for x in iq], True)
        h.sync_device(0, [pl.SyncIn(o.soft, o.n_symbols, 1, 0, 0.7, 0) for o in out])
        llr_dev = h.device_alloc(4096)
        h.demap_device([pl.DemapIn(out[0].soft, out[0].n_symbols, 0, llr_dev, 400, 0, 1, pl.DEMAP_I8, 1.0, 0.0, 16.0, 0)])

        def state():
            return ([h.peek(c) for c in range(C)], h.stats(), h.channel_stats(), [h.export_state(c) for c in range(C)], bytes(h.sync_records()),
                    [h.sync_history(c).tobytes() for c in range(C)], bytes(h.demap_records(0, 1)))

        before = state()
        call = Call(h, [code], [Frame(code, llrs_of(rng, code, T, 0), T, i % 8, in_mis=i, out_mis=i + 2) for i, T in enumerate((500, 77, 1300))])
        call.enqueue()
        call.check(what="behind a process, a sync and a demap call")
        assert state() == before
    finally:
        if llr_dev:
            h.device_free(llr_dev)
        if call:
            call.free()
        if rows:
            rows.free()
        h.close()


def test_process_sync_demap_viterbi_on_one_stream(oracle_mod):
    """the CPU chain of tests/test_viterbi_control.py once on the GPU: process_device, sync_device, demap_device (int8) and
    viterbi_device enqueued on one stream with no wait between them.  The descriptors of the demap call are the host chain's hits and
    gains (the GPU's soft row is the oracle's, bit for bit); hits, LLRs, payloads and records are byte-equal to the host chain."""
    from tests.test_viterbi_control import CHAIN_CLEAN, CHAIN_FRAME, CHAIN_M, CHAIN_S, CHAIN_SCALE, CHAIN_STEPS, CHAIN_WL, PAYLOAD, chain_points, chain_run, chain_stream

    soft, w, hits, gains, llrs, outs, recs, payloads, coded = chain_run(oracle_mod, CHAIN_CLEAN)
    iq = chain_stream(CHAIN_CLEAN)[0]
    code = UNPUNCTURED[(7, 2)]
    stream = _second_stream()
    h = _handle([code])
    rows = None
    bufs = []
    try:
        h.configure_all(samplesPerBaud=CHAIN_S, constelationSize=CHAIN_M, numAvg=50, phaseAvg=50)
        h.sync_define(0, w)
        h.demap_define(0, *chain_points())
        rows = Rows(h, 1, 8192)
        F = len(hits)
        llr_off, llr_size = _arena([2 * CHAIN_STEPS] * F, [(3 * k) % 8 for k in range(F)])
        out_off, out_size = _arena([PAYLOAD] * F, [(5 * k + 1) % 8 for k in range(F)])
        llr_want, out_want = np.full(llr_size, POISON, np.uint8), np.full(out_size, POISON, np.uint8)
        llr_dev, out_dev = h.device_alloc(llr_size), h.device_alloc(out_size)
        bufs += [llr_dev, out_dev]
        h.upload(llr_dev, llr_want)
        h.upload(out_dev, out_want)
        for k in range(F):
            llr_want[llr_off[k]: llr_off[k] + 2 * CHAIN_STEPS] = llrs[k].view(np.uint8)
            out_want[out_off[k]: out_off[k] + PAYLOAD] = outs[k]
        # the four calls, nothing between them
        # (packets of 8192 samples, as the oracle was fed; the soft symbols of the calls abut in one row: a call's count is known
        # on the host when the call returns)
        n_sym = soft.size // 2
        soft_dev = h.device_alloc(8 * n_sym + 8 * rows.cap)
        bufs.append(soft_dev)
        iq_dev = h.device_alloc(iq.nbytes)
        bufs.append(iq_dev)
        h.upload(iq_dev, iq)
        done = 0
        for a in range(0, iq.size // 2, 8192):
            n = min(8192, iq.size // 2 - a)
            pk, out = (pl.Packet * 1)(), (pl.Output * 1)()
            p, q = pk[0], out[0]
            p.data, p.n_floats, p.sri_xdelta, p.sri_mode, p.sriChanged, p.present, p.format = iq_dev + 8 * a, 2 * n, 0.01, 1, int(a == 0), 1, 0
            q.soft, q.bits, q.phase, q.sampleIndex = soft_dev + 8 * done, rows.bufs[2], rows.bufs[3], rows.bufs[4]
            q.cap_symbols = rows.cap
            h.process_device(0, pk, out, stream.value)
            done += int(out[0].n_symbols)
        assert done == n_sym
        h.sync_device(0, [pl.SyncIn(soft_dev, n_sym, 1, pl.SYNC_RESTART, 0.7, 0)], stream.value)
        h.demap_device([pl.DemapIn(soft_dev, n_sym, hit.pos + CHAIN_WL, llr_dev + llr_off[k], CHAIN_FRAME, 0, 1, pl.DEMAP_I8,
                                   float(g[0]), float(g[1]), CHAIN_SCALE, 0) for k, (hit, g) in enumerate(zip(hits, gains))], stream.value)
        h.viterbi_device([pl.ViterbiIn(llr_dev + llr_off[k], out_dev + out_off[k], CHAIN_STEPS, 1, pl.VITERBI_TERMINATED, 0) for k in range(F)], stream.value)
        got = h.viterbi_records(0, F)
        assert h.download(soft_dev, (2 * n_sym,), np.float32).tobytes() == soft.tobytes()
        srec = h.sync_records()[0]
        assert [x.pos for x in srec.hits[: srec.n_hits]][:F] == [x.pos for x in hits]
        assert h.download(llr_dev, (llr_size,), np.uint8).tobytes() == llr_want.tobytes(), "the LLRs and their guards"
        assert h.download(out_dev, (out_size,), np.uint8).tobytes() == out_want.tobytes(), "the payloads and their guards"
        for k in range(F):
            assert bytes(got[k]) == bytes(recs[k]), "frame %d" % k
            assert out_want[out_off[k]: out_off[k] + PAYLOAD].tobytes() == payloads[k].tobytes() and got[k].n_flip == 0
    finally:
        for p in bufs:
            h.device_free(p)
        if rows:
            rows.free()
        h.close()
        pl.load().hipStreamDestroy(stream)
