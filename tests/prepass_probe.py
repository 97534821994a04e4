"""The pre-pass kernels by themselves: ctypes binding of the test-only probe library (tests/support/prepass_probe.hip ->
psk_soft_amd/libpsk_prepass_probe.so: a shim linked with the product's own psk_gather.o, psk_tune.o, psk_resample.o and
psk_fir.o), the ARENA the kernels run in, the arena the models expect, and the comparator.

An arena is one byte image: sources, destination rows, history slots, and poison everywhere else.  The descriptors have the
product's layout (psk_gather.h, psk_tune.h, psk_resample.h, psk_fir.h) with byte offsets into the arena where the product has pointers.  A
case below lays the arena out, fills the descriptors and computes the arena the launch must leave: a byte copy for the gathers,
tune_model.apply for the tune kernel, tune_model.apply followed by resample_model.apply for the resample kernel and by
fir_model.apply for the filter kernel.  Arena.compare holds the whole downloaded arena to it byte for byte: every row sample,
both history slots (and the padding of a slot behind its payload), every source byte -- the taps are one --, the padding of every
row up to its 128 bytes and every guard byte.

Everything is placed on a 128-byte line (plus the skew a case asks for: the least alignment of a packet) and followed by a
guard of 128 bytes; the extents behind every descriptor are checked against the arena here, in front of every launch.

The two looks (psk_symrate.hip, psk_acquire.hip; the shim links psk_symrate.o and psk_acquire.o too) run in an arena as well: a
LookCase at the end of this file lays out the sources, a region of partials and a region of records -- memory the handle
allocates in the product, which tests/row_guards.py cannot fence --, launches fold and join once each, and expects the bytes
of symrate_model.partials / join_bytes and acquire_model.device_partials / join_bytes: every partial, every record, and poison
in every partial's pad, in every slot no descriptor owns and in the guards.

The word search (psk_sync.hip; the shim links psk_sync.o) closes the file: a SyncCase holds the rows, the words, both history
slots of every searched descriptor, the partials and the records, launches the fold, the join or both, and expects of every
partial the members sync_model.partial_writes lists -- NaN poison in the others --, sync_model.join_bytes of the partials in the
record, the model's history in hist_out, poison in its pad, and everything else as it went up."""
import ctypes
import math
import os

import numpy as np

from tests import acquire_model as am
from tests import fir_model as fm
from tests import resample_model as rm
from tests import symrate_model as sm
from tests import sync_model as ym
from tests import tune_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "psk_soft_amd", "libpsk_prepass_probe.so")

F32 = np.float32
FORMAT_CF32, FORMAT_CS16, FORMAT_CS8, FORMAT_CF16 = 0, 1, 3, 4  # PSK_SOFT_FORMAT_*
FORMATS = (FORMAT_CF32, FORMAT_CS16, FORMAT_CS8, FORMAT_CF16)
DTYPE_OF = {FORMAT_CF32: np.dtype(np.float32), FORMAT_CS16: np.dtype(np.int16), FORMAT_CS8: np.dtype(np.int8), FORMAT_CF16: np.dtype(np.float16)}
SAMPLE_BYTES = {f: 2 * d.itemsize for f, d in DTYPE_OF.items()}
# what lies in the other columns of a strided packet's matrix: a NaN for the float formats, the most negative integer
POISON_OF = {FORMAT_CF32: np.uint32(0x7FC00ABC).view(np.float32), FORMAT_CS16: np.int16(-32768), FORMAT_CS8: np.int8(-128),
             FORMAT_CF16: np.uint16(0x7E55).view(np.float16)}
RS_RESTART, RS_TUNED = 1, 2  # FrontIo::flags (psk_front_src.h): kFrontRestart, kFrontTuned
LINE, GUARD = 128, 128
GUARD_BYTE, ROW_BYTE = 0xA5, 0xC3
REPORTED = 8  # findings a comparison lists at the most

_U8, _U4 = "<u8", "<u4"
GROUP = np.dtype([("src", _U8), ("stride", _U8), ("n_max", _U8), ("tile0", _U8), ("first", _U4), ("g", _U4), ("tiles_c", _U4), ("pad", _U4)])
CHAN = np.dtype([("dst", _U8), ("n", _U8)])
SINGLE = np.dtype([("src", _U8), ("dst", _U8), ("stride", _U8), ("n", _U8)])
TUNE = np.dtype([("src", _U8), ("dst", _U8), ("stride", _U8), ("n", _U8), ("phase", _U8), ("step", _U8), ("format", _U4), ("pad", _U4)])
RESAMPLE = np.dtype([("src", _U8), ("dst", _U8), ("stride", _U8), ("n", _U8), ("phase", _U8), ("step", _U8), ("format", _U4), ("flags", _U4),
                     ("pos", _U8), ("rstep", _U8), ("n_out", _U8), ("hist_in", _U8), ("hist_out", _U8)])
# (psk_fir.h's static_assert pins these offsets: io 0, decim 56, pos 60, n_taps 64, pad 68, n_out 72, taps 80, hist_in 88, hist_out 96)
FIR = np.dtype([("src", _U8), ("dst", _U8), ("stride", _U8), ("n", _U8), ("phase", _U8), ("step", _U8), ("format", _U4), ("flags", _U4),
                ("decim", _U4), ("pos", _U4), ("n_taps", _U4), ("pad", _U4), ("n_out", _U8), ("taps", _U8), ("hist_in", _U8), ("hist_out", _U8)])
# the two looks (psk_symrate.h, psk_acquire.h; the records: include/psk_soft_hip.h)
_F8, _U2, _U1 = "<f8", "<u2", "u1"
SYMRATE_DESC = np.dtype([("src", _U8), ("stride", _U8), ("n", _U8), ("phase", _U8), ("step", _U8), ("wstep", _U8), ("n_blocks", _U4), ("part0", _U4),
                         ("n_piece", _U4), ("channel", _U4), ("S", _U2), ("format", _U1), ("flags", _U1), ("tail", _U4)])
SYMRATE_PART = np.dtype([("d", _F8, 36), ("c", _U4, 9), ("pad", _U4)])
ACQUIRE_DESC = np.dtype([("src", _U8), ("stride", _U8), ("n", _U8), ("phase", _U8), ("step", _U8), ("part0", _U4), ("n_piece", _U4), ("channel", _U4),
                         ("M", _U2), ("format", _U1), ("flags", _U1)])
ACQUIRE_PART = np.dtype([("d", _F8, 17), ("c", _U4, 9), ("pad", _U4)])
SYMRATE_REC = np.dtype([("n_samples", _U8), ("n_used", _U8), ("n_blocks", _U8), ("n_valid", _U8), ("n_pairs", _U8, 8), ("sum_re", _F8, (2, 8)),
                        ("sum_im", _F8, (2, 8)), ("sum_pow", _F8, 2), ("sum_lvl", _F8, 2), ("samplesPerBaud", _U2), ("flags", _U1), ("pad", _U1, 5)])
ACQUIRE_REC = np.dtype([("n_samples", _U8), ("n_valid", _U8), ("n_pairs", _U8, 8), ("sum_re", _F8, 8), ("sum_im", _F8, 8), ("sum_e", _F8),
                        ("constelationSize", _U2), ("flags", _U1), ("pad", _U1, 5)])
# the word search (psk_sync.h; the partial and the record: tests/sync_model.py)
SYNC_DESC = np.dtype([("soft", _U8), ("word", _U8), ("hist_in", _U8), ("hist_out", _U8), ("n", _U8), ("p0", "<i8"), ("n_windows", _U4), ("part0", _U4),
                      ("n_piece", _U4), ("channel", _U4), ("L", _U4), ("flags", _U4), ("threshold", "<f4"), ("Ew", "<f4")])
# in the order of psk_prepass_probe_sizeof
MIRRORS = (GROUP, CHAN, SINGLE, TUNE, RESAMPLE, FIR, SYMRATE_DESC, SYMRATE_PART, ACQUIRE_DESC, ACQUIRE_PART, SYMRATE_REC, ACQUIRE_REC,
           SYNC_DESC, ym.PART_DTYPE, ym.RECORD_DTYPE)
CONSTANTS = ("resample_piece", "resample_inputs", "gather_tile", "gather_min_group", "tune_table_floats", "fir_window", "fir_max_taps",
             "fir_hist_slot_floats", "symrate_piece", "symrate_halo", "symrate_threads", "symrate_min_s", "symrate_max_s", "symrate_max_blocks",
             "acquire_piece", "acquire_halo", "acquire_threads", "sync_piece", "sync_threads", "sync_hist", "sync_hist_slot_floats",
             "sync_max_word", "sync_hits")
LOOK_DATA, LOOK_TUNED = 1, 2  # PSK_SOFT_SR_DATA / PSK_SOFT_A_DATA, PSK_SOFT_SR_TUNED / PSK_SOFT_A_TUNED
FIR_HIST_BYTES = 8 * fm.HIST  # the payload of a history slot of the filter: 127 float2


# ---- the binding -----------------------------------------------------------------------------------------------------------------

_lib = None
_failed = None  # the first HIP error of this process: nothing more is launched after one


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is not built (make -C psk_soft_amd/csrc)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        vp, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        for name, args in (("psk_prepass_probe_sizeof", [i]), ("psk_prepass_probe_constant", [i]),
                           ("psk_prepass_probe_gather_singles", [vp, u64, i, vp, u32, u64]),
                           ("psk_prepass_probe_gather_tiles", [vp, u64, i, vp, u32, vp, u32, u64]),
                           ("psk_prepass_probe_tune", [vp, u64, vp, u32, u64, vp]),
                           ("psk_prepass_probe_resample", [vp, u64, vp, u32, u64]), ("psk_prepass_probe_fir_piece", [i]),
                           ("psk_prepass_probe_fir", [vp, u64, vp, u32, u64]),
                           ("psk_prepass_probe_symrate", [vp, u64, vp, u32, u32, u64, u64]),
                           ("psk_prepass_probe_acquire", [vp, u64, vp, u32, u32, u64, u64, i]),
                           ("psk_prepass_probe_sync", [vp, u64, vp, u32, u32, u64, u64, i])):
            getattr(L, name).argtypes, getattr(L, name).restype = args, i
        _lib = L
    return _lib


def sizeof(which):
    """sizeof of the product's descriptor MIRRORS[which] mirrors"""
    return int(load().psk_prepass_probe_sizeof(which))


def constant(name):
    """a constant of the kernels' headers, by its name in CONSTANTS"""
    return int(load().psk_prepass_probe_constant(CONSTANTS.index(name)))


def fir_piece(decim):
    """fir_piece(decim) of psk_fir.h: the outputs of one piece of the filter pass at that decimation"""
    return int(load().psk_prepass_probe_fir_piece(int(decim)))


def _launch(what, fn, image, *args):
    """the arena after the launch (a new array); raises on a HIP error, and at every call after one"""
    global _failed
    if _failed is not None:
        raise RuntimeError("not run: an earlier launch failed (%s)" % _failed)
    after = np.array(image, np.uint8)
    err = fn(after.ctypes.data, after.size, *args)
    if err != 0:
        _failed = "%s: HIP error %d" % (what, err)
        raise RuntimeError(_failed)
    return after


# ---- launch_resample's grid rule ---------------------------------------------------------------------------------------------------

def resample_grid(n_desc, max_n_out, piece):
    """Workgroups per packet, as psk::launch_resample (psk_resample.hip) shapes its grid: min(pieces of the longest packet,
    ceil(2048 / n_desc)), at least 1, at most 65535.  2048 and the bounds are that function's literals."""
    per = min(-(-max_n_out // piece), -(-2048 // n_desc))
    return max(1, min(per, 65535))


def resample_walk(n_out, per, piece):
    """(the pieces each of the `per` workgroups of a packet takes, the workgroup that writes the history), as
    psk_resample_kernel and rs_packet (psk_resample.hip) have it: piece p goes to workgroup p % per; the owner of the last
    piece, or workgroup 0 of a packet without outputs, writes the history."""
    n_pieces = -(-n_out // piece)
    return [list(range(y, n_pieces, per)) for y in range(per)], ((n_pieces - 1) % per if n_pieces else 0)


def length_for(n_out, step):
    """(n, pos): a packet length and a position below or at 2^33 with exactly n_out outputs"""
    one = 1 << 32
    for pos in (step // 3, step // 3 + (1 << 31), 5, one + 7, (1 << 33) - 9, 1 << 33):
        for n in range(max(1, n_out * step // one - 3), n_out * step // one + 6):
            if rm.count(pos, step, n) == n_out:
                return n, pos
    raise AssertionError((n_out, step))


# ---- launch_fir's grid rule, the kernel's walk and its lanes -----------------------------------------------------------------------

def fir_grid(n_desc, max_pieces):
    """Workgroups per packet, as front_grid_y (psk_front_src.h) has it for psk::launch_fir: min(pieces of the packet with the
    most, ceil(2048 / n_desc)), at least 1, at most 65535.  2048 and the bounds are that function's literals."""
    per = min(max_pieces, -(-2048 // n_desc))
    return max(1, min(per, 65535))


def fir_walk(n_out, per, piece):
    """(the pieces each of the `per` workgroups of a packet takes, the workgroup that writes the history), as psk_fir_kernel and
    fir_packet (psk_fir.hip) have it: piece p goes to workgroup p % per; the owner of the last piece, or workgroup 0 of a
    packet without outputs, writes the history."""
    n_pieces = -(-n_out // piece)
    return [list(range(y, n_pieces, per)) for y in range(per)], ((n_pieces - 1) % per if n_pieces else 0)


def fir_lanes(decim):
    """(R, padded): the outputs a lane produces at that decimation -- 4 at D <= 3, 2 at D <= 7, else 1 -- and whether the LDS
    window is padded, which it is where the lanes' stride R * D is even (fir_outputs_per_lane, fir_pad_shift: psk_fir.hip)"""
    R = 4 if decim <= 3 else 2 if decim <= 7 else 1
    return R, (R * decim) % 2 == 0


def fir_split(decim, n_taps):
    """(lead, head, mid, Q): fir_sums (psk_fir.hip) walks the steps [0, head) and [mid, Q) with a test per output and
    [head, mid) without one; lead = (R-1) * D, Q = lead + T, head = min(lead + 1, Q), mid = max(T, head)"""
    lead = (fir_lanes(decim)[0] - 1) * decim
    Q = lead + n_taps
    head = min(lead + 1, Q)
    return lead, head, max(n_taps, head), Q


# ---- the arena ---------------------------------------------------------------------------------------------------------------------

class Region:
    """bytes [start, end) of the arena.  kind: "source" (never written), "row" (the samples a descriptor's kernel writes),
    "padding" (the rest of the row's lines), "hist_in" (the slot read), "hist_out" (the slot written), "hist_pad" (the bytes of
    a history slot behind its payload: never written); desc: the descriptor it belongs to; unit: bytes of one sample of it"""

    def __init__(self, start, end, kind, desc, unit):
        self.start, self.end, self.kind, self.desc, self.unit = start, end, kind, desc, unit


class Arena:
    def __init__(self):
        self._parts, self.size, self.regions = [], 0, []
        self._fill(GUARD)

    def _fill(self, n, byte=GUARD_BYTE):
        if n:
            self._parts.append(np.full(n, byte, np.uint8))
            self.size += n

    def _place(self, data, skew=0):
        """data on a line (+ skew bytes), the rest of its last line and a guard behind it; its offset"""
        assert self.size % LINE == 0 and 0 <= skew < LINE
        self._fill(skew)
        at = self.size
        self._parts.append(np.frombuffer(np.ascontiguousarray(data).tobytes(), np.uint8))
        self.size += self._parts[-1].size
        self._fill(-self.size % LINE + GUARD)
        return at

    def source(self, data, desc, unit, skew=0):
        at = self._place(data, skew)
        self.regions.append(Region(at, at + np.asarray(data).nbytes, "source", desc, unit))
        return at

    def row(self, n, unit, desc):
        """a row of n samples of `unit` bytes: as the product sizes it, whole lines, one at the least"""
        cap = (max(n, 1) * unit + LINE - 1) // LINE * LINE
        at = self._place(np.full(cap, ROW_BYTE, np.uint8))
        self.regions.append(Region(at, at + n * unit, "row", desc, unit))
        self.regions.append(Region(at + n * unit, at + cap, "padding", desc, unit))
        return at

    def history(self, slot_in, values, desc, slot_bytes=24, payload_bytes=24):
        """the two slots of a channel, `slot_bytes` each, back to back as the handle has them: the first `payload_bytes` of slot
        `slot_in` hold `values` (floats), everything else -- the other slot, and the padding of either slot behind its payload
        -- poison.  The resampler's slots are 24 bytes and all payload, the filter's 1 KiB with 1016 bytes of payload.
        (offset of the slot read, offset of the slot written)"""
        data = np.frombuffer(np.asarray(values, F32).tobytes(), np.uint8)
        assert data.size == payload_bytes <= slot_bytes and payload_bytes % 8 == 0
        pair = np.full(2 * slot_bytes, ROW_BYTE, np.uint8)
        pair[slot_bytes * slot_in : slot_bytes * slot_in + payload_bytes] = data
        at = self._place(pair)
        a, b = at + slot_bytes * slot_in, at + slot_bytes * (slot_in ^ 1)
        self.regions.append(Region(a, a + payload_bytes, "hist_in", desc, 8))
        self.regions.append(Region(b, b + payload_bytes, "hist_out", desc, 8))
        if payload_bytes < slot_bytes:
            for slot in (a, b):
                self.regions.append(Region(slot + payload_bytes, slot + slot_bytes, "hist_pad", desc, 1))
        return a, b

    def image(self):
        img = np.concatenate(self._parts)
        assert img.size == self.size
        # (a row without samples is an empty region: it holds no byte, so the lookups below leave it out)
        self._solid = sorted((r for r in self.regions if r.end > r.start), key=lambda r: r.start)
        self._empty = {(r.kind, r.start) for r in self.regions if r.end == r.start}
        self._starts = np.array([r.start for r in self._solid], np.int64)
        assert all(x.end <= y.start for x, y in zip(self._solid, self._solid[1:]))
        return img

    def _region_at(self, off):
        """(index into the non-empty regions of the last one that starts at or in front of byte `off`, or -1; does it hold it?)"""
        k = int(np.searchsorted(self._starts, off, "right")) - 1
        return k, k >= 0 and off < self._solid[k].end

    def inside(self, kind, off, nbytes):
        """is [off, off + nbytes) inside one region of that kind (an empty range: is it such an empty region)?"""
        if nbytes == 0:
            return (kind, off) in self._empty
        k, holds = self._region_at(off)
        return holds and self._solid[k].kind == kind and off + nbytes <= self._solid[k].end

    def compare(self, want, got):
        """[] if the two images are equal; else at most REPORTED findings in arena order, one per region (or guard) that
        differs: dict(desc, where, sample, offset, n_bytes, want, got, message) -- the first differing sample of the region,
        its bytes as hex strings, and how many bytes of the region differ"""
        assert want.size == got.size == self.size
        diff = np.flatnonzero(want != got)
        found, at = [], 0
        while at < diff.size and len(found) < REPORTED:
            off = int(diff[at])
            k, holds = self._region_at(off)
            r, guard = (self._solid[k] if k >= 0 else None), not holds
            if guard:
                lo = r.end if r is not None else 0
                hi = self._solid[k + 1].start if k + 1 < len(self._solid) else self.size
                where, unit, sample, first = "guard", 1, None, off
            else:
                lo, hi, where, unit = r.start, r.end, r.kind, r.unit
                sample = (off - lo) // unit
                first = lo + sample * unit
            stop = int(np.searchsorted(diff, hi, "left"))
            w, g = want[first : first + unit].tobytes().hex(), got[first : first + unit].tobytes().hex()
            desc = r.desc if r is not None else None
            if guard:
                msg = "guard: %d byte(s) changed, the first %d byte(s) behind the %s of descriptor %s (offset %d): %s -> %s" % (
                    stop - at, off - lo, r.kind if r is not None else "start", desc, off, w, g)
            else:
                msg = "descriptor %s %s: %d byte(s) differ, the first in sample %d (offset %d): want %s, got %s" % (
                    desc, where, stop - at, sample, off, w, g)
            found.append(dict(desc=desc, where=where, sample=sample, offset=off, n_bytes=stop - at, want=w, got=g, message=msg))
            at = stop
        return found


def messages(found):
    return "\n".join(f["message"] for f in found)


# ---- cases: an arena, its descriptors, the arena expected behind the launch ----------------------------------------------------

def _strided(iq, fmt, stride, col):
    """the matrix a packet of stride `stride` is column `col` of -- n frames, everything else poison -- and the byte offset of
    the packet's sample 0 in it; the packet itself for stride 1"""
    dt = DTYPE_OF[fmt]
    x = np.ascontiguousarray(iq, dt)
    n = x.size // 2
    if stride == 1:
        return x[: 2 * n], 0
    mat = np.full((n, stride, 2), POISON_OF[fmt], dt)
    mat[:, col, :] = x[: 2 * n].reshape(n, 2)
    return mat, col * SAMPLE_BYTES[fmt]


class _Case:
    def __init__(self):
        self.arena = Arena()
        self._writes = []  # (offset, bytes the launch must leave there)

    def _finish(self):
        self.image = self.arena.image()
        self.want = self.image.copy()
        for off, data in self._writes:
            b = np.frombuffer(np.ascontiguousarray(data).tobytes(), np.uint8)
            self.want[off : off + b.size] = b

    def _extents(self, src, sb, stride, n, dst, unit, n_dst):
        """what a kernel may touch behind a descriptor lies in the arena's source and row of it"""
        a = self.arena
        assert n >= 1 and stride >= 1
        assert a.inside("source", src, sb) and a.inside("source", src + (n - 1) * stride * sb, sb), (src, sb, stride, n)
        assert dst % LINE == 0 and a.inside("row", dst, n_dst * unit), (dst, unit, n_dst)

    def check(self, after):
        return self.arena.compare(self.want, after)


class ResampleCase(_Case):
    """One launch of the resample kernel.  packets: dicts of fmt, stride (1 or more; the packet is column i % stride of its
    matrix), iq (interleaved I/Q in the format's dtype), tune ((phase, step) or None), pos, rstep, restart, hist (six floats in
    the slot that is read, or None: the handle's zeros), slot (which of the two is read; default i % 2)."""

    def __init__(self, packets):
        super().__init__()
        self.packets = packets
        self.desc = np.zeros(len(packets), RESAMPLE)
        self.rows, self.hists = [], []
        for i, p in enumerate(packets):
            fmt, stride, sb = p["fmt"], p["stride"], SAMPLE_BYTES[p["fmt"]]
            data, col_off = _strided(p["iq"], fmt, stride, i % stride)
            n = np.asarray(p["iq"]).size // 2
            x = np.ascontiguousarray(p["iq"], DTYPE_OF[fmt])[: 2 * n]
            s = x.astype(F32) if p["tune"] is None else tm.apply(p["tune"][0], p["tune"][1], x)
            hist = np.zeros(6, F32) if p["hist"] is None else np.asarray(p["hist"], F32)
            y, h_out = rm.apply(p["pos"], p["rstep"], s, hist, p["restart"])
            n_out = y.size // 2
            assert n_out == rm.count(p["pos"], p["rstep"], n)
            d = self.desc[i]
            # (the least alignment of a packet, one sample, for every second contiguous one)
            d["src"] = self.arena.source(data, i, sb, skew=sb if stride == 1 and i % 2 else 0) + col_off
            d["dst"] = self.arena.row(n_out, 8, i)
            d["hist_in"], d["hist_out"] = self.arena.history(p.get("slot", i % 2), hist, i)
            d["stride"], d["n"], d["format"] = stride, n, fmt
            d["flags"] = (RS_RESTART if p["restart"] else 0) | (RS_TUNED if p["tune"] is not None else 0)
            if p["tune"] is not None:
                d["phase"], d["step"] = p["tune"][0] & tm.MASK, p["tune"][1] & tm.MASK
            d["pos"], d["rstep"], d["n_out"] = p["pos"], p["rstep"], n_out
            self._writes += [(int(d["dst"]), y), (int(d["hist_out"]), h_out)]
            self.rows.append(y)
            self.hists.append(h_out)
        self.max_n_out = int(self.desc["n_out"].max())
        self._finish()
        for d in self.desc:
            self._extents(int(d["src"]), SAMPLE_BYTES[int(d["format"])], int(d["stride"]), int(d["n"]), int(d["dst"]), 8, int(d["n_out"]))
            assert self.arena.inside("hist_in", int(d["hist_in"]), 24) and self.arena.inside("hist_out", int(d["hist_out"]), 24)
            assert (1 << 31) <= int(d["rstep"]) <= (1 << 33) and int(d["pos"]) <= (1 << 33)  # (what the entry lets through)

    def run(self):
        return _launch("resample", load().psk_prepass_probe_resample, self.image, self.desc.ctypes.data, len(self.desc), self.max_n_out)


class FirCase(_Case):
    """One launch of the filter kernel.  packets: dicts of fmt, stride (the packet is column i % stride of its matrix), iq
    (interleaved I/Q in the format's dtype), tune ((phase, step) or None), taps (1 .. 128 floats), D, pos (below D), restart,
    hist (254 floats in the slot that is read, or None: the handle's zeros), slot (which of the two is read; default i % 2)."""

    def __init__(self, packets):
        super().__init__()
        self.packets = packets
        self.desc = np.zeros(len(packets), FIR)
        self.rows, self.hists = [], []
        slot_bytes = 4 * constant("fir_hist_slot_floats")
        for i, p in enumerate(packets):
            fmt, stride, sb = p["fmt"], p["stride"], SAMPLE_BYTES[p["fmt"]]
            data, col_off = _strided(p["iq"], fmt, stride, i % stride)
            n = np.asarray(p["iq"]).size // 2
            x = np.ascontiguousarray(p["iq"], DTYPE_OF[fmt])[: 2 * n]
            s = x.astype(F32) if p["tune"] is None else tm.apply(p["tune"][0], p["tune"][1], x)
            taps = np.ascontiguousarray(p["taps"], F32).reshape(-1)
            hist = np.zeros(2 * fm.HIST, F32) if p["hist"] is None else np.asarray(p["hist"], F32)
            y, h_out = fm.apply(taps, p["D"], p["pos"], s, hist, p["restart"])
            d = self.desc[i]
            # (the least alignment of a packet, one sample, for every second contiguous one)
            d["src"] = self.arena.source(data, i, sb, skew=sb if stride == 1 and i % 2 else 0) + col_off
            d["taps"] = self.arena.source(taps, i, 4)
            d["dst"] = self.arena.row(y.size // 2, 8, i)
            d["hist_in"], d["hist_out"] = self.arena.history(p.get("slot", i % 2), hist, i, slot_bytes, FIR_HIST_BYTES)
            d["stride"], d["n"], d["format"] = stride, n, fmt
            d["flags"] = (RS_RESTART if p["restart"] else 0) | (RS_TUNED if p["tune"] is not None else 0)
            if p["tune"] is not None:
                d["phase"], d["step"] = p["tune"][0] & tm.MASK, p["tune"][1] & tm.MASK
            d["decim"], d["pos"], d["n_taps"], d["n_out"] = p["D"], p["pos"], taps.size, y.size // 2
            self._writes += [(int(d["dst"]), y), (int(d["hist_out"]), h_out)]
            self.rows.append(y)
            self.hists.append(h_out)
        self.pieces = [-(-int(d["n_out"]) // fir_piece(int(d["decim"]))) for d in self.desc]
        self.max_pieces = max(self.pieces)
        self._finish()
        a = self.arena
        for d in self.desc:
            D, T, pos, n, n_out = int(d["decim"]), int(d["n_taps"]), int(d["pos"]), int(d["n"]), int(d["n_out"])
            self._extents(int(d["src"]), SAMPLE_BYTES[int(d["format"])], int(d["stride"]), n, int(d["dst"]), 8, n_out)
            # (what the entry lets through: nothing is launched that the kernel's own guards would have to reject)
            assert 1 <= D <= fm.MAX_DECIM and 1 <= T <= fm.MAX_TAPS == constant("fir_max_taps") and 0 <= pos < D, (D, T, pos)
            assert n_out == fm.count(pos, D, n) and n < (1 << 30) and int(d["pad"]) == 0
            assert int(d["taps"]) % 4 == 0 and a.inside("source", int(d["taps"]), 4 * T)
            assert int(d["hist_in"]) % 8 == 0 and a.inside("hist_in", int(d["hist_in"]), FIR_HIST_BYTES)
            assert int(d["hist_out"]) % 8 == 0 and a.inside("hist_out", int(d["hist_out"]), FIR_HIST_BYTES)

    def run(self):
        return _launch("fir", load().psk_prepass_probe_fir, self.image, self.desc.ctypes.data, len(self.desc), self.max_pieces)


class TuneCase(_Case):
    """One launch of the tune kernel.  packets: dicts of fmt, stride, iq, phase, step."""

    def __init__(self, packets):
        super().__init__()
        self.packets = packets
        self.desc = np.zeros(len(packets), TUNE)
        self.rows = []
        for i, p in enumerate(packets):
            fmt, stride, sb = p["fmt"], p["stride"], SAMPLE_BYTES[p["fmt"]]
            data, col_off = _strided(p["iq"], fmt, stride, i % stride)
            n = np.asarray(p["iq"]).size // 2
            y = tm.apply(p["phase"], p["step"], np.ascontiguousarray(p["iq"], DTYPE_OF[fmt])[: 2 * n])
            d = self.desc[i]
            d["src"] = self.arena.source(data, i, sb, skew=sb if stride == 1 and i % 2 else 0) + col_off
            d["dst"] = self.arena.row(n, 8, i)
            d["stride"], d["n"], d["format"] = stride, n, fmt
            d["phase"], d["step"] = p["phase"] & tm.MASK, p["step"] & tm.MASK
            self._writes.append((int(d["dst"]), y))
            self.rows.append(y)
        self.max_n = int(self.desc["n"].max())
        self._finish()
        for d in self.desc:
            self._extents(int(d["src"]), SAMPLE_BYTES[int(d["format"])], int(d["stride"]), int(d["n"]), int(d["dst"]), 8, int(d["n"]))

    def run(self):
        """(the arena behind the launch, the device's tables behind it as (C, F), shaped like tune_model.tables())"""
        tab = np.zeros(constant("tune_table_floats"), F32)
        after = _launch("tune", load().psk_prepass_probe_tune, self.image, self.desc.ctypes.data, len(self.desc), self.max_n, tab.ctypes.data)
        return after, (tab[: tab.size // 2].reshape(-1, 2), tab[tab.size // 2 :].reshape(-1, 2))


class SinglesCase(_Case):
    """One launch of the plain strided gather.  sample_bytes 2, 4 or 8; packets: (n, stride); the samples are drawn here."""

    def __init__(self, sample_bytes, packets, seed):
        super().__init__()
        rng = np.random.default_rng(seed)
        self.sample_bytes = sb = sample_bytes
        self.desc = np.zeros(len(packets), SINGLE)
        for i, (n, stride) in enumerate(packets):
            mat = rng.integers(0, 256, (n, stride, sb), dtype=np.uint8)
            col = i % stride
            d = self.desc[i]
            d["src"] = self.arena.source(mat, i, sb, skew=sb if i % 2 else 0) + col * sb
            d["dst"] = self.arena.row(n, sb, i)
            d["stride"], d["n"] = stride, n
            self._writes.append((int(d["dst"]), mat[:, col, :]))
        self.max_n = int(self.desc["n"].max())
        self._finish()
        for d in self.desc:
            self._extents(int(d["src"]), sb, int(d["stride"]), int(d["n"]), int(d["dst"]), sb, int(d["n"]))

    def run(self):
        return _launch("gather_singles", load().psk_prepass_probe_gather_singles, self.image, self.sample_bytes, self.desc.ctypes.data,
                       len(self.desc), self.max_n)


class TilesCase(_Case):
    """One launch of the tile gather.  groups: (lengths of the g adjacent columns, columns of the matrix in front of them,
    columns behind them); the descriptors are filled as front_describe (psk_capi.cpp) fills them."""

    def __init__(self, sample_bytes, groups, seed):
        super().__init__()
        rng = np.random.default_rng(seed)
        tile = 64  # (kGatherTile: tests/test_prepass_probe.py holds it to the header's)
        self.sample_bytes = sb = sample_bytes
        self.groups = np.zeros(len(groups), GROUP)
        self.chans = np.zeros(sum(len(g[0]) for g in groups), CHAN)
        c_at, self.n_tiles = 0, 0
        for k, (lens, front, behind) in enumerate(groups):
            g, n_max, width = len(lens), max(lens), front + len(lens) + behind
            mat = rng.integers(0, 256, (n_max, width, sb), dtype=np.uint8)
            src = self.arena.source(mat, c_at, sb, skew=sb if k % 2 else 0) + front * sb
            G = self.groups[k]
            G["src"], G["stride"], G["n_max"], G["tile0"], G["first"], G["g"], G["tiles_c"] = src, width, n_max, self.n_tiles, c_at, g, -(-g // tile)
            self.n_tiles += int(G["tiles_c"]) * -(-n_max // tile)
            for j, n in enumerate(lens):
                c = self.chans[c_at]
                c["dst"], c["n"] = self.arena.row(n, sb, c_at), n
                self._writes.append((int(c["dst"]), mat[:n, front + j, :]))
                c_at += 1
        self._finish()
        for G in self.groups:
            for j in range(int(G["g"])):
                c = self.chans[int(G["first"]) + j]
                assert 1 <= int(c["n"]) <= int(G["n_max"])
                self._extents(int(G["src"]) + j * sb, sb, int(G["stride"]), int(c["n"]), int(c["dst"]), sb, int(c["n"]))

    def run(self):
        return _launch("gather_tiles", load().psk_prepass_probe_gather_tiles, self.image, self.sample_bytes, self.groups.ctypes.data,
                       len(self.groups), self.chans.ctypes.data, len(self.chans), self.n_tiles)


# ---- the two looks: fold and join, their partials and their records ----------------------------------------------------------------

LOOK_GRID_MAX = 65535  # packets a grid of launch_*_fold / launch_*_join covers in one trip (their literal)


def look_trips(n_desc):
    """trips of the packet loop `c += gridDim` of both folds and both joins: one up to 65535 descriptors"""
    return -(-n_desc // LOOK_GRID_MAX)


def _coprime(n, near):
    """a multiplier coprime to n, at or above `near`: i -> i * a % n is a permutation of range(n)"""
    a = max(1, near)
    while math.gcd(a, n) != 1:
        a += 1
    return a


class LookCase(_Case):
    """One launch of a look's fold and one of its join.  kind: "symrate" or "acquire".  protos: the distinct packets -- dicts of
    fmt, stride (the packet is column `col` of its matrix), iq (interleaved I/Q in the format's dtype), tune ((phase, step) or
    None), S (symrate) or M (acquire), skew (bytes in front of a contiguous packet: its least alignment); their models run once.
    uses: one (proto, data) per descriptor -- a descriptor without `data` has everything but its DATA flag and its source: the
    join gives it the zero record, the fold must leave its partials alone.

    The layout gives a wrong store something to hit: the descriptors take their partials in another order than their own (i ->
    i * a % n), with a slot nobody owns behind every `spare_every`-th; `channel` is a permutation with slots no descriptor names;
    the partials' pads, the unowned slots and a guard of 128 bytes behind each region are poison that has to come back."""

    def __init__(self, kind, protos, uses, spare_every=3, tables=True):
        super().__init__()
        self.kind, self.protos, self.uses, self.tables = kind, protos, uses, tables
        sym = kind == "symrate"
        self.desc_dt, self.part_dt, self.rec_dt = (SYMRATE_DESC, SYMRATE_PART, SYMRATE_REC) if sym else (ACQUIRE_DESC, ACQUIRE_PART, ACQUIRE_REC)
        self.piece = sm.PIECE if sym else am.PIECE
        psize, rsize, body = self.part_dt.itemsize, self.rec_dt.itemsize, self.part_dt.fields["pad"][1]
        a = self.arena
        for k, p in enumerate(protos):
            fmt, sb = p["fmt"], SAMPLE_BYTES[p["fmt"]]
            x = np.ascontiguousarray(p["iq"], DTYPE_OF[fmt])
            p["n"] = n = x.size // 2
            data, col_off = _strided(x, fmt, p["stride"], k % p["stride"])
            p["src"] = a.source(data, k, sb, skew=p.get("skew", 0) if p["stride"] == 1 else 0) + col_off
            tuned = p["tune"] is not None and (int(p["tune"][0]) | int(p["tune"][1])) != 0
            if sym:
                p["parts"] = sm.partials(x, p["S"], p["tune"])
                p["units"] = sm.n_blocks_of(n, p["S"])
                assert p["parts"], "a packet the look does not take"
                p["record"] = sm.join_bytes(p["parts"], n, p["S"], tuned)
            else:
                p["parts"] = am.device_partials(x, p["M"], p["tune"])
                p["units"] = n
                p["record"] = am.join_bytes(p["parts"], n, p["M"], tuned)
            p["flags"] = LOOK_DATA | (LOOK_TUNED if tuned else 0)
            p["part_bytes"] = [(sm if sym else am).partial_bytes(q) for q in p["parts"]]
            assert len(p["parts"]) == -(-p["units"] // self.piece) and len(p["record"]) == rsize and len(p["part_bytes"][0]) == body
        n = len(uses)
        self.desc = np.zeros(n, self.desc_dt)
        # the partials: descriptor order[0] takes the first slots, order[1] the next ..; a spare slot behind every spare_every-th
        mul = _coprime(n, int(0.618 * n))
        order = [(i * mul + n // 2) % n for i in range(n)]
        part0, spare, at = [0] * n, [], 0
        for j, i in enumerate(order):
            part0[i] = at
            at += len(protos[uses[i][0]]["parts"])
            if j % spare_every == spare_every - 1:
                spare.append(at)
                at += 1
        self.n_slots = at
        self.n_rec = n + max(2, n // 16)
        cmul = _coprime(self.n_rec, int(0.382 * self.n_rec))
        channel = [(i * cmul + 1) % self.n_rec for i in range(n)]
        self.part_off = a._place(np.full(self.n_slots * psize, ROW_BYTE, np.uint8))
        self.rec_off = a._place(np.full(self.n_rec * rsize, ROW_BYTE, np.uint8))
        R, zero = a.regions, bytes(rsize)
        for i, (k, data) in enumerate(uses):
            p = protos[k]
            for q in range(len(p["parts"])):
                o = self.part_off + (part0[i] + q) * psize
                if data:
                    R.append(Region(o, o + body, "partial", i, 4))
                    R.append(Region(o + body, o + psize, "partial_pad", i, 4))
                    self._writes.append((o, p["part_bytes"][q]))
                else:
                    R.append(Region(o, o + psize, "spare_partial", i, 4))
            o = self.rec_off + channel[i] * rsize
            R.append(Region(o, o + rsize, "record", i, 8))
            self._writes.append((o, p["record"] if data else zero))
        for sl in spare:
            R.append(Region(self.part_off + sl * psize, self.part_off + (sl + 1) * psize, "spare_partial", None, 4))
        for ch in sorted(set(range(self.n_rec)) - set(channel)):
            R.append(Region(self.rec_off + ch * rsize, self.rec_off + (ch + 1) * rsize, "spare_record", None, 8))
        d = self.desc
        pk = [protos[k] for k, _ in uses]
        d["src"] = [p["src"] if data else 0 for p, (_, data) in zip(pk, uses)]
        d["stride"], d["n"] = [p["stride"] for p in pk], [p["n"] for p in pk]
        d["phase"] = [p["tune"][0] & tm.MASK if p["flags"] & LOOK_TUNED else 0 for p in pk]
        d["step"] = [p["tune"][1] & tm.MASK if p["flags"] & LOOK_TUNED else 0 for p in pk]
        d["part0"], d["n_piece"], d["channel"] = part0, [len(p["parts"]) for p in pk], channel
        d["format"] = [p["fmt"] for p in pk]
        d["flags"] = [p["flags"] if data else p["flags"] & ~LOOK_DATA for p, (_, data) in zip(pk, uses)]
        if sym:
            d["S"], d["n_blocks"] = [p["S"] for p in pk], [p["units"] for p in pk]
            d["wstep"] = [(1 << 64) // p["S"] for p in pk]  # (sr_wstep: floor(2^64 / S))
        else:
            d["M"] = [p["M"] for p in pk]
        self.part0, self.channel, self.spare = part0, channel, spare
        self.max_piece = max(len(protos[k]["parts"]) for k, data in uses if data)
        self._finish()
        self._check_extents()

    def _check_extents(self):
        """what the two kernels may touch behind every descriptor lies where the arena has it"""
        a, d, sym = self.arena, self.desc, self.kind == "symrate"
        psize, rsize = self.part_dt.itemsize, self.rec_dt.itemsize
        assert self.part_off % 8 == 0 and self.rec_off % 8 == 0 and a.size < (1 << 31)
        assert len(set(self.channel)) == len(self.channel) and max(self.channel) < self.n_rec
        ends = np.asarray(d["part0"], np.int64) + np.asarray(d["n_piece"], np.int64)
        assert int(ends.max()) <= self.n_slots and int(d["n_piece"].min()) >= 1
        taken = np.zeros(self.n_slots, np.int32)
        for lo, hi in zip(d["part0"], ends):
            taken[lo:hi] += 1
        assert taken.max() == 1 and not taken[self.spare].any()
        assert a.inside("spare_partial", self.part_off + self.spare[0] * psize, psize) if self.spare else True
        seen = {}
        for i, (k, data) in enumerate(self.uses):
            if not data:
                assert int(d["src"][i]) == 0 and not int(d["flags"][i]) & LOOK_DATA
                continue
            p = self.protos[k]
            assert int(d["flags"][i]) & LOOK_DATA and (self.tables or not int(d["flags"][i]) & LOOK_TUNED)
            if k in seen:
                continue
            seen[k] = i
            sb, stride, n = SAMPLE_BYTES[p["fmt"]], p["stride"], p["n"]
            used = int(d["n_blocks"][i]) * int(d["S"][i]) if sym else n
            assert 1 <= used <= n and stride >= 1 and int(d["n_piece"][i]) == -(-p["units"] // self.piece)
            if sym:
                assert sm.MIN_S <= int(d["S"][i]) <= sm.MAX_S and 2 <= int(d["n_blocks"][i]) <= sm.MAX_BLOCKS
            else:
                assert int(d["M"][i]) in (2, 4, 8)
            src = int(d["src"][i])
            assert src % sb == 0 and a.inside("source", src, sb) and a.inside("source", src + (used - 1) * stride * sb, sb), (i, src, used)
            assert a.inside("partial", self.part_off + int(d["part0"][i]) * psize, psize - 4)
            assert a.inside("record", self.rec_off + int(d["channel"][i]) * rsize, rsize)

    def field(self, f):
        """the field of the partial or of the record a finding's first byte lies in"""
        if f["where"] in ("partial", "partial_pad", "spare_partial"):
            dt, at = self.part_dt, (f["offset"] - self.part_off) % self.part_dt.itemsize
        elif f["where"] in ("record", "spare_record"):
            dt, at = self.rec_dt, (f["offset"] - self.rec_off) % self.rec_dt.itemsize
        else:
            return None
        for name in dt.names:
            sub, off = dt.fields[name][:2]
            if off <= at < off + sub.itemsize:
                return "%s[%d]" % (name, (at - off) // sub.base.itemsize) if sub.shape else name
        return "padding"

    def check(self, after):
        found = self.arena.compare(self.want, after)
        for f in found:
            f["field"] = self.field(f)
            if f["field"]:
                f["message"] += " (%s)" % f["field"]
        return found

    def run(self):
        fn = load().psk_prepass_probe_symrate if self.kind == "symrate" else load().psk_prepass_probe_acquire
        extra = () if self.kind == "symrate" else (1 if self.tables else 0,)
        return _launch(self.kind, fn, self.image, self.desc.ctypes.data, len(self.desc), self.max_piece, self.part_off, self.rec_off, *extra)


# ---- the word search: fold and join (psk_sync.hip) -----------------------------------------------------------------------------------

SYNC_DATA, SYNC_RESTART = 1, 2  # SyncDesc::flags (psk_sync.h): kSyncData, kSyncRestart
SYNC_SLOT_BYTES, SYNC_HIST_BYTES = 1024, 8 * ym.HIST  # a history slot, and its payload: 127 float2
SYNC_WORD_BYTES = 8 * ym.MAX_WORD  # a word slot: 128 float2
NAN_WORD = 0x7FC00ABC  # a quiet NaN as poison: what must not be read shows in whatever is made of it
JOIN_CHUNK = 64  # partials the join takes a trip


def nan_poison(nbytes):
    assert nbytes % 4 == 0
    return np.frombuffer(np.full(nbytes // 4, NAN_WORD, "<u4").tobytes(), np.uint8)


def sync_grid(n_desc, max_piece):
    """Workgroups per channel, as front_grid_y (psk_front_src.h) has it for psk::launch_sync_fold: min(pieces of the channel
    with the most, ceil(2048 / n_desc)), at least 1, at most 65535.  2048 and the bounds are that function's literals."""
    per = min(max_piece, -(-2048 // n_desc))
    return max(1, min(per, 65535))


def sync_walk(n_piece, per):
    """the pieces each of the `per` workgroups of a channel takes (psk_sync_fold_kernel: p = blockIdx.x, p += gridDim.x)"""
    return [list(range(y, n_piece, per)) for y in range(per)]


class SyncCase(_Case):
    """One launch of the word search's fold, of its join, or of both (which: bit 0 the fold, bit 1 the join).  protos: the
    distinct rows, modelled once -- dicts of word (2 L floats), thr, x (2 n floats), restart, hist (254 floats in front of a
    continued row; None: zeros), skew (0 or 8 bytes past a line) --, or SYNTHETIC ones for the join alone: dicts of parts (partials
    as tests/sync_model.py has them), n, n_windows, L; their partials are in the arena before the launch, NaN poison in every
    member partial_writes does not list.  uses: one (proto, data) per descriptor; a descriptor without `data` is all zeros except
    `channel`, as sync_enqueue (psk_capi.cpp) builds it: it owns no partial and no history, its record is 456 zero bytes.

    The arena: the rows; the words, 128 float2 a slot with NaN behind L; a pair of history slots per searched descriptor -- the
    one read holds the history, NaN poison for a restarted row, which may not read it -- ; the partials, in another order than
    the descriptors' (i -> i * a % n) with a slot nobody owns behind every `spare_every`-th, NaN poison throughout; the records,
    `channel` a permutation with slots no descriptor names.  Expected: of a partial the members partial_writes lists and poison in
    the others, the model's 1016 bytes in hist_out and poison in its 8 pad bytes, join_bytes of the partials in the record, and
    everything else as it went up."""

    def __init__(self, protos, uses, spare_every=3, which=3):
        super().__init__()
        self.protos, self.uses, self.which = protos, uses, which
        psize, rsize = ym.PART_BYTES, ym.RECORD_BYTES
        a = self.arena
        words = {}
        for k, p in enumerate(protos):
            p["synthetic"] = "x" not in p
            if p["synthetic"]:
                assert which == 2, "synthetic partials are for the join alone"
            else:
                w, x = np.ascontiguousarray(p["word"], F32), np.ascontiguousarray(p["x"], F32)
                p["L"], p["n"] = w.size // 2, x.size // 2
                flags = ym.RESTART if p["restart"] else 0
                p["p0"], p["n_windows"] = ym.windows(p["n"], p["L"], p["restart"])
                p["parts"], p["hist_out"] = ym.partials_and_history(w, p["thr"], x, flags, p.get("hist"))
                p["Ew"] = ym.word_energy(w)
                p["src"] = a.source(x, k, 8, skew=p.get("skew", 0))
                key = w.tobytes()
                if key not in words:
                    slot = np.concatenate([np.frombuffer(key, np.uint8), nan_poison(SYNC_WORD_BYTES - len(key))])
                    words[key] = a.source(slot, "word L%d" % p["L"], 8)
                p["word_off"] = words[key]
            p["record"] = ym.join_bytes(p["parts"], p["n"], p["n_windows"], p["L"])
            p["writes"] = [ym.partial_writes(q) for q in p["parts"]]
            assert len(p["parts"]) == max(1, -(-p["n_windows"] // ym.PIECE)) and len(p["record"]) == rsize
        n = len(uses)
        self.desc = np.zeros(n, SYNC_DESC)
        searched = [i for i, (_, data) in enumerate(uses) if data]
        # the partials: searched descriptor order[0] takes the first slots, order[1] the next ..; a spare slot behind every spare_every-th
        m = len(searched)
        mul = _coprime(m, int(0.618 * m))
        order = [searched[(j * mul + m // 2) % m] for j in range(m)]
        part0, spare, at = [0] * n, [], 0
        for j, i in enumerate(order):
            part0[i] = at
            at += len(protos[uses[i][0]]["parts"])
            if j % spare_every == spare_every - 1:
                spare.append(at)
                at += 1
        self.n_slots = at
        self.n_rec = n + max(2, min(n // 16, 512))
        cmul = _coprime(self.n_rec, int(0.382 * self.n_rec))
        channel = [(i * cmul + 1) % self.n_rec for i in range(n)]
        hist_in, hist_out = [0] * n, [0] * n
        for i in searched:
            p = protos[uses[i][0]]
            if p["synthetic"]:
                continue
            h = p.get("hist")
            values = np.frombuffer(nan_poison(SYNC_HIST_BYTES).tobytes(), F32) if p["restart"] else np.zeros(2 * ym.HIST, F32) if h is None else h
            hist_in[i], hist_out[i] = a.history(i % 2, values, i, SYNC_SLOT_BYTES, SYNC_HIST_BYTES)
            self._writes.append((hist_out[i], p["hist_out"]))
        pimg = nan_poison(self.n_slots * psize).copy()
        for i in searched:
            p = protos[uses[i][0]]
            for q, writes in enumerate(p["writes"]):
                o = (part0[i] + q) * psize
                for off, b in writes:
                    if p["synthetic"]:
                        pimg[o + off: o + off + len(b)] = np.frombuffer(b, np.uint8)
        self.part_off = a._place(pimg)
        self.rec_off = a._place(np.full(self.n_rec * rsize, ROW_BYTE, np.uint8))
        R, zero = a.regions, bytes(rsize)
        for i, (k, data) in enumerate(uses):
            p = protos[k]
            if data:
                for q, writes in enumerate(p["writes"]):
                    o = self.part_off + (part0[i] + q) * psize
                    R.append(Region(o, o + psize, "partial", i, 4))
                    if which & 1:
                        self._writes += [(o + off, b) for off, b in writes]
            o = self.rec_off + channel[i] * rsize
            R.append(Region(o, o + rsize, "record", i, 8))
            if which & 2:
                self._writes.append((o, p["record"] if data else zero))
        for sl in spare:
            R.append(Region(self.part_off + sl * psize, self.part_off + (sl + 1) * psize, "spare_partial", None, 4))
        for ch in sorted(set(range(self.n_rec)) - set(channel)):
            R.append(Region(self.rec_off + ch * rsize, self.rec_off + (ch + 1) * rsize, "spare_record", None, 8))
        d = self.desc
        d["channel"] = channel
        pk = [protos[uses[i][0]] for i in searched]
        real = [not p["synthetic"] for p in pk]
        d["soft"][searched] = [p["src"] if r else 0 for p, r in zip(pk, real)]
        d["word"][searched] = [p["word_off"] if r else 0 for p, r in zip(pk, real)]
        d["hist_in"][searched], d["hist_out"][searched] = [hist_in[i] for i in searched], [hist_out[i] for i in searched]
        d["n"][searched], d["n_windows"][searched], d["L"][searched] = [p["n"] for p in pk], [p["n_windows"] for p in pk], [p["L"] for p in pk]
        d["p0"][searched] = [p["p0"] if r else 0 for p, r in zip(pk, real)]
        d["part0"][searched], d["n_piece"][searched] = [part0[i] for i in searched], [len(p["parts"]) for p in pk]
        d["flags"][searched] = [SYNC_DATA | (SYNC_RESTART if r and p["restart"] else 0) for p, r in zip(pk, real)]
        d["threshold"][searched] = [p["thr"] if r else 0.5 for p, r in zip(pk, real)]
        d["Ew"][searched] = [p["Ew"] if r else 1.0 for p, r in zip(pk, real)]
        self.part0, self.channel, self.spare, self.searched = part0, channel, spare, searched
        self.spare_channels = sorted(set(range(self.n_rec)) - set(channel))
        self.max_piece = max(len(p["parts"]) for p in pk)
        self.per = sync_grid(n, self.max_piece)
        self._finish()
        self._check_extents()

    def _check_extents(self):
        """what the two kernels may touch behind every descriptor lies where the arena has it"""
        a, d = self.arena, self.desc
        psize, rsize = ym.PART_BYTES, ym.RECORD_BYTES
        assert self.part_off % 8 == 0 and self.rec_off % 8 == 0 and a.size < (1 << 31) and self.which in (1, 2, 3)
        assert len(set(self.channel)) == len(self.channel) and max(self.channel) < self.n_rec
        assert a.size >= self.rec_off + self.n_rec * rsize + GUARD and self.rec_off >= self.part_off + self.n_slots * psize + GUARD
        taken = np.zeros(self.n_slots, np.int32)
        for i, (k, data) in enumerate(self.uses):
            x = d[i]
            assert a.inside("record", self.rec_off + int(x["channel"]) * rsize, rsize), i
            if not data:
                z = x.copy()
                z["channel"] = 0
                assert z.tobytes() == bytes(SYNC_DESC.itemsize), "a descriptor without data is zeros except its channel"
                continue
            p = self.protos[k]
            L, n, nw, np_ = int(x["L"]), int(x["n"]), int(x["n_windows"]), int(x["n_piece"])
            assert int(x["flags"]) & SYNC_DATA and 1 <= L <= ym.MAX_WORD and 1 <= n < (1 << 30), (i, L, n)
            assert np_ == max(1, -(-nw // ym.PIECE)) and int(x["part0"]) + np_ <= self.n_slots, (i, nw, np_)
            taken[int(x["part0"]): int(x["part0"]) + np_] += 1
            for q in (0, np_ - 1):
                assert a.inside("partial", self.part_off + (int(x["part0"]) + q) * psize, psize), (i, q)
            if p["synthetic"]:
                assert self.which == 2
                continue
            restart = bool(int(x["flags"]) & SYNC_RESTART)
            assert (int(x["p0"]), nw) == ym.windows(n, L, restart) and int(x["p0"]) == (0 if restart else -(L - 1))
            # the fold reads x[0 .. n-1] (the last window ends at p0 + nw - 1 + L - 1 = n - 1), w[0 .. L-1], the 127 symbols of
            # hist_in unless restarted, and writes 127 symbols of hist_out
            assert nw == 0 or int(x["p0"]) + nw - 1 + L - 1 == n - 1
            assert int(x["soft"]) % 8 == 0 and a.inside("source", int(x["soft"]), 8 * n), (i, n)
            assert int(x["word"]) % 8 == 0 and a.inside("source", int(x["word"]), 8 * L), (i, L)
            assert int(x["hist_in"]) % 8 == 0 and a.inside("hist_in", int(x["hist_in"]), SYNC_HIST_BYTES), i
            assert int(x["hist_out"]) % 8 == 0 and a.inside("hist_out", int(x["hist_out"]), SYNC_HIST_BYTES), i
        assert taken.max() == 1 and not taken[self.spare].any()
        for sl in self.spare[:1] + self.spare[-1:]:
            assert a.inside("spare_partial", self.part_off + sl * psize, psize)

    def partial_bytes(self, image, i, q):
        o = self.part_off + (self.part0[i] + q) * ym.PART_BYTES
        return image[o: o + ym.PART_BYTES].tobytes()

    def record_bytes(self, image, i):
        o = self.rec_off + self.channel[i] * ym.RECORD_BYTES
        return image[o: o + ym.RECORD_BYTES].tobytes()

    def field(self, f):
        """the member of the partial or of the record a finding's first byte lies in"""
        if f["where"] in ("partial", "spare_partial"):
            dt, at = ym.PART_DTYPE, (f["offset"] - self.part_off) % ym.PART_BYTES
        elif f["where"] in ("record", "spare_record"):
            dt, at = ym.RECORD_DTYPE, (f["offset"] - self.rec_off) % ym.RECORD_BYTES
        else:
            return None
        for name in dt.names:
            sub, off = dt.fields[name][:2]
            if off <= at < off + sub.itemsize:
                return "%s[%d]" % (name, (at - off) // sub.base.itemsize) if sub.shape else name
        return "padding"

    def check(self, after):
        found = self.arena.compare(self.want, after)
        for f in found:
            f["field"] = self.field(f)
            if f["field"]:
                f["message"] += " (%s)" % f["field"]
        return found

    def run(self):
        self._check_extents()
        return _launch("sync", load().psk_prepass_probe_sync, self.image, self.desc.ctypes.data, len(self.desc), self.max_piece, self.part_off,
                       self.rec_off, self.which)
