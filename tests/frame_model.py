"""A numpy model of psk_soft_frame_search_device and psk_soft_frame_cut_device (include/psk_soft_frame.h, "frames as aligned
bytes"), independent of the product's code: the stream is unpacked to one bit an element (np.unpackbits), the search compares a
sliding window view of it with the word's bits, the cut gathers bytes through a plain index array.  The convolutional byte
interleaver of the transmitter is here too.  The tests hold psk_soft_frame_search_host, psk_soft_frame_cut_host and the device to
it byte for byte, records included."""
import numpy as np

HIT_DTYPE = np.dtype([("pos", "<u4"), ("diff", "<u2"), ("pol", "u1"), ("zero", "u1")])
SEARCH_DTYPE = np.dtype(
    [
        ("flags", "<u4"),
        ("length", "<u4"),
        ("n_windows", "<u4"),
        ("n_hit", "<u4", (2,)),
        ("min_diff", "<u4"),
        ("min_pos", "<u4"),
        ("min_pol", "<u4"),
        ("best_phase", "<u4"),
        ("best_score", "<u4"),
        ("best_inv", "<u4"),
        ("n_listed", "<u4"),
        ("pad", "<u4", (4,)),
        ("hits", HIT_DTYPE, (16,)),
    ]
)
CUT_DTYPE = np.dtype([("flags", "<u4"), ("n_bytes", "<u4"), ("span", "<u4"), ("n_ones", "<u4"), ("pad", "<u4", (4,))])
SEARCH_BYTES, SEARCH_IN_BYTES, CUT_BYTES, CUT_IN_BYTES = 192, 48, 32, 48
SEARCH_OFFSETS = dict(flags=0, length=4, n_windows=8, n_hit=12, min_diff=20, min_pos=24, min_pol=28, best_phase=32, best_score=36,
                      best_inv=40, n_listed=44, pad=48, hits=64)
SEARCH_IN_OFFSETS = dict(bits=0, bit0=8, n_bits=16, word=20, max_diff=24, period=28, flags=32, pad=36)
CUT_OFFSETS = dict(flags=0, n_bytes=4, span=8, n_ones=12, pad=16)
CUT_IN_OFFSETS = dict(bits=0, bit=8, out=16, n_bytes=24, format=28, branch0=32, flags=36, pad=40)
HIT_OFFSETS = dict(pos=0, diff=4, pol=6, zero=7)
DATA, REC_INVERT, PLANNED, INVERT = 1, 2, 128, 1
HITS = 16

CCSDS_ASM = 0x1ACFFC1D
DVB_PERIOD, DVB_B, DVB_M = 1632, 12, 17


def stream_bits(buf, bit0, n_bits):
    """the stream bits of (buf, bit0): bit i is bit 7 - ((bit0 + i) & 7) of byte (bit0 + i) >> 3"""
    return np.unpackbits(np.ascontiguousarray(buf, np.uint8))[int(bit0) : int(bit0) + int(n_bits)]


def pack_at(bits, bit0, rng=None):
    """the bytes that hold `bits` from bit bit0 on; the bits around them random (rng) or zero"""
    n = int(bit0) + len(bits)
    total = 8 * ((n + 7) // 8)
    allb = np.zeros(total, np.uint8) if rng is None else rng.integers(0, 2, total).astype(np.uint8)
    allb[bit0:n] = bits
    return np.packbits(allb)


def word_bits(length, value):
    return np.array([(int(value) >> (length - 1 - j)) & 1 for j in range(length)], np.uint8)


def search(length, word, care, bits, max_diff, period):
    """the record of one stream whose bits (0 / 1, one an element) are `bits`: a SEARCH_DTYPE scalar array"""
    rec = np.zeros((), SEARCH_DTYPE)
    bits = np.asarray(bits, np.uint8)
    n_windows = max(0, len(bits) - length + 1)
    rec["flags"], rec["length"], rec["n_windows"] = DATA, length, n_windows
    if not n_windows:
        return rec
    w, c = word_bits(length, word), word_bits(length, care)
    C = int(c.sum())
    assert C >= 1 and 2 * max_diff < C
    win = np.lib.stride_tricks.sliding_window_view(bits, length)
    d = ((win ^ w) & c).sum(axis=1).astype(np.int64)
    diff = np.minimum(d, C - d)
    pol = (C - d < d).astype(np.int64)
    hit = diff <= max_diff
    rec["n_hit"] = [int((hit & (pol == 0)).sum()), int((hit & (pol == 1)).sum())]
    at = int(np.argmin(diff))  # (the first of the smallest)
    rec["min_diff"], rec["min_pos"], rec["min_pol"] = diff[at], at, pol[at]
    pos = np.flatnonzero(hit)
    if period:
        score = np.bincount(pos % period, minlength=period)
        best = int(np.argmax(score))  # (the first of the greatest)
        rec["best_phase"], rec["best_score"] = best, score[best]
        pos = pos[pos % period == best]
        rec["best_inv"] = int(pol[pos].sum())
    pos = pos[:HITS]
    rec["n_listed"] = len(pos)
    for k, p in enumerate(pos):
        rec["hits"][k] = (p, diff[p], pol[p], 0)
    return rec


def source_index(branches, cell, branch0, n_bytes):
    """the stream byte every output byte comes from"""
    i = np.arange(n_bytes, dtype=np.int64)
    if branches <= 1 or cell == 0:
        return i
    return i + ((branch0 + i) % branches) * cell * branches


def span(branches, cell, branch0, n_bytes):
    return int(source_index(branches, cell, branch0, n_bytes).max()) + 1


def cut(branches, cell, bits, n_bytes, branch0=0, table=None, flags=0):
    """(the output bytes, the CUT_DTYPE record) of a frame that starts at bits[0] (0 / 1, one an element)"""
    src = source_index(branches, cell, branch0, n_bytes)
    sp = int(src.max()) + 1
    stream = np.packbits(np.asarray(bits[: 8 * sp], np.uint8))
    assert len(stream) == sp, "the stream must hold the frame's span"
    out = stream[src] ^ np.uint8(0xFF if flags & INVERT else 0)
    if table is not None:
        out = np.asarray(table, np.uint8)[out]
    rec = np.zeros((), CUT_DTYPE)
    rec["flags"], rec["n_bytes"], rec["span"] = DATA | (flags << 1), n_bytes, sp
    rec["n_ones"] = int(np.unpackbits(out).sum())
    return out.astype(np.uint8), rec


def interleave(data, branches, cell, rng=None):
    """The transmitter's convolutional byte interleaver: byte k goes down branch k mod branches, which delays it by
    (k mod branches) * cell cells of `branches` bytes.  Returns len(data) + (branches - 1) * cell * branches bytes; what the delay
    lines held before the first byte is random (rng) or zero."""
    data = np.asarray(data, np.uint8)
    k = np.arange(len(data), dtype=np.int64)
    total = len(data) + (branches - 1) * cell * branches
    y = np.zeros(total, np.uint8) if rng is None else rng.integers(0, 256, total).astype(np.uint8)
    y[k + (k % branches) * cell * branches] = data
    return y


def record_bytes(rec):
    """a ctypes record or a numpy record as bytes"""
    return rec.tobytes() if isinstance(rec, np.ndarray) else bytes(rec)
