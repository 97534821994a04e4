"""The directed cases of the psk_soft_frame_ family, shared by tests/test_frame_control.py (the host definition against the model)
and tests/test_gpu_frame.py (the device against both), and the stream of the chain test.  A plain module: everything is built
once from fixed seeds and left unchanged."""
import functools

import numpy as np

from tests import frame_model as fm


class SearchCase:
    """one stream: the word, the stream's bits (0 / 1, one an element), the bit of its first byte at which it starts"""

    def __init__(self, label, length, word, care, bits, bit0=0, max_diff=0, period=0):
        self.label, self.length, self.word, self.care = label, length, int(word), int(care)
        self.bits, self.bit0, self.max_diff, self.period = np.asarray(bits, np.uint8), bit0, max_diff, period

    @property
    def n_bits(self):
        return len(self.bits)

    @functools.cached_property
    def want(self):
        return fm.search(self.length, self.word, self.care, self.bits, self.max_diff, self.period)

    def packed(self, rng=None):
        return fm.pack_at(self.bits, self.bit0, rng)


def plant(bits, pos, length, word, inverted=False):
    bits[pos : pos + length] = fm.word_bits(length, word) ^ (1 if inverted else 0)


def full(length):
    return (1 << length) - 1


def _rand_word(rng, length):
    return int.from_bytes(rng.bytes(8), "little") & full(length)


@functools.lru_cache(None)
def search_cases():
    rng = np.random.default_rng(1500)
    out = []
    # every length class, both ends of max_diff, every bit0 mod 8: windows of 33 .. 64 bits at a bit offset straddle three dwords
    for k, L in enumerate((1, 7, 8, 9, 31, 32, 33, 63, 64)):
        word = _rand_word(rng, L)
        bits = rng.integers(0, 2, 700 + 31 * k).astype(np.uint8)
        for pos in (5, 300, 301 + L):
            if pos + L <= len(bits):
                plant(bits, pos, L, word, inverted=pos == 300)
        for md in sorted({0, (L - 1) // 2}):
            out.append(SearchCase("L=%d max_diff=%d" % (L, md), L, word, full(L), bits, bit0=(3 * k + md) % 8 + 8 * (k % 3), max_diff=md))
    # care with holes
    for L, care in ((32, 0xF0F0FF0F), (64, 0x8000000000000001), (64, 0x00FFFF0000FFFF00), (9, 0b101010101), (33, 1 << 32 | 1)):
        word = _rand_word(rng, L)  # (the bits outside care are anything)
        bits = rng.integers(0, 2, 600).astype(np.uint8)
        plant(bits, 77, L, word)
        C = bin(care).count("1")
        out.append(SearchCase("holes L=%d care=%#x" % (L, care), L, word, care, bits, bit0=5, max_diff=(C - 1) // 2, period=0))
        out.append(SearchCase("holes L=%d care=%#x folded" % (L, care), L, word, care, bits, bit0=2, max_diff=0, period=11))
    # bit0 mod 8, long windows
    bits = rng.integers(0, 2, 900).astype(np.uint8)
    for b0 in range(8):
        plant(bits, 100 * b0 + 3, 64, 0x0123456789ABCDEF, inverted=b0 % 2 == 1)
    for b0 in range(8):
        out.append(SearchCase("bit0=%d L=64" % b0, 64, 0x0123456789ABCDEF, full(64), bits, bit0=b0, max_diff=3))
        out.append(SearchCase("bit0=%d L=32" % (b0 + 16), 32, fm.CCSDS_ASM, full(32), bits[: 500 + b0], bit0=b0 + 16, max_diff=2))
    # the ends of a stream
    for L in (1, 32, 64):
        word = _rand_word(rng, L)
        for n in (L - 1, L, L + 1):
            if n < 1:
                continue
            bits = rng.integers(0, 2, n).astype(np.uint8)
            if n >= L:
                plant(bits, n - L, L, word, inverted=L == 32)
            for P in (0, 3):
                out.append(SearchCase("n_bits=%d L=%d P=%d" % (n, L, P), L, word, full(L), bits, bit0=(n + L) % 8, period=P))
    # periods: 1, L - 1, a prime, n_windows, above n_windows
    L, word = 16, 0xEB90
    bits = rng.integers(0, 2, 16 + 13 * 40).astype(np.uint8)
    for m in range(0, 40, 3):
        plant(bits, 7 + 13 * m, L, word, inverted=m % 2 == 1)
    nw = len(bits) - L + 1
    for P in (1, L - 1, 13, 127, nw, nw + 1, nw + 500, 1 << 20):
        out.append(SearchCase("period=%d" % P, L, word, full(L), bits, bit0=P % 8, max_diff=1, period=P))
    # ties: every window of a stream of zeros is a hit of diff 0 (the first position is the minimum, the phases tie: phase 0 wins);
    # two phases with two hits each (the smaller wins); a minimum met twice
    zeros = np.zeros(4 + 7 * 30 - 1, np.uint8)
    out.append(SearchCase("tie: zeros", 4, 0, 0xF, zeros, bit0=3, period=7))
    out.append(SearchCase("tie: ones against zeros", 4, 0, 0xF, 1 - zeros, bit0=6, period=5))
    bits = rng.integers(0, 2, 2000).astype(np.uint8)
    for pos in (50 + 9, 50 + 100 + 9, 50 + 4, 50 + 300 + 4):
        plant(bits, pos, 32, fm.CCSDS_ASM)
    out.append(SearchCase("tie: two phases", 32, fm.CCSDS_ASM, full(32), bits, bit0=1, period=50))
    bits = rng.integers(0, 2, 800).astype(np.uint8)
    for pos in (400, 90):
        plant(bits, pos, 32, fm.CCSDS_ASM)
        bits[pos + 7] ^= 1
    out.append(SearchCase("tie: the minimum twice", 32, fm.CCSDS_ASM, full(32), bits, bit0=4, max_diff=0))
    # 0, 16 and 17 hits, unfolded and at one phase
    for hits in (0, 16, 17):
        bits = rng.integers(0, 2, 64 + 48 * 18).astype(np.uint8)
        for m in range(hits):
            plant(bits, 11 + 48 * m, 32, 0x35C1A7E2, inverted=m % 5 == 2)
        for P in (0, 48):
            c = SearchCase("%d hits P=%d" % (hits, P), 32, 0x35C1A7E2, full(32), bits, bit0=hits % 8, period=P)
            assert int(c.want["n_hit"].sum()) == hits and int(c.want["n_listed"]) == min(hits, 16), c.label
            out.append(c)
    return tuple(out)


def tile_edge_cases(tile):
    """phases across a tile edge, windows across a tile of windows (period 0: turns * tile windows)"""
    rng = np.random.default_rng(1501)
    out = []
    for P in (tile - 1, tile, tile + 1, 2 * tile + 1):
        bits = rng.integers(0, 2, 8 + 6 * P).astype(np.uint8)
        for phase in (P - 1, tile - 1 if tile - 1 < P else 0):
            for m in range(5):
                plant(bits, phase + m * P, 8, 0x47, inverted=m == 3)
        out.append(SearchCase("tile edge period=%d" % P, 8, 0x47, 0xFF, bits, bit0=P % 8, period=P))
    n = 256 * tile
    bits = rng.integers(0, 2, 2 * n + 100).astype(np.uint8)
    for pos in (n - 33, n - 32, n - 1, n, 2 * n - 1, 2 * n + 40):
        plant(bits, pos, 32, fm.CCSDS_ASM, inverted=pos == n)
    out.append(SearchCase("tiles of windows", 32, fm.CCSDS_ASM, full(32), bits, bit0=5, max_diff=1))
    out.append(SearchCase("tiles of windows, listed late", 32, fm.CCSDS_ASM, full(32), bits[n - 40 :], bit0=2, max_diff=0))
    return out


class CutCase:
    """one frame: the format, the stream's bits from the frame's first bit on (exactly its span), the bit of the stream's first byte
    at which it starts"""

    def __init__(self, label, branches, cell, n_bytes, bit, branch0=0, table=None, flags=0, seed=0):
        self.label, self.branches, self.cell, self.n_bytes, self.bit = label, branches, cell, n_bytes, bit
        self.branch0, self.table, self.flags = branch0, table, flags
        self.span = fm.span(branches, cell, branch0, n_bytes)
        self.bits = np.random.default_rng(seed).integers(0, 2, 8 * self.span).astype(np.uint8)

    @functools.cached_property
    def want(self):
        return fm.cut(self.branches, self.cell, self.bits, self.n_bytes, self.branch0, self.table, self.flags)

    def packed(self, rng=None):
        return fm.pack_at(self.bits, self.bit, rng)


SHAPES = ((12, 17), (1, 5), (5, 0), (2, 1), (3, 5))


@functools.lru_cache(None)
def cut_cases():
    rng = np.random.default_rng(1502)
    table = rng.permutation(256).astype(np.uint8)
    out = []
    seed = 0
    for bit in range(8):
        for n in (1, 3, 4, 5, 204, 1275):
            seed += 1
            out.append(CutCase("plain bit=%d n=%d" % (bit, n), 1, 0, n, bit + 8 * (n % 3), table=table if (bit + n) % 2 else None,
                               flags=(bit + n // 3) % 2, seed=seed))
    for B, M in SHAPES:
        for b0 in range(B):
            seed += 1
            n = 204 if (B, M) == (12, 17) else 1 + (7 * b0 + 11 * B) % 40
            out.append(CutCase("B=%d M=%d branch0=%d n=%d" % (B, M, b0, n), B, M, n, (b0 + B) % 8, branch0=b0,
                               table=table if b0 % 2 else None, flags=(b0 // 2) % 2, seed=seed))
    return tuple(out)


# ---- the chain: rs -> interleaver -> junk bits -> convolutional code -> LLRs ---------------------------------------------------------------

CHAIN_JUNK_BITS = 13
CHAIN_PACKETS = 24
CHAIN_TAIL_BYTES = 16  # behind the interleaver's output: the decoder's unterminated tail falls here, outside every frame


@functools.lru_cache(None)
def chain():
    """dict: data (CHAIN_PACKETS x 188, byte 0 the sync byte, inverted on every eighth packet), packets (x 204, byte errors in some),
    errors (bytes put wrong per packet), sent (the bits in front of the convolutional encoder), llr (int8, +-16, a fixed set of
    signs flipped)"""
    from psk_soft_amd import lib as pl
    from tests import viterbi_model as vm

    rng = np.random.default_rng(1503)
    data = rng.integers(0, 256, (CHAIN_PACKETS, 188)).astype(np.uint8)
    data[:, 0] = 0x47
    data[::8, 0] = 0xB8
    packets = np.stack([pl.rs_encode_host(*pl.RS_DVB, 1, d) for d in data])
    errors = [(0, 1, 8, 3)[q % 4] for q in range(CHAIN_PACKETS)]
    for q, e in enumerate(errors):
        at = 1 + rng.choice(203, e, replace=False)  # (the sync byte stays: the search is not what the outer code is tested on)
        packets[q, at] ^= rng.integers(1, 256, e).astype(np.uint8)
    # (the delay lines start with zeros: behind the last packet the sync byte's branch carries no look-alike)
    stream = np.concatenate([fm.interleave(packets.reshape(-1), fm.DVB_B, fm.DVB_M), rng.integers(0, 256, CHAIN_TAIL_BYTES).astype(np.uint8)])
    sent = np.concatenate([rng.integers(0, 2, CHAIN_JUNK_BITS).astype(np.uint8), np.unpackbits(stream)])
    K, g = 7, vm.CODES[(7, 2)]
    code_bits = pl.viterbi_encode(K, g, 1, 3, sent)
    llr = np.where(code_bits == 0, 16, -16).astype(np.int8)
    flip = np.arange(37, llr.size, 211)  # (one in 211, far apart against the code's free distance of 10)
    llr[flip] = -llr[flip]
    return dict(data=data, packets=packets, errors=errors, sent=sent, llr=llr, K=K, g=g, n_steps=len(sent))
