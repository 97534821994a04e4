"""A numpy model of psk_soft_rs_device (include/psk_soft_rs.h, "frames as corrected bytes"), independent of the product's
algorithm: exp / log tables for the field, the locator from the syndromes' Hankel matrix by Gaussian elimination
(Peterson-Gorenstein-Zierler: with v <= t errors the t x t matrix has rank v), its roots by trying every one of the n
positions, the error values by solving the Vandermonde system by Gaussian elimination -- no Berlekamp-Massey, no Forney.  Whatever
it returns as decoded it has checked against the definition itself: the result has zero syndromes and differs from the received
word in at most t bytes, all inside the n positions; otherwise the codeword is FAILED.  The encoder is here too."""
import functools
import math

import numpy as np

FAILED = 255
WITH_PARITY = 1
DATA, PLANNED = 1, 128
RECORD_BYTES, IN_BYTES = 64, 32
RECORD_DTYPE = np.dtype([("flags", "<u4"), ("n", "<u2"), ("k", "<u2"), ("depth", "u1"), ("nroots", "u1"), ("pad0", "u1", 6),
                         ("n_err", "u1", 8), ("n_bit", "<u2", 8), ("pad1", "u1", 24)])
CCSDS = (0x187, 112, 11, 32, 255)  # gfpoly, fcr, prim, nroots, n
DVB = (0x11D, 0, 1, 16, 204)
PRIMITIVE_POLYS = (0x11D, 0x12B, 0x12D, 0x14D, 0x15F, 0x163, 0x165, 0x169, 0x171, 0x187, 0x18D, 0x1A9, 0x1C3, 0x1CF, 0x1E7, 0x1F5)


@functools.lru_cache(maxsize=None)
def tables(gfpoly):
    """(exp of 512 entries, log of 256) of GF(2)[x] / gfpoly with alpha = 2; raises unless alpha has order 255"""
    exp = np.zeros(512, np.int64)
    log = np.zeros(256, np.int64)
    a = 1
    for i in range(255):
        if i and a == 1:
            raise ValueError("alpha has an order below 255")
        exp[i] = a
        log[a] = i
        a <<= 1
        if a & 0x100:
            a ^= gfpoly
    if a != 1:
        raise ValueError("alpha does not return to 1")
    exp[255:510] = exp[:255]
    return exp, log


def is_primitive(gfpoly):
    try:
        tables(gfpoly)
        return True
    except ValueError:
        return False


def mul(gfpoly, a, b):
    """element-wise product of integer arrays (or scalars)"""
    exp, log = tables(gfpoly)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a == 0) | (b == 0), 0, exp[log[a] + log[b]])


def inv(gfpoly, a):
    exp, log = tables(gfpoly)
    assert a != 0
    return int(exp[(255 - log[a]) % 255])


def apow(gfpoly, e):
    return int(tables(gfpoly)[0][e % 255])


class Code:
    def __init__(self, gfpoly, fcr, prim, nroots, n=255, depth=1, mask=None):
        assert 0x100 <= gfpoly <= 0x1FF and is_primitive(gfpoly)
        assert 0 <= fcr <= 254 and 1 <= prim <= 254 and math.gcd(prim, 255) == 1
        assert 2 <= nroots <= 64 and nroots + 1 <= n <= 255 and 1 <= depth <= 8
        self.gfpoly, self.fcr, self.prim, self.nroots, self.n, self.depth = gfpoly, fcr, prim, nroots, n, depth
        self.k, self.t = n - nroots, nroots // 2
        self.mask = np.zeros(0, np.uint8) if mask is None else np.asarray(mask, np.uint8).reshape(-1)
        assert self.mask.size <= n * depth
        self.roots = [apow(gfpoly, prim * (fcr + m)) for m in range(nroots)]
        # powers[m, i] = root_m^(n-1-i): what byte i contributes to syndrome m
        exp, log = tables(gfpoly)
        e = (np.array([prim * (fcr + m) for m in range(nroots)], np.int64)[:, None] * (n - 1 - np.arange(n))[None, :]) % 255
        self.powers = exp[e]
        # the generator, g[d] the coefficient of x^d
        g = [1]
        for r in self.roots:
            g = [0] + g
            for d in range(len(g) - 1):
                g[d] ^= int(mul(gfpoly, g[d + 1], r))
        self.g = g

    @property
    def args(self):
        """the code arguments of the host entries"""
        return (self.gfpoly, self.fcr, self.prim, self.nroots, self.n, self.depth)

    def syndromes(self, word):
        """the nroots syndromes of a word of n bytes"""
        prod = mul(self.gfpoly, self.powers, np.asarray(word, np.int64)[None, :])
        return np.bitwise_xor.reduce(prod, axis=1)

    def apply_mask(self, frame):
        out = np.array(frame, np.uint8).reshape(-1).copy()
        out[: self.mask.size] ^= self.mask
        return out

    def encode_word(self, data):
        """a codeword of n bytes from k data bytes: the parity is the remainder of d(x) x^nroots by g(x)"""
        g = np.array(self.g[: self.nroots], np.int64)
        par = np.zeros(self.nroots, np.int64)  # par[d]: the coefficient of x^d
        for b in np.asarray(data, np.int64):
            fb = int(b ^ par[-1])
            par = np.concatenate([[0], par[:-1]]) ^ mul(self.gfpoly, g, fb)
        return np.concatenate([np.asarray(data, np.uint8), par[::-1].astype(np.uint8)])

    def encode(self, data):
        """the frame (n * depth bytes, interleaved, masked) of k * depth data bytes, data[i * depth + j] byte i of codeword j"""
        data = np.asarray(data, np.uint8).reshape(self.k, self.depth)
        frame = np.stack([self.encode_word(data[:, j]) for j in range(self.depth)], axis=1).reshape(-1)
        return self.apply_mask(frame)

    def g_shifted(self, s):
        """g(x) x^s as a word of n bytes: a codeword; s = 0 .. k-1"""
        w = np.zeros(self.n, np.uint8)
        for d, c in enumerate(self.g):
            w[self.n - 1 - (d + s)] = c
        return w

    def _solve(self, A, b):
        """x with A x = b over the field by Gaussian elimination, A square; None if singular"""
        gp = self.gfpoly
        v = A.shape[0]
        M = np.concatenate([A, b[:, None]], axis=1).astype(np.int64)
        for c in range(v):
            piv = next((r for r in range(c, v) if M[r, c]), None)
            if piv is None:
                return None
            M[[c, piv]] = M[[piv, c]]
            M[c] = mul(gp, M[c], inv(gp, int(M[c, c])))
            for r in range(v):
                if r != c and M[r, c]:
                    M[r] ^= mul(gp, M[c], M[r, c])
        return M[:, v]

    def _rank(self, A):
        gp = self.gfpoly
        M = A.astype(np.int64).copy()
        rank = 0
        for c in range(M.shape[1]):
            piv = next((r for r in range(rank, M.shape[0]) if M[r, c]), None)
            if piv is None:
                continue
            M[[rank, piv]] = M[[piv, rank]]
            M[rank] = mul(gp, M[rank], inv(gp, int(M[rank, c])))
            for r in range(rank + 1, M.shape[0]):
                if M[r, c]:
                    M[r] ^= mul(gp, M[rank], M[r, c])
            rank += 1
        return rank

    def decode_word(self, word):
        """(the result word, n_err, n_bit) of a received word of n bytes, by the definition"""
        gp, n, t = self.gfpoly, self.n, self.t
        word = np.asarray(word, np.uint8)
        S = self.syndromes(word)
        if not S.any():
            return word.copy(), 0, 0
        failed = (word.copy(), FAILED, 0)
        if t == 0:
            return failed
        H = np.array([[S[a + b] for b in range(t)] for a in range(t)], np.int64)
        v = self._rank(H)
        if v == 0:
            return failed
        # sigma_1 .. sigma_v with S[a + v] = sum_b sigma_(b+1) S[a + v - 1 - b], a = 0 .. v-1
        A = np.array([[S[a + v - 1 - b] for b in range(v)] for a in range(v)], np.int64)
        sig = self._solve(A, np.array([S[a + v] for a in range(v)], np.int64))
        if sig is None:
            return failed
        # the positions i whose locator X = beta^(n-1-i) has Lambda(1 / X) = 0, Lambda = 1 + sigma_1 x + ...
        exp, log = tables(gp)
        p = n - 1 - np.arange(n)
        xinv = exp[(255 - (self.prim * p) % 255) % 255]
        val = np.ones(n, np.int64)
        xp = np.ones(n, np.int64)
        for d in range(v):
            xp = mul(gp, xp, xinv)
            val ^= mul(gp, xp, int(sig[d]))
        pos = np.flatnonzero(val == 0)
        if pos.size != v:
            return failed
        # the values: sum_p e_p root_m^(n-1-i_p) = S_m for m = 0 .. v-1
        e = self._solve(self.powers[:v][:, pos], S[:v])
        if e is None:
            return failed
        out = word.copy()
        out[pos] ^= e.astype(np.uint8)
        # the definition itself
        diff = out != word
        if self.syndromes(out).any() or int(diff.sum()) > t:
            return failed
        return out, int(diff.sum()), int(np.unpackbits(out ^ word).sum())

    def decode(self, frame, flags=0):
        """(the output bytes, the record as a RECORD_DTYPE scalar) of one frame of n * depth bytes"""
        n, I = self.n, self.depth
        rx = self.apply_mask(np.asarray(frame, np.uint8).reshape(-1)[: n * I]).reshape(n, I)
        rec = np.zeros((), RECORD_DTYPE)
        res = np.zeros((n, I), np.uint8)
        for j in range(I):
            res[:, j], rec["n_err"][j], rec["n_bit"][j] = self.decode_word(rx[:, j])
        rec["flags"] = DATA | flags << 1
        rec["n"], rec["k"], rec["depth"], rec["nroots"] = n, self.k, I, self.nroots
        return res[: n if flags & WITH_PARITY else self.k].reshape(-1).copy(), rec


def assert_same(rec, mrec, ctx=""):
    """a ctypes record of the library against a model record, byte for byte"""
    got = bytes(rec)
    want = mrec.tobytes()
    assert len(got) == len(want) == RECORD_BYTES
    if got != want:
        g = np.frombuffer(got, RECORD_DTYPE)[0]
        raise AssertionError("%s: record differs: got %s, want %s" % (ctx, g, mrec))


def random_code(rng, depth=None, mask=True):
    """a code drawn over every parameter"""
    gfpoly = int(rng.choice(PRIMITIVE_POLYS))
    prim = int(rng.choice([p for p in range(1, 255) if math.gcd(p, 255) == 1]))
    nroots = int(rng.integers(2, 65))
    n = int(rng.integers(nroots + 1, 256))
    depth = int(rng.integers(1, 9)) if depth is None else depth
    m = rng.integers(0, 256, int(rng.integers(0, n * depth + 1))).astype(np.uint8) if mask else None
    return Code(gfpoly, int(rng.integers(0, 255)), prim, nroots, n, depth, m)


def corrupt(rng, frame, code, j, count, values=None):
    """`count` distinct bytes of codeword j of a frame changed (by random non-zero values, or by `values`); returns the positions"""
    pos = rng.choice(code.n, count, replace=False)
    for q, i in enumerate(pos):
        frame[i * code.depth + j] ^= int(rng.integers(1, 256)) if values is None else values[q % len(values)]
    return pos


def directed_cases(rng, code, encode=None):
    """[(label, frame)]: the directed cases of one code, each on a frame of fresh random data whose other codewords carry 0 .. t
    random errors; the case itself is on codeword (case number) mod depth.  Error counts 0, 1, t, t+1 with the values 1 and 0xff;
    the positions 0, k-1, k, n-1, 63, 64; the neighbour case (even nroots: the codeword plus t+1 of the non-zero bytes of a shifted
    g(x), which lies t from the neighbour c + g); the pad case (a shortened code with t zero bytes or more in front: the part
    inside the n positions of g(x) shifted t bytes into the pad, t+1 from c, which the full-length code would correct into the
    pad).  What each must give is the model's to say.  encode: the encoder to use (data -> frame), the model's own by default."""
    n, k, t, I = code.n, code.k, code.t, code.depth
    cases = []

    def fresh(label, edit):
        j = len(cases) % I
        frame = (encode or code.encode)(rng.integers(0, 256, k * I).astype(np.uint8))
        for o in range(I):
            if o != j:
                corrupt(rng, frame, code, o, int(rng.integers(0, t + 1)))
        for i, v in edit:
            frame[i * I + j] ^= v
        cases.append((label, frame))

    fresh("clean", [])
    for v in (1, 0xFF):
        for cnt in sorted({1, t, t + 1}):
            if cnt <= n:
                fresh("%d errors of value %d" % (cnt, v), [(int(i), v) for i in rng.choice(n, cnt, replace=False)])
    edge = sorted({i for i in (0, k - 1, k, n - 1, 63, 64) if i < n})
    for i in edge:
        fresh("one error at %d" % i, [(i, int(rng.integers(1, 256)))])
    fresh("errors at the first %d of %s" % (t, edge), [(i, int(rng.integers(1, 256))) for i in edge[:t]])
    if code.nroots % 2 == 0:
        gs = code.g_shifted(int(rng.integers(0, k)))
        nz = np.flatnonzero(gs)
        assert nz.size == code.nroots + 1  # (the code is MDS: g has no zero coefficient)
        fresh("neighbour", [(int(i), int(gs[i])) for i in rng.choice(nz, t + 1, replace=False)])
    if 255 - n >= t:
        s = k - 1 + t  # g(x) x^s: its top t coefficients lie in the pad
        fresh("pad", [(n - 1 - (d + s), code.g[d]) for d in range(code.nroots + 1) if d + s <= n - 1])
    return cases
