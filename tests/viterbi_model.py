"""The Viterbi decoder of include/psk_soft_hip.h ("frames as payload bits"), written from the header's text alone in numpy
integers: the code and its puncturing, the count of LLRs, the encoder, the decoder with its record, and a brute-force maximum over
every input sequence for tiny frames.  It shares no code with the library."""
import numpy as np

PACKED, TERMINATED, ANY_START = 1, 2, 4
DATA, PLANNED = 1, 128
MAX_STEPS = 65536
RECORD_BYTES, IN_BYTES = 64, 32
RECORD_DTYPE = np.dtype([("n_steps", "<u8"), ("n_llr", "<u8"), ("metric", "<i8"), ("sum_abs", "<i8"), ("n_flip", "<u4"), ("n_zero", "<u4"),
                         ("end_state", "<u4"), ("start_state", "<u4"), ("n_bits", "<u4"), ("flags", "<u4"), ("pad", "<u4", (2,))])
assert RECORD_DTYPE.itemsize == RECORD_BYTES

# the codes the tests share: (K, polynomials); the K = 7 pair is the 171/133 code, the others are the usual best codes of their K
CODES = {
    (3, 2): (0o7, 0o5), (3, 3): (0o7, 0o7, 0o5), (3, 4): (0o7, 0o7, 0o5, 0o5),
    (4, 2): (0o17, 0o15), (4, 3): (0o17, 0o15, 0o13), (4, 4): (0o17, 0o15, 0o15, 0o13),
    (5, 2): (0o35, 0o23), (5, 3): (0o37, 0o33, 0o25), (5, 4): (0o37, 0o35, 0o33, 0o25),
    (6, 2): (0o75, 0o53), (6, 3): (0o75, 0o53, 0o47), (6, 4): (0o75, 0o71, 0o67, 0o53),
    (7, 2): (0o171, 0o133), (7, 3): (0o171, 0o165, 0o133), (7, 4): (0o175, 0o171, 0o155, 0o133),
}
# the punctured rates of the K = 7 code, n = 2: (P, keep); bit p*2 + j of keep: code bit j of a step with t mod P == p is sent
#   2/3: [1 1; 1 0]   3/4: [1 1; 1 0; 0 1]   7/8: [1 1; 0 1; 0 1; 0 1; 1 0; 0 1; 1 0]   (rows: steps; columns: g0, g1)


def keep_of(rows):
    keep = 0
    n = len(rows[0])
    for p, row in enumerate(rows):
        for j, b in enumerate(row):
            keep |= b << (p * n + j)
    return len(rows), keep


PUNCTURED = {
    "1/2": (1, 3),
    "2/3": keep_of([(1, 1), (1, 0)]),
    "3/4": keep_of([(1, 1), (1, 0), (0, 1)]),
    "7/8": keep_of([(1, 1), (0, 1), (0, 1), (0, 1), (1, 0), (0, 1), (1, 0)]),
}


def parity(x):
    return bin(int(x)).count("1") & 1


def code_ok(K, g, P, keep):
    n = len(g)
    if not (3 <= K <= 7 and 2 <= n <= 4 and 1 <= P <= 16 and n * P <= 32):
        return False
    if keep <= 0 or keep >> (n * P):
        return False
    if any(p == 0 or p >> K for p in g):
        return False
    every = 0
    for p in g:
        every |= p
    return bool((every >> (K - 1)) & 1) and bool(every & 1)


def kept(n, P, keep, t):
    """the code bits j a step t carries"""
    return [j for j in range(n) if (keep >> ((t % P) * n + j)) & 1]


def count(n, P, keep, n_steps):
    per_period = bin(keep).count("1")
    full, rest = divmod(n_steps, P)
    return full * per_period + sum(len(kept(n, P, keep, t)) for t in range(rest))


def encode(K, g, P, keep, bits):
    """the kept code bits in order of (t, j), from state 0"""
    s, out = 0, []
    for t, u in enumerate(bits):
        r = (int(u) << (K - 1)) | s
        c = [parity(r & p) for p in g]
        out += [c[j] for j in kept(len(g), P, keep, t)]
        s = r >> 1
    return np.array(out, np.uint8)


def path_metric(K, g, P, keep, llr, bits, start=0):
    """sum of (c ? -l : +l) over the kept bits of the path the input bits take from state `start`; the state it ends in"""
    s, m, k = start, 0, 0
    for t, u in enumerate(bits):
        r = (int(u) << (K - 1)) | s
        for j in kept(len(g), P, keep, t):
            m += -int(llr[k]) if parity(r & g[j]) else int(llr[k])
            k += 1
        s = r >> 1
    return m, s


def brute_force(K, g, P, keep, llr, n_steps, flags=0):
    """the largest path metric over every input sequence (and, with ANY_START, every start state) that ends where the flags say"""
    best = None
    starts = range(1 << (K - 1)) if flags & ANY_START else (0,)
    for start in starts:
        for v in range(1 << n_steps):
            bits = [(v >> t) & 1 for t in range(n_steps)]
            m, end = path_metric(K, g, P, keep, llr, bits, start)
            if flags & TERMINATED and end != 0:
                continue
            best = m if best is None or m > best else best
    return best


def pack(bits):
    out = np.zeros((len(bits) + 7) // 8, np.uint8)
    for i, b in enumerate(bits):
        out[i >> 3] |= int(b) << (7 - (i & 7))
    return out


def decode(K, g, P, keep, llr, n_steps, flags=0):
    """(the output bytes, the record as RECORD_DTYPE) of one frame; llr: the frame's int8 LLRs"""
    assert code_ok(K, g, P, keep) and 0 < n_steps <= MAX_STEPS and not flags & ~7
    n, NS = len(g), 1 << (K - 1)
    mask = NS - 1
    assert not (flags & TERMINATED and n_steps < K - 1)
    l_all = np.asarray(llr).astype(np.int64)
    states = np.arange(NS)
    pred = [((states << 1) & mask) | b for b in (0, 1)]
    u_of = states >> (K - 2)
    # sign[b][s, j]: +1 where code bit j of the branch p_b -> s is 0, -1 where it is 1
    sign = []
    for b in (0, 1):
        r = (u_of << (K - 1)) | pred[b]
        sign.append(np.array([[-1 if parity(int(x) & p) else 1 for p in g] for x in r], np.int64))
    pm = np.full(NS, -(1 << 30), np.int64)
    pm[0] = 0
    if flags & ANY_START:
        pm[:] = 0
    dec = np.zeros((n_steps, NS), np.uint8)
    pos = np.zeros(n_steps + 1, np.int64)
    k = 0
    for t in range(n_steps):
        l = np.zeros(n, np.int64)
        for j in kept(n, P, keep, t):
            l[j] = l_all[k]
            k += 1
        pos[t + 1] = k
        a0, a1 = pm[pred[0]] + sign[0] @ l, pm[pred[1]] + sign[1] @ l
        d = a1 > a0
        pm = np.where(d, a1, a0)
        dec[t] = d
        assert pm.min() > -(1 << 31) and pm.max() < (1 << 31)  # (int32 holds every metric)
    s = 0 if flags & TERMINATED else int(np.argmax(pm))  # (argmax: the first maximum)
    end, metric = s, int(pm[s])
    n_bits = n_steps - (K - 1) if flags & TERMINATED else n_steps
    bits = np.zeros(n_steps, np.uint8)
    sum_abs = n_flip = n_zero = 0
    for t in range(n_steps - 1, -1, -1):
        u = s >> (K - 2)
        prev = ((s << 1) & mask) | int(dec[t, s])
        r = (u << (K - 1)) | prev
        for i, j in enumerate(kept(n, P, keep, t)):
            l = int(l_all[pos[t] + i])
            c = parity(r & g[j])
            sum_abs += abs(l)
            n_zero += l == 0
            n_flip += l != 0 and (l < 0) != (c == 1)
        bits[t] = u
        s = prev
    rec = np.zeros((), RECORD_DTYPE)
    rec["n_steps"], rec["n_llr"], rec["metric"], rec["sum_abs"] = n_steps, k, metric, sum_abs
    rec["n_flip"], rec["n_zero"], rec["end_state"], rec["start_state"] = n_flip, n_zero, end, s
    rec["n_bits"], rec["flags"] = n_bits, DATA | (flags << 1)
    out = bits[:n_bits]
    return (pack(out) if flags & PACKED else out.copy()), rec


def as_np(rec):
    """a ctypes record, or an array of them, as RECORD_DTYPE"""
    return np.frombuffer(bytes(rec), RECORD_DTYPE)


def assert_same(rec, model, ctx):
    """byte for byte; on a miss, name the first member that differs"""
    got = as_np(rec)[0]
    if got.tobytes() == model.tobytes():
        return
    for name in RECORD_DTYPE.names:
        assert got[name].tobytes() == model[name].tobytes(), "%s: %s differs: %r != %r" % (ctx, name, got[name], model[name])
    raise AssertionError(ctx)


def tie_llrs(rng, n_llr):
    """LLRs in -2 .. 2: paths tie at almost every step"""
    return rng.integers(-2, 3, n_llr).astype(np.int8)
