"""The definition of include/psk_soft_hip.h, "where frames start", restated in numpy: float32 throughout, every operation rounded
once (numpy rounds each elementwise operation; nothing here can fuse), the loop over j = 0 .. L-1 in that order vectorised over the
windows, hits and best by the header's rules.  The tests hold psk_soft_sync_host and the device to it byte for byte.

partials / partial_writes / join_bytes state what one piece of the device's fold leaves in its SyncPartial and what the join may
read of it: the probe (tests/prepass_probe.py) holds the partials, the histories and the records of the kernels alone to them.

Also the stimulus of the issue's three oracle cases (a word written into random PSK data every `period` symbols) and helpers that
read a record."""
import math

import numpy as np

F32 = np.float32
MAX_WORD, HITS, HIST = 128, 16, 127
HIST_FLOATS = 2 * HIST
RECORD_BYTES, IN_BYTES, HIT_BYTES = 456, 32, 24
PIECE, THREADS = 1024, 256
RESTART = 1
DATA, PLANNED = 1, 128
FLT_MIN = F32(np.finfo(np.float32).tiny)

HIT_DTYPE = np.dtype([("pos", "<i8"), ("cr", "<f4"), ("ci", "<f4"), ("e", "<f4"), ("m", "<f4")])
RECORD_DTYPE = np.dtype([("n_symbols", "<u8"), ("n_windows", "<u8"), ("n_valid", "<u8"), ("n_hits", "<u8"), ("best", HIT_DTYPE),
                         ("hits", HIT_DTYPE, (HITS,)), ("word_len", "<u4"), ("flags", "<u4"), ("pad", "<u4", (2,))])
assert HIT_DTYPE.itemsize == HIT_BYTES and RECORD_DTYPE.itemsize == RECORD_BYTES


def word_energy(word):
    """Ew: the float32 sum, in index order, of wr*wr + wi*wi"""
    w = np.ascontiguousarray(word, F32).reshape(-1, 2)
    t = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]
    s = t[0]
    for v in t[1:]:
        s = F32(s + v)
    return F32(s)


def windows(n, L, restart):
    """(p0, n_windows)"""
    p0 = 0 if restart else -(L - 1)
    return p0, max(0, n - L - p0 + 1)


def model_windows(word, soft, flags=0, hist_in=None):
    """every window of the row: (pos int64, cr, ci, e, m float32, valid bool), and the history behind the row (254 float32)"""
    w = np.ascontiguousarray(word, F32).reshape(-1, 2)
    x = np.ascontiguousarray(soft, F32).reshape(-1, 2)
    L, n = len(w), len(x)
    restart = bool(flags & RESTART)
    hist = np.zeros((HIST, 2), F32)
    if hist_in is not None and not (restart and n):
        hist = np.ascontiguousarray(hist_in, F32).reshape(HIST, 2).copy()
    if n == 0:
        z = np.zeros(0, F32)
        return np.zeros(0, np.int64), z, z, z, z, np.zeros(0, bool), hist.reshape(-1).copy()
    full = np.concatenate([hist, x])  # full[HIST + g] = x[g]
    p0, nw = windows(n, L, restart)
    pos = p0 + np.arange(nw, dtype=np.int64)
    cr = ci = e = None
    with np.errstate(all="ignore"):
        xe = full[:, 0] * full[:, 0] + full[:, 1] * full[:, 1]  # te of every symbol
        for j in range(L):
            seg = full[HIST + p0 + j: HIST + p0 + j + nw]
            tr = seg[:, 0] * w[j, 0] + seg[:, 1] * w[j, 1]
            ti = seg[:, 1] * w[j, 0] - seg[:, 0] * w[j, 1]
            te = xe[HIST + p0 + j: HIST + p0 + j + nw]
            if j == 0:
                cr, ci, e = tr.copy(), ti.copy(), te.copy()
            else:
                cr, ci, e = cr + tr, ci + ti, e + te
        q = cr * cr + ci * ci
        d = e * word_energy(word)
        m = q / d
        valid = np.isfinite(cr) & np.isfinite(ci) & np.isfinite(e) & np.isfinite(q) & np.isfinite(d) & (d >= FLT_MIN)
    assert all(a.dtype == F32 for a in (cr, ci, e, q, d, m))
    new_hist = full[len(full) - HIST:].reshape(-1).copy()
    return pos, cr, ci, e, m, valid, new_hist


def model_record(word, threshold, soft, flags=0, hist_in=None):
    """(the record as a numpy scalar of RECORD_DTYPE, the history behind the row)"""
    pos, cr, ci, e, m, valid, new_hist = model_windows(word, soft, flags, hist_in)
    rec = np.zeros((), RECORD_DTYPE)
    n = np.ascontiguousarray(soft, F32).size // 2
    if n == 0:
        return rec, new_hist
    rec["n_symbols"], rec["n_windows"] = n, len(pos)
    rec["word_len"], rec["flags"] = np.ascontiguousarray(word, F32).size // 2, DATA

    def put(slot, k):
        slot["pos"], slot["cr"], slot["ci"], slot["e"], slot["m"] = pos[k], cr[k], ci[k], e[k], m[k]

    vi = np.flatnonzero(valid)
    rec["n_valid"] = len(vi)
    if len(vi):
        put(rec["best"], vi[np.argmax(m[vi])])  # (argmax: the first of equal maxima; m of a valid window is never NaN)
    with np.errstate(invalid="ignore"):
        hi = np.flatnonzero(valid & (m >= F32(threshold)))
    rec["n_hits"] = len(hi)
    for s, k in enumerate(hi[:HITS]):
        put(rec["hits"][s], k)
    return rec, new_hist


# ---- what a piece of the device's fold leaves, and what its join may read (psk_sync.h: SyncPartial) --------------------------------

PART_DTYPE = np.dtype([("n_valid", "<u4"), ("n_hits", "<u4"), ("best", HIT_DTYPE), ("hits", HIT_DTYPE, (HITS,))])
PART_BYTES = PART_DTYPE.itemsize
assert PART_BYTES == 8 + HIT_BYTES * (1 + HITS)


def partials_and_history(word, threshold, soft, flags=0, hist_in=None):
    """(one partial per piece of PIECE windows -- one for a row without a window --, the history behind the row).  A partial is a
    dict: n_valid, n_hits, best (a HIT_DTYPE scalar: the piece's first maximum; None without a valid window), hits (the piece's
    first min(n_hits, 16) hits, an array of HIT_DTYPE)."""
    pos, cr, ci, e, m, valid, new_hist = model_windows(word, soft, flags, hist_in)
    with np.errstate(invalid="ignore"):
        hit = valid & (m >= F32(threshold))
    every = np.zeros(len(pos), HIT_DTYPE)
    every["pos"], every["cr"], every["ci"], every["e"], every["m"] = pos, cr, ci, e, m
    out = []
    for lo in range(0, max(len(pos), 1), PIECE):
        hi = min(lo + PIECE, len(pos))
        vi = lo + np.flatnonzero(valid[lo:hi])
        hk = lo + np.flatnonzero(hit[lo:hi])
        best = every[vi[np.argmax(m[vi])]].copy() if len(vi) else None  # (argmax: the first of equal maxima)
        out.append(dict(n_valid=len(vi), n_hits=len(hk), best=best, hits=every[hk[:HITS]].copy()))
    return out, new_hist


def partials(word, threshold, soft, flags=0, hist_in=None):
    return partials_and_history(word, threshold, soft, flags, hist_in)[0]


def partial_writes(p):
    """the (offset, bytes) pairs the owner of a partial stores, and nothing else: the two counts always, `best` only with a valid
    window, hits[k] only for k < min(n_hits, 16)"""
    out = [(0, np.array([p["n_valid"], p["n_hits"]], "<u4").tobytes())]
    if p["n_valid"]:
        out.append((PART_DTYPE.fields["best"][1], p["best"].tobytes()))
    k = min(int(p["n_hits"]), HITS)
    assert len(p["hits"]) >= k
    if k:
        out.append((PART_DTYPE.fields["hits"][1], p["hits"][:k].tobytes()))
    return out


def join_bytes(parts, n, n_windows, L):
    """the 456 bytes of the record from the partials alone, in piece order; it reads of a partial what the join may read: the
    counts, `best` where n_valid != 0, hits[k] for k < min(n_hits, 16).  A later best must be greater."""
    rec = np.zeros((), RECORD_DTYPE)
    rec["n_symbols"], rec["n_windows"], rec["word_len"], rec["flags"] = n, n_windows, L, DATA
    nv = nh = 0
    best = None
    for p in parts:
        k = min(int(p["n_hits"]), HITS)
        if k and nh < HITS:
            take = min(k, HITS - nh)
            rec["hits"][nh: nh + take] = p["hits"][:take]
        if p["n_valid"] and (best is None or p["best"]["m"] > best["m"]):
            best = p["best"]
        nv, nh = nv + int(p["n_valid"]), nh + int(p["n_hits"])
    rec["n_valid"], rec["n_hits"] = nv, nh
    if best is not None:
        rec["best"] = best
    return rec.tobytes()


def as_np(rec):
    """a ctypes SyncRecord (or an array of them) as numpy of RECORD_DTYPE"""
    return np.frombuffer(bytes(rec), RECORD_DTYPE)


def assert_same(rec, model, ctx):
    """byte for byte; on a miss, name the first member that differs"""
    got = as_np(rec)[0]
    if got.tobytes() == model.tobytes():
        return
    for name in RECORD_DTYPE.names:
        assert got[name].tobytes() == model[name].tobytes(), "%s: %s differs: %r != %r" % (ctx, name, got[name], model[name])
    raise AssertionError(ctx)


def hits_of(rec):
    """[(pos, cr, ci, e, m)] of the stored hits of a record (numpy or ctypes)"""
    r = rec if isinstance(rec, np.void) or isinstance(rec, np.ndarray) else as_np(rec)[0]
    k = min(int(r["n_hits"]), HITS)
    return [tuple(h) for h in r["hits"][:k].tolist()]


# ---- the stimulus of the oracle cases ------------------------------------------------------------------------------------------

def psk_points(M, idx):
    """the points as the demodulator's soft stream shows them: QPSK on the diagonals, BPSK and 8-PSK from the real axis"""
    return np.exp(2j * math.pi * (np.asarray(idx) / M + (0.125 if M == 4 else 0.0)))


def framed_symbols(M, word_len, period, n_symbols, first, seed):
    """(symbol indices 0 .. M-1 of the stream, the word's indices, the word positions): a random word written every `period`
    symbols, from `first`, into random data"""
    rng = np.random.default_rng(seed)
    word = rng.integers(0, M, word_len)
    data = rng.integers(0, M, n_symbols)
    starts = list(range(first, n_symbols - word_len + 1, period))
    for s in starts:
        data[s: s + word_len] = word
    return data, word, starts


def framed_stream(M, S, word_len, period, n_symbols, first, sigma, seed):
    """interleaved float32 I/Q of the stream at S samples a symbol with a rectangular pulse and noise, the word as interleaved
    float32 points, the word's symbol positions"""
    data, word, starts = framed_symbols(M, word_len, period, n_symbols, first, seed)
    rng = np.random.default_rng(seed + 1)
    z = np.repeat(psk_points(M, data), S)
    z = z + sigma * (rng.standard_normal(len(z)) + 1j * rng.standard_normal(len(z)))
    iq = np.empty(2 * len(z), F32)
    iq[0::2], iq[1::2] = z.real, z.imag
    wz = psk_points(M, word)
    w = np.empty(2 * word_len, F32)
    w[0::2], w[1::2] = wz.real, wz.imag
    return iq, w, starts
