"""The arithmetic of psk_soft_symrate_t (include/psk_soft_hip.h, "symbol rate of a packet") restated in numpy, for the tests of
psk_soft_symrate_device, psk_soft_symrate_host and psk_soft_symrate_derive.

The model restates the DEVICE's order of additions (psk_soft_amd/csrc/psk_symrate.hip), so a device record is compared with it
byte for byte (record_bytes):

  a block     W = width(S) lanes share it; lane l adds the terms of the positions l, l + W, ... in that order from +0.0, then the
              lanes are added by the xor tree W/2, .., 1 (lane 0's result).  An invalid block is all zeros.
  a piece     512 blocks; lane t of 256 adds the terms of the blocks t, t + 256 of the piece from +0.0 (a term that does not
              enter is +0.0), each wave of 64 lanes by the xor tree 32, .., 1, then the four waves in order.
  the packet  lane l of 64 adds the partials l, l + 64, ... from +0.0, then the xor tree.

psk_soft_symrate_host adds in index order: assert_close compares it with the model within the documented bound -- n * 2^-53 *
sum|t| for n doubles added in any order, for the lag sums with the block sums' own error (S * 2^-53 * sum|term| per component)
carried through the product.  A term off by one float32 rounding (6e-8 relative) misses that bound by orders of magnitude.
Tuned samples and the phasor tables come from tests/tune_model.py."""
import math
import struct

import numpy as np

from tests import tune_model as tm

SR_DATA, SR_TUNED, SR_PLANNED = 1, 2, 128
LAGS = tuple(1 << j for j in range(8))
HALO, PIECE, MAX_BLOCKS, THREADS = 128, 512, 4096, 256
MIN_S, MAX_S = 4, 1024
F32, F64 = np.float32, np.float64
U = 2.0 ** -53
RECORD_BYTES = 392


def width(S):
    w = 1
    while 8 * w < S and w < 64:
        w <<= 1
    return w


def n_blocks_of(n, S):
    return min(n // S, MAX_BLOCKS)


def position_phasors(S):
    """(c_p, s_p), p = 0 .. S-1: W of the phase words (0 - p * floor(2^64 / S)) mod 2^64"""
    return tm.phasors(0, -((1 << 64) // S), S)


def _tree(a, w):
    """the xor tree over the last axis (w lanes): every lane's value, as the device's shuffles leave them"""
    idx = np.arange(w)
    off = w >> 1
    while off >= 1:
        a = a + a[..., idx ^ off]
        off >>= 1
    return a


def _lanes(terms, w):
    """terms: (..., n) float64, n a multiple of w; lane l adds terms l, l + w, ... in order from +0.0.  Returns (..., w)."""
    t = terms.reshape(terms.shape[:-1] + (-1, w))
    acc = np.zeros(t.shape[:-2] + (w,), F64)
    for i in range(t.shape[-2]):
        acc = acc + t[..., i, :]
    return acc


def block_sums(x, S, tree=None):
    """x: interleaved float32 I/Q (converted, tuned).  Returns dict(B (nb, 4) float64: B_e re, im, B_g re, im; lvl (nb, 2);
    valid (nb,) bool) in the device's order, invalid blocks zeroed; and absz (nb, 2): the sum of |z| per block, for the bounds.
    tree: another xor tree in place of _tree (tests/test_prepass_probe.py builds a wrong writer with one)."""
    n = x.size // 2
    nb = n_blocks_of(n, S)
    nu = nb * S
    re, im = x[0 : 2 * nu : 2].astype(F32), x[1 : 2 * nu : 2].astype(F32)
    with np.errstate(all="ignore"):
        e = ((re * re).astype(F32) + (im * im).astype(F32)).astype(F32)
        dr, di = np.zeros(nu, F32), np.zeros(nu, F32)
        dr[1:] = (re[1:] - re[:-1]).astype(F32)
        di[1:] = (im[1:] - im[:-1]).astype(F32)
        g = ((dr * dr).astype(F32) + (di * di).astype(F32)).astype(F32)
        g[0] = F32(0)
        fin = np.isfinite(re) & np.isfinite(im) & np.isfinite(e) & np.isfinite(g)
        fin[1:] &= np.isfinite(re[:-1]) & np.isfinite(im[:-1])
        valid = fin.reshape(nb, S).all(axis=1)
        c, s = position_phasors(S)
        c, s = np.tile(c, nb), np.tile(s, nb)
        w = width(S)
        pad = (-S) % w
        cols = []
        for z in (e, g):
            cols += [(z * c).astype(F32), (z * s).astype(F32)]
        cols += [e, g]
        out = np.empty((nb, 6), F64)
        for q, t in enumerate(cols):
            t = np.where(valid[:, None], t.astype(F64).reshape(nb, S), 0.0)  # (keeps NaN out of the arithmetic below)
            t = np.concatenate([t, np.zeros((nb, pad), F64)], axis=1)
            out[:, q] = (tree or _tree)(_lanes(t, w), w)[:, 0]
        absz = np.stack([np.where(valid[:, None], np.abs(z.astype(F64)).reshape(nb, S), 0.0).sum(axis=1) for z in (e, g)], axis=1)
    out[~valid] = 0.0
    return dict(B=out[:, :4].copy(), lvl=out[:, 4:].copy(), valid=valid, absz=absz)


def _piece_terms(b, lo, hi):
    """The 36 per-block terms (and 9 masks) of the blocks [lo, hi): terms (36, hi - lo) float64 with +0.0 where a term does not
    enter; counts (9,)."""
    B, lvl, valid = b["B"], b["lvl"], b["valid"]
    m = np.arange(lo, hi)
    va = valid[m]
    terms = np.zeros((36, hi - lo), F64)
    counts = np.zeros(9, np.int64)
    with np.errstate(all="ignore"):
        for z in range(2):
            ar, ai = B[m, 2 * z], B[m, 2 * z + 1]
            terms[32 + z] = np.where(va, ar * ar + ai * ai, 0.0)
            terms[34 + z] = np.where(va, lvl[m, z], 0.0)
            for j, L in enumerate(LAGS):
                k = m - L
                has = k >= 0
                kk = np.where(has, k, 0)
                ok = va & has & valid[kk]
                br, bi = B[kk, 2 * z], B[kk, 2 * z + 1]
                terms[16 * z + j] = np.where(ok, ar * br + ai * bi, 0.0)
                terms[16 * z + 8 + j] = np.where(ok, ai * br - ar * bi, 0.0)
                counts[j] = int(ok.sum())
    counts[8] = int(va.sum())
    return terms, counts


def piece_partial(b, lo, hi):
    """(36 doubles, 9 counts): what the fold leaves in the SymratePartial of the piece of the blocks [lo, hi)"""
    t, c = _piece_terms(b, lo, hi)
    turns = -(-(hi - lo) // THREADS)
    t = np.concatenate([t, np.zeros((36, turns * THREADS - (hi - lo)), F64)], axis=1)
    lanes = _lanes(t, THREADS)  # (36, 256)
    waves = _tree(lanes.reshape(36, THREADS // 64, 64), 64)[:, :, 0]
    p = waves[:, 0]
    for w in range(1, THREADS // 64):
        p = p + waves[:, w]
    return p, c


def _piece_partials(b):
    nb = b["valid"].size
    return [piece_partial(b, lo, min(lo + PIECE, nb)) for lo in range(0, nb, PIECE)]


def partial_bytes(p):
    """the 324 bytes of a SymratePartial in front of its pad"""
    d, c = p
    return np.asarray(d, "<f8").tobytes() + np.asarray(c, "<u4").tobytes()


def join_bytes(parts, n, S, tuned):
    """the record the join makes of a packet's partials: 392 bytes"""
    s, c = _join(parts)
    nb = n_blocks_of(n, S)
    return struct.pack("<4Q8Q36dHB5x", n, nb * S, nb, int(c[8]), *[int(v) for v in c[:8]], *[float(v) for v in np.concatenate(
        [s[0:8], s[16:24], s[8:16], s[24:32], s[32:36]])], S, SR_DATA | (SR_TUNED if tuned else 0))


def _join(parts):
    """the packet's 36 sums and 9 counts: the join of its pieces' partials in the device's order"""
    n_piece = len(parts)
    t = np.stack([p for p, _ in parts], axis=1)  # (36, n_piece)
    t = np.concatenate([t, np.zeros((36, (-n_piece) % 64), F64)], axis=1)
    return _tree(_lanes(t, 64), 64)[:, 0], sum(c for _, c in parts)


def _fold(b):
    """the packet's 36 sums and 9 counts in the device's order"""
    return _join(_piece_partials(b))


def _converted(iq, S, tune):
    """(the float32 samples the look uses -- converted, tuned --, tuned?)"""
    tuned = tune is not None and (int(tune[0]) | int(tune[1])) != 0
    x = np.asarray(iq)[: 2 * n_blocks_of(np.asarray(iq).size // 2, S) * S]
    return (tm.apply(tune[0], tune[1], x) if tuned else x.astype(F32)), tuned


def partials(iq, S, tune=None):
    """[(d: 36 float64, c: 9 int64)] per piece of the packet, as the fold kernel leaves them in its SymratePartial (the record
    is their join: model_record); [] for a packet the look does not take"""
    n = 0 if iq is None else np.asarray(iq).size // 2
    if not (MIN_S <= S <= MAX_S) or n < 2 * S:
        return []
    return _piece_partials(block_sums(_converted(iq, S, tune)[0], S))


def zero_record():
    return dict(n_samples=0, n_used=0, n_blocks=0, n_valid=0, n_pairs=[0] * 8, sum_re=[[0.0] * 8, [0.0] * 8], sum_im=[[0.0] * 8, [0.0] * 8],
                sum_pow=[0.0, 0.0], sum_lvl=[0.0, 0.0], samplesPerBaud=0, flags=0)


def model_record(iq, S, tune=None):
    """What the device's record of a packet must be, to the byte.  iq: the packet's samples, interleaved, of any packet dtype
    (None: no packet); S: the channel's samplesPerBaud; tune: None or (phase, step).  Returns a dict of the record's fields (and
    `blocks`: block_sums' result, for the bounds of assert_close)."""
    n = 0 if iq is None else np.asarray(iq).size // 2
    if not (MIN_S <= S <= MAX_S) or n < 2 * S:
        return zero_record()  # (the zero record of a covered channel without a look)
    nb = n_blocks_of(n, S)
    x, tuned = _converted(iq, S, tune)
    b = block_sums(x, S)
    parts = _piece_partials(b)
    s, c = _join(parts)
    r = zero_record()
    r.update(n_samples=n, n_used=nb * S, n_blocks=nb, n_valid=int(c[8]), n_pairs=[int(v) for v in c[:8]], samplesPerBaud=S,
             flags=SR_DATA | (SR_TUNED if tuned else 0), blocks=b, parts=parts)
    for z in range(2):
        r["sum_re"][z] = [float(v) for v in s[16 * z : 16 * z + 8]]
        r["sum_im"][z] = [float(v) for v in s[16 * z + 8 : 16 * z + 16]]
        r["sum_pow"][z] = float(s[32 + z])
        r["sum_lvl"][z] = float(s[34 + z])
    return r


def record_bytes(m):
    """the 392 bytes of psk_soft_symrate_t with the fields of m (a model_record, or anything else with its keys)"""
    flat = list(m["sum_re"][0]) + list(m["sum_re"][1]) + list(m["sum_im"][0]) + list(m["sum_im"][1]) + list(m["sum_pow"]) + list(m["sum_lvl"])
    return struct.pack("<4Q8Q36dHB5x", m["n_samples"], m["n_used"], m["n_blocks"], m["n_valid"], *m["n_pairs"], *flat, m["samplesPerBaud"], m["flags"])


def as_dict(r):
    """a lib.Symrate (or anything with its fields) as a dict of model_record's keys"""
    return dict(n_samples=int(r.n_samples), n_used=int(r.n_used), n_blocks=int(r.n_blocks), n_valid=int(r.n_valid), n_pairs=[int(v) for v in r.n_pairs],
                sum_re=[[float(v) for v in r.sum_re[z]] for z in range(2)], sum_im=[[float(v) for v in r.sum_im[z]] for z in range(2)],
                sum_pow=[float(v) for v in r.sum_pow], sum_lvl=[float(v) for v in r.sum_lvl], samplesPerBaud=int(r.samplesPerBaud), flags=int(r.flags))


def assert_bytes(r, model, ctx=""):
    """r: a lib.Symrate from the device; the model's bytes, nothing less"""
    got, want = bytes(r), record_bytes(model)
    assert len(got) == RECORD_BYTES == len(want), ctx
    if got != want:
        g = as_dict(r)
        diff = [k for k in g if g[k] != model[k] and not (isinstance(g[k], float) and math.isnan(g[k]))]
        raise AssertionError("%s: the record differs from the model in %s\n got  %r\n want %r" % (ctx, diff, {k: g[k] for k in diff}, {k: model[k] for k in diff}))


def bounds(model):
    """per sum of the record: how far a record that adds the same terms in another order may lie from the model's"""
    b = model["blocks"]
    B, valid, S = b["B"], b["valid"], model["samplesPerBaud"]
    nb = valid.size
    # a component of a block sum: S doubles in any order, |term| <= 1.000001 |z|
    dB = 1.000001 * S * U * b["absz"]  # (nb, 2)
    out = dict(sum_re=[[0.0] * 8, [0.0] * 8], sum_im=[[0.0] * 8, [0.0] * 8], sum_pow=[0.0, 0.0], sum_lvl=[0.0, 0.0])
    for z in range(2):
        mod = np.hypot(B[:, 2 * z], B[:, 2 * z + 1])
        d = math.sqrt(2.0) * dB[:, z]
        out["sum_lvl"][z] = model["n_used"] * U * float(b["absz"][:, z].sum()) + 1e-300
        out["sum_pow"][z] = float((2.0 * mod * d + d * d + 4.0 * U * mod * mod).sum() + nb * U * (mod * mod).sum()) + 1e-300
        for j, L in enumerate(LAGS):
            if nb <= L:
                continue
            ok = valid[L:] & valid[:-L]
            a, c, da, dc = mod[L:][ok], mod[:-L][ok], d[L:][ok], d[:-L][ok]
            t = float((a * dc + c * da + da * dc + 4.0 * U * a * c).sum() + ok.sum() * U * (a * c).sum()) + 1e-300
            out["sum_re"][z][j] = out["sum_im"][z][j] = t
    return out


def assert_close(r, model, ctx=""):
    """r: a lib.Symrate that adds in another order (psk_soft_symrate_host): integers, flags and pad equal, sums within bounds()"""
    g = as_dict(r)
    for k in ("n_samples", "n_used", "n_blocks", "n_valid", "n_pairs", "samplesPerBaud", "flags"):
        assert g[k] == model[k], "%s: %s is %r, the model says %r" % (ctx, k, g[k], model[k])
    assert bytes(r.pad) == bytes(5), ctx
    if "blocks" not in model:
        assert bytes(r) == record_bytes(model), ctx
        return
    bd = bounds(model)
    for k in ("sum_pow", "sum_lvl"):
        for z in range(2):
            assert abs(g[k][z] - model[k][z]) <= bd[k][z], "%s: %s[%d] = %r, the model says %r, bound %.3g" % (ctx, k, z, g[k][z], model[k][z], bd[k][z])
    for k in ("sum_re", "sum_im"):
        for z in range(2):
            for j in range(8):
                assert abs(g[k][z][j] - model[k][z][j]) <= bd[k][z][j], "%s: %s[%d][%d] = %r, the model says %r, bound %.3g" % (
                    ctx, k, z, j, g[k][z][j], model[k][z][j], bd[k][z][j])


def derive(r):
    """psk_soft_symrate_derive in Python, on anything with the record's fields"""
    nan = float("nan")
    d = dict(samples_per_symbol=nan, step_ratio=nan, coherence=nan, mean_level=nan, detector=-1, lags_used=0)
    if not (r.flags & SR_DATA) or not r.n_pairs[0] or not r.n_valid:
        return d

    def coh(z, j):
        return math.hypot(r.sum_re[z][j], r.sum_im[z][j]) / (r.n_pairs[j] * (r.sum_pow[z] / r.n_valid))

    c0 = [0.0 if r.sum_re[z][0] == 0.0 and r.sum_im[z][0] == 0.0 else coh(z, 0) for z in range(2)]
    if c0[0] == 0.0 and c0[1] == 0.0:
        return d
    z = 1 if c0[1] > c0[0] else 0
    two_pi = 2.0 * math.pi
    f = math.atan2(r.sum_im[z][0], r.sum_re[z][0]) / two_pi
    used = 1
    for j in range(1, 8):
        if r.n_pairs[j] < 8 or coh(z, j) < 0.5 * c0[z]:
            break
        L = float(1 << j)
        dd = math.atan2(r.sum_im[z][j], r.sum_re[z][j]) - two_pi * L * f
        dd -= two_pi * float(np.rint(dd / two_pi))
        f += dd / (two_pi * L)
        used += 1
    S = float(r.samplesPerBaud)
    d.update(samples_per_symbol=S / (1.0 + f), step_ratio=1.0 / (1.0 + f), coherence=c0[z], mean_level=r.sum_lvl[z] / (r.n_valid * S), detector=z, lags_used=used)
    return d


def assert_derived(got, want, ctx=""):
    """got: lib.symrate_derive(rec); want: derive(rec) -- the integers equal, the doubles within 1e-12 relative, the NaN patterns equal"""
    for k in ("detector", "lags_used"):
        assert got[k] == want[k], "%s: %s %r, the model says %r" % (ctx, k, got[k], want[k])
    for k in ("samples_per_symbol", "step_ratio", "coherence", "mean_level"):
        a, b = got[k], want[k]
        assert math.isnan(a) == math.isnan(b), "%s: %s = %r, the model says %r" % (ctx, k, a, b)
        assert math.isnan(a) or abs(a - b) <= 1e-12 * max(1.0, abs(b)), "%s: %s = %r, the model says %r" % (ctx, k, a, b)
