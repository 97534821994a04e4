"""The arithmetic of psk_soft_acquire_t (include/psk_soft_hip.h, "carrier offset of a packet") restated in numpy, for the tests of
psk_soft_acquire_device, psk_soft_acquire_host and psk_soft_acquire_derive.

Per-sample and per-lag terms in float32, every product, sum and quotient rounded on its own; the sums with math.fsum (exact).  A
record is compared with the model like this: the counts, constelationSize and the flags EQUAL, the pad zero; each sum within
n * 2^-53 * sum|t_i| of the exact sum of its n float32 terms t_i -- the textbook bound for n doubles added in any order.  A term
that was off by one float rounding (6e-8 relative) would miss that bound by orders of magnitude.  Tuned samples come from
tests/tune_model.py."""
import math
import struct

import numpy as np

from tests import tune_model as tm

A_DATA, A_TUNED, A_PLANNED = 1, 2, 128
LAGS = tuple(1 << j for j in range(8))
F32 = np.float32
FLT_MIN = np.finfo(np.float32).tiny


def _mul(a, b):
    return (a * b).astype(F32)


def sample_terms(iq, M):
    """iq: interleaved re, im (float32), M in (2, 4, 8).  Returns dict(e, valid, ur, ui): float32 arrays and a boolean mask, one
    entry per sample (ur, ui are meaningless where valid is False)."""
    iq = np.ascontiguousarray(iq, F32)
    n = iq.size // 2
    re, im = iq[0 : 2 * n : 2].copy(), iq[1 : 2 * n : 2].copy()
    with np.errstate(all="ignore"):
        e = (_mul(re, re) + _mul(im, im)).astype(F32)
        q = _mul(e, e)
        pr, pi = re, im
        for _ in range({2: 1, 4: 2, 8: 3}[M]):
            r2 = (_mul(pr, pr) - _mul(pi, pi)).astype(F32)
            i2 = (_mul(pr, pi) + _mul(pi, pr)).astype(F32)
            pr, pi = r2, i2
        a = e if M == 2 else q if M == 4 else _mul(q, q)
        valid = np.isfinite(re) & np.isfinite(im) & np.isfinite(q) & np.isfinite(pr) & np.isfinite(pi) & np.isfinite(a) & (a >= FLT_MIN)
        safe = np.where(valid, a, F32(1))
        ur = (np.where(valid, pr, F32(0)) / safe).astype(F32)
        ui = (np.where(valid, pi, F32(0)) / safe).astype(F32)
    return dict(e=e, valid=valid, ur=ur, ui=ui)


def lag_terms(t, L):
    """(t_re, t_im): float32 arrays, one entry per k >= L with samples k and k - L both valid"""
    ur, ui, valid = t["ur"], t["ui"], t["valid"]
    if ur.size <= L:
        return np.zeros(0, F32), np.zeros(0, F32)
    ok = valid[L:] & valid[:-L]
    a_r, a_i, b_r, b_i = ur[L:][ok], ui[L:][ok], ur[:-L][ok], ui[:-L][ok]
    t_re = (_mul(a_r, b_r) + _mul(a_i, b_i)).astype(F32)
    t_im = (_mul(a_i, b_r) - _mul(a_r, b_i)).astype(F32)
    return t_re, t_im


def _sum_and_bound(t):
    t = [float(v) for v in t]
    return math.fsum(t), len(t) * 2.0 ** -53 * math.fsum(abs(v) for v in t)


def model_record(iq, M, tune=None):
    """What the record of a packet must be.  iq: the packet's samples, interleaved, of any packet dtype (None: no packet); M: the
    channel's constelationSize; tune: None or (phase, step).  Returns dict: the integer fields by name (n_pairs a list),
    `sums` = {"sum_e": (exact, bound), "sum_re": [(exact, bound)] * 8, "sum_im": likewise}."""
    zero = dict(n_samples=0, n_valid=0, n_pairs=[0] * 8, constelationSize=0, flags=0,
                sums=dict(sum_e=(0.0, 0.0), sum_re=[(0.0, 0.0)] * 8, sum_im=[(0.0, 0.0)] * 8))
    n = 0 if iq is None else np.asarray(iq).size // 2
    if n == 0 or M not in (2, 4, 8):
        return zero  # (the zero record of a covered channel without a look)
    tuned = tune is not None and (int(tune[0]) | int(tune[1])) != 0
    x = tm.apply(tune[0], tune[1], iq) if tuned else np.asarray(iq)[: 2 * n].astype(F32)
    t = sample_terms(x, M)
    rec = dict(n_samples=n, n_valid=int(t["valid"].sum()), n_pairs=[], constelationSize=M, flags=A_DATA | (A_TUNED if tuned else 0))
    sums = dict(sum_e=_sum_and_bound(t["e"][t["valid"]]), sum_re=[], sum_im=[])
    for L in LAGS:
        t_re, t_im = lag_terms(t, L)
        rec["n_pairs"].append(int(t_re.size))
        sums["sum_re"].append(_sum_and_bound(t_re))
        sums["sum_im"].append(_sum_and_bound(t_im))
    rec["sums"] = sums
    return rec


# ---- the device's order of additions (psk_soft_amd/csrc/psk_acquire.hip), restated: bytes, not bounds -----------------------------
#
#   a piece     4096 samples.  Lag sums (stage 2): lane t of 256 adds the float32 products of the samples t, t + 256, ... of the
#               piece as doubles from +0.0 (a pair that does not enter adds a zero); each wave of 64 lanes by the xor tree
#               32, .., 1; then the four waves in order.  Energy (stage 1): lane t takes the sample pairs start + 2t, + 512, ...
#               (start: 128 samples in front of the piece, or 0 in the first piece), adds e of the first then of the second
#               sample, only of valid samples of the piece itself; the same tree, the same order of waves.
#   the packet  lane l of 64 adds the partials l, l + 64, ... from +0.0, then the xor tree.
#
# The per-sample and per-lag float32 terms are sample_terms' and lag_terms' arithmetic; model_record above stays the judge of this
# restatement (tests/test_prepass_probe.py holds device_record to it under assert_record on every packet the probe uses).

PIECE, HALO, THREADS = 4096, 128, 256
RECORD_BYTES, PARTIAL_SUMS, PARTIAL_COUNTS = 224, 17, 9
F64 = np.float64


def _tree64(a):
    """the xor tree 32, .., 1 over the last axis (64 lanes): lane 0's value"""
    idx = np.arange(64)
    off = 32
    while off >= 1:
        a = a + a[..., idx ^ off]
        off >>= 1
    return a[..., 0]


def _in_turn(t):
    """t: (..., turns, lanes): every lane adds its terms in turn order from +0.0"""
    acc = np.zeros(t.shape[:-2] + t.shape[-1:], F64)
    for i in range(t.shape[-2]):
        acc = acc + t[..., i, :]
    return acc


def _waves(lanes):
    """lanes: (..., 256): each wave by the tree, the four waves in order"""
    w = _tree64(lanes.reshape(lanes.shape[:-1] + (THREADS // 64, 64)))
    p = w[..., 0]
    for k in range(1, THREADS // 64):
        p = p + w[..., k]
    return p


def _converted(iq, tune):
    n = np.asarray(iq).size // 2
    tuned = tune is not None and (int(tune[0]) | int(tune[1])) != 0
    return (tm.apply(tune[0], tune[1], iq) if tuned else np.asarray(iq)[: 2 * n].astype(F32)), tuned


def device_partials(iq, M, tune=None):
    """[(d: 17 float64 -- sum_re[8], sum_im[8], sum_e --, c: 9 int64 -- n_pairs[8], n_valid)] per piece of the packet, as the fold
    kernel leaves them in its AcquirePartial; [] for no packet"""
    n = 0 if iq is None else np.asarray(iq).size // 2
    if n == 0 or M not in (2, 4, 8):
        return []
    t = sample_terms(_converted(iq, tune)[0], M)
    ur, ui, valid = t["ur"], t["ui"], t["valid"]
    with np.errstate(all="ignore"):
        e = np.where(valid, t["e"], F32(0)).astype(F64)
    lag = np.zeros((16, n), F64)
    hit = np.zeros((8, n), bool)
    for j, L in enumerate(LAGS):
        if n <= L:
            continue
        ok = valid[L:] & valid[:-L]
        t_re = (_mul(ur[L:], ur[:-L]) + _mul(ui[L:], ui[:-L])).astype(F32)
        t_im = (_mul(ui[L:], ur[:-L]) - _mul(ur[L:], ui[:-L])).astype(F32)
        lag[j, L:] = np.where(ok, t_re, F32(0))
        lag[8 + j, L:] = np.where(ok, t_im, F32(0))
        # (the device counts the products that are not (0, 0); an invalid sample's phasor is (0, 0))
        hit[j, L:] = ok & ((t_re != 0) | (t_im != 0))
    out = []
    for lo in range(0, n, PIECE):
        hi = min(lo + PIECE, n)
        turns = -(-(hi - lo) // THREADS)
        end = lo + turns * THREADS
        seg = np.zeros((16, end - lo), F64)
        seg[:, : hi - lo] = lag[:, lo:hi]
        d = np.empty(PARTIAL_SUMS, F64)
        d[:16] = _waves(_in_turn(seg.reshape(16, turns, THREADS)))
        start = lo - HALO if lo else 0
        trips = -(-(end - start) // (2 * THREADS))
        es = np.zeros(trips * 2 * THREADS, F64)
        es[lo - start : hi - start] = e[lo:hi]
        es = es.reshape(trips, THREADS, 2)  # (trip, lane, first / second sample of the lane's pair)
        d[16] = _waves(_in_turn(es.transpose(0, 2, 1).reshape(2 * trips, THREADS)))
        c = np.array([int(hit[j, lo:hi].sum()) for j in range(8)] + [int(valid[lo:hi].sum())], np.int64)
        out.append((d, c))
    return out


def partial_bytes(p):
    """the 172 bytes of an AcquirePartial in front of its pad"""
    d, c = p
    return np.asarray(d, "<f8").tobytes() + np.asarray(c, "<u4").tobytes()


def join_bytes(parts, n, M, tuned):
    """the record the join makes of a packet's partials: 224 bytes"""
    k = len(parts)
    t = np.zeros((PARTIAL_SUMS, -(-k // 64) * 64), F64)
    t[:, :k] = np.stack([d for d, _ in parts], axis=1)
    s = _tree64(_in_turn(t.reshape(PARTIAL_SUMS, -1, 64)))
    c = sum(c for _, c in parts)
    return struct.pack("<2Q8Q17dHB5x", n, int(c[8]), *[int(v) for v in c[:8]], *[float(v) for v in s], M, A_DATA | (A_TUNED if tuned else 0))


def device_record(iq, M, tune=None):
    """the 224 bytes of the device's record of a packet; the zero record for no packet"""
    parts = device_partials(iq, M, tune)
    if not parts:
        return bytes(RECORD_BYTES)
    return join_bytes(parts, np.asarray(iq).size // 2, M, tune is not None and (int(tune[0]) | int(tune[1])) != 0)


def assert_record(r, model, ctx=""):
    """r: a lib.Acquire (or anything with its fields); model: model_record(...)"""
    for k in ("n_samples", "n_valid", "constelationSize", "flags"):
        assert int(getattr(r, k)) == int(model[k]), "%s: %s is %r, the model says %r" % (ctx, k, getattr(r, k), model[k])
    assert list(r.n_pairs) == model["n_pairs"], "%s: n_pairs %r, the model says %r" % (ctx, list(r.n_pairs), model["n_pairs"])
    assert bytes(r.pad) == bytes(5), ctx
    checks = [("sum_e", float(r.sum_e)) + model["sums"]["sum_e"]]
    for j in range(8):
        checks.append(("sum_re[%d]" % j, float(r.sum_re[j])) + model["sums"]["sum_re"][j])
        checks.append(("sum_im[%d]" % j, float(r.sum_im[j])) + model["sums"]["sum_im"][j])
    for name, got, exact, bound in checks:
        assert abs(got - exact) <= bound, "%s: %s = %r, exact sum %r, off by %.3g > bound %.3g" % (ctx, name, got, exact, abs(got - exact), bound)


def derive(r):
    """psk_soft_acquire_derive in Python, on anything with the record's fields: dict(offset_cycles_per_sample, coherence,
    mean_energy, lags_used)"""
    nan = float("nan")
    d = dict(offset_cycles_per_sample=nan, coherence=nan, mean_energy=nan, lags_used=0)
    if not (r.flags & A_DATA) or not r.n_pairs[0] or (r.sum_re[0] == 0.0 and r.sum_im[0] == 0.0):
        return d
    M, two_pi = float(r.constelationSize), 2.0 * math.pi
    c0 = math.hypot(r.sum_re[0], r.sum_im[0]) / r.n_pairs[0]
    f = math.atan2(r.sum_im[0], r.sum_re[0]) / (two_pi * M)
    used = 1
    for j in range(1, 8):
        if not r.n_pairs[j] or math.hypot(r.sum_re[j], r.sum_im[j]) / r.n_pairs[j] < 0.5 * c0:
            break
        L = float(1 << j)
        dd = math.atan2(r.sum_im[j], r.sum_re[j]) - two_pi * M * L * f
        dd -= two_pi * float(np.rint(dd / two_pi))
        f += dd / (two_pi * M * L)
        used += 1
    d.update(offset_cycles_per_sample=f, coherence=c0, mean_energy=r.sum_e / r.n_valid if r.n_valid else nan, lags_used=used)
    return d


def assert_derived(got, want, ctx=""):
    """got: lib.acquire_derive(rec); want: derive(rec) -- lags_used equal, the doubles within 1e-12, the NaN patterns equal"""
    assert got["lags_used"] == want["lags_used"], "%s: lags_used %r, the model says %r" % (ctx, got["lags_used"], want["lags_used"])
    for k in ("offset_cycles_per_sample", "coherence", "mean_energy"):
        a, b = got[k], want[k]
        assert math.isnan(a) == math.isnan(b), "%s: %s = %r, the model says %r" % (ctx, k, a, b)
        if k == "offset_cycles_per_sample":
            assert math.isnan(a) or abs(a - b) <= 1e-12, "%s: %s = %r, the model says %r" % (ctx, k, a, b)
        else:
            assert math.isnan(a) or abs(a - b) <= 1e-12 * max(1.0, abs(b)), "%s: %s = %r, the model says %r" % (ctx, k, a, b)
