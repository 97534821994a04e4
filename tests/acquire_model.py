"""The arithmetic of psk_soft_acquire_t (include/psk_soft_hip.h, "carrier offset of a packet") restated in numpy, for the tests of
psk_soft_acquire_device, psk_soft_acquire_host and psk_soft_acquire_derive.

Per-sample and per-lag terms in float32, every product, sum and quotient rounded on its own; the sums with math.fsum (exact).  A
record is compared with the model like this: the counts, constelationSize and the flags EQUAL, the pad zero; each sum within
n * 2^-53 * sum|t_i| of the exact sum of its n float32 terms t_i -- the textbook bound for n doubles added in any order.  A term
that was off by one float rounding (6e-8 relative) would miss that bound by orders of magnitude.  Tuned samples come from
tests/tune_model.py."""
import math

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
