"""The arithmetic of psk_soft_quality_t (include/psk_soft_hip.h) restated in numpy, for the tests of PSK_SOFT_OPT_QUALITY.

Per-symbol terms in float32, every product and sum rounded on its own; the sums with math.fsum (exact).  A record is compared
with the model like this: the four counts, the copied first / last values (as bit patterns), the snapshot fields and the flags
EQUAL; each of the four sums within n * 2^-53 * sum|t_i| of the exact sum of its n terms t_i -- the textbook bound for n doubles
added in any order.  A per-symbol term that was off by one float rounding (6e-8 relative) would miss that bound (about 1e-12
relative at 10^4 symbols) by orders of magnitude."""

import math

import numpy as np

Q_SOFT, Q_PHASE, Q_INDEX, Q_LOCK, Q_PLANNED = 1, 2, 4, 8, 128
F32 = np.float32
FLT_MIN = np.finfo(np.float32).tiny


def _mul(a, b):
    return (a * b).astype(F32)


def symbol_terms(soft, M):
    """soft: interleaved re, im (float32).  Returns dict(e, q, finite, c_re, c_im, lock): float32 arrays and boolean masks, one
    entry per symbol (c_* are meaningless where lock is False)."""
    soft = np.ascontiguousarray(soft, F32)
    re, im = soft[0::2].copy(), soft[1::2].copy()
    with np.errstate(all="ignore"):
        e = (_mul(re, re) + _mul(im, im)).astype(F32)
        q = _mul(e, e)
        finite = np.isfinite(re) & np.isfinite(im) & np.isfinite(q)
        lock = np.zeros(re.size, bool)
        c_re = np.zeros(re.size, F32)
        c_im = np.zeros(re.size, F32)
        if M in (2, 4, 8):
            pr, pi = re, im
            for _ in range({2: 1, 4: 2, 8: 3}[M]):
                r2 = (_mul(pr, pr) - _mul(pi, pi)).astype(F32)
                i2 = (_mul(pr, pi) + _mul(pi, pr)).astype(F32)
                pr, pi = r2, i2
            a = e if M == 2 else q if M == 4 else _mul(q, q)
            lock = finite & np.isfinite(pr) & np.isfinite(pi) & np.isfinite(a) & (a >= FLT_MIN)
            safe = np.where(lock, a, F32(1))
            c_re = (pr / safe).astype(F32)
            c_im = (pi / safe).astype(F32)
    return dict(e=e, q=q, finite=finite, c_re=c_re, c_im=c_im, lock=lock)


def _sum_and_bound(t):
    t = [float(v) for v in t]
    return math.fsum(t), len(t) * 2.0 ** -53 * math.fsum(abs(v) for v in t)


def model_record(soft, phase, index, M, S, diff):
    """What the record of a call must be.  soft / phase / index: the rows the call wrote (numpy arrays), or None where the call
    had no pointer for the stream; the number of symbols is taken from whichever is given (soft has two floats a symbol).
    Returns dict: the integer and copied fields by name, `sums` = {name: (exact, bound)}."""
    n = soft.size // 2 if soft is not None else phase.size if phase is not None else index.size
    rec = dict(n_symbols=n, n_finite=0, n_lock=0, index_changes=0, phase_first=F32(0), phase_last=F32(0), index_first=0, index_last=0,
               constelationSize=0, samplesPerBaud=0, differentialDecoding=0, flags=0)
    sums = dict(sum_e=(0.0, 0.0), sum_e2=(0.0, 0.0), sum_lock_re=(0.0, 0.0), sum_lock_im=(0.0, 0.0))
    if n == 0:
        rec["sums"] = sums
        return rec  # (the zero record of a covered channel that emitted nothing)
    rec.update(constelationSize=M, samplesPerBaud=S, differentialDecoding=int(bool(diff)))
    flags = 0
    if soft is not None:
        flags |= Q_SOFT
        t = symbol_terms(soft, M)
        rec["n_finite"] = int(t["finite"].sum())
        sums["sum_e"] = _sum_and_bound(t["e"][t["finite"]])
        sums["sum_e2"] = _sum_and_bound(t["q"][t["finite"]])
        if M in (2, 4, 8):
            flags |= Q_LOCK
            rec["n_lock"] = int(t["lock"].sum())
            sums["sum_lock_re"] = _sum_and_bound(t["c_re"][t["lock"]])
            sums["sum_lock_im"] = _sum_and_bound(t["c_im"][t["lock"]])
    if phase is not None:
        flags |= Q_PHASE
        rec["phase_first"], rec["phase_last"] = F32(phase[0]), F32(phase[n - 1])
    if index is not None and index.size:
        flags |= Q_INDEX
        rec["index_first"], rec["index_last"] = int(index[0]), int(index[-1])
        rec["index_changes"] = int(np.count_nonzero(index[1:] != index[:-1]))
    rec["flags"] = flags
    rec["sums"] = sums
    return rec


INT_FIELDS = ("n_symbols", "n_finite", "n_lock", "index_changes", "index_first", "index_last", "constelationSize", "samplesPerBaud",
              "differentialDecoding", "flags")


def assert_record(q, model, ctx=""):
    """q: a lib.Quality (or anything with its fields); model: model_record(...)"""
    for k in INT_FIELDS:
        assert int(getattr(q, k)) == int(model[k]), "%s: %s is %r, the model says %r" % (ctx, k, getattr(q, k), model[k])
    for k in ("phase_first", "phase_last"):
        a, b = np.array([getattr(q, k)], F32).view(np.uint32)[0], np.array([model[k]], F32).view(np.uint32)[0]
        assert a == b, "%s: %s has bits %08x, the model %08x" % (ctx, k, a, b)
    assert bytes(q.pad) == bytes(6), ctx
    for k, (exact, bound) in model["sums"].items():
        got = float(getattr(q, k))
        assert abs(got - exact) <= bound, "%s: %s = %r, exact sum %r, off by %.3g > bound %.3g" % (ctx, k, got, exact, abs(got - exact), bound)


def derive(q):
    """psk_soft_quality_derive in Python, on anything with the record's fields: dict(lock, snr_db, mean_energy, index_change_rate)"""
    nan = float("nan")
    d = dict(lock=nan, snr_db=nan, mean_energy=nan, index_change_rate=nan)
    if (q.flags & Q_LOCK) and q.n_lock:
        d["lock"] = math.hypot(q.sum_lock_re, q.sum_lock_im) / q.n_lock
    if q.n_finite:
        m2, m4 = q.sum_e / q.n_finite, q.sum_e2 / q.n_finite
        d["mean_energy"] = m2
        dd = 2.0 * m2 * m2 - m4
        if dd > 0 and not q.differentialDecoding:
            s = math.sqrt(dd)
            if m2 - s > 0:
                d["snr_db"] = 10.0 * math.log10(s / (m2 - s))
    if (q.flags & Q_INDEX) and q.n_symbols >= 2:
        d["index_change_rate"] = q.index_changes / (q.n_symbols - 1)
    return d
