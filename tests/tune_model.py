"""The tuned packet of include/psk_soft_hip.h ("tuned packets") restated in numpy, for the tests of psk_soft_process_device_tuned
and psk_soft_tune_apply.

phase and step are integers mod 2^64 (turns x 2^64).  Sample k is converted to float32 exactly and multiplied by W(p_k),
p_k = phase + k * step: the product of a coarse table entry (the top ten bits of p_k) and a fine one (the next ten), every
operation float32 and rounded on its own.  The tables come from the C library's cosf / sinf through ctypes (the definition names
glibc 2.35's; tests/test_libm_pin.py pins the library's own copy against them)."""
import ctypes
import ctypes.util
import math

import numpy as np

F32 = np.float32
MASK = (1 << 64) - 1
N_TABLE = 1024
_tables = None


def tables():
    """(C, F): complex64-like pairs as float32 arrays of shape (1024, 2): (cos, sin) of h * pi / 512 and of l * pi / 2^19"""
    global _tables
    if _tables is None:
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for f in (libm.cosf, libm.sinf):
            f.argtypes, f.restype = [ctypes.c_float], ctypes.c_float
        out = []
        for scale in (math.pi / 512.0, math.pi / 524288.0):  # 0x1.921fb54442d18p-8, 0x1.921fb54442d18p-18
            t = np.empty((N_TABLE, 2), F32)
            for k in range(N_TABLE):
                a = float(F32(float(k) * scale))
                t[k] = (libm.cosf(a), libm.sinf(a))
            out.append(t)
        _tables = tuple(out)
    return _tables


def phase_words(phase, step, n):
    """p_k = phase + k * step mod 2^64, k = 0 .. n-1, as uint64"""
    with np.errstate(over="ignore"):
        return (np.uint64(int(phase) & MASK) + np.arange(n, dtype=np.uint64) * np.uint64(int(step) & MASK)).astype(np.uint64)


def phasors(phase, step, n):
    """W(p_k) as two float32 arrays (re, im)"""
    C, F = tables()
    p = phase_words(phase, step, n)
    h = (p >> np.uint64(54)).astype(np.int64)
    lo = ((p >> np.uint64(44)) & np.uint64(1023)).astype(np.int64)
    cr, ci, fr, fi = C[h, 0], C[h, 1], F[lo, 0], F[lo, 1]
    wr = ((cr * fr).astype(F32) - (ci * fi).astype(F32)).astype(F32)
    wi = ((cr * fi).astype(F32) + (ci * fr).astype(F32)).astype(F32)
    return wr, wi


def apply(phase, step, iq):
    """iq: interleaved I/Q of any packet dtype (float32, int16, int8, float16; an odd last element is dropped).  Returns the
    interleaved float32 I/Q of the tuned packet: what the CF32 packet of the contract holds."""
    x = np.asarray(iq)
    n = x.size // 2
    x = x[: 2 * n].astype(F32)  # (exact for every format)
    xr, xi = x[0::2], x[1::2]
    wr, wi = phasors(phase, step, n)
    with np.errstate(all="ignore"):
        y = np.empty(2 * n, F32)
        y[0::2] = ((xr * wr).astype(F32) - (xi * wi).astype(F32)).astype(F32)
        y[1::2] = ((xr * wi).astype(F32) + (xi * wr).astype(F32)).astype(F32)
    return y


def step_word(cycles_per_sample):
    """psk_soft_tune_step restated: r = f - floor(f), (r * 2^64) truncated, mod 2^64; 0 for a non-finite f"""
    f = float(cycles_per_sample)
    if not math.isfinite(f):
        return 0
    r = f - math.floor(f)
    return int(r * 2.0 ** 64) & MASK  # (r * 2^64 is exact: a power of two)


def advance(phase, step, n):
    return (int(phase) + int(step) * int(n)) & MASK


def lock_of(soft, M):
    """lock of psk_soft_quality_derive over the soft symbols of a run (tests/quality_model.py's terms)"""
    from tests import quality_model as qm

    t = qm.symbol_terms(soft, M)
    n = int(t["lock"].sum())
    return math.hypot(math.fsum(float(v) for v in t["c_re"][t["lock"]]), math.fsum(float(v) for v in t["c_im"][t["lock"]])) / n
