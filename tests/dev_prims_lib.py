"""ctypes binding of the test-only device library (tests/support/dev_prims.hip -> psk_soft_amd/libpsk_dev_prims.so): every
device-math and wave primitive of the product headers behind an elementwise kernel of its own.  One C entry,
psk_dev_prims_run(op, in, out, n); run() below checks the arrays against the table and raises on a HIP error."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "psk_soft_amd", "libpsk_dev_prims.so")

f32, f64, i32, u32, i64 = np.float32, np.float64, np.int32, np.uint32, np.int64
DIVERGENT = 1 << 30
_T = {0: i32, 1: f32, 2: f64}  # the element type of wave_up1 / wave_up1_zero / read_lane by parameter

# name: (id, input dtypes, output dtypes, has a lane-divergent form); a callable takes the parameter
OPS = {
    "atan2": (1, (f32, f32), (f32,), lambda p: p == 1),
    "sincos": (2, (f32,), (f32, f32), True),
    "slice8_fast": (3, (f32, f32), (u32, u32), True),
    "slice8": (4, (f32, f32), (u32,), lambda p: p == 1),
    "slice8_atan": (5, (f32, f32), (u32,), lambda p: p == 1),
    "div_known": (6, (f64, f64, f64), (f64,), True),
    "norm": (7, (f32, f32), (f32,), True),
    "cmul": (8, (f32,) * 4, (f32, f32), True),
    "cpow": (9, (f32, f32), (f32, f32), True),
    "cdiv": (10, (f32,) * 4, (f32, f32), True),
    "to_long": (11, (f64,), (i64,), True),
    "unwrap": (12, (f32, f64), (i64,), True),
    "fit_den": (13, (f32, u32), (f32, f32), True),
    "fit_value": (14, (f64, f64, f32, u32), (f32, f32, f32), True),
    "fit_known": (15, (f64, f64, f32, u32), (f32, f32), False),
    "qpsk": (16, (f32, f32), (i32, i32), True),
    "wrap_test": (17, (f32, f32), (u32,), True),
    "scan_f64": (18, (f64,), (f64,), False),
    "sum_f64": (19, (f64,), (f64,), False),
    "scan_i32": (20, (i32,), (i32,), False),
    "scan_f32_multi": (21, (f32,), (f32,), False),  # parameter N: arrays of n * N elements, case-major
    "max_f32": (22, (f32,), (f32,), False),
    "max_u32": (23, (u32,), (u32,), False),
    "min_u32": (24, (u32,), (u32,), False),
    "up1": (25, lambda p: (_T[p], _T[p]), lambda p: (_T[p],), False),
    "up1_zero": (26, lambda p: (_T[p],), lambda p: (_T[p],), False),
    "read_lane": (27, lambda p: (_T[p], i32), lambda p: (_T[p],), False),
    "med3": (28, (i32, i32, i32), (i32,), True),
    # psk_tile_any.h: the front stages call these with the whole wave, none has a lane-divergent form
    "any_merge": (29, (f64, f64, f64, f64, i32, i32), (f64, f64, i32), False),  # a.best, a.second, b.best, b.second, a.k, b.k
    "any_max_f64": (30, (f64,), (f64,), False),
    "any_min_u32": (31, (u32,), (u32,), False),
    "any_max_f64_multi": (32, (f64,), (f64,), False),  # parameter U = 8: arrays of n * U elements, case-major
    "any_min_u32_multi": (33, (u32,), (u32,), False),
}
MULTI = ("scan_f32_multi", "any_max_f64_multi", "any_min_u32_multi")  # the parameter is the number of elements per case
TAB_DEV, TAB_WAVE = 0, 1  # the parameter of atan2 / slice8 / slice8_atan


def cpow_param(M, recover):
    return M | (int(bool(recover)) << 8)


_lib = None
_failed = None  # the first HIP error of this process: nothing more is launched after one


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is not built (make -C psk_soft_amd/csrc)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.psk_dev_prims_run.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_longlong]
        L.psk_dev_prims_run.restype = ctypes.c_int
        _lib = L
    return _lib


def signature(name, param=0):
    oid, ins, outs, div = OPS[name]
    ins = ins(param) if callable(ins) else ins
    outs = outs(param) if callable(outs) else outs
    div = div(param) if callable(div) else div
    return oid, ins, outs, div


def run(name, inputs, param=0, divergent=False):
    """outputs (a tuple of arrays) of `name` with `param` over the cases of `inputs`, a multiple of 64 of them"""
    global _failed
    if _failed is not None:
        raise RuntimeError("not run: an earlier call failed (%s)" % _failed)
    oid, ins, outs, div = signature(name, param)
    mult = param if name in MULTI else 1
    assert len(inputs) == len(ins), name
    n = inputs[0].size // mult
    assert n > 0 and n % 64 == 0, (name, n)
    assert not divergent or div, "%s has no lane-divergent form" % name
    arrs = []
    for a, t in zip(inputs, ins):
        a = np.ascontiguousarray(a, dtype=t)
        assert a.size == n * mult, (name, a.size, n)
        arrs.append(a)
    res = [np.empty(n * mult, t) for t in outs]
    pin = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    pout = (ctypes.c_void_p * len(res))(*[r.ctypes.data for r in res])
    err = load().psk_dev_prims_run(oid | (param << 8) | (DIVERGENT if divergent else 0), pin, pout, n)
    if err != 0:
        _failed = "psk_dev_prims_run(%s, param %d): HIP error %d" % (name, param, err)
        raise RuntimeError(_failed)
    return tuple(res)
