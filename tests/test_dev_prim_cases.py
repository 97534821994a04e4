"""The case sets of the device-primitive tests (tests/dev_prim_cases.py) without a GPU: their pinned digests, the reference side
run to its end for every form, the HOST build of psk_libm.h held to glibc on the directed cases (tests/support/libm_pin.cpp
draws at random only), and the conditions on the inputs -- evaluated with the reference alone -- that keep
tests/test_gpu_dev_prims.py from passing vacuously.  DESIGN.md section 4.4."""
import json
import os
import re

import numpy as np
import pytest

from tests import dev_prim_cases as dc
from tests import dev_prims_lib as dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dev_prim_cases.json")
u32, f32, f64 = np.uint32, np.float32, np.float64


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(kind):
        if kind not in cache:
            c = dc.Cases(kind, digests=True)
            klass, names = dc.classes(kind, c.inputs) if c.unit == 1 else (None, None)
            cache[kind] = (c, klass, names, dc.layouts(kind, c.n, klass))
        return cache[kind]

    yield get
    cache.clear()


def test_every_case_set_is_the_pinned_one(cases):
    """sha256 of the operand bytes per case set: a set changes only on purpose (tests/golden/make_dev_prim_cases.py)"""
    with open(GOLDEN) as f:
        pinned = {e["name"]: e for e in json.load(f)}
    seen = {}
    for kind in dc.KINDS:
        c = cases(kind)[0]
        for name in c.sets:
            seen[name] = dict(name=name, cases=int(c.counts[name]), sha256=c.digests[name])
    assert sorted(seen) == sorted(pinned)
    wrong = [n for n in seen if seen[n] != pinned[n]]
    assert not wrong, wrong


def test_the_table_lists_every_operation_and_form():
    """every entry of the device library is driven, in every form the issue lists, and the library is built the product's way"""
    assert {f.op for f in dc.FORMS} == set(dp.OPS)
    labels = {f.label for f in dc.FORMS}
    assert len(labels) == len(dc.FORMS) == 93
    for N in range(1, 33):
        assert "wave_scan_f32_multi<%d>" % N in labels
    for M in (1, 2, 3, 4, 5, 8, 16, 64):
        assert {"cpow_uint<true>(M=%d)" % M, "cpow_uint<false>(M=%d)" % M} <= labels
    assert {"any_merge", "any_max_f64", "any_min_u32", "any_max_f64_multi<8>", "any_min_u32_multi<8>"} <= labels
    for f in dc.FORMS:
        if f.family == "any":  # psk_tile_any.h: whole waves only, refused in the divergent mode like the AtanTabDev forms
            assert not f.divergent and not dp.signature(f.op, f.param)[3], f.label
    for f in dc.FORMS:  # a lane-divergent run only of what has one, and of everything behind an __any guard or AtanTabWave
        _, _, _, can = dp.signature(f.op, f.param)
        assert can or not f.divergent, f.label
    guarded = {"atan2f_wave<AtanTabWave>", "sincosf_wave(dep=0)", "slice_8psk<AtanTabWave>", "slice_8psk_atan<AtanTabWave>",
               "cmul<true>", "cdiv<true>"} | {"cpow_uint<true>(M=%d)" % M for M in dc.CPOW_M}
    assert {f.label for f in dc.FORMS if f.divergent} == guarded
    src = open(os.path.join(ROOT, "tests", "support", "dev_prims.hip")).read()
    assert '#include "psk_tile_any.h"' in src  # (the header itself, unchanged: not a copy of its functions)
    mk = open(os.path.join(ROOT, "psk_soft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^\$\(OBJDIR\)/dev_prims\.o:.*\bpsk_tile_any\.h\b", mk, re.M)
    rule = re.search(r"^\$\(OBJDIR\)/dev_prims\.o:.*\n\t(.*)$", mk, re.M).group(1)
    assert rule == "$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -c ../../tests/support/dev_prims.hip -o $@"
    assert "dev_prims" not in re.search(r"^\$\(LIB\):.*$", mk, re.M).group(0)
    assert re.search(r"^all:.*\$\(DEVPRIMS\)", mk, re.M)


def test_the_reference_side_runs_to_its_end(cases):
    """every form's reference over all its cases: the right shapes and types, a mask that leaves something to compare"""
    for form in dc.FORMS:
        c = cases(form.kind)[0]
        ref = dc.form_reference(form, c.inputs)
        _, ins, outs, _ = dp.signature(form.op, form.param)
        assert len(ref) == len(outs) and [r.dtype for r in ref] == [np.dtype(t) for t in outs], form.label
        assert all(r.size == c.inputs[0].size for r in ref), form.label
        for mask in dc.compare_mask(form, ref):
            assert mask is None or mask.mean() >= 0.5, form.label  # (the screened forms: a finite result in half the cases)


def _directed(c):
    """the cases of a kind that are not the random set's"""
    keep = np.array([not n.endswith("/random") for n in c.sets])[c.set_of]
    return tuple(a[keep] for a in c.inputs)


def test_the_host_build_matches_glibc_on_the_directed_cases(cases):
    """lm_atan2f, lm_atanf, the straight-line forms with their companions, lm_sincosf, lm_div_known, and lm_slice8_fast's sector
    wherever near is false -- on every directed case set, and on the random ones as well"""
    for part in (_directed, lambda c: c.inputs):
        y, x = part(cases("atan2")[0])
        want = dc.oracle_array("atan2f", (y, x), (f32,))[0]
        assert not dc.differs(dc._host_call("lmh_atan2f", (y, x), (f32,))[0], want).any()
        got, special = dc._host_call("lmh_atan2f_ordinary", (y, x), (f32, np.int32))
        assert not dc.differs(got, want).any()
        assert np.array_equal(special != 0, dc.classes("atan2", (y, x))[0] == 2)
        one = np.ones_like(y)
        assert not dc.differs(dc._host_call("lmh_atanf", (y,), (f32,))[0], dc.oracle_array("atan2f", (y, one), (f32,))[0]).any()
        (t,) = part(cases("sincos")[0])
        want = dc.oracle_array("sincosf", (t,), (f32, f32))
        for fn in ("lmh_sincosf", "lmh_sincosf_ordinary"):
            got = dc._host_call(fn, (t,), (f32, f32))
            assert not dc.differs(got[0], want[0]).any() and not dc.differs(got[1], want[1]).any(), fn
        assert not dc.differs(dc.oracle_array("polar1", (t,), (f32, f32))[0], want[1]).any()  # polar(1, t) = (cosf, sinf)
        a, b, rb = part(cases("div_known")[0])
        with np.errstate(all="ignore"):
            assert not dc.differs(dc._host_call("lmh_div_known", (a, b, rb), (f64,))[0], a / b).any()
        re_, im = part(cases("slice8")[0])
        sector, near = dc.host_slice8_fast(re_, im)
        want = dc.oracle_array("slice8", (re_, im), (np.int32,))[0]
        assert np.array_equal(sector[near == 0], want[near == 0])


def _waves(klass, ix):
    return klass[ix].reshape(-1, 64)


def test_every_class_in_whole_waves_and_in_mixed_ones(cases):
    """rare and special (atan2f), tiny, big and nonfinite (sincosf), near (the slicer) and the recoveries (cmul, cdiv): the
    grouped layout has a wave of nothing else, the shuffled one a wave that holds the class next to ordinary lanes"""
    for kind in ("atan2", "sincos", "slice8", "cmul", "cdiv"):
        c, klass, names, lay = cases(kind)
        g, s = _waves(klass, lay["grouped"]), _waves(klass, lay["shuffled"])
        for k in range(1, len(names)):
            assert (g == k).all(axis=1).any(), (kind, names[k])
            assert ((s == k).any(axis=1) & (s == 0).any(axis=1)).any(), (kind, names[k])
        assert (g == 0).all(axis=1).any(), kind
        for ix in lay.values():  # a layout is the cases, all of them, and padding from among them
            assert ix.size % 64 == 0 and np.array_equal(np.unique(ix), np.arange(c.n)), kind


def test_atanf_ranges_from_both_sides(cases):
    """each of the five ranges of s_atanf.c, and |y/x| within 8 ulps below and at or above each of its bounds, 2^-29 and 2^25"""
    y, x = cases("atan2")[0].inputs
    fin = dc.classes("atan2", (y, x))[0] != 2
    a = dc.atan2_ratio(y[fin], x[fin])
    assert set(np.unique(dc.atan_range(a))) == {0, 1, 2, 3, 4}
    ia = a.view(u32).astype(np.int64)
    for bound in (0x3EE00000, 0x3F300000, 0x3F980000, 0x401C0000, 0x31000000, 0x4C000000):
        assert ((ia >= bound - 8) & (ia < bound)).any() and ((ia >= bound) & (ia <= bound + 8)).any(), hex(bound)
        assert (ia == bound - 1).any() and (ia == bound).any(), hex(bound)
    k = (((y.view(u32) >> 23) & 0xFF).astype(int) - ((x.view(u32) >> 23) & 0xFF).astype(int))[fin]
    assert {-62, -61, -60, -59, 59, 60, 61, 62} <= set(np.unique(k))


def test_near_on_both_sides_of_every_boundary_ray(cases):
    """the eight boundary rays of the 8-PSK slicer (odd multiples of pi/8), each from both sides -- sixteen half-neighbourhoods:
    near is true and false in each, and among the near cases of a ray both neighbouring sectors occur in the oracle's index"""
    re_, im = cases("slice8")[0].inputs
    ok = np.isfinite(re_) & np.isfinite(im) & ((re_ != 0) | (im != 0))
    re_, im = re_[ok], im[ok]
    near = dc.host_slice8_fast(re_, im)[1] != 0
    index = dc.oracle_array("slice8", (re_, im), (np.int32,))[0]
    u = np.arctan2(im.astype(f64), re_.astype(f64)) / (np.pi / 4) - 0.5  # boundary j sits at u = j
    j = np.round(u)
    side, close = u > j, np.abs(u - j) < 0.01
    j = j.astype(int) % 8
    for ray in range(8):
        for s in (False, True):
            sel = close & (j == ray) & (side == s)
            assert near[sel].any() and (~near[sel]).any(), (ray, s)
        sel = close & (j == ray) & near
        assert {ray, (ray + 1) % 8} <= set(np.unique(index[sel])), ray


def test_every_recovery_branch_is_taken(cases):
    """__mulsc3: an infinite left factor, an infinite right one, both, an overflowed product, nothing to recover; __divsc3:
    a zero divisor, an infinite numerator, an infinite divisor, none -- and the divisor (0, 0) in all four signs"""
    assert set(np.unique(dc.cmul_branch(*cases("cmul")[0].inputs))) == {0, 1, 2, 3, 4, 5}
    a, b, c, d = cases("cdiv")[0].inputs
    assert set(np.unique(dc.cdiv_branch(a, b, c, d))) == {0, 1, 2, 3, 4}
    z = (c == 0) & (d == 0)
    assert len({(bool(s), bool(t)) for s, t in zip(np.signbit(c[z]), np.signbit(d[z]))}) == 4
    for M in dc.CPOW_M:  # the powers: recoveries inside (a result that is not finite) and plain cases, both plentiful
        klass = cases("cpow/%d" % M)[1]
        assert 0.001 < klass.mean() < 0.5, M


def test_half_integer_unwrap_quotients_from_both_sides(cases):
    """(phaseEstimate - thisPhase) / 2 pi next to k + 1/2 from below and from above for every k = +-2^j up to 2^20: within
    2^-20 |k|, a few float steps of phaseEstimate (its spacing, over 2 pi, is about 2^-24 |k|), and never further than 1/4"""
    c = cases("unwrap")[0]
    pe, th = c.inputs
    with np.errstate(invalid="ignore"):
        q = (pe.astype(f64) - th) / (2 * np.pi)
    fin = np.isfinite(q) & (np.abs(q) < 2.0 ** 22)
    q = q[fin]
    k = np.floor(q)
    d = q - k - 0.5
    close = np.abs(d) < np.minimum(0.25, 2.0 ** -20 * np.maximum(1.0, np.abs(k)))
    for j in range(21):
        for kk in (2.0 ** j, -(2.0 ** j)):
            sel = close & (k == kk)
            assert (d[sel] < 0).any() and (d[sel] > 0).any(), kk
    want = dc.oracle_array("unwrap", (pe, th), (np.int64,))[0]
    assert (want == np.iinfo(np.int64).min).any()  # NaN, infinities and counts beyond 2^63


def test_the_order_of_additions_shows_in_the_scans(cases):
    """in at least half of the mixed-sign waves the model's last lane differs in its bits from the left-to-right sum"""
    for kind in ("scan_f64",) + tuple("scan_f32_multi/%d" % n for n in range(1, 33)):
        v = cases(kind)[0].inputs[0]
        if kind == "scan_f64":
            w, n_mixed = v.reshape(-1, 64)[:dc.N_SCAN_WAVES], dc.N_SCAN_WAVES
            planes = [w]
        else:
            N = int(kind.split("/")[1])
            n_mixed = 128
            planes = [np.ascontiguousarray(v.reshape(-1, 64, N)[:n_mixed, :, k]) for k in range(N)]
        for w in planes:
            model = dc.scan_model(w)[:, 63]
            seq = np.add.accumulate(w, axis=1)[:, 63]
            assert dc.differs(model, seq).mean() >= 0.5, kind
    v = cases("scan_f32_multi/32")[0].inputs[0].reshape(-1, 64, 32)  # each of the N interleaved scans has data of its own
    assert len({v[:, :, k].tobytes() for k in range(32)}) == 32


def test_wave_max_stays_within_its_contract(cases):
    """non-negative and no NaN, with +0, denormals and +inf among the inputs"""
    v = cases("max_f32")[0].inputs[0]
    b = v.view(u32)
    assert (b <= 0x7F800000).all() and (b == 0).any() and ((b > 0) & (b < 0x800000)).any() and (b == 0x7F800000).any()
    w = b.reshape(-1, 64)
    assert (w.max(axis=1) == 0).any() and ((w.max(axis=1) > 0) & (w.max(axis=1) < 0x800000)).any()


def test_fit_cases_cover_every_window_length(cases):
    """every pts 2 .. 65535 with each of the four xdelta, for the denominator, the fit and the steady-state fit (a wave per
    pair, uniform); sums from zero through 2400 rad times 65535 points up to float overflow of the results, and non-finite"""
    for kind, xi in (("fit_den", 0), ("fit_value", 2), ("fit_known", 2)):
        c = cases(kind)[0]
        x, p = c.inputs[xi], c.inputs[xi + 1]
        pairs = np.unique(x.view(u32).astype(np.uint64) << np.uint64(32) | p.astype(np.uint64))
        assert pairs.size == 4 * 65534 and set(np.unique(x)) == set(dc.FIT_XDELTA) and p.min() == 2 and p.max() == 65535, kind
    c = cases("fit_known")[0]
    ys, xys, x, p = c.inputs
    assert (x.reshape(-1, 64) == x.reshape(-1, 64)[:, :1]).all() and (p.reshape(-1, 64) == p.reshape(-1, 64)[:, :1]).all()
    fit, m = dc.reference("fit_known", c.inputs)
    assert (ys == 0).any() and np.isnan(ys).any() and np.isinf(ys).any() and np.isinf(xys).any()
    fin = np.isfinite(fit)
    assert 0.5 < fin.mean() < 0.95 and np.isinf(fit).any() and np.isinf(m).any()  # results up to overflow, and beyond
    assert (np.abs(fit[fin]) > 2400.0).any() and (np.abs(ys[np.isfinite(ys)]) > 2400.0 * 65535).any()


def test_division_numerators_of_every_kind(cases):
    """lm_div_known and the sums of both fits: numerators that are -0.0, +0.0, infinite and NaN, quotients that are denormal, that
    overflow, and on both sides of the 2^-500 and 2^500 where the three-step quotient hands over to the division -- with each of
    the product's divisors (2 pi, a float's value, an integer)"""
    a, b, _ = cases("div_known")[0].inputs
    with np.errstate(all="ignore"):
        q = a / b
    kinds = {"two_pi": b == 2 * np.pi, "integer": (b == np.floor(b)) & (b >= 1) & (b <= 65535), "float": b != np.floor(b)}
    tiny = 2.2250738585072014e-308
    for name, sel in kinds.items():
        aa, qq = a[sel], np.abs(q[sel])
        assert ((aa == 0) & np.signbit(aa)).any() and ((aa == 0) & ~np.signbit(aa)).any(), name
        assert np.isposinf(aa).any() and np.isneginf(aa).any() and np.isnan(aa).any(), name
        assert ((qq > 0) & (qq < tiny)).any(), name
        assert name != "float" or (np.isinf(qq) & np.isfinite(aa)).any()  # (a divisor below 1: the others cannot overflow)
        for edge in (2.0 ** -500, 2.0 ** 500):
            assert ((qq < edge) & (qq > edge * 2.0 ** -12)).any() and ((qq >= edge) & (qq < edge * 2.0 ** 12)).any(), (name, edge)
    for kind in ("fit_value", "fit_known"):
        ys, xys = cases(kind)[0].inputs[:2]
        for v in (ys, xys):
            assert ((v == 0) & np.signbit(v)).any() and np.isinf(v).any() and np.isnan(v).any(), kind
            assert ((np.abs(v) > 0) & (np.abs(v) < tiny)).any() and (np.abs(v) > 1e300).any(), kind


def test_first_maximum_cases_reach_every_lane_and_tie(cases):
    """psk_tile_any.h's case sets: the extremum sits in each of the 64 lanes in turn (far from the others and one step from
    them), equal extrema occur in every pair of lanes from {0, 15, 16, 31, 32, 47, 48, 63} and nowhere else in the wave, every
    lane but one holds the identity (-inf, 0xFFFFFFFF) for each of the 64 lanes, finite values stand next to NaN (and the
    reference drops the NaN), the unsigned values lie on both sides of 2^31 -- in each of the eight interleaved planes too,
    which all differ; the merges hold equal `best` with the lower phase on either side, and equal phases."""
    for kind in dc.ANY_KINDS:
        c = cases(kind)[0]
        U = c.unit // 64
        v = c.inputs[0].reshape(-1, 64, U)
        is_f = v.dtype == f64
        names = [n.rsplit("/", 1)[1] for n in c.sets]
        assert len({v[:, :, u].tobytes() for u in range(U)}) == U, kind
        for u in range(U):
            w = v[:, :, u]
            part = {n: w[c.set_of == j] for j, n in enumerate(names)}
            best = (lambda x: np.fmax.reduce(x, axis=1)) if is_f else (lambda x: x.min(axis=1))
            e = part["each_lane"]
            hit = e == best(e)[:, None]
            assert (hit.sum(axis=1) == 1).all() and np.array_equal(np.nonzero(hit[:64])[1], np.arange(64)), kind
            assert np.array_equal(np.nonzero(hit[64:])[1], np.arange(64)), kind
            rest = e[64:][~hit[64:]].reshape(64, 63)  # (one step from 63 equal values)
            assert (rest == rest[:, :1]).all(), kind
            p = part["pairs"]
            hit = p == best(p)[:, None]
            assert [tuple(np.nonzero(h)[0]) for h in hit] == list(dc.ANY_PAIRS) and len(dc.ANY_PAIRS) == 28, kind
            one = part["inf_but_one" if is_f else "max_but_one"]
            ident = np.isneginf(one) if is_f else one == 0xFFFFFFFF
            assert ((~ident).sum(axis=1) <= 1).all() and np.array_equal(np.nonzero(~ident | np.eye(64, dtype=bool))[1], np.arange(64)), kind
            eq = part["equal"][: (10 if is_f else 5)]
            assert (eq.view(np.uint64 if is_f else u32) == eq.view(np.uint64 if is_f else u32)[:, :1]).all(), kind
            if is_f:
                n = part["nan"]
                assert (np.isnan(n).any(axis=1) & np.isfinite(n).any(axis=1)).all() and np.isfinite(best(n)).all(), kind
                assert (np.isfinite(n).sum(axis=1) == 1).sum() >= 64, kind
                z = part["equal"][10:]
                assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any(), kind
            else:
                r = part["random"]
                assert ((r < 1 << 31).any(axis=1) & (r >= 1 << 31).any(axis=1)).all(), kind
                assert (r.astype(np.int32).min(axis=1).astype(u32) != r.min(axis=1)).mean() > 0.9, kind  # a signed minimum is another
    ab, as_, bb, bs, ak, bk = cases("any_merge")[0].inputs
    tie = ab == bb
    assert (tie & (ak < bk)).sum() > 1000 and (tie & (ak > bk)).sum() > 1000 and (tie & (ak == bk)).sum() > 100
    best, second, k = dc.reference("any_merge", (ab, as_, bb, bs, ak, bk))
    assert (k[tie] == np.minimum(ak, bk)[tie]).all()  # the first of equal sums
    assert ((ab == 0) & (bb == 0) & (np.signbit(ab) != np.signbit(bb))).any() and np.isnan(ab).any() and (ak == 0x7FFFFFFF).any()
