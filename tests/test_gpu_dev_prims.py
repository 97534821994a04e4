"""Every device-math and wave primitive of psk_libm.h, psk_device_math.h, psk_wave.h, psk_wave_scan_gen.h and psk_tile_any.h run
on the GPU by itself (tests/support/dev_prims.hip, compiled with the product's flags into psk_soft_amd/libpsk_dev_prims.so) and held bit
for bit to the reference side of tests/dev_prim_cases.py: the oracle's exported primitives, this machine's glibc, numpy models
of the documented DPP step order.  The comparison rule is assert_parity's, per element and without a tolerance.  Every case set
runs grouped by class (whole waves ordinary, whole waves rare) and under a fixed shuffle (rare and ordinary lanes share waves:
ordinary lanes go through the wave-uniform patch code); the forms behind __any guards and the AtanTabWave forms run once more
inside a lane-divergent branch.  tests/test_dev_prim_cases.py (no GPU) checks that the cases reach what they are meant to.
DESIGN.md section 4.4 has the table, the counts, the durations and the rehearsal."""
import numpy as np
import pytest

from tests import dev_prim_cases as dc
from tests import dev_prims_lib as dp

pytestmark = pytest.mark.gpu
N_SHOWN = 3  # operands shown per (form, layout, case set, class) that differs


def _report(form, how, c, klass, names, ix, ins, out_k, bad):
    """one line per case set and class among the elements of `bad`: how many differ, the first few operands as hex patterns"""
    pos = np.nonzero(bad)[0]
    case = ix[pos // c.unit]
    key = c.set_of[case] * 16 + (klass[case] if klass is not None else 0)
    lines = []
    for k in np.unique(key):
        sel = pos[key == k]
        cls = "" if klass is None else " class %s" % names[k % 16]
        lines.append("%s [%s] %s%s output %d: %d of %d differ, first at operands %s" % (
            form.label, how, c.sets[k // 16], cls, out_k, sel.size, bad.size, " ".join(dc.hexes(ins, i) for i in sel[:N_SHOWN])))
    return lines


def run_family(family):
    failures, compared = [], 0
    forms = [f for f in dc.FORMS if f.family == family]
    for kind in dict.fromkeys(f.kind for f in forms):
        c = dc.Cases(kind)
        klass, names = dc.classes(kind, c.inputs) if c.unit == 1 else (None, None)
        lay = dc.layouts(kind, c.n, klass)
        for form in (f for f in forms if f.kind == kind):
            ref = dc.form_reference(form, c.inputs)
            runs = [(name, ix, False) for name, ix in lay.items()]
            if form.divergent:
                runs.append(("shuffled, lane-divergent", lay["shuffled"], True))
            for how, ix, divergent in runs:
                ins = dc.take(c.inputs if form.n_in is None else c.inputs[:form.n_in], ix, c.unit)
                want = dc.take(ref, ix, c.unit)
                got = dp.run(form.op, ins, form.param, divergent=divergent)
                for k, mask in enumerate(dc.compare_mask(form, want)):
                    bad = dc.differs(got[k], want[k], raw=form.rule == "raw", zeros=form.rule == "zeros")
                    if mask is not None:
                        bad &= mask
                    compared += int(bad.size if mask is None else mask.sum())
                    if bad.any():
                        failures += _report(form, how, c, klass, names, ix, ins, k, bad)
    print("%s: %d forms, %d values compared, %d lines of differences" % (family, len(forms), compared, len(failures)))
    assert not failures, "\n" + "\n".join(failures)


def test_libm():
    """atan2f_wave with the table in lanes and in constants, sincosf_wave with both forms of `dep`, lm_div_known"""
    run_family("libm")


def test_slicing_and_bits():
    """lm_slice8_fast (sector wherever near is false, near against the host build), slice_8psk and slice_8psk_atan with both
    table forms, qpsk_bits with both maps.  (The near / far class split and the reference of `near` come from psk_libm.h
    compiled for the host when this test runs; tests/test_dev_prim_cases.py pins that build to glibc and the oracle.)"""
    run_family("slicing")


def test_complex():
    """norm_f, cmul<true> and <false>, cdiv<true> (the Annex G recoveries behind wave-uniform tests)"""
    run_family("complex")


def test_complex_pow():
    """cpow_uint<true> and <false> for M = 1, 2, 3, 4, 5, 8, 16, 64"""
    run_family("cpow")


def test_unwrap_and_fit():
    """to_long_x86 and unwrap_count with both forms of `dep`, wrap_test, fit_denominator and fit_value for every window length"""
    run_family("unwrap_fit")


def test_fit_known():
    """fit_known + fit_value_known: a wave per (xdelta, window length), its members are wave-uniform; estimate and slope are
    both held to the oracle's bit for bit, non-finite sums included"""
    run_family("fit_known")


def test_wave_primitives():
    """the DPP scans (all 32 generated interleaved ones among them), maxima and minima, lane shifts and reads, v_med3_i32"""
    run_family("wave")


def test_first_maximum_reductions():
    """psk_tile_any.h, the reductions behind every timing pick of the run-time and wide front stages: any_merge, any_max_f64,
    any_min_u32 and their level-by-level forms of eight, held to "the maximum over 64 values", "the minimum over 64 values"
    and the merge's three lines -- the extremum in every lane in turn, equal extrema on both sides of every DPP row boundary,
    -inf / 0xFFFFFFFF in every lane but one, finite values next to NaN; zeros of either sign count as equal (the callers only
    test ==)"""
    run_family("any")
