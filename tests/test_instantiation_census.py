"""The census table (tests/instantiation_census.py) against the Makefile, its draws against their pinned digests, and the
conditions its stimuli have to meet for the GPU rows (tests/test_gpu_instantiations.py) to mean what they say -- all with
the CPU oracle, no GPU."""
import json
import os
import time

import numpy as np
import pytest

from tests import instantiation_census as ic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instantiation_census.json")


def test_every_compiled_unit_has_a_row():
    """The rows are the Makefile's units, each once: 231 float units, 90 packet-format units, 15 time-tiled fronts, minus
    nothing.  A unit the Makefile grows has no path (instantiation_census.path_of raises) or moves a total."""
    units = ic.makefile_units()
    counts = {k: len(v) for k, v in units.items()}
    print("compiled units: %(float)d float, %(format)d packet-format, %(tile)d time-tiled fronts" % counts)
    assert counts == dict(float=231, format=90, tile=15)
    rows = ic.all_rows()
    assert sorted(r.unit for r in rows) == sorted(units["float"] + units["format"] + units["tile"])
    assert len({r.name for r in rows}) == len(rows) == 336
    assert {p: len(ic.rows(p)) for p in ic.PATHS} == ic.PATH_COUNTS
    # the rule of the two variants the launch lines do not tell apart: the H8_E0 rows are the H0 rows over again
    h0 = {r.S: r for r in ic.rows("settle_in_place") if r.H == 0}
    for r in ic.rows("settle_in_place_h8"):
        assert r.digest() != h0[r.S].digest() and r.props == h0[r.S].props and r.env == {"PSK_SOFT_REREAD": "0"}
        assert all(np.array_equal(a, b) for a, b in zip(r.packets, h0[r.S].packets))
    # rows nobody can drive are named, and only format_exact may have any
    from tests.test_gpu_instantiations import UNREACHABLE

    assert UNREACHABLE <= {r.name for r in ic.rows("format_exact")}
    print("rows: %d, minus %d unreachable" % (len(rows), len(UNREACHABLE)))
    # a unit that is not one of the family's has no row to hide behind
    for bad in ("psk_fast_S33_H1_E0", "psk_fast_S17_H8_E1", "psk_fast_S8_H16_E0", "psk_fast_cs16_S17_H1_E0", "psk_tile_S17_H1"):
        with pytest.raises(ValueError):
            ic.path_of(bad)


def test_every_draw_is_the_pinned_one():
    """sha256 of properties, environment and packet bytes per row: a row's stimulus changes only on purpose"""
    with open(GOLDEN) as f:
        pinned = {e["name"]: e["sha256"] for e in json.load(f)}
    rows = ic.all_rows()
    assert sorted(pinned) == sorted(r.name for r in rows)
    wrong = [r.name for r in rows if r.digest() != pinned[r.name]]
    assert not wrong, wrong


def test_shapes(oracle_mod):
    """Three calls a row; the first emits the class's history and two blocks more, every call ends in a partial block -- of
    1 .. 3, 60 .. 100 and 127 symbols --, no packet is a multiple of samplesPerBaud, numAvg sits on an edge of its class, and
    the oracle emits what the table says."""
    t0 = time.perf_counter()
    seen_M, seen_n, seen_diff = set(), set(), set()
    for r in ic.all_rows():
        S, A = r.props["samplesPerBaud"], r.props["numAvg"]
        Hc = 1 if r.fmt else 8 if r.H == 0 else r.H
        assert S == r.S and A in {1: (128,), 2: (129, 256), 4: (257, 512), 8: (513, 1024)}[Hc], r.name
        assert len(r.packets) == 3 and all(p.size % 2 == 0 and (p.size // 2) % S for p in r.packets), r.name
        assert r.emit == ic.emitted(r.props, [p.size // 2 for p in r.packets]), r.name
        assert r.emit[0] // ic.KB >= Hc + 2 and 1 <= r.emit[0] % ic.KB <= 3, r.name
        assert 60 <= r.emit[1] % ic.KB <= 100 and r.emit[2] % ic.KB == 127, r.name
        want = [np.float32 if r.path == "format_exact" else ic.FORMAT_DTYPE.get(r.fmt, np.float32)] + [ic.FORMAT_DTYPE.get(r.fmt, np.float32)] * 2
        assert [p.dtype for p in r.packets] == [np.dtype(t) for t in want], r.name
        ref = ic.oracle_calls(oracle_mod, r)
        assert [c["phase"].size for c in ref] == r.emit and [c["index"].size for c in ref] == r.emit, r.name
        seen_M.add(r.props["constelationSize"]), seen_n.add(r.props["phaseAvg"]), seen_diff.add(r.props["differentialDecoding"])
    assert seen_M == {2, 4, 8} and seen_n == {1, 2, 50, 385} and seen_diff == {0, 1}
    print("shapes of 336 rows with the oracle: %.2f s" % (time.perf_counter() - t0))


def test_a_sure_near_tie_in_every_block(oracle_mod):
    """The four tie-driven paths and the two format paths: the float64 model of the window sums finds a position with its two
    largest sums within 2^-22 of each other in every block of every call, the tail block included -- below the smallest
    acceptance threshold a unit's screening can have, so every block is settled exactly; the number of blocks is what the GPU
    test holds timing_exact_blocks against.  The float streams stay finite throughout -- but for the first soft symbol of a
    channel with differential decoding, which the reference divides by a `last` of zero."""
    t0 = time.perf_counter()
    n = 0
    for path in ic.TIE_PATHS + ("format_settle", "format_exact"):
        for r in ic.rows(path):
            iq = np.concatenate([np.asarray(p).astype(np.float64) for p in r.packets])
            if path == "format_exact":
                assert np.isnan(iq).sum() == 1 and np.isnan(np.asarray(r.packets[0])[0::2]).sum() == 1, r.name
                iq = np.nan_to_num(iq, nan=float(ic.FORMAT_AMPLITUDE[r.fmt]))
            flags = ic.near_tie_blocks(iq, r.props, r.emit)
            assert [len(f) for f in flags] == r.blocks(), r.name
            if path == "format_exact":  # (the calls in the row's format; none of their windows holds the poisoned symbol)
                assert np.nonzero(np.isnan(r.packets[0]))[0][0] // (2 * r.S) < r.emit[0] - 1, r.name
                flags = flags[1:]
            assert all(all(f) for f in flags), r.name
            n += sum(len(f) for f in flags)
            if path in ic.TIE_PATHS:
                for k, c in enumerate(ic.oracle_calls(oracle_mod, r)):
                    first = 2 if k == 0 and r.props["differentialDecoding"] else 0
                    assert np.isfinite(c["soft"][first:]).all() and np.isfinite(c["phase"]).all(), r.name
    print("a near-tie in each of %d blocks: %.2f s" % (n, time.perf_counter() - t0))


def test_the_overflowing_power_leaves_the_third_call_finite_but_for_its_end(oracle_mod):
    """exact_tier_h1: calls 0 and 1 are finite; in call 2 at least 95 % of the oracle's soft and phase values are finite and
    the M-th power of the sample picked for the scaled symbol overflows (the screened tier refuses the call there), while
    every sample and every energy is finite (no other refusal site)."""
    for r in ic.rows("exact_tier_h1"):
        assert r.props["constelationSize"] in (4, 8), r.name
        for p in r.packets:
            assert np.isfinite(p).all() and np.isfinite(p.astype(np.float32)[0::2] ** 2 + p.astype(np.float32)[1::2] ** 2).all(), r.name
        ref = ic.oracle_calls(oracle_mod, r)
        for k, c in enumerate(ref[:2]):
            first = 2 if k == 0 and r.props["differentialDecoding"] else 0  # (the reference divides by a `last` of zero)
            assert np.isfinite(c["soft"][first:]).all() and np.isfinite(c["phase"]).all(), r.name
        for key in ("soft", "phase"):
            assert np.isfinite(ref[2][key]).mean() >= 0.95, (r.name, key)
        # the sample the oracle picks for the scaled symbol: the larger component of its M-th power is beyond binary32
        # whatever the order of the multiplications (the values themselves may come out finite: arg() of infinities is)
        g, S, M = r.draw["symbol"], r.S, r.props["constelationSize"]
        k2 = g - (sum(r.emit) - r.emit[2])
        assert r.emit[2] - 3 <= k2 < r.emit[2], r.name
        iq = np.concatenate(r.packets).astype(np.float64)
        j = g * S + int(ref[2]["index"][k2])
        assert np.hypot(iq[2 * j], iq[2 * j + 1]) ** M / np.sqrt(2.0) > float(np.finfo(np.float32).max), r.name


def test_the_poisoned_first_call_never_recovers(oracle_mod):
    """format_exact: the oracle's phase is NaN, infinite or astronomically large (an unwrap count of more than 32 bits: what
    (long)NaN leaves behind) everywhere in the two calls sent in the row's format -- the feedback the screened tier's fit stage
    refuses; what the rows compare there is bits, sampleIndex, the non-finite patterns and the bits of whatever is finite."""
    for r in ic.rows("format_exact"):
        ref = ic.oracle_calls(oracle_mod, r)
        for c in ref[1:]:
            with np.errstate(invalid="ignore"):
                far = ~np.isfinite(c["phase"]) | (np.abs(c["phase"]) > 2.0 ** 31 * 2 * np.pi)
            assert far.all(), r.name
            assert c["index"].size and c["bits"].size, r.name
