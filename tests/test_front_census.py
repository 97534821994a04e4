"""The census of the run-time and wide front stages (tests/front_census.py) without a GPU: the table against the issue's list,
the draws against their pinned digests, the shapes against the tile and variant rules restated here, and -- with the CPU oracle
and the float64 models of the window sums -- the conditions that keep tests/test_gpu_front_census.py from passing vacuously.  Its
comparison is then fed stand-in results built from the models and must report each at its row and call.  DESIGN.md section 4.8."""
import copy
import json
import os
import time

import numpy as np
import pytest

from tests import front_census as fc
from tests import test_gpu_front_census as gf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_census.json")
MAIN = ("any1", "any4", "any16", "wide")


@pytest.fixture(scope="module")
def refs(oracle_mod):
    """the oracle's streams of every row, computed once and left alone"""
    return {r.name: fc.oracle_calls(oracle_mod, r) for r in fc.all_rows()}


# ---- the rules of the library, restated (not imported) -------------------------------------------------------------------

def body_of(max_S):
    """launch_tile_front_any: the body by the launch's largest samplesPerBaud; wider symbols are psk_wide.hip's"""
    return "wide" if max_S > 1024 else 1 if max_S <= 64 else 4 if max_S <= 256 else 16


def tile_blocks(total_blocks, z, k_min, max_A, target=4096):
    """place_tiles: blocks of 128 symbols to a tile of a launch set -- its blocks (times the chunks of its widest channel for the
    wide symbols) over the target number of tiles, at least k_min and at most 16; lengthened towards the longest window only
    where tiles enough remain to fill the machine"""
    bz = total_blocks * z
    K = min(max(bz // target, k_min), 16)
    k_win = -(-max_A // 128)
    if K < k_win:
        k_fill, k_long = bz // (target // 2), min(k_win, 64)
        K = k_long if k_fill > k_long else max(k_fill, K)
    return K


def test_the_table_is_the_issues():
    S_of = {v: sorted({r.S for r in fc.rows(v)}) for v in fc.VARIANTS}
    assert S_of == dict(any1=[2, 8, 16, 33, 40, 63, 64], any4=[40, 65, 128, 255, 256], any16=[40, 100, 257, 1000, 1023, 1024],
                        wide=[1025, 2048, 2049, 5000], far=[8, 1025])
    rows = fc.all_rows()
    assert len({r.name for r in rows}) == len(rows) == 28 + 23 + 24 + 16 + 2
    for v in MAIN:  # every kind at every samplesPerBaud; the body the launch picks is the variant's, whatever the row's own width
        assert {(r.S, r.kind) for r in fc.rows(v) if not r.fmt} == {(S, k) for S in S_of[v] for k in fc.KINDS}, v
        assert body_of(max(r.S for r in fc.rows(v))) == dict(any1=1, any4=4, any16=16, wide="wide")[v]
        lo, hi = fc.S_RANGE[v]
        assert lo <= max(r.S for r in fc.rows(v)) <= hi
    assert [(r.S, r.kind, r.fmt, r.packets[0].dtype) for r in fc.rows("any4") if r.fmt] == [
        (65, "tie", f, np.dtype(fc.FORMAT_DTYPE[f])) for f in ("cs16", "cs8", "cf16")]
    assert all(r.packets[0].dtype == np.float32 for r in rows if not r.fmt)
    for r in fc.rows("any1"):  # below 33 a window class has an instantiation (psk_ctl.h: fast_kernel_has) unless the window is long
        assert r.S > 32 or r.A > (1024 if r.S <= 16 else 512), r.name
    far = fc.rows("far")
    assert [(r.S, r.props["phaseAvg"], r.far, r.kind) for r in far] == [(8, 32641, True, "drift"), (1025, 32641, True, "drift")]
    assert all(not r.far and r.props["phaseAvg"] <= 512 for v in MAIN for r in fc.rows(v))
    for r in rows:
        ki = fc.KINDS.index(r.kind)
        want = (2, 4)[(r.S + r.A + ki) % 2] if r.kind in ("drift", "before") else (2, 4, 8)[(r.S + r.A + ki) % 3]
        assert r.props["constelationSize"] == want and r.props["differentialDecoding"] == int((r.S + r.A + 2 * ki) % 5 == 0), r.name
    for v in MAIN:
        assert {r.props["constelationSize"] for r in fc.rows(v)} == {2, 4, 8}, v
        n_diff = sum(r.props["differentialDecoding"] for r in fc.rows(v))
        assert 0.1 <= n_diff / len(fc.rows(v)) <= 0.3, (v, n_diff)


def test_every_draw_is_the_pinned_one():
    """sha256 of properties, options and packet bytes per row: a row's stimulus changes only on purpose"""
    with open(GOLDEN) as f:
        pinned = {e["name"]: e for e in json.load(f)}
    rows = fc.all_rows()
    assert sorted(pinned) == sorted(r.name for r in rows)
    wrong = [r.name for r in rows if r.digest() != pinned[r.name]["sha256"] or r.draw["attempt"] != pinned[r.name]["attempt"]]
    assert not wrong, wrong


def test_shapes(refs):
    """Three calls a row from a cold start, one of them of three tiles by the restated tile rule; over a variant's rows the calls
    end in chunks of 1 and of 7 symbols, in waves of 1 and of 63, in a block of 127; calls 2 and 3 start from carried samples
    that end inside a symbol, with picks on both sides of them; numAvg reaches 1, 2 and the edges of the variant's rebuild."""
    for v in fc.VARIANTS:
        rows = fc.rows(v)
        for k in range(3):  # the tile of every launch set of every call is the one the rows were laid out for
            for front, k_min in (("any", 2), ("wide", 1)):
                mine = [r for r in rows if r.front == front and r.emit[k]]
                if mine:
                    z = -(-max(r.S for r in mine) // 1024) if front == "wide" else 1
                    K = tile_blocks(sum(-(-r.emit[k] // fc.KB) for r in mine), z, k_min, max(r.A for r in mine))
                    assert K * fc.KB == fc.TILE[front], (v, k, front, K)
        for r in rows:
            assert len(r.packets) == 3 and [p.size // 2 for p in r.packets] == r.lens, r.name
            assert fc.emitted(r.S, r.A, r.lens) == (r.emit, r.rem) and all(r.emit), r.name
            assert [c["index"].size for c in refs[r.name]] == r.emit and [c["phase"].size for c in refs[r.name]] == r.emit, r.name
            assert max(r.tiles()) >= 3 and max(r.emit) > 2 * fc.tile_symbols(r.S), r.name
            assert r.lens[0] == (r.emit[0] + r.A - 1) * r.S + r.rem[0], r.name  # a cold first call: it fills the window itself
            assert r.rem[0] and r.rem[1], r.name  # the carried samples of calls 2 and 3 end inside a symbol
            assert sum(r.lens) <= 5000 * 400, r.name
            if r.burst_call is not None:
                assert r.tiles()[r.burst_call] >= 3, r.name
    for v in MAIN:
        rows = fc.rows(v)
        n_out = np.array([n for r in rows for n in r.emit])
        assert {1, 7} <= set(n_out % 8) and {1, 63} <= set(n_out % 64) and 127 in set(n_out % 128), v
        # picks on both sides of the carried samples' end: a later call that emits more symbols than the window holds
        assert any(r.emit[k] > r.A and r.rem[k - 1] for r in rows for k in (1, 2)), v
        assert {1, 2} <= {r.A for r in rows}, v
    for S in (33, 40, 63, 64):  # <1>: the staged window (numAvg - 1 symbols) of exactly one batch of 512 // S symbols, and one more
        assert {512 // S, 512 // S + 1} <= {r.A - 1 for r in fc.rows("any1") if r.S == S}, S
    assert all(r.A > 1024 for r in fc.rows("any1") if r.S <= 16)  # the staged rebuild at its longest
    assert {0, 1, 3} <= {(r.A - 1) % 4 for r in fc.rows("any4")}
    assert {r.S for r in fc.rows("any4") if r.S <= 64} == {40} and {r.S for r in fc.rows("any16") if r.S <= 256} == {40, 100}


def test_tie_rows_tell_the_first_maximum_from_the_last(refs):
    """In every call of every tie row the first and the last maximum of the exact window sums differ in at least a quarter of
    the symbols (here: in all), and the oracle's sampleIndex is the first.  The pairs are the issue's."""
    seen = set()
    for r in fc.all_rows():
        if r.kind != "tie":
            continue
        first, last, _ = fc.exact_picks(fc.energies(r.packets, r.S), r.A)
        for k, (f, l, c) in enumerate(zip(fc.per_call(first, r.emit), fc.per_call(last, r.emit), refs[r.name])):
            assert (f != l).mean() >= 0.25, (r.name, k)
            assert np.array_equal(c["index"].astype(np.int64), f), (r.name, k)
            seen |= {(r.variant, r.S, int(a), int(b)) for a, b in set(zip(f, l))}
        assert np.asarray(r.packets[0]).astype(np.float64).max() <= 8 * fc.FORMAT_SCALE.get(r.fmt, 1), r.name
    def tied(v, S):
        return {(a, b) for vv, SS, a, b in seen if vv == v and SS == S}
    for v, S in (("any1", 64), ("any4", 65), ("any4", 256), ("any16", 1024), ("wide", 2049)):
        assert {(15, 16), (31, 32), (47, 48), (0, S - 1)} <= tied(v, S), (v, S)
    for v, S in (("any4", 65), ("any4", 128), ("any4", 255), ("any16", 257), ("any16", 1023), ("wide", 1025), ("wide", 5000)):
        assert any(b == a + 64 for a, b in tied(v, S)), (v, S)
        assert (S - 65, S - 1) in tied(v, S), (v, S)  # the last phase of a lane's last register
    assert (0, 64) in tied("any4", 65) and (0, 256) in tied("any16", 257)  # a lane's second and fifth phase
    for S in (1025, 2048, 2049, 5000):
        assert (1023, 1024) in tied("wide", S), S  # across the chunk boundary
    assert (0, 1024) in tied("wide", 1025) and (0, 2048) in tied("wide", 2049)  # the last chunk's only phase


def test_drift_rows_drift_and_the_others_do_not(refs):
    """Drift rows: the oracle's sampleIndex is the running-sum model's, and in the second half of the burst's call it differs
    from the exact pick in at least a quarter of the symbols, in at least two tiles after the first; the calls before and after
    are clean (every pick 0); the certificate fails with 4 bits to spare.  Kept rows: the oracle's picks are the exact ones in
    every call, and 24 + spread exponent + log2(numAvg + 256) stays at least 4 below 53.  Before rows: the burst is in the window
    of every symbol of call 1, whose picks are unambiguous; calls 2 and 3 are clean and exact."""
    t0 = time.perf_counter()
    n = dict(drift=0, kept=0, before=0)
    for r in fc.all_rows():
        if r.kind == "tie":
            continue
        e = fc.energies(r.packets, r.S)
        T = fc.tile_symbols(r.S)
        first, _, _ = fc.exact_picks(e, r.A)
        exact = fc.per_call(first, r.emit)
        index = [c["index"].astype(np.int64) for c in refs[r.name]]
        run = fc.running_picks(e, r.A, r.emit)
        assert all(np.array_equal(a, b) for a, b in zip(index, run)), r.name  # (the model is the oracle's arithmetic)
        clean = e[np.arange(e.shape[0]) != r.burst_symbol]
        assert clean.min() == clean.max() and 0.5 <= clean.max() < 1.0, r.name  # one energy: in exact arithmetic everything ties
        spread = np.log2(e.max() / e.min())
        rule = 24 + fc.spread_exponent(e) + fc.terms_log2(r.A)  # tile_fold's integers; it refuses above 52
        burst = np.asarray(np.concatenate(r.packets)[2 * r.burst_symbol * r.S : 2 * (r.burst_symbol + 1) * r.S], np.float64)
        assert (np.hypot(burst[0::2], burst[1::2]) ** r.props["constelationSize"] < 1e37).all(), r.name  # no refusal by overflow
        if r.kind == "kept":
            assert all(np.array_equal(a, b) for a, b in zip(index, exact)), r.name
            assert rule <= 48 and 24 + spread + np.log2(r.A + 256) <= 49 and spread > 10, (r.name, rule, spread)
            after = r.burst_symbol + 1 - sum(r.emit[:1])  # once the burst has left the window: every pick 0
            assert not index[0].any() and not index[1][after:].any() and not index[2].any(), r.name
        else:
            assert rule >= 56, (r.name, rule)
            lo, hi = np.hypot(burst[0::2], burst[1::2]).min(), np.hypot(burst[0::2], burst[1::2]).max()
            assert 2e4 * 0.999 <= lo and hi <= 2e6 * 1.001 and (hi / lo > 10 or r.S == 2), r.name  # log-uniform over two decades
        if r.kind == "before":
            assert r.burst_symbol == r.emit[0] - 1 < r.A, r.name  # in every window of call 1, gone with its last symbol
            assert all(np.array_equal(a, b) and not a.any() for a, b in zip(index[1:], exact[1:])), r.name
            assert np.array_equal(index[0], exact[0]), r.name
        if r.kind == "drift":
            k = r.burst_call
            u = r.burst_symbol - (r.A - 1) - sum(r.emit[:k])  # the output of that call with which the burst enters the window
            assert k == 1 and 0 < u < T and u + r.A <= r.emit[k] // 2, r.name  # first tile; gone before the second half
            half = np.arange(r.emit[k] // 2, r.emit[k])
            differs = index[k][half] != exact[k][half]
            assert differs.mean() >= 0.25, (r.name, differs.mean())
            assert len({int(t) for t in half[differs] // T if t >= 1}) >= 2, r.name
            assert not index[0].any() and not index[2].any() and not exact[0].any() and not exact[2].any(), r.name
            # what tiles that start from fresh sums and do not refuse would put out: the oracle's picks in the first tile, the exact
            # picks in every tile that begins once the burst has left -- not the oracle's, in a quarter of the second half at least
            fresh = fc.running_picks(e, r.A, r.emit, tile=T)[k]
            gone = -(-(u + r.A) // T) * T
            assert np.array_equal(fresh[gone:], exact[k][gone:]) and np.array_equal(fresh[:T], index[k][:T]), r.name
            assert (fresh[half] != index[k][half]).mean() >= 0.25, r.name
        n[r.kind] += 1
    assert n == dict(drift=22 + 2, kept=22, before=22), n  # (a row of each kind per samplesPerBaud and variant, and the far fit's two)
    print("conditions of %s rows with the oracle and the models: %.2f s" % (n, time.perf_counter() - t0))


# ---- rehearsal: the GPU test's comparison, fed stand-ins built from the models ------------------------------------------

def _faithful(variant):
    """results as a correct library would give them: the oracle's streams, the statistics and launch lines of section 4.8"""
    rows = fc.rows(variant)
    good = dict(channels_fast=1, channels_tiled=1, channels_guard=0, channels_sequential=0)
    refused = dict(channels_fast=0, channels_tiled=0, channels_guard=1, channels_sequential=1)
    stats = [[dict(refused if r.burst_call == k else good) for r in rows] for k in range(3)]
    traces = []
    for k in range(3):
        lines = []
        for front in ("any", "wide"):
            mine = [r.S for r in rows if r.front == front and r.emit[k]]
            names = gf.FAR_LINES[front] if variant == "far" else (gf.FRONT_LINE[front],)
            lines += [dict(what=w, S=max(mine), H=0, cnt=len(mine), slot=k % 2, stream="0x0") for w in names if mine]
        traces.append(lines)
    return rows, stats, traces


def test_rehearsal_the_comparison_reports_stand_ins_at_their_row_and_call(refs):
    """Faithful results pass.  Then, one at a time: the last maximum in place of the first on the tie rows; the picks of fresh
    sums, with the statistics of a call that was carried, on the drift rows; all four streams of the last chunk of eight
    symbols one symbol late on the <1> rows; a front launch of another body.  No kernel is built wrong for this."""
    for v in fc.VARIANTS:
        rows, stats, traces = _faithful(v)
        ref = [refs[r.name] for r in rows]
        assert gf.compare(v, rows, {c: ref[c] for c in range(len(rows))}, ref, stats, stats, traces) == {}, v

        # 1. last-maximum picks on the tie rows
        got = {c: copy.deepcopy(ref[c]) for c in range(len(rows))}
        for c, r in enumerate(rows):
            if r.kind == "tie":
                _, last, _ = fc.exact_picks(fc.energies(r.packets, r.S), r.A)
                for k, l in enumerate(fc.per_call(last, r.emit)):
                    got[c][k]["index"] = l.astype(np.int16)
        wrong = gf.compare(v, rows, got, ref, stats, stats, traces)
        assert sorted(wrong) == sorted(r.name for r in rows if r.kind == "tie"), v
        for w in wrong.values():
            assert [m.split(" sampleIndex")[0] for m in w] == ["parity: call %d" % k for k in range(3)], w

        # 2. fresh-sum picks on the drift rows, as from a tile that did not refuse
        got = {c: copy.deepcopy(ref[c]) for c in range(len(rows))}
        carried = copy.deepcopy(stats)
        for c, r in enumerate(rows):
            if r.kind == "drift":
                k = r.burst_call
                got[c][k]["index"] = fc.running_picks(fc.energies(r.packets, r.S), r.A, r.emit, tile=fc.tile_symbols(r.S))[k].astype(np.int16)
                carried[k][c] = dict(channels_fast=1, channels_tiled=1, channels_guard=0, channels_sequential=0)
        wrong = gf.compare(v, rows, got, ref, carried, stats, traces)
        assert sorted(wrong) == sorted(r.name for r in rows if r.kind == "drift"), v
        for w in wrong.values():
            assert len(w) == 2 and w[0].startswith("parity: call 1 sampleIndex") and w[1].startswith("statistics: call 1"), w
        wrong = gf.compare(v, rows, {c: ref[c] for c in range(len(rows))}, ref, stats, carried, traces)  # (the statistics alone, traced run)
        assert all(w == [m for m in w if m.startswith("statistics (traced): call 1")] and len(w) == 1 for w in wrong.values()), wrong
        assert sorted(wrong) == sorted(r.name for r in rows if r.kind == "drift"), v

    # 3. the last chunk of eight symbols, one symbol late, wherever a call of a <1> row ends in a chunk of 7
    rows, stats, traces = _faithful("any1")
    ref = [refs[r.name] for r in rows]
    got = {c: copy.deepcopy(ref[c]) for c in range(len(rows))}
    where = []
    for c, r in enumerate(rows):
        for k, n in enumerate(r.emit):
            if n % 8 == 7:
                a = n - 7
                for key in gf.KEYS:
                    per = got[c][k][key].size // n
                    seg = got[c][k][key][a * per :].reshape(7, per)
                    got[c][k][key][a * per :] = np.roll(seg, 1, axis=0).ravel()
                if any(got[c][k][key].tobytes() != ref[c][k][key].tobytes() for key in gf.KEYS):  # (seven equal symbols: nothing moved)
                    where.append((r.name, k))
    assert len(where) >= 3 and any(r.emit[k] > 2 * fc.tile_symbols(r.S) for r in rows for name, k in where if name == r.name)
    wrong = gf.compare("any1", rows, got, ref, stats, stats, traces)
    assert sorted((name, int(m.split("call ")[1].split()[0])) for name, w in wrong.items() for m in w) == sorted(where)

    # 4. the launch lines: another body's front, a missing front, a second front stage
    rows, stats, traces = _faithful("any4")
    ref = [refs[r.name] for r in rows]
    same = {c: ref[c] for c in range(len(rows))}
    for change, text in ((lambda t: t.update(S=64), "with S [64]"), (lambda t: t.update(S=1024), "with S [1024]"),
                         (lambda t: t.update(what="tile_front"), "has no 'tile_front_any'")):
        bad = copy.deepcopy(traces)
        change(bad[1][0])
        wrong = gf.compare("any4", rows, same, ref, stats, stats, bad)
        assert list(wrong) == [gf.LAUNCHES] and len(wrong[gf.LAUNCHES]) == 1 and "call 1" in wrong[gf.LAUNCHES][0] and text in wrong[gf.LAUNCHES][0], wrong
    bad = copy.deepcopy(traces)
    bad[2].append(dict(bad[2][0], what="wide_front (chunk, pick)", S=2048))
    assert "call 2 launches" in gf.compare("any4", rows, same, ref, stats, stats, bad)[gf.LAUNCHES][0]
    rows, stats, traces = _faithful("far")
    ref = [refs[r.name] for r in rows]
    bad = [[t for t in lines if not t["what"].startswith("far_fit (wide)")] for lines in traces]
    wrong = gf.compare("far", rows, {c: ref[c] for c in range(2)}, ref, stats, stats, bad)
    assert list(wrong) == [gf.LAUNCHES] and len(wrong[gf.LAUNCHES]) == 3 and all("far_fit (wide)" in m for m in wrong[gf.LAUNCHES])
