"""tests/prepass_probe.py and tests/prepass_probe_cases.py without a GPU.

First the comparator, the way tests/test_row_guards.py validates its module: a numpy stand-in for the kernel fills an arena;
a clean fill is reported clean, and each of five injected faults -- the stores a wrong pre-pass kernel would make -- is reported
at its place.  Then the inputs of tests/test_gpu_prepass_probe.py: every launch shape, piece edge and arithmetic edge those
tests are there for is asserted to be in them, against restatements of the launch functions' grid rules; nothing about the
inputs is left to chance.  The descriptors' mirrors are held to the sizeof the probe library exports."""
import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests import prepass_probe as pp
from tests import prepass_probe_cases as pc
from tests import resample_model as rm
from tests import tune_model as tm

F32 = np.float32
SUBNORMAL = 2.0 ** -126


# ---- the mirrors -------------------------------------------------------------------------------------------------------------------

def test_the_mirrors_have_the_products_sizes():
    for which, dt in enumerate(pp.MIRRORS):
        assert pp.sizeof(which) == dt.itemsize, (which, dt)
    assert pp.sizeof(len(pp.MIRRORS)) == -1
    assert pc.piece() == pl.resample_piece() and pc.piece() % 2 == 0
    assert pp.constant("gather_tile") == 64 and pp.constant("gather_min_group") == 8
    assert pp.constant("resample_inputs") == 2 * pc.piece() + 4
    C, F = tm.tables()
    assert pp.constant("tune_table_floats") == C.size + F.size


# ---- the comparator ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    """six packets: the four formats, strides 1 and 7, tuned and not, restart and histories, an odd and an even n_out, one
    packet without output"""
    rng = np.random.default_rng(11)
    spec = [(41, 5, pc.STEP_837), (64, 0, pc.ONE), (33, 77, 1 << 31), (2, pc.POS_MAX, pc.ONE), (90, 1 << 31, 1 << 33), (17, 255, pc.DRAWN_STEPS[0])]
    return pp.ResampleCase([pc._packet(rng, k, n, pos, step) for k, (n, pos, step) in enumerate(spec)])


def _written(case):
    """the arena after a stand-in kernel that writes what the descriptors ask for, and nothing else"""
    after = case.image.copy()
    for d, y, h in zip(case.desc, case.rows, case.hists):
        for off, v in ((int(d["dst"]), y), (int(d["hist_out"]), h)):
            b = np.frombuffer(np.asarray(v, F32).tobytes(), np.uint8)
            after[off : off + b.size] = b
    return after


def _one(case, after):
    found = case.check(after)
    assert len(found) == 1, pp.messages(found)
    return found[0]


def test_a_correct_writer_is_clean(small):
    assert [int(n) for n in small.desc["n_out"]] == [rm.count(p["pos"], p["rstep"], p["iq"].size // 2) for p in small.packets]
    assert small.desc["n_out"][3] == 0 and {int(n) % 2 for n in small.desc["n_out"]} == {0, 1}
    assert small.check(_written(small)) == []
    assert small.check(small.image) != [], "an arena nothing was written to is not clean"


def test_one_ulp_in_one_sample(small):
    after = _written(small)
    d = small.desc[4]
    k = int(d["n_out"]) - 2
    after[int(d["dst"]) + 8 * k] ^= 1  # (the lowest mantissa bit of the real part)
    f = _one(small, after)
    assert (f["desc"], f["where"], f["sample"], f["n_bytes"]) == (4, "row", k, 1), f
    assert f["want"] != f["got"] and int(f["want"][:2], 16) ^ int(f["got"][:2], 16) == 1 and f["want"][2:] == f["got"][2:]
    assert "descriptor 4 row" in f["message"] and "sample %d" % k in f["message"]


def test_sixteen_bytes_stored_where_eight_were_due(small):
    """the odd last output stored as a pair: its second half lands in the row's padding"""
    after = _written(small)
    i = next(i for i, d in enumerate(small.desc) if int(d["n_out"]) % 2 == 1)
    d = small.desc[i]
    last = int(d["dst"]) + 8 * (int(d["n_out"]) - 1)
    assert (last + 8) % pp.LINE != 0
    after[last + 8 : last + 16] = after[last : last + 8]
    f = _one(small, after)
    assert (f["desc"], f["where"], f["sample"], f["n_bytes"]) == (i, "padding", 0, 8), f
    assert f["want"] == "c3" * 8 and f["got"] == after[last : last + 8].tobytes().hex()


def test_a_missing_last_sample(small):
    after = _written(small)
    d = small.desc[0]
    n_out = int(d["n_out"])
    after[int(d["dst"]) + 8 * (n_out - 1) : int(d["dst"]) + 8 * n_out] = pp.ROW_BYTE
    f = _one(small, after)
    assert (f["desc"], f["where"], f["sample"], f["got"]) == (0, "row", n_out - 1, "c3" * 8), f


def test_a_history_written_to_the_slot_that_was_read(small):
    after = _written(small)
    for i in (2, 3):  # (either order of the two slots; 3 is the packet without output)
        d = small.desc[i]
        h = after[int(d["hist_out"]) : int(d["hist_out"]) + 24].copy()
        after[int(d["hist_out"]) : int(d["hist_out"]) + 24] = pp.ROW_BYTE
        after[int(d["hist_in"]) : int(d["hist_in"]) + 24] = h
    found = small.check(after)
    assert sorted((f["desc"], f["where"]) for f in found) == [(2, "hist_in"), (2, "hist_out"), (3, "hist_in"), (3, "hist_out")], pp.messages(found)
    assert small.desc[2]["hist_in"] < small.desc[2]["hist_out"] and small.desc[3]["hist_in"] > small.desc[3]["hist_out"]


def test_a_changed_source_byte(small):
    after = _written(small)
    d = small.desc[1]  # (stride 7: a byte of another column of its matrix)
    assert d["stride"] == 7
    off = int(d["src"]) + 3 * 7 * pp.SAMPLE_BYTES[int(d["format"])] + pp.SAMPLE_BYTES[int(d["format"])]
    after[off] ^= 0x10
    f = _one(small, after)
    assert (f["desc"], f["where"], f["offset"], f["n_bytes"]) == (1, "source", off, 1), f


def test_a_changed_guard_byte(small):
    after = _written(small)
    d = small.desc[5]
    cap = (int(d["n_out"]) * 8 + pp.LINE - 1) // pp.LINE * pp.LINE
    after[int(d["dst"]) + cap + 2] = 0
    f = _one(small, after)
    assert (f["desc"], f["where"], f["offset"]) == (5, "guard", int(d["dst"]) + cap + 2), f
    assert "2 byte(s) behind the padding of descriptor 5" in f["message"]
    after = _written(small)
    after[3] = 0  # (in front of everything)
    assert _one(small, after)["where"] == "guard"


# ---- resample: the launch shapes -----------------------------------------------------------------------------------------------------

def _mixes(case):
    """every format at both strides, tuned and untuned, restart and a carried history (preset and the handle's zeros)"""
    d = case.desc
    assert {(int(f), int(s)) for f, s in zip(d["format"], d["stride"])} == {(f, s) for f in pp.FORMATS for s in (1, 7)}
    assert {int(f) for f in d["flags"]} == {0, 1, 2, 3}
    kept = [p for p in case.packets if not p["restart"]]
    assert any(p["hist"] is None for p in kept) and any(p["hist"] is not None for p in kept)
    assert any(p["hist"] is not None for p in case.packets if p["restart"]), "a preset history that must not show"
    assert {int(a > b) for a, b in zip(d["hist_in"], d["hist_out"])} == {0, 1}


def _walks(case):
    P = pc.piece()
    per = pp.resample_grid(len(case.desc), case.max_n_out, P)
    return per, [pp.resample_walk(int(n), per, P) for n in case.desc["n_out"]]


def _tiny_ones(case, longs):
    d = case.desc
    tiny = [i for i in range(len(d)) if int(d["n_out"][i]) not in longs or int(d["n"][i]) <= 40]
    assert len(d) - len(tiny) == 10 or len(d) == 1, "all but ten packets are tiny"
    small = d[tiny] if len(d) > 1 else d[:0]
    if len(d) > 1:
        assert 1 <= small["n"].min() and small["n"].max() == 40 and {1, 2, 3} <= {int(n) for n in small["n"]}
        quiet = small[(small["pos"] == pc.POS_MAX) & (small["n_out"] == 0)]
        assert {int(n) for n in quiet["n"]} == {1, 2}, "packets without output whose history still moves"
        assert any(case.hists[i].tobytes() != np.zeros(6, F32).tobytes() for i in tiny if int(d["n_out"][i]) == 0)


def test_shape_one_packet():
    P = pc.piece()
    cases = [pc.resample_shape(1, v) for v in range(4)]
    assert {int(c.desc["format"][0]) for c in cases} == set(pp.FORMATS)
    assert {int(c.desc["stride"][0]) for c in cases} == {1, 7} and {int(c.desc["flags"][0]) & 2 for c in cases} == {0, 2}
    for c in cases:
        per, walks = _walks(c)
        assert c.max_n_out == 3 * P + 1 and per == 4
        assert walks[0] == ([[0], [1], [2], [3]], 3), "one workgroup per piece; the last one writes the history"


def test_shape_700_packets():
    P = pc.piece()
    c = pc.resample_shape(700)
    per, walks = _walks(c)
    assert len(c.desc) == 700 and c.max_n_out == 7 * P + 1 and per == 3
    longest = walks[int(np.argmax(c.desc["n_out"]))]
    assert longest == ([[0, 3, 6], [1, 4, 7], [2, 5]], 1), "three workgroups; two of them take three pieces, one writes the history"
    assert {w[1] for w in walks} == {0, 1, 2}, "the history's owner is each of the workgroups for some packet"
    _mixes(c)
    _tiny_ones(c, set(pc._long_outputs(P)[700][2]))


def test_shape_1100_packets():
    P = pc.piece()
    c = pc.resample_shape(1100)
    per, walks = _walks(c)
    assert len(c.desc) == 1100 and c.max_n_out == 6 * P - 1 and per == 2
    owner = {int(n): w[1] for n, w in zip(c.desc["n_out"], walks)}
    assert [owner[n] for n in (2 * P + 1, 3 * P, 4 * P + 2, 5 * P + 3, 6 * P - 1)] == [0, 0, 0, 1, 1]
    assert all(len(w[0][0]) >= 2 for n, w in zip(c.desc["n_out"], walks) if int(n) > 2 * P), "workgroup 0 loops"
    assert all(len(p) >= 2 for n, w in zip(c.desc["n_out"], walks) if int(n) > 3 * P for p in w[0]), "both workgroups loop"
    assert walks[int(np.argmax(c.desc["n_out"]))] == ([[0, 2, 4], [1, 3, 5]], 1)
    _mixes(c)
    _tiny_ones(c, set(pc._long_outputs(P)[1100][2]))


def test_shape_2100_packets():
    P = pc.piece()
    c = pc.resample_shape(2100)
    per, walks = _walks(c)
    assert len(c.desc) == 2100 and c.max_n_out == 4 * P and per == 1
    assert walks[int(np.argmax(c.desc["n_out"]))] == ([[0, 1, 2, 3]], 0), "one workgroup walks every piece, then writes the history"
    _mixes(c)
    _tiny_ones(c, set(pc._long_outputs(P)[2100][2]))


def test_the_long_packets_cover_formats_and_piece_tails():
    P = pc.piece()
    for packets in (700, 1100, 2100):
        c = pc.resample_shape(packets)
        d = c.desc[c.desc["n_out"] >= P - 1]
        assert len(d) == 10 and {int(f) for f in d["format"]} == set(pp.FORMATS) and {int(s) for s in d["stride"]} == {1, 7}
        assert {int(f) & 2 for f in d["flags"]} == {0, 2}
        assert {int(n) % 2 for n in d["n_out"]} == {0, 1}, "an odd last output (8 bytes) and an even one (16)"
        assert len({int(s) for s in d["rstep"]}) >= 5


def test_every_model_row_is_finite():
    cases = [pc.resample_shape(1, v) for v in range(4)] + [pc.resample_shape(n) for n in (700, 1100, 2100)] + [pc.resample_edges()[0]]
    cases += [pc.tune_case(n) for n in pc.TUNE_COUNTS]
    for c in cases:
        assert all(np.isfinite(y).all() for y in c.rows)
        assert all(np.isfinite(h).all() for h in getattr(c, "hists", []))
        assert all(np.isfinite(np.asarray(p["iq"], np.float64)).all() for p in c.packets)


# ---- resample: the arithmetic edges ------------------------------------------------------------------------------------------------

def _tuned(p):
    x = np.asarray(p["iq"])
    return x.astype(F32) if p["tune"] is None else tm.apply(p["tune"][0], p["tune"][1], x)


def test_edges_steps_fractions_and_positions():
    case, kinds = pc.resample_edges()
    d = case.desc
    assert pc.STEPS[:4] == (1 << 31, 1 << 32, 1 << 33, int(8.37 / 8 * 2 ** 32)) and len(pc.STEPS) > 4
    assert {(int(s), int(p) & 0xFFFFFFFF) for s, p in zip(d["rstep"], d["pos"])} >= {(s, f) for s in pc.STEPS for f in pc.FRACTIONS}
    assert {int(p) >> 32 for p in d["pos"][kinds["grid"]]} == {0, 1}
    w = rm.taps(np.array([0, 255, 256], np.uint64))
    assert [float(x[0]) for x in w] == [0.0, 1.0, 0.0, 0.0] and [float(x[1]) for x in w] == [0.0, 1.0, 0.0, 0.0], "mu is 0 below a fraction of 256"
    assert float(w[1][2]) != 1.0
    gone = d[kinds["pos_max"]]
    assert (gone["pos"] == 1 << 33).all() and {int(s) for s in gone["rstep"]} == set(pc.STEPS) and (gone["n_out"] > 100).all()


def test_edges_every_product_of_the_scaled_packets_is_subnormal():
    case, kinds = pc.resample_edges()
    assert len(kinds["tiny"]) == 4
    for i in kinds["tiny"]:
        p, d = case.packets[i], case.desc[i]
        assert d["format"] == pp.FORMAT_CF32
        s = _tuned(p).astype(np.float64).reshape(-1, 2)
        hist = np.zeros((3, 2)) if p["restart"] or p["hist"] is None else np.asarray(p["hist"], np.float64).reshape(3, 2)
        ext = np.concatenate([hist, s])
        t = int(d["pos"]) + np.arange(int(d["n_out"]), dtype=np.uint64) * np.uint64(int(d["rstep"]))
        w = rm.taps(t & np.uint64(0xFFFFFFFF))
        idx = (t >> np.uint64(32)).astype(np.int64)
        prods = np.stack([w[k].astype(np.float64)[:, None] * ext[idx + k] for k in range(4)])
        assert np.abs(prods).max() < SUBNORMAL and np.count_nonzero(prods) > 0.7 * prods.size
        if p["tune"] is not None:  # (the products of the rotation as well)
            assert np.abs(np.asarray(p["iq"], np.float64)).max() * 1.000001 < SUBNORMAL
        y = case.rows[i]
        assert np.abs(y).max() < SUBNORMAL and np.count_nonzero(y) > 0.95 * y.size, "the model keeps its denormals"
        assert np.count_nonzero(case.hists[i]) == 6
    assert {bool(case.packets[i]["tune"]) for i in kinds["tiny"]} == {False, True}


def test_edges_large_samples_and_signed_zeros():
    case, kinds = pc.resample_edges()
    for i in kinds["huge"]:
        p = case.packets[i]
        assert np.abs(p["iq"]).max() == F32(pc.HUGE * (0.5 if p["tune"] is not None else 1.0))
        assert np.isfinite(case.rows[i]).all() and np.abs(case.rows[i]).max() > 2.0 ** 124
    assert {bool(case.packets[i]["tune"]) for i in kinds["huge"]} == {False, True}
    seen = set()
    for i in kinds["zeros"]:
        p, d = case.packets[i], case.desc[i]
        assert (int(d["rstep"]), int(d["pos"]), int(d["flags"]) & 2) == (1 << 32, 0, 0)
        x = np.asarray(p["iq"], F32)
        zeros = x[x == 0]
        assert {bool(b) for b in np.signbit(zeros)} == {False, True}
        seen.add((int(d["format"]), bool((x != 0).any())))
        y = case.rows[i]
        # the stream delayed by two samples: equal as numbers; only the sign of a zero may differ (the header's sentence)
        delayed = np.concatenate([np.zeros(6, F32) if p["restart"] or p["hist"] is None else np.asarray(p["hist"], F32), x])[2 : 2 + y.size]
        assert np.array_equal(y, delayed)
        assert (np.signbit(y) != np.signbit(delayed))[y == 0].any(), "the model's zeros do change sign: the case is worth its place"
        assert np.array_equal(np.signbit(y)[y != 0], np.signbit(delayed)[y != 0])
    assert seen == {(pp.FORMAT_CF32, False), (pp.FORMAT_CF16, False), (pp.FORMAT_CF32, True), (pp.FORMAT_CF16, True)}


# ---- tune ------------------------------------------------------------------------------------------------------------------------------

def test_tune_cases_reach_the_edges_of_a_piece():
    assert pc.TUNE_COUNTS == (1, 200, 300, 2100) and pc.TUNE_LENGTHS == (1, 2, 511, 512, 513, 8191, 8192, 8193, 70001)
    want_grid = {1: (9, 8192), 200: (9, 8192), 300: (7, 10240), 2100: (1, 70144)}
    for count in pc.TUNE_COUNTS:
        c = pc.tune_case(count)
        d = c.desc
        assert len(d) == count and c.max_n == 70001 and pc.tune_grid(count, c.max_n) == want_grid[count]
        if count == 1:
            continue
        for fmt in pp.FORMATS:
            for stride in (1, 5):
                mine = {int(n) for n in d["n"][(d["format"] == fmt) & (d["stride"] == stride)]}
                assert mine >= set(pc.TUNE_LENGTHS[:-1]), (count, fmt, stride)
        assert {int(n) for n in d["n"][d["stride"] == 1]} >= {70001} and {int(n) for n in d["n"][d["stride"] == 5]} >= {70001, 20001}
        words = {(int(p), int(s)) for p, s in zip(d["phase"], d["step"])}
        assert words == set(pc.TUNE_WORDS) and {s for _, s in words} >= {0, 1, 1 << 63, (1 << 64) - 1}
        assert all(p for p, s in words if s == 0), "step 0 with a phase that is not 0"
        tiny = [i for i, p in enumerate(c.packets) if p["tiny"]]
        assert tiny and {int(d["stride"][i]) for i in tiny} == {1, 5}
        for i in tiny:
            assert np.abs(np.asarray(c.packets[i]["iq"], np.float64)).max() * 1.000001 < SUBNORMAL
            assert np.abs(c.rows[i]).max() < SUBNORMAL and np.count_nonzero(c.rows[i]) > 0.95 * c.rows[i].size


# ---- gathers ---------------------------------------------------------------------------------------------------------------------------

def test_gather_cases():
    for sb in (2, 4, 8):
        want_grid = {1: 5, 300: 5, 2100: 1}
        for count in pc.SINGLES_COUNTS:
            c = pc.singles_case(sb, count)
            assert len(c.desc) == count and c.max_n == 4097 and pc.singles_grid(count, c.max_n) == want_grid[count]
            assert c.desc["n"].min() == (1 if count > 1 else 4097) and {int(s) for s in c.desc["stride"]} == ({1, 3, 11} if count > 1 else {3})
            if count > 1:
                assert {int(n) for n in c.desc["n"]} >= set(pc.SINGLES_LENGTHS)
        w = pc.tiles_widths_case(sb)
        assert [int(g) for g in w.groups["g"]] == [8, 9, 63, 64, 65, 130] and [int(t) for t in w.groups["tiles_c"]] == [1, 1, 1, 1, 2, 3]
        for G in w.groups:
            lens = {int(n) for n in w.chans["n"][int(G["first"]) : int(G["first"]) + int(G["g"])]}
            assert lens == {1, 63, 64, 65, 200} and int(G["n_max"]) == 200
        assert w.n_tiles == (1 + 1 + 1 + 1 + 2 + 3) * 4
        m = pc.tiles_many_case(sb)
        assert len(m.groups) == 2100 and (m.groups["g"] == 8).all() and (m.chans["n"] == 10).all()
        assert m.n_tiles == 2100 > 2048, "more tiles than launch_gather_tiles gives workgroups: a second trip of tl += gridDim.x"
        assert [int(t) for t in m.groups["tile0"][:3]] == [0, 1, 2]
