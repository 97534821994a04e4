"""tests/prepass_probe.py and tests/prepass_probe_cases.py without a GPU.

First the comparator, the way tests/test_row_guards.py validates its module: a numpy stand-in for the kernel fills an arena;
a clean fill is reported clean, and each of five injected faults -- the stores a wrong pre-pass kernel would make -- is reported
at its place.  Then the inputs of tests/test_gpu_prepass_probe.py: every launch shape, piece edge and arithmetic edge those
tests are there for is asserted to be in them, against restatements of the launch functions' grid rules; nothing about the
inputs is left to chance.  The descriptors' mirrors are held to the sizeof the probe library exports.

The filter kernel (psk_fir.hip) follows in the same order at the end of the file: the mirror and the constants, the comparator on
a FirCase with eight injected faults, what the grid, the three launch shapes and the arithmetic edges reach, and fir_model.apply
held to the rounding bound of a float64 convolution.

The two looks (psk_symrate.hip, psk_acquire.hip) close the file: the mirrors of their descriptors, partials and records and the
constants; the comparator on a LookCase -- a clean numpy writer, then one ulp in one term of one block, a validity ballot over
the whole wave, a tree one level short at four and at 32 lanes a block, a written pad, a record of 400 bytes, a record at the
descriptor's index, n_pairs off by one at lag 128, a halo taken from the partner packet of the second trip, a second-trip packet
skipped, and an acquire join without the partials 64 and above --; what the width, validity, edge and 70000-descriptor cases
reach, against restatements of sr_width, the wave / sub walk of stage 1 and the grid rule; and acquire_model.device_record, the
restated order of additions, held to the exact model_record on every acquire packet of the probe.

The word search (psk_sync.hip) follows in the same order: the mirrors and the constants; sync_model.partials / join_bytes held to
model_record and model_windows on every row of every case; the comparator on a numpy stand-in for fold and join -- clean on all
nine cases, and fourteen injected faults (SYNC_FAULTS) each reported by the cases named there --; and what the cases reach: every
word length on two pieces walked both ways, second and third pieces of a workgroup, the join's second and third trip, the cap of
16 hits met in lane 0, in lane 63 and at the chunk edge, the channel loop's second trip, the shift of a short row's history."""
import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests import acquire_model as am
from tests import fir_model as fm
from tests import prepass_probe as pp
from tests import prepass_probe_cases as pc
from tests import resample_model as rm
from tests import symrate_model as sm
from tests import sync_model as ym
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


# ---- fir: the mirror, the comparator ------------------------------------------------------------------------------------------------------

def test_the_fir_mirror_and_constants():
    assert pp.MIRRORS[5] is pp.FIR and pp.FIR.itemsize == 104 == pp.sizeof(5)
    assert [pp.FIR.fields[f][1] for f in ("src", "decim", "pos", "n_taps", "pad", "n_out", "taps", "hist_in", "hist_out")] == [0, 56, 60, 64, 68, 72, 80, 88, 96]
    assert pp.constant("fir_window") == fm.WINDOW and pp.constant("fir_max_taps") == fm.MAX_TAPS
    assert 4 * pp.constant("fir_hist_slot_floats") == 1024 == pp.FIR_HIST_BYTES + 8
    for D in pc.FIR_DS:
        assert pp.fir_piece(D) == fm.piece(D) == pl.fir_piece(D) and pp.fir_piece(D) % 2 == 0
    assert (pp.fir_piece(1), pp.fir_piece(16), pp.fir_piece(0), pp.fir_piece(17)) == (3968, 248, -1, -1)
    assert [pp.fir_lanes(D)[0] for D in pc.FIR_DS] == [4] * 3 + [2] * 4 + [1] * 9
    assert [D for D in pc.FIR_DS if not pp.fir_lanes(D)[1]] == [9, 11, 13, 15], "the unpadded layout"


@pytest.fixture(scope="module")
def fir_small():
    """six packets: the four formats, strides 1 and 7, tuned and not, restart and histories, a D of each lane class and of both
    layouts, odd and even n_out, one packet without output"""
    rng = np.random.default_rng(12)
    spec = [(3, 1, 50, 10), (5, 0, 50, 7), (9, 2, 100, 128), (4, 3, 2, 5), (16, 5, 215, 2), (1, 0, 33, 1)]
    return pp.FirCase([pc._fir_packet(rng, k, D, pos, n, T) for k, (D, pos, n, T) in enumerate(spec)])


def _fir_ext(p):
    """(history in front ‖ the samples the filter sees) of a packet, float32 complex, as (127 + n, 2)"""
    s = _tuned(p)
    hist = np.zeros(2 * fm.HIST, F32) if p["restart"] or p["hist"] is None else np.asarray(p["hist"], F32)
    return np.concatenate([hist, s[: 2 * (s.size // 2)]]).reshape(-1, 2)


def test_fir_a_correct_writer_is_clean(fir_small):
    c = fir_small
    assert [int(n) for n in c.desc["n_out"]] == [17, 10, 11, 0, 14, 33]
    assert [int(n) for n in c.desc["n_out"]] == [fm.count(p["pos"], p["D"], p["iq"].size // 2) for p in c.packets]
    assert {int(f) for f in c.desc["format"]} == set(pp.FORMATS) and {int(s) for s in c.desc["stride"]} == {1, 7}
    assert {int(f) & 2 for f in c.desc["flags"]} == {0, 2} and {int(f) & 1 for f in c.desc["flags"]} == {0, 1}
    assert c.check(_written(c)) == []
    assert c.check(c.image) != [], "an arena nothing was written to is not clean"
    assert all(np.array_equal(h, _fir_ext(p)[-fm.HIST:].reshape(-1)) for h, p in zip(c.hists, c.packets))


def test_fir_one_ulp_in_one_output(fir_small):
    after = _written(fir_small)
    d = fir_small.desc[4]
    k = int(d["n_out"]) - 3
    after[int(d["dst"]) + 8 * k + 4] ^= 1  # (the lowest mantissa bit of the imaginary part)
    f = _one(fir_small, after)
    assert (f["desc"], f["where"], f["sample"], f["n_bytes"]) == (4, "row", k, 1), f
    assert "descriptor 4 row" in f["message"] and "sample %d" % k in f["message"]


def test_fir_an_output_summed_in_descending_tap_order(fir_small):
    after = _written(fir_small)
    i, m = 2, 6
    p, d = fir_small.packets[i], fir_small.desc[i]
    h, ext, T = np.asarray(p["taps"], F32), _fir_ext(p), int(d["n_taps"])
    at = p["pos"] + m * p["D"] + fm.HIST
    up = (h[0] * ext[at]).astype(F32)
    for j in range(1, T):
        up = (up + (h[j] * ext[at - j]).astype(F32)).astype(F32)
    assert up.tobytes() == fir_small.rows[i][2 * m : 2 * m + 2].tobytes(), "the ascending sum is the model's"
    down = (h[T - 1] * ext[at - (T - 1)]).astype(F32)
    for j in range(T - 2, -1, -1):
        down = (down + (h[j] * ext[at - j]).astype(F32)).astype(F32)
    assert T == 128 and down.tobytes() != up.tobytes() and np.allclose(down, up, rtol=1e-4, atol=1e-3)
    after[int(d["dst"]) + 8 * m : int(d["dst"]) + 8 * m + 8] = np.frombuffer(down.tobytes(), np.uint8)
    f = _one(fir_small, after)
    assert (f["desc"], f["where"], f["sample"]) == (i, "row", m), f
    assert f["want"] == up.tobytes().hex() and f["got"] == down.tobytes().hex()


def test_fir_the_odd_last_output_stored_as_sixteen_bytes(fir_small):
    after = _written(fir_small)
    for i in (0, 2, 5):  # (a D of each lane class)
        d = fir_small.desc[i]
        assert int(d["n_out"]) % 2 == 1
        last = int(d["dst"]) + 8 * (int(d["n_out"]) - 1)
        assert (last + 8) % pp.LINE != 0
        after[last + 8 : last + 16] = after[last : last + 8]
    found = fir_small.check(after)
    assert [(f["desc"], f["where"], f["sample"], f["n_bytes"]) for f in found] == [(i, "padding", 0, 8) for i in (0, 2, 5)], pp.messages(found)
    assert all(f["want"] == "c3" * 8 for f in found)


def test_fir_a_history_shifted_by_one_sample(fir_small):
    after = _written(fir_small)
    for i in (1, 3):  # (3 is the packet without output: two samples joined to the old history)
        d, p = fir_small.desc[i], fir_small.packets[i]
        ext = _fir_ext(p)
        off = int(d["hist_out"])
        after[off : off + pp.FIR_HIST_BYTES] = np.frombuffer(ext[-fm.HIST - 1 : -1].tobytes(), np.uint8)
    found = fir_small.check(after)
    assert [(f["desc"], f["where"]) for f in found] == [(1, "hist_out"), (3, "hist_out")], pp.messages(found)
    assert found[0]["sample"] <= 1 and found[0]["n_bytes"] > 900


def test_fir_a_history_written_to_the_slot_that_was_read(fir_small):
    after = _written(fir_small)
    H = pp.FIR_HIST_BYTES
    for i in (2, 3):  # (either order of the two slots)
        d = fir_small.desc[i]
        h = after[int(d["hist_out"]) : int(d["hist_out"]) + H].copy()
        after[int(d["hist_out"]) : int(d["hist_out"]) + H] = pp.ROW_BYTE
        after[int(d["hist_in"]) : int(d["hist_in"]) + H] = h
    found = fir_small.check(after)
    assert sorted((f["desc"], f["where"]) for f in found) == [(2, "hist_in"), (2, "hist_out"), (3, "hist_in"), (3, "hist_out")], pp.messages(found)
    assert fir_small.desc[2]["hist_in"] < fir_small.desc[2]["hist_out"] and fir_small.desc[3]["hist_in"] > fir_small.desc[3]["hist_out"]
    assert abs(int(fir_small.desc[2]["hist_in"]) - int(fir_small.desc[2]["hist_out"])) == 1024


def test_fir_a_changed_pad_byte_of_a_history_slot(fir_small):
    for i, slot in ((0, "hist_out"), (1, "hist_in")):  # (lane 127 storing a 128th sample; the same behind the slot that is read)
        after = _written(fir_small)
        off = int(fir_small.desc[i][slot]) + pp.FIR_HIST_BYTES + 3
        assert fir_small.image[off] == pp.ROW_BYTE
        after[off] = 0
        f = _one(fir_small, after)
        assert (f["desc"], f["where"], f["sample"], f["offset"], f["want"], f["got"]) == (i, "hist_pad", 3, off, "c3", "00"), f


def test_fir_a_changed_tap_and_a_changed_guard_byte(fir_small):
    after = _written(fir_small)
    d = fir_small.desc[0]
    off = int(d["taps"]) + 4 * 9
    after[off] ^= 0x01
    f = _one(fir_small, after)
    assert (f["desc"], f["where"], f["sample"], f["offset"], f["n_bytes"]) == (0, "source", 9, off, 1), f
    after = _written(fir_small)
    behind = max(int(d["hist_in"]), int(d["hist_out"])) + 1024
    after[behind + 2] = 0
    f = _one(fir_small, after)
    assert (f["desc"], f["where"], f["offset"]) == (0, "guard", behind + 2), f
    assert "2 byte(s) behind the hist_pad of descriptor 0" in f["message"]
    after = _written(fir_small)
    after[int(d["taps"]) + 4 * int(d["n_taps"])] = 0  # (the byte behind the last tap)
    assert _one(fir_small, after)["where"] == "guard"


# ---- fir: what the grid reaches -------------------------------------------------------------------------------------------------------------

def _fir_mixes(case):
    """every format at both strides, tuned (every step of TUNE_STEPS) and untuned, restart and a carried history (preset and
    the handle's zeros), either order of the two slots"""
    d = case.desc
    assert {(int(f), int(s)) for f, s in zip(d["format"], d["stride"])} == {(f, s) for f in pp.FORMATS for s in (1, 7)}
    assert {int(f) for f in d["flags"]} == {0, 1, 2, 3}
    assert {int(s) for s, f in zip(d["step"], d["flags"]) if int(f) & 2} == {s & tm.MASK for s in pc.TUNE_STEPS}
    kept = [p for p in case.packets if not p["restart"]]
    assert any(p["hist"] is None for p in kept) and any(p["hist"] is not None for p in kept)
    assert any(p["hist"] is not None for p in case.packets if p["restart"]), "a preset history that must not show"
    assert {int(a > b) for a, b in zip(d["hist_in"], d["hist_out"])} == {0, 1}


def test_fir_grid_reaches_every_decimation_tap_edge_and_tail():
    assert pc.FIR_DS == tuple(range(1, 17))
    for D in pc.FIR_DS:
        c = pc.fir_grid(D)
        d = c.desc
        P = pp.fir_piece(D)
        R, padded = pp.fir_lanes(D)
        lead = (R - 1) * D
        assert (d["decim"] == D).all() and len(d) <= 80
        # every piece has a workgroup of its own
        assert c.max_pieces == 3 and pp.fir_grid(len(d), c.max_pieces) == 3
        assert pp.fir_walk(2 * P + 1, 3, P) == ([[0], [1], [2]], 2)
        taps = sorted({int(t) for t in d["n_taps"]})
        assert taps == pc.fir_grid_taps(D) and {1, 2, 64, 127, 128} <= set(taps)
        for T in taps:
            mine = d[d["n_taps"] == T]
            assert sorted(int(n) for n in mine["n_out"]) == sorted(pc.fir_grid_outputs(D)), (D, T)
        assert set(pc.fir_grid_outputs(D)) == {1, 2, 3, 4, 5, P - 1, P, P + 1, 2 * P + 1}
        counts = {min(P, int(n) - m0) for n in d["n_out"] for m0 in range(0, int(n), P)}  # (cnt_out of every piece)
        assert counts == {1, 2, 3, 4, 5, P - 1, P} and {n % R for n in counts} == set(range(R)), "every tail of a lane's R outputs"
        assert {int(p) for p in d["pos"]} == set(range(D))
        splits = {T: pp.fir_split(D, T) for T in taps}
        assert all(s[0] == lead and s[1] == lead + 1 and s[3] == lead + T for T, s in splits.items())
        if lead > 0:
            assert {lead, lead + 1, lead + 2} <= set(taps)
            # T below, at and above head; the loop without tests [head, mid) with zero trips (T = lead, lead + 1), one, many
            assert {(T > s[1]) - (T < s[1]) for T, s in splits.items()} == {-1, 0, 1}
            assert [splits[T][2] - splits[T][1] for T in (1, lead, lead + 1, lead + 2)] == [0, 0, 0, 1]
            assert splits[128][2] - splits[128][1] == 127 - lead > 4
        else:
            assert R == 1 and lead == 0 and [splits[T][2] - splits[T][1] for T in (1, 2, 128)] == [0, 1, 127]
        assert padded == (D not in (9, 11, 13, 15))
        _fir_mixes(c)


def _fir_walks(case):
    per = pp.fir_grid(len(case.desc), case.max_pieces)
    return per, [pp.fir_walk(int(d["n_out"]), per, pp.fir_piece(int(d["decim"]))) for d in case.desc]


def _fir_long(case):
    return [i for i in range(len(case.desc)) if int(case.desc["n"][i]) > 128]


def _fir_short_ones(case):
    d = case.desc
    long_ = _fir_long(case)
    assert len(long_) == 10, "all but ten packets are short"
    short = np.delete(d, long_)
    lens = {int(n) for n in short["n"]}
    assert lens <= set(range(1, 41)) | set(pc.FIR_JOIN_LENGTHS), "1 .. 40 samples, or the join of an old history and a shorter packet"
    assert lens >= set(pc.FIR_JOIN_LENGTHS) | {3, 39, 40} and len(lens) >= 40
    assert {int(D) for D in short["decim"]} == set(pc.FIR_DS)
    quiet = [i for i in range(len(d)) if i % 50 == 10 and i not in long_]
    assert len(quiet) >= len(d) // 50 - 1
    for i in quiet:
        assert int(d["pos"][i]) >= int(d["n"][i]) and int(d["n_out"][i]) == 0 and case.pieces[i] == 0
        p = case.packets[i]
        before = np.zeros(2 * fm.HIST, F32) if p["restart"] or p["hist"] is None else np.asarray(p["hist"], F32)
        assert case.hists[i].tobytes() != before.tobytes(), "no output, and a history that still moves"
    assert {int(d["n"][i]) for i in quiet} >= {1, 2, 3}


def _fir_long_cover(case):
    d = case.desc[_fir_long(case)]
    assert [int(D) for D in d["decim"]] == list(pc.FIR_LONG_DS)
    assert {pp.fir_lanes(int(D))[0] for D in d["decim"]} == {4, 2, 1}, "a D of each lane class"
    assert {D for D in pc.FIR_LONG_DS if not pp.fir_lanes(D)[1]} == {9, 15} and {D for D in pc.FIR_LONG_DS if D >= 8 and pp.fir_lanes(D)[1]} == {8, 12, 16}
    assert {int(f) for f in d["format"]} == set(pp.FORMATS) and {int(s) for s in d["stride"]} == {1, 7}
    assert {int(f) & 2 for f in d["flags"]} == {0, 2}
    assert {int(n) % 2 for n in d["n_out"]} == {0, 1}


def test_fir_shape_700_packets():
    c = pc.fir_shape(700)
    per, walks = _fir_walks(c)
    assert len(c.desc) == 700 and c.max_pieces == 8 and per == 3
    long_ = _fir_long(c)
    P = pp.fir_piece(int(c.desc["decim"][long_[0]]))
    assert int(c.desc["n_out"][long_[0]]) == 7 * P + 1
    assert walks[long_[0]] == ([[0, 3, 6], [1, 4, 7], [2, 5]], 1), "three workgroups; two of them take three pieces, one writes the history"
    assert {walks[i][1] for i in long_} == {0, 1, 2}, "the history's owner is each of the workgroups for some packet"
    assert all(w == ([[0], [], []], 0) or w == ([[], [], []], 0) for i, w in enumerate(walks) if i not in long_)
    _fir_mixes(c)
    _fir_short_ones(c)
    _fir_long_cover(c)


def test_fir_shape_1100_packets():
    c = pc.fir_shape(1100)
    per, walks = _fir_walks(c)
    assert len(c.desc) == 1100 and c.max_pieces == 6 and per == 2
    long_ = _fir_long(c)
    assert [c.pieces[i] for i in long_] == [3, 3, 5, 6, 6, 6, 5, 3, 3, 2]
    assert [walks[i][1] for i in long_] == [0, 0, 0, 1, 1, 1, 0, 0, 0, 1], "the owner is not always the highest-numbered workgroup"
    assert walks[long_[4]] == ([[0, 2, 4], [1, 3, 5]], 1) and walks[long_[2]] == ([[0, 2, 4], [1, 3]], 0)
    _fir_mixes(c)
    _fir_short_ones(c)
    _fir_long_cover(c)


def test_fir_shape_2100_packets():
    c = pc.fir_shape(2100)
    per, walks = _fir_walks(c)
    assert len(c.desc) == 2100 and c.max_pieces == 4 and per == 1
    long_ = _fir_long(c)
    assert walks[long_[0]] == ([[0, 1, 2, 3]], 0), "one workgroup walks every piece, then writes the history"
    assert sorted({c.pieces[i] for i in long_}) == [1, 2, 3, 4]
    _fir_mixes(c)
    _fir_short_ones(c)
    _fir_long_cover(c)


def _fir_cases():
    return [pc.fir_grid(D) for D in pc.FIR_DS] + [pc.fir_shape(n) for n in pc.FIR_SHAPES] + [pc.fir_edges()[0]]


def test_fir_every_input_and_model_row_is_finite():
    for c in _fir_cases():
        assert all(np.isfinite(y).all() for y in c.rows) and all(np.isfinite(h).all() for h in c.hists)
        for p in c.packets:
            assert np.isfinite(np.asarray(p["iq"], np.float64)).all() and np.isfinite(p["taps"]).all()
            assert p["hist"] is None or np.isfinite(p["hist"]).all()
        assert c.image.size < 48 << 20


# ---- fir: the arithmetic edges ------------------------------------------------------------------------------------------------------------

def test_fir_edges_reach_each_lane_class_with_one_tap_among_the_counts():
    case, kinds = pc.fir_edges()
    d = case.desc
    assert set(kinds) == {"tiny", "subtaps", "zeros", "huge"} and 24 <= len(d) <= 48 and case.max_pieces == 1
    assert [pp.fir_lanes(D)[0] for D in pc.FIR_EDGE_DS] == [4, 2, 1]
    for kind, idx in kinds.items():
        for D in pc.FIR_EDGE_DS:
            mine = [i for i in idx if int(d["decim"][i]) == D]
            assert 1 in {int(d["n_taps"][i]) for i in mine} and len({int(d["n_taps"][i]) for i in mine}) >= 2, (kind, D)


def test_fir_edges_every_product_of_the_scaled_packets_is_subnormal():
    case, kinds = pc.fir_edges()
    for i in kinds["tiny"]:
        p, d = case.packets[i], case.desc[i]
        assert d["format"] == pp.FORMAT_CF32
        h = np.asarray(p["taps"], np.float64)
        assert (np.abs(h) >= 0.5).all() and (np.abs(h) <= 1.5).all()
        ext = _fir_ext(p).astype(np.float64)
        at = p["pos"] + np.arange(int(d["n_out"])) * p["D"] + fm.HIST
        prods = np.stack([h[j] * ext[at - j] for j in range(h.size)])
        assert np.abs(prods).max() < SUBNORMAL
        if not p["restart"]:
            assert np.count_nonzero(prods) > 0.95 * prods.size
        if p["tune"] is not None:  # (the products of the rotation as well)
            assert np.abs(np.asarray(p["iq"], np.float64)).max() * 1.000001 < SUBNORMAL
        y = case.rows[i]
        assert np.abs(y).max() < 64 * SUBNORMAL and np.count_nonzero(y) > 0.95 * y.size, "the model keeps its denormals"
        assert np.count_nonzero(case.hists[i]) > 0.95 * case.hists[i].size
    assert {bool(case.packets[i]["tune"]) for i in kinds["tiny"]} == {False, True}
    assert {bool(case.packets[i]["restart"]) for i in kinds["tiny"]} == {False, True}


def test_fir_edges_subnormal_and_zero_taps_signed_zeros_and_large_samples():
    case, kinds = pc.fir_edges()
    sub = pc.FIR_SUBNORMAL
    assert sub.view(np.uint32) == 0x11 and 0 < float(sub) < SUBNORMAL
    first = set()
    for i in kinds["subtaps"]:
        h = np.asarray(case.packets[i]["taps"], F32)
        first.add((int(case.desc["decim"][i]), int(h[:1].view(np.uint32)[0])))
        if h.size >= 5:
            assert {0x11, 0x0, 0x80000000, 0x80000011} <= {int(b) for b in h.view(np.uint32)} and (np.abs(h) > 1e-3).any()
        y = case.rows[i]
        if h.size == 1:  # (a product with the subnormal tap is subnormal; with a zero it is a zero of the product's sign)
            assert (np.count_nonzero(y) > 0.9 * y.size and np.abs(y).max() < SUBNORMAL) if h[0] != 0 else {bool(b) for b in np.signbit(y)} == {False, True}
        else:
            assert np.count_nonzero(y) > 0.9 * y.size
    assert first == {(D, b) for D in pc.FIR_EDGE_DS for b in (0x11, 0x0, 0x80000000)}, "each of them as tap 0, at every D"
    seen = set()
    for i in kinds["zeros"]:
        p, d = case.packets[i], case.desc[i]
        x = np.asarray(p["iq"], F32)
        assert (np.asarray(p["taps"]) < 0).all() and int(d["flags"]) & 2 == 0
        assert {bool(b) for b in np.signbit(x[x == 0])} == {False, True}
        seen.add((int(d["format"]), bool((x != 0).any()), int(d["n_taps"])))
        y = case.rows[i]
        assert {bool(b) for b in np.signbit(y[y == 0])} == {False, True}
        if int(d["n_taps"]) == 1:
            # h[0] * s keeps the sign of the product; an addition to +0 in the first step would lose it
            s0 = _fir_ext(p)[p["pos"] + np.arange(int(d["n_out"])) * p["D"] + fm.HIST].reshape(-1)
            assert np.array_equal(np.signbit(y), ~np.signbit(s0)) and (np.signbit(y) & (y == 0)).any()
            assert not np.signbit((F32(0.0) + y)[y == 0]).any()
    assert {s[0] for s in seen} == {pp.FORMAT_CF32, pp.FORMAT_CF16} and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == {1, 3}
    for i in kinds["huge"]:
        p, T = case.packets[i], int(case.desc["n_taps"][i])
        top = pc.HUGE / T * (0.5 if p["tune"] is not None else 1.0)
        assert np.abs(p["iq"]).max() == F32(top) and np.abs(p["taps"]).max() == 1.0
        assert np.isfinite(case.rows[i]).all() and np.abs(case.rows[i]).max() > top / 4
    assert {bool(case.packets[i]["tune"]) for i in kinds["huge"]} == {False, True}
    assert max(np.abs(case.rows[i]).max() for i in kinds["huge"]) > 2.0 ** 123


# ---- fir: a second reference -----------------------------------------------------------------------------------------------------------------

def test_fir_model_lies_within_the_rounding_bound_of_a_float64_convolution():
    """over the grid's untuned float32 packets: |y - y64| <= gamma_T * sum_j |h[j]| |s[i-j]|, gamma_T = T u / (1 - T u), u = 2^-24
    -- T products and T - 1 additions, each rounded once.  (The packets scaled by 2^-130 are not among these: underflow adds
    an absolute term.)"""
    u = 2.0 ** -24
    seen, tightest = 0, 0.0
    for D in pc.FIR_DS:
        c = pc.fir_grid(D)
        for i, p in enumerate(c.packets):
            if p["fmt"] != pp.FORMAT_CF32 or p["tune"] is not None:
                continue
            h = np.asarray(p["taps"], np.float64)
            T, n_out = h.size, int(c.desc["n_out"][i])
            ext = _fir_ext(p).astype(np.float64)
            at = p["pos"] + np.arange(n_out) * D + fm.HIST
            win = ext[at[:, None] - np.arange(T)[None, :]]  # (n_out, T, 2)
            y64 = np.einsum("j,mjq->mq", h, win)
            mag = np.einsum("j,mjq->mq", np.abs(h), np.abs(win))
            err = np.abs(c.rows[i].astype(np.float64).reshape(-1, 2) - y64)
            gamma = T * u / (1.0 - T * u)
            # (y64 itself is off by gamma_T(2^-53) * mag at the most: 2^-29 of the bound)
            assert (err <= gamma * mag * (1.0 + 2.0 ** -20)).all(), (D, i, T, float((err / np.maximum(mag, 1e-300)).max()), gamma)
            tightest = max(tightest, float((err / np.maximum(gamma * mag, 1e-300)).max()))
            seen += 1
    assert seen >= 4 * len(pc.FIR_DS) and 0.0 < tightest <= 1.0


# ---- the two looks (psk_symrate.hip, psk_acquire.hip): the mirrors, the comparator on a LookCase, what the cases reach ---------------

def test_the_look_constants_are_the_models():
    assert (pp.constant("symrate_piece"), pp.constant("symrate_halo"), pp.constant("symrate_threads")) == (sm.PIECE, sm.HALO, sm.THREADS)
    assert (pp.constant("symrate_min_s"), pp.constant("symrate_max_s"), pp.constant("symrate_max_blocks")) == (sm.MIN_S, sm.MAX_S, sm.MAX_BLOCKS)
    assert (pp.constant("acquire_piece"), pp.constant("acquire_halo"), pp.constant("acquire_threads")) == (am.PIECE, am.HALO, am.THREADS)
    assert pp.constant("acquire_piece") == pl.acquire_piece() and pp.constant("symrate_piece") == pl.symrate_piece()
    assert pp.SYMRATE_REC.itemsize == sm.RECORD_BYTES and pp.ACQUIRE_REC.itemsize == am.RECORD_BYTES
    assert pp.SYMRATE_PART.fields["pad"][1] == 324 and pp.ACQUIRE_PART.fields["pad"][1] == 172
    assert [pp.SYMRATE_REC.fields[k][1] for k in ("n_pairs", "sum_re", "sum_im", "sum_pow", "sum_lvl", "samplesPerBaud", "flags", "pad")] == [
        32, 96, 224, 352, 368, 384, 386, 387]  # (tests/test_symrate_control.py holds the binding's record to the same offsets)


def _sr_width(S):
    """sr_width of psk_symrate.h, restated: used to choose inputs, never to compute an expected byte"""
    return 1 if S <= 8 else 2 if S <= 16 else 4 if S <= 32 else 8 if S <= 64 else 16 if S <= 128 else 32 if S <= 256 else 64


def _float_packet(S, blocks, seed, bad=None):
    x = pc.sr_signal(S, blocks * S + 3, seed)
    if bad is not None:
        x[2 * (bad * S + 2)] = np.nan
    return dict(fmt=pp.FORMAT_CF32, stride=1, skew=0, tune=None, S=S, iq=x)


@pytest.fixture(scope="module")
def look_small():
    """six symrate descriptors over five packets: width 4 with two pieces, width 32, width 4 with a NaN in block 17 of 40, a
    tuned strided CS16 packet, a short one used twice -- once without data"""
    protos = [_float_packet(24, 600, 1), _float_packet(200, 40, 2), _float_packet(24, 40, 3, bad=17), _float_packet(8, 5, 4)]
    q = pc._look_mix(4, 9 * 70)
    q.update(fmt=pp.FORMAT_CS16, stride=7, S=9, iq=pc._as_format(pc.sr_signal(9, 9 * 70, 5), pp.FORMAT_CS16))
    assert q["tune"] is not None
    protos.append(q)
    return pp.LookCase("symrate", protos, [(0, True), (1, True), (3, False), (2, True), (4, True), (3, True)], spare_every=2)


def _look_written(case, over=None, skip=(), at_index=(), tail=None):
    """The arena after a stand-in for fold and join that writes what the models say.  over: {descriptor: (partials, n, S or M,
    tuned)} -- that descriptor's partials come from a wrong fold, its record is the join of them; skip: descriptors neither kernel
    reaches; at_index: descriptors whose record goes to records[c], not records[channel]; tail: (descriptor, bytes): a join that
    stores that many bytes more behind the record."""
    after = case.image.copy()
    mod = sm if case.kind == "symrate" else am
    psize, rsize = case.part_dt.itemsize, case.rec_dt.itemsize

    def put(off, b):
        after[off : off + len(b)] = np.frombuffer(b, np.uint8)

    for i, (k, data) in enumerate(case.uses):
        if i in skip:
            continue
        p = case.protos[k]
        parts, rec = p["part_bytes"], p["record"] if data else bytes(rsize)
        if over and i in over:
            wrong, n, unit, tuned = over[i]
            parts, rec = [mod.partial_bytes(q) for q in wrong], mod.join_bytes(wrong, n, unit, tuned)
        if data:
            for q, b in enumerate(parts):
                put(case.part_off + (case.part0[i] + q) * psize, b)
        put(case.rec_off + (i if i in at_index else case.channel[i]) * rsize, rec)
    if tail:  # (behind every rightful store: the join's workgroups run in no order)
        put(case.rec_off + case.channel[tail[0]] * rsize + rsize, b"\x11" * tail[1])
    return after


def _places(found):
    return sorted((f["desc"] if f["desc"] is not None else -1, f["where"]) for f in found)


def _pieces(b):
    nb = b["valid"].size
    return [sm.piece_partial(b, lo, min(lo + sm.PIECE, nb)) for lo in range(0, nb, sm.PIECE)]


def test_look_a_correct_writer_is_clean(look_small):
    c = look_small
    assert c.check(_look_written(c)) == []
    nothing = c.check(c.image)
    assert nothing and {f["where"] for f in nothing} <= {"partial", "record"}, "an arena nothing was written to is not clean"
    # the layout has what a wrong store would hit
    assert list(c.desc["channel"]) != list(range(len(c.desc))) and sorted(c.part0) != c.part0 and c.spare
    assert len(set(c.channel)) == len(c.channel) < c.n_rec and c.desc["n_piece"][0] == 2 and c.max_piece == 2
    assert not c.desc["flags"][2] & pp.LOOK_DATA and c.desc["src"][2] == 0 and c.desc["flags"][4] & pp.LOOK_TUNED
    assert c.want[c.rec_off + c.channel[2] * 392 :][:392].tobytes() == bytes(392)
    assert [_sr_width(int(S)) for S in c.desc["S"]] == [4, 32, 1, 4, 2, 1] == [sm.width(int(S)) for S in c.desc["S"]]


def test_look_one_ulp_in_one_term_of_one_block(look_small):
    c, p = look_small, look_small.protos[0]
    b = sm.block_sums(p["iq"], 24)
    term = F32(b["B"][300, 0] / 24)
    b["B"][300, 0] += float(np.spacing(term))  # (one float32 ulp of one of the block's 24 terms)
    after = _look_written(c, over={0: (_pieces(b), p["n"], 24, False)})
    found = c.check(after)
    assert _places(found) == [(0, "partial"), (0, "record")], pp.messages(found)
    part, rec = sorted(found, key=lambda f: f["where"])
    assert part["offset"] < c.part_off + (c.part0[0] + 1) * 328, "block 300 and its partners lie in piece 0"
    assert part["field"].startswith("d[") and rec["field"].startswith("sum_re") and "descriptor 0 record" in rec["message"]


def test_look_a_ballot_over_the_whole_wave(look_small):
    """validity taken from the wave's ballot without the lane group's mask: the 16 blocks that share block 17's wave go with it"""
    c, p = look_small, look_small.protos[2]
    b = sm.block_sums(p["iq"], 24)
    assert [int(m) for m in np.flatnonzero(~b["valid"])] == [17]
    G = 64 // _sr_width(24)
    lo = 17 // G * G
    b["valid"][lo : lo + G], b["B"][lo : lo + G], b["lvl"][lo : lo + G] = False, 0.0, 0.0
    found = c.check(_look_written(c, over={3: (_pieces(b), p["n"], 24, False)}))
    assert _places(found) == [(3, "partial"), (3, "record")], pp.messages(found)
    assert [f["field"] for f in found if f["where"] == "record"] == ["n_valid"]


def _short_tree(a, w):
    """the xor tree without its last level"""
    idx = np.arange(w)
    off = w >> 1
    while off >= 2:
        a = a + a[..., idx ^ off]
        off >>= 1
    return a


@pytest.mark.parametrize("i, S, W", [(0, 24, 4), (1, 200, 32)])
def test_look_a_tree_one_level_short(look_small, i, S, W):
    c, p = look_small, look_small.protos[i]
    assert _sr_width(S) == W == sm.width(S)
    b = sm.block_sums(p["iq"], S, tree=_short_tree)
    found = c.check(_look_written(c, over={i: (_pieces(b), p["n"], S, False)}))
    assert _places(found) == [(i, "partial")] * int(c.desc["n_piece"][i]) + [(i, "record")], pp.messages(found)
    assert all(f["field"].startswith(("d[", "sum_")) for f in found)


def test_look_a_written_pad_a_long_record_and_a_record_at_the_descriptors_index(look_small):
    c = look_small
    after = _look_written(c)
    o = c.part_off + (c.part0[4]) * 328 + 324
    after[o : o + 4] = 0
    f = _one(c, after)
    assert (f["desc"], f["where"], f["field"], f["n_bytes"]) == (4, "partial_pad", "pad", 4), f
    # 400 bytes stored: the eight behind the record are the next slot's
    found = c.check(_look_written(c, tail=(1, 8)))
    assert len(found) == 1 and found[0]["n_bytes"] <= 8 and found[0]["offset"] == c.rec_off + (c.channel[1] + 1) * 392, pp.messages(found)
    assert found[0]["where"] in ("record", "spare_record", "guard") and found[0]["desc"] != 1
    # records[c] in place of records[d.channel]
    assert c.channel[5] != 5
    found = c.check(_look_written(c, at_index=(5,)))
    owner = c.channel.index(5) if 5 in c.channel else None
    assert _places(found) == sorted([(5, "record"), (owner if owner is not None else -1, "record" if owner is not None else "spare_record")])
    assert next(f for f in found if f["desc"] == 5)["got"] == "c3" * 8


def test_look_n_pairs_off_by_one_at_lag_128(look_small):
    c, p = look_small, look_small.protos[0]
    parts = [(d.copy(), k.copy()) for d, k in p["parts"]]
    parts[1][1][7] += 1
    found = c.check(_look_written(c, over={0: (parts, p["n"], 24, False)}))
    assert [(f["desc"], f["where"], f["field"]) for f in found] == [(0, "partial", "c[7]"), (0, "record", "n_pairs[7]")], pp.messages(found)


# ---- the packet loop's second trip -----------------------------------------------------------------------------------------------------

def _pair_kind(case, c):
    """which of pc.LOOP_KINDS the descriptors c and c + 65535 are, from the descriptors and the packets themselves"""
    (ka, da), (kb, db) = case.uses[c], case.uses[c + pp.LOOK_GRID_MAX]
    a, b = case.protos[ka], case.protos[kb]
    clean = lambda p: not p.get("bad")  # noqa: E731
    if da and db and len(a["parts"]) == 2 and clean(a) and len(b["parts"]) == 1 and b["units"] == 3:
        return 0
    if da and db and len(b["parts"]) == 2 and clean(b) and len(a["parts"]) == 1 and a["units"] == 3:
        return 1
    if da and not db:
        return 2
    if da and db and a.get("bad") and clean(b):
        return 3
    return None


@pytest.mark.parametrize("which", ("symrate", "acquire"))
def test_look_loop_reaches_the_second_trip_with_partners_that_differ(which):
    case = pc.symrate_loop() if which == "symrate" else pc.acquire_loop()
    n = len(case.desc)
    assert n == pc.LOOP_DESCRIPTORS > pp.LOOK_GRID_MAX + 1 and pp.look_trips(n) == 2 and pp.look_trips(pp.LOOK_GRID_MAX) == 1
    assert case.max_piece == 2 and len(case.protos) <= 32 and case.arena.size <= 64 << 20
    kinds = [_pair_kind(case, c) for c in range(pc.LOOP_PAIRS)]
    assert all(k is not None for k in kinds) and {0, 1, 2, 3} == set(kinds)
    if which == "symrate":
        # the invalid-block packet's model says so, and the two-piece packet is valid throughout
        assert sm.model_record(case.protos[2]["iq"], 4)["n_valid"] == 600 - 3 and {100, 511, 599} == case.protos[2]["bad"]
        m = sm.model_record(case.protos[0]["iq"], 4, case.protos[0]["tune"])
        assert m["n_valid"] == m["n_blocks"] == 600
    else:
        assert int(case.protos[2]["parts"][0][1][8]) < am.PIECE and int(case.protos[0]["parts"][0][1][8]) == am.PIECE
    data = np.array([d for _, d in case.uses])
    assert 0.1 < 1 - data[pc.LOOP_PAIRS : pp.LOOK_GRID_MAX].mean() < 0.2, "every seventh of the rest has no data"
    assert case.check(_look_written(case)) == []


def test_look_a_halo_taken_from_the_partner_of_the_second_trip():
    """descriptor 65535 + 4 is a first piece of three blocks; its workgroup's partner on the first trip, descriptor 4, left 512
    valid blocks in LDS.  A fold that kept them as the halo pairs blocks 0 .. 2 with them."""
    case = pc.symrate_loop()
    c = 4
    assert _pair_kind(case, c) == 0
    a, b = case.protos[case.uses[c][0]], case.protos[case.uses[c + pp.LOOK_GRID_MAX][0]]
    ba, bb = (sm.model_record(p["iq"], p["S"], p["tune"])["blocks"] for p in (a, b))
    fake = {k: np.concatenate([ba[k][384:512], bb[k]]) for k in ("B", "lvl", "valid")}
    wrong = [sm.piece_partial(fake, sm.HALO, sm.HALO + 3)]
    i = c + pp.LOOK_GRID_MAX
    found = case.check(_look_written(case, over={i: (wrong, b["n"], b["S"], b["tune"] is not None)}))
    assert _places(found) == [(i, "partial"), (i, "record")], pp.messages(found)
    assert next(f for f in found if f["where"] == "record")["field"] == "n_pairs[0]"


@pytest.mark.parametrize("which", ("symrate", "acquire"))
def test_look_a_second_trip_packet_skipped(which):
    case = pc.symrate_loop() if which == "symrate" else pc.acquire_loop()
    i = pp.LOOK_GRID_MAX + 1
    assert case.uses[i][1]
    found = case.check(_look_written(case, skip=(i,)))
    assert _places(found) == [(i, "partial")] * int(case.desc["n_piece"][i]) + [(i, "record")], pp.messages(found)
    assert all(f["got"].startswith("c3c3c3c3") for f in found)


def test_look_acquire_partials_64_and_above_left_out_of_the_join():
    case = pc.acquire_lengths_case(False)
    i = len(case.desc) - 1
    p = case.protos[i]
    assert p["n"] == 65 * am.PIECE + 131 and len(p["parts"]) == 66
    after = _look_written(case)
    rec = am.join_bytes(p["parts"][:64], p["n"], p["M"], False)
    o = case.rec_off + case.channel[i] * 224
    after[o : o + 224] = np.frombuffer(rec, np.uint8)
    f = _one(case, after)
    assert (f["desc"], f["where"], f["field"]) == (i, "record", "n_valid"), f


# ---- what the look cases reach -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", pc.SR_WIDTHS)
def test_symrate_width_launch_reaches_the_edges_of_its_lane_groups(W):
    case = pc.symrate_width(W)
    G = 64 // W
    Ss = sorted({p["S"] for p in case.protos})
    assert Ss == list(pc.SR_CLASS_S[W]) and all(_sr_width(S) == W == sm.width(S) for S in Ss)
    want = {2, 3, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 255, 256, 257, 511, 512, 513, 639, 640, 641, 1025}
    want = {b for b in want if b >= 2} - ({1025} if W >= 32 else set())
    for S in Ss:
        assert {p["blocks"] for p in case.protos if p["S"] == S} == want
    assert {p["n"] - p["blocks"] * p["S"] for p in case.protos} >= {0, 3} and any(p["n"] - p["blocks"] * p["S"] == p["S"] - 1 for p in case.protos)
    assert {p["fmt"] for p in case.protos} == set(pp.FORMATS) and {p["stride"] for p in case.protos} == {1, 7}
    assert {p["tune"] is None for p in case.protos} == {False, True} and {bool(p["skew"]) for p in case.protos if p["stride"] == 1} == {False, True}
    assert {len(p["parts"]) for p in case.protos} >= {1, 2} and case.arena.size <= 64 << 20
    if W == 64:  # a ragged last turn of the widest lane group: 257 .. 1023
        assert [S for S in Ss if S % 64] == [257, 511, 1000]
    assert case.check(_look_written(case)) == []


@pytest.mark.parametrize("W", (4, 32))
def test_symrate_model_at_the_widths_nothing_had_compared_against_the_host(W):
    """symrate_model.width and _tree at the widths of two and of five tree levels, held to psk_soft_symrate_host's index order"""
    case = pc.symrate_width(W)
    for p in [q for q in case.protos if q["blocks"] in (3, 257, 641)]:
        m = sm.model_record(p["iq"], p["S"], p["tune"])
        assert sm.record_bytes(m) == p["record"]
        sm.assert_close(pl.symrate_host(p["S"], np.asarray(p["iq"], F32), p["tune"]), m, "S %d, %d blocks" % (p["S"], p["blocks"]))


@pytest.mark.parametrize("W", pc.SR_WIDTHS)
def test_symrate_validity_cases_invalidate_the_blocks_the_definition_says(W):
    case = pc.symrate_validity(W)
    S, G = pc.SR_VALIDITY_S[W], 64 // W
    assert _sr_width(S) == W and (W == 1 or S % W), "the last turn is ragged"
    seen = set()
    for p in case.protos:
        nb, b, pos = p["spot"]
        m = sm.model_record(p["iq"], S, p["tune"])
        bad = {b, b + 1} if pos == S - 1 and b + 1 < nb else {b}
        # (the definition: a block with a non-finite sample, and the one whose first g reaches back to it; every other block --
        # the neighbours of the same wave among them -- stays valid)
        assert set(np.flatnonzero(~m["blocks"]["valid"])) == bad == p["bad"], p["spot"]
        assert m["n_valid"] == nb - len(bad) and sm.record_bytes(m) == p["record"]
        turn, sub = pc.sr_wave_slot(b, G)
        seen |= {("sub", sub == 0, sub == G - 1), ("pos", pos)}
        if b == nb - 1 and sub < G - 1:
            seen.add("last block, the rest of its wave not live")
        if pos >= (S - 1) // W * W and S % W:
            seen.add("ragged turn")
    assert {("pos", q) for q in {0, W - 1, min(W, S - 1), S - 1}} <= seen
    assert ("sub", True, G == 1) in seen and ("sub", G == 1, True) in seen
    assert G == 1 or "last block, the rest of its wave not live" in seen
    assert W == 1 or "ragged turn" in seen
    spots = {p["spot"] for p in case.protos}
    assert (642, 511, S - 1) in spots and (642, 383, S - 1) in spots and {p["blocks"] for p in case.protos} == {40, 41, 642}
    assert case.check(_look_written(case)) == []


def test_symrate_edges_reach_subnormals_overflow_and_signed_zeros():
    case, kinds = pc.symrate_edges()
    assert set(kinds) == {"tiny", "huge", "zeros"} and {_sr_width(p["S"]) for p in case.protos} == {1, 4, 32, 64}
    for k in kinds["tiny"]:
        p = case.protos[k]
        x = np.asarray(p["iq"], F32)
        assert 0 < np.abs(x).max() < SUBNORMAL
        m = sm.model_record(p["iq"], p["S"], p["tune"])
        assert m["n_valid"] == m["n_blocks"] and m["sum_lvl"] == [0.0, 0.0], "every e underflows to zero: valid blocks, zero sums"
    for k in kinds["huge"]:
        p = case.protos[k]
        m = sm.model_record(p["iq"], p["S"], p["tune"])
        assert m["n_valid"] == 0 and not any(m["n_pairs"]) and p["record"][96:384] == bytes(288)
    for k in kinds["zeros"]:
        p = case.protos[k]
        assert np.signbit(np.asarray(p["iq"], F32)[np.asarray(p["iq"], F32) == 0]).any()
        assert sm.model_record(p["iq"], p["S"], p["tune"])["n_valid"] == p["units"]
    assert case.check(_look_written(case)) == []


@pytest.mark.parametrize("mixed", (False, True))
def test_acquire_cases_reach_every_length_format_and_placement_and_the_restated_order_is_the_exact_one(mixed):
    case = pc.acquire_lengths_case(mixed)
    P, lens = am.PIECE, pc.acquire_lengths()
    assert lens[-3:] == (64 * P, 64 * P + 1, 65 * P + 131) and {p["n"] for p in case.protos} == set(lens)
    assert {(p["fmt"], p["place"]) for p in case.protos} == {(f, q) for f in pp.FORMATS for q in pc.PLACEMENTS}
    assert {(p["fmt"], p["place"]) for p in case.protos if p["n"] > 64 * P - 1} >= {(pp.FORMAT_CF32, "aligned"), (pp.FORMAT_CS8, "strided")}
    assert {p["M"] for p in case.protos if p["n"] >= 64 * P} == {2, 4, 8} == {p["M"] for p in case.protos if p["n"] < 64 * P}
    assert set().union(*(p["marks"] for p in case.protos)) == {"nonfinite", "zeros", "underflow"}
    assert {p["tune"] is not None for p in case.protos} == ({False, True} if mixed else {False}) and case.tables == mixed
    assert max(len(p["parts"]) for p in case.protos) == 66 == case.max_piece
    for i, d in enumerate(case.desc):  # aligned: one load takes a pair; skewed: the pair's size does not divide the address
        p = case.protos[i]
        pair = 2 * pp.SAMPLE_BYTES[p["fmt"]]
        assert (int(d["src"]) % pair == 0) == (p["place"] != "skewed") or p["place"] == "strided", (i, p["place"])
    for p in case.protos:
        r = pl.Acquire.from_buffer_copy(p["record"])
        m = am.model_record(p["iq"], p["M"], p["tune"])
        am.assert_record(r, m, "n %d M %d" % (p["n"], p["M"]))
        assert p["record"] == am.device_record(p["iq"], p["M"], p["tune"])
        if "underflow" in p["marks"] or "nonfinite" in p["marks"]:
            assert m["n_valid"] < p["n"]
    assert case.check(_look_written(case)) == []


def test_acquire_loop_packets_the_restated_order_is_the_exact_one():
    for p in pc.acquire_loop().protos:
        am.assert_record(pl.Acquire.from_buffer_copy(p["record"]), am.model_record(p["iq"], p["M"], p["tune"]), "n %d M %d" % (p["n"], p["M"]))


def test_the_bound_of_a_long_acquire_packet_is_wider_than_one_float32_rounding():
    """why the long packets are held byte for byte: at 65 P + 131 samples assert_record's bound passes a term off by a float32 ulp"""
    p = pc.acquire_lengths_case(False).protos[-1]
    exact, bound = am.model_record(p["iq"], p["M"])["sums"]["sum_re"][0]
    assert bound > 2.0 ** -24 and p["n"] == 65 * am.PIECE + 131


# ---- the word search (psk_sync.hip): the mirrors, the models, the comparator on a SyncCase, what the cases reach ----------------------

SP = ym.PIECE
PART, REC = ym.PART_BYTES, ym.RECORD_BYTES


def test_the_sync_mirrors_and_constants_are_the_models():
    assert [pp.sizeof(k) for k in (12, 13, 14)] == [pp.SYNC_DESC.itemsize, PART, REC] == [80, 416, 456]
    assert (pp.constant("sync_piece"), pp.constant("sync_threads"), pp.constant("sync_hist")) == (ym.PIECE, ym.THREADS, ym.HIST)
    assert (pp.constant("sync_hist_slot_floats"), pp.constant("sync_max_word"), pp.constant("sync_hits")) == (256, ym.MAX_WORD, ym.HITS)
    assert 4 * pp.constant("sync_hist_slot_floats") == pp.SYNC_SLOT_BYTES == pp.SYNC_HIST_BYTES + 8 and pl.sync_piece() == ym.PIECE
    assert [ym.PART_DTYPE.fields[k][1] for k in ("n_valid", "n_hits", "best", "hits")] == [0, 4, 8, 32]
    assert [pp.SYNC_DESC.fields[k][1] for k in ("soft", "word", "hist_in", "hist_out", "n", "p0", "n_windows", "part0", "n_piece", "channel",
                                                "L", "flags", "threshold", "Ew")] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72, 76]
    # sync_grid restates front_grid_y: 2048 workgroups spread over the descriptors, no more than the longest row has pieces
    assert [pp.sync_grid(n, 7) for n in (1, 256, 292, 293, 682, 683, 700, 1024, 1100, 2048, 2049, 2100, 66135)] == [7, 7, 7, 7, 4, 3, 3, 2, 2, 1, 1, 1, 1]
    assert pp.sync_grid(1, 1 << 20) == 2048 and pp.sync_walk(7, 3) == [[0, 3, 6], [1, 4], [2, 5]] and pp.sync_walk(1, 3) == [[0], [], []]


def _flags(p):
    return ym.RESTART if p["restart"] else 0


SYNC_MODELLED = ("lengths", "walk 700", "chunks", "loop", "short rows")  # (the other cases are made of the same rows)


@pytest.mark.parametrize("name", SYNC_MODELLED)
def test_sync_the_partials_of_every_row_join_to_the_models_record(name):
    """partials is not its own judge: join_bytes of the partials of every row of every case is model_record's record, the
    history model_windows'; the chunked join below -- the device's trips of 64 -- agrees with both"""
    case = pc.SYNC_CASES[name]()
    for k, p in enumerate(case.protos):
        rec, hist = ym.model_record(p["word"], p["thr"], p["x"], _flags(p), p["hist"])
        assert p["record"] == rec.tobytes(), (name, k)
        assert p["hist_out"].tobytes() == hist.tobytes() == ym.model_windows(p["word"], p["x"], _flags(p), p["hist"])[-1].tobytes(), (name, k)
        assert _sync_join(p["parts"], p["n"], p["n_windows"], p["L"]) == p["record"], (name, k)
        assert int(rec["n_windows"]) == p["n_windows"] and len(p["parts"]) == max(1, -(-p["n_windows"] // SP))
        for q in p["parts"]:
            assert q["n_hits"] <= q["n_valid"] <= SP and len(q["hits"]) == min(q["n_hits"], ym.HITS) and (q["best"] is None) == (q["n_valid"] == 0)


# ---- a numpy stand-in for the two kernels, and the faults a wrong kernel would make --------------------------------------------------

def _sync_join(parts, n, n_windows, L, fault=None):
    """the record as psk_sync_join_kernel makes it: trips of 64 partials, `before` = the hits of the trips before plus a scan
    of this one, the best of a trip merged into the best so far.  fault: what a wrong join would do."""
    rec = np.zeros((), ym.RECORD_DTYPE)
    rec["n_symbols"], rec["n_windows"], rec["word_len"], rec["flags"] = n, n_windows, L, ym.DATA
    nv = nh = 0
    best, seventeenth = None, None
    later = fault == "best_later_pieces"
    for base in range(0, len(parts), pp.JOIN_CHUNK):
        chunk = parts[base: base + pp.JOIN_CHUNK]
        before = 0 if fault == "before_drops_nh" else nh
        mine = None
        for q in chunk:
            ph = int(q["n_hits"])
            if ph and before < ym.HITS:
                take = min(ph, ym.HITS - before)
                rec["hits"][before: before + take] = q["hits"][:take]
            elif ph and before == ym.HITS and seventeenth is None:
                seventeenth = q["hits"][0]
            if ph > ym.HITS - before >= 0 and seventeenth is None and len(q["hits"]) > ym.HITS - before:
                seventeenth = q["hits"][ym.HITS - before]
            before += ph
            if q["n_valid"] and (mine is None or q["best"]["m"] > mine["m"] or (later and q["best"]["m"] == mine["m"])):
                mine = q["best"]
            nv, nh = nv + int(q["n_valid"]), nh + ph
        if mine is not None and (best is None or mine["m"] > best["m"] or (fault in ("best_later_pieces", "best_later_chunks") and mine["m"] == best["m"])):
            best = mine
    rec["n_valid"], rec["n_hits"] = nv, nh
    if best is not None:
        rec["best"] = best
    out = bytearray(rec.tobytes())
    if fault == "hit17_join" and seventeenth is not None:
        at = ym.RECORD_DTYPE.fields["hits"][1] + ym.HITS * ym.HIT_BYTES
        out[at:] = seventeenth.tobytes()[: REC - at]  # (hits[16]: it lies on word_len, flags and the pad)
    return bytes(out)


SYNC_FAULTS = {
    "walk_stops": ("walk 2100", "lengths spread"),     # a walk that stops after gridDim.x pieces
    "stale_hits": ("walk 700", "walk 2100"),           # a second piece's hits taken from the first piece's list
    "before_drops_nh": ("chunks", "join alone"),       # nh of the earlier chunks dropped from `before`
    "hit17_fold": ("walk 1100",),                      # a 17th hit stored by the fold
    "hit17_join": ("join alone", "chunks"),            # ... and by the join
    "best_later_pieces": ("walk 700",),                # the later of two equal bests kept, across pieces
    "best_later_chunks": ("chunks", "join alone"),     # ... and across chunks only
    "best_no_valid": ("walk 1100", "short rows"),      # best written for a piece with no valid window
    "hit_past": ("short rows", "lengths"),             # hits[min(n_hits, 16)] written
    "hist_1024": ("short rows",),                      # 1024 bytes of history written
    "hist_read_restart": ("short rows",),              # hist_in read under restart
    "spare_record": ("lengths",),                      # a record written for a spare channel
    "no_zero_record": ("loop", "lengths spread"),      # no zero record for a descriptor without data
    "next_part0": ("walk 700", "loop"),                # a partial written through the next descriptor's part0
}


def _sync_written(case, fault=None):
    """The arena after a stand-in for fold and join that stores what the models say and nothing else -- the partials through
    partial_writes, piece by piece as the workgroups walk them; the record by _sync_join --, or with one fault."""
    after = case.image.copy()
    late = []  # stores that no rightful store may cover: the workgroups run in no order

    def put(off, b):
        after[off: off + len(b)] = np.frombuffer(bytes(b), np.uint8)

    nxt = dict(zip(case.searched, case.searched[1:]))
    for i, (k, data) in enumerate(case.uses):
        p = case.protos[k]
        rec_at = case.rec_off + case.channel[i] * REC
        if not data:
            if case.which & 2 and fault != "no_zero_record":
                put(rec_at, bytes(REC))
            continue
        parts = list(p["parts"])
        if case.which & 1:
            owner = [y for y, walk in enumerate(pp.sync_walk(len(parts), case.per)) for _ in walk]
            assert sorted(q for walk in pp.sync_walk(len(parts), case.per) for q in walk) == list(range(len(parts))) and len(owner) == len(parts)
            if fault == "walk_stops":
                parts = [q if j < case.per else None for j, q in enumerate(parts)]
            if fault == "stale_hits":
                for j in range(case.per, len(parts)):
                    prev, own = p["parts"][j - case.per]["hits"], parts[j]["hits"].copy()
                    own[: min(len(prev), len(own))] = prev[: min(len(prev), len(own))]
                    parts[j] = dict(parts[j], hits=own)
            base = case.part0[nxt[i]] if fault == "next_part0" and i in nxt else case.part0[i]
            for j, q in enumerate(parts):
                if q is None:
                    continue
                o = case.part_off + (base + j) * PART
                for off, b in ym.partial_writes(q):
                    put(o + off, b)
                kept = min(int(q["n_hits"]), ym.HITS)
                if fault == "best_no_valid" and not q["n_valid"]:
                    put(o + 8, bytes(ym.HIT_BYTES))
                if fault == "hit_past" and kept < ym.HITS:
                    put(o + 32 + ym.HIT_BYTES * kept, bytes(ym.HIT_BYTES))
                if fault == "hit17_fold" and q["n_hits"] > ym.HITS:
                    late.append((o + PART, q["hits"][ym.HITS - 1].tobytes()))
            h = p["hist_out"]
            if fault == "hist_read_restart" and p["restart"]:
                h = np.concatenate([np.frombuffer(pp.nan_poison(pp.SYNC_HIST_BYTES).tobytes(), F32), p["x"]])[-2 * ym.HIST:]
            put(int(case.desc["hist_out"][i]), h.tobytes() + (bytes(8) if fault == "hist_1024" else b""))
        if case.which & 2:
            put(rec_at, _sync_join([q for q in parts if q is not None], p["n"], p["n_windows"], p["L"], fault))
    if fault == "spare_record":
        put(case.rec_off + case.spare_channels[len(case.spare_channels) // 2] * REC, bytes(REC))
    for off, b in late:
        put(off, b)
    return after


@pytest.mark.parametrize("name", sorted(pc.SYNC_CASES))
def test_sync_a_correct_writer_is_clean_on_every_case(name):
    case = pc.SYNC_CASES[name]()
    found = case.check(_sync_written(case))
    assert found == [], pp.messages(found)
    nothing = case.check(case.image)
    assert nothing and {f["where"] for f in nothing} <= {"partial", "record", "hist_out"}, "an arena nothing was written to is not clean"
    # the layout has what a wrong store would hit
    assert case.spare and case.spare_channels and list(case.desc["channel"]) != list(range(len(case.desc)))
    assert [case.part0[i] for i in case.searched] != sorted(case.part0[i] for i in case.searched) or len(case.searched) < 3


@pytest.mark.parametrize("fault", sorted(SYNC_FAULTS))
def test_sync_every_fault_is_reported_by_its_cases(fault):
    for name in SYNC_FAULTS[fault]:
        case = pc.SYNC_CASES[name]()
        found = case.check(_sync_written(case, fault))
        assert found, "%s goes unseen by %s" % (fault, name)
        where = {f["where"] for f in found}
        if fault in ("before_drops_nh", "hit17_join", "best_later_pieces", "best_later_chunks"):
            assert where == {"record"}, pp.messages(found)
            want = {"before_drops_nh": ("hits",), "hit17_join": ("word_len",), "best_later_pieces": ("best",), "best_later_chunks": ("best",)}[fault]
            assert all(f["field"].startswith(want) for f in found), pp.messages(found)
        elif fault in ("hist_1024",):
            assert where == {"hist_pad"}, pp.messages(found)
        elif fault in ("hist_read_restart",):
            assert where == {"hist_out"}, pp.messages(found)
        elif fault == "spare_record":
            assert where == {"spare_record"} and len(found) == 1, pp.messages(found)
        elif fault == "no_zero_record":
            assert where == {"record"} and all(f["got"] == "c3" * 8 for f in found), pp.messages(found)
        elif fault in ("best_no_valid", "hit_past"):
            assert where == {"partial"} and all(f["field"].startswith(("best", "hits")) for f in found), pp.messages(found)


def test_sync_the_faults_across_chunks_need_rows_of_more_than_64_pieces():
    """what the suite's rows of at most four pieces could not show: each of these goes unseen by the walk cases"""
    case = pc.SYNC_CASES["walk 700"]()
    for fault in ("before_drops_nh", "best_later_chunks"):
        assert case.check(_sync_written(case, fault)) == [], fault


# ---- what the sync cases reach -----------------------------------------------------------------------------------------------------------

def _piece_of(p, pos):
    return (int(pos) - p["p0"]) // SP


def test_sync_lengths_reach_every_word_length_on_two_pieces_walked_both_ways():
    one, two = pc.SYNC_CASES["lengths"](), pc.SYNC_CASES["lengths spread"]()
    assert (len(one.desc), one.per, one.max_piece) == (256, 2, 2) and (len(two.desc), two.per, two.max_piece) == (256 + 1900, 1, 2)
    assert pp.sync_walk(2, 2) == [[0], [1]] and pp.sync_walk(2, 1) == [[0, 1]]
    assert sorted((p["L"], p["restart"]) for p in one.protos) == [(L, r) for L in range(1, 129) for r in (False, True)]
    for p in one.protos:
        L = p["L"]
        assert p["n_windows"] == SP + 65 and len(p["parts"]) == 2 and p["n"] == SP + 65 + (L - 1 if p["restart"] else 0)
        # the second piece: one full turn of wave 0 and one lane of its second
        assert p["n_windows"] - SP == 64 + 1 and p["parts"][1]["n_valid"] == 65
        hits = [int(h) for h in np.frombuffer(p["record"], ym.RECORD_DTYPE)[0]["hits"]["pos"][: min(16, sum(q["n_hits"] for q in p["parts"]))]]
        if not p["restart"] and L >= 2:
            assert -(L // 2) in hits, "L %d: the word across the row's start is found through hist_in" % L
        assert all(q["n_hits"] >= 1 for q in p["parts"]), L
    # the same rows, the same expected bytes
    for k, i in enumerate(two.searched):
        assert two.uses[i] == (k, True) and two.record_bytes(two.want, i) == one.record_bytes(one.want, k)
        assert [two.partial_bytes(two.want, i, q) for q in (0, 1)] == [one.partial_bytes(one.want, k, q) for q in (0, 1)]
    assert sum(1 for _, data in two.uses if not data) == 1900


def test_sync_walk_cases_reach_second_and_third_pieces_of_a_workgroup():
    cases = {n: pc.sync_walk(n) for n in pc.SYNC_WALK_SHAPES}
    assert [cases[n].per for n in pc.SYNC_WALK_SHAPES] == [3, 2, 1] and all(c.max_piece == 7 for c in cases.values())
    pr = cases[700].protos
    assert [len(p["parts"]) for p in pr] == [7, 5, 4, 3, 2, 4, 1, 2, 1, 1, 3, 5]
    assert {(p["L"], p["restart"]) for p in pr} == {(2, True), (2, False), (31, True), (31, False), (128, True), (128, False)}
    walks = pp.sync_walk(7, 3)
    assert max(len(w) for w in walks) == 3 and len({len(w) for w in walks}) == 2, "three pieces for one workgroup, and a ragged walk"
    assert pp.sync_walk(1, 3)[1:] == [[], []] and pp.sync_walk(2, 3)[2] == [], "blockIdx.x >= n_piece beside a channel of seven"
    for n, c in cases.items():
        used = {k for k, data in c.uses if data}
        assert used == set(range(12)) and sum(1 for _, data in c.uses if not data) > n // 10
        near = [(len(c.protos[c.uses[i][0]]["parts"]), len(c.protos[c.uses[i + 1][0]]["parts"])) for i in range(n - 1) if c.uses[i][1] and c.uses[i + 1][1]]
        assert {(7, 1), (1, 7)} & set(near) or {(7, 2), (2, 7)} & set(near)
    # hits in every piece
    assert all(q["n_hits"] >= 3 for q in pr[0]["parts"]) and all(q["n_hits"] >= 1 for q in pr[5]["parts"])
    # more than 16 hits in a piece that is not its workgroup's first, at every shape, hits of the piece before under them, and
    # fewer hits in the piece the workgroup takes next
    cp, _, cn = pc.SYNC_WALK_CROWD
    assert pr[0]["parts"][cp]["n_hits"] == cn + 3 > ym.HITS
    for per in (3, 2, 1):
        assert cp >= per and pr[0]["parts"][cp - per]["n_hits"] == 3 and pr[0]["parts"][cp + per]["n_hits"] == 3
    assert [q["n_hits"] for q in pr[10]["parts"]] == [2, 18, 18]
    # a piece without a valid window between two with
    z = pr[1]["parts"]
    assert z[pc.SYNC_WALK_ZEROS]["n_valid"] == 0 and z[pc.SYNC_WALK_ZEROS]["best"] is None and z[1]["n_valid"] == SP and z[3]["n_valid"] == SP
    assert np.frombuffer(pr[1]["record"], ym.RECORD_DTYPE)[0]["hits"]["pos"][0] == -1
    # equal bests in the four pieces of the periodic row: pieces 0 and 3 share a workgroup of three, 0 and 1 do not
    bests = [q["best"] for q in pr[2]["parts"]]
    assert len({b.tobytes()[8:] for b in bests}) == 1 and [int(b["pos"]) for b in bests] == [int(bests[0]["pos"]) + SP * k for k in range(4)]
    assert np.frombuffer(pr[2]["record"], ym.RECORD_DTYPE)[0]["best"]["pos"] == bests[0]["pos"]
    assert 0 in walks[0] and 3 in walks[0] and 1 in walks[1]
    # the NaN at the piece edge takes the windows that meet it, on both sides
    assert pr[11]["parts"][1]["n_valid"] == SP - 30 and pr[11]["parts"][2]["n_valid"] == SP - 1


def test_sync_chunk_cases_reach_the_joins_second_and_third_trip():
    case = pc.SYNC_CASES["chunks"]()
    pr = case.protos
    assert tuple(len(p["parts"]) for p in pr) == pc.SYNC_CHUNK_PIECES and case.per == 130 and pr[7]["n_windows"] % SP != 0
    assert [(p["L"], p["restart"]) for p in pr[:8]] == [(2, r) for r in (True, False, True, False, True, False, True, False)]
    rec = [np.frombuffer(p["record"], ym.RECORD_DTYPE)[0] for p in pr]
    chunk_hits = lambda p, c: sum(q["n_hits"] for q in p["parts"][64 * c: 64 * c + 64])  # noqa: E731
    # 2: the cap is met in lane 63 of the first trip; 3: the 16th stored hit lies in the second
    assert (chunk_hits(pr[2], 0), rec[2]["n_hits"]) == (20, 20) and _piece_of(pr[2], rec[2]["hits"]["pos"][15]) == 63
    assert (chunk_hits(pr[3], 0), chunk_hits(pr[3], 1), rec[3]["n_hits"]) == (10, 10, 20) and _piece_of(pr[3], rec[3]["hits"]["pos"][15]) == 64
    assert _piece_of(pr[3], rec[3]["hits"]["pos"][9]) < 64 <= _piece_of(pr[3], rec[3]["hits"]["pos"][10])
    # 4: hits in the second chunk only
    assert (chunk_hits(pr[4], 0), chunk_hits(pr[4], 1), rec[4]["n_hits"]) == (0, 4, 4) and _piece_of(pr[4], rec[4]["hits"]["pos"][0]) == 64
    # 5: 20 hits in one piece of chunk 0, then three in chunk 1: counted, none stored
    assert pr[5]["parts"][5]["n_hits"] == 20 and chunk_hits(pr[5], 1) == 3 and rec[5]["n_hits"] == 23
    assert {_piece_of(pr[5], x) for x in rec[5]["hits"]["pos"]} == {5}
    # 6: the cap met in the third trip; 7: ten either side of piece 64, 130 pieces
    assert [chunk_hits(pr[6], c) for c in range(3)] == [5, 5, 10] and _piece_of(pr[6], rec[6]["hits"]["pos"][15]) == 128
    assert [chunk_hits(pr[7], c) for c in range(3)] == [10, 8, 2] and rec[7]["n_hits"] == 20
    # 8: the best of the second chunk is strictly greater than every best before it
    b = [q["best"]["m"] for q in pr[8]["parts"]]
    assert pr[8]["L"] == 31 and _piece_of(pr[8], rec[8]["best"]["pos"]) == 64 and b[64] > max(b[:64]) and b[64] > max(b[65:])
    assert rec[8]["n_valid"] == pr[8]["n_windows"] == 65 * SP + 40
    # 9: equal bests in chunk 0 and chunk 1: the first
    b = pr[9]["parts"]
    assert b[10]["best"].tobytes()[8:] == b[65]["best"].tobytes()[8:] and _piece_of(pr[9], rec[9]["best"]["pos"]) == 10
    assert all(q["best"]["m"] < b[10]["best"]["m"] for j, q in enumerate(b) if j not in (10, 65))
    # the totals of a trip fit 32 bits, the counts are 64-bit sums of them
    assert all(int(r["n_valid"]) == sum(q["n_valid"] for q in p["parts"]) for r, p in zip(rec, pr)) and int(rec[7]["n_valid"]) > 64 * SP


def test_sync_join_alone_reaches_the_cap_in_lane_0_lane_63_and_at_the_chunk_edge():
    case = pc.SYNC_CASES["join alone"]()
    assert case.which == 2 and [len(p["parts"]) for p in case.protos[:4]] == [1, 64, 65, 200]
    by = {p["name"]: p for p in case.protos}
    rec = {k: np.frombuffer(p["record"], ym.RECORD_DTYPE)[0] for k, p in by.items()}
    assert int(rec["full 200"]["n_valid"]) == int(rec["full 200"]["n_hits"]) == 204800
    assert rec["full 200"]["hits"].tobytes() == by["full 200"]["parts"][0]["hits"].tobytes()

    def met(p):
        """(the piece in which the 16th hit lies, the hits in front of that piece)"""
        total = 0
        for j, c in enumerate(p["counts"]):
            if total + c >= ym.HITS:
                return j, total
            total += c

    assert met(by["lane 0"]) == (0, 0) and met(by["lane 63"]) == (63, 0) and met(by["chunk edge"]) == (64, 15) and met(by["second chunk"]) == (64, 0)
    assert met(by["cycle"]) == (2, 1)
    for name in ("cycle", "lane 0", "lane 63", "chunk edge", "second chunk"):
        p = by[name]
        assert len(p["parts"]) == 130 and set(p["counts"]) == set(pc.SYNC_HIT_COUNTS), name
        assert any(q["n_valid"] == 0 for q in p["parts"]) and len({float(q["best"]["m"]) for q in p["parts"] if q["n_valid"]}) == 11
    # the best of several equal maxima, in chunk 0 and in chunk 1, is the first
    top = [j for j, q in enumerate(by["full 200"]["parts"]) if q["best"]["m"] == rec["full 200"]["best"]["m"]]
    assert top[0] < 64 <= top[-1] and int(rec["full 200"]["best"]["pos"]) == top[0] * SP + 517
    # NaN poison in every member partial_writes does not list
    poison = pp.nan_poison(ym.HIT_BYTES).tobytes()
    for i in case.searched:
        for j, q in enumerate(case.protos[case.uses[i][0]]["parts"]):
            b = case.partial_bytes(case.image, i, j)
            kept = min(q["n_hits"], ym.HITS)
            assert b[32 + 24 * kept:] == poison * (ym.HITS - kept) and (b[8:32] == poison) == (q["n_valid"] == 0)
            assert b[32: 32 + 24 * kept] == q["hits"].tobytes()


def test_sync_loop_reaches_the_second_trip_with_partners_that_differ():
    case = pc.SYNC_CASES["loop"]()
    n = len(case.desc)
    assert n == pc.SYNC_LOOP_DESCRIPTORS == 65535 + 600 and pp.look_trips(n) == 2 and case.per == 1 and case.max_piece == 5
    assert 65535 * REC < case.arena.size <= 32 << 20 and len(case.searched) == 60  # (nearly all of it records)
    kinds = []
    for k in range(pc.SYNC_LOOP_PAIRS):
        i = pc.sync_loop_first(k)
        (ka, da), (kb, db) = case.uses[i], case.uses[i + pp.LOOK_GRID_MAX]
        a, b = case.protos[ka], case.protos[kb]
        shape = lambda p, d: (p["L"], len(p["parts"])) if d else None  # noqa: E731
        kinds.append({((128, 1), (3, 5)): 0, ((3, 5), (128, 1)): 1}.get((shape(a, da), shape(b, db)), 2 if da and not db else 3 if db and not da else None))
    assert kinds == [k % 4 for k in range(pc.SYNC_LOOP_PAIRS)]
    assert {case.uses[i][0] for i in case.searched} == {0, 1, 2, 3}
    paired = {pc.sync_loop_first(k) + t for k in range(pc.SYNC_LOOP_PAIRS) for t in (0, pp.LOOK_GRID_MAX)}
    assert all(not data for i, (_, data) in enumerate(case.uses) if i not in paired)


def test_sync_short_rows_shift_the_history():
    case = pc.SYNC_CASES["short rows"]()
    seen = set()
    for p in case.protos:
        L, n = p["L"], p["n"]
        seen.add((L, n, p["restart"]))
        front = np.zeros(2 * ym.HIST, F32) if p["restart"] else p["hist"]
        assert p["hist_out"].tobytes() == np.concatenate([front, p["x"]])[-2 * ym.HIST:].tobytes()
        if n < ym.HIST:
            assert p["hist_out"][: 2 * (ym.HIST - n)].tobytes() == front[2 * n:].tobytes()
        assert p["n_windows"] == (max(0, n - L + 1) if p["restart"] else n) and len(p["parts"]) == 1
    assert seen == {(L, n, r) for L in pc.SYNC_SHORT_L for n in pc.sync_short_lengths(L) for r in (False, True)}
    assert any(p["n_windows"] == 0 and p["parts"][0]["best"] is None for p in case.protos), "a restarted row shorter than its word"
    assert {int(d["soft"]) % 128 for d in case.desc} == {0, 8}
