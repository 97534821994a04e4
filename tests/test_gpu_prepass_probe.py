"""The gather, tune, resample and filter kernels and (at the end of the file) the two looks and the word search by themselves on a real MI355X (psk_soft_amd/libpsk_prepass_probe.so: a shim
linked with the product's own psk_gather.o, psk_tune.o, psk_resample.o and psk_fir.o).  The demodulator behind these kernels shows one row sample
in eight at samplesPerBaud 8; here every byte of the arena a launch ran in is compared with the arena
the models expect -- a byte copy for the gathers, tests/tune_model.py for the tune kernel, tests/tune_model.py followed by
tests/resample_model.py for the resample kernel, tests/tune_model.py followed by tests/fir_model.py for the filter kernel: every
row sample and both history slots bit for bit, no tolerance, and every source byte (the taps among them), every byte of row
padding, the padding of the filter's history slots and every guard byte unchanged.  The inputs hold finite samples only.

The inputs come from tests/prepass_probe_cases.py; tests/test_prepass_probe.py asserts, without a GPU, the launch shapes and the
edges each of them reaches, and that the comparator reports a wrong store at its place."""
import numpy as np
import pytest

from tests import prepass_probe as pp
from tests import prepass_probe_cases as pc
from tests import tune_model as tm

pytestmark = pytest.mark.gpu


def _clean(case, after, ctx):
    found = case.check(after)
    assert not found, "%s:\n%s" % (ctx, pp.messages(found))


# ---- resample ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", range(4))
def test_resample_one_packet_a_workgroup_per_piece(variant):
    """one packet of 3P+1 outputs: four workgroups, a piece each (the shape the rest of the suite runs), in each format"""
    case = pc.resample_shape(1, variant)
    _clean(case, case.run(), "one packet, variant %d" % variant)


@pytest.mark.parametrize("packets", [700, 1100, 2100])
def test_resample_workgroups_that_walk_several_pieces(packets):
    """700 packets: three workgroups a packet, up to three pieces each; 1100: two, the history's owner workgroup 0 for some
    packets and 1 for others; 2100: one workgroup walks every piece, then writes the history.  All but ten packets have 1 .. 40
    samples, some no output at all: their histories still move."""
    case = pc.resample_shape(packets)
    _clean(case, case.run(), "%d packets" % packets)


def test_resample_arithmetic_edges():
    """every step with the pos fractions 0, 255, 256 and 2^32 - 1; pos 2^33; samples scaled by 2^-130 (a flush to zero anywhere
    would show) and up to 2^125; zeros of both signs at step 2^32, pos 0"""
    case, kinds = pc.resample_edges()
    _clean(case, case.run(), "arithmetic edges %s" % {k: (v[0], v[-1]) for k, v in kinds.items()})


# ---- fir -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", pc.FIR_DS)
def test_fir_every_decimation(D):
    """one launch at D: tap counts 1, 2, lead, lead + 1, lead + 2 (the edges of the three-way split of the tap walk), 64, 127,
    128 x outputs 1 .. 5, P-1, P, P+1, 2P+1 (every tail of a lane's R outputs, both sides of a piece edge), every pos below D,
    the four formats, strides 1 and 7, tuned and not, restart, a preset history and zeros; every piece has its own workgroup"""
    case = pc.fir_grid(D)
    _clean(case, case.run(), "D = %d, %d packets" % (D, len(case.desc)))


@pytest.mark.parametrize("packets", pc.FIR_SHAPES)
def test_fir_workgroups_that_walk_several_pieces(packets):
    """700 packets: three workgroups a packet take pieces (0,3,6), (1,4,7), (2,5) of the longest; 1100: two, the history's owner
    workgroup 0 for some packets and 1 for others; 2100: one workgroup walks every piece, then writes the history.  D is mixed
    over 1 .. 16 within a launch; all but ten packets are short, every 50th has pos >= n: no output, and its history moves."""
    case = pc.fir_shape(packets)
    _clean(case, case.run(), "%d filtered packets" % packets)


def test_fir_arithmetic_edges():
    """at a D of each lane class: float32 samples scaled by 2^-130 under taps near 1 (every product subnormal); subnormal, +0 and
    -0 taps, each as tap 0; zeros of both signs under negative taps; samples up to 2^125 / T"""
    case, kinds = pc.fir_edges()
    _clean(case, case.run(), "arithmetic edges %s" % {k: (v[0], v[-1]) for k, v in kinds.items()})


# ---- tune ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", pc.TUNE_COUNTS)
def test_tune(count):
    """lengths at the edges of kTuneMinPiece and of the 512-sample unit, both loops of tune_piece with their tails, the four
    formats, steps 0 (with a phase), 1, 2^63 and 2^64 - 1, packets scaled by 2^-130; and the device's tables behind the launch"""
    case = pc.tune_case(count)
    after, (C, F) = case.run()
    wc, wf = tm.tables()
    assert np.array_equal(C.view(np.uint32), wc.view(np.uint32)) and np.array_equal(F.view(np.uint32), wf.view(np.uint32)), "tune_tables()"
    _clean(case, after, "%d tuned packets" % count)


# ---- gathers ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", pc.SINGLES_COUNTS)
@pytest.mark.parametrize("sample_bytes", [2, 4, 8])
def test_gather_singles(sample_bytes, count):
    case = pc.singles_case(sample_bytes, count)
    _clean(case, case.run(), "%d singles of %d-byte samples" % (count, sample_bytes))


@pytest.mark.parametrize("sample_bytes", [2, 4, 8])
def test_gather_tiles_group_widths_and_ragged_columns(sample_bytes):
    """groups 8, 9, 63, 64, 65 and 130 columns wide, the columns of each 1, 63, 64, 65 and 200 frames long"""
    case = pc.tiles_widths_case(sample_bytes)
    _clean(case, case.run(), "tile widths, %d-byte samples" % sample_bytes)


@pytest.mark.parametrize("sample_bytes", [2, 4, 8])
def test_gather_tiles_more_tiles_than_workgroups(sample_bytes):
    """2100 groups of 8 columns by 10 frames: workgroups 0 .. 51 take a second tile"""
    case = pc.tiles_many_case(sample_bytes)
    _clean(case, case.run(), "%d tiles, %d-byte samples" % (case.n_tiles, sample_bytes))


# ---- the two looks: fold and join ------------------------------------------------------------------------------------------------------
#
# psk_symrate.hip and psk_acquire.hip through the shim, psk_symrate.o and psk_acquire.o as the product's build made them: one
# launch of the fold, one of the join.  The arena holds the sources, the partials and the records; the expected bytes are
# tests/symrate_model.py's and tests/acquire_model.py's restatements of the device's order of additions -- every partial of every
# piece and every record byte for byte, and every pad of a partial, every partial and record slot no descriptor owns, every
# source byte and every guard byte unchanged.

@pytest.mark.parametrize("W", pc.SR_WIDTHS)
def test_symrate_every_lane_width(W):
    """every S of the width class x block counts either side of one wave's blocks, of the workgroup's four waves, of a turn of
    stage 2, of a piece and of its halo; ragged tails; the four formats, strides 1 and 7, tuned and not"""
    case = pc.symrate_width(W)
    _clean(case, case.run(), "width %d, %d packets, arena %d bytes" % (W, len(case.desc), case.arena.size))


@pytest.mark.parametrize("W", pc.SR_WIDTHS)
def test_symrate_a_non_finite_sample_takes_its_block_and_no_other_of_the_wave(W):
    """40, 41 and 642 blocks, one NaN or inf a packet: in the first lane's first and second turn, the group's last lane, a ragged
    last turn; in a block that is the first and one that is the last of its wave, in the packet's last block with the rest of
    the wave idle; the last sample of block 511 (piece 1's own blocks and its halo) and of block 383 (its halo alone)"""
    case = pc.symrate_validity(W)
    _clean(case, case.run(), "validity at width %d, %d packets" % (W, len(case.desc)))


def test_symrate_arithmetic_edges():
    """samples scaled by 2^-130, samples whose e overflows, zeros of both signs"""
    case, kinds = pc.symrate_edges()
    _clean(case, case.run(), "arithmetic edges %s" % {k: (v[0], v[-1]) for k, v in kinds.items()})


def test_symrate_more_packets_than_the_grid_has_rows():
    """70000 descriptors: the workgroups of packets 0 .. 4464 take packets 65535 .. 69999 on a second trip, with the LDS of the
    first still in place -- two pieces in front of a first piece of three blocks and the reverse, data in front of none, invalid
    blocks in front of valid ones"""
    case = pc.symrate_loop()
    _clean(case, case.run(), "%d symrate descriptors, arena %d bytes" % (len(case.desc), case.arena.size))


@pytest.mark.parametrize("mixed", (False, True))
def test_acquire_lengths_formats_and_placements(mixed):
    """the lengths at the edges of a piece and the three of 64 pieces and more (the join's lanes 0 and 1 take two partials), each
    format aligned to its pair, one sample off and at stride 7; inf, NaN, zeros and underflowing samples across piece boundaries;
    without a tuned packet (no tables) and with"""
    case = pc.acquire_lengths_case(mixed)
    _clean(case, case.run(), "acquire lengths, mixed %d, arena %d bytes" % (mixed, case.arena.size))


def test_acquire_more_packets_than_the_grid_has_rows():
    case = pc.acquire_loop()
    _clean(case, case.run(), "%d acquire descriptors, arena %d bytes" % (len(case.desc), case.arena.size))


# ---- the word search: fold and join ----------------------------------------------------------------------------------------------------
#
# psk_sync.hip through the shim, psk_sync.o as the product's build made it.  The arena holds the rows, the words, both history
# slots of every searched descriptor, the partials and the records -- the last three are memory the handle owns in the product,
# which the guards of tests/test_gpu_sync.py cannot fence.  Expected, byte for byte: of every partial the members
# sync_model.partial_writes lists and NaN poison in the others (an unwritten best, hits[k] from min(n_hits, 16) on), the record
# sync_model.join_bytes makes of the partials, the model's 1016 bytes of history and poison in the 8 behind them, 456 zero bytes
# for a descriptor without data, and every spare partial, spare record, row, word, hist_in and guard byte as it went up.
# tests/test_prepass_probe.py asserts what each case reaches.

def _sync_clean(name):
    case = pc.SYNC_CASES[name]()
    after = case.run()
    _clean(case, after, "sync %s: %d descriptors, arena %d bytes, %d workgroup(s) a channel" % (name, len(case.desc), case.arena.size, case.per))
    return case, after


def test_sync_every_word_length():
    """L = 1 .. 128, a continued and a restarted row each, P + 65 windows: 256 descriptors, a workgroup a piece.  Then the same
    256 among 1900 descriptors without data: one workgroup a channel walks both pieces, and leaves the same bytes."""
    one, a = _sync_clean("lengths")
    two, b = _sync_clean("lengths spread")
    assert (one.per, two.per) == (2, 1)
    for k, i in enumerate(two.searched):
        assert two.uses[i][0] == one.uses[k][0] == k
        assert two.record_bytes(b, i) == one.record_bytes(a, k), "L %d" % (k // 2 + 1)
        for q in range(2):
            assert two.partial_bytes(b, i, q) == one.partial_bytes(a, k, q), "L %d, piece %d" % (k // 2 + 1, q)


@pytest.mark.parametrize("n_desc", pc.SYNC_WALK_SHAPES)
def test_sync_workgroups_that_walk_several_pieces(n_desc):
    """700, 1100 and 2100 descriptors: three, two and one workgroup a channel over rows of up to seven pieces -- more than 16
    hits in a piece that is not its workgroup's first, a piece without a valid window between two with, equal bests in pieces of
    one workgroup and of two, channels of one piece next to channels of seven"""
    _sync_clean("walk %d" % n_desc)


def test_sync_rows_of_more_than_64_pieces():
    """rows of 1, 63, 64, 65, 127, 128, 129 and 130 pieces: the join's second and third trip -- the hits of the chunks before
    carried, the cap of 16 met across a chunk edge, the best across chunks"""
    _sync_clean("chunks")


def test_sync_join_alone_on_written_partials():
    """the join by itself on partials numpy wrote, NaN poison in every member it may not read: 1, 64, 65 and 200 pieces of 1024
    hits; 0, 1, 15, 16, 17 and 1024 hits mixed, the cap met in lane 0, in lane 63 and at the chunk edge"""
    case, after = _sync_clean("join alone")
    full = case.protos[3]
    rec = np.frombuffer(case.record_bytes(after, case.searched[3]), pc.ym.RECORD_DTYPE)[0]
    assert len(full["parts"]) == 200 and int(rec["n_valid"]) == int(rec["n_hits"]) == 204800
    assert rec["hits"].tobytes() == full["parts"][0]["hits"].tobytes()


def test_sync_more_channels_than_the_grid_has_rows():
    """65535 + 600 descriptors, 40 pairs (i, i + 65535) that differ in L, in their pieces and in having data at all"""
    _sync_clean("loop")


def test_sync_short_rows_and_the_history():
    """rows of 1, L - 1, 126, 127, 128 and 300 symbols at L = 1, 64, 128: the history shifted by fewer than 127 symbols"""
    _sync_clean("short rows")
