"""tests/row_guards.py on numpy stand-ins (no GPU): the layout is what DESIGN.md section 4.5 says, a stand-in that writes its
rows correctly is reported clean, and each of five injected faults -- the stores a wrong emit stage would make -- is reported
at its place.  This is the demonstration that the GPU tests built on the module would catch a wrong kernel."""
import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests import row_guards as rg

# channel: symbols, bits per symbol, samplesPerBaud > 1.  An odd bits row (channel 0: bare alignment; 3: a line), a channel
# without sampleIndex (samplesPerBaud 1), one without bits (constelationSize 16), one that emits nothing, one symbol
SHAPES = [(131, 3, True), (257, 2, True), (64, 1, False), (77, 1, True), (129, 0, True), (0, 2, True), (1, 3, True)]
COUNTS = [dict(n_symbols=n, n_bits=n * b, n_sampleIndex=n if s else 0) for n, b, s in SHAPES]
ABSENT = [(), (), ("bits",), (), ("phase", "index"), (), ("soft",)]
BASE = 0x7F0000400000  # a made-up device address on a line


def _packets():
    rng = np.random.default_rng(5)
    return [rng.standard_normal(2 * 300).astype(np.float32), rng.integers(-9, 9, 2 * 301).astype(np.int16), rng.integers(-9, 9, 2 * 33).astype(np.int8),
            None, rng.standard_normal(2 * 7).astype(np.float16), np.zeros(0, np.float32), rng.standard_normal(2).astype(np.float32)]


@pytest.fixture()
def layout():
    return rg.Layout(COUNTS, absent=ABSENT, packets=_packets(), call=3)


def _written(layout):
    """the arenas after a stand-in kernel that writes every row it has a pointer for, and nothing else"""
    after = layout.images()
    for s in rg.STREAMS:
        for r in layout.arenas[s].rows:
            if r.present:
                after[s][r.start : r.end] = (np.arange(r.nbytes) * 7 + r.channel) % 251
    return after


def test_layout(layout):
    img = layout.images()
    for s in rg.STREAMS:
        a, al = layout.arenas[s], rg.MIN_ALIGN[s]
        assert [r.channel for r in a.rows] == list(range(len(COUNTS)))
        edge = 0
        for r in a.rows:
            assert r.nbytes == rg.row_bytes(s, COUNTS[r.channel])
            if r.channel % 2 == 0:
                assert r.start % (2 * al) == al, "the least alignment the ABI asks for, and no more"
            else:
                assert r.start % rg.LINE == 0
            assert r.start - rg.GUARD >= edge, "the guard in front does not reach into the guard behind the row before"
            edge = r.end + rg.GUARD
            assert edge <= a.size
            assert (img[s][r.start - rg.GUARD : r.start] == rg.GUARD_BYTE).all() and (img[s][r.end : r.end + rg.GUARD] == rg.GUARD_BYTE).all()
            assert (img[s][r.start : r.end] == rg.ROW_BYTE).all()
            assert r.present == (s not in ABSENT[r.channel])
        assert img[s].size == a.size and np.count_nonzero(img[s] == rg.ROW_BYTE) == sum(r.nbytes for r in a.rows)
    assert layout.arenas["bits"].rows[0].end % 4 == 2, "a guard that starts where no 4-byte store starts"
    assert layout.arenas["index"].rows[2].nbytes == 0 and layout.arenas["bits"].rows[4].nbytes == 0 and layout.arenas["soft"].rows[5].nbytes == 0


def test_packets_lie_between_guards(layout):
    img, pk = layout.images()["packet"], _packets()
    edge = 0
    for c, at in enumerate(layout.packet_at):
        if pk[c] is None:
            assert at is None
            continue
        off, n, fmt = at
        sb = rg.FORMAT_ALIGN[fmt]
        assert n == pk[c].size and fmt == rg.FORMAT_OF[pk[c].dtype]
        assert off % (2 * sb) == sb if c % 2 == 0 else off % rg.LINE == 0
        assert off - rg.GUARD >= edge
        edge = off + pk[c].nbytes + rg.GUARD
        assert img[off : off + pk[c].nbytes].tobytes() == pk[c].tobytes()
        assert (img[off - rg.GUARD : off] == rg.GUARD_BYTE).all() and (img[off + pk[c].nbytes : edge] == rg.GUARD_BYTE).all()
    assert edge <= img.size


def test_fill_hands_over_exact_rows(layout):
    n = len(COUNTS)
    pk, out = (pl.Packet * n)(), (pl.Output * n)()
    bases = {s: BASE + i * (1 << 24) for i, s in enumerate(rg.STREAMS + ("packet",))}
    layout.fill(bases, pk, out, sri_changed=True)
    for c in range(n):
        assert out[c].cap_symbols == COUNTS[c]["n_symbols"], "the tightest legal value"
        for s in rg.STREAMS:
            p = getattr(out[c], rg.FIELD[s])
            assert (p is None) == (s in ABSENT[c])
            if p is not None:
                assert p == bases[s] + layout.arenas[s].rows[c].start and p % rg.MIN_ALIGN[s] == 0
        assert pk[c].present == (layout.packet_at[c] is not None)
        if pk[c].present:
            assert pk[c].data == bases["packet"] + layout.packet_at[c][0] and pk[c].n_floats == layout.packet_at[c][1]
            assert pk[c].sriChanged == 1 and pk[c].sri_mode == 1
    all_null = rg.Layout(COUNTS[:1], absent=[rg.STREAMS], packets=_packets()[:1])
    all_null.fill(bases, pk, out)
    assert out[0].cap_symbols == 0 and all(getattr(out[0], f) is None for f in rg.FIELD.values())
    with pytest.raises(AssertionError):
        layout.fill(dict(bases, soft=BASE + 8), pk, out)


def test_a_correct_writer_is_clean(layout):
    after = _written(layout)
    assert layout.check(after) == []
    for c in range(len(COUNTS)):
        got = layout.extract(after, c)
        for s in rg.STREAMS:
            if s in ABSENT[c]:
                assert got[s] is None
            else:
                assert got[s].dtype == rg.DTYPE[s] and got[s].nbytes == rg.row_bytes(s, COUNTS[c])


def _one(layout, after):
    found = layout.check(after)
    assert len(found) == 1, rg.messages(found)
    return found[0]


def test_two_bytes_past_an_odd_bits_row(layout):
    """the second half of a 4-byte store at the odd tail of a bits row"""
    after = _written(layout)
    r = layout.arenas["bits"].rows[0]
    assert r.nbytes % 4 == 2
    after["bits"][r.end : r.end + 2] = (0x01, 0x00)
    f = _one(layout, after)
    assert (f["call"], f["channel"], f["stream"], f["where"]) == (3, 0, "bits", "behind")
    assert f["offsets"] == [0, 1] and f["values"] == [1, 0]
    assert "channel 0 bits" in f["message"] and "0 .. 1 bytes past its end" in f["message"]


def test_sixteen_bytes_past_a_soft_row(layout):
    """store_f4u of two symbols where one was valid"""
    after = _written(layout)
    r = layout.arenas["soft"].rows[3]
    after["soft"][r.end : r.end + 16] = 0
    f = _one(layout, after)
    assert (f["channel"], f["stream"], f["where"]) == (3, "soft", "behind")
    assert f["offsets"] == list(range(rg.REPORTED)) and "channel 3 soft: 16 byte(s)" in f["message"] and "0 .. 15 bytes past its end" in f["message"]


def test_a_whole_block_behind_the_end(layout):
    """a wave's soft output for one block, one block late"""
    after = _written(layout)
    r = layout.arenas["soft"].rows[1]
    after["soft"][r.end : r.end + 1024] = 0x11
    f = _one(layout, after)
    assert (f["channel"], f["stream"], f["where"]) == (1, "soft", "behind")
    assert "1024 byte(s)" in f["message"] and "0 .. 1023 bytes past its end" in f["message"]


def test_two_bytes_in_front_of_a_row(layout):
    after = _written(layout)
    r = layout.arenas["index"].rows[1]
    after["index"][r.start - 2 : r.start] = (0xFF, 0x7F)
    f = _one(layout, after)
    assert (f["channel"], f["stream"], f["where"]) == (1, "index", "front")
    assert f["offsets"] == [-2, -1] and f["values"] == [0xFF, 0x7F]
    assert "channel 1 index" in f["message"] and "1 .. 2 bytes before its start" in f["message"]


def test_one_packet_byte_changed(layout):
    after = _written(layout)
    off = layout.packet_at[1][0] + 77
    after["packet"][off] ^= 0x40
    f = _one(layout, after)
    assert (f["channel"], f["stream"], f["where"], f["offsets"]) == (1, "packet", "packet", [off])
    assert "offset %d (channel 1)" % off in f["message"]
    # and a byte of the guard between two packets
    after = _written(layout)
    after["packet"][layout.packet_at[0][0] - 1] = 0
    assert _one(layout, after)["where"] == "packet"


def test_a_store_through_a_pointer_the_call_did_not_have(layout):
    """the place of an absent row must stay as it went up; a row the call had a pointer for must not"""
    after = _written(layout)
    r = layout.arenas["phase"].rows[4]
    assert not r.present
    after["phase"][r.start + 8 : r.start + 12] = 0
    f = _one(layout, after)
    assert (f["channel"], f["stream"], f["where"], f["offsets"]) == (4, "phase", "row", [8, 9, 10, 11])
    after = _written(layout)
    r = layout.arenas["phase"].rows[0]
    after["phase"][r.start : r.end] = rg.ROW_BYTE
    f = _one(layout, after)
    assert (f["channel"], f["stream"], f["where"]) == (0, "phase", "unwritten")


def test_a_frame_matrix_is_its_own_guard():
    """packet_image: every byte of the caller's arena outside the packets is compared as well"""
    m = np.arange(64 * 12, dtype=np.float32).reshape(64, 12).view(np.uint8).reshape(-1)
    lay = rg.Layout(COUNTS[:2], packet_image=(m, [(8 * 3, 2 * 32, 0), (8 * 4, 2 * 32, 0)]))
    after = _written(lay)
    assert lay.check(after) == []
    after["packet"][8 * 5 + 1] ^= 1
    assert _one(lay, after)["offsets"] == [41]
