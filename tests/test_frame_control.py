"""The psk_soft_frame_ family without a GPU (include/psk_soft_frame.h): the exports and the layouts, known answers, the host
definitions (psk_soft_frame_search_host, psk_soft_frame_cut_host, psk_soft_frame_span) against the numpy model of
tests/frame_model.py byte for byte, every refusal, and the planned records of control-plane-only handles."""
import ctypes
import os
import re

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from tests import frame_cases as fc
from tests import frame_model as fm

ERR_INVALID_ARG = 1  # PSK_SOFT_ERR_INVALID_ARG
NEW = (
    "psk_soft_frame_word_define", "psk_soft_frame_search_device", "psk_soft_get_frame_search", "psk_soft_frame_search_host",
    "psk_soft_frame_tile", "psk_soft_frame_format_define", "psk_soft_frame_cut_device", "psk_soft_get_frame_cut",
    "psk_soft_frame_cut_host", "psk_soft_frame_span", "psk_soft_frame_search_bytes", "psk_soft_frame_search_in_bytes",
    "psk_soft_frame_cut_bytes", "psk_soft_frame_cut_in_bytes",
)


def host_search(c, rng=None):
    return pl.frame_search_host(c.length, c.word, c.care, c.packed(rng), c.n_bits, c.bit0, c.max_diff, c.period)


def host_cut(c, rng=None):
    return pl.frame_cut_host(c.branches, c.cell, c.packed(rng), c.bit, c.n_bytes, c.branch0, c.table, c.flags)


# ---- 1. exports, header, layouts ---------------------------------------------------------------------------------------------------------

def test_the_symbols_are_exported_and_the_records_have_their_layout():
    L = pl.load()
    assert L.psk_soft_abi_version() == 2
    assert set(pl.FRAME_EXPORTS) == set(NEW) and len(pl.FRAME_EXPORTS) == len(NEW)
    assert not set(pl.FRAME_EXPORTS) & (set(pl.EXPORTS) | set(pl.RS_EXPORTS))
    for name in NEW:
        assert hasattr(L, name), name
    inc = os.path.join(os.path.dirname(pl._HERE), "include")
    declared = set(re.findall(r"\b(psk_soft_[a-z_]+)\s*\(", open(os.path.join(inc, "psk_soft_frame.h")).read()))
    assert declared == set(pl.FRAME_EXPORTS), declared ^ set(pl.FRAME_EXPORTS)
    assert '#include "psk_soft_frame.h"' in open(os.path.join(inc, "psk_soft_hip.h")).read()
    for cls, size, offsets, query in (
        (pl.FrameSearchRecord, fm.SEARCH_BYTES, fm.SEARCH_OFFSETS, L.psk_soft_frame_search_bytes),
        (pl.FrameSearchIn, fm.SEARCH_IN_BYTES, fm.SEARCH_IN_OFFSETS, L.psk_soft_frame_search_in_bytes),
        (pl.FrameCutRecord, fm.CUT_BYTES, fm.CUT_OFFSETS, L.psk_soft_frame_cut_bytes),
        (pl.FrameCutIn, fm.CUT_IN_BYTES, fm.CUT_IN_OFFSETS, L.psk_soft_frame_cut_in_bytes),
    ):
        assert ctypes.sizeof(cls) == size == query(), cls
        assert {k: getattr(cls, k).offset for k, _ in cls._fields_} == offsets, cls
    assert ctypes.sizeof(pl.FrameHit) == 8 and {k: getattr(pl.FrameHit, k).offset for k, _ in pl.FrameHit._fields_} == fm.HIT_OFFSETS
    assert (fm.SEARCH_BYTES, fm.SEARCH_IN_BYTES, fm.CUT_BYTES, fm.CUT_IN_BYTES) == (192, 48, 32, 48)
    assert fm.SEARCH_DTYPE.itemsize == 192 and fm.CUT_DTYPE.itemsize == 32
    assert {k: fm.SEARCH_DTYPE.fields[k][1] for k in fm.SEARCH_DTYPE.names} == fm.SEARCH_OFFSETS
    assert (pl.FRAME_DATA, pl.FRAME_REC_INVERT, pl.FRAME_PLANNED, pl.FRAME_INVERT) == (fm.DATA, fm.REC_INVERT, fm.PLANNED, fm.INVERT)
    assert L.psk_soft_frame_tile() >= 1


def test_build_checks_the_new_exports():
    src = open(os.path.join(os.path.dirname(pl._HERE), "__graft_entry__.py")).read()
    assert "lib.FRAME_EXPORTS" in src


# ---- 2. known answers ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", (100, 101, 102, 103, 104))
def test_the_attached_sync_marker_behind_junk_bits(seed):
    """0x1ACFFC1D behind 11 junk bits, four frames of 4 + 255 random bytes, 20 bit flips, max_diff 2: the hits are the four markers"""
    rng = np.random.default_rng(seed)
    frames = [np.concatenate([np.frombuffer(fm.CCSDS_ASM.to_bytes(4, "big"), np.uint8), rng.integers(0, 256, 255).astype(np.uint8)])
              for _ in range(4)]
    bits = np.concatenate([rng.integers(0, 2, 11).astype(np.uint8), np.unpackbits(np.concatenate(frames))])
    flip = rng.choice(bits.size, 20, replace=False)
    bits[flip] ^= 1
    rec = pl.frame_search_host(32, fm.CCSDS_ASM, 0xFFFFFFFF, np.packbits(bits), bits.size, 0, 2, 0)
    assert [k[0] for k in rec.listed] == [11, 2083, 4155, 6227] and all(k[2] == 0 for k in rec.listed)
    assert list(rec.n_hit) == [4, 0] and rec.n_windows == bits.size - 31
    assert bytes(rec) == fm.search(32, fm.CCSDS_ASM, 0xFFFFFFFF, bits, 2, 0).tobytes()
    # folded over the frame length the markers share one phase
    rec = pl.frame_search_host(32, fm.CCSDS_ASM, 0xFFFFFFFF, np.packbits(bits), bits.size, 0, 2, 2072)
    assert (rec.best_phase, rec.best_score, rec.best_inv) == (11, 4, 0) and [k[0] for k in rec.listed] == [11, 2083, 4155, 6227]


def _dvb_bits(seed):
    rng = np.random.default_rng(seed)
    packets = rng.integers(0, 256, (16, 204)).astype(np.uint8)
    packets[:, 0] = 0x47
    packets[::8, 0] = 0xB8
    return np.concatenate([rng.integers(0, 2, 13).astype(np.uint8), np.unpackbits(packets.reshape(-1))])


@pytest.mark.parametrize("seed", (0, 1, 2, 3, 4))
def test_the_dvb_sync_byte_by_its_period(seed):
    """16 packets behind 13 junk bits, 0x47 with every eighth 0xB8, L = 8, max_diff 0, P = 1632: phase 13 scores 16, no other above 8"""
    bits = _dvb_bits(seed)
    rec = pl.frame_search_host(8, 0x47, 0xFF, np.packbits(bits), bits.size, 0, 0, 1632)
    assert (rec.best_phase, rec.best_score, rec.best_inv, rec.n_listed) == (13, 16, 2, 16)
    assert rec.listed == [(13 + 1632 * k, 0, 1 if k % 8 == 0 else 0) for k in range(16)]
    want = fm.search(8, 0x47, 0xFF, bits, 0, 1632)
    assert bytes(rec) == want.tobytes()
    win = np.lib.stride_tricks.sliding_window_view(bits, 8)
    v = np.packbits(win, axis=1).reshape(-1)
    score = np.bincount(np.flatnonzero((v == 0x47) | (v == 0xB8)) % 1632, minlength=1632)
    score[13] = 0
    assert score.max() <= 8
    # the whole stream inverted: the fourteen plain sync bytes are the inverted ones
    rec = pl.frame_search_host(8, 0x47, 0xFF, np.packbits(bits ^ 1), bits.size, 0, 0, 1632)
    assert (rec.best_phase, rec.best_score, rec.best_inv) == (13, 16, 14)


# ---- 3. the host definition against the model -----------------------------------------------------------------------------------------------

def test_search_host_against_the_model_on_the_directed_cases():
    rng = np.random.default_rng(7)
    cases = fc.search_cases() + tuple(fc.tile_edge_cases(pl.load().psk_soft_frame_tile()))
    labels = " ".join(c.label for c in cases)
    for L in (1, 7, 8, 9, 31, 32, 33, 63, 64):
        assert "L=%d " % L in labels
    for c in cases:
        assert bytes(host_search(c, rng)) == c.want.tobytes(), c.label
    # the cases are what they say
    by = {c.label: c.want for c in cases}
    assert int(by["tie: zeros"]["best_phase"]) == 0 and int(by["tie: zeros"]["min_pos"]) == 0
    assert int(by["tie: ones against zeros"]["min_pol"]) == 1
    assert (int(by["tie: two phases"]["best_phase"]), int(by["tie: two phases"]["best_score"])) == (4, 2)
    assert (int(by["tie: the minimum twice"]["min_diff"]), int(by["tie: the minimum twice"]["min_pos"])) == (1, 90)
    assert int(by["n_bits=31 L=32 P=0"]["n_windows"]) == 0 and int(by["n_bits=32 L=32 P=3"]["n_hit"][1]) == 1
    assert int(by["period=%d" % (1 << 20)]["best_phase"]) == 7


def test_search_host_against_the_model_on_random_draws():
    rng = np.random.default_rng(8)
    for trial in range(400):
        L = int(rng.integers(1, 65))
        care = int.from_bytes(rng.bytes(8), "little") & fc.full(L) or 1
        if trial % 3 == 0:
            care = fc.full(L)
        word = int.from_bytes(rng.bytes(8), "little") & fc.full(L)
        C = bin(care).count("1")
        md = int(rng.integers(0, (C + 1) // 2))
        n = int(rng.integers(1, 600))
        P = int(rng.choice([0, 1, 2, 7, max(L - 1, 1), 53, 64, 65, 1000]))
        bits = rng.integers(0, 2, n).astype(np.uint8)
        if trial % 2:  # (a stream that is mostly the word over and over has hits of both polarities)
            for pos in range(int(rng.integers(0, 20)), n - L, L + int(rng.integers(0, 30))):
                fc.plant(bits, pos, L, word, inverted=bool(rng.integers(0, 2)))
        c = fc.SearchCase("draw %d" % trial, L, word, care, bits, int(rng.integers(0, 64)), md, P)
        assert bytes(host_search(c, rng)) == c.want.tobytes(), (c.label, L, n, c.bit0, md, P)


# ---- 4. the cut ----------------------------------------------------------------------------------------------------------------------------

def test_cut_host_and_span_against_the_model():
    rng = np.random.default_rng(9)
    for c in fc.cut_cases():
        out, rec = host_cut(c, rng)
        assert out.tobytes() == c.want[0].tobytes() and bytes(rec) == c.want[1].tobytes(), c.label
        assert pl.frame_span(c.branches, c.cell, c.branch0, c.n_bytes) == c.span == rec.span, c.label
    labels = [c.label for c in fc.cut_cases()]
    for B, M in fc.SHAPES:
        for b0 in range(B):
            assert any(s.startswith("B=%d M=%d branch0=%d " % (B, M, b0)) for s in labels)
    assert pl.frame_span(12, 17, 0, 204) == 203 + 11 * 204 + 1 and pl.frame_span(1, 5, 0, 9) == 9 and pl.frame_span(5, 0, 3, 9) == 9
    for B, M in ((255, 255), (2, 1), (7, 3)):
        for n in (1, 2, B - 1, B, B + 1, 3 * B + 2):
            for b0 in {0, B // 2, B - 1}:
                if n >= 1:
                    assert pl.frame_span(B, M, b0, n) == fm.span(B, M, b0, n), (B, M, b0, n)
    assert pl.frame_span(12, 17, 0, 1 << 20) == fm.span(12, 17, 0, 1 << 20)
    # refused arguments give 0; the greatest format is within the delay bound (255 * 254 * 255 <= 2^24), so the bound refuses nothing
    # that branches <= 255 and cell <= 255 have not refused already
    for args in ((0, 0, 0, 1), (256, 0, 0, 1), (12, 256, 0, 1), (12, 17, 12, 1), (12, 17, 0, 0), (12, 17, 0, (1 << 20) + 1)):
        assert pl.frame_span(*args) == 0, args
    assert 255 * 254 * 255 <= pl.FRAME_MAX_DELAY and pl.frame_span(255, 255, 254, 1) == 254 * 255 * 255 + 1


def test_an_interleaver_in_the_model_then_the_cut_returns_the_packets():
    rng = np.random.default_rng(10)
    table = rng.permutation(256).astype(np.uint8)
    inverse = np.argsort(table).astype(np.uint8)
    for B, M in fc.SHAPES:
        n, count = (204, 6) if (B, M) == (12, 17) else (4 * B + 3, 9)
        packets = rng.integers(0, 256, (count, n)).astype(np.uint8)
        for bit in (0, 3, 13):
            for use_table in (False, True):
                sent = inverse[packets] if use_table else packets  # (the transmitter maps with the inverse table)
                stream = np.concatenate([fm.interleave(sent.reshape(-1), B, M, rng) ^ 0xFF, rng.integers(0, 256, 1).astype(np.uint8)])
                buf = fm.pack_at(np.unpackbits(stream), bit, rng)
                for q in range(count):
                    out, rec = pl.frame_cut_host(B, M, buf, bit + 8 * n * q, n, (n * q) % B, table if use_table else None, pl.FRAME_INVERT)
                    assert out.tobytes() == packets[q].tobytes(), (B, M, bit, use_table, q)
                    assert rec.flags == pl.FRAME_DATA | pl.FRAME_REC_INVERT and rec.n_ones == int(np.unpackbits(packets[q]).sum())


# ---- 5. refusals and control-plane-only handles -------------------------------------------------------------------------------------------

def _refused(call):
    with pytest.raises(pl.PskSoftError) as e:
        call()
    assert e.value.status == ERR_INVALID_ARG, e.value


def _sin(**kw):
    k = pl.FrameSearchIn(0x1000, 0, 100, 1, 0, 0, 0, (ctypes.c_uint32 * 3)(0, 0, 0))
    for name, v in kw.items():
        if name.startswith("pad"):
            k.pad[int(name[3:])] = v
        else:
            setattr(k, name, v)
    return k


def _cin(**kw):
    k = pl.FrameCutIn(0x1000, 0, 0x2000, 10, 0, 0, 0, (ctypes.c_uint32 * 2)(0, 0))
    for name, v in kw.items():
        if name.startswith("pad"):
            k.pad[int(name[3:])] = v
        else:
            setattr(k, name, v)
    return k


SEARCH_FAULTS = (dict(word=17), dict(word=3), dict(max_diff=16), dict(max_diff=1 << 31), dict(period=(1 << 20) + 1), dict(n_bits=0),
                 dict(n_bits=(1 << 31) + 1), dict(flags=1), dict(pad0=1), dict(pad1=1), dict(pad2=1))
CUT_FAULTS = (dict(format=17), dict(format=3), dict(format=1, branch0=12), dict(branch0=1), dict(n_bytes=0), dict(n_bytes=(1 << 20) + 1),
              dict(flags=2), dict(pad0=1), dict(pad1=1), dict(out=0))


def test_define_refusals():
    h = pl.Handle(1, device=pl.DEVICE_NONE)
    try:
        for args in ((16, 32, 1, 1), (0, 0, 0, 1), (0, 65, 1, 1), (0, 8, 0x100, 0xFF), (0, 8, 0x47, 0x1FF), (0, 8, 0x47, 0), (0, 63, 1 << 63, 1)):
            _refused(lambda: h.frame_word_define(*args))
        h.frame_word_define(15, 64, (1 << 64) - 1, 1 << 63)
        h.frame_word_define(0, 1, 1, 1)
        for args in ((16, 1, 0), (0, 0, 0), (0, 256, 0), (0, 12, 256)):
            _refused(lambda: h.frame_format_define(*args))
        h.frame_format_define(15, 255, 255)
        with pytest.raises(ValueError):
            h.frame_format_define(0, 1, 0, np.zeros(255, np.uint8))
        L = pl.load()
        assert L.psk_soft_frame_word_define(None, 0, 8, 0x47, 0xFF) == ERR_INVALID_ARG
        assert L.psk_soft_frame_format_define(None, 0, 1, 0, None) == ERR_INVALID_ARG
    finally:
        h.close()


def test_call_refusals_change_nothing_and_planned_records():
    L = pl.load()
    h = pl.Handle(1, device=pl.DEVICE_NONE)
    try:
        h.frame_word_define(0, 32, fm.CCSDS_ASM)
        h.frame_word_define(1, 8, 0x47)
        h.frame_format_define(0, 12, 17)
        h.frame_format_define(1, 1, 0, np.arange(256, dtype=np.uint8)[::-1].copy())
        # nothing to read before a call
        _refused(lambda: h.frame_search_records(0, 1))
        _refused(lambda: h.frame_cut_records(0, 1))
        # a good call of each kind: planned records
        sins = [_sin(n_bits=100, max_diff=2), _sin(word=0), _sin(bits=0), _sin(word=2, n_bits=7, period=1632), _sin(word=2, n_bits=8, max_diff=3)]
        h.frame_search_device(sins)
        got = h.frame_search_records(0, 5)
        want = np.zeros(5, fm.SEARCH_DTYPE)
        for i, (length, nw) in ((0, (32, 69)), (3, (8, 0)), (4, (8, 1))):
            want[i]["flags"], want[i]["length"], want[i]["n_windows"] = fm.PLANNED, length, nw
        assert bytes(got) == want.tobytes()
        cins = [_cin(), _cin(bits=0), _cin(format=1, branch0=11, n_bytes=204, flags=1), _cin(format=2, n_bytes=1 << 20)]
        h.frame_cut_device(cins)
        got = h.frame_cut_records(0, 4)
        want = np.zeros(4, fm.CUT_DTYPE)
        for i, (n, sp, fl) in ((0, (10, 10, 0)), (2, (204, fm.span(12, 17, 11, 204), 1)), (3, (1 << 20, 1 << 20, 0))):
            want[i]["flags"], want[i]["n_bytes"], want[i]["span"] = fm.PLANNED | (fl << 1), n, sp
        assert bytes(got) == want.tobytes()
        search_before, cut_before = bytes(h.frame_search_records(0, 5)), bytes(h.frame_cut_records(0, 4))
        # every refusal, in the last stream of a call whose others are good; the records stay
        for fault in SEARCH_FAULTS:
            _refused(lambda: h.frame_search_device([_sin(max_diff=1), _sin(**fault)]))
        for fault in CUT_FAULTS:
            _refused(lambda: h.frame_cut_device([_cin(), _cin(**fault)]))
        _refused(lambda: h.frame_search_device([_sin(word=2, max_diff=4)]))  # (2 max_diff = C)
        assert L.psk_soft_frame_search_device(h._h, 0, (pl.FrameSearchIn * 1)(), None) == ERR_INVALID_ARG
        assert L.psk_soft_frame_search_device(h._h, (1 << 20) + 1, (pl.FrameSearchIn * 1)(), None) == ERR_INVALID_ARG
        assert L.psk_soft_frame_search_device(h._h, 1, None, None) == ERR_INVALID_ARG
        assert L.psk_soft_frame_search_device(None, 1, (pl.FrameSearchIn * 1)(), None) == ERR_INVALID_ARG
        assert L.psk_soft_frame_cut_device(h._h, 0, (pl.FrameCutIn * 1)(), None) == ERR_INVALID_ARG
        assert L.psk_soft_frame_cut_device(h._h, (1 << 20) + 1, (pl.FrameCutIn * 1)(), None) == ERR_INVALID_ARG
        assert L.psk_soft_frame_cut_device(h._h, 1, None, None) == ERR_INVALID_ARG
        assert L.psk_soft_frame_cut_device(None, 1, (pl.FrameCutIn * 1)(), None) == ERR_INVALID_ARG
        _refused(lambda: h.frame_search_records(3, 3))
        _refused(lambda: h.frame_search_records(0, 0))
        _refused(lambda: h.frame_cut_records(4, 1))
        assert L.psk_soft_get_frame_search(h._h, 0, 1, None) == ERR_INVALID_ARG
        assert L.psk_soft_get_frame_cut(h._h, 0, 1, None) == ERR_INVALID_ARG
        assert bytes(h.frame_search_records(0, 5)) == search_before and bytes(h.frame_cut_records(0, 4)) == cut_before
        # the last call's records replace the ones before
        h.frame_search_device([_sin(word=2, n_bits=1 << 31, period=1 << 20)])
        rec = h.frame_search_records(0, 1)[0]
        assert (rec.flags, rec.length, rec.n_windows) == (fm.PLANNED, 8, (1 << 31) - 7)
        _refused(lambda: h.frame_search_records(1, 1))
    finally:
        h.close()


def test_host_definition_refusals():
    L = pl.load()
    rec, crec = pl.FrameSearchRecord(), pl.FrameCutRecord()
    buf = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    good = _sin(bits=buf.ctypes.data, n_bits=100)
    assert L.psk_soft_frame_search_host(32, fm.CCSDS_ASM, 0xFFFFFFFF, ctypes.byref(good), ctypes.byref(rec)) == pl.OK
    for length, word, care in ((0, 0, 1), (65, 1, 1), (8, 0x100, 0xFF), (8, 1, 0x100), (8, 1, 0)):
        assert L.psk_soft_frame_search_host(length, word, care, ctypes.byref(good), ctypes.byref(rec)) == ERR_INVALID_ARG
    assert L.psk_soft_frame_search_host(32, 1, 1, None, ctypes.byref(rec)) == ERR_INVALID_ARG
    assert L.psk_soft_frame_search_host(32, 1, 1, ctypes.byref(good), None) == ERR_INVALID_ARG
    for fault in SEARCH_FAULTS:
        if "word" in fault:
            continue  # (the host definition does not look at the slot)
        k = _sin(bits=buf.ctypes.data, n_bits=100, **fault) if "n_bits" not in fault else _sin(bits=buf.ctypes.data, **fault)
        assert L.psk_soft_frame_search_host(32, fm.CCSDS_ASM, 0xFFFFFFFF, ctypes.byref(k), ctypes.byref(rec)) == ERR_INVALID_ARG, fault
    # skipped: the zero record
    rec.flags = 77
    assert L.psk_soft_frame_search_host(32, 1, 1, ctypes.byref(_sin(word=0)), ctypes.byref(rec)) == pl.OK and bytes(rec) == bytes(192)
    good = _cin(bits=buf.ctypes.data, out=out.ctypes.data)
    assert L.psk_soft_frame_cut_host(1, 0, None, ctypes.byref(good), ctypes.byref(crec)) == pl.OK
    for B, M in ((0, 0), (256, 0), (12, 256)):
        assert L.psk_soft_frame_cut_host(B, M, None, ctypes.byref(good), ctypes.byref(crec)) == ERR_INVALID_ARG
    assert L.psk_soft_frame_cut_host(1, 0, None, None, ctypes.byref(crec)) == ERR_INVALID_ARG
    assert L.psk_soft_frame_cut_host(1, 0, None, ctypes.byref(good), None) == ERR_INVALID_ARG
    for fault in CUT_FAULTS:
        if "format" in fault:
            continue  # (nor at the format's)
        k = _cin(bits=buf.ctypes.data, **({"out": out.ctypes.data, **fault}))
        assert L.psk_soft_frame_cut_host(1, 0, None, ctypes.byref(k), ctypes.byref(crec)) == ERR_INVALID_ARG, fault
    crec.flags = 77
    assert L.psk_soft_frame_cut_host(1, 0, None, ctypes.byref(_cin(bits=0)), ctypes.byref(crec)) == pl.OK and bytes(crec) == bytes(32)


# ---- 6. the chain test's stream is decodable --------------------------------------------------------------------------------------------

def test_the_chain_stream_decodes_outside_its_tail():
    """what tests/test_gpu_frame.py's chain relies on, checked without a GPU: psk_soft_viterbi_host returns the sent bits outside the
    unterminated tail, the tail lies behind every frame the chain cuts, and the host definitions walk the chain to the data"""
    ch = fc.chain()
    out, vrec = pl.viterbi_host(ch["K"], ch["g"], 1, 3, ch["llr"], ch["n_steps"], pl.VITERBI_PACKED)
    got = np.unpackbits(out)[: ch["n_steps"]]
    good = ch["n_steps"] - 8 * fc.CHAIN_TAIL_BYTES
    assert np.array_equal(got[:good], ch["sent"][:good])
    span = pl.frame_span(fm.DVB_B, fm.DVB_M, 0, 204)
    assert fc.CHAIN_JUNK_BITS + 8 * (204 * (fc.CHAIN_PACKETS - 1) + span) <= good
    rec = pl.frame_search_host(8, 0x47, 0xFF, out, good, 0, 0, fm.DVB_PERIOD)
    assert (rec.best_phase, rec.best_score, rec.best_inv) == (fc.CHAIN_JUNK_BITS, fc.CHAIN_PACKETS, 3)
    for q in range(fc.CHAIN_PACKETS):
        pkt, _ = pl.frame_cut_host(fm.DVB_B, fm.DVB_M, out, rec.best_phase + fm.DVB_PERIOD * q, 204, 0)
        assert pkt.tobytes() == ch["packets"][q].tobytes()
        data, rrec = pl.rs_host(*pl.RS_DVB, 1, pkt)
        assert data.tobytes() == ch["data"][q].tobytes() and rrec.n_err[0] == ch["errors"][q]
