"""psk_soft_rs_device without a GPU: the exports and the layouts, known answers of the encoder, the host-side definition
(psk_soft_rs_host) and the encoder against tests/rs_model.py byte for byte -- random codes drawn over every parameter and the
directed cases: error counts 0, 1, t, t+1, the values 1 and 0xff, the positions 0, k-1, k, n-1, 63 and 64, the neighbour
codeword, the root in the pad of a shortened code, every mask length, with and without parity, every depth --, every refusal, and
the entry on control-plane-only handles (PSK_SOFT_DEVICE_NONE): it checks, then leaves planned records and nothing else."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import rs_model as rm

NEW = ("psk_soft_rs_define", "psk_soft_rs_device", "psk_soft_get_rs", "psk_soft_rs_host", "psk_soft_rs_encode_host", "psk_soft_rs_bytes",
       "psk_soft_rs_in_bytes")


def test_the_symbols_are_exported_and_the_records_have_their_layout():
    L = pl.load()
    for name in NEW:
        assert name in pl.RS_EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    # the family has a header of its own, which psk_soft_hip.h includes, and a list of its own next to EXPORTS: the header and the
    # list are held to each other as tests/test_control_plane.py holds psk_soft_hip.h and EXPORTS
    assert len(pl.RS_EXPORTS) == len(NEW) == 7 and not set(pl.RS_EXPORTS) & set(pl.EXPORTS)
    inc = os.path.join(os.path.dirname(pl._HERE), "include")
    declared = set(re.findall(r"\b(psk_soft_[a-z_]+)\s*\(", open(os.path.join(inc, "psk_soft_rs.h")).read()))
    assert declared == set(pl.RS_EXPORTS), declared ^ set(pl.RS_EXPORTS)
    assert '#include "psk_soft_rs.h"' in open(os.path.join(inc, "psk_soft_hip.h")).read()
    R, I = pl.RsRecord, pl.RsIn
    assert ctypes.sizeof(R) == 64 == rm.RECORD_BYTES == L.psk_soft_rs_bytes() == rm.RECORD_DTYPE.itemsize
    assert ctypes.sizeof(I) == 32 == rm.IN_BYTES == L.psk_soft_rs_in_bytes()
    names = ("flags", "n", "k", "depth", "nroots", "pad0", "n_err", "n_bit", "pad1")
    assert [getattr(R, k).offset for k in names] == [0, 4, 6, 8, 9, 10, 16, 24, 40]
    assert [rm.RECORD_DTYPE.fields[k][1] for k in names] == [0, 4, 6, 8, 9, 10, 16, 24, 40]
    assert [getattr(I, k).offset for k in ("in_", "out", "code", "flags", "pad")] == [0, 8, 16, 20, 24]
    assert pl.RS_WITH_PARITY == 1 == rm.WITH_PARITY and (pl.RS_DATA, pl.RS_REC_WITH_PARITY, pl.RS_PLANNED) == (1, 2, 128) == (rm.DATA, 2, rm.PLANNED)
    assert (pl.RS_SLOTS, pl.RS_MAX_FRAMES, pl.RS_MAX_DEPTH, pl.RS_MAX_ROOTS, pl.RS_FAILED) == (16, 1 << 20, 8, 64, 255) and rm.FAILED == 255
    assert pl.RS_CCSDS == rm.CCSDS == (0x187, 112, 11, 32, 255) and pl.RS_DVB == rm.DVB == (0x11D, 0, 1, 16, 204)


# ---- known answers -------------------------------------------------------------------------------------------------------------------

def _parity_of_one(params):
    gfpoly, fcr, prim, nroots, n = params
    data = np.zeros(n - nroots, np.uint8)
    data[-1] = 1
    frame = pl.rs_encode_host(gfpoly, fcr, prim, nroots, n, 1, data)
    assert frame[: n - nroots].tobytes() == data.tobytes()
    return [int(x) for x in frame[n - nroots:]]


def test_the_generator_of_the_dvb_code():
    """data = k-1 zeros then a 1: the parity is g(x) without its leading 1"""
    assert _parity_of_one(rm.DVB) == [59, 13, 104, 189, 68, 209, 30, 8, 163, 65, 41, 229, 98, 50, 36, 59]


def test_the_generator_of_the_ccsds_code():
    p = _parity_of_one(rm.CCSDS)
    assert p[-1] == 1
    full = [1] + p  # (the leading 1 restored: 33 coefficients, a palindrome)
    assert full == full[::-1] and all(p[i] == p[30 - i] for i in range(31))
    exp, log = rm.tables(0x187)
    assert [int(log[x]) for x in p[:16]] == [249, 59, 66, 4, 43, 126, 251, 97, 30, 3, 213, 50, 66, 170, 5, 24]


def test_which_field_polynomials_are_primitive():
    """the 16 primitive polynomials of degree 8 are taken, every other value of 0x100 .. 0x1ff is refused"""
    L = pl.load()
    data, out = np.zeros(255, np.uint8), np.zeros(255 * 8, np.uint8)
    taken = [p for p in range(0x100, 0x200) if L.psk_soft_rs_encode_host(p, 0, 1, 2, 255, 1, None, 0, data.ctypes.data, out.ctypes.data) == 0]
    assert tuple(taken) == rm.PRIMITIVE_POLYS and all(rm.is_primitive(p) == (p in taken) for p in range(0x100, 0x200))


# ---- the definition ------------------------------------------------------------------------------------------------------------------

def check_host(code, frame, flags, ctx, model=None):
    """model: what code.decode(frame, WITH_PARITY) gave, if the caller has it already"""
    out, rec = pl.rs_host(*code.args, frame, code.mask, flags)
    mout, mrec = model or code.decode(frame, rm.WITH_PARITY)
    if not flags & rm.WITH_PARITY:  # (the same codewords, the data alone)
        mout, mrec = mout[: code.k * code.depth], mrec.copy()
        mrec["flags"] = rm.DATA
    assert out.dtype == mout.dtype and out.tobytes() == mout.tobytes(), ctx + ": output"
    rm.assert_same(rec, mrec, ctx)
    return out, rec


def check_encoder(code, rng):
    data = rng.integers(0, 256, code.k * code.depth).astype(np.uint8)
    frame = pl.rs_encode_host(*code.args, data, code.mask)
    assert frame.tobytes() == code.encode(data).tobytes(), "encoder, code %s" % (code.args,)
    out, rec = check_host(code, frame, 0, "a clean frame, code %s" % (code.args,))
    assert out.tobytes() == data.tobytes() and rec.failed == 0 and rec.corrected_bytes == 0 and rec.corrected_bits == 0
    return data, frame


@pytest.mark.parametrize("seed", range(6))
def test_rs_host_against_the_model_on_random_codes(seed):
    """codes drawn over every parameter -- field, fcr, prim, nroots even and odd, n, depth, mask --; per codeword 0, 1, t, t+1, t+2 or
    some other number of errors; what must happen is the model's to say"""
    rng = np.random.default_rng(seed)
    seen = set()
    for it in range(12):
        code = rm.random_code(rng)
        data, frame = check_encoder(code, rng)
        for j in range(code.depth):
            cnt = int(rng.choice([0, 1, code.t, code.t + 1, code.t + 2, int(rng.integers(0, code.t + 1))]))
            rm.corrupt(rng, frame, code, j, min(cnt, code.n))
        model = code.decode(frame, rm.WITH_PARITY)
        for flags in (0, rm.WITH_PARITY):
            out, rec = check_host(code, frame, flags, "seed %d code %s flags %d" % (seed, code.args, flags), model)
            assert out.size == (code.n if flags else code.k) * code.depth and rec.flags == 1 | flags << 1
            seen |= {("failed" if e == rm.FAILED else "ok") for e in rec.n_err[: code.depth]}
            assert all(e == 0 for e in rec.n_err[code.depth:]) and all(b == 0 for b in rec.n_bit[code.depth:])
    assert seen == {"failed", "ok"}


DIRECTED = [(rm.CCSDS, 1), (rm.DVB, 2), ((0x11D, 0, 1, 2, 5), 8), ((0x12D, 254, 254, 3, 70), 7), ((0x1F5, 1, 7, 33, 130), 3), ((0x187, 112, 11, 16, 255), 4),
            ((0x11D, 0, 1, 64, 65), 5), ((0x163, 77, 13, 64, 255), 1), ((0x11D, 0, 1, 16, 64), 6)]


@pytest.mark.parametrize("params,depth", DIRECTED)
def test_rs_host_against_the_model_on_the_directed_cases(params, depth):
    """every depth 1 .. 8 over the codes; the neighbour case must decode to the neighbour with n_err = t and the pad case must fail"""
    rng = np.random.default_rng(depth)
    nd = params[4] * depth
    for q, mlen in enumerate((0, 1, nd - 1, nd)):  # (every mask length)
        code = rm.Code(*params, depth=depth, mask=rng.integers(0, 256, mlen).astype(np.uint8) if mlen else None)
        cases = rm.directed_cases(rng, code)
        labels = [c[0] for c in cases]
        assert ("neighbour" in labels) == (code.nroots % 2 == 0) and ("pad" in labels) == (255 - code.n >= code.t)
        for i, (label, frame) in enumerate(cases):
            if q and label not in ("neighbour", "pad", "clean") and (i + q) % 4:
                continue  # (the full set with no mask, a quarter of it with each of the others)
            j = i % depth
            model = code.decode(frame, rm.WITH_PARITY)
            for flags in (0, rm.WITH_PARITY):
                out, rec = check_host(code, frame, flags, "%s, code %s mask %d flags %d" % (label, code.args, mlen, flags), model)
            if label == "neighbour":
                assert rec.n_err[j] == code.t, label
            elif label == "pad":
                assert rec.n_err[j] == rm.FAILED and rec.n_bit[j] == 0, label
            elif label == "clean":
                assert rec.n_err[j] == 0
            elif label.startswith("one error at"):
                assert rec.n_err[j] == 1
            elif label.startswith("%d errors" % code.t) or label.startswith("1 errors"):
                assert rec.n_err[j] == int(label.split()[0]) and rec.n_bit[j] == rec.n_err[j] * (1 if label.endswith(" 1") else 8)


def test_a_failed_codeword_goes_out_as_received_with_the_mask_taken_off():
    rng = np.random.default_rng(9)
    code = rm.Code(*rm.DVB, depth=2, mask=rng.integers(0, 256, 300).astype(np.uint8))
    data, frame = check_encoder(code, rng)
    rm.corrupt(rng, frame, code, 1, code.t + 1)
    out, rec = check_host(code, frame, rm.WITH_PARITY, "t+1 errors in codeword 1")
    assert list(rec.n_err)[:2] == [0, rm.FAILED] and rec.failed == 1
    received = code.apply_mask(frame).reshape(code.n, 2)
    assert out.reshape(code.n, 2)[:, 1].tobytes() == received[:, 1].tobytes()
    assert out.reshape(code.n, 2)[: code.k, 0].tobytes() == data.reshape(code.k, 2)[:, 0].tobytes()


# ---- refusals of the host entries ------------------------------------------------------------------------------------------------------

BAD_CODES = dict(gfpoly_low=(0xFF, 0, 1, 16, 255, 1), gfpoly_high=(0x200, 0, 1, 16, 255, 1), gfpoly_0x11b=(0x11B, 0, 1, 16, 255, 1),
                 gfpoly_0x11f=(0x11F, 0, 1, 16, 255, 1), gfpoly_even=(0x11C, 0, 1, 16, 255, 1), fcr=(0x11D, 255, 1, 16, 255, 1),
                 prim_0=(0x11D, 0, 0, 16, 255, 1), prim_255=(0x11D, 0, 255, 16, 255, 1), prim_3=(0x11D, 0, 3, 16, 255, 1), prim_85=(0x11D, 0, 85, 16, 255, 1),
                 nroots_1=(0x11D, 0, 1, 1, 255, 1), nroots_0=(0x11D, 0, 1, 0, 255, 1), nroots_65=(0x11D, 0, 1, 65, 255, 1), n_is_nroots=(0x11D, 0, 1, 16, 16, 1),
                 n_256=(0x11D, 0, 1, 16, 256, 1), n_0=(0x11D, 0, 1, 16, 0, 1), depth_0=(0x11D, 0, 1, 16, 255, 0), depth_9=(0x11D, 0, 1, 16, 255, 9),
                 huge=(0x11D, 0, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))


def test_rs_host_and_encoder_bad_arguments():
    L = pl.load()
    buf, out, mask = np.zeros(255 * 8, np.uint8), np.zeros(255 * 8, np.uint8), np.zeros(255 * 8, np.uint8)
    rec = pl.RsRecord()

    def frame(in_p=buf.ctypes.data, out_p=out.ctypes.data, code=1, flags=0, pad=(0, 0)):
        return pl.RsIn(in_p, out_p, code, flags, (ctypes.c_uint32 * 2)(*pad))

    def host(args, k, mask_p=None, mask_len=0, r=rec):
        return L.psk_soft_rs_host(*args, mask_p, mask_len, ctypes.byref(k) if k is not None else None, ctypes.byref(r) if r is not None else None)

    def encode(args, mask_p=None, mask_len=0, data_p=buf.ctypes.data, out_p=out.ctypes.data):
        return L.psk_soft_rs_encode_host(*args, mask_p, mask_len, data_p, out_p)

    good = (0x11D, 0, 1, 16, 204, 2)
    assert host(good, frame()) == 0 and encode(good) == 0
    for name, args in BAD_CODES.items():
        assert host(args, frame()) == 1, name
        assert encode(args) == 1, name
    # the mask: longer than the frame, or null with a length
    assert host(good, frame(), mask.ctypes.data, 408) == 0 and host(good, frame(), mask.ctypes.data, 409) == 1 and host(good, frame(), None, 1) == 1
    assert encode(good, mask.ctypes.data, 408) == 0 and encode(good, mask.ctypes.data, 409) == 1 and encode(good, None, 1) == 1
    assert encode(good, data_p=None) == 1 and encode(good, out_p=None) == 1
    for k in (frame(flags=2), frame(flags=0x80000000), frame(pad=(1, 0)), frame(pad=(0, 1)), frame(out_p=0)):
        assert host(good, k) == 1
    assert host(good, None) == 1 and host(good, frame(), r=None) == 1
    # a skipped frame gives the zero record and writes nothing
    out[:] = 9
    for k in (frame(code=0), frame(in_p=0), frame(code=0, flags=99, pad=(3, 3), out_p=0)):
        rec.flags = 5
        assert host(good, k) == 0 and bytes(rec) == bytes(64)
    assert (out == 9).all()


# ---- the entry on a control-plane-only handle --------------------------------------------------------------------------------------------

def _dry(nch=4):
    h = pl.Handle(nch, device=pl.DEVICE_NONE)
    h.rs_define(0, *rm.CCSDS, depth=5)
    h.rs_define(15, 0x11D, 0, 1, 3, 70, 8)
    h.rs_define(3, *rm.DVB, depth=1, mask=np.arange(204, dtype=np.uint8))
    return h


def _in(in_=0x10000, out=0x20000, code=1, flags=0, pad=(0, 0)):
    return pl.RsIn(in_, out, code, flags, (ctypes.c_uint32 * 2)(*pad))


def test_the_planned_records():
    h = _dry()
    L = pl.load()
    arr = (pl.RsRecord * 7)()
    assert L.psk_soft_get_rs(h._h, 0, 1, arr) == 1  # (no call yet)
    h.rs_device([_in(), _in(code=16, flags=1, in_=0x10001, out=0x20003), _in(code=0), _in(in_=0), _in(code=4), (0x10000, 0x20000, 4, 1)])
    r = h.get_rs(0, 6)
    want = np.zeros(6, rm.RECORD_DTYPE)
    for i, (n, k, depth, nroots, fl) in {0: (255, 223, 5, 32, 128), 1: (70, 67, 8, 3, 128 | 2), 4: (204, 188, 1, 16, 128), 5: (204, 188, 1, 16, 128 | 2)}.items():
        want[i]["n"], want[i]["k"], want[i]["depth"], want[i]["nroots"], want[i]["flags"] = n, k, depth, nroots, fl
    assert bytes(r) == want.tobytes()
    assert bytes(h.get_rs(5, 1)) == want[5].tobytes()
    assert L.psk_soft_get_rs(h._h, 0, 7, arr) == 1 and L.psk_soft_get_rs(h._h, 6, 1, arr) == 1 and L.psk_soft_get_rs(h._h, 0, 0, arr) == 1
    assert L.psk_soft_get_rs(h._h, 0, 1, None) == 1 and L.psk_soft_get_rs(None, 0, 1, arr) == 1
    # the records are the LAST call's
    h.rs_device([_in(code=4)])
    assert h.get_rs(0, 1)[0].n == 204 and L.psk_soft_get_rs(h._h, 1, 1, arr) == 1
    h.close()


def test_every_refusal_leaves_everything_as_it_was():
    h = _dry()
    L = pl.load()
    h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=50, phaseAvg=50)
    h.rs_device([_in(), _in(code=4), _in(code=16)])
    before = bytes(h.get_rs(0, 3))
    blob, stats, peek = [h.export_state(c) for c in range(4)], h.stats(), [h.peek(c) for c in range(4)]
    good = _in()
    bad = dict(slot_above_15=_in(code=17), slot_never_defined=_in(code=2), slot_huge=_in(code=0xFFFFFFFF), unknown_flags=_in(flags=2),
               high_flag=_in(flags=0x80000000), pad0=_in(pad=(1, 0)), pad1=_in(pad=(0, 7)), null_out=_in(out=0))
    for name, k in bad.items():
        for place in (0, 2):  # (first and last of the call)
            ins = [good, good, good]
            ins[place] = k
            with pytest.raises(pl.PskSoftError) as e:
                h.rs_device(ins)
            assert e.value.status == 1, name
            assert bytes(h.get_rs(0, 3)) == before, name
    arr = (pl.RsIn * 2)(good, good)
    assert L.psk_soft_rs_device(h._h, 0, arr, None) == 1 and L.psk_soft_rs_device(h._h, (1 << 20) + 1, arr, None) == 1
    assert L.psk_soft_rs_device(h._h, 2, None, None) == 1 and L.psk_soft_rs_device(None, 2, arr, None) == 1
    assert bytes(h.get_rs(0, 3)) == before
    # the codes: every refusal of a definition leaves the slot as it was (slot 1 undefined, slot 0 the CCSDS code at depth 5)
    mask = np.zeros(255 * 8, np.uint8)
    assert L.psk_soft_rs_define(h._h, 16, 0x11D, 0, 1, 16, 204, 1, None, 0) == 1 and L.psk_soft_rs_define(None, 1, 0x11D, 0, 1, 16, 204, 1, None, 0) == 1
    for name, args in BAD_CODES.items():
        for slot in (0, 1):
            assert L.psk_soft_rs_define(h._h, slot, *args, None, 0) == 1, name
    for slot in (0, 1):
        assert L.psk_soft_rs_define(h._h, slot, 0x11D, 0, 1, 16, 204, 2, mask.ctypes.data, 409) == 1
        assert L.psk_soft_rs_define(h._h, slot, 0x11D, 0, 1, 16, 204, 2, None, 1) == 1
    with pytest.raises(pl.PskSoftError):
        h.rs_device([_in(code=2)])
    h.rs_device([_in()])
    assert (h.get_rs(0, 1)[0].n, h.get_rs(0, 1)[0].depth) == (255, 5)
    # a redefinition takes: slot 0 as the DVB code with a mask of the whole frame
    assert L.psk_soft_rs_define(h._h, 0, 0x11D, 0, 1, 16, 204, 2, mask.ctypes.data, 408) == 0
    h.rs_device([_in()])
    r = h.get_rs(0, 1)[0]
    assert (r.n, r.k, r.depth, r.nroots, r.flags) == (204, 188, 2, 16, 128)
    # what is wrong on a skipped frame is not looked at
    h.rs_device([_in(code=0, flags=99, pad=(3, 3), out=0), _in(in_=0, out=0, code=40)])
    assert bytes(h.get_rs(0, 2)) == bytes(2 * 64)
    # the control plane has not moved
    assert [h.export_state(c) for c in range(4)] == blob and h.stats() == stats
    assert [h.peek(c) for c in range(4)] == peek
    h.close()


def test_the_binding_sums_what_the_record_leaves_out():
    r = pl.RsRecord()
    r.depth = 4
    for j, (e, b) in enumerate(((0, 0), (3, 11), (255, 0), (16, 70))):
        r.n_err[j], r.n_bit[j] = e, b
    assert (r.failed, r.corrected_bytes, r.corrected_bits) == (1, 19, 81)
    assert math.gcd(11, 255) == 1
