"""psk_soft_viterbi_device without a GPU: the exports and the layouts, the host-side definition (psk_soft_viterbi_host) against
tests/viterbi_model.py byte for byte, the brute-force maximum for tiny frames, ties, the metric bound at 65536 steps, the count
and the encoder, the entry on control-plane-only handles (PSK_SOFT_DEVICE_NONE) -- it checks, then leaves planned records and
nothing else --, and what the pass is for: convolutionally coded payloads behind the words found in the soft symbols of the
reference (the oracle), demapped to int8 LLRs and decoded to the bits that were sent."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import demap_model as dm
from tests import sync_model as sm
from tests import viterbi_model as vm

F32 = np.float32
NEW = ("psk_soft_viterbi_define", "psk_soft_viterbi_device", "psk_soft_get_viterbi", "psk_soft_viterbi_host", "psk_soft_viterbi_encode_host",
       "psk_soft_viterbi_count", "psk_soft_viterbi_bytes", "psk_soft_viterbi_in_bytes")
G7 = vm.CODES[(7, 2)]
ALL_FLAGS = tuple(range(8))


def test_the_symbols_are_exported_and_the_records_have_their_layout():
    L = pl.load()
    for name in NEW:
        assert name in pl.EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    assert len(pl.EXPORTS) == 81 + len(NEW) and all(k.startswith("psk_soft_viterbi_") or k == "psk_soft_get_viterbi" for k in NEW)
    R, I = pl.ViterbiRecord, pl.ViterbiIn
    assert ctypes.sizeof(R) == 64 == vm.RECORD_BYTES == L.psk_soft_viterbi_bytes()
    assert ctypes.sizeof(I) == 32 == vm.IN_BYTES == L.psk_soft_viterbi_in_bytes()
    names = ("n_steps", "n_llr", "metric", "sum_abs", "n_flip", "n_zero", "end_state", "start_state", "n_bits", "flags", "pad")
    assert [getattr(R, k).offset for k in names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56]
    assert [vm.RECORD_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56]
    names = ("llr", "out", "n_steps", "code", "flags", "pad")
    assert [getattr(I, k).offset for k in names] == [0, 8, 16, 20, 24, 28]
    assert (pl.VITERBI_PACKED, pl.VITERBI_TERMINATED, pl.VITERBI_ANY_START) == (1, 2, 4) == (vm.PACKED, vm.TERMINATED, vm.ANY_START)
    assert (pl.VITERBI_DATA, pl.VITERBI_PLANNED) == (1, 128) == (vm.DATA, vm.PLANNED)
    assert (pl.VITERBI_REC_PACKED, pl.VITERBI_REC_TERMINATED, pl.VITERBI_REC_ANY_START) == (2, 4, 8)
    assert (pl.VITERBI_SLOTS, pl.VITERBI_MAX_FRAMES, pl.VITERBI_MAX_STEPS) == (16, 1 << 20, 65536) and vm.MAX_STEPS == 65536


# ---- the definition ----------------------------------------------------------------------------------------------------------

def check_host(K, g, P, keep, llr, n_steps, flags, ctx):
    out, rec = pl.viterbi_host(K, g, P, keep, llr, n_steps, flags)
    mout, mrec = vm.decode(K, g, P, keep, llr, n_steps, flags)
    assert out.dtype == mout.dtype and out.tobytes() == mout.tobytes(), ctx + ": output"
    vm.assert_same(rec, mrec, ctx)
    return out, rec


def noisy_llrs(rng, K, g, P, keep, n_steps, terminated, sigma=0.8, scale=24.0):
    """(the input bits, int8 LLRs of their code bits behind Gaussian noise)"""
    u = rng.integers(0, 2, n_steps).astype(np.uint8)
    if terminated and n_steps >= K - 1:
        u[n_steps - (K - 1):] = 0
    c = vm.encode(K, g, P, keep, u)
    y = (1.0 - 2.0 * c) + sigma * rng.standard_normal(c.size)
    return u, np.clip(np.rint(y * scale), -127, 127).astype(np.int8)


@pytest.mark.parametrize("K", (3, 4, 5, 6, 7))
@pytest.mark.parametrize("n", (2, 3, 4))
def test_viterbi_host_against_the_model_every_code_and_flag(K, n):
    g = vm.CODES[(K, n)]
    rng = np.random.default_rng(100 * K + n)
    for flags in ALL_FLAGS:
        for T in (K - 1, K, 9, 67, 130):
            u, llr = noisy_llrs(rng, K, g, 1, (1 << n) - 1, T, flags & vm.TERMINATED)
            out, rec = check_host(K, g, 1, (1 << n) - 1, llr, T, flags, "K %d n %d flags %d T %d" % (K, n, flags, T))
            assert rec.n_llr == n * T and rec.flags == 1 | flags << 1
            if not flags & vm.ANY_START:
                assert rec.start_state == 0 and rec.metric <= rec.sum_abs and (rec.metric == rec.sum_abs) == (rec.n_flip == 0)
    # a terminated frame shorter than its tail is refused; K-2 steps without the flag decode
    with pytest.raises(pl.PskSoftError):
        pl.viterbi_host(K, g, 1, (1 << n) - 1, np.zeros(64, np.int8), K - 2, vm.TERMINATED)
    if K > 3:
        check_host(K, g, 1, (1 << n) - 1, vm.tie_llrs(rng, 64), K - 2, 0, "K-2 steps")
    check_host(K, g, 1, (1 << n) - 1, vm.tie_llrs(rng, 64), 1, 0, "one step")


@pytest.mark.parametrize("rate", ("2/3", "3/4", "7/8"))
def test_viterbi_host_against_the_model_punctured(rate):
    P, keep = vm.PUNCTURED[rate]
    rng = np.random.default_rng(P)
    for flags in ALL_FLAGS:
        for T in [6 + k for k in range(P + 1)] + [150 + k for k in range(P)]:  # (a frame ends at every phase of the period)
            u, llr = noisy_llrs(rng, 7, G7, P, keep, T, flags & vm.TERMINATED, sigma=0.5)
            out, rec = check_host(7, G7, P, keep, llr, T, flags, "rate %s flags %d T %d" % (rate, flags, T))
            assert rec.n_llr == vm.count(2, P, keep, T) == pl.viterbi_count(7, G7, P, keep, T)
    # a keep whose first phases carry nothing: frames without any LLR decode (to zeros) and read nothing
    P, keep = 3, 0b110000
    for T in (1, 2, 3, 7):
        out, rec = check_host(7, G7, P, keep, np.array([5, -7, 3, 3, -9, 1], np.int8), T, 0, "sparse keep T %d" % T)
        assert rec.n_llr == 2 * (T // 3)


@pytest.mark.parametrize("K", (3, 4))
def test_the_decoded_path_has_the_brute_force_maximum(K):
    rng = np.random.default_rng(K)
    for n in (2, 3):
        g = vm.CODES[(K, n)]
        for P, keep in ((1, (1 << n) - 1), (2, ((1 << (2 * n)) - 1) & ~2)):
            for T, flags in ((1, 0), (5, 0), (9, 0), (12, 0), (12, vm.TERMINATED), (8, vm.ANY_START), (7, vm.ANY_START | vm.TERMINATED), (10, vm.TERMINATED)):
                for llr in (rng.integers(-5, 6, n * T).astype(np.int8), vm.tie_llrs(rng, n * T)):
                    out, rec = pl.viterbi_host(K, g, P, keep, llr, T, flags)
                    want = vm.brute_force(K, g, P, keep, llr, T, flags)
                    ctx = (K, n, P, T, flags, llr.tolist())
                    assert rec.metric == want, ctx
                    # the decoded bits, with the tail's zeros, take that path from the start state the record names
                    u = list(out) + [0] * (T - len(out))
                    assert vm.path_metric(K, g, P, keep, llr, u, int(rec.start_state)) == (want, int(rec.end_state)), ctx


def test_ties_and_all_zero_frames():
    rng = np.random.default_rng(7)
    for (K, n), g in vm.CODES.items():
        for flags in ALL_FLAGS:
            T = 40 + K
            check_host(K, g, 1, (1 << n) - 1, vm.tie_llrs(rng, n * T), T, flags, "ties K %d n %d flags %d" % (K, n, flags))
            out, rec = check_host(K, g, 1, (1 << n) - 1, np.zeros(n * T, np.int8), T, flags, "zeros K %d n %d flags %d" % (K, n, flags))
            # every path ties at 0: state 0 wins every first maximum and predecessor 0 every comparison
            assert not out.any() and (rec.end_state, rec.start_state, rec.metric, rec.sum_abs, rec.n_flip, rec.n_zero) == (0, 0, 0, 0, 0, n * T)
    for rate, (P, keep) in vm.PUNCTURED.items():
        for flags in ALL_FLAGS:
            T = 61
            check_host(7, G7, P, keep, vm.tie_llrs(rng, vm.count(2, P, keep, T)), T, flags, "ties %s flags %d" % (rate, flags))


def test_a_noiseless_round_trip_gives_the_bits_back():
    rng = np.random.default_rng(11)
    for (K, n), g in vm.CODES.items():
        for P, keep in ((1, (1 << n) - 1),) + (tuple(vm.PUNCTURED.values()) if (K, n) == (7, 2) else ()):
            T = 300
            u = rng.integers(0, 2, T).astype(np.uint8)
            u[T - (K - 1):] = 0
            c = pl.viterbi_encode(K, g, P, keep, u)
            assert c.tobytes() == vm.encode(K, g, P, keep, u).tobytes()
            llr = np.where(c == 1, -20, 20).astype(np.int8)
            for flags in (vm.TERMINATED, vm.TERMINATED | vm.PACKED):
                out, rec = pl.viterbi_host(K, g, P, keep, llr, T, flags)
                bits = np.unpackbits(out)[: rec.n_bits] if flags & vm.PACKED else out
                assert rec.n_bits == T - (K - 1) and bits.tobytes() == u[: rec.n_bits].tobytes(), (K, n, P)
                assert rec.n_flip == 0 and rec.metric == rec.sum_abs == 20 * c.size and rec.n_zero == 0
                if flags & vm.PACKED and rec.n_bits % 8:
                    assert out[-1] & ((1 << (8 - rec.n_bits % 8)) - 1) == 0  # (the unused low bits of the last byte)


@pytest.mark.parametrize("value", (127, -127, -128))
def test_the_metric_bound_at_65536_steps(value):
    K, n, T = 7, 4, 65536
    g = vm.CODES[(K, n)]
    llr = np.full(n * T, value, np.int8)
    out, rec = pl.viterbi_host(K, g, 1, 15, llr, T, 0)
    assert rec.n_llr == n * T and rec.sum_abs == abs(value) * n * T and rec.n_zero == 0 and rec.start_state == 0
    assert abs(rec.metric) <= 4 * 128 * 65536 < 1 << 26
    if value > 0:
        # every LLR says 0: the all-zero path agrees with all of them
        assert not out.any() and rec.metric == rec.sum_abs and rec.n_flip == 0 and rec.end_state == 0
    else:
        # every LLR says 1.  The path is the best one, so no path does better: the all-ones input, whose code bits are 1 wherever
        # a polynomial has an odd number of taps, is one of them; and the identity metric = sum_abs - 2 |value| n_flip holds
        ones = sum(vm.parity(p) for p in g)
        assert rec.metric >= abs(value) * (2 * ones - n) * (T - K) - abs(value) * n * K
        assert rec.metric == rec.sum_abs - 2 * abs(value) * rec.n_flip
        assert 0 < rec.n_flip < n * T // 2


def test_the_count_is_the_length_of_the_encoders_output():
    for (K, n), g in vm.CODES.items():
        patterns = [(1, (1 << n) - 1), (2, ((1 << (2 * n)) - 1) & ~2), (3, 1 | 1 << (3 * n - 1))]
        if n == 2:
            patterns += list(vm.PUNCTURED.values()) + [(16, 0x9E3779B9), (16, 0x80000000)]
        for P, keep in patterns:
            for T in range(0, 3 * P + 2):
                c = pl.viterbi_encode(K, g, P, keep, np.ones(T, np.uint8))
                assert c.size == pl.viterbi_count(K, g, P, keep, T) == vm.count(n, P, keep, T), (K, n, P, keep, T)
    assert pl.viterbi_count(7, G7, 1, 3, 1 << 40) == 2 << 40
    # patterns the definition refuses have no count
    for P, keep in ((0, 1), (17, 1), (1, 0), (1, 4), (2, 16)):
        assert pl.viterbi_count(7, G7, P, keep, 10) == 0


def test_viterbi_host_and_encoder_bad_arguments():
    L = pl.load()
    llr = np.zeros(64, np.int8)
    bad_codes = ((2, G7[:2], 1, 3), (8, G7, 1, 3), (7, (0o171,), 1, 1), (7, (1, 1, 1, 1, 1), 1, 31), (7, (0o171, 0), 1, 3), (7, (0o171, 0o333), 1, 3),
                 (7, (0o170, 0o132), 1, 3), (7, (0o071, 0o033), 1, 3), (7, G7, 0, 3), (7, G7, 17, 3), (7, (0o171, 0o133, 0o165), 11, 1), (7, G7, 1, 0),
                 (7, G7, 1, 4), (7, G7, 3, 64))
    for K, g, P, keep in bad_codes:
        assert not vm.code_ok(K, g, P, keep), (K, g, P, keep)
        with pytest.raises(pl.PskSoftError) as e:
            pl.viterbi_host(K, g, P, keep, llr, 8, 0)
        assert e.value.status == 1, (K, g, P, keep)
        pol = np.array(g, np.uint32)
        bits, out = np.zeros(8, np.uint8), np.zeros(64, np.uint8)
        assert L.psk_soft_viterbi_encode_host(K, len(g), pol.ctypes.data, P, keep, bits.ctypes.data, 8, out.ctypes.data) == 1
    # taps at bit K-1 and at bit 0 may come from different polynomials
    assert vm.code_ok(7, (0o170, 0o033), 1, 3)
    pl.viterbi_host(7, (0o170, 0o033), 1, 3, llr, 8, 0)
    pol = np.array(G7, np.uint32)
    out = np.zeros(64, np.uint8)
    rec = pl.ViterbiRecord()

    def host(k, g=pol.ctypes.data, r=rec):
        return L.psk_soft_viterbi_host(7, 2, g, 1, 3, ctypes.byref(k) if k is not None else None, ctypes.byref(r) if r is not None else None)

    def frame(llr_p=llr.ctypes.data, out_p=out.ctypes.data, n_steps=8, code=1, flags=0, pad=0):
        return pl.ViterbiIn(llr_p, out_p, n_steps, code, flags, pad)

    assert host(frame()) == 0
    for k in (frame(flags=8), frame(flags=0x80000000), frame(pad=1), frame(out_p=0), frame(n_steps=65537), frame(n_steps=5, flags=vm.TERMINATED)):
        assert host(k) == 1
    assert host(None) == 1 and host(frame(), g=None) == 1 and host(frame(), r=None) == 1
    # a skipped frame gives the zero record and writes nothing
    out[:] = 9
    for k in (frame(n_steps=0), frame(code=0), frame(llr_p=0), frame(n_steps=0, flags=99, pad=3, out_p=0)):
        rec.metric = 5
        assert host(k) == 0 and bytes(rec) == bytes(64)
    assert (out == 9).all()


# ---- the entry on a control-plane-only handle ------------------------------------------------------------------------------------

def _dry(nch=4):
    h = pl.Handle(nch, device=pl.DEVICE_NONE)
    h.viterbi_define(0, 7, G7)
    h.viterbi_define(15, 3, vm.CODES[(3, 3)])
    h.viterbi_define(3, 7, G7, *vm.PUNCTURED["3/4"])
    return h


def _in(llr=0x10000, out=0x20000, n_steps=100, code=1, flags=0, pad=0):
    return pl.ViterbiIn(llr, out, n_steps, code, flags, pad)


def _no_call_yet(h):
    return pl.load().psk_soft_get_viterbi(h._h, 0, 1, (pl.ViterbiRecord * 1)()) == 1


def test_the_planned_records():
    h = _dry()
    assert _no_call_yet(h)
    h.viterbi_device([_in(), _in(code=16, flags=7, out=0x20001, n_steps=7), _in(n_steps=0), _in(code=0), _in(llr=0), _in(code=4, flags=vm.TERMINATED, llr=0x10003)])
    r = h.viterbi_records(0, 6)
    want = np.zeros(6, vm.RECORD_DTYPE)
    for k, (T, n_llr, n_bits, fl) in {0: (100, 200, 100, 128), 1: (7, 21, 5, 128 | 14), 5: (100, 134, 94, 128 | 4)}.items():
        want[k]["n_steps"], want[k]["n_llr"], want[k]["n_bits"], want[k]["flags"] = T, n_llr, n_bits, fl
    assert bytes(r) == want.tobytes()
    assert bytes(h.viterbi_records(5, 1)) == want[5].tobytes()
    L = pl.load()
    arr = (pl.ViterbiRecord * 7)()
    assert L.psk_soft_get_viterbi(h._h, 0, 7, arr) == 1 and L.psk_soft_get_viterbi(h._h, 6, 1, arr) == 1 and L.psk_soft_get_viterbi(h._h, 0, 0, arr) == 1
    assert L.psk_soft_get_viterbi(h._h, 0, 1, None) == 1 and L.psk_soft_get_viterbi(None, 0, 1, arr) == 1
    # the records are the LAST call's
    h.viterbi_device([_in(n_steps=5)])
    assert h.viterbi_records(0, 1)[0].n_steps == 5 and L.psk_soft_get_viterbi(h._h, 1, 1, arr) == 1
    h.close()


def test_every_refusal_leaves_everything_as_it_was():
    h = _dry()
    L = pl.load()
    h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=50, phaseAvg=50)
    h.viterbi_device([_in(), _in(n_steps=33), _in(code=16)])
    before = bytes(h.viterbi_records(0, 3))
    blob, stats, peek = [h.export_state(c) for c in range(4)], h.stats(), [h.peek(c) for c in range(4)]
    good = _in()
    bad = dict(slot_above_15=_in(code=17), slot_never_defined=_in(code=2), unknown_flags=_in(flags=8), high_flag=_in(flags=0x80000000), pad=_in(pad=1),
               null_out=_in(out=0), too_long=_in(n_steps=65537), far_too_long=_in(n_steps=0xFFFFFFFF), short_tail=_in(n_steps=5, flags=vm.TERMINATED),
               short_tail_k3=_in(n_steps=1, code=16, flags=vm.TERMINATED | vm.PACKED))
    for name, k in bad.items():
        for place in (0, 2):  # (first and last of the call)
            ins = [good, good, good]
            ins[place] = k
            with pytest.raises(pl.PskSoftError) as e:
                h.viterbi_device(ins)
            assert e.value.status == 1, name
            assert bytes(h.viterbi_records(0, 3)) == before, name
    h.viterbi_device([_in(n_steps=6, flags=vm.TERMINATED), _in(n_steps=2, code=16, flags=vm.TERMINATED), good])  # (the shortest that pass)
    assert [r.n_bits for r in h.viterbi_records(0, 3)] == [0, 0, 100]
    h.viterbi_device([_in(), _in(n_steps=33), _in(code=16)])
    arr = (pl.ViterbiIn * 2)(good, good)
    assert L.psk_soft_viterbi_device(h._h, 0, arr, None) == 1 and L.psk_soft_viterbi_device(h._h, (1 << 20) + 1, arr, None) == 1
    assert L.psk_soft_viterbi_device(h._h, 2, None, None) == 1 and L.psk_soft_viterbi_device(None, 2, arr, None) == 1
    assert bytes(h.viterbi_records(0, 3)) == before
    # the codes: every refusal of a definition leaves the slot as it was (slot 1 undefined, slot 0 the K = 7 code)
    pol = np.array(G7, np.uint32)
    zero = np.array([0o171, 0], np.uint32)
    for slot, K, n, g, P, keep in ((16, 7, 2, pol, 1, 3), (1, 2, 2, pol, 1, 3), (1, 8, 2, pol, 1, 3), (1, 7, 1, pol, 1, 1), (1, 7, 5, pol, 1, 31), (1, 7, 2, None, 1, 3),
                                   (1, 7, 2, zero, 1, 3), (1, 6, 2, pol, 1, 3), (1, 7, 2, pol, 0, 3), (1, 7, 2, pol, 17, 3), (1, 7, 2, pol, 1, 0), (1, 7, 2, pol, 1, 4),
                                   (0, 3, 2, pol, 1, 3), (0, 7, 2, pol, 2, 16)):
        assert L.psk_soft_viterbi_define(h._h, slot, K, n, g.ctypes.data if g is not None else None, P, keep) == 1
    with pytest.raises(pl.PskSoftError):
        h.viterbi_device([_in(code=2)])
    h.viterbi_device([_in(n_steps=6, flags=vm.TERMINATED)])  # (slot 0 still has K = 7: with K = 3 there would be 4 bits)
    assert h.viterbi_records(0, 1)[0].n_bits == 0
    # a redefinition takes: slot 0 as the K = 3 code
    h.viterbi_define(0, 3, vm.CODES[(3, 3)])
    h.viterbi_device([_in(n_steps=6, flags=vm.TERMINATED)])
    assert (h.viterbi_records(0, 1)[0].n_bits, h.viterbi_records(0, 1)[0].n_llr) == (4, 18)
    # what is wrong on a skipped frame is not looked at
    h.viterbi_device([_in(n_steps=0, flags=99, pad=3, code=40), _in(code=0, out=0), _in(llr=0, out=0, n_steps=1 << 30)])
    assert bytes(h.viterbi_records(0, 3)) == bytes(3 * 64)
    # the control plane has not moved
    assert [h.export_state(c) for c in range(4)] == blob and h.stats() == stats
    assert [h.peek(c) for c in range(4)] == peek
    h.close()


# ---- what the pass is for: coded payloads behind the words of the reference's soft symbols ----------------------------------------

# QPSK, a 32-symbol word every 500 symbols, 8 samples a symbol, as tests/test_sync_control.py builds its streams -- with data of its
# own: behind every word lies a frame of PAYLOAD bits and a tail of 6 zeros, coded with the K = 7 171/133 code and mapped by Gray
# labels, MSB first; the symbols between the frames are random.  (sigma per component, seed); at sigma 0.3 the reference's tracker
# slips a cycle between two frames on some noise draws, and the seed is one on which the twelve hits keep one rotation.
CHAIN_CLEAN, CHAIN_NOISY = (0.1, 21), (0.3, 23)
CHAIN_M, CHAIN_WL, CHAIN_SYMBOLS, CHAIN_FIRST, CHAIN_PERIOD, CHAIN_S = 4, 32, 6200, 137, 500, 8
PAYLOAD = 400
CHAIN_STEPS = PAYLOAD + 6        # trellis steps of a frame
CHAIN_FRAME = CHAIN_STEPS        # QPSK symbols of a frame: two code bits a step, two bits a symbol
CHAIN_SCALE = 16.0               # int8 LLRs: |l| <= 4 sqrt(2) (1 + a few sigma) * 16 stays below 127 at both noise levels
_chain_streams, _chain_runs = {}, {}


def chain_stream(case):
    """(interleaved I/Q, the word as points, the word positions, the payloads, the code bits of the frames) -- built once"""
    if case not in _chain_streams:
        sigma, seed = case
        rng = np.random.default_rng(seed)
        word = rng.integers(0, CHAIN_M, CHAIN_WL)
        data = rng.integers(0, CHAIN_M, CHAIN_SYMBOLS)
        starts = list(range(CHAIN_FIRST, CHAIN_SYMBOLS - CHAIN_WL + 1, CHAIN_PERIOD))
        labels = dm.gray_labels(CHAIN_M)
        point_of = np.argsort(labels)  # the point whose label is v
        payloads, coded = [], []
        for s in starts:
            data[s: s + CHAIN_WL] = word
            if s + CHAIN_WL + CHAIN_FRAME > CHAIN_SYMBOLS:
                continue
            u = np.concatenate([rng.integers(0, 2, PAYLOAD), np.zeros(6, np.int64)]).astype(np.uint8)
            c = vm.encode(7, G7, 1, 3, u)
            data[s + CHAIN_WL: s + CHAIN_WL + CHAIN_FRAME] = point_of[2 * c[0::2] + c[1::2]]
            payloads.append(u[:PAYLOAD]), coded.append(c)
        z = np.repeat(sm.psk_points(CHAIN_M, data), CHAIN_S)
        z = z + sigma * (rng.standard_normal(len(z)) + 1j * rng.standard_normal(len(z)))
        iq = np.empty(2 * len(z), F32)
        iq[0::2], iq[1::2] = z.real, z.imag
        wz = sm.psk_points(CHAIN_M, word)
        w = np.empty(2 * CHAIN_WL, F32)
        w[0::2], w[1::2] = wz.real, wz.imag
        _chain_streams[case] = (iq, w, starts, payloads, coded)
    return _chain_streams[case]


def chain_points():
    pz = sm.psk_points(CHAIN_M, np.arange(CHAIN_M))
    points = np.empty(2 * CHAIN_M, F32)
    points[0::2], points[1::2] = pz.real, pz.imag
    return points, dm.gray_labels(CHAIN_M)


def chain_run(oracle_mod, case):
    """oracle -> sync_host -> demap_gain -> demap_host int8 -> viterbi_host over the twelve frames, computed once: (the soft row, the
    word, the hits, the gains, the LLRs of every frame, the decoded payloads, the records, the payloads sent, the code bits sent)"""
    if case not in _chain_runs:
        iq, w, starts, payloads, coded = chain_stream(case)
        o = oracle_mod.OracleComponent()
        o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = CHAIN_S, CHAIN_M, 50, 50
        soft = oracle_mod.run_stream(o, iq, 0.01, packet_complex=8192)["soft"]
        rec, _ = pl.sync_host(w, 0.7, soft, pl.SYNC_RESTART)
        hits = list(rec.hits[: rec.n_hits])
        found = [s for s in starts if s + CHAIN_WL + CHAIN_FRAME <= soft.size // 2]
        assert [h.pos for h in hits][: len(found)] == found and len(found) == 12 == len(payloads)
        hits = hits[:12]
        points, labels = chain_points()
        Ew = pl.sync_word_energy(w)
        der = [pl.sync_derive(h, CHAIN_M, CHAIN_WL, Ew) for h in hits]
        assert len({d["rotation"] for d in der}) == 1, "a cycle slip: pick another seed"
        gains, llrs, outs, recs = [], [], [], []
        for h, d in zip(hits, der):
            gain = pl.demap_gain(d, CHAIN_M)
            llr, dr = pl.demap_host(points, labels, soft, h.pos + CHAIN_WL, CHAIN_FRAME, gain, CHAIN_SCALE, pl.DEMAP_I8)
            assert dr.n_clip == 0 and llr.size == 2 * CHAIN_STEPS  # (an int8 scale that clips nothing)
            out, vr = pl.viterbi_host(7, G7, 1, 3, llr, CHAIN_STEPS, pl.VITERBI_TERMINATED)
            mout, mvr = vm.decode(7, G7, 1, 3, llr, CHAIN_STEPS, vm.TERMINATED)
            assert out.tobytes() == mout.tobytes()
            vm.assert_same(vr, mvr, "%r frame at %d" % (case, h.pos))
            gains.append(gain), llrs.append(llr), outs.append(out), recs.append(vr)
        _chain_runs[case] = (soft, w, hits, gains, llrs, outs, recs, payloads, coded)
    return _chain_runs[case]


def test_clean_frames_decode_to_the_payloads_that_were_sent(oracle_mod):
    soft, w, hits, gains, llrs, outs, recs, payloads, coded = chain_run(oracle_mod, CHAIN_CLEAN)
    hard = sum(int(((l < 0).astype(np.uint8) != c).sum()) for l, c in zip(llrs, coded))
    print("sigma", CHAIN_CLEAN[0], "hard-decision errors", hard, "of", 12 * 2 * CHAIN_STEPS, "largest |l|", max(int(np.abs(l.astype(int)).max()) for l in llrs))
    assert hard == 0
    for out, r, u in zip(outs, recs, payloads):
        assert r.n_bits == PAYLOAD and out.tobytes() == u.tobytes()
        assert r.n_flip == 0 and r.metric == r.sum_abs and r.end_state == 0 and r.start_state == 0


def test_noisy_frames_decode_with_fewer_errors_than_their_hard_decisions(oracle_mod):
    soft, w, hits, gains, llrs, outs, recs, payloads, coded = chain_run(oracle_mod, CHAIN_NOISY)
    hard = sum(int(((l < 0).astype(np.uint8) != c).sum()) for l, c in zip(llrs, coded))
    decoded = sum(int((out != u).sum()) for out, u in zip(outs, payloads))
    flips = sum(int(r.n_flip) for r in recs)
    print("sigma", CHAIN_NOISY[0], "hard-decision errors", hard, "of", 12 * 2 * CHAIN_STEPS, "decoded payload errors", decoded, "of", 12 * PAYLOAD,
          "n_flip summed", flips)
    assert hard > 0 and decoded < hard
    if decoded == 0:
        # the decoded path is the one that was sent: an LLR disagrees with it exactly where the channel flipped it.  (An LLR of 0 is
        # a hard decision for 0 but no disagreement; the draw has none, which the first assertion says.)
        assert not any((l == 0).any() for l in llrs)
        assert flips == hard
