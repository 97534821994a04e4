"""cap_symbols on control-plane handles (no GPU): one rule for every entry (include/psk_soft_hip.h, psk_soft_output_t).

A call that emits more symbols into a channel than cap_symbols says its rows hold is refused with PSK_SOFT_ERR_CAPACITY when
ANY of the channel's four pointers is non-null -- a row of bits or sampleIndex alone is a row like the others --, a call
whose rows hold exactly n_symbols is accepted, and a channel without rows needs no room.  A refused call changes nothing:
peek, query, the state blob and the statistics of every channel read as before, and the same call with room gives what a
fresh handle gives.

The matrix: the four entries x the planning paths (plan_each: a batch of unlike channels, the short row on a 2-PSK channel
with an odd bits row -- `each` -- and on a samplesPerBaud 1 channel, which has no sampleIndex -- `each_s1`; plan_stamped: 20 channels alike,
the short row once on channel 0, where the stamp's own plan_call refuses, and once on a later channel, where its early-out
leaves for the ordinary path; a call of more than 2^20 symbols, which the library cuts -- the plan of the whole call refuses
before anything is cut) x the 15 non-empty sets of non-null pointers.  The mixed-batch cut in time is not in it: that verdict
comes from the schedule of the launches, which a control-plane handle never chooses (process_round commits behind the plan
pass).  Nothing is dereferenced on such a handle; the addresses are those of real numpy buffers all the same.
On a control-plane handle psk_soft_process_host IS psk_soft_process_device (it hands the call over before its own checks): the
"host" column holds that hand-over, not the capacity check psk_soft_process_host makes on a real handle, which
tests/test_gpu_row_guards.py::test_host_entry_on_a_real_handle holds on a GPU.

Before the rule was one rule, the device entries refused only when soft or phase was among the pointers: the sets {bits},
{sampleIndex} and {bits, sampleIndex} were accepted with a row one symbol short on process_device, _strided and _tuned."""
import ctypes
import itertools

import numpy as np
import pytest

from psk_soft_amd import lib as pl

ERR_CAPACITY = 6
ENTRIES = ("device", "strided", "tuned", "host")
STREAMS = ("soft", "bits", "phase", "sampleIndex")
POINTER_SETS = [s for k in range(1, 5) for s in itertools.combinations(STREAMS, k)]
assert len(POINTER_SETS) == 15
RESULTS = ("ret", "n_symbols", "n_bits", "n_sampleIndex", "sri_pushed", "sri_soft_xdelta", "sri_bits_xdelta", "n_warn")
LONG = (1 << 20) + 37  # symbols of the cut call


class Path:
    """channels, their properties, the complex samples of the warm-up call and of the call under test, the short channel"""

    def __init__(self, name, props, warm, n, short, limits=None):
        self.name, self.props, self.warm, self.n, self.short, self.limits = name, props, warm, n, short, limits or {}
        self.nch = len(props)


_UNLIKE = ((3, 8), (1, 4), (5, 16), (2, 2), (7, 8))
_ALIKE = [dict(samplesPerBaud=4, constelationSize=8, numAvg=10, phaseAvg=20)] * 20
PATHS = {
    # unlike channels (samplesPerBaud 1: no sampleIndex; constelationSize 16: no bits; an odd n_bits): never stamped
    # (samplesPerBaud 1 emits only with numAvg 0: the window it waits for is never pushed, cpp/psk_soft.cpp:445)
    "each": Path("each", [dict(samplesPerBaud=S, constelationSize=M, numAvg=7 * (S > 1), phaseAvg=9) for S, M in _UNLIKE], 700, 1503, 3),
    "each_s1": Path("each_s1", [dict(samplesPerBaud=S, constelationSize=M, numAvg=7 * (S > 1), phaseAvg=9) for S, M in _UNLIKE[:3]], 700, 1503, 1),
    "stamped_first": Path("stamped_first", _ALIKE, 512, 2049, 0),
    "stamped_later": Path("stamped_later", _ALIKE, 512, 2049, 13),
    "cut": Path("cut", [dict(samplesPerBaud=2, constelationSize=4, numAvg=4, phaseAvg=50)] * 2, 64, 2 * LONG, 1),
}


class Call:
    """the arrays of one call over all channels of a path: real buffers behind every pointer"""

    def __init__(self, path, n, first, pointers, caps):
        nch = path.nch
        self.pk, self.out = (pl.Packet * nch)(), (pl.Output * nch)()
        # (one buffer behind all packets and one per stream behind all rows: nothing reads or writes them, and pages of
        # zeros that nobody touches cost nothing.  The packet buffer holds stride 2.
        # A call of n samples emits at most n symbols, whatever cap_symbols claims.)
        self.keep = [np.zeros(4 * n + 16, np.float32), np.zeros(2 * n + 16, np.float32), np.zeros(3 * n + 16, np.int16),
                     np.zeros(n + 16, np.float32), np.zeros(n + 16, np.int16)]
        for i in range(nch):
            p, o = self.pk[i], self.out[i]
            p.data, p.n_floats, p.sri_xdelta, p.sri_mode, p.sriChanged, p.present = self.keep[0].ctypes.data, 2 * n, 0.25, 1, int(first), 1
            for k, s in enumerate(STREAMS):
                setattr(o, s, self.keep[1 + k].ctypes.data if s in pointers else None)
            o.cap_symbols = caps[i]
        self.strides = (ctypes.c_uint64 * nch)(*([2] * nch))
        self.tunes = (pl.Tune * nch)(*[pl.Tune(1 << 40, 1 << 50)] * nch)

    def run(self, h, entry, ch0=0):
        """the status of the call (nothing raised)"""
        L, n = h._L, len(self.pk)
        if entry == "device":
            return L.psk_soft_process_device(h._h, ch0, n, self.pk, self.out, None)
        if entry == "strided":
            return L.psk_soft_process_device_strided(h._h, ch0, n, self.pk, self.strides, self.out, None)
        if entry == "tuned":
            return L.psk_soft_process_device_tuned(h._h, ch0, n, self.pk, self.strides, self.tunes, self.out, None)
        return L.psk_soft_process_host(h._h, ch0, n, self.pk, self.out)

    def results(self):
        return [tuple(getattr(o, k) for k in RESULTS) for o in self.out]


def _handle(path):
    h = pl.Handle(path.nch, device=pl.DEVICE_NONE, **path.limits)
    h.configure(0, path.props)
    return h


def _warm(h, path, entry="device"):
    """a first call with room to spare: windows filled, SRI pushed, the alike channels standing behind one stamp"""
    c = Call(path, path.warm, True, STREAMS, [1 << 40] * path.nch)
    assert c.run(h, entry) == pl.OK
    return c


def _snapshot(h):
    n = h.n_channels
    return ([h.peek(c) for c in range(n)], [tuple(getattr(h.query(c), k) for k in pl.PROP_NAMES) for c in range(n)],
            [h.export_state(c) for c in range(n)], h.channel_stats(), h.stats())


_FRESH = {}


def _fresh(name):
    """what a fresh handle gives for the path's call with room to spare: results per channel, blobs, peeks"""
    if name not in _FRESH:
        path = PATHS[name]
        h = _handle(path)
        _warm(h, path)
        c = Call(path, path.n, False, STREAMS, [1 << 40] * path.nch)
        assert c.run(h, "device") == pl.OK
        _FRESH[name] = (c.results(), _snapshot(h))
        h.close()
    return _FRESH[name]


def test_the_paths_are_the_ones_meant():
    res, _ = _fresh("each")
    n = {k: [r[RESULTS.index(k)] for r in res] for k in ("n_symbols", "n_bits", "n_sampleIndex")}
    assert n["n_sampleIndex"][1] == 0 and n["n_symbols"][1] > 0, "samplesPerBaud 1 emits no sampleIndex"
    assert n["n_bits"][2] == 0 and n["n_symbols"][2] > 0, "constelationSize 16 emits no bits"
    assert n["n_bits"][3] % 2 == 1, "an odd bits row"
    res, _ = _fresh("cut")
    assert res[1][RESULTS.index("n_symbols")] > 1 << 20, "the library cuts this call"
    res, _ = _fresh("stamped_first")
    assert len(set(res)) == 1 and res[0][RESULTS.index("n_symbols")] > 0


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(PATHS))
def test_one_symbol_short_is_refused_and_exactly_enough_accepted(name, entry):
    path = PATHS[name]
    want, fresh_snap = _fresh(name)
    n_sym = [r[RESULTS.index("n_symbols")] for r in want]
    assert n_sym[path.short] > 0
    wrong = []
    for pointers in POINTER_SETS:
        h = _handle(path)
        _warm(h, path, entry)
        before = _snapshot(h)
        caps = list(n_sym)
        caps[path.short] -= 1
        st = Call(path, path.n, False, pointers, caps).run(h, entry)
        if st != ERR_CAPACITY:
            wrong.append("%s: a row one symbol short gives %s" % ("+".join(pointers), pl.STATUS_NAMES.get(st, st)))
            h.close()
            continue
        if _snapshot(h) != before:
            wrong.append("%s: the refused call changed the handle" % "+".join(pointers))
        c = Call(path, path.n, False, pointers, n_sym)
        st = c.run(h, entry)
        if st != pl.OK:
            wrong.append("%s: rows of exactly n_symbols give %s" % ("+".join(pointers), pl.STATUS_NAMES.get(st, st)))
        elif c.results() != want:
            wrong.append("%s: counts / SRI fields differ from a fresh handle's" % "+".join(pointers))
        elif _snapshot(h)[:3] != fresh_snap[:3]:
            wrong.append("%s: state differs from a fresh handle's" % "+".join(pointers))
        h.close()
    assert not wrong, "%s, %s:\n  %s" % (name, entry, "\n  ".join(wrong))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(PATHS))
def test_a_channel_without_rows_needs_no_room(name, entry):
    """all four pointers null and cap_symbols 0: accepted, counted and committed like any other call"""
    path = PATHS[name]
    want, fresh_snap = _fresh(name)
    h = _handle(path)
    _warm(h, path, entry)
    c = Call(path, path.n, False, (), [0] * path.nch)
    assert c.run(h, entry) == pl.OK, pl.load().psk_soft_last_error()
    assert c.results() == want
    assert _snapshot(h)[:3] == fresh_snap[:3]
    h.close()


def test_a_short_row_in_a_covered_range_leaves_the_neighbours_alone():
    """the refused call covers [2, 5) of 7 channels; nothing of the handle moves"""
    props = PATHS["each"].props + PATHS["each"].props[:2]
    whole = Path("whole", props, 700, 1501, 0)
    h = _handle(whole)
    _warm(h, whole)
    before = _snapshot(h)
    part = Path("part", props[2:5], 700, 1501, 1)
    g = _handle(whole)
    _warm(g, whole)
    ok = Call(part, part.n, False, STREAMS, [1 << 40] * 3)
    assert ok.run(g, "device", 2) == pl.OK
    n_sym = [r[RESULTS.index("n_symbols")] for r in ok.results()]
    for pointers in POINTER_SETS:
        caps = list(n_sym)
        caps[1] -= 1
        assert Call(part, part.n, False, pointers, caps).run(h, "device", 2) == ERR_CAPACITY, pointers
        assert _snapshot(h) == before, pointers
    h.close()
    g.close()
