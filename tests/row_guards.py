"""Device rows of exactly n_symbols between guard words.  A plain module: tests/test_row_guards.py
proves it on numpy stand-ins without a GPU, tests/test_gpu_row_guards.py and tests/test_gpu_instantiations.py hand its rows
to psk_soft_process_device on one.

A Layout is one call's memory: an arena per output stream (soft, bits, phase, index) and one for the packets.  Every
channel has a row in every arena, `cap_symbols = n_symbols` long -- the counts come from a control-plane handle driven with
the same properties and packets (Planner) --, GUARD bytes in front of it and GUARD bytes behind it, the guard behind starting
at the row's last byte + 1 whatever that address is.  Even channels start at the least alignment the ABI asks for and no
more (soft 8 bytes past a 16-byte boundary, the others 4 bytes past an 8-byte one), odd channels on a 128-byte boundary.  A
stream that emits nothing for a channel, and one the call passes a null pointer for, keeps its place and its guards.

The arenas are filled with GUARD_BYTE, the rows with ROW_BYTE; packets lie in their arena as they are.  check() reads the
arenas as they are after the call: every byte outside the rows must still be GUARD_BYTE, every byte of a row the call had no
pointer for ROW_BYTE, a row it had a pointer for must not be ROW_BYTE from end to end, and the packet arena must be the one
uploaded, byte for byte."""
import numpy as np

GUARD = 1024  # bytes: one wave's soft output for one block (64 lanes x 2 symbols x 8 bytes)
GUARD_BYTE, ROW_BYTE = 0xA5, 0x3C
STREAMS = ("soft", "bits", "phase", "index")
DTYPE = dict(soft=np.float32, bits=np.int16, phase=np.float32, index=np.int16)
MIN_ALIGN = dict(soft=8, bits=4, phase=4, index=4)
FIELD = dict(soft="soft", bits="bits", phase="phase", index="sampleIndex")
FORMAT_ALIGN = {0: 8, 1: 4, 3: 2, 4: 4}  # Packet.format: bytes of a complex sample
FORMAT_OF = {np.dtype(np.float32): 0, np.dtype(np.int16): 1, np.dtype(np.int8): 3, np.dtype(np.float16): 4}
REPORTED = 6  # changed bytes named per row
LINE = 128
NULL_SETS = ((), ("soft",), ("bits",), ("phase",), ("index",), ("soft", "phase"), ("soft", "phase", "index"), STREAMS)
"""the streams a channel's call leaves out, cycled over the channels of a batch: none, each single one, all but bits, all but
bits and sampleIndex, all four (cap_symbols 0)"""


def row_bytes(stream, counts):
    """bytes of a channel's row: counts = dict(n_symbols, n_bits, n_sampleIndex)"""
    return {"soft": 8 * counts["n_symbols"], "phase": 4 * counts["n_symbols"], "bits": 2 * counts["n_bits"],
            "index": 2 * counts["n_sampleIndex"]}[stream]


def _start(cursor, align, bare):
    """the first address >= cursor on a LINE boundary (not bare), or `align` bytes past a 2 * align boundary (bare)"""
    if not bare:
        return -(-cursor // LINE) * LINE
    return -(-(cursor - align) // (2 * align)) * (2 * align) + align


class Row:
    def __init__(self, channel, stream, start, nbytes, present):
        self.channel, self.stream, self.start, self.nbytes, self.present = channel, stream, start, nbytes, present

    end = property(lambda self: self.start + self.nbytes)


class Arena:
    """offsets are relative to a base on a LINE boundary"""

    def __init__(self, name):
        self.name, self.rows, self.size = name, [], 0

    def add(self, channel, nbytes, align, bare, present=True):
        r = Row(channel, self.name, _start(self.size + GUARD, align, bare), nbytes, present)
        self.rows.append(r)
        self.size = r.end + GUARD
        return r


class Layout:
    """counts: one dict(n_symbols, n_bits, n_sampleIndex) per channel.  absent: per channel the streams the call passes a
    null pointer for (default: none).  packets: per channel None or an array (float32, int16, int8, float16: the format),
    laid out like the rows -- or packet_image = (bytes, [(offset, n_elements, format) or None per channel]): an input arena
    the caller has built, a frame matrix for one, whose every byte outside the packets is their guard."""

    def __init__(self, counts, absent=None, packets=None, packet_image=None, call=0):
        n = len(counts)
        self.call, self.counts = call, counts
        self.absent = [tuple(a) for a in (absent or [()] * n)]
        self.arenas = {s: Arena(s) for s in STREAMS}
        for c in range(n):
            for s in STREAMS:
                self.arenas[s].add(c, row_bytes(s, counts[c]), MIN_ALIGN[s], c % 2 == 0, s not in self.absent[c])
        if packet_image is not None:
            self.packet_bytes = np.frombuffer(bytes(packet_image[0]), np.uint8).copy()
            self.packet_at = list(packet_image[1])
        else:
            a = Arena("packet")
            self.packet_at = []
            for c, p in enumerate(packets):
                if p is None:
                    self.packet_at.append(None)
                    continue
                p = np.ascontiguousarray(p)
                fmt = FORMAT_OF[p.dtype]
                self.packet_at.append((a.add(c, p.nbytes, FORMAT_ALIGN[fmt], c % 2 == 0).start, p.size, fmt))
            self.packet_bytes = np.full(max(a.size, 2 * GUARD), GUARD_BYTE, np.uint8)
            for c, p in enumerate(packets):
                if p is not None and p.size:
                    off = self.packet_at[c][0]
                    self.packet_bytes[off : off + p.nbytes] = np.ascontiguousarray(p).view(np.uint8).reshape(-1)

    def images(self):
        """the arenas as they go up: {stream: uint8 array}, and "packet" """
        out = {"packet": self.packet_bytes.copy()}
        for s, a in self.arenas.items():
            img = np.full(a.size, GUARD_BYTE, np.uint8)
            for r in a.rows:
                img[r.start : r.end] = ROW_BYTE
            out[s] = img
        return out

    def fill(self, bases, pk, out, sri_changed=False, xdelta=0.01):
        """pointers, lengths and cap_symbols of the call into the ctypes arrays pk / out; bases: {arena: device address}"""
        for s in list(STREAMS) + ["packet"]:
            assert bases[s] % LINE == 0, "arena %s is not on a %d-byte boundary" % (s, LINE)
        for c, cnt in enumerate(self.counts):
            at = self.packet_at[c]
            if at is None:
                pk[c].present = 0
            else:
                pk[c].data, pk[c].n_floats, pk[c].format = bases["packet"] + at[0], at[1], at[2]
                pk[c].sri_xdelta, pk[c].sri_mode, pk[c].sriChanged, pk[c].present = xdelta, 1, int(sri_changed), 1
            for s in STREAMS:
                r = self.arenas[s].rows[c]
                setattr(out[c], FIELD[s], bases[s] + r.start if r.present else None)
            out[c].cap_symbols = cnt["n_symbols"] if len(self.absent[c]) < 4 else 0

    def extract(self, after, c):
        """the four streams of channel c out of the arenas as they are after the call (None: the call had no pointer)"""
        out = {}
        for s in STREAMS:
            r = self.arenas[s].rows[c]
            out[s] = after[s][r.start : r.end].copy().view(DTYPE[s]) if r.present else None
        return out

    def check(self, after):
        """[finding]: dict(call, channel, stream, where, offsets, values, message); empty: every guard, every row without a
        pointer and every packet byte is as it went up"""
        found = []

        def report(r, where, idx, vals, expect, text):
            found.append(dict(call=self.call, channel=r.channel if r else None, stream=r.stream if r else "packet", where=where,
                              offsets=[int(i) for i in idx[:REPORTED]], values=[int(v) for v in vals[:REPORTED]],
                              message="call %d channel %s %s: %d byte(s) changed %s (%s; 0x%02x expected)"
                              % (self.call, r.channel if r else "-", r.stream if r else "packet", len(idx), text,
                                 ", ".join("0x%02x" % v for v in vals[:REPORTED]), expect)))

        for s, a in self.arenas.items():
            img = np.asarray(after[s], np.uint8)
            assert img.size == a.size, (s, img.size, a.size)
            guard = np.ones(a.size, bool)
            for r in a.rows:
                guard[r.start : r.end] = False
            bad = np.nonzero(guard & (img != GUARD_BYTE))[0]
            if bad.size:
                # a changed guard byte belongs to the row it is nearest to: d bytes past the end of the row in front of it
                # (d = 0: the byte at the row's last byte + 1) or d bytes before the start of the row behind it
                starts, ends, n = np.array([r.start for r in a.rows]), np.array([r.end for r in a.rows]), len(a.rows)
                k = np.searchsorted(starts, bad, side="right") - 1
                past = np.where(k >= 0, bad - ends[np.maximum(k, 0)], a.size)
                before = np.where(k + 1 < n, starts[np.minimum(k + 1, n - 1)] - bad, a.size)
                for j in range(n):
                    r = a.rows[j]
                    m = (k == j) & (past < before)
                    if m.any():
                        report(r, "behind", past[m], img[bad[m]], GUARD_BYTE, "behind the row, %d .. %d bytes past its end" % (past[m][0], past[m][-1]))
                    m = (k + 1 == j) & (past >= before)
                    if m.any():
                        report(r, "front", -before[m], img[bad[m]], GUARD_BYTE,
                               "in front of the row, %d .. %d bytes before its start" % (before[m][-1], before[m][0]))
            for r in a.rows:
                row = img[r.start : r.end]
                if not r.present:
                    w = np.nonzero(row != ROW_BYTE)[0]
                    if w.size:
                        report(r, "row", w, row[w], ROW_BYTE, "in the place of a row the call had no pointer for, from byte %d" % w[0])
                elif r.nbytes >= 8 and (row == ROW_BYTE).all():
                    report(r, "unwritten", np.arange(0), row[:0], ROW_BYTE, "-- the row of %d bytes was never written" % r.nbytes)
        img = np.asarray(after["packet"], np.uint8)
        assert img.size == self.packet_bytes.size
        w = np.nonzero(img != self.packet_bytes)[0]
        if w.size:
            found.append(dict(call=self.call, channel=self._packet_channel(int(w[0])), stream="packet", where="packet",
                              offsets=[int(i) for i in w[:REPORTED]], values=[int(v) for v in img[w[:REPORTED]]],
                              message="call %d packet arena: %d byte(s) changed, the first at offset %d (channel %s): 0x%02x, 0x%02x uploaded"
                              % (self.call, w.size, w[0], self._packet_channel(int(w[0])), img[w[0]], self.packet_bytes[w[0]])))
        return found

    def _packet_channel(self, off):
        """the channel whose packet holds the arena offset, or the one whose packet starts nearest"""
        best = None
        for c, at in enumerate(self.packet_at):
            if at is not None and (best is None or abs(at[0] - off) < abs(self.packet_at[best][0] - off)):
                best = c
        return best


def messages(found):
    return [f["message"] for f in found]


# ---- on a GPU -----------------------------------------------------------------------------------------------------------

class Planner:
    """the counts of every call, from a control-plane handle driven like the real one"""

    def __init__(self, n_channels, **limits):
        from psk_soft_amd import lib as pl

        self.h = pl.Handle(n_channels, device=pl.DEVICE_NONE, **limits)

    def counts(self, ch0, packets, sri_changed, xdelta=0.01):
        """packets: None or an array per channel of [ch0, ch0 + len)"""
        plan = [None if p is None else dict(n_floats=int(np.asarray(p).size), xdelta=xdelta, sriChanged=sri_changed,
                                            format=FORMAT_OF[np.asarray(p).dtype]) for p in packets]
        return [{k: int(r[k]) for k in ("n_symbols", "n_bits", "n_sampleIndex")} for r in self.h.plan_only(ch0, plan)]


class DeviceRows:
    """The arenas of a handle's calls in device memory: one upload and one download per arena per call."""

    def __init__(self, h):
        self.h, self.dev, self.calls = h, {}, 0

    def _base(self, name, size):
        have = self.dev.get(name)
        if have is None or have[1] < size:
            if have:
                self.h.device_free(have[0])
            have = self.dev[name] = (self.h.device_alloc(size + size // 2), size + size // 2)
        return have[0]

    def close(self):
        for p, _ in self.dev.values():
            self.h.device_free(p)
        self.dev = {}

    def run(self, layout, ch0=0, sri_changed=False, xdelta=0.01, call=None):
        """One call on the layout's rows.  call(pk, out, bases): the entry (default Handle.process_device at ch0).  Returns
        (one dict of streams per channel as Layout.extract gives them, the findings of Layout.check, the Output array)."""
        from psk_soft_amd import lib as pl

        n = len(layout.counts)
        up = layout.images()
        bases = {name: self._base(name, img.size) for name, img in up.items()}
        for name, img in up.items():
            self.h.upload(bases[name], img)
        pk, out = (pl.Packet * n)(), (pl.Output * n)()
        layout.fill(bases, pk, out, sri_changed, xdelta)
        if call:
            call(pk, out, bases)
        else:
            self.h.process_device(ch0, pk, out)
        self.h.synchronize()
        after = {name: self.h.download(bases[name], (img.size,), np.uint8) for name, img in up.items()}
        self.calls += 1
        for c in range(n):
            for k in ("n_symbols", "n_bits", "n_sampleIndex"):
                assert int(getattr(out[c], k)) == layout.counts[c][k], "channel %d: the call gives %s = %d, the plan %d" % (
                    c, k, getattr(out[c], k), layout.counts[c][k])
        return [layout.extract(after, c) for c in range(n)], layout.check(after), out
