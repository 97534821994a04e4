"""The resampled packet of include/psk_soft_hip.h ("resampled packets") restated in numpy, for the tests of
psk_soft_process_device_resampled and psk_soft_resample_apply.

pos and step are integers in input samples x 2^32.  The output instants t_m = pos + m * step (uint64) run while t_m < n * 2^32;
an output is the cubic Lagrange polynomial through s[i-3] .. s[i], i = t_m >> 32, evaluated mu = the top 24 bits of t_m's
fraction behind s[i-2]: every operation float32 and rounded on its own (.astype(float32) after each).  s[-3 .. -1] is the
history, three complex samples carried from packet to packet."""
import math

import numpy as np

F32 = np.float32
ONE = 1 << 32
RESTART = 1
W0, W3 = F32(-1.0 / 6.0), F32(1.0 / 6.0)
HALF = F32(0.5)


def count(pos, step, n):
    """n_out: the m with pos + m * step < n * 2^32 (big-integer arithmetic)"""
    end = int(n) << 32
    return 0 if pos >= end else (end - int(pos) + int(step) - 1) // int(step)


def advance(pos, step, n):
    """pos of the next packet: pos + n_out * step - n * 2^32"""
    return int(pos) + count(pos, step, n) * int(step) - (int(n) << 32)


def step_word(in_per_out):
    """psk_soft_resample_step restated: (r * 2^32) truncated; 0 for a non-finite value or one outside [0.5, 2]"""
    r = float(in_per_out)
    if not math.isfinite(r) or r < 0.5 or r > 2.0:
        return 0
    return int(r * 4294967296.0)  # (exact: a power of two)


def taps(frac):
    """the four weights for the fractions `frac` (uint64 array, the low 32 bits of the instants), float32 arrays"""
    a = ((frac >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)  # (24 bits: exact)
    b, c, d = (a - F32(1)).astype(F32), (a - F32(2)).astype(F32), (a + F32(1)).astype(F32)
    w0 = (((a * b).astype(F32) * c).astype(F32) * W0).astype(F32)
    w1 = (((d * b).astype(F32) * c).astype(F32) * HALF).astype(F32)
    w2 = (((d * a).astype(F32) * c).astype(F32) * -HALF).astype(F32)
    w3 = (((d * a).astype(F32) * b).astype(F32) * W3).astype(F32)
    return w0, w1, w2, w3


def apply(pos, step, iq, history=None, restart=False):
    """iq: interleaved I/Q, already float32-exact samples s[0 .. n-1] (an odd last element is dropped; any packet dtype: the
    conversion is exact).  history: six floats (three complex samples, oldest first) or None for zeros; restart: zeros whatever
    `history` says.  Returns (interleaved float32 I/Q of the n_out outputs, the history behind the packet as six float32)."""
    x = np.asarray(iq)
    n = x.size // 2
    x = x[: 2 * n].astype(F32)
    h = np.zeros(6, F32) if history is None or restart else np.asarray(history, F32).copy()
    assert h.size == 6
    ext = np.concatenate([h, x])  # ext[2 * (j + 3)] = re s[j]
    n_out = count(pos, step, n)
    y = np.empty(2 * n_out, F32)
    if n_out:
        with np.errstate(over="ignore"):
            t = (np.uint64(pos) + np.arange(n_out, dtype=np.uint64) * np.uint64(step)).astype(np.uint64)
        i = (t >> np.uint64(32)).astype(np.int64)
        w0, w1, w2, w3 = taps(t & np.uint64(0xFFFFFFFF))
        with np.errstate(all="ignore"):
            for q in (0, 1):
                s0, s1, s2, s3 = (ext[2 * (i + k) + q] for k in range(4))  # s[i-3 .. i]
                acc = ((w0 * s0).astype(F32) + (w1 * s1).astype(F32)).astype(F32)
                acc = (acc + (w2 * s2).astype(F32)).astype(F32)
                y[q::2] = (acc + (w3 * s3).astype(F32)).astype(F32)
    return y, ext[-6:].copy()


class Stream:
    """a channel's resampler carried from packet to packet: pos, step and the history"""

    def __init__(self, step, pos=0, history=None):
        self.step, self.pos = int(step), int(pos)
        self.history = np.zeros(6, F32) if history is None else np.asarray(history, F32).copy()

    def push(self, iq, restart=False):
        """one packet through: returns its outputs; pos and the history move on"""
        n = np.asarray(iq).size // 2
        y, self.history = apply(self.pos, self.step, iq, self.history, restart)
        self.pos = advance(self.pos, self.step, n)
        return y
