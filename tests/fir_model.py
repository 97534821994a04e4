"""The filtered packet of include/psk_soft_hip.h ("filtered packets") restated in numpy, for the tests of
psk_soft_process_device_filtered and psk_soft_fir_apply.

Output m of a packet of n samples is, re and im separately, acc = h[0] * s[i], then acc = acc + h[j] * s[i-j] for j = 1 .. T-1
in that order, i = pos + m * D: every operation float32 and rounded on its own (one .astype(float32) after each), the loop over
the taps outermost, so every step is one vector operation over all outputs.  s[-127 .. -1] is the history, 127 complex samples
carried from packet to packet whatever the filter's length.  Counts and positions are Python integers."""
import numpy as np

F32 = np.float32
MAX_TAPS, SLOTS, MAX_DECIM = 128, 64, 16
HIST = MAX_TAPS - 1
RESTART = 1
WINDOW = 4096  # inputs of one piece of the device's pass


def count(pos, decim, n):
    """n_out: the m with pos + m * decim < n"""
    pos, decim, n = int(pos), int(decim), int(n)
    return 0 if pos >= n else (n - pos + decim - 1) // decim


def advance(pos, decim, n):
    """pos of the next packet: pos + n_out * decim - n"""
    return int(pos) + count(pos, decim, n) * int(decim) - int(n)


def piece(decim):
    """outputs of one piece of the device's pass at that decimation: (4096 - 128) / D, rounded down to even"""
    return ((WINDOW - MAX_TAPS) // int(decim)) & ~1


def apply(taps, decim, pos, iq, history=None, restart=False):
    """taps: 1 .. 128 floats; iq: interleaved I/Q, already float32-exact samples s[0 .. n-1] (an odd last element is dropped; any
    packet dtype: the conversion is exact).  history: 254 floats (127 complex samples, oldest first) or None for zeros;
    restart: zeros whatever `history` says.  Returns (interleaved float32 I/Q of the n_out outputs, the history behind the
    packet as 254 float32)."""
    h = np.asarray(taps, F32).reshape(-1)
    assert 1 <= h.size <= MAX_TAPS and 1 <= decim <= MAX_DECIM and 0 <= pos < decim
    x = np.asarray(iq)
    n = x.size // 2
    x = x[: 2 * n].astype(F32)
    hist = np.zeros(2 * HIST, F32) if history is None or restart else np.asarray(history, F32).copy()
    assert hist.size == 2 * HIST
    ext = np.concatenate([hist, x])  # ext[2 * (j + 127)] = re s[j]
    n_out = count(pos, decim, n)
    y = np.empty(2 * n_out, F32)
    if n_out:
        i = int(pos) + np.arange(n_out, dtype=np.int64) * int(decim) + HIST  # (index of s[i_m] in ext, in samples)
        with np.errstate(all="ignore"):
            for q in (0, 1):
                comp = ext[q::2]
                acc = (h[0] * comp[i]).astype(F32)
                for j in range(1, h.size):
                    acc = (acc + (h[j] * comp[i - j]).astype(F32)).astype(F32)
                y[q::2] = acc
    return y, ext[-2 * HIST:].copy()


class Stream:
    """a channel's filter carried from packet to packet: pos and the history (the taps and the decimation may change)"""

    def __init__(self, pos=0, history=None):
        self.pos = int(pos)
        self.history = np.zeros(2 * HIST, F32) if history is None else np.asarray(history, F32).copy()

    def push(self, taps, decim, iq, restart=False):
        """one packet through: returns its outputs; pos and the history move on"""
        n = np.asarray(iq).size // 2
        y, self.history = apply(taps, decim, self.pos, iq, self.history, restart)
        self.pos = advance(self.pos, decim, n)
        return y
