#!/usr/bin/env python3
"""sync_rates.py -- what the word search of psk_soft_sync_device costs on one MI355X, next to the demodulator call that produced the
rows it searches and to the filter pass at the same number of taps: everything resident in HBM, everything on ONE stream, every step
between two HIP events on that stream, medians over --steps steps after --warmup.

One shape, --channels x --symbols soft symbols a channel (4096 x 32768), QPSK, samplesPerBaud 8, sc16 packets (int8 values):

  t_process   psk_soft_process_device of the packets: --symbols x 8 samples a channel in, the four rows out
  t_sync      per word length L (16, 32, 64, 128): psk_soft_sync_device over the soft rows of that call, a continuing row (as many
              windows as symbols), with windows and multiply-adds (L a window, four real ones each) per second
  t_fir       per L: the filter pre-pass alone (PSK_SOFT_DIAG_GATHER_ONLY) with L taps, decimation 1, over the same rows read as
              CF32 packets -- as many outputs as the search has windows, two real multiply-adds a tap

The records of a few channels of a restarted search are checked against psk_soft_sync_host on the downloaded rows, byte for byte.
One JSON object on stdout (and in --out).

    python tools/sync_rates.py [--steps 10] [--warmup 3] [--channels 4096] [--symbols 32768] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cs16_rates import A, M, NPH, S, packets  # noqa: E402
from cs8_rates import quantise_torch  # noqa: E402
from fir_rates import taps_of  # noqa: E402
from strided_rates import Outs, timed  # noqa: E402

WORD_LENGTHS = (16, 32, 64, 128)
THRESHOLD = 0.8


def sync_ins(pl, out, C, slot, flags):
    return (pl.SyncIn * C)(*[pl.SyncIn(out[c].soft, out[c].n_symbols, slot + 1, flags, THRESHOLD, 0) for c in range(C)])


def host_check(pl, np, h, o, words, channels, raw):
    """the records of `channels` behind a restarted search of every word against psk_soft_sync_host of the downloaded rows"""
    for slot, w in enumerate(words):
        C = len(o.out)
        h.sync_device(0, sync_ins(pl, o.out, C, slot, pl.SYNC_RESTART), raw)
        for c in channels:
            n = int(o.out[c].n_symbols)
            x = o.soft[c, : 2 * n].cpu().numpy()
            want, hist = pl.sync_host(w, THRESHOLD, x, pl.SYNC_RESTART)
            if bytes(h.sync_records(c, 1)[0]) != bytes(want) or h.sync_history(c).tobytes() != hist.tobytes():
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--symbols", type=int, default=32768)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("sync_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    C, N = args.channels, args.symbols * S
    result = {"tool": "sync_rates", "device": torch.cuda.get_device_name(0), "scale": 40.0, "piece_windows": pl.sync_piece(),
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH), "steps": args.steps, "warmup": args.warmup,
              "threshold": THRESHOLD, "timing": "HIP events on one stream around every step; medians", "shape": [C, args.symbols]}
    data = quantise_torch(synth_channels_torch(C, M, S, N, dev)).to(torch.int16).contiguous()
    row = data.stride(0) * data.element_size()
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    cap = (N // S + 2 + 63) // 64 * 64
    h = pl.Handle(C, device=0)
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
    pk0 = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, pl.FORMAT_CS16, True)
    pk = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, pl.FORMAT_CS16, False)
    o = Outs(pl, torch, C, cap, dev)
    h.process_device(0, pk0, o.out, raw)
    h.synchronize()
    result["t_process"] = timed(torch, st, lambda: h.process_device(0, pk, o.out, raw), args.steps, args.warmup)
    h.synchronize()
    n_sym = [int(o.out[c].n_symbols) for c in range(C)]
    result["symbols_per_channel"] = [min(n_sym), max(n_sym)]
    # the words: unit QPSK points on the diagonals, random, one slot per length
    rng = np.random.default_rng(1)
    words = []
    for slot, L in enumerate(WORD_LENGTHS):
        z = np.exp(2j * np.pi * (rng.integers(0, 4, L) / 4 + 0.125))
        w = np.empty(2 * L, np.float32)
        w[0::2], w[1::2] = z.real, z.imag
        words.append(w)
        h.sync_define(slot, w)
    result["records_equal_host"] = host_check(pl, np, h, o, words, sorted({0, 1, C // 2, C - 1}), raw)
    result["t_sync"] = {}
    windows = sum(n_sym)
    for slot, L in enumerate(WORD_LENGTHS):
        ins = sync_ins(pl, o.out, C, slot, 0)
        r = timed(torch, st, lambda: h.sync_device(0, ins, raw), args.steps, args.warmup)
        sec = r["median_ms"] * 1e-3
        r.update(word_len=L, windows=windows, windows_per_s=windows / sec, gmac_per_s=4.0 * L * windows / sec / 1e9,
                 bytes_read=8 * windows, over_process=r["median_ms"] / result["t_process"]["median_ms"])
        result["t_sync"]["L%d" % L] = r
    h.synchronize()
    # the filter pass alone over the same rows, as many taps as the word has points
    os.environ["PSK_SOFT_DIAG_GATHER_ONLY"] = "1"
    g = pl.Handle(C, device=0)
    os.environ.pop("PSK_SOFT_DIAG_GATHER_ONLY")
    g.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
    fpk = packets(pl, C, lambda c: o.soft[c].data_ptr(), 0, pl.FORMAT_CF32, False)
    for c in range(C):
        fpk[c].n_floats = 2 * n_sym[c]
    outs = (pl.Output * C)()  # (never looked at: the ordinary call is left out)
    result["t_fir"] = {}
    for slot, L in enumerate(WORD_LENGTHS):
        g.fir_define(slot, taps_of(L))
        firs = (pl.Fir * C)(*[pl.Fir(1 + slot, 1, 0, 0) for _ in range(C)])
        r = timed(torch, st, lambda: g.process_device_filtered(0, fpk, None, None, firs, None, outs, raw), args.steps, args.warmup)
        r.update(taps=L, outputs=windows, gmac_per_s=2.0 * L * windows / (r["median_ms"] * 1e-3) / 1e9)
        result["t_fir"]["L%d" % L] = r
        result["t_sync"]["L%d" % L]["over_fir"] = result["t_sync"]["L%d" % L]["median_ms"] / r["median_ms"]
    g.synchronize()
    g.close()
    h.close()
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if result["records_equal_host"] else 1


if __name__ == "__main__":
    sys.exit(main())
