#!/usr/bin/env python3
"""demap_rates.py -- what psk_soft_demap_device costs on one MI355X, next to the demodulator call that wrote the rows it reads and
to a device-to-device copy that moves the same number of bytes: everything resident in HBM, everything on ONE stream, every step
between two HIP events on that stream, medians over --steps steps after --warmup.

One shape, --channels x --symbols soft symbols a channel (4096 x 32768), QPSK, samplesPerBaud 8, sc16 packets (int8 values):

  t_process   psk_soft_process_device of the packets: --symbols x 8 samples a channel in, the four rows out
  t_demap     per M (4, 8), output form (i8, f32) and cut -- "row": one segment a row; "frames": frames of 512 symbols, each a
              segment of its own, 64 a row --: psk_soft_demap_device over the soft rows of that call (the same rows for both M:
              the values do not matter to the time), with symbols per second and bytes per second (8 read, B or 4 B written a
              symbol).  The time is the stream's: it holds the entry's own host work (one 64-byte descriptor a segment, checked,
              filled in and copied up) wherever the stream waits for it; t_host is the call's wall time on the host
  t_copy      per M and form: one torch copy of (bytes read + bytes written) / 2 bytes, which reads and writes as many bytes
              in all as the demap call

The values and the records of a few segments are checked against psk_soft_demap_host on the downloaded rows, byte for byte.
One JSON object on stdout (and in --out).

    python tools/demap_rates.py [--steps 10] [--warmup 3] [--channels 4096] [--symbols 32768] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cs16_rates import A, M, NPH, S, packets  # noqa: E402
from cs8_rates import quantise_torch  # noqa: E402
from strided_rates import Outs, timed  # noqa: E402

FRAME = 512
GAIN, SCALE = (0.8, -0.6), 16.0
SLOTS = {4: 0, 8: 1}


def the_map(np, Mc):
    """Gray labels on unit points: QPSK on the diagonals, 8-PSK from the real axis"""
    z = np.exp(2j * np.pi * (np.arange(Mc) / Mc + (0.125 if Mc == 4 else 0.0)))
    p = np.empty(2 * Mc, np.float32)
    p[0::2], p[1::2] = z.real, z.imag
    return p, np.array([k ^ (k >> 1) for k in range(Mc)], np.uint8)


def segments(pl, o, n_sym, out_ptr, Mc, i8, frames):
    """the DemapIn table: a row as one segment, or as frames of FRAME symbols; the values of a row abut in its part of `out`"""
    B = {4: 2, 8: 3}[Mc]
    item = 1 if i8 else 4
    rows = []
    at = 0
    for c, n in enumerate(n_sym):
        cuts = [(k * FRAME, FRAME) for k in range(n // FRAME)] if frames else [(0, n)]
        for pos, count in cuts:
            rows.append(pl.DemapIn(o.out[c].soft, n, pos, out_ptr + at + pos * B * item, count, 0, SLOTS[Mc] + 1, pl.DEMAP_I8 if i8 else 0,
                                   GAIN[0], GAIN[1], SCALE, 0))
        at += -(-n * B * item // 16) * 16
    return (pl.DemapIn * len(rows))(*rows), at


def host_check(pl, np, torch, h, o, ins, out, picks, maps):
    """values and records of the segments `picks` of the last call against psk_soft_demap_host of the downloaded rows"""
    base = out.data_ptr()
    for k in picks:
        s = ins[k]
        c = next(c for c in range(len(o.out)) if o.out[c].soft == s.soft)
        x = o.soft[c, : 2 * int(s.n_symbols)].cpu().numpy()
        Mc = 4 if s.map == SLOTS[4] + 1 else 8
        want, rec = pl.demap_host(*maps[Mc], x, s.pos, s.count, GAIN, SCALE, s.flags)
        got = out[s.out - base: s.out - base + want.nbytes].cpu().numpy().tobytes()
        if got != want.tobytes() or bytes(h.demap_records(k, 1)[0]) != bytes(rec):
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
        raise SystemExit("demap_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    C, N = args.channels, args.symbols * S
    result = {"tool": "demap_rates", "device": torch.cuda.get_device_name(0), "piece_symbols": pl.demap_piece(), "frame_symbols": FRAME,
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH), "steps": args.steps, "warmup": args.warmup,
              "timing": "HIP events on one stream around every step; medians", "shape": [C, args.symbols]}
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
    maps = {Mc: the_map(np, Mc) for Mc in SLOTS}
    for Mc, slot in SLOTS.items():
        h.demap_define(slot, *maps[Mc])
    result["t_demap"], result["t_copy"] = {}, {}
    ok = True
    for Mc in SLOTS:
        B = {4: 2, 8: 3}[Mc]
        for i8 in (True, False):
            form = "i8" if i8 else "f32"
            out = torch.zeros(sum(-(-n * B * (1 if i8 else 4) // 16) * 16 for n in n_sym), dtype=torch.uint8, device=dev)
            for frames in (False, True):
                ins, _ = segments(pl, o, n_sym, out.data_ptr(), Mc, i8, frames)
                symbols = sum(int(s.count) for s in ins) if frames else sum(n_sym)
                host_ms = []

                def step():
                    t0 = time.perf_counter()
                    h.demap_device(ins, raw)
                    host_ms.append((time.perf_counter() - t0) * 1e3)

                r = timed(torch, st, step, args.steps, args.warmup)
                ok = host_check(pl, np, torch, h, o, ins, out, sorted({0, 1, len(ins) // 2, len(ins) - 1}), maps) and ok
                sec = r["median_ms"] * 1e-3
                rd, wr = 8 * symbols, symbols * B * (1 if i8 else 4)
                r.update(M=Mc, form=form, cut="frames" if frames else "row", segments=len(ins), symbols=symbols, bytes_read=rd, bytes_written=wr,
                         symbols_per_s=symbols / sec, gbytes_per_s=(rd + wr) / sec / 1e9, t_host_median_ms=sorted(host_ms[args.warmup:])[args.steps // 2],
                         over_process=r["median_ms"] / result["t_process"]["median_ms"])
                result["t_demap"]["M%d_%s_%s" % (Mc, form, r["cut"])] = r
            # a copy that reads and writes as many bytes in all as the one-segment-a-row call
            rd, wr = 8 * sum(n_sym), sum(n_sym) * B * (1 if i8 else 4)
            half = (rd + wr) // 2
            src, dst = torch.zeros(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
            r = timed(torch, st, lambda: dst.copy_(src), args.steps, args.warmup)
            r.update(bytes_copied=half, gbytes_per_s=2 * half / (r["median_ms"] * 1e-3) / 1e9)
            result["t_copy"]["M%d_%s" % (Mc, form)] = r
            for cut in ("row", "frames"):
                d = result["t_demap"]["M%d_%s_%s" % (Mc, form, cut)]
                d["over_copy"] = d["median_ms"] / r["median_ms"]
            del src, dst, out
    result["values_and_records_equal_host"] = ok
    h.synchronize()
    h.close()
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
