#!/usr/bin/env python3
"""frame_rates.py -- what psk_soft_frame_search_device and psk_soft_frame_cut_device cost on one MI355X, next to the
psk_soft_viterbi_device call that writes the bits they read and next to a device-to-device copy of the bytes the cut writes:
everything resident in HBM, everything on ONE stream, every step between two HIP events on that stream, medians over --steps
steps after --warmup.

Two shapes of --streams streams each, 8 distinct streams of random data going round; a stream is one Viterbi frame (K = 7 171/133,
PACKED, unterminated, 16 junk bytes at its end):

  ccsds_i5    6 frames of the 32-bit marker 0x1ACFFC1D + 1275 bytes (CCSDS (255,223), interleave depth 5) behind 11 junk bits;
              searched with L = 32, max_diff 2, unfolded (P = 0) and folded over the frame length (P = 10232); cut plain, 1275
              bytes a frame behind every marker
  dvb_i1      24 packets of 204 bytes, 0x47 with every eighth 0xB8, through the (12, 17) interleaver, behind 13 junk bits;
              searched with L = 8, max_diff 0, P = 1632; cut with the (12, 17) format, 204 bytes a packet

and per shape

  t_viterbi   the call that leaves the same payload where the search and the cut read it
  t_search    psk_soft_frame_search_device over all the streams (fold + join): ms, streams and payload bits per second,
              over_viterbi = t_search / t_viterbi
  t_cut       psk_soft_frame_cut_device of every frame of every stream: ms, frames per second, bytes written per second
  t_copy      a device-to-device copy of as many bytes as the cut writes: the floor a gather can approach; over_copy = t_cut / t_copy

The records of four streams of every search call, and the outputs and records of four frames of every cut call, are checked
against psk_soft_frame_search_host / psk_soft_frame_cut_host on the downloaded payload, byte for byte.  One JSON object on stdout
(and in --out).

    python tools/frame_rates.py [--steps 10] [--warmup 3] [--streams 2048] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from strided_rates import timed  # noqa: E402

G = (0o171, 0o133)
DISTINCT = 8
TAIL_BYTES = 16
ASM = 0x1ACFFC1D


def interleave(np, data, branches, cell):
    """the transmitter's convolutional byte interleaver: byte k is delayed by (k mod branches) * cell * branches bytes"""
    k = np.arange(len(data), dtype=np.int64)
    y = np.zeros(len(data) + (branches - 1) * cell * branches, np.uint8)
    y[k + (k % branches) * cell * branches] = data
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from psk_soft_amd import lib as pl

    if not torch.cuda.is_available():
        raise SystemExit("frame_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    S = args.streams
    result = {"tool": "frame_rates", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "streams": S,
              "tile": int(pl.load().psk_soft_frame_tile()), "timing": "HIP events on one stream around every step; medians", "shapes": {}}
    vin_dtype = np.dtype([("llr", "<u8"), ("out", "<u8"), ("n_steps", "<u4"), ("code", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
    sin_dtype = np.dtype([("bits", "<u8"), ("bit0", "<u8"), ("n_bits", "<u4"), ("word", "<u4"), ("max_diff", "<u4"), ("period", "<u4"),
                          ("flags", "<u4"), ("pad", "<u4", 3)])
    cin_dtype = np.dtype([("bits", "<u8"), ("bit", "<u8"), ("out", "<u8"), ("n_bytes", "<u4"), ("format", "<u4"), ("branch0", "<u4"),
                          ("flags", "<u4"), ("pad", "<u4", 2)])
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    h = pl.Handle(1, device=0)
    h.viterbi_define(0, 7, G)
    h.frame_word_define(0, 32, ASM)
    h.frame_word_define(1, 8, 0x47)
    h.frame_format_define(0, 12, 17)
    rng = np.random.default_rng(15)
    ok = True

    def ccsds_stream():
        frames = [np.concatenate([np.frombuffer(ASM.to_bytes(4, "big"), np.uint8), rng.integers(0, 256, 1275).astype(np.uint8)]) for _ in range(6)]
        return 11, np.concatenate(frames + [rng.integers(0, 256, TAIL_BYTES).astype(np.uint8)])

    def dvb_stream():
        p = rng.integers(0, 256, (24, 204)).astype(np.uint8)
        p[:, 0] = 0x47
        p[::8, 0] = 0xB8
        return 13, np.concatenate([interleave(np, p.reshape(-1), 12, 17), rng.integers(0, 256, TAIL_BYTES).astype(np.uint8)])

    shapes = {
        # name: (make, word slot, max_diff, periods, frames a stream, first frame's bit behind the junk, bits a frame, n_bytes, format)
        "ccsds_i5": (ccsds_stream, 0, 2, (0, 8 * 1279), 6, 32, 8 * 1279, 1275, 0),
        "dvb_i1": (dvb_stream, 1, 0, (1632,), 24, 0, 1632, 204, 1),
    }
    for name, (make, wslot, max_diff, periods, per_stream, first_bit, frame_bits, n_bytes, fmt) in shapes.items():
        streams = [make() for _ in range(DISTINCT)]
        junk, nbytes = streams[0][0], streams[0][1].size
        T = junk + 8 * nbytes
        good = T - 8 * TAIL_BYTES  # (the decoder's unterminated tail is junk)
        stride = (T + 7) // 8 + 3  # (streams at every byte alignment)
        llr_rows = np.zeros((DISTINCT, 2 * T), np.int8)
        sent = []
        for q, (_, body) in enumerate(streams):
            bits = np.concatenate([rng.integers(0, 2, junk).astype(np.uint8), np.unpackbits(body)])
            sent.append(bits)
            llr_rows[q] = np.where(pl.viterbi_encode(7, G, 1, 3, bits) == 0, 24, -24).astype(np.int8)
        idx = torch.arange(S, device=dev) % DISTINCT
        llr = torch.from_numpy(llr_rows).to(dev)[idx].contiguous().reshape(-1)
        payload = torch.zeros(S * stride + 8, dtype=torch.uint8, device=dev)
        vins = (pl.ViterbiIn * S)()
        a = np.frombuffer(vins, vin_dtype)
        a["llr"] = llr.data_ptr() + np.arange(S, dtype=np.uint64) * np.uint64(2 * T)
        a["out"] = payload.data_ptr() + np.arange(S, dtype=np.uint64) * np.uint64(stride)
        a["n_steps"], a["code"], a["flags"] = T, 1, pl.VITERBI_PACKED
        sh = {"streams": S, "stream_bits": good, "frames_per_stream": per_stream, "frame_bytes": n_bytes, "t_search": {}}
        r = timed(torch, st, lambda: h.viterbi_device(vins, raw), args.steps, args.warmup)
        h.synchronize()
        host_payload = payload.cpu().numpy()
        for q in range(DISTINCT):
            got = np.unpackbits(host_payload[q * stride: q * stride + (T + 7) // 8])[:good]
            ok = ok and bool((got == sent[q][:good]).all())
        r.update(steps_per_frame=T, payload_bits=S * good, payload_bits_per_s=S * good / (r["median_ms"] * 1e-3))
        sh["t_viterbi"] = r
        del llr

        length, word = (32, ASM) if wslot == 0 else (8, 0x47)
        for P in periods:
            sins = (pl.FrameSearchIn * S)()
            a = np.frombuffer(sins, sin_dtype)
            a["bits"] = payload.data_ptr() + np.arange(S, dtype=np.uint64) * np.uint64(stride)
            a["n_bits"], a["word"], a["max_diff"], a["period"] = good, wslot + 1, max_diff, P
            host_ms = []

            def step():
                t0 = time.perf_counter()
                h.frame_search_device(sins, raw)
                host_ms.append((time.perf_counter() - t0) * 1e3)

            r = timed(torch, st, step, args.steps, args.warmup)
            first_hits = []
            for s in sorted({0, 1, S // 2, S - 1}):
                want = pl.frame_search_host(length, word, pl.FRAME_CCSDS_ASM[2] if wslot == 0 else 0xFF, host_payload[s * stride:], good, 0, max_diff, P)
                got = h.frame_search_records(s, 1)[0]
                ok = ok and bytes(got) == bytes(want) and got.n_listed >= min(per_stream, 16)
                first_hits.append(got.listed[:2])
            sec = r["median_ms"] * 1e-3
            r.update(period=P, streams_per_s=S / sec, payload_bits_per_s=S * good / sec, first_hits_of_checked_streams=first_hits,
                     t_host_median_ms=sorted(host_ms[args.warmup:])[args.steps // 2], over_viterbi=r["median_ms"] / sh["t_viterbi"]["median_ms"])
            sh["t_search"]["period_%d" % P] = r

        F = S * per_stream
        out = torch.zeros(F * n_bytes, dtype=torch.uint8, device=dev)
        cins = (pl.FrameCutIn * F)()
        a = np.frombuffer(cins, cin_dtype)
        f = np.arange(F, dtype=np.uint64)
        a["bits"] = payload.data_ptr() + (f // np.uint64(per_stream)) * np.uint64(stride)
        a["bit"] = junk + first_bit + (f % np.uint64(per_stream)) * np.uint64(frame_bits)
        a["out"] = out.data_ptr() + f * np.uint64(n_bytes)
        a["n_bytes"], a["format"] = n_bytes, fmt
        host_ms = []

        def step():
            t0 = time.perf_counter()
            h.frame_cut_device(cins, raw)
            host_ms.append((time.perf_counter() - t0) * 1e3)

        r = timed(torch, st, step, args.steps, args.warmup)
        B, M = (12, 17) if fmt else (1, 0)
        for k in sorted({0, 1, F // 2, F - 1}):
            s, j = divmod(k, per_stream)
            want, rec = pl.frame_cut_host(B, M, host_payload[s * stride:], junk + first_bit + j * frame_bits, n_bytes)
            got = out[k * n_bytes: (k + 1) * n_bytes].cpu().numpy().tobytes()
            ok = ok and got == want.tobytes() and bytes(h.frame_cut_records(k, 1)[0]) == bytes(rec)
        sec = r["median_ms"] * 1e-3
        src = torch.zeros_like(out)
        c = timed(torch, st, lambda: out.copy_(src), args.steps, args.warmup)
        r.update(frames=F, frames_per_s=F / sec, bytes_written=F * n_bytes, gbytes_written_per_s=F * n_bytes / sec / 1e9,
                 t_host_median_ms=sorted(host_ms[args.warmup:])[args.steps // 2], over_viterbi=r["median_ms"] / sh["t_viterbi"]["median_ms"],
                 over_copy=r["median_ms"] / c["median_ms"])
        c.update(bytes=F * n_bytes, gbytes_per_s=F * n_bytes / (c["median_ms"] * 1e-3) / 1e9)
        sh["t_cut"], sh["t_copy"] = r, c
        result["shapes"][name] = sh
        del out, src, payload
    result["records_and_outputs_equal_host"] = ok
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
