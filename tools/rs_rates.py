#!/usr/bin/env python3
"""rs_rates.py -- what psk_soft_rs_device costs on one MI355X, next to the psk_soft_viterbi_device call that writes the bytes it
decodes: everything resident in HBM, everything on ONE stream, every step between two HIP events on that stream, medians over
--steps steps after --warmup.

Two frame shapes, 64 distinct frames of random data going round:

  ccsds_i5    CCSDS (255,223), 0x187 / 112 / 11 / 32, interleave depth 5: frames of 1275 bytes, --ccsds-frames a call
  dvb_i1      DVB (204,188), 0x11d / 0 / 1 / 16, depth 1: frames of 204 bytes, --dvb-frames a call

and per shape

  t_viterbi   psk_soft_viterbi_device (K = 7 171/133, PACKED | TERMINATED) over int8 LLRs of the same frames: the call that leaves
              the same payload where the rs call reads it
  t_rs        psk_soft_rs_device with "clean" frames (every syndrome zero), "t_errors" (t byte errors in every codeword) and
              "tenth_failed" (t + 1 byte errors in every tenth codeword, the others clean): ms, frames and codewords per second;
              for clean also the bytes read and written per second next to read_ceiling, psk_soft_probe_read_ms over the same
              input buffer.  The time is the stream's and holds the entry's own host work (one 32-byte descriptor a frame)
              wherever the stream waits for it; t_host is the call's wall time on the host.

Outputs and records of four frames of every rs call are checked against psk_soft_rs_host on the downloaded input, byte for byte.
One JSON object on stdout (and in --out).

    python tools/rs_rates.py [--steps 10] [--warmup 3] [--ccsds-frames 16384] [--dvb-frames 65536] [--out FILE.json]
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
DISTINCT = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ccsds-frames", type=int, default=16384)
    ap.add_argument("--dvb-frames", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from psk_soft_amd import lib as pl

    if not torch.cuda.is_available():
        raise SystemExit("rs_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    shapes = {"ccsds_i5": (pl.RS_CCSDS, 5, args.ccsds_frames), "dvb_i1": (pl.RS_DVB, 1, args.dvb_frames)}
    result = {"tool": "rs_rates", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
              "timing": "HIP events on one stream around every step; medians", "shapes": {}}
    in_dtype = np.dtype([("in", "<u8"), ("out", "<u8"), ("code", "<u4"), ("flags", "<u4"), ("pad", "<u4", 2)])
    vin_dtype = np.dtype([("llr", "<u8"), ("out", "<u8"), ("n_steps", "<u4"), ("code", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    h = pl.Handle(1, device=0)
    h.viterbi_define(0, 7, G)
    rng = np.random.default_rng(14)
    ok = True
    for slot, (name, ((gfpoly, fcr, prim, nroots, n), depth, F)) in enumerate(shapes.items()):
        code = (gfpoly, fcr, prim, nroots, n, depth)
        k, t, nin, nout = n - nroots, nroots // 2, n * depth, (n - nroots) * depth
        h.rs_define(slot, *code)
        clean = np.stack([pl.rs_encode_host(*code, rng.integers(0, 256, nout).astype(np.uint8)) for _ in range(DISTINCT)])

        def with_errors(count, every):
            """`count` byte errors in every `every`-th codeword of the call (codewords counted across the distinct frames)"""
            x = clean.copy()
            for q in range(DISTINCT):
                for j in range(depth):
                    if (q * depth + j) % every == 0:
                        for i in rng.choice(n, count, replace=False):
                            x[q, i * depth + j] ^= int(rng.integers(1, 256))
            return x

        cases = {"clean": clean, "t_errors": with_errors(t, 1), "tenth_failed": with_errors(t + 1, 10)}
        idx = torch.arange(F, device=dev) % DISTINCT
        out = torch.zeros(F * nout, dtype=torch.uint8, device=dev)
        sh = {"code": dict(gfpoly=gfpoly, fcr=fcr, prim=prim, nroots=nroots, n=n, depth=depth), "frames": F, "codewords": F * depth,
              "frame_bytes": nin, "t_rs": {}}

        # the Viterbi call that writes the same payload: int8 LLRs of the clean frames
        T = 8 * nin + 6
        llr_rows = np.zeros((DISTINCT, 2 * T), np.int8)
        for q in range(DISTINCT):
            bits = np.concatenate([np.unpackbits(clean[q]), np.zeros(6, np.uint8)])
            llr_rows[q] = np.where(pl.viterbi_encode(7, G, 1, 3, bits) == 0, 24, -24).astype(np.int8)
        llr = torch.from_numpy(llr_rows).to(dev)[idx].contiguous().reshape(-1)
        payload = torch.zeros(F * nin, dtype=torch.uint8, device=dev)
        vins = (pl.ViterbiIn * F)()
        a = np.frombuffer(vins, vin_dtype)
        a["llr"] = llr.data_ptr() + np.arange(F, dtype=np.uint64) * np.uint64(2 * T)
        a["out"] = payload.data_ptr() + np.arange(F, dtype=np.uint64) * np.uint64(nin)
        a["n_steps"], a["code"], a["flags"] = T, 1, pl.VITERBI_PACKED | pl.VITERBI_TERMINATED
        r = timed(torch, st, lambda: h.viterbi_device(vins, raw), args.steps, args.warmup)
        h.synchronize()
        ok = ok and bool((payload.reshape(F, nin)[:DISTINCT].cpu().numpy() == clean).all())
        r.update(steps_per_frame=T, payload_bytes=F * nin, payload_bits_per_s=F * nin * 8 / (r["median_ms"] * 1e-3))
        sh["t_viterbi"] = r
        del llr

        for case, rows in cases.items():
            buf = payload if case == "clean" else torch.from_numpy(rows).to(dev)[idx].contiguous().reshape(-1)
            ins = (pl.RsIn * F)()
            a = np.frombuffer(ins, in_dtype)
            a["in"] = buf.data_ptr() + np.arange(F, dtype=np.uint64) * np.uint64(nin)
            a["out"] = out.data_ptr() + np.arange(F, dtype=np.uint64) * np.uint64(nout)
            a["code"] = slot + 1
            host_ms = []

            def step():
                t0 = time.perf_counter()
                h.rs_device(ins, raw)
                host_ms.append((time.perf_counter() - t0) * 1e3)

            r = timed(torch, st, step, args.steps, args.warmup)
            n_err = []
            for f in sorted({0, 1, F // 2, F - 1}):
                want, rec = pl.rs_host(*code, buf[f * nin: (f + 1) * nin].cpu().numpy())
                got = out[f * nout: (f + 1) * nout].cpu().numpy().tobytes()
                grec = h.get_rs(f, 1)[0]
                ok = ok and got == want.tobytes() and bytes(grec) == bytes(rec)
                n_err.append(list(grec.n_err)[:depth])
            sec = r["median_ms"] * 1e-3
            r.update(frames_per_s=F / sec, codewords_per_s=F * depth / sec, n_err_of_checked_frames=n_err,
                     t_host_median_ms=sorted(host_ms[args.warmup:])[args.steps // 2], over_viterbi=r["median_ms"] / sh["t_viterbi"]["median_ms"])
            if case == "clean":
                read_ms = h.probe_read_ms(buf.data_ptr(), F * nin, 5)
                r.update(bytes_moved=F * (nin + nout), gbytes_per_s=F * (nin + nout) / sec / 1e9, read_ceiling_ms=read_ms,
                         read_ceiling_gbytes_per_s=F * nin / (read_ms * 1e-3) / 1e9)
            sh["t_rs"][case] = r
        result["shapes"][name] = sh
        del out, payload
    result["outputs_and_records_equal_host"] = ok
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
