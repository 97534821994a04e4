#!/usr/bin/env python3
"""strided_rates.py -- what psk_soft_process_device_strided costs on one MI355X: packets straight from a frame-major matrix
(a channelizer's output, [frame][channel]) against the same samples handed over contiguous, and against what a host does
without the entry -- transpose the matrix itself with torch, then call psk_soft_process_device.

Per format (cf32 / sc16 / sc8; int8 values, round(40 x), cast), QPSK, samplesPerBaud 8, numAvg 100, everything resident in HBM,
everything on ONE stream, every step timed with a pair of HIP events on that stream, medians over --steps steps after --warmup:

  t_contig    psk_soft_process_device on [channel][time] data
  t_strided   psk_soft_process_device_strided on the same samples laid out [frame][channel]
  t_diy       torch: the frame matrix .transpose(0, 1).contiguous() (one element a complex sample), then t_contig's call
  t_gather    the gather pass of t_strided alone (a handle created under PSK_SOFT_DIAG_GATHER_ONLY=1), with the bytes it reads
              and writes per second, next to the live read ceiling of the box (psk_soft_probe_read_ms over the matrix) and the
              copy ceiling of the MI355X guide (6.29 TB/s, read + write, float4 copy)

for three shapes: 4096 channels x 2^18 samples (the condition: t_strided <= 1.05 x t_diy), 64 channels x 2^20 samples, and 4096
channels x 2^16 samples in every second column of a matrix twice as wide (no frame groups: every packet gathered as a single).
The first step of every variant is compared: the three must give the same bits on every channel.  One JSON object on stdout
(and in --out).

    python tools/strided_rates.py [--steps 10] [--warmup 3] [--out profiles/r08/strided_rates.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cs16_rates import A, M, NPH, S, outputs, packets  # noqa: E402
from cs8_rates import quantise_torch  # noqa: E402

GUIDE_COPY_CEILING_TBS = 6.29
BOUND = 1.05


def _formats(pl, torch):
    # (name, PSK_SOFT_FORMAT_*, element type, a type as wide as one complex sample)
    return (("cf32", pl.FORMAT_CF32, torch.float32, torch.int64), ("sc16", pl.FORMAT_CS16, torch.int16, torch.int32),
            ("sc8", pl.FORMAT_CS8, torch.int8, torch.int16))


class Outs:
    def __init__(self, pl, torch, C, cap, dev):
        self.soft = torch.zeros((C, 2 * cap), dtype=torch.float32, device=dev)
        self.phase = torch.zeros((C, cap), dtype=torch.float32, device=dev)
        self.sidx = torch.zeros((C, cap), dtype=torch.int16, device=dev)
        self.bits = torch.zeros((C, 2 * cap), dtype=torch.int16, device=dev)
        self.out = outputs(pl, C, cap, lambda c: self.soft[c].data_ptr(), lambda c: self.bits[c].data_ptr(),
                           lambda c: self.phase[c].data_ptr(), lambda c: self.sidx[c].data_ptr())

    def same(self, torch, other):
        return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for a, b in ((self.soft, other.soft), (self.phase, other.phase), (self.sidx, other.sidx), (self.bits, other.bits)))


def timed(torch, st, step, steps, warmup):
    """median, min and max (ms) of `steps` runs of step() on stream `st`, each between two events, after `warmup` runs"""
    with torch.cuda.stream(st):
        for _ in range(warmup):
            step()
        st.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            step()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def run_shape(pl, torch, iq8, name, fmt, tdt, wide, width, col0, col_step, steps, warmup):
    """one format, one shape: iq8 (C, 2N) int8 values; the channels sit in columns col0, col0 + col_step, ... of a matrix
    `width` wide"""
    dev = iq8.device
    C, N = iq8.shape[0], iq8.shape[1] // 2
    cap = (N // S + 2 + 63) // 64 * 64
    sb = 2 * torch.empty((), dtype=tdt).element_size()
    contig = iq8.to(tdt).contiguous()                                 # [channel][time][I, Q]
    frame = torch.zeros((N, width, 2), dtype=tdt, device=dev)         # [frame][column][I, Q]
    frame[:, col0 : col0 + col_step * C : col_step, :] = contig.view(C, N, 2).permute(1, 0, 2)
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    res = {"shape": [C, N], "matrix_width": width, "first_column": col0, "column_step": col_step, "sample_bytes": sb}

    def handle(env=None):
        if env:
            os.environ[env] = "1"
        h = pl.Handle(C, device=0)
        if env:
            os.environ.pop(env)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
        return h

    def strided_packets(first):
        pk = packets(pl, C, lambda c: frame.data_ptr() + sb * (col0 + col_step * c), 2 * N, fmt, first)
        return pk, (pl.ctypes.c_uint64 * C)(*([width] * C))

    # t_contig
    h, o_c = handle(), Outs(pl, torch, C, cap, dev)
    row = contig.stride(0) * contig.element_size()
    pk0 = packets(pl, C, lambda c: contig.data_ptr() + c * row, 2 * N, fmt, True)
    pk = packets(pl, C, lambda c: contig.data_ptr() + c * row, 2 * N, fmt, False)
    h.process_device(0, pk0, o_c.out, raw)
    h.synchronize()
    first_c = [int(o_c.out[c].n_symbols) for c in range(C)]
    keep_c = Outs(pl, torch, C, cap, dev)
    for a, b in ((keep_c.soft, o_c.soft), (keep_c.phase, o_c.phase), (keep_c.sidx, o_c.sidx), (keep_c.bits, o_c.bits)):
        a.copy_(b)
    torch.cuda.synchronize()
    res["t_contig"] = timed(torch, st, lambda: h.process_device(0, pk, o_c.out, raw), steps, warmup)
    st_c = h.stats()
    res["channels_fast"], res["channels_tiled"], res["channels_sequential"] = st_c["channels_fast"], st_c["channels_tiled"], st_c["channels_sequential"]
    res["read_ceiling_ms"] = h.probe_read_ms(frame.data_ptr(), frame.numel() * frame.element_size(), 5)
    h.close()

    # t_strided
    h, o_s = handle(), Outs(pl, torch, C, cap, dev)
    spk0, strides = strided_packets(True)
    spk, _ = strided_packets(False)
    h.process_device_strided(0, spk0, strides, o_s.out, raw)
    h.synchronize()
    torch.cuda.synchronize()
    same_s = first_c == [int(o_s.out[c].n_symbols) for c in range(C)] and o_s.same(torch, keep_c)
    res["t_strided"] = timed(torch, st, lambda: h.process_device_strided(0, spk, strides, o_s.out, raw), steps, warmup)
    h.close()
    del o_s

    # t_gather: the pass alone
    h, o_g = handle("PSK_SOFT_DIAG_GATHER_ONLY"), Outs(pl, torch, C, cap, dev)
    res["t_gather"] = timed(torch, st, lambda: h.process_device_strided(0, spk, strides, o_g.out, raw), steps, warmup)
    h.close()
    del o_g

    # t_diy: torch transposes, then the contiguous call
    h, o_d = handle(), Outs(pl, torch, C, cap, dev)
    frame_w = frame.view(wide).squeeze(-1)  # (N, width): one element a complex sample
    state = {}

    def diy(first=False):
        t = frame_w.transpose(0, 1).contiguous()  # (width, N)
        if state.get("ptr") != t.data_ptr():  # (the caching allocator hands the same block back: built once in practice)
            state["ptr"] = t.data_ptr()
            state["builds"] = state.get("builds", 0) + 1
            prow = t.stride(0) * t.element_size()
            state["pk"] = packets(pl, C, lambda c: t.data_ptr() + (col0 + col_step * c) * prow, 2 * N, fmt, False)
            state["pk0"] = packets(pl, C, lambda c: t.data_ptr() + (col0 + col_step * c) * prow, 2 * N, fmt, True)
        h.process_device(0, state["pk0" if first else "pk"], o_d.out, raw)

    with torch.cuda.stream(st):
        diy(True)
    h.synchronize()
    torch.cuda.synchronize()
    same_d = first_c == [int(o_d.out[c].n_symbols) for c in range(C)] and o_d.same(torch, keep_c)
    res["t_diy"] = timed(torch, st, diy, steps, warmup)
    res["t_diy_transpose"] = timed(torch, st, lambda: frame_w.transpose(0, 1).contiguous(), steps, warmup)
    res["diy_packet_builds"] = state["builds"]
    h.close()

    res["first_step_identical"] = bool(same_s and same_d)
    moved = 2 * C * N * sb  # the pass reads every sample once and writes it once
    g = res["t_gather"]["median_ms"]
    res["gather_bytes_read_plus_written"] = moved
    res["gather_tb_per_s"] = moved / (g * 1e-3) / 1e12
    res["read_ceiling_tb_per_s"] = frame.numel() * frame.element_size() / (res["read_ceiling_ms"] * 1e-3) / 1e12
    res["guide_copy_ceiling_tb_per_s"] = GUIDE_COPY_CEILING_TBS
    res["ratio_strided_over_diy"] = res["t_strided"]["median_ms"] / res["t_diy"]["median_ms"]
    res["ratio_strided_over_contig"] = res["t_strided"]["median_ms"] / res["t_contig"]["median_ms"]
    res["condition_strided_le_1p05_diy"] = bool(res["ratio_strided_over_diy"] <= BOUND)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--nsamp", type=int, default=1 << 18)
    ap.add_argument("--few-channels", type=int, default=64)
    ap.add_argument("--few-nsamp", type=int, default=1 << 20)
    ap.add_argument("--singles-nsamp", type=int, default=1 << 16)
    ap.add_argument("--cases", default="headline,few,singles")
    ap.add_argument("--formats", default="cf32,sc16,sc8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("strided_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    result = {"tool": "strided_rates", "device": torch.cuda.get_device_name(0), "scale": 40.0, "bound": BOUND,
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH), "steps": args.steps, "warmup": args.warmup,
              "timing": "HIP events on one stream around every step; medians"}
    cases = {"headline": (args.channels, args.nsamp, None), "few": (args.few_channels, args.few_nsamp, None),
             "singles": (args.channels, args.singles_nsamp, 2)}
    for case in args.cases.split(","):
        C, N, step = cases[case]
        iq8 = quantise_torch(synth_channels_torch(C, M, S, N, dev)).contiguous()
        result[case] = {}
        for name, fmt, tdt, wide in _formats(pl, torch):
            if name not in args.formats.split(","):
                continue
            width, col0, col_step = (C, 0, 1) if step is None else (step * C, 1, step)
            result[case][name] = run_shape(pl, torch, iq8, name, fmt, tdt, wide, width, col0, col_step, args.steps, args.warmup)
            torch.cuda.empty_cache()
        del iq8
        torch.cuda.empty_cache()
    if "headline" in result:
        result["condition_met"] = {k: v["condition_strided_le_1p05_diy"] for k, v in result["headline"].items()}
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(v["first_step_identical"] for case in result.values() if isinstance(case, dict) for v in case.values()
             if isinstance(v, dict) and "first_step_identical" in v)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
