// psk_demap.hip -- psk_soft_demap_device: segments of soft rows as per-bit soft decisions (max-log LLRs), one psk_soft_demap_t
// per segment.
//
// A segment is `count` symbols of a row from `pos` on, turned by a complex gain and held against a map of M points the caller
// defined (include/psk_soft_hip.h, "frames as soft bits"; psk_demap.h restates the arithmetic).  One pass over the segments, two
// kernels:
//
//   fold   grid (workgroups per segment, segments), one workgroup of 256 lanes per piece of kDemapPiece symbols of one segment;
//          the pieces of a segment go round its workgroups, the segments beyond 65535 take further trips of the segment loop.
//          Consecutive lanes take consecutive symbols with one 8-byte load each (lane t the symbols t, t + 256, t + 512, t + 768
//          of the piece, all four loads issued before the first is used); positions in front of the row come from the sync
//          history the descriptor names, or are zeros.  The map -- at most 8 points and labels -- and the descriptor are
//          wave-uniform.  The B values of a symbol go into LDS, float32 or int8, and from there to the segment's output with
//          full dwords: a lane stores dword k, k + 256, ... of the piece's values.  The int8 values are staged at the byte
//          offset their destination has within a dword, so the dword body is aligned in LDS and in memory alike; byte stores
//          are used only for the at most three bytes in front of the body and behind it (B = 3 and any `out` make a piece's
//          values begin and end anywhere).  No byte outside the piece's count * B values is written.
//          The lane adds e and dmin of its finite symbols in doubles in the order above, counts finite symbols, clamped and NaN
//          values; a fixed xor-tree across each wave, the four waves in order: one partial per piece.
//   join   one wave per segment: the partials in ascending piece order, 64 loaded at a time, added one after the other from
//          piece 0's; the record, or the zero record for a skipped segment.
//
// Which lane adds which symbol, and in which order, depends on the symbol's index in the segment only -- not on the batch, the
// grid, the stream or the alignment of `out` --, so the same segment gives the same bytes.  No atomics.  The arithmetic
// (psk_demap.h) is rounded once per operation (the unit is built with -ffp-contract=off), denormals kept.  Plain vector loads and
// stores only; the rows, the history and the maps are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_demap.h"
#include "psk_front_src.h"

namespace psk {

namespace {

constexpr uint32_t kWaves = kDemapThreads / 64u;
constexpr uint32_t kTurns = kDemapPiece / kDemapThreads;
constexpr uint32_t kStageWords = kDemapPiece * kDemapMaxB + 1u;  // the values of a piece as float32; as int8 behind up to 3 bytes

__device__ __forceinline__ double d_wave_sum(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ uint32_t d_wave_sum(uint32_t v)
{
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

}  // namespace

__global__ __launch_bounds__(kDemapThreads) void psk_demap_fold_kernel(const DemapDesc *__restrict__ desc, uint32_t nseg,
                                                                       const DemapMap *__restrict__ maps,
                                                                       DemapPartial *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) uint32_t stage[kStageWords];
    __shared__ double red_d[kWaves][2];
    __shared__ uint32_t red_c[kWaves][3];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t c = blockIdx.y; c < nseg; c += gridDim.y) {
        const DemapDesc d = desc[c];
        // (uniform for the workgroup, like every branch on the descriptor and the map below)
        if (!(d.flags & kDemapData) || blockIdx.x >= d.n_piece || d.map >= kDemapSlots)
            continue;
        const DemapMap m = maps[d.map];
        const uint32_t B = m.B;
        if (!B || B > kDemapMaxB || m.M != (1u << B))
            continue;
        const bool i8 = (d.flags & kDemapI8) != 0;
        const PSK_GLOBAL f2 *const row = (const PSK_GLOBAL f2 *)d.soft;
        const PSK_GLOBAL f2 *const front = (const PSK_GLOBAL f2 *)d.front;
        for (uint32_t p = blockIdx.x; p < d.n_piece; p += gridDim.x) {
            const uint32_t lo = p * kDemapPiece;  // (n_piece = ceil(count / kDemapPiece): lo < count)
            const uint32_t cnt = d.count - lo < kDemapPiece ? d.count - lo : kDemapPiece;
            const int64_t g0 = d.pos + (int64_t)lo;  // (g0 + cnt <= the row's length: the entry checked pos + count)
            // where the piece's values go: value k of the piece is value lo * B + k of the segment
            const uint64_t v0 = (uint64_t)lo * B;
            const uint32_t sh = i8 ? (uint32_t)(((uintptr_t)d.out + v0) & 3u) : 0u;
            __syncthreads();  // (the LDS of the piece before is read out)
            f2 x[kTurns];
#pragma unroll
            for (uint32_t turn = 0; turn < kTurns; turn++) {
                const uint32_t i = turn * kDemapThreads + t;
                const int64_t g = g0 + (int64_t)i;
                x[turn] = f2{0.0f, 0.0f};
                if (i < cnt) {
                    if (g >= 0)
                        x[turn] = row[g];
                    else if (front)
                        x[turn] = front[g + (int64_t)kDemapFront];  // (g >= -127)
                }
            }
            double se = 0.0, serr = 0.0;
            uint32_t nf = 0, nclip = 0, nnan = 0;
#pragma unroll
            for (uint32_t turn = 0; turn < kTurns; turn++) {
                const uint32_t i = turn * kDemapThreads + t;
                float e, dmin, v[kDemapMaxB];
                const bool fin = dm_symbol(m, x[turn].x, x[turn].y, d.gain_re, d.gain_im, d.scale, &e, &dmin, v);
                if (i >= cnt)
                    continue;
                if (fin) {
                    se += (double)e;
                    serr += (double)dmin;
                    nf++;
                }
#pragma unroll
                for (uint32_t j = 0; j < kDemapMaxB; j++) {
                    if (j >= B)
                        break;
                    nnan += v[j] != v[j] ? 1u : 0u;
                    if (i8)
                        reinterpret_cast<int8_t *>(stage)[sh + i * B + j] = (int8_t)dm_i8(v[j], &nclip);
                    else
                        reinterpret_cast<float *>(stage)[i * B + j] = dm_f32(v[j]);
                }
            }
            {
                const double a = d_wave_sum(se), b = d_wave_sum(serr);
                const uint32_t c0 = d_wave_sum(nf), c1 = d_wave_sum(nclip), c2 = d_wave_sum(nnan);
                if (lane == 0)
                    red_d[wave][0] = a, red_d[wave][1] = b, red_c[wave][0] = c0, red_c[wave][1] = c1, red_c[wave][2] = c2;
            }
            __syncthreads();
            const uint32_t nval = cnt * B;
            if (i8) {
                PSK_GLOBAL uint8_t *const o = (PSK_GLOBAL uint8_t *)d.out + v0;
                const uint8_t *const sb = reinterpret_cast<const uint8_t *>(stage) + sh;  // byte k of the piece
                const uint32_t to_dword = (4u - sh) & 3u;
                const uint32_t head = nval < to_dword ? nval : to_dword;
                const uint32_t body = (nval - head) / 4u, tail = nval - head - 4u * body;
                // (with a body, sh + head is 0 or 4: the body is whole dwords of the stage and of memory)
                const uint32_t *const sw = reinterpret_cast<const uint32_t *>(sb + head);
                PSK_GLOBAL uint32_t *const ow = (PSK_GLOBAL uint32_t *)(o + head);
                for (uint32_t k = t; k < body; k += kDemapThreads) ow[k] = sw[k];
                if (t >= 64u && t < 64u + head)
                    o[t - 64u] = sb[t - 64u];
                if (t >= 128u && t < 128u + tail)
                    o[head + 4u * body + (t - 128u)] = sb[head + 4u * body + (t - 128u)];
            } else {
                PSK_GLOBAL uint32_t *const o = (PSK_GLOBAL uint32_t *)d.out + v0;
                for (uint32_t k = t; k < nval; k += kDemapThreads) o[k] = stage[k];
            }
            if (t == 0) {
                // the waves in order, from wave 0's value
                double a = red_d[0][0], b = red_d[0][1];
                uint32_t c0 = red_c[0][0], c1 = red_c[0][1], c2 = red_c[0][2];
                for (uint32_t w = 1; w < kWaves; w++) {
                    a += red_d[w][0], b += red_d[w][1];
                    c0 += red_c[w][0], c1 += red_c[w][1], c2 += red_c[w][2];
                }
                PSK_GLOBAL DemapPartial *const q = (PSK_GLOBAL DemapPartial *)part + (d.part0 + p);
                q->sum_e = a, q->sum_err = b;
                q->n_finite = c0, q->n_clip = c1, q->n_nan = c2, q->pad = 0u;
            }
        }
    }
}

__global__ __launch_bounds__(64) void psk_demap_join_kernel(const DemapDesc *__restrict__ desc, uint32_t nseg,
                                                            const DemapMap *__restrict__ maps, const DemapPartial *__restrict__ part,
                                                            psk_soft_demap_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < nseg; c += gridDim.x) {
        const DemapDesc d = desc[c];
        const bool data = (d.flags & kDemapData) != 0 && d.map < kDemapSlots;
        double se = 0.0, serr = 0.0;
        uint64_t nf = 0, nclip = 0, nnan = 0;
        for (uint32_t base = 0; data && base < d.n_piece; base += 64u) {
            const uint32_t left = d.n_piece - base, n = left < 64u ? left : 64u;
            DemapPartial q = {};
            if (lane < n) {
                const PSK_GLOBAL DemapPartial *const g = (const PSK_GLOBAL DemapPartial *)part + (d.part0 + base + lane);
                q.sum_e = g->sum_e, q.sum_err = g->sum_err;
                q.n_finite = g->n_finite, q.n_clip = g->n_clip, q.n_nan = g->n_nan;
            }
            // the pieces one after the other, from piece 0's value: every lane forms the same sums
            for (uint32_t k = 0; k < n; k++) {
                const double a = __shfl(q.sum_e, (int)k), b = __shfl(q.sum_err, (int)k);
                const bool first = base == 0u && k == 0u;
                se = first ? a : se + a;
                serr = first ? b : serr + b;
                nf += (uint32_t)__shfl((int)q.n_finite, (int)k);
                nclip += (uint32_t)__shfl((int)q.n_clip, (int)k);
                nnan += (uint32_t)__shfl((int)q.n_nan, (int)k);
            }
        }
        if (lane != 0)
            continue;
        psk_soft_demap_t r = {};  // (pad stays zero; lane 0 alone stores the 64 bytes)
        if (data) {
            r.n_symbols = d.count;
            r.n_finite = nf, r.n_clip = nclip, r.n_nan = nnan;
            r.sum_e = se, r.sum_err = serr;
            r.bits = maps[d.map].B;
            r.flags = PSK_SOFT_DEMAP_DATA | ((d.flags & kDemapI8) ? PSK_SOFT_DEMAP_REC_I8 : 0u);
        }
        records[c] = r;
    }
}

hipError_t launch_demap_fold(const DemapDesc *desc, uint32_t nseg, uint32_t max_piece, const DemapMap *maps, DemapPartial *part,
                             hipStream_t stream)
{
    if (!nseg || !max_piece)
        return hipSuccess;
    // the shared grid rule for the workgroups of a segment; more than 65535 segments take further trips of the segment loop
    const dim3 grid(front_grid_y(max_piece, nseg), nseg < 65535u ? nseg : 65535u);
    hipLaunchKernelGGL(psk_demap_fold_kernel, grid, dim3(kDemapThreads), 0, stream, desc, nseg, maps, part);
    return hipGetLastError();
}

hipError_t launch_demap_join(const DemapDesc *desc, uint32_t nseg, const DemapMap *maps, const DemapPartial *part,
                             psk_soft_demap_t *records, hipStream_t stream)
{
    if (!nseg)
        return hipSuccess;
    hipLaunchKernelGGL(psk_demap_join_kernel, dim3(nseg < 65535u ? nseg : 65535u), dim3(64), 0, stream, desc, nseg, maps, part, records);
    return hipGetLastError();
}

}  // namespace psk
