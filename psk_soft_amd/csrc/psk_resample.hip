// psk_resample.hip -- the resample pre-pass of psk_soft_process_device_resampled: every resampled packet of a call, whatever its
// format and stride, read once, shifted in frequency if it is also tuned (psk_tune.h: tune_rotate), interpolated at the call's
// output instants (psk_resample.h: resample_taps / resample_mix) and written as float2 rows of the handle's gather scratch; the
// ordinary call then runs on the rows as on CF32 packets.  One launch per call.
//
// A workgroup walks pieces of kResamplePiece outputs of one packet.  Per piece it loads the inputs the piece needs, s[i(m0)-3 ..
// i(m1-1)], once -- converted (psk_pkt_cvt.h), rotated with the phasor tables in LDS as the tune kernel does, the channel's history
// slot supplying the indices below 0 -- into LDS as float2; every lane then computes two adjacent outputs an iteration from LDS
// and stores them as 16 bytes.  A lane issues all its loads of a piece (nine at most) before it uses the first.  The instant of a
// lane's first output costs one 64-bit multiply per piece, every further one a
// 64-bit add; the phase word of its first input likewise.  The workgroup that takes the packet's last piece (or the first one of
// a packet without outputs) writes the history behind the packet into the channel's other slot.  Plain vector loads and stores
// only; the source is never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_pkt_cvt.h"
#include "psk_resample.h"
#include "psk_soft_hip.h"
#include "psk_tune.h"

namespace psk {

#define PSK_GLOBAL __attribute__((address_space(1)))
typedef float rs_f2 __attribute__((ext_vector_type(2)));
typedef float rs_f4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kRsThreads = 256;
constexpr uint32_t kRsLoads = (kResampleInputs + kRsThreads - 1u) / kRsThreads;  // inputs a lane loads per piece, at most
static_assert(kResamplePiece % 2u == 0, "a piece starts on an even output: the 16-byte stores are aligned");
static_assert(sizeof(float) * (kTuneTableFloats + 2u * kResampleInputs) <= 65536u, "tables and samples in static LDS");

// one sample as it lies in the packet (a load), and its float2 (arithmetic only: a lane keeps its loads apart from their first use)
template <int FMT>
struct RsRaw {
    typedef typename PktWord<FMT>::type type;
};
template <>
struct RsRaw<PSK_SOFT_FORMAT_CF32> {
    typedef rs_f2 type;
};
template <int FMT>
__device__ inline typename RsRaw<FMT>::type rs_load_raw(const PSK_GLOBAL void *src, uint64_t idx)
{
    return reinterpret_cast<const PSK_GLOBAL typename RsRaw<FMT>::type *>(src)[idx];
}
template <int FMT>
__device__ inline rs_f2 rs_cvt(typename RsRaw<FMT>::type raw)
{
    if constexpr (FMT == PSK_SOFT_FORMAT_CF32) {
        return raw;
    } else {
        const float2 v = pkt_cvt<FMT>(raw);
        return rs_f2{v.x, v.y};
    }
}
template <int FMT>
__device__ inline rs_f2 rs_load(const PSK_GLOBAL void *src, uint64_t idx)
{
    return rs_cvt<FMT>(rs_load_raw<FMT>(src, idx));
}

// s[idx] of the packet of d, 0 <= idx < d.n: converted and, if the packet is tuned, rotated by W(p), p = d.phase + idx * d.step
template <int FMT>
__device__ inline rs_f2 rs_sample(const ResampleDesc &d, const float *tab, uint64_t idx, uint64_t p)
{
    const rs_f2 x = rs_load<FMT>((const PSK_GLOBAL void *)d.src, idx * d.stride);
    if (!(d.flags & kResampleTuned))
        return x;
    float yr, yi;
    tune_rotate(tab, p, x.x, x.y, &yr, &yi);
    return rs_f2{yr, yi};
}

// entry q (0 .. 2, oldest first) of the history in front of the packet
__device__ inline rs_f2 rs_history(const ResampleDesc &d, uint32_t q)
{
    if (d.flags & kResampleRestart)
        return rs_f2{0.0f, 0.0f};
    return ((const PSK_GLOBAL rs_f2 *)d.hist_in)[q];
}

// the output at the instant t; s holds the inputs from index i0 - 3 on, i0 <= t >> 32
__device__ inline rs_f2 rs_output(const rs_f2 *s, uint64_t t, uint64_t i0)
{
    const uint32_t l = (uint32_t)((t >> 32) - i0);
    float w[4];
    resample_taps((uint32_t)t, w);
    const rs_f2 a = s[l], b = s[l + 1u], c = s[l + 2u], e = s[l + 3u];
    return rs_f2{resample_mix(w, a.x, b.x, c.x, e.x), resample_mix(w, a.y, b.y, c.y, e.y)};
}

// outputs [m0, m1) of the packet of d, m0 even, m1 - m0 <= kResamplePiece; a piece that would not fit the LDS (a step above
// 2^33: the entry refuses those) is left out by the whole workgroup
template <int FMT>
__device__ inline void rs_piece(const ResampleDesc &d, const float *tab, rs_f2 *s, uint64_t m0, uint64_t m1)
{
    const uint64_t t0 = d.pos + m0 * d.rstep, t1 = d.pos + (m1 - 1u) * d.rstep;
    const uint64_t i0 = t0 >> 32;
    const uint64_t cnt = (t1 >> 32) - i0 + 4u;  // s[i0 - 3 .. i(m1 - 1)]; i(m1 - 1) < d.n as t1 < d.n * 2^32
    if (cnt > kResampleInputs)
        return;
    {
        // LDS entry k holds s[i0 - 3 + k].  All of a lane's loads are issued before the first is used: the index of a lane with
        // nothing to load (k >= cnt, or an entry the history supplies) is clamped into the packet, so the loads are unconditional
        // within an iteration, and the iterations' bound is the workgroup's.
        const PSK_GLOBAL void *__restrict__ src = (const PSK_GLOBAL void *)d.src;
        const uint32_t iters = ((uint32_t)cnt + kRsThreads - 1u) / kRsThreads;
        typename RsRaw<FMT>::type v[kRsLoads];
#pragma unroll
        for (uint32_t j = 0; j < kRsLoads; j++) {
            const uint64_t q = i0 + threadIdx.x + j * kRsThreads;  // (index into history ‖ packet)
            const uint64_t idx = q < 3u ? 0u : q - 3u < d.n ? q - 3u : d.n - 1u;
            v[j] = j < iters ? rs_load_raw<FMT>(src, idx * d.stride) : typename RsRaw<FMT>::type{};
        }
        uint64_t p = d.phase + (i0 + threadIdx.x - 3u) * d.step;  // (mod 2^64; not used below index 0)
        const uint64_t adv = d.step * kRsThreads;
#pragma unroll
        for (uint32_t j = 0; j < kRsLoads; j++, p += adv) {
            const uint32_t k = threadIdx.x + j * kRsThreads;
            if (k >= (uint32_t)cnt)
                continue;
            rs_f2 x = rs_cvt<FMT>(v[j]);
            if (i0 + k < 3u) {
                x = rs_history(d, (uint32_t)(i0 + k));
            } else if (d.flags & kResampleTuned) {
                float yr, yi;
                tune_rotate(tab, p, x.x, x.y, &yr, &yi);
                x = rs_f2{yr, yi};
            }
            s[k] = x;
        }
    }
    __syncthreads();
    {
        PSK_GLOBAL rs_f2 *__restrict__ dst = (PSK_GLOBAL rs_f2 *)d.dst;
        uint64_t m = m0 + 2u * threadIdx.x;
        uint64_t t = d.pos + m * d.rstep;
        const uint64_t adv = d.rstep * (2u * kRsThreads);
        for (; m < m1; m += 2u * kRsThreads, t += adv) {
            const rs_f2 ya = rs_output(s, t, i0);
            if (m + 1u < m1) {
                const rs_f2 yb = rs_output(s, t + d.rstep, i0);
                *reinterpret_cast<PSK_GLOBAL rs_f4 *>(dst + m) = rs_f4{ya.x, ya.y, yb.x, yb.y};
            } else {
                dst[m] = ya;
            }
        }
    }
    __syncthreads();  // (the next piece overwrites s)
}

// the history behind the packet: the last three of (history in front ‖ s[0 .. n-1]), by lanes 0 .. 2
template <int FMT>
__device__ inline void rs_write_history(const ResampleDesc &d, const float *tab)
{
    if (threadIdx.x >= 3u)
        return;
    const uint64_t q = d.n + threadIdx.x;  // index into the joined sequence, whose last three are n .. n + 2
    const rs_f2 v = q < 3u ? rs_history(d, (uint32_t)q) : rs_sample<FMT>(d, tab, q - 3u, d.phase + (q - 3u) * d.step);
    ((PSK_GLOBAL rs_f2 *)d.hist_out)[threadIdx.x] = v;
}

template <int FMT>
__device__ inline void rs_packet(const ResampleDesc &d, const float *tab, rs_f2 *s, uint64_t n_pieces, bool owns_tail)
{
    for (uint64_t piece = blockIdx.y; piece < n_pieces; piece += gridDim.y) {
        const uint64_t m0 = piece * kResamplePiece;
        rs_piece<FMT>(d, tab, s, m0, d.n_out - m0 < kResamplePiece ? d.n_out : m0 + kResamplePiece);
    }
    if (owns_tail)
        rs_write_history<FMT>(d, tab);
}

// grid: x = descriptor (one packet), y = workgroups that share its pieces, piece p going to workgroup p % gridDim.y
__global__ __launch_bounds__(kRsThreads) void psk_resample_kernel(const ResampleDesc *__restrict__ desc, const float *__restrict__ d_tab)
{
    __shared__ __attribute__((aligned(16))) float lds[kTuneTableFloats + 2u * kResampleInputs];
    float *const tab = lds;
    rs_f2 *const s = reinterpret_cast<rs_f2 *>(lds + kTuneTableFloats);
    const ResampleDesc d = desc[blockIdx.x];
    const uint64_t n_pieces = (d.n_out + kResamplePiece - 1u) / kResamplePiece;
    const bool owns_tail = n_pieces ? (n_pieces - 1u) % gridDim.y == blockIdx.y : blockIdx.y == 0;
    if (blockIdx.y >= n_pieces && !owns_tail)
        return;  // (the whole workgroup: nothing of this packet is left for it)
    if (d.flags & kResampleTuned) {
        const PSK_GLOBAL rs_f4 *g = (const PSK_GLOBAL rs_f4 *)d_tab;
        rs_f4 *const t = reinterpret_cast<rs_f4 *>(tab);
#pragma unroll
        for (uint32_t k = 0; k < kTuneTableFloats / 4u / kRsThreads; k++) t[threadIdx.x + k * kRsThreads] = g[threadIdx.x + k * kRsThreads];
        __syncthreads();
    }
    switch (d.format) {
    case PSK_SOFT_FORMAT_CF32: rs_packet<PSK_SOFT_FORMAT_CF32>(d, tab, s, n_pieces, owns_tail); break;
    case PSK_SOFT_FORMAT_CS16: rs_packet<PSK_SOFT_FORMAT_CS16>(d, tab, s, n_pieces, owns_tail); break;
    case PSK_SOFT_FORMAT_CS8: rs_packet<PSK_SOFT_FORMAT_CS8>(d, tab, s, n_pieces, owns_tail); break;
    case PSK_SOFT_FORMAT_CF16: rs_packet<PSK_SOFT_FORMAT_CF16>(d, tab, s, n_pieces, owns_tail); break;
    default: break;
    }
}

hipError_t launch_resample(const ResampleDesc *desc, uint32_t n_desc, uint64_t max_n_out, const float *d_tab, hipStream_t stream)
{
    if (!n_desc)
        return hipSuccess;
    // as launch_tune shapes its grid: about 2048 workgroups in all (eight per CU), none without a piece of the longest packet
    uint64_t per = (max_n_out + kResamplePiece - 1u) / kResamplePiece;
    const uint64_t fill = (2048u + n_desc - 1u) / n_desc;
    per = per < fill ? per : fill;
    per = per < 1u ? 1u : per > 65535u ? 65535u : per;
    hipLaunchKernelGGL(psk_resample_kernel, dim3(n_desc, (uint32_t)per), dim3(kRsThreads), 0, stream, desc, d_tab);
    return hipGetLastError();
}

}  // namespace psk
