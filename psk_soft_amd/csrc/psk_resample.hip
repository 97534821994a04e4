// psk_resample.hip -- the resample pre-pass of psk_soft_process_device_resampled: every resampled packet of a call, whatever its
// format and stride, read once, shifted in frequency if it is also tuned (psk_front_src.h: tune_rotate), interpolated at the call's
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

#include "psk_front_src.h"
#include "psk_resample.h"
#include "psk_soft_hip.h"
#include "psk_tune.h"

namespace psk {

constexpr uint32_t kRsThreads = 256;
constexpr uint32_t kRsLoads = (kResampleInputs + kRsThreads - 1u) / kRsThreads;  // inputs a lane loads per piece, at most
static_assert(kResamplePiece % 2u == 0, "a piece starts on an even output: the 16-byte stores are aligned");
static_assert(sizeof(float) * (kTuneTableFloats + 2u * kResampleInputs) <= 65536u, "tables and samples in static LDS");

// s[idx] of the packet of d, 0 <= idx < d.io.n: converted and, if the packet is tuned, rotated by W(p), p = d.io.phase + idx * d.io.step
template <int FMT>
__device__ inline f2 rs_sample(const ResampleDesc &d, const float *tab, uint64_t idx, uint64_t p)
{
    const f2 x = src_load<FMT>((const PSK_GLOBAL void *)d.io.src, idx * d.io.stride);
    return d.io.flags & kFrontTuned ? src_rotate(tab, p, x) : x;
}

// entry q (0 .. 2, oldest first) of the history in front of the packet
__device__ inline f2 rs_history(const ResampleDesc &d, uint32_t q)
{
    if (d.io.flags & kFrontRestart)
        return f2{0.0f, 0.0f};
    return ((const PSK_GLOBAL f2 *)d.hist_in)[q];
}

// the output at the instant t; s holds the inputs from index i0 - 3 on, i0 <= t >> 32
__device__ inline f2 rs_output(const f2 *s, uint64_t t, uint64_t i0)
{
    const uint32_t l = (uint32_t)((t >> 32) - i0);
    float w[4];
    resample_taps((uint32_t)t, w);
    const f2 a = s[l], b = s[l + 1u], c = s[l + 2u], e = s[l + 3u];
    return f2{resample_mix(w, a.x, b.x, c.x, e.x), resample_mix(w, a.y, b.y, c.y, e.y)};
}

// outputs [m0, m1) of the packet of d, m0 even, m1 - m0 <= kResamplePiece; a piece that would not fit the LDS (a step above
// 2^33: the entry refuses those) is left out by the whole workgroup
template <int FMT>
__device__ inline void rs_piece(const ResampleDesc &d, const float *tab, f2 *s, uint64_t m0, uint64_t m1)
{
    const uint64_t t0 = d.pos + m0 * d.rstep, t1 = d.pos + (m1 - 1u) * d.rstep;
    const uint64_t i0 = t0 >> 32;
    const uint64_t cnt = (t1 >> 32) - i0 + 4u;  // s[i0 - 3 .. i(m1 - 1)]; i(m1 - 1) < d.io.n as t1 < d.io.n * 2^32
    if (cnt > kResampleInputs)
        return;
    // LDS entry k holds s[i0 - 3 + k]
    src_fill<FMT, kRsThreads, kRsLoads>(
        d.io, (d.io.flags & kFrontTuned) != 0, tab, (int64_t)i0 - (int64_t)kResampleHist, (uint32_t)cnt,
        [&](int64_t g) { return rs_history(d, (uint32_t)(g + (int64_t)kResampleHist)); }, [&](uint32_t k, f2 x) { s[k] = x; });
    __syncthreads();
    {
        PSK_GLOBAL f2 *__restrict__ dst = (PSK_GLOBAL f2 *)d.io.dst;
        uint64_t m = m0 + 2u * threadIdx.x;
        uint64_t t = d.pos + m * d.rstep;
        const uint64_t adv = d.rstep * (2u * kRsThreads);
        for (; m < m1; m += 2u * kRsThreads, t += adv) {
            const f2 ya = rs_output(s, t, i0);
            if (m + 1u < m1) {
                const f2 yb = rs_output(s, t + d.rstep, i0);
                *reinterpret_cast<PSK_GLOBAL f4 *>(dst + m) = f4{ya.x, ya.y, yb.x, yb.y};
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
    if (threadIdx.x >= kResampleHist)
        return;
    const uint64_t q = d.io.n + threadIdx.x;  // index into the joined sequence, whose last three are n .. n + 2
    const f2 v = q < kResampleHist ? rs_history(d, (uint32_t)q)
                                   : rs_sample<FMT>(d, tab, q - kResampleHist, d.io.phase + (q - kResampleHist) * d.io.step);
    ((PSK_GLOBAL f2 *)d.hist_out)[threadIdx.x] = v;
}

template <int FMT>
__device__ inline void rs_packet(const ResampleDesc &d, const float *tab, f2 *s, uint64_t n_pieces, bool owns_tail)
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
    f2 *const s = reinterpret_cast<f2 *>(lds + kTuneTableFloats);
    const ResampleDesc d = desc[blockIdx.x];
    const uint64_t n_pieces = (d.n_out + kResamplePiece - 1u) / kResamplePiece;
    const bool owns_tail = n_pieces ? (n_pieces - 1u) % gridDim.y == blockIdx.y : blockIdx.y == 0;
    if (blockIdx.y >= n_pieces && !owns_tail)
        return;  // (the whole workgroup: nothing of this packet is left for it)
    if (d.io.flags & kFrontTuned) {
        src_tables_to_lds<kRsThreads>(tab, d_tab);
        __syncthreads();
    }
    src_dispatch(d.io.format, [&](auto fmt) { rs_packet<decltype(fmt)::value>(d, tab, s, n_pieces, owns_tail); });
}

hipError_t launch_resample(const ResampleDesc *desc, uint32_t n_desc, uint64_t max_n_out, const float *d_tab, hipStream_t stream)
{
    if (!n_desc)
        return hipSuccess;
    const uint32_t per = front_grid_y((max_n_out + kResamplePiece - 1u) / kResamplePiece, n_desc);
    hipLaunchKernelGGL(psk_resample_kernel, dim3(n_desc, per), dim3(kRsThreads), 0, stream, desc, d_tab);
    return hipGetLastError();
}

}  // namespace psk
