// psk_acquire.hip -- psk_soft_acquire_device: one look at a packet per channel, one psk_soft_acquire_t per channel.
//
// The record holds the lag products of the samples' unit M-th-power phasors (include/psk_soft_hip.h, "carrier offset of a
// packet"); the host turns it into a carrier offset (psk_soft_acquire_derive).  One pass over the packets, two kernels:
//
//   fold   grid (pieces, packets), one workgroup of 256 lanes per piece of kAcquirePiece samples of one packet.
//          Stage 1: the piece and the kAcquireHalo samples in front of it are read once (psk_pkt_cvt.h for the four formats; a
//          lane takes two adjacent samples: one 16-byte load of a contiguous CF32 row, 8 bytes of CS16 / CF16, 4 of CS8), tuned
//          inline (tune_rotate on the tables in LDS, as psk_tune.hip does), and every sample's unit phasor u_k goes into LDS --
//          (0, 0) for an invalid sample and for the halo of the packet's first piece.  The lane adds the energies of its valid
//          samples.
//          Stage 2: lane t takes the samples t, t + 256, ... of the piece and forms their eight lag products out of LDS into
//          double accumulators, without a branch: a product with an invalid sample is (+-0, +-0) and adds nothing; the pairs
//          are counted per wave by a ballot of the products that are not (0, 0) (psk_acquire.h: acq_sample).
//          A fixed xor-tree across each wave, the four waves in order: one partial per piece.
//   join   one wave per packet: the partials in a fixed order, the record; the zero record for a packet without data.
//
// Which lane adds which sample, and in which order, depends on the sample's index in the packet and on the packet's length only
// -- not on the format, the stride, the alignment, the batch or the grid --, so the same samples give the same bytes.  No
// floating-point atomics.  The per-sample arithmetic (psk_acquire.h) is float32, rounded once (the unit is built with
// -ffp-contract=off), the division correctly rounded, denormals kept.  Plain vector loads and stores only; the packets are
// never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_acquire.h"
#include "psk_front_src.h"
#include "psk_tune.h"

namespace psk {

namespace {

typedef uint32_t a_u2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kWaves = kAcquireThreads / 64u;
constexpr uint32_t kSums = 2u * kAcquireLags + 1u, kCounts = kAcquireLags + 1u;

__device__ __forceinline__ double a_wave_sum(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// lanes of the wave for which `p` holds: the same number in every lane
__device__ __forceinline__ uint32_t a_wave_count(bool p) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); }
// a float the compiler takes for a scalar of unknown origin: keeps the lag products of stage 2 out of packed instructions, which
// cost gfx950 as much as the two scalar ones they stand for (Makefile, -fno-slp-vectorize) and here compute lanes nobody reads
__device__ __forceinline__ float a_scalar(float v)
{
    asm("" : "+v"(v));
    return v;
}

// samples k and k + 1 (k even) of a packet of format FMT as they lie, `pair`: both exist and one load may take them
template <int FMT>
__device__ __forceinline__ void a_load2(const PSK_GLOBAL void *src, uint64_t stride, uint64_t k, bool two, bool wide, f2 *x0, f2 *x1)
{
    *x1 = f2{0.0f, 0.0f};
    if constexpr (FMT == PSK_SOFT_FORMAT_CF32) {
        const PSK_GLOBAL f2 *p = reinterpret_cast<const PSK_GLOBAL f2 *>(src);
        if (two && wide) {
            const f4 z = *reinterpret_cast<const PSK_GLOBAL f4 *>(p + k);
            *x0 = f2{z.x, z.y}, *x1 = f2{z.z, z.w};
            return;
        }
        *x0 = p[k * stride];
        if (two)
            *x1 = p[(k + 1u) * stride];
    } else if constexpr (FMT == PSK_SOFT_FORMAT_CS8) {
        const PSK_GLOBAL uint16_t *p = reinterpret_cast<const PSK_GLOBAL uint16_t *>(src);
        uint32_t w0, w1 = 0;
        if (two && wide) {
            const uint32_t z = *reinterpret_cast<const PSK_GLOBAL uint32_t *>(p + k);
            w0 = z & 0xffffu, w1 = z >> 16;
        } else {
            w0 = p[k * stride];
            if (two)
                w1 = p[(k + 1u) * stride];
        }
        const float2 a = pkt_cvt<FMT>(w0), b = pkt_cvt<FMT>(w1);
        *x0 = f2{a.x, a.y}, *x1 = f2{b.x, b.y};
    } else {
        const PSK_GLOBAL uint32_t *p = reinterpret_cast<const PSK_GLOBAL uint32_t *>(src);
        uint32_t w0, w1 = 0;
        if (two && wide) {
            const a_u2 z = *reinterpret_cast<const PSK_GLOBAL a_u2 *>(p + k);
            w0 = z.x, w1 = z.y;
        } else {
            w0 = p[k * stride];
            if (two)
                w1 = p[(k + 1u) * stride];
        }
        const float2 a = pkt_cvt<FMT>(w0), b = pkt_cvt<FMT>(w1);
        *x0 = f2{a.x, a.y}, *x1 = f2{b.x, b.y};
    }
}

// Stage 1 of a piece: samples [start, hi) into LDS slot k + halo - lo (start = lo - halo, or 0 in the packet's first piece: even),
// zeros behind them up to `end` (the piece rounded up to whole turns of stage 2); energies of [lo, hi) into se, their count --
// the same in every lane of the wave -- into nv.
template <int FMT, bool TAB>
__device__ __forceinline__ void a_stage1(const AcquireDesc &d, const float *tab, f2 *u, uint64_t start, uint64_t lo, uint64_t hi, uint64_t end,
                                         int P, double &se, uint32_t &nv)
{
    const PSK_GLOBAL void *__restrict__ src = (const PSK_GLOBAL void *)d.src;
    const bool tuned = TAB && (d.flags & PSK_SOFT_A_TUNED) != 0;
    // one load for the pair: a contiguous row whose pairs are aligned to their size (start and every k below are even)
    const uint32_t pair_bytes = FMT == PSK_SOFT_FORMAT_CF32 ? 16u : FMT == PSK_SOFT_FORMAT_CS8 ? 4u : 8u;
    const bool wide = d.stride == 1 && ((uintptr_t)d.src & (pair_bytes - 1u)) == 0;
    const uint64_t step = d.step;
    uint64_t p = d.phase + (start + 2u * threadIdx.x) * step;
    const uint64_t adv = step * (2u * kAcquireThreads);
    for (uint64_t k = start + 2u * threadIdx.x; k < end; k += 2u * kAcquireThreads, p += adv) {  // (end - start is a multiple of 128)
        const bool one = k < hi, two = k + 1u < hi;
        f2 x0 = f2{0.0f, 0.0f}, x1 = f2{0.0f, 0.0f};
        if (one)
            a_load2<FMT>(src, d.stride, k, two, wide, &x0, &x1);
        if (tuned) {
            x0 = src_rotate(tab, p, x0);
            x1 = src_rotate(tab, p + step, x1);
        }
        float e0, e1, r0, i0, r1, i1;
        // (a sample that is not there is (0, 0): invalid, its phasor (0, 0))
        const bool ok0 = acq_sample(x0.x, x0.y, P, &e0, &r0, &i0);
        const bool ok1 = acq_sample(x1.x, x1.y, P, &e1, &r1, &i1);
        const uint32_t s = (uint32_t)(k + kAcquireHalo - lo);
        *reinterpret_cast<f4 *>(u + s) = f4{r0, i0, r1, i1};  // (s is even)
        const bool in = k >= lo;  // (lo is even: a pair never straddles it)
        se += (double)(in && ok0 ? e0 : 0.0f);
        se += (double)(in && ok1 ? e1 : 0.0f);
        nv += a_wave_count(in && ok0) + a_wave_count(in && ok1);
    }
}

}  // namespace

// TAB: the launch has tuned packets (the workgroup copies the tables into LDS)
template <bool TAB>
__global__ __launch_bounds__(kAcquireThreads) void psk_acquire_fold_kernel(const AcquireDesc *__restrict__ desc, uint32_t nch,
                                                                           const float *__restrict__ d_tab,
                                                                           AcquirePartial *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float tab[TAB ? kTuneTableFloats : 4u];
    __shared__ __attribute__((aligned(16))) f2 u[kAcquireHalo + kAcquirePiece];
    __shared__ double red_d[kWaves][kSums];
    __shared__ uint32_t red_c[kWaves][kCounts];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    if constexpr (TAB)
        src_tables_to_lds<kAcquireThreads>(tab, d_tab);
    for (uint32_t c = blockIdx.y; c < nch; c += gridDim.y) {
        const AcquireDesc d = desc[c];
        // (uniform for the workgroup, like every branch on the descriptor below)
        if (!(d.flags & PSK_SOFT_A_DATA) || blockIdx.x >= d.n_piece)
            continue;
        const uint64_t lo = (uint64_t)blockIdx.x * kAcquirePiece;
        const uint64_t hi = d.n - lo < kAcquirePiece ? d.n : lo + kAcquirePiece;
        const uint64_t start = lo ? lo - kAcquireHalo : 0u;
        const uint64_t end = lo + (hi - lo + kAcquireThreads - 1u) / kAcquireThreads * kAcquireThreads;
        const int P = d.M == 2 ? 1 : d.M == 4 ? 2 : 3;
        __syncthreads();  // (the tables are in place; the LDS of the packet before is read out)
        if (!lo && t < kAcquireHalo)
            u[t] = f2{0.0f, 0.0f};  // (nothing lies in front of the packet: no pairs)
        double se = 0.0;
        uint32_t nv = 0;
        src_dispatch(d.format, [&](auto fmt) { a_stage1<decltype(fmt)::value, TAB>(d, tab, u, start, lo, hi, end, P, se, nv); });
        __syncthreads();
        // stage 2: sample k of the piece sits in slot k + halo - lo, its partner of lag L in the slot L in front of it
        double sr[kAcquireLags], si[kAcquireLags];
        uint32_t np[kAcquireLags];
#pragma unroll
        for (uint32_t j = 0; j < kAcquireLags; j++) sr[j] = si[j] = 0.0, np[j] = 0;
        // (whole turns: the slots behind the packet's end hold zeros, and the trip count is the same for every lane)
        const uint32_t turns = (uint32_t)(end - lo) / kAcquireThreads;
        for (uint32_t turn = 0; turn < turns; turn++) {
            const uint32_t s = kAcquireHalo + turn * kAcquireThreads + t;
            const f2 a = u[s];
            const float ar = a_scalar(a.x), ai = a_scalar(a.y);
#pragma unroll
            for (uint32_t j = 0; j < kAcquireLags; j++) {
                const f2 b = u[s - (1u << j)];
                float tr, ti;
                acq_lag(ar, ai, a_scalar(b.x), a_scalar(b.y), &tr, &ti);
                // (a pair of valid samples: acq_sample's a >= FLT_MIN keeps |u| within a few ulp of 1, so |t| is within a few
                // ulp of 1 as well and one of tr, ti is far from 0; any other pair has a (0, 0) factor and t = (+-0, +-0))
                sr[j] += (double)tr;
                si[j] += (double)ti;
                np[j] += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(tr != 0.0f) | __builtin_amdgcn_ballot_w64(ti != 0.0f));
            }
        }
        // the wave's lanes by the fixed tree, then the waves in order
#pragma unroll
        for (uint32_t j = 0; j < kAcquireLags; j++) {
            const double r = a_wave_sum(sr[j]), i = a_wave_sum(si[j]);
            if (lane == 0)
                red_d[wave][j] = r, red_d[wave][kAcquireLags + j] = i, red_c[wave][j] = np[j];
        }
        {
            const double e = a_wave_sum(se);
            if (lane == 0)
                red_d[wave][2u * kAcquireLags] = e, red_c[wave][kAcquireLags] = nv;
        }
        __syncthreads();
        PSK_GLOBAL AcquirePartial *const out = (PSK_GLOBAL AcquirePartial *)part + (d.part0 + blockIdx.x);
        if (t < kSums) {
            double v = red_d[0][t];
            for (uint32_t w = 1; w < kWaves; w++) v += red_d[w][t];
            out->d[t] = v;
        } else if (t >= 64u && t < 64u + kCounts) {
            uint32_t v = 0;
            for (uint32_t w = 0; w < kWaves; w++) v += red_c[w][t - 64u];
            out->c[t - 64u] = v;
        }
    }
}

__global__ __launch_bounds__(64) void psk_acquire_join_kernel(const AcquireDesc *__restrict__ desc, uint32_t nch,
                                                              const AcquirePartial *__restrict__ part,
                                                              psk_soft_acquire_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const AcquireDesc d = desc[c];
        const bool data = (d.flags & PSK_SOFT_A_DATA) != 0;
        double s[kSums];
        uint64_t n[kCounts];
#pragma unroll
        for (uint32_t j = 0; j < kSums; j++) s[j] = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < kCounts; j++) n[j] = 0;
        // lane l adds the partials l, l + 64, ... in that order; then the fixed tree
        for (uint32_t k = lane; data && k < d.n_piece; k += 64u) {
            const PSK_GLOBAL AcquirePartial *const p = (const PSK_GLOBAL AcquirePartial *)part + (d.part0 + k);
#pragma unroll
            for (uint32_t j = 0; j < kSums; j++) s[j] += p->d[j];
#pragma unroll
            for (uint32_t j = 0; j < kCounts; j++) n[j] += p->c[j];
        }
#pragma unroll
        for (uint32_t j = 0; j < kSums; j++) s[j] = a_wave_sum(s[j]);
#pragma unroll
        for (uint32_t j = 0; j < kCounts; j++)
            for (int off = 32; off >= 1; off >>= 1) n[j] += (uint64_t)__shfl_xor((long long)n[j], off);
        if (lane != 0)
            continue;
        psk_soft_acquire_t r = {};  // (pad stays zero; lane 0 alone stores the 224 bytes)
        if (data) {
            r.n_samples = d.n;
            r.n_valid = n[kAcquireLags];
            for (uint32_t j = 0; j < kAcquireLags; j++) {
                r.n_pairs[j] = n[j];
                r.sum_re[j] = s[j];
                r.sum_im[j] = s[kAcquireLags + j];
            }
            r.sum_e = s[2u * kAcquireLags];
            r.constelationSize = d.M;
            r.flags = d.flags;
        }
        records[d.channel] = r;
    }
}

hipError_t launch_acquire_fold(const AcquireDesc *desc, uint32_t nch, uint32_t max_piece, const float *d_tab, AcquirePartial *part,
                               hipStream_t stream)
{
    if (!nch || !max_piece)
        return hipSuccess;
    const dim3 grid(max_piece, nch < 65535u ? nch : 65535u);
    if (d_tab)
        hipLaunchKernelGGL(psk_acquire_fold_kernel<true>, grid, dim3(kAcquireThreads), 0, stream, desc, nch, d_tab, part);
    else
        hipLaunchKernelGGL(psk_acquire_fold_kernel<false>, grid, dim3(kAcquireThreads), 0, stream, desc, nch, d_tab, part);
    return hipGetLastError();
}

hipError_t launch_acquire_join(const AcquireDesc *desc, uint32_t nch, const AcquirePartial *part, psk_soft_acquire_t *records,
                               hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    hipLaunchKernelGGL(psk_acquire_join_kernel, dim3(nch < 65535u ? nch : 65535u), dim3(64), 0, stream, desc, nch, part, records);
    return hipGetLastError();
}

}  // namespace psk
