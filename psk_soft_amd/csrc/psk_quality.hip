// psk_quality.hip -- PSK_SOFT_OPT_QUALITY: the reduction pass behind a call, one psk_soft_quality_t per channel.
//
// The record stands in for what the reference offers a person who wants to know whether a channel holds a signal: its two
// debug ports, phase (reference cpp/psk_soft.cpp:482) and sampleIndex (:466), watched in a plot.  Here the GPU reduces the
// rows the call has just written -- soft 8 bytes and sampleIndex 2 bytes a symbol, phase at its two ends only -- while they
// are still in HBM.  Memory-bound; two kernels:
//
//   fold   grid (segments, channels), one wave per segment of kQualitySegSymbols symbols of one channel.  A lane takes
//          consecutive symbol pairs (16-byte loads of soft where the row is 16-byte aligned, 8-byte otherwise; one 4-byte load
//          of the two indices), its predecessor's index comes through a lane shift, the segment's first through one extra
//          2-byte load.  Double accumulators per lane, a fixed xor-tree across the wave, one partial per segment.
//   join   one wave per channel: the partials in a fixed order, the copied first / last values, the record.  Channels that
//          emitted nothing get their zero record here, in stream order.
//
// The arithmetic per symbol is fixed by include/psk_soft_hip.h (float32, every operation rounded once -- the unit is built with
// -ffp-contract=off --, correctly rounded division, denormals kept) so that a test can restate it exactly; the order of the
// double additions is fixed by the code below (no floating-point atomics): the same call gives the same bytes.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "psk_quality.h"

namespace psk {

namespace {

// The row pointers come out of a descriptor, so the compiler takes them for generic and would emit FLAT loads; they are global
// memory (device or page-locked host), and the loads below say so (as the wave-scan kernels do, psk_wave.h).
#define PSK_Q_GLOBAL __attribute__((address_space(1)))
typedef float q_f2 __attribute__((ext_vector_type(2)));
typedef float q_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool q_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct QAcc {
    double se = 0.0, sq = 0.0, lr = 0.0, li = 0.0;
    uint32_t nf = 0, nl = 0, chg = 0;
};

// one soft symbol; P = log2(M) squarings for the lock sums, 0 = none
__device__ __forceinline__ void q_symbol(QAcc &a, float re, float im, int P)
{
    const float e = re * re + im * im;
    const float q = e * e;
    if (!(q_finite(re) && q_finite(im) && q_finite(q)))
        return;
    a.se += (double)e;
    a.sq += (double)q;
    a.nf++;
    if (!P)
        return;
    float pr = re, pi = im;
    for (int k = 0; k < P; k++) {
        const float r2 = pr * pr - pi * pi;
        const float i2 = pr * pi + pi * pr;
        pr = r2, pi = i2;
    }
    const float m = P == 1 ? e : P == 2 ? q : q * q;
    if (q_finite(pr) && q_finite(pi) && q_finite(m) && m >= FLT_MIN) {
        a.lr += (double)(pr / m);
        a.li += (double)(pi / m);
        a.nl++;
    }
}

__device__ __forceinline__ double q_wave_sum(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ uint32_t q_wave_sum(uint32_t v)
{
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}
__device__ __forceinline__ uint64_t q_wave_sum64(uint64_t v)
{
    for (int off = 32; off >= 1; off >>= 1) v += (uint64_t)__shfl_xor((long long)v, off);
    return v;
}

}  // namespace

__global__ __launch_bounds__(64) void psk_quality_fold_kernel(const QualityDesc *__restrict__ desc, uint32_t nch,
                                                              QualityPartial *__restrict__ part)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.y; c < nch; c += gridDim.y) {
        const QualityDesc d = desc[c];
        if (blockIdx.x >= d.n_seg)  // (wave-uniform, like every branch on the descriptor below)
            continue;
        const uint64_t lo = (uint64_t)blockIdx.x * kQualitySegSymbols;
        const uint64_t hi = lo + kQualitySegSymbols < d.n_symbols ? lo + kQualitySegSymbols : d.n_symbols;
        const bool has_soft = (d.flags & PSK_SOFT_Q_SOFT) != 0, has_idx = (d.flags & PSK_SOFT_Q_INDEX) != 0;
        const uint64_t idx_hi = hi < d.n_sidx ? hi : d.n_sidx;
        const int P = !(d.flags & PSK_SOFT_Q_LOCK) ? 0 : d.M == 2 ? 1 : d.M == 4 ? 2 : d.M == 8 ? 3 : 0;
        const bool al16 = ((uintptr_t)d.soft & 15u) == 0;
        const PSK_Q_GLOBAL q_f2 *soft = (const PSK_Q_GLOBAL q_f2 *)d.soft;
        const PSK_Q_GLOBAL int16_t *sidx = (const PSK_Q_GLOBAL int16_t *)d.sidx;
        QAcc a;
        // the index in front of the segment (lane 0's predecessor in the first iteration; later lane 63's last)
        int carry = has_idx && lo > 0 && lo - 1 < idx_hi ? (int)sidx[lo - 1] : 0;
        for (uint64_t base = lo; base < hi; base += 128u) {
            const uint64_t i0 = base + 2u * lane;
            if (has_soft) {
                if (i0 + 1 < hi) {
                    q_f4 z;
                    if (al16) {
                        z = *(const PSK_Q_GLOBAL q_f4 *)(soft + i0);
                    } else {
                        const q_f2 u = soft[i0], v = soft[i0 + 1];
                        z = q_f4{u.x, u.y, v.x, v.y};
                    }
                    q_symbol(a, z.x, z.y, P);
                    q_symbol(a, z.z, z.w, P);
                } else if (i0 < hi) {
                    const q_f2 u = soft[i0];
                    q_symbol(a, u.x, u.y, P);
                }
            }
            if (has_idx) {
                const bool w0 = i0 < idx_hi, w1 = i0 + 1 < idx_hi;
                int s0 = 0, s1 = 0;
                if (w1) {  // (rows are 4-byte aligned and i0 is even)
                    const uint32_t v = *(const PSK_Q_GLOBAL uint32_t *)(sidx + i0);
                    s0 = (int16_t)(v & 0xffffu), s1 = (int16_t)(v >> 16);
                } else if (w0) {
                    s0 = sidx[i0];
                }
                const int last = w1 ? s1 : s0;
                const int up = __shfl_up(last, 1);
                const int pred = lane == 0 ? carry : up;
                if (w0 && i0 >= 1 && s0 != pred)
                    a.chg++;
                if (w1 && s1 != s0)
                    a.chg++;
                carry = __shfl(last, 63);
            }
        }
        const double se = q_wave_sum(a.se), sq = q_wave_sum(a.sq), lr = q_wave_sum(a.lr), li = q_wave_sum(a.li);
        const uint32_t nf = q_wave_sum(a.nf), nl = q_wave_sum(a.nl), chg = q_wave_sum(a.chg);
        if (lane == 0) {
            QualityPartial p;
            p.sum_e = se, p.sum_e2 = sq, p.lock_re = lr, p.lock_im = li;
            p.n_finite = nf, p.n_lock = nl, p.index_changes = chg;
            part[d.seg0 + blockIdx.x] = p;
        }
    }
}

__global__ __launch_bounds__(64) void psk_quality_join_kernel(const QualityDesc *__restrict__ desc, uint32_t nch,
                                                              const QualityPartial *__restrict__ part,
                                                              psk_soft_quality_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const QualityDesc d = desc[c];
        double se = 0.0, sq = 0.0, lr = 0.0, li = 0.0;
        uint64_t nf = 0, nl = 0, chg = 0;
        // lane l adds the partials l, l + 64, ... in that order; then the fixed tree
        for (uint32_t s = lane; s < d.n_seg; s += 64u) {
            const QualityPartial p = part[d.seg0 + s];
            se += p.sum_e, sq += p.sum_e2, lr += p.lock_re, li += p.lock_im;
            nf += p.n_finite, nl += p.n_lock, chg += p.index_changes;
        }
        se = q_wave_sum(se), sq = q_wave_sum(sq), lr = q_wave_sum(lr), li = q_wave_sum(li);
        nf = q_wave_sum64(nf), nl = q_wave_sum64(nl), chg = q_wave_sum64(chg);
        if (lane != 0)
            continue;
        psk_soft_quality_t r = {};
        if (d.n_symbols) {
            r.n_symbols = d.n_symbols;
            r.n_finite = nf, r.n_lock = nl, r.index_changes = chg;
            r.sum_e = se, r.sum_e2 = sq, r.sum_lock_re = lr, r.sum_lock_im = li;
            if (d.flags & PSK_SOFT_Q_PHASE) {
                r.phase_first = d.phase[0];
                r.phase_last = d.phase[d.n_symbols - 1];
            }
            if (d.flags & PSK_SOFT_Q_INDEX) {
                r.index_first = d.sidx[0];
                r.index_last = d.sidx[d.n_sidx - 1];
            }
            r.constelationSize = d.M, r.samplesPerBaud = d.S;
            r.differentialDecoding = d.diff, r.flags = d.flags;
        }
        records[d.channel] = r;
    }
}

hipError_t launch_quality_fold(const QualityDesc *desc, uint32_t nch, uint32_t max_seg, QualityPartial *part, hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    hipLaunchKernelGGL(psk_quality_fold_kernel, dim3(max_seg ? max_seg : 1u, nch < 65535u ? nch : 65535u), dim3(64), 0, stream, desc, nch,
                       part);
    return hipGetLastError();
}

hipError_t launch_quality_join(const QualityDesc *desc, uint32_t nch, const QualityPartial *part, psk_soft_quality_t *records,
                               hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    hipLaunchKernelGGL(psk_quality_join_kernel, dim3(nch), dim3(64), 0, stream, desc, nch, part, records);
    return hipGetLastError();
}

}  // namespace psk
