// psk_acquire.h -- what the host (psk_capi.cpp) and the acquire pass of psk_soft_acquire_device (psk_acquire.hip) share, and the
// per-sample and per-lag terms of include/psk_soft_hip.h ("carrier offset of a packet"), which psk_soft_acquire_host (host) and
// the kernels (device) both take from here.
#ifndef PSK_ACQUIRE_H
#define PSK_ACQUIRE_H

#include <hip/hip_runtime_api.h>
#include <float.h>
#include <stdint.h>
#include <string.h>

#include "psk_soft_hip.h"

namespace psk {

constexpr uint32_t kAcquireLags = 8;        // lags 1, 2, 4 .. 128
constexpr uint32_t kAcquireHalo = 128;      // the longest lag: samples in front of a piece that its products reach back to
constexpr uint32_t kAcquirePiece = 4096;    // samples of one piece of the fold: a constant, never derived from the batch
constexpr uint32_t kAcquireThreads = 256;

// One covered channel of one call.  flags: PSK_SOFT_A_DATA (a data record; without it the join writes the zero record and the fold
// has nothing to do), PSK_SOFT_A_TUNED (phase / step are applied).
struct AcquireDesc {
    const void *src;
    uint64_t stride;  // in complex samples of the format; 1: contiguous
    uint64_t n;       // complex samples
    uint64_t phase, step;
    uint32_t part0, n_piece;  // the packet's partials: [part0, part0 + n_piece) of the scratch
    uint32_t channel;         // of the handle
    uint16_t M;
    uint8_t format, flags;
};

// what one piece adds up: sum_re[8], sum_im[8], sum_e; n_pairs[8], n_valid
struct AcquirePartial {
    double d[2 * kAcquireLags + 1];
    uint32_t c[kAcquireLags + 1];
    uint32_t pad;  // (never written, never read)
};

#if defined(__HIPCC__)
#define PSK_ACQ_HD __host__ __device__
#else
#define PSK_ACQ_HD
#endif

PSK_ACQ_HD inline bool acq_finite(float v)
{
    return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u;
}

// One sample: P = log2(M) squarings.  Returns whether it is valid; then *e is its energy and (*ur, *ui) its unit M-th-power
// phasor.  An invalid sample's phasor is (0, 0): its lag products with the (finite) phasor of any valid sample are (+-0, +-0),
// which add nothing to a sum, while the product of two valid samples has modulus 1 to a few float roundings and is never (0, 0)
// -- that is how the kernel counts the pairs without keeping a flag per sample.
PSK_ACQ_HD inline bool acq_sample(float re, float im, int P, float *e_out, float *ur, float *ui)
{
    const float e = re * re + im * im;
    const float q = e * e;
    float pr = re, pi = im;
    for (int k = 0; k < P; k++) {
        const float r2 = pr * pr - pi * pi;
        const float i2 = pr * pi + pi * pr;
        pr = r2, pi = i2;
    }
    const float a = P == 1 ? e : P == 2 ? q : q * q;
    const bool ok = acq_finite(re) && acq_finite(im) && acq_finite(q) && acq_finite(pr) && acq_finite(pi) && acq_finite(a) && a >= FLT_MIN;
    *e_out = e;
    *ur = ok ? pr / a : 0.0f;
    *ui = ok ? pi / a : 0.0f;
    return ok;
}

// the product of sample k's phasor with the conjugate of sample k - L's
PSK_ACQ_HD inline void acq_lag(float ur, float ui, float vr, float vi, float *t_re, float *t_im)
{
    *t_re = ur * vr + ui * vi;
    *t_im = ui * vr - ur * vi;
}

// grid (max_piece, packets): the partials of every piece of every data packet.  d_tab: the tune tables in device memory, or
// nullptr when no packet of the launch is tuned.
hipError_t launch_acquire_fold(const AcquireDesc *desc, uint32_t nch, uint32_t max_piece, const float *d_tab, AcquirePartial *part,
                               hipStream_t stream);
// one wave per packet: the partials in piece order, the record (or the zero record)
hipError_t launch_acquire_join(const AcquireDesc *desc, uint32_t nch, const AcquirePartial *part, psk_soft_acquire_t *records,
                               hipStream_t stream);

}  // namespace psk
#endif
