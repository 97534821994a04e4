// psk_resample.h -- the resample pre-pass of psk_soft_process_device_resampled (psk_resample.hip, psk_capi.cpp): the fractional
// resampler of include/psk_soft_hip.h ("Resampled packets"), its tap arithmetic and its descriptors.
//
// An output at the instant t (input samples x 2^32, counted from the packet's sample 0) is the cubic Lagrange polynomial through
// the four samples s[i-3] .. s[i], i = t >> 32, evaluated mu = frac(t) behind s[i-2]: a pure delay of two input samples, so a
// packet never needs its successor.  resample_taps() and resample_mix() below ARE that definition: psk_soft_resample_apply
// (host) and the kernel (device) both call them; every operation is float32, rounded once, none fused (-ffp-contract=off).
#ifndef PSK_RESAMPLE_H
#define PSK_RESAMPLE_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_front_src.h"

namespace psk {

// Outputs of one piece of a packet (one pass of a workgroup over its LDS); even.  Samples (16 KiB) and the tune tables (16 KiB)
// leave room for four workgroups on a CU.
constexpr uint32_t kResamplePiece = 1024;
// inputs a piece can need: at the largest step (2 input samples per output) 2 * piece + 3, rounded up to a whole 16 bytes
constexpr uint32_t kResampleInputs = 2u * kResamplePiece + 4u;
constexpr uint64_t kResampleStepMin = 1ull << 31, kResampleStepMax = 1ull << 33, kResamplePosMax = 1ull << 33;
constexpr uint64_t kResampleMaxN = 1ull << 30;  // a resampled packet is shorter than this many samples

// a channel's history: two slots of kResampleHist float2 (a launch reads the current one and writes the other), padded to 64 bytes
constexpr uint32_t kResampleHist = 3, kResampleHistSlotFloats = 2u * kResampleHist, kResampleHistFloats = 16;

// One resampled packet: its source (io; phase / step of the NCO if kFrontTuned), and the resampler's own: n_out float2 at io.dst,
// the history in front of the packet (three float2, oldest first; zeros if kFrontRestart) and where the history behind it goes --
// the channel's other slot, never the one read.
struct ResampleDesc {
    FrontIo io;
    uint64_t pos, rstep, n_out;
    const float *hist_in;
    float *hist_out;
};
// (tests/prepass_probe.py mirrors the layout)
static_assert(sizeof(ResampleDesc) == 96 && offsetof(ResampleDesc, io) == 0 && offsetof(ResampleDesc, pos) == 56 &&
                  offsetof(ResampleDesc, rstep) == 64 && offsetof(ResampleDesc, n_out) == 72 && offsetof(ResampleDesc, hist_in) == 80 &&
                  offsetof(ResampleDesc, hist_out) == 88,
              "ResampleDesc: the shared head, then the resampler's own");

// outputs of a packet of n samples: the m with pos + m * step < n * 2^32 (n < 2^30, step >= 2^31: nothing overflows)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t resample_count(uint64_t pos, uint64_t step, uint64_t n)
{
    const uint64_t end = n << 32;
    return pos >= end ? 0u : (end - pos + step - 1u) / step;
}

// the four weights of the instant whose fraction is `frac` (the low 32 bits of t): mu = the top 24 bits, exact in a float
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void resample_taps(uint32_t frac, float *w)
{
    const float a = (float)(frac >> 8) * 0x1p-24f;
    const float b = a - 1.0f, c = a - 2.0f, d = a + 1.0f;
    w[0] = ((a * b) * c) * (float)(-1.0 / 6.0);
    w[1] = ((d * b) * c) * 0.5f;
    w[2] = ((d * a) * c) * -0.5f;
    w[3] = ((d * a) * b) * (float)(1.0 / 6.0);
}

// one component of the output: s0 .. s3 = s[i-3] .. s[i]
#if defined(__HIPCC__)
__host__ __device__
#endif
inline float resample_mix(const float *w, float s0, float s1, float s2, float s3)
{
    return ((w[0] * s0 + w[1] * s1) + w[2] * s2) + w[3] * s3;
}

// descriptors and tables (`d_tab`: the upload of tune_tables(); may be null if no descriptor is tuned) in device memory;
// max_n_out = the most outputs any packet of the launch has
hipError_t launch_resample(const ResampleDesc *desc, uint32_t n_desc, uint64_t max_n_out, const float *d_tab, hipStream_t stream);

}  // namespace psk
#endif
