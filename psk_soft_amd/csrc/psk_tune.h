// psk_tune.h -- the tune pre-pass of psk_soft_process_device_tuned (psk_tune.hip, psk_capi.cpp): the per-packet frequency shift
// of include/psk_soft_hip.h ("Tuned packets"), its tables and its descriptors.
//
// Sample k of a tuned packet is converted to float as its format defines and multiplied by the phasor W(p_k) of the phase word
// p_k = phase + k * step (turns x 2^64, mod 2^64).  W comes from two tables of 1024 entries, a coarse one indexed by the top ten
// bits of p_k and a fine one by the next ten; the product of the two entries and the product with the sample are plain float32
// operations, each rounded once, none fused.  tune_rotate() below IS that definition: psk_soft_tune_apply (host) and the kernel
// (device) both call it, on the same tables, which the host builds once per process with lm_sincosf (glibc 2.35's sinf / cosf,
// psk_libm.h) and uploads once per handle.
#ifndef PSK_TUNE_H
#define PSK_TUNE_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace psk {

constexpr uint32_t kTuneTable = 1024;  // entries of either table; the tables lie back to back: [coarse | fine], (cos, sin) pairs
constexpr uint32_t kTuneTableFloats = 4u * kTuneTable;

// One tuned packet: n complex samples of `format`, `stride` samples apart at src, become n float2 at dst.
struct TuneDesc {
    const void *src;
    float *dst;       // 128-byte aligned, in the handle's gather scratch
    uint64_t stride;  // 1: contiguous (the caller's packet, or its row behind the tile gather)
    uint64_t n;
    uint64_t phase, step;
    uint32_t format;  // PSK_SOFT_FORMAT_*
    uint32_t pad;
};

// y = x * W(p), tab = [coarse | fine]
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void tune_rotate(const float *tab, uint64_t p, float xr, float xi, float *yr, float *yi)
{
    const uint32_t top = (uint32_t)(p >> 44);  // the top 20 bits; the rest of the phase word is truncated
    const float *const c = tab + 2u * (top >> 10), *const f = tab + 2u * (kTuneTable + (top & (kTuneTable - 1u)));
    const float cr = c[0], ci = c[1], fr = f[0], fi = f[1];
    const float wr = cr * fr - ci * fi, wi = cr * fi + ci * fr;
    *yr = xr * wr - xi * wi;
    *yi = xr * wi + xi * wr;
}

// the tables, built at the first call (host memory, kTuneTableFloats floats, valid for the life of the process)
const float *tune_tables();

// descriptors and tables (`d_tab`: the upload of tune_tables()) in device memory; max_n = the longest packet of the launch
hipError_t launch_tune(const TuneDesc *desc, uint32_t n_desc, uint64_t max_n, const float *d_tab, hipStream_t stream);

}  // namespace psk
#endif
