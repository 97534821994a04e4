// psk_fir.h -- the filter pre-pass of psk_soft_process_device_filtered (psk_fir.hip, psk_capi.cpp): the decimating real-tap FIR of
// include/psk_soft_hip.h ("Filtered packets"), its arithmetic and its descriptors.
//
// Output m of a packet is the sum over the taps h[0 .. T-1] of h[j] * s[i - j], i = pos + m * D, accumulated in ascending j from
// h[0] * s[i]; s[-127 .. -1] is the channel's history.  fir_step() below IS one step of that sum: psk_soft_fir_apply (host) and
// the kernel (device) both call it; every operation is float32, rounded once, none fused (-ffp-contract=off).
#ifndef PSK_FIR_H
#define PSK_FIR_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_front_src.h"

namespace psk {

constexpr uint32_t kFirMaxTaps = 128, kFirSlots = 64, kFirMaxDecim = 16;
constexpr uint32_t kFirHist = kFirMaxTaps - 1u;     // samples of a channel's history
constexpr uint32_t kFirHistSlotFloats = 256;        // one slot of the history: 127 float2, padded to 1 KiB
constexpr uint32_t kFirWindow = 4096;               // inputs (float2) of one piece: the LDS window of a workgroup
constexpr uint64_t kFirMaxN = 1ull << 30;           // a filtered packet is shorter than this many samples

// One filtered packet: its source (io; phase / step of the NCO if kFrontTuned), and the filter's own: n_taps taps at `taps`
// (device memory), n_out float2 at io.dst, the history in front of the packet (127 float2, oldest first; zeros if kFrontRestart)
// and where the history behind it goes -- the channel's other slot, never the one read.
struct FirDesc {
    FrontIo io;
    uint32_t decim, pos, n_taps, pad;
    uint64_t n_out;
    const float *taps;
    const float *hist_in;
    float *hist_out;
};
static_assert(sizeof(FirDesc) == 104 && offsetof(FirDesc, io) == 0 && offsetof(FirDesc, decim) == 56 && offsetof(FirDesc, pos) == 60 &&
                  offsetof(FirDesc, n_taps) == 64 && offsetof(FirDesc, pad) == 68 && offsetof(FirDesc, n_out) == 72 &&
                  offsetof(FirDesc, taps) == 80 && offsetof(FirDesc, hist_in) == 88 && offsetof(FirDesc, hist_out) == 96,
              "FirDesc: the shared head, then the filter's own");

// outputs of a packet of n samples: the m with pos + m * decim < n
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t fir_count(uint64_t pos, uint64_t decim, uint64_t n)
{
    return pos >= n ? 0u : (n - pos + decim - 1u) / decim;
}

// outputs of one piece at the decimation D: those whose inputs fit the window behind the longest filter's reach; even, so a
// piece starts on a 16-byte boundary of its row
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr uint32_t fir_piece(uint32_t decim)
{
    return ((kFirWindow - kFirMaxTaps) / decim) & ~1u;
}

// one step of an output's sum, one component: the first (tap 0) starts it, every further one adds its product
#if defined(__HIPCC__)
__host__ __device__
#endif
inline float fir_step(bool first, float acc, float h, float s)
{
    const float p = h * s;
    return first ? p : acc + p;
}

// descriptors and tables (`d_tab`: the upload of tune_tables(); may be null if no descriptor is tuned) in device memory;
// max_pieces = the most pieces any packet of the launch has
hipError_t launch_fir(const FirDesc *desc, uint32_t n_desc, uint64_t max_pieces, const float *d_tab, hipStream_t stream);

}  // namespace psk
#endif
