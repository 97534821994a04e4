// psk_quality.h -- what the host (psk_capi.cpp) and the reduction pass of PSK_SOFT_OPT_QUALITY (psk_quality.hip) share.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_soft_hip.h"

namespace psk {

// symbols of one segment of the fold: one wave, 32 iterations of a symbol pair a lane
constexpr uint32_t kQualitySegSymbols = 4096;

// One channel of one call for the pass: the call's WHOLE output rows.  The descriptors go up from pinned memory in front of
// the two launches.  flags: the PSK_SOFT_Q_* of the record; a pointer whose flag is off is not dereferenced.
struct QualityDesc {
    const float *soft;
    const float *phase;
    const int16_t *sidx;
    uint64_t n_symbols;
    uint64_t n_sidx;
    uint32_t seg0, n_seg;  // the channel's partials: [seg0, seg0 + n_seg) of the scratch (n_seg 0: nothing to fold)
    uint32_t channel;      // of the handle
    uint16_t M, S;
    uint8_t diff, flags, pad[2];
};

// what one segment adds up
struct QualityPartial {
    double sum_e, sum_e2, lock_re, lock_im;
    uint64_t n_finite, n_lock, index_changes;
};

// grid (max_seg, channels): the partials of every segment of every channel
hipError_t launch_quality_fold(const QualityDesc *desc, uint32_t nch, uint32_t max_seg, QualityPartial *part, hipStream_t stream);
// one wave per channel: the partials in segment order, the copied ends, the record
hipError_t launch_quality_join(const QualityDesc *desc, uint32_t nch, const QualityPartial *part, psk_soft_quality_t *records,
                               hipStream_t stream);

}  // namespace psk
