// psk_sync.h -- what the host (psk_capi.cpp) and the word search of psk_soft_sync_device (psk_sync.hip) share, and the per-symbol
// and per-window terms of include/psk_soft_hip.h ("where frames start"), which psk_soft_sync_host (host) and the kernels (device)
// both take from here.
#ifndef PSK_SYNC_H
#define PSK_SYNC_H

#include <float.h>
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_soft_hip.h"

namespace psk {

constexpr uint32_t kSyncMaxWord = PSK_SOFT_SYNC_MAX_WORD;
constexpr uint32_t kSyncSlots = PSK_SOFT_SYNC_SLOTS;
constexpr uint32_t kSyncHits = PSK_SOFT_SYNC_HITS;
constexpr uint32_t kSyncHist = kSyncMaxWord - 1u;       // symbols of a channel's history
constexpr uint32_t kSyncHistSlotFloats = 256;           // a history slot: 127 float2 in 1 KiB
constexpr uint32_t kSyncThreads = 256;
constexpr uint32_t kSyncPiece = 1024;                   // windows of one piece of the fold: a constant, never derived from the batch
constexpr uint32_t kSyncStage = kSyncPiece + kSyncMaxWord - 1u;  // symbols a piece stages at the most
constexpr uint64_t kSyncMaxN = (uint64_t)1 << 30;       // symbols of a row: fewer than this
static_assert(kSyncPiece % kSyncThreads == 0, "a wave owns a whole run of windows of a piece");

enum : uint32_t { kSyncData = 1u, kSyncRestart = 2u };  // SyncDesc::flags: the channel is searched; its history in front is zeros

// One covered channel of one call.  Without kSyncData the join writes the zero record and the fold has nothing to do.
struct SyncDesc {
    const float *soft;     // the row: n (re, im) pairs
    const float *word;     // L (re, im) pairs of the slot, device memory
    const float *hist_in;  // the channel's current history slot: 127 (re, im) pairs (not read with kSyncRestart)
    float *hist_out;       // ... and its other slot
    uint64_t n;
    int64_t p0;               // position of window 0: 0 with kSyncRestart, -(L - 1) otherwise
    uint32_t n_windows;
    uint32_t part0, n_piece;  // the channel's partials: [part0, part0 + n_piece) of the scratch; at least 1 for a searched channel
    uint32_t channel;         // of the handle
    uint32_t L;
    uint32_t flags;
    float threshold, Ew;
};

// what one piece leaves: hits[k] is written for k < min(n_hits, 16) only
struct SyncPartial {
    uint32_t n_valid, n_hits;
    psk_soft_sync_hit_t best;  // read if n_valid != 0
    psk_soft_sync_hit_t hits[kSyncHits];
};

#if defined(__HIPCC__)
#define PSK_SY_HD __host__ __device__
#else
#define PSK_SY_HD
#endif

PSK_SY_HD inline bool sy_finite(float v)
{
    return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u;
}

// te of one symbol
PSK_SY_HD inline float sy_energy(float xr, float xi) { return xr * xr + xi * xi; }

// one step j of a window: x = x[p + j], te = sy_energy(x), w = w[j]; first: j == 0, the accumulators start from the term
// (the units that include this are built with -ffp-contract=off)
PSK_SY_HD inline void sy_step(bool first, float xr, float xi, float te, float wr, float wi, float *cr, float *ci, float *e)
{
    const float tr = xr * wr + xi * wi;
    const float ti = xi * wr - xr * wi;
    *cr = first ? tr : *cr + tr;
    *ci = first ? ti : *ci + ti;
    *e = first ? te : *e + te;
}

// the metric of a window from its sums; returns whether the window is valid
PSK_SY_HD inline bool sy_metric(float cr, float ci, float e, float Ew, float *m)
{
    const float q = cr * cr + ci * ci;
    const float d = e * Ew;
    *m = q / d;
    return sy_finite(cr) && sy_finite(ci) && sy_finite(e) && sy_finite(q) && sy_finite(d) && d >= FLT_MIN;
}

// Ew of a word of L points
PSK_SY_HD inline float sy_word_energy(const float *w, uint32_t L)
{
    float s = 0.0f;
    for (uint32_t j = 0; j < L; j++) {
        const float t = w[2u * j] * w[2u * j] + w[2u * j + 1u] * w[2u * j + 1u];
        s = j ? s + t : t;
    }
    return s;
}

// windows of a row of n symbols, and the position of the first
inline uint32_t sync_windows(uint64_t n, uint32_t L, bool restart, int64_t *p0_out)
{
    const int64_t p0 = restart ? 0 : -(int64_t)(L - 1u);
    *p0_out = p0;
    const int64_t last = (int64_t)n - (int64_t)L;
    return last < p0 ? 0u : (uint32_t)(last - p0 + 1);
}

// grid (workgroups per channel, channels): the partials of every piece of every searched channel, the new histories
hipError_t launch_sync_fold(const SyncDesc *desc, uint32_t nch, uint32_t max_piece, SyncPartial *part, hipStream_t stream);
// one wave per channel: the partials in piece order, the record (or the zero record)
hipError_t launch_sync_join(const SyncDesc *desc, uint32_t nch, const SyncPartial *part, psk_soft_sync_t *records, hipStream_t stream);

}  // namespace psk
#endif
