// psk_demap.h -- what the host (psk_capi.cpp) and the demapper of psk_soft_demap_device (psk_demap.hip) share, and the per-symbol
// terms of include/psk_soft_hip.h ("frames as soft bits"), which psk_soft_demap_host (host) and the kernels (device) both take
// from here.
//
// The definition, restated.  A map is M = 2, 4 or 8 points p[0 .. M-1] with B = log2 M bit labels, bit j of a symbol being
// (label >> (B-1-j)) & 1.  Per symbol x of a segment with gain g and LLR scale s, every operation float32 and rounded once:
//     y.re = x.re*g.re - x.im*g.im     y.im = x.re*g.im + x.im*g.re     e = y.re*y.re + y.im*y.im
//     d[k] = (y.re - p[k].re)^2 + (y.im - p[k].im)^2,  k = 0 .. M-1
//     dmin = min d[k];  l[j] = min{d[k] : bit j of label k is 1} - min{d[k] : bit j is 0};  v[j] = l[j] * s
// A minimum is the FIRST minimum, k ascending from the set's first member: a later one must compare less, so a NaN in the first
// member stays.  Value i*B + j of the segment is v[j] of its symbol i: as it is (float32), or rintf (ties to even), clamped to
// -127 .. 127, a NaN written as 0 (int8); a float32 NaN is written as the quiet NaN 0x7fc00000.  A symbol is FINITE when y.re,
// y.im, e and dmin are; the record sums e and dmin of the finite symbols in doubles, in an order that depends on the symbol's
// index in the segment only: pieces of kDemapPiece symbols; lane t of 256 its symbols t, t + 256, t + 512, t + 768 from 0.0; a
// xor tree across each wave, offsets 32 .. 1; the four waves in order from wave 0's value; the pieces in ascending order from
// piece 0's.
#ifndef PSK_DEMAP_H
#define PSK_DEMAP_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "psk_soft_hip.h"

namespace psk {

constexpr uint32_t kDemapSlots = PSK_SOFT_DEMAP_SLOTS;
constexpr uint32_t kDemapMaxSegments = PSK_SOFT_DEMAP_MAX_SEGMENTS;
constexpr uint32_t kDemapMaxM = 8, kDemapMaxB = 3;
constexpr uint32_t kDemapFront = 127;                  // symbols in front of a row that PSK_SOFT_DEMAP_FRONT reaches: the sync history
constexpr uint32_t kDemapThreads = 256;
constexpr uint32_t kDemapPiece = 1024;                 // symbols of one piece of the fold: a constant, never derived from the batch
constexpr uint64_t kDemapMaxN = (uint64_t)1 << 30;     // symbols of a row: fewer than this
static_assert(kDemapPiece % kDemapThreads == 0, "a lane takes whole turns of a piece");

enum : uint32_t { kDemapData = 1u, kDemapI8 = 2u };    // DemapDesc::flags: the segment is demapped; its values are int8

// a map as the kernels read it: wave-uniform, 128 bytes
struct DemapMap {
    float p[2u * kDemapMaxM];  // (re, im) pairs
    uint32_t label[kDemapMaxM];
    uint32_t M, B;
    uint32_t pad[6];
};
static_assert(sizeof(DemapMap) == 128, "a map is 128 bytes");

// One segment of one call.  Without kDemapData the join writes the zero record and the fold has nothing to do.
struct DemapDesc {
    const float *soft;   // the row's symbol 0
    const float *front;  // the 127 (re, im) pairs in front of the row (read only where pos < 0); nullptr: zeros
    void *out;
    int64_t pos;         // first symbol of the segment, relative to the row; >= -127
    uint32_t count;
    uint32_t map;        // the slot
    uint32_t flags;
    uint32_t part0, n_piece;  // the segment's partials: [part0, part0 + n_piece) of the scratch
    float gain_re, gain_im, scale;
};
static_assert(sizeof(DemapDesc) == 64, "a descriptor is 64 bytes");

// what one piece leaves
struct DemapPartial {
    double sum_e, sum_err;
    uint32_t n_finite, n_clip, n_nan, pad;
};
static_assert(sizeof(DemapPartial) == 32, "a partial is 32 bytes");

#if defined(__HIPCC__)
#define PSK_DM_HD __host__ __device__
#else
#define PSK_DM_HD
#endif

PSK_DM_HD inline bool dm_finite(float v)
{
    return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u;
}

// One symbol x against the map: e, dmin and v[0 .. B-1]; returns whether the symbol is finite.
// (the units that include this are built with -ffp-contract=off)
PSK_DM_HD inline bool dm_symbol(const DemapMap &m, float xr, float xi, float gr, float gi, float scale, float *e_out, float *dmin_out,
                                float *v)
{
    const float yr = xr * gr - xi * gi;
    const float yi = xr * gi + xi * gr;
    const float e = yr * yr + yi * yi;
    float dmin = 0.0f, lo1[kDemapMaxB] = {}, lo0[kDemapMaxB] = {};
    uint32_t seen1 = 0, seen0 = 0;  // (bit j: the set of bit j has had its first member)
#pragma unroll
    for (uint32_t k = 0; k < kDemapMaxM; k++) {
        if (k >= m.M)
            break;
        const float dr = yr - m.p[2u * k], di = yi - m.p[2u * k + 1u];
        const float d = dr * dr + di * di;
        dmin = (k == 0u || d < dmin) ? d : dmin;
#pragma unroll
        for (uint32_t j = 0; j < kDemapMaxB; j++) {
            if (j >= m.B)
                break;
            // (the labels are the same for every symbol of a segment: the branch is uniform)
            if ((m.label[k] >> (m.B - 1u - j)) & 1u) {
                lo1[j] = (!((seen1 >> j) & 1u) || d < lo1[j]) ? d : lo1[j];
                seen1 |= 1u << j;
            } else {
                lo0[j] = (!((seen0 >> j) & 1u) || d < lo0[j]) ? d : lo0[j];
                seen0 |= 1u << j;
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kDemapMaxB; j++)
        if (j < m.B)
            v[j] = (lo1[j] - lo0[j]) * scale;
    *e_out = e, *dmin_out = dmin;
    return dm_finite(yr) && dm_finite(yi) && dm_finite(e) && dm_finite(dmin);
}

// v as the float32 the segment stores: v as it is, a NaN as the quiet NaN 0x7fc00000 -- the sign and the payload of a NaN that
// arithmetic hands on or makes are not pinned down by IEEE 754 and did differ between host and device; the bytes must not
PSK_DM_HD inline float dm_f32(float v) { return v != v ? __builtin_bit_cast(float, 0x7fc00000u) : v; }

// v as the int8 the segment stores: rintf (ties to even), clamped to -127 .. 127, a NaN as 0; counts what the clamp changed
PSK_DM_HD inline int32_t dm_i8(float v, uint32_t *n_clip)
{
    if (v != v)
        return 0;
    const float r = __builtin_rintf(v);
    if (r > 127.0f) {
        ++*n_clip;
        return 127;
    }
    if (r < -127.0f) {
        ++*n_clip;
        return -127;
    }
    return (int32_t)r;
}

inline uint32_t demap_pieces(uint32_t count) { return (count + kDemapPiece - 1u) / kDemapPiece; }

// grid (workgroups per segment, segments): the values of every piece of every demapped segment, its partial
hipError_t launch_demap_fold(const DemapDesc *desc, uint32_t nseg, uint32_t max_piece, const DemapMap *maps, DemapPartial *part,
                             hipStream_t stream);
// one wave per segment: the partials in piece order, the record (or the zero record)
hipError_t launch_demap_join(const DemapDesc *desc, uint32_t nseg, const DemapMap *maps, const DemapPartial *part,
                             psk_soft_demap_t *records, hipStream_t stream);

}  // namespace psk
#endif
