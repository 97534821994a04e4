// psk_frame.h -- what the host (psk_capi.cpp) and the kernels of psk_soft_frame_search_device and psk_soft_frame_cut_device
// (psk_frame.hip) share, and the terms of include/psk_soft_frame.h ("frames as aligned bytes"): the window of a stream formed from
// the aligned dwords that hold it, the verdict on a window, the source index of an output byte of the cut, the descriptors and the
// fold's partial.  Everything is integer arithmetic: the host computes with the same functions the kernels do.
#ifndef PSK_FRAME_H
#define PSK_FRAME_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_soft_hip.h"

namespace psk {

constexpr uint32_t kFrameSlots = PSK_SOFT_FRAME_SLOTS;
constexpr uint32_t kFrameMaxStreams = PSK_SOFT_FRAME_MAX_STREAMS;
constexpr uint32_t kFrameMaxFrames = PSK_SOFT_FRAME_MAX_FRAMES;
constexpr uint32_t kFrameMaxPeriod = PSK_SOFT_FRAME_MAX_PERIOD;
constexpr uint32_t kFrameMaxBits = PSK_SOFT_FRAME_MAX_BITS;
constexpr uint32_t kFrameMaxBytes = PSK_SOFT_FRAME_MAX_BYTES;
constexpr uint32_t kFrameMaxDelay = PSK_SOFT_FRAME_MAX_DELAY;
constexpr uint32_t kFrameHits = PSK_SOFT_FRAME_HITS;
constexpr uint32_t kFrameCutFlagMask = PSK_SOFT_FRAME_INVERT;
constexpr uint32_t kFrameTile = 64u;         // phases of a workgroup of the fold: one a lane of its one wave
constexpr uint32_t kFrameTurns = 256u;       // period 0: a tile is kFrameTile * kFrameTurns consecutive windows
constexpr uint32_t kFrameSearchGrid = 65535u;  // workgroups of the join, which take the streams w, w + grid, ...
constexpr uint32_t kFrameCutGrid = 65535u;     // workgroups of the cut, which take the frames w, w + grid, ...
constexpr uint32_t kFrameCutLanes = 256u;      // a workgroup of the cut
constexpr uint32_t kFrameNoDiff = 0xffffffffu;  // FrameSearchPartial::min_diff of a tile none of whose windows exist

enum : uint32_t { kFrameData = 1u };  // flags bit 0 of both descriptors: the record is written from data

// a word as the handle keeps it; length 0: the slot was never defined
struct FrameWord {
    uint64_t word, care;
    uint32_t length, ncare;
};
// a format as the handle keeps it; branches 0: the slot was never defined
struct FrameFormat {
    uint32_t branches, cell;
    bool table;
};

// One stream of one search call.  Without kFrameData the join writes the zero record and the fold has no tile of it.
struct FrameSearchDesc {
    const uint8_t *bits;
    uint64_t bit0;
    uint64_t word, care;
    uint32_t n_windows, length, ncare, max_diff;
    uint32_t period, flags;
    uint32_t part0, n_tile;  // the stream's partials: [part0, part0 + n_tile) of the call's, one a tile, in tile order
};
static_assert(sizeof(FrameSearchDesc) == 64, "a descriptor is 64 bytes");

// What a tile of the fold leaves.  Period P > 0: the tile's phases are [tile kFrameTile, ...) and best_* its best phase; P = 0: the
// tile's windows are [tile kFrameTile kFrameTurns, ...) and hits its first kFrameHits hits in position order.
struct FrameSearchPartial {
    uint32_t n_hit[2];
    uint32_t min_diff, min_pos, min_pol;  // kFrameNoDiff: no window
    uint32_t best_phase, best_score, best_inv;
    uint32_t n_listed;
    uint32_t pad[3];
    psk_soft_frame_hit_t hits[kFrameHits];
};
static_assert(sizeof(FrameSearchPartial) == 176, "a partial is 176 bytes");

// One frame of one cut call.  Without kFrameData the kernel writes the zero record and nothing else.
struct FrameCutDesc {
    const uint8_t *bits;
    uint64_t bit;
    uint8_t *out;
    uint32_t n_bytes, branches;
    uint32_t stride;   // M B: the stream bytes a branch lies behind the one before it; 0: no interleaver
    uint32_t branch0;
    uint32_t flags;    // kFrameData | the frame's PSK_SOFT_FRAME_* flags << 1: the record's flags as they are
    uint32_t table;    // 1 + the slot whose table applies; 0: the identity
    uint32_t span;
    uint32_t pad[3];
};
static_assert(sizeof(FrameCutDesc) == 64, "a descriptor is 64 bytes");

#if defined(__HIPCC__)
#define PSK_FRAME_HD __host__ __device__
#else
#define PSK_FRAME_HD
#endif

PSK_FRAME_HD inline uint32_t frame_popcount(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }

// a dword as it was loaded (little-endian) with its first byte most significant: stream order
PSK_FRAME_HD inline uint32_t frame_msb_first(uint32_t le) { return __builtin_bswap32(le); }

// The `length` (1 .. 64) bits from bit `o` (0 .. 31) of the 96 bits w0 w1 w2 (each MSB first), right-aligned.  w1 counts only when
// o + length > 32 and w2 only when o + length > 64: a caller that has not read them passes anything.
PSK_FRAME_HD inline uint64_t frame_window(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t o, uint32_t length)
{
    const uint64_t hi = ((uint64_t)w0 << 32) | w1;
    const uint64_t top = o ? (hi << o) | ((uint64_t)w2 >> (32u - o)) : hi;  // the 64 bits from bit o, left-aligned
    return top >> (64u - length);
}

// the verdict on a window with d of the C care positions differing: its diff, its polarity, whether it is a hit
struct FrameVerdict {
    uint32_t diff, pol;
    bool hit;
};
PSK_FRAME_HD inline FrameVerdict frame_verdict(uint32_t d, uint32_t ncare, uint32_t max_diff)
{
    FrameVerdict v;
    v.pol = ncare - d < d ? 1u : 0u;
    v.diff = v.pol ? ncare - d : d;
    v.hit = v.diff <= max_diff;
    return v;
}

// the key by which the smallest diff, then the smallest position wins; the polarity rides in bit 0
PSK_FRAME_HD inline uint64_t frame_min_key(uint32_t diff, uint32_t pos, uint32_t pol) { return ((uint64_t)diff << 40) | ((uint64_t)pos << 1) | pol; }
// the key by which the greatest score, then the smallest phase wins (phase < 2^20)
PSK_FRAME_HD inline uint64_t frame_best_key(uint32_t score, uint32_t phase) { return ((uint64_t)score << 20) | (0xfffffu - phase); }

// the cut: the stream byte that output byte i comes from
PSK_FRAME_HD inline uint32_t frame_source(uint32_t i, uint32_t branch0, uint32_t branches, uint32_t stride)
{
    return stride ? i + ((branch0 + i) % branches) * stride : i;
}

// what psk_soft_frame_word_define refuses of a word
inline bool frame_word_ok(uint32_t length, uint64_t word, uint64_t care)
{
    if (length < 1u || length > 64u || !care)
        return false;
    const uint64_t above = length == 64u ? 0ull : ~0ull << length;
    return !((word | care) & above);
}
// what psk_soft_frame_format_define refuses of a format
inline bool frame_format_ok(uint32_t branches, uint32_t cell)
{
    return branches >= 1u && branches <= 255u && cell <= 255u && (uint64_t)branches * (branches - 1u) * cell <= kFrameMaxDelay;
}
// M B, or 0 without an interleaver
inline uint32_t frame_stride(uint32_t branches, uint32_t cell) { return branches > 1u ? branches * cell : 0u; }
// 1 + the greatest source index of a frame.  A branch lies M B >= B bytes behind the one before it and the last B outputs are
// less than B apart, so a frame of at least B bytes reaches furthest with its last output on the last branch.
inline uint32_t frame_span(uint32_t branches, uint32_t cell, uint32_t branch0, uint32_t n_bytes)
{
    const uint32_t stride = frame_stride(branches, cell);
    if (!stride)
        return n_bytes;
    if (n_bytes >= branches)
        return n_bytes - 1u - (branch0 + n_bytes) % branches + (branches - 1u) * stride + 1u;
    uint32_t top = 0;
    for (uint32_t i = 0; i < n_bytes; i++) {
        const uint32_t q = frame_source(i, branch0, branches, stride);
        top = q > top ? q : top;
    }
    return top + 1u;
}
// the tiles of a stream's fold
inline uint32_t frame_tiles(uint32_t n_windows, uint32_t period)
{
    if (!n_windows)
        return 0u;
    if (!period)
        return (uint32_t)(((uint64_t)n_windows + kFrameTile * kFrameTurns - 1u) / (kFrameTile * kFrameTurns));
    const uint32_t phases = period < n_windows ? period : n_windows;  // (a phase at or above n_windows has no window)
    return (phases + kFrameTile - 1u) / kFrameTile;
}

// The fold: a workgroup of one wave per tile of the call (n_part of them; it finds its stream by its first partial); then the
// join, a wave per stream, which stores the records whole.
hipError_t launch_frame_search(const FrameSearchDesc *desc, uint32_t nstream, uint32_t n_part, FrameSearchPartial *part,
                               psk_soft_frame_search_t *records, hipStream_t stream);
// Workgroup w cuts the frames w, w + grid, ... of the call.  tables: 256 bytes a slot.
hipError_t launch_frame_cut(const FrameCutDesc *desc, uint32_t nframe, uint32_t grid, const uint8_t *tables, psk_soft_frame_cut_t *records,
                            hipStream_t stream);

}  // namespace psk
#endif
