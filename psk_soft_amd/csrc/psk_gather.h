// psk_gather.h -- descriptors of the gather pre-pass of psk_soft_process_device_strided (psk_gather.hip, psk_capi.cpp).
//
// A strided packet is one column of a frame-major matrix: sample k of the packet sits k * stride samples behind `data`.  The
// pass copies every such packet into a contiguous row of the handle's gather scratch, in the packet's own element type (2, 4 or
// 8 bytes a complex sample), and the ordinary call then runs on the rows.
#ifndef PSK_GATHER_H
#define PSK_GATHER_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace psk {

// A frame group: g packets of one format and one stride whose data pointers lie one sample apart -- g adjacent columns of an
// [n][stride] matrix.  Lengths may differ from column to column (chans[first + j].n); n_max is the longest.
struct GatherGroup {
    const void *src;   // sample 0 of the first column
    uint64_t stride;   // samples between consecutive frames
    uint64_t n_max;    // frames of the longest column
    uint64_t tile0;    // first tile of the group in the launch's tile list (ascending over the groups of a launch)
    uint32_t first;    // its columns are chans[first .. first + g)
    uint32_t g;
    uint32_t tiles_c;  // tiles across the columns: ceil(g / kGatherTile)
    uint32_t pad;
};
struct GatherChan {
    void *dst;   // the column's row in the gather scratch, 128-byte aligned
    uint64_t n;  // complex samples
};
// A packet outside every group (or in a group too narrow for the tile kernel): n samples, `stride` samples apart, to dst
struct GatherSingle {
    const void *src;
    void *dst;
    uint64_t stride, n;
};

constexpr uint32_t kGatherTile = 64;  // the tile kernel moves 64 columns x 64 frames at a time
// Groups narrower than this go to the plain strided gather, column by column: below 8 columns a frame's share of a 4-byte
// sample is under 32 bytes, and the tile kernel would fetch whole 128-byte lines for a quarter of their bytes or less while
// seven eighths of its lanes idle.
constexpr uint32_t kGatherMinGroup = 8;

// bytes: 2 (CS8), 4 (CS16, CF16) or 8 (CF32) per complex sample.  Descriptors in device memory.
hipError_t launch_gather_tiles(int bytes, const GatherGroup *groups, uint32_t n_groups, const GatherChan *chans, uint64_t n_tiles,
                               hipStream_t stream);
hipError_t launch_gather_singles(int bytes, const GatherSingle *desc, uint32_t n_desc, uint64_t max_n, hipStream_t stream);

}  // namespace psk
#endif
