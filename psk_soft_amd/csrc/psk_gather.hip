// psk_gather.hip -- the gather pre-pass of psk_soft_process_device_strided: packets that are columns of a frame-major matrix
// (a channelizer's output, [frame][channel]) copied into contiguous rows of the handle's gather scratch, in their own element
// type.  Nothing is converted: a complex sample moves as one 2-, 4- or 8-byte word (CS8, CS16, CF32), so a gathered CS16 / CS8
// row still reaches the in-place builds of the wave-scan kernels.
//
// Two kernels.  Frame groups (psk_gather.h) take an LDS-tiled transpose: loads with the lanes along the columns of a frame,
// stores with the lanes along time, both sides whole runs of contiguous bytes.  Everything else takes a plain strided gather,
// one lane one sample: every load touches a line of its own, the stores are coalesced -- slow and correct.
// Plain vector loads and stores only; the source is never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_front_src.h"
#include "psk_gather.h"

namespace psk {

// (PSK_GLOBAL, psk_front_src.h: the descriptors carry plain pointers; the kernels read and write through them as global memory --
// device memory or page-locked host memory, never LDS or scratch -- so that the compiler issues global, not flat, loads and stores)

// LDS tile: tile[column][frame], kGatherTile x kGatherTile samples, every row padded so that neither side conflicts on the 64
// banks of 4 bytes.  The load side writes tile[lane][f] (a column per lane): the row pitch in 4-byte words must be odd (4-byte
// samples: 65), odd in 8-byte words (8-byte samples: 65, two half-waves of 32 lanes each over all 64 banks), and for 2-byte
// samples 33 words (66 samples) sends the 64 lanes to 64 different banks.  The store side reads a row with consecutive lanes.
template <typename T> struct GatherPitch { static constexpr uint32_t v = kGatherTile + 1; };
template <> struct GatherPitch<uint16_t> { static constexpr uint32_t v = kGatherTile + 2; };

// grid: a few workgroups per CU whatever the shape; each walks the launch's tile list with the stride of the grid.  Tile `tl`
// belongs to the last group whose tile0 <= tl; inside a group the tiles run across the columns first, so that neighbouring
// workgroups read neighbouring pieces of the same frames.  256 threads = 4 waves; wave w loads frames w, w + 4, ... of the tile
// (lane = column: 64 columns x sizeof(T) contiguous bytes a frame, 128 bytes for the 2-byte samples) and stores columns
// w, w + 4, ... (lane = frame: 64 x sizeof(T) contiguous bytes of a row; the 2-byte samples go out in pairs, 4 bytes a lane,
// two columns a wave).  A lane loads only frames below its own column's length and stores only below it: ragged lengths read
// nothing behind a packet's last sample and write nothing behind its row.
template <typename T>
__global__ __launch_bounds__(256) void psk_gather_tile_kernel(const GatherGroup *__restrict__ groups, uint32_t n_groups,
                                                              const GatherChan *__restrict__ chans, uint64_t n_tiles)
{
    constexpr uint32_t P = GatherPitch<T>::v;
    __shared__ __attribute__((aligned(16))) T tile[kGatherTile * P];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        uint32_t lo = 0, hi = n_groups;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (groups[mid].tile0 <= tl)
                lo = mid;
            else
                hi = mid;
        }
        const GatherGroup g = groups[lo];
        const uint64_t local = tl - g.tile0;
        const uint32_t c0 = (uint32_t)(local % g.tiles_c) * kGatherTile;
        const uint64_t t0 = (local / g.tiles_c) * kGatherTile;
        const GatherChan *__restrict__ ch = chans + g.first;
        {
            const uint32_t c = c0 + lane;
            const uint64_t n_c = c < g.g ? ch[c].n : 0u;
            const PSK_GLOBAL T *__restrict__ src = (const PSK_GLOBAL T *)g.src + c;
            T v[kGatherTile / 4];
#pragma unroll
            for (uint32_t k = 0; k < kGatherTile / 4; k++) {
                const uint64_t t = t0 + w + 4u * k;
                v[k] = t < n_c ? src[t * g.stride] : T(0);
            }
#pragma unroll
            for (uint32_t k = 0; k < kGatherTile / 4; k++) tile[lane * P + w + 4u * k] = v[k];
        }
        __syncthreads();
        if constexpr (sizeof(T) == 2) {
            const uint32_t sub = lane >> 5, wd = lane & 31u;
            const uint64_t t = t0 + 2u * wd;
#pragma unroll
            for (uint32_t k = 0; k < kGatherTile / 8; k++) {
                const uint32_t j = 2u * (w + 4u * k) + sub;
                const uint32_t c = c0 + j;
                if (c < g.g) {
                    const GatherChan cc = ch[c];
                    const uint32_t v = *reinterpret_cast<const uint32_t *>(&tile[j * P + 2u * wd]);
                    PSK_GLOBAL uint16_t *d = (PSK_GLOBAL uint16_t *)cc.dst + t;
                    if (t + 1u < cc.n)
                        *(PSK_GLOBAL uint32_t *)d = v;  // (rows are 128-byte aligned and t is even)
                    else if (t < cc.n)
                        *d = (uint16_t)v;
                }
            }
        } else {
            const uint64_t t = t0 + lane;
#pragma unroll
            for (uint32_t k = 0; k < kGatherTile / 4; k++) {
                const uint32_t j = w + 4u * k;
                const uint32_t c = c0 + j;
                if (c < g.g) {
                    const GatherChan cc = ch[c];
                    if (t < cc.n)
                        ((PSK_GLOBAL T *)cc.dst)[t] = tile[j * P + lane];
                }
            }
        }
        __syncthreads();
    }
}

// grid: x = descriptor (one packet), y = pieces of it; a thread moves four samples an iteration, the loads issued before the
// stores.
template <typename T>
__global__ __launch_bounds__(256) void psk_gather_single_kernel(const GatherSingle *__restrict__ desc)
{
    const GatherSingle d = desc[blockIdx.x];
    const PSK_GLOBAL T *__restrict__ src = (const PSK_GLOBAL T *)d.src;
    PSK_GLOBAL T *__restrict__ dst = (PSK_GLOBAL T *)d.dst;
    const uint64_t step = (uint64_t)gridDim.y * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x;
    for (; i + 3 * step < d.n; i += 4 * step) {
        const T a = src[i * d.stride], b = src[(i + step) * d.stride], c = src[(i + 2 * step) * d.stride], e = src[(i + 3 * step) * d.stride];
        dst[i] = a;
        dst[i + step] = b;
        dst[i + 2 * step] = c;
        dst[i + 3 * step] = e;
    }
    for (; i < d.n; i += step) dst[i] = src[i * d.stride];
}

hipError_t launch_gather_tiles(int bytes, const GatherGroup *groups, uint32_t n_groups, const GatherChan *chans, uint64_t n_tiles,
                               hipStream_t stream)
{
    if (!n_groups || !n_tiles)
        return hipSuccess;
    // eight workgroups per CU (256 CUs) at the most, each walking the tile list
    const uint32_t grid = (uint32_t)(n_tiles < 2048u ? n_tiles : 2048u);
    if (bytes == 2)
        hipLaunchKernelGGL(psk_gather_tile_kernel<uint16_t>, dim3(grid), dim3(256), 0, stream, groups, n_groups, chans, n_tiles);
    else if (bytes == 4)
        hipLaunchKernelGGL(psk_gather_tile_kernel<uint32_t>, dim3(grid), dim3(256), 0, stream, groups, n_groups, chans, n_tiles);
    else if (bytes == 8)
        hipLaunchKernelGGL(psk_gather_tile_kernel<uint64_t>, dim3(grid), dim3(256), 0, stream, groups, n_groups, chans, n_tiles);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_gather_singles(int bytes, const GatherSingle *desc, uint32_t n_desc, uint64_t max_n, hipStream_t stream)
{
    if (!n_desc)
        return hipSuccess;
    // no piece shorter than 1024 samples (a thread's four)
    const dim3 grid(n_desc, front_grid_y((max_n + 1023u) / 1024u, n_desc));
    if (bytes == 2)
        hipLaunchKernelGGL(psk_gather_single_kernel<uint16_t>, grid, dim3(256), 0, stream, desc);
    else if (bytes == 4)
        hipLaunchKernelGGL(psk_gather_single_kernel<uint32_t>, grid, dim3(256), 0, stream, desc);
    else if (bytes == 8)
        hipLaunchKernelGGL(psk_gather_single_kernel<uint64_t>, grid, dim3(256), 0, stream, desc);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace psk
