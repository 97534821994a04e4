// psk_frame.hip -- psk_soft_frame_search_device and psk_soft_frame_cut_device: a known word found in the decoded bits of a stream,
// one psk_soft_frame_search_t per stream, and byte frames cut from a stream at any bit, one psk_soft_frame_cut_t per frame
// (include/psk_soft_frame.h, "frames as aligned bytes"; psk_frame.h holds the terms the host shares).
//
// The search is a fold and a join.
//   fold   A workgroup of one wave per tile of the call.  With a period P a tile is kFrameTile phases of one stream: lane l owns the
//          phase tile kFrameTile + l and walks the windows phase + m P, m = 0, 1, ...  Without one a tile is kFrameTile kFrameTurns
//          consecutive windows and lane l walks the windows base + l + m kFrameTile.  Either way the lanes of a turn read
//          neighbouring bits: a window is formed from the one, two or three aligned dwords that hold it (byte-reversed to
//          MSB-first, funnel-shifted: frame_window), so a turn of the wave touches one or two cache lines, which the next turns hit
//          again while P is small and which the other tiles of the stream share otherwise.  The reads go straight to global
//          memory: a staged piece in LDS would be filled once and read once by a lane (a window belongs to one phase), so it
//          saves no traffic the cache does not already save.  The count is a popcount of (window ^ word) & care.  A tile leaves
//          its counts, its minimum, its best phase and (P = 0) its first kFrameHits hits, listed in position order by ballot.
//   join   One wave per stream: the partials merged in tile order -- sums, the minimum by (diff, position), the best phase by
//          (score, smallest phase), the lists concatenated --; with P > 0 the best phase walked once more for its first
//          kFrameHits hits; the record stored whole.
// No atomics: every tie is settled by position through the keys of psk_frame.h.
//
// The cut is one launch of workgroups of kFrameCutLanes lanes; workgroup w takes the frames w, w + grid, ...  A lane takes aligned
// dwords of the output: where all four bytes are the frame's it stores the dword, at the ragged head and tail single bytes.
// Without an interleaver the four source bytes are 32 consecutive stream bits (two dwords, one funnel shift); with one every
// byte is gathered on its own.  The table sits in LDS (256 bytes, loaded when a frame's table differs from the workgroup's last):
// its lookups are random bytes, which LDS serves without taking vector-memory slots from the gather's loads.
// Plain vector loads and stores only; streams and tables are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_frame.h"

namespace psk {

namespace {

#define PSK_FRAME_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint32_t frame_wave_sum(uint32_t v)
{
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}
__device__ __forceinline__ uint64_t frame_shfl_xor64(uint64_t v, int off)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t frame_wave_min(uint64_t v)
{
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = frame_shfl_xor64(v, off);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t frame_wave_max(uint64_t v)
{
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = frame_shfl_xor64(v, off);
        v = o > v ? o : v;
    }
    return v;
}
// the value of the first lane for which `mine` holds (some lane's must)
__device__ __forceinline__ uint32_t frame_first_of(bool mine, uint32_t v)
{
    const uint64_t m = __ballot(mine);
    return (uint32_t)__shfl((int)v, m ? __builtin_ctzll(m) : 0);
}

// A stream as the kernels read it: the aligned dwords from `base` on, stream bit 0 being bit g0 (0 .. 38) of them.
struct FrameBits {
    const PSK_FRAME_GLOBAL uint32_t *base;
    uint32_t g0;
};
__device__ __forceinline__ FrameBits frame_bits(const uint8_t *bits, uint64_t bit0)
{
    const uintptr_t a = (uintptr_t)bits;
    FrameBits b;
    b.base = (const PSK_FRAME_GLOBAL uint32_t *)(a & ~(uintptr_t)3);
    b.g0 = (uint32_t)(a & 3u) * 8u + (uint32_t)bit0;
    return b;
}
// the `length` stream bits from bit p on: only dwords that hold one of them are read
__device__ __forceinline__ uint64_t frame_read(const FrameBits &b, uint32_t p, uint32_t length)
{
    const uint32_t g = b.g0 + p, idx = g >> 5, o = g & 31u;
    const uint32_t w0 = frame_msb_first(b.base[idx]);
    uint32_t w1 = 0, w2 = 0;
    if (o + length > 32u)
        w1 = frame_msb_first(b.base[idx + 1u]);
    if (o + length > 64u)
        w2 = frame_msb_first(b.base[idx + 2u]);
    return frame_window(w0, w1, w2, o, length);
}

__device__ __forceinline__ uint64_t frame_hit_word(uint32_t pos, uint32_t diff, uint32_t pol)
{
    return (uint64_t)pos | ((uint64_t)diff << 32) | ((uint64_t)pol << 48);  // psk_soft_frame_hit_t as it lies in memory
}

// One turn of a walk: the verdict on window p of the lanes that `have` one, its hit listed behind the `listed` so far (in lane
// order, which is position order) while there is room.  Wave-uniform control: every lane of the wave calls it.
template <class List>
__device__ __forceinline__ FrameVerdict frame_turn(const FrameSearchDesc &d, const FrameBits &b, bool have, uint32_t p, uint32_t lane, bool list,
                                                   uint32_t &listed, List put)
{
    FrameVerdict v = {0u, 0u, false};
    if (have) {
        const uint64_t win = frame_read(b, p, d.length);
        v = frame_verdict(frame_popcount((win ^ d.word) & d.care), d.ncare, d.max_diff);
    }
    if (list && listed < kFrameHits) {
        const bool hit = have && v.hit;
        const uint64_t m = __ballot(hit);
        if (m) {
            const uint32_t at = listed + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (hit && at < kFrameHits)
                put(at, frame_hit_word(p, v.diff, v.pol));
            const uint32_t all = listed + (uint32_t)__popcll(m);
            listed = all < kFrameHits ? all : kFrameHits;
        }
    }
    return v;
}

__global__ __launch_bounds__(64) void psk_frame_fold_kernel(const FrameSearchDesc *__restrict__ desc, uint32_t nstream,
                                                            FrameSearchPartial *__restrict__ part)
{
    const uint32_t id = blockIdx.x, lane = threadIdx.x;
    // the stream of this tile: the last one whose first partial is at or below id (a stream without tiles shares its first
    // partial with the next one that has some)
    uint32_t lo = 0, hi = nstream - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (desc[mid].part0 <= id)
            lo = mid;
        else
            hi = mid - 1u;
    }
    const FrameSearchDesc d = desc[lo];
    const uint32_t tile = id - d.part0;
    if (!(d.flags & kFrameData) || tile >= d.n_tile)
        return;
    const FrameBits b = frame_bits(d.bits, d.bit0);
    const uint32_t P = d.period;
    const uint32_t first = P ? tile * kFrameTile + lane : tile * (kFrameTile * kFrameTurns) + lane;
    const uint32_t stride = P ? P : kFrameTile;
    const uint64_t tile_end = (uint64_t)tile * (kFrameTile * kFrameTurns) + kFrameTile * kFrameTurns;
    const uint32_t end = P || tile_end > d.n_windows ? d.n_windows : (uint32_t)tile_end;
    const bool owns = !P || first < P;
    PSK_FRAME_GLOBAL uint64_t *const hits = (PSK_FRAME_GLOBAL uint64_t *)part[id].hits;

    uint32_t nh0 = 0, nh1 = 0, listed = 0;
    uint64_t min_key = ~0ull;
    for (uint64_t p = first;; p += stride) {
        const bool have = owns && p < end;
        if (!__ballot(have))
            break;
        const FrameVerdict v = frame_turn(d, b, have, (uint32_t)p, lane, !P, listed, [&](uint32_t at, uint64_t w) { hits[at] = w; });
        if (have) {
            const uint64_t key = frame_min_key(v.diff, (uint32_t)p, v.pol);
            min_key = key < min_key ? key : min_key;
            nh0 += v.hit && !v.pol ? 1u : 0u;
            nh1 += v.hit && v.pol ? 1u : 0u;
        }
    }
    const uint64_t my_best = P && owns ? frame_best_key(nh0 + nh1, first) : 0ull;
    const uint64_t best = frame_wave_max(my_best);
    const uint32_t inv = frame_first_of(my_best == best, nh1);
    const uint32_t s0 = frame_wave_sum(nh0), s1 = frame_wave_sum(nh1);
    min_key = frame_wave_min(min_key);
    if (lane < 12u) {
        const bool any = min_key != ~0ull;
        uint32_t w = 0;
        w = lane == 0u ? s0 : lane == 1u ? s1 : w;
        w = lane == 2u ? (any ? (uint32_t)(min_key >> 40) : kFrameNoDiff) : w;
        w = lane == 3u && any ? (uint32_t)(min_key >> 1) & 0x7fffffffu : w;
        w = lane == 4u && any ? (uint32_t)min_key & 1u : w;
        w = lane == 5u && P ? 0xfffffu - ((uint32_t)best & 0xfffffu) : w;
        w = lane == 6u && P ? (uint32_t)(best >> 20) : w;
        w = lane == 7u && P ? inv : w;
        w = lane == 8u ? listed : w;
        ((PSK_FRAME_GLOBAL uint32_t *)&part[id])[lane] = w;
    }
}

__global__ __launch_bounds__(64) void psk_frame_join_kernel(const FrameSearchDesc *__restrict__ desc, uint32_t nstream,
                                                            const FrameSearchPartial *__restrict__ part,
                                                            psk_soft_frame_search_t *__restrict__ records)
{
    __shared__ uint64_t s_hits[kFrameHits];
    const uint32_t lane = threadIdx.x;
    for (uint32_t s = blockIdx.x; s < nstream; s += gridDim.x) {
        const FrameSearchDesc d = desc[s];
        PSK_FRAME_GLOBAL uint32_t *const rec = (PSK_FRAME_GLOBAL uint32_t *)(records + s);
        if (!(d.flags & kFrameData)) {  // (uniform) the zero record
            if (lane < sizeof(psk_soft_frame_search_t) / 4u)
                rec[lane] = 0u;
            continue;
        }
        __syncthreads();  // (one wave: the last stream's list is stored)
        if (lane < kFrameHits)
            s_hits[lane] = 0ull;
        __syncthreads();
        const uint32_t P = d.period;
        const FrameSearchPartial *const mine = part + d.part0;
        uint32_t nh0 = 0, nh1 = 0, my_inv = 0;
        uint64_t min_key = ~0ull, my_best = 0ull;
        for (uint32_t t = lane; t < d.n_tile; t += 64u) {
            const FrameSearchPartial &q = mine[t];
            nh0 += q.n_hit[0], nh1 += q.n_hit[1];
            if (q.min_diff != kFrameNoDiff) {
                const uint64_t key = frame_min_key(q.min_diff, q.min_pos, q.min_pol);
                min_key = key < min_key ? key : min_key;
            }
            if (P) {
                const uint64_t key = frame_best_key(q.best_score, q.best_phase);
                if (key > my_best)
                    my_best = key, my_inv = q.best_inv;
            }
        }
        nh0 = frame_wave_sum(nh0), nh1 = frame_wave_sum(nh1);
        min_key = frame_wave_min(min_key);
        const uint64_t best = frame_wave_max(my_best);
        const bool folded = P && d.n_tile;
        const uint32_t best_inv = folded ? frame_first_of(my_best == best, my_inv) : 0u;
        const uint32_t best_phase = folded ? 0xfffffu - ((uint32_t)best & 0xfffffu) : 0u;
        const uint32_t best_score = folded ? (uint32_t)(best >> 20) : 0u;

        uint32_t listed = 0;
        if (!P) {
            // the tiles' lists one behind the other, 64 tiles a step
            for (uint32_t c = 0; c < d.n_tile && listed < kFrameHits; c += 64u) {
                const uint32_t t = c + lane, n = t < d.n_tile ? mine[t].n_listed : 0u;
                uint32_t incl = n;
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t below = (uint32_t)__shfl_up((int)incl, off);
                    incl += lane >= (uint32_t)off ? below : 0u;
                }
                const uint32_t at = listed + incl - n;
                for (uint32_t j = 0; j < n && at + j < kFrameHits; j++)
                    s_hits[at + j] = ((const PSK_FRAME_GLOBAL uint64_t *)mine[t].hits)[j];
                const uint32_t all = listed + (uint32_t)__shfl((int)incl, 63);
                listed = all < kFrameHits ? all : kFrameHits;
            }
        } else if (best_score) {
            // the best phase once more, 64 of its windows a turn
            const FrameBits b = frame_bits(d.bits, d.bit0);
            for (uint64_t p = best_phase + (uint64_t)lane * P; listed < kFrameHits; p += 64ull * P) {
                const bool have = p < d.n_windows;
                if (!__ballot(have))
                    break;
                frame_turn(d, b, have, (uint32_t)p, lane, true, listed, [&](uint32_t at, uint64_t w) { s_hits[at] = w; });
            }
        }
        __syncthreads();
        if (lane < 16u) {
            const bool any = min_key != ~0ull;
            uint32_t w = 0;
            w = lane == 0u ? d.flags : lane == 1u ? d.length : lane == 2u ? d.n_windows : lane == 3u ? nh0 : lane == 4u ? nh1 : w;
            w = lane == 5u && any ? (uint32_t)(min_key >> 40) : w;
            w = lane == 6u && any ? (uint32_t)(min_key >> 1) & 0x7fffffffu : w;
            w = lane == 7u && any ? (uint32_t)min_key & 1u : w;
            w = lane == 8u ? best_phase : lane == 9u ? best_score : lane == 10u ? best_inv : lane == 11u ? listed : w;
            rec[lane] = w;
            ((PSK_FRAME_GLOBAL uint64_t *)rec)[8u + lane] = s_hits[lane];
        }
    }
}

// the stream byte whose first bit is bit g of the stream's dwords
__device__ __forceinline__ uint32_t frame_byte(const FrameBits &b, uint32_t g)
{
    const uint32_t idx = g >> 5, o = g & 31u;
    const uint32_t w0 = frame_msb_first(b.base[idx]);
    if (o <= 24u)
        return (w0 >> (24u - o)) & 0xffu;
    const uint32_t w1 = frame_msb_first(b.base[idx + 1u]);
    return ((w0 << (o - 24u)) | (w1 >> (56u - o))) & 0xffu;
}

__global__ __launch_bounds__(256) void psk_frame_cut_kernel(const FrameCutDesc *__restrict__ desc, uint32_t nframe,
                                                            const uint8_t *__restrict__ tables, psk_soft_frame_cut_t *__restrict__ records)
{
    __shared__ uint8_t s_table[256];
    __shared__ uint32_t s_ones[kFrameCutLanes / 64u];
    const uint32_t tid = threadIdx.x;
    uint32_t table = 0;  // 1 + the slot whose table s_table holds
    for (uint32_t f = blockIdx.x; f < nframe; f += gridDim.x) {
        const FrameCutDesc d = desc[f];
        PSK_FRAME_GLOBAL uint32_t *const rec = (PSK_FRAME_GLOBAL uint32_t *)(records + f);
        if (!(d.flags & kFrameData)) {  // (uniform) the zero record
            if (tid < sizeof(psk_soft_frame_cut_t) / 4u)
                rec[tid] = 0u;
            continue;
        }
        __syncthreads();  // (the last frame's table lookups and count are behind every wave)
        if (d.table && d.table != table) {  // (uniform)
            s_table[tid] = ((const PSK_FRAME_GLOBAL uint8_t *)tables)[(size_t)(d.table - 1u) * 256u + tid];
            table = d.table;
            __syncthreads();
        }
        const FrameBits b = frame_bits(d.bits, d.bit);
        const uintptr_t oa = (uintptr_t)d.out;
        const uint32_t off = (uint32_t)(oa & 3u), n = d.n_bytes;
        PSK_FRAME_GLOBAL uint32_t *const out32 = (PSK_FRAME_GLOBAL uint32_t *)(oa - off);
        PSK_FRAME_GLOBAL uint8_t *const out8 = (PSK_FRAME_GLOBAL uint8_t *)d.out;
        const uint32_t n_group = (off + n + 3u) >> 2;
        const uint32_t inv = (d.flags >> 1) & PSK_SOFT_FRAME_INVERT ? 0xffffffffu : 0u;
        uint32_t ones = 0;
        for (uint32_t grp = tid; grp < n_group; grp += kFrameCutLanes) {
            const int32_t i0 = (int32_t)(4u * grp) - (int32_t)off;  // the output byte at the dword's first byte
            const bool whole = i0 >= 0 && (uint32_t)i0 + 4u <= n;
            uint32_t v = 0, valid = 0;  // the dword as it lies in memory; 0xff in the bytes that are the frame's
            if (whole && !d.stride) {
                const uint32_t g = b.g0 + 8u * (uint32_t)i0, idx = g >> 5, o = g & 31u;
                const uint32_t w0 = frame_msb_first(b.base[idx]);
                uint32_t m = w0;
                if (o)
                    m = (w0 << o) | (frame_msb_first(b.base[idx + 1u]) >> (32u - o));
                v = __builtin_bswap32(m);
                valid = 0xffffffffu;
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++) {
                    const int32_t i = i0 + (int32_t)j;
                    if (i >= 0 && (uint32_t)i < n) {
                        v |= frame_byte(b, b.g0 + 8u * frame_source((uint32_t)i, d.branch0, d.branches, d.stride)) << (8u * j);
                        valid |= 0xffu << (8u * j);
                    }
                }
            }
            v = (v ^ inv) & valid;
            if (d.table)
                v = ((uint32_t)s_table[v & 0xffu] | ((uint32_t)s_table[(v >> 8) & 0xffu] << 8) | ((uint32_t)s_table[(v >> 16) & 0xffu] << 16) |
                     ((uint32_t)s_table[v >> 24] << 24)) &
                    valid;
            ones += (uint32_t)__popc(v);
            if (whole) {
                out32[grp] = v;
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++)
                    if ((valid >> (8u * j)) & 1u)
                        out8[i0 + (int32_t)j] = (uint8_t)(v >> (8u * j));
            }
        }
        ones = frame_wave_sum(ones);
        if ((tid & 63u) == 0u)
            s_ones[tid >> 6] = ones;
        __syncthreads();
        if (tid < sizeof(psk_soft_frame_cut_t) / 4u) {
            uint32_t total = 0;
            for (uint32_t w = 0; w < kFrameCutLanes / 64u; w++) total += s_ones[w];
            rec[tid] = tid == 0u ? d.flags : tid == 1u ? n : tid == 2u ? d.span : tid == 3u ? total : 0u;
        }
    }
}

}  // namespace

hipError_t launch_frame_search(const FrameSearchDesc *desc, uint32_t nstream, uint32_t n_part, FrameSearchPartial *part,
                               psk_soft_frame_search_t *records, hipStream_t stream)
{
    if (!nstream)
        return hipSuccess;
    if (n_part)
        hipLaunchKernelGGL(psk_frame_fold_kernel, dim3(n_part), dim3(64), 0, stream, desc, nstream, part);
    const uint32_t grid = nstream < kFrameSearchGrid ? nstream : kFrameSearchGrid;
    hipLaunchKernelGGL(psk_frame_join_kernel, dim3(grid), dim3(64), 0, stream, desc, nstream, part, records);
    return hipGetLastError();
}

hipError_t launch_frame_cut(const FrameCutDesc *desc, uint32_t nframe, uint32_t grid, const uint8_t *tables, psk_soft_frame_cut_t *records,
                            hipStream_t stream)
{
    if (!nframe || !grid)
        return hipSuccess;
    hipLaunchKernelGGL(psk_frame_cut_kernel, dim3(grid), dim3(kFrameCutLanes), 0, stream, desc, nframe, tables, records);
    return hipGetLastError();
}

}  // namespace psk
