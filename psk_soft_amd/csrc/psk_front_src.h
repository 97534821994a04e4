// psk_front_src.h -- the packet source of the front stages (psk_tune.hip, psk_resample.hip, psk_fir.hip, psk_acquire.hip): how a
// pre-pass reads one sample of a packet -- format, stride, optional rotation by the phasor tables -- said once.
//
// Host and device: the head every descriptor of these passes begins with (FrontIo), the rotation itself (tune_rotate, which IS
// the definition of a tuned sample: psk_soft_tune_apply on the host and every kernel call it, on the same tables) and the grid
// rule of the passes that cut packets into pieces.  Device only: the loads, the conversion, the tables' copy into LDS, the one
// switch over the formats and the window fill with a history in front.
#ifndef PSK_FRONT_SRC_H
#define PSK_FRONT_SRC_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace psk {

constexpr uint32_t kTuneTable = 1024;  // entries of either table; the tables lie back to back: [coarse | fine], (cos, sin) pairs
constexpr uint32_t kTuneTableFloats = 4u * kTuneTable;

// One packet as a front stage reads and writes it: n complex samples of `format`, `stride` samples apart at src; what the stage
// makes of them goes to dst as float2.  Sample k of a tuned packet is rotated by W(phase + k * step).
struct FrontIo {
    const void *src;
    float *dst;       // 128-byte aligned, in the handle's gather scratch
    uint64_t stride;  // 1: contiguous (the caller's packet, or its row behind the tile gather)
    uint64_t n;
    uint64_t phase, step;
    uint32_t format;  // PSK_SOFT_FORMAT_*
    uint32_t flags;   // kFront*; the tune kernel's packets are all tuned and have no history: 0
};
enum : uint32_t { kFrontRestart = 1u, kFrontTuned = 2u };  // FrontIo::flags: the history in front is zeros; the packet is tuned
// (tests/prepass_probe.py mirrors the layout)
static_assert(sizeof(FrontIo) == 56 && offsetof(FrontIo, src) == 0 && offsetof(FrontIo, dst) == 8 && offsetof(FrontIo, stride) == 16 &&
                  offsetof(FrontIo, n) == 24 && offsetof(FrontIo, phase) == 32 && offsetof(FrontIo, step) == 40 &&
                  offsetof(FrontIo, format) == 48 && offsetof(FrontIo, flags) == 52,
              "the shared head of TuneDesc, ResampleDesc and FirDesc");

// y = x * W(p), tab = [coarse | fine].  W comes from two tables of 1024 entries, a coarse one indexed by the top ten bits of the
// phase word p (turns x 2^64) and a fine one by the next ten; the product of the two entries and the product with the sample are
// plain float32 operations, each rounded once, none fused.
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

// W(p) by itself, the (wr, wi) of tune_rotate: the phasor of a phase word for a pass that multiplies something other than a
// sample by it (psk_symrate.h)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void tune_phasor(const float *tab, uint64_t p, float *wr, float *wi)
{
    const uint32_t top = (uint32_t)(p >> 44);
    const float *const c = tab + 2u * (top >> 10), *const f = tab + 2u * (kTuneTable + (top & (kTuneTable - 1u)));
    const float cr = c[0], ci = c[1], fr = f[0], fi = f[1];
    *wr = cr * fr - ci * fi;
    *wi = cr * fi + ci * fr;
}

// The grid rule of a pass whose grid is (descriptors, workgroups per descriptor): about 2048 workgroups in all (eight per CU),
// none without a piece of the longest packet, which has `pieces` of them.
inline uint32_t front_grid_y(uint64_t pieces, uint32_t n_desc)
{
    const uint64_t fill = (2048u + n_desc - 1u) / n_desc;
    const uint64_t per = pieces < fill ? pieces : fill;
    return (uint32_t)(per < 1u ? 1u : per > 65535u ? 65535u : per);
}

}  // namespace psk

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "psk_pkt_cvt.h"

namespace psk {

// (the descriptors carry plain pointers; the kernels read and write through them as global memory, see psk_gather.hip)
#define PSK_GLOBAL __attribute__((address_space(1)))
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

// one sample as it lies in the packet (a load), and its float2 (arithmetic only: a lane can keep its loads apart from their first use)
template <int FMT>
struct SrcRaw {
    typedef typename PktWord<FMT>::type type;
};
template <>
struct SrcRaw<PSK_SOFT_FORMAT_CF32> {
    typedef f2 type;
};
template <int FMT>
__device__ inline typename SrcRaw<FMT>::type src_load_raw(const PSK_GLOBAL void *src, uint64_t idx)
{
    return reinterpret_cast<const PSK_GLOBAL typename SrcRaw<FMT>::type *>(src)[idx];
}
template <int FMT>
__device__ inline f2 src_cvt(typename SrcRaw<FMT>::type raw)
{
    if constexpr (FMT == PSK_SOFT_FORMAT_CF32) {
        return raw;
    } else {
        const float2 v = pkt_cvt<FMT>(raw);
        return f2{v.x, v.y};
    }
}
// the sample at index idx (samples, the stride multiplied in by the caller)
template <int FMT>
__device__ inline f2 src_load(const PSK_GLOBAL void *src, uint64_t idx)
{
    return src_cvt<FMT>(src_load_raw<FMT>(src, idx));
}
// x * W(p)
__device__ inline f2 src_rotate(const float *tab, uint64_t p, f2 x)
{
    float yr, yi;
    tune_rotate(tab, p, x.x, x.y, &yr, &yi);
    return f2{yr, yi};
}

// the two phasor tables (16 KiB) from device memory into the workgroup's LDS; the caller synchronises
template <uint32_t THREADS>
__device__ inline void src_tables_to_lds(float *tab, const float *d_tab)
{
    const PSK_GLOBAL f4 *g = (const PSK_GLOBAL f4 *)d_tab;
    f4 *const t = reinterpret_cast<f4 *>(tab);
#pragma unroll
    for (uint32_t k = 0; k < kTuneTableFloats / 4u / THREADS; k++) t[threadIdx.x + k * THREADS] = g[threadIdx.x + k * THREADS];
}

// the one switch over the formats: f(std::integral_constant<int, FMT>{}); a format the library does not know does nothing
template <class F>
__device__ inline void src_dispatch(uint32_t format, F &&f)
{
    switch (format) {
    case PSK_SOFT_FORMAT_CF32: f(std::integral_constant<int, PSK_SOFT_FORMAT_CF32>{}); break;
    case PSK_SOFT_FORMAT_CS16: f(std::integral_constant<int, PSK_SOFT_FORMAT_CS16>{}); break;
    case PSK_SOFT_FORMAT_CS8: f(std::integral_constant<int, PSK_SOFT_FORMAT_CS8>{}); break;
    case PSK_SOFT_FORMAT_CF16: f(std::integral_constant<int, PSK_SOFT_FORMAT_CF16>{}); break;
    default: break;
    }
}

// The window fill of a pass that keeps a history in front of the packet: store(k, x) for k < cnt <= LOADS * THREADS, x = s[g0 + k]
// of the packet of io -- converted, rotated if `tuned` -- or hist(g0 + k) where g0 + k < 0; g0 + cnt <= io.n.  All of a lane's
// loads are issued before the first is used: the index of a lane with nothing to load (k >= cnt, or an entry the history
// supplies) is clamped into the packet, so the loads are unconditional within an iteration, and the iterations' bound is the
// workgroup's.
template <int FMT, uint32_t THREADS, uint32_t LOADS, class H, class S>
__device__ inline void src_fill(const FrontIo &io, bool tuned, const float *tab, int64_t g0, uint32_t cnt, H &&hist, S &&store)
{
    const PSK_GLOBAL void *__restrict__ src = (const PSK_GLOBAL void *)io.src;
    const uint32_t iters = (cnt + THREADS - 1u) / THREADS;
    typename SrcRaw<FMT>::type v[LOADS];
#pragma unroll
    for (uint32_t j = 0; j < LOADS; j++) {
        const int64_t g = g0 + (int64_t)(threadIdx.x + j * THREADS);
        const uint64_t idx = g < 0 ? 0u : (uint64_t)g < io.n ? (uint64_t)g : io.n - 1u;
        v[j] = j < iters ? src_load_raw<FMT>(src, idx * io.stride) : typename SrcRaw<FMT>::type{};
    }
    uint64_t p = io.phase + (uint64_t)(g0 + (int64_t)threadIdx.x) * io.step;  // (mod 2^64; not used below index 0)
    const uint64_t adv = io.step * THREADS;
#pragma unroll
    for (uint32_t j = 0; j < LOADS; j++, p += adv) {
        const uint32_t k = threadIdx.x + j * THREADS;
        if (k >= cnt)
            continue;
        const int64_t g = g0 + (int64_t)k;
        f2 x = src_cvt<FMT>(v[j]);
        if (g < 0)
            x = hist(g);
        else if (tuned)
            x = src_rotate(tab, p, x);
        store(k, x);
    }
}

}  // namespace psk
#endif
#endif
