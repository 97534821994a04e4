// psk_fir.hip -- the filter pre-pass of psk_soft_process_device_filtered: every filtered packet of a call, whatever its format and
// stride, read once, shifted in frequency if it is also tuned (psk_front_src.h: tune_rotate), filtered with the real taps of its slot
// and decimated (psk_fir.h: fir_step) and written as float2 rows of the handle's gather scratch; the resample pass or the ordinary
// call then runs on the rows as on CF32 packets.  One launch per call.
//
// A workgroup walks pieces of fir_piece(D) outputs of one packet.  Per piece it loads the inputs the piece needs,
// s[i(m0) - (T-1) .. i(m1-1)], once -- converted (psk_pkt_cvt.h), rotated with the phasor tables in LDS as the tune kernel does, the
// channel's history slot supplying the indices below 0 -- into LDS as float2.  A lane issues all its loads of a piece (sixteen at
// most) before it uses the first.
//
// The sum.  A lane produces R consecutive outputs (R = 4 at D <= 3, 2 at D <= 7, else 1: at a large D a piece has too few outputs
// to give every lane several) from ONE walk over the inputs they share: step q = 0, 1, .. reads the sample s[top - q], top = the
// newest input of the lane's last output, and feeds it to every output r of the lane with the tap j = q - (R-1-r) * D, if that is
// a tap.  Each output meets its taps in ascending j, whatever R, so the result is the definition's to the bit; an LDS read of a
// sample feeds R outputs.  The taps of a step are one row of a table in LDS, G[q][c] = h[q - c*D], built once per workgroup from
// the slot's taps: every lane of a wave reads the same row, a broadcast read (16 bytes at R = 4), no vector-memory traffic in the
// loop.  Steps where every output of the lane has a tap (the bulk, at T > (R-1) * D) run without a test.
//
// LDS banks.  The lanes of a wave read samples R * D apart with ds_read_b64 (64 banks, lane groups of 32).  An odd stride
// (D = 9, 11, 13, 15) spreads a group over all banks.  An even one does not: unpadded, the strides 4, 8, 12, 16 samples put 4, 8, 4
// and 16 lanes of a group on the same pair of banks.  So at an even stride sample k lies at entry k + k / 32 -- one float2 of
// padding behind every 32 --, which leaves two lanes on a pair at the worst, at every D (counted over the lane groups of a
// piece).  Tables 16 KiB + G 2.5 KiB + samples 33.5 KiB = 52 KiB of static LDS: three workgroups on a CU.
//
// The workgroup that takes the packet's last piece (or the first one of a packet without outputs) writes the history behind the
// packet, 127 samples, into the channel's other slot.  Plain vector loads and stores only; the source is never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_fir.h"
#include "psk_front_src.h"
#include "psk_soft_hip.h"
#include "psk_tune.h"

namespace psk {

constexpr uint32_t kFirThreads = 256;
constexpr uint32_t kFirLoads = kFirWindow / kFirThreads;  // inputs a lane loads per piece, at most
// entries behind the window that a lane whose last outputs lie behind the piece's end may read (their sums are not stored)
constexpr uint32_t kFirSlack = 64;
// the entry of sample k; sh = fir_pad_shift() of the packet's decimation
__host__ __device__ constexpr uint32_t fir_pad(uint32_t k, uint32_t sh) { return k + (k >> sh); }
constexpr uint32_t kFirSampleEntries = (fir_pad(kFirWindow + kFirSlack, 5u) + 2u) & ~1u;
// rows of G: (R-1) * D + T steps, R floats each; the most at R = 4, D = 3
constexpr uint32_t kFirGFloats = 640;
static_assert(4u * (3u * 3u + kFirMaxTaps) <= kFirGFloats && 2u * (7u + kFirMaxTaps) <= kFirGFloats, "G holds every row");
static_assert(fir_piece(1) * 1u + kFirMaxTaps <= kFirWindow && (fir_piece(3) + 2u) * 3u + kFirMaxTaps <= kFirWindow + kFirSlack, "a piece fits its window");
static_assert(sizeof(float) * (kTuneTableFloats + kFirGFloats + 2u * kFirSampleEntries) <= 65536u, "tables, taps and samples in static LDS");

__host__ __device__ constexpr uint32_t fir_outputs_per_lane(uint32_t decim) { return decim <= 3u ? 4u : decim <= 7u ? 2u : 1u; }
// padding behind every 32 samples where the lanes' stride, R * D samples, is even; none (k >> 31 = 0) where it is odd
__host__ __device__ constexpr uint32_t fir_pad_shift(uint32_t decim) { return (fir_outputs_per_lane(decim) * decim) & 1u ? 31u : 5u; }

// entry q (0 .. 126, oldest first) of the history in front of the packet
__device__ inline f2 fir_history(const FirDesc &d, uint32_t q)
{
    if (d.io.flags & kFrontRestart)
        return f2{0.0f, 0.0f};
    return ((const PSK_GLOBAL f2 *)d.hist_in)[q];
}

// the row of G of step q
template <int R>
__device__ inline void fir_row(const float *G, uint32_t q, float *h)
{
    if constexpr (R == 4) {
        const f4 v = reinterpret_cast<const f4 *>(G)[q];
        h[0] = v.x, h[1] = v.y, h[2] = v.z, h[3] = v.w;
    } else if constexpr (R == 2) {
        const f2 v = reinterpret_cast<const f2 *>(G)[q];
        h[0] = v.x, h[1] = v.y;
    } else {
        h[0] = G[q];
    }
}

// outputs [m0, m0 + cnt_out) of the packet of d from the window whose entry 0 is s[i(m0) - (T-1)]; R outputs a lane
template <int R>
__device__ inline void fir_sums(const FirDesc &d, const float *G, const f2 *s, uint64_t m0, uint32_t cnt_out)
{
    PSK_GLOBAL f2 *__restrict__ dst = (PSK_GLOBAL f2 *)d.io.dst;
    const uint32_t D = d.decim, T = d.n_taps, sh = fir_pad_shift(D);
    const uint32_t lead = (uint32_t)(R - 1) * D, Q = lead + T;
    // steps [0, head): some output has not started; [head, mid): every output has a tap, none its first; [mid, Q): some are through
    const uint32_t head = lead + 1u < Q ? lead + 1u : Q, mid = T > head ? T : head;
    for (uint32_t u = threadIdx.x; u * R < cnt_out; u += kFirThreads) {
        const uint32_t top = (u * R + (uint32_t)(R - 1)) * D + (T - 1u);
        float ar[R], ai[R];
#pragma unroll
        for (int r = 0; r < R; r++) ar[r] = ai[r] = 0.0f;
        // (c = R-1-r: the output c behind the lane's last one meets the tap q - c*D at step q)
        auto tested = [&](uint32_t q0, uint32_t q1) {
            for (uint32_t q = q0; q < q1; q++) {
                const f2 x = s[fir_pad(top - q, sh)];
                float h[R];
                fir_row<R>(G, q, h);
#pragma unroll
                for (int c = 0; c < R; c++) {
                    const int32_t j = (int32_t)q - c * (int32_t)D;
                    if (j >= 0 && j < (int32_t)T) {
                        ar[R - 1 - c] = fir_step(j == 0, ar[R - 1 - c], h[c], x.x);
                        ai[R - 1 - c] = fir_step(j == 0, ai[R - 1 - c], h[c], x.y);
                    }
                }
            }
        };
        tested(0u, head);
#pragma unroll 4
        for (uint32_t q = head; q < mid; q++) {
            const f2 x = s[fir_pad(top - q, sh)];
            float h[R];
            fir_row<R>(G, q, h);
#pragma unroll
            for (int c = 0; c < R; c++) {
                ar[R - 1 - c] = fir_step(false, ar[R - 1 - c], h[c], x.x);
                ai[R - 1 - c] = fir_step(false, ai[R - 1 - c], h[c], x.y);
            }
        }
        tested(mid, Q);
        const uint64_t m = m0 + (uint64_t)u * R;
        const uint32_t left = cnt_out - u * R;  // (>= 1)
#pragma unroll
        for (int r = 0; r < R; r += 2) {
            if (R > 1 && (uint32_t)r + 1u < left)
                *reinterpret_cast<PSK_GLOBAL f4 *>(dst + m + r) = f4{ar[r], ai[r], ar[R > 1 ? r + 1 : r], ai[R > 1 ? r + 1 : r]};
            else if ((uint32_t)r < left)
                dst[m + r] = f2{ar[r], ai[r]};
        }
    }
}

// outputs [m0, m1) of the packet of d, m0 even, m1 - m0 <= fir_piece(D)
template <int FMT>
__device__ inline void fir_one_piece(const FirDesc &d, const float *tab, const float *G, f2 *s, uint64_t m0, uint64_t m1)
{
    const uint32_t cnt_out = (uint32_t)(m1 - m0);
    const uint32_t cnt = (cnt_out - 1u) * d.decim + d.n_taps;  // s[i(m0) - (T-1) .. i(m1-1)]; i(m1-1) < d.io.n
    if (cnt > kFirWindow)
        return;  // (a descriptor the entry would have refused: the whole workgroup leaves the piece out)
    // the LDS entry of sample k < cnt becomes s[i(m0) - (T-1) + k]
    const uint32_t sh = fir_pad_shift(d.decim);
    src_fill<FMT, kFirThreads, kFirLoads>(
        d.io, (d.io.flags & kFrontTuned) != 0, tab, (int64_t)(d.pos + m0 * d.decim) - (int64_t)(d.n_taps - 1u), cnt,
        [&](int64_t g) { return fir_history(d, (uint32_t)(g + (int64_t)kFirHist)); }, [&](uint32_t k, f2 x) { s[fir_pad(k, sh)] = x; });
    __syncthreads();
    switch (fir_outputs_per_lane(d.decim)) {
    case 4: fir_sums<4>(d, G, s, m0, cnt_out); break;
    case 2: fir_sums<2>(d, G, s, m0, cnt_out); break;
    default: fir_sums<1>(d, G, s, m0, cnt_out); break;
    }
    __syncthreads();  // (the next piece overwrites s)
}

// the history behind the packet: the last 127 of (history in front ‖ s[0 .. n-1]), by lanes 0 .. 126
template <int FMT>
__device__ inline void fir_write_history(const FirDesc &d, const float *tab)
{
    if (threadIdx.x >= kFirHist)
        return;
    const uint64_t q = d.io.n + threadIdx.x;  // index into the joined sequence, whose last 127 are n .. n + 126
    f2 v;
    if (q < kFirHist) {
        v = fir_history(d, (uint32_t)q);
    } else {
        const uint64_t idx = q - kFirHist;
        v = src_load<FMT>((const PSK_GLOBAL void *)d.io.src, idx * d.io.stride);
        if (d.io.flags & kFrontTuned)
            v = src_rotate(tab, d.io.phase + idx * d.io.step, v);
    }
    ((PSK_GLOBAL f2 *)d.hist_out)[threadIdx.x] = v;
}

template <int FMT>
__device__ inline void fir_packet(const FirDesc &d, const float *tab, const float *G, f2 *s, uint64_t n_pieces, bool owns_tail)
{
    const uint32_t piece = fir_piece(d.decim);
    for (uint64_t p = blockIdx.y; p < n_pieces; p += gridDim.y) {
        const uint64_t m0 = p * piece;
        fir_one_piece<FMT>(d, tab, G, s, m0, d.n_out - m0 < piece ? d.n_out : m0 + piece);
    }
    if (owns_tail)
        fir_write_history<FMT>(d, tab);
}

// grid: x = descriptor (one packet), y = workgroups that share its pieces, piece p going to workgroup p % gridDim.y
__global__ __launch_bounds__(kFirThreads) void psk_fir_kernel(const FirDesc *__restrict__ desc, const float *__restrict__ d_tab)
{
    __shared__ __attribute__((aligned(16))) float lds[kTuneTableFloats + kFirGFloats + 2u * kFirSampleEntries];
    float *const tab = lds;
    float *const G = lds + kTuneTableFloats;
    f2 *const s = reinterpret_cast<f2 *>(lds + kTuneTableFloats + kFirGFloats);
    const FirDesc d = desc[blockIdx.x];
    if (!d.decim || d.decim > kFirMaxDecim || !d.n_taps || d.n_taps > kFirMaxTaps)
        return;  // (the entry refuses these)
    const uint32_t piece = fir_piece(d.decim);
    const uint64_t n_pieces = (d.n_out + piece - 1u) / piece;
    const bool owns_tail = n_pieces ? (n_pieces - 1u) % gridDim.y == blockIdx.y : blockIdx.y == 0;
    if (blockIdx.y >= n_pieces && !owns_tail)
        return;  // (the whole workgroup: nothing of this packet is left for it)
    if (d.io.flags & kFrontTuned)
        src_tables_to_lds<kFirThreads>(tab, d_tab);
    if (blockIdx.y < n_pieces) {
        // G[q][c] = h[q - c*D], zero where that is no tap (those entries are never used)
        const uint32_t R = fir_outputs_per_lane(d.decim), rows = (R - 1u) * d.decim + d.n_taps;
        const PSK_GLOBAL float *h = (const PSK_GLOBAL float *)d.taps;
        for (uint32_t e = threadIdx.x; e < rows * R; e += kFirThreads) {
            const int32_t j = (int32_t)(e / R) - (int32_t)((e % R) * d.decim);
            G[e] = j >= 0 && j < (int32_t)d.n_taps ? h[j] : 0.0f;
        }
    }
    __syncthreads();
    src_dispatch(d.io.format, [&](auto fmt) { fir_packet<decltype(fmt)::value>(d, tab, G, s, n_pieces, owns_tail); });
}

hipError_t launch_fir(const FirDesc *desc, uint32_t n_desc, uint64_t max_pieces, const float *d_tab, hipStream_t stream)
{
    if (!n_desc)
        return hipSuccess;
    hipLaunchKernelGGL(psk_fir_kernel, dim3(n_desc, front_grid_y(max_pieces, n_desc)), dim3(kFirThreads), 0, stream, desc, d_tab);
    return hipGetLastError();
}

}  // namespace psk
