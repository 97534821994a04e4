// psk_viterbi.hip -- psk_soft_viterbi_device: frames of int8 LLRs decoded with a K = 3 .. 7 convolutional code, one
// psk_soft_viterbi_t per frame (include/psk_soft_hip.h, "frames as payload bits"; psk_viterbi.h restates the arithmetic).
//
// One launch, workgroups of one wave; a wave decodes one frame at a time, a state a lane.  Workgroup w takes the frames w,
// w + grid, ... of the call: the grid is held to 65535 and to what the scratch bound lets be in flight, the rest are further
// trips of the same workgroups.  For K < 7 the lanes at or above 2^(K-1) are idle: they are masked out of the ballots and of the
// first-maximum, and no lane ever reads their metric (a predecessor is a state below 2^(K-1)).
//
//   forward    Lane s keeps pm[s] in a register.  Its two incoming branches' code bits are constants of the code, formed once
//              per frame.  The two predecessor metrics come by a cross-lane read (ds_bpermute) of lanes (2s) & mask and that + 1.
//              A step's LLRs are wave-uniform: the wave reads them ahead, 64 aligned dwords at a time (a dword is loaded only if
//              it holds a byte of the frame), and hands them out by v_readlane at a uniform index.  The 64 decisions of a step
//              are one __ballot word; the words of 64 steps are collected one a lane and go out with one
//              coalesced 512-byte store into the workgroup's slice of the handle's scratch.
//   end        TERMINATED: state 0.  Otherwise the first maximum over the active lanes: a xor-tree maximum, then the lowest
//              lane that holds it.
//   traceback  64 steps at a time, from the back: the 64 decision words are loaded back one a lane (the load of the chunk
//              before is issued ahead of the walk), and the walk is v_readlane and scalar arithmetic -- no dependent load a
//              step.  It leaves the chunk's 64 decoded bits as one word and the state in front of the chunk.  From those every
//              lane forms the register of its own step, re-encodes it and holds it against the step's LLRs (byte loads, inside
//              the frame) for n_flip, n_zero and sum_abs.  The word of decoded bits is stored as it is, bit-reversed within
//              bytes, for PACKED, or spread one bit a byte; whole dwords where a dword lies inside the chunk's bytes, byte
//              stores at the unaligned head and tail.  No byte outside the frame's output is written.
//
// Everything is int32 and needs no normalisation: |pm| stays below 2^26 on reachable states, an unreachable one between -2^31 and
// -2^30 + 2^26 (psk_soft_hip.h).  Plain vector loads and stores only; the LLRs and the codes are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_viterbi.h"

namespace psk {

namespace {

#define PSK_VT_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint32_t vt_readlane(uint32_t v, uint32_t lane)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
__device__ __forceinline__ uint32_t vt_wave_sum(uint32_t v)
{
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

// The frame's LLRs handed out one after the other: a window of 64 aligned dwords, one a lane, from the dword that holds the
// frame's first byte on.  Everything but `word` is wave-uniform.
struct LlrWindow {
    const PSK_VT_GLOBAL uint32_t *base;  // the aligned dword that holds the frame's first LLR
    uint32_t first, end;                 // byte offsets from base: the first LLR (0 .. 3), one past the last
    uint32_t win;                        // byte offset of the window, a multiple of 256
    uint32_t off;                        // byte offset of the next LLR
    uint32_t word;                       // lane i: the dword at win + 4 i

    __device__ __forceinline__ void fill(uint32_t lane)
    {
        const uint32_t b = win + 4u * lane;
        // (b + 4 > first always; b < end: the dword holds a byte of the frame.  A frame without LLRs loads nothing.)
        word = (b < end && end > first) ? base[b >> 2] : 0u;
    }
    __device__ __forceinline__ void open(const int8_t *llr, uint32_t n_llr, uint32_t lane)
    {
        const uintptr_t a = (uintptr_t)llr;
        base = (const PSK_VT_GLOBAL uint32_t *)(a & ~(uintptr_t)3);
        first = (uint32_t)(a & 3u), end = first + n_llr;
        win = 0u, off = first;
        fill(lane);
    }
    __device__ __forceinline__ int32_t next(uint32_t lane)
    {
        if (off - win >= 256u) {
            win += 256u;
            fill(lane);
        }
        const uint32_t w = vt_readlane(word, (off - win) >> 2);
        const int32_t l = (int32_t)(int8_t)(w >> (8u * (off & 3u)));
        off++;
        return l;
    }
};

// nb bytes to dst, byte k being (src >> 8k) & 0xff for PACKED (nb <= 8) or (src >> k) & 1 otherwise (nb <= 64): lane j takes the
// aligned dword j of the destination's span; a dword that lies inside the nb bytes goes out whole, the others byte by byte
template <bool kPacked>
__device__ __forceinline__ void vt_store_chunk(uint8_t *dst, uint32_t nb, uint64_t src, uint32_t lane)
{
    const uint32_t a = (uint32_t)((uintptr_t)dst & 3u);
    const int32_t i0 = (int32_t)(4u * lane) - (int32_t)a;  // the chunk's byte that lands on byte 0 of the lane's dword
    if (i0 >= (int32_t)nb)
        return;
    uint32_t v = 0;
#pragma unroll
    for (int32_t m = 0; m < 4; m++) {
        const int32_t i = i0 + m;
        uint32_t byte = 0;
        if (i >= 0 && i < (int32_t)nb)
            byte = kPacked ? (uint32_t)(src >> (8 * i)) & 0xffu : (uint32_t)(src >> i) & 1u;
        v |= byte << (8 * m);
    }
    PSK_VT_GLOBAL uint8_t *const o = (PSK_VT_GLOBAL uint8_t *)dst;
    if (i0 >= 0 && i0 + 4 <= (int32_t)nb) {
        *(PSK_VT_GLOBAL uint32_t *)(o + i0) = v;
        return;
    }
#pragma unroll
    for (int32_t m = 0; m < 4; m++) {
        const int32_t i = i0 + m;
        if (i >= 0 && i < (int32_t)nb)
            o[i] = (uint8_t)(v >> (8 * m));
    }
}

// one frame with a code of N polynomials
template <uint32_t N>
__device__ __forceinline__ void vt_frame(const ViterbiDesc &d, const ViterbiCode &c, PSK_VT_GLOBAL uint64_t *dec, uint32_t lane,
                                         psk_soft_viterbi_t *rec)
{
    const uint32_t K = c.K, P = c.P, keep = c.keep;
    const uint32_t n_state = 1u << (K - 1u), mask = n_state - 1u;
    const bool active = lane < n_state;
    const uint32_t frame_flags = d.flags >> 1;
    const uint32_t T = d.n_steps;

    // ---- forward ----
    const uint32_t bits0 = vt_branch_bits(c, lane & mask, 0u), bits1 = vt_branch_bits(c, lane & mask, 1u);
    const int p0 = (int)((lane << 1) & mask), p1 = p0 | 1;
    int32_t pm = ((frame_flags & PSK_SOFT_VITERBI_ANY_START) || lane == 0u) ? 0 : kViterbiUnreached;
    LlrWindow in;
    in.open(d.llr, d.n_llr, lane);
    uint32_t phase = 0;
    for (uint32_t t0 = 0; t0 < T; t0 += kViterbiChunk) {
        const uint32_t cnt = T - t0 < kViterbiChunk ? T - t0 : kViterbiChunk;
        uint32_t lo = 0, hi = 0;  // lane i: the decision word of step t0 + i
        for (uint32_t i = 0; i < cnt; i++) {
            const uint32_t km = vt_keep_of(N, keep, phase);
            phase = vt_next_phase(P, phase);
            int32_t l[N];
#pragma unroll
            for (uint32_t j = 0; j < N; j++) l[j] = ((km >> j) & 1u) ? in.next(lane) : 0;
            const int32_t a = __shfl(pm, p0), b = __shfl(pm, p1);
            uint32_t dbit;
            pm = vt_acs(a, vt_bm<N>(bits0, l), b, vt_bm<N>(bits1, l), &dbit);
            const uint64_t w = __ballot(active && dbit);
            lo = lane == i ? (uint32_t)w : lo;
            hi = lane == i ? (uint32_t)(w >> 32) : hi;
        }
        dec[t0 + lane] = ((uint64_t)hi << 32) | lo;  // (the slice holds a multiple of kViterbiChunk words)
    }

    // ---- the end state ----
    uint32_t s;
    if (frame_flags & PSK_SOFT_VITERBI_TERMINATED) {
        s = 0u;
    } else {
        int32_t best = active ? pm : INT32_MIN;
        for (int off = 32; off >= 1; off >>= 1) {
            const int32_t o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        s = (uint32_t)__builtin_ctzll(__ballot(active && pm == best));  // (lane 0 is active: the ballot is not empty)
    }
    s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
    const uint32_t end_state = s;
    const int32_t metric = (int32_t)vt_readlane((uint32_t)pm, s);

    // ---- traceback ----
    const uint32_t n_bits = (frame_flags & PSK_SOFT_VITERBI_TERMINATED) ? T - (K - 1u) : T;
    uint32_t sum_abs = 0, n_flip = 0, n_zero = 0;
    const uint32_t last = (T - 1u) & ~(kViterbiChunk - 1u);
    uint64_t w_next = dec[last + lane];
    for (uint32_t t0 = last;; t0 -= kViterbiChunk) {
        const uint32_t cnt = T - t0 < kViterbiChunk ? T - t0 : kViterbiChunk;
        const uint32_t wlo = (uint32_t)w_next, whi = (uint32_t)(w_next >> 32);
        if (t0)
            w_next = dec[t0 - kViterbiChunk + lane];
        uint64_t ubits = 0;  // bit i: u of step t0 + i
        for (uint32_t i = cnt; i-- > 0u;) {
            const uint64_t w = ((uint64_t)vt_readlane(whi, i) << 32) | vt_readlane(wlo, i);
            ubits |= (uint64_t)(s >> (K - 2u)) << i;
            s = ((s << 1) & mask) | (uint32_t)((w >> s) & 1u);
        }
        // s is the state in front of step t0.  Bit i + K-1 of E is u of step t0 + i and its low K-1 bits are s, so the register
        // of step t0 + i is the K bits of E from bit i on.
        if (lane < cnt) {
            const uint32_t e_lo = (uint32_t)(ubits << (K - 1u)) | s;                                // E bits 0 .. 31
            const uint64_t e_hi = ubits >> (32u - (K - 1u));                                        // E bits 32 .. 69
            const uint64_t e_mid = lane < 32u ? (((uint64_t)(uint32_t)e_hi << 32) | e_lo) >> lane  // E from bit `lane` on
                                              : e_hi >> (lane - 32u);
            const uint32_t r = (uint32_t)e_mid & ((1u << K) - 1u);
            const uint32_t cb = vt_code_bits(c, r);
            const uint32_t t = t0 + lane;
            const uint32_t km = vt_keep_of(N, keep, t % P);
            const PSK_VT_GLOBAL int8_t *q = (const PSK_VT_GLOBAL int8_t *)d.llr + (uint32_t)vt_count(N, P, keep, t);
#pragma unroll
            for (uint32_t j = 0; j < N; j++)
                if ((km >> j) & 1u)
                    vt_tally((int32_t)*q++, (cb >> j) & 1u, &sum_abs, &n_flip, &n_zero);
        }
        // the chunk's bits of the output: those below n_bits
        if (t0 < n_bits) {
            const uint32_t nb = n_bits - t0 < kViterbiChunk ? n_bits - t0 : kViterbiChunk;
            const uint64_t u = nb < 64u ? ubits & ((1ull << nb) - 1ull) : ubits;
            if (frame_flags & PSK_SOFT_VITERBI_PACKED)  // bit i to byte i >> 3 at bit 7 - (i & 7): every byte bit-reversed
                vt_store_chunk<true>((uint8_t *)d.out + t0 / 8u, (nb + 7u) / 8u, __builtin_bswap64(__builtin_bitreverse64(u)), lane);
            else
                vt_store_chunk<false>((uint8_t *)d.out + t0, nb, u, lane);
        }
        if (!t0)
            break;
    }

    sum_abs = vt_wave_sum(sum_abs), n_flip = vt_wave_sum(n_flip), n_zero = vt_wave_sum(n_zero);
    if (lane == 0u) {
        psk_soft_viterbi_t r = {};  // (pad stays zero; lane 0 alone stores the 64 bytes)
        r.n_steps = T, r.n_llr = d.n_llr;
        r.metric = metric, r.sum_abs = sum_abs;
        r.n_flip = n_flip, r.n_zero = n_zero;
        r.end_state = end_state, r.start_state = s;
        r.n_bits = n_bits, r.flags = d.flags;
        *rec = r;
    }
}

}  // namespace

__global__ __launch_bounds__(64) void psk_viterbi_kernel(const ViterbiDesc *__restrict__ desc, uint32_t nframe, uint32_t steps_cap,
                                                         const ViterbiCode *__restrict__ codes, uint64_t *__restrict__ scratch,
                                                         psk_soft_viterbi_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x;
    PSK_VT_GLOBAL uint64_t *const dec = (PSK_VT_GLOBAL uint64_t *)scratch + (uint64_t)blockIdx.x * steps_cap;
    for (uint32_t f = blockIdx.x; f < nframe; f += gridDim.x) {
        const ViterbiDesc d = desc[f];
        psk_soft_viterbi_t *const rec = records + f;
        // (uniform for the wave, like every branch on the descriptor and the code below; the host has checked all of it)
        bool ok = (d.flags & kViterbiData) && d.code < kViterbiSlots && d.n_steps && d.n_steps <= steps_cap;
        ViterbiCode c = {};
        if (ok) {
            c = codes[d.code];
            ok = c.K >= kViterbiMinK && c.K <= kViterbiMaxK && c.P && c.P <= kViterbiMaxP;
        }
        if (ok && c.n == 2u)
            vt_frame<2>(d, c, dec, lane, rec);
        else if (ok && c.n == 3u)
            vt_frame<3>(d, c, dec, lane, rec);
        else if (ok && c.n == 4u)
            vt_frame<4>(d, c, dec, lane, rec);
        else if (lane == 0u)
            *rec = psk_soft_viterbi_t{};
    }
}

hipError_t launch_viterbi(const ViterbiDesc *desc, uint32_t nframe, uint32_t grid, uint32_t steps_cap, const ViterbiCode *codes,
                          uint64_t *scratch, psk_soft_viterbi_t *records, hipStream_t stream)
{
    if (!nframe || !grid)
        return hipSuccess;
    hipLaunchKernelGGL(psk_viterbi_kernel, dim3(grid), dim3(64), 0, stream, desc, nframe, steps_cap, codes, scratch, records);
    return hipGetLastError();
}

}  // namespace psk
