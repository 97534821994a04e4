// psk_viterbi.h -- what the host (psk_capi.cpp) and the decoder of psk_soft_viterbi_device (psk_viterbi.hip) share, and the
// per-step terms of include/psk_soft_hip.h ("frames as payload bits"), which psk_soft_viterbi_host (host) and the kernel (device)
// both take from here: the code bits of a state's two incoming branches, the puncture walk, the branch metric and the
// add-compare-select.
//
// The definition, restated.  A code is K = 3 .. 7, n = 2 .. 4 polynomials g[j] of K bits, bit K-1 tapping the current input.  A
// state is the K-1 last inputs, the newest at bit K-2.  State s is entered from p_b = ((s << 1) & mask) | b, b = 0, 1, with the
// input u = s >> (K-2); the register of that branch is r = (u << (K-1)) | p_b and its code bit j is parity(r & g[j]).  A step
// with t mod P == p carries the code bits j whose bit p*n + j of `keep` is set, as int8 LLRs in order of (t, j), positive meaning
// 0; bm = sum over the kept j of (c_j ? -l_j : +l_j); pm'[s] = max_b(pm[p_b] + bm_b) in int32, b = 1 winning only if strictly
// greater.  Everything is an integer: there is no rounding and no order of summation to keep.
#ifndef PSK_VITERBI_H
#define PSK_VITERBI_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_soft_hip.h"

namespace psk {

constexpr uint32_t kViterbiSlots = PSK_SOFT_VITERBI_SLOTS;
constexpr uint32_t kViterbiMaxFrames = PSK_SOFT_VITERBI_MAX_FRAMES;
constexpr uint32_t kViterbiMaxSteps = PSK_SOFT_VITERBI_MAX_STEPS;
constexpr uint32_t kViterbiMaxN = 4, kViterbiMinK = 3, kViterbiMaxK = 7, kViterbiMaxP = 16;
constexpr uint32_t kViterbiChunk = 64;                 // steps whose decision words one coalesced store carries, one a lane
// decision words (8 bytes, one a step) a call keeps in flight: the scratch bound of the header
constexpr uint64_t kViterbiScratchWords = PSK_SOFT_VITERBI_SCRATCH_BYTES / 8u;
constexpr int32_t kViterbiUnreached = -(1 << 30);      // the start metric of every state but 0
constexpr uint32_t kViterbiFlagMask = PSK_SOFT_VITERBI_PACKED | PSK_SOFT_VITERBI_TERMINATED | PSK_SOFT_VITERBI_ANY_START;

enum : uint32_t { kViterbiData = 1u };                 // ViterbiDesc::flags bit 0: the frame is decoded; the frame's flags << 1 above it

// a code as the kernel reads it: wave-uniform, 32 bytes.  K == 0: the slot was never defined
struct ViterbiCode {
    uint32_t K, n, P, keep;
    uint32_t g[kViterbiMaxN];
};
static_assert(sizeof(ViterbiCode) == 32, "a code is 32 bytes");

// One frame of one call.  Without kViterbiData the kernel writes the zero record and nothing else.
struct ViterbiDesc {
    const int8_t *llr;
    void *out;
    uint32_t n_steps;
    uint32_t code;   // the slot
    uint32_t flags;  // kViterbiData | the frame's PSK_SOFT_VITERBI_* flags << 1: the record's flags as they are
    uint32_t n_llr;  // vt_count of the frame
};
static_assert(sizeof(ViterbiDesc) == 32, "a descriptor is 32 bytes");

#if defined(__HIPCC__)
#define PSK_VT_HD __host__ __device__
#else
#define PSK_VT_HD
#endif

PSK_VT_HD inline uint32_t vt_popc(uint32_t v) { return (uint32_t)__builtin_popcount(v); }

// what psk_soft_viterbi_define refuses of a code
PSK_VT_HD inline bool vt_code_ok(uint32_t K, uint32_t n, const uint32_t *g, uint32_t P, uint32_t keep)
{
    if (K < kViterbiMinK || K > kViterbiMaxK || n < 2u || n > kViterbiMaxN || !P || P > kViterbiMaxP || n * P > 32u || !keep)
        return false;
    if (n * P < 32u && (keep >> (n * P)))
        return false;
    uint32_t all = 0;
    for (uint32_t j = 0; j < n; j++) {
        if (!g[j] || (g[j] >> K))
            return false;
        all |= g[j];
    }
    return ((all >> (K - 1u)) & 1u) && (all & 1u);
}

// the puncture walk: the code bits (bit j) that a step of phase p = t mod P carries
PSK_VT_HD inline uint32_t vt_keep_of(uint32_t n, uint32_t keep, uint32_t p) { return (keep >> (p * n)) & ((1u << n) - 1u); }
PSK_VT_HD inline uint32_t vt_next_phase(uint32_t P, uint32_t p) { return p + 1u == P ? 0u : p + 1u; }

// the LLRs in front of step t: whole periods, then the phases 0 .. t mod P - 1 of the one begun
PSK_VT_HD inline uint64_t vt_count(uint32_t n, uint32_t P, uint32_t keep, uint32_t t)
{
    const uint32_t rem = t % P;
    const uint32_t low = rem ? keep & (0xffffffffu >> (32u - n * rem)) : 0u;  // (rem < P: n * rem < 32)
    return (uint64_t)(t / P) * vt_popc(keep) + vt_popc(low);
}

// the code bits (bit j = c_j) of the branch that enters state s from its predecessor b
PSK_VT_HD inline uint32_t vt_branch_bits(const ViterbiCode &c, uint32_t s, uint32_t b)
{
    const uint32_t mask = (1u << (c.K - 1u)) - 1u;
    const uint32_t r = ((s >> (c.K - 2u)) << (c.K - 1u)) | (((s << 1) & mask) | b);
    uint32_t bits = 0;
    for (uint32_t j = 0; j < kViterbiMaxN; j++)
        if (j < c.n)
            bits |= (vt_popc(r & c.g[j]) & 1u) << j;
    return bits;
}
// the same of a register r as the traceback and the encoder meet it
PSK_VT_HD inline uint32_t vt_code_bits(const ViterbiCode &c, uint32_t r)
{
    uint32_t bits = 0;
    for (uint32_t j = 0; j < kViterbiMaxN; j++)
        if (j < c.n)
            bits |= (vt_popc(r & c.g[j]) & 1u) << j;
    return bits;
}

// the branch metric of code bits `bits` against the step's LLRs; l[j] is 0 where bit j is not kept, so it contributes 0
template <uint32_t N>
PSK_VT_HD inline int32_t vt_bm(uint32_t bits, const int32_t *l)
{
    int32_t bm = 0;
#pragma unroll
    for (uint32_t j = 0; j < N; j++) bm += ((bits >> j) & 1u) ? -l[j] : l[j];
    return bm;
}

// add-compare-select: the new metric, the decision in *d (1 only if strictly greater)
PSK_VT_HD inline int32_t vt_acs(int32_t pm0, int32_t bm0, int32_t pm1, int32_t bm1, uint32_t *d)
{
    const int32_t a0 = pm0 + bm0, a1 = pm1 + bm1;
    *d = a1 > a0 ? 1u : 0u;
    return a1 > a0 ? a1 : a0;
}

// what an LLR adds to the record against the code bit c of the decoded path
PSK_VT_HD inline void vt_tally(int32_t l, uint32_t c, uint32_t *sum_abs, uint32_t *n_flip, uint32_t *n_zero)
{
    *sum_abs += (uint32_t)(l < 0 ? -l : l);
    *n_zero += l == 0 ? 1u : 0u;
    *n_flip += (l != 0 && (l < 0) != (c != 0u)) ? 1u : 0u;
}

inline uint32_t viterbi_bits(uint32_t K, uint32_t n_steps, uint32_t flags)
{
    return (flags & PSK_SOFT_VITERBI_TERMINATED) ? n_steps - (K - 1u) : n_steps;
}

// Workgroups of one wave; workgroup w decodes the frames w, w + grid, ... and keeps its decisions in the `steps_cap` words (a
// multiple of kViterbiChunk, at least the longest frame of the call) from scratch + w * steps_cap on.
hipError_t launch_viterbi(const ViterbiDesc *desc, uint32_t nframe, uint32_t grid, uint32_t steps_cap, const ViterbiCode *codes,
                          uint64_t *scratch, psk_soft_viterbi_t *records, hipStream_t stream);

}  // namespace psk
#endif
