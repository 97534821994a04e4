// psk_rs.hip -- psk_soft_rs_device: frames of bytes decoded with a Reed-Solomon code over GF(256), one psk_soft_rs_t per frame
// (include/psk_soft_rs.h, "frames as corrected bytes"; psk_rs.h restates the arithmetic).
//
// One launch, workgroups of one wave; a wave decodes one frame at a time, its codewords j = 0 .. I-1 one after the other.
// Workgroup w takes the frames w, w + grid, ... of the call: the grid is held to kRsMaxGrid, the rest are further trips of the same
// workgroups (which keep their tables).  Lane L holds the bytes L, L + 64, L + 128 and L + 192 of the codeword (byte loads at frame offset i I + j, the
// mask applied as they are read; no byte outside the frame is read).
//
//   syndromes  One a lane, lane m < nroots: Horner over the n bytes, each handed out by v_readlane at a uniform index.  When
//              every syndrome is zero (one ballot) the wave goes straight to the copy.
//   locator    Berlekamp-Massey, a coefficient a lane: the discrepancy is a wave xor-reduction of lambda[i] S[r-i] (the
//              syndromes come by a cross-lane read), the shift of B a cross-lane read of the lane below.  Coefficients above
//              x^63 fall off the wave; no lane below them depends on them, and a locator longer than t <= 32 is a failure.
//   roots      Chien search, four positions a lane: Lambda, Omega = S Lambda mod x^nroots and Lambda' evaluated at 1 / X_p,
//              the coefficients handed out by v_readlane; the root count by ballot.
//   values     Forney (rs_magnitude) at the roots.
//   check      The outcome is the definition's exactly if: the locator's length is its degree and at most t, it has as many
//              roots among the n positions as its degree, no value is zero, and the syndromes of the error pattern are the
//              received word's (recomputed by the same Horner).  Otherwise the codeword has failed and goes out as received.
//
// A field multiply is exp[log a + log b] from tables in LDS, built by the wave whenever a frame's field differs from the last one's.
// Every branch on a descriptor, a code, a discrepancy or an outcome is wave-uniform.  Plain vector loads and stores only; the
// frames, the codes and the masks are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_rs.h"

namespace psk {

namespace {

#define PSK_RS_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint32_t rs_readlane(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }
__device__ __forceinline__ uint32_t rs_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t rs_wave_xor(uint32_t v)
{
    for (int off = 32; off >= 1; off >>= 1) v ^= (uint32_t)__shfl_xor((int)v, off);
    return v;
}
__device__ __forceinline__ uint32_t rs_wave_sum(uint32_t v)
{
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

// The field.  exp / log tables in LDS, of the field the workgroup last met: exp[i] = alpha^i for i = 0 .. 509, so that
// log a + log b needs no modulo; both 256-byte aligned, so the 64 lanes of a byte read meet at most two dwords a bank.  Measured
// against eight shift-and-xor steps a multiply (gf_mul, which still builds the tables): DESIGN.md 2.16.
__shared__ __attribute__((aligned(256))) uint8_t g_rs_exp[512];
__shared__ __attribute__((aligned(256))) uint8_t g_rs_log[256];
__device__ __forceinline__ void rs_tables(uint32_t gfpoly, uint32_t lane)
{
    __syncthreads();  // (one wave: what it read of the old tables is behind it)
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
        const uint32_t i = lane + 64u * q;
        if (i < 255u) {
            const uint32_t e = gf_pow(gfpoly, 2u, i);
            g_rs_exp[i] = (uint8_t)e, g_rs_exp[i + 255u] = (uint8_t)e, g_rs_log[e] = (uint8_t)i;
        }
    }
    if (lane == 0u)
        g_rs_log[0] = 0, g_rs_exp[510] = 0, g_rs_exp[511] = 0;
    __syncthreads();
}
__device__ __forceinline__ uint32_t rs_mul(uint32_t a, uint32_t b)
{
    const uint32_t r = g_rs_exp[(uint32_t)g_rs_log[a] + (uint32_t)g_rs_log[b]];
    return (a && b) ? r : 0u;
}
__device__ __forceinline__ uint32_t rs_dev_inv(uint32_t a) { return g_rs_exp[255u - g_rs_log[a]]; }  // (a != 0)
__device__ __forceinline__ uint32_t rs_dev_alpha(uint32_t e) { return g_rs_exp[e % 255u]; }

// lane m: sum_i w_i x^(n-1-i), w_i being byte i of the word whose bytes L + 64 q lane L holds in w[q]
__device__ __forceinline__ uint32_t rs_horner(uint32_t n, const uint32_t *w, uint32_t x)
{
    uint32_t s = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
        if (n <= 64u * q)
            break;
        const uint32_t cnt = n - 64u * q < 64u ? n - 64u * q : 64u;
        for (uint32_t l = 0; l < cnt; l++) s = rs_mul(s, x) ^ rs_readlane(w[q], l);
    }
    return s;
}

// The error pattern of a word with the syndromes s (lane m < nroots; 0 above, not all zero): e[q] the value at byte lane + 64 q.
// Returns the number of errors, or kRsFailed with e all zero.
__device__ __forceinline__ uint32_t rs_correct(const RsCode &c, uint32_t s, uint32_t x, uint32_t lane, uint32_t *e)
{
    const uint32_t nroots = c.nroots, n = c.n, t = nroots / 2u;
    e[0] = e[1] = e[2] = e[3] = 0u;

    // ---- Berlekamp-Massey: lam and B a coefficient a lane ----
    uint32_t lam = lane == 0u ? 1u : 0u, B = lam, len = 0;
    for (uint32_t r = 0; r < nroots; r++) {
        const uint32_t sv = (uint32_t)__shfl((int)s, (int)((r - lane) & 63u));
        const uint32_t delta = rs_uniform(rs_wave_xor(lane <= r ? rs_mul(lam, sv) : 0u));
        const uint32_t below = (uint32_t)__shfl((int)B, (int)((lane - 1u) & 63u));
        const uint32_t Bs = lane == 0u ? 0u : below;  // x B
        if (delta) {
            const uint32_t T = lam ^ rs_mul(delta, Bs);
            if (2u * len <= r) {
                B = rs_mul(lam, rs_dev_inv(delta));
                len = r + 1u - len;
            } else {
                B = Bs;
            }
            lam = T;
        } else {
            B = Bs;
        }
    }
    const uint64_t nz = __ballot(lam != 0u);  // (lam[0] = 1 always: not empty)
    const uint32_t deg = 63u - (uint32_t)__builtin_clzll(nz);
    if (len > t || deg != len)
        return kRsFailed;

    // ---- Omega = S Lambda mod x^nroots, lane L its coefficient L ----
    uint32_t om = 0;
    for (uint32_t i = 0; i <= deg; i++) {
        const uint32_t sv = (uint32_t)__shfl((int)s, (int)((lane - i) & 63u));
        om ^= lane >= i ? rs_mul(rs_readlane(lam, i), sv) : 0u;
    }

    // ---- Chien and Forney: the positions lane + 64 q ----
    uint32_t nroot = 0, bad = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
        if (n <= 64u * q)
            break;
        const uint32_t i = lane + 64u * q;
        const bool valid = i < n;
        const uint32_t p = valid ? n - 1u - i : 0u;
        const uint32_t xinv = rs_dev_alpha(255u - rs_locator_exp(c, p));
        uint32_t lamv = 0, omv = 0, der = 0, xp = 1u, xprev = 0u;  // xp = xinv^d, xprev = xinv^(d-1)
        for (uint32_t d = 0; d <= deg; d++) {
            const uint32_t ld = rs_readlane(lam, d), od = rs_readlane(om, d);
            lamv ^= rs_mul(ld, xp);
            omv ^= d < deg ? rs_mul(od, xp) : 0u;
            der ^= (d & 1u) ? rs_mul(ld, xprev) : 0u;
            xprev = xp;
            xp = rs_mul(xp, xinv);
        }
        const bool root = valid && lamv == 0u;
        nroot += (uint32_t)__builtin_popcountll(__ballot(root));
        // (rs_magnitude: X_p^(1 - fcr) omega / deriv)
        const uint32_t xf = rs_dev_alpha(rs_locator_exp(c, p) * ((256u - c.fcr) % 255u));
        const uint32_t v = root && der ? rs_mul(rs_mul(xf, omv), rs_dev_inv(der)) : 0u;
        bad |= root && !v ? 1u : 0u;
        e[q] = root ? v : 0u;
    }
    bool ok = nroot == deg && __ballot(bad != 0u) == 0ull;
    if (ok) {
        // the pattern's syndromes are the word's
        const uint32_t s2 = rs_horner(n, e, x);
        ok = __ballot(lane < nroots && s2 != s) == 0ull;
    }
    if (!ok) {
        e[0] = e[1] = e[2] = e[3] = 0u;
        return kRsFailed;
    }
    return deg;
}

}  // namespace

__global__ __launch_bounds__(64) void psk_rs_kernel(const RsDesc *__restrict__ desc, uint32_t nframe, const RsCode *__restrict__ codes,
                                                    const uint8_t *__restrict__ masks, psk_soft_rs_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x;
    uint32_t field = 0;  // the gfpoly of the tables in LDS
    for (uint32_t f = blockIdx.x; f < nframe; f += gridDim.x) {
        const RsDesc d = desc[f];
        psk_soft_rs_t *const rec = records + f;
        // (uniform for the wave, like every branch on the descriptor and the code below; the host has checked all of it)
        bool ok = (d.flags & kRsData) && d.code < kRsSlots && d.in && d.out;
        RsCode c = {};
        if (ok) {
            c = codes[d.code];
            ok = c.gfpoly >= 0x100u && c.gfpoly <= 0x1ffu && c.nroots >= 2u && c.nroots <= kRsMaxRoots && c.n > c.nroots && c.n <= 255u &&
                 c.depth >= 1u && c.depth <= kRsMaxDepth && c.mask_len <= c.n * c.depth;
        }
        if (!ok) {
            if (lane < 8u)
                ((PSK_RS_GLOBAL uint64_t *)rec)[lane] = 0ull;
            continue;
        }
        if (c.gfpoly != field) {  // (uniform)
            rs_tables(c.gfpoly, lane);
            field = c.gfpoly;
        }
        const uint32_t n = c.n, I = c.depth, k = n - c.nroots;
        const uint32_t n_out = (d.flags >> 1) & PSK_SOFT_RS_WITH_PARITY ? n : k;
        const PSK_RS_GLOBAL uint8_t *const in = (const PSK_RS_GLOBAL uint8_t *)d.in;
        const PSK_RS_GLOBAL uint8_t *const mask = (const PSK_RS_GLOBAL uint8_t *)masks + (size_t)d.code * kRsMaskStride;
        PSK_RS_GLOBAL uint8_t *const out = (PSK_RS_GLOBAL uint8_t *)d.out;
        const uint32_t x = lane < c.nroots ? rs_dev_alpha(c.prim * (c.fcr + lane)) : 0u;  // rs_root
        uint64_t errs = 0, bits_lo = 0, bits_hi = 0;  // n_err[0 .. 7], n_bit[0 .. 3], n_bit[4 .. 7] as the record holds them
        for (uint32_t j = 0; j < I; j++) {
            uint32_t w[4], e[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint32_t i = lane + 64u * q, off = i * I + j;
                w[q] = 0u;
                if (i < n) {
                    w[q] = in[off];
                    if (off < c.mask_len)
                        w[q] ^= mask[off];
                }
            }
            uint32_t s = rs_horner(n, w, x);
            s = lane < c.nroots ? s : 0u;
            uint32_t n_err = 0, n_bit = 0;
            if (__ballot(s != 0u) != 0ull) {
                n_err = rs_correct(c, s, x, lane, e);
                n_bit = rs_wave_sum((uint32_t)(__builtin_popcount(e[0]) + __builtin_popcount(e[1]) + __builtin_popcount(e[2]) + __builtin_popcount(e[3])));
            }
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint32_t i = lane + 64u * q;
                if (i < n_out)
                    out[i * I + j] = (uint8_t)(w[q] ^ e[q]);
            }
            errs |= (uint64_t)n_err << (8u * j);
            bits_lo |= j < 4u ? (uint64_t)n_bit << (16u * j) : 0ull;
            bits_hi |= j >= 4u ? (uint64_t)n_bit << (16u * (j - 4u)) : 0ull;
        }
        // the record's 64 bytes as eight words, one a lane: flags, n, k | depth, nroots, pad | n_err | n_bit | n_bit | pad
        if (lane < 8u) {
            const uint64_t head = (uint64_t)d.flags | ((uint64_t)n << 32) | ((uint64_t)k << 48);
            const uint64_t word = lane == 0u ? head : lane == 1u ? (uint64_t)(I | (c.nroots << 8)) : lane == 2u ? errs : lane == 3u ? bits_lo
                                                                                                             : lane == 4u ? bits_hi : 0ull;
            ((PSK_RS_GLOBAL uint64_t *)rec)[lane] = word;
        }
    }
}

hipError_t launch_rs(const RsDesc *desc, uint32_t nframe, uint32_t grid, const RsCode *codes, const uint8_t *masks, psk_soft_rs_t *records,
                     hipStream_t stream)
{
    if (!nframe || !grid)
        return hipSuccess;
    hipLaunchKernelGGL(psk_rs_kernel, dim3(grid), dim3(64), 0, stream, desc, nframe, codes, masks, records);
    return hipGetLastError();
}

}  // namespace psk
