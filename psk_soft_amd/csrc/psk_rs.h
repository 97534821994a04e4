// psk_rs.h -- what the host (psk_capi.cpp) and the decoder of psk_soft_rs_device (psk_rs.hip) share, and the terms of
// include/psk_soft_rs.h ("frames as corrected bytes"): the field multiply, power and inverse (shift-and-xor; the host computes
// with them, the kernel builds its exp / log tables with them and multiplies by table), the code struct, the roots of the
// generator, the locator of a position and the magnitude of an error (Forney), which the kernel restates in table terms.
//
// The definition, restated.  GF(256) = GF(2)[x] / gfpoly with alpha = 2 primitive.  Byte i of a codeword of n bytes is the
// coefficient of x^(n-1-i): position i has the power p = n-1-i and the locator X_p = beta^p with beta = alpha^prim.  The generator's
// roots are beta^(fcr + m), m = 0 .. nroots-1, so an error pattern e has the syndromes S_m = sum_p e_p X_p^(fcr + m).  With
// Lambda(x) = prod (1 - X_p x), Omega = S Lambda mod x^nroots and Lambda' the formal derivative,
// e_p = X_p^(1 - fcr) Omega(1 / X_p) / Lambda'(1 / X_p).  Everything is a field element: no rounding, no order to keep.
#ifndef PSK_RS_H
#define PSK_RS_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_soft_hip.h"

namespace psk {

constexpr uint32_t kRsSlots = PSK_SOFT_RS_SLOTS;
constexpr uint32_t kRsMaxFrames = PSK_SOFT_RS_MAX_FRAMES;
constexpr uint32_t kRsMaxDepth = PSK_SOFT_RS_MAX_DEPTH;
constexpr uint32_t kRsMaxRoots = PSK_SOFT_RS_MAX_ROOTS;
constexpr uint32_t kRsFailed = PSK_SOFT_RS_FAILED;
constexpr uint32_t kRsMaskBytes = 255u * PSK_SOFT_RS_MAX_DEPTH;  // the longest frame, and so the longest mask
constexpr uint32_t kRsMaskStride = 2048u;                        // bytes of device memory per slot's mask
constexpr uint32_t kRsFlagMask = PSK_SOFT_RS_WITH_PARITY;
constexpr uint32_t kRsMaxGrid = 65535u;                          // workgroups of a launch (8192 was measured slower: DESIGN.md 2.16)

enum : uint32_t { kRsData = 1u };  // RsDesc::flags bit 0: the frame is decoded; the frame's flags << 1 above it

// a code as the kernel reads it: wave-uniform, 32 bytes.  gfpoly == 0: the slot was never defined
struct RsCode {
    uint32_t gfpoly, fcr, prim, nroots;
    uint32_t n, depth, mask_len, pad;
};
static_assert(sizeof(RsCode) == 32, "a code is 32 bytes");

// One frame of one call.  Without kRsData the kernel writes the zero record and nothing else.
struct RsDesc {
    const uint8_t *in;
    uint8_t *out;
    uint32_t code;   // the slot
    uint32_t flags;  // kRsData | the frame's PSK_SOFT_RS_* flags << 1: the record's flags as they are
    uint32_t pad[2];
};
static_assert(sizeof(RsDesc) == 32, "a descriptor is 32 bytes");

#if defined(__HIPCC__)
#define PSK_RS_HD __host__ __device__
#else
#define PSK_RS_HD
#endif

// a * b in GF(2)[x] / gfpoly: eight shift-and-xor steps, no table (the host's multiply; the kernel builds its tables with it)
PSK_RS_HD inline uint32_t gf_mul(uint32_t gfpoly, uint32_t a, uint32_t b)
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        r <<= 1;
        r ^= (r & 0x100u) ? gfpoly : 0u;
        r ^= ((b >> i) & 1u) ? a : 0u;
    }
    return r;
}
// a^e, e = 0 .. 255
PSK_RS_HD inline uint32_t gf_pow(uint32_t gfpoly, uint32_t a, uint32_t e)
{
    uint32_t r = 1;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        r = gf_mul(gfpoly, r, r);
        r = ((e >> i) & 1u) ? gf_mul(gfpoly, r, a) : r;
    }
    return r;
}
// 1 / a = a^254 (a != 0; 0 gives 0)
PSK_RS_HD inline uint32_t gf_inv(uint32_t gfpoly, uint32_t a) { return gf_pow(gfpoly, a, 254u); }

PSK_RS_HD inline uint32_t rs_gcd(uint32_t a, uint32_t b)
{
    while (b) {
        const uint32_t r = a % b;
        a = b, b = r;
    }
    return a;
}

// what psk_soft_rs_define refuses of a code
inline bool rs_code_ok(uint32_t gfpoly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t depth, uint32_t mask_len)
{
    if (gfpoly < 0x100u || gfpoly > 0x1ffu || fcr > 254u || prim < 1u || prim > 254u || rs_gcd(prim, 255u) != 1u)
        return false;
    if (nroots < 2u || nroots > kRsMaxRoots || n < nroots + 1u || n > 255u || depth < 1u || depth > kRsMaxDepth || mask_len > n * depth)
        return false;
    // alpha = 2 has order 255: its first return to 1 is at the 255th power
    uint32_t a = 1;
    for (uint32_t i = 1; i <= 255u; i++) {
        a <<= 1;
        a ^= (a & 0x100u) ? gfpoly : 0u;
        if (a == 1u)
            return i == 255u;
    }
    return false;
}

// alpha^e for any e below 2^24
PSK_RS_HD inline uint32_t rs_alpha_pow(uint32_t gfpoly, uint32_t e) { return gf_pow(gfpoly, 2u, e % 255u); }
// root m of the generator: alpha^(prim (fcr + m))
PSK_RS_HD inline uint32_t rs_root(const RsCode &c, uint32_t m) { return rs_alpha_pow(c.gfpoly, c.prim * (c.fcr + m)); }
// the exponent of alpha of the locator X_p of power p (p = n-1-i for byte i), 0 .. 254
PSK_RS_HD inline uint32_t rs_locator_exp(const RsCode &c, uint32_t p) { return (c.prim * p) % 255u; }
// 1 / X_p
PSK_RS_HD inline uint32_t rs_locator_inv(const RsCode &c, uint32_t p) { return rs_alpha_pow(c.gfpoly, 255u - rs_locator_exp(c, p)); }
// the error value at a root 1 / X_p of the locator polynomial: X_p^(1 - fcr) omega / deriv (deriv != 0)
PSK_RS_HD inline uint32_t rs_magnitude(const RsCode &c, uint32_t p, uint32_t omega, uint32_t deriv)
{
    const uint32_t x = rs_alpha_pow(c.gfpoly, rs_locator_exp(c, p) * ((256u - c.fcr) % 255u));
    return gf_mul(c.gfpoly, gf_mul(c.gfpoly, x, omega), gf_inv(c.gfpoly, deriv));
}

// Workgroups of one wave; workgroup w decodes the frames w, w + grid, ... of the call.  masks: kRsMaskStride bytes a slot.
hipError_t launch_rs(const RsDesc *desc, uint32_t nframe, uint32_t grid, const RsCode *codes, const uint8_t *masks, psk_soft_rs_t *records,
                     hipStream_t stream);

}  // namespace psk
#endif
