// psk_symrate.h -- what the host (psk_capi.cpp) and the symbol-rate pass of psk_soft_symrate_device (psk_symrate.hip) share, and
// the per-sample, per-block and per-lag terms of include/psk_soft_hip.h ("symbol rate of a packet"), which psk_soft_symrate_host
// (host) and the kernels (device) both take from here.
#ifndef PSK_SYMRATE_H
#define PSK_SYMRATE_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_soft_hip.h"

namespace psk {

constexpr uint32_t kSymrateLags = 8;            // lags of 1, 2, 4 .. 128 blocks
constexpr uint32_t kSymrateHalo = 128;          // the longest lag: blocks in front of a piece that its products reach back to
constexpr uint32_t kSymratePiece = 512;         // blocks of one piece of the fold: a constant, never derived from the batch
constexpr uint32_t kSymrateMaxBlocks = 4096;    // blocks a look uses at the most
constexpr uint32_t kSymrateThreads = 256;
constexpr uint32_t kSymrateMinS = 4, kSymrateMaxS = 1024;
// what one piece adds up -- doubles: per detector z sum_re[8] at 16 z, sum_im[8] at 16 z + 8; sum_pow[2] at 32, sum_lvl[2] at 34;
// counts: n_pairs[8], n_valid
constexpr uint32_t kSymrateSums = 4u * kSymrateLags + 4u, kSymrateCounts = kSymrateLags + 1u;

// One covered channel of one call.  flags: PSK_SOFT_SR_DATA (a data record; without it the join writes the zero record and the
// fold has nothing to do), PSK_SOFT_SR_TUNED (phase / step are applied).
struct SymrateDesc {
    const void *src;
    uint64_t stride;  // in complex samples of the format; 1: contiguous
    uint64_t n;       // complex samples of the packet (the look reads the first n_blocks * S of them)
    uint64_t phase, step;
    uint64_t wstep;           // sr_wstep(S)
    uint32_t n_blocks;
    uint32_t part0, n_piece;  // the packet's partials: [part0, part0 + n_piece) of the scratch
    uint32_t channel;         // of the handle
    uint16_t S;
    uint8_t format, flags;
};

struct SymratePartial {
    double d[kSymrateSums];
    uint32_t c[kSymrateCounts];
    uint32_t pad;  // (never written, never read)
};

#if defined(__HIPCC__)
#define PSK_SR_HD __host__ __device__
#else
#define PSK_SR_HD
#endif

PSK_SR_HD inline bool sr_finite(float v)
{
    return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u;
}

// floor(2^64 / S), S >= 2: the phase word of one position of a block
PSK_SR_HD inline uint64_t sr_wstep(uint32_t S)
{
    const uint64_t q = ~(uint64_t)0 / S;
    return ~(uint64_t)0 % S == S - 1u ? q + 1u : q;
}
// the phase word of position p of a block: it restarts in every block
PSK_SR_HD inline uint64_t sr_phase(uint32_t p, uint64_t wstep) { return (uint64_t)0 - (uint64_t)p * wstep; }

// lanes that share one block in the device's fold (a power of two, 1 .. 64; about eight positions a lane, so that the tree is
// the smaller part of the work): lane l of them adds the positions l, l + W, ... in that order, then the lanes are added by a
// xor tree.  S <= 8: one lane a block, no tree.  The host adds in index order; the model of the tests restates this one.
PSK_SR_HD inline uint32_t sr_width(uint32_t S)
{
    uint32_t w = 1;
    while (8u * w < S && w < 64u) w <<= 1;
    return w;
}

// One sample and the one in front of it (has_prev: there is one).  *e is the envelope term, *g the transition term; returns
// whether the sample lets its block stay valid.
PSK_SR_HD inline bool sr_sample(float re, float im, float pre, float pim, bool has_prev, float *e_out, float *g_out)
{
    const float e = re * re + im * im;
    const float dr = re - pre, di = im - pim;
    const float g = has_prev ? dr * dr + di * di : 0.0f;
    *e_out = e, *g_out = g;
    return sr_finite(re) && sr_finite(im) && (!has_prev || (sr_finite(pre) && sr_finite(pim))) && sr_finite(e) && sr_finite(g);
}

// the two float32 products of one detector's term with the phasor of its position
PSK_SR_HD inline void sr_term(float z, float c, float s, float *t_re, float *t_im)
{
    *t_re = z * c;
    *t_im = z * s;
}

// B[m] * conj(B[m - L]) and |B[m]|^2, in doubles (the units that include this are built with -ffp-contract=off)
PSK_SR_HD inline void sr_lag(double ar, double ai, double br, double bi, double *t_re, double *t_im)
{
    *t_re = ar * br + ai * bi;
    *t_im = ai * br - ar * bi;
}
PSK_SR_HD inline double sr_pow(double ar, double ai) { return ar * ar + ai * ai; }

// grid (max_piece, packets): the partials of every piece of every data packet.  d_tab: the phasor tables in device memory
// (always needed: the block phasors come from them).
hipError_t launch_symrate_fold(const SymrateDesc *desc, uint32_t nch, uint32_t max_piece, const float *d_tab, SymratePartial *part,
                               hipStream_t stream);
// one wave per packet: the partials in piece order, the record (or the zero record)
hipError_t launch_symrate_join(const SymrateDesc *desc, uint32_t nch, const SymratePartial *part, psk_soft_symrate_t *records,
                               hipStream_t stream);

}  // namespace psk
#endif
