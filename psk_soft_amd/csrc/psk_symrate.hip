// psk_symrate.hip -- psk_soft_symrate_device: one look at a packet per channel, one psk_soft_symrate_t per channel.
//
// The record holds the lag products of the packet's block sums (include/psk_soft_hip.h, "symbol rate of a packet"); the host
// turns it into samples per symbol (psk_soft_symrate_derive).  One pass over the packets, two kernels:
//
//   fold   grid (pieces, packets), one workgroup of 256 lanes per piece of kSymratePiece blocks of one packet.
//          Stage 1: the piece's blocks and the kSymrateHalo blocks in front of it are folded into their sums.  W = sr_width(S)
//          adjacent lanes share a block (64 / W blocks a wave at a time, the four waves side by side; W = 1 up to S = 8, about
//          eight positions a lane beyond): lane l of them reads the samples at positions l, l + W, ... and the one in front of
//          each -- its own last one where W = 1 -- (src_load of psk_front_src.h for the four formats, rotated by src_rotate on
//          the tables in LDS), forms e, g and their products with the position's phasor (tune_phasor, the same tables) and
//          adds them in doubles in that order; a xor tree over the W lanes.  The six sums of a block
//          (B_e, B_g, the two levels) and its validity go into LDS -- zeros for an invalid block and for the halo of the
//          packet's first piece.
//          Stage 2: lane t takes the blocks t, t + 256 of the piece and forms their eight lag products for both detectors out
//          of LDS into double accumulators; a pair with an invalid block adds +0.  The pairs are counted per wave by a ballot.
//          A fixed xor-tree across each wave, the four waves in order: one partial per piece.
//   join   one wave per packet: the partials in a fixed order, the record; the zero record for a packet without data.
//
// Which lane adds which sample, and in which order, depends on the sample's index in the packet, on S and on the number of
// blocks only -- not on the format, the stride, the batch or the grid --, so the same samples give the same bytes.  No
// floating-point atomics.  The arithmetic (psk_symrate.h) is rounded once per operation (the unit is built with
// -ffp-contract=off), denormals kept.  Plain vector loads and stores only; the packets are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_front_src.h"
#include "psk_symrate.h"

namespace psk {

namespace {

constexpr uint32_t kWaves = kSymrateThreads / 64u;
constexpr uint32_t kSlots = kSymrateHalo + kSymratePiece;
constexpr uint32_t kBlockSums = 6;  // B_e (re, im), B_g (re, im), level e, level g

__device__ __forceinline__ double s_wave_sum(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Stage 1 of a piece: the blocks [start, hi) into the LDS slots b + halo - lo.
template <int FMT>
__device__ __forceinline__ void s_stage1(const SymrateDesc &d, const float *tab, double (*bq)[kSlots], uint32_t *vld, uint32_t start,
                                         uint32_t lo, uint32_t hi)
{
    const PSK_GLOBAL void *__restrict__ src = (const PSK_GLOBAL void *)d.src;
    const bool tuned = (d.flags & PSK_SOFT_SR_TUNED) != 0;
    const uint32_t S = d.S, W = sr_width(S), G = 64u / W;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t sub = lane / W, l = lane & (W - 1u);
    // the lanes of this lane's block, as a mask of the wave
    const uint64_t group = (W == 64u ? ~(uint64_t)0 : (((uint64_t)1 << W) - 1u)) << (sub * W);
    // (the bound is the wave's: every lane of it takes part in the tree and the ballot below)
    for (uint32_t base = start + wave * G; base < hi; base += kWaves * G) {
        const uint32_t b = base + sub;
        const bool live = b < hi;
        double a[kBlockSums];
#pragma unroll
        for (uint32_t j = 0; j < kBlockSums; j++) a[j] = 0.0;
        bool ok = true;
        f2 last = f2{0.0f, 0.0f};  // (W == 1: the sample in front is the lane's own last one, as it was rotated)
        for (uint32_t p0 = 0; p0 < S; p0 += W) {
            const uint32_t p = p0 + l;
            if (live && p < S) {
                const uint64_t k = (uint64_t)b * S + p;  // (< n_blocks * S <= d.n)
                const bool has_prev = k != 0, own = W == 1u && p0 != 0u;
                f2 x = src_load<FMT>(src, k * d.stride);
                f2 y = has_prev && !own ? src_load<FMT>(src, (k - 1u) * d.stride) : f2{0.0f, 0.0f};
                if (tuned) {
                    const uint64_t ph = d.phase + k * d.step;
                    x = src_rotate(tab, ph, x);
                    if (!own)
                        y = src_rotate(tab, ph - d.step, y);
                }
                if (own)
                    y = last;
                last = x;
                float e, g, c, s, tr, ti;
                ok = sr_sample(x.x, x.y, y.x, y.y, has_prev, &e, &g) && ok;
                tune_phasor(tab, sr_phase(p, d.wstep), &c, &s);
                sr_term(e, c, s, &tr, &ti);
                a[0] += (double)tr, a[1] += (double)ti;
                sr_term(g, c, s, &tr, &ti);
                a[2] += (double)tr, a[3] += (double)ti;
                a[4] += (double)e, a[5] += (double)g;
            }
        }
        for (uint32_t off = W >> 1; off >= 1u; off >>= 1) {
#pragma unroll
            for (uint32_t j = 0; j < kBlockSums; j++) a[j] += __shfl_xor(a[j], (int)off);
        }
        const bool valid = (__builtin_amdgcn_ballot_w64(ok) & group) == group;
        if (live && l == 0) {
            const uint32_t s = b + kSymrateHalo - lo;  // (< kSlots: b < lo + kSymratePiece)
#pragma unroll
            for (uint32_t j = 0; j < kBlockSums; j++) bq[j][s] = valid ? a[j] : 0.0;
            vld[s] = valid ? 1u : 0u;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kSymrateThreads) void psk_symrate_fold_kernel(const SymrateDesc *__restrict__ desc, uint32_t nch,
                                                                           const float *__restrict__ d_tab,
                                                                           SymratePartial *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float tab[kTuneTableFloats];
    __shared__ double bq[kBlockSums][kSlots];
    __shared__ uint32_t vld[kSlots];
    __shared__ double red_d[kWaves][kSymrateSums];
    __shared__ uint32_t red_c[kWaves][kSymrateCounts];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    src_tables_to_lds<kSymrateThreads>(tab, d_tab);
    for (uint32_t c = blockIdx.y; c < nch; c += gridDim.y) {
        const SymrateDesc d = desc[c];
        // (uniform for the workgroup, like every branch on the descriptor below)
        if (!(d.flags & PSK_SOFT_SR_DATA) || blockIdx.x >= d.n_piece)
            continue;
        const uint32_t lo = blockIdx.x * kSymratePiece;
        const uint32_t hi = d.n_blocks - lo < kSymratePiece ? d.n_blocks : lo + kSymratePiece;
        const uint32_t start = lo ? lo - kSymrateHalo : 0u;
        __syncthreads();  // (the tables are in place; the LDS of the packet before is read out)
        // no block is valid until stage 1 says so: the halo of the packet's first piece, the slots behind the packet's end
        for (uint32_t s = t; s < kSlots; s += kSymrateThreads) vld[s] = 0u;
        __syncthreads();
        src_dispatch(d.format, [&](auto fmt) { s_stage1<decltype(fmt)::value>(d, tab, bq, vld, start, lo, hi); });
        __syncthreads();
        // stage 2: block m of the piece sits in slot m + halo - lo, its partner of lag L in the slot L in front of it
        double sr[2][kSymrateLags], si[2][kSymrateLags], pw[2] = {0.0, 0.0}, lv[2] = {0.0, 0.0};
        uint32_t np[kSymrateLags], nv = 0;
#pragma unroll
        for (uint32_t j = 0; j < kSymrateLags; j++) sr[0][j] = si[0][j] = sr[1][j] = si[1][j] = 0.0, np[j] = 0;
        // (whole turns: the slots behind the packet's end are invalid, and the trip count is the same for every lane)
        const uint32_t turns = (hi - lo + kSymrateThreads - 1u) / kSymrateThreads;
        for (uint32_t turn = 0; turn < turns; turn++) {
            const uint32_t s = kSymrateHalo + turn * kSymrateThreads + t;
            const bool va = vld[s] != 0u;
            // (a slot stage 1 has not written holds whatever was there: read, never used)
            const double er = bq[0][s], ei = bq[1][s], gr = bq[2][s], gi = bq[3][s];
            pw[0] += va ? sr_pow(er, ei) : 0.0;
            pw[1] += va ? sr_pow(gr, gi) : 0.0;
            lv[0] += va ? bq[4][s] : 0.0;
            lv[1] += va ? bq[5][s] : 0.0;
            nv += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(va));
#pragma unroll
            for (uint32_t j = 0; j < kSymrateLags; j++) {
                const uint32_t sb = s - (1u << j);
                const bool ok = va && vld[sb] != 0u;
                double tr, ti;
                sr_lag(er, ei, bq[0][sb], bq[1][sb], &tr, &ti);
                sr[0][j] += ok ? tr : 0.0;
                si[0][j] += ok ? ti : 0.0;
                sr_lag(gr, gi, bq[2][sb], bq[3][sb], &tr, &ti);
                sr[1][j] += ok ? tr : 0.0;
                si[1][j] += ok ? ti : 0.0;
                np[j] += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
            }
        }
        // the wave's lanes by the fixed tree, then the waves in order
#pragma unroll
        for (uint32_t z = 0; z < 2u; z++) {
#pragma unroll
            for (uint32_t j = 0; j < kSymrateLags; j++) {
                const double r = s_wave_sum(sr[z][j]), i = s_wave_sum(si[z][j]);
                if (lane == 0)
                    red_d[wave][16u * z + j] = r, red_d[wave][16u * z + kSymrateLags + j] = i;
            }
            const double p = s_wave_sum(pw[z]), v = s_wave_sum(lv[z]);
            if (lane == 0)
                red_d[wave][32u + z] = p, red_d[wave][34u + z] = v;
        }
        if (lane == 0) {
#pragma unroll
            for (uint32_t j = 0; j < kSymrateLags; j++) red_c[wave][j] = np[j];
            red_c[wave][kSymrateLags] = nv;
        }
        __syncthreads();
        PSK_GLOBAL SymratePartial *const out = (PSK_GLOBAL SymratePartial *)part + (d.part0 + blockIdx.x);
        if (t < kSymrateSums) {
            double v = red_d[0][t];
            for (uint32_t w = 1; w < kWaves; w++) v += red_d[w][t];
            out->d[t] = v;
        } else if (t >= 64u && t < 64u + kSymrateCounts) {
            uint32_t v = 0;
            for (uint32_t w = 0; w < kWaves; w++) v += red_c[w][t - 64u];
            out->c[t - 64u] = v;
        }
    }
}

__global__ __launch_bounds__(64) void psk_symrate_join_kernel(const SymrateDesc *__restrict__ desc, uint32_t nch,
                                                              const SymratePartial *__restrict__ part,
                                                              psk_soft_symrate_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const SymrateDesc d = desc[c];
        const bool data = (d.flags & PSK_SOFT_SR_DATA) != 0;
        double s[kSymrateSums];
        uint64_t n[kSymrateCounts];
#pragma unroll
        for (uint32_t j = 0; j < kSymrateSums; j++) s[j] = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < kSymrateCounts; j++) n[j] = 0;
        // lane l adds the partials l, l + 64, ... in that order; then the fixed tree
        for (uint32_t k = lane; data && k < d.n_piece; k += 64u) {
            const PSK_GLOBAL SymratePartial *const p = (const PSK_GLOBAL SymratePartial *)part + (d.part0 + k);
#pragma unroll
            for (uint32_t j = 0; j < kSymrateSums; j++) s[j] += p->d[j];
#pragma unroll
            for (uint32_t j = 0; j < kSymrateCounts; j++) n[j] += p->c[j];
        }
#pragma unroll
        for (uint32_t j = 0; j < kSymrateSums; j++) s[j] = s_wave_sum(s[j]);
#pragma unroll
        for (uint32_t j = 0; j < kSymrateCounts; j++)
            for (int off = 32; off >= 1; off >>= 1) n[j] += (uint64_t)__shfl_xor((long long)n[j], off);
        if (lane != 0)
            continue;
        psk_soft_symrate_t r = {};  // (pad stays zero; lane 0 alone stores the 392 bytes)
        if (data) {
            r.n_samples = d.n;
            r.n_blocks = d.n_blocks;
            r.n_used = (uint64_t)d.n_blocks * d.S;
            r.n_valid = n[kSymrateLags];
            for (uint32_t z = 0; z < 2u; z++) {
                for (uint32_t j = 0; j < kSymrateLags; j++) {
                    r.sum_re[z][j] = s[16u * z + j];
                    r.sum_im[z][j] = s[16u * z + kSymrateLags + j];
                }
                r.sum_pow[z] = s[32u + z];
                r.sum_lvl[z] = s[34u + z];
            }
            for (uint32_t j = 0; j < kSymrateLags; j++) r.n_pairs[j] = n[j];
            r.samplesPerBaud = d.S;
            r.flags = d.flags;
        }
        records[d.channel] = r;
    }
}

hipError_t launch_symrate_fold(const SymrateDesc *desc, uint32_t nch, uint32_t max_piece, const float *d_tab, SymratePartial *part,
                               hipStream_t stream)
{
    if (!nch || !max_piece)
        return hipSuccess;
    const dim3 grid(max_piece, nch < 65535u ? nch : 65535u);
    hipLaunchKernelGGL(psk_symrate_fold_kernel, grid, dim3(kSymrateThreads), 0, stream, desc, nch, d_tab, part);
    return hipGetLastError();
}

hipError_t launch_symrate_join(const SymrateDesc *desc, uint32_t nch, const SymratePartial *part, psk_soft_symrate_t *records,
                               hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    hipLaunchKernelGGL(psk_symrate_join_kernel, dim3(nch < 65535u ? nch : 65535u), dim3(64), 0, stream, desc, nch, part, records);
    return hipGetLastError();
}

}  // namespace psk
