// psk_wide.hip -- the front stage of the time-tiled kernels for wide symbols: samplesPerBaud 1025 .. 65535.
//
// psk_tile_front_any_kernel (psk_tile.hip) lays the timing phases of a symbol across the lanes, at most 16 a lane in registers:
// samplesPerBaud <= 1024.  A wide symbol has few symbols per call and many phases per symbol, so the parallel work is across the
// phases.  Two launches stand in for that kernel, and what comes behind them (parallel fit, fit, back) is the same:
//
//   chunk  grid (tiles, channels, phase chunks): one wave per tile, channel and chunk of 1024 timing phases.  It runs the
//          walk of the 16-phases-a-lane front stage over its chunk -- the window sums in double, in the reference's order of
//          additions (cpp/psk_soft.cpp:445-452: a symbol's energies are added as its samples arrive; :572-577: the leaving
//          symbol's are subtracted after the pick), the tile's first window a fresh sum as there -- and writes per symbol a
//          record: the chunk's first maximum, its runner-up and the phase.  A symbol's loads are 8 KiB contiguous per chunk.
//          Per tile and chunk it writes the exponent range and the largest of the energies it loaded, and whether one was
//          not finite.
//   pick   grid (tiles, channels): one wave per tile and channel, a lane per symbol.  It merges the chunk records of a symbol
//          in phase order -- the larger sum wins, the lower phase on a tie: std::max_element with `<` (:462), the first maximum
//          -- and then does what the 16-phases-a-lane kernel does after its pick: the picked sample, its M-th power, atan2f,
//          the raw phase and the sample to scratch, sampleIndex to the caller, and the tile's TileInfo for the fit kernel's
//          fold (tile_fold, psk_tile.hip).
//
// Non-finite sums.  The reference's first maximum skips NaN sums except at phase 0, which a merge of chunk maxima does not
// reproduce.  It need not: a NaN or infinite sum needs a non-finite sample energy (finite float energies summed in double do
// not overflow), every such energy sets the tile's refuse flag, and the fit kernel's fold then hands the call to the
// reference-order kernel (ChanState::guard = 1; psk_kernels.hip, the PSK_SEQ_WIDE build), nothing committed.  The pick of such
// a call is still a sample of its symbol: the phase is clamped to the symbol.
//
// Offsets: sample j of the call = symbol * samplesPerBaud + phase, in 64 bits (65535 * 2^15 already passes 2^31).
#include "psk_tile_kernel.h"
#include "psk_tile_any.h"

namespace psk {

constexpr int kWideChunk = 1024;  // phases of a chunk: 16 a lane
constexpr int kWideNP = kWideChunk / kWave;

struct WideRec {  // one symbol's pick within one chunk
    double best, second;
    uint32_t k;  // phase of `best` within the SYMBOL (chunk offset included); 0x7fffffff: every sum of the chunk was NaN
    uint32_t pad;
};
struct WideStat {  // one tile's energies within one chunk
    uint32_t umax, umin1, refuse;
    float emax;
};

__global__ __launch_bounds__(64) void psk_wide_chunk_kernel(const ChanPlan *__restrict__ plans, const uint32_t *__restrict__ list,
                                                            uint32_t ch0, const float2 *__restrict__ rings, uint32_t ring_cap,
                                                            WideRec *__restrict__ rec, WideStat *__restrict__ wst, uint32_t zmax)
{
    const int lane = threadIdx.x & 63;
    const uint32_t bi = list[blockIdx.y];
    const ChanPlan &p = plans[bi];
    if (!tile_plan_mine(p) || !(p.lf_flags & PLAN_ANYFRONT))
        return;
    const uint32_t S = p.S, z = blockIdx.z;
    const uint32_t k0 = z * (uint32_t)kWideChunk;
    if (k0 >= S)
        return;  // (the launch is sized for its widest channel)
    const int n_out = (int)p.n_out;
    const int n_blocks = (n_out + kB - 1) / kB;
    const int c_begin = (int)(blockIdx.x * p.tile_blocks);
    if (c_begin >= n_blocks)
        return;
    const int c_end = c_begin + (int)p.tile_blocks < n_blocks ? c_begin + (int)p.tile_blocks : n_blocks;
    const int i_begin = c_begin * kB, i_end = c_end * kB < n_out ? c_end * kB : n_out;
    const uint32_t ch = ch0 + bi;
    XView X;
    X.ring = reinterpret_cast<const f2g *>(rings + ((size_t)ch * 2u + p.ring_src) * ring_cap);
    X.in = reinterpret_cast<const f2g *>(p.in);
    X.L0 = p.ring_len0;
    const int A = (int)p.A;
    const int nk = S - k0 < (uint32_t)kWideChunk ? (int)(S - k0) : kWideChunk;  // phases of this chunk

    unsigned umax = 0u, umin1 = 0xFFFFFFFFu;
    bool refuse = false;
    float emax = 0.0f;
    // phase lane + 64 j of the chunk of symbol tau: entering samples go through the guard's bookkeeping, leaving ones have been
    // through it when they entered
    auto load = [&](long long tau, float (&e)[kWideNP], bool book) {
        const uint64_t j0 = (uint64_t)tau * (uint64_t)S + k0;
#pragma unroll
        for (int j = 0; j < kWideNP; j++) {
            const int k = lane + kWave * j;
            float en = 0.0f;
            if (k < nk) {
                const float2 v = x_at(X, j0 + (uint64_t)k);
                en = norm_f(v.x, v.y);
                if (book) {
                    const unsigned eb = __float_as_uint(en);
                    if (eb >= 0x7F800000u)
                        refuse = true;  // (inf / NaN: the reference-order kernel's)
                    umax = eb > umax ? eb : umax;
                    umin1 = (eb - 1u) < umin1 ? (eb - 1u) : umin1;
                    emax = __builtin_fmaxf(emax, en);
                }
            }
            e[j] = en;
        }
    };
    double W[kWideNP];
#pragma unroll
    for (int j = 0; j < kWideNP; j++) W[j] = 0.0;
    // the window in front of the tile's first symbol: symbols i_begin .. i_begin + numAvg - 2, in order
    const long long tau_end = (long long)i_begin + A - 1;
    for (long long tau = i_begin; tau < tau_end; tau++) {
        float e[kWideNP];
        load(tau, e, true);
#pragma unroll
        for (int j = 0; j < kWideNP; j++) W[j] += (double)e[j];
    }
    // (the next symbol's two loads are in flight while this one is reduced)
    float e_in[kWideNP], e_out[kWideNP];
    load((long long)i_begin + A - 1, e_in, true);
    load(i_begin, e_out, false);
    WideRec *const rec_row = rec + p.tile_off * zmax + z;
    for (int i = i_begin; i < i_end; i++) {
        float n_in[kWideNP], n_out_e[kWideNP];
        const bool more = i + 1 < i_end;
        if (more) {
            load((long long)i + A, n_in, true);
            load(i + 1, n_out_e, false);
        }
        // the newest symbol of the window arrives
#pragma unroll
        for (int j = 0; j < kWideNP; j++) W[j] += (double)e_in[j];
        // first maximum over the chunk's phases and the runner-up (as psk_tile_front_any_kernel)
        AnyTop top;
        top.best = -__builtin_inf();
        top.second = -__builtin_inf();
        top.k = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < kWideNP; j++) {
            const int k = lane + kWave * j;
            if (k < nk) {
                AnyTop one;
                one.best = W[j];
                one.second = -__builtin_inf();
                one.k = k;
                top = any_merge(top, one);
            }
        }
        const double best = any_max_f64(top.best);
        const unsigned k_win = any_min_u32(top.best == best ? (unsigned)top.k : 0xFFFFFFFFu);
        const double second = any_max_f64((unsigned)top.k == k_win ? top.second : top.best);
        if (lane == 0) {
            WideRec r;
            r.best = best;
            r.second = second;
            r.k = k_win < (unsigned)nk ? k0 + k_win : 0x7fffffffu;
            r.pad = 0u;
            rec_row[(size_t)i * zmax] = r;
        }
        // the oldest symbol of the window leaves
#pragma unroll
        for (int j = 0; j < kWideNP; j++) W[j] -= (double)e_out[j];
        if (more) {
#pragma unroll
            for (int j = 0; j < kWideNP; j++) e_in[j] = n_in[j], e_out[j] = n_out_e[j];
        }
    }
    const unsigned umax_w = wave_max_u32(umax), umin1_w = wave_min_u32(umin1);
    const bool refuse_w = vote_any(refuse);
    const float emax_w = wave_max_f32(__builtin_fmaxf(emax, 0.0f));
    if (lane == 0) {
        WideStat s;
        s.umax = umax_w;
        s.umin1 = umin1_w;
        s.refuse = refuse_w ? 1u : 0u;
        s.emax = emax_w;
        wst[(size_t)(p.tile_base + blockIdx.x) * zmax + z] = s;
    }
}

__global__ __launch_bounds__(64) void psk_wide_pick_kernel(const ChanPlan *__restrict__ plans, const uint32_t *__restrict__ list,
                                                           uint32_t ch0, const float2 *__restrict__ rings, uint32_t ring_cap,
                                                           const WideRec *__restrict__ rec, const WideStat *__restrict__ wst, uint32_t zmax,
                                                           TileInfo *__restrict__ tiles, float *__restrict__ t_raw, float2 *__restrict__ t_s,
                                                           PfChan *__restrict__ pf_chan)
{
    const int lane = threadIdx.x & 63;
    const uint32_t bi = list[blockIdx.y];
    const ChanPlan &p = plans[bi];
    if (!tile_plan_mine(p) || !(p.lf_flags & PLAN_ANYFRONT))
        return;
    const int n_out = (int)p.n_out;
    const int n_blocks = (n_out + kB - 1) / kB;
    const int c_begin = (int)(blockIdx.x * p.tile_blocks);
    if (c_begin >= n_blocks)
        return;
    if (blockIdx.x == 0 && lane == 0)  // the call's entry in the parallel fit's bookkeeping (psk_pfit.h: PfChan) starts clean
        pf_chan[bi].fail = pf_chan[bi].done = pf_chan[bi].slow_blocks = pf_chan[bi].retry = 0u;
    const int c_end = c_begin + (int)p.tile_blocks < n_blocks ? c_begin + (int)p.tile_blocks : n_blocks;
    const int i_begin = c_begin * kB, i_end = c_end * kB < n_out ? c_end * kB : n_out;
    const uint32_t ch = ch0 + bi;
    XView X;
    X.ring = reinterpret_cast<const f2g *>(rings + ((size_t)ch * 2u + p.ring_src) * ring_cap);
    X.in = reinterpret_cast<const f2g *>(p.in);
    X.L0 = p.ring_len0;
    const uint32_t S = p.S, M = p.M, A = p.A;
    const uint32_t Z = (S + kWideChunk - 1) / kWideChunk;
    const AtanTabDev atab = atan_tab_dev(lane);
    float *raw_row = t_raw + p.tile_off;
    float2 *s_row = t_s + p.tile_off;
    const WideRec *const rec_row = rec + p.tile_off * zmax;

    float gap_rel = __builtin_inff(), wmax = 0.0f;
    unsigned k_last = 0u;
    bool refuse = false;
    for (int g = i_begin; g < i_end; g += kWave) {
        const int i = g + lane;
        const bool live = i < i_end;
        AnyTop top;
        top.best = -__builtin_inf();
        top.second = -__builtin_inf();
        top.k = 0x7fffffff;
        for (uint32_t z = 0; live && z < Z; z++) {  // in phase order: the first maximum stays in front on a tie
            const WideRec r = rec_row[(size_t)i * zmax + z];
            AnyTop one;
            one.best = r.best;
            one.second = r.second;
            one.k = (int)r.k;
            top = any_merge(top, one);
        }
        // (every sum NaN: the tile refuses, see above -- the pick is clamped to the symbol)
        const uint32_t kbest = live && (uint32_t)top.k < S ? (uint32_t)top.k : 0u;
        k_last = (i == i_end - 1) ? kbest : k_last;
        wmax = live ? __builtin_fmaxf(wmax, (float)top.best * 1.0000002f) : wmax;
        const float gq = (float)(top.best - top.second) / (2.0f * drift_bound(i + 1 + kB, A));
        const float gap_new = (gq < gap_rel) ? gq : ((gq == gq) ? gap_rel : 0.0f);
        gap_rel = live ? gap_new : gap_rel;
        // the pick (cpp/psk_soft.cpp:465): its M-th power and raw phase
        const uint64_t j_pick = live ? (uint64_t)i * (uint64_t)S + kbest : (uint64_t)X.L0;
        const float2 pk = x_at(X, j_pick);
        cf32 sv;
        sv.re = pk.x, sv.im = pk.y;
        const cf32 pw = cpow_uint<false>(sv, M);
        const float raw = atan2f_wave(pw.im, pw.re, atab);
        if (live) {
            if (!(is_fin(pw.re) && is_fin(pw.im)))
                refuse = true;
            raw_row[i] = raw;
            s_row[i] = pk;
            if (p.sidx)
                p.sidx[i] = (int16_t)(unsigned short)kbest;  // (short)(unsigned short)k, as the reference narrows it
        }
    }
    // the tile's energies, over its chunks
    unsigned umax = 0u, umin1 = 0xFFFFFFFFu, refuse_b = refuse ? 1u : 0u;
    float emax = 0.0f;
    for (uint32_t z = (uint32_t)lane; z < Z; z += kWave) {
        const WideStat s = wst[(size_t)(p.tile_base + blockIdx.x) * zmax + z];
        umax = s.umax > umax ? s.umax : umax;
        umin1 = s.umin1 < umin1 ? s.umin1 : umin1;
        refuse_b |= s.refuse;
        emax = __builtin_fmaxf(emax, s.emax);
    }
    const unsigned umax_w = wave_max_u32(umax), umin1_w = wave_min_u32(umin1);
    const bool refuse_w = vote_any(refuse_b != 0u);
    const float emax_w = wave_max_f32(__builtin_fmaxf(emax, 0.0f));
    // (gap_rel and wmax are non-negative, +inf or NaN: their bit patterns order like the values, a NaN maximum stays on top)
    const unsigned gap_b = wave_min_u32(__float_as_uint(gap_rel)), wmax_b = wave_max_u32(__float_as_uint(wmax));
    const unsigned k_last_w = wave_max_u32(k_last);
    if (lane == 0) {
        TileInfo &t = tiles[p.tile_base + blockIdx.x];
        t.umax = umax_w;
        t.umin1 = umin1_w;
        t.refuse = refuse_w ? 1u : 0u;
        t.gap_rel = __uint_as_float(gap_b);
        t.wmax = __uint_as_float(wmax_b);
        t.stat_exact = (uint32_t)(c_end - c_begin);
        t.last_k = k_last_w;
        t.cap = __builtin_inff();
        t.emax = emax_w;
    }
}

size_t wide_rec_bytes() { return sizeof(WideRec); }
size_t wide_stat_bytes() { return sizeof(WideStat); }
uint32_t wide_chunks(uint32_t S) { return (S + kWideChunk - 1) / kWideChunk; }

// rec: wide_rec_bytes() x (symbols of the launch's tiles) x zmax; wst: wide_stat_bytes() x (tiles of the launch) x zmax, zmax =
// wide_chunks(largest samplesPerBaud of the launch) <= 64
hipError_t launch_wide_front(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, uint32_t max_tiles, uint32_t max_S,
                             const float2 *rings, uint32_t ring_cap, TileInfo *tiles, float *t_raw, float2 *t_s, PfChan *pf_chan, void *rec,
                             void *wst, hipStream_t stream)
{
    if (!nch || !max_tiles)
        return hipSuccess;
    const uint32_t zmax = wide_chunks(max_S);
    for (uint32_t off = 0; off < nch; off += kGridYMax) {  // (channels are the grid's y dimension: slices of 65535)
        const uint32_t n = nch - off < kGridYMax ? nch - off : kGridYMax;
        hipLaunchKernelGGL(psk_wide_chunk_kernel, dim3(max_tiles, n, zmax), dim3(kWave), 0, stream, plans, list + off, ch0, rings, ring_cap,
                           static_cast<WideRec *>(rec), static_cast<WideStat *>(wst), zmax);
    }
    for (uint32_t off = 0; off < nch; off += kGridYMax) {
        const uint32_t n = nch - off < kGridYMax ? nch - off : kGridYMax;
        hipLaunchKernelGGL(psk_wide_pick_kernel, dim3(max_tiles, n), dim3(kWave), 0, stream, plans, list + off, ch0, rings, ring_cap,
                           static_cast<const WideRec *>(rec), static_cast<const WideStat *>(wst), zmax, tiles, t_raw, t_s, pf_chan);
    }
    return hipGetLastError();
}

}  // namespace psk
