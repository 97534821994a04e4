// psk_farfit.hip -- the fit stage of the time-tiled kernels for fit windows no LDS holds: phaseAvg 32641 .. 65535
// (PSK_SOFT_OPT_FAR_FIT, PLAN_FARFIT).
//
// psk_tile_fit_kernel (psk_tile.hip) keeps LinearFit::yvals of the running call in an LDS ring of phaseAvg + 128 floats, and
// 32768 floats is all the LDS there is.  The ring is not needed there for a window of 128 values or more: the value that leaves
// the window at position t is y[t - n], pushed at least n - 127 positions -- 255 blocks -- before the block that needs it.  This
// kernel is that one with the ring in device memory (psk_fast_loop.h: far_ring_fence, the FAR variants): a row of kFarRingFloats floats per channel in a
// scratch of the handle.  Per block: one coalesced read of the 128 leaving values ahead of the unwrap passes, which work on
// registers as before, and one store of the block's own 128 values once their counts are final -- 1 KiB of traffic a block.
// The row is NOT the channel's yvals buffer (`yv`): a call the exactness guard or the unwrap refuses is redone by the
// reference-order kernel from the old state, which writing in place would have destroyed (fit_cap == phaseAvg + 1).  The prologue
// copies the carried values in, the epilogue writes the surviving ones back, as for the LDS ring.
// Front and back stage are the ordinary ones (psk_tile.hip, psk_wide.hip); the parallel fit is not attempted.
#include "psk_tile_kernel.h"

namespace psk {

// a power of two >= phaseAvg + 128 for every phaseAvg a ushort holds: 512 KiB a row
constexpr uint32_t kFarRingFloats = 131072u;

// ---- fit: one wave per channel ----
__global__ __launch_bounds__(64) void psk_far_fit_kernel(const ChanPlan *__restrict__ plans, const uint32_t *__restrict__ list, uint32_t ch0,
                                                         ChanState *__restrict__ states, float2 *__restrict__ rings, uint32_t ring_cap,
                                                         float *__restrict__ yvs, uint32_t fit_cap, float *__restrict__ far_y,
                                                         uint32_t far_rows, TileInfo *__restrict__ tiles, const float *__restrict__ t_raw,
                                                         const float2 *__restrict__ t_s, float *__restrict__ t_est)
{
    const int lane = threadIdx.x & 63;
    const uint32_t bi = list[blockIdx.x];
    const ChanPlan &p = plans[bi];
    if (!tile_plan_mine(p) || !(p.lf_flags & PLAN_FARFIT))
        return;
    const uint32_t ch = ch0 + bi;
    ChanState *st = &states[ch];
    const int n_out = (int)p.n_out;
    const int n_blocks = (n_out + kB - 1) / kB;
    const int n_tiles = (n_blocks + (int)p.tile_blocks - 1) / (int)p.tile_blocks;
    TileInfo *const ti = tiles + p.tile_base;

    int exact_blocks = 0;
    float emax = 0.0f;
    // (a row outside the scratch -- the host never plans one -- is refused like a call the tiles cannot carry, not written to)
    const bool refuse = tile_fold(p, ti, n_tiles, lane, exact_blocks, emax) || p.far_row >= far_rows;
    if (lane == 0)
        st->emax_hint = emax;  // (not part of the reference's state: kept whether or not the call stays here)
    if (refuse) {
        if (lane == 0) {
            st->guard = 1u;
            atomicAdd(p.handed_over, 1u);
        }
        return;
    }

    float2 *ring_base = rings + (size_t)ch * 2u * ring_cap;
    const float2 *ring_src = ring_base + (size_t)p.ring_src * ring_cap;
    float2 *ring_dst = ring_base + (size_t)(p.ring_src ^ 1u) * ring_cap;
    float *yv = yvs + (size_t)ch * fit_cap;
    XView X;
    X.ring = reinterpret_cast<const f2g *>(ring_src);
    X.in = reinterpret_cast<const f2g *>(p.in);
    X.L0 = p.ring_len0;

    float *const yring = far_y + (size_t)p.far_row * kFarRingFloats;
    const uint32_t ymask = kFarRingFloats - 1u;
    FastCarry cy;
    call_prologue<true>(p, st, yv, fit_cap, yring, ymask, lane, cy);  // (the carried values into the row, and a fence behind them)
    const float last0_re = cy.last_re, last0_im = cy.last_im;

    const uint32_t n = p.lf_n;
    const float xd = p.lf_xdelta;
    float den_s = cy.den, xavg_s = cy.xavg;
    if (n > 1)
        fit_denominator(xd, n, den_s, xavg_s);
    const FitKnown fk = fit_known(xd, n, den_s, xavg_s);
    const float *raw_row = t_raw + p.tile_off;
    float *est_row = t_est + p.tile_off;
    float2 nxt = *reinterpret_cast<const float2 *>(raw_row + 2 * lane);
    for (int c = 0; c < n_blocks; c++) {
        const int i0 = c * kB + 2 * lane;
        const float raw[kR] = {nxt.x, nxt.y};
        if (c + 1 < n_blocks)  // (the next block's raw phases are on their way while this one is fitted)
            nxt = *reinterpret_cast<const float2 *>(raw_row + i0 + kB);
        const bool valid[kR] = {i0 < n_out, i0 + 1 < n_out};
        const int rem = n_out - c * kB;
        const int nvalid = rem < kB ? rem : kB;
        const int lane_last = (nvalid - 1) >> 1, r_last = (nvalid - 1) & 1;
        // what leaves the window in this block: pushed by earlier blocks or carried in, fenced, one load a lane
        float z[kR];
        far_ring_preread(yring, ymask, cy.q, n, lane, z);
        float est[kR];
        fit_stage<false, true>(c, lane, n, xd, den_s, xavg_s, fk, valid, raw, nvalid, lane_last, r_last, yring, ymask, cy, est, z);
        if (__any(cy.refuse)) {
            if (lane == 0) {
                st->guard = 1u;
                atomicAdd(p.handed_over, 1u);
            }
            return;
        }
        *reinterpret_cast<float2 *>(est_row + i0) = make_float2(est[0], est[1]);  // (rows padded to whole blocks)
    }
    far_ring_fence();  // (the epilogue reads the window across the lanes)

    cy.last_k = ti[n_tiles - 1].last_k;
    cy.stat_exact_blocks = (uint32_t)exact_blocks;
    if (p.diff) {  // psk_soft_i::last = the last sample output (cpp/psk_soft.cpp:486-491)
        const float2 l = t_s[p.tile_off + (uint64_t)(n_out - 1)];
        cy.last_re = l.x;
        cy.last_im = l.y;
    }
    if (lane == 0) {  // the back kernel starts from the old one
        ti[0].last0_re = last0_re;
        ti[0].last0_im = last0_im;
    }
    call_epilogue<true>(p, st, yv, fit_cap, yring, ymask, X, ring_dst, lane, cy, kGuardTiled);
}

// ---- a far channel's call that emits nothing: one wave per channel ----
// What psk_fast_kernel<0, 1, false> does for the other channels that emit nothing -- prologue (LinearFit::reset() sums if it ran)
// and epilogue (end-of-call wrap, state commit) around no symbols -- with the window in the channel's row: no LDS holds it.
__global__ __launch_bounds__(64) void psk_far_quiet_kernel(const ChanPlan *__restrict__ plans, const uint32_t *__restrict__ list, uint32_t ch0,
                                                           ChanState *__restrict__ states, float2 *__restrict__ rings, uint32_t ring_cap,
                                                           float *__restrict__ yvs, uint32_t fit_cap, float *__restrict__ far_y,
                                                           uint32_t far_rows)
{
    const int lane = threadIdx.x & 63;
    const uint32_t bi = list[blockIdx.x];
    const ChanPlan &p = plans[bi];
    if (p.mode != PLAN_FAST || p.n_out != 0 || p.far_row >= far_rows)
        return;
    const uint32_t ch = ch0 + bi;
    ChanState *st = &states[ch];
    float2 *ring_base = rings + (size_t)ch * 2u * ring_cap;
    const float2 *ring_src = ring_base + (size_t)p.ring_src * ring_cap;
    float2 *ring_dst = ring_base + (size_t)(p.ring_src ^ 1u) * ring_cap;
    float *yv = yvs + (size_t)ch * fit_cap;
    XView X;
    X.ring = reinterpret_cast<const f2g *>(ring_src);
    X.in = reinterpret_cast<const f2g *>(p.in);
    X.L0 = p.ring_len0;
    float *const yring = far_y + (size_t)p.far_row * kFarRingFloats;
    const uint32_t ymask = kFarRingFloats - 1u;
    FastCarry cy;
    call_prologue<true>(p, st, yv, fit_cap, yring, ymask, lane, cy);
    call_epilogue<true>(p, st, yv, fit_cap, yring, ymask, X, ring_dst, lane, cy, 0u);
}

hipError_t launch_far_quiet(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                            uint32_t ring_cap, float *yvs, uint32_t fit_cap, float *far_y, uint32_t far_rows, hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    if (!far_y || !far_rows)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(psk_far_quiet_kernel, dim3(nch), dim3(kWave), 0, stream, plans, list, ch0, states, rings, ring_cap, yvs, fit_cap, far_y,
                       far_rows);
    return hipGetLastError();
}

size_t far_ring_bytes() { return sizeof(float) * (size_t)kFarRingFloats; }

hipError_t launch_far_fit(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                          uint32_t ring_cap, float *yvs, uint32_t fit_cap, float *far_y, uint32_t far_rows, TileInfo *tiles,
                          const float *t_raw, const float2 *t_s, float *t_est, hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    if (!far_y || !far_rows)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(psk_far_fit_kernel, dim3(nch), dim3(kWave), 0, stream, plans, list, ch0, states, rings, ring_cap, yvs, fit_cap, far_y,
                       far_rows, tiles, t_raw, t_s, t_est);
    return hipGetLastError();
}

}  // namespace psk
