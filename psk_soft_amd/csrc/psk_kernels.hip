// psk_kernels.hip -- CDNA4 (gfx950) kernels for the psk_soft hot path.
//
// One 64-lane wavefront owns one channel (= one psk_soft_i instance) for the whole call; the
// 4096-channel headline workload is 4096 single-wave workgroups = 16 waves per CU, no
// inter-workgroup communication.
//
//   psk_fast_kernel<S,H,EXACT>  the wave-scan kernel (psk_fast_kernel.h, psk_fast_loop.h): the
//       wave walks the packet in blocks of 128 output symbols, two per lane.
//       timing   (cpp/psk_soft.cpp:445-466, 568-584)  per-phase window energy
//                W_k(i) = W_k(i-1) + e_k(i+A-1) - e_k(i-1) as DPP prefix scans: screened in
//                float with a rigorous margin test (EXACT = 0), or exact in double under the
//                exponent-spread guard (EXACT = 1, runs on the calls the screening refused);
//       phase    (cpp/psk_soft.cpp:474-482, 48-87, 135-174)  M-th power, atan2f, then the
//                feedback unwrap + sliding least-squares fit as two double prefix scans (ySum,
//                xySum with the reference's float-rounded terms, quirk Q4), the unwrap count
//                speculated by consecutive differences and verified / corrected by a
//                fixed-point pass that fixes >= 1 more position per pass;
//       output   (cpp/psk_soft.cpp:484-566)  de-rotation, hard bits, 4 output streams.
//   psk_seq_kernel    the reference-order kernel (this file): lane 0 replays the reference's
//       statement order exactly (any property values, samplesPerBaud == 1, calls longer than
//       2^20 symbols, and every call both wave-scan kernels refused: energy sums that are not exact with an
//       argmax too close to call, an unwrap that does not settle).
//
// Built with -ffp-contract=off (quirk Q9).  No MFMA: the path is a streaming complex-MAC
// with O(1) flop/byte, bound by HBM.
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

// -DPSK_INST_PKT=cs16 (cs8, cf16; Makefile: psk_seq_cs16.o ...): the reference-order kernel alone, reading complex int16 (complex
// int8, complex binary16) packets, in namespace psk_cs16 (psk_cs8, psk_cf16; see psk_fast_inst.hip), exported as launch_seq_cs16
// (launch_seq_cs8, launch_seq_cf16) -- it redoes the calls the wave-scan kernels of that format hand over
#define PSK_PASTE_(a, b) a##b
#define PSK_PASTE(a, b) PSK_PASTE_(a, b)
#ifdef PSK_INST_PKT
#define PSK_PKT_NS PSK_PASTE(psk_, PSK_INST_PKT)
#define psk PSK_PKT_NS
#endif
// -DPSK_SEQ_WIDE=1 (Makefile: psk_seq_wide.o): the reference-order kernel alone for samplesPerBaud > kSeqMaxS, in namespace psk_seqw,
// exported as launch_seq_wide: symbolEnergy[] lives in a row of device memory per channel of the launch (psk_capi.cpp sizes the
// rows by the launch's widest channel), and the loops over it are spread over the wave's lanes -- element k always in lane
// k mod 64, so that no lane reads a sum another lane has written
#if PSK_SEQ_WIDE
#define psk psk_seqw
#endif
#include "psk_fast_kernel.h"

namespace psk {

// ---------------------------------------------------------------------------------
// reference-order kernel
// ---------------------------------------------------------------------------------
struct SeqFit {  // class LinearFit (cpp/psk_soft.h:33-53) on the circular HBM buffer
    float *yv;
    uint32_t cap, head, len, n;
    float xdelta, den, xavg, m, b;
    double ySum, xySum;
    uint32_t count;

    __device__ float at(uint32_t j) const { return yv[(head + j) % cap]; }
    __device__ float calc_fit()
    {
        if (len > 1)
            return fit_value(ySum, xySum, xdelta, len, den, xavg, m, b);
        m = 0.0f;
        b = len ? at(len - 1) : 0.0f;
        return b;
    }
    __device__ float reset_sums()  // cpp/psk_soft.cpp:110-122
    {
        ySum = 0.0;
        xySum = 0.0;
        for (uint32_t j = 0; j < len; j++) {
            float y = at(j);
            ySum += (double)y;
            float jx = (float)j * xdelta;
            float jxy = jx * y;
            xySum += (double)jxy;
        }
        fit_denominator(xdelta, len, den, xavg);
        count = 0;
        return calc_fit();
    }
    __device__ float next(float yval)  // cpp/psk_soft.cpp:48-87
    {
        if (count == kResyncCount)
            reset_sums();
        bool steady = (len == n);
        if (steady) {
            ySum -= (double)at(0);
            head = (head + 1) % cap;
            len--;
            xySum -= (double)xdelta * ySum;
        }
        ySum += (double)yval;
        float t = yval * (float)len;
        t = t * xdelta;
        xySum += (double)t;
        yv[(head + len) % cap] = yval;
        len++;
        if (!steady)
            fit_denominator(xdelta, len, den, xavg);
        count++;
        return calc_fit();
    }
    __device__ float subtract_const(float c)  // cpp/psk_soft.cpp:126-133
    {
        for (uint32_t j = 0; j < len; j++) {
            uint32_t pos = (head + j) % cap;
            yv[pos] = yv[pos] - c;
        }
        return reset_sums();
    }
};

struct SeqEmit {
    const ChanPlan *p;
    SeqFit fit;
    float pe;
    cf32 last;
    uint64_t n_emit;
};

// the per-symbol body, cpp/psk_soft.cpp:471-566, in the reference's statement order
__device__ void seq_emit_symbol(SeqEmit &E, cf32 sample, int sampleIndex, bool have_index)
{
    const ChanPlan &p = *E.p;
    const uint64_t i = E.n_emit++;
    if (have_index && p.sidx)
        p.sidx[i] = (int16_t)(unsigned short)sampleIndex;
    cf32 pw = cpow_uint<true>(sample, p.M);
    double thisPhase = (double)lm_atan2f(pw.im, pw.re);
    long long numWraps = unwrap_count(E.pe, thisPhase);
    thisPhase += (double)numWraps * kTwoPi;
    E.pe = E.fit.next((float)thisPhase);
    if (p.phase)
        p.phase[i] = E.pe;
    float phaseCorrection = 0.0f;
    if (p.diff) {
        cf32 decoded = cdiv<true>(sample, E.last);
        E.last = sample;
        sample = decoded;
    } else {
        phaseCorrection = -E.pe / (float)p.M;
    }
    if (p.M == 4)
        phaseCorrection = (float)((double)phaseCorrection + kPi4);
    float sn, cs;
    lm_sincosf(phaseCorrection, &sn, &cs);
    cf32 ph;
    ph.re = 1.0f * cs;
    ph.im = 1.0f * sn;
    cf32 corr = cmul<true>(sample, ph);
    if (p.soft) {
        p.soft[2 * i] = corr.re;
        p.soft[2 * i + 1] = corr.im;
    }
    if (!p.bits) {
    } else if (p.bpb == 1) {
        p.bits[i] = (int16_t)(corr.re < 0);
    } else if (p.bpb == 2) {
        int b0, b1;
        qpsk_bits(corr.re, corr.im, (p.lf_flags & PLAN_QPSK_SIGN_MAP) != 0, b0, b1);
        p.bits[2 * i] = (int16_t)b0;
        p.bits[2 * i + 1] = (int16_t)b1;
    } else if (p.bpb == 3) {
        unsigned short sym = slice_8psk(corr.re, corr.im);
        for (int j = 0; j != 3; j++) {
            p.bits[3 * i + j] = (int16_t)(sym & 1);
            sym = sym >> 1;
        }
    }
}

__global__ __launch_bounds__(64) void psk_seq_kernel(const ChanPlan *__restrict__ plans, const uint32_t *__restrict__ list, uint32_t ch0,
                                                     ChanState *__restrict__ states, float2 *__restrict__ rings,
                                                     uint32_t ring_cap, float *__restrict__ yvs, uint32_t fit_cap
#if PSK_SEQ_WIDE
                                                     , double *__restrict__ symE_rows, uint32_t symE_stride
#endif
                                                     )
{
#if PSK_SEQ_WIDE
    double *const symE = symE_rows + (size_t)blockIdx.x * symE_stride;
#else
    __shared__ double symE[kSeqMaxS];
#endif
    __shared__ float2 chunk[kSeqChunk];
    __shared__ uint64_t sh_head;
    const int lane = threadIdx.x & 63;
    {
        const uint32_t *hdr = plan_header(plans);
        if (hdr[0] == 0u && hdr[1] == 0u)
            return;  // no channel planned for this kernel, none handed over (psk_plan.h)
    }
    // (list: the channels of one launch set, where the window classes of a batch end their calls on streams of their own --
    // psk_capi.cpp, deferred join --; null: every channel of the batch)
    const uint32_t bi = list ? list[blockIdx.x] : blockIdx.x;
    const ChanPlan &p = plans[bi];
    const uint32_t ch = ch0 + bi;
    ChanState *st = &states[ch];
    const bool redo = (p.mode == PLAN_FAST) && (st->guard == 1u);  // both wave-scan kernels refused
    if (!(p.mode == PLAN_SEQ || p.mode == PLAN_SEQ_S1 || redo))
        return;
    // samplesPerBaud == 1 (a symbol per sample, no timing recovery): planned for this kernel, or handed over by the time-tiled ones
    const bool s1 = p.mode == PLAN_SEQ_S1 || (redo && p.S == 1u);
    float2 *ring_base = rings + (size_t)ch * 2u * ring_cap;
    const float2 *ring_src = ring_base + (size_t)p.ring_src * ring_cap;
    float2 *ring_dst = ring_base + (size_t)(p.ring_src ^ 1u) * ring_cap;
    XView X;
    X.ring = reinterpret_cast<const f2g *>(ring_src);
    X.in = reinterpret_cast<const pkt_t *>(p.in);
    X.L0 = p.ring_len0;
    const uint32_t S = p.S;
    const uint64_t N = p.n_in;
    const uint64_t D = (uint64_t)S * p.A;

    SeqEmit E;
    uint32_t idx = 0, count = p.count0;
    uint64_t head = 0, size = X.L0;
    if (lane == 0) {
        E.p = &p;
        E.fit.yv = yvs + (size_t)ch * fit_cap;
        E.fit.cap = fit_cap;
        E.fit.head = p.lf_head;
        E.fit.len = p.lf_len0;
        E.fit.n = p.lf_n;
        E.fit.xdelta = p.lf_xdelta;
        E.fit.den = st->lf_den;
        E.fit.xavg = st->lf_xavg;
        E.fit.m = st->lf_m;
        E.fit.b = st->lf_b;
        E.fit.ySum = st->lf_ySum;
        E.fit.xySum = st->lf_xySum;
        E.fit.count = p.lf_count0;
        E.pe = st->phaseEstimate;
        E.last.re = st->last_re;
        E.last.im = st->last_im;
        E.n_emit = 0;
        if (p.lf_flags & LF_RECOMPUTE)
            E.fit.reset_sums();
#if !PSK_SEQ_WIDE
        if (!s1) {  // resyncEnergy ran in this call's prologue, :619-636
            for (uint32_t k = 0; k < S; k++) symE[k] = 0.0;
            for (uint64_t j = 0; j < X.L0; j++) {
                const float2 v = x_at(X, j);
                symE[idx] += (double)norm_f(v.x, v.y);
                idx++;
                if (idx == S)
                    idx = 0;
            }
            count = 0;
        }
#endif
    }
#if PSK_SEQ_WIDE
    // resyncEnergy ran in this call's prologue, :619-636: element k sums samples k, k + S, ... in order
    auto resync = [&](uint64_t from, uint64_t n) {
        for (uint32_t k = lane; k < S; k += kWave) {
            double acc = 0.0;
            for (uint64_t j = k; j < n; j += S) {
                const float2 v = x_at(X, from + j);
                acc += (double)norm_f(v.x, v.y);
            }
            symE[k] = acc;
        }
    };
    if (!s1) {
        resync(0, X.L0);
        idx = (uint32_t)(X.L0 % S);
        count = 0;
    }
    for (uint64_t base = 0; base < N; base += kSeqChunk) {
        const uint32_t cnt = (N - base) < (uint64_t)kSeqChunk ? (uint32_t)(N - base) : (uint32_t)kSeqChunk;
        __syncthreads();
        for (uint32_t j = lane; j < cnt; j += kWave) chunk[j] = x_at(X, X.L0 + base + j);
        __syncthreads();
        if (s1) {  // samplesPerBaud == 1, :468-469
            if (lane == 0)
                for (uint32_t jj = 0; jj < cnt; jj++) {
                    cf32 cur;
                    cur.re = chunk[jj].x;
                    cur.im = chunk[jj].y;
                    seq_emit_symbol(E, cur, 0, false);
                }
            continue;
        }
        // the samples up to the next symbol boundary: each adds to its own element, :447-451
        for (uint32_t jj = 0; jj < cnt;) {
            const uint32_t run = S - idx < cnt - jj ? S - idx : cnt - jj;
            for (uint32_t k = idx + ((uint32_t)(lane - (int)idx) & (kWave - 1)); k < idx + run; k += kWave) {
                const float2 v = chunk[jj + (k - idx)];
                symE[k] += (double)norm_f(v.x, v.y);
            }
            size += run;
            jj += run;
            idx += run;
            if (idx < S)
                continue;
            idx = 0;  // :587
            if (size != D)  // :457
                continue;
            // std::max_element with `<` (:462): the running best moves on a strictly larger sum only, so a NaN never wins and
            // holds phase 0 if it stands there -- the first maximum among the sums that are not NaN, else 0
            double bv = 0.0;
            uint32_t bk = 0xFFFFFFFFu;
            for (uint32_t k = lane; k < S; k += kWave) {
                const double v = symE[k];
                if (v == v && (bk == 0xFFFFFFFFu || bv < v))
                    bv = v, bk = k;
            }
            for (int d = 1; d < kWave; d <<= 1) {
                const double ov = __shfl_xor(bv, d);
                const uint32_t ok = (uint32_t)__shfl_xor((int)bk, d);
                if (ok != 0xFFFFFFFFu && (bk == 0xFFFFFFFFu || bv < ov || (ov == bv && ok < bk)))
                    bv = ov, bk = ok;
            }
            const bool nan0 = lane == 0 && !(symE[0] == symE[0]);
            const uint32_t best = (__any(nan0) || bk >= S) ? 0u : bk;
            if (lane == 0) {
                float2 pk = x_at(X, head + best);
                cf32 smp;
                smp.re = pk.x;
                smp.im = pk.y;
                seq_emit_symbol(E, smp, (int)best, true);
            }
            for (uint32_t k = lane; k < S; k += kWave) {  // :572-577
                float2 o = x_at(X, head + k);
                symE[k] -= (double)norm_f(o.x, o.y);
            }
            head += S;  // :579-580
            size -= S;
            count++;
            if (count == kResyncCount) {  // :582-583
                resync(head, size);
                count = 0;
            }
        }
    }
#else
    for (uint64_t base = 0; base < N; base += kSeqChunk) {
        const uint32_t cnt = (N - base) < (uint64_t)kSeqChunk ? (uint32_t)(N - base) : (uint32_t)kSeqChunk;
        __syncthreads();
        for (uint32_t j = lane; j < cnt; j += kWave) chunk[j] = x_at(X, X.L0 + base + j);
        __syncthreads();
        if (lane == 0) {
            for (uint32_t jj = 0; jj < cnt; jj++) {
                float2 v = chunk[jj];
                cf32 cur;
                cur.re = v.x;
                cur.im = v.y;
                if (s1) {  // samplesPerBaud == 1, :468-469
                    seq_emit_symbol(E, cur, 0, false);
                    continue;
                }
                symE[idx] += (double)norm_f(cur.re, cur.im);  // :447-451
                size++;
                if (idx == S - 1) {  // :454
                    if (size == D) {  // :457
                        uint32_t best = 0;
                        for (uint32_t k = 1; k < S; k++)
                            if (symE[best] < symE[k])
                                best = k;
                        float2 pk = x_at(X, head + best);
                        cf32 smp;
                        smp.re = pk.x;
                        smp.im = pk.y;
                        seq_emit_symbol(E, smp, (int)best, true);
                        for (uint32_t k = 0; k < S; k++) {  // :572-577
                            float2 o = x_at(X, head + k);
                            symE[k] -= (double)norm_f(o.x, o.y);
                        }
                        head += S;  // :579-580
                        size -= S;
                        count++;
                        if (count == kResyncCount) {  // :582-583
                            for (uint32_t k = 0; k < S; k++) symE[k] = 0.0;
                            uint32_t ix = 0;
                            for (uint64_t j = 0; j < size; j++) {
                                float2 o = x_at(X, head + j);
                                symE[ix] += (double)norm_f(o.x, o.y);
                                ix++;
                                if (ix == S)
                                    ix = 0;
                            }
                            count = 0;
                        }
                    }
                    idx = 0;  // :587
                } else {
                    idx++;  // :590
                }
            }
        }
    }
#endif
    if (lane == 0) {
        // end-of-call wrap, cpp/psk_soft.cpp:592-603
        const float wrapValue = (float)(kTwoPi * (double)p.M);
        if (!(p.lf_flags & PLAN_NO_WRAP) && wrap_test(E.pe, wrapValue)) {
            float qv = E.pe / wrapValue;
            long long numWraps = to_long_x86(__builtin_round((double)qv));
            E.pe = E.fit.subtract_const((float)numWraps * wrapValue);
        }
        st->lf_ySum = E.fit.ySum;
        st->lf_xySum = E.fit.xySum;
        st->last_re = E.last.re;
        st->last_im = E.last.im;
        st->phaseEstimate = E.pe;
        st->lf_den = E.fit.den;
        st->lf_xavg = E.fit.xavg;
        st->lf_m = E.fit.m;
        st->lf_b = E.fit.b;
        st->stat_blocks = 0;
        st->stat_extra = 0;
        st->stat_exact = 0;
        st->stat_chain = 0;
        st->guard = redo ? 2u : 0u;  // 2 = "the guard sent this call here" (statistics)
        st->pad_state = 0x7F800000u;  // (the largest window sum is not tracked here: a piece that continues this call assumes the worst)
        sh_head = head;
    }
    __syncthreads();
    if (!s1) {
        const uint64_t h = sh_head;
        for (uint32_t j = lane; j < p.ring_len1; j += kWave) ring_dst[j] = x_at(X, h + j);
    }
}

}  // namespace psk

#if !defined(PSK_INST_PKT) && !PSK_SEQ_WIDE
// ---------------------------------------------------------------------------------
// launchers (called from psk_capi.cpp through plain C++ declarations).  Every (samplesPerBaud,
// history depth, screened / exact) instantiation of the wave-scan kernel is its own translation
// unit (psk_fast_inst.hip): co-compiled template instantiations perturb each other's register
// allocation on gfx950.
// ---------------------------------------------------------------------------------
namespace psk {
#define PSK_DECL(S, H, E) hipError_t launch_fast_S##S##_H##H##_E##E(PSK_FAST_ARGS);
#define PSK_DECL_SH(S, H) PSK_DECL(S, H, 0) PSK_DECL(S, H, 1)
// (numAvg <= 128: the screened kernel settles near-ties itself; its exact-timing sibling takes the calls with
// non-finite samples or a non-finite / astronomically large phase estimate in the channel state)
#define PSK_DECL_S(S) PSK_DECL_SH(S, 1) PSK_DECL_SH(S, 2) PSK_DECL_SH(S, 4)
// (H = 0: the screened tier without window history in registers, psk_fast_loop.h REREAD -- the launches of the numAvg 513 ... 1024 class)
PSK_DECL(2, 0, 0) PSK_DECL(3, 0, 0) PSK_DECL(4, 0, 0) PSK_DECL(5, 0, 0) PSK_DECL(6, 0, 0) PSK_DECL(7, 0, 0) PSK_DECL(8, 0, 0) PSK_DECL(9, 0, 0)
PSK_DECL(10, 0, 0) PSK_DECL(11, 0, 0) PSK_DECL(12, 0, 0) PSK_DECL(13, 0, 0) PSK_DECL(14, 0, 0) PSK_DECL(15, 0, 0) PSK_DECL(16, 0, 0)
PSK_DECL_S(2)
PSK_DECL_S(3)
PSK_DECL_S(4)
PSK_DECL_S(5)
PSK_DECL_S(6)
PSK_DECL_S(7)
PSK_DECL_S(8)
PSK_DECL_S(9)
PSK_DECL_S(10)
PSK_DECL_S(11)
PSK_DECL_S(12)
PSK_DECL_S(13)
PSK_DECL_S(14)
PSK_DECL_S(15)
PSK_DECL_S(16)
PSK_DECL_SH(2, 8)
PSK_DECL_SH(3, 8)
PSK_DECL_SH(4, 8)
PSK_DECL_SH(5, 8)
PSK_DECL_SH(6, 8)
PSK_DECL_SH(7, 8)
PSK_DECL_SH(8, 8)
PSK_DECL_SH(9, 8)
PSK_DECL_SH(10, 8)
PSK_DECL_SH(11, 8)
PSK_DECL_SH(12, 8)
PSK_DECL_SH(13, 8)
PSK_DECL_SH(14, 8)
PSK_DECL_SH(15, 8)
PSK_DECL_SH(16, 8)
#define PSK_DECL_S_WIDE(S) PSK_DECL_SH(S, 1) PSK_DECL_SH(S, 2) PSK_DECL_SH(S, 4)
PSK_DECL_S_WIDE(17)
PSK_DECL_S_WIDE(18)
PSK_DECL_S_WIDE(19)
PSK_DECL_S_WIDE(20)
PSK_DECL_S_WIDE(21)
PSK_DECL_S_WIDE(22)
PSK_DECL_S_WIDE(23)
PSK_DECL_S_WIDE(24)
PSK_DECL_S_WIDE(25)
PSK_DECL_S_WIDE(26)
PSK_DECL_S_WIDE(27)
PSK_DECL_S_WIDE(28)
PSK_DECL_S_WIDE(29)
PSK_DECL_S_WIDE(30)
PSK_DECL_S_WIDE(31)
PSK_DECL_S_WIDE(32)

// `list` = the nch indices into the batch (plans[], states[ch0 + .]) this launch covers, one workgroup each.
// S = 0: the channels that emit nothing this call.  Otherwise S in {2,3,4,5,6,7,8,10,12,16}, H in {1,2,4}
// blocks of window history, exact = 0 (screened timing) / 1 (exact timing, runs on refused calls).
hipError_t launch_fast(int S, int H, int exact, PSK_FAST_ARGS)
{
    if (S == 0)
        return launch_fast_inst<0, 1, false>(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream);
    {
        // Windows of 513 ... 1024 symbols: eight blocks of history in registers are 430 ... 480 VGPRs, one wave to a SIMD; the variant
        // that reads the symbols leaving the window a second time instead (H == 0) keeps four -- twice the loads, and still a
        // quarter faster at every batch size measured (4096 channels, numAvg 600: 6.37 -> 4.80 ms; 2048: 3.24 -> 2.16; 256: 1.72
        // -> 1.55).  For the shorter windows (two / four blocks, two waves to a SIMD) the registers win.  PSK_SOFT_REREAD
        // (environment): 0 never, 1 the eight-block class (default), 2 every window longer than a block.
        static const int reread = [] { const char *e = getenv("PSK_SOFT_REREAD"); return e ? atoi(e) : 1; }();
        if (!exact && S >= 2 && S <= 16 && ((reread >= 1 && H == 8) || (reread >= 2 && H > 1))) {
#define PSK_CASE0(Sv) \
    if (S == Sv)      \
        return launch_fast_S##Sv##_H0_E0(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream);
            PSK_CASE0(2) PSK_CASE0(3) PSK_CASE0(4) PSK_CASE0(5) PSK_CASE0(6) PSK_CASE0(7) PSK_CASE0(8) PSK_CASE0(9) PSK_CASE0(10)
            PSK_CASE0(11) PSK_CASE0(12) PSK_CASE0(13) PSK_CASE0(14) PSK_CASE0(15) PSK_CASE0(16)
#undef PSK_CASE0
        }
    }
#define PSK_CASE(Sv, Hv)                                                                                              \
    if (S == Sv && H == Hv)                                                                                           \
        return exact ? launch_fast_S##Sv##_H##Hv##_E1(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream) \
                     : launch_fast_S##Sv##_H##Hv##_E0(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream);
#define PSK_CASE1(Sv)                                                                                                 \
    if (S == Sv && H == 1)                                                                                            \
        return exact ? hipSuccess                                                                                     \
                     : launch_fast_S##Sv##_H1_E0(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream);
#define PSK_CASE_S(Sv) PSK_CASE(Sv, 1) PSK_CASE(Sv, 2) PSK_CASE(Sv, 4)
    PSK_CASE_S(2)
    PSK_CASE_S(3)
    PSK_CASE_S(4)
    PSK_CASE_S(5)
    PSK_CASE_S(6)
    PSK_CASE_S(7)
    PSK_CASE_S(8)
    PSK_CASE_S(9)
    PSK_CASE_S(10)
    PSK_CASE_S(11)
    PSK_CASE_S(12)
    PSK_CASE_S(13)
    PSK_CASE_S(14)
    PSK_CASE_S(15)
    PSK_CASE_S(16)
    PSK_CASE(2, 8)
    PSK_CASE(3, 8)
    PSK_CASE(4, 8)
    PSK_CASE(5, 8)
    PSK_CASE(6, 8)
    PSK_CASE(7, 8)
    PSK_CASE(8, 8)
    PSK_CASE(9, 8)
    PSK_CASE(10, 8)
    PSK_CASE(11, 8)
    PSK_CASE(12, 8)
    PSK_CASE(13, 8)
    PSK_CASE(14, 8)
    PSK_CASE(15, 8)
    PSK_CASE(16, 8)
#define PSK_CASE_S_WIDE(Sv) PSK_CASE(Sv, 1) PSK_CASE(Sv, 2) PSK_CASE(Sv, 4)
    PSK_CASE_S_WIDE(17)
    PSK_CASE_S_WIDE(18)
    PSK_CASE_S_WIDE(19)
    PSK_CASE_S_WIDE(20)
    PSK_CASE_S_WIDE(21)
    PSK_CASE_S_WIDE(22)
    PSK_CASE_S_WIDE(23)
    PSK_CASE_S_WIDE(24)
    PSK_CASE_S_WIDE(25)
    PSK_CASE_S_WIDE(26)
    PSK_CASE_S_WIDE(27)
    PSK_CASE_S_WIDE(28)
    PSK_CASE_S_WIDE(29)
    PSK_CASE_S_WIDE(30)
    PSK_CASE_S_WIDE(31)
    PSK_CASE_S_WIDE(32)
    return hipErrorInvalidValue;
}
#else
namespace psk {
#endif

#if PSK_SEQ_WIDE
// (symE: a row of symE_stride doubles for each of the nch channels of the list)
hipError_t launch_seq(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                      uint32_t ring_cap, float *yvs, uint32_t fit_cap, double *symE, uint32_t symE_stride, hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    hipLaunchKernelGGL(psk_seq_kernel, dim3(nch), dim3(kWave), 0, stream, plans, list, ch0, states, rings, ring_cap, yvs,
                       fit_cap, symE, symE_stride);
    return hipGetLastError();
}
#else
hipError_t launch_seq(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                      uint32_t ring_cap, float *yvs, uint32_t fit_cap, hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    hipLaunchKernelGGL(psk_seq_kernel, dim3(nch), dim3(kWave), 0, stream, plans, list, ch0, states, rings, ring_cap, yvs,
                       fit_cap);
    return hipGetLastError();
}
#endif
// Measurement support: the empirical read ceiling -- 16-byte loads over a
// buffer, summed, nothing written (the sum only reaches memory if it is NaN-free and equals a value
// it cannot have).  4 independent loads per thread in flight, grid-stride, 2048 workgroups of 256.
__global__ __launch_bounds__(256) void psk_read_probe_kernel(const float4 *__restrict__ src, uint64_t n_vec,
                                                             float *__restrict__ sink)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (; i + 3 * stride < n_vec; i += 4 * stride) {
        const float4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        acc.x += a.x + b.x + c.x + d.x;
        acc.y += a.y + b.y + c.y + d.y;
        acc.z += a.z + b.z + c.z + d.z;
        acc.w += a.w + b.w + c.w + d.w;
    }
    for (; i < n_vec; i += stride) {
        const float4 a = src[i];
        acc.x += a.x, acc.y += a.y, acc.z += a.z, acc.w += a.w;
    }
    const float t = acc.x + acc.y + acc.z + acc.w;
    if (t == 1.2345678e-30f)
        *sink = t;
}

hipError_t launch_read_probe(const void *src, uint64_t bytes, float *sink, hipStream_t stream)
{
    hipLaunchKernelGGL(psk_read_probe_kernel, dim3(2048), dim3(256), 0, stream, (const float4 *)src, bytes / 16u, sink);
    return hipGetLastError();
}
}  // namespace psk
#ifdef PSK_INST_PKT
#undef psk
namespace psk {
hipError_t PSK_PASTE(launch_seq_, PSK_INST_PKT)(const void *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, void *states, float2 *rings,
                                                uint32_t ring_cap, float *yvs, uint32_t fit_cap, hipStream_t stream)
{
    return PSK_PKT_NS::launch_seq(static_cast<const PSK_PKT_NS::ChanPlan *>(plans), list, ch0, nch, static_cast<PSK_PKT_NS::ChanState *>(states),
                                  rings, ring_cap, yvs, fit_cap, stream);
}
}  // namespace psk
#endif
#if PSK_SEQ_WIDE
#undef psk
namespace psk {
hipError_t launch_seq_wide(const void *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, void *states, float2 *rings,
                           uint32_t ring_cap, float *yvs, uint32_t fit_cap, double *symE, uint32_t symE_stride, hipStream_t stream)
{
    return psk_seqw::launch_seq(static_cast<const psk_seqw::ChanPlan *>(plans), list, ch0, nch, static_cast<psk_seqw::ChanState *>(states),
                                rings, ring_cap, yvs, fit_cap, symE, symE_stride, stream);
}
}  // namespace psk
#endif
