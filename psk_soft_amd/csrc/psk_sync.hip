// psk_sync.hip -- psk_soft_sync_device: a known word slid along the soft symbols of every channel, one psk_soft_sync_t per channel.
//
// The record holds the windows whose normalised correlation with the word reaches the threshold, and the best window
// (include/psk_soft_hip.h, "where frames start"); the host turns a hit into a rotation (psk_soft_sync_derive).  One pass over the
// rows, two kernels:
//
//   fold   grid (workgroups per channel, channels), one workgroup of 256 lanes per piece of kSyncPiece windows of one channel; the
//          pieces of a channel go round its workgroups.  The workgroup stages the piece's symbols and the L - 1 behind them --
//          the channel's history slot supplying the positions in front of the row -- as float2 in LDS, their energies te next
//          to them (one value per symbol, the same for every window that meets it) and the word.  Wave v owns the windows
//          [256 v, 256 v + 256) of the piece, 64 at a time: consecutive lanes take consecutive windows, so a step j of the sum
//          reads the symbols with unit-stride 8-byte LDS reads (no bank conflict) and the word point as a broadcast.  Every
//          window is summed on its own, j = 0 .. L-1 -- not with a sliding energy sum, which would make a value depend on where
//          its piece began.  Hits are compacted in position order: a ballot and a prefix count per wave and turn into the
//          wave's list in LDS, then the four lists in wave order.  The best of a lane (first maximum: a later window must be
//          greater), of a wave (a xor tree on (m, position): the smaller position wins a tie), of the waves in order.  One
//          partial per piece.  The workgroup that takes piece 0 also writes the history behind the row, 127 symbols, into the
//          channel's other slot.
//   join   one wave per channel: the partials in piece order, 64 at a time -- counts added, a prefix count of the hits that
//          places the first 16, the best by the same rule --, the record put together in LDS and stored by all lanes; the zero
//          record for a channel that is not searched.
//
// Which lane sums which window depends on the window's index in the row only -- not on the batch, the grid or the stream --, and
// a window's value on no other window: the same symbols give the same bytes.  No atomics.  The arithmetic (psk_sync.h) is rounded
// once per operation (the unit is built with -ffp-contract=off), denormals kept, the division correctly rounded.  Plain vector
// loads and stores only; the rows and the words are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_front_src.h"
#include "psk_sync.h"

namespace psk {

namespace {

constexpr uint32_t kWaves = kSyncThreads / 64u;
constexpr uint32_t kWaveRun = kSyncPiece / kWaves;  // windows of a piece one wave owns
constexpr uint32_t kTurns = kWaveRun / 64u;

struct Best {
    bool has;
    float m, cr, ci, e;
    int64_t pos;
};

// a is replaced by b where b is the better of the two: the greater m, the smaller position on a tie
__device__ __forceinline__ void best_take(Best &a, const Best &b)
{
    if (b.has && (!a.has || b.m > a.m || (b.m == a.m && b.pos < a.pos)))
        a = b;
}

__device__ __forceinline__ Best best_wave(Best a)
{
    for (int off = 32; off >= 1; off >>= 1) {
        Best b;
        b.has = __shfl_xor((int)a.has, off) != 0;
        b.m = __shfl_xor(a.m, off), b.cr = __shfl_xor(a.cr, off), b.ci = __shfl_xor(a.ci, off), b.e = __shfl_xor(a.e, off);
        b.pos = (int64_t)__shfl_xor((long long)a.pos, off);
        best_take(a, b);
    }
    return a;
}

__device__ __forceinline__ psk_soft_sync_hit_t best_hit(const Best &b)
{
    psk_soft_sync_hit_t h;
    h.pos = b.pos, h.cr = b.cr, h.ci = b.ci, h.e = b.e, h.m = b.m;
    return h;
}

// a hit to and from global memory, member by member (plain vector stores and loads)
__device__ __forceinline__ void hit_store(PSK_GLOBAL psk_soft_sync_hit_t *to, const psk_soft_sync_hit_t &h)
{
    to->pos = h.pos, to->cr = h.cr, to->ci = h.ci, to->e = h.e, to->m = h.m;
}
__device__ __forceinline__ psk_soft_sync_hit_t hit_load(const PSK_GLOBAL psk_soft_sync_hit_t *from)
{
    psk_soft_sync_hit_t h;
    h.pos = from->pos, h.cr = from->cr, h.ci = from->ci, h.e = from->e, h.m = from->m;
    return h;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask, uint32_t lane)
{
    return (uint32_t)__builtin_popcountll(mask & (((uint64_t)1 << lane) - 1u));
}

// symbol g of the joined sequence (history in front, g < 0; the row, 0 <= g < n)
__device__ __forceinline__ f2 sync_symbol(const SyncDesc &d, int64_t g)
{
    if (g >= 0)
        return ((const PSK_GLOBAL f2 *)d.soft)[g];
    if (d.flags & kSyncRestart)
        return f2{0.0f, 0.0f};
    return ((const PSK_GLOBAL f2 *)d.hist_in)[g + (int64_t)kSyncHist];  // (g >= -(L - 1) >= -127)
}

}  // namespace

__global__ __launch_bounds__(kSyncThreads) void psk_sync_fold_kernel(const SyncDesc *__restrict__ desc, uint32_t nch,
                                                                     SyncPartial *__restrict__ part)
{
    __shared__ f2 sx[kSyncStage + 1u];
    __shared__ float se[kSyncStage + 1u];
    __shared__ f2 sw[kSyncMaxWord];
    __shared__ psk_soft_sync_hit_t w_hits[kWaves][kSyncHits];
    __shared__ psk_soft_sync_hit_t w_best[kWaves];
    __shared__ uint32_t w_nv[kWaves], w_nh[kWaves], w_has[kWaves];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t c = blockIdx.y; c < nch; c += gridDim.y) {
        const SyncDesc d = desc[c];
        // (uniform for the workgroup, like every branch on the descriptor below)
        if (!(d.flags & kSyncData) || blockIdx.x >= d.n_piece || !d.L || d.L > kSyncMaxWord)
            continue;
        const uint32_t L = d.L;
        __syncthreads();  // (the LDS of the channel before is read out)
        if (t < L)
            sw[t] = ((const PSK_GLOBAL f2 *)d.word)[t];
        for (uint32_t p = blockIdx.x; p < d.n_piece; p += gridDim.x) {
            const uint32_t w_lo = p * kSyncPiece;  // (n_piece = max(1, ceil(n_windows / kSyncPiece)): w_lo <= n_windows)
            const uint32_t cnt = d.n_windows - w_lo < kSyncPiece ? d.n_windows - w_lo : kSyncPiece;
            const int64_t p_lo = d.p0 + (int64_t)w_lo;
            // entry k becomes x[p_lo + k]; the last one, k = cnt + L - 2, is x[p_lo + cnt - 1 + L - 1] with p_lo + cnt - 1 <= n - L
            const uint32_t n_stage = cnt ? cnt + L - 1u : 0u;
            for (uint32_t k = t; k < n_stage; k += kSyncThreads) {
                const f2 x = sync_symbol(d, p_lo + (int64_t)k);
                sx[k] = x;
                se[k] = sy_energy(x.x, x.y);
            }
            __syncthreads();
            uint32_t nv = 0, nh = 0;  // (the wave's: the same in all its lanes)
            Best mine;
            mine.has = false, mine.m = mine.cr = mine.ci = mine.e = 0.0f, mine.pos = 0;
            for (uint32_t turn = 0; turn < kTurns; turn++) {
                const uint32_t w0 = wave * kWaveRun + turn * 64u;
                if (w0 >= cnt)
                    break;  // (the wave's bound)
                const uint32_t wi = w0 + lane;  // (< kSyncPiece: the reads below stay inside sx and se, live or not)
                const bool live = wi < cnt;
                float cr = 0.0f, ci = 0.0f, e = 0.0f;
                {
                    const f2 x = sx[wi], w = sw[0];
                    sy_step(true, x.x, x.y, se[wi], w.x, w.y, &cr, &ci, &e);
                }
#pragma unroll 4
                for (uint32_t j = 1; j < L; j++) {
                    const f2 x = sx[wi + j], w = sw[j];
                    sy_step(false, x.x, x.y, se[wi + j], w.x, w.y, &cr, &ci, &e);
                }
                float m;
                const bool valid = sy_metric(cr, ci, e, d.Ew, &m) && live;
                const bool hit = valid && m >= d.threshold;
                const int64_t pos = p_lo + (int64_t)wi;
                const uint64_t hm = __builtin_amdgcn_ballot_w64(hit);
                nv += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid));
                const uint32_t at = nh + lanes_below(hm, lane);
                if (hit && at < kSyncHits) {
                    psk_soft_sync_hit_t h;
                    h.pos = pos, h.cr = cr, h.ci = ci, h.e = e, h.m = m;
                    w_hits[wave][at] = h;
                }
                nh += (uint32_t)__builtin_popcountll(hm);
                if (valid && (!mine.has || m > mine.m)) {
                    mine.has = true;
                    mine.m = m, mine.cr = cr, mine.ci = ci, mine.e = e, mine.pos = pos;
                }
            }
            const Best wb = best_wave(mine);
            if (lane == 0) {
                w_nv[wave] = nv, w_nh[wave] = nh, w_has[wave] = wb.has ? 1u : 0u;
                w_best[wave] = best_hit(wb);
            }
            __syncthreads();
            PSK_GLOBAL SyncPartial *const out = (PSK_GLOBAL SyncPartial *)part + (d.part0 + p);
            if (t < kWaves * kSyncHits) {
                // the lists in wave order: entry k of wave v goes behind all hits of the waves in front of it
                const uint32_t v = t / kSyncHits, k = t % kSyncHits;
                uint32_t base = 0;
                for (uint32_t u = 0; u < v; u++) base += w_nh[u];
                if (k < w_nh[v] && base + k < kSyncHits)
                    hit_store(&out->hits[base + k], w_hits[v][k]);
            } else if (t == 64u) {
                uint32_t sv = 0, sh = 0, pick = kWaves;
                for (uint32_t v = 0; v < kWaves; v++) {
                    sv += w_nv[v], sh += w_nh[v];
                    // (the waves' windows ascend with the wave: a later wave must be greater)
                    if (w_has[v] && (pick == kWaves || w_best[v].m > w_best[pick].m))
                        pick = v;
                }
                out->n_valid = sv, out->n_hits = sh;
                if (pick != kWaves)
                    hit_store(&out->best, w_best[pick]);
            }
            __syncthreads();  // (the next piece overwrites the LDS)
        }
        // the history behind the row: the last 127 of (history in front || x[0 .. n-1]), whose indices are n - 127 .. n - 1
        if (blockIdx.x == 0 && t < kSyncHist)
            ((PSK_GLOBAL f2 *)d.hist_out)[t] = sync_symbol(d, (int64_t)d.n - (int64_t)kSyncHist + (int64_t)t);
    }
}

__global__ __launch_bounds__(64) void psk_sync_join_kernel(const SyncDesc *__restrict__ desc, uint32_t nch,
                                                           const SyncPartial *__restrict__ part, psk_soft_sync_t *__restrict__ records)
{
    __shared__ psk_soft_sync_t rec;
    constexpr uint32_t kWords = sizeof(psk_soft_sync_t) / 4u;
    static_assert(sizeof(psk_soft_sync_t) % 4u == 0, "the record is stored as 32-bit words");
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const SyncDesc d = desc[c];
        const bool data = (d.flags & kSyncData) != 0;
        __syncthreads();  // (the record of the channel before is stored)
        for (uint32_t k = lane; k < kWords; k += 64u) reinterpret_cast<uint32_t *>(&rec)[k] = 0u;
        __syncthreads();
        uint64_t nv = 0, nh = 0;  // (the wave's)
        Best best;
        best.has = false, best.m = best.cr = best.ci = best.e = 0.0f, best.pos = 0;
        for (uint32_t base = 0; data && base < d.n_piece; base += 64u) {
            const uint32_t k = base + lane;
            const bool live = k < d.n_piece;
            const PSK_GLOBAL SyncPartial *const p = (const PSK_GLOBAL SyncPartial *)part + (d.part0 + (live ? k : 0u));
            const uint32_t pv = live ? p->n_valid : 0u, ph = live ? p->n_hits : 0u;
            // hits in front of this lane's piece: the earlier chunks', and an inclusive scan over the lanes less its own
            uint32_t scan = ph;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)scan, off);
                if ((int)lane >= off)
                    scan += up;
            }
            const uint64_t before = nh + (scan - ph);
            if (ph && before < kSyncHits) {
                const uint32_t room = kSyncHits - (uint32_t)before, take = ph < room ? ph : room;  // (ph above 16: 16 were stored)
                for (uint32_t j = 0; j < take; j++) rec.hits[before + j] = hit_load(&p->hits[j]);
            }
            Best b;
            b.has = pv != 0u;
            b.m = b.cr = b.ci = b.e = 0.0f, b.pos = 0;
            if (b.has) {
                const psk_soft_sync_hit_t h = hit_load(&p->best);
                b.m = h.m, b.cr = h.cr, b.ci = h.ci, b.e = h.e, b.pos = h.pos;
            }
            // (the positions ascend with the piece, so the smaller position is the earlier piece, in this chunk and across chunks)
            best_take(best, best_wave(b));
            // the chunk's totals, the same in every lane (a piece has 1024 windows: 64 of them fit 32 bits)
            uint32_t cv = pv, ch = ph;
            for (int off = 32; off >= 1; off >>= 1) cv += (uint32_t)__shfl_xor((int)cv, off), ch += (uint32_t)__shfl_xor((int)ch, off);
            nv += cv, nh += ch;
        }
        if (data && lane == 0) {
            rec.n_symbols = d.n, rec.n_windows = d.n_windows;
            rec.n_valid = nv, rec.n_hits = nh;
            if (best.has)
                rec.best = best_hit(best);
            rec.word_len = d.L, rec.flags = PSK_SOFT_SYNC_DATA;
        }
        __syncthreads();
        PSK_GLOBAL uint32_t *const out = (PSK_GLOBAL uint32_t *)(records + d.channel);
        for (uint32_t k = lane; k < kWords; k += 64u) out[k] = reinterpret_cast<const uint32_t *>(&rec)[k];
    }
}

hipError_t launch_sync_fold(const SyncDesc *desc, uint32_t nch, uint32_t max_piece, SyncPartial *part, hipStream_t stream)
{
    if (!nch || !max_piece)
        return hipSuccess;
    // the shared grid rule for the workgroups of a channel; more than 65535 channels take a second trip of the channel loop
    const dim3 grid(front_grid_y(max_piece, nch), nch < 65535u ? nch : 65535u);
    hipLaunchKernelGGL(psk_sync_fold_kernel, grid, dim3(kSyncThreads), 0, stream, desc, nch, part);
    return hipGetLastError();
}

hipError_t launch_sync_join(const SyncDesc *desc, uint32_t nch, const SyncPartial *part, psk_soft_sync_t *records, hipStream_t stream)
{
    if (!nch)
        return hipSuccess;
    hipLaunchKernelGGL(psk_sync_join_kernel, dim3(nch < 65535u ? nch : 65535u), dim3(64), 0, stream, desc, nch, part, records);
    return hipGetLastError();
}

}  // namespace psk
