// psk_tune.hip -- the tune pre-pass of psk_soft_process_device_tuned: every tuned packet of a call, whatever its format and
// stride, read once, shifted in frequency (psk_tune.h: tune_rotate) and written as float2 rows of the handle's gather scratch;
// the ordinary call then runs on the rows as on CF32 packets.  One launch per call.
//
// A workgroup first copies the two phasor tables (16 KiB) from device memory into LDS, then walks one piece of one packet: per
// sample one conversion (psk_pkt_cvt.h), two 8-byte LDS reads, a complex product of the two table entries and one with the
// sample -- no sinf / cosf on the device.  The phase word of a lane's first sample costs one 64-bit multiply per piece, every
// further one a 64-bit add.  Plain vector loads and stores only; the source is never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_front_src.h"
#include "psk_libm.h"
#include "psk_soft_hip.h"
#include "psk_tune.h"

namespace psk {

constexpr uint32_t kTuneThreads = 256;
// No piece shorter than this many samples (but the packet's last): the 16 KiB of tables a workgroup copies, from the L2 after
// the first few, stay under a fifth of the 96 KiB and more that the piece itself moves.  A multiple of 2 * kTuneThreads: every
// piece starts on an even sample, so the 16-byte stores of the contiguous path are aligned.
constexpr uint64_t kTuneMinPiece = 8192;

// samples [i0, i1) of the packet of d; i0 is a multiple of 2 * kTuneThreads
template <int FMT>
__device__ inline void tune_piece(const TuneDesc &d, const float *tab, uint64_t i0, uint64_t i1)
{
    const PSK_GLOBAL void *__restrict__ src = (const PSK_GLOBAL void *)d.src;
    PSK_GLOBAL f2 *__restrict__ dst = (PSK_GLOBAL f2 *)d.dst;
    const uint64_t step = d.step;
    if (d.stride == 1) {
        // a lane takes two adjacent samples: 16 bytes a store.  Two such pairs an iteration, the loads issued before the stores.
        uint64_t i = i0 + 2u * threadIdx.x;
        uint64_t p = d.phase + i * step;
        const uint64_t adv = step * (2u * kTuneThreads);
        for (; i + 2u * kTuneThreads + 1u < i1; i += 4u * kTuneThreads, p += 2u * adv) {
            const f2 a = src_load<FMT>(src, i), b = src_load<FMT>(src, i + 1u);
            const f2 c = src_load<FMT>(src, i + 2u * kTuneThreads), e = src_load<FMT>(src, i + 2u * kTuneThreads + 1u);
            const f2 ya = src_rotate(tab, p, a), yb = src_rotate(tab, p + step, b);
            const f2 yc = src_rotate(tab, p + adv, c), ye = src_rotate(tab, p + adv + step, e);
            *reinterpret_cast<PSK_GLOBAL f4 *>(dst + i) = f4{ya.x, ya.y, yb.x, yb.y};
            *reinterpret_cast<PSK_GLOBAL f4 *>(dst + i + 2u * kTuneThreads) = f4{yc.x, yc.y, ye.x, ye.y};
        }
        for (; i < i1; i += 2u * kTuneThreads, p += adv) {
            const f2 ya = src_rotate(tab, p, src_load<FMT>(src, i));
            if (i + 1u < i1) {
                const f2 yb = src_rotate(tab, p + step, src_load<FMT>(src, i + 1u));
                *reinterpret_cast<PSK_GLOBAL f4 *>(dst + i) = f4{ya.x, ya.y, yb.x, yb.y};
            } else {
                dst[i] = ya;
            }
        }
    } else {
        // a column of a frame-major matrix read where it lies, one lane one sample: every load a memory line of its own
        uint64_t i = i0 + threadIdx.x;
        uint64_t p = d.phase + i * step;
        const uint64_t adv = step * kTuneThreads;
        for (; i + kTuneThreads < i1; i += 2u * kTuneThreads, p += 2u * adv) {
            const f2 a = src_load<FMT>(src, i * d.stride), b = src_load<FMT>(src, (i + kTuneThreads) * d.stride);
            dst[i] = src_rotate(tab, p, a);
            dst[i + kTuneThreads] = src_rotate(tab, p + adv, b);
        }
        for (; i < i1; i += kTuneThreads, p += adv) dst[i] = src_rotate(tab, p, src_load<FMT>(src, i * d.stride));
    }
}

// grid: x = descriptor (one packet), y = pieces of it, `piece` samples each (a multiple of 2 * kTuneThreads)
__global__ __launch_bounds__(kTuneThreads) void psk_tune_kernel(const TuneDesc *__restrict__ desc, const float *__restrict__ d_tab, uint64_t piece)
{
    __shared__ __attribute__((aligned(16))) float tab[kTuneTableFloats];
    const TuneDesc d = desc[blockIdx.x];
    const uint64_t i0 = (uint64_t)blockIdx.y * piece;
    if (i0 >= d.n)
        return;  // (the whole workgroup: nothing of this packet is left for it)
    const uint64_t i1 = d.n - i0 < piece ? d.n : i0 + piece;
    src_tables_to_lds<kTuneThreads>(tab, d_tab);
    __syncthreads();
    src_dispatch(d.format, [&](auto fmt) { tune_piece<decltype(fmt)::value>(d, tab, i0, i1); });
}

hipError_t launch_tune(const TuneDesc *desc, uint32_t n_desc, uint64_t max_n, const float *d_tab, hipStream_t stream)
{
    if (!n_desc || !max_n)
        return hipSuccess;
    // no piece shorter than kTuneMinPiece
    const uint64_t per = front_grid_y((max_n + kTuneMinPiece - 1u) / kTuneMinPiece, n_desc);
    const uint64_t unit = 2u * kTuneThreads;
    const uint64_t piece = ((max_n + per - 1u) / per + unit - 1u) / unit * unit;
    hipLaunchKernelGGL(psk_tune_kernel, dim3(n_desc, (uint32_t)per), dim3(kTuneThreads), 0, stream, desc, d_tab, piece);
    return hipGetLastError();
}

// C[h] = (cosf(a), sinf(a)), a = (float)(h * pi / 512); F[l] likewise with pi / 2^19: glibc 2.35's sinf / cosf (lm_sincosf)
const float *tune_tables()
{
    static const float *const tab = [] {
        float *t = new float[kTuneTableFloats];
        for (uint32_t k = 0; k < kTuneTable; k++) {
            const float a = (float)((double)k * 0x1.921fb54442d18p-8), b = (float)((double)k * 0x1.921fb54442d18p-18);
            lm_sincosf(a, &t[2u * k + 1u], &t[2u * k]);
            lm_sincosf(b, &t[2u * (kTuneTable + k) + 1u], &t[2u * (kTuneTable + k)]);
        }
        return t;
    }();
    return tab;
}

}  // namespace psk
