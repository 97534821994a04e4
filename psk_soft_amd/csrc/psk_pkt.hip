// psk_pkt.hip -- packets that are not float2: complex int16 (sc16, PSK_SOFT_FORMAT_CS16), complex int8 (sc8, PSK_SOFT_FORMAT_CS8)
// and complex binary16 (cf16, PSK_SOFT_FORMAT_CF16: interleaved IEEE half I,Q, torch.complex32).  The dispatch of the wave-scan and
// reference-order kernels that read them in place, and the conversion pre-pass for the window classes those do not cover.
//
// numAvg <= 128 and samplesPerBaud 2 .. 16 (the headline's class) have builds of the wave-scan kernel for each of these formats,
// screened and exact tier (psk_fast_inst.hip with PSK_INST_PKT=cs16 | cs8 | cf16: the loads of psk_fast_loop.h convert as they
// read), and of the reference-order kernel that redoes what they hand over (psk_kernels.hip, launch_seq_<format>).  Every other
// such channel -- other window classes, calls of the time-tiled kernels, calls that emit nothing -- first goes through the kernel
// below, which converts its packet into float2 rows of the handle's conversion scratch (psk_capi.cpp: StreamScratch,
// psk_soft_handle::cvt); the plan points at the rows and everything after that is the float path.  The casts int16 -> float and
// int8 -> float and the widening binary16 -> binary32 are exact (subnormal halves become normal floats, never flushed; a quiet NaN
// keeps sign and payload), so such a packet gives bit for bit what the CF32 packet of the converted values gives, either way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_front_src.h"
#include "psk_pkt_cvt.h"
#include "psk_plan.h"
#include "psk_soft_hip.h"

// the formats (name in symbols and files, PSK_SOFT_FORMAT_* id), and the samplesPerBaud of their in-place builds (Makefile PKT_S)
#define PSK_PKT_FORMATS(X) X(cs16, PSK_SOFT_FORMAT_CS16) X(cs8, PSK_SOFT_FORMAT_CS8) X(cf16, PSK_SOFT_FORMAT_CF16)
#define PSK_PKT_S(X, f, id)                                                                                                        \
    X(f, id, 2) X(f, id, 3) X(f, id, 4) X(f, id, 5) X(f, id, 6) X(f, id, 7) X(f, id, 8) X(f, id, 9) X(f, id, 10) X(f, id, 11)      \
    X(f, id, 12) X(f, id, 13) X(f, id, 14) X(f, id, 15) X(f, id, 16)

namespace psk {

#define PSK_PKT_CHECK(f, id) static_assert(PSK_PKT_ID_##f == id, "a build named " #f " reads format " #id " (psk_plan.h)");
PSK_PKT_FORMATS(PSK_PKT_CHECK)
#undef PSK_PKT_CHECK

// grid: x = descriptor (one packet), y = pieces of it; a thread converts four samples an iteration, the loads issued before the
// stores.  Every access is one sample (loads: 4 bytes, CS8 2) or 8 bytes (stores) at consecutive lanes: whole cache lines per wave.
template <int FMT>
__global__ __launch_bounds__(256) void psk_pkt_convert_kernel(const CvtDesc *__restrict__ desc)
{
    const CvtDesc d = desc[blockIdx.x];
    const typename PktWord<FMT>::type *__restrict__ src = reinterpret_cast<const typename PktWord<FMT>::type *>(d.src);
    float2 *__restrict__ dst = reinterpret_cast<float2 *>(d.dst);
    const uint64_t stride = (uint64_t)gridDim.y * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < d.n; i += 4 * stride) {
        const uint32_t a = src[i], b = src[i + stride], c = src[i + 2 * stride], e = src[i + 3 * stride];
        dst[i] = pkt_cvt<FMT>(a);
        dst[i + stride] = pkt_cvt<FMT>(b);
        dst[i + 2 * stride] = pkt_cvt<FMT>(c);
        dst[i + 3 * stride] = pkt_cvt<FMT>(e);
    }
    for (; i < d.n; i += stride) dst[i] = pkt_cvt<FMT>(src[i]);
}

// n_desc descriptors of packets of format fmt in device memory (behind the plans of the call), the longest max_n samples
hipError_t launch_convert(int fmt, const CvtDesc *desc, uint32_t n_desc, uint64_t max_n, hipStream_t stream)
{
    if (!n_desc)
        return hipSuccess;
    // no piece shorter than 1024 samples (a thread's four)
    const uint32_t per = front_grid_y((max_n + 1023u) / 1024u, n_desc);
#define PSK_PKT_CONVERT(f, id) \
    if (fmt == id)             \
        hipLaunchKernelGGL(psk_pkt_convert_kernel<id>, dim3(n_desc, per), dim3(256), 0, stream, desc);
    PSK_PKT_FORMATS(PSK_PKT_CONVERT)
#undef PSK_PKT_CONVERT
    return hipGetLastError();
}

// The wave-scan instantiations that read these packets in place (psk_fast_inst.hip with PSK_INST_PKT, Makefile PKT_FORMATS x PKT_S):
// numAvg <= 128 (one block of window history), samplesPerBaud 2 .. 16, screened and exact tier; and the reference-order kernel of
// each format (psk_kernels.hip with PSK_INST_PKT).  Every other window class takes the pre-pass.
#define PSK_PKT_FAST_ARGS \
    const void *, const uint32_t *, uint32_t, uint32_t, void *, float2 *, uint32_t, float *, uint32_t, uint32_t, uint32_t, hipStream_t
#define PSK_PKT_DECL(f, id, S)                                  \
    hipError_t launch_fast_##f##_S##S##_H1_E0(PSK_PKT_FAST_ARGS); \
    hipError_t launch_fast_##f##_S##S##_H1_E1(PSK_PKT_FAST_ARGS);
#define PSK_PKT_DECL_F(f, id)                                                                                                      \
    PSK_PKT_S(PSK_PKT_DECL, f, id)                                                                                                 \
    hipError_t launch_seq_##f(const void *, const uint32_t *, uint32_t, uint32_t, void *, float2 *, uint32_t, float *, uint32_t, hipStream_t);
PSK_PKT_FORMATS(PSK_PKT_DECL_F)
#undef PSK_PKT_DECL_F
#undef PSK_PKT_DECL

bool fast_pkt_has(int fmt, int S)
{
#define PSK_PKT_HAS(f, id, Sv)  \
    if (fmt == id && S == Sv) \
        return true;
#define PSK_PKT_HAS_F(f, id) PSK_PKT_S(PSK_PKT_HAS, f, id)
    PSK_PKT_FORMATS(PSK_PKT_HAS_F)
#undef PSK_PKT_HAS_F
#undef PSK_PKT_HAS
    return false;
}

hipError_t launch_fast_pkt(int fmt, int S, int exact, const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states,
                           float2 *rings, uint32_t ring_cap, float *yvs, uint32_t fit_cap, uint32_t y_len, uint32_t r_len, hipStream_t stream)
{
#define PSK_PKT_CASE(f, id, Sv)                                                                                                         \
    if (fmt == id && S == Sv)                                                                                                           \
        return exact ? launch_fast_##f##_S##Sv##_H1_E1(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream) \
                     : launch_fast_##f##_S##Sv##_H1_E0(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream);
#define PSK_PKT_CASE_F(f, id) PSK_PKT_S(PSK_PKT_CASE, f, id)
    PSK_PKT_FORMATS(PSK_PKT_CASE_F)
#undef PSK_PKT_CASE_F
#undef PSK_PKT_CASE
    return hipErrorInvalidValue;
}

hipError_t launch_seq_pkt(int fmt, const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                          uint32_t ring_cap, float *yvs, uint32_t fit_cap, hipStream_t stream)
{
#define PSK_PKT_SEQ(f, id) \
    if (fmt == id)         \
        return launch_seq_##f(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, stream);
    PSK_PKT_FORMATS(PSK_PKT_SEQ)
#undef PSK_PKT_SEQ
    return hipErrorInvalidValue;
}

}  // namespace psk
