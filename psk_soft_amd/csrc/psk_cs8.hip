// psk_cs8.hip -- complex int8 (sc8, PSK_SOFT_FORMAT_CS8) packets: the dispatch of the wave-scan kernels that read them in
// place, and the conversion pre-pass for the window classes those do not cover.
//
// The same layering as complex int16 (psk_cs16.hip): numAvg <= 128 and samplesPerBaud 2 .. 16 have CS8 builds of the wave-scan
// kernel, screened and exact tier (psk_fast_inst.hip with PSK_INST_CS8=1), and of the reference-order kernel (psk_kernels.hip,
// launch_seq_cs8); every other CS8 channel first goes through the kernel below, which converts its packet into float2 rows of
// the handle's conversion scratch.  The cast int8 -> float is exact, so a CS8 packet gives bit for bit what the CF32 packet of
// the values (float)v gives -- and what the CS16 packet of the same values gives.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_plan.h"

namespace psk {

// grid: x = descriptor (one CS8 packet), y = pieces of it; a thread converts four samples an iteration, the loads issued before
// the stores.  A CS8 packet is only 2-byte aligned (one complex sample), so every load is one sample, 2 bytes, at consecutive
// lanes (128 bytes a wave); the stores are 8 bytes.  CvtDesc::src points at the int8 pairs here (I in the low byte).
__global__ __launch_bounds__(256) void psk_cs8_convert_kernel(const CvtDesc *__restrict__ desc)
{
    const CvtDesc d = desc[blockIdx.x];
    const uint16_t *__restrict__ src = reinterpret_cast<const uint16_t *>(d.src);
    float2 *__restrict__ dst = reinterpret_cast<float2 *>(d.dst);
    const uint64_t stride = (uint64_t)gridDim.y * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x;
    auto cvt = [](uint32_t v) {
        // sign-extended bytes (v_bfe_i32), then v_cvt_f32_i32 -- exact for every int8
        return make_float2((float)(int32_t)(int8_t)(uint8_t)v, (float)(int32_t)(int8_t)(uint8_t)(v >> 8));
    };
    for (; i + 3 * stride < d.n; i += 4 * stride) {
        const uint32_t a = src[i], b = src[i + stride], c = src[i + 2 * stride], e = src[i + 3 * stride];
        dst[i] = cvt(a);
        dst[i + stride] = cvt(b);
        dst[i + 2 * stride] = cvt(c);
        dst[i + 3 * stride] = cvt(e);
    }
    for (; i < d.n; i += stride) dst[i] = cvt(src[i]);
}

// n_desc descriptors in device memory (behind the plans of the call), the longest max_n samples
hipError_t launch_cs8_convert(const CvtDesc *desc, uint32_t n_desc, uint64_t max_n, hipStream_t stream)
{
    if (!n_desc)
        return hipSuccess;
    // about 2048 workgroups in all (eight per CU), no piece shorter than 1024 samples (a thread's four)
    uint64_t per = (max_n + 1023u) / 1024u;
    const uint64_t fill = (2048u + n_desc - 1u) / n_desc;
    per = per < fill ? per : fill;
    per = per < 1u ? 1u : per > 65535u ? 65535u : per;
    hipLaunchKernelGGL(psk_cs8_convert_kernel, dim3(n_desc, (uint32_t)per), dim3(256), 0, stream, desc);
    return hipGetLastError();
}

// The wave-scan instantiations that read CS8 packets in place (psk_fast_inst.hip with PSK_INST_CS8=1, Makefile FAST_CS8_S): numAvg
// <= 128 (one block of window history), samplesPerBaud 2 .. 16, screened and exact tier.  Every other window class takes the pre-pass.
#define PSK_CS8_DECL(S)                                                                                                                \
    hipError_t launch_fast_cs8_S##S##_H1_E0(const void *, const uint32_t *, uint32_t, uint32_t, void *, float2 *, uint32_t, float *,    \
                                             uint32_t, uint32_t, uint32_t, hipStream_t);                                               \
    hipError_t launch_fast_cs8_S##S##_H1_E1(const void *, const uint32_t *, uint32_t, uint32_t, void *, float2 *, uint32_t, float *,    \
                                             uint32_t, uint32_t, uint32_t, hipStream_t);
PSK_CS8_DECL(2) PSK_CS8_DECL(3) PSK_CS8_DECL(4) PSK_CS8_DECL(5) PSK_CS8_DECL(6) PSK_CS8_DECL(7) PSK_CS8_DECL(8) PSK_CS8_DECL(9)
PSK_CS8_DECL(10) PSK_CS8_DECL(11) PSK_CS8_DECL(12) PSK_CS8_DECL(13) PSK_CS8_DECL(14) PSK_CS8_DECL(15) PSK_CS8_DECL(16)
#undef PSK_CS8_DECL

bool fast_cs8_has(int S) { return S >= 2 && S <= 16; }

hipError_t launch_fast_cs8(int S, int exact, const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states,
                           float2 *rings, uint32_t ring_cap, float *yvs, uint32_t fit_cap, uint32_t y_len, uint32_t r_len, hipStream_t stream)
{
#define PSK_CS8_CASE(Sv)                                                                                                               \
    if (S == Sv)                                                                                                                       \
        return exact ? launch_fast_cs8_S##Sv##_H1_E1(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream) \
                     : launch_fast_cs8_S##Sv##_H1_E0(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream);
    PSK_CS8_CASE(2) PSK_CS8_CASE(3) PSK_CS8_CASE(4) PSK_CS8_CASE(5) PSK_CS8_CASE(6) PSK_CS8_CASE(7) PSK_CS8_CASE(8)
    PSK_CS8_CASE(9) PSK_CS8_CASE(10) PSK_CS8_CASE(11) PSK_CS8_CASE(12) PSK_CS8_CASE(13) PSK_CS8_CASE(14) PSK_CS8_CASE(15)
    PSK_CS8_CASE(16)
#undef PSK_CS8_CASE
    return hipErrorInvalidValue;
}

}  // namespace psk
