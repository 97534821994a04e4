// psk_cf16.hip -- complex binary16 (cf16, PSK_SOFT_FORMAT_CF16: interleaved IEEE half I,Q, torch.complex32) packets: the dispatch
// of the wave-scan kernels that read them in place, and the conversion pre-pass for the window classes those do not cover.
//
// The same layering as complex int16 (psk_cs16.hip), whose geometry a CF16 packet shares -- one 32-bit word per sample, 4-byte
// aligned: numAvg <= 128 and samplesPerBaud 2 .. 16 have CF16 builds of the wave-scan kernel, screened and exact tier
// (psk_fast_inst.hip with PSK_INST_CF16=1), and of the reference-order kernel (psk_kernels.hip, launch_seq_cf16); every other CF16
// channel first goes through the kernel below, which widens its packet into float2 rows of the handle's conversion scratch.  The
// widening binary16 -> binary32 is exact (subnormal halves become normal floats, never flushed; a quiet NaN keeps sign and
// payload), so a CF16 packet gives bit for bit what the CF32 packet of the widened values gives, either way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_plan.h"

namespace psk {

// grid: x = descriptor (one CF16 packet), y = pieces of it; a thread widens four samples an iteration, the loads issued
// before the stores.  Every access is 4 bytes (loads) or 8 (stores) at consecutive lanes: whole cache lines per wave.
__global__ __launch_bounds__(256) void psk_cf16_convert_kernel(const CvtDesc *__restrict__ desc)
{
    const CvtDesc d = desc[blockIdx.x];
    const uint32_t *__restrict__ src = d.src;
    float2 *__restrict__ dst = reinterpret_cast<float2 *>(d.dst);
    const uint64_t stride = (uint64_t)gridDim.y * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x;
    auto cvt = [](uint32_t v) {
        // v_cvt_f32_f16 of either half (psk_wave.h: cf16_f2 is the same two conversions)
        return make_float2((float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xffffu)), (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)));
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
hipError_t launch_cf16_convert(const CvtDesc *desc, uint32_t n_desc, uint64_t max_n, hipStream_t stream)
{
    if (!n_desc)
        return hipSuccess;
    // about 2048 workgroups in all (eight per CU), no piece shorter than 1024 samples (a thread's four)
    uint64_t per = (max_n + 1023u) / 1024u;
    const uint64_t fill = (2048u + n_desc - 1u) / n_desc;
    per = per < fill ? per : fill;
    per = per < 1u ? 1u : per > 65535u ? 65535u : per;
    hipLaunchKernelGGL(psk_cf16_convert_kernel, dim3(n_desc, (uint32_t)per), dim3(256), 0, stream, desc);
    return hipGetLastError();
}

// The wave-scan instantiations that read CF16 packets in place (psk_fast_inst.hip with PSK_INST_CF16=1, Makefile FAST_CF16_S): numAvg
// <= 128 (one block of window history), samplesPerBaud 2 .. 16, screened and exact tier.  Every other window class takes the pre-pass.
#define PSK_CF16_DECL(S)                                                                                                               \
    hipError_t launch_fast_cf16_S##S##_H1_E0(const void *, const uint32_t *, uint32_t, uint32_t, void *, float2 *, uint32_t, float *,   \
                                              uint32_t, uint32_t, uint32_t, hipStream_t);                                              \
    hipError_t launch_fast_cf16_S##S##_H1_E1(const void *, const uint32_t *, uint32_t, uint32_t, void *, float2 *, uint32_t, float *,   \
                                              uint32_t, uint32_t, uint32_t, hipStream_t);
PSK_CF16_DECL(2) PSK_CF16_DECL(3) PSK_CF16_DECL(4) PSK_CF16_DECL(5) PSK_CF16_DECL(6) PSK_CF16_DECL(7) PSK_CF16_DECL(8) PSK_CF16_DECL(9)
PSK_CF16_DECL(10) PSK_CF16_DECL(11) PSK_CF16_DECL(12) PSK_CF16_DECL(13) PSK_CF16_DECL(14) PSK_CF16_DECL(15) PSK_CF16_DECL(16)
#undef PSK_CF16_DECL

bool fast_cf16_has(int S) { return S >= 2 && S <= 16; }

hipError_t launch_fast_cf16(int S, int exact, const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states,
                            float2 *rings, uint32_t ring_cap, float *yvs, uint32_t fit_cap, uint32_t y_len, uint32_t r_len, hipStream_t stream)
{
#define PSK_CF16_CASE(Sv)                                                                                                              \
    if (S == Sv)                                                                                                                       \
        return exact ? launch_fast_cf16_S##Sv##_H1_E1(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream) \
                     : launch_fast_cf16_S##Sv##_H1_E0(plans, list, ch0, nch, states, rings, ring_cap, yvs, fit_cap, y_len, r_len, stream);
    PSK_CF16_CASE(2) PSK_CF16_CASE(3) PSK_CF16_CASE(4) PSK_CF16_CASE(5) PSK_CF16_CASE(6) PSK_CF16_CASE(7) PSK_CF16_CASE(8)
    PSK_CF16_CASE(9) PSK_CF16_CASE(10) PSK_CF16_CASE(11) PSK_CF16_CASE(12) PSK_CF16_CASE(13) PSK_CF16_CASE(14) PSK_CF16_CASE(15)
    PSK_CF16_CASE(16)
#undef PSK_CF16_CASE
    return hipErrorInvalidValue;
}

}  // namespace psk
