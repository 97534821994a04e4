// psk_pkt_cvt.h -- one sample of a packet that is not float2, as it lies in memory, and its float2: shared by the conversion
// pre-pass (psk_pkt.hip) and the tune pre-pass (psk_tune.hip).
#ifndef PSK_PKT_CVT_H
#define PSK_PKT_CVT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_soft_hip.h"

namespace psk {

// one sample as it lies in a packet of format FMT -- a 32-bit word, I in the low half; for CS8 a 16-bit word, I in the low byte
// (a CS8 packet is only 2-byte aligned, one complex sample) -- and its float2
template <int FMT>
struct PktWord {
    typedef uint32_t type;
};
template <>
struct PktWord<PSK_SOFT_FORMAT_CS8> {
    typedef uint16_t type;
};
template <int FMT>
__device__ inline float2 pkt_cvt(uint32_t v);
// sign-extended halves: v_bfe_i32 / v_ashrrev_i32, then v_cvt_f32_i32 -- exact for every int16
template <>
__device__ inline float2 pkt_cvt<PSK_SOFT_FORMAT_CS16>(uint32_t v)
{
    return make_float2((float)(int32_t)(int16_t)(v & 0xffffu), (float)((int32_t)v >> 16));
}
// sign-extended bytes (v_bfe_i32), then v_cvt_f32_i32 -- exact for every int8
template <>
__device__ inline float2 pkt_cvt<PSK_SOFT_FORMAT_CS8>(uint32_t v)
{
    return make_float2((float)(int32_t)(int8_t)(uint8_t)v, (float)(int32_t)(int8_t)(uint8_t)(v >> 8));
}
// v_cvt_f32_f16 of either half (psk_wave.h: cf16_f2 is the same two conversions)
template <>
__device__ inline float2 pkt_cvt<PSK_SOFT_FORMAT_CF16>(uint32_t v)
{
    return make_float2((float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xffffu)), (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)));
}

}  // namespace psk
#endif
