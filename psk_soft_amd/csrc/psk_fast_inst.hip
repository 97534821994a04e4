// psk_fast_inst.hip -- one instantiation of the wave-scan kernel per translation unit:
//   hipcc -DPSK_INST_S=8 -DPSK_INST_H=1 -DPSK_INST_E=0 -c psk_fast_inst.hip -o psk_fast_S8_H1_E0.o
// (S = samplesPerBaud, H = blocks of window history in registers, E = 0 screened / 1 exact timing)
// -DPSK_INST_CS16=1: the same instantiation reading complex int16 packets (psk_wave.h: pkt_t), exported as launch_fast_cs16_S*.
// Everything of such a unit lives in namespace psk_cs16 -- the kernel keeps its template arguments, and two definitions of
// psk::psk_fast_kernel<8,1,false> in one library would be one symbol.
// -DPSK_INST_CS8=1: the same for complex int8 packets, in namespace psk_cs8, exported as launch_fast_cs8_S*.
// -DPSK_INST_CF16=1: the same for complex binary16 packets, in namespace psk_cf16, exported as launch_fast_cf16_S*.
#if PSK_INST_CS16
#include <hip/hip_runtime.h>
#define psk psk_cs16
#elif PSK_INST_CS8
#include <hip/hip_runtime.h>
#define psk psk_cs8
#elif PSK_INST_CF16
#include <hip/hip_runtime.h>
#define psk psk_cf16
#endif
#include "psk_fast_kernel.h"

#define PSK_CAT_(a, b, c, d, e, f) a##b##c##d##e##f
#define PSK_CAT(a, b, c, d, e, f) PSK_CAT_(a, b, c, d, e, f)

#if PSK_INST_CS16
#undef psk
namespace psk {
// (the plan and state types of the two namespaces are one definition, psk_plan.h, compiled twice)
hipError_t PSK_CAT(launch_fast_cs16_S, PSK_INST_S, _H, PSK_INST_H, _E, PSK_INST_E)(const void *plans, const uint32_t *list, uint32_t ch0,
                                                                                   uint32_t nch, void *states, float2 *rings, uint32_t ring_cap,
                                                                                   float *yvs, uint32_t fit_cap, uint32_t y_len, uint32_t r_len,
                                                                                   hipStream_t stream)
{
    return psk_cs16::launch_fast_inst<PSK_INST_S, PSK_INST_H, (PSK_INST_E != 0)>(static_cast<const psk_cs16::ChanPlan *>(plans), list, ch0,
                                                                                 nch, static_cast<psk_cs16::ChanState *>(states), rings,
                                                                                 ring_cap, yvs, fit_cap, y_len, r_len, stream);
}
}  // namespace psk
#elif PSK_INST_CS8
#undef psk
namespace psk {
hipError_t PSK_CAT(launch_fast_cs8_S, PSK_INST_S, _H, PSK_INST_H, _E, PSK_INST_E)(const void *plans, const uint32_t *list, uint32_t ch0,
                                                                                  uint32_t nch, void *states, float2 *rings, uint32_t ring_cap,
                                                                                  float *yvs, uint32_t fit_cap, uint32_t y_len, uint32_t r_len,
                                                                                  hipStream_t stream)
{
    return psk_cs8::launch_fast_inst<PSK_INST_S, PSK_INST_H, (PSK_INST_E != 0)>(static_cast<const psk_cs8::ChanPlan *>(plans), list, ch0,
                                                                                nch, static_cast<psk_cs8::ChanState *>(states), rings,
                                                                                ring_cap, yvs, fit_cap, y_len, r_len, stream);
}
}  // namespace psk
#elif PSK_INST_CF16
#undef psk
namespace psk {
hipError_t PSK_CAT(launch_fast_cf16_S, PSK_INST_S, _H, PSK_INST_H, _E, PSK_INST_E)(const void *plans, const uint32_t *list, uint32_t ch0,
                                                                                   uint32_t nch, void *states, float2 *rings, uint32_t ring_cap,
                                                                                   float *yvs, uint32_t fit_cap, uint32_t y_len, uint32_t r_len,
                                                                                   hipStream_t stream)
{
    return psk_cf16::launch_fast_inst<PSK_INST_S, PSK_INST_H, (PSK_INST_E != 0)>(static_cast<const psk_cf16::ChanPlan *>(plans), list, ch0,
                                                                                 nch, static_cast<psk_cf16::ChanState *>(states), rings,
                                                                                 ring_cap, yvs, fit_cap, y_len, r_len, stream);
}
}  // namespace psk
#else
namespace psk {
hipError_t PSK_CAT(launch_fast_S, PSK_INST_S, _H, PSK_INST_H, _E, PSK_INST_E)(PSK_FAST_ARGS)
{
    return launch_fast_inst<PSK_INST_S, PSK_INST_H, (PSK_INST_E != 0)>(plans, list, ch0, nch, states, rings, ring_cap, yvs,
                                                                       fit_cap, y_len, r_len, stream);
}
}  // namespace psk
#endif
