// psk_fast_inst.hip -- one instantiation of the wave-scan kernel per translation unit:
//   hipcc -DPSK_INST_S=8 -DPSK_INST_H=1 -DPSK_INST_E=0 -c psk_fast_inst.hip -o psk_fast_S8_H1_E0.o
// (S = samplesPerBaud, H = blocks of window history in registers, E = 0 screened / 1 exact timing)
// -DPSK_INST_PKT=cs16 (cs8, cf16): the same instantiation reading complex int16 (complex int8, complex binary16) packets
// (psk_wave.h: pkt_t), exported as launch_fast_cs16_S* (launch_fast_cs8_S*, launch_fast_cf16_S*).  Everything of such a unit lives
// in namespace psk_cs16 (psk_cs8, psk_cf16) -- the kernel keeps its template arguments, and two definitions of
// psk::psk_fast_kernel<8,1,false> in one library would be one symbol.
#define PSK_PASTE_(a, b) a##b
#define PSK_PASTE(a, b) PSK_PASTE_(a, b)
#ifdef PSK_INST_PKT
#include <hip/hip_runtime.h>
#define PSK_PKT_NS PSK_PASTE(psk_, PSK_INST_PKT)
#define psk PSK_PKT_NS
#endif
#include "psk_fast_kernel.h"

#define PSK_CAT_(a, b, c, d, e, f) a##b##c##d##e##f
#define PSK_CAT(a, b, c, d, e, f) PSK_CAT_(a, b, c, d, e, f)

#ifdef PSK_INST_PKT
#undef psk
namespace psk {
// (the plan and state types of the two namespaces are one definition, psk_plan.h, compiled twice)
hipError_t PSK_CAT(PSK_PASTE(PSK_PASTE(launch_fast_, PSK_INST_PKT), _S), PSK_INST_S, _H, PSK_INST_H, _E, PSK_INST_E)(
    const void *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, void *states, float2 *rings, uint32_t ring_cap, float *yvs,
    uint32_t fit_cap, uint32_t y_len, uint32_t r_len, hipStream_t stream)
{
    return PSK_PKT_NS::launch_fast_inst<PSK_INST_S, PSK_INST_H, (PSK_INST_E != 0)>(static_cast<const PSK_PKT_NS::ChanPlan *>(plans), list, ch0,
                                                                                   nch, static_cast<PSK_PKT_NS::ChanState *>(states), rings,
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
