// psk_tune.h -- the tune pre-pass of psk_soft_process_device_tuned (psk_tune.hip, psk_capi.cpp): the per-packet frequency shift
// of include/psk_soft_hip.h ("Tuned packets"), its tables and its descriptors.
//
// Sample k of a tuned packet is converted to float as its format defines and multiplied by the phasor W(p_k) of the phase word
// p_k = phase + k * step (turns x 2^64, mod 2^64).  W comes from two tables of 1024 entries, a coarse one indexed by the top ten
// bits of p_k and a fine one by the next ten; the product of the two entries and the product with the sample are plain float32
// operations, each rounded once, none fused.  tune_rotate() (psk_front_src.h) IS that definition: psk_soft_tune_apply (host) and
// the kernels (device) all call it, on the same tables, which the host builds once per process with lm_sincosf (glibc 2.35's
// sinf / cosf, psk_libm.h) and uploads once per handle.
#ifndef PSK_TUNE_H
#define PSK_TUNE_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "psk_front_src.h"

namespace psk {

// One tuned packet: n complex samples of `format`, `stride` samples apart at src, become n float2 at dst; flags stays 0.
typedef FrontIo TuneDesc;

// the tables, built at the first call (host memory, kTuneTableFloats floats, valid for the life of the process)
const float *tune_tables();

// descriptors and tables (`d_tab`: the upload of tune_tables()) in device memory; max_n = the longest packet of the launch
hipError_t launch_tune(const TuneDesc *desc, uint32_t n_desc, uint64_t max_n, const float *d_tab, hipStream_t stream);

}  // namespace psk
#endif
