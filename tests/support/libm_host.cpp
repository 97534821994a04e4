// libm_host.cpp -- the PRODUCT header psk_soft_amd/csrc/psk_libm.h compiled for the host as a small shared library with
// array entries (tests/dev_prim_cases.py builds and loads it): the directed case sets go through the host build of every
// form, which tests/test_dev_prim_cases.py holds to glibc, and lm_slice8_fast's `near` flag of this build is what the
// device's flag is held to (tests/test_gpu_dev_prims.py).  Same flags as tests/test_libm_pin.py.
#include <stdint.h>

#include "psk_libm.h"

extern "C" {
void lmh_atan2f(const float *y, const float *x, float *r, long n)
{
    for (long i = 0; i < n; i++) r[i] = psk::lm_atan2f(y[i], x[i]);
}
void lmh_atanf(const float *x, float *r, long n)
{
    for (long i = 0; i < n; i++) r[i] = psk::lm_atanf(x[i]);
}
// the straight-line form with its non-finite companion, as atan2f_wave composes them; special[i] = *special
void lmh_atan2f_ordinary(const float *y, const float *x, float *r, int32_t *special, long n)
{
    for (long i = 0; i < n; i++) {
        bool sp;
        float v = psk::lm_atan2f_ordinary(y[i], x[i], &sp);
        if (sp)
            v = psk::lm_atan2f_nonfinite(y[i], x[i]);
        r[i] = v;
        special[i] = sp;
    }
}
void lmh_sincosf(const float *t, float *s, float *c, long n)
{
    for (long i = 0; i < n; i++) psk::lm_sincosf(t[i], &s[i], &c[i]);
}
void lmh_sincosf_ordinary(const float *t, float *s, float *c, long n)
{
    for (long i = 0; i < n; i++) {
        bool sp;
        psk::lm_sincosf_ordinary(t[i], &s[i], &c[i], &sp);
    }
}
void lmh_slice8_fast(const float *re, const float *im, int32_t *sector, int32_t *near, long n)
{
    for (long i = 0; i < n; i++) {
        bool nb;
        sector[i] = (int32_t)psk::lm_slice8_fast(re[i], im[i], &nb);
        near[i] = nb;
    }
}
void lmh_div_known(const double *a, const double *b, const double *rb, double *q, long n)
{
    for (long i = 0; i < n; i++) q[i] = psk::lm_div_known(a[i], b[i], rb[i]);
}
}
