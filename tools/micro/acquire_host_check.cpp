// acquire_host_check.cpp -- a stand-alone caller of psk_soft_acquire_host and psk_soft_acquire_derive for the host sanitizers
// (tools/acquire_host_sanitize.sh): lengths around the lag window, tuned and untuned, non-finite and out-of-range samples,
// hand-made records.  Prints one line per case; exits non-zero when a result is implausible.  No GPU is touched.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "psk_soft_hip.h"

static int bad = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            bad++;                                                  \
        }                                                           \
    } while (0)

int main()
{
    const double f = 0.011, two_pi = 6.283185307179586;
    const uint64_t lengths[] = {0, 1, 2, 3, 127, 128, 129, 130, 1000, 4097};
    for (uint16_t M : {2, 4, 8}) {
        for (uint64_t n : lengths) {
            std::vector<float> x(2 * n);
            for (uint64_t k = 0; k < n; k++) {
                const double a = two_pi * (f * (double)k + (double)(k / 4 % M) / M);
                x[2 * k] = (float)std::cos(a), x[2 * k + 1] = (float)std::sin(a);
            }
            for (int variant = 0; variant < 4; variant++) {
                std::vector<float> y = x;
                if (variant == 1 && n > 2)
                    y[n] = std::numeric_limits<float>::infinity(), y[3] = std::numeric_limits<float>::quiet_NaN();
                if (variant == 2)
                    for (float &v : y) v *= 1e-24f;
                if (variant == 3)
                    for (float &v : y) v *= 3e19f;
                const psk_soft_tune_t tune = {0x0123456789abcdefull, psk_soft_tune_step(-0.004)};
                for (const psk_soft_tune_t *t : {(const psk_soft_tune_t *)nullptr, &tune}) {
                    psk_soft_acquire_t rec;
                    CHECK(psk_soft_acquire_host(M, t, y.data(), n, &rec) == PSK_SOFT_OK);
                    psk_soft_acquire_derived_t d;
                    CHECK(psk_soft_acquire_derive(&rec, &d) == PSK_SOFT_OK);
                    CHECK(rec.n_samples == n && rec.n_valid <= n);
                    if (variant >= 2)
                        CHECK(rec.n_valid == 0 && d.lags_used == 0 && std::isnan(d.offset_cycles_per_sample));
                    if (variant == 0 && n >= 1000)
                        CHECK(d.lags_used == 8 && std::fabs(d.offset_cycles_per_sample - (t ? f - 0.004 : f)) < 1e-5);
                    std::printf("M %u n %llu variant %d tuned %d: valid %llu lags %d offset %.9f coherence %.6f\n", (unsigned)M,
                                (unsigned long long)n, variant, t != nullptr, (unsigned long long)rec.n_valid, d.lags_used,
                                d.offset_cycles_per_sample, d.coherence);
                }
            }
        }
    }
    // hand-made records: nothing to derive from, and a lag without pairs
    psk_soft_acquire_t r = {};
    psk_soft_acquire_derived_t d;
    CHECK(psk_soft_acquire_derive(&r, &d) == PSK_SOFT_OK && d.lags_used == 0 && std::isnan(d.coherence));
    r.flags = PSK_SOFT_A_DATA, r.constelationSize = 4, r.n_valid = 10, r.sum_e = 10.0;
    for (int j = 0; j < 8; j++) r.n_pairs[j] = 9, r.sum_re[j] = 9.0;
    r.n_pairs[3] = 0;
    CHECK(psk_soft_acquire_derive(&r, &d) == PSK_SOFT_OK && d.lags_used == 3 && d.offset_cycles_per_sample == 0.0 && d.mean_energy == 1.0);
    CHECK(psk_soft_acquire_derive(nullptr, &d) == PSK_SOFT_ERR_INVALID_ARG);
    CHECK(psk_soft_acquire_host(3, nullptr, nullptr, 0, &r) == PSK_SOFT_ERR_INVALID_ARG);
    CHECK(psk_soft_acquire_bytes() == sizeof(psk_soft_acquire_t) && sizeof(psk_soft_acquire_t) == 224);
    std::printf("%s\n", bad ? "acquire_host_check: FAILED" : "acquire_host_check: ok");
    return bad ? 1 : 0;
}
