// symrate_host_check.cpp -- a stand-alone caller of psk_soft_symrate_host and psk_soft_symrate_derive for the host sanitizers
// (tools/symrate_host_sanitize.sh): block lengths at both ends of the range, lengths around two blocks, the lag window and the
// cap, tuned and untuned, non-finite and out-of-range samples, hand-made records.  Prints one line per case; exits non-zero when
// a result is implausible.  No GPU is touched.
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
    const double two_pi = 6.283185307179586, pi = 3.141592653589793;
    for (uint16_t S : {4, 5, 8, 33, 1024}) {
        const double sps = 1.04 * S;
        const uint64_t blocks[] = {0, 1, 2, 3, 127, 128, 129, 130, 1000, 4097};
        for (uint64_t b : blocks) {
            if (S == 1024 && b > 130)
                continue;
            for (uint64_t extra : {(uint64_t)0, (uint64_t)S - 1}) {
                const uint64_t n = b * S + extra;
                std::vector<float> x(2 * n);
                for (uint64_t k = 0; k < n; k++) {
                    const double u = (double)k / sps, f = u - std::floor(u);
                    const double amp = 0.2 + 0.8 * std::sin(pi * f), a = two_pi * (0.003 * (double)k + (double)((uint64_t)u * 7 % 4) / 4.0);
                    x[2 * k] = (float)(amp * std::cos(a)), x[2 * k + 1] = (float)(amp * std::sin(a));
                }
                for (int variant = 0; variant < 3; variant++) {
                    std::vector<float> y = x;
                    if (variant == 1 && n > 2)
                        y[n] = std::numeric_limits<float>::infinity(), y[3] = std::numeric_limits<float>::quiet_NaN();
                    if (variant == 2)
                        for (float &v : y) v *= 3e19f;
                    const psk_soft_tune_t tune = {0x0123456789abcdefull, psk_soft_tune_step(-0.004)};
                    for (const psk_soft_tune_t *t : {(const psk_soft_tune_t *)nullptr, &tune}) {
                        psk_soft_symrate_t rec;
                        CHECK(psk_soft_symrate_host(S, t, y.data(), n, &rec) == PSK_SOFT_OK);
                        psk_soft_symrate_derived_t d;
                        CHECK(psk_soft_symrate_derive(&rec, &d) == PSK_SOFT_OK);
                        const uint64_t nb = n / S < 2 ? 0 : n / S > 4096 ? 4096 : n / S;
                        CHECK(rec.n_blocks == nb && rec.n_used == nb * S && rec.n_valid <= nb && rec.n_samples == (nb ? n : 0));
                        if (variant == 2)
                            CHECK(rec.n_valid == 0 && d.lags_used == 0 && std::isnan(d.samples_per_symbol) && d.detector == -1);
                        if (variant == 0 && b >= 1000)
                            CHECK(d.lags_used == 8 && d.detector == 0 && std::fabs(d.samples_per_symbol / sps - 1.0) < 5e-4);
                        std::printf("S %u n %llu variant %d tuned %d: blocks %llu valid %llu lags %d detector %d sps %.6f coherence %.6f\n", (unsigned)S,
                                    (unsigned long long)n, variant, t != nullptr, (unsigned long long)rec.n_blocks,
                                    (unsigned long long)rec.n_valid, d.lags_used, d.detector, d.samples_per_symbol, d.coherence);
                    }
                }
            }
        }
    }
    // hand-made records: nothing to derive from, a lag with fewer than 8 pairs, the tie
    psk_soft_symrate_t r = {};
    psk_soft_symrate_derived_t d;
    CHECK(psk_soft_symrate_derive(&r, &d) == PSK_SOFT_OK && d.lags_used == 0 && std::isnan(d.coherence) && d.detector == -1);
    r.flags = PSK_SOFT_SR_DATA, r.samplesPerBaud = 8, r.n_blocks = r.n_valid = 10, r.n_used = r.n_samples = 80;
    for (int z = 0; z < 2; z++) {
        r.sum_pow[z] = 10.0, r.sum_lvl[z] = 80.0;
        for (int j = 0; j < 8; j++) r.sum_re[z][j] = 9.0;
    }
    for (int j = 0; j < 8; j++) r.n_pairs[j] = 9;
    r.n_pairs[3] = 7;
    CHECK(psk_soft_symrate_derive(&r, &d) == PSK_SOFT_OK && d.lags_used == 3 && d.detector == 0 && d.samples_per_symbol == 8.0 && d.step_ratio == 1.0 &&
          d.mean_level == 1.0);
    CHECK(psk_soft_symrate_derive(nullptr, &d) == PSK_SOFT_ERR_INVALID_ARG);
    CHECK(psk_soft_symrate_host(3, nullptr, nullptr, 0, &r) == PSK_SOFT_ERR_INVALID_ARG);
    CHECK(psk_soft_symrate_host(1025, nullptr, nullptr, 0, &r) == PSK_SOFT_ERR_INVALID_ARG);
    CHECK(psk_soft_symrate_bytes() == sizeof(psk_soft_symrate_t) && sizeof(psk_soft_symrate_t) == 392);
    std::printf("%s\n", bad ? "symrate_host_check: FAILED" : "symrate_host_check: ok");
    return bad ? 1 : 0;
}
