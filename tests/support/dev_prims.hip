// dev_prims.hip -- TEST SUPPORT: every device-math and wave primitive of the product headers (psk_libm.h,
// psk_device_math.h, psk_wave.h, psk_wave_scan_gen.h, and the first-maximum reductions of psk_tile_any.h) behind an elementwise kernel of its own, so that tests can hold
// each of them, run on the device by itself, to the oracle bit for bit (tests/test_gpu_dev_prims.py).
//
// The headers are included unchanged and this file is compiled with the product's flags (psk_soft_amd/csrc/Makefile,
// target ../libpsk_dev_prims.so); it is not linked into the product library.  Blocks are 64 threads: one wave per 64
// consecutive cases.  Results leave through plain per-lane stores.
//
// One C entry:  int psk_dev_prims_run(int op, const void *const *in, void *const *out, long long n)
//   op = id | param << 8 | PSK_DP_DIVERGENT   (ids, parameters and the arrays of each: the table in run() below and
//   tests/dev_prims_lib.py); n = number of cases, a multiple of 64; in[k] / out[k] are host arrays.  It allocates, copies,
//   launches, synchronises, copies back and returns the HIP error code (hipErrorInvalidValue for a bad op or n).
// With PSK_DP_DIVERGENT the primitive runs inside a lane-divergent branch, twice: first with the lanes of LANE_MASK_A
// active, then in a second launch with the others; either way only some of lanes 0-29 are active.  The forms that read the
// range table from lanes (AtanTabDev) need every lane active and are refused in that mode; so are the reductions of
// psk_tile_any.h, which the front stages call with the whole wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psk_wave.h"
#include "psk_tile_any.h"

using namespace psk;

namespace {

enum {
    OP_ATAN2 = 1,      // param: 0 AtanTabDev, 1 AtanTabWave      in y, x (f32)                 out f32
    OP_SINCOS = 2,     // param: 0 dep = 0, 1 dep loop-varying    in t (f32)                    out sin, cos (f32)
    OP_SLICE8_FAST = 3,  //                                       in re, im (f32)               out sector, near (u32)
    OP_SLICE8 = 4,     // param: table form                       in re, im (f32)               out u32
    OP_SLICE8_ATAN = 5,  // param: table form                     in re, im (f32)               out u32
    OP_DIV_KNOWN = 6,  // param: 0 rb given, 1 rb = 1.0 / b on the device   in a, b, rb (f64)   out f64
    OP_NORM = 7,       //                                         in re, im (f32)               out f32
    OP_CMUL = 8,       // param: RECOVER                          in a, b, c, d (f32)           out re, im (f32)
    OP_CPOW = 9,       // param: M | RECOVER << 8                 in re, im (f32)               out re, im (f32)
    OP_CDIV = 10,      // (RECOVER)                               in a, b, c, d (f32)           out re, im (f32)
    OP_TO_LONG = 11,   // param: dep form                         in v (f64)                    out i64
    OP_UNWRAP = 12,    // param: dep form                         in phaseEstimate (f32), thisPhase (f64)   out i64
    OP_FIT_DEN = 13,   //                                         in xdelta (f32), pts (u32)    out denominator, xAvg (f32)
    OP_FIT_VALUE = 14,  //                                        in ySum, xySum (f64), xdelta (f32), pts (u32)   out fit, m, b (f32)
    OP_FIT_KNOWN = 15,  // (xdelta, pts uniform over a wave)      in the same                   out fit, m (f32)
    OP_QPSK = 16,      // param: sign map                         in re, im (f32)               out b0, b1 (i32)
    OP_WRAP_TEST = 17,  //                                        in phaseEstimate, wrapValue (f32)   out u32
    OP_SCAN_F64 = 18,  //                                         in f64                        out f64
    OP_SUM_F64 = 19,   //                                         in f64                        out f64 (every lane: the sum)
    OP_SCAN_I32 = 20,  //                                         in i32                        out i32
    OP_SCAN_F32_MULTI = 21,  // param: N = 1 .. 32                in f32 [n][N]                 out f32 [n][N]
    OP_MAX_F32 = 22,   //                                         in f32 (>= 0)                 out f32 (every lane)
    OP_MAX_U32 = 23,   //                                         in u32                        out u32
    OP_MIN_U32 = 24,   //                                         in u32                        out u32
    OP_UP1 = 25,       // param: 0 int, 1 float, 2 double         in v, carry                   out (lane 0: its own carry)
    OP_UP1_ZERO = 26,  // param: type                             in v                          out
    OP_READ_LANE = 27,  // param: 1 float, 2 double               in v, lane (i32, the wave's first counts)   out
    OP_MED3 = 28,      //                                         in a, b, c (i32)              out i32
    OP_ANY_MERGE = 29,  //                 in a.best, a.second, b.best, b.second (f64), a.k, b.k (i32)   out best, second (f64), k (i32)
    OP_ANY_MAX_F64 = 30,  //                                      in f64                        out f64 (every lane)
    OP_ANY_MIN_U32 = 31,  //                                      in u32                        out u32 (every lane)
    OP_ANY_MAX_F64_MULTI = 32,  // param: U = 8                   in f64 [n][U]                 out f64 [n][U]
    OP_ANY_MIN_U32_MULTI = 33,  // param: U = 8                   in u32 [n][U]                 out u32 [n][U]
    OP_COUNT
};
constexpr int PSK_DP_DIVERGENT = 1 << 30;
constexpr uint64_t LANE_MASK_A = 0x9249A4D2B5A56A95ull;  // 30 lanes, 16 of them among lanes 0-29

constexpr int MAX_IN = 6, MAX_OUT = 3;
struct Args {
    const void *in[MAX_IN];
    void *out[MAX_OUT];
    int loop;  // 1, known at run time only: the trip count of the loop that makes `dep` loop-varying
};

template <class T>
__device__ __forceinline__ T ld(const Args &a, int k, long long i)
{
    return static_cast<const T *>(a.in[k])[i];
}
template <class T>
__device__ __forceinline__ void st(const Args &a, int k, long long i, T v)
{
    static_cast<T *>(a.out[k])[i] = v;
}

template <int TAB>
struct TabOf;
template <>
struct TabOf<0> {
    static __device__ __forceinline__ AtanTabDev make(int lane) { return atan_tab_dev(lane); }
};
template <>
struct TabOf<1> {
    static __device__ __forceinline__ AtanTabWave make(int) { return AtanTabWave(); }
};

// ---- one functor per operation and form: run(args, case index, lane) ----
template <int TAB>
struct Atan2 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int lane)
    {
        const auto tab = TabOf<TAB>::make(lane);
        st<float>(a, 0, i, atan2f_wave(ld<float>(a, 0, i), ld<float>(a, 1, i), tab));
    }
};
template <int DEP>
struct SinCos {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        const float t = ld<float>(a, 0, i);
        float s = 0.0f, c = 0.0f;
        if (DEP) {
#pragma unroll 1
            for (int it = 0; it < a.loop; it++) sincosf_wave(t, &s, &c, it + (int)blockIdx.x);
        } else {
            sincosf_wave(t, &s, &c, 0);
        }
        st<float>(a, 0, i, s);
        st<float>(a, 1, i, c);
    }
};
struct Slice8Fast {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        bool nearb;
        const unsigned s = lm_slice8_fast(ld<float>(a, 0, i), ld<float>(a, 1, i), &nearb);
        st<uint32_t>(a, 0, i, s);
        st<uint32_t>(a, 1, i, nearb ? 1u : 0u);
    }
};
template <int TAB, bool ATAN>
struct Slice8 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int lane)
    {
        const auto tab = TabOf<TAB>::make(lane);
        const float re = ld<float>(a, 0, i), im = ld<float>(a, 1, i);
        st<uint32_t>(a, 0, i, ATAN ? slice_8psk_atan(re, im, tab) : slice_8psk(re, im, tab));
    }
};
template <int DEVRB>
struct DivKnown {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        const double b = ld<double>(a, 1, i);
        const double rb = DEVRB ? 1.0 / b : ld<double>(a, 2, i);
        st<double>(a, 0, i, lm_div_known(ld<double>(a, 0, i), b, rb));
    }
};
struct Norm {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        st<float>(a, 0, i, norm_f(ld<float>(a, 0, i), ld<float>(a, 1, i)));
    }
};
template <bool RECOVER>
struct CMul {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        cf32 x = {ld<float>(a, 0, i), ld<float>(a, 1, i)}, y = {ld<float>(a, 2, i), ld<float>(a, 3, i)};
        const cf32 r = cmul<RECOVER>(x, y);
        st<float>(a, 0, i, r.re);
        st<float>(a, 1, i, r.im);
    }
};
template <bool RECOVER>
struct CPow {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        cf32 x = {ld<float>(a, 0, i), ld<float>(a, 1, i)};
        const cf32 r = cpow_uint<RECOVER>(x, (unsigned)a.loop);  // (the exponent travels in Args::loop: wave-uniform)
        st<float>(a, 0, i, r.re);
        st<float>(a, 1, i, r.im);
    }
};
struct CDiv {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        cf32 x = {ld<float>(a, 0, i), ld<float>(a, 1, i)}, y = {ld<float>(a, 2, i), ld<float>(a, 3, i)};
        const cf32 r = cdiv<true>(x, y);
        st<float>(a, 0, i, r.re);
        st<float>(a, 1, i, r.im);
    }
};
template <int DEP>
struct ToLong {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        const double v = ld<double>(a, 0, i);
        long long r = 0;
        if (DEP) {
#pragma unroll 1
            for (int it = 0; it < a.loop; it++) r = to_long_x86(v, it + (int)blockIdx.x);
        } else {
            r = to_long_x86(v);
        }
        st<long long>(a, 0, i, r);
    }
};
template <int DEP>
struct Unwrap {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        const float pe = ld<float>(a, 0, i);
        const double th = ld<double>(a, 1, i);
        long long r = 0;
        if (DEP) {
#pragma unroll 1
            for (int it = 0; it < a.loop; it++) r = unwrap_count(pe, th, it + (int)blockIdx.x);
        } else {
            r = unwrap_count(pe, th);
        }
        st<long long>(a, 0, i, r);
    }
};
struct FitDen {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        float den = 1.0f, xavg = 0.0f;
        fit_denominator(ld<float>(a, 0, i), ld<uint32_t>(a, 1, i), den, xavg);
        st<float>(a, 0, i, den);
        st<float>(a, 1, i, xavg);
    }
};
struct FitValue {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        const float xd = ld<float>(a, 2, i);
        const uint32_t pts = ld<uint32_t>(a, 3, i);
        float den = 1.0f, xavg = 0.0f, m, b;
        fit_denominator(xd, pts, den, xavg);
        const float v = fit_value(ld<double>(a, 0, i), ld<double>(a, 1, i), xd, pts, den, xavg, m, b);
        st<float>(a, 0, i, v);
        st<float>(a, 1, i, m);
        st<float>(a, 2, i, b);
    }
};
struct FitKnownOp {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        const float xd = ld<float>(a, 2, i);
        const uint32_t pts = ld<uint32_t>(a, 3, i);
        float den = 1.0f, xavg = 0.0f, m;
        fit_denominator(xd, pts, den, xavg);
        const FitKnown k = fit_known(xd, pts, den, xavg);
        const float v = fit_value_known(ld<double>(a, 0, i), ld<double>(a, 1, i), k, m);
        st<float>(a, 0, i, v);
        st<float>(a, 1, i, m);
    }
};
struct Qpsk {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        int b0, b1;
        qpsk_bits(ld<float>(a, 0, i), ld<float>(a, 1, i), a.loop != 0, b0, b1);  // (the map travels in Args::loop: wave-uniform, known at run time only)
        st<int>(a, 0, i, b0);
        st<int>(a, 1, i, b1);
    }
};
struct WrapTest {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        st<uint32_t>(a, 0, i, wrap_test(ld<float>(a, 0, i), ld<float>(a, 1, i)) ? 1u : 0u);
    }
};
struct ScanF64 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<double>(a, 0, i, wave_scan_f64(ld<double>(a, 0, i))); }
};
struct SumF64 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<double>(a, 0, i, wave_sum_f64(ld<double>(a, 0, i))); }
};
struct ScanI32 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<int>(a, 0, i, wave_scan_i32(ld<int>(a, 0, i))); }
};
template <int N>
struct ScanF32Multi {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        float v[N];
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = ld<float>(a, 0, i * N + k);
        wave_scan_f32_multi(v);
#pragma unroll
        for (int k = 0; k < N; k++) st<float>(a, 0, i * N + k, v[k]);
    }
};
struct MaxF32 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<float>(a, 0, i, wave_max_f32(ld<float>(a, 0, i))); }
};
struct MaxU32 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<uint32_t>(a, 0, i, wave_max_u32(ld<uint32_t>(a, 0, i))); }
};
struct MinU32 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<uint32_t>(a, 0, i, wave_min_u32(ld<uint32_t>(a, 0, i))); }
};
template <class T>
struct Up1 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<T>(a, 0, i, wave_up1(ld<T>(a, 0, i), ld<T>(a, 1, i))); }
};
template <class T>
struct Up1Zero {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<T>(a, 0, i, wave_up1_zero(ld<T>(a, 0, i))); }
};
template <class T>
struct ReadLane {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        const int lane = uni(ld<int>(a, 1, i)) & 63;
        st<T>(a, 0, i, read_lane(ld<T>(a, 0, i), lane));
    }
};
struct Med3 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        st<int>(a, 0, i, med3_i32(ld<int>(a, 0, i), ld<int>(a, 1, i), ld<int>(a, 2, i)));
    }
};
struct AnyMerge {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        AnyTop x, y;
        x.best = ld<double>(a, 0, i), x.second = ld<double>(a, 1, i), x.k = ld<int>(a, 4, i);
        y.best = ld<double>(a, 2, i), y.second = ld<double>(a, 3, i), y.k = ld<int>(a, 5, i);
        const AnyTop r = any_merge(x, y);
        st<double>(a, 0, i, r.best);
        st<double>(a, 1, i, r.second);
        st<int>(a, 2, i, r.k);
    }
};
struct AnyMaxF64 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<double>(a, 0, i, any_max_f64(ld<double>(a, 0, i))); }
};
struct AnyMinU32 {
    static __device__ __forceinline__ void run(const Args &a, long long i, int) { st<uint32_t>(a, 0, i, any_min_u32(ld<uint32_t>(a, 0, i))); }
};
template <int U>
struct AnyMaxF64Multi {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        double v[U];
#pragma unroll
        for (int k = 0; k < U; k++) v[k] = ld<double>(a, 0, i * U + k);
        any_max_f64_multi(v);
#pragma unroll
        for (int k = 0; k < U; k++) st<double>(a, 0, i * U + k, v[k]);
    }
};
template <int U>
struct AnyMinU32Multi {
    static __device__ __forceinline__ void run(const Args &a, long long i, int)
    {
        unsigned v[U];
#pragma unroll
        for (int k = 0; k < U; k++) v[k] = ld<uint32_t>(a, 0, i * U + k);
        any_min_u32_multi(v);
#pragma unroll
        for (int k = 0; k < U; k++) st<uint32_t>(a, 0, i * U + k, v[k]);
    }
};

// every lane of every wave active: the grid is exactly n / 64 blocks of 64 threads
template <class Op>
__global__ __launch_bounds__(64) void k_full(Args a)
{
    const int lane = (int)threadIdx.x;
    Op::run(a, (long long)blockIdx.x * 64 + lane, lane);
}
// the same inside a lane-divergent branch: the lanes of `mask` run the primitive, the others nothing
template <class Op>
__global__ __launch_bounds__(64) void k_div(Args a, uint64_t mask)
{
    const int lane = (int)threadIdx.x;
    if ((mask >> lane) & 1) Op::run(a, (long long)blockIdx.x * 64 + lane, lane);
}

struct Shape {
    int n_in, in_sz[MAX_IN], n_out, out_sz[MAX_OUT];
    int mult;            // elements per case (N of the interleaved scans), else 1
    bool whole_wave;     // a cross-lane primitive or a table held in lanes: no divergent form
};

template <class Op>
hipError_t launch(const Args &a, long long n, bool divergent)
{
    const dim3 grid((unsigned)(n / 64)), block(64);
    if (!divergent) {
        hipLaunchKernelGGL(k_full<Op>, grid, block, 0, 0, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_div<Op>, grid, block, 0, 0, a, LANE_MASK_A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_div<Op>, grid, block, 0, 0, a, ~LANE_MASK_A);
    return hipGetLastError();
}

template <int N>
hipError_t launch_scan_multi(int want, const Args &a, long long n)
{
    if (want == N)
        return launch<ScanF32Multi<N>>(a, n, false);
    if constexpr (N < 32)
        return launch_scan_multi<N + 1>(want, a, n);
    return hipErrorInvalidValue;
}

}  // namespace

extern "C" int psk_dev_prims_run(int op, const void *const *in, void *const *out, long long n)
{
    const bool divergent = (op & PSK_DP_DIVERGENT) != 0;
    const int id = op & 0xff, param = (op >> 8) & 0xffff;
    if (n <= 0 || n % 64 != 0 || n / 64 > 0x7fffffffLL || !in || !out)
        return (int)hipErrorInvalidValue;
    Shape s = {};
    s.mult = 1;
    const int F = 4, D = 8;
    auto shape = [&](int n_in, int i0, int i1, int i2, int i3, int n_out, int o0, int o1, int o2, bool whole) {
        s.n_in = n_in, s.in_sz[0] = i0, s.in_sz[1] = i1, s.in_sz[2] = i2, s.in_sz[3] = i3;
        s.n_out = n_out, s.out_sz[0] = o0, s.out_sz[1] = o1, s.out_sz[2] = o2, s.whole_wave = whole;
    };
    const int tsz = param == 2 ? D : F;  // OP_UP1 / OP_UP1_ZERO / OP_READ_LANE: element size of the type
    switch (id) {
    case OP_ATAN2: shape(2, F, F, 0, 0, 1, F, 0, 0, param == 0); break;
    case OP_SINCOS: shape(1, F, 0, 0, 0, 2, F, F, 0, false); break;
    case OP_SLICE8_FAST: shape(2, F, F, 0, 0, 2, F, F, 0, false); break;
    case OP_SLICE8:
    case OP_SLICE8_ATAN: shape(2, F, F, 0, 0, 1, F, 0, 0, param == 0); break;
    case OP_DIV_KNOWN: shape(3, D, D, D, 0, 1, D, 0, 0, false); break;
    case OP_NORM: shape(2, F, F, 0, 0, 1, F, 0, 0, false); break;
    case OP_CMUL:
    case OP_CDIV: shape(4, F, F, F, F, 2, F, F, 0, false); break;
    case OP_CPOW: shape(2, F, F, 0, 0, 2, F, F, 0, false); break;
    case OP_TO_LONG: shape(1, D, 0, 0, 0, 1, D, 0, 0, false); break;
    case OP_UNWRAP: shape(2, F, D, 0, 0, 1, D, 0, 0, false); break;
    case OP_FIT_DEN: shape(2, F, F, 0, 0, 2, F, F, 0, false); break;
    case OP_FIT_VALUE: shape(4, D, D, F, F, 3, F, F, F, false); break;
    case OP_FIT_KNOWN: shape(4, D, D, F, F, 2, F, F, 0, true); break;
    case OP_QPSK: shape(2, F, F, 0, 0, 2, F, F, 0, false); break;
    case OP_WRAP_TEST: shape(2, F, F, 0, 0, 1, F, 0, 0, false); break;
    case OP_SCAN_F64:
    case OP_SUM_F64: shape(1, D, 0, 0, 0, 1, D, 0, 0, true); break;
    case OP_SCAN_I32:
    case OP_MAX_F32:
    case OP_MAX_U32:
    case OP_MIN_U32: shape(1, F, 0, 0, 0, 1, F, 0, 0, true); break;
    case OP_SCAN_F32_MULTI:
        if (param < 1 || param > 32)
            return (int)hipErrorInvalidValue;
        shape(1, F, 0, 0, 0, 1, F, 0, 0, true);
        s.mult = param;
        break;
    case OP_UP1: shape(2, tsz, tsz, 0, 0, 1, tsz, 0, 0, true); break;
    case OP_UP1_ZERO: shape(1, tsz, 0, 0, 0, 1, tsz, 0, 0, true); break;
    case OP_READ_LANE: shape(2, tsz, F, 0, 0, 1, tsz, 0, 0, true); break;
    case OP_MED3: shape(3, F, F, F, 0, 1, F, 0, 0, false); break;
    case OP_ANY_MERGE:
        shape(6, D, D, D, D, 3, D, D, F, true);
        s.in_sz[4] = s.in_sz[5] = F;
        break;
    case OP_ANY_MAX_F64: shape(1, D, 0, 0, 0, 1, D, 0, 0, true); break;
    case OP_ANY_MIN_U32: shape(1, F, 0, 0, 0, 1, F, 0, 0, true); break;
    case OP_ANY_MAX_F64_MULTI:
    case OP_ANY_MIN_U32_MULTI:
        if (param != 8)  // (the one width the front stage instantiates)
            return (int)hipErrorInvalidValue;
        shape(1, id == OP_ANY_MAX_F64_MULTI ? D : F, 0, 0, 0, 1, id == OP_ANY_MAX_F64_MULTI ? D : F, 0, 0, true);
        s.mult = param;
        break;
    default: return (int)hipErrorInvalidValue;
    }
    if (divergent && s.whole_wave)
        return (int)hipErrorInvalidValue;

    Args a = {};
    a.loop = 1;
    void *dev[MAX_IN + MAX_OUT] = {};
    hipError_t e = hipSuccess;
    auto bytes = [&](int sz) { return (size_t)sz * (size_t)s.mult * (size_t)n; };
    for (int k = 0; k < s.n_in && e == hipSuccess; k++) {
        e = hipMalloc(&dev[k], bytes(s.in_sz[k]));
        if (e == hipSuccess)
            e = hipMemcpy(dev[k], in[k], bytes(s.in_sz[k]), hipMemcpyHostToDevice);
        a.in[k] = dev[k];
    }
    for (int k = 0; k < s.n_out && e == hipSuccess; k++) {
        e = hipMalloc(&dev[MAX_IN + k], bytes(s.out_sz[k]));
        if (e == hipSuccess)
            e = hipMemset(dev[MAX_IN + k], 0xA5, bytes(s.out_sz[k]));
        a.out[k] = dev[MAX_IN + k];
    }
    if (e == hipSuccess) {
        switch (id) {
        case OP_ATAN2: e = param == 0 ? launch<Atan2<0>>(a, n, false) : launch<Atan2<1>>(a, n, divergent); break;
        case OP_SINCOS: e = param == 0 ? launch<SinCos<0>>(a, n, divergent) : launch<SinCos<1>>(a, n, divergent); break;
        case OP_SLICE8_FAST: e = launch<Slice8Fast>(a, n, divergent); break;
        case OP_SLICE8: e = param == 0 ? launch<Slice8<0, false>>(a, n, false) : launch<Slice8<1, false>>(a, n, divergent); break;
        case OP_SLICE8_ATAN: e = param == 0 ? launch<Slice8<0, true>>(a, n, false) : launch<Slice8<1, true>>(a, n, divergent); break;
        case OP_DIV_KNOWN: e = param == 0 ? launch<DivKnown<0>>(a, n, divergent) : launch<DivKnown<1>>(a, n, divergent); break;
        case OP_NORM: e = launch<Norm>(a, n, divergent); break;
        case OP_CMUL: e = param ? launch<CMul<true>>(a, n, divergent) : launch<CMul<false>>(a, n, divergent); break;
        case OP_CPOW:
            a.loop = param & 0xff;
            e = (param >> 8) ? launch<CPow<true>>(a, n, divergent) : launch<CPow<false>>(a, n, divergent);
            break;
        case OP_CDIV: e = launch<CDiv>(a, n, divergent); break;
        case OP_TO_LONG: e = param == 0 ? launch<ToLong<0>>(a, n, divergent) : launch<ToLong<1>>(a, n, divergent); break;
        case OP_UNWRAP: e = param == 0 ? launch<Unwrap<0>>(a, n, divergent) : launch<Unwrap<1>>(a, n, divergent); break;
        case OP_FIT_DEN: e = launch<FitDen>(a, n, divergent); break;
        case OP_FIT_VALUE: e = launch<FitValue>(a, n, divergent); break;
        case OP_FIT_KNOWN: e = launch<FitKnownOp>(a, n, false); break;
        case OP_QPSK:
            a.loop = param ? 1 : 0;
            e = launch<Qpsk>(a, n, divergent);
            break;
        case OP_WRAP_TEST: e = launch<WrapTest>(a, n, divergent); break;
        case OP_SCAN_F64: e = launch<ScanF64>(a, n, false); break;
        case OP_SUM_F64: e = launch<SumF64>(a, n, false); break;
        case OP_SCAN_I32: e = launch<ScanI32>(a, n, false); break;
        case OP_SCAN_F32_MULTI: e = launch_scan_multi<1>(param, a, n); break;
        case OP_MAX_F32: e = launch<MaxF32>(a, n, false); break;
        case OP_MAX_U32: e = launch<MaxU32>(a, n, false); break;
        case OP_MIN_U32: e = launch<MinU32>(a, n, false); break;
        case OP_UP1:
            e = param == 0 ? launch<Up1<int>>(a, n, false) : param == 1 ? launch<Up1<float>>(a, n, false) : launch<Up1<double>>(a, n, false);
            break;
        case OP_UP1_ZERO:
            e = param == 0 ? launch<Up1Zero<int>>(a, n, false)
                           : param == 1 ? launch<Up1Zero<float>>(a, n, false) : launch<Up1Zero<double>>(a, n, false);
            break;
        case OP_READ_LANE: e = param == 2 ? launch<ReadLane<double>>(a, n, false) : launch<ReadLane<float>>(a, n, false); break;
        case OP_MED3: e = launch<Med3>(a, n, divergent); break;
        case OP_ANY_MERGE: e = launch<AnyMerge>(a, n, false); break;
        case OP_ANY_MAX_F64: e = launch<AnyMaxF64>(a, n, false); break;
        case OP_ANY_MIN_U32: e = launch<AnyMinU32>(a, n, false); break;
        case OP_ANY_MAX_F64_MULTI: e = launch<AnyMaxF64Multi<8>>(a, n, false); break;
        case OP_ANY_MIN_U32_MULTI: e = launch<AnyMinU32Multi<8>>(a, n, false); break;
        default: e = hipErrorInvalidValue; break;
        }
    }
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    for (int k = 0; k < s.n_out && e == hipSuccess; k++)
        e = hipMemcpy(out[k], dev[MAX_IN + k], bytes(s.out_sz[k]), hipMemcpyDeviceToHost);
    for (int k = 0; k < MAX_IN + MAX_OUT; k++)
        if (dev[k])
            (void)hipFree(dev[k]);
    return (int)e;
}
