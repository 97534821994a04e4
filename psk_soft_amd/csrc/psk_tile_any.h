// psk_tile_any.h -- the wave reductions of the run-time front stages: the first maximum over the timing phases of a symbol
// (std::max_element, cpp/psk_soft.cpp:462) and its runner-up.  Shared by psk_tile_front_any_kernel (psk_tile.hip) and the
// wide-symbol front stage (psk_wide.hip).
#ifndef PSK_TILE_ANY_H
#define PSK_TILE_ANY_H

#include "psk_fast_kernel.h"

namespace psk {

struct AnyTop {
    double best, second;
    int k;
};
PSK_DEV AnyTop any_merge(const AnyTop &a, const AnyTop &b)  // first maximum: the larger sum, the lower phase on a tie
{
    const bool b_wins = b.best > a.best || (b.best == a.best && b.k < a.k);
    AnyTop r;
    r.best = b_wins ? b.best : a.best;
    r.k = b_wins ? b.k : a.k;
    const double loser = b_wins ? a.best : b.best;
    const double s2 = a.second > b.second ? a.second : b.second;
    r.second = loser > s2 ? loser : s2;
    return r;
}
// wave-wide maximum of a double / minimum of an unsigned: the scan pattern of wave_scan_f64 (row_shr 1, 2, 4, 8, row_bcast 15
// and 31) with the extremum in place of the addition, lanes without a source taking the identity; the result sits in lane 63
template <int CTRL, int ROW_MASK>
PSK_DEV double any_f64_from(double v)
{
    return __hiloint2double(__builtin_amdgcn_update_dpp((int)0xFFF00000u, __double2hiint(v), CTRL, ROW_MASK, 0xF, false),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, false));
}
PSK_DEV double any_max_f64(double v)
{
    v = __builtin_fmax(v, any_f64_from<0x111, 0xF>(v));
    v = __builtin_fmax(v, any_f64_from<0x112, 0xF>(v));
    v = __builtin_fmax(v, any_f64_from<0x114, 0xF>(v));
    v = __builtin_fmax(v, any_f64_from<0x118, 0xF>(v));
    v = __builtin_fmax(v, any_f64_from<0x142, 0xA>(v));
    v = __builtin_fmax(v, any_f64_from<0x143, 0xC>(v));
    return read_lane(v, 63);
}
// the same for U independent values, level by level: U chains that do not wait for one another
template <int CTRL, int ROW_MASK, int U>
PSK_DEV void any_max_f64_level(double (&v)[U])
{
    double o[U];
#pragma unroll
    for (int u = 0; u < U; u++) o[u] = any_f64_from<CTRL, ROW_MASK>(v[u]);
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = __builtin_fmax(v[u], o[u]);
}
template <int U>
PSK_DEV void any_max_f64_multi(double (&v)[U])
{
    any_max_f64_level<0x111, 0xF>(v);
    any_max_f64_level<0x112, 0xF>(v);
    any_max_f64_level<0x114, 0xF>(v);
    any_max_f64_level<0x118, 0xF>(v);
    any_max_f64_level<0x142, 0xA>(v);
    any_max_f64_level<0x143, 0xC>(v);
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = read_lane(v[u], 63);
}
template <int CTRL, int ROW_MASK>
PSK_DEV unsigned any_u32_from(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xF, false);
}
PSK_DEV unsigned any_min_u32(unsigned v)
{
    unsigned o;
    o = any_u32_from<0x111, 0xF>(v), v = o < v ? o : v;
    o = any_u32_from<0x112, 0xF>(v), v = o < v ? o : v;
    o = any_u32_from<0x114, 0xF>(v), v = o < v ? o : v;
    o = any_u32_from<0x118, 0xF>(v), v = o < v ? o : v;
    o = any_u32_from<0x142, 0xA>(v), v = o < v ? o : v;
    o = any_u32_from<0x143, 0xC>(v), v = o < v ? o : v;
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
template <int CTRL, int ROW_MASK, int U>
PSK_DEV void any_min_u32_level(unsigned (&v)[U])
{
    unsigned o[U];
#pragma unroll
    for (int u = 0; u < U; u++) o[u] = any_u32_from<CTRL, ROW_MASK>(v[u]);
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = o[u] < v[u] ? o[u] : v[u];
}
template <int U>
PSK_DEV void any_min_u32_multi(unsigned (&v)[U])
{
    any_min_u32_level<0x111, 0xF>(v);
    any_min_u32_level<0x112, 0xF>(v);
    any_min_u32_level<0x114, 0xF>(v);
    any_min_u32_level<0x118, 0xF>(v);
    any_min_u32_level<0x142, 0xA>(v);
    any_min_u32_level<0x143, 0xC>(v);
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = (unsigned)__builtin_amdgcn_readlane((int)v[u], 63);
}

}  // namespace psk
#endif
