// Float64 helpers shared by the CTC decoders that work on path probabilities on the device (ctcbeam.hip, ctclex.hip, ctcwords.hip): the
// log-sum-exp of two terms as the host specification states it (tatt_amd/read.py `_beam_real`), wave-wide maxima, minima and sums, and
// the move of a value to the lane above (`lx_below`, the neighbour states of ctclex.hip and ctcwords.hip).
#pragma once
#include "common.h"

#define CB_NEG (-__builtin_inf())

__device__ __forceinline__ double cb_lse(double a, double b) {
    const double m = a > b ? a : b, n = a > b ? b : a;
    return n == CB_NEG ? m : m + log1p(exp(n - m));
}

// Wave maximum and sum by data-parallel-primitive moves: four shifts inside each row of 16 lanes leave the row's result in its lane 15,
// two row broadcasts carry it on, lane 63 holds the wave's and hands it to every lane through scalar registers.  A lane without a source
// takes the neutral element (its own value for the maximum, 0 for the sum).
template <int CTRL, int ROWS>
__device__ __forceinline__ double cb_add(double v) {
    return v + __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xf, false),
                                __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ double cb_wave_sum(double v) {
    v = cb_add<0x111, 0xf>(v);                                       // row_shr:1, 2, 4, 8
    v = cb_add<0x112, 0xf>(v);
    v = cb_add<0x114, 0xf>(v);
    v = cb_add<0x118, 0xf>(v);
    v = cb_add<0x142, 0xa>(v);                                       // row_bcast:15 into rows 1 and 3
    v = cb_add<0x143, 0xc>(v);                                       // row_bcast:31 into rows 2 and 3
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
template <int CTRL>
__device__ __forceinline__ float cb_max(float v) {
    const int i = __float_as_int(v);
    return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false)));
}
__device__ __forceinline__ float cb_wave_max(float v) {
    v = cb_max<0x111>(v);
    v = cb_max<0x112>(v);
    v = cb_max<0x114>(v);
    v = cb_max<0x118>(v);
    v = cb_max<0x142>(v);
    v = cb_max<0x143>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

template <int CTRL>
__device__ __forceinline__ double cb_maxd(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return fmax(v, __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false),
                                    __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false)));
}
__device__ __forceinline__ double cb_wave_maxd(double v) {           // (no NaN ever gets here)
    v = cb_maxd<0x111>(v);
    v = cb_maxd<0x112>(v);
    v = cb_maxd<0x114>(v);
    v = cb_maxd<0x118>(v);
    v = cb_maxd<0x142>(v);
    v = cb_maxd<0x143>(v);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
template <int CTRL>
__device__ __forceinline__ int cb_mini(int v) {
    const int o = __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
    return o < v ? o : v;
}
__device__ __forceinline__ int cb_wave_mini(int v) {
    v = cb_mini<0x111>(v);
    v = cb_mini<0x112>(v);
    v = cb_mini<0x114>(v);
    v = cb_mini<0x118>(v);
    v = cb_mini<0x142>(v);
    v = cb_mini<0x143>(v);
    return __builtin_amdgcn_readlane(v, 63);
}

// the value the lane below holds (lane - 1), -inf in lane 0 of the wave; G == 16 never looks across a row of 16 lanes (a segment's
// first lane takes no neighbour), so the row shift alone serves it
template <int G>
__device__ __forceinline__ double lx_below(double v, int lane) {
    const int nh = (int)0xfff00000, nl = 0;                          // -inf
    int hi = __builtin_amdgcn_update_dpp(nh, __double2hiint(v), 0x111, 0xf, 0xf, false);         // row_shr:1
    int lo = __builtin_amdgcn_update_dpp(nl, __double2loint(v), 0x111, 0xf, 0xf, false);
    if (G > 16) {
        const int bh = __builtin_amdgcn_update_dpp(nh, __double2hiint(v), 0x142, 0xf, 0xf, false);   // row_bcast:15 into rows 1, 2, 3
        const int bl = __builtin_amdgcn_update_dpp(nl, __double2loint(v), 0x142, 0xf, 0xf, false);
        if ((lane & 15) == 0) {
            hi = bh;
            lo = bl;
        }
    }
    return __hiloint2double(hi, lo);
}

// the same move for a 32-bit value (a token's start step in ctcwords.hip); lane 0 of the wave takes `fill`
__device__ __forceinline__ int lx_below_i(int v, int lane, int fill) {
    int r = __builtin_amdgcn_update_dpp(fill, v, 0x111, 0xf, 0xf, false);                        // row_shr:1
    const int b = __builtin_amdgcn_update_dpp(fill, v, 0x142, 0xf, 0xf, false);                  // row_bcast:15 into rows 1, 2, 3
    if ((lane & 15) == 0) r = b;
    return r;
}

// Exclusive scans of a wave's 64 values (ctcpat.hip: the sum over every lane but one's own is prefix + suffix, a sum of non-negative
// terms, never total - own).  Inside a row of 16 lanes: four row shifts make the inclusive scan, one more shift makes it exclusive (the
// row's first / last lane takes 0); across rows: the rows' totals are read from the rows' last / first lanes and the earlier / later
// ones are added.  The order of the additions is fixed.
template <int CTRL>
__device__ __forceinline__ double cb_moved(double v) {               // the value CTRL moves here, 0 for a lane without a source
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ double cb_lane_value(double v, int k) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}
__device__ __forceinline__ double cb_wave_excl_prefix(double v, int lane) {
    v = v + cb_moved<0x111>(v);                                      // row_shr:1, 2, 4, 8
    v = v + cb_moved<0x112>(v);
    v = v + cb_moved<0x114>(v);
    v = v + cb_moved<0x118>(v);
    const double t0 = cb_lane_value(v, 15), t1 = cb_lane_value(v, 31), t2 = cb_lane_value(v, 47);
    const int row = lane >> 4;
    return cb_moved<0x111>(v) + (row == 0 ? 0.0 : row == 1 ? t0 : row == 2 ? t0 + t1 : (t0 + t1) + t2);
}
__device__ __forceinline__ double cb_wave_excl_suffix(double v, int lane) {
    v = v + cb_moved<0x101>(v);                                      // row_shl:1, 2, 4, 8
    v = v + cb_moved<0x102>(v);
    v = v + cb_moved<0x104>(v);
    v = v + cb_moved<0x108>(v);
    const double t1 = cb_lane_value(v, 16), t2 = cb_lane_value(v, 32), t3 = cb_lane_value(v, 48);
    const int row = lane >> 4;
    return cb_moved<0x101>(v) + (row == 3 ? 0.0 : row == 2 ? t3 : row == 1 ? t3 + t2 : (t3 + t2) + t1);
}
