// Pillow's 8-bit bicubic resampler (Resample.c: bicubic_filter, precompute_coeffs, normalize_coeffs_8bpc), the device functions shared by
// collate.hip (images into the device) and export.hip (images out of it).  tests/pil_resample_ref.py is the specification.
// Every file that includes this header is compiled with -ffp-contract=off (tatt_amd/build.py): a fused multiply-add in the polynomial or
// in `center` changes coefficients.
#pragma once
#include <math.h>

#define COL_PB 22                      // Pillow's PRECISION_BITS

static __host__ __device__ inline int col_ksize(int in, int out) {
    double fs = (double)in / out;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(2.0 * fs) * 2 + 1;
}

__device__ __forceinline__ double col_bicubic(double x) {          // Pillow's bicubic_filter, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// row `xx` of the coefficient table of a pass from `in` to `out` samples: kk[xx][0 .. n) and bounds[xx] = (first source sample, n)
__device__ __forceinline__ void col_coeffs(int xx, int in, int out, int ksize, int* kk, int* bounds) {
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, center = (xx + 0.5) * scale, ss = 1.0 / fs;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;                                                   // (<= ksize: Pillow sizes its own table by the same bound)
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += col_bicubic((x + xmin - center + 0.5) * ss);
    int* k = kk + xx * ksize;
    for (int x = 0; x < xmax; ++x) {
        double w = col_bicubic((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        k[x] = w < 0 ? (int)(-0.5 + w * (1 << COL_PB)) : (int)(0.5 + w * (1 << COL_PB));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
}

__device__ __forceinline__ int col_clip8(int acc) {
    const int v = acc >> COL_PB;                                    // arithmetic shift
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
