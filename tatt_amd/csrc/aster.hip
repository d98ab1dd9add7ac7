// The ASTER recogniser (reference model/recognizer/): the pieces its front and encoder need beyond the shared operators (its attention
// decoder is csrc/attndec.hip).
//   resize_bilinear_ac : F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=True)        (recognizer_builder.py:77)
//   grid_sample_sized  : tatt_grid_sample_fwd with an output size of its own (32 x 128 in, 32 x 100 out; tps_spatial_transformer.py:110-114)
//   add_relu           : relu(a + b), the tail of AsterBlock (resnet_aster.py:59-60)
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void resize_bilinear_ac_kernel(const float* __restrict__ x, long xsn, long xsc, long xsh, long xsw, float* __restrict__ y,
                                          int B, int C, int H, int W, int Ho, int Wo) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * C * Ho * Wo) return;
    const int ox = idx % Wo, oy = (idx / Wo) % Ho, c = (idx / ((long)Wo * Ho)) % C, b = idx / ((long)Wo * Ho * C);
    // torch's area_pixel_compute_scale for align_corners=True: (in - 1) / (out - 1) in fp32, source index = scale * destination index
    const float sh = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, sw = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const float fy = sh * oy, fx = sw * ox;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 < H - 1 ? y0 + 1 : y0, x1 = x0 < W - 1 ? x0 + 1 : x0;
    const float ly = fy - y0, lx = fx - x0;
    const float* p = x + b * xsn + c * xsc;
    const float v00 = p[y0 * xsh + x0 * xsw], v01 = p[y0 * xsh + x1 * xsw], v10 = p[y1 * xsh + x0 * xsw], v11 = p[y1 * xsh + x1 * xsw];
    y[idx] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}
TATT_API int tatt_resize_bilinear_ac(const float* x, long xsn, long xsc, long xsh, long xsw, float* y, int B, int C, int H, int W,
                                     int Ho, int Wo, hipStream_t st) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return 1;
    hipLaunchKernelGGL(resize_bilinear_ac_kernel, dim3(cdiv((long)B * C * Ho * Wo, 256)), dim3(256), 0, st, x, xsn, xsc, xsh, xsw, y, B, C,
                       H, W, Ho, Wo);
    return LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct SizedSampleGeom { int B, C, H, W, Ho, Wo; long xsn, xsc, xsh, xsw; };

__device__ __forceinline__ float sized_tap(const float* x, const SizedSampleGeom& g, int b, int c, int yi, int xi) {
    if (xi < 0 || xi >= g.W || yi < 0 || yi >= g.H) return 0.f;
    return x[b * g.xsn + c * g.xsc + yi * g.xsh + xi * g.xsw];
}
// out (B,Ho,Wo,C) NHWC; one thread per output pixel
__global__ void grid_sample_sized_kernel(const float* __restrict__ x, const float* __restrict__ src, float* __restrict__ out,
                                         SizedSampleGeom g) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)g.B * g.Ho * g.Wo) return;
    const int b = idx / ((long)g.Ho * g.Wo);
    const float cx = fminf(fmaxf(src[idx * 2], 0.f), 1.f), cy = fminf(fmaxf(src[idx * 2 + 1], 0.f), 1.f);
    const float gx = 2.f * cx - 1.f, gy = 2.f * cy - 1.f;
    const float ix = ((gx + 1.f) * g.W - 1.f) * 0.5f, iy = ((gy + 1.f) * g.H - 1.f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = ix - fx, ty = iy - fy;
    for (int c = 0; c < g.C; ++c) {
        const float v00 = sized_tap(x, g, b, c, y0, x0), v01 = sized_tap(x, g, b, c, y0, x0 + 1);
        const float v10 = sized_tap(x, g, b, c, y0 + 1, x0), v11 = sized_tap(x, g, b, c, y0 + 1, x0 + 1);
        out[idx * g.C + c] = v00 * (1.f - tx) * (1.f - ty) + v01 * tx * (1.f - ty) + v10 * (1.f - tx) * ty + v11 * tx * ty;
    }
}
TATT_API int tatt_grid_sample_sized_fwd(const float* x, long xsn, long xsc, long xsh, long xsw, const float* src, float* out, int B,
                                        int C, int H, int W, int Ho, int Wo, hipStream_t st) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return 1;
    SizedSampleGeom g = {B, C, H, W, Ho, Wo, xsn, xsc, xsh, xsw};
    hipLaunchKernelGGL(grid_sample_sized_kernel, dim3(cdiv((long)B * Ho * Wo, 256)), dim3(256), 0, st, x, src, out, g);
    return LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void add_relu_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = fmaxf(a[i] + b[i], 0.f);
}
TATT_API int tatt_add_relu(const float* a, const float* b, float* y, long n, hipStream_t st) {
    if (n < 1) return 1;
    hipLaunchKernelGGL(add_relu_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a, b, y, n);
    return LAUNCH_CHECK();
}
