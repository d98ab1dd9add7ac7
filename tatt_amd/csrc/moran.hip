// The MORAN recogniser (reference model/moran/): the rectifier's chain of tiny dependent launches as ONE launch (the other chain of its
// eval path, the attention decoder, is csrc/attndec.hip).
//   morn_rectify : the tail of the MORN rectifier (morn.py:62-69 and :76-82): relu(+-o) -> 2x2 stride-1 max-pools -> their difference ->
//                  grid_sample at the regular grid -> offsets_grid (set or accumulated) -> grid_sample of the image at (gx, gy + offsets)
// Both samplers are bilinear with zeros padding and align_corners=False, which is how the installed torch runs the reference's calls.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------------------
#define MR_MAXMAP 4096    // floats of one image's offsets map staged in LDS (the product's is 4 x 12)

struct MornGeom { int first, B, C, H, W, Ho, Wo, h, w; long xsn, xsc, xsh, xsw; };

// p[i][j] = max2x2(relu(o))[i][j] - max2x2(relu(-o))[i][j] on the (h - 1) x (w - 1) pooled map, zero outside it
__device__ __forceinline__ float morn_pooled(const float* so, int h, int w, int i, int j) {
    if (i < 0 || j < 0 || i >= h - 1 || j >= w - 1) return 0.f;
    const float a = so[i * w + j], b = so[i * w + j + 1], c = so[(i + 1) * w + j], d = so[(i + 1) * w + j + 1];
    const float pos = fmaxf(fmaxf(fmaxf(a, b), fmaxf(c, d)), 0.f);
    const float neg = fmaxf(fmaxf(fmaxf(-a, -b), fmaxf(-c, -d)), 0.f);
    return pos - neg;
}
__device__ __forceinline__ float morn_tap(const float* x, const MornGeom& g, int yi, int xi) {
    if (xi < 0 || xi >= g.W || yi < 0 || yi >= g.H) return 0.f;
    return x[yi * g.xsh + xi * g.xsw];
}
// the reference's regular grid: float64 `arange * 2. / (n - 1) - 1`, rounded to fp32 once
__device__ __forceinline__ float morn_coord(int i, int n) { return (float)((double)i * 2.0 / (double)(n - 1) - 1.0); }

// grid (cdiv(Ho * Wo, 256), B): one thread per output pixel, a work-group stays inside one image
__global__ __launch_bounds__(256) void morn_rectify_kernel(const float* __restrict__ o, float* __restrict__ acc,
                                                           const float* __restrict__ x, float* __restrict__ out, MornGeom g) {
    __shared__ float so[MR_MAXMAP];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < g.h * g.w; i += 256) so[i] = o[(long)b * g.h * g.w + i];
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= g.Ho * g.Wo) return;
    const int oy = pix / g.Wo, ox = pix % g.Wo;
    const float gx = morn_coord(ox, g.Wo), gy = morn_coord(oy, g.Ho);
    // ---- the offsets map sampled at the regular grid (the pooled map is (h - 1) x (w - 1))
    float gval;
    {
        const float ix = ((gx + 1.f) * (float)(g.w - 1) - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)(g.h - 1) - 1.f) * 0.5f;
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float tx = ix - fx, ty = iy - fy;
        const float v00 = morn_pooled(so, g.h, g.w, y0, x0), v01 = morn_pooled(so, g.h, g.w, y0, x0 + 1);
        const float v10 = morn_pooled(so, g.h, g.w, y0 + 1, x0), v11 = morn_pooled(so, g.h, g.w, y0 + 1, x0 + 1);
        gval = v00 * (1.f - tx) * (1.f - ty) + v01 * tx * (1.f - ty) + v10 * (1.f - tx) * ty + v11 * tx * ty;
    }
    const long ai = (long)b * g.Ho * g.Wo + pix;
    const float off = g.first ? gval : acc[ai] + gval;
    acc[ai] = off;
    // ---- the image sampled at (gx, gy + offsets)
    const float sy = gy + off;
    const float ix = ((gx + 1.f) * (float)g.W - 1.f) * 0.5f, iy = ((sy + 1.f) * (float)g.H - 1.f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    // (offsets of a trained network stay within the image; the clamp keeps the int conversion defined for any input, and a tap
    // that far out reads as zero either way)
    const int x0 = (int)fminf(fmaxf(fx, -2.f), (float)g.W + 1.f), y0 = (int)fminf(fmaxf(fy, -2.f), (float)g.H + 1.f);
    const float tx = ix - fx, ty = iy - fy;
    for (int c = 0; c < g.C; ++c) {
        const float* xc = x + b * g.xsn + c * g.xsc;
        const float v00 = morn_tap(xc, g, y0, x0), v01 = morn_tap(xc, g, y0, x0 + 1);
        const float v10 = morn_tap(xc, g, y0 + 1, x0), v11 = morn_tap(xc, g, y0 + 1, x0 + 1);
        out[ai * g.C + c] = v00 * (1.f - tx) * (1.f - ty) + v01 * tx * (1.f - ty) + v10 * (1.f - tx) * ty + v11 * tx * ty;
    }
}
TATT_API int tatt_morn_rectify(const float* o, int h, int w, float* acc, int first, const float* x, long xsn, long xsc, long xsh,
                               long xsw, float* out, int B, int C, int H, int W, int Ho, int Wo, hipStream_t st) {
    if (h < 2 || w < 2 || C < 1 || C > 4 || (long)h * w > MR_MAXMAP) return 1;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || Ho < 2 || Wo < 2 || (long)Ho * Wo > (1L << 24)) return 1;
    MornGeom g = {first ? 1 : 0, B, C, H, W, Ho, Wo, h, w, xsn, xsc, xsh, xsw};
    hipLaunchKernelGGL(morn_rectify_kernel, dim3(cdiv((long)Ho * Wo, 256), B), dim3(256), 0, st, o, acc, x, out, g);
    return LAUNCH_CHECK();
}
