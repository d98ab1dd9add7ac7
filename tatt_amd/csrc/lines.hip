// Text lines of any width through a model that knows one LR size: the two device ends of the windowed path (tatt_amd/lines.py is the
// specification, tests/test_lines*.py hold both to it).  A line is resized to the window height at its own aspect ratio (h x wl), cut
// into h x w windows, every window is super-resolved like a training crop, and the SR windows are merged back into one image.
//   line_windows_kernel  the way in: for every window of every line `line.resize((wl, h), BICUBIC).crop((x0, 0, x0 + w, h))`, ToTensor and
//                        the window's OWN mask plane.  Pillow's resampler treats every output column on its own, horizontal pass first, so
//                        the window is computed without the rest of the line: bit for bit the host's.
//   line_blend_kernel    the way out: quantise the SR windows (the arithmetic of export.hip) and merge them with integer tent weights.
// Both follow collate.hip / export.hip: no traffic between work-groups, no atomics, every loop bounded by descriptor values that were
// checked, every quantity read from DEVICE memory (a captured launch sees what the staging copy in front of it wrote), the same check
// on the host before the launch and in the kernel.  Compiled with -ffp-contract=off (tatt_amd/build.py), for pil_resample.h's tables in
// double and for the quantisation (one fp32 multiply, then one fp32 add).
//
// line_windows_kernel, one work-group of 256 threads per window, is pil_window_body of pil_resample.h on the FULL-LINE geometry: the
// coefficient rows x0 .. x0 + w - 1 of the table W_src -> wl, the horizontal pass for those w columns only, the vertical pass into the
// float planes, the mask plane from the mean of the WINDOW (not the line: each window must look like a training crop).
// LDS per window at the limits (LIN_* of line_limits.h): horizontal table 32,768 + bounds 2,048, vertical table and bounds < 5,120,
// L 16,384, the intermediate 65,536, the reduction 16: under 122 KB of the CU's 160 KB.  A launch asks for what its largest window needs.
//
// line_blend_kernel, grid (lines, column tiles), one thread per output PIXEL and step: the windows that cover canvas column X are found
// by a binary search in the line's table of window starts (LDS), each contributes its quantised value with the weight min(j + 1, W - j)
// of its local column j, and the pixel is the weighted mean rounded half up, (2 N + D) / (2 D), in integers.
#include "common.h"
#include "pil_resample.h"         // pil_win_layout, pil_window_body; exp_quant
#include "line_limits.h"          // LIN_* limits, lin_takes (shared with scene.hip)

#define LIN_DESC 12                    // ints per window row: src byte offset, H_src, W_src, h, wl, x0, w, mask flag, out float offset, 0, 0, 0

#define BLD_THREADS 256
#define BLD_DESC 8                     // ints per line row: first window, windows, wl, scale, rule, c0, out byte offset, row pitch in bytes
#define BLD_MAX_WINDOWS 1024           // windows of one line (its starts live in LDS)
#define BLD_MAX_TILES 64               // grid.y

// 0: the row is taken; 1: a reserved word is set; 2: geometry beyond tatt_line_limits; 3: the source or the planes leave packed / out
static __host__ __device__ inline int lin_check(const int* d, long packed_bytes, long out_floats) {
    const int off = d[0], hs = d[1], ws = d[2], h = d[3], wl = d[4], x0 = d[5], w = d[6], out_off = d[8];
    if (d[9] != 0 || d[10] != 0 || d[11] != 0) return 1;
    if (!lin_takes(hs, ws, h, wl, x0, w)) return 2;
    if (off < 0 || off + (long)hs * ws * 3 > packed_bytes) return 3;
    if (out_off < 0 || out_off + (long)(3 + (d[7] != 0)) * h * w > out_floats) return 3;
    return 0;
}

__global__ __launch_bounds__(LIN_THREADS) void line_windows_kernel(const unsigned char* __restrict__ packed, long packed_bytes,
                                                                   const int* __restrict__ desc, float* __restrict__ out_base,
                                                                   long out_floats, int lds_bytes) {
    extern __shared__ __align__(16) unsigned char lin_lds[];
    const int tid = threadIdx.x;
    const int* d = desc + (long)blockIdx.x * LIN_DESC;
    const int src_off = d[0], hs = d[1], ws = d[2], h = d[3], wl = d[4], x0 = d[5], w = d[6], mask = d[7] != 0, out_off = d[8];
    // The host entry refuses such rows before it launches; a replayed launch re-checks so that a stale row cannot reach outside the
    // buffers: the window's planes (when they lie inside) are filled with NaN, nothing else is touched.
    const long N = (long)h * w, planes = 3 + mask;
    if (h < 1 || w < 1 || h > LIN_MAX_H || w > LIN_MAX_W || out_off < 0 || out_off + planes * N > out_floats) return;
    float* out = out_base + out_off;
    const bool ok = lin_check(d, packed_bytes, out_floats) == 0;
    const PilWinLayout g = ok ? pil_win_layout<LIN_THREADS>(hs, ws, h, wl, w, mask) : PilWinLayout{};
    if (!ok || g.total > lds_bytes) return pil_win_refuse<LIN_THREADS>(out, planes * N, tid);
    pil_window_body<LIN_THREADS>(packed + src_off, (long)(3 * ws), g, lin_lds, hs, ws, h, wl, x0, w, mask, out, tid);
}

TATT_API int tatt_line_limits(int* out) {
    if (!out) return 1;
    out[0] = LIN_MAX_ROWS;
    out[1] = LIN_MAX_COLS;
    out[2] = LIN_MAX_WL;
    out[3] = LIN_MAX_H;
    out[4] = LIN_MAX_W;
    out[5] = LIN_MAX_INTER;
    out[6] = LIN_MAX_TABLE;
    out[7] = BLD_MAX_WINDOWS;
    return 0;
}

TATT_API int tatt_line_windows(const unsigned char* packed, long packed_bytes, const int* desc, const int* desc_host, int n_windows,
                               float* out, long out_floats, hipStream_t st) {
    if (!packed || !desc || !desc_host || !out || n_windows <= 0 || packed_bytes <= 0 || out_floats <= 0) return 1;
    int lds = 0;
    for (int i = 0; i < n_windows; ++i) {
        const int* d = desc_host + (long)i * LIN_DESC;
        const int rc = lin_check(d, packed_bytes, out_floats);
        if (rc) return rc;
        const int total = pil_win_layout<LIN_THREADS>(d[1], d[2], d[3], d[4], d[6], d[7] != 0).total;
        if (total > LIN_LDS) return 2;
        if (total > lds) lds = total;
    }
    static TattPerDevice attr_once;                 // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(line_windows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LIN_LDS);
    });
    hipLaunchKernelGGL(line_windows_kernel, dim3(n_windows), dim3(LIN_THREADS), (size_t)lds, st, packed, packed_bytes, desc, out, out_floats,
                       lds);
    return LAUNCH_CHECK();
}

// ---- the way out ----------------------------------------------------------------------------------------------------------------------
// 0: the row is taken; 1: no such rule; 2: geometry (scale, wl, window count); 3: windows, channels or destination bytes leave
// src / starts / out.  The same function refuses on the host before the launch and in the kernel.
static __host__ __device__ inline int bld_check(const int* d, int B, int C, int H, int W, int n_starts, long out_bytes) {
    const int first = d[0], n = d[1], wl = d[2], scale = d[3], rule = d[4], c0 = d[5], off = d[6], pitch = d[7];
    if (rule != 0 && rule != 1) return 1;
    if (H < 1 || W < 1 || scale < 1 || W % scale != 0 || n < 1 || n > BLD_MAX_WINDOWS) return 2;
    if (wl < W / scale || wl > LIN_MAX_WL || (long)scale * wl * 3 > 0x7fffffffL / H) return 2;
    if (first < 0 || first > B - n || first > n_starts - n || c0 < 0 || c0 > C - 3) return 3;
    if (off < 0 || pitch < 3 * scale * wl || (long)off + (long)(H - 1) * pitch + 3L * scale * wl > out_bytes) return 3;
    return 0;
}

// the line's window starts (host copy): the first at 0, the last flush right, increasing, no column left uncovered
static inline bool bld_starts_ok(const int* s, int n, int wl, int w) {
    if (s[0] != 0 || s[n - 1] != wl - w) return false;
    for (int k = 1; k < n; ++k)
        if (s[k] <= s[k - 1] || s[k] - s[k - 1] > w) return false;
    return true;
}

__global__ __launch_bounds__(BLD_THREADS) void line_blend_kernel(const float* __restrict__ src, long st_n, long st_c, long st_h, long st_w,
                                                                 int B, int C, int H, int W, const int* __restrict__ desc,
                                                                 const int* __restrict__ starts, int n_starts,
                                                                 unsigned char* __restrict__ out_base, long out_bytes) {
    __shared__ int sx[BLD_MAX_WINDOWS];                             // canvas column of every window's first column
    const int tid = threadIdx.x;
    const int* d = desc + (long)blockIdx.x * BLD_DESC;
    // a replayed launch re-checks: nothing is written for a row the host entry would have refused
    if (bld_check(d, B, C, H, W, n_starts, out_bytes) != 0) return;
    const int first = d[0], n = d[1], wl = d[2], scale = d[3], rule = d[4], c0 = d[5], pitch = d[7];
    const int cw = scale * wl, npix = H * cw;
    if ((long)blockIdx.y * BLD_THREADS >= npix) return;
    for (int k = tid; k < n; k += BLD_THREADS) sx[k] = scale * starts[first + k];
    __syncthreads();
    const float* s = src + (long)first * st_n + (long)c0 * st_c;
    unsigned char* out = out_base + d[6];
    for (int i = blockIdx.y * BLD_THREADS + tid; i < npix; i += gridDim.y * BLD_THREADS) {
        const int y = i / cw, X = i - y * cw;
        int lo = 0, hi = n;                                          // the first window that ends beyond X (starts increase)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sx[mid] + W > X) hi = mid; else lo = mid + 1;
        }
        int n0 = 0, n1 = 0, n2 = 0, den = 0;
        for (int k = lo; k < n; ++k) {
            const int j = X - sx[k];
            if (j < 0) break;
            if (j >= W) continue;                                    // (only a stale table: the search already skipped these)
            const int wt = min(j + 1, W - j);
            const float* p = s + k * st_n + y * st_h + j * st_w;
            n0 += wt * exp_quant(p[0], rule);
            n1 += wt * exp_quant(p[st_c], rule);
            n2 += wt * exp_quant(p[2 * st_c], rule);
            den += wt;
        }
        unsigned char* q = out + (long)y * pitch + 3 * X;
        q[0] = (unsigned char)(den ? (2 * n0 + den) / (2 * den) : 0);
        q[1] = (unsigned char)(den ? (2 * n1 + den) / (2 * den) : 0);
        q[2] = (unsigned char)(den ? (2 * n2 + den) / (2 * den) : 0);
    }
}

TATT_API int tatt_line_blend(const float* src, long st_n, long st_c, long st_h, long st_w, int B, int C, int H, int W, const int* desc,
                             const int* desc_host, int n_lines, const int* starts, const int* starts_host, int n_starts,
                             unsigned char* out, long out_bytes, hipStream_t st) {
    if (!src || !desc || !desc_host || !starts || !starts_host || !out || n_lines <= 0 || n_starts <= 0 || out_bytes <= 0) return 1;
    if (B <= 0 || C < 3 || H <= 0 || W <= 0 || st_n < 0 || st_c < 0 || st_h < 0 || st_w < 0) return 1;
    long most = 0;
    for (int i = 0; i < n_lines; ++i) {
        const int* d = desc_host + (long)i * BLD_DESC;
        const int rc = bld_check(d, B, C, H, W, n_starts, out_bytes);
        if (rc) return rc;
        if (!bld_starts_ok(starts_host + d[0], d[1], d[2], W / d[3])) return 2;
        const long npix = (long)H * d[3] * d[2];
        if (npix > most) most = npix;
    }
    int tiles = cdiv(most, BLD_THREADS * 4);                        // about four pixels per thread
    if (tiles > BLD_MAX_TILES) tiles = BLD_MAX_TILES;
    hipLaunchKernelGGL(line_blend_kernel, dim3(n_lines, tiles), dim3(BLD_THREADS), 0, st, src, st_n, st_c, st_h, st_w, B, C, H, W, desc,
                       starts, n_starts, out, out_bytes);
    return LAUNCH_CHECK();
}
