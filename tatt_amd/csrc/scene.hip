// Scene images: the text boxes of a photograph super-resolved and pasted back (tatt_amd/scene.py is the specification, tests/test_scene*.py
// hold the kernels to it).  The model and the tent blend are those of the windowed path (lines.hip); this file adds the two ends that need
// the whole picture:
//   scene_windows_kernel  line_windows_kernel of lines.hip for sources that are SUB-RECTANGLES of one uploaded image: a row carries the
//                         row pitch of the image and the box origin, the (W_src, H_src) of the tables are the box's.  Pillow's
//                         `scene.crop(box).resize(..)` sees the box's pixels alone, so do the coefficient rows here.
//   resize_u8_kernel      Pillow's 8-bit bicubic `Image.resize`, uint8 RGB in device memory to uint8 RGB in device memory, TILED over the
//                         output, so an image of any size goes through: the up-scaled scene (the background) and every SR line resized
//                         into its box (the pastes, optionally feathered against what the canvas already holds).
// Both follow collate.hip / export.hip / lines.hip: no traffic between work-groups, no atomics, every loop bounded by descriptor values
// that were checked, every quantity read from DEVICE memory, the same check on the host before the launch and in the kernel.  Compiled
// with -ffp-contract=off (tatt_amd/build.py) for pil_resample.h's tables in double.
//
// resize_u8_kernel, grid (tile, item), 256 threads, one tile of th x 64 output pixels per work-group.  A tile of Pillow's resize depends
// only on the source rows and columns that the coefficient rows of its own output rows and columns name, so a tile is computed alone:
//   phase 0  the tile's coefficient rows in LDS: 64 rows of the horizontal table W_src -> OW, th rows of the vertical table H_src -> OH
//   phase 1  horizontal pass for the source rows r0 .. r0 + nr - 1 that the tile's vertical rows name, rounded to uint8 as Pillow rounds
//            its intermediate image, into LDS [nr][64][3].  A wave takes 64 neighbouring output columns of ONE source row: its lanes read
//            one contiguous span of that row (64 * W_src / OW + ksize pixels), i.e. a few cache lines per tap.
//   phase 2  vertical pass from LDS: a wave reads, per tap, the 192 consecutive bytes of one intermediate row (lane x bytes 3x .. 3x + 2:
//            48 consecutive dwords, lanes sharing a dword are served by one broadcast -- no bank conflict), then clips, feathers and
//            stores its pixel (a wave writes 192 contiguous bytes of a canvas row).
// A pass whose sizes agree is skipped as Pillow skips it (the vertical pass then reads the source itself, the horizontal one writes
// th rows).  th = 32 while the tile's source rows fit RSZ_INTER_ROWS = 192 rows of intermediate, halved until they do (down-scales
// beyond ~5 : 1 in the vertical; 1 row at 16 : 1), so the LDS of a tile is bounded whatever the factor: horizontal table <= 64 * 65 * 4,
// intermediate <= 192 * 192, vertical table <= 2,944, bounds 768: under 58 KB; an up-scale takes under 10 KB.  No per-thread arrays.
#include "common.h"
#include "pil_resample.h"         // col_ksize, col_coeffs, col_clip8 (shared with collate.hip, export.hip and lines.hip)

// ---- windows of boxes ------------------------------------------------------------------------------------------------------------------
#define SCW_THREADS 256
#define SCW_DESC 16                    // ints per window row: lines.hip's words 0 .. 8, [9] row pitch in bytes, [10] box x, [11] box y, [12..15] 0
#define SCW_MAX_ROWS 256               // the limits of lines.hip (tatt_line_limits): one host fallback decides for both
#define SCW_MAX_COLS 16384
#define SCW_MAX_WL 4096
#define SCW_MAX_H 64
#define SCW_MAX_W 256
#define SCW_MAX_INTER 65536
#define SCW_MAX_TABLE 32768
#define SCW_LDS 126976

struct ScwLayout { int ksh, ksv, kh, bh, kv, bv, lum, inter, red, total; };

// 0: the row is taken; 1: a reserved word is set; 2: geometry beyond tatt_line_limits; 3: the box or the planes leave packed / out
static __host__ __device__ inline int scw_check(const int* d, long packed_bytes, long out_floats) {
    const int off = d[0], hs = d[1], ws = d[2], h = d[3], wl = d[4], x0 = d[5], w = d[6], out_off = d[8], pitch = d[9], bx = d[10], by = d[11];
    if (d[12] != 0 || d[13] != 0 || d[14] != 0 || d[15] != 0) return 1;
    if (hs < 1 || ws < 1 || h < 1 || w < 1 || h > SCW_MAX_H || w > SCW_MAX_W || wl < w || wl > SCW_MAX_WL) return 2;
    if (x0 < 0 || x0 > wl - w || hs > SCW_MAX_ROWS || ws > SCW_MAX_COLS) return 2;
    if (ws != wl && ((long)hs * w * 3 > SCW_MAX_INTER || (long)w * col_ksize(ws, wl) * 4 > SCW_MAX_TABLE)) return 2;
    if (off < 0 || bx < 0 || by < 0 || pitch < 3L * ((long)bx + ws)) return 3;
    if (off + ((long)by + hs - 1) * pitch + 3L * ((long)bx + ws) > packed_bytes) return 3;
    if (out_off < 0 || out_off + (long)(3 + (d[7] != 0)) * h * w > out_floats) return 3;
    return 0;
}

// byte offsets of the window's LDS regions (16-byte aligned); only for rows scw_check accepted
static __host__ __device__ inline ScwLayout scw_layout(int hs, int ws, int h, int wl, int w, int mask) {
    ScwLayout g;
    int o = 0;
    auto take = [&o](int bytes) { const int at = o; o += (bytes + 15) & ~15; return at; };
    g.ksh = ws == wl ? 0 : col_ksize(ws, wl);
    g.ksv = hs == h ? 0 : col_ksize(hs, h);
    g.kh = take(w * g.ksh * 4);
    g.bh = take(g.ksh ? w * 8 : 0);
    g.kv = take(h * g.ksv * 4);
    g.bv = take(g.ksv ? h * 8 : 0);
    g.lum = take(mask ? h * w : 0);
    g.inter = take(g.ksh ? hs * w * 3 : 0);
    g.red = take(mask ? (SCW_THREADS / 64) * 4 : 0);
    g.total = o;
    return g;
}

// the vertical pass over the window's h * w pixels from s1 = uint8 rows `row_bytes` apart whose pixel 0 is the window's first column (the
// box in the image, or the horizontal pass's result); returns this thread's share of sum(L)
__device__ __forceinline__ int scw_vertical(const unsigned char* __restrict__ s1, long row_bytes, const int* kv, const int* bv, int ksv,
                                            int h, int w, float* __restrict__ out, unsigned char* lum, int tid) {
    const int N = h * w;
    int lsum = 0;
    for (int i = tid; i < N; i += SCW_THREADS) {
        const int y = i / w, x = i - y * w;
        int r, g, b;
        if (ksv) {
            const int ymin = bv[2 * y], n = bv[2 * y + 1];
            const int* k = kv + y * ksv;
            const unsigned char* p = s1 + ymin * row_bytes + x * 3;
            int a0 = 1 << (COL_PB - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < n; ++t, p += row_bytes) {
                const int kt = k[t];
                a0 += p[0] * kt;
                a1 += p[1] * kt;
                a2 += p[2] * kt;
            }
            r = col_clip8(a0), g = col_clip8(a1), b = col_clip8(a2);
        } else {
            const unsigned char* p = s1 + y * row_bytes + x * 3;
            r = p[0], g = p[1], b = p[2];
        }
        out[i] = __fdiv_rn((float)r, 255.f);
        out[N + i] = __fdiv_rn((float)g, 255.f);
        out[2 * N + i] = __fdiv_rn((float)b, 255.f);
        if (lum) {
            const int L = (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16;
            lum[i] = (unsigned char)L;
            lsum += L;
        }
    }
    return lsum;
}

__global__ __launch_bounds__(SCW_THREADS) void scene_windows_kernel(const unsigned char* __restrict__ packed, long packed_bytes,
                                                                    const int* __restrict__ desc, float* __restrict__ out_base,
                                                                    long out_floats, int lds_bytes) {
    extern __shared__ __align__(16) unsigned char scw_lds[];
    const int tid = threadIdx.x;
    const int* d = desc + (long)blockIdx.x * SCW_DESC;
    const int hs = d[1], ws = d[2], h = d[3], wl = d[4], x0 = d[5], w = d[6], mask = d[7] != 0, out_off = d[8];
    // The host entry refuses such rows before it launches; a replayed launch re-checks so that a stale row cannot reach outside the
    // buffers: the window's planes (when they lie inside) are filled with NaN, nothing else is touched.
    const long N = (long)h * w, planes = 3 + mask;
    if (h < 1 || w < 1 || h > SCW_MAX_H || w > SCW_MAX_W || out_off < 0 || out_off + planes * N > out_floats) return;
    float* out = out_base + out_off;
    const bool ok = scw_check(d, packed_bytes, out_floats) == 0;
    const ScwLayout g = ok ? scw_layout(hs, ws, h, wl, w, mask) : ScwLayout{};
    if (!ok || g.total > lds_bytes) {
        for (long i = tid; i < planes * N; i += SCW_THREADS) out[i] = __builtin_nanf("");
        return;
    }
    const long pitch = d[9];
    const unsigned char* src = packed + d[0] + (long)d[11] * pitch + 3L * d[10];          // the box's first pixel
    int* kh = (int*)(scw_lds + g.kh);
    int* bh = (int*)(scw_lds + g.bh);
    int* kv = (int*)(scw_lds + g.kv);
    int* bv = (int*)(scw_lds + g.bv);
    unsigned char* lum = mask ? scw_lds + g.lum : nullptr;
    unsigned char* inter = scw_lds + g.inter;
    int* red = (int*)(scw_lds + g.red);

    // phase 0: row x0 + i of the box's horizontal table lands in row i of the window's (col_coeffs indexes by the line's column)
    const int nh = g.ksh ? w : 0, nv = g.ksv ? h : 0;
    for (int i = tid; i < nh + nv; i += SCW_THREADS) {
        if (i < nh) col_coeffs(x0 + i, ws, wl, g.ksh, kh - (long)x0 * g.ksh, bh - 2L * x0);
        else col_coeffs(i - nh, hs, h, g.ksv, kv, bv);
    }
    if (nh + nv) __syncthreads();

    // phase 1: the horizontal pass for the window's w columns
    if (g.ksh) {
        const int n1 = hs * w;
        for (int i = tid; i < n1; i += SCW_THREADS) {
            const int yy = i / w, xx = i - yy * w;
            const int xmin = bh[2 * xx], n = bh[2 * xx + 1];
            const int* k = kh + xx * g.ksh;
            const unsigned char* p = src + yy * pitch + xmin * 3;
            int a0 = 1 << (COL_PB - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < n; ++x, p += 3) {
                const int kx = k[x];
                a0 += p[0] * kx;
                a1 += p[1] * kx;
                a2 += p[2] * kx;
            }
            inter[i * 3] = (unsigned char)col_clip8(a0);
            inter[i * 3 + 1] = (unsigned char)col_clip8(a1);
            inter[i * 3 + 2] = (unsigned char)col_clip8(a2);
        }
        __syncthreads();
    }

    // phase 2 (two call sites: the source pointer is LDS in one and global memory in the other)
    int lsum = g.ksh ? scw_vertical(inter, 3L * w, kv, bv, g.ksv, h, w, out, lum, tid)
                     : scw_vertical(src + (long)x0 * 3, pitch, kv, bv, g.ksv, h, w, out, lum, tid);
    if (!mask) return;

    // phase 3: the window's own mask plane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = lsum;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int i = 0; i < SCW_THREADS / 64; ++i) total += red[i];
    const int n = (int)N;
    for (int i = tid; i < n; i += SCW_THREADS) out[3 * n + i] = (int)lum[i] * n <= total ? 1.f : 0.f;
}

TATT_API int tatt_scene_windows(const unsigned char* packed, long packed_bytes, const int* desc, const int* desc_host, int n_windows,
                                float* out, long out_floats, hipStream_t st) {
    if (!packed || !desc || !desc_host || !out || n_windows <= 0 || packed_bytes <= 0 || out_floats <= 0) return 1;
    int lds = 0;
    for (int i = 0; i < n_windows; ++i) {
        const int* d = desc_host + (long)i * SCW_DESC;
        const int rc = scw_check(d, packed_bytes, out_floats);
        if (rc) return rc;
        const int total = scw_layout(d[1], d[2], d[3], d[4], d[6], d[7] != 0).total;
        if (total > SCW_LDS) return 2;
        if (total > lds) lds = total;
    }
    static TattPerDevice attr_once;                 // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scene_windows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SCW_LDS);
    });
    hipLaunchKernelGGL(scene_windows_kernel, dim3(n_windows), dim3(SCW_THREADS), (size_t)lds, st, packed, packed_bytes, desc, out,
                       out_floats, lds);
    return LAUNCH_CHECK();
}

// ---- the tiled resampler ---------------------------------------------------------------------------------------------------------------
#define RSZ_THREADS 256
#define RSZ_DESC 16                    // ints per item row: src byte offset, H_src, W_src, src pitch, dst byte offset, OH, OW, dst pitch, feather, 0 x 7
#define RSZ_TH 32                      // tile height (halved for steep vertical down-scales: rsz_layout)
#define RSZ_TW 64                      // tile width
#define RSZ_MAX_DOWN 16                // largest in / out per axis (ksize <= 65)
#define RSZ_MAX_SIDE 32768             // largest side of a source or a target
#define RSZ_MAX_FEATHER 4096
#define RSZ_INTER_ROWS 192             // rows of the horizontal pass's result a tile keeps in LDS
#define RSZ_MAX_ITEMS 65535            // grid.y
#define SCN_MAX_BOXES 4096             // boxes of one scene (scene.py refuses more before anything is planned)
#define RSZ_LDS 65536                  // no tile needs more (see the head of the file)

struct RszLayout { int ksh, ksv, th, span, kh, bh, kv, bv, inter, total; };

// 0: the row is taken; 1: a reserved word is set or the feather is negative; 2: geometry beyond tatt_scene_limits; 3: the source or the
// target rectangle leaves its buffer
static __host__ __device__ inline int rsz_check(const int* d, long src_bytes, long dst_bytes) {
    const int so = d[0], hs = d[1], ws = d[2], sp = d[3], dof = d[4], oh = d[5], ow = d[6], dp = d[7], f = d[8];
    for (int i = 9; i < RSZ_DESC; ++i)
        if (d[i] != 0) return 1;
    if (f < 0) return 1;
    if (hs < 1 || ws < 1 || oh < 1 || ow < 1 || hs > RSZ_MAX_SIDE || ws > RSZ_MAX_SIDE || oh > RSZ_MAX_SIDE || ow > RSZ_MAX_SIDE) return 2;
    if (hs > (long)RSZ_MAX_DOWN * oh || ws > (long)RSZ_MAX_DOWN * ow || f > RSZ_MAX_FEATHER) return 2;
    if (so < 0 || sp < 3L * ws || so + (long)(hs - 1) * sp + 3L * ws > src_bytes) return 3;
    if (dof < 0 || dp < 3L * ow || dof + (long)(oh - 1) * dp + 3L * ow > dst_bytes) return 3;
    return 0;
}

// an upper bound of the source samples that n consecutive output samples of a pass in -> out name: the first one starts no lower than
// center0 - support - 0.5, the last one ends no higher than center0 + (n - 1) * scale + support + 0.5 (col_coeffs)
static __host__ __device__ inline int rsz_span(int in, int out, int n) {
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    const long s = (long)ceil((n - 1) * scale + 4.0 * fs) + 2;
    return s > in ? in : (int)s;
}

// tile height and LDS regions of an item (16-byte aligned); only for rows rsz_check accepted
static __host__ __device__ inline RszLayout rsz_layout(int hs, int ws, int oh, int ow) {
    RszLayout g;
    int o = 0;
    auto take = [&o](int bytes) { const int at = o; o += (bytes + 15) & ~15; return at; };
    g.ksh = ws == ow ? 0 : col_ksize(ws, ow);
    g.ksv = hs == oh ? 0 : col_ksize(hs, oh);
    g.th = RSZ_TH;
    if (g.ksv)
        while (g.th > 1 && rsz_span(hs, oh, g.th) > RSZ_INTER_ROWS) g.th >>= 1;
    g.span = g.ksv ? rsz_span(hs, oh, g.th) : g.th;
    g.kh = take(RSZ_TW * g.ksh * 4);
    g.bh = take(g.ksh ? RSZ_TW * 8 : 0);
    g.kv = take(g.th * g.ksv * 4);
    g.bv = take(g.ksv ? g.th * 8 : 0);
    g.inter = take(g.ksh ? g.span * RSZ_TW * 3 : 0);
    g.total = o;
    return g;
}

static __host__ __device__ inline long rsz_tiles(int oh, int ow, int th) { return (long)((oh + th - 1) / th) * ((ow + RSZ_TW - 1) / RSZ_TW); }

// phase 2 of one tile: s1 = uint8 rows `row_bytes` apart, row 0 = source row `r0`, pixel 0 = the tile's first column (LDS or global)
__device__ __forceinline__ void rsz_column(const unsigned char* s1, long row_bytes, int r0, const int* kv, const int* bv, int ksv,
                                           int y0, int x0, int tn, int tw, int oh, int ow, int f, unsigned char* dst, long dp, int tid) {
    const int n2 = tn * tw, D = f + 1;
    for (int i = tid; i < n2; i += RSZ_THREADS) {
        const int y = i / tw, x = i - y * tw;
        int r, g, b;
        if (ksv) {
            const int ymin = bv[2 * y], n = bv[2 * y + 1];
            const int* k = kv + y * ksv;
            const unsigned char* p = s1 + (ymin - r0) * row_bytes + x * 3;
            int a0 = 1 << (COL_PB - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < n; ++t, p += row_bytes) {
                const int kt = k[t];
                a0 += p[0] * kt;
                a1 += p[1] * kt;
                a2 += p[2] * kt;
            }
            r = col_clip8(a0), g = col_clip8(a1), b = col_clip8(a2);
        } else {
            const unsigned char* p = s1 + (y0 + y - r0) * row_bytes + x * 3;
            r = p[0], g = p[1], b = p[2];
        }
        const int Y = y0 + y, X = x0 + x;
        unsigned char* q = dst + Y * dp + X * 3L;
        if (f > 0) {                                                 // feather: weight a / D of the new pixel, rounded half up
            const int a = min(min(min(Y, oh - 1 - Y), min(X, ow - 1 - X)), f) + 1;
            if (a < D) {
                r = (2 * (a * r + (D - a) * q[0]) + D) / (2 * D);
                g = (2 * (a * g + (D - a) * q[1]) + D) / (2 * D);
                b = (2 * (a * b + (D - a) * q[2]) + D) / (2 * D);
            }
        }
        q[0] = (unsigned char)r;
        q[1] = (unsigned char)g;
        q[2] = (unsigned char)b;
    }
}

// (src_base and dst_base may be one buffer: the line canvases and the scene canvas of a paste; the rectangles of a launch are disjoint)
__global__ __launch_bounds__(RSZ_THREADS) void resize_u8_kernel(const unsigned char* src_base, long src_bytes, const int* __restrict__ desc,
                                                                unsigned char* dst_base, long dst_bytes, int lds_bytes) {
    extern __shared__ __align__(16) unsigned char rsz_lds[];
    const int tid = threadIdx.x;
    const int* d = desc + (long)blockIdx.y * RSZ_DESC;
    // a replayed launch re-checks: nothing is written for a row the host entry would have refused
    if (rsz_check(d, src_bytes, dst_bytes) != 0) return;
    const int hs = d[1], ws = d[2], oh = d[5], ow = d[6], f = d[8];
    const long sp = d[3], dp = d[7];
    const RszLayout g = rsz_layout(hs, ws, oh, ow);
    if (g.total > lds_bytes || (long)blockIdx.x >= rsz_tiles(oh, ow, g.th)) return;
    const int tiles_x = (ow + RSZ_TW - 1) / RSZ_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * g.th, x0 = tx * RSZ_TW;
    const int tn = min(g.th, oh - y0), tw = min(RSZ_TW, ow - x0);
    const unsigned char* src = src_base + d[0];
    unsigned char* dst = dst_base + d[4];
    int* kh = (int*)(rsz_lds + g.kh);
    int* bh = (int*)(rsz_lds + g.bh);
    int* kv = (int*)(rsz_lds + g.kv);
    int* bv = (int*)(rsz_lds + g.bv);
    unsigned char* inter = rsz_lds + g.inter;

    // phase 0: rows x0 .. x0 + tw - 1 and y0 .. y0 + tn - 1 of the two tables land in rows 0 .. of the tile's
    const int nh = g.ksh ? tw : 0, nv = g.ksv ? tn : 0;
    for (int i = tid; i < nh + nv; i += RSZ_THREADS) {
        if (i < nh) col_coeffs(x0 + i, ws, ow, g.ksh, kh - (long)x0 * g.ksh, bh - 2L * x0);
        else col_coeffs(y0 + i - nh, hs, oh, g.ksv, kv - (long)y0 * g.ksv, bv - 2L * y0);
    }
    if (nh + nv) __syncthreads();

    // the source rows the tile reads: first sample of its first output row .. last sample of its last one (both increase with the row)
    const int r0 = g.ksv ? bv[0] : y0;
    const int nr = g.ksv ? bv[2 * (tn - 1)] + bv[2 * (tn - 1) + 1] - r0 : tn;
    if (g.ksh && nr > g.span) return;                                // (rsz_span bounds it: never taken, and the same in every thread)

    // phase 1
    if (g.ksh) {
        const int n1 = nr * tw;
        for (int i = tid; i < n1; i += RSZ_THREADS) {
            const int yy = i / tw, xx = i - yy * tw;
            const int xmin = bh[2 * xx], n = bh[2 * xx + 1];
            const int* k = kh + xx * g.ksh;
            const unsigned char* p = src + (r0 + yy) * sp + xmin * 3L;
            int a0 = 1 << (COL_PB - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < n; ++x, p += 3) {
                const int kx = k[x];
                a0 += p[0] * kx;
                a1 += p[1] * kx;
                a2 += p[2] * kx;
            }
            unsigned char* q = inter + (yy * RSZ_TW + xx) * 3;
            q[0] = (unsigned char)col_clip8(a0);
            q[1] = (unsigned char)col_clip8(a1);
            q[2] = (unsigned char)col_clip8(a2);
        }
        __syncthreads();
    }

    // phase 2 (two call sites: the source pointer is LDS in one and global memory in the other)
    if (g.ksh) rsz_column(inter, RSZ_TW * 3L, r0, kv, bv, g.ksv, y0, x0, tn, tw, oh, ow, f, dst, dp, tid);
    else rsz_column(src + x0 * 3L, sp, 0, kv, bv, g.ksv, y0, x0, tn, tw, oh, ow, f, dst, dp, tid);
}

TATT_API int tatt_resize_u8(const unsigned char* src, long src_bytes, const int* desc, const int* desc_host, int n_items,
                            unsigned char* dst, long dst_bytes, hipStream_t st) {
    if (!src || !desc || !desc_host || !dst || n_items <= 0 || src_bytes <= 0 || dst_bytes <= 0) return 1;
    if (n_items > RSZ_MAX_ITEMS) return 2;
    int lds = 0;
    long tiles = 0;
    for (int i = 0; i < n_items; ++i) {
        const int* d = desc_host + (long)i * RSZ_DESC;
        const int rc = rsz_check(d, src_bytes, dst_bytes);
        if (rc) return rc;
        const RszLayout g = rsz_layout(d[1], d[2], d[5], d[6]);
        if (g.total > RSZ_LDS) return 2;
        if (g.total > lds) lds = g.total;
        const long t = rsz_tiles(d[5], d[6], g.th);
        if (t > tiles) tiles = t;
    }
    if (tiles > 0x7fffffffL) return 2;
    hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)tiles, n_items), dim3(RSZ_THREADS), (size_t)lds, st, src, src_bytes, desc, dst,
                       dst_bytes, lds);
    return LAUNCH_CHECK();
}

TATT_API int tatt_scene_limits(int* out) {
    if (!out) return 1;
    out[0] = RSZ_MAX_SIDE;
    out[1] = SCN_MAX_BOXES;
    out[2] = RSZ_TH;
    out[3] = RSZ_TW;
    out[4] = RSZ_MAX_DOWN;
    out[5] = RSZ_MAX_FEATHER;
    out[6] = RSZ_INTER_ROWS;
    out[7] = RSZ_MAX_ITEMS;
    return 0;
}
