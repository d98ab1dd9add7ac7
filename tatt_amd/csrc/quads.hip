// Scene images with quadrilateral text boxes (tatt_amd/quads.py is the specification, tests/test_quads*.py hold the kernel to it).  ONE
// kernel, used twice: a projective warp of uint8 RGB in device memory to uint8 RGB in device memory with a two-tap sampler per axis,
//   mode 0  rectify: the scene -> the upright crop of a quad, every destination pixel written;
//   mode 1  paste: the finished line -> the quad's bounding box of the canvas, only the pixels whose source point lies inside the line
//           painted, feathered by the distance to the line's nearest side against what the canvas holds.
// warp_u8_kernel, grid (tile, item), 256 threads, one thread per destination pixel of a tile of 8 x 32.  Per pixel (i, j), with J = 2 j + 1,
// I = 2 i + 1 and the item's nine 64-bit matrix entries:
//   X = m00 J + m01 I + m02, Y = m10 J + m11 I + m12, Wd = m20 J + m21 I + m22;  gx = floor(256 X / Wd), gy = floor(256 Y / Wd)
//   fx = gx - 128: x0 = fx >> 8, ax = fx & 255 (fy alike); the four taps clamped to the source; the bilinear sum rounded at 2^15 >> 16.
// All of it is 64-bit integer arithmetic with true floor division (two emulated 64-bit divisions per pixel: the kernel's known cost), no
// floating point anywhere, so the result equals `warp_u8_host` byte for byte.  No traffic between work-groups, no atomics, no LDS: the taps
// are uint8 gathers served by the L2.  Every quantity is read from DEVICE memory (the launch can be captured); the same check runs on the
// host before the launch and in the kernel, every tap is clamped, every store lies in a rectangle the check accepted.
#include "common.h"

#define WRP_THREADS 256
#define WRP_DESC 32                    // ints per item row: src byte offset, H_src, W_src, src pitch, dst byte offset, OH, OW, dst pitch, feather,
                                       // mode, m00 lo, m00 hi, .. m22 lo, m22 hi (row-major), 0 x 4
#define WRP_TH 8                       // tile height
#define WRP_TW 32                      // tile width
#define WRP_MAX_SIDE 32768             // largest side of a source or a target
#define WRP_MAX_FEATHER 4096
#define WRP_MAX_ITEMS 65535            // grid.y

// 0: the row is taken; 1: a reserved word is set, the feather is negative or the mode unknown; 2: geometry beyond tatt_quad_limits; 3: the
// source or the target rectangle leaves its buffer
static __host__ __device__ inline int wrp_check(const int* d, long src_bytes, long dst_bytes) {
    const int so = d[0], hs = d[1], ws = d[2], sp = d[3], dof = d[4], oh = d[5], ow = d[6], dp = d[7], f = d[8], mode = d[9];
    for (int i = 28; i < WRP_DESC; ++i)
        if (d[i] != 0) return 1;
    if (f < 0 || (mode != 0 && mode != 1)) return 1;
    if (hs < 1 || ws < 1 || oh < 1 || ow < 1 || hs > WRP_MAX_SIDE || ws > WRP_MAX_SIDE || oh > WRP_MAX_SIDE || ow > WRP_MAX_SIDE) return 2;
    if (f > WRP_MAX_FEATHER) return 2;
    if (so < 0 || sp < 3L * ws || so + (long)(hs - 1) * sp + 3L * ws > src_bytes) return 3;
    if (dof < 0 || dp < 3L * ow || dof + (long)(oh - 1) * dp + 3L * ow > dst_bytes) return 3;
    return 0;
}

static __host__ __device__ inline long wrp_tiles(int oh, int ow) { return (long)((oh + WRP_TH - 1) / WRP_TH) * ((ow + WRP_TW - 1) / WRP_TW); }

// matrix entry k of a row (two's complement, low word first); the sums below wrap like the host yardstick's int64 for a matrix no plan
// would pass (computed unsigned: no signed overflow)
static __host__ __device__ inline unsigned long wrp_entry(const int* d, int k) {
    return (unsigned long)(unsigned)d[10 + 2 * k] | ((unsigned long)(unsigned)d[11 + 2 * k] << 32);
}

// floor(n / d) for d > 0
static __host__ __device__ inline long wrp_floor_div(long n, long d) {
    const long q = n / d;
    return (n % d < 0) ? q - 1 : q;
}

static __host__ __device__ inline int wrp_clamp(long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }
static __host__ __device__ inline int wrp_min(int a, int b) { return a < b ? a : b; }

// destination pixel (i, j) of a row wrp_check accepted: src the source's first pixel, q the destination pixel's three bytes
static __host__ __device__ inline void wrp_pixel(const int* d, const unsigned char* src, int i, int j, unsigned char* q) {
    const int hs = d[1], ws = d[2], f = d[8], mode = d[9];
    const long sp = d[3];
    const unsigned long J = 2UL * j + 1, I = 2UL * i + 1;
    const long X = (long)(wrp_entry(d, 0) * J + wrp_entry(d, 1) * I + wrp_entry(d, 2));
    const long Y = (long)(wrp_entry(d, 3) * J + wrp_entry(d, 4) * I + wrp_entry(d, 5));
    const long Wd = (long)(wrp_entry(d, 6) * J + wrp_entry(d, 7) * I + wrp_entry(d, 8));
    if (Wd <= 0) {                                                   // beyond the horizon: outside
        if (mode == 0) q[0] = q[1] = q[2] = 0;
        return;
    }
    const long gx = wrp_floor_div((long)((unsigned long)X << 8), Wd), gy = wrp_floor_div((long)((unsigned long)Y << 8), Wd);
    if (mode == 1 && (gx < 0 || gx >= 256L * ws || gy < 0 || gy >= 256L * hs)) return;
    const long fx = gx - 128, fy = gy - 128;
    const long x0 = fx >> 8, y0 = fy >> 8;
    const int ax = (int)(fx & 255), ay = (int)(fy & 255);
    const int xa = wrp_clamp(x0, ws - 1), xb = wrp_clamp(x0 + 1, ws - 1), ya = wrp_clamp(y0, hs - 1), yb = wrp_clamp(y0 + 1, hs - 1);
    const unsigned char* r0 = src + ya * sp;
    const unsigned char* r1 = src + yb * sp;
    const unsigned char *p00 = r0 + xa * 3, *p01 = r0 + xb * 3, *p10 = r1 + xa * 3, *p11 = r1 + xb * 3;
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int top = (256 - ax) * p00[c] + ax * p01[c], bot = (256 - ax) * p10[c] + ax * p11[c];
        v[c] = ((256 - ay) * top + ay * bot + 32768) >> 16;
    }
    if (mode == 1 && f > 0) {                                        // feather: weight a / D of the new pixel, rounded half up
        const int xi = (int)(gx >> 8), yi = (int)(gy >> 8), D = f + 1;
        const int a = wrp_min(wrp_min(wrp_min(xi, ws - 1 - xi), wrp_min(yi, hs - 1 - yi)), f) + 1;
        if (a < D) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (2 * (a * v[c] + (D - a) * q[c]) + D) / (2 * D);
        }
    }
    q[0] = (unsigned char)v[0];
    q[1] = (unsigned char)v[1];
    q[2] = (unsigned char)v[2];
}

// tile t of an oh x ow destination, thread tid -> its pixel (i, j); false beyond the destination
static __host__ __device__ inline bool wrp_place(long t, int tid, int oh, int ow, int* i, int* j) {
    if (t >= wrp_tiles(oh, ow)) return false;
    const int tiles_x = (ow + WRP_TW - 1) / WRP_TW;
    const int ty = (int)(t / tiles_x), tx = (int)(t - (long)ty * tiles_x);
    *i = ty * WRP_TH + tid / WRP_TW;
    *j = tx * WRP_TW + tid % WRP_TW;
    return *i < oh && *j < ow;
}

// (src_base and dst_base may be one buffer: the scene and its crops, the line rectangles and the canvas; the targets of a launch are
// disjoint and overlap no source)
__global__ __launch_bounds__(WRP_THREADS) void warp_u8_kernel(const unsigned char* src_base, long src_bytes, const int* __restrict__ desc,
                                                              unsigned char* dst_base, long dst_bytes) {
    const int* d = desc + (long)blockIdx.y * WRP_DESC;
    // a replayed launch re-checks: nothing is written for a row the host entry would have refused
    if (wrp_check(d, src_bytes, dst_bytes) != 0) return;
    int i, j;
    if (!wrp_place(blockIdx.x, (int)threadIdx.x, d[5], d[6], &i, &j)) return;
    wrp_pixel(d, src_base + d[0], i, j, dst_base + d[4] + i * (long)d[7] + j * 3L);
}

TATT_API int tatt_warp_u8(const unsigned char* src, long src_bytes, const int* desc, const int* desc_host, int n_items,
                          unsigned char* dst, long dst_bytes, hipStream_t st) {
    if (!src || !desc || !desc_host || !dst || n_items <= 0 || src_bytes <= 0 || dst_bytes <= 0) return 1;
    if (n_items > WRP_MAX_ITEMS) return 2;
    long tiles = 0;
    for (int i = 0; i < n_items; ++i) {
        const int* d = desc_host + (long)i * WRP_DESC;
        const int rc = wrp_check(d, src_bytes, dst_bytes);
        if (rc) return rc;
        const long t = wrp_tiles(d[5], d[6]);
        if (t > tiles) tiles = t;
    }
    if (tiles > 0x7fffffffL) return 2;
    hipLaunchKernelGGL(warp_u8_kernel, dim3((unsigned)tiles, n_items), dim3(WRP_THREADS), 0, st, src, src_bytes, desc, dst, dst_bytes);
    return LAUNCH_CHECK();
}

TATT_API int tatt_quad_limits(int* out) {
    if (!out) return 1;
    out[0] = WRP_TH;
    out[1] = WRP_TW;
    out[2] = WRP_MAX_ITEMS;
    out[3] = WRP_MAX_SIDE;
    out[4] = WRP_MAX_FEATHER;
    out[5] = WRP_DESC;
    return 0;
}
