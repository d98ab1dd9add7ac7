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
// Both kernels are a descriptor row, its check and a body of pil_resample.h: scene_windows_kernel runs pil_window_body from the box's
// first pixel with the image's row pitch; resize_u8_kernel, grid (tile, item), 256 threads, runs pil_tile_body (one tile of th x 64
// output pixels per work-group, LDS bounded whatever the factor) and clips, feathers and stores the pixel it is handed (a wave writes
// 192 contiguous bytes of a canvas row).
#include "common.h"
#include "pil_resample.h"         // pil_win_layout, pil_window_body; pil_tile_layout, pil_tiles, pil_tile_body
#include "line_limits.h"          // LIN_* limits, lin_takes (shared with lines.hip)

// ---- windows of boxes ------------------------------------------------------------------------------------------------------------------
#define SCW_DESC 16                    // ints per window row: lines.hip's words 0 .. 8, [9] row pitch in bytes, [10] box x, [11] box y, [12..15] 0

// 0: the row is taken; 1: a reserved word is set; 2: geometry beyond tatt_line_limits; 3: the box or the planes leave packed / out
static __host__ __device__ inline int scw_check(const int* d, long packed_bytes, long out_floats) {
    const int off = d[0], hs = d[1], ws = d[2], h = d[3], wl = d[4], x0 = d[5], w = d[6], out_off = d[8], pitch = d[9], bx = d[10], by = d[11];
    if (d[12] != 0 || d[13] != 0 || d[14] != 0 || d[15] != 0) return 1;
    if (!lin_takes(hs, ws, h, wl, x0, w)) return 2;
    if (off < 0 || bx < 0 || by < 0 || pitch < 3L * ((long)bx + ws)) return 3;
    if (off + ((long)by + hs - 1) * pitch + 3L * ((long)bx + ws) > packed_bytes) return 3;
    if (out_off < 0 || out_off + (long)(3 + (d[7] != 0)) * h * w > out_floats) return 3;
    return 0;
}

__global__ __launch_bounds__(LIN_THREADS) void scene_windows_kernel(const unsigned char* __restrict__ packed, long packed_bytes,
                                                                    const int* __restrict__ desc, float* __restrict__ out_base,
                                                                    long out_floats, int lds_bytes) {
    extern __shared__ __align__(16) unsigned char scw_lds[];
    const int tid = threadIdx.x;
    const int* d = desc + (long)blockIdx.x * SCW_DESC;
    const int hs = d[1], ws = d[2], h = d[3], wl = d[4], x0 = d[5], w = d[6], mask = d[7] != 0, out_off = d[8];
    // The host entry refuses such rows before it launches; a replayed launch re-checks so that a stale row cannot reach outside the
    // buffers: the window's planes (when they lie inside) are filled with NaN, nothing else is touched.
    const long N = (long)h * w, planes = 3 + mask;
    if (h < 1 || w < 1 || h > LIN_MAX_H || w > LIN_MAX_W || out_off < 0 || out_off + planes * N > out_floats) return;
    float* out = out_base + out_off;
    const bool ok = scw_check(d, packed_bytes, out_floats) == 0;
    const PilWinLayout g = ok ? pil_win_layout<LIN_THREADS>(hs, ws, h, wl, w, mask) : PilWinLayout{};
    if (!ok || g.total > lds_bytes) return pil_win_refuse<LIN_THREADS>(out, planes * N, tid);
    const long pitch = d[9];
    const unsigned char* box = packed + d[0] + (long)d[11] * pitch + 3L * d[10];          // the box's first pixel
    pil_window_body<LIN_THREADS>(box, pitch, g, scw_lds, hs, ws, h, wl, x0, w, mask, out, tid);
}

TATT_API int tatt_scene_windows(const unsigned char* packed, long packed_bytes, const int* desc, const int* desc_host, int n_windows,
                                float* out, long out_floats, hipStream_t st) {
    if (!packed || !desc || !desc_host || !out || n_windows <= 0 || packed_bytes <= 0 || out_floats <= 0) return 1;
    int lds = 0;
    for (int i = 0; i < n_windows; ++i) {
        const int* d = desc_host + (long)i * SCW_DESC;
        const int rc = scw_check(d, packed_bytes, out_floats);
        if (rc) return rc;
        const int total = pil_win_layout<LIN_THREADS>(d[1], d[2], d[3], d[4], d[6], d[7] != 0).total;
        if (total > LIN_LDS) return 2;
        if (total > lds) lds = total;
    }
    static TattPerDevice attr_once;                 // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scene_windows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LIN_LDS);
    });
    hipLaunchKernelGGL(scene_windows_kernel, dim3(n_windows), dim3(LIN_THREADS), (size_t)lds, st, packed, packed_bytes, desc, out,
                       out_floats, lds);
    return LAUNCH_CHECK();
}

// ---- the tiled resampler ---------------------------------------------------------------------------------------------------------------
#define RSZ_THREADS 256
#define RSZ_DESC 16                    // ints per item row: src byte offset, H_src, W_src, src pitch, dst byte offset, OH, OW, dst pitch, feather, 0 x 7
#define RSZ_MAX_DOWN 16                // largest in / out per axis (ksize <= 65)
#define RSZ_MAX_SIDE 32768             // largest side of a source or a target
#define RSZ_MAX_FEATHER 4096
#define RSZ_MAX_ITEMS 65535            // grid.y
#define SCN_MAX_BOXES 4096             // boxes of one scene (scene.py refuses more before anything is planned)
#define RSZ_LDS 65536                  // no tile needs more (pil_resample.h: under 58 KB)

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

// (src_base and dst_base may be one buffer: the line canvases and the scene canvas of a paste; the rectangles of a launch are disjoint)
__global__ __launch_bounds__(RSZ_THREADS) void resize_u8_kernel(const unsigned char* src_base, long src_bytes, const int* __restrict__ desc,
                                                                unsigned char* dst_base, long dst_bytes, int lds_bytes) {
    extern __shared__ __align__(16) unsigned char rsz_lds[];
    const int* d = desc + (long)blockIdx.y * RSZ_DESC;
    // a replayed launch re-checks: nothing is written for a row the host entry would have refused
    if (rsz_check(d, src_bytes, dst_bytes) != 0) return;
    const int hs = d[1], ws = d[2], oh = d[5], ow = d[6], f = d[8], D = f + 1;
    const long dp = d[7];
    const PilTileLayout g = pil_tile_layout(hs, ws, oh, ow);
    if (g.total > lds_bytes || (long)blockIdx.x >= pil_tiles(oh, ow, g.th)) return;
    unsigned char* dst = dst_base + d[4];
    pil_tile_body<RSZ_THREADS>(src_base + d[0], d[3], g, rsz_lds, hs, ws, oh, ow, blockIdx.x, threadIdx.x, [&](int Y, int X, int r, int gg, int b) {
        unsigned char* q = dst + Y * dp + X * 3L;
        if (f > 0) {                                                 // feather: weight a / D of the new pixel, rounded half up
            const int a = min(min(min(Y, oh - 1 - Y), min(X, ow - 1 - X)), f) + 1;
            if (a < D) {
                r = (2 * (a * r + (D - a) * q[0]) + D) / (2 * D);
                gg = (2 * (a * gg + (D - a) * q[1]) + D) / (2 * D);
                b = (2 * (a * b + (D - a) * q[2]) + D) / (2 * D);
            }
        }
        q[0] = (unsigned char)r;
        q[1] = (unsigned char)gg;
        q[2] = (unsigned char)b;
    });
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
        const PilTileLayout g = pil_tile_layout(d[1], d[2], d[5], d[6]);
        if (g.total > RSZ_LDS) return 2;
        if (g.total > lds) lds = g.total;
        const long t = pil_tiles(d[5], d[6], g.th);
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
    out[2] = PIL_TILE_H;
    out[3] = PIL_TILE_W;
    out[4] = RSZ_MAX_DOWN;
    out[5] = RSZ_MAX_FEATHER;
    out[6] = PIL_TILE_INTER_ROWS;
    out[7] = RSZ_MAX_ITEMS;
    return 0;
}
