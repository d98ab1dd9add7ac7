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
// floating point anywhere, so the result equals `warp_u8_host` byte for byte.  The check and the pixel function stand in
// csrc/warp_pixel.h, built from the parts tatt_poly_paste_u8 is built from; the same text runs on the host.  No traffic between
// work-groups, no atomics, no LDS: the taps are uint8 gathers served by the L2.  Every quantity is read from DEVICE memory (the launch can
// be captured); the same check runs on the host before the launch and in the kernel, every tap is clamped, every store lies in a
// rectangle the check accepted.
#include "common.h"
#include "warp_pixel.h"

#define WRP_THREADS 256

// (src_base and dst_base may be one buffer: the scene and its crops, the line rectangles and the canvas; the targets of a launch are
// disjoint and overlap no source)
__global__ __launch_bounds__(WRP_THREADS) void warp_u8_kernel(const unsigned char* src_base, long src_bytes, const int* __restrict__ desc,
                                                              unsigned char* dst_base, long dst_bytes) {
    const int* d = desc + (long)blockIdx.y * WRP_DESC;
    // a replayed launch re-checks: nothing is written for a row the host entry would have refused
    if (wrp_check(d, src_bytes, dst_bytes) != 0) return;
    int i, j;
    if (!warp_place(blockIdx.x, (int)threadIdx.x, d[5], d[6], &i, &j)) return;
    wrp_pixel(d, src_base + d[0], i, j, dst_base + d[4] + i * (long)d[7] + j * 3L);
}

TATT_API int tatt_warp_u8(const unsigned char* src, long src_bytes, const int* desc, const int* desc_host, int n_items,
                          unsigned char* dst, long dst_bytes, hipStream_t st) {
    if (!src || !desc || !desc_host || !dst || n_items <= 0 || src_bytes <= 0 || dst_bytes <= 0) return 1;
    if (n_items > WARP_MAX_ITEMS) return 2;
    long tiles = 0;
    for (int i = 0; i < n_items; ++i) {
        const int* d = desc_host + (long)i * WRP_DESC;
        const int rc = wrp_check(d, src_bytes, dst_bytes);
        if (rc) return rc;
        const long t = warp_tiles(d[5], d[6]);
        if (t > tiles) tiles = t;
    }
    if (tiles > 0x7fffffffL) return 2;
    hipLaunchKernelGGL(warp_u8_kernel, dim3((unsigned)tiles, n_items), dim3(WRP_THREADS), 0, st, src, src_bytes, desc, dst, dst_bytes);
    return LAUNCH_CHECK();
}

TATT_API int tatt_quad_limits(int* out) {
    if (!out) return 1;
    out[0] = WARP_TH;
    out[1] = WARP_TW;
    out[2] = WARP_MAX_ITEMS;
    out[3] = WARP_MAX_SIDE;
    out[4] = WARP_MAX_FEATHER;
    out[5] = WRP_DESC;
    return 0;
}
