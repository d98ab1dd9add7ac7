// The checks and the pixel functions of tatt_warp_u8 (csrc/quads.hip; tatt_amd/quads.py is the specification) and of tatt_poly_paste_u8
// (csrc/polys.hip; tatt_amd/polys.py), built from ONE set of parts: the 64-bit entry decode, the floor division, the tile, the linear
// form of a matrix row at a pixel, the four-tap sample, the feather blend, the front of the row check.  Plain C++ on 64-bit integers, no
// floating point, nothing of the HIP runtime: the same text runs in the kernels, in the host entries and in a stand-alone host program
// under the sanitizers (tools/polys_host).
#pragma once

#ifndef WARP_HD
#define WARP_HD __host__ __device__
#endif

#define WARP_TH 8                      // tile height
#define WARP_TW 32                     // tile width
#define WARP_MAX_SIDE 32768            // largest side of a source, a line or a target
#define WARP_MAX_FEATHER 4096
#define WARP_MAX_ITEMS 65535           // grid.y
#define WRP_DESC 32                    // ints per item row of tatt_warp_u8: src byte offset, H_src, W_src, src pitch, dst byte offset, OH, OW, dst
                                       // pitch, feather, mode, m00 lo, m00 hi, .. m22 lo, m22 hi (row-major), 0 x 4
#define PLY_DESC 16                    // ints per item row of tatt_poly_paste_u8: line byte offset, H, W, line pitch, dst byte offset, OH, OW, dst
                                       // pitch, feather, first strip row, strip count, 0 x 5
#define PLY_STRIP_DESC 32              // ints per strip row: scale U_k, scale w_k, then fifteen 64-bit values as (low, high) words: m00 .. m22
                                       // (row-major), A, B, C of the seam the strip begins at, A, B, C of the seam it ends at
#define PLY_MAX_STRIPS 15              // of one item (the 16 points poly_check takes make 7)

// ---- the parts ------------------------------------------------------------------------------------------------------------------------
// 64-bit value k of a run of (low, high) int32 words (two's complement); the sums below are computed unsigned, so that they wrap like
// the host yardstick's int64 for values no plan would pass
static WARP_HD inline unsigned long warp_entry(const int* w, int k) {
    return (unsigned long)(unsigned)w[2 * k] | ((unsigned long)(unsigned)w[2 * k + 1] << 32);
}

// values 3 k, 3 k + 1, 3 k + 2 of such a run as a linear form at the pixel centre (J, I) = (2 j + 1, 2 i + 1): a matrix row (X, Y, Wd for
// k = 0, 1, 2) or the edge function of a seam
static WARP_HD inline long warp_form(const int* w, int k, unsigned long J, unsigned long I) {
    return (long)(warp_entry(w, 3 * k) * J + warp_entry(w, 3 * k + 1) * I + warp_entry(w, 3 * k + 2));
}

// floor(n / d) for d > 0
static WARP_HD inline long warp_floor_div(long n, long d) {
    const long q = n / d;
    return (n % d < 0) ? q - 1 : q;
}

// gx = floor(256 X / Wd) (gy alike) for Wd > 0
static WARP_HD inline long warp_coord(long V, long Wd) { return warp_floor_div((long)((unsigned long)V << 8), Wd); }

static WARP_HD inline int warp_clamp(long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }
static WARP_HD inline int warp_min(int a, int b) { return a < b ? a : b; }

static WARP_HD inline long warp_tiles(int oh, int ow) { return (long)((oh + WARP_TH - 1) / WARP_TH) * ((ow + WARP_TW - 1) / WARP_TW); }

// tile t of an oh x ow destination, thread tid -> its pixel (i, j); false beyond the destination
static WARP_HD inline bool warp_place(long t, int tid, int oh, int ow, int* i, int* j) {
    if (t >= warp_tiles(oh, ow)) return false;
    const int tiles_x = (ow + WARP_TW - 1) / WARP_TW;
    const int ty = (int)(t / tiles_x), tx = (int)(t - (long)ty * tiles_x);
    *i = ty * WARP_TH + tid / WARP_TW;
    *j = tx * WARP_TW + tid % WARP_TW;
    return *i < oh && *j < ow;
}

// the bilinear sample of an (hs, ws) source of pitch sp at (gx, gy) in 1 / 256 pixels: four taps clamped to the source, rounded at 2^15
static WARP_HD inline void warp_sample(const unsigned char* src, int hs, int ws, long sp, long gx, long gy, int* v) {
    const long fx = (long)((unsigned long)gx - 128UL), fy = gy - 128;
    const long x0 = fx >> 8, y0 = fy >> 8;
    const int ax = (int)(fx & 255), ay = (int)(fy & 255);
    const int xa = warp_clamp(x0, ws - 1), xb = warp_clamp(x0 + 1, ws - 1), ya = warp_clamp(y0, hs - 1), yb = warp_clamp(y0 + 1, hs - 1);
    const unsigned char* r0 = src + ya * sp;
    const unsigned char* r1 = src + yb * sp;
    const unsigned char *p00 = r0 + xa * 3, *p01 = r0 + xb * 3, *p10 = r1 + xa * 3, *p11 = r1 + xb * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int top = (256 - ax) * p00[c] + ax * p01[c], bot = (256 - ax) * p10[c] + ax * p11[c];
        v[c] = ((256 - ay) * top + ay * bot + 32768) >> 16;
    }
}

// the feather f > 0 of the sample v at source pixel (yi, xi) against what q holds: weight a / D of the new pixel, rounded half up
static WARP_HD inline void warp_feather(int hs, int ws, int f, int xi, int yi, const unsigned char* q, int* v) {
    const int D = f + 1;
    const int a = warp_min(warp_min(warp_min(xi, ws - 1 - xi), warp_min(yi, hs - 1 - yi)), f) + 1;
    if (a < D) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (2 * (a * v[c] + (D - a) * q[c]) + D) / (2 * D);
    }
}

static WARP_HD inline void warp_store(unsigned char* q, const int* v) {
    q[0] = (unsigned char)v[0];
    q[1] = (unsigned char)v[1];
    q[2] = (unsigned char)v[2];
}

// The front of the row check.  Words 0 .. 8 of an item row are the same for both kernels (source byte offset, H, W, pitch, target byte
// offset, OH, OW, pitch, feather), its reserved words are [reserved, desc).  Three tests, which wrp_check and ply_check put between their
// own in the order of their refusal codes: no reserved word set and the feather not negative (else 1) ..
static WARP_HD inline bool warp_check_words(const int* d, int reserved, int desc) {
    for (int i = reserved; i < desc; ++i)
        if (d[i] != 0) return false;
    return d[8] >= 0;
}

// .. the four sides within the limits (else 2; the feather's limit, also 2, stays with the callers: from this test alone, returned as it
// stands, the compiler still knows 1 <= OW <= WARP_MAX_SIDE where warp_place divides the tile index, and divides in 32 bits) ..
static WARP_HD inline bool warp_check_sides(const int* d) {
    const int hs = d[1], ws = d[2], oh = d[5], ow = d[6];
    if (hs < 1 || ws < 1 || oh < 1 || ow < 1 || hs > WARP_MAX_SIDE || ws > WARP_MAX_SIDE || oh > WARP_MAX_SIDE || ow > WARP_MAX_SIDE) return false;
    return true;
}

// .. the source and the target rectangle inside their buffers (else 3)
static WARP_HD inline bool warp_check_buffers(const int* d, long src_bytes, long dst_bytes) {
    const int so = d[0], hs = d[1], ws = d[2], sp = d[3], dof = d[4], oh = d[5], ow = d[6], dp = d[7];
    if (so < 0 || sp < 3L * ws || so + (long)(hs - 1) * sp + 3L * ws > src_bytes) return false;
    if (dof < 0 || dp < 3L * ow || dof + (long)(oh - 1) * dp + 3L * ow > dst_bytes) return false;
    return true;
}

// ---- tatt_warp_u8 ---------------------------------------------------------------------------------------------------------------------
// 0: the row is taken; 1: a reserved word is set, the feather is negative or the mode unknown; 2: geometry beyond tatt_quad_limits; 3: the
// source or the target rectangle leaves its buffer
static WARP_HD inline int wrp_check(const int* d, long src_bytes, long dst_bytes) {
    if (!warp_check_words(d, 28, WRP_DESC) || (d[9] != 0 && d[9] != 1)) return 1;
    if (!warp_check_sides(d)) return 2;
    if (d[8] > WARP_MAX_FEATHER) return 2;
    return warp_check_buffers(d, src_bytes, dst_bytes) ? 0 : 3;
}

// destination pixel (i, j) of a row wrp_check accepted: src the source's first pixel, q the destination pixel's three bytes
static WARP_HD inline void wrp_pixel(const int* d, const unsigned char* src, int i, int j, unsigned char* q) {
    const int hs = d[1], ws = d[2], f = d[8], mode = d[9];
    const unsigned long J = 2UL * j + 1, I = 2UL * i + 1;
    const long Wd = warp_form(d + 10, 2, J, I);
    if (Wd <= 0) {                                                   // beyond the horizon: outside
        if (mode == 0) q[0] = q[1] = q[2] = 0;
        return;
    }
    const long gx = warp_coord(warp_form(d + 10, 0, J, I), Wd), gy = warp_coord(warp_form(d + 10, 1, J, I), Wd);
    if (mode == 1 && (gx < 0 || gx >= 256L * ws || gy < 0 || gy >= 256L * hs)) return;
    int v[3];
    warp_sample(src, hs, ws, d[3], gx, gy, v);
    if (mode == 1 && f > 0) warp_feather(hs, ws, f, (int)(gx >> 8), (int)(gy >> 8), q, v);
    warp_store(q, v);
}

// ---- tatt_poly_paste_u8 ---------------------------------------------------------------------------------------------------------------
// 0: the item is taken; 1: a reserved word is set or the feather is negative; 2: geometry beyond tatt_poly_limits (a side, the feather,
// the strip count, a strip's columns outside the line); 3: the line or the target rectangle leaves its buffer; 4: the item's strip rows
// leave the strip table
static WARP_HD inline int ply_check(const int* d, const int* strips, int n_strips, long src_bytes, long dst_bytes) {
    const int ws = d[2], first = d[9], count = d[10];
    if (!warp_check_words(d, 11, PLY_DESC)) return 1;
    if (!warp_check_sides(d)) return 2;
    if (d[8] > WARP_MAX_FEATHER || count < 1 || count > PLY_MAX_STRIPS) return 2;
    if (!warp_check_buffers(d, src_bytes, dst_bytes)) return 3;
    if (first < 0 || (long)first + count > n_strips) return 4;
    for (int s = 0; s < count; ++s) {
        const int* r = strips + (long)(first + s) * PLY_STRIP_DESC;
        if (r[0] < 0 || r[1] < 1 || (long)r[0] + r[1] > ws) return 2;
    }
    return 0;
}

// destination pixel (i, j) of an item ply_check accepted: rows the item's first strip row, src the line's first pixel, q the destination
// pixel's three bytes.  The strips are walked in order; the edge tests (two multiply-adds each) come first, the matrix and the two
// divisions only for a strip whose edge tests pass (Wd, then Y and gy with its test, only then X and gx); the first strip that claims the
// pixel paints it.
static WARP_HD inline void ply_pixel(const int* d, const int* rows, const unsigned char* src, int i, int j, unsigned char* q) {
    const int hs = d[1], ws = d[2], f = d[8], count = d[10];
    const unsigned long J = 2UL * j + 1, I = 2UL * i + 1;
    bool done = false;
    for (int s = 0; s < count; ++s) {                                // (a uniform trip count: the rows stay uniform loads)
        const int* r = rows + (long)s * PLY_STRIP_DESC;
        if (done) continue;
        if (s > 0 && warp_form(r + 2, 3, J, I) < 0) continue;
        if (s < count - 1 && warp_form(r + 2, 4, J, I) >= 0) continue;
        const long Wd = warp_form(r + 2, 2, J, I);
        if (Wd <= 0) continue;                                       // beyond the strip's horizon
        const long gy = warp_coord(warp_form(r + 2, 1, J, I), Wd);
        if (gy < 0 || gy >= 256L * hs) continue;
        const long gx = warp_coord(warp_form(r + 2, 0, J, I), Wd);
        if (s == 0 && gx < 0) continue;                              // the outer sides keep the quad kernel's test
        if (s == count - 1 && gx >= 256L * r[1]) continue;
        done = true;
        // the sample is taken from the WHOLE line (gx of an inner strip is bounded by its seams, not by a test)
        const long gxg = (long)((unsigned long)gx + 256UL * (unsigned long)r[0]);
        int v[3];
        warp_sample(src, hs, ws, d[3], gxg, gy, v);
        // feather against the sides of the WHOLE line: nothing fades at a seam
        if (f > 0) warp_feather(hs, ws, f, warp_clamp(gxg >> 8, ws - 1), (int)(gy >> 8), q, v);
        warp_store(q, v);
    }
}
