// The check and the pixel function of tatt_poly_paste_u8 (csrc/polys.hip; tatt_amd/polys.py is the specification).  Plain C++ on 64-bit
// integers, no floating point, nothing of the HIP runtime: the same text runs in the kernel, in the host entry and in a stand-alone host
// program under the sanitizers.  The bilinear taps and the feather restate wrp_pixel of quads.hip (which stays as it is).
#pragma once

#ifndef PLY_HD
#define PLY_HD __host__ __device__
#endif

#define PLY_DESC 16                    // ints per item row: line byte offset, H, W, line pitch, dst byte offset, OH, OW, dst pitch, feather,
                                       // first strip row, strip count, 0 x 5
#define PLY_STRIP_DESC 32              // ints per strip row: scale U_k, scale w_k, then fifteen 64-bit values as (low, high) words: m00 .. m22
                                       // (row-major), A, B, C of the seam the strip begins at, A, B, C of the seam it ends at
#define PLY_TH 8                       // tile height
#define PLY_TW 32                      // tile width
#define PLY_MAX_SIDE 32768             // largest side of a line or a target
#define PLY_MAX_FEATHER 4096
#define PLY_MAX_ITEMS 65535            // grid.y
#define PLY_MAX_STRIPS 15              // of one item (the 16 points poly_check takes make 7)

// 0: the item is taken; 1: a reserved word is set or the feather is negative; 2: geometry beyond tatt_poly_limits (a side, the feather,
// the strip count, a strip's columns outside the line); 3: the line or the target rectangle leaves its buffer; 4: the item's strip rows
// leave the strip table
static PLY_HD inline int ply_check(const int* d, const int* strips, int n_strips, long src_bytes, long dst_bytes) {
    const int so = d[0], hs = d[1], ws = d[2], sp = d[3], dof = d[4], oh = d[5], ow = d[6], dp = d[7], f = d[8], first = d[9], count = d[10];
    for (int i = 11; i < PLY_DESC; ++i)
        if (d[i] != 0) return 1;
    if (f < 0) return 1;
    if (hs < 1 || ws < 1 || oh < 1 || ow < 1 || hs > PLY_MAX_SIDE || ws > PLY_MAX_SIDE || oh > PLY_MAX_SIDE || ow > PLY_MAX_SIDE) return 2;
    if (f > PLY_MAX_FEATHER || count < 1 || count > PLY_MAX_STRIPS) return 2;
    if (so < 0 || sp < 3L * ws || so + (long)(hs - 1) * sp + 3L * ws > src_bytes) return 3;
    if (dof < 0 || dp < 3L * ow || dof + (long)(oh - 1) * dp + 3L * ow > dst_bytes) return 3;
    if (first < 0 || (long)first + count > n_strips) return 4;
    for (int s = 0; s < count; ++s) {
        const int* r = strips + (long)(first + s) * PLY_STRIP_DESC;
        if (r[0] < 0 || r[1] < 1 || (long)r[0] + r[1] > ws) return 2;
    }
    return 0;
}

static PLY_HD inline long ply_tiles(int oh, int ow) { return (long)((oh + PLY_TH - 1) / PLY_TH) * ((ow + PLY_TW - 1) / PLY_TW); }

// 64-bit value k of a strip row (two's complement, low word first); the sums below are computed unsigned, so that they wrap like the
// host yardstick's int64 for values no plan would pass
static PLY_HD inline unsigned long ply_entry(const int* r, int k) {
    return (unsigned long)(unsigned)r[2 + 2 * k] | ((unsigned long)(unsigned)r[3 + 2 * k] << 32);
}

// floor(n / d) for d > 0
static PLY_HD inline long ply_floor_div(long n, long d) {
    const long q = n / d;
    return (n % d < 0) ? q - 1 : q;
}

static PLY_HD inline int ply_clamp(long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }
static PLY_HD inline int ply_min(int a, int b) { return a < b ? a : b; }

// destination pixel (i, j) of an item ply_check accepted: rows the item's first strip row, src the line's first pixel, q the destination
// pixel's three bytes.  The strips are walked in order; the edge tests (two multiply-adds each) come first, the matrix and the two
// divisions only for a strip whose edge tests pass; the first strip that claims the pixel paints it.
static PLY_HD inline void ply_pixel(const int* d, const int* rows, const unsigned char* src, int i, int j, unsigned char* q) {
    const int hs = d[1], ws = d[2], f = d[8], count = d[10];
    const long sp = d[3];
    const unsigned long J = 2UL * j + 1, I = 2UL * i + 1;
    bool done = false;
    for (int s = 0; s < count; ++s) {                                // (a uniform trip count: the rows stay uniform loads)
        const int* r = rows + (long)s * PLY_STRIP_DESC;
        if (done) continue;
        if (s > 0 && (long)(ply_entry(r, 9) * J + ply_entry(r, 10) * I + ply_entry(r, 11)) < 0) continue;
        if (s < count - 1 && (long)(ply_entry(r, 12) * J + ply_entry(r, 13) * I + ply_entry(r, 14)) >= 0) continue;
        const long Wd = (long)(ply_entry(r, 6) * J + ply_entry(r, 7) * I + ply_entry(r, 8));
        if (Wd <= 0) continue;                                       // beyond the strip's horizon
        const long Y = (long)(ply_entry(r, 3) * J + ply_entry(r, 4) * I + ply_entry(r, 5));
        const long gy = ply_floor_div((long)((unsigned long)Y << 8), Wd);
        if (gy < 0 || gy >= 256L * hs) continue;
        const long X = (long)(ply_entry(r, 0) * J + ply_entry(r, 1) * I + ply_entry(r, 2));
        const long gx = ply_floor_div((long)((unsigned long)X << 8), Wd);
        if (s == 0 && gx < 0) continue;                              // the outer sides keep the quad kernel's test
        if (s == count - 1 && gx >= 256L * r[1]) continue;
        done = true;
        const long gxg = (long)((unsigned long)gx + 256UL * (unsigned long)r[0]);
        const long fx = (long)((unsigned long)gxg - 128UL), fy = gy - 128;   // (gx of an inner strip is bounded by its seams, not by a test)
        const long x0 = fx >> 8, y0 = fy >> 8;
        const int ax = (int)(fx & 255), ay = (int)(fy & 255);
        const int xa = ply_clamp(x0, ws - 1), xb = ply_clamp(x0 + 1, ws - 1), ya = ply_clamp(y0, hs - 1), yb = ply_clamp(y0 + 1, hs - 1);
        const unsigned char* r0 = src + ya * sp;
        const unsigned char* r1 = src + yb * sp;
        const unsigned char *p00 = r0 + xa * 3, *p01 = r0 + xb * 3, *p10 = r1 + xa * 3, *p11 = r1 + xb * 3;
        int v[3];
        for (int c = 0; c < 3; ++c) {
            const int top = (256 - ax) * p00[c] + ax * p01[c], bot = (256 - ax) * p10[c] + ax * p11[c];
            v[c] = ((256 - ay) * top + ay * bot + 32768) >> 16;
        }
        if (f > 0) {                                                 // feather against the sides of the WHOLE line: nothing fades at a seam
            const int xi = ply_clamp(gxg >> 8, ws - 1), yi = (int)(gy >> 8), D = f + 1;
            const int a = ply_min(ply_min(ply_min(xi, ws - 1 - xi), ply_min(yi, hs - 1 - yi)), f) + 1;
            if (a < D) {
                for (int c = 0; c < 3; ++c) v[c] = (2 * (a * v[c] + (D - a) * q[c]) + D) / (2 * D);
            }
        }
        q[0] = (unsigned char)v[0];
        q[1] = (unsigned char)v[1];
        q[2] = (unsigned char)v[2];
    }
}

// tile t of an oh x ow destination, thread tid -> its pixel (i, j); false beyond the destination
static PLY_HD inline bool ply_place(long t, int tid, int oh, int ow, int* i, int* j) {
    if (t >= ply_tiles(oh, ow)) return false;
    const int tiles_x = (ow + PLY_TW - 1) / PLY_TW;
    const int ty = (int)(t / tiles_x), tx = (int)(t - (long)ty * tiles_x);
    *i = ty * PLY_TH + tid / PLY_TW;
    *j = tx * PLY_TW + tid % PLY_TW;
    return *i < oh && *j < ow;
}
