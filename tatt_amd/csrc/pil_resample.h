// Pillow's 8-bit bicubic resampler (Resample.c: bicubic_filter, precompute_coeffs, normalize_coeffs_8bpc, the two-pass resize of RGB
// bytes) as device functions, one definition each.  tests/pil_resample_ref.py is the specification.  Who includes what:
//   the tables (col_ksize, col_coeffs, col_clip8)   collate.hip, export.hip, lines.hip, scene.hip, read.hip
//   the quantiser (exp_quant)                       export.hip (images out of the device), lines.hip (the blend of SR windows)
//   the RGB passes (pil_taps, pil_horizontal, pil_vertical) and the two kernel bodies built from them:
//     pil_window_body   one work-group per item, the whole item in LDS, float planes and the item's own mask plane out:
//                       line_windows_kernel (lines.hip), scene_windows_kernel (scene.hip).  collate_kernel runs the same two passes
//                       from a body of its own (collate.hip says why).
//     pil_tile_body     grid (tile, item), th x 64 output pixels per work-group, the pixel handed to the kernel's sink:
//                       resize_u8_kernel (scene.hip, feathered uint8 store), line_luma_kernel (read.hip, fp32 luma store)
// Every body is __forceinline__ and templated on the work-group size; a kernel keeps its descriptor row, its check and what it does with
// a refused row.  Every file that includes this header is compiled with -ffp-contract=off (tatt_amd/build.py): a fused multiply-add in
// the polynomial or in `center` changes coefficients, and one in exp_quant changes bytes.
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

// fp32 sample -> byte.  t = x * 255.0f in ONE fp32 multiply; rule 0 ("floor"): clip, truncate; rule 1 ("round"): t + 0.5f in one fp32
// add, clip, truncate.  NaN -> 0 under both rules, +-inf clips.
__device__ __forceinline__ int exp_quant(float x, int rule) {
    float t = __fmul_rn(x, 255.0f);
    if (rule) t = __fadd_rn(t, 0.5f);
    if (!(t > 0.0f)) return 0;                                      // negatives, -0.0, -inf and NaN
    return t >= 255.0f ? 255 : (int)t;
}

// ---- the passes over interleaved RGB bytes ---------------------------------------------------------------------------------------------
struct PilRgb { int r, g, b; };

// one output pixel of a pass: acc = 2^21 + sum p[t * step] * k[t] per channel in int32, clamp(acc >> 22, 0, 255)
__device__ __forceinline__ PilRgb pil_taps(const unsigned char* p, long step, const int* k, int n) {
    int a0 = 1 << (COL_PB - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t, p += step) {
        const int kt = k[t];
        a0 += p[0] * kt;
        a1 += p[1] * kt;
        a2 += p[2] * kt;
    }
    return {col_clip8(a0), col_clip8(a1), col_clip8(a2)};
}

// How the rows of a source lie: a `long` is the distance of two rows in BYTES (any pitch: a box of an image, the rows of a canvas);
// PilPacked is a packed image, rows `pixels` RGB pixels apart and nothing between them, whose pixel (row, x) is addressed by its INDEX,
// ((long)row * pixels + x) * 3 -- one multiply by the width and one by 3 where the byte form needs a 64 x 32-bit multiply by the pitch.
// pil_at: byte offset of pixel (row, x); pil_step: of one row; pil_packed_as: the rows of a packed w-pixel image in the caller's form.
struct PilPacked { int pixels; };
template <class X> __device__ __forceinline__ long pil_at(long row_bytes, int row, X x) { return row * row_bytes + x * 3; }
template <class X> __device__ __forceinline__ long pil_at(PilPacked s, int row, X x) { return ((long)row * s.pixels + x) * 3; }
__device__ __forceinline__ long pil_step(long row_bytes) { return row_bytes; }
__device__ __forceinline__ long pil_step(PilPacked s) { return (long)s.pixels * 3; }
__device__ __forceinline__ long pil_packed_as(long, int w) { return 3L * w; }
__device__ __forceinline__ PilPacked pil_packed_as(PilPacked, int w) { return {w}; }

// horizontal pass: the `rows` source rows from row r0 on (src = row 0, rows `stride` apart) into uint8 inter[rows][pitch][3] for the
// `cols` output columns whose coefficient rows are kh / bh (LDS), rounded to uint8 as Pillow rounds its intermediate image.
// Consecutive threads take consecutive columns of one row.  (r0 is a parameter so that r0 + yy is formed in 32 bits: with r0 rows
// added to `src` by the caller the compiler multiplies 64 x 64 bits per pixel.)
template <int THREADS, class Stride>
__device__ __forceinline__ void pil_horizontal(const unsigned char* src, Stride stride, int r0, const int* kh, const int* bh, int ksh,
                                               int rows, int cols, int pitch, unsigned char* inter, int tid) {
    const int n1 = rows * cols;
    for (int i = tid; i < n1; i += THREADS) {
        const int yy = i / cols, xx = i - yy * cols;
        const PilRgb v = pil_taps(src + pil_at(stride, r0 + yy, (long)bh[2 * xx]), 3, kh + xx * ksh, bh[2 * xx + 1]);
        unsigned char* q = inter + (yy * pitch + xx) * 3;
        q[0] = (unsigned char)v.r;
        q[1] = (unsigned char)v.g;
        q[2] = (unsigned char)v.b;
    }
}

// vertical pass over tn x tw output pixels; sink(y, x, r, g, b) takes each.  s1 = uint8 rows `stride` apart whose row 0 is source row
// r0 and whose pixel 0 is output column 0 (the source itself or the horizontal pass's result); kv / bv are the coefficient rows of the tn
// output rows; without a vertical pass (ksv == 0) output row y is source row y0 + y.  Call it once per address space of s1 (LDS,
// global): one call site for both would make every load a flat one.
template <int THREADS, class Stride, class Sink>
__device__ __forceinline__ void pil_vertical(const unsigned char* s1, Stride stride, int r0, const int* kv, const int* bv, int ksv, int y0,
                                             int tn, int tw, int tid, Sink&& sink) {
    const int n2 = tn * tw;
    for (int i = tid; i < n2; i += THREADS) {
        const int y = i / tw, x = i - y * tw;
        PilRgb v;
        if (ksv) {
            v = pil_taps(s1 + pil_at(stride, bv[2 * y] - r0, x), pil_step(stride), kv + y * ksv, bv[2 * y + 1]);
        } else {
            const unsigned char* p = s1 + pil_at(stride, y0 + y - r0, x);
            v = {p[0], p[1], p[2]};
        }
        sink(y, x, v.r, v.g, v.b);
    }
}

// ---- the window family: one work-group per item ----------------------------------------------------------------------------------------
// An item is the h x w window at column x0 of `source.resize((wl, h), BICUBIC)`, as float planes (ToTensor) with its OWN mask plane
// (1.0 where gray <= mean gray of the window).  Pillow's resampler treats every output column on its own, horizontal pass first, so the
// window is computed without the rest of the line.  A whole image is the window x0 = 0, w = wl.
struct PilWinLayout { int ksh, ksv, kh, bh, kv, bv, lum, inter, red, total; };

// byte offsets of the item's LDS regions (16-byte aligned); only for geometry the entry's check accepted
template <int THREADS>
static __host__ __device__ inline PilWinLayout pil_win_layout(int hs, int ws, int h, int wl, int w, int mask) {
    PilWinLayout g;
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
    g.red = take(mask ? (THREADS / 64) * 4 : 0);
    g.total = o;
    return g;
}

// the planes of a refused item: NaN
template <int THREADS>
__device__ __forceinline__ void pil_win_refuse(float* out, long floats, int tid) {
    for (long i = tid; i < floats; i += THREADS) out[i] = __builtin_nanf("");
}

// src = the source's first pixel, rows `stride` apart (bytes, or PilPacked); lds holds g.total bytes; out = the item's 3 + mask planes of h * w floats
//   phase 0  coefficient tables in LDS: rows x0 .. x0 + w - 1 of the horizontal table W_src -> wl, the vertical table H_src -> h
//   phase 1  horizontal pass into LDS for those w columns only; skipped when W_src == wl (Pillow skips it too: a copy, not a resample)
//   phase 2  vertical pass (skipped when H_src == h) straight into the planes, __fdiv_rn(v, 255) (IEEE division); with the mask,
//            L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 per pixel into LDS and sum(L) reduced over the work-group in integers
//   phase 3  mask plane: 1.0 where L * N <= sum(L), else 0.0 -- `0 if L > mean(L) else 255` without a rounding: L is an integer and
//            sum(L) / N is at least 1 / N away from any larger integer
template <int THREADS, class Stride>
__device__ __forceinline__ void pil_window_body(const unsigned char* src, Stride stride, const PilWinLayout& g, unsigned char* lds, int hs,
                                                int ws, int h, int wl, int x0, int w, bool mask, float* out, int tid) {
    int* kh = (int*)(lds + g.kh);
    int* bh = (int*)(lds + g.bh);
    int* kv = (int*)(lds + g.kv);
    int* bv = (int*)(lds + g.bv);
    unsigned char* lum = lds + g.lum;
    unsigned char* inter = lds + g.inter;
    int* red = (int*)(lds + g.red);

    // phase 0: row x0 + i of the line's horizontal table lands in row i of the window's (col_coeffs indexes by the line's column)
    const int nh = g.ksh ? w : 0, nv = g.ksv ? h : 0;
    for (int i = tid; i < nh + nv; i += THREADS) {
        if (i < nh) col_coeffs(x0 + i, ws, wl, g.ksh, kh - (long)x0 * g.ksh, bh - 2L * x0);
        else col_coeffs(i - nh, hs, h, g.ksv, kv, bv);
    }
    if (nh + nv) __syncthreads();

    // phase 1
    if (g.ksh) {
        pil_horizontal<THREADS>(src, stride, 0, kh, bh, g.ksh, hs, w, w, inter, tid);
        __syncthreads();
    }

    // phase 2
    const int n = h * w;
    int lsum = 0;
    auto sink = [&](int y, int x, int r, int gg, int b) {
        const int i = y * w + x;
        out[i] = __fdiv_rn((float)r, 255.f);
        out[n + i] = __fdiv_rn((float)gg, 255.f);
        out[2 * n + i] = __fdiv_rn((float)b, 255.f);
        if (mask) {
            const int L = (19595 * r + 38470 * gg + 7471 * b + 0x8000) >> 16;
            lum[i] = (unsigned char)L;
            lsum += L;
        }
    };
    if (g.ksh) pil_vertical<THREADS>(inter, pil_packed_as(stride, w), 0, kv, bv, g.ksv, 0, h, w, tid, sink);
    else pil_vertical<THREADS>(src + x0 * 3L, stride, 0, kv, bv, g.ksv, 0, h, w, tid, sink);
    if (!mask) return;

    // phase 3
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = lsum;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int i = 0; i < THREADS / 64; ++i) total += red[i];
    for (int i = tid; i < n; i += THREADS) out[3 * n + i] = (int)lum[i] * n <= total ? 1.f : 0.f;
}

// ---- the tile family: grid (tile, item) ------------------------------------------------------------------------------------------------
// A tile of Pillow's resize depends only on the source rows and columns that the coefficient rows of its own output rows and columns
// name, so a work-group computes one tile of th x PIL_TILE_W output pixels alone.  th = PIL_TILE_H while the tile's source rows fit
// PIL_TILE_INTER_ROWS rows of intermediate, halved until they do (down-scales beyond ~5 : 1 in the vertical; 1 row at 16 : 1), so the
// LDS of a tile is bounded whatever the factor while in <= 16 out per axis (ksize <= 65): horizontal table <= 64 * 65 * 4, intermediate
// <= 192 * 192, vertical table <= 2,944, bounds 768: under 58 KB; an up-scale takes under 10 KB.
#define PIL_TILE_H 32
#define PIL_TILE_W 64
#define PIL_TILE_INTER_ROWS 192        // rows of the horizontal pass's result a tile keeps in LDS

struct PilTileLayout { int ksh, ksv, th, span, kh, bh, kv, bv, inter, total; };

// an upper bound of the source samples that n consecutive output samples of a pass in -> out name: the first one starts no lower than
// center0 - support - 0.5, the last one ends no higher than center0 + (n - 1) * scale + support + 0.5 (col_coeffs)
static __host__ __device__ inline int pil_span(int in, int out, int n) {
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    const long s = (long)ceil((n - 1) * scale + 4.0 * fs) + 2;
    return s > in ? in : (int)s;
}

// tile height and LDS regions of an item (16-byte aligned)
static __host__ __device__ inline PilTileLayout pil_tile_layout(int hs, int ws, int oh, int ow) {
    PilTileLayout g;
    int o = 0;
    auto take = [&o](int bytes) { const int at = o; o += (bytes + 15) & ~15; return at; };
    g.ksh = ws == ow ? 0 : col_ksize(ws, ow);
    g.ksv = hs == oh ? 0 : col_ksize(hs, oh);
    g.th = PIL_TILE_H;
    if (g.ksv)
        while (g.th > 1 && pil_span(hs, oh, g.th) > PIL_TILE_INTER_ROWS) g.th >>= 1;
    g.span = g.ksv ? pil_span(hs, oh, g.th) : g.th;
    g.kh = take(PIL_TILE_W * g.ksh * 4);
    g.bh = take(g.ksh ? PIL_TILE_W * 8 : 0);
    g.kv = take(g.th * g.ksv * 4);
    g.bv = take(g.ksv ? g.th * 8 : 0);
    g.inter = take(g.ksh ? g.span * PIL_TILE_W * 3 : 0);
    g.total = o;
    return g;
}

static __host__ __device__ inline long pil_tiles(int oh, int ow, int th) {
    return (long)((oh + th - 1) / th) * ((ow + PIL_TILE_W - 1) / PIL_TILE_W);
}

// tile `tile` (< pil_tiles) of the item src (rows sp bytes apart, hs x ws) -> oh x ow; sink(Y, X, r, g, b) takes output pixel (Y, X)
//   phase 0  the tile's coefficient rows in LDS: rows x0 .. x0 + tw - 1 and y0 .. y0 + tn - 1 of the two tables land in rows 0 ..
//   phase 1  horizontal pass for the source rows r0 .. r0 + nr - 1 that the tile's vertical rows name, into LDS [nr][64][3].  A wave
//            takes 64 neighbouring output columns of ONE source row: its lanes read one contiguous span of that row
//            (64 * W_src / OW + ksize pixels), i.e. a few cache lines per tap.
//   phase 2  vertical pass from LDS: a wave reads, per tap, the 192 consecutive bytes of one intermediate row (lane x bytes 3x .. 3x + 2:
//            48 consecutive dwords, lanes sharing a dword are served by one broadcast -- no bank conflict)
// A pass whose sizes agree is skipped as Pillow skips it (the vertical pass then reads the source itself, the horizontal one writes
// tn rows).  No per-thread arrays.
template <int THREADS, class Sink>
__device__ __forceinline__ void pil_tile_body(const unsigned char* src, long sp, const PilTileLayout& g, unsigned char* lds, int hs, int ws,
                                              int oh, int ow, unsigned tile, int tid, Sink&& sink) {
    const int tiles_x = (ow + PIL_TILE_W - 1) / PIL_TILE_W;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * g.th, x0 = tx * PIL_TILE_W;
    const int tn = min(g.th, oh - y0), tw = min(PIL_TILE_W, ow - x0);
    int* kh = (int*)(lds + g.kh);
    int* bh = (int*)(lds + g.bh);
    int* kv = (int*)(lds + g.kv);
    int* bv = (int*)(lds + g.bv);
    unsigned char* inter = lds + g.inter;

    // phase 0
    const int nh = g.ksh ? tw : 0, nv = g.ksv ? tn : 0;
    for (int i = tid; i < nh + nv; i += THREADS) {
        if (i < nh) col_coeffs(x0 + i, ws, ow, g.ksh, kh - (long)x0 * g.ksh, bh - 2L * x0);
        else col_coeffs(y0 + i - nh, hs, oh, g.ksv, kv - (long)y0 * g.ksv, bv - 2L * y0);
    }
    if (nh + nv) __syncthreads();

    // the source rows the tile reads: first sample of its first output row .. last sample of its last one (both increase with the row)
    const int r0 = g.ksv ? bv[0] : y0;
    const int nr = g.ksv ? bv[2 * (tn - 1)] + bv[2 * (tn - 1) + 1] - r0 : tn;
    if (g.ksh && nr > g.span) return;                                // (pil_span bounds it: never taken, and the same in every thread)

    // phase 1
    if (g.ksh) {
        pil_horizontal<THREADS>(src, sp, r0, kh, bh, g.ksh, nr, tw, PIL_TILE_W, inter, tid);
        __syncthreads();
    }

    // phase 2
    auto at = [&](int y, int x, int r, int gg, int b) { sink(y0 + y, x0 + x, r, gg, b); };
    if (g.ksh) pil_vertical<THREADS>(inter, PIL_TILE_W * 3L, r0, kv, bv, g.ksv, y0, tn, tw, tid, at);
    else pil_vertical<THREADS>(src + x0 * 3L, sp, 0, kv, bv, g.ksv, y0, tn, tw, tid, at);
}
