// Batch collation on the device: the image half of the reference's collate function (alignCollate_realWTLAMask.__call__ ->
// resizeNormalize, dataset/dataset.py:1266-1319,1980-2003) for every image of a batch in ONE launch: PIL's bicubic resize of an RGB
// uint8 image, ToTensor (uint8 -> float / 255, CHW) and the binarised mask plane (gray <= mean gray -> 1).  Everything after the decode
// is integer arithmetic on uint8 pixels, so the result is BIT FOR BIT what Pillow + torch give on the host (tests/pil_resample_ref.py
// is the specification; tests/test_collate_device*.py hold both to the installed Pillow).
//
// Layout: one work-group of 256 threads per output image ("item"); no traffic between work-groups, no atomics, every loop bounded by
// the item's sizes.  Every quantity the kernel reads (descriptor rows, pixels) comes from DEVICE memory, so a captured launch sees
// whatever the staging copy in front of it wrote.
//   phase 0  coefficient tables in LDS, in double, exactly as Pillow's precompute_coeffs + normalize_coeffs_8bpc (col_coeffs): one thread
//            per output column / row.  This file is compiled with -ffp-contract=off (tatt_amd/build.py).
//   phase 1  horizontal pass (pil_horizontal), source (interleaved RGB in global memory) -> uint8 [H_src][OW][3] in LDS.  Skipped when
//            W_src == OW (Pillow skips it too: a copy, not a resample).
//   phase 2  vertical pass (pil_vertical, skipped when H_src == OH) straight into the float planes out[c][y][x] = float(v) / 255 (IEEE
//            division), consecutive threads on consecutive x; with the mask, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 per pixel
//            into LDS and sum(L) reduced over the work-group in integers
//   phase 3  mask plane: 1.0 where L * N <= sum(L), else 0.0 -- `0 if L > mean(L) else 255` without a rounding
// The two passes are pil_resample.h's, shared with every resampling kernel; the source is addressed as a packed image (PilPacked).
// The BODY around them -- layout with a static reduction block, check, sink, mask plane -- is this kernel's own copy of what
// pil_window_body does for lines.hip and scene.hip: on that body, which computes the same, tatt_collate_images ran 0.3 us (0.5 %)
// slower per batch of 96 items, outside the run-to-run spread, whichever way the source was addressed
// (profiles/pil_resample_core_ab.txt).
// LDS per item: tables ((4 W_src + 3 OW) + (4 H_src + 3 OH) ints at most, bounds 2 (OW + OH) ints), L (OH * OW bytes), the
// intermediate (H_src * OW * 3 bytes): 138.3 KB at the limits below, of the CU's 160 KB.
#include "common.h"
#include "pil_resample.h"         // col_ksize, col_coeffs; pil_horizontal, pil_vertical, PilPacked

#define COL_THREADS 256
#define COL_DESC 8                     // ints per descriptor row: src byte offset, H_src, W_src, OH, OW, mask flag, out float offset, 0
#define COL_MAX_ROWS 256               // source rows / columns the resampling passes take
#define COL_MAX_COLS 1024
#define COL_MAX_INTER 98304            // bytes of the horizontal pass's result (H_src * OW * 3)
#define COL_MAX_OH 64
#define COL_MAX_OW 256
#define COL_LDS 147456                 // dynamic LDS of every launch (the largest item: 141,568 bytes + alignment)

struct ColLayout { int ksh, ksv, kh, bh, kv, bv, lum, inter, total; };

static __host__ __device__ inline bool col_takes(int hs, int ws, int oh, int ow) {
    if (hs < 1 || ws < 1 || oh < 1 || ow < 1 || oh > COL_MAX_OH || ow > COL_MAX_OW) return false;
    if (hs > COL_MAX_ROWS || ws > COL_MAX_COLS) return false;
    return ws == ow || (long)hs * ow * 3 <= COL_MAX_INTER;
}

// byte offsets of the item's LDS regions (16-byte aligned); only for sizes col_takes accepted
static __host__ __device__ inline ColLayout col_layout(int hs, int ws, int oh, int ow, int mask) {
    ColLayout g;
    int o = 0;
    auto take = [&o](int bytes) { const int at = o; o += (bytes + 15) & ~15; return at; };
    g.ksh = ws == ow ? 0 : col_ksize(ws, ow);
    g.ksv = hs == oh ? 0 : col_ksize(hs, oh);
    g.kh = take(ow * g.ksh * 4);
    g.bh = take(g.ksh ? ow * 8 : 0);
    g.kv = take(oh * g.ksv * 4);
    g.bv = take(g.ksv ? oh * 8 : 0);
    g.lum = take(mask ? oh * ow : 0);
    g.inter = take(g.ksh ? hs * ow * 3 : 0);
    g.total = o;
    return g;
}

__global__ __launch_bounds__(COL_THREADS) void collate_kernel(const unsigned char* __restrict__ packed, long packed_bytes,
                                                              const int* __restrict__ desc, float* __restrict__ out_base,
                                                              long out_floats) {
    extern __shared__ __align__(16) unsigned char col_lds[];
    __shared__ int red[COL_THREADS / 64];
    const int tid = threadIdx.x;
    const int* d = desc + (long)blockIdx.x * COL_DESC;
    const int src_off = d[0], hs = d[1], ws = d[2], oh = d[3], ow = d[4], mask = d[5] != 0, out_off = d[6];
    // The host entry refuses such rows before it launches; a replayed launch re-checks so that a stale descriptor cannot reach outside
    // the buffers: the item's planes (when they lie inside) are filled with NaN, nothing else is touched.
    const long N = (long)oh * ow, planes = 3 + mask;
    const bool out_ok = oh >= 1 && ow >= 1 && oh <= COL_MAX_OH && ow <= COL_MAX_OW && out_off >= 0 && out_off + planes * N <= out_floats;
    if (!out_ok) return;
    float* out = out_base + out_off;
    if (!col_takes(hs, ws, oh, ow) || src_off < 0 || src_off + (long)hs * ws * 3 > packed_bytes) {
        for (long i = tid; i < planes * N; i += COL_THREADS) out[i] = __builtin_nanf("");
        return;
    }
    const ColLayout g = col_layout(hs, ws, oh, ow, mask);         // (total <= COL_LDS for everything col_takes accepts: see the header comment)
    const unsigned char* src = packed + src_off;
    int* kh = (int*)(col_lds + g.kh);
    int* bh = (int*)(col_lds + g.bh);
    int* kv = (int*)(col_lds + g.kv);
    int* bv = (int*)(col_lds + g.bv);
    unsigned char* lum = mask ? col_lds + g.lum : nullptr;
    unsigned char* inter = col_lds + g.inter;

    // phase 0
    const int nh = g.ksh ? ow : 0, nv = g.ksv ? oh : 0;
    for (int i = tid; i < nh + nv; i += COL_THREADS) {
        if (i < nh) col_coeffs(i, ws, ow, g.ksh, kh, bh);
        else col_coeffs(i - nh, hs, oh, g.ksv, kv, bv);
    }
    __syncthreads();

    // phase 1
    if (g.ksh) {
        pil_horizontal<COL_THREADS>(src, PilPacked{ws}, 0, kh, bh, g.ksh, hs, ow, ow, inter, tid);
        __syncthreads();
    }

    // phase 2 (two call sites: the source pointer is LDS in one and global memory in the other)
    const int n = oh * ow;
    int lsum = 0;
    auto sink = [&](int y, int x, int r, int gg, int b) {
        const int i = y * ow + x;
        out[i] = __fdiv_rn((float)r, 255.f);
        out[n + i] = __fdiv_rn((float)gg, 255.f);
        out[2 * n + i] = __fdiv_rn((float)b, 255.f);
        if (lum) {
            const int L = (19595 * r + 38470 * gg + 7471 * b + 0x8000) >> 16;
            lum[i] = (unsigned char)L;
            lsum += L;
        }
    };
    if (g.ksh) pil_vertical<COL_THREADS>(inter, PilPacked{ow}, 0, kv, bv, g.ksv, 0, oh, ow, tid, sink);
    else pil_vertical<COL_THREADS>(src, PilPacked{ow}, 0, kv, bv, g.ksv, 0, oh, ow, tid, sink);
    if (!mask) return;

    // phase 3
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = lsum;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < COL_THREADS / 64; ++w) total += red[w];
    for (int i = tid; i < n; i += COL_THREADS) out[3 * n + i] = (int)lum[i] * n <= total ? 1.f : 0.f;
}

TATT_API int tatt_collate_limits(int* out) {
    if (!out) return 1;
    out[0] = COL_MAX_ROWS;
    out[1] = COL_MAX_COLS;
    out[2] = COL_MAX_INTER;
    out[3] = COL_MAX_OH;
    out[4] = COL_MAX_OW;
    return 0;
}

TATT_API int tatt_collate_images(const unsigned char* packed, long packed_bytes, const int* desc, const int* desc_host, int n_items,
                                 float* out, long out_floats, hipStream_t st) {
    if (!packed || !desc || !desc_host || !out || n_items <= 0 || packed_bytes <= 0 || out_floats <= 0) return 1;
    for (int i = 0; i < n_items; ++i) {
        const int* d = desc_host + (long)i * COL_DESC;
        const int hs = d[1], ws = d[2], oh = d[3], ow = d[4];
        if (!col_takes(hs, ws, oh, ow) || col_layout(hs, ws, oh, ow, d[5] != 0).total > COL_LDS) return 2;
        if (d[0] < 0 || d[0] + (long)hs * ws * 3 > packed_bytes) return 3;
        if (d[6] < 0 || d[6] + (long)(3 + (d[5] != 0)) * oh * ow > out_floats) return 3;
    }
    static TattPerDevice attr_once;                 // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(collate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, COL_LDS);
    });
    hipLaunchKernelGGL(collate_kernel, dim3(n_items), dim3(COL_THREADS), (size_t)COL_LDS, st, packed, packed_bytes, desc, out, out_floats);
    return LAUNCH_CHECK();
}
