// Image export on the device: the per-image host code behind the reference's eval loop and display helpers
// (interfaces/super_resolution.py:1572-1622: `.data.cpu().numpy() * 255`, clip, astype(uint8), a cubic resize, the lr_sr_hr panel;
// interfaces/base.py:565-618: ToPILImage -> Resize(.., BICUBIC) -> ToTensor, make_grid(nrow=1), save_image) for every image of a batch
// in ONE launch: quantise the fp32 samples to uint8, PIL's bicubic resize, interleaved RGB bytes at an offset and a row pitch the caller
// chooses (so that several launches can lay their items into one canvas).  Once the floats are quantised everything is integer
// arithmetic, so the result is BIT FOR BIT what numpy + Pillow give on the host (tests/export_ref.py is the specification;
// tests/test_export_device*.py hold both to the installed Pillow).  The mirror image of collate.hip, whose phases it follows.
//
// Layout: one work-group of 256 threads per item; no traffic between work-groups, no atomics, every loop bounded by the item's sizes.
// Every quantity the kernel reads (descriptor rows, samples) comes from DEVICE memory, so the launch can be captured.
//   quantise t = x * 255.0f, ONE IEEE fp32 multiply (no reciprocal; this file is compiled with -ffp-contract=off, tatt_amd/build.py, so
//            that the add of rule 1 is not fused into it: float32(k) / 255 * 255 truncates back to k for every byte k only then);
//            rule 0 ("floor", the eval loop): clip t to [0, 255], truncate; rule 1 ("round", save_image): t + 0.5f in one fp32 add,
//            clip, truncate.  NaN -> 0 under both rules, +-inf clips.  Done on the fly wherever a pass reads a source sample.
//   phase 0  coefficient tables in LDS, in double (pil_resample.h, as every resampling kernel)
//   phase 1  horizontal pass, source -> uint8 [H][OW][3] in LDS; skipped when W == OW (Pillow skips it too)
//   phase 2  vertical pass (skipped when H == OH), straight to out[offset + y * pitch + 3 x + c]; one BYTE per thread and step, so
//            consecutive threads write consecutive bytes and read consecutive bytes of the intermediate
// LDS per item: tables (max(5 OW, 4 W + 3 OW) + max(5 OH, 4 H + 3 OH) ints at most, bounds 2 (OW + OH) ints) and the intermediate
// (H * OW * 3 bytes): 120,112 bytes at most over every geometry within the limits below, of the CU's 160 KB.  A launch asks for what its largest item needs (none at the
// native size) and the kernel refuses a row that needs more.
#include "common.h"
#include "pil_resample.h"         // col_ksize, col_coeffs, col_clip8, exp_quant

#define EXP_THREADS 256
#define EXP_DESC 8                     // ints per descriptor row: b, c0, OH, OW, rule, out byte offset, row pitch in bytes, 0
#define EXP_MAX_H 128                  // source rows / columns a resampling pass takes (twice the large tile's HR each way)
#define EXP_MAX_W 512
#define EXP_MAX_OH 128
#define EXP_MAX_OW 512
#define EXP_MAX_INTER 98304            // bytes of the horizontal pass's result (H * OW * 3): 64 rows at OW = 512, what binds there
#define EXP_LDS 122880                 // most dynamic LDS of a launch (the largest item: 120,112 bytes, 86 x 512 -> 127 x 381)

struct ExpLayout { int ksh, ksv, kh, bh, kv, bv, inter, total; };

// byte offsets of the item's LDS regions (16-byte aligned); only for sizes exp_check accepted
static __host__ __device__ inline ExpLayout exp_layout(int H, int W, int oh, int ow) {
    ExpLayout g;
    int o = 0;
    auto take = [&o](int bytes) { const int at = o; o += (bytes + 15) & ~15; return at; };
    g.ksh = W == ow ? 0 : col_ksize(W, ow);
    g.ksv = H == oh ? 0 : col_ksize(H, oh);
    g.kh = take(ow * g.ksh * 4);
    g.bh = take(g.ksh ? ow * 8 : 0);
    g.kv = take(oh * g.ksv * 4);
    g.bv = take(g.ksv ? oh * 8 : 0);
    g.inter = take(g.ksh ? H * ow * 3 : 0);
    g.total = o;
    return g;
}

// 0: the row is taken; 1: bad argument (rule, reserved word); 2: geometry beyond tatt_export_limits; 3: channels, source or destination
// bytes leave src / out.  The same function refuses on the host before the launch and in the kernel.
static __host__ __device__ inline int exp_check(const int* d, int B, int C, int H, int W, long out_bytes) {
    const int b = d[0], c0 = d[1], oh = d[2], ow = d[3], rule = d[4], off = d[5], pitch = d[6];
    if ((rule != 0 && rule != 1) || d[7] != 0) return 1;
    if (H < 1 || W < 1 || oh < 1 || ow < 1 || (long)oh * ow * 3 > 0x7fffffffL) return 2;
    if (oh != H || ow != W) {                                       // (an item at the native size is only quantised: no pass, no limit)
        if (H > EXP_MAX_H || W > EXP_MAX_W || oh > EXP_MAX_OH || ow > EXP_MAX_OW) return 2;
        if (W != ow && (long)H * ow * 3 > EXP_MAX_INTER) return 2;
    }
    if (b < 0 || b >= B || c0 < 0 || c0 > C - 3) return 3;
    if (off < 0 || pitch < 3 * ow || (long)off + (long)(oh - 1) * pitch + 3L * ow > out_bytes) return 3;
    return 0;
}

__global__ __launch_bounds__(EXP_THREADS) void export_kernel(const float* __restrict__ src, long st_n, long st_c, long st_h, long st_w,
                                                             int B, int C, int H, int W, const int* __restrict__ desc,
                                                             unsigned char* __restrict__ out_base, long out_bytes, int lds_bytes) {
    extern __shared__ __align__(16) unsigned char exp_lds[];
    const int tid = threadIdx.x;
    const int* d = desc + (long)blockIdx.x * EXP_DESC;
    // The host entry refuses such rows before it launches; a replayed launch re-checks so that a stale descriptor cannot reach outside
    // the buffers: nothing is written for a row it refuses.
    if (exp_check(d, B, C, H, W, out_bytes) != 0) return;
    const int b = d[0], c0 = d[1], oh = d[2], ow = d[3], rule = d[4], pitch = d[6];
    const ExpLayout g = exp_layout(H, W, oh, ow);
    if (g.total > lds_bytes) return;
    const float* s = src + (long)b * st_n + (long)c0 * st_c;
    unsigned char* out = out_base + d[5];
    int* kh = (int*)(exp_lds + g.kh);
    int* bh = (int*)(exp_lds + g.bh);
    int* kv = (int*)(exp_lds + g.kv);
    int* bv = (int*)(exp_lds + g.bv);
    unsigned char* inter = exp_lds + g.inter;

    // phase 0
    const int nh = g.ksh ? ow : 0, nv = g.ksv ? oh : 0;
    for (int i = tid; i < nh + nv; i += EXP_THREADS) {
        if (i < nh) col_coeffs(i, W, ow, g.ksh, kh, bh);
        else col_coeffs(i - nh, H, oh, g.ksv, kv, bv);
    }
    if (nh + nv) __syncthreads();

    // phase 1: inter[yy][xx][c], one byte per thread and step
    const int row = ow * 3;
    if (g.ksh) {
        const int n1 = H * row;
        for (int i = tid; i < n1; i += EXP_THREADS) {
            const int yy = i / row, r = i - yy * row, xx = r / 3, c = r - xx * 3;
            const int xmin = bh[2 * xx], n = bh[2 * xx + 1];
            const int* k = kh + xx * g.ksh;
            const float* p = s + c * st_c + yy * st_h + xmin * st_w;
            int acc = 1 << (COL_PB - 1);
            for (int x = 0; x < n; ++x, p += st_w) acc += exp_quant(*p, rule) * k[x];
            inter[i] = (unsigned char)col_clip8(acc);
        }
        __syncthreads();
    }

    // phase 2: out[y][x][c] from the intermediate (LDS) or, without a horizontal pass, from the quantised source itself
    const int n2 = oh * row;
    for (int j = tid; j < n2; j += EXP_THREADS) {
        const int y = j / row, r = j - y * row, x = r / 3, c = r - x * 3;
        int v;
        if (g.ksv) {
            const int ymin = bv[2 * y], n = bv[2 * y + 1];
            const int* k = kv + y * g.ksv;
            int acc = 1 << (COL_PB - 1);
            if (g.ksh) {
                const unsigned char* p = inter + ymin * row + r;
                for (int t = 0; t < n; ++t, p += row) acc += (int)*p * k[t];
            } else {
                const float* p = s + c * st_c + ymin * st_h + x * st_w;
                for (int t = 0; t < n; ++t, p += st_h) acc += exp_quant(*p, rule) * k[t];
            }
            v = col_clip8(acc);
        } else {
            v = g.ksh ? (int)inter[j] : exp_quant(s[c * st_c + y * st_h + x * st_w], rule);
        }
        out[(long)y * pitch + r] = (unsigned char)v;
    }
}

TATT_API int tatt_export_limits(int* out) {
    if (!out) return 1;
    out[0] = EXP_MAX_H;
    out[1] = EXP_MAX_W;
    out[2] = EXP_MAX_OH;
    out[3] = EXP_MAX_OW;
    out[4] = EXP_MAX_INTER;
    return 0;
}

TATT_API int tatt_export_images(const float* src, long st_n, long st_c, long st_h, long st_w, int B, int C, int H, int W,
                                const int* desc, const int* desc_host, int n_items, unsigned char* out, long out_bytes, hipStream_t st) {
    if (!src || !desc || !desc_host || !out || n_items <= 0 || out_bytes <= 0 || B <= 0 || C < 3 || H <= 0 || W <= 0) return 1;
    if (st_n < 0 || st_c < 0 || st_h < 0 || st_w < 0) return 1;
    int lds = 0;
    for (int i = 0; i < n_items; ++i) {
        const int* d = desc_host + (long)i * EXP_DESC;
        const int rc = exp_check(d, B, C, H, W, out_bytes);
        if (rc) return rc;
        const int total = exp_layout(H, W, d[2], d[3]).total;
        if (total > EXP_LDS) return 2;
        if (total > lds) lds = total;
    }
    static TattPerDevice attr_once;                 // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(export_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, EXP_LDS);
    });
    hipLaunchKernelGGL(export_kernel, dim3(n_items), dim3(EXP_THREADS), (size_t)lds, st, src, st_n, st_c, st_h, st_w, B, C, H, W, desc, out,
                       out_bytes, lds);
    return LAUNCH_CHECK();
}
