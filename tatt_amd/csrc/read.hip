// Reading super-resolved text lines at their own width (tatt_amd/read.py is the specification, tests/test_read*.py hold the kernels to it).
//   line_luma_kernel        the recogniser's input of every line of a call in ONE launch: Pillow's 8-bit bicubic resize of the uint8 line
//                           canvas (where tatt_line_blend left it in device memory) to (32, rw), then n = 299 R + 587 G + 114 B and
//                           float(n) * float(1 / 255000), stored as fp32 straight into the line's place in its bucket tensor.  One fp32
//                           multiply, nothing to contract: bit for bit `read.line_luma_host`.
//   ctc_greedy_read_kernel  greedy CTC decoding that says how sure it is: per step the arg-max (ties to the lower class), the maximum and
//                           sum exp(x - max) across the wave, i.e. the soft-max probability 1 / sum of the decision; repeats merged, blank 0
//                           dropped; one record row per image, scattered through an index array so that the launches of all buckets of a
//                           call fill ONE record buffer in input order.
// line_luma_kernel tiles the output as resize_u8_kernel of scene.hip does: grid (tile, line), 256 threads, pil_tile_body of pil_resample.h
// (th x 64 output pixels per work-group; the tile's coefficient rows, the horizontal pass of the source rows it names into LDS, the
// vertical pass) with the luma store as its sink.  Like its siblings: no traffic between work-groups, no atomics, every loop bounded by
// descriptor values that were checked, every quantity read from DEVICE memory, the same check on the host before the launch and in the
// kernel.  Compiled with -ffp-contract=off (tatt_amd/build.py) for pil_resample.h's tables in double.
#include "common.h"
#include "pil_resample.h"         // pil_tile_layout, pil_tiles, pil_tile_body

#define RD_THREADS 256
#define RD_DESC 8                      // ints per line row: src byte offset, H, W, pitch, rw, float offset of the target, 0, 0
#define RD_OH 32                       // the recogniser's input height
#define RD_MAX_RW 1020                 // widest input: T = rw / 4 + 1 <= 256 steps
#define RD_MAX_DOWN 16                 // largest in / out per axis (ksize <= 65)
#define RD_MAX_W 32768                 // widest line canvas
#define RD_MAX_LINES 65535             // grid.y
#define RD_LDS 65536                   // no tile needs more: 64 * 65 * 4 + 512 + th * ksv * 4 + 8 th + 192 * 192 with th * ksv <= 32 * 9 or th <= 8
#define RD_MAX_T 256
#define RD_MAX_C 64

// 0: the row is taken; 1: a reserved word is set; 2: geometry beyond tatt_read_limits; 3: the source rectangle or the target leaves its buffer
static __host__ __device__ inline int rd_check(const int* d, long src_bytes, long out_floats) {
    const int so = d[0], hs = d[1], ws = d[2], sp = d[3], rw = d[4], fo = d[5];
    if (d[6] != 0 || d[7] != 0) return 1;
    if (hs < 1 || ws < 1 || rw < 1 || rw > RD_MAX_RW || ws > RD_MAX_W) return 2;
    if (hs > RD_MAX_DOWN * RD_OH || ws > (long)RD_MAX_DOWN * rw) return 2;
    if (so < 0 || sp < 3L * ws || so + (long)(hs - 1) * sp + 3L * ws > src_bytes) return 3;
    if (fo < 0 || fo + (long)RD_OH * rw > out_floats) return 3;
    return 0;
}

__global__ __launch_bounds__(RD_THREADS) void line_luma_kernel(const unsigned char* __restrict__ src_base, long src_bytes,
                                                               const int* __restrict__ desc, float* __restrict__ out_base,
                                                               long out_floats, int lds_bytes) {
    extern __shared__ __align__(16) unsigned char rd_lds[];
    const int tid = threadIdx.x;
    const int* d = desc + (long)blockIdx.y * RD_DESC;
    const int hs = d[1], ws = d[2], rw = d[4], fo = d[5];
    // The host entry refuses such rows before it launches; a replayed launch re-checks so that a stale row cannot reach outside the
    // buffers: the line's own target (when it lies inside) is filled with NaN by the work-groups of its grid row, nothing else is touched.
    if (rw < 1 || rw > RD_MAX_RW || fo < 0 || fo + (long)RD_OH * rw > out_floats) return;
    float* out = out_base + fo;
    const bool ok = rd_check(d, src_bytes, out_floats) == 0;
    const PilTileLayout g = ok ? pil_tile_layout(hs, ws, RD_OH, rw) : PilTileLayout{};
    if (!ok || g.total > lds_bytes) {
        for (int i = blockIdx.x * RD_THREADS + tid; i < RD_OH * rw; i += gridDim.x * RD_THREADS) out[i] = __builtin_nanf("");
        return;
    }
    if ((long)blockIdx.x >= pil_tiles(RD_OH, rw, g.th)) return;
    const float inv = (float)(1.0 / 255000.0);
    pil_tile_body<RD_THREADS>(src_base + d[0], d[3], g, rd_lds, hs, ws, RD_OH, rw, blockIdx.x, tid, [&](int Y, int X, int r, int gg, int b) {
        out[(long)Y * rw + X] = (float)(299 * r + 587 * gg + 114 * b) * inv;                  // (n <= 255000: exact in fp32)
    });
}

TATT_API int tatt_line_luma(const unsigned char* src, long src_bytes, const int* desc, const int* desc_host, int n_lines, float* out,
                            long out_floats, hipStream_t st) {
    if (!src || !desc || !desc_host || !out || n_lines <= 0 || src_bytes <= 0 || out_floats <= 0) return 1;
    if (n_lines > RD_MAX_LINES) return 2;
    int lds = 0, tiles = 0;
    for (int i = 0; i < n_lines; ++i) {
        const int* d = desc_host + (long)i * RD_DESC;
        const int rc = rd_check(d, src_bytes, out_floats);
        if (rc) return rc;
        const PilTileLayout g = pil_tile_layout(d[1], d[2], RD_OH, d[4]);
        if (g.total > RD_LDS) return 2;
        if (g.total > lds) lds = g.total;
        const int t = (int)pil_tiles(RD_OH, d[4], g.th);
        if (t > tiles) tiles = t;
    }
    hipLaunchKernelGGL(line_luma_kernel, dim3(tiles, n_lines), dim3(RD_THREADS), (size_t)lds, st, src, src_bytes, desc, out, out_floats,
                       lds);
    return LAUNCH_CHECK();
}

TATT_API int tatt_read_limits(int* out) {
    if (!out) return 1;
    out[0] = RD_OH;
    out[1] = RD_MAX_RW;
    out[2] = RD_MAX_DOWN;
    out[3] = RD_MAX_W;
    out[4] = RD_MAX_LINES;
    out[5] = RD_MAX_T;
    out[6] = RD_MAX_C;
    out[7] = RD_DESC;
    return 0;
}

// ---- greedy CTC with confidences -------------------------------------------------------------------------------------------------------
// One wave per image, lane = class.  logits (T, B, C) by element strides.  Record row of image b, at record + index[b] * st_rec, in
// 32-bit words: [0, cap) the decoded classes padded with -1 | [cap, 2 cap) for every decoded class the first step of its run, padded with
// -1 | [2 cap, 3 cap) fp32: the soft-max probability of the arg-max at that step, padded with 0 | [3 cap] the decoded length |
// [3 cap + 1] fp32: the minimum over ALL T steps of the arg-max's probability.  A row index outside 0 .. n_rows - 1 writes nothing.
__global__ __launch_bounds__(64) void ctc_greedy_read_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c, int T,
                                                             int C, const int* __restrict__ index, int* __restrict__ record,
                                                             int n_rows, int cap, long st_rec) {
    __shared__ int cls[RD_MAX_T];
    __shared__ int stp[RD_MAX_T];
    __shared__ float prob[RD_MAX_T];
    __shared__ int n_sh;
    __shared__ float conf_sh;
    const int bidx = blockIdx.x, lane = threadIdx.x;
    const float* x = logits + bidx * st_b + lane * st_c;
#pragma unroll 4                                                     // (the steps are independent: four reduction chains in flight)
    for (int t = 0; t < T; ++t) {
        const float v0 = lane < C ? x[t * st_t] : -INFINITY;
        float v = v0;
        int k = lane < C ? lane : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(v, o, 64);
            const int k2 = __shfl_xor(k, o, 64);
            // a NaN wins over any number (torch.argmax), ties and NaN against NaN go to the lower class
            const bool take = k2 != 0x7fffffff && ((v2 != v2) ? (v == v || k2 < k) : (v == v && (v2 > v || (v2 == v && k2 < k))));
            if (take) { v = v2; k = k2; }
        }
        const float s = wave_sum(lane < C ? expf(v0 - v) : 0.f);          // (>= 1: the arg-max's own term)
        if (lane == 0) {
            cls[t] = k;
            prob[t] = 1.f / s;
        }
    }
    __syncthreads();
    if (lane == 0) {
        int n = 0, last = 0;
        float conf = INFINITY;
        for (int t = 0; t < T; ++t) {
            const int c = cls[t];
            const float p = prob[t];
            conf = p < conf || p != p ? p : conf;
            if (c != last) {
                if (c != 0) { cls[n] = c; stp[n] = t; prob[n] = p; ++n; }      // (n <= t: written only after index t was read)
                last = c;
            }
        }
        n_sh = n;
        conf_sh = conf;
    }
    __syncthreads();
    const int row = index[bidx], n = n_sh;
    if (row < 0 || row >= n_rows) return;
    int* rec = record + row * st_rec;
    for (int r = lane; r < cap; r += 64) {
        rec[r] = r < n ? cls[r] : -1;
        rec[cap + r] = r < n ? stp[r] : -1;
        rec[2 * cap + r] = r < n ? __float_as_int(prob[r]) : 0;
    }
    if (lane == 0) {
        rec[3 * cap] = n;
        rec[3 * cap + 1] = __float_as_int(conf_sh);
    }
}

TATT_API int tatt_ctc_greedy_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* index,
                                  int* record, int n_rows, int cap, long st_rec, hipStream_t st) {
    if (!logits || !index || !record) return 1;
    if (T <= 0 || T > RD_MAX_T || B <= 0 || C <= 0 || C > RD_MAX_C || n_rows <= 0 || cap < T || st_rec < 3L * cap + 2) return 1;
    hipLaunchKernelGGL(ctc_greedy_read_kernel, dim3(B), dim3(64), 0, st, logits, st_t, st_b, st_c, T, C, index, record, n_rows, cap,
                       st_rec);
    return LAUNCH_CHECK();
}
