// The ASTER recogniser (reference model/recognizer/): the pieces its front and encoder need beyond the shared operators, and its
// attention decoder (model/recognizer/attention_recognition_head.py) as ONE launch.
//   resize_bilinear_ac : F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=True)        (recognizer_builder.py:77)
//   grid_sample_sized  : tatt_grid_sample_fwd with an output size of its own (32 x 128 in, 32 x 100 out; tps_spatial_transformer.py:110-114)
//   add_relu           : relu(a + b), the tail of AsterBlock (resnet_aster.py:59-60)
//   gru_cell           : the gate arithmetic of one nn.GRU step from gi / gh (the step-by-step route of the decoder)
//   attn_decode        : all L steps of the decoder, one work-group per image (see below)
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void resize_bilinear_ac_kernel(const float* __restrict__ x, long xsn, long xsc, long xsh, long xsw, float* __restrict__ y,
                                          int B, int C, int H, int W, int Ho, int Wo) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * C * Ho * Wo) return;
    const int ox = idx % Wo, oy = (idx / Wo) % Ho, c = (idx / ((long)Wo * Ho)) % C, b = idx / ((long)Wo * Ho * C);
    // torch's area_pixel_compute_scale for align_corners=True: (in - 1) / (out - 1) in fp32, source index = scale * destination index
    const float sh = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, sw = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const float fy = sh * oy, fx = sw * ox;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 < H - 1 ? y0 + 1 : y0, x1 = x0 < W - 1 ? x0 + 1 : x0;
    const float ly = fy - y0, lx = fx - x0;
    const float* p = x + b * xsn + c * xsc;
    const float v00 = p[y0 * xsh + x0 * xsw], v01 = p[y0 * xsh + x1 * xsw], v10 = p[y1 * xsh + x0 * xsw], v11 = p[y1 * xsh + x1 * xsw];
    y[idx] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}
TATT_API int tatt_resize_bilinear_ac(const float* x, long xsn, long xsc, long xsh, long xsw, float* y, int B, int C, int H, int W,
                                     int Ho, int Wo, hipStream_t st) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return 1;
    hipLaunchKernelGGL(resize_bilinear_ac_kernel, dim3(cdiv((long)B * C * Ho * Wo, 256)), dim3(256), 0, st, x, xsn, xsc, xsh, xsw, y, B, C,
                       H, W, Ho, Wo);
    return LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct SizedSampleGeom { int B, C, H, W, Ho, Wo; long xsn, xsc, xsh, xsw; };

__device__ __forceinline__ float sized_tap(const float* x, const SizedSampleGeom& g, int b, int c, int yi, int xi) {
    if (xi < 0 || xi >= g.W || yi < 0 || yi >= g.H) return 0.f;
    return x[b * g.xsn + c * g.xsc + yi * g.xsh + xi * g.xsw];
}
// out (B,Ho,Wo,C) NHWC; one thread per output pixel
__global__ void grid_sample_sized_kernel(const float* __restrict__ x, const float* __restrict__ src, float* __restrict__ out,
                                         SizedSampleGeom g) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)g.B * g.Ho * g.Wo) return;
    const int b = idx / ((long)g.Ho * g.Wo);
    const float cx = fminf(fmaxf(src[idx * 2], 0.f), 1.f), cy = fminf(fmaxf(src[idx * 2 + 1], 0.f), 1.f);
    const float gx = 2.f * cx - 1.f, gy = 2.f * cy - 1.f;
    const float ix = ((gx + 1.f) * g.W - 1.f) * 0.5f, iy = ((gy + 1.f) * g.H - 1.f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = ix - fx, ty = iy - fy;
    for (int c = 0; c < g.C; ++c) {
        const float v00 = sized_tap(x, g, b, c, y0, x0), v01 = sized_tap(x, g, b, c, y0, x0 + 1);
        const float v10 = sized_tap(x, g, b, c, y0 + 1, x0), v11 = sized_tap(x, g, b, c, y0 + 1, x0 + 1);
        out[idx * g.C + c] = v00 * (1.f - tx) * (1.f - ty) + v01 * tx * (1.f - ty) + v10 * (1.f - tx) * ty + v11 * tx * ty;
    }
}
TATT_API int tatt_grid_sample_sized_fwd(const float* x, long xsn, long xsc, long xsh, long xsw, const float* src, float* out, int B,
                                        int C, int H, int W, int Ho, int Wo, hipStream_t st) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return 1;
    SizedSampleGeom g = {B, C, H, W, Ho, Wo, xsn, xsc, xsh, xsw};
    hipLaunchKernelGGL(grid_sample_sized_kernel, dim3(cdiv((long)B * Ho * Wo, 256)), dim3(256), 0, st, x, src, out, g);
    return LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void add_relu_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = fmaxf(a[i] + b[i], 0.f);
}
TATT_API int tatt_add_relu(const float* a, const float* b, float* y, long n, hipStream_t st) {
    if (n < 1) return 1;
    hipLaunchKernelGGL(add_relu_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a, b, y, n);
    return LAUNCH_CHECK();
}

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.f / (1.f + expf(-x)); }

// hout[r,j] = (1 - z) n + z h with r = sig(gi_r + gh_r), z = sig(gi_z + gh_z), n = tanh(gi_n + r gh_n); gi, gh (R, 3H) in gate order r|z|n
__global__ void gru_cell_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ h,
                                float* __restrict__ hout, int R, int H) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)R * H) return;
    const int r = i / H, j = i % H;
    const float* a = gi + (long)r * 3 * H;
    const float* b = gh + (long)r * 3 * H;
    const float rg = sigmoid_acc(a[j] + b[j]), zg = sigmoid_acc(a[H + j] + b[H + j]);
    const float n = tanhf(a[2 * H + j] + rg * b[2 * H + j]);
    hout[i] = (1.f - zg) * n + zg * h[i];
}
TATT_API int tatt_gru_cell(const float* gi, const float* gh, const float* h, float* hout, int R, int H, hipStream_t st) {
    if (R < 1 || H < 1) return 1;
    hipLaunchKernelGGL(gru_cell_kernel, dim3(cdiv((long)R * H, 256)), dim3(256), 0, st, gi, gh, h, hout, R, H);
    return LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The attention decoder, all L steps in one launch.
//
// One work-group of 512 threads per image carries that image's rows (1: forced / greedy, 5: its beams) through every step; nothing is
// exchanged between work-groups, so the launch has no in-flight synchronisation, no residency requirement and no wait that could expire.
// Per step and row (DecoderUnit.forward, attention_recognition_head.py:258-271):
//   sProj = sEmbed(s);  e_t = wEmbed(tanh(sProj + xProj_t));  alpha = softmax_t(e);  ctx = sum_t alpha_t x_t
//   gi = E2[y_prev] + W_ih[:, 512:] ctx   (E2 = tgt_embedding W_ih[:, :512]^T + b_ih: step-invariant, built once per parameter set)
//   gh = W_hh s + b_hh;  s' = GRU gates;  logits = fc(s')
// The weights are read TRANSPOSED ([k][out], prepared once per parameter set): a thread owns one output, walks k, reads its weight
// coalesced with its neighbours' and the rows' activations as LDS broadcasts, so one weight read serves all the image's rows and no
// product is reduced across lanes.  Every dot product runs as 4 interleaved chains (k mod 4) summed pairwise at the end.
#define AD_D 512          // sDim = attDim = xDim
#define AD_MAXT 32
#define AD_MAXC 128
#define AD_MAXL 100
#define AD_THREADS 512

struct AttnDecArgs {
    const float *x, *xproj, *WsT, *bs, *wv, *wb, *E2, *WicT, *WhhT, *bhh, *fcT, *fcb;
    const int* targets;
    float* logits;
    int* ids;
    float* scores;
    int B, T, C, L, eos, mode;
};

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float sum4(const float* c) { return (c[0] + c[1]) + (c[2] + c[3]); }
__device__ __forceinline__ float comp(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
// candidate order of the beam: score descending, then flat index ascending
__device__ __forceinline__ bool cand_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

template <int R>
__global__ __launch_bounds__(AD_THREADS) void attn_decode_kernel(AttnDecArgs a) {
    constexpr int HL = R > 1 ? AD_MAXL : 1;
    __shared__ __attribute__((aligned(16))) float sS[2][R][AD_D];        // the rows' states: current / next
    __shared__ __attribute__((aligned(16))) float sP[R][AD_D];           // sProj; later the 4 partial sums of fc ([4][R][128])
    __shared__ __attribute__((aligned(16))) float sC[R][AD_D];           // context
    __shared__ float sE[R][AD_MAXT];                                     // energies, then alpha
    __shared__ float sLog[R][AD_MAXC];
    __shared__ float sSeq[R], sMax[R], sLsum[R];
    __shared__ int sY[R], sPred[R];
    __shared__ int hSym[HL][R], hPred[HL][R], hOut[HL][R];               // the beam's stored decisions
    __shared__ float hScore[HL][R];
    __shared__ int sStop;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, C = a.C, L = a.L;
    int cur = 0;
    for (int i = tid; i < R * AD_D; i += AD_THREADS) sS[0][i / AD_D][i % AD_D] = 0.f;
    if (tid < R) { sY[tid] = C; sSeq[tid] = tid == 0 ? 0.f : -INFINITY; }
    if (tid == 0) sStop = 0;
    int done_at = L;                                                    // greedy: the step after the first EOS

    for (int step = 0; step < L; ++step) {
        __syncthreads();
        if (R > 1) {
            bool dead = true;
#pragma unroll
            for (int r = 0; r < R; ++r) dead = dead && sSeq[r] == -INFINITY;
            if (dead) {      // every beam has ended: whatever the network gives, all candidates stay at -inf and the tie rule selects
                             // flat indices 0..R-1 (beam 0, classes 0..R-1); only the bookkeeping goes on
                if (tid < R) { hSym[step][tid] = tid; hPred[step][tid] = 0; hScore[step][tid] = -INFINITY; }
                continue;
            }
        }
        // ---- sProj = sEmbed(s)
        {
            float acc[R][4];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.f;
            const float* w = a.WsT + tid;
#pragma unroll 2
            for (int k = 0; k < AD_D; k += 4) {
                float wk[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) wk[i] = w[(long)(k + i) * AD_D];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 sv = *reinterpret_cast<const float4*>(&sS[cur][r][k]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[r][i] = fmaf(wk[i], comp(sv, i), acc[r][i]);
                }
            }
            const float bias = a.bs[tid];
#pragma unroll
            for (int r = 0; r < R; ++r) sP[r][tid] = sum4(acc[r]) + bias;
        }
        __syncthreads();
        // ---- e[r][t] = wEmbed(tanh(sProj[r] + xProj[t])): one (row, position) pair per wave and trip
        {
            const float4 w0 = *reinterpret_cast<const float4*>(a.wv + lane * 4), w1 = *reinterpret_cast<const float4*>(a.wv + 256 + lane * 4);
            const float wb = a.wb[0];
            for (int p = wave; p < R * T; p += AD_THREADS / 64) {
                const int r = p / T, t = p % T;
                const float* xp = a.xproj + ((long)b * T + t) * AD_D;
                const float4 x0 = *reinterpret_cast<const float4*>(xp + lane * 4), x1 = *reinterpret_cast<const float4*>(xp + 256 + lane * 4);
                const float4 p0 = *reinterpret_cast<const float4*>(&sP[r][lane * 4]), p1 = *reinterpret_cast<const float4*>(&sP[r][256 + lane * 4]);
                float s0 = w0.x * tanhf(p0.x + x0.x) + w0.y * tanhf(p0.y + x0.y);
                float s1 = w0.z * tanhf(p0.z + x0.z) + w0.w * tanhf(p0.w + x0.w);
                float s2 = w1.x * tanhf(p1.x + x1.x) + w1.y * tanhf(p1.y + x1.y);
                float s3 = w1.z * tanhf(p1.z + x1.z) + w1.w * tanhf(p1.w + x1.w);
                const float s = wave_sum((s0 + s1) + (s2 + s3));
                if (lane == 0) sE[r][t] = s + wb;
            }
        }
        __syncthreads();
        // ---- alpha = softmax over the T positions (lanes beyond T are padding)
        if (wave < R) {
            const float v = lane < T ? sE[wave][lane] : -INFINITY;
            const float m = wave_max_f(v);
            const float e = lane < T ? expf(v - m) : 0.f;
            const float s = wave_sum(e);
            if (lane < T) sE[wave][lane] = e / s;
        }
        __syncthreads();
        // ---- context
        {
            float acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = 0.f;
            const float* xb = a.x + (long)b * T * AD_D + tid;
            for (int t = 0; t < T; ++t) {
                const float xv = xb[(long)t * AD_D];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(sE[r][t], xv, acc[r]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) sC[r][tid] = acc[r];
        }
        __syncthreads();
        // ---- GRU: thread j owns hidden unit j (its three gate rows of both matrices)
        {
            float ar[R][4], az[R][4], ani[R][4], anh[R][4];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) ar[r][i] = az[r][i] = ani[r][i] = anh[r][i] = 0.f;
            const float* wi = a.WicT + tid;
            const float* wh = a.WhhT + tid;
#pragma unroll 1
            for (int k = 0; k < AD_D; k += 4) {
                float ir[4], iz[4], in_[4], hr[4], hz[4], hn[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long o = (long)(k + i) * (3 * AD_D);
                    ir[i] = wi[o]; iz[i] = wi[o + AD_D]; in_[i] = wi[o + 2 * AD_D];
                    hr[i] = wh[o]; hz[i] = wh[o + AD_D]; hn[i] = wh[o + 2 * AD_D];
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 cv = *reinterpret_cast<const float4*>(&sC[r][k]);
                    const float4 hv = *reinterpret_cast<const float4*>(&sS[cur][r][k]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float c = comp(cv, i), h = comp(hv, i);
                        ar[r][i] = fmaf(ir[i], c, ar[r][i]); ar[r][i] = fmaf(hr[i], h, ar[r][i]);
                        az[r][i] = fmaf(iz[i], c, az[r][i]); az[r][i] = fmaf(hz[i], h, az[r][i]);
                        ani[r][i] = fmaf(in_[i], c, ani[r][i]);
                        anh[r][i] = fmaf(hn[i], h, anh[r][i]);
                    }
                }
            }
            const float br = a.bhh[tid], bz = a.bhh[AD_D + tid], bn = a.bhh[2 * AD_D + tid];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float* e2 = a.E2 + (long)sY[r] * (3 * AD_D);
                const float rg = sigmoid_acc((sum4(ar[r]) + e2[tid]) + br);
                const float zg = sigmoid_acc((sum4(az[r]) + e2[AD_D + tid]) + bz);
                const float n = tanhf((sum4(ani[r]) + e2[2 * AD_D + tid]) + rg * (sum4(anh[r]) + bn));
                sS[cur ^ 1][r][tid] = (1.f - zg) * n + zg * sS[cur][r][tid];
            }
        }
        __syncthreads();
        // ---- logits = fc(s'): 4 quarters of k x 128 classes, partial sums through LDS
        {
            float (*part)[R][AD_MAXC] = reinterpret_cast<float (*)[R][AD_MAXC]>(&sP[0][0]);
            const int q = tid >> 7, c = tid & 127;
            if (c < C) {
                float acc[R];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = 0.f;
                const float* w = a.fcT + c;
                for (int k = q * 128; k < q * 128 + 128; k += 4) {
                    float wk[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) wk[i] = w[(long)(k + i) * C];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float4 hv = *reinterpret_cast<const float4*>(&sS[cur ^ 1][r][k]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[r] = fmaf(wk[i], comp(hv, i), acc[r]);
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) part[q][r][c] = acc[r];
            }
            __syncthreads();
            for (int i = tid; i < R * AD_MAXC; i += AD_THREADS) {
                const int r = i >> 7, cc = i & 127;
                if (cc < C) sLog[r][cc] = ((part[0][r][cc] + part[1][r][cc]) + (part[2][r][cc] + part[3][r][cc])) + a.fcb[cc];
            }
        }
        __syncthreads();
        // ---- what the mode does with the logits
        if (R == 1) {
            if (a.mode == 0) {
                if (tid < C) a.logits[((long)b * L + step) * C + tid] = sLog[0][tid];
                if (tid == 0) sY[0] = min(max(a.targets[(long)b * L + step], 0), C);      // (E2 has C + 1 rows)
            } else if (wave == 0) {
                const float v0 = lane < C ? sLog[0][lane] : -INFINITY, v1 = lane + 64 < C ? sLog[0][lane + 64] : -INFINITY;
                float bv = v0; int bi = lane;
                if (v1 > v0) { bv = v1; bi = lane + 64; }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
                    if (cand_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
                }
                const float s = wave_sum((lane < C ? expf(v0 - bv) : 0.f) + (lane + 64 < C ? expf(v1 - bv) : 0.f));
                if (lane == 0) {
                    a.ids[(long)b * L + step] = bi;
                    a.scores[(long)b * L + step] = 1.f / s;
                    sY[0] = bi;
                    if (bi == a.eos) sStop = 1;
                }
            }
            cur ^= 1;
            __syncthreads();
            if (a.mode == 1 && sStop) { done_at = step + 1; break; }
        } else {
            if (wave < R) {      // log-softmax pieces of row `wave`: max and log of the sum
                const float v0 = lane < C ? sLog[wave][lane] : -INFINITY, v1 = lane + 64 < C ? sLog[wave][lane + 64] : -INFINITY;
                const float m = wave_max_f(fmaxf(v0, v1));
                const float s = wave_sum((lane < C ? expf(v0 - m) : 0.f) + (lane + 64 < C ? expf(v1 - m) : 0.f));
                if (lane == 0) { sMax[wave] = m; sLsum[wave] = logf(s); }
            }
            __syncthreads();
            if (wave == 0) {     // the R best of the R * C candidates seq[r] + log_softmax[r][c], flat index f = r * C + c
                constexpr int PER = (R * AD_MAXC) / 64;
                float cv[PER]; int ci[PER];
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int f = lane + 64 * i;
                    if (f < R * C) {
                        const int r = f / C, c = f % C;
                        cv[i] = sSeq[r] + ((sLog[r][c] - sMax[r]) - sLsum[r]); ci[i] = f;
                    } else { cv[i] = -INFINITY; ci[i] = 0x7fffffff; }
                }
                float nseq = 0.f; int nsym = 0, npred = 0;
                for (int kk = 0; kk < R; ++kk) {
                    float bv = cv[0]; int bi = ci[0];
#pragma unroll
                    for (int i = 1; i < PER; ++i) if (cand_before(cv[i], ci[i], bv, bi)) { bv = cv[i]; bi = ci[i]; }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
                        if (cand_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
                    }
#pragma unroll
                    for (int i = 0; i < PER; ++i) if (ci[i] == bi) { cv[i] = -INFINITY; ci[i] = 0x7fffffff; }      // taken
                    if (lane == kk) { nseq = bv; nsym = bi % C; npred = min(bi / C, R - 1); }      // (the clamp only matters for NaN scores)
                }
                if (lane < R) {
                    hSym[step][lane] = nsym; hPred[step][lane] = npred; hScore[step][lane] = nseq;
                    sY[lane] = nsym; sPred[lane] = npred;
                    sSeq[lane] = nsym == a.eos ? -INFINITY : nseq;
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) sS[cur][r][tid] = sS[cur ^ 1][sPred[r]][tid];      // state.index_select(predecessors)
        }
    }
    __syncthreads();
    if (R == 1) {
        // greedy: beyond the first EOS the ids are EOS and the scores 0 (the reference goes on decoding there; nothing reads it)
        if (a.mode == 1)
            for (int t = done_at + tid; t < L; t += AD_THREADS) { a.ids[(long)b * L + t] = a.eos; a.scores[(long)b * L + t] = 0.f; }
        return;
    }
    // ---- the beam's backtracking (attention_recognition_head.py:127-187), on this image's R slots
    if (tid == 0) {
        int tp[R]; float s[R]; bool used[R];
        for (int k = 0; k < R; ++k) used[k] = false;
        for (int k = 0; k < R; ++k) {                 // stored_scores[-1].topk(R)
            int best = -1;
            for (int j = 0; j < R; ++j)
                if (!used[j] && (best < 0 || cand_before(hScore[L - 1][j], j, hScore[L - 1][best], best))) best = j;
            used[best] = true; tp[k] = best; s[k] = hScore[L - 1][best];
        }
        int found = 0;
        for (int t = L - 1; t >= 0; --t) {
            int cs[R], np[R];
            for (int k = 0; k < R; ++k) { cs[k] = hSym[t][tp[k]]; np[k] = hPred[t][tp[k]]; }
            for (int k = 0; k < R; ++k) tp[k] = np[k];
            for (int j = R - 1; j >= 0; --j)
                if (hSym[t][j] == a.eos) {
                    const int rk = R - (found % R) - 1;
                    ++found;
                    tp[rk] = hPred[t][j]; cs[rk] = hSym[t][j]; s[rk] = hScore[t][j];
                }
            for (int k = 0; k < R; ++k) hOut[t][k] = cs[k];
        }
        int best = 0;                                 // s.topk(R)[0]
        for (int k = 1; k < R; ++k) if (cand_before(s[k], k, s[best], best)) best = k;
        sPred[0] = best;
    }
    __syncthreads();
    for (int t = tid; t < L; t += AD_THREADS) { a.ids[(long)b * L + t] = hOut[t][sPred[0]]; a.scores[(long)b * L + t] = 1.f; }
}

TATT_API int tatt_attn_decode(const float* x, const float* xproj, const float* WsT, const float* bs, const float* wv, const float* wb,
                              const float* E2, const float* WicT, const float* WhhT, const float* bhh, const float* fcT,
                              const float* fcb, const int* targets, float* logits, int* ids, float* scores, int B, int T, int C, int L,
                              int sDim, int attDim, int xDim, int eos, int mode, int beam, hipStream_t st) {
    if (sDim != AD_D || attDim != AD_D || xDim != AD_D) return 1;
    if (B < 1 || T < 1 || T > AD_MAXT || C < 2 || C > AD_MAXC || L < 1 || L > AD_MAXL || mode < 0 || mode > 2) return 1;
    if (mode == 0 && (!targets || !logits)) return 1;
    if (mode != 0 && (!ids || !scores)) return 1;
    if (mode == 2 && (beam != 5 || C < 5)) return 1;
    AttnDecArgs a = {x, xproj, WsT, bs, wv, wb, E2, WicT, WhhT, bhh, fcT, fcb, targets, logits, ids, scores, B, T, C, L, eos, mode};
    if (mode == 2) hipLaunchKernelGGL(attn_decode_kernel<5>, dim3(B), dim3(AD_THREADS), 0, st, a);
    else hipLaunchKernelGGL(attn_decode_kernel<1>, dim3(B), dim3(AD_THREADS), 0, st, a);
    return LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The beam's backtracking alone, for the step-by-step route (the one launch does it in LDS): stored decisions sym, pred (slot of the
// previous step, clamped to [0, K)), score, each (L, B, K) -> ids (B, L) of the best sequence per image.  One thread per image (a chain of
// L dependent steps on K slots); ws (B, L, K) ints holds the sequences until the final order is known.
#define BT_MAXK 8
__global__ void beam_backtrack_kernel(const int* __restrict__ sym, const int* __restrict__ pred, const float* __restrict__ score,
                                      int* __restrict__ ids, int* __restrict__ ws, int L, int B, int K, int eos) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int tp[BT_MAXK]; float s[BT_MAXK]; bool used[BT_MAXK];
    const long last = ((long)(L - 1) * B + b) * K;
    for (int k = 0; k < K; ++k) used[k] = false;
    for (int k = 0; k < K; ++k) {
        int best = -1;
        for (int j = 0; j < K; ++j)
            if (!used[j] && (best < 0 || cand_before(score[last + j], j, score[last + best], best))) best = j;
        used[best] = true; tp[k] = best; s[k] = score[last + best];
    }
    int found = 0;
    for (int t = L - 1; t >= 0; --t) {
        const long o = ((long)t * B + b) * K;
        int cs[BT_MAXK], np[BT_MAXK];
        for (int k = 0; k < K; ++k) { cs[k] = sym[o + tp[k]]; np[k] = min(max(pred[o + tp[k]], 0), K - 1); }
        for (int k = 0; k < K; ++k) tp[k] = np[k];
        for (int j = K - 1; j >= 0; --j)
            if (sym[o + j] == eos) {
                const int rk = K - (found % K) - 1;
                ++found;
                tp[rk] = min(max(pred[o + j], 0), K - 1); cs[rk] = eos; s[rk] = score[o + j];
            }
        for (int k = 0; k < K; ++k) ws[((long)b * L + t) * K + k] = cs[k];
    }
    int best = 0;
    for (int k = 1; k < K; ++k) if (cand_before(s[k], k, s[best], best)) best = k;
    for (int t = 0; t < L; ++t) ids[(long)b * L + t] = ws[((long)b * L + t) * K + best];
}
TATT_API int tatt_beam_backtrack(const int* sym, const int* pred, const float* score, int* ids, int* ws, int L, int B, int K, int eos,
                                 hipStream_t st) {
    if (L < 1 || B < 1 || K < 1 || K > BT_MAXK) return 1;
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, sym, pred, score, ids, ws, L, B, K, eos);
    return LAUNCH_CHECK();
}
