// The MORAN recogniser (reference model/moran/): the two chains of tiny dependent launches of its eval path, each as ONE launch.
//   morn_rectify : the tail of the MORN rectifier (morn.py:62-69 and :76-82): relu(+-o) -> 2x2 stride-1 max-pools -> their difference ->
//                  grid_sample at the regular grid -> offsets_grid (set or accumulated) -> grid_sample of the image at (gx, gy + offsets)
//   moran_decode : all L steps of one direction of the ASRN attention decoder (asrn_res.py:39-65,127-155), one work-group per image
// Both samplers are bilinear with zeros padding and align_corners=False, which is how the installed torch runs the reference's calls.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------------------
#define MR_MAXMAP 4096    // floats of one image's offsets map staged in LDS (the product's is 4 x 12)

struct MornGeom { int first, B, C, H, W, Ho, Wo, h, w; long xsn, xsc, xsh, xsw; };

// p[i][j] = max2x2(relu(o))[i][j] - max2x2(relu(-o))[i][j] on the (h - 1) x (w - 1) pooled map, zero outside it
__device__ __forceinline__ float morn_pooled(const float* so, int h, int w, int i, int j) {
    if (i < 0 || j < 0 || i >= h - 1 || j >= w - 1) return 0.f;
    const float a = so[i * w + j], b = so[i * w + j + 1], c = so[(i + 1) * w + j], d = so[(i + 1) * w + j + 1];
    const float pos = fmaxf(fmaxf(fmaxf(a, b), fmaxf(c, d)), 0.f);
    const float neg = fmaxf(fmaxf(fmaxf(-a, -b), fmaxf(-c, -d)), 0.f);
    return pos - neg;
}
__device__ __forceinline__ float morn_tap(const float* x, const MornGeom& g, int yi, int xi) {
    if (xi < 0 || xi >= g.W || yi < 0 || yi >= g.H) return 0.f;
    return x[yi * g.xsh + xi * g.xsw];
}
// the reference's regular grid: float64 `arange * 2. / (n - 1) - 1`, rounded to fp32 once
__device__ __forceinline__ float morn_coord(int i, int n) { return (float)((double)i * 2.0 / (double)(n - 1) - 1.0); }

// grid (cdiv(Ho * Wo, 256), B): one thread per output pixel, a work-group stays inside one image
__global__ __launch_bounds__(256) void morn_rectify_kernel(const float* __restrict__ o, float* __restrict__ acc,
                                                           const float* __restrict__ x, float* __restrict__ out, MornGeom g) {
    __shared__ float so[MR_MAXMAP];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < g.h * g.w; i += 256) so[i] = o[(long)b * g.h * g.w + i];
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= g.Ho * g.Wo) return;
    const int oy = pix / g.Wo, ox = pix % g.Wo;
    const float gx = morn_coord(ox, g.Wo), gy = morn_coord(oy, g.Ho);
    // ---- the offsets map sampled at the regular grid (the pooled map is (h - 1) x (w - 1))
    float gval;
    {
        const float ix = ((gx + 1.f) * (float)(g.w - 1) - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)(g.h - 1) - 1.f) * 0.5f;
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float tx = ix - fx, ty = iy - fy;
        const float v00 = morn_pooled(so, g.h, g.w, y0, x0), v01 = morn_pooled(so, g.h, g.w, y0, x0 + 1);
        const float v10 = morn_pooled(so, g.h, g.w, y0 + 1, x0), v11 = morn_pooled(so, g.h, g.w, y0 + 1, x0 + 1);
        gval = v00 * (1.f - tx) * (1.f - ty) + v01 * tx * (1.f - ty) + v10 * (1.f - tx) * ty + v11 * tx * ty;
    }
    const long ai = (long)b * g.Ho * g.Wo + pix;
    const float off = g.first ? gval : acc[ai] + gval;
    acc[ai] = off;
    // ---- the image sampled at (gx, gy + offsets)
    const float sy = gy + off;
    const float ix = ((gx + 1.f) * (float)g.W - 1.f) * 0.5f, iy = ((sy + 1.f) * (float)g.H - 1.f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    // (offsets of a trained network stay within the image; the clamp keeps the int conversion defined for any input, and a tap
    // that far out reads as zero either way)
    const int x0 = (int)fminf(fmaxf(fx, -2.f), (float)g.W + 1.f), y0 = (int)fminf(fmaxf(fy, -2.f), (float)g.H + 1.f);
    const float tx = ix - fx, ty = iy - fy;
    for (int c = 0; c < g.C; ++c) {
        const float* xc = x + b * g.xsn + c * g.xsc;
        const float v00 = morn_tap(xc, g, y0, x0), v01 = morn_tap(xc, g, y0, x0 + 1);
        const float v10 = morn_tap(xc, g, y0 + 1, x0), v11 = morn_tap(xc, g, y0 + 1, x0 + 1);
        out[ai * g.C + c] = v00 * (1.f - tx) * (1.f - ty) + v01 * tx * (1.f - ty) + v10 * (1.f - tx) * ty + v11 * tx * ty;
    }
}
TATT_API int tatt_morn_rectify(const float* o, int h, int w, float* acc, int first, const float* x, long xsn, long xsc, long xsh,
                               long xsw, float* out, int B, int C, int H, int W, int Ho, int Wo, hipStream_t st) {
    if (h < 2 || w < 2 || C < 1 || C > 4 || (long)h * w > MR_MAXMAP) return 1;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || Ho < 2 || Wo < 2 || (long)Ho * Wo > (1L << 24)) return 1;
    MornGeom g = {first ? 1 : 0, B, C, H, W, Ho, Wo, h, w, xsn, xsc, xsh, xsw};
    hipLaunchKernelGGL(morn_rectify_kernel, dim3(cdiv((long)Ho * Wo, 256), B), dim3(256), 0, st, o, acc, x, out, g);
    return LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The attention decoder, all L steps of one direction in one launch.
//
// One work-group of 256 threads per image; nothing is exchanged between work-groups, so the launch has no in-flight synchronisation,
// no residency requirement and no wait that could expire.  Per step (AttentionCell.forward / Attention.forward with test=True):
//   hp = h2h(h);  e_t = score(tanh(fproj_t + hp));  alpha = softmax_t(e);  ctx = sum_t alpha_t feats_t
//   gi = W_ih[:, :256] ctx + E2[y]   (E2 = char_embeddings W_ih[:, 256:]^T + b_ih: step-invariant, built once per parameter set)
//   gh = W_hh h + b_hh;  h' = GRU gates;  logits = generator(h');  y = argmax + 1 (greedy) or the next target (forced)
// The weights are read TRANSPOSED ([k][out]): thread j owns h2h_j and the three gates of hidden unit j, walks k, reads its weights
// coalesced with its neighbours' and the activations as LDS broadcasts; no product is reduced across lanes.  Every dot product runs as
// 4 interleaved chains (k mod 4) summed pairwise at the end.  The image's feats and fproj rows live in LDS for all steps.
#define MD_H 256          // hidden = feature = embedding size
#define MD_MAXT 32
#define MD_MAXC 64
#define MD_MAXL 64

struct MoranDecArgs {
    const float *feats, *fproj, *WhT, *bh, *wv, *E2, *WicT, *WhhT, *bhh, *genT, *genb;
    const int* targets;
    float* logits;
    int* ids;
    int B, T, C, L, mode;
};

__device__ __forceinline__ float md_sum4(const float* c) { return (c[0] + c[1]) + (c[2] + c[3]); }
__device__ __forceinline__ float md_comp(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
__device__ __forceinline__ float md_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float md_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(MD_H) void moran_decode_kernel(MoranDecArgs a) {
    extern __shared__ __attribute__((aligned(16))) float md_lds[];      // feats [T][256] | fproj [T][256]
    __shared__ __attribute__((aligned(16))) float sH[2][MD_H];           // the state: current / next
    __shared__ __attribute__((aligned(16))) float sP[MD_H];              // h2h(h); later the 4 partial sums of the generator ([4][64])
    __shared__ __attribute__((aligned(16))) float sC[MD_H];              // context
    __shared__ float sE[MD_MAXT];                                        // energies, then alpha
    __shared__ float sLog[MD_MAXC];
    __shared__ int sY;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, C = a.C, L = a.L;
    float* sF = md_lds;
    float* sFP = md_lds + T * MD_H;
    for (int i = tid; i < T * MD_H / 4; i += MD_H) {
        reinterpret_cast<float4*>(sF)[i] = reinterpret_cast<const float4*>(a.feats + (long)b * T * MD_H)[i];
        reinterpret_cast<float4*>(sFP)[i] = reinterpret_cast<const float4*>(a.fproj + (long)b * T * MD_H)[i];
    }
    sH[0][tid] = 0.f;
    if (tid == 0) sY = a.mode == 0 ? min(max(a.targets[(long)b * L], 0), C) : 0;
    int cur = 0;

    for (int step = 0; step < L; ++step) {
        __syncthreads();
        // ---- hp = h2h(h)
        {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            const float* w = a.WhT + tid;
#pragma unroll 4
            for (int k = 0; k < MD_H; k += 4) {
                const float4 hv = *reinterpret_cast<const float4*>(&sH[cur][k]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(w[(long)(k + i) * MD_H], md_comp(hv, i), acc[i]);
            }
            sP[tid] = md_sum4(acc) + a.bh[tid];
        }
        __syncthreads();
        // ---- e[t] = score(tanh(fproj[t] + hp)): one position per wave and trip, a lane holds 4 of the 256 terms
        {
            const float4 w0 = *reinterpret_cast<const float4*>(a.wv + lane * 4);
            const float4 p0 = *reinterpret_cast<const float4*>(&sP[lane * 4]);
            for (int t = wave; t < T; t += MD_H / 64) {
                const float4 x0 = *reinterpret_cast<const float4*>(&sFP[t * MD_H + lane * 4]);
                const float s0 = w0.x * tanhf(p0.x + x0.x) + w0.y * tanhf(p0.y + x0.y);
                const float s1 = w0.z * tanhf(p0.z + x0.z) + w0.w * tanhf(p0.w + x0.w);
                const float s = wave_sum(s0 + s1);
                if (lane == 0) sE[t] = s;
            }
        }
        __syncthreads();
        // ---- alpha = softmax over the T positions (lanes beyond T are padding)
        if (wave == 0) {
            const float v = lane < T ? sE[lane] : -INFINITY;
            const float m = md_wave_max(v);
            const float e = lane < T ? expf(v - m) : 0.f;
            const float s = wave_sum(e);
            if (lane < T) sE[lane] = e / s;
        }
        __syncthreads();
        // ---- context
        {
            float acc = 0.f;
            for (int t = 0; t < T; ++t) acc = fmaf(sE[t], sF[t * MD_H + tid], acc);
            sC[tid] = acc;
        }
        __syncthreads();
        // ---- GRU: thread j owns hidden unit j (its three gate rows of both matrices)
        {
            float ar[4], az[4], ani[4], anh[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ar[i] = az[i] = ani[i] = anh[i] = 0.f;
            const float* wi = a.WicT + tid;
            const float* wh = a.WhhT + tid;
#pragma unroll 2
            for (int k = 0; k < MD_H; k += 4) {
                const float4 cv = *reinterpret_cast<const float4*>(&sC[k]);
                const float4 hv = *reinterpret_cast<const float4*>(&sH[cur][k]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long o = (long)(k + i) * (3 * MD_H);
                    const float c = md_comp(cv, i), h = md_comp(hv, i);
                    ar[i] = fmaf(wi[o], c, ar[i]); ar[i] = fmaf(wh[o], h, ar[i]);
                    az[i] = fmaf(wi[o + MD_H], c, az[i]); az[i] = fmaf(wh[o + MD_H], h, az[i]);
                    ani[i] = fmaf(wi[o + 2 * MD_H], c, ani[i]);
                    anh[i] = fmaf(wh[o + 2 * MD_H], h, anh[i]);
                }
            }
            const float* e2 = a.E2 + (long)sY * (3 * MD_H);
            const float rg = md_sigmoid((md_sum4(ar) + e2[tid]) + a.bhh[tid]);
            const float zg = md_sigmoid((md_sum4(az) + e2[MD_H + tid]) + a.bhh[MD_H + tid]);
            const float n = tanhf((md_sum4(ani) + e2[2 * MD_H + tid]) + rg * (md_sum4(anh) + a.bhh[2 * MD_H + tid]));
            sH[cur ^ 1][tid] = (1.f - zg) * n + zg * sH[cur][tid];
        }
        __syncthreads();
        // ---- logits = generator(h'): 4 quarters of k x 64 classes, partial sums through LDS
        {
            const int q = tid >> 6, c = tid & 63;
            if (c < C) {
                float acc = 0.f;
                const float* w = a.genT + c;
                for (int k = q * 64; k < q * 64 + 64; k += 4) {
                    const float4 hv = *reinterpret_cast<const float4*>(&sH[cur ^ 1][k]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc = fmaf(w[(long)(k + i) * C], md_comp(hv, i), acc);
                }
                sP[q * MD_MAXC + c] = acc;
            }
            __syncthreads();
            if (tid < C) {
                const float v = ((sP[tid] + sP[MD_MAXC + tid]) + (sP[2 * MD_MAXC + tid] + sP[3 * MD_MAXC + tid])) + a.genb[tid];
                sLog[tid] = v;
                a.logits[((long)b * L + step) * C + tid] = v;
            }
        }
        __syncthreads();
        // ---- the next step's embedding row
        if (a.mode == 0) {
            if (tid == 0 && step + 1 < L) sY = min(max(a.targets[(long)b * L + step + 1], 0), C);      // (E2 has C + 1 rows)
        } else if (wave == 0) {
            float bv = lane < C ? sLog[lane] : -INFINITY;
            int bi = lane;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }      // ties go to the lower class
            }
            bi = min(bi, C - 1);                                                  // (only matters for NaN logits)
            if (lane == 0) { a.ids[(long)b * L + step] = bi; sY = bi + 1; }
        }
        cur ^= 1;
    }
}

static TattPerDevice md_attr_site;

TATT_API int tatt_moran_decode(const float* feats, const float* fproj, const float* WhT, const float* bh, const float* wv,
                               const float* E2, const float* WicT, const float* WhhT, const float* bhh, const float* genT,
                               const float* genb, const int* targets, float* logits, int* ids, int B, int T, int C, int L, int H,
                               int mode, hipStream_t st) {
    if (H != MD_H) return 1;
    if (B < 1 || T < 1 || T > MD_MAXT || C < 2 || C > MD_MAXC || L < 1 || L > MD_MAXL || mode < 0 || mode > 1) return 1;
    if (!logits || (mode == 0 && !targets) || (mode == 1 && !ids)) return 1;
    tatt_per_device(md_attr_site, [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(moran_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  2 * MD_MAXT * MD_H * (int)sizeof(float));
    });
    MoranDecArgs a = {feats, fproj, WhT, bh, wv, E2, WicT, WhhT, bhh, genT, genb, targets, logits, ids, B, T, C, L, mode};
    hipLaunchKernelGGL(moran_decode_kernel, dim3(B), dim3(MD_H), 2 * T * MD_H * sizeof(float), st, a);
    return LAUNCH_CHECK();
}
