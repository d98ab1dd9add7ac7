// ImageLoss of the TATT training step (gfx950): reference loss/image_loss.py:19-34 (ImageLoss.forward, gradient=True,
// loss_weight=[1, 1e-4]) with GradientPriorLoss.gradient_map (:50-58):
//
//   loss_b = w0 * mean_{c,h,w} (sr - hr)^2  +  w1 * mean_{c<3,h,w} | G(sr) - G(hr) |
//   G(x)[h,w] = sqrt( ((x[h,w+1] - x[h,w-1]) / 2)^2 + ((x[h-1,w] - x[h+1,w]) / 2)^2 + 1e-6 )        (zero padding)
//
// The reference evaluates this with ~40 element-wise torch kernels forward and as many backward on (B,4,2H,2W) images; here
// it is one forward kernel over 16 one-wave work-groups per image and a one-wave launch that finishes the per-sample loss (and the
// batch mean * scale the training loop applies, interfaces/super_resolution.py:889-894), and one backward kernel that recomputes the
// four neighbouring gradient-map terms of every pixel instead of saving intermediate maps.  Both images are addressed by explicit strides: the SR output of the
// generator is NCHW-shaped over NHWC memory, the HR target is plain NCHW.  HBM-bound and tiny (0.8 MB per image pair).
#include "common.h"

struct ImgView {
    const float* p;
    long sn, sc, sh, sw;
};
struct LossP {
    ImgView sr, hr;
    int B, C, H, W;
    float w0, w1;
};

// Gradient-map value from the four neighbours (zero where the image ends); dx, dy are the halved central differences.  The sum of
// squares is written out in the two forms the first kernels of this file were compiled to under -ffp-contract=fast, because the last
// bit of the loss and of its gradient depends on them: sr's map as fma(dx, dx, dy * dy), hr's map (a packed multiply) as
// dx * dx + dy * dy with both products rounded.  loss_pin keeps a product from being contracted into the addition that follows it.
__device__ __forceinline__ float loss_pin(float x) {
    asm("" : "+v"(x));
    return x;
}
template <bool SR>
__device__ __forceinline__ float grad_mag(float r, float l, float t, float b, float& dx, float& dy) {
    dx = (r - l) * 0.5f;
    dy = (t - b) * 0.5f;
    const float ss = SR ? __builtin_fmaf(dx, dx, loss_pin(dy * dy)) : loss_pin(dx * dx) + loss_pin(dy * dy);
    return sqrtf(loss_pin(ss) + 1e-6f);
}
// central differences of channel plane x (pointer already offset to (n, c)) at (h, w), zero padded
template <bool SR>
__device__ __forceinline__ float grad_terms(const float* x, long sh, long sw, int h, int w, int H, int W, float& dx, float& dy) {
    const float r = (w + 1 < W) ? x[h * sh + (w + 1) * sw] : 0.f;
    const float l = (w > 0) ? x[h * sh + (w - 1) * sw] : 0.f;
    const float t = (h > 0) ? x[(h - 1) * sh + w * sw] : 0.f;
    const float b = (h + 1 < H) ? x[(h + 1) * sh + w * sw] : 0.f;
    return grad_mag<SR>(r, l, t, b, dx, dy);
}
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Forward.  The sums are those of a 1024-thread group per image -- thread t adds pixels t, t + 1024, ... in fp64, each of the 16 waves
// reduces by wave_sum_d, the 16 wave sums are added in order -- but every wave is a work-group of its own (B * 16 of them instead of
// B), leaves its two sums in ws[(n * 16 + wave) * 2 + {0, 1}], and image_loss_finish_kernel adds them: loss[n] and the mean keep their bits.
// QUAD: C == 4 and sr's channels are adjacent in memory (the generator's NHWC output): one 16-byte load per sr pixel, the centre
// and the four neighbours of both images issued before the arithmetic (clamped addresses, the padding zero selected afterwards).
#define LOSS_WAVES 16
template <bool QUAD>
__global__ __launch_bounds__(64) void image_loss_fwd_kernel(LossP p, double* __restrict__ ws) {
    const int n = blockIdx.x / LOSS_WAVES, wv = blockIdx.x % LOSS_WAVES, t = wv * 64 + threadIdx.x;
    const float* s = p.sr.p + n * p.sr.sn;
    const float* g = p.hr.p + n * p.hr.sn;
    const int gc = p.C < 3 ? p.C : 3;
    double am = 0.0, ag = 0.0;
    for (int i = t; i < p.H * p.W; i += 64 * LOSS_WAVES) {
        const int h = i / p.W, w = i - h * p.W;
        if constexpr (QUAD) {
            const bool hr_ = w + 1 < p.W, hl_ = w > 0, ht_ = h > 0, hb_ = h + 1 < p.H;
            const int wr = hr_ ? w + 1 : w, wl = hl_ ? w - 1 : w, ht = ht_ ? h - 1 : h, hb = hb_ ? h + 1 : h;
            const f32x4 sc = *reinterpret_cast<const f32x4*>(s + h * p.sr.sh + w * p.sr.sw);
            const f32x4 sR = *reinterpret_cast<const f32x4*>(s + h * p.sr.sh + wr * p.sr.sw);
            const f32x4 sL = *reinterpret_cast<const f32x4*>(s + h * p.sr.sh + wl * p.sr.sw);
            const f32x4 sT = *reinterpret_cast<const f32x4*>(s + ht * p.sr.sh + w * p.sr.sw);
            const f32x4 sB = *reinterpret_cast<const f32x4*>(s + hb * p.sr.sh + w * p.sr.sw);
            float gC[4], gR[3], gL[3], gT[3], gB[3];
#pragma unroll
            for (int c = 0; c < 4; ++c) gC[c] = g[c * p.hr.sc + h * p.hr.sh + w * p.hr.sw];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* gp = g + c * p.hr.sc;
                gR[c] = gp[h * p.hr.sh + wr * p.hr.sw];
                gL[c] = gp[h * p.hr.sh + wl * p.hr.sw];
                gT[c] = gp[ht * p.hr.sh + w * p.hr.sw];
                gB[c] = gp[hb * p.hr.sh + w * p.hr.sw];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = sc[c] - gC[c];
                am += (double)(d * d);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float dx, dy;
                const float gs = grad_mag<true>(hr_ ? sR[c] : 0.f, hl_ ? sL[c] : 0.f, ht_ ? sT[c] : 0.f, hb_ ? sB[c] : 0.f, dx, dy);
                const float gh = grad_mag<false>(hr_ ? gR[c] : 0.f, hl_ ? gL[c] : 0.f, ht_ ? gT[c] : 0.f, hb_ ? gB[c] : 0.f, dx, dy);
                ag += (double)fabsf(gs - gh);
            }
        } else {
            for (int c = 0; c < p.C; ++c) {
                const float d = s[c * p.sr.sc + h * p.sr.sh + w * p.sr.sw] - g[c * p.hr.sc + h * p.hr.sh + w * p.hr.sw];
                am += (double)(d * d);
            }
            for (int c = 0; c < gc; ++c) {
                float dx, dy;
                const float gs = grad_terms<true>(s + c * p.sr.sc, p.sr.sh, p.sr.sw, h, w, p.H, p.W, dx, dy);
                const float gh = grad_terms<false>(g + c * p.hr.sc, p.hr.sh, p.hr.sw, h, w, p.H, p.W, dx, dy);
                ag += (double)fabsf(gs - gh);
            }
        }
    }
    am = wave_sum_d(am);
    ag = wave_sum_d(ag);
    if (threadIdx.x == 0) {
        ws[(long)blockIdx.x * 2] = am;
        ws[(long)blockIdx.x * 2 + 1] = ag;
    }
}

// one wave: lane i finishes images i, i + 64, ... (the 16 wave sums in order), then the batch mean * scale when `out` is given
__global__ __launch_bounds__(64) void image_loss_finish_kernel(LossP p, const double* __restrict__ ws, float* __restrict__ loss,
                                                               float scale, float* __restrict__ out) {
    const int gc = p.C < 3 ? p.C : 3;
    const double hw = (double)p.H * p.W;
    double a = 0.0;
    for (int i = threadIdx.x; i < p.B; i += 64) {
        const double* wn = ws + (long)i * LOSS_WAVES * 2;
        double m = 0.0, q = 0.0;
#pragma unroll
        for (int k = 0; k < LOSS_WAVES; ++k) { m += wn[2 * k]; q += wn[2 * k + 1]; }
        const float l = (float)(p.w0 * m / (p.C * hw) + p.w1 * q / (gc * hw));
        loss[i] = l;
        a += (double)l;
    }
    if (!out) return;
    a = wave_sum_d(a);
    if (threadIdx.x == 0) out[0] = (float)(a / p.B * scale);
}

// d loss / d sr, one thread per pixel (all channels).  gper: per-sample upstream gradients (B) or NULL; gscalar: upstream
// gradient of the scaled batch mean (1 element) -- then every sample gets gscalar * scale_over_b.
__global__ __launch_bounds__(256) void image_loss_bwd_kernel(LossP p, const float* __restrict__ gper, const float* __restrict__ gscalar,
                                                             float scale_over_b, float* __restrict__ dsr) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long hw = (long)p.H * p.W;
    if (i >= p.B * hw) return;
    const int n = i / hw, r = i - n * hw;
    const int h = r / p.W, w = r - h * p.W;
    const float up = gper ? gper[n] : gscalar[0] * scale_over_b;
    const float* s = p.sr.p + n * p.sr.sn;
    const float* g = p.hr.p + n * p.hr.sn;
    const int gc = p.C < 3 ? p.C : 3;
    const float km = up * p.w0 * 2.f / (float)(p.C * hw);
    const float kg = up * p.w1 * 0.5f / (float)(gc * hw);
    for (int c = 0; c < p.C; ++c) {
        const long o = c * p.sr.sc + h * p.sr.sh + w * p.sr.sw;
        float v = km * (s[o] - g[c * p.hr.sc + h * p.hr.sh + w * p.hr.sw]);
        if (c < gc) {
            const float* sc = s + c * p.sr.sc;
            const float* hc = g + c * p.hr.sc;
            // pixel (h,w) is the RIGHT neighbour of (h,w-1), the LEFT one of (h,w+1), the TOP one of (h+1,w), the BOTTOM one of (h-1,w)
            float acc = 0.f;
            const int qh[4] = {h, h, h + 1, h - 1}, qw[4] = {w - 1, w + 1, w, w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (qh[k] < 0 || qh[k] >= p.H || qw[k] < 0 || qw[k] >= p.W) continue;
                float dx, dy, hx, hy;
                const float gs = grad_terms<true>(sc, p.sr.sh, p.sr.sw, qh[k], qw[k], p.H, p.W, dx, dy);
                const float gh = grad_terms<false>(hc, p.hr.sh, p.hr.sw, qh[k], qw[k], p.H, p.W, hx, hy);
                const float df = gs - gh;
                const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);          // torch: d|x| = sgn(x)
                const float term = (k < 2 ? dx : dy) / gs;
                acc = __builtin_fmaf(term, (k & 1) ? -sg : sg, acc);   // (one fused multiply-add, as compiled from the start)
            }
            v = __builtin_fmaf(kg, acc, v);
        }
        dsr[n * p.sr.sn + o] = v;
    }
}

// The same gradient for C == 4 with adjacent sr channels (16-byte aligned quads, dsr alike).  The gradient-map terms of the four
// neighbours of (h, w) read nine pixels between them: (h, w), (h, w +- 2), (h +- 2, w), (h +- 1, w +- 1).  They are loaded once, all
// before the arithmetic (clamped addresses, zero selected outside the image, which is grad_terms' padding), and every neighbour's
// term is computed from those registers with the expressions and the order of image_loss_bwd_kernel.
enum { FP_C = 0, FP_L2, FP_R2, FP_T2, FP_B2, FP_TL, FP_TR, FP_BL, FP_BR, FP_N };
__global__ __launch_bounds__(256) void image_loss_bwd_quad_kernel(LossP p, const float* __restrict__ gper, const float* __restrict__ gscalar,
                                                                  float scale_over_b, float* __restrict__ dsr) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long hw = (long)p.H * p.W;
    if (i >= p.B * hw) return;
    const int n = i / hw, r = i - n * hw;
    const int h = r / p.W, w = r - h * p.W;
    const float up = gper ? gper[n] : gscalar[0] * scale_over_b;
    const float* s = p.sr.p + n * p.sr.sn;
    const float* g = p.hr.p + n * p.hr.sn;
    const int gc = 3;
    const float km = up * p.w0 * 2.f / (float)(p.C * hw);
    const float kg = up * p.w1 * 0.5f / (float)(gc * hw);
    const int fh[FP_N] = {0, 0, 0, -2, 2, -1, -1, 1, 1}, fw[FP_N] = {0, -2, 2, 0, 0, -1, 1, -1, 1};
    f32x4 S[FP_N];
    float G[FP_N][3];
    bool in[FP_N];
#pragma unroll
    for (int f = 0; f < FP_N; ++f) {
        const int hh = h + fh[f], ww = w + fw[f];
        in[f] = hh >= 0 && hh < p.H && ww >= 0 && ww < p.W;
        const int hc = clampi(hh, p.H - 1), wc = clampi(ww, p.W - 1);
        S[f] = *reinterpret_cast<const f32x4*>(s + hc * p.sr.sh + wc * p.sr.sw);
#pragma unroll
        for (int c = 0; c < 3; ++c) G[f][c] = g[c * p.hr.sc + hc * p.hr.sh + wc * p.hr.sw];
    }
    const float g3 = g[3 * p.hr.sc + h * p.hr.sh + w * p.hr.sw];
#pragma unroll
    for (int f = 1; f < FP_N; ++f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            S[f][c] = in[f] ? S[f][c] : 0.f;
            G[f][c] = in[f] ? G[f][c] : 0.f;
        }
    }
    // neighbour k of the loop in image_loss_bwd_kernel: its (right, left, top, bottom) within the footprint
    const int nr[4] = {FP_C, FP_R2, FP_BR, FP_TR}, nl[4] = {FP_L2, FP_C, FP_BL, FP_TL};
    const int nt[4] = {FP_TL, FP_TR, FP_C, FP_T2}, nb[4] = {FP_BL, FP_BR, FP_B2, FP_C};
    const int qh[4] = {h, h, h + 1, h - 1}, qw[4] = {w - 1, w + 1, w, w};
    f32x4 out;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float v = km * (S[FP_C][c] - (c < 3 ? G[FP_C][c < 3 ? c : 0] : g3));
        if (c < gc) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (qh[k] < 0 || qh[k] >= p.H || qw[k] < 0 || qw[k] >= p.W) continue;
                float dx, dy, hx, hy;
                const float gs = grad_mag<true>(S[nr[k]][c], S[nl[k]][c], S[nt[k]][c], S[nb[k]][c], dx, dy);
                const float gh = grad_mag<false>(G[nr[k]][c < 3 ? c : 0], G[nl[k]][c < 3 ? c : 0], G[nt[k]][c < 3 ? c : 0], G[nb[k]][c < 3 ? c : 0], hx, hy);
                const float df = gs - gh;
                const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);          // torch: d|x| = sgn(x)
                const float term = (k < 2 ? dx : dy) / gs;
                acc = __builtin_fmaf(term, (k & 1) ? -sg : sg, acc);   // (one fused multiply-add, as compiled from the start)
            }
            v = __builtin_fmaf(kg, acc, v);
        }
        out[c] = v;
    }
    *reinterpret_cast<f32x4*>(dsr + n * p.sr.sn + h * p.sr.sh + w * p.sr.sw) = out;
}

static LossP make_lossp(const float* sr, long s_n, long s_c, long s_h, long s_w, const float* hr, long h_n, long h_c, long h_h,
                        long h_w, int B, int C, int H, int W, float w0, float w1) {
    LossP p = {{sr, s_n, s_c, s_h, s_w}, {hr, h_n, h_c, h_h, h_w}, B, C, H, W, w0, w1};
    return p;
}

// sr quads: four adjacent channels per pixel, every pixel on a 16-byte boundary
static bool loss_quad_route(const float* sr, long s_n, long s_c, long s_h, long s_w, int C, const float* dsr) {
    return C == 4 && s_c == 1 && s_n % 4 == 0 && s_h % 4 == 0 && s_w % 4 == 0 && ((((uintptr_t)sr) | ((uintptr_t)dsr)) & 15) == 0;
}

// loss[b] per sample; if loss_mean != NULL also loss_mean[0] = scale * mean_b loss[b].  ws: B * 32 doubles of workspace (the wave sums)
TATT_API int tatt_image_loss_fwd(const float* sr, long s_n, long s_c, long s_h, long s_w, const float* hr, long h_n, long h_c,
                                 long h_h, long h_w, float* loss, float* loss_mean, float scale, double* ws, int B, int C, int H,
                                 int W, float w0, float w1, hipStream_t st) {
    if (!ws || (((uintptr_t)ws) & 7)) return 1;
    LossP p = make_lossp(sr, s_n, s_c, s_h, s_w, hr, h_n, h_c, h_h, h_w, B, C, H, W, w0, w1);
    if (loss_quad_route(sr, s_n, s_c, s_h, s_w, C, nullptr))
        hipLaunchKernelGGL(image_loss_fwd_kernel<true>, dim3(B * LOSS_WAVES), dim3(64), 0, st, p, ws);
    else
        hipLaunchKernelGGL(image_loss_fwd_kernel<false>, dim3(B * LOSS_WAVES), dim3(64), 0, st, p, ws);
    hipLaunchKernelGGL(image_loss_finish_kernel, dim3(1), dim3(64), 0, st, p, ws, loss, scale, loss_mean);
    return LAUNCH_CHECK();
}

// dsr has the strides of sr.  Exactly one of gper (B per-sample gradients) / gscalar (gradient of the scaled mean) is non-NULL.
TATT_API int tatt_image_loss_bwd(const float* sr, long s_n, long s_c, long s_h, long s_w, const float* hr, long h_n, long h_c,
                                 long h_h, long h_w, const float* gper, const float* gscalar, float scale, float* dsr,
                                 int B, int C, int H, int W, float w0, float w1, hipStream_t st) {
    if ((gper == nullptr) == (gscalar == nullptr)) return 1;
    LossP p = make_lossp(sr, s_n, s_c, s_h, s_w, hr, h_n, h_c, h_h, h_w, B, C, H, W, w0, w1);
    const long total = (long)B * H * W;
    if (loss_quad_route(sr, s_n, s_c, s_h, s_w, C, dsr))
        hipLaunchKernelGGL(image_loss_bwd_quad_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, p, gper, gscalar, scale / B, dsr);
    else
        hipLaunchKernelGGL(image_loss_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, p, gper, gscalar, scale / B, dsr);
    return LAUNCH_CHECK();
}

// ---- SemanticLoss: the distillation loss between the student's and the teacher's text priors (reference
// loss/semantic_loss.py:21-38, used at interfaces/super_resolution.py:711):
//   L = mean |gt - pred|  +  mean (gt + e) (log(gt + e) - log(pred + e)),   e = 1e-20   (nn.KLDivLoss, reduction 'mean')
// One work-group (the priors are B x 26 x 37 values); backward w.r.t. pred only (the teacher is detached). ----
__global__ __launch_bounds__(1024) void semantic_loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt, long n,
                                                                 float* __restrict__ out) {
    __shared__ double red[16];
    double a = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const float p = pred[i], g = gt[i];
        const float ge = g + 1e-20f;
        a += (double)fabsf(g - p) + (double)(ge * (logf(ge) - logf(p + 1e-20f)));
    }
    a = wave_sum_d(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += red[k];
        out[0] = (float)(s / (double)n);
    }
}
__global__ void semantic_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ gout,
                                         long n, float* __restrict__ dpred) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p = pred[i], g = gt[i];
    const float d = g - p;
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    dpred[i] = gout[0] * (-sg - (g + 1e-20f) / (p + 1e-20f)) / (float)n;
}
TATT_API int tatt_semantic_loss_fwd(const float* pred, const float* gt, long n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(semantic_loss_fwd_kernel, dim3(1), dim3(1024), 0, st, pred, gt, n, out);
    return LAUNCH_CHECK();
}
TATT_API int tatt_semantic_loss_bwd(const float* pred, const float* gt, const float* gout, long n, float* dpred, hipStream_t st) {
    hipLaunchKernelGGL(semantic_loss_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, pred, gt, gout, n, dpred);
    return LAUNCH_CHECK();
}

// ---- calculate_psnr (reference utils/ssim_psnr.py:9-15): 20 log10(255 / sqrt(mean((255 a - 255 b)^2))) over the first 3 channels;
// +inf when the images are identical.  Strided (B,C,H,W) views like the loss above. ----
__global__ __launch_bounds__(1024) void psnr_kernel(LossP p, float* __restrict__ out) {
    __shared__ double red[16];
    const int gc = p.C < 3 ? p.C : 3;
    const long hw = (long)p.H * p.W, total = (long)p.B * gc * hw;
    double a = 0.0;
    for (long i = threadIdx.x; i < total; i += 1024) {
        const int w = i % p.W; long r = i / p.W;
        const int h = r % p.H; r /= p.H;
        const int c = r % gc; const int n = r / gc;
        const float d = 255.f * p.sr.p[n * p.sr.sn + c * p.sr.sc + h * p.sr.sh + w * p.sr.sw] -
                        255.f * p.hr.p[n * p.hr.sn + c * p.hr.sc + h * p.hr.sh + w * p.hr.sw];
        a += (double)(d * d);
    }
    a = wave_sum_d(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += red[k];
        const double mse = s / (double)total;
        out[0] = mse == 0.0 ? INFINITY : (float)(20.0 * log10(255.0 / sqrt(mse)));
    }
}
TATT_API int tatt_psnr(const float* a, long a_n, long a_c, long a_h, long a_w, const float* b, long b_n, long b_c, long b_h, long b_w,
                       float* out, int B, int C, int H, int W, hipStream_t st) {
    LossP p = make_lossp(a, a_n, a_c, a_h, a_w, b, b_n, b_c, b_h, b_w, B, C, H, W, 0.f, 0.f);
    hipLaunchKernelGGL(psnr_kernel, dim3(1), dim3(1024), 0, st, p, out);
    return LAUNCH_CHECK();
}
