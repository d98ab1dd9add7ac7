// CTC loss for the label term of the training step (reference: torch.nn.CTCLoss(blank=0, reduction='none'),
// interfaces/super_resolution.py:51, used under --use_label at :827-851).  ONE launch fuses what the reference runs as three operators
// (log_softmax, the CTC forward recursion, the CTC backward): per sample the negative log-likelihood and the UNIT gradient w.r.t. the
// un-normalised scores; a second, element-wise launch scales that gradient by the incoming one.
//
// Every label quantity (codes, offsets, target lengths, input lengths) is read from DEVICE memory, so a captured launch sees whatever the
// buffers hold when it is replayed.
//
// Layout: one work-group (4 waves) per sample.
//   phase A  all waves   rows t = wave, wave + 4, ...: lane = class (two per lane, C <= 128); row log-softmax by wave butterflies (or a
//                        plain copy when the input already holds log-probabilities) into LDS lp[T][C]; extended labels l'[S] into LDS
//   phase B  wave 0      extended states across the lanes (s = lane, lane + 64, lane + 128): alpha_t(s) into the LDS table al[T][Smax]
//                        (neighbours s-1, s-2 are read from row t-1 of the table), nll from the last row; then beta as a rolling
//                        double-buffered vector, al[t][s] <- alpha_t(s) + beta_t(s) in place.  One wave: LDS hand-offs need no barrier.
//   phase C  all waves   wave = row, lane = class: logsumexp over the states with l'_s == c in ascending s (online, fixed order); for raw
//                        logits the row's log-softmax backward g - p sum(g) (a wave sum); gradient store
// LDS: (T*C + T*Smax + 3*Smax) floats with Smax = 2T + 1: 10 KB at T = 26, C = 37; 67.3 KB at the capacity T = 64, C = 128.
// All arithmetic fp32 in log space; logsumexp of all -inf operands is -inf.  No atomics, no cross-work-group traffic, every loop bounded by
// T, S or C.  Nothing is indexed by label DATA without a range check: a sample whose codes leave [0, C) or whose offset / length leave
// the codes array is infeasible.
#include "common.h"
#include <math.h>

#define CTC_MAX_T 64
#define CTC_MAX_C 128
#define CTC_THREADS 256
#define CTC_NS 3                       // states per lane of wave 0: 2 * CTC_MAX_T + 1 <= 64 * CTC_NS

static inline long ctc_lds_bytes(int T, int C) { return ((long)T * C + (long)(T + 3) * (2 * T + 1)) * 4; }

__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    if (!(m > -INFINITY)) return a + b + c;             // all -inf -> -inf (a NaN operand stays a NaN)
    return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// exp(lp) - exp(logsumexp_{s < s_end: l'_s = c}(ab[s]) - lp + nll): the logsumexp online in ascending s, (m, acc) with acc = sum exp(v - m)
__device__ __forceinline__ float ctc_grad_elem(const float* ab, const int* lab, int s_end, int c, float l, float nl) {
    float m = -INFINITY, acc = 0.f;
    for (int s = 0; s < s_end; ++s) {
        if (lab[s] != c) continue;
        const float v = ab[s];
        if (v == -INFINITY) continue;
        if (v > m) {
            acc = acc * expf(m - v) + 1.f;
            m = v;
        } else {
            acc += expf(v - m);                                           // (a NaN lands here and stays)
        }
    }
    float g = expf(l);
    if (acc != 0.f) g -= expf(m + logf(acc) - l + nl);
    return g;
}

__global__ __launch_bounds__(CTC_THREADS) void ctc_loss_fwd_kernel(const float* __restrict__ x, long st_t, long st_b, long st_c,
                                                                   int normalized, const int* __restrict__ codes, long n_codes,
                                                                   const int* __restrict__ offs, const int* __restrict__ tgt_len,
                                                                   const int* __restrict__ in_len, int blank, int zero_inf,
                                                                   float* __restrict__ nll, float* __restrict__ grad, int T, int B,
                                                                   int C, int Smax) {
    extern __shared__ __attribute__((aligned(16))) float ctc_smem[];
    float* lp = ctc_smem;                        // [T][C]     log-probabilities
    float* al = lp + T * C;                      // [T][Smax]  alpha, then alpha + beta
    float* br = al + T * Smax;                   // [2][Smax]  beta of the step before
    int* lab = (int*)(br + 2 * Smax);            // [Smax]     extended labels, -1 = a code outside [0, C)
    __shared__ float s_nll;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = tgt_len[b];
    const int Tin = in_len ? in_len[b] : T;
    const long off = offs[b];
    const int Tb = Tin < 0 ? 0 : (Tin > T ? T : Tin);
    const float nanv = __builtin_nanf("");
    // decided without looking at a code: ignored (L < 0), empty (no steps, no targets) or infeasible (more targets than steps, lengths
    // or offsets that leave the arrays).  Work-group uniform, before any barrier.
    const bool ignored = L < 0;
    const bool early_bad = !ignored && (Tin < 0 || Tin > T || L > Tb || off < 0 || off + (long)L > n_codes);
    if (ignored || early_bad || Tb == 0) {
        const bool loud = early_bad && !zero_inf;
        if (tid == 0) nll[b] = loud ? INFINITY : 0.f;
        if (grad)
            for (int i = tid; i < T * C; i += CTC_THREADS) {
                const int t = i / C, c = i - t * C;
                grad[((long)t * B + b) * C + c] = (loud && t < Tb) ? nanv : 0.f;
            }
        return;
    }
    const int S = 2 * L + 1;                     // <= 2 * Tb + 1 <= Smax
    // ---- phase A ----
    for (int s = tid; s < S; s += CTC_THREADS) {
        int c = blank;
        if (s & 1) {
            c = codes[off + (s >> 1)];
            if (c < 0 || c >= C) c = -1;
        }
        lab[s] = c;
    }
    for (int t = wave; t < Tb; t += CTC_THREADS / 64) {
        const float* row = x + (long)t * st_t + (long)b * st_b;
        const bool h0 = lane < C, h1 = lane + 64 < C;
        float v0 = h0 ? row[(long)lane * st_c] : -INFINITY;
        float v1 = h1 ? row[(long)(lane + 64) * st_c] : -INFINITY;
        if (!normalized) {
            float m = fmaxf(v0, v1);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            v0 -= m;
            v1 -= m;
            const float e = wave_sum((h0 ? expf(v0) : 0.f) + (h1 ? expf(v1) : 0.f));
            const float le = logf(e);
            v0 -= le;
            v1 -= le;
        }
        if (h0) lp[t * C + lane] = v0;
        if (h1) lp[t * C + lane + 64] = v1;
    }
    __syncthreads();
    // ---- phase B ----
    if (wave == 0) {
        int lb[CTC_NS];                          // own extended label (0 when invalid: only used as an index then)
        bool have[CTC_NS], skip_dn[CTC_NS], skip_up[CTC_NS], invalid = false;
#pragma unroll
        for (int j = 0; j < CTC_NS; ++j) {
            const int s = lane + 64 * j;
            have[j] = s < S;
            const int l0 = have[j] ? lab[s] : 0;
            invalid |= l0 < 0;
            lb[j] = l0 < 0 ? 0 : l0;
            skip_dn[j] = have[j] && s > 1 && lab[s - 2] != l0;           // the transition s-2 -> s exists
            skip_up[j] = have[j] && s + 2 < S && lab[s + 2] != l0;       // the transition s -> s+2 exists
        }
        const bool bad_codes = __any(invalid);
        float ll = -INFINITY;
        if (!bad_codes) {
            // alpha
#pragma unroll
            for (int j = 0; j < CTC_NS; ++j) {
                const int s = lane + 64 * j;
                if (have[j]) al[s] = s < 2 ? lp[lb[j]] : -INFINITY;
            }
            wave_lds_sync();
            for (int t = 1; t < Tb; ++t) {
                const float* pr = al + (t - 1) * Smax;
#pragma unroll
                for (int j = 0; j < CTC_NS; ++j) {
                    const int s = lane + 64 * j;
                    if (have[j]) {
                        const float a0 = pr[s];
                        const float a1 = s > 0 ? pr[s - 1] : -INFINITY;
                        const float a2 = skip_dn[j] ? pr[s - 2] : -INFINITY;
                        al[t * Smax + s] = ctc_lse3(a0, a1, a2) + lp[t * C + lb[j]];
                    }
                }
                wave_lds_sync();
            }
            const float* last = al + (Tb - 1) * Smax;
            ll = ctc_lse3(last[S - 1], S > 1 ? last[S - 2] : -INFINITY, -INFINITY);
        }
        const bool feasible = !bad_codes && ll != -INFINITY;             // (a NaN likelihood runs on and stays a NaN)
        if (feasible && grad) {
            // beta, rolling; the table receives alpha + beta
            float bt[CTC_NS];
#pragma unroll
            for (int j = 0; j < CTC_NS; ++j) {
                const int s = lane + 64 * j;
                bt[j] = -INFINITY;
                if (have[j]) {
                    if (s >= S - 2) bt[j] = lp[(Tb - 1) * C + lb[j]];
                    br[s] = bt[j];
                    al[(Tb - 1) * Smax + s] += bt[j];
                }
            }
            wave_lds_sync();
            int cur = 0;
            for (int t = Tb - 2; t >= 0; --t) {
                const float* nx = br + cur * Smax;
                float* wr = br + (cur ^ 1) * Smax;
#pragma unroll
                for (int j = 0; j < CTC_NS; ++j) {
                    const int s = lane + 64 * j;
                    if (have[j]) {
                        const float b1 = s + 1 < S ? nx[s + 1] : -INFINITY;
                        const float b2 = skip_up[j] ? nx[s + 2] : -INFINITY;
                        bt[j] = ctc_lse3(bt[j], b1, b2) + lp[t * C + lb[j]];
                        wr[s] = bt[j];
                        al[t * Smax + s] += bt[j];
                    }
                }
                cur ^= 1;
                wave_lds_sync();
            }
        }
        if (lane == 0) s_nll = feasible ? -ll : INFINITY;
    }
    __syncthreads();
    // ---- phase C ----
    const float nl = s_nll;
    const bool infeasible = nl == INFINITY;
    if (tid == 0) nll[b] = (infeasible && zero_inf) ? 0.f : nl;
    if (!grad) return;
    // A target EQUAL to the blank is not a CTC target (torch documents "targets cannot be blank"), but the reference's collate emits [0]
    // for an empty word, and torch's CPU operator -- the yardstick of this kernel -- then ASSIGNS the last row's entry of the final
    // target's class after the final blank's, instead of adding the two: followed here so that the drop-in is exact.  Never the case for
    // the labels TextPriorSR.set_labels encodes (classes 1..36).
    const bool last_is_blank = S > 1 && lab[S - 2] == blank;
    for (int t = wave; t < T; t += CTC_THREADS / 64) {                  // wave = row, lane = class (two per lane)
        float g0 = 0.f, g1 = 0.f;
        if (t < Tb) {
            if (infeasible) {
                g0 = g1 = zero_inf ? 0.f : nanv;
            } else {
                const int s_end = (last_is_blank && t == Tb - 1) ? S - 1 : S;
                const float l0 = lane < C ? lp[t * C + lane] : 0.f, l1 = lane + 64 < C ? lp[t * C + lane + 64] : 0.f;
                if (lane < C) g0 = ctc_grad_elem(al + t * Smax, lab, s_end, lane, l0, nl);
                if (lane + 64 < C) g1 = ctc_grad_elem(al + t * Smax, lab, s_end, lane + 64, l1, nl);
                if (!normalized) {
                    // the log-softmax backward, g - p sum_c g: in exact arithmetic the row sums to 0 and this changes nothing; in fp32
                    // it takes out the common error of the row (alpha + beta + nll cancels at the magnitude of nll)
                    const float rs = wave_sum(g0 + g1);
                    if (lane < C) g0 -= expf(l0) * rs;
                    if (lane + 64 < C) g1 -= expf(l1) * rs;
                }
            }
        }
        float* go = grad + ((long)t * B + b) * C;
        if (lane < C) go[lane] = g0;
        if (lane + 64 < C) go[lane + 64] = g1;
    }
}

// dx[t,b,c] = grad[t,b,c] * gout[b]
__global__ __launch_bounds__(256) void ctc_loss_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ gout,
                                                           float* __restrict__ dx, long n, int B, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    dx[i] = grad[i] * gout[(i / C) % B];
}

TATT_API int tatt_ctc_loss_takes(int T, int C) { return T >= 1 && T <= CTC_MAX_T && C >= 1 && C <= CTC_MAX_C ? 1 : 0; }

TATT_API int tatt_ctc_loss_fwd(const float* x, long st_t, long st_b, long st_c, int normalized, const int* codes, long n_codes,
                               const int* offs, const int* tgt_len, const int* in_len, int blank, int zero_infinity, float* nll,
                               float* grad, int T, int B, int C, hipStream_t st) {
    if (!tatt_ctc_loss_takes(T, C) || B <= 0 || blank < 0 || blank >= C || n_codes < 0) return 1;
    static TattPerDevice attr_once;                 // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_loss_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ctc_lds_bytes(CTC_MAX_T, CTC_MAX_C));
    });
    hipLaunchKernelGGL(ctc_loss_fwd_kernel, dim3(B), dim3(CTC_THREADS), (size_t)ctc_lds_bytes(T, C), st, x, st_t, st_b, st_c,
                       normalized, codes, n_codes, offs, tgt_len, in_len, blank, zero_infinity, nll, grad, T, B, C, 2 * T + 1);
    return LAUNCH_CHECK();
}

TATT_API int tatt_ctc_loss_bwd(const float* grad, const float* gout, float* dx, int T, int B, int C, hipStream_t st) {
    if (T <= 0 || B <= 0 || C <= 0) return 1;
    const long n = (long)T * B * C;
    hipLaunchKernelGGL(ctc_loss_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, grad, gout, dx, n, B, C);
    return LAUNCH_CHECK();
}
