// Lexicon decoding of the line reader (tatt_amd/read.py `ctc_lexicon_read_host` is the specification, tests/test_lexicon*.py hold the
// kernels to it): the exact CTC log-probability of EVERY word of a closed list under every line's logits, then the N best words of a line.
//   ctc_lexicon_score_kernel<G>   one (line, word) pair per SEGMENT of G lanes, G = 16, 32 or 64: a word of length L has S = 2 L + 1 states
//                                 (a blank between and around its characters), one per lane, so a wave carries 64 / G words and a
//                                 work-group of four waves 256 / G.  The host sorts the words by the smallest G that holds them; a launch
//                                 covers the words of one G, grid (tiles of 256 / G words, lines).
//                                 Staging, per work-group: the line's T x C fp32 logits go into LDS once, with the step's maximum mx (fp32)
//                                 and ls = log sum exp(double(x) - double(mx)) (float64), a wave per step with lane = class.  A lane then
//                                 forms lp = (double(x[t][c]) - double(mx[t])) - ls[t], the specification's two subtractions in its order.
//                                 A NaN, a +inf or a step without a finite logit flags the line: all its scores are NaN.  After the one
//                                 barrier behind the staging the waves never meet again.
//                                 The recursion, per step, lane of state s with its class c = ext[s] in a register: a = alpha[s];
//                                 s >= 1: a = lse(a, alpha[s - 1]);  s >= 2, c != 0 and c != ext[s - 2]: a = lse(a, alpha[s - 2]);
//                                 alpha'[s] = a + lp[c] -- the specification's operands in its order.  alpha[s - 1] and alpha[s - 2] come
//                                 through data-parallel-primitive moves (a shift by one lane inside a row of 16; for G > 16 a row's lane 0
//                                 takes lane 15 of the row below it through a row broadcast): no LDS in the step loop.
//                                 The arithmetic of a word does not depend on G: the moves (`lx_below`, ctc_f64.h) are exact.
//   ctc_lexicon_select_kernel     one work-group per line: the nbest <= 16 largest finite scores (comparisons only: exact), ties to the
//                                 lower word index, logz = m + log sum exp(score - m) in float64, one record row per line.
// Every loop is bounded by T, C, K, LX_NBEST or a literal.  Nothing is indexed by lexicon DATA without a range check: a word whose length,
// code offset or codes are out of range scores NaN, one whose own index is out of range is not written.  No atomics, no traffic between
// work-groups.  All of alpha, lse and the log-soft-max are float64 (the logits are fp32).
#include "common.h"
#include "ctc_f64.h"

#define LX_MAX_T 256
#define LX_MAX_C 64
#define LX_MAX_L 31                            // 2 L + 1 states fit the 64 lanes of a wave
#define LX_MAX_K 65536
#define LX_NBEST 16
#define LX_THREADS 256
#define LX_WORD 4                              // ints per packed word: length | offset of its codes | the caller's index | 0
#define LX_STAGE 8                             // steps a wave has in flight while it stages
#define LX_LDS_MAX (LX_MAX_T * (8 + 4 + 4 * LX_MAX_C))

static_assert(2 * LX_MAX_L + 1 <= 64, "a word's states fit a wave");

template <int G>
__global__ __launch_bounds__(LX_THREADS) void ctc_lexicon_score_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c,
                                                                       int T, int C, const int* __restrict__ codes, int n_codes,
                                                                       const int* __restrict__ words, int K, int first, int count,
                                                                       double* __restrict__ scores, long st_sc) {
    extern __shared__ double lx_lds[];
    double* ls = lx_lds;                                             // [T]
    float* mx = reinterpret_cast<float*>(ls + T);                    // [T]
    float* xs = mx + T;                                              // [T][C]
    __shared__ int flag_sh[LX_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.y;

    // ---- staging: a wave per step, lane = class, LX_STAGE steps in flight ----
    const float* x = logits + b * st_b + lane * st_c;
    int flag = 0;
    for (int t0 = wave; t0 < T && !flag; t0 += 4 * LX_STAGE) {
        float xv[LX_STAGE];
#pragma unroll
        for (int u = 0; u < LX_STAGE; ++u) {
            const int t = t0 + 4 * u;
            xv[u] = lane < C && t < T ? x[t * st_t] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < LX_STAGE; ++u) {
            const int t = t0 + 4 * u;
            if (t < T && !flag) {                                    // (the same in every lane of the wave)
                const float xc = xv[u];
                const float m = cb_wave_max(xc);                     // (fmaxf skips a NaN: looked for on its own)
                if (__ballot(xc != xc || xc == INFINITY) != 0 || m == -INFINITY) {
                    flag = 1;
                } else {
                    const double s = cb_wave_sum(lane < C ? exp((double)xc - (double)m) : 0.0);
                    if (lane < C) xs[t * C + lane] = xc;
                    if (lane == 0) {
                        mx[t] = m;
                        ls[t] = log(s);
                    }
                }
            }
        }
    }
    if (lane == 0) flag_sh[wave] = flag;
    __syncthreads();
    const bool flagged = (flag_sh[0] | flag_sh[1] | flag_sh[2] | flag_sh[3]) != 0;

    // ---- the segment's word ----
    constexpr int WPW = 64 / G;                                      // words per wave
    const int seg = lane / G, s = lane % G;
    const int slot0 = (blockIdx.x * (LX_THREADS / 64) + wave) * WPW;
    if (slot0 >= count) return;                                      // (the whole wave; nothing below meets another wave)
    const bool live = slot0 + seg < count;
    int L = 0, off = 0, orig = -1;
    if (live) {
        const int* w = words + (long)(first + slot0 + seg) * LX_WORD;        // (first + count <= K: the entry saw to it)
        L = w[0];
        off = w[1];
        orig = w[2];
    }
    const bool shape_ok = L >= 0 && L <= LX_MAX_L && 2 * L + 1 <= G && off >= 0 && off <= n_codes - L;
    const int S = shape_ok ? 2 * L + 1 : 1;
    const bool on = live && s < S;
    int c = 0, below2 = 0;                                           // ext[s], ext[s - 2]
    bool bad = live && !shape_ok;
    if (on && (s & 1)) {
        c = codes[off + (s >> 1)];
        if (s >= 3) below2 = codes[off + (s >> 1) - 1];
        if (c < 1 || c >= C) {                                       // (never an index into the staged logits)
            bad = true;
            c = 0;
        }
    }
    const unsigned long long segment = (G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull) << (seg * G);
    const bool word_bad = (__ballot(bad) & segment) != 0;
    const bool skip = s >= 2 && c != 0 && c != below2;
    const bool out = live && s == S - 1 && orig >= 0 && orig < K;    // the lane that holds alpha[S - 1] stores
    double* dst = scores + b * st_sc + (out ? orig : 0);
    if (flagged) {
        if (out) *dst = __builtin_nan("");
        return;
    }

    // ---- the recursion ----
    double a = on && s <= 1 ? ((double)xs[c] - (double)mx[0]) - ls[0] : CB_NEG;
#pragma unroll 1
    for (int t = 1; t < T; ++t) {
        const double lp = ((double)xs[t * C + c] - (double)mx[t]) - ls[t];
        const double a1 = lx_below<G>(a, lane);
        const double a2 = lx_below<G>(a1, lane);
        double v = a;
        if (s >= 1) v = cb_lse(v, a1);
        if (skip) v = cb_lse(v, a2);
        a = on ? v + lp : CB_NEG;
    }
    const double a1 = lx_below<G>(a, lane);
    if (out) *dst = word_bad ? __builtin_nan("") : (S == 1 ? a : cb_lse(a, a1));
}

// 32-bit words of a record row: entries | flag | logz (2) | per entry logp (2), word index, 0
static inline long lx_record_words(int nbest) { return 4 + 4 * (long)nbest; }

__global__ __launch_bounds__(LX_THREADS) void ctc_lexicon_select_kernel(const double* __restrict__ scores, long st_sc, int K, int nbest,
                                                                        const int* __restrict__ index, int* __restrict__ record,
                                                                        int n_rows, long st_rec) {
    __shared__ double rv[LX_THREADS];
    __shared__ int ri[LX_THREADS];
    const int tid = threadIdx.x;
    const int row = index[blockIdx.x];
    if (row < 0 || row >= n_rows) return;                            // (the whole work-group)
    const double* sc = scores + blockIdx.x * st_sc;
    int* rec = record + row * st_rec;
    const double inf = __builtin_inf();
    double pv = inf, top = CB_NEG;                                   // the last pick (value, index); the first pick's value
    int pi = -1, n_out = 0;
    for (int i = 0; i < nbest; ++i) {
        // the largest finite score after the last pick in the order (value descending, index ascending)
        double bv = CB_NEG;
        int bi = 0x7fffffff;
        for (int k = tid; k < K; k += LX_THREADS) {
            const double v = sc[k];
            const bool finite = v == v && v != CB_NEG && v != inf;
            const bool after = v < pv || (v == pv && k > pi);
            if (finite && after && (v > bv || (v == bv && k < bi))) {
                bv = v;
                bi = k;
            }
        }
        rv[tid] = bv;
        ri[tid] = bi;
        __syncthreads();
        for (int o = LX_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) {
                const double ov = rv[tid + o];
                const int oi = ri[tid + o];
                if (oi != 0x7fffffff && (ri[tid] == 0x7fffffff || ov > rv[tid] || (ov == rv[tid] && oi < ri[tid]))) {
                    rv[tid] = ov;
                    ri[tid] = oi;
                }
            }
            __syncthreads();
        }
        pv = rv[0];
        pi = ri[0];
        __syncthreads();                                             // (read before the next round writes)
        if (pi == 0x7fffffff) break;                                 // fewer finite scores than nbest (the same in every thread)
        if (i == 0) top = pv;
        if (tid == 0) {
            int* e = rec + 4 + 4 * i;
            e[0] = __double2loint(pv);
            e[1] = __double2hiint(pv);
            e[2] = pi;
            e[3] = 0;
        }
        ++n_out;
    }
    // ---- logz over ALL K words, and whether every score is a NaN (a flagged line) ----
    double sum = 0.0;
    int nans = 0;
    for (int k = tid; k < K; k += LX_THREADS) {
        const double v = sc[k];
        if (v != v) ++nans;
        else if (n_out > 0 && v != inf) sum += exp(v - top);         // (exp(-inf) = 0)
    }
    rv[tid] = sum;
    ri[tid] = nans;
    __syncthreads();
    for (int o = LX_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            rv[tid] += rv[tid + o];
            ri[tid] += ri[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int flag = ri[0] == K;
        const double logz = flag ? __builtin_nan("") : (n_out > 0 ? top + log(rv[0]) : CB_NEG);
        rec[0] = n_out;
        rec[1] = flag;
        rec[2] = __double2loint(logz);
        rec[3] = __double2hiint(logz);
    }
}

template <int G>
static int lx_launch(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* codes, int n_codes,
                      const int* words, int K, int first, int count, double* scores, long st_sc, hipStream_t st) {
    if (count <= 0) return 0;
    int rc = 0;
    static TattPerDevice attr_once;                                  // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_lexicon_score_kernel<G>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, LX_LDS_MAX);
    });
    if (rc) return rc;                                               // (beyond 64 KB of LDS the launch depends on it)
    const size_t lds = (size_t)T * (8 + 4 + 4 * (size_t)C);
    hipLaunchKernelGGL(ctc_lexicon_score_kernel<G>, dim3(cdiv(count, LX_THREADS / G), B), dim3(LX_THREADS), lds, st, logits, st_t, st_b,
                       st_c, T, C, codes, n_codes, words, K, first, count, scores, st_sc);
    return 0;
}

TATT_API int tatt_ctc_lexicon_score(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* codes,
                                    int n_codes, const int* words, int K, int k16, int k32, int k64, double* scores, long st_sc,
                                    hipStream_t st) {
    if (!logits || !codes || !words || !scores) return 1;
    if (T <= 0 || T > LX_MAX_T || C <= 0 || C > LX_MAX_C || B <= 0 || B > 65535 || K <= 0 || K > LX_MAX_K || n_codes < 0) return 1;
    if (k16 < 0 || k32 < 0 || k64 < 0 || (long)k16 + k32 + k64 != K || st_sc < K) return 1;
    int rc = lx_launch<16>(logits, st_t, st_b, st_c, T, B, C, codes, n_codes, words, K, 0, k16, scores, st_sc, st);
    if (!rc) rc = lx_launch<32>(logits, st_t, st_b, st_c, T, B, C, codes, n_codes, words, K, k16, k32, scores, st_sc, st);
    if (!rc) rc = lx_launch<64>(logits, st_t, st_b, st_c, T, B, C, codes, n_codes, words, K, k16 + k32, k64, scores, st_sc, st);
    return rc ? rc : LAUNCH_CHECK();
}

TATT_API int tatt_ctc_lexicon_select(const double* scores, long st_sc, int B, int K, int nbest, const int* index, int* record, int n_rows,
                                     long st_rec, hipStream_t st) {
    if (!scores || !index || !record) return 1;
    if (B <= 0 || K <= 0 || K > LX_MAX_K || st_sc < K || nbest < 1 || nbest > LX_NBEST || n_rows <= 0 || st_rec < lx_record_words(nbest))
        return 1;
    hipLaunchKernelGGL(ctc_lexicon_select_kernel, dim3(B), dim3(LX_THREADS), 0, st, scores, st_sc, K, nbest, index, record, n_rows,
                       st_rec);
    return LAUNCH_CHECK();
}

TATT_API int tatt_lexicon_limits(int* out) {
    if (!out) return 1;
    out[0] = LX_MAX_T;
    out[1] = LX_MAX_C;
    out[2] = LX_MAX_L;
    out[3] = LX_MAX_K;
    out[4] = LX_NBEST;
    return 0;
}
