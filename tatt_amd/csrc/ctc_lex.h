// The CTC lexicon core: what the three closed-list decoders of the line reader -- ctclex.hip (one list for all lines), ctclexp.hip (a list
// per line) and ctcwords.hip (word segmentation) -- have in common, stated once: the limits and the record layout, the staging of a
// line's logits into LDS, the alpha recursion of one word on a segment of lanes, and the N-best selection over a row of scores.
// The kernels, their grids, their LDS layouts and their argument checks stay in the three files.
// Who calls what: the limits and the record layout serve all three; `lx_select` both select kernels; `lx_stage` the score and the pairs
// kernel; `lx_word` the score kernel.  Two copies remain, each marked RESTATED where it stands and to be changed WITH the function here:
// ctc_words_kernel's staging loop (`lx_stage<WD_STAGE>` with the work-group's own wave count) and the recursion in ctclexp.hip's
// `lxp_body` (`lx_word`).  Both compute the same bytes through the functions, with the same step loops instruction for instruction; the
// calls move those loops by 4 to 16 bytes and the two entries' times follow where the loops lie (profiles/ctc_lex_core_ab.txt has
// the measurements: fold them in when a compiler places the code differently).
// This header is compiled under -ffp-contract=fast (ctclex.hip, ctclexp.hip) and under -ffp-contract=off (ctcwords.hip), and a word's
// score must not depend on which: it holds NO floating-point multiply, so nothing in it can contract into a fused multiply-add (float64
// subtractions, additions, comparisons, exp, log and log1p only).  Keep it so.
// It also compiles for the CPU stand-in of tools/words_host (TATT_HOST_STANDIN): no intrinsic beyond those that stand-in emulates.
#pragma once
#include "common.h"
#include "ctc_f64.h"

#define LX_MAX_T 256
#define LX_MAX_C 64
#define LX_MAX_L 31                            // 2 L + 1 states fit the 64 lanes of a wave
#define LX_MAX_K 65536                         // words of one list
#define LX_NBEST 16
#define LX_THREADS 256                         // of the score, pairs and select kernels
#define LX_STAGE 8                             // steps a wave of those kernels has in flight while it stages
#define LX_WORD 4                              // ints per packed word: length | offset of its codes | the caller's index | 0
#define LX_STAGE_LDS(T, C) ((size_t)(T) * (8 + 4 + 4 * (size_t)(C)))           // the staged logits: ls [T] | mx [T] | xs [T][C]
#define LX_LDS_MAX (LX_MAX_T * (8 + 4 + 4 * LX_MAX_C))

static_assert(2 * LX_MAX_L + 1 <= 64, "a word's states fit a wave");

#ifdef TATT_HOST_STANDIN                        // (work-groups run one after the other, a lane is a thread)
#define LX_SHARED static
#else
#define LX_SHARED __shared__
#endif

// 32-bit words of a record row: entries | flag | logz (2) | per entry logp (2), word index, 0
static inline long lx_record_words(int nbest) { return 4 + 4 * (long)nbest; }

// Staging: a wave per step, lane = class, STAGE steps in flight; `line` is the line's logits, `waves` the waves of the work-group.
// xs[t][c] = the logit, mx[t] = the step's maximum (fp32), ls[t] = log sum exp(double(x) - double(mx)) (float64).  Returns this WAVE's
// flag: a NaN, a +inf or a step without a finite logit among its steps (the work-group combines the flags behind a barrier).
template <int STAGE>
__device__ __forceinline__ int lx_stage(const float* __restrict__ line, long st_t, long st_c, int T, int C, int waves, double* ls,
                                        float* mx, float* xs) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* x = line + lane * st_c;
    int flag = 0;
    for (int t0 = wave; t0 < T && !flag; t0 += waves * STAGE) {
        float xv[STAGE];
#pragma unroll
        for (int u = 0; u < STAGE; ++u) {
            const int t = t0 + waves * u;
            xv[u] = lane < C && t < T ? x[t * st_t] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < STAGE; ++u) {
            const int t = t0 + waves * u;
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
    return flag;
}

// The alpha recursion of one word on its segment of G lanes (lane s of the segment = state s): the word has length L and its codes at
// codes[off ..]; row[j] takes its score where 0 <= j < limit.  `live`: the segment has a word at all; `flagged` (the same in the whole
// work-group): the line's scores are NaN.  A word whose length, offset or codes are out of range scores NaN.  Called by whole waves.
template <int G>
__device__ __forceinline__ void lx_word(const double* ls, const float* mx, const float* xs, bool flagged, int T, int C,
                                        const int* __restrict__ codes, int n_codes, bool live, int L, int off, int j, int limit,
                                        double* __restrict__ row) {
    const int lane = threadIdx.x & 63, seg = lane / G, s = lane % G;
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
    const bool out = live && s == S - 1 && j >= 0 && j < limit;      // the lane that holds alpha[S - 1] stores
    double* dst = row + (out ? j : 0);
    if (flagged) {
        if (out) *dst = __builtin_nan("");
        return;
    }

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

// The N-best selection of one work-group of LX_THREADS threads over the K scores of sc (K the same in every thread, 0 <= K): the nbest
// largest finite scores (comparisons only: exact), ties to the lower index, and logz = m + log sum exp(score - m) over ALL K into rec.
// The flag "every score a NaN" (a flagged line) is kept for K >= 1: K = 0 writes entries = 0, flag = 0, logz = -inf.
__device__ __forceinline__ void lx_select(const double* __restrict__ sc, int K, int nbest, int* __restrict__ rec) {
    LX_SHARED double rv[LX_THREADS];
    LX_SHARED int ri[LX_THREADS];
    const int tid = threadIdx.x;
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
    // ---- logz over ALL K words, and whether every score is a NaN ----
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
        const int flag = K >= 1 && ri[0] == K;
        const double logz = flag ? __builtin_nan("") : (n_out > 0 ? top + log(rv[0]) : CB_NEG);
        rec[0] = n_out;
        rec[1] = flag;
        rec[2] = __double2loint(logz);
        rec[3] = __double2hiint(logz);
    }
}
