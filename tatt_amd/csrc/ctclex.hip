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
// The staging (`lx_stage`), a word's recursion (`lx_word`) and the selection (`lx_select`) described above are the text of ctc_lex.h,
// which ctclexp.hip and ctcwords.hip include too (who calls what: there); the kernels here fetch a segment's word, or a line's row, and
// call them.
// Registers (hipcc's resource report, gfx950): score <16>, <32>, <64> 99 VGPRs, 62 SGPRs, 4 waves per SIMD; select 40 VGPRs, 54 SGPRs,
// 8 waves per SIMD; scratch = 0 in all (profiles/ctc_lex_core_ab.txt).
#include "ctc_lex.h"

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

    const int flag = lx_stage<LX_STAGE>(logits + b * st_b, st_t, st_c, T, C, LX_THREADS / 64, ls, mx, xs);
    if (lane == 0) flag_sh[wave] = flag;
    __syncthreads();
    const bool flagged = (flag_sh[0] | flag_sh[1] | flag_sh[2] | flag_sh[3]) != 0;

    // ---- the segment's word ----
    constexpr int WPW = 64 / G;                                      // words per wave
    const int seg = lane / G;
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
    lx_word<G>(ls, mx, xs, flagged, T, C, codes, n_codes, live, L, off, orig, K, scores + b * st_sc);
}

__global__ __launch_bounds__(LX_THREADS) void ctc_lexicon_select_kernel(const double* __restrict__ scores, long st_sc, int K, int nbest,
                                                                        const int* __restrict__ index, int* __restrict__ record,
                                                                        int n_rows, long st_rec) {
    const int row = index[blockIdx.x];
    if (row < 0 || row >= n_rows) return;                            // (the whole work-group)
    lx_select(scores + blockIdx.x * st_sc, K, nbest, record + row * st_rec);
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
    hipLaunchKernelGGL(ctc_lexicon_score_kernel<G>, dim3(cdiv(count, LX_THREADS / G), B), dim3(LX_THREADS), LX_STAGE_LDS(T, C), st, logits,
                       st_t, st_b, st_c, T, C, codes, n_codes, words, K, first, count, scores, st_sc);
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
