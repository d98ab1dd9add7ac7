// Per-line lexicons of the line reader (tatt_amd/read.py `ctc_line_lexicons_read_host` is the specification, tests/test_line_lexicons*.py
// hold the kernels to it): every line of a chunk is read against a list of words of its OWN, so the launch takes a LIST OF (line, word)
// PAIRS where ctclex.hip takes the full product of lines and words.
//   ctc_lexicon_pairs_kernel      one work-group per TILE: a row (line b of the chunk, segment class G, first pair, pair count <= 256 / G)
//                                 of the host's tile table; a pair is (packed position in the union of all lists, position j in the
//                                 line's own list).  1-D grid, no empty work-groups: a line of 1,000 words beside 47 of 50 costs the
//                                 tiles of its pairs and nothing else.  The work-group stages its line's logits into LDS as
//                                 ctc_lexicon_score_kernel does, then a segment of G lanes runs that kernel's recursion for its pair and
//                                 stores to scores[b][j].  G is the same in the whole work-group: a switch over the three bodies, so ONE
//                                 launch per chunk serves all three segment classes.
//                                 The staging is ctc_lex.h's `lx_stage`, the function ctclex.hip calls too.  The recursion is that
//                                 header's `lx_word` RESTATED in `lxp_body`, the operands in the same order: a word's score is bit for
//                                 bit the one-list path's (tests/test_line_lexicons_device_gpu.py).  Calling `lx_word` here computes
//                                 the same bytes with the same step loops, instruction for instruction, but moves them by 4 to 12
//                                 bytes, and this kernel's time follows where they lie: tatt_ctc_lexicon_score_pairs then ran 0.2 to
//                                 0.6 % slower than before the shared header, outside the run's spread (profiles/ctc_lex_core_ab.txt).
//                                 A change to the recursion is made in ctc_lex.h AND here.
//   ctc_lexicon_select_rows_kernel   ctc_lexicon_select_kernel with a count per line: K_b = counts[b] into the same `lx_select`, so a
//                                 line of K_b words gets the 64 bits of logz a (1, K_b) buffer gets there.  K_b = 0 writes entries = 0,
//                                 flag = 0, logz = -inf (the flag rule "every score a NaN" is kept for K_b >= 1).
// Every loop is bounded by T, C, a tile's count (<= 256 / G), a line's count (<= 65536), LX_NBEST or a literal.  Nothing is indexed by
// table DATA without a range check: a tile whose line, class or pair range is out of range, a pair whose union position or j (against
// the line's count and the row stride) is out of range writes nothing; a word whose length, code offset or codes are out of range scores
// NaN.  No atomics, no traffic between work-groups.
// Registers (hipcc's resource report, gfx950): pairs 99 VGPRs, 81 SGPRs, 4 waves per SIMD; select_rows 40 VGPRs, 8 waves per SIMD;
// scratch = 0 in both (profiles/ctc_lex_core_ab.txt).
#include "ctc_lex.h"

#define LXP_MAX_U 1048576                       // distinct words of all lines
#define LXP_TILE 4                              // ints per tile row: line | segment class | first pair | pairs
#define LXP_PAIR 2                              // ints per pair: packed union position | position in the line's list

// the words of one tile's pairs at segment class G; `flagged` and everything of the tile is the same in the whole work-group
template <int G>
__device__ __forceinline__ void lxp_body(const double* ls, const float* mx, const float* xs, bool flagged, int T, int C,
                                         const int* __restrict__ codes, int n_codes, const int* __restrict__ words, int U,
                                         const int* __restrict__ pairs, int first, int count, int limit, double* __restrict__ row) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int WPW = 64 / G;                                      // words per wave
    const int seg = lane / G, s = lane % G;
    const int slot0 = wave * WPW;
    if (slot0 >= count) return;                                      // (the whole wave; nothing below meets another wave)
    bool live = slot0 + seg < count;
    int L = 0, off = 0, j = -1;
    if (live) {
        const int* p = pairs + (long)(first + slot0 + seg) * LXP_PAIR;       // (first + count <= n_pairs: the kernel saw to it)
        const int u = p[0];
        j = p[1];
        if (u >= 0 && u < U) {
            const int* w = words + (long)u * LX_WORD;
            L = w[0];
            off = w[1];
        } else {
            live = false;                                            // no such word: nothing is written
        }
    }
    // ---- ctc_lex.h's lx_word<G>(..., live, L, off, j, limit, row) RESTATED, the operands in its order (see the top) ----
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

__global__ __launch_bounds__(LX_THREADS) void ctc_lexicon_pairs_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c,
                                                                       int T, int B, int C, const int* __restrict__ codes, int n_codes,
                                                                       const int* __restrict__ words, int U,
                                                                       const int* __restrict__ tiles, const int* __restrict__ pairs,
                                                                       int n_pairs, const int* __restrict__ counts, int max_count,
                                                                       double* __restrict__ scores, long st_sc) {
    extern __shared__ double lxp_lds[];
    double* ls = lxp_lds;                                            // [T]
    float* mx = reinterpret_cast<float*>(ls + T);                    // [T]
    float* xs = mx + T;                                              // [T][C]
    LX_SHARED int flag_sh[LX_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int* tile = tiles + (long)blockIdx.x * LXP_TILE;
    const int b = tile[0], G = tile[1], first = tile[2], count = tile[3];
    if (b < 0 || b >= B || (G != 16 && G != 32 && G != 64) || count < 1 || count > LX_THREADS / G || first < 0 || first > n_pairs - count)
        return;                                                      // (the whole work-group: no such tile)
    const int kb = counts[b];
    const int limit = kb < max_count ? kb : max_count;               // j < the line's count and inside the row (max_count <= st_sc)

    const int flag = lx_stage<LX_STAGE>(logits + b * st_b, st_t, st_c, T, C, LX_THREADS / 64, ls, mx, xs);
    if (lane == 0) flag_sh[wave] = flag;
    __syncthreads();
    const bool flagged = (flag_sh[0] | flag_sh[1] | flag_sh[2] | flag_sh[3]) != 0;

    double* row = scores + b * st_sc;
    switch (G) {                                                     // (the same in the whole work-group)
    case 16: lxp_body<16>(ls, mx, xs, flagged, T, C, codes, n_codes, words, U, pairs, first, count, limit, row); break;
    case 32: lxp_body<32>(ls, mx, xs, flagged, T, C, codes, n_codes, words, U, pairs, first, count, limit, row); break;
    default: lxp_body<64>(ls, mx, xs, flagged, T, C, codes, n_codes, words, U, pairs, first, count, limit, row); break;
    }
}

__global__ __launch_bounds__(LX_THREADS) void ctc_lexicon_select_rows_kernel(const double* __restrict__ scores, long st_sc,
                                                                             const int* __restrict__ counts, int nbest,
                                                                             const int* __restrict__ index, int* __restrict__ record,
                                                                             int n_rows, long st_rec) {
    const int row = index[blockIdx.x];
    if (row < 0 || row >= n_rows) return;                            // (the whole work-group)
    const int K = counts[blockIdx.x];
    if (K < 0 || K > LX_MAX_K || K > st_sc) return;                  // (likewise: no such line)
    lx_select(scores + blockIdx.x * st_sc, K, nbest, record + row * st_rec);
}

TATT_API int tatt_ctc_lexicon_score_pairs(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* codes,
                                          int n_codes, const int* words, int U, const int* tiles, int n_tiles, const int* pairs,
                                          int n_pairs, const int* counts, int max_count, double* scores, long st_sc, hipStream_t st) {
    if (!logits || !codes || !words || !tiles || !pairs || !counts || !scores) return 1;
    if (T <= 0 || T > LX_MAX_T || C <= 0 || C > LX_MAX_C || B <= 0 || B > 65535 || U <= 0 || U > LXP_MAX_U || n_codes < 0) return 1;
    if (n_tiles <= 0 || n_pairs <= 0 || n_tiles > n_pairs || (long)n_pairs > (long)B * LX_MAX_K) return 1;
    if (max_count < 1 || max_count > LX_MAX_K || st_sc < max_count) return 1;
    int rc = 0;
    static TattPerDevice attr_once;                                  // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_lexicon_pairs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      LX_LDS_MAX);
    });
    if (rc) return rc;                                               // (beyond 64 KB of LDS the launch depends on it)
    hipLaunchKernelGGL(ctc_lexicon_pairs_kernel, dim3(n_tiles), dim3(LX_THREADS), LX_STAGE_LDS(T, C), st, logits, st_t, st_b, st_c, T, B, C,
                       codes, n_codes, words, U, tiles, pairs, n_pairs, counts, max_count, scores, st_sc);
    return LAUNCH_CHECK();
}

TATT_API int tatt_ctc_lexicon_select_rows(const double* scores, long st_sc, int B, const int* counts, int nbest, const int* index,
                                          int* record, int n_rows, long st_rec, hipStream_t st) {
    if (!scores || !counts || !index || !record) return 1;
    if (B <= 0 || st_sc < 1 || nbest < 1 || nbest > LX_NBEST || n_rows <= 0 || st_rec < lx_record_words(nbest))
        return 1;
    hipLaunchKernelGGL(ctc_lexicon_select_rows_kernel, dim3(B), dim3(LX_THREADS), 0, st, scores, st_sc, counts, nbest, index, record,
                       n_rows, st_rec);
    return LAUNCH_CHECK();
}

TATT_API int tatt_line_lexicons_limits(int* out) {
    if (!out) return 1;
    out[0] = LX_MAX_T;
    out[1] = LX_MAX_C;
    out[2] = LX_MAX_L;
    out[3] = LX_MAX_K;
    out[4] = LXP_MAX_U;
    out[5] = LX_NBEST;
    return 0;
}
