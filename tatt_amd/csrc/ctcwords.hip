// Word segmentation of the line reader (tatt_amd/read.py `ctc_words_host` is the specification, tests/test_words*.py hold the kernel to
// it): the most probable alignment of a line whose collapsed string is a sequence of words of a closed list, with the span of steps of
// every word -- token passing over a CTC network.
//   ctc_words_kernel<R>   ONE work-group per line, it meets no other work-group.  The packed lexicon of ctclex.hip is laid over PACKED
//                         LANES: the k16 words take 16 lanes each, then -- from the next multiple of 64 -- the k32 words 32 each, then
//                         the k64 words 64 each, so no segment crosses a wave.  Thread tid, slot r < R holds packed lane r * threads +
//                         tid in registers: a token (float64 score, start step) and one word of constants.  Lane s of a word's segment
//                         is the state ch[s / 2] (s even) or the in-word blank bl[s / 2] (s odd), s < 2 L - 1.
//                         Staging as ctclex.hip: the line's T x C fp32 logits in LDS with mx (fp32) and ls (float64) per step, a wave per
//                         step; lp = (double(x) - double(mx)) - ls, written to lp_out where the caller asks for it.  The limits and
//                         the packed word's layout are ctc_lex.h's; the staging loop is that header's `lx_stage` RESTATED here, with
//                         WD_STAGE steps in flight and the work-group's own wave count.  Called as a function it computes the same
//                         bytes and leaves the step loop's instructions as they are, but the staging comes out 16 bytes longer and the
//                         29 KB step loop of <16>, which now starts on a 64-byte boundary, starts 16 bytes behind one:
//                         tatt_ctc_words_read ran 0.85 % slower (padded back onto the boundary: at this text's speed;
//                         profiles/ctc_lex_core_ab.txt).  A change to the staging rule is made in ctc_lex.h AND here.
//                         One step t, two barriers (one behind A, one behind B and C):
//                           A  every lane: m = own token; s >= 1: the token of lane s - 1; ch[j], j >= 1, w[j] != w[j - 1]: the token of
//                              lane s - 2; s == 0: (enter[t][w[0]] + word_penalty, start t) -- each replaces m only where STRICTLY
//                              greater, in this order; the new token is (lp + m, start of m).  The neighbours come through
//                              data-parallel-primitive moves (ctc_f64.h lx_below).  A word's last state then raises X[t][c], c its last
//                              class, by a 64-bit LDS maximum on the score's order-preserving integer image.
//                           B  the last states that hold X[t][c] lower Xrec[t][c] by a 32-bit LDS minimum on
//                              caller's index << 14 | start << 6 | first class: the lower caller's index wins a tie.
//                           C  wave 0, after its share of B, lane = class a: enter[t + 1][a], Esrc[t + 1][a], G[t + 1], Gsrc[t + 1] from G[t] and X[t][.],
//                              candidates in ascending class, only a strictly greater one replaces.
//                         Then thread 0 takes logp = max in order (G[T - 1], X[T - 1][c]) and walks Xrec / Esrc / Gsrc back (two passes
//                         of at most T words: count, then write left to right) into the line's record row.
//                         Everything after the log-soft-max is float64 addition, comparison and copies: the record equals the
//                         specification run on lp_out BIT FOR BIT.
// The back-trace tables live in LDS beside the staged logits.  Dynamic LDS at the limits (T = 256, C = 64):
//   ls 2,048 + X 1,024 + enter 512 + mx 1,024 + logits 65,536 + Xrec 65,536 + Esrc 16,384 + Gsrc 256 = 152,320 bytes of the CU's 163,840.
// Registers (hipcc's resource report, gfx950): <16> 99 VGPRs, 73 SGPRs; <1>, <2>, <4>, <8> 73 VGPRs, 70 SGPRs; scratch = 0 in all.  That
// rests on WD_OPAQUE and the sched_barrier per slot below, which keep the compiler from hoisting per-slot values out of the step loop:
// take the report again when the compiler changes (tools/kres.sh tatt_amd/csrc/ctcwords.hip; ScratchSize must stay 0).
// Every loop is bounded by T, C, R or a literal.  Nothing is indexed by lexicon DATA without a range check: a word whose length, code
// offset, codes or own index are out of range takes no part.  No traffic between work-groups.
#include "ctc_lex.h"

#define WD_THREADS 1024
#define WD_SLOTS 16                            // packed lanes a thread holds: 16 x (2 of score + start + constants) registers
#define WD_LANES (WD_THREADS * WD_SLOTS)
#define WD_STAGE 4                             // steps a wave has in flight while it stages
#define WD_NONE 0xffffffffu

static inline long wd_pad64(long v) { return (v + 63) / 64 * 64; }
// the staged logits, then X [2][64] and enter [64] (float64), Xrec (4 T C), Esrc (T C) and Gsrc (T)
static inline size_t wd_lds(int T, int C) { return LX_STAGE_LDS(T, C) + 2 * 64 * 8 + 64 * 8 + (size_t)T * C * 5 + (size_t)T; }
#define WD_LDS_MAX (LX_LDS_MAX + 2 * 64 * 8 + 64 * 8 + LX_MAX_T * LX_MAX_C * 5 + LX_MAX_T)
static_assert(WD_LDS_MAX <= 160 * 1024, "the tables of a line fit the LDS of a CU");

// constants of a packed lane, one 32-bit word
#define WD_C(m) ((m) & 63)                     // the state's class (0: an in-word blank)
#define WD_C0(m) (((m) >> 6) & 63)             // the word's first class
#define WD_ON (1 << 12)
#define WD_SKIP (1 << 13)                      // ch[j], j >= 1, w[j] != w[j - 1]: lane s - 2 is a candidate
#define WD_FIRST (1 << 14)                     // s == 0: the word is entered here
#define WD_LAST (1 << 15)                      // ch[L - 1]
#define WD_ORIG(m) ((unsigned)(m) >> 16)       // the caller's index of the word

// keeps what derives from a value from being hoisted out of the step loop and held in registers (nothing for the host stand-in of
// tools/words_host, which compiles this file for the CPU)
#ifdef TATT_HOST_STANDIN
#define WD_OPAQUE(v) ((void)(v))
#else
#define WD_OPAQUE(v) asm volatile("" : "+v"(v))
#endif

// a float64 that is no NaN <-> an unsigned integer of the same order; 0 stands for "nothing yet" and reads as -inf
__device__ __forceinline__ unsigned long long wd_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double wd_val(unsigned long long k) {
    if (k == 0) return CB_NEG;
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

template <int R>
__global__ __launch_bounds__(WD_THREADS) void ctc_words_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c, int T,
                                                               int C, const int* __restrict__ codes, int n_codes,
                                                               const int* __restrict__ words, int K, int k16, int k32, int k64,
                                                               double word_penalty, const int* __restrict__ index,
                                                               int* __restrict__ record, int n_rows, int cap, long st_rec,
                                                               double* __restrict__ lp_out, long st_lp) {
    extern __shared__ double wd_lds_base[];
    double* ls = wd_lds_base;                                        // [T]
    unsigned long long* xk = reinterpret_cast<unsigned long long*>(ls + T);      // [2][64]: X of the even and the odd steps
    double* enter = reinterpret_cast<double*>(xk + 128);             // [64]
    float* mx = reinterpret_cast<float*>(enter + 64);                // [T]
    float* xs = mx + T;                                              // [T][C]
    unsigned* xrec = reinterpret_cast<unsigned*>(xs + T * C);        // [T][C]
    unsigned char* esrc = reinterpret_cast<unsigned char*>(xrec + T * C);        // [T][C]
    unsigned char* gsrc = esrc + T * C;                              // [T]
    const int tid = threadIdx.x, threads = blockDim.x, wave = tid >> 6, lane = tid & 63, waves = threads >> 6, b = blockIdx.x;
    const int row = index[b];
    if (row < 0 || row >= n_rows) return;                            // (the whole work-group: nothing is written)
    int* rec = record + row * st_rec;

    // ---- staging: a wave per step, lane = class, WD_STAGE steps in flight (ctc_lex.h's lx_stage<WD_STAGE> restated: see the top) ----
    const float* x = logits + b * st_b + lane * st_c;
    int flag = 0;
    for (int t0 = wave; t0 < T && !flag; t0 += waves * WD_STAGE) {
        float xv[WD_STAGE];
#pragma unroll
        for (int u = 0; u < WD_STAGE; ++u) {
            const int t = t0 + waves * u;
            xv[u] = lane < C && t < T ? x[t * st_t] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < WD_STAGE; ++u) {
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
    for (int i = tid; i < T * C; i += threads) xrec[i] = WD_NONE;
    for (int i = tid; i < 128; i += threads) xk[i] = 0ull;
    const bool flagged = __syncthreads_or(flag) != 0;
    if (flagged) {
        const double nan = __builtin_nan("");
        if (lp_out)
            for (int i = tid; i < T * C; i += threads) lp_out[b * st_lp + i] = nan;
        if (tid == 0) {
            rec[0] = 0;
            rec[1] = 1;
            rec[2] = __double2loint(nan);
            rec[3] = __double2hiint(nan);
        }
        return;
    }
    if (lp_out)
        for (int i = tid; i < T * C; i += threads) {
            const int t = i / C;
            lp_out[b * st_lp + i] = ((double)xs[i] - (double)mx[t]) - ls[t];
        }

    // ---- the constants of this thread's packed lanes (a wave lies in one segment class: the classes start at multiples of 64) ----
    const int n16 = (k16 * 16 + 63) / 64 * 64, n32 = (k32 * 32 + 63) / 64 * 64;
    int meta[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int p = r * threads + tid;
        const int G = p < n16 ? 16 : p < n16 + n32 ? 32 : 64;        // (the same in every lane of the wave)
        const int q = p < n16 ? p : p < n16 + n32 ? p - n16 : p - n16 - n32;
        const int slot = q / G, s = q % G;
        const int count = G == 16 ? k16 : G == 32 ? k32 : k64, first = G == 16 ? 0 : G == 32 ? k16 : k16 + k32;
        const bool live = slot < count;                              // (first + count <= K: the entry saw to it)
        int L = 0, off = 0, orig = -1;
        if (live) {
            const int* w = words + (long)(first + slot) * LX_WORD;
            L = w[0];
            off = w[1];
            orig = w[2];
        }
        const bool shape_ok = L >= 1 && L <= LX_MAX_L && 2 * L + 1 <= G && off >= 0 && off <= n_codes - L && orig >= 0 && orig < K;
        const bool on = live && shape_ok && s < 2 * L - 1;
        const int j = s >> 1;
        int c = 0, below = 0, c0 = 0;                                // w[j], w[j - 1], w[0]
        bool bad = live && !shape_ok;
        if (on) c0 = codes[off];
        if (on && !(s & 1)) {
            c = codes[off + j];
            if (j >= 1) below = codes[off + j - 1];
            if (c < 1 || c >= C) bad = true;                         // (never an index into the staged logits)
        }
        const unsigned long long segment = (G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull) << ((lane / G) * G);
        const bool word_bad = (__ballot(bad) & segment) != 0;        // a word with anything out of range takes no part
        int m = 0;
        if (on && !word_bad) {
            m = WD_ON | (c0 << 6) | (orig << 16);
            if (!(s & 1)) {
                m |= c;
                if (j >= 1 && c != below) m |= WD_SKIP;
                if (j == 0) m |= WD_FIRST;
                if (j == L - 1) m |= WD_LAST;
            }
        }
        meta[r] = m;
        __builtin_amdgcn_sched_barrier(0);
    }

    // wave 0, lane = class a: enter[tn][a] and G[tn] from G[tn - 1] (g) and X[tn - 1][.]; X of step tn is cleared for its maxima
    double g = 0.0;                                                  // G[-1]
    auto form = [&](int tn) {
        const unsigned long long* xp = xk + ((tn + 1) & 1) * 64;
        double m = g, gm = g;
        int src = 0, gs = 0;
        for (int c = 1; c < C; ++c) {
            const double v = wd_val(xp[c]);
            if (v > gm) {
                gm = v;
                gs = c;
            }
            if (c != lane && v > m) {
                m = v;
                src = c;
            }
        }
        enter[lane] = m;
        if (lane >= 1 && lane < C) esrc[tn * C + lane] = (unsigned char)src;
        if (lane == 0) gsrc[tn] = (unsigned char)gs;
        xk[(tn & 1) * 64 + lane] = 0ull;
        g = (((double)xs[tn * C] - (double)mx[tn]) - ls[tn]) + gm;
    };
    if (wave == 0) form(0);
    __syncthreads();

    // ---- the recursion ----
    constexpr int RG = (R + 3) / 4;                                  // the start steps are bytes, four slots to a register
    double a[R];
    unsigned st4[RG];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = CB_NEG;
#pragma unroll
    for (int q = 0; q < RG; ++q) st4[q] = 0u;
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        unsigned long long* xt = xk + (t & 1) * 64;
        const double base = (double)mx[t], lst = ls[t];
#pragma unroll
        for (int q = 0; q < RG; ++q) {
            const unsigned p0 = st4[q];
            const unsigned p1 = (unsigned)lx_below_i((int)p0, lane, 0), p2 = (unsigned)lx_below_i((int)p1, lane, 0);
            unsigned pn = 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = 4 * q + u;
                if (r < R) {
                    int m = meta[r];
                    WD_OPAQUE(m);                                    // (what derives from the constants is worked out here, not kept)
                    const int c = WD_C(m);
                    const double a1 = lx_below<64>(a[r], lane), a2 = lx_below<64>(a1, lane);
                    double v = a[r];
                    unsigned vs = (p0 >> (8 * u)) & 255u;
                    if (!(m & WD_FIRST) && a1 > v) {
                        v = a1;
                        vs = (p1 >> (8 * u)) & 255u;
                    }
                    if ((m & WD_SKIP) && a2 > v) {
                        v = a2;
                        vs = (p2 >> (8 * u)) & 255u;
                    }
                    if (m & WD_FIRST) {
                        const double e = enter[c] + word_penalty;
                        if (e > v) {
                            v = e;
                            vs = (unsigned)t;
                        }
                    }
                    const double lp = ((double)xs[t * C + c] - base) - lst;
                    const bool on = (m & WD_ON) != 0;
                    a[r] = on ? lp + v : CB_NEG;
                    pn |= (on ? vs : 0u) << (8 * u);
                    if ((m & WD_LAST) && a[r] != CB_NEG) {
                        const unsigned long long key = wd_key(a[r]);
                        if (key > xt[c]) atomicMax(&xt[c], key);     // (the look before is a filter only: X never falls within a step)
                    }
                    __builtin_amdgcn_sched_barrier(0);               // (one slot after the other: 16 slots in flight do not fit 128 VGPRs)
                }
            }
            st4[q] = pn;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int m = meta[r];
            double av = a[r];
            WD_OPAQUE(m);
            WD_OPAQUE(av);                                           // (the score's integer image is formed again, not kept over the barrier)
            const int c = WD_C(m);
            if ((m & WD_LAST) && av != CB_NEG && wd_key(av) == xt[c])
                atomicMin(&xrec[t * C + c], (WD_ORIG(m) << 14) | (((st4[r / 4] >> (8 * (r % 4))) & 255u) << 6) | WD_C0(m));
        }
        // (C) beside (B): both only read X of this step; what (C) writes -- enter, Esrc and Gsrc of step t + 1, X of the other parity --
        // nobody reads before the barrier below
        if (wave == 0 && t + 1 < T) form(t + 1);
        __syncthreads();
    }
    if (tid != 0) return;

    // ---- the end and the back-trace: one thread ----
    const unsigned long long* xe = xk + ((T - 1) & 1) * 64;
    double logp = g;
    int cls = 0;
    for (int c = 1; c < C; ++c) {
        const double v = wd_val(xe[c]);
        if (v > logp) {
            logp = v;
            cls = c;
        }
    }
    int n = 0;
    for (int pass = 0; pass < 2; ++pass) {                           // count, then write left to right
        int c = cls, e = T - 1, p = T - 1, i = 0;                    // a word ends at e in class c; or (c == 0) G[p] is walked back
        for (int guard = 0; guard <= T && logp != CB_NEG; ++guard) {
            if (c == 0) {
                while (p >= 0 && gsrc[p] == 0) --p;
                if (p < 0) break;
                c = gsrc[p];
                e = p - 1;
            }
            if (e < 0 || c < 1 || c >= C) break;                     // (cannot happen: the tables are this work-group's own)
            const unsigned w = xrec[e * C + c];
            if (w == WD_NONE) break;                                 // (nor this)
            const int start = (w >> 6) & 255, c0 = w & 63;
            if (pass == 1 && n - 1 - i >= 0 && n - 1 - i < cap) {
                int* ent = rec + 4 + 2 * (n - 1 - i);
                ent[0] = (int)(w >> 14);
                ent[1] = start | (e << 16);
            }
            ++i;
            c = c0 >= 1 && c0 < C && start >= 0 && start <= e ? esrc[start * C + c0] : 0;
            e = start - 1;
            p = start - 1;
            if (c == 0 && p < 0) break;
        }
        if (pass == 0) n = i < cap ? i : cap;
    }
    rec[0] = n;
    rec[1] = 0;
    rec[2] = __double2loint(logp);
    rec[3] = __double2hiint(logp);
}

template <int R>
static int wd_launch(int threads, size_t lds, const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* codes,
                     int n_codes, const int* words, int K, int k16, int k32, int k64, double word_penalty, const int* index, int* record,
                     int n_rows, int cap, long st_rec, double* lp_out, long st_lp, hipStream_t st) {
    int rc = 0;
    static TattPerDevice attr_once;                                  // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_words_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      WD_LDS_MAX);
    });
    if (rc) return rc;                                               // (beyond 64 KB of LDS the launch depends on it)
    hipLaunchKernelGGL(ctc_words_kernel<R>, dim3(B), dim3(threads), lds, st, logits, st_t, st_b, st_c, T, C, codes, n_codes, words, K, k16,
                       k32, k64, word_penalty, index, record, n_rows, cap, st_rec, lp_out, st_lp);
    return LAUNCH_CHECK();
}

TATT_API int tatt_ctc_words_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* codes, int n_codes,
                                 const int* words, int K, int k16, int k32, int k64, double word_penalty, const int* index, int* record,
                                 int n_rows, int cap, long st_rec, double* lp_out, long st_lp, hipStream_t st) {
    if (!logits || !codes || !words || !index || !record) return 1;
    if (T <= 0 || T > LX_MAX_T || C <= 0 || C > LX_MAX_C || B <= 0 || B > 65535 || K <= 0 || K > LX_MAX_K || n_codes < 0) return 1;
    if (k16 < 0 || k32 < 0 || k64 < 0 || (long)k16 + k32 + k64 != K) return 1;
    const long lanes = wd_pad64(16L * k16) + wd_pad64(32L * k32) + 64L * k64;
    if (lanes > WD_LANES) return 1;
    if (!(word_penalty == word_penalty) || word_penalty == __builtin_inf() || word_penalty == -__builtin_inf()) return 1;
    if (n_rows <= 0 || cap < T || st_rec < 4 + 2 * (long)cap || (lp_out && st_lp < (long)T * C)) return 1;
    const int slots = lanes <= 1 * WD_THREADS ? 1 : lanes <= 2 * WD_THREADS ? 2 : lanes <= 4 * WD_THREADS ? 4 : lanes <= 8 * WD_THREADS ? 8 : 16;
    const int threads = (int)wd_pad64((lanes + slots - 1) / slots);
    const size_t lds = wd_lds(T, C);
#define WD_GO(R_) wd_launch<R_>(threads, lds, logits, st_t, st_b, st_c, T, B, C, codes, n_codes, words, K, k16, k32, k64, word_penalty, \
                                 index, record, n_rows, cap, st_rec, lp_out, st_lp, st)
    switch (slots) {
        case 1: return WD_GO(1);
        case 2: return WD_GO(2);
        case 4: return WD_GO(4);
        case 8: return WD_GO(8);
        default: return WD_GO(16);
    }
#undef WD_GO
}

TATT_API int tatt_words_limits(int* out) {
    if (!out) return 1;
    out[0] = LX_MAX_T;
    out[1] = LX_MAX_C;
    out[2] = WD_LANES;
    out[3] = WD_THREADS;
    out[4] = WD_SLOTS;
    return 0;
}
