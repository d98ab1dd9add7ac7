// CTC forced alignment of the line reader (tatt_amd/read.py `ctc_align_host` is the specification, tests/test_align*.py hold the kernel
// to it): the most probable alignment of a line that spells a GIVEN string, with the steps every character spans -- the Viterbi
// recursion over the 2 L + 1 states of the string with a back-trace.
//   ctc_align_kernel   ONE work-group of 256 threads per line, it meets no other work-group.  The string of chunk line b is read ON THE
//                      DEVICE from row index[b] of `src` (the decode launch's own record, or a packed table of caller strings): its
//                      length at word len_at, its classes from word cls_at, and -- gate_at >= 0 -- a word that must be >= 1 for a
//                      string to exist at all (a beam row's "entries written").
//                      Staging: ctc_lex.h's `lx_stage` (the line's T x C fp32 logits in LDS with mx (fp32) and ls (float64) per step);
//                      lp = (double(x) - double(mx)) - ls as `lx_word` forms it, written to lp_out where the caller asks for it.
//                      Thread s = state s (even: a blank, odd: the character s / 2).  v lies in an LDS double buffer, ONE barrier per
//                      step t >= 1: the candidate is v[s], then v[s - 1] (s >= 1), then v[s - 2] (s odd, s >= 3, another class than
//                      s - 2) -- each replaces only where STRICTLY greater, in this order; the new v[s] is that value + lp[t][c(s)]
//                      and the move taken (0, 1, 2) is a byte of the back-pointer table in LDS.
//                      The end is state 2 L, or 2 L - 1 where strictly greater.  Thread 0 walks the T - 1 pointers back and leaves every
//                      character's first and last step in LDS; behind one barrier thread k sums lp[t][class k] over the run of
//                      character k, left to right, and writes its pair and its sum.
//                      Everything after the log-soft-max is float64 addition, comparison and copies: the record equals the
//                      specification run on lp_out BIT FOR BIT.
// Dynamic LDS for T steps, C classes and strings of at most cap_len characters (SP = the 2 cap_len + 1 states rounded up to 4):
//   ls 8 T + v 2 x 256 x 8 + mx 4 T + logits 4 T C + first / last 2 x 128 x 4 + pointers T SP bytes;
//   at the limits (T = 256, C = 64, 127 characters): 2,048 + 4,096 + 1,024 + 65,536 + 1,024 + 65,536 = 139,264 of the CU's 163,840.
// Every loop is bounded by T, C or the 255 states.  Nothing is indexed by string DATA without a range check: a length outside
// 0 .. min(cap_len, 127) or a class outside 1 .. C - 1 refuses the string (flag 2).  No global scratch, no traffic between work-groups.
// `src` and `record` may be the same buffer (the string is read before anything is written, by the work-group that writes the row).
#include "ctc_lex.h"

#define AL_THREADS 256
#define AL_MAX_L 127                           // 2 L + 1 = 255 states, one thread each
#define AL_MAX_S (2 * AL_MAX_L + 1)

static_assert(AL_MAX_S <= AL_THREADS, "a string's states fit the work-group");

static inline int al_pad4(int v) { return (v + 3) / 4 * 4; }
// the staged logits, then v [2][256] (float64), first / last [2][128] (int) and the back-pointers [T][SP] (bytes)
static inline size_t al_lds(int T, int C, int sp) { return LX_STAGE_LDS(T, C) + 2 * AL_THREADS * 8 + 2 * 128 * 4 + (size_t)T * sp; }
#define AL_LDS_MAX (LX_LDS_MAX + 2 * AL_THREADS * 8 + 2 * 128 * 4 + LX_MAX_T * 256)
static_assert(AL_LDS_MAX <= 160 * 1024, "the tables of a line fit the LDS of a CU");

// 32-bit words of the alignment part of a record row: characters | flag | logp (2) | cap_len pairs (first, last) | cap_len float64
static inline long al_record_words(int cap_len) { return 4 + 4 * (long)cap_len; }

__global__ __launch_bounds__(AL_THREADS) void ctc_align_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c, int T,
                                                               int C, const int* __restrict__ index, const int* src, long src_stride,
                                                               int len_at, int cls_at, int gate_at, int* record, int n_rows,
                                                               long rec_stride, int rec_at, int cap_len, int sp,
                                                               double* __restrict__ lp_out) {
    extern __shared__ double al_lds_base[];
    double* ls = al_lds_base;                                        // [T]
    double* vb = ls + T;                                             // [2][256]
    float* mx = reinterpret_cast<float*>(vb + 2 * AL_THREADS);       // [T]
    float* xs = mx + T;                                              // [T][C]
    int* first = reinterpret_cast<int*>(xs + T * C);                 // [128]
    int* last = first + 128;                                         // [128]
    unsigned char* bp = reinterpret_cast<unsigned char*>(last + 128);            // [T][sp]
    const int tid = threadIdx.x, b = blockIdx.x;
    const int row = index[b];
    if (row < 0 || row >= n_rows) return;                            // (the whole work-group: nothing is written)
    int* rec = record + row * rec_stride + rec_at;
    const int* str = src + row * src_stride;

    // ---- the string, read before anything of the row is written ----
    const int gate = gate_at >= 0 ? str[gate_at] : 1;
    int L = str[len_at];
    const bool shape_ok = L >= 0 && L <= cap_len && L <= AL_MAX_L;
    if (!shape_ok) L = 0;
    const int S = 2 * L + 1, s = tid;
    int c = 0, below2 = 0;                                           // c(s), c(s - 2)
    int bad = !shape_ok;
    if (gate >= 1 && s < S && (s & 1)) {
        c = str[cls_at + (s >> 1)];
        if (s >= 3) below2 = str[cls_at + (s >> 1) - 1];
        if (c < 1 || c >= C) {                                       // (never an index into the staged logits)
            bad = 1;
            c = 0;
        }
    }
    const bool skip = (s & 1) && s >= 3 && c != below2;

    // ---- staging ----
    const int flag = lx_stage<LX_STAGE>(logits + b * st_b, st_t, st_c, T, C, AL_THREADS / 64, ls, mx, xs);
    const bool flagged = __syncthreads_or(flag) != 0;
    const bool refused = __syncthreads_or(bad) != 0;
    const double nan = __builtin_nan("");
    if (lp_out) {
        double* lp = lp_out + (long)b * T * C;
        for (int i = tid; i < T * C; i += AL_THREADS) lp[i] = flagged ? nan : ((double)xs[i] - (double)mx[i / C]) - ls[i / C];
    }
    if (flagged || gate < 1 || refused) {                            // (the same in every thread)
        if (tid == 0) {
            rec[0] = 0;
            rec[1] = flagged || gate < 1 ? 1 : 2;
            rec[2] = __double2loint(nan);
            rec[3] = __double2hiint(nan);
        }
        return;
    }

    // ---- the recursion: thread = state, one barrier per step ----
    const bool on = s < S;
    if (on) vb[s] = s <= 1 ? ((double)xs[c] - (double)mx[0]) - ls[0] : CB_NEG;
    if (tid < 128) {
        first[tid] = 0;
        last[tid] = -1;
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 1; t < T; ++t) {
        const double* cur = vb + ((t + 1) & 1) * AL_THREADS;
        double* nxt = vb + (t & 1) * AL_THREADS;
        if (on) {
            const double lp = ((double)xs[t * C + c] - (double)mx[t]) - ls[t];
            double v = cur[s];
            int p = 0;
            if (s >= 1) {
                const double a1 = cur[s - 1];
                if (a1 > v) {
                    v = a1;
                    p = 1;
                }
            }
            if (skip) {
                const double a2 = cur[s - 2];
                if (a2 > v) {
                    v = a2;
                    p = 2;
                }
            }
            nxt[s] = v + lp;
            bp[t * sp + s] = (unsigned char)p;
        }
        __syncthreads();
    }
    const double* fin = vb + ((T - 1) & 1) * AL_THREADS;
    double logp = fin[S - 1];
    int state = S - 1;
    if (L >= 1 && fin[S - 2] > logp) {
        logp = fin[S - 2];
        state = S - 2;
    }
    const bool feasible = logp != CB_NEG;                            // (the same in every thread: all read the same two values)

    // ---- the back-trace: one thread walks T - 1 pointers, then thread k sums the run of character k ----
    if (tid == 0 && feasible) {
        for (int t = T - 1; t >= 0; --t) {
            if (state & 1) {
                const int k = state >> 1;
                if (last[k] < 0) last[k] = t;
                first[k] = t;
            }
            if (t >= 1) {
                const int p = bp[t * sp + state];
                state = state >= p ? state - p : 0;                  // (cannot fall below 0: the table is this work-group's own)
            }
        }
    }
    __syncthreads();
    if (feasible && tid < L) {
        const int cls = str[cls_at + tid], f = first[tid], l = last[tid];
        double sum = 0.0;
        for (int t = f; t <= l && t < T; ++t) {
            const double lp = ((double)xs[t * C + cls] - (double)mx[t]) - ls[t];
            sum = t == f ? lp : sum + lp;
        }
        rec[4 + 2 * tid] = f;
        rec[5 + 2 * tid] = l;
        rec[4 + 2 * cap_len + 2 * tid] = __double2loint(sum);
        rec[5 + 2 * cap_len + 2 * tid] = __double2hiint(sum);
    }
    if (tid == 0) {
        rec[0] = feasible ? L : 0;
        rec[1] = 0;
        rec[2] = __double2loint(logp);
        rec[3] = __double2hiint(logp);
    }
}

TATT_API int tatt_ctc_align(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* index, const int* src,
                            int src_rows, long src_stride, int len_at, int cls_at, int gate_at, int* record, int n_rows, long rec_stride,
                            int rec_at, int cap_len, double* lp_out, hipStream_t st) {
    if (!logits || !index || !src || !record) return 1;
    if (T <= 0 || T > LX_MAX_T || C < 2 || C > LX_MAX_C || B <= 0 || B > 65535) return 1;
    if (cap_len < 0 || cap_len > AL_MAX_L || n_rows <= 0 || src_rows < n_rows) return 1;
    if (src_stride <= 0 || len_at < 0 || len_at >= src_stride || cls_at < 0 || cls_at + (long)cap_len > src_stride) return 1;
    if (gate_at < -1 || gate_at >= src_stride) return 1;
    if (rec_at < 0 || (rec_at & 1) || (rec_stride & 1) || rec_at + al_record_words(cap_len) > rec_stride) return 1;
    if (((size_t)record & 7) != 0) return 1;                         // (the float64 fields are stored as two words, but stay aligned)
    const int sp = al_pad4(2 * cap_len + 1);
    const size_t lds = al_lds(T, C, sp);
    int rc = 0;
    static TattPerDevice attr_once;                                  // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      AL_LDS_MAX);
    });
    if (rc) return rc;                                               // (beyond 64 KB of LDS the launch depends on it)
    hipLaunchKernelGGL(ctc_align_kernel, dim3(B), dim3(AL_THREADS), lds, st, logits, st_t, st_b, st_c, T, C, index, src, src_stride,
                       len_at, cls_at, gate_at, record, n_rows, rec_stride, rec_at, cap_len, sp, lp_out);
    return LAUNCH_CHECK();
}

TATT_API int tatt_align_limits(int* out) {
    if (!out) return 1;
    out[0] = LX_MAX_T;
    out[1] = LX_MAX_C;
    out[2] = AL_MAX_L;
    return 0;
}
