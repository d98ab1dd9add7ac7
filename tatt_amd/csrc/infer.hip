// Eval-only kernels of the inference session (tatt_amd/infer.py): the CRNN's bidirectional LSTM layer as one launch, eval BatchNorm
// folded into the preceding convolution, greedy CTC decoding compared with the labels on the device, and the attention recognisers' id
// sequences scored against the same labels (tatt_amd/recog.py).
#include "handoff.h"

// ------------------------------------------------------------------------------------------------
// One bidirectional LSTM layer, forward only, all T steps in ONE launch (H = 256).
//
// Tiling and arithmetic are those of lstm_fwd_step_kernel (lstm.hip): one work-group per (16 batch rows x 16 hidden units x
// direction), h_{t-1} W_hh^T on v_mfma_f32_16x16x4_f32 with the contraction split over the 4 waves and reduced in the same order,
// the cell update in the epilogue -- so `out` is bitwise equal to the per-step launches.  Here the work-group keeps its W_hh slice
// (4 gates x 16 units x this wave's 64 columns: 64 VGPRs per lane), its b_hh and its c state in registers for the whole chain, and
// writes nothing but `out` (no cell sequence, no gate saves: there is no backward).
//
// What crosses work-groups per step is h_{t-1}: a tile's contraction reads the 16 rows x 256 units its (row block, direction) GROUP
// of 16 members produced one step earlier.  The hand-off is the protocol of handoff.h: flags[group * 64 + member] = steps published,
// only wave 0 stores (and drains), and only the members of one group wait on one another -- no grid-wide barrier.
// Error word flags[LCH_ERR], sticky code TATT_STICKY_LSTM.  Residency: the whole grid (cdiv(Bt,16) x 16 x 2 <= 256 work-groups of 256
// threads) must be co-resident -- tatt_lstm_fwd_chain refuses larger grids (the caller takes the step kernels).
// ------------------------------------------------------------------------------------------------
#define LCH_ERR 1023                       // index of the error word in the sync buffer (1024 words)
#define LCH_H 256
struct LstmChainP {
    const float* gi;            // (T, Bt, 8H): [dir][gate][H] along the last axis, b_ih included
    const float* whh[2];        // (4H, H)
    const float* bhh[2];        // (4H)
    float* out;                 // (T, Bt, 2H)
    unsigned* flags;            // 1024 words, zeroed by the entry
    unsigned* sticky;           // the device's sticky error word (common.h), may be null
    int T, Bt;
};
__global__ __launch_bounds__(256) void lstm_fwd_chain_kernel(LstmChainP p) {
    constexpr int H = LCH_H;
    __shared__ float red[4][4][16][17];
    __shared__ __attribute__((aligned(16))) float stage[16][16];
    __shared__ int s_dead;
    const int d = blockIdx.z, mem = blockIdx.y;
    const int m0 = blockIdx.x * 16, j0 = mem * 16;
    const int grp = d * gridDim.x + blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int T = p.T, Bt = p.Bt;
    const int i = lane & 15, q = lane >> 4;
    const int kb = wave * (H / 4);
    const int arow = min(m0 + i, Bt - 1);
    f32x4 b[4][4];                                                   // this wave's W_hh slice, resident for the chain
#pragma unroll
    for (int ss = 0; ss < 4; ++ss)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            b[g][ss] = *reinterpret_cast<const f32x4*>(p.whh[d] + ((long)g * H + j0 + i) * H + kb + 16 * ss + 4 * q);
    const int m = t >> 4, j = t & 15;
    const bool live = m0 + m < Bt;
    const long row = m0 + m;
    float bh[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bh[g] = p.bhh[d][g * H + j0 + j];
    float c = 0.f;
    if (t == 0) s_dead = 0;
    __syncthreads();
    unsigned* flags = p.flags + grp * 64;
    const long plane = (long)Bt * 2 * H;                            // floats of one time slice of `out`
    for (int s = 0; s < T; ++s) {
        const int tt = d ? T - 1 - s : s, tp = d ? tt + 1 : tt - 1;
        f32x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (s > 0) {
            HANDOFF_WAIT(wave == 0, lane, 1, flags, 16, (unsigned)s, s_dead, p.flags + LCH_ERR, p.sticky, TATT_STICKY_LSTM)
            f32x4 a[4];
            const int off = (arow * 2 * H + d * H + kb + 4 * q) * 4;
#pragma unroll
            for (int ss = 0; ss < 4; ++ss)
                a[ss] = __builtin_bit_cast(f32x4, ld16_sc1(p.out + (long)tp * plane, (int)(plane * 4), off + 64 * ss));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ss = 0; ss < 4; ++ss)
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ss][u], b[g][ss][u], acc[g], 0, 0, 0);
        }
        {
            const int col = lane & 15, rb = (lane >> 4) * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave][g][rb + r][col] = acc[g][r];
        }
        __syncthreads();
        if (live) {
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                pre[g] = (red[0][g][m][j] + red[1][g][m][j]) + (red[2][g][m][j] + red[3][g][m][j]) + bh[g] +
                         p.gi[((long)tt * Bt + row) * 8 * H + (d * 4 + g) * H + j0 + j];
            const float ig = sigmoid_f(pre[0]), fg = sigmoid_f(pre[1]), gg = tanhf(pre[2]), og = sigmoid_f(pre[3]);
            c = __builtin_fmaf(ig, gg, fg * c);          // the contraction hipcc picks for the step kernel's fg * cp + ig * gg
            stage[m][j] = og * tanhf(c);
        }
        __syncthreads();
        if (t < 64) {                                                // 16 rows x 4 sixteen-byte pieces
            const int r = t >> 2, j4 = (t & 3) * 4;
            if (m0 + r < Bt) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&stage[r][j4]);
                st16_sc1(p.out + (long)tt * plane, (int)(plane * 4), ((m0 + r) * 2 * H + d * H + j0 + j4) * 4, &v);
            }
            handoff_drain();                                         // the storing wave only
        }
        handoff_post(flags + mem, (unsigned)(s + 1));
    }
}

// asked once per device (the first call is eager: the session's warm-up runs before it captures)
static int lstm_chain_capacity_now() {
    static std::mutex mu;
    static int cap[64];
    static bool known[64] = {};
    int dev = 0, cus = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    std::lock_guard<std::mutex> lk(mu);
    if (!known[dev]) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(lstm_fwd_chain_kernel), 256, 0) != hipSuccess) return -1;
        cap[dev] = n * cus;
        known[dev] = true;
    }
    return cap[dev];
}

// gi (T, Bt, 8H) incl. b_ih, whh* (4H, H), bhh* (4H), out (T, Bt, 2H), sync: 1024 words of workspace (zeroed here; word LCH_ERR is
// the launch's error word).  Returns 1 for geometries it does not take (H != 256, a grid of more than 256 work-groups or more than
// the device holds at once): the caller runs the per-step kernels instead.
TATT_API int tatt_lstm_fwd_chain(const float* gi, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
                                 float* out, unsigned* sync, int T, int Bt, int H, hipStream_t st) {
    if (H != LCH_H || Bt <= 0 || T <= 0) return 1;
    const int nrb = cdiv(Bt, 16), grid = nrb * (H / 16) * 2;
    if (grid > 256 || (2 * nrb - 1) * 64 + 16 > LCH_ERR) return 1;     // flags[group * 64 + member] stay below the error word
    if (grid > lstm_chain_capacity_now()) return 1;
    if (hipMemsetAsync(sync, 0, 1024 * sizeof(unsigned), st) != hipSuccess) return 3;
    LstmChainP p = {gi, {whh_f, whh_r}, {bhh_f, bhh_r}, out, sync, tatt_sticky_ptr(), T, Bt};
    hipLaunchKernelGGL(lstm_fwd_chain_kernel, dim3(nrb, H / 16, 2), dim3(256), 0, st, p);
    return LAUNCH_CHECK();
}

// out[0]: work-groups of lstm_fwd_chain_kernel the CURRENT device holds at once (occupancy per CU x CUs the process sees).
TATT_API int tatt_lstm_chain_capacity(int* out) {
    const int n = lstm_chain_capacity_now();
    if (n < 0) return 1;
    out[0] = n;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Eval BatchNorm folded into the preceding convolution: per output channel o, s = gamma_o / sqrt(var_o + eps),
//   w'[o, :] = w[o, :] * s,   b'_o = (b_o - mean_o) * s + beta_o     (a missing conv bias counts as 0)
// w, w_out (Cout, K) contiguous.  One work-group per output channel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_fold_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                      float* __restrict__ w_out, float* __restrict__ b_out, int K) {
    const int o = blockIdx.x;
    const float s = gamma[o] / sqrtf(var[o] + eps);
    const float* src = w + (long)o * K;
    float* dst = w_out + (long)o * K;
    for (int k = threadIdx.x; k < K; k += blockDim.x) dst[k] = src[k] * s;
    if (threadIdx.x == 0) b_out[o] = ((bias ? bias[o] : 0.f) - mean[o]) * s + beta[o];
}
TATT_API int tatt_bn_fold(const float* w, const float* bias, const float* gamma, const float* beta, const float* mean,
                          const float* var, float eps, float* w_out, float* b_out, int Cout, int K, hipStream_t st) {
    if (Cout <= 0 || K <= 0) return 1;
    hipLaunchKernelGGL(bn_fold_kernel, dim3(Cout), dim3(256), 0, st, w, bias, gamma, beta, mean, var, eps, w_out, b_out, K);
    return LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------
// Greedy CTC decoding compared with encoded labels (the reference's get_string_crnn + str_filt + string equality, as
// io.ctc_greedy_decode does it): per image the arg-max class of every step (ties to the lowest index, as torch.argmax), repeats
// merged and blank 0 dropped, then the classes the keep mask excludes dropped; the result is compared with label[b][0 .. len_b)
// (class indices, len_b < 0: a label that cannot match).  One wave per image, lane = class (C <= 64).
// logits (T, B, C) by element strides; keep (C) int; label (B, T) int; label_len (B) int.
// Outputs (each may be NULL): correct (B) 0/1; counter: += number of correct images (one vector atomic per image);
// dec (B, T) the decoded classes after the keep mask, padded with -1; dec_len (B).
// ------------------------------------------------------------------------------------------------
// The decoding both kernels share: arg-max of every step over the wave, then lane 0 merges repeats, drops the blank and the classes the
// keep mask excludes, compacting in place (seq[n] is written only after seq[t >= n] was read).  seq: >= T ints of LDS, n_out: one.
// Returns the decoded length n; seq[0 .. n) holds the classes, visible to every lane.
__device__ __forceinline__ int ctc_greedy_decode(const float* __restrict__ logits, long st_t, long st_b, long st_c, int T, int C,
                                                 const int* __restrict__ keep, int* seq, int* n_out) {
    const int bidx = blockIdx.x, lane = threadIdx.x;
    for (int t = 0; t < T; ++t) {
        float v = lane < C ? logits[t * st_t + bidx * st_b + lane * st_c] : -INFINITY;
        int k = lane < C ? lane : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(v, o, 64);
            const int k2 = __shfl_xor(k, o, 64);
            // a NaN wins over any number (torch.argmax), ties and NaN against NaN go to the lower class
            const bool take = k2 != 0x7fffffff && ((v2 != v2) ? (v == v || k2 < k) : (v == v && (v2 > v || (v2 == v && k2 < k))));
            if (take) { v = v2; k = k2; }
        }
        if (lane == 0) seq[t] = k;
    }
    __syncthreads();
    if (lane == 0) {
        int n = 0, last = 0;
        for (int t = 0; t < T; ++t) {
            const int c = seq[t];
            if (c != last) {
                if (c != 0 && keep[c]) seq[n++] = c;
                last = c;
            }
        }
        *n_out = n;
    }
    __syncthreads();
    return *n_out;
}

__global__ __launch_bounds__(64) void ctc_greedy_match_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c, int T,
                                                              int C, const int* __restrict__ keep, const int* __restrict__ label,
                                                              const int* __restrict__ label_len, int* correct, int* counter,
                                                              int* dec, int* dec_len) {
    __shared__ int seq[256];
    __shared__ int n_sh;
    const int bidx = blockIdx.x;
    const int n = ctc_greedy_decode(logits, st_t, st_b, st_c, T, C, keep, seq, &n_sh);
    if (threadIdx.x != 0) return;
    const int L = label_len[bidx];
    bool ok = n == L;
    for (int r = 0; r < n; ++r) {
        if (dec) dec[(long)bidx * T + r] = seq[r];
        if (ok && label[(long)bidx * T + r] != seq[r]) ok = false;
    }
    if (dec)
        for (int r = n; r < T; ++r) dec[(long)bidx * T + r] = -1;
    if (dec_len) dec_len[bidx] = n;
    if (correct) correct[bidx] = ok ? 1 : 0;
    if (counter && ok) atomicAdd(counter, 1);
}
TATT_API int tatt_ctc_greedy_match(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* keep,
                                   const int* label, const int* label_len, int* correct, int* counter, int* dec, int* dec_len,
                                   hipStream_t st) {
    if (T <= 0 || T > 256 || B <= 0 || C <= 0 || C > 64) return 1;
    hipLaunchKernelGGL(ctc_greedy_match_kernel, dim3(B), dim3(64), 0, st, logits, st_t, st_b, st_c, T, C, keep, label, label_len,
                       correct, counter, dec, dec_len);
    return LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------
// The match kernel plus the edit distance (the eval loop's editdistance.eval(pred, label), reference
// interfaces/super_resolution.py:1531-1556): the same decoding, then the Levenshtein distance with unit costs between the decoded
// classes p_1..p_n (n <= T) and the label codes l_1..l_m (m <= 64).  One wave per image; lane j-1 holds column j of the DP row:
//   tmp[j]  = min(D[i-1][j] + 1, D[i-1][j-1] + (p_i != l_j))              (deletion, substitution / match)
//   D[i][j] = min(i + j, j + min_{1 <= k <= j}(tmp[k] - k))               (the insertions, as a prefix minimum: 6 shuffle steps)
// Columns beyond m hold the padding -1, which equals no class, and never feed a lower column.
// label (B, 64) int: classes 1 .. C-1, any code >= 64 for a character outside the alphabet (it equals no decoded class), padding -1;
// label_len (B): m, or < 0 (or > 64) for a label the cap excludes: dist -1, not correct, counted in skipped.
// Outputs (each may be NULL): correct / counter / dec / dec_len as in the match kernel (correct <=> dist == 0), dec rows st_dec ints
// apart and the elements of correct, dec_len and dist st_img ints apart (so that they can be columns of one record tensor);
// dist (B); hist (65) int: hist[max(n, m)] += dist (index 0 is never written); scored, skipped: += 1.
// ------------------------------------------------------------------------------------------------
// The recurrence above, shared by the score kernels (ctc_greedy_score_kernel, ids_score_kernel): seq[0 .. n) the decoded codes in LDS
// (any n), lj the label code of this lane's column (lane j-1 holds column j), m <= 64 the label's length.  Every lane of the wave calls
// it; returns the distance D[n][m] in every lane.
__device__ __forceinline__ int lev_wave(const int* seq, int n, int lj, int m) {
    const int lane = threadIdx.x, j = lane + 1;
    int row = j;                                                 // D[0][j]
    for (int i = 1; i <= n; ++i) {
        const int p = seq[i - 1];
        int diag = __shfl_up(row, 1, 64);
        if (lane == 0) diag = i - 1;                             // D[i-1][0]
        int s = min(row + 1, diag + (p != lj ? 1 : 0)) - j;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int s2 = __shfl_up(s, o, 64);
            if (lane >= o) s = min(s, s2);
        }
        row = min(i + j, j + s);
    }
    const int d = __shfl(row, m > 0 ? m - 1 : 0, 64);
    return m == 0 ? n : d;
}

__global__ __launch_bounds__(64) void ctc_greedy_score_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c, int T,
                                                              int C, const int* __restrict__ keep, const int* __restrict__ label,
                                                              const int* __restrict__ label_len, int* correct, int* counter,
                                                              int* dec, int* dec_len, int* dist, long st_dec, long st_img,
                                                              int* hist, int* scored, int* skipped) {
    __shared__ int seq[256];
    __shared__ int n_sh;
    const int bidx = blockIdx.x, lane = threadIdx.x;
    const int n = ctc_greedy_decode(logits, st_t, st_b, st_c, T, C, keep, seq, &n_sh);
    if (dec)
        for (int r = lane; r < T; r += 64) dec[bidx * st_dec + r] = r < n ? seq[r] : -1;
    const int m = label_len[bidx];
    int d = -1;
    if (m >= 0 && m <= 64) d = lev_wave(seq, n, label[(long)bidx * 64 + lane], m);      // (uniform over the wave)
    if (lane != 0) return;
    if (dec_len) dec_len[bidx * st_img] = n;
    if (dist) dist[bidx * st_img] = d;
    if (correct) correct[bidx * st_img] = d == 0 ? 1 : 0;
    if (counter && d == 0) atomicAdd(counter, 1);
    if (d < 0) {
        if (skipped) atomicAdd(skipped, 1);
        return;
    }
    if (scored) atomicAdd(scored, 1);
    const int M = max(n, m);
    if (hist && d > 0 && M <= 64) atomicAdd(hist + M, d);
}
TATT_API int tatt_ctc_greedy_score(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* keep,
                                   const int* label, const int* label_len, int* correct, int* counter, int* dec, int* dec_len,
                                   int* dist, long st_dec, long st_img, int* hist, int* scored, int* skipped, hipStream_t st) {
    if (T <= 0 || T > 256 || B <= 0 || C <= 0 || C > 64) return 1;
    if (hist && T > 64) return 1;                                // max(n, m) must index the 65 bins
    hipLaunchKernelGGL(ctc_greedy_score_kernel, dim3(B), dim3(64), 0, st, logits, st_t, st_b, st_c, T, C, keep, label, label_len,
                       correct, counter, dec, dec_len, dist, st_dec, st_img, hist, scored, skipped);
    return LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------
// Id sequences scored on the device (the attention recognisers' ids -> string -> str_filt -> editdistance.eval of the eval loop,
// io._evaluate_ids): ids holds G * B rows of L class ids, st_row ints apart, row r = g * B + b = image b of image kind g; the labels
// (B, 64) / (B) are those of the score kernel above, shared by the G kinds.  A row is walked through the character map cmap (C) int:
// an id outside [0, C) or with cmap[id] == 0 is dropped, cmap[id] == -1 stops the row, any other value is a label code (1 .. 63) and is
// appended -> n <= L codes, then lev_wave against the label.  One wave per row: lanes map the row into LDS, lane 0 compacts it in place
// (seq[n] is written only after seq[t >= n] was read).  Nothing crosses work-groups but the integer atomics.
// Outputs (each may be NULL): rec row r, st_rec >= L + 3 ints apart: codes padded with -1 (L) | n | correct | dist (-1 for a label the
// cap excludes); counter (G): [g] += correct; stats (G, bins + 2): [g][max(n, m)] += dist | [g][bins] += 1 scored | [g][bins + 1] += 1
// skipped, bins > max(L, 64) so that max(n, m) indexes a bin.
// ------------------------------------------------------------------------------------------------
#define IDS_MAXL 128
__global__ __launch_bounds__(64) void ids_score_kernel(const int* __restrict__ ids, long st_row, int B, int L,
                                                       const int* __restrict__ cmap, int C, const int* __restrict__ label,
                                                       const int* __restrict__ label_len, int* rec, long st_rec, int* counter,
                                                       int* stats, int bins) {
    __shared__ int seq[IDS_MAXL];
    __shared__ int n_sh;
    const int r = blockIdx.x, lane = threadIdx.x;
    const int g = r / B, b = r - g * B;
    for (int t = lane; t < L; t += 64) {
        const int id = ids[(long)r * st_row + t];
        seq[t] = (id < 0 || id >= C) ? 0 : cmap[id];
    }
    __syncthreads();
    if (lane == 0) {
        int n = 0;
        for (int t = 0; t < L; ++t) {
            const int c = seq[t];
            if (c == -1) break;
            if (c != 0) seq[n++] = c;
        }
        n_sh = n;
    }
    __syncthreads();
    const int n = n_sh;
    if (rec)
        for (int t = lane; t < L; t += 64) rec[(long)r * st_rec + t] = t < n ? seq[t] : -1;
    const int m = label_len[b];
    int d = -1;
    if (m >= 0 && m <= 64) d = lev_wave(seq, n, label[(long)b * 64 + lane], m);          // (uniform over the wave)
    if (lane != 0) return;
    if (rec) {
        int* tail = rec + (long)r * st_rec + L;
        tail[0] = n;
        tail[1] = d == 0 ? 1 : 0;
        tail[2] = d;
    }
    if (counter && d == 0) atomicAdd(counter + g, 1);
    if (!stats) return;
    int* row = stats + (long)g * (bins + 2);
    if (d < 0) {
        atomicAdd(row + bins + 1, 1);
        return;
    }
    atomicAdd(row + bins, 1);
    const int M = max(n, m);
    if (d > 0 && M < bins) atomicAdd(row + M, d);
}
TATT_API int tatt_ids_score(const int* ids, long st_row, int G, int B, int L, const int* cmap, int C, const int* label,
                            const int* label_len, int* rec, long st_rec, int* counter, int* stats, int bins, hipStream_t st) {
    if (L < 1 || L > IDS_MAXL || C < 1 || C > 256 || G < 1 || B < 1 || (long)G * B > 0x7fffffffL) return 1;
    if (stats && bins < (L > 64 ? L : 64) + 1) return 1;          // max(n, m) must index a bin
    if (!ids || !cmap || !label || !label_len || st_row < L || (rec && st_rec < L + 3)) return 1;
    hipLaunchKernelGGL(ids_score_kernel, dim3(G * B), dim3(64), 0, st, ids, st_row, B, L, cmap, C, label, label_len, rec, st_rec,
                       counter, stats, bins);
    return LAUNCH_CHECK();
}
