// The attention decoder the ASTER and MORAN recognisers share (reference model/recognizer/attention_recognition_head.py and
// model/moran/asrn_res.py:39-65,127-155): additive attention over the encoder positions, context, one GRU cell, a linear head.
//   gru_cell       : the gate arithmetic of one GRU step from gi / gh (the step-by-step route of both decoders)
//   attn_decode    : all L steps of ASTER's head, one work-group per image          (tatt_attn_decode: forced, greedy, beam)
//   moran_decode   : all L steps of one direction of MORAN's `Attention`, likewise  (tatt_moran_decode: forced, greedy)
//   beam_backtrack : the beam's backtracking alone, for the step-by-step route
// Both one-launch entries run ONE kernel template, attn_decode_kernel<D, R>; what differs between the heads travels in AttnDecArgs.
#include "common.h"

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.f / (1.f + expf(-x)); }

// hout[r,j] = (1 - z) n + z h with r = sig(gi_r + gh_r), z = sig(gi_z + gh_z), n = tanh(gi_n + r gh_n); gi, gh (R, 3H) in gate order r|z|n
__global__ void gru_cell_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ h,
                                float* __restrict__ hout, int R, int H) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)R * H) return;
    const int r = i / H, j = i % H;
    const float* a = gi + (long)r * 3 * H;
    const float* b = gh + (long)r * 3 * H;
    const float rg = sigmoid_acc(a[j] + b[j]), zg = sigmoid_acc(a[H + j] + b[H + j]);
    const float n = tanhf(a[2 * H + j] + rg * b[2 * H + j]);
    hout[i] = (1.f - zg) * n + zg * h[i];
}
TATT_API int tatt_gru_cell(const float* gi, const float* gh, const float* h, float* hout, int R, int H, hipStream_t st) {
    if (R < 1 || H < 1) return 1;
    hipLaunchKernelGGL(gru_cell_kernel, dim3(cdiv((long)R * H, 256)), dim3(256), 0, st, gi, gh, h, hout, R, H);
    return LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The attention decoder, all L steps in one launch.
//
// One work-group of D threads per image (D = state = attention = feature size) carries that image's R rows (1: forced / greedy,
// 5: its beams) through every step; nothing is exchanged between work-groups, so the launch has no in-flight synchronisation, no
// residency requirement and no wait that could expire.  Per step and row:
//   sProj = Ws s + bs;  e_t = wv . tanh(sProj + xproj_t) [+ wb];  alpha = softmax_t(e);  ctx = sum_t alpha_t x_t
//   gi = E2[y] + Wic ctx   (E2 = embedding W_ih[:, embedding columns]^T + b_ih: step-invariant, built once per parameter set)
//   gh = W_hh s + b_hh;  s' = GRU gates;  logits = fc(s')
// The weights are read TRANSPOSED ([k][out], prepared once per parameter set): a thread owns one output, walks k, reads its weight
// coalesced with its neighbours' and the rows' activations as LDS broadcasts, so one weight read serves all the image's rows and no
// product is reduced across lanes.  Every dot product runs as 4 interleaved chains (k mod 4) summed pairwise at the end.
// Where an image's x and xproj rows fit into 64 KB of LDS (D = 256) they are staged there for all steps; otherwise they are read
// from global memory.
// What the heads do with a step's logits is data: forced (targets given) or arg-max, the embedding row of step 0 (y0), the offset from
// an arg-max to its embedding row (yadd), which target a forced step reads (tshift), where a greedy row stops (eos; negative: nowhere),
// and which of logits / ids / scores are asked for.  R > 1 is the beam search, backtracking included.
#define AD_MAXT 32
#define AD_MAXL 100       // steps the beam's history holds (each entry point has its own limit on L)

struct AttnDecArgs {
    const float *x, *xproj, *WsT, *bs, *wv, *wb, *E2, *WicT, *WhhT, *bhh, *fcT, *fcb;      // wb: null = no bias on the score
    // R = 1 only (the beam is ASTER's `beam_search`: never forced, no logits, row y0 first, an arg-max is its own row, scores of 1):
    const int* targets;      // (B, L), null = not forced.  The embedding row of forced step i is targets[i + tshift], y0 where that is < 0
    float* logits;           // (B, L, C) or null
    // every R:
    int* ids;                // (B, L): the arg-max (R = 1, not forced) or the best beam
    float* scores;           // (B, L): the arg-max's softmax value (R = 1, may be null); 1 (beam)
    int B, T, C, L, eos, y0, yadd, tshift;      // (yadd, tshift: R = 1 only)
};

__device__ __forceinline__ float sum4(const float* c) { return (c[0] + c[1]) + (c[2] + c[3]); }
__device__ __forceinline__ float comp(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
// candidate order of the arg-max and the beam: score descending, then (flat) index ascending
__device__ __forceinline__ bool cand_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }
__device__ __forceinline__ void wave_best(float& bv, int& bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (cand_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}
__device__ __forceinline__ int target_row(const AttnDecArgs& a, int b, int i) {      // (E2 has C + 1 rows)
    return i < 0 ? a.y0 : min(max(a.targets[(long)b * a.L + i], 0), a.C);
}

constexpr bool attn_staged(int D) { return 2 * AD_MAXT * D * sizeof(float) <= 64 * 1024; }

template <int D, int R>
__global__ __launch_bounds__(D) void attn_decode_kernel(AttnDecArgs a) {
    constexpr int MAXC = D / 4, NW = D / 64, NG = D / 256, PC = MAXC / 64;      // classes; waves; float4 groups, classes per lane
    constexpr bool STAGED = attn_staged(D);
    // unroll factors of the two long k loops, per instantiation: the parent kernels' for one row (4 / 2 at D = 256, 2 / 1 at D = 512); five
    // rows run fastest at 1 / 1 (measured: profiles/attndec_shared_decoder_ab.txt; the GRU loop at 2 spills there)
    constexpr int U_PROJ = D == 256 ? 4 : R == 1 ? 2 : 1, U_GRU = D == 256 ? 2 : 1;
    constexpr int HL = R > 1 ? AD_MAXL : 1;
    extern __shared__ __attribute__((aligned(16))) float staged_lds[];          // STAGED: x [T][D] | xproj [T][D]
    __shared__ __attribute__((aligned(16))) float sS[2][R][D];           // the rows' states: current / next
    __shared__ __attribute__((aligned(16))) float sP[R][D];              // sProj; later the 4 partial sums of fc ([4][R][MAXC])
    __shared__ __attribute__((aligned(16))) float sC[R][D];              // context
    __shared__ float sE[R][AD_MAXT];                                     // energies, then alpha
    __shared__ float sLog[R][MAXC];
    __shared__ float sSeq[R], sMax[R], sLsum[R];
    __shared__ int sY[R], sPred[R];
    __shared__ int hSym[HL][R], hPred[HL][R], hOut[HL][R];               // the beam's stored decisions
    __shared__ float hScore[HL][R];
    __shared__ int sStop;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, C = a.C, L = a.L;
    // x and xproj of this image: the staged copies are addressed through xs / xps.  Where they stay in global memory every use forms its
    // address from a.x / a.xproj on the spot: a 64-bit base kept live across the step loop costs the five-row kernel 3 % (same file)
    const float* xs = a.x + (long)b * T * D;
    const float* xps = a.xproj + (long)b * T * D;
    if (STAGED) {
        for (int i = tid; i < T * D / 4; i += D) {
            reinterpret_cast<float4*>(staged_lds)[i] = reinterpret_cast<const float4*>(xs)[i];
            reinterpret_cast<float4*>(staged_lds + T * D)[i] = reinterpret_cast<const float4*>(xps)[i];
        }
        xs = staged_lds;
        xps = staged_lds + T * D;
    }
    int cur = 0;
    for (int i = tid; i < R * D; i += D) sS[0][i / D][i % D] = 0.f;
    if (tid < R) { sY[tid] = a.targets ? target_row(a, b, a.tshift) : a.y0; sSeq[tid] = tid == 0 ? 0.f : -INFINITY; }
    if (tid == 0) sStop = 0;
    int done_at = L;                                                    // greedy: the step after the first EOS

    for (int step = 0; step < L; ++step) {
        __syncthreads();
        if (R == 1 && sStop) { done_at = step; break; }
        if (R > 1) {
            bool dead = true;
#pragma unroll
            for (int r = 0; r < R; ++r) dead = dead && sSeq[r] == -INFINITY;
            if (dead) {      // every beam has ended: whatever the network gives, all candidates stay at -inf and the tie rule selects
                             // flat indices 0..R-1 (beam 0, classes 0..R-1); only the bookkeeping goes on
                if (tid < R) { hSym[step][tid] = tid; hPred[step][tid] = 0; hScore[step][tid] = -INFINITY; }
                continue;
            }
        }
        // ---- sProj = Ws s + bs
        {
            float acc[R][4];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.f;
            const float* w = a.WsT + tid;
#pragma unroll U_PROJ
            for (int k = 0; k < D; k += 4) {
                float wk[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) wk[i] = w[(long)(k + i) * D];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 sv = *reinterpret_cast<const float4*>(&sS[cur][r][k]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[r][i] = fmaf(wk[i], comp(sv, i), acc[r][i]);
                }
            }
            const float bias = a.bs[tid];
#pragma unroll
            for (int r = 0; r < R; ++r) sP[r][tid] = sum4(acc[r]) + bias;
        }
        __syncthreads();
        // ---- e[r][t] = wv . tanh(sProj[r] + xproj[t]): one (row, position) pair per wave and trip, a lane holds 4 * NG of the D terms
        {
            float4 wv[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) wv[g] = *reinterpret_cast<const float4*>(a.wv + g * 256 + lane * 4);
            const float wb = a.wb ? a.wb[0] : 0.f;
            for (int p = wave; p < R * T; p += NW) {
                const int r = R == 1 ? 0 : p / T, t = R == 1 ? p : p % T;
                float s = 0.f;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const float4 w = wv[g];
                    const float4 xv = *reinterpret_cast<const float4*>((STAGED ? xps + t * D : a.xproj + ((long)b * T + t) * D) + g * 256 + lane * 4);
                    const float4 pv = *reinterpret_cast<const float4*>(&sP[r][g * 256 + lane * 4]);
                    const float s0 = w.x * tanhf(pv.x + xv.x) + w.y * tanhf(pv.y + xv.y);
                    const float s1 = w.z * tanhf(pv.z + xv.z) + w.w * tanhf(pv.w + xv.w);
                    s = g == 0 ? s0 + s1 : s + (s0 + s1);
                }
                s = wave_sum(s);
                if (lane == 0) sE[r][t] = a.wb ? s + wb : s;
            }
        }
        __syncthreads();
        // ---- alpha = softmax over the T positions (lanes beyond T are padding)
        if (wave < R) {
            const float v = lane < T ? sE[wave][lane] : -INFINITY;
            const float m = wave_max(v);
            const float e = lane < T ? expf(v - m) : 0.f;
            const float s = wave_sum(e);
            if (lane < T) sE[wave][lane] = e / s;
        }
        __syncthreads();
        // ---- context
        {
            float acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = 0.f;
            for (int t = 0; t < T; ++t) {
                const float xv = STAGED ? xs[t * D + tid] : (a.x + (long)b * T * D + tid)[(long)t * D];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(sE[r][t], xv, acc[r]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) sC[r][tid] = acc[r];
        }
        __syncthreads();
        // ---- GRU: thread j owns hidden unit j (its three gate rows of both matrices)
        {
            float ar[R][4], az[R][4], ani[R][4], anh[R][4];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) ar[r][i] = az[r][i] = ani[r][i] = anh[r][i] = 0.f;
            const float* wi = a.WicT + tid;
            const float* wh = a.WhhT + tid;
#pragma unroll U_GRU
            for (int k = 0; k < D; k += 4) {
                float ir[4], iz[4], in_[4], hr[4], hz[4], hn[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long o = (long)(k + i) * (3 * D);
                    ir[i] = wi[o]; iz[i] = wi[o + D]; in_[i] = wi[o + 2 * D];
                    hr[i] = wh[o]; hz[i] = wh[o + D]; hn[i] = wh[o + 2 * D];
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 cv = *reinterpret_cast<const float4*>(&sC[r][k]);
                    const float4 hv = *reinterpret_cast<const float4*>(&sS[cur][r][k]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float c = comp(cv, i), h = comp(hv, i);
                        ar[r][i] = fmaf(ir[i], c, ar[r][i]); ar[r][i] = fmaf(hr[i], h, ar[r][i]);
                        az[r][i] = fmaf(iz[i], c, az[r][i]); az[r][i] = fmaf(hz[i], h, az[r][i]);
                        ani[r][i] = fmaf(in_[i], c, ani[r][i]);
                        anh[r][i] = fmaf(hn[i], h, anh[r][i]);
                    }
                }
            }
            const float br = a.bhh[tid], bz = a.bhh[D + tid], bn = a.bhh[2 * D + tid];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float* e2 = a.E2 + (long)sY[r] * (3 * D);
                const float rg = sigmoid_acc((sum4(ar[r]) + e2[tid]) + br);
                const float zg = sigmoid_acc((sum4(az[r]) + e2[D + tid]) + bz);
                const float n = tanhf((sum4(ani[r]) + e2[2 * D + tid]) + rg * (sum4(anh[r]) + bn));
                sS[cur ^ 1][r][tid] = (1.f - zg) * n + zg * sS[cur][r][tid];
            }
        }
        __syncthreads();
        // ---- logits = fc(s'): 4 quarters of k x MAXC classes, partial sums through LDS
        {
            float (*part)[R][MAXC] = reinterpret_cast<float (*)[R][MAXC]>(&sP[0][0]);
            const int q = tid / MAXC, c = tid % MAXC;
            if (c < C) {
                float acc[R];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = 0.f;
                const float* w = a.fcT + c;
                for (int k = q * (D / 4); k < (q + 1) * (D / 4); k += 4) {
                    float wk[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) wk[i] = w[(long)(k + i) * C];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float4 hv = *reinterpret_cast<const float4*>(&sS[cur ^ 1][r][k]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[r] = fmaf(wk[i], comp(hv, i), acc[r]);
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) part[q][r][c] = acc[r];
            }
            __syncthreads();
            for (int i = tid; i < R * MAXC; i += D) {
                const int r = i / MAXC, cc = i % MAXC;
                if (cc < C) sLog[r][cc] = ((part[0][r][cc] + part[1][r][cc]) + (part[2][r][cc] + part[3][r][cc])) + a.fcb[cc];
            }
        }
        __syncthreads();
        // ---- what the caller wants done with the logits
        if (R == 1) {
            if (a.logits && tid < C) a.logits[((long)b * L + step) * C + tid] = sLog[0][tid];
            if (a.targets) {
                if (tid == 0 && step + 1 + a.tshift < L) sY[0] = target_row(a, b, step + 1 + a.tshift);
            } else if (wave == 0) {
                float v[PC];
#pragma unroll
                for (int i = 0; i < PC; ++i) v[i] = lane + 64 * i < C ? sLog[0][lane + 64 * i] : -INFINITY;
                float bv = v[0]; int bi = lane;
#pragma unroll
                for (int i = 1; i < PC; ++i) if (v[i] > bv) { bv = v[i]; bi = lane + 64 * i; }
                wave_best(bv, bi);
                bi = min(bi, C - 1);                                              // (only matters for NaN logits)
                float s = 0.f;
                if (a.scores) {
#pragma unroll
                    for (int i = 0; i < PC; ++i) {
                        const float e = lane + 64 * i < C ? expf(v[i] - bv) : 0.f;
                        s = i == 0 ? e : s + e;
                    }
                    s = wave_sum(s);
                }
                if (lane == 0) {
                    a.ids[(long)b * L + step] = bi;
                    if (a.scores) a.scores[(long)b * L + step] = 1.f / s;
                    sY[0] = bi + a.yadd;
                    if (bi == a.eos) sStop = 1;
                }
            }
            cur ^= 1;
        } else {
            if (wave < R) {      // log-softmax pieces of row `wave`: max and log of the sum
                float v[PC], m = -INFINITY, s = 0.f;
#pragma unroll
                for (int i = 0; i < PC; ++i) { v[i] = lane + 64 * i < C ? sLog[wave][lane + 64 * i] : -INFINITY; m = i == 0 ? v[i] : fmaxf(m, v[i]); }
                m = wave_max(m);
#pragma unroll
                for (int i = 0; i < PC; ++i) {
                    const float e = lane + 64 * i < C ? expf(v[i] - m) : 0.f;
                    s = i == 0 ? e : s + e;
                }
                s = wave_sum(s);
                if (lane == 0) { sMax[wave] = m; sLsum[wave] = logf(s); }
            }
            __syncthreads();
            if (wave == 0) {     // the R best of the R * C candidates seq[r] + log_softmax[r][c], flat index f = r * C + c
                constexpr int PER = (R * MAXC) / 64;
                float cv[PER]; int ci[PER];
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int f = lane + 64 * i;
                    if (f < R * C) {
                        const int r = f / C, c = f % C;
                        cv[i] = sSeq[r] + ((sLog[r][c] - sMax[r]) - sLsum[r]); ci[i] = f;
                    } else { cv[i] = -INFINITY; ci[i] = 0x7fffffff; }
                }
                float nseq = 0.f; int nsym = 0, npred = 0;
                for (int kk = 0; kk < R; ++kk) {
                    float bv = cv[0]; int bi = ci[0];
#pragma unroll
                    for (int i = 1; i < PER; ++i) if (cand_before(cv[i], ci[i], bv, bi)) { bv = cv[i]; bi = ci[i]; }
                    wave_best(bv, bi);
#pragma unroll
                    for (int i = 0; i < PER; ++i) if (ci[i] == bi) { cv[i] = -INFINITY; ci[i] = 0x7fffffff; }      // taken
                    if (lane == kk) { nseq = bv; nsym = bi % C; npred = min(bi / C, R - 1); }      // (the clamp only matters for NaN scores)
                }
                if (lane < R) {
                    hSym[step][lane] = nsym; hPred[step][lane] = npred; hScore[step][lane] = nseq;
                    sY[lane] = nsym; sPred[lane] = npred;
                    sSeq[lane] = nsym == a.eos ? -INFINITY : nseq;
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) sS[cur][r][tid] = sS[cur ^ 1][sPred[r]][tid];      // state.index_select(predecessors)
        }
    }
    __syncthreads();
    if (R == 1) {
        // greedy: beyond the first EOS the ids are EOS and the scores 0 (the reference goes on decoding there; nothing reads it)
        for (int t = done_at + tid; t < L; t += D) { a.ids[(long)b * L + t] = a.eos; if (a.scores) a.scores[(long)b * L + t] = 0.f; }
        return;
    }
    // ---- the beam's backtracking (attention_recognition_head.py:127-187), on this image's R slots
    if (tid == 0) {
        int tp[R]; float s[R]; bool used[R];
        for (int k = 0; k < R; ++k) used[k] = false;
        for (int k = 0; k < R; ++k) {                 // stored_scores[-1].topk(R)
            int best = -1;
            for (int j = 0; j < R; ++j)
                if (!used[j] && (best < 0 || cand_before(hScore[L - 1][j], j, hScore[L - 1][best], best))) best = j;
            used[best] = true; tp[k] = best; s[k] = hScore[L - 1][best];
        }
        int found = 0;
        for (int t = L - 1; t >= 0; --t) {
            int cs[R], np[R];
            for (int k = 0; k < R; ++k) { cs[k] = hSym[t][tp[k]]; np[k] = hPred[t][tp[k]]; }
            for (int k = 0; k < R; ++k) tp[k] = np[k];
            for (int j = R - 1; j >= 0; --j)
                if (hSym[t][j] == a.eos) {
                    const int rk = R - (found % R) - 1;
                    ++found;
                    tp[rk] = hPred[t][j]; cs[rk] = hSym[t][j]; s[rk] = hScore[t][j];
                }
            for (int k = 0; k < R; ++k) hOut[t][k] = cs[k];
        }
        int best = 0;                                 // s.topk(R)[0]
        for (int k = 1; k < R; ++k) if (cand_before(s[k], k, s[best], best)) best = k;
        sPred[0] = best;
    }
    __syncthreads();
    for (int t = tid; t < L; t += D) { a.ids[(long)b * L + t] = hOut[t][sPred[0]]; a.scores[(long)b * L + t] = 1.f; }
}

template <int D, int R>
static int attn_decode_launch(const AttnDecArgs& a, hipStream_t st) {
    if (attn_staged(D)) {
        static TattPerDevice site;
        tatt_per_device(site, [] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_decode_kernel<D, R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      2 * AD_MAXT * D * (int)sizeof(float));
        });
    }
    hipLaunchKernelGGL((attn_decode_kernel<D, R>), dim3(a.B), dim3(D), attn_staged(D) ? 2 * a.T * D * sizeof(float) : 0, st, a);
    return LAUNCH_CHECK();
}

// ASTER's head: <BOS> = row C starts a row, an arg-max is its own embedding row, forced step i reads targets[i - 1], greedy rows stop at EOS
TATT_API int tatt_attn_decode(const float* x, const float* xproj, const float* WsT, const float* bs, const float* wv, const float* wb,
                              const float* E2, const float* WicT, const float* WhhT, const float* bhh, const float* fcT,
                              const float* fcb, const int* targets, float* logits, int* ids, float* scores, int B, int T, int C, int L,
                              int sDim, int attDim, int xDim, int eos, int mode, int beam, hipStream_t st) {
    if (sDim != 512 || attDim != 512 || xDim != 512) return 1;
    if (B < 1 || T < 1 || T > AD_MAXT || C < 2 || C > 128 || L < 1 || L > 100 || mode < 0 || mode > 2) return 1;
    if (mode == 0 && (!targets || !logits)) return 1;
    if (mode != 0 && (!ids || !scores)) return 1;
    if (mode == 2 && (beam != 5 || C < 5)) return 1;
    const bool forced = mode == 0;
    AttnDecArgs a = {x, xproj, WsT, bs, wv, wb, E2, WicT, WhhT, bhh, fcT, fcb, forced ? targets : nullptr, forced ? logits : nullptr,
                     forced ? nullptr : ids, forced ? nullptr : scores, B, T, C, L, eos, C, 0, -1};
    return mode == 2 ? attn_decode_launch<512, 5>(a, st) : attn_decode_launch<512, 1>(a, st);
}

// MORAN's `Attention`: row 0 starts a greedy row, an arg-max c reads row c + 1, forced step i reads targets[i], no stop, no score bias
TATT_API int tatt_moran_decode(const float* feats, const float* fproj, const float* WhT, const float* bh, const float* wv,
                               const float* E2, const float* WicT, const float* WhhT, const float* bhh, const float* genT,
                               const float* genb, const int* targets, float* logits, int* ids, int B, int T, int C, int L, int H,
                               int mode, hipStream_t st) {
    if (H != 256) return 1;
    if (B < 1 || T < 1 || T > AD_MAXT || C < 2 || C > 64 || L < 1 || L > 64 || mode < 0 || mode > 1) return 1;
    if (!logits || (mode == 0 && !targets) || (mode == 1 && !ids)) return 1;
    AttnDecArgs a = {feats, fproj, WhT, bh, wv, nullptr, E2, WicT, WhhT, bhh, genT, genb, mode == 0 ? targets : nullptr, logits,
                     mode == 1 ? ids : nullptr, nullptr, B, T, C, L, -1, 0, 1, 0};
    return attn_decode_launch<256, 1>(a, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The beam's backtracking alone, for the step-by-step route (the one launch does it in LDS): stored decisions sym, pred (slot of the
// previous step, clamped to [0, K)), score, each (L, B, K) -> ids (B, L) of the best sequence per image.  One thread per image (a chain of
// L dependent steps on K slots); ws (B, L, K) ints holds the sequences until the final order is known.
#define BT_MAXK 8
__global__ void beam_backtrack_kernel(const int* __restrict__ sym, const int* __restrict__ pred, const float* __restrict__ score,
                                      int* __restrict__ ids, int* __restrict__ ws, int L, int B, int K, int eos) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int tp[BT_MAXK]; float s[BT_MAXK]; bool used[BT_MAXK];
    const long last = ((long)(L - 1) * B + b) * K;
    for (int k = 0; k < K; ++k) used[k] = false;
    for (int k = 0; k < K; ++k) {
        int best = -1;
        for (int j = 0; j < K; ++j)
            if (!used[j] && (best < 0 || cand_before(score[last + j], j, score[last + best], best))) best = j;
        used[best] = true; tp[k] = best; s[k] = score[last + best];
    }
    int found = 0;
    for (int t = L - 1; t >= 0; --t) {
        const long o = ((long)t * B + b) * K;
        int cs[BT_MAXK], np[BT_MAXK];
        for (int k = 0; k < K; ++k) { cs[k] = sym[o + tp[k]]; np[k] = min(max(pred[o + tp[k]], 0), K - 1); }
        for (int k = 0; k < K; ++k) tp[k] = np[k];
        for (int j = K - 1; j >= 0; --j)
            if (sym[o + j] == eos) {
                const int rk = K - (found % K) - 1;
                ++found;
                tp[rk] = min(max(pred[o + j], 0), K - 1); cs[rk] = eos; s[rk] = score[o + j];
            }
        for (int k = 0; k < K; ++k) ws[((long)b * L + t) * K + k] = cs[k];
    }
    int best = 0;
    for (int k = 1; k < K; ++k) if (cand_before(s[k], k, s[best], best)) best = k;
    for (int t = 0; t < L; ++t) ids[(long)b * L + t] = ws[((long)b * L + t) * K + best];
}
TATT_API int tatt_beam_backtrack(const int* sym, const int* pred, const float* score, int* ids, int* ws, int L, int B, int K, int eos,
                                 hipStream_t st) {
    if (L < 1 || B < 1 || K < 1 || K > BT_MAXK) return 1;
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, sym, pred, score, ids, ws, L, B, K, eos);
    return LAUNCH_CHECK();
}
