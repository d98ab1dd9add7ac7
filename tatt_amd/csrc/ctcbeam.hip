// CTC prefix beam search of the line reader (tatt_amd/read.py `ctc_beam_read_host` is the specification, tests/test_beam*.py hold the
// kernel to it): the N most probable STRINGS of a line, each with its log-probability summed over its alignments.
//   ctc_beam_read_kernel    one line per wave (a work-group of 64 lanes), no exchange between lines.  Per step: the log-soft-max in
//                           float64 with lane = class; lane r < |beam| works out the stay candidate of beam entry r; lane c then holds the
//                           candidates (r, c) of all r in registers (key r C + c: c = 0 is the stay candidate, c >= 1 the extension of r by
//                           c); `beam` rounds of a wave maximum (ties to the lower key) pick the new beam in descending order.
// A prefix is a node of the line's trie (parent node, class), at most 1 + T beam nodes, all in LDS.  IDENTITY IS THE NODE: a string has one
// node for the whole launch, because a selected extension (parent, class) is looked up in an open-addressing table of the line before a
// node is made -- also when its prefix had left the beam and comes back while strings that start with it stayed.  With unique nodes, "the
// extension of q by c is the beam entry r" is exactly parent[node r] == node q and class[node r] == c: such an extension adds into r's
// stay candidate and is no candidate of its own.  The table has CB_TABLE > 2 CB_NODES slots, so a probe sequence ends at an empty slot; it is
// bounded by CB_TABLE all the same, and a key that cannot be placed raises the line's flag.
// All of pb, pnb, lse and the log-soft-max are float64 (the logits are fp32); nothing is rounded to fp32 on the way into the record.
// Every loop is bounded by T, C, CB_BEAM, CB_TABLE or a literal; the candidate registers are indexed by unrolled loops only (no scratch).
// Wave-wide maxima, minima and sums go through data-parallel-primitive moves (row shifts, row broadcasts) and a lane read: no LDS, and
// the result is the same in every lane.  The kernel is instantiated for 4, 8 and 16 beam entries; a launch takes the smallest that fits.
// LM = true (tatt_ctc_beam_lm_read; specification `ctc_beam_lm_read_host`) fuses a character n-gram model into the search: every entry
// carries one more float64, the sum of the increments W[history][class] of its string (the host's table `CharLM.increments`: weight and
// bonus are already in it, so the kernel only ADDS entries of the table, left to right, and the term is the specification's bit for bit);
// candidates are ranked by acoustic + LM, the record keeps the two apart, and after the last step the beam is ranked once more with the
// end-of-line increment W[history][0] added.  Every LM statement stands under `if constexpr (LM)`.
// PAT = true (tatt_ctc_beam_pattern_read; specification `ctc_beam_pattern_read_host`) holds the search to a format, a DFA over the classes
// (`read.Pattern`: `ptab` S rows of C bytes, the next state or 255; `pacc` S bytes): the DFA state is a property of the trie NODE, one
// byte written where the node is made (so a prefix that leaves the beam and comes back keeps its state; the byte is loaded by the lane
// that selected the extension, beside its table look-up, and lane 0, which places the nodes one after the other, only copies it); lane c tests
// ptab[state_r C + c] for its BM candidates where the LM loads stand, an extension the format does not continue with is no candidate,
// and after the last step the entries in a non-accepting state are dropped, the rest keeping their order.  An extension that spells a
// prefix already in the beam needs no test: that prefix's node was made through the same table entry.  A table entry >= S is read as
// 255, so no content of the table can lead a load astray.  The record row is the plain search's.  Every statement of it stands under
// `if constexpr (PAT)`; only <BM, false, true> is instantiated.
#include "common.h"
#include "ctc_f64.h"                                           // CB_NEG, cb_lse, the wave maxima / minima / sums

#define CB_MAX_T 256
#define CB_MAX_C 64
#define CB_BEAM 16
#define CB_NODES (1 + CB_MAX_T * CB_BEAM)      // the root and at most `beam` new nodes per step
#define CB_TABLE 16384                         // slots of the (parent, class) -> node table: a power of two above 2 CB_NODES
#define CB_TABLE_BITS 14
#define CB_EMPTY 0xffff

static_assert(CB_TABLE > 2 * CB_NODES && CB_TABLE == 1 << CB_TABLE_BITS && CB_NODES < CB_EMPTY, "table and node ids");

// 32-bit words of one entry of a record row: float64 logp (2) | length | pad | cap classes, an even count
static __host__ __device__ inline int cb_entry_words(int cap) { return 4 + cap + (cap & 1); }
// with a language model: float64 logp (2) | float64 lm (2) | length | pad | cap classes, an even count
static __host__ __device__ inline int cb_lm_entry_words(int cap) { return 6 + cap + (cap & 1); }
#define CB_MAX_S 64                            // most states of a format's DFA (PAT): a state is a byte, 255 says "no such string"
#define CB_LM_ORDER 3                          // most classes of an n-gram: the table has C^order entries, at most 64^3 doubles = 2 MB

__device__ __forceinline__ unsigned cb_hash(int parent, int c) {
    return ((unsigned)(parent * CB_MAX_C + c) * 2654435761u) >> (32 - CB_TABLE_BITS);
}

// BM: the beam entries the kernel keeps registers and unrolled loops for (beam <= BM <= CB_BEAM): a launch takes the smallest that fits.
// LM: lmw is the table W of C^order doubles, row = the last order - 1 classes of a prefix (0: before the line begins), column = the class
template <int BM, bool LM, bool PAT>
__global__ __launch_bounds__(64) void ctc_beam_read_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c, int T,
                                                           int C, int beam, int nbest, const int* __restrict__ index,
                                                           int* __restrict__ record, int n_rows, int cap, long st_rec,
                                                           const double* __restrict__ lmw, int order,
                                                           const unsigned char* __restrict__ ptab,
                                                           const unsigned char* __restrict__ pacc, int S) {
    __shared__ double lp[CB_MAX_C];                                  // the step's log-soft-max
    __shared__ double pb[2][CB_BEAM], pnb[2][CB_BEAM], tot[2][CB_BEAM];      // the beam, by rank; [cur] is read, [cur ^ 1] written
    __shared__ int node[2][CB_BEAM];
    __shared__ double spb[CB_BEAM], spnb[CB_BEAM], stot[CB_BEAM];    // the stay candidate of every entry
    __shared__ int ext_par[CB_BEAM], ext_cls[CB_BEAM];               // selected extensions that still need their node
    __shared__ unsigned short kill[CB_BEAM * CB_MAX_C];              // [r][c] == t + 1: the extension of r by c went into a stay candidate
    __shared__ unsigned short par[CB_NODES];                         // the trie
    __shared__ unsigned char cls[CB_NODES];
    __shared__ unsigned short table[CB_TABLE];                       // node id or CB_EMPTY
    __shared__ int state_sh[2];                                      // nodes in use, flag
    __shared__ int len_sh[CB_BEAM];
    __shared__ int last_sh[CB_BEAM];                                 // the last class of every entry's prefix, -1 for the empty one
    __shared__ double lmv[2][LM ? CB_BEAM : 1];                      // LM: the LM term of every entry, by rank, buffered as the beam is
    __shared__ int ctx[LM ? CB_BEAM : 1];                            // LM: the row of W that every entry's prefix selects
    __shared__ unsigned char nstate[PAT ? CB_NODES : 1];             // PAT: the DFA state of every node's string
    __shared__ int pst[PAT ? CB_BEAM : 1];                           // PAT: the DFA state of every entry, by rank
    __shared__ int ext_st[PAT ? CB_BEAM : 1];                        // PAT: the DFA state of a selected extension that needs its node
    const int lane = threadIdx.x;
    const float* x = logits + blockIdx.x * st_b + lane * st_c;

    for (int i = lane; i < CB_TABLE; i += 64) table[i] = CB_EMPTY;
    for (int i = lane; i < CB_BEAM * CB_MAX_C; i += 64) kill[i] = 0;
    if (lane < 2 * CB_BEAM) {                                        // (entries beyond the beam are read, and selected away: keep them tame)
        (&pb[0][0])[lane] = CB_NEG;
        (&tot[0][0])[lane] = CB_NEG;
        if (lane < CB_BEAM) {
            stot[lane] = CB_NEG;
            last_sh[lane] = -1;
            if constexpr (LM) ctx[lane] = 0;                         // (rows beyond the beam are loaded from, too: row 0)
            if constexpr (PAT) pst[lane] = 0;                        // (likewise: state 0)
        }
        if constexpr (LM) (&lmv[0][0])[lane] = 0.0;                  // (the empty prefix: 0)
    }
    __syncthreads();
    if (lane == 0) {
        par[0] = 0;
        cls[0] = 0;
        if constexpr (PAT) nstate[0] = 0;                            // the start state
        node[0][0] = 0;                                              // the empty prefix is the root
        pb[0][0] = 0.0;
        pnb[0][0] = CB_NEG;
        tot[0][0] = 0.0;
        state_sh[0] = 1;
        state_sh[1] = 0;
    }
    int nb = 1, cur = 0, flag = 0;                                   // (the same in every lane)
    float xn = lane < C ? x[0] : -INFINITY;
    __syncthreads();

#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const float xc = xn;
        if (t + 1 < T) xn = lane < C ? x[(t + 1) * st_t] : -INFINITY;        // (in flight during this step)
        // ---- the log-soft-max, lane = class ----
        const float mx = cb_wave_max(xc);                              // (fmaxf skips a NaN: looked for on its own)
        if (__ballot(xc != xc || xc == INFINITY) != 0 || mx == -INFINITY) {
            flag = 1;
            break;
        }
        const double d = (double)xc - (double)mx;
        const double s = cb_wave_sum(lane < C ? exp(d) : 0.0);
        const double lpc = d - log(s);                               // (-inf beyond C)
        if (lane < C) lp[lane] = lpc;
        __syncthreads();
        // ---- lane r: the stay candidate of entry r, with the extension that spells the same string ----
        if (lane < nb) {
            const int nd = node[cur][lane];
            const double a = tot[cur][lane] + lp[0];
            double b = CB_NEG;
            last_sh[lane] = nd != 0 ? cls[nd] : -1;
            if constexpr (PAT) pst[lane] = nstate[nd];
            if constexpr (LM) {                                      // (the root: cls[0] = par[0] = 0, "before the line begins")
                const int c1 = cls[nd], c2 = cls[par[nd]];
                ctx[lane] = order == 1 ? 0 : order == 2 ? c1 : c2 * C + c1;
            }
            if (nd != 0) {
                const int last = cls[nd], p = par[nd];
                b = pnb[cur][lane] + lp[last];
                int q = -1;                                          // (at most one: the nodes of a beam are distinct)
#pragma unroll
                for (int i = 0; i < BM; ++i)
                    if (i < nb && node[cur][i] == p) q = i;
                if (q >= 0) {
                    const int last_q = p != 0 ? cls[p] : -1;
                    b = cb_lse(b, (last == last_q ? pb[cur][q] : tot[cur][q]) + lp[last]);
                    kill[q * CB_MAX_C + last] = (unsigned short)(t + 1);
                }
            }
            spb[lane] = a;
            spnb[lane] = b;
            stot[lane] = cb_lse(a, b);
        }
        __syncthreads();
        // ---- lane c: the candidates (r, c) of every r ----
        double v[BM];                                                // (every load below is issued whatever nb is: no branch, one wait)
        double w[LM ? BM : 1];
        if constexpr (LM) {
#pragma unroll
            for (int r = 0; r < BM; ++r) w[r] = lmw[lane < C ? ctx[r] * C + lane : 0];       // (coalesced; the table lives in L2)
        }
        bool go[PAT ? BM : 1];                                       // PAT: the format continues from entry r with this lane's class
        if constexpr (PAT) {
#pragma unroll
            for (int r = 0; r < BM; ++r) go[r] = ptab[lane < C ? pst[r] * C + lane : 0] < S;         // (at most 4 KB: it lives in L2)
        }
#pragma unroll
        for (int r = 0; r < BM; ++r) {
            const double ext = (lane == last_sh[r] ? pb[cur][r] : tot[cur][r]) + lpc;
            const bool struck = kill[r * CB_MAX_C + lane] == (unsigned short)(t + 1);
            double val;
            if constexpr (LM)                                        // (first the LM term of the candidate, then the one sum)
                val = lane == 0 ? stot[r] + lmv[cur][r] : (struck ? CB_NEG : ext + (lmv[cur][r] + w[r]));
            else if constexpr (PAT)
                val = lane == 0 ? stot[r] : (struck || !go[r] ? CB_NEG : ext);
            else
                val = lane == 0 ? stot[r] : (struck ? CB_NEG : ext);
            v[r] = r < nb && lane < C ? val : CB_NEG;
        }
        // ---- the `beam` largest, descending, ties to the lower key; lane i keeps the i-th ----
        int nsel = 0, my_r = 0, my_c = 0;
        double my_val = CB_NEG;
        for (int i = 0; i < beam; ++i) {
            double bv = CB_NEG;
            int br = 0;
#pragma unroll
            for (int r = 0; r < BM; ++r)
                if (v[r] > bv) { bv = v[r]; br = r; }                // (the lowest r among equals: this lane's lowest key)
            const double top = cb_wave_maxd(bv);                     // (the same in every lane)
            if (top == CB_NEG) break;                                // fewer candidates than `beam`
            const unsigned long long eq = __ballot(bv == top);
            int wc = __ffsll(eq) - 1;
            int wr = __builtin_amdgcn_readlane(br, wc);
            if (eq & (eq - 1)) {                                     // equal values in several lanes: the lowest key r C + c
                const int k = cb_wave_mini(bv == top ? br * C + lane : 0x7fffffff);
                wr = k / C;
                wc = k - wr * C;
            }
            if (lane == wc) {
#pragma unroll
                for (int r = 0; r < BM; ++r)
                    if (r == wr) v[r] = CB_NEG;
            }
            if (lane == i) { my_r = wr; my_c = wc; my_val = top; }
            ++nsel;
        }
        nsel = __builtin_amdgcn_readfirstlane(nsel);
        // ---- lane i: entry i of the new beam.  A selected extension LOOKS UP (parent, class) first: nothing writes the table meanwhile ----
        const int nxt = cur ^ 1;
        bool miss = false;
        if (lane < nsel) {
            const int r = my_r, c = my_c;
            if (c == 0) {
                node[nxt][lane] = node[cur][r];
                pb[nxt][lane] = spb[r];
                pnb[nxt][lane] = spnb[r];
                if constexpr (LM) {
                    my_val = stot[r];                                // (my_val was the score: the acoustic sum again)
                    lmv[nxt][lane] = lmv[cur][r];
                }
            } else {
                const int p = node[cur][r];
                if constexpr (LM) {                                  // (the operations of the candidate phase on the same operands)
                    my_val = (c == last_sh[r] ? pb[cur][r] : tot[cur][r]) + lp[c];
                    lmv[nxt][lane] = lmv[cur][r] + lmw[ctx[r] * C + c];
                }
                pb[nxt][lane] = CB_NEG;
                pnb[nxt][lane] = my_val;
                const unsigned h = cb_hash(p, c);
                int found = -1;
                for (int probe = 0; probe < CB_TABLE; ++probe) {
                    const int e = table[(h + probe) & (CB_TABLE - 1)];
                    if (e == CB_EMPTY) break;
                    if (par[e] == p && cls[e] == c) {
                        found = e;
                        break;
                    }
                }
                miss = found < 0;
                node[nxt][lane] = miss ? 0 : found;
                ext_par[lane] = p;
                ext_cls[lane] = c;
                if constexpr (PAT) ext_st[lane] = ptab[pst[r] * C + c];      // (lane i's own load, beside its look-up; < S: it was a candidate)
            }
            tot[nxt][lane] = my_val;
        }
        // ---- a node is made only where there was none: the keys of one step differ, so lane 0 places them one after the other ----
        const unsigned long long todo = __ballot(miss);
        if (todo != 0) {                                             // (the same in every lane)
            __syncthreads();
            if (lane == 0) {
                int nn = state_sh[0], bad = 0;
                for (int i = 0; i < nsel; ++i) {
                    if (!((todo >> i) & 1)) continue;
                    const int c = ext_cls[i], p = ext_par[i];
                    const unsigned h = cb_hash(p, c);
                    int made = -1;
                    for (int probe = 0; probe < CB_TABLE && nn < CB_NODES; ++probe) {
                        const unsigned slot = (h + probe) & (CB_TABLE - 1);
                        if (table[slot] != CB_EMPTY) continue;       // (another key: this one is not in the table)
                        par[nn] = (unsigned short)p;
                        cls[nn] = (unsigned char)c;
                        if constexpr (PAT) nstate[nn] = (unsigned char)ext_st[i];
                        table[slot] = (unsigned short)nn;
                        made = nn++;
                        break;
                    }
                    if (made < 0) { bad = 1; made = 0; }
                    node[nxt][i] = made;
                }
                state_sh[0] = nn;
                if (bad) state_sh[1] = 1;
            }
        }
        __syncthreads();
        nb = nsel;
        cur = nxt;
        if (state_sh[1] != 0) {                                      // (cannot happen with the table sized as it is)
            flag = 1;
            break;
        }
    }

    // ---- the record row ----
    const int row = index[blockIdx.x];
    if (row < 0 || row >= n_rows) return;
    int* rec = record + row * st_rec;
    if (flag) {
        if (lane == 0) {
            rec[0] = 0;
            rec[1] = 1;
        }
        return;
    }
    constexpr int HD = LM ? 6 : 4;                                   // words of an entry before its classes
    int n_out = nb < nbest ? nb : nbest;
    const int es = LM ? cb_lm_entry_words(cap) : cb_entry_words(cap);
    int src = lane;                                                  // the beam entry that record entry `lane` is
    if constexpr (LM) {
        // ---- the line ends here: final = (tot + lm) + W[history][0]; descending, ties to the lower rank.  The step loop is over, so
        // stot takes the finals, spb the LM terms with the end increment, ext_par the beam entry of every position ----
        if (lane < nb) {
            const int nd = node[cur][lane], c1 = cls[nd], c2 = cls[par[nd]];
            const double wend = lmw[(order == 1 ? 0 : order == 2 ? c1 : c2 * C + c1) * C];
            stot[lane] = (tot[cur][lane] + lmv[cur][lane]) + wend;
            spb[lane] = lmv[cur][lane] + wend;
        }
        __syncthreads();
        if (lane < nb) {
            const double f = stot[lane];
            int pos = 0;
#pragma unroll
            for (int j = 0; j < BM; ++j)
                if (j < nb && (stot[j] > f || (stot[j] == f && j < lane))) ++pos;
            ext_par[pos] = lane;
        }
        __syncthreads();
        if (lane < n_out) src = ext_par[lane];
    }
    if constexpr (PAT) {
        // ---- the line ends here: entries whose state does not accept are dropped, the rest keep their order.  The step loop is over,
        // so ext_cls takes "entry r is accepted", ext_par the beam entry of every position ----
        if (lane < nb) {
            const int q = nstate[node[cur][lane]];
            ext_cls[lane] = q < S && pacc[q] != 0;
        }
        __syncthreads();
        int pos = 0, kept = 0;
#pragma unroll
        for (int j = 0; j < BM; ++j) {
            const int a = j < nb ? ext_cls[j] : 0;
            kept += a;
            if (j < lane) pos += a;
        }
        if (lane < nb && ext_cls[lane] != 0) ext_par[pos] = lane;
        __syncthreads();
        n_out = kept < nbest ? kept : nbest;
        if (lane < n_out) src = ext_par[lane];
    }
    if (lane < n_out) {                                              // lane i walks its entry back to the root
        int* e = rec + 2 + lane * es;
        const int first = node[cur][src];
        int len = 0;
        for (int nd = first; nd != 0 && len < T; nd = par[nd]) ++len;        // (a node's depth is at most the steps taken: len <= T <= cap)
        const double lg = tot[cur][src];
        e[0] = __double2loint(lg);
        e[1] = __double2hiint(lg);
        if constexpr (LM) {
            const double lm = spb[src];
            e[2] = __double2loint(lm);
            e[3] = __double2hiint(lm);
        }
        e[HD - 2] = len;
        e[HD - 1] = 0;
        int nd = first;
        for (int k = len - 1; k >= 0; --k) {
            e[HD + k] = cls[nd];
            nd = par[nd];
        }
        len_sh[lane] = len;
    }
    __syncthreads();
    for (int i = 0; i < n_out; ++i) {
        int* e = rec + 2 + i * es;
        for (int k = len_sh[i] + lane; k < es - HD; k += 64) e[HD + k] = -1;
    }
    if (lane == 0) {
        rec[0] = n_out;
        rec[1] = 0;
    }
}

template <bool LM, bool PAT>
static int cb_launch(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest, const int* index,
                     int* record, int n_rows, int cap, long st_rec, const double* lmw, int order, const unsigned char* ptab,
                     const unsigned char* pacc, int S, hipStream_t st) {
    if (!logits || !index || !record) return 1;
    if (T <= 0 || T > CB_MAX_T || B <= 0 || C <= 0 || C > CB_MAX_C || n_rows <= 0 || cap < T) return 1;
    const int es = LM ? cb_lm_entry_words(cap) : cb_entry_words(cap);
    if (nbest < 1 || nbest > beam || beam > CB_BEAM || st_rec < 2 + (long)nbest * es) return 1;
    if (beam <= 4)
        hipLaunchKernelGGL((ctc_beam_read_kernel<4, LM, PAT>), dim3(B), dim3(64), 0, st, logits, st_t, st_b, st_c, T, C, beam, nbest, index,
                           record, n_rows, cap, st_rec, lmw, order, ptab, pacc, S);
    else if (beam <= 8)
        hipLaunchKernelGGL((ctc_beam_read_kernel<8, LM, PAT>), dim3(B), dim3(64), 0, st, logits, st_t, st_b, st_c, T, C, beam, nbest, index,
                           record, n_rows, cap, st_rec, lmw, order, ptab, pacc, S);
    else
        hipLaunchKernelGGL((ctc_beam_read_kernel<CB_BEAM, LM, PAT>), dim3(B), dim3(64), 0, st, logits, st_t, st_b, st_c, T, C, beam, nbest,
                           index, record, n_rows, cap, st_rec, lmw, order, ptab, pacc, S);
    return LAUNCH_CHECK();
}

TATT_API int tatt_ctc_beam_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest,
                                const int* index, int* record, int n_rows, int cap, long st_rec, hipStream_t st) {
    return cb_launch<false, false>(logits, st_t, st_b, st_c, T, B, C, beam, nbest, index, record, n_rows, cap, st_rec, nullptr, 0, nullptr,
                                   nullptr, 0, st);
}

// the search with the increments table `lmw` of lm_classes^order float64 entries on the device (read.CharLM.increments)
TATT_API int tatt_ctc_beam_lm_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest,
                                   const double* lmw, int order, int lm_classes, const int* index, int* record, int n_rows, int cap,
                                   long st_rec, hipStream_t st) {
    if (!lmw || order < 1 || order > CB_LM_ORDER || lm_classes != C) return 1;
    return cb_launch<true, false>(logits, st_t, st_b, st_c, T, B, C, beam, nbest, index, record, n_rows, cap, st_rec, lmw, order, nullptr,
                                  nullptr, 0, st);
}

// the search held to a format: table S rows of C bytes (the next state, or 255), accept S bytes, both on the device (read.Pattern)
TATT_API int tatt_ctc_beam_pattern_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest,
                                        const unsigned char* table, const unsigned char* accept, int S, const int* index, int* record,
                                        int n_rows, int cap, long st_rec, hipStream_t st) {
    if (!table || !accept || S < 1 || S > CB_MAX_S) return 1;
    return cb_launch<false, true>(logits, st_t, st_b, st_c, T, B, C, beam, nbest, index, record, n_rows, cap, st_rec, nullptr, 0, table,
                                  accept, S, st);
}

TATT_API int tatt_lm_limits(int* out) {
    if (!out) return 1;
    out[0] = CB_LM_ORDER;
    out[1] = CB_MAX_C;
    return 0;
}

TATT_API int tatt_beam_limits(int* out) {
    if (!out) return 1;
    out[0] = CB_MAX_T;
    out[1] = CB_MAX_C;
    out[2] = CB_BEAM;
    out[3] = CB_NODES;
    out[4] = CB_TABLE;
    return 0;
}
