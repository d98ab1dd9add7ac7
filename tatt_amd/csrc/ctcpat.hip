// The exact probability that a line reads as ANY member of a format (tatt_amd/read.py `ctc_pattern_mass_host` is the specification,
// tests/test_pattern*.py hold the kernel to it): the format is a DFA of S states over the C classes (`read.Pattern`), and
//   A[q][e] = the mass of the alignments so far whose collapsed string has driven the DFA to q and that end in the blank (e = 0) or in
//             the class e
// is carried through the T steps in float64 PROBABILITIES (not logs), so that every quantity is a sum of non-negative terms and
// nothing is ever subtracted:
//   A'[q][0]            += p_0 (sum over e of A[q][e])
//   A'[q][c]            += p_c A[q][c]                              the class repeats: same string, same state
//   A'[table[q][c]][c]  += p_c (sum over e != c of A[q][e])         where the format continues with c
//   ctc_pattern_mass_kernel   one line per wave, lane = class.  Lane c OWNS column c of A in LDS (both buffers): it alone reads and
//                             writes A[.][c], one q after the other, so there are no atomics, no barriers inside the step loop and
//                             the order of every sum is fixed.  What crosses lanes goes through data-parallel-primitive moves: the
//                             row's total (cb_wave_sum) and the sum over the OTHER classes as an exclusive prefix scan plus an
//                             exclusive suffix scan.  A row of A whose total is 0 is skipped (the same decision in every lane).
// After a step the largest entry's binary exponent is taken out of all of A: the power of two is applied on the next READ (ldexp: exact
// but for underflow) and the exponents are summed as an integer.  mass = log(sum over accepting q and all e of A[q][e]) + exponent ln 2,
// -inf where nothing is accepted in T steps.  A line with a NaN, a +inf or a step without a finite logit gives NaN and flag 1.
// Dynamic LDS: 2 S C doubles (the two buffers of A; a buffer is zeroed as it is read, so the next step finds it clean) and the S C bytes
// of the table.  Every loop is bounded by T, S, C or a literal.
#include "common.h"
#include "ctc_f64.h"

#define CP_MAX_T 256
#define CP_MAX_C 64
#define CP_MAX_S 64
#define CP_BEAM 16                                                   // most beam entries of tatt_ctc_beam_pattern_read (ctcbeam.hip's CB_BEAM)
#define CP_DEAD 255                                                  // table entry: no string of the format continues this way
#define CP_OUT_WORDS 4                                               // float64 mass (2) | flag | 0
#define CP_LDS_MAX (2 * CP_MAX_S * CP_MAX_C * 8 + CP_MAX_S * CP_MAX_C)

static __host__ __device__ inline int cp_lds_bytes(int S, int C) { return 2 * S * C * 8 + (S * C + 7) / 8 * 8; }

__global__ __launch_bounds__(64) void ctc_pattern_mass_kernel(const float* __restrict__ logits, long st_t, long st_b, long st_c, int T,
                                                              int C, const unsigned char* __restrict__ table,
                                                              const unsigned char* __restrict__ accept, int S,
                                                              const int* __restrict__ index, int* __restrict__ out, int n_rows,
                                                              long st_out) {
    extern __shared__ double cp_lds_base[];
    double* A = cp_lds_base;                                         // [2][S][C]
    unsigned char* tb = reinterpret_cast<unsigned char*>(A + 2 * S * C);         // [S][C]
    const int lane = threadIdx.x, SC = S * C;
    const float* x = logits + blockIdx.x * st_b + lane * st_c;

    for (int i = lane; i < 2 * SC; i += 64) A[i] = 0.0;
    for (int i = lane; i < SC; i += 64) tb[i] = table[i];
    __syncthreads();
    if (lane == 0) A[0] = 1.0;                                       // the empty string, state 0, "ends in the blank"
    __syncthreads();
    int cur = 0, shift = 0, flag = 0;                                // shift: the exponent the entries of A[cur] still carry
    long expo = 0;
    float xn = lane < C ? x[0] : -INFINITY;

#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const float xc = xn;
        if (t + 1 < T) xn = lane < C ? x[(t + 1) * st_t] : -INFINITY;
        const float mx = cb_wave_max(xc);
        if (__ballot(xc != xc || xc == INFINITY) != 0 || mx == -INFINITY) {
            flag = 1;
            break;
        }
        const double e = lane < C ? exp((double)xc - (double)mx) : 0.0;
        const double p = e / cb_wave_sum(e);                         // the soft-max of this lane's class
        double* Ac = A + cur * SC;
        double* An = A + (cur ^ 1) * SC;
        for (int q = 0; q < S; ++q) {
            double a = 0.0;
            if (lane < C) {
                a = ldexp(Ac[q * C + lane], -shift);
                Ac[q * C + lane] = 0.0;                              // (the buffer the step after this one accumulates into)
            }
            const double tot = cb_wave_sum(a);                       // (the same in every lane)
            if (tot == 0.0) continue;
            const double others = cb_wave_excl_prefix(a, lane) + cb_wave_excl_suffix(a, lane);
            if (lane == 0) {
                An[q * C] += p * tot;
            } else if (lane < C) {
                An[q * C + lane] += p * a;
                const int to = tb[q * C + lane];
                if (to < S) An[to * C + lane] += p * others;
            }
        }
        double m = 0.0;
        if (lane < C)
            for (int q = 0; q < S; ++q) m = fmax(m, An[q * C + lane]);
        m = cb_wave_maxd(m);
        shift = 0;
        if (m > 0.0) (void)frexp(m, &shift);                         // m = f 2^shift, 0.5 <= f < 1
        expo += shift;
        cur ^= 1;
    }

    const int row = index[blockIdx.x];
    if (row < 0 || row >= n_rows) return;
    double mass = __longlong_as_double(0x7ff8000000000000ll);        // NaN
    if (!flag) {
        const double* Ac = A + cur * SC;
        double s = 0.0;
        if (lane < C)
            for (int q = 0; q < S; ++q)
                if (accept[q] != 0) s += ldexp(Ac[q * C + lane], -shift);
        s = cb_wave_sum(s);
        mass = s > 0.0 ? log(s) + (double)expo * 0.693147180559945309417 : CB_NEG;
    }
    if (lane == 0) {
        int* o = out + row * st_out;
        o[0] = __double2loint(mass);
        o[1] = __double2hiint(mass);
        o[2] = flag;
        o[3] = 0;
    }
}

// logits (T,B,C) fp32 by element strides; table: S rows of C bytes (next state, or 255), accept: S bytes, both on the device;
// line b writes CP_OUT_WORDS words at out + index[b] st_out (an index outside 0 .. n_rows - 1 writes nothing)
TATT_API int tatt_ctc_pattern_mass(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const unsigned char* table,
                                   const unsigned char* accept, int S, const int* index, int* out, int n_rows, long st_out,
                                   hipStream_t st) {
    if (!logits || !table || !accept || !index || !out) return 1;
    if (T <= 0 || T > CP_MAX_T || B <= 0 || C <= 0 || C > CP_MAX_C || S <= 0 || S > CP_MAX_S || n_rows <= 0 || st_out < CP_OUT_WORDS) return 1;
    int rc = 0;
    static TattPerDevice attr_once;                                  // once per device, under the site lock (common.h)
    tatt_per_device(attr_once, [&] {
        rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_pattern_mass_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      CP_LDS_MAX);
    });
    if (rc) return rc;                                               // (beyond 64 KB of LDS the launch depends on it)
    hipLaunchKernelGGL(ctc_pattern_mass_kernel, dim3(B), dim3(64), (size_t)cp_lds_bytes(S, C), st, logits, st_t, st_b, st_c, T, C, table,
                       accept, S, index, out, n_rows, st_out);
    return LAUNCH_CHECK();
}

TATT_API int tatt_pattern_limits(int* out) {
    if (!out) return 1;
    out[0] = CP_MAX_T;
    out[1] = CP_MAX_C;
    out[2] = CP_MAX_S;
    out[3] = CP_BEAM;
    return 0;
}
