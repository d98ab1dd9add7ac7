/*
 * tatt_hip.h -- C ABI of libtatt_hip.so, the MI355X (gfx950) kernels of the TATT super-resolution
 * hot path (TSRN backbone + TP interpreter + STN/TPS sampler, the TBSRN variant, the training-step losses / optimiser and the
 * CRNN text-prior generator in front of the path; forward and backward).
 *
 * Every entry point takes plain DEVICE pointers, sizes/strides and a hipStream_t; none allocates,
 * synchronises or touches host memory, so a call sequence can be captured in a hipGraph.  Return
 * value: 0 on success, otherwise a hipError_t (or 1 for an unsupported shape).  All tensors are fp32.
 * Feature maps are token-major ("NHWC": row = (b,h,w), contiguous channel axis) unless strides say
 * otherwise.  Scratch ("ws"/"part") sizes are stated per function.
 *
 * The reference (mjq11302010044/TATT) is pure PyTorch, so there is no FFI upstream; each function
 * names the torch.nn call site it replaces (file:line in the reference).  The host-side mirror of the
 * reference's nn.Module surface (tatt_amd/tsrn.py, tbsrn.py, crnn.py, train.py) is the only caller.
 *
 * Activation codes: 0 none, 1 relu, 2 mish (x*tanh(softplus(x)), model/tsrn.py:1056-1064), 3 tanh.
 */
#ifndef TATT_HIP_H
#define TATT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

/* ---- GEMM / convolution (v_mfma_f32_32x32x2_f32, exact fp32) --------------------------------------- */

/* C[z] = act(alpha * (A[z] @ B[z] + bias[z])) + beta * C[z],  A(i,r) = A[i*sam + r*sak] for r < K1 (or all r
 * when A2 == NULL), A2[i*sa2m + (r-K1)*sa2k] otherwise; B(r,j) = B[r*sbk + j*sbn]; C[i*scm + j*scn].
 * splitk > 1: ws >= Z*splitk*M*N floats.  rowsum != NULL (Z == 1): rowsum[i] = alpha * sum_r A(i,r) is produced in the same pass
 * (a bias gradient riding along with the weight-gradient GEMM); with split-K ws needs splitk*M more floats.
 * Replaces nn.Linear (model/tsrn.py:170; model/transformer_v2.py:455-457,788-790; model/stn_head.py:50,53),
 * the 1x1 nn.Conv2d of GruBlock (model/tsrn.py:1071), nn.GRU input projections (model/tsrn.py:1072;
 * model/transformer_v2.py:177) and the packed in/out projections of nn.MultiheadAttention
 * (model/transformer_v2.py:453,786), forward and backward. */
int tatt_gemm(const float* A, long sam, long sak, const float* A2, long sa2m, long sa2k, int K1,
              const float* B, long sbk, long sbn, const float* bias, float* C, long scm, long scn,
              int M, int N, int K, int Z, long bsA, long bsA2, long bsB, long bsC, long bsBias,
              float alpha, float beta, int act, int splitk, float* ws, float* rowsum, hipStream_t st);

/* y[pixel*ldy + co] = act(conv(x, w) + bias) + beta*y; stride 1, 'same' padding; x[n*xsn + h*xsh + w*xsw + c*xsc];
 * wpacked = [KH][KW][Cin][Cout] from tatt_repack_conv_weight.  Also computes the data gradient when given
 * dY as x and the mode-1 packed filter.  splitk > 1 (ws >= splitk*Bn*H*W*Cout floats) for small-M / deep-K shapes.
 * Replaces nn.Conv2d (model/tsrn.py:597,612,877,885,1043,623;
 * model/stn_head.py:15). */
int tatt_conv2d_fwd(const float* x, long xsn, long xsh, long xsw, long xsc, const float* wpacked,
                    const float* bias, float* y, long ldy, int Bn, int H, int W, int Cin, int Cout,
                    int KH, int KW, int act, float beta, int splitk, float* ws, hipStream_t st);

/* tatt_conv2d_fwd without bias / activation / beta that leaves the split contraction UNSUMMED: ws receives *splits partial maps
 * [s][pixel][Cout] (*splits <= splitk; 1 = the finished map) for a consumer that adds them while it loads them
 * (tatt_stn_bn_pool_fwd_parts / tatt_stn_bn_pool_bwd_parts: one launch less per link of the STN head's dependent chain,
 * model/stn_head.py:15).  ws >= max(splitk, 1)*Bn*H*W*Cout floats; `splits` is a HOST pointer, written before the call returns. */
int tatt_conv2d_fwd_partials(const float* x, long xsn, long xsh, long xsw, long xsc, const float* wpacked, int Bn, int H,
                             int W, int Cin, int Cout, int KH, int KW, int splitk, float* ws, int* splits, hipStream_t st);

/* dw_oihw[co][ci][kh][kw] = sum_pixels x[pixel+(kh,kw)][ci] * dy[pixel*lddy + co] + beta*dw; ws >= splitk*KH*KW*Cin*Cout floats */
int tatt_conv2d_wgrad(const float* x, long xsn, long xsh, long xsw, long xsc, const float* dy,
                      long lddy, float* dw_oihw, int Bn, int H, int W, int Cin, int Cout, int KH,
                      int KW, float beta, int splitk, float* ws, hipStream_t st);

/* OIHW nn.Conv2d weight -> GEMM operand; mode 0: [KH][KW][Cin][Cout]; mode 1: [KH][KW][Cout][Cin], taps flipped (data gradient);
 * mode 2: [KH][KW][Cout][Cin]; mode 3: [KH][KW][Cin][Cout], taps flipped -- forward / data-gradient filters with the
 * contraction axis contiguous, for tatt_conv3_c64_fwd_t; modes 6 / 7: the same two 3x3 filters (64 contraction channels) in the
 * per-lane register order of tatt_conv3_c64_fwd_ws16 (4 / 5: retired);
 * modes 8 / 9: the Toeplitz-expanded 9x9 filter of tatt_conv9_c64_to_c4_mfma in its MFMA fragment order (out needs 110,592 floats);
 * modes 10 / 11: the split-bf16 (hi / lo) forward / data-gradient operand of tatt_conv3_c64_fwd_sb (3x3, channel counts multiples
 * of 64; Cout*Cin*9 32-bit words of two bf16, one chunk per 64 contraction channels);
 * modes 12 / 13: the Toeplitz filter of modes 8 / 9 as split-bf16 hi / lo operand fragments of tatt_conv9_c64_to_c4_sb (110,592 words) */
int tatt_repack_conv_weight(const float* w_oihw, float* out, int Cout, int Cin, int KH, int KW,
                            int mode, hipStream_t st);
/* number of 32-bit words the packed layout `mode` of a (Cout, Cin, KH, KW) filter occupies = the size of `out` above; -1 for an
 * unknown mode.  Host-only (no launch): the one place the layout sizes are defined. */
int tatt_repack_words(int Cout, int Cin, int KH, int KW, int mode);
/* the same for n filters in one launch (all packed layouts of a model, refreshed once per optimiser step): ws / outs are HOST arrays
 * of n device pointers, dims a host array of n x 5 ints (Cout, Cin, KH, KW, mode) */
int tatt_repack_conv_weight_batch(const float* const* ws, float* const* outs, const int* dims, int n, hipStream_t st);

/* Weight gradients of one GruBlock in one pass over the tokens (split-bf16 MFMA, hi hi + hi lo + lo hi): per-group partials of
 * dW' (192 x K) = dgi^T [x | xb] with the row sums of dgi (= db') and dW_hh (192 x 64) = dgh^T hprev with the row sums of dgh
 * (= db_hh); reference model/tsrn.py:1075-1084 (GruBlock: 1x1 conv composed with nn.GRU's input projection).  dgi, dgh (M, 192),
 * x, xb, hprev (M, 64) contiguous, xb may be null (K = 64, else 128), M % 32 == 0.  G = persistent work-groups = partial slabs,
 * 1 <= G <= min(M / 32, 256): ws1 >= G*192*K + G*192 floats, ws2 >= G*192*64 + G*192; sum them with tatt_splitk_reduce(ws1, dWp, 192, K, G, 0, 0, 0, dbp, 192) and
 * tatt_splitk_reduce(ws2, dWhh, 192, 64, G, 0, 0, 0, dbhh, 192). */
int tatt_gru_wgrad_sb(const float* dgi, const float* dgh, const float* x, const float* xb, const float* hprev,
                      float* ws1, float* ws2, int M, int G, hipStream_t st);

/* C = sum over S partial (M x N) slabs (+ beta*C); remap_cin > 0: row i = tap*remap_cin + ci, col j = co is scattered to
 * the OIHW filter layout dW[co][ci][tap].  vec (may be NULL): additionally vec[i] = sum over S partial vectors of vec_len
 * floats stored behind the S slabs (the bias-gradient partials of tatt_conv3_c64_wgrad_partial) */
int tatt_splitk_reduce(const float* partial, float* C, int M, int N, int S, int remap_cin, int remap_taps,
                       float beta, float* vec, int vec_len, hipStream_t st);
/* on != 0: split-K reductions issued ON STREAM st from now on (tatt_gemm / tatt_conv2d_wgrad with splitk > 1, tatt_splitk_reduce)
 * are only REGISTERED -- their partial slabs must stay allocated -- and are summed by one launch per 36 entries at
 * tatt_reduce_flush(st) or tatt_reduce_defer(0, st): the 70 small reduction launches behind the weight-gradient GEMMs of a training
 * step become 6.  Results are undefined until the flush.  Accumulating reductions (beta != 0) flush and run immediately.
 * This is the ONLY host-side state the library keeps: one registration table per stream, guarded by a mutex -- callers that drive
 * different streams (several trainers, several host threads) do not interact; calls on ONE stream must come from one thread at a
 * time, as for any stream-ordered API. */
int tatt_reduce_defer(int on, hipStream_t st);
int tatt_reduce_flush(hipStream_t st);

/* Specialised 3x3 convolution, Cin/Cout/W multiples of 64, NHWC contiguous: the SRB / block7 / up-sampler convs
 * (model/tsrn.py:877,885,612,1043), forward and data gradient.  y = act(conv + bias + beta*y) -- as for every 3x3 entry below: the
 * activation acts on the sum, so a contraction chunked over calls (beta = 1) takes its activation on the last chunk.  Filter packed [9][Cout][Cin]
 * (repack mode 2; mode 3 for the data gradient); the filter slice of each tap is staged through LDS, both MFMA operands are
 * read with 16-byte LDS loads along the contraction axis.  Used when Cin != 64. */
int tatt_conv3_c64_fwd_t(const float* x, const float* wt, const float* bias, float* y, int B, int H, int W, int Cin,
                         int Cout, int act, float beta, hipStream_t st);
/* weight-stationary 3x3 convolution for 64 input channels in exact fp32 (reference nn.Conv2d(64, Cout, 3, padding=1):
 * model/tsrn.py:877,885,612,1043 and their data gradients): a persistent work-group keeps the filter in registers, wave = 32 pixels
 * x 16 output channels and the whole 9 x 64 contraction on v_mfma_f32_16x16x4_f32; wl = tatt_repack_conv_weight mode 6 (forward)
 * / mode 7 (data gradient of a 64-output-channel convolution) */
int tatt_conv3_c64_fwd_ws16(const float* x, const float* wl, const float* bias, float* y, int B, int H, int W,
                            int Cout, int act, float beta, hipStream_t st);
/* tatt_conv3_c64_fwd_ws16 with BatchNorm folded in on either side (reference model/tsrn.py:877-886: conv -> bn -> mish -> conv -> bn):
 * in_scale / in_shift (64 floats, nullable): input pixels pass through in_act(x * in_scale[c] + in_shift[c]) while the halo is
 * staged (the producer's BatchNorm + activation; zero padding pads the transformed map); stats (nullable; Cout == 64, act none,
 * beta 0): [min(256, B*H*W/64)][2][64] doubles, per-work-group sum and sum of squares of the output per channel = the stage-1
 * partials tatt_bn_stats_finish turns into mean / rstd / running statistics. */
int tatt_conv3_c64_fwd_ws16_bn(const float* x, const float* wl, const float* bias, float* y, int B, int H, int W,
                               int Cout, int act, float beta, const float* in_scale, const float* in_shift, int in_act,
                               double* stats, hipStream_t st);
/* The same 3x3 convolution on the bf16 matrix cores by operand splitting: a = hi + lo (hi = bf16(a), lo = bf16(a - hi)),
 * a*b ~ hi hi + hi lo + lo hi accumulated in fp32 (the dropped lo*lo term is 2^-16 relative; measured effect on the network:
 * profiles/r03_split_bf16_probe.txt).  x holds cin_total >= 64 channels per pixel; the 64-channel slice starting at ci0 is
 * contracted with the matching chunk of a mode-10 / mode-11 (or 14 / 15: tatt_conv3_sb_packing) packed filter (chunk c starts c*Cout*576 words in); wider inputs are
 * chunked by the caller with beta = 1 and act on the last chunk: y = act(conv + bias + beta*y) on every route.  BatchNorm folding
 * arguments as tatt_conv3_c64_fwd_ws16_bn. */
int tatt_conv3_c64_fwd_sb(const float* x, int cin_total, int ci0, const float* wl, const float* bias, float* y, int B, int H,
                          int W, int Cout, int act, float beta, const float* in_scale, const float* in_shift, int in_act,
                          double* stats, hipStream_t st);
/* The data-gradient convolution (64 -> 64 channels, wl = mode-11 packed filter) of a conv -> bn -> act -> conv -> bn chain (reference
 * model/tsrn.py:877-886, backward) with the BatchNorm backward folded in on both sides:
 *   input side (x2 != NULL): the gradient entering is x * in_scale + x2 * in_scale2 + in_shift per channel -- the BatchNorm backward
 *     dy = a du + b y + c of the layer above with (a, b, c) from tatt_bn_bwd_finish, x = du, x2 = that BatchNorm's input y;
 *   output side (ep_x != NULL): y = (convolution) * ep_act'(ep_gamma xhat + ep_beta), xhat = (ep_x - ep_mean) ep_rstd -- the gradient
 *     through the activation that follows the layer below's BatchNorm -- and stats [min(256, B*H*W/64)][2][64] doubles = the
 *     per-work-group sums of y and y * xhat, i.e. the stage-1 partials of THAT BatchNorm's backward (tatt_bn_bwd_finish sums them). */
int tatt_conv3_c64_dgrad_bn_sb(const float* x, const float* x2, const float* in_scale, const float* in_scale2,
                               const float* in_shift, const float* wl, float* y, int B, int H, int W, const float* ep_x,
                               const float* ep_mean, const float* ep_rstd, const float* ep_gamma, const float* ep_beta,
                               int ep_act, double* stats, hipStream_t st);
/* Which kernel the two entries above launch, and the filter packing it wants.  tatt_conv3_sb_generation (test / A-B hook; returns the
 * previous setting, other values only query): 4 (default) = 4 x 16-pixel tiles, four MFMA waves (one per SIMD, each owning 32 output
 * channels over half the contraction, v_mfma_f32_32x32x16_bf16) with four staging waves beside them (round 6); 3 = the same without
 * staging waves (one 512-register wave per SIMD does everything); 1 = the 64-pixel row tiles of rounds 3-5.  Generation 4 takes
 * H % 4 == 0, any W (the last tile column of a ragged map is cut), act none / ReLU, no tanh; generation 3 H % 4 == 0, W % 16 == 0, no
 * output activation; everything else runs generation 1 (W % 64 == 0).  tatt_conv3_sb_packing:
 * the tatt_repack_conv_weight mode of the FORWARD filter for a call with these arguments -- 10 (generation 1) or 14 (generations
 * 3 / 4); the data-gradient packing is that + 1.  tatt_conv3_sb_route: the generation a call with these arguments runs, 0 when none
 * takes it (generation 1 and W % 64 != 0: the entries return 1).  Generations 3 / 4 address the maps with 32-bit offsets: from
 * B*H*W*max(cin_total, Cout)*4 >= 2^31 - 1 bytes on, generation 1 runs. */
int tatt_conv3_sb_generation(int gen);
int tatt_conv3_sb_packing(int B, int H, int W, int cin_total, int Cout, int act, int ep_act);
int tatt_conv3_sb_route(int B, int H, int W, int cin_total, int Cout, int act, int ep_act);
/* weight-gradient partials part[G][9*Cin][Cout] (G persistent work-groups, G <= B*H*W/64) and, if pdb != NULL, bias-gradient
 * partials pdb[G][Cout] (the column sums of dy the kernel streams anyway; nn.Conv2d's bias gradient); finish with
 * tatt_splitk_reduce(part, dw_oihw, 9*Cin, Cout, G, Cin, 9, beta, db, Cout) where pdb = part + G*9*Cin*Cout */
int tatt_conv3_c64_wgrad_partial(const float* x, const float* dy, float* part, float* pdb, int B, int H, int W,
                                 int Cin, int Cout, int G, hipStream_t st);
/* the same partials on the bf16 matrix cores by operand splitting (hi hi + hi lo + lo hi, fp32 accumulation; csrc/conv3w.hip): same
 * arguments, same outputs up to 2^-16 relative per product */
int tatt_conv3_c64_wgrad_partial_sb(const float* x, const float* dy, float* part, float* pdb, int B, int H, int W,
                                    int Cin, int Cout, int G, hipStream_t st);
/* Test / A-B hook: 2 (default) = 4 x 16-pixel tiles, transposing LDS reads, staging waves beside MFMA waves (round 6; H % 4 == 0,
 * any W: the last tile column of a ragged map is cut; G <= B * (H / 4) * ceil(W / 16)), 1 = the 64-pixel row segments of rounds 3-5
 * (also what H % 4 != 0 runs; W % 64 == 0).  Returns the previous setting.  tatt_conv3_wgrad_sb_route: the generation a call of
 * tatt_conv3_c64_wgrad_partial_sb with this geometry runs, 0 when none takes it (the entry returns 1); generation 2 addresses the maps
 * with 32-bit offsets (B*H*W*max(Cin, Cout)*4 < 2^31 - 1 bytes). */
int tatt_conv3_wgrad_sb_generation(int gen);
int tatt_conv3_wgrad_sb_route(int B, int H, int W, int Cin, int Cout);

/* 9x9 convolution 64 -> 4 channels (fp32 vector ALU; filter through the scalar cache): the final reconstruction conv
 * (model/tsrn.py:623) and, with the mode-1 packed filter, the data gradient of block1 (model/tsrn.py:597).
 * x (B,H,W,C) NHWC, C % 16 == 0, H % 8 == 0, W % 32 == 0; wpacked [81][C][4]; y (B,H,W,4) */
int tatt_conv9_c64_to_c4(const float* x, const float* wpacked, const float* bias, float* y, int B, int H, int W,
                         int C, hipStream_t st);
/* the same convolution on v_mfma_f32_16x16x4_f32: tile columns = (4 neighbouring pixels x 4 output channels), Toeplitz-expanded
 * filter wt (110,592 floats) from tatt_repack_conv_weight mode 8 (forward, reference model/tsrn.py:623) / mode 9 (data gradient of
 * block1's 4->64 convolution, :597); x (B,H,W,64) NHWC contiguous, H % 4 == 0, W % 64 == 0; y (B,H,W,4) */
int tatt_conv9_c64_to_c4_mfma(const float* x, const float* wt, const float* bias, float* y, int B, int H, int W,
                              hipStream_t st);
/* the same Toeplitz convolution on v_mfma_f32_16x16x32_bf16 with every fp32 operand split a = hi + lo (hi hi + hi lo + lo hi, fp32
 * accumulation: 2^-16 relative per product, the arithmetic of tatt_conv3_c64_fwd_sb); wt from tatt_repack_conv_weight mode 12
 * (forward, model/tsrn.py:623) / mode 13 (data gradient of block1's 4->64 convolution, :597); geometry as the _mfma entry */
int tatt_conv9_c64_to_c4_sb(const float* x, const float* wt, const float* bias, float* y, int B, int H, int W,
                            hipStream_t st);
/* 9x9 convolution from 4 channels to 64 (weight-stationary MFMA kernel, k = the 4 input channels): y = act(conv(in, wp) + bias),
 * wp [81][4][64] = tatt_repack_conv_weight mode 0 of block1's filter (reference model/tsrn.py:597) or mode 1 of the 64->4
 * reconstruction filter (its data gradient, :623); in (B,H,W,4), out (B,H,W,64) NHWC contiguous, H % 4 == 0, W % 64 == 0 */
int tatt_conv9_c4_to_c64(const float* in, const float* wp, const float* bias, float* out, int B, int H, int W, int act,
                         hipStream_t st);
/* the same convolution on v_mfma_f32_16x16x32_bf16 with split operands (k = 8 taps x 4 input channels; hi hi + hi lo + lo hi, fp32
 * accumulation: 2^-16 relative per product); same arguments and the same fp32 packed filter (the kernel splits it itself) */
int tatt_conv9_c4_to_c64_sb(const float* in, const float* wp, const float* bias, float* out, int B, int H, int W, int act,
                            hipStream_t st);
/* dw (4,64,9,9) = sum_px x[px+tap][ci] * dy[px][co] on v_mfma_f32_16x16x4_f32 (rows = input channels, columns = (tap, output
 * channel) read Toeplitz-fashion from the dy tile; weight gradient of reference model/tsrn.py:623); H % 4 == 0, W % 64 == 0;
 * part >= min(B*(H/4)*(W/64), 256) * 64 * 336 floats */
int tatt_conv9_c64_c4_wgrad(const float* x, const float* dy, float* dw, float* part, int B, int H, int W,
                            hipStream_t st);
/* x (B,H,W,4), dy (B,H,W,64) -> dw (64,4,9,9): the same kernel with the two tensors' roles exchanged (weight gradient of block1's
 * 4->64 convolution, reference model/tsrn.py:597); same constraints and workspace */
int tatt_conv9_c4_c64_wgrad(const float* x, const float* dy, float* dw, float* part, int B, int H, int W,
                            hipStream_t st);
/* the two 9x9 weight gradients above on v_mfma_f32_16x16x32_bf16 with split operands (the contraction runs over pixels: both operands
 * are gathered 8 pixels per lane from the fp32 images and split hi + lo in registers; hi hi + hi lo + lo hi, fp32 accumulation);
 * same arguments, constraints and workspace */
int tatt_conv9_c64_c4_wgrad_sb(const float* x, const float* dy, float* dw, float* part, int B, int H, int W,
                               hipStream_t st);
int tatt_conv9_c4_c64_wgrad_sb(const float* x, const float* dy, float* dw, float* part, int B, int H, int W,
                               hipStream_t st);

/* ---- reductions / normalisation ------------------------------------------------------------------- */

/* out[c] = scale * sum_m X[m*ld + c] + beta*out[c]  (bias gradients); ws >= 256*C doubles */
int tatt_colsum(const float* X, long ld, int M, int C, float* out, float scale, float beta,
                double* ws, hipStream_t st);

/* train-mode nn.BatchNorm statistics over the M rows (model/tsrn.py:878,886,613; model/stn_head.py:19,51):
 * mean, rstd = 1/sqrt(biased var + eps); running stats updated in place (unbiased var, momentum) when non-NULL.
 * ws >= 256*2*C doubles */
int tatt_bn_stats(const float* X, long ld, int M, int C, float eps, float momentum, float* mean,
                  float* rstd, float* running_mean, float* running_var, double* ws, hipStream_t st);
/* stage 2 of tatt_bn_stats alone: part [G][2][C] doubles (per-block sum, sum of squares; e.g. from tatt_conv3_c64_fwd_ws16_bn) ->
 * mean, rstd, running statistics; scale / shift (nullable): gamma * rstd and beta - mean * gamma * rstd, the folded affine map */
int tatt_bn_stats_finish(const double* part, int G, int C, int M, float eps, float momentum, const float* gamma,
                         const float* beta, float* mean, float* rstd, float* running_mean, float* running_var, float* scale,
                         float* shift, hipStream_t st);
/* eval mode: rstd = 1/sqrt(running_var + eps) */
int tatt_bn_rstd(const float* var, float* rstd, int C, float eps, hipStream_t st);
/* Y = act((X - mean) * rstd * gamma + beta) */
int tatt_bn_apply(const float* X, long ldx, float* Y, long ldy, int M, int C, const float* mean,
                  const float* rstd, const float* gamma, const float* beta, int act, hipStream_t st);
/* backward of tatt_bn_apply (+ batch statistics when training): dX, dgamma, dbeta; sums: 2*C floats scratch;
 * ws >= 256*2*C doubles */
int tatt_bn_bwd(const float* X, long ldx, const float* dY, long lddy, float* dX, long lddx, int M, int C,
                const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                int training, float* dgamma, float* dbeta, float* sums, double* ws, hipStream_t st);
/* The same backward in pieces (round 4): stage-1 partials alone (part: tatt_bn_bwd_groups(M) x 2 x C doubles: sums of
 * du = dY act'(gamma xhat + beta) and du xhat) -- or produced by tatt_conv3_c64_dgrad_bn_sb's epilogue; */
int tatt_bn_bwd_groups(int M);
int tatt_bn_bwd_partials(const float* X, long ldx, const float* dY, long lddy, int M, int C, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, int act, double* part, hipStream_t st);
/* ... their sum over G groups -> dgamma, dbeta and coef[3][C] = (a, b, c) of dX = a du + b X + c (= gamma rstd (du - mean(du) -
 * xhat mean(du xhat))), which a consumer applies while staging (tatt_conv3_c64_dgrad_bn_sb) ... */
int tatt_bn_bwd_finish(const double* part, int G, int C, int M, const float* mean, const float* rstd, const float* gamma,
                       float* dgamma, float* dbeta, float* coef, hipStream_t st);
/* ... or this kernel materialises: dX = a dU + b X + c (M, C contiguous, C % 4 == 0) */
int tatt_bn_bwd_affine(const float* X, const float* dU, float* dX, int M, int C, const float* coef, hipStream_t st);

/* Y = LayerNorm(A + Bres) * gamma + beta over the last axis (C <= 256), stats[M][2] = (mean, 1/denominator).
 * mode 0 = nn.LayerNorm (biased variance, eps inside the sqrt); mode 1 = the TBSRN variant's own LayerNorm
 * (model/tbsrn.py:23-36: unbiased std, eps added to the std).
 * nn.LayerNorm + the residual add in front of it (model/transformer_v2.py:478-483,826-832,380-387).
 * pdrop > 0: Bres goes through nn.Dropout(pdrop) first (mask = tatt_dropout's for the same seed word, site and flat index):
 * LayerNorm(A + Dropout(Bres)) in one pass. */
int tatt_ln_fwd(const float* A, const float* Bres, float* Y, float* stats, int M, int C,
                const float* gamma, const float* beta, float eps, int mode, float pdrop,
                const unsigned long long* seed, unsigned site, hipStream_t st);
/* dX = d(A + Dropout(Bres)) (the gradient of A); dB (pdrop > 0 only) = the gradient of Bres = Dropout'(dX);
 * part >= ceil(M/64)*2*C floats; ws >= 256*2*C doubles */
int tatt_ln_bwd(const float* A, const float* Bres, const float* dY, const float* stats, float* dX, float* dB, int M,
                int C, const float* gamma, float* dgamma, float* dbeta, float* part, double* ws, float eps, int mode,
                float pdrop, const unsigned long long* seed, unsigned site, hipStream_t st);

/* ---- element-wise ------------------------------------------------------------------------------------ */

/* nn.PReLU() with one shared slope (model/tsrn.py:598,173) */
int tatt_prelu_fwd(const float* x, float* y, const float* alpha, long n, hipStream_t st);
/* part >= ceil(n/256) floats: per-block partial d alpha (sum with tatt_colsum(part, 1, G, 1, ...)) */
int tatt_prelu_bwd(const float* x, const float* dy, float* dx, const float* alpha, long n, float* part,
                   hipStream_t st);
int tatt_act_fwd(const float* x, float* y, long n, int act, hipStream_t st);
/* dx = dy * act'(.)  -- ref is the pre-activation, or the OUTPUT when from_output (relu/tanh only) */
int tatt_act_bwd(const float* ref, const float* dy, float* dx, long n, int act, int from_output,
                 hipStream_t st);
/* y = alpha*a + beta*b (b may be NULL) */
int tatt_axpby(const float* a, const float* b, float* y, float alpha, float beta, long n, hipStream_t st);
/* y = ((s0 + s1) + s2) + ... : n <= 8 contiguous, 16-byte aligned tensors of numel floats (srcs: HOST array of n device pointers);
 * the gradient of a tensor with several consumers, which autograd sums with a chain of at::add */
int tatt_add_n(const float* const* srcs, int n, float* y, long numel, hipStream_t st);
/* y[m,:] = a[m,:] + b[m % period,:]  (positional embedding broadcast over the batch) */
int tatt_add_rowbcast(const float* a, const float* b, float* y, long rows, int C, long period,
                      hipStream_t st);
/* nn.PixelShuffle(2) + activation on NHWC maps: out[b,2h+i,2w+j,c] = act(in[b,h,w,4c+2i+j]) (model/tsrn.py:1045-1052) */
int tatt_pixel_shuffle_fwd(const float* in, float* out, int B, int H, int W, int C, int act,
                           hipStream_t st);
int tatt_pixel_shuffle_bwd(const float* in, const float* dout, float* din, int B, int H, int W, int C,
                           int act, hipStream_t st);
/* nn.MaxPool2d(kernel (kh,kw), stride (sh,sw), padding (ph,pw)) on NHWC maps (model/stn_head.py:36-44; model/crnn/crnn.py:57-69);
 * out is (B, (H+2ph-kh)/sh+1, (W+2pw-kw)/sw+1, C); the gradient goes to the first maximum of each window */
int tatt_maxpool_fwd(const float* in, float* out, int B, int H, int W, int C, int kh, int kw, int sh, int sw,
                     int ph, int pw, hipStream_t st);
int tatt_maxpool_bwd(const float* in, const float* dout, float* din, int B, int H, int W, int C, int kh,
                     int kw, int sh, int sw, int ph, int pw, hipStream_t st);
/* nn.Dropout(p): y = keep ? x/(1-p) : 0 with a counter-based mask keyed by (*seed, site, index); the same call
 * with dy as x is the backward (model/transformer_v2.py:27,456,461-462,789,795-797) */
int tatt_dropout(const float* x, float* y, long n, float p, const unsigned long long* seed, unsigned site,
                 hipStream_t st);
/* advance the device-resident seed word and (snap != NULL) copy the new value to `snap`: one call per TRAINING FORWARD; every
   dropout site of that forward and of its backward reads the snapshot (graph-replay safe; several forwards may be in flight) */
int tatt_bump_seed(unsigned long long* seed, unsigned long long* snap, hipStream_t st);
/* out[0] = 100 MHz wall clock at this point of the stream (a one-thread launch): timelines inside a replayed hipGraph (tooling) */
int tatt_stamp(unsigned long long* out, hipStream_t st);
/* dst[i0*d0+i1*d1+i2*d2+i3*d3] = src[i0*s0+...] + beta*dst  (layout changes, parameter gathers) */
int tatt_copy4d(const float* src, float* dst, int n0, int n1, int n2, int n3, long s0, long s1, long s2,
                long s3, long d0, long d1, long d2, long d3, float beta, hipStream_t st);

/* ---- optimiser (flat buffers; step-varying scalars live in device memory => hipGraph-replayable) --------- */

/* out[0] = ||g||_2 ; ws >= 1024 doubles  (torch.nn.utils.clip_grad_norm_, interfaces/super_resolution.py:1083-1084) */
int tatt_l2norm(const float* g, long n, float* out, double* ws, hipStream_t st);
/* p -= Adam(g * gscale * min(1, max_norm/(gnorm*gscale + 1e-6))); gnorm: device float; step: device int64, 1-based
 * (torch.optim.Adam(lr, betas=(0.5,0.999)), interfaces/base.py:527, config/super_resolution.yaml:26-29) */
int tatt_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                   float eps, const float* gnorm, float max_norm, float gscale, const long long* step,
                   hipStream_t st);

/* ---- GRU recurrences --------------------------------------------------------------------------------- */

/* Bidirectional GRU recurrence, hidden 32 (nn.GRU(64,32,bidirectional), model/tsrn.py:1072) given the input
 * projection gi[tok][192] = [fwd r,z,n | rev r,z,n]; out[tok][64] = [fwd h | rev h].
 * token(s,t) = (s / s_in)*stride_hi + (s % s_in)*stride_lo + t*stride_t on the NHWC token grid: vertical scan
 * (gru1): s_in=W, stride_hi=H*W, stride_lo=1, stride_t=W, T=H; horizontal (gru2): s_in=1, stride_hi=W, stride_t=1, T=W. */
int tatt_gru32_fwd(const float* gi, const float* whh_f, const float* bhh_f, const float* whh_r,
                   const float* bhh_r, float* out, float* gates, int nseq, int T, int s_in, long stride_hi,
                   long stride_lo, long stride_t, hipStream_t st);
/* gates (may be NULL: inference): [tok][256] = per direction {r, z, n, W_hn h + b_hn} x 32, what autograd keeps of
 * torch.nn.GRU's forward for its backward.
 * BPTT from those: writes dgi[tok][192], dgh[tok][192] (recurrent-side gate gradients) and hprev[tok][64] */
int tatt_gru32_bwd(const float* gates, const float* out, const float* dout, const float* whh_f,
                   const float* whh_r, float* dgi, float* dgh, float* hprev, int nseq, int T, int s_in,
                   long stride_hi, long stride_lo, long stride_t, hipStream_t st);

/* Second generation of the two recurrences above (round 4; same reference lines, same arguments, same results up to the order of
 * fp32 summation): one WAVE per (sequence, direction), two lanes per hidden unit, halves joined by v_permlane32_swap. */
int tatt_gru32_fwd2(const float* gi, const float* whh_f, const float* bhh_f, const float* whh_r,
                    const float* bhh_r, float* out, float* gates, int nseq, int T, int s_in, long stride_hi,
                    long stride_lo, long stride_t, hipStream_t st);
/* frag == NULL: dgi, dgh, hprev as tatt_gru32_bwd.  frag != NULL (T % 8 == 0 and nseq * T / 8 % 4 == 0, else returns 1): dgi as
 * before; instead of dgh / hprev (unused, may be NULL) the operands of the weight-gradient pass in bf16 hi / lo MFMA fragment
 * order, nseq * T / 32 K-steps of 10240 floats: [K-step][slot 0..19][hi, lo][lane][4 dwords], slots d*8 + {r0 r1 z0 z1 n0 n1 gn0
 * gn1}, 16 + d*2 + {0, 1} = h_{t-1}; consumed by tatt_gru_wgrad_frag */
int tatt_gru32_bwd2(const float* gates, const float* out, const float* dout, const float* whh_f,
                    const float* whh_r, float* dgi, float* dgh, float* hprev, float* frag, int nseq, int T, int s_in,
                    long stride_hi, long stride_lo, long stride_t, hipStream_t st);
/* Weight gradients of one GruBlock (as tatt_gru_wgrad_sb; reference model/tsrn.py:1075-1084) from that fragment stream and the
 * token-major inputs x (M, 64) | xb (M, 64 or NULL) under the same sequence geometry.  1 <= G <= min(nseq * T / 32, 256);
 * ws1 >= G*192*K + G*192 floats (K = 128 with xb, else 64), ws2 >= G*192*32 + G*192; finish with
 * tatt_splitk_reduce(ws1, dWp, 192, K, G, 0, 0, 0, dbp, 192) and tatt_splitk_reduce(ws2, dWhh_c, 192, 32, G, 0, 0, 0, dbhh, 192)
 * where dWhh_c (192, 32) = [dW_hh forward; dW_hh reverse] */
int tatt_gru_wgrad_frag(const float* frag, const float* x, const float* xb, float* ws1, float* ws2, int nseq, int T,
                        int s_in, long stride_hi, long stride_lo, long stride_t, int G, hipStream_t st);
/* The same for a block whose forward projection read x through tatt_tokgemm_sb_in: x is transformed while it is staged, bit for bit as
 * there.  Exactly one of: in_mean, in_rstd, in_gamma, in_beta (64 floats each; x becomes (x - mean) * rstd * gamma + beta, rounded as
 * tatt_bn_apply), or in_add (M, 64) contiguous and 16-byte aligned (x becomes x + in_add; without xb only); the others NULL, else
 * returns 1.  xb and the fragment stream are read as they are. */
int tatt_gru_wgrad_frag_in(const float* frag, const float* x, const float* xb, float* ws1, float* ws2, int nseq, int T,
                           int s_in, long stride_hi, long stride_lo, long stride_t, int G, const float* in_mean,
                           const float* in_rstd, const float* in_gamma, const float* in_beta, const float* in_add,
                           hipStream_t st);

/* backward step, fused form: dh = dhseq_next + dhcarry + dgh_cur @ whh, then the gate part of the NEXT step on the same tile:
 * dgi_acc += input-side gate grads, dgh_next = recurrent-side gate grads, dhcarry = dh*z  (whhT = whh transposed) */
int tatt_qgru_bwd_fused(const float* dgh_cur0, const float* dgh_cur1, const float* whhT0, const float* whhT1,
                        const float* dhseq_next0, const float* dhseq_next1, const float* gsave_next0,
                        const float* gsave_next1, const float* hprev_next0, const float* hprev_next1,
                        float* dhcarry0, float* dhcarry1, float* dgi_acc0, float* dgi_acc1, float* dgh_next0,
                        float* dgh_next1, int Wb, int HID, hipStream_t st);

/* GruBlock glue: compose the 1x1 conv (Wc (64,K), bc) with the GRU input projections into Wp (192,K) = [wih_f; wih_r] Wc,
 * bp (192) = [wih_f; wih_r] bc + [bih_f; bih_r]  (reference GruBlock.forward, model/tsrn.py:1075-1081) */
int tatt_gru_compose(const float* wih_f, const float* wih_r, const float* bih_f, const float* bih_r,
                     const float* Wc, const float* bc, float* Wp, float* bp, int K, hipStream_t st);
/* tatt_gru_compose for n GruBlocks in one launch (a generator composes all of its blocks once per forward): ptrs = HOST array of
 * n x 8 device pointers (wih_f, wih_r, bih_f, bih_r, Wc, bc, Wp, bp), Ks = HOST array of the n conv input widths */
int tatt_gru_compose_batch(const float* const* ptrs, const int* Ks, int n, hipStream_t st);
/* ... and map the gradients of the composed projection back: dwih_d (96,64) = dWp_d Wc^T + dbp_d bc^T,
 * dWc (64,K) = sum_d wih_d^T dWp_d, dbc (64) = sum_d wih_d^T dbp_d; dwhh_d (96,32) = d-th diagonal block of dWhh (192,64) */
int tatt_gru_tail(const float* dWp, const float* dbp, const float* Wc, const float* bc, const float* wih_f,
                  const float* wih_r, float* dwih_f, float* dwih_r, float* dWc, float* dbc, int K,
                  const float* dWhh, float* dwhh_f, float* dwhh_r, hipStream_t st);

/* tatt_gru_tail with dWhh given compact: dWhh_c (192, 32) = [dW_hh forward; dW_hh reverse] (tatt_gru_wgrad_frag) */
int tatt_gru_tail_c(const float* dWp, const float* dbp, const float* Wc, const float* bc, const float* wih_f,
                    const float* wih_r, float* dwih_f, float* dwih_r, float* dWc, float* dbc, int K,
                    const float* dWhh_c, float* dwhh_f, float* dwhh_r, hipStream_t st);

/* One time step of the query-embedding GRU (nn.GRU(64*H, 32*H, bidirectional), model/transformer_v2.py:177,218;
 * time axis = sample axis), both directions: gi* (Wb,3*HID) incl. b_ih, whh* (3*HID,HID),
 * hprev* (Wb,HID) or NULL for h=0, hnew* (Wb,HID), gsave* (4,Wb,HID) = r,z,n,(W_hn h+b_hn) or NULL. */
int tatt_qgru_fwd_step(const float* gi0, const float* gi1, const float* whh0, const float* whh1,
                       const float* bhh0, const float* bhh1, const float* hprev0, const float* hprev1,
                       float* hnew0, float* hnew1, float* gsave0, float* gsave1, int Wb, int HID,
                       hipStream_t st);
/* backward step, gate part: dh = dhseq + dhcarry (dhcarry ignored when first); dgi_acc (+)= input-side gate grads;
 * dgh = recurrent-side gate grads; dhcarry = dh*z */
int tatt_qgru_bwd_gates(const float* dhseq0, const float* dhseq1, const float* gsave0, const float* gsave1,
                        const float* hprev0, const float* hprev1, float* dhcarry0, float* dhcarry1,
                        float* dgi_acc0, float* dgi_acc1, float* dgh0, float* dgh1, int Wb, int HID, int first,
                        hipStream_t st);
/* backward step, matmul part: dhcarry (Wb,HID) += dgh (Wb,3*HID) @ whh (3*HID,HID); whhT* = whh transposed (HID,3*HID) */
int tatt_qgru_bwd_mm(const float* dgh0, const float* dgh1, const float* whhT0, const float* whhT1,
                     float* dhcarry0, float* dhcarry1, int Wb, int HID, hipStream_t st);

/* The backward recurrence above as ONE persistent launch: fused steps s0 .. s1-1 of the T-1 (step s = tatt_qgru_bwd_fused with the
 * forward direction at time T-1-s and the reverse direction at time s; model/transformer_v2.py:201-221 backward).  A work-group keeps
 * its tile's W_hh^T slice, dhcarry and dgi accumulators in registers; dgh crosses work-groups per step through write-through (sc1)
 * stores and per-(row block, direction) flag words -- no grid-wide barrier.  dgh* (T, Wb, 3*HID): slot T-1 (dir 0) / 0 (dir 1) filled
 * by tatt_qgru_bwd_gates(first = 1), which also initialises dhcarry* and dgi_acc*; hbuf0 + t*Wb*HID = h_prev of time t (dir 0),
 * hbuf1 + (t+1)*Wb*HID = h_prev of time t (dir 1); gsave* (T, 4, Wb, HID); dhseq* (T, Wb, HID).  sync: 1024 words (zeroed here when
 * s0 == 0); sync[1023] != 0 afterwards: a wall-clock-bounded spin expired (results invalid).  Returns 1 for geometries it does not
 * take (HID != 512, Wb % 16 != 0, more than 256 work-groups): use the per-step entry points then.  whhT*: W_hh^T (HID, 3*HID) with
 * transposed != 0, W_hh itself (3*HID, HID) with 0 (no transposition launch needed: the slices are read once per launch).
 * xch* non-NULL (workspace of T*Wb*3*HID floats per direction): the recurrent product runs on the bf16 matrix cores with split operands
 * (hi hi + hi lo + lo hi, fp32 accumulation) and the exchanged tensor travels in operand form; NULL: exact fp32 products. */
int tatt_qgru_bwd_chain(float* dgh0, float* dgh1, const float* whhT0, const float* whhT1, const float* dhseq0,
                        const float* dhseq1, const float* gsave0, const float* gsave1, const float* hbuf0,
                        const float* hbuf1, float* dhcarry0, float* dhcarry1, float* dgi_acc0, float* dgi_acc1,
                        unsigned* sync, int T, int Wb, int HID, int s0, int s1, int transposed, float* xch0, float* xch1,
                        hipStream_t st);

/* Recurrent weight gradient of the query GRU after the backward recurrence (the gradient nn.GRU's autograd accumulates over the time
 * steps, model/transformer_v2.py:201-221 backward): for both directions d in one launch dW_d (N x K) = A_d^T B_d and db_d (N) = column
 * sums of A_d, with A_d = dgh of direction d (M = T*Wb tokens, N = 3*HID) and B_d = h_prev of the same tokens (M, K = HID), contiguous;
 * split-bf16 products (hi hi + hi lo + lo hi, fp32 accumulation) on the bf16 matrix cores.  M % 32 == 0, N % 128 == 0, K % 128 == 0;
 * the contraction is split S ways (1 <= S <= M / 32); ws_d >= S*N*K + S*N floats.  Leaves the per-split partials: finish each
 * direction with tatt_splitk_reduce(ws_d, dW_d, N, K, S, 0, 0, 0, db_d, N).  Returns 1 / 2 for geometries it does not take. */
int tatt_qgru_wgrad_sb(const float* A0, const float* A1, const float* B0, const float* B1, float* ws0, float* ws1, int M, int N,
                       int K, int S, hipStream_t st);

/* The forward recurrence (T calls of tatt_qgru_fwd_step) as one persistent launch, time steps s0 .. s1-1 (direction 0 at time s,
 * direction 1 at time T-1-s), same hand-off as tatt_qgru_bwd_chain with h as the exchanged tensor.  hbuf* (T+1, Wb, HID): h of time t
 * at slot t+1 (direction 0; slot 0 zero) / slot t (direction 1; slot T zero), zero slots filled by the caller; gsave* (T, 4, Wb, HID)
 * or NULL; gi* (Wb, 3*HID) incl. b_ih, or NULL: the launch computes the projection itself from x (Wb, IN), wih* (3*HID, IN), bih*
 * (IN % 1024 == 0); q (T, 2*HID/C, Wb, C) or NULL: h also in the (sample, H, W, C) layout of the query embedding.
 * xch* non-NULL (workspace of (T+1)*Wb*HID floats per direction, s0 == 0): split-bf16 form as for tatt_qgru_bwd_chain.
 * model/transformer_v2.py:201-221. */
int tatt_qgru_fwd_chain(const float* gi0, const float* gi1, const float* whh0, const float* whh1, const float* bhh0,
                        const float* bhh1, float* hbuf0, float* hbuf1, float* gsave0, float* gsave1, unsigned* sync,
                        int T, int Wb, int HID, int s0, int s1, const float* x, const float* wih0, const float* wih1,
                        const float* bih0, const float* bih1, int IN, float* q, int C, float* xch0, float* xch1, hipStream_t st);

/* ---- STN head glue (model/stn_head.py:25-106): everything between two of its convolutions as ONE launch ------------------------
 * The launches below synchronise their (<= 128) work-groups INSIDE the launch: partial sums leave through write-through stores, each
 * work-group raises a flag word and waits for the others'.  `sync` is a 256-word buffer per call site, zeroed ONCE by the caller when
 * it is allocated and then reused (word 254 = epoch, word 255 = error: a wall-clock-bounded spin expired, results invalid); launches
 * that share a sync buffer must not overlap. */

/* A (B,H/ph,W/pw,C) = maxpool_{ph x pw}(relu(batchnorm_train(X))), X (B,H,W,C) contiguous; mean, rstd (C) out; running statistics
 * updated (NULL: not); part >= 128*2*C doubles.  nn.BatchNorm2d + nn.ReLU + nn.MaxPool2d of stn_head.py:9-15,33-49.  ph, pw in {1,2},
 * C in {32, 64, 128, 256} and at most 128 * 4 * 1024 / C pool windows, else 1. */
int tatt_stn_bn_pool_fwd(const float* X, float* A, const float* gamma, const float* beta, float* mean, float* rstd,
                         float* running_mean, float* running_var, double* part, unsigned* sync, int B, int H, int W, int C,
                         int ph, int pw, float eps, float momentum, hipStream_t st);
/* the same with the producing convolution's split contraction folded in: Xparts = S partial maps (S,B,H,W,C) as
 * tatt_conv2d_fwd_partials leaves them; X = their sum in slab order + bias (NULL: none; tatt_splitk_reduce adds the same terms four-way
 * interleaved: last-bit differences) is written to Xout (the backward reads it) and normalised + pooled into A */
int tatt_stn_bn_pool_fwd_parts(const float* Xparts, int S, const float* bias, float* Xout, float* A, const float* gamma,
                               const float* beta, float* mean, float* rstd, float* running_mean, float* running_var,
                               double* part, unsigned* sync, int B, int H, int W, int C, int ph, int pw, float eps,
                               float momentum, hipStream_t st);
/* its backward: dA -> dX (gradient w.r.t. X), dgamma, dbeta, dbias = column sums of dX (the producing convolution's bias gradient;
 * NULL: skipped).  The pooled gradient goes to the first maximum of its window (tatt_maxpool_bwd's rule).  part >= 128*3*C doubles. */
int tatt_stn_bn_pool_bwd(const float* X, const float* dA, const float* gamma, const float* beta, const float* mean,
                         const float* rstd, float* dX, float* dgamma, float* dbeta, float* dbias, double* part,
                         unsigned* sync, int B, int H, int W, int C, int ph, int pw, hipStream_t st);
/* tatt_stn_bn_pool_bwd with dA given as S partial maps (S,B,H/ph,W/pw,C) of the data-gradient convolution behind it (summed in
 * slab order while they are loaded; S = 1: the map itself) */
int tatt_stn_bn_pool_bwd_parts(const float* X, const float* dAparts, int S, const float* gamma, const float* beta,
                               const float* mean, const float* rstd, float* dX, float* dgamma, float* dbeta, float* dbias,
                               double* part, unsigned* sync, int B, int H, int W, int C, int ph, int pw, hipStream_t st);
/* x.view(B,-1) of the (B,256,1,2) map [given NHWC: A6 (B,2,256)] -> Linear(512,512) -> BatchNorm1d(train) -> ReLU -> x0.1 ->
 * Linear(512,NO): U (B,512) = first Linear's output, S (B,512) = the second Linear's input, ctrl (B,NO); W1 (512,512), W2 (NO,512)
 * row-major [out][in]; part >= 32*B*NO floats.  stn_head.py:51-58,96-106.  B <= 64, NO % 4 == 0, NO <= 64, else 1. */
int tatt_stn_fc_fwd(const float* A6, const float* W1, const float* b1, const float* g1, const float* be1, float* rm1,
                    float* rv1, const float* W2, const float* b2, float* U, float* mean1, float* rstd1, float* S,
                    float* ctrl, float* part, unsigned* sync, int B, int NO, float eps, float momentum, hipStream_t st);
/* its backward incl. every parameter gradient: dW2 (NO,512), db2, dgamma1, dbeta1, dW1 (512,512), db1, dA6 (B,2,256); dU (B,512)
 * is workspace (the tensor the work-groups exchange). */
int tatt_stn_fc_bwd(const float* dctrl, const float* W2, const float* S, const float* U, const float* mean1,
                    const float* rstd1, const float* g1, const float* W1, const float* A6, float* dW2, float* db2,
                    float* dg1, float* dbe1, float* dW1, float* db1, float* dU, float* dA6, unsigned* sync, int B, int NO,
                    hipStream_t st);

/* ---- attention core ------------------------------------------------------------------------------------ */

/* ctx = dropout(softmax(Q K^T)) V per head (E=64, 4 heads, S <= 32), wavg = head-mean of the dropped
 * probabilities (may be NULL).  Q (B,Lq,64) already projected and scaled; K,V (B,S,64).
 * Core of nn.MultiheadAttention (model/transformer_v2.py:472-474,821-824). */
int tatt_attn_fwd(const float* Q, const float* K, const float* V, float* ctx, float* wavg, int B, int Lq,
                  int S, float pdrop, const unsigned long long* seed, unsigned site, hipStream_t st);
/* part >= B*ceil(Lq/64)*2*S*64 floats; dwavg may be NULL */
int tatt_attn_bwd(const float* Q, const float* K, const float* V, const float* dctx, const float* dwavg,
                  float* dQ, float* dK, float* dV, float* part, int B, int Lq, int S, float pdrop,
                  const unsigned long long* seed, unsigned site, hipStream_t st);

/* Row softmax over materialised attention scores (TBSRN FeatureEnhancer self-attention, model/tbsrn.py:130-151):
 * S (rows x L, L <= 4096) is overwritten by softmax(S); Pd (nullable) receives dropout(softmax(S)) */
int tatt_softmax_rows_fwd(float* S, float* Pd, long rows, int L, float pdrop, const unsigned long long* seed,
                          unsigned site, hipStream_t st);
/* dP (gradient w.r.t. the dropped probabilities) is overwritten by the gradient w.r.t. the scores */
int tatt_softmax_rows_bwd(const float* P, float* dP, long rows, int L, float pdrop, const unsigned long long* seed,
                          unsigned site, hipStream_t st);

/* ---- token-matrix projections on the bf16 matrix cores (csrc/tokgemm.hip) ------------------------------------------ */

/* Y (M x N) = [X1 | X2] (M x K) W^T + bias by operand splitting (hi + lo bf16, three products, fp32 accumulation; same arithmetic as
 * tatt_conv3_c64_fwd_sb): the GRU input projections of the GruBlocks (reference model/tsrn.py:1075-1084) and their data gradients.
 * Wp = packed operand from tatt_tokgemm_pack (N*K 32-bit words); X1 (M, K1), X2 (M, K - K1) (NULL when K1 == K); output columns
 * [0, N1) go to Y1 (M, N1), the rest to Y2 (M, N - N1) (NULL when N1 == N).  M a multiple of 64; (N, K) one of (192, 128), (192, 64),
 * (128, 192), (64, 192), (64, 64), (64, 128). */
int tatt_tokgemm_sb(const float* X1, const float* X2, int K1, const float* Wp, const float* bias, float* Y1, float* Y2, int N1,
                    int M, int N, int K, hipStream_t st);
/* The forward projection of a GruBlock that follows a BatchNorm or a residual sum, without that map in memory: columns [0, K1) of
 * every token row are transformed in registers before the hi / lo split.  Exactly one of: in_mean, in_rstd, in_gamma, in_beta (64
 * floats each; the columns become (x - mean) * rstd * gamma + beta, rounded as tatt_bn_apply rounds it), or in_add (M, K1) contiguous
 * and 16-byte aligned (the columns become X1 + in_add; K = K1 only); the others NULL, else returns 1.  K1 = 64, N = 192, K = 64 or 128;
 * the columns from X2 pass unchanged; the result equals tatt_tokgemm_sb on the materialised map bit for bit. */
int tatt_tokgemm_sb_in(const float* X1, const float* X2, int K1, const float* Wp, const float* bias, float* Y1, float* Y2, int N1,
                       int M, int N, int K, const float* in_mean, const float* in_rstd, const float* in_gamma,
                       const float* in_beta, const float* in_add, hipStream_t st);
/* The same with an epilogue: act = 1 (ReLU) after the bias; accum != 0: Y += instead of Y = (sums of data gradients into one map).
 * Also takes (N, K) = (128, 128) and (128, 64): the TBSRN FeatureEnhancer projections (reference model/tbsrn.py:77-151). */
int tatt_tokgemm_sb_ex(const float* X1, const float* X2, int K1, const float* Wp, const float* bias, float* Y1, float* Y2, int N1,
                       int M, int N, int K, int act, int accum, hipStream_t st);
/* The epilogues of a position-wise feed-forward w_2(Dropout(relu(w_1 x))) (reference PositionwiseFeedForward, model/tbsrn.py:154-164):
 * Y = Dropout_pdrop(act(X Wp^T + bias)) with the mask tatt_dropout draws for Y's flat index (forward of w_1), or, with `gate`,
 * Y = (X Wp^T) * gate_scale where gate > 0, else 0 (data gradient of w_2 gated by the saved forward output F: F > 0 exactly where the
 * unit was active and kept, gate_scale = 1 / (1 - pdrop)).  One source, one destination; shapes of tatt_tokgemm_sb_ex, and with
 * pdrop > 0 or a gate only those tatt_tokgemm_sb_ffn_takes(N, K) answers 1 for (the others return 1). */
int tatt_tokgemm_sb_ffn(const float* X, const float* Wp, const float* bias, float* Y, int M, int N, int K, int act, float pdrop,
                        const unsigned long long* seed, unsigned site, const float* gate, float gate_scale, hipStream_t st);
int tatt_tokgemm_sb_ffn_takes(int N, int K);
/* Y = X Wp^T + bias + addend: addend (M, N) contiguous and left intact, Y must not alias it; (N, K) within 128 x 128.  The sum of a
 * data gradient and the gradient a residual connection carries (TBSRN FeatureEnhancer sub-layers) without an element-wise launch. */
int tatt_tokgemm_sb_add(const float* X, const float* Wp, const float* bias, const float* addend, float* Y, int M, int N, int K,
                        hipStream_t st);
/* trans = 0: w(n, k) = W[n*ldw + k] (y = x W^T);  trans = 1: w(n, k) = W[k*ldw + n] (dx = dy W).  out: N*K words */
int tatt_tokgemm_pack(const float* W, float* out, int N, int K, int ldw, int trans, hipStream_t st);
/* n packs in one launch: ptrs = HOST array of n x 2 device pointers (W, out), dims = HOST array of n x 4 ints (N, K, ldw, trans) */
int tatt_tokgemm_pack_batch(const float* const* ptrs, const int* dims, int n, hipStream_t st);

/* Weight gradient of a token projection y = x W^T + b on the bf16 matrix cores with split operands (csrc/tokwgrad.hip): per-split
 * partials of dW (N x K) = A^T B and db (N) = column sums of A for A = dY (M, N), B = X (M, K) contiguous, M % 32 == 0, N, K in
 * {64, 128}, 1 <= S <= M / 32 (every split owns at least one 32-token chunk); ws >= S*N*K + S*N floats.  Finish with
 * tatt_splitk_reduce(ws, dW, N, K, S, 0, 0, 0, db, N).  The nn.Linear weight gradients of the TBSRN FeatureEnhancer (reference
 * model/tbsrn.py:77-164). */
int tatt_tok_wgrad_sb(const float* A, const float* B, float* ws, int M, int N, int K, int S, hipStream_t st);

/* ---- score-free self-attention of the TBSRN FeatureEnhancer (csrc/sattn.hip) ---------------------------------- */

/* O (B,P,E) = dropout_{pdrop}(softmax(Q K^T * scale)) V per head of 32 channels (E = 32 h, P a multiple of 64): reference
 * `attention` / MultiHeadedAttention (model/tbsrn.py:96-151) without materialising the (B,h,P,P) scores; lse (B,h,P) receives the
 * log-sum-exp of the scaled scores per query (the only thing the backward needs besides Q, K, V, O).  Dropout masks = those of
 * tatt_softmax_rows_fwd for the same seed word and site (flat index ((b h + head) P + q) P + key). */
int tatt_sattn_fwd(const float* Q, const float* K, const float* V, float* O, float* lse, int B, int P, int h, float scale,
                   float pdrop, const unsigned long long* seed, unsigned site, hipStream_t st);
/* gradients of the same (probabilities recomputed tile by tile, no atomics: deterministic); Dws: workspace of B*h*P floats */
int tatt_sattn_bwd(const float* Q, const float* K, const float* V, const float* O, const float* lse, const float* dO,
                   float* dQ, float* dK, float* dV, float* Dws, int B, int P, int h, float scale, float pdrop,
                   const unsigned long long* seed, unsigned site, hipStream_t st);
/* The same pair with the dropout keep decisions handed from the forward to the backward as bits instead of being recomputed in all three
 * kernels (the counter hash is 19 of the ~30 VALU issue slots a score costs): `bits` = B h P P / 32 words the forward fills (layout:
 * csrc/sattn2.hip) and the backward of the same call reads; null = recompute (= the entries above).  Only the split-bf16 kernels use
 * them; whatever runs, a backward must be given what its forward was given.  Same masks, same results as the entries above. */
int tatt_sattn_fwd_bits(const float* Q, const float* K, const float* V, float* O, float* lse, unsigned* bits, int B, int P, int h,
                        float scale, float pdrop, const unsigned long long* seed, unsigned site, hipStream_t st);
int tatt_sattn_bwd_bits(const float* Q, const float* K, const float* V, const float* O, const float* lse, const float* dO,
                        const unsigned* bits, float* dQ, float* dK, float* dV, float* Dws, int B, int P, int h, float scale,
                        float pdrop, const unsigned long long* seed, unsigned site, hipStream_t st);
/* Test / A-B hook: 2 (default) = the split-bf16 kernels (csrc/sattn2.hip: three v_mfma_f32_32x32x16_bf16 products of hi / lo halves per
 * fp32 product; P % 128 == 0, B h P^2 < 4e9), 1 = the exact-fp32 MFMA kernels (also what other geometries run).  Returns the previous
 * setting.  tatt_sattn2_takes: 1 when the split-bf16 kernels run this geometry under the current setting -- the only case in which
 * tatt_sattn_fwd_bits fills `bits`. */
int tatt_sattn_generation(int gen);
int tatt_sattn2_takes(int B, int P, int h);

/* ---- one TP-interpreter transformer layer as ONE kernel (csrc/tplayer.hip) --------------------------------- */

/* Reference TransformerDecoderLayer_TP.forward_post (model/transformer_v2.py:806-833: cross-attention over the S <= 32 projected
 * keys / values of the text prior -> +residual -> LayerNorm -> FFN -> +residual -> LayerNorm; the self-attention is commented
 * out upstream) and TransformerEncoderLayer.forward_post (:470-484), E = 64, 4 heads, dim_ff = 64:
 *   q    = ((x + qpos) in_w[0:64]^T + in_b[0:64]) / 4          qpos: (B,L,64) [qbs = L*64] or (L,64) broadcast [qbs = 0]
 *   ctx  = dropout_{p_attn}(softmax(q K^T)) V per head,        wavg (B,L,S; nullable) = head mean of the dropped probabilities
 *   x1   = LN_A(x + dropout_{p_res}(ctx out_w^T + out_b))
 *   xout = LN_B(x1 + dropout_{p_res}(w2 dropout_{p_ffn}(relu(w1 x1 + b1)) + b2))                        (nullable)
 *   fin  = fin_scale * (LN_F(x) [if fin_both] + LN_F(xout))   when lnF_w != NULL: the stacked final norms of
 *          TransformerDecoder.forward (:380-390) averaged as TPInterpreter does (model/tsrn.py:218)       (nullable)
 * K, V: (B,S,64) = the key / value rows of the packed in-projection applied beforehand.  Dropout sites site0 .. site0+3 draw the
 * masks of tatt_attn_fwd / tatt_ln_fwd / tatt_dropout / tatt_ln_fwd for the same seed word and flat element index. */
int tatt_tplayer_fwd(const float* x, const float* qpos, long qbs, const float* K, const float* V, const float* in_w,
                     const float* in_b, const float* out_w, const float* out_b, const float* w1, const float* b1,
                     const float* w2, const float* b2, const float* lnA_w, const float* lnA_b, const float* lnB_w,
                     const float* lnB_b, const float* lnF_w, const float* lnF_b, float fin_scale, int fin_both, float* xout,
                     float* fin, float* wavg, int B, int L, int S, float p_attn, float p_res, float p_ffn,
                     const unsigned long long* seed, unsigned site0, float eps, hipStream_t st);
/* Backward of the layer, recomputed from x (the forward saves nothing else): upstream gradients dxout (of xout), dfin (of fin;
 * required when lnF_w != NULL), dwavg (of wavg) -- each nullable; dqacc (nullable) is added to dqpos (the next layer's dqpos).
 * Writes dx (B,L,64), dqpos (B,L,64; nullable), and partial records: kvpart (dK / dV per work-group and sample) and ppart
 * (parameter gradients per work-group) -- sizes from tatt_tplayer_geom -- to be summed by the two reducers. */
int tatt_tplayer_bwd(const float* x, const float* qpos, long qbs, const float* K, const float* V, const float* in_w,
                     const float* in_b, const float* out_w, const float* out_b, const float* w1, const float* b1,
                     const float* w2, const float* b2, const float* lnA_w, const float* lnA_b, const float* lnB_w,
                     const float* lnB_b, const float* lnF_w, const float* lnF_b, float fin_scale, int fin_both,
                     const float* dxout, const float* dfin, const float* dwavg, const float* dqacc, float* dx,
                     float* dqpos, float* kvpart, float* ppart, int B, int L, int S, float p_attn, float p_res,
                     float p_ffn, const unsigned long long* seed, unsigned site0, float eps, hipStream_t st);
/* host-side: out[0] = work-groups, out[1] = dK/dV records per work-group, out[2] = floats of kvpart, out[3] = floats of ppart */
int tatt_tplayer_geom(int B, int L, int* out);
/* dK, dV (B,S,64) = sums of the kvpart records */
int tatt_tplayer_reduce_kv(const float* kvpart, float* dK, float* dV, int B, int L, int S, hipStream_t st);
/* parameter gradients = sums of the ppart records: d_in_w receives 64x64 (the query rows of the packed in-projection), d_in_b 64;
 * any destination may be NULL; betaF = 1 accumulates into d_lnF_w / d_lnF_b */
int tatt_tplayer_reduce_params(const float* ppart, int B, int L, float* d_in_w, float* d_in_b, float* d_out_w, float* d_out_b,
                               float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_lnA_w, float* d_lnA_b,
                               float* d_lnB_w, float* d_lnB_b, float* d_lnF_w, float* d_lnF_b, float betaF, hipStream_t st);

/* the same reduction over G records (the second-generation backward below has its own work-group count) */
int tatt_tplayer_reduce_params_g(const float* ppart, int G, float* d_in_w, float* d_in_b, float* d_out_w, float* d_out_b,
                                 float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_lnA_w, float* d_lnA_b,
                                 float* d_lnB_w, float* d_lnB_b, float* d_lnF_w, float* d_lnF_b, float betaF, hipStream_t st);

/* ---- second-generation backward of the layer (csrc/tplayer2.hip): split-bf16 products on the bf16 matrix cores, a wave owns 16
 * tokens and chains every product in registers (transposed MFMA orientation), weight gradients shared by the four waves of a
 * work-group.  Same inputs, outputs and dropout masks as tatt_tplayer_bwd; takes L % 64 == 0, S <= 32 (tatt_tplayer2_geom says). */
/* host-side: out[0] = 1 if the geometry is taken, out[1] = work-groups, out[2] = floats of kvpart, out[3] = floats of ppart,
 * out[4] = ints of kvflags, out[5] = 32-bit words of wimg, out[6] = 32-bit words of kvf, out[7] = floats of wimg32, out[8] = floats of
 * kvf32 */
int tatt_tplayer2_geom(int B, int L, int S, int* out);
/* packed operands of one layer, one launch: wimg = the four 64x64 matrices (in_w: query rows of the packed in-projection) as MFMA A
 * fragments, forward and transposed, bf16 hi / lo, and kvf = K, V (B,S,64) as the four fragment forms of the attention products (the
 * backward's split-bf16 operands); wimg32 / kvf32 = the forward's exact-fp32 operands (one float per lane and v_mfma_f32_16x16x4_f32 step) */
int tatt_tplayer2_prep(const float* in_w, const float* out_w, const float* w1, const float* w2, const float* K, const float* V,
                       unsigned* wimg, unsigned* kvf, float* wimg32, float* kvf32, int B, int S, hipStream_t st);
/* the same packing with the key / value projections folded in, ONE launch for nl = 1 or 2 layers over one memory: K = (mem + pos) Wk^T + bk and
 * V = mem Wv^T + bv (Wk / Wv = rows 64..127 / 128..191 of the layer's packed in-projection) are computed per (layer, sample) in fp32 and leave
 * only as the fragment forms above; kin (B,S,64; nullable) receives mem + pos (the backward's weight gradients read it).  pos: (B,S,64) with
 * pos_bs = S*64, or (S,64) with pos_bs = 0.  in_w ... kvf32 are HOST arrays of nl device pointers. */
int tatt_tplayer2_kvprep(const float* mem, const float* pos, long pos_bs, const float* const* in_w, const float* const* in_b,
                         const float* const* out_w, const float* const* w1, const float* const* w2, unsigned* const* wimg,
                         unsigned* const* kvf, float* const* wimg32, float* const* kvf32, float* kin, int B, int S, int nl,
                         hipStream_t st);
/* the layer's forward in the same organisation (training mode), exact fp32 products (v_mfma_f32_16x16x4_f32): arguments as tatt_tplayer_fwd
 * with the matrices / K / V replaced by wimg32 / kvf32; hmask (B*L 64-bit words, nullable) receives the relu-and-kept bits of the FFN's hidden layer -- word [16-token tile][channel
 * block][r], bit = lane -- which tatt_tplayer2_bwd reads instead of re-deciding the relu (a recomputation that differs from the forward in
 * the last bits flips a relu whose pre-activation is within ~1e-5 of zero: O(1) error on that token's gradients) */
int tatt_tplayer2_fwd(const float* x, const float* qpos, long qbs, const float* wimg32, const float* kvf32, const float* in_b,
                      const float* out_b, const float* b1, const float* b2, const float* lnA_w, const float* lnA_b,
                      const float* lnB_w, const float* lnB_b, const float* lnF_w, const float* lnF_b, float fin_scale,
                      int fin_both, float* xout, float* fin, float* wavg, unsigned long long* hmask, int B, int L, int S,
                      float p_attn, float p_res, float p_ffn, const unsigned long long* seed, unsigned site0, float eps,
                      hipStream_t st);
/* arguments as tatt_tplayer_bwd with the matrices / K / V replaced by their packed forms; kvflags: which sample the dK / dV
 * records of a work-group belong to (read by tatt_tplayer2_reduce_kv); ppart is summed by tatt_tplayer_reduce_params_g;
 * hmask: the bits tatt_tplayer2_fwd left (nullable: the relu is then decided by the recomputation) */
int tatt_tplayer2_bwd(const float* x, const float* qpos, long qbs, const unsigned* wimg, const unsigned* kvf, const float* in_b,
                      const float* out_b, const float* b1, const float* b2, const float* lnA_w, const float* lnA_b,
                      const float* lnB_w, const float* lnB_b, const float* lnF_w, const float* lnF_b, float fin_scale,
                      int fin_both, const float* dxout, const float* dfin, const float* dwavg, const float* dqacc, float* dx,
                      float* dqpos, float* kvpart, float* ppart, int* kvflags, const unsigned long long* hmask, int B, int L, int S,
                      float p_attn, float p_res, float p_ffn, const unsigned long long* seed, unsigned site0, float eps,
                      hipStream_t st);
int tatt_tplayer2_reduce_kv(const float* kvpart, const int* kvflags, float* dK, float* dV, int B, int L, int S, hipStream_t st);

/* ---- launches that synchronise their work-groups in flight: residency and the sticky error word -------------------------------- */

/* The persistent query-GRU recurrences (tatt_qgru_fwd_chain / _bwd_chain) and the STN-head launches (tatt_stn_*) exchange data between
 * work-groups INSIDE a launch: their whole grid must be resident at once.  These report, for the CURRENT device, how many work-groups of
 * each kernel fit (hipOccupancyMaxActiveBlocksPerMultiprocessor x the CUs the process sees), so that a caller on a partitioned or
 * CU-masked device takes the per-step / operator-chain path instead:
 *   tatt_qgru_chain_capacity: out[0] forward split-bf16, out[1] forward fp32, out[2] backward split-bf16, out[3] backward fp32
 *                             (a launch needs (Wb / 16) * 2 * (HID / 16) work-groups);
 *   tatt_stn_capacity:        out[0] the map launches (need <= 128), out[1] the fully connected launches (need 32). */
int tatt_qgru_chain_capacity(int* out);
int tatt_stn_capacity(int* out);
/* Every wait inside those launches is bounded by the wall clock (2 s); one that expires raises the launch's own error word AND ORs a code
 * (1: query GRU, 2: STN head, 4: LSTM chain) into the device's sticky word -- one zero-initialised 32-bit word in device memory registered here, which the
 * library never resets (NULL unregisters). */
int tatt_set_sticky(unsigned* word);
/* One-thread launch that traps (GPU exception: the process dies) if the sticky word is non-zero; no-op without a registered word.  Issued
 * in front of the optimiser kernels it keeps gradients of a launch that gave up waiting from ever reaching the weights. */
int tatt_sync_guard(hipStream_t st);

/* diagnostic: `groups` work-groups of 512 threads (lds_bytes of LDS each, <= 64 KB) that stay resident for `ticks` of the 100 MHz wall
 * clock (<= 1 s) and do nothing else -- a stand-in for a collective's channel kernels in the residency tests; sink: any device word */
int tatt_cu_holder(int groups, long ticks, int lds_bytes, unsigned* sink, hipStream_t st);

/* ---- small launches that keep the replayed step free of framework kernels ------------------------------------------------------------ */
/* dst[offs[k] .. + ns[k]) <- srcs[k] (zeros where srcs[k] == NULL) for k < count: one bucket of the flat gradient buffer gathered from
 * the parameters' gradient tensors in ONE launch.  srcs / offs / ns are HOST arrays; the table travels in the kernel arguments. */
int tatt_gather_grads(const float* const* srcs, const long* offs, const int* ns, int count, float* dst, hipStream_t st);
/* v[i] += 1 for n 64-bit counters */
int tatt_inc_i64(long long* v, int n, hipStream_t st);
/* y[0 .. n) = 0 */
int tatt_zero_f32(float* y, long n, hipStream_t st);

/* ---- TPS rectification ---------------------------------------------------------------------------------- */

/* src[b,p,:] = repr[p,:] @ (inv @ [ctrl[b]; pad])  (model/tps_spatial_transformer.py:103-105); N ctrl points, P pixels */
int tatt_tps_grid_fwd(const float* ctrl, const float* inv, const float* pad, const float* repr, float* src,
                      int B, int N, int P, hipStream_t st);
int tatt_tps_grid_bwd(const float* dsrc, const float* inv, const float* repr, float* dctrl, int B, int N,
                      int P, hipStream_t st);
/* out (B,H,W,C) = F.grid_sample(x, 2*clamp(src,0,1)-1) bilinear / zeros / align_corners=False
 * (model/tps_spatial_transformer.py:107-111,11); x[b*xsn + c*xsc + h*xsh + w*xsw] */
int tatt_grid_sample_fwd(const float* x, long xsn, long xsc, long xsh, long xsw, const float* src, float* out,
                         int B, int C, int H, int W, hipStream_t st);
/* gradient w.r.t. src (through the clamp); the LR image carries no gradient */
int tatt_grid_sample_bwd(const float* x, long xsn, long xsc, long xsh, long xsw, const float* src,
                         const float* dout, float* dsrc, int B, int C, int H, int W, hipStream_t st);

/* ImageLoss(gradient=True, loss_weight=[w0, w1]).forward (reference loss/image_loss.py:19-34,50-58): per-sample
 * loss[b] = w0*mean((sr-hr)^2) + w1*mean|gradient_map(sr[:3]) - gradient_map(hr[:3])|; when loss_mean != NULL also
 * loss_mean[0] = scale * mean_b loss[b] (interfaces/super_resolution.py:889-894 uses scale 100).  sr / hr are (B,C,H,W) images
 * addressed by element strides (n, c, h, w).  ws: workspace of B * 32 doubles (the fp64 wave sums of every image; the launch
 * spreads an image over 16 work-groups). */
int tatt_image_loss_fwd(const float* sr, long s_n, long s_c, long s_h, long s_w, const float* hr, long h_n, long h_c,
                        long h_h, long h_w, float* loss, float* loss_mean, float scale, double* ws, int B, int C, int H, int W,
                        float w0, float w1, hipStream_t st);
/* its gradient w.r.t. sr (dsr has sr's strides); exactly one of gper (B per-sample upstream gradients) and gscalar (upstream
 * gradient of the scaled batch mean, 1 element) is non-NULL */
int tatt_image_loss_bwd(const float* sr, long s_n, long s_c, long s_h, long s_w, const float* hr, long h_n, long h_c,
                        long h_h, long h_w, const float* gper, const float* gscalar, float scale, float* dsr,
                        int B, int C, int H, int W, float w0, float w1, hipStream_t st);

/* CRNN text-prior generator.  Bidirectional nn.LSTM (model/crnn/crnn.py:5-26), one launch per time step for
 * both directions; time-major (T, Bt, *) row-major tensors; gi (T,Bt,8H) = x W_ih^T + b_ih for [fwd | rev] x gates (i,f,g,o);
 * out (T,Bt,2H) = [h_fwd | h_rev] doubles as the h_{t-1} operand; cseq (2,T,Bt,H), gsave (2,T,Bt,4,H) are kept for the
 * backward.  H multiple of 256.  Step s handles time s (fwd) / T-1-s (rev). */
int tatt_lstm_fwd_step(const float* gi, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
                       float* out, float* cseq, float* gsave, int T, int Bt, int H, int s, hipStream_t st);
/* backward step s = T-1..0: dgates (2,T,Bt,4H) receives the pre-activation gate gradients of time(s); whhT_d = W_hh_d^T (H,4H);
 * dccarry (2,Bt,H) scratch carried between steps */
int tatt_lstm_bwd_step(const float* dout, const float* whhT_f, const float* whhT_r, const float* cseq, const float* gsave,
                       float* dgates, float* dccarry, int T, int Bt, int H, int s, hipStream_t st);
/* ---- eval-only kernels of the inference session (csrc/infer.hip, tatt_amd/infer.py) ---------------------------------------------- */
/* One bidirectional LSTM layer (H = 256), forward only, all T steps in ONE launch: same tiling, products and reduction order as
 * tatt_lstm_fwd_step (bitwise equal `out`), W_hh slice / b_hh / c state resident per work-group, h_{t-1} handed between the 16
 * work-groups of a (row block, direction) group with bounded waits (sticky code 4).  Writes only out (T,Bt,2H); gi as for
 * tatt_lstm_fwd_step; sync: 1024 words of workspace (zeroed by the call, word 1023 = this launch's error word).  Returns 1 for
 * geometries it does not take (H != 256, more than 256 work-groups = cdiv(Bt,16)*32, or more than the device holds at once). */
int tatt_lstm_fwd_chain(const float* gi, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
                        float* out, unsigned* sync, int T, int Bt, int H, hipStream_t st);
/* out[0]: work-groups of the chain kernel the current device holds at once */
int tatt_lstm_chain_capacity(int* out);
/* eval BatchNorm folded into the preceding convolution: s_o = gamma_o / sqrt(var_o + eps), w_out[o,:] = w[o,:] s_o,
 * b_out[o] = (bias[o] - mean[o]) s_o + beta[o] (bias may be NULL: 0).  w, w_out (Cout, K) contiguous. */
int tatt_bn_fold(const float* w, const float* bias, const float* gamma, const float* beta, const float* mean,
                 const float* var, float eps, float* w_out, float* b_out, int Cout, int K, hipStream_t st);
/* greedy CTC decoding (arg-max per step, ties to the lower class; repeats merged, blank 0 dropped; classes with keep[c] == 0 dropped)
 * of logits (T,B,C) by element strides, C <= 64, T <= 256, compared with label (B,T) int class indices / label_len (B) (< 0: cannot
 * match).  correct (B) 0/1, counter (+= correct images), dec (B,T) padded with -1, dec_len (B): each may be NULL. */
int tatt_ctc_greedy_match(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* keep,
                          const int* label, const int* label_len, int* correct, int* counter, int* dec, int* dec_len,
                          hipStream_t st);
/* tatt_ctc_greedy_match plus the Levenshtein distance (unit costs) between the decoding (n <= T classes) and the label, one wave per
 * image: the eval loop's editdistance.eval(pred, label) (interfaces/super_resolution.py:1531-1556).  label (B,64) int: classes of the
 * alphabet, ONE code >= 64 for every other kept character (it equals no decoded class), padding -1; label_len (B): m <= 64, or < 0
 * for a label the 64-character cap excludes.  correct / counter / dec / dec_len as in the match kernel (correct <=> dist == 0); dist (B),
 * -1 for an excluded label; dec rows are st_dec ints apart, the elements of correct, dec_len and dist st_img ints apart (columns of one
 * record tensor); hist (65): hist[max(n, m)] += dist, index 0 never written; scored / skipped: += 1 per image.  Integer atomics: the
 * totals do not depend on the order.  mean of dist / (max(n, m) + 1e-10) = sum_M hist[M] / (M + 1e-10) / scored.  Each output may be
 * NULL.  Returns 1 for T > 256, C > 64, B <= 0, and for T > 64 with a histogram. */
int tatt_ctc_greedy_score(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* keep,
                          const int* label, const int* label_len, int* correct, int* counter, int* dec, int* dec_len,
                          int* dist, long st_dec, long st_img, int* hist, int* scored, int* skipped, hipStream_t st);
/* id sequences scored on the device, one wave per row: what the eval loop does with an attention recogniser's ids (ids -> string ->
 * str_filt -> editdistance.eval, io._evaluate_ids).  ids: G*B rows of L class ids, st_row ints apart, row g*B + b = image b of image
 * kind g; cmap (C) int: 0 drops the id (as does an id outside [0,C)), -1 stops the row, any other value is a label code 1..63 and is
 * appended (n <= L codes); label (B,64) / label_len (B) as for tatt_ctc_greedy_score, shared by the G kinds.  rec row r, st_rec >= L + 3
 * ints apart: codes padded with -1 (L) | n | correct | dist (the record of tatt_ctc_greedy_score, L wide; dist -1: excluded label, not
 * correct); counter (G): [g] += correct; stats (G, bins + 2): [g][max(n, m)] += dist | [g][bins] += 1 scored | [g][bins + 1] += 1
 * skipped.  Integer atomics: the totals do not depend on the order.  rec, counter, stats: each may be NULL.  Returns 1 before any launch
 * for L < 1, L > 128, C < 1, C > 256, G*B < 1, and for stats with bins < max(L, 64) + 1. */
int tatt_ids_score(const int* ids, long st_row, int G, int B, int L, const int* cmap, int C, const int* label,
                   const int* label_len, int* rec, long st_rec, int* counter, int* stats, int bins, hipStream_t st);
/* out (B,OH,OW) = 0.299 R + 0.587 G + 0.114 B of F.interpolate(img[:, :3], (OH,OW), mode='bicubic') (interfaces/base.py:797-815);
 * img (B,C>=3,H,W) by element strides */
int tatt_bicubic_luma(const float* img, long sn, long sc, long sh, long sw, float* out, int B, int H, int W, int OH,
                      int OW, hipStream_t st);
/* out = F.interpolate(img, (OH,OW), mode='bicubic') of an fp32 batch, forward only (the eval loop's LR baseline,
 * interfaces/super_resolution.py:1417-1418), in the arithmetic of tatt_bicubic_luma: fp32 scale in / out, source = (o + 0.5) scale - 0.5,
 * A = -0.75, border taps clamped, horizontal sums first.  img (B,C,H,W) and out (B,C,OH,OW) by element strides (channels-last tensors
 * and channel slices are read / written as they are).  Returns 1 for a non-positive size. */
int tatt_bicubic_resize(const float* img, long sn, long sc, long sh, long sw, float* out, long on, long oc, long oh_s,
                        long ow_s, int B, int C, int H, int W, int OH, int OW, hipStream_t st);

/* SemanticLoss(pred, gt) = mean|gt - pred| + mean (gt+1e-20)(log(gt+1e-20) - log(pred+1e-20)) over n elements (reference
 * loss/semantic_loss.py:21-38: the student / teacher prior distillation loss); out[0] scalar; backward w.r.t. pred */
int tatt_semantic_loss_fwd(const float* pred, const float* gt, long n, float* out, hipStream_t st);
int tatt_semantic_loss_bwd(const float* pred, const float* gt, const float* gout, long n, float* dpred, hipStream_t st);
/* ---- CTC label supervision (csrc/ctc.hip; reference torch.nn.CTCLoss(blank=0, reduction='none'), interfaces/super_resolution.py:51,827-851) -- */
/* ONE launch: nll[b] = -log p(target_b | x[:, b]) and, when grad != NULL, the unit gradient w.r.t. the un-normalised scores,
 *   grad[t,b,c] = p[t,b,c] - exp(logsumexp_{s: l'_s = c}(alpha_t(s) + beta_t(s)) - lp[t,b,c] + nll[b]),  rows t >= in_len[b] zero
 * (grad (T,B,C) contiguous; the convention of ATen's backward; with normalized = 0 the row's log-softmax backward g - p sum_c g is applied
 * as well: zero in exact arithmetic, it takes the row's common fp32 error out).  x (T,B,C) by element strides; normalized = 1: x holds log-probabilities
 * (the drop-in form), 0: raw logits, the row log-softmax runs inside.  Labels from DEVICE memory: codes (n_codes int32), offs (B) element
 * offset of each sample's first code, tgt_len (B), in_len (B, or NULL = T for all).  tgt_len < 0: the sample is ignored (nll 0, gradient 0).
 * A target EQUAL to blank (not a CTC target; the reference's collate emits one for an empty word) gives what torch's CPU operator gives.
 * Infeasible samples (more targets, with the blanks repeats need, than steps; a code outside [0, C); an offset / length that leaves
 * codes or x): nll = +inf and a NaN gradient, or 0 and 0 with zero_infinity.  Bitwise reproducible (no atomics, fixed summation order).
 * Takes T <= 64, C <= 128 (tatt_ctc_loss_takes answers 1); returns 1 otherwise. */
int tatt_ctc_loss_fwd(const float* x, long st_t, long st_b, long st_c, int normalized, const int* codes, long n_codes,
                      const int* offs, const int* tgt_len, const int* in_len, int blank, int zero_infinity, float* nll,
                      float* grad, int T, int B, int C, hipStream_t st);
/* dx[t,b,c] = grad[t,b,c] * gout[b]; all contiguous */
int tatt_ctc_loss_bwd(const float* grad, const float* gout, float* dx, int T, int B, int C, hipStream_t st);
int tatt_ctc_loss_takes(int T, int C);
/* ---- batch collation (csrc/collate.hip; reference resizeNormalize + alignCollate_realWTLAMask, dataset/dataset.py:1266-1319,1980-2003) -- */
/* ONE launch, one work-group per item: PIL's bicubic resize (Image.resize(.., BICUBIC) of an RGB uint8 image, both passes in 22-bit fixed
 * point), ToTensor (float(v) / 255, planes C,H,W) and, with the mask flag, the fourth plane `1 where gray <= mean gray` -- bit for bit
 * what Pillow and torch give on the host.  packed (packed_bytes): the interleaved RGB sources; desc (n_items, 8) int32 in DEVICE memory:
 *   [0] byte offset of the source in packed  [1] H_src  [2] W_src  [3] OH  [4] OW  [5] mask flag  [6] float offset of the item's
 *   (3 + mask, OH, OW) planes in out  [7] 0
 * A pass whose source and target size agree is skipped, as in Pillow.  desc_host: the same rows in HOST memory, read before the launch
 * only to refuse what the kernel does not take: 2 for a geometry beyond tatt_collate_limits, 3 for a source or planes that leave
 * packed / out (out_floats), 1 for bad arguments; there is no fallback in here.  The kernel itself reads only device memory (the launch
 * can be captured) and re-checks every row: a row it would have refused gets NaN planes, or nothing when they lie outside out. */
int tatt_collate_images(const unsigned char* packed, long packed_bytes, const int* desc, const int* desc_host, int n_items,
                        float* out, long out_floats, hipStream_t st);
/* out[0..4]: most source rows, most source columns, most bytes of the horizontal pass's result (H_src * OW * 3, counted when
 * W_src != OW), largest OH, largest OW */
int tatt_collate_limits(int* out);
/* ---- image export (csrc/export.hip; reference eval loop interfaces/super_resolution.py:1572-1622: `.data.cpu().numpy() * 255`, clip,
 * astype(uint8), cubic resize, lr_sr_hr panel; tripple_display / test_display interfaces/base.py:565-618: ToPILImage -> Resize(.., BICUBIC)
 * -> ToTensor, make_grid(nrow=1), save_image) -- */
/* ONE launch, one work-group per item: quantise three channels of an fp32 image to uint8 and resize them as PIL does
 * (Image.fromarray(q).resize((OW, OH), BICUBIC), both passes in 22-bit fixed point) into interleaved RGB bytes -- bit for bit what numpy
 * and Pillow give on the host.  src: a (B, C, H, W) fp32 batch by element strides (channels-last SR tensors are read as they are);
 * desc (n_items, 8) int32 in DEVICE memory:
 *   [0] image index b  [1] first channel c0 (the item is channels c0 .. c0 + 2)  [2] OH  [3] OW  [4] quantisation rule
 *   [5] byte offset of the item's first pixel in out  [6] row pitch in bytes, >= 3 OW  [7] 0
 * Rule 0 ("floor", the eval loop): t = x * 255.0f (one fp32 multiply), clipped to [0, 255], truncated.  Rule 1 ("round",
 * torchvision.utils.save_image): t + 0.5f (one fp32 add), clipped, truncated.  NaN gives 0 under both rules, +-inf clips.
 * A pass whose source and target size agree is skipped, as in Pillow.  Offset and pitch let several launches lay their items into one
 * canvas (the lr_sr_hr panel).  desc_host: the same rows in HOST memory, read before the launch only to refuse what the kernel does not
 * take: 2 for a geometry beyond tatt_export_limits, 3 for an item whose channels, source or destination bytes leave src / out
 * (out_bytes), 1 for bad arguments (a rule other than 0 / 1 among them); there is no fallback in here.  The kernel itself reads only
 * device memory (the launch can be captured) and re-checks every row: it writes nothing for a row it refuses. */
int tatt_export_images(const float* src, long st_n, long st_c, long st_h, long st_w, int B, int C, int H, int W,
                       const int* desc, const int* desc_host, int n_items, unsigned char* out, long out_bytes, hipStream_t st);
/* out[0..4]: largest H, largest W, largest OH, largest OW, most bytes of the horizontal pass's result (H * OW * 3, counted when
 * W != OW).  Host only: needs no GPU. */
int tatt_export_limits(int* out);
/* ---- text lines of any width (csrc/lines.hip; tatt_amd/lines.py is the specification) -- */
/* ONE launch, one work-group per window: window x0 .. x0 + w - 1 of `line = img.resize((wl, h), BICUBIC)` for an RGB uint8 source,
 * ToTensor (float(v) / 255, planes C,H,W) and, with the mask flag, the fourth plane `1 where gray <= the WINDOW's mean gray` -- bit for
 * bit `resize_normalize`-style output of `line.crop((x0, 0, x0 + w, h))`.  The coefficient tables are those of the full line (W_src -> wl,
 * H_src -> h); only the window's columns are computed.  packed (packed_bytes): the interleaved RGB sources, one per LINE (all windows of a
 * line name the same offset); desc (n_windows, 12) int32 in DEVICE memory:
 *   [0] byte offset of the source in packed  [1] H_src  [2] W_src  [3] h  [4] wl  [5] x0  [6] w  [7] mask flag  [8] float offset of the
 *   window's (3 + mask, h, w) planes in out  [9..11] 0
 * A pass whose source and target size agree is skipped, as in Pillow.  desc_host: the same rows in HOST memory, read before the launch
 * only to refuse what the kernel does not take: 2 for a geometry beyond tatt_line_limits (or x0 outside 0 .. wl - w), 3 for a source or
 * planes that leave packed / out (out_floats), 1 for bad arguments or a reserved word; there is no fallback in here.  The kernel itself
 * reads only device memory (the launch can be captured) and re-checks every row: a row it would have refused gets NaN planes, or nothing
 * when they lie outside out. */
int tatt_line_windows(const unsigned char* packed, long packed_bytes, const int* desc, const int* desc_host, int n_windows,
                      float* out, long out_floats, hipStream_t st);
/* ONE launch for all lines: the SR windows src (B, C, H, W) fp32 by element strides (channels-last or contiguous) merged into one
 * (H, scale * wl, 3) uint8 canvas per line.  desc (n_lines, 8) int32 in DEVICE memory:
 *   [0] index of the line's first window in src and in starts  [1] its windows  [2] wl  [3] scale (W = scale * w)  [4] quantisation rule
 *   [5] first channel c0  [6] byte offset of the canvas in out  [7] row pitch in bytes, >= 3 * scale * wl
 * starts (n_starts) int32 in DEVICE memory: the LR column x_k of every window.  Every window is quantised like tatt_export_images (rule 0:
 * x * 255.0f clipped and truncated; rule 1: + 0.5f first; NaN -> 0).  Canvas column X takes every window k with
 * scale * x_k <= X < scale * x_k + W at its local column j = X - scale * x_k with the integer weight min(j + 1, W - j); the pixel is
 * (2 N + D) / (2 D) for N = sum weight * value, D = sum weight.  desc_host / starts_host: the same in HOST memory, read before the launch
 * only to refuse: 1 bad arguments or rule, 2 geometry (scale not dividing W, wl beyond tatt_line_limits, more windows than it reports,
 * starts that do not begin at 0, end flush right, increase and cover every column), 3 windows, channels or destination bytes that leave
 * src / starts / out (out_bytes).  The kernel reads only device memory and re-checks every row: it writes nothing for a row it refuses. */
int tatt_line_blend(const float* src, long st_n, long st_c, long st_h, long st_w, int B, int C, int H, int W, const int* desc,
                    const int* desc_host, int n_lines, const int* starts, const int* starts_host, int n_starts,
                    unsigned char* out, long out_bytes, hipStream_t st);
/* out[0..7]: most source rows, most source columns, largest wl, largest window height, largest window width, most bytes of the
 * horizontal pass's result (H_src * w * 3) and of its coefficient rows (w * ksize * 4), both counted when W_src != wl, most windows of
 * one line.  Host only: needs no GPU. */
int tatt_line_limits(int* out);
/* ---- scene images (csrc/scene.hip; tatt_amd/scene.py is the specification) -- */
/* tatt_line_windows for sources that are SUB-RECTANGLES (text boxes) of uploaded images: ONE launch, one work-group per window, bit for
 * bit the windows of `scene.crop(box)`.  desc (n_windows, 16) int32 in DEVICE memory: words [0..8] as tatt_line_windows has them, with
 * [0] the byte offset of the IMAGE's first pixel in packed and [1] H_src, [2] W_src the BOX's height and width (the coefficient tables
 * are the box's, not the image's);  [9] the image's row pitch in bytes, >= 3 * ([10] + W_src)  [10] box x0  [11] box y0  [12..15] 0.
 * A source of its own (the host fallback: a box beyond tatt_line_limits, resized by PIL) has pitch 3 * W_src and origin (0, 0).
 * Limits and return codes are those of tatt_line_windows (2 beyond tatt_line_limits, 3 for a box or planes that leave packed / out,
 * a negative origin or a pitch below the box's right edge, 1 for bad arguments or a reserved word); the kernel reads only device memory
 * and re-checks every row: a row it would have refused gets NaN planes, or nothing when they lie outside out. */
int tatt_scene_windows(const unsigned char* packed, long packed_bytes, const int* desc, const int* desc_host, int n_windows,
                       float* out, long out_floats, hipStream_t st);
/* Pillow's 8-bit bicubic Image.resize, uint8 RGB in device memory to uint8 RGB in device memory, tiled over the output (grid: tile x
 * item), so sources and targets of any size up to tatt_scene_limits go through; bit for bit Image.resize((OW, OH), BICUBIC): horizontal
 * pass first, its result rounded to uint8, a pass whose sizes agree skipped.  desc (n_items, 16) int32 in DEVICE memory:
 *   [0] byte offset of the source's first pixel in src  [1] H_src  [2] W_src  [3] source row pitch in bytes, >= 3 W_src
 *   [4] byte offset of the target's first pixel in dst  [5] OH  [6] OW  [7] target row pitch in bytes, >= 3 OW
 *   [8] feather F >= 0  [9..15] 0
 * F = 0 stores the resized pixels.  F > 0 blends them into what dst holds: a pixel at distance d = min(i, OH - 1 - i, j, OW - 1 - j)
 * from the nearest side of the target rectangle takes a = min(d + 1, F + 1), D = F + 1 and becomes
 * (2 (a new + (D - a) old) + D) / (2 D) in integers.  src and dst may be one buffer; the target rectangles of one launch must be
 * disjoint and must not overlap a source (the caller's layers see to it).  Every per-axis factor OUT / IN from 1 / 16 up is taken.
 * desc_host: the same rows in HOST memory, read before the launch only to refuse: 1 bad arguments, a reserved word or a negative
 * feather, 2 a geometry beyond tatt_scene_limits (a side, a down-scale beyond 16, the feather, more than 65535 items), 3 a source or
 * target rectangle that leaves src (src_bytes) / dst (dst_bytes).  The kernel reads only device memory (the launch can be captured)
 * and re-checks every row: it writes nothing for a row it refuses. */
int tatt_resize_u8(const unsigned char* src, long src_bytes, const int* desc, const int* desc_host, int n_items,
                   unsigned char* dst, long dst_bytes, hipStream_t st);
/* out[0..7]: largest side of a source or target of tatt_resize_u8, most boxes of one scene, tile height, tile width, largest down-scale
 * factor per axis, largest feather, most intermediate rows of a tile (the tile height is halved until its source rows fit), most items
 * of one launch.  Host only: needs no GPU. */
int tatt_scene_limits(int* out);
/* ---- quadrilateral text boxes (csrc/quads.hip; tatt_amd/quads.py is the specification) -- */
/* A projective warp of uint8 RGB in device memory to uint8 RGB in device memory, tiled over the output (grid: tile x item, one thread per
 * destination pixel), byte for byte `warp_u8_host`.  desc (n_items, 32) int32 in DEVICE memory:
 *   [0] byte offset of the source's first pixel in src  [1] H_src  [2] W_src  [3] source row pitch in bytes, >= 3 W_src
 *   [4] byte offset of the target's first pixel in dst  [5] OH  [6] OW  [7] target row pitch in bytes, >= 3 OW
 *   [8] feather F >= 0  [9] mode: 0 rectify, 1 paste  [10..27] the nine entries of the integer matrix m, row-major, each a 64-bit two's
 *   complement value as (low word, high word)  [28..31] 0
 * Destination pixel (i, j): with J = 2 j + 1, I = 2 i + 1: X = m00 J + m01 I + m02, Y = m10 J + m11 I + m12, Wd = m20 J + m21 I + m22 in
 * 64-bit integers; gx = floor(256 X / Wd), gy = floor(256 Y / Wd) (true floor division); fx = gx - 128, x0 = fx >> 8, ax = fx & 255 (fy
 * alike); the pixel is ((256 - ay) ((256 - ax) p[y0][x0] + ax p[y0][x0 + 1]) + ay ((256 - ax) p[y0 + 1][x0] + ax p[y0 + 1][x0 + 1]) +
 * 32768) >> 16 per channel, every tap index clamped to the source.  Mode 0 writes every destination pixel (zero where Wd <= 0).  Mode 1
 * paints a pixel iff Wd > 0, 0 <= gx < 256 W_src and 0 <= gy < 256 H_src and leaves every other pixel as it is; with F > 0 a painted pixel
 * at d = min(xi, W_src - 1 - xi, yi, H_src - 1 - yi), xi = gx >> 8, yi = gy >> 8, takes a = min(d + 1, F + 1), D = F + 1 and becomes
 * (2 (a new + (D - a) old) + D) / (2 D).  src and dst may be one buffer; the target rectangles of one launch must be disjoint and must
 * not overlap a source.  desc_host: the same rows in HOST memory, read before the launch only to refuse: 1 bad arguments, a reserved
 * word, a negative feather or an unknown mode, 2 a geometry beyond tatt_quad_limits (a side, the feather, more than 65535 items), 3 a
 * source or target rectangle that leaves src (src_bytes) / dst (dst_bytes).  The kernel reads only device memory (the launch can be
 * captured), re-checks every row (it writes nothing for a row it refuses) and clamps every tap whatever the matrix says. */
int tatt_warp_u8(const unsigned char* src, long src_bytes, const int* desc, const int* desc_host, int n_items,
                 unsigned char* dst, long dst_bytes, hipStream_t st);
/* out[0..5]: tile height, tile width, most items of one launch, largest side of a source or target, largest feather, ints per
 * descriptor row.  Host only: needs no GPU. */
int tatt_quad_limits(int* out);
/* ---- polygon text instances: curved text (csrc/polys.hip; tatt_amd/polys.py is the specification) -- */
/* The finished lines of polygons of 2 N points (N - 1 strips each, every strip a quad with a projective map of its own) pasted into the
 * polygons' bounding boxes, uint8 RGB in device memory to uint8 RGB in device memory, tiled over the output (grid: tile x item, one
 * thread per destination pixel), byte for byte `poly_paste_host`.  items (n_items, 16) int32 in DEVICE memory, one row per polygon:
 *   [0] byte offset of the line's first pixel in src  [1] H  [2] W  [3] line row pitch in bytes, >= 3 W
 *   [4] byte offset of the target's first pixel in dst  [5] OH  [6] OW  [7] target row pitch in bytes, >= 3 OW
 *   [8] feather F >= 0  [9] the item's first row in strips  [10] its strip count, 1 .. 15  [11..15] 0
 * strips (n_strips, 32) int32 in DEVICE memory, one row per strip, the strips of an item consecutive:
 *   [0] scale U_k, the strip's first column in the line  [1] scale w_k, its columns ([0] >= 0, [1] >= 1, [0] + [1] <= W)
 *   [2..19] the nine entries of the strip's integer matrix m, row-major, each a 64-bit two's complement value as (low word, high word)
 *   [20..25] A, B, C of the seam the strip begins at, alike (0 for an item's first strip)
 *   [26..31] A, B, C of the seam the strip ends at (0 for an item's last strip)
 * Destination pixel (i, j), J = 2 j + 1, I = 2 i + 1: the strips are tried in order and the first that claims the pixel paints it; a
 * pixel none claims is left as it is.  Strip k of n claims it iff A J + B I + C >= 0 for its first seam (k >= 1), A J + B I + C < 0 for
 * its last seam (k <= n - 2), Wd > 0, 0 <= gy < 256 H, gx >= 0 (k = 0) and gx < 256 [1] (k = n - 1), with X, Y, Wd, gx, gy as
 * tatt_warp_u8 states them.  The sample: gxg = gx + 256 [0], fx = gxg - 128, fy = gy - 128, the four taps clamped to the (H, W) line, the
 * bilinear sum of tatt_warp_u8; with F > 0, d = min(xi, W - 1 - xi, yi, H - 1 - yi) for xi = clamp(gxg >> 8, 0, W - 1), yi = gy >> 8 and
 * the blend of tatt_warp_u8 (one text for both entries: csrc/warp_pixel.h).  All in 64-bit integers.  src and dst may be one buffer;
 * the target rectangles of one launch must be disjoint and must not overlap a line.  items_host / strips_host: the same rows in HOST memory, read before the launch only to refuse:
 * 1 bad arguments, a reserved word or a negative feather, 2 a geometry beyond tatt_poly_limits (a side, the feather, the strip count, a
 * strip's columns outside the line, more than 65535 items), 3 a line or target rectangle that leaves src (src_bytes) / dst (dst_bytes),
 * 4 an item whose strip rows leave the table of n_strips rows.  The kernel reads only device memory (the launch can be captured),
 * re-checks every item (it writes nothing for an item it refuses) and clamps every tap whatever the matrices say. */
int tatt_poly_paste_u8(const unsigned char* src, long src_bytes, const int* items, const int* items_host, int n_items,
                       const int* strips, const int* strips_host, int n_strips, unsigned char* dst, long dst_bytes, hipStream_t st);
/* out[0..7]: tile height, tile width, most items of one launch, largest side of a line or target, largest feather, ints per item row,
 * ints per strip row, most strips of one polygon.  Host only: needs no GPU. */
int tatt_poly_limits(int* out);
/* ---- reading super-resolved lines at their own width (csrc/read.hip; tatt_amd/read.py is the specification) -- */
/* ONE launch for all lines of a call: every uint8 RGB line canvas in src (where tatt_line_blend left it) goes through Pillow's 8-bit
 * bicubic Image.resize((rw, 32), BICUBIC) (horizontal pass first, its result rounded to uint8, a pass whose sizes agree skipped), then
 * n = 299 R + 587 G + 114 B and float(n) * float(1 / 255000) -- bit for bit read.line_luma_host -- stored as the fp32 (32, rw) plane
 * at its float offset in out, tiled over the output (grid: tile x line).  desc (n_lines, 8) int32 in DEVICE memory:
 *   [0] byte offset of the line's first pixel in src  [1] H  [2] W  [3] row pitch in bytes, >= 3 W  [4] rw  [5] float offset of the
 *   (32, rw) target in out  [6..7] 0
 * desc_host: the same rows in HOST memory, read before the launch only to refuse: 1 bad arguments or a reserved word, 2 a geometry
 * beyond tatt_read_limits (rw, a down-scale beyond 16 per axis, the width, more than 65535 lines), 3 a source rectangle or a target
 * that leaves src (src_bytes) / out (out_floats).  The kernel reads only device memory and re-checks every row: a row it would have
 * refused gets a NaN target, or nothing when the target lies outside out. */
int tatt_line_luma(const unsigned char* src, long src_bytes, const int* desc, const int* desc_host, int n_lines, float* out,
                   long out_floats, hipStream_t st);
/* out[0..7]: the target height (32), largest rw, largest down-scale factor per axis, widest line, most lines of one launch, most steps T
 * and most classes C of tatt_ctc_greedy_read, ints per descriptor row.  Host only: needs no GPU. */
int tatt_read_limits(int* out);
/* greedy CTC decoding with confidences of logits (T,B,C) by element strides, T <= 256, C <= 64, one wave per image: per step the
 * arg-max (ties to the lower class) and its soft-max probability 1 / sum_c exp(x_c - max); repeats merged, blank 0 dropped, every other
 * class kept.  Image b writes the record row index[b] (rows st_rec 32-bit words apart; an index outside 0 .. n_rows - 1 writes nothing):
 *   [0, cap) decoded classes padded with -1  [cap, 2 cap) the first step of each decoded class's run, padded with -1
 *   [2 cap, 3 cap) fp32: the probability at that step, padded with 0  [3 cap] the decoded length
 *   [3 cap + 1] fp32: the minimum over ALL T steps of the arg-max's probability
 * Returns 1 for geometries it does not take (T, C, cap < T, st_rec < 3 cap + 2). */
int tatt_ctc_greedy_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* index, int* record,
                         int n_rows, int cap, long st_rec, hipStream_t st);
/* CTC prefix beam search (csrc/ctcbeam.hip; specification read.ctc_beam_read_host) of logits (T,B,C) fp32 by element strides, blank 0,
 * one wave per image, log-soft-max and all path sums in float64: the nbest most probable STRINGS of an image, best first, each with
 * logp = log of the sum over its alignments that the beam of `beam` prefixes kept.  A prefix is a node of the image's trie in LDS, found
 * through a (parent, class) table before a node is made, so a string has one identity however often it leaves and re-enters the beam.
 * Image b writes the record row index[b] (rows st_rec 32-bit words apart; an index outside 0 .. n_rows - 1 writes nothing):
 *   [0] entries written n <= nbest (fewer where the logits allow fewer strings)  [1] flag  then n entries of es = 4 + cap + (cap & 1)
 *   words, entry i at 2 + i es (8-byte aligned in a row that is): [0..1] the float64 logp as it is, low word first  [2] its length
 *   [3] 0  [4 ..) cap classes (+ one pad word for an odd cap) padded with -1.  Words beyond the n entries are left as they were.
 * flag 1, with [0] = 0 and nothing else written: a NaN or +inf logit, a step without a finite logit (-inf logits are legal otherwise),
 * or a key the table could not place (impossible at the table's size).
 * Returns 1 before any launch for: a null pointer, T outside 1 .. 256, C outside 1 .. 64, B or n_rows <= 0, not 1 <= nbest <= beam <= 16,
 * cap < T, st_rec < 2 + nbest es. */
int tatt_ctc_beam_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest,
                       const int* index, int* record, int n_rows, int cap, long st_rec, hipStream_t st);
/* out[0..4]: most steps T, most classes C and most beam entries of tatt_ctc_beam_read, the nodes of an image's trie (1 + 256 * 16) and
 * the slots of its lookup table.  Host only: needs no GPU. */
int tatt_beam_limits(int* out);
/* tatt_ctc_beam_read with a character n-gram language model fused into the search (the same kernel, instantiated with the LM statements;
 * specification read.ctc_beam_lm_read_host).  lmw: the increments table W of read.CharLM.increments on the device, lm_classes^order
 * float64 entries, W[h_1, .., h_{order-1}, c] with the most recent class of the history last and 0 for "before the line begins";
 * column 0 is the end of the line.  Weight and bonus are in the table: the kernel only adds its entries, in the order of the string, so an
 * entry's LM term equals the specification's bit for bit.  Candidates are ranked by (acoustic sum) + (LM term); after the last step the
 * beam is ranked once more by (tot + lm) + W[history][0], descending, ties to the lower rank, and the first nbest are written.
 * Record row: [0] entries  [1] flag  then per entry es = 6 + cap + (cap & 1) words: [0..1] float64 logp, the ACOUSTIC sum over the
 * alignments kept  [2..3] float64 lm, the LM term with the end increment  [4] length  [5] 0  [6 ..) cap classes padded with -1.
 * Returns 1 before any launch for everything tatt_ctc_beam_read refuses (with this es), a null table, order outside 1 .. 3,
 * lm_classes != C. */
int tatt_ctc_beam_lm_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest,
                          const double* lmw, int order, int lm_classes, const int* index, int* record, int n_rows, int cap, long st_rec,
                          hipStream_t st);
/* out[0..1]: the largest order and the most classes of a table tatt_ctc_beam_lm_read takes.  Host only: needs no GPU. */
int tatt_lm_limits(int* out);
/* tatt_ctc_beam_read held to a FORMAT (the same kernel, instantiated with the pattern statements; specification
 * read.ctc_beam_pattern_read_host).  The format is a DFA over the classes (read.Pattern): table: S rows of C bytes on the device,
 * table[q C + c] the state after class c in state q, or 255 where no string of the format continues that way (column 0 is never
 * read; an entry >= S is read as 255); accept: S bytes, non-zero for an accepting state; state 0 is the start state.  The state is kept
 * per trie node.  The extension of a beam entry by c is a candidate only where the table has a state for it; keys, tie rule and order
 * are the plain search's.  After the last step the entries in a non-accepting state are dropped and the first nbest of the rest are
 * written, in their order: the record row is tatt_ctc_beam_read's, [0] may be 0 on a clean line.
 * Returns 1 before any launch for everything tatt_ctc_beam_read refuses, a null table or accept, S outside 1 .. 64. */
int tatt_ctc_beam_pattern_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, int beam, int nbest,
                               const unsigned char* table, const unsigned char* accept, int S, const int* index, int* record,
                               int n_rows, int cap, long st_rec, hipStream_t st);
/* The exact log-probability that a line reads as ANY member of a format (csrc/ctcpat.hip; specification read.ctc_pattern_mass_host):
 * the sum over ALL alignments whose collapsed string the DFA (table, accept, S as above) accepts, carried per (state, last class) in
 * float64 probabilities with a power-of-two rescale per step; O(T S C) per line, one line per wave, no atomics, a fixed order of every
 * sum.  Line b writes 4 words at out + index[b] st_out (an index outside 0 .. n_rows - 1 writes nothing): [0..1] the float64 mass as
 * it is, low word first (-inf: nothing is accepted in T steps; NaN on a flagged line)  [2] flag (a NaN or +inf logit, a step without a
 * finite logit)  [3] 0.
 * Returns 1 before any launch, writing nothing, for: a null pointer, T outside 1 .. 256, C or S outside 1 .. 64, B or n_rows <= 0,
 * st_out < 4. */
int tatt_ctc_pattern_mass(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const unsigned char* table,
                          const unsigned char* accept, int S, const int* index, int* out, int n_rows, long st_out, hipStream_t st);
/* out[0..3]: most steps T, most classes C and most DFA states S of the two entries above, most beam entries.  Host only: needs no GPU. */
int tatt_pattern_limits(int* out);
/* Lexicon decoding (csrc/ctclex.hip; specification read.ctc_lexicon_read_host): scores[b][k] = the exact CTC log-probability (blank 0,
 * the forward recursion of read.ctc_string_logp_host in float64) of word k of a closed list under the logits (T,B,C) fp32 of image b,
 * given by element strides.  The list is packed by the host (read.Lexicon): codes: the class ids of all words one after the other
 * (n_codes ints; the buffer holds at least one), words: K rows of 4 ints
 *   [0] the word's length L <= 31  [1] the offset of its codes  [2] the caller's index of the word, 0 .. K - 1  [3] 0
 * sorted by segment class: first the k16 words run in segments of 16 lanes (2 L + 1 <= 16), then the k32 of 32 lanes, then the k64 of 64
 * (a word may sit in a wider class than its length asks for, never in a narrower one); k16 + k32 + k64 = K.  One launch per non-empty
 * class, grid (tiles of 256 / lanes words, B).  scores: (B, K) float64, rows st_sc doubles apart, written at the CALLER's index: -inf
 * where no alignment of T steps spells the word; NaN for every word of an image with a NaN or +inf logit or a step without a finite
 * logit, and for a word whose length, offset or codes (outside 1 .. C - 1) are out of range; a row whose own index is out of range is
 * not written.
 * Returns 1 before any launch for: a null pointer, T outside 1 .. 256, C outside 1 .. 64, B outside 1 .. 65535, K outside 1 .. 65536,
 * n_codes < 0, a negative class count or k16 + k32 + k64 != K, st_sc < K. */
int tatt_ctc_lexicon_score(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* codes, int n_codes,
                           const int* words, int K, int k16, int k32, int k64, double* scores, long st_sc, hipStream_t st);
/* The nbest <= 16 words of largest FINITE score of every image (descending, ties to the lower word index: comparisons only) and
 * logz = m + log sum_k exp(scores[b][k] - m), m the largest score, in float64; one work-group per image.  Image b writes the record row
 * index[b] (rows st_rec 32-bit words apart; an index outside 0 .. n_rows - 1 writes nothing):
 *   [0] entries written n <= nbest (fewer where fewer words have an alignment)  [1] flag  [2..3] the float64 logz as it is, low word
 *   first (-inf without a finite score)  then n entries of 4 words, entry i at 4 + 4 i: [0..1] the float64 logp  [2] the word's index
 *   [3] 0.  Words beyond the n entries are left as they were.
 * flag 1, with [0] = 0 and logz = NaN: every score of the image is a NaN (what tatt_ctc_lexicon_score writes for a flagged image).
 * Returns 1 before any launch for: a null pointer, B or n_rows <= 0, K outside 1 .. 65536, st_sc < K, nbest outside 1 .. 16,
 * st_rec < 4 + 4 nbest. */
int tatt_ctc_lexicon_select(const double* scores, long st_sc, int B, int K, int nbest, const int* index, int* record, int n_rows,
                            long st_rec, hipStream_t st);
/* out[0..4]: most steps T, most classes C, the longest word, most words K of a lexicon and most entries nbest.  Host only: needs no GPU. */
int tatt_lexicon_limits(int* out);
/* Per-line lexicons (csrc/ctclexp.hip; specification read.ctc_line_lexicons_read_host): every image b of the chunk has a list of words of
 * its own, and exactly the listed (image, word) pairs are scored.  codes / words: the UNION of all lists packed as tatt_ctc_lexicon_score
 * takes a list (U rows of 4 ints [length, offset of its codes, union index, 0]).  tiles: n_tiles rows of 4 ints
 *   [0] image b of the chunk  [1] segment class G = 16, 32 or 64  [2] first pair  [3] pairs of the tile, 1 .. 256 / G
 * pairs: n_pairs rows of 2 ints [0] the word's row in `words`  [1] j, its position in the image's own list; counts: B ints, the words of
 * every image's list.  ONE launch, one work-group per tile, which meets no other: scores[b * st_sc + j] = the exact CTC log-probability
 * of the pair's word under the logits of image b, bit for bit what tatt_ctc_lexicon_score writes for that word and image (NaN for every
 * pair of a flagged image, and for a word whose length, code offset or codes are out of range).  A tile whose image, class or pair range
 * is out of range, a pair whose word row is outside 0 .. U - 1 or whose j is outside 0 .. min(counts[b], max_count) - 1 writes nothing.
 * Returns 1 before any launch for: a null pointer, T outside 1 .. 256, C outside 1 .. 64, B outside 1 .. 65535, U outside 1 .. 1048576,
 * n_codes < 0, n_tiles <= 0, n_pairs <= 0, n_tiles > n_pairs, n_pairs > 65536 B, max_count outside 1 .. 65536, st_sc < max_count. */
int tatt_ctc_lexicon_score_pairs(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* codes, int n_codes,
                                 const int* words, int U, const int* tiles, int n_tiles, const int* pairs, int n_pairs, const int* counts,
                                 int max_count, double* scores, long st_sc, hipStream_t st);
/* tatt_ctc_lexicon_select with a count per image: image b has K_b = counts[b] scores, 0 <= K_b <= min(st_sc, 65536) (an image whose
 * count is outside that writes nothing).  The record row, the order of the entries and the 64 bits of logz are what
 * tatt_ctc_lexicon_select gives a (1, K_b) buffer.  K_b = 0: entries 0, flag 0, logz = -inf; flag 1 needs K_b >= 1 and every score a NaN.
 * Returns 1 before any launch for: a null pointer, B or n_rows <= 0, st_sc < 1, nbest outside 1 .. 16, st_rec < 4 + 4 nbest. */
int tatt_ctc_lexicon_select_rows(const double* scores, long st_sc, int B, const int* counts, int nbest, const int* index, int* record,
                                 int n_rows, long st_rec, hipStream_t st);
/* out[0..5]: most steps T, most classes C, the longest word, most words of ONE image's list, most distinct words of all lists (the
 * union) and most entries nbest.  Host only: needs no GPU. */
int tatt_line_lexicons_limits(int* out);
/* Word segmentation (csrc/ctcwords.hip; specification read.ctc_words_host): the most probable ALIGNMENT of image b whose collapsed
 * string is a sequence of words of the closed list (of length >= 1), with the steps every word spans -- token passing in float64 over
 * lp = log-soft-max of the logits (T,B,C) fp32 given by element strides, blank 0.  codes / words / K / k16 / k32 / k64: the packed list
 * exactly as tatt_ctc_lexicon_score takes it.  The list is laid over packed lanes: 16 per word of the first class, then from the next
 * multiple of 64 lanes 32 per word of the second, then from the next multiple of 64 lanes 64 per word of the third;
 * tatt_words_limits()[2] is the most lanes a call takes.  word_penalty is added wherever a word is entered.  ONE launch, one work-group
 * per image, which meets no other work-group.  Image b writes the record row index[b] (an index outside 0 .. n_rows - 1 writes
 * nothing, neither record nor lp_out), rows st_rec ints apart, in 32-bit words:
 *   [0] words written n <= cap  [1] flag  [2..3] the float64 logp as it is, low word first (-inf where no sequence of list words has an
 *   alignment: n = 0)  then n entries of 2 words, left to right: [0] the caller's index of the word  [1] first | last << 16, the step
 *   at which the word's first character was entered and the step at which it ended.  Words beyond the n entries are left as they were.
 * flag 1, with [0] = 0 and logp = NaN: a NaN, a +inf or a step without a finite logit.
 * lp_out, where not NULL: the (B, T, C) float64 log-soft-max the decoding ran on, image b at lp_out + b st_lp (NaN on a flagged image).
 * Returns 1 before any launch for: a null pointer (lp_out may be NULL), T outside 1 .. 256, C outside 1 .. 64, B outside 1 .. 65535,
 * K outside 1 .. 65536, n_codes < 0, a negative class count or k16 + k32 + k64 != K, more lanes than the limit, a word_penalty that is
 * not finite, n_rows <= 0, cap < T, st_rec < 4 + 2 cap, st_lp < T C with a non-NULL lp_out. */
int tatt_ctc_words_read(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* codes, int n_codes,
                        const int* words, int K, int k16, int k32, int k64, double word_penalty, const int* index, int* record,
                        int n_rows, int cap, long st_rec, double* lp_out, long st_lp, hipStream_t st);
/* out[0..4]: most steps T, most classes C, most packed lanes of a list, the threads of a work-group and the lanes a thread holds at that
 * limit.  Host only: needs no GPU. */
int tatt_words_limits(int* out);
/* CTC forced alignment (csrc/ctcalign.hip; specification read.ctc_align_host): the most probable ALIGNMENT of image b that spells a
 * given string, with the steps every character spans -- the Viterbi recursion over the string's 2 L + 1 states in float64 over
 * lp = log-soft-max of the logits (T,B,C) fp32 given by element strides, blank 0.  ONE launch, one work-group per image, which meets no
 * other.  The string of image b is read ON THE DEVICE from row index[b] of the int32 buffer src (src_rows >= n_rows rows, src_stride
 * words apart): its length L at word len_at, its classes from word cls_at; gate_at >= 0 names a word that must be >= 1 for a string to
 * exist (gate_at = -1: none).  src may be `record` itself (a decode launch's row: the string is read before the row is written).
 * Image b writes 4 + 4 cap_len words from word rec_at of the record row index[b] (an index outside 0 .. n_rows - 1 writes nothing,
 * neither record nor lp_out), rows rec_stride ints apart; rec_at and rec_stride even, record 8-byte aligned:
 *   [0] characters located n  [1] flag  [2..3] the float64 logp of the best alignment as it is, low word first (-inf where no
 *   alignment of T steps spells the string: n = 0)  [4 ..) cap_len pairs (first step, last step) of which n are written
 *   [4 + 2 cap_len ..) cap_len float64 of which n are written: the sum of lp[t][class] over the character's steps, left to right.
 *   Words beyond the n stated characters are left as they were.
 * flag 1, with n = 0 and logp = NaN: a NaN, a +inf or a step without a finite logit, or a gate word < 1.  flag 2, with n = 0 and
 * logp = NaN: L < 0, L > cap_len, L > 127 or a class outside 1 .. C - 1.  Flag 1 wins over flag 2.
 * lp_out: NULL or (B, T, C) float64, contiguous: the log-soft-max the recursion ran on, (double(x) - double(max)) - log sum exp (NaN on a
 * flagged image).  Everything after it is float64 addition and comparison: the record equals the specification run on lp_out bit for bit.
 * Returns 1 before any launch for: a null pointer (lp_out aside), T outside 1 .. 256, C outside 2 .. 64, B outside 1 .. 65535,
 * cap_len outside 0 .. 127, n_rows <= 0, src_rows < n_rows, len_at or gate_at outside the row, cls_at + cap_len > src_stride, an odd
 * rec_at or rec_stride, rec_at + 4 + 4 cap_len > rec_stride, a record that is not 8-byte aligned. */
int tatt_ctc_align(const float* logits, long st_t, long st_b, long st_c, int T, int B, int C, const int* index, const int* src,
                   int src_rows, long src_stride, int len_at, int cls_at, int gate_at, int* record, int n_rows, long rec_stride,
                   int rec_at, int cap_len, double* lp_out, hipStream_t st);
/* out[0..2]: most steps T, most classes C and the longest string.  Host only: needs no GPU. */
int tatt_align_limits(int* out);
/* calculate_psnr (reference utils/ssim_psnr.py:9-15) of two (B,C,H,W) images in [0,1] given by element strides, first 3 channels */
int tatt_psnr(const float* a, long a_n, long a_c, long a_h, long a_w, const float* b, long b_n, long b_c, long b_h, long b_w,
              float* out, int B, int C, int H, int W, hipStream_t st);

/* ---- SSIM / TRI_SSIM losses and the rotation augmentation of the shipped recipe (train_TATT.sh: --tssim_loss
 * --rotate_train=5) -------------------------------------------------------------------------------------------------------- */
/* out[n] = mean over (C,H,W) of the SSIM map of sample n -- reference utils/ssim_psnr.py:76-97 (_ssim, x3 == NULL) or :99-129
 * (_tri_ssim); 11x11 Gaussian window (sigma 1.5, :28-37), zero padding, one depth-wise filter per channel.  Images (B,C,H,W) are
 * given by element strides.  ws: B*C*ceil(H/16)*ceil(W/64) doubles. */
int tatt_ssim_fwd(const float* x1, long a_n, long a_c, long a_h, long a_w, const float* x2, long b_n, long b_c, long b_h,
                  long b_w, const float* x3, long c_n, long c_c, long c_h, long c_w, int B, int C, int H, int W,
                  float* out, double* ws, hipStream_t st);
/* gradients of sum_n gs[n] * out[n] w.r.t. the images (contiguous (B,C,H,W) outputs; any of dx1/dx2/dx3 may be NULL).
 * maps: workspace of B*C*5*H*W floats. */
int tatt_ssim_bwd(const float* x1, long a_n, long a_c, long a_h, long a_w, const float* x2, long b_n, long b_c, long b_h,
                  long b_w, const float* x3, long c_n, long c_c, long c_h, long c_w, int B, int C, int H, int W,
                  const float* gs, float* maps, float* dx1, float* dx2, float* dx3, hipStream_t st);
/* out (B,C,H,W contiguous) = F.grid_sample(x, F.affine_grid(theta (B,2,3), x.shape)) -- bilinear, zeros padding,
 * align_corners=False: the resampling of torch_distortion / TextSR.torch_rotate_img (reference model/__init__.py:4-29,
 * interfaces/super_resolution.py:126-157).  x by element strides. */
int tatt_affine_sample_fwd(const float* x, long xsn, long xsc, long xsh, long xsw, const float* theta, float* out, int B,
                           int C, int H, int W, hipStream_t st);
/* gradient w.r.t. the image (deterministic gather; dout, dimg contiguous (B,C,H,W), C <= 4) */
int tatt_affine_sample_bwd(const float* theta, const float* dout, float* dimg, int B, int C, int H, int W,
                           hipStream_t st);

/* ---- the ASTER recogniser (reference model/recognizer/; csrc/aster.hip, its decoder csrc/attndec.hip) ------------------------------- */
/* y (B,C,Ho,Wo contiguous) = F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=True) (recognizer_builder.py:77: the STN head
 * reads the image squeezed to 32 x 64); x[b*xsn + c*xsc + h*xsh + w*xsw] */
int tatt_resize_bilinear_ac(const float* x, long xsn, long xsc, long xsh, long xsw, float* y, int B, int C, int H, int W,
                            int Ho, int Wo, hipStream_t st);
/* tatt_grid_sample_fwd with an output size of its own: src (B, Ho*Wo, 2), out (B,Ho,Wo,C), x (B,C,H,W) by element strides
 * (the recogniser rectifies its 32 x 128 input into 32 x 100: recognizer_builder.py:20-21,79) */
int tatt_grid_sample_sized_fwd(const float* x, long xsn, long xsc, long xsh, long xsw, const float* src, float* out, int B,
                               int C, int H, int W, int Ho, int Wo, hipStream_t st);
/* y = relu(a + b): the tail of AsterBlock (resnet_aster.py:59-60), where the activation follows the residual sum */
int tatt_add_relu(const float* a, const float* b, float* y, long n, hipStream_t st);
/* one nn.GRU step from its projections: gi, gh (R, 3H) in gate order r|z|n, h (R, H) -> hout (R, H) (the decoder's step-by-step route) */
int tatt_gru_cell(const float* gi, const float* gh, const float* h, float* hout, int R, int H, hipStream_t st);
/* AttentionRecognitionHead (attention_recognition_head.py), all L steps in ONE launch, one work-group per image, no synchronisation
 * between work-groups.  x, xproj (B,T,512): encoder features and xEmbed(x); WsT (512,512) = sEmbed.weight^T, bs; wv (512), wb (1): wEmbed;
 * E2 (C+1, 1536) = tgt_embedding.weight W_ih[:, :512]^T + b_ih; WicT (512,1536) = W_ih[:, 512:]^T; WhhT (512,1536) = W_hh^T, bhh (1536);
 * fcT (512, C) = fc.weight^T, fcb (C).
 * mode 0 forced: y_prev from targets (B,L) int (clamped to [0, C]) -> logits (B,L,C);
 * mode 1 greedy (`sample`): ids (B,L) int, scores (B,L) = the arg-max's softmax value; beyond a row's first EOS ids = eos, scores = 0;
 * mode 2 beam (`beam_search`, beam = 5, backtracking included; candidates ordered by score descending, then flat index ascending):
 *        ids = the best sequence per image, scores = 1.
 * Takes T <= 32, 2 <= C <= 128 (5 <= C for the beam), L <= 100, sDim = attDim = xDim = 512; anything else returns 1. */
int tatt_attn_decode(const float* x, const float* xproj, const float* WsT, const float* bs, const float* wv, const float* wb,
                     const float* E2, const float* WicT, const float* WhhT, const float* bhh, const float* fcT,
                     const float* fcb, const int* targets, float* logits, int* ids, float* scores, int B, int T, int C, int L,
                     int sDim, int attDim, int xDim, int eos, int mode, int beam, hipStream_t st);
/* the backtracking of `beam_search` alone (attention_recognition_head.py:127-187; tatt_attn_decode does it itself): stored decisions
 * sym, pred (slot of the previous step), score, each (L, B, K), K <= 8 -> ids (B, L) of the best sequence per image; ws: B*L*K ints.
 * Ties: score descending, then index ascending. */
int tatt_beam_backtrack(const int* sym, const int* pred, const float* score, int* ids, int* ws, int L, int B, int K, int eos,
                        hipStream_t st);

/* ---- the MORAN recogniser (reference model/moran/; csrc/moran.hip, its decoder csrc/attndec.hip) ------------------------------------ */
/* The tail of the MORN rectifier in ONE launch (morn.py:62-69 for the first pass, :76-82 for the second).  o (B,h,w): the offsets
 * network's output.  Per output pixel of the Ho x Wo regular grid (the reference's fp32 grid: float64 arange * 2 / (n - 1) - 1 rounded
 * once): g = grid_sample(maxpool_{2,1}(relu(o)) - maxpool_{2,1}(relu(-o)), grid); acc (B,Ho,Wo) = g if `first` else acc + g;
 * out (B,Ho,Wo,C) = grid_sample(x, (gx, gy + acc)), x (B,C,H,W) read as x[b*xsn + c*xsc + y*xsh + x*xsw].  Both samplers are bilinear,
 * zeros padding, align_corners=False (how the installed torch runs the reference's calls).
 * Returns 1 for h < 2, w < 2, C > 4, h * w > 4096, Ho < 2 or Wo < 2. */
int tatt_morn_rectify(const float* o, int h, int w, float* acc, int first, const float* x, long xsn, long xsc, long xsh,
                      long xsw, float* out, int B, int C, int H, int W, int Ho, int Wo, hipStream_t st);
/* One direction of the ASRN attention decoder (asrn_res.py:39-65 the cell, :127-155 the test-mode loop), all L steps in ONE launch, one
 * work-group per image, no synchronisation between work-groups.  feats, fproj (B,T,256): encoder features and i2h(feats);
 * WhT (256,256) = h2h.weight^T, bh (256); wv (256) = score.weight; E2 (C+1, 768) = char_embeddings W_ih[:, 256:]^T + b_ih;
 * WicT (256,768) = W_ih[:, :256]^T (the context comes first in the GRU input); WhhT (256,768) = W_hh^T, bhh (768);
 * genT (256, C) = generator.weight^T, genb (C).  The embedding row of step 0 is 0 (greedy) or targets[b, 0] (forced).
 * mode 0 forced: the embedding row of step i is targets[b, i] (B,L) int, clamped to [0, C] -> logits (B,L,C);
 * mode 1 greedy: y = argmax + 1, ties to the lower class, no stop at '$' -> logits (B,L,C) and ids (B,L) int.
 * Takes H = 256 (hidden = feature = embedding size), T <= 32, 2 <= C <= 64, L <= 64; anything else returns 1. */
int tatt_moran_decode(const float* feats, const float* fproj, const float* WhT, const float* bh, const float* wv,
                      const float* E2, const float* WicT, const float* WhhT, const float* bhh, const float* genT,
                      const float* genb, const int* targets, float* logits, int* ids, int B, int T, int C, int L, int H,
                      int mode, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif /* TATT_HIP_H */
