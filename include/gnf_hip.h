/* gnf_hip.h -- C ABI of libgnf_hip.so: the MI355X (gfx950) kernels under the
 * Conditioner / Normalizer plug-in API of Graphical-Normalizing-Flows.
 *
 * The reference has no FFI of its own (it is pure Python on torch ops); the drop-in
 * boundary is the Python class protocol of models/ (SURVEY.md 8b).  Each entry point
 * below replaces the torch-op sequence of the cited reference lines and is what the
 * host-side mirror (graphical-normalizing-flows_amd/models) binds with ctypes.
 *
 * Conventions (all entry points):
 *   - plain C types only; device pointers are raw (tensor.data_ptr()); fp32 everywhere;
 *   - `stream` is a hipStream_t passed as void* (torch's current stream);
 *   - returns 0 on success, a negative GNF_E* code for bad arguments, or a positive
 *     hipError_t from the launch; never throws, never allocates, never synchronises;
 *   - the caller owns and sizes every buffer, including workspaces (gnf_*_ws_bytes);
 *   - no global mutable state: safe for one process per GPU and for several streams;
 *   - strides are in ELEMENTS, not bytes;
 *   - ALIGNMENT: every fp32 array -- inputs, outputs, parameters, cotangents, gradient arrays -- may sit at any
 *     4-byte-aligned address (a slice of a [n, 21] data set, a view into a flat parameter or gradient buffer); 16-byte
 *     alignment only selects faster kernels (the float4 forms of the row-wise and Adam kernels, the exact-K tall-layer
 *     kernels, the dedicated GEMM families) and never changes what is computed beyond the rounding of another summation
 *     order.  The exceptions, all of them buffers the library itself fills and that are read in 16-byte pieces -- they must
 *     be 16-byte aligned, and the entry points refuse another address with GNF_EINVAL before any launch:
 *       the saved conv1 activations a1save / a1saved (gnf_mnistcnn_conv_fwd_save, *_a1),
 *       the weight images `pack` of gnf_monotonic_pack and gnf_made_prefix_pack and of every entry point that reads them,
 *       the byte workspaces `ws` of gnf_monotonic_bwd and `ws` / `prep` of gnf_mnistcnn_sparse_fwd_prepared_fc2.
 *     and the measurement probe gnf_probe_copy, a float4 stream copy by definition, refuses a dst / src that is not.
 *     (Every other `void*` workspace should be 16-byte aligned as well; any allocator's result is.)
 *     tests/test_gpu_alignment.py runs every entry point at the offsets 4, 8 and 12;
 *   - an EMPTY batch (B, n_img, M or the row count = 0) is a valid call, as it is in the
 *     reference (torch ops on [0, d] tensors): arrays sized by the batch may then be NULL
 *     (torch hands out a null data_ptr for them), nothing is launched over them, and the
 *     backward entry points still write ZERO parameter gradients.
 */
#ifndef GNF_HIP_H
#define GNF_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 11 still: gnf_lenet_gated_*, gnf_lenet_rows_*, gnf_image_prep, gnf_dagmlp_*, gnf_dag_levels*, gnf_toy_sample, gnf_shuffle_keys, gnf_tab_batch, gnf_group_bias_*, gnf_spline_*, gnf_made_prefix*_spline, gnf_made_prefix_do, gnf_nll_do_* and gnf_affine_do_* were ADDED under this number (no existing symbol
 * changed; a binding written against the earlier 11 keeps working, and tests/test_cifar_factory.py pins the value);
 * gnf_strade_* (gnf_strade_adjoint* among them) likewise, and gnf_monotonic_inv_route / gnf_monotonic_inv_kernel and
 * gnf_spline_route */
#define GNF_ABI_VERSION 11
#define GNF_EINVAL (-1)   /* bad argument (null pointer, negative size, ...)          */
#define GNF_ESHAPE (-2)   /* shape not supported by any compiled kernel instantiation */
#define GNF_EWS    (-3)   /* workspace too small                                      */

typedef void* gnf_stream_t;

int gnf_abi_version(void);

/* ---- Affine normalizer: models/Normalizers/AffineNormalizer.py:9-17 -------------------
 * mu = clamp(h[..,0],-5,5); sigma = exp(clamp(h[..,1],-5,2)); z = x*sigma + mu.
 * x,z,jac: [B,d] contiguous.  h[b,i,c] at b*h_sb + i*h_sd + c*h_sc (MADE hands over a
 * permuted view).  jac (= sigma), logdet (= sum_i log sigma = sum_i clamp(h1)) and logn
 * (= -0.5 sum_i (log 2pi + z^2), the NormalLogDensity of NormalizingFlowFactories.py:15-16
 * fused into the pass that produces z) may be NULL.  clamp_inplace != 0 writes the clamped
 * values back into h like the reference's clamp_ does. */
int gnf_affine_fwd(const float* x, float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                   float* z, float* jac, float* logdet, float* logn, int clamp_inplace,
                   int64_t B, int64_t d, gnf_stream_t stream);
/* Backward of the above.  gz: [B,d] or NULL; gjac: [B,d] or NULL; glogdet, glogn: [B] or
 * NULL (glogn: z's cotangent gains -z*glogn[b], z recomputed in the kernel).
 * gx: [B,d] or NULL.  gh[b,i,c] at b*g_sb + i*g_sd + c*g_sc receives components 0,1
 * (components >= 2 are never read by the normalizer: caller zero-fills them). */
int gnf_affine_bwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                   const float* gz, const float* gjac, const float* glogdet, const float* glogn,
                   float* gx, float* gh, int64_t g_sb, int64_t g_sd, int64_t g_sc,
                   int64_t B, int64_t d, gnf_stream_t stream);
/* x = (z - mu)/sigma  (AffineNormalizer.py:14-17). */
int gnf_affine_inv(const float* z, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                   float* x, int64_t B, int64_t d, gnf_stream_t stream);

/* ---- Spline normalizer: monotone rational-quadratic spline (Durkan et al. 2019), K bins on [-T, T], identity outside ---
 * 2 <= K <= 32, T > 0 (else GNF_EINVAL).  Of the h_c components of h[b,i,:] (addressed as in gnf_affine_*; h_c < 3K-1:
 * GNF_ESHAPE) the first 3K-1 are read: K width logits, K height logits, K-1 derivative logits.
 *   w = 1e-3 + (1 - 1e-3 K) softmax(h[0:K]),  X_0 = -T, X_k = -T + 2T sum_{j<k} w_j, X_K = T; Y alike from h[K:2K];
 *   D_0 = D_K = 1, D_k = 1e-3 + softplus(h[2K+k-1]);  k = #{j in 1..K-1: x >= X_j}, W = X_{k+1}-X_k, H = Y_{k+1}-Y_k,
 *   xi = (x-X_k)/W, s = H/W, e = D_{k+1}+D_k-2s, den = s + e xi(1-xi):
 *   z = Y_k + H (s xi^2 + D_k xi(1-xi))/den,  jac = s^2 (D_{k+1} xi^2 + 2 s xi(1-xi) + D_k (1-xi)^2)/den^2   for -T <= x <= T,
 *   z = x, jac = 1 otherwise (NaN and +-inf included).
 * fwd: z [B,d]; jac [B,d], logdet [B] (= sum_i log jac) and logn [B] (= -0.5 sum_i (log 2pi + z^2)) may be NULL; the
 *   reductions happen in the pass that produces z, in a fixed order.
 * bwd: recomputes the forward; cotangents gz, gjac [B,d], glogdet, glogn [B], each may be NULL; gx [B,d] or NULL;
 *   gh[b,i,c] at b*g_sb + i*g_sd + c*g_sc receives components 0 .. 3K-2 (the caller zero-fills any beyond).
 * inv: x = the inverse of z.  out_cols == NULL: x [B,d].  out_cols (int32 [B]) given: the variable-major scatter form
 *   of gnf_monotonic_inv_scatter -- z [B,d] holds B variables of d samples and element (b,j) goes to
 *   x[j*out_width + out_cols[b]]; nothing else of x is written. */
int gnf_spline_fwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, double T,
                   float* z, float* jac, float* logdet, float* logn, int64_t B, int64_t d, gnf_stream_t stream);
int gnf_spline_bwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, double T,
                   const float* gz, const float* gjac, const float* glogdet, const float* glogn, float* gx, float* gh,
                   int64_t g_sb, int64_t g_sd, int64_t g_sc, int64_t B, int64_t d, gnf_stream_t stream);
int gnf_spline_inv(const float* z, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, double T,
                   float* x, const int32_t* out_cols, int64_t out_width, int64_t B, int64_t d, gnf_stream_t stream);
/* How the three entry points above would run a problem: which = 0 (fwd), 1 (bwd), 2 (inv) and the h address, strides, h_c,
 * K, B and d the entry point itself would get; gh and its strides for which = 1 (ignored otherwise); scatter != 0: inv with
 * out_cols.  One line in buf (len bytes, NUL included; too short: GNF_EINVAL):
 *   "spline_fwd_k rows_per_wg=<RT> chunks=<nchunk> grid=<workgroups> lds=<dynamic LDS bytes> h=<span16|span4|rows>
 *    tiles16=<staged tiles of h that take the 16-byte path>", then " gh=<span16|span4|rows> gtiles16=<..>" for bwd and
 *   " out=<plain|cols>" for inv.  fwd gives a workgroup RT = 128 / d whole rows, or one row in chunks of 128 columns
 *   (grid x chunks staged tiles); spline_bwd_k and spline_inv_k tile the B d elements by 128 whatever the rows are:
 *   rows_per_wg=0 chunks=1.  h= names the layout's route (DESIGN.md section 6 has the table of conditions): span16 is
 *   decided per tile, and tiles16 counts the tiles that take it, the others going by dwords.
 * Host arithmetic only, from the function the entry points launch from: nothing is launched, no pointer is dereferenced (h
 * and gh count by their low four bits alone, NULL still being refused), GNF_EINVAL / GNF_ESHAPE as the entry points
 * (the tail bound, which the query is not given, apart); an empty batch gives the empty line. */
int gnf_spline_route(int which, const void* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, int64_t B,
                     int64_t d, const void* gh, int64_t g_sb, int64_t g_sd, int64_t g_sc, int scatter, char* buf, int len);

/* ---- row reductions: models/NormalizingFlow.py:70, NormalizingFlowFactories.py:15-16 --
 * logsum:  out[b] = sum_i log(jac[b,i]);        bwd: gjac[b,i] = g[b]/jac[b,i]
 * normal:  out[b] = -0.5*sum_i(log(2pi)+z^2);   bwd: gz[b,i]  = -z[b,i]*g[b]        */
int gnf_logsum_rows_fwd(const float* jac, float* out, int64_t B, int64_t d, gnf_stream_t stream);
int gnf_logsum_rows_bwd(const float* jac, const float* g, float* gjac, int64_t B, int64_t d, gnf_stream_t stream);
int gnf_normal_logdensity_fwd(const float* z, float* out, int64_t B, int64_t d, gnf_stream_t stream);
int gnf_normal_logdensity_bwd(const float* z, const float* g, float* gz, int64_t B, int64_t d, gnf_stream_t stream);
/* Both reductions of a flow step's tail in ONE pass over z and jac (the "gnf_nll_reduce" of SURVEY.md 8b; used behind
 * normalizers whose kernel cannot reduce over a row itself, i.e. the Monotonic one):
 *   logdet[b] = sum_i log(jac[b,i])   logn[b] = -0.5*sum_i(log(2pi)+z[b,i]^2)
 * bwd: gz[b,i] = (gz_in ? gz_in[b,i] : 0) - z[b,i]*glogn[b],  gjac[b,i] = glogdet[b]/jac[b,i]
 *      (glogdet / glogn / gz_in may be NULL = zero). */
int gnf_nll_reduce_fwd(const float* z, const float* jac, float* logdet, float* logn, int64_t B, int64_t d,
                       gnf_stream_t stream);
int gnf_nll_reduce_bwd(const float* z, const float* jac, const float* glogdet, const float* glogn, const float* gz_in,
                       float* gz, float* gjac, int64_t B, int64_t d, gnf_stream_t stream);
/* Interventional likelihood (csrc/gnf_do_terms.hip): the same two reductions over the FREE variables only, the truncated
 * factorisation  log p(x | do(x_S)) = sum_{i not in S} [log jac_i + log N(z_i)].
 *   pin    uint8 [R, d], device, contiguous, ANY address (read byte by byte); non-zero = variable i is an intervention
 *          target in regime r.  NULL is GNF_EINVAL: the unmasked entry points above exist.
 *   regime int32 [B] or NULL.  NULL: R == 1 applies row 0 of pin to every sample, R == B applies row b to sample b, any
 *          other R is GNF_EINVAL.  A regime id outside [0, R) never indexes the table: that sample's logdet and logn are NaN,
 *          and in the backward its row of every output cotangent is NaN.
 *   fwd:  logdet[b] = sum_{i free} log jac[b,i]     logn[b] = -0.5 sum_{i free} (log 2pi + z[b,i]^2)
 *   bwd:  free:    gz[b,i] = (gz_in ? gz_in[b,i] : 0) - z[b,i] glogn[b]    gjac[b,i] = glogdet[b] / jac[b,i]
 *         pinned:  gz[b,i] = (gz_in ? gz_in[b,i] : 0)                      gjac[b,i] = +0
 *         (glogdet / glogn / gz_in may be NULL = zero)
 * A pinned element's z and jac never enter a sum or a cotangent (select, not multiply: they may be inf, NaN or 0).  B == 0
 * returns 0 before any pointer is looked at.  Fixed summation order for a given (B, d, R, alignment), no atomics, no
 * workspace. */
int gnf_nll_do_fwd(const float* z, const float* jac, const uint8_t* pin, const int32_t* regime, int64_t R, float* logdet,
                   float* logn, int64_t B, int64_t d, gnf_stream_t stream);
int gnf_nll_do_bwd(const float* z, const float* jac, const uint8_t* pin, const int32_t* regime, int64_t R,
                   const float* glogdet, const float* glogn, const float* gz_in, float* gz, float* gjac, int64_t B, int64_t d,
                   gnf_stream_t stream);
/* The fused form for the Affine normalizer: gnf_affine_fwd / _bwd (without clamp_inplace; any strides of h / gh) with
 * logdet / logn reduced over the free columns in the pass that writes z.  z (and jac, optional) are written for EVERY column;
 * a pinned column's z is defined and unused.  bwd: gz / gjac (optional) act on every element as in gnf_affine_bwd; the row
 * cotangents glogdet / glogn reach gh and gx through free elements only.  logn / glogn may be NULL as in the unmasked pair. */
int gnf_affine_do_fwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, const uint8_t* pin,
                      const int32_t* regime, int64_t R, float* z, float* jac, float* logdet, float* logn, int64_t B,
                      int64_t d, gnf_stream_t stream);
int gnf_affine_do_bwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, const uint8_t* pin,
                      const int32_t* regime, int64_t R, const float* gz, const float* gjac, const float* glogdet,
                      const float* glogn, float* gx, float* gh, int64_t g_sb, int64_t g_sd, int64_t g_sc, int64_t B, int64_t d,
                      gnf_stream_t stream);
/* FCNormalizingFlow.loss (models/NormalizingFlow.py:144-146): out[0] = addend[0] - mean_b(logdet[b] + logn[b]) (addend: the
 * constraints term as a device scalar, or NULL = 0), one workgroup, fixed summation order;
 * bwd: glogdet[b] = glogn[b] = -g[0]/B (g: device scalar; the addend's cotangent is g itself). */
int gnf_nll_mean_fwd(const float* logdet, const float* logn, const float* addend, float* out, int64_t B,
                     gnf_stream_t stream);
int gnf_nll_mean_bwd(const float* g, float* glogdet, float* glogn, int64_t B, gnf_stream_t stream);
/* The same loss from z itself (round 5): out[0] = addend[0] - mean_b(logdet[b] + logN(z[b,:])), logN as in
 * NormalizingFlowFactories.py:15-16 -- the loss scores the z it is handed, whatever wrote it (no density remembered from
 * the forward pass).  One workgroup, B*d <= gnf_nll_loss_max_elems() (GNF_ESHAPE above: use gnf_normal_logdensity_fwd +
 * gnf_nll_mean_fwd).  bwd: gz[b,i] = g[0] z[b,i] / B, glogdet[b] = -g[0] / B. */
int64_t gnf_nll_loss_max_elems(void);
int gnf_nll_loss_fwd(const float* z, const float* logdet, const float* addend, float* out, int64_t B, int64_t d,
                     gnf_stream_t stream);
int gnf_nll_loss_bwd(const float* g, const float* z, float* gz, float* glogdet, int64_t B, int64_t d, gnf_stream_t stream);
/* out[n] = sum_m a[m*lda + n]  (bias gradients; deterministic two-level reduction).
 * ws: >= gnf_colsum_ws_bytes(M,N) bytes. */
int64_t gnf_colsum_ws_bytes(int64_t M, int64_t N);
int gnf_colsum(const float* a, int64_t lda, float* out, int64_t M, int64_t N, float* ws, gnf_stream_t stream);

/* ---- Linear / masked-Linear layers of the conditioner MLPs ----------------------------------------------------------
 * MADE's MaskedLinear (models/Conditionners/AutoregressiveConditioner.py:14-25: F.linear(x, mask * W, b)) and the plain
 * Linear + ReLU chains of CouplingMLP / DAGMLP, forward and autograd.  x: [M,K], W: [N,K] (nn.Linear layout), y: [M,N],
 * all contiguous.  The mask is either `mask` ([N,K], 0/1, may be NULL = none) or, when deg_out / deg_in are given, the
 * degree rule mask[o][i] = deg_in[i] <= deg_out[o] (strict != 0: <) of AutoregressiveConditioner.py:85-96 evaluated in
 * the kernel -- the caller guarantees that `mask` (still needed by the large-batch path) equals it.  M <= 128 rows run on
 * the weight-streaming kernels of gnf_linear.hip (no mask stream, no split-K partials), anything else on the tiled GEMM.
 *   fwd:    y  = act(x (W o mask)^T + b)                       relu != 0: act = ReLU
 *   bwd_x:  gx = (g (W o mask)) o [gate > 0]                   g: [M,N]; gate: [M,K] (the layer's input) or NULL
 *   bwd_w:  gW = (g^T a) o mask, gb = column sums of g         a: [M,K]; gb: [N] or NULL
 *   bwd:    bwd_w and bwd_x of one layer (what autograd runs for F.linear when both the weight and the input need a
 *           gradient); at M <= 128, and for tall batches with a narrow output (M >= 2048, N <= 64, K <= 128, no mask:
 *           MNISTCNN.fc2, DAGMLP), the two run in ONE launch.  gxsum ([K] or NULL): the column sums of gx = the bias
 *           gradient of the layer that produced `a`; gnf_linear_gxsum_fused() tells whether it comes out of the same
 *           launch (else: one more pass over gx)
 * ws: >= gnf_linear_ws_bytes(M,N,K) bytes. */
int64_t gnf_linear_ws_bytes(int64_t M, int64_t N, int64_t K);
int gnf_linear_fwd(const float* x, const float* W, const float* b, const float* mask, const float* deg_out,
                   const float* deg_in, int strict, int relu, float* y, int64_t M, int64_t N, int64_t K,
                   float* ws, int64_t ws_bytes, gnf_stream_t stream);
int gnf_linear_bwd_x(const float* g, const float* W, const float* mask, const float* deg_out, const float* deg_in,
                     int strict, const float* gate, float* gx, int64_t M, int64_t N, int64_t K,
                     float* ws, int64_t ws_bytes, gnf_stream_t stream);
int gnf_linear_bwd_w(const float* g, const float* a, const float* mask, const float* deg_out, const float* deg_in,
                     int strict, float* gW, float* gb, int64_t M, int64_t N, int64_t K,
                     float* ws, int64_t ws_bytes, gnf_stream_t stream);
int gnf_linear_bwd(const float* g, const float* W, const float* a, const float* mask, const float* deg_out,
                   const float* deg_in, int strict, const float* gate, float* gx, float* gW, float* gb, float* gxsum,
                   int64_t M, int64_t N, int64_t K, float* ws, int64_t ws_bytes, gnf_stream_t stream);
int gnf_linear_gxsum_fused(int64_t M, int64_t N, int64_t K, int masked);

/* ---- fp32 MFMA GEMM with fused masks / bias / ReLU ------------------------------------
 * Replaces F.linear(input, mask*weight, bias) (AutoregressiveConditioner.py:24-25), the
 * nn.Linear+ReLU chains of CouplingMLP / DAGMLP / MNISTCNN.fc* and their autograd
 * backward.  C[m,n] = epi( sum_k A[m,k] * (B[k,n] * Bmask[k,n]) ):
 *   A[m,k] at m*sam + k*sak;  B and Bmask (NULL = none) at k*sbk + n*sbn;
 *   epi: + bias[n] (NULL = none);  * Cmask[m*scmm + n*scmn] (NULL = none);
 *        relu if flags&GNF_GEMM_RELU;  * (gate[m*sgm + n*sgn] > 0) (NULL = none);
 *   C[m,n] at m*scm + n*scn.  v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fma chain. */
#define GNF_GEMM_RELU 1
/* Optional split-K workspace: when gnf_gemm_ws_bytes(M,N,K) > 0 and `ws` holds at least
 * that many bytes, K is spread over several workgroups (few output tiles, long K: the
 * weight-gradient shapes) and a second kernel reduces the partials and applies the
 * epilogue.  ws == NULL always selects the single-pass kernel. */
/* name of the kernel family the most recent gnf_gemm (or Linear entry point routed through it) of the calling thread
 * dispatched to -- "gemm_tall_k", "gemm_wide_k", "gemm_kmajor_k", "gemm_vec_k<128,128>", ...: measurement and tests only. */
const char* gnf_gemm_last_kernel(void);
int64_t gnf_gemm_ws_bytes(int64_t M, int64_t N, int64_t K);
/* the share of gnf_gemm_ws_bytes the fp32-MFMA kernels' split-K partials need: a workspace of exactly this size keeps a call on
 * the fp32 kernels (measurement / tests) where the full size also admits the split-bf16 kernels below */
int64_t gnf_gemm_f32_ws_bytes(int64_t M, int64_t N, int64_t K);
int gnf_gemm(const float* A, int64_t sam, int64_t sak,
             const float* B, const float* Bmask, int64_t sbk, int64_t sbn,
             float* C, int64_t scm, int64_t scn,
             const float* bias,
             const float* Cmask, int64_t scmm, int64_t scmn,
             const float* gate, int64_t sgm, int64_t sgn,
             int flags, int64_t M, int64_t N, int64_t K, float* ws, int64_t ws_bytes, gnf_stream_t stream);

/* ---- the same product on the bf16 matrix pipe with fp32 accuracy (round 6; models/MLP.py:44 and its autograd) ---------
 * Every fp32 operand is split exactly into three bf16 numbers (hi + mid + lo, round-to-nearest at each level) on its way
 * into LDS; a product is the sum of its six leading cross terms (hi hi | hi mid, mid hi | hi lo, lo hi, mid mid), each exact
 * in the fp32 accumulator of v_mfma_f32_16x16x32_bf16; `classes` = 1 / 2 / 3 accumulators per output tile of the GENERAL
 * kernel (3: the magnitude classes are summed separately and added once at the end; measurement), `classes` = 0: the
 * product's choice -- a dedicated kernel (gnf_gemm_split_last_kernel names it) when the shape has one and `ws` holds
 * gnf_gemm_split_ws_bytes(M, N, K) bytes (pre-split fragment-major planes of the small operand / split-K partials).  C[m,n] = epi(sum_k A[m,k] B[k,n]), epi = + bias[n], relu.
 * splits > 1: K is cut into `splits` ranges, partial z goes to C + z * c_split_stride (no epilogue; the caller adds them).
 * Operands must be finite (inf * 0 cross terms would give NaN where an fp32 product gives inf).
 * Measured against the fp32-MFMA kernels and an fp64 product: profiles/r06_split_bf16_error.txt. */
int64_t gnf_gemm_split_ws_bytes(int64_t M, int64_t N, int64_t K);
const char* gnf_gemm_split_last_kernel(void);
/* 1 unless the environment holds GNF_TRUE_F32=1: gnf_gemm (and the Linear entry points routed through it) then never leave the
 * v_mfma_f32_* kernels. */
int gnf_gemm_split_enabled(void);
int gnf_gemm_split_bf16(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
                        float* C, int64_t scm, int64_t scn, const float* bias, int relu,
                        int64_t M, int64_t N, int64_t K, int classes, int splits, int64_t c_split_stride,
                        void* ws, int64_t ws_bytes, gnf_stream_t stream);

/* ---- DAG conditioner gate: models/Conditionners/DAGConditioner.py:94-166 --------------
 * e[(b*d+i)*ld_e + j] = x[b,j] * gate(importance(A[i,j])) (+ one-hot of i in columns
 * d..2d-1 when hot != 0, ld_e >= 2d).
 *   imp_mode 0: raw A (DAG:151-153)  1: soft threshold 2(sigmoid(2A^2)-.5) (:118-119)
 *            2: soft * (soft > h_thresh)  3: A^2 * (A^2 > h_thresh)   (:121-124)
 *   gate_mode 0: deterministic x*imp   1: Gumbel-softmax gate (:95-103)
 *             2: noise gate imp*(x + n*|1-imp|) (:114-116)
 * Randomness: if u1 != NULL the uniforms (gate 1: u1,u2; gate 2: u1 holds N(0,1)
 * samples) are read from [B,d,d] arrays (parity tests); otherwise a Philox4x32-10
 * stream keyed by (seed, offset) is used -- counter = (b*d+i)*ceil(d/4) + j/4, one call
 * serving the four adjacent columns 4(j/4) .. 4(j/4)+3 -- and the backward regenerates the
 * same numbers from the same (seed, offset). */
/* ws: >= gnf_dag_gate_fwd_ws_bytes(d) bytes (per-(i,j) table of importance / gate constants). */
int64_t gnf_dag_gate_fwd_ws_bytes(int64_t d);
int gnf_dag_gate_fwd(const float* x, const float* A, float* e, int64_t ld_e,
                     int imp_mode, int gate_mode, float h_thresh, float temperature,
                     const float* u1, const float* u2, uint64_t seed, uint64_t offset,
                     int hot, float* ws, int64_t B, int64_t d, gnf_stream_t stream);
/* ge: [(B*d), ld_e].  gA: [d,d] (written, not accumulated) or NULL; gx: [B,d] or NULL.
 * tab_fwd: the workspace the matching gnf_dag_gate_fwd call was given, if the caller kept it intact (its first
 * gnf_dag_gate_fwd_ws_bytes(d) bytes hold the per-(i,j) table of the same A and gate settings), else NULL = recomputed.
 * ws: >= gnf_dag_gate_bwd_ws_bytes(B,d). */
int64_t gnf_dag_gate_bwd_ws_bytes(int64_t B, int64_t d);
int gnf_dag_gate_bwd(const float* x, const float* A, const float* ge, int64_t ld_e,
                     int imp_mode, int gate_mode, float h_thresh, float temperature,
                     const float* u1, const float* u2, uint64_t seed, uint64_t offset, const float* tab_fwd,
                     float* gA, float* gx, float* ws, int64_t B, int64_t d, gnf_stream_t stream);

/* ---- structural zeros of the gate backward (round 5) --------------------------------------------------------------
 * dL/dA[i,j] = dP/dA[i,j] * sum_b dL/de[b,i,j] x[b,j] dgate/dP (DAGConditioner.py:118-119: dP/dA = 8 A s(1-s) is
 * EXACTLY zero wherever A is zero -- 97.2 % of MNIST_A_prior(28, 2), NormalizingFlowFactories.py:35-46), so with no
 * gradient wanted for x the cotangent of e is only needed at the columns j of row i with dP/dA[i,j] != 0.
 *   plan (gnf_dag_gate_plan_bytes(d) bytes, written by gnf_dag_gate_fwd_plan from the very table its gate uses):
 *     int32 count[d] (columns with dP/dA != 0 in row i, also when more than GNF_DAG_PLAN_KC),
 *     int16 cols[d][GNF_DAG_PLAN_KC] (those columns in ascending order, -1 padded),
 *     int32 overflow (1 when some count exceeds GNF_DAG_PLAN_KC).
 *   Consumers (gnf_mnistcnn_conv_bwd_cols, gnf_dag_gate_bwd_cols) use the lists only if overflow == 0 and run
 *   their dense code otherwise; the decision is taken on the device, nothing is cached on the host.
 *   ge_cols [(B*d), GNF_DAG_PLAN_KC]: ge_cols[(b*d+i)*KC + k] = dL/de[b,i,cols[i][k]] for k < count[i].
 * gnf_dag_gate_fwd_plan = gnf_dag_gate_fwd that also writes the plan (plan == NULL: exactly gnf_dag_gate_fwd).
 * gnf_dag_gate_bwd_cols: gA only (x frozen), no one-hot columns (ld_e = d); tab_fwd (required) = the forward's ws;
 *   ge [(B*d), d] is read when the plan overflows, ge_cols otherwise; accumulate != 0: gA += (A's other contribution, the
 *   acyclicity term's, is already there: no separate add launch). */
#define GNF_DAG_PLAN_KC 32
int64_t gnf_dag_gate_plan_bytes(int64_t d);
int gnf_dag_gate_fwd_plan(const float* x, const float* A, float* e, int64_t ld_e,
                          int imp_mode, int gate_mode, float h_thresh, float temperature,
                          const float* u1, const float* u2, uint64_t seed, uint64_t offset,
                          int hot, float* ws, int32_t* plan, int64_t plan_bytes, int64_t B, int64_t d,
                          gnf_stream_t stream);
int64_t gnf_dag_gate_bwd_cols_ws_bytes(int64_t B, int64_t d);
int gnf_dag_gate_bwd_cols(const float* x, const float* ge, const float* ge_cols, const int32_t* plan,
                          int imp_mode, int gate_mode, float temperature,
                          const float* u1, const float* u2, uint64_t seed, uint64_t offset, const float* tab_fwd,
                          float* gA, int accumulate, float* ws, int64_t B, int64_t d, gnf_stream_t stream);

/* ---- DAG acyclicity + l1 term: DAGConditioner.get_power_trace / loss (DAGConditioner.py:176-194, 268-271) --------
 * The d x d matrix power stays on the GEMM library; these entries fuse the ~40 elementwise / reduction
 * launches around it.  alpha, lambd, c, dag_const, l1_weight: device scalars (the conditioner's buffers).
 *   prep:  Bm = I + min(1, alpha) * alpha_factor * A o A                                 (:184-190)
 *   value: out4 = [loss, h, coef, l1/d^2] with h = tr(Bm^k) - d = sum_ij P_ij Bm_ji - d, P = Bm^(k-1) (NULL when k = 0),
 *          loss = dag_const (lambd h + c/2 h^2) + l1 mean|A|, coef = dag_const (lambd + c h) k 2 alpha_eff.
 *          ws: >= 2 * 256 floats.
 *   bwd:   gA = g (coef A o P^T + l1/d^2 sign(A))  with g the device scalar d/d loss.       (written, not accumulated) */
int gnf_dag_loss_prep(const float* A, const float* alpha, float alpha_factor, float* Bm, int64_t d, gnf_stream_t stream);
int gnf_dag_loss_value(const float* A, const float* Bm, const float* P, const float* alpha, float alpha_factor,
                       const float* lambd, const float* c, const float* dag_const, const float* l1_weight, int k,
                       float* out4, float* ws, int64_t d, gnf_stream_t stream);
int gnf_dag_loss_bwd(const float* A, const float* P, const float* out4, const float* g, float* gA, int64_t d,
                     gnf_stream_t stream);

/* ---- Monotonic (UMNN) normalizer: models/Normalizers/MonotonicNormalizer.py:21-83 -----
 * Integrand net: Linear(1+c,H1) ReLU ... Linear(H_last,1) ELU+1.05 evaluated on rows
 * (x[b,i], h[b,i,:]).  `nl` = number of Linear layers (>= 2); W[l]: [out_l,in_l]
 * row-major, b[l]: [out_l]; dims[0]=1+c, dims[l+1]=out_l, dims[nl]=1.
 *   z   = h[..,0] + (xT/2) * sum_k cc_w[k] f(xT (cc_t[k]+1)/2 ; h),  xT = S*(x/S)
 *   jac = f(x; h)
 * cc_w, cc_t: S+1 device floats (host-built Clenshaw-Curtis rule; UMNN 1.0's
 * construction, see oracle/gnf_oracle.py: parity unpinned).  n = B*d elements; element
 * e=(b,i): x[e], h at b*h_sb + i*h_sd + c*h_sc with b=e/d, i=e%d.
 * pack: >= gnf_monotonic_pack_floats(...) floats of workspace holding the padded weight
 * image (written by gnf_monotonic_pack, read by fwd/bwd/inv of the same step). */
#define GNF_MONO_MAX_LAYERS 8
typedef struct {
  int nl;                                   /* number of Linear layers */
  int dims[GNF_MONO_MAX_LAYERS + 1];
  const float* W[GNF_MONO_MAX_LAYERS];
  const float* b[GNF_MONO_MAX_LAYERS];
} gnf_mono_net;

int64_t gnf_monotonic_pack_floats(const gnf_mono_net* net);
int gnf_monotonic_pack(const gnf_mono_net* net, float* pack, gnf_stream_t stream);
int gnf_monotonic_fwd(const float* pack, const gnf_mono_net* net,
                      const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                      const float* cc_w, const float* cc_t, int S,
                      float* z, float* jac, int64_t B, int64_t d, gnf_stream_t stream);
/* Wide integrand nets (hidden widths 97..112, 145..160: the [100]^3 / [150]^3 nets of UCIExperiments.yml) and the peeled
 * narrow nets (all hidden widths equal, 49..51: the reference's default [50, 50, 50]) run their hidden->hidden products on
 * the bf16 matrix pipe with exact 3 x bf16 operand splits, six cross terms and fp32 accumulation (as close to an fp64
 * evaluation as the fp32-MFMA kernels or closer, tests/test_gpu_mono_split.py).  GNF_TRUE_F32=1 (read once per process)
 * selects the fp32-MFMA kernels for gnf_monotonic_fwd; gnf_monotonic_fwd_f32 always does (same arguments: the A/B handle
 * of the tests and tools).  gnf_monotonic_fwd_kernel(): name of the kernel family the last forward call of this PROCESS
 * launched ("mono_fwd_wide_split_k", "mono_fwd_wide_k", "mono_fwd_x_k<split>", "mono_fwd_k"); reporting only, not
 * synchronised. */
int gnf_monotonic_fwd_f32(const float* pack, const gnf_mono_net* net,
                          const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                          const float* cc_w, const float* cc_t, int S,
                          float* z, float* jac, int64_t B, int64_t d, gnf_stream_t stream);
const char* gnf_monotonic_fwd_kernel(void);
/* 20-step bisection on [-20,20] with the quadrature inside (MonotonicNormalizer.py:69-83). */
int gnf_monotonic_inv(const float* pack, const gnf_mono_net* net,
                      const float* z, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                      const float* cc_w, const float* cc_t, int S,
                      float* x, int64_t B, int64_t d, gnf_stream_t stream);
/* The same inverse with a strided / scattered result: element (b, j) of the [B, d] problem is written to
 * x[x_row_off[b] + j * x_sd] (x_row_off [B] int32 on the device, element offsets).  The level-scheduled inversion of a DAG flow
 * (NormalizingFlow.py:98-107 restated per topological level) solves a [level rows, batch] problem whose result belongs in
 * columns rows[.] of the [batch, d] sample: x_row_off = rows, x_sd = d -- no transposing copy, no index_put launch. */
int gnf_monotonic_inv_scatter(const float* pack, const gnf_mono_net* net,
                              const float* z, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                              const float* cc_w, const float* cc_t, int S,
                              float* x, const int32_t* x_row_off, int64_t x_sd, int64_t B, int64_t d, gnf_stream_t stream);
/* Which kernel the inverse runs.  gnf_monotonic_inv_route(): the route gnf_monotonic_inv / _inv_scatter would take for this
 * net, S and [B, d] problem, as one line in buf (len bytes, NUL included; too short: GNF_EINVAL):
 *   "<family><<template arguments>> block=<workgroup size> grid=<workgroups> lds=<dynamic LDS bytes>", e.g.
 *   "mono_inv_split_k<HT=2,WM=1,EPG=4> block=192 grid=9 lds=9104" -- families and arguments: mono_fwd_k<HT,WM,INV>,
 *   mono_fwd_x_k<HM,EX,WM,INV>, mono_inv_ks_x_k<HM,EX,epg,waves>, mono_inv_split_x_k<HM,EX,WM,EPG>, mono_inv_split_k<HT,WM,EPG>
 *   (DESIGN.md section 6 has the table of conditions).  Host arithmetic only: nothing is launched, no device pointer is read
 *   (net->W / net->b may be NULL); GNF_ESHAPE / GNF_EINVAL for the nets and S / B / d the entry points refuse with them; an
 *   empty batch gives the empty line.
 * gnf_monotonic_inv_kernel(): the same line for the last inverse launch of this PROCESS ("" before the first); reporting
 *   only, not synchronised.  The returned buffer is rewritten by the next call. */
int gnf_monotonic_inv_route(const gnf_mono_net* net, int S, int64_t B, int64_t d, char* buf, int len);
const char* gnf_monotonic_inv_kernel(void);
/* Backward with UMNN's conventions: gx = gz*f(x;h) + gjac*df/dx(x;h) (Leibniz rule);
 * gh, gW, gb = quadrature of df/dh, df/dtheta weighted by gz*xT/2, plus the gjac path,
 * plus gz on h[..,0].  gW[l]/gb[l] are WRITTEN (same shapes as W[l]/b[l]).
 * gh[e,c] at b*g_sb + i*g_sd + c*g_sc.  ws: >= gnf_monotonic_bwd_ws_bytes(...) bytes. */
int64_t gnf_monotonic_bwd_ws_bytes(const gnf_mono_net* net, int S, int64_t B, int64_t d);
int gnf_monotonic_bwd(const float* pack, const gnf_mono_net* net,
                      const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                      const float* cc_w, const float* cc_t, int S,
                      const float* gz, const float* gjac,
                      float* gx, float* gh, int64_t g_sb, int64_t g_sd, int64_t g_sc,
                      float* const* gW, float* const* gb,
                      void* ws, int64_t ws_bytes, int64_t B, int64_t d, gnf_stream_t stream);
/* Wide integrand nets (H = 145..160): the chain wavefronts of the backward (recompute and data gradient through the
 * hidden->hidden layers) run on the bf16 matrix pipe with exact 3 x bf16 splits, like gnf_monotonic_fwd; peeled narrow nets
 * (H = 49..51, at most three hidden layers): the same for the 48 x 48 main blocks.  The weight-gradient contraction stays
 * fp32 MFMA.  GNF_TRUE_F32=1 / gnf_monotonic_bwd_f32 (same arguments): all fp32 MFMA.  gnf_monotonic_bwd_kernel(): the
 * chain kernel the last backward call of this PROCESS launched (autograd calls from its own thread): "mono_bwd_wide_k<split>",
 * "mono_bwd_wide_k<f32>", "mono_bwd_pair_x_k<split>", "mono_bwd_k". */
int gnf_monotonic_bwd_f32(const float* pack, const gnf_mono_net* net,
                          const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc,
                          const float* cc_w, const float* cc_t, int S,
                          const float* gz, const float* gjac,
                          float* gx, float* gh, int64_t g_sb, int64_t g_sd, int64_t g_sc,
                          float* const* gW, float* const* gb,
                          void* ws, int64_t ws_bytes, int64_t B, int64_t d, gnf_stream_t stream);
const char* gnf_monotonic_bwd_kernel(void);

/* ---- MADE prefix evaluation: inverting an autoregressive step column by column (round 7) -------------------------------
 * NormalizingFlowStep.invert (reference NormalizingFlow.py:98-107) runs d fixed-point passes, each a full MADE forward
 * (AutoregressiveConditioner.py:28-109) and a full normalizer inverse, for ONE new column per pass.  By the MADE's degree
 * rule a hidden unit of degree m is final once the variables of degree 0..m are known, so step t needs only the hidden
 * units of degree t-1 (from the final units below them) and the `out` outputs of the variable of degree t.
 *   net: nh hidden layers of width[l]; W[l] / b[l], l = 0..nh, in nn.Linear layout (W[nh]: [out*d, .], output neuron of
 *     component c of variable v at c*d + v); the plan tables (device, int32): order[l] [width[l]] = the units of layer l in
 *     a stable sort by degree, off[l] [d+1] with off[l][t] = number of units of degree < t, var_of_step [d] = the variable
 *     of degree t; max_new (host) = the largest number of units of one degree in a layer.  The masks are NOT read: the
 *     caller guarantees that they are the degree rule (<= between layers, < into the output layer).
 *   pack: >= gnf_made_prefix_pack_floats(net) floats, written by gnf_made_prefix_pack (weights and biases in degree order;
 *     parameter-only, valid until a parameter or the ordering changes).
 *   gnf_made_prefix runs steps t0 <= t < t1 for B rows:
 *     GNF_MADE_NORM_NONE   (t1 == t0 + 1): h_out[b, c] (B x out, contiguous) = the outputs of variable var_of_step[t0]; the
 *       caller inverts that column, writes x[:, var_of_step[t0]] and calls again with t0 + 1;
 *     GNF_MADE_NORM_AFFINE (out >= 2): x[b, v] = (z[b, v] - clamp(h0, -5, 5)) / exp(clamp(h1, -5, 2)) per step, as
 *       gnf_affine_inv computes it; (t0, t1) = (0, d) is the whole inversion of an Affine + MADE step in one launch.
 *   z, x: [B, d] contiguous; columns of x of degree < t0 are read, the others written (AFFINE) or left alone (NONE).
 *   ws: >= gnf_made_prefix_ws_bytes(net, B) bytes carrying the activations from one call to the next (the SAME buffer for
 *     every call of one inversion, steps in ascending order from 0); may be NULL for (0, d) calls whose tile fits in LDS,
 *     GNF_EWS tells otherwise.  Values are those of the passes up to fp32 summation order.
 *   Conditional MADE (ConditionnalMADE, cond_in = c > 0): the gnf_made_prefix_ctx_* entry points take the same descriptor
 *     with W[0] as [rows, c + d] -- the c context columns in FRONT of the variables, input degree -1, so every unit of the
 *     first layer reads them from step 0 on -- and context [B, c] contiguous (dword-aligned rows, nothing more is assumed).
 *     The activation row becomes [context | x in degree order | hidden 0 | ...], the first layer's prefix at step t is
 *     K = c + t, and pack / ws grow accordingly (first-layer pitch round_up(c + d, 16); ws = 4 B ((c + d + sum width) | 1)
 *     bytes).  Without hidden layers the outputs of the degree-0 variable read the context (K = c at step 0); with hidden
 *     layers they stay the output bias.  The context is read by the launch that runs step 0 (and by a whole inversion held
 *     in LDS); later step launches find it in ws.  cond_in > 2^26: GNF_ESHAPE.  cond_in < 0, or cond_in > 0 with context == NULL and rows to compute:
 *     GNF_EINVAL.  The four entry points without _ctx ARE the cond_in = 0 calls of these (same bits). */
#define GNF_MADE_MAX_HIDDEN 8
#define GNF_MADE_NORM_NONE 0
#define GNF_MADE_NORM_AFFINE 1
typedef struct {
  int nh;                                   /* number of hidden layers (0..GNF_MADE_MAX_HIDDEN) */
  int d, out;                               /* variables; conditioner outputs per variable */
  int max_new;
  int width[GNF_MADE_MAX_HIDDEN];
  const float* W[GNF_MADE_MAX_HIDDEN + 1];
  const float* b[GNF_MADE_MAX_HIDDEN + 1];
  const int32_t* order[GNF_MADE_MAX_HIDDEN];
  const int32_t* off[GNF_MADE_MAX_HIDDEN];
  const int32_t* var_of_step;
} gnf_made_net;
int64_t gnf_made_prefix_pack_floats(const gnf_made_net* net);
int gnf_made_prefix_pack(const gnf_made_net* net, float* pack, gnf_stream_t stream);
int64_t gnf_made_prefix_ws_bytes(const gnf_made_net* net, int64_t B);
int gnf_made_prefix(const gnf_made_net* net, const float* pack, const float* z, float* x, float* h_out, int t0, int t1,
                    int normalizer_mode, int64_t B, void* ws, int64_t ws_bytes, gnf_stream_t stream);
int64_t gnf_made_prefix_ctx_pack_floats(const gnf_made_net* net, int cond_in);
int gnf_made_prefix_ctx_pack(const gnf_made_net* net, int cond_in, float* pack, gnf_stream_t stream);
int64_t gnf_made_prefix_ctx_ws_bytes(const gnf_made_net* net, int cond_in, int64_t B);
int gnf_made_prefix_ctx(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* z,
                        float* x, float* h_out, int t0, int t1, int normalizer_mode, int64_t B, void* ws, int64_t ws_bytes,
                        gnf_stream_t stream);
/* The same two entry points with a third mode: GNF_MADE_NORM_SPLINE (out >= 3 spline_bins - 1, else GNF_ESHAPE; bins and
 * tail as for gnf_spline_inv, else GNF_EINVAL) inverts column var_of_step[t] per step with the arithmetic of gnf_spline_inv
 * on the step's outputs; (0, d) is the whole inversion of a Spline + MADE step in one launch.  NONE / AFFINE: the calls
 * above (spline_bins / spline_tail ignored).  gnf_made_prefix and gnf_made_prefix_ctx themselves refuse the new mode. */
#define GNF_MADE_NORM_SPLINE 2
int gnf_made_prefix_spline(const gnf_made_net* net, const float* pack, const float* z, float* x, float* h_out, int t0, int t1,
                           int normalizer_mode, int spline_bins, double spline_tail, int64_t B, void* ws, int64_t ws_bytes,
                           gnf_stream_t stream);
int gnf_made_prefix_ctx_spline(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* z,
                               float* x, float* h_out, int t0, int t1, int normalizer_mode, int spline_bins, double spline_tail,
                               int64_t B, void* ws, int64_t ws_bytes, gnf_stream_t stream);
/* gnf_made_prefix_ctx_spline with a pin table: the column sweep of an intervention do(x_P = v)
 * (NormalizingFlowStep.intervene).  pin: [d] bytes on the device, one per VARIABLE (not per step), non-zero = pinned; any
 * address (bytes are read one by one).  pin == NULL IS gnf_made_prefix_ctx_spline: the same kernel, the same bits.
 *   A pinned step t (v = var_of_step[t], pin[v] != 0) READS x[b, v], which the caller filled before the call, as the
 *   input of the later steps; it writes neither x nor h_out and computes neither the outputs of v nor its inverse (z[b, v]
 *   is not read).  The hidden units of degree t - 1 are computed as ever: later columns need them.  An un-pinned step is
 *   the step of the entry points above.  (0, d) calls, with the tile in LDS or through ws, take pins like any other.
 *   GNF_MADE_NORM_NONE: t1 > t0 + 1 is allowed when every step of [t0, t1 - 1) is pinned: the launch advances through the
 *   run and writes h_out for step t1 - 1 alone -- nothing when that step is pinned as well.  An un-pinned step inside the
 *   run is GNF_EINVAL.  That check lives HERE, not with the caller: this one form of the call copies the table and the
 *   run's var_of_step entries to the host and waits for the stream (so it cannot be captured into a graph); every other
 *   form is asynchronous as before.  Step launches still load x[:, var_of_step[t0 - 1]] into ws, pinned or inverted.
 *   h_out (NONE) and z (AFFINE / SPLINE) must be non-NULL as above even when every step of the call is pinned; B == 0 or
 *   t1 == t0 returns 0 before any pointer is dereferenced -- except that NONE with t1 > t0 + 1 and pin == NULL is
 *   GNF_EINVAL whatever B (the refusal of the entry points above, which comes first); pin != NULL with B > 0 and
 *   x == NULL is GNF_EINVAL. */
int gnf_made_prefix_do(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* z, float* x,
                       float* h_out, int t0, int t1, int normalizer_mode, int spline_bins, double spline_tail,
                       const uint8_t* pin /* [d], by VARIABLE, device */, int64_t B, void* ws, int64_t ws_bytes,
                       gnf_stream_t stream);

/* ---- StrADE level sweep: inverting a masked net over a GIVEN DAG level by level (StrADEConditioner) --------------------
 * The prefix kernel's idea with "degree" replaced by "topological level": a MADE whose masks encode an arbitrary DAG
 * (models/Conditionners/StrADEConditioner.py: strade_masks) assigns every hidden unit a parent set; the unit's level is the
 * largest level of a variable in its set (-1 for the empty set) and it is FINAL once the variables of the levels up to its
 * own are known.  Level t of the sweep computes, layer by layer, the hidden units of level t - 1 from the units of level
 * < t below them, then the outputs of EVERY variable of level t, inverts those variables and hands them on.  Units and
 * variables are kept in LEVEL order, so "every unit of level < t" is a contiguous K range; inside that range the entries
 * the mask forbids are exact zeros of the weight image, which gnf_strade_pack writes as mask ? W : 0.
 *   net->made: the descriptor of gnf_made_prefix with the tables read by LEVEL: order[l] [width[l]] = the units of layer l
 *     in a stable sort by level, off[l] [nlev + 1] with off[l][t] = number of units of level < t (the empty-set units
 *     count from t = 0 on), var_of_step [d] = the variables in a stable sort by level, max_new = the largest number of
 *     units of one level (the last excepted) in a layer.
 *   mask[l], l = 0..nh: the fp32 0/1 masks in the layout of W[l]; read by gnf_strade_pack alone.
 *   var_off [nlev + 1] (device, int32): var_off[t] = number of variables of level < t; nlev = depth + 1 levels,
 *     1 <= nlev <= d; widest (host) = the largest number of variables of one level.
 *   pack: >= gnf_strade_pack_floats(net, cond_in) floats, 16-byte aligned (else GNF_EINVAL), written by gnf_strade_pack;
 *     parameter-only, valid until a parameter, a mask or the graph changes.
 *   gnf_strade_levels: the whole inversion of B rows in ONE launch, the tile's activation rows
 *     [context | x in level order | hidden 0 | ...] in LDS only (no workspace).  z, x [B, d] and context [B, cond_in]
 *     contiguous, dword-aligned rows, nothing more is assumed.  normalizer_mode: GNF_MADE_NORM_AFFINE (out >= 2) or
 *     GNF_MADE_NORM_SPLINE (out >= 3 spline_bins - 1; bins and tail as for gnf_spline_inv), with the arithmetic of
 *     gnf_affine_inv / gnf_spline_inv; any other mode is GNF_EINVAL.  The outputs of a level are produced in chunks of
 *     GNF_STRADE_CHUNK_VARS variables.
 *   pin: NULL, or [d] bytes on the device, one per VARIABLE, non-zero = pinned (do(x_P = v), as gnf_made_prefix_do): a
 *     pinned variable keeps its level and x[b, v], which the caller filled, is handed on in place of outputs and inverse;
 *     a chunk whose variables are all pinned computes no output product.  pin == NULL is a kernel without that branch.
 *   fp32 with a fixed summation order for a given (net, cond_in, B); no atomics; rows never interact.  B == 0 launches
 *   nothing.  GNF_ESHAPE when a tile of 4 rows does not fit in LDS (160 KB): the caller inverts by passes.  GNF_EINVAL:
 *   a NULL table or operand with rows to compute, nlev outside 1..d, widest outside 1..d, cond_in < 0, B < 0. */
#define GNF_STRADE_CHUNK_VARS 8
typedef struct {
  gnf_made_net made;
  const float* mask[GNF_MADE_MAX_HIDDEN + 1];
  const int32_t* var_off;
  int nlev;
  int widest;
} gnf_strade_net;
int64_t gnf_strade_pack_floats(const gnf_strade_net* net, int cond_in);
int gnf_strade_pack(const gnf_strade_net* net, int cond_in, float* pack, gnf_stream_t stream);
int gnf_strade_levels(const gnf_strade_net* net, int cond_in, const float* context, const float* pack, const float* z,
                      float* x, int normalizer_mode, int spline_bins, double spline_tail,
                      const uint8_t* pin /* [d], by VARIABLE, device, or NULL */, int64_t B, gnf_stream_t stream);

/* ---- MADE adjoint sweep: lambda with J^T lambda = g for one MADE step (NormalizingFlowStep.rsample's backward) ----------
 * The step is z = S(x; context): h = MADE(context, x), z[b, i] = normalizer(x[b, i], h[b, i, :]).  In degree order
 * J = dz/dx = diag(jac) + N with N strictly lower triangular, so J^T lambda = g is solved from the last degree down:
 *   lambda_t = (g[b, v] - u_t) / jac[b, v],  v = var_of_step[t],
 *   u_t = the cotangent that reaches x[b, v] through the MADE when the outputs of every later variable v' = var_of_step[t'],
 *         t' > t, carry the cotangent lambda_t' * dzdh[b, v', :].
 * One launch does the whole solve: it first replays the hidden units from x with the arithmetic (and the tile height) of
 * gnf_made_prefix, keeping the ReLU decisions act > 0 -- those of the column sweep that produced x -- and then walks
 * t = d-1 .. 0, finalising per step the cotangents of the hidden units of degree t (suffix contractions of the transposed
 * weights, the mirror image of the prefix contractions) and u_t.
 *   net, cond_in: as for gnf_made_prefix_ctx (the masks are NOT read: the caller guarantees the degree rule).
 *   pack: >= gnf_made_adjoint_pack_floats(net, cond_in) floats, 16-byte aligned, written by gnf_made_adjoint_pack: the
 *     image of gnf_made_prefix_ctx_pack followed by every layer TRANSPOSED (rows = the units of the layer below in degree
 *     order, pitch = out_features rounded up to 16, the tail zero).  Parameter-only, valid until a parameter or the ordering
 *     changes.
 *   x, g, jac, lambda: [B, d] contiguous; context: [B, cond_in] contiguous (NULL for cond_in = 0); dzdh: [B, d, out]
 *     contiguous, dzdh[b, i, k] = dz[b, i] / dh[b, i, k] (the normalizers are element-wise, so one normalizer backward with
 *     a cotangent of ones yields it whatever the normalizer).  All dword-aligned, nothing more is assumed.  jac != 0.
 *   ws: >= gnf_made_adjoint_ws_bytes(net, cond_in, B) bytes; may be NULL when the tile's rows fit in LDS (160 KB), GNF_EWS
 *     tells otherwise.  force_ws != 0 keeps the rows in ws even when they would fit: the same code on another pointer, the
 *     same bits (a test hook).
 *   fp32 with a fixed summation order for a given (net, cond_in, B); rows never interact.  B = 0 launches nothing. */
int64_t gnf_made_adjoint_pack_floats(const gnf_made_net* net, int cond_in);
int gnf_made_adjoint_pack(const gnf_made_net* net, int cond_in, float* pack, gnf_stream_t stream);
int64_t gnf_made_adjoint_ws_bytes(const gnf_made_net* net, int cond_in, int64_t B);
int gnf_made_adjoint(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* x,
                     const float* g, const float* jac, const float* dzdh, float* lambda, int64_t B, int force_ws, void* ws,
                     int64_t ws_bytes, gnf_stream_t stream);
/* ... under an intervention do(x_P = v) (NormalizingFlowStep.rsample_do's backward).  The equations of the free set F are
 * kept, those of the pinned set P become x_P = v, so lambda_P = 0, lambda_F solves J_FF^T lambda_F = g_F, and
 * dL/dv = g_P - (N^T lambda)_P.  In the sweep, at a pinned step t: u_t as above, lambda_t := 0, gdo_t := g_t - u_t, and the
 * cotangent row of the variable's outputs is exact zeros -- all by SELECTION: jac[b, v] and dzdh[b, v, :] of a pinned v are
 * never read and may hold 0, inf or NaN.
 *   pin: [d] bytes on the device, one per VARIABLE (not per step), non-zero = pinned; any address, read byte by byte (the
 *     table of gnf_made_prefix_do).  NULL: the call above, the same kernel, the same bits; then gdo must be NULL too
 *     (GNF_EINVAL otherwise).  An all-zero table gives those bits as well.
 *   gdo: [B, d] contiguous, dword-aligned, or NULL.  lambda is written everywhere: lambda at free columns, +0 at pinned
 *     ones; gdo, when given, likewise: g - u at pinned columns, +0 at free ones.
 *   Skipped, because the table makes it dead: with t_last the last free step (derived from the table inside the kernel),
 *   the steps t > t_last have u = 0 exactly and run no contraction (lambda = 0, gdo = g), and the replay stops at the hidden
 *   units of degree t_last - 1; every variable pinned runs no layer step at all; with gdo == NULL a pinned step skips the
 *   first-layer contraction behind its u.  ws: gnf_made_adjoint_ws_bytes, as above.  Everything else as above. */
int gnf_made_adjoint_do(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* x,
                        const float* g, const float* jac, const float* dzdh, float* lambda,
                        const uint8_t* pin /* [d], by VARIABLE, device, or NULL */, float* gdo /* [B, d] or NULL */,
                        int64_t B, int force_ws, void* ws, int64_t ws_bytes, gnf_stream_t stream);

/* ---- StrADE adjoint sweep: lambda with J^T lambda = g for one StrADE step (rsample's backward, adjoint_levels) -----------
 * gnf_made_adjoint with "degree" replaced by "topological level", on the tables of gnf_strade_levels.  In level order
 * J = dz/dx = diag(jac) + N with N[p'][p] != 0 only where the level of p' is above the level of p, so J^T lambda = g is
 * solved from the last level down, a whole level at once:
 *   lambda[b, v] = (g[b, v] - u) / jac[b, v],  v = var_of_step[p], var_off[t] <= p < var_off[t + 1],
 *   u = the cotangent that reaches x[b, v] through the masked net when the outputs of every variable v' of a later level
 *       carry the cotangent lambda[b, v'] * dzdh[b, v', :].
 * One launch does the whole solve: it first replays the hidden units from x with the arithmetic and the tile height of
 * gnf_strade_levels for the same (net, cond_in, B) (4 rows where that sweep answers GNF_ESHAPE), keeping the ReLU
 * decisions act > 0, and then walks t = nlev-1 .. 0, finalising per level the cotangents of the hidden units of level t
 * (contractions over the suffix [off[l+1][t], width) of the layer above; the suffix start is not the mask: forbidden
 * entries inside it are exact zeros of the image) and u for the level's variables in chunks of GNF_STRADE_CHUNK_VARS.
 *   net, cond_in: as for gnf_strade_levels; the masks are read by gnf_strade_adjoint_pack alone.
 *   pack: >= gnf_strade_adjoint_pack_floats(net, cond_in) floats, 16-byte aligned (else GNF_EINVAL), written by
 *     gnf_strade_adjoint_pack: the image of gnf_strade_pack, bit for bit, followed by every layer TRANSPOSED (layer l as
 *     [in_features][out_features rounded up to 16], the tail zero, a masked entry an exact zero whatever the weight holds).
 *     Parameter-only, valid until a parameter, a mask or the graph changes.
 *   x, g, jac, lambda: [B, d] contiguous; context: [B, cond_in] contiguous (NULL for cond_in = 0); dzdh: [B, d, out]
 *     contiguous, by VARIABLE index, dzdh[b, i, k] = dz[b, i] / dh[b, i, k].  All dword-aligned, nothing more is assumed.
 *     jac != 0.  The normalizer is not named: jac and dzdh are all the kernel knows of it.
 *   ws: >= gnf_strade_adjoint_workspace_bytes(net, cond_in, B) bytes (spelt out, not abbreviated as the other queries are: the
 *     forward sweep of a StrADE net takes no workspace, and tests/test_strade_masks.py pins that by name); may be NULL when the tile's rows
 *     [context | x | hidden ... | d out output cotangents] fit in LDS (160 KB), GNF_EWS tells otherwise -- never GNF_ESHAPE
 *     for want of LDS.  force_ws != 0 keeps the rows in ws even when they would fit: the same code on another pointer,
 *     the same bits (a test hook).
 *   fp32 with a fixed summation order for a given (net, cond_in, B); no atomics; rows never interact.  B == 0 launches
 *   nothing.  GNF_EINVAL: a NULL operand or table with rows to compute, a misaligned pack, B < 0, and what
 *   gnf_strade_levels refuses of a net.  Every check comes before any launch. */
int64_t gnf_strade_adjoint_pack_floats(const gnf_strade_net* net, int cond_in);
int gnf_strade_adjoint_pack(const gnf_strade_net* net, int cond_in, float* pack, gnf_stream_t stream);
int64_t gnf_strade_adjoint_workspace_bytes(const gnf_strade_net* net, int cond_in, int64_t B);
int gnf_strade_adjoint(const gnf_strade_net* net, int cond_in, const float* context, const float* pack, const float* x,
                       const float* g, const float* jac, const float* dzdh, float* lambda, int64_t B, int force_ws, void* ws,
                       int64_t ws_bytes, gnf_stream_t stream);
/* ... under an intervention do(x_P = v): gnf_made_adjoint_do with levels for degrees.  pin ([d] bytes by VARIABLE, device,
 * any address; NULL = the call above, then gdo must be NULL: GNF_EINVAL otherwise) and gdo ([B, d] or NULL) as there:
 * lambda is +0 at pinned columns, gdo is g - u at pinned columns and +0 at free ones, jac and dzdh of a pinned element are
 * never read.  A pinned variable keeps its level.  Skipped: the levels above the last level that holds a free variable
 * (u = 0 exactly: no contraction, and the replay stops below that level; no layer step at all when every variable is
 * pinned), and, with gdo == NULL, the first-layer contraction of a chunk whose variables are all pinned.
 * ws: gnf_strade_adjoint_workspace_bytes, as above. */
int gnf_strade_adjoint_do(const gnf_strade_net* net, int cond_in, const float* context, const float* pack, const float* x,
                          const float* g, const float* jac, const float* dzdh, float* lambda,
                          const uint8_t* pin /* [d], by VARIABLE, device, or NULL */, float* gdo /* [B, d] or NULL */,
                          int64_t B, int force_ws, void* ws, int64_t ws_bytes, gnf_stream_t stream);

/* ---- MNISTCNN convolutional front: models/MLP.py:36-41 as the DAG embedding net --------
 * (ImageExperiments / NormalizingFlowFactories.py:83-86: size_img = [1,28,28]).
 * e: [n_img, 784] masked images; W1 [16,1,3,3], b1 [16], W2 [16,16,3,3], b2 [16].
 * pooled: [n_img, 2304] = flatten(maxpool2(conv2(relu(conv1(e))))) in [16,12,12] order;
 * argmax: [n_img, 2304] bytes, index 0..3 of the first maximum of each 2x2 window in scan
 * order (what torch's max_pool2d records), consumed by the backward.
 * exact_ties = 0: conv2 in the Winograd F(2x2,3x3) domain (2.25x fewer MFMAs); pool windows whose four values are
 *   EXACTLY equal in exact arithmetic (constant image regions: a deterministic gate on a windowed A) are then decided
 *   by rounding noise of the transforms -- an equally valid subgradient, not torch's.
 * exact_ties = 1: conv2 as the direct implicit GEMM: equal patches give bit-equal outputs, the first maximum wins as
 *   in torch.  models.DAGConditioner selects it for deterministic gates that cannot use the sparse front. */
int gnf_mnistcnn_conv_fwd(const float* e, const float* W1, const float* b1, const float* W2, const float* b2,
                          float* pooled, unsigned char* argmax, int64_t n_img, int exact_ties, gnf_stream_t stream);
/* Backward: recomputes conv1, writes ge [n_img,784] and the parameter gradients (written,
 * not accumulated).  ws: >= gnf_mnistcnn_conv_bwd_ws_bytes(n_img) bytes. */
int64_t gnf_mnistcnn_conv_bwd_ws_bytes(int64_t n_img);
int gnf_mnistcnn_conv_bwd(const float* e, const float* W1, const float* b1, const float* W2,
                          const float* g_pooled, const unsigned char* argmax,
                          float* ge, float* gW1, float* gb1, float* gW2, float* gb2,
                          void* ws, int64_t ws_bytes, int64_t n_img, gnf_stream_t stream);
/* The same backward for the masked copies of a DAG conditioner whose gate backward needs the cotangent of e at the plan's
 * columns only (above): image n is the masked copy (b, i) = (n / d_plan, n % d_plan), d_plan = 784.  Unless a row of the
 * plan overflows, ge is NOT written: ge_cols [n_img, GNF_DAG_PLAN_KC] receives dL/de at the row's columns, and the
 * kernel skips the W1^T dpre1 products of the conv1 positions no such column reaches (7 of 11 position groups at the
 * MNIST prior).  The parameter gradients are those of gnf_mnistcnn_conv_bwd, bit for bit.  plan == NULL: that call. */
int gnf_mnistcnn_conv_bwd_cols(const float* e, const float* W1, const float* b1, const float* W2,
                               const float* g_pooled, const unsigned char* argmax,
                               float* ge, const int32_t* plan, int64_t d_plan, float* ge_cols,
                               float* gW1, float* gb1, float* gW2, float* gb2,
                               void* ws, int64_t ws_bytes, int64_t n_img, gnf_stream_t stream);
/* The Winograd pair with the conv1 + ReLU activations kept by the forward instead of recomputed by the backward: the
 * recompute sits on the fp32 ALU that bounds the backward, the stream on a memory system both kernels leave idle.
 * a1save / a1saved: gnf_mnistcnn_conv_a1_bytes(n_img) bytes, 16-byte aligned -- per image [16 channels][730] floats, rows of
 * pitch 28 (the backward's LDS image); columns 26, 27 of every row and the entries 728, 729 of every channel are written as
 * zeros and the backward RELIES on that.  gnf_mnistcnn_conv_fwd_save with a1save == NULL is gnf_mnistcnn_conv_fwd; with
 * exact_ties = 1 (the direct kernel keeps nothing) a1save must be NULL.  The _a1 backwards take the arguments of their
 * namesakes plus a1saved and return the same bits. */
int64_t gnf_mnistcnn_conv_a1_bytes(int64_t n_img);
int gnf_mnistcnn_conv_fwd_save(const float* e, const float* W1, const float* b1, const float* W2, const float* b2,
                               float* pooled, unsigned char* argmax, float* a1save, int64_t n_img, int exact_ties,
                               gnf_stream_t stream);
int gnf_mnistcnn_conv_bwd_a1(const float* e, const float* a1saved, const float* W1, const float* b1, const float* W2,
                             const float* g_pooled, const unsigned char* argmax,
                             float* ge, float* gW1, float* gb1, float* gW2, float* gb2,
                             void* ws, int64_t ws_bytes, int64_t n_img, gnf_stream_t stream);
int gnf_mnistcnn_conv_bwd_cols_a1(const float* e, const float* a1saved, const float* W1, const float* b1, const float* W2,
                                  const float* g_pooled, const unsigned char* argmax,
                                  float* ge, const int32_t* plan, int64_t d_plan, float* ge_cols,
                                  float* gW1, float* gb1, float* gW2, float* gb2,
                                  void* ws, int64_t ws_bytes, int64_t n_img, gnf_stream_t stream);

/* ---- CIFAR10CNN convolutional front: models/MLP.py:66-68 as the DAG embedding net ---------
 * (NormalizingFlowFactories.py:100-135).  feat = flatten(pool2(relu(conv_k(6->16)(pool2(relu(conv_k(C->6)(e)))))))
 * in torch's (channel, row, column) order, 2 x 2 floor pooling, for the geometries the factory builds:
 *   (C, H, W, k) = (3,32,32,5), (1,32,32,3), (1,16,16,3), (1,8,8,2)  ->  gnf_lenet_conv_feat = 400, 576, 64, 16;
 * any other geometry: gnf_lenet_conv_supported = 0 and GNF_ESHAPE from every other call.
 * e: [n_img, C*H*W] rows of pitch ld_e (elements, >= C*H*W; row offsets are 64-bit); W1 [6,C,k,k], b1 [6], W2 [16,6,k,k],
 * b2 [16]; feat: [n_img, F] contiguous.  Decisions are torch's: ReLU passes pre-activations > 0, a pool window takes its
 * FIRST maximum in scan order, always (no exact_ties switch: equal patches give bit-equal sums in this direct form).
 * argmax2 (may be NULL): [n_img, F] bytes, one per feature: 0..3 = the entry of the second pool's window that carries the
 * gradient, 4 = none (the pooled value is 0).  n_img == 0: returns 0 without a launch. */
int gnf_lenet_conv_supported(int C, int H, int W, int k);
int64_t gnf_lenet_conv_feat(int C, int H, int W, int k);
int gnf_lenet_conv_fwd(const float* e, int64_t ld_e, int C, int H, int W, int k,
                       const float* W1, const float* b1, const float* W2, const float* b2,
                       float* feat, unsigned char* argmax2, int64_t n_img, gnf_stream_t stream);
/* Backward: g_feat [n_img, F] -> gW1, gb1, gW2, gb2 (written, not accumulated; zeros for n_img == 0) and, when ge is
 * not NULL, ge [n_img, C*H*W] rows of pitch ld_ge.  conv1 is always recomputed (its pooled activations are an operand of
 * gW2); the second pool's decisions come from the plane the forward wrote, or are recomputed too when argmax2 is NULL --
 * the same bits either way.  Per-workgroup partial gradients go through ws (>= gnf_lenet_conv_bwd_ws_bytes) and are summed
 * in a fixed order: no float atomics, two calls on the same operands return the same bits, with or without ge. */
int64_t gnf_lenet_conv_bwd_ws_bytes(int C, int H, int W, int k, int64_t n_img);
int gnf_lenet_conv_bwd(const float* e, int64_t ld_e, int C, int H, int W, int k,
                       const float* W1, const float* b1, const float* W2, const float* b2,
                       const unsigned char* argmax2, const float* g_feat,
                       float* ge, int64_t ld_ge, float* gW1, float* gb1, float* gW2, float* gb2,
                       void* ws, int64_t ws_bytes, int64_t n_img, gnf_stream_t stream);

/* ---- the same front with the DAG gate fused in: the masked copies are built in LDS ---------------
 * For a DAG conditioner whose embedding net is this front (d = C*H*W, one masked copy per variable) the images are
 *   e[b*d + i, :] = x[b, :] * gate(b, i, :)          exactly the values gnf_dag_gate_fwd writes (hot = 0),
 * and these entry points build them inside the kernels from x [B, d] (contiguous), the gate's (i, j) table and the noise:
 * neither e nor its cotangent ever exists in memory.  imp_mode, gate_mode, h_thresh, temperature, u1, u2 ([B*d, d] injected
 * uniforms, or NULL for Philox with (seed, offset) and counter (b*d + i) * ceil(d/4) + j/4) are those of gnf_dag_gate_fwd.
 * tab: caller-owned, gnf_dag_gate_fwd_ws_bytes(d) bytes; the forward fills it from A (the gate kernels' table), the
 * backward reads it, so the caller keeps it between the two.  feat [B*d, F] and argmax2 (may be NULL) as for
 * gnf_lenet_conv_fwd, rows in the order b*d + i (64-bit row offsets).  Same return codes and the same refusal of
 * pointers below dword alignment as gnf_lenet_conv_*; B == 0: returns 0 without a launch. */
int gnf_lenet_gated_fwd(const float* x, const float* A, float* tab, int C, int H, int W, int k,
                        int imp_mode, int gate_mode, float h_thresh, float temperature,
                        const float* u1, const float* u2, uint64_t seed, uint64_t offset,
                        const float* W1, const float* b1, const float* W2, const float* b2,
                        float* feat, unsigned char* argmax2, int64_t B, gnf_stream_t stream);
/* Backward: g_feat [B*d, F] -> gW1, gb1, gW2, gb2 (written; zeros for B == 0) and, when gA is not NULL, the gate's
 * gradient gA [d, d] = dP/dA * sum_b dL/de[b,i,j] * de/dp[b,i,j] (accumulate != 0: added to what gA holds; B == 0 then
 * leaves it alone).  There is no gradient for x: a caller that needs one composes gnf_dag_gate_* with gnf_lenet_conv_*.
 * The sums over the samples are taken per (row i, chunk of samples) in registers, written to ws and added in chunk
 * order: no float atomics, the same bits on every call.  argmax2 NULL: conv2 is recomputed, the same bits. */
int64_t gnf_lenet_gated_bwd_ws_bytes(int C, int H, int W, int k, int64_t B);
int gnf_lenet_gated_bwd(const float* x, const float* tab, int C, int H, int W, int k,
                        int imp_mode, int gate_mode, float temperature,
                        const float* u1, const float* u2, uint64_t seed, uint64_t offset,
                        const float* W1, const float* b1, const float* W2, const float* b2,
                        const unsigned char* argmax2, const float* g_feat,
                        float* gA, int accumulate, float* gW1, float* gb1, float* gW2, float* gb2,
                        void* ws, int64_t ws_bytes, int64_t B, gnf_stream_t stream);

/* ---- the same front on a subset of the rows of a DETERMINISTIC gate: inversion and evaluation ---------------
 * NormalizingFlowStep.invert asks a DAG conditioner for the rows of one topological level at a time, and deterministic
 * evaluation for all d of them (DAGConditioner.py:142-153): image (b, r) is
 *   x[b, :] * P[i, :],   i = rows[r]   (rows == NULL: i = r, which needs R <= d),
 * one fp32 product per element -- the bits of torch's broadcast x.unsqueeze(1) * P[rows].unsqueeze(0) -- built in LDS: the
 * [B, R, d] tensor (37.7 MB per sample for a level of all roots at d = 3072) never exists in memory.  Forward only, no
 * argmax plane, nothing kept for a backward.
 * x: [B, d] contiguous, d = C*H*W;  P: the importance matrix [d, d], rows of pitch ld_p (elements, >= d);  rows: R device
 * indices in [0, d), any order, repeats allowed, NOT checked by the kernel;  W1, b1, W2, b2 as for gnf_lenet_conv_fwd.
 * feat: [B, R, F] contiguous (row b*R + r), or [R, B, F] (row r*B + b) when variable_major != 0; 64-bit row offsets.
 * GNF_ESHAPE outside the four geometries; GNF_EINVAL for a NULL operand, B < 0, R < 0, R > d with rows == NULL, ld_p < d and
 * pointers below dword alignment (rows included).  B == 0 or R == 0: returns 0 without a launch (x and feat may be NULL). */
int gnf_lenet_rows_fwd(const float* x, const float* P, int64_t ld_p, const int32_t* rows, int64_t R,
                       int C, int H, int W, int k,
                       const float* W1, const float* b1, const float* W2, const float* b2,
                       float* feat, int variable_major, int64_t B, gnf_stream_t stream);

/* Training behind a FROZEN deterministic gate (A fixed by post_process(), P without a gradient): the same copies, forward
 * with the second pool's decisions kept and a backward for the conv parameters and, optionally, x.  Neither the [B, R, d]
 * product nor its cotangent exists in memory.
 * gnf_lenet_rows_fwd_arg: gnf_lenet_rows_fwd plus argmax2 [B*R, F] bytes in the row order of feat (NULL: exactly
 * gnf_lenet_rows_fwd).
 * gnf_lenet_rows_bwd: g_feat (rows as feat, per variable_major) -> gW1, gb1, gW2, gb2 (written, not accumulated) and, when
 * gx is not NULL, gx[b, j] = sum_r P[rows[r], j] * dL/de[b, r, j], [B, d] contiguous (written).  Repeated indices in rows
 * are rows of their own.  argmax2 NULL: conv2 is recomputed, the same bits.  gx NULL: dL/de is not computed at all, the
 * parameter gradients keep their bits.  There is no gradient for P.  The sums over the rows are taken per (chunk of rows,
 * group of samples) in registers, written to ws and added in chunk order: no float atomics, the same bits on every call.
 * ws: >= gnf_lenet_rows_bwd_ws_bytes(C, H, W, k, R, B, gx != NULL) bytes, else GNF_EWS.  Other return codes as
 * gnf_lenet_rows_fwd (gradient outputs and ws must not be NULL).  B == 0 or R == 0: no zero-sized grid is launched; the
 * parameter gradients, and gx when given, are written as zeros. */
int gnf_lenet_rows_fwd_arg(const float* x, const float* P, int64_t ld_p, const int32_t* rows, int64_t R,
                           int C, int H, int W, int k,
                           const float* W1, const float* b1, const float* W2, const float* b2,
                           float* feat, unsigned char* argmax2, int variable_major, int64_t B, gnf_stream_t stream);
int64_t gnf_lenet_rows_bwd_ws_bytes(int C, int H, int W, int k, int64_t R, int64_t B, int want_gx);
int gnf_lenet_rows_bwd(const float* x, const float* P, int64_t ld_p, const int32_t* rows, int64_t R,
                       int C, int H, int W, int k,
                       const float* W1, const float* b1, const float* W2, const float* b2,
                       const unsigned char* argmax2, const float* g_feat, int variable_major,
                       float* gx, float* gW1, float* gb1, float* gW2, float* gb2,
                       void* ws, int64_t ws_bytes, int64_t B, gnf_stream_t stream);

/* ---- DAG gate and one-hot fused into the first layer of a DAGMLP (DAGConditioner.py:7-20, 94-169) ---------------
 * The tabular DAG flows feed the masked copies e[b*d + i, :] = (x[b, :] * gate(b, i, :) | one-hot(i)) to a Linear/ReLU
 * chain.  These entry points compute the first layer on copies built in LDS,
 *   a1[b*d + i, n] = act( b1[n] + [hot] W1[n, d + i] + sum_{j<d} W1[n, j] * x[b, j] * gate(b, i, j) ),
 * act = ReLU (relu != 0) or the identity: neither e nor its cotangent exists in memory, and the one-hot half of the layer
 * is a column of W1 added in the epilogue.  Gate settings, the injected uniforms u1, u2 ([B*d, d]) and the Philox counter
 * ((b*d + i) * ceil(d/4) + j/4) are those of gnf_dag_gate_fwd: the copies have the bits that entry point writes.
 * Domain: 1 <= d <= 64, 1 <= H <= 2^20 (gnf_dagmlp_supported; GNF_ESHAPE from every entry point outside it, nothing is
 * launched), B >= 0.  x [B, d] contiguous; A [d, d] contiguous; W1 [H, >= d (hot: 2 d)] rows of pitch ld_w; b1 [H];
 * a1 and g [B*d, H] contiguous.  tab: caller-owned, gnf_dag_gate_fwd_ws_bytes(d) bytes; the forward fills it from A, the
 * backward reads it.  Any dword address for every array (16-byte alignment selects the 16-byte loads and stores, the
 * summation order is the same).  B == 0: batch-sized pointers may be NULL, no tile kernel is launched (the forward still
 * fills tab), and the backward writes zero parameter gradients. */
int gnf_dagmlp_supported(int64_t d, int64_t H);
int gnf_dagmlp_gated_fwd(const float* x, const float* A, float* tab, int imp_mode, int gate_mode,
                         float h_thresh, float temperature, const float* u1, const float* u2,
                         uint64_t seed, uint64_t offset, const float* W1, int64_t ld_w, const float* b1,
                         int hot, int relu, float* a1, int64_t B, int64_t d, int64_t H, gnf_stream_t stream);
/* Backward: g = dL/da1, ALREADY multiplied by [a1 > 0] when the forward applied the ReLU.  Every output may be NULL:
 *   gx  [B, d]      gx[b, j] = sum_i de[b*d+i, j] * d e / d x  (the gate; P for the deterministic and the noise gate),
 *                   de = g W1[:, :d] kept on chip;
 *   gA  [d, d]      dP/dA * sum_b de * d e / d p   (accumulate != 0: added to what gA holds; B == 0 then leaves it alone);
 *   gW1 [H, ..]     rows of pitch ld_gw: columns [0, d) = g^T e and, with hot, [d, 2 d) = sum_b g[b*d+i, :]; columns behind
 *                   them are not touched;
 *   gb1 [H]         column sums of g.
 * The noise is regenerated; nothing but tab is kept from the forward.  Per-workgroup partial sums go through ws
 * (>= gnf_dagmlp_gated_bwd_ws_bytes(B, d, H) bytes, else GNF_EWS) and are added in workgroup order: no float atomics, the
 * same call returns the same bits. */
int64_t gnf_dagmlp_gated_bwd_ws_bytes(int64_t B, int64_t d, int64_t H);
int gnf_dagmlp_gated_bwd(const float* x, const float* tab, int imp_mode, int gate_mode, float temperature,
                         const float* u1, const float* u2, uint64_t seed, uint64_t offset,
                         const float* W1, int64_t ld_w, int hot, const float* g,
                         float* gx, float* gA, int accumulate, float* gW1, int64_t ld_gw, float* gb1,
                         void* ws, int64_t ws_bytes, int64_t B, int64_t d, int64_t H, gnf_stream_t stream);
/* The same first layer on rows of a DETERMINISTIC gate (inversion by levels, evaluation): copy (b, r) is
 * x[b, :] * P[i, :], i = rows[r] (rows == NULL: i = r, R <= d), one fp32 product per element; with hot the epilogue adds
 * W1[n, d + i].  P [d, d] rows of pitch ld_p; rows: R int32 device indices in [0, d), repeats allowed, not checked.
 * a1: row b*R + r, or r*B + b when variable_major != 0 (64-bit offsets), pitch H.  Forward only, no table.
 * B == 0 or R == 0: returns 0 without a launch. */
int gnf_dagmlp_rows_fwd(const float* x, const float* P, int64_t ld_p, const int32_t* rows, int64_t R,
                        const float* W1, int64_t ld_w, const float* b1, int hot, int relu, float* a1,
                        int variable_major, int64_t B, int64_t d, int64_t H, gnf_stream_t stream);

/* ---- sparse masked-image front for a DETERMINISTIC DAG gate ---------------
 * Replaces, for evaluation / sampling, the chain  e = x * P[i]  (DAGConditioner.py:142-153, deterministic branches)
 * -> conv1/ReLU/conv2/maxpool (MLP.py:36-41) -> fc1 + ReLU (MLP.py:43-44)  when every row i of the importance matrix
 * P [784,784] is zero outside the 5x5 window around pixel i (MNIST_A_prior with kernel 2,
 * NormalizingFlowFactories.py:35-46): only the 14x14 crop around the window is convolved and fc1 contracts the
 * 5x5x16 pooled block that can differ from the constant background (exact, not an approximation).
 *   x [B,784];  pix [R] (device): the masked copies (pixel indices i) to evaluate, SORTED by crop origin
 *   g(i) = 8*o(i/28) + o(i%28), o(p) = clamp(floor((p-6)/2), 0, 7);
 *   groups [2*64] (device): for each origin g the first output row and the number of output rows (= B * number of
 *   pix entries with that origin);  max_group_rows: the largest of those counts (host value, sizes the grid);
 *   W1 [16,1,3,3], b1, W2 [16,16,3,3], b2: conv parameters;  Wfc1 [F,2304], bfc1 [F]  (F % 4 == 0);
 *   h1 [R*B, F] (out): relu(fc1(...)) of masked copy pix[r] of sample b at row r*B + b;
 *   pd_save [R*B, 400], argmax_save [R*B, 400] bytes (both or neither; NULL for inference): what the backward
 *   needs -- the pooled block minus the background in [cell][channel] order and the max-pool winners.
 * ws: >= gnf_mnistcnn_sparse_ws_bytes(R*B, F) bytes. */
int64_t gnf_mnistcnn_sparse_ws_bytes(int64_t n_rows, int64_t F);
int gnf_mnistcnn_sparse_fwd(const float* x, int64_t B, const float* P, const int32_t* pix, int64_t R,
                            const int32_t* groups, int64_t max_group_rows,
                            const float* W1, const float* b1, const float* W2, const float* b2,
                            const float* Wfc1, const float* bfc1, int64_t F,
                            float* h1, float* pd_save, unsigned char* argmax_save,
                            void* ws, int64_t ws_bytes, gnf_stream_t stream);
/* The training form of the same call (a backward follows): pd_save / argmax_save are required, and instead of a
 * workspace whose first R*B*400 floats the call would never touch (pd goes to pd_save), the caller hands in ONLY the buffer
 * of the parameter-only tables (>= gnf_mnistcnn_sparse_prep_bytes(F) bytes), which it keeps alive and passes to
 * gnf_mnistcnn_sparse_bwd_tables.  Same h1 / pd_save / argmax_save as gnf_mnistcnn_sparse_fwd, bit for bit.
 * (Round 6: an in-flight forward pinned 125 MB of dead workspace per conditioner at B = 100.) */
int gnf_mnistcnn_sparse_fwd_train(const float* x, int64_t B, const float* P, const int32_t* pix, int64_t R,
                                  const int32_t* groups, int64_t max_group_rows,
                                  const float* W1, const float* b1, const float* W2, const float* b2,
                                  const float* Wfc1, const float* bfc1, int64_t F,
                                  float* h1, float* pd_save, unsigned char* argmax_save,
                                  void* tables, int64_t tables_bytes, gnf_stream_t stream);
/* The same front for a caller that evaluates it MANY times with unchanged parameters (the 109 levels of one sampling
 * pass, NormalizingFlow.py:98-107 under ImageExperiments.py:341-350): the parameter-only tables -- the fc1 weight columns
 * of each crop origin, conv2's response to the all-zero image and fc1 of that background -- are built once by
 * gnf_mnistcnn_sparse_prepare into `prep` (>= gnf_mnistcnn_sparse_prep_bytes(F) bytes) and read by every
 * gnf_mnistcnn_sparse_fwd_prepared call (inference only: nothing is saved for a backward; ws >= R*B*400*4 bytes).
 * Same h1 as gnf_mnistcnn_sparse_fwd, bit for bit.  The last 64 floats of the tables are slack no kernel reads; they are
 * written as zeros, so the buffer is defined to its end. */
int64_t gnf_mnistcnn_sparse_prep_bytes(int64_t F);
int gnf_mnistcnn_sparse_prepare(const float* b1, const float* W2, const float* b2, const float* Wfc1, const float* bfc1,
                                int64_t F, void* prep, int64_t prep_bytes, gnf_stream_t stream);
int gnf_mnistcnn_sparse_fwd_prepared(const float* x, int64_t B, const float* P, const int32_t* pix, int64_t R,
                                     const int32_t* groups, int64_t max_group_rows,
                                     const float* W1, const float* b1, const float* W2, const float* b2, int64_t F,
                                     const void* prep, float* h1, void* ws, int64_t ws_bytes, gnf_stream_t stream);
/* The prepared front followed by fc2 (MLP.py:47: out = fc2(relu(fc1(.)))) in the same call: the fc1 + ReLU + fc2 chain of
 * the masked copies is ONE launch (a workgroup per 16 rows of a crop origin, relu(fc1) never leaves LDS) -- two launches per
 * level of a sampling pass instead of three, ~7 us instead of ~23 after the crop kernel.
 *   Wfc2 [out_d, F], bfc2 [out_d];  h2 [R*B, out_d] (out), row r*B + b as h1 above.
 * GNF_ESHAPE unless F == 128 and out_d <= 32 (the reference's MNISTCNN: fc1 2304 -> 128, fc2 128 -> out_d = 30 for the
 * Monotonic normalizer's conditioner, ImageExperiments.py:60-66); other widths take gnf_mnistcnn_sparse_fwd_prepared and
 * gnf_linear_fwd.  Equal to that pair up to fp32 summation order.  ws >= R*B*400*4 bytes. */
int gnf_mnistcnn_sparse_fwd_prepared_fc2(const float* x, int64_t B, const float* P, const int32_t* pix, int64_t R,
                                         const int32_t* groups, int64_t max_group_rows,
                                         const float* W1, const float* b1, const float* W2, const float* b2, int64_t F,
                                         const void* prep, const float* Wfc2, const float* bfc2, int64_t out_d,
                                         float* h2, void* ws, int64_t ws_bytes, gnf_stream_t stream);
/* Backward w.r.t. the network parameters (training with a frozen deterministic gate: P and x get no gradient).
 * g_h1 [R*B, F]: cotangent of h1 with the ReLU already applied (zero where h1 == 0).  Gradients are written, not
 * accumulated: gW1 [16,1,3,3], gb1 [16], gW2 [16,16,3,3], gb2 [16], gWfc1 [F,2304], gbfc1 [F].
 * The fc1 weight gradient is contracted per CHUNK of output rows so that the few large origins do not serialise:
 *   kgroups [2*n_kgroups] (device): (first output row, row count) of each chunk, a chunk lying inside one origin's
 *   rows, the chunks of an origin consecutive;  origin_chunks [2*64] (device): (first chunk, number of chunks). */
int64_t gnf_mnistcnn_sparse_bwd_ws_bytes(int64_t n_rows, int64_t F, int64_t n_kgroups);
/* gnf_mnistcnn_sparse_bwd against the parameter-only tables the FORWARD of the same step built (tables = the forward's
 * `(float*)ws + R*B*400`, or a gnf_mnistcnn_sparse_prepare buffer: fc1 column blocks per crop origin | background response): the
 * two table launches (~30 us of a 2.6 ms frozen-gate step) run once per step instead of twice.  tables == NULL: builds them. */
int gnf_mnistcnn_sparse_bwd_tables(const float* x, int64_t B, const float* P, const int32_t* pix, int64_t R,
                                   const int32_t* groups, int64_t max_group_rows,
                                   const int32_t* kgroups, int64_t n_kgroups, const int32_t* origin_chunks,
                                   const float* W1, const float* b1, const float* W2, const float* b2,
                                   const float* Wfc1, int64_t F, const void* tables,
                                   const float* pd, const unsigned char* argmax, const float* g_h1,
                                   float* gW1, float* gb1, float* gW2, float* gb2, float* gWfc1, float* gbfc1,
                                   void* ws, int64_t ws_bytes, gnf_stream_t stream);
int gnf_mnistcnn_sparse_bwd(const float* x, int64_t B, const float* P, const int32_t* pix, int64_t R,
                            const int32_t* groups, int64_t max_group_rows,
                            const int32_t* kgroups, int64_t n_kgroups, const int32_t* origin_chunks,
                            const float* W1, const float* b1, const float* W2, const float* b2,
                            const float* Wfc1, int64_t F,
                            const float* pd, const unsigned char* argmax, const float* g_h1,
                            float* gW1, float* gb1, float* gW2, float* gb2, float* gWfc1, float* gbfc1,
                            void* ws, int64_t ws_bytes, gnf_stream_t stream);

/* ---- Adam on one flat fp32 buffer (torch.optim.Adam semantics, L2 weight decay) --------
 * ImageExperiments.py:173 / UCIExperiments.py:97; used by the data-parallel harness after
 * the single RCCL all-reduce.  grad_scale multiplies the (summed) gradient first.  Hyper-parameters are doubles:
 * 1-beta, lr/(1-beta1^t) and sqrt(1-beta2^t) are formed in double and rounded once, as torch.optim.Adam forms them
 * (tested against it on the device, 1e-6). */
int gnf_adam_step(float* p, const float* g, float* m, float* v, int64_t n,
                  double lr, double beta1, double beta2, double eps, double weight_decay,
                  double grad_scale, int step, gnf_stream_t stream);

/* Same update (torch.optim.Adam at ImageExperiments.py:173 / UCIExperiments.py:97), with the step count in device
 * memory: step_dev points to TWO ints, {number of steps already taken, 0} -- the second is the ticket counter by which
 * the last workgroup of the launch increments the first when advance != 0, and reads 0 again afterwards (a step over
 * several disjoint runs of the flat buffer, e.g. around a frozen parameter, advances on its last launch only):
 * nothing step-dependent is passed by value, so a captured hipGraph of a whole training step can be replayed
 * (gnf_hip.dp.GraphedStep -- the launch-bound configurations). */
int gnf_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n,
                      double lr, double beta1, double beta2, double eps, double weight_decay,
                      double grad_scale, int* step_dev, int advance, gnf_stream_t stream);

/* ---- batch preparation of the image driver in one launch (train_image.py; reference lib/transform.py:5-21,
 * ImageExperiments.py:33-37, :97) --------------------------------------------------------------------------------------
 * Output row b < B is row rows[b] of a uint8 data set, optionally mirrored, dequantised and logit-transformed:
 *   pixel = data[rows[b], src(j)],  y = alpha + (1 - 2 alpha) (pixel + u) / 256,  x[b, j] = log y - log (1 - y),
 *   bpp_term[b] = sum_j log2 y + log2 (1 - y)        (the data term of bits per pixel, from y itself and not from x).
 * 1 - y is evaluated as alpha + (1 - 2 alpha) (256 - pixel - u) / 256: the same number without the cancellation of the
 * subtraction (a white pixel at alpha = 1e-6 keeps its full precision).  Logarithms: v_log_f32, 1 ulp.
 * data: [n_rows, d] bytes, row-major, at ANY byte address;  d = C*H*W (C, H, W matter only for the flip).
 * rows: B int32 device indices, any order, repeats allowed, or NULL for rows 0 .. B-1 (needs B <= n_rows).  The host copy is
 *   not required and nothing is read back: the kernel CLAMPS every index into [0, n_rows), so an index outside the data set
 *   prepares the first / last row instead of reading outside it.  Keeping the indices inside is the caller's contract.
 * flip_mode 0: no flip;  1: the byte mask flip [B] decides (nonzero = mirrored);  2: one Philox coin per output row,
 *   p = 1/2.  A mirrored row reads source column W-1-w for output (c, h, w).
 * u: [B, d] explicit uniforms indexed by OUTPUT element (the parity hook, as u1 / u2 of the gate), or NULL for Philox.
 * Philox layout (seed = key, offset = the caller's call counter; philox4x32_10 and u01_open of csrc/gnf_common.h):
 *   output element e = b*d + j:  u = u01_open(r[e & 3]),  r = philox4x32_10(counter = (e >> 2, offset), key = seed),
 *     counter words (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset)), key words (lo32(seed), hi32(seed));
 *   coin of row b (flip_mode 2): counter words (lo32(b), hi32(b) | 0x80000000, lo32(offset), hi32(offset)), same key;
 *     mirrored when bit 31 of r[0] is set.  No element reaches that counter (e >> 2 < 2^62).
 *   Row b's noise and coin depend on (seed, offset, b, d) only, not on B.  tests/test_gpu_image_prep.py pins the layout.
 * x: [B, d] contiguous;  bpp_term: [B] or NULL.  The row sum is taken in a fixed order without atomics: the same bits on
 * every call.  Two kernels, chosen by the arguments, with BIT-IDENTICAL results: quads as one dword load + one float4 store
 * when d % 4 == 0, data is dword-aligned, x and u are 16-byte aligned (and W % 4 == 0 unless flip_mode is 0); bytes and
 * single floats otherwise.
 * GNF_EINVAL: B < 0, C / H / W < 1, flip_mode outside 0..2, alpha outside [0, .5), and for B > 0 a NULL data or x,
 * n_rows < 1, flip_mode 1 without flip, rows NULL with B > n_rows, a float / int32 pointer below dword alignment.
 * GNF_ESHAPE: B >= 2^31.  B == 0: returns 0 without a launch; every batch-sized pointer may be NULL.
 * (Added under ABI version 11: no existing symbol changed.) */
int gnf_image_prep(const unsigned char* data, int64_t n_rows, const int32_t* rows, int flip_mode,
                   const unsigned char* flip, int C, int H, int W, const float* u, uint64_t seed, uint64_t offset,
                   float alpha, float* x, float* bpp_term, int64_t B, gnf_stream_t stream);

/* ---- training batches of the toy driver (train_toy.py; reference lib/toy_data.py:11-226) -----------------------------
 * x[b, 2p], x[b, 2p + 1] for b < B, p < P: one draw of the 2-D base problem kinds[p], times col_scale[2p], col_scale[2p + 1].
 * kinds: HOST array of P problem numbers, 1 <= P <= 8 (read during the call, packed into a kernel argument):
 *    0 2igaussians   1 2gaussians   2 4gaussians   3 8gaussians   4 swissroll   5 circles   6 moons   7 pinwheel
 *    8 2spirals      9 checkerboard 10 line        11 line-noisy  12 cos        13 joint_gaussian
 *   The reference's composites are block lists: 2spirals-8gaussians = {8, 3}, 8-MIX = {8, 3, 4, 5, 10, 7, 9, 6} with the
 *   reciprocals of its `std` vector as col_scale (gnf_hip.ops.toy_blocks).
 * col_scale: HOST array of 2P factors or NULL (no scaling); passed by value as well.
 * u: device [B, P, 8] explicit uniforms in (0, 1) (the parity hook, as u of gnf_image_prep), or NULL for Philox.
 * Philox layout (seed = key, offset = the caller's call counter; philox4x32_10 and u01_open of csrc/gnf_common.h):
 *   u_{4q + w} of (b, p) = u01_open(r[w]),  r = philox4x32_10(counter words (lo32(b), (p << 8) | q, lo32(offset), hi32(offset)),
 *   key words (lo32(seed), hi32(seed))),  q = 0, 1.  Which uniform feeds which variate of a problem, and the arithmetic of each
 *   problem: the table at the head of csrc/gnf_toy_data.hip; train_toy.toy_reference is the same arithmetic in torch.
 *   A value depends on (seed, offset, b, p, kinds[p], col_scale[2p..2p+1]) only: not on B, P, ldx or the other blocks.
 *   tests/test_gpu_toy_data.py pins the layout.
 * x: device, element (b, c) at x + b*ldx + c, ldx >= 2P; columns >= 2P of a row are not touched.  Dword alignment suffices:
 *   a pair is stored as one float2 when x is 8-byte aligned and ldx is even, as two floats otherwise -- the same bits.
 * Per-batch counts the reference fixes (the two arms of 2spirals, the rings / moons, the five pinwheel classes) are fair
 *   draws per sample here, and pinwheel returns all B rows (the reference 5 (B // 5)): DESIGN.md section 1.
 * GNF_EINVAL: P outside 1..8, kinds NULL or an entry outside 0..13, B < 0, B > 2^32 (the sample index is one counter word),
 *   ldx < 2P, and for B > 0 a NULL x or an x / u below dword alignment.  Checked before any launch.
 * B == 0: returns 0 without a launch; x and u may be NULL.  One launch, one thread per (sample, block), no LDS, no workspace.
 * (Added under ABI version 11: no existing symbol changed.) */
int gnf_toy_sample(const int32_t* kinds, int P, const float* col_scale, const float* u, uint64_t seed, uint64_t offset,
                   float* x, int64_t ldx, int64_t B, gnf_stream_t stream);

/* ---- graph queries of the DAG conditioner (DAGConditioner.py:76-85, 240-254, 262-266) ---------------------------------
 * Topological levels, depth and acyclicity of G directed graphs on d nodes each; what the reference asks networkx on the
 * host (is_directed_acyclic_graph, find_cycle, dag_longest_path_length) after copying a d x d matrix there.
 * M: element (g, i, j) at M + g*stride_g + i*ld + j (strides in elements), ld >= d; stride_g == 0: ONE matrix shared by
 *   all graphs (G thresholds over it).  Node j is a parent of node i in graph g when pred_g(M[g, i, j]) holds:
 *     elem_type GNF_DAG_ELEM_F32, thresholds == NULL:  m != 0            (a NaN is an edge, as `P != 0` in torch)
 *     elem_type GNF_DAG_ELEM_F32, thresholds [G] fp32: m > thresholds[g]  compared in fp32 (a NaN is no edge)
 *     elem_type GNF_DAG_ELEM_U8 (torch's bool storage): m != 0;  thresholds must be NULL.
 *   A diagonal entry that satisfies the predicate is a self loop, i.e. a cycle.
 * level [G, d] int32: the length of the longest parent chain of node i (roots: 0); -1 for every node on or behind a cycle.
 * info [G, 2] int32: (n_levelled, n_levels).  Graph g is acyclic iff n_levelled == d; its depth (the number of edges of its
 *   longest path) is then n_levels - 1.  Every entry of level and info is written.
 * ws: >= gnf_dag_levels_ws_bytes(G, d) bytes (G * (ceil(d/64) + 1) * d * 8: the predicate as bits, and per row the mask of its
 *   nonzero words), else GNF_EWS; 8-BYTE aligned (it is written as 64-bit words), else GNF_EINVAL.
 * Alignment: dword for an fp32 M, thresholds, level and info; any byte address for a uint8 M.
 * Domain: 1 <= d <= 4096 (gnf_dag_levels_supported; outside it GNF_ESHAPE from gnf_dag_levels and gnf_dag_levels_ws_bytes,
 *   nothing is touched), G >= 0 and G * ceil(d/4) < 2^31.  G == 0: returns 0 without a launch.
 * GNF_EINVAL: G < 0, an unknown elem_type, and for G > 0 a NULL M / level / info / ws, ld < d, stride_g < 0, thresholds with a
 *   uint8 M, an operand below its alignment.  Checked before any launch.
 * Two launches: a pack kernel (one wavefront per row, 64 columns -> one word by __ballot) and a peel kernel with exactly one
 * workgroup per graph, a counted loop of at most d + 1 rounds and integer LDS atomics only: the same call returns the same
 * integers, and they are those of a Kahn walk on the host.
 * (Added under ABI version 11: no existing symbol changed.) */
#define GNF_DAG_ELEM_F32 0
#define GNF_DAG_ELEM_U8  1
int gnf_dag_levels_supported(int64_t d);
int64_t gnf_dag_levels_ws_bytes(int64_t G, int64_t d);
int gnf_dag_levels(const void* M, int elem_type, int64_t stride_g, int64_t ld, const float* thresholds,
                   int32_t* level, int32_t* info, void* ws, int64_t ws_bytes, int64_t G, int64_t d,
                   gnf_stream_t stream);

/* ---- training batches of the tabular driver from device memory (train_uci.py; reference UCIExperiments.py:120-135,
 * datasets' batch_iter) ------------------------------------------------------------------------------------------------
 * gnf_shuffle_keys writes the keys whose ascending sort is one epoch's permutation of n rows:
 *   keys[i] = ((r[i & 3] >> 1) << 32) | i,  r = philox4x32_10(counter words (lo32(i >> 2), 0, lo32(offset), hi32(offset)),
 *   key words (lo32(seed), hi32(seed)))  (philox4x32_10 of csrc/gnf_common.h; seed = key, offset = the epoch number).
 * The high word holds 31 random bits, so every key is non-negative and a signed or unsigned sort, on the device or in numpy,
 * orders them alike; the low word breaks ties, so (sorted keys) & 0xffffffff is a bijection of 0 .. n-1 by construction and
 * a pure function of (seed, offset, n): the same on every rank without a broadcast, and after a resume.  The sort is the
 * caller's (torch.sort); tests/test_uci_batches_host.py restates the layout in numpy, tests/test_gpu_tab_batch.py pins it.
 * keys: device int64 [n], 8-byte aligned.  Domain 0 <= n < 2^31.
 * GNF_EINVAL: n < 0, and for n > 0 a NULL keys or one below 8-byte alignment.  GNF_ESHAPE: n >= 2^31.
 * n == 0: returns 0 without a launch; keys may be NULL.  One launch, one thread per four keys, no LDS, no workspace.
 * (Added under ABI version 11: no existing symbol changed.) */
int gnf_shuffle_keys(uint64_t seed, uint64_t offset, int64_t n, int64_t* keys, gnf_stream_t stream);

/* One minibatch gathered out of a tabular data set: output row r < B is row perm[pos + r*stride] of X,
 *   pos = first, plus cursor[0] when cursor != NULL.
 * X: device fp32, element (i, j) at X + i*ldx + j, n_rows rows of d columns, ldx >= d (strides in elements).
 * perm: device int32 [n_perm] row indices, any values (repeats allowed), or NULL for the identity over the rows: the position
 *   is then the row index, n_perm is ignored and n_rows bounds the positions.
 * first, stride: the batch is every stride-th position from `first` (stride = the number of ranks, first = the batch's start
 *   plus the rank: the round-robin deal of train_uci.shard_batches).
 * cursor: device int32*, or NULL.  The kernel only READS cursor[0]; advancing it is a separate stream-ordered operation of
 *   the caller, so no workgroup can observe an advanced cursor.  Nothing step-dependent is then passed by value and a captured
 *   launch can be replayed (gnf_hip.dp.DeviceBatches.gather_into).
 * x: device [B, d] contiguous.
 * The kernel CLAMPS the position into [0, n_perm) and the row index into [0, n_rows), as gnf_image_prep clamps its indices: a
 *   wrong cursor or a perm entry outside the data set prepares a wrong row and never reads outside either array.  Without a
 *   cursor the last position is known to the host: first + (B-1)*stride >= n_perm is GNF_EINVAL.
 * Two kernels, chosen by the arguments, with BIT-IDENTICAL results (both only move floats): float4 units when d % 4 == 0,
 *   ldx % 4 == 0 and X and x are 16-byte aligned; otherwise, at any dword address and any d, the d / 4 quads of a row as
 *   dwordx4 accesses at dword alignment and its d % 4 last floats singly.  A row is moved by an aligned group of 1 .. 64 lanes
 *   along the row; its perm entry is read once, by the group's first lane.
 * GNF_EINVAL: B < 0, d < 1, ldx < d, stride < 1, first < 0, and for B > 0 a NULL X or x, n_rows < 1, perm given with
 *   n_perm < 1, X / x / perm / cursor below dword alignment, the range check above.  Checked before any launch.
 * GNF_ESHAPE: B*d >= 2^31.  B == 0: returns 0 without a launch; every pointer may be NULL.
 * One launch, no LDS, no workspace.
 * (Added under ABI version 11: no existing symbol changed.) */
int gnf_tab_batch(const float* X, int64_t n_rows, int64_t d, int64_t ldx, const int32_t* perm, int64_t n_perm,
                  int64_t first, int64_t stride, const int32_t* cursor, float* x, int64_t B, gnf_stream_t stream);

/* ---- a bias per group of G consecutive rows: the context half of a DAGMLP's first layer -------------------------------
 * The d masked copies of a sample share one context row, so the context columns of the first Linear contribute
 * cb = context W1[:, in_net:]^T, ONE row per sample, to the G = d rows of that sample (DAGMLP.forward with a context).
 *   fwd:  out[r, n]   = act(y[r, n] + cb[r / G, n])      r < M, n < H;  relu != 0: act = ReLU, else the identity
 *   bwd:  g_pre[r, n] = g[r, n] * [a[r, n] > 0]          a: the saved forward OUTPUT, or NULL for the identity (g_pre = g)
 *         g_cb[b, n]  = sum_{i < G} g_pre[b*G + i, n]    accumulated in fp32 in ascending i
 * y, out, g, a, g_pre: [M, H] contiguous;  cb, g_cb: [M / G, H] contiguous.  out may be y and g_pre may be g (in place: a
 * thread reads an element before it writes it and is its only writer).  g_pre may be NULL when a is NULL.
 * Every element of g_pre and g_cb has one writer that adds in a fixed order: no atomics, no partial sums, the same bits on
 * every call and for every deal of the work to wavefronts.
 * Two kernels each, chosen by the arguments, with BIT-IDENTICAL results: 16-byte accesses when H % 4 == 0 and every array is
 * 16-byte aligned; single dwords at any dword address and any H otherwise.
 * GNF_EINVAL: M < 0, H < 1, G < 1, and for M > 0 a NULL y / cb / out (g / g_cb; a without g_pre) or a pointer below dword
 * alignment.  GNF_ESHAPE: M % G != 0.  M == 0: returns 0 without a launch; every pointer may be NULL.
 * One launch, no LDS, no workspace.
 * (Added under ABI version 11: no existing symbol changed.) */
int gnf_group_bias_fwd(const float* y, const float* cb, float* out, int relu, int64_t M, int64_t H, int64_t G,
                       gnf_stream_t stream);
int gnf_group_bias_bwd(const float* g, const float* a, float* g_pre, float* g_cb, int64_t M, int64_t H, int64_t G,
                       gnf_stream_t stream);

/* ---- device-ceiling probes (measurement aids for bench.py) ---------------
 * gnf_probe_mfma_f32 launches `blocks` workgroups of 8 wavefronts that do nothing but
 * independent v_mfma_f32_16x16x4_f32 chains and returns the number of flops the launch issues
 * (negative on error); gnf_probe_copy is a STREAM copy of n floats (n % 4 == 0). */
int64_t gnf_probe_mfma_f32(float* out, int iters, int blocks, gnf_stream_t stream);
int gnf_probe_copy(float* dst, const float* src, int64_t n, gnf_stream_t stream);
/* an empty grid of `grid` workgroups of `block` threads: the launch-ramp floor of a kernel of that launch shape (measurement) */
int gnf_probe_empty(int64_t grid, int block, gnf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
