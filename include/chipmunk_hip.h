/*
 * chipmunk_hip.h -- C ABI of the MI355X (gfx950) column-sparse DiT hot path.
 *
 * One entry point per operator of the reference's PyTorch operator surface
 * (`TORCH_LIBRARY(chipmunk)`, reference csrc/chipmunk.cpp:45-60).  Plain pointers and sizes only:
 * no torch types cross this boundary.  The torch-side registration that turns these back into
 * `torch.ops.chipmunk.*` lives in chipmunk_amd/csrc/torch_registry.cpp; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless stated otherwise; bf16 tensors are raw 16-bit storage;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); calls only enqueue work;
 *   - return value 0 = success; non-zero = error, message available from chipmunk_last_error();
 *     nothing is ever written to stderr and the process is never exited (the reference exit()s in
 *     csrc/mlp/csp_mlp_mm2_and_scatter_add.cu:15-42; that behaviour is deliberately not reproduced);
 *   - strides are in ELEMENTS for dims (batch, head, token); the head dimension (128) is contiguous.
 */
#ifndef CHIPMUNK_HIP_H
#define CHIPMUNK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHIPMUNK_OK 0
#define CHIPMUNK_ERR_INVALID 1 /* bad shape / argument (the reference raises TORCH_CHECK / std::runtime_error) */
#define CHIPMUNK_ERR_LAUNCH 2  /* HIP launch failure */
#define CHIPMUNK_ERR_UNSUPPORTED 3 /* a fused entry point that does not apply to this launch: nothing was enqueued, use the unfused operators */

/* element types for the dtype-generic ops (reference dispatches bf16/fp16/fp32: topk_indices.cu:171-215) */
#define CHIPMUNK_DTYPE_BF16 0
#define CHIPMUNK_DTYPE_FP16 1
#define CHIPMUNK_DTYPE_FP32 2

/* Thread-local message of the last failing call on this thread ("" if none). */
const char *chipmunk_last_error(void);
/* ABI version of this library (bumped on signature changes). */
int chipmunk_abi_version(void);
/* Tuning knob: selects a kernel variant ("mm1_variant", "mm2_variant", "attn_variant", ...); 0 = shipped default.
 * Results are identical across variants; only speed differs.  Used by tools/kbench.py for A/B measurement. */
int chipmunk_set_option(const char *name, int value);
/* Seed of the random-key hash of chipmunk_topk_indices / _topk_delta_indices / _topk_mask (`random_amount` > 0).
 * Every such launch draws a fresh set (per-launch salt = f(seed, launch counter), mixed on the device with the first
 * element of each row); setting the seed restarts the sequence, so seed + launch order reproduce a run.  Replaces the
 * reference's per-call cuRAND reseed (csrc/indexed_io/topk_indices.cu:46-49) and torch.randint (modules/attn.py:77). */
int chipmunk_set_random_seed(uint64_t seed);

/* ---------------------------------------------------------------- column-sparse attention
 * Replaces chipmunk::csp_attn (reference csrc/attn/csp_attn.cu:315-423; schema csrc/chipmunk.cpp:52).
 * For every (b, h, 192-query group g): J = indices[b,h,g,0:counts[b,h,g]];
 *   o[b,h,i,:] += o_scale * sum_{j in J} softmax_j(q_i.k_j / sqrt(128)) v_j     for i in group g
 * q,o: [B,H,Nq,128] bf16 (strided); k,v: [B,H,Nk,128] bf16 (strided); indices [B,H,G,idx_stride] int32
 * (G = ceil(Nq/192), row stride idx_stride >= max count); counts [B,H,G] int32; o_scale in {1,-1}.
 * The accumulate is bf16: o_new = bf16(o_old + bf16(o_scale*result)) (csp_attn.cu:294-300). */
int chipmunk_csp_attn(const void *q, const void *k, const void *v, void *o, const int64_t q_strides[3],
                      const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                      const int32_t *indices, const int32_t *counts, int B, int H, int Nq, int Nk, int idx_stride,
                      int o_scale, void *stream);

/* Out-of-place form of chipmunk_csp_attn: o_out = o_in + bf16(o_scale * sparse_attention), o_in untouched; o_in and
 * o_out share `o_strides`.  It replaces the `o = out_cache.clone(); csp_attn(q, k, v, o, ...)` pair of the reference's
 * sparse step (src/chipmunk/modules/attn.py:186-188): same bytes, one kernel, no 2 x B*H*N*128*2-byte copy. */
int chipmunk_csp_attn_out(const void *q, const void *k, const void *v, const void *o_in, void *o_out,
                          const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                          const int64_t o_strides[3], const int32_t *indices, const int32_t *counts, int B, int H,
                          int Nq, int Nk, int idx_stride, int o_scale, void *stream);

/* chipmunk_csp_attn_out over RAGGED index rows (no reference counterpart; the reference's index tensor is [B,H,G,Nk] int32 --
 * 7 GB per HunyuanVideo layer for 0.56 GB of kept keys, which is why its modules store a bit-packed mask and rebuild the indices
 * in every step, modules/attn.py:95-100,161): row (b,h,g) = indices + idx_offsets[(b*H+h)*G+g], idx_offsets[item+1] -
 * idx_offsets[item] entries wide (B*H*G+1 int64 offsets, each a multiple of 4; indices 16-byte aligned); counts as before.
 * chipmunk_compact_indices builds that layout from a padded tensor: flat[offsets[r] + j] = indices[r*idx_stride + j] for
 * j < counts[r], 0 up to offsets[r+1]. */
int chipmunk_csp_attn_out_ragged(const void *q, const void *k, const void *v, const void *o_in, void *o_out,
                                 const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                                 const int64_t o_strides[3], const int32_t *indices, const int64_t *idx_offsets,
                                 const int32_t *counts, int B, int H, int Nq, int Nk, int o_scale, void *stream);
int chipmunk_compact_indices(const int32_t *indices, int64_t idx_stride, const int32_t *counts, const int64_t *offsets,
                             int32_t *flat, int64_t rows, void *stream);

/* Replaces chipmunk::csp_128_attn (reference csrc/attn/csp_128_attn.cu:355-461; schema csrc/chipmunk.cpp:53).
 * Same math, out of place into `o` (contiguous [B,H,Nq,128] bf16, fully overwritten), contiguous q/k/v. */
int chipmunk_csp_128_attn(const void *q, const void *k, const void *v, void *o, const int32_t *indices,
                          const int32_t *counts, int B, int H, int Nq, int Nk, int idx_stride, void *stream);

/* Replaces chipmunk::dense_attn (reference csrc/attn/dense_attn.cu:246-372; schema csrc/chipmunk.cpp:54).
 * o [B,H,Nq,128] bf16 contiguous; l [B,H,Nq] fp32 = 1 / sum_j exp(q_i.k_j / sqrt(128)) (dense_attn.cu:225-227). */
int chipmunk_dense_attn(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                        const int64_t k_strides[3], const int64_t v_strides[3], void *o, float *l, int B, int H,
                        int Nq, int Nk, void *stream);

/* The dense operators with an output layout: o_strides = (batch, head, row) element strides of `o`, rows of 128 contiguous
 * elements (NULL = contiguous [B,H,Nq,128], i.e. the entries above).  Token-major storage [B,Nq,H,128] -- strides
 * {Nq*H*128, 128, H*128} -- is what the model's next GEMM reads: the reference's `rearrange(o, "b h s d -> b s (h d)")`
 * (a 2 x B*H*Nq*256-byte copy after every attention, e.g. hunyuan/modules/models.py:264) becomes a view.  The sparse step
 * keeps the layout by itself: chipmunk_csp_attn / chipmunk_csp_attn_out take o_strides already. */
int chipmunk_dense_attn_strided(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                                const int64_t k_strides[3], const int64_t v_strides[3], void *o, const int64_t *o_strides,
                                float *l, int B, int H, int Nq, int Nk, void *stream);
int chipmunk_dense_colsum_attn_strided(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                                       const int64_t k_strides[3], const int64_t v_strides[3], const float *p, void *o,
                                       const int64_t *o_strides, void *cs, float *l, int B, int H, int Nq, int Nk,
                                       int cs_stride, void *stream);
int chipmunk_dense_colsum_topk_mask_strided(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                                            const int64_t k_strides[3], const int64_t v_strides[3], const float *p, void *o,
                                            const int64_t *o_strides, float *l, int B, int H, int Nq, int Nk,
                                            const void *static_mask, int64_t static_stride, int static_rows,
                                            const void *group_flags, void *mask, int k_top, double random_amount, void *stream);

/* Replaces chipmunk::dense_colsum_attn (reference csrc/attn/dense_colsum_attn.cu:521-668; schema chipmunk.cpp:55).
 * p [B,H,Nq] fp32 = previous step's l.  cs [B,H,ceil(Nq/192),cs_stride] bf16:
 *   cs[b,h,g,j] = sum_{i in group g} bf16(exp(s_ij - m_i)) * bf16(exp(m_i) * p_i)   for j < Nk
 * (dense_colsum_attn.cu:267-277); columns j >= Nk are left untouched.
 * Launches that fill the CUs run as ONE pass (the column sums ride the dense kernel's softmax pipeline) and keep, per
 * (device, stream), a library-owned buffer of bf16 partial sums of B*H*ceil(Nq/256)*2*Nk*2 bytes (halved per chunk of
 * heads if that cannot be allocated; bounded, see chipmunk_release_scratch); the first call on a stream allocates it, so call
 * once before capturing a graph. */
int chipmunk_dense_colsum_attn(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                               const int64_t k_strides[3], const int64_t v_strides[3], const float *p, void *o,
                               void *cs, float *l, int B, int H, int Nq, int Nk, int cs_stride, void *stream);

/* Row-wise pass of the block around the operators (torch ops in the reference's model code, e.g.
 * examples/hunyuan/hyvideo/modules/models.py:184-186, 262-275): with y, gate, x_out set
 *   x_out = bf16(x + gate * y);  xm = bf16(shift + bf16(LayerNorm(x_out)) * bf16(1 + scale))
 * and with y = gate = x_out = NULL the LayerNorm + modulate of x alone.  x, y, x_out, xm [rows, cols] bf16 contiguous (x_out may
 * be x); gate, shift, scale [cols] bf16; LayerNorm over cols without affine, statistics in fp32 (two passes over the row in
 * registers).  cols % 8 == 0, cols <= 8192, 16-byte aligned pointers.  One read of x and y, one write of x_out and xm. */
int chipmunk_residual_ln_modulate(const void *x, const void *y, const void *gate, const void *shift, const void *scale,
                                  void *x_out, void *xm, int64_t rows, int cols, double eps, void *stream);

/* The same pass for Wan's blocks (reference examples/wan/wan/modules/model.py:100-110, 317-334): an fp32 residual stream, fp32
 * vectors given per SEQUENCE, and a LayerNorm that is either modulated or affine.  Rows are B sequences of L rows of cols columns.
 *   x [B*L, cols]: x_dtype 2 = fp32, 1 = bf16 (the stream before the first block).  xm [B*L, cols] bf16.
 *   y [B*L, cols] bf16 and x_out [B*L, cols] fp32 come together (x_out may be an fp32 x):
 *       x_out = fp32(fp32(x) + fp32(fp32(y) * gate))   -- two roundings, never a fused multiply-add; gate = NULL: fp32(x) + fp32(y).
 *     A gate without y is refused, and so is a bf16 x with y and no gate (torch would keep that sum in bf16).
 *   gate, shift, scale fp32: sequence b reads its vector at p + b * batch_stride (elements); stride 0 = one vector [cols] for all.
 *   Exactly one pair of (shift, scale) and (weight, bias) is set; weight, bias fp32 [cols].  With v = x_out (x without y) and
 *   xn = (v - mean) / sqrt(var + eps) over cols (biased variance, statistics in fp32, two passes over the row in registers):
 *       xm = bf16(xn * fp32(1 + scale) + shift)    or    xm = bf16(xn * weight + bias)        -- evaluated in fp32, rounded once;
 *     for a bf16 x without y and with a modulation xn is rounded to bf16 first (WanLayerNorm's .type_as; with the affine pair that
 *     cast is the one rounding above).
 * cols % 8 == 0, cols <= 8192; 16-byte aligned pointers, batch strides 0 or multiples of 4 that cover cols.  A batch of B sequences
 * gives the bits of B calls.  One read of x and y, one write of x_out and xm; the vectors stay in registers up to cols = 3072 and are
 * re-read per row (from L2) above. */
int chipmunk_residual_ln_modulate_f32(const void *x, int x_dtype, const void *y, const float *gate, int64_t gate_batch_stride,
                                      const float *shift, const float *scale, int64_t mod_batch_stride, const float *weight,
                                      const float *bias, float *x_out, void *xm, int64_t B, int64_t L, int cols, double eps,
                                      void *stream);

/* ---------------------------------------------------------------- column-sparse MLP
 * Replaces chipmunk::csp_mlp_mm1 (reference csrc/mlp/csp_mlp_mm1.cu:625-702; schema csrc/chipmunk.cpp:47).
 * For 128-row group g and packed column j < counts[g]:
 *   c[m,j] = bf16( gelu_tanh(a[m,:].b[idx[g,j],:] + bias[idx[g,j]]) - pa_cache[idx[g,j], m] )
 * a [M,K], b [F,K] (= fc1.weight), c [M,F] (packed; columns >= counts[g] untouched), bias [F],
 * pa_cache [F,M] (column-major activation cache), indices [M/128,F] int32, counts [M/128] int32; all bf16.
 * Requires M % 128 == 0, K % 64 == 0 (csp_mlp_mm1.cu:215,230); counts need only be multiples of 16. */
int chipmunk_csp_mlp_mm1(const void *a, const void *b, void *c, const void *bias, const void *pa_cache,
                         const int32_t *indices, const int32_t *counts, int M, int K, int F, void *stream);

/* GEMM1 that also applies the scatter-add of its own output: after computing c as above,
 *   pa_cache[idx[g,j], m] = bf16(pa_cache[idx[g,j], m] + c[m,j])          (== chipmunk_csp_scatter_add(c, pa_cache, ...))
 * from the cache block the epilogue already holds in LDS.  Bit-identical to chipmunk_csp_mlp_mm1 followed by
 * chipmunk_csp_scatter_add; saves that kernel's launch and its re-read of c and the cache.  Each (group, column) block of
 * the cache is read and written by exactly one workgroup. */
int chipmunk_csp_mlp_mm1_scatter(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                 const int32_t *indices, const int32_t *counts, int M, int K, int F, void *stream);

/* fp8 (OCP e4m3fn) GEMM1 for BASELINE config C5: native counterpart of the reference's Triton csp_mlp_mm1_fp8
 * (src/chipmunk/triton/csp_mlp_mm1.py:37-164).  a [M,K] fp8, b [F,K] fp8; scale_a / scale_b: device pointers to ONE
 * fp32 each (the reference passes 0-dim tensors holding the RECIPROCAL quantisation scales, modules/mlp.py:98-99):
 *   x = bf16(gelu_tanh(a.b[idx] * scale_a * scale_b + bias[idx]));  c[m,j] = bf16(x - pa_cache[idx, m])
 * update_cache = 1 additionally stores x into pa_cache like the Triton kernel (:140); 0 leaves the cache to the
 * scatter-add (the bf16 path's contract); 2 applies that scatter-add itself -- pa_cache[idx, m] += c[m, j] in bf16, bit for
 * bit what chipmunk_csp_scatter_add would do afterwards (as chipmunk_csp_mlp_mm1_scatter on the bf16 path).
 * Requires K % 128 == 0. */
int chipmunk_csp_mlp_mm1_fp8(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                             const int32_t *indices, const int32_t *counts, const float *scale_a,
                             const float *scale_b, int M, int K, int F, int update_cache, void *stream);

/* Replaces chipmunk::csp_mlp_mm2_and_scatter_add (reference csrc/mlp/csp_mlp_mm2_and_scatter_add.cu:96-259 plus the
 * Triton GEMM src/chipmunk/triton/csp_mlp_mm2.py:26-129; schema csrc/chipmunk.cpp:48).
 *  (i)  unpacked_colmajor[idx[g,c], g*128 + r] += packed[g*128 + r, c]           (bf16 add, c < counts[g])
 *  (ii) mma_c[m,:] = bf16(sum_{c<counts[g]} mma_a[m,c] * mma_b[idx[g,c],:]) + mma_c[m,:]
 * packed, mma_a [M,F]; unpacked_colmajor [F,M]; mma_b [F,N2] (= fc2.weight.T contiguous); mma_c [M,N2].
 * `num_sms_scatter_add` is the reference's SM-partition hint (kept for signature parity; ignored). */
int chipmunk_csp_mlp_mm2_and_scatter_add(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                         const int32_t *counts, const void *mma_a, const void *mma_b, void *mma_c,
                                         int M, int F, int N2, int num_sms_scatter_add, void *stream);

/* Replaces chipmunk::csp_scatter_add (reference csrc/indexed_io/scatter_add.cu:102-181; schema chipmunk.cpp:59): (i) only. */
int chipmunk_csp_scatter_add(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                             const int32_t *counts, int M, int F, int num_sms, void *stream);

/* GEMM (ii) alone: the native counterpart of the reference's Triton csp_mlp_mm2 (triton/csp_mlp_mm2.py:104-129). */
int chipmunk_csp_mlp_mm2(const void *mma_a, const void *mma_b, void *mma_c, const int32_t *indices,
                         const int32_t *counts, int M, int F, int N2, void *stream);

/* The sparse-MLP operators for ANY number of token rows (no reference counterpart: the reference requires M % 128 == 0).
 * M > 0; G = ceil(M / 128) groups, the last one with M - 128 (G - 1) rows; indices [G, F], counts [G].
 *   - Row-major tensors (a [M,K], c / packed / mma_a [M,F], mma_c [M,N2]) hold exactly M rows: no byte at or past row M is loaded
 *     or stored, and rows < M get the bits the entries above give them on the problem padded with zero rows.
 *   - The column-major activation cache is [F, ldc]: column f starts at element f * ldc.  ldc >= M and ldc % 8 == 0; elements
 *     [M, ldc) of a column are padding the operator may overwrite with anything (nothing read there reaches a row < M), and
 *     nothing outside F * ldc elements is touched.  ldc == M is allowed when M % 8 == 0 (a contiguous [F, M] cache).
 * K, F, N2, alignment and 32-bit-offset conditions (with F * ldc in place of F * M) as for the entries they extend. */
int chipmunk_csp_mlp_mm1_ragged(const void *a, const void *b, void *c, const void *bias, const void *pa_cache,
                                const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, void *stream);
int chipmunk_csp_mlp_mm1_scatter_ragged(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                        const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc,
                                        void *stream);
int chipmunk_csp_mlp_mm1_fp8_ragged(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                    const int32_t *indices, const int32_t *counts, const float *scale_a,
                                    const float *scale_b, int M, int K, int F, int ldc, int update_cache, void *stream);
int chipmunk_csp_mlp_mm2_ragged(const void *mma_a, const void *mma_b, void *mma_c, const int32_t *indices,
                                const int32_t *counts, int M, int F, int N2, void *stream);
int chipmunk_csp_mlp_mm2_and_scatter_add_ragged(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                                const int32_t *counts, const void *mma_a, const void *mma_b, void *mma_c,
                                                int M, int F, int N2, int ldc, void *stream);
int chipmunk_csp_scatter_add_ragged(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                    const int32_t *counts, int M, int F, int ldc, void *stream);

/* Batches: the same operators over B sequences of M rows in ONE launch (no reference counterpart: the reference hard-wires B = 1).
 * The ragged contract above holds per sequence (any M > 0, ldc >= M, ldc % 8 == 0); the argument order is that of the *_ragged entry
 * followed by `int B` and, where a cache is passed, `int64_t cache_batch_stride`.
 *   - Row-major tensors are dense [B, M, .]: a [B,M,K], c / packed / mma_a [B,M,F], mma_c [B,M,N2].
 *   - indices [B, G, F] and counts [B, G], G = ceil(M / 128): what chipmunk_topk_indices writes for B * G rows.
 *   - The cache is [B, F, ldc]; sequence b's starts at element b * cache_batch_stride, with cache_batch_stride >= F * ldc and a
 *     multiple of 8 (elements).  Nothing outside the F * ldc elements of each sequence is touched.
 *   - Weights (b, mma_b) and bias are shared by all sequences.
 *   - B >= 1 and B * G <= 65535.  The 32-bit-offset conditions apply per sequence: B * M * F may exceed 2^31.
 * Every output element gets the bits B calls of the *_ragged entry on the sequences' slices give it.  Each failed check returns
 * CHIPMUNK_ERR_INVALID with a message that names the rule, before anything is enqueued. */
int chipmunk_csp_mlp_mm1_batched(const void *a, const void *b, void *c, const void *bias, const void *pa_cache,
                                 const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int B,
                                 int64_t cache_batch_stride, void *stream);
int chipmunk_csp_mlp_mm1_scatter_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                         const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int B,
                                         int64_t cache_batch_stride, void *stream);
int chipmunk_csp_mlp_mm1_fp8_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                     const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                     int M, int K, int F, int ldc, int update_cache, int B, int64_t cache_batch_stride,
                                     void *stream);
int chipmunk_csp_mlp_mm2_batched(const void *mma_a, const void *mma_b, void *mma_c, const int32_t *indices,
                                 const int32_t *counts, int M, int F, int N2, int B, void *stream);
int chipmunk_csp_mlp_mm2_and_scatter_add_batched(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                                 const int32_t *counts, const void *mma_a, const void *mma_b, void *mma_c,
                                                 int M, int F, int N2, int ldc, int B, int64_t cache_batch_stride,
                                                 void *stream);
int chipmunk_csp_scatter_add_batched(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                     const int32_t *counts, int M, int F, int ldc, int B, int64_t cache_batch_stride,
                                     void *stream);

/* Gated GEMM1 (SwiGLU / GEGLU feed-forwards, fc2(act(x Wg + bg) * (x Wu + bu)); no reference counterpart).  For group g and packed
 * column j < counts[g], with i = idx[g,j]:
 *   c[m,j] = bf16( act(a[m,:].b_gate[i,:] + bias_gate[i]) * (a[m,:].b_up[i,:] + bias_up[i]) - pa_cache[i, m] )
 * in fp32 with one rounding.  b_gate and b_up are [F,K] bf16 with row stride K: two weights, or the two halves of one fused [2F,K]
 * projection in either order.  bias_gate / bias_up are bf16 [F] or NULL (= zero).  act is one of the CHIPMUNK_ACT_* codes below.
 * update_cache = 1 also applies pa_cache[i, m] = bf16(pa_cache[i, m] + c[m,j]), the arithmetic of chipmunk_csp_scatter_add on c;
 * 0 leaves the cache as it is.  Contract of the *_ragged entries (any M >= 1, ldc >= M, ldc % 8 == 0, K % 64 == 0, F % 64 == 0) and,
 * for *_batched, of the batch entries above (weights and biases shared by all sequences).  bf16 only: e4m3 operands take the *_glu_fp8
 * entries below.
 * A failed check returns CHIPMUNK_ERR_INVALID with a message, before anything is enqueued. */
#define CHIPMUNK_ACT_GELU_TANH 0 /* x * 0.5 * (1 + tanh(0.79788456 (x + 0.044715 x^3))): the code of chipmunk_csp_mlp_mm1 */
#define CHIPMUNK_ACT_SILU 1      /* x / (1 + exp(-x)) */
#define CHIPMUNK_ACT_GELU_ERF 2  /* 0.5 x (1 + erf(x / sqrt 2)) */
int chipmunk_csp_mlp_mm1_glu(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                             const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K,
                             int F, int ldc, int act, int update_cache, void *stream);
int chipmunk_csp_mlp_mm1_glu_batched(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                     const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts, int M,
                                     int K, int F, int ldc, int act, int update_cache, int B, int64_t cache_batch_stride,
                                     void *stream);
/* The gated GEMM1 with fp8 projections: a [M,K], b_gate / b_up [F,K] are OCP e4m3 bytes (float8_e4m3fn; two weights or the halves of one
 * [2F,K] tensor, row stride K), scale_a / scale_b_gate / scale_b_up one device float each -- the RECIPROCAL quantisation scales, as
 * chipmunk_csp_mlp_mm1_fp8 takes them.  In fp32, accumulators from zero:
 *   gate = (a[m,:].b_gate[i,:]) * scale_a * scale_b_gate + bias_gate[i],   up = (a[m,:].b_up[i,:]) * scale_a * scale_b_up + bias_up[i]
 *   c[m,j] = bf16( fma(act(gate), up, -pa_cache[i, m]) )
 * Biases (NULL = zero), the cache and c are bf16; update_cache 0 / 1 and every other rule as chipmunk_csp_mlp_mm1_glu[_batched], except
 * K % 128 == 0 and 1 byte per element of a and the weights in the 32-bit-offset limits. */
int chipmunk_csp_mlp_mm1_glu_fp8(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                 const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts,
                                 const float *scale_a, const float *scale_b_gate, const float *scale_b_up, int M, int K, int F,
                                 int ldc, int act, int update_cache, void *stream);
int chipmunk_csp_mlp_mm1_glu_fp8_batched(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                         const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts,
                                         const float *scale_a, const float *scale_b_gate, const float *scale_b_up, int M, int K,
                                         int F, int ldc, int act, int update_cache, int B, int64_t cache_batch_stride,
                                         void *stream);

/* Ungated activations: GEMM1 of fc2(act(x W1 + b1)) for any of the CHIPMUNK_ACT_* codes above, with or without a bias (no reference
 * counterpart: chipmunk_csp_mlp_mm1 and the reference compute tanh-GeLU with a bias only).  For group g and packed column
 * j < counts[g], with i = idx[g,j]:
 *   bf16:  c[m,j] = bf16( act(a[m,:].b[i,:] + bias[i]) - pa_cache[i, m] )              fp32, the bias inside the sum, one rounding
 *   fp8:   t = bf16( act((a[m,:].b[i,:] * scale_a) * scale_b + bias[i]) );  c[m,j] = bf16( t - pa_cache[i, m] )
 * bias is bf16 [F] or NULL (= zero).  act = CHIPMUNK_ACT_GELU_TANH with a bias gives the bits of chipmunk_csp_mlp_mm1[_scatter] /
 * chipmunk_csp_mlp_mm1_fp8.  update_cache, bf16 pair: 0 leaves the cache, 1 also applies the scatter-add of c (the bits of
 * chipmunk_csp_scatter_add afterwards); fp8 pair: 0 / 1 / 2 as chipmunk_csp_mlp_mm1_fp8 (1 stores t, 2 applies the scatter-add).
 * Contract of the *_ragged entries (any M >= 1, ldc >= M, ldc % 8 == 0, F % 64 == 0; K % 64 == 0 for bf16, K % 128 == 0 and e4m3 a / b
 * with two reciprocal scales for fp8) and, for *_batched, of the batch entries above.  An unknown act, an update_cache out of range or
 * a K off its multiple returns CHIPMUNK_ERR_INVALID with a message, before anything is enqueued. */
int chipmunk_csp_mlp_mm1_act(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                             const int32_t *counts, int M, int K, int F, int ldc, int act, int update_cache, void *stream);
int chipmunk_csp_mlp_mm1_act_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                     const int32_t *counts, int M, int K, int F, int ldc, int act, int update_cache, int B,
                                     int64_t cache_batch_stride, void *stream);
int chipmunk_csp_mlp_mm1_fp8_act(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                 const int32_t *counts, const float *scale_a, const float *scale_b, int M, int K, int F, int ldc,
                                 int act, int update_cache, void *stream);
int chipmunk_csp_mlp_mm1_fp8_act_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                         const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                         int M, int K, int F, int ldc, int act, int update_cache, int B, int64_t cache_batch_stride,
                                         void *stream);

/* fp8 row scales: chipmunk_csp_mlp_mm1_fp8_act[_batched] with one activation scale per token row and one weight scale per fc1 column
 * (dynamic per-token x per-output-channel quantisation; no reference counterpart).  The contract is that of the entries above -- any
 * M >= 1, ldc, act, update_cache 0 / 1 / 2, bias bf16 [F] or NULL -- except that
 *   scale_a is fp32 [M] ([B, M] for the batched entry): the RECIPROCAL scale of row m (chipmunk_quantize_fp8_rowwise's scale_recip),
 *   scale_b is fp32 [F]: the RECIPROCAL scale of weight row i, read at the GATHERED column i = idx[g,j],
 *   t = bf16( act((a[m,:].b[i,:] * scale_a[m]) * scale_b[i] + bias[i]) );  c[m,j] = bf16( t - pa_cache[i, m] )
 * in the multiplication order of the scalar form: constant vectors give the bits of chipmunk_csp_mlp_mm1_fp8_act.  No element of scale_a
 * at or past M (B * M) and none of scale_b at or past F is read. */
int chipmunk_csp_mlp_mm1_fp8_act_rs(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                    const int32_t *counts, const float *scale_a, const float *scale_b, int M, int K, int F, int ldc,
                                    int act, int update_cache, void *stream);
int chipmunk_csp_mlp_mm1_fp8_act_rs_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                            const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                            int M, int K, int F, int ldc, int act, int update_cache, int B,
                                            int64_t cache_batch_stride, void *stream);

/* fp8 fc2: GEMM (ii) over e4m3 rows of fc2^T (weight-only fp8).  mma_a [M,F] bf16 packed deltas, mma_b [F,N2] OCP e4m3 bytes
 * (float8_e4m3fn), plain row-major, scale_b one device float -- the weight's RECIPROCAL quantisation scale --, mma_c [M,N2] bf16:
 *   mma_c[m,:] = bf16( bf16( (sum_{c < counts[g]} mma_a[m,c] * f(mma_b[indices[g,c],:])) * scale_b[0] ) + mma_c[m,:] )
 * f widens e4m3 to bf16 (exact); the sum is chipmunk_csp_mlp_mm2's, in fp32, on the widened weights, so with scale_b a power of two the
 * result has the bits of chipmunk_csp_mlp_mm2 on bf16(f(mma_b) * scale_b).  Any M > 0 (the *_ragged contract), indices / counts / groups
 * as for chipmunk_csp_mlp_mm2[_ragged|_batched]; N2 a positive multiple of 16 (one 16-byte chunk of a row is 16 columns); M*F, F*N2 and
 * M*N2 below 2^31 per sequence; *_batched: B sequences, B * ceil(M/128) <= 65535. */
int chipmunk_csp_mlp_mm2_w8(const void *mma_a, const void *mma_b, const float *scale_b, void *mma_c, const int32_t *indices,
                            const int32_t *counts, int M, int F, int N2, void *stream);
int chipmunk_csp_mlp_mm2_w8_batched(const void *mma_a, const void *mma_b, const float *scale_b, void *mma_c, const int32_t *indices,
                                    const int32_t *counts, int M, int F, int N2, int B, void *stream);

/* fp8 fc1, weight-only: chipmunk_csp_mlp_mm1_act[_batched|_gm] over an e4m3 weight with bf16 activations (no reference counterpart).
 * a [M,K] bf16; b [F,K] OCP e4m3 bytes (float8_e4m3fn), plain row-major; scale_b fp32 on the device, the weight's RECIPROCAL
 * quantisation scale: one number (scale_n == 1) or one per row of b (scale_n == F, read at the GATHERED column i = idx[g,j]):
 *   c[m,j] = bf16( act( (sum_k a[m,k] * f(b[i,k])) * scale_b[i] + bias[i] ) - pa_cache[i, m] )
 * f widens e4m3 to bf16 (exact); the sum is chipmunk_csp_mlp_mm1_act's, in fp32 from zero, on the widened weight; the scale and then the
 * bias are applied in fp32, each rounded (no fma); act and the subtraction are one rounding.  With a power-of-two scale and no bias the
 * result has the bits of chipmunk_csp_mlp_mm1_act on bf16(f(b) * scale_b).  bias is bf16 [F] or NULL (= zero); update_cache 0 leaves
 * the cache, 1 also applies the scatter-add of c.  Contract of chipmunk_csp_mlp_mm1_act and its *_batched / *_gm forms: any M >= 1,
 * ldc >= M, ldc % 8 == 0, F % 64 == 0, K % 64 == 0, F*K, M*K and F*ldc below 2^31.  A null a / b / scale_b / c / pa_cache, a scale_n
 * other than 1 or F, a scale_b off 4-byte alignment, a K off its multiple, an update_cache outside 0 / 1 or an unknown act returns
 * CHIPMUNK_ERR_INVALID with a message, before anything is enqueued.  No element of scale_b at or past scale_n is read. */
int chipmunk_csp_mlp_mm1_w8(const void *a, const void *b, const float *scale_b, int scale_n, void *c, const void *bias, void *pa_cache,
                            const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int act, int update_cache,
                            void *stream);
int chipmunk_csp_mlp_mm1_w8_batched(const void *a, const void *b, const float *scale_b, int scale_n, void *c, const void *bias,
                                    void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int act,
                                    int update_cache, int B, int64_t cache_batch_stride, void *stream);

/* gated fp8, weight-only: chipmunk_csp_mlp_mm1_glu[_batched|_gm] over e4m3 gate / up weights with bf16 activations (no reference
 * counterpart).  a [M,K] bf16; b_gate / b_up [F,K] OCP e4m3 bytes (float8_e4m3fn), row stride K: two weights, or the halves of one
 * fused [2F,K] projection in either order; scale_gate / scale_up fp32 on the device, each weight's RECIPROCAL quantisation scale: one
 * number (its _n == 1) or one per row (its _n == F, read at the GATHERED column i = idx[g,j]).  In fp32:
 *   g = (sum_k a[m,k] * f(b_gate[i,k])) * scale_gate[i] + bias_gate[i],   u = (sum_k a[m,k] * f(b_up[i,k])) * scale_up[i] + bias_up[i]
 *   c[m,j] = bf16( fma(act(g), u, -pa_cache[i, m]) )
 * f widens e4m3 to bf16 (exact); the sums are chipmunk_csp_mlp_mm1_glu's, from zero, on the widened weights; each scale and then each
 * bias is applied in fp32, each rounded (no fma); act, the product and the subtraction are one rounding.  With power-of-two scales and
 * no biases the result has the bits of chipmunk_csp_mlp_mm1_glu on bf16(f(b_gate) * scale_gate), bf16(f(b_up) * scale_up).  Biases are
 * bf16 [F] or NULL (= zero); update_cache 0 leaves the cache, 1 also applies the scatter-add of c.  Contract of
 * chipmunk_csp_mlp_mm1_glu and its *_batched / *_gm forms: any M >= 1, ldc >= M, ldc % 8 == 0, F % 64 == 0, K % 64 == 0, F*K, M*K and
 * F*ldc below 2^31.  A null a / b_gate / b_up / scale_gate / scale_up / c / pa_cache, a scale_gate_n or scale_up_n other than 1 or F, a
 * scale off 4-byte alignment, a K off its multiple, an update_cache outside 0 / 1 or an unknown act returns CHIPMUNK_ERR_INVALID with a
 * message, before anything is enqueued.  No element of a scale at or past its _n is read. */
int chipmunk_csp_mlp_mm1_glu_w8(const void *a, const void *b_gate, const void *b_up, const float *scale_gate, int scale_gate_n,
                                const float *scale_up, int scale_up_n, void *c, const void *bias_gate, const void *bias_up,
                                void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int act,
                                int update_cache, void *stream);
int chipmunk_csp_mlp_mm1_glu_w8_batched(const void *a, const void *b_gate, const void *b_up, const float *scale_gate, int scale_gate_n,
                                        const float *scale_up, int scale_up_n, void *c, const void *bias_gate, const void *bias_up,
                                        void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc,
                                        int act, int update_cache, int B, int64_t cache_batch_stride, void *stream);

/* Weight-only fp8 linear layer for few rows (W8Linear.forward under mlp.w8_stream_rows; no reference counterpart): the weight is read
 * once as e4m3 and widened in registers, no widened copy exists.
 *   x [M, K] bf16, rows ldx elements apart; w [F, K] OCP e4m3 bytes (float8_e4m3fn), plain row-major; scale_b fp32 on the device, the
 *   weight's RECIPROCAL quantisation scale: one number (scale_n == 1) or one per row of w (scale_n == F); bias bf16 [F] or NULL;
 *   y [M, F] bf16, rows ldy elements apart.
 *   S[m,i] = sum_k x[m,k] * f(w[i,k])     f widens e4m3 to bf16 (exact); fp32, from zero, in an order that depends on K and F only
 *   y[m,i] = bf16( bf16( S[m,i] * scale_b[i] ) + bias[i] )      the product and the sum each rounded, never an fma
 *   y[m,i] = bf16( S[m,i] * scale_b[i] )                        without a bias
 * Row independence: the bits of output row m depend on input row m, w, scale_b and bias and on nothing else -- not on M, not on the other
 * rows, not on the row block row m falls in.  K is not split over workgroups, nothing is accumulated with atomics, two launches give
 * the same bits.  Rows of x at and past M are never read; of y only [0, M) x [0, F) is written.
 * Refused with CHIPMUNK_ERR_INVALID and a message, before anything is enqueued: a null x / w / scale_b / y; M < 1, K < 64, F < 8;
 * K % 64 != 0 or F % 8 != 0; M > CHIPMUNK_W8_LINEAR_MAX_M (the grid carries 128 rows per block of its y dimension); a scale_n other than
 * 1 or F; a scale_b off 4-byte alignment; x, w, y or bias off 16-byte alignment; ldx or ldy no multiple of 8 elements; ldx < K or
 * ldy < F.  No element of scale_b at or past scale_n is read. */
#define CHIPMUNK_W8_LINEAR_MAX_M (1 << 20)
int chipmunk_w8_linear(const void *x, int64_t ldx, const void *w, const float *scale_b, int scale_n, const void *bias, void *y,
                       int64_t ldy, int M, int K, int F, void *stream);

/* Group-major cache: the activation cache of one sequence as [G, F, 128] bf16, contiguous, G = ceil(M / 128) -- element (g, i, r) is
 * activation column i of token row g * 128 + r -- instead of the column-major [F, ldc] (no reference counterpart).  The 256-byte pieces of
 * a group's kept columns then lie on a 256-byte grid inside one F * 256-byte window.  Rows of the last group at or past M are never
 * read for a result and never written.  A batch is [B, G, F, 128]: sequence b's block starts at element b * cache_batch_stride, with
 * cache_batch_stride >= G * F * 128 and a multiple of 8 elements (checked for B = 1 as well); nothing outside the blocks is touched.
 * G * F * 128 < 2^31.  Each *_gm entry is its *_batched namesake without `ldc`: same operands, same arithmetic and the same bits for
 * c and for every cache element, B >= 1 with B = 1 the single-sequence launch, B * G <= 65535.  Each failed check returns
 * CHIPMUNK_ERR_INVALID with a message that names the rule, before anything is enqueued. */
int chipmunk_csp_mlp_mm1_act_gm(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                const int32_t *counts, int M, int K, int F, int act, int update_cache, int B,
                                int64_t cache_batch_stride, void *stream);
int chipmunk_csp_mlp_mm1_fp8_act_gm(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                    const int32_t *counts, const float *scale_a, const float *scale_b, int M, int K, int F, int act,
                                    int update_cache, int B, int64_t cache_batch_stride, void *stream);
int chipmunk_csp_mlp_mm1_fp8_act_rs_gm(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                       const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                       int M, int K, int F, int act, int update_cache, int B, int64_t cache_batch_stride,
                                       void *stream);
int chipmunk_csp_mlp_mm1_glu_gm(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K,
                                int F, int act, int update_cache, int B, int64_t cache_batch_stride, void *stream);
int chipmunk_csp_mlp_mm1_glu_fp8_gm(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                    const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts,
                                    const float *scale_a, const float *scale_b_gate, const float *scale_b_up, int M, int K, int F,
                                    int act, int update_cache, int B, int64_t cache_batch_stride, void *stream);
int chipmunk_csp_mlp_mm1_w8_gm(const void *a, const void *b, const float *scale_b, int scale_n, void *c, const void *bias, void *pa_cache,
                               const int32_t *indices, const int32_t *counts, int M, int K, int F, int act, int update_cache, int B,
                               int64_t cache_batch_stride, void *stream);
int chipmunk_csp_mlp_mm1_glu_w8_gm(const void *a, const void *b_gate, const void *b_up, const float *scale_gate, int scale_gate_n,
                                   const float *scale_up, int scale_up_n, void *c, const void *bias_gate, const void *bias_up,
                                   void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int act,
                                   int update_cache, int B, int64_t cache_batch_stride, void *stream);
/* chipmunk_csp_scatter_add_batched on the group-major cache: unpacked_groups[b][g, idx[b,g,j], r] += packed[b, g * 128 + r, j] */
int chipmunk_csp_scatter_add_gm(const void *packed, void *unpacked_groups, const int32_t *indices, const int32_t *counts, int M,
                                int F, int B, int64_t cache_batch_stride, void *stream);
/* [B,R,C] -> [B, ceil(R/128), C, 128] for 16-bit elements: builds the group-major cache of a full step, dst[b, g, c, r] =
 * src[b, g * 128 + r, c], the rows of the last group at or past R zero.  src and dst contiguous and 16-byte aligned. */
int chipmunk_transpose16_groups(const void *src, void *dst, int B, int R, int C, void *stream);

/* ---------------------------------------------------------------- indexed IO
 * Replaces chipmunk::topk_indices (reference csrc/indexed_io/topk_indices.cu:145-218; schema chipmunk.cpp:58).
 * activation [B*R, C] of `dtype`; indices [B*R, C] int32; counts [B*R] int32.  Threshold = element
 * int(1024*sparsity) of the ascending-sorted first 1024 values of the row (:94-101); keep x >= threshold.
 * Deterministic canonical order (a refinement of the reference's atomics-dependent order): kept columns
 * ascending, then padding up to `multiple_of` with "last rejected column of residue t (mod 1024)" for ascending t.
 * random_amount > 0 (cuRAND in the reference) keeps extra columns chosen by a counter-based hash. */
int chipmunk_topk_indices(const void *activation, int dtype, int32_t *indices, int32_t *counts, int rows, int cols,
                          double sparsity_amount, int multiple_of, double random_amount, void *stream);

/* Fused |activation - cache| -> topk_indices -> copy_indices for the sparse-MLP step with bm == mbm (reference
 * src/chipmunk/modules/mlp.py:70-85): ranks the element-wise |delta| (rounded to the tensor dtype like the eager ops),
 * writes indices / counts exactly like chipmunk_topk_indices on that delta, and copies every selected column of
 * `activation` into `cache`.  One kernel instead of abs + sum + topk_indices + copy_indices. */
int chipmunk_topk_delta_indices(const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts,
                                int rows, int cols, double sparsity_amount, int multiple_of, double random_amount,
                                void *stream);

/* chipmunk_topk_indices with a column count per row from the row's mass (not in the reference; config mlp.top_p).
 * For a row of values v_c (the activations as given):
 *   mass     m_c = v_c where v_c > 0; a zero, negative or NaN entry carries none
 *   total    sum of m_c over the whole row (not over the sample); target = float(top_p) * total
 *   thr_p    the largest t with sum{m_c : v_c >= t} >= target, so a class of equal values is taken whole; +inf when total == 0
 *   thr_q    chipmunk_topk_indices' threshold: element int(1024 * sparsity_amount) of the ascending-sorted first 1024 values;
 *            -inf for sparsity_amount == 0 (no cap)
 *   thr_min  the same order statistic at 1 - min_keys (its index never below thr_q's); +inf for min_keys == 0
 *   kept     m_c > 0 and v_c >= min(max(thr_p, thr_q), thr_min)
 * Random keys (a hash draw below random_amount on a column not kept), padding up to multiple_of with rejected columns, the order
 * (kept columns ascending first) and counts (kept + padding) are chipmunk_topk_indices'.  The kept set is a subset of what
 * chipmunk_topk_indices keeps (the cap is a threshold: no tie-break).  An all-zero row keeps nothing (count 0 with random_amount
 * 0; chipmunk_topk_indices keeps the whole row).  sparsity_amount == 1 keeps nothing.  The floor is a sampled quantile like the cap:
 * blind to columns past the first 1024.  0 < top_p <= 1, 0 <= min_keys <= 1 - sparsity_amount, cols >= 1024.
 * The sums are fp32 in one fixed order (a thread's columns ascending, the wave's DPP tree, the 16 wave partials ascending), no
 * floating-point atomics: the same launch gives the same bits, and rows whose sums are exact in fp32 give exactly the rule above. */
int chipmunk_topk_indices_p(const void *activation, int dtype, int32_t *indices, int32_t *counts, int rows, int cols,
                            double sparsity_amount, double top_p, double min_keys, int multiple_of, double random_amount,
                            void *stream);

/* chipmunk_topk_delta_indices with the selection of chipmunk_topk_indices_p: v_c = |T(activation_c - cache_c)| rounded to the element
 * type T; every listed column (padding included) of `activation` is copied into `cache`. */
int chipmunk_topk_delta_indices_p(const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts, int rows,
                                  int cols, double sparsity_amount, double top_p, double min_keys, int multiple_of,
                                  double random_amount, void *stream);

/* chipmunk_topk_delta_indices over several block-mean rows per 128-row group (not in the reference's kernels; its modules/mlp.py:70-85
 * with bm > mbm does this in torch, and the gated MLP pairs gate and up means; config mlp.fused_group_topk_delta).
 * activation, cache [B, rows, cols] of `dtype`; G = ceil(rows / R) groups per sequence, group g owns rows [g*R, min((g+1)*R, rows));
 * indices [B, G, cols] int32; counts [B, G] int32.  The ranked value of column c in a group is
 *   s_c = T( sum_i float( T(|activation_i[c] - cache_i[c]|) ) ),  i ascending over the group's rows, summed in fp32, rounded to T once
 * -- for R == 2 bit for bit what (activation - cache).abs().reshape(B, G, 2, cols).sum(2) gives, for R == 1 chipmunk_topk_delta_indices'
 * value.  Threshold, random keys (hashed on row b*G + g), order, padding and counts are chipmunk_topk_indices' on the row of scores;
 * every listed column (padding included) of `activation` is copied into `cache` in every row the group owns.  sparsity_amount == 0
 * lists and copies everything, == 1 nothing.  cols >= 1024, 1 <= R <= 64, rows >= 1, B*G < 2^31. */
int chipmunk_topk_group_delta_indices(const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts, int B,
                                      int rows, int R, int cols, double sparsity_amount, int multiple_of, double random_amount,
                                      void *stream);

/* ... with the selection of chipmunk_topk_indices_p on the row of scores (the masses are the scores). */
int chipmunk_topk_group_delta_indices_p(const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts, int B,
                                        int rows, int R, int cols, double sparsity_amount, double top_p, double min_keys,
                                        int multiple_of, double random_amount, void *stream);

/* chipmunk_dense_colsum_attn + chipmunk_topk_mask without the cs tensor between them (reference modules/attn.py:131-141 calls
 * dense_colsum_attn, then random_and_topk on its 3.55 GB result at HunyuanVideo size): o, l as chipmunk_dense_colsum_attn,
 * mask [B*H*ceil(Nq/192), Nk] bool bytes as chipmunk_topk_mask would produce from that call's cs -- bit for bit.
 * Returns CHIPMUNK_ERR_UNSUPPORTED without enqueuing anything when the launch would not take the one-pass route in one piece
 * (small launches, Nk % 4 != 0, Nk > 524 288, no room for the partial sums): run the two operators then. */
int chipmunk_dense_colsum_topk_mask(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                                    const int64_t k_strides[3], const int64_t v_strides[3], const float *p, void *o, float *l,
                                    int B, int H, int Nq, int Nk, const void *static_mask, int64_t static_stride, int static_rows,
                                    const void *group_flags, void *mask, int k_top, double random_amount, void *stream);

/* Fused mask construction of the attention mask-building step (reference
 * src/chipmunk/modules/attn.py:76-82 `random_and_topk`):
 *   mask[r, c] = ((c in topk_k(cs[r, :n])) | (u(r, c) < random_amount)) & group_flags[r]  |  static_mask[r % static_rows, c]
 * cs [rows, cs_stride] bf16 column sums; static_mask (optional) bool bytes with row stride static_stride, broadcast over
 * rows modulo static_rows; group_flags (optional) one byte per row; mask [rows, n] bool bytes, fully overwritten.
 * Exactly k columns per active row come from the top-k part; ties at the k-th value are broken deterministically (the
 * reference's torch.topk leaves that choice unspecified); u is a counter-based hash (RNG streams cannot match torch's
 * randint), so results are comparable with the reference chain for random_amount = 0.
 * Ties are taken in ascending order of ((c mod 4096) div 4, c).  n <= 524 288: rows of up to 122 880 columns keep their keys in
 * registers, longer ones take the streaming form of the kernel (same bits; tuning option topk_mask_stream = 1 sends every row there). */
int chipmunk_topk_mask(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                       int static_rows, const void *group_flags, void *mask, int rows, int n, int k,
                       double random_amount, void *stream);

/* chipmunk_topk_mask with a per-row count (not in the reference): an active row keeps the smallest top set of its columns that
 * carries a share top_p of the row's column-sum mass, at least k_min and at most k columns (k clamped to n):
 *   order   bf16 value descending, ties by ((c mod 4096) div 4, c) ascending -- the order chipmunk_topk_mask selects in
 *   mass    m_c = cs[c] where that is positive and finite, 0 otherwise (the contract is finite, non-negative cs);
 *           total = sum of m_c, target = top_p * total
 *   k_p     the smallest count whose prefix of the order has mass >= target; 0 when total is 0
 *   s       min(k, max(k_p, k_min)); the row's top-k part is the first s columns of the order, i.e. chipmunk_topk_mask's for k := s
 * Inactive rows, the random part and the static part are those of chipmunk_topk_mask.  0 < top_p <= 1, k_min >= 0.
 * The sums are fp32 in one fixed order (a thread's columns ascending, the wave's xor tree, the 16 wave totals ascending): the
 * same launch gives the same bits, and rows whose sums are exact in fp32 give exactly the rule above. */
int chipmunk_topk_mask_p(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                         int static_rows, const void *group_flags, void *mask, int rows, int n, int k,
                         double random_amount, double top_p, int k_min, void *stream);

/* chipmunk_dense_colsum_topk_mask_strided with the selection of chipmunk_topk_mask_p (k_top is the cap); o_strides NULL = the
 * plain [B, H, Nq, 128] layout.  CHIPMUNK_ERR_UNSUPPORTED as there: run chipmunk_dense_colsum_attn and chipmunk_topk_mask_p. */
int chipmunk_dense_colsum_topk_mask_p_strided(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                                              const int64_t k_strides[3], const int64_t v_strides[3], const float *p, void *o,
                                              const int64_t *o_strides, float *l, int B, int H, int Nq, int Nk,
                                              const void *static_mask, int64_t static_stride, int static_rows,
                                              const void *group_flags, void *mask, int k_top, double random_amount,
                                              double top_p, int k_min, void *stream);

/* ---- Padded batches: per-sequence key lengths (not in the reference).
 * k_lens: int32 [B] in DEVICE memory (a captured graph replays with whatever it holds then; no call reads it on the host),
 * 1 <= k_lens[b] <= Nk, clamped into that range by the kernels.  For sequence b the keys j >= k_lens[b] do not exist: o, l,
 * the column sums and the mask are those of the same call on K / V cropped to k_lens[b] rows; cs[b, :, :, j] and mask[b, :, :, j]
 * are 0 for j >= k_lens[b].  All Nq query rows are computed.  k_lens == NULL is the entry point without the suffix, bit for bit.
 * No K / V row at or past k_lens[b] is read -- the padding may hold anything, NaN included -- with one exception: launches that
 * take the 64-row kernels (Nk >= 1024 on a full machine; options attn_dense64 / attn_colsum64) read rows 0..63 of a sequence
 * with k_lens[b] < 64, so the FIRST 64 ROWS of K and V must be finite.  Routing is decided on Nk, never on the lengths.
 * Otherwise each entry is its namesake: chipmunk_dense_attn_strided, chipmunk_dense_colsum_attn_strided,
 * chipmunk_dense_colsum_topk_mask_strided, chipmunk_dense_colsum_topk_mask_p_strided (o_strides NULL = plain layout,
 * CHIPMUNK_ERR_UNSUPPORTED as there), chipmunk_topk_mask, chipmunk_topk_mask_p.
 * The mask entries: rows [b * seq_rows, (b + 1) * seq_rows) of cs / mask belong to sequence b (seq_rows = H * groups, rows a
 * multiple of it); a row selects among its first k_lens[b] columns only -- they alone enter the counts, the top-p mass and the tie
 * order, k is capped at k_lens[b] -- and its bytes past them are 0 whatever the random part, the static mask and the group flag say. */
int chipmunk_dense_attn_varlen(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                               const int64_t k_strides[3], const int64_t v_strides[3], void *o, const int64_t *o_strides,
                               float *l, const int32_t *k_lens, int B, int H, int Nq, int Nk, void *stream);
int chipmunk_dense_colsum_attn_varlen(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                                      const int64_t k_strides[3], const int64_t v_strides[3], const float *p, void *o,
                                      const int64_t *o_strides, void *cs, float *l, const int32_t *k_lens, int B, int H,
                                      int Nq, int Nk, int cs_stride, void *stream);
int chipmunk_dense_colsum_topk_mask_varlen(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                                           const int64_t k_strides[3], const int64_t v_strides[3], const float *p, void *o,
                                           const int64_t *o_strides, float *l, const int32_t *k_lens, int B, int H, int Nq,
                                           int Nk, const void *static_mask, int64_t static_stride, int static_rows,
                                           const void *group_flags, void *mask, int k_top, double random_amount, void *stream);
int chipmunk_dense_colsum_topk_mask_p_varlen(const void *q, const void *k, const void *v, const int64_t q_strides[3],
                                             const int64_t k_strides[3], const int64_t v_strides[3], const float *p, void *o,
                                             const int64_t *o_strides, float *l, const int32_t *k_lens, int B, int H, int Nq,
                                             int Nk, const void *static_mask, int64_t static_stride, int static_rows,
                                             const void *group_flags, void *mask, int k_top, double random_amount,
                                             double top_p, int k_min, void *stream);
int chipmunk_topk_mask_varlen(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                              int static_rows, const void *group_flags, void *mask, const int32_t *k_lens, int seq_rows,
                              int rows, int n, int k, double random_amount, void *stream);
int chipmunk_topk_mask_p_varlen(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                                int static_rows, const void *group_flags, void *mask, const int32_t *k_lens, int seq_rows,
                                int rows, int n, int k, double random_amount, double top_p, int k_min, void *stream);

/* Replaces chipmunk::mask_to_indices (reference csrc/indexed_io/mask_to_indices.cu:92-143; schema chipmunk.cpp:60).
 * mask [rows, n] bool bytes; indices [rows, pad_n] int32; counts [rows] int32.  Bit-exact order: True columns of
 * residue class t (mod 32) ascending for t = 0..31, then the first False columns ascending up to multiple_of. */
int chipmunk_mask_to_indices(const void *mask, int32_t *indices, int32_t *counts, int64_t rows, int n, int pad_n,
                             int multiple_of, void *stream);

/* Fused variant: same output from the bit-packed mask (reference ops/bitpack.py:4-40 layout,
 * little-endian, flat) without materialising the bool mask.  Requires n % 8 == 0. */
int chipmunk_packed_mask_to_indices(const void *packed, int32_t *indices, int32_t *counts, int64_t rows, int n,
                                    int pad_n, int multiple_of, void *stream);

/* Same kept set, counts and padding columns as chipmunk_mask_to_indices, but the kept columns come out ASCENDING
 * (packed != 0: input is the bit-packed mask).  Not the reference's order; for consumers that only need the set
 * (the attention kernels): ascending keys make the K/V gather walk DRAM pages in order. */
int chipmunk_mask_to_sorted_indices(const void *mask, int packed, int32_t *indices, int32_t *counts, int64_t rows,
                                    int n, int pad_n, int multiple_of, void *stream);

/* The same rows written straight into the ragged layout of chipmunk_csp_attn_out_ragged, without the padded [rows, pad_n] tensor
 * (no reference counterpart).  chipmunk_mask_row_counts: counts[r] = kept columns of row r rounded up to multiple_of (what the three
 * entries above write; it may exceed n) and lengths[r] = min(counts[r], pad_n) rounded up to 32, the row's width in `flat`.  The
 * caller turns the lengths into offsets (offsets[0] = 0, offsets[r + 1] = offsets[r] + lengths[r]) and allocates flat.
 * chipmunk_mask_to_ragged_indices: flat[offsets[r] ...] = the kept columns of row r (sorted != 0: ascending, else the reference's
 * order), then the first False columns ascending up to counts[r] while there are any, then zeros up to offsets[r + 1]; nothing
 * is written past a row's width.  packed != 0: the mask is bit-packed, n % 8 == 0.  flat 16-byte aligned. */
int chipmunk_mask_row_counts(const void *mask, int packed, int32_t *counts, int64_t *lengths, int64_t rows, int n, int pad_n,
                             int multiple_of, void *stream);
int chipmunk_mask_to_ragged_indices(const void *mask, int packed, int sorted, const int64_t *offsets, int32_t *flat, int64_t rows,
                                    int n, int multiple_of, void *stream);

/* Replaces chipmunk::copy_indices (reference csrc/indexed_io/copy_indices.cu:82-154; schema chipmunk.cpp:57).
 * dst[b,row,idx] = src[b,row,idx] for the first counts[b,row/R] entries of inds[b,row/R,:]; elem_size 2 or 4. */
int chipmunk_copy_indices(const void *src, void *dst, const int32_t *inds, const int32_t *counts, int B, int M, int R,
                          int F, int elem_size, void *stream);

/* [B,R,C] -> [B,C,R] for 16-bit elements: builds the column-major activation cache `pa.transpose(-1,-2).contiguous()`
 * of the sparse MLP's full step (reference src/chipmunk/modules/mlp.py:56) at HBM rate. */
int chipmunk_transpose16(const void *src, void *dst, int B, int R, int C, void *stream);
/* ... with an output pitch: dst is [B, C, ld], ld >= R; elements [R, ld) of every output row are written as zeros (the activation
 * cache of a token count that is not a multiple of 8, see the *_ragged MLP entries). */
int chipmunk_transpose16_pitched(const void *src, void *dst, int B, int R, int C, int ld, void *stream);

/* [rows, C] bf16 -> [rows / mbm, C] bf16: mean over consecutive blocks of `mbm` rows, fp32 sums, one rounding (the caller's
 * `block_mean(x, mbm)` in front of the fc1 probe of every sparse MLP step, src/chipmunk/modules/mlp.py:11-16,62).  rows % mbm == 0,
 * mbm % 4 == 0, C % 8 == 0. */
int chipmunk_block_mean(const void *x, void *out, int64_t rows, int C, int mbm, void *stream);
/* ... for any rows > 0: out is [ceil(rows / mbm), C] and the last block is the mean over the rows present (fp32 sum, one rounding). */
int chipmunk_block_mean_ragged(const void *x, void *out, int64_t rows, int C, int mbm, void *stream);

/* bf16 [n] -> OCP fp8 e4m3 [n]: F8Linear.quantize_input's `(x * scale).clamp(-max, max).to(float8_e4m3fn)` (reference
 * src/chipmunk/modules/mlp_fp8.py, the input side of csp_mlp_mm1_fp8) as one pass with the same roundings (fp32 product -> bf16 -> clamp ->
 * e4m3, round-to-nearest-even).  scale: one float on the device.  n % 8 == 0. */
int chipmunk_quantize_fp8(const void *x, const float *scale, void *out, int64_t n, float max_value, void *stream);

/* bf16 [rows, K] -> OCP fp8 e4m3 [rows, K] with one dynamic scale per row (F8Linear.quantize_input_rowwise; no reference counterpart), in
 * one pass over HBM.  Per row r, in fp32 with IEEE division:
 *   amax = max_k |x[r,k]|;  scale = min(max_value / max(amax, 1e-12), max_value)
 *   out[r,k] = e4m3_rne( clamp(float(x[r,k]) * scale, -max_value, max_value) );  scale_recip[r] = 1 / scale
 * The product is fp32 and rounded once, into e4m3: torch's `x.float() * scale[:, None]` chain, NOT chipmunk_quantize_fp8's (which rounds
 * the product to bf16 first, as torch's bf16 x 0-dim product does).  scale_recip is fp32 [rows], the number GEMM1 multiplies its sums by.
 * rows >= 0, K % 16 == 0, K <= CHIPMUNK_QUANTIZE_ROWWISE_MAX_K; x 16-byte, out 8-byte, scale_recip 4-byte aligned; anything else returns
 * CHIPMUNK_ERR_INVALID before anything is enqueued.  A row that holds a NaN or an Inf is outside the contract: its bytes and its scale
 * are unspecified. */
#define CHIPMUNK_QUANTIZE_ROWWISE_MAX_K 16384
int chipmunk_quantize_fp8_rowwise(const void *x, void *out, float *scale_recip, int64_t rows, int K, float max_value, void *stream);

/* bitpack / bitunpack (reference src/chipmunk/ops/bitpack.py:4-69): 8 bools -> 1 byte, little-endian, flat. */
int chipmunk_bitpack(const void *mask, void *packed, int64_t n, void *stream);
int chipmunk_bitunpack(const void *packed, void *mask, int64_t n, void *stream);

/* ---------------------------------------------------------------- token reorder
 * dst[o, i, :] = src[o, map[i], :] for o < outer, i < n_out; rows of `row_bytes` bytes, src has n_src rows per outer
 * index.  One gather for each of the reference's token reorders -- patchify / unpatchify / patchify_rope
 * (src/chipmunk/ops/patch.py:7-80) and voxel_chunk_no_padding / reverse_voxel_chunk_no_padding
 * (src/chipmunk/ops/voxel.py:9-99) -- whose permutations the host side computes once per shape. `map` int32 [n_out]. */
int chipmunk_gather_rows(const void *src, void *dst, const int32_t *map, int64_t outer, int64_t n_src, int64_t n_out,
                         int64_t row_bytes, void *stream);

/* ---------------------------------------------------------------- pinned host offload pool
 * Replaces the reference's per-layer pinned CPU buffers and its two module-level CUDA streams' copies
 * (src/chipmunk/util/storage/offloaded_tensor.py:12-13 the streams, :42-44,71 `torch.empty(..., pin_memory=True)`, :104-118 and
 * :140-160 `copy_(non_blocking=True)`): hipHostMalloc'd buffers owned by the library and hipMemcpyAsync on the caller's side stream.
 * chipmunk_host_alloc: page-locked host memory (hipHostMallocDefault); chipmunk_host_free gives it back (the caller makes sure no copy
 * on it is in flight).  chipmunk_copy_d2h_async / _h2d_async: one hipMemcpyAsync of `bytes` contiguous bytes on `stream` (a dense
 * permuted tensor travels as its storage); ordering against other streams is the caller's (events), as in the reference.
 * chipmunk_host_bytes: bytes currently allocated through chipmunk_host_alloc (diagnostic). */
int chipmunk_host_alloc(size_t bytes, void **host_ptr);
int chipmunk_host_free(void *host_ptr);
int chipmunk_copy_d2h_async(void *host_dst, const void *dev_src, size_t bytes, void *stream);
int chipmunk_copy_h2d_async(void *dev_dst, const void *host_src, size_t bytes, void *stream);
size_t chipmunk_host_bytes(void);

/* Gives back the library's device scratch (work plans, split partials, the multi-GB partial column sums of the fused
 * dense_colsum_attn pass -- bounded by option "big_scratch_gb", default 24).  Synchronises the device. */
int chipmunk_release_scratch(void);
/* How many requests for the multi-GB column-sum scratch were refused since the last release (each one sent a dense_colsum_attn /
 * dense_colsum_topk_mask call down the slower two-pass or chunked route): 0 in a healthy run. */
int chipmunk_big_scratch_fallbacks(void);

/* ---------------------------------------------------------------- projection output -> attention operands
 * qkv [n rows of row_stride elements, the first 3*heads*128 of each = (q|k|v, head, 128)] bf16  ->  q, k, v [heads, n, 128] bf16
 * with RMSNorm over the 128 head elements applied to q and k: bf16(bf16(x * rsqrt(mean(x^2) + eps)) * weight); weights bf16
 * [128] or NULL (= ones).  Optionally the rotary embedding of q and k for the first rope_rows tokens (the image tokens;
 * apply_rotary_emb, posemb_layers.py:133-172, (cos, sin) form): bf16(x * cos + rotate_half(x) * sin) in fp32, freqs_cos /
 * freqs_sin fp32 [rope_rows, 128] or both NULL.  One pass instead of the caller's rearrange + two RMSNorm modules + rotary
 * embedding + three transposes (examples/hunyuan/hyvideo/modules/models.py:188-199,376-392; norm_layers.py:43-58). */
int chipmunk_qkv_split_norm(const void *qkv, int64_t row_stride, const void *q_weight, const void *k_weight, void *q, void *k,
                            void *v, int64_t n, int heads, float eps, const float *freqs_cos, const float *freqs_sin,
                            int64_t rope_rows, void *stream);

/* ---------------------------------------------------------------- Wan attention operands: row-wide RMSNorm + rotary, one pass
 * x [B, n rows of row_stride elements, batch_stride elements apart] bf16; the first parts * heads * 128 columns of a row are
 * `parts` (1 .. 3) consecutive blocks of C = heads * 128 columns (q | k | v), columns behind them are never read.  Part p goes to
 * out_p [B, heads, n, 128] bf16 (contiguous).  Per part, independently:
 *   - bit p of norm_mask: WanRMSNorm over the WHOLE row of C values (examples/wan/wan/modules/model.py:81-97, not per head as
 *     chipmunk_qkv_split_norm): r = 1 / sqrt(mean(x^2) + eps) in fp32, y = bf16(x * r);
 *   - a weight [C] for a normalised part, w_p with dtype code 0 (none, w_p NULL), 1 (bf16: bf16(y * w)) or 2 (fp32: y * w kept in
 *     fp32, torch's promotion -- what Wan computes with fp32 parameters);
 *   - bit p of rope_mask: for tokens < rope_rows the pair (2i, 2i+1) = (re, im) becomes (re * c - im * s, re * s + im * c) in fp32
 *     (rope_apply, model.py:49-78, which multiplies in fp64), c / s from freqs_cos / freqs_sin fp32 [rope_rows, 128] -- both
 *     entries of a pair carry the pair's angle, the table format of chipmunk_qkv_split_norm -- shared by all heads and batches.
 * Every value is rounded once more, to bf16, when it is stored (model.py:164).  A part with neither bit set is a bit copy into
 * the head-major layout (v).  heads in 1 .. 64; pointers 16-byte aligned, strides multiples of 8 elements; both tables or
 * neither; rope_rows <= n.  Sums run in a fixed order: launches are bit-reproducible, and a row's result does not depend on B.
 * The cross-attention operands (model.py:195-196, 236-239) are the same call without a rotation. */
int chipmunk_split_heads_rownorm(const void *x, int64_t batch_stride, int64_t row_stride, int parts, const void *w0, int w0_dtype,
                                 const void *w1, int w1_dtype, const void *w2, int w2_dtype, void *out0, void *out1, void *out2,
                                 unsigned norm_mask, unsigned rope_mask, int64_t B, int64_t n, int heads, float eps,
                                 const float *freqs_cos, const float *freqs_sin, int64_t rope_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CHIPMUNK_HIP_H */
