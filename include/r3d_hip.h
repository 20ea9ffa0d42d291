/* libr3d_hip.so -- C ABI of the MI355X (gfx950) kernels behind R3D's RGB+Depth token-fusion training step.
 *
 * The reference (olivesgatech/R3D) is pure Python on stock PyTorch ops and has NO FFI / plugin API of its own
 * (SURVEY.md F3, 8(b)); every entry point below therefore replaces an ATen op *sequence* of the reference and cites
 * the reference lines it stands in for (paths relative to the reference root).  The host side that calls them
 * (r3d_amd/engine.py via ctypes) mirrors the reference's Python surface (FUTR / train / opts); INTEGRATION.md shows
 * the binding a maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes, no torch types; every pointer is DEVICE memory owned by the caller
 *     (PyTorch's caching allocator in practice), fp32 unless stated, row-major with explicit leading dimensions;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); work is only ENQUEUED on it:
 *     no device synchronisation, no device allocation, no host<->device copies, no mutable globals
 *     -> safe under hipGraph capture and from autograd's backward thread (one process per GPU);
 *   - return 0 on success, a negative R3D_E* code for a rejected argument, or the positive hipError_t of a failed launch;
 *   - rows of activations are ordered (clip b, frame s) b-major: row = b*S + s.  The reference's seq-first [S,B,H]
 *     tensors (model/futr_safuser_tokenfusion.py:201-204) are the same data indexed the other way round.
 */
#ifndef R3D_HIP_H
#define R3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3D_ABI_VERSION 2

/* ---- error codes ---------------------------------------------------------------------------------------- */
#define R3D_OK 0
#define R3D_EINVAL (-1)
#define R3D_EALIGN (-2)
#define R3D_ENORCCL (-3)      /* r3d_allreduce_flat: no RCCL is mapped into the process */
#define R3D_ERCCL_BASE (-100) /* r3d_allreduce_flat: ncclResult_t r is returned as R3D_ERCCL_BASE - r */

int r3d_abi_version(void);
/* Writes up to `cap` bytes "gfx950;<build info>" -- used by the host to fail loudly on a stale library. */
int r3d_build_info(char* buf, int cap);

/* ---- gradient exchange (data parallel; replaces the per-step nn.DataParallel gather through device 0, main_darai.py:129-133)
 * In-place sum of buf[0..count) (fp32) over the ranks of `comm` (an ncclComm_t the caller created, e.g. r3d_amd.rccl.RcclComm):
 * ncclAllReduce of the RCCL copy already loaded in the process (PyTorch's), enqueued on `stream` like every other entry
 * point -- one more kernel in stream order, capturable into the step's hipGraph.  1/world is folded into
 * r3d_adamw_flat's grad_scale.  The library itself does not link RCCL. */
int r3d_allreduce_flat(float* buf, int64_t count, void* comm, void* stream);

/* ---- GEMM family ------------------------------------------------------------------------------------------
 * One fp32-exact MFMA GEMM (v_mfma_f32_32x32x2_f32, LDS-staged k-major tiles) carries every dense contraction of
 * the step: nn.Linear forward  (layout NT: model/futr_safuser_tokenfusion.py:179,195,222-231;
 * model/extras/transformerblock.py:21,34,84-88; nn.MultiheadAttention in/out projections and FFN of
 * model/extras/transformer.py:289-327), its input gradient (NN) and its weight gradient (TN) -- the ops autograd
 * derives for the reference at train/train_proposed_depth.py:214.
 *
 *   layout R3D_GEMM_NT: C[M,N] = A[M,K] . B[N,K]^T      (A rows lda, B rows ldb; both K-contiguous)
 *   layout R3D_GEMM_NN: C[M,N] = A[M,K] . B[K,N]
 *   layout R3D_GEMM_TN: C[M,N] = A[K,M]^T . B[K,N]
 *
 * Prologue on A (NT/NN only): row m is read from row (m ^ a_row_xor) and, if a_add != NULL,
 *   A'[m,k] = A[m^xor,k] + a_add[(m % a_add_mod), k]   (broadcast add of positional / query embeddings,
 *   model/extras/transformer.py:289,300-302).
 * Epilogue, in this order:  v = alpha*acc (+ bias[n]);  pre_out[m,n] = v (if given);
 *   act: 0 none | 1 relu | 2 exact-erf gelu;  v *= drop_scale*drop_mask[m,n] (if given);
 *   mul: 0 none | 1 v *= (aux[m,n] > 0) | 2 v *= gelu'(aux[m,n])         (backward of relu / gelu);
 *   v += res1[m,n] + res2[m,n] (if given);  if (accumulate) v += C[m,n];  C[m,n] = v.
 *   c_row_xor = 1 applies the whole epilogue at row m^1 instead of m: the modality swap that the fuser's masked
 *   2-token attention reduces to (softmax([[-inf,s],[s,-inf]]) = [[0,1],[1,0]] exactly; SURVEY.md F5b,
 *   model/extras/transformerblock.py:24-33 under the mask of model/futr_safuser_tokenfusion.py:68-72).
 * splitk > 1: the K range is cut into `splitk` slabs of k_per_split (multiple of 16); raw partial sums go to
 *   `partial` ([splitk][M][N] floats, caller-owned) and r3d_splitk_reduce*() applies the epilogue.
 */
#define R3D_GEMM_NT 0
#define R3D_GEMM_NN 1
#define R3D_GEMM_TN 2

typedef struct r3d_gemm_desc {
    const float* A; const float* B; float* C;
    int32_t layout, M, N, K;
    int32_t lda, ldb, ldc;
    const float* a_add; int32_t a_add_mod, a_add_ld, a_row_xor;
    const float* b_add; int32_t b_add_mod, b_add_ld;   /* NN/TN only: B'[k,:] = B[k,:] + b_add[k % mod,:] */
    const float* bias;
    float* pre_out; int32_t ldpre;
    int32_t act;
    const uint8_t* drop_mask; int32_t lddrop; float drop_scale;
    const float* aux; int32_t ldaux, mul;
    const float* res1; int32_t ldr1;
    const float* res2; int32_t ldr2;
    float alpha; int32_t accumulate;
    float* bias_grad;        /* TN only, splitk == 1: bias_grad[m] = sum_k A[k,m] (the nn.Linear bias gradient, free
                                 with the weight-gradient GEMM that already streams dY through LDS) */
    int32_t c_row_xor;       /* output (and pre_out/aux/res/drop operand) row index = m ^ c_row_xor: pair swap at store */
    int32_t splitk, k_per_split; float* partial;
    int32_t tile;            /* 0 = auto; workgroup tile: 1 = 32x32 (4 k-split waves), 2 = 64x64, 3 = 128x128,
                                4 = 64x64 with 2 k-split wave groups, 5 = 128x128 with 2 k-split wave groups,
                                10 = TN product with 128 x 128 tiles on the bf16 matrix cores (prec == 1; M, N, lda, ldb % 4 == 0,
                                    alpha / accumulate epilogue or adam_*: the depth weight gradient beyond tile 7's limits),
                                12 = tile 10's kernel with ONE LDS stage and <= 128 registers: two workgroups per CU (the planner's pick),
                                11 = tile 9 with uniform waves (kept for measurement),
                                8 / 9 = split-K NT product with 64 x 64 / 128 x 128 tiles on the bf16 matrix cores (prec == 1,
                                    K % 8 == 0, 16-byte aligned K-contiguous operands, no prologue: the forward depth projection),
                                7 = tile 6 on the bf16 matrix cores (prec == 1),
                                6 = persistent 64-column panels with A^T resident in registers (TN, K <= 128, M <= 128,
                                    plain epilogue: the weight gradient of a wide layer from few rows) */
    int32_t vec;             /* filled by the library: operands allow 16-byte loads */
    /* AdamW in the epilogue (adam_m != NULL; weight-gradient GEMMs with splitk == 1, tile 2, 3 or -- TN, prec == 1 -- 10 / 12,
     * N % 4 == 0, 16-byte aligned C / moments, no other epilogue operand): the
     * product alpha * A.B is the GRADIENT and is not stored; C is the PARAMETER, adam_m / adam_v its moments (same
     * layout and ldc), all three updated in place exactly as r3d_adamw_flat would (lr, step: device scalars).  Saves the
     * gradient's write and re-read and one pass over the parameter: depth_projection.weight is 86 % of the model. */
    float* adam_m; float* adam_v; const float* adam_lr; const int64_t* adam_step;
    float adam_beta1, adam_beta2, adam_eps, adam_wd, adam_gscale;
    int32_t prec;            /* 0: v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain).  1: the kernels that have one may take the
                                 bf16x3 path: every fp32 operand split EXACTLY into three bf16 terms, the six leading
                                 products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (error per product <= 3 * 2^-24,
                                 the size of an fp32 rounding; 2.7x less matrix-core time).  Today: tile 7 = tile 6's
                                 persistent weight-gradient panels, chosen by r3d_gemm_plan when prec == 1 */
} r3d_gemm_desc;

int r3d_gemm_f32(const r3d_gemm_desc* d, void* stream);
/* Sums the split-K slabs of a previous r3d_gemm_f32(d with splitk>1) and applies d's epilogue. */
int r3d_splitk_reduce(const r3d_gemm_desc* d, void* stream);
/* Workspace floats r3d_gemm_f32 needs in d->partial for this (M,N,splitk). */
int64_t r3d_gemm_partial_floats(int32_t M, int32_t N, int32_t splitk);
/* Two split-K NT products with the same M x N, both on tile 8 (prec == 1; K % 8 == 0, k_per_split % 64 == 0, partial set and
 * distinct), in ONE launch: the second product's K-splits take the workgroups after the first's; the raw slabs of both are left
 * for the caller's reducer (r3d_embed_fuse_fwd: the depth projection and the RGB embedding of
 * model/futr_safuser_tokenfusion.py:179,194-195 side by side). */
int r3d_gemm_bf3_nt_pair(const r3d_gemm_desc* first, const r3d_gemm_desc* second, void* stream);
/* Heuristic the host uses to pick (tile, splitk, k_per_split) for a shape on a 256-CU part; fills the desc. */
int r3d_gemm_plan(r3d_gemm_desc* d);
/* Grouped launch: n independent problems of one layout in ONE kernel (all weight gradients of a step; each is
 * latency-bound, so the ~5 us per-launch floor dominates, not the FLOPs).  prepare() (host only) validates the
 * descriptors, fills tile/vec and prefix[0..n] (first workgroup of each problem; prefix[n] = grid size); the caller
 * copies both arrays to device memory once per shape and calls launch() every step. */
int r3d_gemm_grouped_prepare(r3d_gemm_desc* descs, int n, int tile, int32_t* prefix);
/* host_prefix (optional): the HOST copy of prefix[0..n]; with it, groups of <= 32 problems carry the table in the kernel
 * arguments and a workgroup finds its problem without touching memory (the device-side search is a chain of dependent
 * scalar loads in front of every workgroup's first operand load). */
int r3d_gemm_grouped_launch(const r3d_gemm_desc* dev_descs, const int32_t* dev_prefix, const int32_t* host_prefix, int n,
                            int total_tiles, int layout, int tile, void* stream);

/* ---- row-wise kernels ---------------------------------------------------------------------------------------
 * LayerNorm (eps 1e-5, biased variance, affine): depth_layernorm (model/futr_safuser_tokenfusion.py:147,196),
 * Block.norm1/norm2 (model/extras/transformerblock.py:122,127,131-134), fuser.norm (:25,93), decoder norm1/2/3 and
 * decoder.norm (model/extras/transformer.py:265-267,292-329,182-183).
 *
 * r3d_layernorm_fwd: y = act(LN(x)), saves mean/rstd per row.
 *   nsplit > 0: x is the [nsplit][rows][H] split-K slab buffer of r3d_gemm_f32; the slabs are summed, `bias` added and
 *     the sum (the nn.Linear output) stored to pre_out before normalising -- fuses depth_projection's reduction with
 *     depth_layernorm + ReLU (:195-197).
 *   pair_out != NULL: rows come in (token, modality) pairs and pair_out[n] = (y[2n] + y[2n+1]) / 2, the
 *     torch.mean(x, dim=1) over the two modality tokens (:94).
 * r3d_layernorm_bwd: dx = LN'(dy) [+ add1 + add2]; dgamma/dbeta written (not accumulated).
 *   dy2 (optional, same shape as x) is added to dy first (a second consumer of the LN output);
 *   pair_in: dy holds one row per pair and each row of the pair receives dy/2 (backward of the mean above);
 *   relu: dy is first masked by [LN(x) > 0] (recomputed);  dx2 (optional) = dx * drop_scale * drop_mask;
 *   ws: r3d_layernorm_bwd_ws_floats(rows, H) floats of scratch (0 when rows <= 64).
 */
int r3d_layernorm_fwd(const float* x, int ldx, int nsplit, const float* bias, float* pre_out, const float* gamma,
                      const float* beta, float* y, int ldy, float* mean, float* rstd, float* pair_out, int rows, int H,
                      int relu, void* stream);
int64_t r3d_layernorm_bwd_ws_floats(int rows, int H);
int r3d_layernorm_bwd(const float* dy, int lddy, int pair_in, const float* dy2, int lddy2, const float* x, int ldx,
                      const float* mean,
                      const float* rstd, const float* gamma, const float* beta, int relu, const float* add1, int ldadd1,
                      const float* add2, int ldadd2, float* dx, int lddx, float* dx2, int lddx2,
                      const uint8_t* drop_mask, int lddrop, float drop_scale, float* dgamma, float* dbeta, float* ws,
                      int rows, int H, int defer_finalize, void* stream);
/* With defer_finalize != 0 the reduction of the per-block partial dgamma/dbeta left in ws is done later by this call
 * (so the host can take it off the critical path). */
int r3d_layernorm_bwd_finalize(const float* ws, int rows, int H, float* dgamma, float* dbeta, void* stream);
/* Up to 4 independent LayerNorm sites of the same width in ONE launch (what a step saves is the dependent launch, ~5 us).
 * The job structs carry exactly the arguments of r3d_layernorm_fwd / r3d_layernorm_bwd (backward: ws must be given when
 * the site needs it -- parameter reductions are always deferred to r3d_layernorm_bwd_finalize*; rows_per_block and
 * nblocks are filled by the library).  Host arrays; copied into the kernel argument. */
typedef struct r3d_ln_fwd_job {
    const float* x; int32_t ldx, nsplit; const float* bias; float* pre_out;
    const float* gamma; const float* beta; float* y; int32_t ldy; float* mean; float* rstd;
    float* pair_out; int32_t rows, H, relu;
} r3d_ln_fwd_job;
typedef struct r3d_ln_bwd_job {
    const float* dy; int32_t lddy, pair_in; const float* dy2; int32_t lddy2;
    const float* x; int32_t ldx; const float* mean; const float* rstd; const float* gamma; const float* beta; int32_t relu;
    const float* add1; int32_t ldadd1; const float* add2; int32_t ldadd2;
    float* dx; int32_t lddx;
    float* dx2; int32_t lddx2; const uint8_t* drop_mask; int32_t lddrop; float drop_scale;
    float* dgamma; float* dbeta; float* ws;
    int32_t rows, H, rows_per_block, nblocks;
} r3d_ln_bwd_job;
int r3d_layernorm_fwd_multi(const r3d_ln_fwd_job* jobs, int njobs, void* stream);
int r3d_layernorm_bwd_multi(r3d_ln_bwd_job* jobs, int njobs, void* stream);
/* r3d_layernorm_bwd_multi (hidden <= 128) carrying an INDEPENDENT small attention backward (the arguments of
 * r3d_mha_core_bwd; 8 queries, dh 16, <= 64 keys) as extra workgroups: the backward of decoder layer 0's query
 * self-attention feeds parameter gradients only and rides beside the fuser's norm2 backward. */
typedef struct r3d_mha_bwd_job {
    const float* q; int32_t ldq; const float* k; int32_t ldk; const float* v; int32_t ldv;
    const float* probs; const uint8_t* drop_mask; float drop_scale;
    const float* d_o; int32_t lddo; float* dq; int32_t lddq; float* dk; int32_t lddk; float* dv; int32_t lddv;
    int32_t B, heads, Lq, Lk, dh;
} r3d_mha_bwd_job;
int r3d_layernorm_bwd_multi_mha(r3d_ln_bwd_job* jobs, int njobs, const r3d_mha_bwd_job* mha, void* stream);
/* The same for many LayerNorm sites in one launch; jobs live in device memory. */
/* rows > 0: ws holds the partials r3d_layernorm_bwd left for that many rows; rows < 0: exactly -rows (dgamma, dbeta)
 * pairs [-rows][2][H] written by another producer (r3d_embed_fuse_bwd). */
typedef struct r3d_ln_finalize_job { const float* ws; float* dgamma; float* dbeta; int32_t rows, H; } r3d_ln_finalize_job;
int r3d_layernorm_bwd_finalize_batched(const r3d_ln_finalize_job* dev_jobs, int njobs, int max_H, void* stream);
/* out[c] (+)= sum_r x[r,c]: bias gradients.  ws: r3d_colsum_ws_floats(rows, cols) floats. */
int64_t r3d_colsum_ws_floats(int rows, int cols);
int r3d_colsum(const float* x, int ld, int rows, int cols, float* out, float* ws, int accumulate, void* stream);
/* out[r,c] (+)= sum over rows with row % mod == r: gradients of query_embed / pos_embedding, which the forward
 * broadcasts over clips (model/futr_safuser_tokenfusion.py:190,205-209). */
int r3d_rowmod_sum(const float* x, int ld, int rows, int cols, int mod, float* out, int ldo, int accumulate,
                   void* stream);

/* Batched form: job j writes dst[r,:] = sum over rows with row % mod == r of (src1 [+ src2]); mod == 1 is a bias gradient. */
typedef struct r3d_rowsum_job { const float* src1; const float* src2; float* dst; int32_t ld1, ld2, ldd, rows, cols, mod; } r3d_rowsum_job;
int r3d_rowmod_sum_batched(const r3d_rowsum_job* dev_jobs, int njobs, int max_cols, int max_mod, void* stream);
/* ++*a, ++*b (either may be NULL): step counter and dropout offset in one launch. */
int r3d_tick(int64_t* a, int64_t* b, void* stream);
/* out[r,:] = x[r,:] + add[r % mod,:]: with_pos_embed (model/extras/transformer.py:278-279,289,300-302); x may be NULL. */
int r3d_add_rowbcast(const float* x, int ldx, const float* add, int ldadd, int mod, float* out, int ldo, int rows, int cols,
                     void* stream);

/* ---- nn.Linear -> dropout -> residuals -> LayerNorm in ONE launch (gemm_ln.hip; hidden size 128) ----------------
 * y = LN(pre), pre = drop_scale * drop_mask * (A . W^T + bias) + res1 + res2      (A [M,K], W [H,K], both K-contiguous)
 * -- the sub-layer epilogues of model/extras/transformerblock.py:131-134 (attn.proj + x -> norm2; mlp fc2 + x),
 * model/futr_safuser_tokenfusion.py:92-94 (+ x_res -> norm -> mean over the two modality tokens: pair_out[n] =
 * (y[2n] + y[2n+1]) / 2) and model/extras/transformer.py:292-293,304-306 (out_proj -> dropout -> + tgt -> norm1 / norm2).
 * A workgroup owns 16 complete rows, so the LayerNorm is the GEMM's epilogue: one dependent launch and one memory round
 * trip of the pre-norm rows less per site than r3d_gemm_f32 + r3d_layernorm_fwd.  pre_out (the LayerNorm's input, read
 * by the backward), mean and rstd are written exactly as those two entry points write them.  K == 0: no product, the
 * rows already in pre_out are normalised (a plain LayerNorm job riding in the same launch).  Up to 4 jobs per launch.
 * Requirements (r3d_gemm_ln_supported): H == 128, M % 16 == 0, K in {0, 128, 256, 384, 512}, A / W 16-byte aligned with lda, ldw % 4 == 0.
 */
typedef struct r3d_gemm_ln_job {
    const float* A; int32_t lda;
    const float* W; int32_t ldw;
    const float* bias;
    const uint8_t* drop_mask; int32_t lddrop; float drop_scale;
    const float* res1; int32_t ldr1;
    const float* res2; int32_t ldr2;
    float* pre_out; int32_t ldpre;
    const float* gamma; const float* beta;
    float* y; int32_t ldy; float* mean; float* rstd;
    float* pair_out;
    int32_t M, K;
} r3d_gemm_ln_job;
int r3d_gemm_ln_supported(int M, int K, int H);
int r3d_gemm_ln_fwd(const r3d_gemm_ln_job* jobs, int njobs, int H, void* stream);
/* The same launch carrying an INDEPENDENT small attention core (the arguments of r3d_mha_core_fwd; heads * 8 queries, dh 16,
 * <= 64 keys: r3d_gemm_ln_mha_supported) as extra workgroups: the query self-attention of decoder layer 0
 * (model/extras/transformer.py:289-291 with tgt = 0, model/futr_safuser_tokenfusion.py:205-209) depends on parameters only,
 * so it needs no launch of its own and rides beside the fuser's attn.proj + norm2. */
typedef struct r3d_mha_job {
    const float* q; int32_t ldq; const float* k; int32_t ldk; const float* v; int32_t ldv;
    const uint8_t* key_padding_mask; const int64_t* key_label; int32_t pad_idx;
    float* probs; const uint8_t* drop_mask; float drop_scale; float* o; int32_t ldo;
    int32_t B, heads, Lq, Lk, dh;
} r3d_mha_job;
int r3d_gemm_ln_mha_supported(int heads, int Lq, int Lk, int dh);
int r3d_gemm_ln_mha_fwd(const r3d_gemm_ln_job* jobs, int njobs, int H, const r3d_mha_job* mha, void* stream);

/* ---- the SA-Fuser block and its row-local neighbourhood as ONE launch (csrc/fuser_chain.hip; hidden = 128) -------------
 * Fuser role, 16 token rows (8 frames) per workgroup:  V = h1 Wv^T stored pair-swapped (the closed form of the masked
 * 2-token attention, model/futr_safuser_tokenfusion.py:68-72,77) -> x1 = x0 + vsw Wproj^T + b -> h2 = norm2(x1) ->
 * u = h2 W1^T + b1, f1 = GELU(u) -> x3 = x1 (+ x0 when add_xres) + f1 W2^T + b2 -> y = fuser.norm(x3) ->
 * fused = mean of the token pair (model/extras/transformerblock.py:118-135, model/futr_safuser_tokenfusion.py:83-94) ->
 * seg = fused Wseg^T + b (:228-232), cakv = (fused + pos[frame %% S]) Wkv^T + b (model/extras/transformer.py:300-302).
 * Query role, 2 clips per workgroup (decoder layer 0 with tgt = 0, transformer.py:289-293,300):
 * sa_qkv = qpos Win^T + b -> attention core (probabilities p_sa, dropout drop_sa) -> t1_pre = dropout(sa_o Wout^T + b) ->
 * t1 = norm1(t1_pre) -> caq = (t1 + qpos) Wq^T + b.
 * All matrices row-major and dense: activations [2N, 128] (u, f1: [2N, 512]; fused [N, 128]; seg [N, K]; cakv [N, 256];
 * sa_qkv [B*Q, 384]), weights as nn.Linear stores them ([out, in]).  y may be NULL.  Requirements:
 * r3d_fuser_chain_supported. */
typedef struct r3d_fuser_chain_fwd_args {
    const float* x0; const float* h1;
    const float* wv; const float* wproj; const float* bproj; const float* g2; const float* be2;
    const float* w1; const float* b1; const float* w2; const float* b2; const float* gf; const float* bef;
    const float* pos; const float* wkv; const float* bkv; const float* wseg; const float* bseg;
    float* vsw; float* x1; float* h2; float* m2; float* r2; float* u; float* f1; float* x3; float* y; float* mf; float* rf;
    float* fused; float* seg; float* cakv;
    const float* qpos; const float* w_in; const float* b_in; const float* w_out; const float* b_out; const float* g1;
    const float* be1; const float* wq; const float* bq;
    const uint8_t* drop_sa; const uint8_t* drop_d1; float drop_scale;
    float* sa_qkv; float* p_sa; float* sa_o; float* t1_pre; float* t1; float* m1; float* r1; float* caq;
    int32_t N, S, K, H, add_xres, B, Q, heads;
    uint64_t* timeline;      /* profiling aid, normally NULL: wave 0 of the first workgroup of each role stores wall_clock64()
                                (100 MHz) at its stage boundaries -- fuser role [0..15], query role [16..31] */
    /* optional (all or none): bf16x3 operand-order planes (r3d_weight_planes) of wv, wproj, w1, w2, wkv, wseg as
     * B[n = output column][k = input column] -- the fuser role then runs on the bf16 matrix cores (three-way exact operand
     * split, six products, fp32 accumulate: the precision of r3d_gemm_desc::prec = 1) */
    const uint16_t* pl_wv; const uint16_t* pl_wproj; const uint16_t* pl_w1; const uint16_t* pl_w2; const uint16_t* pl_wkv;
    const uint16_t* pl_wseg;
} r3d_fuser_chain_fwd_args;
/* bf16x3 operand-order planes: for a matrix B[n][k] (N x K), bf16 element (tile t = n / 16, k-step s = k / 32, plane p of
 * {high, middle, low}, lane = n %% 16 + 16 ((k %% 32) / 8), e = k %% 8) at index ((((t * ceil(K/32) + s) * 3 + p) * 64 + lane) * 8
 * + e); zero where n >= N or k >= K.  transposed != 0: B[n][k] = src[k * ld + n] (the planes of the transpose: input-gradient
 * products), else src[n * ld + k]. */
typedef struct r3d_plane_job {
    const float* src; uint16_t* dst; int32_t ld, N, K, transposed, first_block, pad_;
} r3d_plane_job;
int64_t r3d_weight_plane_elems(int N, int K);
int r3d_weight_planes(const r3d_plane_job* jobs_device, int njobs, int total_blocks, void* stream);
int r3d_fuser_chain_supported(int N, int H, int K, int B, int Q, int heads);
int r3d_fuser_chain_fwd(const r3d_fuser_chain_fwd_args* a, void* stream);
/* The adjoint of r3d_fuser_chain_fwd, one launch.  Fuser role: d(memory + pos) = d_cakv Wkv (stored in d_fused: the
 * positional embedding's gradient) + d_seg Wseg (+ d_extra [N,128], optional: the effective-rank penalty's gradient) ->
 * fuser.norm backward (half of a frame's gradient to each token row) -> d_u = (d_x3 W2) GELU'(u) -> d_h2 = d_u W1 ->
 * norm2 backward + d_x3 -> d_v = unswap(d_x1 Wproj) -> d_h1 = d_v Wv -> norm1 backward + d_x1 (+ d_x3 when add_xres) ->
 * embd_drop -> token-exchange backward (masks m_rgb / m_dep [128], ReLU gate of the RGB embedding) -> depth LayerNorm +
 * ReLU backward (autograd of model/futr_safuser_tokenfusion.py:83-94,56-62,183,195-197).  Stored for the weight-gradient
 * launch: d_x3, d_u, d_x1, d_v (d_h2, d_h1 optional).  LayerNorm parameter-gradient partials: part_nf / part_n2
 * [2N/4][2][128] (one (dgamma, dbeta) pair per 4 rows), part_n1 / part_dep [N][2][128] (one per frame).
 * Query role: caqin = d_caq Wq -> decoder norm1 backward (dy = caqin + d_t1_res; partials part_d1 [B*Q/4][2][128]) ->
 * sap = dropout' -> sao = sap Wout -> attention core backward (saqkv) -> sain = saqkv Win (transformer.py:289-293,300). */
typedef struct r3d_fuser_chain_bwd_args {
    const float* d_cakv; const float* d_seg; const float* d_extra; const float* wkv; const float* wseg;
    const float* x3; const float* mf; const float* rf; const float* gf;
    const float* w2; const float* u; const float* w1; const float* x1; const float* m2; const float* r2; const float* g2;
    const float* wproj; const float* wv; const float* x0; const float* m1; const float* r1; const float* g1n;
    const uint8_t* drop_x0; const float* m_rgb; const float* m_dep; const float* rgb; const float* dep_pre;
    const float* mean_d; const float* rstd_d; const float* lnd_g; const float* lnd_b;
    float* d_fused; float* d_x3; float* d_u; float* d_h2; float* d_x1; float* d_v; float* d_h1; float* d_rgb_pre;
    float* d_dep_pre; float* part_nf; float* part_n2; float* part_n1; float* part_dep;
    const float* d_caq; const float* d_t1_res; const float* wq; const float* t1_pre; const float* m1d; const float* r1d;
    const float* g1d; const uint8_t* drop_d1; const float* w_out; const float* sa_qkv; const float* p_sa;
    const uint8_t* drop_sa; const float* w_in;
    float* caqin; float* t1pre_out; float* sap; float* sao; float* saqkv; float* sain; float* part_d1;
    float drop_scale;
    int32_t N, S, K, H, add_xres, B, Q, heads;
    uint64_t* timeline;      /* as in r3d_fuser_chain_fwd_args */
    /* optional (all or none; K <= 32): bf16x3 operand-order planes of the TRANSPOSED weights (r3d_plane_job::transposed = 1) of
     * wkv, wseg, w2, w1, wproj, wv -- the fuser role's input-gradient products then run on the bf16 matrix cores */
    const uint16_t* pl_wkv_t; const uint16_t* pl_wseg_t; const uint16_t* pl_w2_t; const uint16_t* pl_w1_t;
    const uint16_t* pl_wproj_t; const uint16_t* pl_wv_t;
} r3d_fuser_chain_bwd_args;
int r3d_fuser_chain_bwd(const r3d_fuser_chain_bwd_args* a, void* stream);

/* ---- build-defined THREE-modality fuser pieces (csrc/fuser3.hip; BASELINE configs[4]; the reference's CMFuser is
 * two-token, model/futr_safuser_tokenfusion.py:74-81 -- SURVEY.md 8(d): checked against the build's own CPU restatement) ----
 * Rows frame-major: the tokens of frame n are rows 3n, 3n + 1, 3n + 2.
 * exchange3: x0[3n + m] = (mask[m] ? x_{(m+1) %% 3}[n] : x_m[n]) * keep  (mask [3][C] 1.0 / 0.0, drop_mask optional [3N, C]);
 * attn3: attention over a frame's three tokens with the -inf diagonal (every token attends to the two others), qkv [3N, 3C] =
 *        [q | k | v] per row, C / heads <= 128, probs [N][heads][3][2]; triple_mean: torch.mean over the three tokens. */
int r3d_token_exchange3_fwd(const float* xa, const float* xb, const float* xc, const float* mask, const uint8_t* drop_mask,
                            float drop_scale, float* x0, int N, int C, void* stream);
int r3d_token_exchange3_bwd(const float* dx0, const float* mask, const uint8_t* drop_mask, float drop_scale, float* da, float* db,
                            float* dc, int N, int C, void* stream);
int r3d_attn3_fwd(const float* qkv, float* probs, float* out, int N, int C, int heads, void* stream);
int r3d_attn3_bwd(const float* qkv, const float* d_out, float* d_qkv, int N, int C, int heads, void* stream);
int r3d_triple_mean_fwd(const float* y, float* out, int N, int C, void* stream);
int r3d_triple_mean_bwd(const float* d_out, float* dy, int N, int C, void* stream);

/* ---- token selection / exchange: CMFuser.token_fusion (model/futr_safuser_tokenfusion.py:33-66) ------------- */
/* out[c] = sum_r |x[r,c]| in fp64 (the eval-mode score before the division by B*T, :49-50). */
int r3d_colabssum(const float* x, int ld, int rows, int cols, double* out, void* stream);
/* k smallest of nvec score vectors of length C (torch.topk(..., largest=False) on CPU, :52-54), bit-exact as a SET
 * including ties (libstdc++ introselect emulation when the k-th boundary cuts a group of equal scores).
 * idx_out [nvec][k] ascending; mask_out [nvec][C] 1.0/0.0 (optional); used_serial [nvec] (optional diagnostics). */
int r3d_token_select(const float* score_f, const double* score_sum, double count, int nvec, int C, int k,
                     int64_t* idx_out, float* mask_out, int* used_serial, void* stream);
/* x0[2n] = mask_rgb ? dep[n] : rgb[n];  x0[2n+1] = mask_dep ? rgb[n] : dep[n]; then embd_drop (:56-62, :83). */
int r3d_token_exchange_fwd(const float* rgb, const float* dep, const float* mask_rgb, const float* mask_dep, float* x0,
                           const uint8_t* drop_mask, float drop_scale, int N, int H, void* stream);
/* d_rgb_pre = ((1-mask_rgb) g[2n] + mask_dep g[2n+1]) * [rgb > 0];  d_dep = mask_rgb g[2n] + (1-mask_dep) g[2n+1]. */
int r3d_token_exchange_bwd(const float* dx0, const float* rgb, const float* mask_rgb, const float* mask_dep,
                           const uint8_t* drop_mask, float drop_scale, float* d_rgb_pre, float* d_dep, int N, int H,
                           void* stream);

/* ---- decoder attention core: nn.MultiheadAttention minus its projections (model/extras/transformer.py:289-304) --
 * q rows b*Lq+i, k/v rows b*Lk+j, head h in columns [h*dh, (h+1)*dh).  probs [B][heads][Lq][Lk] = softmax before
 * dropout (saved for backward).  Padded keys: key_padding_mask [B][Lk] (1 = padded) and/or key_label [B][Lk] int64
 * with key padded iff label == pad_idx (get_pad_mask, model/futr_safuser_tokenfusion.py:168,243-244); both may be NULL.
 * drop_mask like probs or NULL. */
int r3d_mha_core_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                     const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx, float* probs,
                     const uint8_t* drop_mask, float drop_scale, float* o, int ldo, int B, int heads, int Lq, int Lk,
                     int dh, void* stream);
int r3d_mha_core_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* probs,
                     const uint8_t* drop_mask, float drop_scale, const float* d_o, int lddo, float* dq, int lddq, float* dk,
                     int lddk, float* dv, int lddv, int B, int heads, int Lq, int Lk, int dh, void* stream);
/* 1 if the two calls above run an (Lq, Lk, dh) problem (bwd != 0: r3d_mha_core_bwd), else 0; host-only, the same test
 * the launches apply: Lq * dh <= 1024 and the core's LDS (score matrix, its gradient, two key chunks) within 160 KiB. */
int r3d_mha_core_supported(int Lq, int Lk, int dh, int bwd);

/* ---- tiled attention core (csrc/attention_tiled.hip): the same product for long sequences -----------------------
 * Operands, scale 1/sqrt(dh), key masks and the dropout keep-mask (uint8 [B][heads][Lq][Lk], applied with drop_scale to the
 * normalised probabilities) exactly as r3d_mha_core_*, but no [Lq][Lk] tensor is written: the forward streams 64-key
 * tiles under an online softmax and writes o and lse [B][heads][Lq] = log sum_j exp(s_ij) over the unmasked keys; the
 * backward recomputes the probabilities from q, k, lse and the mask arguments (pass the forward's), needs the forward's
 * o, and writes delta [B][heads][Lq] = rowsum(dO o O) into the caller's workspace.  Two backward kernels (one per query
 * tile for dq, one per key tile for dk / dv), no atomics: results are bitwise reproducible.  No allocation, no host
 * synchronisation.  A clip whose keys are all masked gives NaN rows, as r3d_mha_core_fwd does. */
int r3d_mha_tiled_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                      const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx, const uint8_t* drop_mask,
                      float drop_scale, float* o, int ldo, float* lse, int B, int heads, int Lq, int Lk, int dh,
                      void* stream);
int r3d_mha_tiled_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                      const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx, const uint8_t* drop_mask,
                      float drop_scale, const float* o, int ldo, const float* lse, const float* d_o, int lddo, float* delta,
                      float* dq, int lddq, float* dk, int lddk, float* dv, int lddv, int B, int heads, int Lq, int Lk,
                      int dh, void* stream);
/* 1 if the two calls above run an (Lq, Lk, dh) problem, else 0; host-only, the same test the launches apply before they
 * launch anything: Lq >= 1, Lk >= 1 and 1 <= dh <= 128 (forward and backward alike). */
int r3d_mha_tiled_supported(int Lq, int Lk, int dh, int bwd);

/* ---- split-key attention core (csrc/attention_splitk.hip): few queries against many keys --------------------------
 * The same product once more, for the token-fusion decoder's cross-attention (n_query rows per clip against the S frames
 * of the memory) past r3d_mha_core_*'s LDS: 1 <= Lq <= 16, Lk >= 1, 1 <= dh <= 128.  Operands, scale, key masks, the
 * dropout keep-mask, o, lse [B][heads][Lq] and delta [B][heads][Lq] exactly as r3d_mha_tiled_*: the two pairs are
 * interchangeable on the same buffers (a forward of one, the backward of the other).  The KEYS are spread over the chip:
 * grid (ceil(Lk / chunk), heads, B) with chunk = r3d_mha_splitk_chunk(Lk, dh), a pure function of its arguments and a
 * multiple of 64.  Forward: every workgroup writes its chunk maximum, chunk sum and unnormalised
 * sum exp(s - m_c) keep drop_scale v to ws; a second launch merges the chunks in chunk order into o and lse.  Backward:
 * every workgroup recomputes delta and P = exp(s - lse), writes dk and dv of its keys (each element once) and its dq
 * partial to ws; a second launch sums the partials in chunk order and writes delta.  ws: r3d_mha_splitk_ws_floats(...)
 * floats owned by the caller (bwd != 0: what r3d_mha_splitk_bwd needs), contents undefined on entry.  No atomics, no
 * workgroup waits on another, every sum has a fixed order: results are bitwise reproducible.  No allocation, no host
 * synchronisation.  A refused shape returns R3D_EINVAL before anything is launched.  A clip whose keys are all masked
 * gives NaN rows, as r3d_mha_core_fwd does. */
int r3d_mha_splitk_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                       const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx, const uint8_t* drop_mask,
                       float drop_scale, float* o, int ldo, float* lse, float* ws, int B, int heads, int Lq, int Lk, int dh,
                       void* stream);
int r3d_mha_splitk_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                       const uint8_t* key_padding_mask, const int64_t* key_label, int pad_idx, const uint8_t* drop_mask,
                       float drop_scale, const float* o, int ldo, const float* lse, const float* d_o, int lddo, float* delta,
                       float* dq, int lddq, float* dk, int lddk, float* dv, int lddv, float* ws, int B, int heads, int Lq,
                       int Lk, int dh, void* stream);
/* host-only: 1 if the two calls above run an (Lq, Lk, dh) problem; the keys per workgroup; the floats of ws. */
int r3d_mha_splitk_supported(int Lq, int Lk, int dh, int bwd);
int r3d_mha_splitk_chunk(int Lk, int dh);
size_t r3d_mha_splitk_ws_floats(int B, int heads, int Lq, int Lk, int dh, int bwd);

/* ---- fused decoder layer, one workgroup per clip (TransformerDecoderLayer.forward_post, model/extras/transformer.py:
 * 281-330; final decoder.norm :182-183; fc|fc_len head futr_safuser_tokenfusion.py:219-226) --------------------------
 * Replaces ~17 dependent launches per layer by one.  Supported when one clip's layer fits a CU's LDS
 * (r3d_decoder_fused_supported); otherwise the host composes the layer from the GEMM / attention / LayerNorm entry points.
 * ptrs[R3D_DEC_FWD_NPTRS], in this order (N = optional, may be NULL):
 *   0-17  parameters: self_attn.in_proj_weight, .in_proj_bias, .out_proj.weight, .out_proj.bias, norm1.weight, norm1.bias,
 *         multihead_attn.in_proj_weight, .in_proj_bias, .out_proj.weight, .out_proj.bias, norm2.weight, norm2.bias,
 *         linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm3.weight, norm3.bias
 *   18 memory [B*S,H]   19 pos [S,H]   20 query_pos [Q,H]   21 tgt_in [B*Q,H] (N: layer 0, tgt = 0)
 *   22 key_label int64 [B*S] (N)       23-28 dropout keep masks uint8 (N): sa_p, ca_p, d1, d2, d3, ff
 *   29-48 saved activations (outputs): sa_qkv [BQ,3H], p_sa [B,h,Q,Q], sa_o, t1_pre, t1 [BQ,H], m1, r1 [BQ], caq [BQ,H],
 *         cakv [B*S,2H], p_ca [B,h,Q,S], ca_o, t2_pre, t2 [BQ,H], m2, r2 [BQ], ff1 [BQ,4H], t3_pre, t3 [BQ,H], m3, r3 [BQ]
 *   49-56 tail of the last layer (all N together): decoder.norm.weight, .bias, tgtF [BQ,H], mF, rF [BQ],
 *         head weight [n_head_out,H], head bias [n_head_out], actdur [BQ,n_head_out] */
#define R3D_DEC_FWD_NPTRS 57
int r3d_decoder_fused_supported(int S, int Q, int H, int heads);
int r3d_decoder_layer_fwd(const void* const* ptrs, int nptrs, int B, int S, int Q, int H, int heads, int pad_idx,
                          float drop_scale, int n_head_out, void* stream);

/* ---- the seam between the input projections and the fuser block, one launch per direction (train mode) -----------
 * forward : split-K slab sums of input_embed (+bias, ReLU :183) and depth_projection (+bias, LayerNorm, ReLU :195-197),
 *           token exchange + embd_drop (:56-62,83), fuser.blocks.0.norm1 (transformerblock.py:122).
 *           rgb_src: ns_r > 0 -> slabs [ns_r][N][H]; ns_r == 0 -> the finished embedding (rgb_out may alias it).
 *           dep_src: slabs [ns_d][N][H], ns_d >= 1 (a finished pre-LayerNorm matrix is one slab).
 * backward: norm1 backward (+ residual gradients add1, add2), exchange backward, ReLU of the RGB embedding, depth
 *           LayerNorm + ReLU backward; ws_n1 / ws_dep [N][2][H] receive one (dgamma, dbeta) partial per frame
 *           (r3d_layernorm_bwd_finalize_batched job with rows = -N).  All matrices contiguous, ld = H <= 1024. */
int r3d_embed_fuse_fwd(const float* rgb_src, int ns_r, const float* bias_r, const float* dep_src, int ns_d,
                       const float* bias_d, const float* lnd_gamma, const float* lnd_beta, const float* mask_rgb,
                       const float* mask_dep, const uint8_t* drop_mask, float drop_scale, const float* ln1_gamma,
                       const float* ln1_beta, float* rgb_out, float* dep_pre_out, float* mean_d, float* rstd_d,
                       float* dep_out, float* x0, float* h1, float* m1, float* r1, int N, int H, void* stream);
/* r3d_embed_fuse_fwd and r3d_weight_planes (below: jobs_device / njobs / total_blocks as there) in ONE launch: the re-split of
 * the chain weights rides as extra workgroups of the seam. */
int r3d_embed_fuse_fwd_planes(const float* rgb_src, int ns_r, const float* bias_r, const float* dep_src, int ns_d,
                              const float* bias_d, const float* lnd_gamma, const float* lnd_beta, const float* mask_rgb,
                              const float* mask_dep, const uint8_t* drop_mask, float drop_scale, const float* ln1_gamma,
                              const float* ln1_beta, float* rgb_out, float* dep_pre_out, float* mean_d, float* rstd_d,
                              float* dep_out, float* x0, float* h1, float* m1, float* r1, int N, int H,
                              const r3d_plane_job* jobs_device, int njobs, int total_blocks, void* stream);
int r3d_embed_fuse_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1, const float* ln1_gamma,
                       const float* add1, const float* add2, const uint8_t* drop_mask, float drop_scale,
                       const float* mask_rgb, const float* mask_dep, const float* rgb, const float* dep_pre,
                       const float* mean_d, const float* rstd_d, const float* lnd_gamma, const float* lnd_beta,
                       float* d_rgb_pre, float* d_dep_pre, float* ws_n1, float* ws_dep, int N, int H, void* stream);
/* ---- the same seam for THREE modalities (build-defined, as r3d_token_exchange3_*: model/futr_safuser_tokenfusion3.py) ----
 * r3d_embed_fuse3_fwd : the slab conventions of r3d_embed_fuse_fwd for rgb_src / dep_src; the third embedding is
 *                       gz = relu(LN_g(b_gaze + w_gaze . gaze[n])) with gaze [N][gaze_dim], w_gaze [H][gaze_dim],
 *                       1 <= gaze_dim <= 8.  mask [3][H] (1.0 / 0.0): token m takes its masked columns from modality
 *                       (m + 1) mod 3; drop_mask (optional) [3N][H].  x0 / h1 [3N][H] and m1 / r1 [3N], rows frame-major
 *                       (3n + m); rgb_out, dep_pre_out, dep_out, gz_pre_out, gz_out [N][H]; mean_* / rstd_* [N].
 * r3d_embed_fuse3_bwd : norm1 backward (+ add1, add2), dropout, exchange adjoint, the RGB ReLU and both LayerNorm + ReLU
 *                       adjoints -> d_rgb_pre, d_dep_pre, d_gz_pre [N][H]; ws_n1 / ws_dep / ws_gz [N][2][H] per-frame
 *                       (dgamma, dbeta) partials (r3d_layernorm_bwd_finalize_batched job with rows = -N).
 *                       (d gaze_projection = d_gz_pre^T . gaze with its column sums is an r3d_gemm_f32 TN product with
 *                       bias_grad: its scalar path takes an output gaze_dim wide.)
 * No atomics: the same call gives the same bits.  All matrices contiguous, ld = H <= 1024. */
int r3d_embed_fuse3_fwd(const float* rgb_src, int ns_r, const float* bias_r, const float* dep_src, int ns_d,
                        const float* bias_d, const float* lnd_gamma, const float* lnd_beta, const float* gaze,
                        const float* w_gaze, const float* b_gaze, const float* lng_gamma, const float* lng_beta, int gaze_dim,
                        const float* mask, const uint8_t* drop_mask, float drop_scale, const float* ln1_gamma,
                        const float* ln1_beta, float* rgb_out, float* dep_pre_out, float* mean_d, float* rstd_d,
                        float* dep_out, float* gz_pre_out, float* mean_g, float* rstd_g, float* gz_out, float* x0, float* h1,
                        float* m1, float* r1, int N, int H, void* stream);
int r3d_embed_fuse3_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1, const float* ln1_gamma,
                        const float* add1, const float* add2, const uint8_t* drop_mask, float drop_scale, const float* mask,
                        const float* rgb, const float* dep_pre, const float* mean_d, const float* rstd_d,
                        const float* lnd_gamma, const float* lnd_beta, const float* gz_pre, const float* mean_g,
                        const float* rstd_g, const float* lng_gamma, const float* lng_beta, float* d_rgb_pre,
                        float* d_dep_pre, float* d_gz_pre, float* ws_n1, float* ws_dep, float* ws_gz, int N, int H,
                        void* stream);

/* ---- the BN-blend token fuser of model/futr_safuser_batchnormalization.py:38-76 -------------------------
 * r3d_bn_stats     : BatchNorm1d statistics of both embeddings [N, C] (batch statistics + running-stat update when
 *                    training, running statistics otherwise) -> mean / rstd [2][C], absgamma [2][C] (selection score).
 * r3d_bn_blend_fwd : x0 [2N, C] = embd_drop(blend(BN(rgb), BN(dep))) with alpha on the selected channels, h1 = norm1(x0).
 * r3d_bn_blend_bwd : norm1 backward (+ add1), dropout, blend backward -> five [N, C] term matrices whose column sums
 *                    (r3d_rowmod_sum_batched, mod = 1) are d beta_rgb, d gamma_rgb, d beta_dep, d gamma_dep, d alpha;
 *                    norm1 parameter partials ws_n1 [N][2][C] (finalize job with rows = -N).
 * r3d_bn_bwd_apply : BatchNorm input gradients from those sums; d_rgb_pre includes input_embed's ReLU. */
int r3d_bn_stats(const float* x_rgb, const float* x_dep, float* run_mean_rgb, float* run_var_rgb, int64_t* nbt_rgb,
                 float* run_mean_dep, float* run_var_dep, int64_t* nbt_dep, const float* gamma_rgb, const float* gamma_dep,
                 float* mean, float* rstd, float* absgamma, int N, int C, int training, float momentum, void* stream);
int r3d_bn_blend_fwd(const float* rgb, const float* dep, const float* mean, const float* rstd, const float* gamma_rgb,
                     const float* beta_rgb, const float* gamma_dep, const float* beta_dep, const float* alpha,
                     const float* mask_rgb, const float* mask_dep, const uint8_t* drop_mask, float drop_scale,
                     const float* ln1_gamma, const float* ln1_beta, float* x0, float* h1, float* m1, float* r1, int N, int C,
                     void* stream);
int r3d_bn_blend_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1, const float* ln1_gamma,
                     const float* add1, const uint8_t* drop_mask, float drop_scale, const float* rgb, const float* dep,
                     const float* mean, const float* rstd, const float* gamma_rgb, const float* beta_rgb,
                     const float* gamma_dep, const float* beta_dep, const float* alpha, const float* mask_rgb,
                     const float* mask_dep, float* t_drb, float* t_drbx, float* t_ddb, float* t_ddbx, float* t_dal,
                     float* ws_n1, int N, int C, void* stream);
int r3d_bn_bwd_apply(const float* rgb, const float* dep, const float* mean, const float* rstd, const float* gamma_rgb,
                     const float* gamma_dep, const float* t_drb, const float* t_ddb, const float* dgamma_rgb,
                     const float* dbeta_rgb, const float* dgamma_dep, const float* dbeta_dep, float* d_rgb_pre, float* d_dep,
                     int N, int C, int training, void* stream);
/* ---- the plain SA-Fuser of model/futr_safuser_depth.py:36-62 (no selection, no exchange, no x_res) ---------------------------
 * r3d_plain_fuse_fwd : r3d_embed_fuse_fwd with x0 [2N, H] = embd_drop([rgb; dep] + tok) (tok = fuser.modality_token [H])
 *                      in place of the exchange; jobs_device / njobs / total_blocks (optional, NULL = none) as
 *                      r3d_embed_fuse_fwd_planes.
 * r3d_plain_fuse_bwd : norm1 backward (+ add1), dropout -> d_rgb_pre (with input_embed's ReLU), d_dep_pre (depth LayerNorm
 *                      + ReLU backward), the per-frame partials ws_n1 / ws_dep [N][2][H], and t_tok [N, H] = the sum of each
 *                      frame's two post-dropout row gradients (column sum = d modality_token).  d_rgb_pre, d_dep_pre, ws_n1,
 *                      ws_dep: all given, or all NULL for t_tok alone. */
int r3d_plain_fuse_fwd(const float* rgb_src, int ns_r, const float* bias_r, const float* dep_src, int ns_d,
                       const float* bias_d, const float* lnd_gamma, const float* lnd_beta, const float* tok,
                       const uint8_t* drop_mask, float drop_scale, const float* ln1_gamma, const float* ln1_beta,
                       float* rgb_out, float* dep_pre_out, float* mean_d, float* rstd_d, float* dep_out, float* x0,
                       float* h1, float* m1, float* r1, int N, int H, const r3d_plane_job* jobs_device, int njobs,
                       int total_blocks, void* stream);
int r3d_plain_fuse_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1, const float* ln1_gamma,
                       const float* add1, const uint8_t* drop_mask, float drop_scale, const float* rgb,
                       const float* dep_pre, const float* mean_d, const float* rstd_d, const float* lnd_gamma,
                       const float* lnd_beta, float* d_rgb_pre, float* d_dep_pre, float* ws_n1, float* ws_dep,
                       float* t_tok, int N, int H, void* stream);
/* ---- the activation-magnitude token fuser of model/futr_safuser_tokenfusion_vary.py:36-56 -----------------------------
 * (selection: r3d_colabssum + r3d_token_select with k = C // 4 on the scores mean_(B,T) |x|, in every mode)
 * r3d_scaled_exchange_fwd : x0 [2N, C] = embd_drop(scaled exchange): selected RGB channels <- alpha * dep, selected depth
 *                           channels <- alpha * rgb; h1 = norm1(x0), m1 / r1 [2N].
 * r3d_scaled_exchange_bwd : norm1 backward (+ add1), dropout, exchange adjoint -> d_rgb_pre (with input_embed's ReLU),
 *                           d_dep, and t_dal [N, C] whose column sum is d alpha; optional norm1 partials ws_n1 [N][2][C]. */
int r3d_scaled_exchange_fwd(const float* rgb, const float* dep, const float* mask_rgb, const float* mask_dep,
                            const float* alpha, const uint8_t* drop_mask, float drop_scale, const float* ln1_gamma,
                            const float* ln1_beta, float* x0, float* h1, float* m1, float* r1, int N, int C, void* stream);
int r3d_scaled_exchange_bwd(const float* d_h1, const float* x0, const float* m1, const float* r1, const float* ln1_gamma,
                            const float* add1, const uint8_t* drop_mask, float drop_scale, const float* rgb,
                            const float* dep, const float* mask_rgb, const float* mask_dep, const float* alpha,
                            float* d_rgb_pre, float* d_dep, float* t_dal, float* ws_n1, int N, int C, void* stream);
/* Data-parallel BatchNorm for that fuser (the statistics of the GLOBAL batch, as one process running the reference sees
 * them; replaces what torch.nn.SyncBatchNorm would do for futr_safuser_batchnormalization.py:45-46):
 * r3d_bn_sync_pack     : the local moments left by r3d_bn_stats -> out [4C + 1] = (mean [2][C], M2 = N var [2][C], N);
 * r3d_bn_sync_finalize : all [world][4C + 1] (every rank's pack, rank order) -> global mean / rstd [2][C] by Chan's
 *                        parallel-variance combination, running-statistics update from the global moments, nfrac[0] =
 *                        n_local / n_global. */
int r3d_bn_sync_pack(const float* mean, const float* rstd, int N, int C, float* out, void* stream);
int r3d_bn_sync_finalize(const float* all, int world, int n_local, int C, float* mean, float* rstd, float* run_mean_rgb,
                         float* run_var_rgb, int64_t* nbt_rgb, float* run_mean_dep, float* run_var_dep, int64_t* nbt_dep,
                         float* nfrac, float momentum, void* stream);

/* ---- the decoder's tail, one launch per direction (row-local on the B*Q query rows) ------------------------------
 * forward : last layer's norm3 (transformer.py:329) -> decoder.norm (:182-183) -> heads fc | fc_len as one [n_head, H]
 *           product (futr_safuser_tokenfusion.py:219-226).  x = pre-norm3 rows [rows, H] contiguous.
 * backward: heads' input gradient -> decoder.norm backward -> norm3 backward; dx = gradient w.r.t. x, dx2 = dx * dropout3
 *           mask (:328).  LayerNorm parameter gradients: partials wsF / ws3 in r3d_layernorm_bwd's layout for `rows` rows,
 *           or final values in dgF/dbF/dg3/db3 when one block covers all rows (rows <= 4). */
int r3d_decoder_tail_fwd(const float* x, const float* g3, const float* b3, const float* gF, const float* bF,
                         const float* w_head, const float* b_head, int n_head, float* t3, float* m3, float* r3, float* tgtF,
                         float* mF, float* rF, float* out, int ld_out, int rows, int H, void* stream);
int r3d_decoder_tail_bwd(const float* d_out, int ld_dout, const float* w_head, int n_head, const float* t3, const float* mF,
                         const float* rF, const float* gF, const float* x, const float* m3, const float* r3, const float* g3,
                         const uint8_t* drop_mask, float drop_scale, float* dx, float* dx2, float* dgF, float* dbF,
                         float* dg3, float* db3, float* wsF, float* ws3, int rows, int H, void* stream);

/* ---- losses: utils.py:325-328,358-378,410-490 as composed at train/train_proposed_depth.py:171-213 ------------- */
int r3d_losses_fwd_bwd(const float* seg_logits, int ld_seg, const float* act_logits, int ld_act, const float* dur,
                       int ld_dur, const int64_t* past_label, const int64_t* target, const float* target_dur, int B, int S,
                       int Q, int K, int pad_idx, int exclude_idx, int val_mode, const float* dur_den, float grad_scale,
                       float* d_seg, int ld_dseg, float* d_act, int ld_dact, float* d_dur, int ld_ddur, float* loss_out,
                       int64_t* counts, float* ws, int64_t* tick_a, int64_t* tick_b, void* stream);
/* ws: r3d_losses_ws_floats floats, 16-byte aligned and ZERO before the first call (it ends with the arrival counter of
 * the single-launch reduction, which every call leaves at zero).  tick_a / tick_b: optional device int64 counters
 * incremented once per call (the engine's step counter and dropout offset). */
int64_t r3d_losses_ws_floats(int B, int S, int Q);
/* The same launch with seg logits of Kseg classes (the RNN baseline's fc_seg has n_class - 1 outputs, model/rnn.py:37):
 * ld_seg / ld_dseg >= Kseg, seg labels outside [0, Kseg) are ignored.  Kseg == K computes what r3d_losses_fwd_bwd does. */
int r3d_losses_fwd_bwd_kseg(const float* seg_logits, int ld_seg, const float* act_logits, int ld_act, const float* dur,
                            int ld_dur, const int64_t* past_label, const int64_t* target, const float* target_dur, int B,
                            int S, int Q, int K, int Kseg, int pad_idx, int exclude_idx, int val_mode, const float* dur_den,
                            float grad_scale, float* d_seg, int ld_dseg, float* d_act, int ld_dact, float* d_dur,
                            int ld_ddur, float* loss_out, int64_t* counts, float* ws, int64_t* tick_a, int64_t* tick_b,
                            void* stream);

/* ---- training step only: the decoder's tail, the three losses and the tail's backward as ONE launch -------------------
 * = r3d_decoder_tail_fwd (transformer.py:329,182-183; futr_safuser_tokenfusion.py:219-226) -> r3d_losses_fwd_bwd
 * (train_proposed_depth.py:171-213) -> r3d_decoder_tail_bwd, same arithmetic per row.  The anticipation logits live in
 * out [B*Q, ld_out]: K action columns + 1 duration column; d_out likewise.  wsF / ws3: LayerNorm parameter-gradient
 * partials in r3d_layernorm_bwd's layout for B*Q rows.  ws: as for r3d_losses_fwd_bwd.
 * r3d_decoder_tail_losses_supported: hidden <= 128, K + 1 <= 24, Q == 8, B*Q <= 1024; callers fall back to the three
 * separate entry points otherwise. */
typedef struct r3d_tail_losses_args {
    const float* x; const float* g3; const float* b3; const float* gF; const float* bF;
    const float* w_head; const float* b_head; int n_head;
    float* t3; float* m3; float* r3; float* tgtF; float* mF; float* rF; float* out; int ld_out; int H;
    const float* seg; int ld_seg; const int64_t* past_label; const int64_t* target; const float* target_dur;
    int B, S, Q, K, pad_idx, exclude_idx; const float* dur_den; float grad_scale;
    float* d_seg; int ld_dseg; float* d_out; int ld_dout; float* loss_out; int64_t* counts; int64_t* tick_a; int64_t* tick_b;
    const uint8_t* drop; float drop_scale; float* dx; float* dx2; float* wsF; float* ws3;
    int defer_finalize;      /* != 0: the launch leaves the per-unit loss partials in ws (and ticks the counters) but does NOT
                                reduce them into loss_out / counts -- no arrival atomics, no last-workgroup pass at the end of
                                the step's longest small kernel; r3d_losses_finalize or r3d_adamw_flat_dropout_fin does it */
} r3d_tail_losses_args;
int r3d_decoder_tail_losses_supported(int H, int n_head, int Q, int rows);
int r3d_decoder_tail_losses(const r3d_tail_losses_args* a, float* ws, void* stream);

/* ---- the decoder layer's query side as ONE launch (csrc/decoder_chain.hip; hidden 128, 8 queries, 8 heads, <= 64 keys) ----
 * One workgroup per clip.  phases (bit mask):
 *   1  forward : cross-attention core on (caq, cakv[:, :128] = keys, cakv[:, 128:] = values; key j of clip b padded iff
 *                key_label[b][j] == pad_idx; probabilities p_ca, dropout drop_ca) -> t2_pre = dropout(ca_o Wo^T + bo) + t1 ->
 *                t2 = norm2(t2_pre) -> ff1 = dropout(relu(t2 W1^T + b1)) -> t3_pre = dropout(ff1 W2^T + b2) + t2
 *                (model/extras/transformer.py:300-306,325-328)
 *   2  tail    : r3d_decoder_tail_losses on the clip (norm3 -> decoder.norm -> heads -> the three losses -> back to d_t3pre /
 *                d_ff2); `tail` and `ws` as for that entry point; tail->x must be t3_pre, tail->dx / dx2 must be d_t3pre / d_ff2
 *   4  backward: d_ff1 = (d_ff2 W2) relu' dropout' -> d t2 = d_ff1 W1 + d_t3pre -> norm2 backward (d_t2pre; LayerNorm parameter
 *                partials part_d2 [B*Q/4][2][128], one pair per 4 rows) -> d_cap = dropout' -> d_cao = d_cap Wo -> attention core
 *                backward (d_caq [B*Q,128], d_cakv [B*S,256])
 * 7 = the training step's whole decoder after the key/value projection in one launch; 1 and 4 stand alone.  Matrices dense
 * row-major; dropout masks optional (NULL). */
typedef struct r3d_decoder_chain_args {
    const float* caq; const float* cakv; const int64_t* key_label; float* p_ca; const uint8_t* drop_ca; float* ca_o;
    const float* wo; const float* bo; const uint8_t* drop_d2; const float* t1; float* t2_pre; const float* g2; const float* be2;
    float* t2; float* m2; float* r2; const float* w1; const float* b1; const uint8_t* drop_ff; float* ff1;
    const float* w2; const float* b2; const uint8_t* drop_d3; float* t3_pre;
    const float* d_t3pre; const float* d_ff2; float* d_ff1; float* d_t2pre; float* d_cap; float* d_cao; float* d_caq;
    float* d_cakv; float* part_d2;
    float drop_scale;
    int32_t pad_idx, B, S, H, Q, heads, phases;
    uint64_t* timeline;      /* profiling aid, normally NULL: wave 0 of clip 0 stores wall_clock64() (100 MHz) at its stage
                                boundaries [0..31] */
    /* optional (all or none): bf16x3 operand-order planes (r3d_weight_planes) of wo, w1, w2 and of their transposes -- the
     * products then run on the bf16 matrix cores */
    const uint16_t* pl_wo; const uint16_t* pl_w1; const uint16_t* pl_w2; const uint16_t* pl_w2_t; const uint16_t* pl_w1_t;
    const uint16_t* pl_wo_t;
} r3d_decoder_chain_args;
int r3d_decoder_chain_supported(int H, int Q, int heads, int S);
int r3d_decoder_chain(const r3d_decoder_chain_args* d, const r3d_tail_losses_args* tail, float* ws, void* stream);

/* ---- optimiser / dropout masks: main_darai.py:135, train/train_proposed_depth.py:215 -------------------------- */
/* torch.optim.AdamW semantics over flat arenas of n floats (n % 4 == 0, 16-byte aligned); g is multiplied by
 * grad_scale first (1/world after a sum all-reduce).  lr and the 1-based step are read from device memory. */
int r3d_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, const int64_t* step,
                   float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream);
/* r3d_adamw_flat and r3d_dropout_mask (the NEXT step's masks: the pool is free once the backward has run) in one launch. */
int r3d_adamw_flat_dropout(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, const int64_t* step,
                           float beta1, float beta2, float eps, float weight_decay, float grad_scale, uint8_t* mask,
                           int64_t n_mask, float p_drop, uint64_t seed, const int64_t* offset, void* stream);
/* The reduction r3d_decoder_tail_losses(defer_finalize) left out: loss_out[4] / counts[4] from the 4-float partials of the
 * B*S + B*Q + B units in `part` (the ws of that call), exactly as the undeferred launch computes them (fp64 sums, fixed
 * order).  Stand-alone launch, or -- r3d_adamw_flat_dropout_fin -- one extra workgroup of the AdamW launch, where it costs
 * nothing: the losses are host-visible statistics (utils.py:375-376 reads them per step with .item(); here once per
 * epoch), nothing on the device depends on them. */
typedef struct r3d_loss_finalize_job {
    const float* part; int32_t B, S, Q, has_seg;
    const float* dur_den;            /* optional device scalar, as in r3d_losses_fwd_bwd */
    float* loss_out; int64_t* counts;
    double* acc_loss; int64_t* acc_counts;   /* optional running sums [4] each: acc += this step's values (the epoch statistics
                                                of train/train_proposed_depth.py:216-228, kept on the device) */
} r3d_loss_finalize_job;
int r3d_losses_finalize(const r3d_loss_finalize_job* job, void* stream);
/* r3d_adamw_flat carrying the reduction as its workgroup 0 (fin != NULL), as r3d_adamw_flat_dropout_fin does. */
int r3d_adamw_flat_fin(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, const int64_t* step,
                       float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                       const r3d_loss_finalize_job* fin, void* stream);
int r3d_adamw_flat_dropout_fin(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, const int64_t* step,
                               float beta1, float beta2, float eps, float weight_decay, float grad_scale, uint8_t* mask,
                               int64_t n_mask, float p_drop, uint64_t seed, const int64_t* offset,
                               const r3d_loss_finalize_job* fin, void* stream);
/* The same update on a [rows x cols] block (leading dimension ld) of p/g/m/v: a pixel shard of depth_projection.weight. */
int r3d_adamw_2d(float* p, const float* g, float* m, float* v, int rows, int cols, int ld, const float* lr,
                 const int64_t* step, float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream);
/* mask[i] = 1 with probability 1-p (Philox4x32-10 keyed by seed, counter (i/4, *offset)). */
int r3d_dropout_mask(uint8_t* mask, int64_t n, float p, uint64_t seed, const int64_t* offset, void* stream);

/* ---- effective rank (build-side) ------------------------------------------------- */
int64_t r3d_erank_lds_bytes(int R, int C);
int r3d_erank_jacobi(const float* x, int ld, int64_t batch_stride, int batch, int R, int C, int gram, float* sigma,
                     float* af_t, float* stats, int max_sweeps, void* stream);
/* Any size: two-level (block) one-sided Jacobi with the columns in HBM; one matrix X[R, C].  r3d_erank_blocked_sizes
 * fills out[0] = floats of af_t ([Cpad][Rp], the rotated columns (X V)^T; Rp = R rounded up to 4 is the row stride,
 * rows past C and the row tails R..Rp-1 are zero), out[1] = ints of ctrl (scratch), out[2] = Rp, out[3] = columns per
 * block.  af_t must be 16-byte aligned.  sigma [C] unsorted, stats [4] = {erank, entropy, sum sigma, sweeps}.
 * max_sweeps <= 0 selects 16.  Enqueues its launches, no sync. */
int r3d_erank_blocked_sizes(int R, int C, int max_sweeps, int64_t* out);
int r3d_erank_blocked(const float* x, int ld, int R, int C, float* sigma, float* af_t, int* ctrl, float* stats,
                      int max_sweeps, void* stream);
/* The same with the input optionally given transposed (x_transposed != 0: x is [C][ld] = X^T of the [R, C] matrix that
 * is decomposed): the rank-regularised training step decomposes fused^T without a transposition pass when the token
 * matrix has fewer rows than columns. */
int r3d_erank_blocked_t(const float* x, int ld, int x_transposed, int R, int C, float* sigma, float* af_t, int* ctrl,
                        float* stats, int max_sweeps, void* stream);
/* coef[k] = gout * d erank / d sigma_k / sigma_k^3; zero for negligible sigma and, with max_rank = min(R, C) > 0, for
 * everything but the max_rank largest (a rank-deficient X has no defined singular vectors beyond its rank). */
int r3d_erank_bwd_coef(const float* sigma, const float* stats, const float* gout, float* coef, int C, int max_rank,
                       void* stream);
int r3d_scale_rows(float* x, int ld, int rows, int cols, const float* coef, void* stream);
/* y[r, :] = x[r, :] * coef[r] (y == x with the same ld: in place, r3d_scale_rows). */
int r3d_scale_rows_into(const float* x, int ldx, float* y, int ldy, int rows, int cols, const float* coef, void* stream);
/* The backward in its well-conditioned form: U = (X V) Sigma^-1, V^T = Sigma^-1 (2 I - U^T U) U^T X (one Neumann term of
 * (U^T U)^-1: the plain V^T = Sigma^-1 U^T X amplifies the residual coupling of a small column with a large one by
 * sigma_j / sigma_i), dX = U diag(g) V^T.  r3d_erank_bwd_coef2: cg[k] = gout * (d erank / d sigma_k) / sigma_k,
 * inv[k] = 1 / sigma_k (zero where r3d_erank_bwd_coef's coefficient is).  r3d_erank_bwd_fix: w[r,:] = cg[r] (2 w[r,:] - p[r,:])
 * on dense [rows, cols] matrices.  The host composes the four GEMMs (r3d_amd/erank.py: erank_backward). */
int r3d_erank_bwd_coef2(const float* sigma, const float* stats, const float* gout, float* cg, float* inv, int C, int max_rank,
                        void* stream);
int r3d_erank_bwd_fix(float* w, const float* p, const float* cg, int rows, int cols, void* stream);
/* The tall rank route's basis clean-up: out [C, C] = I + L, L[i, j] = g2[i, j] / sigma_j^2 where sigma_j > sigma_i (ties:
 * j < i), 0 elsewhere; g2 = (R V)^T (R V).  V^T <- 2 V^T - (I + L) V^T takes out of every right singular vector its
 * component along the vectors of larger singular values (first order). */
int r3d_erank_deflate_mask(const float* g2, const float* sigma, float* out, int C, void* stream);
/* r3d_erank_jacobi that also carries the right singular basis (batch == 1): every rotation is applied to the rows of
 * V^T as well, vt_out [C][C] = (V0 V')^T.  vt_in = V0^T from an earlier decomposition of a nearby matrix and x = X V0
 * (NULL: identity): a warm start, 3-5 sweeps instead of 10-11.  Matrix and basis must fit the LDS together
 * (r3d_erank_lds_bytes_v).  r3d_erank_vt_polish: one Newton-Schulz step vt <- 1.5 vt_raw - 0.5 gv with
 * gv = (vt_raw vt_raw^T) vt_raw, which keeps the carried basis orthogonal to rounding over many steps. */
int64_t r3d_erank_lds_bytes_v(int R, int C);
int r3d_erank_jacobi_warm(const float* x, int ld, int64_t batch_stride, int batch, int R, int C, int gram, float* sigma,
                          float* af_t, float* stats, int max_sweeps, const float* vt_in, float* vt_out, void* stream);
int r3d_erank_vt_polish(const float* vt_raw, const float* gv, float* vt, int64_t n, void* stream);
/* The kernel instance r3d_erank_jacobi_warm (blocked == 0; warm != 0: with vt_out) or r3d_erank_blocked_t (blocked != 0)
 * launches for an [R, C] matrix; host only, no launch.  out[9] = {blocked, G, NCH, EXACT, level, warm, b, nreal, nblk}:
 * level = the LDS kernel's pair order (0 general, 1 level order, 2 level order in 2 x 2 blocks); b, nreal, nblk = the
 * blocked route's columns per block, blocks of real columns and blocks swept (even: a dummy block when nreal is odd).
 * R3D_EINVAL when the route does not take the matrix.  The launchers dispatch on the same plan. */
int r3d_erank_plan(int R, int C, int warm, int blocked, int32_t* out);

/* ---- depth-as-query model (reference model/futr_unsupervised_depth.py) ------------------------------------------------
 * r3d_posenc_fwd / bwd: PositionalEncoding.forward (model/extras/position.py:29-35) on b-major rows,
 *   y[r, :] = dropout(x[r, :] + table[r % S, :]); backward dx = dy * keep * scale, zero where gate <= 0 (gate: NULL or
 *   the post-ReLU embedding of futr_unsupervised_depth.py:97).  drop: NULL or rows*H contiguous keep-bytes.
 * r3d_avgpool_rows_fwd / bwd: F.adaptive_avg_pool1d over the S decoder rows of each clip down to Q rows (:134). */
int r3d_posenc_fwd(const float* x, int ldx, const float* table, int ldt, int S, const uint8_t* drop, float drop_scale,
                   float* y, int ldy, int rows, int H, void* stream);
int r3d_posenc_bwd(const float* dy, int lddy, const uint8_t* drop, float drop_scale, const float* gate, int ldg, float* dx,
                   int lddx, int rows, int H, void* stream);
int r3d_avgpool_rows_fwd(const float* x, int ldx, float* y, int ldy, int B, int S, int Q, int H, void* stream);
int r3d_avgpool_rows_bwd(const float* dy, int lddy, float* dx, int lddx, int B, int S, int Q, int H, void* stream);
/* Label-index queries of model/futr_proposed.py:103-106: out[r, :] = weight[idx[r], :] + table[r % S, :] (nn.Embedding +
 * the sinusoidal table) and the lookup's adjoint d_weight[e, :] = sum_{r : idx[r] == e} d_out[r, :] (deterministic). */
int r3d_embed_gather_fwd(const float* weight, int n_embed, const int64_t* idx, const float* table, int ldt, int S, float* out,
                         int ldo, int rows, int H, void* stream);
int r3d_embed_gather_bwd(const float* d_out, int ldd, const int64_t* idx, float* d_weight, int n_embed, int rows, int H,
                         void* stream);

/* ---- device-resident clip store (r3d_amd/clipcache.py; clipcache.hip) ------------------------------------------------
 * The padded batch of the reference's dataset + my_collate (data/basedataset_darai_depth.py:110-130,174-206) gathered from
 * frame pools in device memory, all five tensors in ONE launch:
 *   features            [B, S_f, D]  row (b, s) = rgb_pool[ids_f[off_f[items[b]] + s]]     or zeros past the item's length
 *   depth               [B, S_d, P]  row (b, s) = depth_pool[ids_d[off_d[items[b]] + s]]   or zeros
 *   past_label          [B, S_l]     lab[off_l[items[b]] + s]                              or pad_idx
 *   trans_future_dur    [B, S_q]     q_dur[off_q[items[b]] + s]                            or (float)pad_idx
 *   trans_future_target [B, S_q]     q_tgt[off_q[items[b]] + s]                            or pad_idx
 * off_* are CSR offsets of n_items + 1 entries (off[0] = 0, off[n_items] = the table's length); items may repeat.  An item id
 * outside [0, n_items) or a pool id outside [0, F) reads nothing and yields padding.  Pools and outputs are dense fp32 rows;
 * any row length collates (16-byte loads when D / P % 4 == 0 and the bases are 16-byte aligned, dword loads otherwise).
 * Extents of 0 (B, S_*, D, P, F) are legal and enqueue nothing for that part.  R3D_EINVAL: a negative extent, a NULL pool
 * with F > 0 rows, or a NULL table / output that a non-empty part would touch. */
typedef struct r3d_clip_collate_job {
    const float* rgb_pool; int64_t F_rgb, D;
    const float* depth_pool; int64_t F_dep, P;
    int64_t n_items;
    const int64_t* off_f; const int64_t* ids_f;
    const int64_t* off_d; const int64_t* ids_d;
    const int64_t* off_l; const int64_t* lab;
    const int64_t* off_q; const float* q_dur; const int64_t* q_tgt;
    const int64_t* items; int64_t B;
    int64_t S_f, S_d, S_l, S_q, pad_idx;
    float* features; float* depth; int64_t* past_label; float* trans_future_dur; int64_t* trans_future_target;
} r3d_clip_collate_job;
int r3d_clip_collate(const r3d_clip_collate_job* job, void* stream);

/* The same launch over a LIST of tracks (r3d_amd/clipcache.py: a layout), for batches that are not the five tensors above: one
 * launch writes tracks[0 .. n_tracks) in that order.  Track t, with item = items[b] and o = off[item]:
 *   R3D_CLIP_FRAMES_F32  out fp32 [B, S, width]  row (b, s) = src[ids[o + s]] (src: a pool of `rows` rows of `width` floats)
 *   R3D_CLIP_WORDS_I64   out int64 [B, S]        src[o + s]                   (src: a table of `rows` words; width = 1)
 *   R3D_CLIP_WORDS_F32   out fp32 [B, S]         src[o + s]
 * for s < off[item + 1] - o; every other element of `out` is written with `pad` (cast to float for the fp32 kinds) by the same
 * launch.  off: CSR of n_items + 1 entries; tracks may share one (two word tracks of one length).  An item id outside
 * [0, n_items), a pool id outside [0, rows) or a word index outside [0, rows) reads nothing and yields padding.
 * Frame rows of R3D_CLIP_WIDE_ROW (256) floats or more take r3d_clip_collate's mapping (one workgroup per destination row and
 * 16-KiB chunk; 16-byte loads when width % 4 == 0 and src / out are 16-byte aligned, dword loads otherwise).  Narrower rows and
 * all word tracks are packed: a workgroup writes 4096 consecutive elements of `out`, element e of a frame track being column
 * e % width of row e / width, so a track of 8-byte rows costs a workgroup per 16 KiB, not per row.  The packed workgroups
 * lead the grid (their dependent loads run under the wide rows' traffic); the outputs keep the tracks' order.
 * B = 0, S = 0 and n_tracks = 0 are legal and enqueue nothing for that part.  R3D_EINVAL, before anything is enqueued: n_tracks
 * outside [0, R3D_CLIP_MAX_TRACKS], an unknown kind, a negative B / n_items / S / rows, and on a track with B S > 0: width <= 0
 * (or != 1 on a word track), a NULL items / off / out, or with rows > 0 a NULL src (or ids, for frames).
 * Enqueue only (capturable), no atomics, all row arithmetic 64-bit. */
#define R3D_CLIP_MAX_TRACKS 8
#define R3D_CLIP_WIDE_ROW 256
enum { R3D_CLIP_FRAMES_F32 = 0, R3D_CLIP_WORDS_I64 = 1, R3D_CLIP_WORDS_F32 = 2 };
typedef struct r3d_clip_track {
    int32_t kind, reserved;
    const void* src; int64_t rows, width;
    const int64_t* off; const int64_t* ids;     /* ids: frame tracks only */
    int64_t S, pad;
    void* out;
} r3d_clip_track;
typedef struct r3d_clip_tracks_job {
    const int64_t* items; int64_t B, n_items;
    int32_t n_tracks, reserved;
    r3d_clip_track tracks[R3D_CLIP_MAX_TRACKS];
} r3d_clip_tracks_job;
int r3d_clip_collate_tracks(const r3d_clip_tracks_job* job, void* stream);

/* ---- bidirectional LSTM layer (model/rnn.py:20,93: nn.LSTM(H, H/2, num_layers=2, bidirectional=True, batch_first=True))
 * The recurrence of one layer, both directions in one launch (one workgroup per clip and direction, W_hh in registers).
 * h = H / 2; rows are b-major (row = b * S + t); direction d (0 forward, 1 reverse) owns columns [4h d, 4h d + 4h) of the
 * gate tensors and [h d, h d + h) of the state tensors.  Gate order i, f, g, o; h0 = c0 = 0; no packing, no masking.
 * r3d_lstm_supported: 8 <= H <= 256, H % 8 == 0.
 * r3d_lstm_layer_fwd: gin [B*S, 8h] = X W_ih^T + b_ih of both directions (the caller's GEMM); b_hh is added here.
 *   Writes y [B*S, 2h] (the layer output), gates [B*S, 8h] (activated), cell [B*S, 2h] (c_t) and hprev [B*S, 2h]
 *   (h_{t-1} in the direction's own order, zero at its first step, so that dW_hh = dG^T hprev per direction).
 * r3d_lstm_layer_bwd: dy [B*S, 2h] = dL/d(layer output); writes dg [B*S, 8h] = dL/d(pre-activation gates).  Then
 *   dW_ih = dG^T X, dW_hh(d) = dG(d)^T hprev(d), d b_ih = d b_hh = column sums of dG, dX = dG W_ih are the caller's GEMMs. */
int r3d_lstm_supported(int H);
int r3d_lstm_layer_fwd(const float* gin, int ldgin, const float* whh_fwd, const float* whh_rev, const float* bhh_fwd,
                       const float* bhh_rev, float* y, int ldy, float* gates, int ldgates, float* cell, int ldcell,
                       float* hprev, int ldhprev, int B, int S, int H, void* stream);
int r3d_lstm_layer_bwd(const float* dy, int lddy, const float* whh_fwd, const float* whh_rev, const float* gates, int ldgates,
                       const float* cell, int ldcell, float* dg, int lddg, int B, int S, int H, void* stream);

/* ---- the same layer, stepwise: one launch per time step, W_hh spread over the chip (csrc/lstm_steps.hip), for hidden sizes
 * whose W_hh no single workgroup holds.  Same tensors and layouts as above, so the GEMMs around the recurrence are unchanged.
 * r3d_lstm_steps_supported: 8 <= H <= 1024, H % 8 == 0.
 * r3d_lstm_steps_ws_floats: the backward's workspace: the dc carry [B, 2h] followed by the transposed W_hh [2][h][4h]
 *   (B H + 2 H H floats); R3D_EINVAL for a shape the route does not take.
 * r3d_lstm_steps_layer_fwd / _bwd: one call enqueues the S step launches of a layer (the backward one transposing launch
 *   first), each checked; nothing waits across workgroups, so the calls can be captured in a hipGraph.  gin, gates, y, dg, ws,
 *   W_hh and b_hh must be 16-byte aligned and ldgin, ldgates, ldy, lddg multiples of 4 (R3D_EALIGN otherwise). */
int r3d_lstm_steps_supported(int H);
int64_t r3d_lstm_steps_ws_floats(int B, int H);
int r3d_lstm_steps_layer_fwd(const float* gin, int ldgin, const float* whh_fwd, const float* whh_rev, const float* bhh_fwd,
                             const float* bhh_rev, float* y, int ldy, float* gates, int ldgates, float* cell, int ldcell,
                             float* hprev, int ldhprev, int B, int S, int H, void* stream);
int r3d_lstm_steps_layer_bwd(const float* dy, int lddy, const float* whh_fwd, const float* whh_rev, const float* gates,
                             int ldgates, const float* cell, int ldcell, float* dg, int lddg, int B, int S, int H, float* ws,
                             void* stream);

/* ---- temporal convolution (reference model/tcn.py: weight_norm(nn.Conv1d(C_in, C_out, 3, padding=2d, dilation=d)) + Chomp1d)
 * Activations are [rows = B*S, C] row-major, a clip's S frames consecutive; tap j of weight_v [C_out, C_in, 3] reads frame
 * t - (2 - j) d of the same clip (zeros before frame 0).  The three products are fp32-MFMA tile GEMMs whose operand loader
 * applies the frame shift and the clip mask: no im2col copy exists.  Weight normalisation stays factored: s = g / |v|.
 * r3d_tconv_supported: rows % S == 0, c_in and c_out multiples of 32, rows * max(c_in, c_out) < 2^31, rows <= 64 * 65535.
 * r3d_tconv_wnorm: s[o] = g[o] / |v[o]|, inv_norm[o] = 1 / |v[o]| (norm over the C_in * 3 values, fixed order).
 * r3d_tconv_fwd: P = X (*) v (raw, written when p_out != NULL); y = dropout(relu(s P + bias)) (drop: NULL or rows * c_out
 *   keep-bytes); with out != NULL also out = relu(y + res) (the block's residual sum).
 * r3d_tconv_bwd_prep: dz = (y > 0) ? drop_scale * dy : 0; d_bias = column sums of dz; d_g[o] = <dz[:, o], p[:, o]> inv_norm[o];
 *   coef[o] = <dz[:, o], p[:, o]> inv_norm[o]^2.  ws: r3d_tconv_ws_floats(rows, c_out) floats (chunk partials, summed in order).
 * r3d_tconv_dx: dx = sum_j shift_j(dz * s) v_j [+ res], zeroed where gate <= 0 (gate: NULL or the ReLU output below).
 * r3d_tconv_wgrad: d_v = s (G - coef v) with G[o, c, j] = sum_r dz[r, o] x[r - (2 - j) d, c]; coef == NULL: d_v = G (s NULL: 1).
 *   Long batches are cut into row ranges (one partial G each, summed range by range: one order); ws holds the partials,
 *   r3d_tconv_wgrad_ws_floats(rows, c_in, c_out) floats (0: none needed, ws may be NULL).
 * r3d_ce_rows_fwd_bwd: utils.py cal_loss without smoothing or excluded class over `rows` logit rows: loss_out[1] = loss_out[3]
 *   = mean over ALL rows of (CE of the rows whose target != pad_idx) + 2 [argmax == pad_idx]; counts[2], counts[3] = correct,
 *   total over those rows; d_logits (NULL: none) = d loss / d logits.  A target outside [0, C) is treated as padding.
 *   One workgroup walks all rows (fixed order): sized for the B * 8 rows of this model, rows <= 65536, C <= 65536. */
int r3d_tconv_supported(int rows, int S, int c_in, int c_out, int dilation);
int64_t r3d_tconv_ws_floats(int rows, int c_out);
int r3d_tconv_wnorm(const float* v, const float* g, int c_in, int c_out, float* s, float* inv_norm, void* stream);
int r3d_tconv_fwd(const float* x, int ldx, const float* v, const float* s, const float* bias, int rows, int S, int c_in,
                  int c_out, int dilation, float* p_out, int ldp, float* y, int ldy, const uint8_t* drop, float drop_scale,
                  const float* res, int ldres, float* out, int ldout, void* stream);
int r3d_tconv_bwd_prep(const float* dy, int lddy, const float* y, int ldy, const float* p, int ldp, float drop_scale,
                       const float* inv_norm, int rows, int c_out, float* dz, int lddz, float* d_bias, float* d_g, float* coef,
                       float* ws, void* stream);
int r3d_tconv_dx(const float* dz, int lddz, const float* v, const float* s, int rows, int S, int c_in, int c_out, int dilation,
                 const float* res, int ldres, const float* gate, int ldgate, float* dx, int lddx, void* stream);
int r3d_tconv_wgrad(const float* dz, int lddz, const float* x, int ldx, const float* v, const float* s, const float* coef,
                    int rows, int S, int c_in, int c_out, int dilation, float* d_v, float* ws, void* stream);
int64_t r3d_tconv_wgrad_ws_floats(int rows, int c_in, int c_out);
int r3d_ce_rows_supported(int rows, int C);
int r3d_ce_rows_fwd_bwd(const float* logits, int ld, const int64_t* target, int rows, int C, int pad_idx, float* loss_out,
                        int64_t* counts, float* d_logits, int ldd, void* stream);

/* ---- streaming QR: the effective rank of a whole data set (qr_stream.hip) --------------------------------------------
 * R [lanes, H, H] fp32, row-major, upper triangular (the strictly lower part stays zero): lanes independent accumulators
 * with R^T R = sum X^T X over the rows folded in, never forming the square.  One workgroup per lane; every reduction has
 * a fixed order, no atomics, no workgroup waits on another: the same (lanes, call sequence) gives the same bits.
 * r3d_qr_append_supported: 1 <= H <= 2048.  r3d_qr_append_tile_rows: the rows of one LDS tile at width H (0: refused).
 * r3d_qr_append: folds the rows of x [n, H] (row stride ldx >= H) in; lane g takes rows [g ceil(n / lanes), ...).
 *   row_label (NULL: every row counts) and pad_idx as key_label / pad_idx of r3d_mha_tiled_fwd: a row whose label equals
 *   pad_idx is staged as zeros, and a zero row changes nothing.  rows (NULL: not counted) int64 [lanes]: each lane adds
 *   its count of valid rows to its own slot.  n = 0 is a no-op; 1 <= lanes <= 64.
 * r3d_qr_merge: lane g + stride is folded into lane g (R and rows) for every g that is a multiple of 2 stride, in one
 *   launch; stride = 1, 2, 4, ... < lanes leaves the total in lane 0.  The source lanes are left as they are. */
int r3d_qr_append_supported(int H);
int r3d_qr_append_tile_rows(int H);
int r3d_qr_append(const float* x, int64_t ldx, int n, int H, const int64_t* row_label, int pad_idx, float* R, int64_t* rows,
                  int lanes, void* stream);
int r3d_qr_merge(float* R, int64_t* rows, int H, int lanes, int stride, void* stream);

/* ---- blocked fold into the same accumulators (qr_fold_wy.hip): the in-step rank penalty on tall token matrices ----------
 * r3d_qr_append's contract without labels (every row counts, nothing is counted), computed panel by panel in the
 * compact-WY form: 16 columns are factored with the reflector formula, everything right of them is updated by fp32-input
 * MFMA products.  The result is upper triangular with R^T R = sum X^T X (diagonal signs free, not the bits of
 * r3d_qr_append) and feeds r3d_qr_merge.  Fixed-order sums, no atomics: the same call gives the same bits.
 * r3d_qr_fold_wy_supported: H a multiple of 16 whose LDS tile keeps at least 32 rows next to 16 staged rows of R
 *   (16 <= H <= 720).  r3d_qr_fold_wy_tile_rows: the rows of one tile at width H (a multiple of 16; 0: refused).
 * r3d_qr_fold_wy: n = 0 is a no-op; 1 <= lanes <= 64; ldx >= H; a refused H is R3D_EINVAL before any launch. */
int r3d_qr_fold_wy_supported(int H);
int r3d_qr_fold_wy_tile_rows(int H);
int r3d_qr_fold_wy(const float* x, int64_t ldx, int n, int H, float* R, int lanes, void* stream);

/* ---- supervised contrastive loss (supcon.hip; reference loss/spc.py SupConLoss) -----------------------------------------
 * x [N, D] fp32 (row stride ldx >= D): the contrast rows, view by view; row r carries labels[r mod bsz] (int64 [bsz];
 * NULL: the sample index r mod bsz, the SimCLR case) and N is a multiple of bsz.  The first A rows are anchors (A = N:
 * contrast_mode 'all', A = bsz: 'one').  With s_ij = x_i . x_j / temperature, C(i) = { j != i : row j not ignored },
 * lse_i = log sum_{C(i)} exp s_ij, Pos(i) = { j in C(i) : y_j = y_i }, P_i = |Pos(i)|:
 *   loss = sum over non-ignored anchors with P_i > 0 of -(temperature / base_temperature) (mean_{Pos(i)} s_ij - lse_i),
 *          divided by max(1, number of non-ignored anchors n_a).
 * A row is ignored when has_ignore != 0, labels != NULL and its label equals ignore_index: neither anchor nor contrast.
 * A row with no admissible contrast (N = 1, everything else ignored) contributes 0.  normalize != 0: every row is divided
 * by max(|x|, 1e-12) while it is staged (F.normalize); no normalised copy is written.  64 x 64 score tiles streamed through
 * LDS under an online log-sum-exp that never includes the diagonal: no N x N tensor, fixed-order reductions, no atomics
 * (the same call gives the same bits), no allocation, no host synchronisation.
 * ws: r3d_supcon_ws_floats(N) floats owned by the caller: lse [N], positive mean [N], P [N], 1 / max(|x|, 1e-12) [N]
 *   (1 without normalize) and n_a; the forward writes it, the backward reads it.  Rows >= A keep lse, mean and P unwritten.
 * r3d_supcon_fwd: loss_out[0] = loss.
 * r3d_supcon_bwd: the forward's arguments again; dx [N, D] (row stride lddx >= D) = (add != 0 ? dx : 0) + gscale * d_loss[0]
 *   * d loss / d x, d_loss a device scalar (NULL: 1).  One launch, one sweep of the column tiles per 64-row tile.
 * r3d_supcon_supported: 1 <= D <= 256 (host-only).  A refused shape returns R3D_EINVAL before anything is enqueued. */
int r3d_supcon_supported(int D);
int64_t r3d_supcon_ws_floats(int N);
int r3d_supcon_fwd(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                   int64_t ignore_index, float temperature, float base_temperature, int normalize, float* ws,
                   float* loss_out, void* stream);
int r3d_supcon_bwd(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                   int64_t ignore_index, float temperature, float base_temperature, int normalize, const float* ws,
                   const float* d_loss, float gscale, float* dx, int lddx, int add, void* stream);
/* The wide route (opt-in): the same loss on rows of 1 <= D <= 2048 columns, the width walked in chunks of 256 columns.
 * D <= 256 makes the launches of the pair above (the same bits).  257 <= D: the score tile is accumulated over the chunks
 * before the statistics read it; normalize != 0 computes 1 / max(|x|, 1e-12) per row in a launch of its own and scales the
 * scores by it (the rows are staged raw); the backward runs one workgroup per (64-row tile, 256-column chunk of dx), and
 * with normalize stages dz in ws and finishes dx = (dz - z (z . dz)) / |x| in a row epilogue launch.  The conditions of
 * the pair above hold for every launch.
 * r3d_supcon_wide_ws_floats: the layout above (4 N + 4 floats), then with normalize and D > 256 dz [N, D], which the
 *   backward writes (hence no const on its ws).  0 for a refused shape.
 * r3d_supcon_wide_supported: 1 <= D <= 2048 (host-only).  A refused shape returns R3D_EINVAL before anything is enqueued. */
int r3d_supcon_wide_supported(int D);
int64_t r3d_supcon_wide_ws_floats(int N, int D, int normalize);
int r3d_supcon_wide_fwd(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                        int64_t ignore_index, float temperature, float base_temperature, int normalize, float* ws,
                        float* loss_out, void* stream);
int r3d_supcon_wide_bwd(const float* x, int ldx, const int64_t* labels, int bsz, int N, int A, int D, int has_ignore,
                        int64_t ignore_index, float temperature, float base_temperature, int normalize, float* ws,
                        const float* d_loss, float gscale, float* dx, int lddx, int add, void* stream);

/* ---- temporal auxiliary losses (temporal.hip; reference utils.py :229-321, :493; train_unsupervised.py :34) --------------
 * Every call enqueues only; no allocation, no atomics, fixed-order reductions (the same call gives the same bits), no host
 * synchronisation.  B >= 1 clips of T >= 1 frames, B T < 2^30, B <= 65535; rows are x [B T, W] with row stride ldx >= W.
 * r3d_label_runs: labels int64 [B, T].  A run starts at t = 0 and wherever labels[b, t] != labels[b, t - 1].  Writes, all
 *   int32: first / last [B, T] (the first and last frame of the frame's run), starts [B, T] (starts[b, r] = first frame of
 *   run r, T past the last run), count [B].  One launch.
 * r3d_temporal_width_supported: 1 <= W <= 256, the width limit of both losses below (host-only).
 *
 * Cluster loss, x [B T, C]: run r of clip b has n_r frames and mean m_r, R_b = count[b], total = sum_b R_b,
 *   loss = sum_{b,r} (1 / (n_r C)) sum_{t in r, c} (x - m_r)^2 / total
 *        + sum_{b: R_b > 1} sum_{i<j} 1 / (1e-5 + |m_i - m_j|) / (M (n_last - 1)),
 *   M = clips with R_b > 1, n_last = R_b of the last of them in batch order (0 when M = 0).  The backward takes the
 *   gradient of |m_i - m_j| as 0 where it is 0.  T <= 32 * 65535.
 * ws: r3d_tcluster_ws_floats(B, T, C) floats: the run means, the runs' intra terms, the pair-tile partials, 1 / total and
 *   1 / (M (n_last - 1)); the forward writes it, the backward reads it.
 * r3d_tcluster_bwd: dx (row stride lddx >= C) = (add != 0 ? dx : 0) + gscale * d_loss[0] * d loss / d x; d_loss a device
 *   scalar (NULL: 1).
 *
 * Contrastive loss, x [B T, D]: z = x / max(|x|, 1e-12), s = z z^T / temperature per clip, p_tc = softmax over all c of the
 *   clip.  Frame t of the run (st, en): P(t) = { c : st <= c <= en, c != t - st }, |P_r| = sum_{t in r} |P(t)|,
 *   loss = sum_b sum_r sum_{t in r} sum_{c in P(t)} -log(p_tc + 1e-5) / (|P_r| + 1e-5) / B.
 * 64 x 64 score tiles streamed through LDS, no [T, T] tensor.  ws: r3d_tcontrast_ws_floats(B, T) = 5 B T floats: lse, Q_t =
 *   sum_{P(t)} p / (p + 1e-5), 1 / max(|x|, 1e-12), the row's loss term and max(|x|, 1e-12).  r3d_tcontrast_bwd: dx as above, one launch.
 *
 * Focal loss, pred [N, C] (row stride ld >= C, any C >= 1), gold int64 [N].  A row is masked when gold equals pad_idx,
 *   or exclude_idx with has_exclude != 0, or lies outside [0, C).  With CE = lse - pred[gold], p = exp(-CE):
 *   loss = sum over unmasked rows of alpha (1 - p)^gamma CE + penalty_weight [argmax == pad_idx], divided by N.  gamma >= 1.
 * r3d_focal_rows: loss_out != NULL: loss_out[0] = loss, flags uint8 [N] = [unmasked and argmax == gold], counts int64 [2] =
 *   (sum of flags, unmasked rows), ws [N] floats of scratch.  d_pred != NULL: d_pred (row stride lddp >= C) = (add != 0 ?
 *   d_pred : 0) + gscale * d_loss[0] * d loss / d pred.  At least one of loss_out and d_pred.
 * A refused shape returns R3D_EINVAL before anything is enqueued. */
int r3d_label_runs(const int64_t* labels, int B, int T, int* first, int* last, int* starts, int* count, void* stream);
int r3d_temporal_width_supported(int W);
int64_t r3d_tcluster_ws_floats(int B, int T, int C);
int r3d_tcluster_fwd(const float* x, int ldx, int B, int T, int C, const int* starts, const int* last, const int* count,
                     float* ws, float* loss_out, void* stream);
int r3d_tcluster_bwd(const float* x, int ldx, int B, int T, int C, const int* starts, const int* last, const int* count,
                     const float* ws, const float* d_loss, float gscale, float* dx, int lddx, int add, void* stream);
int64_t r3d_tcontrast_ws_floats(int B, int T);
int r3d_tcontrast_fwd(const float* x, int ldx, int B, int T, int D, const int* first, const int* last, float temperature,
                      float* ws, float* loss_out, void* stream);
int r3d_tcontrast_bwd(const float* x, int ldx, int B, int T, int D, const int* first, const int* last, float temperature,
                      const float* ws, const float* d_loss, float gscale, float* dx, int lddx, int add, void* stream);
int r3d_focal_rows(const float* pred, int ld, const int64_t* gold, int N, int C, int64_t pad_idx, int has_exclude,
                   int64_t exclude_idx, float alpha, float gamma, float penalty_weight, float* ws, float* loss_out,
                   uint8_t* flags, int64_t* counts, const float* d_loss, float gscale, float* d_pred, int lddp, int add,
                   void* stream);

/* ---- AFFT baseline: the pooled-head chain (csrc/afft.hip; model/afft.py:189-201 of the reference) ----------------
 * Behind the fused tokens [B S, H] the model is pooled = adaptive_avg_pool1d(fused, Q) (window of output q:
 * [floor(q S / Q), ceil((q + 1) S / Q)), padded frames included) and actdur = pooled . w_head^T + b_head with w_head =
 * [fc.weight ; fc_len.weight] [K + 1, H].  One workgroup per clip.
 * r3d_afft_head_fwd: writes pooled [B Q, H] (contiguous) and out [B Q, K + 1] (row stride ld_out); reads the fields up to
 *   ld_out, B, S, Q, K, H only.
 * r3d_afft_head_step: the same, then the clip's anticipation CE rows and duration unit exactly as r3d_losses_fwd_bwd computes
 *   them (pad_idx, exclude_idx, dur_den, grad_scale as there), d_out [B Q, K + 1] = d(total) / d(out) * grad_scale, and
 *   d_fused [B S, H] (row stride ld_dfused) = (add != 0 ? d_fused : 0) + gscale * pool^T(d_out . w_head).  The loss partials go
 *   to ws (r3d_losses_ws_floats(B, S, Q) floats, 16-byte aligned) in r3d_losses_fwd_bwd's unit layout
 *   with the B S segmentation units written as zeros (no precondition on what ws held): reduce them with r3d_losses_finalize or r3d_adamw_flat*_fin and
 *   has_seg = 0.  tick_a / tick_b (optional device int64) are incremented once per call.  No atomics; the same call gives
 *   the same bits.
 * r3d_afft_head_supported (host-only): H % 4 == 0, H <= 1024, Q <= 64, 2 <= n_head <= 1024 and Q * (H + n_head) floats
 *   within 152 KiB of LDS.  A refused shape returns R3D_EINVAL before anything is enqueued; fused, pooled, w_head, d_fused
 *   and ws 16-byte aligned, ld_fused and ld_dfused multiples of 4 (R3D_EALIGN). */
typedef struct r3d_afft_head_args {
    const float* fused; int32_t ld_fused;
    const float* w_head; const float* b_head; int32_t n_head;       /* n_head = K + 1 */
    float* pooled; float* out; int32_t ld_out;
    int32_t B, S, Q, K, H;
    const int64_t* past_label; const int64_t* target; const float* target_dur;
    int32_t pad_idx, exclude_idx;
    const float* dur_den; float grad_scale;
    float* d_out; int32_t ld_dout;
    float* d_fused; int32_t ld_dfused; float gscale; int32_t add;
    int64_t* tick_a; int64_t* tick_b;
} r3d_afft_head_args;
int r3d_afft_head_supported(int H, int Q, int n_head);
int r3d_afft_head_fwd(const r3d_afft_head_args* args, void* stream);
int r3d_afft_head_step(const r3d_afft_head_args* args, float* ws, void* stream);

/* ---- CNN baseline: the segmentation-head step (csrc/cnn.hip; model/cnn.py of the reference: seg = fc_seg(x)) -------------
 * One launch over the N = B S frame rows, one workgroup per 64 rows:
 *   logits = x . w^T + b [N, Kseg], stored to seg (row stride ld_seg) when seg is not NULL;
 *   unit r of ws (r3d_losses_fwd_bwd's layout, r3d_losses_ws_floats(B, S, Q) floats with N = B S) = the segmentation unit
 *     r3d_losses_fwd_bwd_kseg computes for row r: masked when labels[r] is pad_idx, exclude_idx or outside [0, Kseg), + 2
 *     when the arg-max (first occurrence of the largest logit) is pad_idx; reduce with has_seg = 1.  Only the N segmentation
 *     units are written: run it AFTER r3d_afft_head_step on the same ws (which zeroes them and writes the others);
 *   d_seg [N, Kseg] (row stride ld_dseg) = (softmax(logits) - onehot) grad_scale / N, zero on masked rows;
 *   d_pre [N, H] = (x > 0) ? d_seg . w + d_x0 + d_extra : 0; d_x0 and d_extra are optional [N, H] with their own row strides.
 * w [Kseg, H] contiguous.  No atomics; the same call gives the same bits.
 * r3d_cnn_seg_supported (host-only): H % 4 == 0, 8 <= H <= 256, 1 <= Kseg <= 1023.  A refused shape returns R3D_EINVAL
 * before anything is enqueued; x, w, d_x0, d_extra, d_pre and ws 16-byte aligned, ld_x, ld_dx0, ld_dextra and ld_dpre
 * multiples of 4 (R3D_EALIGN). */
typedef struct r3d_cnn_seg_args {
    const float* x; int32_t ld_x;
    const float* w; const float* b;
    const int64_t* labels;
    int32_t N, H, Kseg;
    int32_t pad_idx, exclude_idx; float grad_scale;
    float* seg; int32_t ld_seg;
    float* d_seg; int32_t ld_dseg;
    const float* d_x0; int32_t ld_dx0;
    const float* d_extra; int32_t ld_dextra;
    float* d_pre; int32_t ld_dpre;
} r3d_cnn_seg_args;
int r3d_cnn_seg_supported(int H, int Kseg);
int r3d_cnn_seg_step(const r3d_cnn_seg_args* args, float* ws, void* stream);

/* ---- L3 query model: cross-clip attention (csrc/attention_xclip.hip; model/futr_unsupervised_temp3.py:99-102) --------------
 * nn.MultiheadAttention(batch_first=True) called after 'b t c -> t b c': for each frame t and head h the B rows { b S + t }
 * attend to one another, no mask, no dropout.  qkv [B S, 3 H] (row stride ld >= 3 H, H = heads dh) is the in-projection
 * output, columns [q | k | v], head h at columns h dh of each part; it is read in place (the keys of one group lie S ld
 * floats apart), no transposed copy is made.
 * r3d_xclip_fwd: o [B S, H] (row stride ldo) = softmax(q k^T / sqrt(dh)) v per (t, h).
 * r3d_xclip_bwd: d_qkv [B S, 3 H] (row stride lddq), every element written once (not accumulated), from qkv and d_o [B S, H]
 *   (row stride lddo); the probabilities are recomputed.
 * Each launch enqueues only; no atomics, fixed-order sums (the same call gives the same bits).  16-byte loads are used where
 * the pointers, row strides and column offsets are multiples of 4 floats; any alignment runs.
 * r3d_xclip_supported (host-only): 1 <= B <= 64, 1 <= dh <= 128; also S >= 1 and B S 3 H < 2^31.  A refused shape returns
 *   R3D_EINVAL before anything is enqueued.
 * r3d_xclip_frame_run (host-only): the consecutive frames one workgroup owns at that shape (0: refused). */
int r3d_xclip_supported(int B, int dh);
int r3d_xclip_frame_run(int B, int S, int heads, int dh, int bwd);
int r3d_xclip_fwd(const float* qkv, int ld, float* o, int ldo, int B, int S, int heads, int dh, void* stream);
int r3d_xclip_bwd(const float* qkv, int ld, const float* d_o, int lddo, float* d_qkv, int lddq, int B, int S, int heads,
                  int dh, void* stream);

/* ---- L3 query loop: the loss mix (csrc/l3mix.hip; train/train_unsupervised.py:357-362) -------------------------------------
 * Over the N = B S frame rows: l2_correct[r] = [past_label[r] != pad_idx and argmax(seg[r]) == past_label[r]] (the first
 * index of the maximum; seg [N, Kseg], row stride ld_seg), l3_flags the flags of r3d_focal_rows,
 *   m = mean_r (l3_flags[r] && l2_correct[r] ? 1 : 5),  c = 1/m,  a = (1 - c)(1 - wf),  b = (1 - c) wf,
 *   total = (1 - c)((1 - wf) l3[0] + wf lc[0]) + c ((loss3[1] + loss3[2]) + loss3[0]),
 * loss3 = the loss_out of r3d_losses_fwd_bwd (seg, action, duration); l3, lc, wf device scalars.  Writes out[5] = (m, a, b,
 * c, total), l2_flags uint8 [N] when not NULL, and multiplies d_seg [N, Kseg] (row stride ld_dseg) and d_actdur [rows_ad,
 * cols_ad] (row stride ld_dad) by c in place (either may be NULL).  ws: r3d_l3mix_ws_ints(N) int32 of scratch.  Two launches,
 * enqueue only; the count behind m is an integer sum: no float atomics, the same call gives the same bits. */
int64_t r3d_l3mix_ws_ints(int N);
int r3d_l3mix(const float* seg, int ld_seg, const int64_t* past_label, const uint8_t* l3_flags, int N, int Kseg, int pad_idx,
              const float* l3, const float* lc, const float* loss3, const float* wf, float* d_seg, int ld_dseg,
              float* d_actdur, int rows_ad, int cols_ad, int ld_dad, uint8_t* l2_flags, int* ws, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3D_HIP_H */
