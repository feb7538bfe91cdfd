/* libaudiolm_hip.so -- C ABI of the MI355X (gfx950) kernels behind the audiolm token-transformer training hot path.
 *
 * The reference (lucidrains/audiolm-pytorch) has no FFI of its own: its hot path is stock PyTorch ops.  This header is the
 * drop-in boundary a maintainer binds instead of those ops (ctypes stub: INTEGRATION.md; the in-tree binding is
 * audiolm-pytorch_amd/_lib.py).  Each entry cites the reference code it replaces (paths relative to
 * /root/reference/audiolm_pytorch/).
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer owned by the caller (PyTorch allocator), incl. workspaces
 *   - bf16 tensors are raw uint16 bit patterns (void*); fp32 statistics / master weights / gradients are float*
 *   - `ld*` = leading dimension (row stride) in ELEMENTS; row-major everywhere
 *   - kernels are stateless, re-entrant, asynchronous on `stream` (a hipStream_t passed as void*); callable from any thread.
 *     The launchers' only process state is the dynamic-LDS limit table (csrc/launch.hpp): which (kernel, device) pairs already had
 *     hipFuncAttributeMaxDynamicSharedMemorySize raised, guarded by a mutex -- a second GPU gets its own entries
 *   - return 0 on success, a hipError_t value (> 0) or ALM_ERR_* (>= 10001) otherwise; nothing is printed
 */
#pragma once
#ifdef __cplusplus
extern "C" {
#endif

#define ALM_ERR_BAD_ARG 10001
#define ALM_ERR_UNSUPPORTED 10002

/* ---- dense contractions (MFMA) -------------------------------------------------------------------------------------------
 * C[z1][z2][M,N] (+)= alpha * A[z1][z2][M,K] . B[z1][z2][N,K]^T (+ bias[N]);  bf16 operands, fp32 accumulate, C bf16 or fp32.
 * Replaces aten::mm / addmm / bmm behind nn.Linear and einsum at audiolm_pytorch.py:255-259 (FFN), :351 (to_q, to_kv),
 * :395 (to_out), :719 / :961 (semantic logits, bias), :972 / :1335 / :1350 (per-quantizer logit heads, batched over z2 = q),
 * and all their dgrad / wgrad forms (operands transposed with alm_transpose_bf16 / alm_pack_weight).
 * K % 8 == 0, lda/ldb % 8 == 0, batch strides % 8 == 0. */
int alm_gemm_bf16_nt(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long long lda, long long ldb,
                     long long ldc, int nb1, int nb2, long long sA1, long long sA2, long long sB1, long long sB2, long long sC1,
                     long long sC2, float alpha, int out_f32, int accumulate, void* stream);
/* alm_gemm_bf16_nt with a caller-owned workspace (round 6): NT launches that leave most of the chip idle on 256 x 256 tiles (every D- / 512-wide projection
 * of audiolm_pytorch.py:255-259, :351, :395 at M = 8192 rows; to_q / dAO at M = 16384) run on the staggered 256 x 256 tile with IN-LAUNCH split-K when the
 * measured cost model picks it (alm_gemm_nt_plan): each K slice publishes its fp32 accumulators to `ws`, the tile's LAST ARRIVER (per-tile ticket counter,
 * agent scope) sums them in fixed slice order and runs the usual epilogue (alpha, bias, accumulate, bf16 / fp32) -- bitwise deterministic, one launch.
 * ws: alm_gemm_nt_ws_bytes() bytes, 16-byte aligned, used by one stream at a time; its first 4096 bytes (the counters) must be ZERO when first handed over,
 * every launch leaves them zero.  ws == NULL or too small: exactly alm_gemm_bf16_nt. */
int alm_gemm_bf16_nt_ws(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long long lda, long long ldb, long long ldc,
                        int nb1, int nb2, long long sA1, long long sA2, long long sB1, long long sB2, long long sC1, long long sC2, float alpha,
                        int out_f32, int accumulate, void* ws, long long ws_bytes, void* stream);
/* un-batched, with a GIVEN number of K slices on the staggered 256 x 256 tile (tests / scripts/ab_nt_inl.py); slices 1 = the plain staggered tile; M, N >= 256 */
int alm_gemm_bf16_nt_inl(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long long lda, long long ldb, long long ldc,
                         float alpha, int out_f32, int accumulate, int slices, void* ws, long long ws_bytes, void* stream);
/* plan of alm_gemm_bf16_nt_ws (with_ws = 1) / alm_gemm_bf16_nt (0) for nb problems, no launch: plan[0] = block tile (1 = 128 x 128, 16 = its 4-stage DMA-ring
 * form, 13 = 256 x 256 staggered, 11 = 384 x 256), plan[1] = K slices (1: no split), plan[2] = workspace bytes that plan uses, plan[3] = workgroups */
int alm_gemm_nt_plan(int M, int N, int K, int nb, int with_ws, int* plan);
int alm_gemm_nt_ws_bytes(void);
/* two independent un-batched NT problems (bf16 or fp32 outputs, no bias, alpha 1) in ONE launch: pairs of projections that sit next to each other in
 * the step and each leave most of the chip idle on their own -- to_q || to_kv (audiolm_pytorch.py:351 / :347: x_norm . Wq^T beside x . Wkv^T) and their two
 * dgrads.  Falls back to two launches when the problems do not pick the same tile; results are identical either way. */
int alm_gemm_bf16_nt_group2(const void* A0, const void* B0, void* C0, int M0, int N0, int K0, long long lda0, long long ldb0, long long ldc0,
                            const void* A1, const void* B1, void* C1, int M1, int N1, int K1, long long lda1, long long ldb1, long long ldc1,
                            int out_f32, void* stream);
/* tile-selectable, un-batched form of alm_gemm_bf16_nt (tests / benchmarks): tile 0 = auto, 1 = 128x128x64 (4 waves), 2 = 256x256x64
 * (8 waves, lock-step), 13 = 256x256x64 with staggered wave rows (the production big tile), 11 = 384x256x64 (8 waves); other ids ->
 * ALM_ERR_UNSUPPORTED (the variants that were measured and not adopted live in the bench-only csrc/lab/gemm_lab.hip). */
int alm_gemm_bf16_nt_tile(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long long lda, long long ldb,
                          long long ldc, float alpha, int out_f32, int accumulate, int tile, void* stream);
/* split-K forms for long-K / few-tile contractions (weight gradients: K = B*N tokens): fp32 C (+)= alpha * op(A) . op(B),
 * deterministic two-stage reduction through `ws` (alm_gemm_splitk_ws_floats(M,N,K,nb) floats; may be NULL when that
 * query returns 0).  `nb` same-shape problems per launch with element strides sA / sB / sC between them (sA, sB % 8 == 0).
 *   _nt_: A[M][K], B[N][K] (K-contiguous operands)
 *   _tn_: At[K][M], Bt[K][N] (contraction-major operands = the row-major activations themselves):
 *         dW[out][in] = sum_tokens dY[token][out] * X[token][in], the wgrad of every nn.Linear on the path
 *         (autograd of audiolm_pytorch.py:255-259, :351, :395, :961, :972) with no transposed copies; lda/ldb % 8 == 0. */
int alm_gemm_splitk_slices(int M, int N, int K, int nb);
int alm_gemm_splitk_ws_floats(int M, int N, int K, int nb);
/* block tile of the split-K plan for this problem: 1 = 128 x 128 (4 waves), otherwise a 256 x 256 tile */
int alm_gemm_splitk_tile(int M, int N, int K, int nb);
/* host-side plan queries (no launch): the kernel a launch WILL take.  The launchers and these queries (alm_gemm_nt_plan and the split-K / grouped ones
 * too) call ONE set of decision functions (csrc/gemm_plan.hpp, final_tile for the block tile), so a query cannot drift from the launch it describes.
 *   alm_gemm_nt_tile_choice: block tile of alm_gemm_bf16_nt(M, N) with nb = nb1 * nb2 problems: 1 = 128 x 128 (4 waves), 13 = 256 x 256 with staggered
 *     wave rows, 11 = 384 x 256 (the shipped choice; A/B environment hooks not applied)
 *   alm_gemm_tn_batched_plan: alm_gemm_bf16_tn_batched(M, N, K) over nb problems -> 0 = one full-K launch, 1 = uniform split-K (plan = {tile, slices, 0, 0}),
 *     2 = hybrid: plan = {panels at full K, slices of the tail, first row / column of the tail in the last problem, tail cut along M}; plan: int[4] | NULL */
int alm_gemm_nt_tile_choice(int M, int N, int nb);
int alm_gemm_tn_batched_plan(int M, int N, int K, int nb, int* plan);
int alm_gemm_bf16_nt_splitk(const void* A, const void* B, float* C, float* ws, int M, int N, int K, long long lda, long long ldb,
                            long long ldc, int nb, long long sA, long long sB, long long sC, float alpha, int accumulate, void* stream);
int alm_gemm_bf16_tn_splitk(const void* At, const void* Bt, float* C, float* ws, int M, int N, int K, long long lda, long long ldb,
                            long long ldc, int nb, long long sA, long long sB, long long sC, float alpha, int accumulate, void* stream);
/* two-level batched _tn_ form: C[z1][z2] (+)= alpha * At[z1][z2]^T . Bt[z1][z2] for nb1 x nb2 same-shape problems (element strides per level): every
 * layer's gradient of one weight kind in ONE launch from stacked activation buffers (the deferred weight-gradient mode of the fused backward).
 * ws: alm_gemm_splitk_ws_floats(M, N, K, nb1 * nb2) floats (NULL when that is 0). */
int alm_gemm_bf16_tn_batched(const void* At, const void* Bt, float* C, float* ws, int M, int N, int K, long long lda, long long ldb, long long ldc,
                             int nb1, int nb2, long long sA1, long long sA2, long long sB1, long long sB2, long long sC1, long long sC2, float alpha,
                             int accumulate, void* stream);
/* Grouped leftovers of the batched weight gradients.  The parts of the _tn_batched calls that do not fill whole rounds of the chip's 256 CUs (the tails of
 * the hybrid plan, the weight kinds with few tiles) are independent and contract over the same K: ONE launch cuts the 256 x 256 tiles of up to 8 jobs into
 * uniform K slices that fill whole rounds, ONE table-driven reduce sums the slices in slice order (a fixed function of the inputs: no atomics).
 * A job is one two-level batched _tn_ problem (every field as in alm_gemm_bf16_tn_batched; 16 eight-byte words, no padding). */
typedef struct {
    const void* At; const void* Bt; float* C;
    int M, N, K, nb1, nb2, accumulate; float alpha; int reserved;
    long long lda, ldb, ldc, sA1, sA2, sB1, sB2, sC1, sC2;
} AlmTnJob;
/*   _batched_panels: step (a) of alm_gemm_bf16_tn_batched's hybrid plan alone -- the panels that fill whole rounds, at full K, straight into C (the same
 *     kernel, raster and arithmetic: those C tiles are bitwise the ones alm_gemm_bf16_tn_batched writes) -- and `rest` = what is left as a job: the tail's
 *     sub-matrix of the last problem, or the whole problem when the plan has no whole round (then nothing is launched).  rest->M == 0: nothing left.
 *   _grouped: the jobs (all of one K) in one launch + one reduce.  slices: 0 = the cost model's choice, > 0 = that many (lowered to what K allows);
 *     1 = no partials, no reduce (ws may be NULL).  ws: alm_gemm_tn_grouped_ws_floats(jobs, njobs, slices) floats.
 *   _grouped_plan (no launch): plan[0] = 256 x 256 tiles of all jobs, plan[1] = slices S, plan[2] = K-steps (of 64) per slice, plan[3] = pieces
 *     (tiles x S), plan[4] = workgroups launched, plan[5] = rounds of the busiest XCD's 32 CUs; plan: int[6] | NULL; returns S (< 0: bad jobs). */
int alm_gemm_bf16_tn_batched_panels(const void* At, const void* Bt, float* C, int M, int N, int K, long long lda, long long ldb, long long ldc,
                                    int nb1, int nb2, long long sA1, long long sA2, long long sB1, long long sB2, long long sC1, long long sC2, float alpha,
                                    int accumulate, AlmTnJob* rest, void* stream);
int alm_gemm_bf16_tn_grouped(const AlmTnJob* jobs, int njobs, float* ws, int slices, void* stream);
int alm_gemm_tn_grouped_plan(const AlmTnJob* jobs, int njobs, int slices, int* plan);
int alm_gemm_tn_grouped_ws_floats(const AlmTnJob* jobs, int njobs, int slices);
/* dst[c][r] = src[r][c]; columns [rows, rows_pad) of dst are zero-filled (K-padding of a transposed GEMM operand). */
int alm_transpose_bf16(const void* src, void* dst, int rows, int cols, long long ld_src, long long ld_dst, int rows_pad, void* stream);
/* nb matrices (element strides bs_src / bs_dst) in ONE launch: the per-sequence key / value sets of a conditioning context (xattn.py). */
int alm_transpose_bf16_batched(const void* src, void* dst, int rows, int cols, long long ld_src, long long ld_dst, int rows_pad, int nb,
                               long long bs_src, long long bs_dst, void* stream);
/* fp32 master weight -> zero-padded bf16 copy (dst, may be NULL) and zero-padded bf16 transpose (dstT, may be NULL).
 * This is the autocast weight cast of trainer.py:1241 (accelerator.autocast), done once per optimiser step. */
int alm_pack_weight(const float* src, int rows, int cols, long long ld_src, void* dst, long long ld_dst, int rows_pad, int cols_pad,
                    void* dstT, long long ld_dstT, void* stream);

/* the same for up to 8 weights in ONE launch (a transformer layer's q / kv / out / W1 x-half / W1 gate-half / W2) */
typedef struct {
    const float* src; int rows, cols; long long ld_src;
    void* dst; long long ld_dst; int rows_pad, cols_pad;
    void* dstT; long long ld_dstT;
} AlmPackJob;
int alm_pack_weights_multi(const AlmPackJob* jobs, int njobs, void* stream);

/* ---- LayerNorm (gamma only, eps 1e-5): audiolm_pytorch.py:191-198 ---------------------------------------------------------- */
/* rows <= 0 returns 0.  Otherwise, before any launch: ALM_ERR_BAD_ARG for a NULL x / gamma / y / mean / rstd / dy / dx, D < 4 or D % 4, a leading
 * dimension that is no multiple of 4 or narrower than D (ldc / lde only with xcopy / extra); ALM_ERR_UNSUPPORTED for D > 2048 and for an fp32 dy with a
 * bf16 x or dx.  alm_colsum / alm_colsum_partial: ALM_ERR_BAD_ARG for a NULL out / ws, and with rows > 0 a NULL in or ld < cols. */
int alm_ln_partial_blocks(int rows);
int alm_layernorm_fwd(const void* x, int x_is_bf16, long long ldx, const float* gamma, void* y, int y_is_f32, long long ldy, void* xcopy_bf16,
                      long long ldc, float* mean, float* rstd, int rows, int D, void* stream);   /* y bf16, or fp32 (final LayerNorm feeding the logit heads) */
int alm_layernorm_bwd(const void* dy, int dy_is_f32, long long lddy, const void* x, int x_is_bf16, long long ldx, const float* mean,
                      const float* rstd, const float* gamma, const void* extra_bf16, long long lde, void* dx, int dx_is_bf16,
                      long long lddx, float* dgamma_part, int rows, int D, void* stream);
/* out[c] (+)= scale * sum_r in[r][c]  (second stage of every parameter-gradient reduction; bias gradients) */
int alm_colsum(const void* in, int in_is_bf16, long long ld, int rows, int cols, float* out, float scale, int accumulate, float* ws,
               void* stream);          /* ws: alm_colsum_chunks(rows) * cols floats (two-stage reduction of tall inputs) or NULL */
int alm_colsum_chunks(int rows);
/* stage 1 alone: ws[alm_colsum_chunks(rows)][cols] partial column sums of an fp32 matrix (the consumer sums the chunk rows: alm_hc_param_grads) */
int alm_colsum_partial(const float* in, long long ld, int rows, int cols, float* ws, void* stream);

/* ---- GEGLU + inner LayerNorm: audiolm_pytorch.py:246-260 (gate = second half, exact-erf GELU, LN over int(dim*8/3)) -------- */
/* standalone GEGLU module (audiolm_pytorch.py:246-249) on fp32 rows [rows][2 inner] -> [rows][inner]: y = x * gelu(gate), gate = the second half.
 * alm_geglu_ln_*: u [rows][ldu] holds the x half at columns [0, inner_pad) and the gate half at [gate_offset, gate_offset + inner_pad); the pad columns
 * [inner, inner_pad) are never counted and come out zero.  rows <= 0 returns 0.  Otherwise, before any launch: ALM_ERR_UNSUPPORTED for inner < 1,
 * inner_pad < inner, inner_pad > 3072, inner_pad / ldu / gate_offset no multiple of 8; ALM_ERR_BAD_ARG for a NULL pointer (dgamma_part may be NULL),
 * gate_offset < inner_pad, ldu < gate_offset + inner_pad, ldo / lddh < inner_pad or no multiple of 4. */
int alm_geglu_fwd(const float* x, float* y, long long rows, int inner, void* stream);
int alm_geglu_bwd(const float* dy, const float* x, float* dx, long long rows, int inner, void* stream);
int alm_geglu_partial_blocks(int rows);
int alm_geglu_ln_fwd(const void* u_bf16, long long ldu, int gate_offset, const float* gamma, void* out_bf16, long long ldo, float* mean,
                     float* rstd, int rows, int inner, int inner_pad, void* stream);
int alm_geglu_ln_bwd(const void* dhn_bf16, long long lddh, const void* u_bf16, long long ldu, int gate_offset, const float* gamma,
                     const float* mean, const float* rstd, void* du_bf16, float* dgamma_part, int rows, int inner, int inner_pad,
                     void* stream);

/* ---- causal multi-query flash attention: attend.py:69-146 as called from audiolm_pytorch.py:381-394 ------------------------
 * q (B,N,H*64) bf16, k/v (B,N,64) bf16 single shared head, mask (B,N) uint8 (1 = attend) or NULL, scale = 64^-0.5.
 * lse fp32 [B][H][N].  Backward: dq bf16; dk/dv fp32 partials [alm_mqa_bwd_parts(B,N,H)][B*N][lddk] (64 columns each, `part_stride`
 * floats between partials; summed by alm_kv_grad_pack: deterministic, no atomics); delta = fp32 workspace [2][B][H][N].
 * dropout_p in [0, 1) / seed: training-mode attention dropout (attend.py:92 `dropout_p`, :140 `attn_dropout(attn)`): the softmax OUTPUT of pair
 * (b, h, i, j) is kept iff hash(seed, b, h, i * N + j) >= dropout_p * 2^32 (a stateless 32-bit finaliser, the same in forward, dQ and dK/dV) and
 * scaled by 1 / (1 - dropout_p); 0 = off (the default path, no cost).  Pass the forward's (dropout_p, seed, seed_dev) to the backward.
 * seed_dev (device uint64 | NULL): when given, the stream is seed + *seed_dev with the counter read when the kernel RUNS -- a hipGraph replay then
 * draws a new mask each time (a by-value seed is baked into the captured launch); the caller advances the counter on the device between steps.
 * A query without a visible key (every key j <= i masked) gets o = 0 and lse = -inf and contributes nothing to dq, dk, dv or the table gradient; a
 * masked key gets dk = dv = 0 and its K / V rows never reach an output.
 * Refused before any launch.  ALM_ERR_UNSUPPORTED: B, N, H < 1, H > 64, dim_head != 64, N rows of pitch ldq / ldk / ldv of 2^31 bytes or more, N + 64
 * rows of any pitch of 2^32 bytes or more (the tile DMA's 32-bit offsets would wrap).  ALM_ERR_BAD_ARG: N * lddo * 2 >= 2^31 (backward);
 * dropout_p outside [0, 1); a NULL q / k / v / o / lse (backward: also dout / dq / dk / dv / delta); ldq, lddo < H*64 or no multiple
 * of 8 (16-byte tile DMA and fragment loads), ldk, ldv < 64 or no multiple of 8 (the same), ldo, lddq < H*64 or no multiple of 4 (8-byte stores of o and
 * dq), lddk < 64, part_stride < B*N*lddk when alm_mqa_bwd_parts(B,N,H) > 1; q, k, v, dout not 16-byte aligned, dq not 8-byte aligned, o not 8-byte aligned
 * in the forward (the backward only READS o, with global loads that take any element-aligned address: its base is not checked there).
 * dk / dv / lse / delta are read and written one float at a time: they need no alignment beyond a float's, and lddk, part_stride need no multiple. */
int alm_mqa_attn_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, const unsigned char* mask,
                     void* o, long long ldo, float* lse, int B, int N, int H, int dim_head, float scale, float dropout_p,
                     unsigned long long seed, const void* seed_dev, void* stream);
int alm_mqa_attn_bwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, const unsigned char* mask,
                     const void* o, long long ldo, const float* lse, const void* dout, long long lddo, void* dq, long long lddq, float* dk,
                     float* dv, long long lddk, long long part_stride, float* delta, int B, int N, int H, int dim_head, float scale,
                     float dropout_p, unsigned long long seed, const void* seed_dev, void* stream);
/* number of head groups (4 heads each) of the forward / dQ kernels (the table-gradient partial rows of the bias variants count in these) */
int alm_mqa_head_groups(int H);
/* number of dk / dv partial sets alm_mqa_attn_bwd / alm_mqa_attn_bias_bwd WRITE for this shape (the dK/dV kernel runs 4 or 2 heads per workgroup: H / 4 or
 * H / 2 partials, part_stride floats apart): the caller allocates this many and hands them all to alm_kv_grad_pack(nparts) */
int alm_mqa_bwd_parts(int B, int N, int H);
/* The same attention with the STRUCTURED SCORE BIAS of the `flash_attn=False` models -- Attend.forward's `sim + attn_bias` (attend.py:118-
 * 121) with the bias tensors of RelativePositionBias (audiolm_pytorch.py:202-242), the Coarse cross-attention override (:924-936) and the
 * Fine (frame, quantizer) table (:1227-1298) -- without ever materialising the (h, n, n) tensor:
 *     bias(h, i, j) = (qattr[i] & kattr[j]) ? tbl[h][0] : tbl[h][(qkey4[i] - kkey4[j]) / 4]
 * tbl fp32 [H][LT] in raw-score units (bias / scale; slot 0 = cross_attn_bias / null_pos_bias); qkey4 / kkey4 / qattr / kattr int32 [N]
 * (16-byte aligned, shared by the batch; qkey4 - kkey4 is a BYTE offset into a table row, offsets outside [0, 4 LT) read 0).
 * Backward additionally accumulates d(loss)/d(tbl) into dtbl_part [alm_attn_bias_part_rows(B, N, H)][LT] (per-workgroup partial tables:
 * zero before the first layer, alm_attn_bias_grad_reduce after the last -- all layers of a stack share one table). */
int alm_mqa_attn_bias_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, const unsigned char* mask,
                          void* o, long long ldo, float* lse, int B, int N, int H, int dim_head, float scale, const float* tbl, int LT,
                          const int* qkey4, const int* kkey4, const int* qattr, const int* kattr, float dropout_p, unsigned long long seed,
                          const void* seed_dev, void* stream);
int alm_mqa_attn_bias_bwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, const unsigned char* mask,
                          const void* o, long long ldo, const float* lse, const void* dout, long long lddo, void* dq, long long lddq,
                          float* dk, float* dv, long long lddk, long long part_stride, float* delta, int B, int N, int H, int dim_head,
                          float scale, const float* tbl, int LT, const int* qkey4, const int* kkey4, const int* qattr, const int* kattr,
                          float* dtbl_part, float dropout_p, unsigned long long seed, const void* seed_dev, void* stream);
int alm_attn_bias_part_rows(int B, int N, int H);
int alm_attn_bias_grad_reduce(const float* dtbl_part, float* dtbl, int B, int N, int H, int LT, float scale, void* stream);
/* The small MLPs that produce `tbl` (RelativePositionBias.net audiolm_pytorch.py:214-221, FineTransformer.pos_bias_mlp :1065-1071): first
 * layer (in_dim 1 or 2 -> C) + SiLU, SiLU forward / backward for the C x C layers (which run on alm_gemm_*), last layer (C -> H) written
 * straight into the table layout [H][L + 1] (x inv_scale, slot 0 = special * inv_scale), and their backward passes. */
int alm_posmlp_in_fwd(const float* x, const float* W, const float* b, float* pre, void* act_bf16, int L, int in_dim, int C, void* stream);
int alm_posmlp_in_bwd_chunks(int L);
int alm_posmlp_in_bwd(const void* dpre_bf16, const float* x, float* partial, int L, int in_dim, int C, void* stream);
int alm_silu_fwd(const float* pre, void* act_bf16, long long n, void* stream);
int alm_silu_bwd(const float* dact, const float* pre, void* dpre_bf16, long long n, void* stream);
int alm_posmlp_out_fwd(const void* act_bf16, const float* W, const float* b, const float* special, float* tbl, int L, int C, int H,
                       float inv_scale, void* stream);
int alm_posmlp_out_bwd(const float* dtbl, const float* W, const float* pre, void* g_bf16, void* dpre_bf16, float* dspecial, int L, int C, int H,
                       int Hp, float inv_scale, void* stream);
/* ---- attention over a short, always-visible key set: the conditioning paths of Attention.forward (audiolm_pytorch.py:307-406) ----------------
 * cross-attention layers (Transformer(cross_attend=True), :450: keys = [null_kv | to_kv(context_norm(text embeds))], non-causal, :372-388) and
 * `cond_as_self_attn_prefix` (:330-345: the text embeds prepended to the causal self-attention keys).  The three small contractions
 * S_e = Q K_e^T [B][N*H][Me], O_e = P_e V_e, and their gradients run on alm_gemm_bf16_*; these entries are the row-wise softmax pieces.
 * Row r = (b*N + n)*H + h; statistics (lse, ndelta) use the flash kernels' [B][H][N] layout.
 *   softmax_fwd: P = exp(S*scale - lse_tot) on unmasked keys (emask uint8 [B][Me], NULL = all), lse_tot = logaddexp(lse_self, lse_e)
 *                (lse_self NULL: no causal self part), fself[r] = exp(lse_self - lse_tot): the weight of the self part's output.
 *   combine:     O[(b n)][h*dh + d] = fself[r] * O_self + O_e[r][d]        (O_self / fself NULL: cross-attention)
 *   softmax_bwd: dS = P o (dP + ndelta) * scale, ndelta[b][h][n] = -sum_d dO*O of the JOINT output (alm_xattn_delta, or the workspace
 *                alm_mqa_attn_bwd filled when a self part exists).
 * The same pieces serve the reference's MATH path with an arbitrary dense attn_bias (attend.py:98-146: sim = q k^T * scale + attn_bias, key mask,
 * causal triu(j - i + 1)): `bias` fp32 [H][N][ldbias] (NULL: none) is added to the scaled scores, `causal_off` makes key e visible to query n iff
 * e <= n + causal_off (Me - N for the reference's rule; 0x7fffffff: not causal); alm_xattn_dbias: dbias[h][n][e] = sum_b P o (dP + ndelta). */
int alm_xattn_softmax_fwd(const float* S, long long ldS, const unsigned char* emask, const float* lse_self, float scale, void* P_bf16, long long ldP,
                          float* lse_tot, float* fself, const float* bias, long long ldbias, int causal_off, int B, int N, int H, int Me, void* stream);
int alm_xattn_dbias(const void* P_bf16, long long ldP, const float* dP, long long lddP, const float* ndelta, float* dbias, long long lddb, int Me, int B,
                    int N, int H, void* stream);
int alm_xattn_combine(const void* o_self_bf16, long long ldos, const float* fself, const float* o_e, void* out_bf16, long long ldo, long long tokens,
                      int H, int dim_head, void* stream);
int alm_xattn_softmax_bwd(const void* P_bf16, long long ldP, const float* dP, long long lddP, const float* ndelta, float scale, void* dS_bf16,
                          long long lddS, int Me, int B, int N, int H, void* stream);
int alm_xattn_delta(const void* o_bf16, long long ldo, const void* dout_bf16, long long lddo, float* ndelta, int B, int N, int H, int dim_head,
                    void* stream);
/* value residual, audiolm_pytorch.py:353-358 / :534-535 */
int alm_value_residual_mix(const void* v, long long ldv, const void* v0, long long ldv0, void* out, long long ldo, long long rows,
                           int dim_head, void* stream);
/* dkv_bf16 [rows][ldo] = (sum of the nparts fp32 partial sets of dk | the same of dv) rounded once; mode 0: no value residual, 1: dv is halved and added to
 * acc_v0 [rows][dim_head], 2: acc_v0 is added to dv.  rows == 0 returns 0.  ALM_ERR_BAD_ARG before any launch: mode outside 0..2, mode != 0 without acc_v0,
 * nparts < 1, rows < 0, a NULL dk / dv / dkv_bf16, dim_head < 1, ld < dim_head, ldo < 2 dim_head, part_stride < rows * ld with nparts > 1.  Scalar accesses only. */
int alm_kv_grad_pack(const float* dk, const float* dv, long long ld, int nparts, long long part_stride, float* acc_v0, void* dkv_bf16,
                     long long ldo, long long rows, int dim_head, int mode, void* stream);

/* cross-entropy means + the wrappers' weighted combination (audiolm_pytorch.py:1561-1565, :1826-1854, :2112-2137: F.cross_entropy(..., ignore_index) per
 * head, then (loss_a * n_a * w + loss_b * n_b) / (n_a + n_b)) from the per-group loss SUMS: loss[0] = sum_g w_g * sum_g[0] / max(#(labels_g != ignore), 1);
 * scales[g] = w_g / max(count_g, 1) (the backward's factor).  G <= 4 groups; unused slots NULL / 0. */
int alm_loss_combine(const float* s0, const float* s1, const float* s2, const float* s3, const long long* l0, const long long* l1, const long long* l2,
                     const long long* l3, long long n0, long long n1, long long n2, long long n3, float w0, float w1, float w2, float w3, int G,
                     long long ignore_index, float* loss, float* scales, void* stream);

/* CoarseTransformerWrapper.forward's id bookkeeping of a training step, audiolm_pytorch.py:1785-1810 (append eos, key mask of pad / eos semantic keys,
 * their ids zeroed, mask padded over [start | semantic | coarse start | coarse]) + the embedding source codes of :894-918 (start tokens, semantic ids,
 * coarse rows id + (i mod Q) * codebook_size) + the label tensors (ids with the eos appended), in one launch.  N = ns0 + nc0 + 3.
 * sem_has_eos != 0: the semantic rows already are [ids | eos | pad ...] (alm_unique_consecutive_i64, unique_consecutive = True, :1794-1795): nothing is
 * appended to them, sem_labels is [B][ns0] and N = ns0 + nc0 + 2. */
int alm_coarse_prepare(const long long* sem, long long ld_sem, const long long* coarse, long long ld_coarse, int B, int ns0, int nc0, long long pad_id,
                       long long sem_eos, long long coarse_eos, int Q, int C, long long* sem_labels, long long* coarse_labels, int* src_a, void* keep,
                       int sem_has_eos, void* stream);
/* SemanticTransformerWrapper.forward's id bookkeeping of a training step, audiolm_pytorch.py:1536-1548 (`append_eos_id`, input ids = ids[:, :-1]) + the
 * embedding source codes of SemanticTransformer.forward :709-714 ([start token | ids]; a negative id is the zero vector, :176-181) in one launch.
 * sem int64 [B][n0]; labels int64 [B][n0 + 1] = [ids | eos]; src_a int32 [B][n0 + 1] = [start | ids]; num_rows = rows of the embedding table (< 2^24).
 * has_eos != 0: the rows already are [ids | eos | pad ...]: labels [B][n0] = the rows, src_a [B][n0] = [start | rows without their last column]. */
int alm_semantic_prepare(const long long* sem, long long ld_sem, int B, int n0, long long eos_id, long long num_rows, long long* labels, int* src_a,
                         int has_eos, void* stream);
/* batch_unique_consecutive, audiolm_pytorch.py:162-164 (per row torch.unique_consecutive, right-padded with `pad` to the longest row), as one launch:
 * out int64 [B][n + append_eos] holds every collapsed row followed by pad, lengths int32 [B] the kept ids per row -- the caller reads the lengths ONCE and
 * slices out[:, :max(lengths)] (the reference's host loop synchronises per row).  append_eos != 0: the rows are [ids | eos_id] (append_eos_id :155-160, which
 * the wrappers apply before the collapse, :1536-1539 / :1788-1795). */
int alm_unique_consecutive_i64(const long long* ids, long long ld, int B, int n, int append_eos, long long eos_id, long long pad, long long* out,
                               long long ld_out, int* lengths, void* stream);
/* FineTransformer.forward's id bookkeeping, audiolm_pytorch.py:1171-1223 (key mask of pad / eos coarse keys, their ids zeroed, mask padded over
 * [coarse start | coarse | fine start | fine], embedding source codes id + (i mod Q) * codebook_size per table) in one launch.  fine: the first nf ids of
 * each row (the training wrapper drops the last one, :2086).  src_a int32 [B][n + nf + 2], keep bool [B][n + nf + 2]. */
int alm_fine_prepare(const long long* coarse, long long ld_coarse, const long long* fine, long long ld_fine, int B, int n, int nf, long long pad_id,
                     long long eos_id, int Qc, int Qf, int C, int* src_a, void* keep, void* stream);

/* forgetful causal mask, audiolm_pytorch.py:82-89 (`rand[:, 0] = -max; mask = ~zeros.scatter(1, rand.topk(k).indices, 1)`): keep [B][N] bytes (torch.bool
 * storage) &= NOT(one of the `drop` largest scores of its row); column 0 is never dropped; equal scores at the threshold go in index order.
 * drop <= N - 1, N <= 16384. */
int alm_forgetful_mask(const float* score, long long ld_score, void* keep, long long ld_keep, int B, int N, int drop, void* stream);

/* ---- hyper-connection residual streams: third-party `hyper_connections` used at audiolm_pytorch.py:24, 446-454, 524, 551 ----
 * R [B][S][N][D], stored fp32 or (r_bf16) bf16 -- under trainer.py:1241's autocast the reference's streams are bf16 tensors; the arithmetic is
 * fp32 in registers either way.  Tensors standing for all streams at once (the `*_bcast` forms) are always fp32 [B*N][D].
 * coef: per-token fp32 record of alm_hc_coef_width(S) floats (alpha | beta | pre-activations | 1/norm). */
int alm_hc_coef_width(int S);
int alm_hc_partial_width(int S, int D);
int alm_hc_grads_width(int S, int D);
int alm_hc_partial_rows(int mode, int fused_ln, int r_bf16, int S, long long tokens, int D);
/* Which kernel variant a launch takes -- the host functions the launchers themselves call, no device needed.
 * alm_hc_fwd_prefetch: 1 = the software-prefetching forward kernel (bf16 streams, no rin_bcast, D == 256 * waves per token), 0 = the plain one.
 * alm_hc_bwd_variant : -1 = plain kernel, 0 / 1 / 2 = prefetching kernel with stream tensors everywhere / broadcast dRn / broadcast R, 3 = the LDS-DMA
 *   kernel (S 4, D 1024, bf16, mode 3, fused LayerNorm).  want_dR / want_dsum: dR / dsum != NULL; ld_max: the largest row stride among dx, dxn, extra,
 *   y_prev, dy; aligned16: dRn, R, dxn, extra, y_prev all start on 16-byte boundaries with row strides that are multiples of 8 elements, and coef_prev
 *   and dbeta are given.  Arguments alm_hc_bwd refuses give -1. */
int alm_hc_fwd_prefetch(int r_bf16, int rin_bcast, int D);
int alm_hc_bwd_variant(int mode, int fused_ln, int r_bf16, int S, int B, int N, int D, int dRn_bcast, int r_bcast, int want_dR, int want_dsum,
                       long long ld_max, int aligned16);
/* Both launchers return ALM_ERR_BAD_ARG before any launch for B < 1, N < 1, D < 4, a mode outside {1, 2, 3, 5} (forward) / {1, 2, 3} (backward) and for a
 * base pointer below the alignment of the kernels' vector accesses: 16 bytes for fp32 rows (fp32 / broadcast streams, xs_out, xn32_out, dsum, dx) and
 * ln_gamma, 8 bytes for bf16 rows (bf16 streams, y_prev, x_out, xn_out, dxn, extra, dy).
 * forward.  mode 1: depth connection only, R_out[t] = sum_s alpha[s][t+1] R_in[s] + beta[t] y_prev (coef_prev = that branch's record);
 * mode 2: width connection of a branch (its 7 parameters) + the branch's pre-LayerNorm: x, xn = LN(x) ln_gamma, mean, rstd, coef;
 * mode 3: mode 1 of the previous branch fused with mode 2 of the next one on the freshly computed residual (one pass over R);
 * mode 5: depth connection + stream sum (:551) + final LayerNorm (:555): xs_out fp32 [B*N][D], mean, rstd and the LayerNorm output either as
 *         xn_out bf16 or -- xn32_out != NULL -- as fp32 [B*N][D] (what the logit heads read).
 * rin_bcast: R_in is ONE fp32 [B*N][D] tensor that every stream equals (the state right after the stream expansion, :524). */
int alm_hc_fwd(const void* R_in, int rin_bcast, int r_bf16, const void* y_prev_bf16, long long ldy, const float* coef_prev, void* R_out,
               const float* hc_gamma, const float* Wa, const float* sa, const float* Aa, const float* wb, const float* sb, const float* Bb,
               const float* ln_gamma, void* x_out_bf16, long long ldx, void* xn_out_bf16, long long ldxn, float* xn32_out, float* mean,
               float* rstd, float* coef, float* xs_out, int mode, int B, int S, int N, int D, void* stream);
/* backward.  mode 2: width-connection backward (dR, parameter-gradient partial rows); mode 1: depth-connection backward
 * (dy = sum_t beta[t] dRn[t], dbeta_out[t] = <dRn[t], y>); mode 3: mode 2 of branch k+1 fused with mode 1 of branch k on the
 * freshly computed dR.  dRn_bcast: dRn is fp32 [B*N][D] and stands for all S streams (gradient of the final stream sum).
 * r_bcast: R is one fp32 [B*N][D] tensor for all streams (first branch); dsum (optional): fp32 [B*N][D] sum over streams of dR = the gradient of
 * the stream expansion (:524); dR may then be NULL.  r_bf16: dRn / R / dR (the non-bcast forms) hold bf16.
 * The gradient wrt the branch input comes either as dx (fp32 [B*N][lddx], already through the branch's LayerNorm backward) or -- fused
 * mode, dx == NULL -- as dxn (bf16, gradient wrt the LayerNorm OUTPUT) + optional extra (bf16, added to dx directly: the K/V path of
 * the attention branch) + the LayerNorm statistics / weight: the LayerNorm backward (audiolm_pytorch.py:191-198 autograd) then happens
 * inside this kernel and its weight gradient joins the outputs.
 * partial: [alm_hc_partial_rows(mode, dx == NULL, r_bf16, S, B*N, D)][alm_hc_partial_width(S, D)] floats -> alm_colsum_partial (`chunks` partial sums) -> alm_hc_param_grads(sums, chunks, ...), whose
 * output is dWa[D][S+1] | dwb[D] | dgamma[D] | dAa[S][S+1] | dBb[S] | dsa | dsb | dln[D]  (alm_hc_grads_width(S, D) floats). */
int alm_hc_bwd(const void* dRn, int dRn_bcast, int r_bf16, const float* dx, long long lddx, const void* dxn_bf16, long long lddxn,
               const void* extra_bf16, long long ldex, const float* mean, const float* rstd, const float* ln_gamma, const void* R, int r_bcast,
               const float* coef, const float* dbeta, const float* hc_gamma, const float* Wa, const float* sa, const float* wb, const float* sb,
               void* dR, float* dsum, float dsum_scale, float* partial, const void* y_prev_bf16, long long ldy, const float* coef_prev, void* dy_bf16, long long lddy,
               float* dbeta_out, int mode, int B, int S, int N, int D, void* stream);
int alm_hc_param_grads(const float* sums, int chunks, const float* hc_gamma, const float* Wa, const float* wb, float* out, int S, int D, void* stream);
/* the same finish for nb <= 16 width connections in two launches (column sums of every problem's partial rows, then the parameter gradients): the deferred
 * mode of the fused backward keeps the partial rows of all 12 branches of a 6-layer stack and finishes them together (24 small launches -> 2).  HOST pointer
 * arrays; ws: nb * 16 * alm_hc_partial_width(S, D) floats; outs[z]: alm_hc_grads_width(S, D) floats. */
int alm_hc_param_grads_batched(const float* const* parts, const int* rows, int nb, const float* const* gammas, const float* const* Was,
                               const float* const* wbs, float* ws, float* const* outs, int S, int D, void* stream);
int alm_streams_expand(const float* x, float* R, int B, int S, long long nd, void* stream);   /* :524 */
int alm_streams_reduce(const float* R, float* x, int B, int S, long long nd, void* stream);   /* :551 */
int alm_residual_add(const float* x, const void* y_bf16, long long ldy, float* out, long long rows, int D, void* stream);
int alm_f32_to_bf16(const float* a, const float* b_or_null, void* out_bf16, long long ldo, long long rows, int D, void* stream);
int alm_add_f32(const float* a, const float* b, float* out, long long n, float scale, void* stream);   /* out = (a + b) * scale */

/* ---- token-id side: embedding assembly (:709-713, :894-918, :1186-1223), logit-head regrouping (:965-983, :1325-1361),
 *      cross-entropy (:1561-1565, :1839-1849, :2122-2132) -------------------------------------------------------------------- */
/* source codes: (table << 24) | row, -1 = zero vector.  table_rows[t] = number of rows of table t: a code whose table or row is out of range
 * (nn.Embedding raises IndexError for it, audiolm_pytorch.py:709 / :901-906 / :1204-1213) reads as a zero vector, is skipped by the scatter, and
 * sets *err_flag (device int32, may be NULL) to 1 -- never an out-of-bounds access. */
int alm_embed_assemble(const float* const* tables, const int* table_rows, int ntables, const int* src_a, const int* src_b, float* out,
                       long long rows, int D, int* err_flag, void* stream);
int alm_embed_scatter_add(float* const* grad_tables, const int* table_rows, int ntables, const int* src_a, const int* src_b, const float* dout,
                          float alpha, long long rows, int D, void* stream);
/* the same scatter with ONE OWNER per destination row and fixed summation order: no atomics, bitwise run-to-run deterministic gradients (the
 * reference's embedding backward, aten::embedding_dense_backward under audiolm_pytorch.py:709 / :901-918, is not; SURVEY section 5 asks for
 * reproducible runs).  Every row of every table is WRITTEN (zero where no token maps to it): the gradient buffers need no clearing.
 * Skewed ids: destination rows with more than 128 tokens are listed by a histogram (integer atomics: exact) and summed by (row, token-range) workers whose
 * partials the row's last arriver adds in range order -- the sums stay a fixed function of the code arrays.  ALM_EMBED_SCATTER_HOT=0: owners only (A/B).
 * ws: alm_embed_scatter_ws_floats(...) floats (chunk partials of the few-row tables + hot-row partials + the listing's int workspace; the call zeroes what
 * it needs).  rows < 2^28, D % 4 == 0, ws 16-byte aligned. */
int alm_embed_scatter_ws_floats(const int* table_rows, int ntables, long long rows, int D);
int alm_embed_scatter_owned(float* const* grad_tables, const int* table_rows, int ntables, const int* src_a, const int* src_b, const float* dout,
                            float alpha, long long rows, int D, float* ws, void* stream);
int alm_gather_rows_bf16(const void* in, long long ld_in, const int* idx, void* out, long long ld_out, long long rows, int D, void* stream);
int alm_scatter_rows_bf16(const void* in, long long ld_in, const int* idx, void* out, long long ld_out, long long rows, int D, void* stream);
/* split-bf16 operands of the logit-head contraction (the heads read the fp32 final hidden states / fp32 master weights at ~16 mantissa bits:
 * x = hi + lo with hi = bf16(x), lo = bf16(x - hi); logits = hi.Whi + hi.Wlo + lo.Whi on the bf16 MFMA, fp32 accumulate):
 * hi[r] / lo[r] = split(in[idx ? idx[r] : r]) for r < rows_out; source rows < 0 or >= rows_in give zero rows (ragged head groups, row padding). */
int alm_gather_split_bf16(const float* in, long long ld_in, long long rows_in, const int* idx, void* hi, void* lo, long long ld_out,
                          long long rows_out, int D, void* stream);
/* rows <= 0 returns 0; otherwise ALM_ERR_BAD_ARG before any launch for a NULL pointer, C < 1, ld < C, Cpad < C, ldd < Cpad.  A label equal to
 * ignore_index, negative or >= C is ignored (loss 0, gradient row 0).  alm_reduce_sum: ALM_ERR_BAD_ARG for a NULL out, n < 0, or a NULL in with n > 0. */
int alm_cross_entropy_fwd(const float* logits, long long ld, const long long* labels, float* loss_rows, float* lse, long long rows, int C,
                          int ignore_index, void* stream);
int alm_cross_entropy_bwd(const float* logits, long long ld, const long long* labels, const float* lse, const float* gscale, void* dlogits_bf16,
                          long long ldd, long long rows, int C, int Cpad, int ignore_index, void* stream);
int alm_reduce_sum(const float* in, long long n, float* out, float scale, void* stream);

/* ---- autoregressive sampling: attention of ONE new position per sequence over a key / value cache (Attention.forward with kv_cache,
 * audiolm_pytorch.py:360-394, driven by the generate() loops :1476-1507, :1677-1706, :1965-1994).  cache bf16 [B][nmax][128] (k | v, v already
 * value-residual mixed); kv_new bf16 [B][ldkv] is appended at index `pos` by the call; keys 0 .. pos are attended (mask uint8 [B][ldm], 1 =
 * attend, or NULL).  Structured score bias as in alm_mqa_attn_bias_fwd: tbl [H][LT] + per-key kkey4 / kattr (device) and the new position's
 * qkey4 / qattr BY VALUE; tbl NULL = none.  pos_dev (device int32) non-NULL: the position is read from the device at run time and the
 * query-side values from qkey4_vec / qattr_vec [nmax] -- the launch a captured hipGraph replays for every sampling step. */
int alm_mqa_decode_attn(const void* q, long long ldq, void* cache, long long cache_stride, const void* kv_new, long long ldkv,
                        const unsigned char* mask, long long ldm, void* out, long long ldo, int B, int H, int dim_head, int pos, int nmax,
                        float scale, const float* tbl, int LT, int qkey4, int qattr, const int* kkey4, const int* kattr, const int* pos_dev,
                        const int* qkey4_vec, const int* qattr_vec, void* stream);

/* ---- fused optimiser step: global-norm clip (trainer.py:953-954 accelerator.clip_grad_norm_) + Adam / AdamW (optimizer.py:get_optimizer) over
 * every parameter in two kernels.  `tensors`: HOST array of `ntensors` AlmOptTensor (device pointers inside): it travels in the kernel arguments, 64
 * tensors per launch -- no staged host-to-device copy per step (the gradient storage moves every step, so the table cannot live on the device);
 * `chunks`: DEVICE int32 pairs (tensor index, chunk index), tensor-major, one per alm_opt_chunk_elems() elements of each tensor (shape-dependent: cached).  alm_opt_grad_sumsq writes one partial sum of squares per chunk (alm_reduce_sum over it =
 * the squared global gradient norm, kept on the device); alm_opt_adam_step applies coef = min(1, max_norm / (sqrt(*sumsq) + 1e-6)) to the
 * gradients on the fly (sumsq NULL: no clipping), then torch.optim.Adam's update (decoupled_weight_decay 1: AdamW).  All fp32.
 * Both entry points validate the WHOLE table before the first launch, so ALM_ERR_BAD_ARG means that no tensor has been touched: every n >= 0; where
 * n > 0 the pointers the entry point reads are non-NULL (alm_opt_adam_step: p, g, m, v; alm_opt_grad_sumsq: g only); nchunks equals the table's total
 * chunk count, sum of ceil(n / alm_opt_chunk_elems()); alm_opt_adam_step: step >= 1.  An entry with n = 0 may carry NULL pointers. */
typedef struct AlmOptTensor {
    void* p; const void* g; void* m; void* v;   /* parameter, gradient, exp_avg, exp_avg_sq */
    long long n;                                /* elements */
    float wd; int step;                         /* weight decay of this tensor; its own 1-based step count of THIS update (bias corrections), 0: the launch's `step` */
} AlmOptTensor;
int alm_opt_chunk_elems(void);
int alm_opt_grad_sumsq(const AlmOptTensor* tensors, int ntensors, const int* chunks, int nchunks, float* partial, void* stream);
int alm_opt_adam_step(const AlmOptTensor* tensors, int ntensors, const int* chunks, int nchunks, float lr, float beta1, float beta2, float eps, int step,
                      int decoupled_weight_decay, const float* sumsq, float max_norm, void* stream);

/* The same update for the dense GEMM weights, fused with their bf16 re-pack (round 4): walks each weight matrix in alm_pack_weights_multi's tiles and
 * writes the new fp32 parameter, both moments and both packed images (dst / dstT as in AlmPackJob) -- the forward after an optimiser step then finds its
 * packed copies current (core.layer_weights) instead of re-reading every master weight.  `jobs`: HOST array.  Bit-identical to alm_opt_adam_step
 * followed by alm_pack_weights_multi.  Needs even leading dimensions / paddings and 8-byte (fp32) / 4-byte (bf16) aligned bases: ALM_ERR_BAD_ARG otherwise. */
typedef struct AlmOptPackJob {
    void* p; const void* g; void* m; void* v;   /* fp32 [rows][cols] views, row stride ld: parameter, gradient, exp_avg, exp_avg_sq */
    int rows, cols; long long ld;
    void* dst; long long ld_dst; int rows_pad, cols_pad;
    void* dstT; long long ld_dstT;
    float wd; int step;                         /* as AlmOptTensor */
} AlmOptPackJob;
int alm_opt_adam_pack_step(const AlmOptPackJob* jobs, int njobs, float lr, float beta1, float beta2, float eps, int step, int decoupled_weight_decay,
                           const float* sumsq, float max_norm, void* stream);

/* ---- SoundStream tokenize path (encode only): soundstream.py:332-345, 362-380, 519-531 (causal conv encoder), :592-607 / :840 ----
 * (eval-mode GroupedResidualVQ of vector-quantize-pytorch, restated in oracle/rvq_restated.py).  All fp32: the code indices are an
 * argmin over float distances, so both kernels run on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), never bf16.
 * conv: x [B][Cin][Tin] -> out [B][Cout][Tout], Tout = (Tin - stride) / stride + 1; left reflect pad dilation*(ksize-1) + 1 - stride;
 *       out = act(conv + bias) (+ residual), act = ELU when `elu`.  wp = weights packed once by alm_conv1d_pack. */
int alm_conv1d_packed_floats(int Cout, int Cin, int ksize);
int alm_conv1d_pack(const float* w, float* wp, int Cout, int Cin, int ksize, void* stream);
int alm_conv1d_causal(const float* x, const float* wp, const float* bias, const float* residual, float* out, int B, int Cin, int Cout, int Tin,
                      int ksize, int stride, int dilation, int elu, int zero_pad, void* stream);
/* one ResidualUnit (soundstream.py:362-369: x + ELU(conv_k1(ELU(conv_k,dilation(x)))), CausalConv1d reflect left pad, stride 1) in ONE launch; the
 * intermediate stays in registers.  w7p / w1p: alm_conv1d_pack images of the two conv weights; x, out fp32 [B][C][T].  C % 32 == 0 and C <= 256, else
 * ALM_ERR_UNSUPPORTED (run the two alm_conv1d_causal launches).  Bitwise equal to those two launches (same fma chains on the exact-fp32 matrix core). */
int alm_resunit_causal(const float* x, const float* w7p, const float* b7, const float* w1p, const float* b1, float* out, int B, int C, int T,
                       int ksize, int dilation, void* stream);
/* decoder side (soundstream.py:347-360, 382-395, 615-627, 691-709).  zero_pad = 1 above pads with zeros instead of reflecting: a
 * CausalConvTranspose1d(k = 2 s, stride s) is that conv with k = 2 over s * Cout phase-major output channels (weights re-indexed on the host),
 * followed by alm_phase_interleave: y [B][s * Cout][n] -> out [B][Cout][n * s].  alm_rvq_decode: codes -> summed code vectors. */
int alm_phase_interleave(const float* y, float* out, int B, int Cout, int s, int n, void* stream);
int alm_rvq_decode(const long long* idx, long long ldi, const float* E, float* out, long long ldo, int T, int d, int C, int Q, void* stream);
/* rvq: frames x [T][ldx] (d columns of one group), codebooks E [Q][C][d]; Et [Q][alm_rvq_padded_dim(d)][CP] floats (MFMA-ordered image)
 * / e2 [Q][CP] packed once by alm_rvq_pack (CP = alm_rvq_padded_codes(C)); idx int64 [T][ldi] (Q columns): per quantizer argmin_e sqrt(clamp(|r|^2 + |e|^2 - 2 r.e, 0)) with
 * first-index tie-breaking, r -= E[idx]; quant (optional) = sum of the selected code vectors. */
int alm_rvq_padded_codes(int C);
int alm_rvq_padded_dim(int d);
int alm_rvq_pack(const float* E, float* Et, float* e2, int Q, int C, int d, void* stream);
int alm_rvq_encode(const float* x, long long ldx, const float* E, const float* Et, const float* e2, long long* idx, long long ldi, float* quant,
                   long long ldq, int T, int d, int C, int Q, void* stream);
int alm_bct_to_btc(const float* in, float* out, int B, int C, int T, void* stream);   /* 'b c n -> b n c', soundstream.py:823 */
/* ---- train-mode residual VQ (csrc/rvq_train.hip; soundstream.py:592-607: EMA codebooks, commitment loss, rotation trick, dead-code expiry, k-means
 * init; restated in tests/rvq_train_restated.py).  fp32, no float atomics: every output is bitwise reproducible.  The assignment stays on alm_rvq_encode
 * (one quantizer per call on the current residual).  Rows r / x / out / g_out / dx are [M][ld*] column views of one group (d columns), idx an int64
 * column ([M] with stride ldi; -1 or a value outside [0, C) = the row takes no part), E one layer's [C][d] or all layers' [Q][C][d] codebooks.
 *   alm_rvq_code_stats     : n [C] = rows per code (as floats), s [C][d] = their sums: stable counting sort of the rows by code, then a code's rows
 *                            are added in ascending row order in chunks of alm_rvq_code_stats_chunk() rows, the chunks' partials in chunk order; codes
 *                            without rows get n = 0, s = 0.  ws: alm_rvq_code_stats_ws_floats(M, d, C) 4-byte words (-1: too large).  C <= 8192.
 *   alm_rvq_train_quantize : one layer, in place: quant = E[idx]; y = rotate_to(r, quant) (rotation) or r + (quant - r); resid -= y; out += y;
 *                            loss[0] = loss_scale * sum over rows of |quant - r|^2, reduced in a fixed order through part
 *                            (alm_rvq_train_quantize_blocks(M) floats).  d <= 1024, else ALM_ERR_UNSUPPORTED (also _expire / _bwd).
 *   alm_rvq_ema_update     : cluster_size = cluster_size * decay + n * (1 - decay); embed_avg likewise from s; embed = embed_avg / smoothed with
 *                            smoothed = (cluster_size + eps) / (sum + C eps) * sum, the sum over C in a fixed order (total: one float of workspace).
 *                            dead int [1 + C]: the number of codes with cluster_size < threshold after the update, then those codes, ascending.
 *   alm_rvq_expire         : for i < count: code dead[i] gets embed = the layer-q residual of row rows[i] (recomputed from x, the saved idx [M][ldi]
 *                            and the pre-update codebooks E [Q][C][d]), embed_avg = threshold * that row, cluster_size = threshold.
 *   alm_rvq_kmeans_update  : means = n == 0 ? means : s / max(n, 1); with embed != NULL also embed = means, embed_avg = means * n, cluster_size = n.
 *   alm_rvq_train_bwd      : dx = sum over the layers of (dy / dr)^T g_out + coef[q] (r_q - quant_q), every row's chain recomputed from x, idx
 *                            [M][ldi] (Q columns) and the pre-update codebooks E [Q][C][d] with the forward's own arithmetic.  g_out / coef may be NULL. */
int alm_rvq_code_stats_chunk(void);
int alm_rvq_code_stats_ws_floats(int M, int d, int C);
int alm_rvq_code_stats(const float* r, long long ldr, const long long* idx, long long ldi, float* n, float* s, float* ws, long long ws_floats, int M, int d,
                       int C, void* stream);
int alm_rvq_train_quantize_blocks(int M);
int alm_rvq_train_quantize(float* resid, long long ldr, const long long* idx, long long ldi, const float* E, float* out, long long ldo, float* loss,
                           float* part, float loss_scale, int rotation, int M, int d, int C, void* stream);
int alm_rvq_ema_update(float* cluster_size, float* embed_avg, float* embed, const float* n, const float* s, float decay, float eps, float threshold,
                       int* dead, float* total, int C, int d, void* stream);
int alm_rvq_expire(const int* dead, int count, const long long* rows, const float* x, long long ldx, const long long* idx, long long ldi, const float* E,
                   int q, int rotation, float threshold, float* cluster_size, float* embed_avg, float* embed, int M, int d, int C, void* stream);
int alm_rvq_kmeans_update(float* means, const float* n, const float* s, float* embed, float* embed_avg, float* cluster_size, int C, int d, void* stream);
int alm_rvq_train_bwd(const float* x, long long ldx, const long long* idx, long long ldi, const float* E, const float* g_out, long long ldg,
                      const float* coef, float* dx, long long lddx, int rotation, int M, int d, int C, int Q, void* stream);
/* backward of the codec's conv stacks (csrc/codec_bwd.hip), exact fp32 on the matrix core, no float atomics (bitwise reproducible).  g = dL/dout
 * [B][Cout][Tout]; y = the saved post-ELU output of the conv (same shape) or NULL: g is read as g * (y > 0 ? 1 : y + 1) (ELU backward fused into
 * the load).  Shapes, pad and zero_pad as in alm_conv1d_causal.
 *   alm_conv1d_dgrad : dx [B][Cin][Tin] = the input gradient incl. the reflect fold (+ residual [B][Cin][Tin] if given).  wt = alm_conv1d_pack
 *                      image of the TRANSPOSED weight [Cin][Cout][k] (alm_conv1d_packed_floats(Cin, Cout, k) floats).
 *   alm_conv1d_wgrad : dw [Cout][Cin][k], db [Cout] from x [B][Cin][Tin]: one partial per time chunk (alm_conv1d_wgrad_chunk(B, Tout) steps) and
 *                      32 x 32 channel tile into ws, then summed in chunk order.  ws: alm_conv1d_wgrad_ws_floats floats, owned by the caller.
 *   alm_phase_deinterleave : adjoint of alm_phase_interleave, g [B][Cout][n * s] -> y [B][s * Cout][n].
 * The adjoint of alm_bct_to_btc is alm_bct_to_btc with C and T exchanged. */
int alm_conv1d_wgrad_chunk(int B, int Tout);
int alm_conv1d_wgrad_ws_floats(int B, int Cin, int Cout, int Tout, int ksize);
int alm_conv1d_dgrad(const float* g, const float* y, const float* wt, const float* residual, float* dx, int B, int Cin, int Cout, int Tin, int ksize,
                     int stride, int dilation, int zero_pad, void* stream);
int alm_conv1d_wgrad(const float* g, const float* y, const float* x, float* dw, float* db, float* ws, long long ws_floats, int B, int Cin, int Cout,
                     int Tin, int ksize, int stride, int dilation, int zero_pad, void* stream);
int alm_phase_deinterleave(const float* g, float* y, int B, int Cout, int s, int n, void* stream);
/* input resampling (soundstream.py:779-795: process_input calls torchaudio.functional.resample(x, input_sample_hz, target_sample_hz); torchaudio's
 * windowed-sinc polyphase resampler, third-party, restated in audiolm-pytorch_amd/resample.py), fp32.  o / n = orig / new rate over their gcd,
 * table [n][taps] = the sinc kernel (taps = 2 W + o, built on the host), rows of len_in samples x [rows][ld_x] -> len_out = ceil(n len_in / o)
 * samples y [rows][ld_y]:  y[j n + p] = sum_k table[p][k] x[j o + k - W]  (x = 0 outside [0, len_in)).
 * _bwd is the adjoint with the same geometry: dy [rows][ld_dy] (len_out) -> dx [rows][ld_dx] (len_in), dx[i] = sum over the (j, p) with
 * j n + p < len_out and 0 <= i + W - j o < taps of table[p][i + W - j o] dy[j n + p] (a gather: no atomics, bitwise deterministic).
 * Lengths and strides are 64-bit.  ALM_ERR_BAD_ARG when len_out != ceil(n len_in / o), taps != 2 W + o or a size is negative;
 * ALM_ERR_UNSUPPORTED when one 8-frame input window exceeds the LDS (o in the tens of thousands). */
int alm_resample_sinc(const float* x, long long ld_x, float* y, long long ld_y, const float* table, int taps, long long rows, long long len_in,
                      long long len_out, int o, int n, int W, void* stream);
int alm_resample_sinc_bwd(const float* dy, long long ld_dy, float* dx, long long ld_dx, const float* table, int taps, long long rows,
                          long long len_in, long long len_out, int o, int n, int W, void* stream);
/* ---- HubertWithKmeans (hubert_kmeans.py:37-121): the fairseq HuBERT-base feature model (fairseq models/hubert/hubert.py HubertModel.forward
 * with features_only, models/wav2vec/wav2vec2.py ConvFeatureExtractionModel / TransformerEncoder / TransformerSentenceEncoderLayer, third-party,
 * restated in tests/hubert_restated.py) and the k-means assignment (hubert_kmeans.py:114-116).  fp32 on the exact-fp32 matrix core, [B][C][T].
 * conv0 (wav2vec2.py ConvFeatureExtractionModel, mode 'default': conv(1 -> C, ksize, stride, no bias) + GroupNorm(C, C) + GELU): wave [B][ld_wave]
 *   (Tin samples per row) -> Tout = (Tin - ksize) / stride + 1.  _stats takes the per-(row, channel) mean / rstd over time without storing the
 *   activation: part [B][C][alm_hubert_conv0_chunks(Tout)][2] floats of workspace, stats [B][C][2] = (mean, rstd), biased variance, shifted sums
 *   per chunk merged in chunk order (deterministic, no atomics).  _apply recomputes the conv and writes gelu((c - mean) rstd gamma + beta) to
 *   out [B][C][Tout].  ksize <= 16, else ALM_ERR_UNSUPPORTED.  Lengths and row offsets are 64-bit. */
int alm_hubert_conv0_chunks(long long Tout);
int alm_hubert_conv0_stats(const float* wave, long long ld_wave, const float* w, float* part, float* stats, int B, int C, long long Tin,
                           long long Tout, int ksize, int stride, float eps, void* stream);
int alm_hubert_conv0_apply(const float* wave, long long ld_wave, const float* w, const float* stats, const float* gamma, const float* beta,
                           float* out, int B, int C, long long Tin, long long Tout, int ksize, int stride, void* stream);
/* csrc/dense_f32.hip, shared with the T5 encoder and EnCodec's LSTM projection.
 * conv1d with symmetric zero padding `pad` and `groups` (wav2vec2.py conv layers 1..6: pad 0, GELU; TransformerEncoder.pos_conv + SamePad + GELU
 * + the residual add of extract_features: groups 16, k 128, pad 64, Tout = Tin; the nn.Linear layers: k 1): x [B][Cin][Tin], w [Cout][Cin / groups]
 * [ksize] (torch's layout, unpacked), out [B][Cout][Tout] = (gelu ? erf-GELU : id)(conv + bias) + residual; bias / residual may be NULL.
 * Tout <= (Tin + 2 pad - ksize) / stride + 1 (a smaller Tout drops trailing outputs), else ALM_ERR_BAD_ARG.  Batch and channel-row offsets are
 * 64-bit; in-row indices are 32-bit, ALM_ERR_UNSUPPORTED when (Tout + 64) stride + ksize or (Cin / groups) ksize reaches 2^31. */
int alm_conv1d_valid(const float* x, const float* w, const float* bias, const float* residual, float* out, int B, int Cin, int Cout, int Tin,
                     int Tout, int ksize, int stride, int pad, int groups, int gelu, void* stream);
/* nn.LayerNorm over the channel axis of [B][C][T] (wav2vec2.py: layer_norm, encoder.layer_norm, self_attn_layer_norm, final_layer_norm), the
 * arguments of alm_layernorm_bct; 32 channel slices per time step and a two-pass variance, for sequences too short to fill the chip one thread per t. */
int alm_layernorm_bct_split(const float* x, const float* gamma, const float* beta, float* out, int B, int C, int T, float eps, void* stream);
/* csrc/dense_f32.hip.  fairseq MultiheadAttention (self-attention, no mask, eval):
 * qkv [B][3 H dim_head][T] (q | k | v channel blocks) -> out [B][H dim_head][T] =
 * softmax((scale q) . k) v per head, flash style (online softmax, no score matrix in memory).  dim_head == 64, else ALM_ERR_UNSUPPORTED. */
int alm_mha_attn_fwd(const float* qkv, float* out, int B, int H, int T, int dim_head, float scale, void* stream);

/* ---- FairseqVQWav2Vec (vq_wav2vec.py:19-81; csrc/vq_wav2vec.hip): fairseq's Wav2VecModel with the k-means quantizer (models/wav2vec/wav2vec.py
 * ConvFeatureExtractionModel + KmeansVectorQuantizer, third-party, restated in tests/vq_wav2vec_restated.py).  fp32, [B][C][T]; the convs are
 * alm_conv1d_valid, the code search alm_rvq_encode.  No atomics: every result is bitwise reproducible.
 * _group_stats: nn.GroupNorm(G, C) statistics of x [B][C][T]: stats [B][G][2] = (mean, rstd) over each sample's contiguous (C / G) x T block, biased
 *   variance; part [B][G][alm_vqw2v_group_chunks(C, T, G)][2] floats of workspace: (mean, M2) per chunk of 4096 elements, centred sums (never
 *   E[x^2] - E[x]^2), merged by Chan's update in fp64 in a fixed order.
 * _group_apply: in place, x = gamma[c] (x - mean) rstd + beta[c]; relu: max(., 0); residual [B][C][r_T] (or NULL): x = (x + residual[t * rstep])
 *   * scale, needs (T - 1) rstep < r_T; logc: x = log(|x| + 1).  In that order (ConvFeatureExtractionModel.forward).
 * _group_apply_t: out [B][T][C] = gamma (x - mean) rstd + beta, the transposed store the per-group code search reads with row stride C.
 * _conv0_stats / _conv0_apply: layer 0 (Cin = 1) without storing the un-normalised activation, the arguments of alm_hubert_conv0_* with
 *   GroupNorm(1, C): part [B][C][alm_hubert_conv0_chunks(Tout)][2] (the same partials), stats [B][2], out = relu(.) (logc: log(. + 1) after it).
 * ALM_ERR_BAD_ARG when G does not divide C; ALM_ERR_UNSUPPORTED when C T (and with it an in-group index) does not fit 32 bits or B G > 65535;
 * alm_vqw2v_group_chunks returns -1 for such a shape.  Sample and group offsets are 64-bit. */
int alm_vqw2v_group_chunks(int C, int T, int G);
int alm_vqw2v_group_stats(const float* x, float* part, float* stats, int B, int C, int T, int G, float eps, void* stream);
int alm_vqw2v_group_apply(float* x, const float* stats, const float* gamma, const float* beta, const float* residual, int B, int C, int T, int G,
                          int r_T, int rstep, float scale, int relu, int logc, void* stream);
int alm_vqw2v_group_apply_t(const float* x, const float* stats, const float* gamma, const float* beta, float* out, int B, int C, int T, int G,
                            void* stream);
int alm_vqw2v_conv0_stats(const float* wave, long long ld_wave, const float* w, float* part, float* stats, int B, int C, long long Tin,
                          long long Tout, int ksize, int stride, float eps, void* stream);
int alm_vqw2v_conv0_apply(const float* wave, long long ld_wave, const float* w, const float* stats, const float* gamma, const float* beta,
                          float* out, int B, int C, long long Tin, long long Tout, int ksize, int stride, int logc, void* stream);

/* ---- T5 text encoder (csrc/t5.hip; _attn_fwd: csrc/dense_f32.hip): transformers T5Stack (encoder) as the reference's t5.py:68-110 calls it,
 * restated in tests/t5_restated.py.
 * fp32, inference only.  Activations are [C][N], N = B T columns (sample b = columns b T .. b T + T - 1); the bias-less Linear layers are
 * alm_conv1d_valid with B = 1, ksize = 1, Tin = N.
 * _embed: ids int64 [N] -> out [D][N] = table[ids[n]][c], table [vocab][D].  An id outside [0, vocab) is not dereferenced: zero column and
 *   *err_flag = 1 (err_flag may be NULL).
 * _rmsnorm: T5LayerNorm, out = w x rsqrt(mean_c(x^2) + eps) (no mean subtraction, no bias), fixed summation order.  mask uint8 [N] or NULL:
 *   columns with mask 0 are written as exact 0.0.  transpose_out: out is [N][C] row-major instead of [C][N].  out must not alias x.
 * _gate: gated: x [2 F][N] -> out [F][N] = gelu_new(x[f]) x[F + f] (tanh form of GELU); else x [F][N] -> relu(x).
 * _attn_fwd: qkv [3 H 64][N] (q | k | v channel blocks, q unscaled) -> out [H 64][N] = softmax_j(q_i . k_j + bias[h][j - i + T - 1]) v_j over the
 *   keys j of the same sample with mask[b][j] != 0; bias [H][2 T - 1], mask uint8 [B][T] or NULL.  A masked key has probability exactly 0; a
 *   sample with every key masked gives zeros.  dim_head == 64 and T <= 2048, else ALM_ERR_UNSUPPORTED. */
int alm_t5_embed(const long long* ids, const float* table, float* out, int N, int D, long long vocab, int* err_flag, void* stream);
int alm_t5_rmsnorm(const float* x, const float* w, const unsigned char* mask, float* out, int C, int N, float eps, int transpose_out, void* stream);
int alm_t5_gate(const float* x, float* out, long long F, long long N, int gated, void* stream);
int alm_t5_attn_fwd(const float* qkv, const float* bias, const unsigned char* mask, float* out, int B, int H, int T, int dim_head, void* stream);
/* SoundStream LocalTransformer (soundstream.py:397-440 = local-attention's LocalMHA + FeedForward; third-party, restated), fp32, in the codec's
 * [B][C][T] layout; the Linear layers are k = 1 alm_conv1d_causal calls.
 *   alm_layernorm_bct : nn.LayerNorm over the channel axis (weight gamma, bias beta)
 *   alm_geglu_bct     : out[b][i][t] = x[b][i][t] * gelu(x[b][I + i][t])                          (x [B][2 I][T])
 *   alm_local_attn    : qkv [B][3 H dh][T] (q | k | v channel blocks) -> out [B][H dh][T]: l2-normalised q / k times q_scale / k_scale [dh]
 *                       (qk_rmsnorm) and `scale`, rotary + xpos from the slot tables cos_t / sin_t / xpos_t [2 window][dh] (slot s of the
 *                       (look-back | own) window pair; queries sit in slots window .. 2 window - 1), key j visible to query i iff
 *                       0 <= i - j <= window, softmax, values, times sigmoid(gates [B][H][T]) (gates may be NULL).  dh in {32, 64}, window <= 256. */
int alm_layernorm_bct(const float* x, const float* gamma, const float* beta, float* out, int B, int C, int T, float eps, void* stream);
int alm_geglu_bct(const float* x, float* out, int B, int I, int T, void* stream);
int alm_local_attn(const float* qkv, const float* q_scale, const float* k_scale, const float* cos_t, const float* sin_t, const float* xpos_t,
                   const float* gates, float* out, int B, int H, int dim_head, int T, int window, float scale, void* stream);
/* backward of the three (csrc/local_attn_bwd.hip), exact fp32, no atomics: every sum has a fixed order (bitwise reproducible).
 *   alm_local_attn_bwd : from qkv, the scales, the slot tables, gates (required), o = the saved GATED output of alm_local_attn and dO = dL/do:
 *                       dqkv [B][3 H dh][T], dgates [B][H][T] (pre-sigmoid), dq_scale / dk_scale [dh].  Three launches: the dQ pass (one thread per
 *                       query; also dgates, and lse / delta into ws), the dK/dV pass (one thread per key over the queries j .. j + window that see
 *                       it) and the finish of the scale gradients, which adds one partial per (b, h, window) in that order.
 *                       ws: alm_local_attn_bwd_ws_floats = 2 B H T + 2 B H ceil(T / window) dh floats, owned by the caller (-1: past 2^31).
 *                       alm_local_attn_bwd_supported(dh, window) = 1 iff dh in {32, 64}, window <= 256 and 4 dh window floats of LDS fit 160 KiB
 *                       (dh 64: window <= 160) -- exactly what alm_local_attn accepts; anything else is ALM_ERR_UNSUPPORTED.
 *   alm_layernorm_bct_bwd : dx [B][C][T] (+ residual [B][C][T] if given) from dy and the forward INPUT x (mean / rstd are recomputed, and kept in
 *                       ws [2][B][T] = alm_layernorm_bct_bwd_ws_floats floats for the second launch); dgamma / dbeta [C] (both or neither) as one
 *                       workgroup per channel, thread-strided sums and a fixed tree.
 *   alm_geglu_bct_bwd : du [B][2 I][T] from dh [B][I][T] and the saved pre-activation u [B][2 I][T] (erf GELU and its exact derivative). */
int alm_local_attn_bwd_supported(int dim_head, int window);
int alm_local_attn_bwd_ws_floats(int B, int H, int dim_head, int T, int window);
int alm_local_attn_bwd(const float* qkv, const float* q_scale, const float* k_scale, const float* cos_t, const float* sin_t, const float* xpos_t,
                       const float* gates, const float* o, const float* dO, float* dqkv, float* dgates, float* dq_scale, float* dk_scale, float* ws,
                       long long ws_floats, int B, int H, int dim_head, int T, int window, float scale, void* stream);
int alm_layernorm_bct_bwd_ws_floats(int B, int T);
int alm_layernorm_bct_bwd(const float* dy, const float* x, const float* gamma, const float* residual, float* dx, float* dgamma, float* dbeta,
                          float* ws, int B, int C, int T, float eps, void* stream);
int alm_geglu_bct_bwd(const float* dh, const float* u, float* du, int B, int I, int T, void* stream);

/* ---- EnCodec 24 kHz (csrc/encodec.hip): the causal SEANet encoder / decoder and LSTM that the reference's encodec.py:25-177 runs through Meta's model,
 * restated in tests/encodec_restated.py.  fp32.  The residual VQ is alm_rvq_pack / alm_rvq_encode / alm_rvq_decode above.
 * alm_conv1d_causal_pre = alm_conv1d_causal with `pre_elu`: out = act(bias + conv(pre_elu ? ELU(x) : x)) (+ residual) -- SEANet applies ELU before each conv.
 * alm_lstm_seq: nn.LSTM(H, H, L), gate order i f g o, zero initial state, one launch per time step issued from this one call (alm_lstm_launches(T, L) =
 * T + L - 1 launches: launch t advances layer l to time t - l; no workgroup waits for another one).  xproj [T][B][4H] = W_ih_l0 x_t without bias,
 * w_ih / w_hh [L][4H][H] (w_ih's layer-0 slice is not read), bias [L][4H] = b_ih + b_hh, hseq [L][T][B][H] (every layer's outputs), c [L][B][H] scratch;
 * optional skip [T][B][H] and out [B][H][T] = the last layer's h (+ skip).  H <= 1024, else ALM_ERR_UNSUPPORTED. */
int alm_conv1d_causal_pre(const float* x, const float* wp, const float* bias, const float* residual, float* out, int B, int Cin, int Cout, int Tin,
                          int ksize, int stride, int dilation, int pre_elu, int elu, int zero_pad, void* stream);
int alm_lstm_launches(int T, int L);
int alm_lstm_seq(const float* xproj, const float* w_ih, const float* w_hh, const float* bias, float* hseq, float* c, const float* skip, float* out,
                 int T, int B, int H, int L, void* stream);

/* ---- wave discriminators of SoundStream training (csrc/discr.hip), fp32, no atomics ---------------------------------------------------------------
 * Grouped strided zero-padded conv1d, y = act(conv1d(x, w, bias, stride, padding, groups)) with act 0 = identity, 1 = LeakyReLU(0.1)
 * (reference soundstream.py:92-140).  x [B][Cin][Tin], w [Cout][Cin / groups][k] (nn.Conv1d's layout, read as it is), y [B][Cout][Tout],
 * Tout = alm_gconv1d_out_len = (Tin + 2 padding - k) / stride + 1 (-1 when the padded input is shorter than the kernel).
 *   alm_gconv1d_dgrad : dx [B][Cin][Tin] from g = dL/dy; y = the saved OUTPUT of an act = 1 layer (g is multiplied by 1 where y > 0, else 0.1) or null.
 *   alm_gconv1d_wgrad : dw [Cout][Cin / groups][k], db [Cout]; partial sums per split of the (batch, 64-step chunk) list into ws
 *                       (alm_gconv1d_wgrad_ws_floats floats, caller-owned; -1: outside the kernel's envelope), then added in split order.
 * alm_avgpool1d_* : AvgPool1d(2 f, stride f, padding f), count_include_pad; x [rows][T] -> y [rows][T / f + 1] (alm_avgpool1d_out_len) and its adjoint.
 * alm_loss_mean_fwd : out[0] = mean of the mode's term over n elements, summed in a fixed order (ws: alm_loss_ws_floats floats):
 *     ALM_LOSS_HINGE_DISCR relu(1 + a) + relu(1 - b) (a = fake, b = real logits), ALM_LOSS_HINGE_GEN -a (b unused), ALM_LOSS_L1 |a - b|, ALM_LOSS_MSE (a - b)^2,
 *     ALM_LOSS_L1_COMPLEX the modulus |a - b| of interleaved (re, im) pairs with n counted in complex elements (F.l1_loss on complex tensors).
 * alm_loss_mean_bwd : da, db (either may be null) = gout[0] / n * d term / d a, d b; gout is read from device memory. */
#define ALM_LOSS_HINGE_DISCR 0
#define ALM_LOSS_HINGE_GEN 1
#define ALM_LOSS_L1 2
#define ALM_LOSS_MSE 3
#define ALM_LOSS_L1_COMPLEX 4
int alm_gconv1d_out_len(int Tin, int ksize, int stride, int padding);
int alm_gconv1d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int Tin, int ksize, int stride, int padding,
                    int groups, int act, void* stream);
int alm_gconv1d_dgrad(const float* g, const float* y, const float* w, float* dx, int B, int Cin, int Cout, int Tin, int ksize, int stride, int padding,
                      int groups, void* stream);
/* out [B][Cout][Tout] = m(y) conv1d(v, w) without a bias, m(y) = 1 where the saved output y > 0 and 0.1 elsewhere (y null: no mask): the derivative of
 * alm_gconv1d_dgrad(g, y, w) with respect to g applied to v [B][Cin][Tin] (double backward of the gradient penalty); the tiling of alm_gconv1d_fwd. */
int alm_gconv1d_fwd_masked(const float* v, const float* w, const float* y, float* out, int B, int Cin, int Cout, int Tin, int ksize, int stride,
                           int padding, int groups, void* stream);
int alm_gconv1d_wgrad_ws_floats(int B, int Cin, int Cout, int Tin, int ksize, int stride, int padding, int groups);
int alm_gconv1d_wgrad(const float* g, const float* y, const float* x, float* dw, float* db, float* ws, long long ws_floats, int B, int Cin, int Cout,
                      int Tin, int ksize, int stride, int padding, int groups, void* stream);
int alm_avgpool1d_out_len(int T, int f);
int alm_avgpool1d_fwd(const float* x, float* y, long long rows, int T, int f, void* stream);
int alm_avgpool1d_bwd(const float* g, float* dx, long long rows, int T, int f, void* stream);
int alm_loss_ws_floats(void);
int alm_loss_mean_fwd(const float* a, const float* b, float* out, float* ws, long long n, int mode, void* stream);
int alm_loss_mean_bwd(const float* a, const float* b, const float* gout, float* da, float* db, long long n, int mode, void* stream);
/* gradient penalty (soundstream.py:70-83) of G [R][n]: out[0] = weight / R sum_r (|G_r| - center)^2, norms [R] = |G_r| kept for the backward.  A row's
 * squares are summed per block over contiguous spans in a fixed lane order, the partials in index order (ws: alm_grad_penalty_ws_floats(R, n) floats,
 * -1 outside the envelope R <= 65535).  _bwd: dG = gout[0] weight 2 (|G_r| - center) / R G / |G_r| (0 for a row of norm 0); gout is read from device
 * memory. */
int alm_grad_penalty_ws_floats(int R, long long n);
int alm_grad_penalty_fwd(const float* G, float* out, float* norms, float* ws, long long ws_floats, int R, long long n, float weight, float center,
                         void* stream);
int alm_grad_penalty_bwd(const float* G, const float* norms, const float* gout, float* dG, int R, long long n, float weight, float center, void* stream);

/* ---- ComplexSTFTDiscriminator of SoundStream training (csrc/stft_discr.hip), fp32, no atomics -------------------------------------------------------
 * Complex tensors are interleaved (re, im) pairs (torch.complex64's storage); a gradient is the pair (dL/dre, dL/dim) (reference soundstream.py:173-310).
 * Every matrix product is an implicit GEMM on the exact-fp32 matrix core.
 * alm_stft_fwd : x [B][n] -> X [B][F][T][2], torch.stft(center=True, pad_mode='reflect') with T = alm_stft_frames = (n + 2 (n_fft / 2) - n_fft) / hop + 1
 *     (-1 unless n > n_fft / 2: one reflection must land inside the clip; the launchers then return ALM_ERR_UNSUPPORTED).  basis [n_fft][2 F]: column
 *     2 f = w[k] cos(2 pi f k / n_fft), 2 f + 1 = -w[k] sin(.), the window zero-padded and centred to n_fft, times n_fft^-0.5 when normalized; F <= n_fft.
 *     The reflect padding is index mirroring inside the operand load.
 * alm_stft_bwd : dx [B][n] from dX: the frames' gradient [n_fft][B T] into ws (alm_stft_bwd_ws_floats floats; -1: outside the envelope), then every
 *     sample gathers its own sum over its padded positions (itself, its mirrors) and the frames covering each, in a fixed order.
 * alm_cconv2d_* : zero-padded complex conv2d, dilation 1.  x [B][Cin][H][W][2], w [Cout][Cin][kh][kw][2] and bias [Cout][2] (view_as_real of a complex
 *     nn.Conv2d's parameters, read as they are), y [B][Cout][Ho][Wo][2] = conv + bias (+ residual [B][Cout][Ho][Wo][2] when not null).
 *     alm_cconv2d_out_hw writes Ho = (H + 2 ph - kh) / sh + 1 and Wo and returns 0, or -1 when the padded input is smaller than the kernel.
 *   alm_cconv2d_dgrad : dx [B][Cin][H][W][2] from g = dL/dy.  Its derivative with respect to g is alm_cconv2d_fwd with a null bias (bias and
 *                       residual of alm_cconv2d_fwd may be null: nothing is added).
 *   alm_cconv2d_wgrad : dw in the parameter's layout, db [Cout][2]; partial sums per split of the (b, ho, wo) list into ws
 *                       (alm_cconv2d_wgrad_ws_floats floats, caller-owned; -1: outside the kernel's envelope), then added in split order.
 * alm_modrelu_fwd : y = relu(|z| + b) z / |z| over n complex elements, b a scalar in device memory; z = 0 gives relu(b) + 0i.
 * alm_modrelu_bwd : where |z| + b > 0, with u = z / |z|: dz = g + b (g - u (u . g)) / |z| and db += u . g (at z = 0: dz = 0, db += g_re); else 0.
 *     dz may be null; db[0] is summed in two fixed-order stages through ws (alm_modrelu_ws_floats floats).
 * alm_cabs_fwd / _bwd : y = |z| [n] and dz = g z / |z| (0 at z = 0).
 * Second order (double backward of the gradient penalty), with u = z / |z|, r = |z|, P = I - u u^T on (re, im) pairs:
 * alm_modrelu_bwd2 : alm_modrelu_bwd as a function of (g, z, b) against the cotangents v [n][2] of dz (null: zero) and beta[0] (device) of db, one
 *     launch: dg = v + (b / r) P v + beta u;  dz = -(b / r^2) (<v, P g> u + (u . g) P v + (u . v) P g) + (beta / r) P g (may be null);
 *     db[0] = sum <v, P g> / r in the two fixed-order stages of alm_modrelu_bwd (same ws); all 0 where |z| + b <= 0; at z = 0: dg = (beta, 0).
 * alm_cabs_bwd2 : alm_cabs_bwd against the cotangent v of dz: dg [n] = u . v, dz = g P v / r (may be null); both 0 at z = 0. */
int alm_stft_frames(int n, int n_fft, int hop);
int alm_stft_fwd(const float* x, const float* basis, float* X, int B, int n, int n_fft, int hop, int F, void* stream);
int alm_stft_bwd_ws_floats(int B, int n, int n_fft, int hop);
int alm_stft_bwd(const float* dX, const float* basis, float* dx, float* ws, long long ws_floats, int B, int n, int n_fft, int hop, int F, void* stream);
int alm_cconv2d_out_hw(int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int* Ho, int* Wo);
int alm_cconv2d_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int B, int Cin, int Cout, int H, int W, int kh,
                    int kw, int sh, int sw, int ph, int pw, void* stream);
int alm_cconv2d_dgrad(const float* g, const float* w, float* dx, int B, int Cin, int Cout, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw,
                      void* stream);
int alm_cconv2d_wgrad_ws_floats(int B, int Cin, int Cout, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw);
int alm_cconv2d_wgrad(const float* g, const float* x, float* dw, float* db, float* ws, long long ws_floats, int B, int Cin, int Cout, int H, int W, int kh,
                      int kw, int sh, int sw, int ph, int pw, void* stream);
int alm_modrelu_ws_floats(void);
int alm_modrelu_fwd(const float* z, const float* b, float* y, long long n, void* stream);
int alm_modrelu_bwd(const float* g, const float* z, const float* b, float* dz, float* db, float* ws, long long n, void* stream);
int alm_cabs_fwd(const float* z, float* y, long long n, void* stream);
int alm_cabs_bwd(const float* g, const float* z, float* dz, long long n, void* stream);
int alm_modrelu_bwd2(const float* g, const float* z, const float* b, const float* v, const float* beta, float* dg, float* dz, float* db, float* ws,
                     long long n, void* stream);
int alm_cabs_bwd2(const float* g, const float* z, const float* v, float* dg, float* dz, long long n, void* stream);

/* ---- multi-spectral mel-spectrogram reconstruction loss of SoundStream training (csrc/mel_loss.hip), fp32, no atomics ---------------------------------
 * torchaudio.transforms.MelSpectrogram (power 2, center, reflect, one-sided, HTK) per scale and the two per-frame norms of reference
 * soundstream.py:933-945; real and fake waves run as one batch [real | fake].  Every matrix product is on the exact-fp32 matrix core.
 * alm_mel_power_fwd : x [B][n] -> P [B][F][T] = |STFT|^2 (T = alm_stft_frames), the DFT product of alm_stft_fwd with the power formed in its epilogue.
 *     basis [n_fft][2 F] as for alm_stft_fwd (torchaudio's normalized=True, 1 / sqrt(sum w^2), multiplied in by the host); the reduction runs over the
 *     basis rows [k_lo, k_hi) only (the window's support; the rows outside must be zeros).  X (may be null) receives the complex spectrum
 *     [B - x_from][F][T][2] of the batch rows from x_from on.
 * alm_mel_project_fwd : mel [B][n_mels][T] = fb^T P, fb [F][n_mels].
 * alm_mel_frame_loss_fwd : mel [2 Bh][n_mels][T] (first half real, second fake) -> norms [Bh T] = per frame ||log max(Mo, 1e-20) - log max(Mr, 1e-20)||_2,
 *     means[0] = mean over frames of sum_m |Mo - Mr|, means[1] = mean of norms, loss[0] = means[0] + alpha means[1]; two fixed-order stages through ws
 *     (alm_mel_loss_ws_floats floats).
 * alm_mel_frame_loss_bwd : dmel [Bh][n_mels][T] = d(gout loss) / d(fake mel), gout a scalar in device memory; sign(0) = 0, 0 through an inactive clamp
 *     and where a frame's norm is 0.
 * alm_mel_power_bwd : dX [B][F][T][2] = 2 X (fb dmel): the gradient of the spectrum X [B][F][T][2], the operand of alm_stft_bwd. */
int alm_mel_power_fwd(const float* x, const float* basis, float* P, float* X, int B, int x_from, int n, int n_fft, int hop, int F, int k_lo, int k_hi,
                      void* stream);
int alm_mel_project_fwd(const float* P, const float* fb, float* mel, int B, int F, int T, int n_mels, void* stream);
int alm_mel_loss_ws_floats(void);
int alm_mel_frame_loss_fwd(const float* mel, float* norms, float* loss, float* means, float* ws, int Bh, int n_mels, int T, float alpha, void* stream);
int alm_mel_frame_loss_bwd(const float* mel, const float* norms, const float* gout, float* dmel, int Bh, int n_mels, int T, float alpha, void* stream);
int alm_mel_power_bwd(const float* dmel, const float* fb, const float* X, float* dX, int B, int F, int T, int n_mels, void* stream);

/* ---- the denoising SoundStream: squeeze-excite inside the ResidualUnit and the FiLM conditioners (csrc/film_se.hip), exact fp32, no atomics ------
 * SqueezeExcite (reference soundstream.py:145-169) as the ResidualUnit applies it: per column (b, t) of u [B][C][T] the cumulative mean over the
 * CHANNEL axis, m[c] = (u[0] + .. + u[c]) / (c + 1), then gate = sigmoid(W2 silu(W1 m + b1) + b2) with W1 [inner][C], W2 [C][inner] (the nn.Conv1d
 * k = 1 weights as they are) and out = u * gate (+ residual [B][C][T] if given).
 *   alm_se_gate_supported(C, inner) = 1 iff C >= 1 and 1 <= inner <= 128; anything else is ALM_ERR_UNSUPPORTED.
 *   alm_se_gate_bwd : from g = dL/dout and the forward input u (everything else is recomputed): du [B][C][T] (the skip's gradient is the caller's),
 *                     dW1 [inner][C], db1 [inner], dW2 [C][inner], db2 [C].  The parameter gradients are alm_conv1d_wgrad (k = 1) over operands left
 *                     in ws: per-chunk partials summed in chunk order, bitwise reproducible.  ws: alm_se_gate_bwd_ws_floats floats, owned by the
 *                     caller (-1: outside the envelope or past 2^31).
 * FiLM (soundstream.py:442-449) on x [rows][C]: y = x * gamma + beta, (gamma | beta)[i] = W[i][0] cond0 + W[i][1] cond1 + b[i], W [2 C][2], b [2 C].
 *   alm_film_bwd : dx = g * gamma, dW [2 C][2] and db [2 C] from dgamma = sum_r g x, dbeta = sum_r g: per-row-chunk partials in ws
 *                  (alm_film_bwd_ws_floats floats, owned by the caller), summed in chunk order. */
int alm_se_gate_supported(int C, int inner);
int alm_se_gate_fwd(const float* u, const float* residual, const float* W1, const float* b1, const float* W2, const float* b2, float* out, int B, int C,
                    int inner, int T, void* stream);
int alm_se_gate_bwd_ws_floats(int B, int C, int inner, int T);
int alm_se_gate_bwd(const float* g, const float* u, const float* W1, const float* b1, const float* W2, const float* b2, float* du, float* dW1, float* db1,
                    float* dW2, float* db2, float* ws, long long ws_floats, int B, int C, int inner, int T, void* stream);
int alm_film_fwd(const float* x, const float* W, const float* b, float* y, int rows, int C, float cond0, float cond1, void* stream);
int alm_film_bwd_ws_floats(int rows, int C);
int alm_film_bwd(const float* g, const float* x, const float* W, const float* b, float* dx, float* dW, float* db, float* ws, long long ws_floats, int rows,
                 int C, float cond0, float cond1, void* stream);

/* ---- residual finite scalar quantization (csrc/fsq.hip; FSQ, arXiv 2309.15505 Appendix A, in the residual form of vector-quantize-pytorch's
 * GroupedResidualFSQ, restated in tests/fsq_restated.py).  fp32, no float atomics: every output is bitwise reproducible.  One call serves one group:
 * x / out / g / dx are the group's dim_g columns of row-major matrices with leading dimensions ldx / ldo / ldg / ldd; W_in [d][dim_g], b_in [d],
 * W_out [dim_g][d], b_out [dim_g] are the nn.Linear tensors as they are, or ALL NULL in the identity case, which needs dim_g == d.
 * Limits: d <= 8 levels, dim_g <= 1024, Q <= 32 layers, else ALM_ERR_UNSUPPORTED.
 *   consts : alm_fsq_consts_floats(Q) = 56 + 16 Q floats computed by the caller in double and rounded once to fp32: rows of 8 (entry j < d used)
 *            half_l, offset, shift, 1 / half_w, half_w, basis, levels, then scale [Q][8] and 1 / scale [Q][8].  The kernels call no atanh / pow.
 *   alm_fsq_fwd    : z = W_in x + b_in; for q <= k: c_q = rint(tanh(r_q / scale_q + shift) half_l - offset), idx[.][q] = sum_j (c_q[j] + half_w[j])
 *                    basis[j], r_{q+1} = r_q - c_q / half_w scale_q; idx int64 [M][ldi] (Q columns, -1 past k); out = W_out zsum + b_out; z [M][d]
 *                    (DOUBLE) is written when not NULL (the backward's input).  x is read once, out written once.  z and the chain are carried
 *                    in double (scale_q by repeated division): layer q amplifies an error of z by (L - 1)^q, which in fp32 would leave the deep
 *                    layers' codes to rounding noise; so the indices are those of float64 arithmetic on the same fp32 inputs.
 *   alm_fsq_decode : idx [M][ldi] (ncols <= Q columns, negative = no code) -> out = W_out (sum_q ((idx_q / basis) % levels - half_w) / half_w scale_q) + b_out
 *   alm_fsq_bwd    : g_z = W_out^T g; dz = g_z sum_{q <= k} (half_l / half_w) (1 - tanh(..)^2) with the chain recomputed from z; dx = W_in^T dz;
 *                    dW_in = dz^T x, db_in = sum dz, dW_out = g^T zsum, db_out = sum g as per-row-chunk partials in ws (alm_fsq_bwd_ws_floats floats,
 *                    owned by the caller; 0 in the identity case), summed in chunk order.  Identity: dx only (z and the gradient pointers unused). */
int alm_fsq_consts_floats(int Q);
int alm_fsq_fwd(const float* x, long long ldx, const float* W_in, const float* b_in, const float* W_out, const float* b_out, const float* consts,
                long long* idx, long long ldi, float* out, long long ldo, double* z, int M, int dim_g, int d, int Q, int k, void* stream);
int alm_fsq_decode(const long long* idx, long long ldi, const float* W_out, const float* b_out, const float* consts, float* out, long long ldo, int M,
                   int dim_g, int d, int Q, int ncols, void* stream);
int alm_fsq_bwd_ws_floats(int M, int dim_g, int d);
int alm_fsq_bwd(const float* g, long long ldg, const float* x, long long ldx, const double* z, const float* W_in, const float* W_out, const float* consts,
                float* dx, long long ldd, float* dW_in, float* db_in, float* dW_out, float* db_out, float* ws, long long ws_floats, int M, int dim_g,
                int d, int Q, int k, void* stream);

/* ---- residual lookup-free quantization (csrc/lfq.hip; LFQ, arXiv 2310.05737, in the residual form of vector-quantize-pytorch's GroupedResidualLFQ,
 * restated in tests/lfq_restated.py).  fp32 tensors, no float atomics: every output is bitwise reproducible.  One call serves one group, laid out
 * like the FSQ calls above (column views with leading dimensions; W_in [d][dim_g], b_in [d], W_out [dim_g][d], b_out [dim_g], or ALL NULL in the
 * identity case dim_g == d).  d = log2(codebook_size).  Limits: d <= 10, dim_g <= 1024, Q <= 32, else ALM_ERR_UNSUPPORTED.
 *   alm_lfq_fwd    : z = W_in x + b_in; for q <= k, s_q = 2^-q: bit_q[j] = r_q[j] > 0, quant_q = +-s_q, idx[.][q] = sum_j bit_q[j] 2^(d-1-j),
 *                    r_{q+1} = r_q - quant_q; idx int64 [M][ldi] (Q columns, -1 past k); out = W_out (sum_q quant_q) + b_out.  z and the chain are
 *                    carried in DOUBLE (the logits of layer q multiply an error of z by 2 inv_temperature 2^-q); z [M][d] (double) is written when
 *                    not NULL.  With losses != NULL (training mode; needs z, avg and ws) also, per layer q <= k, with p_m = softmax_c(2
 *                    inv_temperature <r_q[m], C_q[c]>) over the 2^d sign patterns C_q[c] = +-s_q and H(t) = -sum_c t_c log max(t_c, 1e-5):
 *                      losses[q] = entropy_w (mean_m H(p_m) - gamma H(mean_m p_m)) + commit_w mean_{m,j} (r_q - quant_q)^2      (0 for q > k)
 *                    and avg [Q][2^d] (double) = mean_m p_m (zero rows for q > k), which the backward needs.  The softmax factorises over the bits, so a
 *                    probability is a product of d per-bit sigmoids, formed in double for all 2^d codes; the sum over the rows goes through
 *                    per-row-chunk partials in ws (alm_lfq_fwd_ws_doubles doubles, owned by the caller) added in chunk order by a finish launch.
 *   alm_lfq_decode : idx [M][ldi] (ncols <= Q columns, negative = no code) -> out = W_out (sum_q +-2^-q by the bits of idx_q) + b_out
 *   alm_lfq_bwd    : g_z = W_out^T g; dz = (k + 1) g_z + sum_{q <= k} g_loss[q] d losses[q] / d r_q (the chain recomputed from z; g_loss [Q] floats
 *                    on the device, or NULL for none); dx = W_in^T dz; dW_in = dz^T x, db_in = sum dz, dW_out = g^T zsum, db_out = sum g as
 *                    per-row-chunk partials summed in chunk order.  ws: alm_lfq_bwd_ws_floats floats (the per-layer loss gradients [Q][M][d], then
 *                    the partials).  Identity: dx only (the parameter pointers NULL); z is still needed. */
int alm_lfq_fwd_ws_doubles(int M, int d, int Q);
int alm_lfq_fwd(const float* x, long long ldx, const float* W_in, const float* b_in, const float* W_out, const float* b_out, long long* idx,
                long long ldi, float* out, long long ldo, double* z, float* losses, double* avg, double* ws, long long ws_doubles, int M, int dim_g,
                int d, int Q, int k, float inv_temperature, float entropy_w, float commit_w, float gamma, void* stream);
int alm_lfq_decode(const long long* idx, long long ldi, const float* W_out, const float* b_out, float* out, long long ldo, int M, int dim_g, int d,
                   int Q, int ncols, void* stream);
int alm_lfq_bwd_ws_floats(int M, int dim_g, int d, int Q);
int alm_lfq_bwd(const float* g, long long ldg, const float* g_loss, const float* x, long long ldx, const double* z, const double* avg,
                const float* W_in, const float* W_out, float* dx, long long ldd, float* dW_in, float* db_in, float* dW_out, float* db_out, float* ws,
                long long ws_floats, int M, int dim_g, int d, int Q, int k, float inv_temperature, float entropy_w, float commit_w, float gamma,
                void* stream);

/* ---- the gate-loop layer of SoundStream(use_gate_loop_layers=True) (csrc/gate_loop.hip; restated in tests/gate_loop_restated.py).  Codec layout
 * [B][C][T] fp32, time contiguous; exact fp32, no atomics: every output is bitwise reproducible.
 *   alm_gate_loop_norm_fwd : xn = x r gamma, r[b,t] = sqrt(C) / max(||x[b,:,t]||_2, 1e-12)   (the k = 1 projection z = W xn is alm_conv1d_causal)
 *   alm_gate_loop_scan_fwd : z [B][3 C][T] (rows q | kv | a) -> h[t] = sigmoid(z_a[t]) h[t-1] + z_kv[t], h[-1] = 0 (so a[0] has no effect);
 *                            out = z_q h + 2 x, or with h_only out = h (x may be NULL).  A workgroup scans one chunk of alm_gate_loop_chunk() steps
 *                            of one row (lanes compose 4 consecutive steps, a 64-lane shuffle scan, waves through LDS); rows longer than a chunk
 *                            take three launches (chunk aggregates, an ordered carry pass per row, apply) and need ws (alm_gate_loop_scan_ws_floats
 *                            floats, owned by the caller; 0 for rows of at most one chunk, then ws may be NULL).  The chunk length is a constant of
 *                            the library.  16-byte accesses when T % 4 == 0 and the tensors are 16-byte aligned, scalar ones otherwise.
 *   alm_gate_loop_scan_bwd : g = dL/dout [B][C][T], z, h (of an h_only forward) -> dz [B][3 C][T]: dq = g h, dkv = dh with
 *                            dh[t] = g[t] q[t] + a[t+1] dh[t+1] (the same scan from the row's end, gate shifted by one), da = dh h[t-1] a (1 - a),
 *                            exactly 0 at t = 0.  Without the 2 g of the two skips (alm_gate_loop_norm_bwd adds it).
 *   alm_gate_loop_norm_bwd : dxn = dL/dxn -> dx = r gamma dxn - x (r^3 / C) sum_k dxn_k gamma_k x_k + 2 g; dgamma [C] = sum_{b,t} dxn x r from
 *                            per-block partials in ws (alm_gate_loop_norm_bwd_ws_floats floats), added in block order.
 * Limits: B <= 65535 for the two norm calls, B C ceil(T / chunk) < 2^31 / 3 for the scans; else ALM_ERR_UNSUPPORTED. */
int alm_gate_loop_chunk(void);
int alm_gate_loop_norm_fwd(const float* x, const float* gamma, float* xn, int B, int C, int T, void* stream);
int alm_gate_loop_scan_ws_floats(int B, int C, int T);
int alm_gate_loop_scan_fwd(const float* z, const float* x, float* out, float* ws, long long ws_floats, int B, int C, int T, int h_only, void* stream);
int alm_gate_loop_scan_bwd(const float* g, const float* z, const float* h, float* dz, float* ws, long long ws_floats, int B, int C, int T, void* stream);
int alm_gate_loop_norm_bwd_ws_floats(int B, int C, int T);
int alm_gate_loop_norm_bwd(const float* dxn, const float* x, const float* gamma, const float* g, float* dx, float* dgamma, float* ws,
                           long long ws_floats, int B, int C, int T, void* stream);

/* ---- launch lists (round 6): a recorded sequence of the launches above re-issued by ONE host call ---------------------------------------------
 * The depth loop of audiolm_pytorch.py:528-547 (Transformer.forward) and its backward are ~190 launches per training step whose ORDER and scalar arguments
 * depend only on the model configuration and the batch shape; only buffer addresses change between steps.  The host records the sequence once per shape
 * (audiolm-pytorch_amd/launchlist.py: every pointer argument classified as base + byte offset against a table of bases -- the step's activation arena, the
 * inputs, every parameter, every packed weight image) and alm_list_run re-issues it: the same entry points, in the same order, on `stream` -- the results are
 * bit-identical to issuing them one by one.  Nothing is baked (unlike a hipGraph replay): addresses, the stream and the weight images are live.
 *   entries[e] = {op (alm_list_op_id of the entry point), nargs (must equal alm_list_op_nargs), first (index of its first slot)}
 *   slots[i]   = one 64-bit value per C argument (int / long long sign-extended, float = its bit pattern in the low word, pointer = byte offset)
 *   reloc[i]   = ALM_LIST_LITERAL: slots[i] as is;  1 .. nbases: bases[reloc - 1] + slots[i];  ALM_LIST_STREAM: the `stream` argument;
 *                ALM_LIST_HOST_PTRS: a HOST array of pointers = the resolved slots starting at index slots[i];  ALM_LIST_HOST_INTS: a HOST array of ints
 *                packed into the slots starting at index slots[i] (alm_hc_param_grads_batched takes both)
 * Returns 0, or the first failing launch's code with its index in *failed_at (launches before it were issued).  alm_memset_zero: zero-fill by a kernel (a small hipMemsetAsync node of a captured hipGraph is not replayed correctly on ROCm 7.0: scripts/debug/memset_node_probe.py). */
typedef struct { int op; int nargs; int first; int reserved; } AlmListEntry;
#define ALM_LIST_LITERAL 0
#define ALM_LIST_STREAM 0xFFFF
#define ALM_LIST_HOST_PTRS 0xFFFE
#define ALM_LIST_HOST_INTS 0xFFFD
int alm_memset_zero(void* ptr, long long bytes, void* stream);
int alm_list_op_id(const char* name);
int alm_list_op_nargs(int op);
int alm_list_run(const AlmListEntry* entries, int n, const unsigned long long* slots, const unsigned short* reloc, int nslots,
                 const unsigned long long* bases, int nbases, void* stream, int* failed_at);

#ifdef __cplusplus
}
#endif
