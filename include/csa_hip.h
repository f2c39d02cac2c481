/* C ABI of libcsa_hip.so — MI355X (gfx950) kernels for the CSA-Trans attention hot path.
 *
 * Every entry point replaces one piece of the reference's PyTorch-eager hot path
 * (paths relative to the reference repo saeyoon17/Code-Structure-Aware-Transformer):
 *
 *   csa_sbm_fwd        module/sbm_attn.py:32-66   SBMAttention.forward (+ STE.py:10-15 sampling)
 *                      module/sbm_attn.py:77-87   FullAttention.forward   (flags & CSA_FLAG_DENSE)
 *   csa_sbm_maps       module/sbm_attn.py:62,57   the returned `attn` / `graph` maps (optional)
 *   csa_sbm_bwd        autograd of the above incl. STE.py:17-19 (hardtanh straight-through)
 *   csa_dense_attn_fwd/_bwd  module/sbm_attn.py:69-87 FullAttention (csa_sbm_* with CSA_FLAG_DENSE)
 *   csa_ste_sample     module/STE.py:10-15        standalone sampler (bit-exact test surface)
 *   csa_rel_attn_fwd   module/disentangled_attn.py:44-65 DisentangledAttn.rel_attn
 *   csa_rel_attn_bwd   autograd of rel_attn (gather backward = deterministic scatter-add)
 *   csa_adamw_step     script/optimizer.py:49-106 AdamW.step (all parameters in one launch)
 *   csa_grad_sumsq / csa_grad_norm_finish / csa_adamw_step_clipped  global gradient-norm clipping in front of
 *                      that step (script/train.py:93,171 construct the trainer with max_grad_norm=1.0)
 *   csa_gen_logsoftmax_fwd/_bwd  module/components.py:95-102 Generator: log(softmax(dropout(logits)))
 *   csa_bias_grad      Linear bias gradient (column sums of dY) of the encoder/decoder glue
 *   csa_layernorm_fwd/_bwd  nn.LayerNorm of the encoder glue (module/components.py SublayerConnection)
 *   csa_ast_relations  my_ast.py:198-273 + dataset/base_data_set.py:33-36 (host C++, no GPU)
 *   csa_decode_attn / csa_argmax_rows  module/base_seq2seq.py:117-145 GreedyGenerator, one KV-cached decode step
 *                      (and their device-stepped forms for a captured step: csa_decode_attn_step, csa_decode_embed,
 *                      csa_argmax_rows_step)
 *   csa_beam_row_topk / csa_beam_select / csa_decode_attn_beam  beam search over the same cached step (no
 *                      counterpart in the reference, whose only strategy is the greedy loop above): per-row top-W
 *                      and log-sum-exp, the per-AST merge with its in-place state update, and the decode attention
 *                      reading its cache through an ancestry table and one memory projection per AST
 *
 * Conventions (all entry points):
 *   - fp32 data; device pointers; sizes and strides are int64 ELEMENT counts; the last
 *     (feature) dimension is always contiguous, so a (B,H,N,d) operand is described by its
 *     b/h/n strides (the non-contiguous split_heads view of sbm_attn.py:137-140 is accepted).
 *   - The SBM and dense entry points (csa_sbm_fwd / csa_sbm_bwd / csa_sbm_maps) take N queries against
 *     M keys and support N != M; the CSE relation attention (csa_rel_attn_*) is square by definition.
 *   - The caller allocates every output, the saved state and the workspace (sizes from the
 *     *_bytes() queries), and owns every stream and event: the library never allocates, never
 *     creates a stream or event, never synchronises the host and never throws. It enqueues
 *     everything on `stream` (stream-ordered, graph-capturable, re-entrant) on the device that
 *     stream belongs to, whatever the calling thread's current device is. Its only state is a
 *     per-thread last-error string and a cache of which kernels already had their (idempotent)
 *     dynamic-LDS attribute raised on which device. Results are deterministic for fixed inputs
 *     (integer atomics only; float reductions use fixed-order partial slabs), whatever the
 *     backward schedule.
 *   - Errors: CSA_INVALID_ARG (null/inconsistent arguments), CSA_UNSUPPORTED_SHAPE (outside
 *     the compiled instantiations, see csa_sbm_supported), CSA_LAUNCH_FAILED (HIP error; text
 *     via csa_last_error_str on the calling thread).
 */
#ifndef CSA_HIP_H
#define CSA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSA_ABI_VERSION 10

typedef enum csa_status {
  CSA_OK = 0,
  CSA_INVALID_ARG = 1,
  CSA_UNSUPPORTED_SHAPE = 2,
  CSA_LAUNCH_FAILED = 3
} csa_status;

/* flags */
#define CSA_FLAG_DENSE 1u /* FullAttention (graph == 1, no cluster projection, no sampling) */
/* ABI v6: the caller will not run csa_sbm_bwd on this forward's state (inference / no_grad): the state omits the
 * projection MLP's saved activations, which only the backward reads (csa_sbm_state_bytes shrinks, the forward
 * skips their stores); csa_sbm_bwd rejects such a state. */
#define CSA_FLAG_FWD_ONLY 2u
/* ABI v8: the call pair runs with dtype CSA_DTYPE_BF16. csa_sbm_bwd_workspace_bytes then omits the fp32 backward's
 * ds / G tile handoff (bf16 mode recomputes S and dP on the query side instead), which is O(B*H*N*M) floats: with
 * clusters two (B,H,NQB,NKB,32,32) fp32 planes (at B=16, H=8, N=M=1024: 1.07 GB), without (DENSE) one plane.
 * csa_sbm_bwd lays a bf16 call's workspace out without the handoff whether or not the flag is set (a buffer sized
 * without it is merely larger); the flag on an fp32 call is CSA_INVALID_ARG. csa_sbm_state_bytes ignores it. */
#define CSA_FLAG_BF16_WS 4u

/* ABI v5: schedule of an attention backward's two halves (csa_rel_attn_bwd_args .schedule). The key half
 * may run on a caller-owned side stream beside the query half, forked from and joined back into `stream`
 * with two caller-owned events (capture-safe); outputs are bitwise the same either way. AUTO uses the side
 * stream when the query half's grid leaves a partial last round of workgroups on the device (side_stream
 * must be set, else it runs in order). ABI v6, csa_sbm_bwd: the projection backward's key-block items (they
 * need only the key half's dT) run on the side stream beside the query half (k_attn_bwd_qg) and its query-
 * block items on CSA_SCHED_CONCURRENT only (AUTO runs in order: faster at the headline shape, measured).
 * Bitwise-identical results either way. */
#define CSA_SCHED_AUTO 0u
#define CSA_SCHED_IN_ORDER 1u
#define CSA_SCHED_CONCURRENT 2u /* needs side_stream / side_fork / side_join */

/* operand precision of the N^2 attention contractions (dtype field of the args structs). Storage is
 * fp32 either way. CSA_DTYPE_F32 is the reference's precision (sbm_attn.py:120-126 forces fp32) and
 * the parity mode (rtol 1e-4 / atol 1e-5). CSA_DTYPE_BF16 rounds the operands of QK^T, dX V^T, PV, dQ,
 * dK, dV, of the projection MLP (three d x d layers, forward and backward chains and weight-gradient
 * products) and of sigmoid(. C^T) and its backward (SBM), and of the CSE's c2c, PV and their gradients
 * to bf16 for v_mfma_f32_32x32x16_bf16 (fp32 accumulation; north_star tolerance 2e-2). T = Kh S^T, expA,
 * the sampling threshold and every softmax / normalisation / elementwise step stay fp32. Inside the saved
 * state (opaque, csa_sbm_state_bytes unchanged) bf16 mode keeps the projection MLP's activations as bf16,
 * rounded as its MFMAs round them; the backward of the same call pair reads them back. */
#define CSA_DTYPE_F32 0
#define CSA_DTYPE_BF16 1

/* Optional per-stage timing: caller-created hipEvent_t handles; when start[s] and stop[s] are
 * non-NULL the library records them on `stream` around stage s (no library-side state). */
enum {
  CSA_STAGE_PREP = 0,       /* cluster softmax + fragment prep */
  CSA_STAGE_PROJ_FWD = 1,   /* k_proj_fwd */
  CSA_STAGE_ATTN_FWD = 2,   /* k_attn_fwd */
  CSA_STAGE_ATTN_BWD_Q = 3, /* k_attn_bwd_qg (bf16 mode: k_attn_bwd_qr) */
  CSA_STAGE_ATTN_BWD_KV = 4,/* k_attn_bwd_kv */
  CSA_STAGE_PROJ_BWD = 5,   /* k_proj_bwd (concurrent schedule: its query-block items only) */
  CSA_STAGE_REDUCE = 6,     /* slab reduction + cluster grad */
  CSA_STAGE_PROJ_BWD_K = 7, /* concurrent schedule: k_proj_bwd's key-block items, on the side stream */
  CSA_STAGE_ATTN_ROWPREP = 8, /* ABI v7: k_attn_rowprep, timed apart from k_attn_bwd_kv */
  CSA_STAGE_COUNT = 9
};
typedef struct csa_prof {
  void* start[CSA_STAGE_COUNT];
  void* stop[CSA_STAGE_COUNT];
} csa_prof;
/* ABI v9: the same profiling struct (slots 0..5) around the CSE relation attention's stages (d_k = 64 fused path):
 * csa_rel_attn_args.prof / csa_rel_attn_bwd_args.prof */
enum {
  CSA_REL_STAGE_LOGITS = 0, /* k_rel_logits + k_rel_prep (relation logits, code planes) */
  CSA_REL_STAGE_FWD = 1,    /* k_rel_fwd_f */
  CSA_REL_STAGE_QSTAT = 2,  /* k_rel_qstat (row statistics for the key side) */
  CSA_REL_STAGE_BWD_K = 3,  /* k_rel_bwd_kh (fp32) / k_rel_bwd_kf (bf16) */
  CSA_REL_STAGE_BWD_Q = 4,  /* k_rel_bwd_qg (fp32) / k_rel_bwd_qf (bf16) */
  CSA_REL_STAGE_LGRAD = 5   /* k_rel_lgrad + k_sum_splits2 (dlq, dlk) */
};

typedef struct csa_sbm_fwd_args {
  int64_t B, H, N, M, d, k; /* batch, heads, queries, keys, head_dim, clusters (k ignored if DENSE) */
  const float* Q; int64_t q_sb, q_sh, q_sn; /* (B,H,N,d) */
  const float* K; int64_t k_sb, k_sh, k_sn; /* (B,H,M,d) */
  const float* V; int64_t v_sb, v_sh, v_sn; /* (B,H,M,d) */
  const float* key_mask; int64_t mask_sb;   /* (B,M) 1.0 = padded key (sbm_attn.py:61); may be NULL */
  const float* cluster_w;                   /* layer.weight (H*k, d) contiguous (sbm_attn.py:19) */
  const float* proj_w[3]; const float* proj_b[3]; /* proj.0/.3/.6 weight (d,d) and bias (d) */
  const float* uniforms;      /* (B,H,N,M) contiguous host-supplied draws, or NULL = Philox */
  uint64_t seed, offset;      /* Philox key / counter offset (sampling + dropout) */
  float attn_dropout;         /* drop_attn p (0 in eval) — sbm_attn.py:14,63 */
  float proj_dropout;         /* proj Dropout p (0 in eval) — sbm_attn.py:24,27 */
  uint32_t flags;
  uint32_t dtype;             /* CSA_DTYPE_F32 or CSA_DTYPE_BF16 */
  float* X;                   /* out (B,H,N,d), strides x_* below */
  float* sparsity;            /* out (H,) head-wise sparsity (sbm_attn.py:64); NULL if DENSE */
  void* state;                /* csa_sbm_state_bytes(): saved for backward and csa_sbm_maps */
  const csa_prof* prof;       /* optional stage timing (NULL = off) */
  /* ABI v3: element strides of X; all three 0 = (B,H,N,d) contiguous. d stays contiguous; like
   * Q/K/V, X must be 16-byte aligned with strides multiple of 4 elements. A (B,N,H,d) buffer read
   * as (B,H,N,d) makes combine_heads (sbm_attn.py:143-146) a free view. */
  int64_t x_sb, x_sh, x_sn;
} csa_sbm_fwd_args;

typedef struct csa_sbm_bwd_args {
  const csa_sbm_fwd_args* fwd; /* the forward's arguments (same inputs and the filled state) */
  const float* dX;             /* (B,H,N,d), strides dx_* below */
  const float* dsparsity;      /* (H,) or NULL */
  const float* dgraph;         /* (B,H,N,M) grad of the returned graph map, or NULL */
  float* dQ; float* dK; float* dV; /* out (B,H,N|M,d), strides dq_* / dk_* / dv_* below */
  float* dcluster_w;           /* out (H*k, d); NULL if DENSE */
  float* dproj_w[3]; float* dproj_b[3]; /* out; NULL if DENSE */
  void* workspace;             /* csa_sbm_bwd_workspace_bytes(); required (ABI v6: also for DENSE) */
  const csa_prof* prof;        /* optional stage timing (NULL = off) */
  /* ABI v3: element strides (b, h, row) of dX, dQ, dK, dV; a zero triple = contiguous. E.g. dQ/dK/dV
   * as the three head-major views of one packed (B,N,3,H,d) gradient of a fused QKV projection. */
  int64_t dx_sb, dx_sh, dx_sn, dq_sb, dq_sh, dq_sn, dk_sb, dk_sh, dk_sn, dv_sb, dv_sh, dv_sn;
  /* ABI v4: (B,H,N,M) contiguous upstream gradient of the returned attn map (sbm_attn.py:62, the tensor the
   * reference returns), or NULL. */
  const float* dattn;
  /* ABI v5: CSA_SCHED_* and the caller's side lane: a hipStream_t of the same device as `stream` and two
   * hipEvent_t (hipEventDisableTiming) used only between this call's fork and join. NULL = in order. */
  uint32_t schedule;
  void* side_stream; void* side_fork; void* side_join;
} csa_sbm_bwd_args;

int csa_abi_version(void);
/* sha256 (hex) of the csrc/ sources + headers and this header the library was built from
 * (csa_amd/build.py:source_hash); lets a caller prove the loaded binary matches its source tree. */
const char* csa_source_hash(void);
const char* csa_status_str(csa_status s);
const char* csa_last_error_str(void);
/* 1 if (d, k, flags) is a compiled instantiation */
int csa_sbm_supported(int64_t d, int64_t k, uint32_t flags);
size_t csa_sbm_state_bytes(int64_t B, int64_t H, int64_t N, int64_t M, int64_t d, int64_t k, uint32_t flags);
size_t csa_sbm_bwd_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t M, int64_t d, int64_t k, uint32_t flags);

csa_status csa_sbm_fwd(const csa_sbm_fwd_args* a, void* stream);
/* Materialise attn (B,H,N,M) and/or graph (B,H,N,M) fp32 maps from a completed forward. */
csa_status csa_sbm_maps(const csa_sbm_fwd_args* a, float* graph, float* attn, void* stream);
csa_status csa_sbm_bwd(const csa_sbm_bwd_args* a, void* stream);
/* FullAttention (module/sbm_attn.py:77-87): the two calls above with CSA_FLAG_DENSE forced (k, cluster_w,
 * proj_*, uniforms and sparsity ignored). */
csa_status csa_dense_attn_fwd(const csa_sbm_fwd_args* a, void* stream);
csa_status csa_dense_attn_bwd(const csa_sbm_bwd_args* a, void* stream);

/* STE.py:10-15 as A = (u < clamp(p, lo, hi)); n elements, contiguous. */
csa_status csa_ste_sample(const float* p, const float* u, float* A, int64_t n, float lo, float hi, void* stream);
/* STE.py:17-19: gin = hardtanh(A * gout). */
csa_status csa_ste_backward(const float* A, const float* gout, float* gin, int64_t n, void* stream);

/* ---- CSE disentangled relation attention (module/disentangled_attn.py:44-65) ---- */
typedef struct csa_rel_attn_args {
  int64_t B, H, N, L, d; /* H must be 8 (4 parent + 4 sibling heads, disentangled_attn.py:29-33) */
  const float* q; int64_t q_sb, q_sh, q_sn;
  const float* k; int64_t k_sb, k_sh, k_sn;
  const float* v; int64_t v_sb, v_sh, v_sn;
  const float* lq; const float* lk; /* (H, L, d) contiguous (batch dim 1 dropped) */
  const uint8_t* rel;  int64_t rel_sb, rel_sh;  /* (B,*,N,N) relation index < L; head stride may be 0 */
  const uint8_t* mask; int64_t mask_sb, mask_sh;/* (B,*,N,N) 1 = masked (-1e9); head stride may be 0 */
  int64_t rel_head_group; /* heads [0,g) read plane 0, heads [g,H) plane 1 (CSE: 4); 0 = use rel_sh */
  uint32_t dtype;          /* CSA_DTYPE_F32 or CSA_DTYPE_BF16 (bf16: d = 64 only) */
  float* out;          /* (B,H,N,d), strides o_* below */
  float* row_stats;    /* (B,H,N,2) saved (row max, 1/row sum) for backward; kept separate because
                          fully masked rows sit at -1e9 where max + log(sum) is not representable */
  void* state;         /* csa_rel_attn_state_bytes(): relation logits q.lk^T, k.lq^T, kept for backward */
  /* ABI v3: element strides (b, h, row) of out; zero triple = (B,H,N,d) contiguous. Non-contiguous
   * layouts need d = 64 (the fused path); 16-byte aligned, strides multiple of 4 elements. */
  int64_t o_sb, o_sh, o_sn;
  const csa_prof* prof; /* ABI v9: optional stage timing (CSA_REL_STAGE_*; NULL = off) */
} csa_rel_attn_args;

typedef struct csa_rel_attn_bwd_args {
  const csa_rel_attn_args* fwd;
  const float* dout;   /* (B,H,N,d), strides do_* below */
  float* dq; float* dk; float* dv; /* (B,H,N,d), strides dq_* / dk_* / dv_* below */
  float* dlq; float* dlk;          /* (H,L,d) */
  void* workspace;
  /* ABI v3: element strides (b, h, row); a zero triple = contiguous; non-contiguous needs d = 64 */
  int64_t do_sb, do_sh, do_sn, dq_sb, dq_sh, dq_sn, dk_sb, dk_sh, dk_sn, dv_sb, dv_sh, dv_sn;
  /* ABI v5: schedule and side lane as in csa_sbm_bwd_args; only the d_k = 64 fused path uses them, and of it
   * only bf16 mode (CSA_DTYPE_BF16): the fp32 fused backward hands the key half's g tiles to the query half
   * (k_rel_bwd_kh -> k_rel_bwd_qg) and runs in order whatever the schedule */
  uint32_t schedule;
  void* side_stream; void* side_fork; void* side_join;
  const csa_prof* prof; /* ABI v9: optional stage timing (CSA_REL_STAGE_*; NULL = off) */
} csa_rel_attn_bwd_args;

size_t csa_rel_attn_state_bytes(int64_t B, int64_t H, int64_t N, int64_t L, int64_t d);
size_t csa_rel_attn_bwd_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t L, int64_t d);
csa_status csa_rel_attn_fwd(const csa_rel_attn_args* a, void* stream);
csa_status csa_rel_attn_bwd(const csa_rel_attn_bwd_args* a, void* stream);

/* ---- AdamW step (script/optimizer.py:49-106; script/train.py:80 uses correct_bias=False) ----
 * Per element, in the reference's op order:
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p += -step_size * m / (sqrt(v) + eps);
 *   p += -decay * p  (decay = lr * weight_decay, applied after the Adam update as in the reference)
 * step_size = lr, or lr * sqrt(1 - b2^t) / (1 - b1^t) with correct_bias (computed by the caller).
 * torch.amp GradScaler semantics without a host sync: when found_inf is non-NULL and *found_inf != 0
 * the whole step is skipped (nothing written); when grad_scale is non-NULL each gradient is used as
 * g * (float)(1.0 / (double)*grad_scale), GradScaler.unscale_'s inv_scale (grads are not written back). */
#define CSA_ADAMW_CHUNK 4096
typedef struct csa_adamw_tensor { /* one parameter tensor, contiguous fp32 (device pointers) */
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t numel;
} csa_adamw_tensor;

typedef struct csa_adamw_args {
  const csa_adamw_tensor* tensors; /* device array, ntensors entries */
  const int32_t* chunk_tensor;     /* device (nchunks): tensor of each CSA_ADAMW_CHUNK-element chunk */
  const int64_t* chunk_start;      /* device (ntensors): first chunk of each tensor */
  int64_t ntensors, nchunks;
  float beta1, beta2, one_minus_beta1, one_minus_beta2; /* 1-b as the reference's fp32 alpha/value */
  float eps, step_size, decay;
  const float* grad_scale;         /* device scalar or NULL (gradients already unscaled) */
  const float* found_inf;          /* device scalar or NULL (no inf check) */
} csa_adamw_args;

csa_status csa_adamw_step(const csa_adamw_args* a, void* stream);

/* ---- v10 addition: global gradient-norm clipping in front of the AdamW step, no host sync ----
 * The L2 norm over every gradient of the step, in two launches driven by the AdamW tables (no atomics,
 * a fixed summation order: the result is a pure function of the gradients):
 *   csa_grad_sumsq: one workgroup per chunk writes partials[first + chunk] = sum of g^2 over the chunk,
 *     the raw gradients squared and accumulated in fp64 (1e25-sized or GradScaler-scaled gradients do
 *     not overflow). Only the descriptors' grad and numel are read. Parameter groups with tables of
 *     their own fill disjoint ranges of one partials array through `first`. nchunks == 0: CSA_OK, no launch.
 *   csa_grad_norm_finish: one workgroup sums the n partials and writes the 4-float state
 *     state[0] = (float)(sqrt(total) / (double)*grad_scale)   the norm of the UNSCALED gradients
 *                                                            (grad_scale NULL: scale 1)
 *     state[1] = min(1, max_norm / (state[0] + 1e-6))        torch.nn.utils.clip_grad_norm_'s coefficient;
 *                                                            1 when max_norm <= 0 (measure only) or n == 0
 *     state[2] = 1 when the norm is inf or NaN, else 0; then state[1] = 0
 *     state[3] = 0
 *   csa_adamw_step_clipped: csa_adamw_step with that state. The step is skipped when clip[2] != 0, exactly
 *     as for found_inf (torch would write NaN into every parameter instead); otherwise each gradient is
 *     used as (g * inv_scale) * clip[1], two fp32 multiplies in the order of unscale_ then
 *     clip_grad_norm_. Gradients are never written. clip == NULL is csa_adamw_step. */
typedef struct csa_grad_sumsq_args {
  const csa_adamw_tensor* tensors; /* the three tables of csa_adamw_args */
  const int32_t* chunk_tensor;
  const int64_t* chunk_start;
  int64_t ntensors, nchunks;
  double* partials;                /* device, at least first + nchunks entries */
  int64_t first;                   /* >= 0: this call's first slot in partials */
} csa_grad_sumsq_args;

csa_status csa_grad_sumsq(const csa_grad_sumsq_args* a, void* stream);
csa_status csa_grad_norm_finish(const double* partials, int64_t n, const float* grad_scale, float max_norm,
                                float* state, void* stream);
csa_status csa_adamw_step_clipped(const csa_adamw_args* a, const float* clip, void* stream);

/* ---- Generator head (module/components.py:95-102): logp = log(softmax(dropout(logits), -1)) ----
 * logits/logp/dlogp/dlogits: (rows, V) contiguous fp32. dropout p in [0,1) (0 = eval); the keep mask
 * is regenerated in the backward from (seed, offset): Philox stream 4, element (row, col) ->
 * u16 (col & 7) of philox({col >> 3, row, 0, (4 << 28) ^ offset}), keep <=> u16 >= ceil(p * 65536).
 * Backward is the reference autograd chain: t = dlogp / s, dz = keep / (1-p) * s * (t - sum(t * s)). */
csa_status csa_gen_logsoftmax_fwd(const float* logits, float* logp, int64_t rows, int64_t V, float dropout,
                                  uint64_t seed, uint64_t offset, void* stream);
csa_status csa_gen_logsoftmax_bwd(const float* dlogp, const float* logp, float* dlogits, int64_t rows, int64_t V,
                                  float dropout, uint64_t seed, uint64_t offset, void* stream);

/* ---- ABI v10: KV-cached greedy decoding (module/base_seq2seq.py:117-145 GreedyGenerator, one token per step) ----
 * csa_decode_attn: out[b, h*hd : (h+1)*hd] = softmax(scale * q[b,h] . K[b,h,j] over keys j < len, masked keys
 * at -inf) . V[b,h,j], one query row per (b, h), fp32 throughout. hd % 4 == 0 and hd <= 128
 * (csa_decode_attn_supported); any len >= 1. q is (B,H,hd) and K / V are (B,H,>=len,hd) through their element
 * strides, hd contiguous: the same call reads the decoder's self-attention cache and the two planes of a
 * (B,S,2,H,hd) cross-attention memory projection. mask: optional (B,>=len) bytes, non-zero = masked key (a head
 * stride mask_sh != 0 reads a per-head (B,H,>=len) mask instead); a row whose keys are all masked gives NaN (0/0,
 * as SDPA with an all -inf mask), never a fault.
 * Append mode (k_new and v_new both set; len == t + 1): this step's key / value rows (B,H,hd) are stored to
 * cache row t of K / V and used as key t from k_new / v_new themselves; cache rows above t are not touched.
 * Every pointer 16-byte aligned, every stride a multiple of 4 elements. Deterministic (fixed summation order). */
typedef struct csa_decode_attn_args {
  int64_t B, H, hd, len, t;                   /* t: append position, read only in append mode */
  const float* q; int64_t q_sb, q_sh;         /* (B,H,hd) */
  float* K; int64_t k_sb, k_sh, k_sn;         /* (B,H,>=len,hd); written (row t) only in append mode */
  float* V; int64_t v_sb, v_sh, v_sn;
  const float* k_new; int64_t kn_sb, kn_sh;   /* (B,H,hd) or NULL */
  const float* v_new; int64_t vn_sb, vn_sh;   /* (B,H,hd) or NULL */
  const uint8_t* mask; int64_t mask_sb, mask_sh; /* (B,>=len) with mask_sh = 0, (B,H,>=len), or NULL */
  float scale;                                /* hd^-0.5 */
  float* out;                                 /* (B, H*hd) contiguous */
} csa_decode_attn_args;

int csa_decode_attn_supported(int64_t hd);
csa_status csa_decode_attn(const csa_decode_attn_args* a, void* stream);
/* Row argmax of x (rows, V) contiguous fp32: idx[r * idx_stride] = the LOWEST index of row r's maximum (strict >
 * from index 0; an all -inf row gives 0; always in [0, V)), e.g. ys[:, t+1] of an int64 (B, T) token buffer in
 * place. Optional: is_pad[r * pad_stride] = (index == pad_id) as a byte (the next step's key mask), maxval[r] = the
 * row maximum. The eval-mode Generator's log(softmax(z)) is monotone in z, so this is its torch.max(out, 1)[1]. */
csa_status csa_argmax_rows(const float* x, int64_t rows, int64_t V, int64_t* idx, int64_t idx_stride, uint8_t* is_pad,
                           int64_t pad_stride, int64_t pad_id, float* maxval, void* stream);

/* ---- v10 additions: device-stepped decoding (one captured HIP graph replayed for every step of a batch) ----
 * The step index t is read ON THE DEVICE from t_dev (one int32 shared by all rows, 4-byte aligned), so a launch
 * does not depend on the step. None of the three syncs or allocates; a value of t outside the stated range makes
 * the launch store nothing and read no row.
 *
 * csa_decode_attn_step: append-mode csa_decode_attn with t = *t_dev and t + 1 keys. a->len is the CAPACITY (the rows
 * K / V and the mask hold), a->t is ignored, k_new / v_new are required. For equal t, out and the stored cache row
 * are bitwise those of csa_decode_attn. Valid t: [0, capacity). */
csa_status csa_decode_attn_step(const csa_decode_attn_args* a, const int32_t* t_dev, void* stream);
/* x[b, :] = LayerNorm(W[ys[b * ys_stride + t], :] + pe[t, :]) (gamma, beta, eps), the Embeddings row of target
 * position t: ys (B, T) int64 token buffer with a row stride, W (vocab, E), pe (max_len, E) or NULL for no positional
 * term, x (B, E) contiguous; E as csa_layernorm_supported. Bitwise the gather + add + csa_layernorm_fwd (the same row
 * reduction). A token id outside [0, vocab) is clamped into it. Valid t: [0, min(T, max_len)). */
csa_status csa_decode_embed(const int64_t* ys, int64_t ys_stride, int64_t B, int64_t T, const int32_t* t_dev,
                            const float* W, int64_t vocab, const float* pe, int64_t max_len, const float* gamma,
                            const float* beta, float eps, float* x, int64_t E, void* stream);
/* csa_argmax_rows with the destination column chosen on the device: ys[r * ys_stride + t + 1] = the row argmax (same
 * tie rule), pad[r * pad_stride + t + 1] = (index == pad_id) when pad is given, and when head_pad is given (a
 * contiguous (rows, H, T) byte mask) the same byte at head_pad[(h * rows + r) * T + t + 1] for every h < H: the
 * (H, rows, T) view in which the decoder key-pads its heads. Valid t + 1: [1, T). */
csa_status csa_argmax_rows_step(const float* x, int64_t rows, int64_t V, int64_t* ys, int64_t ys_stride, int64_t T,
                                uint8_t* pad, int64_t pad_stride, uint8_t* head_pad, int64_t H, int64_t pad_id,
                                const int32_t* t_dev, void* stream);

/* ---- v10 additions: early stop at EOS for the device-stepped decode step ----
 * csa_argmax_rows_fin_step: csa_argmax_rows_step with a finished flag per row, fin (rows) bytes. A row with
 * fin[r] != 0 takes pad_id and PAD byte 1 (pad and every head of head_pad) whatever its logits; a live row takes its
 * argmax as above and sets fin[r] = 1 when that is eos_id (eos_id < 0: never). fin is otherwise left as it is.
 * Valid t + 1: [1, T), as csa_argmax_rows_step.
 *
 * csa_decode_advance: the end of a step, in place of the counter's increment. state is int32[4] = {all_prev,
 * steps_run, parked, reserved}, zeroed by the caller before step 0; all_now = every byte of fin[0 .. rows) is non-zero
 * (rows = 0: true). One workgroup, no atomics, no waiting:
 *   parked != 0                         nothing changes;
 *   otherwise                           steps_run += 1, then
 *     all_prev != 0 or t + 1 >= T - 1   *t_dev = -1, parked = 1 (every step kernel stores nothing for t < 0);
 *     else                              *t_dev = t + 1, all_prev = all_now.
 * So the counter parks after the first step that BEGAN with every row finished, one step after the step that finished
 * the last row, or after step T - 2; steps_run is then the number of steps that ran. fin may have any alignment; t_dev
 * and state are 4-byte aligned. T >= 2. Neither entry point syncs or allocates. */
csa_status csa_argmax_rows_fin_step(const float* x, int64_t rows, int64_t V, int64_t* ys, int64_t ys_stride, int64_t T,
                                    uint8_t* pad, int64_t pad_stride, uint8_t* head_pad, int64_t H, int64_t pad_id,
                                    uint8_t* fin, int64_t eos_id, const int32_t* t_dev, void* stream);
csa_status csa_decode_advance(const uint8_t* fin, int64_t rows, int64_t T, int32_t* t_dev, int32_t* state,
                              void* stream);

/* ---- v10 additions: beam search over the device-stepped decode step ----
 * Rows are R = B * W hypotheses, row r = b * W + w of AST b, beam width 1 <= W <= 8; the token buffer has T columns,
 * 2 <= T <= 256 (csa_beam_supported states both limits). All fp32, deterministic (fixed reduction orders, no float
 * atomics), no allocation, no sync. Each reads the step t from t_dev as above; a t outside the stated range makes
 * the launch store nothing and read no row, so one captured graph serves every step.
 *
 * csa_beam_row_topk: for each row of z (rows, V) contiguous, V >= W: lse[r] = m + log sum exp(z - m) (an all -inf row
 * gives -inf), topv[r, 0..W) = the W largest logits in descending order and topi[r, 0..W) their indices, the lowest
 * index first among equal values (-inf entries included: an all -inf row gives 0 .. W-1). t_dev may be NULL (the
 * launch is then unconditional); otherwise valid t: [0, t_end). */
int csa_beam_supported(int64_t W, int64_t T);
csa_status csa_beam_row_topk(const float* z, int64_t rows, int64_t V, int64_t W, float* lse, float* topv, int32_t* topi,
                             const int32_t* t_dev, int64_t t_end, void* stream);
/* csa_beam_select: one beam step of every AST, in place. Candidates of AST b: for a live row r (fin[r] == 0) the W
 * pairs (cum[r] + (topv[r, k] - lse[r]), topi[r, k]); for a finished row the single pair (cum[r], pad_id). A score
 * that is -inf or NaN counts as -inf. The best W (score descending, then parent row ascending, then token ascending)
 * become rows b*W + 0 .. b*W + W-1: child c of parent p takes columns 0..t of p's tokens and pad rows and 0..t-1 of
 * its anc row, then tokens[c, t+1] = token, pad[c, t+1] = (token == pad_id), anc[c, t] = p (the cache row where key
 * t of c's history was stored), cum[c] = score, fin[c] = fin[p] || token == eos_id (eos_id < 0: never), and, when
 * parent is given, parent[c] = p. All reads of an AST's rows precede all writes. Valid t: [0, T - 1). */
typedef struct csa_beam_select_args {
  int64_t B, W, T;
  const float* topv; const int32_t* topi;     /* (B*W, W) contiguous, from csa_beam_row_topk */
  const float* lse;                           /* (B*W) */
  float* cum; uint8_t* fin;                   /* (B*W) in / out */
  int64_t* tokens; int64_t tok_stride;        /* (B*W, T) in / out, row strides >= T */
  uint8_t* pad; int64_t pad_stride;           /* (B*W, T) in / out: the self-attention key mask */
  int32_t* anc; int64_t anc_stride;           /* (B*W, T) in / out: the ancestry table of csa_decode_attn_beam */
  int32_t* parent;                            /* (B*W) out, or NULL */
  int64_t eos_id, pad_id;
  const int32_t* t_dev;
} csa_beam_select_args;
csa_status csa_beam_select(const csa_beam_select_args* a, void* stream);
/* csa_decode_attn_beam: csa_decode_attn (t_dev NULL) or csa_decode_attn_step (t_dev set) over a->B = R rows with
 * beam addressing; the chunk walk, the softmax and the summation order are theirs, so on a cache that really was
 * gathered the results are bitwise equal.
 * Self-attention (anc set; append mode and kv_group == 1 required): key / value j < t of row r is read from cache row
 * anc[r * anc_stride + j] (clamped into [0, R)), key t from k_new / v_new, which are stored at cache row r, position
 * t, as without a table; the mask byte is mask[r, j]. No cache row is moved. anc_stride >= len.
 * Cross-attention (anc NULL): K, V and the mask are read at batch index r / kv_group, so the kv_group hypotheses of
 * an AST share one (R / kv_group, S, 2, H, hd) projection; R % kv_group == 0.
 * Otherwise validated as csa_decode_attn (alignment, strides multiples of 4 elements). */
csa_status csa_decode_attn_beam(const csa_decode_attn_args* a, const int32_t* t_dev, const int32_t* anc,
                                int64_t anc_stride, int64_t kv_group, void* stream);

/* ---- v10 additions: sampled decoding (temperature, top-k, top-p) over the device-stepped decode step ----
 * One Gumbel-max draw per row of the (rows, V) fp32 last-position logits, 1 <= V <= 32768 (csa_sample_rows_supported),
 * at the step t read from t_dev; a t outside [0, T - 1) makes the launch store nothing and read no row. Per row r:
 *   y_j = fl32(logits[r, j] * inv_temperature); -inf and NaN entries are never candidates;
 *   top_k (0 < top_k < candidates, else off): kept are the y_j >= the top_k-th largest value, every tie included;
 *   top_p (< 1, else off): with p the softmax of y over the top-k set, kept are the j whose strictly larger entries
 *     hold a mass below top_p (whole classes of equal values; the maximal class always);
 *   token = argmax over the kept j of fl32(y_j + g_j), the lowest index on a tie, g_j = -log(-log u_j),
 *     u_j = ((w_j >> 9) + 0.5) * 2^-23, w_j = word j & 3 of Philox4x32-7 with counter {j >> 2, r, t,
 *     (7 << 28) ^ lo32(offset)} and key (lo32(seed), hi32(seed)); {seed, offset} are read from rng_dev on the device,
 *     so a captured graph draws anew whenever the caller rewrites those 16 bytes;
 *   logp = y_token - log sum exp(y over the kept set). A row without a candidate gives token 0 and logp -inf.
 * A row with fin[r] != 0 takes (pad_id, logp 0) and stays finished; otherwise fin[r] |= (token == eos_id), eos_id < 0:
 * never. Stores ys[r, t + 1] = token, pad[r, t + 1] = (token == pad_id), logp[r, t] (logp may be NULL) and fin[r].
 * Deterministic (fixed reduction orders, no float atomics; results do not depend on the logits' alignment), no
 * allocation, no sync. */
typedef struct csa_sample_rows_args {
  const float* logits; int64_t rows, V, logits_stride;  /* (rows, V), row stride >= V */
  int64_t* ys; int64_t ys_stride;                       /* (rows, T) in / out, row strides >= T */
  uint8_t* pad; int64_t pad_stride;                     /* (rows, T) in / out: the self-attention key mask */
  float* logp; int64_t logp_stride;                     /* (rows, T - 1) out, or NULL; row stride >= T - 1 */
  int64_t T;
  uint8_t* fin;                                         /* (rows) in / out */
  float inv_temperature, top_p;                         /* 1 / temperature > 0; top_p > 0 */
  int64_t top_k;                                        /* >= 0 */
  int64_t eos_id, pad_id;
  const uint64_t* rng_dev;                              /* {seed, offset} on the device, 8-byte aligned */
  const int32_t* t_dev;
} csa_sample_rows_args;
int csa_sample_rows_supported(int64_t V);
csa_status csa_sample_rows(const csa_sample_rows_args* a, void* stream);

/* ---- v10 additions: decoding constraints (repetition penalty, n-gram, length and token bans) on that step ----
 * Rewrites the (rows, V) fp32 last-position logits IN PLACE, between the generator's linear and whichever selection
 * follows (csa_argmax_rows_step, csa_beam_row_topk, csa_sample_rows), which see a banned token as a -inf logit and
 * renormalise over what is left. 2 <= T <= 1024 (csa_constrain_rows_supported); V is not limited. The step t is read
 * from t_dev, or is the host value a->t when t_dev is NULL; a t outside [0, T - 1) makes the launch store nothing and
 * read no row, and so does fin[r] != 0 for its row (fin may be NULL: no row is finished). Per row r, with the history
 * h[0 .. L) = ys[r, 0 .. t], L = t + 1, the literal token columns (BOS included, PAD and EOS as any other id; an id
 * outside [0, V) takes part in every comparison and is never written):
 *   repetition_penalty theta (1: off): for every DISTINCT in-range token v of h, once however often it occurs,
 *     z_v = z_v > 0 ? fl32(z_v / theta) : fl32(z_v * theta), one correctly rounded fp32 operation each, so 0, -inf and
 *     NaN map to themselves;
 *   no_repeat_ngram n (0: off): for every i in [0, L - n] with h[i + k] == h[L - (n - 1) + k] for all 0 <= k < n - 1,
 *     token h[i + n - 1] is banned (n = 1 bans every history token; L < n bans nothing);
 *   min_length: eos_id is banned while t < min_length (off when eos_id < 0 or min_length == 0);
 *   suppress: every in-range id of the device list (at most 256 entries) is banned at every step.
 * A ban stores -inf and wins over the penalty. Nothing else in the row is read or written. Deterministic, no atomics,
 * no allocation, no sync: capturable. */
typedef struct csa_constrain_rows_args {
  float* logits; int64_t rows, V, logits_stride;   /* in / out, row stride >= V */
  const int64_t* ys; int64_t ys_stride, T;          /* (rows, T) token buffer, row stride >= T */
  const uint8_t* fin;                               /* (rows) or NULL */
  float repetition_penalty;                         /* in (0, inf); 1 = off */
  int64_t no_repeat_ngram, min_length, eos_id;
  const int32_t* suppress; int64_t n_suppress;      /* device list, <= 256, or NULL / 0 */
  int64_t t; const int32_t* t_dev;                  /* t_dev NULL: the host value t */
} csa_constrain_rows_args;
int csa_constrain_rows_supported(int64_t T);
csa_status csa_constrain_rows(const csa_constrain_rows_args* a, void* stream);

/* ---- v10 additions: validation metrics of decoded ids (csrc/csa_metric.hip) ----
 * Smoothed sentence BLEU-4 (valid_metrices/google_bleu.py compute_bleu(smooth=True) behind bleu_output_transform) and
 * ROUGE-L (valid_metrices/rouge/rouge.py calc_score, beta = 1.2) of `rows` hypothesis rows against rows / group
 * reference rows; hypothesis row r belongs to reference r / group (1: greedy, W: a beam's n-best list, S: samples).
 * A row's length is the index of its first eos_id, or its full width when it holds none; PAD, UNK and every other id
 * are ordinary tokens. An empty hypothesis is the reference's one-token placeholder, which matches nothing: len_h = 1,
 * poss = (1, 0, 0, 0), no match, lcs = 0. A row whose reference is empty is invalid: valid = 0 and every other output 0.
 * Per row, n = 1..4: m_n = sum over n-grams g of min(count_hyp(g), count_ref(g)), poss_n = max(len_h - n + 1, 0),
 *   bleu  = exp(sum_n 0.25 * log((m_n + 1) / (poss_n + 1))) * bp, bp = 1 if len_h / len_r > 1 else exp(1 - len_r / len_h);
 *   rouge = (1 + beta^2) p r / (r + beta^2 p), p = lcs / len_h, r = lcs / len_r; 0 when lcs = 0;
 * both in fp64 on the device. stats row: m1..m4, poss1..poss4, len_h, len_r, lcs, valid (CSA_SEQ_METRICS_FIELDS int32).
 * 1 <= Th, Tr <= 256 (csa_seq_metrics_supported). A row's outputs depend on that row and its reference alone.
 * Deterministic, no atomics, no allocation, no sync: capturable. */
#define CSA_SEQ_METRICS_FIELDS 12
typedef struct csa_seq_metrics_args {
  const int64_t* hyp; int64_t rows, Th, hyp_stride;   /* (rows, Th) ids, row stride >= Th */
  const int64_t* ref; int64_t Tr, ref_stride;         /* (rows / group, Tr) ids, row stride >= Tr */
  int64_t group, eos_id;                              /* group >= 1 and divides rows */
  int32_t* stats;                                     /* (rows, 12) contiguous */
  double* bleu; double* rouge;                        /* (rows) each */
} csa_seq_metrics_args;
int csa_seq_metrics_supported(int64_t Th, int64_t Tr);
csa_status csa_seq_metrics(const csa_seq_metrics_args* a, void* stream);

/* ---- v10 additions: the structure encodings of the use_pegen ablations (csrc/csa_pe.hip) ----
 * Tree positional encoding (module/csa_trans.py:19-64): pos (rows, depth * width) fp32, p (n_feat) fp32,
 * out / dout (rows, depth * width * n_feat) fp32, all contiguous:
 *   out[r, j * n_feat + f] = pos[r, j] * w[j, f],  w[j, f] = tanh(p_f)^(j / width) * sqrt((1 - tanh(p_f)^2) * d_model / 2),
 * the power an integer power by repeated multiplication (p_f = 0: w = 0 below depth 0, sqrt(d_model / 2) at depth 0).
 * The backward writes dp (n_feat) alone, with torch's pow gradient (0 at exponent 0, 1 at exponent 1): fp64 row-block
 * partials stored to the caller's workspace and summed in a fixed order, no atomics, bitwise repeatable.
 * Supported: depth <= 64 and depth * width * n_feat <= 1024. */
int csa_tree_pos_supported(int64_t depth, int64_t width, int64_t n_feat);
size_t csa_tree_pos_bwd_workspace_bytes(int64_t rows, int64_t depth, int64_t width, int64_t n_feat);
csa_status csa_tree_pos_fwd(const float* pos, const float* p, float* out, int64_t rows, int64_t depth, int64_t width,
                            int64_t n_feat, float d_model, void* stream);
csa_status csa_tree_pos_bwd(const float* pos, const float* p, const float* dout, float* dp, int64_t rows, int64_t depth,
                            int64_t width, int64_t n_feat, float d_model, void* workspace, void* stream);

/* Batched Laplacian eigenvectors (module/base_seq2seq.py:12-36,70-82), one workgroup per AST b with n = num_node[b]
 * clamped to [0, N]: A = adj[b, :n, :n] != 0 (symmetric; anything outside the block is ignored), D = the row sums of A
 * clipped below at 1, L = I - D^-1/2 A D^-1/2. pe[b, :n, :n] holds L's eigenvectors as columns in ascending order of
 * eigenvalue, each with its largest-magnitude entry (the first on ties) positive, eigenvalues[b, :n] the eigenvalues;
 * the rest of pe[b] and eigenvalues[b] is written as zeros. One-sided Jacobi on L + I in LDS; status[b] is 0, or 1 when
 * the sweep cap was reached before convergence (nothing asserts on the device); sweeps[b] (optional) is the number of
 * sweeps run. Deterministic, no atomics, no allocation, no sync.
 * Supported: N <= pegen_dim and (N * (N | 1) + 2 * N + 41) * 4 bytes within the CU's 160 KiB of LDS (N <= 201). */
typedef struct csa_lap_pe_args {
  int64_t B, N, pegen_dim;
  const uint8_t* adj;        /* (B, N, N) contiguous bytes, non-zero = edge */
  const int32_t* num_node;   /* (B) */
  float* pe;                 /* (B, N, pegen_dim) */
  float* eigenvalues;        /* (B, N) */
  int32_t* status;           /* (B) */
  int32_t* sweeps;           /* (B) or NULL */
} csa_lap_pe_args;
int csa_lap_pe_supported(int64_t N, int64_t pegen_dim);
csa_status csa_lap_pe(const csa_lap_pe_args* a, void* stream);

/* ---- v10 additions: batch preparation on the device (csrc/csa_batch.hip) ----
 * Every structural field of a batch of ASTs from parents (B, N) int32 and num_node (B) int32 in one launch, one (or,
 * for large N, several) workgroups per AST; what the host builds in csa_ast_relations and csa_amd/data.py's
 * adjacency / tree_positions / triplet_ids, bit for bit. The contract on a tree is the host builder's: parent[0] < 0
 * and 0 <= parent[v] < v for 0 < v < n, n = num_node[b] clamped to [0, N] (a longer tree is truncated to its first N
 * nodes); any such topological numbering is accepted, not only pre-order (ancestors are found from an Euler-tour
 * interval computed in the kernel, never from the ids). Nodes >= n of the parent array are not read.
 *   depth(v), child_idx(v): the node's depth (root 0) and its rank among its parent's children in increasing id.
 *   rawL[i][j] = depth(j) - depth(i) when one of i, j is a proper ancestor of the other, else 0;
 *   rawT[i][j] = child_idx(j) - child_idx(i) for distinct children of one parent, else 0;
 *   L, T (B, N, N) uint8 = clamp(raw + 75, 0, 149); L_mask, T_mask (B, N, N) bytes = (raw == 0);
 *   adj (B, N, N) bytes = 1 inside the n x n block where |rawL| <= 1, else 0;
 *   tree_pos (B, N, 128) fp32: node v's row is its parent's row plus a 1 at 128 - 8 depth + min(child_idx, 7) when
 *     depth <= 16; the rows of the root and of nodes >= n are zero;
 *   triplet (B, N) int64 = 2 + min(depth, 15) * 64 + min(child_idx(parent), 7) * 8 + min(child_idx, 7) (the root's
 *     parent index is 0), 0 (PAD) for nodes >= n.
 * A NULL output pointer means that field is not built (its memory is not touched). Every parent value is range-checked
 * before it is used as an index. A malformed tree sets status[b] = 1 (else 0) and gets the fields of the empty tree:
 * planes 75, masks 1, adj 0, tree_pos 0, triplet PAD; the other ASTs of the batch are unaffected.
 * The planes may start at any byte address ((B, 2, N, N) buffers with N odd): aligned dword stores with byte stores at a
 * plane's two ends; each output byte is written exactly once. parents, num_node and status are 4-byte aligned, tree_pos
 * 16, triplet 8. Deterministic, no atomics, no allocation, no sync: capturable.
 * Supported: 1 <= N <= 3276 (20 bytes of tables per node within 64 KiB of LDS). The tables are set up by single lanes in
 * O(n) dependent LDS steps per AST. */
typedef struct csa_ast_batch_args {
  int64_t B, N;
  const int32_t* parents;    /* (B, N) */
  const int32_t* num_node;   /* (B) */
  uint8_t* L; uint8_t* T; uint8_t* L_mask; uint8_t* T_mask;   /* (B, N, N) each, or NULL */
  int64_t plane_sb;          /* batch stride of those four in bytes: 0 = N * N, 2 N * N = halves of (B, 2, N, N) buffers */
  uint8_t* adj;              /* (B, N, N) or NULL */
  float* tree_pos;           /* (B, N, 128) or NULL */
  int64_t* triplet;          /* (B, N) or NULL */
  int32_t* status;           /* (B) */
} csa_ast_batch_args;
int csa_ast_batch_supported(int64_t N);
csa_status csa_ast_batch(const csa_ast_batch_args* a, void* stream);

/* ---- v10 additions: the log-probability of one given token per row of logits (csrc/csa_score.hip) ----
 * Teacher-forced scoring without the (rows, V) log-probability tensor of log_softmax + gather. logits (rows, V) fp32
 * with a row stride ld >= V in elements (4-byte aligned; 16-byte loads where a row's base is 16-byte aligned), target
 * (rows) int64. With m_r = max_j z[r, j] and S_r = sum_j exp(z[r, j] - m_r), lse_r = m_r + log S_r:
 *   logp[r] = (z[r, t_r] - m_r) - log S_r, a true log-softmax at the target (never log of softmax: no underflow to
 *             -inf); a row whose target is ignore_id or lies outside [0, V) is "ignored" and gets logp = 0;
 *   lse[r]  = the pair {m_r, log S_r}, (rows, 2) fp32, written for every row, ignored ones included. It is kept as the
 *             unevaluated sum because one fp32 m + log S rounds at the size of m, which exp(z - lse) would turn into a
 *             relative error of the backward (5e-4 at |z| ~ 1e4).
 * -inf logits are legal and contribute 0 to S; a -inf target logit gives logp = -inf; a row that holds a NaN gives NaN;
 * a row of -inf alone gives NaN, as torch.log_softmax does; +inf logits are unspecified.
 * The backward writes dz[r, j] = g[r] * ([j == t_r] - exp((z[r, j] - m_r) - log S_r)), row stride dz_ld >= V; an
 * ignored row is written as zeros whatever g[r] holds, NaN included. dz MAY ALIAS logits (dz == logits with
 * dz_ld == ld: every element is read by the lane that writes it, before the write); any other overlap is not allowed.
 * Forward launch classes by V, one workgroup per row: register-resident rows of 512 lanes x NG groups of 8 columns for
 * V <= 4096 NG, NG = 1..6 (thresholds 4096, 8192, 12288, 16384, 20480, 24576), and a two-pass streaming kernel above
 * 24576. The backward is elementwise given lse: one workgroup per (row, 4096 columns), no classes.
 * Supported: 1 <= V <= 2^24 (csa_token_logp_supported). rows == 0 or V == 0 returns CSA_OK and launches nothing.
 * Deterministic (fixed reduction orders), no atomics, no allocation, no sync: capturable. */
int csa_token_logp_supported(int64_t V);
csa_status csa_token_logp_fwd(const float* logits, int64_t ld, const int64_t* target, int64_t rows, int64_t V,
                              int64_t ignore_id, float* logp, float* lse, void* stream);
csa_status csa_token_logp_bwd(const float* g, const float* logits, int64_t ld, const int64_t* target, const float* lse,
                              float* dz, int64_t dz_ld, int64_t rows, int64_t V, int64_t ignore_id, void* stream);

/* ---- v10 additions: full-sequence (teacher-forced) decoder attention, forward and backward (csrc/csa_seqattn.hip) ----
 *   out[r, i, h*hd : (h+1)*hd] = sum_j softmax_j(scale * q[r,h,i] . K[kb,h,j] + m(r,h,i,j)) * V[kb,h,j],  kb = r / kv_group
 * fp32 throughout. q is (R,H,T,hd) and K / V are (R / kv_group,H,S,hd) through their element strides, hd contiguous: the
 * strided views of a packed (B,T,3,H,hd) or (B,S,2,H,hd) projection are read in place; the kv_group query rows of an
 * AST read ONE K/V. out is (R,T,H*hd) contiguous, lse (R,H,T) the row log-sum-exp of the scaled, masked scores, saved
 * for the backward. m is -inf on a masked key and 0 elsewhere; key j is masked for query i of (r, h) when
 *   causal is set and j > i (causal requires S == T and kv_group == 1), or
 *   mask (optional uint8 rows of mask_ld >= S bytes) holds a non-zero byte at column j of row
 *     mask_mode 0: r / kv_group        (a (B,S) memory mask; with kv_group == 1 a row's own PAD columns)
 *     mask_mode 1: (r * H + h) % R     (the head-repeated target mask of the reference decode, DecodeCache.head_pad).
 * A query row whose keys are all masked gives NaN in out (0/0, as SDPA and the decode-step kernel) and lse = -inf; its
 * own gradients are unspecified, its contribution to dk / dv is exact zeros, and neither pass faults on it.
 * Backward: dout (R,T,H*hd) contiguous; dq, dk, dv are written through their own strides (hd contiguous), so they may
 * be slices of one packed gradient buffer. dk / dv have K / V's shape: the sum over the kv_group rows and the T queries
 * of an AST is taken inside the kernel, rows and query tiles in ascending order; a key that is masked for every query
 * gets exact zeros. workspace: the byte count the workspace query returns (rowsum(dout * out), (R,H,T) fp32).
 * Supported: hd in {8, 64}, 1 <= T <= 256, S >= 1, R * H * ceil(max(T, S) / 16) below 2^31; 16 x 16 tiles on
 * v_mfma_f32_16x16x4_f32, one wave per workgroup, one launch forward and two backward. Every pointer 16-byte aligned
 * (lse, workspace: 4), every stride a non-negative multiple of 4 elements. Deterministic (fixed summation orders, no
 * atomics), no allocation, no sync: capturable. */
typedef struct csa_seq_attn_args {
  int64_t R, H, T, S, hd, kv_group;
  const float* q; int64_t q_sr, q_sh, q_st;   /* (R,H,T,hd) */
  const float* k; int64_t k_sb, k_sh, k_sn;   /* (R / kv_group,H,S,hd) */
  const float* v; int64_t v_sb, v_sh, v_sn;
  const uint8_t* mask; int64_t mask_ld;       /* NULL, or rows of mask_ld >= S bytes */
  int32_t mask_mode, causal;
  float scale;                                /* hd^-0.5 */
  float* out;                                 /* (R,T,H*hd) contiguous */
  float* lse;                                 /* (R,H,T) */
} csa_seq_attn_args;

typedef struct csa_seq_attn_bwd_args {
  const csa_seq_attn_args* fwd;               /* the forward's arguments, out and lse as it wrote them */
  const float* dout;                          /* (R,T,H*hd) contiguous */
  float* dq; int64_t dq_sr, dq_sh, dq_st;
  float* dk; int64_t dk_sb, dk_sh, dk_sn;
  float* dv; int64_t dv_sb, dv_sh, dv_sn;
  void* workspace;
} csa_seq_attn_bwd_args;

int csa_seq_attn_supported(int64_t hd, int64_t T, int64_t S);
size_t csa_seq_attn_bwd_workspace_bytes(int64_t R, int64_t H, int64_t T);
csa_status csa_seq_attn_fwd(const csa_seq_attn_args* a, void* stream);
csa_status csa_seq_attn_bwd(const csa_seq_attn_bwd_args* b, void* stream);

/* ---- Linear bias gradient: db[c] (+)= sum_r dy[r, c], dy (rows, cols) contiguous fp32 ----
 * Two passes (row-slice partials into the caller's workspace, then a fixed-order sum): deterministic. */
size_t csa_bias_grad_workspace_bytes(int64_t rows, int64_t cols);
csa_status csa_bias_grad(const float* dy, float* db, int64_t rows, int64_t cols, int accumulate, void* workspace,
                         void* stream);

/* ---- LayerNorm over the last dim (nn.LayerNorm(cols), affine) of the encoder/decoder glue ----
 * x, y, dy, dx: (rows, cols) contiguous fp32, cols % 4 == 0 and cols <= 1024 (csa_layernorm_supported);
 * stats: (rows, 2) saved (mean, rstd). Backward writes dx, dgamma, dbeta (deterministic: fixed-order
 * column partials in the caller's workspace). */
int csa_layernorm_supported(int64_t cols);
size_t csa_layernorm_bwd_workspace_bytes(int64_t rows, int64_t cols);
csa_status csa_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats,
                             int64_t rows, int64_t cols, float eps, void* stream);
csa_status csa_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, float* dx,
                             float* dgamma, float* dbeta, int64_t rows, int64_t cols, void* workspace, void* stream);

/* ---- Residual + dropout of the pre-LN blocks (module/components.py SublayerConnection
 * `x + self.dropout(sublayer(self.norm(x)))`; module/sbm_model.py:29-31 `self.dropout1(out) + X` and
 * `self.mlpblock(self.norm2(X)) + X`, whose last mlpblock module is the Dropout) ----
 * x, o, y, dy, d_o: n fp32 elements in the same memory order, 16-byte aligned; 0 < p < 1.
 * y = x + keep * o / (1 - p); d_o = keep * dy / (1 - p) (the residual gradient is dy itself).
 * keep for element i: Philox4x32-7 stream 5 (oracle/philox.py:res_keep), regenerated by the backward.
 * All 64 bits of `seed` are the Philox key (low word, high word); the low 32 bits of `offset` enter the
 * last counter word as (5 << 28) ^ (uint32_t)offset, its high 32 bits are ignored
 * (tests/test_elementwise_train_gpu.py: distinct (seed, offset) pairs give distinct masks). */
csa_status csa_residual_dropout_fwd(const float* x, const float* o, float* y, int64_t n, float p, uint64_t seed,
                                    uint64_t offset, void* stream);
csa_status csa_residual_dropout_bwd(const float* dy, float* d_o, int64_t n, float p, uint64_t seed, uint64_t offset,
                                    void* stream);

/* ---- GELU + dropout of the feed-forward blocks (module/components.py FeedForward
 * `linear2(dropout(gelu(linear1(x))))`; module/sbm_model.py:22-26 mlpblock GELU -> Dropout) ----
 * h, y, dy, dh: n fp32 elements in the same memory order, 16-byte aligned; 0 <= p < 1.
 * y = keep * gelu(h) / (1 - p) (exact erf GELU); dh = keep * dy / (1 - p) * gelu'(h).
 * keep for element i: Philox4x32-7 stream 6 (oracle/philox.py:ffn_keep), regenerated by the backward.
 * Key and counter as above: all 64 bits of `seed`, (6 << 28) ^ (uint32_t)offset; p = 0 reads neither.
 * Non-finite h gives the IEEE value of these formulas: gelu(+inf) = +inf, gelu(-inf) = NaN, gelu'(+-inf) = NaN,
 * NaN stays NaN; a dropped element is 0 * value, so a dropped +inf is NaN as well. */
csa_status csa_gelu_dropout_fwd(const float* h, float* y, int64_t n, float p, uint64_t seed, uint64_t offset,
                                void* stream);
csa_status csa_gelu_dropout_bwd(const float* dy, const float* h, float* dh, int64_t n, float p, uint64_t seed,
                                uint64_t offset, void* stream);

/* ---- Host data path: AST relation planes (my_ast.py:198-273, dataset/base_data_set.py:33-36) ----
 * parent: (B, max_size) int32, pre-order ids (parent[v] < v, parent[0] = -1); n_nodes: (B,) int32
 * (trees longer than max_size are truncated to their pre-order prefix). Outputs (B, max_size,
 * max_size) uint8 host arrays: L / T = clamp(raw + 75, 0, 149), L_mask / T_mask = (raw == 0).
 * Runs on the host (nthreads std::threads); no HIP call. */
csa_status csa_ast_relations(const int32_t* parent, const int32_t* n_nodes, int64_t B, int64_t max_size, uint8_t* L,
                             uint8_t* T, uint8_t* L_mask, uint8_t* T_mask, int nthreads);

/* collect_fn's encoding (dataset/base_data_set.py:33-36) of raw fp32 relation matrices (any shape, n
 * elements, e.g. a stacked (B, N, N) batch of split_matrices.npz L / T): idx = clamp(raw + 75, 0, 149),
 * mask = (raw == 0). Host only; replaces the per-item torch.clamp / eq / stack of the reference. */
csa_status csa_collate_relations(const float* L_raw, const float* T_raw, int64_t n, uint8_t* L, uint8_t* T,
                                 uint8_t* L_mask, uint8_t* T_mask, int nthreads);

#ifdef __cplusplus
}
#endif
#endif /* CSA_HIP_H */
