/*
 * fira_hip.h — C ABI of libfira_hip.so: the MI355X (gfx950) compute path of the FIRA
 * commit-message model (GNN encoder + Transformer decoder with dual copy head).
 *
 * The reference (DJjjjhao/FIRA-ICSE) has no FFI: its hot path is a chain of stock PyTorch ops
 * (SURVEY.md §2.2).  Each entry point below replaces the reference lines cited next to it; a
 * binding (ctypes / cgo / JNI) only needs this header.  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller unless marked "host";
 *   - nothing allocates: scratch comes from the caller (fira_workspace_bytes);
 *   - work is enqueued on the hipStream_t passed as `void* stream` (NULL = default stream),
 *     nothing synchronises; distinct streams may be driven from distinct threads;
 *   - return 0 on success, non-zero on error (message: fira_last_error(), thread-local);
 *   - activations are row-major [rows, 256] fp32; nn.Linear weights are [out, in] row-major
 *     exactly as in the reference's state_dict; ids are int32.
 */
#ifndef FIRA_HIP_H
#define FIRA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIRA_ABI_VERSION 11

/* ---- model geometry: reference run_model.py:30-46 (args) ---------------------------------- */
typedef struct fira_dims {
    int32_t sou_len;         /* 210 code-token nodes                                   */
    int32_t sub_len;         /* 160 sub-token nodes                                    */
    int32_t ast_len;         /* 280 AST + edit-operation nodes                         */
    int32_t tar_len;         /* 30 message positions                                   */
    int32_t d_model;         /* 256 (kernels are specialised for 256)                  */
    int32_t n_head;          /* 8   (head width 32)                                    */
    int32_t n_layer;         /* 6                                                      */
    int32_t vocab;           /* 24650                                                  */
    int32_t ast_vocab;       /* 71                                                     */
    int32_t d_ff;            /* 1024                                                   */
} fira_dims;

/* ---- one collated batch of commits (replaces the 8-tensor batch of Dataset.py:336-343) ---- */
typedef struct fira_batch {
    int32_t B;               /* commits in the batch                                   */
    int32_t nnz;             /* entries of the block-diagonal adjacency                */
    const int32_t* sou;      /* [B, sou_len]  code-token ids                           */
    const int32_t* tar;      /* [B, tar_len]  decoder input ids                        */
    const int32_t* mark;     /* [B, sou_len]  0 pad,1 deleted,2 context,3 added (dense; the kernels read code_mark) */
    const int32_t* ast_change; /* [B, ast_len]                                         */
    const int32_t* tar_label;/* [B, tar_len]  labels incl. copy ids (>= vocab)         */
    const int32_t* sub_token;/* [B, sub_len]                                           */
    /* ---- computed node list.  The encoder only runs on the nodes listed here; padded nodes (id 0 and no edge but
     * their self-loop) may be left out: they are masked wherever they could be read and get zero gradient
     * (SURVEY.md §8a N1).  Listing every node (identity lists) reproduces the reference's dense computation. ---- */
    int32_t n_nodes;         /* Nc: computed nodes of the batch                                              */
    const int32_t* node_rows;/* [Nc] ascending global node index b*N + local (N = sou+sub+ast)               */
    const int32_t* rowptr;   /* [Nc + 1] CSR row offsets over the computed nodes                             */
    const int32_t* col;      /* [nnz] COMPACT node ids (position in node_rows)                               */
    const float*   val;      /* [nnz] D^-1/2 (A+I) D^-1/2 entries (fp32 of Dataset.py:291)                   */
    int32_t n_code;          /* Cc: computed code-token nodes (local < sou_len)                              */
    const int32_t* code_rows;/* [Cc] their compact ids, ASCENDING (v4: kernels invert the list by binary search)    */
    const int32_t* code_mark;/* [Cc] their mark value (0 pad,1 deleted,2 context,3 added)                    */
    int32_t n_mem;           /* Mc: computed memory nodes (local < sou_len + sub_len)                        */
    const int32_t* mem_rows; /* [Mc] their compact ids, ASCENDING                                            */
    const int32_t* mem_dst;  /* [Mc] their dense memory row b*(sou_len+sub_len) + local                      */
    const int32_t* head_rows;/* [n_head_rows] optional: flat (b*tar_len+t) indices of the target rows whose shifted
                                label is a vocabulary id (0 < label < vocab), ascending, no duplicates; only these
                                rows need the vocabulary GEMM in training.  NULL = all rows.           */
    int32_t n_head_rows;
    /* ---- optional (emb_items NULL = scatter with atomics per position): the code / sub-token positions of the batch
     * grouped by word id for the embedding gradient (gnn_transformer.py:46-52 backward).  Frequent tokens ('(' ';' ...)
     * occur hundreds of times per batch; one wave sums up to 32 positions of one id before touching the table row. */
    int32_t n_emb_items;
    const int32_t* emb_item_tok; /* [n_emb_items] word id of the item (never 0 = padding_idx); the items of one word
                                  * are ADJACENT (a word with a single item is written without atomics)           */
    const int32_t* emb_item_ptr; /* [n_emb_items + 1] offsets into emb_rows; at most 32 rows per item              */
    const int32_t* emb_rows;     /* COMPACT node ids (position in node_rows) of code / sub-token nodes, grouped by word id */
    /* ---- optional, together with emb_*: the computed AST / edit-operation nodes with a non-zero id, so that the whole
     * embedding gradient is taken from the compact node rows (no dense [B,650,256] scatter in the backward pass) */
    int32_t n_ast_items;
    const int32_t* ast_rows;     /* [n_ast_items] compact node ids                                               */
    const int32_t* ast_ids;      /* [n_ast_items] their ast_change ids (never 0)                                  */
    /* ---- optional (v5): computed TARGET rows.  The decoder of a training step only has to run on the positions that are
     * read by someone: position t of commit b matters as an attention key while tar[b,t] != 0 and as a loss row while the
     * shifted label tar_label[b,t+1] != 0 -- the padded tail (about 45 % of the B*30 rows on FIRA's data; it is computed by
     * the reference too, gnn_transformer.py:108-122, but carries zero loss weight, Model.py:82, and is masked as a key)
     * can be left out.  dec_off[b] .. dec_off[b+1] = the range of commit b's rows in the compact target-row layout; the
     * rows kept are the PREFIX t < dec_off[b+1] - dec_off[b] of its tar_len positions (so compact position == position,
     * causal order is preserved) and the prefix must cover every position with a non-zero id or shifted label.
     * NULL (or fira_train_opts.compact_dec == 0) = all B*tar_len rows. */
    const int32_t* dec_off;      /* [B + 1] ascending, dec_off[0] = 0, 1 <= dec_off[b+1] - dec_off[b] <= tar_len          */
    int32_t n_dec_rows;          /* dec_off[B]                                                                         */
    /* ---- optional (v8): a HOST copy of dec_off ([B + 1], host memory, valid for the duration of the call).  With it the
     * library may split the decoder's chain at a commit boundary into two commit-lanes on two streams (it needs the row
     * offset of that boundary on the host to size the launches); NULL = one lane.  Results do not depend on it. */
    const int32_t* dec_off_host;
} fira_batch;

typedef struct fira_train_opts {
    float    dropout;        /* 0.1 in the reference (Attention/FFN/Combination); 0 = off */
    float    gcn_dropout;    /* 0.2 (gnn_transformer.py:43)                             */
    uint64_t seed;           /* dropout stream seed; masks are re-derived in backward   */
    int32_t  compact_head;   /* 1 = run the vocabulary head only on rows whose label != 0 (results identical) */
    int32_t  dtype;          /* FIRA_F32 (reference arithmetic) or FIRA_BF16: nn.Linear products on the bf16 MFMA with
                                fp32 accumulation (operands rounded to bf16, everything stored in fp32) -- BASELINE
                                configs[2]; LayerNorm / soft-max / loss / Adam are fp32 in both modes           */
    int32_t  compact_dec;    /* (v5) 1 = run the decoder / output head on the rows of fira_batch.dec_off only: loss and
                                gradients are those of the dense run (only rows nobody reads are skipped); the dropout
                                element index of a decoder site is then (compact row) * 256 + column            */
    int32_t  zero_grads;     /* (v5) 1 = the call clears grads[0, live) itself, beside the encoder's forward pass on a
                                library-owned stream, instead of the caller filling 111 MB ahead of the step    */
} fira_train_opts;
#define FIRA_F32 0
#define FIRA_BF16 1
#define FIRA_F32X3 2      /* (v9, fira_gcn_layer_* and fira_combination_block_* only) fp32 data and accuracy, the product on the bf16 matrix cores: every operand as
                           * three bf16 terms hi + mid + lo, six of the nine term products, fp32 accumulation (see below)           */
#define FIRA_BF16X1 3     /* (v9, same entries) the engine's bf16 mode on the same machinery: ONE bf16 plane -- both operands rounded to
                           * bf16 once (RNE), fp32 accumulation; weight argument = the planes as for FIRA_F32X3                       */

const char* fira_last_error(void);
int         fira_abi_version(void);

/* ---- parameter layout: one flat fp32 buffer holding the 338 state-dict tensors ------------
 * (SURVEY.md §8b "Checkpoint").  Index order == reference state_dict order.                  */
int    fira_param_count(const fira_dims* d);
/* name_buf >= 128 bytes; shape has up to 2 entries (ndim returned). offset/numel in floats.  */
int    fira_param_info(const fira_dims* d, int index, char* name_buf, int64_t* offset, int64_t* numel,
                       int32_t* ndim, int64_t shape[2]);
int64_t fira_param_total(const fira_dims* d);            /* floats in the flat buffer        */
/* Gradient readiness groups of the flat buffer: [0, split) = output head + decoder (complete when the `mid` event of
 * fira_train_fwd_bwd fires), [split, live) = encoder, [live, total) = tensors no kernel touches. */
int    fira_param_groups(const fira_dims* d, int64_t* split, int64_t* live);

/* bytes of caller-provided scratch for a batch of B commits. mode: 0 = forward only, 1 = training */
size_t fira_workspace_bytes(const fira_dims* d, int B, int mode);
/* scratch for fira_decode_begin / fira_decode_step with n_beam hypotheses per commit */
size_t fira_decode_workspace_bytes(const fira_dims* d, int B, int n_beam);
/* (v6) the same for the flags fira_decode_begin_ex / fira_decode_step_ex will be called with: FIRA_DECODE_KV_BF16 adds the
 * bf16 copy of the cross-attention K|V (148 MB at batch 64); flags 0 == fira_decode_workspace_bytes */
size_t fira_decode_workspace_bytes_ex(const fira_dims* d, int B, int n_beam, int flags);

/* Per-kernel-class HIP-event profiling (bench.py's roofline leg).  Classes: 0 GEMM (work = FLOP), 1 CSR SpMM
 * (work = algorithmic bytes), 2 attention, 3 row ops, 4 copy score, 5 head/loss, 6 Adam (with clipping on: the sum of squares
 * of the gradient is booked here too).  report() synchronises,
 * returns per class the summed event time [ms], summed work and launch count since the last report, and resets. */
#define FIRA_PROF_NCLASS 7
/* two more classes are reported when n_class asks for them: 7 = the decoder's M = B*30 products (a sub-set of class 0's
 * launches, split out of it), 8 = the fused GCN-layer launches (work = FLOP of the product, bytes = algorithmic bytes) */
void fira_prof_enable(int on);
/* bytes (may be NULL): for the GEMM class, the algorithmic operand + result bytes 4*(M*K + N*K + M*N) of its launches */
int  fira_prof_report(int n_class, double* ms, double* work, double* bytes, int64_t* count);

/* =========================== op level (one reference op each) ============================== */

/* C[M,N] (+)= op(A)·op(B) (+ bias[n]) (relu).  Replaces every nn.Linear / its backward
 * (addmm/mm calls listed in SURVEY.md §2.3).  transA=0: A stored [M,K] (lda); transA=1: A stored
 * [K,M].  transB=1: B stored [N,K] (the nn.Linear weight layout); transB=0: B stored [K,N].
 * flags: bit0 relu, bit1 accumulate into C (C += ...), splitk >= 1 partitions K over grid.z (0 = automatic tile / split choice, what the fused entry points use)
 * (partials combined with fp32 atomics; requires accumulate semantics, C pre-initialised).     */
#define FIRA_GEMM_RELU 1
#define FIRA_GEMM_ACCUM 2
/* bits 4-5 (testing / tuning): force a tile: 0 auto, 1 128x128, 2 64x128, 3 64x64 */
#define FIRA_GEMM_TILE_SHIFT 4
int fira_gemm_f32(void* stream, int transA, int transB, int M, int N, int K,
                  const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                  const float* bias, int flags, int splitk);
/* The same product on the bf16 MFMA (v_mfma_f32_32x32x16_bf16): A and B are fp32 in memory, rounded to bf16
 * (nearest-even) while they are staged, accumulated and stored in fp32 -- torch.autocast(bfloat16) around F.linear.
 * Tile bits: 0 auto, 1 128x128, 2/3 64x64.  Products it does not take (M, N or K < 32, unaligned) run in fp32.   */
int fira_gemm_bf16(void* stream, int transA, int transB, int M, int N, int K,
                   const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                   const float* bias, int flags, int splitk);

/* bf16 weight shadows.  In bf16 mode the model-level entry points keep, inside the workspace, a bf16 copy of every 2-D
 * weight as stored ([out, in]) and transposed ([in, out]), refreshed by one launch per call: the forward product reads
 * the first, the data gradient the second -- both as the k-contiguous operand of the same kernel, at half the weight
 * bytes and without transposing loads.  Op-level forms of the two steps:
 *   fira_weight_shadow : Wb[rows, cols] = bf16(W), WbT[cols, rows] = bf16(W^T)                  (uint16_t = raw bf16)
 *   fira_gemm_bf16_wb  : C[M,N] (+)= A[M,K] (fp32, rounded while staged) . Bb[N,K]^T (+bias)(relu); ldb % 8 == 0      */
int fira_weight_shadow(void* stream, int rows, int cols, const float* W, uint16_t* Wb, uint16_t* WbT);
int fira_gemm_bf16_wb(void* stream, int M, int N, int K, const float* A, int lda, const uint16_t* Bb, int ldb,
                      float* C, int ldc, const float* bias, int flags, int splitk);

/* Y[r,:] = sum_j val[j] * X[col[j],:]  over CSR row r (d = 256).  The GCN aggregation
 * torch.bmm(edge.float(), x) (gnn_transformer.py:80); its backward is the same call because
 * the normalised adjacency is symmetric.  variant: 0 auto, 1 row gather (round 5: a wave owns four
 * consecutive rows and batches their index and neighbour-row requests), 2 LDS-staged (needs graph_rows > 0:
 * rows per graph, cols local to the graph's row block), 5 the round-1 gather, one row per wave (also what
 * variant 1 runs on feature matrices of 2 GiB and more). */
int fira_csr_spmm_f32(void* stream, int n_rows, const int32_t* rowptr, const int32_t* col, const float* val,
                      const float* X, int ldx, float* Y, int ldy, int graph_rows, int variant);
/* The same aggregation with the block-dense MFMA variants and the measured variant choice:
 *   3  block-dense, fp32 MFMA   (graph_rows <= 512; a workgroup densifies 32 rows of one graph's adjacency into LDS
 *                                and multiplies them with the graph's feature rows: the literal torch.bmm of
 *                                gnn_transformer.py:80, fp32 arithmetic)
 *   4  block-dense, bf16 MFMA   (A_hat and X rounded to bf16, fp32 accumulate: torch.autocast's bmm, FIRA_BF16 only)
 *   0  auto: by density nnz / (n_rows * graph_rows) -- row-per-wave CSR below the measured crossover, block-dense above
 *      (profiles/r3_spmm_crossover.md); dtype (FIRA_F32 | FIRA_BF16) says whether bf16 operands are allowed.
 * CSR rows must hold sorted column ids (equal neighbours are summed), as data.py builds them.                       */
int fira_csr_spmm(void* stream, int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const float* val,
                  const float* X, int ldx, float* Y, int ldy, int graph_rows, int variant, int dtype);

/* One GCN layer per launch (v6; reference gnn_transformer.py:74-86: fc1 -> torch.bmm(edge, x) -> fc2 -> dropout -> +x ->
 * LayerNorm).  There is no non-linearity between fc1, the aggregation and fc2, so the layer is evaluated in the folded form
 *     sum = dropout( (A_hat X) W21^T + b2 + (A_hat 1) c21^T ) + X ,   y = LayerNorm(sum)
 * with W21 = fc2.weight . fc1.weight [256,256] and c21 = fc2.weight . fc1.bias [256] formed by the caller; the forward
 * launch takes it TRANSPOSED (W21t = W21^T row-major, i.e. [in, out]: the kernel streams the weight k-major).  A workgroup
 * gathers 32 rows of A_hat X from the CSR adjacency into LDS, multiplies them with W21 on the MFMA (fp32 chains, or bf16
 * operands with fp32 accumulation for FIRA_BF16) and finishes the rows: the aggregated rows never travel through HBM.
 * CSR as for fira_csr_spmm_f32 (global column ids, sorted).  sum / y [n_rows,256], stats [n_rows,2] = {mean, 1/std} for
 * the backward LayerNorm; rowsum_out (optional) [n_rows] = A_hat 1; dropout element index = row*256 + col of `site`.
 *
 * Backward of the data path (A_hat symmetric):  V = A_hat dY ;  dX += V W21 ;  the weight gradient is dW21 = V^T X.
 * dY = gradient w.r.t. the un-dropped branch output (what fira_add_layernorm_bwd returns as dx_drop); W21 row-major
 * [out, in] (k-major for this product); V [n_rows,256] is written, dX [n_rows,256] is accumulated into.                  */
int fira_gcn_layer_fwd(void* stream, int n_rows, const int32_t* rowptr, const int32_t* col, const float* val,
                       const float* X, const float* W21t, const float* bias, const float* c21, const float* gamma,
                       const float* beta, float* sum, float* y, float* stats, float* rowsum_out, float dropout,
                       uint64_t seed, uint32_t site, int dtype);
int fira_gcn_layer_bwd(void* stream, int n_rows, const int32_t* rowptr, const int32_t* col, const float* val,
                       const float* dY, const float* W21, float* V, float* dX, int dtype);
/* (v9) dtype FIRA_F32X3 -- what the engine's fp32 mode runs: the gathered rows are split into three bf16 terms by the wave
 * that gathered them, the weight arrives pre-split: the weight argument (W21t / W21 above) is then the output of
 * fira_gcn_weight_planes for the matrix B [256 n][256 k] with  out = U B^T , i.e. B = W21 for fira_gcn_layer_fwd and
 * B = W21^T for fira_gcn_layer_bwd.  planes: n_mats x 3 x 65536 bf16 (hi | mid | lo plane, each in MFMA fragment order).
 * The result differs from the FIRA_F32 launch by fp32 rounding noise only (the dropped lo.lo, lo.mid, mid.lo terms are
 * below 2^-24 of a product).                                                                                           */
int fira_gcn_weight_planes(void* stream, int n_mats, const float* B, uint16_t* planes);
/* (v10) out [M, ldo] = x [M, 256] W^T + bias for N = a multiple of 256 output columns, W [N, 256] row-major given as the planes of
 * its N / 256 row blocks (fira_gcn_weight_planes(N / 256, W, planes)): the nn.Linear of the cross-attention K|V projection of all
 * layers on the encoder's memory rows (gnn_transformer.py:139-141; what fira_train_step runs on its auxiliary stream).
 * dtype FIRA_F32X3: three bf16 terms per operand (fp32-accurate); FIRA_BF16X1: both operands rounded to bf16 once.            */
int fira_linear_x3(void* stream, int M, int N, const float* x, int ldx, const uint16_t* w_planes, const float* bias, float* out,
                   int ldo, int dtype);
/* ... and its data gradient: dx [M, lddx >= 256] (+)= dy [M, K] W for W [K, 256] row-major with K a multiple of 256 (the d-memory
 * products of the decoder's backward pass, K = 1024 per layer pair).  wt_planes: the planes of the TRANSPOSED [256, 256] row
 * blocks of W (block kb transposed, then fira_gcn_weight_planes), K / 256 of them.                                           */
int fira_linear_dgrad_x3(void* stream, int M, int K, const float* dy, int lddy, const uint16_t* wt_planes, float* dx, int lddx,
                         int accumulate, int dtype);
/* (v10) The generator projection's data gradient (Model.py:54 backward): dx [M, lddx >= 256] += dy [M, K] W for W [K, 256], K ANY
 * size (the vocabulary; dy's row pitch lddy >= K, a multiple of 4 floats; columns past K are never read as operands).  The
 * reduction is split over workgroups and summed with float atomics: dx must hold what the product is added to (zeros for the
 * plain product).  planes_ws: fira_dgrad_x3_splitk_planes_bytes(K) bytes of scratch (the planes of W's transposed row blocks,
 * written by the call).  dtype FIRA_F32X3 | FIRA_BF16X1.                                                                     */
size_t fira_dgrad_x3_splitk_planes_bytes(int K);
int fira_dgrad_x3_splitk(void* stream, int M, int K, const float* dy, int lddy, const float* W, uint16_t* planes_ws, float* dx,
                         int lddx, int dtype);
/* The same for fira_combination_block_{fwd,bwd} with dtype FIRA_F32X3: the forward launch takes, in its WqT argument, the planes
 * of the THREE stacked matrices Wq | Wk | Wo as nn.Linear stores them ([out][in]; WkT / WoT are then ignored, pass WqT again);
 * the backward launch takes, in its Wo argument, the planes of Wq^T | Wk^T | Wo^T (Wqk is then ignored).                      */

/* One Combination block (gnn_transformer.py:176-205 with combination_layer.py:7-17) on n_rows code rows as ONE launch
 * (round 5, csrc/comb_fused.hip; dtype FIRA_F32, or FIRA_BF16 = the operands of the three products rounded to bf16, fp32
 * accumulation and storage):
 *     q | k = Xc [Wq | Wk]^T + bqk ;   c = dropout_gate( g0 k + g1 vtab[mark] ),  (g0, g1) = softmax(q k / sqrt 32, q v / sqrt 32)
 *     sum   = dropout_out( c Wo^T + bo ) + Xc ;   y[y_rows[r]] = LayerNorm(sum[r]) ;   stats[r] = {mean, 1/std}
 * WqT / WkT / WoT are the three nn.Linear weights TRANSPOSED ([256 in][256 out], contiguous): the kernel streams them
 * k-major.  vtab: the value projection of the 4-row mark table, row m at vtab + m*ldv.  q|k [n_rows,512] and c [n_rows,256]
 * are stored for the backward pass (fira_combination_bwd reads q|k).  y_rows (optional): output row map (the code rows of
 * the node buffer); dropout element index = row*256 + col under site_gate / site_out (the masks fira_combination_fwd /
 * fira_add_layernorm_fwd draw).                                                                                          */
int fira_combination_block_fwd(void* stream, int n_rows, const float* Xc, const float* WqT, const float* WkT,
                               const float* WoT, const float* bqk, const float* bo, const float* vtab, int ldv,
                               const int32_t* mark, float* qk, float* c, const float* gamma, const float* beta, float* sum,
                               float* y, const int32_t* y_rows, float* stats, float dropout, uint64_t seed,
                               uint32_t site_gate, uint32_t site_out, int dtype);

/* Backward of the block, one launch + one reduction launch: with dy = dG[rows[r]] (the gradient w.r.t. the block's output rows)
 *     ds = LayerNorm'(dy; sum, stats, gamma) ;  dYc = ds * mask_out ;  dc = dYc Wo ;  (dq, dk, dv) = gate'(q, k, vtab[mark], dc * mask_gate)
 *     dG[rows[r]] = ds + dq Wq + dk Wk
 * Wo [256,256] and Wqk [512,256] as nn.Linear stores them.  Written: dYc [n_rows,256] and dqk [n_rows,512] (the operands of the
 * weight gradients dWo = dYc^T c, dWqk = dqk^T Xc); accumulated into: dgamma, dbeta [256], dvtab (row m at dvtab + m*lddv).
 * part: scratch of fira_combination_block_bwd_part_floats() floats.                                                       */
int fira_combination_block_bwd(void* stream, int n_rows, float* dG, const int32_t* rows, const float* sum, const float* stats,
                               const float* gamma, const float* Wo, const float* Wqk, const float* qk, const float* vtab,
                               int ldv, const int32_t* mark, float* dYc, float* dqk, float* dgamma, float* dbeta,
                               float* dvtab, int lddv, float* part, float dropout, uint64_t seed, uint32_t site_gate,
                               uint32_t site_out, int dtype);
int fira_combination_block_bwd_part_floats(void);

/* out[(b*out_bstride + out_off + i), :] = table[idx[b*L + i], :] (+ pos[i,:])  — the embedding
 * gathers of gnn_transformer.py:46-52,110-113 written straight into the node buffer.           */
int fira_embed_gather_fwd(void* stream, int B, int L, const int32_t* idx, const float* table,
                          const float* pos, float* out, int out_bstride, int out_off);
/* dtable[idx,:] += dout[row,:]  (rows with idx == padding_idx skipped; padding_idx < 0: none) */
int fira_embed_gather_bwd(void* stream, int B, int L, const int32_t* idx, float* dtable,
                          const float* dout, int out_bstride, int out_off, int padding_idx);

/* CombinationLayer (combination_layer.py:7-17): c = softmax2(q*k/s, q*v/s) . (k, v), s = sqrt(32),
 * v = vtab[mark[row]] (vtab = linear_layers[2] applied to the 4-row mark table).  qk: [M,512] = [q|k]. */
int fira_combination_fwd(void* stream, int M, const float* qk, const float* vtab, const int32_t* mark,
                         float* out, float dropout, uint64_t seed, uint32_t stream_id);
int fira_combination_bwd(void* stream, int M, const float* qk, const float* vtab, const int32_t* mark,
                         const float* dout, float* dqk, float* dvtab /* [4,256] += */,
                         float dropout, uint64_t seed, uint32_t stream_id);

/* y = LayerNorm(dropout(x) + res) * gamma + beta  (eps 1e-5), rows of 256.  x is overwritten with the
 * pre-norm sum (kept for backward); stats[row] = {mean, rstd}.  Post-LN residual blocks of
 * gnn_transformer.py:86,161,174,205.                                                            */
int fira_add_layernorm_fwd(void* stream, int M, float* x, const float* res, const float* gamma,
                           const float* beta, float* y, float* stats, float dropout, uint64_t seed,
                           uint32_t stream_id);
/* A post-LN residual block split at its LayerNorm (gnn_transformer.py:161,174): the closing product stores the PRE-NORM sum
 *     sum[M,256] = dropout(X W^T + bias) + res          X [M,K] (row pitch ldx), W [256,K], K in {128..1024 step 128}
 * (what fira_add_layernorm_fwd forms from the plain product; same dropout element indices), and the product that consumes the
 * block's output normalises its A rows itself:
 *     Y[M,N] = LN(S) W^T + bias (+relu)                 S [M,256] (row pitch lds), W [N,256];  x_out [M,256] = LN(S) and
 *                                                       stats_out [M,2] = {mean, rstd} are stored as well
 * -- one launch less per block on the dependent chain than product + row kernel + product.  fp32 MFMA, operands 16-byte
 * aligned; returns an error for shapes the coalesced tile kernel does not take (the engine then uses the three launches). */
int fira_linear_presum_f32(void* stream, int M, int K, const float* X, int ldx, const float* W, const float* bias,
                           const float* res, float* sum, float dropout, uint64_t seed, uint32_t stream_id);
int fira_ln_linear_f32(void* stream, int M, int N, const float* S, int lds, const float* W, const float* bias, float* Y,
                       int ldy, int relu, const float* gamma, const float* beta, float* x_out, float* stats_out);
/* (v6) The LayerNorm BACKWARD of such a block inside the data-gradient product that consumes it (the decoder's backward
 * chain: gnn_transformer.py:161,174 backward followed by the closing nn.Linear's data gradient): with dy [M,256] the
 * gradient w.r.t. the block's output, sum / stats the saved pre-norm rows and {mean, 1/std},
 *     ds = LayerNorm'(dy)  [M,256]   (gradient w.r.t. the pre-norm sum = the residual-branch gradient; must not alias dy)
 *     dx_drop = ds * dropout mask of `site`            (the weight gradient's operand)
 *     dX[M,N] = dx_drop . Wt   (Wt row-major [256, N] = the closing nn.Linear's weight [256 out, N in]; relu_mask [M,N]
 *                               optional: dX zeroed where mask <= 0 -- the FFN's ReLU backward)
 *     dgamma / dbeta [256] += column sums (through `part`, caller scratch of ceil(M/32) * 512 floats).                    */
int fira_ln_bwd_linear_f32(void* stream, int M, int N, const float* dy, const float* Wt, float* dX, const float* relu_mask,
                           const float* sum, const float* stats, const float* gamma, float* ds, float* dx_drop,
                           float* dgamma, float* dbeta, float* part, float dropout, uint64_t seed, uint32_t site);
/* bf16 mode twin (K = 256): Wb is the [256,256] bf16 shadow of the weight (fira_weight_shadow), row pitch ldb a multiple
 * of 8; X is rounded to bf16 while staged, fp32 accumulation, fp32 LayerNorm.  M >= 64.                                  */
int fira_linear_layernorm_bf16_fwd(void* stream, int M, const float* X, int ldx, const uint16_t* Wb, int ldb,
                                   const float* bias, const float* res, const float* gamma, const float* beta,
                                   float* sum, float* y, float* stats, float dropout, uint64_t seed,
                                   uint32_t stream_id);
/* ds = dLN/d(sum); dgamma/dbeta += ...;  if dx_drop != NULL: dx_drop = ds * mask/(1-p)           */
int fira_add_layernorm_bwd(void* stream, int M, const float* dy, const float* sum, const float* stats,
                           const float* gamma, float* ds, float* dx_drop, float* dgamma, float* dbeta,
                           float dropout, uint64_t seed, uint32_t stream_id);

/* Dropout is counter-based: the keep/scale factor of element `idx` of a dropout site is a pure function of
 * (seed, site, idx), re-derived in the backward kernels (no mask tensors).  Sites of the model-level entry points:
 * FIRA_SITE(layer, kind); idx = row * 256 + column with `row` the kernel's own row index: the position in
 * fira_batch.code_rows for the two Combination sites, the compact node id for the GCN site, b*tar_len + t for the
 * decoder sites.  fira_dropout_mask writes out[i] = 0 or 1/(1-p) for idx = 0..n-1 (all 1 when p == 0): the hook that
 * lets a CPU restatement of the model run with the SAME masks (tests/test_dropout_gpu.py).
 * Reference sites: combination_layer.py:15-16, gnn_transformer.py:205 (Combination), :83 (GCN), :161 (both
 * attentions), :174 (FeedForward).                                                                               */
#define FIRA_SITE_GATE 0      /* dropout on the gated mix inside the Combination      */
#define FIRA_SITE_COMB_OUT 1  /* on the Combination's output projection               */
#define FIRA_SITE_GCN 2       /* on the GCN's fc2 output (p = gcn_dropout)            */
#define FIRA_SITE_SELF 3      /* on the self-attention output projection              */
#define FIRA_SITE_CROSS 4     /* on the cross-attention output projection             */
#define FIRA_SITE_FFN 5       /* on the feed-forward output                           */
#define FIRA_SITE(layer, kind) ((uint32_t)((layer) * 8 + (kind) + 1))
int fira_dropout_mask(void* stream, uint64_t seed, uint32_t site, int64_t n, float p, float* out);

/* colsum[n] += sum_m X[m,n]  (bias gradients) */
int fira_colsum_f32(void* stream, int M, int N, const float* X, int ldx, float* out);

/* Multi-head attention core of gnn_transformer.py:137-158 (head width 32): per (b, head)
 * O = softmax(mask(Q K^T / sqrt(32), -1e9)) V.  Q rows [B*Tq, ldq], K/V rows [B*Tk, ldk/ldv]; head h at
 * columns h*32.. ; key_valid [B,Tk] (0 = masked); causal != 0 adds key <= query + q_pos0.        */
int fira_attention_fwd(void* stream, int B, int H, int Tq, int Tk, const float* Q, int ldq,
                       const float* K, int ldk, const float* V, int ldv, const int32_t* key_valid,
                       int causal, int q_pos0, float* O, int ldo);
int fira_attention_bwd(void* stream, int B, int H, int Tq, int Tk, const float* Q, int ldq,
                       const float* K, int ldk, const float* V, int ldv, const int32_t* key_valid,
                       int causal, int q_pos0, const float* O, int ldo, const float* dO, int lddo,
                       float* dQ, int lddq, float* dK, int lddk, float* dV, int lddv);
/* Precondition of all attention entry points: every (batch entry, query) sees at least ONE unmasked key.  The reference's
 * masked_fill(-1e9) + softmax would then average V uniformly over ALL Tk keys, masked ones included; the kernels never read
 * rows of masked keys, so an all-masked row returns 0 instead (FIRA batches cannot produce one: position 0 of every
 * commit is its <start> token, Dataset.py:140, and a causal query always sees itself).
 * The forms the engine calls (v5, k_off: v6):
 *   q_off  (optional, [B+1]) ragged query rows: batch entry b's queries are rows q_off[b] .. q_off[b+1] of Q / O / dO /
 *          dQ (at most Tq of them: the decoder's computed target rows, fira_batch.dec_off); self_kv != 0: its keys and
 *          values are the same rows of K / V / dK / dV (self-attention).  key_valid stays dense [B, Tk].
 *   k_off  (optional, [B+1], not with self_kv) ragged KEY rows: batch entry b's keys / values are rows k_off[b] ..
 *          k_off[b+1] of K / V / dK / dV (at most Tk of them) and key_valid is indexed by the same compact rows
 *          (key_valid[k_off[b] + i]).  The engine keeps the cross-attention K|V of the COMPUTED memory rows only
 *          (fira_batch.mem_rows: ~47 % of the B*370 slots), in that layout -- the padded slots of the reference's
 *          [B,370] memory (Model.py:48,61) are masked keys whose soft-max weight is exactly 0.
 *   dtype  FIRA_BF16: the operands of the four matmuls (Q K^T, P V and their gradients) are rounded to bf16 and
 *          multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; scaling, mask, soft-max in fp32 -- what
 *          torch.autocast does to Attention.forward (gnn_transformer.py:149-156).  FIRA_F32: exact fp32 MFMA chains. */
int fira_attention_fwd_ex(void* stream, int B, int H, int Tq, int Tk, const float* Q, int ldq,
                          const float* K, int ldk, const float* V, int ldv, const int32_t* key_valid,
                          int causal, int q_pos0, float* O, int ldo, const int32_t* q_off, int self_kv, int dtype,
                          const int32_t* k_off);
int fira_attention_bwd_ex(void* stream, int B, int H, int Tq, int Tk, const float* Q, int ldq,
                          const float* K, int ldk, const float* V, int ldv, const int32_t* key_valid,
                          int causal, int q_pos0, const float* O, int ldo, const float* dO, int lddo,
                          float* dQ, int lddq, float* dK, int lddk, float* dV, int lddv,
                          const int32_t* q_off, int self_kv, int dtype, const int32_t* k_off);

/* Attention of ONE query per row (the K/V-cached decode step of run_model.py:256): O[b, h*32..] = softmax(q.K^T/sqrt(32)
 * over the valid keys) V.  Row b uses K/V batch entry b / qpk (kb rows of ldk floats per entry; key_valid [BR/qpk, kvb]):
 * the qpk beam rows of a commit share its memory.  Masked keys are never read.  Knew / Vnew (optional, qpk == 1): row b's
 * key / value number Tk-1 is taken from Knew[b*ldn..] / Vnew[b*ldn..] (the merged q|k|v projection's output) and is
 * appended to Kc_out / Vc_out (same geometry as K / V) for the later steps.  k_off (v6, optional, [BR/qpk + 1], not
 * with Knew): ragged key rows as in fira_attention_fwd_ex -- entry e's keys are rows k_off[e] .. k_off[e+1] of K / V and
 * key_valid is indexed by the same rows (kb / kvb are then ignored).                                                 */
int fira_decode_attention(void* stream, int BR, int H, int Tk, const float* Q, int ldq, const float* K, int ldk,
                          const float* V, int ldv, const int32_t* key_valid, float* O, int ldo, int kb, int kvb, int qpk,
                          const float* Knew, const float* Vnew, int ldn, float* Kc_out, float* Vc_out,
                          const int32_t* k_off);

/* CopyNet score (Model.py:15-18): score[b,t,s] = w . tanh(src[b,s,:] + tgt[b,t,:]) + bias, never
 * materialising the [B,T,S,256] tensor.  bwd re-computes tanh.                                   */
int fira_copy_score_fwd(void* stream, int B, int T, int S, const float* src, const float* tgt,
                        const float* w, const float* bias, float* score);
int fira_copy_score_bwd(void* stream, int B, int T, int S, const float* src, const float* tgt,
                        const float* w, const float* dscore, float* dsrc /* = */, float* dtgt /* += */,
                        float* dw /* += */, float* dbias /* += */);

/* Output head + loss (Model.py:54-86), one workgroup per target row bt = b*T + t (BT rows):
 * p = [g0*softmax(logits) ; g1*softmax(mask(score,-1e9))], loss = -log(clamp(p[label],1e-10,1)),
 * label = tar_label shifted left (Model.py:71-77).  compact_row[bt] = row of `logits` holding (b,t), or -1
 * when that row was not computed (NULL = identity).  loss_sum / n_tok are device scalars (+=).  With
 * want_grad the three inputs are overwritten in place by dlogits / dscore / dgate_logits.  With
 * argmax_out != NULL the teacher-forced argmax id of every row is written ('dev' stage, Model.py:85-86). */
int fira_head_loss(void* stream, int BT, int T, int V, int S, const int32_t* compact_row,
                   float* logits, int ldl, float* score /* [BT,S] */, const int32_t* mem_valid /* [B,S] */,
                   float* gate_logits /* [BT,2] */, const int32_t* tar_label /* [B,T] */,
                   float* loss_sum, int32_t* n_tok, int32_t* argmax_out, int want_grad);

/* (v11) The forms of the copy head and the loss that the engine calls (test surface: the same launches, no other kernel):
 *   qpk       (>= 1, divides B) qpk consecutive target batches share one memory: row b reads src / mem_valid entry b / qpk
 *             (the decode step: T = 1, qpk = hypotheses per commit).
 *   mem_valid (optional, [B/qpk, S] forward, [B, S] backward) key mask of the memory slots.  Forward: a masked slot is not
 *             computed, its score is stored as exactly 0 (fira_head_loss replaces it by -1e9).  Backward: dscore of a masked
 *             slot is never read as a gradient (masked_fill passes none) and its dsrc row is exactly 0.
 *   tar_label (optional, [B, T] dense, with V = vocabulary size) training: only the rows t whose shifted label
 *             tar_label[b, t+1] is a copy id (>= V) are computed.  Every other row is left UNWRITTEN, except that masked
 *             slots are still stored as 0 by the workgroups that own a copy row; a commit without any copy label is not
 *             touched at all.  fira_head_loss neither reads nor propagates the unwritten rows: with want_grad it
 *             overwrites all of them with their (zero) gradient.
 *   t_off     (optional, [B+1]) ragged target rows: commit b's rows are t_off[b] .. t_off[b+1] of tgt / score / dscore / dtgt
 *             (at most T of them, position t = row - t_off[b]; fira_batch.dec_off); labels stay dense [B, T].  Rows past
 *             t_off[B] are never touched.
 *   part      (optional, [fira_copy_score_bwd_blocks(B, S), fira_copy_part_stride()] floats) the backward stores one partial
 *             row {dw[256] | dbias} per workgroup -- every row is written, those of all-zero tiles as zeros -- instead of
 *             adding to dw / dbias (which are then not touched and may be NULL); fira_deferred_reduce sums the rows.
 *   row_bt    (optional, [BT]) fira_head_loss on BT computed target rows: row r of score / gate_logits / compact_row is the
 *             flat position row_bt[r] = b*T + t (NULL: r itself).                                                        */
int fira_copy_score_fwd_ex(void* stream, int B, int T, int S, const float* src, const float* tgt, const float* w,
                           const float* bias, float* score, int qpk, const int32_t* mem_valid, const int32_t* tar_label,
                           int V, const int32_t* t_off);
int fira_copy_score_bwd_ex(void* stream, int B, int T, int S, const float* src, const float* tgt, const float* w,
                           const float* dscore, float* dsrc /* = */, float* dtgt /* += */, float* dw /* += */,
                           float* dbias /* += */, const int32_t* mem_valid, float* part, const int32_t* t_off);
int fira_copy_score_bwd_blocks(int B, int S);   /* workgroups (= partial rows) of the backward launch; negative on bad sizes */
int fira_copy_part_stride(void);                /* floats between two partial rows (>= 257)                                  */
int fira_head_loss_ex(void* stream, int BT, int T, int V, int S, const int32_t* compact_row, float* logits, int ldl,
                      float* score, const int32_t* mem_valid, float* gate_logits, const int32_t* tar_label,
                      float* loss_sum, int32_t* n_tok, int32_t* argmax_out, int want_grad, const int32_t* row_bt);

/* (v11) The row kernels of the training step's tail, as the engine calls them (test surface, same launches):
 *   fira_deferred_reduce     dst[c] += sum_p src[p * stride + c], c < width, p < n_part, for n <= fira_deferred_reduce_max()
 *                            entries in ONE launch (`entries` is a HOST array, read during the call): the sums of the partial
 *                            rows that the backward kernels park per workgroup (LayerNorm gamma / beta, the copy head's w / bias).
 *   fira_rows_move           W floats (a multiple of 256) of each of R rows, rows ld_out / ld_in floats apart (a column block of
 *                            a wider matrix; multiples of 4):  mode 0 out[r] = in[src[r]] (src NULL: identity), 1 out[dst[r]] = in[r],
 *                            2 out[dst[r]] += in[r], 3 out[dst[r]] = in[src[r]].  dst holds no duplicates (plain stores).
 *   fira_rank2_rows          out[M,256] = g[M,2] w[2,256]: the data gradient of the 2-way copy gate (Model.py:19).
 *   fira_colsum_weighted     out[n] += sum_m row_weight[m] * X[m,n]  (row_weight NULL: all 1; X rows ldx floats apart).
 *   fira_embed_rows_fwd/bwd  the decoder's token embedding on computed target rows: compact row r is the flat position
 *                            row_bt[r] = b*T + t;  out[r] = table[idx[row_bt[r]]] + pos[t] ;  dtable[idx[row_bt[r]]] += dout[r]
 *                            (rows whose id is padding_idx skipped).  The table is read as stored (no row-sparse Adam view).
 *   fira_embed_grouped_bwd   dtable[item_tok[i]] += sum of the rows rows[item_ptr[i] .. item_ptr[i+1]) of dnode [*,256], one
 *                            wave per item (fira_batch.emb_*: at most 32 rows per item -- more than 64 are NOT summed -- and the
 *                            items of one word ADJACENT: a word with a single item is written without atomics).
 *   fira_embed_list_bwd_small   dtable[ids[k]] += dnode[rows[k]] for k < n, ids in [0, table_rows) (fira_batch.ast_*).
 *   fira_embed_gather_bwd_small fira_embed_gather_bwd for a table of table_rows rows that fits LDS (<= 150 rows).             */
typedef struct fira_red_entry {
    float*       dst;        /* [width]  accumulated into                      */
    const float* src;        /* [n_part, stride] partial rows                  */
    int32_t      width, n_part, stride;
} fira_red_entry;
int fira_deferred_reduce_max(void);
int fira_deferred_reduce(void* stream, int n, const fira_red_entry* entries /* host */);
int fira_rows_move(void* stream, int mode, int R, int W, float* out, int ld_out, const float* in, int ld_in,
                   const int32_t* src, const int32_t* dst);
int fira_rank2_rows(void* stream, int M, const float* g, const float* w, float* out);
int fira_colsum_weighted(void* stream, int M, int N, const float* X, int ldx, float* out, const float* row_weight);
int fira_embed_rows_fwd(void* stream, int R, int T, const int32_t* row_bt, const int32_t* idx, const float* table,
                        const float* pos, float* out);
int fira_embed_rows_bwd(void* stream, int R, const int32_t* row_bt, const int32_t* idx, float* dtable, const float* dout,
                        int padding_idx);
int fira_embed_grouped_bwd(void* stream, int n_items, const int32_t* item_tok, const int32_t* item_ptr, const int32_t* rows,
                           float* dtable, const float* dnode);
int fira_embed_list_bwd_small(void* stream, int n, const int32_t* rows, const int32_t* ids, float* dtable, const float* dnode,
                              int table_rows);
int fira_embed_gather_bwd_small(void* stream, int B, int L, const int32_t* idx, float* dtable, const float* dout,
                                int out_bstride, int out_off, int padding_idx, int table_rows);

/* Adam (run_model.py:396 torch.optim.Adam defaults) over a flat buffer.  grad_scale (device scalar,
 * may be NULL) multiplies g first: 1/n_tok of run_model.py:105 without a host sync.              */
int fira_adam_step(void* stream, int64_t n, float* p, const float* g, float* m, float* v,
                   float lr, float beta1, float beta2, float eps, int step, const float* inv_scale_ntok);
/* Adam for a step whose batch ran as one or two micro-batches: g = g0 (+ g1, may be NULL), each the gradient of the
 * micro-batch's loss SUM; the normaliser 1 / max(n_tok0 (+ n_tok1), 1) of run_model.py:105 is formed inside the kernel
 * from the device token counters.                                                                                  */
int fira_adam_step_mb(void* stream, int64_t n, float* p, const float* g0, const float* g1, float* m, float* v,
                      float lr, float beta1, float beta2, float eps, int step, const int32_t* n_tok0,
                      const int32_t* n_tok1);
/* Data-parallel form (run_model.py:105 over the GLOBAL batch): `count` is a device float holding the all-reduced token count;
 * the gradient is scaled by 1 / max(count, 1) inside the kernel -- no reciprocal / clamp launches between the collective and
 * the update.  fira_pack_stats writes the pair a rank contributes to that collective: out2 = {loss_sum, (float) n_tok}.  */
int fira_adam_step_count(void* stream, int64_t n, float* p, const float* g, float* m, float* v,
                         float lr, float beta1, float beta2, float eps, int step, const float* count);
int fira_pack_stats(void* stream, const float* loss_sum, const int32_t* n_tok, float* out2);
/* out[0] = 1 / max(n_tok[0], 1) on the device */
int fira_inv_count(void* stream, const int32_t* n_tok, float* out);

/* measurement aid: n dependent tiny kernels on `stream`, optionally forking the library's side stream after each (mode 1),
 * recording an event only (mode 2) or forking every 8th kernel (mode 3); scratch: >= 128 floats                       */
int fira_debug_chain(void* stream, int n, int mode, float* scratch);

/* =========================== model level (one call per step) =============================== */

/* forward + backward of TransModel.forward(..., 'train') (Model.py:38-84, run_model.py:104-108):
 * grads (flat, same layout as params) += d(loss_sum)/dparams; loss_sum / n_tok are device scalars
 * that are overwritten.  A fresh gradient: zero grads[0, live) first, or set opts->zero_grads and the
 * call clears it itself (beside the encoder's forward pass, on a library-owned stream).            */
int fira_train_fwd_bwd(void* stream, const fira_dims* d, const fira_batch* batch, const float* params,
                       float* grads, void* workspace, size_t workspace_bytes, const fira_train_opts* opts,
                       float* loss_sum, int32_t* n_tok, void* mid_event);
/* mid_event: optional hipEvent_t recorded on `stream` once the gradients of group [0, split) are final (after the
 * decoder backward, before the encoder backward), so that their RCCL all-reduce can overlap the rest.           */

/* (v8) Weight gradient as a panel product on the bf16 matrix cores (csrc/gemm_wgrad_panel.hip):
 *     C[M,N] += A^T B ;  colsum[m] += sum_k A[k][m]  (optional: the bias gradient)       A [K, lda], B [K, ldb] row-major
 * i.e. dW += dY^T X, db += column sums of dY for an nn.Linear with dY = A, X = B.  One workgroup owns a 256 x 256 tile of C
 * for a slab of K; every operand element is read once per tile.  dtype FIRA_BF16: operands rounded to bf16 (RNE), fp32
 * accumulation; FIRA_F32: every operand split into three bf16 terms, six exact term products per fp32 product -- fp32-accurate
 * (error of the order of 2^-24 of |a||b| per term, tests/test_ops_gpu.py) at 2.7x the fp32 MFMA rate.  Shapes: M >= 32,
 * N a multiple of 256, lda / ldb even, A / B 8-byte aligned, K * ld * 4 < 2 GiB.  C is accumulated into (no atomics: a
 * workgroup owns its tile).  scratch (optional, scratch_floats >= 65 536 per workgroup of a split product): lets K be split
 * into slabs over the chip -- the slabs' partial tiles go there and a closing launch adds them to C; NULL = one slab. */
int fira_gemm_wgrad_panel(void* stream, int dtype, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                          float* C, int ldc, float* colsum, float* scratch, size_t scratch_floats);

/* (v8) FeedForward block of a decoder layer (gnn_transformer.py:163-174) as one entry (two products + the row kernel, or the
 * LayerNorm-prologue forms, chosen as in the model-level calls):
 *     h = relu(x W1^T + b1) [M,F] ;  sum = dropout(h W2^T + b2) + x ;  y = LayerNorm(sum) ;  stats = {mean, 1/std}
 * w1 [F,256], w2 [256,F] as nn.Linear stores them; dropout element index = row*256 + col of `site`.  Backward: dy = gradient
 * w.r.t. y; dx [M,256] is written (must not alias dy); dw1 / db1 / dw2 / db2 / dgamma / dbeta are accumulated into; dyf_ws
 * [M,256] and dh_ws [M,F] are scratch.  dtype FIRA_F32 | FIRA_BF16 (operands of the products rounded, fp32 accumulate). */
int fira_ffn_fwd(void* stream, int M, int F, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                 const float* gamma, const float* beta, float* h, float* sum, float* y, float* stats, float dropout,
                 uint64_t seed, uint32_t site, int dtype);
int fira_ffn_bwd(void* stream, int M, int F, const float* dy, const float* x, const float* h, const float* sum,
                 const float* stats, const float* w1, const float* w2, const float* gamma, float* dx, float* dyf_ws,
                 float* dh_ws, float* dw1, float* db1, float* dw2, float* db2, float* dgamma, float* dbeta, float dropout,
                 uint64_t seed, uint32_t site, int dtype);
/* (v8) Output head + arg-top-k (Model.py:54,85; the candidate ranking of run_model.py:305 restricted to the generator):
 * logits_ws [R, ldl >= V] = x [R,256] Wout^T + bout; ids / vals [R, k] = the k <= 8 largest logits of every row, value
 * descending, ties by ascending id (the order fira_beam_select uses). */
int fira_head_topk(void* stream, int R, int V, int k, const float* x, const float* wout, const float* bout, float* logits_ws,
                   int ldl, int32_t* ids, float* vals, int dtype);

/* (v9) The generator projection alone, logits[R, V] = x[R, 256] W[V, 256]^T + bias (Model.py:54 / :85, out_fc), on the bf16
 * matrix cores at fp32 accuracy: both operands as three bf16 terms, six of the nine term products, fp32 accumulation
 * (csrc/head_x3.hip) -- what the model-level calls run in fp32 mode.  x rows at stride ldx, logits rows at stride ldl (both
 * multiples of 4 floats, 16-byte aligned); scratch: fira_head_logits_x3_scratch_bytes(R) bytes (the planes of x).            */
size_t fira_head_logits_x3_scratch_bytes(int R);
int fira_head_logits_x3(void* stream, int R, int V, const float* x, int ldx, const float* W, const float* bias, float* logits,
                        int ldl, void* scratch);


/* (v7) One optimisation step in one call: `loss.backward(); optimizer.step()` of run_model.py:104-111 for a single device --
 * fira_train_fwd_bwd followed by fira_adam_step_mb over [0, live) with the token normaliser of run_model.py:105, bit for bit
 * (Adam is element-wise).  What the single call adds is the ORDER: the update of the head + decoder slice [0, split) is
 * enqueued as soon as the caller's stream has finished the encoder's backward chain, beside the last weight gradients of the
 * library's other streams; [split, live) follows their join.  params is updated in place, m / v are the Adam moments
 * ([>= live] floats each), step counts from 1.  Data-parallel runs keep the two-call form (the all-reduce sits between). */
/* A learning-rate schedule: a pure function of the step number t = 1, 2, ... (W = warmup_steps, N = decay_steps), evaluated in
 * double and rounded to float once:
 *     w = W > 0 ? min(1, t / W) : 1 ;   q = clamp((t - W) / (N - W), 0, 1)
 *     constant   base * w
 *     inv_sqrt   base * min(t / W, sqrt(W / t))                                   (needs W >= 1)
 *     cosine     t <= W ? base * w : min_lr + (base - min_lr) * 0.5 * (1 + cos(pi q))
 *     linear     t <= W ? base * w : min_lr + (base - min_lr) * (1 - q)
 * fira_lr_at is the one definition: the library takes every rate of a scheduled run from it (fira_adam_opts.sched), and a
 * caller of the entries that take a bare `float lr` passes them fira_lr_at(sched, step).  Host functions, no GPU.            */
typedef struct fira_lr_schedule {
    int32_t kind;          /* 0 constant, 1 inv_sqrt, 2 cosine, 3 linear                                 */
    float   base_lr;       /* the peak rate                                                              */
    int32_t warmup_steps;  /* W >= 0                                                                     */
    int32_t decay_steps;   /* N: the step at which cosine / linear reach min_lr (N > W)                  */
    float   min_lr;        /* 0 <= min_lr <= base_lr                                                     */
} fira_lr_schedule;
float fira_lr_at(const fira_lr_schedule* s, int step);   /* step counts from 1 (below 1: as 1); NULL gives 0 */
int   fira_lr_schedule_check(const fira_lr_schedule* s); /* 0, or non-zero with the reason in fira_last_error() */

typedef struct fira_adam_opts {
    float   lr, beta1, beta2, eps;
    int32_t step;
    float*  m;
    float*  v;
    /* NULL: every step uses `lr`.  Otherwise `lr` is ignored and step j uses fira_lr_at(sched, j) -- the step itself and
     * every update a lazily updated row still owes (fira_train_step_rows), so a rate that changes every step needs no
     * fira_adam_rows_sync.  Read during the call only.                                                                  */
    const fira_lr_schedule* sched;
} fira_adam_opts;
int fira_train_step(void* stream, const fira_dims* d, const fira_batch* batch, float* params, float* grads,
                    void* workspace, size_t workspace_bytes, const fira_train_opts* opts, float* loss_sum,
                    int32_t* n_tok, const fira_adam_opts* adam);

/* (v8) The same step for DATA-PARALLEL runs (replaces nn.DataParallel's scatter / replicate / gather of run_model.py:392-394
 * around run_model.py:104-111), as two calls with the caller's collectives in between:
 *   fira_train_step_begin  forward + backward of the output head and the decoder; records mid_event (as fira_train_fwd_bwd
 *                          does) when every gradient of [0, split) is final.  The step stays pending on the calling thread;
 *                          the batch's arrays, the parameter / gradient buffers and the workspace must stay untouched.
 *   -- caller: all-reduce (loss_sum, n_tok) and grads[0, split) on its own stream behind mid_event, record early_event there --
 *   fira_train_step_end    backward of the encoder; Adam of [0, split) on the caller's stream as soon as that stream has
 *                          passed the encoder's chain AND early_event (beside the library's last weight gradients), scaled by
 *                          1 / max(*count, 1) (count: device float = the all-reduced token count; NULL = this rank's n_tok);
 *                          then the join: grads[split, live) are final on `stream` when the call returns.  adam NULL = no update.
 *   -- caller: all-reduce grads[split, live), then fira_adam_step_count on that slice --
 * One process per GPU, one thread per step: the pending step is thread-local.  Same arithmetic as fira_train_fwd_bwd +
 * fira_adam_step_count (tests/test_dp_gpu.py: two ranks == one process). */
int fira_train_step_begin(void* stream, const fira_dims* d, const fira_batch* batch, const float* params, float* grads,
                          void* workspace, size_t workspace_bytes, const fira_train_opts* opts, float* loss_sum,
                          int32_t* n_tok, void* mid_event /* hipEvent_t, required */);
int fira_train_step_end(void* stream, float* params, const fira_adam_opts* adam, void* early_event /* hipEvent_t or NULL */,
                        const float* count);

/* (v10) fira_train_step with a ROW-SPARSE Adam of the two vocabulary-sized embedding tables (decoder.embedding.weight,
 * encoder.embedding.weight: 2 x 6.3 M of the 27.8 M parameters; run_model.py:396's torch.optim.Adam updates every row of both
 * every step).  An embedding row whose gradient row is all zero still moves under Adam -- its moments decay and the parameter
 * follows -- but that update is a function of the row's (p, m, v) and the step number alone, so it is applied LATER, in
 * registers, bit for bit: ahead of a forward pass for the rows that pass gathers (the batch's token ids), or together with the
 * next step whose gradient row is not zero.  row_step [2 * vocab] int32 (zero-initialised with the moments; decoder table
 * first) holds the step up to which each row of params / m / v is current.  Every 32nd step updates every row, so a row lags
 * at most 31 steps.  Results are those of fira_train_step bit for bit ONCE fira_adam_rows_sync has run: call it (same adam
 * values, step = the last completed step) before anything else reads the tables or the moments -- checkpoint, dev pass,
 * search, another optimizer -- and before changing the schedule, beta or eps (with adam->sched NULL, lr is the schedule:
 * a constant).  adam->step must advance by one per call.  Needs
 * opts->zero_grads = 1.  (Data parallel: fira_train_step_begin_rows / _end_rows below.)                                      */
int fira_train_step_rows(void* stream, const fira_dims* d, const fira_batch* batch, float* params, float* grads,
                         void* workspace, size_t workspace_bytes, const fira_train_opts* opts, float* loss_sum,
                         int32_t* n_tok, const fira_adam_opts* adam, int32_t* row_step);
int fira_adam_rows_sync(void* stream, const fira_dims* d, float* params, const fira_adam_opts* adam, int32_t* row_step);
/* The two pieces fira_train_step_rows is made of, as op-level entries (params / grads / m / v: the flat buffers of geometry d):
 * fira_adam_rows_catchup  rows ids[0 .. n_ids) of table `table` (0 decoder.embedding, 1 encoder.embedding; duplicates and
 *                         out-of-range ids allowed) brought up to step adam->step by zero-gradient updates;
 * fira_adam_rows_step     step adam->step on every row of the selected tables whose gradient row is not all zero (every row
 *                         when step % 32 == 0), normaliser 1 / max(*n_tok, 1) as fira_adam_step_mb or 1 / max(*count, 1).   */
int fira_adam_rows_catchup(void* stream, const fira_dims* d, float* params, const fira_adam_opts* adam, int32_t* row_step,
                           int table, const int32_t* ids, int n_ids);
int fira_adam_rows_step(void* stream, const fira_dims* d, float* params, const float* grads, const fira_adam_opts* adam,
                        int32_t* row_step, const int32_t* n_tok, const float* count /* NULL, or the normaliser 1 / max(*count, 1)
                        of fira_adam_step_count */, int tables /* bit t: table t takes part; 3 = both */);
/* The data-parallel step (fira_train_step_begin / _end) with the same update.  The union of the ranks' touched rows is what
 * the ALL-REDUCED gradient shows as non-zero rows, the same on every rank, so the replicas (tables, moments, row_step) stay
 * identical.  _begin_rows takes the optimizer's values for the lazy reads of its forward pass (nothing is updated there);
 * _end_rows updates [0, split) as fira_train_step_end does, decoder.embedding by rows; encoder.embedding is the caller's:
 * fira_adam_rows_step(tables = 2, count) + fira_adam_step_count on the rest of [split, live) behind the late bucket.          */
int fira_train_step_begin_rows(void* stream, const fira_dims* d, const fira_batch* batch, const float* params, float* grads,
                               void* workspace, size_t workspace_bytes, const fira_train_opts* opts, float* loss_sum,
                               int32_t* n_tok, void* mid_event, const fira_adam_opts* adam, int32_t* row_step);
int fira_train_step_end_rows(void* stream, float* params, const fira_adam_opts* adam, void* early_event, const float* count,
                             int32_t* row_step);

/* Exponential moving average of the weights (csrc/ema.hip; additive, the ABI version is unchanged).  For every element
 *     diff = p - e;   e = e + w * diff
 * the subtraction, the multiply and the add each rounded to fp32 on its own (no fused multiply-add), so a loop of np.float32
 * operations is the reference; an element with p == e keeps its value.  w = (float)(1 - D^K) for a per-step decay D applied
 * every K steps, formed by the caller in double.  0 <= w <= 1 and finite, else non-zero with the reason in fira_last_error()
 * and nothing launched.
 *   fira_ema_update       ema[0, n) toward p[0, n); n >= 1, any 4-byte alignment of either pointer (16-byte accesses where the
 *                         addresses allow, 4-byte ones at the edges).  ema must not overlap p (refused).
 *   fira_ema_update_rows  the whole flat buffer [0, fira_param_total(d)) of a model trained with fira_train_step_rows, in one
 *                         launch: the two vocabulary-sized embedding tables are read as a forward pass reads them -- a row that
 *                         lags behind adam->step with the zero-gradient updates it owes applied in registers (same adam values
 *                         as the step that has just run, step = the last completed step) -- so the average is the one a dense
 *                         Adam would give, bit for bit, WITHOUT fira_adam_rows_sync.  It writes ema only: params, the moments
 *                         and row_step are read.  ema, params and the moments 16-byte aligned; ema overlaps none of them.   */
int fira_ema_update(void* stream, int64_t n, float* ema, const float* p, float w);
int fira_ema_update_rows(void* stream, const fira_dims* d, float* ema, const float* params, const fira_adam_opts* adam,
                         const int32_t* row_step, float w);

/* Clipping by the GLOBAL gradient norm on the device (torch.nn.utils.clip_grad_norm_ between run_model.py:108 and :111,
 * error_if_nonfinite = False) and a guard against non-finite gradients.  With g the flat loss-SUM gradient of [0, live) and
 * inv = 1 / max(n_tok, 1) (or 1 / max(count, 1), the all-reduced token count of a data-parallel step), for max_norm C > 0
 * (C = inf allowed: observe and guard only):
 *     norm = inv * sqrt(sum_i g_i^2) ;   coef = min(1, C / (norm + 1e-6)) ;   Adam sees g_i * inv * coef
 *   - coef == 1: the update is bit-identical to the unclipped kernels' on the same buffers;
 *   - norm not finite (an inf / nan gradient element, or a sum of squares that overflows fp32: an element above about 1.8e19 on
 *     the loss-SUM scale; torch's fp32 norm overflows alike): the step is applied as a ZERO-GRADIENT step -- every element takes g_i := 0, the
 *     step number advances as usual, n_nonfinite counts it.  (Not "leave p, m, v untouched": the host does not know the outcome
 *     without a sync, the bias corrections come from the step number, and the row-sparse update owes untouched rows exactly one
 *     zero-gradient update per step: dense and row-sparse stay equal bit for bit, and every rank of a data-parallel run takes
 *     the same decision from the same all-reduced numbers.)
 * fira_clip_state (device memory, 64 bytes, zero-initialised by the caller once) carries the result from the norm to the updates:
 * sq[k] = the sum of squares of the k-th range it was given (the two readiness buckets; ZeRO-1's shards), norm, coef, zero_flag
 * of the last closing step, and two running counters.
 *   fira_grad_sqsum   state->sq[slot] = sum of g[0, n)^2 (n < 2^31, g 16-byte aligned, n = 0 gives 0).  Fixed summation order (no
 *                     atomics; partials added in a fixed strided + tree order, in double): the same bits on every call and graph replay; relative error <= (D + 1) * 2^-24 against the exact sum,
 *                     D = roundup(ceil((n / 4) / 1024), 1024) / 1024 + 12 (19 for the model's live parameters).  scratch:
 *                     fira_grad_sqsum_scratch_bytes() bytes, 8-byte aligned; slots use disjoint parts of it.
 *   fira_clip_finish  norm / coef / zero_flag / counters from sq[0 .. n_slots), n_slots <= 4; n_tok or count as above.
 *   fira_adam_step_clip / fira_adam_rows_step_clip   fira_adam_step_mb (g1 = NULL) / fira_adam_step_count (count != NULL) and
 *                     fira_adam_rows_step on g * inv * coef, or on a zero gradient under zero_flag.
 *   fira_train_step_clip   fira_train_step_rows (row_step given) / fira_train_step (row_step NULL) with the clipped update: the
 *                     sum of squares of [0, split) runs beside the encoder's backward pass, that of [split, live), the closing
 *                     step and the whole update behind the final join (the early update of [0, split) is what clipping costs).
 *                     scratch as for fira_grad_sqsum.  Nothing synchronises, nothing allocates.                                  */
typedef struct fira_clip_state {
    float   sq[4];
    float   norm;            /* of the last closing step (inf / nan when the gradient was not finite)   */
    float   coef;            /* what the updates multiply by (1 under zero_flag)                        */
    int32_t zero_flag;       /* 1: the updates take a zero gradient                                     */
    int32_t n_clipped;       /* closing steps with coef < 1                                             */
    int32_t n_nonfinite;     /* closing steps with a non-finite norm                                    */
    int32_t reserved[7];
} fira_clip_state;
size_t fira_grad_sqsum_scratch_bytes(void);
int fira_grad_sqsum(void* stream, int64_t n, const float* g, fira_clip_state* state, int slot, void* scratch);
int fira_clip_finish(void* stream, fira_clip_state* state, int n_slots, const int32_t* n_tok, const float* count,
                     float max_norm);
int fira_adam_step_clip(void* stream, int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                        float beta2, float eps, int step, const int32_t* n_tok, const float* count,
                        const fira_clip_state* state);
int fira_adam_rows_step_clip(void* stream, const fira_dims* d, float* params, const float* grads, const fira_adam_opts* adam,
                             int32_t* row_step, const int32_t* n_tok, const float* count, int tables,
                             const fira_clip_state* state);
int fira_train_step_clip(void* stream, const fira_dims* d, const fira_batch* batch, float* params, float* grads,
                         void* workspace, size_t workspace_bytes, const fira_train_opts* opts, float* loss_sum,
                         int32_t* n_tok, const fira_adam_opts* adam, int32_t* row_step /* may be NULL */, float max_norm,
                         fira_clip_state* state, void* scratch);

/* Gradient accumulation: ONE optimizer step over K micro-batches (additive, the ABI version is unchanged).  Every model-level
 * call leaves the gradient of its batch's loss SUM in grads (+= unless opts->zero_grads) and the update kernels form
 * 1 / max(count, 1) themselves, so the sum of the K gradients with the sum of the K token counts IS the step of the big batch:
 * no per-micro-batch weight exists.
 *   fira_accum_stats        stats[0] = (first ? 0 : stats[0]) + *loss_sum ;  total = (first ? 0 : *n_tok_total) + *n_tok ;
 *                           *n_tok_total = total ;  stats[1] = (float) total.  One lane, plain stores, no atomic: the caller's
 *                           stream orders the K calls.  The layout is fira_pack_stats': what takes count = stats + 1 takes this.
 *                           The count is exact as a float below 2^24 tokens (above, (float) total is the int32 rounded to nearest
 *                           even once, never a sum of rounded floats); the int32 total is exact always (below 2^31).  The loss
 *                           sum is a chain of fp32 additions in call order.  first != 0 ignores what the buffers hold.
 *   fira_train_accum_micro  forward + backward of one micro-batch that is NOT the last: fira_train_fwd_bwd, with the word-table
 *                           rows the row-sparse Adam still owes read as fira_train_step_begin_rows reads them (adam, row_step:
 *                           the values of the step being accumulated, adam->step = its number; both NULL = tables up to date).
 *                           grads += (opts->zero_grads = 1 on the first micro-batch only), loss_sum / n_tok overwritten; NOTHING is
 *                           updated, row_step included.  The caller follows it with fira_accum_stats.
 *   fira_train_accum_last   the last micro-batch, run as fira_train_step / _rows (row_step given) / _clip (clip_state given) run
 *                           theirs: behind its loss the call itself adds (*loss_sum, *n_tok) to stats / n_tok_total as
 *                           fira_accum_stats(first = 0) does -- the update is enqueued by the same call, so no caller could --
 *                           and every update (the head + decoder slice beside the last weight gradients, the rows launch, the
 *                           rest behind the join; clipped: everything behind the join) is normalised by
 *                           1 / max(stats[1], 1), the norm of a clipped step included.  With K = 1 use the plain entries.
 * Why micro-batches 2..K need no cleared gradient although fira_train_step_rows "needs opts->zero_grads = 1": the rows update
 * takes "gradient row all zero" for "row untouched", so the tables' gradient must hold nothing but THIS step's sums -- a stale
 * row left by an earlier step would be applied again.  Cleared on the first micro-batch, the accumulated table shows as
 * non-zero rows exactly the UNION of the micro-batches' touched rows (the argument of the all-reduced gradient in data
 * parallel).  A row whose contributions cancel to an all-zero row is taken for untouched and gets its zero-gradient update
 * later -- the same bits, since that is what a dense Adam would apply.  The lazy reads of micro-batches 2..K see rows at
 * step - 1, as the first does: nothing is updated between them.  Data parallel: K - 1 x fira_train_accum_micro, then
 * fira_train_step_begin(_rows) with opts->zero_grads = 0 and the collectives as ever, on the accumulated stats pair.          */
int fira_accum_stats(void* stream, const float* loss_sum, const int32_t* n_tok, float* stats /* [2] */,
                     int32_t* n_tok_total, int first);
int fira_train_accum_micro(void* stream, const fira_dims* d, const fira_batch* batch, const float* params, float* grads,
                           void* workspace, size_t workspace_bytes, const fira_train_opts* opts, float* loss_sum,
                           int32_t* n_tok, const fira_adam_opts* adam /* may be NULL */, int32_t* row_step /* may be NULL */);
int fira_train_accum_last(void* stream, const fira_dims* d, const fira_batch* batch, float* params, float* grads,
                          void* workspace, size_t workspace_bytes, const fira_train_opts* opts, float* loss_sum,
                          int32_t* n_tok, const fira_adam_opts* adam, int32_t* row_step /* may be NULL */,
                          float* stats /* [2] */, int32_t* n_tok_total, float max_norm /* read with clip_state only */,
                          fira_clip_state* clip_state /* NULL: not clipped */, void* clip_scratch);

/* (v8) bf16 wire format of a gradient bucket (BASELINE configs[2]: 55.6 MB instead of 111.2 MB per step on xGMI):
 * out[i] = bf16(in[i]) (round to nearest even) / out[i] = float(in[i]).  n % 4 == 0, 16-byte aligned buffers. */
int fira_f32_to_bf16(void* stream, int64_t n, const float* in, uint16_t* out);
int fira_bf16_to_f32(void* stream, int64_t n, const uint16_t* in, float* out);

/* TransModel.forward(..., 'dev') (Model.py:85-86): teacher-forced argmax ids [B, tar_len].         */
int fira_forward_dev(void* stream, const fira_dims* d, const fira_batch* batch, const float* params,
                     void* workspace, size_t workspace_bytes, int32_t* ids_out, float* loss_sum, int32_t* n_tok,
                     int dtype /* FIRA_F32 | FIRA_BF16 */);

/* Sentence-BLEU statistics of dev() (run_model.py:138-177) on token ids, one row per commit (csrc/bleu.hip; additive, the ABI
 * version is unchanged).  Hypothesis: ids[b] up to its first raw <eos> (all T without one), copy entries resolved through sou /
 * sub_token (index clamped), resolved <pad> dropped; reference: tar[b][1 : first <eos>] (to T without one).  A hypothesis <unkm>
 * matches nothing.  For n = 1..4: cnt = hypothesis n-grams, num = sum over distinct hypothesis n-grams of min(count in the
 * hypothesis, count in the reference).  int32 and exact; T <= 64, V >= 4, L, S >= 1; B == 0 is a no-op.                        */
int fira_dev_bleu_stats(void* stream, int B, int T, int V, int L, int S,
                        const int32_t* ids,  /* [B,T] output indices of fira_forward_dev, in [0, V+L+S) */
                        const int32_t* sou,  /* [B,L] */  const int32_t* sub_token, /* [B,S] */
                        const int32_t* tar,  /* [B,T] */
                        int32_t* hyp,        /* [B,T] resolved vocabulary ids of the hypothesis, compacted, -1 behind hyp_len */
                        int32_t* stats);     /* [B,12]: num[4], cnt[4], hyp_len, ref_len, 0, 0 */

/* The same statistics for every ordered pair of the n candidate messages of a commit (minimum-Bayes-risk selection by expected
 * sentence BLEU; csrc/bleu.hip; additive, the ABI version is unchanged).  The message of candidate (b, i) is tokens[b][i] at
 * positions 1 .. min(length[b][i], T) - 1 with every <pad> (0), <eos> (1) and <start> (2) dropped wherever it stands; ids at or
 * past length are ignored; length <= 1 is the empty message; <unkm> is an ordinary word.  stats[b][i][j] takes candidate i as the
 * hypothesis and candidate j as the reference (the diagonal included: num == cnt there).  int32 and exact; 1 <= n <= 32,
 * 1 <= T <= 64; B == 0 is a no-op.                                                                                             */
int fira_mbr_bleu_stats(void* stream, int B, int n, int T,
                        const int32_t* tokens, /* [B,n,T] vocabulary ids */  const int32_t* length, /* [B,n] */
                        int32_t* stats);       /* [B,n,n,12]: num[4], cnt[4], hyp_len, ref_len, 0, 0 */

/* ROUGE-L statistics on token ids (csrc/rouge.hip; additive, the ABI version is unchanged): lcs = the length of the longest
 * common subsequence of hypothesis and reference, and the two lengths; sentence-level ROUGE-L (F-measure, beta = 1) is
 * 2 lcs / (hyp_len + ref_len), 0 for lcs == 0.  The candidates' messages are exactly fira_mbr_bleu_stats's, the hypothesis and
 * reference of a commit exactly fira_dev_bleu_stats's (a hypothesis <unkm> matches nothing; copy indices clamped), and so are
 * the limits: 1 <= n <= 32, 1 <= T <= 64, V >= 4, L, S >= 1; B == 0 is a no-op.  int32 and exact.  lcs[b][i][j] == lcs[b][j][i],
 * and on the diagonal lcs == hyp_len == ref_len.                                                                               */
int fira_mbr_rouge_l_stats(void* stream, int B, int n, int T,
                           const int32_t* tokens, /* [B,n,T] vocabulary ids */  const int32_t* length, /* [B,n] */
                           int32_t* stats);       /* [B,n,n,4]: lcs, hyp_len, ref_len, 0 (candidate i hypothesis, j reference) */
int fira_dev_rouge_l_stats(void* stream, int B, int T, int V, int L, int S,
                           const int32_t* ids,  /* [B,T] output indices of fira_forward_dev, in [0, V+L+S) */
                           const int32_t* sou,  /* [B,L] */  const int32_t* sub_token, /* [B,S] */
                           const int32_t* tar,  /* [B,T] */
                           int32_t* stats);     /* [B,4]: lcs, hyp_len, ref_len, 0 */

/* METEOR alignment statistics on token ids (csrc/meteor.hip; additive, the ABI version is unchanged): m = the matched word
 * pairs of NLTK's alignment (_match_enums: hypothesis positions from the last to the first, each taking the last free reference
 * position of equal key), chunks = m minus the matches (i, j) for which (i + 1, j + 1) is a match too (0 when m == 0), and the
 * two lengths.  Stage 1 matches equal ids.  Stage 2 runs only when classes [V] is given: the words still free whose ids lie in
 * [0, V) match on equal classes[id]; an id outside [0, V) -- a hypothesis <unkm>, compared as a sentinel -- has no class.  No
 * stemmer and no synonym table is part of the library: with classes == NULL this is exact matching only, hence "meteor_exact" on
 * the Python side (metrics.meteor_exact_from_stats: alpha 0.9, beta 3, gamma 0.5); no figure is comparable with NLTK's METEOR
 * with WordNet.  Messages and limits are the ROUGE-L entries'; with classes, V >= 4 also for the all-pairs entry.  m and chunks
 * are the same for [b][i][j] and [b][j][i]; on the diagonal (len, len > 0 ? 1 : 0, len, len).  int32 and exact; B == 0 is a
 * no-op.                                                                                                                       */
int fira_dev_meteor_stats(void* stream, int B, int T, int V, int L, int S,
                          const int32_t* ids,  /* [B,T] output indices of fira_forward_dev, in [0, V+L+S) */
                          const int32_t* sou,  /* [B,L] */  const int32_t* sub_token, /* [B,S] */
                          const int32_t* tar,  /* [B,T] */
                          const int32_t* classes, /* [V] or NULL */
                          int32_t* stats);     /* [B,4]: m, chunks, hyp_len, ref_len */
int fira_mbr_meteor_stats(void* stream, int B, int n, int T,
                          const int32_t* tokens, /* [B,n,T] vocabulary ids */  const int32_t* length, /* [B,n] */
                          int V, const int32_t* classes, /* [V] or NULL (V is then ignored) */
                          int32_t* stats);       /* [B,n,n,4]: m, chunks, hyp_len, ref_len (candidate i hypothesis, j reference) */

/* Encoder once per batch (run_model.py:202-207) + everything of the decode loop that does not depend
 * on the generated prefix: memory [B,S,256], mem_valid [B,S], cross-attention K/V of all layers,
 * LinearSource(memory).  State lives in the caller's workspace.                                     */
int fira_decode_begin(void* stream, const fira_dims* d, const fira_batch* batch, const float* params,
                      void* workspace, size_t workspace_bytes, int n_beam);
/* One decode step for every (commit, beam) row with KV cache: consumes tokens[B*n_beam] (ids at position
 * `step`), produces dist [B*n_beam, vocab+S] = the reference's `output[:, step, :]` (run_model.py:256-267)
 * if dist != NULL, and/or greedy argmax ids + their probability.  parent[B*n_beam] (may be NULL) re-orders
 * the self-attention cache rows after a beam re-ranking.                                            */
int fira_decode_step(void* stream, const fira_dims* d, const float* params, void* workspace,
                     size_t workspace_bytes, int B, int n_beam, int step, const int32_t* tokens,
                     const int32_t* parent, float* dist, int32_t* best_id, float* best_p);
/* The same two calls with option flags (both calls of one search must carry the same flags):
 *   FIRA_DECODE_KV_BF16  keep a bf16 copy of the cross-attention K|V rows of all layers and stream THAT in every step
 *                        (the cross K|V are 315 of the 379 MB a step moves at batch 64); the arithmetic stays fp32 on the
 *                        widened values.  Not the default: with it the searched ids are no longer bit-identical to the
 *                        reference's fp32 run (bench.py reports the agreement). */
#define FIRA_DECODE_KV_BF16 1
int fira_decode_begin_ex(void* stream, const fira_dims* d, const fira_batch* batch, const float* params,
                         void* workspace, size_t workspace_bytes, int n_beam, int flags);
int fira_decode_step_ex(void* stream, const fira_dims* d, const float* params, void* workspace,
                        size_t workspace_bytes, int B, int n_beam, int step, const int32_t* tokens,
                        const int32_t* parent, float* dist, int32_t* best_id, float* best_p, int flags);

/* Hypothesis bookkeeping of the search loop on the device (run_model.py:225-246 and :268-340).  State per commit:
 * gen [B*n_beam, tar_len] ids starting with <start>, length [B*n_beam], prob [B*n_beam] (slot 0 starts at 1, the others
 * at 0), double-buffered by the caller.  `active` has 9 ints (flags of up to 8 slots + their count), `done` 1 int that
 * latches once no slot runs; after that fira_beam_select only copies the state through.
 *   fira_beam_prepare : finished[r] = last token is <eos>; active[j] = some commit unfinished in slot j;
 *                       tokens[r] = id at position `step` (0 once the hypothesis is shorter) -> fira_decode_step
 *   fira_beam_select  : the n_beam best of { dist[slot j] * prob[j] (-1 if finished) for running slots, in slot order }
 *                       ++ { prob of finished hypotheses, slot order, -1 padded }, ranked by (value desc, index asc);
 *                       copy ids resolved through sou / sub_token; writes the new state and parent[] for the KV cache */
int fira_beam_prepare(void* stream, int B, int n_beam, int tar_len, int step, const int32_t* gen, const int32_t* length,
                      int32_t* tokens, int32_t* finished, int32_t* active, int32_t* done);
int fira_beam_select(void* stream, const fira_dims* d, int B, int n_beam, const float* dist, const int32_t* finished,
                     const int32_t* active, const int32_t* done, const int32_t* sou, const int32_t* sub_token,
                     const int32_t* gen_in, const int32_t* len_in, const float* prob_in, int32_t* gen_out,
                     int32_t* len_out, float* prob_out, int32_t* parent);

/* fira_beam_select under a length-normalised key, in diverse beam groups (csrc/beam_score.hip; additive, the ABI version is
 * unchanged).  The arguments of fira_beam_select, then inv_lp, n_groups, diversity and key_out; the state is the same, since a
 * hypothesis's key is a function of its (prob, length):
 *     key(p, m) = ln(p) * inv_lp[m],  inv_lp[m] = 1 / ((5 + m) / 6)^alpha  (GNMT; computed by the caller in float64, rounded to
 *     fp32, tar_len + 1 entries on the device),  m = words emitted = length - 1 (<start> not counted, <eos> counted),  ln 0 = -inf.
 * Candidates of a step, per commit:
 *     running   entry i of running slot j: p = fp32(dist[j, i] * prob[j]) (the product fira_beam_select forms), m = len_j
 *     carried   a finished hypothesis of the commit: p = prob[j], m = len_j - 1 (fixed from the moment it finished)
 *     void      the entries of a finished hypothesis's row and the padding of the carried list (fira_beam_select's two -1)
 * Total order: void last, then penalised key descending, then p descending, then fira_beam_select's flattened index ascending
 * (running slots in slot order, then the carried list).  With every inv_lp[m] = 1 (alpha = 0) and n_groups = 1 the order is
 * (p descending, index ascending): gen_out, len_out, prob_out and parent equal fira_beam_select's bit for bit.
 * Groups: the n_beam slots are n_groups groups of k = n_beam / n_groups consecutive slots, handled in ascending order within
 * the step; group g takes its k best among the candidates of ITS OWN slots (their running rows and their finished hypotheses)
 * and writes them to its own slots, best first.  Penalised key of a running candidate: key - diversity * c, c = the number of
 * picks made earlier in this step, for this commit, by groups < g that EXTENDED a hypothesis with the same WORD (multiplicity
 * counts); the word of entry i is w(i) of fira_constrain_dist: the generator id, or the sou / sub_token id of a copy slot.
 * Carried candidates are never penalised and contribute to no count.  The penalty affects selection only: prob_out is the raw
 * product, key_out[r] (optional) = key(prob_out[r], len_out[r] - 1), -inf for a probability of 0.  The caller seeds slot g * k
 * of every group with probability 1 and the other slots with 0.  Keys are formed and compared in fp64 on the fp32 products.
 * Once `done` is set the state is copied through (key_out is still written).  Nothing is renormalised.
 * 2 <= n_beam <= 8, n_groups >= 1 divides n_beam, diversity finite and >= 0, tar_len <= 64, sou_len + sub_len <= 1 024,
 * vocab > 8.  One workgroup per commit, the bytes streamed are fira_beam_select's; vector stores only, no global atomics. */
int fira_beam_select_scored(void* stream, const fira_dims* d, int B, int n_beam, const float* dist, const int32_t* finished,
                            const int32_t* active, const int32_t* done, const int32_t* sou, const int32_t* sub_token,
                            const int32_t* gen_in, const int32_t* len_in, const float* prob_in, int32_t* gen_out,
                            int32_t* len_out, float* prob_out, int32_t* parent,
                            const float* inv_lp /* device, [tar_len + 1] */, int n_groups, float diversity,
                            float* key_out /* [B*n_beam] or NULL */);

/* Stochastic beam search: fira_beam_select with a Gumbel-perturbed key (csrc/beam_gumbel.hip; additive, the ABI version is
 * unchanged; Kool, van Hoof and Welling 2019).  It takes fira_beam_select's place in the step loop, after fira_beam_prepare, the
 * step (fira_mix_dist), fira_merge_dist and fira_constrain_dist; the n_beam hypotheses a search ends with are a sample WITHOUT
 * replacement from the model's distribution over messages, best key first, and slot 0 is an ordinary ancestral sample.
 * State per slot, double-buffered by the caller: gen, length and parent as fira_beam_select has them, and three fp32 values in
 * place of prob: phi (log-probability under the sampling model), G (the perturbed key; -inf marks the slot VOID) and logp (the
 * untempered sum of logf(p_entry) of the entries taken -- what fira_sample_advance accumulates).  The caller seeds slot 0 of
 * every commit with phi = G = logp = 0 and the other slots with G = -inf.
 * Per commit b, slot j RUNS if G_j > -inf and finished[b * n_beam + j] == 0.  Its row p = dist[b * n_beam + j, :] is taken as it
 * stands; an entry is VALID if 0 < p_i <= FLT_MAX (a zero, a NaN, an inf are void).  Over the valid entries, all in fp32:
 *     sampling model  q_i = p_i^(1/T) / Z:  u_i = logf(p_i) * (1/T),  um = logf(max_i p_i) * (1/T),
 *                     lnZ = um + logf(sum_i expf(u_i - um))          (always applied, at T = 1 too; fixed summation order)
 *     noise           g_i of fira_decode_step_sample with stream = mix32(base(key[b], seed) + 0x9E3779B9 * (j * tar_len + step + 1))
 *     row score       s_i = fmaf(logf(p_i), 1/T, g_i) -- the sampler's own expression and rounding: the row's arg-max a (lowest
 *                     index on ties) is the sampler's draw for the same (key, seed, j, step), bit for bit
 *     c = phi_j - lnZ,  g_i = c + s_i,  Zmax = c + s_a
 *     key             of a: G_j, by definition.  Of i != a, with d = g_i - Zmax:  G_j where d >= 0 (a tie with a), else
 *                     v = (G_j - g_i) + log1pf(-expf(d)),   key_i = (G_j - fmaxf(0, v)) - log1pf(expf(-fabsf(v)))
 *                     -- the stable form of -log(exp(-G_j) - exp(-Zmax) + exp(-g_i)); no operand of it is infinite
 *     child           length + 1, the id entry i resolves to (sou / sub_token for a copy entry) appended, key as above,
 *                     logp = logp_j + logf(p_i),  phi = phi_j + (logf(p_i) * (1/T) - lnZ),  parent = the row of j
 * A finished hypothesis with G > -inf is CARRIED: it competes with its own (phi, G, logp) unchanged.  Void candidates: the
 * entries that are not valid, and every entry of a void or finished slot's row.  Total order per commit: void last, then key
 * descending, then a row's arg-max entry before every other candidate, then fira_beam_select's flattened index ascending
 * (running slots in slot order, then the carried hypotheses in slot order).  The n_beam best go to slots 0 .. n_beam - 1, best
 * first; where fewer than n_beam candidates are not void the remaining slots are void: G = phi = logp = -inf, length = 1,
 * gen = <start> alone, parent = the slot's own row.  (A void slot never counts as finished, so `done` does not latch while a
 * commit has one: such a search runs its tar_len - 1 steps.)  Once `done` is set the state is copied through.
 * key [B] int32 per commit; seed_dev a DEVICE uint64 read when the kernel runs (one captured graph serves every seed).
 * 1 <= n_beam <= 8, 2 <= tar_len <= 64, 0 <= step <= tar_len - 2, vocab in 9 .. 25 600, sou_len + sub_len <= 1 024, temperature
 * finite and > 0; anything else returns non-zero with the reason in fira_last_error() and nothing is launched.  One workgroup
 * per commit; a running row is read once and kept in registers; vector stores only, no atomics on global memory.          */
int fira_beam_select_gumbel(void* stream, const fira_dims* d, int B, int n_beam, int step, float temperature,
                            const float* dist, const int32_t* finished, const int32_t* done, const int32_t* sou,
                            const int32_t* sub_token, const int32_t* key /* [B] */, const uint64_t* seed_dev,
                            const int32_t* gen_in, const int32_t* len_in, const float* phi_in, const float* G_in,
                            const float* logp_in, int32_t* gen_out, int32_t* len_out, float* phi_out, float* G_out,
                            float* logp_out, int32_t* parent);

/* Lexically constrained beam search: fira_beam_select with dynamic beam allocation (csrc/beam_require.hip; additive, the ABI
 * version is unchanged; Post and Vilar, NAACL 2018).  The arguments of fira_beam_select, then required, n_required and met_out;
 * the state is the same, since the number of required words a hypothesis holds is a function of its gen row.  required and
 * n_required are DEVICE buffers read when the kernel runs: one captured graph serves every word list.
 * Per commit b: C = n_required[b] (a value outside 0..4 is clamped), R_k = required[b, k] for k < C.
 *     w(i)     the word of entry i, as fira_constrain_dist defines it: the generator id, or the sou / sub_token id of a copy slot
 *     met(h)   the set of k such that R_k occurs among gen[1 .. length - 1] (length clamped to 1 .. tar_len)
 *     bank(h)  |met(h)|
 * Candidates of a step: fira_beam_select's, in its flattened index order (running slots in slot order, then the carried list):
 *     running   entry i of running slot j: p = fp32(dist[j, i] * prob[j]), the very product fira_beam_select forms;
 *               bank = |met(h_j) u { k : R_k == w(i) }|
 *     carried   a finished hypothesis: p = prob[j], bank = bank(h_j)
 *     void      fira_beam_select's two -1 cases (the row of a finished hypothesis, the padding of the carried list), plus every
 *               entry with w(i) == <eos> (1) of a running row with bank(h_j) < C: a message may not end before it holds all its
 *               words.  A copy slot that carries id 1 is blocked like the generator entry.
 * Selection, phase 1 (round robin over banks): only candidates with p > 0 take part; within a bank they are ranked by
 * (p descending, flattened index ascending).  Repeat until n_beam picks are made or no positive candidate is left:
 *     for c = C down to 0: if bank c has an unpicked positive candidate, pick its best.
 * Each bank gets an even share, the highest bank first; a bank that runs dry hands its share to the others.
 * Selection, phase 2 (fill): slots still free take the remaining candidates in fira_beam_select's own order: value descending
 * with void = -1, index ascending.  A void candidate is never reached: r running rows leave at least
 * r * (W - copies of <eos> - 1) entries that are not void, and vocab > 8.
 * Written order of the n_beam picks: p > 0 first, then bank descending, then p descending, then pick order ascending.  gen_out,
 * len_out, prob_out and parent are formed as fira_beam_select forms them; met_out[r] (optional) is the bank of the hypothesis
 * written to row r.
 * Anchor: with C = 0 for a commit, phase 1 followed by phase 2 is (p descending, index ascending) and the sort is stable, so that
 * commit's four outputs are fira_beam_select's bit for bit.  Once `done` is set the state is copied through (met_out is still
 * written).  Nothing is renormalised.
 * 2 <= n_beam <= 8, tar_len <= 64, vocab in 9 .. 25 600, sou_len + sub_len <= 1 024; anything else returns non-zero with the
 * reason in fira_last_error() and nothing is launched.  One workgroup of 1 024 threads per commit; every running row is streamed
 * once, the bytes are fira_beam_select's (plus at most 4 re-read entries per row); vector stores only, no global atomics.   */
int fira_beam_select_required(void* stream, const fira_dims* d, int B, int n_beam, const float* dist, const int32_t* finished,
                              const int32_t* active, const int32_t* done, const int32_t* sou, const int32_t* sub_token,
                              const int32_t* gen_in, const int32_t* len_in, const float* prob_in, int32_t* gen_out,
                              int32_t* len_out, float* prob_out, int32_t* parent,
                              const int32_t* required /* device, [B, 4] */, const int32_t* n_required /* device, [B] */,
                              int32_t* met_out /* [B*n_beam] or NULL */);

/* Required PHRASES: fira_beam_select_required with items that are word sequences (csrc/beam_phrase.hip; additive, the ABI version
 * is unchanged; Post and Vilar define dynamic beam allocation for phrases).  The arguments of fira_beam_select, then words,
 * item_len, n_items and met_out -- DEVICE buffers read when the kernel runs: one captured graph serves every list.
 * Per commit b: n = n_items[b] (clamped to 0..4) items, given flattened: item k has l_k = item_len[b, k] words (clamped to
 * 0 .. 4 - (l_0 + .. + l_{k-1}), so the lengths sum to at most 4), the words words[b, o_k .. o_k + l_k), o_k = l_0 + .. + l_{k-1};
 * total = the sum of the l_k.  For a hypothesis h = gen[1 .. length - 1] (length clamped to 1 .. tar_len):
 *     done(h)      the set of items that occur contiguously in h
 *     partial(h)   the largest q >= 1 for which some item k outside done(h) has q < l_k and its first q words are the last q
 *                  words of h; 0 if there is none
 *     progress(h)  (the sum of l_k over done(h)) + partial(h), in 0 .. total;  bank(h) = progress(h)
 * Candidates: fira_beam_select_required's, with
 *     running   entry i of running slot j: p = fp32(dist[j, i] * prob[j]), bank = progress(h_j . w(i))
 *     carried   a finished hypothesis: p = prob[j], bank = progress(h_j)
 *     void      fira_beam_select's two -1 cases, plus every entry with w(i) == <eos> (1) -- the generator entry and every copy slot
 *               that carries id 1 -- of a running row with progress(h_j) < total
 * A hypothesis that breaks a phrase off loses that phrase's partial credit: appending an unrelated word gives the sum over
 * done(h_j) alone.  The two phases, the written order, the four state outputs, the `done` pass-through and the limits are
 * fira_beam_select_required's with C = total; met_out[r] (optional) is the progress of the hypothesis written to row r.
 * Anchors: with every item one word long the five outputs are fira_beam_select_required's bit for bit (words = its required,
 * n_items = its n_required, item_len all 1); with n_items = 0 the four state outputs are fira_beam_select's.
 * 2 <= n_beam <= 8, tar_len <= 64, vocab in 9 .. 25 600, sou_len + sub_len <= 1 024; anything else returns non-zero with the
 * reason in fira_last_error() and nothing is launched.  One workgroup of 1 024 threads per commit; every running row is streamed
 * once (plus at most 4 re-read entries per row); vector stores only, no global atomics.                                        */
int fira_beam_select_phrases(void* stream, const fira_dims* d, int B, int n_beam, const float* dist, const int32_t* finished,
                             const int32_t* active, const int32_t* done, const int32_t* sou, const int32_t* sub_token,
                             const int32_t* gen_in, const int32_t* len_in, const float* prob_in, int32_t* gen_out,
                             int32_t* len_out, float* prob_out, int32_t* parent,
                             const int32_t* words /* device, [B, 4]: the items' words, concatenated */,
                             const int32_t* item_len /* device, [B, 4] */, const int32_t* n_items /* device, [B] */,
                             int32_t* met_out /* [B*n_beam] or NULL */);

/* Contrastive search: the selection of one step (csrc/contrastive.hip; additive, the ABI version is unchanged; Su et al.,
 * NeurIPS 2022).  The state is the beam family's with k slots per commit, 2 <= k <= 8.  Entering step `step`, the k slots of
 * a running commit hold the same chosen prefix gen[0 .. step - 1]; slot j also holds one candidate next word v_j at position
 * `step` (len = step + 1) with its model confidence p_in[j], or is VOID (p_in[j] not > 0).  The decoder step has consumed v_j:
 * hidden[j] is its last hidden state (fira_decode_hidden), dist[j] the distribution after it (as the edit chain left it), and
 * finished[j] says that v_j is <eos> (fira_beam_prepare).  hist[b, i] (i < step) is the hidden state stored when position i
 * was chosen.  Per commit b with ended[b] == 0:
 *   1. sim_j = max_{i < step} cos(hidden[j], hist[b, i]),  cos(a, c) = dot / (sqrt(|a|^2) * sqrt(|c|^2)) in fp32, 0 where a
 *      squared norm is 0; sim_j = 0 at step 0.
 *   2. score_j = fp32(fp32((1 - alpha) * p_in[j]) - fp32(alpha * sim_j)), 1 - alpha formed in fp32; void slots take no part.
 *   3. j* = the slot of the largest score, the lowest slot on ties.  hist[b, step] = hidden[j*];
 *      prob_out[b] = fp32(prob_in[b] * p_in[j*]).
 *   4. finished[j*]: the commit ENDS.  Every slot receives hypothesis j* (gen, len, p_in[j*]) and ended[b] = 1.
 *   5. otherwise the new candidates are the k largest POSITIVE entries of dist[j*], by (value descending, index ascending).
 *      Slot m receives gen[j*] with the word of candidate m appended (the entry itself below vocab, the sou / sub_token id of
 *      its copy slot above, as fira_beam_select resolves it), len + 1 and p_out[m] = the entry's value; where fewer than k
 *      entries are positive the remaining slots are void: gen[j*] unchanged, p_out = -1.
 *   parent[r] = b * k + j* for every row of the commit.
 * A commit with ended[b] != 0, or with no live slot (it is marked ended), is copied through: gen, len, p, prob unchanged,
 * parent = the row itself, hist untouched.  pick_out [B] (j*, or -1 for a commit copied through), sim_out and score_out [B*k]
 * (0 for void slots and commits copied through) are optional.  alpha = 0 is greedy search over the same rows.
 * 2 <= k <= 8, 2 <= tar_len <= 64, 0 <= step <= tar_len - 2, vocab in 9 .. 25 600, sou_len + sub_len <= 1 024, alpha finite
 * in [0, 1]; anything else returns non-zero with the reason in fira_last_error() and nothing is launched.  One workgroup of
 * 1 024 threads per commit: wave j forms slot j's cosines with DPP reductions, then the ONE picked row of dist is streamed;
 * vector stores only, no global atomics.                                                                                */
int fira_contrastive_select(void* stream, const fira_dims* d, int B, int k, int step, float alpha, const float* dist,
                            const float* hidden /* [B*k, 256] */, const int32_t* finished, const int32_t* sou,
                            const int32_t* sub_token, const int32_t* gen_in, const int32_t* len_in, const float* p_in /* [B*k] */,
                            const float* prob_in /* [B] */, float* hist /* [B, tar_len, 256], read and appended */,
                            int32_t* ended /* [B] */, int32_t* gen_out, int32_t* len_out, float* p_out, float* prob_out,
                            int32_t* parent, int32_t* pick_out /* [B] or NULL */, float* sim_out /* [B*k] or NULL */,
                            float* score_out /* [B*k] or NULL */);

/* Greedy search bookkeeping (the same loop at beam 1 without the [B, vocab+S] distribution): consumes the arg-max
 * index / probability fira_decode_step wrote, resolves copy indices through sou / sub_token, appends the id at
 * out[b, step+1], multiplies prob, bumps length, clears alive[b] at <eos>, writes the next step's input ids to `tokens`
 * (0 for ended hypotheses) and adds the number of still-running hypotheses to n_alive[step] (caller zeroes n_alive
 * [tar_len] before the first step).  run_model.py:305-340 with beam_size 1.                                       */
int fira_greedy_advance(void* stream, const fira_dims* d, int B, int step, const int32_t* best_id, const float* best_p,
                        const int32_t* sou, const int32_t* sub_token, int32_t* out, int32_t* length, float* prob,
                        int32_t* alive, int32_t* tokens, int32_t* n_alive);

/* Search constraints (csrc/constrain.hip; additive, the ABI version is unchanged): edits the step's distribution in place
 * between fira_decode_step and fira_beam_select / fira_greedy_advance.  W = vocab + sou_len + sub_len; entry i resolves to the
 * word w(i) = i below vocab, sou[b, i - vocab] below vocab + sou_len, sub_token[b, i - vocab - sou_len] above, as the two
 * selection kernels resolve it (b = r / rows_per_commit: n_beam for a beam search, 1 for greedy).  The hypothesis of row r is
 * h_1 .. h_m = gen[r, 1 .. length[r] - 1], m = length[r] - 1 (<start> at position 0 is not counted; ids at or past length are
 * ignored; length is clamped to 1 .. tar_len).  A row with gen[r, length[r] - 1] == <eos> (1) is finished: its dist is left
 * untouched.  For every other row the blocked words are the union of
 *   ban        every banned[k] inside [0, vocab) (ids outside are ignored; the Python layer rejects them)
 *   no-repeat  for n = no_repeat_ngram >= 1: every h_{j+n-1} with 1 <= j and j + n - 1 <= m whose predecessors h_j .. h_{j+n-2}
 *              equal the last n - 1 words h_{m-n+2} .. h_m (n = 1: every word emitted so far; nothing while m < n; the tail
 *              never matches itself as a completed n-gram: j + n - 1 <= m is the whole condition); 0 = off
 *   min length <eos> while m < min_length
 * and every entry i with w(i) blocked -- the generator id and every copy slot that carries the word -- is set to exactly 0.0f.
 * Every other element keeps its bits; nothing is renormalised (the search ranks products of probabilities: a zero loses).
 * best_id / best_p (both NULL, or both [R]): the arg-max entry of the EDITED row and its value, under fira_decode_step_ex's rule
 * for its own best_id: the largest value, the lowest entry index among equals (there: the first maximum within the generator
 * part, the first within the copy part, the generator part on a tie between the two).  With every constraint off they equal
 * the step's own bit for bit (a finished row reports the arg-max of its untouched row); NaN never wins.  A row whose every
 * positive entry is blocked is not special-cased: all its candidates tie at 0 and the tie rule decides -- entry 0 here, the
 * lowest flattened index in fira_beam_select.  Without best_id the row is not read, only the blocked entries are stored.
 * tar_len <= 64, vocab <= 25 600, sou_len + sub_len <= 1 024 (the limits of fira_decode_step_sample / _score),
 * 0 <= no_repeat_ngram <= tar_len, 0 <= min_length <= tar_len - 2, 0 <= n_banned <= 32, rows_per_commit >= 1 divides R;
 * R == 0 is a no-op.  Any row width and pitch alignment; vector stores only, no atomics on global memory.                  */
int fira_constrain_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen /* [R, tar_len] */,
                        const int32_t* length /* [R] */, const int32_t* sou /* [R / rows_per_commit, sou_len] */,
                        const int32_t* sub_token /* [R / rows_per_commit, sub_len] */, int no_repeat_ngram, int min_length,
                        const int32_t* banned /* device, [n_banned] */, int n_banned,
                        float* dist /* [R, vocab + sou_len + sub_len], in place */,
                        int32_t* best_id, float* best_p /* both NULL or both given */);

/* Search over words (csrc/merge.hip; additive, the ABI version is unchanged): folds the copy entries of the step's distribution
 * into the generator entry of their word, in place, between fira_decode_step and the selection (fira_constrain_dist, if any, then
 * fira_beam_select / fira_greedy_advance).  W = vocab + sou_len + sub_len; row r belongs to commit b = r / rows_per_commit
 * (n_beam for a beam search, 1 for greedy); slot s in [0, sou_len + sub_len) has the source id w_s = sou[b, s] below sou_len,
 * sub_token[b, s - sou_len] above -- the id the selection kernels resolve entry vocab + s to.  Two entries with one id are one
 * continuation (only the id reaches the hypothesis and the next step), so for every id w in [0, vocab) that is the source of at
 * least one slot, with its slots s_1 < s_2 < ... < s_k in ascending slot index:
 *     acc        = ((p[vocab + s_1] + p[vocab + s_2]) + ...) + p[vocab + s_k]
 *     dist[r, w] = acc + dist[r, w]                      (the generator entry is added last, as fira_decode_step_score's p_word)
 *     dist[r, vocab + s_j] = 0.0f                        for j = 1 .. k
 * in plain fp32 additions in exactly this order: no float atomics, no tree reduction, so every run and every graph replay gives
 * the same bits (a loop of np.float32 additions is the reference).  Every other element keeps its bits: generator entries that
 * no slot carries, and slots whose id is outside [0, vocab) -- such an id is never used as an index.  Nothing is renormalised;
 * the row's mass is conserved up to the rounding of the additions.  A masked or padded slot holds exactly 0.0f and may carry
 * id 0 or a stale id: it takes part like any other slot and changes nothing, since x + 0.0f == x for x >= 0.
 * best_id / best_p (both NULL, or both [R]): the arg-max of the row AS STORED and its value, under (value descending, index
 * ascending) -- the order of fira_constrain_dist; NaN never wins.  After the edit the winner is a generator index whenever a
 * word has positive mass.  Without best_id the generator part of the row is not streamed: only the slots, and the generator
 * entries they fold into, are touched.  A finished or ended row is not special-cased (fira_beam_select and fira_greedy_advance
 * ignore such rows).  vocab in 4 .. 25 600, sou_len + sub_len <= 1 024, rows_per_commit >= 1 divides R; R == 0 is a no-op.
 * Any row width and pitch alignment; vector stores only, no atomics on global memory.                                    */
int fira_merge_dist(void* stream, const fira_dims* d, int R, int rows_per_commit,
                    const int32_t* sou /* [R / rows_per_commit, sou_len] */,
                    const int32_t* sub_token /* [R / rows_per_commit, sub_len] */,
                    float* dist /* [R, vocab + sou_len + sub_len], in place */,
                    int32_t* best_id, float* best_p /* both NULL or both given */);

/* Prefix-forced search (csrc/force.hip; additive, the ABI version is unchanged): cuts the step's distribution down to the word a
 * given message start asks for, in place, between fira_decode_step (fira_mix_dist, fira_merge_dist, if any) and fira_constrain_dist,
 * if any, then the selection.  The mirror image of fira_constrain_dist, with its definitions: W = vocab + sou_len + sub_len, entry i
 * resolves to the word w(i), row r belongs to commit b = r / rows_per_commit, len = length[r] clamped to 1 .. tar_len, m = len - 1
 * words emitted, and a row with gen[r, len - 1] == <eos> (1) is finished.  prefix[b, 0 .. prefix_len[b]) are the words the commit's
 * message begins with (no <start>); a negative prefix_len counts as 0, one above tar_len as tar_len.
 *   forced row   not finished and m < min(prefix_len[b], tar_len); its word is y = prefix[b, m].  Every entry i with w(i) != y is
 *                set to exactly +0.0f; every entry with w(i) == y keeps its bits: the generator entry y if 0 <= y < vocab, and every
 *                copy slot that carries y.  Nothing is renormalised.  A y outside [0, vocab) is never used as an index: it matches
 *                slots only (and, where no slot carries it, leaves an all-zero row).
 *   other rows   untouched.
 * best_id / best_p (both NULL, or both [R]): the arg-max of the row as it stands after the edit and its value, under (value
 * descending, index ascending) -- the order of fira_constrain_dist; NaN never wins.  A forced row whose kept entries are all 0
 * reports entry 0 (every candidate ties at 0).  Where no row is forced they equal the step's own bit for bit.  A forced row is not
 * read beyond its kept entries: its arg-max needs only those, and its zeros are plain stores (16-byte ones where the address allows,
 * 4-byte ones at the row's edges and around a kept entry).  A row that is not forced is read once with best_id, else not at all.
 * prefix and prefix_len are DEVICE arrays read when the kernel runs, so one captured launch serves every prefix.
 * tar_len <= 64, vocab in 4 .. 25 600, sou_len + sub_len <= 1 024, rows_per_commit >= 1 divides R; R == 0 is a no-op.  Any row
 * width and any 4-byte alignment of dist; vector stores only, no atomics on global memory.                                    */
int fira_force_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen /* [R, tar_len] */,
                    const int32_t* length /* [R] */, const int32_t* sou /* [R / rows_per_commit, sou_len] */,
                    const int32_t* sub_token /* [R / rows_per_commit, sub_len] */,
                    const int32_t* prefix /* device, [R / rows_per_commit, tar_len]: words only, no <start> */,
                    const int32_t* prefix_len /* device, [R / rows_per_commit] */,
                    float* dist /* [R, vocab + sou_len + sub_len], in place */,
                    int32_t* best_id, float* best_p /* both NULL or both [R] */);

/* Soft word penalties and biases (csrc/penalise.hip; additive, the ABI version is unchanged): multiplies the entries of words the
 * hypothesis already holds, and of a commit's biased words, by given factors, in place, LAST in the edit chain -- after
 * fira_merge_dist, fira_force_dist and fira_constrain_dist, if any, and before the selection.  The soft sibling of
 * fira_constrain_dist, with its definitions: W = vocab + sou_len + sub_len, entry i resolves to the word w(i), row r belongs to
 * commit b = r / rows_per_commit, len = length[r] clamped to 1 .. tar_len, m = len - 1 words emitted, and a row with
 * gen[r, len - 1] == <eos> (1) is finished: it is not touched.  For every other row, with c(w) = the number of positions p in
 * 1 .. m with gen[r, p] == w:
 *   count   every entry i with c(w(i)) > 0:  dist[r, i] <- fl32(dist[r, i] * count_factor[c(w(i))])   (c <= tar_len - 1, so the
 *           index is inside the table; count_factor[0] is never read)
 *   bias    then every entry i whose word equals bias_id[b, q] for some q < min(max(n_bias[b], 0), 16):
 *           dist[r, i] <- fl32(dist[r, i] * bias_factor[b, q]), for the first such q, once
 * The two fp32 multiplications round separately, in that order.  A word is reached through its generator entry and through every
 * diff and sub-token slot of the commit that carries it (fira_decode_step_score's p_word notion); <eos> is no exception.  Every
 * other element keeps its bits; nothing is renormalised.
 * The entry cannot see the contents of the device buffers.  The HOST guarantees: every factor finite and >= 0 (a 0 bans the word
 * as fira_constrain_dist would), the ids of a commit pairwise distinct and inside [0, vocab), n_bias in 0 .. 16.  Otherwise the
 * kernel clamps n_bias to 0 .. 16, ignores a bias id outside [0, vocab), and uses the first of two equal ids; factors are
 * multiplied in as they are.
 * best_id / best_p (both NULL, or both [R]): the arg-max of the row as it then stands and its value, under (value descending,
 * index ascending) -- the order of fira_constrain_dist; NaN never wins.  A finished row reports the arg-max of its untouched row.
 * Without best_id the row is read at its copy slots and at the touched generator entries only.
 * count_factor, bias_id, bias_factor and n_bias are DEVICE arrays read when the kernel runs, so one captured launch serves every
 * penalty value and every bias list.  tar_len in 2 .. 64, vocab in 4 .. 25 600, sou_len + sub_len <= 1 024, rows_per_commit >= 1
 * divides R; R == 0 is a no-op.  Any row width and any 4-byte alignment of dist; vector stores only, no atomics on global memory,
 * no two threads write one address.                                                                                          */
int fira_penalise_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen /* [R, tar_len] */,
                       const int32_t* length /* [R] */, const int32_t* sou /* [R / rows_per_commit, sou_len] */,
                       const int32_t* sub_token /* [R / rows_per_commit, sub_len] */,
                       const float* count_factor /* device, [tar_len] */,
                       const int32_t* bias_id /* device, [R / rows_per_commit, 16] */,
                       const float* bias_factor /* device, [R / rows_per_commit, 16] */,
                       const int32_t* n_bias /* device, [R / rows_per_commit] */,
                       float* dist /* [R, vocab + sou_len + sub_len], in place */,
                       int32_t* best_id, float* best_p /* both NULL or both [R] */);

/* Banned phrases (csrc/phrase.hip; additive, the ABI version is unchanged): blocks the word that would complete a listed n-gram, in
 * place, in the edit chain after fira_constrain_dist and before fira_penalise_dist.  fira_constrain_dist's definitions: W = vocab +
 * sou_len + sub_len, entry i resolves to the word w(i), row r belongs to commit b = r / rows_per_commit, len = length[r] clamped to
 * 1 .. tar_len, m = len - 1 words h_1 .. h_m emitted (prefix words included), and a row with gen[r, len - 1] == <eos> (1) is
 * finished: it is not touched.  Commit b lists n = n_phrases[b] (clamped to 0 .. 8) phrases; phrase q is the l = phrase_len[b, q]
 * words phrase[b, q, 0 .. l); a phrase with l outside 2 .. 4 is ignored.  For every other row and every phrase (w_1 .. w_l):
 *     if m >= l - 1 and (h_{m-l+2} .. h_m) == (w_1 .. w_{l-1}), the word w_l is blocked
 * and every entry i with w(i) blocked -- the generator id and every diff and sub-token slot that carries the word -- is set to
 * exactly 0.0f.  Every other element keeps its bits; nothing is renormalised.  A blocked word outside [0, vocab) is never used as an
 * index: it matches slots only.
 * best_id / best_p (both NULL, or both [R]): the arg-max of the row as it then stands and its value, under (value descending,
 * index ascending) -- the order of fira_constrain_dist; NaN never wins.  Without best_id the row is not read.
 * phrase, phrase_len and n_phrases are DEVICE arrays read when the kernel runs, so one captured launch serves every list.
 * tar_len in 2 .. 64, vocab in 4 .. 25 600, sou_len + sub_len <= 1 024, rows_per_commit >= 1 divides R; R == 0 is a no-op.  Any row
 * width and any 4-byte alignment of dist; vector stores only, no atomics on global memory.                                     */
int fira_ban_phrases_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen /* [R, tar_len] */,
                          const int32_t* length /* [R] */, const int32_t* sou /* [R / rows_per_commit, sou_len] */,
                          const int32_t* sub_token /* [R / rows_per_commit, sub_len] */,
                          const int32_t* phrase /* device, [R / rows_per_commit, 8, 4] */,
                          const int32_t* phrase_len /* device, [R / rows_per_commit, 8] */,
                          const int32_t* n_phrases /* device, [R / rows_per_commit] */,
                          float* dist /* [R, vocab + sou_len + sub_len], in place */,
                          int32_t* best_id, float* best_p /* both NULL or both [R] */);

/* Template-constrained search (csrc/template.hip; additive, the ABI version is unchanged): a deterministic
 * automaton over word classes says which words may come next, in place, in the edit chain after fira_ban_phrases_dist and before
 * fira_penalise_dist.  fira_constrain_dist's definitions: W, w(i), b = r / rows_per_commit, len = length[r] clamped to
 * 1 .. tar_len, m = len - 1 words h_1 .. h_m emitted, and a row with gen[r, len - 1] == <eos> (1) is finished: it is not touched.
 * The tables, at most 32 states and 32 classes:
 *     word_class[vocab]  the class of every vocabulary id (the low five bits of the byte); an id outside [0, vocab), in the
 *                        hypothesis or in a copy slot, has class 0
 *     next[32 * 32]      next[s * 32 + c]: the state after a word of class c in state s, -1 for none (a value of 32 or more: -1)
 *     need[32]           the fewest words from state s to an accepting state; 0 says that s accepts
 *     start[R / rows_per_commit]   the start state of every commit (a value outside 0 .. 31: -1)
 * For every other row: s = start[b], then s = next[s][class(h_p)] for p = 1 .. m, and -1 stays -1; left = tar_len - 1 - len, the
 * positions that stay free after this step's word.  The word w is blocked iff
 *     s == -1,   or   w == <eos> and need[s] != 0,   or   w != <eos> and (s' = next[s][class(w)]) == -1 or need[s'] > left
 * and every entry i with w(i) blocked -- the generator id and every diff and sub-token slot that carries the word -- is set to
 * exactly 0.0f.  Every other element keeps its bits; nothing is renormalised.  A row in which every one of the 32 classes is allowed
 * and <eos> is free is not edited; without best_id it is not read either (so the host fills the columns of unused classes with
 * class 0's column: the accept-everything template then costs the launch and the walk).
 * best_id / best_p (both NULL, or both [R]): the arg-max of the row as it then stands and its value, under (value descending,
 * index ascending) -- the order of fira_constrain_dist; NaN never wins; an all-zero row reports entry 0 with 0.  Without best_id
 * the row is not read.
 * The four tables are DEVICE arrays read when the kernel runs, so one captured launch serves every template; word_class and next
 * may have any alignment (aligned dwords that overlap the table are read, no other).
 * tar_len in 2 .. 64, vocab in 4 .. 25 600, sou_len + sub_len <= 1 024, rows_per_commit >= 1 divides R; R == 0 is a no-op.  Any row
 * width and any 4-byte alignment of dist; vector stores only, no atomics on global memory.                                     */
int fira_template_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen /* [R, tar_len] */,
                       const int32_t* length /* [R] */, const int32_t* sou /* [R / rows_per_commit, sou_len] */,
                       const int32_t* sub_token /* [R / rows_per_commit, sub_len] */,
                       const uint8_t* word_class /* device, [vocab] */, const int8_t* next /* device, [32 * 32] */,
                       const int32_t* need /* device, [32] */, const int32_t* start /* device, [R / rows_per_commit] */,
                       float* dist /* [R, vocab + sou_len + sub_len], in place */,
                       int32_t* best_id, float* best_p /* both NULL or both [R] */);

/* Per-commit word sets (csrc/wordset.hip; additive, the ABI version is unchanged): allow, deny, boost and
 * ground, each a vocabulary-sized bit set per commit, in place, in the edit chain after fira_template_dist and before
 * fira_penalise_dist.  fira_constrain_dist's definitions: W, w(i), b = r / rows_per_commit, len = length[r] clamped to
 * 1 .. tar_len, and a row with gen[r, len - 1] == <eos> (1) is finished: it is not touched.
 * allow, deny, boost, ground: each NULL (not given) or [R / rows_per_commit, ceil(vocab / 32)] uint32; bit w % 32 of word w / 32
 * says that id w is in the set; the bits at or past vocab in the last word are ignored.
 * slot_valid [R / rows_per_commit, ceil((sou_len + sub_len) / 32)] uint32: bit j says that copy slot j (diff positions, then
 * sub-token positions) can be given mass by the copy head; required with ground.  boost_factor [R / rows_per_commit], finite and
 * >= 0 (the host's promise); required with boost.
 *     in(S, w)       S is given, 0 <= w < vocab and the bit is set
 *     carried(b, w)  some VALID slot of commit b has the source id w
 * For every other row the word w is blocked iff
 *     allow is given and w != <eos> and !in(allow, w),   or   in(deny, w),   or   in(ground, w) and !carried(b, w)
 * An id outside [0, vocab) is in no set: blocked under allow, untouched by deny and ground, never used as an index.  Every entry i
 * with w(i) blocked -- the generator id and every diff and sub-token slot that carries the word -- is set to exactly +0.0f.  Every
 * entry that is not blocked and has in(boost, w(i)) becomes fl32(dist[i] * boost_factor[b]): one multiplication, applied once, the
 * last of this link's edits.  Every other element keeps its bits; nothing is renormalised.
 * best_id / best_p (both NULL, or both [R]): the arg-max of the row as it then stands and its value, under (value descending,
 * index ascending) -- the order of fira_constrain_dist; NaN never wins; an all-zero row reports entry 0 with 0.  Without best_id
 * an allowed and unboosted entry is neither read nor written.
 * Every input is a DEVICE array read when the kernel runs, so one captured launch serves every set; which sets are given (NULL or
 * not) is part of the launch.
 * tar_len in 2 .. 64, vocab in 4 .. 25 600, sou_len + sub_len <= 1 024, rows_per_commit >= 1 divides R; R == 0 is a no-op.  Any row
 * width and any 4-byte alignment of dist; vector stores only, no atomics on global memory, no two threads write one address. */
int fira_wordset_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen /* [R, tar_len] */,
                      const int32_t* length /* [R] */, const int32_t* sou /* [R / rows_per_commit, sou_len] */,
                      const int32_t* sub_token /* [R / rows_per_commit, sub_len] */,
                      const uint32_t* allow, const uint32_t* deny, const uint32_t* boost,
                      const uint32_t* ground /* device, each NULL or [R / rows_per_commit, ceil(vocab / 32)] */,
                      const uint32_t* slot_valid /* device, [R / rows_per_commit, ceil((sou_len + sub_len) / 32)] */,
                      const float* boost_factor /* device, [R / rows_per_commit] */,
                      float* dist /* [R, vocab + sou_len + sub_len], in place */,
                      int32_t* best_id, float* best_p /* both NULL or both [R] */);

/* Ensemble decoding (csrc/mix.hip; additive, the ABI version is unchanged): mixes the step distributions of n_members models into
 * one, between the members' fira_decode_step calls and whatever takes a distribution next (fira_merge_dist, fira_constrain_dist,
 * fira_beam_select / fira_beam_select_scored / fira_greedy_advance).  For every element i of the [R, W] rows, in member order,
 * every multiply and every add rounded to fp32 on its own (no fused multiply-add):
 *     acc = weights[0] * dists[0][i];   acc = acc + weights[1] * dists[1][i];   ...   out[i] = acc
 * so a loop of np.float32 operations is the reference and every run and every graph replay gives the same bits.  Nothing is
 * renormalised: with weights that sum to 1 the mix of distributions is a distribution up to rounding.  dists and weights are HOST
 * arrays read at launch; the pointers and the weights travel as kernel arguments, so a captured launch bakes them in.
 * out may be dists[0] (in place over member 0); any other overlap of out with a member is refused.
 * best_id / best_p (both NULL, or both [R]): the arg-max of the row AS STORED and its value, under (value descending, index
 * ascending) -- the order of fira_merge_dist and fira_constrain_dist; NaN never wins.  Without best_id no reduction runs.
 * 2 <= n_members <= 8, W >= 1, every weight finite and >= 0 (else non-zero with the reason in fira_last_error(), nothing
 * launched); R == 0 is a no-op.  Any row width and any 4-byte alignment of any pointer (16-byte accesses where the addresses
 * allow, 4-byte ones at the edges); vector stores only, no atomics on global memory.                                          */
int fira_mix_dist(void* stream, int R, int W, int n_members,
                  const float* const* dists /* HOST array of n_members device pointers, each [R, W] contiguous */,
                  const float* weights /* HOST array of n_members floats */,
                  float* out /* [R, W]; may be dists[0] */,
                  int32_t* best_id, float* best_p /* both NULL or both [R] */);

/* Retrieval-augmented search (csrc/retrieve.hip; additive, the ABI version is unchanged): the nearest
 * training commit's step distribution mixed into the input's (CoRec, Wang et al. 2021).
 *
 *   fira_pool_memory : the vector of every commit of a decode workspace.  mem [B, sou_len + sub_len, 256] and mem_valid
 *     [B, sou_len + sub_len] are fira_decode_memory / fira_decode_mem_valid (n_beam = 1 layout: one block of rows per commit).
 *         v[b, c] = (sum over s with mem_valid[b, s] != 0, ascending s, of mem[b, s, c]) / n_b        n_b = the number of such rows
 *         ss[b]   = ((v[b,0] v[b,0] + v[b,1] v[b,1]) + ...) in ascending c, every multiply and add rounded to fp32 on its own
 *         out[b, c] = v[b, c] / sqrtf(ss[b])
 *     each one IEEE fp32 operation, so a loop of np.float32 operations is the reference, bit for bit.  n_b = 0 or ss = 0 (or a
 *     norm that is not a number): out[b, :] = 0.  Rows with mem_valid == 0 are never read (the workspace leaves them stale).
 *     B == 0 is a no-op.
 *
 *   fira_nn_search : for each of B <= 64 queries Q[b] the store row with the largest dot product,
 *         best_idx[b] = argmax over j in [0, N), j != exclude[b], of <Q[b], store[j]>        (ties: the lowest j)
 *         best_sim[b] = that product clamped to [0, 1]
 *     in ONE pass over the store (tiles of 16 rows x all queries on the fp32 matrix cores, queries in LDS); no [B, N] scores
 *     touch memory.  The product of a (query, row) pair is one ordered fp32 fma chain over k = 0 .. 255 in a fixed permutation
 *     that does not depend on j, so identical store rows tie exactly; |product - exact| <= 256 * 2^-24 * sum |q_k s_k|.  A product
 *     that is NaN never wins; a query whose every admissible product is NaN gets best_idx = -1, best_sim = 0.  exclude (NULL, or
 *     DEVICE [B], -1 = nothing) is read when the kernel runs.  scratch: fira_nn_search_scratch_bytes(B, N) bytes (0 for
 *     arguments fira_nn_search refuses), 8-byte aligned, holding the workgroups' partial winners between the two launches.
 *     Refused with the reason in fira_last_error() and nothing launched: B <= 0, B > 64, N <= 0, exclude with N < 2 (it may leave
 *     no row), a null or misaligned pointer (Q and store 16-byte aligned), a scratch that is too small.
 *
 *   fira_mix_neighbour : between fira_decode_step (+ fira_merge_dist on q with the NEIGHBOUR's sou / sub_token rows) and the edit
 *     chain of the input.  W = vocab + sou_len + sub_len; row r belongs to commit b = r / rows_per_commit; (a, c) = coef[b, 0..1]:
 *         dist[r, i] = a * dist[r, i]                            for vocab <= i < W     (the input's own copy entries)
 *         dist[r, w] = (a * dist[r, w]) + (c * q[r, w])          for 0 <= w < vocab
 *     every multiply and add rounded to fp32 on its own (no fused multiply-add).  q's entries from vocab on are not read: the
 *     neighbour's copy slots refer to the neighbour's diff and reach the mix as words only, through the merge.  coef is a DEVICE
 *     array read when the kernel runs (one captured launch serves every batch); the host forms a = 1 / (1 + lambda sim),
 *     c = lambda sim / (1 + lambda sim), so a + c = 1 and the row stays normalised.  With (a, c) = (1, 0) and a finite q every
 *     element keeps its bits (-0.0 becomes +0.0).  best_id / best_p (both NULL, or both [R]): the arg-max of the row AS STORED and
 *     its value, in the order of fira_mix_dist; NaN never wins.  q must not overlap dist (refused).  Geometry limits of
 *     fira_merge_dist; any 4-byte alignment of q and dist; R == 0 is a no-op.  Vector stores only, no atomics.                    */
int fira_pool_memory(void* stream, const fira_dims* d, int B, const float* mem, const int32_t* mem_valid,
                     float* out /* [B, 256] */);
size_t fira_nn_search_scratch_bytes(int B, int N);
int fira_nn_search(void* stream, const float* Q /* [B, 256] */, int B, const float* store /* [N, 256] */, int N,
                   const int32_t* exclude /* device [B] or NULL */, int32_t* best_idx /* [B] */, float* best_sim /* [B] */,
                   void* scratch, size_t scratch_bytes);
int fira_mix_neighbour(void* stream, const fira_dims* d, int R, int rows_per_commit,
                       const float* coef /* device, [R / rows_per_commit, 2] */,
                       const float* q /* [R, vocab + sou_len + sub_len], merged with the neighbour's ids */,
                       float* dist /* [R, vocab + sou_len + sub_len], in place */,
                       int32_t* best_id, float* best_p /* both NULL or both [R] */);

/* Token-level retrieval for the search: kNN-MT (Khandelwal et al., ICLR 2021; the numpy statement:
 * tests/knn_ref.py).  Additive, the ABI version is unchanged.  The store holds one row per training token: keys [N, 256] (the
 * decoder's last hidden state, fira_decode_hidden, before that token was written), key_sq [N] (the row's sum of squares in
 * ascending column order, every operation rounded to fp32), values [N] (the vocabulary id written there) and owner [N] (the
 * commit the row comes from).
 *
 *   fira_knn_search : for each of R >= 0 queries Q[r] the K (1..16) stored rows with the smallest
 *         s_j = key_sq[j] - 2 <Q[r], keys[j]>                                  (ties: the lowest j; NaN never wins)
 *     over the rows with owner[j] != exclude[r] (owner NULL, exclude NULL or exclude[r] = -1: every row), best first:
 *         idx_out[r, k] = j        d2_out[r, k] = max(0, q_sq[r] + s_j)        q_sq as key_sq, over Q[r]
 *     and idx = -1, d2 = +inf in the slots past the number of admissible rows.  The product is one ordered fp32 chain over
 *     k = 0 .. 255 in a fixed permutation that does not depend on j (fira_nn_search's), so identical keys tie exactly.  One pass
 *     over the store serves a block of up to 64 queries (tiles of 16 rows x the block's queries on the fp32 matrix cores, the
 *     queries in LDS, a partial top-K per query and workgroup); a second launch merges the partials in the same order.  No
 *     [R, N] matrix touches memory.  N <= 8 388 608; row offsets are size_t.  exclude (DEVICE [R]) is read when the kernel
 *     runs.  scratch: fira_knn_search_scratch_bytes(R, N, K) bytes (0 for R = 0 and for arguments fira_knn_search refuses),
 *     8-byte aligned.  Refused with the reason in fira_last_error() and nothing launched: R < 0, N <= 0, N above the limit, K
 *     outside 1..16, exclude without owner, a null or misaligned pointer (Q and keys 16-byte aligned), a scratch that is too
 *     small.  R == 0 is a no-op.  No global atomics, vector stores only, capturable.
 *
 *   fira_mix_knn : between fira_decode_step (and fira_decode_hidden + fira_knn_search) and the edit chain.  W = vocab + sou_len +
 *     sub_len; (lam, inv_T) = coef[0..1], a DEVICE array read when the kernel runs (one captured launch serves every value).
 *     Over the slots with 0 <= idx[r, k] < N (the others are void):
 *         w_k = expf(-(d2[r, k] - d2[r, 0]) * inv_T) / (the sum of these over the non-void slots, ascending k)
 *         dist[r, i] = (1 - lam) * dist[r, i]                                  for every i
 *         dist[r, values[idx[r, k]]] += lam * w_k                              for k = 0 .. K - 1, in this order
 *     every multiply and add rounded to fp32 on its own; nothing is renormalised (the weights sum to 1).  lam == 0, and a row
 *     whose slots are all void: no element of the row is written.  best_id / best_p (both NULL, or both [R]): the arg-max of
 *     the row AS STORED and its value, in the order of fira_mix_dist.  Geometry limits of fira_merge_dist; any 4-byte alignment
 *     of dist; R == 0 is a no-op.                                                                                                 */
size_t fira_knn_search_scratch_bytes(int R, int N, int K);
int fira_knn_search(void* stream, const float* Q /* [R, 256] */, int R, const float* keys /* [N, 256] */,
                    const float* key_sq /* [N] */, const int32_t* owner /* [N] or NULL */,
                    const int32_t* exclude /* device [R] or NULL */, int N, int K, int32_t* idx_out /* [R, K] */,
                    float* d2_out /* [R, K] */, void* scratch, size_t scratch_bytes);
int fira_mix_knn(void* stream, const fira_dims* d, int R, const int32_t* idx /* [R, K] */, const float* d2 /* [R, K] */,
                 const int32_t* values /* [N] */, int N, int K, const float* coef /* device [2]: lam, inv_T */,
                 float* dist /* [R, vocab + sou_len + sub_len], in place */, int32_t* best_id, float* best_p /* both NULL or both [R] */);

/* On-device sampling of candidate messages (temperature, top-k, top-p).  Workspace: fira_decode_begin_ex /
 * fira_decode_workspace_bytes_ex with n_beam = n_sample (1..8) and the same flags (FIRA_DECODE_KV_BF16 allowed).
 *   fira_decode_step_sample : fira_decode_step_ex for the B * n_sample rows (row r = commit r / n_sample, sample
 *     r % n_sample; rows never change parent, so there is no cache permutation), then per row: the distribution p over
 *     vocab + S entries (dist[r, :] if dist != NULL, bit-identical to fira_decode_step's), the filters -- temperature
 *     T > 0 and finite: q ~ p^(1/T); top_k (0 = off, <= vocab + S): keep p >= the k-th largest p counted with
 *     multiplicity; top_p (in (0, 1], 1 = off): renormalise q over what top-k kept and keep q >= the largest v whose
 *     upper set {q >= v} holds at least top_p of the mass; ties at either threshold are kept -- and the Gumbel-max draw
 *     best_id[r] = argmax over kept i of (log p_i / T + g_i), lowest index on ties, with the counter-hash noise
 *       base   = mix32(key[b] ^ mix32((uint32)seed ^ mix32((uint32)(seed >> 32) + 0x632BE5AB)))
 *       stream = mix32(base + 0x9E3779B9 * (uint32)(j * tar_len + step + 1))        (b = r / n_sample, j = r % n_sample)
 *       u      = min(((mix32(i ^ stream) >> 8) + 0.5f) * 2^-24, largest float below 1),  g_i = -log(-log(u))
 *     (mix32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16).  key [B] int32 per commit,
 *     seed_dev a DEVICE uint64 read when the kernel runs (one captured graph serves every seed).  best_p[r] = p_{best_id}
 *     (unfiltered, untempered), bit-identical to dist[r, best_id[r]].  Shapes beyond vocab 25 600 / S 1 024: error.
 *   fira_sample_advance : fira_greedy_advance over the B * n_sample rows (copy ids resolved through commit r / n_sample)
 *     that also adds logf(best_p[r]) to logp[r] for every id it appends.                                            */
int fira_decode_step_sample(void* stream, const fira_dims* d, const float* params, void* workspace,
                            size_t workspace_bytes, int B, int n_sample, int step, const int32_t* tokens,
                            const int32_t* key, const uint64_t* seed_dev, float temperature, int top_k, float top_p,
                            float* dist, int32_t* best_id, float* best_p, int flags);
/* Truncation samplers: fira_decode_step_sample with four more cuts of the row, applied after its filters.  Below, q is the
 * tempered distribution p^(1/T) renormalised over the entries top-k and then top-p kept, and H = -sum q ln q over them (an
 * entry with q = 0 contributes 0); sums are fixed-order fp32 block sums without atomics, as the filters' are.
 *     min_p     in [0, 1), 0 = off: keep q_i >= min_p * max q
 *     epsilon   in [0, 1), 0 = off: keep q_i >= epsilon                                  (epsilon sampling)
 *     eta       in [0, 1), 0 = off: keep q_i >= min(eta, sqrt(eta) * exp(-H))            (eta sampling)
 *     typical_p in (0, 1], 1 = off: with s_i = |-ln q_i - H|, keep s_i <= sigma, sigma the smallest value whose lower set
 *               {s_i <= sigma} holds at least typical_p of the mass (locally typical sampling; bisected over the bits of s)
 *   The first three are lower thresholds on q and so on p: together with top-k and top-p the largest one decides, ties at it
 *   are kept.  typical_p < 1 is a band in p, not a lower threshold: it combines with temperature and top_k only and is an
 *   error with top_p < 1, min_p, epsilon or eta.  Every cut keeps the row's maximum (with its ties), so no row is left empty;
 *   an entry with p = 0 is never kept.  The draw, best_id, best_p and dist are fira_decode_step_sample's; with
 *   (min_p, epsilon, eta, typical_p) = (0, 0, 0, 1) the call IS fira_decode_step_sample, bit for bit.  Values outside
 *   their range or not finite: error.                                                                                 */
int fira_decode_step_sample_cut(void* stream, const fira_dims* d, const float* params, void* workspace,
                                size_t workspace_bytes, int B, int n_sample, int step, const int32_t* tokens,
                                const int32_t* key, const uint64_t* seed_dev, float temperature, int top_k, float top_p,
                                float min_p, float epsilon, float eta, float typical_p, float* dist, int32_t* best_id,
                                float* best_p, int flags);
int fira_sample_advance(void* stream, const fira_dims* d, int B, int n_sample, int step, const int32_t* best_id,
                        const float* best_p, const int32_t* sou, const int32_t* sub_token, int32_t* out, int32_t* length,
                        float* prob, float* logp, int32_t* alive, int32_t* tokens, int32_t* n_alive);

/* Sampling from the search's edited distribution (csrc/sample_row.hip; additive, the ABI version is
 * unchanged): the filters, cuts and Gumbel-max draw of fira_decode_step_sample_cut applied to rows that already exist in memory,
 * after fira_decode_step_ex (fira_mix_dist / fira_mix_neighbour) and the edit chain (fira_merge_dist, fira_force_dist,
 * fira_constrain_dist) and before fira_sample_advance.  W = vocab + sou_len + sub_len; row r belongs to commit
 * b = r / rows_per_commit and is its sample j = r % rows_per_commit; the noise is fira_decode_step_sample's, of (seed, key[b], j,
 * tar_len, step, entry).  dist is only read, at any 4-byte alignment.
 *   Definitions on an UNNORMALISED row (the edits renormalise nothing): those of fira_decode_step_sample_cut with every quantity
 *   taken relative to the row's own sums -- top-p keeps at least top_p of the mass top-k kept, q = w / Z over the kept entries, w
 *   relative to the row's largest entry as it stands (the block maximum, not the step's own maximum: an edit may have zeroed it).
 *   An entry with p = 0 is never kept and never drawn; with fewer than top_k positive entries top-k cuts nothing.  Scaling a row
 *   by a power of two changes neither the kept set nor the draw.
 *   best_id[r] the drawn entry, best_p[r] = dist[r, best_id[r]] bit for bit (edited, untempered, unfiltered: a word's probability
 *   after a merge, the mixed probability after a mix).  On the rows fira_decode_step_sample_cut stores (its dist argument) the
 *   pair equals that call's own, bit for bit.  Every row is written: a row without a positive entry gets what the edit chain's
 *   arg-max reports for it, best_id = 0 and best_p = 0.0f (fira_sample_advance then carries probability 0, log-probability -inf).
 *   Contract: entries finite and non-negative; on anything else the result is unspecified, but best_id stays inside [0, W) and
 *   nothing but best_id / best_p is written.
 * Refused with the reason in fira_last_error() and nothing launched or written: a null best_id or best_p, rows_per_commit outside
 * 1..8 or not dividing R, a negative step, vocab outside 4 .. 25 600 or sou_len + sub_len > 1 024, top_k outside 0..W, and the
 * argument ranges and combinations fira_decode_step_sample_cut refuses; with R > 0 a null dist, key or seed_dev.  R == 0 is a
 * no-op.  Vector stores only, no atomics on global memory.                                                                      */
int fira_sample_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, int step,
                     const float* dist /* [R, vocab + sou_len + sub_len], read only */,
                     const int32_t* key /* [R / rows_per_commit] */, const uint64_t* seed_dev,
                     float temperature, int top_k, float top_p, float min_p, float epsilon, float eta, float typical_p,
                     int32_t* best_id /* [R] */, float* best_p /* [R] */);

/* Teacher-forced scoring of given candidate messages: how probable is this message for this commit?  Workspace:
 * fira_decode_begin_ex / fira_decode_workspace_bytes_ex with n_beam = n_cand (1..8) and the same flags
 * (FIRA_DECODE_KV_BF16 allowed), so the encoder, the cross-attention K|V and LinearSource(memory) are computed once per
 * commit for all its candidates.
 *   fira_decode_step_score : fira_decode_step_ex for the B * n_cand rows (row r = commit r / n_cand, candidate
 *     r % n_cand; rows never change parent, so there is no cache permutation) fed with tokens[r] = the candidate's id at
 *     position `step`, then per row the distribution p over vocab + S entries (dist[r, :] if dist != NULL, bit-identical
 *     to fira_decode_step's) scored against target[r] = the candidate's id at position step + 1 (a vocabulary id; 0 =
 *     nothing to score at this step).  With the candidates stored step-major ([tar_len, B * n_cand]) tokens and target
 *     are two rows of one tensor: one call per step, no bookkeeping kernel.  Written for every row:
 *       p_word[r]     p[y] (y < vocab) + the sum of p[vocab + s] over the memory slots s that are valid and whose source id
 *                     (sou[b, s] for s < sou_len, sub_token[b, s - sou_len] above) is y: the probability of the WORD,
 *                     over every entry that resolves to it; summed in one fixed order without atomics
 *       p_entry[r], entry[r]   the largest single entry that resolves to y and its index (lowest index on ties; -1 and
 *                     0 when no entry resolves to y): what a search is credited with when it emits y
 *       copy_share[r] the copy part of p_word over p_word (0 when p_word == 0)
 *       p_label[r]    p[label[r]] for label[r] in [0, vocab + S) (an entry index; -1 = none -> 0); label, p_label and
 *                     logp_label are given together or all NULL
 *       top_id[r]     the row's arg-max entry, identical to fira_decode_step_ex's best_id
 *     and added to: logp_word[r], logp_entry[r], logp_label[r] += logf(max(p, 1e-10)) (the clamp of fira_head_loss) of
 *     p_word, p_entry and p_label.  Rows with target 0 get p_word = p_entry = copy_share = p_label = 0, entry = -1, and
 *     their sums are left alone.  Every single-entry value is bit-identical to dist[r, index].  sou [B, sou_len] and
 *     sub_token [B, sub_len] are the commit's id rows (as fira_greedy_advance takes them).  Shapes beyond vocab 25 600 /
 *     S 1 024: error.                                                                                                 */
int fira_decode_step_score(void* stream, const fira_dims* d, const float* params, void* workspace,
                           size_t workspace_bytes, int B, int n_cand, int step, const int32_t* tokens,
                           const int32_t* target, const int32_t* label, const int32_t* sou, const int32_t* sub_token,
                           float* dist, float* p_word, float* p_entry, int32_t* entry, float* copy_share, float* p_label,
                           int32_t* top_id, float* logp_word, float* logp_entry, float* logp_label, int flags);

/* Decoder.forward over all tar_len positions on caller-supplied memory [B, sou+sub, 256] / mem_valid [B, sou+sub]
 * (gnn_transformer.py:108-122; the call of run_model.py:256).  Workspace: fira_workspace_bytes(d, B, 0).          */
int fira_decoder_forward(void* stream, const fira_dims* d, const float* params, void* workspace,
                         size_t workspace_bytes, int B, const int32_t* tar, const float* memory,
                         const int32_t* mem_valid, float* out);

/* read-only views into a decode workspace (device pointers), for tests and the Python driver */
const float*   fira_decode_memory(const fira_dims* d, void* workspace, int B, int n_beam);
const int32_t* fira_decode_mem_valid(const fira_dims* d, void* workspace, int B, int n_beam);

/* The decoder's last hidden state of every row (additive, the ABI version is unchanged): copies the final LayerNorm output of
 * the last fira_decode_step* call on `workspace` -- the [B*n_beam, 256] input of the generator projection and of the copy
 * head -- into out (16-byte aligned).  B, n_beam and flags are those of the step call.  One copy launch of B*n_beam KB on
 * `stream`, capturable; the workspace is only read.  Non-zero with the reason in fira_last_error() on a bad argument or a
 * workspace that is too small, before any launch.                                                                       */
int fira_decode_hidden(void* stream, const fira_dims* d, void* workspace, size_t workspace_bytes, int B, int n_beam, int flags,
                       float* out /* [B*n_beam, 256] */);

/* ---- host-side helper (CPU only, no device work) -----------------------------------------------------------------
 * The index lists of fira_batch from one collated batch (int64 id arrays as the reference's Dataset.py produces them,
 * block-diagonal CSR with GLOBAL node ids b*N + local): computed nodes + compact CSR, code / memory rows, word-id
 * groups (items of at most `chunk` positions) and AST / edit (row, id) pairs.  Output arrays are caller-allocated at their
 * worst-case sizes: node_rows [B*N], rowptr_c [B*N+1], col_c / val_c [nnz], code_rows / code_mark [B*L],
 * mem_rows / mem_dst [B*(L+S)], item_tok [B*(L+S)], item_ptr [B*(L+S)+1], emb_rows [B*(L+S)], ast_rows / ast_ids
 * [B*(N-L-S)]; counts[7] = {n_nodes, nnz_c, n_code, n_mem, n_items, n_emb_rows, n_ast}.
 * Same result, bit for bit, as fira_icse_amd/model.py: computed_nodes + compact_embedding_lists (the specification).    */
int fira_host_node_lists(int B, int N, int L, int S, int skip_padding, const int64_t* sou, const int64_t* sub_token,
                         const int64_t* ast_change, const int64_t* mark, const int32_t* rowptr, const int32_t* col,
                         const float* val, int chunk, int32_t* node_rows, int32_t* rowptr_c, int32_t* col_c,
                         float* val_c, int32_t* code_rows, int32_t* code_mark, int32_t* mem_rows, int32_t* mem_dst,
                         int32_t* item_tok, int32_t* item_ptr, int32_t* emb_rows, int32_t* ast_rows, int32_t* ast_ids,
                         int32_t* counts);

/* Block-diagonal CSR of a batch from a store of per-commit CSR graphs (replaces Dataset.py:336-343's dense collate):
 * store_rowptr [n_commits, N+1], store_offset [n_commits+1] (prefix sums of the commits' nnz), store_col / store_val the
 * concatenated entries; rowptr [B*N+1], col (global node ids b*N + local) and val [sum nnz] are caller-allocated.   */
int fira_host_collate_csr(int B, int N, const int64_t* idx, int64_t n_commits, const int32_t* store_rowptr,
                          const int64_t* store_offset, const int32_t* store_col, const float* store_val,
                          int32_t* rowptr, int32_t* col, float* val);

#ifdef __cplusplus
}
#endif
#endif /* FIRA_HIP_H */
