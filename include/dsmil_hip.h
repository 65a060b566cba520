/*
 * dsmil_hip.h — C-ABI of libdsmil_hip.so: the MI355X (gfx950) implementation of the two DSMIL
 * hot paths.  Plain pointers and sizes only; every pointer named "device" is HBM memory owned
 * by the caller; nothing is allocated, freed or synchronised inside the library; all work is
 * enqueued on the HIP stream handed in (hipStream_t passed as void*), in order, and is
 * hipGraph-capturable.  Every function returns 0 on success or a negative DSMIL_E_* code;
 * dsmil_strerror() names it.  No C++ exceptions cross this boundary.
 *
 * The reference (binli123/dsmil-wsi) has no FFI of its own: its boundary is the nn.Module API of
 * dsmil.py.  Each entry point below therefore cites the reference forward it replaces, and
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 */
#ifndef DSMIL_HIP_H
#define DSMIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSMIL_ABI_VERSION 6
#define DSMIL_Q_DIM 128 /* query width hard-coded at dsmil.py:31,33 */

enum {
    DSMIL_OK = 0,
    DSMIL_E_INVALID = -1,     /* null pointer / non-positive size / bad flag           */
    DSMIL_E_UNSUPPORTED = -2, /* shape or dtype outside what the kernels implement      */
    DSMIL_E_WORKSPACE = -3,   /* workspace smaller than dsmil_*_workspace_bytes() says  */
    DSMIL_E_LAUNCH = -4,      /* hipGetLastError() != hipSuccess after a launch         */
    DSMIL_E_ALIGN = -5        /* a pointer is not aligned as the kernels require        */
};

enum { DSMIL_F32 = 0, DSMIL_BF16 = 1 };

/* Parameters of FCLayer + BClassifier, row-major fp32 device pointers, named after the
 * reference state_dict keys (dsmil.py:9,31,33,44):
 *   fc_w  [C,K]  fc_b [C]      i_classifier.fc.0.{weight,bias}      (may be NULL when the
 *                               caller supplies instance logits, see classes_in)
 *   q0_w  [128,K] q0_b [128]   b_classifier.q.0.*  (b_classifier.q.* when nonlinear == 0)
 *   q2_w  [128,128] q2_b [128] b_classifier.q.2.*  (ignored when nonlinear == 0)
 *   fcc_w [C,C,Kv] fcc_b [C]   b_classifier.fcc.*  (Conv1d(C,C,kernel_size=Kv))
 */
typedef struct dsmil_agg_params {
    const float* fc_w;
    const float* fc_b;
    const float* q0_w;
    const float* q0_b;
    const float* q2_w;
    const float* q2_b;
    const float* fcc_w;
    const float* fcc_b;
    int32_t K;         /* feature width of feats (512; 166 MUSK1; 1024 tree)           */
    int32_t Kv;        /* width of the value rows (== K unless passing_v)               */
    int32_t C;         /* number of classes                                             */
    int32_t nonlinear; /* dsmil.py:30-33: 1 = Linear-ReLU-Linear-Tanh query, 0 = Linear  */
} dsmil_agg_params;

/* Supported number of classes C per entry point (dsmil.py:43: the aggregator handles any number of classes):
 *   forward (dsmil_agg_forward / _ex / _bf16, the instance-sharded calls), dsmil_agg_backward / _ex, dsmil_fc_forward:
 *       any C >= 1 (C <= 2 takes dedicated kernels; a larger C walks the classes in pairs)
 *   dsmil_agg_loss_head, dsmil_agg_train_step: 1 <= C <= 64 (one wave of classes); C > 64 -> DSMIL_E_UNSUPPORTED, and
 *       MILNet.bag_loss / training.FusedTrainStep compose the objective from the calls above instead
 * tests/test_agg_classes_gpu.py checks every route at C > 2 against the fp64 oracle. */

/* Replaces MILNet.forward / FCLayer.forward + BClassifier.forward (dsmil.py:10-12,46-62,70-74)
 * for a BATCH of n_bags independent bags stored back to back ("varlen"):
 *   feats    device [total_rows, K] fp32 row-major; bag b owns rows offsets[b]..offsets[b+1]-1
 *   vals     device [total_rows, Kv] fp32 — V of dsmil.py:48; pass feats (or NULL) when
 *            v = Identity (passing_v=False, the only form any reference script uses)
 *   offsets  device int64 [n_bags+1], offsets[0] == 0, non-decreasing, every bag >= 1 row
 *   max_rows the largest bag length (host value; sizes the launch grid)
 *   classes_in  device [total_rows, C] or NULL.  NULL: instance logits are computed here
 *            (FCLayer) and written to classes_out.  Non-NULL: BClassifier.forward(feats, c)
 *            with caller-supplied c (attention_map.py:85); classes_out may then be NULL.
 * Outputs (device, fp32 unless noted):
 *   classes_out [total_rows, C]   instance logits           (dsmil.py:11)
 *   A           [total_rows, C]   attention, softmax over each bag's instances (dsmil.py:56)
 *   B           [n_bags, C, Kv]   bag embeddings            (dsmil.py:57-59)
 *   pred        [n_bags, C]       bag logits                (dsmil.py:60-61)
 *   idx         int64 [n_bags, C] critical-instance index, bag-local (dsmil.py:52, row 0 of
 *                                 the descending sort; lowest index wins on exact ties)
 *   ws / ws_bytes  scratch of at least dsmil_agg_workspace_bytes(...) bytes, 256-B aligned
 */
int dsmil_agg_forward(const float* feats, const float* vals, const int64_t* offsets,
                      int32_t n_bags, int64_t total_rows, int64_t max_rows,
                      const dsmil_agg_params* p, const float* classes_in, float* classes_out,
                      float* A, float* B, float* pred, int64_t* idx, void* ws, size_t ws_bytes,
                      void* stream);

size_t dsmil_agg_workspace_bytes(int32_t n_bags, int64_t total_rows, int32_t K, int32_t Kv,
                                 int32_t C);

/* bf16-storage variant (BASELINE.json configs[2]: "2-class DSMIL aggregator bf16"; the reference
 * itself is fp32 only).  feats/vals are bfloat16 [total_rows,K] / [total_rows,Kv]; the query MLP
 * runs on bf16 MFMA with f32 accumulation from `packed` (dsmil_agg_pack_bf16: q0_w/q2_w rounded
 * to bf16, RNE); instance logits, scores, softmax, value sum and the bag head accumulate in f32
 * from the fp32 pointers in *p (the caller passes bf16-rounded values there if it wants the
 * "everything rounded to bf16" semantics of module.bfloat16()).  Outputs are fp32.
 * Requires K % 8 == 0 and Kv % 4 == 0 (else DSMIL_E_UNSUPPORTED). */
size_t dsmil_agg_packed_bf16_bytes(int32_t K);
int dsmil_agg_pack_bf16(const float* q0_w, const float* q2_w, int32_t K, void* packed, void* stream);
int dsmil_agg_forward_bf16(const void* feats_bf16, const void* vals_bf16, const int64_t* offsets,
                           int32_t n_bags, int64_t total_rows, int64_t max_rows,
                           const dsmil_agg_params* p, const void* packed, const float* classes_in,
                           float* classes_out, float* A, float* B, float* pred, int64_t* idx, void* ws,
                           size_t ws_bytes, void* stream);

/* ---- one bag sharded by INSTANCES over several GPUs ----------------------
 * Each rank holds a contiguous row range of ONE bag and exchanges C*(2+K) floats twice instead of
 * all-gathering the feature rows.  Per rank:
 *   1. dsmil_agg_shard_argmax: classes_out[rows,C] = FCLayer(feats) (dsmil.py:11) and, per class, the
 *      shard's best (value, shard-local index) of dsmil.py:52 (lowest index on ties).
 *      -> exchange (value, global index, the feature row feats[best_idx]) and keep, per class, the
 *         bag-wide winner's row: crit_rows[C,K].
 *   2. dsmil_agg_shard_attend: q_max = q(crit_rows) (dsmil.py:53-54), then the fused query/score/
 *      value-sum kernel over this shard: A_unnorm[rows,C] = exp(s - m_shard), ml[C,2] = (m_shard,
 *      sum_n exp(s - m_shard)), B_unnorm[C,Kv] = sum_n exp(s - m_shard) V[n].
 *      -> merge over ranks: m = max m_r, w_r = exp(m_r - m), l = sum l_r w_r, B = sum B_r w_r / l,
 *         A = A_unnorm w_r / l on each rank, pred = Conv1d head on B (dsmil.py:57-61).
 * Workspace: dsmil_agg_workspace_bytes(1, rows, K, Kv, C).  fp32 only. */
int dsmil_agg_shard_argmax(const float* feats, int64_t rows, const dsmil_agg_params* p,
                           float* classes_out, float* best_val, int64_t* best_idx, void* ws,
                           size_t ws_bytes, void* stream);
int dsmil_agg_shard_attend(const float* feats, const float* vals, int64_t rows,
                           const dsmil_agg_params* p, const float* crit_rows, float* A_unnorm,
                           float* ml, float* B_unnorm, void* ws, size_t ws_bytes, void* stream);

/* Which MFMA form dsmil_agg_forward uses for the fp32 query MLP (dsmil.py:31-33,49):
 *   6 (default) — bf16 MFMA over exact three-plane cuts of both fp32 operands (csrc/agg_split.h), the six
 *                 largest of the nine plane products; the three left out are together < 2^-20 of |x*w|,
 *                 below the rounding an fp32 dot product of this length carries anyway
 *   9           — all nine plane products: every fp32 product formed exactly (env DSMIL_MLP=s9)
 *   0           — v_mfma_f32_32x32x2_f32 (env DSMIL_MLP=f32)
 * The product library always uses 6; experiment builds (libdsmil_hip_expt.so) read the environment variable DSMIL_MLP
 * once per process. */
int dsmil_agg_mlp_form(void);

/* Where the critical instance's query q_max (dsmil.py:53-54) is computed on the few-rows fp32 path (a lone bag, a training
 * step: kernel k_attend_hs): mode 1 (default) = by the first C workgroups of the attend launch itself, handed to the
 * tiles through an agent-scope release/acquire flag (only when the whole launch is resident at once; larger batches take
 * the separate launch anyway); mode 0 = always the separate k_qmax launch between the logits pass and the attend kernel.
 * Both produce the same bits; the switch exists so that a test can compare them (tests/test_agg_gpu.py, hand-off stress).
 * Process-wide.  Returns the previous mode; any other `mode` only queries. */
int dsmil_agg_inline_query(int mode);

/* Which kernel a BATCH of fp32 bags (>= 512 tiles of 128 rows; v = Identity; K a multiple of 128 up to 512) takes for
 * dsmil.py:49-57.  All modes are the same fp32-class arithmetic (tests/test_agg_gpu.py compares them):
 *   2 (default)  k_attend_f3 (csrc/agg_f3.h) for the two-layer query with C <= 2: the query weights stay in registers for
 *                the whole launch, 32-row tiles resident in LDS from the query MLP to the value sum (every feature byte read
 *                once), fp16 MFMA over two-plane cuts of the row-scaled operands, three plane products, one partial per
 *                (workgroup, bag); every other case as mode 1;
 *   1            k_attend_f2 (csrc/agg_f2.h): the same arithmetic on 64-row tiles, weights streamed from L2 per tile;
 *   0            k_query_attend_split of rounds 2-4 (bf16 MFMA, exact three-plane cuts, six products, the tile read twice).
 * Process-wide; returns the previous mode; any other `mode` only queries. */
int dsmil_agg_batch_form(int mode);

/* (ABI 5) Workgroups of the persistent batch kernels (k_attend_f3 / k_attend_f2 / k_attend_bf16_res).  The default is the
 * CONSTANT 256 (the CUs of an unpartitioned MI355X), not the visible CU count: the run of tiles a workgroup owns fixes which
 * tiles share a partial and with it the fp32 summation order, so the outputs are bit-identical on every box (partition
 * mode, masked CUs) — tests/test_agg_gpu.py checks two other grids against the fp64 oracle.  n in 1..1024 sets it
 * (process-wide) and returns the previous value; any other n only queries. */
int dsmil_agg_persistent_grid(int n);

/* (ABI 5, round 6) The kernels around the persistent attend kernel of a bf16 BATCH (K = 512, C <= 2; dsmil.py:50-54 — the
 * instance logits, the critical instance and its query — and the combine of dsmil.py:57-61).  The co-resident forms
 * (k_logits_pipe, a 4-wave k_qmax, the lean k_finish) hold <= 80 registers per lane and a few KiB of LDS, so one wave of them
 * fits on every SIMD beside the resident k_attend_bf16_res workgroup of ANOTHER stream's batch (432 of a SIMD's 512
 * registers): with two or more streams in flight the second read of the features runs under the MFMA kernel of the batch in
 * front instead of behind it (+12-17 % bags/s); alone on the chip they are ~6 % slower than the plain forms.
 *   1 (default)  co-resident forms when the last few batch calls arrived on more than one stream, else the plain forms;
 *   2            always the co-resident forms;      0   never (k_logits_stream, 16-wave k_qmax, k_finish).
 * Outputs are bit-identical in every mode (tests/test_agg_bf16_gpu.py).  Process-wide; returns the previous mode; any other
 * `mode` only queries. */
int dsmil_agg_logits_form(int mode);

/* Compute units of the current device as the library sees them (256 on MI355X); <= 0 without a device.  Diagnostic: recorded
 * by bench.py and the soak so that a result can be tied to the box it ran on. */
int dsmil_device_cus(void);

/* Options of dsmil_agg_forward_ex (all optional; a NULL opts or an all-zero struct = dsmil_agg_forward):
 *   packed_split  the plane-cut query weights of forms 6 / 9 prepared ONCE per weight set instead of on every
 *                 forward (BClassifier.q changes only at optimizer.step(), train_tcga.py:73): dsmil_agg_pack_split
 *                 cuts q0_w [128,K] and q2_w [128,128] (NULL when nonlinear == 0) into a buffer of
 *                 dsmil_agg_packed_split_bytes(K, nonlinear) bytes, 16-B aligned.  Ignored by form 0.
 *   row_map       int64 [total_rows]: logical row i of the batch (bag b, instance i - offsets[b]) lives at physical
 *                 row row_map[i] of feats / vals.  This is train_tcga.py:78-83 `dropout_patches` (a random subset /
 *                 permutation of a bag's rows, `feats[random_indices]`) as an index list folded into the kernels' row
 *                 loads instead of a gathered 20 MB copy.  classes_out / A / idx stay in LOGICAL order (= the order of
 *                 the reference's gathered tensor).
 *   packed_f2     (ABI 4) the same query weights in the form BATCHES of fp32 bags use since round 5 (kernel k_attend_f2:
 *                 two fp16 planes of the power-of-two scaled weights, csrc/agg_f2.h), prepared once per weight set by
 *                 dsmil_agg_pack_f2 into dsmil_agg_packed_f2_bytes(K) bytes, 16-B aligned; NULL = cut inside the forward. */
typedef struct dsmil_agg_opts {
    const void* packed_split;
    const int64_t* row_map;
    const void* packed_f2;
} dsmil_agg_opts;
size_t dsmil_agg_packed_split_bytes(int32_t K, int32_t nonlinear);
int dsmil_agg_pack_split(const float* q0_w, const float* q2_w, int32_t K, void* packed, void* stream);
size_t dsmil_agg_packed_f2_bytes(int32_t K);
int dsmil_agg_pack_f2(const float* q0_w, const float* q2_w, int32_t K, void* packed, void* stream);
int dsmil_agg_forward_ex(const float* feats, const float* vals, const int64_t* offsets,
                         int32_t n_bags, int64_t total_rows, int64_t max_rows,
                         const dsmil_agg_params* p, const dsmil_agg_opts* opts, const float* classes_in,
                         float* classes_out, float* A, float* B, float* pred, int64_t* idx, void* ws,
                         size_t ws_bytes, void* stream);

/* The training objective of ONE bag, train_tcga.py:67-71 (also train_mil.py):
 *   max_prediction = max_n ins_prediction[n,:]  (= classes[idx_c, c], idx = the forward's critical instances)
 *   loss = 0.5 BCEWithLogitsLoss(bag_prediction, y) + 0.5 BCEWithLogitsLoss(max_prediction, y)   (mean over C)
 * and its gradients with respect to the two logit vectors, in one launch (the reference spends ~10 small kernels
 * and their autograd nodes on it):  loss[1], max_pred[C], g_pred[C] = dloss/dpred, g_max[C] = dloss/dmax_pred
 * (each may be NULL except loss).  `classes` / `pred` / `idx` are the forward's outputs for this bag, `label` [C]
 * fp32 0/1.  C <= 64. */
int dsmil_agg_loss_head(const float* classes, const float* pred, const int64_t* idx, const float* label,
                        int32_t C, float* loss, float* max_pred, float* g_pred, float* g_max, void* stream);

/* Class weights of the objective: the criterion train_mil.py:172-173 builds, BCEWithLogitsLoss(pos_weight), and torch's
 * general BCEWithLogitsLoss(weight, pos_weight), as train_mil.py:52-55 applies it to the bag and the max-instance logits.
 * Per logit z of class c with label y (torch's binary_cross_entropy_with_logits):
 *     lw = 1 + (pos_weight[c] - 1) y
 *     term = weight[c] ((1 - y) z + lw (max(-z, 0) + log1p(exp(-|z|))))
 *     d term / dz = weight[c] ((1 - y) - lw sigma(-z))  =  weight[c] (((pos_weight[c] y + 1) - y) sigma(z) - pos_weight[c] y),
 *     evaluated in the second form, torch's backward (sigma formed from exp(-|z|): nothing overflows for large |z|)
 * in place of max(z,0) - z y + log1p(exp(-|z|)) and sigma(z) - y; the 0.5, the mean over the C classes and a batch's mean
 * over its bags are unchanged.  Both members are DEVICE pointers, [C] fp32, and either may be NULL (= all ones).
 * The four *_w entries below have the signature of their unweighted sibling plus `const dsmil_bce_weights*` in front of
 * `stream`, and the sibling's contract otherwise: same launches, same workspace (the sibling's size query answers for
 * both), same limits (C <= 64), same order of checks and error codes, all before any launch, so a refused call has changed
 * nothing.  A NULL struct, or both members NULL, gives the sibling's bits (the sibling IS that call); all-ones vectors agree
 * with it to rounding.  A weight pointer that is not 4-byte aligned -> DSMIL_E_ALIGN (with the sibling's other alignment
 * checks; the loss heads have no other: behind their DSMIL_E_INVALID / DSMIL_E_UNSUPPORTED checks).
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): detected by SYMBOL. */
typedef struct dsmil_bce_weights {
    const float* pos_weight;   /* [C] or NULL */
    const float* weight;       /* [C] or NULL */
} dsmil_bce_weights;
/* dsmil_agg_loss_head with class weights (train_mil.py:172-173, :52-55). */
int dsmil_agg_loss_head_w(const float* classes, const float* pred, const int64_t* idx, const float* label, int32_t C,
                          float* loss, float* max_pred, float* g_pred, float* g_max, const dsmil_bce_weights* bw,
                          void* stream);

/* FCLayer.forward alone (dsmil.py:10-12): classes[total_rows, C] = feats @ fc_w^T + fc_b. */
int dsmil_fc_forward(const float* feats, int64_t total_rows, int32_t K, int32_t C,
                     const float* fc_w, const float* fc_b, float* classes, void* stream);

/* ---- aggregator backward (training step) -----------------------------------------------------
 * Replaces what autograd derives for `loss.backward()` in train_tcga.py:67-72 / train_mil.py for
 * ONE bag through MILNet.forward (dsmil.py:70-74): gradients of every parameter of FCLayer
 * (dsmil.py:6-12) and BClassifier (dsmil.py:27-62) given the upstream gradients of the forward's
 * outputs.  Device pointers, fp32, each gradient has its parameter's shape and is OVERWRITTEN
 * (the caller accumulates into .grad if it needs to).  g_classes / g_A / g_B may be NULL (treated
 * as zero; with g_classes NULL the fc_* gradients are not written).  The arg-max indices are
 * constants of the graph, as in torch.sort + index_select (dsmil.py:51-53).  `A`, `B`, `idx` are
 * the forward's outputs for this bag.  With passing_v (BClassifier.v = Dropout+Linear+ReLU,
 * dsmil.py:39-44) the caller hands the value rows in `vals` and asks for their gradient in
 * `g_vals` [N, Kv] (= A gB^T, NULL to skip), which it pushes through its own v layer. */
typedef struct dsmil_agg_grads {
    float* fc_w;   /* [C, K]      */
    float* fc_b;   /* [C]         */
    float* q0_w;   /* [128, K]    */
    float* q0_b;   /* [128]       */
    float* q2_w;   /* [128, 128]  (unused when !nonlinear) */
    float* q2_b;   /* [128]       */
    float* fcc_w;  /* [C, C, Kv]  */
    float* fcc_b;  /* [C]         */
} dsmil_agg_grads;

/* The size fits either form of the query (p->nonlinear is not an argument): the larger of the two layouts, which from a few
 * thousand rows on is the LINEAR query's (more row ranges of partials).  The same holds for the _rows and _bags queries. */
size_t dsmil_agg_backward_workspace_bytes(int64_t N, int32_t K, int32_t Kv, int32_t C);
/* dsmil_agg_backward_ex adds: g_max [C] — the SPARSE instance-stream gradient of the training objective (the max
 * over instances touches one row per class: g_fc_w[c] += g_max[c] * feats[idx_c], g_fc_b[c] += g_max[c]; may be
 * combined with a dense g_classes or replace it) and row_map (see dsmil_agg_opts; N logical rows).  A, g_A, g_vals,
 * g_classes are in logical row order. */
int dsmil_agg_backward_ex(const float* feats, const float* vals, int64_t N, const dsmil_agg_params* p,
                          const float* A, const float* B, const int64_t* idx, const float* g_classes,
                          const float* g_max, const float* g_pred, const float* g_A, const float* g_B,
                          const dsmil_agg_grads* g, float* g_vals, const int64_t* row_map, void* ws,
                          size_t ws_bytes, void* stream);
int dsmil_agg_backward(const float* feats, const float* vals, int64_t N, const dsmil_agg_params* p,
                       const float* A, const float* B, const int64_t* idx, const float* g_classes,
                       const float* g_pred, const float* g_A, const float* g_B,
                       const dsmil_agg_grads* g, float* g_vals, void* ws, size_t ws_bytes,
                       void* stream);
/* dsmil_agg_backward_rows: everything dsmil_agg_backward_ex does, plus the gradient of the INPUT rows — what autograd
 * leaves in `x.grad` for `x.requires_grad_(); loss.backward()` through MILNet.forward (dsmil.py:70-74), i.e. through the
 * query stream (dsmil.py:49,53-55), FCLayer (dsmil.py:10-12) and, for v = Identity, `B = A^T V` (dsmil.py:57):
 *     g_feats [N, K] = gH q0_w  (+ g_classes fc_w)  (+ g_max[c] fc_w[c] at row idx_c)  (+ A gB  when vals is feats / NULL)
 * OVERWRITTEN, fp32, in LOGICAL row order when row_map is given (the convention of A and g_vals; the caller scatters it
 * if it wants physical rows).  With caller-supplied value rows (passing_v) the value stream's share is NOT included: it
 * reaches the rows through the caller's v layer — dsmil_value_backward_rows adds it.  p->fc_w must be given when g_classes
 * or g_max is.  g_feats == NULL behaves exactly as dsmil_agg_backward_ex (same launches, same bits); with g_feats one
 * more launch (k_bwd_gx, csrc/agg_gx.h), deterministic.  The workspace is the backward's
 * (dsmil_agg_backward_rows_workspace_bytes == dsmil_agg_backward_workspace_bytes today).
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): a caller detects this entry
 * and dsmil_value_backward_rows by SYMBOL (dlsym / hasattr on the loaded library). */
size_t dsmil_agg_backward_rows_workspace_bytes(int64_t N, int32_t K, int32_t Kv, int32_t C);
int dsmil_agg_backward_rows(const float* feats, const float* vals, int64_t N, const dsmil_agg_params* p,
                            const float* A, const float* B, const int64_t* idx, const float* g_classes,
                            const float* g_max, const float* g_pred, const float* g_A, const float* g_B,
                            const dsmil_agg_grads* g, float* g_vals, const int64_t* row_map, void* ws,
                            size_t ws_bytes, void* stream, float* g_feats);

/* ---- aggregator backward over a BATCH of bags (minibatch training) -------------------------------------------------
 * Replaces what autograd derives for `loss.backward()` in train_tcga.py:60-73 applied to SEVERAL bags whose losses are
 * summed before one optimizer.step() (the reference steps once per bag, train_tcga.py:73; a batch is this project's
 * addition): bag b owns rows offsets[b]..offsets[b+1]-1 of the batch, exactly as in dsmil_agg_forward_ex, and
 * `A`, `B`, `idx` are that call's outputs for the same batch.
 *   g_pred [n_bags, C], g_max [n_bags, C] or NULL (sparse: touches row offsets[b] + idx[b,c]), g_classes [total_rows, C],
 *   g_A [total_rows, C], g_B [n_bags, C, Kv] (each NULL = zero): the upstream gradients
 *   g       every parameter gradient = the SUM over the bags of what dsmil_agg_backward_rows gives for bag b alone (the
 *           arg-max indices are constants), OVERWRITTEN; the NULL rules of dsmil_agg_backward_rows
 *   g_vals [total_rows, Kv], g_feats [total_rows, K] (each NULL to skip): the per-bag results laid end to end
 *   row_map int64 [total_rows] or NULL, as in dsmil_agg_opts; the per-row inputs and outputs are in LOGICAL order
 *   max_rows  the largest bag length (host value, 1 <= max_rows <= total_rows; the launch grids are sized by the real
 *           tiles of the batch, not by it)
 * Checks run in the order of dsmil_agg_backward_rows — DSMIL_E_INVALID (NULL offsets, n_bags < 1, total_rows < n_bags
 * included), then DSMIL_E_ALIGN, then DSMIL_E_WORKSPACE — all before any launch; total_rows > 2^30 -> DSMIL_E_UNSUPPORTED
 * (behind the INVALID checks).  Every bag has at least one row.  The call allocates nothing, never synchronises, uses no
 * atomics and sums in a fixed order (bags in order, then k_tn_split's row ranges in order): two runs give the same bits,
 * and a batch of one bag gives the bits of dsmil_agg_backward_rows.  Any C >= 1, any K (K % 4 != 0 takes the
 * register-staged tile).  csrc/agg_bwd_bags.h.
 * dsmil_agg_loss_head_bags: the objective of dsmil_agg_loss_head (train_tcga.py:67-71) for every bag of the batch in one
 * launch: labels [n_bags, C] -> loss [n_bags], max_pred / g_pred / g_max [n_bags, C] (each may be NULL except loss); the
 * gradients are those of each bag's OWN loss (the caller scales them, e.g. by 1 / n_bags for a mean).  C <= 64.
 * Added without a change of DSMIL_ABI_VERSION (it stays 6): detected by SYMBOL, like dsmil_agg_backward_rows. */
size_t dsmil_agg_backward_bags_workspace_bytes(int32_t n_bags, int64_t total_rows, int32_t K, int32_t Kv, int32_t C);
int dsmil_agg_backward_bags(const float* feats, const float* vals, const int64_t* offsets, int32_t n_bags,
                            int64_t total_rows, int64_t max_rows, const dsmil_agg_params* p, const float* A,
                            const float* B, const int64_t* idx, const float* g_classes, const float* g_max,
                            const float* g_pred, const float* g_A, const float* g_B, const dsmil_agg_grads* g,
                            float* g_vals, const int64_t* row_map, void* ws, size_t ws_bytes, void* stream,
                            float* g_feats);
int dsmil_agg_loss_head_bags(const float* classes, const int64_t* offsets, const float* pred, const int64_t* idx,
                             const float* labels, int32_t n_bags, int32_t C, float* loss, float* max_pred,
                             float* g_pred, float* g_max, void* stream);
/* dsmil_agg_loss_head_bags with class weights (train_mil.py:172-173, :52-55; see dsmil_bce_weights): the same [C] vectors
 * for every bag of the batch. */
int dsmil_agg_loss_head_bags_w(const float* classes, const int64_t* offsets, const float* pred, const int64_t* idx,
                               const float* labels, int32_t n_bags, int32_t C, float* loss, float* max_pred,
                               float* g_pred, float* g_max, const dsmil_bce_weights* bw, void* stream);

/* ---- where the fp32 aggregator backward leaves its intermediates — FOR TESTS (tests/test_agg_bwd_precision_gpu.py; no reference
 * counterpart).  dsmil_agg_backward_layout answers, on the host alone (no launch, no device memory touched), what
 * dsmil_agg_backward* (n_bags == 0: the one-bag layout) or dsmil_agg_backward_bags (n_bags >= 1) will do with a workspace for
 * N rows in all: the byte offset of every intermediate from the workspace's start (each region is written once per call and
 * never overwritten, so a test can read the inputs and outputs of every launch back after the call), the row ranges of the
 * contraction over the instances and the row tile of step 4.  The offsets are the launch sequences' own (bwd_layout is called).
 *   gB [sets, C, Kv], Dv [sets, C], qmax / gq [sets, C, 128] (sets = max(n_bags, 1)); gA, gs [N, C]; gz2, Hb, Qb, gH [N, 128];
 *   gqp [T32 (one bag) or N / 32 + n_bags + 1 tile slots (bag b's first: offsets[b] / 32 + b), C, 128];
 *   part0 [S, 128, K], part1 [S, 128, 128], pb0 / pb1 [S, 128]: row range s = rows s R .. min((s + 1) R, N) - 1;
 *   part [splits, C, K], part_b [splits, C]: k_tn_small's (dense g_classes only): row range s = rows s small_rows .. of N
 *   total: the bytes the call needs for this `nonlinear` (the *_workspace_bytes queries answer the nonlinear size)
 *   tile: DSMIL_BWD_TILE_* from N, K and rows_aligned16 (the rows' base address % 16 == 0), as the entry chooses it;
 *   qrow_vec: 4 when the critical-query kernel loads 16 bytes (K % 4 == 0 and rows_aligned16 and q0w_aligned16), else 1.
 * Returns DSMIL_E_INVALID for a NULL `out`, n_bags < 0 or a size <= 0 (N < n_bags included).
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): a caller finds it by symbol. */
#define DSMIL_BWD_TILE_HS 0        /* hidden-split 64-row tile (k_bwd_rows_hs, k_bwd_gh_hs) */
#define DSMIL_BWD_TILE_W1_REG 1    /* one-wave 32-row tile, register-staged (k_bwd_rows<1,1>) */
#define DSMIL_BWD_TILE_W4_DMA 2    /* four-wave 128-row tile, LDS-DMA staged (k_bwd_rows<4,4>, k_bwd_gh<4>) */
#define DSMIL_BWD_TILE_W4_REG 3    /* four-wave 128-row tile, register-staged (k_bwd_rows<4,1>; one bag only) */
typedef struct dsmil_agg_bwd_layout {
    uint64_t gB, Dv, qmax, gq, gA, gs, gz2, Hb, Qb, gH, gqp, part0, part1, pb0, pb1, part, part_b;   /* byte offsets */
    uint64_t total;
    int64_t T32;                   /* 32-row tiles of N rows */
    int32_t S, R, splits, small_rows, tile, qrow_vec;
} dsmil_agg_bwd_layout;
int dsmil_agg_backward_layout(int32_t n_bags, int64_t N, int32_t K, int32_t Kv, int32_t C, int32_t nonlinear,
                              int32_t rows_aligned16, int32_t q0w_aligned16, dsmil_agg_bwd_layout* out);

/* ---- the batched aggregator backward on bf16-STORED rows (training on a bf16 feature cache) -----------------------------
 * Replaces what autograd derives for `loss.backward()` in train_tcga.py:60-73 when the bag's rows are stored in bfloat16
 * (the rows dsmil_agg_forward_bf16 reads; the reference has no such storage: it would widen the bag first).  The contract of
 * dsmil_agg_backward_bags with two omissions — no row_map and no g_feats, like the bf16 forward; a lone bag is a batch of
 * one (offsets = {0, N}), so there is no one-bag entry:
 *   feats_bf16 [total_rows, K], vals_bf16 [total_rows, Kv] or NULL (= feats): raw bfloat16, rows 16-B aligned
 *   *p         fp32 parameters.  The gradient is the analytic gradient of dsmil.py:46-62 (+ the fused FCLayer) at x := the
 *              bf16 rows and W := *p, with the forward's own A, B, idx as inputs (csrc/agg_bwd.hip, header) — exact for
 *              whatever is handed in; to differentiate dsmil_agg_forward_bf16 hand in the bf16-ROUNDED weights it used
 *              (straight-through for its roundings).  A bf16 value is an exact bf16 MFMA operand (plane cut (x, 0, 0)):
 *              no arithmetic is lost against the fp32 call on a widened copy, and no such copy is ever written.
 *   g, g_vals  fp32, as in dsmil_agg_backward_bags
 * Requires K % 8 == 0 and Kv % 4 == 0 (dsmil_agg_forward_bf16's condition; else DSMIL_E_UNSUPPORTED).  Checks run in the
 * order DSMIL_E_INVALID, total_rows > 2^30 and the shape condition (DSMIL_E_UNSUPPORTED), DSMIL_E_ALIGN (rows, workspace,
 * biases), DSMIL_E_WORKSPACE — all before any launch.  Same launch sequence, same workspace layout and size as the fp32
 * call; the rows stay 2 bytes per element for the six kernels that read them (the register-staged and hidden-split tiles:
 * the LDS-DMA tile stages fp32 bytes).  No allocation, no sync, no atomics, fixed-order sums: two runs give the same bits.
 * Added without a change of DSMIL_ABI_VERSION (it stays 6): detected by SYMBOL. */
size_t dsmil_agg_backward_bags_bf16_workspace_bytes(int32_t n_bags, int64_t total_rows, int32_t K, int32_t Kv, int32_t C);
int dsmil_agg_backward_bags_bf16(const void* feats_bf16, const void* vals_bf16, const int64_t* offsets, int32_t n_bags,
                                 int64_t total_rows, int64_t max_rows, const dsmil_agg_params* p, const float* A,
                                 const float* B, const int64_t* idx, const float* g_classes, const float* g_max,
                                 const float* g_pred, const float* g_A, const float* g_B, const dsmil_agg_grads* g,
                                 float* g_vals, void* ws, size_t ws_bytes, void* stream);

/* ---- the value stream of BClassifier(passing_v=True) (ABI 6) ---------------------------------------------------------
 * Replaces `V = self.v(feats)` of dsmil.py:48 with self.v = Sequential(Dropout, Linear(K, K), ReLU) (dsmil.py:35-39; the
 * dropout is the caller's: it hands in the rows it wants projected):  V[n, j] = max(0, sum_k feats[n, k] v_w[j, k] + v_b[j]),
 * fp32 in, fp32 out, fp32-class arithmetic (fp16 MFMA over two-plane cuts of the row-scaled rows and the tensor-scaled
 * weights, three plane products, fp32 accumulation: csrc/agg_value.h).  The result is the `vals` of dsmil_agg_forward.
 *   v_w [Kv, K], v_b [Kv]   b_classifier.v.1.{weight,bias}  (Kv == K in the reference)
 *   dsmil_value_pack     replaces nothing in the reference (its nn.Linear reads the weights as they are): cuts v_w ONCE per
 *                        weight set into dsmil_value_packed_bytes(K, Kv) bytes (16-B aligned) of MFMA-fragment-ordered planes
 *   dsmil_value_forward  dsmil.py:48.  packed: that image, or NULL = cut v_w into `ws` first (then ws must hold
 *                        dsmil_value_workspace_bytes(rows, K, Kv) bytes, 256-B aligned; with an image, ws may be NULL).
 *                        row_map: int64 [rows] or NULL, logical row i is physical row row_map[i] of feats (see
 *                        dsmil_agg_opts); V_out [rows, Kv] is in logical order.  One launch (two with packed == NULL).  Any K:
 *                        K <= 1024 on the matrix cores, wider rows on a plain fp32 kernel.
 *   dsmil_value_backward what autograd derives for dsmil.py:39 behind g_vals (= dsmil_agg_backward's g_vals) for the layer's
 *                        PARAMETERS:  gZ = g_vals * (V > 0),  g_v_w [Kv, K] = gZ^T feats,  g_v_b [Kv] = column sums of gZ
 *                        (both OVERWRITTEN; gZ is never written to memory; bf16 MFMA over exact three-plane cuts, fixed-order
 *                        two-stage sums: two runs give the same bits).  V, g_vals [rows, Kv] in logical order.  The gradient of
 *                        the input rows (gZ v_w) is not computed here (dsmil_value_backward_rows does).  Two launches.
 *   dsmil_value_backward_rows  what autograd derives for dsmil.py:35-39,48 behind g_vals for the layer's INPUT rows:
 *                        g_feats [rows, K] = (g_vals * (V > 0)) v_w, or g_feats += that with accumulate != 0 (the
 *                        aggregator's own g_feats and this term then share one buffer, no separate add pass).  Logical row
 *                        order throughout.  gZ is never written to memory; bf16 MFMA over exact three-plane cuts, six plane
 *                        products, fixed order: two runs give the same bits.  One launch (k_value_gx: csrc/agg_gx.h's tile), any K
 *                        and Kv on the matrix cores.  feats and packed are not read by this product (v_w is cut as it is
 *                        staged: the forward's image is ordered along K, this contraction runs along Kv) and may be NULL;
 *                        it needs no workspace: ws may be NULL (ws_bytes 0); a non-NULL ws must be 256-B aligned.
 *                        Detected by symbol, see dsmil_agg_backward_rows. */
size_t dsmil_value_packed_bytes(int32_t K, int32_t Kv);
int dsmil_value_pack(const float* v_w, int32_t K, int32_t Kv, void* packed, void* stream);
size_t dsmil_value_workspace_bytes(int64_t rows, int32_t K, int32_t Kv);
int dsmil_value_forward(const float* feats, int64_t rows, int32_t K, int32_t Kv, const float* v_w, const float* v_b,
                        const void* packed, const int64_t* row_map, float* V_out, void* ws, size_t ws_bytes, void* stream);
int dsmil_value_backward(const float* feats, const float* V, const float* g_vals, int64_t rows, int32_t K, int32_t Kv,
                         const int64_t* row_map, float* g_v_w, float* g_v_b, void* ws, size_t ws_bytes, void* stream);
int dsmil_value_backward_rows(const float* feats, const float* V, const float* g_vals, int64_t rows, int32_t K, int32_t Kv,
                              const float* v_w, const void* packed, int32_t accumulate, float* g_feats, void* ws,
                              size_t ws_bytes, void* stream);

/* ---- the value stream on bf16-stored rows (ABI 6, additive: detected by SYMBOL like dsmil_agg_backward_rows) -----------------
 * Replaces `V = self.v(feats)` of dsmil.py:48 with self.v = Sequential(Dropout, Linear(K, K), ReLU) (dsmil.py:35-39) for the
 * bf16-storage aggregator (dsmil_agg_forward_bf16, whose `vals` operand the result is):
 *     V[n, j] = bf16(max(0, sum_k feats[n, k] w_b[j, k] + v_b[j])),   w_b = bf16(v_w),  round to nearest even both times,
 * bf16 rows in, bf16 rows out, fp32 accumulation: one bf16 MFMA product per MAC (csrc/agg_value.h, k_value_proj_b16).  Every
 * output's sum runs in an order that depends on K alone — not on the row's place in the call or the number of rows — so a
 * row's result has the same bits in any batch.  No row map.  Its parameter gradients on the same operands are
 * dsmil_value_backward_bf16 below (the input rows of the bf16 path take no gradient).
 *   v_w [Kv, K] fp32 (rounded inside), v_b [Kv] fp32, read as it is (the caller passes bf16-rounded values there if it wants
 *                        what module.bfloat16() holds, as with every bias of the bf16 path).  K % 8 == 0 and Kv % 4 == 0, else
 *                        DSMIL_E_UNSUPPORTED (dsmil_agg_forward_bf16's own condition on its operands).
 *   dsmil_value_pack_bf16     replaces nothing in the reference (dsmil.py:35-39's nn.Linear reads its weights as they are):
 *                        rounds v_w ONCE per weight set into dsmil_value_packed_bf16_bytes(K, Kv) bytes (16-B aligned) in
 *                        MFMA-fragment order, zero padded past K and Kv.
 *   dsmil_value_forward_bf16  dsmil.py:35-39,48.  feats_bf16 [rows, K] (16-B aligned), V_out_bf16 [rows, Kv].  packed: that
 *                        image, or NULL = round v_w into `ws` first (then ws must hold dsmil_value_workspace_bf16_bytes(rows,
 *                        K, Kv) bytes, 256-B aligned; with an image ws may be NULL).  One launch (two with packed == NULL).
 *                        K <= 1024 on the matrix cores, wider rows on a plain kernel (same arithmetic, k order; it reads v_w and
 *                        needs neither image nor workspace).  NULL operands: DSMIL_E_INVALID; a misaligned image, workspace or
 *                        row pointer: DSMIL_E_ALIGN; a short workspace: DSMIL_E_WORKSPACE — all before any launch.  Never
 *                        allocates or synchronises: capturable in a graph. */
size_t dsmil_value_packed_bf16_bytes(int32_t K, int32_t Kv);
int dsmil_value_pack_bf16(const float* v_w, int32_t K, int32_t Kv, void* packed, void* stream);
size_t dsmil_value_workspace_bf16_bytes(int64_t rows, int32_t K, int32_t Kv);
int dsmil_value_forward_bf16(const void* feats_bf16, int64_t rows, int32_t K, int32_t Kv, const float* v_w, const float* v_b,
                             const void* packed, void* V_out_bf16, void* ws, size_t ws_bytes, void* stream);

/* ---- the value layer's parameter gradients on bf16-stored rows (ABI 6, additive: detected by SYMBOL) ----------------------------
 * What autograd derives for dsmil.py:35-39 behind g_vals (= dsmil_agg_backward_bags_bf16's g_vals, fp32, unrounded) for the
 * layer's PARAMETERS, on the operands of the bf16 path as they are stored:
 *     gZ = V > 0 ? g_vals : 0   (a select on the bf16 V: +0, -0 and NaN mask; a NaN / inf in g_vals at a masked position gives 0),
 *     g_v_w [Kv, K] = gZ^T feats,   g_v_b [Kv] = column sums of gZ          (both fp32, OVERWRITTEN),
 * straight-through for the forward's roundings.  feats_bf16 [rows, K] and V_bf16 [rows, Kv] raw bfloat16 (dsmil_value_forward_bf16's
 * input and output), g_vals [rows, Kv] fp32.  A bf16 row is one exact bf16 MFMA operand: the three exact planes of gZ times the
 * one plane of feats, all three products kept, fp32 accumulation (csrc/agg_value.h, k_value_tn_b16); gZ and fp32 copies of feats
 * or V are never written to memory.  Fixed-order two-stage sums, no atomics: two runs give the same bits.  No row map.
 *   Checks, in this order, all before any launch:  DSMIL_E_INVALID (a NULL operand; rows, K or Kv not positive);
 *   DSMIL_E_UNSUPPORTED (K % 8 != 0 or Kv % 4 != 0 — dsmil_value_forward_bf16's condition — or a grid beyond 2^31 - 1
 *   workgroups);  DSMIL_E_ALIGN (feats_bf16 or g_vals not 16-B aligned, V_bf16 not 8-B aligned, ws not 256-B aligned);
 *   DSMIL_E_WORKSPACE (ws_bytes < dsmil_value_backward_bf16_workspace_bytes(rows, K, Kv); that is 0 for non-positive
 *   arguments).  Two launches (contraction, reduce).  Never allocates or synchronises: capturable in a graph. */
size_t dsmil_value_backward_bf16_workspace_bytes(int64_t rows, int32_t K, int32_t Kv);
int dsmil_value_backward_bf16(const void* feats_bf16, const void* V_bf16, const float* g_vals, int64_t rows, int32_t K, int32_t Kv,
                              float* g_v_w, float* g_v_b, void* ws, size_t ws_bytes, void* stream);

/* ---- one training step per C call (ABI 3) --------------------------------------------------------
 * Replaces the body of the reference's training loop for one bag, train_tcga.py:60-75 (train_mil.py:44-56 likewise):
 *     optimizer.zero_grad()
 *     ins_prediction, bag_prediction, _, _ = milnet(bag_feats)                     (:67)
 *     max_prediction, _ = torch.max(ins_prediction, 0)                             (:68)
 *     loss = 0.5 * BCEWithLogitsLoss(bag_prediction, y) + 0.5 * BCEWithLogitsLoss(max_prediction, y)   (:69-71)
 *     loss.backward(); optimizer.step()                                            (:72-73)
 * with optimizer = torch.optim.Adam(milnet.parameters(), lr, betas, weight_decay) (:241; amsgrad = maximize = False).
 * The forward, the loss head, the backward and ONE Adam kernel over the eight parameter tensors are enqueued on
 * `stream`; nothing synchronises.  The parameters in *p are UPDATED IN PLACE (they are the optimiser's tensors), as
 * are the moment tensors in *opt; `loss` (device, 1 float) receives the step's loss (the caller reads it for the
 * progress line of :74 — the step's only host sync).
 *   feats    device [rows, K] fp32, the bag;  row_map int64 [N] or NULL (dropout_patches, :78-83, as an index list)
 *   N        instances that enter the bag (= rows when row_map is NULL)
 *   label    device [C] fp32, the bag label (0/1)
 *   p        MILNet(FCLayer, BClassifier) parameters, v = Identity (Kv == K), C <= 64
 *   opt      Adam state: exp_avg / exp_avg_sq = 8 device pointers each in the order fc_w, fc_b, q0_w, q0_b, q2_w, q2_b,
 *            fcc_w, fcc_b (the q2 entries are ignored when !nonlinear); step = the 1-based index of THIS update
 *            (torch's state['step'] after its increment); hyper-parameters as Python floats (double)
 *   ws       dsmil_agg_train_step_workspace_bytes(N, K, C, nonlinear) bytes, 256-B aligned
 * dsmil_adam_step is the optimiser kernel alone (n_tensors <= DSMIL_ADAM_MAX_TENSORS; numel[i] == 0 skips entry i). */
#define DSMIL_ADAM_MAX_TENSORS 8
typedef struct dsmil_adam_state {
    float* const* exp_avg;
    float* const* exp_avg_sq;
    int64_t step;
    double lr, beta1, beta2, eps, weight_decay;
} dsmil_adam_state;
size_t dsmil_agg_train_step_workspace_bytes(int64_t N, int32_t K, int32_t C, int32_t nonlinear);
int dsmil_agg_train_step(const float* feats, int64_t N, const int64_t* row_map, const float* label,
                         const dsmil_agg_params* p, const dsmil_adam_state* opt, float* loss, void* ws,
                         size_t ws_bytes, void* stream);
int dsmil_adam_step(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const int64_t* numel, int64_t step, double lr, double beta1,
                    double beta2, double eps, double weight_decay, void* stream);

/* ---- one training step on a BATCH of bags per C call ------------------------------------------------
 * The body of train_tcga.py:60-75 applied to n_bags bags stored back to back (offsets / total_rows / max_rows as in
 * dsmil_agg_forward) with ONE optimiser step: the objective is the MEAN over the bags of
 *     0.5 * BCEWithLogitsLoss(bag_prediction, y) + 0.5 * BCEWithLogitsLoss(max instance prediction, y)      (:68-71)
 * and there is one Adam update per call (optimizer as for dsmil_agg_train_step).  The call enqueues, on `stream`: the
 * batched forward, one launch for the objective (each bag's loss, their mean, both logit gradients scaled by 1 / n_bags),
 * and the batched backward (dsmil_agg_backward_bags' launch sequence) whose last two launches apply Adam to the gradient
 * elements they have just summed.  Parameters (*p) and moments (*opt) are UPDATED IN PLACE.  Nothing allocates, nothing
 * synchronises; there are no atomics and every sum runs in a fixed order: two runs from the same state give the same bits,
 * and the gradients are bit for bit those of dsmil_agg_loss_head_bags + dsmil_agg_backward_bags on the same batch.
 *   feats      device [rows, K] fp32;  row_map int64 [total_rows] or NULL (every bag's dropout_patches list, offset added)
 *   labels     device [n_bags, C] fp32 (0/1)
 *   loss_each  device [n_bags]: each bag's own loss;   loss  device [1]: their mean (fp32 sum in bag order / n_bags)
 *   opt        as for dsmil_agg_train_step (step = the 1-based index of THIS update; step <= 0 -> DSMIL_E_INVALID)
 *   ws         dsmil_agg_train_step_bags_workspace_bytes(n_bags, total_rows, K, C, nonlinear) bytes, 256-B aligned: the
 *              batched forward's workspace, the batched backward's, the forward's outputs, the eight gradient tensors
 * dsmil_agg_train_step_bags_bf16: the same on bf16-STORED rows (no row map; a lone bag is a batch of one).  Two launches at
 * its head round the eight fp32 master tensors to bf16 (nearest even, kept as fp32) into the workspace and pack the MFMA
 * image of the rounded query weights (dsmil_agg_pack_bf16); forward (dsmil_agg_forward_bf16) and backward
 * (dsmil_agg_backward_bags_bf16) both read that rounded set (straight-through), Adam updates the fp32 masters.  Its
 * workspace adds the rounded set and the image.
 * Limits are those of the chained calls: C <= 64, v = Identity (Kv == K), n_bags <= 65535, total_rows <= 2^30; bf16 needs
 * K % 8 == 0.  Checks run in this order, ALL before the first launch, so a refused call has changed nothing:
 * DSMIL_E_INVALID (a NULL operand or moment, sizes, Kv != K, step <= 0), DSMIL_E_UNSUPPORTED (the limits above),
 * DSMIL_E_ALIGN (ws not 256-B aligned; labels / loss_each / loss not 4-B, offsets / row_map not 8-B aligned; fp32: q0_b or
 * q2_b not 16-B aligned; bf16: rows not 16-B aligned), DSMIL_E_WORKSPACE.  The *_workspace_bytes queries answer 0 for
 * sizes the entry refuses as invalid (and, bf16, for K % 8 != 0).
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): detected by SYMBOL. */
size_t dsmil_agg_train_step_bags_workspace_bytes(int32_t n_bags, int64_t total_rows, int32_t K, int32_t C, int32_t nonlinear);
int dsmil_agg_train_step_bags(const float* feats, const int64_t* offsets, int32_t n_bags, int64_t total_rows, int64_t max_rows,
                              const int64_t* row_map, const float* labels, const dsmil_agg_params* p,
                              const dsmil_adam_state* opt, float* loss_each, float* loss, void* ws, size_t ws_bytes,
                              void* stream);
size_t dsmil_agg_train_step_bags_bf16_workspace_bytes(int32_t n_bags, int64_t total_rows, int32_t K, int32_t C,
                                                      int32_t nonlinear);
int dsmil_agg_train_step_bags_bf16(const void* feats_bf16, const int64_t* offsets, int32_t n_bags, int64_t total_rows,
                                   int64_t max_rows, const float* labels, const dsmil_agg_params* p,
                                   const dsmil_adam_state* opt, float* loss_each, float* loss, void* ws, size_t ws_bytes,
                                   void* stream);
/* dsmil_agg_train_step_bags / _bf16 with class weights in the objective (train_mil.py:172-173, :52-55; see
 * dsmil_bce_weights): the body of train_mil.py:42-59 for a batch of one — the same launch sequence, the weights enter the
 * one launch of the objective.  ws: the sibling's size query.  The weight pointers are checked with the other 4-byte
 * operands (DSMIL_E_ALIGN, behind DSMIL_E_INVALID and DSMIL_E_UNSUPPORTED). */
int dsmil_agg_train_step_bags_w(const float* feats, const int64_t* offsets, int32_t n_bags, int64_t total_rows,
                                int64_t max_rows, const int64_t* row_map, const float* labels, const dsmil_agg_params* p,
                                const dsmil_adam_state* opt, float* loss_each, float* loss, void* ws, size_t ws_bytes,
                                const dsmil_bce_weights* bw, void* stream);
int dsmil_agg_train_step_bags_bf16_w(const void* feats_bf16, const int64_t* offsets, int32_t n_bags, int64_t total_rows,
                                     int64_t max_rows, const float* labels, const dsmil_agg_params* p,
                                     const dsmil_adam_state* opt, float* loss_each, float* loss, void* ws, size_t ws_bytes,
                                     const dsmil_bce_weights* bw, void* stream);

/* ---- patch embedder: ResNet-18 with InstanceNorm2d, fc = Identity --------------------------
 * Replaces the torchvision backbone that compute_feats.py:157,170 builds and dsmil.IClassifier
 * wraps (dsmil.py:21-25): feats[B,512] = flatten(avgpool(resnet18_IN(x))), and, when `classes`
 * is non-NULL, classes[B,C] = feats @ fc_w^T + fc_b (IClassifier.fc, dsmil.py:24).
 *   x_nchw   device [B,3,H,W] fp32 in [0,1] (what VF.to_tensor yields, compute_feats.py:35-39)
 *   conv1_w  device [64,3,7,7] fp32 — feature_extractor.conv1.weight, used as is
 *   packed   device buffer of dsmil_resnet18_packed_bytes() bytes filled by dsmil_resnet18_pack()
 *            from the other 19 conv weights
 *   ws       scratch of dsmil_resnet18_workspace_bytes(B,H,W) bytes, 256-B aligned
 * conv_w[20]: device pointers to the 20 bias-free conv weights [Cout,Cin,k,k] fp32 in torchvision
 * state_dict order (conv1; layerL.0.conv1, layerL.0.conv2, [layerL.0.downsample.0], layerL.1.conv1,
 * layerL.1.conv2 for L = 1..4) — the order compute_feats.py:226-231 relies on.  conv_w[0] is not
 * read by the packer. */
size_t dsmil_resnet18_packed_bytes(void);
int dsmil_resnet18_pack(const float* const* conv_w, float* packed, void* stream);
size_t dsmil_resnet18_workspace_bytes(int32_t B, int32_t H, int32_t W);
int dsmil_resnet18in_forward(const float* x_nchw, int32_t B, int32_t H, int32_t W,
                             const float* conv1_w, const float* packed, const float* fc_w,
                             const float* fc_b, int32_t C, float* feats, float* classes, void* ws,
                             size_t ws_bytes, void* stream);

/* The same forward fed with DECODED images: x_nhwc is uint8 [B,H,W,3] (row-major, RGB interleaved, as
 * PIL / numpy hold a patch).  The ToTensor step of the reference's loader (compute_feats.py:35-39:
 * VF.to_tensor = HWC uint8 -> CHW float32 / 255, IEEE division) is fused into the stem's input
 * staging, so results are bit-identical to dsmil_resnet18in_forward on the converted tensor while
 * the host->device copy and the first HBM read shrink 4x. */
int dsmil_resnet18in_forward_u8(const uint8_t* x_nhwc, int32_t B, int32_t H, int32_t W,
                                const float* conv1_w, const float* packed, const float* fc_w,
                                const float* fc_b, int32_t C, float* feats, float* classes, void* ws,
                                size_t ws_bytes, void* stream);

/* The same trunk with FROZEN-statistics norms — eval-mode nn.BatchNorm2d, i.e. the reference's
 * `--norm_layer batch` / ImageNet-pretrained extractor (compute_feats.py:149-154, run under
 * i_classifier.eval()).  Each of the 20 norms is y = (x - m[c]) * r[c] with
 *   r = weight / sqrt(running_var + eps),  m = running_mean - bias / r        (r != 0)
 * folded by the caller; bn_mean / bn_rstd are the 20 per-channel arrays concatenated in conv order
 * (dsmil_resnet18_norm_channels() = 4800 floats each).  All conv / pool / residual kernels are the
 * InstanceNorm ones; only the statistics step is replaced.  x is fp32 NCHW, or uint8 NHWC when
 * x_is_u8_nhwc != 0 (see dsmil_resnet18in_forward_u8). */
int32_t dsmil_resnet18_norm_channels(void);
int dsmil_resnet18bn_forward(const void* x, int32_t x_is_u8_nhwc, int32_t B, int32_t H, int32_t W,
                             const float* conv1_w, const float* packed, const float* bn_mean,
                             const float* bn_rstd, const float* fc_w, const float* fc_b, int32_t C,
                             float* feats, float* classes, void* ws, size_t ws_bytes, void* stream);

/* Generic trunk: BasicBlock depth 18 (blocks [2,2,2,2], 20 convs) or 34 ([3,4,6,3], 36 convs), Bottleneck depth 50
 * ([3,4,6,3], 53 convs) or 101 ([3,4,23,3], 104 convs; stride on the 3x3 conv, torchvision's v1.5) — the
 * reference's `--backbone resnet18|resnet34|resnet50|resnet101` (compute_feats.py:155-167).  conv_w is the trunk's
 * dsmil_resnet_num_convs(depth) conv tensors in state_dict order; bn_mean / bn_rstd are NULL for
 * InstanceNorm or the folded frozen-BatchNorm arrays (dsmil_resnet_norm_channels(depth) floats, see
 * dsmil_resnet18bn_forward); x is fp32 NCHW or uint8 NHWC.  Workspace as dsmil_resnet18_workspace_bytes
 * (the activation shapes do not depend on the depth).  The *18* entry points above are these with
 * depth = 18.  feats is [B, dsmil_resnet_feature_dim(depth)] (512 for BasicBlock trunks, 2048 for Bottleneck trunks); the
 * workspace of a Bottleneck trunk is larger: dsmil_resnet_workspace_bytes(depth, B, H, W). */
size_t dsmil_resnet_workspace_bytes(int32_t depth, int32_t B, int32_t H, int32_t W);
int32_t dsmil_resnet_feature_dim(int32_t depth);
int32_t dsmil_resnet_num_convs(int32_t depth);
/* Which matrix pipe the trunk's convolutions run on (for roofline accounting): plane products per fp32 MAC of the
 * Winograd convs (3x3 stride 1) and of the direct convs (3x3 stride 2, 1x1) — 3 = fp16 MFMA over two-plane cuts (round 5,
 * the product form), 9 / 6 = bf16 MFMA over exact three-plane cuts, 0 = v_mfma_f32_32x32x2_f32.  The product library has
 * one form (3 / 3); experiment builds read DSMIL_WINO / DSMIL_CONV once per process. */
int dsmil_resnet_mfma_forms(int32_t* wino_products, int32_t* direct_products);
int32_t dsmil_resnet_norm_channels(int32_t depth);
size_t dsmil_resnet_packed_bytes(int32_t depth);
int dsmil_resnet_pack(int32_t depth, const float* const* conv_w, float* packed, void* stream);
int dsmil_resnet_forward(int32_t depth, const void* x, int32_t x_is_u8_nhwc, int32_t B, int32_t H,
                         int32_t W, const float* conv1_w, const float* packed, const float* bn_mean,
                         const float* bn_rstd, const float* fc_w, const float* fc_b, int32_t C,
                         float* feats, float* classes, void* ws, size_t ws_bytes, void* stream);

/* OPT-IN reduced precision (round 5; no reference counterpart: the reference embeds in fp32, compute_feats.py:70-76).
 * precision = 0: the calls above (fp32-class: every conv as three fp16 plane products of two-plane cuts, csrc/resnet_fwd.hip
 * PlaneProducts<3>).  precision = 1: every conv operand — activations behind the norm + ReLU, and the weights — is rounded to ONE
 * fp16 plane (11 significand bits, round to nearest); products accumulate in f32 on the same MFMA; activations between the layers,
 * InstanceNorm statistics and the pooling stay fp32.  Feature error against the fp32-class path: ~2e-3 abs on features of O(1)
 * (tools/form_error_study.py `f16x1`, tests/test_resnet_gpu.py) — NOT the 1e-4 parity bar; for callers who ask for it
 * (compute_feats.py --precision half).  The packed image must come from dsmil_resnet_pack_ex with the SAME precision (same size as
 * dsmil_resnet_packed_bytes). */
int dsmil_resnet_pack_ex(int32_t depth, const float* const* conv_w, float* packed, int32_t precision, void* stream);
/* (ABI 5, round 6) precision = 2: the OPT-IN bf16-ACTIVATION trunk (csrc/resnet_b16.h; BASELINE.md's "bf16 MFMA / f32 accumulate"
 * row): behind the stem (which runs as in precision 1) every activation is stored in bf16 — NHWC with a one-pixel zero border —
 * and every conv is ONE bf16 MFMA product per MAC with f32 accumulation; InstanceNorm statistics are f32.  ResNet-18 / 34 with
 * InstanceNorm and patches between 64 x 64 and ~1000 pixels wide only (everything else: DSMIL_E_UNSUPPORTED); features agree with
 * precision 0 to bf16 rounding (max ~2e-2, mean ~3e-3 on features of magnitude ~1), NOT to the 1e-4 bar; 1.75-2x the rate of
 * precision 0.
 * precision = 3: the SAME trunk on fp16 activations (11 significant bits instead of 8: features within ~2.6e-3 of precision 0,
 * the class of precision 1, at the rate of precision 2) — activations and conv sums must stay inside fp16's +-65504: true for
 * InstanceNorm trunks with ordinary weights; a caller checks the first forward of a weight set for non-finite features (the
 * Python binding does, and falls back to precision 1).  compute_feats.py --precision half takes it where it applies.
 * The packed image of precisions 2 / 3 is LARGER: size it with dsmil_resnet_packed_bytes_ex(depth, precision) (0 = unsupported
 * depth / precision; precision 0 / 1 = dsmil_resnet_packed_bytes).  Workspace as for the other precisions.  The reference has
 * no such switch; compute_feats.py --precision bf16 exposes precision 2. */
size_t dsmil_resnet_packed_bytes_ex(int32_t depth, int32_t precision);
int dsmil_resnet_forward_ex(int32_t depth, const void* x, int32_t x_is_u8_nhwc, int32_t B, int32_t H, int32_t W,
                            const float* conv1_w, const float* packed, const float* bn_mean, const float* bn_rstd,
                            const float* fc_w, const float* fc_b, int32_t C, float* feats, float* classes, void* ws,
                            size_t ws_bytes, int32_t precision, void* stream);

/* ---- the stages of the 16-bit activation trunk ALONE — FOR TESTS (tests/test_trunk16_gpu.py; no reference counterpart: the
 * reference embeds in fp32, compute_feats.py:70-76).  The trunk of precision 2 / 3 (csrc/resnet_b16.h) is otherwise reachable
 * only end to end, where sixteen rounded conv + norm layers allow no tight bar; these entries run ONE stage of it on buffers the
 * caller controls, through the trunk's own host calls and launches (same kernels, same launch geometry), so that each kernel can be
 * compared with fp64 at a bar derived from its arithmetic.  No product path calls them.
 *   kind     1 = bf16, 2 = fp16 (the element type of precision 2 / 3)
 *   layout   a [B,H,W,C] map is stored as 16-bit NHWC with SHARED zero borders: image n owns rows n (H+1) .. n (H+1) + H of a flat
 *            [rows][W+1][C] array; row 0 of every image and column W of every row are zero, and one more zero row closes the last
 *            image: dsmil_trunk16_positions(B,H,W) = B (H+1) (W+1) + (W+1) positions of C elements.  16-bit buffers are raw uint16,
 *            16-byte aligned; every workspace is 256-byte aligned.
 *   dsmil_trunk16_layout   borders_only = 0: x_nhwc (fp32 [B,H,W,C]) -> out16 (k_b16_pad: rounds to nearest even, writes the zeros).
 *                          borders_only = 1: fills out16 with bytes 0x3C (finite, non-zero in both kinds), then k_b16_borders
 *                          alone: exactly the border positions become zero (x_nhwc is not read, may be NULL).
 *   dsmil_trunk16_conv     k_pack_b16 (fp32 OIHW weights -> fragment order, rounded to nearest even, into ws) + b16::run_conv:
 *                          in16 [positions(B,Hi,Wi), Cin] -> out16 [positions(B,Ho,Wo), Cout], Ho = (Hi + 2 pad - ks) / stride + 1;
 *                          border positions and the closing row are written as zeros.  Forms: 3x3 / stride 1 / pad 1 (Cin % 32 == 0,
 *                          Cout % 64 == 0, maps up to ~126 pixels wide at 64 -> 64 and Cout % 128 != 0, ~254 at Cout % 128 == 0),
 *                          3x3 / stride 2 / pad 1 and 1x1 / stride 2 / pad 0 (Cin % 64 == 0, Cout % 128 == 0).
 *   dsmil_trunk16_norm     run_stats + run_apply: y = [relu]((x - mean) rstd [+ idn]) per (image, channel), biased variance,
 *                          eps 1e-5, f32 statistics; idn16 may be NULL; idn16 with relu = 0 is no form of the trunk
 *                          (DSMIL_E_UNSUPPORTED); y16 may be x16.  Writes the B (H+1) (W+1) positions of the images (borders
 *                          as zeros), NOT the closing row.  C / 8 must divide 256, C <= 2048.
 *   dsmil_trunk16_pool     run_stats + k_pool_b16: feats[B,C] (fp32) = mean over pixels of relu((x - mean) rstd + idn); workspace
 *                          as for dsmil_trunk16_norm (dsmil_trunk16_norm_workspace_bytes: the statistics partials).
 *   dsmil_trunk16_forward  pack_all + b16::trunk on x_nhwc = fp32 [B,Hp,Wp,64] (what the stem hands over); conv_w: the
 *                          dsmil_resnet_num_convs(depth) device pointers of dsmil_resnet_pack (entry 0, the stem's, is not read);
 *                          depth 18 or 34; feats [B,512].
 * Every check runs BEFORE the first launch, in the order DSMIL_E_INVALID (null pointers, non-positive sizes, kind),
 * DSMIL_E_UNSUPPORTED (C % 8, the channel multiples and window limits above, maps of 2^31 elements or more), DSMIL_E_ALIGN,
 * DSMIL_E_WORKSPACE; the *_workspace_bytes queries answer 0 for arguments the entry refuses.
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): a caller finds them by symbol. */
size_t dsmil_trunk16_positions(int32_t B, int32_t H, int32_t W);
int dsmil_trunk16_layout(const float* x_nhwc, void* out16, int32_t B, int32_t H, int32_t W, int32_t C, int32_t kind,
                         int32_t borders_only, void* stream);
size_t dsmil_trunk16_conv_workspace_bytes(int32_t Cin, int32_t Cout, int32_t ks);
int dsmil_trunk16_conv(const void* in16, const float* w_oihw, void* out16, int32_t B, int32_t Hi, int32_t Wi, int32_t Cin,
                       int32_t Cout, int32_t ks, int32_t stride, int32_t pad, int32_t kind, void* ws, size_t ws_bytes,
                       void* stream);
size_t dsmil_trunk16_norm_workspace_bytes(int32_t B, int32_t C);
int dsmil_trunk16_norm(const void* x16, const void* idn16, void* y16, int32_t B, int32_t H, int32_t W, int32_t C, int32_t relu,
                       int32_t kind, void* ws, size_t ws_bytes, void* stream);
int dsmil_trunk16_pool(const void* x16, const void* idn16, float* feats, int32_t B, int32_t H, int32_t W, int32_t C,
                       int32_t kind, void* ws, size_t ws_bytes, void* stream);
size_t dsmil_trunk16_workspace_bytes(int32_t depth, int32_t B, int32_t Hp, int32_t Wp);
int dsmil_trunk16_forward(int32_t depth, const float* x_nhwc, int32_t B, int32_t Hp, int32_t Wp, const float* const* conv_w,
                          float* feats, int32_t kind, void* ws, size_t ws_bytes, void* stream);

/* ---- the stages of the fp32-class trunk ALONE (no reference counterpart): what tests/test_trunk32_gpu.py compares kernel by
 * kernel, and what the embedder's TRAINING forward is composed from (dsmil-wsi_amd/simclr.py).  The default
 * embedder path (fp32 activations, conv operands as two fp16 planes and three plane products: csrc/resnet_fwd.hip, csrc/wino_w1.h)
 * is otherwise reachable only as a whole network, where an InstanceNorm behind every conv rescales what a kernel got wrong; these
 * entries run ONE stage of it on buffers the caller controls, through the trunk's own host calls (plan_conv / pack_conv / run_conv,
 * plan_stem / pack_stem / launch_stem / finish_stem, launch_tail: what dsmil_resnet_pack and dsmil_resnet_forward call — same
 * kernels, same plans, same launch geometry).  The training path calls dsmil_trunk32_conv (and its size query, as the eligibility
 * answer) from NativeConv2d and NativeBasicBlock and dsmil_trunk32_tail from NativeBasicBlock; dsmil_trunk32_conv_plan and
 * dsmil_trunk32_stem are FOR TESTS and tools; the inference path calls none of them.
 *   precision  0 = the product form (two fp16 planes of each operand, products h0 w0 + h0 w1 + h1 w0), 1 = one fp16 plane
 *              (what precision 1 of dsmil_resnet_forward_ex runs); anything else is DSMIL_E_UNSUPPORTED.
 *   maps       fp32 NHWC, 16-byte aligned; statistics [B,C] fp32 (16-byte aligned where a kernel reads them: in_mean / in_rstd,
 *              the stem's and the tail's); every workspace is 256-byte aligned.
 *   dsmil_trunk32_conv_plan  host only, no launch: what plan_conv decides for this conv on B maps of H x W, as
 *                          DSMIL_T32_PLAN_INTS int32: [0] kernel (DSMIL_T32_W1 = k_conv_wino_w1, _UNIT = k_conv_wino_s3, _S6 =
 *                          k_conv_s6), [1] direct tile digits (42 = 128 px x 64 couts, 22 = 64 x 128, 24 = 64 x 256; 0 for
 *                          Winograd), [2..6] Winograd unit IB, TYB, TXB, nby, nbx (0 for direct), [7] Ho, [8] Wo, [9] statistics
 *                          slots per 32-pixel tile (direct; 0 for Winograd), [10] grid.x, [11] grid.y, [12] threads per
 *                          workgroup, [13] plane products per MAC, [14..15] 0.
 *   dsmil_trunk32_conv     the pack kernel the plan calls for (k_pack_wino_s3 / k_pack_conv_s6: w_oihw -> ws), then run_conv:
 *                          x [B,H,W,Cin] -> raw y [B,Ho,Wo,Cout] and mean / rstd [B,Cout] (biased variance, eps 1e-5) from the
 *                          conv's statistics partials (k_in_finalize_cnt / _flat) — or, with bn_m / bn_r [Cout] (both or neither),
 *                          those per-channel values for every image (fill_stats).  in_mean / in_rstd [B,Cin] (both or neither):
 *                          x is a raw map and is staged as relu((x - in_mean) in_rstd).  3x3 / stride 1 / pad 1 runs as Winograd
 *                          F(2x2,3x3), everything else direct.  ks 1 or 3, stride 1 or 2, pad <= ks / 2, Cin % 16 == 0,
 *                          Cout % 64 == 0, both <= 2048, each map under 2^31 elements.
 *   dsmil_trunk32_stem     k_pack_stem_s6 + k_stem_s6 + statistics + pool: x fp32 NCHW [B,3,H,W] or (x_is_u8_nhwc) uint8 NHWC, as
 *                          dsmil_resnet_forward takes -> pooled [B,Hp,Wp,64] = maxpool3x3/2(relu(norm(conv7x7/2(x)))), mean / rstd
 *                          [B,64].  Without bn_m / bn_r the InstanceNorm route (pool fused into the stem, k_in_finalize_stem,
 *                          k_pool_fix_norm); with bn_m / bn_r [64] (negative bn_r allowed) the frozen route (raw map, fill_stats,
 *                          k_norm_relu_maxpool).  H, W >= 32.
 *   dsmil_trunk32_tail     kind 0: out = relu((y2 - m2) r2 + idn); kind 1: out = relu((y2 - m2) r2 + (idn - md) rd) (idn = the raw
 *                          downsample branch; md / rd only here); kind 2: out [B,C] = mean over pixels of kind 0.  y2, idn, out
 *                          [B,HW,C]; k_norm_add_relu's grid is the forward's (8192 workgroups at most, grid stride beyond).  C / 4
 *                          must divide 256 or be a multiple of it (the rule dsmil_norm_bwd states too: one function,
 *                          csrc/emb_host.h).
 * Every check runs BEFORE the first launch, in the order DSMIL_E_INVALID (null pointers, pointer pairs half given, in place,
 * non-positive sizes, kind), DSMIL_E_UNSUPPORTED (precision, the forms, channel multiples and sizes above), DSMIL_E_ALIGN,
 * DSMIL_E_WORKSPACE; the *_workspace_bytes queries answer 0 for arguments the entry refuses.
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): a caller finds them by symbol. */
#define DSMIL_T32_W1 0
#define DSMIL_T32_UNIT 1
#define DSMIL_T32_S6 2
#define DSMIL_T32_OTHER 3       /* a kernel of experiment builds */
#define DSMIL_T32_PLAN_INTS 16
int dsmil_trunk32_conv_plan(int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad, int32_t B, int32_t H, int32_t W,
                            int32_t norm, int32_t precision, int32_t* plan);
size_t dsmil_trunk32_conv_workspace_bytes(int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad, int32_t B, int32_t H,
                                          int32_t W, int32_t precision);
int dsmil_trunk32_conv(const float* x, const float* w_oihw, const float* in_mean, const float* in_rstd, const float* bn_m,
                       const float* bn_r, float* y, float* mean, float* rstd, int32_t B, int32_t H, int32_t W, int32_t Cin,
                       int32_t Cout, int32_t ks, int32_t stride, int32_t pad, int32_t precision, void* ws, size_t ws_bytes,
                       void* stream);
size_t dsmil_trunk32_stem_workspace_bytes(int32_t B, int32_t H, int32_t W);
int dsmil_trunk32_stem(const void* x, int32_t x_is_u8_nhwc, const float* conv1_w, const float* bn_m, const float* bn_r,
                       float* pooled, float* mean, float* rstd, int32_t B, int32_t H, int32_t W, int32_t precision, void* ws,
                       size_t ws_bytes, void* stream);
int dsmil_trunk32_tail(int32_t kind, const float* y2, const float* m2, const float* r2, const float* idn, const float* md,
                       const float* rd, float* out, int32_t B, int32_t HW, int32_t C, int32_t precision, void* stream);

/* ---- background filters of the reference's tilers on decoded tiles -------------------------
 * tiles_nhwc: device uint8 [B,H,W,3] (W <= 1024).  out: device uint64 [B,4] = per tile
 *   {sum over band 0, band 1, band 2 of PIL's ImageFilter.FIND_EDGES image, sum of img_as_ubyte(rgb2hsv(img)[...,1])}.
 * deepzoom_tiler.py:56-61 keeps a tile when mean(out[0..2]) / tile_size^2 > threshold (default 15);
 * test_crop_single.py:17-24 keeps it when out[3] / (H*W) >= t (t = 30 at its call site).  The sums are exact
 * integers: forming the ratios in float64 on the host reproduces the reference's decisions bit for bit. */
int dsmil_tile_stats(const uint8_t* tiles_nhwc, int32_t B, int32_t H, int32_t W, uint64_t* out, void* stream);

/* ---- batched baseline-JPEG decode of a slide's tiles (ABI 5) -----------------------------------------
 * Replaces the per-tile `Image.open(path)` of the reference's loaders (compute_feats.py:28,107; attention_map.py:69-79:
 * Pillow / libjpeg-turbo in DataLoader worker processes) for baseline JPEG tiles (what deepzoom_tiler.py:64 writes): the
 * COMPRESSED bytes of a batch go to the device and are decoded there into uint8 NHWC — the input of
 * dsmil_resnet_forward_ex(x_is_u8_nhwc = 1) — bit for bit what Pillow's defaults produce (islow IDCT, fancy upsampling,
 * YCbCr -> RGB; a grey image gives R = G = B).  Scope: SOF0, 8 bit, Huffman, one interleaved scan, 1 or 3 components, luma
 * sampling 1x1 / 2x1 / 2x2 with 1x1 chroma, restart intervals, arbitrary tables, at most DSMIL_JPEG_MAX_QTABLES distinct
 * quantisation and DSMIL_JPEG_MAX_HTABLES distinct Huffman tables per batch (a tiler writes the same ones into every tile).
 *
 *   dsmil_jpeg_parse   HOST function (no device work): data = the files of the batch back to back in HOST memory, offsets
 *                      [n + 1]; fills `plan` (host memory, dsmil_jpeg_plan_bytes(n) bytes, 16-B aligned): one
 *                      dsmil_jpeg_image per file at byte offset 16 of the plan (status = DSMIL_OK, or DSMIL_E_UNSUPPORTED /
 *                      DSMIL_E_INVALID for a file outside the scope — the caller decodes THOSE with Pillow) followed by the
 *                      batch's de-duplicated tables.  The caller copies data and plan to the device as they are.
 *   dsmil_jpeg_decode  data (data_bytes = offsets[n] bytes), plan: the DEVICE copies; every image with status DSMIL_OK must be width x height; out_nhwc
 *                      device uint8 [n, height, width, 3] (rows of images with another status are left untouched);
 *                      status: device int32 [n] = the record's status, or DSMIL_E_INVALID when the entropy-coded data
 *                      turned out corrupt (the image is then undefined); ws: dsmil_jpeg_workspace_bytes(n, height, width,
 *                      data_bytes) bytes, 256-B aligned.  A memset and four launches on `stream`, no host synchronisation. */
#define DSMIL_JPEG_MAX_QTABLES 256   /* distinct quantisation tables per batch (128 B each in the plan) */
#define DSMIL_JPEG_MAX_HTABLES 64    /* distinct Huffman tables per batch (8.4 KiB each in the plan) */
typedef struct dsmil_jpeg_image {
    int64_t ecs_begin, ecs_end;   /* entropy-coded segment: byte offsets into `data` */
    int32_t width, height;
    int32_t ncomp;                /* 1 (grey) or 3 (YCbCr) */
    int32_t hsamp, vsamp;         /* luma sampling factors (chroma is 1x1) */
    int32_t restart_interval;     /* MCUs between RSTn markers, 0 = none */
    int32_t qt[3];                /* per component: index of its quantisation table in the plan */
    int32_t dc[3], ac[3];         /* per component: indices of its Huffman tables in the plan */
    int32_t status;               /* DSMIL_OK, DSMIL_E_UNSUPPORTED, DSMIL_E_INVALID */
} dsmil_jpeg_image;
size_t dsmil_jpeg_plan_bytes(int32_t n);
size_t dsmil_jpeg_workspace_bytes(int32_t n, int32_t height, int32_t width, int64_t data_bytes);
int dsmil_jpeg_parse(const uint8_t* data, const int64_t* offsets, int32_t n, void* plan);
int dsmil_jpeg_decode(const uint8_t* data, int64_t data_bytes, const void* plan, int32_t n, int32_t height, int32_t width,
                      uint8_t* out_nhwc, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- the reference's feature files (round 6; the data format on both sides of the embedder -> aggregator path) -----------
 * compute_feats.py:80-82 writes a bag's features as `pd.DataFrame(feats).to_csv(path, index=False, float_format='%.4f')` and
 * train_tcga.py:27-32 reads them back; pandas formats the 5.1 M numbers of a 10 000 x 512 bag in 5.4 s — 30-60x the time the
 * device needs to compute them.  dsmil_csv_format_f32 is a HOST function (no device work) that writes the SAME BYTES for the
 * data rows: x float32 [rows, cols] in host memory (rows `row_stride` elements apart), `decimals` in 0..9 (the reference: 4);
 * fields separated by ',', rows ended by '\n', NaN an empty field, infinities 'inf' / '-inf', negative zero '-0.0000' (what
 * pandas writes).  out: at least 64 bytes per value.  Returns the number of bytes written, DSMIL_E_WORKSPACE when `cap` is too
 * small, DSMIL_E_INVALID for bad arguments.  Thread-safe (the caller formats row blocks in parallel). */
int64_t dsmil_csv_format_f32(const float* x, int64_t rows, int64_t cols, int64_t row_stride, int32_t decimals, char* out, int64_t cap);
/* ... and the way back (train_tcga.py:27-32 `pd.read_csv(path)`, then `torch.tensor(..., dtype=torch.float32)`): text = the
 * DATA rows of a feature file (the caller skips the header line), `cols` fields per row -> out float32 [max_rows, cols].  HOST
 * function, thread-safe (the caller parses chunks that end at a line break in parallel).  A '%.4f' field parses to the double
 * pandas' parser gives (one correctly rounded division by 10^4) and is cast to float32 as torch casts it; exponents, 'inf',
 * 'nan', long fields go through strtod; an empty field is NaN; blank lines are skipped.  Returns the rows parsed, or
 * DSMIL_E_INVALID (a field that is not a number, a row of another width, more than max_rows rows: let pandas read the file). */
int64_t dsmil_csv_parse_f32(const char* text, int64_t nbytes, int64_t cols, float* out, int64_t max_rows);
/* The loader's file reads (compute_feats.py:21-56: DataLoader workers open every tile file) — HOST function, thread-safe: n files
 * (paths: NUL-terminated strings back to back, path_off[i] = offset of path i) back to back into `out`; with out == NULL only
 * their sizes (the caller sizes the buffer from the returned total).  sizes[i] = bytes of file i, -1 when it cannot be opened or
 * read.  Returns the total bytes, DSMIL_E_WORKSPACE when `cap` is too small, DSMIL_E_INVALID for bad arguments.  One call per
 * group of files from a Python thread holds no interpreter lock: 25 us of interpreter time per file otherwise, serialised. */
int64_t dsmil_read_files(const char* paths, const int64_t* path_off, int32_t n, uint8_t* out, int64_t cap, int64_t* sizes);

const char* dsmil_strerror(int code);
int dsmil_abi_version(void);
/* Rows per workgroup the launcher picks for the dominant kernel (k_query_attend). */
int dsmil_agg_tile_rows(int32_t n_bags, int64_t total_rows);

/* ---- the aggregator forward's route: which kernels a call takes ----------------------------------------------------------
 * Every forward entry point (dsmil_agg_forward, _ex, _bf16, dsmil_agg_shard_argmax, dsmil_agg_shard_attend, the training
 * step) describes its call as a dsmil_agg_call and launches what the ONE route function of the library (pick_route,
 * csrc/agg_fwd.hip) answers for it.  dsmil_agg_forward_route asks the same function without touching a device, a stream or
 * the library's record of recent streams.  It reads the run-time knobs as they stand (dsmil_agg_batch_form,
 * dsmil_agg_inline_query, dsmil_agg_logits_form).  Diagnostic: the values below name kernels of THIS library build.
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): a caller finds it by symbol. */
typedef struct dsmil_agg_call {
    int64_t total_rows, max_rows;
    int32_t n_bags, K, Kv, C, nonlinear;
    int32_t bf16;            /* dsmil_agg_forward_bf16 (features, values stored as bf16) */
    int32_t aligned;         /* 16-byte alignment of the fp32 operands, bit 0: feats, vals, fc_w, q0_w and q2_w (all of them);
                              * bit 1: fc_w and q0_w; bit 2: crit_rows and q0_w (dsmil_agg_shard_attend) */
    int32_t classes_given;   /* classes_in != NULL */
    int32_t vals_separate;   /* vals != NULL and != feats */
    int32_t row_map;         /* dsmil_agg_opts::row_map != NULL */
    int32_t packed_split;    /* dsmil_agg_opts::packed_split != NULL */
    int32_t packed_f2;       /* dsmil_agg_opts::packed_f2 != NULL */
    int32_t phase;           /* 0 a whole forward, 1 dsmil_agg_shard_argmax, 2 dsmil_agg_shard_attend */
    int32_t skip_pred;       /* the training step: the bag head is left to the caller's next launch */
    int32_t prologue_job;    /* the training step: the logits launch is asked to carry the prologue job */
    int32_t several_streams; /* the library has recently been called on more than one stream (dsmil_agg_logits_form(1)) */
    int32_t cus;             /* compute units of the device; 0 = ask the current device */
} dsmil_agg_call;

enum { DSMIL_LOGITS_NONE = 0, DSMIL_LOGITS_GIVEN, DSMIL_LOGITS_STREAM, DSMIL_LOGITS_PIPE, DSMIL_LOGITS_ARGMAX };
enum { DSMIL_QMAX_LAUNCH = 0, DSMIL_QMAX_INLINE, DSMIL_QMAX_SHARD1, DSMIL_QMAX_SHARD2 };
enum { DSMIL_IMAGE_NONE = 0, DSMIL_IMAGE_F2_CALLER, DSMIL_IMAGE_F2_CUT, DSMIL_IMAGE_SPLIT_CALLER, DSMIL_IMAGE_SPLIT_CUT,
       DSMIL_IMAGE_BF16 };
enum { DSMIL_ATTEND_NONE = 0, DSMIL_ATTEND_F3, DSMIL_ATTEND_F2, DSMIL_ATTEND_BF16_RES, DSMIL_ATTEND_BF16_DMA,
       DSMIL_ATTEND_BF16_RING, DSMIL_ATTEND_SPLIT, DSMIL_ATTEND_HS, DSMIL_ATTEND_F32 };
enum { DSMIL_FINISH_NONE = 0, DSMIL_FINISH_LEAN, DSMIL_FINISH_VEC4, DSMIL_FINISH_SCALAR };

typedef struct dsmil_agg_route {
    int32_t nw;             /* tile regime: 4 = 128-row workgroups, 1 = 32-row (dsmil_agg_tile_rows / 32) */
    int32_t r0;             /* rows per workgroup of the logits pass (= the tile of the arg-max partials) */
    int32_t logits;         /* DSMIL_LOGITS_*: none (shard phase 2) / k_logits_argmax on given classes / k_logits_stream /
                             * k_logits_pipe / k_logits_argmax */
    int32_t logits_vec;     /* k_logits_argmax: 4 = 16-byte loads, 1 = scalar */
    int32_t logits_cp;      /* k_logits_stream, k_logits_pipe: classes per pass (1 or 2) */
    int32_t prologue;       /* the logits launch carries the training step's prologue job */
    int32_t rowmax;         /* the logits launch leaves max |x| per row (k_attend_f2 / k_attend_f3) */
    int32_t qmax;           /* DSMIL_QMAX_*: k_qmax launch / inside k_attend_hs / the shard phases' forms of k_qmax */
    int32_t qmax_vec;       /* k_qmax: 4 or 1 */
    int32_t qmax_threads;   /* k_qmax: 1024, or 256 behind k_logits_pipe */
    int32_t ragged;         /* k_tile_prefix runs: the logits pass works from the list of real tiles */
    int32_t ragged_attend;  /* ... and so does the (persistent) attend kernel */
    int32_t tile_attend;    /* k_tile_prefix: rows per tile of the attend list ... */
    int32_t tile_logits;    /* ... and of the logits list */
    int32_t image;          /* DSMIL_IMAGE_*: the weight image the attend kernel reads and who cuts it */
    int32_t attend;         /* DSMIL_ATTEND_* */
    int32_t attend_nw;      /* waves per 32 rows x this = rows per tile of the ring / split / f32 kernels (4 or 1) */
    int32_t attend_vec;     /* split / f32 kernels: 4 = DMA tile, 1 = register-staged tile */
    int32_t attend_np;      /* split kernel: plane products (6; 9 in experiment builds) */
    int32_t attend_xe;      /* experiment builds: ablation forms of the split kernel (0 in the product library) */
    int32_t attend_tu;
    int32_t finish;         /* DSMIL_FINISH_*: k_finish<4, 2> / k_finish<4> / k_finish<1>; none under the stamp-trace knob */
    int32_t finish_rows;    /* rows per partial tile k_finish is told */
    int32_t pred;           /* k_pred runs */
} dsmil_agg_route;

/* Fills *route for *call.  DSMIL_E_INVALID for null pointers or non-positive sizes, else DSMIL_OK.  HOST function. */
int dsmil_agg_forward_route(const dsmil_agg_call* call, dsmil_agg_route* route);

/* NT-Xent, the SimCLR pre-training loss of the embedder.  Replaces NTXentLoss.forward (simclr/loss/nt_xent.py:47-65: the
 * concatenation, the [2n, 2n] similarity matrix of :40-45 (cosine) or :33-38 (dot), the positives / negatives gather of
 * :53-60 and CrossEntropyLoss(reduction="sum") / 2n of :63-65) and its autograd, without ever forming the matrix:
 *   zis, zjs     device [n, d] fp32 row-major (the two views' projections); R = cat([zjs, zis]) as nt_xent.py:48
 *   temperature  > 0;  cosine != 0: cosine similarity with torch's eps = 1e-8 on the norms, 0: dot products
 *   loss         device [1]:  (1/2n) sum_a [ logsumexp_{b != a}(S_ab / T) - S_{a, (a + n) mod 2n} / T ]
 *   lse          device [2n]: the rows' log-sum-exp, which the backward reads
 *   g_loss       device [1]:  the upstream gradient (read on the device: no host synchronisation)
 *   g_zis, g_zjs device [n, d]: d loss / d zis, d loss / d zjs times g_loss[0]
 *   ws           device, 256-byte aligned, dsmil_ntxent_workspace_bytes(n, d) bytes: O(n d).  The backward rebuilds what it
 *                needs from zis / zjs / lse: it does not depend on what a forward left in ws.
 * 2n <= 2^17 and d <= 4096 (any d: padded to the MFMA k-step), else DSMIL_E_UNSUPPORTED (the size function returns 0).
 * Arithmetic: two fp16 planes of the (normalised) rows, three plane products per MAC on v_mfma_f32_16x16x32_f16, fp32
 * accumulation; split partials combined in a fixed order — results are bit-identical from call to call. */
size_t dsmil_ntxent_workspace_bytes(int64_t n, int d);
int dsmil_ntxent_forward(const float* zis, const float* zjs, int64_t n, int d, float temperature, int cosine, float* loss,
                         float* lse, void* ws, size_t ws_bytes, void* stream);
int dsmil_ntxent_backward(const float* zis, const float* zjs, int64_t n, int d, float temperature, int cosine, const float* lse,
                          const float* g_loss, float* g_zis, float* g_zjs, void* ws, size_t ws_bytes, void* stream);

/* SimCLR's two-view augmentation (simclr/data_aug/dataset_wrapper.py:48-58, twice per patch) on decoded tiles: one record per
 * OUTPUT view, the reference's chain on uint8 RGB stage by stage —
 *   1. crop (i, j, h, w) of tile `tile`, resized to S x S as Pillow's Image.resize(BILINEAR) does it: the horizontal pass first,
 *      rounded to uint8, then the vertical one; coefficients in double, normalised, 22-bit fixed point, accumulator from 1 << 21;
 *      support max(1, w / S); a pass whose in and out sizes agree is skipped
 *   2. horizontal flip                                                              (DSMIL_SIMCLR_FLIP)
 *   3. colour jitter (DSMIL_SIMCLR_JITTER): the four operations in the order packed into `order` (operation k at bits 2k, 2k + 1:
 *      0 brightness, 1 contrast, 2 saturation, 3 hue), each Pillow's ImageEnhance = Image.blend(degenerate, image, factor) in
 *      fp32 with truncation (clipping for factors outside [0, 1]); hue = RGB -> HSV, H += hue (mod 256), HSV -> RGB with
 *      Pillow's widths (Convert.c)
 *   4. greyscale (DSMIL_SIMCLR_GREY): L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in the three channels
 *   5. Gaussian blur (DSMIL_SIMCLR_BLUR): separable, ksize = (int)(0.06 S) taps, weights exp(-(t - (ksize - 1) / 2)^2 / (2 sigma^2))
 *      normalised, reflect-101 border, fp32 without rounding between the passes, rounded to nearest at the end.  The
 *      real-arithmetic definition: cv2.GaussianBlur works in fixed point on 8-bit images and may differ by a level or two.
 *   6. out_nchw (fp32 [n_views, 3, S, S], byte / 255.0f) and / or out_nhwc (uint8 [n_views, S, S, 3]); either may be NULL.
 * 8 <= H, W <= 256;  17 <= S <= 256 with (int)(0.06 S) odd, else DSMIL_E_UNSUPPORTED (the size function returns 0).
 * dsmil_simclr_views: every pointer a device pointer; asynchronous on `stream`, no host synchronisation, no allocation.  A record
 * whose tile or crop lies outside the batch reads nothing and yields an all-zero view (the caller validates on the host).
 * dsmil_simclr_views_host: HOST function, host pointers, the same per-pixel arithmetic compiled for the host; ws is unused (may
 * be NULL); a bad record is DSMIL_E_INVALID.
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): a caller finds them by symbol. */
enum { DSMIL_SIMCLR_FLIP = 1, DSMIL_SIMCLR_JITTER = 2, DSMIL_SIMCLR_GREY = 4, DSMIL_SIMCLR_BLUR = 8 };
typedef struct dsmil_simclr_view {
    int32_t tile;                 /* source tile of the batch */
    int32_t i, j, h, w;           /* crop: top, left, height, width */
    int32_t flags;                /* DSMIL_SIMCLR_* */
    int32_t order;                /* the jitter's order, 2 bits per position */
    int32_t hue;                  /* the byte added to H: trunc(hue_factor * 255) mod 256 */
    float brightness, contrast, saturation;   /* blend factors */
    float sigma;                  /* of the blur */
} dsmil_simclr_view;
size_t dsmil_simclr_views_workspace_bytes(int64_t n_views, int H, int W, int S);
int dsmil_simclr_views(const uint8_t* tiles_nhwc, int64_t n_tiles, int H, int W, const dsmil_simclr_view* views, int64_t n_views,
                       int S, float* out_nchw, uint8_t* out_nhwc, void* ws, size_t ws_bytes, void* stream);
int dsmil_simclr_views_host(const uint8_t* tiles_nhwc, int64_t n_tiles, int H, int W, const dsmil_simclr_view* views,
                            int64_t n_views, int S, float* out_nchw, uint8_t* out_nhwc, void* ws, size_t ws_bytes);

/* Convolution backward for training the embedder (csrc/conv_bwd.hip): the weight gradient and the data gradient of one conv
 * of the ResNet trunks, in the layout and arithmetic class of dsmil_trunk32_conv — fp32 NHWC maps, fp32 OIHW weights, two
 * round-to-nearest fp16 planes per operand, the products h0 w0 + h0 w1 + h1 w0 added smallest first, fp32 accumulation on
 * v_mfma_f32_32x32x16_f16.  With Ho = (H + 2 pad - ks) / stride + 1 (Wo alike):
 *   weight   dw[co][ci][ky][kx] = sum_{n,oy,ox} dy[n,oy,ox,co] v[n, oy stride - pad + ky, ox stride - pad + kx, ci]
 *            v = x, or relu((x - in_mean[n,ci]) in_rstd[n,ci]) when in_mean / in_rstd [B,Cin] are given (both or neither): the
 *            operand the forward's NORM form stages.  Taps outside the map contribute exact zeros.
 *   data     dx[n,iy,ix,ci] = sum_{ky,kx,co} dy[n, (iy + pad - ky) / stride, (ix + pad - kx) / stride, co] w[co][ci][ky][kx]
 *            over the taps whose division is exact and lands in the map (a gather: a pixel no output reads gets +0).
 *   x, dx    device [B,H,W,Cin] fp32;   dy device [B,Ho,Wo,Cout] fp32;   w_oihw, dw_oihw device [Cout,Cin,ks,ks] fp32
 *   ws       device, 256-byte aligned, dsmil_conv_bwd_workspace_bytes(..., which) bytes; which = DSMIL_CONV_BWD_WEIGHT / _DATA
 * Scaling.  The weights carry the forward's 2^8.  dy has no natural range: every call takes max |dy| on the device (no host read)
 * and multiplies dy by 2^s at staging, s = 14 - e for max |dy| = f 2^e, f in [0.5, 1) (s clamped to +-60, 0 for an all-zero
 * dy): the largest element lands in [2^13, 2^14).  2^-s (and 2^-8) are taken out behind the accumulation; all of it is exact.
 * Order.  The weight gradient deals the B Ho Wo positions to workgroups in chunks of plan[CHUNK]; each (chunk, tile) writes one
 * fp32 partial and a finish kernel adds the n_partials partials of an element in chunk order.  No atomics anywhere: two calls on
 * the same inputs are bit-identical.  A call never reads what another call left in ws.
 * Limits, else DSMIL_E_UNSUPPORTED before any launch (the size function returns 0): Cin % 16 == 0 (or Cin == 3 for the weight
 * gradient: the stem, its 147 columns padded with exact zeros), Cout % 64 == 0, ks in {1, 3, 7}, stride in {1, 2}, pad <= ks / 2,
 * at least one output pixel, every element count below 2^31.  Null pointers are DSMIL_E_INVALID, x / dy / dx / statistics off 16
 * bytes or ws off 256 DSMIL_E_ALIGN, a short workspace DSMIL_E_WORKSPACE.  Asynchronous on `stream`; nothing is allocated.
 * dsmil_conv_bwd_plan is a HOST function: out[DSMIL_CONV_BWD_PLAN_*], the rest 0.
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): a caller finds them by symbol. */
enum { DSMIL_CONV_BWD_WEIGHT = 0, DSMIL_CONV_BWD_DATA = 1 };
enum {
    DSMIL_CONV_BWD_PLAN_WHICH = 0,
    DSMIL_CONV_BWD_PLAN_HO = 1,         /* the map of dy */
    DSMIL_CONV_BWD_PLAN_WO = 2,
    DSMIL_CONV_BWD_PLAN_OUT0 = 3,       /* rows of the output GEMM: Cout (weight), B H W (data) */
    DSMIL_CONV_BWD_PLAN_OUT1 = 4,       /* its columns: Cin ks ks (weight), Cin (data) */
    DSMIL_CONV_BWD_PLAN_GRID_X = 5,
    DSMIL_CONV_BWD_PLAN_GRID_Y = 6,
    DSMIL_CONV_BWD_PLAN_GRID_Z = 7,
    DSMIL_CONV_BWD_PLAN_BLOCK = 8,
    DSMIL_CONV_BWD_PLAN_CHUNK = 9,      /* weight: positions per chunk; data: 0 */
    DSMIL_CONV_BWD_PLAN_PARTIALS = 10,  /* partials a dw element is summed from (data: 1) */
    DSMIL_CONV_BWD_PLAN_RUN_LEN = 11,   /* the longest run of contraction indices one accumulator sums: positions (weight),
                                           Cout ks ks (data) */
    DSMIL_CONV_BWD_PLAN_COLS_PAD = 12   /* weight: the Cin ks ks columns padded to the tile; data: 0 */
};
int dsmil_conv_bwd_plan(int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad, int32_t B, int32_t H, int32_t W,
                        int32_t which, int32_t out[16]);
size_t dsmil_conv_bwd_workspace_bytes(int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad, int32_t B, int32_t H,
                                      int32_t W, int32_t which);
int dsmil_conv_bwd_weight(const float* x, const float* in_mean, const float* in_rstd, const float* dy, float* dw_oihw, int32_t B,
                          int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad, void* ws,
                          size_t ws_bytes, void* stream);
int dsmil_conv_bwd_data(const float* dy, const float* w_oihw, float* dx, int32_t B, int32_t H, int32_t W, int32_t Cin,
                        int32_t Cout, int32_t ks, int32_t stride, int32_t pad, void* ws, size_t ws_bytes, void* stream);

/* InstanceNorm / ReLU / residual-add backward for training the embedder (csrc/norm_bwd.hip): the gradient of a RAW conv output
 * from the gradient of what the forward made of it, in the layout of dsmil_trunk32_conv / dsmil_trunk32_tail — fp32 NHWC maps
 * [B,HW,C], statistics [B,C] fp32 (biased variance, no affine).  For a map t with statistics (m, r), x^ = (t - m) r and a masked
 * upstream gradient q:
 *     INB(q; t, m, r)[n,p,c] = r[n,c] ( q[n,p,c] - mean_p q[n,.,c] - x^[n,p,c] mean_p (q x^)[n,.,c] )
 *   DSMIL_NORM_BWD_RELU      g = the gradient of a = relu((y - mean) rstd), the operand dsmil_trunk32_conv stages and
 *                            dsmil_conv_bwd_data differentiates against.  q = g where fl(fl(y - mean) rstd) > 0 (the forward's own
 *                            fp32 evaluation), else 0;  gy = INB(q; y, mean, rstd).  out, yd, md, rd, gyd, gres are NULL.
 *   DSMIL_NORM_BWD_ADD       g = the gradient of out = relu((y - mean) rstd + idn) (dsmil_trunk32_tail kind 0).  q = g where the
 *                            saved out > 0, else 0;  gy = INB(q; y, mean, rstd);  gres = q, the gradient of idn.  yd, md, rd, gyd
 *                            are NULL.
 *   DSMIL_NORM_BWD_ADD_DOWN  as ADD for tail kind 1: gy as above and gyd = INB(q; yd, md, rd); g and out are read once for both
 *                            branches.  gres is NULL.
 *   ws       device, 256-byte aligned, dsmil_norm_bwd_workspace_bytes(kind, B, HW, C) bytes, any contents
 * Arithmetic, all fp32: x^ = fl(fl(t - m) r); the sums of q and of q x^ (fmaf) per (n, c); mean = sum / HW (a correctly rounded
 * division); gy = fl(r fmaf(-x^, mean(q x^), fl(q - mean q))).
 * Order.  The HW pixels of an image are dealt to chunks of plan[CHUNK]; inside a chunk plan[LANES] threads per channel each add
 * every LANES-th pixel serially (at most plan[RUN_LEN] terms per accumulator), their LANES sums are combined in a fixed tree
 * (xor shuffles inside a wave, then the waves through LDS in wave order) into one fp32 partial in ws; the plan[PARTIALS] partials
 * of an (n, c) are added in chunk order; the element pass then runs.  No atomics anywhere: two calls on the same inputs are
 * bit-identical, and a call never reads what another call left in ws.  HW = 1 (with mean = y), a channel whose every element is
 * masked and an all-zero g give exact zeros.
 * Checks, all before the first launch, in this order: DSMIL_E_INVALID (unknown kind; non-positive sizes; a NULL pointer the
 * kind needs, or one given that the kind forbids; an output sharing a byte with an input or with another output);
 * DSMIL_E_UNSUPPORTED (C % 4 != 0, C / 4 neither dividing 256 nor a multiple of it, C > 2048, B HW C >= 2^31; the size function
 * returns 0); DSMIL_E_ALIGN (maps or statistics off 16 bytes, ws off 256); DSMIL_E_WORKSPACE (a short workspace).  Asynchronous
 * on `stream`; nothing is allocated.  dsmil_norm_bwd_plan is a HOST function: out[DSMIL_NORM_BWD_PLAN_*], the rest 0.
 * Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature moved): a caller finds them by symbol. */
enum { DSMIL_NORM_BWD_RELU = 0, DSMIL_NORM_BWD_ADD = 1, DSMIL_NORM_BWD_ADD_DOWN = 2 };
enum {
    DSMIL_NORM_BWD_PLAN_KIND = 0,
    DSMIL_NORM_BWD_PLAN_CHUNK = 1,         /* pixels per chunk */
    DSMIL_NORM_BWD_PLAN_PARTIALS = 2,      /* partials per (n, c) and sum: ceil(HW / chunk) */
    DSMIL_NORM_BWD_PLAN_RUN_LEN = 3,       /* the longest serial run of terms one accumulator adds: ceil(min(HW, chunk) / lanes) */
    DSMIL_NORM_BWD_PLAN_LANES = 4,         /* accumulators per channel and chunk, combined in a fixed tree: 256 / min(C / 4, 256) */
    DSMIL_NORM_BWD_PLAN_SUMS = 5,          /* sums per (n, c): 2, ADD_DOWN 3 */
    DSMIL_NORM_BWD_PLAN_GRID_PARTIAL = 6,  /* workgroups of the chunk sums: B * partials */
    DSMIL_NORM_BWD_PLAN_GRID_FINISH = 7,   /* of the pass that adds the partials */
    DSMIL_NORM_BWD_PLAN_GRID_APPLY = 8,    /* of the element pass: 8192 at most, grid stride beyond */
    DSMIL_NORM_BWD_PLAN_BLOCK = 9,         /* threads per workgroup of every launch */
    DSMIL_NORM_BWD_PLAN_GROUPS = 10        /* 4-channel groups per thread: 1, or 2 at C = 2048 */
};
int dsmil_norm_bwd_plan(int32_t kind, int32_t B, int32_t HW, int32_t C, int32_t out[16]);
size_t dsmil_norm_bwd_workspace_bytes(int32_t kind, int32_t B, int32_t HW, int32_t C);
int dsmil_norm_bwd(int32_t kind, const float* g, const float* out, const float* y, const float* mean, const float* rstd,
                   const float* yd, const float* md, const float* rd, float* gy, float* gyd, float* gres, int32_t B, int32_t HW,
                   int32_t C, void* ws, size_t ws_bytes, void* stream);

/* The stem on the training path (csrc/resnet_fwd.hip, csrc/stem_bwd.hip): a forward that keeps what the backward needs, and the
 * gradient of the RAW stem map from the gradient of pooled = maxpool3x3/2/1(relu((y - mean) rstd)).  fp32 NHWC maps, statistics
 * [B,C] fp32 (biased variance, eps 1e-5, no affine), H1 = (H - 1) / 2 + 1 for the 7x7/2/3 conv and Hp = (H1 - 1) / 2 + 1 for the
 * pool (the same for the widths).
 *   dsmil_trunk32_stem_train   dsmil_trunk32_stem's InstanceNorm route on its two-kernel form (k_pack_stem_s6, k_stem_s6 writing
 *                              the raw map, k_in_finalize_stem) and a pool pass that records the winners:
 *                              x fp32 NCHW [B,3,H,W] or (x_is_u8_nhwc) uint8 NHWC, conv1_w OIHW [64,3,7,7] ->
 *                              y [B,H1,W1,64] (the caller's buffer), mean / rstd [B,64], pooled [B,Hp,Wp,64], win [B,Hp,Wp,64] uint8.
 *                              pooled, mean and rstd are bit-identical to dsmil_trunk32_stem's on the same input.
 *     Winner rule, all fp32: a = fl(fl(y - mean) rstd).  The window of pooled pixel (oy, ox) is rows 2 oy - 1 .. 2 oy + 1 and
 *     columns 2 ox - 1 .. 2 ox + 1, clipped to the map; win = dy * 3 + dx (0..8, dy = row - (2 oy - 1), dx = column - (2 ox - 1): the
 *     position in the UNCLIPPED window, row-major) of the FIRST pixel in row-major order whose a equals the window's largest a —
 *     a later value replaces the current one only if strictly greater, max_pool2d's rule.  The rule is on a, not on y: two
 *     different y may round to one a.  Non-finite inputs are unspecified.
 *     Checks in dsmil_trunk32_stem's order: DSMIL_E_INVALID (a null pointer, non-positive sizes), DSMIL_E_UNSUPPORTED (precision
 *     other than 0 / 1; H or W < 32; B > 65535; B 3 H W or B H1 W1 64 >= 2^31), DSMIL_E_ALIGN (x off 4 bytes unless uint8,
 *     conv1_w or win off 4, y / pooled / mean / rstd off 16, ws off 256), DSMIL_E_WORKSPACE.  The size query answers 0 for what
 *     the entry refuses.
 *   dsmil_stem_pool_bwd        g [B,Hp,Wp,C] = the gradient of pooled, y [B,H1,W1,C], mean / rstd [B,C], win [B,Hp,Wp,C] -> gy
 *                              [B,H1,W1,C]:
 *         q[n,p,c]  = sum over the windows whose winner is p of g[n,w,c]   if fl(fl(y - mean) rstd)[n,p,c] > 0, else 0
 *         gy        = INB(q; y, mean, rstd)                                (the INB of dsmil_norm_bwd, the same fp32 arithmetic)
 *     A GATHER over the pixels of y: a pixel lies in at most four windows — one per dimension for an even coordinate, two for an
 *     odd one — and takes g of a window where win names its position; the (at most four) terms are added in window row-major
 *     order starting from + 0, a window it did not win contributing an exact + 0.  Then, as dsmil_norm_bwd: x^ = fl(fl(y - mean)
 *     rstd); the sums of q and of fma(q, x^) per (n, c); mean = sum / (H1 W1), a correctly rounded division; gy = fl(rstd
 *     fma(-x^, mean(q x^), fl(q - mean q))).
 *     Order.  The H1 W1 pixels of an image, row-major, are dealt to chunks of plan[CHUNK]; inside a chunk plan[LANES] threads per
 *     channel each add every LANES-th pixel serially (at most plan[RUN_LEN] terms per accumulator), their sums are combined in a
 *     fixed tree (xor shuffles inside a wave, then the waves through LDS in wave order) into one partial in ws; the
 *     plan[PARTIALS] partials of an (n, c) are added in chunk order; the element pass then runs.  No atomics anywhere: two calls
 *     on the same inputs are bit-identical, and a call never reads what another call left in ws.  An all-zero g and a channel
 *     whose every element is masked give exact zeros.  win values that no pixel of the window holds select nothing.
 *     Checks, all before the first launch, in this order: DSMIL_E_INVALID (non-positive sizes, a NULL pointer, gy sharing a
 *     byte with an input); DSMIL_E_UNSUPPORTED (C % 4 != 0, C / 4 neither dividing 256 nor a multiple of it, C > 2048,
 *     B H1 W1 C >= 2^31; the size function returns 0); DSMIL_E_ALIGN (g, y, mean, rstd or gy off 16 bytes, win off 4, ws off
 *     256); DSMIL_E_WORKSPACE.  ws: device, 256-byte aligned, dsmil_stem_pool_bwd_workspace_bytes bytes, any contents.
 *     dsmil_stem_pool_bwd_plan is a HOST function: out[DSMIL_STEM_BWD_PLAN_*], the rest 0.
 * Asynchronous on `stream`; nothing is allocated.  Added without a change of DSMIL_ABI_VERSION (it stays 6, no existing signature
 * moved): a caller finds them by symbol. */
enum {
    DSMIL_STEM_BWD_PLAN_HP = 0,            /* the pooled map: (H1 - 1) / 2 + 1 */
    DSMIL_STEM_BWD_PLAN_WP = 1,
    DSMIL_STEM_BWD_PLAN_CHUNK = 2,         /* pixels of y per chunk: 256, doubled while B chunks > 2048, 4096 at most */
    DSMIL_STEM_BWD_PLAN_PARTIALS = 3,      /* partials per (n, c) and sum: ceil(H1 W1 / chunk) */
    DSMIL_STEM_BWD_PLAN_RUN_LEN = 4,       /* the longest serial run of terms one accumulator adds: ceil(min(H1 W1, chunk) / lanes) */
    DSMIL_STEM_BWD_PLAN_LANES = 5,         /* accumulators per channel and chunk, combined in a fixed tree: 256 / min(C / 4, 256) */
    DSMIL_STEM_BWD_PLAN_GRID_PARTIAL = 6,  /* workgroups of the chunk sums: B * partials */
    DSMIL_STEM_BWD_PLAN_GRID_FINISH = 7,   /* of the pass that adds the partials */
    DSMIL_STEM_BWD_PLAN_GRID_APPLY = 8,    /* of the element pass: 8192 at most, grid stride beyond */
    DSMIL_STEM_BWD_PLAN_BLOCK = 9,         /* threads per workgroup of every launch */
    DSMIL_STEM_BWD_PLAN_GROUPS = 10        /* 4-channel groups per thread: 1, or 2 at C = 2048 */
};
size_t dsmil_trunk32_stem_train_workspace_bytes(int32_t B, int32_t H, int32_t W);
int dsmil_trunk32_stem_train(const void* x, int32_t x_is_u8_nhwc, const float* conv1_w, float* y, float* mean, float* rstd,
                             float* pooled, uint8_t* win, int32_t B, int32_t H, int32_t W, int32_t precision, void* ws,
                             size_t ws_bytes, void* stream);
int dsmil_stem_pool_bwd_plan(int32_t B, int32_t H1, int32_t W1, int32_t C, int32_t out[16]);
size_t dsmil_stem_pool_bwd_workspace_bytes(int32_t B, int32_t H1, int32_t W1, int32_t C);
int dsmil_stem_pool_bwd(const float* g, const float* y, const float* mean, const float* rstd, const uint8_t* win, float* gy,
                        int32_t B, int32_t H1, int32_t W1, int32_t C, void* ws, size_t ws_bytes, void* stream);

/* Measurement hooks (bench.py's roofline leg; no reference counterpart).  While enabled, every
 * launch of a dominant kernel is bracketed by hipEventRecord on its own launch stream (up to 4096
 * launches per channel: 0 = k_query_attend of the aggregator, 1 = k_conv of the embedder);
 * dsmil_profile_collect() synchronises on them, returns the summed kernel time and the launch
 * count of one channel, and resets it.  Not for use under graph capture. */
int dsmil_profile_enable(int on);
int dsmil_profile_collect(int channel, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* DSMIL_HIP_H */
