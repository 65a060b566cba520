// agg_bwd_bags.h — the aggregator backward over a BATCH of bags stored back to back (dsmil_agg_backward_bags) and the
// batched loss head (dsmil_agg_loss_head_bags).  Included from agg_bwd.hip, behind the one-bag kernels it builds on.
//
// What train_tcga.py:60-73 does for one bag, applied to n_bags bags with ONE summed gradient (minibatch training; the
// reference steps once per bag).  Every per-ROW kernel of the one-bag backward already only knows rows: k_bwd_gh,
// k_tn_split, k_tn_small, k_bwd_reduce's fixed-order sums run over total_rows unchanged, so the contraction over the
// instances sums over the whole batch in one pass.  What is per BAG gets a batched form here:
//   k_bags_rowbag     rowbag[n] = the bag of row n (binary search of the offsets, once per call)
//   k_bags_prep       one workgroup per bag: gB[b], D[b,c] — k_bwd_prep's block 0, bag by bag
//   k_bags_ga         gA[n,:] = V[n,:] gB[bag(n)]^T — k_fc's row product with the row's own weights
//   k_bags_qrow       q_max[b,c] = q(x[offsets[b] + idx[b,c]]): qrow_body, one workgroup per (bag, class)
//   k_bwd_rows<.., BAGS> / k_bwd_rows_hs<BAGS>   the one-bag tile kernels over a 1-D grid of tile SLOTS (slot_owner,
//                     agg_bwd.hip: the real tiles of a ragged batch plus at most one idle slot per bag); a tile never spans
//                     two bags, reads its bag's q_max and D and writes gs, gz2, H, Q, gqp at batch row positions
//   k_bags_critical   one workgroup per bag: critical_body on the bag's own slice — it sums only its bag's gqp tiles and
//                     touches only rows offsets[b] + idx[b,c] of gz2
//   k_bags_head       fixed-order sums over the bags: g_fcc_w, g_fcc_b and the sparse FCLayer term (n_bags * C critical rows)
//   k_bags_gvals      g_vals[n,:] = A[n,:] gB[bag(n)]
//   k_bags_gx         (agg_gx.h) gx_tile with the row's own gB / idx / g_max in the tail
// The kernels that read the rows (k_bags_ga, k_bags_qrow, the tile kernels, k_tn_split, k_tn_small, k_bags_head) take the
// rows' storage type XT as a template parameter and reach them through ONE fetch (load4 and its forms, agg_common.h):
// dsmil_agg_backward_bags_bf16 is the same launch sequence with XT = bf16_t, 2 bytes per element in HBM throughout.
// Launch boundaries order the steps; no atomics, no hand-offs inside a launch, every sum in a fixed order: two runs give the
// same bits, and a batch of ONE bag gives the bits of dsmil_agg_backward_rows (same arithmetic per element, same tile regime).
//
// Tile regime (from total_rows alone, so that it is the one-bag rule at n_bags = 1): total_rows / 128 >= 512 -> the four-wave
// 128-row tile (k_bwd_rows<4,*>, k_bwd_gh<4>); fewer rows -> the hidden-split 64-row tile (k_bwd_rows_hs, k_bwd_gh_hs), or
// the one-wave register-staged tile when the rows are not 16-B aligned (K % 4 != 0).  n_bags only adds idle slots.
//
// Host code: agg_backward_bags_impl is the batched launch sequence, written out in full here.  It takes the call as a
// BwdCall (agg_bwd.hip) plus offsets / n_bags / max_rows, sizes its workspace with bwd_layout(n_bags, ..) — the one-bag
// layout is the same function at n_bags == 0 — and calls the steps that only know rows (launch_gh, launch_tn_split,
// tn_small, reduce_args, gx_args) where the one-bag sequence calls them.  Step 4 stays its own: over slots there is
// no <4,1> form, so unaligned rows in the four-wave regime take the one-wave tile.
//
// dsmil_agg_train_step_bags / dsmil_agg_train_step_bags_bf16 (the end of this file) chain the batched forward, the mean
// objective (k_loss_head_bags_mean) and this backward with Adam applied by its last two launches (k_bwd_reduce's AdamFuse,
// the same hook in k_bags_head): one C call per minibatch step; on bf16 rows k_round_bf16 rebuilds the rounded weight set.
#pragma once

namespace {

// the largest batch dsmil_agg_backward_bags accepts: every grid of the call (tile slots, 4-element groups of g_vals, the
// 128 x 64 tiles of g_feats) then fits 2^31 - 1 workgroups for K, Kv <= 8192, and R, S of k_tn_split stay ints
constexpr long long BAGS_MAX_ROWS = 1LL << 30;

__global__ __launch_bounds__(256) void k_bags_rowbag(const int64_t* __restrict__ offsets, int n_bags, long long T,
                                                     int* __restrict__ rowbag) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= T) return;
    int lo = 0, hi = n_bags;           // invariant: offsets[lo] <= r < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)offsets[mid] <= r) lo = mid; else hi = mid;
    }
    rowbag[r] = lo;
}

// one workgroup per bag: k_bwd_prep's block 0 (the same sums in the same order)
__global__ __launch_bounds__(256) void k_bags_prep(
    const float* __restrict__ fcc_w, const float* __restrict__ Bm, const float* __restrict__ g_pred,
    const float* __restrict__ g_B, const float* __restrict__ A, const float* __restrict__ g_A,
    const int64_t* __restrict__ offsets, float* __restrict__ gB, float* __restrict__ Dv, float* __restrict__ zero128,
    int Kv, int C) {
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const long long off0 = offsets[b], N = offsets[b + 1] - off0;
    const long long bk = (long long)b * C * Kv;
    const float* gp = g_pred + (long long)b * C;
    for (int c = 0; c < C; ++c) {
        float dpart = 0.f;
        for (int k = tid; k < Kv; k += 256) {
            float g = g_B ? g_B[bk + c * Kv + k] : 0.f;
            for (int o = 0; o < C; ++o) g = fmaf(gp[o], fcc_w[((long long)o * C + c) * Kv + k], g);
            gB[bk + c * Kv + k] = g;
            dpart = fmaf(g, Bm[bk + c * Kv + k], dpart);
        }
        if (g_A)
            for (long long n = tid; n < N; n += 256) dpart = fmaf(A[(off0 + n) * C + c], g_A[(off0 + n) * C + c], dpart);
        const float d = block_sum_256(dpart, red);
        if (tid == 0) Dv[(long long)b * C + c] = d;
    }
    if (b == 0 && tid < QD) zero128[tid] = 0.f;
}

// gA[n,c] = <V[n,:], gB[bag(n),c,:]>: agg_fwd.hip k_fc with the row's own weights (b := 0)
template <int VEC, typename XT = float>
__global__ __launch_bounds__(256) void k_bags_ga(const XT* __restrict__ vals, const float* __restrict__ gB,
                                                 const int* __restrict__ rowbag, float* __restrict__ gA, long long N, int Kv,
                                                 int C, const int64_t* __restrict__ rowmap) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long nw = (long long)gridDim.x * 4;
    for (long long r = wid; r < N; r += nw) {
        const XT* x = vals + phys_row(rowmap, r) * Kv;
        const float* w = gB + (long long)rowbag[r] * C * Kv;
        for (int c = 0; c < C; ++c) {
            float acc = 0.f;
            for (int k0 = 0; k0 < Kv; k0 += 256) {
                const int k = k0 + lane * 4;
                const f32x4 xv = load4<VEC, XT>(x, k, Kv);
                const f32x4 wv = load4<VEC>(w + (long long)c * Kv, k, Kv);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = fmaf(xv[e], wv[e], acc);
            }
            acc = wave_sum(acc) + 0.f;
            if (lane == 0) gA[r * C + c] = acc;
        }
    }
}

// one workgroup per (bag, class)
template <int VEC, typename XT = float>
__global__ __launch_bounds__(256) void k_bags_qrow(
    const XT* __restrict__ feats, const int64_t* __restrict__ offsets, const int64_t* __restrict__ idx,
    const float* __restrict__ q0_w, const float* __restrict__ q0_b, const float* __restrict__ q2_w,
    const float* __restrict__ q2_b, float* __restrict__ qmax, int K, int C, int nonlinear, const int64_t* __restrict__ rowmap) {
    const long long bc = blockIdx.x;
    const long long row = (long long)offsets[bc / C] + (long long)idx[bc];
    qrow_body<VEC, XT>(feats + phys_row(rowmap, row) * (long long)K, q0_w, q0_b, q2_w, q2_b, qmax + bc * QD, K, nonlinear);
}

// one workgroup per bag; its slice of gqp starts at the bag's first 32-row tile slot (k_bwd_rows: offsets[b] / 32 + b)
__global__ __launch_bounds__(1024) void k_bags_critical(const int64_t* __restrict__ offsets, const int64_t* __restrict__ idx,
                                                        const float* __restrict__ gqp, const float* __restrict__ Qbuf,
                                                        float* __restrict__ gz2, float* __restrict__ gq, int C, int nonlinear) {
    const int b = blockIdx.x;
    const long long off0 = offsets[b], Nb = offsets[b + 1] - off0;
    critical_body(idx + (long long)b * C, gqp + (off0 / 32 + b) * C * QD, Qbuf + off0 * QD, gz2 + off0 * QD,
                  gq + (long long)b * C * QD, (Nb + 31) / 32, C, nonlinear);
}

// Sums over the bags, bag 0 first (a lone bag: k_bwd_prep's / k_bwd_reduce's values as they are):
//   g_fc_w[c,k] (+)= sum_b g_max[b,c] x[offsets[b] + idx[b,c], k],  g_fc_b[c] (+)= sum_b g_max[b,c]      (g_max != null)
//   g_fcc_w[o,c,k] = sum_b g_pred[b,o] B[b,c,k],                    g_fcc_b[o] = sum_b g_pred[b,o]
struct BagsHeadArgs {
    const void* feats; const int64_t* offsets; const int64_t* idx; const float* g_max; const int64_t* rowmap;   // feats: XT rows
    float* g_fc_w; float* g_fc_b;
    const float* g_pred; const float* Bm; float* g_fcc_w; float* g_fcc_b;
    int n_bags, K, Kv, C, accumulate;
    AdamFuse af;   // dsmil_agg_train_step_bags: the update of fc_w, fc_b, fcc_w, fcc_b (tensors 0, 1, 6, 7) by the thread that sums the element
};
template <typename XT = float>
__global__ __launch_bounds__(256) void k_bags_head(BagsHeadArgs a) {
    const int C = a.C;
    const XT* feats = reinterpret_cast<const XT*>(a.feats);
    const long long nf = a.g_max ? (long long)C * a.K + C : 0, nw = (long long)C * C * a.Kv;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nf) {
        if (i < (long long)C * a.K) {
            const int c = (int)(i / a.K), k = (int)(i - (long long)c * a.K);
            const float v = a.g_max[c] * load1<XT>(feats, phys_row(a.rowmap, a.idx[c]) * (long long)a.K + k);   // bag 0: offsets[0] == 0
            float g = a.accumulate ? a.g_fc_w[i] + v : v;
            for (int b = 1; b < a.n_bags; ++b) {
                const long long row = (long long)a.offsets[b] + (long long)a.idx[(long long)b * C + c];
                g += a.g_max[(long long)b * C + c] * load1<XT>(feats, phys_row(a.rowmap, row) * (long long)a.K + k);
            }
            a.g_fc_w[i] = g;
            if (a.af.on) adam_elem(a.af.p[0] + i, a.af.m[0] + i, a.af.v[0] + i, g, a.af.h);
        } else {
            const int c = (int)(i - (long long)C * a.K);
            float g = a.accumulate ? a.g_fc_b[c] + a.g_max[c] : a.g_max[c];
            for (int b = 1; b < a.n_bags; ++b) g += a.g_max[(long long)b * C + c];
            a.g_fc_b[c] = g;
            if (a.af.on) adam_elem(a.af.p[1] + c, a.af.m[1] + c, a.af.v[1] + c, g, a.af.h);
        }
        return;
    }
    i -= nf;
    if (i < nw) {
        const long long ck = (long long)C * a.Kv;
        const int o = (int)(i / ck);
        const long long e = i - (long long)o * ck;
        float g = a.g_pred[o] * a.Bm[e];
        for (int b = 1; b < a.n_bags; ++b) g += a.g_pred[(long long)b * C + o] * a.Bm[(long long)b * ck + e];
        a.g_fcc_w[i] = g;
        if (a.af.on) adam_elem(a.af.p[6] + i, a.af.m[6] + i, a.af.v[6] + i, g, a.af.h);
        return;
    }
    i -= nw;
    if (i < C) {
        float g = a.g_pred[i];
        for (int b = 1; b < a.n_bags; ++b) g += a.g_pred[(long long)b * C + i];
        a.g_fcc_b[i] = g;
        if (a.af.on) adam_elem(a.af.p[7] + i, a.af.m[7] + i, a.af.v[7] + i, g, a.af.h);
    }
}

// g_vals[n][k] = sum_c A[n][c] gB[bag(n)][c][k]
template <int VEC>
__global__ void k_bags_gvals(const float* __restrict__ A, const float* __restrict__ gB, const int* __restrict__ rowbag,
                             float* __restrict__ gv, long long N, int Kv, int C) {
    const int k4n = (Kv + 3) / 4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * k4n) return;
    const long long n = i / k4n;
    const int k = (int)(i - n * k4n) * 4;
    const float* gb = gB + (long long)rowbag[n] * C * Kv;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) acc += A[n * C + c] * load4<VEC, float>(gb + (long long)c * Kv, k, Kv);
    if constexpr (VEC == 4) {
        *reinterpret_cast<f32x4*>(gv + n * Kv + k) = acc;
    } else {
        for (int e = 0; e < 4; ++e)
            if (k + e < Kv) gv[n * Kv + k + e] = acc[e];
    }
}

// g_feats of a batch: agg_gx.h's tile body with the row's own gB / idx / g_max in the tail
__global__ __launch_bounds__(256, 2) void k_bags_gx(GxArgs a) { gx_tile<false, true>(a); }

// the training objective of every bag of a batch: k_loss_head (agg_fwd.hip), one wave per bag
__global__ __launch_bounds__(64) void k_loss_head_bags(const float* __restrict__ classes, const int64_t* __restrict__ offsets,
                                                       const float* __restrict__ pred, const int64_t* __restrict__ idx,
                                                       const float* __restrict__ label, int C, float* __restrict__ loss,
                                                       float* __restrict__ max_pred, float* __restrict__ g_pred,
                                                       float* __restrict__ g_max, const float* __restrict__ pos_weight,
                                                       const float* __restrict__ weight) {
    const int c = threadIdx.x, b = blockIdx.x;
    const long long bc = (long long)b * C + c;
    const bool weighted = pos_weight || weight;   // class weights (dsmil_agg_loss_head_bags_w), [C] each or null = ones
    float l = 0.f;
    if (c < C) {
        const float y = label[bc];
        const float zb = pred[bc], zm = classes[((long long)offsets[b] + (long long)idx[bc]) * C + c];
        const float pw = pos_weight ? pos_weight[c] : 1.f, w = weight ? weight[c] : 1.f;
        float lb, lm, db, dm;   // BCEWithLogits(z, y) and its derivative in z (bce_logit, agg_common.h)
        bce_logit(weighted, zb, y, pw, w, lb, db);
        bce_logit(weighted, zm, y, pw, w, lm, dm);
        l = 0.5f * (lb + lm) / (float)C;
        if (max_pred) max_pred[bc] = zm;
        if (g_pred) g_pred[bc] = 0.5f * db / (float)C;
        if (g_max) g_max[bc] = 0.5f * dm / (float)C;
    }
    l = wave_sum(l);   // C <= 64: one wave
    if (threadIdx.x == 0) loss[b] = l;
}

// dsmil_agg_train_step_bags: k_loss_head_bags for the MEAN objective of the batch, in one launch of ONE workgroup (its 16
// waves take the bags in turn, so no hand-off between workgroups is needed for the batch loss):
//   loss_each[b]             the bag's own loss                  — k_loss_head_bags' value
//   g_pred, g_max [b,c]      k_loss_head_bags' value times `scale` = 1.0f / n_bags (formed on the host in fp32): the separate
//                            fp32 product MILNet.batch_loss's backward forms (g * (g_loss / n), g_loss = 1), so the batched
//                            backward is handed the same bits by either path.  The value is rounded by the division before
//                            the product and nothing is added behind it: there is nothing to contract.
//   loss[0]                  the mean: the fp32 sum of loss_each in bag order, divided by n_bags (torch.mean may sum in
//                            another order: the two agree to rounding, not to the bit)
__global__ __launch_bounds__(1024) void k_loss_head_bags_mean(const float* __restrict__ classes, const int64_t* __restrict__ offsets,
                                                              const float* __restrict__ pred, const int64_t* __restrict__ idx,
                                                              const float* __restrict__ label, int n_bags, int C, float scale,
                                                              float* __restrict__ loss_each, float* __restrict__ loss,
                                                              float* __restrict__ g_pred, float* __restrict__ g_max,
                                                              const float* __restrict__ pos_weight,
                                                              const float* __restrict__ weight) {
    const int c = threadIdx.x & 63;
    const bool weighted = pos_weight || weight;   // class weights (dsmil_agg_train_step_bags_w), [C] each or null = ones
    const float pw = (pos_weight && c < C) ? pos_weight[c] : 1.f, w = (weight && c < C) ? weight[c] : 1.f;
    for (int b = threadIdx.x >> 6; b < n_bags; b += 16) {
        const long long bc = (long long)b * C + c;
        float l = 0.f;
        if (c < C) {
            const float y = label[bc];
            const float zb = pred[bc], zm = classes[((long long)offsets[b] + (long long)idx[bc]) * C + c];
            float lb, lm, db, dm;   // BCEWithLogits(z, y) and its derivative in z (bce_logit, agg_common.h)
            bce_logit(weighted, zb, y, pw, w, lb, db);
            bce_logit(weighted, zm, y, pw, w, lm, dm);
            l = 0.5f * (lb + lm) / (float)C;
            const float gp = 0.5f * db / (float)C, gm = 0.5f * dm / (float)C;
            g_pred[bc] = gp * scale;
            g_max[bc] = gm * scale;
        }
        l = wave_sum(l);   // C <= 64: one wave
        if (c == 0) loss_each[b] = l;
    }
    __syncthreads();       // the workgroup's own stores to loss_each are out behind the barrier ...
    if (threadIdx.x == 0) {
        const volatile float* le = loss_each;   // ... and read back by vector loads (never through the scalar cache)
        float s = 0.f;
        for (int b = 0; b < n_bags; ++b) s += le[b];
        *loss = s / (float)n_bags;
    }
}

// dsmil_agg_train_step_bags_bf16: the eight parameter tensors rounded to bf16 (round to nearest even) and kept as fp32 —
// what ops._bf16_params holds per weight set, rebuilt here from the fp32 masters at the head of every step
struct RoundTensors { const float* src[8]; float* dst[8]; long long end[8]; };
__global__ __launch_bounds__(256) void k_round_bf16(RoundTensors t) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= t.end[7]) return;
    int k = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j)
        if (i >= t.end[j]) k = j + 1;
    const long long o = i - (k ? t.end[k - 1] : 0);
    t.dst[k][o] = bf2f(f2bf(t.src[k][o]));
}

// The batched launch sequence.  Workspace: bwd_layout(n_bags, total_rows, ..) (agg_bwd.hip).  c.N = total_rows; g_pred,
// g_max, idx are [n_bags, C], B and g_B [n_bags, C, Kv].
// XT = float: dsmil_agg_backward_bags.  XT = bf16_t: dsmil_agg_backward_bags_bf16 — the same launches on the same workspace
// layout with the rows fetched as bf16 (exact MFMA operands: their plane cut is (x, 0, 0)); no row map, no g_feats, and the
// register-staged / hidden-split tiles only (the LDS-DMA tile stages fp32 bytes as they are).
template <typename XT>
int agg_backward_bags_impl(const BwdCall<XT>& c, const int64_t* offsets, int32_t n_bags, int64_t max_rows,
                           const AdamFuse* adam = nullptr) {
    const int64_t T = c.N;
    if (adam && (!c.g_max || c.g_classes || c.g_vals || c.g_feats)) return DSMIL_E_INVALID;   // the fused optimizer step is the training loop's
    if (!offsets || !c.g_pred || n_bags < 1 || T < n_bags || max_rows < 1 || max_rows > T) return DSMIL_E_INVALID;
    int rc = bwd_common_refusal(c);
    if (rc == DSMIL_E_INVALID) return rc;
    const dsmil_agg_params* p = c.p;
    const dsmil_agg_grads* g = c.g;
    const XT* feats = c.feats;
    const XT* vals = c.vals ? c.vals : feats;
    const int64_t* rowmap = c.rowmap;
    if (T > BAGS_MAX_ROWS) return DSMIL_E_UNSUPPORTED;
    constexpr bool B16 = sizeof(XT) == 2;
    if (B16 && (rowmap || c.g_feats)) return DSMIL_E_INVALID;
    if (B16 && (p->K % 8 || p->Kv % 4)) return DSMIL_E_UNSUPPORTED;          // the bf16 forward's condition
    if (B16 && (((uintptr_t)feats | (uintptr_t)vals) % 16)) return DSMIL_E_ALIGN;
    if (rc) return rc;   // the common alignment refusal ranks behind the batch's own limits
    const int K = p->K, Kv = p->Kv, C = p->C;
    const BwdWs L = bwd_layout(n_bags, T, K, Kv, C, p->nonlinear);
    if (c.ws_bytes < L.total) return DSMIL_E_WORKSPACE;
    const long long n4 = (long long)T * ((Kv + 3) / 4);
    if ((n4 + 255) / 256 > 0x7fffffffLL || (long long)C * n_bags > 0x7fffffffLL) return DSMIL_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)c.stream;
    const BwdBufs b = bwd_carve(c.ws, L);
    const bool v4 = (K % 4 == 0) && (((uintptr_t)feats) % 16 == 0);
    const bool w4 = (K % 4 == 0) && (((uintptr_t)feats | (uintptr_t)p->q0_w) % 16 == 0);
    const bool v4v = (Kv % 4 == 0) && ((uintptr_t)vals % 16 == 0);
    // 0. plane-cut weights W1 | W2 and W2^T, the {0, total_rows} offsets; the row -> bag table
    hipLaunchKernelGGL(k_train_prologue, dim3(240), dim3(256), 0, st, p->q0_w, p->nonlinear ? p->q2_w : nullptr, b.wsplit, b.w2t, K,
                       2 * ((K + 31) / 32), b.off, b.off, (long long)T);
    hipLaunchKernelGGL(k_bags_rowbag, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, offsets, n_bags, (long long)T, b.rowbag);
    // 1. heads: gB, D per bag
    hipLaunchKernelGGL(k_bags_prep, dim3((unsigned)n_bags), dim3(256), 0, st, p->fcc_w, c.Bm, c.g_pred, c.g_B, c.A, c.g_A, offsets, b.gB,
                       b.Dv, b.zero, Kv, C);
    if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
    // 2. gA = V gB[bag]^T
    {
        long long blocks = ((long long)T + 3) / 4;
        if (blocks > 4096) blocks = 4096;
        if (v4v) hipLaunchKernelGGL((k_bags_ga<4, XT>), dim3((unsigned)blocks), dim3(256), 0, st, vals, b.gB, b.rowbag, b.gA, (long long)T, Kv, C, rowmap);
        else hipLaunchKernelGGL((k_bags_ga<1, XT>), dim3((unsigned)blocks), dim3(256), 0, st, vals, b.gB, b.rowbag, b.gA, (long long)T, Kv, C, rowmap);
    }
    // 3. critical queries
    if (w4) hipLaunchKernelGGL((k_bags_qrow<4, XT>), dim3((unsigned)(C * n_bags)), dim3(256), 0, st, feats, offsets, c.idx, p->q0_w, p->q0_b, p->q2_w, p->q2_b, b.qmax, K, C, p->nonlinear, rowmap);
    else hipLaunchKernelGGL((k_bags_qrow<1, XT>), dim3((unsigned)(C * n_bags)), dim3(256), 0, st, feats, offsets, c.idx, p->q0_w, p->q0_b, p->q2_w, p->q2_b, b.qmax, K, C, p->nonlinear, rowmap);
    if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
    // 4. per-row part on MFMA, a 1-D grid of tile slots.  Four-wave regime: the LDS-DMA tile over 128-row slots, or the one-wave
    // register-staged tile over 32-row slots on rows that are not 16-B aligned (no <4,1> form over slots)
    const int nw = (T / 128 >= 512) ? 4 : 1;
    BwdRowsArgs br{};
    br.at = AttendArgs{feats, feats, b.wsplit, offsets, p->q0_w, p->q0_b, p->q2_w, p->q2_b, b.qmax, nullptr, nullptr, nullptr,
                       K, K, C, p->nonlinear, 0, 0, rowmap};
    br.A = c.A; br.gA = b.gA; br.g_A = c.g_A; br.Dv = b.Dv; br.gs = b.gs; br.gz2 = b.gz2; br.Hbuf = b.Hb; br.Qbuf = b.Qb; br.gqp = b.gqp;
    br.n_bags = n_bags;
    if (nw == 4 && v4) rc = launch_tile_kernel(k_bwd_rows<4, 4, true, XT>, br, 4, !B16, T, st, T / 128 + n_bags);
    else if (nw == 1 && v4) rc = launch_hs(k_bwd_rows_hs<true, XT>, br, T / HS_BM + n_bags, st);
    else rc = launch_tile_kernel(k_bwd_rows<1, 1, true, XT>, br, 1, false, T, st, T / 32 + n_bags);
    if (rc) return rc;
    // 5. gradient of the critical queries joins their rows, bag by bag
    hipLaunchKernelGGL(k_bags_critical, dim3((unsigned)n_bags), dim3(1024), 0, st, offsets, c.idx, b.gqp, b.Qb, b.gz2, b.gq, C, p->nonlinear);
    if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
    // 6. gH = (gz2 W2) [H > 0] over the rows of the batch
    if (p->nonlinear && (rc = launch_gh(b, T, C, nw, st))) return rc;
    // 7. weight gradients: the contraction over ALL instance rows of the batch, then the fixed-order reduction
    if ((rc = launch_tn_split(feats, rowmap, T, K, p->nonlinear, L, b, v4, nullptr, st))) return rc;
    // 8. dense instance stream
    if (c.g_classes && (rc = tn_small(c.g_classes, feats, T, C, K, b.part, b.part_b, g->fc_w, g->fc_b, L.splits, w4, st, rowmap))) return rc;
    ReduceArgs ra = reduce_args(c, L, b);
    // `adam` (dsmil_agg_train_step_bags): optimizer.step() where the gradient elements are formed, every thread on its own
    // element.  Each parameter tensor's LAST READER is an earlier launch than its updater:
    //   q0_w, q2_w   forward (their cut image), k_train_prologue, k_bags_qrow            -> updated by k_bwd_reduce
    //   q0_b, q2_b   forward, k_bags_qrow, k_bwd_rows / k_bwd_rows_hs (launch 4)          -> updated by k_bwd_reduce
    //                (k_bwd_gh reads the zero bias and W2^T's planes, k_tn_split no parameter at all)
    //   fcc_w        forward (k_finish), k_bags_prep;   fcc_b: forward (k_pred)            -> updated by k_bags_head
    //   fc_w, fc_b   forward (the logits pass)                                            -> updated by k_bags_head
    // k_bags_head itself reads the rows, offsets, idx, g_max, g_pred and B only, and with `adam` no launch follows it.  On
    // bf16 rows every reader above reads the ROUNDED set of the step's workspace; the fp32 masters are read by the step's
    // first launch (k_round_bf16) and written here.
    if (adam) { ra.af = *adam; ra.af.g_fcc_w = nullptr; ra.af.g_fcc_b = nullptr; ra.af.n_fcc_w = 0; ra.af.n_fcc_b = 0; }
    const long long nred = (long long)QD * K + (p->nonlinear ? QD * QD + 2 * QD : QD);
    hipLaunchKernelGGL(k_bwd_reduce, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, st, ra);
    // the sums over the bags: bag head and the sparse FCLayer term
    BagsHeadArgs ha{feats, offsets, c.idx, c.g_max, rowmap, g->fc_w, g->fc_b, c.g_pred, c.Bm, g->fcc_w, g->fcc_b, n_bags, K, Kv, C,
                    c.g_classes ? 1 : 0, AdamFuse{}};
    if (adam) ha.af = *adam;
    const long long nhead = (c.g_max ? (long long)C * K + C : 0) + (long long)C * C * Kv + C;
    hipLaunchKernelGGL(k_bags_head<XT>, dim3((unsigned)((nhead + 255) / 256)), dim3(256), 0, st, ha);
    if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
    // 9. gradient of the value rows
    if (c.g_vals) {
        if (v4v && (uintptr_t)c.g_vals % 16 == 0)
            hipLaunchKernelGGL(k_bags_gvals<4>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, c.A, b.gB, b.rowbag, c.g_vals, (long long)T, Kv, C);
        else
            hipLaunchKernelGGL(k_bags_gvals<1>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, c.A, b.gB, b.rowbag, c.g_vals, (long long)T, Kv, C);
        if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
    }
    // 10. gradient of the input rows
    if (c.g_feats) {
        GxArgs gx = gx_args(c, b);
        gx.rowbag = b.rowbag; gx.offsets = offsets;
        if (!gx_launch<false, true>(gx, st)) return DSMIL_E_UNSUPPORTED;
        if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
    }
    return DSMIL_OK;
}

// ---- dsmil_agg_train_step_bags / _bf16: one optimiser step on a batch of bags per C call ----------------------------
// workspace: the batched forward's, the batched backward's, the step's own tensors, the eight gradient tensors and, for
// bf16 rows, the rounded parameter set with its packed MFMA image
struct BagsStepWs {
    size_t fwd, bwd, classes, A, B, pred, idx, gpred, gmax, grads, rounded, image, total;
    size_t fwd_bytes, bwd_bytes;
};
BagsStepWs step_bags_layout(int n_bags, long long T, int K, int C, int nonlinear, bool b16) {
    BagsStepWs s;
    s.fwd_bytes = dsmil_agg_workspace_bytes(n_bags, T, K, K, C);
    s.bwd_bytes = bwd_layout(n_bags, T, K, K, C, nonlinear).total;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t p = o; o = al(o + bytes); return p; };
    s.fwd = take(s.fwd_bytes);
    s.bwd = take(s.bwd_bytes);
    s.classes = take((size_t)T * C * 4);
    s.A = take((size_t)T * C * 4);
    s.B = take((size_t)n_bags * C * K * 4);
    s.pred = take((size_t)n_bags * C * 4);
    s.idx = take((size_t)n_bags * C * 8);
    s.gpred = take((size_t)n_bags * C * 4);
    s.gmax = take((size_t)n_bags * C * 4);
    const ParamSizes sz = param_sizes(K, C, nonlinear);
    s.grads = o;   // carve_tensors
    for (int i = 0; i < 8; ++i) take((size_t)sz.n[i] * 4);
    s.rounded = o;
    if (b16)
        for (int i = 0; i < 8; ++i) take((size_t)sz.n[i] * 4);
    s.image = take(b16 ? dsmil_agg_packed_bf16_bytes(K) : 0);
    s.total = o;
    return s;
}

// XT = float: dsmil_agg_train_step_bags; XT = bf16_t: dsmil_agg_train_step_bags_bf16.  A fixed launch sequence:
//   bf16 rows only: k_round_bf16 (masters -> rounded set), k_pack_agg_bf16 (its MFMA image; dsmil_agg_pack_bf16)
//   the batched forward (dsmil_agg_forward_ex, which cuts its own weight image / dsmil_agg_forward_bf16)
//   k_loss_head_bags_mean
//   the batched backward (agg_backward_bags_impl: k_train_prologue first) with Adam in its last two launches
// Every check runs here, before the first launch, and covers what the chained calls would refuse.
template <typename XT>
int agg_train_step_bags_impl(const XT* feats, const int64_t* offsets, int32_t n_bags, int64_t T, int64_t max_rows,
                             const int64_t* row_map, const float* labels, const dsmil_agg_params* p,
                             const dsmil_adam_state* opt, float* loss_each, float* loss, void* ws, size_t ws_bytes,
                             const dsmil_bce_weights* bw, void* stream) {
    constexpr bool B16 = sizeof(XT) == 2;
    const float* pos_weight = bw ? bw->pos_weight : nullptr;   // the _w entries' class weights, [C] each or null = ones
    const float* weight = bw ? bw->weight : nullptr;
    // 1. DSMIL_E_INVALID
    if (!feats || !offsets || !labels || !p || !opt || !loss_each || !loss || !ws) return DSMIL_E_INVALID;
    if (n_bags < 1 || T < n_bags || max_rows < 1 || max_rows > T) return DSMIL_E_INVALID;
    if (p->K <= 0 || p->C <= 0 || p->Kv != p->K) return DSMIL_E_INVALID;
    if (!p->fc_w || !p->fc_b || !p->q0_w || !p->q0_b || !p->fcc_w || !p->fcc_b || (p->nonlinear && (!p->q2_w || !p->q2_b)))
        return DSMIL_E_INVALID;
    const int K = p->K, C = p->C;
    const ParamSizes sz = param_sizes(K, C, p->nonlinear);
    AdamFuse af;   // optimizer.step() on the masters (af.p), applied by the backward's last two launches
    if (!adam_fuse(p, sz, opt, af)) return DSMIL_E_INVALID;
    // 2. DSMIL_E_UNSUPPORTED: the limits of the calls the step chains
    if (C > 64 || n_bags > 65535 || T > BAGS_MAX_ROWS) return DSMIL_E_UNSUPPORTED;
    if (B16 && K % 8) return DSMIL_E_UNSUPPORTED;
    if (((long long)T * ((K + 3) / 4) + 255) / 256 > 0x7fffffffLL) return DSMIL_E_UNSUPPORTED;
    // 3. DSMIL_E_ALIGN (the rounded set of the bf16 step lies in the workspace: aligned with it)
    if ((uintptr_t)ws % 256) return DSMIL_E_ALIGN;
    if (((uintptr_t)labels | (uintptr_t)loss_each | (uintptr_t)loss | (uintptr_t)pos_weight | (uintptr_t)weight) % 4 ||
        (uintptr_t)offsets % 8 || (uintptr_t)row_map % 8)
        return DSMIL_E_ALIGN;
    if (B16 ? ((uintptr_t)feats % 16 != 0) : ((uintptr_t)p->q0_b % 16 || (p->nonlinear && (uintptr_t)p->q2_b % 16))) return DSMIL_E_ALIGN;
    // 4. DSMIL_E_WORKSPACE
    const BagsStepWs L = step_bags_layout(n_bags, T, K, C, p->nonlinear, B16);
    if (ws_bytes < L.total) return DSMIL_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* w8 = (char*)ws;
    float* classes = (float*)(w8 + L.classes); float* A = (float*)(w8 + L.A); float* Bm = (float*)(w8 + L.B);
    float* pred = (float*)(w8 + L.pred); int64_t* idx = (int64_t*)(w8 + L.idx);
    float* gpred = (float*)(w8 + L.gpred); float* gmax = (float*)(w8 + L.gmax);
    const StepTensors gr = carve_tensors(w8 + L.grads, sz, p->nonlinear);   // the gradients
    int rc;
    dsmil_agg_params pr = *p;   // what the forward and the backward read: the masters, or (bf16 rows) the rounded set
    if constexpr (B16) {
        // straight-through (dsmil_agg_backward_bags_bf16): forward and backward at the rounded weights, Adam on the masters
        const StepTensors rnd = carve_tensors(w8 + L.rounded, sz, p->nonlinear);   // the rounded set
        RoundTensors rt{};
        long long tot = 0;
        for (int i = 0; i < 8; ++i) { rt.src[i] = af.p[i]; rt.dst[i] = rnd.t[i]; tot += sz.n[i]; rt.end[i] = tot; }
        hipLaunchKernelGGL(k_round_bf16, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, rt);
        if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
        pr.fc_w = rnd.g.fc_w; pr.fc_b = rnd.g.fc_b; pr.q0_w = rnd.g.q0_w; pr.q0_b = rnd.g.q0_b;
        pr.q2_w = rnd.g.q2_w; pr.q2_b = rnd.g.q2_b; pr.fcc_w = rnd.g.fcc_w; pr.fcc_b = rnd.g.fcc_b;
        rc = dsmil_agg_pack_bf16(pr.q0_w, pr.q2_w, K, w8 + L.image, stream);
        if (rc) return rc;
        rc = dsmil_agg_forward_bf16(feats, nullptr, offsets, n_bags, T, max_rows, &pr, w8 + L.image, nullptr, classes, A, Bm, pred,
                                    idx, w8 + L.fwd, L.fwd_bytes, stream);
    } else {
        dsmil_agg_opts fo{};
        fo.row_map = row_map;
        rc = dsmil_agg_forward_ex(feats, nullptr, offsets, n_bags, T, max_rows, &pr, &fo, nullptr, classes, A, Bm, pred, idx,
                                  w8 + L.fwd, L.fwd_bytes, stream);
    }
    if (rc) return rc;
    // objective (train_tcga.py:68-71 per bag, the mean over the bags) and both upstream gradients, scaled for the mean
    hipLaunchKernelGGL(k_loss_head_bags_mean, dim3(1), dim3(1024), 0, st, classes, offsets, pred, idx, labels, (int)n_bags, C,
                       1.0f / (float)n_bags, loss_each, loss, gpred, gmax, pos_weight, weight);
    if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
    // backward + optimizer.step()
    BwdCall<XT> c{};
    c.feats = feats; c.N = T; c.p = &pr; c.A = A; c.Bm = Bm; c.idx = idx; c.g_max = gmax; c.g_pred = gpred; c.g = &gr.g;
    c.rowmap = row_map; c.ws = w8 + L.bwd; c.ws_bytes = L.bwd_bytes; c.stream = stream;
    return agg_backward_bags_impl(c, offsets, n_bags, max_rows, &af);
}

}  // namespace
