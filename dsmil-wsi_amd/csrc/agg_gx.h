// agg_gx.h — the gradient of the INPUT rows of the aggregator and of the value layer.  Included from agg_bwd.hip (k_bwd_gx,
// k_bags_gx) and, through agg_value.h, from agg_value.hip (k_value_gx): the tile body, the arguments and the launcher.
//
//   k_bwd_gx    g_x [N,K] = G W1  (+ g_c Wf) (+ g_max[c] Wf[c] at row idx_c) (+ A gB)       G = gH (gz2 for the linear query)
//   k_value_gx  g_x [N,K] (+)= (g_vals o [V > 0]) Wv                                        dsmil.py:35-39,48
//
// Both are ONE tile body, gx_tile<MASK>: out[rows, cols] = L[rows, J] W[J, cols] with the contraction index j along the
// MFMA k axis, in the form the rest of the backward uses — bf16 MFMA over EXACT three-plane cuts of both fp32 operands,
// the six largest plane products, smallest first (agg_split.h).  Workgroup = 128 rows x 64 columns, four waves
// (column tile w & 1, pair of 32-row tiles w >> 1: two accumulator tiles each), 32 j per step:
//   * L is row-major along j, the MFMA's k axis: a staging thread owns 8 consecutive j of a row (two 16-B loads; four
//     consecutive lanes cover the 128 B a row contributes to a step), applies the ReLU mask (MASK: the forward's V at the
//     same place, as k_value_tn does), cuts the 8 values (split3: each element cut once per column slab) and writes each
//     plane's 16 bytes with one ds_write_b128;
//   * W is NOT transposed for this product (k_tn_split / the forward read W1 along K): here j is W's SLOW axis, so the
//     forward's packed image (fragments along K) does not serve.  W is small (W1: 256 KiB, Wv: 1 MiB) and stays in L2: a
//     staging thread owns one column and 8 consecutive j (8 coalesced dword loads, a wave reads 256 B of a row of W per
//     instruction) and cuts them in place — no second packed image, no extra launch, any K (K % 4 != 0 included: MUSK's
//     166 takes the same kernel), any J (zero-padded to the step);
//   * LDS: [plane][row or column][32 j] bf16 with k_tn_split's row stride of 80 B; a fragment read is one ds_read_b128;
//   * two register sets: the loads of steps s + 1 and s + 2 are in flight while step s multiplies;
//   * epilogue: lane (l31, hi) holds column 32 ct + l31 of 32 rows: a store instruction writes two full 128-B runs.  g_x
//     is written once and never re-read by this library: non-temporal stores.  The 2C-wide tail of k_bwd_gx (g_c Wf and
//     A gB, plus g_max[c] Wf[c] for the workgroup that owns row idx_c) is fp32 FMAs on the accumulators, class by class
//     in a fixed order — the row coefficients are wave-uniform per half-wave (one broadcast load), Wf[c] / gB[c] one
//     coalesced load per class.
// The grid places the column slabs of one row tile on ONE XCD (k_tn_split's trick): its L2 serves the L rows to the
// other slabs.  No atomics, fixed summation order: two runs give the same bits.
#pragma once
#include "agg_split.h"

namespace {

constexpr int GX_LDW = 20;       // 32-bit words per (plane, row) of the staged operands: 16 j pairs + 4 pad
constexpr int GX_BM = 128;       // rows per workgroup
constexpr int GX_BN = 64;        // columns per workgroup

struct GxArgs {
    const float* L;              // [N, J]  gH / gz2 / g_vals (logical row order)
    const float* V;              // [N, J]  MASK: the forward's V; else unused
    const float* W;              // [J, K]  q0_w / v_w
    float* out;                  // [N, K]
    long long N;
    int J, K, ntile, nslab;
    int accumulate;              // out += instead of out =
    int lvec;                    // rows of L (and V) 16-B aligned, J % 4 == 0
    // the tail of k_bwd_gx (C == 0: none)
    const float* gc;             // [N, C] dense instance-logit gradient, or null
    const float* Wf;             // [C, K] (gc or gmax)
    const float* A;              // [N, C] attention, or null (vals are the caller's: passing_v)
    const float* gB;             // [C, K]
    const int64_t* idx;          // [C] critical rows (gmax)
    const float* gmax;           // [C] sparse max-stream gradient, or null
    int C;
    // BAGS (a batch of bags stored back to back, agg_bwd_bags.h): gB [n_bags, C, K], idx / gmax [n_bags, C] (idx bag-local),
    // rowbag[n] = the bag of row n, offsets [n_bags + 1]
    const int* rowbag;
    const int64_t* offsets;
};

template <bool MASK, bool BAGS = false>
__device__ __forceinline__ void gx_tile(const GxArgs& a) {
    __shared__ __attribute__((aligned(16))) unsigned sA[3 * GX_BM * GX_LDW];
    __shared__ __attribute__((aligned(16))) unsigned sB[3 * GX_BN * GX_LDW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int slab = q % a.nslab, tile = xcd + 8 * (q / a.nslab);
    if (tile >= a.ntile) return;
    const long long row0 = (long long)tile * GX_BM;
    const int col0 = slab * GX_BN;
    const int ct = wave & 1, up = wave >> 1;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    auto mfma_phase = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int j = 2 * ks + hi;    // this lane's 8-j group: MFMA k = 8 hi + i  <->  j = 16 ks + 8 hi + i of the step
            S3Frag fb[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) fb[p].f = *reinterpret_cast<const f32x4*>(&sB[(p * GX_BN + 32 * ct + l31) * GX_LDW + 4 * j]);
            S3Frag fa[2][3];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    fa[tt][p].f = *reinterpret_cast<const f32x4*>(&sA[(p * GX_BM + 32 * (2 * up + tt) + l31) * GX_LDW + 4 * j]);
#pragma unroll
            for (int qq = 3; qq < 9; ++qq)               // the six largest plane products, smallest first
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[tt][S3_PA(qq)].v, fb[S3_PB(qq)].v, acc[tt], 0, 0, 0);
        }
    };
    // staging roles.  L: rows ar, ar + 64 of the tile, 8-j group ag; W: column cb of the slab, 8-j group jb
    const int ag = tid & 3, ar = tid >> 2;
    const int cb = tid & 63, jb = tid >> 6;
    long long lrow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long r = row0 + ar + 64 * i;
        lrow[i] = (r < a.N ? r : a.N - 1) * (long long)a.J;   // (a row past the end is cut like the last row and never stored)
    }
    const int bcol = col0 + cb < a.K ? col0 + cb : a.K - 1;   // (a clamped column's products are never stored)
    float ra[2][2][8], rv[2][2][8], rb[2][8];
    auto prefetch = [&](auto setc, int j0) {                   // branch-free: cells past J re-read in-range cells, zeroed when cut
        constexpr int SET = decltype(setc)::value;
        const int ja = j0 + 8 * ag;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (a.lvec) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int jj = ja + 4 * h < a.J ? ja + 4 * h : 0;
                    const f32x4 g = *(const DSMIL_GLOBAL f32x4*)(a.L + lrow[i] + jj);
#pragma unroll
                    for (int e = 0; e < 4; ++e) ra[SET][i][4 * h + e] = g[e];
                    if constexpr (MASK) {
                        const f32x4 v = *(const DSMIL_GLOBAL f32x4*)(a.V + lrow[i] + jj);
#pragma unroll
                        for (int e = 0; e < 4; ++e) rv[SET][i][4 * h + e] = v[e];
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int jj = ja + e < a.J ? ja + e : 0;
                    ra[SET][i][e] = a.L[lrow[i] + jj];
                    if constexpr (MASK) rv[SET][i][e] = a.V[lrow[i] + jj];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = j0 + 8 * jb + e;
            rb[SET][e] = a.W[(long long)(j < a.J ? j : a.J - 1) * a.K + bcol];
        }
    };
    auto step = [&](auto setc, int j0) {
        constexpr int SET = decltype(setc)::value;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float gz[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bool live = j0 + 8 * ag + e < a.J;
                if constexpr (MASK) live = live && rv[SET][i][e] > 0.f;   // ReLU mask (dsmil.py:39)
                gz[e] = live ? ra[SET][i][e] : 0.f;
            }
            S3Frag f[3];
            split3(gz, f);
#pragma unroll
            for (int p = 0; p < 3; ++p)
                *reinterpret_cast<f32x4*>(&sA[(p * GX_BM + ar + 64 * i) * GX_LDW + 4 * ag]) = f[p].f;
        }
        {
            float wv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[e] = j0 + 8 * jb + e < a.J ? rb[SET][e] : 0.f;
            S3Frag f[3];
            split3(wv, f);
#pragma unroll
            for (int p = 0; p < 3; ++p)
                *reinterpret_cast<f32x4*>(&sB[(p * GX_BN + cb) * GX_LDW + 4 * jb]) = f[p].f;
        }
        __syncthreads();
        prefetch(setc, j0 + 64);   // (past J: harmless re-reads)
        mfma_phase();
        __syncthreads();
    };
    prefetch(std::integral_constant<int, 0>{}, 0);
    prefetch(std::integral_constant<int, 1>{}, 32);
    for (int j0 = 0; j0 < a.J; j0 += 64) {
        step(std::integral_constant<int, 0>{}, j0);
        if (j0 + 32 < a.J) step(std::integral_constant<int, 1>{}, j0 + 32);
    }
    // D[m = row][n = column]: lane holds column col0 + 32 ct + l31, rows row0 + 32 (2 up + tt) + (r & 3) + 8 (r >> 2) + 4 hi
    const int col = col0 + 32 * ct + l31;
    if (col >= a.K) return;
    const int mb = 64 * up + 4 * hi;
    if constexpr (BAGS) {
        // the same tail with the row's OWN bag behind every per-bag operand: per element the classes run in the same order
        // with the same two FMAs, so a batch of one bag gives the one-bag kernel's bits
        const bool fcs = a.gc || a.gmax;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
            for (int r = 0; r < 16; ++r) {
                long long row = row0 + mb + 32 * tt + (r & 3) + 8 * (r >> 2);
                row = row < a.N ? row : a.N - 1;
                const long long bc0 = (long long)a.rowbag[row] * a.C;
                const long long lrow = row - (long long)a.offsets[a.rowbag[row]];
                float v = acc[tt][r];
                for (int c = 0; c < a.C; ++c) {
                    if (fcs) {
                        float cf = a.gc ? a.gc[row * a.C + c] : 0.f;
                        if (a.gmax && lrow == (long long)a.idx[bc0 + c]) cf += a.gmax[bc0 + c];
                        v = fmaf(cf, a.Wf[(long long)c * a.K + col], v);
                    }
                    if (a.A) v = fmaf(a.A[row * a.C + c], a.gB[(bc0 + c) * a.K + col], v);
                }
                acc[tt][r] = v;
            }
    } else
    for (int c = 0; c < a.C; ++c) {   // the 2C-wide tail, class by class (fixed order)
        const bool fcs = a.gc || a.gmax;
        const float wf = fcs ? a.Wf[(long long)c * a.K + col] : 0.f;
        const float gb = a.A ? a.gB[(long long)c * a.K + col] : 0.f;
        const long long ic = a.gmax ? (long long)a.idx[c] : -1;
        const float gm = a.gmax ? a.gmax[c] : 0.f;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                long long row = row0 + mb + 32 * tt + (r & 3) + 8 * (r >> 2);
                row = row < a.N ? row : a.N - 1;
                float v = acc[tt][r];
                if (fcs) {
                    float cf = a.gc ? a.gc[row * a.C + c] : 0.f;
                    if (row == ic) cf += gm;
                    v = fmaf(cf, wf, v);
                }
                if (a.A) v = fmaf(a.A[row * a.C + c], gb, v);
                acc[tt][r] = v;
            }
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long row = row0 + mb + 32 * tt + (r & 3) + 8 * (r >> 2);
            if (row < a.N) {
                float* o = a.out + row * (long long)a.K + col;
                float v = acc[tt][r];
                if (a.accumulate) v += *o;
                __builtin_nontemporal_store(v, o);
            }
        }
}

// the three kernels are one-line wrappers of gx_tile, each DEFINED in the one unit that launches it, so that each is emitted
// once: k_bwd_gx in agg_bwd.hip, k_bags_gx in agg_bwd_bags.h, k_value_gx in agg_value.h
__global__ void k_bwd_gx(GxArgs a);
__global__ void k_value_gx(GxArgs a);
__global__ void k_bags_gx(GxArgs a);

// fills the grid fields and launches; returns false when the grid does not fit
template <bool MASK, bool BAGS = false>
inline bool gx_launch(GxArgs a, hipStream_t st) {
    a.ntile = (int)((a.N + GX_BM - 1) / GX_BM);
    a.nslab = (a.K + GX_BN - 1) / GX_BN;
    const long long wgs = (long long)a.nslab * ((a.ntile + 7) / 8 * 8);
    if (wgs > 0x7fffffffLL) return false;
    if constexpr (BAGS) hipLaunchKernelGGL(k_bags_gx, dim3((unsigned)wgs), dim3(256), 0, st, a);
    else if constexpr (MASK) hipLaunchKernelGGL(k_value_gx, dim3((unsigned)wgs), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_bwd_gx, dim3((unsigned)wgs), dim3(256), 0, st, a);
    return true;
}

}  // namespace
