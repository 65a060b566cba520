// agg_value.h — the value stream of BClassifier(passing_v=True), dsmil.py:35-39,48:  V = ReLU(x Wv^T + bv)  and its
// gradients.  Included from agg_value.hip alone, the unit that holds the layer's entries: the forward's k_pack_value,
// k_value_proj, k_value_proj_valu and, for bf16-stored rows, k_pack_value_b16, k_value_proj_b16, k_value_proj_b16_valu
// (described above them); the parameter gradients' k_value_tn, k_value_reduce and, for bf16-stored rows, k_value_tn_b16
// (described above it); the input-row gradient's k_value_gx, a wrapper of agg_gx.h's tile body.
//
// Forward, k_value_proj.  A GEMM with Kv output columns per row on v_mfma_f32_32x32x16_f16 in the arithmetic of agg_f2.h:
// x' = x * 2^e per ROW, Wv' = Wv * 2^f per TENSOR (f2_scale), both cut into two fp16 planes (split2h_scaled / the pack
// kernel), products h0 w0 + h0 w1 + h1 w0 accumulated in fp32, un-scaled, bias and ReLU on the accumulators.
//   * a workgroup (four waves) owns a tile of 32 RG rows (RG = 2 while the planes of the tile fit: K <= 512; RG = 1 up to
//     K = 1024) and produces ALL Kv columns of it: x is read once;
//   * staging: every thread owns (row, k-octet) cells.  It loads its cells as fp32 into the LDS slots its planes will take
//     (8 fp32 = 32 B = the 16 B of plane 0 + the 16 B of plane 1), keeps the running max |x|, the lanes of a row meet with
//     shuffles, and the thread then cuts ITS OWN cells in place: the row maximum comes from the staged tile itself (no
//     logits pass in front), the raw tile needs no registers, and nobody reads another thread's raw cell (one barrier);
//   * plane image in LDS: [16-k step][plane][hi][row] x 16 B — an A-fragment read is one ds_read_b128 over 32 consecutive
//     16-B cells (conflict-free), RG x 2 reads per 12 RG MFMAs;
//   * wave w owns column groups w, w + 4, ... of 128 columns (four 32 x 32 accumulator tiles per row group: 64 RG
//     accumulator registers).  The weight planes come from the packed image (L2; 1 MiB at K = Kv = 512) as B fragments, two
//     register sets, each refilled for step s + 2 behind the MFMAs of step s;
//   * epilogue: lane (l31, hi) holds column 32 tile + l31 of rows 8q + 4hi + e: a store instruction writes two 128-B runs.
// K is zero-padded to a multiple of 32 in the staged tile and in the pack, Kv to a multiple of 128 columns in the pack.
// K > 1024 takes k_value_proj_valu (plain fp32 FMAs).
//
// Backward, k_value_tn: g_Wv = gZ^T x, g_bv = colsum gZ with gZ = g_vals * (V > 0) formed while the operand is staged.
// The contraction runs over the instance rows, so a per-row power-of-two scale cannot be taken out of the sum: the fp16
// two-plane form would need per-COLUMN maxima of both operands (one more pass over them).  It therefore uses k_tn_split's
// form: bf16 MFMA over exact three-plane cuts (bf16 has fp32's exponent range: no scale), six plane products.  Sibling of
// k_tn_split's scalar staging branch with Kv / 128 unit slabs: workgroup = (64-column slab of x, 128-unit slab of gZ, row
// range); per-range partials are summed in a fixed order by k_value_reduce (two runs: the same bits).
#pragma once
#include "agg_f2.h"
#include "agg_split.h"
#include "agg_gx.h"

namespace {

constexpr int VP_THREADS = 256;
constexpr int VP_TRAILER_BYTES = 256;                 // behind the chunks: {1 / scale(Wv)}
constexpr int VP_MAX_K = 1024;                        // widest K of the MFMA kernel (128 KiB of planes at 32 rows)

__host__ __device__ inline int vp_nks(int K) { return 2 * ((K + 31) / 32); }             // 16-k steps (K padded to 32)
__host__ __device__ inline int vp_ntp(int Kv) { return ((Kv + 31) / 32 + 3) / 4 * 4; }   // 32-column tiles (padded to groups of four)
inline size_t vp_image_bytes(int K, int Kv) { return (size_t)vp_nks(K) * vp_ntp(Kv) * 2 * 64 * 16 + VP_TRAILER_BYTES; }
inline size_t vp_al(size_t n) { return (n + 255) / 256 * 256; }

// row ranges of the backward: R rows each (a multiple of 64), S of them; ~384 workgroups per launch as k_tn_split
inline void vtn_plan(long long rows, int K, int Kv, int& S, int& R) {
    const long long nslab = (long long)((K + 63) / 64) * ((Kv + 127) / 128);
    long long s = 384 / nslab;
    s = s < 1 ? 1 : s;
    long long r = (rows + s - 1) / s;
    r = (r + 63) / 64 * 64;
    R = (int)r;
    S = (int)((rows + r - 1) / r);
}
// the backward's workspace: the row-range partials behind `image_bytes` of weight image (fp32: the forward's image, which a
// caller may cut there, vp_image_bytes; bf16-stored rows: 0, the partials start the workspace)
struct VpWs { size_t part, pb, total; };
inline VpWs vp_ws_layout(long long rows, int K, int Kv, size_t image_bytes) {
    VpWs L;
    int S, R;
    vtn_plan(rows, K, Kv, S, R);
    L.part = vp_al(image_bytes);
    L.pb = L.part + vp_al((size_t)S * Kv * K * 4);
    L.total = L.pb + vp_al((size_t)S * Kv * 4);
    return L;
}

// fp32 Wv [Kv, K] -> two fp16 planes of a Wv (a = f2_scale(max |Wv|)), B-fragment order:
//   [step s][tile t][plane p][lane (l31, hi)][e] = plane_p(a Wv[32 t + l31][16 s + 8 hi + e])   (0 past Kv / K)
//   trailer: {1 / a}
__global__ __launch_bounds__(256) void k_pack_value(const float* __restrict__ v_w, _Float16* __restrict__ out, int K, int Kv,
                                                    int nks, int ntp) {
    __shared__ float s_m[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m = 0.f;
    for (long long i = tid; i < (long long)Kv * K; i += 256) m = fmaxf(m, fabsf(v_w[i]));
    m = wave_max(m);
    if (lane == 0) s_m[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    float inv;
    const float a = f2_scale(m, inv);
    const long long total = (long long)nks * ntp * 1024;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)gridDim.x * 256) {
        const int e = (int)(i & 7), ln = (int)((i >> 3) & 63), p = (int)((i >> 9) & 1);
        const long long st = i >> 10;
        const int t = (int)(st % ntp), s = (int)(st / ntp);
        const int j = 32 * t + (ln & 31), k = 16 * s + 8 * (ln >> 5) + e;
        const float v = (j < Kv && k < K) ? v_w[(long long)j * K + k] * a : 0.f;
        const _Float16 h = (_Float16)v;
        out[i] = p == 0 ? h : (_Float16)(v - (float)h);
    }
    if (blockIdx.x == 0 && tid == 0) *reinterpret_cast<float*>(out + total) = inv;
}

// 8 consecutive values of a row from column k (zero past K); VEC: 16-B aligned rows, K % 4 == 0
__device__ __forceinline__ void vp_load8(const float* __restrict__ row, int k, int K, bool vec, f32x4& a, f32x4& b) {
    if (vec) {
        const int ka = k + 4 <= K ? k : 0, kb = k + 8 <= K ? k + 4 : 0;   // (branch-free: a cell past K re-reads the row's start)
        a = *(const DSMIL_GLOBAL f32x4*)(row + ka);
        b = *(const DSMIL_GLOBAL f32x4*)(row + kb);
        if (k + 4 > K) a = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k + 8 > K) b = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[e] = k + e < K ? row[k + e] : 0.f;
            b[e] = k + 4 + e < K ? row[k + 4 + e] : 0.f;
        }
    }
}

// grid = tiles of 32 RG rows; FULL: K % 32 == 0 and 16-B aligned rows (no padding, no bounds in the staging loads); NKS = the number of 16-k steps when it is a compile-time constant (straight-line MFMA loop:
// the compiler's wait counts are exact there), 0 = the run-time value
template <int RG, int NKS, bool FULL>
__global__ __launch_bounds__(VP_THREADS, 1) void k_value_proj(const float* __restrict__ x, const int64_t* __restrict__ rowmap,
                                                              const f32x4* __restrict__ wimg, const float* __restrict__ bias,
                                                              float* __restrict__ V, long long rows, int K, int Kv, int vec) {
    constexpr int BM = 32 * RG;
    constexpr int RPW = BM / 4;                          // rows a wave stages: 16 / 8
    constexpr int OPW = 64 / RPW;                        // k-octets per wave-wide load: 4 / 8
    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4* sXp = reinterpret_cast<f32x4*>(smem);        // [step][plane 2][hi 2][BM] x 16 B
    const int nks = NKS ? NKS : vp_nks(K);
    const int ntp = vp_ntp(Kv);
    float* sInv = reinterpret_cast<float*>(sXp + (long long)nks * 4 * BM);   // [BM]: 1 / row scale
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const long long row0 = (long long)blockIdx.x * BM;
    // ---- stage: raw fp32 cells into their plane slots, row maxima, cut in place
    {
        const int rr = lane % RPW, o = lane / RPW;
        const int row = RPW * wave + rr;
        long long gr = row0 + row;
        if (gr >= rows) gr = rows - 1;                   // rows past the end are cut like the last row and never stored
        const float* src = x + phys_row(rowmap, gr) * (long long)K;
        const int noct = 2 * nks;
        float m = 0.f;
        if constexpr (FULL) {
            // K % 32 == 0, 16-B aligned rows: unconditional 16-B loads, eight cells in flight per thread (a cell index past the
            // tile's last is clamped: the same cell is written twice with the same values)
            const int nit = (noct + OPW - 1) / OPW;
#pragma unroll 8
            for (int it = 0; it < nit; ++it) {
                int ko = it * OPW + o;
                ko = ko < noct ? ko : noct - 1;
                const f32x4 a = *(const DSMIL_GLOBAL f32x4*)(src + 8 * ko);
                const f32x4 b = *(const DSMIL_GLOBAL f32x4*)(src + 8 * ko + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(a[e]), fabsf(b[e])));
                f32x4* dst = sXp + (long long)((ko >> 1) * 4 + (ko & 1)) * BM + row;
                dst[0] = a;
                dst[2 * BM] = b;
            }
        } else {
            for (int ko = o; ko < noct; ko += OPW) {
                f32x4 a, b;
                vp_load8(src, 8 * ko, K, vec != 0, a, b);
#pragma unroll
                for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(a[e]), fabsf(b[e])));
                f32x4* dst = sXp + (long long)((ko >> 1) * 4 + (ko & 1)) * BM + row;
                dst[0] = a;
                dst[2 * BM] = b;
            }
        }
#pragma unroll
        for (int d = RPW; d < 64; d <<= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
        float inv;
        const float sc = f2_scale(m, inv);
        if (o == 0) sInv[row] = inv;
        for (int ko = o; ko < noct; ko += OPW) {
            f32x4* dst = sXp + (long long)((ko >> 1) * 4 + (ko & 1)) * BM + row;
            const f32x4 a = dst[0], b = dst[2 * BM];
            F2Frag f[2];
            split2h_scaled(a, b, sc, f);
            dst[0] = f[0].f;
            dst[2 * BM] = f[1].f;
        }
    }
    __syncthreads();
    // ---- all Kv columns of the tile: wave w takes the 128-column groups w, w + 4, ...
    const float iw = *reinterpret_cast<const float*>(wimg + (long long)nks * ntp * 128);
    const long long sstride = (long long)ntp * 128;      // 16-B units per step of the image
    for (int g = wave; g < ntp / 4; g += 4) {
        f32x16 acc[RG][4];
#pragma unroll
        for (int rg = 0; rg < RG; ++rg)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[rg][t][r] = 0.f;
        const f32x4* wp = wimg + (long long)g * 512 + lane;
        F2Frag wr[2][4][2];
        auto load_w = [&](auto slot_, int s) {
            constexpr int SL = decltype(slot_)::value;
            const int sw = s < nks ? s : nks - 1;        // (past the last step: a harmless re-read, no branch)
            const f32x4* p = wp + (long long)sw * sstride;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                wr[SL][t][0].f = *(const DSMIL_GLOBAL f32x4*)(p + (2 * t) * 64);
                wr[SL][t][1].f = *(const DSMIL_GLOBAL f32x4*)(p + (2 * t + 1) * 64);
            }
        };
        auto step = [&](auto slot_, int s) {
            constexpr int SL = decltype(slot_)::value;
            F2Frag xa[RG][2];
            const f32x4* p = sXp + (long long)(s * 4 + hi) * BM + l31;
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) {
                xa[rg][0].f = p[32 * rg];
                xa[rg][1].f = p[2 * BM + 32 * rg];
            }
            // smallest products first; the accumulators of a step in turn
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rg = 0; rg < RG; ++rg)
                    acc[rg][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[rg][1].v, wr[SL][t][0].v, acc[rg][t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rg = 0; rg < RG; ++rg)
                    acc[rg][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[rg][0].v, wr[SL][t][1].v, acc[rg][t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rg = 0; rg < RG; ++rg)
                    acc[rg][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[rg][0].v, wr[SL][t][0].v, acc[rg][t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            load_w(slot_, s + 2);
            __builtin_amdgcn_sched_barrier(0);
        };
        constexpr int UNR = NKS ? NKS / 2 : 1;
        load_w(std::integral_constant<int, 0>{}, 0);
        load_w(std::integral_constant<int, 1>{}, 1);
#pragma unroll UNR
        for (int s = 0; s < nks; s += 2) {               // (nks is even)
            step(std::integral_constant<int, 0>{}, s);
            step(std::integral_constant<int, 1>{}, s + 1);
        }
        // ---- un-scale, bias, ReLU, store: reg 4q + e <-> row 32 rg + 8q + 4 hi + e, column 32 (4g + t) + l31
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = 32 * (4 * g + t) + l31;
            const bool jok = j < Kv;
            const float bj = jok ? bias[j] : 0.f;
#pragma unroll
            for (int rg = 0; rg < RG; ++rg)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * rg + 8 * (r >> 2) + 4 * hi + (r & 3);
                    const long long gr = row0 + row;
                    const float v = fmaf(acc[rg][t][r], sInv[row] * iw, bj);
                    if (jok && gr < rows) V[gr * (long long)Kv + j] = v < 0.f ? 0.f : v;   // (a NaN stays a NaN, as torch's ReLU)
                }
        }
    }
}

// any other width (K > VP_MAX_K): one thread per output, fp32 FMAs in k order
__global__ __launch_bounds__(256) void k_value_proj_valu(const float* __restrict__ x, const int64_t* __restrict__ rowmap,
                                                         const float* __restrict__ v_w, const float* __restrict__ bias,
                                                         float* __restrict__ V, long long rows, int K, int Kv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * Kv) return;
    const long long n = i / Kv;
    const int j = (int)(i - n * Kv);
    const float* xr = x + phys_row(rowmap, n) * (long long)K;
    const float* wr = v_w + (long long)j * K;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf(xr[k], wr[k], s);
    s += bias[j];
    V[i] = s < 0.f ? 0.f : s;
}
// ---- bf16-stored rows: k_pack_value_b16, k_value_proj_b16, k_value_proj_b16_valu ------------------------------------------
// V = bf16_rne(max(0, x w_b^T + v_b)) for bf16 rows x and w_b = bf16_rne(Wv): both are exact MFMA operands, so ONE
// v_mfma_f32_32x32x16_bf16 product per MAC replaces the three plane products above — no cut, no scale, fp32 accumulation.
//   * a workgroup (four waves) owns a tile of 64 rows and produces ALL Kv columns of it: x is read once;
//   * the tile lives in LDS as the bf16 it is stored as, [k-octet][row] x 16 B (octet o = k / 8: step o >> 1, half o & 1):
//     2 K bytes per row, half the fp32 kernel's plane image.  K <= 512: 64 KiB, so TWO workgroups share a compute unit and
//     one stages its tile while the other multiplies (the fp32 kernel has one); K <= 1024: 128 KiB, 64 rows where the fp32
//     kernel holds 32;
//   * staging: a wave-wide load takes 8 rows x 128 B (lane = (row & 7, octet & 7): whole 128-B lines), the 8 lanes of a
//     ds_write_b128 group write 8 consecutive cells (conflict-free); no transform, no second pass;
//   * A-fragment read: one ds_read_b128 over 32 consecutive cells per lane half (conflict-free), 2 reads per 8 MFMAs;
//   * wave w owns column groups w, w + 4, ... of 128 columns (four 32 x 32 accumulator tiles per 32 rows: 128 accumulator
//     registers).  The weights come from the packed image (L2; 512 KiB at K = Kv = 512) as B fragments, two register sets,
//     each refilled for step s + 2 behind the MFMAs of step s;
//   * epilogue: bias and ReLU on the accumulators; the lane halves exchange the tiles of a pair (v_permlane32_swap: lanes
//     0..31 then hold tile 2u, lanes 32..63 tile 2u + 1, each for all 32 rows), neighbouring lanes exchange one value (DPP)
//     so that a lane holds two adjacent columns of one row: a 4-byte store instruction writes two rows in 128-B runs.
// Every output's sum runs over the k steps 0, 1, ... in turn whatever its row's place in the call: its bits depend on K alone.
// K is zero-padded to a multiple of 32 in the staged tile and in the pack, Kv to a multiple of 128 columns in the pack.
// K % 8 == 0 and Kv % 4 == 0 (16-B cells, 4-B stores: dsmil_agg_forward_bf16's own condition); K > 1024 takes
// k_value_proj_b16_valu.
constexpr int VB_BM = 64;                             // rows per tile
constexpr int VB_MAX_K = 1024;                        // widest K of the MFMA kernel (128 KiB tile)
inline size_t vb_image_bytes(int K, int Kv) { return (size_t)vp_nks(K) * vp_ntp(Kv) * 64 * 16; }

// fp32 Wv [Kv, K] -> bf16 (round to nearest even), B-fragment order:
//   [step s][tile t][lane (l31, hi)][e] = bf16(Wv[32 t + l31][16 s + 8 hi + e])   (0 past Kv / K)
__global__ __launch_bounds__(256) void k_pack_value_b16(const float* __restrict__ v_w, bf16_t* __restrict__ out, int K, int Kv,
                                                        int nks, int ntp) {
    const long long total = (long long)nks * ntp * 512;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int e = (int)(i & 7), ln = (int)((i >> 3) & 63);
        const long long st = i >> 9;
        const int t = (int)(st % ntp), s = (int)(st / ntp);
        const int j = 32 * t + (ln & 31), k = 16 * s + 8 * (ln >> 5) + e;
        out[i] = (j < Kv && k < K) ? f2bf(v_w[(long long)j * K + k]) : (bf16_t)0;
    }
}

__device__ __forceinline__ float vb_xor1(float v) {   // the value of lane ^ 1 (DPP quad_perm [1, 0, 3, 2])
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
}

// grid = tiles of 64 rows; FULL: K % 64 == 0 (every staging load is a real cell); NKS = the number of 16-k steps when it is a
// compile-time constant (straight-line MFMA loop), 0 = the run-time value
template <int NKS, bool FULL>
__global__ __launch_bounds__(VP_THREADS, 2) void k_value_proj_b16(const bf16_t* __restrict__ x, const f32x4* __restrict__ wimg,
                                                                  const float* __restrict__ bias, bf16_t* __restrict__ V,
                                                                  long long rows, int K, int Kv) {
    constexpr int BM = VB_BM;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4* sX = reinterpret_cast<f32x4*>(smem);          // [k-octet][BM] x 16 B
    const int nks = NKS ? NKS : vp_nks(K);
    const int ntp = vp_ntp(Kv);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const long long row0 = (long long)blockIdx.x * BM;
    // ---- stage: wave w brings rows 16 w .. 16 w + 15, eight rows x eight octets per load instruction
    {
        const int rr = lane & 7, o = lane >> 3;
        const int noct = 2 * nks, kreal = K >> 3;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int row = 16 * wave + 8 * rb + rr;
            long long gr = row0 + row;
            if (gr >= rows) gr = rows - 1;               // rows past the end repeat the last row and are never stored
            const bf16_t* src = x + gr * (long long)K;
            if constexpr (FULL) {
#pragma unroll 8
                for (int ko = o; ko < noct; ko += 8) sX[ko * BM + row] = *(const DSMIL_GLOBAL f32x4*)(src + 8 * ko);
            } else {
                for (int ko = o; ko < noct; ko += 8) {
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (ko < kreal) v = *(const DSMIL_GLOBAL f32x4*)(src + 8 * ko);
                    sX[ko * BM + row] = v;
                }
            }
        }
    }
    __syncthreads();
    // ---- all Kv columns of the tile: wave w takes the 128-column groups w, w + 4, ...
    union Frag { f32x4 f; bf16x8 v; };
    const long long sstride = (long long)ntp * 64;       // 16-B units per step of the image
    for (int g = wave; g < ntp / 4; g += 4) {
        f32x16 acc[2][4];
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[rg][t][r] = 0.f;
        const f32x4* wp = wimg + (long long)g * 256 + lane;
        Frag wr[2][4];
        auto load_w = [&](auto slot_, int s) {
            constexpr int SL = decltype(slot_)::value;
            const int sw = s < nks ? s : nks - 1;        // (past the last step: a harmless re-read, no branch)
            const f32x4* p = wp + (long long)sw * sstride;
#pragma unroll
            for (int t = 0; t < 4; ++t) wr[SL][t].f = *(const DSMIL_GLOBAL f32x4*)(p + t * 64);
        };
        auto step = [&](auto slot_, int s) {
            constexpr int SL = decltype(slot_)::value;
            Frag xa[2];
            const f32x4* p = sX + (s * 2 + hi) * BM + l31;
            xa[0].f = p[0];
            xa[1].f = p[32];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rg = 0; rg < 2; ++rg)
                    acc[rg][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[rg].v, wr[SL][t].v, acc[rg][t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            load_w(slot_, s + 2);
            __builtin_amdgcn_sched_barrier(0);
        };
        constexpr int UNR = NKS ? NKS / 2 : 1;
        load_w(std::integral_constant<int, 0>{}, 0);
        load_w(std::integral_constant<int, 1>{}, 1);
#pragma unroll UNR
        for (int s = 0; s < nks; s += 2) {               // (nks is even)
            step(std::integral_constant<int, 0>{}, s);
            step(std::integral_constant<int, 1>{}, s + 1);
        }
        // ---- bias, ReLU, round, store.  reg 4q + e of tile t <-> row 32 rg + 8q + 4 hi + e, column 32 (4g + t) + l31
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j0 = 32 * (4 * g + 2 * u) + l31, j1 = j0 + 32;
            const float b0 = j0 < Kv ? bias[j0] : 0.f, b1 = j1 < Kv ? bias[j1] : 0.f;
            const int j = hi ? j1 : j0;                  // this lane's column after the half exchange
            const bool jok = (j & ~1) < Kv;              // (Kv % 4 == 0: the pair j & ~1, (j & ~1) + 1 is inside or outside together)
#pragma unroll
            for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float a = acc[rg][2 * u][r] + b0, b = acc[rg][2 * u + 1][r] + b1;
                    a = a < 0.f ? 0.f : a;               // (a NaN stays a NaN, as torch's ReLU)
                    b = b < 0.f ? 0.f : b;
                    // lanes 0..31 keep a (tile 2u, rows 8q + e) and take the upper half's a (tile 2u, rows 8q + 4 + e); lanes
                    // 32..63 take the lower half's b (tile 2u + 1, rows 8q + e) and keep b (tile 2u + 1, rows 8q + 4 + e)
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
                    const float lo = __uint_as_float(sw[0]), up = __uint_as_float(sw[1]);   // rows 8q + e / 8q + 4 + e of column j
                    // an even lane keeps row 8q + e and takes its neighbour's, an odd lane keeps row 8q + 4 + e
                    const bool odd = lane & 1;
                    const float got = vb_xor1(odd ? lo : up);
                    const unsigned w2 = odd ? pack_bf16x2_hw(got, up) : pack_bf16x2_hw(lo, got);
                    const int row = 32 * rg + 8 * (r >> 2) + (odd ? 4 : 0) + (r & 3);
                    const long long gr = row0 + row;
                    if (jok && gr < rows) *reinterpret_cast<unsigned*>(V + gr * (long long)Kv + (j & ~1)) = w2;
                }
        }
    }
}

// any other width (K > VB_MAX_K): one thread per output, fp32 FMAs of the exact bf16 products in k order
__global__ __launch_bounds__(256) void k_value_proj_b16_valu(const bf16_t* __restrict__ x, const float* __restrict__ v_w,
                                                             const float* __restrict__ bias, bf16_t* __restrict__ V,
                                                             long long rows, int K, int Kv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * Kv) return;
    const long long n = i / Kv;
    const int j = (int)(i - n * Kv);
    const bf16_t* xr = x + n * (long long)K;
    const float* wr = v_w + (long long)j * K;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf(bf2f(xr[k]), bf2f(f2bf(wr[k])), s);
    s += bias[j];
    V[i] = f2bf(s < 0.f ? 0.f : s);
}

constexpr int VTN_LDW = 20;      // 32-bit words per (plane, column) row of the staged operands: 16 row pairs + 4 pad (k_tn_split's)
struct VtnArgs {
    const float* G;              // g_vals [N, Kv]   (logical row order)
    const float* V;              // the forward's V [N, Kv]
    const float* X;              // feats [*, K]
    const int64_t* rowmap;       // logical -> physical rows of X, or null
    float* part;                 // [S][Kv][K]
    float* pb;                   // [S][Kv]
    long long N;
    int K, Kv, R, nsk, nsu, S;
};

// workgroup = (column slab cs of 64 columns of x, unit slab us of 128 columns of gZ, row range).  Staging: A thread = unit
// u0 + (tid & 127), 8-row groups (tid >> 7), (tid >> 7) + 2; B thread = column col0 + (tid & 63), 8-row group tid >> 6; the
// ReLU mask is applied to the A values as they are cut.  Two register sets: the loads of steps s + 1 and s + 2 are in flight
// while step s multiplies.  Wave w = (column tile w & 1, unit-tile pair w >> 1).
__global__ __launch_bounds__(256, 2) void k_value_tn(VtnArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned sA[3 * 128 * VTN_LDW];
    __shared__ __attribute__((aligned(16))) unsigned sB[3 * 64 * VTN_LDW];
    __shared__ float s_cs[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int cs = (int)(blockIdx.x % a.nsk);
    const int q = (int)(blockIdx.x / a.nsk);
    const int us = q % a.nsu, split = q / a.nsu;
    const int u0 = us * 128, col0 = cs * 64;
    const long long rbeg = (long long)split * a.R, rend = (rbeg + a.R < a.N) ? rbeg + a.R : a.N;
    const bool want_cs = cs == 0;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int ct = wave & 1, up = wave >> 1;
    auto mfma_phase = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int j = 2 * ks + hi;    // this lane's 8-row group: MFMA k = 8 hi + i  <->  row 16 ks + 8 hi + i
            S3Frag fb[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) fb[p].f = *reinterpret_cast<const f32x4*>(&sB[(p * 64 + 32 * ct + l31) * VTN_LDW + 4 * j]);
            S3Frag fa[2][3];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    fa[tt][p].f = *reinterpret_cast<const f32x4*>(&sA[(p * 128 + 32 * (2 * up + tt) + l31) * VTN_LDW + 4 * j]);
#pragma unroll
            for (int qq = 3; qq < 9; ++qq)               // the six largest plane products, smallest first
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[tt][S3_PA(qq)].v, fb[S3_PB(qq)].v, acc[tt], 0, 0, 0);
        }
    };
    const int u = tid & 127, ja = tid >> 7;
    const int cb = tid & 63, jb = tid >> 6;
    const bool u_ok = u0 + u < a.Kv;
    const int ucol = u_ok ? u0 + u : a.Kv - 1;             // (a clamped unit's values are zeroed when they are cut)
    const int bcol = col0 + cb < a.K ? col0 + cb : a.K - 1;  // (a clamped column's products are never stored)
    float ra[2][2][8], rv[2][2][8], rb[2][8];
    auto prefetch = [&](auto setc, long long r0) {          // branch-free: rows past the range re-read its last row
        constexpr int SET = decltype(setc)::value;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                long long r = r0 + 8 * (ja + 2 * i) + e;
                r = r < rend ? r : rend - 1;
                ra[SET][i][e] = a.G[r * a.Kv + ucol];
                rv[SET][i][e] = a.V[r * a.Kv + ucol];
            }
        long long pr[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long long r = r0 + 8 * jb + e;
            pr[e] = r < rend ? r : rend - 1;
        }
        if (a.rowmap) {
#pragma unroll
            for (int e = 0; e < 8; ++e) pr[e] = (long long)a.rowmap[pr[e]];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) rb[SET][e] = a.X[pr[e] * (long long)a.K + bcol];
    };
    float colsum = 0.f;
    auto step = [&](auto setc, long long r0) {
        constexpr int SET = decltype(setc)::value;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float gz[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool live = u_ok && r0 + 8 * (ja + 2 * i) + e < rend && rv[SET][i][e] > 0.f;   // ReLU mask (dsmil.py:39)
                gz[e] = live ? ra[SET][i][e] : 0.f;
            }
            S3Frag f[3];
            split3(gz, f);
#pragma unroll
            for (int p = 0; p < 3; ++p)
                *reinterpret_cast<f32x4*>(&sA[(p * 128 + u) * VTN_LDW + 4 * (ja + 2 * i)]) = f[p].f;
            if (want_cs) {
#pragma unroll
                for (int e = 0; e < 8; ++e) colsum += gz[e];
            }
        }
        {
            S3Frag f[3];
            split3(rb[SET], f);
#pragma unroll
            for (int p = 0; p < 3; ++p)
                *reinterpret_cast<f32x4*>(&sB[(p * 64 + cb) * VTN_LDW + 4 * jb]) = f[p].f;
        }
        __syncthreads();
        prefetch(setc, r0 + 64);
        mfma_phase();
        __syncthreads();
    };
    prefetch(std::integral_constant<int, 0>{}, rbeg);
    prefetch(std::integral_constant<int, 1>{}, rbeg + 32);
    for (long long r0 = rbeg; r0 < rend; r0 += 64) {
        step(std::integral_constant<int, 0>{}, r0);
        if (r0 + 32 < rend) step(std::integral_constant<int, 1>{}, r0 + 32);
    }
    // D[m = unit][n = column]: lane holds column col0 + 32 ct + l31, units u0 + 32 (2 up + tt) + (r & 3) + 8 (r >> 2) + 4 hi
    const int col = col0 + 32 * ct + l31;
    if (col < a.K) {
        float* o = a.part + (long long)split * a.Kv * a.K;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = u0 + 32 * (2 * up + tt) + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (m < a.Kv) o[(long long)m * a.K + col] = acc[tt][r];
            }
    }
    if (want_cs) {
        s_cs[tid] = colsum;
        __syncthreads();
        if (tid < 128 && u0 + tid < a.Kv) a.pb[(long long)split * a.Kv + u0 + tid] = s_cs[tid] + s_cs[tid + 128];
    }
}

// ---- bf16-stored rows: k_value_tn_b16 ---------------------------------------------------------------------------------------
// The same contraction on the operands of the bf16 path: x [rows, K] and V [rows, Kv] raw bf16, g_vals [rows, Kv] fp32 (the
// bf16 aggregator backward's, unrounded).  A bf16 row is ONE exact bf16 MFMA operand, so x is staged as one plane — no zero
// planes in LDS, no MFMA on them: the three exact planes of gZ times that plane, THREE products per 16-deep step and
// accumulator, all kept (the fp32 kernel issues six of nine); sB is a third of k_value_tn's.  Tile geometry, row ranges
// (vtn_plan), partial layout and k_value_reduce are k_value_tn's.  K % 8 == 0, Kv % 4 == 0.
// Staging is k_tn_split's wide form: a thread owns FOUR columns and 8 consecutive rows, one load per row — 8 bytes of x or V
// (load4_bits), 16 bytes of g_vals — and the LDS holds the columns permuted (unit u0 + 4g + c at position 32c + g, column
// col0 + 4g + c at position 16c + g) so that consecutive lanes write consecutive positions; the epilogue undoes it.  Waves 0, 1
// stage A (gZ = V > 0 ? g : 0 as a select on the bf16 value: +0, -0 and a NaN V mask, a NaN / inf g at a masked position gives
// 0; cut into three planes), wave 2 stages B (x repacked, never widened: 8 rows of a column = 4 words), wave 3 only
// multiplies.  Each role takes its own straight-line loop, steps come in pairs and four pairs are unrolled (R is a multiple of
// 64; the A rows past a range are zero): see k_tn_split for why the wait-count pass needs that shape.
struct VtnB16Args {
    const float* G;              // g_vals [N, Kv]
    const bf16_t* V;             // the forward's V [N, Kv]
    const bf16_t* X;             // feats [N, K]
    float* part;                 // [S][Kv][K]
    float* pb;                   // [S][Kv]
    long long N;
    int K, Kv, R, nsk, nsu, S;
};

__global__ __launch_bounds__(256, 2) void k_value_tn_b16(VtnB16Args a) {
    __shared__ __attribute__((aligned(16))) unsigned sA[3 * 128 * VTN_LDW];
    __shared__ __attribute__((aligned(16))) unsigned sB[64 * VTN_LDW];
    __shared__ float s_cs[512];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cs = (int)(blockIdx.x % a.nsk);
    const int q = (int)(blockIdx.x / a.nsk);
    const int us = q % a.nsu, split = q / a.nsu;
    const int u0 = us * 128, col0 = cs * 64;
    const long long rbeg = (long long)split * a.R, rend = (rbeg + a.R < a.N) ? rbeg + a.R : a.N;
    const bool want_cs = cs == 0;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int ct = wave & 1, up = wave >> 1;
    auto mfma_phase = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int j = 2 * ks + hi;    // this lane's 8-row group: MFMA k = 8 hi + i  <->  row 16 ks + 8 hi + i
            S3Frag fb;
            fb.f = *reinterpret_cast<const f32x4*>(&sB[(32 * ct + l31) * VTN_LDW + 4 * j]);
            S3Frag fa[2][3];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    fa[tt][p].f = *reinterpret_cast<const f32x4*>(&sA[(p * 128 + 32 * (2 * up + tt) + l31) * VTN_LDW + 4 * j]);
#pragma unroll
            for (int p = 2; p >= 0; --p)                 // all three plane products, smallest first; the accumulators in turn
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[tt][p].v, fb.v, acc[tt], 0, 0, 0);
        }
    };
    float cs4[4] = {0.f, 0.f, 0.f, 0.f};
    int csg = 0, csj = 0;                                // the A role's (column group, 8-row group), for the bias sum
    auto stage_loop = [&](auto rolec) {
        constexpr bool RA = decltype(rolec)::value;
        const int g = RA ? (tid & 31) : (tid & 15), jg = RA ? (tid >> 5) : ((tid >> 4) & 3);
        const int ld = RA ? a.Kv : a.K;
        int c4 = (RA ? u0 : col0) + 4 * g;
        const bool c_ok = c4 < ld;                       // (K, Kv % 4 == 0: a group of four is inside or outside together)
        c4 = c_ok ? c4 : ld - 4;                         // a clamped unit's values are zeroed, a clamped column's never stored
        const bf16_t* p16 = (RA ? a.V : a.X) + c4;
        const float* pg = a.G + c4;
        csg = g; csj = jg;
        u32x2 vb[2][8];
        f32x4 vg[2][RA ? 8 : 1];
        auto prefetch = [&](auto setc, long long r0) {   // branch-free: rows past the range re-read its last row
            constexpr int SET = decltype(setc)::value;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                long long r = r0 + 8 * jg + e;
                r = r < rend ? r : rend - 1;
                vb[SET][e] = load4_bits(p16, r * ld);
                if constexpr (RA) vg[SET][e] = *(const DSMIL_GLOBAL f32x4*)(pg + r * ld);
            }
        };
        auto step = [&](auto setc, long long r0) {
            constexpr int SET = decltype(setc)::value;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if constexpr (RA) {
                    float gz[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bool live = c_ok && r0 + 8 * jg + e < rend && bf16x4_at(vb[SET][e], c) > 0.f;   // ReLU mask (dsmil.py:39)
                        gz[e] = live ? vg[SET][e][c] : 0.f;
                    }
                    if (want_cs) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) cs4[c] += gz[e];
                    }
                    S3Frag f[3];
                    split3(gz, f);
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        *reinterpret_cast<f32x4*>(&sA[(p * 128 + 32 * c + g) * VTN_LDW + 4 * jg]) = f[p].f;
                } else {
                    S3Frag f;                            // rows 2i, 2i + 1 of column c: the halves 16 (c & 1) of word c >> 1
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned w1 = c < 2 ? vb[SET][2 * i + 1].x : vb[SET][2 * i + 1].y;
                        const unsigned w0 = c < 2 ? vb[SET][2 * i].x : vb[SET][2 * i].y;
                        f.u[i] = __builtin_amdgcn_perm(w1, w0, (c & 1) ? 0x07060302u : 0x05040100u);
                    }
                    *reinterpret_cast<f32x4*>(&sB[(16 * c + g) * VTN_LDW + 4 * jg]) = f.f;
                }
            }
            __syncthreads();
            prefetch(setc, r0 + 64);
            mfma_phase();
            __syncthreads();
        };
        prefetch(std::integral_constant<int, 0>{}, rbeg);
        prefetch(std::integral_constant<int, 1>{}, rbeg + 32);
        for (long long r0 = rbeg; r0 < rend; r0 += 256) {   // four pairs straight-line, forward exits only
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                if (r0 + 64 * h >= rend) break;
                step(std::integral_constant<int, 0>{}, r0 + 64 * h);
                step(std::integral_constant<int, 1>{}, r0 + 64 * h + 32);
            }
        }
    };
    if (wave < 2) {
        stage_loop(std::true_type{});
    } else if (wave == 2) {
        stage_loop(std::false_type{});
    } else {
        for (long long r0 = rbeg; r0 < rend; r0 += 64) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                __syncthreads();
                mfma_phase();
                __syncthreads();
            }
        }
    }
    // D[m position][n position]: position -> unit u0 + 4 (m & 31) + (m >> 5), column col0 + 4 (n & 15) + (n >> 4)
    const int npos = 32 * ct + l31, col = col0 + 4 * (npos & 15) + (npos >> 4);
    if (col < a.K) {
        float* o = a.part + (long long)split * a.Kv * a.K;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mp = 32 * (2 * up + tt) + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const int m = u0 + 4 * (mp & 31) + (mp >> 5);
                if (m < a.Kv) o[(long long)m * a.K + col] = acc[tt][r];
            }
    }
    if (want_cs) {
        if (wave < 2) {
#pragma unroll
            for (int c = 0; c < 4; ++c) s_cs[csj * 128 + 4 * csg + c] = cs4[c];
        }
        __syncthreads();
        if (tid < 128 && u0 + tid < a.Kv)
            a.pb[(long long)split * a.Kv + u0 + tid] = (s_cs[tid] + s_cs[128 + tid]) + (s_cs[256 + tid] + s_cs[384 + tid]);
    }
}

// fixed-order sums over the row ranges: g_Wv [Kv, K] and g_bv [Kv]
__global__ __launch_bounds__(256) void k_value_reduce(const float* __restrict__ part, const float* __restrict__ pb,
                                                      float* __restrict__ g_w, float* __restrict__ g_b, int K, int Kv, int S) {
    const long long nw = (long long)Kv * K;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nw) {
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += part[(long long)k * nw + i];
        g_w[i] = s;
    } else if (i < nw + Kv) {
        const int j = (int)(i - nw);
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += pb[(long long)k * Kv + j];
        g_b[j] = s;
    }
}

// the gradient of the layer's input rows, g_x (+)= (g_vals o [V > 0]) Wv: agg_gx.h's tile body with the ReLU mask
__global__ __launch_bounds__(256, 2) void k_value_gx(GxArgs a) { gx_tile<true>(a); }

}  // namespace
