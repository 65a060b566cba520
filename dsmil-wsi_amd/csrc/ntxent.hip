// ntxent.hip — NT-Xent (SimCLR) loss, forward and backward, flash-style: the 2N x 2N similarity matrix is formed tile by tile
// on v_mfma_f32_16x16x32_f16 and never stored.  Replaces simclr/loss/nt_xent.py:47-65 of the reference (and its autograd).
//
// With R = cat([zjs, zis]), M = 2N, p(a) = (a + N) mod M and S = R^ R^T (cosine: R^ = R / max(|R|, 1e-8)) or R R^T (dot):
//     loss    = (1/M) sum_a [ logsumexp_{b != a}(S_ab / T) - S_{a,p(a)} / T ]
//     dR^     = (P + P^T - 2 Pi) R^ / (M T),   P_ab = exp(S_ab / T - lse_a), P_aa = 0, Pi the permutation matrix of p
//     dR_a    = (dR^_a - R^_a (R^_a . dR^_a)) / |R_a|                                            (cosine only)
//
// Operands (the library's fp32-class MFMA form, agg_f2.h): x' = R^ 2^e, h0 = rne16(x'), h1 = rne16(x' - h0); three plane
// products per MAC, smallest first: h1 h0, h0 h1, h0 h0 (PlaneProducts<3>).  Cosine: e = 13 (unit rows: |x'| <= 2^13); dot: ONE
// e per call, from the tensor's maximum (max |x'| in [2^13, 2^14)).  D is padded with zeros to the 32-k MFMA step, the rows to
// the 64-row tile.  k_nx_cut writes the planes twice: [row][plane][k] for the S tile (k = feature) and [plane][k][row] for
// the backward's second GEMM (k = row).
//
// Tile: 256 threads own 64 rows a and walk 64-column tiles b of their column split.  Wave w holds S^T of ITS 16 rows:
// the MFMA's A operand is the column tile (four 16-row blocks from LDS, staged in 128-k chunks), its B operand the wave's own
// rows (registers for D <= 256, else re-read from L2), so lane (l15, g) ends with S[a = l15][b = 16 bb + 4 g + e] — one row a
// per lane: the running (max, sum) of the forward needs no exchange per tile, and the same registers, cut into two fp16
// planes of 2^12 W, ARE the A fragments of the backward's second GEMM W R^ (it sums over b, the accumulator's row index;
// the k slots of a 32-k step are then b = 4 g + j and 16 + 4 g + j - 4, and the B fragments are read from the transposed
// planes in that order).  No floating-point atomics: per-(row, split) partials, combined in split order by k_nx_finish /
// k_nx_bwd_fin, so results are bit-identical from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsmil_hip.h"
#include "lds_attr.h"

namespace {

typedef _Float16 nx_f16;
typedef __attribute__((ext_vector_type(8))) _Float16 nx_f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 nx_f16x4;
typedef __attribute__((ext_vector_type(4))) float nx_f32x4;

constexpr int NX_BM = 64;                        // rows a per workgroup = columns b per tile
constexpr int NX_THREADS = 256;
constexpr int NX_KC = 128;                       // k of one staged chunk of the column tile
constexpr int NX_SROW = 2 * NX_KC * 2 + 16;      // bytes per row of the chunk: two planes + 16 pad (ds_read_b128 conflict-free)
constexpr int NX_SBYTES = NX_BM * NX_SROW;
constexpr int NX_NB = 256;                       // features per workgroup of the backward (16 accumulator blocks per wave)
constexpr int NX_TROW = 2 * NX_BM + 16;          // bytes per feature row of the transposed tile (ds_read_b64 conflict-free)
constexpr int NX_TBYTES = 2 * NX_NB * NX_TROW;
constexpr int NX_WSHIFT = 12;                    // W in [-2, 2] is cut as 2^12 W
constexpr int NX_MAX_SPLIT = 8;
constexpr float NX_NEG = -3.0e38f;               // "no column yet" (finite: differences stay NaN-free)
constexpr float NX_LOG2E = 1.44269504088896341f;

__device__ __forceinline__ float nx_exp(float x) { return __builtin_amdgcn_exp2f(x * NX_LOG2E); }

struct NxPlan {
    int M, Mpad, Dpad;
    int nsf, tpf;          // forward: column splits, tiles per split
    int nsb, tpb, nfc;     // backward: column splits, tiles per split, feature chunks
    size_t planes, tplanes, inv, rowmax, sc, pm, pl, pos, part, total;
};

void nx_split(int nct, int want, int& ns, int& tps) {
    want = want < 1 ? 1 : (want > NX_MAX_SPLIT ? NX_MAX_SPLIT : want);
    if (want > nct) want = nct;
    tps = (nct + want - 1) / want;
    ns = (nct + tps - 1) / tps;      // no empty split
}

NxPlan nx_plan(int64_t n, int d) {
    NxPlan P{};
    P.M = (int)(2 * n);
    P.Mpad = (P.M + NX_BM - 1) / NX_BM * NX_BM;
    P.Dpad = (d + 31) / 32 * 32;
    const int rb = P.Mpad / NX_BM;
    P.nfc = (P.Dpad + NX_NB - 1) / NX_NB;
    nx_split(rb, (512 + rb - 1) / rb, P.nsf, P.tpf);
    nx_split(rb, (256 + rb * P.nfc - 1) / (rb * P.nfc), P.nsb, P.tpb);
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    const size_t md = (size_t)P.Mpad * P.Dpad;
    P.planes = o;  o = al(o + md * 4);
    P.tplanes = o; o = al(o + md * 4);
    P.inv = o;     o = al(o + (size_t)P.Mpad * 4);
    P.rowmax = o;  o = al(o + (size_t)P.Mpad * 4);
    P.sc = o;      o = al(o + 16);
    P.pm = o;      o = al(o + (size_t)NX_MAX_SPLIT * P.Mpad * 4);
    P.pl = o;      o = al(o + (size_t)NX_MAX_SPLIT * P.Mpad * 4);
    P.pos = o;     o = al(o + (size_t)P.Mpad * 4);
    P.part = o;    o = al(o + (size_t)P.nsb * md * 4);
    P.total = o;
    return P;
}

__device__ __forceinline__ const float* nx_row(const float* zis, const float* zjs, int a, int N, int D) {
    return a < N ? zjs + (size_t)a * D : zis + (size_t)(a - N) * D;      // R = cat([zjs, zis]) (nt_xent.py:48)
}

// ---- prep 1: 1 / max(|R_a|, 1e-8) (cosine; 1 in dot mode) and max_k |R^_ak| per row.  One wave per row.
__global__ __launch_bounds__(NX_THREADS) void k_nx_rowstat(const float* __restrict__ zis, const float* __restrict__ zjs, int N,
                                                           int D, int cosine, float* __restrict__ inv,
                                                           float* __restrict__ rowmax) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= 2 * N) {                       // the padding rows of the last tile
        if (lane == 0) { inv[a] = 0.f; rowmax[a] = 0.f; }
        return;
    }
    const float* src = nx_row(zis, zjs, a, N, D);
    float ss = 0.f, mx = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float x = src[k];
        ss = fmaf(x, x, ss);
        mx = fmaxf(mx, fabsf(x));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ss += __shfl_xor(ss, off);
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    const float iv = cosine ? 1.0f / fmaxf(sqrtf(ss), 1e-8f) : 1.0f;
    if (lane == 0) { inv[a] = iv; rowmax[a] = mx * iv; }
}

// ---- prep 2: the operand scale 2^e -> sc[0], 2^-e -> sc[1].  One workgroup.
__global__ __launch_bounds__(1024) void k_nx_scale(const float* __restrict__ rowmax, int M, int cosine, float* __restrict__ sc) {
    __shared__ float red[1024];
    const int tid = threadIdx.x;
    float mx = 0.f;
    if (!cosine)
        for (int i = tid; i < M; i += 1024) mx = fmaxf(mx, rowmax[i]);
    red[tid] = mx;
    __syncthreads();
    for (int s = 512; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        int e = 13;
        if (!cosine) {
            int x = 0;
            frexpf(red[0], &x);                                   // max = f 2^x, f in [0.5, 1)
            e = red[0] > 0.f ? 14 - x : 0;
            e = e < -60 ? -60 : (e > 60 ? 60 : e);
        }
        sc[0] = ldexpf(1.0f, e);
        sc[1] = ldexpf(1.0f, -e);
    }
}

// ---- prep 3: the two fp16 planes of R^ 2^e, row-major and transposed.  Workgroup = 64 rows x 64 features.
__global__ __launch_bounds__(NX_THREADS) void k_nx_cut(const float* __restrict__ zis, const float* __restrict__ zjs, int N, int D,
                                                       int Mpad, int Dpad, const float* __restrict__ inv,
                                                       const float* __restrict__ sc, nx_f16* __restrict__ planes,
                                                       nx_f16* __restrict__ tplanes) {
    __shared__ __attribute__((aligned(16))) nx_f16 t[2][64][72];
    const int tid = threadIdx.x, a0 = blockIdx.x * 64, k0 = blockIdx.y * 64, M = 2 * N;
    {
        const int r = tid >> 2, ks = (tid & 3) * 16, a = a0 + r;
        const float f = a < M ? inv[a] * sc[0] : 0.f;             // a power of two times inv: exact
        const float* src = a < M ? nx_row(zis, zjs, a, N, D) : zis;
        nx_f16 h0[16], h1[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = k0 + ks + j;
            const float x = (a < M && k < D) ? src[k] : 0.f;
            const float tt = x * f;
            h0[j] = (nx_f16)tt;
            h1[j] = (nx_f16)(tt - (float)h0[j]);
            t[0][ks + j][r] = h0[j];
            t[1][ks + j][r] = h1[j];
        }
        if (k0 + ks < Dpad) {                                     // Dpad % 32 == 0: a 16-group lies inside or outside
            nx_f16* d0 = planes + ((size_t)a * 2) * Dpad + k0 + ks;
            nx_f16* d1 = d0 + Dpad;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                nx_f16x8 v0, v1;
#pragma unroll
                for (int j = 0; j < 8; ++j) { v0[j] = h0[8 * h + j]; v1[j] = h1[8 * h + j]; }
                *(nx_f16x8*)(d0 + 8 * h) = v0;
                *(nx_f16x8*)(d1 + 8 * h) = v1;
            }
        }
    }
    __syncthreads();
    {
        const int kk = tid >> 2, rs = (tid & 3) * 16, k = k0 + kk;
        if (k < Dpad) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                nx_f16* d = tplanes + ((size_t)p * Dpad + k) * Mpad + a0 + rs;
                *(nx_f16x8*)d = *(const nx_f16x8*)&t[p][kk][rs];
                *(nx_f16x8*)(d + 8) = *(const nx_f16x8*)&t[p][kk][rs + 8];
            }
        }
    }
}

// ---- the S tile: acc[bb][e] = 2^2e S[a = arow][b = c0 + 16 bb + 4 g + e].  RES: the wave's own fragments are in afr.
__device__ __forceinline__ void nx_stage_chunk(const nx_f16* __restrict__ planes, int Dpad, int c0, int kc0, int kcw, char* lds,
                                               int tid) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = tid + NX_THREADS * j, row = i >> 5, p = (i >> 4) & 1, piece = i & 15;
        if (piece * 8 < kcw)
            *(uint4*)(lds + row * NX_SROW + p * (NX_KC * 2) + piece * 16) =
                *(const uint4*)(planes + ((size_t)(c0 + row) * 2 + p) * Dpad + kc0 + piece * 8);
    }
}

__device__ __forceinline__ void nx_step(const char* lds, int ks, int l15, int g, const nx_f16x8& b0, const nx_f16x8& b1,
                                        nx_f32x4 (&acc)[4]) {
    nx_f16x8 a0[4], a1[4];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
        const char* p = lds + (16 * bb + l15) * NX_SROW + ks * 64 + g * 16;
        a0[bb] = *(const nx_f16x8*)p;
        a1[bb] = *(const nx_f16x8*)(p + NX_KC * 2);
    }
    // smallest products first (PlaneProducts<3>); the four accumulators alternate inside each product
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) acc[bb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[bb], b0, acc[bb], 0, 0, 0);
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) acc[bb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[bb], b1, acc[bb], 0, 0, 0);
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) acc[bb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[bb], b0, acc[bb], 0, 0, 0);
}

template <bool RES>
__device__ __forceinline__ void nx_s_tile(const nx_f16* __restrict__ planes, int Dpad, size_t arow, int c0, char* lds,
                                          const nx_f16x8 (&afr)[2][8], nx_f32x4 (&acc)[4], int tid, int l15, int g) {
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) acc[bb] = nx_f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (RES) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c * NX_KC < Dpad) {                               // uniform over the workgroup
                const int kcw = min(NX_KC, Dpad - c * NX_KC);
                __syncthreads();                                  // the chunk's previous readers are done
                nx_stage_chunk(planes, Dpad, c0, c * NX_KC, kcw, lds, tid);
                __syncthreads();
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    if (ks * 32 < kcw) nx_step(lds, ks, l15, g, afr[0][c * 4 + ks], afr[1][c * 4 + ks], acc);
            }
        }
    } else {
        const nx_f16* ap = planes + arow * 2 * Dpad + g * 8;
        for (int kc0 = 0; kc0 < Dpad; kc0 += NX_KC) {
            const int kcw = min(NX_KC, Dpad - kc0);
            __syncthreads();
            nx_stage_chunk(planes, Dpad, c0, kc0, kcw, lds, tid);
            __syncthreads();
            for (int ks = 0; ks < kcw / 32; ++ks) {
                const nx_f16x8 b0 = *(const nx_f16x8*)(ap + kc0 + ks * 32);
                const nx_f16x8 b1 = *(const nx_f16x8*)(ap + Dpad + kc0 + ks * 32);
                nx_step(lds, ks, l15, g, b0, b1, acc);
            }
        }
    }
}

template <bool RES>
__device__ __forceinline__ void nx_load_own(const nx_f16* __restrict__ planes, int Dpad, size_t arow, int g,
                                            nx_f16x8 (&afr)[2][8]) {
    if constexpr (RES) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (s * 32 < Dpad) {
                afr[0][s] = *(const nx_f16x8*)(planes + arow * 2 * Dpad + s * 32 + g * 8);
                afr[1][s] = *(const nx_f16x8*)(planes + arow * 2 * Dpad + Dpad + s * 32 + g * 8);
            } else {
                afr[0][s] = nx_f16x8{};
                afr[1][s] = nx_f16x8{};
            }
        }
    }
}

// ---- forward: per (row, split) the running maximum and sum of exp of the logits, and the positive's logit.
template <bool RES>
__global__ __launch_bounds__(NX_THREADS) void k_nx_fwd(const nx_f16* __restrict__ planes, const float* __restrict__ sc, int N,
                                                       int Mpad, int Dpad, float inv_t, int tiles_per_split,
                                                       float* __restrict__ pm, float* __restrict__ pl,
                                                       float* __restrict__ pos) {
    __shared__ __attribute__((aligned(16))) char lds[NX_SBYTES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int M = 2 * N, a = blockIdx.x * NX_BM + 16 * w + l15, pa = a < N ? a + N : a - N;
    const int nct = Mpad / NX_BM, t0 = blockIdx.y * tiles_per_split, t1 = min(nct, t0 + tiles_per_split);
    const float isc = sc[1], cz = sc[1] * inv_t;
    nx_f16x8 afr[2][8];
    nx_load_own<RES>(planes, Dpad, (size_t)a, g, afr);
    float m = NX_NEG, l = 0.f;
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * NX_BM;
        nx_f32x4 acc[4];
        nx_s_tile<RES>(planes, Dpad, (size_t)a, c0, lds, afr, acc, tid, l15, g);
        float v[16], tmax = NX_NEG;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int b = c0 + 16 * (i >> 2) + 4 * g + (i & 3);
            v[i] = (acc[i >> 2][i & 3] * isc) * cz;
            if (b == pa && a < M) pos[a] = v[i];                  // exactly one lane of the grid per row
            if (!(b < M && b != a)) v[i] = NX_NEG;
            tmax = fmaxf(tmax, v[i]);
        }
        if (tmax > NX_NEG) {
            const float mn = fmaxf(m, tmax);
            l *= nx_exp(m - mn);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (v[i] > NX_NEG) l += nx_exp(v[i] - mn);
            m = mn;
        }
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {                    // the four lanes of a row
        const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off), mn = fmaxf(m, m2);
        l = l * nx_exp(m - mn) + l2 * nx_exp(m2 - mn);            // (lane g = 0 keeps the result)
        m = mn;
    }
    if (g == 0 && a < M) {
        pm[(size_t)blockIdx.y * Mpad + a] = m;
        pl[(size_t)blockIdx.y * Mpad + a] = l;
    }
}

// ---- forward finish: lse[a] from the splits in order, loss = (1/M) sum_a (lse_a - positive_a).  One workgroup.
__global__ __launch_bounds__(1024) void k_nx_finish(const float* __restrict__ pm, const float* __restrict__ pl,
                                                    const float* __restrict__ pos, int M, int Mpad, int ns,
                                                    float* __restrict__ lse, float* __restrict__ loss) {
    __shared__ float red[1024];
    const int tid = threadIdx.x;
    float sum = 0.f;
    for (int a = tid; a < M; a += 1024) {
        float m = NX_NEG;
        for (int s = 0; s < ns; ++s) m = fmaxf(m, pm[(size_t)s * Mpad + a]);
        float l = 0.f;
        for (int s = 0; s < ns; ++s) l += pl[(size_t)s * Mpad + a] * nx_exp(pm[(size_t)s * Mpad + a] - m);
        const float z = m + logf(l);
        lse[a] = z;
        sum += z - pos[a];
    }
    red[tid] = sum;
    __syncthreads();
    for (int s = 512; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) loss[0] = red[0] / (float)M;
}

// ---- backward: part[split][a][n] = 2^(12 + e) sum_{b in split} W_ab R^_bn for the workgroup's 64 rows and 256 features.
template <bool RES>
__global__ __launch_bounds__(NX_THREADS) void k_nx_bwd(const nx_f16* __restrict__ planes, const nx_f16* __restrict__ tplanes,
                                                       const float* __restrict__ sc, const float* __restrict__ lse, int N,
                                                       int Mpad, int Dpad, float inv_t, int tiles_per_split,
                                                       float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lds[];    // chunk of the column tile | transposed tile
    char* tl = lds + NX_SBYTES;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int M = 2 * N, a = blockIdx.x * NX_BM + 16 * w + l15, pa = a < N ? a + N : a - N;
    const int nct = Mpad / NX_BM, t0 = blockIdx.y * tiles_per_split, t1 = min(nct, t0 + tiles_per_split);
    const int n0 = blockIdx.z * NX_NB, nfe = min(NX_NB, Dpad - n0), nnb = nfe / 16;
    const float isc = sc[1], cz = sc[1] * inv_t;
    const float lse_a = a < M ? lse[a] : 0.f;
    nx_f16x8 afr[2][8];
    nx_load_own<RES>(planes, Dpad, (size_t)a, g, afr);
    nx_f32x4 out[16];
#pragma unroll
    for (int nb = 0; nb < 16; ++nb) out[nb] = nx_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * NX_BM;
        nx_f32x4 acc[4];
        nx_s_tile<RES>(planes, Dpad, (size_t)a, c0, lds, afr, acc, tid, l15, g);   // (its barriers also release tl)
        // the transposed tile: [plane][feature][64 b]
        for (int i = tid; i < 2 * nfe * 8; i += NX_THREADS) {
            const int p = i / (nfe * 8), rem = i - p * (nfe * 8), n = rem >> 3, piece = rem & 7;
            *(uint4*)(tl + (p * NX_NB + n) * NX_TROW + piece * 16) =
                *(const uint4*)(tplanes + ((size_t)p * Dpad + n0 + n) * Mpad + c0 + piece * 8);
        }
        // W, cut into two fp16 planes: this lane's 16 values are its A fragments (k slot 8 g + j of step s: b = 32 s + 4 g + j,
        // j < 4, and 32 s + 16 + 4 g + j - 4)
        nx_f16x8 w0[2], w1[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int bb = i >> 2, e = i & 3, b = c0 + 16 * bb + 4 * g + e;
            const float v = (acc[bb][e] * isc) * cz;
            float wv = 0.f;
            if (b < M && a < M && b != a) {
                const float lse_b = lse[b];
                wv = nx_exp(v - lse_a) + nx_exp(v - lse_b) - (b == pa ? 2.0f : 0.0f);
            }
            const float ws = wv * (float)(1 << NX_WSHIFT);
            const nx_f16 h0 = (nx_f16)ws, h1 = (nx_f16)(ws - (float)h0);
            w0[bb >> 1][4 * (bb & 1) + e] = h0;
            w1[bb >> 1][4 * (bb & 1) + e] = h1;
        }
        __syncthreads();
#pragma unroll
        for (int nb = 0; nb < 16; ++nb) {
            if (nb < nnb) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const char* q = tl + (16 * nb + l15) * NX_TROW + (32 * s + 4 * g) * 2;
                    nx_f16x8 r0, r1;
                    const nx_f16x4 r0a = *(const nx_f16x4*)q, r0b = *(const nx_f16x4*)(q + 32);
                    const nx_f16x4 r1a = *(const nx_f16x4*)(q + NX_NB * NX_TROW), r1b = *(const nx_f16x4*)(q + NX_NB * NX_TROW + 32);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { r0[j] = r0a[j]; r0[4 + j] = r0b[j]; r1[j] = r1a[j]; r1[4 + j] = r1b[j]; }
                    out[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[s], r0, out[nb], 0, 0, 0);
                    out[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0[s], r1, out[nb], 0, 0, 0);
                    out[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0[s], r0, out[nb], 0, 0, 0);
                }
            }
        }
    }
    // D[row 4 g + e][col l15]: row = the wave's a, col = the feature
#pragma unroll
    for (int nb = 0; nb < 16; ++nb) {
        if (nb < nnb) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ar = blockIdx.x * NX_BM + 16 * w + 4 * g + e;
                part[((size_t)blockIdx.y * Mpad + ar) * Dpad + n0 + 16 * nb + l15] = out[nb][e];
            }
        }
    }
}

// ---- backward finish: the splits in order, the factors, the cosine projection, the two output tensors.  One wave per row.
__global__ __launch_bounds__(NX_THREADS) void k_nx_bwd_fin(const float* __restrict__ zis, const float* __restrict__ zjs, int N,
                                                           int D, int Mpad, int Dpad, int ns, int cosine, float fac,
                                                           const float* __restrict__ part, const float* __restrict__ inv,
                                                           const float* __restrict__ sc, const float* __restrict__ g_loss,
                                                           float* __restrict__ g_zis, float* __restrict__ g_zjs) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= 2 * N) return;
    const float* src = nx_row(zis, zjs, a, N, D);
    float* dst = a < N ? g_zjs + (size_t)a * D : g_zis + (size_t)(a - N) * D;
    const float f = g_loss[0] * (fac * sc[1]), iv = inv[a];
    const size_t stride = (size_t)Mpad * Dpad;
    const float* pr = part + (size_t)a * Dpad;
    const bool proj = cosine && iv < 0.99e8f;                     // a row below the 1e-8 clamp is scaled, not projected
    float dot = 0.f;
    if (proj) {
        for (int k = lane; k < D; k += 64) {
            float d = 0.f;
            for (int s = 0; s < ns; ++s) d += pr[s * stride + k];
            dot = fmaf(src[k] * iv, d * f, dot);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) dot += __shfl_xor(dot, off);
    }
    for (int k = lane; k < D; k += 64) {
        float d = 0.f;
        for (int s = 0; s < ns; ++s) d += pr[s * stride + k];
        d *= f;
        dst[k] = proj ? (d - (src[k] * iv) * dot) * iv : (cosine ? d * iv : d);
    }
}

int nx_check(const void* zis, const void* zjs, int64_t n, int d, float temperature, const void* ws) {
    if (!zis || !zjs || !ws || n < 1 || d < 1 || !(temperature > 0.f)) return DSMIL_E_INVALID;
    if (2 * n > (1 << 17) || d > 4096) return DSMIL_E_UNSUPPORTED;
    if ((uintptr_t)ws % 256) return DSMIL_E_ALIGN;
    return DSMIL_OK;
}

// the three prep launches: both entry points run them, so the backward never depends on what a forward left in ws
int nx_prep(const float* zis, const float* zjs, int N, int d, int cosine, const NxPlan& P, char* ws, hipStream_t st) {
    float* inv = (float*)(ws + P.inv);
    float* rowmax = (float*)(ws + P.rowmax);
    float* sc = (float*)(ws + P.sc);
    hipLaunchKernelGGL(k_nx_rowstat, dim3(P.Mpad / 4), dim3(NX_THREADS), 0, st, zis, zjs, N, d, cosine, inv, rowmax);
    hipLaunchKernelGGL(k_nx_scale, dim3(1), dim3(1024), 0, st, (const float*)rowmax, P.M, cosine, sc);
    hipLaunchKernelGGL(k_nx_cut, dim3(P.Mpad / 64, (P.Dpad + 63) / 64), dim3(NX_THREADS), 0, st, zis, zjs, N, d, P.Mpad, P.Dpad,
                       (const float*)inv, (const float*)sc, (nx_f16*)(ws + P.planes), (nx_f16*)(ws + P.tplanes));
    return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH;
}

}  // namespace

extern "C" {

size_t dsmil_ntxent_workspace_bytes(int64_t n, int d) {
    if (n < 1 || d < 1 || 2 * n > (1 << 17) || d > 4096) return 0;
    return nx_plan(n, d).total;
}

int dsmil_ntxent_forward(const float* zis, const float* zjs, int64_t n, int d, float temperature, int cosine, float* loss,
                         float* lse, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!loss || !lse) return DSMIL_E_INVALID;
    const int rc = nx_check(zis, zjs, n, d, temperature, ws);
    if (rc) return rc;
    const NxPlan P = nx_plan(n, d);
    if (ws_bytes < P.total) return DSMIL_E_WORKSPACE;
    char* w = (char*)ws;
    cosine = cosine ? 1 : 0;
    const int pr = nx_prep(zis, zjs, (int)n, d, cosine, P, w, stream);
    if (pr) return pr;
    float* pm = (float*)(w + P.pm);
    float* pl = (float*)(w + P.pl);
    float* pos = (float*)(w + P.pos);
    const dim3 grid(P.Mpad / NX_BM, P.nsf);
    const float inv_t = 1.0f / temperature;
    if (P.Dpad <= 256)
        hipLaunchKernelGGL(k_nx_fwd<true>, grid, dim3(NX_THREADS), 0, stream, (const nx_f16*)(w + P.planes),
                           (const float*)(w + P.sc), (int)n, P.Mpad, P.Dpad, inv_t, P.tpf, pm, pl, pos);
    else
        hipLaunchKernelGGL(k_nx_fwd<false>, grid, dim3(NX_THREADS), 0, stream, (const nx_f16*)(w + P.planes),
                           (const float*)(w + P.sc), (int)n, P.Mpad, P.Dpad, inv_t, P.tpf, pm, pl, pos);
    hipLaunchKernelGGL(k_nx_finish, dim3(1), dim3(1024), 0, stream, (const float*)pm, (const float*)pl, (const float*)pos, P.M,
                       P.Mpad, P.nsf, lse, loss);
    return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH;
}

int dsmil_ntxent_backward(const float* zis, const float* zjs, int64_t n, int d, float temperature, int cosine, const float* lse,
                          const float* g_loss, float* g_zis, float* g_zjs, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!lse || !g_loss || !g_zis || !g_zjs) return DSMIL_E_INVALID;
    const int rc = nx_check(zis, zjs, n, d, temperature, ws);
    if (rc) return rc;
    const NxPlan P = nx_plan(n, d);
    if (ws_bytes < P.total) return DSMIL_E_WORKSPACE;
    char* w = (char*)ws;
    cosine = cosine ? 1 : 0;
    const int pr = nx_prep(zis, zjs, (int)n, d, cosine, P, w, stream);
    if (pr) return pr;
    float* part = (float*)(w + P.part);
    const dim3 grid(P.Mpad / NX_BM, P.nsb, P.nfc);
    const float inv_t = 1.0f / temperature;
    const int lds = NX_SBYTES + NX_TBYTES;
    const void* fn = P.Dpad <= 256 ? (const void*)k_nx_bwd<true> : (const void*)k_nx_bwd<false>;
    if (!dsmil_lds::allow(fn, lds)) return DSMIL_E_LAUNCH;
    if (P.Dpad <= 256)
        hipLaunchKernelGGL(k_nx_bwd<true>, grid, dim3(NX_THREADS), lds, stream, (const nx_f16*)(w + P.planes),
                           (const nx_f16*)(w + P.tplanes), (const float*)(w + P.sc), lse, (int)n, P.Mpad, P.Dpad, inv_t, P.tpb,
                           part);
    else
        hipLaunchKernelGGL(k_nx_bwd<false>, grid, dim3(NX_THREADS), lds, stream, (const nx_f16*)(w + P.planes),
                           (const nx_f16*)(w + P.tplanes), (const float*)(w + P.sc), lse, (int)n, P.Mpad, P.Dpad, inv_t, P.tpb,
                           part);
    const float fac = (float)(1.0 / ((double)(1 << NX_WSHIFT) * (double)P.M * (double)temperature));
    hipLaunchKernelGGL(k_nx_bwd_fin, dim3((P.M + 3) / 4), dim3(NX_THREADS), 0, stream, zis, zjs, (int)n, d, P.Mpad, P.Dpad, P.nsb,
                       cosine, fac, (const float*)part, (const float*)(w + P.inv), (const float*)(w + P.sc), g_loss, g_zis,
                       g_zjs);
    return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH;
}

}  // extern "C"
