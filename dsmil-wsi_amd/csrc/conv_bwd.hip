// Convolution backward for training the embedder: the weight gradient and the data gradient of one conv of the ResNet trunks
// (include/dsmil_hip.h, dsmil_conv_bwd_*).  Layout and arithmetic class are the fp32-class trunk's (resnet_fwd.hip, NPD = 3):
// fp32 NHWC maps, fp32 OIHW weights, two round-to-nearest fp16 planes per operand, h1 w0 + h0 w1 + h0 w0 on
// v_mfma_f32_32x32x16_f16 with fp32 accumulators.  Correctness first: one LDS buffer and two barriers per k-step (the
// weight gradient issues the next step's global loads under the MFMAs).
//
//   k_cb_absmax / k_cb_scale   max |dy| -> sc = (2^s, 2^-s), s = 14 - e for max = f 2^e (k_nx_scale's rule), on the device
//   k_conv_wgrad               dw as a TN GEMM over positions: a workgroup owns 64 cout x 64 columns (column = tap Cin + ci) of
//                              one chunk of positions; both operands are position-major in memory, so the staging threads write
//                              a TRANSPOSED fp16 image ([row][32 positions], two positions per dword) and every lane's k
//                              elements are 8 positions
//   k_conv_wgrad_finish        adds the chunks' partials in chunk order, takes 2^-s out, writes OIHW
//   k_cb_pack_dgrad            w OIHW -> fp16 planes of 2^8 w, [tap][Cout/16][plane][Cin][16]
//   k_conv_dgrad               dx as a gather-form implicit GEMM: 64 input positions of one parity class x 64 cin per
//                              workgroup, K = taps x Cout with the (divisible, in-map) mask applied at staging; a tap no row
//                              of the tile reads is skipped
// No atomics: every output element has one writer and a fixed summation order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dsmil_hip.h"
#include "emb_host.h"

namespace {
using namespace emb;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16;
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

constexpr int CB_T = 64;                     // tile edge (rows and columns of a workgroup's output tile)
constexpr int CB_KS = 32;                    // contraction indices per LDS step (two MFMA k-steps)
constexpr int CB_LD = CB_KS + 8;             // halves per LDS row: 80 bytes, 16-byte aligned fragments
constexpr int CB_WLD = CB_KS / 2 + 1;        // dwords per LDS row of the weight gradient's transposed image
constexpr float CB_WSCALE = 256.f, CB_OSCALE = 1.f / 256.f;   // the forward's weight scale (2^EMB_WSHIFT of resnet_fwd.hip)
constexpr int CB_MAXBLOCKS = 256;            // partial maxima of k_cb_absmax
constexpr int CB_CHUNK0 = 256, CB_CHUNK_MAX = 4096, CB_WG_TARGET = 2048, CB_PARTIALS_MAX = 256;

__device__ __forceinline__ int drow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
// the two planes of a: h = rne16(a), l = rne16(a - h) (a - h is exact in fp32)
__device__ __forceinline__ void cut1(float a, f16& h, f16& l) {
    h = (f16)a;
    l = (f16)(a - (float)h);
}

__device__ __forceinline__ unsigned pack2(f16 lo, f16 hi) {
    return (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
}

// ---- the dy scale ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cb_absmax(const float* __restrict__ v, long long n4, float* __restrict__ pmax) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    float mx = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(v + 4 * i);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(q[0]), fabsf(q[1]))), fmaxf(fabsf(q[2]), fabsf(q[3])));
    }
    red[tid] = mx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) pmax[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_cb_scale(const float* __restrict__ pmax, int n, float* __restrict__ sc) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    red[tid] = tid < n ? pmax[tid] : 0.f;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        int x = 0;
        frexpf(red[0], &x);                                   // max = f 2^x, f in [0.5, 1)
        int e = red[0] > 0.f ? 14 - x : 0;
        e = e < -60 ? -60 : (e > 60 ? 60 : e);
        sc[0] = ldexpf(1.0f, e);
        sc[1] = ldexpf(1.0f, -e);
    }
}

// one k-step of a wave's 32 x 32 tile: rows of sa against rows of sb, the three products smallest first
__device__ __forceinline__ void cb_mfmas(const f16 (*sa)[CB_T][CB_LD], const f16 (*sb)[CB_T][CB_LD], int ra, int rb, int hi,
                                         f32x16& acc) {
#pragma unroll
    for (int kk = 0; kk < CB_KS / 16; ++kk) {
        f16x8_t af[2], bf[2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            af[pl] = *reinterpret_cast<const f16x8_t*>(&sa[pl][ra][kk * 16 + 8 * hi]);
            bf[pl] = *reinterpret_cast<const f16x8_t*>(&sb[pl][rb][kk * 16 + 8 * hi]);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[1], bf[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0], bf[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0], bf[0], acc, 0, 0, 0);
    }
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------
struct WgArgs {
    const float* x;
    const float* mean;     // [B,Cin] or null
    const float* rstd;
    const float* dy;
    const float* sc;
    float* part;           // [chunks][Cout][colpad]
    int B, H, W, Cin, Ho, Wo, Cout, ks, stride, pad, Kc, colpad, chunk;
    long long M;           // B Ho Wo
};

// VEC: Cin % 4 == 0, a thread's four columns are four channels of one tap (one 16-byte load); else (the stem) column by column
template <bool VEC, bool NORM>
__global__ __launch_bounds__(256) void k_conv_wgrad(WgArgs a) {
    // [plane][row][position pair]: a dword holds two consecutive positions of one row, so the transposing store is one
    // ds_write_b32 per (row, plane).  Row stride 17 dwords: the 16 row groups x 4 pairs a wave stores land 2 to a bank (a
    // 16-byte-aligned stride puts them 8 to a bank), and the 32 rows of a fragment read hit 32 banks
    __shared__ unsigned sA[2][CB_T][CB_WLD];
    __shared__ unsigned sB[2][CB_T][CB_WLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, l31 = lane & 31, hi = lane >> 5;
    const int col0 = blockIdx.x * CB_T, co0 = blockIdx.y * CB_T;
    const long long p0 = (long long)blockIdx.z * a.chunk;
    const long long pend = (p0 + a.chunk < a.M) ? p0 + a.chunk : a.M;
    const float s = a.sc[0];
    const int g = tid & 15, pr = tid >> 4;        // this thread stages rows 4g .. 4g+3 at positions 2 pr and 2 pr + 1 of a step
    const int HW = a.Ho * a.Wo;
    constexpr int NC = VEC ? 1 : 4;
    int cky[NC], ckx[NC], cci[NC];
    bool cok[NC];
#pragma unroll
    for (int e = 0; e < NC; ++e) {
        const int c = col0 + 4 * g + e;
        cok[e] = c < a.Kc;
        const int tap = cok[e] ? c / a.Cin : 0;
        cci[e] = cok[e] ? c - tap * a.Cin : 0;
        cky[e] = tap / a.ks;
        ckx[e] = tap - cky[e] * a.ks;
    }
    f32x4 ra[2], rb[2];
    auto load = [&](long long p) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long q = p + 2 * pr + i;
            ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (q >= pend) continue;
            ra[i] = *reinterpret_cast<const f32x4*>(a.dy + q * a.Cout + co0 + 4 * g);
            const int n = (int)(q / HW), rem = (int)(q - (long long)n * HW);
            const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
            if constexpr (VEC) {
                const int iy = oy * a.stride - a.pad + cky[0], ix = ox * a.stride - a.pad + ckx[0];
                if (cok[0] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    f32x4 v = *reinterpret_cast<const f32x4*>(a.x + (((long long)n * a.H + iy) * a.W + ix) * a.Cin + cci[0]);
                    if constexpr (NORM) {
                        const f32x4 mu = *reinterpret_cast<const f32x4*>(a.mean + (long long)n * a.Cin + cci[0]);
                        const f32x4 rs = *reinterpret_cast<const f32x4*>(a.rstd + (long long)n * a.Cin + cci[0]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf((v[e] - mu[e]) * rs[e], 0.f);
                    }
                    rb[i] = v;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int iy = oy * a.stride - a.pad + cky[e], ix = ox * a.stride - a.pad + ckx[e];
                    if (cok[e] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                        float v = a.x[(((long long)n * a.H + iy) * a.W + ix) * a.Cin + cci[e]];
                        if constexpr (NORM) v = fmaxf((v - a.mean[(long long)n * a.Cin + cci[e]]) * a.rstd[(long long)n * a.Cin + cci[e]], 0.f);
                        rb[i][e] = v;
                    }
                }
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load(p0);
    for (long long p = p0; p < pend; p += CB_KS) {
        __syncthreads();                               // the previous step's fragments are read
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f16 h0, l0, h1, l1;
            cut1(ra[0][e] * s, h0, l0);                // a power of two: exact
            cut1(ra[1][e] * s, h1, l1);
            sA[0][4 * g + e][pr] = pack2(h0, h1);
            sA[1][4 * g + e][pr] = pack2(l0, l1);
            cut1(rb[0][e], h0, l0);
            cut1(rb[1][e], h1, l1);
            sB[0][4 * g + e][pr] = pack2(h0, h1);
            sB[1][4 * g + e][pr] = pack2(l0, l1);
        }
        __syncthreads();
        if (p + CB_KS < pend) load(p + CB_KS);
#pragma unroll
        for (int kk = 0; kk < CB_KS / 16; ++kk) {
            f16x8_t af[2], bf[2];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const unsigned* pa = &sA[pl][wm * 32 + l31][kk * 8 + 4 * hi];
                const unsigned* pb = &sB[pl][wn * 32 + l31][kk * 8 + 4 * hi];
                af[pl] = __builtin_bit_cast(f16x8_t, u32x4_t{pa[0], pa[1], pa[2], pa[3]});
                bf[pl] = __builtin_bit_cast(f16x8_t, u32x4_t{pb[0], pb[1], pb[2], pb[3]});
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[1], bf[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0], bf[1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0], bf[0], acc, 0, 0, 0);
        }
    }
    float* o = a.part + ((long long)blockIdx.z * a.Cout + co0 + wm * 32) * a.colpad + col0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[(long long)drow(r, hi) * a.colpad] = acc[r];
}

__global__ __launch_bounds__(256) void k_conv_wgrad_finish(const float* __restrict__ part, const float* __restrict__ sc,
                                                           float* __restrict__ dw, int Cout, int Cin, int taps, int colpad,
                                                           int nchunks) {
    const long long total = (long long)Cout * Cin * taps;
    const float inv = sc[1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int t = (int)(i % taps);
        const long long r = i / taps;
        const int ci = (int)(r % Cin), co = (int)(r / Cin);
        const float* src = part + (long long)co * colpad + t * Cin + ci;
        float sum = src[0];
        for (int z = 1; z < nchunks; ++z) sum += src[(long long)z * Cout * colpad];
        dw[i] = sum * inv;
    }
}

// ---- data gradient ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cb_pack_dgrad(const float* __restrict__ w, unsigned short* __restrict__ out, int O, int I,
                                                       int taps) {
    const long long total = (long long)O * I * taps;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int t = (int)(i % taps);
        const long long r = i / taps;
        const int ci = (int)(r % I), o = (int)(r / I);
        f16 h, l;
        cut1(w[i] * CB_WSCALE, h, l);
        const long long base = ((((long long)t * (O / 16) + o / 16) * 2) * I + ci) * 16 + (o & 15);
        out[base] = __builtin_bit_cast(unsigned short, h);
        out[base + (long long)I * 16] = __builtin_bit_cast(unsigned short, l);
    }
}

struct DgArgs {
    const float* dy;
    const unsigned short* wpk;
    const float* sc;
    float* dx;
    int B, H, W, Cin, Ho, Wo, Cout, ks, stride, pad;
    int tile0[5];          // first tile of each parity class (stride^2 classes), and the tile count behind the last
};

// Input pixels are dealt to tiles by PARITY CLASS (iy mod stride, ix mod stride): a tap is divisible for every row of a class
// or for none, so at stride 2 the tap skip below drops three taps of four instead of feeding masked zeros to the MFMAs.
// Pixel j of class (py, px): n = j / (Hc Wc), iy = py + stride (j / Wc mod Hc), ix = px + stride (j mod Wc).
struct DgClass { int py, px, Hc, Wc; long long cnt; };
__host__ __device__ inline DgClass dg_class(int c, int B, int H, int W, int stride) {
    DgClass k;
    k.py = c / stride;
    k.px = c - k.py * stride;
    k.Hc = H > k.py ? (H - k.py + stride - 1) / stride : 0;
    k.Wc = W > k.px ? (W - k.px + stride - 1) / stride : 0;
    k.cnt = (long long)B * k.Hc * k.Wc;
    return k;
}
// -1 behind the class's last pixel, else the pixel's index in the [B, H, W] map
__device__ __forceinline__ long long dg_pixel(const DgClass& k, long long j, int H, int W, int stride, int& n, int& iy, int& ix) {
    if (j >= k.cnt) return -1;
    const int hw = k.Hc * k.Wc;
    n = (int)(j / hw);
    const int rem = (int)(j - (long long)n * hw);
    const int yc = rem / k.Wc;
    iy = k.py + stride * yc;
    ix = k.px + stride * (rem - yc * k.Wc);
    return ((long long)n * H + iy) * W + ix;
}

__global__ __launch_bounds__(256) void k_conv_dgrad(DgArgs a) {
    __shared__ __attribute__((aligned(16))) f16 sA[2][CB_T][CB_LD];
    __shared__ __attribute__((aligned(16))) f16 sB[2][CB_T][CB_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, l31 = lane & 31, hi = lane >> 5;
    int cls = 0;
    while (cls + 1 < a.stride * a.stride && (int)blockIdx.x >= a.tile0[cls + 1]) ++cls;
    const DgClass kc = dg_class(cls, a.B, a.H, a.W, a.stride);
    const long long m0 = (long long)((int)blockIdx.x - a.tile0[cls]) * CB_T;      // first pixel of the tile inside its class
    const int n0 = blockIdx.y * CB_T;
    const float s = a.sc[0];
    const int row = tid >> 2, part = tid & 3;     // staging: row of either tile, 8 of the step's 32 cout
    int n = 0, iy = 0, ix = 0;
    const bool qok = dg_pixel(kc, m0 + row, a.H, a.W, a.stride, n, iy, ix) >= 0;
    const int ci = n0 + row;
    const bool ciok = ci < a.Cin;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int taps = a.ks * a.ks;
    for (int tap = 0; tap < taps; ++tap) {
        const int ky = tap / a.ks, kx = tap - ky * a.ks;
        const int ty = iy + a.pad - ky, tx = ix + a.pad - kx;
        bool ok = qok && ty >= 0 && tx >= 0 && (ty % a.stride) == 0 && (tx % a.stride) == 0;
        const int oy = ok ? ty / a.stride : 0, ox = ok ? tx / a.stride : 0;
        ok = ok && oy < a.Ho && ox < a.Wo;
        if (!__syncthreads_or(ok ? 1 : 0)) continue;   // no row of the tile reads this tap (uniform over the workgroup)
        const float* src = a.dy + (((long long)n * a.Ho + (ok ? oy : 0)) * a.Wo + (ok ? ox : 0)) * a.Cout + part * 8;
        const unsigned short* wt = a.wpk + (long long)tap * a.Cout * 2 * a.Cin + (long long)(ciok ? ci : 0) * 16 + (part & 1) * 8;
        for (int cb = 0; cb < a.Cout; cb += CB_KS) {
            f32x4 d0 = f32x4{0.f, 0.f, 0.f, 0.f}, d1 = d0;
            if (ok) {
                d0 = *reinterpret_cast<const f32x4*>(src + cb);
                d1 = *reinterpret_cast<const f32x4*>(src + cb + 4);
            }
            u32x4_t wb[2] = {u32x4_t{0u, 0u, 0u, 0u}, u32x4_t{0u, 0u, 0u, 0u}};
            if (ciok) {
                const unsigned short* wsrc = wt + (long long)((cb >> 4) + (part >> 1)) * 2 * a.Cin * 16;
                wb[0] = *reinterpret_cast<const u32x4_t*>(wsrc);
                wb[1] = *reinterpret_cast<const u32x4_t*>(wsrc + (long long)a.Cin * 16);
            }
            f16x8_t h8, l8;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f16 h, l;
                cut1(d0[e] * s, h, l);
                h8[e] = h;
                l8[e] = l;
                cut1(d1[e] * s, h, l);
                h8[4 + e] = h;
                l8[4 + e] = l;
            }
            __syncthreads();                           // the previous step's fragments are read
            *reinterpret_cast<f16x8_t*>(&sA[0][row][part * 8]) = h8;
            *reinterpret_cast<f16x8_t*>(&sA[1][row][part * 8]) = l8;
            *reinterpret_cast<u32x4_t*>(&sB[0][row][part * 8]) = wb[0];
            *reinterpret_cast<u32x4_t*>(&sB[1][row][part * 8]) = wb[1];
            __syncthreads();
            cb_mfmas(sA, sB, wm * 32 + l31, wn * 32 + l31, hi, acc);
        }
    }
    const float scale = a.sc[1] * CB_OSCALE;
    const int co = n0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        int pn, py, px;
        const long long p = dg_pixel(kc, m0 + wm * 32 + drow(r, hi), a.H, a.W, a.stride, pn, py, px);
        if (p >= 0 && co < a.Cin) a.dx[p * a.Cin + co] = acc[r] * scale;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct CbPlan {
    int which, Ho, Wo, Kc, colpad, chunk, nchunks, run_len, gmax, tile0[5];
    long long M, n_dy;
    dim3 grid;
    size_t off_sc, off_pmax, off_main, total;
};

int cb_check(int Cin, int Cout, int ks, int stride, int pad, int B, int H, int W, int which) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || ks < 1 || stride < 1 || pad < 0) return DSMIL_E_INVALID;
    if (which != DSMIL_CONV_BWD_WEIGHT && which != DSMIL_CONV_BWD_DATA) return DSMIL_E_INVALID;
    if (!(Cin % 16 == 0 || (Cin == 3 && which == DSMIL_CONV_BWD_WEIGHT)) || Cout % 64 != 0) return DSMIL_E_UNSUPPORTED;
    if ((ks != 1 && ks != 3 && ks != 7) || (stride != 1 && stride != 2) || pad > ks / 2) return DSMIL_E_UNSUPPORTED;
    ConvMap m;
    if (!conv_map(B, H, W, Cin, Cout, ks, stride, pad, m)) return DSMIL_E_UNSUPPORTED;
    return map_fits(Cout, Cin, ks, ks) ? DSMIL_OK : DSMIL_E_UNSUPPORTED;   // the OIHW weights: the finish and pack kernels' index
}

// the shape has passed cb_check.  false: the partials would not fit an int (refused as unsupported)
bool cb_plan(int Cin, int Cout, int ks, int stride, int pad, int B, int H, int W, int which, CbPlan& p) {
    p.which = which;
    p.Ho = outdim(H, ks, stride, pad);
    p.Wo = outdim(W, ks, stride, pad);
    p.n_dy = (long long)B * p.Ho * p.Wo * Cout;
    p.gmax = (int)((p.n_dy / 4 + 255) / 256 < CB_MAXBLOCKS ? (p.n_dy / 4 + 255) / 256 : CB_MAXBLOCKS);
    p.off_sc = 0;
    p.off_pmax = 256;
    p.off_main = p.off_pmax + al256(CB_MAXBLOCKS * sizeof(float));
    size_t main_bytes;
    if (which == DSMIL_CONV_BWD_WEIGHT) {
        p.M = (long long)B * p.Ho * p.Wo;
        p.Kc = Cin * ks * ks;
        p.colpad = (p.Kc + CB_T - 1) / CB_T * CB_T;
        const long long tiles = (long long)(p.colpad / CB_T) * (Cout / CB_T);
        p.chunk = CB_CHUNK0;
        // fewer, longer chunks while there are more workgroups than CB_WG_TARGET or more partials per element than the
        // finish kernel's serial sum should walk
        auto nch_of = [&](int c) { return (p.M + c - 1) / c; };
        while ((nch_of(p.chunk) * tiles > CB_WG_TARGET || nch_of(p.chunk) > CB_PARTIALS_MAX) && p.chunk < CB_CHUNK_MAX) p.chunk *= 2;
        const long long nch = (p.M + p.chunk - 1) / p.chunk;
        if (nch > 65535 || nch * Cout * p.colpad >= 0x7fffffffLL) return false;
        p.nchunks = (int)nch;
        p.run_len = (int)(p.M < p.chunk ? p.M : p.chunk);
        p.grid = dim3(p.colpad / CB_T, Cout / CB_T, p.nchunks);
        main_bytes = (size_t)nch * Cout * p.colpad * sizeof(float);
    } else {
        p.M = (long long)B * H * W;
        p.Kc = 0;
        p.colpad = 0;
        p.chunk = 0;
        p.nchunks = 1;
        p.run_len = Cout * ks * ks;
        long long ntiles = 0;
        for (int c = 0; c < 5; ++c) {
            p.tile0[c] = (int)ntiles;
            if (c < stride * stride) ntiles += (dg_class(c, B, H, W, stride).cnt + CB_T - 1) / CB_T;
        }
        p.grid = dim3((unsigned)ntiles, (Cin + CB_T - 1) / CB_T, 1);
        main_bytes = (size_t)ks * ks * Cout * Cin * 2 * sizeof(unsigned short);
    }
    p.total = p.off_main + al256(main_bytes);
    return true;
}

void cb_scale(const float* dy, const CbPlan& p, char* ws, hipStream_t st) {
    float* pmax = (float*)(ws + p.off_pmax);
    hipLaunchKernelGGL(k_cb_absmax, dim3(p.gmax), dim3(256), 0, st, dy, p.n_dy / 4, pmax);
    hipLaunchKernelGGL(k_cb_scale, dim3(1), dim3(256), 0, st, (const float*)pmax, p.gmax, (float*)(ws + p.off_sc));
}

}  // namespace

extern "C" {

int dsmil_conv_bwd_plan(int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad, int32_t B, int32_t H, int32_t W,
                        int32_t which, int32_t out[16]) {
    if (!out) return DSMIL_E_INVALID;
    if (const int rc = cb_check(Cin, Cout, ks, stride, pad, B, H, W, which)) return rc;
    CbPlan p;
    if (!cb_plan(Cin, Cout, ks, stride, pad, B, H, W, which, p)) return DSMIL_E_UNSUPPORTED;
    for (int i = 0; i < 16; ++i) out[i] = 0;
    const bool wg = which == DSMIL_CONV_BWD_WEIGHT;
    out[DSMIL_CONV_BWD_PLAN_WHICH] = which;
    out[DSMIL_CONV_BWD_PLAN_HO] = p.Ho;
    out[DSMIL_CONV_BWD_PLAN_WO] = p.Wo;
    out[DSMIL_CONV_BWD_PLAN_OUT0] = wg ? Cout : (int32_t)p.M;
    out[DSMIL_CONV_BWD_PLAN_OUT1] = wg ? p.Kc : Cin;
    out[DSMIL_CONV_BWD_PLAN_GRID_X] = (int32_t)p.grid.x;
    out[DSMIL_CONV_BWD_PLAN_GRID_Y] = (int32_t)p.grid.y;
    out[DSMIL_CONV_BWD_PLAN_GRID_Z] = (int32_t)p.grid.z;
    out[DSMIL_CONV_BWD_PLAN_BLOCK] = 256;
    out[DSMIL_CONV_BWD_PLAN_CHUNK] = p.chunk;
    out[DSMIL_CONV_BWD_PLAN_PARTIALS] = p.nchunks;
    out[DSMIL_CONV_BWD_PLAN_RUN_LEN] = p.run_len;
    out[DSMIL_CONV_BWD_PLAN_COLS_PAD] = p.colpad;
    return DSMIL_OK;
}

size_t dsmil_conv_bwd_workspace_bytes(int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad, int32_t B, int32_t H,
                                      int32_t W, int32_t which) {
    if (cb_check(Cin, Cout, ks, stride, pad, B, H, W, which)) return 0;
    CbPlan p;
    return cb_plan(Cin, Cout, ks, stride, pad, B, H, W, which, p) ? p.total : 0;
}

int dsmil_conv_bwd_weight(const float* x, const float* in_mean, const float* in_rstd, const float* dy, float* dw_oihw, int32_t B,
                          int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad, void* ws,
                          size_t ws_bytes, void* stream) {
    if (!x || !dy || !dw_oihw || !ws || (in_mean == nullptr) != (in_rstd == nullptr)) return DSMIL_E_INVALID;
    if (const int rc = cb_check(Cin, Cout, ks, stride, pad, B, H, W, DSMIL_CONV_BWD_WEIGHT)) return rc;
    CbPlan p;
    if (!cb_plan(Cin, Cout, ks, stride, pad, B, H, W, DSMIL_CONV_BWD_WEIGHT, p)) return DSMIL_E_UNSUPPORTED;
    const bool vec = Cin % 4 == 0;
    if ((vec ? !al16(x) || !al16(in_mean) || !al16(in_rstd) : (((uintptr_t)x | (uintptr_t)in_mean | (uintptr_t)in_rstd) & 3) != 0) ||
        !al16(dy) || ((uintptr_t)dw_oihw & 3) || !al256p(ws)) return DSMIL_E_ALIGN;
    if (ws_bytes < p.total) return DSMIL_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    cb_scale(dy, p, w, st);
    float* part = (float*)(w + p.off_main);
    const WgArgs a{x, in_mean, in_rstd, dy, (const float*)(w + p.off_sc), part, B, H, W, Cin, p.Ho, p.Wo, Cout, ks, stride, pad,
                   p.Kc, p.colpad, p.chunk, p.M};
    const bool norm = in_mean != nullptr;
    if (vec && norm) hipLaunchKernelGGL((k_conv_wgrad<true, true>), p.grid, dim3(256), 0, st, a);
    else if (vec) hipLaunchKernelGGL((k_conv_wgrad<true, false>), p.grid, dim3(256), 0, st, a);
    else if (norm) hipLaunchKernelGGL((k_conv_wgrad<false, true>), p.grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_conv_wgrad<false, false>), p.grid, dim3(256), 0, st, a);
    const long long total = (long long)Cout * Cin * ks * ks;
    const int fgrid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_conv_wgrad_finish, dim3(fgrid), dim3(256), 0, st, (const float*)part, (const float*)(w + p.off_sc), dw_oihw,
                       Cout, Cin, ks * ks, p.colpad, p.nchunks);
    return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH;
}

int dsmil_conv_bwd_data(const float* dy, const float* w_oihw, float* dx, int32_t B, int32_t H, int32_t W, int32_t Cin,
                        int32_t Cout, int32_t ks, int32_t stride, int32_t pad, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !w_oihw || !dx || !ws) return DSMIL_E_INVALID;
    if (const int rc = cb_check(Cin, Cout, ks, stride, pad, B, H, W, DSMIL_CONV_BWD_DATA)) return rc;
    CbPlan p;
    if (!cb_plan(Cin, Cout, ks, stride, pad, B, H, W, DSMIL_CONV_BWD_DATA, p)) return DSMIL_E_UNSUPPORTED;
    if (!al16(dy) || !al16(dx) || ((uintptr_t)w_oihw & 3) || !al256p(ws)) return DSMIL_E_ALIGN;
    if (ws_bytes < p.total) return DSMIL_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    cb_scale(dy, p, w, st);
    unsigned short* wpk = (unsigned short*)(w + p.off_main);
    const long long total = (long long)Cout * Cin * ks * ks;
    const int pgrid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_cb_pack_dgrad, dim3(pgrid), dim3(256), 0, st, w_oihw, wpk, Cout, Cin, ks * ks);
    const DgArgs a{dy, (const unsigned short*)wpk, (const float*)(w + p.off_sc), dx, B, H, W, Cin, p.Ho, p.Wo, Cout, ks, stride, pad,
                   {p.tile0[0], p.tile0[1], p.tile0[2], p.tile0[3], p.tile0[4]}};
    hipLaunchKernelGGL(k_conv_dgrad, p.grid, dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH;
}

}  // extern "C"
