// The stem's InstanceNorm / ReLU / max-pool backward for training the embedder (include/dsmil_hip.h, dsmil_stem_pool_bwd*): the
// gradient of the RAW stem map y [B,H1,W1,C] from the gradient g [B,Hp,Wp,C] of pooled = maxpool3x3/2/1(relu((y - m) r)), with
// the winners `win` [B,Hp,Wp,C] (uint8, position dy * 3 + dx in the window) that dsmil_trunk32_stem_train recorded.  fp32 NHWC.
//     q[n,p,c] = sum over the windows w whose winner is p of g[n,w,c]   if fl(fl(y - m) r) > 0, else 0
//     gy       = r (q - mean_p q - x^ mean_p (q x^))                                      (norm_bwd.hip's INB, same arithmetic)
// A GATHER over the pixels of y: pixel (py, px) lies in the windows oy in {py / 2} (py even) or {(py - 1) / 2, (py + 1) / 2} (py
// odd, the second only where it exists), the same for ox: four windows at most, visited in row-major order; the pixel takes g of a
// window where win says its position.  No atomics: q has one reader-side definition, evaluated twice (sums, then elements).
// The three launches are norm_bwd.hip's, with q from the gather:
//   k_sb_partial   one workgroup per (image, chunk of pixels), emb::chan_layout threads: sum q, sum fma(q, x^) per channel, a
//                  thread adds its pixels serially, the pixel lanes of a wave by xor shuffles (widest stride last), the waves
//                  through LDS in wave order -> ws partials
//   k_sb_finish    one thread per (sum, image, channel): the partials in chunk order, divided by H1 W1 -> ws coefficients
//   k_sb_apply     the element pass on emb::chan_grid
// Every output element has one writer and every sum a fixed order: two calls on the same inputs are bit-identical, and a call
// reads nothing from ws that it has not written itself.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "dsmil_hip.h"
#include "emb_host.h"

namespace {
using namespace emb;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct SbArgs {
    const float *g, *y, *mean, *rstd;
    const uint8_t* win;
    float* gy;
    float *part, *coef;          // ws: partials [2][B][n_partials][C], coefficients [2][B][C]
    int B, H1, W1, Hp, Wp, C, chunk, nparts;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 xor4(f32x4 v, int m) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __shfl_xor(v[e], m, 64);
    return o;
}

// what pixel p = py W1 + px of image n collects from the windows it won, channels c4 * 4 .. + 3, before the ReLU mask: its
// windows in row-major order, a window's g added where win names this pixel's position (an exact + 0 elsewhere)
// RECOMP (experiment builds only, DSMIL_STEM_BWD=recompute): the same decision without `win`, from the 3 x 3 values of the
// window — the pixel (its own a = xh) wins where no earlier position holds a value >= a and no later one a value > a
template <bool RECOMP>
__device__ __forceinline__ f32x4 sb_collect(const SbArgs& a, int n, int p, int c4, f32x4 mu, f32x4 rs, f32x4 xh) {
    const int py = p / a.W1, px = p - py * a.W1;
    const int oy0 = py >> 1, ox0 = px >> 1;                  // the first window of each dimension; an odd coordinate has a second
    const int ny = 1 + ((py & 1) && oy0 + 1 < a.Hp), nx = 1 + ((px & 1) && ox0 + 1 < a.Wp);
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    for (int iy = 0; iy < ny; ++iy) {
        const int oy = oy0 + iy, dy = py - 2 * oy + 1;
        for (int ix = 0; ix < nx; ++ix) {
            const int ox = ox0 + ix, pos = dy * 3 + (px - 2 * ox + 1);
            const unsigned o = (((unsigned)n * a.Hp + oy) * (unsigned)a.Wp + ox) * (unsigned)a.C + c4 * 4;
            const f32x4 gv = ld4(a.g + o);
            if constexpr (RECOMP) {
                bool won[4] = {true, true, true, true};
                for (int k = 0; k < 9; ++k) {
                    const int wy = 2 * oy - 1 + k / 3, wx = 2 * ox - 1 + k % 3;
                    if (k == pos || wy < 0 || wy >= a.H1 || wx < 0 || wx >= a.W1) continue;
                    const f32x4 v = ld4(a.y + (((unsigned)n * a.H1 + wy) * (unsigned)a.W1 + wx) * (unsigned)a.C + c4 * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float t = (v[e] - mu[e]) * rs[e];
                        won[e] = won[e] && (k < pos ? t < xh[e] : t <= xh[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) q[e] += won[e] ? gv[e] : 0.f;
            } else {
                const uchar4 w = *reinterpret_cast<const uchar4*>(a.win + o);
                q[0] += w.x == pos ? gv[0] : 0.f;
                q[1] += w.y == pos ? gv[1] : 0.f;
                q[2] += w.z == pos ? gv[2] : 0.f;
                q[3] += w.w == pos ? gv[3] : 0.f;
            }
        }
    }
    return q;
}

// sums[0] = sum q, sums[1] = sum q x^ over the pixels of chunk blockIdx.x % nparts of image blockIdx.x / nparts
template <bool RECOMP>
__global__ __launch_bounds__(256) void k_sb_partial(const SbArgs a) {
    __shared__ f32x4 red[2][256];
    const int C = a.C, HW = a.H1 * a.W1;
    const ChanLayout cl = chan_layout(C);
    const int lanes_c = cl.lanes_c, cpt = cl.cpt, tpb = cl.tpb;
    const int tid = threadIdx.x, c40 = tid % lanes_c, pl = tid / lanes_c;
    const int n = blockIdx.x / a.nparts, k = blockIdx.x % a.nparts;
    const int p0 = k * a.chunk, p1 = min(HW, p0 + a.chunk);
    // rows of the LDS step: a wave narrower than a pixel row of channel groups holds 64 / lanes_c pixel lanes, shuffled first
    const bool shuf = lanes_c < 64;
    const int rows = shuf ? 4 : tpb, row = shuf ? tid / 64 : pl;
    for (int j = 0; j < cpt; ++j) {
        const int c4 = c40 + 256 * j;
        const unsigned sc = (unsigned)n * C + c4 * 4;
        const f32x4 mu = ld4(a.mean + sc), rs = ld4(a.rstd + sc);
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
        for (int p = p0 + pl; p < p1; p += tpb) {
            const f32x4 yv = ld4(a.y + ((unsigned)n * HW + p) * (unsigned)C + c4 * 4);
            f32x4 xh;
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[e] = (yv[e] - mu[e]) * rs[e];
            const f32x4 qc = sb_collect<RECOMP>(a, n, p, c4, mu, rs, xh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float q = xh[e] > 0.f ? qc[e] : 0.f;
                s0[e] += q;
                s1[e] = __fmaf_rn(q, xh[e], s1[e]);
            }
        }
        if (shuf) {
            for (int m = lanes_c; m < 64; m <<= 1) {
                const f32x4 t0 = xor4(s0, m), t1 = xor4(s1, m);
#pragma unroll
                for (int e = 0; e < 4; ++e) { s0[e] += t0[e]; s1[e] += t1[e]; }
            }
        }
        if (j) __syncthreads();                             // the readers of the round before are done
        if (!shuf || (tid & 63) < lanes_c) {
            red[0][row * lanes_c + c40] = s0;
            red[1][row * lanes_c + c40] = s1;
        }
        __syncthreads();
        if (tid < lanes_c) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32x4 t = red[i][tid];
                for (int r = 1; r < rows; ++r) {
                    const f32x4 v = red[i][r * lanes_c + tid];
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] += v[e];
                }
                *reinterpret_cast<f32x4*>(a.part + (((unsigned)i * a.B + n) * a.nparts + k) * (unsigned)C + c4 * 4) = t;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_sb_finish(const float* __restrict__ part, float* __restrict__ coef, int rows, int C,
                                                   int nparts, float hw) {
    const unsigned total = (unsigned)rows * C;              // rows = 2 B
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned r = i / (unsigned)C, c = i % (unsigned)C;
        float s = part[(r * nparts) * (unsigned)C + c];
        for (int k = 1; k < nparts; ++k) s += part[(r * nparts + k) * (unsigned)C + c];
        coef[i] = s / hw;
    }
}

template <bool RECOMP>
__global__ __launch_bounds__(256) void k_sb_apply(const SbArgs a) {
    const int C = a.C, HW = a.H1 * a.W1;
    const ChanLayout cl = chan_layout(C);
    const int lanes_c = cl.lanes_c, cpt = cl.cpt, tpb = cl.tpb;
    const int c40 = threadIdx.x % lanes_c, pl = threadIdx.x / lanes_c;
    const unsigned np = (unsigned)a.B * (unsigned)HW, pstep = gridDim.x * (unsigned)tpb, bc = (unsigned)a.B * C;
    int ncur = -1;
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, rs = mu, mq = mu, mqx = mu;
    for (unsigned p = blockIdx.x * (unsigned)tpb + pl; p < np; p += pstep) {
        const int n = (int)(p / (unsigned)HW), pi = (int)(p - (unsigned)n * HW);
        for (int j = 0; j < cpt; ++j) {
            const int c4 = c40 + 256 * j;
            const unsigned o = p * (unsigned)C + c4 * 4;
            const f32x4 yv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.y + o));
            if (n != ncur || cpt > 1) {                     // the image changes every HW pixels: reload its statistics and means
                const unsigned sc = (unsigned)n * C + c4 * 4;
                mu = ld4(a.mean + sc);
                rs = ld4(a.rstd + sc);
                mq = ld4(a.coef + sc);
                mqx = ld4(a.coef + bc + sc);
            }
            f32x4 xh, o1;
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[e] = (yv[e] - mu[e]) * rs[e];
            const f32x4 qc = sb_collect<RECOMP>(a, n, pi, c4, mu, rs, xh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float q = xh[e] > 0.f ? qc[e] : 0.f;
                o1[e] = rs[e] * __fmaf_rn(-xh[e], mqx[e], q - mq[e]);
            }
            __builtin_nontemporal_store(o1, reinterpret_cast<f32x4*>(a.gy + o));
        }
        ncur = n;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct SbPlan : SumPlan { int Hp, Wp; };                     // (emb_host.h: dsmil_norm_bwd's chunk rule over the H1 W1 pixels)

int sb_check(int B, int H1, int W1, int C) {
    if (B < 1 || H1 < 1 || W1 < 1 || C < 1) return DSMIL_E_INVALID;
    if (!chan_ok(C) || C > 2048) return DSMIL_E_UNSUPPORTED;     // dsmil_norm_bwd's rule
    if (!map_fits(B, H1, W1, C)) return DSMIL_E_UNSUPPORTED;
    return DSMIL_OK;
}

// the shape has passed sb_check.  false: the partials would not fit a 32-bit index (refused as unsupported)
bool sb_plan(int B, int H1, int W1, int C, SbPlan& p) {
    p.Hp = (H1 - 1) / 2 + 1;
    p.Wp = (W1 - 1) / 2 + 1;
    return sum_plan(2, B, H1 * W1, C, p);                    // B H1 W1 C < 2^31
}

// Experiment builds (-DDSMIL_EXPERIMENTS) read DSMIL_STEM_BWD=recompute once per process: the winners recomputed from y instead
// of read from win (A/B, tools/stem_bwd_time.py).  A product build has neither the knob nor the kernels.
#ifdef DSMIL_EXPERIMENTS
bool sb_recompute() {
    static const bool on = [] { const char* s = getenv("DSMIL_STEM_BWD"); return s && !strcmp(s, "recompute"); }();
    return on;
}
void launch_recompute(bool partial, const SbPlan& p, hipStream_t st, const SbArgs& a) {
    if (partial) hipLaunchKernelGGL(k_sb_partial<true>, dim3(p.grid_partial), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_sb_apply<true>, dim3(p.grid_apply), dim3(256), 0, st, a);
}
#else
constexpr bool sb_recompute() { return false; }
inline void launch_recompute(bool, const SbPlan&, hipStream_t, const SbArgs&) {}
#endif

}  // namespace

extern "C" {

int dsmil_stem_pool_bwd_plan(int32_t B, int32_t H1, int32_t W1, int32_t C, int32_t out[16]) {
    if (!out) return DSMIL_E_INVALID;
    if (const int rc = sb_check(B, H1, W1, C)) return rc;
    SbPlan p;
    if (!sb_plan(B, H1, W1, C, p)) return DSMIL_E_UNSUPPORTED;
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[DSMIL_STEM_BWD_PLAN_HP] = p.Hp;
    out[DSMIL_STEM_BWD_PLAN_WP] = p.Wp;
    out[DSMIL_STEM_BWD_PLAN_CHUNK] = p.chunk;
    out[DSMIL_STEM_BWD_PLAN_PARTIALS] = p.nparts;
    out[DSMIL_STEM_BWD_PLAN_RUN_LEN] = p.run_len;
    out[DSMIL_STEM_BWD_PLAN_LANES] = p.lanes;
    out[DSMIL_STEM_BWD_PLAN_GRID_PARTIAL] = p.grid_partial;
    out[DSMIL_STEM_BWD_PLAN_GRID_FINISH] = p.grid_finish;
    out[DSMIL_STEM_BWD_PLAN_GRID_APPLY] = p.grid_apply;
    out[DSMIL_STEM_BWD_PLAN_BLOCK] = 256;
    out[DSMIL_STEM_BWD_PLAN_GROUPS] = p.cpt;
    return DSMIL_OK;
}

size_t dsmil_stem_pool_bwd_workspace_bytes(int32_t B, int32_t H1, int32_t W1, int32_t C) {
    if (sb_check(B, H1, W1, C)) return 0;
    SbPlan p;
    return sb_plan(B, H1, W1, C, p) ? p.total : 0;
}

int dsmil_stem_pool_bwd(const float* g, const float* y, const float* mean, const float* rstd, const uint8_t* win, float* gy,
                        int32_t B, int32_t H1, int32_t W1, int32_t C, void* ws, size_t ws_bytes, void* stream) {
    if (B < 1 || H1 < 1 || W1 < 1 || C < 1 || !g || !y || !mean || !rstd || !win || !gy || !ws) return DSMIL_E_INVALID;
    {
        // gy may share no byte with an input (sizes saturate: such a shape is refused below anyway)
        auto sat = [](unsigned __int128 v) { return v > ((size_t)1 << 62) ? (size_t)1 << 62 : (size_t)v; };
        const size_t nb = sat((unsigned __int128)B * H1 * W1 * C * sizeof(float));
        const size_t pe = sat((unsigned __int128)B * ((H1 - 1) / 2 + 1) * ((W1 - 1) / 2 + 1) * C);   // pooled elements
        const size_t sb = (size_t)B * C * sizeof(float);
        if (overlap(gy, nb, y, nb) || overlap(gy, nb, g, sat((unsigned __int128)pe * sizeof(float))) || overlap(gy, nb, win, pe) ||
            overlap(gy, nb, mean, sb) || overlap(gy, nb, rstd, sb)) return DSMIL_E_INVALID;
    }
    if (const int rc = sb_check(B, H1, W1, C)) return rc;
    SbPlan p;
    if (!sb_plan(B, H1, W1, C, p)) return DSMIL_E_UNSUPPORTED;
    if (!al16(g) || !al16(y) || !al16(mean) || !al16(rstd) || !al16(gy) || ((uintptr_t)win & 3) || !al256p(ws)) return DSMIL_E_ALIGN;
    if (ws_bytes < p.total) return DSMIL_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    float* coef = (float*)((char*)ws + p.off_coef);
    const SbArgs a{g, y, mean, rstd, win, gy, part, coef, B, H1, W1, p.Hp, p.Wp, C, p.chunk, p.nparts};
    const bool recomp = sb_recompute();
    if (recomp) launch_recompute(true, p, st, a);
    else hipLaunchKernelGGL(k_sb_partial<false>, dim3(p.grid_partial), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sb_finish, dim3(p.grid_finish), dim3(256), 0, st, (const float*)part, coef, 2 * B, C, p.nparts,
                       (float)(H1 * W1));
    if (recomp) launch_recompute(false, p, st, a);
    else hipLaunchKernelGGL(k_sb_apply<false>, dim3(p.grid_apply), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH;
}

}  // extern "C"
