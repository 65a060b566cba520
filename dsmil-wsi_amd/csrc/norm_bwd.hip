// InstanceNorm / ReLU / residual-add backward for training the embedder (include/dsmil_hip.h, dsmil_norm_bwd*): the gradient of a
// RAW conv output y from the gradient of what the forward made of it.  fp32 NHWC maps [B,HW,C], statistics [B,C], the layout
// dsmil_trunk32_conv / dsmil_trunk32_tail read and write.  With x^ = (y - m) r and a masked upstream gradient q,
//     gy = r (q - mean_p q - x^ mean_p (q x^))                       (biased variance, no affine)
//   kind RELU      q = g where fl(fl(y - m) r) > 0 (the operand the next conv stages)
//   kind ADD       q = g where the saved out = relu(IN(y) + idn) > 0;  gres = q
//   kind ADD_DOWN  as ADD, and gyd = rd (q - mean_p q - x^d mean_p (q x^d)) for the raw downsample branch yd
// Three launches, memory-bound, no MFMA, no atomics, no hand-off between workgroups inside a launch:
//   k_nb_partial   one workgroup per (image, chunk of pixels): sum q, sum q x^ (and sum q x^d) per channel over the chunk.  The
//                  thread layout is emb::chan_layout (emb_host.h, the forward tail's too): C / 4 channel groups across the threads,
//                  16-byte loads, 256 / (C / 4) pixel lanes; a thread adds its pixels serially (fmaf for the products), the pixel
//                  lanes of a wave are combined by xor shuffles (widest stride last), the waves through LDS in wave order -> ws
//                  partials
//   k_nb_finish    one thread per (sum, image, channel): the partials in chunk order, divided by HW -> ws coefficients
//   k_nb_apply     the element pass on emb::chan_grid, the forward tail's grid (a cap on the workgroups, a grid stride beyond, a
//                  thread keeps its channel group, 32-bit indices)
// Every output element has one writer and every sum a fixed order: two calls on the same inputs are bit-identical, and a call
// reads nothing from ws that it has not written itself.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dsmil_hip.h"
#include "emb_host.h"

namespace {
using namespace emb;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct NbArgs {
    const float *g, *out, *y, *mean, *rstd, *yd, *md, *rd;
    float *gy, *gyd, *gres;
    float *part, *coef;          // ws: partials [nsums][B][n_partials][C], coefficients [nsums][B][C]
    int B, HW, C, chunk, nparts;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 xor4(f32x4 v, int m) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __shfl_xor(v[e], m, 64);
    return o;
}

// sums[0] = sum q, sums[1] = sum q x^, sums[2] = sum q x^d (ADD_DOWN) over the pixels of chunk blockIdx.x % nparts of image
// blockIdx.x / nparts
template <int KIND>
__global__ __launch_bounds__(256) void k_nb_partial(const NbArgs a) {
    constexpr int NS = KIND == DSMIL_NORM_BWD_ADD_DOWN ? 3 : 2;
    __shared__ f32x4 red[NS][256];
    // emb::chan_layout(C), written out: taking it from the struct changes this kernel's instruction stream (k_nb_apply's and
    // k_norm_add_relu's it leaves alone), and the refactor that introduced emb_host.h was to change no device code
    const int C = a.C, c4n = C / 4;
    const int lanes_c = c4n < 256 ? c4n : 256;              // threads across the channel groups of one pixel
    const int cpt = (c4n + 255) / 256;                      // channel groups per thread (2 at C = 2048)
    const int tpb = 256 / lanes_c;                          // pixel lanes
    const int tid = threadIdx.x, c40 = tid % lanes_c, pl = tid / lanes_c;
    const int n = blockIdx.x / a.nparts, k = blockIdx.x % a.nparts;
    const int p0 = k * a.chunk, p1 = min(a.HW, p0 + a.chunk);
    // rows of the LDS step: a wave narrower than a pixel row of channel groups holds 64 / lanes_c pixel lanes, shuffled first
    const bool shuf = lanes_c < 64;
    const int rows = shuf ? 4 : tpb, row = shuf ? tid / 64 : pl;
    for (int j = 0; j < cpt; ++j) {
        const int c4 = c40 + 256 * j;
        const unsigned sc = (unsigned)n * C + c4 * 4;
        const f32x4 mu = ld4(a.mean + sc), rs = ld4(a.rstd + sc);
        f32x4 mud = {0.f, 0.f, 0.f, 0.f}, rsd = mud;
        if constexpr (NS == 3) {
            mud = ld4(a.md + sc);
            rsd = ld4(a.rd + sc);
        }
        f32x4 s[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) s[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int p = p0 + pl; p < p1; p += tpb) {
            const unsigned o = ((unsigned)n * a.HW + p) * (unsigned)C + c4 * 4;
            const f32x4 gv = ld4(a.g + o), yv = ld4(a.y + o);
            f32x4 ov, ydv;
            if constexpr (KIND != DSMIL_NORM_BWD_RELU) ov = ld4(a.out + o);
            if constexpr (NS == 3) ydv = ld4(a.yd + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (yv[e] - mu[e]) * rs[e];
                const float q = (KIND == DSMIL_NORM_BWD_RELU ? xh > 0.f : ov[e] > 0.f) ? gv[e] : 0.f;
                s[0][e] += q;
                s[1][e] = __fmaf_rn(q, xh, s[1][e]);
                if constexpr (NS == 3) s[2][e] = __fmaf_rn(q, (ydv[e] - mud[e]) * rsd[e], s[2][e]);
            }
        }
        if (shuf) {
            for (int m = lanes_c; m < 64; m <<= 1) {
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const f32x4 t = xor4(s[i], m);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[i][e] += t[e];
                }
            }
        }
        if (j) __syncthreads();                             // the readers of the round before are done
        if (!shuf || (tid & 63) < lanes_c) {
#pragma unroll
            for (int i = 0; i < NS; ++i) red[i][row * lanes_c + c40] = s[i];
        }
        __syncthreads();
        if (tid < lanes_c) {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
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

__global__ __launch_bounds__(256) void k_nb_finish(const float* __restrict__ part, float* __restrict__ coef, int rows, int C,
                                                   int nparts, float hw) {
    const unsigned total = (unsigned)rows * C;              // rows = nsums B
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned r = i / (unsigned)C, c = i % (unsigned)C;
        float s = part[(r * nparts) * (unsigned)C + c];
        for (int k = 1; k < nparts; ++k) s += part[(r * nparts + k) * (unsigned)C + c];
        coef[i] = s / hw;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_nb_apply(const NbArgs a) {
    constexpr bool DOWN = KIND == DSMIL_NORM_BWD_ADD_DOWN;
    const int C = a.C;
    const ChanLayout cl = chan_layout(C);
    const int lanes_c = cl.lanes_c, cpt = cl.cpt, tpb = cl.tpb;
    const int c40 = threadIdx.x % lanes_c, pl = threadIdx.x / lanes_c;
    const unsigned np = (unsigned)a.B * (unsigned)a.HW, pstep = gridDim.x * (unsigned)tpb, bc = (unsigned)a.B * C;
    int ncur = -1;
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, rs = mu, mq = mu, mqx = mu, mud = mu, rsd = mu, mqd = mu;
    for (unsigned p = blockIdx.x * (unsigned)tpb + pl; p < np; p += pstep) {
        const int n = (int)(p / (unsigned)a.HW);
        for (int j = 0; j < cpt; ++j) {
            const int c4 = c40 + 256 * j;
            const unsigned o = p * (unsigned)C + c4 * 4;
            const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.g + o));
            const f32x4 yv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.y + o));
            f32x4 ov, ydv;
            if constexpr (KIND != DSMIL_NORM_BWD_RELU) ov = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.out + o));
            if constexpr (DOWN) ydv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.yd + o));
            if (n != ncur || cpt > 1) {                     // the image changes every HW pixels: reload its statistics and means
                const unsigned sc = (unsigned)n * C + c4 * 4;
                mu = ld4(a.mean + sc);
                rs = ld4(a.rstd + sc);
                mq = ld4(a.coef + sc);
                mqx = ld4(a.coef + bc + sc);
                if constexpr (DOWN) {
                    mud = ld4(a.md + sc);
                    rsd = ld4(a.rd + sc);
                    mqd = ld4(a.coef + 2 * bc + sc);
                }
            }
            f32x4 o1, o2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (yv[e] - mu[e]) * rs[e];
                const float q = (KIND == DSMIL_NORM_BWD_RELU ? xh > 0.f : ov[e] > 0.f) ? gv[e] : 0.f;
                const float d = q - mq[e];
                o1[e] = rs[e] * __fmaf_rn(-xh, mqx[e], d);
                if constexpr (DOWN) o2[e] = rsd[e] * __fmaf_rn(-((ydv[e] - mud[e]) * rsd[e]), mqd[e], d);
                else o2[e] = q;
            }
            *reinterpret_cast<f32x4*>(a.gy + o) = o1;
            if constexpr (DOWN) *reinterpret_cast<f32x4*>(a.gyd + o) = o2;
            if constexpr (KIND == DSMIL_NORM_BWD_ADD) *reinterpret_cast<f32x4*>(a.gres + o) = o2;
        }
        ncur = n;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
using NbPlan = SumPlan;                                       // (emb_host.h: the chunk rule stem_bwd.hip shares)

int nb_check(int kind, int B, int HW, int C) {
    if (B < 1 || HW < 1 || C < 1) return DSMIL_E_INVALID;
    if (kind != DSMIL_NORM_BWD_RELU && kind != DSMIL_NORM_BWD_ADD && kind != DSMIL_NORM_BWD_ADD_DOWN) return DSMIL_E_INVALID;
    if (!chan_ok(C) || C > 2048) return DSMIL_E_UNSUPPORTED;     // the layout the forward tail takes too; C <= 2048 is this entry's own limit
    if (!map_fits(B, HW, 1, C)) return DSMIL_E_UNSUPPORTED;
    return DSMIL_OK;
}

// the shape has passed nb_check.  false: the partials would not fit a 32-bit index (refused as unsupported)
bool nb_plan(int kind, int B, int HW, int C, NbPlan& p) { return sum_plan(kind == DSMIL_NORM_BWD_ADD_DOWN ? 3 : 2, B, HW, C, p); }

}  // namespace

extern "C" {

int dsmil_norm_bwd_plan(int32_t kind, int32_t B, int32_t HW, int32_t C, int32_t out[16]) {
    if (!out) return DSMIL_E_INVALID;
    if (const int rc = nb_check(kind, B, HW, C)) return rc;
    NbPlan p;
    if (!nb_plan(kind, B, HW, C, p)) return DSMIL_E_UNSUPPORTED;
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[DSMIL_NORM_BWD_PLAN_KIND] = kind;
    out[DSMIL_NORM_BWD_PLAN_CHUNK] = p.chunk;
    out[DSMIL_NORM_BWD_PLAN_PARTIALS] = p.nparts;
    out[DSMIL_NORM_BWD_PLAN_RUN_LEN] = p.run_len;
    out[DSMIL_NORM_BWD_PLAN_LANES] = p.lanes;
    out[DSMIL_NORM_BWD_PLAN_SUMS] = p.nsums;
    out[DSMIL_NORM_BWD_PLAN_GRID_PARTIAL] = p.grid_partial;
    out[DSMIL_NORM_BWD_PLAN_GRID_FINISH] = p.grid_finish;
    out[DSMIL_NORM_BWD_PLAN_GRID_APPLY] = p.grid_apply;
    out[DSMIL_NORM_BWD_PLAN_BLOCK] = 256;
    out[DSMIL_NORM_BWD_PLAN_GROUPS] = p.cpt;
    return DSMIL_OK;
}

size_t dsmil_norm_bwd_workspace_bytes(int32_t kind, int32_t B, int32_t HW, int32_t C) {
    if (nb_check(kind, B, HW, C)) return 0;
    NbPlan p;
    return nb_plan(kind, B, HW, C, p) ? p.total : 0;
}

int dsmil_norm_bwd(int32_t kind, const float* g, const float* out, const float* y, const float* mean, const float* rstd,
                   const float* yd, const float* md, const float* rd, float* gy, float* gyd, float* gres, int32_t B, int32_t HW,
                   int32_t C, void* ws, size_t ws_bytes, void* stream) {
    if (kind != DSMIL_NORM_BWD_RELU && kind != DSMIL_NORM_BWD_ADD && kind != DSMIL_NORM_BWD_ADD_DOWN) return DSMIL_E_INVALID;
    if (B < 1 || HW < 1 || C < 1 || !g || !y || !mean || !rstd || !gy || !ws) return DSMIL_E_INVALID;
    const bool relu = kind == DSMIL_NORM_BWD_RELU, down = kind == DSMIL_NORM_BWD_ADD_DOWN;
    if (relu ? out != nullptr : out == nullptr) return DSMIL_E_INVALID;
    if (down ? (!yd || !md || !rd || !gyd) : (yd || md || rd || gyd)) return DSMIL_E_INVALID;
    if (kind == DSMIL_NORM_BWD_ADD ? gres == nullptr : gres != nullptr) return DSMIL_E_INVALID;
    {
        // no output may share a byte with an input or with another output (sizes saturate: such a shape is refused below anyway)
        const unsigned __int128 nb128 = (unsigned __int128)B * HW * C * sizeof(float);
        const size_t nb = nb128 > ((size_t)1 << 62) ? (size_t)1 << 62 : (size_t)nb128;
        const size_t sb = (size_t)B * C * sizeof(float);
        const float* outs[3] = {gy, gyd, gres};
        const float* maps[4] = {g, out, y, yd};
        const float* stats[4] = {mean, rstd, md, rd};
        for (int i = 0; i < 3; ++i) {
            if (!outs[i]) continue;
            for (int j = 0; j < 4; ++j) {
                if (maps[j] && overlap(outs[i], nb, maps[j], nb)) return DSMIL_E_INVALID;
                if (stats[j] && overlap(outs[i], nb, stats[j], sb)) return DSMIL_E_INVALID;
            }
            for (int j = i + 1; j < 3; ++j)
                if (outs[j] && overlap(outs[i], nb, outs[j], nb)) return DSMIL_E_INVALID;
        }
    }
    if (const int rc = nb_check(kind, B, HW, C)) return rc;
    NbPlan p;
    if (!nb_plan(kind, B, HW, C, p)) return DSMIL_E_UNSUPPORTED;
    if (!al16(g) || !al16(out) || !al16(y) || !al16(mean) || !al16(rstd) || !al16(yd) || !al16(md) || !al16(rd) || !al16(gy) ||
        !al16(gyd) || !al16(gres) || !al256p(ws)) return DSMIL_E_ALIGN;
    if (ws_bytes < p.total) return DSMIL_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    float* coef = (float*)((char*)ws + p.off_coef);
    const NbArgs a{g, out, y, mean, rstd, yd, md, rd, gy, gyd, gres, part, coef, B, HW, C, p.chunk, p.nparts};
    const dim3 gp(p.grid_partial), ga(p.grid_apply), blk(256);
    if (relu) hipLaunchKernelGGL(k_nb_partial<DSMIL_NORM_BWD_RELU>, gp, blk, 0, st, a);
    else if (down) hipLaunchKernelGGL(k_nb_partial<DSMIL_NORM_BWD_ADD_DOWN>, gp, blk, 0, st, a);
    else hipLaunchKernelGGL(k_nb_partial<DSMIL_NORM_BWD_ADD>, gp, blk, 0, st, a);
    hipLaunchKernelGGL(k_nb_finish, dim3(p.grid_finish), blk, 0, st, (const float*)part, coef, p.nsums * B, C, p.nparts, (float)HW);
    if (relu) hipLaunchKernelGGL(k_nb_apply<DSMIL_NORM_BWD_RELU>, ga, blk, 0, st, a);
    else if (down) hipLaunchKernelGGL(k_nb_apply<DSMIL_NORM_BWD_ADD_DOWN>, ga, blk, 0, st, a);
    else hipLaunchKernelGGL(k_nb_apply<DSMIL_NORM_BWD_ADD>, ga, blk, 0, st, a);
    return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH;
}

}  // extern "C"
