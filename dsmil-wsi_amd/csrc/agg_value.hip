// The value layer of BClassifier(passing_v=True), dsmil.py:35-39,48 — hand-written HIP for gfx950 (MI355X, CDNA4).
//
//   V = ReLU(x Wv^T + bv)                      dsmil_value_forward[_bf16]        k_value_proj[_b16] (wide K: *_valu)
//   g_Wv = gZ^T x, g_bv = colsum gZ            dsmil_value_backward[_bf16]       k_value_tn[_b16], k_value_reduce
//   g_x (+)= gZ Wv        gZ = g_vals o [V>0]  dsmil_value_backward_rows         k_value_gx
// The kernels are agg_value.h's (k_value_gx: agg_gx.h's tile body); this unit is the host code behind every dsmil_value_*
// entry and uses nothing of the aggregator's.  fp32 and bf16-stored rows share ONE host path per direction:
//   value_forward_impl<XT>   refusals, wide-K kernel, image (the caller's, or cut into ws), kernel pick, LDS opt-in, launch;
//                            what differs per dtype is ValueFwd<XT> below
//   vtn_launch(args, ...)    plan -> grid bound -> k_value_tn / k_value_tn_b16 -> k_value_reduce, over VtnArgs / VtnB16Args
//   vp_ws_layout             one workspace layout; the fp32 one keeps room for the forward's image in front
// The ORDER of an entry's refusals is part of its behaviour (tests/test_value_sizes_cabi.py pins it); where the two dtypes
// differ in it (the backwards), each entry keeps its own.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dsmil_hip.h"
#include "agg_common.h"
#include "agg_value.h"
#include "lds_attr.h"

namespace {

inline int launched() { return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH; }

// ---- the forward's per-dtype facts: refusal, image, pack entry, tile rows, LDS bytes, kernel table, the two launches ----
template <typename XT> struct ValueFwd;

template <> struct ValueFwd<float> {     // any K and Kv, 4-B alignment, row map
    using Kernel = void (*)(const float*, const int64_t*, const f32x4*, const float*, float*, long long, int, int, int);
    static int refuse(const float*, const float*, int, int) { return DSMIL_OK; }
    static size_t image_bytes(int K, int Kv) { return vp_image_bytes(K, Kv); }
    static constexpr auto pack = dsmil_value_pack;
    static int tile_rows(int K) { return K <= 512 ? 64 : 32; }                                        // RG = 2 | 1
    static int lds_bytes(int K) { return vp_nks(K) * 4 * tile_rows(K) * 16 + tile_rows(K) * 4; }
    static int vec(const float* x, int K) { return (K % 4 == 0) && ((uintptr_t)x % 16 == 0); }
    static Kernel kernel(const float* x, int K) {
        const bool full = vec(x, K) && K % 32 == 0;
        if (K > 512) return full ? k_value_proj<1, 0, true> : k_value_proj<1, 0, false>;
        return full ? (vp_nks(K) == 32 ? k_value_proj<2, 32, true> : k_value_proj<2, 0, true>) : k_value_proj<2, 0, false>;
    }
    static void launch(Kernel fn, dim3 grid, int lds, hipStream_t st, const float* x, const int64_t* row_map, const void* image,
                       const float* v_b, float* V, long long rows, int K, int Kv) {
        hipLaunchKernelGGL(fn, grid, dim3(VP_THREADS), lds, st, x, row_map, (const f32x4*)image, v_b, V, rows, K, Kv, vec(x, K));
    }
    static void launch_wide(dim3 grid, hipStream_t st, const float* x, const int64_t* row_map, const float* v_w,
                            const float* v_b, float* V, long long rows, int K, int Kv) {
        hipLaunchKernelGGL(k_value_proj_valu, grid, dim3(256), 0, st, x, row_map, v_w, v_b, V, rows, K, Kv);
    }
};

template <> struct ValueFwd<bf16_t> {    // K % 8 == 0, Kv % 4 == 0, 16-B aligned rows, no row map
    using Kernel = void (*)(const bf16_t*, const f32x4*, const float*, bf16_t*, long long, int, int);
    static int refuse(const bf16_t* x, const bf16_t* V, int K, int Kv) {
        if ((K % 8) || (Kv % 4)) return DSMIL_E_UNSUPPORTED;
        return (((uintptr_t)x % 16) || ((uintptr_t)V % 4)) ? DSMIL_E_ALIGN : DSMIL_OK;
    }
    static size_t image_bytes(int K, int Kv) { return vb_image_bytes(K, Kv); }
    static constexpr auto pack = dsmil_value_pack_bf16;
    static int tile_rows(int) { return VB_BM; }
    static int lds_bytes(int K) { return 2 * vp_nks(K) * VB_BM * 16; }
    static Kernel kernel(const bf16_t*, int K) {
        if (K % 64) return k_value_proj_b16<0, false>;
        return vp_nks(K) == 32 ? k_value_proj_b16<32, true> : k_value_proj_b16<0, true>;
    }
    static void launch(Kernel fn, dim3 grid, int lds, hipStream_t st, const bf16_t* x, const int64_t*, const void* image,
                       const float* v_b, bf16_t* V, long long rows, int K, int Kv) {
        hipLaunchKernelGGL(fn, grid, dim3(VP_THREADS), lds, st, x, (const f32x4*)image, v_b, V, rows, K, Kv);
    }
    static void launch_wide(dim3 grid, hipStream_t st, const bf16_t* x, const int64_t*, const float* v_w, const float* v_b,
                            bf16_t* V, long long rows, int K, int Kv) {
        hipLaunchKernelGGL(k_value_proj_b16_valu, grid, dim3(256), 0, st, x, v_w, v_b, V, rows, K, Kv);
    }
};
static_assert(VP_MAX_K == VB_MAX_K, "one wide-K threshold for both dtypes");

template <typename XT>
int value_forward_impl(const XT* x, long long rows, int K, int Kv, const float* v_w, const float* v_b, const void* image,
                       const int64_t* row_map, XT* V, void* ws, size_t ws_bytes, void* stream) {
    using F = ValueFwd<XT>;
    if (!x || !v_w || !v_b || !V || rows <= 0 || K <= 0 || Kv <= 0) return DSMIL_E_INVALID;
    if (const int rc = F::refuse(x, V, K, Kv)) return rc;
    if (rows * (int64_t)Kv / 256 + 1 > 0x7fffffffLL) return DSMIL_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (K > VP_MAX_K) {   // plain kernel: reads v_w itself, needs neither image nor workspace
        F::launch_wide(dim3((unsigned)((rows * Kv + 255) / 256)), st, x, row_map, v_w, v_b, V, rows, K, Kv);
        return launched();
    }
    const bool cut = !image;   // cut Wv into the workspace first (a caller with fixed weights packs once: dsmil_value_pack*)
    if (cut) {
        if (!ws) return DSMIL_E_INVALID;
        if ((uintptr_t)ws % 256) return DSMIL_E_ALIGN;
        if (ws_bytes < F::image_bytes(K, Kv)) return DSMIL_E_WORKSPACE;
        image = ws;
    }
    // Resolve, check, THEN pack, for both dtypes.  The fp32 entry used to pack before this check; an image it cut itself is the
    // 256-B aligned workspace, which the check cannot refuse, so the order is not observable.
    if ((uintptr_t)image % 16) return DSMIL_E_ALIGN;
    if (cut)
        if (const int rc = F::pack(v_w, K, Kv, ws, stream)) return rc;
    const auto fn = F::kernel(x, K);
    const int lds = F::lds_bytes(K), tr = F::tile_rows(K);
    if (!dsmil_lds::allow((const void*)fn, lds)) return DSMIL_E_LAUNCH;
    F::launch(fn, dim3((unsigned)((rows + tr - 1) / tr)), lds, st, x, row_map, image, v_b, V, rows, K, Kv);
    return launched();
}

// ---- the parameter gradients: plan -> grid bound -> contraction over the row ranges -> fixed-order reduce ----
inline auto vtn_kernel(const VtnArgs&) { return k_value_tn; }
inline auto vtn_kernel(const VtnB16Args&) { return k_value_tn_b16; }

// fills the plan fields of `a` from its N, K, Kv; returns the workgroups of the contraction
template <typename Args>
long long vtn_grid(Args& a) {
    vtn_plan(a.N, a.K, a.Kv, a.S, a.R);
    a.nsk = (a.K + 63) / 64; a.nsu = (a.Kv + 127) / 128;
    return (long long)a.nsk * a.nsu * a.S;
}

template <typename Args>
int vtn_launch(Args a, float* g_v_w, float* g_v_b, hipStream_t st) {
    const long long wgs = vtn_grid(a);
    if (wgs > 0x7fffffffLL) return DSMIL_E_UNSUPPORTED;
    hipLaunchKernelGGL(vtn_kernel(a), dim3((unsigned)wgs), dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) return DSMIL_E_LAUNCH;
    const long long n = (long long)a.Kv * a.K + a.Kv;
    hipLaunchKernelGGL(k_value_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.part, a.pb, g_v_w, g_v_b, a.K, a.Kv, a.S);
    return launched();
}

// the operands of either contraction; the partials at their place in ws
template <typename Args, typename XT>
Args vtn_args(const float* g_vals, const XT* V, const XT* x, long long rows, int K, int Kv, void* ws, const VpWs& L) {
    Args a{};
    a.G = g_vals; a.V = V; a.X = x;
    a.part = (float*)((char*)ws + L.part); a.pb = (float*)((char*)ws + L.pb);
    a.N = rows; a.K = K; a.Kv = Kv;
    return a;
}

}  // namespace

extern "C" {

// ---- the weight images (fp32 rows: two scaled fp16 planes, k_pack_value; bf16 rows: one bf16 plane, k_pack_value_b16) ----
size_t dsmil_value_packed_bytes(int32_t K, int32_t Kv) { return (K <= 0 || Kv <= 0) ? 0 : vp_image_bytes(K, Kv); }
size_t dsmil_value_packed_bf16_bytes(int32_t K, int32_t Kv) { return (K <= 0 || Kv <= 0) ? 0 : vb_image_bytes(K, Kv); }

int dsmil_value_pack(const float* v_w, int32_t K, int32_t Kv, void* packed, void* stream) {
    if (!v_w || !packed || K <= 0 || Kv <= 0) return DSMIL_E_INVALID;
    if ((uintptr_t)packed % 16) return DSMIL_E_ALIGN;
    hipLaunchKernelGGL(k_pack_value, dim3(256), dim3(256), 0, (hipStream_t)stream, v_w, (_Float16*)packed, K, Kv, vp_nks(K),
                       vp_ntp(Kv));
    return launched();
}

int dsmil_value_pack_bf16(const float* v_w, int32_t K, int32_t Kv, void* packed, void* stream) {
    if (!v_w || !packed || K <= 0 || Kv <= 0) return DSMIL_E_INVALID;
    if ((uintptr_t)packed % 16) return DSMIL_E_ALIGN;
    hipLaunchKernelGGL(k_pack_value_b16, dim3(256), dim3(256), 0, (hipStream_t)stream, v_w, (bf16_t*)packed, K, Kv, vp_nks(K),
                       vp_ntp(Kv));
    return launched();
}

// ---- the forward ----
int dsmil_value_forward(const float* feats, int64_t rows, int32_t K, int32_t Kv, const float* v_w, const float* v_b,
                        const void* packed, const int64_t* row_map, float* V_out, void* ws, size_t ws_bytes, void* stream) {
    return value_forward_impl<float>(feats, rows, K, Kv, v_w, v_b, packed, row_map, V_out, ws, ws_bytes, stream);
}

size_t dsmil_value_workspace_bf16_bytes(int64_t rows, int32_t K, int32_t Kv) {
    if (rows <= 0 || K <= 0 || Kv <= 0 || K > VB_MAX_K) return 0;   // (the plain kernel of wider rows reads v_w itself)
    return vp_al(vb_image_bytes(K, Kv));
}

int dsmil_value_forward_bf16(const void* feats_bf16, int64_t rows, int32_t K, int32_t Kv, const float* v_w, const float* v_b,
                             const void* packed, void* V_out_bf16, void* ws, size_t ws_bytes, void* stream) {
    return value_forward_impl<bf16_t>((const bf16_t*)feats_bf16, rows, K, Kv, v_w, v_b, packed, nullptr, (bf16_t*)V_out_bf16, ws,
                                      ws_bytes, stream);
}

// ---- the parameter gradients: what autograd derives for dsmil.py:39 behind g_vals ----
size_t dsmil_value_workspace_bytes(int64_t rows, int32_t K, int32_t Kv) {   // (the fp32 forward's too: its image leads)
    if (rows <= 0 || K <= 0 || Kv <= 0) return 0;
    return vp_ws_layout(rows, K, Kv, vp_image_bytes(K, Kv)).total;
}

size_t dsmil_value_backward_bf16_workspace_bytes(int64_t rows, int32_t K, int32_t Kv) {
    if (rows <= 0 || K <= 0 || Kv <= 0) return 0;
    return vp_ws_layout(rows, K, Kv, 0).total;
}

int dsmil_value_backward(const float* feats, const float* V, const float* g_vals, int64_t rows, int32_t K, int32_t Kv,
                         const int64_t* row_map, float* g_v_w, float* g_v_b, void* ws, size_t ws_bytes, void* stream) {
    if (!feats || !V || !g_vals || !g_v_w || !g_v_b || !ws || rows <= 0 || K <= 0 || Kv <= 0) return DSMIL_E_INVALID;
    if ((uintptr_t)ws % 256) return DSMIL_E_ALIGN;
    const VpWs L = vp_ws_layout(rows, K, Kv, vp_image_bytes(K, Kv));
    if (ws_bytes < L.total) return DSMIL_E_WORKSPACE;
    VtnArgs a = vtn_args<VtnArgs>(g_vals, V, feats, rows, K, Kv, ws, L);
    a.rowmap = row_map;
    return vtn_launch(a, g_v_w, g_v_b, (hipStream_t)stream);   // (the grid bound comes last in this entry)
}

int dsmil_value_backward_bf16(const void* feats_bf16, const void* V_bf16, const float* g_vals, int64_t rows, int32_t K,
                              int32_t Kv, float* g_v_w, float* g_v_b, void* ws, size_t ws_bytes, void* stream) {
    if (!feats_bf16 || !V_bf16 || !g_vals || !g_v_w || !g_v_b || !ws || rows <= 0 || K <= 0 || Kv <= 0) return DSMIL_E_INVALID;
    if (K % 8 || Kv % 4) return DSMIL_E_UNSUPPORTED;
    VtnB16Args plan{};
    plan.N = rows; plan.K = K; plan.Kv = Kv;
    if (vtn_grid(plan) > 0x7fffffffLL) return DSMIL_E_UNSUPPORTED;   // (this entry bounds the grid BEFORE alignment and size)
    if ((uintptr_t)feats_bf16 % 16 || (uintptr_t)V_bf16 % 8 || (uintptr_t)g_vals % 16 || (uintptr_t)ws % 256) return DSMIL_E_ALIGN;
    const VpWs L = vp_ws_layout(rows, K, Kv, 0);
    if (ws_bytes < L.total) return DSMIL_E_WORKSPACE;
    return vtn_launch(vtn_args<VtnB16Args>(g_vals, (const bf16_t*)V_bf16, (const bf16_t*)feats_bf16, rows, K, Kv, ws, L), g_v_w,
                      g_v_b, (hipStream_t)stream);
}

// ---- the gradient of the input rows ----
int dsmil_value_backward_rows(const float* feats, const float* V, const float* g_vals, int64_t rows, int32_t K, int32_t Kv,
                              const float* v_w, const void* packed, int32_t accumulate, float* g_feats, void* ws,
                              size_t ws_bytes, void* stream) {
    (void)feats; (void)packed; (void)ws_bytes;   // the product reads neither the rows nor the forward's image (agg_gx.h)
    if (!V || !g_vals || !v_w || !g_feats || rows <= 0 || K <= 0 || Kv <= 0) return DSMIL_E_INVALID;
    if (ws && ((uintptr_t)ws % 256)) return DSMIL_E_ALIGN;
    GxArgs gx{};
    gx.L = g_vals; gx.V = V; gx.W = v_w; gx.out = g_feats; gx.N = rows; gx.J = Kv; gx.K = K;
    gx.accumulate = accumulate ? 1 : 0;
    gx.lvec = (Kv % 4 == 0) && (((uintptr_t)g_vals | (uintptr_t)V) % 16 == 0);
    if (!gx_launch<true>(gx, (hipStream_t)stream)) return DSMIL_E_UNSUPPORTED;
    return launched();
}

}  // extern "C"
