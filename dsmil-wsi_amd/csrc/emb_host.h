// The shape rules that the embedder's host code shares, each stated once ("The shared host rules"): used by
// resnet_fwd.hip (resnet_b16.h's host part and both stage-entry families included), conv_bwd.hip, norm_bwd.hip and stem_bwd.hip.  No kernels
// live here; chan_layout alone is also callable from device code, so that the kernels of the channel-group layout and the
// launches that size their grids read one definition.  Include after <hip/hip_runtime.h>.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace emb {

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }       // (a null pointer passes: optional arguments)
inline bool al256p(const void* p) { return ((uintptr_t)p & 255) == 0; }

// [p, p + bytes) and [q, q + qbytes) share a byte
inline bool overlap(const void* p, size_t bytes, const void* q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b ? b - a < bytes : a - b < qbytes;
}

// an NHWC map whose element offsets fit the kernels' 32-bit index arithmetic (the product cannot overflow here)
inline bool map_fits(int B, int H, int W, int C) { return (__int128)B * H * W * C < 0x7fffffffLL; }

inline int outdim(int x, int ks, int s, int p) { return (x + 2 * p - ks) / s + 1; }

// The output map of a conv, and what every conv family asks of a shape before its own conditions: at least one output pixel,
// the input and the output map each inside 2^31 elements.  Arguments are positive (pad >= 0); false = refuse as unsupported.
struct ConvMap { int Ho, Wo; };
inline bool conv_map(int B, int H, int W, int Cin, int Cout, int ks, int stride, int pad, ConvMap& m) {
    if ((long long)H + 2LL * pad < ks || (long long)W + 2LL * pad < ks) return false;
    m.Ho = (int)(((long long)H + 2LL * pad - ks) / stride + 1);
    m.Wo = (int)(((long long)W + 2LL * pad - ks) / stride + 1);
    return map_fits(B, H, W, Cin) && map_fits(B, m.Ho, m.Wo, Cout);
}

// The channel-group thread layout of the elementwise passes over an fp32 NHWC map (k_norm_add_relu, k_nb_partial, k_nb_apply):
// 256 threads = lanes_c channel groups of four (16-byte accesses) x tpb pixel lanes; a thread keeps its channel group(s) while
// it strides over pixels, cpt of them where C / 4 > 256.
struct ChanLayout { int lanes_c, cpt, tpb; };
__host__ __device__ inline ChanLayout chan_layout(int C) {
    const int c4n = C / 4;
    ChanLayout l;
    l.lanes_c = c4n < 256 ? c4n : 256;                      // threads across the channel groups of one pixel
    l.cpt = (c4n + 255) / 256;                              // channel groups per thread (2 at C = 2048)
    l.tpb = 256 / l.lanes_c;                                // pixels per workgroup per iteration
    return l;
}
// the layout exists: C / 4 divides 256 or is a multiple of it
inline bool chan_ok(int C) { return C >= 4 && C % 4 == 0 && (C / 4 < 256 ? 256 % (C / 4) == 0 : (C / 4) % 256 == 0); }
// workgroups of an element pass over npix pixels: one iteration each up to the cap, a grid stride beyond it
constexpr int CHAN_GRID_MAX = 8192;
inline int chan_grid(long long npix, const ChanLayout& l) {
    const long long nb = (npix + l.tpb - 1) / l.tpb;
    return (int)(nb < CHAN_GRID_MAX ? nb : CHAN_GRID_MAX);
}

// The plan of the per-(image, channel) sums over HW pixels and the element pass behind them (norm_bwd.hip, stem_bwd.hip): chunks
// of 256 pixels, doubled up to 4096 while B x chunks exceeds 2048 workgroups; in a chunk `lanes` accumulators per channel add at
// most run_len terms each; nsums sums per (n, c).  ws: partials [nsums][B][nparts][C], then coefficients [nsums][B][C] at
// off_coef.  B HW C < 2^31 and chan_ok(C) hold.  false: the partials would not fit a 32-bit index (refuse as unsupported)
struct SumPlan {
    int nsums, chunk, nparts, run_len, lanes, cpt, grid_partial, grid_finish, grid_apply;
    size_t off_coef, total;
};
inline bool sum_plan(int nsums, int B, int HW, int C, SumPlan& p) {
    constexpr int CHUNK0 = 256, CHUNK_MAX = 4096, WG_TARGET = 2048;
    p.nsums = nsums;
    const ChanLayout cl = chan_layout(C);
    p.lanes = cl.tpb;
    p.cpt = cl.cpt;
    p.chunk = CHUNK0;
    auto nch = [&](int c) { return (long long)(HW + c - 1) / c; };
    while (nch(p.chunk) * B > WG_TARGET && p.chunk < CHUNK_MAX) p.chunk *= 2;
    p.nparts = (int)nch(p.chunk);
    if (3LL * B * p.nparts * C >= 0x7fffffffLL) return false;
    const int len = HW < p.chunk ? HW : p.chunk;
    p.run_len = (len + p.lanes - 1) / p.lanes;
    p.grid_partial = B * p.nparts;                           // <= B HW < 2^31
    const long long nfin = ((long long)nsums * B * C + 255) / 256;
    p.grid_finish = (int)(nfin < 4096 ? nfin : 4096);
    p.grid_apply = chan_grid((long long)B * HW, cl);
    p.off_coef = al256((size_t)nsums * B * p.nparts * C * sizeof(float));
    p.total = p.off_coef + al256((size_t)nsums * B * C * sizeof(float));
    return true;
}

}  // namespace emb
