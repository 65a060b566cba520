// SimCLR's two-view augmentation on decoded tiles (include/dsmil_hip.h, dsmil_simclr_views): the reference's PIL / OpenCV chain
// (simclr/data_aug/dataset_wrapper.py:48-58) on uint8 RGB, stage by stage, one workgroup per view.
//
// The arithmetic of every stage lives in the __host__ __device__ functions of the first half of this file (sv_*): the kernel
// and dsmil_simclr_views_host are two loop nests around the same functions, so what the host form matches against Pillow on a
// machine without a GPU is what the device computes.  Pillow's float code is plain C without fused multiply-adds; this
// translation unit is compiled with contraction off so that neither side fuses what Pillow rounds twice.
//
// Kernel form: a persistent grid of up to SV_SLOTS workgroups of 1024 threads, workgroup b takes views b, b + grid, ...
//   * S <= 224 ("resident"): the view, S x S x 3 bytes, lives in LDS from the vertical resample pass to the output store
//     (150 528 B at S = 224) beside the two coefficient tables (10 240 B), their bounds (2 048 B) and the blur's weights —
//     162 896 B of the CU's 163 840.
//   * S > 224: the view does not fit; it lives in the workgroup's workspace slot instead (same code, global pointer).
//   The horizontal pass's uint8 intermediate (h x S x 3, h up to 256 rows: as large as the view itself) goes through the
//   workgroup's workspace slot in both forms: written and read back by the same workgroup, it stays in L2.
//   The blur reads the finished view and writes the output directly: a thread walks a segment of one column and keeps the
//   fp32 row sums of its vertical window in registers (sv_blur_column), so there is no float intermediate in memory and
//   every sum runs in the host's order (w[0] first): both sides agree bit for bit.  Both instantiations sit at the 128 VGPRs
//   that 1024-thread workgroups allow (DESIGN.md has the figures); sv_blur_column is written around that ceiling.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dsmil_hip.h"
#include "lds_attr.h"

#pragma clang fp contract(off)

#define SV_HD __host__ __device__ __forceinline__

namespace {

constexpr int SV_THREADS = 1024;
constexpr int SV_SLOTS = 512;         // workgroups of the persistent grid = workspace slots
constexpr int SV_MAXCOEF = 1280;      // >= S * ksize for every supported shape: S (2 ceil(256 / S) + 1) <= 512 + 3 S
constexpr int SV_MAXDIM = 256;
constexpr int SV_RES_MAX_S = 224;     // the largest view that is LDS-resident
constexpr int SV_AUX_BYTES = 2 * SV_MAXCOEF * 4 + 2 * SV_MAXDIM * 2 * 2 + 16 * 4 + 4 * 4;
constexpr int SV_PRECISION_BITS = 32 - 8 - 2;

SV_HD int sv_blur_ksize(int S) { return (int)(0.06 * S); }

SV_HD bool sv_shape_ok(int H, int W, int S) {
    if (H < 8 || W < 8 || H > SV_MAXDIM || W > SV_MAXDIM || S < 17 || S > SV_MAXDIM) return false;
    return (sv_blur_ksize(S) & 1) == 1;
}

SV_HD bool sv_record_ok(const dsmil_simclr_view& r, long long n_tiles, int H, int W) {
    return r.tile >= 0 && r.tile < n_tiles && r.h >= 1 && r.w >= 1 && r.i >= 0 && r.j >= 0 && r.h <= H && r.w <= W &&
           r.i <= H - r.h && r.j <= W - r.w;
}

// ---- Pillow's Resample.c: precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter, one output position ----
SV_HD int sv_resample_ksize(int inSize, int outSize) {
    double filterscale = (double)inSize / outSize;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(1.0 * filterscale) * 2 + 1;
}

SV_HD double sv_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// k[0 .. ksize): the fixed-point coefficients of output xx (zero past *n); *xmin the first source position
SV_HD void sv_resample_coeffs(int inSize, int outSize, int xx, int ksize, int* k, int* xmin_out, int* n_out) {
    const double scale = (double)inSize / outSize;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inSize) xmax = inSize;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += sv_bilinear((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < ksize; ++x) {
        int c = 0;
        if (x < xmax) {
            double w = sv_bilinear((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
            c = w < 0 ? (int)(-0.5 + w * (1 << SV_PRECISION_BITS)) : (int)(0.5 + w * (1 << SV_PRECISION_BITS));
        }
        k[x] = c;
    }
    *xmin_out = xmin;
    *n_out = xmax;
}

SV_HD uint8_t sv_clip8_fixed(int ss) {
    ss >>= SV_PRECISION_BITS;
    return (uint8_t)(ss < 0 ? 0 : ss > 255 ? 255 : ss);
}

// one output byte of a pass: n taps at p, p + stride, ...
SV_HD uint8_t sv_resample_px(const uint8_t* p, long long stride, const int* k, int n) {
    int ss = 1 << (SV_PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) ss += (int)p[t * stride] * k[t];
    return sv_clip8_fixed(ss);
}

// ---- Pillow's Convert.c ----
SV_HD int sv_L(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

SV_HD int sv_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

SV_HD void sv_rgb2hsv(int r, int g, int b, int* uh, int* us, int* uv) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    *uv = maxc;
    if (minc == maxc) {
        *uh = 0;
        *us = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = ((float)(maxc - r)) / cr;
    const float gc = ((float)(maxc - g)) / cr;
    const float bc = ((float)(maxc - b)) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + rc - bc);
    else h = (float)(4.0 + gc - rc);
    double hd = h / 6.0 + 1.0;        // fmod(., 1.0) of a value in [5/6, 11/6]
    if (hd >= 1.0) hd -= 1.0;
    h = (float)hd;
    *uh = sv_clip8((int)(h * 255.0));
    *us = sv_clip8((int)(s * 255.0));
}

SV_HD void sv_hsv2rgb(int h, int s, int v, int* r, int* g, int* b) {
    if (s == 0) {
        *r = *g = *b = v;
        return;
    }
    const int i = (int)floor((float)h * 6.0 / 255.0);
    const float f = (float)((float)h * 6.0 / 255.0 - (float)i);
    const float fs = (float)(((float)s) / 255.0);
    const int p = sv_clip8((int)round((float)v * (1.0 - fs)));
    const int q = sv_clip8((int)round((float)v * (1.0 - fs * f)));
    const int t = sv_clip8((int)round((float)v * (1.0 - fs * (1.0 - f))));
    switch (i % 6) {
        case 0: *r = v; *g = t; *b = p; break;
        case 1: *r = q; *g = v; *b = p; break;
        case 2: *r = p; *g = v; *b = t; break;
        case 3: *r = p; *g = q; *b = v; break;
        case 4: *r = t; *g = p; *b = v; break;
        default: *r = v; *g = p; *b = q; break;
    }
}

// ---- Pillow's Blend.c: in1 the degenerate image's byte, in2 the image's ----
SV_HD int sv_blend(int in1, int in2, float alpha) {
    const float t = (float)in1 + alpha * (float)(in2 - in1);
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t;
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (int)t;
}

// one pixel of a jitter operation (op 0 brightness, 1 contrast, 2 saturation, 3 hue); `mean` is the contrast's grey level
SV_HD void sv_jitter_px(uint8_t* px, int op, const dsmil_simclr_view& r, int mean) {
    const int R = px[0], G = px[1], B = px[2];
    int o0, o1, o2;
    if (op == 0) {
        o0 = sv_blend(0, R, r.brightness); o1 = sv_blend(0, G, r.brightness); o2 = sv_blend(0, B, r.brightness);
    } else if (op == 1) {
        o0 = sv_blend(mean, R, r.contrast); o1 = sv_blend(mean, G, r.contrast); o2 = sv_blend(mean, B, r.contrast);
    } else if (op == 2) {
        const int l = sv_L(R, G, B);
        o0 = sv_blend(l, R, r.saturation); o1 = sv_blend(l, G, r.saturation); o2 = sv_blend(l, B, r.saturation);
    } else {
        int h, s, v;
        sv_rgb2hsv(R, G, B, &h, &s, &v);
        sv_hsv2rgb((h + r.hue) & 255, s, v, &o0, &o1, &o2);
    }
    px[0] = (uint8_t)o0; px[1] = (uint8_t)o1; px[2] = (uint8_t)o2;
}

// int(mean(L) + 0.5) as ImageStat gives it: the integer sum over the count in double
SV_HD int sv_contrast_mean(long long sum, int count) { return (int)((double)sum / (double)count + 0.5); }

// ---- the blur ----
SV_HD void sv_blur_weights(float sigma, int ksize, float* w) {
    const double half = (ksize - 1) / 2.0, s2 = 2.0 * (double)sigma * (double)sigma;
    double sum = 0.0;
    for (int t = 0; t < ksize; ++t) sum += exp(-((t - half) * (t - half)) / s2);
    for (int t = 0; t < ksize; ++t) w[t] = (float)(exp(-((t - half) * (t - half)) / s2) / sum);
}

SV_HD int sv_reflect101(int p, int n) { return p < 0 ? -p : p >= n ? 2 * (n - 1) - p : p; }

// the horizontal pass's value at (row, x) of channel plane `img + c`: taps in order, fp32 fused multiply-adds
SV_HD float sv_blur_row(const uint8_t* row, int x, int S, int ksize, const float* w) {
    const int half = ksize >> 1;
    float a = 0.0f;
    // (kept a loop on the device, where only the border columns come here: unrolled inside sv_blur_column, the compiler holds
    // every tap's reflected position in a register beside the ring, and the kernel spills at its 128-register ceiling)
#pragma unroll 1
    for (int t = 0; t < ksize; ++t) a = fmaf(w[t], (float)row[3 * sv_reflect101(x + t - half, S)], a);
    return a;
}

SV_HD uint8_t sv_round8(float v) {
    const float r = rintf(v);
    return (uint8_t)(r <= 0.0f ? 0 : r >= 255.0f ? 255 : (int)r);
}

SV_HD float sv_to_float(uint8_t b) { return (float)b / 255.0f; }

// The device's separable form: one thread walks rows [y0, y1) of one column (x, c) and keeps the K row sums its vertical window
// needs in registers, so every row sum is evaluated once per segment instead of once per output.  Each row sum is
// sv_blur_row's and the vertical sum runs over the taps in the host's order (w[0] first): the bytes are the host's.
template <int K>
__device__ __forceinline__ void sv_blur_column(const uint8_t* img, int c, int x, int y0, int y1, int S, const float* w, float* of,
                                               uint8_t* ou) {
    constexpr int half = K >> 1;
    float ring[K];
    // away from the left and right borders the taps are K bytes at a constant stride (immediate offsets, no position held in a
    // register); the half-window of columns at either border takes sv_blur_row's loop with the reflection.  Same sums.
    const bool interior = x >= half && x + half < S;
    float wr[K];
#pragma unroll
    for (int t = 0; t < K; ++t) wr[t] = w[t];
    auto row_sum = [&](int y) {
        const uint8_t* row = img + (size_t)sv_reflect101(y, S) * S * 3 + c;
        if (!interior) return sv_blur_row(row, x, S, K, w);
        const uint8_t* p = row + 3 * (x - half);
        float a = 0.0f;
#pragma unroll
        for (int t = 0; t < K; ++t) a = fmaf(wr[t], (float)p[3 * t], a);
        return a;
    };
#pragma unroll
    for (int t = 0; t < K - 1; ++t) ring[t] = row_sum(y0 + t - half);
    for (int y = y0; y < y1; ++y) {
        ring[K - 1] = row_sum(y + half);
        float a = 0.0f;
#pragma unroll
        for (int t = 0; t < K; ++t) a = fmaf(wr[t], ring[t], a);
#pragma unroll
        for (int t = 0; t < K - 1; ++t) ring[t] = ring[t + 1];
        const uint8_t b = sv_round8(a);
        if (ou) ou[((size_t)y * S + x) * 3 + c] = b;
        if (of) of[((size_t)c * S + y) * S + x] = sv_to_float(b);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------------------------------------------------------
struct SvArgs {
    const uint8_t* tiles;
    const dsmil_simclr_view* views;
    float* out_f;
    uint8_t* out_u8;
    uint8_t* ws;
    long long n_tiles, n_views, slot_bytes, tmp_bytes;
    int H, W, S, kblur;
};

template <bool RES>
__global__ __launch_bounds__(SV_THREADS) void k_simclr_views(SvArgs a) {
    extern __shared__ __align__(16) unsigned char sv_lds[];
    const int S = a.S, H = a.H, W = a.W, tid = threadIdx.x;
    const int img_bytes = S * S * 3;
    uint8_t* const slot = a.ws + (size_t)blockIdx.x * a.slot_bytes;
    uint8_t* const tmp = slot;
    uint8_t* img;
    unsigned char* aux;
    if (RES) {
        img = sv_lds;
        aux = sv_lds + ((img_bytes + 15) & ~15);
    } else {
        img = slot + a.tmp_bytes;
        aux = sv_lds;
    }
    int* const coef = (int*)aux;                                          // [2][SV_MAXCOEF]
    short* const bnd = (short*)(aux + 2 * SV_MAXCOEF * 4);                // [2][SV_MAXDIM][2]: first tap, taps
    float* const wts = (float*)(aux + 2 * SV_MAXCOEF * 4 + 2 * SV_MAXDIM * 2 * 2);   // [16]
    int* const red = (int*)(wts + 16);

    for (long long v = blockIdx.x; v < a.n_views; v += gridDim.x) {
        const dsmil_simclr_view r = a.views[v];
        float* const of = a.out_f ? a.out_f + (size_t)v * img_bytes : nullptr;
        uint8_t* const ou = a.out_u8 ? a.out_u8 + (size_t)v * img_bytes : nullptr;
        if (!sv_record_ok(r, a.n_tiles, H, W)) {          // (uniform over the workgroup) nothing is read for it
            for (int e = tid; e < img_bytes; e += SV_THREADS) {
                if (of) of[e] = 0.0f;
                if (ou) ou[e] = 0;
            }
            continue;
        }
        const uint8_t* const crop = a.tiles + (((size_t)r.tile * H + r.i) * W + r.j) * 3;
        const bool need_h = r.w != S, need_v = r.h != S;
        const int ksx = sv_resample_ksize(r.w, S), ksy = sv_resample_ksize(r.h, S);
        if (tid < 2 * S) {
            const int pass = tid >= S, xx = pass ? tid - S : tid;
            int xmin, n;
            sv_resample_coeffs(pass ? r.h : r.w, S, xx, pass ? ksy : ksx, coef + pass * SV_MAXCOEF + xx * (pass ? ksy : ksx), &xmin,
                               &n);
            bnd[(pass * SV_MAXDIM + xx) * 2] = (short)xmin;
            bnd[(pass * SV_MAXDIM + xx) * 2 + 1] = (short)n;
        }
        if (tid == SV_THREADS - 1) {
            red[0] = 0;
            if (r.flags & DSMIL_SIMCLR_BLUR) sv_blur_weights(r.sigma, a.kblur, wts);
        }
        __syncthreads();

        // 1a. horizontal pass: crop rows -> tmp (or straight into the view when no vertical pass follows)
        if (need_h) {
            uint8_t* const dst = need_v ? tmp : img;
            for (int e = tid; e < r.h * S; e += SV_THREADS) {
                const int yy = e / S, xx = e - yy * S;
                const int xmin = bnd[xx * 2], n = bnd[xx * 2 + 1];
                const uint8_t* p = crop + ((size_t)yy * W + xmin) * 3;
                const int* k = coef + xx * ksx;
                uint8_t* o = dst + (size_t)e * 3;
                o[0] = sv_resample_px(p, 3, k, n);
                o[1] = sv_resample_px(p + 1, 3, k, n);
                o[2] = sv_resample_px(p + 2, 3, k, n);
            }
            __syncthreads();
        }
        // 1b. vertical pass -> the view
        if (need_v) {
            const uint8_t* const src = need_h ? tmp : crop;
            const long long stride = need_h ? (long long)S * 3 : (long long)W * 3;
            for (int e = tid; e < S * S; e += SV_THREADS) {
                const int yy = e / S, xx = e - yy * S;
                const int ymin = bnd[(SV_MAXDIM + yy) * 2], n = bnd[(SV_MAXDIM + yy) * 2 + 1];
                const uint8_t* p = src + (size_t)ymin * stride + (size_t)xx * 3;
                const int* k = coef + SV_MAXCOEF + yy * ksy;
                uint8_t* o = img + (size_t)e * 3;
                o[0] = sv_resample_px(p, stride, k, n);
                o[1] = sv_resample_px(p + 1, stride, k, n);
                o[2] = sv_resample_px(p + 2, stride, k, n);
            }
        } else if (!need_h) {
            for (int e = tid; e < S * S; e += SV_THREADS) {
                const int yy = e / S, xx = e - yy * S;
                const uint8_t* p = crop + ((size_t)yy * W + xx) * 3;
                uint8_t* o = img + (size_t)e * 3;
                o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
            }
        }
        __syncthreads();

        // 2. flip: one thread per pixel pair
        if (r.flags & DSMIL_SIMCLR_FLIP) {
            const int half = S >> 1;
            for (int e = tid; e < S * half; e += SV_THREADS) {
                const int yy = e / half, xx = e - yy * half;
                uint8_t* p = img + ((size_t)yy * S + xx) * 3;
                uint8_t* q = img + ((size_t)yy * S + (S - 1 - xx)) * 3;
                const uint8_t p0 = p[0], p1 = p[1], p2 = p[2];
                p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
                q[0] = p0; q[1] = p1; q[2] = p2;
            }
            __syncthreads();
        }
        // 3. colour jitter
        if (r.flags & DSMIL_SIMCLR_JITTER) {
            for (int pos = 0; pos < 4; ++pos) {
                const int op = (r.order >> (2 * pos)) & 3;
                int mean = 0;
                if (op == 1) {
                    int part = 0;
                    for (int e = tid; e < S * S; e += SV_THREADS) {
                        const uint8_t* p = img + (size_t)e * 3;
                        part += sv_L(p[0], p[1], p[2]);
                    }
                    atomicAdd(red, part);            // <= 255 * 2^16: fits
                    __syncthreads();
                    mean = sv_contrast_mean(red[0], S * S);
                    __syncthreads();
                    if (tid == 0) red[0] = 0;
                }
                for (int e = tid; e < S * S; e += SV_THREADS) sv_jitter_px(img + (size_t)e * 3, op, r, mean);
                __syncthreads();
            }
        }
        // 4. greyscale
        if (r.flags & DSMIL_SIMCLR_GREY) {
            for (int e = tid; e < S * S; e += SV_THREADS) {
                uint8_t* p = img + (size_t)e * 3;
                const uint8_t l = (uint8_t)sv_L(p[0], p[1], p[2]);
                p[0] = l; p[1] = l; p[2] = l;
            }
            __syncthreads();
        }
        // 5 + 6. blur and output, in output order
        if ((r.flags & DSMIL_SIMCLR_BLUR) && a.kblur > 1) {
            // columns x row segments: about two work items per thread (3 segments of 75 rows at S = 224); neighbouring
            // threads take neighbouring x of one channel for the fp32 planes, neighbouring bytes for the uint8 form
            const int cols = S * 3, nseg = 2 * SV_THREADS / cols > 0 ? 2 * SV_THREADS / cols : 1, len = (S + nseg - 1) / nseg;
            for (int e = tid; e < cols * nseg; e += SV_THREADS) {
                const int seg = e / cols, col = e - seg * cols;
                // within a segment the interior columns come first and the 2 * half border columns per channel last, so that
                // only the wave across that boundary runs both forms of the row sum
                const int half = a.kblur >> 1, wi = S - 2 * half, b = col - wi * 3;
                int c, x;
                if (b < 0) {
                    c = of ? col / wi : col % 3;
                    x = half + (of ? col - c * wi : col / 3);
                } else {
                    c = b % 3;
                    x = b / 3 < half ? b / 3 : wi + b / 3;
                }
                const int y0 = seg * len, y1 = y0 + len < S ? y0 + len : S;
                if (y0 >= y1) continue;
                switch (a.kblur) {
                    case 3: sv_blur_column<3>(img, c, x, y0, y1, S, wts, of, ou); break;
                    case 5: sv_blur_column<5>(img, c, x, y0, y1, S, wts, of, ou); break;
                    case 7: sv_blur_column<7>(img, c, x, y0, y1, S, wts, of, ou); break;
                    case 9: sv_blur_column<9>(img, c, x, y0, y1, S, wts, of, ou); break;
                    case 11: sv_blur_column<11>(img, c, x, y0, y1, S, wts, of, ou); break;
                    case 13: sv_blur_column<13>(img, c, x, y0, y1, S, wts, of, ou); break;
                    default: sv_blur_column<15>(img, c, x, y0, y1, S, wts, of, ou); break;
                }
            }
        } else {
            if (ou)
                for (int e = tid; e < img_bytes; e += SV_THREADS) ou[e] = img[e];
            if (of)
                for (int e = tid; e < img_bytes; e += SV_THREADS) {
                    const int c = e / (S * S), px = e - c * S * S;
                    of[e] = sv_to_float(img[px * 3 + c]);
                }
        }
        __syncthreads();       // the next view overwrites the tables and the view
    }
}

size_t sv_tmp_bytes(int H, int S) { return ((size_t)H * S * 3 + 255) & ~(size_t)255; }

size_t sv_slot_bytes(int H, int S) {
    return sv_tmp_bytes(H, S) + (S > SV_RES_MAX_S ? (((size_t)S * S * 3 + 255) & ~(size_t)255) : 0);
}

long long sv_grid(long long n_views) { return n_views < SV_SLOTS ? n_views : SV_SLOTS; }

}  // namespace

extern "C" {

size_t dsmil_simclr_views_workspace_bytes(int64_t n_views, int H, int W, int S) {
    if (n_views < 1 || n_views > (1ll << 24) || !sv_shape_ok(H, W, S)) return 0;
    return (size_t)sv_grid(n_views) * sv_slot_bytes(H, S);
}

int dsmil_simclr_views(const uint8_t* tiles_nhwc, int64_t n_tiles, int H, int W, const dsmil_simclr_view* views, int64_t n_views,
                       int S, float* out_nchw, uint8_t* out_nhwc, void* ws, size_t ws_bytes, void* stream) {
    if (!tiles_nhwc || !views || !ws || (!out_nchw && !out_nhwc) || n_tiles < 1 || n_views < 1) return DSMIL_E_INVALID;
    const size_t need = dsmil_simclr_views_workspace_bytes(n_views, H, W, S);
    if (need == 0 || n_tiles > (1ll << 24)) return DSMIL_E_UNSUPPORTED;
    if (ws_bytes < need) return DSMIL_E_WORKSPACE;
    SvArgs a{tiles_nhwc, views, out_nchw, out_nhwc, (uint8_t*)ws, (long long)n_tiles, (long long)n_views,
             (long long)sv_slot_bytes(H, S), (long long)sv_tmp_bytes(H, S), H, W, S, sv_blur_ksize(S)};
    const bool res = S <= SV_RES_MAX_S;
    const int lds = SV_AUX_BYTES + (res ? ((S * S * 3 + 15) & ~15) : 0);
    void (*kern)(SvArgs) = res ? k_simclr_views<true> : k_simclr_views<false>;
    if (!dsmil_lds::allow((const void*)kern, lds)) return DSMIL_E_LAUNCH;
    hipLaunchKernelGGL(kern, dim3((unsigned)sv_grid(n_views)), dim3(SV_THREADS), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? DSMIL_OK : DSMIL_E_LAUNCH;
}

int dsmil_simclr_views_host(const uint8_t* tiles_nhwc, int64_t n_tiles, int H, int W, const dsmil_simclr_view* views,
                            int64_t n_views, int S, float* out_nchw, uint8_t* out_nhwc, void* ws, size_t ws_bytes) {
    (void)ws; (void)ws_bytes;
    if (!tiles_nhwc || !views || (!out_nchw && !out_nhwc) || n_tiles < 1 || n_views < 1) return DSMIL_E_INVALID;
    if (!sv_shape_ok(H, W, S)) return DSMIL_E_UNSUPPORTED;
    for (int64_t v = 0; v < n_views; ++v)
        if (!sv_record_ok(views[v], n_tiles, H, W)) return DSMIL_E_INVALID;
    const int kblur = sv_blur_ksize(S);
    const size_t img_bytes = (size_t)S * S * 3;
    std::vector<uint8_t> tmp((size_t)H * S * 3), img(img_bytes), res(img_bytes);
    std::vector<int> kx((size_t)SV_MAXCOEF), ky((size_t)SV_MAXCOEF), bx(2 * SV_MAXDIM), by(2 * SV_MAXDIM);
    std::vector<float> rows;
    float wts[16];
    for (int64_t v = 0; v < n_views; ++v) {
        const dsmil_simclr_view r = views[v];
        const uint8_t* crop = tiles_nhwc + (((size_t)r.tile * H + r.i) * W + r.j) * 3;
        const bool need_h = r.w != S, need_v = r.h != S;
        const int ksx = sv_resample_ksize(r.w, S), ksy = sv_resample_ksize(r.h, S);
        for (int xx = 0; xx < S; ++xx) {
            sv_resample_coeffs(r.w, S, xx, ksx, kx.data() + xx * ksx, &bx[2 * xx], &bx[2 * xx + 1]);
            sv_resample_coeffs(r.h, S, xx, ksy, ky.data() + xx * ksy, &by[2 * xx], &by[2 * xx + 1]);
        }
        if (need_h) {
            uint8_t* dst = need_v ? tmp.data() : img.data();
            for (int yy = 0; yy < r.h; ++yy)
                for (int xx = 0; xx < S; ++xx)
                    for (int c = 0; c < 3; ++c)
                        dst[((size_t)yy * S + xx) * 3 + c] =
                            sv_resample_px(crop + ((size_t)yy * W + bx[2 * xx]) * 3 + c, 3, kx.data() + xx * ksx, bx[2 * xx + 1]);
        }
        if (need_v) {
            const uint8_t* src = need_h ? tmp.data() : crop;
            const long long stride = need_h ? (long long)S * 3 : (long long)W * 3;
            for (int yy = 0; yy < S; ++yy)
                for (int xx = 0; xx < S; ++xx)
                    for (int c = 0; c < 3; ++c)
                        img[((size_t)yy * S + xx) * 3 + c] = sv_resample_px(src + (size_t)by[2 * yy] * stride + (size_t)xx * 3 + c,
                                                                            stride, ky.data() + yy * ksy, by[2 * yy + 1]);
        } else if (!need_h) {
            for (int yy = 0; yy < S; ++yy) memcpy(img.data() + (size_t)yy * S * 3, crop + (size_t)yy * W * 3, (size_t)S * 3);
        }
        if (r.flags & DSMIL_SIMCLR_FLIP)
            for (int yy = 0; yy < S; ++yy)
                for (int xx = 0; xx < S / 2; ++xx)
                    for (int c = 0; c < 3; ++c) {
                        uint8_t& p = img[((size_t)yy * S + xx) * 3 + c];
                        uint8_t& q = img[((size_t)yy * S + (S - 1 - xx)) * 3 + c];
                        const uint8_t t = p; p = q; q = t;
                    }
        if (r.flags & DSMIL_SIMCLR_JITTER)
            for (int pos = 0; pos < 4; ++pos) {
                const int op = (r.order >> (2 * pos)) & 3;
                int mean = 0;
                if (op == 1) {
                    long long sum = 0;
                    for (int e = 0; e < S * S; ++e) sum += sv_L(img[3 * e], img[3 * e + 1], img[3 * e + 2]);
                    mean = sv_contrast_mean(sum, S * S);
                }
                for (int e = 0; e < S * S; ++e) sv_jitter_px(img.data() + (size_t)e * 3, op, r, mean);
            }
        if (r.flags & DSMIL_SIMCLR_GREY)
            for (int e = 0; e < S * S; ++e) {
                const uint8_t l = (uint8_t)sv_L(img[3 * e], img[3 * e + 1], img[3 * e + 2]);
                img[3 * e] = img[3 * e + 1] = img[3 * e + 2] = l;
            }
        const uint8_t* fin = img.data();
        if ((r.flags & DSMIL_SIMCLR_BLUR) && kblur > 1) {
            // separable with an fp32 intermediate: the same sums, in the same order, as sv_blur_column
            sv_blur_weights(r.sigma, kblur, wts);
            rows.resize(img_bytes);
            for (int yy = 0; yy < S; ++yy)
                for (int xx = 0; xx < S; ++xx)
                    for (int c = 0; c < 3; ++c)
                        rows[((size_t)yy * S + xx) * 3 + c] = sv_blur_row(img.data() + (size_t)yy * S * 3 + c, xx, S, kblur, wts);
            const int half = kblur >> 1;
            for (int yy = 0; yy < S; ++yy)
                for (int e = 0; e < S * 3; ++e) {
                    float acc = 0.0f;
                    for (int t = 0; t < kblur; ++t)
                        acc = fmaf(wts[t], rows[(size_t)sv_reflect101(yy + t - half, S) * S * 3 + e], acc);
                    res[(size_t)yy * S * 3 + e] = sv_round8(acc);
                }
            fin = res.data();
        }
        if (out_nhwc) memcpy(out_nhwc + (size_t)v * img_bytes, fin, img_bytes);
        if (out_nchw)
            for (int c = 0; c < 3; ++c)
                for (int e = 0; e < S * S; ++e) out_nchw[(size_t)v * img_bytes + (size_t)c * S * S + e] = sv_to_float(fin[3 * e + c]);
    }
    return DSMIL_OK;
}

}  // extern "C"
