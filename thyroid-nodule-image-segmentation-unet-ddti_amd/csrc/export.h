// Predict-mode export (main.py --mode predict, Trainer.test --save_overlays): a score plane resized
// back to the resolution of the frame it came from, thresholded into a mask there, and a contour /
// tint overlay of that mask on the gray frame -- the device-side replacement of the matplotlib +
// scikit-image plot of the reference (utils/trainer.py:262-299), which needs neither.  Per-pixel
// functions and steps shared by the device kernels (kernels_export.hip) and the host twins
// unet_resize_f32_mask_host / unet_overlay_u8_host (the edt.h pattern: testable without a GPU).
// The header also compiles for the host alone (EXPORT_HOST_ONLY: no HIP headers).
//
// Resize plan (host only).  Pillow's precompute_coeffs (libImaging/Resample.c) for the BILINEAR
// filter, in double, for one axis in -> out, WITHOUT the 8-bit fixed-point conversion (mode "F"
// images are resampled with the double coefficients): scale = in / out, fs = max(scale, 1),
// support = fs, ksize = 2 ceil(support) + 1; for output xx: center = (xx + 0.5) scale,
// xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in) - xmin,
// taps w = max(0, 1 - |(x + xmin - center + 0.5) * (1 / fs)|), each divided by their sum when that
// is not zero.  coeffs [out][ksize] doubles (zero past xmax), bounds [out] {xmin, xmax}: the layout
// of unet_resize_plan.
//
// Resize pass.  ss = 0.0 in double; for each tap in ascending order ss += (double)pixel * k, the
// multiply and the add rounded separately (a float times a double is not exact in double, so a
// fused multiply-add differs in the last bit); the result is stored as (float)ss.  The horizontal
// pass runs first into a float32 intermediate (Pillow keeps a float32 image between the passes),
// the vertical pass second; an axis whose size does not change is skipped, as Pillow skips it.
//
// Threshold.  EXPORT_SIGMOID_HALF: foreground iff sigmoid(v) > 0.5f, through surf_pred, the
// readout of unet_mask_counts (not v > 0: the float32 sigmoid rounds to exactly 0.5 for tiny
// positive v).  EXPORT_GREATER: foreground iff v > thr; a probability plane of a "prob" TTA merge
// at 0.5, or a logit plane against edge e[k - 1] of operating point k (curve.h: x > e[k - 1]).
// NaN is background under both.
//
// Contour.  A foreground pixel is a contour pixel of width r in 1..3 iff some pixel at city-block
// distance <= r is background or lies outside the image; r = 1 is surf.h's border.
//
// Overlay, integer arithmetic only.  Base (g, g, g) from the gray byte.  Interior prediction pixels
// (foreground, not contour) are tinted when alpha in 0..256 is not zero: channel =
// (g (256 - alpha) + col alpha + 128) >> 8 with col = (255, 0, 0).  Then the contour pixels of the
// ground truth, when given, are solid (0, 0, 255), then those of the prediction solid (255, 0, 0):
// the prediction is drawn last and wins, as the reference plots blue first, then red.  The ground
// truth gets no tint.  A mask byte is foreground iff it is not zero.
//
// Statistics of the prediction mask: int64[6] = {area, contour pixels, x0, y0, x1, y1}, the
// bounding box inclusive; an empty mask gives {0, 0, -1, -1, -1, -1}.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef EXPORT_HOST_ONLY
#define EXPORT_HD inline
#include "mask_readout.h"  // surf_pred, the definition surf.h uses
#else
#include "surf.h"
#define EXPORT_HD SURF_HD
#endif

constexpr int EXPORT_SIGMOID_HALF = 0;
constexpr int EXPORT_GREATER = 1;
constexpr int EXPORT_MAX_WIDTH = 3;
constexpr int EXPORT_STAT_FIELDS = 6;

EXPORT_HD bool export_kind_ok(int kind) { return kind == EXPORT_SIGMOID_HALF || kind == EXPORT_GREATER; }
EXPORT_HD bool export_width_ok(int r) { return r >= 1 && r <= EXPORT_MAX_WIDTH; }
EXPORT_HD bool export_alpha_ok(int alpha) { return alpha >= 0 && alpha <= 256; }

// ---- plan (host) ----
// returns ksize; coeffs / bounds null: ksize alone
inline int export_resize_plan(int in_size, int out_size, double* coeffs, int32_t* bounds) {
    double filterscale, scale;
    filterscale = scale = (double)(float)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    if (!coeffs || !bounds) return ksize;
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        double* k = coeffs + (int64_t)xx * ksize;
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        int x = 0;
        for (; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; ++x) k[x] = 0.0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

// ---- one output pixel of a pass ----
// one tap: the product and the sum each rounded to double on their own.  HIP device code contracts
// a * b + c into one fused operation by default, and so does __dadd_rn(ss, __dmul_rn(a, b)), which
// the headers define as plain + and *: the pragma is what keeps the two roundings apart.
EXPORT_HD double export_mac(double ss, float pixel, double k) {
#if defined(__clang__)
#pragma clang fp contract(off)
    const double prod = (double)pixel * k;
#else
    volatile double prod = (double)pixel * k;  // (volatile: no contraction whatever the flags)
#endif
    return ss + prod;
}

// the taps a table entry may name inside an axis of `in` pixels: a plan of export_resize_plan is
// unchanged, any other table cannot index outside the plane
EXPORT_HD void export_clamp_taps(int in, int ksize, int& first, int& count) {
    first = first < 0 ? 0 : first > in ? in : first;
    count = count < 0 ? 0 : count;
    count = count > ksize ? ksize : count;
    count = count > in - first ? in - first : count;
}

// src: the first tap's pixel, consecutive taps `stride` floats apart
EXPORT_HD float export_resample(const float* src, int64_t stride, const double* k, int count) {
    double ss = 0.0;
    for (int t = 0; t < count; ++t) ss = export_mac(ss, src[t * stride], k[t]);
    return (float)ss;
}

EXPORT_HD bool export_fg(int kind, float v, float thr) { return kind == EXPORT_SIGMOID_HALF ? surf_pred(v) : v > thr; }

// ---- contour ----
// fg(i, j): the mask inside the image
template <typename F>
EXPORT_HD bool export_contour(F fg, int i, int j, int H, int W, int r) {
    if (!fg(i, j)) return false;
    for (int dy = -r; dy <= r; ++dy) {
        const int rem = r - (dy < 0 ? -dy : dy);
        for (int dx = -rem; dx <= rem; ++dx) {
            const int y = i + dy, x = j + dx;
            if (y < 0 || y >= H || x < 0 || x >= W || !fg(y, x)) return true;
        }
    }
    return false;
}

// ---- overlay ----
// pixel classes of a mask: 0 background, 1 interior, 2 contour
constexpr int EXPORT_BG = 0, EXPORT_INTERIOR = 1, EXPORT_CONTOUR = 2;

EXPORT_HD int export_blend(int g, int col, int alpha) { return (g * (256 - alpha) + col * alpha + 128) >> 8; }

// pred_class / gt_class: the classes above (gt_class EXPORT_BG without a ground truth)
EXPORT_HD void export_pixel(int g, int pred_class, int gt_class, int alpha, uint8_t& R, uint8_t& G, uint8_t& B) {
    int r = g, gg = g, b = g;
    if (pred_class == EXPORT_INTERIOR && alpha != 0) {
        r = export_blend(g, 255, alpha);
        gg = export_blend(g, 0, alpha);
        b = gg;
    }
    if (gt_class == EXPORT_CONTOUR) r = 0, gg = 0, b = 255;
    if (pred_class == EXPORT_CONTOUR) r = 255, gg = 0, b = 0;
    R = (uint8_t)r;
    G = (uint8_t)gg;
    B = (uint8_t)b;
}

// ---- host twins ----
// tmp: h * ow floats (used when both axes change)
inline void export_resize_mask_host(const float* src, int h, int w, int oh, int ow, const double* kh,
                                    const int32_t* bh, int ksh, const double* kv, const int32_t* bv, int ksv,
                                    int kind, float thr, float* tmp, float* plane, uint8_t* mask) {
    const bool need_h = ow != w, need_v = oh != h;
    const float* mid = src;
    if (need_h) {
        // without a vertical pass the horizontal one writes the result: tmp then holds oh == h rows
        for (int y = 0; y < h; ++y)
            for (int xx = 0; xx < ow; ++xx) {
                int first = bh[2 * xx], count = bh[2 * xx + 1];
                export_clamp_taps(w, ksh, first, count);
                tmp[(int64_t)y * ow + xx] =
                    export_resample(src + (int64_t)y * w + first, 1, kh + (int64_t)xx * ksh, count);
            }
        mid = tmp;
    }
    for (int yy = 0; yy < oh; ++yy) {
        int first = 0, count = 0;
        if (need_v) {
            first = bv[2 * yy], count = bv[2 * yy + 1];
            export_clamp_taps(h, ksv, first, count);
        }
        for (int xx = 0; xx < ow; ++xx) {
            const float v = need_v ? export_resample(mid + (int64_t)first * ow + xx, ow, kv + (int64_t)yy * ksv, count)
                                   : mid[(int64_t)yy * ow + xx];
            if (plane) plane[(int64_t)yy * ow + xx] = v;
            mask[(int64_t)yy * ow + xx] = export_fg(kind, v, thr) ? 1 : 0;
        }
    }
}

inline void export_overlay_host(const uint8_t* gray, const uint8_t* pred, const uint8_t* gt, int h, int w, int r,
                                int alpha, uint8_t* rgb, int64_t* stats) {
    int64_t area = 0, contour = 0, x0 = -1, y0 = -1, x1 = -1, y1 = -1;
    auto pf = [&](int i, int j) { return pred[(int64_t)i * w + j] != 0; };
    auto gf = [&](int i, int j) { return gt[(int64_t)i * w + j] != 0; };
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            int pc = EXPORT_BG, gc = EXPORT_BG;
            if (pf(i, j)) {
                pc = export_contour(pf, i, j, h, w, r) ? EXPORT_CONTOUR : EXPORT_INTERIOR;
                ++area;
                contour += pc == EXPORT_CONTOUR;
                x0 = x0 < 0 || j < x0 ? j : x0;
                y0 = y0 < 0 ? i : y0;
                x1 = j > x1 ? j : x1;
                y1 = i;
            }
            if (gt && gf(i, j)) gc = export_contour(gf, i, j, h, w, r) ? EXPORT_CONTOUR : EXPORT_INTERIOR;
            uint8_t* o = rgb + 3 * ((int64_t)i * w + j);
            export_pixel(gray[(int64_t)i * w + j], pc, gc, alpha, o[0], o[1], o[2]);
        }
    stats[0] = area, stats[1] = contour, stats[2] = x0, stats[3] = y0, stats[4] = x1, stats[5] = y1;
}
