// Training augmentations on uint8 planes (reference main.py:66-91 build_train_transform:
// Flip -> Rotate -> AdjustBrightness -> TGCAugment -> CLAHE of utils/transforms.py), as per-pixel
// functions shared by the device kernels (kernels_aug.hip) and the host hooks
// unet_augment_u8_host / unet_clahe_u8_host (the edt.h pattern: testable without a GPU).
// Everything here is integer arithmetic or individually rounded float32 arithmetic, so host
// and device agree bit for bit with Pillow and with utils.transforms.clahe_u8.
//
// Geometry.  Pillow's Image.rotate(angle, NEAREST, expand=False, fillcolor=0) is either one of
// its transposes (angle 0 / 180, and 90 / 270 of a square image) or its 16.16 fixed-point
// nearest affine transform (Geometry.c affine_fixed): xin = (a2 + y a1 + x a0) >> 16,
// yin = (a5 + y a4 + x a3) >> 16 in int32 with an arithmetic shift, fill where (xin, yin) lies
// outside the image.  The mode and the six coefficients come from Python
// (unet_hip.data.rotate_plan follows Pillow's own Python, round() and math included).  The
// flips precede the rotate in the chain, so they fold into the source index.  With
// max(h, w) <= AUG_MAX_SIDE and |a0|, |a1|, |a3|, |a4| <= AUG_MAX_COEF (|cos|, |sin| <= 1 in
// 16.16) the two products stay within 2^29 each, and |a2|, |a5| <= AUG_MAX_OFFSET = 3 * 2^28
// (a rotation about the centre needs less than 2.42 * 2^28), so the int32 sums cannot overflow.
// The entry points check all three bounds.
//
// Point operations.  AdjustBrightness is a 256-entry table (Pillow's ImagingBlend with a black
// image; built in Python).  TGCAugment multiplies row band y / bin_h by a float32 gain and
// truncates after clamping to [0, 255] -- NumPy's float32_array *= python_float, clip, astype.
// SpeckleNoise (between the two, on request: unet_augment_noise_u8) multiplies by one float64
// draw per output pixel, made on the host; its float64 steps are rounded one by one as well.
//
// CLAHE restates utils.transforms.clahe_u8 (cv2.createCLAHE): tile histograms over the plane
// padded bottom / right with REFLECT_101 to whole tiles (by index reflection), clipped and
// redistributed, cumulated into one table per tile, and a float32 bilinear blend of the four
// neighbouring tables per pixel.  The blend's products and sums are rounded one by one (no
// FMA): __fmul_rn / __fadd_rn on the device, -ffp-contract=off for this file's host code.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/unet_hip.h"

#define AUG_HD __host__ __device__ __forceinline__

constexpr int AUG_MAX_SIDE = 8192;
constexpr int AUG_MAX_COEF = 1 << 16;
constexpr int AUG_MAX_OFFSET = 3 << 28;
constexpr int AUG_MAX_BINS = 64;       // unet_aug_params::gain
constexpr int CLAHE_MAX_TILES = 256;

#if defined(__HIP_DEVICE_COMPILE__)
#define AUG_MUL(a, b) __fmul_rn((a), (b))
#define AUG_ADD(a, b) __fadd_rn((a), (b))
#define AUG_SUB(a, b) __fsub_rn((a), (b))
#define AUG_DIV(a, b) __fdiv_rn((a), (b))
#define AUG_DMUL(a, b) __dmul_rn((a), (b))
#define AUG_DADD(a, b) __dadd_rn((a), (b))
#else
#define AUG_MUL(a, b) ((a) * (b))
#define AUG_ADD(a, b) ((a) + (b))
#define AUG_SUB(a, b) ((a) - (b))
#define AUG_DIV(a, b) ((a) / (b))
#define AUG_DMUL(a, b) ((a) * (b))
#define AUG_DADD(a, b) ((a) + (b))
#endif

// Flat source index of output pixel (x, y) of an h x w plane, -1 for a fill pixel.
AUG_HD int aug_source(const unet_aug_params& p, int x, int y, int h, int w) {
    int xin, yin;
    switch (p.mode) {
        case UNET_ROT_AFFINE:
            xin = (p.a[2] + y * p.a[1] + x * p.a[0]) >> 16;
            yin = (p.a[5] + y * p.a[4] + x * p.a[3]) >> 16;
            if (xin < 0 || xin >= w || yin < 0 || yin >= h) return -1;
            break;
        case UNET_ROT_180:
            xin = w - 1 - x;
            yin = h - 1 - y;
            break;
        case UNET_ROT_90:  // Image.ROTATE_90 (counter-clockwise), square planes only
            xin = w - 1 - y;
            yin = x;
            break;
        case UNET_ROT_270:
            xin = y;
            yin = h - 1 - x;
            break;
        default:
            xin = x;
            yin = y;
            break;
    }
    if (p.flip_h) xin = w - 1 - xin;
    if (p.flip_v) yin = h - 1 - yin;
    return yin * w + xin;
}

// TGC of one value: (uint8)trunc(min(max(float32(v) * gain, 0), 255)).
AUG_HD uint8_t aug_gain(uint8_t v, float g) {
    float t = AUG_MUL((float)v, g);
    t = t > 0.f ? t : 0.f;  // also a NaN gain -> 0, never an undefined cast
    t = t < 255.f ? t : 255.f;
    return (uint8_t)(int)t;
}

// SpeckleNoise of one value with its float64 noise draw n: f = float32(v) / 255 (a float32
// division), then in float64 d = f + f * n, d * 255, clamped to [0, 255] and truncated -- NumPy's
// float32_array / 255., + float32_array * float64_array, * 255., clip, astype(uint8).
AUG_HD uint8_t aug_speckle(uint8_t v, double n) {
    double d = (double)AUG_DIV((float)v, 255.f);
    d = AUG_DADD(d, AUG_DMUL(d, n));
    d = AUG_DMUL(d, 255.0);
    d = d > 0.0 ? d : 0.0;  // also a NaN draw -> 0, never an undefined cast
    d = d < 255.0 ? d : 255.0;
    return (uint8_t)(int)d;
}

// Row y of an h-row plane: its TGC band, or -1 when the row keeps its values (past the last
// whole band, or bands of zero rows).
AUG_HD int aug_band(int y, int h, int num_bins) {
    if (num_bins <= 0) return -1;
    const int bin_h = h / num_bins;
    if (bin_h == 0 || y >= num_bins * bin_h) return -1;
    return y / bin_h;
}

// ---------------------------------------------------------------------------------------------
// CLAHE
// ---------------------------------------------------------------------------------------------
struct ClaheGeom {
    int h, w, gx, gy;  // plane, tiles along x / y
    int tw, th;        // tile size of the padded plane
    int limit;         // clip limit per bin (0: no clipping)
    float lut_scale;   // float32(255.0 / area)
    float inv_tw, inv_th;
};

// REFLECT_101 (numpy "reflect") of an index in [n, 2 n - 2]
AUG_HD int clahe_reflect(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }

// Bin k of a tile's clipped histogram after the redistribution of the `clipped` excess counts.
AUG_HD int clahe_bin(int count, int k, int limit, int clipped) {
    if (limit <= 0) return count;
    const int batch = clipped / 256, residual = clipped - batch * 256;
    int v = (count < limit ? count : limit) + batch;
    if (residual > 0) {
        const int step = 256 / residual > 1 ? 256 / residual : 1;
        if (k % step == 0 && k / step < residual) ++v;
    }
    return v;
}

AUG_HD uint8_t clahe_round(float v) {
    v = rintf(v);  // to nearest even, as np.rint
    v = v > 0.f ? v : 0.f;
    v = v < 255.f ? v : 255.f;
    return (uint8_t)(int)v;
}

AUG_HD uint8_t clahe_lut_entry(int cum, float lut_scale) {
    return clahe_round(AUG_MUL((float)cum, lut_scale));
}

// Tile pair and blend weight of coordinate i along an axis of g tiles of size 1 / inv.
AUG_HD void clahe_axis(int i, float inv, int g, int& t1, int& t2, float& a, float& a1) {
    const float f = AUG_SUB(AUG_MUL((float)i, inv), 0.5f);
    const float fl = floorf(f);
    const int t = (int)fl;
    a = AUG_SUB(f, fl);
    a1 = AUG_SUB(1.0f, a);
    t2 = t + 1 < g - 1 ? t + 1 : g - 1;
    t1 = t > 0 ? (t < g - 1 ? t : g - 1) : 0;
}

// Pixel (x, y) of value v; lut: [gy][gx][256] tile tables.
AUG_HD uint8_t clahe_pixel(const ClaheGeom& G, const uint8_t* __restrict__ lut, int x, int y,
                           uint8_t v) {
    int tx1, tx2, ty1, ty2;
    float xa, xa1, ya, ya1;
    clahe_axis(x, G.inv_tw, G.gx, tx1, tx2, xa, xa1);
    clahe_axis(y, G.inv_th, G.gy, ty1, ty2, ya, ya1);
    const float l11 = (float)lut[(ty1 * G.gx + tx1) * 256 + v];
    const float l12 = (float)lut[(ty1 * G.gx + tx2) * 256 + v];
    const float l21 = (float)lut[(ty2 * G.gx + tx1) * 256 + v];
    const float l22 = (float)lut[(ty2 * G.gx + tx2) * 256 + v];
    const float top = AUG_MUL(AUG_ADD(AUG_MUL(l11, xa1), AUG_MUL(l12, xa)), ya1);
    const float bot = AUG_MUL(AUG_ADD(AUG_MUL(l21, xa1), AUG_MUL(l22, xa)), ya);
    return clahe_round(AUG_ADD(top, bot));
}
