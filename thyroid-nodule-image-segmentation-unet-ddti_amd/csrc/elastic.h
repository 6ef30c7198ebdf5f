// ElasticDeform on uint8 planes (reference utils/transforms.py:15-42; here utils.transforms
// gaussian_blur + remap_linear_u8 / remap_nearest, the NumPy restatement of cv2.GaussianBlur +
// cv2.remap), as per-pixel functions shared by the device kernels (kernels_elastic.hip) and the
// host hook unet_elastic_u8_host (the edt.h / aug.h pattern: testable without a GPU).
//
// The host draws the two uniform fields rx, ry (np.random.rand(h, w), float64) and the Gaussian
// taps (utils.transforms.gaussian_kernel in Python); everything after that is here, operation by
// operation, every float64 product and sum rounded on its own (no FMA: __dmul_rn / __dadd_rn on
// the device, and this file's translation unit is compiled with -ffp-contract=off):
//
//   u       = r * 2 - 1
//   row     = sum_i k[i] * u[y][reflect101(x - R + i)]       acc = 0.0; acc = acc + k[i] * v
//   blur    = sum_i k[i] * row[reflect101(y - R + i)][x]     R = ksize / 2
//   map_x   = (float)((double)x + blur_x * alpha), map_y likewise
//
// NumPy pads the field by R with "reflect" (REFLECT_101) and blurs rows first; the row pass of a
// padded row is the row pass of the source row it reflects, so only the h rows of the plane are
// kept.  R <= n - 1 on both axes (the entry points refuse smaller planes), so one reflection
// reaches every padded index.
//
// Image: cv2.remap INTER_LINEAR on 1/32-pixel coordinates, X = rintf(map_x * 32) (ties to even),
// x0 = X >> 5, fx = X & 31, the four weights (32 - fx)(32 - fy) 32, ... sum to 2^15 and the pixel
// is (sum + 2^14) >> 15.  Mask: INTER_NEAREST, rintf of each coordinate.  Both take their
// neighbours through BORDER_REFLECT (fedcba|abcdefgh|hgfedcb: period 2 n, a one-pixel axis maps
// to 0) with a true modulo, so coordinates several periods outside the plane are right.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/unet_hip.h"

#define EL_HD __host__ __device__ __forceinline__

constexpr int EL_MAX_SIDE = 8192;
constexpr int EL_MAX_KSIZE = 31;  // unet_elastic_params::k
// |coordinate * 32| is clamped here before the conversion to int32: far beyond any alpha the
// draws produce (the fields are blurs of values in [-1, 1)), it only keeps a non-finite or huge
// coordinate from an undefined cast.  x0 + 1 and the reflect's arithmetic stay within int32.
constexpr float EL_MAX_COORD = 1073741824.f;  // 2^30

#if defined(__HIP_DEVICE_COMPILE__)
#define EL_DMUL(a, b) __dmul_rn((a), (b))
#define EL_DADD(a, b) __dadd_rn((a), (b))
#define EL_FMUL(a, b) __fmul_rn((a), (b))
#else
#define EL_DMUL(a, b) ((a) * (b))
#define EL_DADD(a, b) ((a) + (b))
#define EL_FMUL(a, b) ((a) * (b))
#endif

// REFLECT_101 (numpy "reflect") of an index in [-(n - 1), 2 n - 2]
EL_HD int el_reflect101(int i, int n) { return i < 0 ? -i : (i < n ? i : 2 * (n - 1) - i); }

// cv2.borderInterpolate(i, n, BORDER_REFLECT) of any int32 index
EL_HD int el_reflect(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * n;
    int m = i % period;
    if (m < 0) m += period;
    return m >= n ? period - 1 - m : m;
}

// The uniform draw r in [0, 1) as a displacement seed in [-1, 1): r * 2 - 1.
EL_HD double el_unit(double r) { return EL_DADD(EL_DMUL(r, 2.0), -1.0); }

// One more tap of a blur pass: acc + k * v.
EL_HD double el_tap(double acc, double k, double v) { return EL_DADD(acc, EL_DMUL(k, v)); }

// float32 map coordinate of pixel index i displaced by blur * alpha.
EL_HD float el_map(int i, double blur, double alpha) {
    return (float)EL_DADD((double)i, EL_DMUL(blur, alpha));
}

// rintf(v) as an int32 (a NaN becomes 0).
EL_HD int el_round(float v) {
    v = rintf(v);  // to nearest even, as np.rint / cvRound
    if (!(v > -EL_MAX_COORD)) return v == v ? -(int)EL_MAX_COORD : 0;
    return v < EL_MAX_COORD ? (int)v : (int)EL_MAX_COORD;
}

// remap_linear_u8 of one output pixel.
EL_HD uint8_t el_linear(const uint8_t* __restrict__ src, int h, int w, float mx, float my) {
    const int X = el_round(EL_FMUL(mx, 32.f)), Y = el_round(EL_FMUL(my, 32.f));
    const int x0 = X >> 5, y0 = Y >> 5, fx = X & 31, fy = Y & 31;
    const int xs0 = el_reflect(x0, w), xs1 = el_reflect(x0 + 1, w);
    const int ys0 = el_reflect(y0, h), ys1 = el_reflect(y0 + 1, h);
    const int v = ((int)src[ys0 * w + xs0] * ((32 - fx) * (32 - fy)) +
                   (int)src[ys0 * w + xs1] * (fx * (32 - fy)) +
                   (int)src[ys1 * w + xs0] * ((32 - fx) * fy) + (int)src[ys1 * w + xs1] * (fx * fy)) *
                  32;  // at most 255 * 2^15
    return (uint8_t)((v + (1 << 14)) >> 15);
}

// remap_nearest of one output pixel.
EL_HD uint8_t el_nearest(const uint8_t* __restrict__ src, int h, int w, float mx, float my) {
    return src[el_reflect(el_round(my), h) * w + el_reflect(el_round(mx), w)];
}
