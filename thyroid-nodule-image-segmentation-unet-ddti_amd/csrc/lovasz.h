// Lovasz hinge loss (Berman, Triki, Blaschko: "The Lovasz-Softmax loss", CVPR 2018, the binary
// hinge with per_image=True): the convex surrogate of the Jaccard index, as per-pixel rules shared
// by the device kernels (kernels_lovasz.hip) and the host twin unet_lovasz_host (the edt.h pattern:
// testable without a GPU).
//
// Every (n, c) plane of logits / targets (N, C, H, W) is its own binary problem.  M = H W, i the
// raster index of a pixel of the plane.
//
// Label.  y_i = (t_i >= 0.5f), s_i = y_i ? +1 : -1.  Mixup makes the targets soft and the hinge
// needs a binary label, so a soft target is binarised at one half (0.5 itself is positive; a NaN
// target compares false and is negative).
//
// Error.  e_i = fl32(1 - s_i x_i): the product is exact, so there is one float32 rounding.
//
// Order.  Descending e, ties by ascending i: a STABLE sort, np.argsort(-e, kind="stable") on
// finite e.  The sort runs on lovasz_key(e), an order-reversing map of the float onto uint32, so
// that an ascending least-significant-digit radix sort yields descending e: +inf has the smallest
// key, then the positive floats downwards, +0 and -0 share ONE key (-0 is read as +0), then the
// negative floats down to -inf.  +-inf sort as values.  A NaN has some key of its own (a positive
// NaN sorts before +inf, a negative one after -inf): its place is unspecified, but the sort only
// ever moves the (key, index) pairs it was given, so no index can leave the plane.
//
// Counts.  P = sum y.  For rank r = 0..M-1, cTP_r / cFP_r = the positives / negatives among the
// ranks <= r: exact integers (cFP_r = r + 1 - cTP_r).
//
// Weights.  J_r = 1 - (P - cTP_r) / (P + cFP_r) in float64: one correctly rounded division and
// one subtraction; the denominator is at least 1 in every case (P = 0 included: rank r is then a
// negative).  J_{-1} = 0, g_r = J_r - J_{r-1} in float64, gmap_i = fl32(g_{rank(i)}) where e_i > 0
// and 0 elsewhere, stored in PIXEL order: the per-pixel weight the backward needs.
//
// Loss.  L_plane = sum_r hinge(e_r) g_r, products and sum in float64, hinge(e) = e where e > 0, 0
// where e <= 0 and e itself where it is a NaN (so a NaN logit makes its plane's loss a NaN).
// loss = fl32(sum_planes L_plane / (N C)).
//
// Gradient.  dlogits_i = fl32(fl32((w * -s_i) * gmap_i) / fl32(N C)) where e_i > 0, and 0
// elsewhere (relu'(0) = 0, as torch has it): one float32 product (w * -s_i is exact) and one
// correctly rounded float32 division.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#define LOVASZ_HD __host__ __device__ __forceinline__

constexpr int64_t LOVASZ_MAX_HW = (int64_t)1 << 24;  // the index shares its word with the label
constexpr uint32_t LOVASZ_LABEL_BIT = 0x80000000u;   // of a sorted (index | label) word
constexpr uint32_t LOVASZ_INDEX_MASK = 0x00FFFFFFu;

LOVASZ_HD uint32_t lovasz_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}
LOVASZ_HD float lovasz_float(uint32_t u) {
    float v;
    memcpy(&v, &u, sizeof v);
    return v;
}

LOVASZ_HD bool lovasz_label(float t) { return t >= 0.5f; }

// one rounding: y ? 1 - x : 1 + x
LOVASZ_HD float lovasz_error(float x, bool y) { return 1.0f - (y ? x : -x); }

// ascending keys <=> descending e; -0 -> the key of +0
LOVASZ_HD uint32_t lovasz_key(float e) {
    const uint32_t b = e == 0.0f ? 0u : lovasz_bits(e);
    return (b & 0x80000000u) ? b : b ^ 0x7FFFFFFFu;
}
// the float of a key (the transform is an involution on everything but -0)
LOVASZ_HD float lovasz_unkey(uint32_t k) { return lovasz_float((k & 0x80000000u) ? k : k ^ 0x7FFFFFFFu); }

LOVASZ_HD double lovasz_hinge_of(float e) { return e > 0.0f ? (double)e : (e != e ? (double)e : 0.0); }

// J of a prefix holding ctp positives and cfp negatives, ctp + cfp >= 1
LOVASZ_HD double lovasz_jaccard(int64_t P, int64_t ctp, int64_t cfp) {
    return 1.0 - (double)(P - ctp) / (double)(P + cfp);
}

// g_r of rank r (0-based) whose inclusive positive count is ctp and whose own label is y
LOVASZ_HD double lovasz_grad(int64_t P, int64_t r, int64_t ctp, bool y) {
    const double j = lovasz_jaccard(P, ctp, r + 1 - ctp);
    if (r == 0) return j;
    const int64_t ptp = ctp - (y ? 1 : 0);
    return j - lovasz_jaccard(P, ptp, r - ptp);
}

LOVASZ_HD float lovasz_dlogit(float x, float t, float g, float w, float nc) {
    const bool y = lovasz_label(t);
    const float e = lovasz_error(x, y);
    return e > 0.0f ? ((y ? -w : w) * g) / nc : 0.0f;
}
