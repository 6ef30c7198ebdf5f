// Threshold sweep of Trainer.test (ROC / PR curves, Dice at every operating point, the choice of
// one): a histogram of the logits split by target class, and the per-plane statistics read off
// it, as per-pixel functions and steps shared by the device kernels (kernels_curve.hip) and the
// host twins unet_curve_hist_host / unet_curve_stats_host (the edt.h pattern: testable without a
// GPU).  Everything is defined on the logits, by float comparisons and integer sums alone (no
// transcendental on the device), so the device, the host twin and a NumPy restatement agree bit
// for bit.  The header also compiles for the host alone (CURVE_HOST_ONLY: no HIP headers).
//
// Edges.  B bins, B a power of two in 2..CURVE_MAX_BINS, separated by B - 1 strictly increasing
// float32 edges e[0..B-2].  The standard edges (curve_edges, host only) are the logits of the
// probabilities (j + 1) / B: e[j] = (float)log(t / (1 - t)), t = (j + 1) / B in double.  log(t /
// (1 - t)) is odd about t = 1/2, and the lower half is formed as the negated upper half, so the
// float edges are exactly antisymmetric, e[j] == -e[B-2-j], and e[B/2-1] == 0.0f.
//
// Bin.  bin(x) = the number of j with e[j] < x, in 0..B-1.  NaN compares false everywhere and
// lands in bin 0, as -inf does; +inf lands in bin B-1; -0.0f is not > 0.0f.  curve_bin is a
// branch-free log2(B)-step search whose every read lies inside e[0..B-2] and whose result lies in
// 0..B-1 for ANY contents of e, sorted or not: no input can index outside the histogram.
//
// Class.  u = surf_target_u8(t) (the target readout of unet_mask_counts): u == 1 positive, u == 0
// negative (targets in [0, 1) truncate to 0), anything else (soft mixup targets of 2 or above)
// ignored and counted.
//
// Operating point k in 0..B.  A pixel is predicted positive iff bin(x) >= k: k = 0 every pixel,
// k = B none, and for 1 <= k <= B-1 the rule is x > e[k-1].  k = B/2 is x > 0: the 0.5 readout
// sigmoid(x) > 0.5 (surf_pred), EXCEPT for logits in (0, ~2^-24], where expf(-x) rounds to 1 and
// the float32 sigmoid to exactly 0.5: surf_pred calls those background, k = B/2 foreground.
//
// Per-plane statistics, from a plane's histogram neg[b], pos[b] (int32: H W < 2^31):
//     P = sum pos, Nn = sum neg, TP_k = sum_{b >= k} pos[b], FP_k = sum_{b >= k} neg[b],
//     FN_k = P - TP_k,
//     dice_k = (TP_k + FP_k + P == 0) ? 1.0 : (double)(2 TP_k) / (double)(TP_k + FP_k + P)
//              (one correctly rounded division),
//     best_k = the k of the largest dice_k; on equal doubles the smallest |k - B/2|, then the
//              smaller k (curve_better),
//     auc2 = sum_b pos[b] (2 sum_{b' < b} neg[b'] + neg[b]) in int64: exact, at most 2^61.
// AUROC = auc2 / (2 P Nn), undefined when P == 0 or Nn == 0 (the Mann-Whitney count with ties on
// the binned scores).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef CURVE_HOST_ONLY
#define CURVE_HD inline
inline uint8_t surf_target_u8(float t) { return (uint8_t)(int)t; }  // surf.h's
#else
#include "surf.h"
#define CURVE_HD SURF_HD
#endif

constexpr int CURVE_MIN_BINS = 2;
constexpr int CURVE_MAX_BINS = 1024;
constexpr int CURVE_STAT_FIELDS = 8;  // P, Nn, best_k, TP, FP, FN at best_k, auc2, 0

CURVE_HD bool curve_bins_ok(int B) { return B >= CURVE_MIN_BINS && B <= CURVE_MAX_BINS && (B & (B - 1)) == 0; }

// the standard edges (host): B - 1 floats
inline void curve_edges(int B, float* e) {
    e[B / 2 - 1] = 0.0f;
    for (int j = B / 2; j <= B - 2; ++j) {
        const double t = (double)(j + 1) / (double)B;
        e[j] = (float)log(t / (1.0 - t));
        e[B - 2 - j] = -e[j];
    }
}

// every read at an index <= B - 2, the result in 0..B-1, whatever e holds
CURVE_HD int curve_bin(const float* e, int B, float x) {
    int lo = 0;
    for (int step = B >> 1; step >= 1; step >>= 1) lo += e[lo + step - 1] < x ? step : 0;
    return lo;
}

// 0 negative, 1 positive, -1 ignored
CURVE_HD int curve_class(float t) {
    const uint8_t u = surf_target_u8(t);
    return u == 1 ? 1 : u == 0 ? 0 : -1;
}

// the histogram index of a pixel inside a plane's [2][B] rows (row 0 negatives, 1 positives), or
// -1 for an ignored pixel
CURVE_HD int curve_key(const float* e, int B, float x, float t) {
    const int c = curve_class(t);
    const int b = curve_bin(e, B, x);
    return c < 0 ? -1 : c * B + b;
}

// ---- per-plane statistics: three steps, so that the device runs the middle one in parallel ----
// tp[k], fp[k] for k = 0..B (B + 1 entries each); returns P, Nn, auc2
struct CurveSums {
    int64_t P, Nn, auc2;
};
CURVE_HD CurveSums curve_suffix(const int32_t* neg, const int32_t* pos, int B, int32_t* tp, int32_t* fp) {
    int32_t t = 0, f = 0;
    tp[B] = 0;
    fp[B] = 0;
    for (int b = B - 1; b >= 0; --b) {
        t += pos[b];
        f += neg[b];
        tp[b] = t;
        fp[b] = f;
    }
    int64_t below = 0, auc2 = 0;
    for (int b = 0; b < B; ++b) {
        auc2 += (int64_t)pos[b] * (2 * below + neg[b]);
        below += neg[b];
    }
    return CurveSums{(int64_t)t, (int64_t)f, auc2};
}

CURVE_HD double curve_dice(int64_t tp, int64_t fp, int64_t P) {
    const int64_t den = tp + fp + P;
    return den == 0 ? 1.0 : (double)(2 * tp) / (double)den;
}

// is (d, k) a better operating point than (bd, bk)?
CURVE_HD bool curve_better(double d, int k, double bd, int bk, int B) {
    if (d != bd) return d > bd;
    const int a = k > B / 2 ? k - B / 2 : B / 2 - k, b = bk > B / 2 ? bk - B / 2 : B / 2 - bk;
    return a != b ? a < b : k < bk;
}

CURVE_HD int curve_best(const double* dice, int B) {
    int bk = 0;
    for (int k = 1; k <= B; ++k)
        if (curve_better(dice[k], k, dice[bk], bk, B)) bk = k;
    return bk;
}

CURVE_HD void curve_stat_row(const CurveSums& s, const int32_t* tp, const int32_t* fp, int best_k, int64_t* out) {
    out[0] = s.P;
    out[1] = s.Nn;
    out[2] = best_k;
    out[3] = tp[best_k];
    out[4] = fp[best_k];
    out[5] = s.P - tp[best_k];
    out[6] = s.auc2;
    out[7] = 0;
}

// ---- host twins (unet_curve_hist_host / unet_curve_stats_host): the rules above, one pixel and
// one plane at a time ----
// plane_hist [planes][2][B] is overwritten; total [2 B + 1] (the two rows summed over the planes,
// then the ignored pixels) is accumulated
inline void curve_hist_host(const float* x, const float* t, int planes, int64_t hw, const float* e, int B,
                            int32_t* plane_hist, int64_t* total) {
    for (int64_t p = 0; p < planes; ++p) {
        int32_t* h = plane_hist + p * 2 * B;
        for (int j = 0; j < 2 * B; ++j) h[j] = 0;
        int64_t ignored = 0;
        for (int64_t i = 0; i < hw; ++i) {
            const int key = curve_key(e, B, x[p * hw + i], t[p * hw + i]);
            if (key < 0) ++ignored;
            else ++h[key];
        }
        for (int j = 0; j < 2 * B; ++j) total[j] += h[j];
        total[2 * B] += ignored;
    }
}

// out_i64 [planes][CURVE_STAT_FIELDS]; dice_sum [B + 1] += dice_k, the planes in ascending order.
// tp, fp: B + 1 ints each; dice: B + 1 doubles
inline void curve_stats_host(const int32_t* plane_hist, int planes, int B, int64_t* out_i64, double* dice_sum,
                             int32_t* tp, int32_t* fp, double* dice) {
    for (int64_t p = 0; p < planes; ++p) {
        const int32_t* h = plane_hist + p * 2 * B;
        const CurveSums s = curve_suffix(h, h + B, B, tp, fp);
        for (int k = 0; k <= B; ++k) dice[k] = curve_dice(tp[k], fp[k], s.P);
        curve_stat_row(s, tp, fp, curve_best(dice, B), out_i64 + p * CURVE_STAT_FIELDS);
        for (int k = 0; k <= B; ++k) dice_sum[k] += dice[k];
    }
}
