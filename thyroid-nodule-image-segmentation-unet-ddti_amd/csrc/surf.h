// Surface-distance metrics of Trainer.test (HD, HD95, ASSD: MedPy's hd / hd95 / assd at
// connectivity 1, in pixels), as per-pixel functions and steps shared by the device kernels
// (kernels_surf.hip) and the host hook unet_surface_stats_host (the edt.h pattern: testable
// without a GPU).
//
// Masks.  P = surf_pred(logits[n, 0]) and G = surf_target(targets[n, 0]); these two functions
// ARE the mask readout of unet_mask_counts (kernels_misc.hip calls them), so the surfaces are
// those of the masks the confusion counts are made of.
//
// Border.  border(A) = A & ~binary_erosion(A, generate_binary_structure(2, 1)) with scipy's
// border_value = 0: a foreground pixel is a border pixel iff one of its 4 neighbours is
// background or lies outside the image.  A mask with a foreground pixel has a border pixel
// (its first pixel in raster order has nothing above it), so "no border pixel" == "empty mask".
//
// Distances.  d_PG = { d2_G[p] : p in border(P) }, d2_G the exact int32 squared Euclidean
// distance to the nearest pixel of border(G): edt.h's column and row passes over the uint8 border
// plane, without its final float sqrt.  d_GP likewise.  The distance is sqrt((double)d2).
//
// Per sample: the counts n_PG, n_GP, the float64 sums of the distances, max d2 over both
// directions, and the two order statistics d2_lo, d2_hi of the union multiset that numpy's
// percentile(..., 95) (linear) interpolates between: surf_ranks.  They are selected exactly by a
// most-significant-digit radix select on the uint32 keys, SURF_DIGIT_BITS bits per pass: a pass
// histograms the digit of the keys that still carry the chosen prefix, surf_select_step picks
// the bucket of the wanted rank and reduces the rank to a rank inside that bucket.  lo and hi
// are two such states advanced over the same passes.
//
// A sample whose P or G is empty is undefined (MedPy raises): defined = 0, every other field 0,
// and neither the row pass nor the gather runs for it (edt.h's empty-mask rule is never used).
#pragma once
#include "edt.h"

#define SURF_HD EDT_HD

// ---- the mask readout of unet_mask_counts (utils/trainer.py:217-220): surf_pred, surf_target_u8,
// surf_target, in mask_readout.h so that a host-only build shares the one definition ----
#define READOUT_HD SURF_HD
#include "mask_readout.h"

// ---- border ----
// fg(i, j): the mask inside the image
template <typename F>
SURF_HD bool surf_border(F fg, int i, int j, int H, int W) {
    if (!fg(i, j)) return false;
    const bool inner = i > 0 && fg(i - 1, j) && i + 1 < H && fg(i + 1, j) && j > 0 && fg(i, j - 1) &&
                       j + 1 < W && fg(i, j + 1);
    return !inner;
}

// ---- gather ----
struct SurfAcc {
    int n;       // surface pixels
    int max_d2;  // their largest squared distance
    double sum;  // sum of sqrt(d2)
};
SURF_HD SurfAcc surf_acc_zero() { return SurfAcc{0, 0, 0.0}; }
SURF_HD void surf_acc_add(SurfAcc& a, int d2) {
    a.n += 1;
    a.max_d2 = d2 > a.max_d2 ? d2 : a.max_d2;
    a.sum += sqrt((double)d2);
}
// b after a (partials are merged in index order)
SURF_HD SurfAcc surf_acc_merge(const SurfAcc& a, const SurfAcc& b) {
    return SurfAcc{a.n + b.n, a.max_d2 > b.max_d2 ? a.max_d2 : b.max_d2, a.sum + b.sum};
}

// ---- selection ----
// numpy's linear percentile of n >= 1 sorted values: position 0.95 (n - 1) in float64 (numpy
// forms the same product), between the order statistics lo = floor and hi = ceil
SURF_HD void surf_ranks(int n, int& lo, int& hi) {
    const double pos = 0.95 * (double)(n - 1);
    lo = (int)floor(pos);
    hi = (int)ceil(pos);
}

constexpr int SURF_DIGIT_BITS = 8;
constexpr int SURF_BINS = 1 << SURF_DIGIT_BITS;

// shift of the most significant digit a key <= max_key can have set (0 for max_key < SURF_BINS):
// the passes run at shift, shift - SURF_DIGIT_BITS, ..., 0
SURF_HD int surf_top_shift(int max_key) {
    int s = 0;
    while (((uint32_t)max_key >> s) >= (uint32_t)SURF_BINS) s += SURF_DIGIT_BITS;
    return s;
}

struct SurfSel {
    uint32_t prefix;  // the digits chosen so far, in place (lower bits 0)
    int rank;         // wanted rank among the keys that carry the prefix
};
// does key carry the digits sel chose above `shift`?  (shift + SURF_DIGIT_BITS <= 24 < 32)
SURF_HD bool surf_sel_match(const SurfSel& s, uint32_t key, int shift) {
    return (key >> (shift + SURF_DIGIT_BITS)) == (s.prefix >> (shift + SURF_DIGIT_BITS));
}
SURF_HD int surf_digit(uint32_t key, int shift) { return (int)((key >> shift) & (SURF_BINS - 1)); }
// hist: the digit histogram (at `shift`) of the keys matching s.  The bucket holding rank
// s.rank becomes the next digit; the rank turns into a rank inside that bucket.  No early exit,
// so the SURF_BINS loads are independent of the running sum.
SURF_HD void surf_select_step(SurfSel& s, const int* hist, int shift) {
    int cum = 0, bucket = SURF_BINS - 1, below = 0;
    bool found = false;
    for (int b = 0; b < SURF_BINS; ++b) {
        const int c = hist[b];
        if (!found && s.rank < cum + c) {
            found = true;
            bucket = b;
            below = cum;
        }
        cum += c;
    }
    s.prefix |= (uint32_t)bucket << shift;
    s.rank -= below;
}
