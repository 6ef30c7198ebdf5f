// Connected components of the Trainer.test masks, the post-processing built on them (drop small
// components, keep the largest, fill holes) and the lesion-level hit counts, as per-pixel rules
// shared by the device kernels (kernels_cc.hip) and the host hooks unet_components_host /
// unet_postprocess_host / unet_lesion_stats_host (the edt.h / surf.h pattern: testable without a
// GPU).  Everything is integer, so the result does not depend on the order of the atomics.
//
// Foreground.  cc_fg(src, kind, .): kind 0 a uint8 plane (nonzero), kind 1 float logits through
// surf_pred, kind 2 float targets through surf_target -- the masks unet_mask_counts counts.
// Channel 0 of an (N, C, H, W) tensor is read.  Kind 3 (internal) is the complement of a uint8
// plane: the background that fill_holes labels.
//
// Labels.  scipy.ndimage.label numbers the components in raster order of their first pixel:
// label = 1 + the rank, among the sample's components, of the component's smallest linear index.
// That index is what the union-find converges to: every link L[a] = b has b < a (cc_union links
// the larger root below the smaller), so the root of a component is its smallest pixel, find
// follows strictly decreasing indices, and union retries only from the smaller index an
// atomicMin handed back.  Connectivity 1 is generate_binary_structure(2, 1) (4 neighbours),
// connectivity 2 np.ones((3, 3)) (8 neighbours).
//
// Post-processing of the foreground A of one sample, in this order:
//   1. components with area < min_area leave (cc_keep; min_area <= 1 removes nothing);
//   2. keep_largest keeps the largest remaining one, on equal areas the lowest label: the maximum
//      of cc_key = (area << 32) | (0xFFFFFFFF - root), np.argmax(np.bincount(lab.ravel())[1:]) + 1;
//   3. fill_holes is scipy's binary_fill_holes with its default structure: the complement is
//      labelled at connectivity 1 (whatever the foreground connectivity), the background
//      components that touch the image border stay, every other background pixel is filled.
//
// Lesion statistics of a prediction P against the targets G: the component counts of both, the
// G components holding a pixel of P (gt_hit) and the P components holding a pixel of G (pred_hit).
#pragma once
#include "surf.h"

#define CC_HD EDT_HD

constexpr int CC_TILE_W = 64;  // a tile row is one wave: its runs come from one ballot

enum { CC_KIND_U8 = 0, CC_KIND_LOGITS = 1, CC_KIND_TARGETS = 2, CC_KIND_U8_ZERO = 3 };

// off: element offset of the pixel in src (channel 0 of its sample)
CC_HD bool cc_fg(const void* src, int kind, int64_t off) {
    switch (kind) {
        case CC_KIND_U8: return ((const uint8_t*)src)[off] != 0;
        case CC_KIND_LOGITS: return surf_pred(((const float*)src)[off]);
        case CC_KIND_TARGETS: return surf_target(((const float*)src)[off]);
        default: return ((const uint8_t*)src)[off] == 0;
    }
}

// root of p: L[r] == r.  Every link points at a smaller index, so the walk ends.
CC_HD int cc_find(const int* L, int p) {
    int q = __atomic_load_n(&L[p], __ATOMIC_RELAXED);  // others may be linking meanwhile
    while (q != p) {
        p = q;
        q = __atomic_load_n(&L[p], __ATOMIC_RELAXED);
    }
    return p;
}

// Lock-free union by smaller index.  amin(slot, v) stores min(*slot, v) atomically and returns
// the old value (a plain minimum on the host).  old == a: a was a root and now hangs below b.
// Otherwise somebody linked a below old < a first (and our minimum may have replaced that link):
// a's component still has to meet b's, which union(old, b) does -- from a strictly smaller index.
template <typename AMin>
CC_HD void cc_union(int* L, int a, int b, AMin amin) {
    for (;;) {
        a = cc_find(L, a);
        b = cc_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = amin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

// first column of the run of set bits of m that holds bit x (x in [0, 64), bit x set)
CC_HD int cc_run_start(uint64_t m, int x) {
    const uint64_t below = ~m & (((uint64_t)1 << x) - 1);
    if (!below) return 0;
#ifdef __HIP_DEVICE_COMPILE__
    return 64 - __clzll((long long)below);
#else
    return 64 - __builtin_clzll(below);
#endif
}

// ---- post-processing ----
CC_HD bool cc_keep(int area, int64_t min_area) { return (int64_t)area >= min_area; }
// larger area wins, then the smaller root (= the lower label); 0 is below every component's key
CC_HD uint64_t cc_key(int area, int root) {
    return ((uint64_t)(uint32_t)area << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)root);
}
// does the pixel whose component has `root` and `area` stay after steps 1 and 2?
CC_HD bool cc_stays(int area, int root, int64_t min_area, bool keep_largest, uint64_t best) {
    return cc_keep(area, min_area) && (!keep_largest || best == cc_key(area, root));
}
// a pixel on the image border: its background component is not a hole
CC_HD bool cc_on_border(int i, int j, int H, int W) { return i == 0 || j == 0 || i == H - 1 || j == W - 1; }
