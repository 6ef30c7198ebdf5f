// Flip / rotation test-time augmentation: the eight dihedral views of a square plane, their
// inverses and the merge of the per-view logits, as index maps and a per-element accumulator
// shared by the device kernels (kernels_tta.hip) and the host twins unet_tta_views_host /
// unet_tta_merge_host (the edt.h pattern: testable without a GPU).
//
// Views.  View k in 0..7 has bits h = k & 1, v = (k >> 1) & 1, t = (k >> 2) & 1 and is
//     T_k(x): y = x;  if t: y = y.swapaxes(-1, -2);  if v: y = y[..., ::-1, :];  if h: y = y[..., ::-1]
// so k = 0 is the identity, 1..3 the flips, 4 the transpose, 5 and 6 the two quarter turns (each
// the other's inverse) and 7 the anti-transpose: the dihedral group D4.  A view with t needs
// H == W.  As an index map T_k(x)[i, j] = x[tta_fwd(k, i, j)].
//
// Inverse.  T_k^-1 undoes h, then v, then t: T_k^-1(L)[i, j] = L[tta_inv(k, i, j)] with
//     t = 0: (v ? H-1-i : i, h ? W-1-j : j)        t = 1: (v ? H-1-j : j, h ? W-1-i : i).
//
// View sets.  A bit mask `views` (bit k); K = popcount; the views are taken in ascending k, view
// number q being the q-th set bit.  The stacked tensor is view-major: plane (q N + n) C + c.
//
// Merge.  Per output element, with x_q the logit of view q at tta_inv(k_q, i, j):
//     mode 0 (logit): score = (x_0 + x_1 + ... + x_{K-1}) / (float)K, mask = surf_pred(score)
//     mode 1 (prob):  score = (p_0 + ... + p_{K-1}) / (float)K, p_q = 1.f / (1.f + expf(-x_q)),
//                     mask = score > 0.5f
//     votes = the number of views with surf_pred(x_q) (0..K)
// The sum is a float32 sum in ascending q that starts from the first term (no 0 + x_0), every
// operation rounded on its own (the translation unit is built with -ffp-contract=off, as aug.h's
// is) and the division is the correctly rounded f32 division, so the device, the host twin and a
// NumPy float32 restatement agree bit for bit in mode 0; in mode 1 they differ by expf alone.
#pragma once
#include "surf.h"

#define TTA_HD SURF_HD

constexpr uint32_t TTA_ALL_VIEWS = 0xFFu;
constexpr int TTA_MAX_VIEWS = 8;
constexpr int TTA_MODE_LOGIT = 0;
constexpr int TTA_MODE_PROB = 1;

TTA_HD bool tta_h(int k) { return (k & 1) != 0; }
TTA_HD bool tta_v(int k) { return (k & 2) != 0; }
TTA_HD bool tta_t(int k) { return (k & 4) != 0; }

// the ascending list of the views of a mask
struct TtaViews {
    int K;
    int k[TTA_MAX_VIEWS];
};
TTA_HD TtaViews tta_view_list(uint32_t views) {
    TtaViews l{};
    for (int k = 0; k < TTA_MAX_VIEWS; ++k)
        if (views >> k & 1u) l.k[l.K++] = k;
    return l;
}

// T_k(x)[i, j] = x[si, sj]
TTA_HD void tta_fwd(int k, int i, int j, int H, int W, int& si, int& sj) {
    const int a = tta_v(k) ? H - 1 - i : i;
    const int b = tta_h(k) ? W - 1 - j : j;
    si = tta_t(k) ? b : a;
    sj = tta_t(k) ? a : b;
}
// T_k^-1(L)[i, j] = L[si, sj]
TTA_HD void tta_inv(int k, int i, int j, int H, int W, int& si, int& sj) {
    if (tta_t(k)) {
        si = tta_v(k) ? H - 1 - j : j;
        sj = tta_h(k) ? W - 1 - i : i;
    } else {
        si = tta_v(k) ? H - 1 - i : i;
        sj = tta_h(k) ? W - 1 - j : j;
    }
}

// ---- merge ----
TTA_HD float tta_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

struct TtaAcc {
    float sum;
    int votes;
};
// view q's logit x joins the running sum (q ascending from 0)
TTA_HD void tta_acc_add(TtaAcc& a, int q, float x, int mode) {
    const float term = mode == TTA_MODE_PROB ? tta_sigmoid(x) : x;
    a.sum = q == 0 ? term : a.sum + term;
    a.votes = (q == 0 ? 0 : a.votes) + (surf_pred(x) ? 1 : 0);
}
TTA_HD float tta_score(const TtaAcc& a, int K) { return a.sum / (float)K; }
TTA_HD bool tta_mask(float score, int mode) { return mode == TTA_MODE_PROB ? score > 0.5f : surf_pred(score); }
