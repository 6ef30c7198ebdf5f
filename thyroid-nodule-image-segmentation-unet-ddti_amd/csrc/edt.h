// Exact Euclidean distance transform of the BoundaryLoss targets (reference
// models/loss.py:55-61: scipy.ndimage.distance_transform_edt(1 - targets.astype(uint8))), as
// 1-D passes shared by the device kernels (kernels_edt.hip) and the host hook unet_edt_host
// (the unet_x3_split_host pattern: the algorithm is testable without a GPU).
//
// Site rule.  The reference casts the targets to uint8 and transforms 1 - gt, so a pixel is a
// feature site (distance 0) iff (uint8)t == 1, i.e. 1 <= t < 2 for every t in [0, 256): a soft
// mixup target below 1 is NOT a site, 1.5 is, 2.0 and 255.0 are not.  The comparison form is
// used so that values outside [0, 256) (where the cast is undefined) are simply not sites.
//
// Distance.  dist(i, j) = sqrt(min over sites (y, x) of (i - y)^2 + (j - x)^2).  The minimum
// is formed in int32 (separable: column pass -> vertical distance g to the nearest site of the
// column, row pass -> min_k (j - k)^2 + g[k]^2), so it is exact; with max(H, W) <= EDT_MAX_SIDE
// it stays below 2^24 and the square root is taken in double and rounded to float, which is
// scipy's own float64 result cast to float32 (and, as 53 >= 2 * 24 + 2, also the correctly
// rounded f32 square root).
//
// Empty-mask rule.  For a sample without any site scipy (1.15) returns the distance to a
// virtual site at row -1, column 0: dist(i, j) = sqrt((i + 1)^2 + j^2) (observed for 1x7, 7x1,
// 16x16, 32x48, 64x16, 256^2 and 512^2 inputs).  The reference trains on exactly that, so the
// row pass writes it for samples whose any-site flag is clear.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define EDT_HD __host__ __device__ __forceinline__

constexpr int EDT_MAX_SIDE = 2048;
// g of a column without a site: EDT_INF^2 + (EDT_MAX_SIDE - 1)^2 < 2^27 stays inside int32, and
// a sample with a site always has a finite candidate <= 2 * (EDT_MAX_SIDE - 1)^2 < EDT_INF^2
constexpr int EDT_INF = 8192;

EDT_HD bool edt_site(float t) { return t >= 1.f && t < 2.f; }

// One column of one sample: t / g2 point at row 0 of the column, consecutive rows `stride`
// elements apart.  Writes g^2 (g = rows to the nearest site of the column, EDT_INF if none)
// and returns whether the column holds a site.  Both sweeps load EDT_UNROLL rows before they
// walk the dependent chain over them, so the loads of a batch are in flight together.  T is
// float (the BoundaryLoss targets) or uint8_t (the 0 / 1 border planes of surf.h: 1 is a site).
constexpr int EDT_UNROLL = 8;
template <typename T>
EDT_HD bool edt_column(const T* __restrict__ t, int* __restrict__ g2, int H, int64_t stride) {
    int d = EDT_INF;
    for (int i0 = 0; i0 < H; i0 += EDT_UNROLL) {  // down: distance to the nearest site above
        float v[EDT_UNROLL];
#pragma unroll
        for (int u = 0; u < EDT_UNROLL; ++u) v[u] = i0 + u < H ? (float)t[(i0 + u) * stride] : 0.f;
#pragma unroll
        for (int u = 0; u < EDT_UNROLL; ++u)
            if (i0 + u < H) {
                d = edt_site(v[u]) ? 0 : (d < EDT_INF ? d + 1 : EDT_INF);
                g2[(i0 + u) * stride] = d;
            }
    }
    const bool any = d < EDT_INF;  // H <= EDT_MAX_SIDE < EDT_INF: a site above the last row
    d = EDT_INF;
    for (int i0 = H - 1; i0 >= 0; i0 -= EDT_UNROLL) {  // up: ... or below
        int a[EDT_UNROLL];
#pragma unroll
        for (int u = 0; u < EDT_UNROLL; ++u) a[u] = i0 - u >= 0 ? g2[(i0 - u) * stride] : 0;
#pragma unroll
        for (int u = 0; u < EDT_UNROLL; ++u)
            if (i0 - u >= 0) {
                d = a[u] == 0 ? 0 : (d < EDT_INF ? d + 1 : EDT_INF);
                const int g = a[u] < d ? a[u] : d;
                g2[(i0 - u) * stride] = g * g;
            }
    }
    return any;
}

// Squared distance of pixel j of a row from the row's g^2: min_k (j - k)^2 + g2[k], scanning
// outward from j and stopping once (j - k)^2 alone reaches the best value so far.
EDT_HD int edt_row_min(const int* __restrict__ g2, int W, int j) {
    int best = g2[j];
    for (int r = 1; r < W; ++r) {
        const int rr = r * r;
        if (rr >= best) break;
        const int a = j - r, b = j + r;
        if (a < 0 && b >= W) break;
        if (a >= 0) {
            const int v = rr + g2[a];
            best = v < best ? v : best;
        }
        if (b < W) {
            const int v = rr + g2[b];
            best = v < best ? v : best;
        }
    }
    return best;
}

// sqrt of an exact squared distance d2 < 2^24 (see the header comment)
EDT_HD float edt_sqrt(int d2) { return (float)sqrt((double)d2); }

// the empty-mask rule
EDT_HD float edt_empty(int i, int j) { return edt_sqrt((i + 1) * (i + 1) + j * j); }
