// Lesion morphometry: one row of sixteen integers per connected component of a label plane (the
// planes unet_components writes), as rules shared by the device kernels (kernels_morph.hip) and the
// host twin unet_morphometry_host (the curve.h pattern: testable without a GPU).  The header also
// compiles for the host alone (MORPH_HOST_ONLY: no HIP header).  Everything is integer: sums, minima
// and maxima, so the result does not depend on the order of the atomics and "equal" is bit-equal.
//
// Input.  labels int32 [N, H, W], 0 (or anything <= 0) background, l >= 1 a component; count int32
// [N], the number of components of each sample.  Output.  table int64 [N, max_rows, 16], the row of
// label l at index l - 1.  Rows at or beyond count[n] are zero; a label above max_rows is dropped
// without a memory access (count tells the caller).  x is the column, y the row, sums over the
// pixels of the component:
//    0      area   sum 1
//    1, 2   sx, sy             3, 4, 5  sxx, sxy, syy
//    6..9   x0, y0, x1, y1     the inclusive bounding box
//   10..13  q1, q2, qd, q3     bit-quad counts of the component's own indicator (label == l) over
//                              the (H + 1) (W + 1) 2 x 2 windows of the plane padded with a zero
//                              border: one pixel set, two edge-adjacent, two diagonal, three.  (Four
//                              set follows from q1 + 2 q2 + 2 qd + 3 q3 + 4 q4 = 4 area.)
//   14      d2max  max over the component's pixel pairs of dx^2 + dy^2 (squared maximum Feret
//                  diameter between pixel centres; 0 for one pixel)
//   15      first  smallest linear index y W + x of the component
//
// Bounds.  H, W <= MORPH_MAX_SIDE = 4096: area <= 2^24, coordinates < 2^12, so sx, sy < 2^36 and
// sxx, sxy, syy < 2^48, and every term of the closed forms of a run (at most 4096 pixels) is below
// 2^37: far inside int64.  The central moments area * sxx - sx^2 reach 2^72 and are left to the
// caller's wide integers (shape_descriptors uses Python ints).  d2max <= 2 * 4095^2 < 2^25.
//
// Phases (device; the host twin applies the same rules one plane at a time):
//   reduce   one pass over the (H + 1) x (W + 1) window positions in 64-column tiles.  A tile row is
//            one wave: the runs of equal labels come from one ballot and the leader lane of a run adds
//            its closed-form sums (morph_run_sums); the lane at window position (y, x) classifies the
//            window whose lower right pixel is (y, x) (morph_quad), its left neighbours by a shuffle
//            (lane 0 from the halo column), its upper ones kept from the wave's previous row.
//   extent   a connected component occupies every row of its box, and for two rows the largest |dx|
//            is between an extreme pixel of each, so the farthest pair lies among the row-extreme
//            pixels.  The box heights of a sample's labels are scanned into offsets, then every run
//            leader maxes W - x_first and x_last + 1 into its (component, row) slot (both start at 0,
//            so the scratch is cleared by a memset).  A row holds at most ceil(W / 2) components, so a
//            sample needs at most H ceil(W / 2) slots.
//   feret    one block per (sample, row of the table): over the pairs (i <= j) of the component's
//            rows, d2 = max(xmax_j - xmin_i, xmax_i - xmin_j)^2 + (j - i)^2, max-reduced in integers.
//            The same block zeroes a row without pixels.
#pragma once
#include <stdint.h>

#include <vector>

#ifdef MORPH_HOST_ONLY
#define MORPH_HD inline
#else
#include <hip/hip_runtime.h>
#define MORPH_HD __host__ __device__ __forceinline__
#endif

constexpr int MORPH_FIELDS = 16;
constexpr int MORPH_MAX_SIDE = 4096;
constexpr int MORPH_TILE_W = 64;  // a tile row is one wave
enum {
    MF_AREA = 0, MF_SX, MF_SY, MF_SXX, MF_SXY, MF_SYY, MF_X0, MF_Y0, MF_X1, MF_Y1,
    MF_Q1, MF_Q2, MF_QD, MF_Q3, MF_D2MAX, MF_FIRST
};
// what a minimum field (x0, y0, first) holds before its first pixel
constexpr int64_t MORPH_MIN_INIT = INT64_MAX;

MORPH_HD bool morph_min_field(int f) { return f == MF_X0 || f == MF_Y0 || f == MF_FIRST; }
MORPH_HD bool morph_max_field(int f) { return f == MF_X1 || f == MF_Y1; }

// null, or what is wrong (the first five are UNET_ERR_INVALID, the last UNET_ERR_SHAPE)
inline const char* morph_args_invalid(const void* labels, const void* count, const void* table, int N, int H,
                                      int W, int64_t max_rows) {
    if (!labels || !count || !table) return "labels, count and table must not be null";
    if (N < 1 || H < 1 || W < 1 || max_rows < 1) return "N, H, W, max_rows >= 1";
    if ((int64_t)H * W >= (int64_t)1 << 31) return "H * W must be below 2^31";
    return nullptr;
}
inline bool morph_shape_ok(int H, int W) { return H <= MORPH_MAX_SIDE && W <= MORPH_MAX_SIDE; }
// (component, row) slots of one sample
MORPH_HD int64_t morph_extent_slots(int H, int W) { return (int64_t)H * ((W + 1) / 2); }

// the six sums {area, sx, sy, sxx, sxy, syy} of the n pixels of row y that start at column x0
MORPH_HD void morph_run_sums(int x0, int n, int y, int64_t s[6]) {
    const int64_t n_ = n, x = x0, y_ = y;
    const int64_t t = n_ * (n_ - 1) / 2;                   // sum of i, i < n
    const int64_t t2 = (n_ - 1) * n_ * (2 * n_ - 1) / 6;   // sum of i^2
    s[0] = n_;
    s[1] = n_ * x + t;
    s[2] = n_ * y_;
    s[3] = n_ * x * x + 2 * x * t + t2;
    s[4] = y_ * s[1];
    s[5] = n_ * y_ * y_;
}

// The 2 x 2 window  a b / c d  (labels; <= 0 background): for every distinct label in it, the field
// its own indicator adds one to.  Connected components put two labels into one window only as a
// diagonal pair at connectivity 1 (two q1); the rule itself holds for any label plane.
struct MorphQuad {
    int n;
    int label[4], field[4];
};
// m: the indicator of one label, bit 0 = a, 1 = b, 2 = c, 3 = d (m != 0); -1 for the full window
MORPH_HD int morph_quad_field(int m) {
    const int k = (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1);
    if (k == 1) return MF_Q1;
    if (k == 3) return MF_Q3;
    if (k == 4) return -1;
    return (m == 9 || m == 6) ? MF_QD : MF_Q2;
}
MORPH_HD MorphQuad morph_quad(int a, int b, int c, int d) {
    const int v[4] = {a, b, c, d};
    MorphQuad q;
    q.n = 0;
    for (int i = 0; i < 4; ++i) {
        if (v[i] <= 0) continue;
        int m = 0;
        bool seen = false;
        for (int j = 0; j < 4; ++j) {
            if (v[j] != v[i]) continue;
            if (j < i) seen = true;
            m |= 1 << j;
        }
        if (seen) continue;
        const int f = morph_quad_field(m);
        if (f < 0) continue;
        q.label[q.n] = v[i];
        q.field[q.n] = f;
        ++q.n;
    }
    return q;
}

// the pixels of the run that starts at `lane`, where bit k of cont says that lane k continues the
// run of lane k - 1 (same positive label)
MORPH_HD int morph_run_len(uint64_t cont, int lane) {
    const uint64_t rest = lane >= 63 ? 0 : cont >> (lane + 1);  // bit 63 - lane and above are zero
#ifdef __HIP_DEVICE_COMPILE__
    return __ffsll((long long)~rest);
#else
    return __builtin_ffsll((long long)~rest);
#endif
}

// the extents of a (component, row) slot as the extent pass stores them, both maxima over zero
MORPH_HD int morph_extent_lo(int W, int x_first) { return W - x_first; }  // in 1..W
MORPH_HD int morph_extent_hi(int x_last) { return x_last + 1; }          // in 1..W
// squared distance of the farthest pair between two rows dy apart whose pixels span [xmin, xmax]
MORPH_HD int morph_row_pair_d2(int xmin_i, int xmax_i, int xmin_j, int xmax_j, int dy) {
    const int a = xmax_j - xmin_i, b = xmax_i - xmin_j;
    const int dx = a > b ? a : b;
    return dx * dx + dy * dy;
}

// ---- the host twin (unet_morphometry_host): the rules above, one plane at a time ----

inline void morphometry_host(const int32_t* labels, const int32_t* count, int N, int H, int W, int64_t max_rows,
                             int64_t* table) {
    const int64_t hw = (int64_t)H * W;
    std::vector<int> lo, hi;
    for (int n = 0; n < N; ++n) {
        const int32_t* L = labels + n * hw;
        int64_t* T = table + (int64_t)n * max_rows * MORPH_FIELDS;
        const int64_t K = count[n] < 0 ? 0 : ((int64_t)count[n] < max_rows ? (int64_t)count[n] : max_rows);
        for (int64_t r = 0; r < max_rows; ++r)
            for (int f = 0; f < MORPH_FIELDS; ++f) T[r * MORPH_FIELDS + f] = morph_min_field(f) ? MORPH_MIN_INIT : 0;
        auto at = [&](int y, int x) { return y >= 0 && y < H && x >= 0 && x < W ? L[(int64_t)y * W + x] : 0; };
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W;) {
                const int l = L[(int64_t)y * W + x];
                int e = x + 1;
                if (l > 0)
                    while (e < W && L[(int64_t)y * W + e] == l) ++e;
                if (l > 0 && (int64_t)l <= max_rows) {
                    int64_t* row = T + (int64_t)(l - 1) * MORPH_FIELDS;
                    int64_t s[6];
                    morph_run_sums(x, e - x, y, s);
                    for (int f = 0; f < 6; ++f) row[f] += s[f];
                    const int64_t first = (int64_t)y * W + x;
                    if (x < row[MF_X0]) row[MF_X0] = x;
                    if (y < row[MF_Y0]) row[MF_Y0] = y;
                    if (e - 1 > row[MF_X1]) row[MF_X1] = e - 1;
                    if (y > row[MF_Y1]) row[MF_Y1] = y;
                    if (first < row[MF_FIRST]) row[MF_FIRST] = first;
                }
                x = e;
            }
        for (int y = 0; y <= H; ++y)
            for (int x = 0; x <= W; ++x) {
                const MorphQuad q = morph_quad(at(y - 1, x - 1), at(y - 1, x), at(y, x - 1), at(y, x));
                for (int k = 0; k < q.n; ++k)
                    if ((int64_t)q.label[k] <= max_rows) T[(int64_t)(q.label[k] - 1) * MORPH_FIELDS + q.field[k]] += 1;
            }
        // extents of the rows of every box, then the farthest pair
        for (int64_t r = 0; r < max_rows; ++r) {
            int64_t* row = T + r * MORPH_FIELDS;
            if (r >= K || row[MF_AREA] <= 0) {
                for (int f = 0; f < MORPH_FIELDS; ++f) row[f] = 0;
                continue;
            }
            const int y0 = (int)row[MF_Y0], h = (int)(row[MF_Y1] - row[MF_Y0]) + 1;
            lo.assign((size_t)h, 0);
            hi.assign((size_t)h, 0);
            for (int i = 0; i < h; ++i)
                for (int x = (int)row[MF_X0]; x <= (int)row[MF_X1]; ++x)
                    if (L[(int64_t)(y0 + i) * W + x] == (int)(r + 1)) {
                        if (morph_extent_lo(W, x) > lo[i]) lo[i] = morph_extent_lo(W, x);
                        if (morph_extent_hi(x) > hi[i]) hi[i] = morph_extent_hi(x);
                    }
            int best = 0;
            for (int i = 0; i < h; ++i) {
                if (hi[i] == 0) continue;  // a row without a pixel: not a connected component's
                for (int j = i; j < h; ++j) {
                    if (hi[j] == 0) continue;
                    const int d2 = morph_row_pair_d2(W - lo[i], hi[i] - 1, W - lo[j], hi[j] - 1, j - i);
                    if (d2 > best) best = d2;
                }
            }
            row[MF_D2MAX] = best;
        }
    }
}
