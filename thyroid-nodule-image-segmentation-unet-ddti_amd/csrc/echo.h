// Lesion echogenicity and texture: what the grey values under every connected component of a label
// plane (the planes unet_components writes) and in a band around it look like, as one row of integer
// counts per component.  Rules shared by the device kernel (kernels_echo.hip) and the host twin
// unet_lesion_echo_host (the morph.h pattern: testable without a GPU).  The header also compiles for
// the host alone (ECHO_HOST_ONLY: no HIP header).  Everything is an integer count, so the result does
// not depend on the order of the atomics and "equal" is bit-equal.
//
// Input.  gray uint8 [N, H, W]; labels int32 [N, H, W], anything <= 0 background, l >= 1 a component;
// count int32 [N]; levels G in {8, 16, 32}; ring w in 0..16.  Output.  table int32 [N, max_rows,
// 512 + G G], the row of label l at index l - 1.  Rows at or beyond count[n] are zero and a label
// above min(count[n], max_rows) is dropped without a memory access (count tells the caller).
//     0..255   lesion histogram: column g counts the pixels with label l and grey value g
//   256..511   ring histogram: the owner of a background pixel p is the smallest positive label in
//              the (2 w + 1) x (2 w + 1) window around p clipped to the plane (chessboard distance
//              <= w, ties to the lower label); column 256 + g of the owner's row counts p.  w = 0
//              leaves these columns zero.
//   512...     pooled co-occurrence counts at the quantised level q(g) = (g G) >> 8: for every pixel
//              p and each offset (dy, dx) in (0, 1), (1, 1), (1, 0), (1, -1), if the neighbour is
//              inside the plane and both carry the same label l, entry [q(p)][q(neighbour)] of row l
//              gains one.  Pairs are ordered and counted once, the four directions summed; the
//              caller symmetrises.
//
// Bounds.  H, W <= MORPH_MAX_SIDE = 4096: a histogram column is at most H W <= 2^24 and a
// co-occurrence entry at most 4 H W <= 2^26, so int32 holds every count.
//
// Device: one block per 64 x ECHO_TH tile.  The label tile is staged in LDS with a halo of max(w, 1)
// and its grey bytes with a halo of one; the ring owner of the tile's pixels is a separable minimum
// over the positive labels (rows, then columns) in LDS; the counts go through a small label-keyed LDS
// table (a few slots of 512 + G G counters, flushed with global integer atomics), labels beyond
// the slots straight to global atomics.  The host twin applies the same rules one plane at a time.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(ECHO_HOST_ONLY) && !defined(MORPH_HOST_ONLY)
#define MORPH_HOST_ONLY  // MORPH_MAX_SIDE and morph_shape_ok, without the HIP header
#endif
#include "morph.h"

#ifdef ECHO_HOST_ONLY
#define ECHO_HD inline
#else
#define ECHO_HD __host__ __device__ __forceinline__
#endif

constexpr int ECHO_HIST = 256;            // bins of each of the two histograms
constexpr int ECHO_GLCM0 = 2 * ECHO_HIST;  // first co-occurrence column
constexpr int ECHO_MAX_RING = 16;
constexpr int ECHO_MAX_LEVELS = 32;
constexpr int ECHO_OFFSETS = 4;
constexpr int ECHO_NO_OWNER = INT32_MAX;  // what a window without a positive label gives

ECHO_HD bool echo_levels_ok(int G) { return G == 8 || G == 16 || G == 32; }
ECHO_HD int echo_fields(int G) { return ECHO_GLCM0 + G * G; }
ECHO_HD int echo_quant(int g, int G) { return (g * G) >> 8; }
ECHO_HD int echo_pair_col(int ga, int gb, int G) { return ECHO_GLCM0 + echo_quant(ga, G) * G + echo_quant(gb, G); }
ECHO_HD int echo_dy(int k) { return k == 0 ? 0 : 1; }
ECHO_HD int echo_dx(int k) { return k == 3 ? -1 : (k == 2 ? 0 : 1); }
// a label as the ownership minimum sees it
ECHO_HD int echo_pos(int l) { return l > 0 ? l : ECHO_NO_OWNER; }
// the labels of sample n that have a row: 1..echo_rows_used
ECHO_HD int64_t echo_rows_used(int count_n, int64_t max_rows) {
    return count_n < 0 ? 0 : ((int64_t)count_n < max_rows ? (int64_t)count_n : max_rows);
}

// null, or what is wrong (UNET_ERR_INVALID; the side limit is echo_shape_ok, UNET_ERR_SHAPE)
inline const char* echo_args_invalid(const void* gray, const void* labels, const void* count, const void* table,
                                     int N, int H, int W, int64_t max_rows, int levels, int ring) {
    if (!gray || !labels || !count || !table) return "gray, labels, count and table must not be null";
    if (N < 1 || H < 1 || W < 1 || max_rows < 1) return "N, H, W, max_rows >= 1";
    if ((int64_t)H * W >= (int64_t)1 << 31) return "H * W must be below 2^31";
    if (!echo_levels_ok(levels)) return "levels must be 8, 16 or 32";
    if (ring < 0 || ring > ECHO_MAX_RING) return "ring must be in 0..16";
    return nullptr;
}
inline bool echo_shape_ok(int H, int W) { return morph_shape_ok(H, W); }

// ---- the host twin (unet_lesion_echo_host): the rules above, one plane at a time ----

inline void echo_host(const uint8_t* gray, const int32_t* labels, const int32_t* count, int N, int H, int W,
                      int64_t max_rows, int G, int w, int32_t* table) {
    const int64_t hw = (int64_t)H * W;
    const int F = echo_fields(G);
    std::vector<int> rowmin;
    if (w > 0) rowmin.resize((size_t)hw);
    for (int n = 0; n < N; ++n) {
        const int32_t* L = labels + n * hw;
        const uint8_t* Gy = gray + n * hw;
        int32_t* T = table + (int64_t)n * max_rows * F;
        const int64_t K = echo_rows_used(count[n], max_rows);
        for (int64_t i = 0; i < max_rows * F; ++i) T[i] = 0;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int l = L[(int64_t)y * W + x];
                if (l <= 0 || (int64_t)l > K) continue;
                const int g = Gy[(int64_t)y * W + x];
                int32_t* row = T + (int64_t)(l - 1) * F;
                row[g] += 1;
                for (int k = 0; k < ECHO_OFFSETS; ++k) {
                    const int yy = y + echo_dy(k), xx = x + echo_dx(k);
                    if (yy >= H || xx < 0 || xx >= W) continue;
                    if (L[(int64_t)yy * W + xx] == l) row[echo_pair_col(g, Gy[(int64_t)yy * W + xx], G)] += 1;
                }
            }
        if (w == 0) continue;
        // ownership: the minimum over the window, rows then columns
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int m = ECHO_NO_OWNER;
                const int a = x - w < 0 ? 0 : x - w, b = x + w >= W ? W - 1 : x + w;
                for (int xx = a; xx <= b; ++xx) {
                    const int v = echo_pos(L[(int64_t)y * W + xx]);
                    if (v < m) m = v;
                }
                rowmin[(size_t)y * W + x] = m;
            }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                if (L[(int64_t)y * W + x] > 0) continue;
                int m = ECHO_NO_OWNER;
                const int a = y - w < 0 ? 0 : y - w, b = y + w >= H ? H - 1 : y + w;
                for (int yy = a; yy <= b; ++yy) {
                    const int v = rowmin[(size_t)yy * W + x];
                    if (v < m) m = v;
                }
                if (m == ECHO_NO_OWNER || (int64_t)m > K) continue;
                T[(int64_t)(m - 1) * F + ECHO_HIST + Gy[(int64_t)y * W + x]] += 1;
            }
    }
}
