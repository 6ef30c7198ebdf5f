// Lesion morphometry of a batch of label planes on the device (morph.h: fields, rules, phases).
// One launch per step, all on the caller's stream:
//   init     every table row to the neutral element of its fields (0, or MORPH_MIN_INIT);
//   reduce   block = (sample, tile of 64 x MORPH_TH window positions); wave w walks the tile rows
//            w * MORPH_TH / 4 .. in order and keeps the row above in registers.  Run sums, boxes and
//            bit quads go through a label-keyed table in LDS (MORPH_SLOTS slots, slot = label mod
//            MORPH_SLOTS, claimed by one compare-and-swap), flushed by one global 64-bit atomic per
//            touched field; a label whose slot another label holds adds straight to global memory;
//   offsets  block = sample: exclusive scan of the box heights of the labels <= min(count, max_rows);
//   extent   the row extents of every (component, row) slot, by atomicMax from the run leaders;
//   feret    block = (sample, table row): the farthest pair among the row extents, or the zero row.
// No kernel waits for another block.
#include "morph.h"
#include "kernels_misc.h"

#include <algorithm>

namespace {

constexpr int MORPH_BLOCK = 256;
constexpr int MORPH_WAVES = MORPH_BLOCK / 64;
constexpr int MORPH_TH = 32;                       // tile rows
constexpr int MORPH_ROWS = MORPH_TH / MORPH_WAVES;  // ... per wave, consecutive
constexpr int MORPH_SLOTS = 64;
constexpr int MORPH_SUMS = 10;  // area, sx, sy, sxx, sxy, syy, q1, q2, qd, q3

typedef unsigned long long u64;

__device__ __forceinline__ int sum_index(int f) { return f < 6 ? f : f - 4; }  // MF_Q1.. -> 6..

// ---- init ----
__global__ __launch_bounds__(MORPH_BLOCK) void morph_init_kernel(int64_t* __restrict__ table, int64_t total) {
    for (int64_t i = blockIdx.x * (int64_t)MORPH_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MORPH_BLOCK)
        table[i] = morph_min_field((int)(i & 15)) ? MORPH_MIN_INIT : 0;
}

// ---- reduce ----
// where the contributions of one block go: the LDS table, or global memory for a label without a slot
struct MorphSink {
    int* key;       // [MORPH_SLOTS], 0 = free
    u64* sum;       // [MORPH_SLOTS][MORPH_SUMS]
    int* box;       // [MORPH_SLOTS][5]: x0, y0 (min), x1, y1 (max), first (min)
    u64* rows;      // the sample's table rows
    int64_t max_rows;
    bool lds;

    __device__ __forceinline__ int claim(int label) const {
        if (!lds) return -1;
        const int s = label & (MORPH_SLOTS - 1);
        const int old = atomicCAS(&key[s], 0, label);
        return old == 0 || old == label ? s : -1;
    }
    __device__ __forceinline__ u64* row(int label) const { return rows + (int64_t)(label - 1) * MORPH_FIELDS; }
    __device__ __forceinline__ void run(int label, int x0, int n, int y, int W) const {
        if (label > max_rows) return;
        int64_t s6[6];
        morph_run_sums(x0, n, y, s6);
        const int first = y * W + x0;
        const int s = claim(label);
        if (s >= 0) {
            for (int f = 0; f < 6; ++f) atomicAdd(&sum[s * MORPH_SUMS + f], (u64)s6[f]);
            int* b = box + s * 5;
            atomicMin(&b[0], x0);
            atomicMin(&b[1], y);
            atomicMax(&b[2], x0 + n - 1);
            atomicMax(&b[3], y);
            atomicMin(&b[4], first);
        } else {
            u64* r = row(label);
            for (int f = 0; f < 6; ++f) atomicAdd(&r[f], (u64)s6[f]);
            atomicMin(&r[MF_X0], (u64)x0);
            atomicMin(&r[MF_Y0], (u64)y);
            atomicMax(&r[MF_X1], (u64)(x0 + n - 1));
            atomicMax(&r[MF_Y1], (u64)y);
            atomicMin(&r[MF_FIRST], (u64)first);
        }
    }
    __device__ __forceinline__ void quad(int label, int field) const {
        if (label > max_rows) return;
        const int s = claim(label);
        if (s >= 0) atomicAdd(&sum[s * MORPH_SUMS + sum_index(field)], (u64)1);
        else atomicAdd(&row(label)[field], (u64)1);
    }
};

// block b = (sample n, tile row ty, tile column tx) over the (H + 1) x (W + 1) window positions
__global__ __launch_bounds__(MORPH_BLOCK) void morph_reduce_kernel(const int* __restrict__ labels, int H, int W,
                                                                  int nTx, int nTy, int64_t max_rows, int use_lds,
                                                                  int64_t* __restrict__ table) {
    __shared__ int s_key[MORPH_SLOTS];
    __shared__ u64 s_sum[MORPH_SLOTS * MORPH_SUMS];
    __shared__ int s_box[MORPH_SLOTS * 5];
    const int tiles = nTx * nTy;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty = t / nTx, tx = t - ty * nTx;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int* L = labels + (int64_t)n * H * W;
    MorphSink sink{s_key, s_sum, s_box, (u64*)table + (int64_t)n * max_rows * MORPH_FIELDS, max_rows, use_lds != 0};
    if (use_lds) {
        for (int i = threadIdx.x; i < MORPH_SLOTS; i += MORPH_BLOCK) s_key[i] = 0;
        for (int i = threadIdx.x; i < MORPH_SLOTS * MORPH_SUMS; i += MORPH_BLOCK) s_sum[i] = 0;
        for (int i = threadIdx.x; i < MORPH_SLOTS * 5; i += MORPH_BLOCK) {
            const int f = i % 5;
            s_box[i] = (f == 2 || f == 3) ? -1 : INT32_MAX;
        }
        __syncthreads();
    }
    const int x = tx * MORPH_TILE_W + lane;  // <= W + 63
    const int xl = tx * MORPH_TILE_W - 1;    // the halo column of lane 0
    // label at (y, x), 0 outside the plane
    auto at = [&](int y, int xx) { return y >= 0 && y < H && xx >= 0 && xx < W ? L[(int64_t)y * W + xx] : 0; };
    const int ya = ty * MORPH_TH + wv * MORPH_ROWS;
    int up = at(ya - 1, x);
    int upl = __shfl_up(up, 1);
    if (lane == 0) upl = at(ya - 1, xl);
    for (int r = 0; r < MORPH_ROWS; ++r) {
        const int y = ya + r;
        if (y > H) break;  // wave-uniform
        const int cur = at(y, x);
        int left = __shfl_up(cur, 1);
        const bool cont_here = lane > 0 && cur > 0 && cur == left;  // lane 0 starts a run of its own
        if (lane == 0) left = at(y, xl);
        const uint64_t cont = __ballot(cont_here);
        if (cur > 0 && !cont_here) sink.run(cur, x, morph_run_len(cont, lane), y, W);
        if (x <= W) {
            const MorphQuad q = morph_quad(upl, up, left, cur);
            for (int k = 0; k < q.n; ++k) sink.quad(q.label[k], q.field[k]);
        }
        upl = left;
        up = cur;
    }
    if (!use_lds) return;  // block-uniform
    __syncthreads();
    for (int i = threadIdx.x; i < MORPH_SLOTS * MORPH_FIELDS; i += MORPH_BLOCK) {
        const int s = i >> 4, f = i & 15;
        const int label = s_key[s];
        if (label == 0 || f == MF_D2MAX) continue;
        u64* r = sink.row(label);
        if (morph_min_field(f)) {
            const int v = s_box[s * 5 + (f == MF_X0 ? 0 : f == MF_Y0 ? 1 : 4)];
            if (v != INT32_MAX) atomicMin(&r[f], (u64)v);
        } else if (morph_max_field(f)) {
            const int v = s_box[s * 5 + (f == MF_X1 ? 2 : 3)];
            if (v >= 0) atomicMax(&r[f], (u64)v);
        } else {
            const u64 v = s_sum[s * MORPH_SUMS + sum_index(f)];
            if (v) atomicAdd(&r[f], v);
        }
    }
}

// ---- offsets ----
__device__ __forceinline__ int64_t rows_used(const int* count, int n, int64_t max_rows) {
    const int k = count[n];
    return k < 0 ? 0 : ((int64_t)k < max_rows ? (int64_t)k : max_rows);
}
// box height of table row r (0 for a row without pixels), never above H
__device__ __forceinline__ int box_height(const int64_t* row, int H) {
    if (row[MF_AREA] <= 0) return 0;
    const int64_t h = row[MF_Y1] - row[MF_Y0] + 1;
    return h < 1 ? 0 : h > H ? H : (int)h;
}

// block = sample: off[r] = sum of the box heights of the rows below r, r < min(count, max_rows)
__global__ __launch_bounds__(MORPH_BLOCK) void morph_offsets_kernel(const int64_t* __restrict__ table,
                                                                   const int* __restrict__ count, int H,
                                                                   int64_t max_rows, int64_t* __restrict__ off) {
    __shared__ int64_t wsum[MORPH_WAVES];
    const int n = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t K = rows_used(count, n, max_rows);
    const int64_t* T = table + (int64_t)n * max_rows * MORPH_FIELDS;
    int64_t* o = off + (int64_t)n * max_rows;
    int64_t base = 0;
    for (int64_t r0 = 0; r0 < K; r0 += MORPH_BLOCK) {
        const int64_t r = r0 + threadIdx.x;
        const int64_t h = r < K ? box_height(T + r * MORPH_FIELDS, H) : 0;
        int64_t inc = h;  // inclusive scan inside the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        int64_t pre = 0, tot = 0;
        for (int k = 0; k < MORPH_WAVES; ++k) {
            if (k < wv) pre += wsum[k];
            tot += wsum[k];
        }
        if (r < K) o[r] = base + pre + inc - h;
        base += tot;
        __syncthreads();
    }
}

// ---- extent ----
// block = (sample, tile of 64 x MORPH_TH pixels); ext: 2 ints per slot, `slots` slots per sample
__global__ __launch_bounds__(MORPH_BLOCK) void morph_extent_kernel(const int* __restrict__ labels,
                                                                  const int* __restrict__ count, int H, int W,
                                                                  int nTx, int nTy, int64_t max_rows,
                                                                  const int64_t* __restrict__ table,
                                                                  const int64_t* __restrict__ off, int64_t slots,
                                                                  int* __restrict__ ext) {
    const int tiles = nTx * nTy;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty = t / nTx, tx = t - ty * nTx;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int* L = labels + (int64_t)n * H * W;
    const int64_t K = rows_used(count, n, max_rows);
    const int64_t* T = table + (int64_t)n * max_rows * MORPH_FIELDS;
    const int64_t* o = off + (int64_t)n * max_rows;
    int* e = ext + 2 * slots * n;
    const int x = tx * MORPH_TILE_W + lane;
    for (int r = wv; r < MORPH_TH; r += MORPH_WAVES) {
        const int y = ty * MORPH_TH + r;
        if (y >= H) break;  // wave-uniform
        const int cur = x < W ? L[(int64_t)y * W + x] : 0;
        const int left = __shfl_up(cur, 1);
        const bool cont_here = lane > 0 && cur > 0 && cur == left;
        const uint64_t cont = __ballot(cont_here);
        if (cur <= 0 || cont_here || (int64_t)cur > K) continue;
        const int64_t* row = T + (int64_t)(cur - 1) * MORPH_FIELDS;
        const int h = box_height(row, H);
        const int64_t i = (int64_t)y - row[MF_Y0];
        if (i < 0 || i >= h) continue;
        const int64_t slot = o[cur - 1] + i;
        if (slot < 0 || slot >= slots) continue;
        const int len = morph_run_len(cont, lane);
        atomicMax(&e[2 * slot], morph_extent_lo(W, x));
        atomicMax(&e[2 * slot + 1], morph_extent_hi(x + len - 1));
    }
}

// ---- feret ----
// block = (sample, table row)
__global__ __launch_bounds__(MORPH_BLOCK) void morph_feret_kernel(const int* __restrict__ count, int H, int W,
                                                                 int64_t max_rows, const int64_t* __restrict__ off,
                                                                 int64_t slots, const int* __restrict__ ext,
                                                                 int64_t* __restrict__ table) {
    __shared__ short xmin[MORPH_MAX_SIDE], xmax[MORPH_MAX_SIDE];  // xmax < 0: a row without a pixel
    __shared__ int red[MORPH_WAVES];
    const int64_t b = blockIdx.x;
    const int n = (int)(b / max_rows);
    const int64_t r = b - n * max_rows;
    int64_t* row = table + b * MORPH_FIELDS;
    const int64_t K = rows_used(count, n, max_rows);
    const int h = r < K ? box_height(row, H) : 0;  // block-uniform
    const int64_t o = h > 0 ? off[b] : 0;
    if (h == 0 || o < 0 || o + h > slots) {
        if (h == 0 && threadIdx.x < MORPH_FIELDS) row[threadIdx.x] = 0;
        return;
    }
    const int* e = ext + 2 * (slots * n + o);
    for (int i = threadIdx.x; i < h; i += MORPH_BLOCK) {
        const int lo = e[2 * i], hi = e[2 * i + 1];
        xmin[i] = (short)(W - lo);
        xmax[i] = (short)(hi > 0 && lo > 0 ? hi - 1 : -1);
    }
    __syncthreads();
    int best = 0;
    for (int i = 0; i < h; ++i) {
        const int xi0 = xmin[i], xi1 = xmax[i];
        if (xi1 < 0) continue;
        for (int j = i + threadIdx.x; j < h; j += MORPH_BLOCK) {
            const int xj1 = xmax[j];
            if (xj1 < 0) continue;
            const int d2 = morph_row_pair_d2(xi0, xi1, xmin[j], xj1, j - i);
            best = d2 > best ? d2 : best;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const int v = __shfl_xor(best, d);
        best = v > best ? v : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < MORPH_WAVES; ++k) best = red[k] > best ? red[k] : best;
        row[MF_D2MAX] = best;
    }
}

int64_t align64(int64_t b) { return (b + 63) & ~(int64_t)63; }

}  // namespace

// every grid of a call fits a launch
bool morph_grid_ok(int N, int H, int W, int64_t max_rows) {
    const int64_t lim = (int64_t)1 << 31;
    const int64_t nTx = W / MORPH_TILE_W + 1, nTy = H / MORPH_TH + 1;
    return (int64_t)N * nTx * nTy < lim && max_rows < lim && (int64_t)N * max_rows < lim;
}

// scratch: [N max_rows offsets (int64)][N slots extents (2 ints each), zeroed by every call]
MorphScratch morph_scratch(void* base, int N, int H, int W, int64_t max_rows) {
    MorphScratch s;
    char* p = (char*)base;
    s.slots = morph_extent_slots(H, W);
    s.off = (int64_t*)p;
    p += align64(8 * (int64_t)N * max_rows);
    s.ext = (int*)p;
    s.ext_bytes = (size_t)(8 * (int64_t)N * s.slots);
    p += align64((int64_t)s.ext_bytes);
    s.bytes = (size_t)(p - (char*)base);
    return s;
}

int k_morph_reduce(const int* labels, int N, int H, int W, int64_t max_rows, int use_lds, int64_t* table,
                   hipStream_t s) {
    const int64_t total = (int64_t)N * max_rows * MORPH_FIELDS;
    const unsigned g0 = (unsigned)std::min<int64_t>((total + MORPH_BLOCK - 1) / MORPH_BLOCK, 4096);
    hipLaunchKernelGGL(morph_init_kernel, dim3(g0), dim3(MORPH_BLOCK), 0, s, table, total);
    HIP_OK(hipGetLastError());
    // the window positions: x in [0, W], y in [0, H]
    const int nTx = W / MORPH_TILE_W + 1, nTy = H / MORPH_TH + 1;
    hipLaunchKernelGGL(morph_reduce_kernel, dim3((unsigned)((int64_t)N * nTx * nTy)), dim3(MORPH_BLOCK), 0, s, labels,
                       H, W, nTx, nTy, max_rows, use_lds, table);
    return (int)hipGetLastError();
}

int k_morph_extent(const int* labels, const int* count, int N, int H, int W, int64_t max_rows, const int64_t* table,
                   const MorphScratch& sc, hipStream_t s) {
    HIP_OK(hipMemsetAsync(sc.ext, 0, sc.ext_bytes, s));
    hipLaunchKernelGGL(morph_offsets_kernel, dim3((unsigned)N), dim3(MORPH_BLOCK), 0, s, table, count, H, max_rows,
                       sc.off);
    HIP_OK(hipGetLastError());
    const int nTx = (W + MORPH_TILE_W - 1) / MORPH_TILE_W, nTy = (H + MORPH_TH - 1) / MORPH_TH;
    hipLaunchKernelGGL(morph_extent_kernel, dim3((unsigned)((int64_t)N * nTx * nTy)), dim3(MORPH_BLOCK), 0, s, labels,
                       count, H, W, nTx, nTy, max_rows, table, sc.off, sc.slots, sc.ext);
    return (int)hipGetLastError();
}

int k_morph_feret(const int* count, int N, int H, int W, int64_t max_rows, const MorphScratch& sc, int64_t* table,
                  hipStream_t s) {
    hipLaunchKernelGGL(morph_feret_kernel, dim3((unsigned)((int64_t)N * max_rows)), dim3(MORPH_BLOCK), 0, s, count, H,
                       W, max_rows, sc.off, sc.slots, sc.ext, table);
    return (int)hipGetLastError();
}
