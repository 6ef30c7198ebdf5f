// Lesion echogenicity and texture of a batch of label planes on the device (echo.h: columns, rules).
// Two launches per call, both on the caller's stream:
//   clear   the whole table to zero (a memset: callers may hand in uninitialised memory);
//   count   block = (sample, tile of 64 x ECHO_TH pixels).  The labels of the tile and a halo of
//           max(w, 1) are staged in LDS (<= 0 and everything outside the plane as 0), the grey bytes
//           with a halo of one.  A block whose staged labels are all background has nothing to count
//           and leaves.  The ring owner is a separable minimum in LDS: the row pass takes the minimum
//           over 2 w + 1 columns for every staged row, the pixel then the minimum over 2 w + 1 of
//           those.  A tile row is one wave; lane x adds its pixel to the lesion histogram, the four
//           pairs it starts to the co-occurrence counts, or, on background, itself to its owner's
//           ring histogram.  The adds go into a label-keyed table in LDS (ECHO_POOL counters cut
//           into slots of 512 + G G, slot = label mod slots, claimed by one compare-and-swap) and the
//           non-zero counters of the claimed slots are flushed with one global atomic each; a label
//           whose slot another label holds adds straight to global memory.
//           Inside a lesion all 64 lanes carry one label, and lanes that share a grey level add to
//           one LDS word and serialise.  With `agg` every add is first aggregated over the wave as
//           kernels_curve.hip does it: the lanes that share the first active lane's (label, column)
//           are counted by one ballot and added once, the others add for themselves (the peel only:
//           one table for the block, no per-wave sub-histograms, which do not fit beside the tile).
//           The two ballots and shuffles per add cost more than they save on every input measured
//           (profiles/echo_time.txt: 0.74 x, 0.95 x, and 0.98 x on nearly flat grey), so the default
//           is plain atomics and `agg` exists for that A/B.
// No kernel waits for another block, and nothing but the table is written.
#include "echo.h"
#include "kernels_misc.h"

#include <algorithm>

namespace {

constexpr int ECHO_BLOCK = 256;
constexpr int ECHO_WAVES = ECHO_BLOCK / 64;
constexpr int ECHO_TW = 64;  // a tile row is one wave
constexpr int ECHO_TH = 32;
constexpr int ECHO_ROWS = ECHO_TH / ECHO_WAVES;       // ... per wave, consecutive
constexpr int ECHO_LW = ECHO_TW + 2 * ECHO_MAX_RING;  // staged labels: row stride
constexpr int ECHO_LH = ECHO_TH + 2 * ECHO_MAX_RING;
constexpr int ECHO_GW = ECHO_TW + 2;  // staged grey bytes: one column left and right,
constexpr int ECHO_GH = ECHO_TH + 1;  // one row below
constexpr int ECHO_POOL = 3072;       // counters of the LDS table: 5, 4, 2 slots at G = 8, 16, 32
constexpr int ECHO_MAX_SLOTS = 8;
constexpr unsigned ECHO_NONE = 0xFFFFFFFFu;  // label 0 as the minimum sees it: (unsigned)(0 - 1)

// where the counts of one block go: the LDS table, or global memory for a label without a slot
struct EchoSink {
    int* key;       // [slots], 0 = free
    unsigned* cnt;  // [slots][F]
    int* rows;      // the sample's table rows
    int slots, F;
    bool agg;

    // A plain read first, so that the lanes of a lesion do not all compare-and-swap one word.  It may
    // race with another wave's claim, which is harmless because a key changes once, 0 -> label, and
    // never again: a stale 0 falls through to the compare-and-swap, which decides; any other value
    // read is final.
    __device__ __forceinline__ int claim(int label) const {
        const int s = label % slots;
        const int k = key[s];
        if (k == label) return s;
        if (k != 0) return -1;
        const int old = atomicCAS(&key[s], 0, label);
        return old == 0 || old == label ? s : -1;
    }
    __device__ __forceinline__ void put(int label, int col, int v) const {
        const int s = claim(label);
        if (s >= 0) atomicAdd(&cnt[s * F + col], (unsigned)v);
        else atomicAdd(&rows[(int64_t)(label - 1) * F + col], v);
    }
    // label 0: nothing to add.  All 64 lanes of the wave call this together.
    __device__ __forceinline__ void add(int label, int col) const {
        if (!agg) {
            if (label > 0) put(label, col, 1);
            return;
        }
        const unsigned long long active = __ballot(label > 0);
        if (active == 0) return;  // wave-uniform
        const int leader = __ffsll((long long)active) - 1;
        const int l0 = __shfl(label, leader), c0 = __shfl(col, leader);
        const bool mine = label == l0 && col == c0;
        const unsigned long long same = __ballot(mine);
        if ((int)(threadIdx.x & 63) == leader) put(l0, c0, __popcll(same));
        else if (label > 0 && !mine) put(label, col, 1);
    }
};

// block b = (sample n, tile row ty, tile column tx)
__global__ __launch_bounds__(ECHO_BLOCK) void echo_count_kernel(const uint8_t* __restrict__ gray,
                                                                const int* __restrict__ labels,
                                                                const int* __restrict__ count, int H, int W, int nTx,
                                                                int nTy, int64_t max_rows, int G, int w, int agg,
                                                                int* __restrict__ table) {
    __shared__ int s_lab[ECHO_LH * ECHO_LW];
    __shared__ unsigned s_min[ECHO_LH * ECHO_TW];
    __shared__ uint8_t s_gray[ECHO_GH * ECHO_GW + 2];
    __shared__ unsigned s_cnt[ECHO_POOL];
    __shared__ int s_key[ECHO_MAX_SLOTS];
    const int tiles = nTx * nTy;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty = t / nTx, tx = t - ty * nTx;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = (int)echo_rows_used(count[n], max_rows);
    if (K == 0) return;  // block-uniform: the memset wrote this sample's rows
    const int* L = labels + (int64_t)n * H * W;
    const uint8_t* Gy = gray + (int64_t)n * H * W;
    const int F = echo_fields(G);
    const int slots = ECHO_POOL / F < ECHO_MAX_SLOTS ? ECHO_POOL / F : ECHO_MAX_SLOTS;
    const int h = w > 1 ? w : 1;
    const int y0 = ty * ECHO_TH, x0 = tx * ECHO_TW;
    const int lh = ECHO_TH + 2 * h, lw = ECHO_TW + 2 * h;
    int any = 0;
    for (int i = tid; i < lh * lw; i += ECHO_BLOCK) {
        const int ly = i / lw, lx = i - ly * lw;
        const int y = y0 - h + ly, x = x0 - h + lx;
        int v = y >= 0 && y < H && x >= 0 && x < W ? L[(int64_t)y * W + x] : 0;
        v = v > 0 ? v : 0;
        s_lab[ly * ECHO_LW + lx] = v;
        any |= v;
    }
    if (!__syncthreads_or(any)) return;  // no component within reach of this tile
    for (int i = tid; i < ECHO_GH * ECHO_GW; i += ECHO_BLOCK) {
        const int r = i / ECHO_GW, c = i - r * ECHO_GW;
        const int y = y0 + r, x = x0 - 1 + c;
        s_gray[i] = y < H && x >= 0 && x < W ? Gy[(int64_t)y * W + x] : (uint8_t)0;
    }
    for (int i = tid; i < slots * F; i += ECHO_BLOCK) s_cnt[i] = 0;
    if (tid < ECHO_MAX_SLOTS) s_key[tid] = 0;
    if (w > 0)  // h == w: staged row ly, tile column x covers the staged columns x .. x + 2 w
        for (int i = tid; i < lh * ECHO_TW; i += ECHO_BLOCK) {
            const int ly = i >> 6, x = i & 63;
            const int* p = s_lab + ly * ECHO_LW + x;
            unsigned m = ECHO_NONE;
            for (int k = 0; k <= 2 * w; ++k) m = min(m, (unsigned)(p[k] - 1));
            s_min[i] = m;
        }
    __syncthreads();
    EchoSink sink{s_key, s_cnt, table + (int64_t)n * max_rows * F, slots, F, agg != 0};
    const int x = x0 + lane;
    for (int r = 0; r < ECHO_ROWS; ++r) {
        const int tr = wv * ECHO_ROWS + r;
        if (y0 + tr >= H) break;  // wave-uniform
        const int* p = s_lab + (tr + h) * ECHO_LW + lane + h;
        const uint8_t* q = s_gray + tr * ECHO_GW + lane + 1;
        const int l = p[0];              // 0 on background and outside the plane
        const int lc = l > K ? 0 : l;    // a label without a row is dropped
        const int g = q[0];
        sink.add(lc, g);
        for (int k = 0; k < ECHO_OFFSETS; ++k) {
            const int dy = echo_dy(k), dx = echo_dx(k);
            const bool same = lc > 0 && p[dy * ECHO_LW + dx] == lc;
            sink.add(same ? lc : 0, echo_pair_col(g, q[dy * ECHO_GW + dx], G));
        }
        if (w > 0) {  // block-uniform
            int own = 0;
            if (l == 0 && x < W) {
                unsigned m = ECHO_NONE;
                for (int k = 0; k <= 2 * w; ++k) m = min(m, s_min[(tr + k) * ECHO_TW + lane]);
                own = m < (unsigned)K ? (int)m + 1 : 0;  // m = label - 1
            }
            sink.add(own, ECHO_HIST + g);
        }
    }
    __syncthreads();
    for (int i = tid; i < slots * F; i += ECHO_BLOCK) {
        const int s = i / F, f = i - s * F;
        const int label = s_key[s];
        const unsigned v = s_cnt[i];
        if (label != 0 && v != 0) atomicAdd(&sink.rows[(int64_t)(label - 1) * F + f], (int)v);
    }
}

}  // namespace

// the grid of a call fits a launch
bool echo_grid_ok(int N, int H, int W, int64_t max_rows) {
    const int64_t lim = (int64_t)1 << 31;
    const int64_t nTx = (W + ECHO_TW - 1) / ECHO_TW, nTy = (H + ECHO_TH - 1) / ECHO_TH;
    return (int64_t)N * nTx * nTy < lim && max_rows < lim && (int64_t)N * max_rows < lim;
}

int k_echo_clear(int N, int64_t max_rows, int G, int32_t* table, hipStream_t s) {
    return (int)hipMemsetAsync(table, 0, sizeof(int32_t) * (size_t)N * (size_t)max_rows * (size_t)echo_fields(G), s);
}

int k_echo_count(const uint8_t* gray, const int* labels, const int* count, int N, int H, int W, int64_t max_rows,
                 int G, int w, int agg, int32_t* table, hipStream_t s) {
    const int nTx = (W + ECHO_TW - 1) / ECHO_TW, nTy = (H + ECHO_TH - 1) / ECHO_TH;
    hipLaunchKernelGGL(echo_count_kernel, dim3((unsigned)((int64_t)N * nTx * nTy)), dim3(ECHO_BLOCK), 0, s, gray,
                       labels, count, H, W, nTx, nTy, max_rows, G, w, agg, table);
    return (int)hipGetLastError();
}
