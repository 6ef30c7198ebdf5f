// Lovasz hinge loss on the device (rules in lovasz.h): a stable, segmented key-index radix sort of
// every plane's margin errors and the loss / per-pixel weights read off the sorted order.
//
// A plane of M = H W pixels is cut into tiles of LV_TILE = 2048 consecutive elements, one block of
// four waves each (grid = tiles per plane x planes); wave w of a block owns the w-th 512 elements
// of the tile and walks them in LV_ITEMS = 8 rounds of 64 consecutive elements, so the order of
// the elements is (tile, wave, round, lane) everywhere and every load of a wave is one 256-byte row.
// The sort is least-significant-digit first, four passes of 8-bit digits over (key, word) pairs
// that ping-pong between two buffers; word = raster index | label << 31 (M <= 2^24), so the
// sorted order carries the labels with it and nothing is gathered afterwards.
//
//   lovasz_hist_kernel<FORM>  FORM: forms e, the key and the word of every pixel (8 bytes read, 8
//                       written per pixel) -- else reads the pass's keys -- and counts the tile's
//                       digits of the pass in LDS -> hist[plane][tile][256].
//   lovasz_scan_kernel  one block of 1024 threads per plane: the exclusive scan of hist over
//                       (digit, tile), digit-major, in place; thread (q, d) walks digit d over the
//                       q-th quarter of the tiles (coalesced: 256 digits side by side).  A digit
//                       that holds the whole plane sets skip[plane][pass]: that pass moves nothing
//                       for the plane, its blocks return at once and the plane's buffers do not
//                       swap (every kernel derives a plane's current buffer from its skip flags).
//   lovasz_scatter_kernel  the stable scatter.  Per round a wave finds, for every lane, the lanes
//                       that hold the same digit with eight ballots (match-any); the lowest of them
//                       bumps the wave's own LDS counter of that digit by their number and hands
//                       the old value round, so a lane's rank among the wave's equal digits is
//                       old + the equal lanes below it.  After the rounds thread d turns the four
//                       waves' counters of digit d into offsets (the tile's scanned base, then
//                       wave 0, 1, 2, 3), and every element is stored to base + rank with a plain
//                       vector store.  Equal digits keep their order: stable.
//   lovasz_count_kernel the positives of every tile of the SORTED order -> tilepos[plane][tile].
//   lovasz_plane_kernel per tile: P and the tile's positive prefix from tilepos, an inclusive scan
//                       of the labels (ballots, wave bases in LDS) = cTP_r, then g_r, the float64
//                       product with hinge(e_r) (e_r back from the key), gmap[index_r] = fl32(g_r)
//                       (0 for an inactive pixel), perm[r] = index_r when asked for; the tile's
//                       products are summed in a fixed tree -> part[plane][tile].
//   lovasz_sum_kernel   one block: the tiles of a plane in order, the planes in order per thread,
//                       the threads in order, all in float64 -> sum, loss.
//   lovasz_bwd_kernel   one streaming pass over logits, targets and gmap.
// No kernel uses a float atomic and every sum has a fixed order: run-to-run deterministic.
//
// 256 threads x 8 items: the scatter keeps 8 keys, words and ranks per lane in registers (no
// spill at 4 waves / SIMD) and 4 KiB of counters in LDS, so a CU holds as many blocks as its wave
// slots allow; the LDS atomics are one per distinct digit and wave, never contended.
#include "lovasz.h"
#include "kernels_misc.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace {

constexpr int LV_BLOCK = 256;
constexpr int LV_WAVES = LV_BLOCK / 64;
constexpr int LV_ITEMS = 8;
constexpr int LV_WAVE_SPAN = 64 * LV_ITEMS;      // elements of a tile one wave owns
constexpr int LV_TILE = LV_BLOCK * LV_ITEMS;     // 2048
constexpr int LV_PASSES = 4;
constexpr int LV_SCAN_BLOCK = 1024;

struct LvBuffers {
    uint32_t *key[2], *val[2];  // [planes][M] each
    uint32_t* hist;             // [planes][tiles][256]
    int* skip;                  // [planes][LV_PASSES]
    int* tilepos;               // [planes][tiles]
    double* part;               // [planes][tiles]
};

// the plane's buffer before pass p: one swap per pass that ran
__device__ __forceinline__ int lv_parity(const int* __restrict__ skip, int64_t plane, int p) {
    int par = 0;
    for (int q = 0; q < p; ++q) par ^= skip[plane * LV_PASSES + q] ? 0 : 1;
    return par;
}

// element k (0..LV_ITEMS-1) of this lane inside the tile
__device__ __forceinline__ int lv_offset(int k) {
    return (threadIdx.x >> 6) * LV_WAVE_SPAN + k * 64 + (threadIdx.x & 63);
}

template <bool FORM>
__global__ __launch_bounds__(LV_BLOCK) void lovasz_hist_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ t, int64_t M,
                                                               int tiles, int pass, LvBuffers B) {
    __shared__ unsigned cnt[256];
    const int64_t plane = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - plane * tiles);
    const int64_t base = (int64_t)tile * LV_TILE;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int par = FORM ? 0 : lv_parity(B.skip, plane, pass);
    const uint32_t* __restrict__ keys = B.key[par] + plane * M;
#pragma unroll
    for (int k = 0; k < LV_ITEMS; ++k) {
        const int64_t i = base + lv_offset(k);
        if (i < M) {
            uint32_t key;
            if (FORM) {
                const bool y = lovasz_label(t[plane * M + i]);
                key = lovasz_key(lovasz_error(x[plane * M + i], y));
                B.key[0][plane * M + i] = key;
                B.val[0][plane * M + i] = (uint32_t)i | (y ? LOVASZ_LABEL_BIT : 0u);
            } else {
                key = keys[i];
            }
            atomicAdd(&cnt[(key >> (8 * pass)) & 255u], 1u);
        }
    }
    __syncthreads();
    B.hist[((size_t)plane * tiles + tile) * 256 + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(LV_SCAN_BLOCK) void lovasz_scan_kernel(int64_t M, int tiles, int pass, LvBuffers B) {
    __shared__ unsigned seg[4][256];
    __shared__ unsigned dbase[256];
    __shared__ int whole;
    const int64_t plane = blockIdx.x;
    const int d = threadIdx.x & 255, q = threadIdx.x >> 8;
    uint32_t* __restrict__ h = B.hist + (size_t)plane * tiles * 256;
    const int per = (tiles + 3) / 4;
    const int b0 = min(tiles, q * per), b1 = min(tiles, b0 + per);
    if (threadIdx.x == 0) whole = 0;
    unsigned s = 0;
    for (int b = b0; b < b1; ++b) s += h[(size_t)b * 256 + d];
    seg[q][d] = s;
    __syncthreads();
    if (q == 0) {
        const unsigned tot = (seg[0][d] + seg[1][d]) + (seg[2][d] + seg[3][d]);
        dbase[d] = tot;
        if ((int64_t)tot == M) whole = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        B.skip[plane * LV_PASSES + pass] = whole;
        unsigned run = 0;
        for (int j = 0; j < 256; ++j) {
            const unsigned c = dbase[j];
            dbase[j] = run;
            run += c;
        }
    }
    __syncthreads();
    if (whole) return;  // block-uniform: the scatter of this pass does not run for the plane
    unsigned run = dbase[d];
    for (int j = 0; j < q; ++j) run += seg[j][d];
    for (int b = b0; b < b1; ++b) {
        const unsigned c = h[(size_t)b * 256 + d];
        h[(size_t)b * 256 + d] = run;
        run += c;
    }
}

__global__ __launch_bounds__(LV_BLOCK) void lovasz_scatter_kernel(int64_t M, int tiles, int pass, LvBuffers B) {
    __shared__ unsigned wcnt[LV_WAVES][256];
    const int64_t plane = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - plane * tiles);
    if (B.skip[plane * LV_PASSES + pass]) return;  // block-uniform
    const int par = lv_parity(B.skip, plane, pass);
    const uint32_t* __restrict__ kin = B.key[par] + plane * M;
    const uint32_t* __restrict__ vin = B.val[par] + plane * M;
    uint32_t* __restrict__ kout = B.key[par ^ 1] + plane * M;
    uint32_t* __restrict__ vout = B.val[par ^ 1] + plane * M;
    const int64_t base = (int64_t)tile * LV_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int w = 0; w < LV_WAVES; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    uint32_t key[LV_ITEMS], val[LV_ITEMS];
    unsigned rank[LV_ITEMS];
#pragma unroll
    for (int k = 0; k < LV_ITEMS; ++k) {
        const int64_t i = base + lv_offset(k);
        const bool in = i < M;
        key[k] = in ? kin[i] : 0u;
        val[k] = in ? vin[i] : 0u;
    }
    // every lane of the wave runs every round: the ballots and the shuffle need them all
#pragma unroll
    for (int k = 0; k < LV_ITEMS; ++k) {
        const bool in = base + lv_offset(k) < M;
        const unsigned d = (key[k] >> (8 * pass)) & 255u;
        unsigned long long peers = __ballot(in);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        if (!in) peers = 0;
        const int leader = peers ? __ffsll((long long)peers) - 1 : lane;
        unsigned old = 0;
        if (peers && lane == leader) old = atomicAdd(&wcnt[wave][d], (unsigned)__popcll(peers));
        old = __shfl(old, leader);
        rank[k] = old + (unsigned)__popcll(peers & below);
    }
    __syncthreads();
    {
        unsigned run = B.hist[((size_t)plane * tiles + tile) * 256 + threadIdx.x];
#pragma unroll
        for (int w = 0; w < LV_WAVES; ++w) {
            const unsigned c = wcnt[w][threadIdx.x];
            wcnt[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LV_ITEMS; ++k) {
        const bool in = base + lv_offset(k) < M;
        const unsigned d = (key[k] >> (8 * pass)) & 255u;
        const int64_t dst = (int64_t)wcnt[wave][d] + rank[k];
        if (in && dst < M) {  // dst < M whenever hist is this pass's: the guard costs nothing
            kout[dst] = key[k];
            vout[dst] = val[k];
        }
    }
}

__global__ __launch_bounds__(LV_BLOCK) void lovasz_count_kernel(int64_t M, int tiles, LvBuffers B) {
    __shared__ int red[LV_WAVES];
    const int64_t plane = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - plane * tiles);
    const uint32_t* __restrict__ vin = B.val[lv_parity(B.skip, plane, LV_PASSES)] + plane * M;
    const int64_t base = (int64_t)tile * LV_TILE;
    int c = 0;
#pragma unroll
    for (int k = 0; k < LV_ITEMS; ++k) {
        const int64_t i = base + lv_offset(k);
        c += i < M ? (int)(vin[i] >> 31) : 0;
    }
    for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) B.tilepos[plane * tiles + tile] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(LV_BLOCK) void lovasz_plane_kernel(int64_t M, int tiles, LvBuffers B,
                                                                float* __restrict__ gmap,
                                                                uint32_t* __restrict__ perm) {
    __shared__ long long redP[LV_WAVES], redQ[LV_WAVES];
    __shared__ int wtot[LV_WAVES];
    __shared__ double dred[LV_WAVES];
    const int64_t plane = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - plane * tiles);
    const int par = lv_parity(B.skip, plane, LV_PASSES);
    const uint32_t* __restrict__ kin = B.key[par] + plane * M;
    const uint32_t* __restrict__ vin = B.val[par] + plane * M;
    const int64_t base = (int64_t)tile * LV_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // P = all tiles' positives, before = those of the tiles in front of this one (exact integers)
    long long P = 0, before = 0;
    for (int b = threadIdx.x; b < tiles; b += LV_BLOCK) {
        const int c = B.tilepos[plane * tiles + b];
        P += c;
        before += b < tile ? c : 0;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        P += __shfl_xor(P, s);
        before += __shfl_xor(before, s);
    }
    if (lane == 0) {
        redP[wave] = P;
        redQ[wave] = before;
    }
    uint32_t key[LV_ITEMS], val[LV_ITEMS];
    int incl[LV_ITEMS];  // positives of this wave's span up to and including the element
    int run = 0;
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
#pragma unroll
    for (int k = 0; k < LV_ITEMS; ++k) {
        const int64_t i = base + lv_offset(k);
        const bool in = i < M;
        key[k] = in ? kin[i] : 0u;
        val[k] = in ? vin[i] : 0u;
        const unsigned long long m = __ballot(in && (val[k] >> 31));
        incl[k] = run + __popcll(m & upto);
        run += __popcll(m);
    }
    if (lane == 0) wtot[wave] = run;
    __syncthreads();
    P = (redP[0] + redP[1]) + (redP[2] + redP[3]);
    before = (redQ[0] + redQ[1]) + (redQ[2] + redQ[3]);
    for (int w = 0; w < wave; ++w) before += wtot[w];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < LV_ITEMS; ++k) {
        const int64_t r = base + lv_offset(k);
        if (r < M) {
            const bool y = val[k] >> 31;
            const float e = lovasz_unkey(key[k]);
            const double g = lovasz_grad(P, r, before + incl[k], y);
            acc += lovasz_hinge_of(e) * g;
            const uint32_t idx = val[k] & LOVASZ_INDEX_MASK;
            if ((int64_t)idx < M) gmap[plane * M + idx] = e > 0.0f ? (float)g : 0.0f;
            if (perm) perm[plane * M + r] = idx;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
    if (lane == 0) dred[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) B.part[plane * tiles + tile] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
}

__global__ __launch_bounds__(256) void lovasz_sum_kernel(const double* __restrict__ part, int64_t planes,
                                                        int tiles, double* __restrict__ sum,
                                                        float* __restrict__ loss) {
    __shared__ double acc[256];
    double a = 0.0;
    for (int64_t p = threadIdx.x; p < planes; p += 256) {
        double l = 0.0;
        for (int b = 0; b < tiles; ++b) l += part[p * tiles + b];
        a += l;
    }
    acc[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < 256; ++k) s += acc[k];
    sum[0] = s;
    loss[0] = (float)(s / (double)planes);
}

__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                        const float* __restrict__ g, int64_t total, float nc,
                                                        const float* __restrict__ w, float* __restrict__ dx) {
    const float w0 = w[0];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x)
        dx[i] = lovasz_dlogit(x[i], t[i], g[i], w0, nc);
}

size_t lv_align(size_t b) { return (b + 255) & ~(size_t)255; }

int lv_tiles(int64_t hw) { return (int)((hw + LV_TILE - 1) / LV_TILE); }

// the buffers inside scratch (null: sizes only); returns the bytes
size_t lv_layout(void* scratch, int64_t planes, int64_t hw, LvBuffers& B) {
    const size_t T = (size_t)planes * (size_t)hw, tl = (size_t)planes * lv_tiles(hw);
    char* p = (char*)scratch;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* q = p + off;
        off += lv_align(bytes);
        return (void*)q;
    };
    for (int j = 0; j < 2; ++j) B.key[j] = (uint32_t*)take(sizeof(uint32_t) * T);
    for (int j = 0; j < 2; ++j) B.val[j] = (uint32_t*)take(sizeof(uint32_t) * T);
    B.hist = (uint32_t*)take(sizeof(uint32_t) * 256 * tl);
    B.skip = (int*)take(sizeof(int) * LV_PASSES * (size_t)planes);
    B.tilepos = (int*)take(sizeof(int) * tl);
    B.part = (double*)take(sizeof(double) * tl);
    return off;
}

}  // namespace

bool lovasz_shape_ok(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return false;
    const int64_t hw = (int64_t)H * W;
    if (hw > LOVASZ_MAX_HW) return false;
    // one block per tile in a one-dimensional grid
    return (int64_t)N * C * lv_tiles(hw) < (int64_t)1 << 31;
}

size_t lovasz_scratch_bytes(int N, int C, int H, int W) {
    LvBuffers B;
    return lv_layout(nullptr, (int64_t)N * C, (int64_t)H * W, B);
}

int k_lovasz_fwd(const float* x, const float* t, int N, int C, int H, int W, void* scratch, float* gmap,
                 uint32_t* perm, double* sum, float* loss, hipStream_t s) {
    const int64_t planes = (int64_t)N * C, hw = (int64_t)H * W;
    const int tiles = lv_tiles(hw);
    LvBuffers B;
    lv_layout(scratch, planes, hw, B);
    const dim3 grid((unsigned)(planes * tiles)), block(LV_BLOCK);
    hipLaunchKernelGGL(lovasz_hist_kernel<true>, grid, block, 0, s, x, t, hw, tiles, 0, B);
    HIP_OK(hipGetLastError());
    for (int pass = 0; pass < LV_PASSES; ++pass) {
        if (pass) {
            hipLaunchKernelGGL(lovasz_hist_kernel<false>, grid, block, 0, s, x, t, hw, tiles, pass, B);
            HIP_OK(hipGetLastError());
        }
        hipLaunchKernelGGL(lovasz_scan_kernel, dim3((unsigned)planes), dim3(LV_SCAN_BLOCK), 0, s, hw, tiles, pass, B);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(lovasz_scatter_kernel, grid, block, 0, s, hw, tiles, pass, B);
        HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(lovasz_count_kernel, grid, block, 0, s, hw, tiles, B);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(lovasz_plane_kernel, grid, block, 0, s, hw, tiles, B, gmap, perm);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(lovasz_sum_kernel, dim3(1), dim3(256), 0, s, B.part, planes, tiles, sum, loss);
    return (int)hipGetLastError();
}

int k_lovasz_bwd(const float* x, const float* t, const float* gmap, int N, int C, int H, int W, const float* w,
                 float* dx, hipStream_t s) {
    const int64_t total = (int64_t)N * C * H * W;
    const int grid = (int)std::min<int64_t>(8192, std::max<int64_t>(1, (total + 255) / 256));
    hipLaunchKernelGGL(lovasz_bwd_kernel, dim3(grid), dim3(256), 0, s, x, t, gmap, total,
                       (float)((int64_t)N * C), w, dx);
    return (int)hipGetLastError();
}

// The host twin: the same rules, a stable sort by key, the ranks in order.
void lovasz_host(const float* x, const float* t, int N, int C, int H, int W, float* gmap, uint32_t* perm,
                 double* sum, float* loss) {
    const int64_t planes = (int64_t)N * C, M = (int64_t)H * W;
    std::vector<uint32_t> key((size_t)M), order((size_t)M);
    std::vector<uint8_t> lab((size_t)M);
    double total = 0.0;
    for (int64_t p = 0; p < planes; ++p) {
        const float* xp = x + p * M;
        const float* tp = t + p * M;
        int64_t P = 0;
        for (int64_t i = 0; i < M; ++i) {
            lab[i] = lovasz_label(tp[i]);
            key[i] = lovasz_key(lovasz_error(xp[i], lab[i]));
            P += lab[i];
        }
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        double l = 0.0;
        int64_t ctp = 0;
        for (int64_t r = 0; r < M; ++r) {
            const uint32_t i = order[r];
            ctp += lab[i];
            const float e = lovasz_unkey(key[i]);
            const double g = lovasz_grad(P, r, ctp, lab[i]);
            l += lovasz_hinge_of(e) * g;
            gmap[p * M + i] = e > 0.0f ? (float)g : 0.0f;
            if (perm) perm[p * M + r] = i;
        }
        total += l;
    }
    sum[0] = total;
    loss[0] = (float)(total / (double)planes);
}
