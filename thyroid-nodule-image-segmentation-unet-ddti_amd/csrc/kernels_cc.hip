// Connected-component labelling of a batch of planes on the device, and the post-processing and
// lesion counts built on it (cc.h: definitions and per-pixel rules).  One launch per phase:
//   tile     one block per 64 x TH tile, the tile in LDS: row runs from a wave ballot (a row of 64
//            pixels is one wave), union-find inside the tile with LDS atomicMin, then the global
//            index of the tile-local root (-1: background) as each pixel's provisional label;
//   seam     the pixel pairs across tile borders (at connectivity 2 the diagonal ones too), by
//            cc_union on the labels in global memory;
//   flatten  label[p] = find(p), roots counted per row and per plane, areas added into
//            area[root] (one integer atomicAdd per wave and root);
//   rank     rank of every root in raster order (row counts, then ballot and popcount inside the
//            row), and the rewrite of the labels to 1..K.
// No kernel waits for another block: find follows strictly decreasing indices and cc_union
// retries only from the smaller index an atomicMin returned.  Plane q of a call lives at
// L + q H W; labels are linear indices inside the plane (H W < 2^31).
#include "cc.h"
#include "kernels_misc.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int CC_BLOCK = 256;
constexpr int CC_WAVES = CC_BLOCK / 64;

__device__ __forceinline__ int popc64(uint64_t m) { return __popcll(m); }
__device__ __forceinline__ uint64_t lanes_below(int lane) { return ((uint64_t)1 << lane) - 1; }

__device__ __forceinline__ void union_atomic(int* L, int a, int b) {
    cc_union(L, a, b, [](int* slot, int v) { return atomicMin(slot, v); });
}

// ---- tile pass ----
// block b = (plane q, tile row ty, tile column tx); wave w owns the tile rows w, w + 4, ...
// src points at plane 0's sample, samples `sample_stride` elements apart.
template <int TH>
__global__ __launch_bounds__(CC_BLOCK) void cc_tile_kernel(const void* __restrict__ src, int kind,
                                                          int64_t sample_stride, int H, int W,
                                                          int nTx, int nTy, int conn,
                                                          int* __restrict__ L,
                                                          int* __restrict__ area) {
    __shared__ int lab[TH * CC_TILE_W];
    __shared__ uint64_t rowmask[TH];
    const int tiles = nTx * nTy;
    const int q = blockIdx.x / tiles, t = blockIdx.x - q * tiles;
    const int ty = t / nTx, tx = t - ty * nTx;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t x = (int64_t)tx * CC_TILE_W + lane;
    const int64_t hw = (int64_t)H * W;
    int* Lq = L + q * hw;
    int* aq = area + q * hw;
    for (int r = wv; r < TH; r += CC_WAVES) {
        const int y = ty * TH + r;
        const bool in = y < H && x < W;
        const int64_t p = (int64_t)y * W + x;
        const bool fg = in && cc_fg(src, kind, q * sample_stride + p);
        const uint64_t m = __ballot(fg);
        lab[r * CC_TILE_W + lane] = fg ? r * CC_TILE_W + cc_run_start(m, lane) : -1;
        if (lane == 0) rowmask[r] = m;
        if (in) aq[p] = 0;
    }
    __syncthreads();
    // a run meets the runs of the row above: the first column of every overlap links them
    for (int r = wv; r < TH; r += CC_WAVES) {
        if (r == 0) continue;
        const uint64_t m = rowmask[r], up = rowmask[r - 1];
        if (!((m >> lane) & 1)) continue;
        const bool upc = (up >> lane) & 1;
        const bool upl = lane > 0 && ((up >> (lane - 1)) & 1);
        const bool upr = lane < 63 && ((up >> (lane + 1)) & 1);
        const bool left = lane > 0 && ((m >> (lane - 1)) & 1);
        const int me = r * CC_TILE_W + lane, above = me - CC_TILE_W;
        if (upc) {
            if (!(left && upl)) union_atomic(lab, me, above);
        } else if (conn == 2) {
            if (upl && !left) union_atomic(lab, me, above - 1);
            if (upr) union_atomic(lab, me, above + 1);
        }
    }
    __syncthreads();
    for (int r = wv; r < TH; r += CC_WAVES) {
        const int y = ty * TH + r;
        if (y >= H || x >= W) continue;
        const int v = lab[r * CC_TILE_W + lane];
        int g = -1;
        if (v >= 0) {
            const int root = cc_find(lab, v);
            g = (ty * TH + (root >> 6)) * W + tx * CC_TILE_W + (root & 63);
        }
        Lq[(int64_t)y * W + x] = g;
    }
}

// ---- seam pass ----
// One thread per pixel on the first row of a tile row (nh per plane) or the first column of a
// tile column (nv per plane).  A pair is skipped where two other pairs of the same 2 x 2 block
// already join it (4-adjacent pixels inside one tile are joined by the tile pass; a run of pairs
// along a seam is joined by its first pair inside the tile).
__global__ __launch_bounds__(CC_BLOCK) void cc_seam_kernel(int* L, int64_t total, int H,
                                                          int W, int TH, int nh, int nv, int conn) {
    const int64_t idx = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    if (idx >= total) return;
    const int S = nh + nv;
    const int64_t q = idx / S;
    const int i = (int)(idx - q * S);
    int* Lq = L + q * ((int64_t)H * W);
    if (i < nh) {  // (y, x) against the row above, which belongs to another tile
        const int k = i / W, x = i - k * W, y = (k + 1) * TH;
        const int p = y * W + x, up = p - W;
        if (Lq[p] < 0) return;
        if (Lq[up] >= 0) {
            const bool dup = (x % CC_TILE_W) != 0 && Lq[p - 1] >= 0 && Lq[up - 1] >= 0;
            if (!dup) union_atomic(Lq, p, up);
        } else if (conn == 2) {
            if (x > 0 && Lq[up - 1] >= 0 && Lq[p - 1] < 0) union_atomic(Lq, p, up - 1);
            if (x + 1 < W && Lq[up + 1] >= 0 && Lq[p + 1] < 0) union_atomic(Lq, p, up + 1);
        }
    } else {  // (y, x) against the column to the left, which belongs to another tile
        const int j = i - nh;
        const int k = j / H, y = j - k * H, x = (k + 1) * CC_TILE_W;
        const int p = y * W + x, lf = p - 1;
        if (Lq[p] < 0) return;
        if (Lq[lf] >= 0) {
            const bool dup = (y % TH) != 0 && Lq[p - W] >= 0 && Lq[lf - W] >= 0;
            if (!dup) union_atomic(Lq, p, lf);
        } else if (conn == 2) {
            if (y > 0 && Lq[lf - W] >= 0 && Lq[p - W] < 0) union_atomic(Lq, p, lf - W);
            if (y + 1 < H && Lq[lf + W] >= 0 && Lq[p + W] < 0) union_atomic(Lq, p, lf + W);
        }
    }
}

// ---- per-pixel kernels: block = (plane q, row y, chunk of CC_BLOCK columns), so a wave never
// spans two rows and no thread leaves before the wave's ballots ----
struct Pix {
    int q, y, x, p;  // p = y W + x, valid when in
    bool in;
};
__device__ __forceinline__ Pix cc_pix(int H, int W, int chunks) {
    Pix a;
    const unsigned b = blockIdx.x;
    const unsigned row = b / chunks;
    a.q = row / H;
    a.y = row - a.q * H;
    const int64_t x = (int64_t)(b - row * chunks) * CC_BLOCK + threadIdx.x;
    a.in = x < W;
    a.x = a.in ? (int)x : W;
    a.p = a.in ? a.y * W + a.x : 0;
    return a;
}

template <bool AREAS>
__global__ __launch_bounds__(CC_BLOCK) void cc_flatten_kernel(int* L, int* __restrict__ area,
                                                             int* __restrict__ rowcnt,
                                                             int* __restrict__ cnt, int H, int W,
                                                             int chunks) {
    const Pix a = cc_pix(H, W, chunks);
    const int64_t hw = (int64_t)H * W;
    int* Lq = L + a.q * hw;
    const int lane = threadIdx.x & 63;
    int r = -1;
    if (a.in) {
        const int v = Lq[a.p];
        if (v >= 0) {
            r = cc_find(Lq, v);
            if (r != v) __atomic_store_n(&Lq[a.p], r, __ATOMIC_RELAXED);  // a shorter way to the same root for whoever reads it meanwhile
        }
    }
    const uint64_t roots = __ballot(a.in && r == a.p);
    if (lane == 0 && roots) {
        if (rowcnt) atomicAdd(&rowcnt[a.q * H + a.y], popc64(roots));
        if (cnt) atomicAdd(&cnt[a.q], popc64(roots));
    }
    if (AREAS) {  // one add per wave and root: the lanes of the leader's root leave together
        bool todo = r >= 0;
        for (;;) {
            const uint64_t act = __ballot(todo);
            if (!act) break;
            const int leader = __ffsll((long long)act) - 1;
            const int lr = __shfl(r, leader);
            const bool same = todo && r == lr;
            const uint64_t sm = __ballot(same);
            if (lane == leader) atomicAdd(&area[a.q * hw + lr], popc64(sm));
            if (same) todo = false;
        }
    }
}

// ---- rank pass ----
// block = (plane, row): the roots of the rows above from the row counts, then the roots of this
// row in column order; rk[root] = 1 + rank.  The last row's block writes the plane's count.
__global__ __launch_bounds__(CC_BLOCK) void cc_rank_kernel(const int* __restrict__ L, int* __restrict__ rk,
                                                          const int* __restrict__ rowcnt,
                                                          int* __restrict__ count, int H, int W) {
    __shared__ int red[CC_WAVES], wc[CC_WAVES];
    const int q = blockIdx.x / H, y = blockIdx.x - q * H;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t hw = (int64_t)H * W;
    const int* Lq = L + q * hw;
    int s = 0;
    for (int i = threadIdx.x; i < y; i += CC_BLOCK) s += rowcnt[q * H + i];
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < CC_WAVES; ++k) base += red[k];
    for (int64_t x0 = 0; x0 < W; x0 += CC_BLOCK) {
        const int64_t x = x0 + threadIdx.x;
        const int p = y * W + (x < W ? (int)x : 0);
        const bool root = x < W && Lq[p] == p;
        const uint64_t m = __ballot(root);
        if (lane == 0) wc[wv] = popc64(m);
        __syncthreads();
        int pre = 0, tot = 0;
        for (int k = 0; k < CC_WAVES; ++k) {
            if (k < wv) pre += wc[k];
            tot += wc[k];
        }
        if (root) rk[q * hw + p] = base + pre + popc64(m & lanes_below(lane)) + 1;
        base += tot;
        __syncthreads();
    }
    if (y == H - 1 && threadIdx.x == 0) count[q] = base;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_relabel_kernel(const int* __restrict__ L,
                                                             const int* __restrict__ rk, int64_t total,
                                                             int64_t hw, int* __restrict__ labels) {
    for (int64_t i = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * CC_BLOCK) {
        const int v = L[i];
        labels[i] = v < 0 ? 0 : rk[(i / hw) * hw + v];
    }
}

// ---- post-processing ----
// roots only: how many components stay after step 1, and the largest key among them
__global__ __launch_bounds__(CC_BLOCK) void cc_select_kernel(const int* __restrict__ L,
                                                            const int* __restrict__ area,
                                                            int64_t min_area, int* __restrict__ kept,
                                                            unsigned long long* __restrict__ best,
                                                            int H, int W, int chunks) {
    const Pix a = cc_pix(H, W, chunks);
    const int64_t hw = (int64_t)H * W;
    const int lane = threadIdx.x & 63;
    unsigned long long key = 0;
    if (a.in && L[a.q * hw + a.p] == a.p) {
        const int ar = area[a.q * hw + a.p];
        if (cc_keep(ar, min_area)) key = cc_key(ar, a.p);
    }
    const uint64_t m = __ballot(key != 0);
    if (!m) return;  // wave-uniform
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d);
        key = o > key ? o : key;
    }
    if (lane == 0) {
        atomicAdd(&kept[a.q], popc64(m));
        atomicMax(&best[a.q], key);
    }
}

// out = the pixels that stay after steps 1 and 2; info = {components before, components kept,
// foreground pixels (added), 0}
__global__ __launch_bounds__(CC_BLOCK) void cc_write_kernel(const int* __restrict__ L,
                                                           const int* __restrict__ area,
                                                           int64_t min_area, int keep_largest,
                                                           const int* __restrict__ cnt,
                                                           const int* __restrict__ kept,
                                                           const unsigned long long* __restrict__ best,
                                                           uint8_t* __restrict__ out,
                                                           unsigned long long* __restrict__ info, int H,
                                                           int W, int chunks) {
    const Pix a = cc_pix(H, W, chunks);
    const int64_t hw = (int64_t)H * W;
    bool stay = false;
    if (a.in) {
        const int r = L[a.q * hw + a.p];
        if (r >= 0) stay = cc_stays(area[a.q * hw + r], r, min_area, keep_largest != 0, best[a.q]);
        out[a.q * hw + a.p] = stay ? 1 : 0;
    }
    const uint64_t m = __ballot(stay);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&info[4 * a.q + 2], (unsigned long long)popc64(m));
    if (a.y == 0 && a.x == 0) {
        const int k = kept[a.q];
        info[4 * a.q + 0] = (unsigned long long)cnt[a.q];
        info[4 * a.q + 1] = (unsigned long long)(keep_largest ? (k > 0 ? 1 : 0) : k);
    }
}

// the background components (flattened labels) that touch the image border: flag[root] = 1.
// One thread per border pixel: 2 W of the first and last row, then 2 H of the first and last column.
__global__ __launch_bounds__(CC_BLOCK) void cc_mark_border_kernel(const int* __restrict__ L,
                                                                 int* __restrict__ flag, int64_t total,
                                                                 int H, int W) {
    const int64_t idx = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    if (idx >= total) return;
    const int B = 2 * W + 2 * H;
    const int64_t q = idx / B;
    const int i = (int)(idx - q * B);
    int y, x;
    if (i < 2 * W) {
        y = i < W ? 0 : H - 1;
        x = i < W ? i : i - W;
    } else {
        const int j = i - 2 * W;
        x = j < H ? 0 : W - 1;
        y = j < H ? j : j - H;
    }
    const int64_t hw = (int64_t)H * W;
    const int r = L[q * hw + y * W + x];
    if (r >= 0 && flag[q * hw + r] == 0) atomicOr(&flag[q * hw + r], 1);
}

// a background pixel whose component does not touch the border is a hole
__global__ __launch_bounds__(CC_BLOCK) void cc_fill_kernel(const int* __restrict__ L,
                                                          const int* __restrict__ flag,
                                                          uint8_t* __restrict__ out,
                                                          unsigned long long* __restrict__ info, int H,
                                                          int W, int chunks) {
    const Pix a = cc_pix(H, W, chunks);
    const int64_t hw = (int64_t)H * W;
    bool fill = false;
    if (a.in) {
        const int r = L[a.q * hw + a.p];
        fill = r >= 0 && flag[a.q * hw + r] == 0;
        if (fill) out[a.q * hw + a.p] = 1;
    }
    const uint64_t m = __ballot(fill);
    if ((threadIdx.x & 63) == 0 && m) {
        atomicAdd(&info[4 * a.q + 2], (unsigned long long)popc64(m));
        atomicAdd(&info[4 * a.q + 3], (unsigned long long)popc64(m));
    }
}

// ---- lesion statistics: planes [0, N) the prediction, [N, 2N) the targets, labels flattened ----
// a pixel of both masks flags both of its components
__global__ __launch_bounds__(CC_BLOCK) void cc_hits_kernel(const int* __restrict__ L, int* __restrict__ flag,
                                                          int N, int H, int W, int chunks) {
    const Pix a = cc_pix(H, W, chunks);
    if (!a.in) return;
    const int64_t hw = (int64_t)H * W;
    const int64_t bp = a.q * hw, bg = (a.q + (int64_t)N) * hw;
    const int rp = L[bp + a.p], rg = L[bg + a.p];
    if (rp < 0 || rg < 0) return;
    if (flag[bp + rp] == 0) atomicOr(&flag[bp + rp], 1);
    if (flag[bg + rg] == 0) atomicOr(&flag[bg + rg], 1);
}

// out[4 n ..] += {n_pred, n_gt, gt_hit, pred_hit}: the roots of both plane sets and their flags
__global__ __launch_bounds__(CC_BLOCK) void cc_hit_count_kernel(const int* __restrict__ L,
                                                               const int* __restrict__ flag,
                                                               unsigned long long* __restrict__ out,
                                                               int N, int H, int W, int chunks) {
    const Pix a = cc_pix(H, W, chunks);  // q in [0, 2N)
    const int64_t hw = (int64_t)H * W;
    const bool root = a.in && L[a.q * hw + a.p] == a.p;
    const bool hit = root && flag[a.q * hw + a.p] != 0;
    const uint64_t mr = __ballot(root), mh = __ballot(hit);
    if ((threadIdx.x & 63) != 0 || !mr) return;
    const bool gt = a.q >= N;
    unsigned long long* o = out + 4 * (int64_t)(gt ? a.q - N : a.q);
    atomicAdd(&o[gt ? 1 : 0], (unsigned long long)popc64(mr));
    if (mh) atomicAdd(&o[gt ? 2 : 3], (unsigned long long)popc64(mh));
}

int64_t align64(int64_t b) { return (b + 63) & ~(int64_t)63; }
int chunks_of(int W) { return (W + CC_BLOCK - 1) / CC_BLOCK; }
unsigned pix_grid(int planes, int H, int W) { return (unsigned)((int64_t)planes * H * chunks_of(W)); }

}  // namespace

int cc_tile_rows(int tile) { return tile == 0 ? 16 : tile == 2 ? 64 : 32; }

// every grid of a call over `planes` planes fits a launch
bool cc_grid_ok(int planes, int H, int W) {
    const int64_t lim = (int64_t)1 << 31;
    const int64_t hw = (int64_t)H * W;
    return hw < lim && 2 * ((int64_t)W + H) < lim && (int64_t)planes * H * chunks_of(W) < lim && (int64_t)planes * (2 * (int64_t)W + 2 * H) < lim * 256 &&
           (int64_t)planes * ((hw + 1023) / 1024 + H + W) < lim;
}

// scratch: [N best keys][planes counts][N kept][planes H row counts] (zeroed by every call),
// then [planes H W labels][planes H W areas / flags / ranks]; each part aligned to 64 bytes
CcScratch cc_scratch(void* base, int N, int planes, int H, int W) {
    const int64_t hw = (int64_t)H * W;
    CcScratch s;
    char* p = (char*)base;
    s.best = (unsigned long long*)p;
    p += align64(8 * (int64_t)N);
    s.cnt = (int*)p;
    p += align64(4 * (int64_t)planes);
    s.kept = (int*)p;
    p += align64(4 * (int64_t)N);
    s.rowcnt = (int*)p;
    p += align64(4 * (int64_t)planes * H);
    s.zero_bytes = (size_t)(p - (char*)base);
    s.L = (int*)p;
    p += align64(4 * planes * hw);
    s.area = (int*)p;
    p += align64(4 * planes * hw);
    s.bytes = (size_t)(p - (char*)base);
    return s;
}

int k_cc_tile(const void* src, int kind, int64_t sample_stride, int planes, int H, int W, int conn,
              int tile, int* L, int* area, hipStream_t s) {
    const int TH = cc_tile_rows(tile);
    const int nTx = (W + CC_TILE_W - 1) / CC_TILE_W, nTy = (H + TH - 1) / TH;
    const dim3 grid((unsigned)((int64_t)planes * nTx * nTy)), block(CC_BLOCK);
    if (TH == 16)
        hipLaunchKernelGGL(cc_tile_kernel<16>, grid, block, 0, s, src, kind, sample_stride, H, W, nTx, nTy, conn, L, area);
    else if (TH == 64)
        hipLaunchKernelGGL(cc_tile_kernel<64>, grid, block, 0, s, src, kind, sample_stride, H, W, nTx, nTy, conn, L, area);
    else
        hipLaunchKernelGGL(cc_tile_kernel<32>, grid, block, 0, s, src, kind, sample_stride, H, W, nTx, nTy, conn, L, area);
    return (int)hipGetLastError();
}

int k_cc_seam(int* L, int planes, int H, int W, int conn, int tile, hipStream_t s) {
    const int TH = cc_tile_rows(tile);
    const int nTx = (W + CC_TILE_W - 1) / CC_TILE_W, nTy = (H + TH - 1) / TH;
    const int64_t nh = (int64_t)(nTy - 1) * W, nv = (int64_t)(nTx - 1) * H;  // < 2 H W / 16
    const int64_t total = planes * (nh + nv);
    if (total == 0) return 0;
    hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)((total + CC_BLOCK - 1) / CC_BLOCK)), dim3(CC_BLOCK), 0,
                       s, L, total, H, W, TH, (int)nh, (int)nv, conn);
    return (int)hipGetLastError();
}

int k_cc_flatten(int* L, int* area, int* rowcnt, int* cnt, int planes, int H, int W, hipStream_t s) {
    const dim3 grid(pix_grid(planes, H, W)), block(CC_BLOCK);
    if (area)
        hipLaunchKernelGGL(cc_flatten_kernel<true>, grid, block, 0, s, L, area, rowcnt, cnt, H, W, chunks_of(W));
    else
        hipLaunchKernelGGL(cc_flatten_kernel<false>, grid, block, 0, s, L, area, rowcnt, cnt, H, W, chunks_of(W));
    return (int)hipGetLastError();
}

int k_cc_rank(const int* L, int* rk, const int* rowcnt, int* count, int planes, int H, int W,
              int* labels, hipStream_t s) {
    hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)((int64_t)planes * H)), dim3(CC_BLOCK), 0, s, L, rk,
                       rowcnt, count, H, W);
    HIP_OK(hipGetLastError());
    const int64_t hw = (int64_t)H * W, total = planes * hw;
    const unsigned grid = (unsigned)std::min<int64_t>((total + CC_BLOCK - 1) / CC_BLOCK, 4096);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(grid), dim3(CC_BLOCK), 0, s, L, rk, total, hw, labels);
    return (int)hipGetLastError();
}

int k_cc_select(const int* L, const int* area, int64_t min_area, int* kept, unsigned long long* best,
                int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(cc_select_kernel, dim3(pix_grid(N, H, W)), dim3(CC_BLOCK), 0, s, L, area, min_area,
                       kept, best, H, W, chunks_of(W));
    return (int)hipGetLastError();
}

int k_cc_write(const int* L, const int* area, int64_t min_area, int keep_largest, const int* cnt,
               const int* kept, const unsigned long long* best, uint8_t* out, int64_t* info, int N, int H,
               int W, hipStream_t s) {
    hipLaunchKernelGGL(cc_write_kernel, dim3(pix_grid(N, H, W)), dim3(CC_BLOCK), 0, s, L, area, min_area,
                       keep_largest, cnt, kept, best, out, (unsigned long long*)info, H, W, chunks_of(W));
    return (int)hipGetLastError();
}

int k_cc_fill(const int* L, int* flag, uint8_t* out, int64_t* info, int N, int H, int W, hipStream_t s) {
    const int64_t total = (int64_t)N * (2 * (int64_t)W + 2 * H);
    hipLaunchKernelGGL(cc_mark_border_kernel, dim3((unsigned)((total + CC_BLOCK - 1) / CC_BLOCK)),
                       dim3(CC_BLOCK), 0, s, L, flag, total, H, W);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(cc_fill_kernel, dim3(pix_grid(N, H, W)), dim3(CC_BLOCK), 0, s, L, flag, out,
                       (unsigned long long*)info, H, W, chunks_of(W));
    return (int)hipGetLastError();
}

int k_cc_hits(const int* L, int* flag, int64_t* out, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(cc_hits_kernel, dim3(pix_grid(N, H, W)), dim3(CC_BLOCK), 0, s, L, flag, N, H, W,
                       chunks_of(W));
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(cc_hit_count_kernel, dim3(pix_grid(2 * N, H, W)), dim3(CC_BLOCK), 0, s, L, flag,
                       (unsigned long long*)out, N, H, W, chunks_of(W));
    return (int)hipGetLastError();
}

// ---- the same on the host, one plane at a time, through the same rules ----
namespace {

// L: H W labels of one plane (root = smallest index of the component, flattened; -1 background);
// area (may be null): pixels per root.  Returns the number of components.
int label_plane_host(const void* src, int kind, int64_t off0, int H, int W, int conn, int* L, int* area) {
    const auto amin = [](int* slot, int v) {
        const int old = *slot;
        if (v < old) *slot = v;
        return old;
    };
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            const int p = i * W + j;
            L[p] = cc_fg(src, kind, off0 + p) ? p : -1;
            if (area) area[p] = 0;
        }
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            const int p = i * W + j;
            if (L[p] < 0) continue;
            if (j > 0 && L[p - 1] >= 0) cc_union(L, p, p - 1, amin);
            if (i > 0 && L[p - W] >= 0) cc_union(L, p, p - W, amin);
            if (conn == 2 && i > 0) {
                if (j > 0 && L[p - W - 1] >= 0) cc_union(L, p, p - W - 1, amin);
                if (j + 1 < W && L[p - W + 1] >= 0) cc_union(L, p, p - W + 1, amin);
            }
        }
    int k = 0;
    for (int p = 0; p < H * W; ++p) {
        if (L[p] < 0) continue;
        L[p] = cc_find(L, p);
        k += L[p] == p;
        if (area) area[L[p]] += 1;
    }
    return k;
}

}  // namespace

void components_host(const void* src, int kind, int N, int C, int H, int W, int conn, int* labels,
                     int* count) {
    const int64_t hw = (int64_t)H * W;
    std::vector<int> rk((size_t)hw);
    for (int n = 0; n < N; ++n) {
        int* L = labels + n * hw;
        label_plane_host(src, kind, n * C * hw, H, W, conn, L, nullptr);
        int k = 0;
        for (int64_t p = 0; p < hw; ++p)
            if (L[p] == p) rk[p] = ++k;  // raster order of the roots
        for (int64_t p = 0; p < hw; ++p) L[p] = L[p] < 0 ? 0 : rk[L[p]];
        count[n] = k;
    }
}

void postprocess_host(const void* src, int kind, int N, int C, int H, int W, int conn, int keep_largest,
                      int64_t min_area, int fill_holes, uint8_t* out, int64_t* info) {
    const int64_t hw = (int64_t)H * W;
    std::vector<int> L((size_t)hw), area((size_t)hw);
    for (int n = 0; n < N; ++n) {
        uint8_t* o = out + n * hw;
        int64_t* f = info + 4 * (int64_t)n;
        f[0] = label_plane_host(src, kind, n * C * hw, H, W, conn, L.data(), area.data());
        f[1] = f[2] = f[3] = 0;
        uint64_t best = 0;
        for (int64_t p = 0; p < hw; ++p)
            if (L[p] == p && cc_keep(area[p], min_area)) {
                f[1] += 1;
                const uint64_t key = cc_key(area[p], (int)p);
                best = key > best ? key : best;
            }
        if (keep_largest) f[1] = f[1] > 0 ? 1 : 0;
        for (int64_t p = 0; p < hw; ++p) {
            const int r = L[p];
            o[p] = r >= 0 && cc_stays(area[r], r, min_area, keep_largest != 0, best) ? 1 : 0;
            f[2] += o[p];
        }
        if (!fill_holes) continue;
        label_plane_host(o, CC_KIND_U8_ZERO, 0, H, W, 1, L.data(), nullptr);
        std::fill(area.begin(), area.end(), 0);  // now the flags of the background components
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j)
                if (cc_on_border(i, j, H, W) && L[i * W + j] >= 0) area[L[i * W + j]] = 1;
        for (int64_t p = 0; p < hw; ++p)
            if (L[p] >= 0 && area[L[p]] == 0) {
                o[p] = 1;
                f[2] += 1;
                f[3] += 1;
            }
    }
}

void lesion_stats_host(const void* pred, int kind, const float* targets, int N, int C, int H, int W,
                       int conn, int64_t* out) {
    const int64_t hw = (int64_t)H * W;
    std::vector<int> LP((size_t)hw), LG((size_t)hw), fp((size_t)hw), fg((size_t)hw);
    for (int n = 0; n < N; ++n) {
        int64_t* o = out + 4 * (int64_t)n;
        o[0] = label_plane_host(pred, kind, n * C * hw, H, W, conn, LP.data(), nullptr);
        o[1] = label_plane_host(targets, CC_KIND_TARGETS, n * C * hw, H, W, conn, LG.data(), nullptr);
        std::fill(fp.begin(), fp.end(), 0);
        std::fill(fg.begin(), fg.end(), 0);
        for (int64_t p = 0; p < hw; ++p)
            if (LP[p] >= 0 && LG[p] >= 0) fp[LP[p]] = fg[LG[p]] = 1;
        o[2] = o[3] = 0;
        for (int64_t p = 0; p < hw; ++p) {
            o[2] += LG[p] == p && fg[p];
            o[3] += LP[p] == p && fp[p];
        }
    }
}
