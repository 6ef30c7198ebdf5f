// Test-time augmentation (rules in tta.h): the dihedral views of a batch and the fused un-warp +
// merge of the per-view logits.  Both are streaming kernels: every input element is read once
// per view it appears in and every output element is written once, (4 K + 4 + 2) bytes per
// output element for the merge.  No scratch, no atomics, no host synchronisation.
//
//   views, t = 0   tta_views_vec_kernel: a thread moves one float4 of a row, reversed in its
//                  registers for h, when W % 4 == 0 and both pointers are 16-byte aligned;
//                  tta_views_scalar_kernel (one float per thread) otherwise.
//   views, t = 1   tta_views_tr_kernel: a 64 x 64 tile through LDS (row stride 65), so that the
//                  global read runs along the source rows and the global write along the output
//                  rows, both coalesced, and neither LDS access has a bank conflict.
//   merge          tta_merge_vec_kernel when no view is transposed and the float4 conditions
//                  hold: a thread owns four consecutive outputs, loads the K float4s first and
//                  then sums them in ascending view order.  tta_merge_tile_kernel otherwise: a
//                  block owns a 64 x 64 output tile, a thread 16 of its elements (one column, every
//                  fourth row); it walks the views in ascending order with the sums in registers,
//                  reads t = 0 views straight from global memory (lanes along the row) and stages
//                  t = 1 views through the same LDS transpose as the views kernel.
// The planes of a call ((n, c) pairs) are walked by blockIdx.y with a stride, so any N C fits.
#include "tta.h"
#include "kernels_misc.h"

namespace {

constexpr int TTA_BLOCK = 256;
constexpr int TTA_TILE = 64;
constexpr int TTA_STRIDE = TTA_TILE + 1;
constexpr int TTA_ROWS = TTA_BLOCK / TTA_TILE;  // tile rows one pass of the block covers
constexpr int TTA_OWN = TTA_TILE / TTA_ROWS;    // elements of a tile a thread owns
constexpr unsigned TTA_MAX_GRID_Y = 65535;

// the views one launch handles: view k[z] is number q[z] of the stack
struct TtaLaunchList {
    int n;
    int k[TTA_MAX_VIEWS];
    int q[TTA_MAX_VIEWS];
};

__device__ __forceinline__ float4 rev4(float4 v) { return make_float4(v.w, v.z, v.y, v.x); }

__global__ __launch_bounds__(TTA_BLOCK) void tta_views_vec_kernel(const float* __restrict__ x,
                                                                  float* __restrict__ out, int planes,
                                                                  int H, int W4, TtaLaunchList l) {
    const int e = blockIdx.x * TTA_BLOCK + threadIdx.x;
    if (e >= H * W4) return;
    const int i = e / W4, j4 = e - i * W4;
    const int k = l.k[blockIdx.z], q = l.q[blockIdx.z];
    const bool h = tta_h(k);
    const int src = (tta_v(k) ? H - 1 - i : i) * W4 + (h ? W4 - 1 - j4 : j4);
    const int64_t hw = (int64_t)H * W4 * 4;
    for (int p = blockIdx.y; p < planes; p += gridDim.y) {
        float4 v = reinterpret_cast<const float4*>(x + p * hw)[src];
        if (h) v = rev4(v);
        reinterpret_cast<float4*>(out + ((int64_t)q * planes + p) * hw)[e] = v;
    }
}

__global__ __launch_bounds__(TTA_BLOCK) void tta_views_scalar_kernel(const float* __restrict__ x,
                                                                     float* __restrict__ out, int planes,
                                                                     int H, int W, TtaLaunchList l) {
    const int e = blockIdx.x * TTA_BLOCK + threadIdx.x;
    if (e >= H * W) return;
    const int i = e / W, j = e - i * W;
    const int k = l.k[blockIdx.z], q = l.q[blockIdx.z];
    int si, sj;
    tta_fwd(k, i, j, H, W, si, sj);  // t = 0 here
    const int src = si * W + sj;
    const int64_t hw = (int64_t)H * W;
    for (int p = blockIdx.y; p < planes; p += gridDim.y) out[((int64_t)q * planes + p) * hw + e] = x[p * hw + src];
}

// tile[lj][li] = src[fr ? S-1-j : j][fc ? S-1-i : i] for the output-tile element i = oi0 + li,
// j = oj0 + lj of an S x S plane: the lanes of a wave run along li, i.e. along a source row
__device__ __forceinline__ void tta_stage_transposed(float* tile, const float* __restrict__ src, int S,
                                                     int oi0, int oj0, bool fr, bool fc) {
    const int li = threadIdx.x & (TTA_TILE - 1), l0 = threadIdx.x / TTA_TILE;
    const int i = oi0 + li;
    const int sc = fc ? S - 1 - i : i;
#pragma unroll
    for (int m = 0; m < TTA_OWN; ++m) {
        const int lj = l0 + m * TTA_ROWS;
        const int j = oj0 + lj;
        if (i < S && j < S) tile[lj * TTA_STRIDE + li] = src[(int64_t)(fr ? S - 1 - j : j) * S + sc];
    }
}

__global__ __launch_bounds__(TTA_BLOCK) void tta_views_tr_kernel(const float* __restrict__ x,
                                                                 float* __restrict__ out, int planes, int S,
                                                                 int tiles, TtaLaunchList l) {
    __shared__ float tile[TTA_TILE * TTA_STRIDE];
    const int oi0 = (blockIdx.x / tiles) * TTA_TILE, oj0 = (blockIdx.x % tiles) * TTA_TILE;
    const int k = l.k[blockIdx.z], q = l.q[blockIdx.z];
    const int lj = threadIdx.x & (TTA_TILE - 1), l0 = threadIdx.x / TTA_TILE;
    const int64_t hw = (int64_t)S * S;
    for (int p = blockIdx.y; p < planes; p += gridDim.y) {
        // T_k(x)[i, j] = x[h ? S-1-j : j][v ? S-1-i : i]
        tta_stage_transposed(tile, x + p * hw, S, oi0, oj0, tta_h(k), tta_v(k));
        __syncthreads();
        float* o = out + ((int64_t)q * planes + p) * hw;
#pragma unroll
        for (int m = 0; m < TTA_OWN; ++m) {
            const int li = l0 + m * TTA_ROWS;
            if (oi0 + li < S && oj0 + lj < S) o[(int64_t)(oi0 + li) * S + oj0 + lj] = tile[lj * TTA_STRIDE + li];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(TTA_BLOCK) void tta_merge_vec_kernel(const float* __restrict__ logits, int planes,
                                                                  int H, int W4, TtaViews l, int mode,
                                                                  float* __restrict__ score,
                                                                  uint8_t* __restrict__ mask,
                                                                  uint8_t* __restrict__ votes) {
    const int e = blockIdx.x * TTA_BLOCK + threadIdx.x;
    if (e >= H * W4) return;
    const int i = e / W4, j4 = e - i * W4;
    const int64_t hw = (int64_t)H * W4 * 4;
    int src[TTA_MAX_VIEWS];
#pragma unroll
    for (int q = 0; q < TTA_MAX_VIEWS; ++q)
        if (q < l.K) src[q] = (tta_v(l.k[q]) ? H - 1 - i : i) * W4 + (tta_h(l.k[q]) ? W4 - 1 - j4 : j4);
    for (int p = blockIdx.y; p < planes; p += gridDim.y) {
        float4 x[TTA_MAX_VIEWS];
#pragma unroll
        for (int q = 0; q < TTA_MAX_VIEWS; ++q)
            if (q < l.K) {
                x[q] = reinterpret_cast<const float4*>(logits + ((int64_t)q * planes + p) * hw)[src[q]];
                if (tta_h(l.k[q])) x[q] = rev4(x[q]);
            }
        TtaAcc a[4] = {};
#pragma unroll
        for (int q = 0; q < TTA_MAX_VIEWS; ++q)
            if (q < l.K) {
                tta_acc_add(a[0], q, x[q].x, mode);
                tta_acc_add(a[1], q, x[q].y, mode);
                tta_acc_add(a[2], q, x[q].z, mode);
                tta_acc_add(a[3], q, x[q].w, mode);
            }
        const float4 sc = make_float4(tta_score(a[0], l.K), tta_score(a[1], l.K), tta_score(a[2], l.K),
                                      tta_score(a[3], l.K));
        reinterpret_cast<float4*>(score + p * hw)[e] = sc;
        if (mask)
            reinterpret_cast<uchar4*>(mask + p * hw)[e] =
                make_uchar4(tta_mask(sc.x, mode), tta_mask(sc.y, mode), tta_mask(sc.z, mode), tta_mask(sc.w, mode));
        if (votes)
            reinterpret_cast<uchar4*>(votes + p * hw)[e] =
                make_uchar4((uint8_t)a[0].votes, (uint8_t)a[1].votes, (uint8_t)a[2].votes, (uint8_t)a[3].votes);
    }
}

__global__ __launch_bounds__(TTA_BLOCK) void tta_merge_tile_kernel(const float* __restrict__ logits, int planes,
                                                                   int H, int W, int tiles_j, TtaViews l,
                                                                   int mode, float* __restrict__ score,
                                                                   uint8_t* __restrict__ mask,
                                                                   uint8_t* __restrict__ votes) {
    __shared__ float tile[TTA_TILE * TTA_STRIDE];
    const int oi0 = (blockIdx.x / tiles_j) * TTA_TILE, oj0 = (blockIdx.x % tiles_j) * TTA_TILE;
    const int lj = threadIdx.x & (TTA_TILE - 1), l0 = threadIdx.x / TTA_TILE;
    const int j = oj0 + lj;
    const int64_t hw = (int64_t)H * W;
    for (int p = blockIdx.y; p < planes; p += gridDim.y) {
        TtaAcc a[TTA_OWN] = {};
        for (int q = 0; q < l.K; ++q) {
            const int k = l.k[q];
            const float* L = logits + ((int64_t)q * planes + p) * hw;
            float x[TTA_OWN];
            if (tta_t(k)) {  // H == W; T_k^-1(L)[i, j] = L[v ? H-1-j : j][h ? W-1-i : i]
                tta_stage_transposed(tile, L, H, oi0, oj0, tta_v(k), tta_h(k));
                __syncthreads();
#pragma unroll
                for (int m = 0; m < TTA_OWN; ++m) x[m] = tile[lj * TTA_STRIDE + l0 + m * TTA_ROWS];
                __syncthreads();
            } else {
                const int sj = tta_h(k) ? W - 1 - j : j;
#pragma unroll
                for (int m = 0; m < TTA_OWN; ++m) {
                    const int i = oi0 + l0 + m * TTA_ROWS;
                    x[m] = (i < H && j < W) ? L[(int64_t)(tta_v(k) ? H - 1 - i : i) * W + sj] : 0.f;
                }
            }
#pragma unroll
            for (int m = 0; m < TTA_OWN; ++m) tta_acc_add(a[m], q, x[m], mode);
        }
#pragma unroll
        for (int m = 0; m < TTA_OWN; ++m) {
            const int i = oi0 + l0 + m * TTA_ROWS;
            if (i < H && j < W) {
                const int64_t o = p * hw + (int64_t)i * W + j;
                const float sc = tta_score(a[m], l.K);
                score[o] = sc;
                if (mask) mask[o] = tta_mask(sc, mode);
                if (votes) votes[o] = (uint8_t)a[m].votes;
            }
        }
    }
}

bool aligned(const void* p, size_t a) { return p == nullptr || (uintptr_t)p % a == 0; }
unsigned plane_grid(int planes) { return (unsigned)std::min<int64_t>(planes, TTA_MAX_GRID_Y); }
unsigned chunks(int64_t n) { return (unsigned)((n + TTA_BLOCK - 1) / TTA_BLOCK); }

}  // namespace

int k_tta_views(const float* x, int N, int C, int H, int W, uint32_t views, float* out, hipStream_t s) {
    const TtaViews all = tta_view_list(views);
    TtaLaunchList direct{}, tr{};
    for (int q = 0; q < all.K; ++q) {
        TtaLaunchList& l = tta_t(all.k[q]) ? tr : direct;
        l.k[l.n] = all.k[q];
        l.q[l.n++] = q;
    }
    const int planes = N * C;
    if (direct.n) {
        if (W % 4 == 0 && aligned(x, 16) && aligned(out, 16))
            hipLaunchKernelGGL(tta_views_vec_kernel, dim3(chunks((int64_t)H * (W / 4)), plane_grid(planes), direct.n),
                               dim3(TTA_BLOCK), 0, s, x, out, planes, H, W / 4, direct);
        else
            hipLaunchKernelGGL(tta_views_scalar_kernel, dim3(chunks((int64_t)H * W), plane_grid(planes), direct.n),
                               dim3(TTA_BLOCK), 0, s, x, out, planes, H, W, direct);
        HIP_OK(hipGetLastError());
    }
    if (tr.n) {
        const int tiles = (H + TTA_TILE - 1) / TTA_TILE;
        hipLaunchKernelGGL(tta_views_tr_kernel, dim3((unsigned)(tiles * tiles), plane_grid(planes), tr.n),
                           dim3(TTA_BLOCK), 0, s, x, out, planes, H, tiles, tr);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int k_tta_merge(const float* logits, int N, int C, int H, int W, uint32_t views, int mode, float* score,
                uint8_t* mask, uint8_t* votes, hipStream_t s) {
    const TtaViews l = tta_view_list(views);
    const int planes = N * C;
    if ((views & 0xF0u) == 0 && W % 4 == 0 && aligned(logits, 16) && aligned(score, 16) && aligned(mask, 4) &&
        aligned(votes, 4)) {
        hipLaunchKernelGGL(tta_merge_vec_kernel, dim3(chunks((int64_t)H * (W / 4)), plane_grid(planes)),
                           dim3(TTA_BLOCK), 0, s, logits, planes, H, W / 4, l, mode, score, mask, votes);
    } else {
        const int ti = (H + TTA_TILE - 1) / TTA_TILE, tj = (W + TTA_TILE - 1) / TTA_TILE;
        hipLaunchKernelGGL(tta_merge_tile_kernel, dim3((unsigned)(ti * tj), plane_grid(planes)), dim3(TTA_BLOCK), 0,
                           s, logits, planes, H, W, tj, l, mode, score, mask, votes);
    }
    return (int)hipGetLastError();
}

// ---- host twins: the same tta.h maps and accumulator, one element at a time ----
void tta_views_host(const float* x, int N, int C, int H, int W, uint32_t views, float* out) {
    const TtaViews l = tta_view_list(views);
    const int64_t planes = (int64_t)N * C, hw = (int64_t)H * W;
    for (int q = 0; q < l.K; ++q)
        for (int64_t p = 0; p < planes; ++p)
            for (int i = 0; i < H; ++i)
                for (int j = 0; j < W; ++j) {
                    int si, sj;
                    tta_fwd(l.k[q], i, j, H, W, si, sj);
                    out[(q * planes + p) * hw + (int64_t)i * W + j] = x[p * hw + (int64_t)si * W + sj];
                }
}

void tta_merge_host(const float* logits, int N, int C, int H, int W, uint32_t views, int mode, float* score,
                    uint8_t* mask, uint8_t* votes) {
    const TtaViews l = tta_view_list(views);
    const int64_t planes = (int64_t)N * C, hw = (int64_t)H * W;
    for (int64_t p = 0; p < planes; ++p)
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                TtaAcc a{};
                for (int q = 0; q < l.K; ++q) {
                    int si, sj;
                    tta_inv(l.k[q], i, j, H, W, si, sj);
                    tta_acc_add(a, q, logits[(q * planes + p) * hw + (int64_t)si * W + sj], mode);
                }
                const int64_t o = p * hw + (int64_t)i * W + j;
                const float sc = tta_score(a, l.K);
                score[o] = sc;
                if (mask) mask[o] = tta_mask(sc, mode);
                if (votes) votes[o] = (uint8_t)a.votes;
            }
}
