// Surface-distance statistics of a batch on the device (surf.h: definition, masks, border rule,
// selection): border planes -> exact squared distance transform of both -> per-direction
// gather -> radix select of the two order statistics HD95 interpolates between.  Five launches
// and one memset on the caller's stream, no host synchronisation; every sum is formed in a
// fixed order and every count with integer atomics, so two runs agree bit for bit.
#include "surf.h"
#include "kernels_misc.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int SURF_BLOCK = 256;
constexpr int SURF_COL_BLOCK = 64;   // as the EDT column pass: one wave, many CUs
constexpr int SURF_SEL_BLOCK = 1024;

// Planes.  Plane q in [0, N) is sample q's prediction, plane N + n sample n's target; the
// partner of a plane is the other plane of its sample.
__device__ __forceinline__ int partner(int q, int N) { return q < N ? q + N : q - N; }

// Border planes: one thread per pixel, x fastest (coalesced uint8 stores).
__global__ __launch_bounds__(SURF_BLOCK) void surf_border_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ t,
                                                                int N, int C, int H, int W,
                                                                uint8_t* __restrict__ border) {
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    const int64_t idx = blockIdx.x * (int64_t)SURF_BLOCK + threadIdx.x;
    if (idx >= total) return;
    const int64_t n = idx / hw, r = idx - n * hw;
    const int i = (int)(r / W), j = (int)(r - (int64_t)i * W);
    const float* xs = x + n * C * hw;
    const float* ts = t + n * C * hw;
    border[idx] = surf_border([&](int a, int b) { return surf_pred(xs[(int64_t)a * W + b]); }, i, j, H, W);
    border[total + idx] =
        surf_border([&](int a, int b) { return surf_target(ts[(int64_t)a * W + b]); }, i, j, H, W);
}

// Column pass of edt.h over the 2N border planes: one thread per (plane, column).  flags[q]
// (zeroed by the launcher) becomes 1 when plane q has a border pixel, i.e. its mask is not empty.
__global__ __launch_bounds__(SURF_COL_BLOCK) void surf_columns_kernel(const uint8_t* __restrict__ border,
                                                                     int planes, int H, int W,
                                                                     int* __restrict__ g2,
                                                                     int* __restrict__ flags) {
    const int idx = blockIdx.x * SURF_COL_BLOCK + threadIdx.x;
    if (idx >= planes * W) return;
    const int q = idx / W, j = idx - q * W;
    const int64_t hw = (int64_t)H * W;
    const bool any = edt_column(border + q * hw + j, g2 + q * hw + j, H, W);
    if (any) atomicOr(&flags[q], 1);
}

// Row pass: one block per (plane, row), the row of g^2 in LDS, the squared distance written
// over it -- only where the partner plane has a border pixel, the only places the gather and the
// select read it (a surface is a few pixels per row, and the scan from a pixel far from every
// site is the long one).  Nothing runs for an undefined sample or a row without such a pixel
// (both block-uniform).
__global__ __launch_bounds__(SURF_BLOCK) void surf_rows_kernel(const uint8_t* __restrict__ border,
                                                              int* __restrict__ g2,
                                                              const int* __restrict__ flags, int N,
                                                              int H, int W) {
    extern __shared__ int row[];
    const int q = blockIdx.x / H, i = blockIdx.x - q * H;
    const int p = partner(q, N);
    if (flags[q] == 0 || flags[p] == 0) return;
    const uint8_t* pb = border + ((int64_t)p * H + i) * W;
    int any = 0;
    for (int j = threadIdx.x; j < W; j += SURF_BLOCK) any |= pb[j];
    if (!__syncthreads_or(any)) return;
    int* g = g2 + ((int64_t)q * H + i) * W;
    for (int j = threadIdx.x; j < W; j += SURF_BLOCK) row[j] = g[j];
    __syncthreads();
    for (int j = threadIdx.x; j < W; j += SURF_BLOCK)
        if (pb[j]) g[j] = edt_row_min(row, W, j);
}

// Gather: block (q, g) accumulates, over chunk g of plane q's border pixels, the squared
// distance to the partner plane's border.  A thread's pixels in index order, the wave by a
// butterfly, the four waves in order: the partial is the same in every run.
__global__ __launch_bounds__(SURF_BLOCK) void surf_gather_kernel(const uint8_t* __restrict__ border,
                                                                const int* __restrict__ d2,
                                                                const int* __restrict__ flags,
                                                                int N, int64_t hw, int G,
                                                                int* __restrict__ pn,
                                                                int* __restrict__ pmax,
                                                                double* __restrict__ psum) {
    __shared__ int rn[4], rm[4];
    __shared__ double rs[4];
    const int q = blockIdx.x / G, g = blockIdx.x - q * G;
    const int p = partner(q, N);
    if (flags[q] == 0 || flags[p] == 0) return;
    const int64_t chunk = (hw + G - 1) / G;
    const int64_t i0 = g * chunk, i1 = min(hw, i0 + chunk);
    const uint8_t* b = border + q * hw;
    const int* d = d2 + p * hw;
    SurfAcc a = surf_acc_zero();
    for (int64_t i = i0 + threadIdx.x; i < i1; i += SURF_BLOCK)
        if (b[i]) surf_acc_add(a, d[i]);
    for (int s = 32; s >= 1; s >>= 1) {
        SurfAcc o;
        o.n = __shfl_xor(a.n, s);
        o.max_d2 = __shfl_xor(a.max_d2, s);
        o.sum = __shfl_xor(a.sum, s);
        // the lower lane's value first on both sides of the exchange: one result per wave
        a = (threadIdx.x & s) ? surf_acc_merge(o, a) : surf_acc_merge(a, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        rn[w] = a.n;
        rm[w] = a.max_d2;
        rs[w] = a.sum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    SurfAcc r = SurfAcc{rn[0], rm[0], rs[0]};
    for (int k = 1; k < 4; ++k) r = surf_acc_merge(r, SurfAcc{rn[k], rm[k], rs[k]});
    pn[blockIdx.x] = r.n;
    pmax[blockIdx.x] = r.max_d2;
    psum[blockIdx.x] = r.sum;
}

// One block per sample: merge the gather partials in index order, write the sample's fields,
// then select d2_lo and d2_hi from the union multiset of both directions.
__global__ __launch_bounds__(SURF_SEL_BLOCK) void surf_select_kernel(const uint8_t* __restrict__ border,
                                                                    const int* __restrict__ d2,
                                                                    const int* __restrict__ flags,
                                                                    int N, int64_t hw, int G,
                                                                    const int* __restrict__ pn,
                                                                    const int* __restrict__ pmax,
                                                                    const double* __restrict__ psum,
                                                                    int64_t* __restrict__ out_i64,
                                                                    double* __restrict__ out_f64) {
    __shared__ int hist[2 * SURF_BINS];  // one histogram per state
    __shared__ SurfSel sel[2];
    __shared__ int top;  // < 0: undefined sample
    const int n = blockIdx.x, tid = threadIdx.x;
    int64_t* oi = out_i64 + 6 * (int64_t)n;
    double* of = out_f64 + 2 * (int64_t)n;
    if (tid == 0) {
        if (flags[n] == 0 || flags[N + n] == 0) {
            for (int k = 0; k < 6; ++k) oi[k] = 0;
            of[0] = of[1] = 0.0;
            top = -1;
        } else {
            SurfAcc a[2];
            for (int dir = 0; dir < 2; ++dir) {
                const int64_t base = ((int64_t)dir * N + n) * G;
                a[dir] = surf_acc_zero();
                for (int g = 0; g < G; ++g)
                    a[dir] = surf_acc_merge(a[dir], SurfAcc{pn[base + g], pmax[base + g], psum[base + g]});
            }
            const int mx = a[0].max_d2 > a[1].max_d2 ? a[0].max_d2 : a[1].max_d2;
            oi[0] = 1;
            oi[1] = a[0].n;
            oi[2] = a[1].n;
            oi[3] = mx;
            of[0] = a[0].sum;
            of[1] = a[1].sum;
            int lo, hi;
            surf_ranks(a[0].n + a[1].n, lo, hi);
            sel[0] = SurfSel{0u, lo};
            sel[1] = SurfSel{0u, hi};
            top = surf_top_shift(mx);
        }
    }
    __syncthreads();
    if (top < 0) return;
    for (int shift = top; shift >= 0; shift -= SURF_DIGIT_BITS) {
        if (tid < 2 * SURF_BINS) hist[tid] = 0;
        __syncthreads();
        const SurfSel s0 = sel[0], s1 = sel[1];
        for (int dir = 0; dir < 2; ++dir) {
            const uint8_t* b = border + ((int64_t)dir * N + n) * hw;
            const int* d = d2 + ((int64_t)(1 - dir) * N + n) * hw;
            for (int64_t i = tid; i < hw; i += SURF_SEL_BLOCK) {
                if (!b[i]) continue;
                const uint32_t key = (uint32_t)d[i];
                const int dg = surf_digit(key, shift);
                if (surf_sel_match(s0, key, shift)) atomicAdd(&hist[dg], 1);
                if (surf_sel_match(s1, key, shift)) atomicAdd(&hist[SURF_BINS + dg], 1);
            }
        }
        __syncthreads();
        if (tid == 0 || tid == 64) {  // one wave per state
            SurfSel s = sel[tid >> 6];
            surf_select_step(s, hist + (tid >> 6) * SURF_BINS, shift);
            sel[tid >> 6] = s;
        }
        __syncthreads();
    }
    if (tid == 0) {
        oi[4] = sel[0].prefix;
        oi[5] = sel[1].prefix;
    }
}

int64_t align64(int64_t b) { return (b + 63) & ~(int64_t)63; }

}  // namespace

// chunks per (sample, direction) of the gather: a function of the sample size only
int surf_groups(int64_t hw) { return (int)std::min<int64_t>(64, std::max<int64_t>(1, hw / 4096)); }

// scratch: [2N G float64 sums][2N H W int32 g^2 / d2][2N flags][2N G counts][2N G maxima]
// [2N H W uint8 border planes], each part aligned to 64 bytes
size_t surf_scratch_bytes(int N, int H, int W) {
    const int64_t hw = (int64_t)H * W, pg = 2 * (int64_t)N * surf_groups(hw);
    return (size_t)(align64(8 * pg) + align64(4 * 2 * N * hw) + align64(4 * 2 * (int64_t)N) +
                    2 * align64(4 * pg) + align64(2 * N * hw));
}

int k_surface_stats(const float* x, const float* t, int N, int C, int H, int W, void* scratch,
                    int64_t* out_i64, double* out_f64, hipStream_t s) {
    const int64_t hw = (int64_t)H * W;
    const int G = surf_groups(hw), planes = 2 * N;
    const int64_t pg = (int64_t)planes * G;
    char* p = (char*)scratch;
    double* psum = (double*)p;
    p += align64(8 * pg);
    int* d2 = (int*)p;
    p += align64(4 * planes * hw);
    int* flags = (int*)p;
    p += align64(4 * (int64_t)planes);
    int* pn = (int*)p;
    p += align64(4 * pg);
    int* pmax = (int*)p;
    p += align64(4 * pg);
    uint8_t* border = (uint8_t*)p;
    HIP_OK(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)planes, s));
    const int64_t px = (int64_t)N * hw;
    hipLaunchKernelGGL(surf_border_kernel, dim3((unsigned)((px + SURF_BLOCK - 1) / SURF_BLOCK)),
                       dim3(SURF_BLOCK), 0, s, x, t, N, C, H, W, border);
    HIP_OK(hipGetLastError());
    const int cols = planes * W;
    hipLaunchKernelGGL(surf_columns_kernel, dim3((cols + SURF_COL_BLOCK - 1) / SURF_COL_BLOCK),
                       dim3(SURF_COL_BLOCK), 0, s, border, planes, H, W, d2, flags);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(surf_rows_kernel, dim3(planes * H), dim3(SURF_BLOCK), sizeof(int) * (size_t)W, s,
                       border, d2, flags, N, H, W);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(surf_gather_kernel, dim3((unsigned)pg), dim3(SURF_BLOCK), 0, s, border, d2, flags,
                       N, hw, G, pn, pmax, psum);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(surf_select_kernel, dim3(N), dim3(SURF_SEL_BLOCK), 0, s, border, d2, flags, N, hw,
                       G, pn, pmax, psum, out_i64, out_f64);
    return (int)hipGetLastError();
}

// The same on the host, one sample at a time, through the same functions.  border holds 2 H W
// bytes, d2 2 H W ints.
void surface_stats_host(const float* x, const float* t, int N, int C, int H, int W, uint8_t* border,
                        int* d2, int64_t* out_i64, double* out_f64) {
    const int64_t hw = (int64_t)H * W;
    for (int n = 0; n < N; ++n) {
        const float* xs = x + n * C * hw;
        const float* ts = t + n * C * hw;
        int64_t* oi = out_i64 + 6 * (int64_t)n;
        double* of = out_f64 + 2 * (int64_t)n;
        for (int k = 0; k < 6; ++k) oi[k] = 0;
        of[0] = of[1] = 0.0;
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                border[(int64_t)i * W + j] =
                    surf_border([&](int a, int b) { return surf_pred(xs[(int64_t)a * W + b]); }, i, j, H, W);
                border[hw + (int64_t)i * W + j] =
                    surf_border([&](int a, int b) { return surf_target(ts[(int64_t)a * W + b]); }, i, j, H, W);
            }
        bool any[2] = {false, false};
        for (int q = 0; q < 2; ++q)
            for (int j = 0; j < W; ++j)
                any[q] = edt_column(border + q * hw + j, d2 + q * hw + j, H, W) || any[q];
        if (!any[0] || !any[1]) continue;  // undefined: the fields stay 0
        std::vector<int> row(W);
        for (int q = 0; q < 2; ++q)
            for (int i = 0; i < H; ++i) {
                int* g = d2 + q * hw + (int64_t)i * W;
                const uint8_t* pb = border + (1 - q) * hw + (int64_t)i * W;  // as the row kernel
                std::copy(g, g + W, row.begin());
                for (int j = 0; j < W; ++j)
                    if (pb[j]) g[j] = edt_row_min(row.data(), W, j);
            }
        SurfAcc a[2];
        for (int dir = 0; dir < 2; ++dir) {
            a[dir] = surf_acc_zero();
            for (int64_t i = 0; i < hw; ++i)
                if (border[dir * hw + i]) surf_acc_add(a[dir], d2[(1 - dir) * hw + i]);
        }
        const int mx = std::max(a[0].max_d2, a[1].max_d2);
        oi[0] = 1;
        oi[1] = a[0].n;
        oi[2] = a[1].n;
        oi[3] = mx;
        of[0] = a[0].sum;
        of[1] = a[1].sum;
        SurfSel sel[2] = {{0u, 0}, {0u, 0}};
        surf_ranks(a[0].n + a[1].n, sel[0].rank, sel[1].rank);
        for (int shift = surf_top_shift(mx); shift >= 0; shift -= SURF_DIGIT_BITS) {
            int hist[2][SURF_BINS] = {};
            for (int dir = 0; dir < 2; ++dir)
                for (int64_t i = 0; i < hw; ++i) {
                    if (!border[dir * hw + i]) continue;
                    const uint32_t key = (uint32_t)d2[(1 - dir) * hw + i];
                    for (int k = 0; k < 2; ++k)
                        if (surf_sel_match(sel[k], key, shift)) hist[k][surf_digit(key, shift)] += 1;
                }
            for (int k = 0; k < 2; ++k) surf_select_step(sel[k], hist[k], shift);
        }
        oi[4] = sel[0].prefix;
        oi[5] = sel[1].prefix;
    }
}
