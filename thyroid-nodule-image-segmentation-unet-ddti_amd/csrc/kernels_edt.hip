// BoundaryLoss on the device (reference models/loss.py:48-66): the exact Euclidean distance
// transform of the targets (edt.h: algorithm, site rule, empty-mask rule, size limit) and the
// loss / dlogits kernels over it.
#include "edt.h"
#include "kernels_misc.h"

namespace {

constexpr int EDT_COL_BLOCK = 64;   // one wave: N * W column threads spread over many CUs
constexpr int EDT_ROW_BLOCK = 256;  // threads loop when W exceeds it

// Column pass: one thread per (sample, column), coalesced across columns.  flags[n] (zeroed by
// the launcher) becomes 1 when sample n holds any site.
__global__ __launch_bounds__(EDT_COL_BLOCK) void edt_columns_kernel(const float* __restrict__ t,
                                                                   int N, int C, int H, int W,
                                                                   int* __restrict__ g2,
                                                                   int* __restrict__ flags) {
    const int idx = blockIdx.x * EDT_COL_BLOCK + threadIdx.x;
    if (idx >= N * W) return;
    const int n = idx / W, j = idx - n * W;
    const int64_t hw = (int64_t)H * W;
    const bool any = edt_column(t + n * C * hw + j, g2 + n * hw + j, H, W);
    if (any) atomicOr(&flags[n], 1);
}

// Row pass: one block per (sample, row), the row of g^2 in LDS.
__global__ __launch_bounds__(EDT_ROW_BLOCK) void edt_rows_kernel(const int* __restrict__ g2,
                                                                const int* __restrict__ flags,
                                                                int H, int W,
                                                                float* __restrict__ dist) {
    extern __shared__ int row[];
    const int n = blockIdx.x / H, i = blockIdx.x - n * H;
    const int64_t base = ((int64_t)n * H + i) * W;
    if (flags[n] == 0) {  // block-uniform: the empty-mask rule
        for (int j = threadIdx.x; j < W; j += EDT_ROW_BLOCK) dist[base + j] = edt_empty(i, j);
        return;
    }
    for (int j = threadIdx.x; j < W; j += EDT_ROW_BLOCK) row[j] = g2[base + j];
    __syncthreads();
    for (int j = threadIdx.x; j < W; j += EDT_ROW_BLOCK)
        dist[base + j] = edt_sqrt(edt_row_min(row, W, j));
}

__device__ __forceinline__ float sigmoid_(float x) { return 1.f / (1.f + expf(-x)); }

// sum over one contiguous chunk of sample n's channel 0 of |sigmoid(x) - t| * dist -> part[n][g]
// (G = loss_groups(H W) chunks per sample, a function of the sample size only, as loss_stats)
__global__ __launch_bounds__(256) void boundary_stats_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ t,
                                                            const float* __restrict__ dist,
                                                            int64_t hw, int C, int G,
                                                            float* __restrict__ part) {
    __shared__ float red[4];
    const int n = blockIdx.x / G, g = blockIdx.x - n * G;
    const int64_t chunk = (hw + G - 1) / G;
    const int64_t i0 = g * chunk, i1 = min(hw, i0 + chunk);
    const float* xs = x + n * C * hw;
    const float* ts = t + n * C * hw;
    const float* ds = dist + n * hw;
    float a = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x)
        a += fabsf(sigmoid_(xs[i]) - ts[i]) * ds[i];
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// sum = sum_n (sample n's chunks added in order) / (H W), in double and in a fixed order;
// loss = sum / N (models/loss.py:65-66)
__global__ __launch_bounds__(256) void boundary_sum_kernel(const float* __restrict__ part, int G,
                                                          int N, int64_t hw,
                                                          double* __restrict__ sum,
                                                          float* __restrict__ loss) {
    __shared__ double acc[256];
    double a = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        float v = 0.f;
        for (int g = 0; g < G; ++g) v += part[(int64_t)n * G + g];
        a += (double)v / (double)hw;
    }
    acc[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < 256; ++k) s += acc[k];
    sum[0] = s;
    loss[0] = (float)(s / N);
}

// dlogits[n, 0] = w sign(p - t) dist p (1 - p) / (N H W), sign(0) = 0 (torch's abs backward);
// channels 1.. are zero (the loss reads channel 0 only)
__global__ void boundary_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                    const float* __restrict__ dist, int64_t hw, int C, int N,
                                    const float* __restrict__ w, float* __restrict__ dx) {
    const int64_t per = C * hw, total = per * N;
    const float scale = w[0] / (float)((double)N * (double)hw);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / per, r = i - n * per;
        float g = 0.f;
        if (r < hw) {
            const float pv = sigmoid_(x[i]), df = pv - t[i];
            const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
            g = scale * sg * dist[n * hw + r] * (pv * (1.f - pv));
        }
        dx[i] = g;
    }
}

}  // namespace

// scratch: [N any-site flags, padded to 64 ints][N H W ints of g^2]
int64_t edt_scratch_ints(int N, int H, int W) { return 64 * (((int64_t)N + 63) / 64) + (int64_t)N * H * W; }

int k_edt(const float* t, int N, int C, int H, int W, int* scratch, float* dist, hipStream_t s) {
    int* flags = scratch;
    int* g2 = scratch + 64 * (((int64_t)N + 63) / 64);
    HIP_OK(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)N, s));
    const int cols = N * W;
    hipLaunchKernelGGL(edt_columns_kernel, dim3((cols + EDT_COL_BLOCK - 1) / EDT_COL_BLOCK),
                       dim3(EDT_COL_BLOCK), 0, s, t, N, C, H, W, g2, flags);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(edt_rows_kernel, dim3(N * H), dim3(EDT_ROW_BLOCK), sizeof(int) * (size_t)W, s,
                       g2, flags, H, W, dist);
    return (int)hipGetLastError();
}

void edt_host(const float* t, int N, int C, int H, int W, int* g2, float* dist) {
    const int64_t hw = (int64_t)H * W;
    for (int n = 0; n < N; ++n) {
        const float* tn = t + n * C * hw;
        int* gn = g2 + n * hw;
        float* dn = dist + n * hw;
        bool any = false;
        for (int j = 0; j < W; ++j) any = edt_column(tn + j, gn + j, H, W) || any;
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j)
                dn[(int64_t)i * W + j] = any ? edt_sqrt(edt_row_min(gn + (int64_t)i * W, W, j)) : edt_empty(i, j);
    }
}

int k_boundary_fwd(const float* x, const float* t, const float* dist, int N, int C, int64_t hw,
                   float* part, double* sum, float* loss, hipStream_t s) {
    const int G = loss_groups(hw);
    hipLaunchKernelGGL(boundary_stats_kernel, dim3(N * G), dim3(256), 0, s, x, t, dist, hw, C, G, part);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(boundary_sum_kernel, dim3(1), dim3(256), 0, s, part, G, N, hw, sum, loss);
    return (int)hipGetLastError();
}

int k_boundary_bwd(const float* x, const float* t, const float* dist, int N, int C, int64_t hw,
                   const float* w, float* dx, hipStream_t s) {
    const int64_t total = (int64_t)N * C * hw;
    const int grid = (int)std::min<int64_t>(8192, std::max<int64_t>(1, (total + 255) / 256));
    hipLaunchKernelGGL(boundary_bwd_kernel, dim3(grid), dim3(256), 0, s, x, t, dist, hw, C, N, w, dx);
    return (int)hipGetLastError();
}
