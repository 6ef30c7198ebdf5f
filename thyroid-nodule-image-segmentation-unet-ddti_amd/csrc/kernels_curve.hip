// Threshold sweep (rules in curve.h): the class-split histogram of the logits and the per-plane
// statistics read off it.
//
//   curve_hist_kernel   a streaming pass, 8 bytes read per pixel.  A block of four waves owns one
//                       chunk of CURVE_CHUNK pixels of ONE plane at a time (the (plane, chunk)
//                       items are walked with a grid stride; a block never spans two planes within
//                       an item and waits on no other block).  The edges live in LDS; a pixel's bin
//                       is curve_bin's branch-free log2(B)-step search there.  Every wave adds into
//                       its own [2][B] sub-histogram in LDS, and the block flushes the non-zero sums
//                       of the four once per item to plane_hist with integer atomics (exact, so the
//                       result does not depend on the order).
//                       A segmentation batch is the worst case for a histogram: more than 90 % of
//                       the pixels are confident background and share one or two bins, and 64 lanes
//                       adding to one LDS word serialise.  So each add is aggregated over the wave
//                       first (curve_wave_add).
//                       VEC: float4 loads, when both pointers are 16-byte aligned and hw % 4 == 0
//                       (every plane then starts aligned); one float per lane and step otherwise.
//   curve_total_kernel  total[j] += the sum over the planes of plane_hist[.][j], one thread per j:
//                       no block of the histogram pass touches the 2 B words all of them would
//                       share.  (The ignored pixels go to total[2 B] from the histogram pass, one
//                       64-bit atomic per item that has any.)
//   curve_stats_kernel  one block per plane: thread 0 forms the suffix sums and auc2 in LDS
//                       (curve_suffix), the block the B + 1 dice_k in parallel, thread 0 picks
//                       best_k; the dice_k go to the context's scratch.
//   curve_dice_sum_kernel  dice_sum[k] += dice_k of plane 0, 1, ... in this order, one thread per k:
//                       the fixed order of the host twin, so both agree bit for bit.
#include "curve.h"
#include "kernels_misc.h"

namespace {

constexpr int CURVE_BLOCK = 256;
constexpr int CURVE_WAVES = CURVE_BLOCK / 64;
constexpr int CURVE_CHUNK = 8192;  // pixels of an item: 8 float4 steps of the block
constexpr int CURVE_MAX_GRID = 4096;

// One aggregated add of the wave: every lane brings a key (-1: nothing to add).  The lanes that
// share the first active lane's key are counted with one ballot and added once; whoever is left
// adds for itself.  With 95 % of the pixels in one bin the first lane almost always holds that
// bin, so an add of the wave is one LDS add of the popcount plus a few stragglers; when it does
// not, the stragglers are the dominant bin's lanes and serialise as they would have without the
// peel.  All 64 lanes of the wave must call this together.  (Measured against one LDS atomic per lane
// and against peeling until no lane is left, profiles/curve_time.txt: the first takes 1.3x the time
// on the skewed case, the second 5x on uniform bins.)
__device__ __forceinline__ void curve_wave_add(unsigned* __restrict__ h, int key) {
    const unsigned long long active = __ballot(key >= 0);
    if (active == 0) return;  // wave-uniform
    const int leader = __ffsll((long long)active) - 1;
    const int k0 = __shfl(key, leader);
    const unsigned long long same = __ballot(key == k0);
    const int lane = threadIdx.x & 63;
    if (lane == leader) atomicAdd(&h[k0], (unsigned)__popcll(same));
    else if (key >= 0 && key != k0) atomicAdd(&h[key], 1u);
}

template <bool VEC>
__global__ __launch_bounds__(CURVE_BLOCK) void curve_hist_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ t, int planes,
                                                                 int64_t hw, const float* __restrict__ edges,
                                                                 int B, int chunks, int* __restrict__ plane_hist,
                                                                 unsigned long long* __restrict__ total) {
    extern __shared__ unsigned curve_lds[];  // [B] edges (B - 1 used), then [CURVE_WAVES][2 B] counts
    float* e = reinterpret_cast<float*>(curve_lds);
    unsigned* hist = curve_lds + B;
    unsigned* h = hist + (threadIdx.x >> 6) * 2 * B;
    __shared__ unsigned ignored_s;
    for (int j = threadIdx.x; j < B - 1; j += CURVE_BLOCK) e[j] = edges[j];
    const int64_t items = (int64_t)planes * chunks;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t p = w / chunks;
        const int64_t begin = (w - p * chunks) * CURVE_CHUNK;
        const int64_t end = begin + CURVE_CHUNK < hw ? begin + CURVE_CHUNK : hw;
        for (int j = threadIdx.x; j < CURVE_WAVES * 2 * B; j += CURVE_BLOCK) hist[j] = 0;
        if (threadIdx.x == 0) ignored_s = 0;
        __syncthreads();
        const float* xp = x + p * hw;
        const float* tp = t + p * hw;
        unsigned ignored = 0;
        if (VEC) {
            // the trip count is the block's, so that every lane of a wave reaches curve_wave_add
            for (int64_t i0 = begin; i0 < end; i0 += CURVE_BLOCK * 4) {
                const int64_t i = i0 + threadIdx.x * 4;
                const bool in = i < end;  // hw % 4 == 0: a float4 is inside or outside as a whole
                float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), tv = xv;
                if (in) {
                    xv = *reinterpret_cast<const float4*>(xp + i);
                    tv = *reinterpret_cast<const float4*>(tp + i);
                }
                const int k0 = curve_key(e, B, xv.x, tv.x), k1 = curve_key(e, B, xv.y, tv.y);
                const int k2 = curve_key(e, B, xv.z, tv.z), k3 = curve_key(e, B, xv.w, tv.w);
                ignored += in ? (k0 < 0) + (k1 < 0) + (k2 < 0) + (k3 < 0) : 0;
                curve_wave_add(h, in ? k0 : -1);
                curve_wave_add(h, in ? k1 : -1);
                curve_wave_add(h, in ? k2 : -1);
                curve_wave_add(h, in ? k3 : -1);
            }
        } else {
            for (int64_t i0 = begin; i0 < end; i0 += CURVE_BLOCK) {
                const int64_t i = i0 + threadIdx.x;
                const bool in = i < end;
                const int k = in ? curve_key(e, B, xp[i], tp[i]) : 0;
                ignored += in && k < 0;
                curve_wave_add(h, in ? k : -1);
            }
        }
        if (ignored) atomicAdd(&ignored_s, ignored);
        __syncthreads();
        int* out = plane_hist + p * 2 * B;
        for (int j = threadIdx.x; j < 2 * B; j += CURVE_BLOCK) {
            unsigned s = 0;
#pragma unroll
            for (int v = 0; v < CURVE_WAVES; ++v) s += hist[v * 2 * B + j];
            if (s) atomicAdd(&out[j], (int)s);
        }
        if (threadIdx.x == 0 && ignored_s) atomicAdd(&total[2 * B], (unsigned long long)ignored_s);
        __syncthreads();
    }
}

__global__ __launch_bounds__(CURVE_BLOCK) void curve_total_kernel(const int* __restrict__ plane_hist, int planes,
                                                                  int B, int64_t* __restrict__ total) {
    const int j = blockIdx.x * CURVE_BLOCK + threadIdx.x;
    if (j >= 2 * B) return;
    int64_t s = 0;
    for (int64_t p = 0; p < planes; ++p) s += plane_hist[p * 2 * B + j];
    total[j] += s;
}

__global__ __launch_bounds__(CURVE_BLOCK) void curve_stats_kernel(const int* __restrict__ plane_hist, int planes,
                                                                  int B, int64_t* __restrict__ out_i64,
                                                                  double* __restrict__ dice_all) {
    __shared__ int32_t h[2 * CURVE_MAX_BINS];
    __shared__ int32_t tp[CURVE_MAX_BINS + 1], fp[CURVE_MAX_BINS + 1];
    __shared__ double dice[CURVE_MAX_BINS + 1];
    __shared__ CurveSums sums;
    for (int64_t p = blockIdx.x; p < planes; p += gridDim.x) {
        for (int j = threadIdx.x; j < 2 * B; j += CURVE_BLOCK) h[j] = plane_hist[p * 2 * B + j];
        __syncthreads();
        if (threadIdx.x == 0) sums = curve_suffix(h, h + B, B, tp, fp);
        __syncthreads();
        for (int k = threadIdx.x; k <= B; k += CURVE_BLOCK) {
            const double d = curve_dice(tp[k], fp[k], sums.P);
            dice[k] = d;
            dice_all[p * (B + 1) + k] = d;
        }
        __syncthreads();
        if (threadIdx.x == 0) curve_stat_row(sums, tp, fp, curve_best(dice, B), out_i64 + p * CURVE_STAT_FIELDS);
        __syncthreads();
    }
}

__global__ __launch_bounds__(CURVE_BLOCK) void curve_dice_sum_kernel(const double* __restrict__ dice_all, int planes,
                                                                     int B, double* __restrict__ dice_sum) {
    const int k = blockIdx.x * CURVE_BLOCK + threadIdx.x;
    if (k > B) return;
    double s = dice_sum[k];
    for (int64_t p = 0; p < planes; ++p) s += dice_all[p * (B + 1) + k];
    dice_sum[k] = s;
}

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

size_t curve_scratch_bytes(int planes, int B) { return sizeof(double) * (size_t)planes * (size_t)(B + 1); }

int k_curve_hist(const float* x, const float* t, int planes, int64_t hw, const float* edges, int B, int32_t* plane_hist,
                 int64_t* total, hipStream_t s) {
    HIP_OK(hipMemsetAsync(plane_hist, 0, sizeof(int32_t) * 2 * (size_t)B * (size_t)planes, s));
    const int chunks = (int)((hw + CURVE_CHUNK - 1) / CURVE_CHUNK);  // hw < 2^31
    const int64_t items = (int64_t)planes * chunks;
    const unsigned grid = (unsigned)std::min<int64_t>(items, CURVE_MAX_GRID);
    const size_t lds = sizeof(unsigned) * (size_t)(B + CURVE_WAVES * 2 * B);
    if (hw % 4 == 0 && aligned16(x) && aligned16(t))
        hipLaunchKernelGGL(curve_hist_kernel<true>, dim3(grid), dim3(CURVE_BLOCK), lds, s, x, t, planes, hw, edges, B,
                           chunks, plane_hist, (unsigned long long*)total);
    else
        hipLaunchKernelGGL(curve_hist_kernel<false>, dim3(grid), dim3(CURVE_BLOCK), lds, s, x, t, planes, hw, edges, B,
                           chunks, plane_hist, (unsigned long long*)total);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(curve_total_kernel, dim3((2 * B + CURVE_BLOCK - 1) / CURVE_BLOCK), dim3(CURVE_BLOCK), 0, s,
                       plane_hist, planes, B, total);
    return (int)hipGetLastError();
}

int k_curve_stats(const int32_t* plane_hist, int planes, int B, void* scratch, int64_t* out_i64, double* dice_sum,
                  hipStream_t s) {
    double* dice_all = (double*)scratch;
    hipLaunchKernelGGL(curve_stats_kernel, dim3((unsigned)std::min(planes, CURVE_MAX_GRID)), dim3(CURVE_BLOCK), 0, s,
                       plane_hist, planes, B, out_i64, dice_all);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(curve_dice_sum_kernel, dim3((B + 1 + CURVE_BLOCK - 1) / CURVE_BLOCK), dim3(CURVE_BLOCK), 0, s,
                       dice_all, planes, B, dice_sum);
    return (int)hipGetLastError();
}
