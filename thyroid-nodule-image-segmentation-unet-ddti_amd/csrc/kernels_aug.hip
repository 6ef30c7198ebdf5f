// Device-side training augmentations of uint8 planes (aug.h: algorithms and exactness rules):
// flip + rotate + brightness (+ speckle) + TGC in one gather / point kernel, and CLAHE in three passes
// (tile histograms, one table per tile, per-pixel blend).  Host twins for the CPU tests.
#include <initializer_list>

#include "aug.h"
#include "kernels_misc.h"

namespace {

constexpr int AUG_BLOCK = 256;
constexpr int HIST_PIXELS = 2048;  // tile pixels per histogram block (8 per thread)

// One thread per output pixel, consecutive threads along x (coalesced stores; the loads are
// as coalesced as the rotation allows).  dst != src.  NOISE: the speckle step with noise[idx].
template <bool NOISE>
__global__ __launch_bounds__(AUG_BLOCK) void augment_kernel(const uint8_t* __restrict__ src, int h,
                                                           int w, uint8_t* __restrict__ dst,
                                                           const unet_aug_params p,
                                                           const double* __restrict__ noise) {
    __shared__ uint8_t lut[256];
    __shared__ float gain[AUG_MAX_BINS];
    lut[threadIdx.x] = p.lut[threadIdx.x];
    if (threadIdx.x < AUG_MAX_BINS) gain[threadIdx.x] = p.gain[threadIdx.x];
    __syncthreads();
    const int idx = blockIdx.x * AUG_BLOCK + threadIdx.x;
    if (idx >= h * w) return;
    const int y = idx / w, x = idx - y * w;
    const int s = aug_source(p, x, y, h, w);
    uint8_t v = lut[s < 0 ? 0 : src[s]];
    if (NOISE) v = aug_speckle(v, noise[idx]);
    const int band = aug_band(y, h, p.num_bins);
    if (band >= 0) v = aug_gain(v, gain[band]);
    dst[idx] = v;
}

// Block (chunk, tile): HIST_PIXELS pixels of one tile of the padded plane, counted in LDS and
// flushed into hist[tile][256] (zeroed by the launcher).
__global__ __launch_bounds__(AUG_BLOCK) void clahe_hist_kernel(const uint8_t* __restrict__ src,
                                                              const ClaheGeom G,
                                                              int* __restrict__ hist) {
    __shared__ int bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const int tile = blockIdx.y, tj = tile / G.gx, ti = tile - tj * G.gx;
    const int area = G.th * G.tw;
    const int p0 = blockIdx.x * HIST_PIXELS;
    const int p1 = min(area, p0 + HIST_PIXELS);
    for (int q = p0 + threadIdx.x; q < p1; q += AUG_BLOCK) {
        const int r = q / G.tw, c = q - r * G.tw;
        const int y = clahe_reflect(tj * G.th + r, G.h), x = clahe_reflect(ti * G.tw + c, G.w);
        atomicAdd(&bins[src[y * G.w + x]], 1);
    }
    __syncthreads();
    const int n = bins[threadIdx.x];
    if (n) atomicAdd(&hist[tile * 256 + threadIdx.x], n);
}

// One block per tile, thread k = bin k: clip, redistribute, inclusive scan, table entry.
__global__ __launch_bounds__(AUG_BLOCK) void clahe_lut_kernel(const int* __restrict__ hist,
                                                             const ClaheGeom G,
                                                             uint8_t* __restrict__ lut) {
    __shared__ int sh[2][256];
    const int k = threadIdx.x, tile = blockIdx.x;
    const int count = hist[tile * 256 + k];
    // clipped = sum_k max(count - limit, 0) (tree sum: integers, any order is exact)
    sh[0][k] = G.limit > 0 && count > G.limit ? count - G.limit : 0;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (k < d) sh[0][k] += sh[0][k + d];
        __syncthreads();
    }
    const int clipped = sh[0][0];
    __syncthreads();
    int cur = 0;
    sh[0][k] = clahe_bin(count, k, G.limit, clipped);
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan, double-buffered
        sh[cur ^ 1][k] = sh[cur][k] + (k >= d ? sh[cur][k - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    lut[tile * 256 + k] = clahe_lut_entry(sh[cur][k], G.lut_scale);
}

__global__ __launch_bounds__(AUG_BLOCK) void clahe_apply_kernel(const uint8_t* __restrict__ src,
                                                               const ClaheGeom G,
                                                               const uint8_t* __restrict__ lut,
                                                               uint8_t* __restrict__ dst) {
    const int idx = blockIdx.x * AUG_BLOCK + threadIdx.x;
    if (idx >= G.h * G.w) return;
    const int y = idx / G.w, x = idx - y * G.w;
    dst[idx] = clahe_pixel(G, lut, x, y, src[idx]);
}

}  // namespace

int aug_params_check(const unet_aug_params* p, int h, int w) {
    if (h < 1 || w < 1 || h > AUG_MAX_SIDE || w > AUG_MAX_SIDE) return UNET_ERR_SHAPE;
    if (p->mode < UNET_ROT_NONE || p->mode > UNET_ROT_270) return UNET_ERR_INVALID;
    if ((p->mode == UNET_ROT_90 || p->mode == UNET_ROT_270) && h != w) return UNET_ERR_SHAPE;
    if (p->num_bins < 0) return UNET_ERR_INVALID;
    if (p->num_bins > AUG_MAX_BINS) return UNET_ERR_UNSUPPORTED;
    if (p->mode == UNET_ROT_AFFINE) {
        // the bounds under which aug_source's int32 sums cannot overflow (aug.h)
        for (int k : {0, 1, 3, 4})
            if (p->a[k] > AUG_MAX_COEF || p->a[k] < -AUG_MAX_COEF) return UNET_ERR_INVALID;
        for (int k : {2, 5})
            if (p->a[k] > AUG_MAX_OFFSET || p->a[k] < -AUG_MAX_OFFSET) return UNET_ERR_INVALID;
    }
    return UNET_OK;
}

int k_augment_u8(const uint8_t* src, int h, int w, uint8_t* dst, const unet_aug_params& p,
                 hipStream_t s, const double* noise) {
    const dim3 grid((h * w + AUG_BLOCK - 1) / AUG_BLOCK);
    if (noise)
        hipLaunchKernelGGL(augment_kernel<true>, grid, dim3(AUG_BLOCK), 0, s, src, h, w, dst, p, noise);
    else
        hipLaunchKernelGGL(augment_kernel<false>, grid, dim3(AUG_BLOCK), 0, s, src, h, w, dst, p,
                           noise);
    return (int)hipGetLastError();
}

void augment_u8_host(const uint8_t* src, int h, int w, uint8_t* dst, const unet_aug_params& p,
                     const double* noise) {
    for (int y = 0; y < h; ++y) {
        const int band = aug_band(y, h, p.num_bins);
        for (int x = 0; x < w; ++x) {
            const int s = aug_source(p, x, y, h, w);
            uint8_t v = p.lut[s < 0 ? 0 : src[s]];
            if (noise) v = aug_speckle(v, noise[y * w + x]);
            if (band >= 0) v = aug_gain(v, p.gain[band]);
            dst[y * w + x] = v;
        }
    }
}

int clahe_geom(int h, int w, double clip, int gx, int gy, ClaheGeom& G) {
    if (h < 1 || w < 1 || h > AUG_MAX_SIDE || w > AUG_MAX_SIDE) return UNET_ERR_SHAPE;
    if (gx < 1 || gy < 1) return UNET_ERR_INVALID;
    if ((int64_t)gx * gy > CLAHE_MAX_TILES) return UNET_ERR_UNSUPPORTED;
    const int pad_w = w % gx ? gx - w % gx : 0, pad_h = h % gy ? gy - h % gy : 0;
    if (pad_w > w - 1 || pad_h > h - 1) return UNET_ERR_SHAPE;  // REFLECT_101 cannot reach that far
    G.h = h, G.w = w, G.gx = gx, G.gy = gy;
    G.tw = (w + pad_w) / gx, G.th = (h + pad_h) / gy;
    const int area = G.tw * G.th;
    G.limit = 0;
    if (clip > 0) {
        const double l = clip * (double)area / 256.0;  // Python's float arithmetic, then int()
        G.limit = l >= (double)area ? area : (int)l;   // a limit >= area never clips
        if (G.limit < 1) G.limit = 1;
    }
    G.lut_scale = (float)(255.0 / (double)area);
    G.inv_tw = 1.0f / (float)G.tw;
    G.inv_th = 1.0f / (float)G.th;
    return UNET_OK;
}

size_t clahe_scratch_bytes(const ClaheGeom& G) { return (size_t)G.gx * G.gy * 256 * (sizeof(int) + 1); }

int k_clahe_u8(const uint8_t* src, uint8_t* dst, const ClaheGeom& G, void* scratch, hipStream_t s) {
    const int tiles = G.gx * G.gy, area = G.tw * G.th;
    int* hist = (int*)scratch;
    uint8_t* lut = (uint8_t*)(hist + (size_t)tiles * 256);
    HIP_OK(hipMemsetAsync(hist, 0, sizeof(int) * (size_t)tiles * 256, s));
    hipLaunchKernelGGL(clahe_hist_kernel, dim3((area + HIST_PIXELS - 1) / HIST_PIXELS, tiles),
                       dim3(AUG_BLOCK), 0, s, src, G, hist);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(clahe_lut_kernel, dim3(tiles), dim3(AUG_BLOCK), 0, s, hist, G, lut);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(clahe_apply_kernel, dim3((G.h * G.w + AUG_BLOCK - 1) / AUG_BLOCK),
                       dim3(AUG_BLOCK), 0, s, src, G, lut, dst);
    return (int)hipGetLastError();
}

// hist: tiles * 256 ints, lut: tiles * 256 bytes (caller's)
void clahe_u8_host(const uint8_t* src, uint8_t* dst, const ClaheGeom& G, int* hist, uint8_t* lut) {
    const int tiles = G.gx * G.gy;
    for (int i = 0; i < tiles * 256; ++i) hist[i] = 0;
    for (int y = 0; y < G.gy * G.th; ++y)
        for (int x = 0; x < G.gx * G.tw; ++x)
            ++hist[((y / G.th) * G.gx + x / G.tw) * 256 +
                   src[clahe_reflect(y, G.h) * G.w + clahe_reflect(x, G.w)]];
    for (int t = 0; t < tiles; ++t) {
        const int* ht = hist + t * 256;
        int clipped = 0, cum = 0;
        for (int k = 0; k < 256; ++k)
            if (G.limit > 0 && ht[k] > G.limit) clipped += ht[k] - G.limit;
        for (int k = 0; k < 256; ++k) {
            cum += clahe_bin(ht[k], k, G.limit, clipped);
            lut[t * 256 + k] = clahe_lut_entry(cum, G.lut_scale);
        }
    }
    for (int y = 0; y < G.h; ++y)
        for (int x = 0; x < G.w; ++x) dst[y * G.w + x] = clahe_pixel(G, lut, x, y, src[y * G.w + x]);
}
