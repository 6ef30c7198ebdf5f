// Device-side ElasticDeform of a uint8 image / mask pair (elastic.h: algorithm and exactness
// rules): the row pass of the two Gaussian-blurred displacement fields, then, per output pixel,
// the column pass, the float32 map, the bilinear gather of the image and the nearest gather of the
// mask.  Host twin for the CPU tests.
#include "elastic.h"
#include "kernels_misc.h"

namespace {

constexpr int EL_BLOCK = 256;

// Block (segment, row, field): EL_BLOCK pixels of one row of rx (field 0) or ry (field 1).  The
// segment and its R-wide halos are staged in LDS as u = r * 2 - 1 (each draw is read once,
// coalesced; the halo indices reflect at the row's ends), then thread t sums its ksize taps.
// tmp: [2][h][w].
__global__ __launch_bounds__(EL_BLOCK) void elastic_rows_kernel(const double* __restrict__ rx,
                                                               const double* __restrict__ ry, int h,
                                                               int w, const unet_elastic_params p,
                                                               double* __restrict__ tmp) {
    __shared__ double u[EL_BLOCK + EL_MAX_KSIZE - 1];
    const int R = p.ksize / 2, x0 = blockIdx.x * EL_BLOCK, y = blockIdx.y, f = blockIdx.z;
    const double* __restrict__ row = (f ? ry : rx) + (size_t)y * w;
    const int n = min(EL_BLOCK, w - x0) + 2 * R;  // staged columns x0 - R .. x0 - R + n - 1
    for (int j = threadIdx.x; j < n; j += EL_BLOCK) u[j] = el_unit(row[el_reflect101(x0 - R + j, w)]);
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    double acc = 0.0;
    for (int i = 0; i < p.ksize; ++i) acc = el_tap(acc, p.k[i], u[threadIdx.x + i]);
    tmp[((size_t)f * h + y) * w + x] = acc;
}

// One thread per output pixel, consecutive threads along x: the column pass reads ksize rows of
// tmp at the thread's own x (coalesced), the stores are coalesced, the gathers go where the map
// points.  img / mask (with their destinations) may be null.
__global__ __launch_bounds__(EL_BLOCK) void elastic_remap_kernel(
    const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, int h, int w,
    uint8_t* __restrict__ img_dst, uint8_t* __restrict__ mask_dst, const double* __restrict__ tmp,
    const unet_elastic_params p) {
    const int idx = blockIdx.x * EL_BLOCK + threadIdx.x;
    if (idx >= h * w) return;
    const int y = idx / w, x = idx - y * w, R = p.ksize / 2;
    const double* __restrict__ ty = tmp + (size_t)h * w;
    double bx = 0.0, by = 0.0;
    for (int i = 0; i < p.ksize; ++i) {
        const size_t q = (size_t)el_reflect101(y - R + i, h) * w + x;
        bx = el_tap(bx, p.k[i], tmp[q]);
        by = el_tap(by, p.k[i], ty[q]);
    }
    const float mx = el_map(x, bx, p.alpha), my = el_map(y, by, p.alpha);
    if (img) img_dst[idx] = el_linear(img, h, w, mx, my);
    if (mask) mask_dst[idx] = el_nearest(mask, h, w, mx, my);
}

}  // namespace

int elastic_check(const unet_elastic_params* p, int h, int w) {
    if (p->ksize < 1 || p->ksize > EL_MAX_KSIZE || p->ksize % 2 == 0) return UNET_ERR_INVALID;
    if (!(p->alpha == p->alpha) || p->alpha - p->alpha != 0.0) return UNET_ERR_INVALID;  // finite
    const int R = p->ksize / 2;
    if (h <= R || w <= R || h > EL_MAX_SIDE || w > EL_MAX_SIDE) return UNET_ERR_SHAPE;
    return UNET_OK;
}

size_t elastic_scratch_bytes(int h, int w) { return sizeof(double) * 2 * (size_t)h * w; }

int k_elastic_u8(const uint8_t* img, const uint8_t* mask, int h, int w, uint8_t* img_dst,
                 uint8_t* mask_dst, const double* rx, const double* ry, const unet_elastic_params& p,
                 double* tmp, hipStream_t s) {
    hipLaunchKernelGGL(elastic_rows_kernel, dim3((w + EL_BLOCK - 1) / EL_BLOCK, h, 2), dim3(EL_BLOCK),
                       0, s, rx, ry, h, w, p, tmp);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(elastic_remap_kernel, dim3((h * w + EL_BLOCK - 1) / EL_BLOCK), dim3(EL_BLOCK),
                       0, s, img, mask, h, w, img_dst, mask_dst, tmp, p);
    return (int)hipGetLastError();
}

// tmp: 2 * h * w doubles (caller's)
void elastic_u8_host(const uint8_t* img, const uint8_t* mask, int h, int w, uint8_t* img_dst,
                     uint8_t* mask_dst, const double* rx, const double* ry,
                     const unet_elastic_params& p, double* tmp) {
    const int R = p.ksize / 2;
    for (int f = 0; f < 2; ++f)
        for (int y = 0; y < h; ++y) {
            const double* row = (f ? ry : rx) + (size_t)y * w;
            for (int x = 0; x < w; ++x) {
                double acc = 0.0;
                for (int i = 0; i < p.ksize; ++i)
                    acc = el_tap(acc, p.k[i], el_unit(row[el_reflect101(x - R + i, w)]));
                tmp[((size_t)f * h + y) * w + x] = acc;
            }
        }
    const double* ty = tmp + (size_t)h * w;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            double bx = 0.0, by = 0.0;
            for (int i = 0; i < p.ksize; ++i) {
                const size_t q = (size_t)el_reflect101(y - R + i, h) * w + x;
                bx = el_tap(bx, p.k[i], tmp[q]);
                by = el_tap(by, p.k[i], ty[q]);
            }
            const float mx = el_map(x, bx, p.alpha), my = el_map(y, by, p.alpha);
            if (img) img_dst[y * w + x] = el_linear(img, h, w, mx, my);
            if (mask) mask_dst[y * w + x] = el_nearest(mask, h, w, mx, my);
        }
}
