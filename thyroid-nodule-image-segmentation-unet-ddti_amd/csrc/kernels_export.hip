// Predict-mode export (rules in export.h; replaces the plot of the reference's
// utils/trainer.py:262-299): the resize of a score plane back to its frame's resolution, the
// threshold fused into it, and the contour / tint overlay.
//
//   resize_f32_h_kernel       the horizontal pass over the rows of one plane: one thread per pixel
//                             of the float32 intermediate [h][ow], x fastest.
//   resize_f32_v_mask_kernel  the vertical pass fused with the threshold.  A thread owns four
//                             consecutive pixels of an output row: the taps of a row are wave-uniform
//                             table reads, the intermediate is read row by row (coalesced), and the
//                             mask leaves as one dword and the plane -- only when the caller wants
//                             it -- as one float4 where the row length and the pointers allow, as
//                             single elements elsewhere.  Without a vertical pass (V = false) it
//                             thresholds its input as it is.
//   overlay_kernel            one block of four waves per 64 x 16 tile.  The prediction mask (and the
//                             ground truth, GT = true) is staged with an R-pixel halo in LDS as
//                             bytes, zero outside the image: "background or outside" is then one
//                             test.  A wave reads 64 consecutive bytes of a tile row, 16 dwords, each
//                             broadcast to its four lanes: no bank conflict.  Every thread classifies
//                             four pixels (rows ty, ty + 4, ...), blends, and puts the three bytes
//                             into the tile's RGB rows in LDS, each row shifted by its global
//                             address's low two bits, so that the LDS dwords are the aligned global
//                             dwords: the block then stores whole dwords, bytes only for the partial
//                             dword at either end of a row.  The statistics are reduced over the
//                             wave, then one atomic per field and wave that saw a foreground pixel,
//                             into the zeroed int64 buffer: sums for the two counts, maxima of
//                             W - x, H - y, x + 1, y + 1 for the box (all positive, zero = empty; a
//                             minimum needs no second initial value this way), which
//                             overlay_stats_kernel turns into the inclusive box, -1 when empty.
#include "export.h"
#include "kernels_misc.h"

namespace {

constexpr int EXPORT_BLOCK = 256;
constexpr int OV_TW = 64, OV_TH = 16;                // tile
constexpr int OV_PITCH = OV_TW + 2 * EXPORT_MAX_WIDTH + 2;  // halo row, bytes (72)
constexpr int OV_ROWS = OV_TH + 2 * EXPORT_MAX_WIDTH;
constexpr int OV_RGB_DW = (3 * OV_TW + 3) / 4 + 1;   // dwords of a shifted RGB row (49) ...
constexpr int OV_RGB_PITCH = OV_RGB_DW + 1;          // ... and its pitch in dwords

__global__ __launch_bounds__(EXPORT_BLOCK) void resize_f32_h_kernel(const float* __restrict__ src, int h, int w,
                                                                    int ow, const double* __restrict__ kh,
                                                                    const int* __restrict__ bh, int ksh,
                                                                    float* __restrict__ dst) {
    const int64_t n = (int64_t)h * ow;
    for (int64_t i = blockIdx.x * (int64_t)EXPORT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * EXPORT_BLOCK) {
        const int y = (int)(i / ow), xx = (int)(i - (int64_t)y * ow);
        int first = bh[2 * xx], count = bh[2 * xx + 1];
        export_clamp_taps(w, ksh, first, count);
        dst[i] = export_resample(src + (int64_t)y * w + first, 1, kh + (int64_t)xx * ksh, count);
    }
}

template <bool V>
__global__ __launch_bounds__(EXPORT_BLOCK) void resize_f32_v_mask_kernel(const float* __restrict__ mid, int h, int oh,
                                                                         int ow, const double* __restrict__ kv,
                                                                         const int* __restrict__ bv, int ksv, int kind,
                                                                         float thr, float* __restrict__ plane,
                                                                         uint8_t* __restrict__ mask, int vec) {
    const int quads = (ow + 3) / 4;
    const int64_t n = (int64_t)oh * quads;
    for (int64_t i = blockIdx.x * (int64_t)EXPORT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * EXPORT_BLOCK) {
        const int yy = (int)(i / quads), x0 = 4 * (int)(i - (int64_t)yy * quads);
        int first = 0, count = 0;
        if (V) {
            first = bv[2 * yy], count = bv[2 * yy + 1];
            export_clamp_taps(h, ksv, first, count);
        }
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int xx = x0 + q;
            if (xx >= ow) continue;
            v[q] = V ? export_resample(mid + (int64_t)first * ow + xx, ow, kv + (int64_t)yy * ksv, count)
                     : mid[(int64_t)yy * ow + xx];
        }
        const int64_t o = (int64_t)yy * ow + x0;
        if (vec) {  // ow % 4 == 0 and aligned pointers: the quad is whole
            uchar4 m;
            m.x = export_fg(kind, v[0], thr), m.y = export_fg(kind, v[1], thr);
            m.z = export_fg(kind, v[2], thr), m.w = export_fg(kind, v[3], thr);
            *reinterpret_cast<uchar4*>(mask + o) = m;
            if (plane) *reinterpret_cast<float4*>(plane + o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (x0 + q < ow) {
                    mask[o + q] = export_fg(kind, v[q], thr) ? 1 : 0;
                    if (plane) plane[o + q] = v[q];
                }
        }
    }
}

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// halo tile of one mask: s[(ly + R) * OV_PITCH + lx + R] for ly in -R..OV_TH+R-1, lx in -R..OV_TW+R-1
template <int R>
__device__ __forceinline__ void ov_stage(const uint8_t* __restrict__ m, int H, int W, int ty0, int tx0,
                                         uint8_t* __restrict__ s) {
    constexpr int CW = OV_TW + 2 * R, CH = OV_TH + 2 * R;
    for (int k = threadIdx.x; k < CW * CH; k += EXPORT_BLOCK) {
        const int ly = k / CW, lx = k - ly * CW;
        const int y = ty0 + ly - R, x = tx0 + lx - R;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        s[ly * OV_PITCH + lx] = in && m[(int64_t)y * W + x] != 0 ? 1 : 0;
    }
}

// the class of tile pixel (ly, lx) of a staged mask
template <int R>
__device__ __forceinline__ int ov_class(const uint8_t* __restrict__ s, int ly, int lx) {
    const uint8_t* c = s + (ly + R) * OV_PITCH + lx + R;
    if (!*c) return EXPORT_BG;
    int all = 1;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
        const int rem = R - (dy < 0 ? -dy : dy);
#pragma unroll
        for (int dx = -rem; dx <= rem; ++dx) all &= c[dy * OV_PITCH + dx];
    }
    return all ? EXPORT_INTERIOR : EXPORT_CONTOUR;
}

template <int R, bool GT>
__global__ __launch_bounds__(EXPORT_BLOCK) void overlay_kernel(const uint8_t* __restrict__ gray,
                                                               const uint8_t* __restrict__ pred,
                                                               const uint8_t* __restrict__ gt, int H, int W, int alpha,
                                                               uint8_t* __restrict__ rgb,
                                                               unsigned long long* __restrict__ stats) {
    __shared__ uint8_t sp[OV_ROWS * OV_PITCH];
    __shared__ uint8_t sg[GT ? OV_ROWS * OV_PITCH : 4];
    __shared__ uint32_t srgb[OV_TH * OV_RGB_PITCH];
    const int tx0 = blockIdx.x * OV_TW, ty0 = blockIdx.y * OV_TH;
    ov_stage<R>(pred, H, W, ty0, tx0, sp);
    if (GT) ov_stage<R>(gt, H, W, ty0, tx0, sg);
    __syncthreads();
    const int lx = threadIdx.x & 63, x = tx0 + lx;
    long long area = 0, contour = 0;
    int ex0 = 0, ey0 = 0, ex1 = 0, ey1 = 0;  // maxima of W - x, H - y, x + 1, y + 1
    uint8_t* rgb8 = reinterpret_cast<uint8_t*>(srgb);
#pragma unroll
    for (int q = 0; q < OV_TH / 4; ++q) {
        const int ly = (threadIdx.x >> 6) + 4 * q, y = ty0 + ly;
        if (x >= W || y >= H) continue;
        const int pc = ov_class<R>(sp, ly, lx);
        const int gc = GT ? ov_class<R>(sg, ly, lx) : EXPORT_BG;
        if (pc != EXPORT_BG) {
            ++area;
            contour += pc == EXPORT_CONTOUR;
            ex0 = max(ex0, W - x), ey0 = max(ey0, H - y), ex1 = max(ex1, x + 1), ey1 = max(ey1, y + 1);
        }
        uint8_t r, g, b;
        export_pixel(gray[(int64_t)y * W + x], pc, gc, alpha, r, g, b);
        // the row's first byte lands at the low two bits of its global address
        const unsigned shift = (unsigned)((uintptr_t)(rgb + 3 * ((int64_t)y * W + tx0)) & 3);
        uint8_t* o = rgb8 + ly * (OV_RGB_PITCH * 4) + shift + 3 * lx;
        o[0] = r, o[1] = g, o[2] = b;
    }
    __syncthreads();
    const int cols = min(OV_TW, W - tx0), rows = min(OV_TH, H - ty0);
    for (int k = threadIdx.x; k < rows * OV_RGB_DW; k += EXPORT_BLOCK) {
        const int ly = k / OV_RGB_DW, j = k - ly * OV_RGB_DW;
        uint8_t* row = rgb + 3 * ((int64_t)(ty0 + ly) * W + tx0);  // first byte of the row's tile part
        const int shift = (int)((uintptr_t)row & 3);
        const int b0 = 4 * j - shift, b1 = b0 + 4, nb = 3 * cols;  // the dword's bytes, relative to row
        if (b0 >= nb) continue;
        const uint32_t v = srgb[ly * OV_RGB_PITCH + j];
        if (b0 >= 0 && b1 <= nb) {
            *reinterpret_cast<uint32_t*>(row + b0) = v;
        } else {
            for (int b = max(b0, 0); b < min(b1, nb); ++b) row[b] = (uint8_t)(v >> (8 * (b - b0)));
        }
    }
    // wave-uniform: every lane holds the wave's values after the reductions
    area = wave_sum(area);
    if (area == 0) return;
    contour = wave_sum(contour);
    ex0 = wave_max(ex0), ey0 = wave_max(ey0), ex1 = wave_max(ex1), ey1 = wave_max(ey1);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(stats + 0, (unsigned long long)area);
        if (contour) atomicAdd(stats + 1, (unsigned long long)contour);
        atomicMax(stats + 2, (unsigned long long)ex0);
        atomicMax(stats + 3, (unsigned long long)ey0);
        atomicMax(stats + 4, (unsigned long long)ex1);
        atomicMax(stats + 5, (unsigned long long)ey1);
    }
}

__global__ void overlay_stats_kernel(long long* __restrict__ stats, int H, int W) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool any = stats[0] != 0;
    stats[2] = any ? W - stats[2] : -1;
    stats[3] = any ? H - stats[3] : -1;
    stats[4] = stats[4] - 1;
    stats[5] = stats[5] - 1;
}

bool aligned_to(const void* p, size_t a) { return (uintptr_t)p % a == 0; }

int export_grid(int64_t items) {
    return (int)std::min<int64_t>((items + EXPORT_BLOCK - 1) / EXPORT_BLOCK, 8192);
}

template <int R>
void overlay_launch(const uint8_t* gray, const uint8_t* pred, const uint8_t* gt, int h, int w, int alpha, uint8_t* rgb,
                    unsigned long long* stats, hipStream_t s) {
    const dim3 grid((w + OV_TW - 1) / OV_TW, (h + OV_TH - 1) / OV_TH);
    if (gt)
        hipLaunchKernelGGL((overlay_kernel<R, true>), grid, dim3(EXPORT_BLOCK), 0, s, gray, pred, gt, h, w, alpha, rgb,
                           stats);
    else
        hipLaunchKernelGGL((overlay_kernel<R, false>), grid, dim3(EXPORT_BLOCK), 0, s, gray, pred, gt, h, w, alpha, rgb,
                           stats);
}

}  // namespace

// the float32 intermediate of the horizontal pass
size_t export_scratch_bytes(int h, int w, int ow) { return ow != w ? sizeof(float) * (size_t)h * (size_t)ow : 0; }

int k_resize_f32_mask(const float* src, int h, int w, int oh, int ow, const double* kh, const int* bh, int ksh,
                      const double* kv, const int* bv, int ksv, int kind, float thr, void* scratch, float* plane,
                      uint8_t* mask, hipStream_t s) {
    const bool need_h = ow != w, need_v = oh != h;
    const int vec = ow % 4 == 0 && aligned_to(mask, 4) && (!plane || aligned_to(plane, 16));
    const int vgrid = export_grid((int64_t)oh * ((ow + 3) / 4));
    if (need_h && !need_v) {
        // the horizontal pass alone forms the plane: into `plane` when wanted, else the scratch
        float* mid = plane ? plane : (float*)scratch;
        hipLaunchKernelGGL(resize_f32_h_kernel, dim3(export_grid((int64_t)h * ow)), dim3(EXPORT_BLOCK), 0, s, src, h, w,
                           ow, kh, bh, ksh, mid);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(resize_f32_v_mask_kernel<false>, dim3(vgrid), dim3(EXPORT_BLOCK), 0, s, mid, h, oh, ow, kv,
                           bv, ksv, kind, thr, (float*)nullptr, mask, ow % 4 == 0 && aligned_to(mask, 4));
        return (int)hipGetLastError();
    }
    const float* mid = src;
    if (need_h) {
        hipLaunchKernelGGL(resize_f32_h_kernel, dim3(export_grid((int64_t)h * ow)), dim3(EXPORT_BLOCK), 0, s, src, h, w,
                           ow, kh, bh, ksh, (float*)scratch);
        HIP_OK(hipGetLastError());
        mid = (const float*)scratch;
    }
    if (need_v)
        hipLaunchKernelGGL(resize_f32_v_mask_kernel<true>, dim3(vgrid), dim3(EXPORT_BLOCK), 0, s, mid, h, oh, ow, kv, bv,
                           ksv, kind, thr, plane, mask, vec);
    else
        hipLaunchKernelGGL(resize_f32_v_mask_kernel<false>, dim3(vgrid), dim3(EXPORT_BLOCK), 0, s, mid, h, oh, ow, kv, bv,
                           ksv, kind, thr, plane, mask, vec);
    return (int)hipGetLastError();
}

int k_overlay_u8(const uint8_t* gray, const uint8_t* pred, const uint8_t* gt, int h, int w, int r, int alpha,
                 uint8_t* rgb, int64_t* stats, hipStream_t s) {
    HIP_OK(hipMemsetAsync(stats, 0, sizeof(int64_t) * EXPORT_STAT_FIELDS, s));
    unsigned long long* st = (unsigned long long*)stats;
    if (r == 1) overlay_launch<1>(gray, pred, gt, h, w, alpha, rgb, st, s);
    else if (r == 2) overlay_launch<2>(gray, pred, gt, h, w, alpha, rgb, st, s);
    else overlay_launch<3>(gray, pred, gt, h, w, alpha, rgb, st, s);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(overlay_stats_kernel, dim3(1), dim3(64), 0, s, (long long*)stats, h, w);
    return (int)hipGetLastError();
}
