// The dz pass: the BatchNorm-backward value dz = [!mask || y > 0] (A do + B (y - mean) + C) of a
// conv's output, formed by one elementwise pass in front of its backward GEMMs.
// Sources of `do` (SRC): 0 stored [P][C], 1 DzHead (recomputed from the 1x1 head), 2 DzPool
// (recomputed from the max-pool backward's inputs).  Outputs, one kernel each:
//   f32 in place, stored do only                  bn_dz_rows_kernel    (kernels_misc.hip)
//   bf16 image, stored do also f32 in place       bn_dz16_kernel<SRC>  (kernels_misc.hip)
//   x3 image and the bias's column partials       bn_dz_x3_kernel<SRC> (kernels_gemm_x3.hip)
// The kernels own their thread mapping, rows in flight and stores; every expression that
// decides a bit lives here once: dz_pool_do (also maxpool_bwd_kernel's stored do), dz_head_do,
// dz_finish, and the row helpers dz_load / dz_form built from them.
#pragma once
#include "gemm_common.h"  // Pix, decode_fast

// the last conv's do = [relu: fma(y, sc, sh) > 0] dl[m] w[c]: the 1x1 head's backward with one
// output channel, so head_bwd need not store the full-resolution f32 do (option head_fuse)
struct DzHead {
    const float* dl = nullptr;  // d logits [P] (NCHW with one channel = pixel order)
    const float* w = nullptr;   // head weights [C]
    const float *sc = nullptr, *sh = nullptr;  // the last BN's forward affine
    int relu = 0;               // BN -> ReLU: mask by the activation
};
// an encoder block's second conv: do = [msc: fma(y, msc, msh) > 0] (dskip + [winner == window
// position] dp), the max-pool backward's sum, so maxpool_bwd need not store it (option pool_fuse)
struct DzPool {
    const float* dp = nullptr;     // d pooled [N][H/2][W/2][C]
    const uint8_t* idx = nullptr;  // winner index per pooled element
    const float* dskip = nullptr;  // the concat gradient's skip half (offset applied), row stride ldskip
    int ldskip = 0;
    const float *msc = nullptr, *msh = nullptr;  // BN -> ReLU mask affine, or null
    int H = 0, W = 0;              // full-resolution grid
    float rH = 0.f, rW = 0.f;      // 1 / H, 1 / W (k_bn_dz fills them)
};

struct DzArgs {
    const float* y = nullptr;  // the BN input, row stride ld, channel offset off
    int ld = 0, off = 0;
    int64_t P = 0;
    int C = 0;
    const float* coef = nullptr;  // [4][C]: A, B, C, mean
    int mask = 0;                 // ReLU -> BN order: dz masked by [y > 0]
    // the source of do, exactly one: stored [P][C], the head, or the pool (N H W = P < 2^24 for
    // the f32-reciprocal pixel decode)
    float* d = nullptr;
    DzHead head;
    DzPool pool;
    int N = 0;
    // the outputs: f32 in place over d (stored do only), and at most one image
    bool f32 = false;
    uint16_t* dz16 = nullptr;  // dense bf16 image [P][C], round to nearest even
    uint16_t* dz3 = nullptr;   // x3 image [P][C / 32][3][32]
    float* bpart = nullptr;    // x3: [x3_dz_blocks(P)][C] column sums of dz (the conv bias gradient)
};
// validates, then launches the f32 / bf16 kernel or hands the x3 outputs to k_bn_dz_x3
int k_bn_dz(const DzArgs& a, hipStream_t s);
int k_bn_dz_x3(const DzArgs& a, hipStream_t s);  // (kernels_gemm_x3.hip; a validated by k_bn_dz)

namespace {

// do of one element of the max-pool backward: `win` the winner byte, k the window position
__device__ __forceinline__ float dz_pool_do(float dskip, float dp, uint32_t win, int k, bool masked, float y,
                                            float msc, float msh) {
    float v = dskip;
    if (win == (uint32_t)k) v += dp;
    if (masked && !bn_relu_on(y, msc, msh)) v = 0.f;
    return v;
}
// do of one element of the 1x1 head's backward with one output channel
__device__ __forceinline__ float dz_head_do(float dl, float w, int relu, float y, float sc, float sh) {
    return !relu || bn_relu_on(y, sc, sh) ? dl * w : 0.f;
}
__device__ __forceinline__ f32x4 dz_finish(int mask, f32x4 a, f32x4 d, f32x4 b, f32x4 y, f32x4 mu, f32x4 c) {
    const f32x4 r = bn_dz4(a, d, b, y, mu, c);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (!mask || y[j] > 0.f) ? r[j] : 0.f;
    return o;
}

// Per-octet registers of a thread: the dz coefficients and the source's per-channel values (the
// pool's mask affine, the head's weights and affine; loaded per element inside the row loop, the
// fused pass ran 1.5x slower than the unfused pair).  Members a source does not use are never
// loaded and cost no register.
struct DzCoef {
    f32x4 a[2], b[2], c[2], mu[2];
};
__device__ __forceinline__ DzCoef dz_coef(const float* __restrict__ coef, int C, int c) {
    DzCoef k;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        k.a[h] = *(const f32x4*)(coef + c + 4 * h);
        k.b[h] = *(const f32x4*)(coef + C + c + 4 * h);
        k.c[h] = *(const f32x4*)(coef + 2 * C + c + 4 * h);
        k.mu[h] = *(const f32x4*)(coef + 3 * C + c + 4 * h);
    }
    return k;
}
struct DzSrcCoef {
    f32x4 sc[2], sh[2], w[2];
};
template <int SRC>  // 0: do from memory, 1: DzHead, 2: DzPool
__device__ __forceinline__ DzSrcCoef dz_src_coef(const DzHead& hd, const DzPool& pl, int c) {
    DzSrcCoef k;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if constexpr (SRC == 2) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            k.sc[h] = pl.msc ? *(const f32x4*)(pl.msc + c + 4 * h) : z;
            k.sh[h] = pl.msc ? *(const f32x4*)(pl.msh + c + 4 * h) : z;
        }
        if constexpr (SRC == 1) {
            k.w[h] = *(const f32x4*)(hd.w + c + 4 * h);
            k.sc[h] = *(const f32x4*)(hd.sc + c + 4 * h);
            k.sh[h] = *(const f32x4*)(hd.sh + c + 4 * h);
        }
    }
    return k;
}

// One row's 8 channels in registers.  dz_load only issues the loads, so a kernel can put all
// its rows in flight before dz_form's arithmetic.
struct DzRow {
    f32x4 d[2], y[2];  // do (DzPool: dskip) and the BN input
    f32x4 gp[2];       // DzPool: d pooled, the winner bytes and this pixel's window position
    uint32_t win[2];
    int k;
    float dl;          // DzHead: d logit
};
template <int SRC>
__device__ __forceinline__ void dz_load(DzRow& r, const float* __restrict__ d, const float* __restrict__ y,
                                        int ld, int off, int C, int64_t m, int c, const DzHead& hd,
                                        const DzPool& pl) {
    int64_t po = 0;
    if constexpr (SRC == 1) r.dl = hd.dl[m];
    if constexpr (SRC == 2) {
        const Pix q = decode_fast((int)m, pl.H, pl.W, pl.rH, pl.rW);
        po = ((int64_t)q.img * (pl.H >> 1) + (q.y >> 1)) * (pl.W >> 1) + (q.x >> 1);
        r.k = (q.y & 1) * 2 + (q.x & 1);
        const uint2 w2 = *(const uint2*)(pl.idx + po * C + c);
        r.win[0] = w2.x;
        r.win[1] = w2.y;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if constexpr (SRC == 2) {
            r.d[h] = *(const f32x4*)(pl.dskip + m * pl.ldskip + c + 4 * h);
            r.gp[h] = *(const f32x4*)(pl.dp + po * C + c + 4 * h);
        } else if constexpr (SRC == 0) {
            r.d[h] = *(const f32x4*)(d + m * C + c + 4 * h);
        }
        r.y[h] = *(const f32x4*)(y + m * ld + off + c + 4 * h);
    }
}
// the row's do from its source, then dz: o[h][j] = dz of channel c + 4 h + j
template <int SRC>
__device__ __forceinline__ void dz_form(const DzRow& r, const DzCoef& k, const DzSrcCoef& sk, int mask,
                                        const DzHead& hd, const DzPool& pl, f32x4 (&o)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x4 d = r.d[h];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (SRC == 2)
                d[j] = dz_pool_do(d[j], r.gp[h][j], (r.win[h] >> (8 * j)) & 0xFF, r.k, pl.msc != nullptr,
                                  r.y[h][j], sk.sc[h][j], sk.sh[h][j]);
            if constexpr (SRC == 1) d[j] = dz_head_do(r.dl, sk.w[h][j], hd.relu, r.y[h][j], sk.sc[h][j], sk.sh[h][j]);
        }
        o[h] = dz_finish(mask, k.a[h], d, k.b[h], r.y[h], k.mu[h], k.c[h]);
    }
}

}  // namespace
