// Host launchers of kernels_misc.hip (internal).
#pragma once
#include "../../include/unet_hip.h"
#include "common.h"

// Weight images of the row GEMMs, every 3x3 conv (kind 0) and ConvTranspose (kind 1) of the
// network in one launch.  Offsets w (params), f / d (forward / dgrad images; d < 0: none)
// count floats; bf16 images (round to nearest even) are addressed at the same float offsets.
// A job covers tx x ty 32x32 tiles (conv3: x over cin, y over cout; ConvT: x over cout, y
// over cin) starting at block block0.
struct PackJob {
    int64_t w, f, d;
    int cin, cout, kind, tx, ty, block0;
};
constexpr int MAX_PACK_JOBS = 48;
struct PackJobs {
    int n;
    PackJob j[MAX_PACK_JOBS];
};
int k_pack_all(const PackJobs& jobs, const float* prm, float* pack, int bf16, hipStream_t s);
// (r06) AdamW fused into the weight repack (unet_adamw_repack): the pack jobs' weight tensors
// are updated in place and packed from the updated values; `rest` lists the other arena ranges
// (elementwise AdamW).  Bit-identical to k_adamw over the whole arena followed by k_pack_all.
constexpr int MAX_ADAM_RANGES = 120;
struct AdamRanges {
    int n;
    int64_t off[MAX_ADAM_RANGES];      // arena offset of range k
    int64_t cum[MAX_ADAM_RANGES + 1];  // elements before range k (cum[n] = total)
};
struct AdamwScalars;
int k_pack_adamw(const PackJobs& jobs, const AdamRanges& rest, float* p, const float* g, float* m, float* v,
                 const AdamwScalars& a, float* pack, int bf16, hipStream_t s);
// conv_first: relu = ReLU after (+bias) (model.py order); b may be null (mod.py, bias-free).
// wgrad: mask = dz masked by [y > 0] (ReLU before the BN, model.py order); gb may be null.
int k_conv_first_fwd(const float* x, const float* w, const float* b, float* y, int P, int H, int W,
                     int C, int relu, float* partial, int G, hipStream_t s);
int k_conv_first_wgrad(const float* x, const float* dout, const float* y, const float* coef, int P,
                       int H, int W, int C, int mask, float* partial, int G, float* gw, float* gb,
                       hipStream_t s);
int k_reduce_rows(const float* in, int R, int ncols, float* out, int G, hipStream_t s);
int k_bn_finalize_train(const float* part, int G, int C, double count, const float* gamma,
                        const float* beta, float* rmean, float* rvar, int64_t* nbt, float momentum,
                        float eps, float* scale, float* shift, float* mean, float* invstd,
                        hipStream_t s);
int k_bn_finalize_eval(int C, const float* gamma, const float* beta, const float* rmean,
                       const float* rvar, float eps, float* scale, float* shift, hipStream_t s);
// relu / mscale+mshift: BN -> ReLU order (mod.py:46-47), see the kernels.
// (r06) pool16: the pooled values as the next conv's bf16 image [pooled pixels][C]; skip16 / skip3:
// op(BN(y)) at full resolution as bf16 / x3 into the decoder conv's kept image (ldk channels per
// pixel, channel offset so) -- what k_to_bf16 / k_to_x3 would write there
int k_maxpool_bn(const float* y, int ld, int off, const float* scale, const float* shift, int relu,
                 int N, int H, int W, int C, float* out, uint8_t* idx, hipStream_t s,
                 uint16_t* out3 = nullptr, uint16_t* pool16 = nullptr, uint16_t* skip16 = nullptr,
                 uint16_t* skip3 = nullptr, int ldk = 0, int so = 0);
int k_maxpool_bwd(const float* dp, const uint8_t* idx, const float* dskip, int ldskip, int offskip,
                  const float* y, int ldy, int offy, const float* mscale, const float* mshift,
                  int N, int H, int W, int C, float* dout, float* partial, int G, hipStream_t s);
int k_bn_bwd_finalize2(const float* part, int G, int C, double count, const float* gamma,
                       const float* mean, const float* invstd, float* coef, float* dgamma,
                       float* dbeta, hipStream_t s);
// (the dz pass between them: k_bn_dz, dz_pass.h)
// bf16 image [P][dld] (dld 0 = C: dense) of op(src), channels [0, C), for the LDS-DMA GEMMs
// (affine if scale, ReLU on c < relu)
int k_to_bf16(const float* src, int ld, int off, int C, const float* scale, const float* shift,
              int relu, int64_t P, uint16_t* dst, hipStream_t s, int dld = 0);
int k_bias_reduce(const float* slab, int S, int taps, int C, float* out, hipStream_t s);
// ConvT bias partials [splits][4][C] from the up half of the concat gradient (LDS-DMA wgrad)
int k_up2_bias_partials(const float* d, int ld, int off, int H, int W, int64_t P, int C, int pps,
                        int splits, float* bslab, hipStream_t s);
int k_sum_partials(const float* part, int G, int ncols, float* out, hipStream_t s);
int k_slab_reduce(const float* slab, int S, int Mw, int Nw, int kind, int cin, int cout,
                  float* grad, hipStream_t s);
int k_head_fwd(const float* y, int C, const float* scale, const float* shift, int relu,
               const float* w, const float* b, int O, int P, int HW, float* logits, hipStream_t s);
int k_head_bwd(const float* y, int C, const float* scale, const float* shift, int relu,
               const float* w, int O, int P, int HW, const float* dlog, float* dout, float* partial,
               float* bnpart, int G, hipStream_t s);
int k_pack_1x1_t(const float* w, float* wt, int cin, int cout, hipStream_t s);
// bf16 math: the 1x1 skip weight's bf16 images (RNE), plain Wf[co][ci] and transposed Wt[ci][co]
int k_pack_1x1_bf16(const float* w, uint16_t* wf, uint16_t* wt, int cin, int cout, hipStream_t s);
// Residual blocks (models/mod.py:ResUNet): first-block forward with the Cin = 1 skip,
// backward entry (ReLU mask + BN2 partials), first-block skip weight gradient.
int k_res_first_fwd(const float* x, const float* ws, const float* z, const float* sc,
                    const float* sh, int64_t P, int C, float* out, int ldo, int offo, hipStream_t s);
// (d16: also the dense bf16 image of du, the operand of the skip's bf16 dgrad / wgrad)
int k_res_bwd_prep(float* d, const float* out, int ldo, int offo, const float* z, int64_t P, int C,
                   float* partial, int G, hipStream_t s, uint16_t* d16 = nullptr);
int k_res_first_wgrad(const float* x, const float* du, int P, int C, float* partial, int G,
                      float* gw, hipStream_t s);
// Pillow-exact 8-bit bilinear resize + scale (input pipeline, utils/transforms.py:143-156)
int k_resize_u8(const uint8_t* src, int H, int W, float* dst, int OH, int OW, const int* kh,
                const int* bh, int ksh, const int* kv, const int* bv, int ksv, int need_h,
                int need_v, float divisor, hipStream_t s);
// Channel padding (runtime.hip, unet_ctx::padded): one tensor of the caller's torch-layout
// arena (roff) and of the padded arena (poff).  Dim k holds nseg[k] segments of seg[k] real
// entries, each padded to pseg[k] entries (unused dims: 1, 1, 1).
struct PadDesc {
    int64_t roff, poff, rnumel, pnumel;
    int32_t seg[4], pseg[4], nseg[4];
};
// expand = 1: dst (padded) <- src (torch layout), zeros in the padding;
// expand = 0: dst (torch layout) <- src (padded).  table: device copy of n descriptors.
int k_pad_copy(const PadDesc* table, int n, int64_t max_numel, const float* src, float* dst,
               int expand, hipStream_t s);
// Losses: per-sample stats fp32[4N] + batch sums fp64[8] (see kernels_misc.hip)
// (r06) chunks per sample of loss_stats_kernel; part holds 4 * N * loss_groups(per) floats
int loss_groups(int64_t per);
int k_loss_stats(const float* x, const float* t, int N, int64_t per, float* stats, double* sums,
                 float* part, hipStream_t s);
int k_loss_finalize(const double* sums, float alpha, float beta, float gamma, float* losses,
                    hipStream_t s);
int k_loss_bwd(const float* x, const float* t, int N, int64_t per, const float* stats,
               const double* sums, const float* w, float alpha, float beta, float gamma, float* dx,
               hipStream_t s);
// BoundaryLoss (kernels_edt.hip; algorithm and rules in edt.h).  scratch holds
// edt_scratch_ints(N, H, W) ints; part holds N * loss_groups(hw) floats, hw = H * W
int64_t edt_scratch_ints(int N, int H, int W);
int k_edt(const float* t, int N, int C, int H, int W, int* scratch, float* dist, hipStream_t s);
void edt_host(const float* t, int N, int C, int H, int W, int* g2, float* dist);
int k_boundary_fwd(const float* x, const float* t, const float* dist, int N, int C, int64_t hw,
                   float* part, double* sum, float* loss, hipStream_t s);
int k_boundary_bwd(const float* x, const float* t, const float* dist, int N, int C, int64_t hw,
                   const float* w, float* dx, hipStream_t s);
// Surface-distance statistics (kernels_surf.hip; definition and rules in surf.h).  scratch holds
// surf_scratch_bytes(N, H, W); out_i64 6 and out_f64 2 values per sample (unet_surface_stats)
size_t surf_scratch_bytes(int N, int H, int W);
int k_surface_stats(const float* x, const float* t, int N, int C, int H, int W, void* scratch,
                    int64_t* out_i64, double* out_f64, hipStream_t s);
// border: 2 H W bytes, d2: 2 H W ints
void surface_stats_host(const float* x, const float* t, int N, int C, int H, int W, uint8_t* border,
                        int* d2, int64_t* out_i64, double* out_f64);
// Training augmentations of uint8 planes (kernels_aug.hip; algorithms and rules in aug.h)
struct ClaheGeom;
int aug_params_check(const unet_aug_params* p, int h, int w);
// noise: one float64 SpeckleNoise draw per output pixel (h * w), or null for none
int k_augment_u8(const uint8_t* src, int h, int w, uint8_t* dst, const unet_aug_params& p,
                 hipStream_t s, const double* noise = nullptr);
void augment_u8_host(const uint8_t* src, int h, int w, uint8_t* dst, const unet_aug_params& p,
                     const double* noise = nullptr);
// unet_status of the refusals; fills G
int clahe_geom(int h, int w, double clip, int gx, int gy, ClaheGeom& G);
size_t clahe_scratch_bytes(const ClaheGeom& G);
int k_clahe_u8(const uint8_t* src, uint8_t* dst, const ClaheGeom& G, void* scratch, hipStream_t s);
void clahe_u8_host(const uint8_t* src, uint8_t* dst, const ClaheGeom& G, int* hist, uint8_t* lut);
// ElasticDeform of uint8 planes (kernels_elastic.hip; algorithm and rules in elastic.h).  tmp
// holds elastic_scratch_bytes(h, w); img / mask (with their destinations) may be null
int elastic_check(const unet_elastic_params* p, int h, int w);  // unet_status of the refusals
size_t elastic_scratch_bytes(int h, int w);
int k_elastic_u8(const uint8_t* img, const uint8_t* mask, int h, int w, uint8_t* img_dst,
                 uint8_t* mask_dst, const double* rx, const double* ry, const unet_elastic_params& p,
                 double* tmp, hipStream_t s);
void elastic_u8_host(const uint8_t* img, const uint8_t* mask, int h, int w, uint8_t* img_dst,
                     uint8_t* mask_dst, const double* rx, const double* ry,
                     const unet_elastic_params& p, double* tmp);
// AdamW scalars, each formed in double and rounded to float once (torch Scalar -> float)
struct AdamwScalars {
    float decay;     // 1 - lr * weight_decay
    float w1;        // 1 - beta1 (lerp weight)
    float b2;        // beta2
    float w2;        // 1 - beta2
    float neg_step;  // -lr / (1 - beta1^step)
    float bc2_sqrt;  // (1 - beta2^step) ** 0.5
    float eps;
    float gscale;    // gradient pre-scale (1 = none)
    int lerp_small;  // |w1| < 0.5 (ATen lerp branch)
};
int k_adamw(float* p, const float* g, float* m, float* v, int64_t n, const AdamwScalars& a,
            hipStream_t s);
int k_mask_counts(const float* x, const float* t, int64_t n, uint8_t* mask, int64_t* counts,
                  hipStream_t s);
int k_nchw_to_nhwc(const float* x, int N, int C, int HW, float* y, hipStream_t s);
int k_fill(float* p, int64_t n, float v, hipStream_t s);

// Connected components, post-processing and lesion counts (kernels_cc.hip; rules in cc.h).  The
// phases are separate launchers so that the context can time each one.  Plane q of a call lives
// at L + q H W; `tile` picks the tile rows (cc_tile_rows: 0 = 16, 1 = 32, 2 = 64; 64 columns).
struct CcScratch {
    unsigned long long* best;  // N keys of the largest kept component
    int *cnt, *kept, *rowcnt;  // planes component counts, N kept counts, planes H roots per row
    size_t zero_bytes;         // the leading part every call zeroes
    int *L, *area;             // planes H W labels; areas, or flags, or ranks of the roots
    size_t bytes;
};
CcScratch cc_scratch(void* base, int N, int planes, int H, int W);
bool cc_grid_ok(int planes, int H, int W);
int cc_tile_rows(int tile);
int k_cc_tile(const void* src, int kind, int64_t sample_stride, int planes, int H, int W, int conn,
              int tile, int* L, int* area, hipStream_t s);
int k_cc_seam(int* L, int planes, int H, int W, int conn, int tile, hipStream_t s);
// area / rowcnt / cnt may be null (not wanted)
int k_cc_flatten(int* L, int* area, int* rowcnt, int* cnt, int planes, int H, int W, hipStream_t s);
int k_cc_rank(const int* L, int* rk, const int* rowcnt, int* count, int planes, int H, int W,
              int* labels, hipStream_t s);
int k_cc_select(const int* L, const int* area, int64_t min_area, int* kept, unsigned long long* best,
                int N, int H, int W, hipStream_t s);
int k_cc_write(const int* L, const int* area, int64_t min_area, int keep_largest, const int* cnt,
               const int* kept, const unsigned long long* best, uint8_t* out, int64_t* info, int N, int H,
               int W, hipStream_t s);
int k_cc_fill(const int* L, int* flag, uint8_t* out, int64_t* info, int N, int H, int W, hipStream_t s);
int k_cc_hits(const int* L, int* flag, int64_t* out, int N, int H, int W, hipStream_t s);
void components_host(const void* src, int kind, int N, int C, int H, int W, int conn, int* labels,
                     int* count);
void postprocess_host(const void* src, int kind, int N, int C, int H, int W, int conn, int keep_largest,
                      int64_t min_area, int fill_holes, uint8_t* out, int64_t* info);
void lesion_stats_host(const void* pred, int kind, const float* targets, int N, int C, int H, int W,
                       int conn, int64_t* out);

// Lesion morphometry (kernels_morph.hip; fields, rules and the host twin in morph.h): the table
// int64 [N][max_rows][16] of the label planes unet_components writes.  The phases are separate
// launchers so that the context can time each one; reduce also initialises the table, extent
// clears and fills the row extents behind the box heights' offsets, feret finishes every row.
// scratch holds morph_scratch(...).bytes.  The callers have checked the arguments.
struct MorphScratch {
    int64_t* off;      // N max_rows: first extent slot of every table row
    int* ext;          // N slots (component, row) extents, two ints each
    int64_t slots;     // ... per sample
    size_t ext_bytes;  // the part every call zeroes
    size_t bytes;
};
MorphScratch morph_scratch(void* base, int N, int H, int W, int64_t max_rows);
bool morph_grid_ok(int N, int H, int W, int64_t max_rows);
// use_lds 0: every contribution straight to global memory (the A/B of tools/morph_time.py)
int k_morph_reduce(const int* labels, int N, int H, int W, int64_t max_rows, int use_lds, int64_t* table,
                   hipStream_t s);
int k_morph_extent(const int* labels, const int* count, int N, int H, int W, int64_t max_rows, const int64_t* table,
                   const MorphScratch& sc, hipStream_t s);
int k_morph_feret(const int* count, int N, int H, int W, int64_t max_rows, const MorphScratch& sc, int64_t* table,
                  hipStream_t s);

// Lesion echogenicity and texture (kernels_echo.hip; columns, rules and the host twin in echo.h): the
// table int32 [N][max_rows][512 + G G] of grey planes and the label planes unet_components writes.
// clear zeroes the whole table, count adds every block's histograms and co-occurrence counts to it.
// No scratch.  The callers have checked the arguments.
bool echo_grid_ok(int N, int H, int W, int64_t max_rows);
int k_echo_clear(int N, int64_t max_rows, int G, int32_t* table, hipStream_t s);
// agg 0: one LDS atomic per lane and count (the A/B of tools/echo_time.py)
int k_echo_count(const uint8_t* gray, const int* labels, const int* count, int N, int H, int W, int64_t max_rows,
                 int G, int w, int agg, int32_t* table, hipStream_t s);

// Test-time augmentation (kernels_tta.hip; rules in tta.h): the views of x, view-major, and the
// merge of the per-view logits.  The callers have checked the arguments (ops_abi.hip).
int k_tta_views(const float* x, int N, int C, int H, int W, uint32_t views, float* out, hipStream_t s);
int k_tta_merge(const float* logits, int N, int C, int H, int W, uint32_t views, int mode, float* score,
                uint8_t* mask, uint8_t* votes, hipStream_t s);
void tta_views_host(const float* x, int N, int C, int H, int W, uint32_t views, float* out);
void tta_merge_host(const float* logits, int N, int C, int H, int W, uint32_t views, int mode, float* score,
                    uint8_t* mask, uint8_t* votes);

// Threshold sweep (kernels_curve.hip; rules and the host twins in curve.h): the class-split
// histogram of `planes` planes of hw logits (plane_hist overwritten, total accumulated) and the
// per-plane statistics of such histograms (dice_sum accumulated in ascending plane order).
// scratch holds curve_scratch_bytes(planes, B).  The callers have checked the arguments.
size_t curve_scratch_bytes(int planes, int B);
int k_curve_hist(const float* x, const float* t, int planes, int64_t hw, const float* edges, int B,
                 int32_t* plane_hist, int64_t* total, hipStream_t s);
int k_curve_stats(const int32_t* plane_hist, int planes, int B, void* scratch, int64_t* out_i64,
                  double* dice_sum, hipStream_t s);

// Lovasz hinge loss (kernels_lovasz.hip; rules in lovasz.h): the segmented stable radix sort of every
// plane's errors, the loss and the per-pixel weights gmap (perm may be null), and the dlogits pass.
// scratch holds lovasz_scratch_bytes(N, C, H, W).  The callers have checked the arguments.
bool lovasz_shape_ok(int N, int C, int H, int W);
size_t lovasz_scratch_bytes(int N, int C, int H, int W);
int k_lovasz_fwd(const float* x, const float* t, int N, int C, int H, int W, void* scratch, float* gmap,
                 uint32_t* perm, double* sum, float* loss, hipStream_t s);
int k_lovasz_bwd(const float* x, const float* t, const float* gmap, int N, int C, int H, int W, const float* w,
                 float* dx, hipStream_t s);
void lovasz_host(const float* x, const float* t, int N, int C, int H, int W, float* gmap, uint32_t* perm,
                 double* sum, float* loss);

// Predict-mode export (kernels_export.hip; rules and the host twins in export.h): the float32
// resize of one plane fused with the threshold (plane may be null; scratch holds
// export_scratch_bytes(h, w, ow)) and the contour / tint overlay with the mask statistics (gt may
// be null; stats: 6 int64, overwritten).  The callers have checked the arguments.
size_t export_scratch_bytes(int h, int w, int ow);
int k_resize_f32_mask(const float* src, int h, int w, int oh, int ow, const double* kh, const int* bh,
                      int ksh, const double* kv, const int* bv, int ksv, int kind, float thr, void* scratch,
                      float* plane, uint8_t* mask, hipStream_t s);
int k_overlay_u8(const uint8_t* gray, const uint8_t* pred, const uint8_t* gt, int h, int w, int r, int alpha,
                 uint8_t* rgb, int64_t* stats, hipStream_t s);
