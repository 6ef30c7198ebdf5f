/*
 * unet_hip.h - C ABI of libunet_hip.so, the MI355X-native (gfx950) UNet training /
 * inference path for the DDTI thyroid-nodule workload.
 *
 * The reference (WuJiaqiii/Thyroid-nodule-image-segmentation-UNet-DDTI) is pure Python;
 * its hot path is PyTorch autograd over models/model.py:UNet plus the losses and the
 * optimizer step driven by utils/trainer.py.  Each entry point below replaces one
 * call site of that path (file:line in the reference):
 *
 *   unet_create / unet_destroy      models/model.py:6-31   UNet.__init__ (topology only;
 *                                                           parameters stay torch-owned)
 *   unet_param_info / unet_bn_info  models/model.py:6-31   named_parameters()/named_buffers()
 *                                                           order, shapes and flat offsets
 *   unet_workspace_size             (new)                  device scratch the caller allocates
 *   unet_forward                    models/model.py:53-73  UNet.forward (train: batch-stat BN
 *                                                           + running-stat update; eval:
 *                                                           running-stat BN), called from
 *                                                           utils/trainer.py:84,139,216
 *   unet_backward                   utils/trainer.py:91    loss.backward() through the UNet
 *   unet_loss_stats / _finalize /   utils/trainer.py:85-87 BCEWithLogitsLoss, models/loss.py:13-24
 *   unet_loss_fwd                                           DiceLoss, models/loss.py:34-46
 *                                                           FocalTverskyLoss (two phases so DP
 *                                                           can all-reduce the batch sums)
 *   unet_loss_bwd                   utils/trainer.py:90-91 d(weighted loss)/d(logits)
 *   unet_edt / unet_edt_host        models/loss.py:55-61   targets.astype(uint8) and scipy's
 *                                                           distance_transform_edt(1 - gt), on the
 *                                                           device (no host round trip)
 *   unet_boundary_fwd / _bwd        models/loss.py:52-66   BoundaryLoss and its d/d(logits)
 *   unet_lovasz_fwd / _bwd / _host  (new)                  Lovasz hinge loss (the convex surrogate of
 *                                                           the Jaccard index) over a stable segmented
 *                                                           radix sort, and its d/d(logits)
 *   unet_surface_stats / _host      (new)                  per-sample surface-distance statistics
 *                                                           of Trainer.test's masks (HD, HD95,
 *                                                           ASSD: MedPy's hd / hd95 / assd)
 *   unet_components / _host         (new)                  connected components of a mask, numbered
 *                                                           as scipy.ndimage.label numbers them
 *   unet_postprocess / _host        (new)                  drop small components, keep the largest,
 *                                                           fill holes (scipy's binary_fill_holes)
 *   unet_lesion_stats / _host       (new)                  per-sample component counts of prediction
 *                                                           and target and how many of each are hit
 *   unet_morphometry / _host        (new)                  per-component size and shape integers of
 *                                                           a label plane: area, moments, box, bit
 *                                                           quads, squared maximum Feret diameter
 *   unet_lesion_echo / _host        (new)                  per-component grey-value histograms of
 *                                                           the lesion and of a ring around it, and
 *                                                           pooled co-occurrence counts (GLCM)
 *   unet_tta_views / _host          (new)                  flip / rotation test-time augmentation:
 *                                                           the dihedral views of a batch, view-major
 *   unet_tta_merge / _host          (new)                  un-warp the per-view logits, average
 *                                                           them, threshold; per-pixel view votes
 *   unet_curve_edges / _hist /      (new)                  threshold sweep: the class-split histogram
 *   _stats / _host                                          of the logits and, per plane, Dice at every
 *                                                           operating point, the best one and the
 *                                                           AUROC numerator (ROC / PR curves)
 *   unet_adamw                      utils/trainer.py:41,92 AdamW.step (torch optim/adam.py
 *                                                           _single_tensor_adam, decoupled wd)
 *   unet_mask_counts                utils/trainer.py:217,236-242  sigmoid(x)>0.5 masks and
 *                                                           TP/FP/FN/TN counts
 *   unet_resize_plan / unet_resize_u8  utils/transforms.py:143-156 Resize + ToTensor of the
 *                                   data loader (data/data_loader.py:20-27), on the device
 *   unet_augment_u8 / _host         main.py:66-91          build_train_transform's Flip -> Rotate
 *                                   -> AdjustBrightness -> TGCAugment (utils/transforms.py:57-70,
 *                                   84-93,114-141) of one uint8 plane, on the device
 *   unet_augment_noise_u8 / _host   utils/transforms.py:45-54 the same with SpeckleNoise between
 *                                   AdjustBrightness and TGCAugment (the noise field is the host's)
 *   unet_clahe_u8 / _host           utils/transforms.py:72-81 CLAHE (cv2.createCLAHE) of one plane
 *   unet_elastic_u8 / _host         utils/transforms.py:15-42 ElasticDeform (cv2.GaussianBlur +
 *                                   cv2.remap) of an image / mask pair from the host's two fields
 *   unet_bucket_* / unet_stream_wait_bucket   utils/trainer.py:28-30 nn.DataParallel grad
 *                                   reduction -> per-bucket readiness for an RCCL all-reduce
 *                                   overlapped with the rest of the backward pass
 *
 * Conventions: every function returns 0 (UNET_OK) or a negative unet_status and never
 * throws across the ABI; unet_last_error() returns the text of the last failure on that
 * context.  All pointers are device pointers owned by the caller (PyTorch) unless noted;
 * the library only borrows them for the duration of the call.  Work is enqueued on the
 * caller's stream with no host synchronisation.  A context is not re-entrant.
 *
 * Tensor layouts at the boundary are the reference's: x (N, Cin, H, W), logits
 * (N, Cout, H, W), parameters in torch layout (Conv2d [Cout,Cin,kh,kw],
 * ConvTranspose2d [Cin,Cout,2,2]) packed back to back in named_parameters() order in one
 * flat fp32 arena (offsets from unet_param_info).  BN buffers: running_mean and
 * running_var in one fp32 arena (layer i: mean at bn_off[i], var at bn_off[i]+C_i) and
 * num_batches_tracked in an int64 array, one per BN layer.
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct unet_ctx unet_ctx;
typedef void* unet_stream_t; /* hipStream_t (0 = legacy default stream) */

typedef enum {
    UNET_OK = 0,
    UNET_ERR_INVALID = -1,     /* null pointer / bad argument */
    UNET_ERR_SHAPE = -2,       /* H or W not divisible by 16, N < 1, ... */
    UNET_ERR_HIP = -3,         /* a HIP runtime call failed */
    UNET_ERR_WORKSPACE = -4,   /* workspace too small */
    UNET_ERR_UNSUPPORTED = -5, /* configuration not implemented */
    UNET_ERR_NOMEM = -6,       /* host allocation failed */
    UNET_ERR_INTERNAL = -7     /* unexpected internal failure (caught C++ exception) */
} unet_status;

/* Which reference network the context runs. */
typedef enum {
    UNET_VARIANT_MODEL = 0, /* models/model.py:UNet -- Conv(+bias) -> ReLU -> BN blocks,
                               concat [up, skip], depth 4, base 64 (fixed) */
    UNET_VARIANT_MOD = 1,   /* models/mod.py:9-66 UNet -- Conv(no bias) -> BN -> ReLU blocks,
                               concat [skip, up], base_filters / depth configurable */
    UNET_VARIANT_RES = 2    /* models/mod.py:71-131 ResUNet -- residual blocks
                               ReLU(Conv-BN-ReLU-Conv-BN(x) + Conv1x1(x)), otherwise as MOD
                               (the network main.py:122 builds) */
} unet_variant;

/* Arithmetic of the convolution GEMMs. */
typedef enum {
    UNET_MATH_F32 = 0,  /* f32 products (the reference's fp32): by default (option x3) the GEMMs
                           with 64-multiple channel counts run on v_mfma_f32_32x32x16_bf16 through
                           exact three-way bf16 splits of the f32 operands (six piece products,
                           split f32 accumulators: below the f32 MFMA's error against fp64), the
                           rest on v_mfma_f32_32x32x2_f32 */
    UNET_MATH_BF16 = 1  /* v_mfma_f32_32x32x16_bf16: operands rounded to bf16, f32 accumulate
                           (BASELINE config 4; models/mod.py variant only) */
} unet_math;

typedef struct {
    int in_channels;   /* models/model.py:6 / mod.py:11 in_channels (default 1; must be 1) */
    int out_channels;  /* models/model.py:6 / mod.py:12 out_channels (default 1; 1..4)   */
    int variant;       /* unet_variant (0 = models/model.py)                               */
    int base_filters;  /* mod.py:13 (0 = default 64); a multiple of 8, <= 256.  Channels are
                          padded per level inside the library (the caller's arenas keep the
                          torch layouts): level 0 runs the next power of two >= 32 of
                          base_filters, every deeper level the next multiple of 32 of
                          base_filters << level (base 16: 32, 32, 64, 128, 256 -- only level 0
                          padded; 24: 32, 64, 96, 192, ...; 48: 64, 96, 192, ...) */
    int depth;         /* mod.py:14 (0 = default 5 for mod, 4 for model); 1..6             */
    int math;          /* unet_math of the conv GEMMs (0 = f32)                            */
} unet_cfg;

/* models/model.py:6-31 / models/mod.py:10-41.  device = HIP ordinal the context will
 * launch on.  Zero-initialised fields take the reference defaults. */
int unet_create(const unet_cfg* cfg, int device, unet_ctx** out);
int unet_destroy(unet_ctx* ctx);
const char* unet_last_error(const unet_ctx* ctx);

/* Parameter table in named_parameters() order.  n_floats = size of the flat arena. */
int unet_num_params(const unet_ctx* ctx, int* n_tensors, int64_t* n_floats);
/* name: static string owned by the library; shape: up to 4 dims. */
int unet_param_info(const unet_ctx* ctx, int i, const char** name, int* ndim, int64_t shape[4],
                    int64_t* offset);
/* BN layer table: n_layers, total floats of the running-stat arena (mean|var per layer). */
int unet_num_bn(const unet_ctx* ctx, int* n_layers, int64_t* n_floats);
int unet_bn_info(const unet_ctx* ctx, int i, const char** name, int* channels, int64_t* offset);

/* Bytes of device workspace for one forward (+backward when training) at (N, H, W).
 * H and W must be multiples of max(16, 2**depth).  The size depends on the configuration, the
 * shape, `training` and the schedule options (unet_set_option) in force at the call, and on
 * nothing else: ask again after changing an option.
 *
 * The workspace contract of unet_forward / unet_backward:
 *   - `workspace` must be 256-byte aligned (hipMalloc and torch's allocator give more).  The
 *     planner places every region at a multiple of 256 bytes from the base, and the kernels read
 *     them with 16-byte loads and LDS-DMA; a misaligned base is UNET_ERR_INVALID, and fewer than
 *     unet_workspace_size bytes UNET_ERR_WORKSPACE, both before any device work.
 *   - Its contents on entry do not matter: a forward reads nothing from it that it (or, with the
 *     fused AdamW, unet_adamw_repack) has not written, whatever bytes an earlier tenant left,
 *     NaN patterns included.  A backward reads only what the training forward on the same
 *     workspace and the backward itself wrote.
 *   - Nothing outside [workspace, workspace + unet_workspace_size) is written, apart from the
 *     outputs named below (logits, the BN buffers of a training forward, grads). */
int unet_workspace_size(unet_ctx* ctx, int N, int H, int W, int training, size_t* bytes);

/* Forward.  params: flat arena; bn_running: running-stat arena (updated when training);
 * bn_count: int64[n_bn] num_batches_tracked (incremented when training); x: (N,Cin,H,W);
 * logits: (N,Cout,H,W).  The workspace keeps what backward needs; pass the same one. */
int unet_forward(unet_ctx* ctx, const float* params, float* bn_running, int64_t* bn_count,
                 const float* x, float* logits, void* workspace, size_t ws_bytes, int N, int H,
                 int W, int training, unet_stream_t stream);

/* Backward of the last training forward run with this workspace.  dlogits: (N,Cout,H,W).
 * grads: flat arena laid out like params; every entry is overwritten (zero_grad -> None
 * semantics, utils/trainer.py:81). */
int unet_backward(unet_ctx* ctx, const float* params, const float* dlogits, float* grads,
                  void* workspace, size_t ws_bytes, int N, int H, int W, unet_stream_t stream);

/* Losses over logits/targets (N, C, H, W) (targets may be soft, e.g. mixup), in two
 * phases so that data parallelism can insert one collective between them:
 *   unet_loss_stats     per-sample partials stats (device fp32[4*N]) and the batch sums
 *                       sums (device fp64[8]) = {sum bce_elem, sum_n dice_n, TP, sum p,
 *                       sum t, samples, elements, 0}
 *   [DP: all-reduce(SUM) sums across ranks -- the loss of the gathered batch, exactly
 *        what nn.DataParallel evaluates (utils/trainer.py:28-30,85-90); FocalTversky's
 *        TP/FP/FN are batch-global (models/loss.py:41-45)]
 *   unet_loss_finalize  losses (device fp32[3]) <- {bce_mean, dice_loss, focal_tversky}
 * unet_loss_fwd = unet_loss_stats + unet_loss_finalize (single process).
 * focal uses (alpha, beta, gamma) of utils/trainer.py:38 / models/loss.py:27 defaults.
 * (r06) unet_loss_stats sums each sample in chunks into a context-owned scratch (grown on
 * demand without a host synchronisation; an outgrown buffer is released by unet_destroy): one
 * loss pass per context in flight at a time, i.e. issue a context's loss calls on one stream. */
int unet_loss_stats(unet_ctx* ctx, const float* logits, const float* targets, int N, int C, int H,
                    int W, float* stats, double* sums, unet_stream_t stream);
int unet_loss_finalize(unet_ctx* ctx, const double* sums, float* losses, float focal_alpha,
                       float focal_beta, float focal_gamma, unet_stream_t stream);
int unet_loss_fwd(unet_ctx* ctx, const float* logits, const float* targets, int N, int C, int H,
                  int W, float* stats, double* sums, float* losses, float focal_alpha,
                  float focal_beta, float focal_gamma, unet_stream_t stream);
/* dlogits = w[0]*dBCE + w[1]*dDice + w[2]*dFocal of the batch described by `sums`
 * (w a device fp32[3]).  With all-reduced sums each rank writes its slice of the
 * gathered batch's dlogits, so the ranks' gradients SUM to the reference's. */
int unet_loss_bwd(unet_ctx* ctx, const float* logits, const float* targets, int N, int C, int H,
                  int W, const float* stats, const double* sums, const float* w, float* dlogits,
                  float focal_alpha, float focal_beta, float focal_gamma, unet_stream_t stream);

/* BoundaryLoss (models/loss.py:48-66): mean_n mean_hw |sigmoid(x[n,0]) - t[n,0]| * dist[n], dist
 * the exact Euclidean distance transform of the target (models/loss.py:55-61:
 * scipy.ndimage.distance_transform_edt(1 - targets.astype(np.uint8)[n, 0])).
 *   unet_edt       targets (N, C, H, W) f32, only channel 0 read -> dist (N, 1, H, W) f32, bit for
 *                  bit scipy's float64 result cast to float32.  A pixel is a feature site
 *                  (distance 0) iff (uint8)t == 1, i.e. 1 <= t < 2: a soft mixup target below 1 is
 *                  not a site.  dist = sqrt(min over sites of dy^2 + dx^2), the minimum exact in
 *                  int32.  A sample WITHOUT any site gets scipy's answer for an all-background
 *                  input, the distance to a virtual site at row -1, column 0:
 *                  sqrt((i + 1)^2 + j^2) (observed with scipy 1.15; the reference trains on it).
 *                  max(H, W) > 2048 is UNET_ERR_SHAPE (keeps the squared distance below 2^24,
 *                  where the float32 result is exact); no other shape constraint.
 *   unet_edt_host  HOST function: the same 1-D passes (csrc/edt.h, shared host / device source)
 *                  on host pointers.
 *   unet_boundary_fwd  sum (device fp64[1]) = sum_n mean_hw |p - t| dist (per sample in chunks,
 *                  then double, as unet_loss_stats), loss (device fp32[1]) = sum / N.
 *   unet_boundary_bwd  dlogits[n,0] = w[0] sign(p - t) dist p (1 - p) / (N H W) with sign(0) = 0
 *                  (torch's abs backward), w a device fp32[1]; channels 1.. are written as zero.
 * All work is enqueued on `stream` with no host synchronisation; the scratch is owned by the
 * context and grown on demand (an outgrown buffer is released by unet_destroy), so issue a
 * context's boundary calls on one stream, or order the streams. */
int unet_edt(unet_ctx* ctx, const float* targets, int N, int C, int H, int W, float* dist,
             unet_stream_t stream);
int unet_edt_host(const float* targets, int N, int C, int H, int W, float* dist);
int unet_boundary_fwd(unet_ctx* ctx, const float* logits, const float* targets, const float* dist,
                      int N, int C, int H, int W, double* sum, float* loss, unet_stream_t stream);
int unet_boundary_bwd(unet_ctx* ctx, const float* logits, const float* targets, const float* dist,
                      int N, int C, int H, int W, const float* w, float* dlogits,
                      unet_stream_t stream);

/* Lovasz hinge loss (Berman et al., CVPR 2018, per_image=True; rules in csrc/lovasz.h, kernels in
 * csrc/kernels_lovasz.hip).  Every (n, c) plane of logits / targets (N, C, H, W) is its own binary
 * problem over its M = H W pixels, i the raster index:
 *   label   y_i = (t_i >= 0.5f), s_i = y_i ? +1 : -1: a soft (mixup) target is binarised at one half;
 *   error   e_i = fl32(1 - s_i x_i) (the product is exact: one rounding);
 *   order   descending e, ties by ascending i (a STABLE sort: np.argsort(-e, kind="stable")); +0 and
 *           -0 are equal keys, +-inf sort as values; the place of a NaN is unspecified, its plane's
 *           loss is NaN, and no index ever leaves the plane;
 *   counts  P = sum y; cTP_r, cFP_r = positives / negatives among the ranks <= r (exact integers);
 *   weights J_r = 1 - (P - cTP_r) / (P + cFP_r) in float64 (the denominator is >= 1), J_{-1} = 0,
 *           g_r = J_r - J_{r-1};
 *   loss    L_plane = sum_r max(e_r, 0) g_r, products and sum in float64 in a fixed order (run-to-run
 *           deterministic).
 *   unet_lovasz_fwd  gmap (N, C, H, W) f32, in PIXEL order: fl32(g_rank(i)) where e_i > 0, 0 elsewhere
 *                  (the per-pixel weight the backward needs); perm (optional, may be null): uint32
 *                  (N, C, H W), the raster indices of every plane in sorted order, all M of them;
 *                  sum (device fp64[1]) = sum_planes L_plane; loss (device fp32[1]) = sum / (N C).
 *                  H W > 2^24 is UNET_ERR_SHAPE; no other shape constraint.
 *   unet_lovasz_bwd  dlogits_i = (w[0] * -s_i) * gmap_i / (N C) where e_i > 0, 0 elsewhere
 *                  (relu'(0) = 0), in float32 in this order; w a device fp32[1].
 *   unet_lovasz_host HOST function: the same rules (csrc/lovasz.h, shared host / device source) with a
 *                  stable sort by key, on host pointers; gmap and perm are bit-equal to the device's.
 * All work is enqueued on `stream` with no host synchronisation; the scratch (16 bytes per pixel) is
 * owned by the context and grown on demand (an outgrown buffer is released by unet_destroy), so issue
 * a context's Lovasz calls on one stream, or order the streams. */
int unet_lovasz_fwd(unet_ctx* ctx, const float* logits, const float* targets, int N, int C, int H, int W,
                    float* gmap, uint32_t* perm, double* sum, float* loss, unet_stream_t stream);
int unet_lovasz_bwd(unet_ctx* ctx, const float* logits, const float* targets, const float* gmap, int N,
                    int C, int H, int W, const float* w, float* dlogits, unet_stream_t stream);
int unet_lovasz_host(const float* logits, const float* targets, int N, int C, int H, int W, float* gmap,
                     uint32_t* perm, double* sum, float* loss);

/* AdamW over flat arenas of n floats (one launch for all parameter tensors; any part of a
 * parameter arena, too: the weight images of unet_adamw_repack are dropped if it overlaps theirs).
 * Hyper-parameters are the optimizer's Python floats (double); the library forms
 * 1 - lr*wd, 1 - beta1, 1 - beta2, -lr/(1 - beta1^step) and (1 - beta2^step)**0.5 in
 * double and rounds each to float once, as torch does (optim/adam.py _single_tensor_adam).
 * grads are multiplied by grad_scale first when it is not 1. */
int unet_adamw(unet_ctx* ctx, float* params, const float* grads, float* exp_avg,
               float* exp_avg_sq, int64_t n, int step, double lr, double beta1, double beta2,
               double eps, double weight_decay, double grad_scale, unet_stream_t stream);

/* (r06) The same AdamW step (utils/trainer.py:41,92 AdamW(...).step()) over the whole parameter
 * arena of this context (n == the unet_num_params float count), fused with the weight repack
 * the next forward needs: every 3x3 conv / ConvT weight tile is updated and packed into the
 * context's own GEMM images in one pass, the other tensors are updated elementwise.  Results
 * are bit-identical to unet_adamw.  The context holds ONE set of images: those of the arena
 * repacked last.  The next unet_forward on the same `params` pointer reads them instead of
 * repacking; a forward on any other arena (another model of this configuration) packs into
 * its own workspace, as every forward did before.  The images stop being read once
 *   - the arena is declared written by other means (unet_arena_changed, unet_params_changed:
 *     load_state_dict, another optimizer, a broadcast),
 *   - unet_adamw on this context writes into any part of the arena,
 *   - unet_set_option changes a value (which images exist depends on the options), or
 *   - the next repack replaces them.
 * Each training forward records, with its workspace, whether it read the context's images.
 * Its unet_backward reads the same ones: the workspace's own, or the context's -- and then
 * refuses (UNET_ERR_INVALID) only if a later unet_adamw_repack REWROTE them in between.  An
 * invalidation alone rewrites nothing and never fails a backward.  Another n, or a
 * channel-padded network, runs the plain unet_adamw. */
int unet_adamw_repack(unet_ctx* ctx, float* params, const float* grads, float* exp_avg,
                      float* exp_avg_sq, int64_t n, int step, double lr, double beta1, double beta2,
                      double eps, double weight_decay, double grad_scale, unet_stream_t stream);
/* The caller changed the parameter arena outside unet_adamw_repack: the next forward repacks
 * (whichever arena the context's images belong to). */
int unet_params_changed(unet_ctx* ctx);
/* The same, scoped to one arena: the caller wrote into [params, params + n) floats.  The
 * images are dropped only if they belong to an arena that range overlaps, so a model that
 * shares this context with others does not cost them their images. */
int unet_arena_changed(unet_ctx* ctx, const float* params, int64_t n);

/* Mask readout + confusion counts, utils/trainer.py:101-107,217-242, utils/utils.py:225-251.
 * counts (device int64[6]) += {TP, FP, FN, TN} of (sigmoid(logits) > 0.5) vs targets cast to
 * an integer (== 1 is positive), then {|pred AND t!=0|, |pred OR t!=0|} (the bool cast of
 * calculate_iou).  mask (optional, may be null): uint8 (N,C,H,W). */
int unet_mask_counts(unet_ctx* ctx, const float* logits, const float* targets, int64_t n,
                     uint8_t* mask, int64_t* counts, unet_stream_t stream);

/* Surface-distance statistics of the masks unet_mask_counts reads (MedPy's hd, hd95 and assd at
 * connectivity 1, in pixels; csrc/surf.h).  Per sample n, with P = sigmoid(logits[n, 0]) > 0.5
 * and G = ((int)targets[n, 0] == 1) (channels above 0 are not read):
 *   border(A)  the foreground pixels of A with a 4-neighbour that is background or outside the
 *              image (A & ~binary_erosion(A), border_value 0);
 *   d_PG       the squared Euclidean distances, exact in int32, from each pixel of border(P) to
 *              the nearest pixel of border(G); d_GP likewise from border(G) to border(P);
 *   out_i64[6 n ..] = {defined, n_PG, n_GP, max_d2, d2_lo, d2_hi}: the sizes of d_PG and d_GP,
 *              the largest squared distance of both, and the order statistics
 *              floor(0.95 (n - 1)) and ceil(0.95 (n - 1)) of the n = n_PG + n_GP squared
 *              distances of both (the two values numpy.percentile(.., 95) interpolates between),
 *              selected exactly by a radix select;
 *   out_f64[2 n ..] = {sum_PG, sum_GP}: the float64 sums of sqrt(d2) over d_PG and d_GP.
 * So HD = sqrt(max_d2), HD95 = lerp(sqrt(d2_lo), sqrt(d2_hi), frac(0.95 (n - 1))) and
 * ASSD = (sum_PG / n_PG + sum_GP / n_GP) / 2.  A sample whose P or G is empty is undefined:
 * defined = 0 and every other field 0.  Both outputs are device memory; all work is enqueued on
 * `stream` with no host synchronisation, every sum in a fixed order (two runs agree bit for
 * bit); the scratch is owned by the context and grown on demand (one stream per context, or
 * ordered streams).  max(H, W) > 2048 is UNET_ERR_SHAPE, a null pointer UNET_ERR_INVALID.
 * unet_surface_stats_host is the HOST twin (host pointers, same source); its float64 sums run
 * over the pixels in raster order. */
int unet_surface_stats(unet_ctx* ctx, const float* logits, const float* targets, int N, int C,
                       int H, int W, int64_t* out_i64, double* out_f64, unet_stream_t stream);
int unet_surface_stats_host(const float* logits, const float* targets, int N, int C, int H, int W,
                            int64_t* out_i64, double* out_f64);

/* Connected components of the masks unet_mask_counts reads, the post-processing built on them and
 * lesion-level detection counts (csrc/cc.h; kernels in csrc/kernels_cc.hip).  All integer and
 * exact: the device, the host twins and scipy agree bit for bit, whatever the order of the atomics.
 * src is (N, C, H, W), channel 0 read, and `kind` selects its foreground:
 *   0  uint8, nonzero (C = 1: a uint8[N, H, W] plane);
 *   1  float logits, sigmoid(x) > 0.5 as unet_mask_counts forms it;
 *   2  float targets, (int)t == 1.
 * connectivity 1 is scipy's generate_binary_structure(2, 1) (4 neighbours), 2 is np.ones((3, 3))
 * (8 neighbours).
 *   unet_components   labels int32[N, H, W] = scipy.ndimage.label of each sample: 0 background,
 *                     1..K components in raster order of their first pixel (label = 1 + the rank,
 *                     among the sample's components, of the component's smallest linear index);
 *                     count int32[N] = K.  Phases, one launch each: a tile pass (a 64-column tile
 *                     per block in LDS, row runs by wave ballot, union-find with LDS atomicMin), a
 *                     seam pass (lock-free union by smaller index across tile borders), a flatten
 *                     pass (label = find, roots per row, areas) and a rank pass (raster rank of the
 *                     roots, then the labels rewritten to 1..K).  No kernel waits for another block.
 *   unet_postprocess  out uint8[N, H, W] in {0, 1}, out != src: of each sample's foreground,
 *                     (1) the components with area >= min_area (min_area <= 1 keeps all), then
 *                     (2) if keep_largest, the largest of them, on equal areas the lowest label
 *                     (np.argmax(np.bincount(lab.ravel())[1:]) + 1; empty stays empty), then
 *                     (3) if fill_holes, scipy.ndimage.binary_fill_holes (default structure: the
 *                     background components, at connectivity 1, that do not touch the image
 *                     border become foreground).  info int64[4 N] = {components before,
 *                     components kept, foreground pixels after, pixels filled} per sample.
 *   unet_lesion_stats out int64[4 N] = {n_pred, n_gt, gt_hit, pred_hit} per sample for the
 *                     prediction `pred` (any kind) and the float targets (kind 2, same N, C, H, W):
 *                     the component counts of both, the target components that hold a pixel of the
 *                     prediction and the predicted components that hold a pixel of the target.
 * A connectivity other than 1 or 2, an unknown kind, N, C, H or W < 1, H * W >= 2^31 or a null
 * pointer is UNET_ERR_INVALID; a batch whose pixel count does not fit one launch (about 2^39) is
 * UNET_ERR_SHAPE.  Outputs are device memory; all work is enqueued on `stream` with no host
 * synchronisation; labels, areas and flags live in a context-owned scratch grown on demand (one
 * stream per context, or ordered streams).  The _host functions are the HOST twins (host
 * pointers, the same cc.h rules). */
int unet_components(unet_ctx* ctx, const void* src, int kind, int N, int C, int H, int W,
                    int connectivity, int32_t* labels, int32_t* count, unet_stream_t stream);
int unet_components_host(const void* src, int kind, int N, int C, int H, int W, int connectivity,
                         int32_t* labels, int32_t* count);
int unet_postprocess(unet_ctx* ctx, const void* src, int kind, int N, int C, int H, int W,
                     int connectivity, int keep_largest, int64_t min_area, int fill_holes,
                     uint8_t* out, int64_t* info, unet_stream_t stream);
int unet_postprocess_host(const void* src, int kind, int N, int C, int H, int W, int connectivity,
                          int keep_largest, int64_t min_area, int fill_holes, uint8_t* out,
                          int64_t* info);
int unet_lesion_stats(unet_ctx* ctx, const void* pred, int kind, const float* targets, int N, int C,
                      int H, int W, int connectivity, int64_t* out, unet_stream_t stream);
int unet_lesion_stats_host(const void* pred, int kind, const float* targets, int N, int C, int H,
                           int W, int connectivity, int64_t* out);

/* Lesion morphometry: the size and shape integers of every connected component (csrc/morph.h;
 * kernels in csrc/kernels_morph.hip).  labels int32[N, H, W] and count int32[N] as unet_components
 * writes them (0 background, 1..count[n] the components).  table int64[N, max_rows, 16], the row of
 * label l at index l - 1, with x the column, y the row and the sums over the component's pixels:
 *    0      area                          1, 2   sx, sy            3, 4, 5  sxx, sxy, syy
 *    6..9   x0, y0, x1, y1 (inclusive bounding box)
 *   10..13  q1, q2, qd, q3: the 2 x 2 windows of the zero-padded plane, (H + 1) (W + 1) of them, in
 *           which the component's own indicator has one pixel, two edge-adjacent, two diagonal, three
 *           (perimeter and Euler number follow; four set from q1 + 2 q2 + 2 qd + 3 q3 + 4 q4 = 4 area)
 *   14      d2max: the largest dx^2 + dy^2 over the component's pixel pairs (squared maximum Feret
 *           diameter between pixel centres; 0 for one pixel)
 *   15      first: the component's smallest linear index y W + x
 * Rows at or beyond count[n] are zero.  A component whose label exceeds max_rows is dropped without a
 * memory access; count[n] > max_rows tells the caller.  All integer and exact: the device, the host
 * twin and a NumPy restatement agree bit for bit, whatever the order of the atomics.  Phases: a
 * reduce pass (64-column tiles, the runs of a tile row from one wave ballot, closed-form run sums,
 * a label-keyed LDS table per block before the 64-bit global atomics), a row-extent pass behind a
 * scan of the box heights (at most H ceil(W / 2) (component, row) slots per sample) and one block
 * per table row over the pairs of its row extremes.  No kernel waits for another block.
 * A null pointer, N, H, W or max_rows < 1, or H * W >= 2^31 is UNET_ERR_INVALID; H or W above 4096
 * (which keeps sxx, sxy, syy below 2^48), or N * max_rows >= 2^31, is UNET_ERR_SHAPE.  labels, count
 * and table are device memory; all work is enqueued on `stream` with no host synchronisation; the
 * offsets and extents live in a context-owned scratch grown on demand (one stream per context, or
 * ordered streams).  unet_morphometry_host is the HOST twin (host pointers, the same morph.h rules). */
int unet_morphometry(unet_ctx* ctx, const int32_t* labels, const int32_t* count, int N, int H, int W,
                     int64_t max_rows, int64_t* table, unet_stream_t stream);
int unet_morphometry_host(const int32_t* labels, const int32_t* count, int N, int H, int W,
                          int64_t max_rows, int64_t* table);

/* Lesion echogenicity and texture: the grey values under every connected component and in a band
 * around it, as integer counts (csrc/echo.h; kernel in csrc/kernels_echo.hip).  gray uint8[N, H, W];
 * labels int32[N, H, W] and count int32[N] as unet_components writes them (anything <= 0 background);
 * levels G in {8, 16, 32}; ring w in 0..16.  table int32[N, max_rows, 512 + G G], the row of label l
 * at index l - 1:
 *     0..255  lesion histogram: column g counts the pixels with label l and grey value g
 *   256..511  ring histogram: the owner of a background pixel is the smallest positive label in the
 *             (2 w + 1) x (2 w + 1) window around it, clipped to the plane (chessboard distance <= w,
 *             ties to the lower label); column 256 + g of the owner's row counts the pixel.  w = 0
 *             leaves these columns zero.
 *   512...    pooled co-occurrence counts at the level q(g) = (g G) >> 8: for every pixel p and offset
 *             (dy, dx) in (0, 1), (1, 1), (1, 0), (1, -1) whose neighbour lies in the plane and carries
 *             p's label l, entry [q(p)][q(neighbour)] of row l gains one (ordered pairs, counted once,
 *             the four directions summed; the caller symmetrises).
 * Every count is at most 4 H W <= 2^26.  Rows at or beyond count[n] are zero.  A label above
 * min(count[n], max_rows) is dropped without a memory access; count[n] > max_rows tells the caller.
 * The call clears the table itself (uninitialised memory may be handed in) and uses no scratch.  All
 * integer and exact: the device, the host twin and a NumPy restatement agree bit for bit, whatever
 * the launch geometry and the order of the atomics.  One block per 64 x 32 tile stages the labels
 * with a halo of max(w, 1) in LDS, finds the ring owners by a separable minimum there, and counts
 * into a label-keyed LDS table (option echo_agg = 1: wave-aggregated adds) flushed by global integer
 * atomics; labels beyond its slots add straight to global memory.
 * A null pointer, N, H, W or max_rows < 1, H * W >= 2^31, levels outside {8, 16, 32} or ring outside
 * 0..16 is UNET_ERR_INVALID; H or W above 4096, or N * max_rows >= 2^31, is UNET_ERR_SHAPE.  gray,
 * labels, count and table are device memory; all work is enqueued on `stream` with no host
 * synchronisation.  unet_lesion_echo_host is the HOST twin (host pointers, the same echo.h rules). */
int unet_lesion_echo(unet_ctx* ctx, const uint8_t* gray, const int32_t* labels, const int32_t* count,
                     int N, int H, int W, int64_t max_rows, int levels, int ring, int32_t* table,
                     unet_stream_t stream);
int unet_lesion_echo_host(const uint8_t* gray, const int32_t* labels, const int32_t* count, int N, int H,
                          int W, int64_t max_rows, int levels, int ring, int32_t* table);

/* Flip / rotation test-time augmentation (csrc/tta.h; kernels in csrc/kernels_tta.hip).  View k in
 * 0..7 has bits h = k & 1, v = (k >> 1) & 1, t = (k >> 2) & 1:
 *   T_k(x): y = x;  if t: y = y.swapaxes(-1, -2);  if v: y = y[..., ::-1, :];  if h: y = y[..., ::-1]
 * (0 identity, 1..3 the flips, 4 transpose, 5 and 6 the quarter turns, 7 anti-transpose: D4).  `views`
 * is a bit mask (bit k), K = popcount(views), the views taken in ascending k; named sets of the
 * Python level: hflip 0x03, flips 0x0F, d4 0xFF.
 *   unet_tta_views  out (K N, C, H, W), view-major: out[q N + n] = T_{k_q}(x[n]).  A pure
 *                   permutation, bit-exact.
 *   unet_tta_merge  logits (K N, C, H, W) in the same order: the model's output for `out`.  Per
 *                   output element (n, c, i, j), x_q = T_{k_q}^-1(logits[q N + n, c])[i, j] (the
 *                   inverse undoes h, then v, then t), and
 *                     mode 0 (logit): score = (x_0 + ... + x_{K-1}) / (float)K,
 *                                     mask = 1 / (1 + expf(-score)) > 0.5f (unet_mask_counts' readout);
 *                     mode 1 (prob):  score = (p_0 + ... + p_{K-1}) / (float)K with
 *                                     p_q = 1.f / (1.f + expf(-x_q)), mask = score > 0.5f;
 *                     votes = the number of views with 1 / (1 + expf(-x_q)) > 0.5f (0..K).
 *                   The sum is a float32 sum in ascending q, each operation rounded on its own, the
 *                   division the correctly rounded one: two runs, and in mode 0 the device and the
 *                   host twin, agree bit for bit.  score float (N, C, H, W); mask and votes uint8
 *                   (N, C, H, W), either may be null; no output may overlap logits.
 * views == 0 or a bit above 7, a mode other than 0 / 1, N, C, H or W < 1, H * W >= 2^31, a null x /
 * out / logits / score or an output overlapping logits is UNET_ERR_INVALID; a view with t when
 * H != W, or K * N * C >= 2^31, is UNET_ERR_SHAPE.  A row length that is no multiple of 4 and
 * pointers that are only 4-byte aligned are legal (a scalar path).  All work is enqueued on `stream`
 * with no host synchronisation, no scratch and no atomics.  The _host functions are the HOST twins
 * (host pointers, the same tta.h rules). */
int unet_tta_views(unet_ctx* ctx, const float* x, int N, int C, int H, int W, uint32_t views,
                   float* out, unet_stream_t stream);
int unet_tta_views_host(const float* x, int N, int C, int H, int W, uint32_t views, float* out);
int unet_tta_merge(unet_ctx* ctx, const float* logits, int N, int C, int H, int W, uint32_t views,
                   int mode, float* score, uint8_t* mask, uint8_t* votes, unet_stream_t stream);
int unet_tta_merge_host(const float* logits, int N, int C, int H, int W, uint32_t views, int mode,
                        float* score, uint8_t* mask, uint8_t* votes);

/* Threshold sweep (csrc/curve.h; kernels in csrc/kernels_curve.hip): ROC / PR curves, Dice at every
 * operating point and the choice of one, from a histogram of the logits split by target class.
 * Everything is defined on the logits by float comparisons and integer sums (no transcendental on
 * the device), so the device, the host twins and a NumPy restatement agree bit for bit.
 *   Edges   B bins, B a power of two in 2..1024, separated by B - 1 strictly increasing float32
 *           edges e[0..B-2].  unet_curve_edges (a HOST function) writes the standard ones, the
 *           logits of the probabilities (j + 1) / B: e[j] = (float)log(t / (1 - t)), t = (j + 1) / B
 *           in double, exactly antisymmetric, e[B/2 - 1] == 0.0f.
 *   Bin     bin(x) = the number of j with e[j] < x, in 0..B-1: NaN and -inf in bin 0, +inf in bin
 *           B-1, -0.0f not > 0.0f.  The search yields an in-range bin for any contents of `edges`.
 *   Class   u = (uint8_t)(int)t, unet_mask_counts' target readout: u == 1 positive, u == 0 negative,
 *           anything else ignored and counted.
 *   Operating point k in 0..B: predicted positive iff bin(x) >= k (k = 0 every pixel, k = B none,
 *           else x > e[k-1]).  k = B/2 is x > 0: unet_mask_counts' sigmoid(x) > 0.5 readout, except
 *           for logits in (0, ~2^-24], where expf(-x) rounds to 1 and the readout says background.
 *   unet_curve_hist   logits, targets: `planes` contiguous planes of hw floats ((N, C, H, W) is N C
 *           planes).  plane_hist int32 [planes][2][B] (row 0 negatives, 1 positives) is overwritten;
 *           total int64 [2 B + 1] is accumulated (+=, as unet_mask_counts' counts): the two rows
 *           summed over the planes, then the ignored pixels.
 *   unet_curve_stats  per plane, with P = sum pos, Nn = sum neg, TP_k / FP_k the sums over b >= k,
 *           dice_k = (TP_k + FP_k + P == 0) ? 1.0 : (double)(2 TP_k) / (double)(TP_k + FP_k + P),
 *           best_k the k of the largest dice_k (equal doubles: the smallest |k - B/2|, then the
 *           smaller k) and auc2 = sum_b pos[b] (2 sum_{b' < b} neg[b'] + neg[b]) (AUROC = auc2 /
 *           (2 P Nn)): out_i64 [planes][8] = {P, Nn, best_k, TP, FP, FN at best_k, auc2, 0};
 *           dice_sum double [B + 1] += dice_k over the planes in ascending plane order (a fixed
 *           order: two runs, and the device and the host twin, agree bit for bit).
 * A null pointer, B no power of two or outside 2..1024, planes < 1 or hw < 1 is UNET_ERR_INVALID;
 * hw >= 2^31 is UNET_ERR_SHAPE.  Pointers that are only 4-byte aligned and an hw that is no multiple
 * of 4 are legal (a scalar path).  All work is enqueued on `stream` with no host synchronisation;
 * the statistics use a context-owned scratch grown on demand.  The _host functions are the HOST
 * twins (host pointers, the same curve.h rules). */
int unet_curve_edges(int B, float* edges);
int unet_curve_hist(unet_ctx* ctx, const float* logits, const float* targets, int planes, int64_t hw,
                    const float* edges, int B, int32_t* plane_hist, int64_t* total,
                    unet_stream_t stream);
int unet_curve_hist_host(const float* logits, const float* targets, int planes, int64_t hw,
                         const float* edges, int B, int32_t* plane_hist, int64_t* total);
int unet_curve_stats(unet_ctx* ctx, const int32_t* plane_hist, int planes, int B, int64_t* out_i64,
                     double* dice_sum, unet_stream_t stream);
int unet_curve_stats_host(const int32_t* plane_hist, int planes, int B, int64_t* out_i64,
                          double* dice_sum);

/* Gradient buckets for data-parallel overlap.  Bucket b covers grads[offset, offset+len)
 * and is complete once the event recorded by unet_backward for it has fired; buckets
 * become ready in order 0, 1, ... (decoder first). */
int unet_num_buckets(const unet_ctx* ctx, int* n);
int unet_bucket_range(const unet_ctx* ctx, int b, int64_t* offset, int64_t* len);
/* Make `stream` wait (device-side) until bucket b of the last backward is complete. */
int unet_stream_wait_bucket(unet_ctx* ctx, int b, unet_stream_t stream);
/* The hipEvent_t (returned as void*) that each unet_backward records on its stream when
 * bucket b is complete -- for a caller that drives RCCL (ncclAllReduce on its own
 * hipStream_t) without torch: hipStreamWaitEvent(comm_stream, ev, 0), then reduce
 * grads[offset, offset+len).  Owned by the context (valid until unet_destroy; created by
 * the first unet_backward, UNET_ERR_INVALID before it). */
int unet_bucket_event(unet_ctx* ctx, int b, void** hip_event);

/* Input pipeline (data/data_loader.py:20-27 + utils/transforms.py:143-156): the reference
 * resizes every PIL image and mask with TF.resize (= Pillow Image.resize(size, BILINEAR))
 * and scales with TF.to_tensor (float(u8) / 255).  unet_resize_plan is a HOST function:
 * Pillow's resampling coefficients (22-bit fixed point) and source bounds for one axis,
 * coeffs[out_size * ksize], bounds[2 * out_size] = {first, count}; pass coeffs = bounds =
 * NULL to get *ksize only.  unet_resize_u8 resizes one (h, w) uint8 image on the device
 * into dst (oh, ow) fp32, divided by `divisor` (255 for ToTensor), bit-identical to
 * Pillow + torch; kh/bh (width: w -> ow) and kv/bv (height: h -> oh) are device copies of the
 * plans (ignored for an axis whose size does not change). */
int unet_resize_plan(int in_size, int out_size, int32_t* coeffs, int32_t* bounds, int* ksize);
int unet_resize_u8(unet_ctx* ctx, const uint8_t* src, int h, int w, float* dst, int oh, int ow,
                   const int32_t* kh, const int32_t* bh, int ksh, const int32_t* kv,
                   const int32_t* bv, int ksv, float divisor, unet_stream_t stream);

/* Training augmentations of the input pipeline (main.py:66-91 build_train_transform), applied to
 * the decoded uint8 planes before unet_resize_u8; bit-identical to the host chain (Pillow's
 * transposes, Image.rotate(angle, NEAREST, expand=False, fillcolor=0), ImageEnhance.Brightness,
 * the NumPy TGCAugment and CLAHE of utils/transforms.py).  csrc/aug.h is the shared host / device
 * source.  The host draws one sample's parameters (same RNG calls as the host chain) and passes
 * them BY VALUE: nothing is uploaded and nothing synchronises. */
typedef enum {
    UNET_ROT_NONE = 0,   /* no rotation (angle % 360 == 0) */
    UNET_ROT_AFFINE = 1, /* Pillow's 16.16 fixed-point nearest affine transform, coefficients a[] */
    UNET_ROT_180 = 2,    /* Image.ROTATE_180 */
    UNET_ROT_90 = 3,     /* Image.ROTATE_90 (counter-clockwise); square planes only */
    UNET_ROT_270 = 4     /* Image.ROTATE_270; square planes only */
} unet_rot_mode;

typedef struct {
    int32_t mode;        /* unet_rot_mode */
    int32_t flip_h;      /* FLIP_LEFT_RIGHT before the rotation (folded into the source index) */
    int32_t flip_v;      /* FLIP_TOP_BOTTOM before the rotation */
    int32_t num_bins;    /* TGC bands (0 = none, at most 64); band i = rows [i bin_h, (i + 1) bin_h),
                            bin_h = h / num_bins; later rows (and bin_h == 0) keep their values */
    int32_t a[6];        /* UNET_ROT_AFFINE: xin = (a[2] + y a[1] + x a[0]) >> 16,
                            yin = (a[5] + y a[4] + x a[3]) >> 16 (int32, arithmetic shift); the
                            pixel is 0 unless 0 <= xin < w and 0 <= yin < h.  |a[0,1,3,4]| <= 2^16,
                            |a[2,5]| <= 3 * 2^28 (UNET_ERR_INVALID otherwise) */
    uint8_t lut[256];    /* brightness table applied to the gathered value (identity = none) */
    float gain[64];      /* TGC: v = (uint8)trunc(min(max(float(v) * gain[band], 0), 255)) */
} unet_aug_params;

/* dst (h, w) <- flip, rotate, brightness table and TGC of src (h, w), uint8, dst != src, one
 * launch.  A mask takes the same call with the identity table and num_bins = 0.  h or w above
 * 8192, or mode 90 / 270 with h != w, is UNET_ERR_SHAPE; num_bins > 64 is UNET_ERR_UNSUPPORTED.
 * unet_augment_u8_host is the HOST twin (host pointers, same source). */
int unet_augment_u8(unet_ctx* ctx, const uint8_t* src, int h, int w, uint8_t* dst,
                    const unet_aug_params* params, unet_stream_t stream);
int unet_augment_u8_host(const uint8_t* src, int h, int w, uint8_t* dst,
                         const unet_aug_params* params);
/* unet_augment_u8 with the reference's SpeckleNoise (utils/transforms.py:45-54) between the
 * brightness table and the TGC gain: noise holds one float64 draw per OUTPUT pixel (h * w, the
 * host's np.random.normal field; device memory for unet_augment_noise_u8, host memory for the
 * _host twin), v = (uint8)trunc(min(max((f + f * noise) * 255.0, 0), 255)), f = float32(v) / 255,
 * the float64 steps rounded one by one.  noise = NULL gives unet_augment_u8's output bit for bit. */
int unet_augment_noise_u8(unet_ctx* ctx, const uint8_t* src, int h, int w, uint8_t* dst,
                          const unet_aug_params* params, const double* noise,
                          unet_stream_t stream);
int unet_augment_noise_u8_host(const uint8_t* src, int h, int w, uint8_t* dst,
                               const unet_aug_params* params, const double* noise);

/* The reference's ElasticDeform (utils/transforms.py:15-42) on the decoded uint8 planes, first in
 * the chain; bit-identical to utils.transforms.gaussian_blur + remap_linear_u8 / remap_nearest
 * (csrc/elastic.h is the shared host / device source).  The host draws alpha, sigma and the two
 * uniform float64 fields (np.random.rand(h, w) twice) and computes the Gaussian taps
 * (utils.transforms.gaussian_kernel); the rest runs here: u = r * 2 - 1, a separable ksize-tap
 * float64 blur with REFLECT_101 borders (rows first, every product and sum rounded on its own),
 * map = (float)(index + blur * alpha), a bilinear gather of the image on 1/32-pixel coordinates
 * with 15-bit integer weights and a nearest gather of the mask, both with BORDER_REFLECT. */
typedef struct {
    int32_t ksize;       /* odd, 1 .. 31 (the reference uses 17) */
    double k[31];        /* the ksize Gaussian taps */
    double alpha;        /* displacement scale, finite */
} unet_elastic_params;

/* img_dst / mask_dst (h, w) <- the deformed img / mask (h, w), uint8, under the one map of the
 * fields rx, ry (h * w float64 each; device memory, read-only).  img or mask may be NULL (that
 * plane is skipped, its destination ignored), not both; a destination must differ from its source.
 * Two launches: the row pass of both fields into a context-owned scratch of 2 h w doubles (grown
 * on demand without a host synchronisation, as for unet_clahe_u8: one stream per context, or
 * ordered streams), then column pass + map + gathers per output pixel.  ksize even, below 1 or
 * above 31, or a non-finite alpha is UNET_ERR_INVALID; a side <= ksize / 2 (REFLECT_101 has
 * nothing to reflect) or above 8192 is UNET_ERR_SHAPE.  unet_elastic_u8_host is the HOST twin
 * (host pointers, same source). */
int unet_elastic_u8(unet_ctx* ctx, const uint8_t* img, const uint8_t* mask, int h, int w,
                    uint8_t* img_dst, uint8_t* mask_dst, const double* rx, const double* ry,
                    const unet_elastic_params* params, unet_stream_t stream);
int unet_elastic_u8_host(const uint8_t* img, const uint8_t* mask, int h, int w, uint8_t* img_dst,
                         uint8_t* mask_dst, const double* rx, const double* ry,
                         const unet_elastic_params* params);

/* dst (h, w) <- CLAHE of src with clip limit `clip` (<= 0: no clipping) and gx x gy tiles along
 * x / y, bit-identical to utils.transforms.clahe_u8(img, clip, (gx, gy)): histograms of the tiles
 * of the plane padded bottom / right with REFLECT_101 to whole tiles, clipped at
 * max((int)(clip * area / 256), 1) with the excess redistributed, one table per tile, float32
 * bilinear blend of the four neighbouring tables.  gx * gy > 256 is UNET_ERR_UNSUPPORTED; a
 * padding larger than the axis can reflect (pad > n - 1) or a side above 8192 is UNET_ERR_SHAPE.
 * The tile histograms and tables live in a context-owned scratch grown on demand without a host
 * synchronisation, so issue a context's CLAHE calls on one stream, or order the streams.
 * unet_clahe_u8_host is the HOST twin. */
int unet_clahe_u8(unet_ctx* ctx, const uint8_t* src, int h, int w, uint8_t* dst, double clip,
                  int gx, int gy, unet_stream_t stream);
int unet_clahe_u8_host(const uint8_t* src, int h, int w, uint8_t* dst, double clip, int gx,
                       int gy);

/* Predict-mode export (csrc/export.h holds the rules; no reference counterpart beyond the contour
 * plot of utils/trainer.py:262-299, which this replaces without matplotlib or scikit-image).
 *
 * unet_resize_f32_plan (host only): Pillow's BILINEAR plan of one axis in_size -> out_size for
 * mode "F" images: coeffs [out_size][*ksize] doubles and bounds [out_size] {first, count}, the
 * layout of unet_resize_plan.  coeffs / bounds NULL: *ksize alone.
 *
 * unet_resize_f32_mask: plane (oh, ow) <- the float32 plane src (h, w) resized as
 * Image.fromarray(src, "F").resize((ow, oh), BILINEAR) does, bit for bit (double accumulation of
 * float pixel x double tap, product and sum rounded separately; the horizontal pass first into a
 * float32 intermediate; an unchanged axis skipped), and mask (oh, ow) uint8 in {0, 1} <- its
 * threshold: kind UNET_EXPORT_SIGMOID_HALF: sigmoid(v) > 0.5f as unet_mask_counts reads it (thr
 * ignored); UNET_EXPORT_GREATER: v > thr.  plane may be NULL (the resized plane then never reaches
 * memory beyond the intermediate).  kh / bh / ksh: the plan w -> ow, kv / bv / ksv: h -> oh (device
 * memory; an unchanged axis needs none).  The intermediate lives in a context-owned scratch grown
 * on demand without a host synchronisation (the outgrown buffer is kept until unet_destroy): issue
 * a context's calls on one stream, or order the streams.  A non-positive size or an unknown kind
 * is UNET_ERR_INVALID.
 *
 * unet_overlay_u8: rgb (h, w, 3) interleaved bytes <- the gray plane (h, w) with the prediction
 * mask pred (h, w; nonzero = foreground) tinted at alpha in 0..256 (0: none) inside and its contour
 * of width r in 1..3 (foreground pixels with a background or outside pixel at city-block distance
 * <= r) solid red on top of the solid blue contour of gt (h, w), which may be NULL.  stats:
 * int64[6] = {area, contour pixels, x0, y0, x1, y1} of pred (inclusive box; an empty mask gives
 * 0, 0, -1, -1, -1, -1), overwritten.  r or alpha outside its range, or a non-positive size, is
 * UNET_ERR_INVALID.  The _host functions are the HOST twins (host pointers, same source). */
enum { UNET_EXPORT_SIGMOID_HALF = 0, UNET_EXPORT_GREATER = 1 };
int unet_resize_f32_plan(int in_size, int out_size, double* coeffs, int32_t* bounds, int* ksize);
int unet_resize_f32_mask(unet_ctx* ctx, const float* src, int h, int w, int oh, int ow,
                         const double* kh, const int32_t* bh, int ksh, const double* kv,
                         const int32_t* bv, int ksv, int kind, float thr, float* plane,
                         uint8_t* mask, unet_stream_t stream);
int unet_resize_f32_mask_host(const float* src, int h, int w, int oh, int ow, const double* kh,
                              const int32_t* bh, int ksh, const double* kv, const int32_t* bv,
                              int ksv, int kind, float thr, float* plane, uint8_t* mask);
int unet_overlay_u8(unet_ctx* ctx, const uint8_t* gray, const uint8_t* pred, const uint8_t* gt,
                    int h, int w, int r, int alpha, uint8_t* rgb, int64_t* stats,
                    unet_stream_t stream);
int unet_overlay_u8_host(const uint8_t* gray, const uint8_t* pred, const uint8_t* gt, int h, int w,
                         int r, int alpha, uint8_t* rgb, int64_t* stats);

/* Kernel-schedule options of a context (new; no reference counterpart).  The defaults are
 * the measured-best schedules; the named alternatives (tiles, LDS-DMA vs register-staged
 * bf16 kernels, XCD block order, ...) exist for A/B runs and the bit-identity tests.  The
 * library never reads the environment: an option changes only when set here.
 * Names (runtime.hip OPTION_TABLE, in this order; unet_option_name enumerates them):
 *   wgrad_row3 wgrad_row3_tile wgrad_row3_big wgrad_row3_blocks wgrad_row3_n32 wgrad_blocks
 *   wgrad16_blocks wgrad_tile_w wgrad_tile_n tile_n128 tile_n128_dgrad tile_n64 tile_n64_dgrad
 *   tile_n32 tile_convt64 tile_convt tile_convt_dgrad rg16 rg16_tile rg16_bn_k rg16_r3 rg16_n128
 *   rg16_n128_bn wg16 wg16_tile wg16_r3 convt16 wg16t xcd16 xcd_remap dz_in_wgrad x3 x3_tile
 *   x3_wtile x3_wblocks x3_n64 x3_r3 head_fuse pool_fuse x3_wwaves x3_wwaves1 tile_group
 *   cc_tile morph_lds echo_agg
 * Set them between steps, not between a forward and its backward: the workspace plan and
 * which saved images exist depend on them (x3, convt16, the bf16 kernel choices, ...), so
 * unet_backward returns UNET_ERR_INVALID when any option differs from those of the training
 * unet_forward that last ran on its workspace (or when none did; the context remembers the
 * 64 most recent such workspaces). */
int unet_set_option(unet_ctx* ctx, const char* name, int64_t value);
int unet_get_option(const unet_ctx* ctx, const char* name, int64_t* value);
/* i-th option name (0 ..), UNET_ERR_INVALID past the last one; *name is static. */
int unet_option_name(int i, const char** name);

/* Per-kernel timing: when enabled, unet_forward/unet_backward bracket every launch with
 * HIP events; unet_timing_read synchronises and returns, per kernel family, the launch
 * count, total ms and algorithmic FLOP of the last call(s) since the last reset. */
int unet_timing_enable(unet_ctx* ctx, int enable);
/* Time only the launches whose label ("family/kernel|layer") contains `substring`
 * (NULL or "" = every launch): keeps the event overhead off the rest of the step. */
int unet_timing_filter(unet_ctx* ctx, const char* substring);
int unet_timing_reset(unet_ctx* ctx);
int unet_timing_count(unet_ctx* ctx, int* n_families);
int unet_timing_read(unet_ctx* ctx, int i, const char** family, int64_t* launches,
                     double* total_ms, double* flop);

/* Debug/test view into a workspace: byte offset of an intermediate tensor.
 * kind: 0 y[i] (post-ReLU conv output, NHWC, channel stride *ld, channel offset *off),
 *       1 BN scale[i], 2 BN shift[i], 3 BN batch mean[i], 4 BN invstd[i],
 *       5 pooled[l] (NHWC dense; not written when the next conv runs on the x3 kernels:
 *       the max-pool then stores that conv's x3 operand image instead), 6 concat buffer[l]
 *       (NHWC, 2*64<<l channels),
 *       7 d(concat)[l] of the last backward, 8 max-pool winner index[l] (uint8 NHWC dense,
 *       window position 0..3 in torch's scan order), 9 (ResUNet only) out[b], the stored output
 *       ReLU(BN2(z2) + skip(x)) of residual block b = 0 .. 2 depth (encoders, bottleneck,
 *       decoders; NHWC, channel stride *ld, channel offset *off: an encoder's lives in the skip
 *       half of its concat buffer).  *count = elements (pixels*ld for NHWC). */
int unet_debug_view(unet_ctx* ctx, int N, int H, int W, int training, int kind, int index,
                    int64_t* byte_offset, int64_t* count, int* ld, int* off);

/* Test hooks of the exact three-way bf16 split the x3 GEMMs use (csrc/x3_split.h; no
 * reference counterpart).  n f32 values (n a multiple of 32) become the x3 image the kernels
 * stream, bf16 bit patterns [n / 32][3][32]: for v = v[32 r + j], out[96 r + j] = h,
 * out[96 r + 32 + j] = m, out[96 r + 64 + j] = l, with v = h + m + l exactly for normal and
 * huge finite v; +-inf / NaN keep h = v, m = l = 0.  unet_x3_split_host runs the shared source on the host (bit-level RNE);
 * unet_x3_split_device runs the device pass (to_x3_kernel, hardware bf16 conversion) on n
 * device floats into a device buffer, enqueued on `stream`. */
int unet_x3_split_host(const float* v, int64_t n, uint16_t* out);
int unet_x3_split_device(unet_ctx* ctx, const float* v, int64_t n, uint16_t* out,
                         unet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H */
