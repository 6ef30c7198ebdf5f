// What the two translation units behind include/unet_hip.h share: the context (unet_ctx with
// its layer tables, options, timing records and scratch buffers), the error / exception guards
// of the C ABI and the launch bookkeeping.  runtime.hip holds the network (graph, plan, forward,
// backward, AdamW), ops_abi.hip the stand-alone entry points (losses, metrics, augmentations).
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/unet_hip.h"
#include "kernels_misc.h"

constexpr int MAX_DEPTH = 6;

// A parameter tensor.  shape / off / numel describe the torch tensor in the caller's flat
// arena (what unet_param_info reports); poff / pshape the same tensor in the context's
// channel-padded arena (== the torch layout unless the network is padded, see
// unet_ctx::padded).  Padded dims are segmented: dim k holds nseg[k] segments of seg[k]
// real entries, each padded to pseg[k] (2 segments for a concat input [skip | up]).
struct ParamT {
    std::string name;
    int ndim;
    int64_t shape[4];
    int64_t off, numel;
    int stage;           // backward stage after which its gradient is final
    int64_t poff, pnumel;
    int64_t seg[4], pseg[4], nseg[4];
};

struct ConvL {
    int cin, cout, level, block, which;
    int64_t w, b;        // param offsets (b < 0: bias-free conv)
    int64_t pf, pd;      // packed weight offsets (floats) inside the pack region
};
struct BnL {
    int C;               // channels the kernels see (padded)
    int rC;              // channels of the torch module (running stats, gamma, beta)
    int64_t g, b;        // gamma / beta offsets in the (padded) parameter arena
    int64_t run;         // running_mean offset in the (padded) bn arena (var at run + C)
    int64_t rrun;        // ... in the caller's bn arena (var at rrun + rC)
    std::string name;
};
struct ConvTL {
    int cin, cout, in_level;
    int64_t w, b;
    int64_t pf, pd;
};

struct TimeRec {
    std::string label;
    hipEvent_t a, b;
    double flop;
};

// Kernel-schedule options of one context (unet_set_option).  The defaults are the
// measured-best schedules; the alternatives exist for A/B runs and tests and are chosen
// explicitly through the ABI (never from the environment).  None of them changes the
// numerics except where noted as bit-identical alternatives in DESIGN.md.
struct Options {
    int wgrad_row3 = 1;        // f32 3x3 wgrad on the one-row-of-taps kernel: 0 never,
                               // 1 every eligible layer (default: r02 A/B, conv wgrad
                               // 27.1 -> 24.4 ms/step), 2 layers with a 64-channel operand
    int wgrad_row3_tile = -1;  // its tile (a WG3_* id), -1 = by channel counts
    int wgrad_blocks = 2048;       // split-K target (blocks) of the one-tap f32 weight gradients
    int rg16_bn_k = 0;             // rg16: E_STORE_BN GEMMs with K below this take the 128x128 tile
                                   // (8192 until the one-barrier halo kernel, r04: 0 is 1-1.5 %
                                   // faster on config 4, profiles/r04_c4_barrier_ab.txt)
    int wgrad16_blocks = 1536;     // split-K target (blocks) of the bf16 weight gradients
                                   // (config 4 A/B: 1536 +1.4 % over 2048, 1024 -4.7 %)
    int wgrad_row3_big = WG3_128x64;  // row3 tile where Cin, Cout % 128 == 0 (-1 = WG3_128x128)
    int wgrad_row3_n32 = 1;        // row3 weight gradients for 32-channel operands too (WG3_32x32 ..,
                                   // one / two waves: the split-K target counts four-wave blocks)
    int wgrad_row3_blocks = 1536;  // split-K target (blocks) of the row3 weight gradients
                                   // (r02 sweep 512..2048: 1536 best, 391 vs 386 img/s)
    int wgrad_tile_w = WG_128x128;  // f32 wgrad tile, both channel counts multiples of 128
    int wgrad_tile_n = WG_64x64;    // ... 64-channel layers (3 waves/SIMD)
    int tile_n128 = -1;        // f32 row-GEMM tile, N % 128 == 0 (-1 = pick_tile's default)
    int tile_n128_dgrad = -1;  // ... dgrad-type
    int tile_n64 = RG_P128x64;  // ... N = 64 outputs (forward-type)
    int tile_n64_dgrad = RG_P3_128x64;  // ... N = 64, dgrad-type (pipelined 128x64 at three blocks per
                               // CU: level-0 dgrads 1.50-1.55 -> 1.40-1.45 ms, r03)
    int tile_convt64 = RG_128x64;  // ConvT forward with 64 output channels (grid N = 256)
    int tile_n32 = RG_256x32G;  // f32 row GEMMs with 32 outputs: 256 x 32 with operands
                               // straight from global memory (r04, ResUNet(32, 4) 263 -> 282
                               // img/s, (16, 4) 419 -> 478), or RG_256x32, the LDS-staged one
    int tile_convt = -1;       // ConvT forward, >= 128 output channels (-1 = tile_n128's)
    int tile_convt_dgrad = RG_P3_128x64A;  // ConvT input gradient (-1 = tile_n128_dgrad's; pipelined
                               // 128x64 at three blocks per CU: the K = 4 Cout short-K GEMMs
                               // with their BN-partials epilogue, 1.33 -> 1.15 ms per step)
    int rg16 = 1;              // bf16 row GEMMs on the LDS-DMA kernel (0: register-staged)
    int rg16_tile = -1;        // its tile (-1 = per GEMM, rg16_pick())
    int rg16_n128 = R16_H512x128;  // rg16 tile of the GEMMs whose N is not a multiple of 256 (the
                               // 128-output layers; -1 = 128x128, 6 = 512x128, 20 = 512x128 tap-row
                               // halo for 3x3 convs, 6 elsewhere; r04 config 4: 122.7 -> 124.8
                               // img/s with 20, 121.9 with 6)
    int rg16_n128_bn = 0;      // ... also for the short-K E_STORE_BN GEMMs (else 128x128)
    int rg16_r3 = 1;           // 256x256 3x3-conv GEMMs (W >= 16) on the tap-row halo kernel (R16_H256x256;
                               // config 4: +0.9..1.2 % over three A/B pairs, r03)
    int wg16 = 1;              // bf16 3x3 wgrad on the LDS-DMA transposed-read kernel
    int wg16_tile = W16_256x256;  // its tile
    int convt16 = 1;           // bf16 training: the ConvT forward stores the up half of the
                               // decoder's concat straight into that conv's bf16 operand image
                               // (no f32 up half; its prep pass converts the skip half only)
    int wg16_r3 = W16_R3M;     // 3x3 layers with W % 64 == 0 on the tap-row bf16 weight gradient:
                               // 7 = 16x16x32 MFMAs with the re-read stagger (r06, config 4
                               // +1.3 % over 4, profiles/r06_c4_wg16_ab.txt; also at W = 32 / 16,
                               // +1.4 %, r06_c4_deep_wgrad_ab.txt), 4 = 32x32x16, four LDS stages
                               // (r04: 122.7 -> 125.2 img/s), 0 = off (one-tap kernel)
    int wg16t = 1;             // bf16 ConvT wgrad on the same kernel
    int xcd16 = 1;             // XCD-contiguous block order, LDS-DMA kernels
    int xcd_remap = 1;         // ... f32 GEMMs: 0 none, 1 both (default: r03 PMC, HBM bytes
                               // per launch rowgemm 128x128 2.21 -> 1.00 GB, row3 wgrad
                               // 2.02 -> 0.97 GB at equal time), 2 row GEMMs, 3 wgrad
    int dz_in_wgrad = 256;     // layers with Cin <= this form the BN-backward dz in the weight
                               // gradient's B' loader, which also stores it for the dgrad (no
                               // bn_dz pass; f32, both BN orders since r04; 0 = off).  Every A'-tile row of
                               // blocks re-reads do and y instead of dz, so the fusion pays
                               // where few A' tiles share a pixel slice (profiles/
                               // r03_tile_experiments.txt: Cin 64..256 gain, 512..1024 lose)
    int x3 = 1;                // f32 math: conv / ConvT GEMMs whose channel counts are multiples
                               // of 64 on the bf16 matrix cores through exact three-way operand
                               // splits (kernels_gemm_x3.hip; fp64 error below the f32 MFMA
                               // kernels'); 0 = the f32 MFMA kernels everywhere
    int x3_tile = -1;          // its row-GEMM tile (-1 = x3_pick())
    int x3_wtile = -1;         // its weight-gradient tile (-1 = by channel counts)
    int x3_wblocks = 1536;     // split-K target (blocks) of its 128x128 weight gradients
    int x3_n64 = X3_128x64;    // its row-GEMM tile for 64 outputs (or X3_256x64)
    int x3_r3 = 1;             // its 256x128 3x3 GEMMs on the tap-row halo kernel (tile 4)
    int x3_wwaves = 3;         // tap-row x3 weight gradients: split-K so the grid is this many full
                               // waves of block slots (0 = the x3_wblocks target; r05,
                               // profiles/r05_wwaves_ab.txt)
    int x3_wwaves1 = 3;        // the same for the one-tap x3 weight gradients (ConvT, 8x8):
                               // +0.45 % (profiles/r05_wwaves_ab.txt)
    int pool_fuse = 1;         // x3 and (r06) bf16 paths: the encoder block's second conv recomputes its `do` from
                               // the max-pool backward's inputs instead of maxpool_bwd storing it
    int head_fuse = 1;         // x3 (r05) and bf16 (r06) paths, one output channel: the last conv's dz
                               // pass recomputes `do` from the head instead of head_bwd storing it
    int tile_group = 1;        // (r06) row-GEMM tile order of the LDS-DMA kernels (rg16, x3): 1 = grouped
                               // where the N tiles are many (tile_group_auto), 0 = M-major (r05);
                               // bit-identical
    int cc_tile = 1;           // connected components: tile rows (0 = 16, 1 = 32, 2 = 64; 64 columns);
                               // same labels for every value (profiles/cc_time.txt)
    int morph_lds = 1;         // lesion morphometry: the reduce pass aggregates per block in an LDS table
                               // (0 = every run straight to global atomics; same table either way,
                               // profiles/morph_time.txt)
    int echo_agg = 0;          // lesion echogenicity: 1 = every LDS add is first aggregated over the wave
                               // (0 = one LDS atomic per lane, which measured faster on every
                               // input; same table either way, profiles/echo_time.txt)
};

// A device buffer one feature's entry points own through the context, grown on demand (grow):
// one per feature, since two features' work may be in flight together.
struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
};

struct unet_ctx {
    int device = 0;
    int cus = 256;  // compute units of the device (split-K sizing by whole waves of block slots)
    int in_ch = 1, out_ch = 1;
    int variant = UNET_VARIANT_MODEL;
    int base = 64, depth = 4;  // base: channels of level 0 as the kernels see them (padded)
    int rbase = 64;            // base_filters of the reference module (models/mod.py:13)
    // Narrow networks (base_filters 16 / 24 / 32 / 48 of the reference's model grid,
    // config/config.yaml) run with every level's channels zero-padded to the next power of
    // two >= 64, the widths the GEMM tiles and channel-quad kernels are built for.  The
    // caller's arenas keep the torch layouts; unet_forward / unet_backward expand them
    // into padded arenas in the workspace (zeros in the padding: zero weights, gamma,
    // beta, so padded channels stay exactly 0 through BN / ReLU / pooling / ConvT / the
    // head and add +0 to every real sum) and compact the running stats and gradients back.
    bool padded = false;
    bool bn_relu = false;    // BN -> ReLU (mod.py) instead of ReLU -> BN (model.py)
    bool skip_first = false; // concat [skip, up] (mod.py) instead of [up, skip] (model.py)
    bool bf16 = false;       // conv GEMMs on bf16 MFMA (f32 accumulate), BASELINE config 4
    bool res = false;        // residual blocks (mod.py:ResUNet): block outputs materialised
    std::vector<ParamT> params;
    int64_t n_param_floats = 0;   // caller's (torch-layout) arena
    int64_t n_pparam_floats = 0;  // padded arena (== n_param_floats unless padded)
    std::vector<ConvL> conv;
    std::vector<BnL> bn;
    std::vector<ConvTL> convt;
    std::vector<int64_t> skip_w, skip_pd;  // per block: 1x1 skip weight, its dgrad image
    std::vector<int64_t> skip_pf;          // bf16 math: its plain bf16 image (skip_pd: bf16 too)
    int64_t head_w = 0, head_b = 0;
    int64_t n_bn_floats = 0;      // caller's running-stat arena
    int64_t n_pbn_floats = 0;     // padded
    int64_t pack_floats = 0;
    std::vector<PadDesc> pad_params, pad_bn;  // expand / compact tables (padded only)
    int64_t pad_max_numel = 0, pad_bn_max = 0;
    int cmax = 0;
    std::string err;
    // buckets (DP overlap): contiguous grad ranges, ready after backward stage bucket_stage
    std::vector<int64_t> bucket_off, bucket_len;
    std::vector<int> bucket_stage;
    std::vector<int> bucket_p0, bucket_p1;     // parameter tensors [p0, p1) of each bucket
    std::vector<int64_t> bucket_pmax;          // ... their largest padded numel
    std::vector<hipEvent_t> bucket_ev;
    // timing
    bool timing = false;
    std::string tfilter;  // time only launches whose label contains this (empty = all)
    std::vector<TimeRec> trec;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    Options opt;
    // what unet_backward must know about the training forward it completes, kept per forward
    // (keyed by its workspace: one context serves every model of its configuration on the
    // device, and their forwards and backwards interleave).  A host-side table, not a header
    // in the workspace itself: reading device memory back would cost a synchronisation.
    //  * opt: the workspace plan and which saved images exist (x3, convt16, the bf16 kernels,
    //    ...) depend on the options, so the backward refuses to run under different ones (it
    //    would read saved activations at shifted offsets, or an up half the forward never wrote)
    //  * used_pp / pp_gen: whether the forward read the context's weight images instead of
    //    packing into its workspace, and their generation then
    struct FwdRec {
        const void* ws;
        Options opt;
        bool used_pp;
        uint64_t pp_gen;
        uint64_t seq;
    };
    static constexpr size_t MAX_FWD_RECS = 64;  // forwards awaiting a backward; the oldest leaves
    std::vector<FwdRec> fwd_recs;
    uint64_t fwd_seq = 0;
    // (r06) weight images written by unet_adamw_repack (AdamW fused into the repack): device
    // buffers owned by the context, valid (pp_ok) for the parameter arena
    // [pp_src, pp_src + n_param_floats) under the options they were written with, until that
    // arena is written otherwise (unet_arena_changed, unet_adamw on an overlapping range,
    // unet_params_changed), an option changes, or another repack.  pp_gen counts repacks: the
    // images a forward read stay usable by its backward for as long as the generation stands,
    // whether or not pp_ok was cleared in between (clearing it rewrites nothing).
    float* pp = nullptr;
    uint16_t* pp3 = nullptr;
    const float* pp_src = nullptr;
    bool pp_ok = false;
    uint64_t pp_gen = 0;
    // Scratch of the stand-alone entry points (ops_abi.hip), grown without a host
    // synchronisation: work in flight may still read an outgrown buffer, so it is retired,
    // not freed, until unet_destroy.
    Scratch loss;      // unet_loss_stats: 4 floats per chunk
    Scratch boundary;  // unet_edt: any-site flags + g^2; unet_boundary_fwd: chunk sums
    Scratch clahe;     // unet_clahe_u8: tile histograms + tables
    Scratch elastic;   // unet_elastic_u8: the row pass of both fields
    Scratch surface;   // unet_surface_stats: border planes, squared distances, gather partials
    Scratch cc;        // unet_components / _postprocess / _lesion_stats: labels, areas and flags, counts
    Scratch curve;     // unet_curve_stats: the planes' dice_k before their ordered sum
    Scratch exportbuf; // unet_resize_f32_mask: the float32 intermediate of the horizontal pass
    Scratch lovasz;    // unet_lovasz_fwd: the sort's key / word buffers, histograms, tile sums
    Scratch morph;     // unet_morphometry: row offsets and row extents of the components
    std::vector<void*> retired;

    int nconv() const { return (int)conv.size(); }
    int chl[MAX_DEPTH + 1] = {};                           // kernel (padded) channels per level
    int ch(int level) const { return chl[level]; }         // kernel (padded) channels
    int rch(int level) const { return rbase << level; }   // torch module channels
    int up_off(int l) const { return skip_first ? ch(l) : 0; }    // CAT_l channel offsets
    int skip_off(int l) const { return skip_first ? 0 : ch(l); }
};

namespace {

int fail(unet_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) {
        try {
            c->err = buf;
        } catch (...) {  // out of memory for the message itself: keep the code
        }
    }
    return code;
}

// Every extern "C" entry runs its body inside ABI_TRY / ABI_CATCH(ctx): no C++ exception
// (std::bad_alloc from the graph / plan / timing containers, ...) unwinds into the caller.
#define ABI_TRY try {
#define ABI_CATCH(ctx)                                                                      \
    }                                                                                       \
    catch (const std::bad_alloc&) {                                                         \
        return fail(const_cast<unet_ctx*>(ctx), UNET_ERR_NOMEM, "out of host memory");       \
    }                                                                                       \
    catch (const std::exception& e_) {                                                      \
        return fail(const_cast<unet_ctx*>(ctx), UNET_ERR_INTERNAL, "internal error: %s",     \
                    e_.what());                                                             \
    }                                                                                       \
    catch (...) {                                                                           \
        return fail(const_cast<unet_ctx*>(ctx), UNET_ERR_INTERNAL, "internal error");        \
    }

// The same guard for a host twin, which has no context to carry a message: runs body (its
// temporaries may not fit in host memory) and turns what it throws into the status code.
template <class F>
int catch_to_status(F&& body) {
    try {
        body();
        return UNET_OK;
    } catch (const std::bad_alloc&) {
        return UNET_ERR_NOMEM;
    } catch (...) {
        return UNET_ERR_INTERNAL;
    }
}

// The tail of an entry point that launches directly, untimed: r is what the k_ launcher returned.
inline int launched(unet_ctx* c, const char* name, int r) {
    return r ? fail(c, UNET_ERR_HIP, "%s launch %d", name, r) : UNET_OK;
}

// At least `bytes` in sc; returns at once when it has them.  Never synchronises and never frees:
// the outgrown buffer joins c->retired (see unet_ctx::loss).
inline int grow(unet_ctx* c, Scratch& sc, size_t bytes, const char* what) {
    if (bytes <= sc.bytes) return UNET_OK;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, UNET_ERR_HIP, "hipSetDevice");
    if (sc.p) c->retired.reserve(c->retired.size() + 1);  // so the push_back below cannot throw
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess)
        return fail(c, UNET_ERR_HIP, "hipMalloc: %s scratch: %zu bytes", what, bytes);
    if (sc.p) c->retired.push_back(sc.p);
    sc.p = p;
    sc.bytes = bytes;
    return UNET_OK;
}

inline AdamwScalars adamw_scalars(int step, double lr, double b1, double b2, double eps, double wd,
                                  double gscale) {
    // torch optim/adam.py _single_tensor_adam: every scalar is a Python float (double)
    // that ATen rounds to float once when it meets the fp32 tensor
    AdamwScalars a;
    a.decay = (float)(1.0 - lr * wd);                 // param.mul_(1 - lr * weight_decay)
    a.w1 = (float)(1.0 - b1);                         // exp_avg.lerp_(grad, 1 - beta1)
    a.lerp_small = fabs(1.0 - b1) < 0.5 ? 1 : 0;
    a.b2 = (float)b2;                                 // exp_avg_sq.mul_(beta2)
    a.w2 = (float)(1.0 - b2);                         // .addcmul_(grad, grad, value=1 - beta2)
    const double bc1 = 1.0 - pow(b1, (double)step);   // beta1 ** step (Python float pow)
    const double bc2 = 1.0 - pow(b2, (double)step);
    a.neg_step = (float)(-(lr / bc1));                // addcdiv_(..., value=-step_size)
    a.bc2_sqrt = (float)pow(bc2, 0.5);                // bias_correction2 ** 0.5
    a.eps = (float)eps;                               // .add_(eps)
    a.gscale = (float)gscale;
    return a;
}

// launch bookkeeping (optional per-launch HIP-event timing)
struct Launcher {
    unet_ctx* c;
    hipStream_t s;
    hipEvent_t ev() {
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            c->ev_pool.push_back(e);
        }
        return c->ev_pool[c->ev_used++];
    }
    template <class F>
    int run(const std::string& label, double flop, F&& f) {
        hipEvent_t a = nullptr, b = nullptr;
        const bool timed = c->timing && (c->tfilter.empty() || label.find(c->tfilter) != std::string::npos);
        if (timed) {
            a = ev();
            b = ev();
            (void)hipEventRecord(a, s);
        }
        int r = f();
        if (r != 0) return fail(c, UNET_ERR_HIP, "%s: launch failed (%d: %s)", label.c_str(), r,
                                r > 0 ? hipGetErrorString((hipError_t)r) : "bad shape");
        if (timed) {
            (void)hipEventRecord(b, s);
            c->trec.push_back(TimeRec{label, a, b, flop});
        }
        return 0;
    }
};

}  // namespace
