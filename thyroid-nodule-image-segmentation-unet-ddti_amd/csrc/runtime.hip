// Native runtime behind include/unet_hip.h: the layer graph of the reference UNets
// (models/model.py:UNet and models/mod.py:UNet), the workspace plan (NHWC activations,
// zero-copy concat buffers, packed weights, backward scratch), the per-layer routes (which kernel
// family runs each GEMM and who writes its operand image: make_routes, decided once per plan)
// and the forward / backward / optimizer orchestration on one HIP stream, every GEMM described
// and launched through run_rowgemm / run_wgrad.  The context itself is in runtime_internal.h; the
// entry points that need no graph or plan (losses, metrics, augmentations) are in ops_abi.hip.
//
// Both reference networks are the same encoder / bottleneck / decoder topology over
// depth D levels of C_l = base << l channels:
//   block l < D      encoder at level l          (model.py encoder{l+1}; mod.py encoders.l)
//   block D          bottleneck at level D       (model.py middle.1;     mod.py bottleneck)
//   block D+1+j      decoder at level D-1-j      (model.py decoder*/final.0; mod.py decoders.j)
//   ConvT k          level D-k -> D-k-1, reads block D+k's output, feeds block D+1+k through
//                    the concat CAT_{D-k-1}      (model.py middle.2/decoder*.1; mod.py upconvs.k)
// and they differ in the order inside a block (model.py:36-41 Conv(+bias) -> ReLU -> BN;
// mod.py:45-50 Conv(no bias) -> BN -> ReLU), the concat order (model.py:64 [up, skip];
// mod.py:64 [skip, up]) and the parameter names / registration order.  mod.py:ResUNet
// (:71-131) has the same skeleton with residual blocks ReLU(conv(x) + skip(x)): there the
// block output is materialised by the 1x1 skip GEMM's epilogue (E_RESID) and every
// consumer reads it plainly.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include "dz_pass.h"
#include "runtime_internal.h"

namespace {

constexpr float BN_EPS = 1e-5f;       // nn.BatchNorm2d default (models/model.py:38,41)
constexpr float BN_MOMENTUM = 0.1f;   // nn.BatchNorm2d default
constexpr int RED_G = 512;            // first-level blocks of the channel reductions
constexpr int WIDE_G = 2048;          // ... of the level-0 bandwidth passes (more loads in flight)
// blocks of a channel-reduction pass over P pixels: RED_G, up to WIDE_G on large levels (the
// partial buffers hold P/64 + 1 rows: p.stats / p.part per conv of the level, p.hpart WIDE_G)
inline int wide_g(int64_t P) { return (int)std::min<int64_t>(WIDE_G, std::max<int64_t>(RED_G, P / 64)); }
constexpr int STAT_G = 256;           // second level of the BN-stat reduction

struct OptionDesc {
    const char* name;
    int Options::*field;
};
// (include/unet_hip.h lists these names; tests/test_lib_cpu.py checks the two agree)
const OptionDesc OPTION_TABLE[] = {
    {"wgrad_row3", &Options::wgrad_row3},
    {"wgrad_row3_tile", &Options::wgrad_row3_tile},
    {"wgrad_row3_big", &Options::wgrad_row3_big},
    {"wgrad_row3_blocks", &Options::wgrad_row3_blocks},
    {"wgrad_row3_n32", &Options::wgrad_row3_n32},
    {"wgrad_blocks", &Options::wgrad_blocks},
    {"wgrad16_blocks", &Options::wgrad16_blocks},
    {"wgrad_tile_w", &Options::wgrad_tile_w},
    {"wgrad_tile_n", &Options::wgrad_tile_n},
    {"tile_n128", &Options::tile_n128},
    {"tile_n128_dgrad", &Options::tile_n128_dgrad},
    {"tile_n64", &Options::tile_n64},
    {"tile_n64_dgrad", &Options::tile_n64_dgrad},
    {"tile_n32", &Options::tile_n32},
    {"tile_convt64", &Options::tile_convt64},
    {"tile_convt", &Options::tile_convt},
    {"tile_convt_dgrad", &Options::tile_convt_dgrad},
    {"rg16", &Options::rg16},
    {"rg16_tile", &Options::rg16_tile},
    {"rg16_bn_k", &Options::rg16_bn_k},
    {"rg16_r3", &Options::rg16_r3},
    {"rg16_n128", &Options::rg16_n128},
    {"rg16_n128_bn", &Options::rg16_n128_bn},
    {"wg16", &Options::wg16},
    {"wg16_tile", &Options::wg16_tile},
    {"wg16_r3", &Options::wg16_r3},
    {"convt16", &Options::convt16},
    {"wg16t", &Options::wg16t},
    {"xcd16", &Options::xcd16},
    {"xcd_remap", &Options::xcd_remap},
    {"dz_in_wgrad", &Options::dz_in_wgrad},
    {"x3", &Options::x3},
    {"x3_tile", &Options::x3_tile},
    {"x3_wtile", &Options::x3_wtile},
    {"x3_wblocks", &Options::x3_wblocks},
    {"x3_n64", &Options::x3_n64},
    {"x3_r3", &Options::x3_r3},
    {"head_fuse", &Options::head_fuse},
    {"pool_fuse", &Options::pool_fuse},
    {"x3_wwaves", &Options::x3_wwaves},
    {"x3_wwaves1", &Options::x3_wwaves1},
    {"tile_group", &Options::tile_group},
    {"cc_tile", &Options::cc_tile},
    {"morph_lds", &Options::morph_lds},
    {"echo_agg", &Options::echo_agg},
};

// Parameter table in the reference's named_parameters() order, layer tables, packing
// offsets and gradient buckets.
// One dimension of a parameter tensor: nseg segments of seg real entries, each padded to
// pseg entries (nseg = 2 for the [skip | up] concat input of a decoder block).
struct Dim {
    int64_t seg, pseg, nseg;
};

void build_graph(unet_ctx* c) {
    const int D = c->depth;
    const int nb = 2 * D + 1;
    c->conv.assign(2 * nb, ConvL{});
    c->bn.assign(2 * nb, BnL{});
    c->convt.assign(D, ConvTL{});
    c->params.clear();
    int64_t off = 0, poff = 0;
    // returns the tensor's offset in the padded arena (what the kernels index)
    auto add = [&](const std::string& name, std::initializer_list<Dim> dims, int stage) {
        ParamT p;
        p.name = name;
        p.ndim = (int)dims.size();
        p.numel = 1;
        p.pnumel = 1;
        int i = 0;
        for (const Dim& d : dims) {
            p.shape[i] = d.seg * d.nseg;
            p.seg[i] = d.seg;
            p.pseg[i] = d.pseg;
            p.nseg[i] = d.nseg;
            p.numel *= d.seg * d.nseg;
            p.pnumel *= d.pseg * d.nseg;
            ++i;
        }
        for (; i < 4; ++i) {
            p.shape[i] = 0;
            p.seg[i] = p.pseg[i] = p.nseg[i] = 1;
        }
        p.off = off;
        p.poff = poff;
        p.stage = stage;
        off += p.numel;
        poff += p.pnumel;
        c->params.push_back(p);
        return p.poff;
    };
    auto level_of = [&](int b) { return b <= D ? b : 2 * D - b; };
    auto lvl = [&](int l) { return Dim{c->rch(l), c->ch(l), 1}; };  // one level's channels
    auto block_cin = [&](int b) {  // kernel (padded) input channels of block b
        if (b == 0) return c->in_ch;
        if (b <= D) return c->ch(b - 1);
        return 2 * c->ch(level_of(b));
    };
    auto block_in_dim = [&](int b) {  // the same as a torch dimension
        if (b == 0) return Dim{c->in_ch, c->in_ch, 1};
        if (b <= D) return lvl(b - 1);
        return Dim{c->rch(level_of(b)), c->ch(level_of(b)), 2};  // concat of two halves
    };
    const Dim k3{3, 3, 1}, k2{2, 2, 1}, k1{1, 1, 1};
    // backward stage after which a block's gradients are final: 0 = head + last decoder,
    // then ConvT k together with block D+k (k = D-1 .. 0), then the encoders
    auto stage_of_block = [&](int b) { return 2 * D - b; };
    // 3x3 conv + BN pair `which` of block b; names per variant
    auto conv_pair = [&](int b, int which, const std::string& pfx) {
        const int i = 2 * b + which;
        ConvL& L = c->conv[i];
        L.cout = c->ch(level_of(b));
        L.cin = which == 0 ? block_cin(b) : L.cout;
        L.level = level_of(b);
        L.block = b;
        L.which = which;
        BnL& B = c->bn[i];
        B.C = L.cout;
        B.rC = c->rch(L.level);
        const Dim dout = lvl(L.level), din = which == 0 ? block_in_dim(b) : dout;
        const int st = stage_of_block(b);
        const std::string cp = c->res ? pfx + ".conv" : pfx;  // ResidualBlock.conv (mod.py:75)
        L.w = add(cp + (which ? ".3.weight" : ".0.weight"), {dout, din, k3, k3}, st);
        if (c->variant == UNET_VARIANT_MODEL) {  // model.py:33-43: 0 conv, 2 BN, 3 conv, 5 BN
            L.b = add(pfx + (which ? ".3.bias" : ".0.bias"), {dout}, st);
            B.name = pfx + (which ? ".5" : ".2");
        } else {  // mod.py:43-51 / :75-81: 0 conv (no bias), 1 BN, 3 conv, 4 BN
            L.b = -1;
            B.name = cp + (which ? ".4" : ".1");
        }
        B.g = add(B.name + ".weight", {dout}, st);
        B.b = add(B.name + ".bias", {dout}, st);
    };
    c->skip_w.assign(nb, -1);
    c->skip_pd.assign(nb, -1);
    c->skip_pf.assign(nb, -1);
    auto block = [&](int b, const std::string& pfx) {
        conv_pair(b, 0, pfx);
        conv_pair(b, 1, pfx);
        if (c->res)  // ResidualBlock.skip, Conv2d(in, out, 1, bias=False) (mod.py:83)
            c->skip_w[b] = add(pfx + ".skip.weight", {lvl(level_of(b)), block_in_dim(b), k1, k1},
                               stage_of_block(b));
    };
    auto convT = [&](int k, const std::string& name) {
        ConvTL& T = c->convt[k];
        T.in_level = D - k;
        T.cin = c->ch(D - k);
        T.cout = c->ch(D - k - 1);
        const int st = stage_of_block(D + k);
        T.w = add(name + ".weight", {lvl(D - k), lvl(D - k - 1), k2, k2}, st);
        T.b = add(name + ".bias", {lvl(D - k - 1)}, st);
    };
    const Dim dout_head{c->out_ch, c->out_ch, 1};
    if (c->variant == UNET_VARIANT_MODEL) {
        // models/model.py:6-31 registration order (D = 4, base 64)
        const char* bname[9] = {"encoder1", "encoder2", "encoder3", "encoder4", "middle.1",
                                "decoder3.0", "decoder2.0", "decoder1.0", "final.0"};
        const char* tname[4] = {"middle.2", "decoder3.1", "decoder2.1", "decoder1.1"};
        for (int b = 0; b <= D; ++b) block(b, bname[b]);
        for (int k = 0; k < D; ++k) {
            convT(k, tname[k]);
            block(D + 1 + k, bname[D + 1 + k]);
        }
        c->head_w = add("final.1.weight", {dout_head, lvl(0), k1, k1}, 0);
        c->head_b = add("final.1.bias", {dout_head}, 0);
    } else {
        // models/mod.py:21-41: encoders, (pools), bottleneck, upconvs, decoders, final_conv
        for (int l = 0; l < D; ++l) block(l, "encoders." + std::to_string(l));
        block(D, "bottleneck");
        for (int k = 0; k < D; ++k) convT(k, "upconvs." + std::to_string(k));
        for (int k = 0; k < D; ++k) block(D + 1 + k, "decoders." + std::to_string(k));
        c->head_w = add("final_conv.weight", {dout_head, lvl(0), k1, k1}, 0);
        c->head_b = add("final_conv.bias", {dout_head}, 0);
    }
    c->n_param_floats = off;
    c->n_pparam_floats = poff;
    int64_t run = 0, rrun = 0;
    for (auto& B : c->bn) {  // named_buffers() order == conv order in both variants
        B.run = run;
        B.rrun = rrun;
        run += 2 * B.C;
        rrun += 2 * B.rC;
    }
    c->n_bn_floats = rrun;
    c->n_pbn_floats = run;
    // expand / compact tables (the bn arena: mean and var vectors of each layer)
    c->pad_params.clear();
    c->pad_bn.clear();
    c->pad_max_numel = c->pad_bn_max = 0;
    if (c->padded) {
        for (const ParamT& p : c->params) {
            PadDesc d{p.off, p.poff, p.numel, p.pnumel, {1, 1, 1, 1}, {1, 1, 1, 1}, {1, 1, 1, 1}};
            for (int k = 0; k < 4; ++k) {
                d.seg[k] = (int32_t)p.seg[k];
                d.pseg[k] = (int32_t)p.pseg[k];
                d.nseg[k] = (int32_t)p.nseg[k];
            }
            c->pad_params.push_back(d);
            c->pad_max_numel = std::max(c->pad_max_numel, p.pnumel);
        }
        for (const BnL& B : c->bn)
            for (int v = 0; v < 2; ++v) {
                PadDesc d{B.rrun + v * B.rC, B.run + v * B.C, B.rC, B.C,
                          {B.rC, 1, 1, 1}, {B.C, 1, 1, 1}, {1, 1, 1, 1}};
                c->pad_bn.push_back(d);
                c->pad_bn_max = std::max<int64_t>(c->pad_bn_max, B.C);
            }
    }
    c->cmax = 0;
    for (auto& L : c->conv) c->cmax = std::max(c->cmax, std::max(L.cin, L.cout));
    // packed weights (forward + dgrad images); conv 0 (Cin = in_channels) has its own kernel
    int64_t pk = 0;
    for (int i = 0; i < c->nconv(); ++i) {
        ConvL& L = c->conv[i];
        const int64_t n = (int64_t)L.cin * L.cout * 9;
        if (i == 0 && L.cin < 32) {
            L.pf = L.pd = -1;
            continue;
        }
        // (every image starts at a multiple of 32 floats: the x3 copy of the whole region,
        // converted as rows of 32, then holds each image's x3 image at 3x its offset)
        L.pf = pk;
        pk += (n + 31) / 32 * 32;
        L.pd = pk;
        pk += (n + 31) / 32 * 32;
    }
    for (auto& T : c->convt) {
        const int64_t n = (int64_t)T.cin * T.cout * 4;
        T.pf = pk;
        pk += (n + 31) / 32 * 32;
        T.pd = pk;
        pk += (n + 31) / 32 * 32;
    }
    for (int b = 1; b < nb && c->res; ++b) {  // transposed skip images for the dgrad
        c->skip_pd[b] = pk;
        pk += ((int64_t)c->conv[2 * b].cin * c->conv[2 * b].cout + 31) / 32 * 32;
        if (c->bf16) {  // the forward GEMM's bf16 image (f32 reads the parameter itself)
            c->skip_pf[b] = pk;
            pk += ((int64_t)c->conv[2 * b].cin * c->conv[2 * b].cout + 31) / 32 * 32;
        }
    }
    c->pack_floats = pk;
    // gradient buckets: walk the arena from its end (what backward finishes first), open a
    // new bucket whenever a tensor finishes later than everything already in the current one
    // (so buckets become ready in order 0, 1, ...); tensors that finish earlier join it
    c->bucket_off.clear();
    c->bucket_len.clear();
    c->bucket_stage.clear();
    int64_t end = c->n_param_floats;
    int cur = -1;
    for (int t = (int)c->params.size() - 1; t >= 0; --t) {
        const ParamT& p = c->params[t];
        if (cur >= 0 && p.stage > cur) {
            c->bucket_off.push_back(p.off + p.numel);
            c->bucket_len.push_back(end - (p.off + p.numel));
            c->bucket_stage.push_back(cur);
            end = p.off + p.numel;
            cur = -1;
        }
        cur = std::max(cur, p.stage);
    }
    c->bucket_off.push_back(0);
    c->bucket_len.push_back(end);
    c->bucket_stage.push_back(cur);
    // the parameter tensors of each bucket (contiguous in arena order): a channel-padded
    // network compacts exactly these into the caller's arena before the bucket's event
    c->bucket_p0.assign(c->bucket_off.size(), 0);
    c->bucket_p1.assign(c->bucket_off.size(), 0);
    c->bucket_pmax.assign(c->bucket_off.size(), 0);
    for (size_t b = 0; b < c->bucket_off.size(); ++b) {
        int p0 = -1, p1 = -1;
        for (int t = 0; t < (int)c->params.size(); ++t) {
            const ParamT& q = c->params[t];
            if (q.off >= c->bucket_off[b] && q.off + q.numel <= c->bucket_off[b] + c->bucket_len[b]) {
                if (p0 < 0) p0 = t;
                p1 = t + 1;
                c->bucket_pmax[b] = std::max(c->bucket_pmax[b], q.pnumel);
            }
        }
        c->bucket_p0[b] = p0 < 0 ? 0 : p0;
        c->bucket_p1[b] = p1 < 0 ? 0 : p1;
    }
}

// ------------------------------------------------------------------------------------
// Routes.  Which kernel family runs each GEMM of a layer and who writes its operand image,
// decided once per plan by make_routes (below, after the rules it applies); make_plan sizes
// the workspace from it, forward_impl and backward_impl only read it.
// ------------------------------------------------------------------------------------
// one row GEMM as the plan fixes it (tiles.h; t is never null: NO_TILE where an option names none)
struct GemmPlan {
    RowGeom g{};
    const Tile* t = &NO_TILE;
};
// a weight gradient's tile (t16: the LDS-DMA tile where the family is FAM_DMA16, which keeps the
// register-staged tile's partition) and split-K partition
struct WgradCfg {
    const Tile* t = &NO_TILE;
    const Tile* t16 = &NO_TILE;
    int splits = 1, pps = 0;
};

enum Family : uint8_t {
    FAM_NONE,   // not a GEMM: the single-input-channel first conv / first skip (k_conv_first_*,
                // k_res_first_*)
    FAM_REG,    // the f32 kernels, or in bf16 math the register-staged bf16 ones (kernels_gemm.hip,
                // kernels_gemm_pipe.hip)
    FAM_DMA16,  // the LDS-DMA bf16 kernels rg16 / wg16 (kernels_gemm16.hip)
    FAM_X3,     // f32 math on split bf16 operands (kernels_gemm_x3.hip)
};
// who writes (half of) a conv's bf16 / x3 operand image
enum Writer : uint8_t {
    W_PREP,   // the conv's own prep pass (prep16 / prep_x3)
    W_CONVT,  // the ConvT forward's out16 / out3 store (the up half of a decoder's concat)
    W_POOL,   // the max-pool (the skip half of a decoder's concat; the whole image of an encoder's)
};
struct Route {
    Family fwd = FAM_NONE;    // forward GEMM
    Family dgrad = FAM_NONE;  // input gradient (bf16: rg16_on(cout, cin), not the forward's (cin, cout))
    Family wgrad = FAM_NONE;  // weight gradient
    bool keep = false;        // training: the forward's operand image is kept for the weight gradient
                              // (Plan::x16 / t16 / x3 / t3; a skip GEMM reads its block's conv image)
    // convs on FAM_DMA16 / FAM_X3: the writers of the image's up and skip halves (a conv that
    // reads no concat: both name the whole image)
    Writer up = W_PREP, skip = W_PREP;
    bool head_fuse = false;   // the last conv's dz pass recomputes `do` from the 1x1 head
    bool pool_fuse = false;   // an encoder's second conv: ... from the max-pool backward's inputs
    // chosen by plan_tiles, after the families: the forward and input-gradient GEMMs (geometry with
    // the epilogue the block structure gives it, and tile), the weight gradient's tile and split-K
    // partition, and whether that kernel's B' loader forms the BN-backward dz (option dz_in_wgrad)
    GemmPlan f, d;
    WgradCfg w;
    bool dzw = false;
};
// (fixed arrays: a plan is made four times per training step, and unet_adamw_repack reads `x3`
// from a record of its own, so building one allocates nothing)
struct Routes {
    Route conv[2 * (2 * MAX_DEPTH + 1)];  // per conv
    Route convt[MAX_DEPTH];               // per ConvT
    Route skip[2 * MAX_DEPTH + 1];        // per block (residual network)
    bool x3 = false;                      // some GEMM is on FAM_X3: the plan carries pack3
};

// ------------------------------------------------------------------------------------
// Workspace plan.  A bump allocator over the caller's buffer; the same function sizes and
// carves it so forward and backward agree on every pointer.
// ------------------------------------------------------------------------------------
struct Plan {
    int N, H, W;
    int64_t P[MAX_DEPTH + 1];  // pixels per level
    Routes rt;
    float* pack;
    float* x_nhwc;
    std::vector<float*> y;
    std::vector<int> ldy, offy;
    std::vector<float*> scale, shift, mean, invstd;
    float* cat[MAX_DEPTH];
    float* cat_scale[MAX_DEPTH];
    float* cat_shift[MAX_DEPTH];
    float* pool[MAX_DEPTH];
    uint8_t* idx[MAX_DEPTH];
    std::vector<float*> out;  // residual network: block outputs (ld, off)
    std::vector<int> ldout, offout;
    float* stats;
    float* stats2;
    // backward
    float* g[3];
    float* dcat[MAX_DEPTH];
    float* slab;
    float* part;   // BN-backward column partials [rows][2][C]
    float* part2;  // second-level reduction of part
    float* hpart;  // head / conv-first weight-gradient partials
    float* bslab;  // [splits][Nw] bias-gradient column sums from the wgrad kernels
    float* coef;
    float* gdz;    // option dz_in_wgrad: the dz the weight gradient stores for the dgrad
    // bf16 LDS-DMA GEMMs: prepared operand image (dense [pixels][C] bf16) and a zero page
    uint16_t* s16;
    uint16_t* r16;  // residual network, bf16: scratch image of a block's input (conv1 + skip)
    void* zero16;
    std::vector<uint16_t*> x16;  // training, bf16: per-conv input images kept for the wgrad
    std::vector<uint16_t*> t16;  // training, bf16: per-ConvT input images kept for the wgrad
    // f32 GEMMs on split bf16 operands (option x3): x3 copy of the weight images, per-conv /
    // per-ConvT input images kept for the weight gradients, one scratch image
    uint16_t* pack3;
    uint16_t* s3;
    std::vector<uint16_t*> x3;
    std::vector<uint16_t*> t3;
    // channel-padded networks: padded parameter / running-stat / gradient arenas and the
    // device copies of the expand / compact tables
    float* pprm;
    float* pbn;
    float* pgrad;
    float* ugrad;  // padded network: the caller's (torch-layout) gradient arena
    PadDesc* ptab;
    PadDesc* btab;
    size_t bytes;
};

// Every region starts at a multiple of WS_ALIGN bytes from the workspace base, and the
// kernels read the regions with 16-byte loads and LDS-DMA: the base itself must be aligned
// (unet_forward / unet_backward refuse one that is not).
constexpr int WS_ALIGN = 256;

inline bool ws_aligned(const void* ws) { return ((uintptr_t)ws & (WS_ALIGN - 1)) == 0; }

struct Bump {
    char* base;
    size_t off = 0;
    template <class T>
    T* take(int64_t n) {
        off = (off + WS_ALIGN - 1) & ~(size_t)(WS_ALIGN - 1);
        T* p = base ? (T*)(base + off) : nullptr;
        off += (size_t)n * sizeof(T);
        return p;
    }
};

// wgrad tile (tiles.h WG_TILES / WGB_TILES) + split-K over pixels so that every layer
// launches >= 2048 blocks; options wgrad_tile_{w,n} override (tuning runs).
// 3x3 weight gradients on rows that are a multiple of 32 pixels take the one-row-of-taps tiles
// (WG3_*, wgrad_row3_kernel) when option wgrad_row3 selects them: 1 = every eligible layer,
// 2 = only layers with a 64-channel operand (the 256x256 / 128x128 levels), 0 = never.
// The split-K partition follows from the (default) tile dims; the bf16 LDS-DMA weight
// gradient (wg16_tile) reuses the register-staged tile's partition, so its tile choice
// never changes the summation order.
WgradCfg wgrad_cfg(const unet_ctx* c, const WgGeom& g, bool bf16) {
    const Options& o = c->opt;
    const int CA = g.CA, CB = g.CB, tapsA = gather_taps(g.amode), tapsB = gather_taps(g.bmode);
    const int64_t P = g.P;
    const Tile* t;
    if (bf16) {
        t = wgb_desc((CA % 128 == 0 && CB % 128 == 0) ? WGB_128x128
                     : CA % 128 == 0 ? WGB_128x64 : CB % 128 == 0 ? WGB_64x128 : WGB_64x64);
    } else {
        int id;
        if (CA % 128 == 0 && CB % 128 == 0)
            id = o.wgrad_tile_w;
        else if (CA % 64 == 0 && CB % 64 == 0 && (CA % 128 || CB % 128) && o.wgrad_tile_n >= 0)
            id = (CA % 128 == 0) ? WG_128x64 : (CB % 128 == 0 ? WG_64x128 : o.wgrad_tile_n);
        else if (CA % 64)  // 32-channel operands (narrow networks' level 0)
            id = WG_32x32;
        else if (CB % 64)
            id = WG_64x32;
        else
            id = WG_64x64;
        t = wg_desc(id);
        if (!t) t = wg_desc(WG_64x64);  // an option that names no tile (both counts divide 64 then)
        // a row3 tile exists for this GEMM (the smallest one fits), and the option selects it
        const bool row3 = wg_row3_ok(*wg_desc(WG3_32x32), g) &&
                          (o.wgrad_row3 == 1 || (o.wgrad_row3 == 2 && (CA == 64 || CB == 64)));
        const bool r3n = CA % 64 || CB % 64;  // a 32-channel operand (r04)
        const auto row3_opt = [](int id) { const Tile* q = wg_desc(id); return q && q->taps == 3 ? q : nullptr; };
        if (row3 && r3n && o.wgrad_row3_n32) {
            t = wg_desc(CA % 64 ? (CB % 64 ? WG3_32x32 : WG3_32x64) : WG3_64x32);
        } else if (row3 && !r3n) {
            const Tile* forced = row3_opt(o.wgrad_row3_tile);
            t = forced ? forced
                       : wg_desc(CA % 128 == 0 ? (CB % 128 == 0 ? WG3_128x128 : WG3_128x64)
                                               : (CB % 128 == 0 ? WG3_64x128 : WG3_64x64));
            // option wgrad_row3_big: the tile of the layers whose channel counts both divide
            // 128.  Default 128x64 rather than 128x128: the same GEMM time (126 TF/s)
            // but twice the tiles, so the 1536-block target needs half the split-K slices and
            // the slab reduction halves (r02 A/B: wgrad_reduce 1.09 -> 0.64 ms, 404 -> 408 img/s)
            if (!forced && row3_opt(o.wgrad_row3_big) && CA % 128 == 0 && CB % 128 == 0)
                t = row3_opt(o.wgrad_row3_big);
        }
    }
    WgradCfg w;
    w.t = t;
    const int64_t tiles = (int64_t)(tapsA * CA / (t->bm * t->taps)) * (tapsB * CB / t->bn);
    // blocks to launch: 2048 one-tap blocks; a row3 block does the work of three, and every
    // extra split adds a full Mw x Nw slab to write and reduce
    const int64_t target =
        bf16 ? o.wgrad16_blocks : (t->taps == 3 ? o.wgrad_row3_blocks : o.wgrad_blocks) * t->per4;
    int64_t s = (target + tiles - 1) / tiles;
    const int64_t maxs = P / (8 * t->bk) > 0 ? P / (8 * t->bk) : 1;  // >= 8 chunks per split
    // (P need not be a multiple of the pixel chunk: the kernel zero-fills the tail)
    if (s > maxs) s = maxs;
    if (s < 1) s = 1;
    int64_t pps = (P + s - 1) / s;
    pps = (pps + 127) / 128 * 128;
    // (r06) bf16 3x3 weight gradients on the tap-row kernel (W % 64 == 0): the 1536-block target
    // above, counted in one-tap 128x128 tiles, launches (CA / 128) 3 (CB / 128) tap-row blocks
    // per split, i.e. 513-576 blocks on 256 one-block-per-CU slots -- a third wave holding 1-64
    // blocks, and the kernel took three block durations instead of two.  Instead pick the split
    // count s minimising waves(s) x chunks per block(s) + the slab traffic of s splits (the
    // one-tap kernel, option wg16_r3 = 0, gets the same partition: bit-identical).
    // (W = 32 / 16: the deep levels' tap-row instances, W16_R3M, r06)
    const Tile& m16 = *wg16_desc(W16_R3M);
    if (bf16 && conv_wgrad(g) && wg16_row3_rows(m16, g.W) && CA % m16.bm == 0 && CB % m16.bn == 0 && P % 64 == 0) {
        const int64_t t3 = (int64_t)(CA / m16.bm) * 3 * (CB / m16.bn);
        const int64_t slots = c->cus;
        double best = -1;
        for (int64_t sc = 1; sc <= maxs; ++sc) {
            const int64_t waves = (t3 * sc + slots - 1) / slots;
            const int64_t chunks = (P + 64 * sc - 1) / (64 * sc);
            // ~1.2 us per 64-pixel chunk of a 128x128x3 block; slabs written and reduced at ~5 TB/s
            const double cost = waves * chunks * 1.2e-6 + sc * 9.0 * CA * CB * 8 / 5e12;
            if (best < 0 || cost < best) best = cost, s = sc;
        }
        pps = (P + s - 1) / s;
        pps = (pps + 63) / 64 * 64;
    }
    w.pps = (int)pps;
    w.splits = (int)((P + pps - 1) / pps);
    return w;
}

// bf16 math: conv / ConvT GEMMs whose K channels are a multiple of 64 and whose N is a
// multiple of 128 run on the LDS-DMA kernel (kernels_gemm16.hip) from a prepared bf16
// operand image; option rg16 = 0 keeps the register-staged bf16 kernel (A/B runs),
// rg16_tile picks its tile (tiles.h RG16_TILES).
bool rg16_on(const unet_ctx* c, int C, int N) {
    return c->bf16 && c->opt.rg16 != 0 && C % 64 == 0 && N % 128 == 0;
}
// tile for one LDS-DMA row GEMM.  Option rg16_tile forces a tile (128x128 where N does not
// divide into it).  Every tile emits BN partials in 128-row groups, so the choice changes
// speed only.  Default: the 256x256 tile (8 waves, one block per CU) unless
//  * it would leave CUs idle: fewer than 256 blocks (the 16x16 / 32x32 levels of config 4:
//    bottleneck fwd 0.48 -> 0.37 ms, its dgrad 0.90 -> 0.48 ms on the 128x128 tile), or
//  * option rg16_bn_k > K for a BN-backward-partials GEMM (E_STORE_BN: reads the BN input,
//    writes f32 and reduces per-channel partials): with one block per CU nothing hides that
//    epilogue, while two co-resident 128x128 blocks overlap one's epilogue with the other's
//    MFMAs (r01: level-1 dgrad 1.15 -> 0.80 ms, profiles/r01_rg16_tile_sweep.txt; default 0
//    since the r04 one-barrier halo kernel made the 256x256 / 512x128 tiles faster overall).
int rg16_pick(const unet_ctx* c, const RowGeom& g) {
    const Options& o = c->opt;
    const int cout = g.emode == E_CONVT ? g.cout : 0;
    auto fits = [&](int id) {
        const Tile* t = rg16_desc(id);
        if (!t || (t->kind == K_HALO && !halo_ok(*t, g))) return false;
        return g.N % t->bn == 0 && (cout == 0 || cout % t->bn == 0);
    };
    const int forced = o.rg16_tile;
    if (forced >= 0) return fits(forced) ? forced : R16_128x128;
    const int t0 = R16_128x128;
    int t4 = R16_256x256;
    if (o.rg16_r3 && fits(R16_H256x256)) t4 = R16_H256x256;  // option rg16_r3: the tap-row halo kernel
    if (!fits(R16_256x256)) {
        // option rg16_n128: a 512-row tile for the 128-output GEMMs (halo kernel for 3x3 convs)
        // (rg16_r3 = 0 turns the halo kernel off here too: the one-tap 512x128 tile instead)
        int tn = o.rg16_n128;
        if (tn == R16_H512x128 && (!o.rg16_r3 || !fits(R16_H512x128))) tn = R16_512x128;
        if (tn < 0 || !fits(tn)) return t0;
        if ((g.M + 511) / 512 * (g.N / 128) < 256) return t0;
        if (g.emode == E_STORE_BN && g.K < o.rg16_bn_k && !o.rg16_n128_bn) return t0;
        return tn;
    }
    const int64_t blocks = (g.M + 255) / 256 * (g.N / 256);
    // (r06) a grid too small for 256x256 that fills the CUs with 256x128 takes it (the 16^2
    // bottleneck's 4096-output GEMMs of config 4) instead of 128x128 at two blocks per CU
    if (blocks < 256) return (g.M + 255) / 256 * (g.N / 128) >= 256 && fits(R16_256x128) ? R16_256x128 : t0;
    if (g.emode == E_STORE_BN && g.K < o.rg16_bn_k) return t0;
    return t4;
}
// 3x3 weight gradients of layers with Cin, Cout multiples of 128 on the LDS-DMA
// transposed-read kernel (kernels_gemm16.hip wgrad16_kernel) from the forward's bf16 input
// image and the dz image; option wg16 = 0 keeps the register-staged bf16 wgrad, wg16_tile
// picks the tile.
bool wg16_on(const unet_ctx* c, int CA, int CB) {
    return c->bf16 && c->opt.wg16 != 0 && CA % 128 == 0 && CB % 128 == 0;
}
// XCD-contiguous block order for the LDS-DMA bf16 kernels: on by default (config 4 A/B:
// wgrad 718 -> 766 TF/s, forward 854 -> 871, dgrad -2 %, step +2 %); option xcd16 = 0 off
int xcd16_on(const unet_ctx* c) { return c->opt.xcd16 != 0 ? 1 : 0; }
// tile: option wg16_tile (default 256x256) where both channel counts allow it; option wg16_r3: a
// 3x3 layer the tap-row kernel takes (three taps per block from one halo row) on it.  (The split
// count, sized for >= 2048 128x128 tiles, gives >= 512 256x256 ones.)  g.pps: the split chosen.
const Tile* wg16_pick(const unet_ctx* c, const WgGeom& g) {
    const Tile* t = wg16_desc(c->opt.wg16_tile);
    if (!t || g.CA % t->bm || g.CB % t->bn) t = wg16_desc(W16_128x128);
    const Tile* r3 = wg16_desc(c->opt.wg16_r3);
    return r3 && r3->taps == 3 && wg16_row3_ok(*r3, g) ? r3 : t;
}
// ConvT weight gradient on the LDS-DMA transposed-read kernel (A' = the forward's bf16
// ConvT input image, B' = the bf16 image of the concat gradient's up half, G_UP2-gathered);
// the bias gradient then comes from k_up2_bias_partials.  Option wg16t = 0 keeps the
// register-staged kernel.
bool convt_wg16_on(const unet_ctx* c, int cin, int cout) {
    return c->opt.wg16t != 0 && wg16_on(c, cin, cout) && rg16_on(c, cin, 4 * cout) &&
           rg16_on(c, cout, cin);
}

// f32 math on the bf16 matrix cores (option x3, kernels_gemm_x3.hip): a 3x3 conv / ConvT
// whose in- and output channels are multiples of 64 runs its forward, input-gradient and
// weight-gradient GEMMs on x3 images (exact three-way bf16 splits of the f32 operands, six
// MFMA products, split f32 accumulators: fp64 error ~3x below the f32 MFMA kernels',
// profiles/r04_x3_probe_*.txt).  The residual network's 1x1 skip GEMMs keep the f32 kernels.
// (r05, removed in r06: option x3_n32, x3 for the 32-multiple channel counts of the reference
// grid's narrow widths on a 128 x 32 row tile and 32-wide weight-gradient tiles -- slower than the
// f32 MFMA kernels there, profiles/r05_x3_n32_ab.txt.)
bool x3_conv_on(const unet_ctx* c, int cin, int cout) {
    return c->opt.x3 && !c->bf16 && cin % 64 == 0 && cout % 64 == 0;
}

// The routes of this context under its present options: the one place rg16_on, wg16_on,
// convt_wg16_on, x3_conv_on and the convt16 / pool_fuse / head_fuse options are asked.
// P0: pixels of level 0 (the pool_fuse kernels decode pixel indices below 2^24).
Routes make_routes(const unet_ctx* c, bool training, int64_t P0) {
    const int D = c->depth, NC = c->nconv();
    Routes r;
    // a 3x3 conv / ConvT; wg16: the LDS-DMA weight gradient applies (training keeps the image)
    auto gemms = [&](Route& q, int cin, int cout, bool wg16) {
        if (x3_conv_on(c, cin, cout)) {
            q.fwd = q.dgrad = q.wgrad = FAM_X3;
            q.keep = training;
        } else {
            q.fwd = rg16_on(c, cin, cout) ? FAM_DMA16 : FAM_REG;
            q.dgrad = rg16_on(c, cout, cin) ? FAM_DMA16 : FAM_REG;
            q.keep = training && wg16;
            q.wgrad = q.keep ? FAM_DMA16 : FAM_REG;
        }
        r.x3 = r.x3 || q.fwd == FAM_X3;
    };
    for (int i = 0; i < NC; ++i) {
        const ConvL& L = c->conv[i];
        if (L.pf >= 0) gemms(r.conv[i], L.cin, L.cout, wg16_on(c, L.cin, L.cout) && rg16_on(c, L.cin, L.cout));
    }
    for (int k = 0; k < D; ++k) {
        const ConvTL& T = c->convt[k];
        gemms(r.convt[k], T.cin, T.cout, convt_wg16_on(c, T.cin, T.cout));
    }
    // the residual network's 1x1 skip GEMMs keep the f32 kernels in f32 math; bf16: the weight
    // gradient on the LDS-DMA kernel where the block's first conv keeps its image
    for (int b = 1; b <= 2 * D && c->res; ++b) {
        const ConvL& L = c->conv[2 * b];
        Route& q = r.skip[b];
        q.fwd = rg16_on(c, L.cin, L.cout) ? FAM_DMA16 : FAM_REG;
        q.dgrad = rg16_on(c, L.cout, L.cin) ? FAM_DMA16 : FAM_REG;
        q.wgrad = r.conv[2 * b].wgrad == FAM_DMA16 ? FAM_DMA16 : FAM_REG;
    }
    // a dz pass that leaves no f32 dz: both backward GEMMs read its image
    auto image_dz = [](const Route& q) {
        return q.wgrad == FAM_X3 || (q.wgrad == FAM_DMA16 && q.dgrad == FAM_DMA16);
    };
    for (int b = 0; b < D && !c->res; ++b) {
        // the max-pool stores op(pooled) as the operand image of the next encoder block's first
        // conv: x3 always (r05), bf16 where training keeps the image (r06)
        Route& nx = r.conv[2 * (b + 1)];
        if (nx.fwd == FAM_X3 || nx.wgrad == FAM_DMA16) nx.up = nx.skip = W_POOL;
        // option pool_fuse (x3 r05, bf16 r06): the encoder block's second conv recomputes its
        // `do` in the dz pass, where that pass writes an image only
        const ConvL& C1 = c->conv[2 * b + 1];
        r.conv[2 * b + 1].pool_fuse = c->opt.pool_fuse && C1.cout == c->ch(b) && (P0 >> (2 * b)) < (1 << 24) &&
                                      image_dz(r.conv[2 * b + 1]);
        // option convt16 (training): the decoder conv at this level reads its kept image only, so
        // the max-pool stores the skip half of the concat there and the ConvT the up half (bf16:
        // skip-first concat, identity affine).  Not in the residual network, whose 1x1 skip GEMM
        // reads the f32 concat as well.
        Route& dec = r.conv[2 * (2 * D - b)];
        if (c->opt.convt16 && dec.keep && (dec.fwd == FAM_X3 || (dec.fwd == FAM_DMA16 && c->skip_first))) {
            dec.skip = W_POOL;
            if (r.convt[D - 1 - b].fwd == dec.fwd) dec.up = W_CONVT;
        }
    }
    // option head_fuse (x3 r05, bf16 r06), one output channel: head_bwd stores no `do`
    r.conv[NC - 1].head_fuse = c->opt.head_fuse && !c->res && c->out_ch == 1 &&
                               c->conv[NC - 1].cout == c->base && image_dz(r.conv[NC - 1]);
    return r;
}

// row-GEMM tile: the tap-row halo kernel for 3x3 convs (256 x 128, or 128 x 64 for the 64-output
// GEMMs); otherwise the one-tap tiles (256 x 128, 128 x 128 where the 256-row grid would leave CUs
// idle, 128 x 64 / 256 x 64: option x3_n64)
int x3_pick(const unet_ctx* c, const RowGeom& g) {
    auto fits = [&](int id) {
        const Tile* t = x3_desc(id);
        if (!t || g.N % t->bn) return false;
        return g.emode != E_CONVT || g.cout % t->bn == 0 || t->bn % g.cout == 0;
    };
    // the halo tiles: 3x3 convs on rows of 16 .. 256k pixels (option x3_r3), for either tile by
    // the 256-row one's rule (which implies the 128-row one's)
    const bool r3ok = halo_ok(*x3_desc(X3_H256x128), g);
    const int ft = c->opt.x3_tile;
    if (ft >= 0 && fits(ft) && (x3_desc(ft)->kind != K_HALO || r3ok)) return ft;
    if (g.N % 128 == 0 && fits(X3_256x128)) {
        const int64_t blocks = (int64_t)(g.M + 255) / 256 * (g.N / 128);
        if (blocks < 256) return X3_128x128;
        return c->opt.x3_r3 && r3ok ? X3_H256x128 : X3_256x128;
    }
    // 64 outputs: the 128 x 64 halo tile where the 256-row grid fills the chip (r05: 0.2 % over
    // a 256 x 64 halo tile, 1.032 vs 1.103 ms for a 512 x 64 one, profiles/r05_halo_k16.txt)
    if (g.N % 64 == 0 && c->opt.x3_r3 && r3ok && (int64_t)(g.M + 255) / 256 >= 512) return X3_H128x64;
    return fits(c->opt.x3_n64) ? c->opt.x3_n64 : -1;
}

// weight gradient: 128x128 tile where both channel counts allow it, else 64x64; split-K over
// pixels so the grid has >= x3_wblocks 128x128 blocks (4x that of 64x64 ones); pixels per
// split a multiple of 256
// 3x3 convs the tap-row kernel takes (wx3_row3_ok): 64x128 or 64x64 per tap, three taps per block
// (r06: 64 x 64 rather than 128 x 64 where only the input channels divide 128 -- config 2's
// 128 -> 64 level-0 conv 1.53 -> 1.24 ms, profiles/r06_c2_wtile_ab.txt)
WgradCfg x3_wgrad_cfg(const unet_ctx* c, const WgGeom& g) {
    const int CA = g.CA, CB = g.CB;
    const int64_t P = g.P;
    auto fits = [&](const Tile* t) {
        return t && (t->taps == 3 ? wx3_row3_ok(*t, g) : CA % t->bm == 0 && CB % t->bn == 0);
    };
    const Tile* t = wx3_desc((CA % 128 == 0 && CB % 128 == 0) ? WX3_128x128 : WX3_64x64);
    if (fits(wx3_desc(WX3_R3_64x128))) t = wx3_desc(WX3_R3_64x128);
    else if (fits(wx3_desc(WX3_R3_64x64))) t = wx3_desc(WX3_R3_64x64);
    if (fits(wx3_desc(c->opt.x3_wtile))) t = wx3_desc(c->opt.x3_wtile);
    WgradCfg w;
    w.t = t;
    const bool tap_row = t->taps == 3;
    const int64_t tiles = tap_row ? (int64_t)(CA / t->bm) * 3 * (CB / t->bn)
                                  : (int64_t)(gather_taps(g.amode) * CA / t->bm) * (gather_taps(g.bmode) * CB / t->bn);
    // blocks per 128x128 one-tap block of work: by area (one-tap), half that (tap-row)
    const int area = std::max(1, 16384 / (t->bm * t->bn));
    const int64_t target = (int64_t)c->opt.x3_wblocks * (tap_row ? std::max(1, area / 2) : area);
    int64_t splits = std::max<int64_t>(1, (target + tiles - 1) / tiles);
    int64_t pps = (P + splits - 1) / splits;
    pps = (pps + 255) / 256 * 256;
    const int ww = tap_row ? c->opt.x3_wwaves : c->opt.x3_wwaves1;
    if (ww > 0) {
        // (r05) exactly `ww` full waves of block slots (CUs x blocks per CU): at most that many
        // blocks, pixel splits in 32-pixel steps.  The 256-pixel rounding above can land a few
        // blocks past a wave boundary (1024: 2049 blocks on 2048 slots, -4 %)
        const int64_t slots = (int64_t)c->cus * t->per_cu * ww;
        const int64_t s = std::max<int64_t>(1, slots / tiles);
        pps = (P + s - 1) / s;
        pps = (pps + 31) / 32 * 32;
    }
    w.pps = (int)pps;
    w.splits = (int)((P + pps - 1) / pps);
    return w;
}

// point g at x3 operands: A image `img` (lda = C channels), weights w3
void use_x3(const unet_ctx* c, const Plan& p, RowGemmArgs& g, const uint16_t* img, int C, const uint16_t* w3) {
    g.a = nullptr;
    g.a16 = img;
    g.lda = C;
    g.aoff = 0;
    g.ascale = g.ashift = nullptr;
    g.arelu = 0;
    g.acoef = nullptr;
    g.ay = nullptr;  // (the f32 dgrad's description of dz's source: no x3 kernel reads it)
    g.lday = g.offay = 0;
    g.bt = nullptr;
    g.bt16 = w3;
    g.zero16 = p.zero16;
    g.xcd = 1;
    g.tgm = c->opt.tile_group ? -1 : 0;
}

// launch labels, printed from the descriptor (tests/kernel_cases.py and profiles/kernel_coverage.txt
// parse them): <site>/<kernel><tag>_<BM>x<BN>[x<BK> | s<stages>]|<layer> (rowgemm: the tag last)
std::string tile_label(const char* site, const char* kernel, const char* tag, const Tile& t, const char* third,
                       int layer, const char* tag_last = "") {
    char b[112], k[16] = "";
    if (third) snprintf(k, sizeof k, "%s%d", third, t.bk);
    snprintf(b, sizeof b, "%s/%s%s_%dx%d%s%s|%d", site, kernel, tag, t.bm, t.bn, k, tag_last, layer);
    return b;
}

// Row-GEMM tile choice for an output width N (tiles.h ROW_TILES).
//  * f32, N % 128 == 0: the software-pipelined 128x128 kernel, forward with its global loads
//    two chunks ahead, dgrad too since r03 (one chunk ahead, removed in r06).  r02
//    A/B (config 2):
//    401 img/s against 390 for the register-staged tiles (t7 / t4 / t0 by grid size), the
//    dominant kernel 128.9 vs 122.2 TF/s; the two schedules store identical bits
//    (tests/test_gpu_parity.py::test_pipe_gemm_bit_identical);
//  * f32, N = 64 outputs: the pipelined 128x64 with loads two chunks ahead on the
//    forward GEMMs (level-0 128 -> 64 conv 112 -> 117 TF/s), the register-staged 128x64
//    on the ConvT forward and since r03 the three-blocks-per-CU tiles on the dgrads
//    (options tile_n64 / tile_n64_dgrad / tile_convt64; profiles/r02_pipe_exp.txt).
// bf16 MFMA (register-staged): a chunk of 64 K per barrier (4 MFMA k-steps) by default.
// Options tile_* override (tuning runs; -1 = automatic).
int pick_tile(const unet_ctx* c, int N, bool dgrad, bool bf16, bool convt = false) {
    const Options& o = c->opt;
    if (bf16) return N % 128 == 0 ? RG_128x128K64 : RG_128x64;  // register-staged bf16 tiles
    if (N % 64) return o.tile_n32;  // 32 outputs (narrow networks' level 0)
    if (N % 128) return convt && !dgrad ? o.tile_convt64 : (dgrad ? o.tile_n64_dgrad : o.tile_n64);
    if (convt && !dgrad && o.tile_convt >= 0) return o.tile_convt;
    if (convt && dgrad && o.tile_convt_dgrad >= 0) return o.tile_convt_dgrad;
    // dgrad on the two-chunks-ahead tile too since r03's prologue fence (loop waits vmcnt(2)
    // -> vmcnt(8)): conv dgrads 23.4 -> 23.0 ms per step
    if (dgrad) return o.tile_n128_dgrad >= 0 ? o.tile_n128_dgrad : RG_P128x128;
    return o.tile_n128 >= 0 ? o.tile_n128 : RG_P128x128;
}

// the tile of one row GEMM of family fam (convt: a ConvT's forward or input gradient; its forward's
// grid N is 4 cout and its f32 tile goes by cout)
const Tile* row_pick(const unet_ctx* c, Family fam, const RowGeom& g, bool dgrad, bool convt) {
    if (fam == FAM_X3) return &tile_or_none(x3_desc(x3_pick(c, g)));
    if (fam == FAM_DMA16) return &tile_or_none(rg16_desc(rg16_pick(c, g)));
    return &tile_or_none(row_desc(pick_tile(c, g.emode == E_CONVT ? g.cout : g.N, dgrad, c->bf16, convt)));
}

// Tiles and splits, after the routes (p: N, H, W, P and rt.*.{fwd, dgrad, wgrad} set): every GEMM's
// geometry -- the input gradients' epilogues follow from the block structure here, in one place --
// its tile, and in a training plan the weight gradient's split-K partition.  make_plan sizes the
// slabs from it; forward_impl, backward_impl, run_rowgemm and run_wgrad only read it.
void plan_tiles(const unet_ctx* c, Plan& p, bool training) {
    const int D = c->depth;
    auto layer = [&](Route& q, int level, RowGeom f, RowGeom d, WgGeom wg, bool convt) {
        f.M = d.M = (int)p.P[level];
        f.W = d.W = wg.W = p.W >> level;
        wg.H = p.H >> level;
        wg.P = p.P[level];
        if (q.fwd == FAM_NONE) return;
        q.f = {f, row_pick(c, q.fwd, f, false, convt)};
        if (!training) return;
        q.d = {d, row_pick(c, q.dgrad, d, true, convt)};
        q.w = q.wgrad == FAM_X3 ? x3_wgrad_cfg(c, wg) : wgrad_cfg(c, wg, c->bf16);
        wg.pps = q.w.pps;
        if (q.wgrad == FAM_DMA16) q.w.t16 = wg16_pick(c, wg);
    };
    for (int i = 0; i < c->nconv(); ++i) {
        const ConvL& L = c->conv[i];
        Route& q = p.rt.conv[i];
        // the input gradient of a block's second conv is the `do` of the first one's BN (its
        // epilogue emits that layer's partials); the residual block's first conv adds to the skip's
        const int de = L.which == 1 ? E_STORE_BN : c->res ? E_ADD : E_STORE;
        layer(q, L.level, {G_CONV3, c->bn_relu ? E_STATS : E_BIAS_RELU_STATS, 0, L.cout, 9 * L.cin, 0, 0},
              {G_CONV3, de, 0, L.cin, 9 * L.cout, 0, 0}, {G_CONV3, G_IDENT, 0, L.cin, L.cout, 0, 0, 0}, false);
        // option dz_in_wgrad: f32 register-staged weight-gradient tiles with the dz loader, with a
        // dgrad to feed (every conv but the first)
        q.dzw = training && q.wgrad == FAM_REG && !c->bf16 && c->opt.dz_in_wgrad && L.cin <= c->opt.dz_in_wgrad &&
                q.dgrad == FAM_REG && i > 0 && q.w.t->dz;
    }
    for (int k = 0; k < D; ++k) {
        const ConvTL& T = c->convt[k];
        // (residual network: d(block output); the block's own backward entry masks it)
        layer(p.rt.convt[k], T.in_level, {G_IDENT, E_CONVT, 0, 4 * T.cout, T.cin, 0, T.cout},
              {G_UP2, c->res ? E_STORE : E_STORE_BN, 0, T.cin, 4 * T.cout, 0, 0},
              {G_IDENT, G_UP2, 0, T.cin, T.cout, 0, 0, 0}, true);
    }
    for (int b = 1; b <= 2 * D && c->res; ++b) {
        const ConvL& L = c->conv[2 * b];
        layer(p.rt.skip[b], L.level, {G_IDENT, E_RESID, 0, L.cout, L.cin, 0, 0},
              {G_IDENT, E_STORE, 0, L.cin, L.cout, 0, 0}, {G_IDENT, G_IDENT, 0, L.cin, L.cout, 0, 0, 0}, false);
    }
}


void make_plan(unet_ctx* c, int N, int H, int W, bool training, char* base, Plan& p) {
    Bump b{base};
    const int D = c->depth, NC = c->nconv();
    p.N = N;
    p.H = H;
    p.W = W;
    for (int l = 0; l <= D; ++l) p.P[l] = (int64_t)N * (H >> l) * (W >> l);
    p.rt = make_routes(c, training, p.P[0]);
    plan_tiles(c, p, training);
    p.y.assign(NC, nullptr);
    p.ldy.assign(NC, 0);
    p.offy.assign(NC, 0);
    p.scale.assign(NC, nullptr);
    p.shift.assign(NC, nullptr);
    p.mean.assign(NC, nullptr);
    p.invstd.assign(NC, nullptr);
    p.pack = b.take<float>(c->pack_floats);
    p.pprm = p.pbn = p.pgrad = p.ugrad = nullptr;
    p.ptab = p.btab = nullptr;
    if (c->padded) {
        p.pprm = b.take<float>(c->n_pparam_floats);
        p.pbn = b.take<float>(c->n_pbn_floats);
        p.pgrad = training ? b.take<float>(c->n_pparam_floats) : nullptr;
        p.ptab = b.take<PadDesc>((int64_t)c->pad_params.size());
        p.btab = b.take<PadDesc>((int64_t)c->pad_bn.size());
    }
    p.x_nhwc = b.take<float>(p.P[0] * c->in_ch);  // NHWC copy of x (conv-0 wgrad input)
    for (int l = 0; l < D; ++l) {
        const int C = c->ch(l);
        p.cat[l] = b.take<float>(p.P[l] * 2 * C);
        p.cat_scale[l] = b.take<float>(2 * C);
        p.cat_shift[l] = b.take<float>(2 * C);
        p.pool[l] = b.take<float>(p.P[l + 1] * C);
        p.idx[l] = b.take<uint8_t>(p.P[l + 1] * C);
    }
    for (int i = 0; i < NC; ++i) {
        const ConvL& L = c->conv[i];
        if (L.block < D && L.which == 1 && !c->res) {
            // the encoder output lives in the skip half of its concat buffer, and its BN
            // affine is that half of the concat affine
            const int l = L.block, so = c->skip_off(l);
            p.y[i] = p.cat[l];
            p.ldy[i] = 2 * c->ch(l);
            p.offy[i] = so;
            p.scale[i] = p.cat_scale[l] ? p.cat_scale[l] + so : nullptr;
            p.shift[i] = p.cat_shift[l] ? p.cat_shift[l] + so : nullptr;
        } else {
            p.y[i] = b.take<float>(p.P[L.level] * L.cout);
            p.ldy[i] = L.cout;
            p.offy[i] = 0;
            p.scale[i] = b.take<float>(L.cout);
            p.shift[i] = b.take<float>(L.cout);
        }
        p.mean[i] = b.take<float>(L.cout);
        p.invstd[i] = b.take<float>(L.cout);
    }
    p.out.assign(2 * D + 1, nullptr);
    p.ldout.assign(2 * D + 1, 0);
    p.offout.assign(2 * D + 1, 0);
    for (int blk = 0; blk <= 2 * D && c->res; ++blk) {
        const ConvL& L = c->conv[2 * blk + 1];
        if (blk < D) {  // encoder output: the skip half of its concat buffer
            p.out[blk] = p.cat[blk];
            p.ldout[blk] = 2 * L.cout;
            p.offout[blk] = c->skip_off(blk);
        } else {
            p.out[blk] = b.take<float>(p.P[L.level] * L.cout);
            p.ldout[blk] = L.cout;
        }
    }
    // BN-stat partials: rows = M / 64 (smallest row tile) of the row GEMM, or RED_G for the
    // first conv
    int64_t srows = 0;
    for (int i = 0; i < NC; ++i) {
        const int64_t r = std::max<int64_t>((p.P[c->conv[i].level] + 63) / 64, RED_G);
        srows = std::max(srows, r * 2 * c->conv[i].cout);
    }
    p.stats = b.take<float>(srows);
    p.stats2 = b.take<float>((int64_t)STAT_G * 2 * c->cmax);
    p.s16 = p.r16 = nullptr;
    p.zero16 = b.take<char>(256);  // zeroed 16-B page: padding taps of the LDS-DMA GEMMs
    if (c->bf16) {
        int64_t n16 = 0;
        for (const ConvL& L : c->conv) n16 = std::max(n16, p.P[L.level] * std::max(L.cin, L.cout));
        for (const ConvTL& T : c->convt)
            n16 = std::max(n16, std::max(p.P[T.in_level] * T.cin, p.P[T.in_level - 1] * T.cout));
        p.s16 = b.take<uint16_t>(n16);
        // (where training keeps the image for an LDS-DMA weight gradient, x16, that one is shared)
        if (c->res) p.r16 = b.take<uint16_t>(n16);
    }
    p.x16.assign(NC, nullptr);
    for (int i = 0; i < NC; ++i)
        if (p.rt.conv[i].wgrad == FAM_DMA16)
            p.x16[i] = b.take<uint16_t>(p.P[c->conv[i].level] * c->conv[i].cin);
    p.t16.assign(c->convt.size(), nullptr);
    for (size_t k = 0; k < c->convt.size(); ++k) {
        const ConvTL& T = c->convt[k];
        if (p.rt.convt[k].wgrad == FAM_DMA16) p.t16[k] = b.take<uint16_t>(p.P[T.in_level] * T.cin);
    }
    // option x3: weight images, kept input images, one scratch image (dz, the concat
    // gradient's up half, and every input image of an inference pass)
    p.pack3 = p.s3 = nullptr;
    p.x3.assign(NC, nullptr);
    p.t3.assign(c->convt.size(), nullptr);
    {
        int64_t n3 = 0;
        for (int i = 0; i < NC; ++i) {
            const ConvL& L = c->conv[i];
            if (p.rt.conv[i].fwd != FAM_X3) continue;
            n3 = std::max(n3, p.P[L.level] * std::max(L.cin, L.cout));
            if (p.rt.conv[i].keep) p.x3[i] = b.take<uint16_t>(3 * p.P[L.level] * L.cin);
        }
        for (size_t k = 0; k < c->convt.size(); ++k) {
            const ConvTL& T = c->convt[k];
            if (p.rt.convt[k].fwd != FAM_X3) continue;
            n3 = std::max(n3, std::max(p.P[T.in_level] * T.cin, p.P[T.in_level - 1] * T.cout));
            if (p.rt.convt[k].keep) p.t3[k] = b.take<uint16_t>(3 * p.P[T.in_level] * T.cin);
        }
        if (p.rt.x3) {
            p.pack3 = b.take<uint16_t>(3 * c->pack_floats);
            p.s3 = b.take<uint16_t>(3 * n3);
        }
    }
    if (training) {
        int64_t gmax = p.P[0] * c->base;
        for (int i = 0; i < NC; ++i) {
            gmax = std::max(gmax, p.P[c->conv[i].level] * c->conv[i].cout);
            gmax = std::max(gmax, p.P[c->conv[i].level] * c->conv[i].cin);
        }
        p.g[0] = b.take<float>(gmax);
        p.g[1] = b.take<float>(gmax);
        p.g[2] = c->res ? b.take<float>(gmax) : nullptr;
        for (int l = 0; l < D; ++l) p.dcat[l] = b.take<float>(p.P[l] * 2 * c->ch(l));
        int64_t smax = 0, bmax = 0;
        for (int i = 1; i < NC; ++i) {
            const ConvL& L = c->conv[i];
            const WgradCfg& w = p.rt.conv[i].w;
            smax = std::max(smax, (int64_t)w.splits * 9 * L.cin * L.cout);
            bmax = std::max(bmax, (int64_t)w.splits * L.cout);
        }
        for (int blk = 1; blk <= 2 * D && c->res; ++blk) {
            const ConvL& L = c->conv[2 * blk];
            smax = std::max(smax, (int64_t)p.rt.skip[blk].w.splits * L.cin * L.cout);
        }
        for (size_t k = 0; k < c->convt.size(); ++k) {
            const ConvTL& T = c->convt[k];
            const WgradCfg& w = p.rt.convt[k].w;
            smax = std::max(smax, (int64_t)w.splits * T.cin * 4 * T.cout);
            bmax = std::max(bmax, (int64_t)w.splits * 4 * T.cout);
        }
        p.slab = b.take<float>(smax);
        int64_t pmax = (int64_t)RED_G * 2 * c->cmax;
        for (int i = 0; i < NC; ++i)  // dgrad epilogues: ceil(P/64) rows of 2*C (BM >= 64)
            pmax = std::max(pmax, (p.P[c->conv[i].level] / 64 + 1) * 2 * c->conv[i].cout);
        p.part = b.take<float>(pmax);
        p.part2 = b.take<float>((int64_t)STAT_G * 2 * c->cmax);
        p.hpart = b.take<float>((int64_t)WIDE_G *
                                std::max<int64_t>(10 * c->base, (int64_t)c->out_ch * (c->base + 1)));
        p.bslab = b.take<float>(std::max<int64_t>(bmax, 1));
        p.coef = b.take<float>(4 * (int64_t)c->cmax);  // BN-backward dz coefficients [4][C]
        p.gdz = (c->opt.dz_in_wgrad && !c->bf16) ? b.take<float>(gmax) : nullptr;
    } else {
        p.gdz = nullptr;
        p.g[0] = p.g[1] = p.g[2] = p.slab = p.part = p.part2 = p.hpart = p.bslab = p.coef = nullptr;
        for (int l = 0; l < D; ++l) p.dcat[l] = nullptr;
    }
    p.bytes = b.off + 256;
}

#define RUN(label, flop, expr)                            \
    do {                                                  \
        int rc_ = L.run(label, flop, [&]() { return (expr); }); \
        if (rc_) return rc_;                              \
    } while (0)

int stats_finalize(unet_ctx* c, Launcher& L, Plan& p, int i, int R, int64_t count, bool training,
                   const float* prm, float* bn_run, int64_t* bn_cnt) {
    const BnL& B = c->bn[i];
    const int C = B.C;
    hipStream_t s = L.s;
    if (!training) {
        RUN("bn_finalize", 0,
            k_bn_finalize_eval(C, prm + B.g, prm + B.b, bn_run + B.run, bn_run + B.run + C, BN_EPS,
                               p.scale[i], p.shift[i], s));
        return 0;
    }
    const float* part = p.stats;
    int G = R;
    if (R > STAT_G) {
        RUN("bn_stats_reduce", 0, k_reduce_rows(p.stats, R, 2 * C, p.stats2, STAT_G, s));
        part = p.stats2;
        G = STAT_G;
    }
    RUN("bn_finalize", 0,
        k_bn_finalize_train(part, G, C, (double)count, prm + B.g, prm + B.b,
                            bn_run ? bn_run + B.run : nullptr,
                            bn_run ? bn_run + B.run + C : nullptr, bn_cnt ? bn_cnt + i : nullptr,
                            BN_MOMENTUM, BN_EPS, p.scale[i], p.shift[i], p.mean[i], p.invstd[i],
                            s));
    return 0;
}

// Input operand of conv i: pointer, ld, offset, affine and the ReLU span (channels
// [0, relu) get ReLU after the affine: BN -> ReLU order).
struct Operand {
    const float* ptr;
    int ld, off;
    const float* scale;
    const float* shift;
    int relu;
};

Operand conv_input(unet_ctx* c, Plan& p, int i) {
    const ConvL& L = c->conv[i];
    const int D = c->depth;
    if (L.which == 1)
        return {p.y[i - 1], p.ldy[i - 1], p.offy[i - 1], p.scale[i - 1], p.shift[i - 1],
                c->bn_relu ? L.cin : 0};
    if (L.block >= 1 && L.block <= D)  // after a max-pool (already normalised + activated)
        return {p.pool[L.block - 1], L.cin, 0, nullptr, nullptr, 0};
    if (L.block > D) {  // concat: the skip half carries the encoder's BN (+ReLU) affine
        const int l = L.level;
        if (c->res) return {p.cat[l], 2 * c->ch(l), 0, nullptr, nullptr, 0};  // materialised
        return {p.cat[l], 2 * c->ch(l), 0, p.cat_scale[l], p.cat_shift[l],
                c->bn_relu ? c->ch(l) : 0};
    }
    return {nullptr, 0, 0, nullptr, nullptr, 0};  // conv 0: x
}

// Input operand of ConvT k: the second conv of the bottleneck / decoder block D + k, or the
// block's materialised output (residual network)
Operand convt_input(const unet_ctx* c, const Plan& p, int k) {
    const int b = c->depth + k, src = 2 * b + 1;
    if (c->res) return {p.out[b], p.ldout[b], p.offout[b], nullptr, nullptr, 0};
    return {p.y[src], p.ldy[src], p.offy[src], p.scale[src], p.shift[src],
            c->bn_relu ? c->convt[k].cin : 0};
}

// BN partial rows a row GEMM emits: one per 128-row group, whatever its tile (gemm_common.h
// row_epilogue), so the BN statistics do not depend on the tile choice
int bn_groups(int64_t M) { return (int)((M + 127) / 128); }

const float* bias_ptr(const float* prm, int64_t off) { return off >= 0 ? prm + off : nullptr; }

// XCD-aware block order for the f32 GEMMs (option xcd_remap: 0 none, 1 both, 2 row GEMMs
// only, 3 wgrad only; A/B runs)
int xcd_remap_on(const unet_ctx* c) { return c->opt.xcd_remap == 1 || c->opt.xcd_remap == 2; }
int xcd_remap_wgrad(const unet_ctx* c) { return c->opt.xcd_remap == 1 || c->opt.xcd_remap == 3; }

// weight image of a row GEMM: f32, or bf16 packed into the same slot (half its size)
void set_weights(const unet_ctx* c, RowGemmArgs& g, const float* img) {
    g.xcd = xcd_remap_on(c);
    if (c->bf16)
        g.bt16 = (const uint16_t*)img;
    else
        g.bt = img;
}

// point g's A operand at the prepared bf16 image `img` (lda = C channels)
void use_a16(const unet_ctx* c, const Plan& p, RowGemmArgs& g, const uint16_t* img, int C) {
    g.a16 = img;
    g.lda = C;
    g.aoff = 0;
    g.ascale = g.ashift = nullptr;
    g.arelu = 0;
    g.acoef = nullptr;
    g.zero16 = p.zero16;
    g.xcd = xcd16_on(c);
    g.tgm = c->opt.tile_group ? -1 : 0;
}

// device copies of the expand / compact tables (the host tables live in the context, so
// the asynchronous copy's source outlives it)
int upload_pad_tables(unet_ctx* c, Plan& p, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(p.ptab, c->pad_params.data(), sizeof(PadDesc) * c->pad_params.size(),
                                  hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(p.btab, c->pad_bn.data(), sizeof(PadDesc) * c->pad_bn.size(),
                           hipMemcpyHostToDevice, s);
    return (int)e;
}

// the pack job table of every 3x3 conv (but the Cin = in_channels first conv) and ConvT weight
// (dgrad images too when `dgrad`); false when the table overflows
bool build_pack_jobs(const unet_ctx* c, bool dgrad, PackJobs& jobs) {
    jobs.n = 0;
    int blocks = 0;
    auto add = [&](int64_t w, int64_t f, int64_t d, int cin, int cout, int kind) {
        PackJob& J = jobs.j[jobs.n++];
        J.w = w;
        J.f = f;
        J.d = dgrad ? d : -1;
        J.cin = cin;
        J.cout = cout;
        J.kind = kind;
        J.tx = ((kind == 0 ? cin : cout) + 31) / 32;
        J.ty = ((kind == 0 ? cout : cin) + 31) / 32;
        J.block0 = blocks;
        blocks += J.tx * J.ty;
    };
    for (const ConvL& C : c->conv) {
        if (C.pf < 0) continue;
        if (jobs.n >= MAX_PACK_JOBS) return false;
        add(C.w, C.pf, C.pd, C.cin, C.cout, 0);
    }
    for (const ConvTL& T : c->convt) {
        if (jobs.n >= MAX_PACK_JOBS) return false;
        add(T.w, T.pf, T.pd, T.cin, T.cout, 1);
    }
    return true;
}

// whether the plan of this context carries x3 weight images (make_plan's pack3)
// (which GEMMs run x3 depends on neither `training` nor the pixel count: any values do)
bool plan_has_pack3(const unet_ctx* c) { return make_routes(c, true, 0).x3; }

// the record of the training forward on workspace `ws` (the latest one: a workspace is reused)
unet_ctx::FwdRec* find_fwd(unet_ctx* c, const void* ws) {
    for (auto& r : c->fwd_recs)
        if (r.ws == ws) return &r;
    return nullptr;
}

unet_ctx::FwdRec* note_fwd(unet_ctx* c, const void* ws) {
    unet_ctx::FwdRec* r = find_fwd(c, ws);
    if (!r && c->fwd_recs.size() < unet_ctx::MAX_FWD_RECS) {
        c->fwd_recs.push_back({});
        r = &c->fwd_recs.back();
    }
    if (!r) r = &*std::min_element(c->fwd_recs.begin(), c->fwd_recs.end(),
                                   [](const unet_ctx::FwdRec& a, const unet_ctx::FwdRec& b) { return a.seq < b.seq; });
    r->ws = ws;
    r->opt = c->opt;
    r->used_pp = false;
    r->pp_gen = c->pp_gen;
    r->seq = ++c->fwd_seq;
    return r;
}

// whether [a, a + na) and [b, b + nb) floats share an address
bool ranges_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na > 0 && nb > 0 && a0 < b0 + 4 * (uint64_t)nb && b0 < a0 + 4 * (uint64_t)na;
}

// ------------------------------------------------------------------------------------
// Describing and launching a GEMM.  A site fills RowGemmArgs / WgradArgs as the f32 /
// register-staged kernels read them and names the image where its family (Route) reads one;
// run_rowgemm / run_wgrad switch the operands over, build the label and launch the plan's tile.
// ------------------------------------------------------------------------------------
// what the launch helpers of one forward / backward pass share
struct Pass {
    unet_ctx* c;
    Plan& p;
    Launcher L;
};

// a row GEMM over the pixels of `level`, as the plan fixed it
RowGemmArgs rowgemm_at(const Plan& p, int level, const RowGeom& q) {
    RowGemmArgs g{};
    g.zero16 = p.zero16;
    g.H = p.H >> level;
    g.W = q.W;
    g.M = q.M;
    g.N = q.N;
    g.K = q.K;
    g.C = q.K / gather_taps(q.amode);
    g.amode = q.amode;
    g.emode = q.emode;
    g.cout = q.cout;
    return g;
}

// a weight gradient over the pixels of `level`, split as wc says
WgradArgs wgrad_at(const unet_ctx* c, const Plan& p, int level, const WgradCfg& wc) {
    WgradArgs w{};
    w.H = p.H >> level;
    w.W = p.W >> level;
    w.P = (int)p.P[level];
    w.pps = wc.pps;
    w.splits = wc.splits;
    w.slab = p.slab;
    w.bf16 = c->bf16;
    return w;
}

// A (row GEMM) / A' (weight gradient) = op(a)
template <class Args>
void set_operand(Args& g, const Operand& a) {
    g.a = a.ptr;
    g.lda = a.ld;
    g.aoff = a.off;
    g.ascale = a.scale;
    g.ashift = a.shift;
    g.arelu = a.relu;
}

// E_STORE_BN dgrad epilogue: the result is the `do` of BN layer j, so the store also emits that
// layer's partials (masked first by the ReLU after the BN in BN -> ReLU order)
void bn_epilogue(const unet_ctx* c, const Plan& p, RowGemmArgs& g, int j) {
    g.ey = p.y[j];
    g.ldey = p.ldy[j];
    g.offey = p.offy[j];
    if (c->bn_relu) {
        g.escale = p.scale[j];
        g.eshift = p.shift[j];
    }
    g.stats = p.part;
}

// the scratch image of a family (dz, the concat gradient's up half, an inference pass's inputs)
uint16_t* scratch_image(const Plan& p, Family fam) { return fam == FAM_X3 ? p.s3 : p.s16; }

// the operand image conv i's forward GEMM reads: the one kept for its weight gradient, else
// scratch (residual network, bf16: the block's first conv shares its image with the skip GEMM,
// which runs after the second conv has reused the scratch image)
uint16_t* conv_image(const unet_ctx* c, const Plan& p, int i) {
    if (p.rt.conv[i].fwd == FAM_X3) return p.x3[i] ? p.x3[i] : p.s3;
    return p.x16[i] ? p.x16[i] : (c->res && c->conv[i].which == 0) ? p.r16 : p.s16;
}

// channels [coff, coff + n) of op(a) into the bf16 / x3 image img ([M][ld]) at the same offset
int prep_image(Launcher& L, Family fam, const Operand& a, int coff, int n, int64_t M, uint16_t* img,
               int ld) {
    const float* sc = a.scale ? a.scale + coff : nullptr;
    const float* sh = a.shift ? a.shift + coff : nullptr;
    const int relu = std::min(std::max(a.relu - coff, 0), n);
    if (fam == FAM_X3)
        RUN("prep_x3", 0, k_to_x3(a.ptr, a.ld, a.off + coff, n, sc, sh, relu, M, img, ld, coff, L.s));
    else
        RUN("prep16", 0, k_to_bf16(a.ptr, a.ld, a.off + coff, n, sc, sh, relu, M, img + coff, L.s, ld));
    return 0;
}

// the weight gradient reads images instead: A' = the forward's kept image `img` ([pixels][CA]),
// B' = the family's scratch image ([pixels][CB])
void use_images(const unet_ctx* c, const Plan& p, WgradArgs& w, Family fam, const uint16_t* img) {
    w.a = (const float*)img;
    w.lda = w.CA;
    w.aoff = 0;
    w.ascale = w.ashift = nullptr;
    w.arelu = 0;
    w.b = (const float*)scratch_image(p, fam);
    w.ldb = w.CB;
    w.boff = 0;
    w.by = nullptr;
    w.bcoef = nullptr;
    w.zero16 = p.zero16;
    w.xcd = fam == FAM_X3 ? 1 : xcd16_on(c);
}

// One row GEMM of family `fam` on the plan's tile.  g: the GEMM as the f32 / register-staged kernel
// reads it, and in g.a16 the prepared image ([pixels][g.C]) the other two families read instead.
// wimg: the weight image in the pack region (f32, or bf16 in the same slot; the x3 copy of the
// region holds its x3 image at 3x the offset), or the 1x1 skip parameter itself.
int run_rowgemm(Pass& ps, const char* site, int layer, double flop, Family fam, const Tile& t,
                const float* wimg, RowGemmArgs& g) {
    unet_ctx* c = ps.c;
    Launcher& L = ps.L;
    if (fam == FAM_X3) {
        use_x3(c, ps.p, g, g.a16, g.C, ps.p.pack3 + 3 * (wimg - ps.p.pack));
        RUN(tile_label(site, "x3", t.tag, t, nullptr, layer), flop, launch_rowgemm_x3(g, t.id, L.s));
        return 0;
    }
    set_weights(c, g, wimg);
    if (fam == FAM_DMA16) {
        use_a16(c, ps.p, g, g.a16, g.C);
        RUN(tile_label(site, "rg16", t.tag, t, "s", layer), flop, launch_rowgemm16(g, t.id, L.s));
        return 0;
    }
    RUN(tile_label(site, "rowgemm", "", t, "x", layer, t.tag), flop, launch_rowgemm(g, t.id, L.s));
    return 0;
}

// One weight gradient of family `fam`, tiled and split as wc says.
int run_wgrad(Pass& ps, const char* site, int layer, double flop, Family fam, const WgradCfg& wc,
              const WgradArgs& w) {
    Launcher& L = ps.L;
    if (fam == FAM_X3) {
        RUN(tile_label(site, "wx3", wc.t->tag, *wc.t, nullptr, layer), flop, launch_wgrad_x3(w, wc.t->id, L.s));
    } else if (fam == FAM_DMA16) {
        // (the tap-row kernels are 3x3 only)
        RUN(tile_label(site, "wg16", w.amode == G_CONV3 ? wc.t16->tag : "", *wc.t16, "s", layer), flop,
            launch_wgrad16(w, wc.t16->id, L.s));
    } else {
        RUN(tile_label(site, "wgrad", wc.t->tag, *wc.t, "x", layer), flop, launch_wgrad(w, wc.t->id, L.s));
    }
    return 0;
}

// rec: this training forward's record (nullptr: an eval forward, no backward follows)
int forward_impl(unet_ctx* c, const float* prm, float* bn_run, int64_t* bn_cnt, const float* x,
                 float* logits, Plan& p, bool training, unet_ctx::FwdRec* rec, hipStream_t s) {
    Pass ps{c, p, Launcher{c, s}};
    Launcher& L = ps.L;
    const int H = p.H, W = p.W, D = c->depth, NC = c->nconv();
    // 1. weight images for the row GEMMs: re-packed every call (params may have changed through
    //    the optimizer or load_state_dict; ~0.1 ms of HBM traffic per step at config 2) unless
    //    the fused AdamW of unet_adamw_repack wrote them for exactly these parameters (r06)
    const bool use_pp = c->pp_ok && c->pp_src == prm && c->pp && (!p.pack3 || c->pp3);
    if (rec) {
        rec->used_pp = use_pp;
        rec->pp_gen = c->pp_gen;
    }
    if (use_pp) {
        p.pack = c->pp;
        if (p.pack3) p.pack3 = c->pp3;
    } else {
        PackJobs jobs{};
        if (!build_pack_jobs(c, training, jobs)) return fail(c, UNET_ERR_INTERNAL, "pack job table full");
        if (jobs.n) RUN("pack", 0, k_pack_all(jobs, prm, p.pack, c->bf16, s));
        // option x3: the whole region as rows of 32 floats (every image 32-aligned)
        if (p.pack3)
            RUN("pack", 0, k_to_x3(p.pack, 32, 0, 32, nullptr, nullptr, 0, c->pack_floats / 32, p.pack3,
                                   32, 0, s));
    }
    // the residual blocks' 1x1 skip weights: written on every call, next to the conv images
    // (whichever buffer holds those), so they are never stale
    for (int b = 1; b <= 2 * D && c->res && c->bf16; ++b)
        RUN("pack", 0, k_pack_1x1_bf16(prm + c->skip_w[b], (uint16_t*)(p.pack + c->skip_pf[b]),
                                       (uint16_t*)(p.pack + c->skip_pd[b]), c->conv[2 * b].cin,
                                       c->conv[2 * b].cout, s));
    for (int b = 1; b <= 2 * D && c->res && !c->bf16 && training; ++b)
        RUN("pack", 0, k_pack_1x1_t(prm + c->skip_w[b], p.pack + c->skip_pd[b], c->conv[2 * b].cin,
                                    c->conv[2 * b].cout, s));
    // 2. concat affine: identity on the up-sampled half (no BN between ConvT and concat)
    for (int l = 0; l < D; ++l) {
        const int C = c->ch(l), uo = c->up_off(l);
        RUN("fill", 0, k_fill(p.cat_scale[l] + uo, C, 1.f, s));
        RUN("fill", 0, k_fill(p.cat_shift[l] + uo, C, 0.f, s));
    }
    if (p.zero16) RUN("fill", 0, (int)hipMemsetAsync(p.zero16, 0, 256, s));
    // in_channels == 1: NCHW == NHWC; keep a private copy for the conv-0 wgrad
    RUN("copy_x", 0, (int)hipMemcpyAsync(p.x_nhwc, x, sizeof(float) * p.P[0] * c->in_ch,
                                         hipMemcpyDeviceToDevice, s));
    const float* xin = p.x_nhwc;

    auto conv = [&](int i) -> int {
        const ConvL& C = c->conv[i];
        const Route& rt = p.rt.conv[i];
        const int64_t M = p.P[C.level];
        if (rt.fwd == FAM_NONE) {
            const int R = wide_g(M);
            RUN("conv_first_fwd", 2.0 * M * 9 * C.cout,
                k_conv_first_fwd(xin, prm + C.w, bias_ptr(prm, C.b), p.y[0], (int)M, H >> C.level,
                                 W >> C.level, C.cout, c->bn_relu ? 0 : 1, p.stats, R, s));
            return stats_finalize(c, L, p, i, R, M, training, prm, bn_run, bn_cnt);
        }
        const Operand a = conv_input(c, p, i);
        RowGemmArgs g = rowgemm_at(p, C.level, rt.f.g);
        set_operand(g, a);
        g.out = p.y[i];
        g.ldo = p.ldy[i];
        g.ooff = p.offy[i];
        g.bias = bias_ptr(prm, C.b);
        g.stats = p.stats;
        if (rt.fwd != FAM_REG) {
            uint16_t* img = conv_image(c, p, i);
            if (rt.up == W_PREP) {  // the whole image (over a skip half the max-pool may have stored)
                if (int rc = prep_image(L, rt.fwd, a, 0, C.cin, M, img, C.cin)) return rc;
            } else if (rt.skip == W_PREP) {  // the ConvT stored the up half: convert the skip half
                if (int rc = prep_image(L, rt.fwd, a, c->skip_off(C.level), c->ch(C.level), M, img, C.cin))
                    return rc;
            }  // (else the max-pool, or the ConvT and the max-pool, stored the whole image)
            g.a16 = img;
        }
        if (int rc = run_rowgemm(ps, "conv_fwd", i, 2.0 * M * C.cout * 9 * C.cin, rt.fwd, *rt.f.t,
                                 p.pack + C.pf, g))
            return rc;
        return stats_finalize(c, L, p, i, bn_groups(M), M, training, prm, bn_run, bn_cnt);
    };
    auto convT = [&](int k) -> int {
        const ConvTL& T = c->convt[k];
        const Route& rt = p.rt.convt[k];
        const int lo = T.in_level - 1;
        const Operand a = convt_input(c, p, k);
        RowGemmArgs g = rowgemm_at(p, T.in_level, rt.f.g);
        set_operand(g, a);
        g.out = p.cat[lo];
        g.ldo = 2 * c->ch(lo);
        g.ooff = c->up_off(lo);
        g.bias = prm + T.b;
        if (rt.fwd != FAM_REG) {
            const bool x3 = rt.fwd == FAM_X3;
            uint16_t* kept = x3 ? p.t3[k] : p.t16[k];
            uint16_t* img = kept ? kept : x3 ? p.s3 : p.s16;
            if (int rc = prep_image(L, rt.fwd, a, 0, T.cin, g.M, img, T.cin)) return rc;
            g.a16 = img;
            // option convt16 (training): the up half of the decoder's concat goes straight into
            // that conv's kept operand image, its only reader (identity affine); the conv's prep
            // pass then converts the skip half only, or nothing where the max-pool stored it
            const int idec = 2 * (D + 1 + k);
            if (p.rt.conv[idec].up == W_CONVT) (x3 ? g.out3 : g.out16) = conv_image(c, p, idec);
        }
        return run_rowgemm(ps, "convT_fwd", 100 + k, 2.0 * g.M * g.N * g.K, rt.fwd, *rt.f.t,
                           p.pack + T.pf, g);
    };

    // residual block b closes with out = ReLU(BN2(z2) + skip(x)) (mod.py:86)
    auto block_out = [&](int b) -> int {
        const ConvL& CL = c->conv[2 * b];
        const Route& rt = p.rt.skip[b];
        const int i2 = 2 * b + 1;
        const int64_t M = p.P[CL.level];
        if (rt.fwd == FAM_NONE) {  // Cin = 1: the skip is a per-channel scale of the image
            RUN("res_out", 0, k_res_first_fwd(xin, prm + c->skip_w[b], p.y[i2], p.scale[i2],
                                              p.shift[i2], M, CL.cout, p.out[b], p.ldout[b],
                                              p.offout[b], s));
            return 0;
        }
        RowGemmArgs g = rowgemm_at(p, CL.level, rt.f.g);
        set_operand(g, conv_input(c, p, 2 * b));
        g.out = p.out[b];
        g.ldo = p.ldout[b];
        g.ooff = p.offout[b];
        g.ey = p.y[i2];
        g.ldey = p.ldy[i2];
        g.offey = p.offy[i2];
        g.escale = p.scale[i2];
        g.eshift = p.shift[i2];
        // LDS-DMA: from the image conv1 read (rounded once, read twice)
        if (rt.fwd == FAM_DMA16) g.a16 = conv_image(c, p, 2 * b);
        // (f32: the torch layout [co][ci] of the parameter is already Bt[n][k])
        return run_rowgemm(ps, "skip_fwd", b, 2.0 * M * CL.cout * CL.cin, rt.fwd, *rt.f.t,
                           c->bf16 ? p.pack + c->skip_pf[b] : prm + c->skip_w[b], g);
    };

    int rc;
    for (int b = 0; b <= D; ++b) {
        if ((rc = conv(2 * b))) return rc;
        if ((rc = conv(2 * b + 1))) return rc;
        if (c->res && (rc = block_out(b))) return rc;
        if (b < D) {
            const int i = 2 * b + 1, C = c->ch(b);
            if (c->res)
                RUN("maxpool_fwd", 0,
                    k_maxpool_bn(p.out[b], p.ldout[b], p.offout[b], nullptr, nullptr, 0, p.N, H >> b,
                                 W >> b, C, p.pool[b], p.idx[b], s));
            else {
                // x3 (r05) / bf16 training (r06): op(pooled) straight into the operand image of the
                // next encoder block's first conv (no f32 pooled tensor, no prep pass)
                const int j = 2 * (b + 1);
                uint16_t *out3 = nullptr, *o16 = nullptr, *s16 = nullptr, *s3 = nullptr;
                if (p.rt.conv[j].up == W_POOL) (p.rt.conv[j].fwd == FAM_X3 ? out3 : o16) = conv_image(c, p, j);
                // (r06) the skip half of the decoder conv at this level (its ConvT stores the
                // up half, option convt16): op(BN(y)) as that conv's kept operand image
                const int idec = 2 * (2 * D - b);
                if (p.rt.conv[idec].skip == W_POOL)
                    (p.rt.conv[idec].fwd == FAM_X3 ? s3 : s16) = conv_image(c, p, idec);
                RUN("maxpool_fwd", 0,
                    k_maxpool_bn(p.y[i], p.ldy[i], p.offy[i], p.scale[i], p.shift[i],
                                 c->bn_relu ? 1 : 0, p.N, H >> b, W >> b, C,
                                 out3 || o16 ? nullptr : p.pool[b],  // (its images are the only readers)
                                 p.idx[b], s, out3, o16, s16, s3, c->conv[idec].cin, c->skip_off(b)));
            }
        }
    }
    for (int k = 0; k < D; ++k) {
        if ((rc = convT(k))) return rc;
        const int b = D + 1 + k;
        if ((rc = conv(2 * b))) return rc;
        if ((rc = conv(2 * b + 1))) return rc;
        if (c->res && (rc = block_out(b))) return rc;
    }
    const int last = NC - 1;
    if (c->res)
        RUN("head_fwd", 2.0 * p.P[0] * c->base * c->out_ch,
            k_head_fwd(p.out[2 * D], c->base, nullptr, nullptr, 0, prm + c->head_w, prm + c->head_b,
                       c->out_ch, (int)p.P[0], H * W, logits, s));
    else
        RUN("head_fwd", 2.0 * p.P[0] * c->base * c->out_ch,
            k_head_fwd(p.y[last], c->base, p.scale[last], p.shift[last], c->bn_relu ? 1 : 0,
                       prm + c->head_w, prm + c->head_b, c->out_ch, (int)p.P[0], H * W, logits, s));
    return 0;
}

int backward_impl(unet_ctx* c, const float* prm, const float* dlogits, float* grads, Plan& p,
                  hipStream_t s) {
    Pass ps{c, p, Launcher{c, s}};
    Launcher& L = ps.L;
    const int H = p.H, W = p.W, D = c->depth, NC = c->nconv();
    int rc;
    // (weight gradients run on the same stream as the dgrad chain: a second stream measured
    // 1 % slower, every GEMM fills the chip on its own)
    // BatchNorm backward is fused: the producer of `do` (head_bwd, a dgrad epilogue,
    // maxpool_bwd) leaves {sum do, sum do*y} column partials in p.part (do already masked by
    // the following ReLU in BN -> ReLU order); this finalize turns them into dgamma, dbeta
    // and the per-channel coefficients of dz = A do + B (y - mean) + C (masked by [y > 0] in
    // ReLU -> BN order).
    auto bn_finalize = [&](int i, int R) -> int {
        const ConvL& C = c->conv[i];
        const BnL& B = c->bn[i];
        const float* part = p.part;
        int G = R;
        if (R > STAT_G) {
            RUN("bn_bwd_reduce", 0, k_reduce_rows(p.part, R, 2 * C.cout, p.part2, STAT_G, s));
            part = p.part2;
            G = STAT_G;
        }
        RUN("bn_bwd_finalize", 0,
            k_bn_bwd_finalize2(part, G, C.cout, (double)p.P[C.level], prm + B.g, p.mean[i],
                               p.invstd[i], p.coef, grads + B.g, grads + B.b, s));
        return 0;
    };
    // dz = A do + B (y - mean) + C as one elementwise pass over do, or (option dz_in_wgrad)
    // inside the weight gradient's B' loader, which also stores it for the dgrad
    const int dz_mask = c->bn_relu ? 0 : 1;
    // what the dz pass of an encoder block's second conv recomputes its `do` from where the
    // route says pool_fuse: the max-pool backward's inputs (the encoder loop fills it)
    DzPool pool_src;
    // conv i backward from do_i (dense [P][cout]).
    // dgrad -> dx (ld ldx), with the epilogue the plan gave it (rt.d.g.emode): where dx is the
    // `do` of BN layer i-1 (second conv of a block) it also emits that layer's partials;
    // *rows = their count.
    auto conv_bwd = [&](int i, const float* dout, float* dx, int ldx, int* rows) -> int {
        const ConvL& C = c->conv[i];
        const Route& rt = p.rt.conv[i];
        const int Hl = H >> C.level, Wl = W >> C.level;
        const int64_t P = p.P[C.level];
        const double flop = 2.0 * P * C.cout * 9 * C.cin;
        if (rt.wgrad == FAM_NONE) {
            RUN("conv_first_wgrad", 2.0 * P * 9 * C.cout,
                k_conv_first_wgrad(p.x_nhwc, dout, p.y[0], p.coef, (int)P, Hl, Wl, C.cout, dz_mask,
                                   p.hpart, wide_g(P), grads + C.w,
                                   C.b >= 0 ? grads + C.b : nullptr, s));
            return 0;
        }
        const WgradCfg& wc = rt.w;
        WgradArgs w = wgrad_at(c, p, C.level, wc);
        w.CA = C.cin;
        w.amode = G_CONV3;
        w.CB = C.cout;
        w.bmode = G_IDENT;
        w.Mw = 9 * C.cin;
        w.Nw = C.cout;
        // the dz pass (dz_pass.h).  Outputs by family: x3 -> the x3 image (and the conv bias's
        // column partials); LDS-DMA dgrad / wgrad -> the bf16 image, with the f32 dz in place
        // only while a register-staged kernel still consumes it; else f32 in place
        const bool x3 = rt.wgrad == FAM_X3;
        const bool wg16 = !x3 && rt.wgrad == FAM_DMA16, rg16 = !x3 && rt.dgrad == FAM_DMA16;
        const bool dz16 = rg16 || wg16;
        const bool f32 = !x3 && (!wg16 || !(dx && rg16));
        // option dz_in_wgrad: the weight gradient's B' loader forms dz from do and y (the
        // bn_dz pass disappears) and its first A'-tile blocks store it for the dgrad (both BN
        // orders; BN -> ReLU forms dz unmasked, do already carries the ReLU mask)
        const bool dzw = rt.dzw;
        if (!dzw) {
            DzArgs z;
            z.y = p.y[i], z.ld = p.ldy[i], z.off = p.offy[i];
            z.P = P, z.C = C.cout, z.coef = p.coef, z.mask = dz_mask;
            // the image outputs can take a do that its producer did not store
            if (rt.pool_fuse && (x3 || dz16)) {
                if (f32) return fail(c, UNET_ERR_INTERNAL, "pool_fuse: conv %d needs an f32 dz", i);
                z.pool = pool_src;
                z.pool.H = Hl, z.pool.W = Wl, z.N = p.N;
            } else if (rt.head_fuse && (x3 || dz16)) {
                if (f32) return fail(c, UNET_ERR_INTERNAL, "head_fuse: conv %d needs an f32 dz", i);
                z.head = DzHead{dlogits, prm + c->head_w, p.scale[i], p.shift[i], c->bn_relu ? 1 : 0};
            } else {
                z.d = const_cast<float*>(dout);
            }
            z.f32 = f32;
            z.dz16 = dz16 ? p.s16 : nullptr;
            z.dz3 = x3 ? p.s3 : nullptr;
            z.bpart = x3 && C.b >= 0 ? p.part : nullptr;
            RUN("bn_dz", 0, k_bn_dz(z, s));
        }
        if (x3) {
            // the weight gradient from the forward's kept input image and dz, the input gradient from dz
            if (C.b >= 0) {  // many 256-row partials: one two-level reduction (as the BN statistics)
                const int G = x3_dz_blocks(P);
                if (G > STAT_G) {
                    RUN("bias_grad", 0, k_reduce_rows(p.part, G, C.cout, p.part2, STAT_G, s));
                    RUN("bias_grad", 0, k_sum_partials(p.part2, STAT_G, C.cout, grads + C.b, s));
                } else {
                    RUN("bias_grad", 0, k_sum_partials(p.part, G, C.cout, grads + C.b, s));
                }
            }
            use_images(c, p, w, FAM_X3, p.x3[i]);
        } else {
            w.xcd = xcd_remap_wgrad(c);
            set_operand(w, conv_input(c, p, i));
            w.b = dout;
            w.ldb = C.cout;
            w.by = p.y[i];
            w.ldby = p.ldy[i];
            w.offby = p.offy[i];
            w.bcoef = dzw ? p.coef : nullptr;
            w.dzout = dzw ? p.gdz : nullptr;
            w.bdznomask = dz_mask ? 0 : 1;
            w.lddz = C.cout;
            w.bias_slab = C.b >= 0 ? p.bslab : nullptr;
            if (wg16) use_images(c, p, w, FAM_DMA16, p.x16[i]);
        }
        if ((rc = run_wgrad(ps, "conv_wgrad", i, flop, rt.wgrad, wc, w))) return rc;
        RUN("wgrad_reduce", 0,
            k_slab_reduce(p.slab, wc.splits, w.Mw, w.Nw, 0, C.cin, C.cout, grads + C.w, s));
        if (rt.wgrad != FAM_X3 && C.b >= 0)
            RUN("bias_grad", 0, k_bias_reduce(p.bslab, wc.splits, 1, C.cout, grads + C.b, s));
        if (!dx) return 0;
        // the input gradient: A = dz (f32: in place in dout, or the copy the weight gradient
        // stored; LDS-DMA / x3: its scratch image)
        RowGemmArgs g = rowgemm_at(p, C.level, rt.d.g);
        g.a = dzw ? p.gdz : dout;
        g.lda = C.cout;
        g.ay = p.y[i];
        g.lday = p.ldy[i];
        g.offay = p.offy[i];
        g.a16 = scratch_image(p, rt.dgrad);
        g.out = dx;
        g.ldo = ldx;
        if (g.emode == E_STORE_BN) bn_epilogue(c, p, g, i - 1);
        if (rows) *rows = bn_groups(P);
        return run_rowgemm(ps, "conv_dgrad", i, flop, rt.dgrad, *rt.d.t, p.pack + C.pd, g);
    };
    // ConvT k backward: dOut = up half of dcat[lo]; dx = `do` of its input's BN (partials ->
    // rows)
    auto convT_bwd = [&](int k, float* dx, int* rows) -> int {
        const ConvTL& T = c->convt[k];
        const Route& rt = p.rt.convt[k];
        const int src = 2 * (D + k) + 1;
        const int lo = T.in_level - 1;
        const int Hi = H >> T.in_level, Wi = W >> T.in_level;
        const int64_t Pin = p.P[T.in_level];
        const double flop = 2.0 * Pin * T.cin * 4 * T.cout;
        const Operand up{p.dcat[lo], 2 * c->ch(lo), c->up_off(lo), nullptr, nullptr, 0};
        // the up half of the concat gradient as a bf16 / x3 image in the scratch image: B'
        // (gathered 2x2) of an image weight gradient, A of an image input gradient
        const bool wimg = rt.wgrad != FAM_REG;
        if (wimg && (rc = prep_image(L, rt.wgrad, up, 0, T.cout, p.P[lo], scratch_image(p, rt.wgrad), T.cout)))
            return rc;
        const WgradCfg& wc = rt.w;
        WgradArgs w = wgrad_at(c, p, T.in_level, wc);
        w.xcd = xcd_remap_wgrad(c);
        set_operand(w, convt_input(c, p, k));
        w.CA = T.cin;
        w.amode = G_IDENT;
        w.b = up.ptr;
        w.ldb = up.ld;
        w.boff = up.off;
        w.CB = T.cout;
        w.bmode = G_UP2;
        w.bias_slab = p.bslab;
        w.Mw = T.cin;
        w.Nw = 4 * T.cout;
        if (wimg) {  // from the forward's kept image; the bias gradient from its own pass
            use_images(c, p, w, rt.wgrad, rt.wgrad == FAM_X3 ? p.t3[k] : p.t16[k]);
            w.bias_slab = nullptr;
        }
        if ((rc = run_wgrad(ps, "convT_wgrad", 100 + k, flop, rt.wgrad, wc, w))) return rc;
        if (wimg)
            RUN("bias_grad", 0, k_up2_bias_partials(up.ptr, up.ld, up.off, Hi, Wi, Pin, T.cout, wc.pps,
                                                    wc.splits, p.bslab, s));
        RUN("wgrad_reduce", 0,
            k_slab_reduce(p.slab, wc.splits, w.Mw, w.Nw, 1, T.cin, T.cout, grads + T.w, s));
        RUN("bias_grad", 0, k_bias_reduce(p.bslab, wc.splits, 4, T.cout, grads + T.b, s));
        if (!wimg && rt.dgrad != FAM_REG &&
            (rc = prep_image(L, rt.dgrad, up, 0, T.cout, p.P[lo], scratch_image(p, rt.dgrad), T.cout)))
            return rc;
        RowGemmArgs g = rowgemm_at(p, T.in_level, rt.d.g);
        set_operand(g, up);
        g.a16 = scratch_image(p, rt.dgrad);
        g.out = dx;
        g.ldo = T.cin;
        if (g.emode == E_STORE_BN) bn_epilogue(c, p, g, src);
        *rows = bn_groups(Pin);
        return run_rowgemm(ps, "convT_dgrad", 100 + k, flop, rt.dgrad, *rt.d.t, p.pack + T.pd, g);
    };
    // gradient bucket b is final once stage bucket_stage[b] is done: record its event (a
    // channel-padded network first compacts the bucket's tensors into the caller's arena,
    // so its all-reduce can overlap the rest of the backward as well)
    auto stage_done = [&](int st) -> int {
        for (size_t b = 0; b < c->bucket_stage.size(); ++b) {
            if (c->bucket_stage[b] != st) continue;
            if (c->padded && c->bucket_p1[b] > c->bucket_p0[b])
                RUN("pad_compact", 0,
                    k_pad_copy(p.ptab + c->bucket_p0[b], c->bucket_p1[b] - c->bucket_p0[b],
                               c->bucket_pmax[b], p.pgrad, p.ugrad, 0, s));
            (void)hipEventRecord(c->bucket_ev[b], s);
        }
        return 0;
    };

    float* G0 = p.g[0];
    float* G1 = p.g[1];
    int R = 0;
    if (c->res) {
        // Residual block b from d(out) in G0: du = d(out)[out > 0] (+ BN2 partials); the skip
        // conv's weight / input gradients from du; BN2 + conv2, then BN1-ReLU + conv1 whose
        // input gradient is ADDED to the skip's in dx (ld ldx; null for the first block).
        auto block_bwd = [&](int b, float* dx, int ldx) -> int {
            const ConvL& CL = c->conv[2 * b];
            const Route& rt = p.rt.skip[b];
            const int i1 = 2 * b, i2 = 2 * b + 1;
            const int64_t P = p.P[CL.level];
            const double flop = 2.0 * P * CL.cin * CL.cout;
            // bf16 math: du's bf16 image with it, where an LDS-DMA skip GEMM reads it (the scratch
            // image is free until conv2's dz pass, which follows the skip's GEMMs)
            const bool du16 = rt.wgrad == FAM_DMA16 || rt.dgrad == FAM_DMA16;
            RUN("res_bwd_prep", 0, k_res_bwd_prep(G0, p.out[b], p.ldout[b], p.offout[b], p.y[i2], P,
                                                  CL.cout, p.part, RED_G, s, du16 ? p.s16 : nullptr));
            if (rt.wgrad == FAM_NONE) {
                RUN("skip_wgrad", 2.0 * P * CL.cout,
                    k_res_first_wgrad(p.x_nhwc, G0, (int)P, CL.cout, p.hpart, RED_G,
                                      grads + c->skip_w[b], s));
            } else {
                const WgradCfg& wc = rt.w;
                WgradArgs w = wgrad_at(c, p, CL.level, wc);
                w.xcd = xcd_remap_wgrad(c);
                set_operand(w, conv_input(c, p, i1));
                w.CA = CL.cin;
                w.amode = G_IDENT;
                w.b = G0;
                w.ldb = CL.cout;
                w.CB = CL.cout;
                w.bmode = G_IDENT;
                w.Mw = CL.cin;
                w.Nw = CL.cout;
                // A' = the forward's image of the block input (conv1 keeps it), B' = du's image
                if (rt.wgrad == FAM_DMA16) use_images(c, p, w, FAM_DMA16, p.x16[i1]);
                if ((rc = run_wgrad(ps, "skip_wgrad", b, flop, rt.wgrad, wc, w))) return rc;
                RUN("wgrad_reduce", 0, k_slab_reduce(p.slab, wc.splits, w.Mw, w.Nw, 2, CL.cin, CL.cout,
                                                     grads + c->skip_w[b], s));
                RowGemmArgs g = rowgemm_at(p, CL.level, rt.d.g);
                g.a = G0;
                g.lda = CL.cout;
                g.a16 = p.s16;
                g.out = dx;
                g.ldo = ldx;
                if ((rc = run_rowgemm(ps, "skip_dgrad", b, flop, rt.dgrad, *rt.d.t, p.pack + c->skip_pd[b], g)))
                    return rc;
            }
            if ((rc = bn_finalize(i2, RED_G))) return rc;
            if ((rc = conv_bwd(i2, G0, G1, CL.cout, &R))) return rc;
            if ((rc = bn_finalize(i1, R))) return rc;
            return conv_bwd(i1, G1, dx, ldx, nullptr);
        };
        RUN("head_bwd", 2.0 * p.P[0] * c->base * c->out_ch * 2,
            k_head_bwd(p.out[2 * D], c->base, nullptr, nullptr, 0, prm + c->head_w, c->out_ch,
                       (int)p.P[0], H * W, dlogits, G0, p.hpart, nullptr, wide_g(p.P[0]), s));
        RUN("head_grad", 0, k_sum_partials(p.hpart, wide_g(p.P[0]), c->out_ch * c->base + c->out_ch,
                                           grads + c->head_w, s));
        if ((rc = block_bwd(2 * D, p.dcat[0], 2 * c->base))) return rc;
        if ((rc = stage_done(0))) return rc;
        for (int k = D - 1; k >= 0; --k) {
            const int b = D + k;
            if ((rc = convT_bwd(k, G0, &R))) return rc;
            const int l = c->conv[2 * b].level;
            if (b > D) {
                if ((rc = block_bwd(b, p.dcat[l], 2 * c->ch(l)))) return rc;
            } else if ((rc = block_bwd(b, p.g[2], c->conv[2 * b].cin))) {
                return rc;
            }
            if ((rc = stage_done(D - k))) return rc;
        }
        for (int b = D - 1; b >= 0; --b) {
            const int C = c->ch(b);
            RUN("maxpool_bwd", 0,
                k_maxpool_bwd(p.g[2], p.idx[b], p.dcat[b], 2 * C, c->skip_off(b), nullptr, 0, 0,
                              nullptr, nullptr, p.N, H >> b, W >> b, C, G0, nullptr, RED_G, s));
            if ((rc = block_bwd(b, b > 0 ? p.g[2] : nullptr, b > 0 ? c->conv[2 * b].cin : 0)))
                return rc;
            if ((rc = stage_done(2 * D - b))) return rc;
        }
        return 0;
    }
    // ---- head + last decoder block (stage 0) ----
    const int last = NC - 1;
    // (r05) one output channel on the x3 path (r06: and on the bf16 path's LDS-DMA GEMMs): the
    // last conv's dz pass recomputes `do` = mask * dl * w from the logit gradient, so head_bwd
    // stores no full-resolution f32 `do`
    const bool head_fuse = p.rt.conv[last].head_fuse;
    RUN("head_bwd", 2.0 * p.P[0] * c->base * c->out_ch * 2,
        k_head_bwd(p.y[last], c->base, p.scale[last], p.shift[last], c->bn_relu ? 1 : 0,
                   prm + c->head_w, c->out_ch, (int)p.P[0], H * W, dlogits, head_fuse ? nullptr : G0,
                   p.hpart, p.part, wide_g(p.P[0]), s));
    RUN("head_grad", 0, k_sum_partials(p.hpart, wide_g(p.P[0]), c->out_ch * c->base + c->out_ch,
                                       grads + c->head_w, s));
    if ((rc = bn_finalize(last, wide_g(p.P[0])))) return rc;
    if ((rc = conv_bwd(last, G0, G1, c->base, &R))) return rc;
    if ((rc = bn_finalize(last - 1, R))) return rc;
    if ((rc = conv_bwd(last - 1, G1, p.dcat[0], 2 * c->base, nullptr))) return rc;
    if ((rc = stage_done(0))) return rc;
    // ---- ConvT k, then block D+k (the block whose output it up-samples) ----
    for (int k = D - 1; k >= 0; --k) {
        const int b = D + k;
        const int i1 = 2 * b + 1, i0 = 2 * b;
        if ((rc = convT_bwd(k, G0, &R))) return rc;
        if ((rc = bn_finalize(i1, R))) return rc;
        if ((rc = conv_bwd(i1, G0, G1, c->conv[i1].cin, &R))) return rc;
        if ((rc = bn_finalize(i0, R))) return rc;
        if (b > D) {
            const int l = c->conv[i0].level;  // input is CAT_l
            if ((rc = conv_bwd(i0, G1, p.dcat[l], 2 * c->ch(l), nullptr))) return rc;
        } else {
            // bottleneck: its input is pool[D-1]; G0 <- d pool[D-1]
            if ((rc = conv_bwd(i0, G1, G0, c->conv[i0].cin, nullptr))) return rc;
        }
        if ((rc = stage_done(D - k))) return rc;
    }
    // ---- encoders ----
    float* cur = G0;
    for (int b = D - 1; b >= 0; --b) {
        const int C = c->ch(b);
        const int i1 = 2 * b + 1, i0 = 2 * b;
        float* nxt = cur == G0 ? G1 : G0;
        // up to 2048 blocks on the large levels (512 left the pass at ~4.7 TB/s); the partial
        // rows fit: p.part holds P/64 + 1 rows of 2C for every conv of the level
        const int Gmp = wide_g(p.P[b]);
        const bool pool_fuse = p.rt.conv[i1].pool_fuse;
        pool_src = DzPool{};
        if (pool_fuse) {
            pool_src.dp = cur;
            pool_src.idx = p.idx[b];
            pool_src.dskip = p.dcat[b] + c->skip_off(b);
            pool_src.ldskip = 2 * C;
            pool_src.msc = c->bn_relu ? p.scale[i1] : nullptr;
            pool_src.msh = c->bn_relu ? p.shift[i1] : nullptr;
        }
        RUN("maxpool_bwd", 0,
            k_maxpool_bwd(cur, p.idx[b], p.dcat[b], 2 * C, c->skip_off(b), p.y[i1], p.ldy[i1],
                          p.offy[i1], c->bn_relu ? p.scale[i1] : nullptr,
                          c->bn_relu ? p.shift[i1] : nullptr, p.N, H >> b, W >> b, C,
                          pool_fuse ? nullptr : nxt, p.part, Gmp, s));
        cur = nxt;
        nxt = cur == G0 ? G1 : G0;
        if ((rc = bn_finalize(i1, Gmp))) return rc;
        if ((rc = conv_bwd(i1, cur, nxt, C, &R))) return rc;
        cur = nxt;
        nxt = cur == G0 ? G1 : G0;
        if ((rc = bn_finalize(i0, R))) return rc;
        if (b > 0) {
            if ((rc = conv_bwd(i0, cur, nxt, c->conv[i0].cin, nullptr))) return rc;
            cur = nxt;
        } else {
            if ((rc = conv_bwd(0, cur, nullptr, 0, nullptr))) return rc;
        }
        if ((rc = stage_done(2 * D - b))) return rc;
    }
    return 0;
}

bool shape_ok(const unet_ctx* c, int N, int H, int W) {
    const int q = 1 << std::max(c->depth, 4);  // every level even; >= 16 (model.py contract)
    return N >= 1 && H >= q && W >= q && H % q == 0 && W % q == 0;
}

}  // namespace

// ====================================== C ABI ======================================
extern "C" {

int unet_create(const unet_cfg* cfg, int device, unet_ctx** out) {
    if (!out) return UNET_ERR_INVALID;
    *out = nullptr;
    try {
        std::unique_ptr<unet_ctx> c(new unet_ctx());
        c->device = device;
        int cus = 0;  // (no device in a CPU-only process: keep the MI355X's 256)
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->cus = cus;
        else
            (void)hipGetLastError();
        if (cfg) {
            c->in_ch = cfg->in_channels;
            c->out_ch = cfg->out_channels;
            c->variant = cfg->variant;
            c->bf16 = cfg->math == UNET_MATH_BF16;
            if (cfg->math != UNET_MATH_F32 && cfg->math != UNET_MATH_BF16) return UNET_ERR_UNSUPPORTED;
            if (c->variant == UNET_VARIANT_MOD || c->variant == UNET_VARIANT_RES) {
                // mod.py:13-14 / :91-92 defaults base 64, depth 5
                c->base = cfg->base_filters > 0 ? cfg->base_filters : 64;
                c->depth = cfg->depth > 0 ? cfg->depth : 5;
            } else if ((cfg->base_filters > 0 && cfg->base_filters != 64) ||
                       (cfg->depth > 0 && cfg->depth != 4)) {
                return UNET_ERR_UNSUPPORTED;  // models/model.py:UNet has a fixed topology
            }
        }
        // The first conv kernel is specialised for a single input channel (every BASELINE
        // config); the GEMM tiles need 32-multiples of channels at every level (32-output
        // row tiles 13 / 14 and 32-channel wgrad tiles 8..10 for a 32-channel level 0) and the
        // channel-quad row kernels (pool, head, BN backward) a power-of-two channel count,
        // so the kernels run base 32, 64, 128 or 256.  Other base_filters (the reference
        // grid's 16 / 24 / 48, config/config.yaml; any multiple of 8 up to 256) run padded to
        // the next power of two >= 32 (unet_ctx::padded); the head's fused BN-partials path
        // handles up to 4 classes.
        // Per level: level 0 runs the next power of two >= 32 channels (the head and
        // first-conv kernels want a power-of-two channel-quad count), every deeper level the
        // next multiple of 32 of base_filters << l (a K-chunk is 32 channels of one tap), and
        // since r06 an odd multiple of 32 from 96 on the next multiple of 64 (below), so base
        // 16 pads level 0 only (16 -> 32, then 32, 64, ...: r03 padded every level 2x), base 48
        // levels 0 and 1 (48 -> 64, 96 -> 128, then 192, 384, ...), base 24 levels 0..2 (24 ->
        // 32, 48 -> 64, 96 -> 128).
        c->rbase = c->base;
        if (c->base < 8 || c->base > 256 || c->base % 8 || c->depth < 1 || c->depth > MAX_DEPTH)
            return UNET_ERR_UNSUPPORTED;
        c->padded = false;
        for (int l = 0; l <= c->depth; ++l) {
            int pc = 32;
            if (l == 0) {
                while (pc < c->rbase) pc <<= 1;
            } else {
                pc = ((c->rbase << l) + 31) / 32 * 32;
                // (r06) 96, 160, 224, ... channels run padded to the next multiple of 64: the
                // x3 GEMMs (f32 math on the bf16 matrix cores) take 64-multiples, and padded x3
                // beats the native f32 MFMA kernels (96 -> 128: 1.78x the FLOPs at ~2.2x the
                // rate; base 48's 96-channel level 1 and base 24's level 2)
                if (pc % 64 == 32 && pc >= 96) pc += 32;
            }
            c->chl[l] = pc;
            c->padded = c->padded || pc != (c->rbase << l);
        }
        c->base = c->chl[0];
        if ((c->variant != UNET_VARIANT_MODEL && c->variant != UNET_VARIANT_MOD &&
             c->variant != UNET_VARIANT_RES) || c->in_ch != 1 ||
            c->out_ch < 1 || c->out_ch > 4 || c->ch(c->depth) > 8192)
            return UNET_ERR_UNSUPPORTED;
        if ((c->padded || c->base < 64) && c->bf16)  // the bf16 kernels: 128-multiples of real channels
            return UNET_ERR_UNSUPPORTED;
        c->res = c->variant == UNET_VARIANT_RES;
        c->bn_relu = c->variant != UNET_VARIANT_MODEL;
        c->skip_first = c->bn_relu;
        // bf16 GEMMs: the BN -> ReLU networks of models/mod.py (UNet, ResUNet)
        if (c->bf16 && c->variant != UNET_VARIANT_MOD && c->variant != UNET_VARIANT_RES)
            return UNET_ERR_UNSUPPORTED;
        build_graph(c.get());
        *out = c.release();
        return UNET_OK;
    } catch (const std::bad_alloc&) {
        return UNET_ERR_NOMEM;
    } catch (...) {
        return UNET_ERR_INTERNAL;
    }
}

int unet_destroy(unet_ctx* c) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    for (auto e : c->bucket_ev) (void)hipEventDestroy(e);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    // (a retired buffer implies a live scratch; nothing allocated: no device call at all)
    void* const own[] = {c->pp,      c->pp3,       c->loss.p,    c->boundary.p, c->clahe.p,
                         c->elastic.p, c->surface.p, c->cc.p,    c->curve.p,   c->exportbuf.p,
                         c->lovasz.p,  c->morph.p};
    if (std::any_of(std::begin(own), std::end(own), [](void* p) { return p != nullptr; })) {
        (void)hipSetDevice(c->device);
        for (void* p : own)
            if (p) (void)hipFree(p);
        for (void* p : c->retired) (void)hipFree(p);
    }
    delete c;
    return UNET_OK;
    ABI_CATCH(c)
}

const char* unet_last_error(const unet_ctx* c) { return c ? c->err.c_str() : "null context"; }

int unet_num_params(const unet_ctx* c, int* n, int64_t* nf) {
    if (!c) return UNET_ERR_INVALID;
    if (n) *n = (int)c->params.size();
    if (nf) *nf = c->n_param_floats;
    return UNET_OK;
}

int unet_param_info(const unet_ctx* c, int i, const char** name, int* ndim, int64_t shape[4],
                    int64_t* offset) {
    ABI_TRY
    if (!c || i < 0 || i >= (int)c->params.size()) return UNET_ERR_INVALID;
    const ParamT& p = c->params[i];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = p.ndim;
    if (shape)
        for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
    if (offset) *offset = p.off;
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_num_bn(const unet_ctx* c, int* n, int64_t* nf) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    if (n) *n = c->nconv();
    if (nf) *nf = c->n_bn_floats;
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_bn_info(const unet_ctx* c, int i, const char** name, int* ch, int64_t* off) {
    ABI_TRY
    if (!c || i < 0 || i >= c->nconv()) return UNET_ERR_INVALID;
    if (name) *name = c->bn[i].name.c_str();
    if (ch) *ch = c->bn[i].rC;
    if (off) *off = c->bn[i].rrun;
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_workspace_size(unet_ctx* c, int N, int H, int W, int training, size_t* bytes) {
    ABI_TRY
    if (!c || !bytes) return UNET_ERR_INVALID;
    if (!shape_ok(c, N, H, W)) return fail(c, UNET_ERR_SHAPE, "bad shape N=%d H=%d W=%d", N, H, W);
    Plan p;
    make_plan(c, N, H, W, training != 0, nullptr, p);
    *bytes = p.bytes;
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_forward(unet_ctx* c, const float* params, float* bn_running, int64_t* bn_count,
                 const float* x, float* logits, void* ws, size_t ws_bytes, int N, int H, int W,
                 int training, unet_stream_t stream) {
    ABI_TRY
    if (!c || !params || !x || !logits || !ws) return c ? fail(c, UNET_ERR_INVALID, "null pointer") : UNET_ERR_INVALID;
    if (!ws_aligned(ws)) return fail(c, UNET_ERR_INVALID, "workspace %p is not %d-byte aligned", ws, WS_ALIGN);
    if (!shape_ok(c, N, H, W)) return fail(c, UNET_ERR_SHAPE, "bad shape N=%d H=%d W=%d", N, H, W);
    if (!training && !bn_running)
        return fail(c, UNET_ERR_INVALID, "eval forward needs running statistics");
    Plan p;
    make_plan(c, N, H, W, training != 0, nullptr, p);
    if (ws_bytes < p.bytes) return fail(c, UNET_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, p.bytes);
    make_plan(c, N, H, W, training != 0, (char*)ws, p);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, UNET_ERR_HIP, "hipSetDevice");
    if (!c->timing) c->ev_used = 0;
    unet_ctx::FwdRec* rec = training ? note_fwd(c, ws) : nullptr;
    const hipStream_t s = (hipStream_t)stream;
    if (!c->padded)
        return forward_impl(c, params, bn_running, bn_count, x, logits, p, training != 0, rec, s);
    // narrow network: torch-layout arenas -> padded arenas, forward, running stats back
    int r = upload_pad_tables(c, p, s);
    if (!r) r = k_pad_copy(p.ptab, (int)c->pad_params.size(), c->pad_max_numel, params, p.pprm, 1, s);
    if (!r && bn_running)
        r = k_pad_copy(p.btab, (int)c->pad_bn.size(), c->pad_bn_max, bn_running, p.pbn, 1, s);
    if (r) return fail(c, UNET_ERR_HIP, "channel-padding expand: %d", r);
    r = forward_impl(c, p.pprm, bn_running ? p.pbn : nullptr, bn_count, x, logits, p,
                     training != 0, rec, s);
    if (r) return r;
    if (training && bn_running &&
        k_pad_copy(p.btab, (int)c->pad_bn.size(), c->pad_bn_max, p.pbn, bn_running, 0, s))
        return fail(c, UNET_ERR_HIP, "channel-padding compact (running stats)");
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_backward(unet_ctx* c, const float* params, const float* dlogits, float* grads, void* ws,
                  size_t ws_bytes, int N, int H, int W, unet_stream_t stream) {
    ABI_TRY
    if (!c || !params || !dlogits || !grads || !ws) return c ? fail(c, UNET_ERR_INVALID, "null pointer") : UNET_ERR_INVALID;
    if (!ws_aligned(ws)) return fail(c, UNET_ERR_INVALID, "workspace %p is not %d-byte aligned", ws, WS_ALIGN);
    if (!shape_ok(c, N, H, W)) return fail(c, UNET_ERR_SHAPE, "bad shape N=%d H=%d W=%d", N, H, W);
    const unet_ctx::FwdRec* rec = find_fwd(c, ws);
    if (!rec) return fail(c, UNET_ERR_INVALID, "backward without a training forward on this workspace");
    for (const OptionDesc& d : OPTION_TABLE)
        if (c->opt.*d.field != rec->opt.*d.field)
            return fail(c, UNET_ERR_INVALID,
                        "option '%s' changed between the training forward (%d) and its backward "
                        "(%d): the workspace plan depends on it",
                        d.name, rec->opt.*d.field, c->opt.*d.field);
    Plan p;
    make_plan(c, N, H, W, true, nullptr, p);
    if (ws_bytes < p.bytes) return fail(c, UNET_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, p.bytes);
    make_plan(c, N, H, W, true, (char*)ws, p);
    // (r06) this forward read the fused AdamW's weight images: they must not have been rewritten
    // since.  A forward that packed into its own workspace finds its images there, whatever
    // the context's hold by now.
    if (rec->used_pp) {
        if (c->pp_gen != rec->pp_gen)
            return fail(c, UNET_ERR_INVALID,
                        "the weight images the training forward used were rewritten before its "
                        "backward (unet_adamw_repack in between)");
        p.pack = c->pp;
        if (p.pack3) p.pack3 = c->pp3;
    }
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, UNET_ERR_HIP, "hipSetDevice");
    if (c->bucket_ev.empty()) {
        c->bucket_ev.resize(c->bucket_off.size());
        for (auto& e : c->bucket_ev) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    }
    const hipStream_t s = (hipStream_t)stream;
    if (!c->padded) return backward_impl(c, params, dlogits, grads, p, s);
    // narrow network: the padded parameters expanded by the forward are still in the
    // workspace; each bucket's gradients are compacted into the caller's arena as soon as
    // they are final (backward_impl stage_done), then its event is recorded
    p.ugrad = grads;
    return backward_impl(c, p.pprm, dlogits, p.pgrad, p, s);
    ABI_CATCH(c)
}

int unet_adamw(unet_ctx* c, float* params, const float* grads, float* m, float* v, int64_t n,
               int step, double lr, double b1, double b2, double eps, double wd, double gscale,
               unet_stream_t stream) {
    ABI_TRY
    if (!c || !params || !grads || !m || !v || n < 0 || step < 1) return UNET_ERR_INVALID;
    // the plain update packs nothing: the images of an arena it writes into are stale
    if (c->pp_ok && ranges_overlap(params, n, c->pp_src, c->n_param_floats)) c->pp_ok = false;
    const AdamwScalars a = adamw_scalars(step, lr, b1, b2, eps, wd, gscale);
    return launched(c, "adamw", k_adamw(params, grads, m, v, n, a, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_adamw_repack(unet_ctx* c, float* params, const float* grads, float* m, float* v, int64_t n,
                      int step, double lr, double b1, double b2, double eps, double wd, double gscale,
                      unet_stream_t stream) {
    ABI_TRY
    if (!c || !params || !grads || !m || !v || n < 0 || step < 1) return UNET_ERR_INVALID;
    // a narrow (channel-padded) network packs from its padded arena: the plain update, and the
    // next forward repacks (unet_adamw drops the images of an arena it writes into)
    if (n != c->n_param_floats || c->padded) {
        return unet_adamw(c, params, grads, m, v, n, step, lr, b1, b2, eps, wd, gscale, stream);
    }
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, UNET_ERR_HIP, "hipSetDevice");
    const bool x3 = plan_has_pack3(c);
    if (!c->pp && hipMalloc((void**)&c->pp, sizeof(float) * (size_t)std::max<int64_t>(c->pack_floats, 32)) != hipSuccess) {
        c->pp = nullptr;
        return fail(c, UNET_ERR_HIP, "hipMalloc: weight images: %lld floats", (long long)c->pack_floats);
    }
    if (x3 && !c->pp3 &&
        hipMalloc((void**)&c->pp3, 3 * sizeof(uint16_t) * (size_t)std::max<int64_t>(c->pack_floats, 32)) != hipSuccess) {
        c->pp3 = nullptr;
        return fail(c, UNET_ERR_HIP, "hipMalloc: x3 weight images: %lld floats", (long long)c->pack_floats);
    }
    PackJobs jobs{};
    if (!build_pack_jobs(c, true, jobs)) return fail(c, UNET_ERR_INTERNAL, "pack job table full");
    // the arena ranges the pack jobs do not cover, in order
    std::vector<std::pair<int64_t, int64_t>> wr;  // [begin, end) of the packed weight tensors
    for (int k = 0; k < jobs.n; ++k) {
        const PackJob& J = jobs.j[k];
        wr.push_back({J.w, J.w + (int64_t)J.cin * J.cout * (J.kind == 0 ? 9 : 4)});
    }
    std::sort(wr.begin(), wr.end());
    AdamRanges rest{};
    int64_t at = 0, cum = 0;
    auto gap = [&](int64_t b, int64_t e) -> bool {
        if (e <= b) return true;
        if (rest.n >= MAX_ADAM_RANGES) return false;
        rest.off[rest.n] = b;
        rest.cum[rest.n] = cum;
        cum += e - b;
        ++rest.n;
        return true;
    };
    for (auto& r : wr) {
        if (!gap(at, r.first)) return fail(c, UNET_ERR_INTERNAL, "adamw range table full");
        at = std::max(at, r.second);
    }
    if (!gap(at, n)) return fail(c, UNET_ERR_INTERNAL, "adamw range table full");
    rest.cum[rest.n] = cum;
    const AdamwScalars a = adamw_scalars(step, lr, b1, b2, eps, wd, gscale);
    const hipStream_t s = (hipStream_t)stream;
    c->pp_ok = false;
    ++c->pp_gen;
    int r = k_pack_adamw(jobs, rest, params, grads, m, v, a, c->pp, c->bf16 ? 1 : 0, s);
    if (!r && x3) r = k_to_x3(c->pp, 32, 0, 32, nullptr, nullptr, 0, c->pack_floats / 32, c->pp3, 32, 0, s);
    if (int e = launched(c, "adamw repack", r)) return e;
    c->pp_src = params;
    c->pp_ok = true;
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_params_changed(unet_ctx* c) {
    if (!c) return UNET_ERR_INVALID;
    c->pp_ok = false;
    return UNET_OK;
}

int unet_arena_changed(unet_ctx* c, const float* params, int64_t n) {
    if (!c || !params || n < 0) return UNET_ERR_INVALID;
    if (c->pp_ok && ranges_overlap(params, n, c->pp_src, c->n_param_floats)) c->pp_ok = false;
    return UNET_OK;
}

int unet_set_option(unet_ctx* c, const char* name, int64_t value) {
    ABI_TRY
    if (!c || !name) return UNET_ERR_INVALID;
    for (const OptionDesc& d : OPTION_TABLE)
        if (strcmp(d.name, name) == 0) {
            // the weight images are those of the options they were written under (which of
            // them exist, x3 among them, depends on the options)
            if (c->opt.*d.field != (int)value) c->pp_ok = false;
            c->opt.*d.field = (int)value;
            return UNET_OK;
        }
    return fail(c, UNET_ERR_INVALID, "unknown option '%s'", name);
    ABI_CATCH(c)
}

int unet_get_option(const unet_ctx* c, const char* name, int64_t* value) {
    ABI_TRY
    if (!c || !name || !value) return UNET_ERR_INVALID;
    for (const OptionDesc& d : OPTION_TABLE)
        if (strcmp(d.name, name) == 0) {
            *value = c->opt.*d.field;
            return UNET_OK;
        }
    return UNET_ERR_INVALID;
    ABI_CATCH(c)
}

int unet_num_buckets(const unet_ctx* c, int* n) {
    ABI_TRY
    if (!c || !n) return UNET_ERR_INVALID;
    *n = (int)c->bucket_off.size();
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_bucket_range(const unet_ctx* c, int b, int64_t* off, int64_t* len) {
    ABI_TRY
    if (!c || b < 0 || b >= (int)c->bucket_off.size()) return UNET_ERR_INVALID;
    if (off) *off = c->bucket_off[b];
    if (len) *len = c->bucket_len[b];
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_stream_wait_bucket(unet_ctx* c, int b, unet_stream_t stream) {
    ABI_TRY
    if (!c || b < 0 || b >= (int)c->bucket_ev.size()) return UNET_ERR_INVALID;
    if (hipStreamWaitEvent((hipStream_t)stream, c->bucket_ev[b], 0) != hipSuccess)
        return fail(c, UNET_ERR_HIP, "hipStreamWaitEvent");
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_bucket_event(unet_ctx* c, int b, void** hip_event) {
    ABI_TRY
    if (!c || !hip_event || b < 0 || b >= (int)c->bucket_ev.size()) return UNET_ERR_INVALID;
    *hip_event = (void*)c->bucket_ev[b];
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_option_name(int i, const char** name) {
    if (!name || i < 0 || i >= (int)(sizeof OPTION_TABLE / sizeof OPTION_TABLE[0]))
        return UNET_ERR_INVALID;
    *name = OPTION_TABLE[i].name;
    return UNET_OK;
}

int unet_timing_enable(unet_ctx* c, int en) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    c->timing = en != 0;
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_timing_filter(unet_ctx* c, const char* substring) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    c->tfilter = substring ? substring : "";
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_timing_reset(unet_ctx* c) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    c->trec.clear();
    c->ev_used = 0;
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_timing_count(unet_ctx* c, int* n) {
    ABI_TRY
    if (!c || !n) return UNET_ERR_INVALID;
    *n = (int)c->trec.size();
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_timing_read(unet_ctx* c, int i, const char** family, int64_t* launches, double* total_ms,
                     double* flop) {
    ABI_TRY
    if (!c || i < 0 || i >= (int)c->trec.size()) return UNET_ERR_INVALID;
    TimeRec& t = c->trec[i];
    if (hipEventSynchronize(t.b) != hipSuccess) return fail(c, UNET_ERR_HIP, "event sync");
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, t.a, t.b);
    if (family) *family = t.label.c_str();
    if (launches) *launches = 1;
    if (total_ms) *total_ms = ms;
    if (flop) *flop = t.flop;
    return UNET_OK;
    ABI_CATCH(c)
}

int unet_debug_view(unet_ctx* c, int N, int H, int W, int training, int kind, int index,
                    int64_t* byte_offset, int64_t* count, int* ld, int* off) {
    ABI_TRY
    if (!c || !byte_offset || !count) return UNET_ERR_INVALID;
    if (!shape_ok(c, N, H, W)) return fail(c, UNET_ERR_SHAPE, "bad shape");
    Plan p;
    char* const base = (char*)(uintptr_t)4096;  // fake base: offsets only
    make_plan(c, N, H, W, training != 0, base, p);
    const void* q = nullptr;
    int64_t n = 0;
    int l = 1, o = 0;
    if (kind <= 4) {
        if (index < 0 || index >= c->nconv()) return UNET_ERR_INVALID;
        const ConvL& L = c->conv[index];
        const int C = L.cout;
        if (kind == 0) {
            q = p.y[index];
            l = p.ldy[index];
            o = p.offy[index];
            n = p.P[L.level] * l;
        } else {
            q = kind == 1 ? p.scale[index] : kind == 2 ? p.shift[index] : kind == 3 ? p.mean[index] : p.invstd[index];
            n = C;
        }
    } else if (kind == 9) {  // residual network: the stored output of block `index`
        if (!c->res || index < 0 || index > 2 * c->depth) return UNET_ERR_INVALID;
        q = p.out[index];
        l = p.ldout[index];
        o = p.offout[index];
        n = p.P[c->conv[2 * index].level] * l;
    } else {
        if (index < 0 || index >= c->depth) return UNET_ERR_INVALID;
        const int C = c->ch(index);
        if (kind == 5) {
            // the x3 path's max-pool writes the next conv's x3 image instead (forward_impl):
            // the f32 pooled buffer is never written there
            // (r06) ... and a bf16 training pass pools into the next conv's bf16 image
            const Route& rj = p.rt.conv[2 * (index + 1)];
            if (rj.up == W_POOL)
                return fail(c, UNET_ERR_INVALID, "debug view 5: level %d pools into %s image", index,
                            rj.fwd == FAM_X3 ? "an x3" : "a bf16");
            q = p.pool[index];
            n = p.P[index + 1] * C;
            l = C;
        } else if (kind == 6) {
            q = p.cat[index];
            n = p.P[index] * 2 * C;
            l = 2 * C;
        } else if (kind == 7) {
            if (!training) return UNET_ERR_INVALID;
            q = p.dcat[index];
            n = p.P[index] * 2 * C;
            l = 2 * C;
        } else if (kind == 8) {  // max-pool winner index (uint8, window position 0..3)
            q = p.idx[index];
            n = p.P[index + 1] * C;
            l = C;
        } else {
            return UNET_ERR_INVALID;
        }
    }
    *byte_offset = (int64_t)((const char*)q - base);
    *count = n;
    if (ld) *ld = l;
    if (off) *off = o;
    return UNET_OK;
    ABI_CATCH(c)
}

}  // extern "C"
