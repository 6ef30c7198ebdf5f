// The stand-alone entry points of include/unet_hip.h: losses, distance transform, surface and
// lesion metrics, the Lovasz hinge loss, connected components, lesion morphometry, lesion echogenicity, test-time augmentation, the threshold sweep, the predict-mode
// export (resize back + overlay), resize and the training augmentations, each with its host twin where
// it has one.  None of them reads the layer graph
// or a workspace plan (runtime.hip): they use the context's device, error string, launch timer
// and their feature's scratch buffer (runtime_internal.h).
#include <algorithm>

#include "runtime_internal.h"
#include "aug.h"
#include "cc.h"
#include "curve.h"
#include "echo.h"
#include "edt.h"
#include "export.h"
#include "morph.h"
#include "tta.h"
#include "x3_split.h"

namespace {

// Pillow's precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) for the
// BILINEAR filter (support 1) over the full source extent [0, in_size): same double
// arithmetic in the same order, then the 22-bit fixed-point conversion.
int pil_resample_plan(int in_size, int out_size, int32_t* kk, int32_t* bounds) {
    const double in0 = 0.0, in1 = (double)(float)in_size;
    double filterscale, scale;
    filterscale = scale = (double)(in1 - in0) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    if (!kk || !bounds) return ksize;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        double ww = 0.0;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        int x = 0;
        for (; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; ++x) k[x] = 0;
        for (x = 0; x < ksize; ++x)
            kk[(int64_t)xx * ksize + x] = k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << (32 - 8 - 2)))
                                                   : (int32_t)(0.5 + k[x] * (1 << (32 - 8 - 2)));
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

}  // namespace

extern "C" {

int unet_loss_stats(unet_ctx* c, const float* logits, const float* targets, int N, int C, int H,
                    int W, float* stats, double* sums, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !stats || !sums) return UNET_ERR_INVALID;
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail(c, UNET_ERR_SHAPE, "bad loss shape");
    const int64_t per = (int64_t)C * H * W;
    if (int r = grow(c, c->loss, sizeof(float) * 4 * (size_t)N * loss_groups(per), "loss")) return r;
    return launched(c, "loss_stats",
                    k_loss_stats(logits, targets, N, per, stats, sums, (float*)c->loss.p, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_loss_finalize(unet_ctx* c, const double* sums, float* losses, float fa, float fb,
                       float fg, unet_stream_t stream) {
    ABI_TRY
    if (!c || !sums || !losses) return UNET_ERR_INVALID;
    return launched(c, "loss_finalize", k_loss_finalize(sums, fa, fb, fg, losses, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_loss_fwd(unet_ctx* c, const float* logits, const float* targets, int N, int C, int H,
                  int W, float* stats, double* sums, float* losses, float fa, float fb, float fg,
                  unet_stream_t stream) {
    const int r = unet_loss_stats(c, logits, targets, N, C, H, W, stats, sums, stream);
    return r ? r : unet_loss_finalize(c, sums, losses, fa, fb, fg, stream);
}

int unet_loss_bwd(unet_ctx* c, const float* logits, const float* targets, int N, int C, int H,
                  int W, const float* stats, const double* sums, const float* w, float* dlogits,
                  float fa, float fb, float fg, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !stats || !sums || !w || !dlogits) return UNET_ERR_INVALID;
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail(c, UNET_ERR_SHAPE, "bad loss shape");
    return launched(c, "loss_bwd",
                    k_loss_bwd(logits, targets, N, (int64_t)C * H * W, stats, sums, w, fa, fb, fg, dlogits,
                               (hipStream_t)stream));
    ABI_CATCH(c)
}

static bool edt_shape_ok(int N, int C, int H, int W) {
    return N >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= EDT_MAX_SIDE && W <= EDT_MAX_SIDE &&
           (int64_t)N * std::max(H, W) < (int64_t)1 << 31;
}

int unet_edt(unet_ctx* c, const float* targets, int N, int C, int H, int W, float* dist,
             unet_stream_t stream) {
    ABI_TRY
    if (!c || !targets || !dist) return UNET_ERR_INVALID;
    if (!edt_shape_ok(N, C, H, W))
        return fail(c, UNET_ERR_SHAPE, "edt: N, C, H, W >= 1 and max(H, W) <= %d", EDT_MAX_SIDE);
    if (int r = grow(c, c->boundary, sizeof(int) * (size_t)edt_scratch_ints(N, H, W), "boundary")) return r;
    return launched(c, "edt", k_edt(targets, N, C, H, W, (int*)c->boundary.p, dist, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_edt_host(const float* targets, int N, int C, int H, int W, float* dist) {
    if (!targets || !dist) return UNET_ERR_INVALID;
    if (!edt_shape_ok(N, C, H, W)) return UNET_ERR_SHAPE;
    return catch_to_status([&] {
        std::vector<int> g2((size_t)N * H * W);
        edt_host(targets, N, C, H, W, g2.data(), dist);
    });
}

int unet_boundary_fwd(unet_ctx* c, const float* logits, const float* targets, const float* dist,
                      int N, int C, int H, int W, double* sum, float* loss, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !dist || !sum || !loss) return UNET_ERR_INVALID;
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail(c, UNET_ERR_SHAPE, "bad loss shape");
    const int64_t hw = (int64_t)H * W;
    if (int r = grow(c, c->boundary, sizeof(float) * (size_t)N * loss_groups(hw), "boundary")) return r;
    return launched(c, "boundary_fwd",
                    k_boundary_fwd(logits, targets, dist, N, C, hw, (float*)c->boundary.p, sum, loss,
                                   (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_boundary_bwd(unet_ctx* c, const float* logits, const float* targets, const float* dist,
                      int N, int C, int H, int W, const float* w, float* dlogits,
                      unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !dist || !w || !dlogits) return UNET_ERR_INVALID;
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail(c, UNET_ERR_SHAPE, "bad loss shape");
    return launched(c, "boundary_bwd",
                    k_boundary_bwd(logits, targets, dist, N, C, (int64_t)H * W, w, dlogits, (hipStream_t)stream));
    ABI_CATCH(c)
}

// ---- Lovasz hinge loss (kernels_lovasz.hip, lovasz.h) ----
int unet_lovasz_fwd(unet_ctx* c, const float* logits, const float* targets, int N, int C, int H, int W,
                    float* gmap, uint32_t* perm, double* sum, float* loss, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !gmap || !sum || !loss) return UNET_ERR_INVALID;
    if (!lovasz_shape_ok(N, C, H, W))
        return fail(c, UNET_ERR_SHAPE, "lovasz: N, C, H, W >= 1 and H * W <= 2^24");
    if (int r = grow(c, c->lovasz, lovasz_scratch_bytes(N, C, H, W), "lovasz")) return r;
    return launched(c, "lovasz_fwd",
                    k_lovasz_fwd(logits, targets, N, C, H, W, c->lovasz.p, gmap, perm, sum, loss,
                                 (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_lovasz_bwd(unet_ctx* c, const float* logits, const float* targets, const float* gmap, int N, int C,
                    int H, int W, const float* w, float* dlogits, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !gmap || !w || !dlogits) return UNET_ERR_INVALID;
    if (!lovasz_shape_ok(N, C, H, W))
        return fail(c, UNET_ERR_SHAPE, "lovasz: N, C, H, W >= 1 and H * W <= 2^24");
    return launched(c, "lovasz_bwd",
                    k_lovasz_bwd(logits, targets, gmap, N, C, H, W, w, dlogits, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_lovasz_host(const float* logits, const float* targets, int N, int C, int H, int W, float* gmap,
                     uint32_t* perm, double* sum, float* loss) {
    if (!logits || !targets || !gmap || !sum || !loss) return UNET_ERR_INVALID;
    if (!lovasz_shape_ok(N, C, H, W)) return UNET_ERR_SHAPE;
    return catch_to_status([&] { lovasz_host(logits, targets, N, C, H, W, gmap, perm, sum, loss); });
}

static bool surf_shape_ok(int N, int C, int H, int W) {
    return N >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= EDT_MAX_SIDE && W <= EDT_MAX_SIDE &&
           2 * (int64_t)N * std::max(H, W) < (int64_t)1 << 31 &&
           (int64_t)N * H * W < (int64_t)1 << 36;
}

int unet_surface_stats(unet_ctx* c, const float* logits, const float* targets, int N, int C, int H,
                       int W, int64_t* out_i64, double* out_f64, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !out_i64 || !out_f64) return UNET_ERR_INVALID;
    if (!surf_shape_ok(N, C, H, W))
        return fail(c, UNET_ERR_SHAPE, "surface_stats: N, C, H, W >= 1 and max(H, W) <= %d",
                    EDT_MAX_SIDE);
    if (int r = grow(c, c->surface, surf_scratch_bytes(N, H, W), "surface")) return r;
    return launched(c, "surface_stats",
                    k_surface_stats(logits, targets, N, C, H, W, c->surface.p, out_i64, out_f64,
                                    (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_surface_stats_host(const float* logits, const float* targets, int N, int C, int H, int W,
                            int64_t* out_i64, double* out_f64) {
    if (!logits || !targets || !out_i64 || !out_f64) return UNET_ERR_INVALID;
    if (!surf_shape_ok(N, C, H, W)) return UNET_ERR_SHAPE;
    return catch_to_status([&] {
        std::vector<uint8_t> border(2 * (size_t)H * W);
        std::vector<int> d2(2 * (size_t)H * W);
        surface_stats_host(logits, targets, N, C, H, W, border.data(), d2.data(), out_i64, out_f64);
    });
}

// ---- connected components, post-processing, lesion counts (kernels_cc.hip, cc.h) ----
static const char* cc_args_error(int kind, int N, int C, int H, int W, int conn) {
    if (conn != 1 && conn != 2) return "connectivity must be 1 or 2";
    if (kind < 0 || kind > 2) return "kind must be 0 (uint8 mask), 1 (logits) or 2 (targets)";
    if (N < 1 || C < 1 || H < 1 || W < 1) return "N, C, H, W >= 1";
    if ((int64_t)H * W >= (int64_t)1 << 31) return "H * W must be below 2^31";
    return nullptr;
}

// tile, seam and flatten of `planes` planes read from src (see k_cc_tile) into sc.L at plane q0
static int cc_label(unet_ctx* c, Launcher& ln, const char* what, const void* src, int kind,
                    int64_t sample_stride, int q0, int planes, int H, int W, int conn,
                    const CcScratch& sc, bool areas, bool rows, bool counts) {
    const int64_t hw = (int64_t)H * W;
    const int tile = c->opt.cc_tile;
    int* L = sc.L + q0 * hw;
    int* area = sc.area + q0 * hw;
    hipStream_t s = ln.s;
    const std::string w = what;
    if (int r = ln.run("cc/tile|" + w, 0, [&] { return k_cc_tile(src, kind, sample_stride, planes, H, W, conn, tile, L, area, s); }))
        return r;
    if (int r = ln.run("cc/seam|" + w, 0, [&] { return k_cc_seam(L, planes, H, W, conn, tile, s); })) return r;
    return ln.run("cc/flatten|" + w, 0, [&] {
        return k_cc_flatten(L, areas ? area : nullptr, rows ? sc.rowcnt + (int64_t)q0 * H : nullptr,
                            counts ? sc.cnt + q0 : nullptr, planes, H, W, s);
    });
}

static int cc_prepare(unet_ctx* c, const char* what, int N, int planes, int H, int W, hipStream_t s,
                      CcScratch& sc) {
    if (!cc_grid_ok(planes, H, W)) return fail(c, UNET_ERR_SHAPE, "%s: batch too large for one launch", what);
    const size_t need = cc_scratch(nullptr, N, planes, H, W).bytes;
    if (int r = grow(c, c->cc, need, "components")) return r;
    sc = cc_scratch(c->cc.p, N, planes, H, W);
    if (hipMemsetAsync(c->cc.p, 0, sc.zero_bytes, s) != hipSuccess) return fail(c, UNET_ERR_HIP, "%s: memset", what);
    return UNET_OK;
}

int unet_components(unet_ctx* c, const void* src, int kind, int N, int C, int H, int W,
                    int connectivity, int32_t* labels, int32_t* count, unet_stream_t stream) {
    ABI_TRY
    if (!c || !src || !labels || !count) return UNET_ERR_INVALID;
    if (const char* e = cc_args_error(kind, N, C, H, W, connectivity))
        return fail(c, UNET_ERR_INVALID, "components: %s", e);
    hipStream_t s = (hipStream_t)stream;
    CcScratch sc;
    if (int r = cc_prepare(c, "components", N, N, H, W, s, sc)) return r;
    Launcher ln{c, s};
    const int64_t hw = (int64_t)H * W;
    if (int r = cc_label(c, ln, "components", src, kind, C * hw, 0, N, H, W, connectivity, sc, false, true, false))
        return r;
    return ln.run("cc/rank|components", 0,
                  [&] { return k_cc_rank(sc.L, sc.area, sc.rowcnt, count, N, H, W, labels, s); });
    ABI_CATCH(c)
}

int unet_postprocess(unet_ctx* c, const void* src, int kind, int N, int C, int H, int W,
                     int connectivity, int keep_largest, int64_t min_area, int fill_holes,
                     uint8_t* out, int64_t* info, unet_stream_t stream) {
    ABI_TRY
    if (!c || !src || !out || !info) return UNET_ERR_INVALID;
    if (const char* e = cc_args_error(kind, N, C, H, W, connectivity))
        return fail(c, UNET_ERR_INVALID, "postprocess: %s", e);
    if ((const void*)out == src) return fail(c, UNET_ERR_INVALID, "postprocess: out must differ from src");
    hipStream_t s = (hipStream_t)stream;
    CcScratch sc;
    if (int r = cc_prepare(c, "postprocess", N, N, H, W, s, sc)) return r;
    if (hipMemsetAsync(info, 0, 4 * sizeof(int64_t) * (size_t)N, s) != hipSuccess)
        return fail(c, UNET_ERR_HIP, "postprocess: memset");
    Launcher ln{c, s};
    const int64_t hw = (int64_t)H * W;
    if (int r = cc_label(c, ln, "postprocess", src, kind, C * hw, 0, N, H, W, connectivity, sc, true, false, true))
        return r;
    if (int r = ln.run("cc/select|postprocess", 0,
                       [&] { return k_cc_select(sc.L, sc.area, min_area, sc.kept, sc.best, N, H, W, s); }))
        return r;
    if (int r = ln.run("cc/write|postprocess", 0, [&] {
            return k_cc_write(sc.L, sc.area, min_area, keep_largest, sc.cnt, sc.kept, sc.best, out, info, N, H, W, s);
        }))
        return r;
    if (!fill_holes) return UNET_OK;
    // the complement of `out` at connectivity 1; the tile pass leaves the flags (sc.area) zero
    if (int r = cc_label(c, ln, "fill", out, CC_KIND_U8_ZERO, hw, 0, N, H, W, 1, sc, false, false, false))
        return r;
    return ln.run("cc/fill|fill", 0, [&] { return k_cc_fill(sc.L, sc.area, out, info, N, H, W, s); });
    ABI_CATCH(c)
}

int unet_lesion_stats(unet_ctx* c, const void* pred, int kind, const float* targets, int N, int C,
                      int H, int W, int connectivity, int64_t* out, unet_stream_t stream) {
    ABI_TRY
    if (!c || !pred || !targets || !out) return UNET_ERR_INVALID;
    if (const char* e = cc_args_error(kind, N, C, H, W, connectivity))
        return fail(c, UNET_ERR_INVALID, "lesion_stats: %s", e);
    if (N > (1 << 29)) return fail(c, UNET_ERR_SHAPE, "lesion_stats: batch too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    CcScratch sc;
    if (int r = cc_prepare(c, "lesion_stats", N, 2 * N, H, W, s, sc)) return r;
    if (hipMemsetAsync(out, 0, 4 * sizeof(int64_t) * (size_t)N, s) != hipSuccess)
        return fail(c, UNET_ERR_HIP, "lesion_stats: memset");
    Launcher ln{c, s};
    const int64_t hw = (int64_t)H * W;
    if (int r = cc_label(c, ln, "pred", pred, kind, C * hw, 0, N, H, W, connectivity, sc, false, false, false))
        return r;
    if (int r = cc_label(c, ln, "targets", targets, CC_KIND_TARGETS, C * hw, N, N, H, W, connectivity, sc,
                         false, false, false))
        return r;
    return ln.run("cc/hits|lesion", 0, [&] { return k_cc_hits(sc.L, sc.area, out, N, H, W, s); });
    ABI_CATCH(c)
}

int unet_components_host(const void* src, int kind, int N, int C, int H, int W, int connectivity,
                         int32_t* labels, int32_t* count) {
    if (!src || !labels || !count || cc_args_error(kind, N, C, H, W, connectivity)) return UNET_ERR_INVALID;
    return catch_to_status([&] { components_host(src, kind, N, C, H, W, connectivity, labels, count); });
}

int unet_postprocess_host(const void* src, int kind, int N, int C, int H, int W, int connectivity,
                          int keep_largest, int64_t min_area, int fill_holes, uint8_t* out,
                          int64_t* info) {
    if (!src || !out || !info || (const void*)out == src || cc_args_error(kind, N, C, H, W, connectivity))
        return UNET_ERR_INVALID;
    return catch_to_status([&] {
        postprocess_host(src, kind, N, C, H, W, connectivity, keep_largest, min_area, fill_holes, out, info);
    });
}

int unet_lesion_stats_host(const void* pred, int kind, const float* targets, int N, int C, int H, int W,
                           int connectivity, int64_t* out) {
    if (!pred || !targets || !out || cc_args_error(kind, N, C, H, W, connectivity)) return UNET_ERR_INVALID;
    return catch_to_status([&] { lesion_stats_host(pred, kind, targets, N, C, H, W, connectivity, out); });
}

// ---- lesion morphometry (kernels_morph.hip, morph.h) ----
int unet_morphometry(unet_ctx* c, const int32_t* labels, const int32_t* count, int N, int H, int W,
                     int64_t max_rows, int64_t* table, unet_stream_t stream) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    if (const char* e = morph_args_invalid(labels, count, table, N, H, W, max_rows))
        return fail(c, UNET_ERR_INVALID, "morphometry: %s", e);
    if (!morph_shape_ok(H, W)) return fail(c, UNET_ERR_SHAPE, "morphometry: H, W <= %d", MORPH_MAX_SIDE);
    if (!morph_grid_ok(N, H, W, max_rows))
        return fail(c, UNET_ERR_SHAPE, "morphometry: batch too large for one launch");
    if (int r = grow(c, c->morph, morph_scratch(nullptr, N, H, W, max_rows).bytes, "morphometry")) return r;
    const MorphScratch sc = morph_scratch(c->morph.p, N, H, W, max_rows);
    Launcher ln{c, (hipStream_t)stream};
    const int lds = c->opt.morph_lds;
    if (int r = ln.run("morph/reduce", 0, [&] { return k_morph_reduce(labels, N, H, W, max_rows, lds, table, ln.s); }))
        return r;
    if (int r = ln.run("morph/extent", 0,
                       [&] { return k_morph_extent(labels, count, N, H, W, max_rows, table, sc, ln.s); }))
        return r;
    return ln.run("morph/feret", 0, [&] { return k_morph_feret(count, N, H, W, max_rows, sc, table, ln.s); });
    ABI_CATCH(c)
}

int unet_morphometry_host(const int32_t* labels, const int32_t* count, int N, int H, int W, int64_t max_rows,
                          int64_t* table) {
    if (morph_args_invalid(labels, count, table, N, H, W, max_rows)) return UNET_ERR_INVALID;
    if (!morph_shape_ok(H, W)) return UNET_ERR_SHAPE;
    return catch_to_status([&] { morphometry_host(labels, count, N, H, W, max_rows, table); });
}

// ---- lesion echogenicity and texture (kernels_echo.hip, echo.h) ----
int unet_lesion_echo(unet_ctx* c, const uint8_t* gray, const int32_t* labels, const int32_t* count, int N, int H,
                     int W, int64_t max_rows, int levels, int ring, int32_t* table, unet_stream_t stream) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    if (const char* e = echo_args_invalid(gray, labels, count, table, N, H, W, max_rows, levels, ring))
        return fail(c, UNET_ERR_INVALID, "lesion_echo: %s", e);
    if (!echo_shape_ok(H, W)) return fail(c, UNET_ERR_SHAPE, "lesion_echo: H, W <= %d", MORPH_MAX_SIDE);
    if (!echo_grid_ok(N, H, W, max_rows))
        return fail(c, UNET_ERR_SHAPE, "lesion_echo: batch too large for one launch");
    Launcher ln{c, (hipStream_t)stream};
    const int agg = c->opt.echo_agg;
    if (int r = ln.run("echo/clear", 0, [&] { return k_echo_clear(N, max_rows, levels, table, ln.s); })) return r;
    return ln.run("echo/count", 0, [&] {
        return k_echo_count(gray, labels, count, N, H, W, max_rows, levels, ring, agg, table, ln.s);
    });
    ABI_CATCH(c)
}

int unet_lesion_echo_host(const uint8_t* gray, const int32_t* labels, const int32_t* count, int N, int H, int W,
                          int64_t max_rows, int levels, int ring, int32_t* table) {
    if (echo_args_invalid(gray, labels, count, table, N, H, W, max_rows, levels, ring)) return UNET_ERR_INVALID;
    if (!echo_shape_ok(H, W)) return UNET_ERR_SHAPE;
    return catch_to_status([&] { echo_host(gray, labels, count, N, H, W, max_rows, levels, ring, table); });
}

// ---- test-time augmentation (kernels_tta.hip, tta.h) ----
// UNET_OK, or the error code with *msg set
static int tta_args_error(int N, int C, int H, int W, uint32_t views, const char** msg) {
    *msg = nullptr;
    if (views == 0 || (views & ~TTA_ALL_VIEWS)) *msg = "views must be a non-empty mask of the bits 0..7";
    else if (N < 1 || C < 1 || H < 1 || W < 1) *msg = "N, C, H, W >= 1";
    else if ((int64_t)H * W >= (int64_t)1 << 31) *msg = "H * W must be below 2^31";
    if (*msg) return UNET_ERR_INVALID;
    if ((views & 0xF0u) && H != W) *msg = "a transposed view (k >= 4) needs H == W";
    else if ((int64_t)tta_view_list(views).K * N * C >= (int64_t)1 << 31) *msg = "K * N * C must be below 2^31";
    return *msg ? UNET_ERR_SHAPE : UNET_OK;
}

static bool tta_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}
// does an output of the merge overlap its input?
static bool tta_merge_aliases(const float* logits, int N, int C, int H, int W, uint32_t views, const float* score,
                              const uint8_t* mask, const uint8_t* votes) {
    const size_t n = (size_t)N * C * H * W, in = sizeof(float) * n * tta_view_list(views).K;
    return tta_overlap(logits, in, score, sizeof(float) * n) || tta_overlap(logits, in, mask, n) ||
           tta_overlap(logits, in, votes, n);
}

int unet_tta_views(unet_ctx* c, const float* x, int N, int C, int H, int W, uint32_t views, float* out,
                   unet_stream_t stream) {
    ABI_TRY
    if (!c || !x || !out) return UNET_ERR_INVALID;
    const char* e;
    if (int r = tta_args_error(N, C, H, W, views, &e)) return fail(c, r, "tta_views: %s", e);
    Launcher ln{c, (hipStream_t)stream};
    return ln.run("tta/views", 0, [&] { return k_tta_views(x, N, C, H, W, views, out, ln.s); });
    ABI_CATCH(c)
}

int unet_tta_merge(unet_ctx* c, const float* logits, int N, int C, int H, int W, uint32_t views, int mode,
                   float* score, uint8_t* mask, uint8_t* votes, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !score) return UNET_ERR_INVALID;
    const char* e;
    if (int r = tta_args_error(N, C, H, W, views, &e)) return fail(c, r, "tta_merge: %s", e);
    if (mode != TTA_MODE_LOGIT && mode != TTA_MODE_PROB)
        return fail(c, UNET_ERR_INVALID, "tta_merge: mode must be 0 (logit) or 1 (prob)");
    if (tta_merge_aliases(logits, N, C, H, W, views, score, mask, votes))
        return fail(c, UNET_ERR_INVALID, "tta_merge: an output overlaps logits");
    Launcher ln{c, (hipStream_t)stream};
    return ln.run("tta/merge", 0,
                  [&] { return k_tta_merge(logits, N, C, H, W, views, mode, score, mask, votes, ln.s); });
    ABI_CATCH(c)
}

int unet_tta_views_host(const float* x, int N, int C, int H, int W, uint32_t views, float* out) {
    if (!x || !out) return UNET_ERR_INVALID;
    const char* e;
    if (int r = tta_args_error(N, C, H, W, views, &e)) return r;
    return catch_to_status([&] { tta_views_host(x, N, C, H, W, views, out); });
}

int unet_tta_merge_host(const float* logits, int N, int C, int H, int W, uint32_t views, int mode, float* score,
                        uint8_t* mask, uint8_t* votes) {
    if (!logits || !score) return UNET_ERR_INVALID;
    const char* e;
    if (int r = tta_args_error(N, C, H, W, views, &e)) return r;
    if ((mode != TTA_MODE_LOGIT && mode != TTA_MODE_PROB) ||
        tta_merge_aliases(logits, N, C, H, W, views, score, mask, votes))
        return UNET_ERR_INVALID;
    return catch_to_status([&] { tta_merge_host(logits, N, C, H, W, views, mode, score, mask, votes); });
}

// ---- threshold sweep (kernels_curve.hip, curve.h) ----
// UNET_OK, or the error code with *msg set
static int curve_args_error(int planes, int64_t hw, int B, const char** msg) {
    *msg = nullptr;
    if (!curve_bins_ok(B)) *msg = "B must be a power of two in 2..1024";
    else if (planes < 1) *msg = "planes >= 1";
    else if (hw >= 0 && hw < 1) *msg = "hw >= 1";
    if (*msg) return UNET_ERR_INVALID;
    if (hw < 0) return UNET_OK;  // the statistics have no hw
    if (hw >= (int64_t)1 << 31) *msg = "hw must be below 2^31";
    return *msg ? UNET_ERR_SHAPE : UNET_OK;
}

int unet_curve_edges(int B, float* edges) {
    if (!edges || !curve_bins_ok(B)) return UNET_ERR_INVALID;
    curve_edges(B, edges);
    return UNET_OK;
}

int unet_curve_hist(unet_ctx* c, const float* logits, const float* targets, int planes, int64_t hw,
                    const float* edges, int B, int32_t* plane_hist, int64_t* total, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !edges || !plane_hist || !total) return UNET_ERR_INVALID;
    const char* e;
    if (int r = curve_args_error(planes, hw < 1 ? 0 : hw, B, &e)) return fail(c, r, "curve_hist: %s", e);
    Launcher ln{c, (hipStream_t)stream};
    return ln.run("curve/hist", 0,
                  [&] { return k_curve_hist(logits, targets, planes, hw, edges, B, plane_hist, total, ln.s); });
    ABI_CATCH(c)
}

int unet_curve_hist_host(const float* logits, const float* targets, int planes, int64_t hw, const float* edges,
                         int B, int32_t* plane_hist, int64_t* total) {
    if (!logits || !targets || !edges || !plane_hist || !total) return UNET_ERR_INVALID;
    const char* e;
    if (int r = curve_args_error(planes, hw < 1 ? 0 : hw, B, &e)) return r;
    curve_hist_host(logits, targets, planes, hw, edges, B, plane_hist, total);
    return UNET_OK;
}

int unet_curve_stats(unet_ctx* c, const int32_t* plane_hist, int planes, int B, int64_t* out_i64,
                     double* dice_sum, unet_stream_t stream) {
    ABI_TRY
    if (!c || !plane_hist || !out_i64 || !dice_sum) return UNET_ERR_INVALID;
    const char* e;
    if (int r = curve_args_error(planes, -1, B, &e)) return fail(c, r, "curve_stats: %s", e);
    if (int r = grow(c, c->curve, curve_scratch_bytes(planes, B), "curve")) return r;
    Launcher ln{c, (hipStream_t)stream};
    return ln.run("curve/stats", 0,
                  [&] { return k_curve_stats(plane_hist, planes, B, c->curve.p, out_i64, dice_sum, ln.s); });
    ABI_CATCH(c)
}

int unet_curve_stats_host(const int32_t* plane_hist, int planes, int B, int64_t* out_i64, double* dice_sum) {
    if (!plane_hist || !out_i64 || !dice_sum) return UNET_ERR_INVALID;
    const char* e;
    if (int r = curve_args_error(planes, -1, B, &e)) return r;
    return catch_to_status([&] {
        std::vector<int32_t> cnt(2 * (size_t)(B + 1));
        std::vector<double> dice((size_t)B + 1);
        curve_stats_host(plane_hist, planes, B, out_i64, dice_sum, cnt.data(), cnt.data() + B + 1, dice.data());
    });
}

// ---- predict-mode export (kernels_export.hip, export.h) ----
// null, or what is wrong with the arguments of the resize
static const char* export_resize_error(const float* src, int h, int w, int oh, int ow, const double* kh,
                                       const int32_t* bh, int ksh, const double* kv, const int32_t* bv, int ksv,
                                       int kind, const uint8_t* mask) {
    if (!src || !mask) return "src and mask must not be null";
    if (h < 1 || w < 1 || oh < 1 || ow < 1) return "h, w, oh, ow >= 1";
    if (!export_kind_ok(kind)) return "kind must be 0 (sigmoid > 0.5) or 1 (greater than thr)";
    if ((int64_t)h * ow >= (int64_t)1 << 31 || (int64_t)oh * ow >= (int64_t)1 << 31) return "plane too large";
    if ((ow != w && (!kh || !bh || ksh < 1)) || (oh != h && (!kv || !bv || ksv < 1)))
        return "missing coefficient tables";
    return nullptr;
}

static const char* export_overlay_error(const uint8_t* gray, const uint8_t* pred, int h, int w, int r, int alpha,
                                        const uint8_t* rgb, const int64_t* stats) {
    if (!gray || !pred || !rgb || !stats) return "gray, pred, rgb and stats must not be null";
    if (h < 1 || w < 1) return "h, w >= 1";
    if ((int64_t)h * w >= (int64_t)1 << 29) return "plane too large";
    if (!export_width_ok(r)) return "contour width r must be 1, 2 or 3";
    if (!export_alpha_ok(alpha)) return "alpha must be in 0..256";
    return nullptr;
}

int unet_resize_f32_plan(int in_size, int out_size, double* coeffs, int32_t* bounds, int* ksize) {
    ABI_TRY
    if (in_size < 1 || out_size < 1 || !ksize) return UNET_ERR_INVALID;
    *ksize = export_resize_plan(in_size, out_size, coeffs, bounds);
    return UNET_OK;
    ABI_CATCH((unet_ctx*)nullptr)
}

int unet_resize_f32_mask(unet_ctx* c, const float* src, int h, int w, int oh, int ow, const double* kh,
                         const int32_t* bh, int ksh, const double* kv, const int32_t* bv, int ksv, int kind,
                         float thr, float* plane, uint8_t* mask, unet_stream_t stream) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    if (const char* e = export_resize_error(src, h, w, oh, ow, kh, bh, ksh, kv, bv, ksv, kind, mask))
        return fail(c, UNET_ERR_INVALID, "resize_f32_mask: %s", e);
    if (int r = grow(c, c->exportbuf, export_scratch_bytes(h, w, ow), "export")) return r;
    Launcher ln{c, (hipStream_t)stream};
    return ln.run("export/resize", 0, [&] {
        return k_resize_f32_mask(src, h, w, oh, ow, kh, bh, ksh, kv, bv, ksv, kind, thr, c->exportbuf.p, plane, mask,
                                 ln.s);
    });
    ABI_CATCH(c)
}

int unet_resize_f32_mask_host(const float* src, int h, int w, int oh, int ow, const double* kh, const int32_t* bh,
                              int ksh, const double* kv, const int32_t* bv, int ksv, int kind, float thr,
                              float* plane, uint8_t* mask) {
    if (export_resize_error(src, h, w, oh, ow, kh, bh, ksh, kv, bv, ksv, kind, mask)) return UNET_ERR_INVALID;
    return catch_to_status([&] {
        std::vector<float> tmp(ow != w ? (size_t)h * ow : 0);
        export_resize_mask_host(src, h, w, oh, ow, kh, bh, ksh, kv, bv, ksv, kind, thr, tmp.data(), plane, mask);
    });
}

int unet_overlay_u8(unet_ctx* c, const uint8_t* gray, const uint8_t* pred, const uint8_t* gt, int h, int w, int r,
                    int alpha, uint8_t* rgb, int64_t* stats, unet_stream_t stream) {
    ABI_TRY
    if (!c) return UNET_ERR_INVALID;
    if (const char* e = export_overlay_error(gray, pred, h, w, r, alpha, rgb, stats))
        return fail(c, UNET_ERR_INVALID, "overlay: %s", e);
    Launcher ln{c, (hipStream_t)stream};
    return ln.run("export/overlay", 0, [&] { return k_overlay_u8(gray, pred, gt, h, w, r, alpha, rgb, stats, ln.s); });
    ABI_CATCH(c)
}

int unet_overlay_u8_host(const uint8_t* gray, const uint8_t* pred, const uint8_t* gt, int h, int w, int r, int alpha,
                         uint8_t* rgb, int64_t* stats) {
    if (export_overlay_error(gray, pred, h, w, r, alpha, rgb, stats)) return UNET_ERR_INVALID;
    export_overlay_host(gray, pred, gt, h, w, r, alpha, rgb, stats);
    return UNET_OK;
}

int unet_x3_split_host(const float* v, int64_t n, uint16_t* out) {
    if (!v || !out || n < 0 || n % 32) return UNET_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = i / 32, j = i % 32;
        x3_split(v[i], X3CvtHost{}, out[96 * r + j], out[96 * r + 32 + j], out[96 * r + 64 + j]);
    }
    return UNET_OK;
}

int unet_x3_split_device(unet_ctx* c, const float* v, int64_t n, uint16_t* out, unet_stream_t stream) {
    ABI_TRY
    if (!c || !v || !out || n < 32 || n % 32) return c ? fail(c, UNET_ERR_INVALID, "x3 split: n") : UNET_ERR_INVALID;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, UNET_ERR_HIP, "hipSetDevice");
    return launched(c, "to_x3", k_to_x3(v, 32, 0, 32, nullptr, nullptr, 0, n / 32, out, 32, 0, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_mask_counts(unet_ctx* c, const float* logits, const float* targets, int64_t n,
                     uint8_t* mask, int64_t* counts, unet_stream_t stream) {
    ABI_TRY
    if (!c || !logits || !targets || !counts || n < 0) return UNET_ERR_INVALID;
    return launched(c, "mask_counts", k_mask_counts(logits, targets, n, mask, counts, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_resize_plan(int in_size, int out_size, int32_t* coeffs, int32_t* bounds, int* ksize) {
    ABI_TRY
    if (in_size < 1 || out_size < 1 || !ksize) return UNET_ERR_INVALID;
    *ksize = pil_resample_plan(in_size, out_size, coeffs, bounds);
    return UNET_OK;
    ABI_CATCH((unet_ctx*)nullptr)
}

int unet_resize_u8(unet_ctx* c, const uint8_t* src, int h, int w, float* dst, int oh, int ow,
                   const int32_t* kh, const int32_t* bh, int ksh, const int32_t* kv,
                   const int32_t* bv, int ksv, float divisor, unet_stream_t stream) {
    ABI_TRY
    if (!c || !src || !dst || h < 1 || w < 1 || oh < 1 || ow < 1 || !(divisor > 0.f))
        return UNET_ERR_INVALID;
    const int need_h = ow != w, need_v = oh != h;
    if ((need_h && (!kh || !bh || ksh < 1)) || (need_v && (!kv || !bv || ksv < 1)))
        return fail(c, UNET_ERR_INVALID, "resize: missing coefficient tables");
    return launched(c, "resize",
                    k_resize_u8(src, h, w, dst, oh, ow, kh, bh, ksh, kv, bv, ksv, need_h, need_v, divisor,
                                (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_augment_u8(unet_ctx* c, const uint8_t* src, int h, int w, uint8_t* dst,
                    const unet_aug_params* params, unet_stream_t stream) {
    ABI_TRY
    if (!c || !src || !dst || !params || src == dst) return UNET_ERR_INVALID;
    if (int r = aug_params_check(params, h, w))
        return fail(c, r, "augment: plane %d x %d, mode %d, %d TGC bands", h, w, params->mode,
                    params->num_bins);
    return launched(c, "augment", k_augment_u8(src, h, w, dst, *params, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_augment_u8_host(const uint8_t* src, int h, int w, uint8_t* dst,
                         const unet_aug_params* params) {
    if (!src || !dst || !params || src == dst) return UNET_ERR_INVALID;
    if (int r = aug_params_check(params, h, w)) return r;
    augment_u8_host(src, h, w, dst, *params);
    return UNET_OK;
}

int unet_augment_noise_u8(unet_ctx* c, const uint8_t* src, int h, int w, uint8_t* dst,
                          const unet_aug_params* params, const double* noise,
                          unet_stream_t stream) {
    ABI_TRY
    if (!c || !src || !dst || !params || src == dst) return UNET_ERR_INVALID;
    if (int r = aug_params_check(params, h, w))
        return fail(c, r, "augment: plane %d x %d, mode %d, %d TGC bands", h, w, params->mode,
                    params->num_bins);
    return launched(c, "augment", k_augment_u8(src, h, w, dst, *params, (hipStream_t)stream, noise));
    ABI_CATCH(c)
}

int unet_augment_noise_u8_host(const uint8_t* src, int h, int w, uint8_t* dst,
                               const unet_aug_params* params, const double* noise) {
    if (!src || !dst || !params || src == dst) return UNET_ERR_INVALID;
    if (int r = aug_params_check(params, h, w)) return r;
    augment_u8_host(src, h, w, dst, *params, noise);
    return UNET_OK;
}

// both entry points: which planes are asked for, and whether they may be written
static bool elastic_args_ok(const uint8_t* img, const uint8_t* mask, const uint8_t* img_dst,
                            const uint8_t* mask_dst, const double* rx, const double* ry,
                            const unet_elastic_params* p) {
    return p && rx && ry && (img || mask) && (!img || (img_dst && img_dst != img)) &&
           (!mask || (mask_dst && mask_dst != mask));
}

int unet_elastic_u8(unet_ctx* c, const uint8_t* img, const uint8_t* mask, int h, int w,
                    uint8_t* img_dst, uint8_t* mask_dst, const double* rx, const double* ry,
                    const unet_elastic_params* params, unet_stream_t stream) {
    ABI_TRY
    if (!c || !elastic_args_ok(img, mask, img_dst, mask_dst, rx, ry, params)) return UNET_ERR_INVALID;
    if (int r = elastic_check(params, h, w))
        return fail(c, r, "elastic: plane %d x %d, ksize %d", h, w, params->ksize);
    if (int r = grow(c, c->elastic, elastic_scratch_bytes(h, w), "elastic")) return r;
    return launched(c, "elastic",
                    k_elastic_u8(img, mask, h, w, img_dst, mask_dst, rx, ry, *params, (double*)c->elastic.p,
                                 (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_elastic_u8_host(const uint8_t* img, const uint8_t* mask, int h, int w, uint8_t* img_dst,
                         uint8_t* mask_dst, const double* rx, const double* ry,
                         const unet_elastic_params* params) {
    if (!elastic_args_ok(img, mask, img_dst, mask_dst, rx, ry, params)) return UNET_ERR_INVALID;
    if (int r = elastic_check(params, h, w)) return r;
    return catch_to_status([&] {
        std::vector<double> tmp(2 * (size_t)h * w);
        elastic_u8_host(img, mask, h, w, img_dst, mask_dst, rx, ry, *params, tmp.data());
    });
}

int unet_clahe_u8(unet_ctx* c, const uint8_t* src, int h, int w, uint8_t* dst, double clip, int gx,
                  int gy, unet_stream_t stream) {
    ABI_TRY
    if (!c || !src || !dst) return UNET_ERR_INVALID;
    ClaheGeom G;
    if (int r = clahe_geom(h, w, clip, gx, gy, G))
        return fail(c, r, "clahe: plane %d x %d, grid %d x %d", h, w, gx, gy);
    if (int r = grow(c, c->clahe, clahe_scratch_bytes(G), "clahe")) return r;
    return launched(c, "clahe", k_clahe_u8(src, dst, G, c->clahe.p, (hipStream_t)stream));
    ABI_CATCH(c)
}

int unet_clahe_u8_host(const uint8_t* src, int h, int w, uint8_t* dst, double clip, int gx,
                       int gy) {
    if (!src || !dst) return UNET_ERR_INVALID;
    ClaheGeom G;
    if (int r = clahe_geom(h, w, clip, gx, gy, G)) return r;
    return catch_to_status([&] {
        std::vector<int> hist((size_t)gx * gy * 256);
        std::vector<uint8_t> lut((size_t)gx * gy * 256);
        clahe_u8_host(src, dst, G, hist.data(), lut.data());
    });
}

}  // extern "C"
