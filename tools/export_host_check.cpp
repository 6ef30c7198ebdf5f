// export.h compiled for the host alone (-DEXPORT_HOST_ONLY, no HIP header) as a stand-alone program:
// the plan, the resize and the overlay twins (the rules of the plot they replace, the reference's
// utils/trainer.py:262-299, are in export.h) run over the edge shapes of the tests and are checked
// against a direct restatement.  Meant to be built with -fsanitize=address,undefined:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DEXPORT_HOST_ONLY \
//         -I thyroid-nodule-image-segmentation-unet-ddti_amd/csrc tools/export_host_check.cpp -o export_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "export.h"

static uint32_t rng_state = 2463534242u;
static float rnd() {  // uniform in [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) / 16777216.0f;
}

static int fails = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__); \
            ++fails;                                            \
        }                                                       \
    } while (0)

struct Plan {
    std::vector<double> k;
    std::vector<int32_t> b;
    int ks;
};

static Plan make_plan(int in, int out) {
    Plan p;
    p.ks = export_resize_plan(in, out, nullptr, nullptr);
    // exact sizes: a write past either table is an ASan report
    p.k.assign((size_t)out * p.ks, -1.0);
    p.b.assign(2 * (size_t)out, -1);
    CHECK(export_resize_plan(in, out, p.k.data(), p.b.data()) == p.ks);
    for (int xx = 0; xx < out; ++xx) {
        const int first = p.b[2 * xx], count = p.b[2 * xx + 1];
        CHECK(first >= 0 && count >= 1 && count <= p.ks && first + count <= in);
        double s = 0;
        for (int t = 0; t < p.ks; ++t) {
            CHECK(p.k[(size_t)xx * p.ks + t] >= 0.0);
            if (t >= count) CHECK(p.k[(size_t)xx * p.ks + t] == 0.0);
            s += p.k[(size_t)xx * p.ks + t];
        }
        CHECK(s > 1.0 - 1e-12 && s < 1.0 + 1e-12);
    }
    return p;
}

static void resize_case(int h, int w, int oh, int ow) {
    std::vector<float> src((size_t)h * w);
    for (float& v : src) v = 12.f * (rnd() - 0.5f);
    const Plan ph = make_plan(w, ow), pv = make_plan(h, oh);
    const bool nh = ow != w, nv = oh != h;
    std::vector<float> tmp(nh ? (size_t)h * ow : 0), plane((size_t)oh * ow, -7.f);
    std::vector<uint8_t> mask((size_t)oh * ow, 9), mask2((size_t)oh * ow, 9);
    for (int kind : {EXPORT_SIGMOID_HALF, EXPORT_GREATER}) {
        export_resize_mask_host(src.data(), h, w, oh, ow, nh ? ph.k.data() : nullptr, nh ? ph.b.data() : nullptr, ph.ks,
                                nv ? pv.k.data() : nullptr, nv ? pv.b.data() : nullptr, pv.ks, kind, 0.25f, tmp.data(),
                                plane.data(), mask.data());
        export_resize_mask_host(src.data(), h, w, oh, ow, nh ? ph.k.data() : nullptr, nh ? ph.b.data() : nullptr, ph.ks,
                                nv ? pv.k.data() : nullptr, nv ? pv.b.data() : nullptr, pv.ks, kind, 0.25f, tmp.data(),
                                nullptr, mask2.data());
        CHECK(mask == mask2);
        // the direct restatement: both passes written out, long double sums as a bound
        for (int yy = 0; yy < oh; ++yy)
            for (int xx = 0; xx < ow; ++xx) {
                long double ss = 0;
                const int fy = nv ? pv.b[2 * yy] : yy, cy = nv ? pv.b[2 * yy + 1] : 1;
                for (int a = 0; a < cy; ++a) {
                    const int fx = nh ? ph.b[2 * xx] : xx, cx = nh ? ph.b[2 * xx + 1] : 1;
                    long double row = 0;
                    for (int b = 0; b < cx; ++b)
                        row += (long double)src[(size_t)(fy + a) * w + fx + b] * (nh ? ph.k[(size_t)xx * ph.ks + b] : 1.0);
                    ss += (long double)(float)row * (nv ? pv.k[(size_t)yy * pv.ks + a] : 1.0);
                }
                const float got = plane[(size_t)yy * ow + xx];
                CHECK(fabsl((long double)got - ss) <= 2e-6L * (1.0L + fabsl(ss)));
                const bool fg = kind == EXPORT_GREATER ? got > 0.25f : surf_pred(got);
                CHECK(mask[(size_t)yy * ow + xx] == (fg ? 1 : 0));
            }
    }
    if (!nh && !nv)
        for (size_t i = 0; i < src.size(); ++i) CHECK(plane[i] == src[i]);
}

static void overlay_case(int h, int w, const std::vector<uint8_t>& pred, bool with_gt) {
    std::vector<uint8_t> gray((size_t)h * w), gt((size_t)h * w);
    for (auto& v : gray) v = (uint8_t)(rnd() * 256.f);
    for (size_t i = 0; i < gt.size(); ++i) gt[i] = pred[(i + 1) % pred.size()];
    for (int r = 1; r <= 3; ++r)
        for (int alpha : {0, 96, 256}) {
            std::vector<uint8_t> rgb(3 * (size_t)h * w, 7);
            int64_t st[EXPORT_STAT_FIELDS];
            export_overlay_host(gray.data(), pred.data(), with_gt ? gt.data() : nullptr, h, w, r, alpha, rgb.data(), st);
            int64_t area = 0, cont = 0, x0 = -1, y0 = -1, x1 = -1, y1 = -1;
            auto at = [&](const std::vector<uint8_t>& m, int i, int j) {
                return i >= 0 && i < h && j >= 0 && j < w && m[(size_t)i * w + j] != 0;
            };
            auto is_contour = [&](const std::vector<uint8_t>& m, int i, int j) {
                if (!at(m, i, j)) return false;
                for (int y = i - r; y <= i + r; ++y)
                    for (int x = j - r; x <= j + r; ++x)
                        if (std::abs(y - i) + std::abs(x - j) <= r && !at(m, y, x)) return true;
                return false;
            };
            for (int i = 0; i < h; ++i)
                for (int j = 0; j < w; ++j) {
                    const int g = gray[(size_t)i * w + j];
                    int R = g, G = g, B = g;
                    const bool fg = at(pred, i, j), cp = is_contour(pred, i, j);
                    if (fg) {
                        ++area, cont += cp;
                        x0 = x0 < 0 || j < x0 ? j : x0, y0 = y0 < 0 || i < y0 ? i : y0;
                        x1 = j > x1 ? j : x1, y1 = i > y1 ? i : y1;
                    }
                    if (fg && !cp && alpha) R = (g * (256 - alpha) + 255 * alpha + 128) >> 8, G = B = (g * (256 - alpha) + 128) >> 8;
                    if (with_gt && is_contour(gt, i, j)) R = 0, G = 0, B = 255;
                    if (cp) R = 255, G = 0, B = 0;
                    const uint8_t* o = &rgb[3 * ((size_t)i * w + j)];
                    CHECK(o[0] == R && o[1] == G && o[2] == B);
                }
            CHECK(st[0] == area && st[1] == cont && st[2] == x0 && st[3] == y0 && st[4] == x1 && st[5] == y1);
        }
}

int main() {
    const int shapes[][4] = {{16, 16, 23, 37}, {16, 16, 7, 5},  {16, 16, 16, 31}, {16, 16, 31, 16}, {16, 16, 16, 16},
                             {48, 48, 360, 560}, {16, 16, 1, 1}, {16, 16, 1, 40},  {1, 1, 5, 3},     {33, 47, 11, 9}};
    for (const auto& s : shapes) resize_case(s[0], s[1], s[2], s[3]);
    {  // a table that names taps outside the plane is clamped, not followed
        int first = -3, count = 99;
        export_clamp_taps(16, 3, first, count);
        CHECK(first == 0 && count == 3);
        first = 15, count = 3;
        export_clamp_taps(16, 3, first, count);
        CHECK(first == 15 && count == 1);
        first = 40, count = 2;
        export_clamp_taps(16, 3, first, count);
        CHECK(first == 16 && count == 0);
    }
    const int sizes[][2] = {{5, 7}, {17, 65}, {1, 1}, {1, 9}, {9, 1}, {90, 140}};
    for (const auto& s : sizes) {
        const int h = s[0], w = s[1];
        const size_t n = (size_t)h * w;
        std::vector<uint8_t> m(n, 0);
        overlay_case(h, w, m, true);  // empty
        m.assign(n, 255);
        overlay_case(h, w, m, false);  // full
        m.assign(n, 0);
        m[n - 1] = 1;
        overlay_case(h, w, m, true);  // one pixel in a corner
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) m[(size_t)i * w + j] = (i - h / 2) * (i - h / 2) + (j - w / 3) * (j - w / 3) <= (h * h) / 9;
        overlay_case(h, w, m, true);  // disc
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) m[(size_t)i * w + j] = j % 3 == 0;
        overlay_case(h, w, m, true);  // vertical stripes
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) m[(size_t)i * w + j] = i % 3 != 1;
        overlay_case(h, w, m, false);  // horizontal stripes
        for (size_t i = 0; i < n; ++i) m[i] = rnd() < 0.6f;
        overlay_case(h, w, m, true);  // noise
    }
    if (fails) return 1;
    std::printf("export_host_check ok\n");
    return 0;
}
