// echo.h compiled for the host alone (-DECHO_HOST_ONLY, no HIP header) as a stand-alone program: the
// host twin runs over the shapes of the shared case list (tests/echo_ref.py: the smallest planes, sides
// off the tile size, a component across the seams and on all four borders, diagonal neighbours, two
// components closer than the ring, single-pixel components with distinct labels, counts 0 / 1 / many,
// max_rows below the largest label, negative background; every ring width and level count) and is
// checked against a brute-force restatement (the whole window of every background pixel, every pair).
// Every buffer is sized exactly and the table carries guard words and starts as garbage, so a
// sanitizer sees an access past either end and the check sees a word the call did not clear.
// Meant to be built with -fsanitize=address,undefined:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DECHO_HOST_ONLY \
//         -I thyroid-nodule-image-segmentation-unet-ddti_amd/csrc tools/echo_host_check.cpp -o echo_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "echo.h"

static uint32_t rng_state = 2025u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static int fails = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__); \
            ++fails;                                            \
        }                                                       \
    } while (0)

struct Case {
    int N, H, W;
    std::vector<int32_t> lab, count;
    std::vector<uint8_t> gray;
    Case(int n, int h, int w) : N(n), H(h), W(w), lab((size_t)n * h * w, 0), count((size_t)n, 0), gray((size_t)n * h * w) {
        for (auto& g : gray) g = (uint8_t)(rnd() & 255);
    }
    int32_t& at(int n, int y, int x) { return lab[((size_t)n * H + y) * W + x]; }
    void box(int n, int y0, int y1, int x0, int x1, int l) {
        for (int y = y0; y < y1 && y < H; ++y)
            for (int x = x0; x < x1 && x < W; ++x) at(n, y, x) = l;
        if (l > count[n]) count[n] = l;
    }
};

// the rules, pixel by pixel
static std::vector<int32_t> brute(const Case& c, int64_t max_rows, int G, int w) {
    const int F = 512 + G * G;
    std::vector<int32_t> t((size_t)c.N * max_rows * F, 0);
    static const int DY[4] = {0, 1, 1, 1}, DX[4] = {1, 1, 0, -1};
    for (int n = 0; n < c.N; ++n) {
        const int32_t* L = c.lab.data() + (size_t)n * c.H * c.W;
        const uint8_t* g = c.gray.data() + (size_t)n * c.H * c.W;
        int32_t* T = t.data() + (size_t)n * max_rows * F;
        int64_t K = c.count[n] < 0 ? 0 : c.count[n];
        if (K > max_rows) K = max_rows;
        for (int y = 0; y < c.H; ++y)
            for (int x = 0; x < c.W; ++x) {
                const int l = L[y * c.W + x];
                if (l > 0) {
                    if (l > K) continue;
                    T[(size_t)(l - 1) * F + g[y * c.W + x]] += 1;
                    for (int k = 0; k < 4; ++k) {
                        const int yy = y + DY[k], xx = x + DX[k];
                        if (yy < 0 || yy >= c.H || xx < 0 || xx >= c.W || L[yy * c.W + xx] != l) continue;
                        const int qa = (g[y * c.W + x] * G) >> 8, qb = (g[yy * c.W + xx] * G) >> 8;
                        T[(size_t)(l - 1) * F + 512 + qa * G + qb] += 1;
                    }
                    continue;
                }
                int own = 0;
                for (int yy = y - w; yy <= y + w && w > 0; ++yy)
                    for (int xx = x - w; xx <= x + w; ++xx) {
                        if (yy < 0 || yy >= c.H || xx < 0 || xx >= c.W) continue;
                        const int v = L[yy * c.W + xx];
                        if (v > 0 && (own == 0 || v < own)) own = v;
                    }
                if (own > 0 && own <= K) T[(size_t)(own - 1) * F + 256 + g[y * c.W + x]] += 1;
            }
    }
    return t;
}

static void run(const char* name, const Case& c, int64_t max_rows, int G, int w) {
    const size_t words = (size_t)c.N * max_rows * (512 + G * G), guard = 8;
    std::vector<int32_t> buf(words + 2 * guard);
    for (auto& v : buf) v = (int32_t)0xA5A5A5A5u;  // garbage the call has to clear, and the guards
    echo_host(c.gray.data(), c.lab.data(), c.count.data(), c.N, c.H, c.W, max_rows, G, w, buf.data() + guard);
    const std::vector<int32_t> want = brute(c, max_rows, G, w);
    bool same = true, guards = true;
    for (size_t i = 0; i < words; ++i) same &= buf[guard + i] == want[i];
    for (size_t i = 0; i < guard; ++i) guards &= buf[i] == (int32_t)0xA5A5A5A5u && buf[guard + words + i] == (int32_t)0xA5A5A5A5u;
    if (!same || !guards) {
        std::printf("FAILED %s (G %d, w %d, max_rows %lld): table %s, guards %s\n", name, G, w, (long long)max_rows,
                    same ? "equal" : "DIFFERS", guards ? "intact" : "OVERWRITTEN");
        ++fails;
    }
}

static void all_settings(const char* name, const Case& c, int64_t max_rows) {
    static const int GS[3] = {8, 16, 32}, WS[4] = {0, 1, 8, 16};
    for (int G : GS)
        for (int w : WS) run(name, c, max_rows, G, w);
}

int main() {
    {
        Case c(1, 1, 1);
        c.box(0, 0, 1, 0, 1, 1);
        all_settings("1x1", c, 1);
    }
    {
        Case a(1, 1, 70), b(1, 70, 1);
        a.box(0, 0, 1, 58, 67, 1);
        b.box(0, 58, 67, 0, 1, 1);
        all_settings("1x70", a, 1);
        all_settings("70x1", b, 1);
    }
    {   // 67 x 131: a cross over every seam, boxes near it, one of them on the corner
        Case c(1, 67, 131);
        c.box(0, 30, 35, 0, 131, 1);
        c.box(0, 0, 67, 62, 67, 1);
        c.box(0, 0, 10, 0, 12, 2);
        c.box(0, 40, 50, 70, 90, 3);
        c.box(0, 52, 67, 100, 131, 4);
        all_settings("67x131", c, 4);
        all_settings("67x131 rows 2", c, 2);
        all_settings("67x131 rows 9", c, 9);
        for (auto& g : c.gray) g = 93;
        all_settings("67x131 constant", c, 4);
        for (size_t i = 0; i < c.gray.size(); ++i) c.gray[i] = (uint8_t)((i % 131) & 255);
        all_settings("67x131 ramp", c, 4);
    }
    {   // a frame on all four borders and an island in it
        Case c(1, 40, 70);
        c.box(0, 0, 40, 0, 70, 1);
        c.box(0, 3, 37, 3, 67, 0);
        c.box(0, 10, 20, 20, 40, 2);
        all_settings("frame", c, 2);
    }
    {   // diagonal neighbours; two bars closer than the ring
        Case c(1, 20, 40);
        c.box(0, 4, 10, 4, 10, 1);
        c.box(0, 10, 16, 10, 16, 2);
        c.box(0, 2, 18, 25, 28, 3);
        c.box(0, 2, 18, 31, 34, 4);
        all_settings("diagonal and bars", c, 4);
    }
    {   // single-pixel components with distinct labels, negative background between them
        Case c(1, 33, 70);
        int k = 0;
        for (int y = 0; y < 33; ++y)
            for (int x = 0; x < 70; ++x) c.at(0, y, x) = (y + x) % 2 == 0 ? ++k : -(int)(rnd() % 3);
        c.count[0] = k;
        all_settings("checkerboard", c, k);
        all_settings("checkerboard rows 100", c, 100);
    }
    {   // N = 3: counts 0, 1, many; a count below the labels present (they are dropped)
        Case c(3, 37, 66);
        c.box(1, 5, 30, 10, 60, 1);
        int k = 0;
        for (int y = 0; y < 37; y += 3)
            for (int x = 0; x < 66; x += 4) c.box(2, y, y + 2, x, x + 3, ++k);
        all_settings("N3", c, k);
        all_settings("N3 rows 3", c, 3);
        c.count[2] = 5;
        all_settings("N3 short count", c, k);
        c.count[2] = -4;
        all_settings("N3 negative count", c, 2);
    }
    CHECK(echo_args_invalid(nullptr, &fails, &fails, &fails, 1, 1, 1, 1, 16, 8) != nullptr);
    CHECK(echo_args_invalid(&fails, &fails, &fails, &fails, 1, 1, 1, 1, 16, 8) == nullptr);
    CHECK(echo_args_invalid(&fails, &fails, &fails, &fails, 1, 1, 1, 0, 16, 8) != nullptr);
    CHECK(echo_args_invalid(&fails, &fails, &fails, &fails, 1, 1, 1, 1, 12, 8) != nullptr);
    CHECK(echo_args_invalid(&fails, &fails, &fails, &fails, 1, 1, 1, 1, 16, 17) != nullptr);
    CHECK(echo_args_invalid(&fails, &fails, &fails, &fails, 1, 1, 1, 1, 16, -1) != nullptr);
    CHECK(echo_shape_ok(4096, 4096) && !echo_shape_ok(4097, 1) && !echo_shape_ok(1, 4097));
    CHECK(echo_fields(8) == 576 && echo_fields(32) == 1536 && echo_quant(255, 32) == 31 && echo_quant(0, 8) == 0);
    if (fails) {
        std::printf("echo_host_check: %d failures\n", fails);
        return 1;
    }
    std::printf("echo_host_check ok\n");
    return 0;
}
