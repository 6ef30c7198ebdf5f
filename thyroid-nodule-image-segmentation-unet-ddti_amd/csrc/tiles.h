// The GEMM tiles, named once (host only; included at the end of common.h).  Seven id spaces, one per
// kernel family: an enum whose enumerators carry the ids of the option ABI (unet_set_option
// "rg16_tile" 19, tests/kernel_cases.py), one constant table of descriptors, one lookup, and next
// to them the eligibility rule of each tile kind -- asked by the runtime where it picks a tile
// (make_plan) and by the launcher where it checks its arguments.  The kernel files static_assert
// each row against its template type, so a row cannot drift from its kernel.
#pragma once

enum TileKind : uint8_t {
    K_REG,         // operands staged through registers into one LDS image
    K_REG2,        // ... into two LDS images (label tag d)
    K_PIPE,        // software-pipelined, global loads two chunks ahead (kernels_gemm_pipe.hip)
    K_DIRECT,      // operands straight from global memory
    K_DMA,         // LDS-DMA, one tap per block
    K_HALO,        // tap-row halo row GEMM: the three dx taps of a 3x3 conv from one halo row
    K_TAPROW,      // tap-row weight gradient: one row of 3x3 taps (three accumulator sets) per block
    K_TAPROW_M16,  // ... on 16x16x32 MFMAs with the re-read stagger
};

struct Tile {
    int id;
    int bm, bn;     // block tile (tap-row weight gradients: per tap; bm = channels of ONE tap)
    int bk;         // what the family's label prints third: K chunk / pixel chunk / LDS stages
    int taps;       // taps of the M dimension one block covers (1 or 3)
    int per_cu;     // block slots per CU (0: nothing reads it)
    int per4;       // blocks the split-K target counts as one four-wave block
    TileKind kind;
    bool dz;        // the OP_DZ loader (dz formed inside the weight gradient) is instantiated
    const char* tag;
    int fallback;   // K_PIPE: the same shape on the register-staged kernel
};

template <int N>
constexpr const Tile* find_tile(const Tile (&tab)[N], int id) {
    for (int i = 0; i < N; ++i)
        if (tab[i].id == id) return &tab[i];
    return nullptr;
}
// what a label prints and a launcher refuses where an option names no tile
inline constexpr Tile NO_TILE = {-1, 0, 0, 0, 1, 0, 1, K_REG, false, "", -1};
inline const Tile& tile_or_none(const Tile* t) { return t ? *t : NO_TILE; }

// f32 / register-staged row GEMM (kernels_gemm.hip, kernels_gemm_pipe.hip); label rowgemm_BMxBNxBK
enum RowTileId {
    RG_128x128D = 0, RG_128x64 = 1, RG_128x128 = 4, RG_128x128K64 = 6, RG_128x32 = 13, RG_256x32 = 14,
    RG_256x32G = 15, RG_P128x128 = 18, RG_P128x64 = 19, RG_P3_128x64 = 25, RG_P3_128x64A = 26,
};
inline constexpr Tile ROW_TILES[] = {
    {RG_128x128D, 128, 128, 32, 1, 0, 1, K_REG2, false, "d", -1},   // two LDS images
    {RG_128x64, 128, 64, 32, 1, 0, 1, K_REG, false, "", -1},        // 64 outputs; the bf16 tile of N % 128 != 0
    {RG_128x128, 128, 128, 32, 1, 0, 1, K_REG, false, "", -1},
    {RG_128x128K64, 128, 128, 64, 1, 0, 1, K_REG2, false, "d", -1}, // bf16: 64 K per barrier (4 MFMA k-steps)
    {RG_128x32, 128, 32, 32, 1, 0, 1, K_REG2, false, "d", -1},      // 32 outputs (narrow networks' level 0), 2 waves
    {RG_256x32, 256, 32, 32, 1, 0, 1, K_REG2, false, "d", -1},      // ... 4 waves, LDS-staged
    // 32 outputs, 32-k chunks, two waves per SIMD (r04, ResUNet(32, 4) 263 -> 282 img/s)
    {RG_256x32G, 256, 32, 32, 1, 0, 1, K_DIRECT, false, "g", -1},
    // r02 A/B (config 2) 401 img/s against 390 for the register-staged tiles, identical bits
    {RG_P128x128, 128, 128, 32, 1, 0, 1, K_PIPE, false, "p", RG_128x128},
    {RG_P128x64, 128, 64, 32, 1, 0, 1, K_PIPE, false, "p", RG_128x64},  // level-0 128 -> 64 conv 112 -> 117 TF/s
    // 128x64 at three blocks per CU (48 KB of LDS each): a third resident block overlaps the
    // epilogues of the short-K GEMMs; loading one / two chunks ahead
    {RG_P3_128x64, 128, 64, 32, 1, 3, 1, K_PIPE, false, "p", RG_128x64},
    {RG_P3_128x64A, 128, 64, 32, 1, 3, 1, K_PIPE, false, "p", RG_128x64},
};
constexpr const Tile* row_desc(int id) { return find_tile(ROW_TILES, id); }

// f32 weight gradient (kernels_gemm.hip); label wgrad[3]_BMxBNxpixels.  The row3 tiles (tag 3) take
// one row of 3x3 taps per block; every tile has the dz loader
enum WgTileId {
    WG_128x128 = 0, WG_64x128 = 3, WG_128x64 = 5, WG_64x64 = 7, WG_64x32 = 8, WG_32x32 = 9,
    WG3_64x64 = 20, WG3_128x64 = 21, WG3_64x128 = 22, WG3_128x128 = 23, WG3_32x32 = 24, WG3_64x32 = 25,
    WG3_32x64 = 26,
};
inline constexpr Tile WG_TILES[] = {
    {WG_128x128, 128, 128, 32, 1, 0, 1, K_REG, true, "", -1},  // 4 waves
    {WG_64x128, 64, 128, 32, 1, 0, 1, K_REG, true, "", -1},    // 2 waves
    {WG_128x64, 128, 64, 32, 1, 0, 1, K_REG, true, "", -1},    // 4 waves
    {WG_64x64, 64, 64, 32, 1, 0, 1, K_REG, true, "", -1},      // 64-channel layers, 3 waves / SIMD
    {WG_64x32, 64, 32, 32, 1, 0, 1, K_REG, true, "", -1},      // 32-channel operands (narrow level 0)
    {WG_32x32, 32, 32, 32, 1, 0, 1, K_REG, true, "", -1},
    {WG3_64x64, 64, 64, 32, 3, 0, 1, K_TAPROW, true, "3", -1},    // 4 waves, 3 x 32x32 per wave
    // the default where Cin, Cout % 128 == 0: 126 TF/s as 128x128 but half its split-K slices
    {WG3_128x64, 128, 64, 32, 3, 0, 1, K_TAPROW, true, "3", -1},
    {WG3_64x128, 64, 128, 32, 3, 0, 1, K_TAPROW, true, "3", -1},
    {WG3_128x128, 128, 128, 32, 3, 0, 1, K_TAPROW, true, "3", -1},  // 192 accumulators
    // 32-channel operands (r04): one / two waves, so 4 / 2 blocks per four-wave block
    {WG3_32x32, 32, 32, 32, 3, 0, 4, K_TAPROW, true, "3", -1},
    {WG3_64x32, 64, 32, 32, 3, 0, 2, K_TAPROW, true, "3", -1},  // Cin 64 (a [skip | up] concat), Cout 32
    {WG3_32x64, 32, 64, 32, 3, 0, 2, K_TAPROW, true, "3", -1},
};
constexpr const Tile* wg_desc(int id) { return find_tile(WG_TILES, id); }

// register-staged bf16 weight gradient (channel-major wgradT_kernel); same label
enum WgBfTileId { WGB_128x128 = 0, WGB_64x64 = 2, WGB_128x64 = 3, WGB_64x128 = 4 };
inline constexpr Tile WGB_TILES[] = {
    {WGB_128x128, 128, 128, 32, 1, 0, 1, K_REG, false, "", -1},
    {WGB_64x64, 64, 64, 64, 1, 0, 1, K_REG, false, "", -1},  // narrow tiles: 64-pixel chunks
    {WGB_128x64, 128, 64, 64, 1, 0, 1, K_REG, false, "", -1},
    {WGB_64x128, 64, 128, 64, 1, 0, 1, K_REG, false, "", -1},
};
constexpr const Tile* wgb_desc(int id) { return find_tile(WGB_TILES, id); }

// rg16: LDS-DMA bf16 row GEMM (kernels_gemm16.hip); label rg16[r3]_BMxBNs<stages>
enum Rg16TileId {
    R16_128x128 = 0, R16_256x128 = 2, R16_256x256 = 4, R16_512x128 = 6, R16_H256x256 = 19,
    R16_H512x128 = 20,
};
inline constexpr Tile RG16_TILES[] = {
    {R16_128x128, 128, 128, 2, 1, 2, 1, K_DMA, false, "", -1},  // 64 KB LDS: small grids, hidden epilogues
    {R16_256x128, 256, 128, 2, 1, 1, 1, K_DMA, false, "", -1},  // 8 waves, 96 KB
    {R16_256x256, 256, 256, 2, 1, 1, 1, K_DMA, false, "", -1},  // 8 waves of 128x64, 128 KB
    {R16_512x128, 512, 128, 2, 1, 1, 1, K_DMA, false, "", -1},  // 160 KB: the 128-output layers
    {R16_H256x256, 256, 256, 2, 1, 1, 1, K_HALO, false, "r3", -1},  // config 4 +0.9..1.2 % (r03)
    {R16_H512x128, 512, 128, 2, 1, 1, 1, K_HALO, false, "r3", -1},  // r04 config 4 122.7 -> 124.8 img/s
};
constexpr const Tile* rg16_desc(int id) { return find_tile(RG16_TILES, id); }

// wg16: LDS-DMA bf16 weight gradient, transposed reads; label wg16[r3|r3m]_BMxBNs<stages>
enum Wg16TileId { W16_128x128 = 0, W16_256x256 = 2, W16_R3 = 4, W16_R3M = 7 };
inline constexpr Tile WG16_TILES[] = {
    {W16_128x128, 128, 128, 2, 1, 2, 1, K_DMA, false, "", -1},  // 64 pixels per stage, 64 KB
    {W16_256x256, 256, 256, 2, 1, 1, 1, K_DMA, false, "", -1},  // 8 waves of 128x64, 128 KB
    {W16_R3, 128, 128, 4, 3, 1, 1, K_TAPROW, false, "r3", -1},  // 32x32x16 MFMAs (r04 122.7 -> 125.2 img/s)
    // r06, config 4 +1.3 % over W16_R3; also the deep levels' W = 32 / 16 (+1.4 %)
    {W16_R3M, 128, 128, 4, 3, 1, 1, K_TAPROW_M16, false, "r3m", -1},
};
constexpr const Tile* wg16_desc(int id) { return find_tile(WG16_TILES, id); }

// x3 row GEMM (kernels_gemm_x3.hip); label x3[r3]_BMxBN
enum X3TileId {
    X3_256x128 = 0, X3_128x128 = 1, X3_128x64 = 2, X3_256x64 = 3, X3_H256x128 = 4, X3_H128x64 = 6,
};
inline constexpr Tile X3_TILES[] = {
    {X3_256x128, 256, 128, 32, 1, 1, 1, K_DMA, false, "", -1},  // 8 waves of 64x64, 144 KB
    {X3_128x128, 128, 128, 32, 1, 1, 1, K_DMA, false, "", -1},  // grids below 256 blocks of 256x128
    {X3_128x64, 128, 64, 32, 1, 2, 1, K_DMA, false, "", -1},    // the 64-output layers
    {X3_256x64, 256, 64, 32, 1, 1, 1, K_DMA, false, "", -1},    // 8 waves of 64x32
    {X3_H256x128, 256, 128, 32, 1, 1, 1, K_HALO, false, "r3", -1},  // one block of 8 waves per CU
    // r05: 0.2 % over a 256x64 halo tile, 1.032 vs 1.103 ms for a 512x64 one
    {X3_H128x64, 128, 64, 32, 1, 2, 1, K_HALO, false, "r3", -1},
};
constexpr const Tile* x3_desc(int id) { return find_tile(X3_TILES, id); }

// x3 weight gradient; label wx3[r3]_BMxBN, 32-pixel chunks
enum Wx3TileId { WX3_128x128 = 0, WX3_64x64 = 1, WX3_R3_64x128 = 2, WX3_R3_64x64 = 4 };
inline constexpr Tile WX3_TILES[] = {
    {WX3_128x128, 128, 128, 32, 1, 1, 1, K_DMA, false, "", -1},
    {WX3_64x64, 64, 64, 32, 1, 2, 1, K_DMA, false, "", -1},
    {WX3_R3_64x128, 64, 128, 32, 3, 1, 1, K_TAPROW, false, "r3", -1},  // four stages with the stagger
    // 4 waves, two LDS stages (r06: config 2's 128 -> 64 conv 1.53 -> 1.24 ms against 128x64)
    {WX3_R3_64x64, 64, 64, 32, 3, 2, 1, K_TAPROW, false, "r3", -1},
};
constexpr const Tile* wx3_desc(int id) { return find_tile(WX3_TILES, id); }

// ---- eligibility: one rule per tile kind, a function of the descriptor and the GEMM's geometry ----
// a row GEMM: gather and epilogue mode, sizes, row width, E_CONVT's cout
struct RowGeom { int amode, emode, M, N, K, W, cout; };
// a weight gradient; pps = 0 before the split is chosen
struct WgGeom { int amode, bmode; int64_t P; int CA, CB, H, W, pps; };
inline RowGeom row_geom(const RowGemmArgs& a) { return {a.amode, a.emode, a.M, a.N, a.K, a.W, a.cout}; }
inline WgGeom wgrad_geom(const WgradArgs& a) { return {a.amode, a.bmode, a.P, a.CA, a.CB, a.H, a.W, a.pps}; }
// halo row GEMMs (rg16, x3): BM % W == 0 or W % BM == 0 keeps a tile on whole rows / row
// segments; W >= 16 bounds the halo
inline bool halo_ok(const Tile& t, const RowGeom& g) {
    return g.amode == G_CONV3 && g.W >= 16 && !(t.bm % g.W && g.W % t.bm);
}
inline bool conv_wgrad(const WgGeom& g) { return g.amode == G_CONV3 && g.bmode == G_IDENT && g.W > 0; }
// f32 row3: rows and pixel splits in whole pixel chunks
inline bool wg_row3_ok(const Tile& t, const WgGeom& g) {
    return conv_wgrad(g) && g.W % t.bk == 0 && g.CA % t.bm == 0 && g.CB % t.bn == 0 && g.pps % t.bk == 0;
}
// wg16 tap-row: row widths (the m16 tile also the deep levels' 32 / 16) ...
inline bool wg16_row3_rows(const Tile& t, int W) {
    return W % 64 == 0 || (t.kind == K_TAPROW_M16 && (W == 32 || W == 16));
}
// ... whole 64-pixel chunks per image and per split
inline bool wg16_row3_ok(const Tile& t, const WgGeom& g) {
    return conv_wgrad(g) && g.CA % t.bm == 0 && g.CB % t.bn == 0 && wg16_row3_rows(t, g.W) &&
           (g.H * g.W) % 64 == 0 && g.pps % 64 == 0 && g.P % 64 == 0;
}
// x3 tap-row: rows of 32k pixels, or (r05) 16-pixel rows in pairs
inline bool wx3_row3_ok(const Tile& t, const WgGeom& g) {
    return conv_wgrad(g) && g.CA % t.bm == 0 && g.CB % t.bn == 0 &&
           (g.W % 32 == 0 || (g.W == 16 && g.H % 2 == 0)) && g.pps % 32 == 0 && g.P % 32 == 0;
}
