// The conv tile table: which tiles exist, their geometry, which kernels may launch them, and how a
// `cfg` argument of the C ABI names one.  Constexpr data and host helpers only: run_halo
// (conv_halo_x3.hip) validates and sizes grids from it, the launchers (conv_halo.h launch_family,
// conv_pw.hip launch_pw) instantiate kernels from it.  Adding or retiring a tile is one row here
// (plus tests/conv_tiles.py, the tests' own statement of the accepted ids).
#pragma once
#include <string>

namespace fsmi {
namespace halo {

enum TileFamily : unsigned {   // who may launch a halo tile
  kTileS1 = 1,        // stride-1 1x1 / 3x3 kernels, 2D maps and volumes
  kTileKG = 2,        // cfg 16 + id: two in-block K groups -- the register-weight tiles that fit two waves
                      // per SIMD (<= 256 VGPRs) with 512-thread blocks
  kTilePipe = 4,      // cfg 32 + id: pipelined staging (2D maps; a volume runs the plain tile)
  kTileUp2 = 8,       // 2x2 / 2x2x2 transposed-conv phases
  kTileS2 = 16,       // stride 2
  kTile2DOnly = 32,   // no volume instantiation
};

// A block owns BM couts x (TR rows x 32 px); WM of its 4 waves lie along the couts.  wreg: each wave
// keeps its weight fragments in registers one tap ahead (conv_halo_wreg_kernel); otherwise they go
// per tap through LDS (conv_halo_x3_kernel).
struct HaloTile {
  int id, BM, TR, WM;
  bool wreg;
  unsigned fam;
};
constexpr HaloTile kHaloTiles[] = {
    {0, 64, 8, 1, false, kTileS1},
    {1, 128, 4, 2, false, kTileS1},
    {2, 64, 8, 1, true, kTileS1 | kTilePipe | kTileUp2},
    {3, 128, 4, 2, true, kTileS1 | kTileKG | kTilePipe | kTileUp2},
    {4, 128, 2, 2, true, kTileS1 | kTileKG | kTilePipe | kTileS2},      // one pixel fragment per wave
    {5, 64, 4, 1, true, kTileS1 | kTileKG | kTilePipe | kTileUp2 | kTileS2},
    {6, 32, 8, 1, true, kTileS1 | kTilePipe | kTileUp2},
    {7, 32, 4, 1, true, kTileS1 | kTileKG | kTilePipe | kTileUp2 | kTileS2},
    {8, 128, 8, 2, true, kTileS1 | kTilePipe},
    {9, 256, 4, 4, true, kTileS1 | kTilePipe},
    {10, 64, 2, 2, true, kTileS2},                                     // 52 KB of LDS at stride 2
    {11, 256, 5, 4, true, kTileS1 | kTilePipe | kTile2DOnly},          // 5 rows: 24 row tiles at H = 120
};
constexpr int kNumHaloTiles = sizeof(kHaloTiles) / sizeof(kHaloTiles[0]);

// Pointwise tiles (conv_pw.hip): BM couts x PX pixels of the flattened plane, WM waves along the
// couts, an NS-deep LDS-DMA ring; coop: the block splits each chunk to fp16 once, not every wave.
// Deeper rings (6 / 8 chunks) measured 5-40 % slower on every 1x1 layer shape (tools/pw_bench.py).
struct PwTile { int id, BM, PX, WM, NS; bool coop; };
constexpr PwTile kPwTiles[] = {
    {24, 128, 128, 2, 3, false}, {25, 128, 64, 2, 4, false}, {26, 64, 128, 1, 3, false},
    {27, 256, 64, 4, 4, true},   {28, 128, 64, 2, 4, true},  {29, 128, 128, 2, 3, true},
};
constexpr int kNumPwTiles = sizeof(kPwTiles) / sizeof(kPwTiles[0]);
constexpr int kDepthTile = 30;     // depth-blocked (17, 1, 1) volume tile (conv_depth.hip)

template <class T, int N>
constexpr const T* find_tile(const T (&rows)[N], int id) {      // nullptr: no such tile
  for (const T& t : rows)
    if (t.id == id) return &t;
  return nullptr;
}
constexpr const HaloTile* halo_tile(int id) { return find_tile(kHaloTiles, id); }
constexpr const PwTile* pw_tile(int id) { return find_tile(kPwTiles, id); }
constexpr bool tile_in(int id, unsigned fam) { return halo_tile(id) && (halo_tile(id)->fam & fam) != 0; }

// the halo tiles of a family that a 2D map (d3 false) or a volume may take, for messages: "2, 3, 5"
inline std::string tile_ids(unsigned fam, bool d3 = false) {
  std::string s;
  for (const HaloTile& t : kHaloTiles)
    if ((t.fam & fam) && !(d3 && (t.fam & kTile2DOnly))) s += (s.empty() ? "" : ", ") + std::to_string(t.id);
  return s;
}

// cfg = (pipelined ? 32 : 0) + (K groups ? 16 : 0) + halo tile id, or 24..29 a pointwise tile, or 30
// the depth tile (-1: the entry point's policy).  `id`: the halo tile's, or the cfg itself of the others.
enum class TileKind { halo, pointwise, depth };
struct TileCfg { int id, kg; bool pipe; TileKind kind; };
constexpr TileCfg decode_cfg(int cfg) {
  const bool pipe = cfg >= 32;
  if (pipe) cfg -= 32;
  if (cfg == kDepthTile) return {cfg, 1, pipe, TileKind::depth};
  if (cfg >= kPwTiles[0].id) return {cfg, 1, pipe, TileKind::pointwise};    // one without a row is refused
  return cfg >= 16 ? TileCfg{cfg - 16, 2, pipe, TileKind::halo} : TileCfg{cfg, 1, pipe, TileKind::halo};
}
// also the index of fsmi_conv_launch_counts and the cfg of the clock tag
constexpr int encode_cfg(const TileCfg& t) { return (t.pipe ? 32 : 0) + (t.kg == 2 ? 16 : 0) + t.id; }

}  // namespace halo
}  // namespace fsmi
