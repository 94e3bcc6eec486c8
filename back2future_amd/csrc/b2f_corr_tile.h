// Tile geometry and sampling record of the block-per-tile warp + cost-volume kernels: what b2f_corr.hip (variants 0 - 3) shares with
// the experiment kernels built from the same pieces (variants 4 and 8, tools/experiments/csrc/b2f_corr_exp.hip).
#pragma once

namespace b2f {

namespace {
constexpr int TH = 8, TW = 16, R = 4;
constexpr int HH = TH + 2 * R;      // 16 halo rows
constexpr int HWD = TW + 2 * R;     // 24 halo cols
constexpr int HP = 32;              // LDS row pitch in pixels (multiple of 16 -> conflict-free b128)
constexpr int NHALO = HH * HWD;     // 384

// Bilinear sampling record of one halo pixel of one neighbour map: the four blend
// weights (all 0 for a halo pixel outside the image: CostVolMulti's out-of-range -> 0) and
// the top-left pixel index with the offsets of the right / bottom neighbours.  A neighbour
// outside the image has weight exactly 0 (coordinates are clamped first), so its address is
// folded onto the clamped pixel instead of branching around the load.
struct SampIdx {
    int idx;           // top-left pixel index (y*w + x)
    int flags;         // bit0: right neighbour is x+1 (else folded onto x), bit1: bottom is y+1
};
}  // namespace

// the two-pixel kernels' 16 x 16 tile (see warp_costvol_2px_kernel)
namespace v2 {
constexpr int TH2 = 16, TW2 = 16;
constexpr int HH2 = TH2 + 2 * R, HW2 = TW2 + 2 * R;   // 24 x 24 halo
constexpr int HP2 = 32;                              // LDS row pitch in pixels
constexpr int NH2 = HH2 * HW2;                       // 576 halo pixels per map
constexpr int PL2 = HH2 * HP2 + 4;                   // float4 per (map, k4) plane: 772 = 4 (mod 8), so that the lane pair
                                                     // (pixel, k4 = 0 | 1) of the gather writes distinct LDS banks
}  // namespace v2

}  // namespace b2f
