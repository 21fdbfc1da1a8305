// Stride-2 tiles of the halo conv (fsmi_conv3d_halo_x3_ex, stride 2): the hourglass's
// BasicConv3d(k=3, s=2, p=1) (core/foundation_stereo.py:50-58) with KS = KD = 3, and -- as volumes of
// depth 1 -- the context net's 3x3 s2 p1 convs and 1x1 s2 projections (core/extractor.py:20-80).
// The register-weight tiles of family kTileS2 (conv_tiles.h), no K groups.  The staged window of a
// TR x 32 output tile is (2 TR + KS - 2) x (63 + KS - 1) input pixels: for KS = 3, 52 KB of LDS at
// TR = 2 (three blocks per CU), 94 KB at TR = 4 (one).
#include "conv_halo.h"

namespace fsmi {
namespace halo {

int launch_s2(int ks, int id, const HaloArgs& a, hipStream_t s) {
  return ks == 1 ? launch_family<1, true, 1, 2, kTileS2>(id, a, s) : launch_family<3, true, 1, 2, kTileS2>(id, a, s);
}

}  // namespace halo
}  // namespace fsmi
