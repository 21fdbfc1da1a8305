// 2x2x2 volume tiles of the halo conv: the eight output phases of a ConvTranspose3d(k=4, s=2, p=1)
// (fsmi_conv3d_up2_halo_x3).  The register-weight tiles of family kTileUp2 (conv_tiles.h); no K groups.
#include "conv_halo.h"

FSMI_HALO_LAUNCH_CFG(2, true)
