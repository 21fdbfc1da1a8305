// 2x2 tiles of the halo conv on 2D maps: the four output phases of a ConvTranspose2d(k=4, s=2, p=1)
// (fsmi_conv2d_up2_halo_x3; spx_2_gru.conv1 and spx_gru, core/foundation_stereo.py:183-191).
// The register-weight tiles of family kTileUp2 (conv_tiles.h); no K groups.
#include "conv_halo.h"

FSMI_HALO_LAUNCH_CFG(2, false)
