"""Tile ids (``cfg``) a conv may take: the tests' own statement, written by hand, of what the tile table
csrc/conv_tiles.h (rows, family masks, ``decode_cfg``) and ``run_halo`` in csrc/conv_halo_x3.hip accept.
tests/test_tiles_host.py probes the C entry points against these lists on the CPU; a tile added to or retired
from the table is added or retired here by hand as well.

2D, stride 1: tile c (0..9, 11) = couts x (rows x 32 px); 16 + c the K-group variant of c in {3, 4, 5, 7};
32 + c the pipelined-staging variant of c in {2..9, 11}; 24..29 the pointwise LDS-DMA tiles (conv_pw.hip).

Volumes (NCDHW with D > 1 or KD > 1; 2D maps in safe range mode run the same instantiation), stride 1:
tiles 0..9 and the K-group variants 16 + c of c in {3, 4, 5, 7}, on every kernel (KD odd, KS in {1, 3}).
The 5-row tile 11 and the pointwise tiles are 2D only; 32 + c is accepted and runs the plain tile c.
Tile 30 is the depth-blocked kernel of csrc/conv_depth.hip and takes (17, 1, 1) convs only.  Stride-2
volume convs take tiles 4, 5, 7 and 10 (conv_halo_s2_3d.hip), the transposed-conv phase launches
(``fsmi_conv3d_up2_halo_x3`` / ``fsmi_conv2d_up2_halo_x3``) tiles 2, 3, 5, 6, 7.

Plain constants: the per-tile test matrices parametrise over them, and tests/test_gate_host.py /
tests/test_volume_host.py check that tuning/fsmi_conv.json selects nothing outside them.
"""

# -1: the C-side default policy (one of POLICY_DEFAULTS, by Cout / kernel size / Cin)
HALO_2D = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 19, 20, 21, 23, 34, 35, 36, 37, 38, 39, 40, 41, 43]
# 1x1 only, H*W % 4 == 0, 16-B aligned segments
PW_2D = [24, 25, 26, 27, 28, 29]
# what cfg < 0 resolves to
POLICY_DEFAULTS = [2, 3, 4, 5, 6]
# stride-1 volume tiles (-1: the policy; DEPTH_TILE for a (17, 1, 1) kernel, else one of POLICY_DEFAULTS)
VOLUME_3D = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 19, 20, 21, 23]
# (17, 1, 1) only
DEPTH_TILE = 30
# stride-2 tiles
S2_3D = [4, 5, 7, 10]
# transposed-conv phase tiles
UP2 = [2, 3, 5, 6, 7]
