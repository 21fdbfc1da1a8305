"""Tile ids (``cfg``) a stride-1 2D conv may take, read off ``run_halo`` in csrc/conv_halo_x3.hip.

tile c (0..9, 11) = couts x (rows x 32 px); 16 + c the K-group variant of c in {3, 4, 5, 7}; 32 + c the
pipelined-staging variant of c in {2..9, 11}; 24..29 the pointwise LDS-DMA tiles (conv_pw.hip).  Plain
constants: the per-tile test matrices parametrise over them, and tests/test_gate_host.py checks that
tuning/fsmi_conv.json selects nothing outside them.
"""

# -1: the C-side default policy (one of POLICY_DEFAULTS, by Cout / kernel size / Cin)
HALO_2D = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 19, 20, 21, 23, 34, 35, 36, 37, 38, 39, 40, 41, 43]
# 1x1 only, H*W % 4 == 0, 16-B aligned segments
PW_2D = [24, 25, 26, 27, 28, 29]
# what cfg < 0 resolves to
POLICY_DEFAULTS = [2, 3, 4, 5, 6]
