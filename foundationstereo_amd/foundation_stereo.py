"""FoundationStereo forward with the MI355X-native hot path (``core/foundation_stereo.py``).

Module tree and ``state_dict`` keys are the reference's (checkpoints load
unchanged; ``feature.*`` belongs to the out-of-scope backbone).  What changes
is the data path:

* a1+a2: gwc + concat + the 1x1x1 ``corr_stem[0]`` conv are ONE kernel
  (``ops.comb_volume_stem``) writing the 28-channel stem volume directly --
  the 32-channel comb volume and its cat copy never exist in HBM;
* a3: 3D filtering: every stride-1 Conv3d + BN block on the halo split-precision kernel
  (``ops.conv3d``), the classifier head on ``ops.conv3d_direct``, the disparity transformer
  on ``ops.disparity_transformer``, the stride-2 convs and ConvTranspose3d on the halo
  kernel's stride-2 / phase tiles, FeatureAtt folded into the producing conv's epilogue;
* a4: softmax + soft-argmin fused (``ops.softmax_regression``); skipped when an
  ``init_disp`` is supplied (hierarchical pass) since the reference discards it;
* a5/a6: geometry encoding + per-iteration lookup on HIP (``geometry.py``);
* a7: ConvGRU with fused gates (``update.py``);
* a9: softmax(9) + convex x4 upsampling fused (``ops.softmax_context_upsample``).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, streams
from . import submodule as _sub
from . import update as _update
from .backbone import Feature
from .extractor import ContextNetDino, SyntheticFeature
from .geometry import Combined_Geo_Encoding_Volume
from .submodule import (BasicConv, BasicConv_IN, ChannelAttentionEnhancement, Conv2x, Conv3dNormActReduced,
                        CostVolumeDisparityAttention, FeatureAtt, ResnetBasicBlock3D, SpatialAttentionExtractor,
                        build_concat_volume, build_gwc_volume)
from .update import BasicSelectiveMultiUpdateBlock
from .utils import InputPadder

_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


def autocast(enabled, dtype="float16"):
    """``torch.cuda.amp.autocast(enabled)`` of the reference (fp16); ``mixed_dtype`` may select bf16."""
    return torch.autocast("cuda", dtype=getattr(torch, dtype), enabled=bool(enabled))


def normalize_image(img):
    """(x/255 - mean)/std per RGB channel (core/foundation_stereo.py:37-42)."""
    key = (img.device, img.dtype)
    if key not in _NORM_CACHE:     # device constants made once (an H2D copy cannot be graph-captured)
        _NORM_CACHE[key] = (torch.tensor(_MEAN, device=img.device, dtype=img.dtype).view(1, 3, 1, 1),
                            torch.tensor(_STD, device=img.device, dtype=img.dtype).view(1, 3, 1, 1))
    mean, std = _NORM_CACHE[key]
    return ((img / 255.0 - mean) / std).contiguous()


_NORM_CACHE = {}


# The one switch of this file: the range guard of the split-precision convs, enforced per eager forward
# (see forward); FSMI_RANGE_GUARD=0, or a caller that checks ops.check_range() itself and sets the
# attribute, leaves the flag to the caller.  update.OVERLAP (bench.py) also decides whether the context
# net (+ stem_2, CAM / SAM), the FeatureAtt gates and the hourglass's disparity-transformer branch run on
# side streams beside the 3D path; they fork and join through streams.py (fork / join), which names the
# streams and checks every wait under capture (capture_fork).
RANGE_GUARD = os.environ.get("FSMI_RANGE_GUARD", "1") != "0"


def _gated(seq, x, gate):
    """seq(x) * sigmoid(gate) broadcast over depth, the gate applied by seq's last block
    (a Conv3dNormActReduced: its second conv's epilogue)."""
    for m in list(seq)[:-1]:
        x = m(x)
    return seq[-1](x, fatt=gate)


class hourglass(nn.Module):
    """3-level 3D hourglass with feature attention and the disparity transformer
    (core/foundation_stereo.py:45-123)."""

    def __init__(self, cfg, in_channels, feat_dims=None):
        super().__init__()
        self.cfg = cfg
        c = in_channels

        def down(ci, co):
            return nn.Sequential(BasicConv(ci, co, is_3d=True, bn=True, relu=True, kernel_size=3, padding=1, stride=2,
                                           dilation=1),
                                 Conv3dNormActReduced(co, co, kernel_size=3, kernel_disp=17))

        def up(ci, co):
            return BasicConv(ci, co, deconv=True, is_3d=True, bn=True, relu=True, kernel_size=(4, 4, 4),
                             padding=(1, 1, 1), stride=(2, 2, 2))

        def agg(ci, co):
            return nn.Sequential(BasicConv(ci, co, is_3d=True, kernel_size=1, padding=0, stride=1),
                                 Conv3dNormActReduced(co, co, kernel_size=3, kernel_disp=17),
                                 Conv3dNormActReduced(co, co, kernel_size=3, kernel_disp=17))

        self.conv1 = down(c, 2 * c)
        self.conv2 = down(2 * c, 4 * c)
        self.conv3 = down(4 * c, 6 * c)
        self.conv3_up = up(6 * c, 4 * c)
        self.conv2_up = up(4 * c, 2 * c)
        self.conv1_up = up(2 * c, c)
        self.conv_out = nn.Sequential(Conv3dNormActReduced(c, c, kernel_size=3, kernel_disp=17),
                                      Conv3dNormActReduced(c, c, kernel_size=3, kernel_disp=17))
        self.agg_0 = agg(8 * c, 4 * c)
        self.agg_1 = agg(4 * c, 2 * c)
        self.atts = nn.ModuleDict({"4": CostVolumeDisparityAttention(d_model=c, nhead=4, dim_feedforward=c,
                                                                     norm_first=False, num_transformer=4,
                                                                     max_len=self.cfg["max_disp"] // 16)})
        self.conv_patch = nn.Sequential(nn.Conv3d(c, c, kernel_size=4, stride=4, padding=0, groups=c),
                                        nn.BatchNorm3d(c))
        self.feature_att_8 = FeatureAtt(2 * c, feat_dims[1])
        self.feature_att_16 = FeatureAtt(4 * c, feat_dims[2])
        self.feature_att_32 = FeatureAtt(6 * c, feat_dims[3])
        self.feature_att_up_16 = FeatureAtt(4 * c, feat_dims[2])
        self.feature_att_up_8 = FeatureAtt(2 * c, feat_dims[1])

    def gate_logits(self, features):
        """The five FeatureAtt gates (pre-sigmoid), in the order forward uses them."""
        return (self.feature_att_8.logits(features[1]), self.feature_att_16.logits(features[2]),
                self.feature_att_32.logits(features[3]), self.feature_att_up_16.logits(features[2]),
                self.feature_att_up_8.logits(features[1]))

    def forward(self, x, features, gates=None):
        """``gates``: precomputed ``gate_logits(features)`` (ready on the current stream)."""
        # patch embed, transformer and the x4 trilinear add on HIP (csrc/transformer.hip), decided here, before
        # the fork: the add needs conv1_up(c1) in x's shape, which it has whenever x's axes are even (a
        # stride-2 conv leaves ceil(n / 2), the deconv doubles that) -- and _dt_fast takes multiples of 4 only
        dt_fast = self._dt_fast(x)
        if dt_fast:
            # the disparity transformer branch (patch embed + 4 encoder layers, ~0.45 ms at cfg2, a few
            # hundred waves) reads only x: it runs on a side stream beside conv1 .. conv1_up, or with
            # update.OVERLAP off on the calling stream, in order
            main = streams.current(x.device)
            dt_s = streams.side(x.device, streams.BRANCH) if _update.OVERLAP else main
            with streams.fork(dt_s, main):
                scale, shift = self._patch_fold()
                t = self.atts["4"](ops.dt_patch_embed(_sub._f32(x), self.conv_patch[0].weight.float(), scale, shift))
        if _sub.FATT_FUSE and not self.training:
            # each FeatureAtt's sigmoid(gate) * cv in the epilogue of the conv that produces cv
            # (core/foundation_stereo.py:93-109, core/submodule.py:452-453)
            g8, g16, g32, gu16, gu8 = gates if gates is not None else self.gate_logits(features)
            c1 = _gated(self.conv1, x, g8)
            c2 = _gated(self.conv2, c1, g16)
            c3 = _gated(self.conv3, c2, g32)
            c2 = _gated(self.agg_0, torch.cat((self.conv3_up(c3), c2), dim=1), gu16)
            c1 = _gated(self.agg_1, torch.cat((self.conv2_up(c2), c1), dim=1), gu8)
        else:
            c1 = self.feature_att_8(self.conv1(x), features[1])
            c2 = self.feature_att_16(self.conv2(c1), features[2])
            c3 = self.feature_att_32(self.conv3(c2), features[3])
            c2 = self.feature_att_up_16(self.agg_0(torch.cat((self.conv3_up(c3), c2), dim=1)), features[2])
            c1 = self.feature_att_up_8(self.agg_1(torch.cat((self.conv2_up(c2), c1), dim=1)), features[1])
        conv = self.conv1_up(c1)
        if dt_fast:
            streams.join(main, dt_s, t)
            return self.conv_out(ops.upsample4_add_(conv.float().contiguous(), t))
        t = self.atts["4"](self.conv_patch(x))
        conv = conv + F.interpolate(t, scale_factor=4, mode="trilinear", align_corners=False)
        return self.conv_out(conv)

    def _dt_fast(self, x) -> bool:
        pc, bn = self.conv_patch[0], self.conv_patch[1]
        return (_sub._hip(x) and not self.training and _sub.DT_FAST
                and pc.groups == pc.in_channels == pc.out_channels and pc.kernel_size == (4, 4, 4)
                and pc.stride == (4, 4, 4) and pc.padding == (0, 0, 0) and bn.track_running_stats
                and all(n % 4 == 0 for n in x.shape[2:]))

    def _patch_fold(self):
        """conv_patch bias + eval BatchNorm3d as per-channel (scale, shift), cached per version."""
        pc, bn = self.conv_patch[0], self.conv_patch[1]

        def build():
            inv = (bn.running_var.double() + bn.eps).rsqrt() * (bn.weight.double() if bn.weight is not None else 1)
            b = pc.bias.double() if pc.bias is not None else torch.zeros_like(inv)
            shift = (b - bn.running_mean.double()) * inv + (bn.bias.double() if bn.bias is not None else 0)
            return inv.float().contiguous(), shift.float().contiguous()

        return _sub._cached(self, "_fsmi_patch", [pc.weight, pc.bias, bn.weight, bn.bias, bn.running_mean,
                                                  bn.running_var], build)


def _poison_outputs(out):
    """ops.range_poison_ on every tensor of a captured forward's result (a tensor, or the
    (init_disp, disp_preds) pair of training mode); a non-contiguous one is replaced by a contiguous
    copy first, so the poison reaches every element the caller reads."""
    if isinstance(out, torch.Tensor):
        if not out.is_floating_point():
            return out
        if not out.is_contiguous():
            out = out.contiguous()
        return ops.range_poison_(out)
    if isinstance(out, (list, tuple)):
        return type(out)(_poison_outputs(o) for o in out)
    return out


class FoundationStereo(nn.Module):
    """core/foundation_stereo.py:127-274.  ``feature``: the backbone module (default: ``Feature`` when
    ``args.backbone == "real"``, else the synthetic stand-in whose features are preset in HBM)."""

    def __init__(self, args, feature=None):
        super().__init__()
        self.args = args
        context_dims = args.hidden_dims
        self.cv_group = 8
        volume_dim = 28
        self.cnet = ContextNetDino(args, output_dim=[args.hidden_dims, context_dims], downsample=args.n_downsample)
        self.update_block = BasicSelectiveMultiUpdateBlock(self.args, self.args.hidden_dims[0], volume_dim=volume_dim)
        self.sam = SpatialAttentionExtractor()
        self.cam = ChannelAttentionEnhancement(self.args.hidden_dims[0])
        self.context_zqr_convs = nn.ModuleList([nn.Conv2d(context_dims[i], args.hidden_dims[i] * 3, kernel_size=3,
                                                          padding=1) for i in range(self.args.n_gru_layers)])
        if feature is None:
            # the reference always builds the real backbone (core/foundation_stereo.py:143); here
            # args.backbone == "real" does (Feature, EdgeNeXt-S + DepthAnythingV2 on the HIP engine), the
            # default keeps the seeded synthetic stand-in of the north-star benchmark (backbone excluded)
            feature = Feature(args) if args.get("backbone", "synthetic") == "real" else SyntheticFeature(args)
        self.feature = feature
        self.proj_cmb = nn.Conv2d(self.feature.d_out[0], 12, kernel_size=1, padding=0)
        self.stem_2 = nn.Sequential(BasicConv_IN(3, 32, kernel_size=3, stride=2, padding=1),
                                    nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.InstanceNorm2d(32), nn.ReLU())
        self.stem_4 = nn.Sequential(BasicConv_IN(32, 48, kernel_size=3, stride=2, padding=1),
                                    nn.Conv2d(48, 48, 3, 1, 1, bias=False), nn.InstanceNorm2d(48), nn.ReLU())
        self.spx_2_gru = Conv2x(32, 32, True, bn=False)
        self.spx_gru = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
        self.corr_stem = nn.Sequential(
            nn.Conv3d(32, volume_dim, kernel_size=1),
            BasicConv(volume_dim, volume_dim, kernel_size=3, padding=1, is_3d=True),
            ResnetBasicBlock3D(volume_dim, volume_dim, kernel_size=3, stride=1, padding=1),
            ResnetBasicBlock3D(volume_dim, volume_dim, kernel_size=3, stride=1, padding=1))
        self.corr_feature_att = FeatureAtt(volume_dim, self.feature.d_out[0])
        self.cost_agg = hourglass(cfg=self.args, in_channels=volume_dim, feat_dims=self.feature.d_out)
        self.classifier = nn.Sequential(
            BasicConv(volume_dim, volume_dim // 2, kernel_size=3, padding=1, is_3d=True),
            ResnetBasicBlock3D(volume_dim // 2, volume_dim // 2, kernel_size=3, stride=1, padding=1),
            nn.Conv3d(volume_dim // 2, 1, kernel_size=7, padding=3))
        r = self.args.corr_radius
        self.dx = torch.linspace(-r, r, 2 * r + 1, requires_grad=False).reshape(1, 1, 2 * r + 1, 1)
        self.fused_volume = True
        # plain attributes (no buffers: state_dict is the reference's).  keep_logits: the forward leaves the
        # classifier's fp32 logits (B, max_disp / 4, H / 4, W / 4) in last_logits for ``confidence``
        self.keep_logits = False
        self.last_logits = None

    # ------------------------------------------------------------ volume build
    def _stem_weights(self):
        """Fold proj_cmb into the concat columns of corr_stem[0] (exact algebra, fp64)."""
        stem, proj = self.corr_stem[0], self.proj_cmb

        def build():
            S = stem.weight.reshape(stem.weight.shape[0], -1).double()       # (Cs, 32)
            sb = stem.bias.double()
            P = proj.weight.reshape(proj.weight.shape[0], -1).double()        # (12, C)
            pb = proj.bias.double()
            G = self.cv_group
            Sl, Sr = S[:, G:G + 12], S[:, G + 12:G + 24]
            wa, ba = Sl @ P, Sl @ pb + sb
            wb, bb = Sr @ P, Sr @ pb
            return [t.float().contiguous() for t in (S[:, :G], wa, ba, wb, bb)]

        return _sub._cached(self, "_fsmi_stem", [stem.weight, stem.bias, proj.weight, proj.bias], build)

    def build_stem_volume(self, fl0, fr0):
        """gwc + concat + corr_stem[0] -> (B, 28, D4, H4, W4) (core/foundation_stereo.py:207-213)."""
        D4 = self.args["max_disp"] // 4
        fl0, fr0 = fl0.float(), fr0.float()
        if not self.fused_volume:
            gwc = build_gwc_volume(fl0, fr0, D4, self.cv_group)
            cat = build_concat_volume(self.proj_cmb(fl0), self.proj_cmb(fr0), D4)
            return self.corr_stem[0](torch.cat([gwc, cat], dim=1))
        wg, wa, ba, wb, bb = self._stem_weights()
        A = ops.pointwise_proj(fl0, wa, ba)
        Bm = ops.pointwise_proj(fr0, wb, bb)
        return ops.comb_volume_stem(fl0, fr0, A, Bm, wg, D4)

    def _backbone(self, image1, image2):
        B = len(image1)
        out, vit_feat = self.feature(torch.cat([image1, image2], dim=0))
        return [o[:B] for o in out], [o[B:] for o in out], vit_feat[:B]

    def _context(self, image1, vit_feat):
        """stem_2 and the context features (core/foundation_stereo.py:207,221-226)."""
        stem_2x = _sub.run_seq(self.stem_2, image1)      # BasicConv_IN s2 + conv3x3 + IN + ReLU
        cnet_list = self.cnet(image1, vit_feat=vit_feat, num_layers=self.args.n_gru_layers)
        net_list = [torch.tanh(x[0]) for x in cnet_list]
        inp_list = [torch.relu(x[1]) for x in cnet_list]
        inp_list = [self.cam(x) * x for x in inp_list]
        att = [self.sam(x) for x in inp_list]
        return stem_2x, net_list, inp_list, att

    def upsample_disp(self, disp, mask_feat_4, stem_2x):
        """core/foundation_stereo.py:183-191: returns (B,1,H,W) fp32."""
        with autocast(self.args.mixed_precision, self.args.get("mixed_dtype", "float16")):
            xspx = self.spx_2_gru(mask_feat_4, stem_2x)
            spx = self.spx_gru[0]
            if len(self.spx_gru) == 1 and _sub.fast_up2d(xspx, spx):
                logits = _sub.deconv2d_bn_act(xspx, spx)      # ConvTranspose2d(64, 9, 4, 2, 1) + bias on HIP
            else:
                logits = self.spx_gru(xspx)
        return ops.softmax_context_upsample(disp.float(), logits.float(), 4.0).unsqueeze(1)

    def forward(self, image1, image2, iters=12, flow_init=None, test_mode=False, low_memory=False, init_disp=None):
        """core/foundation_stereo.py:194-254.  On a HIP device outside graph capture the range guard
        of the split-precision convs is enforced here, once per forward: the flag is read after the
        forward and a forward that overflowed is re-run in safe range mode (ops.guarded) -- no
        disparity computed past the flag is returned.  That read synchronises the host with the
        device once per eager forward; a caller that checks ``ops.check_range()`` itself can set
        ``foundation_stereo.RANGE_GUARD = False`` to skip it.  A captured forward ends with a
        device-side check instead: every returned disparity tensor (test mode's one, or
        ``init_disp`` and each of ``disp_preds``) is NaN-filled when the flag is set
        (ops.range_poison_).

        With ``self.keep_logits`` set, the classifier's fp32 logits of this forward stay in
        ``self.last_logits`` (``confidence.from_model``); the classifier then also runs when ``init_disp``
        is given, which stays the disparity the refinement starts from.  Under capture the tensor is
        graph-static memory, valid until the next replay, and is range-poisoned along with the outputs.
        With the flag off (the default) nothing is kept and nothing extra runs."""
        def run():
            return self._forward(image1, image2, iters, flow_init, test_mode, low_memory, init_disp)
        if not (image1.is_cuda and RANGE_GUARD):
            return run()
        if streams.capturing():
            # a captured forward cannot synchronise: its last node NaN-fills the disparity when the
            # flag is set, so a replay that overflowed never returns a finite result (ShardedStereo
            # reads the flag after a replay and recovers)
            out = _poison_outputs(run())
            if self.keep_logits and self.last_logits is not None:
                self.last_logits = _poison_outputs(self.last_logits)
            return out
        return ops.guarded(run)

    def _forward(self, image1, image2, iters=12, flow_init=None, test_mode=False, low_memory=False, init_disp=None):
        B = len(image1)
        if not self.keep_logits:
            self.last_logits = None        # nothing is kept with the flag off, an earlier forward's logits included
        image1 = normalize_image(image1)
        image2 = normalize_image(image2)
        mp = self.args.mixed_precision
        md = self.args.get("mixed_dtype", "float16")
        with autocast(mp, md):
            features_left, features_right, vit_feat = self._backbone(image1, image2)
            # the two HBM / MFMA kernels the north star measures run ALONE on the chip, before any
            # side stream forks: the cost-volume build, then the all-pairs correlation pyramid (it
            # needs only the features; the side streams' convs used to stretch it 10x beside the
            # classifier).  ~70 us on the main stream; the side streams are far off the critical path.
            # With grad enabled the geometry volume builds the pyramid itself, as it always has.
            vol = self.build_stem_volume(features_left[0], features_right[0])
            hip = image1.is_cuda and not torch.is_grad_enabled()
            corr_pyr = Combined_Geo_Encoding_Volume.corr_pyramid(
                features_left[0].float(), features_right[0].float(), self.args.corr_levels) if hip else None
            # the side streams of what follows, or the main stream itself (streams.fork / join then run it
            # in order): the context on the motion stream, the gates on the branch stream
            ctx_overlap = _update.OVERLAP and hip
            main = streams.current(image1.device)
            ctx_s = streams.side(image1.device, streams.MOTION) if ctx_overlap else main
            g_s = streams.side(image1.device, streams.BRANCH) if ctx_overlap else main
            # stem_2 + context net + CAM / SAM read only the images and vit_feat: beside the 3D filtering,
            # joined before the loop.  ctx_pre also where only update_block.forward will run, which does
            # not take it
            with streams.fork(ctx_s, main):
                stem_2x, net_list, inp_list, att = self._context(image1, vit_feat)
                ctx_pre = self.update_block.context_pre(inp_list)
            if _sub.FATT_FUSE and not self.training:
                # the six FeatureAtt gates (2D 1x1 convs on the features), ready long before the volume
                # convs that apply them; an event joins only them
                with streams.fork(g_s, main):
                    gates = (self.corr_feature_att.logits(features_left[0]),) + \
                        self.cost_agg.gate_logits(features_left)
                    g_ev = streams.record(g_s)
                # corr_feature_att's sigmoid(gate) * vol in the last ResNet block's epilogue; the gates
                # are joined right before it (~1 ms of volume convs after the fork)
                for m in list(self.corr_stem)[1:-1]:
                    vol = m(vol)
                streams.join(main, g_s, *gates, event=g_ev)
                vol = self.corr_stem[-1](vol, fatt=gates[0])
                vol = self.cost_agg(vol, features_left, gates=gates[1:])
            else:
                vol = self.corr_feature_att(self.corr_stem[1:](vol), features_left[0])
                vol = self.cost_agg(vol, features_left)
            # the volume pyramid (HBM-bound) on the main stream right after the hourglass, before the
            # classifier's convs start: the gate and disparity-transformer branches joined inside the
            # hourglass and the context stream (~1/10 of the hourglass's work) has long finished
            geo_fn = Combined_Geo_Encoding_Volume(features_left[0].float(), features_right[0].float(), vol.float(),
                                                  num_levels=self.args.corr_levels, dx=self.dx,
                                                  init_corr_pyramid=corr_pyr)
            if init_disp is None or self.keep_logits:
                cl = self.classifier
                head = cl[2]   # Conv3d(14, 1, 7, padding=3): direct gfx950 kernel (MIOpen: ~1 TFLOP/s here)
                logits = ops.conv3d_direct(cl[1](cl[0](vol)).float(), head.weight.float(),
                                           head.bias.float()).squeeze(1)
                if self.keep_logits:
                    self.last_logits = logits
                if init_disp is None:      # a given one stays (run_hierachical's second pass)
                    init_disp = ops.softmax_regression(logits)
            streams.join(main, ctx_s, stem_2x, *net_list, *inp_list, *att, *(ctx_pre or ()))

        disp = init_disp.float()
        disp_preds = []
        disp_up = None
        overlap = _update.OVERLAP and _update._fast(disp)
        if overlap:     # fp32 state for the HIP loop (fp16 / bf16 context features under autocast)
            net_list, inp_list, att = _update._f32s(net_list), _update._f32s(inp_list), _update._f32s(att)
        if overlap and test_mode and self.args.n_gru_layers == 3 and iters > 0:
            # gru16 / gru08 one iteration ahead on their own stream (same math, see run_pipelined)
            net_list, mask_feat_4, disp = self.update_block.run_pipelined(net_list, inp_list, geo_fn,
                                                                          disp.detach(), att, iters, pre=ctx_pre)
            return self.upsample_disp(disp, mask_feat_4, stem_2x)
        for itr in range(iters):
            disp = disp.detach()
            if overlap:    # lookup + motion encoder on a side stream beside gru16/gru08 (same math)
                net_list, mask_feat_4, delta_disp = self.update_block.forward_overlapped(
                    net_list, inp_list, geo_fn, disp, att, pre=ctx_pre)
            else:
                geo_feat = geo_fn(disp)
                with autocast(mp, md):
                    net_list, mask_feat_4, delta_disp = self.update_block(net_list, inp_list, geo_feat, disp, att)
            disp = disp + delta_disp.float()
            if test_mode and itr < iters - 1:
                continue
            disp_up = self.upsample_disp(disp, mask_feat_4, stem_2x)
            disp_preds.append(disp_up)
        if test_mode:
            return disp_up
        return init_disp, disp_preds

    def run_hierachical(self, image1, image2, iters=12, test_mode=False, low_memory=False, small_ratio=0.5):
        """Coarse-to-fine driver (core/foundation_stereo.py:257-274), including the
        reference's ``+= padder._pad[0]`` on the upsampled init."""
        B, _, H, W = image1.shape
        img1_small = F.interpolate(image1, scale_factor=small_ratio, align_corners=False, mode="bilinear")
        img2_small = F.interpolate(image2, scale_factor=small_ratio, align_corners=False, mode="bilinear")
        padder = InputPadder(img1_small.shape[-2:], divis_by=32, force_square=False)
        img1_small, img2_small = padder.pad(img1_small, img2_small)
        disp_small = self.forward(img1_small, img2_small, test_mode=True, iters=iters, low_memory=low_memory)
        disp_small = padder.unpad(disp_small.float())
        disp_small_up = F.interpolate(disp_small, size=(H, W), mode="bilinear", align_corners=True) * 1 / small_ratio
        disp_small_up = disp_small_up.clip(0, None)
        padder = InputPadder(image1.shape[-2:], divis_by=32, force_square=False)
        image1, image2, disp_small_up = padder.pad(image1, image2, disp_small_up)
        disp_small_up += padder._pad[0]
        init_disp = F.interpolate(disp_small_up, scale_factor=0.25, mode="bilinear", align_corners=True) * 0.25
        disp = self.forward(image1, image2, iters=iters, test_mode=test_mode, low_memory=low_memory,
                            init_disp=init_disp)
        return padder.unpad(disp.float())
