"""Drop-in for ``core/update.py``: the selective ConvGRU refinement block.

Every 1x1 / 3x3 convolution of the loop (motion encoder, SelectiveConvGRU,
DispHead incl. the EdgeNeXt MLPs, mask head) runs on the halo-tiled
split-precision MFMA kernel (``ops.conv2d``, ``fsmi_conv2d_halo_x3``) with
the reference's cats done as zero-copy input segments and bias / ReLU / GELU /
layer-scale / residual / 0.25-scale fused into the epilogue.  Weights are
packed once per (module, weight version).  The gates between the convs --
sigmoid of z/r, ``r*h``, ``cat([r*h, x])``, ``tanh``, ``(1-z)h + zq`` and the
``small*att + large*(1-att)`` selection -- run in the epilogues of the gate convs
(``ops.conv2d_gate``); ``convz`` and ``convr`` run as ONE conv with stacked
weights.  ``RaftConvGRU`` on its own and the torch path keep the two gate kernels
``ops.gru_reset`` / ``ops.gru_blend``.  The two 7x7 convs run on their
own kernels: ``convd1`` (1 -> 64, + ReLU) on ``ops.conv2d_1in``, the depthwise
``dwconv`` on ``ops.dwconv2d``; ``pool2x`` is ``ops.pool2x`` and ``interp``
``ops.resize_bilinear``.  Under the reference's autocast the same HIP path runs
(fp16 inputs cast up, fp32 compute); with grad enabled the module runs the plain
torch path (``CONV_ENGINE = "miopen"`` forces it: bench.py's ``--conv-engine``).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, streams
from .submodule import EdgeNextConvEncoder, _cached, _f32, _hip

# What still switches a path here, and who uses it:
#   CONV_ENGINE     "miopen" forces the torch path (bench.py --conv-engine)
#   OVERLAP         side streams for the motion path, the GRU small branches, the mask head and the gru16 /
#                   gru08 pipeline (FSMI_OVERLAP; bench.py).  The streams, and every fork / join / wait
#                   between them, are streams.py's.  No knob here picks between two copies of a sequence:
#                   each schedule is written once, forked, and a knob only picks the stream a fork goes to --
#                   the slot's side stream, or the calling stream itself, on which streams.fork / join do
#                   nothing and the same sequence runs in order.  Whether a SelectiveConvGRU forks its small
#                   branch is its caller's ``fork_small`` argument
#   PIPE_BRANCH     run_pipelined: gru04's small branch on its own stream, i.e. its ``fork_small``
#                   (FSMI_PIPE_BRANCH; tests/test_gpu_capture_fork.py)
#   MOTION_ON_MAIN  run_pipelined: the motion path (lookup + encoder) forks to the main stream, i.e. stays on
#                   it, instead of the motion stream (FSMI_MOTION_ON_MAIN; tests/test_gpu_capture_fork.py)
#   CTX_PRE         SelectiveConvGRU.conv0's context segment convolved once per forward (context_pre);
#                   False: every iteration (tests/test_gpu_ctx_pre.py, test_gpu_range.py set the attribute)
#   COUT1           DispHead's last conv (128 -> 1) on its own fp32 kernel (ops.conv3x3_cout1); False: the
#                   halo conv tile (tests/test_gpu_ctx_pre.py sets the attribute)
CONV_ENGINE = "fsmi"
OVERLAP = os.environ.get("FSMI_OVERLAP", "1") != "0"
PIPE_BRANCH = os.environ.get("FSMI_PIPE_BRANCH", "1") != "0"
MOTION_ON_MAIN = os.environ.get("FSMI_MOTION_ON_MAIN", "0") != "0"
CTX_PRE = True
COUT1 = True


def _fast(x) -> bool:
    """The HIP path applies: ROCm tensor, no grad.  Under the reference's autocast
    (scripts/run_demo.py:161) fp16 / bf16 inputs are cast up and the loop still runs on the HIP
    kernels in fp32."""
    return CONV_ENGINE == "fsmi" and _hip(x)


def _f32s(xs):
    return [_f32(x) for x in xs]


def _packed(*mods, cin_order=None):
    """Halo-kernel weights of one Conv2d/Linear (or several stacked along Cout),
    cached on the first module and rebuilt when any weight/bias changes.  ``cin_order``: input
    channels packed in this order (the caller passes its segments in the same order); a subset of
    the input channels packs the conv restricted to them (one cache slot per order)."""
    def build():
        ws = [m.weight if m.weight.dim() == 4 else m.weight[:, :, None, None] for m in mods]
        if cin_order is not None:
            # runs of consecutive channels as slices: no index tensor to upload (a pack first built
            # under a stream capture must not copy from the host)
            runs = []
            for c in cin_order:
                if runs and c == runs[-1][1]:
                    runs[-1][1] = c + 1
                else:
                    runs.append([c, c + 1])
            ws = [torch.cat([w[:, a:b] for a, b in runs], 1) for w in ws]
        pk = ops.PackedConv(*ws, mode="halo")
        bias = torch.cat([m.bias.detach().float() for m in mods]).contiguous()
        return pk, bias

    slot = "_fsmi_pack" if cin_order is None else f"_fsmi_pack_{tuple(cin_order)}"
    return _cached(mods[0], slot, [t for m in mods for t in (m.weight, m.bias)], build)


def _conv(mods, segs, act=None, **kw):
    mods = mods if isinstance(mods, tuple) else (mods,)
    pk, bias = _packed(*mods)
    return ops.conv2d(segs, pk, bias=bias, act=act, **kw)


__all__ = ["DispHead", "ConvGRU", "BasicMotionEncoder", "pool2x", "pool4x", "interp", "RaftConvGRU",
           "SelectiveConvGRU", "BasicSelectiveMultiUpdateBlock"]


class DispHead(nn.Module):
    """core/update.py:20-32."""

    def __init__(self, input_dim=128, hidden_dim=256, output_dim=1):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(input_dim, input_dim, kernel_size=3, padding=1), nn.ReLU(),
            EdgeNextConvEncoder(input_dim, expan_ratio=4, kernel_size=7, norm=None),
            EdgeNextConvEncoder(input_dim, expan_ratio=4, kernel_size=7, norm=None),
            nn.Conv2d(input_dim, output_dim, 3, padding=1))

    def forward(self, x, res=None, out=None, co0=0):
        """``res``: returns res + head(x) from the last conv's epilogue (the loop's ``disp + delta``,
        same fp32 sum), written into channel ``co0`` of ``out`` when given (HIP path only)."""
        if not _fast(x):
            y = self.conv(x)
            return y if res is None else res + y
        y = _conv(self.conv[0], [_f32(x)], "relu")
        for enc in (self.conv[2], self.conv[3]):
            d = ops.dwconv2d(y, enc.dwconv.weight, enc.dwconv.bias)   # depthwise 7x7; norm=None
            if enc.pwconv1.out_features == 4 * enc.pwconv1.in_features == 512:
                # x + gamma * pw2(gelu(pw1(.))) in one kernel: the 4C GELU map stays in LDS
                pk1, b1 = _packed(enc.pwconv1)
                pk2, b2 = _packed(enc.pwconv2)
                y = ops.edgenext_mlp(d, y, pk1, b1, pk2, b2, gamma=enc.gamma)
            else:
                e = _conv(enc.pwconv1, [d], "gelu")
                y = _conv(enc.pwconv2, [e], gamma=enc.gamma, res=y)  # x + gamma * pw2(gelu(pw1(.)))
        if res is not None:
            res = res.float()
            if not res.is_contiguous():
                res = res.contiguous()
        last = self.conv[4]
        if COUT1 and last.out_channels == 1 and last.kernel_size == (3, 3):
            # one output channel: a per-pixel fp32 dot product, not a 32-row MFMA tile
            return ops.conv3x3_cout1(y, last.weight, last.bias, res=res, out=out, co0=co0)
        return _conv(last, [y], res=res, out=out, co0=co0)


class ConvGRU(nn.Module):
    """core/update.py:34-48 (unused by FoundationStereo; kept for API parity)."""

    def __init__(self, hidden_dim, input_dim, kernel_size=3):
        super().__init__()
        p = kernel_size // 2
        self.convz = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=p)
        self.convr = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=p)
        self.convq = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=p)

    def forward(self, h, cz, cr, cq, *x_list):
        x = torch.cat(x_list, dim=1)
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(self.convz(hx) + cz)
        r = torch.sigmoid(self.convr(hx) + cr)
        q = torch.tanh(self.convq(torch.cat([r * h, x], dim=1)) + cq)
        return (1 - z) * h + z * q


class BasicMotionEncoder(nn.Module):
    """core/update.py:51-70."""

    def __init__(self, args, ngroup=8):
        super().__init__()
        self.args = args
        cor_planes = args.corr_levels * (2 * args.corr_radius + 1) * (ngroup + 1)
        self.convc1 = nn.Conv2d(cor_planes, 256, 1, padding=0)
        self.convc2 = nn.Conv2d(256, 256, 3, padding=1)
        self.convd1 = nn.Conv2d(1, 64, 7, padding=3)
        self.convd2 = nn.Conv2d(64, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 256, 128 - 1, 3, padding=1)

    def encode_into(self, disp, corr, out):
        """Writes cat([relu(conv(...)), disp]) into ``out`` (B, 128, H, W) without the cat copy."""
        return self._encode_rest(disp, _conv(self.convc1, [corr], "relu"), out)

    def motion_into(self, disp, geo_fn, out):
        """The motion path of one iteration: the lookup ``geo_fn(disp)`` and this encoder."""
        return self.encode_into(disp, geo_fn(disp), out)

    def _disp_feat(self, disp, out=None):
        d = ops.conv2d_1in(disp, self.convd1.weight, self.convd1.bias, relu=True)   # 7x7, 1 -> 64
        return _conv(self.convd2, [d], "relu", out=out)

    def _encode_rest(self, disp, c1, out):
        c = _conv(self.convc2, [c1], "relu")
        d = self._disp_feat(disp)
        # cat([cor, dsp]) with the disparity features (~disp magnitude: ~200 at cfg5) as the FIRST
        # segment: the halo conv fixes a block's exponent from its first chunk (conv_halo.h)
        nc, nd = c.shape[1], d.shape[1]
        pk, b = _packed(self.conv, cin_order=tuple(range(nc, nc + nd)) + tuple(range(nc)))
        ops.conv2d([d, c], pk, bias=b, act="relu", out=out, co0=0)
        tail = out[:, self.conv.out_channels:]
        if tail.data_ptr() != disp.data_ptr():        # run_pipelined has the head write it in place
            tail.copy_(disp)
        return out

    def forward(self, disp, corr):
        if _fast(corr):
            corr, disp = _f32(corr), _f32(disp)
            B, _, H, W = corr.shape
            return self.encode_into(disp, corr, corr.new_empty(B, self.conv.out_channels + 1, H, W))
        cor = F.relu(self.convc2(F.relu(self.convc1(corr))))
        dsp = F.relu(self.convd2(F.relu(self.convd1(disp))))
        out = F.relu(self.conv(torch.cat([cor, dsp], dim=1)))
        return torch.cat([out, disp], dim=1)


def pool2x(x):
    if _fast(x):
        return ops.pool2x(_f32(x))
    return F.avg_pool2d(x, 3, stride=2, padding=1)


def pool4x(x):
    return F.avg_pool2d(x, 5, stride=4, padding=1)


def interp(x, dest):
    if _fast(x):
        return ops.resize_bilinear(_f32(x), dest.shape[2:])
    return F.interpolate(x, dest.shape[2:], mode="bilinear", align_corners=True)


def _stacked_zr(gru):
    """[convz; convr] weights stacked along out-channels (cached per weight version)."""
    wz, wr, bz, br = gru.convz.weight, gru.convr.weight, gru.convz.bias, gru.convr.bias
    return _cached(gru, "_fsmi_zr", [wz, wr, bz, br],
                   lambda: (torch.cat([wz, wr], 0).contiguous(), torch.cat([bz, br], 0).contiguous()))


class RaftConvGRU(nn.Module):
    """core/update.py:83-95."""

    def __init__(self, hidden_dim=128, input_dim=256, kernel_size=3):
        super().__init__()
        p = kernel_size // 2
        self.convz = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=p)
        self.convr = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=p)
        self.convq = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=p)

    def zr(self, hx):
        w, b = _stacked_zr(self)
        return F.conv2d(hx, w, b, padding=self.convz.padding)

    def zr_fast(self, hx):
        return _conv((self.convz, self.convr), [hx])

    def forward(self, h, x, hx):
        fast = _fast(hx)
        if fast:
            h, x, hx = _f32(h), _f32(x), _f32(hx)
        zr = self.zr_fast(hx) if fast else self.zr(hx).float()
        qin, _ = ops.gru_reset(zr, zr, h.float(), x.float())
        q = _conv(self.convq, [qin]) if fast else self.convq(qin).float()
        ones = torch.ones_like(h[:, :1])
        return ops.gru_blend(zr, zr, q, q, h, ones)


class SelectiveConvGRU(nn.Module):
    """core/update.py:98-119 with fused gate kernels."""

    def __init__(self, hidden_dim=128, input_dim=256, small_kernel_size=1, large_kernel_size=3, patch_size=None):
        super().__init__()
        self.conv0 = nn.Sequential(nn.Conv2d(input_dim, input_dim, kernel_size=3, padding=1), nn.ReLU())
        self.conv1 = nn.Sequential(nn.Conv2d(input_dim + hidden_dim, input_dim + hidden_dim, kernel_size=3,
                                             padding=1), nn.ReLU())
        self.small_gru = RaftConvGRU(hidden_dim, input_dim, small_kernel_size)
        self.large_gru = RaftConvGRU(hidden_dim, input_dim, large_kernel_size)

    def context_pre(self, inp):
        """conv0's contribution of the context segment plus its bias, ``W0[:, :Ci] * inp + b0``.

        ``x[0]`` of every call is the level's context feature ``inp[i]``, fixed for the whole
        refinement loop (core/foundation_stereo.py:222-226 build it once; core/update.py:142-151 pass
        it each iteration), and conv0 is linear in its input channels: this part is computed once
        per forward and passed back as ``forward(..., pre=)``, which convolves only the remaining
        channels and adds it before the ReLU (act 7) -- 1/3 (gru04 / gru08) and 1/2 (gru16) of
        conv0's MACs per iteration.  HIP path only."""
        inp = _f32(inp)
        pk, b = _packed(self.conv0[0], cin_order=tuple(range(inp.shape[1])))
        return ops.conv2d([inp], pk, bias=b)

    def _conv0_rest(self, segs, pre):
        """ReLU(W0[:, segs] * cat(segs) + pre), ``segs`` the (tensor, conv0 input channel offset) pairs
        ``pre`` does not cover (see ``context_pre``).  The first segment's LAST 32 channels go first:
        the motion features (gru04) carry the disparity (~1e2 px) as their last channel, and the kernel
        fixes a tile's block exponent from its first 32-channel chunk (range mode 2, conv_halo.h
        chunk_exp), as the motion encoder orders its own cat."""
        t0, c0 = segs[0]
        c1 = t0.shape[1]
        if c1 > 32 and (c1 - 32) % 8 == 0:
            ss = [(t0, c1 - 32, 32), (t0, 0, c1 - 32)]
            order = list(range(c0 + c1 - 32, c0 + c1)) + list(range(c0, c0 + c1 - 32))
        else:
            ss, order = [t0], list(range(c0, c0 + c1))
        for t, c in segs[1:]:
            ss.append(t)
            order += list(range(c, c + t.shape[1]))
        pk, _ = _packed(self.conv0[0], cin_order=tuple(order))
        return ops.conv2d(ss, pk, act="relu_pre", res=pre)

    def forward(self, att, h, *x, pre=None, fork_small=True):
        """``pre``: ``context_pre(x[0])`` of this forward's context feature (HIP path; x[0] is then not read;
        the torch path ignores it, its conv0 takes the whole cat).  ``fork_small``: with ``OVERLAP`` the small
        branch runs on the branch stream; False (a caller on a side stream, streams.py capture_fork): in order."""
        if _fast(h):
            h = _f32(h)
            if pre is not None:
                segs, c = [], x[0].shape[1]
                for t in x[1:]:
                    segs.append((_f32(t), c))
                    c += t.shape[1]
                xc = self._conv0_rest(segs, pre)
            else:
                xc = _conv(self.conv0[0], _f32s(x), "relu")          # cat(x) as input segments
            hx = _conv(self.conv1[0], [xc, h], "relu")
            # gates in the conv epilogues: z / r*h from the stacked zr convs, then each convq reads
            # [r*h, x] as two segments and blends straight into the new state
            att = att.float().contiguous()
            out = torch.empty_like(h)

            def branch(gru, mode):
                z, rh = torch.empty_like(h), torch.empty_like(h)
                pk, b = _packed(gru.convz, gru.convr)
                ops.conv2d_gate([hx], pk, b, "zr", h=h, z=z, rh=rh)
                pk, b = _packed(gru.convq)
                return pk, b, z, rh

            sg = self.small_gru

            def small():                                 # out = small branch * att
                pk, b, z, rh = branch(sg, "blend_small")
                ops.conv2d_gate([rh, xc], pk, b, "blend_small", h=h, z=z, att=att, out=out)

            # small (1x1) branch on a side stream beside the large branch's zr conv; the
            # large blend adds into ``out`` after the small blend has written it
            main = streams.current(h.device)
            side = streams.side(h.device, streams.BRANCH) if OVERLAP and fork_small else main
            with streams.fork(side, main):
                small()
            pk, b, z, rh = branch(self.large_gru, "blend_large")
            streams.join(main, side)
            ops.conv2d_gate([rh, xc], pk, b, "blend_large", h=h, z=z, att=att, out=out)
            return out
        x = torch.cat(x, dim=1) if len(x) > 1 else x[0]
        x = self.conv0(x)
        hx = self.conv1(torch.cat([x, h], dim=1))
        # .float(): no-ops in fp32; under the reference's fp16 autocast the gates stay fp32
        zr_s = self.small_gru.zr(hx).float()
        zr_l = self.large_gru.zr(hx).float()
        h = h.float()
        qs_in, ql_in = ops.gru_reset(zr_s, zr_l, h, x.float())
        q_s = self.small_gru.convq(qs_in).float()
        q_l = self.large_gru.convq(ql_in).float()
        return ops.gru_blend(zr_s, zr_l, q_s, q_l, h, att.float())


class BasicSelectiveMultiUpdateBlock(nn.Module):
    """core/update.py:122-159."""

    def __init__(self, args, hidden_dim=128, volume_dim=8):
        super().__init__()
        self.args = args
        self.encoder = BasicMotionEncoder(args, volume_dim)
        n = args.n_gru_layers
        if n == 3:
            self.gru16 = SelectiveConvGRU(hidden_dim, hidden_dim * 2)
        if n >= 2:
            self.gru08 = SelectiveConvGRU(hidden_dim, hidden_dim * (n == 3) + hidden_dim * 2)
        self.gru04 = SelectiveConvGRU(hidden_dim, hidden_dim * (n > 1) + hidden_dim * 2)
        self.disp_head = DispHead(hidden_dim, 256)
        self.mask = nn.Sequential(nn.Conv2d(128, 64, 3, padding=1), nn.ReLU(inplace=True),
                                  nn.Conv2d(64, 32, 3, padding=1), nn.ReLU(inplace=True))

    def forward(self, net, inp, corr, disp, att):
        if _fast(corr):     # one iteration in order on the calling stream; conv0 convolves the whole cat (pre=None)
            corr = _f32(corr)
            return self._iteration(_f32s(net), _f32s(inp), lambda d: corr, _f32(disp), _f32s(att), None, False)
        n = self.args.n_gru_layers
        if n == 3:
            net[2] = self.gru16(att[2], net[2], inp[2], pool2x(net[1]))
        if n >= 2:
            if n > 2:
                net[1] = self.gru08(att[1], net[1], inp[1], pool2x(net[0]), interp(net[2], net[1]))
            else:
                net[1] = self.gru08(att[1], net[1], inp[1], pool2x(net[0]))
        motion = torch.cat([inp[0], self.encoder(disp, corr)], dim=1)
        if n > 1:
            net[0] = self.gru04(att[0], net[0], motion, interp(net[1], net[0]))
        delta_disp = self.disp_head(net[0])
        mask = .25 * self.mask(net[0])
        return net, mask, delta_disp

    def context_pre(self, inp):
        """Per GRU level (gru04, gru08, gru16 as ``inp``), ``SelectiveConvGRU.context_pre`` of its context
        feature: the loop-invariant part of conv0, computed once per forward (HIP path; None otherwise or
        with ``update.CTX_PRE = False``)."""
        if not CTX_PRE or not inp or not _fast(inp[0]):
            return None
        grus = [self.gru04, getattr(self, "gru08", None), getattr(self, "gru16", None)]
        return [g.context_pre(x) for g, x in zip(grus, inp) if g is not None]

    def forward_overlapped(self, net, inp, geo_fn, disp, att, pre=None):
        """``forward(net, inp, geo_fn(disp), disp, att)`` with the motion path -- the lookup and
        the motion encoder, which depend only on ``disp`` -- on a side stream, concurrently with
        gru16 / gru08 (small 1/16 and 1/8 maps that leave most CUs idle), joined before gru04, and the mask
        head on the branch stream beside the disparity head (both read net[0] only).  With ``OVERLAP`` off
        the same sequence runs on the calling stream.  ``pre``: ``context_pre(inp)`` or None."""
        return self._iteration(net, inp, geo_fn, disp, att, pre, OVERLAP)

    def _iteration(self, net, inp, geo_fn, disp, att, pre, overlap):
        """One refinement iteration on the HIP path; ``overlap``: the motion and branch streams, else every
        stream is the calling one (streams.fork / join then run the sequence in order).
        Cross-stream buffers (``enc``) are allocated on the calling stream and ``disp`` is only
        released by the caller after the join, so the caching allocator never recycles memory a
        pending side-stream kernel still reads.  Captures into a hipGraph as a fork/join."""
        dev, n = disp.device, self.args.n_gru_layers
        main = streams.current(dev)
        s_mot = streams.side(dev, streams.MOTION) if overlap else main
        s_br = streams.side(dev, streams.BRANCH) if overlap else main
        B, _, H, W = disp.shape
        enc = disp.new_empty(B, self.encoder.conv.out_channels + 1, H, W)
        with streams.fork(s_mot, main):
            self.encoder.motion_into(disp, geo_fn, enc)
        p0, p1, p2 = (list(pre) + [None] * 3)[:3] if pre is not None else (None, None, None)
        if n == 3:
            net[2] = self.gru16(att[2], net[2], inp[2], pool2x(net[1]), pre=p2)
        if n >= 2:
            xs = [pool2x(net[0])] + ([interp(net[2], net[1])] if n > 2 else [])
            net[1] = self.gru08(att[1], net[1], inp[1], *xs, pre=p1)
        streams.join(main, s_mot)
        if n > 1:       # motion = cat([inp[0], enc]) stays two segments of gru04.conv0's input
            net[0] = self.gru04(att[0], net[0], inp[0], enc, interp(net[1], net[0]), pre=p0)
        with streams.fork(s_br, main):
            mask = self._mask_head(net[0])
        delta_disp = self.disp_head(net[0])
        streams.join(main, s_br)
        return net, mask, delta_disp

    def _mask_head(self, n0):
        """0.25 * mask(n0) on the HIP path (the scale in the last conv's epilogue)."""
        return _conv(self.mask[2], [_conv(self.mask[0], [n0], "relu")], "relu", alpha=0.25)

    def run_pipelined(self, net, inp, geo_fn, disp, att, iters, pre=None):
        """``iters`` refinement iterations (``disp += forward(net, inp, geo_fn(disp), disp, att)[2]``
        each) with gru16 / gru08 running one iteration ahead on a stream of their own.

        gru16(t+1) needs only net[1](t) and net[2](t), so it runs beside gru04(t) and the heads;
        gru08(t+1) needs net[0](t), so it starts as soon as gru04(t) is done, beside the disparity
        head and the motion path of t+1 (lookup + encoder, on the motion stream, which need only
        disp(t+1)).  The critical path per iteration is gru04 + max(head + motion, gru08) instead of
        gru16 + gru08 + gru04 + head.  Every value is computed by the same kernels from the same
        inputs as ``forward`` (bit-identical); only the order of independent work changes.
        One pipeline stream and whole-stream joins: ``join(main, s_gru)`` is issued after
        gru08(t) and before gru16(t+1) is enqueued, so gru04(t) waits for the former only.  The
        mask head shares the motion stream.  A tensor read on another stream is freed only after
        the freeing stream has joined the reader, so the caching allocator never recycles memory
        a pending kernel still reads.  Returns (net, mask, disp); the mask head runs in the last
        iteration only (test mode discards the others).  ``pre``: ``context_pre(inp)`` (loop-invariant
        conv0 parts per level) or None."""
        dev = disp.device
        main = streams.current(dev)
        s_mask, s_gru = streams.side(dev, streams.MOTION), streams.side(dev, streams.PIPELINE)
        s_mot = main if MOTION_ON_MAIN else s_mask       # the motion path's stream; the mask head keeps s_mask
        n0, n1, n2 = net
        p0, p1, p2 = pre if pre is not None else (None, None, None)
        B, _, H, W = disp.shape
        nc = self.encoder.conv.out_channels
        # fork_small=False for every GRU on the pipeline stream: its branches run in order there -- a fork
        # from it would be a side stream waiting on the pipeline stream and waited on by it (capture_fork)
        with streams.fork(s_gru, main):
            n2 = self.gru16(att[2], n2, inp[2], pool2x(n1), pre=p2, fork_small=False)
            n1 = self.gru08(att[1], n1, inp[1], pool2x(n0), interp(n2, n1), pre=p1, fork_small=False)
        mask = None
        # the disparity lives in the last channel of the encoder output it feeds: the disparity head
        # writes disp + delta straight into the next iteration's buffer (no cat copy, no add pass)
        enc = disp.new_empty(B, nc + 1, H, W)                                   # on main
        enc[:, nc:].copy_(disp)
        disp = enc[:, nc:]
        for t in range(iters):
            with streams.fork(s_mot, main):
                self.encoder.motion_into(disp, geo_fn, enc)
            streams.join(main, s_gru)                     # gru08(t): enqueued last on s_gru so far
            streams.join(main, s_mot)                     # motion(t)
            if t + 1 < iters:
                with streams.on(s_gru):                  # gru16(t+1), beside gru04(t): behind gru08(t), no wait
                    n2 = self.gru16(att[2], n2, inp[2], pool2x(n1), pre=p2, fork_small=False)
                    # gru08(t+1)'s upsampled gru16 input, also beside gru04(t): one kernel less between
                    # gru04(t) and gru08(t+1)
                    up2 = interp(n2, n1)
            # gru04's small branch on the branch stream (a 4th stream) unless PIPE_BRANCH is off
            n0 = self.gru04(att[0], n0, inp[0], enc, interp(n1, n0), pre=p0, fork_small=PIPE_BRANCH)
            if t + 1 < iters:
                with streams.fork(s_gru, main):          # gru08(t+1) after gru04(t), beside the heads + motion(t+1)
                    n1 = self.gru08(att[1], n1, inp[1], pool2x(n0), up2, pre=p1, fork_small=False)
                enc = disp.new_empty(B, nc + 1, H, W)
                self.disp_head(n0, res=disp, out=enc, co0=nc)
                disp = enc[:, nc:]
                streams.join(main, s_mot)
            else:
                # test mode upsamples only the last iteration's disparity: the reference computes the
                # mask head every iteration and discards all but the last (core/foundation_stereo.py:243-244)
                with streams.fork(s_mask, main):
                    mask = self._mask_head(n0)
                disp = self.disp_head(n0, res=disp)
                streams.join(main, s_mask)
        streams.join(main, s_gru)
        return [n0, n1, n2], mask, disp
