"""CPU side of the backbone kernel tests (tests/test_gpu_backbone_kernels.py):

* tests/backbone_reference.py, the fp64 reference those tests compare against, agrees with torch's own
  functionals in fp64;
* a plain fp32 restatement of every operation stays inside its tolerance on the GPU test's inputs (the
  tolerances are reachable), and the fp64 result rounded to fp32 passes;
* the comparison discriminates: reference-made "device results" carrying one fault each are refused by the
  GPU test's own check functions, on the GPU test's own case lists;
* the case lists exercise what they claim: the expected key-range counts equal the restated
  ``vit_attn_splits``, the InstanceNorm cases carry the path they take and both paths occur.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import backbone_reference as br
from tests.test_gpu_backbone_kernels import (ATTN_CASES, ATTN_PADDING_CASES, BICUBIC_CASES, IN_3P, IN_CASES, IN_REG,
                                             IN_TRIPLES, LN_CASES, SOFTARGMIN_CASES, TOKEN_CASES, UPSAMPLE_CASES,
                                             XCA_CASES, _check, _check_bicubic, _check_exact)

f32 = torch.float32


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _refused(got, ref, tol, what):
    with pytest.raises(AssertionError, match="max .diff."):
        _check(got.float(), ref, tol, what)


# ---------------------------------------------------------------- the reference matches torch

def test_reference_matches_torch_norms():
    c = br.layernorm_inputs(17, 50, 21, 7, "mean64", "wb")
    x, w, b = c["x"].double(), c["w"].double(), c["b"].double()
    want = F.layer_norm(x[:, :, 7:28].transpose(1, 2), (17,), w, b, 1e-6).transpose(1, 2)
    assert _rel(c["ref"], want) <= 1e-12
    want = F.layer_norm(x.transpose(1, 2), (17,), None, None, 1e-3).transpose(1, 2)
    assert _rel(br.layernorm_ref(c["x"], eps=1e-3), want) <= 1e-12
    c = br.instnorm_inputs(257, "mean64")
    for eps in (1e-5, 1e-3):
        assert _rel(br.instnorm_ref(c["x"], eps=eps), F.instance_norm(c["x"].double(), eps=eps)) <= 1e-12
    want = F.relu(F.leaky_relu(F.instance_norm(c["x"].double(), eps=1e-5), 0.01) + c["res"].double())
    assert _rel(br.instnorm_ref(c["x"], "leaky", c["res"], "relu"), want) <= 1e-12


def test_reference_matches_torch_attention():
    c = br.attention_inputs(1, 2, 65, 128)
    q, k, v = (a.double().transpose(-1, -2) for a in br.split_qkv(c["qkv"], 2))       # (B, heads, Tp, hd)
    want = F.scaled_dot_product_attention(q, k[:, :, :65], v[:, :, :65], scale=0.125)
    assert _rel(c["ref"], want.transpose(-1, -2).reshape(1, 128, 128)) <= 1e-12
    c = br.xca_inputs(96, 8, 129)
    q, k, v = c["qkv"].double().view(2, 3, 8, 12, 129).unbind(1)
    a = torch.softmax(F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1) * c["temp"].double(), -1)
    assert _rel(c["ref"], (a @ v).reshape(2, 96, 129)) <= 1e-12


def test_reference_matches_torch_layout_and_heads():
    for k in (2, 4):
        x = br.d2s_input(k)
        B, CK, H, W = x.shape
        C = CK // (k * k)
        # pixel_shuffle wants channel c * k * k + ky * k + kx
        want = F.pixel_shuffle(x.view(B, k * k, C, H, W).transpose(1, 2).reshape(B, CK, H, W), k)
        assert torch.equal(br.depth_to_space_ref(x, k), want)
    c = br.tokens_inputs(2, 5, 7, 64)
    seq = torch.cat([c["emb"], c["cls"].view(1, 5, 1).expand(2, -1, -1)], 2) + c["pos"][None, :, :8]
    assert torch.equal(c["ref"][:, :, :8], seq) and not bool(c["ref"][:, :, 8:].any())
    c = br.softargmin_inputs(20)
    want = (torch.softmax(c["x"].double(), 1) * torch.arange(20.0, dtype=torch.double).view(1, 20, 1, 1)).sum(1, True)
    assert _rel(c["ref"], want) <= 1e-12
    c = br.upsample_inputs(3, 5)
    # independently: every output pixel's 9 neighbours gathered by index
    d = F.pad(c["disp"].double() * 4.0, (1, 1, 1, 1))
    p = torch.softmax(c["logits"].double(), 1)
    want = torch.zeros(2, 12, 20, dtype=torch.double)
    for kk in range(9):
        nb = d[:, 0, kk // 3:kk // 3 + 3, kk % 3:kk % 3 + 5]
        want += p[:, kk] * nb.repeat_interleave(4, 1).repeat_interleave(4, 2)
    assert _rel(c["ref_softmax"], want) <= 1e-12
    for Hi, Wi, Ho, Wo in BICUBIC_CASES + [(50, 30, 33, 71)]:
        x = br.bicubic_input(Hi, Wi)
        want = F.interpolate(x.double(), size=(Ho, Wo), mode="bicubic", align_corners=False)
        assert _rel(br.bicubic_ref(x, (Ho, Wo)), want) <= 1e-12


# ---------------------------------------------------------------- LayerNorm

def _ln_args(c):
    return c["x"], c["w"], c["b"], c["eps"], c["n"], c["off"]


def _one_pass(v, dims, eps):
    """(v - mean) / sqrt(E[v^2] - mean^2 + eps) in fp32."""
    v = v.float()
    mean = v.mean(dims, keepdim=True)
    var = (v * v).mean(dims, keepdim=True) - mean * mean
    return (v - mean) / (var.clamp_min(0) + eps).sqrt()


def test_layernorm_check():
    worst = 0.0
    seen = {"one-pass": 0, "cnt": 0}
    for case in LN_CASES:
        c = br.layernorm_inputs(*case)
        C, n, off = c["C"], c["n"], c["off"]
        what = f"layernorm {case}"
        _check(c["ref"].float(), c["ref"], c["tol"], what + " fp64 rounded")
        e = _check(br.layernorm_ref(*_ln_args(c), dtype=f32), c["ref"], c["tol"], what + " in fp32")
        worst = max(worst, e / c["tol"])
        w = 1.0 if c["w"] is None else c["w"].double().view(1, -1, 1)
        b = 0.0 if c["b"] is None else c["b"].double().view(1, -1, 1)
        # the one-pass variance is off by up to an ulp of E[x^2] ~ 4097 (5e-4 of the unit variance), a
        # different amount per token: a single token (n = 1) may by chance sit inside the tolerance
        if c["stats"] == "mean64" and n >= 16:
            seen["one-pass"] += 1
            got = _one_pass(c["x"][:, :, off:off + n], 1, c["eps"]).double() * w + b
            _refused(got, c["ref"], c["tol"], what + " one-pass variance")
        if C % 16:
            # mean and variance over LN_G * cnt channels, cnt the first channel group's
            seen["cnt"] += 1
            v = c["x"].double()[:, :, off:off + n]
            Cr = 16 * ((C + 15) // 16)
            mean = v.sum(1, keepdim=True) / Cr
            var = ((v - mean) ** 2).sum(1, keepdim=True) / Cr
            _refused((v - mean) / (var + c["eps"]).sqrt() * w + b, c["ref"], c["tol"], what + " cnt-rounded C")
    print(f"layernorm: fp32 restatement at most {worst:.3g} of the tolerance")
    assert seen["one-pass"] >= 8 and seen["cnt"] >= 8, seen
    assert {c[5] for c in LN_CASES} == {"wb", "w", None}


# ---------------------------------------------------------------- InstanceNorm

def test_instnorm_paths_labelled():
    for HW, _, path in IN_CASES:
        assert path == br.instnorm_path(HW), (HW, path)
    assert {p for _, _, p in IN_CASES} == {IN_REG, IN_3P}
    hws = {hw for hw, _, _ in IN_CASES}
    assert {br.IN_REG_MAX, br.IN_REG_MAX + 1} <= hws, "the boundary between the two kernels"


def test_instnorm_check():
    worst = 0.0
    one_pass = set()
    for HW, stats, path in IN_CASES:
        c = br.instnorm_inputs(HW, stats)
        for act, res, act2 in IN_TRIPLES:
            r = c["res"] if res else None
            ref = br.instnorm_ref(c["x"], act, r, act2)
            tol = br.norm_tol(ref)
            what = f"instance norm HW {HW} {stats} {act}/{res}/{act2}"
            _check(ref.float(), ref, tol, what + " fp64 rounded")
            worst = max(worst, _check(br.instnorm_ref(c["x"], act, r, act2, dtype=f32), ref, tol, what + " in fp32") / tol)
            if stats == "mean64":
                got = br.ACTS[act](_one_pass(c["x"], (2, 3), 1e-5)).double()
                if res:
                    got = br.ACTS[act2](got + r.double())
                _refused(got, ref, tol, what + " one-pass variance")
                one_pass.add(path)
    print(f"instance norm: fp32 restatement at most {worst:.3g} of the tolerance")
    assert one_pass == {IN_REG, IN_3P}


# ---------------------------------------------------------------- attention

def test_attention_cases_split_as_claimed():
    for B, heads, T, Tp, ns, _ in ATTN_CASES:
        assert br.attn_splits(B, heads, T, Tp)[0] == ns, (B, heads, T, Tp)
        assert Tp % 64 == 0 and T <= Tp
    assert {c[4] for c in ATTN_CASES} >= {1, 2, 5, 8}
    assert br.attn_splits(1, 1, 1600, 1600) == (5, 5) and min(8, 25 // 4) == 6      # 6 asked for, 5 returned
    for B, heads, T, Tp in ATTN_PADDING_CASES:
        assert T < Tp


def _attn_scores(c):
    q, k, v = br.split_qkv(c["qkv"].double(), c["heads"])
    return torch.einsum("bhdi,bhdj->bhij", q, k) * c["scale"], v          # (B, heads, Tp queries, Tp keys)


def _attn_out(p, v, keys):
    return torch.einsum("bhij,bhdj->bhdi", p, v[..., keys]).reshape(v.shape[0], -1, v.shape[-1])


def test_attention_check():
    worst = 0.0
    seen = set()
    for B, heads, T, Tp, ns, variant in ATTN_CASES:
        c = br.attention_inputs(B, heads, T, Tp, variant)
        ref, tol = c["ref"], c["tol"]
        what = f"attention T {T} Tp {Tp} {variant}"
        _check(ref.float(), ref, tol, what + " fp64 rounded")
        e = _check(br.sdpa_ref(c["qkv"], heads, T, c["scale"], dtype=f32), ref, tol, what + " in fp32")
        worst = max(worst, e / tol)
        s, v = _attn_scores(c)
        dominant = variant == "dominant"          # there the keys >= 256 weigh nothing, by construction
        if T < Tp and not dominant:
            seen.add("key T")
            _refused(_attn_out(torch.softmax(s[..., :T + 1], -1), v, slice(0, T + 1)), ref, tol, what + " key T included")
        if T > 1 and not dominant:
            seen.add("key T - 1")
            _refused(_attn_out(torch.softmax(s[..., :T - 1], -1), v, slice(0, T - 1)), ref, tol, what + " key T - 1 dropped")
        if ns > 1:
            per = br.attn_splits(B, heads, T, Tp)[1] * 64
            last = (ns - 1) * per
            seen.add("ranges")
            if not dominant:
                _refused(_attn_out(torch.softmax(s[..., :last], -1), v, slice(0, last)), ref, tol,
                         what + " last key range dropped")
            num, den = 0.0, 0.0
            for r in range(ns):
                keys = slice(r * per, min(T, (r + 1) * per))
                p = torch.exp(s[..., keys] - s[..., keys].amax(-1, keepdim=True))
                num = num + _attn_out(p, v, keys)
                den = den + p.sum(-1).unsqueeze(2).expand(-1, -1, 64, -1).reshape(B, heads * 64, Tp)
            _refused(num / den, ref, tol, what + " ranges merged without their weights")
    print(f"attention: fp32 restatement at most {worst:.3g} of the tolerance")
    assert seen == {"key T", "key T - 1", "ranges"}
    # the dominant case is what it claims: for most queries the second range's weight 2^(m_1 - m_0) is below
    # fp32's smallest normal
    c = br.attention_inputs(1, 1, 449, 512, "dominant")
    s, _ = _attn_scores(c)
    gap = (s[..., :256].amax(-1) - s[..., 256:449].amax(-1)) * 1.4426950408889634
    assert float((gap > 126).double().mean()) > 0.5, float((gap > 126).double().mean())


def test_attention_padding_inputs():
    for B, heads, T, Tp in ATTN_PADDING_CASES:
        c = br.attention_inputs(B, heads, T, Tp)
        for value in (0.0, 1e3):
            qkv = br.attention_padding(c, value)
            assert torch.equal(qkv[..., :T], c["qkv"][..., :T])
            assert bool((qkv[..., T:].abs() == value).all())
            assert _rel(br.sdpa_ref(qkv, heads, T, 0.125)[..., :T], c["ref"][..., :T]) == 0.0
        assert float(qkv[..., T:].min()) == -1e3 and float(qkv[..., T:].max()) == 1e3


# ---------------------------------------------------------------- XCA

def test_xca_check():
    worst = 0.0
    seen = set()
    for C, heads, N, variant in XCA_CASES:
        c = br.xca_inputs(C, heads, N, variant)
        ch = C // heads
        ref, tol = c["ref"], c["tol"]
        what = f"xca C {C} heads {heads} N {N} {variant}"
        _check(ref.float(), ref, tol, what + " fp64 rounded")
        worst = max(worst, _check(br.xca_ref(c["qkv"], c["temp"], heads, dtype=f32), ref, tol, what + " in fp32") / tol)
        q, k, v = c["qkv"].double().view(2, 3, heads, ch, N).unbind(1)
        temp = c["temp"].double().view(1, heads, 1, 1)
        qn, kn = q.norm(dim=-1, keepdim=True), k.norm(dim=-1, keepdim=True)
        if ch > 1:                    # with one channel per head the softmax is over one score: always 1
            seen.add("k norm")
            a = torch.softmax((q / qn.clamp_min(1e-12)) @ k.transpose(-2, -1) * temp, -1)
            _refused((a @ v).reshape(2, C, N), ref, tol, what + " k not normalised")
        if variant == "rows":
            seen.add("clamp")
            qh = q / (qn * qn).clamp_min(1e-12).sqrt()
            kh = k / (kn * kn).clamp_min(1e-12).sqrt()
            a = torch.softmax(qh @ kh.transpose(-2, -1) * temp, -1)
            _refused((a @ v).reshape(2, C, N), ref, tol, what + " clamp on the squared norm")
            assert float(qn[:, :, 0].max()) == 0.0 and float(kn[:, :, 1].max()) == 0.0
            assert 1e-12 < float(qn[:, :, 2].min()) and float(qn[:, :, 2].max()) < 1e-6
    print(f"xca: fp32 restatement at most {worst:.3g} of the tolerance")
    assert seen == {"k norm", "clamp"}
    assert {c[0] // c[1] for c in XCA_CASES} >= {1, 40}


# ---------------------------------------------------------------- exact kernels

def test_tokens_check():
    for B, C, N, Tp in TOKEN_CASES:
        c = br.tokens_inputs(B, C, N, Tp)
        _check_exact(c["ref"].clone(), c["ref"], "unfaulted")
        assert bool((c["pos"][:, N + 1:] != 0).all()) if Tp > N + 1 else True
        if Tp > N + 1:
            got = c["ref"].clone()
            got[:, :, N + 1:] += c["pos"][None, :, N + 1:]
            with pytest.raises(AssertionError, match="elements differ"):
                _check_exact(got, c["ref"], "pos added past column N")
    assert any(Tp > N + 1 for _, _, N, Tp in TOKEN_CASES) and any(Tp == N + 1 for _, _, N, Tp in TOKEN_CASES)


# ---------------------------------------------------------------- bicubic, soft-argmin, upsampling

def test_bicubic_check():
    refused = 0
    for Hi, Wi, Ho, Wo in BICUBIC_CASES:
        x = br.bicubic_input(Hi, Wi)
        what = f"bicubic {Hi}x{Wi} -> {Ho}x{Wo}"
        _check_bicubic(br.bicubic_ref(x, (Ho, Wo)).float(), x, (Ho, Wo), what + " fp64 rounded")
        _check_bicubic(br.bicubic_ref(x, (Ho, Wo), dtype=f32), x, (Ho, Wo), what + " in fp32")
        zero = br.bicubic_ref(x, (Ho, Wo), border="zero")
        # no tap outside the image carries weight at identity size (weights 0, 1, 0, 0) or at an integer
        # downscale (64 -> 16 reads pixels 4 i ... 4 i + 3)
        assert bool((zero != br.bicubic_ref(x, (Ho, Wo))).any()) == ((Hi, Wi) in ((1, 1), (2, 3)))
        if (Hi, Wi) in ((1, 1), (2, 3)):
            with pytest.raises(AssertionError, match="max .diff."):
                _check_bicubic(zero.float(), x, (Ho, Wo), what + " zero taps")
            refused += 1
    assert refused == 2
    x = br.bicubic_input(32, 40)
    assert torch.equal(br.bicubic_ref(x, (32, 40), dtype=f32), x)


def test_softargmin_check():
    worst = [0.0, 0.0]
    tails = 0
    for D, variant in SOFTARGMIN_CASES:
        c = br.softargmin_inputs(D, variant)
        tol = br.softargmin_tol(D)
        what = f"soft-argmin D {D} {variant}"
        _check(c["ref"].float(), c["ref"], tol, what + " fp64 rounded")
        worst[0] = max(worst[0], _check(br.softargmin_ref(c["x"], True, dtype=f32), c["ref"], tol, what + " in fp32") / tol)
        rtol = br.regression_tol(D)
        got = br.softargmin_ref(c["prob"], False, dtype=f32)
        if rtol:
            worst[1] = max(worst[1], _check(got, c["ref_prob"], rtol, what + " plain sum in fp32") / rtol)
        else:
            _check_exact(got, torch.zeros_like(got), what)
        if variant == "onehot":
            assert torch.equal(c["ref"].float(), c["hot"].float())
        if variant == "pm88":
            assert float(c["x"].amax(1).min()) > 87 and float(c["x"].amin(1).max()) < -87
        if D > 8 and D % 8:
            tails += 1
            D8 = D - D % 8
            _refused(br.softargmin_ref(c["x"][:, :D8], True), c["ref"], tol, what + " tail ignored")
    print(f"soft-argmin: fp32 restatement at most {worst[0]:.3g} of the tolerance, the plain sum {worst[1]:.3g}")
    assert tails >= 6
    assert {D for D, _ in SOFTARGMIN_CASES} >= {1, 7, 8, 9, 20}


def test_upsample_check():
    worst = [0.0, 0.0]
    for h, w, variant in UPSAMPLE_CASES:
        c = br.upsample_inputs(h, w, variant)
        what = f"upsample {h}x{w} {variant}"
        for i, (sm, ref, wts, scale) in enumerate([(False, c["ref_plain"], c["wts"], 1.0),
                                                   (True, c["ref_softmax"], c["logits"], 4.0)]):
            tol = br.upsample_tol(sm)
            _check(ref.float(), ref, tol, what + " fp64 rounded")
            e = _check(br.upsample_ref(c["disp"], wts, sm, scale, dtype=f32), ref, tol, what + f" in fp32 (softmax {sm})")
            worst[i] = max(worst[i], e)
            _refused(br.upsample_ref(c["disp"], wts, sm, scale, padding="replicate"), ref, tol, what + " clamped padding")
        if variant == "pm80":
            assert float(c["logits"].amax(1).min()) > 78 and float(c["logits"].amin(1).max()) < -78
    print(f"upsample: fp32 restatement {worst[0]:.3g} (weights given), {worst[1]:.3g} (softmax, scale 4)")
