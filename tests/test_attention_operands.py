"""CPU: the selective-softmax operands of tests/test_attention_exact.py (tests/hip_util.py) are what they claim -- gaps, margins,
set sizes, GroupNorm statistics, the kernels' q rounding, the fused projection, and the fp64 oracle's answer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops
from tests.hip_util import (QS_INFER, QS_TRAIN, assert_banded_rel_l2_tokens, assert_exact_bound, bf16_rne, selective_operands,
                            selective_reference)

CASES = [(2, 100, 64, "R1"), (2, 100, 64, "R2"), (2, 100, 64, "R3"), (2, 100, 64, "stair"), (2, 1000, 128, "R3"),
         (2, 1024, 128, "R2"), (1, 1000, 128, "stair"), (2, 48, 64, "R2"), (3, 8, 16, "R1"), (2, 100, 16, "R3"), (2, 1000, 96, "stair"),
         (2, 33, 32, "stair"), (2, 64, 256, "R3")]


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


@pytest.mark.parametrize("B,L,C,regime", CASES)
def test_gaps_margins_and_sets(B, L, C, regime):
    o = selective_operands(B, L, C, regime, seed=5, fused=True)
    r = selective_reference(o["qh"], o["k"], o["v"], j=o["j"])
    assert float(r["gap"].min()) >= 24
    if regime == "R1":
        assert float(r["margin"].abs().max()) == 0
    elif regime == "R2":
        assert 30 <= float(r["margin"].min()) == float(r["margin"].max()) <= 90
    elif regime == "R3":
        assert float(r["margin"].min()) >= 140
    else:
        # stair: S(i) in the last tile; the maximum of each key tile (every tile holds every code) lies 0, 7.75 or 8.25 above the
        # running maximum, which is raised only by more than 8 (attention_tile, tr_attn_fwd_mfma_kernel)
        H = C // 8
        s = (o["qh"].view(B, L, H, 8).transpose(1, 2) @ o["k"].view(B, L, H, 8).permute(0, 2, 3, 1))
        T = (L + 31) // 32
        tmax = torch.stack([s[..., 32 * t:32 * t + 32].amax(-1) for t in range(T - 1)], -1).flatten(0, 2)
        steps = set()
        for row in tmax.tolist():
            m = row[0]
            for t in row[1:]:
                steps.add(t - m)
                m = t if t - m > 8 else m
        assert steps <= {0.0, 7.75, 8.25} and (T < 4 or {7.75, 8.25} <= steps), steps
        sel = s == s.amax(-1, keepdim=True)
        assert not bool(sel[..., :32 * (T - 1)].any())
    # mean over 2^j keys of |v| <= 7 (one sign per (image, head, dim)): exact in bf16, never 0
    out = r["out"]
    assert torch.equal(bf16_rne(out).double(), out) and bool((out != 0).all())
    # every head / image selects differently (signed permutations per head, codes per image)
    H = C // 8
    if H > 1 and L > 8:
        o4 = out.view(B, L, H, 8)
        assert not torch.equal(o4[:, :, 0], o4[:, :, 1])


@pytest.mark.parametrize("B,L,C,regime", CASES)
def test_kernel_rounding_of_q_lands_on_the_codes(B, L, C, regime):
    o = selective_operands(B, L, C, regime, seed=6, fused=True)
    for q, qs in ((o["q_infer"], QS_INFER), (o["q_train"], QS_TRAIN)):
        assert torch.equal(bf16(q * torch.tensor(qs, dtype=torch.float32)), o["qh"])


@pytest.mark.parametrize("B,L,C,regime", CASES)
def test_fused_groupnorm_and_projection_are_exact(B, L, C, regime):
    """GroupNorm statistics of x are mean 0 / variance 1 exactly; the kernel's folded weights W' = bf16(bf16(w * qs) * a) with
    a = gamma * rsqrt(1 + eps) (+-4 fp32 ulps) and bias b' = b reproduce qh, k, v after the one bf16 rounding of the projection."""
    o = selective_operands(B, L, C, regime, seed=7, fused=True)
    x, G = o["x"].double(), o["groups"]
    xg = x.view(B, L, G, C // G)
    assert bool((xg.mean((1, 3)) == 0).all()) and bool((xg.pow(2).mean((1, 3)) == 1).all())
    scale = torch.tensor([QS_INFER] * C + [1.0] * 2 * C, dtype=torch.float32)
    w32 = bf16(o["wqkv"] * scale[:, None])
    b32 = o["bqkv"] * scale
    for ulps in (-4, 0, 4):
        a = float(o["gamma"][0]) / np.sqrt(1 + o["eps"]) * (1 + ulps * 2.0 ** -24)
        wf = bf16(w32 * torch.tensor(a, dtype=torch.float32))
        assert torch.equal(wf, w32)
    assert_exact_bound(2.0 ** -4, (C, 256.0), (1, 256.0))
    y = bf16(o["x"] @ w32.T + b32)
    assert torch.equal(y[..., :C], o["qh"]) and torch.equal(y[..., C:2 * C], o["k"]) and torch.equal(y[..., 2 * C:], o["v"])


@pytest.mark.parametrize("B,L,C,regime", [c for c in CASES if c[1] <= 256])
def test_fp64_oracle_gives_the_mean(B, L, C, regime):
    """oracle GroupNorm -> to_q / to_k / to_v -> SDPA in fp64 equals the mean of V over S(i) to within 2^-20 relative (the other keys
    carry <= L 2^-24 of the weight), so its bf16 rounding is the exact reference."""
    o = selective_operands(B, L, C, regime, seed=8, fused=True)
    r = selective_reference(o["qh"], o["k"], o["v"], j=o["j"])
    x = o["x"].double().transpose(1, 2).unsqueeze(-1)                       # (B, C, L, 1)
    xn = ops.group_norm_silu(x, o["gamma"].double(), o["beta"].double(), o["groups"], o["eps"], silu=False)
    xn = xn[..., 0].transpose(1, 2)
    w, bb = o["wqkv"].double(), o["bqkv"].double()
    q, k, v = (F.linear(xn, w[i * C:(i + 1) * C], bb[i * C:(i + 1) * C]) for i in range(3))
    qh4, kh4, vh4 = (t.view(B, L, C // 8, 8).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh4, kh4, vh4).transpose(1, 2).reshape(B, L, C)
    assert float(((ref - r["out"]).abs() / r["out"].abs()).max()) < 2.0 ** -20
    assert torch.equal(bf16_rne(r["out"]), ref.to(torch.bfloat16).double())


def test_banded_tokens_sees_a_local_error():
    ref = torch.randn(4, 100, 64, generator=torch.Generator().manual_seed(0))
    assert_banded_rel_l2_tokens(ref * (1 + 1e-3), ref, 4e-3)
    for sl in ((slice(None), slice(96, 100)), (2, slice(None), slice(8, 16)), (slice(None), slice(0, 32))):
        z = ref.clone()
        z[sl] *= 1.02
        with pytest.raises(AssertionError):
            assert_banded_rel_l2_tokens(z, ref, 4e-3)
