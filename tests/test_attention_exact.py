"""GPU: every attention route bit for bit on selective-softmax operands (tests/hip_util.py selective_operands).

Each query i gives one set S(i) of 2^j keys equal scores and every other key a score >= 32 log2 units lower (>= 160 for training,
where the backward needs exp2 to underflow to exactly 0).  The output is then the mean of V over S(i) on every route, in any tile
order and under either stabiliser (the first key tile's maximum or the running maximum), and that mean is exact in bf16.  Regimes:
R1 (S(i) in the first key tile), R2 (30..90 above its maximum: the fast path with P >> 1), R3 (>= 140 above it: only the overflow
fallback of attention_qkv2_d8_kernel can get it right), stair (tile maxima rise by 7.75 / 8.25 log2 units around the running-maximum
threshold; S(i) in the last, ragged tile).  The route each shape takes comes from rldm_test_attention_route, not from a copy of the
launch geometry."""
import ctypes as C

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from tests.hip_util import (RefCache, _ulps, assert_bitexact, assert_exact_bound, bf16_rne, hip_attention, hip_attention_qkv,
                            selective_operands, selective_reference)

pytestmark = pytest.mark.gpu
NAMES = ("image", "token", "channel")
_refs = RefCache(cap=16)


def route(B, L, Cc):
    r = (C.c_int * 6)()
    _lib.check(_lib.lib().rldm_test_attention_route(B, L, Cc, r), "rldm_test_attention_route")
    return dict(gen=r[0], pair=r[1], hg=r[2], waves=r[3], proj=r[4], seam=r[5])


def regimes(L, stair=True):
    return ["R1"] + (["R2", "R3"] if L > 32 else []) + (["stair"] if stair and L > 32 else [])


def case(B, L, Cc, regime, fused, seed=1, **kw):
    def make():
        o = selective_operands(B, L, Cc, regime, seed=seed, fused=fused, **kw)
        o["ref"] = selective_reference(o["qh"], o["k"], o["v"], j=o["j"])
        return o
    return _refs.get((B, L, Cc, regime, fused, seed, tuple(sorted(kw.items()))), make)


def check_operands(o, regime):
    r = o["ref"]
    assert float(r["gap"].min()) >= o["gap"]
    if regime == "R1":
        assert float(r["margin"].max()) == 0
    elif regime in ("R2", "R3"):
        m = r["margin"]
        assert float(m.min()) == float(m.max()) == o["margin"]
        assert (30 <= o["margin"] <= 90) if regime == "R2" else o["margin"] >= 140


# ---- inference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 8, 33, 100, 1024])
@pytest.mark.parametrize("Cc", [8, 64, 256])
def test_attention_d8_exact(L, Cc):
    """attention_d8_kernel (rldm_test_attention: the running-maximum loop of attention_tile on a given q / k / v)."""
    B = 2
    for regime in regimes(L):
        o = case(B, L, Cc, regime, False)
        check_operands(o, regime)
        qkv = torch.cat([o["q_infer"], o["k"], o["v"]], -1)
        out = hip_attention(qkv, Cc)
        assert_bitexact(out, bf16_rne(o["ref"]["out"]), NAMES, f"attention_d8 B{B} L{L} C{Cc} {regime}")


# (64, 64, 256) and (64, 32, 256) would take HG = 8, but qkv2 declines them (its LDS image exceeds 160 KiB): the first generation runs
FIRST_GEN = [(2, L, Cc) for Cc in (16, 32, 96) for L in (8, 100, 1000)] + [(64, 64, 256), (64, 32, 256)]
QKV2 = [(2, 256, 256), (2, 100, 64), (1, 48, 64), (2, 1024, 128), (2, 1000, 128), (16, 64, 256), (32, 64, 256), (128, 32, 128),
        (256, 64, 64)]


def _fused(B, L, Cc, regime, seed=1):
    o = case(B, L, Cc, regime, True, seed)
    check_operands(o, regime)
    out = hip_attention_qkv(o["x"], o["gamma"], o["beta"], o["wqkv"], o["bqkv"], groups=o["groups"], eps=o["eps"])
    assert_bitexact(out, bf16_rne(o["ref"]["out"]), NAMES, f"attention_qkv B{B} L{L} C{Cc} {regime}")


@pytest.mark.parametrize("B,L,Cc", FIRST_GEN)
def test_attention_qkv_first_generation_exact(B, L, Cc):
    assert route(B, L, Cc)["gen"] == 1
    for regime in regimes(L, stair=Cc >= 32):
        _fused(B, L, Cc, regime)


@pytest.mark.parametrize("B,L,Cc", QKV2)
def test_attention_qkv2_exact(B, L, Cc):
    """attention_qkv2_d8_kernel: PAIR = 1 for L > 992, HG > 1 at large batch x heads; R3 is right only if the fallback ran."""
    r = route(B, L, Cc)
    assert r["gen"] == 2 and r["pair"] == (1 if L > 992 else 0), r
    for regime in regimes(L):
        _fused(B, L, Cc, regime)


def test_attention_qkv2_routes_reach_every_heads_per_workgroup():
    """HG = 1, 2, 4, 8 and PAIR = 1 all occur in QKV2 (and R3 runs under PAIR = 1 and under HG > 1 there, L > 32)."""
    rs = {s: route(*s) for s in QKV2}
    assert {r["hg"] for r in rs.values()} == {1, 2, 4, 8}, rs
    assert any(r["pair"] for r in rs.values()) and any(r["hg"] > 1 and s[1] > 32 for s, r in rs.items())
    assert rs[(16, 64, 256)]["hg"] == 2 and rs[(32, 64, 256)]["hg"] == 4 and rs[(256, 64, 64)]["hg"] == 8


# ---- the block: attention + output projection -----------------------------------------------------------------------------------------
def _block_shapes():
    out = []
    for Cc in (64, 128, 256):
        for L in (64, 128, 256, 512, 1024):
            for B in (1, 2, 4, 8, 16, 32):
                if route(B, L, Cc)["proj"]:
                    out.append((B, L, Cc))
    return out


def hip_attention_block(o, wout, bout, mode):
    dev = torch.device("cuda")
    B, L, Cc = o["x"].shape
    xs = o["x"].to(dev).contiguous()
    y = torch.empty((B, L, Cc), device=dev)
    st = torch.empty((B, L // 64, Cc, 2), device=dev)
    host = [np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (o["gamma"], o["beta"], o["wqkv"], o["bqkv"], wout, bout)]
    ptr = [h.ctypes.data_as(C.c_void_p) for h in host]
    _lib.check(_lib.lib().rldm_test_attention_block(C.c_void_p(xs.data_ptr()), B, L, Cc, o["groups"], o["eps"], *ptr, mode,
                                                    C.c_void_p(y.data_ptr()), C.c_void_p(st.data_ptr()), _lib.stream_ptr(dev)),
               f"rldm_test_attention_block mode {mode}")
    torch.cuda.synchronize()
    return y.cpu(), st.cpu()


def test_attention_block_exact_in_every_form():
    """y = x + to_out(attention) and y's statistics partials: the tail as its own launch (0), behind the seam (1, where every
    workgroup is resident), the regular conv (2).  to_out has two +-1 entries per row and a bias on the 1/8 grid, so y is exact in
    fp32 and rounded once; the partials are exact fp32 sums of bf16(y) and its squares."""
    shapes = _block_shapes()
    assert {(8, 1024, 128), (16, 1024, 128), (8, 512, 64)} <= set(shapes), shapes
    for B, L, Cc in shapes:
        r = route(B, L, Cc)
        g = torch.Generator().manual_seed(B * L + Cc)
        wout = torch.zeros(Cc, Cc)
        for row in range(Cc):
            cols = torch.randperm(Cc, generator=g)[:2]
            wout[row, cols] = (torch.randint(0, 2, (2,), generator=g) * 2 - 1).float()
        bout = torch.randint(-8, 9, (Cc,), generator=g).float() / 8
        for regime in ("R1", "R3"):
            o = case(B, L, Cc, regime, True)
            mean = bf16_rne(o["ref"]["out"]).double()
            assert_exact_bound(2.0 ** -3, (2, 7.0), (1, 1.0), (1, 1.0))
            yref = bf16_rne(o["x"].double() + bout.double() + mean @ wout.double().T)
            blocks = yref.view(B, L // 64, 64, Cc)
            sref = torch.stack([blocks.sum(2), (blocks * blocks).sum(2)], -1)
            assert_exact_bound(2.0 ** -6, (64, float(yref.abs().max()) ** 2))
            got = {}
            for mode in (0, 1, 2):
                if mode == 1 and not r["seam"]:
                    continue
                y, st = hip_attention_block(o, wout, bout, mode)
                what = f"attention block B{B} L{L} C{Cc} {regime} mode {mode}"
                assert_bitexact(y, yref, NAMES, what)
                if mode < 2:
                    assert_bitexact(st, sref, ("image", "block", "channel", "kind"), what + " stats")
                else:
                    tot = torch.zeros_like(sref)
                    tot[:, 0] = sref.sum(1)
                    assert_bitexact(st, tot, ("image", "block", "channel", "kind"), what + " stats (totals)")
                got[mode] = y
            for mode in got:
                assert torch.equal(got[mode], got[0])


# ---- training -----------------------------------------------------------------------------------------------------------------------
K_SCALE, K_LN2 = np.float32(0.35355339059327373), np.float32(0.6931471805599453)
TRAIN = [(2, L, Cc) for L in (1, 4, 31, 33, 200, 1024) for Cc in (8, 64, 256)]


def _train_reference(o, dO):
    """o (exact: P = 1 on S(i) once the maximum is the selected score, so the denominator is 2^j and inv = 2^-j exactly),
    lse (fp64), and the exact accumulators of dq (sum dS k), dk (sum dS qh) and dv (sum P dO) per head; dS = 2^-j dO_d (v_d - mean_d)
    with dO one-hot per (token, head) is exact in bf16, so every sum below is exact in fp32."""
    qh, k, v = o["qh"], o["k"], o["v"]
    B, L, Cc = qh.shape
    H = Cc // 8
    mean = o["ref"]["out"].float()
    acc = {n: torch.zeros(B, L, Cc) for n in ("dq", "dk", "dv")}
    for b in range(B):
        q4, k4, v4, d4, m4 = (t[b].view(L, H, 8).transpose(0, 1) for t in (qh, k, v, dO, mean))
        s = q4 @ k4.transpose(-1, -2)
        sel = (s == s.amax(-1, keepdim=True)).float()
        P = sel / sel.sum(-1, keepdim=True)
        dP = d4 @ v4.transpose(-1, -2)
        delta = (d4 * m4).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        assert torch.equal(dS.to(torch.bfloat16).float(), dS)
        # every sum below: multiples of 2^-8 (dS: 2^-6, qh: 2^-2, k: integers, P dO: 2^-3), exact while its |terms| stay < 2^24 units
        for bound in (dS.abs() @ k4.abs(), dS.abs().transpose(-1, -2) @ q4.abs(), P.transpose(-1, -2) @ d4.abs()):
            assert_exact_bound(2.0 ** -8, (1, float(bound.max())))
        for n, t in (("dq", dS @ k4), ("dk", dS.transpose(-1, -2) @ q4), ("dv", P.transpose(-1, -2) @ d4)):
            acc[n][b] = t.transpose(0, 1).reshape(L, Cc)
    lse = (o["ref"]["smax"] + o["j"]) * np.log(2.0)                    # (B, H, L), log2 units -> natural
    return mean, lse, acc


def _one_hot_dO(B, L, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    dO = torch.zeros(B, L, Cc // 8, 8)
    idx = torch.randint(0, 8, (B, L, Cc // 8, 1), generator=g)
    val = (torch.randint(0, 2, idx.shape, generator=g) * 2 - 1).float() * 2.0 ** torch.randint(0, 2, idx.shape, generator=g).float()
    return dO.scatter_(-1, idx, val).view(B, L, Cc)


@pytest.mark.parametrize("B,L,Cc", TRAIN)
def test_train_attention_exact(B, L, Cc):
    """train_attn.hip forward / backward through the stride-C and the packed [B][L][3C] entry points.  o and dv exact; dq and dk
    exact up to their one final fp32 multiply (kScale, kLn2), which the reference repeats in fp32; lse within 2 fp32 ulps of the
    fp64 (selected score + j) ln 2 (the kernel rounds m + log2(2^j) and the product by ln 2)."""
    from rangeldm_amd import train_ops as T
    for regime in (["R1", "R3", "stair"] if L > 32 else ["R1"]):
        kw = dict(alpha=96.0, gap=160) if regime != "R3" else dict(alpha=96.0, gap=160, margin=200)
        o = case(B, L, Cc, regime, False, seed=2, **kw)
        assert float(o["ref"]["gap"].min()) >= 160
        dO = _one_hot_dO(B, L, Cc, seed=L + Cc)
        mean, lse_ref, acc = _train_reference(o, dO)
        what = f"train attention B{B} L{L} C{Cc} {regime}"
        dq_ref = acc["dq"] * torch.tensor(K_SCALE)
        dk_ref = acc["dk"] * torch.tensor(K_LN2)
        q, k, v = (t.cuda() for t in (o["q_train"], o["k"], o["v"]))
        out, lse = T.attention_forward(q, k, v)
        dq, dk, dv = T.attention_backward(q, k, v, out, dO.cuda(), lse)
        assert_bitexact(out, mean, NAMES, what + " o")
        assert _ulps(lse.cpu(), lse_ref) <= 2, what + " lse"
        assert_bitexact(dv, acc["dv"], NAMES, what + " dv")
        assert_bitexact(dq, dq_ref, NAMES, what + " dq")
        assert_bitexact(dk, dk_ref, NAMES, what + " dk")
        # packed entry points: the same operands as thirds of one [B][L][3C] tensor, every column of dqkv written
        qkv = torch.cat([q, k, v], -1).contiguous()
        o2, lse2 = T.attention_qkv_forward(qkv)
        assert torch.equal(o2, out) and torch.equal(lse2, lse), what + " packed forward"
        dqkv = torch.full_like(qkv, float("nan"))
        delta = torch.empty_like(lse2)
        p = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().rldm_train_attention_qkv_backward(p(qkv), p(o2), p(dO.cuda().contiguous()), p(lse2), B, L, Cc, p(delta),
                                                                p(dqkv), _lib.stream_ptr(qkv.device)), "rldm_train_attention_qkv_backward")
        torch.cuda.synchronize()
        for n, part, ref in (("dq", dqkv[..., :Cc], dq), ("dk", dqkv[..., Cc:2 * Cc], dk), ("dv", dqkv[..., 2 * Cc:], dv)):
            assert_bitexact(part, ref, NAMES, what + f" packed {n}")
