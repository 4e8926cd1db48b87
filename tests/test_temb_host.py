"""CPU: the fp64 reference and the counted bound of the time-embedding table (rows_linear_kernel / launch_temb, csrc/elementwise.hip),
shared with tests/test_temb_gpu.py.

The table of a UNet: row r = every resnet's time_emb_proj(SiLU(emb_r)) side by side in the library's resnet order (down blocks, the
mid block's two, up blocks), emb_r = linear_2(SiLU(linear_1(sinusoid(t_r)))).  `temb_reference` evaluates that with
oracle.ops.timestep_embedding / oracle.unet.time_embedding on fp64 copies of the fp32 weights (the weights themselves are exact).

`temb_bound` is a per-element a-priori bound on |fp32 evaluation - fp64 reference|, counted, not fitted.  u = 2^-24; an fp32 rounding
is a relative error <= u; gamma_n = n u / (1 - n u); a function stated as E ulp accurate has a relative error <= E 2^-23 = 2 E u.
  sinusoid, column k (j = k mod half, half = K / 2, K = block_out_channels[0]):
      e = (c j) / (half - shift)   c = fp32(-ln 1e4), the product, the quotient: 3 roundings         |de| <= |e| ((1 + u)^3 - 1)
      f = expf(e)                  the argument's error through exp, then expf's own E_EXP ulp       rel_f = exp(|de|) (1 + 2 E_EXP u) - 1
      a = t f                      t is an integer < 2^24 (exact); one rounding                       |da| <= |a| ((1 + rel_f)(1 + u) - 1)
      x = sinf(a) or cosf(a)       |sin'|, |cos'| <= 1, then E_SIN ulp of the result                  dx = |da| + 2 E_SIN u (|x| + |da|)
  (the angle term dominates: at t = 999, j = 0 it is 999 (2 E_EXP + 1) u = 3e-4, a property of evaluating t f in fp32 at all.)
  a Linear stage y = b + sum_k w_k x_k over K inputs, any summation order, fused or separate multiply-add, given its computed inputs:
      s = gamma_(K+1) (sum |w| |x| + |b|)                                 (|x|: the reference's, plus the inputs' own bound)
  SiLU as the kernel evaluates it, v rcp(1 + exp2(-log2e v)) -- silu_f, csrc/common.h: the constant and the product (2 roundings
  of the exponent, |v| (2 u) after exp2), exp2 (E_EXP2 ulp), the sum, rcp (E_RCP ulp), the product:
      ev = rel_silu(|v|) |SiLU(v)|                                        (torch's fp32 v / (1 + exp(-v)) has fewer roundings)
Three stages: p1 = linear_1(x) (K inputs), h1 = SiLU(p1), p2 = linear_2(h1) (4 K), h2 = SiLU(p2), out = projections(h2) (4 K).

How the sources reach the output.  Stage by stage -- d_out = sum |w| d_in + s, with |SiLU'| <= 1.1 in between -- every stage multiplies
what it receives by the absolute row sum of its weights, about 20 for a 512-wide stage of these unit-variance weights, where the
signed map amplifies by about 1: that bound comes to 2e-2 .. 0.4 on a table whose entries are below 1.2, and no two rows could be
told apart by it.  So the sources are the ones above, but each is carried to the output through the SIGNED product of what lies
between, whose absolute value is taken once, at the end.  With D1 = diag SiLU'(p1), D2 = diag SiLU'(p2) of the row,
M = Wp D2 W2 and the expansion SiLU(v + d) = SiLU(v) + SiLU'(v) d + r, |r| <= d^2 / 4 (|SiLU''| <= 1/2):
      out^ - out = M D1 W1 dx_ + M (D1 rho1 + r1 + ev1) + Wp (D2 rho2 + r2 + ev2) + rho3,      |rho_i| <= s_i
      bound      = |M D1 W1| dx + |M| (|D1| s1 + r1 + ev1) + |Wp| (|D2| s2 + r2 + ev2) + s3
which is rigorous for the same model of arithmetic: the stage-by-stage bounds still size the second-order terms r1 = dp1^2 / 4
(dp1 = |W1| dx + s1) and the magnitudes the sources are relative to; r2 = dp2^2 / 4 uses the sharp dp2 = |W2 D1 W1| dx +
|W2| (|D1| s1 + r1 + ev1) + s2.  The result is 1e-4 .. 4e-3; its largest part is s2 through |Wp| |D2|, the worst-case summation
error of the 4 K-wide linear_2.

ASSUMED, not measured: E_EXP = E_SIN = E_EXP2 = E_RCP = 2 ulp.  The ROCm installation this was written against carries no document
that states the accuracy of expf / sinf / cosf or of the exp2 / rcp instructions (no ULP table under its share/ or include/ trees), so
each function is given 2 ulp.  The quotient of e counts as one rounding (hipcc's default: correctly rounded fp32 division).

Measured here on the CPU (torch's own fp32 evaluation of the same oracle, every case below): worst error / bound = 0.027 (K = 32,
(flip, shift) = (False, 1), n = 130, t = 929); 0.025 / 0.027 at K = 32, 0.006 - 0.007 at 96, 0.003 - 0.005 at 128 (both row counts),
0.003 at 160.  The distance is the worst-case summation term gamma_(4K+1) against errors that mostly cancel.  Row separation: the
closest pair of rows of a case (neighbouring timesteps, e.g. 742 / 741) differs by more than 4 x the bound on 98 % (K = 32), 91 %
(96), 81 - 86 % (128, both row counts) and 75 % (160) of the columns; the assertion asks for half.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet as o_unet
from rangeldm_amd.config import UNetConfig
from rangeldm_amd.params import unet_param_shapes
from rangeldm_amd.synth import synth_state_dict

U = 2.0 ** -24
E_EXP = E_SIN = E_EXP2 = E_RCP = 2          # ulp; assumed (module docstring)
SILU_LIP = 1.1                              # max |SiLU'| = 1.09984 (at v = 2.3994)

# block_out_channels[0] against the kernel's 128-wide K chunk: below one chunk; below, not a power of two; one chunk; a chunk and a tail.
# (rldm_unet_create takes multiples of 32 only, which all four are: no width had to be replaced.  It also means every Linear's output
# count -- 4 K, and the row length, a sum of block widths -- is a multiple of 16: the kernel's `o < O` guard of a ragged last 16-output
# block cannot be reached through a UNet and stays unexercised.)
WIDTHS = (32, 96, 128, 160)
SINUSOIDS = ((True, 0), (False, 1))         # (flip_sin_to_cos, freq_shift): diffusers' UNet2DModel, sgm's get_timestep_embedding
CONFIGS = [(k, flip, shift) for k in WIDTHS for flip, shift in SINUSOIDS]


def config_id(c):
    return f"K{c[0]}-{'flip' if c[1] else 'noflip'}-shift{c[2]}"


def temb_config(K, flip, shift):
    """A UNet that only needs to be created and finalized: two levels (K, 64) of one layer, no attention, a 4 x 2 sample.  Eight resnets
    of widths K, 64, 64, 64, 64, 64, K, K: the projections' column offsets are not multiples of one width."""
    return UNetConfig(sample_size=(4, 2), layers_per_block=1, block_out_channels=(K, 64), down_block_types=("DownBlock2D",) * 2,
                      up_block_types=("UpBlock2D",) * 2, add_attention=False, flip_sin_to_cos=flip, freq_shift=shift)


def temb_state_dict(cfg):
    K, (flip, shift) = cfg.block_out_channels[0], (cfg.flip_sin_to_cos, cfg.freq_shift)
    return synth_state_dict(unet_param_shapes(cfg), prefix=f"temb/{K}/{int(flip)}{shift}.")


def resnet_order(cfg):
    """resnet prefixes in the library's order (unet_build_layers, csrc/runtime.hip) with their widths."""
    boc, L = cfg.block_out_channels, len(cfg.block_out_channels)
    out = [(f"down_blocks.{i}.resnets.{j}", boc[i]) for i in range(L) for j in range(cfg.layers_per_block)]
    out += [("mid_block.resnets.0", boc[-1]), ("mid_block.resnets.1", boc[-1])]
    out += [(f"up_blocks.{i}.resnets.{j}", boc[L - 1 - i]) for i in range(L) for j in range(cfg.layers_per_block + 1)]
    return out


def timesteps_130():
    """130 distinct timesteps: 0, 1, 999 and 127 others, in no order (two passes of 64 rows and two rows of a third)."""
    rest = (torch.randperm(997, generator=torch.Generator().manual_seed(130)) + 2)[:127].tolist()
    ts = rest[:40] + [999] + rest[40:90] + [0] + rest[90:] + [1]
    assert len(ts) == 130 and len(set(ts)) == 130
    return ts


TS_1000 = list(range(999, -1, -1))
# (config, timesteps) of every comparison against the reference: all eight at n = 130, the 128-wide pair at n = 1000
CASES = [(c, "130") for c in CONFIGS] + [(c, "1000") for c in CONFIGS if c[0] == 128]


def case_id(case):
    return f"{config_id(case[0])}-n{case[1]}"


def case_timesteps(tag):
    return timesteps_130() if tag == "130" else TS_1000


def _table(sd, cfg, ts):
    """[n][ld] in sd's precision: the oracle's time embedding and every resnet's projection, in resnet order"""
    t = torch.tensor(ts, dtype=torch.long)
    emb = o_unet.time_embedding(sd, cfg, t, len(ts))
    h = F.silu(emb)
    return torch.cat([F.linear(h, sd[p + ".time_emb_proj.weight"], sd[p + ".time_emb_proj.bias"]) for p, _ in resnet_order(cfg)], 1)


def temb_reference(sd, cfg, ts):
    sd64 = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items() if "time_emb" in k}
    ref = _table(sd64, cfg, ts)
    assert ref.dtype == torch.float64
    return ref


def temb_oracle_fp32(sd, cfg, ts):
    sd32 = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if "time_emb" in k}
    out = _table(sd32, cfg, ts)
    assert out.dtype == torch.float32
    return out


def gamma(n):
    return n * U / (1 - n * U)


def _sum_source(w, b, x, dx):
    """s of a Linear stage: gamma_(K+1) (sum |w| (|x| + dx) + |b|), [n][O]"""
    return gamma(w.shape[1] + 1) * ((x.abs() + dx) @ w.abs().T + b.abs()[None, :])


def _silu_rel(m):
    """relative error of silu_f's evaluation at |v| <= m"""
    eps_e = torch.exp(m * ((1 + U) ** 2 - 1)) * (1 + 2 * E_EXP2 * U) - 1          # exp2(-log2e v)
    eps_s = (1 + eps_e) * (1 + U) - 1                                            # 1 + exp2(..): the sum inherits at most eps_e
    return (1 + eps_s / (1 - eps_s)) * (1 + 2 * E_RCP * U) * (1 + U) - 1          # rcp, the product with v


def _silu_prime(v):
    sg = torch.sigmoid(v)
    return sg * (1 + v * (1 - sg))


def temb_bound(sd, cfg, ts, chunk=32):
    """-> [n][ld] fp64: the module docstring's bound for every element of the table."""
    K, shift = cfg.block_out_channels[0], cfg.freq_shift
    half = K // 2
    w = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items() if "time_emb" in k}
    W1, b1 = w["time_embedding.linear_1.weight"], w["time_embedding.linear_1.bias"]
    W2, b2 = w["time_embedding.linear_2.weight"], w["time_embedding.linear_2.bias"]
    Wp = torch.cat([w[p + ".time_emb_proj.weight"] for p, _ in resnet_order(cfg)], 0)
    bp = torch.cat([w[p + ".time_emb_proj.bias"] for p, _ in resnet_order(cfg)], 0)
    t = torch.tensor(ts, dtype=torch.float64)
    assert float(t.max()) < 2 ** 24
    # ---- the sinusoid ----
    j = torch.arange(half, dtype=torch.float64)
    e = -math.log(10000.0) * j / (half - shift)
    rel_f = torch.exp(e.abs() * ((1 + U) ** 3 - 1)) * (1 + 2 * E_EXP * U) - 1
    a = t[:, None] * torch.exp(e)[None, :]
    da = a.abs() * ((1 + rel_f)[None, :] * (1 + U) - 1)
    s, c = torch.sin(a), torch.cos(a)
    x = torch.cat([c, s] if cfg.flip_sin_to_cos else [s, c], 1)
    dx = torch.cat([da, da], 1)
    dx = dx + 2 * E_SIN * U * (x.abs() + dx)
    # ---- the reference's intermediate values, the sources, the stage-by-stage bounds that size the second-order terms ----
    p1 = F.linear(x, W1, b1)
    h1 = F.silu(p1)
    p2 = F.linear(h1, W2, b2)
    h2 = F.silu(p2)
    D1, D2 = _silu_prime(p1), _silu_prime(p2)
    assert float(D1.abs().max()) <= SILU_LIP and float(D2.abs().max()) <= SILU_LIP
    s1 = _sum_source(W1, b1, x, dx)
    dp1 = dx @ W1.abs().T + s1
    ev1 = _silu_rel(p1.abs() + dp1) * (h1.abs() + SILU_LIP * dp1)
    r1 = dp1 * dp1 / 4
    dh1 = SILU_LIP * dp1 + ev1
    s2 = _sum_source(W2, b2, h1, dh1)
    v1 = D1.abs() * s1 + r1 + ev1                                  # what enters h1 beside D1 W1 dx_
    out = torch.empty((len(ts), Wp.shape[0]), dtype=torch.float64)
    for r0 in range(0, len(ts), chunk):
        sl = slice(r0, min(r0 + chunk, len(ts)))
        J1 = (W2[None, :, :] * D1[sl, None, :]) @ W1               # [rows][D][K]: W2 D1 W1
        dp2 = (J1.abs() @ dx[sl, :, None])[..., 0] + v1[sl] @ W2.abs().T + s2[sl]
        ev2 = _silu_rel(p2[sl].abs() + dp2) * (h2[sl].abs() + SILU_LIP * dp2)
        r2 = dp2 * dp2 / 4
        dh2 = SILU_LIP * dp2 + ev2
        s3 = _sum_source(Wp, bp, h2[sl], dh2)
        M = (Wp[None, :, :] * D2[sl, None, :]) @ W2                # [rows][ld][D]: Wp D2 W2
        A1 = (M * D1[sl, None, :]) @ W1                            # [rows][ld][K]: M D1 W1
        out[sl] = ((A1.abs() @ dx[sl, :, None])[..., 0] + (M.abs() @ v1[sl, :, None])[..., 0]
                   + (D2[sl].abs() * s2[sl] + r2 + ev2) @ Wp.abs().T + s3)
    return out


_CACHE = {}


def temb_case(case):
    """-> (cfg, sd, timesteps, fp64 reference, bound), computed once per case and left unchanged."""
    if case not in _CACHE:
        (K, flip, shift), tag = case
        cfg = temb_config(K, flip, shift)
        sd = temb_state_dict(cfg)
        ts = case_timesteps(tag)
        _CACHE[case] = (cfg, sd, ts, temb_reference(sd, cfg, ts), temb_bound(sd, cfg, ts))
    return _CACHE[case]


def worst_ratio(got, ref, bound):
    """-> (max |got - ref| / bound, its (row, column))"""
    r = (got.double() - ref).abs() / bound
    i = int(r.argmax())
    return float(r.flatten()[i]), divmod(i, r.shape[1])


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
def test_layout_of_the_cases():
    for c in CONFIGS:
        cfg = temb_config(*c)
        widths = [wd for _, wd in resnet_order(cfg)]
        assert widths == [c[0], 64, 64, 64, 64, 64, c[0], c[0]]
        shapes = unet_param_shapes(cfg)
        assert sorted(p for p, _ in resnet_order(cfg)) == sorted(k[:-len(".time_emb_proj.bias")] for k in shapes if k.endswith(".time_emb_proj.bias"))
        for p, wd in resnet_order(cfg):
            assert tuple(shapes[p + ".time_emb_proj.weight"]) == (wd, 4 * c[0])
    ts = timesteps_130()
    assert {0, 1, 999} <= set(ts) and ts == timesteps_130()
    assert TS_1000[0] == 999 and TS_1000[-1] == 0 and len(TS_1000) == 1000


def test_fp64_reference_is_the_fp32_oracle_in_higher_precision():
    """the dtype switch changes the precision and nothing else: fp64 and fp32 evaluations agree to fp32 accuracy, flip and shift reach both"""
    for c in ((32, True, 0), (32, False, 1)):
        cfg = temb_config(*c)
        sd = temb_state_dict(cfg)
        ts = [0, 1, 500, 999]
        ref, o32 = temb_reference(sd, cfg, ts), temb_oracle_fp32(sd, cfg, ts)
        assert ref.shape == o32.shape == (4, 3 * 32 + 5 * 64)
        assert float((ref - o32.double()).abs().max()) < 1e-4 * float(ref.abs().max())
    a = temb_reference(sd, temb_config(32, True, 0), ts)
    assert float((a - ref).abs().max()) > 1e-2                   # same weights, the other sinusoid: another table


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fp32_oracle_stays_inside_the_bound(case):
    cfg, sd, ts, ref, bound = temb_case(case)
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and float(bound.min()) > 0
    ratio, (r, col) = worst_ratio(temb_oracle_fp32(sd, cfg, ts), ref, bound)
    print(f"{case_id(case)}: fp32 oracle worst error / bound = {ratio:.3f} at row {r} (t = {ts[r]}) column {col}; "
          f"bound in [{float(bound.min()):.2e}, {float(bound.max()):.2e}], |ref| max {float(ref.abs().max()):.3f}")
    assert ratio <= 1.0, f"torch's fp32 evaluation leaves the bound ({ratio:.3f} x) at row {r} (t = {ts[r]}) column {col}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rows_of_distinct_timesteps_are_told_apart(case):
    """A row that holds another timestep's values cannot pass the comparison: every other row of the case is more than 4 x the bound away
    (both rows' bounds: the larger) on at least half of the columns."""
    cfg, sd, ts, ref, bound = temb_case(case)
    n, ld = ref.shape
    worst, pair = 1.0, None
    for i in range(n):
        far = (ref - ref[i][None, :]).abs() > 4 * torch.maximum(bound, bound[i][None, :])
        frac = far.double().mean(1)
        frac[i] = 1.0
        k = int(frac.argmin())
        if float(frac[k]) < worst:
            worst, pair = float(frac[k]), (ts[i], ts[k])
    print(f"{case_id(case)}: the closest pair of rows (timesteps {pair}) differs by > 4 x bound on {100 * worst:.1f} % of {ld} columns")
    assert worst >= 0.5, f"timesteps {pair}: only {100 * worst:.1f} % of the columns tell the rows apart"
