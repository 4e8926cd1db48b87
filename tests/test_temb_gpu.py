"""GPU: the time-embedding table (rows_linear_kernel / launch_temb, csrc/elementwise.hip) on its own, through rldm_test_temb -- the
conversion and the call rldm_unet_forward (1 or B rows) and the samplers (num_steps rows) make.

A workgroup owns 16 outputs and walks the rows in passes of 64, restaging its LDS tiles every pass.  Up to here the suite ran at most 50
rows through it and saw it only behind whole-network relative-L2 gates.  Three checks:
  * rows are independent, bit for bit: row i of an n-row table is the 1-row table of its timestep, for n either side of one and two
    passes and for the 1000 rows of a DDPM sampler (second and later passes, the r0 + r offset, a later pass's tail guard, the barrier
    in front of the restaging);
  * every element is within tests/test_temb_host.py's counted bound of the fp64 reference, for block_out_channels[0] below, at and
    above the 128-wide K chunk and both sinusoid conventions (flip_sin_to_cos, freq_shift; the three Linear stages; the column
    offsets of the projections);
  * a forward with per-sample timesteps and B = 130 reads row b for sample b.

Measured on an MI355X (first run), worst |table - reference| / bound per case:
    K = 32: 0.024 (flip, shift 0) / 0.027 (no flip, shift 1)      K = 96: 0.0066 / 0.0064      K = 128: 0.0041 / 0.0039
    K = 160: 0.0034 / 0.0031      K = 128 at n = 1000: 0.0044 / 0.0045
the same figures as torch's fp32 evaluation on the CPU (0.003 .. 0.027): the bound's largest part is the worst-case summation term
of the 4 K-wide linear_2, which real roundings stay far below.  A wrong row, a swapped sinusoid or a shifted column is off by 4 x
the bound or more on most columns (tests/test_temb_host.py asserts that for rows).
The bound's assumed constants (2 ulp per function) are stated, and marked as assumed, in tests/test_temb_host.py."""
import pytest
import torch

from rangeldm_amd.config import UNetConfig
from rangeldm_amd.params import unet_param_shapes
from rangeldm_amd.synth import normal, synth_state_dict
from tests.hip_util import hip_temb, hip_temb_layout
from tests.test_temb_host import (CASES, CONFIGS, TS_1000, case_id, config_id, resnet_order, temb_case, temb_config, temb_state_dict,
                                  worst_ratio)

pytestmark = pytest.mark.gpu
ROW_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129)
_MODELS = {}


def _model(config):
    """-> (finalized UNet2DModelHIP, ld, {resnet prefix: column}, {timestep: its 1-row table}) of a (K, flip, shift)"""
    from rangeldm_amd.unet import UNet2DModelHIP
    if config not in _MODELS:
        cfg = temb_config(*config)
        m = UNet2DModelHIP(cfg)
        m.load_state_dict(temb_state_dict(cfg))
        ld, offs = hip_temb_layout(m)
        _MODELS[config] = (m, ld, offs, {})
    return _MODELS[config]


def _single(config, t):
    m, ld, _, rows = _model(config)
    if t not in rows:
        rows[t] = hip_temb(m, [t], ld)[0]
    return rows[t]


def _timesteps(n):
    """n timesteps that start 999, 0, 1 and go on without order; 500 stands at 3, 4, 66 and 128: a repeat inside the first pass, one in
    the second and one in the third"""
    g = torch.Generator().manual_seed(7)
    ts = [999, 0, 1, 500, 500] + [t if t != 500 else 501 for t in torch.randint(0, 1000, (124,), generator=g).tolist()]
    ts[66] = ts[128] = 500
    return ts[:n]


def _assert_rows(config, ts, what):
    m, ld, _, _ = _model(config)
    tab = hip_temb(m, ts, ld)
    assert tab.shape == (len(ts), ld) and torch.isfinite(tab).all(), what
    want = torch.stack([_single(config, t) for t in ts])
    bad = (tab.view(torch.int32) != want.view(torch.int32)).any(1).nonzero().flatten().tolist()
    assert not bad, (f"{what}: {len(bad)} of {len(ts)} rows differ from the 1-row table of their timestep; first rows {bad[:8]} "
                     f"(timesteps {[ts[i] for i in bad[:8]]})")
    return tab


@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_layout_is_the_resnet_order(config):
    _, ld, offs, _ = _model(config)
    want, col = {}, 0
    for p, width in resnet_order(temb_config(*config)):
        want[p] = col
        col += width
    assert offs == want and list(offs) == list(want) and ld == col


@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_row_i_of_an_n_row_table_is_the_one_row_table_of_its_timestep(config):
    for n in ROW_COUNTS:
        ts = _timesteps(n)
        assert len(ts) == n and (n < 3 or {0, 1, 999} <= set(ts))
        tab = _assert_rows(config, ts, f"{config_id(config)} n = {n}")
        rep = [i for i, t in enumerate(ts) if t == 500]
        assert n < 129 or rep == [3, 4, 66, 128]
        for i in rep[1:]:
            assert torch.equal(tab[i].view(torch.int32), tab[rep[0]].view(torch.int32)), f"n = {n}: rows {rep[0]} and {i} hold timestep 500 and differ"
    # two different timesteps do give two different rows (the 1-row tables are not one constant)
    assert not torch.equal(_single(config, 0), _single(config, 1)) and not torch.equal(_single(config, 999), _single(config, 998))


@pytest.mark.parametrize("config", [c for c in CONFIGS if c[1]], ids=config_id)
def test_the_1000_rows_of_a_ddpm_sampler_are_the_one_row_tables(config):
    """999 .. 0, as a 1000-step sampler builds its table: 16 passes, the last of 40 rows"""
    _assert_rows(config, TS_1000, f"{config_id(config)} n = 1000")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_table_within_the_counted_bound_of_the_fp64_reference(case):
    cfg, sd, ts, ref, bound = temb_case(case)
    m, ld, _, _ = _model(case[0])
    tab = hip_temb(m, ts, ld)
    assert tab.shape == ref.shape and torch.isfinite(tab).all()
    ratio, (r, col) = worst_ratio(tab, ref, bound)
    print(f"{case_id(case)}: worst |table - reference| / bound = {ratio:.4f} at row {r} (t = {ts[r]}) column {col}")
    over = int(((tab.double() - ref).abs() > bound).sum())
    assert over == 0, (f"{case_id(case)}: {over} of {tab.numel()} elements leave the bound; worst {ratio:.3g} x at row {r} (t = {ts[r]}) "
                       f"column {col}: {float(tab[r, col])} against {float(ref[r, col])}")


SMALL = dict(sample_size=(64, 8), block_out_channels=(32, 32, 64, 64))


def test_per_sample_timesteps_past_one_pass_read_their_own_row():
    """B = 130 distinct per-sample timesteps: sample b of that forward against sample b of the same-batch forward with the scalar
    timestep ts[b] -- the same plan and kernels, only the row of the table that the convs add differs (row b of 130 against row 0 of 1)."""
    from rangeldm_amd.unet import UNet2DModelHIP
    cfg = UNetConfig(**SMALL)
    m = UNet2DModelHIP(cfg)
    m.load_state_dict(synth_state_dict(unet_param_shapes(cfg), prefix="temb/small."))
    B = 130
    ts = (torch.randperm(997, generator=torch.Generator().manual_seed(131))[:B] + 2).tolist()
    ts[0], ts[64], ts[129] = 999, 0, 1
    assert len(set(ts)) == B
    x = torch.from_numpy(normal(5, "temb/small/x", (B, cfg.in_channels, *cfg.sample_size))).cuda()
    per = m(x, torch.tensor(ts)).sample.cpu()
    assert torch.isfinite(per).all()
    outs = {}
    for b in (0, 63, 64, 65, 129):
        outs[b] = m(x, ts[b]).sample.cpu()
        assert torch.equal(per[b], outs[b][b]), f"sample {b} (timestep {ts[b]}) of the per-sample forward is not the scalar-timestep forward's"
    assert not torch.equal(outs[0][63], outs[63][63])          # (the timestep does reach the output)
