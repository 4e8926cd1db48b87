"""GPU parity, model level: UNet2DModelHIP / AutoencoderKLHIP / schedulers / pipelines (through the C ABI) against the
CPU oracle and the golden vectors captured from the reference's own modules (tests/golden, see
oracle/validate_against_reference.py).

Tolerances: bf16 storage + fp32 accumulation => rel-L2 <= 2e-2 per network forward (teacher-forced)
and per decoded image of a free-running trajectory with injected noise; <= 1e-2 on the final latent x_0 of the full 50-step
full-width sampler (measured on MI355X: 1.9e-3 DDIM, 2.4e-3 strided DDPM; decoded image 7e-3); fp32 elementwise kernels <= 1e-6."""
import numpy as np
import pytest
import torch

from rangeldm_amd.config import UNetConfig, VAEConfig
from rangeldm_amd._lib import Flag, Flag2
from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
from rangeldm_amd.synth import synth_state_dict, normal
from oracle import unet as o_unet, vae as o_vae, schedulers as o_sched, pipelines as o_pipe
from tests.hip_util import rel_l2

pytestmark = pytest.mark.gpu
TOL_FWD = 1.2e-2     # one network forward, teacher-forced (round 4: 2e-2 -> 1.2e-2; measured 4-8e-3, so a regression that doubles the error fails)
TOL_TRAJ = 2e-2      # decoded image at the end of a free-running trajectory
TOL_X0 = 5e-3        # final latent of the 50-step full-width sampler (round 4: 1e-2 -> 5e-3; measured 1.9-2.4e-3)


def T(a):
    return torch.from_numpy(np.asarray(a))


def hip_unet(cfg, prefix):
    from rangeldm_amd.unet import UNet2DModelHIP
    sd = synth_state_dict(unet_param_shapes(cfg), prefix=prefix)
    m = UNet2DModelHIP(cfg)
    m.load_state_dict(sd)
    return m, sd


_VAE = {}


def hip_vae():
    from rangeldm_amd.vae import AutoencoderKLHIP
    if "m" not in _VAE:
        cfg = VAEConfig()
        sd = synth_state_dict(vae_param_shapes(cfg), prefix="vae.")
        m = AutoencoderKLHIP(cfg)
        m.load_state_dict(sd)
        _VAE["m"], _VAE["sd"], _VAE["cfg"] = m, sd, cfg
    return _VAE["m"], _VAE["sd"], _VAE["cfg"]


SMALL = dict(sample_size=(64, 8), block_out_channels=(32, 32, 64, 64))


@pytest.mark.parametrize("kw,B", [
    (dict(**SMALL), 2),
    (dict(**SMALL, in_channels=12), 1),                                   # upsample config channels
    (dict(sample_size=(128, 8), block_out_channels=(32, 32, 64, 64)), 3),  # nuScenes-like aspect, odd batch
    (dict(sample_size=(128, 32), in_channels=3, out_channels=2, block_out_channels=(32, 32, 64, 64, 96, 96),
          down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
          up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4), 1),   # RangeDM topology
])
def test_unet_forward_small(kw, B):
    cfg = UNetConfig(**kw)
    m, sd = hip_unet(cfg, "t.")
    x = T(normal(3, "x", (B, cfg.in_channels, *cfg.sample_size)))
    ref = o_unet.OracleUNet(cfg, sd)(x, 480).sample
    out = m(x.cuda(), 480).sample.cpu()
    assert out.shape == ref.shape
    assert rel_l2(out, ref) < TOL_FWD
    # 0-d tensor timestep (what `for t in scheduler.timesteps` yields) and per-sample timesteps (training path)
    out0 = m(x.cuda(), torch.tensor(480)).sample.cpu()
    assert torch.equal(out0, out)
    ts = torch.tensor([(37 * (i + 1)) % 1000 for i in range(B)])
    ref_ps = o_unet.OracleUNet(cfg, sd)(x, ts).sample
    assert rel_l2(m(x.cuda(), ts).sample.cpu(), ref_ps) < TOL_FWD


@pytest.mark.parametrize("size,B", [((32, 4), 2), ((64, 8), 1)])
def test_wide_concatenation_runs_half_by_half(size, B):
    """RangeDM's 512-channel levels concatenate to 1024 input channels (ldm/configs/RangeDM.yaml:19-21), more than conv_small.hip's LDS
    tile takes: the resnet runs as gn_apply (two outputs) + conv1 in two halves + conv2 (+ the shortcut as one or two pointwise convs),
    NetCommon::resnet_wide.  A two-level 512-channel UNet exercises both forms -- (64, 8): the 64-pixel tiles of the 512-pixel level, where
    the 3x3 tile and the shortcut's tile do not fit the LDS together -- against the oracle, and against the same network on the generic
    kernel (rldm_debug_set_flags(Flag.NO_WIDE_SPLIT))."""
    from rangeldm_amd import _lib
    cfg = UNetConfig(sample_size=size, block_out_channels=(512, 512), down_block_types=("DownBlock2D", "AttnDownBlock2D"),
                     up_block_types=("AttnUpBlock2D", "UpBlock2D"))
    x = T(normal(17, "x", (B, cfg.in_channels, *cfg.sample_size)))
    outs, launches = [], []
    for flags in (0, Flag.NO_WIDE_SPLIT):
        _lib.lib().rldm_debug_set_flags(flags)
        try:
            m, sd = hip_unet(cfg, "wide.")
            outs.append(m(x.cuda(), 321).sample.cpu())
            launches.append(m.num_launches(B))
        finally:
            _lib.lib().rldm_debug_set_flags(0)
    ref = o_unet.OracleUNet(cfg, sd)(x, 321).sample
    print(f"wide concat {size}: split {float(rel_l2(outs[0], ref)):.3e} generic {float(rel_l2(outs[1], ref)):.3e}, launches {launches}")
    assert launches[0] > launches[1]                          # (the split is in force: more, cheaper launches)
    assert rel_l2(outs[0], ref) < TOL_FWD and rel_l2(outs[1], ref) < TOL_FWD
    assert rel_l2(outs[0], outs[1]) < TOL_FWD / 2


@pytest.mark.parametrize("B", [8, 16])
def test_fused_attention_projection_matches_separate_launch(B):
    """The 1024-token attention launch carries the block's output projection (+ x, + GroupNorm statistics) behind a cluster seam
    (attention_proj_tail); rldm_debug_set_flags(Flag.ATTN_PROJ_LAUNCH) keeps the projection a conv_small launch, NO_PERSISTENT runs
    the SAME tail as a launch of its own (identical bits).  All three against the oracle."""
    from rangeldm_amd import _lib
    cfg = UNetConfig()
    x = T(normal(19, "x", (B, cfg.in_channels, *cfg.sample_size)))
    outs, launches = {}, {}
    for flags in (0, Flag.ATTN_PROJ_LAUNCH, Flag.NO_PERSISTENT):
        _lib.lib().rldm_debug_set_flags(flags)
        try:
            m, sd = hip_unet(cfg, "fp.")
            outs[flags] = m(x.cuda(), 450).sample.cpu()
            launches[flags] = m.num_launches(B)
            assert m.trunk_status(B) == 0
        finally:
            _lib.lib().rldm_debug_set_flags(0)
    ref = o_unet.OracleUNet(cfg, sd)(x[:2], 450).sample
    assert launches[0] == launches[Flag.ATTN_PROJ_LAUNCH] - 5          # five attention blocks at 1024 tokens
    assert torch.equal(outs[0], outs[Flag.NO_PERSISTENT])
    assert rel_l2(outs[0][:2], ref) < TOL_FWD and rel_l2(outs[Flag.ATTN_PROJ_LAUNCH][:2], ref) < TOL_FWD
    assert rel_l2(outs[0], outs[Flag.ATTN_PROJ_LAUNCH]) < TOL_FWD / 2


def test_unet_forward_nuscenes_config():
    """BASELINE config 3 (ldm/configs/nuscenes.yaml: 256 x 8 latents, full channel widths): its lowest level has 32 x 1 images,
    which run on conv_small.hip's 32-pixel tiles (3x3 over 256 / 512 channels and the attention output projection)."""
    cfg = UNetConfig(sample_size=(256, 8))
    m, sd = hip_unet(cfg, "nu.")
    x = T(normal(5, "x", (2, cfg.in_channels, *cfg.sample_size)))
    ref = o_unet.OracleUNet(cfg, sd)(x, 333).sample
    out = m(x.cuda(), 333).sample.cpu()
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert rel_l2(out, ref) < TOL_FWD


def test_unet_forward_full_config_golden(golden):
    """RangeLDM KITTI-360 config (30.1 M params, 256x16 latents) against the committed oracle output."""
    g = golden("unet")
    cfg = UNetConfig()
    m, _ = hip_unet(cfg, "")
    out = m(T(g["unet_x"]).cuda(), int(g["unet_t"][0])).sample.cpu()
    assert rel_l2(out, T(g["unet_eps_oracle"])) < TOL_FWD
    assert abs(m.flops(1) / 1e9 - 34.071) < 0.35          # 34.071 GFLOP per sample-forward


@pytest.mark.parametrize("size", [(256, 16), (256, 8)])
def test_producer_side_groupnorm_matches_consumer_side(size):
    """Producer-side GroupNorm (conv_small.hip epilogue: a conv whose tile owns a whole <= 64-pixel image writes the normalised +
    activated copies its consumers read) against the same network with every GroupNorm applied by the consumer
    (rldm_debug_set_flags(Flag.CONSUMER_GN)): the arithmetic is the same, only the summation split of the statistics (one 64-pixel tile
    against two 32-pixel tiles) differs, and a last-bit change of a scale flips bf16 roundings downstream -- so the two forwards differ by about what either differs from the oracle."""
    from rangeldm_amd import _lib
    cfg = UNetConfig(sample_size=size)
    x = T(normal(11, "x", (2, cfg.in_channels, *cfg.sample_size))).cuda()
    outs = []
    for flags in (0, Flag.CONSUMER_GN):
        _lib.lib().rldm_debug_set_flags(flags)
        try:
            m, _ = hip_unet(cfg, "ps.")
            outs.append((m(x, 250).sample.cpu(), m.num_launches(2) if hasattr(m, "num_launches") else None))
            assert m.trunk_status(2) == 0
        finally:
            _lib.lib().rldm_debug_set_flags(0)
    assert torch.isfinite(outs[0][0]).all()
    d = rel_l2(outs[0][0], outs[1][0])
    print("producer- vs consumer-side GroupNorm: rel-L2", float(d))
    assert d < TOL_FWD / 2
    if outs[0][1] is not None:
        assert outs[0][1] < outs[1][1]                     # the separate gn_apply launches in front of the up-block convs are gone


@pytest.mark.parametrize("B,size", [(2, (256, 16)), (16, (256, 16)), (13, (256, 16)), (5, (256, 16)), (4, (256, 8)), (9, (256, 8))])
def test_persistent_trunk_matches_separate_launches(B, size):
    """The persistent trunk launch (trunk.hip: the convs of the 32x2 level and the mid block as phases of one launch, the channel
    tiles of an image handing over through their XCD's L2; from 13 images on also the 64x4 level as multi-tile clusters -- 4 pixel
    tiles x 4 channel tiles per image, GroupNorm folds and gn_apply as phases) against the same plan as separate launches
    (rldm_debug_set_flags(Flag.NO_PERSISTENT)): the SAME kernels' code on the SAME operands in the same order, so the outputs are identical,
    and repeated forwards (the cluster counters re-arm themselves) stay identical."""
    from rangeldm_amd import _lib
    cfg = UNetConfig(sample_size=size)              # (256, 8): the nuScenes network, whose lowest level has 32 x 1 images
    x = T(normal(13, "x", (B, cfg.in_channels, *cfg.sample_size))).cuda()
    outs, launches = [], []
    for flags in (0, Flag.NO_PERSISTENT):
        _lib.lib().rldm_debug_set_flags(flags)
        try:
            m, _ = hip_unet(cfg, "tk.")
            o1 = m(x, 250).sample.cpu()
            o2 = m(x, 250).sample.cpu()
            o3 = m(x, 731).sample.cpu()
            assert m.trunk_status(B) == 0
            assert torch.equal(o1, o2)
            outs.append((o1, o3))
            launches.append(m.num_launches(B))
        finally:
            _lib.lib().rldm_debug_set_flags(0)
    assert launches[0] < launches[1]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("B,size", [(16, (256, 16)), (24, (256, 8))])      # (24 x 16 tiles = 384 workgroups: where the 8-beam level takes the 4-wave instance)
def test_full_height_tiles_in_and_out_of_the_persistent_launch(B, size):
    """conv_stream's tiles as tall as the image (8 x 16 on 16-beam levels, 16 x 8 on 8-beam ones: the halo rows above / below are never
    staged) against the 16 x 8 tiles with a staged halo ring (rldm_debug_set_flags2(Flag2.HALO_RING)), each as phases of the persistent launch
    and as launches of their own (rldm_debug_set_flags(Flag.NO_PERSISTENT)).  The kernel picks its instance from the phase record, not
    from the tile's shape: a 16 x 8 tile on an 8-beam level is BOTH shapes."""
    from rangeldm_amd import _lib
    cfg = UNetConfig(sample_size=size)
    x = T(normal(17, "x", (B, cfg.in_channels, *cfg.sample_size))).cuda()
    outs = {}
    for f2 in (0, Flag2.HALO_RING):
        for f1 in (0, Flag.NO_PERSISTENT):
            _lib.lib().rldm_debug_set_flags(f1)
            _lib.lib().rldm_debug_set_flags2(f2)
            try:
                m, _ = hip_unet(cfg, "fh.")
                o = m(x, 411).sample.cpu()
                assert m.trunk_status(B) == 0
                assert torch.isfinite(o).all()
                outs[(f2, f1)] = o
            finally:
                _lib.lib().rldm_debug_set_flags(0)
                _lib.lib().rldm_debug_set_flags2(0)
    for f2 in (0, Flag2.HALO_RING):
        assert torch.equal(outs[(f2, 0)], outs[(f2, Flag.NO_PERSISTENT)])
    # two tilings of the same sums: the statistics partials are grouped differently, nothing else (bf16 roundings flip and travel through
    # the network: measured 2.6e-3; the same bound as the other plan variants)
    assert rel_l2(outs[(0, 0)], outs[(Flag2.HALO_RING, 0)]) < TOL_FWD / 2


def test_unet_errors():
    cfg = UNetConfig(**SMALL)
    from rangeldm_amd.unet import UNet2DModelHIP
    m = UNet2DModelHIP(cfg)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 5, 64, 8).cuda(), 0)                # weights not loaded
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="t.")
    bad = dict(sd)
    bad.pop("conv_in.weight")
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad)
    m.load_state_dict(sd)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 4, 64, 8).cuda(), 0)                # wrong channel count


def test_vae_matches_reference_goldens(golden):
    """decode / encode against outputs of the reference's own sgm Decoder / Encoder (tests/golden/vae.npz)."""
    g = golden("vae")
    m, sd, cfg = hip_vae()
    img = m.decode(T(g["vae_z"]).cuda()).sample.cpu()
    assert rel_l2(img, T(g["vae_image_ref"])) < TOL_FWD
    mom = m.encode(T(g["vae_x"]).cuda()).latent_dist.parameters.cpu()
    assert rel_l2(mom, T(g["vae_moments_ref"])) < TOL_FWD
    full = m.decode(T(g["vae_zfull"]).cuda()).sample.cpu()
    assert full.shape == (1, 2, 1024, 64)
    assert rel_l2(full, T(g["vae_image_full_ref_f16"]).float()) < TOL_FWD
    assert abs(m.decode_flops(1, 256, 16) / 1e9 - 156.99) < 1.6


def test_diag_gaussian_sample(golden):
    g, v = golden("dg"), golden("vae")
    from rangeldm_amd.vae import DiagonalGaussianDistributionHIP
    d = DiagonalGaussianDistributionHIP(T(v["vae_moments_ref"]).cuda())
    s = d.sample(noise=T(g["dg_noise"])).cpu()
    assert (s - T(g["dg_sample_ref"])).abs().max() < 1e-5


@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction", "sample"])
def test_scheduler_steps_match_oracle(ptype):
    """DDIM / DDPM steps for every `prediction_type` diffusers' schedulers accept (the reference trains epsilon or v_prediction,
    ldm/train_unconditional.py:505-510), add_noise and get_velocity, against the oracle twin + float64 known answers."""
    from rangeldm_amd.config import SchedulerConfig
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP
    x = T(normal(5, "sx", (2, 4, 32, 8)))
    e = T(normal(5, "se", (2, 4, 32, 8)))
    z = T(normal(5, "sz", (2, 4, 32, 8)))
    cfgp = SchedulerConfig(prediction_type=ptype)
    for n in (50, 10):
        s, so = DDIMSchedulerHIP(cfgp), o_sched.OracleDDIMScheduler(cfgp)
        p, po = DDPMSchedulerHIP(cfgp), o_sched.OracleDDPMScheduler(cfgp)
        for sch in (s, so, p, po):
            sch.set_timesteps(n)
        assert s.timesteps.tolist() == so.timesteps.tolist()
        for t in (int(s.timesteps[0]), int(s.timesteps[n // 2]), 0):
            a = s.step(e.cuda(), t, x.cuda()).prev_sample.cpu()
            assert (a - so.step(e, t, x).prev_sample).abs().max() < 2e-5 * (1 + so.step(e, t, x).prev_sample.abs().max())
            b = p.step(e.cuda(), t, x.cuda(), noise=z.cuda()).prev_sample.cpu()
            rb = po.step(e, t, x, noise=z).prev_sample
            assert (b - rb).abs().max() < 2e-5 * (1 + rb.abs().max())
            a_eta = s.step(e.cuda(), t, x.cuda(), eta=0.5, variance_noise=z.cuda()).prev_sample.cpu()
            r_eta = so.step(e, t, x, eta=0.5, noise=z).prev_sample
            assert (a_eta - r_eta).abs().max() < 2e-5 * (1 + r_eta.abs().max())
    # known answers: SURVEY.md B.4 (epsilon); the other prediction types from the published closed forms in float64
    s = DDIMSchedulerHIP(cfgp)
    s.set_timesteps(50)
    xk = torch.tensor([1.5409961, -0.2934289, -2.1787894, 0.5684313]).view(1, 1, 2, 2)
    ek = torch.tensor([-1.0845224, -1.3985955, 0.4033468, 0.8380263]).view(1, 1, 2, 2)
    out = s.step(ek.cuda(), 980, xk.cuda()).prev_sample.cpu().flatten()
    if ptype == "epsilon":
        assert torch.allclose(out, torch.tensor([2.1102533, -0.0538026, -2.7386351, 0.5099728]), atol=3e-6)
    ac = np.cumprod(1.0 - np.linspace(1e-4, 0.02, 1000, dtype=np.float32).astype(np.float64))
    a_t, a_p = ac[980], ac[960]
    xd, od = xk.double().numpy().ravel(), ek.double().numpy().ravel()
    if ptype == "epsilon":
        x0, pe = (xd - np.sqrt(1 - a_t) * od) / np.sqrt(a_t), od
    elif ptype == "v_prediction":
        x0, pe = np.sqrt(a_t) * xd - np.sqrt(1 - a_t) * od, np.sqrt(a_t) * od + np.sqrt(1 - a_t) * xd
    else:
        x0, pe = od, (xd - np.sqrt(a_t) * od) / np.sqrt(1 - a_t)
    want = np.sqrt(a_p) * x0 + np.sqrt(1 - a_p) * pe
    assert np.abs(out.double().numpy() - want).max() < 2e-5 * (1 + np.abs(want).max())
    pk = DDPMSchedulerHIP(cfgp)
    pk.set_timesteps(50)
    outp = pk.step(ek.cuda(), 980, xk.cuda(), noise=torch.zeros_like(xk).cuda()).prev_sample.cpu().double().numpy().ravel()
    cur_a = a_t / a_p
    wantp = np.sqrt(a_p) * (1 - cur_a) / (1 - a_t) * x0 + np.sqrt(cur_a) * (1 - a_p) / (1 - a_t) * xd
    assert np.abs(outp - wantp).max() < 2e-5 * (1 + np.abs(wantp).max())
    # add_noise (ldm/train_unconditional.py:498) and get_velocity (:508)
    t = torch.tensor([3, 977])
    got = s.add_noise(x.cuda(), e.cuda(), t).cpu()
    assert (got - o_sched.OracleDDPMScheduler().add_noise(x, e, t)).abs().max() < 1e-6
    vel = pk.get_velocity(x.cuda(), e.cuda(), t).cpu()
    assert (vel - po.get_velocity(x, e, t)).abs().max() < 1e-6
    sa, sb = np.sqrt(ac[[3, 977]]), np.sqrt(1 - ac[[3, 977]])
    wantv = sa[:, None] * e.double().numpy().reshape(2, -1) - sb[:, None] * x.double().numpy().reshape(2, -1)
    assert np.abs(vel.double().numpy().reshape(2, -1) - wantv).max() < 1e-5


@pytest.mark.parametrize("ptype", ["v_prediction", "sample"])
def test_captured_sampler_honours_prediction_type(ptype):
    """The scheduler tail fused into conv_out's epilogue (captured sampler) against the same pipeline stepping through
    scheduler.step (`fused=False`) and against the oracle's loop, for a non-epsilon scheduler."""
    from rangeldm_amd.config import SchedulerConfig
    from rangeldm_amd.pipelines import DDIMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
    cfg = UNetConfig(**SMALL)
    m, sd = hip_unet(cfg, "vp.")
    cfgp = SchedulerConfig(prediction_type=ptype)
    x_T = T(normal(17, "xT", (2, 4, 64, 8)))
    outs = []
    for fused in (True, False):
        pipe = DDIMPipelineRange(unet=m, scheduler=DDIMSchedulerHIP(cfgp), pos_encoding=True)
        outs.append(pipe(batch_size=2, num_inference_steps=6, latents=x_T, output_type="torch", fused=fused).cpu())
    assert torch.isfinite(outs[0]).all() and rel_l2(outs[0], outs[1]) < 1e-5
    ref = o_pipe.ddim_pipeline(o_unet.OracleUNet(cfg, sd), o_sched.OracleDDIMScheduler(cfgp), x_T, 6, pos_encoding=True)
    eps_run = DDIMPipelineRange(unet=m, scheduler=DDIMSchedulerHIP(), pos_encoding=True)(
        batch_size=2, num_inference_steps=6, latents=x_T, output_type="torch").cpu()
    assert rel_l2(outs[0], ref) < 3 * TOL_FWD
    assert rel_l2(outs[0], eps_run) > 0.1                               # (the prediction type does reach the kernel)


def _small_unet(in_ch, out_ch, prefix):
    cfg = UNetConfig(sample_size=(32, 8), in_channels=in_ch, out_channels=out_ch, block_out_channels=(32, 32, 64, 64))
    return hip_unet(cfg, prefix)[0], cfg


def test_ldm_pipeline_matches_reference_loop(golden):
    """LDMPipelineRange (strided DDPM with injected noise, as shipped) vs the image the REFERENCE's loop produced."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    g = golden("ldm")
    unet, _ = _small_unet(5, 4, "small.")
    vae, _, _ = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDPMSchedulerHIP(), pos_encoding=True)
    zs = torch.cat([T(g["ldm_step_noise"]), torch.zeros(1, 2, 4, 32, 8)], 0)
    fused = pipe(batch_size=2, num_inference_steps=4, latents=T(g["ldm_x_T"]), step_noise=zs, output_type="torch").cpu()
    loop = pipe(batch_size=2, num_inference_steps=4, latents=T(g["ldm_x_T"]), step_noise=zs.cuda(), output_type="torch",
                fused=False).cpu()
    assert fused.shape == (2, 2, 128, 32)
    assert rel_l2(fused, T(g["ldm_image_ref"])) < TOL_TRAJ
    assert rel_l2(loop, T(g["ldm_image_ref"])) < TOL_TRAJ
    assert rel_l2(fused, loop) < 1e-5              # same kernels, graph vs per-call


def test_ddim_pipeline_matches_reference_loop(golden):
    from rangeldm_amd.pipelines import DDIMPipelineRange
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    g = golden("ddim")
    unet, cfg = _small_unet(3, 2, "smalldm.")
    pipe = DDIMPipelineRange(unet=unet, scheduler=DDPMSchedulerHIP(), pos_encoding=True)
    gen = torch.Generator().manual_seed(21)          # same CPU generator the golden was drawn with
    img = pipe(batch_size=2, generator=gen, num_inference_steps=5, output_type="torch").cpu()
    assert rel_l2(img, T(g["ddim_image_ref"])) < TOL_TRAJ
    gen = torch.Generator().manual_seed(21)
    loop = pipe(batch_size=2, generator=gen, num_inference_steps=5, output_type="torch", fused=False).cpu()
    assert rel_l2(img, loop) < 1e-5
    with pytest.raises(ValueError):
        pipe(batch_size=2, generator=[torch.Generator()], num_inference_steps=2)


def test_ddpm_pipeline_matches_reference_loop(golden):
    """DDPMPipelineRange (ldm/pipelines.py:34-117: pixel space, ancestral, x_T with the UNet's in_channels, the caller's
    generator handed to every scheduler.step) vs the image the REFERENCE's loop produced from the same CPU generator."""
    from rangeldm_amd.pipelines import DDPMPipelineRange, ImagePipelineOutput
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    g = golden("ddpmpix")
    unet, cfg = _small_unet(3, 3, "smallpx.")
    pipe = DDPMPipelineRange(unet=unet, scheduler=DDPMSchedulerHIP())
    ref = T(g["ddpmpix_image_ref"])
    # (a) the generator the golden was drawn with: x_T, then one z per step with t > 0, all off one stream
    for fused in (True, False):
        gen = torch.Generator().manual_seed(41)
        img = pipe(batch_size=2, generator=gen, num_inference_steps=4, output_type="torch", fused=fused).cpu()
        assert img.shape == (2, 3, 32, 8)
        assert rel_l2(img, ref) < TOL_TRAJ, (fused, rel_l2(img, ref))
    # (b) the same noise injected from device buffers
    zs = torch.cat([T(g["ddpmpix_step_noise"]), torch.zeros(1, 2, 3, 32, 8)], 0).cuda()
    fused = pipe(batch_size=2, num_inference_steps=4, latents=T(g["ddpmpix_x_T"]), step_noise=zs, output_type="torch").cpu()
    loop = pipe(batch_size=2, num_inference_steps=4, latents=T(g["ddpmpix_x_T"]), step_noise=zs, output_type="torch",
                fused=False).cpu()
    assert rel_l2(fused, ref) < TOL_TRAJ and rel_l2(loop, ref) < TOL_TRAJ
    assert rel_l2(fused, loop) < 1e-5              # same kernels, graph vs per-call
    assert rel_l2(fused, img) < 1e-5               # injected == drawn
    # (c) the output_type tail (ldm/pipelines.py:109-117): (x/2+0.5).clamp(0,1), NHWC numpy
    gen = torch.Generator().manual_seed(41)
    out = pipe(batch_size=2, generator=gen, num_inference_steps=4, output_type="np")
    assert isinstance(out, ImagePipelineOutput) and out.images.shape == (2, 32, 8, 3)
    assert np.array_equal(out.images, (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy())    # exactly the tail, on this run's x_0
    # against the reference's array: |x_0| reaches tens with random weights, so most pixels sit on a clamp; the rest move by err / 2
    assert np.abs(out.images - g["ddpmpix_image_np_ref"]).mean() < 5e-3
    assert (np.abs(out.images - g["ddpmpix_image_np_ref"]) > 0.25).mean() < 2e-3
    with pytest.raises(ValueError):
        pipe(batch_size=2, num_inference_steps=4, latents=torch.zeros(2, 2, 32, 8))


def test_upscale_pipeline_matches_reference_loop(golden):
    from rangeldm_amd.pipelines import LDMUpscalePipelineRange
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    from rangeldm_amd.encoders import SparseRangeImageEncoder2
    g = golden("up")
    unet, _ = _small_unet(12, 4, "smallup.")
    vae, _, _ = hip_vae()
    pipe = LDMUpscalePipelineRange(vae=vae, unet=unet, scheduler=DDPMSchedulerHIP())
    zs = torch.cat([T(g["up_step_noise"]), torch.zeros(1, 2, 4, 32, 8)], 0)
    img = pipe(image=T(g["up_cond"]).cuda(), condition_encoder=SparseRangeImageEncoder2(), batch_size=2,
               num_inference_steps=3, latents=T(g["up_x_T"]), step_noise=zs, output_type="torch").cpu()
    assert rel_l2(img, T(g["up_image_ref"])) < TOL_TRAJ
    with pytest.raises(ValueError):
        pipe(image=None)


def test_teacher_forced_trajectory():
    """feed the ORACLE's x_t to the HIP UNet at every step; eps must agree per step."""
    cfg = UNetConfig(**SMALL)
    m, sd = hip_unet(cfg, "t.")
    ou = o_unet.OracleUNet(cfg, sd)
    traj = []
    x_T = T(normal(7, "xT", (2, 4, 64, 8)))
    o_pipe.ddim_pipeline(ou, o_sched.OracleDDIMScheduler(), x_T, 10, pos_encoding=True, trajectory=traj)
    pe = o_pipe.pos_encoding_channel(2, 64, 8)
    sched = o_sched.OracleDDIMScheduler()
    sched.set_timesteps(10)
    for (x_t, eps_ref), t in zip(traj, sched.timesteps):
        eps = m(torch.cat([x_t, pe], 1).cuda(), t).sample.cpu()
        assert rel_l2(eps, eps_ref) < TOL_FWD, int(t)


def test_full_config_sampler_properties():
    """BASELINE config-2 shapes (batch reduced to 2): finite, deterministic, per-sample independent."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
    cfg = UNetConfig()
    unet, _ = hip_unet(cfg, "")
    vae, _, _ = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    x_T = T(normal(9, "xT", (2, 4, 256, 16)))
    a = pipe(batch_size=2, num_inference_steps=6, latents=x_T, output_type="torch").cpu()
    b = pipe(batch_size=2, num_inference_steps=6, latents=x_T, output_type="torch").cpu()
    assert a.shape == (2, 2, 1024, 64) and torch.isfinite(a).all()
    assert torch.equal(a, b)                                           # no atomics anywhere: bit-reproducible
    solo = pipe(batch_size=1, num_inference_steps=6, latents=x_T[1:], output_type="torch").cpu()
    assert rel_l2(solo[0], a[1]) < 2e-2                                 # GroupNorm / attention never mix samples


@pytest.mark.parametrize("sched_name", ["ddim", "ddpm"])
def test_batch16_sampler_clusters_match_launch_per_layer(sched_name):
    """BASELINE config 2 at its real batch (16 images: every level of the UNet runs as clusters of 16 workgroups per image inside
    persistent launches, trunk.hip) through the CAPTURED sampler -- step graphs, fused scheduler tail, VAE decode -- against the same
    sampler with the clusters off (rldm_debug_set_flags(Flag.NO_CLUSTERS): one launch per layer above the 32x2 level).  Same kernels' code on
    the same operands: identical images; the launch count drops."""
    from rangeldm_amd import _lib
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP
    cfg = UNetConfig()
    x_T = T(normal(21, "xT", (16, 4, 256, 16)))
    zs = T(normal(22, "zs", (3, 16, 4, 256, 16)))
    outs, launches = [], []
    for flags in (0, Flag.NO_CLUSTERS):
        _lib.lib().rldm_debug_set_flags(flags)
        try:
            unet, _ = hip_unet(cfg, "")
            vae, _, _ = hip_vae()
            sched = DDIMSchedulerHIP() if sched_name == "ddim" else DDPMSchedulerHIP()
            pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=sched, pos_encoding=True)
            kw = dict(batch_size=16, num_inference_steps=3, latents=x_T, output_type="torch")
            if sched_name == "ddpm":
                kw["step_noise"] = zs
            a = pipe(**kw).cpu()
            b = pipe(**kw).cpu()                          # replayed graphs: the cluster counters re-arm themselves
            assert torch.isfinite(a).all() and torch.equal(a, b)
            outs.append(a)
            launches.append(unet.num_launches(16))
        finally:
            _lib.lib().rldm_debug_set_flags(0)
    assert launches[0] < launches[1]
    assert torch.equal(outs[0], outs[1])


def test_sampler_falls_back_when_the_cluster_self_check_fails(monkeypatch):
    """The persistent launches check their one assumption (an image's workgroups on one XCD, all resident) at the sampler's eager
    warm-up step; if the check word is set, the process falls back to one launch per layer -- same kernels, same images.  The failure
    is injected (RLDM_TEST_TRUNK_FAIL)."""
    from rangeldm_amd import _lib
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
    cfg = UNetConfig()
    x_T = T(normal(23, "xT", (16, 4, 256, 16)))
    outs = []
    try:
        for fail in (False, True):
            if fail:
                monkeypatch.setenv("RLDM_TEST_TRUNK_FAIL", "1")
            unet, _ = hip_unet(cfg, "")
            vae, _, _ = hip_vae()
            pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
            outs.append(pipe(batch_size=16, num_inference_steps=2, latents=x_T, output_type="torch").cpu())
            assert torch.isfinite(outs[-1]).all()
    finally:
        monkeypatch.delenv("RLDM_TEST_TRUNK_FAIL", raising=False)
        _lib.lib().rldm_debug_set_flags(0)              # (the fall-back sets Flag.NO_PERSISTENT for the process)
    assert torch.equal(outs[0], outs[1])


def test_mid_run_cluster_failure_is_reported_by_the_same_call():
    """A cluster wait that gives up in the MIDDLE of a run (not at the warm-up step) used to cost one call's images silently.  Now the
    call that tripped it raises (rldm_sampler_status, asked by every pipeline __call__), its outputs are NaN-marked on the device by the
    call's last launch, and the sampler has rebuilt itself as one launch per layer -- same kernels, same tiles, so the retry returns
    exactly the images of a healthy run.  The failure is injected (rldm_debug_inject_trunk_error: the self-check word is set on the
    sampler's stream ahead of the step graphs, as a timed-out poll would)."""
    from rangeldm_amd import _lib
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
    cfg = UNetConfig()
    x_T = T(normal(23, "xT", (16, 4, 256, 16)))
    unet, _ = hip_unet(cfg, "")
    vae, _, _ = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    kw = dict(batch_size=16, num_inference_steps=2, latents=x_T, output_type="torch")
    good = pipe(**kw).cpu()
    assert torch.isfinite(good).all()
    h = pipe._fused.get(unet, vae, pipe.scheduler, 16, 2, 0, True, 0)
    # (1) the synchronous contract: the failing call raises
    _lib.check(_lib.lib().rldm_debug_inject_trunk_error(h, 1), "inject")
    with pytest.raises(RuntimeError, match="self-check"):
        pipe(**kw)
    again = pipe(**kw).cpu()                               # the sampler fell back by itself: one launch per layer, identical images
    assert torch.equal(again, good)
    # (2) an asynchronous caller: the outputs of the failed call are NaN-marked, status() says why
    unet2, _ = hip_unet(cfg, "")
    pipe2 = LDMPipelineRange(vae=vae, unet=unet2, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    assert torch.equal(pipe2(**kw).cpu(), good)
    h2 = pipe2._fused.get(unet2, vae, pipe2.scheduler, 16, 2, 0, True, 0)
    _lib.check(_lib.lib().rldm_debug_inject_trunk_error(h2, 1), "inject")
    bad = pipe2(check=False, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(bad).all()                          # every image of the failed call, not just the head of the first
    with pytest.raises(RuntimeError, match="self-check"):
        pipe2._fused.status(h2)
    assert torch.equal(pipe2(**kw).cpu(), good)
    # the fall-back is scoped to the sampler that failed: a fresh one still builds its persistent launches
    unet3, _ = hip_unet(cfg, "")
    assert unet3.num_launches(16) <= 40


def test_two_samplers_on_two_streams_do_not_share_persistent_launches():
    """Persistent launches need the chip to themselves (256 co-resident workgroups waiting for each other).  A second sampler whose call
    arrives on ANOTHER stream while the first one's is still in flight drops its persistent launches by itself (no debug flag for the
    host to know about); both calls return the images of the serial runs."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
    cfg = UNetConfig()
    vae, _, _ = hip_vae()
    xa = T(normal(31, "xTa", (16, 4, 256, 16)))
    xb = T(normal(32, "xTb", (16, 4, 256, 16)))
    pipes = []
    for _ in range(2):
        unet, _sd = hip_unet(cfg, "")
        pipes.append(LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True))
    kw = dict(batch_size=16, num_inference_steps=4, output_type="torch")
    ref_a = pipes[0](latents=xa, **kw).cpu()               # serial (each has the device to itself: persistent launches on)
    ref_b = pipes[1](latents=xb, **kw).cpu()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = pipes[0](latents=xa, check=False, **kw)
    with torch.cuda.stream(s2):
        b = pipes[1](latents=xb, check=False, **kw)          # sees pipes[0]'s call in flight on s1: one launch per layer from here on
    torch.cuda.synchronize()
    for p in pipes:
        p._fused.status_all()
    assert torch.equal(a.cpu(), ref_a) and torch.equal(b.cpu(), ref_b)


def test_concurrent_chains_match_single_chain(monkeypatch):
    """The sampler splits a batch >= 32 into chains of >= 16 samples on separate streams (sampler_num_lanes, sampler.hip);
    RLDM_LANES forces the split at a small batch here.  Samples never interact, so the chains must reproduce the
    single-chain images (up to the tile routing, which depends on the chain's batch) -- for DDIM and for the DDPM mode,
    whose step noise is sliced per chain."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP
    cfg = UNetConfig()
    vae, _, _ = hip_vae()
    x_T = T(normal(11, "xT", (4, 4, 256, 16)))
    for sched in (DDIMSchedulerHIP, DDPMSchedulerHIP):
        out = {}
        for lanes in ("1", "2", "4"):
            monkeypatch.setenv("RLDM_LANES", lanes)
            unet, _ = hip_unet(cfg, "")
            pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=sched(), pos_encoding=True)
            zs = T(normal(12, "zs", (4, 4, 4, 256, 16)))               # [step][B, C, W, H] ancestral noise (DDPM mode only)
            out[lanes] = pipe(batch_size=4, num_inference_steps=4, latents=x_T, step_noise=zs, output_type="torch").cpu()
            assert torch.isfinite(out[lanes]).all()
        assert rel_l2(out["2"], out["1"]) < 2e-2, sched.__name__
        assert rel_l2(out["4"], out["1"]) < 2e-2, sched.__name__
        for j in range(4):                                              # every sample, not just the average
            assert rel_l2(out["2"][j], out["1"][j]) < 3e-2


@pytest.mark.gpu
def test_graph_trace_names_only_a_live_plan():
    """rldm_debug_graph_trace walks the ops of the plan the last traced step ran.  That plan belongs to a sampler lane: once the
    sampler is destroyed there is no traced plan and the call returns 0 (as before any trace was taken), and a second traced
    sampler makes the trace live again.  Smallest shape that builds a plan: the smoke UNet, no VAE, batch 2, 2 DDIM steps."""
    import ctypes as C
    from rangeldm_amd import _lib
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
    cfg = UNetConfig(sample_size=(64, 8), block_out_channels=(32, 32, 64, 64))
    unet, _ = hip_unet(cfg, "trace.")
    x_T = T(normal(21, "trace/xT", (2, 4, 64, 8))).cuda()
    out = torch.empty_like(x_T)
    sched = DDIMSchedulerHIP()
    sched.set_timesteps(2)
    ts = np.ascontiguousarray(sched.timesteps.numpy().astype(np.int64))
    coef = sched.sampler_table(0.0)
    L = _lib.lib()

    def trace():
        stamps = (C.c_ulonglong * 4096)()
        names = C.create_string_buffer(1 << 16)
        n = L.rldm_debug_graph_trace(stamps, 4096, names, len(names))
        return n, [s for s in names.value.decode().split("\n") if s]

    def traced_sample():
        sc = _lib.SamplerConfigC()
        sc.batch, sc.num_steps, sc.mode, sc.pos_encoding = 2, 2, _lib.RLDM_SAMPLER_DDIM, 1
        sc.plan_flags = int(Flag.GRAPH_TRACE)
        sc.coef = coef.ctypes.data_as(C.POINTER(C.c_float))
        sc.timesteps = ts.ctypes.data_as(C.POINTER(C.c_int64))
        h = C.c_void_p()
        _lib.check(L.rldm_sampler_create(unet._h, None, C.byref(sc), C.byref(h)), "rldm_sampler_create")
        _lib.check(L.rldm_sample(h, C.c_void_p(x_T.data_ptr()), None, None, C.c_void_p(out.data_ptr()), None,
                                 _lib.stream_ptr(x_T.device)), "rldm_sample")
        _lib.check(L.rldm_sampler_status(h), "rldm_sampler_status")
        return h

    h = traced_sample()
    n, names = trace()
    assert n > 0 and len(names) == n
    L.rldm_sampler_destroy(h)
    assert trace()[0] == 0
    h2 = traced_sample()
    n2, names2 = trace()
    L.rldm_sampler_destroy(h2)
    assert n2 == n and names2 == names
    assert torch.isfinite(out).all()


# ---- goldens computed BY REFERENCE CODE (oracle/validate_unet_against_reference.py): the skip-concat / temb UNet `Model`
# of vae/sgm/modules/diffusionmodules/model.py:521-704 after the reference's surgery, with the reference's multi-head
# CrossAttention (vae/sgm/modules/attention.py:194-284) in every attention block ------------------------------------------
from tests.test_oracle_golden import REF_UNETS, SGM_SINUSOID, ref_unet_sd     # noqa: E402


def hip_ref_unet(cfg, prefix):
    from rangeldm_amd.unet import UNet2DModelHIP
    m = UNet2DModelHIP(cfg)
    m.load_state_dict(ref_unet_sd(cfg, prefix))
    return m


@pytest.mark.parametrize("name", list(REF_UNETS))
@pytest.mark.parametrize("sinus", ["sgm", "unet2d"])
def test_unet_matches_reference_model(golden, name, sinus):
    g = golden("unetref")
    cfg = UNetConfig(**REF_UNETS[name], **(SGM_SINUSOID if sinus == "sgm" else {}))
    m = hip_ref_unet(cfg, f"ref/{name}.")
    out = m(T(g[f"unetref_{name}_{sinus}_x"]).cuda(), T(g[f"unetref_{name}_{sinus}_t"])).sample.cpu()
    assert rel_l2(out, T(g[f"unetref_{name}_{sinus}_eps"])) < TOL_FWD


def test_unet_full_width_matches_reference_model(golden):
    """RangeLDM KITTI-360 config, 30.1 M parameters, (1, 5, 256, 16): eps of the reference-composed Model."""
    g = golden("unetref")
    m = hip_ref_unet(UNetConfig(**SGM_SINUSOID), "ref/full.")
    out = m(T(g["unetref_full_x"]).cuda(), int(g["unetref_full_t"][0])).sample.cpu()
    assert rel_l2(out, T(g["unetref_full_sgm_eps"])) < TOL_FWD


def test_other_presets_full_size_match_reference(golden):
    """BASELINE configs 4, 3 and 1 at full width / size: the 12-channel upsample UNet, the nuScenes-shape VAE decode
    (sgm Decoder) and the 113.7 M-parameter RangeDM UNet on a 1024 x 64 image."""
    from rangeldm_amd.config import PRESETS
    g = golden("presets")
    m = hip_ref_unet(UNetConfig(in_channels=12, **SGM_SINUSOID), "ref/up.")
    assert rel_l2(m(T(g["presets_up_x"]).cuda(), 700).sample.cpu(), T(g["presets_up_eps"])) < TOL_FWD
    del m
    vae, _, _ = hip_vae()
    img = vae.decode(T(g["presets_nusc_z"]).cuda()).sample.cpu()
    assert img.shape == (1, 2, 1024, 32)
    assert rel_l2(img, T(g["presets_nusc_image_f16"]).float()) < TOL_FWD
    kw = {k: v for k, v in PRESETS["RangeDM"]["unet"].to_dict().items() if k not in SGM_SINUSOID}
    m = hip_ref_unet(UNetConfig(**kw, **SGM_SINUSOID), "ref/rangedm.")
    out = m(T(g["presets_rangedm_x_f16"]).float().cuda(), 900).sample.cpu()
    assert out.shape == (1, 2, 1024, 64)
    ref = T(g["presets_rangedm_eps"])
    # (one sample: the worst-case gate is per output channel and per quarter of the azimuth instead of per sample)
    worst = max(float(rel_l2(out[:, c, q * 256:(q + 1) * 256], ref[:, c, q * 256:(q + 1) * 256])) for c in range(2) for q in range(4))
    print(f"RangeDM B=1: rel-L2 {float(rel_l2(out, ref)):.3e}, worst (channel, azimuth quarter) {worst:.3e}")
    assert rel_l2(out, ref) < TOL_FWD and worst < 1.5 * TOL_FWD


@pytest.mark.parametrize("sched", ["ddim", "ddpm"])
def test_50_step_full_width_sampler_matches_reference_loop(golden, sched):
    """The headline workload (BASELINE config 2) at batch 1, all 50 steps, free-running: the golden is the reference's own
    LDMPipelineRange.__call__ (ldm/pipelines.py:282-383) driving the reference-composed Model and the sgm Decoder in fp32.
    With random weights x grows to |x_0| ~ 4e3, so errors are relative."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP
    g = golden("traj")
    unet = hip_ref_unet(UNetConfig(**SGM_SINUSOID), "ref/full.")
    vae, _, _ = hip_vae()
    x_T = T(normal(51, f"traj/{sched}/x_T", (1, 4, 256, 16)))
    if sched == "ddim":
        pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
        zs = None
    else:
        pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDPMSchedulerHIP(), pos_encoding=True)
        zs = torch.stack([T(normal(52, f"traj/z/{i}", (1, 4, 256, 16))) for i in range(50)])
    h = pipe._fused.get(unet, vae, pipe.scheduler, 1, 50, 0 if sched == "ddim" else 1, True, 0)
    img = torch.empty((1, 2, 1024, 64), device="cuda")
    lat = torch.empty((1, 4, 256, 16), device="cuda")
    pipe._fused.run(h, x_T.cuda().contiguous(), None if zs is None else zs.cuda().contiguous(), None, img, latents_out=lat)
    e_lat = rel_l2(lat.cpu(), T(g[f"traj_{sched}_latent_ref"]))
    e_img = rel_l2(img.cpu(), T(g[f"traj_{sched}_image_ref_f16"]).float())
    print(f"50-step {sched}: final latent rel-L2 {e_lat:.3e}, decoded image rel-L2 {e_img:.3e}")
    assert e_lat < TOL_X0 and e_img < TOL_TRAJ
    # the public call gives the same image
    img2 = pipe(batch_size=1, num_inference_steps=50, latents=x_T, step_noise=zs, output_type="torch")
    assert torch.equal(img2, img)
    # teacher-forced along the reference trajectory: eps at the reference's x_t of steps 1, 10, 25, 40, 49
    pe = o_pipe.pos_encoding_channel(1, 256, 16)
    ts = pipe.scheduler.timesteps
    cfg = UNetConfig(**SGM_SINUSOID)
    ou = o_unet.OracleUNet(cfg, ref_unet_sd(cfg, "ref/full."))
    for i in (1, 10, 25, 40, 49):
        x = torch.cat([T(g[f"traj_{sched}_x_step{i}"]), pe], 1)
        assert rel_l2(unet(x.cuda(), ts[i]).sample.cpu(), ou(x, ts[i]).sample) < TOL_FWD, i


def test_batch16_forward_matches_reference_model(golden):
    """The HEADLINE batch against reference code, directly: 16 x (5, 256, 16) through the plan every level of which runs as clusters
    of 16 workgroups per image inside persistent launches (trunk.hip variants 0 / 1 / 2 exist only from 13 images on), against eps of
    the reference-composed full-width Model at two timesteps (tests/golden/b16.npz, oracle/validate_batch16_against_reference.py)."""
    g = golden("b16")
    m = hip_ref_unet(UNetConfig(**SGM_SINUSOID), "ref/full.")
    x = T(normal(61, "b16/x", (16, 5, 256, 16))).cuda()
    n_clustered = m.num_launches(16)
    for t in (480, 37):
        out = m(x, t).sample.cpu()
        ref = T(g[f"b16_eps_t{t}_f16"]).float()
        e = rel_l2(out, ref)
        worst = max(float(rel_l2(out[j], ref[j])) for j in range(16))
        print(f"B=16 forward t={t}: rel-L2 {float(e):.3e}, worst sample {worst:.3e}, {n_clustered} launches")
        assert e < TOL_FWD and worst < 1.5 * TOL_FWD
    assert m.trunk_status(16) == 0
    assert n_clustered <= 40                               # (the cluster plan, not the launch-per-layer one: 90+)


def test_other_configs_at_their_batch_match_reference_model(golden):
    """BASELINE config 4 (12-channel upsample UNet) at its batch 16 -- the same cluster plan as the headline -- and config 3's per-GPU
    share (nuScenes 256 x 8 latents, 4 images: the 32 x 1 level as one persistent launch with its 32-token attention phases), one
    forward each against the reference-composed Model (tests/golden/b16.npz)."""
    g = golden("b16")
    m = hip_ref_unet(UNetConfig(in_channels=12, **SGM_SINUSOID), "ref/up.")
    x = T(normal(66, "b16/up_x", (16, 12, 256, 16))).cuda()
    ref = T(g["b16_up_eps_t700_f16"]).float()
    out = m(x, 700).sample.cpu()
    worst = max(float(rel_l2(out[j], ref[j])) for j in range(16))
    print(f"upsample B=16: rel-L2 {float(rel_l2(out, ref)):.3e}, worst sample {worst:.3e}")
    assert rel_l2(out, ref) < TOL_FWD and worst < 1.5 * TOL_FWD and m.trunk_status(16) == 0
    del m
    m = hip_ref_unet(UNetConfig(sample_size=(256, 8), **SGM_SINUSOID), "ref/nusc.")
    x = T(normal(67, "b16/nusc_x", (4, 5, 256, 8))).cuda()
    ref = T(g["b16_nusc4_eps_t250"])
    out = m(x, 250).sample.cpu()
    worst = max(float(rel_l2(out[j], ref[j])) for j in range(4))
    print(f"nuScenes B=4: rel-L2 {float(rel_l2(out, ref)):.3e}, worst sample {worst:.3e}")
    assert rel_l2(out, ref) < TOL_FWD and worst < 1.5 * TOL_FWD and m.trunk_status(4) == 0
    # ... and config 3's whole batch on one GPU (`eval_batch_size: 32`): clusters at every level, conv_stream on 32 x 4 tiles
    x = T(normal(68, "b16/nusc32_x", (32, 5, 256, 8))).cuda()
    ref = T(g["b16_nusc32_eps_t610_f16"]).float()
    out = m(x, 610).sample.cpu()
    worst = max(float(rel_l2(out[j], ref[j])) for j in range(32))
    print(f"nuScenes B=32: rel-L2 {float(rel_l2(out, ref)):.3e}, worst sample {worst:.3e}, {m.num_launches(32)} launches")
    assert rel_l2(out, ref) < TOL_FWD and worst < 1.5 * TOL_FWD and m.trunk_status(32) == 0


def test_batch16_sampler_matches_reference_loop(golden):
    """... and the captured batch-16 sampler (step graphs, fused scheduler tail, clusters ON): x_0 after 3 DDIM steps against the
    reference's own LDMPipelineRange loop (ldm/pipelines.py:353-362) at batch 16, at the latent tolerance of the 50-step test."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
    g = golden("b16")
    unet = hip_ref_unet(UNetConfig(**SGM_SINUSOID), "ref/full.")
    vae, _, _ = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    x_T = T(normal(62, "b16/x_T", (16, 4, 256, 16)))
    h = pipe._fused.get(unet, vae, pipe.scheduler, 16, 3, 0, True, 0)
    img = torch.empty((16, 2, 1024, 64), device="cuda")
    lat = torch.empty((16, 4, 256, 16), device="cuda")
    pipe._fused.run(h, x_T.cuda().contiguous(), None, None, img, latents_out=lat)
    ref = T(g["b16_ddim3_latent_f16"]).float()
    e = rel_l2(lat.cpu(), ref)
    worst = max(float(rel_l2(lat[j].cpu(), ref[j])) for j in range(16))
    print(f"B=16 3-step DDIM: final latent rel-L2 {float(e):.3e}, worst sample {worst:.3e}")
    assert e < TOL_X0 and worst < 2 * TOL_X0
    assert torch.isfinite(img).all()
    assert unet.num_launches(16) <= 40


def test_batch16_headline_run_matches_reference_loop(golden):
    """The headline workload itself (BASELINE config 2): all 50 DDIM steps at batch 16, captured step graphs + persistent launches, against
    x_0 of the reference's own LDMPipelineRange loop (ldm/pipelines.py:353-362) driving the reference-composed Model
    (tests/golden/b16long.npz, written by `python -m oracle.validate_batch16_against_reference --long`, which also checks the oracle's
    50-step run against it)."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
    g = golden("b16long")
    unet = hip_ref_unet(UNetConfig(**SGM_SINUSOID), "ref/full.")
    vae, _, _ = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    x_T = T(normal(62, "b16/x_T", (16, 4, 256, 16)))
    h = pipe._fused.get(unet, vae, pipe.scheduler, 16, 50, 0, True, 0)
    img = torch.empty((16, 2, 1024, 64), device="cuda")
    lat = torch.empty((16, 4, 256, 16), device="cuda")
    pipe._fused.run(h, x_T.cuda().contiguous(), None, None, img, latents_out=lat)
    ref = T(g["b16long_ddim50_latent_f16"]).float()
    e = rel_l2(lat.cpu(), ref)
    worst = max(float(rel_l2(lat[j].cpu(), ref[j])) for j in range(16))
    print(f"B=16 50-step DDIM: final latent rel-L2 {float(e):.3e}, worst sample {worst:.3e}")
    assert e < TOL_X0 and worst < 2 * TOL_X0
    assert torch.isfinite(img).all()


def test_upscale_full_width_pipeline_matches_reference_loop(golden):
    """BASELINE config 4 end to end at full width: LDMUpscalePipelineRange.__call__ (ldm/pipelines.py:414-519) for 10 strided-DDPM
    steps at batch 2 on the 12-channel UNet (30.1 M parameters) with SparseRangeImageEncoder2, against the reference's loop driving
    the reference-composed Model and the sgm Decoder (tests/golden/upfull.npz)."""
    from rangeldm_amd.pipelines import LDMUpscalePipelineRange
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    from rangeldm_amd.encoders import SparseRangeImageEncoder2
    g = golden("upfull")
    unet = hip_ref_unet(UNetConfig(in_channels=12, **SGM_SINUSOID), "ref/up.")
    vae, _, _ = hip_vae()
    pipe = LDMUpscalePipelineRange(vae=vae, unet=unet, scheduler=DDPMSchedulerHIP())
    cond_img = T(normal(63, "upfull/cond", (2, 2, 1024, 16)))
    x_T = T(normal(64, "upfull/x_T", (2, 4, 256, 16)))
    zs = torch.stack([T(normal(65, f"upfull/z/{i}", (2, 4, 256, 16))) for i in range(10)])
    img = pipe(image=cond_img.cuda(), condition_encoder=SparseRangeImageEncoder2(), batch_size=2, num_inference_steps=10,
               latents=x_T, step_noise=zs, output_type="torch").cpu()
    e_img = rel_l2(img, T(g["upfull_image_f16"]).float())
    print(f"full-width upscale pipeline, 10 steps: decoded image rel-L2 {float(e_img):.3e}")
    assert img.shape == (2, 2, 1024, 64) and e_img < TOL_TRAJ
    # the latent itself (the discriminating quantity: the decoder's GroupNorms renormalise it)
    cond = SparseRangeImageEncoder2()(cond_img.cuda()).contiguous()
    h = pipe._fused.get(unet, vae, pipe.scheduler, 2, 10, 1, False, 8)
    lat = torch.empty((2, 4, 256, 16), device="cuda")
    out = torch.empty((2, 2, 1024, 64), device="cuda")
    pipe._fused.run(h, x_T.cuda().contiguous(), zs.cuda().contiguous(), cond, out, latents_out=lat)
    e_lat = rel_l2(lat.cpu(), T(g["upfull_latent"]))
    print(f"full-width upscale pipeline, 10 steps: final latent rel-L2 {float(e_lat):.3e}")
    assert e_lat < TOL_X0


def test_inpainting_mask_path_matches_reference(golden):
    """LDMUpscalePipelineRange with a mask: encode_masked_image (ldm/pipelines.py:406-412) + the conditional loop."""
    from rangeldm_amd.pipelines import LDMUpscalePipelineRange
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    g = golden("inpaint")
    unet, _ = _small_unet(9, 4, "smallinp.")
    vae, _, _ = hip_vae()
    pipe = LDMUpscalePipelineRange(vae=vae, unet=unet, scheduler=DDPMSchedulerHIP())
    img, mask = T(g["inpaint_image"]), T(g["inpaint_mask"])
    cond = pipe.encode_masked_image((img * mask).cuda(), mask.cuda(), noise=T(g["inpaint_enc_noise"])).cpu()
    assert cond.shape == (2, 5, 32, 8)
    assert torch.equal(cond[:, 4:], T(g["inpaint_cond_ref"])[:, 4:])            # nearest-resized mask: exact
    assert rel_l2(cond[:, :4], T(g["inpaint_cond_ref"])[:, :4]) < TOL_FWD
    zs = torch.cat([T(g["inpaint_step_noise"]), torch.zeros(1, 2, 4, 32, 8)], 0)
    for fused in (True, False):
        out = pipe(image=(img * mask).cuda(), mask=mask.cuda(), batch_size=2, num_inference_steps=3, latents=T(g["inpaint_x_T"]),
                   step_noise=zs.cuda() if not fused else zs, encode_noise=T(g["inpaint_enc_noise2"]), output_type="torch",
                   fused=fused).cpu()
        assert rel_l2(out, T(g["inpaint_image_ref"])) < TOL_TRAJ, fused


def test_reloading_weights_under_a_live_sampler():
    """load_state_dict on a model a pipeline already sampled with (periodic EMA evaluation during training): the sampler
    must re-plan on the new device weights, not replay graphs over the freed ones."""
    from rangeldm_amd.pipelines import DDIMPipelineRange
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    unet, cfg = _small_unet(3, 2, "reload.a.")
    sd_a = synth_state_dict(unet_param_shapes(cfg), prefix="reload.a.")
    sd_b = synth_state_dict(unet_param_shapes(cfg), prefix="reload.b.")
    pipe = DDIMPipelineRange(unet=unet, scheduler=DDPMSchedulerHIP(), pos_encoding=True)
    x_T = T(normal(13, "reload/x", (2, 2, 32, 8)))
    a1 = pipe(batch_size=2, num_inference_steps=4, latents=x_T, output_type="torch").cpu()
    unet.load_state_dict(sd_b)
    b1 = pipe(batch_size=2, num_inference_steps=4, latents=x_T, output_type="torch").cpu()
    ob = o_pipe.ddim_pipeline(o_unet.OracleUNet(cfg, sd_b), o_sched.OracleDDIMScheduler(), x_T, 4, pos_encoding=True)
    assert rel_l2(b1, ob) < TOL_TRAJ and rel_l2(b1, a1) > 0.1
    unet.load_state_dict(sd_a)
    assert torch.equal(pipe(batch_size=2, num_inference_steps=4, latents=x_T, output_type="torch").cpu(), a1)
