"""Host: what the three sampling drivers share (rangeldm_amd.inference: build_models, device_rng_kwargs) and that their refusals still
come before any model is built.  The model classes are replaced by recorders: configs and state dicts are what is compared."""
import numpy as np
import pytest

from rangeldm_amd import inference, inference_conditional as IC, rng
from rangeldm_amd.config import UNetConfig, VAEConfig
from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
from rangeldm_amd.synth import synth_state_dict


class FakeModel:
    made = []

    def __init__(self, config):
        self.config, self.state = config, None
        FakeModel.made.append(self)

    def load_state_dict(self, sd):
        self.state = sd


class FakeUNet(FakeModel):
    pass


class FakeVAE(FakeModel):
    pass


@pytest.fixture
def fake_models(monkeypatch):
    import rangeldm_amd.unet
    import rangeldm_amd.vae
    monkeypatch.setattr(rangeldm_amd.unet, "UNet2DModelHIP", FakeUNet)
    monkeypatch.setattr(rangeldm_amd.vae, "AutoencoderKLHIP", FakeVAE)
    FakeModel.made = []
    return FakeModel.made


def same_state(a, b):
    return list(a) == list(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


UNET = UNetConfig(sample_size=(32, 8), block_out_channels=(32, 32, 64, 64))
VAE = VAEConfig(ch=32, sample_size=(128, 32))


def test_build_models_with_synthetic_weights(fake_models):
    """What each driver's own block did: UNet from synth_state_dict(seed, prefix ""), VAE (latent configs only) from prefix "vae."."""
    cfg = dict(unet=UNET, vae=VAE)
    unet, vae, sched_cfg = inference.build_models(cfg, None, False, 7)
    assert [type(m) for m in fake_models] == [FakeUNet, FakeVAE] and sched_cfg is None
    assert unet.config is UNET and vae.config is VAE and cfg == dict(unet=UNET, vae=VAE)
    assert same_state(unet.state, synth_state_dict(unet_param_shapes(UNET), seed=7, prefix=""))
    assert same_state(vae.state, synth_state_dict(vae_param_shapes(VAE), seed=7, prefix="vae."))
    assert not same_state(unet.state, synth_state_dict(unet_param_shapes(UNET), seed=8, prefix=""))
    # a pixel-space config: no VAE is built
    del fake_models[:]
    unet, vae, sched_cfg = inference.build_models(dict(unet=UNET, vae=None), None, False, 7)
    assert [type(m) for m in fake_models] == [FakeUNet] and vae is None and sched_cfg is None
    assert same_state(unet.state, synth_state_dict(unet_param_shapes(UNET), seed=7, prefix=""))


@pytest.mark.parametrize("latent", [True, False])
def test_build_models_from_an_output_dir(fake_models, monkeypatch, latent):
    """--weights: the checkpoint's own configs replace cfg["unet"] / cfg["vae"], its scheduler config is returned, --ema is passed on."""
    import rangeldm_amd.checkpoint
    other_unet, other_vae = UNetConfig(sample_size=(64, 8), block_out_channels=(32, 32, 64, 64)), VAEConfig(ch=16, sample_size=(256, 32))
    asked = []

    def load_output_dir(path, with_vae=True, ema=False):
        asked.append((path, with_vae, ema))
        ck = dict(unet_config=other_unet, unet={"u": 1}, scheduler_config={"prediction_type": "v_prediction"})
        if with_vae:
            ck.update(vae_config=other_vae, vae={"v": 2})
        return ck
    monkeypatch.setattr(rangeldm_amd.checkpoint, "load_output_dir", load_output_dir)
    cfg = dict(unet=UNET, vae=VAE if latent else None)
    unet, vae, sched_cfg = inference.build_models(cfg, "some/dir", True, 7)
    assert asked == [("some/dir", latent, True)] and sched_cfg == {"prediction_type": "v_prediction"}
    assert cfg["unet"] is other_unet and unet.config is other_unet and unet.state == {"u": 1}
    if latent:
        assert cfg["vae"] is other_vae and vae.config is other_vae and vae.state == {"v": 2}
    else:
        assert cfg["vae"] is None and vae is None and len(fake_models) == 1


@pytest.mark.parametrize("world", [1, 2])
def test_device_rng_keywords_address_the_global_sample_index(world):
    B, samples, seed = 3, 14, 99
    seen = []
    for rank in range(world):
        for i in range(inference.plan_iterations(samples, B, world)):
            kw = inference.device_rng_kwargs(seed, i, B, rank, world)
            assert sorted(kw) == ["generator", "sample_offset"]
            g = kw["generator"]
            assert isinstance(g, rng.DeviceGenerator) and g.get_state() == (seed, 0)        # a fresh generator: every call is draw 0
            assert kw["sample_offset"] == (rank + world * i) * B
            keep = inference.image_indices(i, B, rank, world, samples)
            if keep:
                assert keep[0] == (0, kw["sample_offset"])      # sample_offset = the global index of the call's first image
            seen += [kw["sample_offset"] + j for j in range(B)]
    assert sorted(seen)[:samples] == list(range(samples)) and len(set(seen)) == len(seen)


def test_the_drivers_refuse_before_they_build_a_model(monkeypatch, tmp_path):
    def built(*a, **k):
        raise AssertionError("a model was built before the refusal")
    monkeypatch.setattr(inference, "build_models", built)
    monkeypatch.setattr(IC, "build_models", built)
    guided = ["--guided", "--samples", "1"]
    # in this order in main_guided: conditional config, pixel-space config, scheduler, resampling, DPM-Solver++
    with pytest.raises(ValueError, match="unconditional config"):
        IC.main(guided + ["--cfg", "upsample", "--decoder-guidance"])
    with pytest.raises(ValueError, match="pixel-space"):
        IC.main(guided + ["--task", "densification", "--cfg", "RangeDM", "--decoder-guidance", "--scheduler", "ddpm"])
    with pytest.raises(NotImplementedError, match="DDIM"):
        IC.main(guided + ["--cfg", "RangeLDM", "--decoder-guidance", "--scheduler", "ddpm", "--jump-length", "2"])
    with pytest.raises(NotImplementedError, match="resample"):
        IC.main(guided + ["--cfg", "RangeLDM", "--decoder-guidance", "--jump-length", "2"])
    with pytest.raises(NotImplementedError, match="DPM-Solver"):
        IC.main(guided + ["--cfg", "RangeLDM", "--scheduler", "dpmsolver++"])
    # the config readers of inference.main and inference_conditional.main
    plain = tmp_path / "plain.yaml"
    plain.write_text("with_vae: True\nmodel_config:\n  sample_size: [256, 16]\n")
    with pytest.raises(NotImplementedError, match="all_circonv"):
        inference.main(["--cfg", str(plain), "--samples", "1", "--out", str(tmp_path / "o")])
    both = tmp_path / "both.yaml"
    both.write_text("all_circonv: True\nupsample: 4\ninpainting: 0.1\n")
    with pytest.raises(ValueError, match="exactly one"):
        IC.main(["--cfg", str(both), "--samples", "1", "--out", str(tmp_path / "o")])
    assert not (tmp_path / "o").exists()
