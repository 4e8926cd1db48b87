"""UNet training step (ldm/train_unconditional.py:466-558).

GPU: rangeldm_amd.training.UNetTrainer (HIP kernels behind the C ABI, host-side tape) against torch autograd +
torch.optim.AdamW on the oracle UNet (oracle/unet.py).  Tolerances: conv / linear operands are rounded to bf16
(`mixed_precision: bf16`), fp32 accumulation -- per-forward 2e-2 (the sampling path's gate), per-parameter gradients
4e-2 relative L2 and 1.5e-2 over all 3.5 M gradients at once.
CPU: bucket planning, lr / EMA schedules, min-SNR weights, and a world-size-2 gloo run of the bucketed averaging logic.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rangeldm_amd.config import UNetConfig
from rangeldm_amd.params import unet_param_shapes
from rangeldm_amd.synth import synth_state_dict
from rangeldm_amd import training as TR

SMALL = dict(sample_size=(32, 8), block_out_channels=(32, 32, 64, 64))


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def oracle_grads(cfg, sd, x, t, target, weights=None):
    from oracle import unet as o_unet
    sdt = {k: torch.from_numpy(np.array(v)).float().requires_grad_() for k, v in sd.items()}
    pred = o_unet.unet_forward.__wrapped__(sdt, cfg, x, t)
    if weights is None:
        loss = F.mse_loss(pred, target)
    else:
        loss = (F.mse_loss(pred, target, reduction="none").mean((1, 2, 3)) * weights).mean()
    loss.backward()
    return pred.detach(), float(loss), {k: v.grad for k, v in sdt.items()}


def test_schedules_and_buckets():
    b = TR.plan_buckets([10, 20, 5, 100, 1, 1], 30)
    assert b == [(0, 2, 0, 30), (2, 4, 30, 105), (4, 6, 135, 2)]
    assert sum(n for *_, n in b) == 137 and TR.plan_buckets([7], 100) == [(0, 1, 0, 7)]
    assert TR.cosine_lr(0, 1e-4, 500, 10000) == 0.0 and abs(TR.cosine_lr(250, 1e-4, 500, 10000) - 5e-5) < 1e-12
    assert abs(TR.cosine_lr(500, 1e-4, 500, 10000) - 1e-4) < 1e-12
    assert abs(TR.cosine_lr(5250, 1e-4, 500, 10000) - 5e-5) < 1e-12 and TR.cosine_lr(10000, 1e-4, 500, 10000) < 1e-12
    assert TR.ema_decay(1) == 0.0 and abs(TR.ema_decay(2) - (1 - 2 ** -0.75)) < 1e-12
    assert TR.ema_decay(10 ** 9) == 0.9999
    ac = torch.cumprod(1 - torch.linspace(1e-4, 0.02, 1000), 0)
    w = TR.snr_weights(ac, torch.tensor([0, 999]), 5.0)
    snr = ac / (1 - ac)
    assert abs(float(w[0]) - 5.0 / float(snr[0])) < 1e-6 and abs(float(w[1]) - 1.0) < 1e-6


def _gloo_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    sizes = [1000, 30, 5000, 7, 2000]
    buckets = TR.plan_buckets(sizes, 3000)
    flat = torch.arange(sum(sizes), dtype=torch.float32) * (rank + 1)
    pend = [torch.distributed.all_reduce(flat[off:off + n], async_op=True) for _, _, off, n in reversed(buckets)]
    for p in pend:
        p.wait()
    flat.mul_(1.0 / world)
    out[rank] = bool(torch.allclose(flat, torch.arange(sum(sizes), dtype=torch.float32) * (sum(range(1, world + 1)) / world)))
    torch.distributed.destroy_process_group()


def test_bucketed_gradient_average_world2_gloo():
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_gloo_worker, args=(2, 29611, out), nprocs=2, join=True)
    assert out[0] and out[1]


def test_fused_tape_shape_logic():
    """Which networks / input sizes the fused training blocks cover, and at which levels they run (host logic, no GPU)."""
    full = UNetConfig()
    _, groups = TR.plan_parameter_order(list(unet_param_shapes(full)), unet_param_shapes(full))
    assert TR.fused_tape_supported(full, groups, 8, 256, 16) and TR.fused_tape_supported(full, groups, 16, 256, 16)
    assert not TR.fused_tape_supported(full, groups, 17, 256, 16)           # the weight gradient's per-image coefficient table
    assert not TR.fused_tape_supported(full, groups, 8, 128, 8)             # the lowest level would be 16 pixels: tiles straddle images
    assert not TR.fused_tape_supported(full, groups, 8, 256, 32)            # 32 beams: outside the all-taps weight-gradient geometry
    assert not TR.fused_tape_supported(full, {k: v for k, v in groups.items() if k != "time_emb_proj_all"}, 8, 256, 16)
    small = UNetConfig(**SMALL)                                             # 32-channel levels: no 64-channel chunks
    _, g2 = TR.plan_parameter_order(list(unet_param_shapes(small)), unet_param_shapes(small))
    assert not TR.fused_tape_supported(small, g2, 2, 32, 8)
    assert TR.fused_levels(256, 16, 4, 1024) == [True, True, False, False] and TR.fused_levels(256, 16, 4, 0) == [True] * 4
    assert TR.fused_levels(64, 8, 2, 1024) == [False, False]


def test_parameter_order_makes_fused_groups_contiguous():
    """plan_parameter_order: a permutation of the state-dict names in which the weights (and the biases) of every fused group
    -- all time_emb_proj layers, to_q / to_k / to_v of each attention block -- are consecutive, so one [sum N][K] matrix in
    the flat fp32 buffers is the stacked Linear; bucket planning still covers every parameter once."""
    for cfg in (UNetConfig(), UNetConfig(**SMALL)):
        shapes = unet_param_shapes(cfg)
        names, fused = TR.plan_parameter_order(list(shapes), shapes)
        assert sorted(names) == sorted(shapes) and len(set(names)) == len(names)
        assert "time_emb_proj_all" in fused and len(fused) == 1 + sum(n.endswith("to_q.weight") for n in shapes)
        for key, grp in fused.items():
            for members in (grp["weights"], grp["biases"]):
                i = names.index(members[0])
                assert names[i:i + len(members)] == members, key
            assert len({shapes[m][1] for m in grp["weights"]}) == 1                    # one K for the stacked matrix
            assert [shapes[w][0] for w in grp["weights"]] == [shapes[b][0] for b in grp["biases"]]
        sizes = [int(np.prod(shapes[n])) for n in names]
        buckets = TR.plan_buckets(sizes, 1 << 20)
        assert buckets[0][0] == 0 and buckets[-1][1] == len(names) and sum(b[3] for b in buckets) == sum(sizes)
        assert all(buckets[i][1] == buckets[i + 1][0] for i in range(len(buckets) - 1))
        # the stacked time_emb_proj comes before the blocks that use it: its bucket is among the last to complete in backward
        assert names.index(fused["time_emb_proj_all"]["weights"][0]) < names.index("down_blocks.0.resnets.0.norm1.weight")


@pytest.mark.gpu
@pytest.mark.parametrize("kw,B,weights", [
    (dict(**SMALL), 2, None),
    (dict(sample_size=(16, 4), block_out_channels=(32, 64), down_block_types=("DownBlock2D", "AttnDownBlock2D"),
          up_block_types=("AttnUpBlock2D", "UpBlock2D")), 3, [0.3, 1.0, 0.6]),
    # the fused tape (round 5: GroupNorm inside its producers / consumers, concatenations read in place) needs 64-multiples of
    # channels and >= 64-pixel images at every level
    (dict(sample_size=(64, 8), block_out_channels=(64, 128), down_block_types=("DownBlock2D", "AttnDownBlock2D"),
          up_block_types=("AttnUpBlock2D", "UpBlock2D")), 2, [0.4, 1.0]),
])
def test_unet_gradients_match_autograd(kw, B, weights):
    cfg = UNetConfig(**kw)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, cfg.in_channels, *cfg.sample_size, generator=g)
    target = torch.randn(B, cfg.out_channels, *cfg.sample_size, generator=g)
    t = torch.tensor([17, 480, 977][:B])
    w = None if weights is None else torch.tensor(weights)
    pred_ref, loss_ref, gref = oracle_grads(cfg, sd, x, t, target, w)
    tr = TR.UNetTrainer(cfg, sd, use_ema=False)
    tr.fused_min_pixels = 0                     # (every level on the fused blocks where the shapes allow them)
    from rangeldm_amd import train_ops as T
    pred = tr.forward(x.cuda(), t.cuda())
    assert tr.last_forward_fused == (cfg.block_out_channels[0] == 64)
    assert rel(T.unpack_output(pred), pred_ref) < 2e-2
    loss, dpred = T.mse(pred, target.cuda(), None if w is None else w.cuda())
    assert abs(float(loss) - loss_ref) < 2e-2 * loss_ref
    tr.backward(dpred)
    flat_ref = torch.cat([gref[n].reshape(-1) for n in tr.names])
    rms = float(flat_ref.double().norm() / flat_ref.numel() ** 0.5)

    def err(n):
        # relative L2 with a floor: some gradients are analytically ZERO (a key bias shifts every score of a query equally
        # and softmax does not see it), so their reference norm is rounding noise
        # (the key bias's zero comes from sum_j dS_ij = 0, which bf16-rounded dS -- the matrix-core attention backward --
        # only honours to 2^-9 per term: its floor is three times higher)
        d = float((tr.g[n].double().cpu() - gref[n].double()).norm())
        floor = 6e-2 if n.endswith("to_k.bias") else 2e-2
        return d / (float(gref[n].double().norm()) + floor * rms * gref[n].numel() ** 0.5)
    ranked = sorted(((err(n), n) for n in tr.names), reverse=True)
    assert ranked[0][0] < 4e-2, ranked[:6]
    assert rel(tr.grads, flat_ref) < 1.5e-2
    # a second forward / backward accumulates into the same buffer (gradient accumulation)
    tr.backward(T.mse(tr.forward(x.cuda(), t.cuda()), target.cuda(), None if w is None else w.cuda())[1])
    assert rel(tr.grads, 2 * flat_ref) < 1.5e-2


@pytest.mark.gpu
def test_full_config_gradients_match_oracle_autograd():
    """BASELINE config 5's network at its real width (128 / 128 / 256 / 256 on 256x16 latents, 30.1 M parameters), batch 2, in the
    PRODUCTION routing (fused tape at the two high-resolution levels, op-per-layer tape below): every parameter gradient against
    torch autograd on the oracle UNet run on the host (the `accelerator.backward(loss)` of ldm/train_unconditional.py:545).  Gates
    at twice the measured errors (half the small configurations' gates)."""
    cfg = UNetConfig()
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="trfull.")
    g = torch.Generator().manual_seed(5)
    B = 2
    x = torch.randn(B, cfg.in_channels, *cfg.sample_size, generator=g)
    target = torch.randn(B, cfg.out_channels, *cfg.sample_size, generator=g)
    t = torch.tensor([40, 911])
    w = torch.tensor([0.5, 1.0])
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    pred_ref, loss_ref, gref = oracle_grads(cfg, sd, x, t, target, w)
    tr = TR.UNetTrainer(cfg, sd, use_ema=False)
    from rangeldm_amd import train_ops as T
    pred = tr.forward(x.cuda(), t.cuda())
    assert tr.last_forward_fused and tr.last_forward_fused_levels == [True, True, False, False]
    assert rel(T.unpack_output(pred), pred_ref) < 2e-2
    loss, dpred = T.mse(pred, target.cuda(), w.cuda())
    assert abs(float(loss) - loss_ref) < 2e-2 * loss_ref
    tr.backward(dpred)
    flat_ref = torch.cat([gref[n].reshape(-1) for n in tr.names])
    rms = float(flat_ref.double().norm() / flat_ref.numel() ** 0.5)

    def err(n):
        d = float((tr.g[n].double().cpu() - gref[n].double()).norm())
        floor = 6e-2 if n.endswith("to_k.bias") else 2e-2
        return d / (float(gref[n].double().norm()) + floor * rms * gref[n].numel() ** 0.5)
    ranked = sorted(((err(n), n) for n in tr.names), reverse=True)
    print("full-width gradient check: worst parameters", ranked[:4], "all", rel(tr.grads, flat_ref))
    # measured (round 6): worst parameter 9.0e-3 (down_blocks.3.attentions.0.to_q.bias), all 30.1 M gradients at once 4.2e-3
    assert ranked[0][0] < 2e-2, ranked[:6]
    assert rel(tr.grads, flat_ref) < 8e-3


@pytest.mark.gpu
def test_training_steps_follow_adamw_and_reduce_the_loss():
    """Ten steps on one fixed batch: the loss falls; the first two steps are checked against torch.optim.AdamW +
    clip_grad_norm_ + EMA driven by the oracle's autograd gradients."""
    cfg = UNetConfig(**SMALL)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 32, 8, generator=g)
    target = torch.randn(2, 4, 32, 8, generator=g)
    t = torch.tensor([100, 700])
    lr = 1e-3
    tr = TR.UNetTrainer(cfg, sd, lr=lr, lr_warmup_steps=0, total_steps=10 ** 6, use_ema=True)
    # reference: same loop with torch autograd on the oracle
    params = {k: torch.nn.Parameter(torch.from_numpy(np.array(v)).float()) for k, v in sd.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=lr, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    from oracle import unet as o_unet
    ema_ref = {k: v.detach().clone() for k, v in params.items()}
    losses = []
    for step in range(1, 11):
        losses.append(float(tr.train_step(x.cuda(), t.cuda(), target.cuda())))
        if step <= 2:
            opt.zero_grad()
            F.mse_loss(o_unet.unet_forward.__wrapped__(params, cfg, x, t), target).backward()
            torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
            opt.step()
            dec = TR.ema_decay(step)
            for k in ema_ref:
                ema_ref[k].sub_((1 - dec) * (ema_ref[k] - params[k].detach()))
            got = tr.state_dict()
            # Adam's first updates are +-lr whatever the gradient's size: a sign flip of a near-zero gradient moves a
            # parameter by 2 lr.  Gate the bulk (98 %) at half a step and the total at a small fraction of the update norm.
            d = torch.cat([(got[k] - params[k].detach()).reshape(-1) for k in tr.names]).abs()
            assert float((d > 0.5 * lr).float().mean()) < 0.02, (step, float((d > 0.5 * lr).float().mean()))
            upd = torch.cat([(params[k].detach() - torch.from_numpy(np.array(sd[k]))).reshape(-1) for k in tr.names])
            assert float(d.norm() / upd.norm()) < 0.15
            got_ema = tr.state_dict(ema=True)
            de = torch.cat([(got_ema[k] - ema_ref[k]).reshape(-1) for k in tr.names]).abs()
            assert float((de > 0.5 * lr).float().mean()) < 0.02
    assert losses[-1] < 0.8 * losses[0], losses
    assert all(math.isfinite(v) for v in losses)


@pytest.mark.gpu
def test_bucketed_allreduce_path_on_one_gpu(tmp_path):
    """The RCCL path with world size 1: bucket bookkeeping must launch every bucket exactly once and leave the gradients
    equal to the single-process ones; then save_pretrained -> sampling model round trip."""
    cfg = UNetConfig(**SMALL)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    x = torch.randn(2, 5, 32, 8, generator=torch.Generator().manual_seed(1)).cuda()
    target = torch.randn(2, 4, 32, 8, generator=torch.Generator().manual_seed(2)).cuda()
    t = torch.tensor([5, 900]).cuda()
    from rangeldm_amd import train_ops as T
    a = TR.UNetTrainer(cfg, sd, use_ema=False, bucket_mb=1)
    a.backward(T.mse(a.forward(x, t), target)[1], reduce=False)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29612", RANK="0", WORLD_SIZE="1")
    torch.distributed.init_process_group("nccl", rank=0, world_size=1)
    try:
        b = TR.UNetTrainer(cfg, sd, use_ema=True, bucket_mb=1)
        assert len(b.buckets) >= 3
        b.backward(T.mse(b.forward(x, t), target)[1], reduce=True)
        assert all(r == 0 for r in [0])                               # (buckets all fired: pending handles were waited)
        # a bucket reduced too early or twice would be off by O(1).  Run to run the gradients agree to ~6e-9 (split-K fp32 atomics
        # reorder sums) -- except that in about 1 run of 100 that last-bit noise flips the bf16 rounding of one activation on its way
        # into a conv (a 0.2 % change of that operand), which shows as 1e-4 .. 2.5e-3 of the gradient norm, with or without a
        # collective (tools/flaky_probe.py finds the runs, tools/flaky_bisect.py the op and the pixel)
        assert rel(b.grads, a.grads) < 5e-3
        b.optimizer_step()
    finally:
        torch.distributed.destroy_process_group()
    b.save_pretrained(str(tmp_path))
    from rangeldm_amd.unet import UNet2DModelHIP
    m = UNet2DModelHIP.from_pretrained(str(tmp_path), subfolder="unet_ema")
    assert torch.isfinite(m(x, 10).sample).all()


@pytest.mark.gpu
def test_save_state_resume_and_gradient_accumulation(tmp_path):
    """accelerator.save_state / load_state and gradient_accumulation_steps (ldm/train_unconditional.py:449-463,466,560-584):
    a resumed trainer continues exactly where the saved one was (moments, EMA, lr / EMA warm-up position), and two
    half-batches accumulated give the step of the whole batch."""
    cfg = UNetConfig(**SMALL)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    lr = 1e-3
    kw = dict(lr=lr, lr_warmup_steps=3, total_steps=40, use_ema=True)
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(4, 5, 32, 8, generator=g).cuda(), torch.randint(0, 1000, (4,), generator=g).cuda(),
                torch.randn(4, 4, 32, 8, generator=g).cuda()) for _ in range(4)]
    a = TR.UNetTrainer(cfg, sd, **kw)
    for x, t, y in batches[:2]:
        a.train_step(x, t, y)
    a.save_state(str(tmp_path / "state.pt"))
    assert set(torch.load(str(tmp_path / "state.pt"), map_location="cpu", weights_only=True)) == {
        "params", "exp_avg", "exp_avg_sq", "global_step", "names", "ema", "micro", "grads", "hp"}
    for x, t, y in batches[2:]:
        a.train_step(x, t, y)
    b = TR.UNetTrainer(cfg, synth_state_dict(unet_param_shapes(cfg), prefix="other."), **kw)      # different weights: all restored
    b.load_state(str(tmp_path / "state.pt"))
    assert b.global_step == 2
    for x, t, y in batches[2:]:
        b.train_step_graphed(x, t, y)                                # (and the device-side step counter was resynchronised)
    _adam_close(a.state_dict(), b.state_dict(), lr, "resumed parameters")
    _adam_close(a.state_dict(ema=True), b.state_dict(ema=True), lr, "resumed ema")
    # accumulation: 2 x (batch 2) == 1 x (batch 4)
    c = TR.UNetTrainer(cfg, sd, **kw)
    d = TR.UNetTrainer(cfg, sd, gradient_accumulation_steps=2, **kw)
    for x, t, y in batches[:2]:
        c.train_step(x, t, y)
        d.train_step(x[:2], t[:2], y[:2])
        assert d.global_step == c.global_step - 1                    # no optimizer step inside the window
        d.train_step(x[2:], t[2:], y[2:])
    assert d.global_step == c.global_step == 2
    _adam_close(c.state_dict(), d.state_dict(), lr, "accumulated parameters")
    with pytest.raises(NotImplementedError):
        d.train_step_graphed(*batches[0])


@pytest.mark.gpu
def test_cabi_collectives_on_one_gpu(monkeypatch):
    """rldm_comm_* / rldm_allgather_images / rldm_allreduce_grads (RCCL bound at run time behind the C ABI) with world size 1:
    the communicator comes up on the RCCL copy the process already holds, the collectives run on the current stream, and the
    trainer's bucketed path gives the single-process gradients when it goes through them (RLDM_COLLECTIVE=cabi)."""
    from rangeldm_amd import distributed as D, train_ops as T
    comm = D.Communicator(rank=0, world=1)
    assert "rccl" in comm.rccl_origin()
    img = torch.randn(3, 2, 64, 8, device="cuda")
    out = comm.all_gather_images(img)
    g = torch.randn(1000, device="cuda")
    ref = g.clone()
    comm.all_reduce_grads(g, average=True)
    torch.cuda.synchronize()
    assert torch.equal(out, img) and torch.equal(g, ref)
    del comm
    cfg = UNetConfig(**SMALL)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    x = torch.randn(2, 5, 32, 8, generator=torch.Generator().manual_seed(1)).cuda()
    target = torch.randn(2, 4, 32, 8, generator=torch.Generator().manual_seed(2)).cuda()
    t = torch.tensor([5, 900]).cuda()
    a = TR.UNetTrainer(cfg, sd, use_ema=False, bucket_mb=1)
    a.backward(T.mse(a.forward(x, t), target)[1], reduce=False)
    monkeypatch.setenv("RLDM_COLLECTIVE", "cabi")
    monkeypatch.setattr(D, "_COMM", None)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29614", RANK="0", WORLD_SIZE="1")
    torch.distributed.init_process_group("gloo", rank=0, world_size=1)      # (rendezvous only: the bytes go through the C ABI)
    try:
        b = TR.UNetTrainer(cfg, sd, use_ema=False, bucket_mb=1)
        world = b.backward(T.mse(b.forward(x, t), target)[1], reduce=True)
        torch.cuda.synchronize()
        assert world == 1 and D._COMM is not None                    # averaged inside the collective, on the C-ABI communicator
        assert rel(b.grads, a.grads) < 5e-3                           # (see test_bucketed_allreduce_path_on_one_gpu)
        full = D.all_gather_images(img)                               # world 1: returned as is
        assert full is img
    finally:
        torch.distributed.destroy_process_group()
        D._COMM = None


@pytest.mark.gpu
def test_operand_repack_tiled_equals_elementwise():
    """The tiled transpose (one launch, all layers incl. the fused groups and the 5- / 4-channel ends with their zero pads)
    writes exactly the bytes of the per-layer kernel."""
    from rangeldm_amd import train_ops as T
    cfg = UNetConfig(**SMALL)
    tr = TR.UNetTrainer(cfg, synth_state_dict(unet_param_shapes(cfg), prefix="tr."), use_ema=False)
    for wf in tr.wf.values():
        wf.fill_(7.0)
    for wt in tr.wt.values():
        if wt is not None:
            wt.fill_(7.0)
    tr.repack(tiled=True)
    got = {n: (tr.wf[n].clone(), None if tr.wt[n] is None else tr.wt[n].clone()) for n in tr.wf}
    tr.repack(tiled=False)
    for n, (N, Cin, taps, off, need_t) in tr.layers.items():
        w = tr.params[off:off + N * Cin * taps].view(N, Cin, taps)
        wf, wt = T.pack_weights(w, taps)
        assert torch.equal(got[n][0].view(torch.int16), wf.view(torch.int16)), n
        assert torch.equal(tr.wf[n].view(torch.int16), wf.view(torch.int16)), n
        if need_t:
            assert torch.equal(got[n][1].view(torch.int16), wt.view(torch.int16)), n


def _adam_close(a, b, lr, what):
    """parameters of two runs agree: a sign flip of a near-zero gradient moves an Adam parameter by 2 lr, nothing else may"""
    d = torch.cat([(a[k] - b[k]).reshape(-1) for k in a]).abs()
    frac = float((d > 0.5 * lr).float().mean())
    assert frac < 0.01, (what, frac)


@pytest.mark.gpu
def test_graphed_steps_equal_eager_steps():
    """train_step_graphed (captured HIP graphs, step number / lr / bias corrections / EMA decay computed on the device) against
    train_step (every launch from the host, scalars from the host) over six different batches, lr warm-up included."""
    cfg = UNetConfig(**SMALL)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    lr = 1e-3
    kw = dict(lr=lr, lr_warmup_steps=3, total_steps=40, use_ema=True)
    a, b = TR.UNetTrainer(cfg, sd, **kw), TR.UNetTrainer(cfg, sd, **kw)
    g = torch.Generator().manual_seed(11)
    for step in range(1, 7):
        x = torch.randn(2, 4, 32, 8, generator=g).cuda()
        target = torch.randn(2, 4, 32, 8, generator=g).cuda()
        t = torch.randint(0, 1000, (2,), generator=g).cuda()
        w = torch.rand(2, generator=g).cuda()
        la = a.train_step(x, t, target, w, pos_encoding=True)
        lb = b.train_step_graphed(x, t, target, w, pos_encoding=True)
        assert abs(float(la) - float(lb)) < (1e-4 if step == 1 else 1e-2) * abs(float(la)), (step, float(la), float(lb))
        assert a.global_step == b.global_step == step
        if step >= 2:                                     # (step 1 of the graphed trainer is the eager sizing step)
            dyn = b._dyn.cpu()
            assert abs(float(dyn[0]) - TR.cosine_lr(step - 1, lr, 3, 40)) < 1e-9
            assert abs(float(dyn[1]) - (1 - 0.95 ** step)) < 1e-6 and abs(float(dyn[2]) - (1 - 0.999 ** step)) < 1e-7
            assert abs(float(dyn[3]) - TR.ema_decay(step)) < 1e-6
            assert int(b._step_dev) == step
    assert len(b._graphs) == 1 and len(next(iter(b._graphs.values()))["segments"]) == 1
    _adam_close(a.state_dict(), b.state_dict(), lr, "parameters")
    _adam_close(a.state_dict(ema=True), b.state_dict(ema=True), lr, "ema")
    assert abs(float(a.last_grad_norm) - float(b.last_grad_norm)) < 2e-2 * float(a.last_grad_norm)   # (two chaotic trajectories)
    # mixing the two kinds of step keeps the device step counter in line
    x = torch.randn(2, 4, 32, 8, generator=g).cuda()
    a.train_step(x, t, target, w, pos_encoding=True)
    b.train_step(x, t, target, w, pos_encoding=True)
    a.train_step(x, t, target, w, pos_encoding=True)
    b.train_step_graphed(x, t, target, w, pos_encoding=True)
    assert int(b._step_dev) == b.global_step == 8
    _adam_close(a.state_dict(), b.state_dict(), lr, "parameters after mixed steps")
    # a larger batch grows the library's scratch buffers (sizing step, capture, replay); the batch-2 graph captured before the growth
    # still holds the outgrown blocks' addresses, and replaying it afterwards must find them allocated
    for B in (32, 32, 32, 2):
        x, target = torch.randn(B, 4, 32, 8, generator=g).cuda(), torch.randn(B, 4, 32, 8, generator=g).cuda()
        t, w = torch.randint(0, 1000, (B,), generator=g).cuda(), torch.rand(B, generator=g).cuda()
        a.train_step(x, t, target, w, pos_encoding=True)
        b.train_step_graphed(x, t, target, w, pos_encoding=True)
    assert len(b._graphs) == 2 and int(b._step_dev) == b.global_step == 12
    _adam_close(a.state_dict(), b.state_dict(), lr, "parameters after a larger batch")
    _adam_close(a.state_dict(ema=True), b.state_dict(ema=True), lr, "ema after a larger batch")


@pytest.mark.gpu
def test_graphed_full_config_matches_eager():
    """RangeLDM-size UNet, batch 4: five steps replayed from the captured graph against five eager steps (the large-tensor paths
    -- slab GroupNorm, split-K convs, all-taps weight gradient -- only exist at this size; a memset node inside the graph once
    replayed wrongly from the second replay on, which only this comparison sees)."""
    cfg = UNetConfig()
    sd = synth_state_dict(unet_param_shapes(cfg))
    kw = dict(lr=1e-4, lr_warmup_steps=2, total_steps=100, use_ema=True)
    a, b = TR.UNetTrainer(cfg, sd, **kw), TR.UNetTrainer(cfg, sd, **kw)
    g = torch.Generator().manual_seed(5)
    for step in range(1, 6):
        x = torch.randn(4, 4, 256, 16, generator=g).cuda()
        target = torch.randn(4, 4, 256, 16, generator=g).cuda()
        t = torch.randint(0, 1000, (4,), generator=g).cuda()
        la = float(a.train_step(x, t, target, pos_encoding=True))
        lb = float(b.train_step_graphed(x, t, target, pos_encoding=True))
        na, nb = float(a.last_grad_norm) ** 0.5, float(b.last_grad_norm) ** 0.5
        assert math.isfinite(lb) and abs(la - lb) < 2e-3 * abs(la), (step, la, lb)
        assert abs(na - nb) < 2e-2 * na, (step, na, nb)
    d = (a.params - b.params).abs()
    assert float((d > 0.5e-4).float().mean()) < 0.02


@pytest.mark.gpu
def test_graphed_steps_cut_at_gradient_buckets_on_one_gpu():
    """The multi-rank form of the captured step with world size 1: one graph per gradient bucket, the RCCL all-reduce of a
    bucket launched between the replays, the optimizer segment after the waits -- same parameters as eager steps."""
    cfg = UNetConfig(**SMALL)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    lr = 1e-3
    kw = dict(lr=lr, lr_warmup_steps=0, total_steps=100, use_ema=True, bucket_mb=1)
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(2, 5, 32, 8, generator=g).cuda(), torch.randint(0, 1000, (2,), generator=g).cuda(),
                torch.randn(2, 4, 32, 8, generator=g).cuda()) for _ in range(4)]
    a = TR.UNetTrainer(cfg, sd, **kw)
    for x, t, target in batches:
        a.train_step(x, t, target)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29613", RANK="0", WORLD_SIZE="1")
    torch.distributed.init_process_group("nccl", rank=0, world_size=1)
    try:
        b = TR.UNetTrainer(cfg, sd, **kw)
        for x, t, target in batches:
            b.train_step_graphed(x, t, target, reduce=True)
        torch.cuda.synchronize()
        segs = next(iter(b._graphs.values()))["segments"]
        assert [act for _, act in segs] == list(range(len(b.buckets) - 1, -1, -1)) + ["wait", None]
    finally:
        torch.distributed.destroy_process_group()
    _adam_close(a.state_dict(), b.state_dict(), lr, "parameters")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["--eager", "--graphed", "--full"])
def test_two_data_parallel_ranks_on_one_gpu(mode):
    """tools/dp_probe.py: two real ranks (gloo on device tensors; RCCL refuses two ranks per device) through the eager and the
    captured, bucket-cut step: identical parameters on both ranks, equal to one process trained on the concatenated batch."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29541 + ["--eager", "--graphed", "--full"].index(mode)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tools", "dp_probe.py")] + ([mode] if mode != "--graphed" else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "max |rank0 - rank1| = 0.000e+00" in r.stdout, r.stdout[-1000:]


@pytest.mark.gpu
def test_training_step_loop_body_unconditional_and_conditional():
    """`training_step` = the loop body of ldm/train_unconditional.py:479-556 (VAE encode + sample, add_noise, pos-encoding,
    min-SNR weights) and its conditional twin (ldm/train_conditional.py:418-447, upsample: 4 + 8 folded-condition channels)."""
    from rangeldm_amd.encoders import SparseRangeImageEncoder2
    from rangeldm_amd.config import VAEConfig
    from rangeldm_amd.params import vae_param_shapes
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    from rangeldm_amd.vae import AutoencoderKLHIP
    vae = AutoencoderKLHIP(VAEConfig())
    vae.load_state_dict(synth_state_dict(vae_param_shapes(VAEConfig()), prefix="vae."))
    sched = DDPMSchedulerHIP()
    g = torch.Generator().manual_seed(9)
    imgs = torch.randn(2, 2, 128, 32, generator=g) * 0.5
    cfg = UNetConfig(sample_size=(32, 8), in_channels=5, block_out_channels=(32, 32, 64, 64))
    tr = TR.UNetTrainer(cfg, synth_state_dict(unet_param_shapes(cfg), prefix="tr."), lr_warmup_steps=0, lr=1e-3)
    l0 = [float(TR.training_step(tr, vae, sched, imgs.cuda(), generator=torch.Generator().manual_seed(1), pos_encoding=True,
                                 snr_gamma=5.0)) for _ in range(6)]
    assert all(math.isfinite(v) for v in l0) and l0[-1] < l0[0]       # same noise / timesteps every call: it must fall
    cfg_c = UNetConfig(sample_size=(32, 8), in_channels=12, block_out_channels=(32, 32, 64, 64))
    trc = TR.UNetTrainer(cfg_c, synth_state_dict(unet_param_shapes(cfg_c), prefix="trc."), lr_warmup_steps=0, lr=1e-3)
    down = torch.randn(2, 2, 128, 8, generator=g)
    cond = SparseRangeImageEncoder2()(down)
    assert tuple(cond.shape) == (2, 8, 32, 8)
    l1 = [float(TR.training_step(trc, vae, sched, imgs.cuda(), generator=torch.Generator().manual_seed(1), pos_encoding=False,
                                 condition=cond)) for _ in range(6)]
    assert all(math.isfinite(v) for v in l1) and l1[-1] < l1[0]
    # v_prediction (ldm/train_unconditional.py:505-510, :532-534): the target is the velocity, the min-SNR weights use SNR + 1; the
    # first loss of a step on given latents / noise / timesteps equals the oracle's, computed from the same model output
    from rangeldm_amd.config import SchedulerConfig
    from oracle.schedulers import OracleDDPMScheduler
    from rangeldm_amd import train_ops as T
    sv = DDPMSchedulerHIP(SchedulerConfig(prediction_type="v_prediction"))
    trv = TR.UNetTrainer(cfg, synth_state_dict(unet_param_shapes(cfg), prefix="tr."), lr_warmup_steps=0, lr=1e-3)
    lat = torch.randn(2, 4, 32, 8, generator=g)
    noise = torch.randn(2, 4, 32, 8, generator=g)
    ts = torch.tensor([120, 870])
    pe = torch.zeros(2, 1, 32, 8)
    pe[:, :, 0, :] = 1
    pred = T.unpack_output(trv.forward(torch.cat([sv.add_noise(lat.cuda(), noise.cuda(), ts).cpu(), pe], 1).cuda(), ts.cuda())).cpu()
    target = OracleDDPMScheduler(SchedulerConfig(prediction_type="v_prediction")).get_velocity(lat, noise, ts)
    w = TR.snr_weights(sv.alphas_cumprod, ts, 5.0, v_prediction=True)
    want = float(((pred - target) ** 2).mean((1, 2, 3)).mul(w).mean())
    got = float(TR.training_step(trv, None, sv, lat.cuda(), pos_encoding=True, snr_gamma=5.0, noise=noise.cuda(), timesteps=ts))
    assert abs(got - want) < 2e-3 * want, (got, want)
    with pytest.raises(ValueError, match="Unknown prediction type"):
        TR.training_step(trv, None, DDPMSchedulerHIP(SchedulerConfig(prediction_type="sample")), lat.cuda(), noise=noise.cuda(), timesteps=ts)


@pytest.mark.gpu
def test_fused_tape_equals_layer_tape_full_config():
    """BASELINE config-5 shapes, batch 2: the fused tape (3 launches per resnet forward; GroupNorm only inside conv kernels) against
    the op-per-layer tape (fused_tape = False) on the same weights: same prediction and same gradients up to the bf16
    rounding of operands (z = x a + b against ((x - mean) rstd) gamma + beta: last-bit differences in fp32 flip bf16 roundings, which
    a 60-conv network amplifies to 4e-3 on the prediction) and the order of the fp32 atomics."""
    from rangeldm_amd import train_ops as T
    cfg = UNetConfig()
    sd = synth_state_dict(unet_param_shapes(cfg))
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 4, 256, 16, generator=g).cuda()
    target = torch.randn(2, 4, 256, 16, generator=g).cuda()
    t = torch.tensor([101, 902]).cuda()
    out = []
    for fused, min_px in ((True, 0), (False, 0), (True, 1024)):
        tr = TR.UNetTrainer(cfg, sd, use_ema=False)
        tr.fused_tape, tr.fused_min_pixels = fused, min_px
        pred = tr.forward(x, t, pos_encoding=True)
        assert tr.last_forward_fused == fused
        assert tr.last_forward_fused_levels == ([fused] * 4 if min_px == 0 else [True, True, False, False])
        loss, dpred = T.mse(pred, target)
        tr.backward(dpred)
        out.append((pred.clone(), float(loss), tr.grads.clone(), {n: tr.g[n].clone() for n in tr.names}))
    (pa, la, ga, da), (pb, lb, gb, db), (pc, lc, gc, dc) = out
    # (the default: fused blocks at the two high-resolution levels, op-per-layer blocks below)
    assert rel(pc, pb) < 8e-3 and abs(lc - lb) < 2e-3 * lb and rel(gc, gb) < 2e-2, (rel(pc, pb), lc, lb, rel(gc, gb))
    assert rel(pa, pb) < 8e-3 and abs(la - lb) < 2e-3 * lb, (rel(pa, pb), la, lb)
    assert rel(ga, gb) < 2e-2, rel(ga, gb)
    rms = float(gb.double().norm() / gb.numel() ** 0.5)
    worst = sorted(((float((da[n].double() - db[n].double()).norm()) /
                     (float(db[n].double().norm()) + 2e-2 * rms * db[n].numel() ** 0.5), n) for n in da), reverse=True)
    assert worst[0][0] < 5e-2, worst[:6]
    print('fused vs layer tape:', rel(pa, pb), rel(ga, gb), worst[:3])


@pytest.mark.gpu
def test_grouped_weight_gradients_equal_per_layer_launches():
    """(round 6) BASELINE config-5 shapes, batch 2: the weight gradients of the step queued and run as grouped launches
    (rldm_train_wgrad_group: block id -> layer, tile, K slice; the slices of a tile summed by its last arriver) against one launch
    per layer where the tape reaches it.  Same kernels' body on the same operands: the differences are the K-slice boundaries and the
    summation order of fp32 partial sums (and the atomics of the data path: the two runs are two runs).  Also: nothing stays queued
    behind backward, a second backward accumulates (the ticket counters re-arm), and the step captured in graphs replays it."""
    from rangeldm_amd import train_ops as T
    cfg = UNetConfig()
    sd = synth_state_dict(unet_param_shapes(cfg))
    g = torch.Generator().manual_seed(33)
    x = torch.randn(2, 4, 256, 16, generator=g).cuda()
    target = torch.randn(2, 4, 256, 16, generator=g).cuda()
    t = torch.tensor([77, 640]).cuda()
    grads = []
    for grouped in (True, False):
        tr = TR.UNetTrainer(cfg, sd, use_ema=False)
        tr.wgrad_group = grouped
        loss, dpred = T.mse(tr.forward(x, t, pos_encoding=True), target)
        tr.backward(dpred)
        assert T.wgrad_group_pending() == 0
        g1 = tr.grads.clone()
        tr.backward(T.mse(tr.forward(x, t, pos_encoding=True), target)[1])
        assert rel(tr.grads, 2 * g1) < 5e-3                     # (the gate of the run-to-run comparisons of this file)
        grads.append((g1, {n: tr.g[n].clone() * 0.5 for n in tr.names}))
    (ga, da), (gb, db) = grads
    assert rel(ga, gb) < 5e-3, rel(ga, gb)
    rms = float(gb.double().norm() / gb.numel() ** 0.5)
    worst = sorted(((float((da[n].double() - db[n].double()).norm()) /
                     (float(db[n].double().norm()) + 2e-2 * rms * db[n].numel() ** 0.5), n) for n in da), reverse=True)
    print("grouped vs per-layer weight gradients:", rel(ga, gb), worst[:3])
    assert worst[0][0] < 1e-2, worst[:6]


@pytest.mark.gpu
def test_full_config_gradient_is_the_directional_derivative():
    """BASELINE config-5 shapes (RangeLDM UNet, 256 x 16 latents, batch reduced to 2): a size-independent property instead of
    the CPU oracle -- along the gradient direction the loss must change at the rate |g|:
    (L(w + e g/|g|) - L(w - e g/|g|)) / (2 e) = |g| up to O(e^2) and the bf16 operand rounding of the forward passes."""
    from rangeldm_amd import train_ops as T
    cfg = UNetConfig()
    sd = synth_state_dict(unet_param_shapes(cfg))
    tr = TR.UNetTrainer(cfg, sd, use_ema=False)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 4, 256, 16, generator=g).cuda()
    target = torch.randn(2, 4, 256, 16, generator=g).cuda()
    t = torch.tensor([333, 871]).cuda()

    def loss_at():
        tr.repack()
        return float(T.mse(tr.forward(x, t, pos_encoding=True), target)[0])
    loss0, dpred = T.mse(tr.forward(x, t, pos_encoding=True), target)
    tr.backward(dpred)
    grad = tr.grads.clone()
    assert torch.isfinite(grad).all() and float(loss0) > 0
    gn = float(grad.double().norm())
    assert gn > 0
    eps = 0.02
    w0 = tr.params.clone()
    tr.params.copy_(w0 + eps * grad / gn)
    lp = loss_at()
    tr.params.copy_(w0 - eps * grad / gn)
    lm = loss_at()
    tr.params.copy_(w0)
    slope = (lp - lm) / (2 * eps)
    assert abs(slope / gn - 1) < 0.1, (slope, gn, float(loss0), lp, lm)
    # every parameter received a gradient (no dead branch in the tape), including both ends of the network
    for n in ("conv_in.weight", "time_embedding.linear_1.weight", "mid_block.attentions.0.to_q.weight",
              "up_blocks.3.resnets.2.conv_shortcut.weight", "conv_out.bias", "down_blocks.1.downsamplers.0.conv.weight",
              "up_blocks.0.upsamplers.0.conv.weight"):
        assert float(tr.g[n].abs().max()) > 0, n
