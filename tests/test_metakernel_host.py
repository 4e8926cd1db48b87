"""CPU: the host half of rangeldm_amd/metakernel.py against the reference's Meta-Kernel discriminator as recorded in
tests/golden/metakernel.npz (tools/make_metakernel_golden.py), and its numpy / torch statements against torch autograd.

Gate of test_forward_host_reproduces_the_golden: forward_host states the same arithmetic as the reference module with other torch
ops (index gathers instead of pad + unfold, the coov weight permuted instead of the patches), so the two differ by fp32 rounding of
differently ordered sums alone.  The golden records the reference against itself with 1 thread and with all threads (`threads_rel`,
2e-6 .. 7e-6 relative L2 where it was written); the gate is max(that, 1e-5) relative L2 per array, tests/test_discriminator_host.py's
rule.  The parameters of `null_grads` (a coov.bias in front of a BatchNorm) have a gradient of exactly zero in exact arithmetic and
rounding noise in the recording (norms of 1e-8 .. 1e-6, different from run to run), so a relative distance means nothing for them:
they are bounded instead, at 1e-4 of the gradient norm of the BatchNorm bias behind them -- the sum of the same dy BEFORE the
normalisation's backward took its mean out; fp32 cancellation leaves about 1e-7 of it per term, the recording's own noise is at
1e-5 of it or below."""
import numpy as np
import pytest
import torch

from rangeldm_amd import discriminator as D
from rangeldm_amd import metakernel as MK
from tests.disc_util import META as U


def test_keys_are_the_reference_modules():
    keys = [str(k) for k in U.golden()["keys"]]
    assert list(MK.param_shapes(MK.MetaKernelConfig())) == keys
    sd = MK.init_state(MK.MetaKernelConfig(), 0)
    assert list(sd) == keys
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in MK.param_shapes().items())
    got = MK.config_from_state(sd)
    assert (got.in_channels, got.ndf, got.n_layers) == (2, 64, 3)
    assert abs(got.azi - 0.00613592) < 1e-8 and abs(got.inc - 0.0074594) < 1e-8
    names = MK.trainable_names()
    assert [k for k in keys if not k.endswith(D.BUFFER_SUFFIXES + MK.TABLE_SUFFIXES)] == names
    assert sd["main.0.cos_azi"].shape == (1, 1, 1, 1, 4, 4) and sd["main.3.num_batches_tracked"].dtype == torch.int64
    assert MK.output_size(None, 1024, 64) == (126, 6) and MK.output_size(None, 32, 24) == (2, 1) and MK.output_size(None, 64, 32) == (6, 2)
    specs = MK.layer_specs()
    assert [(L["name"], L["cin"], L["cout"], L["stride"]) for L in specs] == [("main.0", 2, 64, 2), ("main.2", 64, 128, 2), ("main.5", 128, 256, 2),
                                                                             ("main.8", 256, 512, 1), ("main.11", 512, 1, 1)]
    assert [L["azi"] / 0.00613592 for L in specs] == [1, 2, 4, 8, 8] and [L["bn"] for L in specs] == [None, "main.3", "main.6", "main.9", None]
    with pytest.raises(NotImplementedError, match="log"):
        MK.MetaKernelConfig(log=True)


def test_init_state_is_seeded_and_follows_the_reference():
    a, b = MK.init_state(None, 3), MK.init_state(None, 3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["main.2.coov.weight"], MK.init_state(None, 4)["main.2.coov.weight"])
    w = a["main.8.coov.weight"]                                  # 2 M values: the sample moments are tight
    assert abs(float(w.mean())) < 1e-4 and abs(float(w.std()) - 0.02) < 1e-4
    g = a["main.9.weight"]
    assert abs(float(g.mean()) - 1.0) < 5e-3 and abs(float(g.std()) - 0.02) < 3e-3 and float(a["main.9.bias"].abs().max()) == 0.0
    for k, fan_in in (("main.0.mlp_coord.0.weight", 3), ("main.5.mlp_coord.0.bias", 3), ("main.5.mlp_coord.2.weight", 128),
                      ("main.5.mlp_coord.2.bias", 128), ("main.8.coov.bias", 16 * 256)):
        bound = 1.0 / np.sqrt(fan_in)
        assert 0.8 * bound < float(a[k].abs().max()) <= bound, k


def test_tables_are_the_references_bits():
    """init_state's tables against the ones the reference's constructor built (recorded before the state was loaded)."""
    g, sd = U.golden(), MK.init_state(None, 0)
    recorded = [k for k in g if k.startswith("ref_table.")]
    assert len(recorded) == 20
    for k in recorded:
        assert np.array_equal(g[k].view(np.uint32), sd[k[len("ref_table."):]].numpy().view(np.uint32)), k
    t = MK.make_tables(0.5, 0.25)
    assert float(t["cos_azi"][0, 0, 0, 0, 1, 2]) == 1.0 and float(t["sin_azi"][0, 0, 0, 0, 0, 3]) == float(torch.sin(torch.Tensor([0.5])))
    assert float(t["sin_inc"][0, 0, 0, 0, 0, 1]) == float(torch.sin(torch.Tensor([0.25]) * -2))     # inc goes with shift_h, the first index


@pytest.mark.parametrize("ndf,W,H", U.CASES)
def test_forward_host_reproduces_the_golden(ndf, W, H):
    gc, hc = U.golden_case(ndf, W, H), U.host_case(ndf, W, H)
    gate = max(float(gc["threads_rel"]), 1e-5)
    null = [str(k) for k in U.golden()["null_grads"]]
    worst = {}
    for k in ("logits_real", "logits_fake"):
        assert tuple(hc[k].shape) == gc[k].shape
        worst[k] = U.rel(hc[k], gc[k])
    for k in ("d_loss", "g_loss"):
        worst[k] = abs(hc[k] - float(gc[k])) / abs(float(gc[k]))
    for k, v in gc.items():
        if k.startswith(("d_grad.", "g_grad.")):
            full = hc[k.replace("_grad.", "_full.")]
            name = k[7:]
            if name in null:
                bn = "main.%d.bias" % (int(name.split(".")[1]) + 1)
                bound = 1e-4 * float(gc[f"{k[0]}_norm.{bn}"])
                assert float(full.double().norm()) <= bound and float(gc[k[0] + "_norm." + name]) <= bound, (k, float(full.norm()), bound)
                continue
            worst[k] = U.rel(U.sampled(full), v)
            nk = k.replace("_grad.", "_norm.")
            worst[nk] = abs(float(full.double().norm()) - float(gc[nk])) / (float(gc[nk]) + 1e-30)
            if name in ("real", "fake"):
                for c in (0, 1):
                    worst[f"{nk}.c{c}"] = abs(float(full[:, c].double().norm()) - float(gc[f"{nk}.c{c}"])) / float(gc[f"{nk}.c{c}"])
        elif k.startswith("buf."):
            if k.endswith("num_batches_tracked"):
                assert int(hc[k]) == int(v) == 2
            else:
                worst[k] = U.rel(hc[k], v)
    assert sum(k.startswith("d_grad.") for k in gc) == len(MK.trainable_names(MK.MetaKernelConfig(ndf=ndf))) + 2      # every parameter, both inputs
    assert sum(k.startswith("g_grad.") for k in gc) == len(MK.trainable_names(MK.MetaKernelConfig(ndf=ndf))) + 1
    bad = {k: v for k, v in worst.items() if not v <= gate}
    print(f"ndf {ndf} {W}x{H}: worst {max(worst.values()):.2e} ({max(worst, key=worst.get)}), gate {gate:.1e}")
    assert not bad, bad


def test_the_range_path_carries_gradient():
    """With r detached the logits are the same, channel 1's input gradient is the same and channel 0's is not: the gradient that
    reaches the range channel through pe -> MLP -> m is real (more than a tenth of channel 0's gradient, in relative L2)."""
    full, cut = U.host_case(16, 32, 24), U.host_case(16, 32, 24, detach_r=True)
    assert torch.equal(full["logits_fake"], cut["logits_fake"])
    for k in ("d_full.real", "d_full.fake", "g_full.fake"):
        assert torch.equal(full[k][:, 1], cut[k][:, 1]), k
        assert U.rel(cut[k][:, 0], full[k][:, 0]) > 0.1, k
    for k in full:
        if k.startswith("d_full.main."):
            assert torch.equal(full[k], cut[k]), k                # (the parameters' gradients do not pass through r's own graph)


def _random_layer(seed, B, W, H, Cc, N):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    return dict(x=rn(B, Cc, W, H), r=torch.rand(B, 1, W, H, generator=g, dtype=torch.float64) * 6, tabs=[rn(4, 4) for _ in range(4)],
                w1=rn(Cc, 3), b1=rn(Cc), w2=rn(Cc, Cc), b2=rn(Cc), coov=rn(N, 16 * Cc, 1, 1) * 0.3, bias=rn(N))


@pytest.mark.parametrize("B,W,H,Cc,N,stride", [(2, 8, 6, 4, 5, 2), (1, 5, 3, 3, 2, 1), (2, 7, 5, 2, 3, 2), (1, 4, 3, 6, 1, 1)])
def test_host_statements_against_autograd_in_fp64(B, W, H, Cc, N, stride):
    """pe_host, mlp_host, modconv_host (through layer_host) against autograd of the torch layer: output, returned r and all eight
    gradients, the next layer's dr included; then each statement on its own."""
    p = {k: ([t.clone().requires_grad_() for t in v] if k == "tabs" else v.clone().requires_grad_()) for k, v in _random_layer(5, B, W, H, Cc, N).items()}
    y, rn = MK._layer_torch(p["x"], p["r"], p["tabs"], p["w1"], p["b1"], p["w2"], p["b2"], p["coov"], p["bias"], stride, False)
    Wo, Ho = (W - 2) // stride + 1, (H - 2) // stride + 1
    assert y.shape == (B, N, Wo, Ho) and rn.shape == (B, 1, Wo, Ho)
    g = torch.Generator().manual_seed(6)
    dy, drn = torch.randn(y.shape, generator=g, dtype=torch.float64), torch.randn(rn.shape, generator=g, dtype=torch.float64)
    keys = ("x", "r", "w1", "b1", "w2", "b2", "coov", "bias")
    want = dict(zip(keys, torch.autograd.grad((y * dy).sum() + (rn * drn).sum(), [p[k] for k in keys])))
    n = lambda t: t.detach().numpy()                              # noqa: E731
    tab = torch.stack([t.detach() for t in p["tabs"]]).reshape(4, 16).numpy()
    o = MK.layer_host(n(p["x"].permute(0, 2, 3, 1)), n(p["r"][:, 0]), tab, n(p["w1"]), n(p["b1"]), n(p["w2"]), n(p["b2"]), n(p["coov"]),
                      n(p["bias"]), stride, dy=n(dy.permute(0, 2, 3, 1)), dr_next=n(drn[:, 0]))
    tol = 1e-12
    assert U.rel(o["y"], y.detach().permute(0, 2, 3, 1)) < tol and np.array_equal(o["r_next"], n(rn[:, 0]))
    for got, k in (("dx", "x"), ("dr", "r"), ("dw1", "w1"), ("db1", "b1"), ("dw2", "w2"), ("db2", "b2"), ("dcoov", "coov"), ("dbias", "bias")):
        ref = want[k].permute(0, 2, 3, 1) if k == "x" else want[k][:, 0] if k == "r" else want[k].reshape(o[got].shape)
        assert U.rel(o[got], ref) < tol, (got, U.rel(o[got], ref))
    # the three statements on their own: pe (with its gradient to r), the MLP, the modulated conv
    r0 = p["r"].detach()[:, 0].clone().requires_grad_()
    rp = MK._patches(r0[:, None], stride, MK.R_OUTSIDE)[..., 0]
    ca, sa, ci, si = [t.detach() for t in p["tabs"]]
    pe = torch.stack([(rp * ca) * ci - rp[:, :, :, 2, 2, None, None], (rp * ca) * si, rp * sa], -1).reshape(-1, 3)
    dpe = torch.randn(pe.shape, generator=g, dtype=torch.float64)
    ph = MK.pe_host(n(r0), tab, stride, dpe=n(dpe))
    assert U.rel(ph["pe"], pe.detach()) < tol and U.rel(ph["dr"], torch.autograd.grad((pe * dpe).sum(), r0)[0]) < tol
    assert int((ph["src"] < 0).sum()) == (o["src"] < 0).sum() > 0
    pe_l = pe.detach().requires_grad_()
    w1, b1, w2, b2 = (p[k].detach().requires_grad_() for k in ("w1", "b1", "w2", "b2"))
    m = torch.nn.functional.linear(torch.nn.functional.leaky_relu(torch.nn.functional.linear(pe_l, w1, b1), 0.2), w2, b2)
    dm = torch.randn(m.shape, generator=g, dtype=torch.float64)
    mh = MK.mlp_host(n(pe_l), n(w1), n(b1), n(w2), n(b2), dm=n(dm))
    assert U.rel(mh["m"], m.detach()) < tol
    for got, ref in zip(("dpe", "dw1", "db1", "dw2", "db2"), torch.autograd.grad((m * dm).sum(), [pe_l, w1, b1, w2, b2])):
        assert U.rel(mh[got], ref) < tol, got
    xs, ms, cw, cb = p["x"].detach().requires_grad_(), m.detach().requires_grad_(), p["coov"].detach().requires_grad_(), p["bias"].detach().requires_grad_()
    P = (ms.reshape(B, Wo, Ho, 4, 4, Cc) * MK._patches(xs, stride, 0.0)).reshape(-1, 16 * Cc)
    yy = P @ cw.reshape(N, Cc, 16).permute(0, 2, 1).reshape(N, -1).t() + cb
    dyy = torch.randn(yy.shape, generator=g, dtype=torch.float64)
    ch = MK.modconv_host(n(xs.permute(0, 2, 3, 1)), ph["src"], n(ms), n(cw).reshape(N, -1), n(cb), dy=n(dyy))
    assert U.rel(ch["y"], yy.detach()) < tol
    gx, gm, gw, gb = torch.autograd.grad((yy * dyy).sum(), [xs, ms, cw, cb])
    assert U.rel(ch["dx"], gx.permute(0, 2, 3, 1)) < tol and U.rel(ch["dm"], gm) < tol
    assert U.rel(ch["dcoov"], gw.reshape(N, -1)) < tol and U.rel(ch["dbias"], gb) < tol


def test_bf16_emulation_rounds_only_the_gemm_operands():
    """On operands exact in bf16 the emulated linear and its two gradients ARE the fp32 ones; on generic operands they are those of
    the rounded operands.  In the network the C = 2 layer's MLP stays fp32."""
    g = torch.Generator().manual_seed(9)
    for exact in (True, False):
        if exact:
            a, w, dy = (torch.randint(-3, 4, s, generator=g).float() for s in ((12, 16), (8, 16), (12, 8)))
        else:
            a, w, dy = (torch.randn(s, generator=g) for s in ((12, 16), (8, 16), (12, 8)))
        r = lambda t: t.to(torch.bfloat16).float()                  # noqa: E731
        a1, w1 = a.clone().requires_grad_(), w.clone().requires_grad_()
        y = MK._Bf16Linear.apply(a1, w1)
        y.backward(dy)
        assert torch.equal(y.detach(), r(a) @ r(w).t())
        assert torch.equal(a1.grad, r(dy) @ r(w)) and torch.equal(w1.grad, r(dy).t() @ r(a))
        if exact:
            assert torch.equal(y.detach(), a @ w.t()) and torch.equal(a1.grad, dy @ w) and torch.equal(w1.grad, dy.t() @ a)
    # a one-layer-deep look at the network: with a coov weight and inputs that bf16 holds exactly and in_channels = 2, bf16=True changes
    # nothing in the first layer's MLP, so the first layer's output moves only by the rounding of m x
    hc, he = U.host_case(16, 32, 24), U.host_case(16, 32, 24, bf16=True)
    assert 1e-4 < U.rel(he["logits_fake"], hc["logits_fake"]) < 5e-2
