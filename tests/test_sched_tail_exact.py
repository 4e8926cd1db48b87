"""GPU: the scheduler step exactly where a captured sampler runs it -- in the epilogue of the UNet's output layer (conv_o4_kernel at 128
channels, the generic kernel's fp32-NCHW epilogue elsewhere), through rldm_test_conv_sched, which fills the plan's scheduler block the
way sampler_build_plans does.  Beside the arithmetic (kernels.h sched_prev, inlined into each epilogue) the epilogues pick row *step of
the device coefficient table, offset the noise by step * stride, rewrite the x0 history in multistep mode and store bf16(x_prev) into
the next step's conv_in input; every one of those is pinned here.

Group A, exact operands: GroupNorm with gamma = 0 makes the conv's input silu(beta) per channel (tests/test_conv_exact.py), thinned
weights keep |eps| <= 64 on the 2^-8 grid, and on the grids of tests/test_sched_tail_host.py every intermediate of every mode is exact in
fp32 -- fused or not, there is one right answer, sched_tail_reference.  The table and the noise carry NaN in every row but the one
`step` selects, and the noise pointer is offset as a second lane's is, so a wrong row, a dropped stride or a dropped lane offset reads
NaN; every buffer is large enough for those wrong reads to stay inside it.
Group B, real operands: the fused tail against the stand-alone launch (rldm_sched_step / rldm_sched_dpmsolver_step) on the eps the
fused kernel wrote -- the same int32 bits.  sched_prev leaves fma contraction to the compiler at each inlining site; this is the test
that notices if two sites ever contract differently.
The route of every case is asserted from the name of the launch that carried the step, as the library reports it."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd._lib import Flag
from rangeldm_amd.config import SchedulerConfig, UNetConfig
from rangeldm_amd.synth import normal
from tests.hip_util import RefCache, amax, assert_bitexact, assert_exact_bound, hip_conv_sched, int_grid
from tests.test_conv_exact import H_GRID, HU, U, _b, _gn0_ref, _gn_beta
from tests.test_sched_tail_host import (E_MAX, E_UNIT, EXACT_ROW, EXACT_ROW_C4_ZERO, MODE_NAMES, MODES, PTYPES, X_MAX, X_UNIT, Z_MAX,
                                        Z_UNIT, assert_grid, assert_trace_exact, grid_draw, sched_tail_reference)

pytestmark = pytest.mark.gpu
_refs = RefCache(cap=32)
DPM = _lib.RLDM_SAMPLER_DPMSOLVER
GENERIC = int(Flag.NO_CONV_SMALL | Flag.NO_STREAM_REGW)
O4_SHAPES = [(2, 128, 256, 16, 4), (16, 128, 64, 8, 2), (3, 128, 256, 16, 3), (2, 128, 1024, 8, 1)]
# (route the launch must report, routing flags, (B, Cin, W, H, N))
CASES = ([("conv_o4_kernel", 0, s) for s in O4_SHAPES] + [("conv_igemm_kernel", GENERIC, s) for s in O4_SHAPES] +
         [("conv_igemm_kernel", 0, (1, 128, 32, 16, 4)),          # fewer than 64 workgroups: conv_o4 declines
          ("conv_igemm_kernel", 0, (2, 32, 32, 8, 4)),            # the output layer of the reduced test networks
          ("conv_igemm_kernel", 0, (2, 64, 64, 32, 2))])
CASE_IDS = [f"{r.split('_')[1]}{'-forced' if f else ''}-" + "x".join(map(str, s)) for r, f, s in CASES]
SENTINEL = -21846                   # 0xAAAA: a bf16 bit pattern no x_prev of these tests rounds to (-3.03e-13)
NAN = float("nan")


def _i32(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _table(row):
    """[3][5] on the device: `row` at index 1 between two rows of NaN; and step = 1"""
    t = torch.full((3, 5), NAN, dtype=torch.float32)
    t[1] = torch.tensor([float(v) for v in row], dtype=torch.float32)
    return t.cuda(), torch.ones(1, dtype=torch.int32).cuda()


def _lane_noise(z, B):
    """z (B, N, W, H) as row 1 of a [3][(B + 1) images] step-noise tensor of which this lane owns images 1 .. B: NaN everywhere else.
    -> (whole buffer, the lane's view of it = what rldm_sample hands its second lane, the step stride)."""
    n = z.numel()
    per = n // B
    stride = per * (B + 1)
    buf = torch.full((3 * stride,), NAN, dtype=torch.float32)
    buf[stride + per:stride + per + n] = z.reshape(-1)
    buf = buf.cuda()
    return buf, buf[per:], stride


def _pack_expect(x_prev, pack_ld, slack):
    """the int16 image of the pack tensor [B][W][H][pack_ld] (+ `slack` elements): bf16 RNE of x_prev in channels < N, sentinel elsewhere"""
    B, N, W, H = x_prev.shape
    want = torch.full((B, W, H, pack_ld), SENTINEL, dtype=torch.int16)
    want[..., :N] = x_prev.float().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).view(torch.int16)
    return torch.cat([want.reshape(-1), torch.full((slack,), SENTINEL, dtype=torch.int16)])


def _with_flags(flags, fn):
    _lib.lib().rldm_debug_set_flags(flags)
    try:
        return fn()
    finally:
        _lib.lib().rldm_debug_set_flags(0)


# ---- group A ------------------------------------------------------------------------------------------------------------------------
def _exact_conv(shape):
    """operands of the gamma = 0 output layer with |eps| <= E_MAX on the E_UNIT grid, and that eps (fp64 reference, exact in fp32)"""
    B, Cin, W, H, N = shape
    beta, h = _gn_beta(Cin, 401, True)
    b = _b((N,), 402)
    hmax = max(abs(v) for v in H_GRID)
    for density in (1.0, 0.5, 0.35, 0.25, 0.15, 0.1, 0.05):          # thin the weights until the bound holds
        w = int_grid((N, Cin, 3, 3), 403, -4, 4, exp=-5, density=density)
        bound = float(w.abs().sum(dim=(1, 2, 3)).max()) * hmax + amax(b)
        if bound <= E_MAX:
            break
    assert bound <= E_MAX and float(w.abs().sum()) > 0, "no density keeps |eps| <= 64"
    assert_exact_bound(HU * U, (Cin * 9, hmax * amax(w)), (1, amax(b)))
    assert HU * U == E_UNIT
    x0 = int_grid((B, Cin, W, H), 404, -3, 3) * 0.5 + 0.25
    e = _gn0_ref(h, B, W, H, w, b)
    assert_grid(e.numpy(), E_UNIT, E_MAX, "eps")
    return x0, w, b, beta, e.float()


def _exact_case(shape):
    B, Cin, W, H, N = shape
    x0, w, b, beta, e = _exact_conv(shape)
    n = B * N * W * H
    x = grid_draw(n, X_UNIT, X_MAX, 411).reshape(B, N, W, H)
    z = grid_draw(n, Z_UNIT, Z_MAX, 412).reshape(B, N, W, H)
    return x0, w, b, beta, e, x, z


@pytest.mark.parametrize("ptype", range(3), ids=PTYPES)
@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
@pytest.mark.parametrize("route,flags,shape", CASES, ids=CASE_IDS)
def test_fused_tail_exact(route, flags, shape, mode, ptype):
    """eps, x_prev, the x0 history and the pack tensor of one fused launch against the fp64 formulas, element for element: beside x,
    aliasing x, with c4 == 0 over NaN noise, and without a pack tensor"""
    B, Cin, W, H, N = shape
    x0, w, b, beta, e, x, z = _refs.get(("A", shape), lambda: _exact_case(shape))
    what = f"{route} {shape} {MODE_NAMES[mode]} {PTYPES[ptype]}"
    trace = []
    prev, x0_ref = sched_tail_reference(mode, ptype, EXACT_ROW, e.numpy(), x.numpy(), z.numpy(), trace)
    assert_trace_exact(trace + [prev, x0_ref], what)
    prev, x0_ref = torch.from_numpy(prev).float(), torch.from_numpy(np.broadcast_to(x0_ref, prev.shape).copy()).float()
    gamma = torch.zeros(Cin)

    def run(row, x_dev, x_prev_dev, noise_view, stride, pack, pack_ld):
        tab, step = _table(row)
        eps, name = _with_flags(flags, lambda: hip_conv_sched(x0, w, b, gamma, beta, mode, ptype, tab, step, x_dev, noise_view, stride,
                                                              x_prev_dev, pack=pack, pack_ld=pack_ld))
        assert name.startswith(route + "<"), f"{what}: the step rode on {name}, not on {route}"
        assert_bitexact(eps, e, what=f"eps, {what}")
        assert torch.equal(_i32(tab)[1], _i32(torch.tensor([float(v) for v in row]))) and int(step.cpu()) == 1
        return eps

    def operands(zz):
        """-> (whole noise buffer or history, what the kernel gets, stride)"""
        if mode == DPM:
            hist = zz.clone().cuda()
            return hist, hist, 0
        return _lane_noise(zz, B)

    slack = 16
    # 1: x_prev beside x, pack_ld = N
    xd, out = x.cuda(), torch.full_like(x, NAN).cuda()
    buf, view, stride = operands(z)
    before = buf.clone()
    pack = torch.full((B * W * H * N + slack,), SENTINEL, dtype=torch.int16).cuda()
    run(EXACT_ROW, xd, out, view, stride, pack, N)
    assert_bitexact(out, prev, what=f"x_prev, {what}")
    assert torch.equal(_i32(xd), _i32(x)), f"{what}: x was written"
    if mode == DPM:
        assert_bitexact(buf, x0_ref, what=f"x0 history, {what}")
    else:
        assert torch.equal(_i32(buf), _i32(before)), f"{what}: the noise tensor was written"
    assert torch.equal(pack.cpu(), _pack_expect(prev, N, slack)), f"{what}: pack store, pack_ld {N}"
    # 2: x_prev aliasing x, as the sampler runs it; pack_ld = 8
    xd = x.cuda()
    buf, view, stride = operands(z)
    pack = torch.full((B * W * H * 8 + slack,), SENTINEL, dtype=torch.int16).cuda()
    run(EXACT_ROW, xd, xd, view, stride, pack, 8)
    assert_bitexact(xd, prev, what=f"x_prev aliasing x, {what}")
    assert torch.equal(pack.cpu(), _pack_expect(prev, 8, slack)), f"{what}: pack store, pack_ld 8"
    if mode == DPM:
        assert_bitexact(buf, x0_ref, what=f"x0 history (aliased run), {what}")
    # 3: c4 == 0 -- the noise / history is not an operand: all NaN, result finite; the history is overwritten all the same; pack_ld = 16
    prev0, _ = sched_tail_reference(mode, ptype, EXACT_ROW_C4_ZERO, e.numpy(), x.numpy(), None)
    prev0 = torch.from_numpy(prev0).float()
    xd, out = x.cuda(), torch.full_like(x, NAN).cuda()
    buf, view, stride = operands(torch.full_like(z, NAN))
    pack = torch.full((B * W * H * 16 + slack,), SENTINEL, dtype=torch.int16).cuda()
    run(EXACT_ROW_C4_ZERO, xd, out, view, stride, pack, 16)
    assert torch.isfinite(out).all(), f"{what}: c4 == 0 read the noise / history"
    assert_bitexact(out, prev0, what=f"x_prev with c4 == 0, {what}")
    assert torch.equal(pack.cpu(), _pack_expect(prev0, 16, slack)), f"{what}: pack store, pack_ld 16"
    if mode == DPM:
        assert_bitexact(buf, x0_ref, what=f"x0 history with c4 == 0, {what}")
    # 4: no pack tensor: the same eps, x_prev and history
    xd, out = x.cuda(), torch.full_like(x, NAN).cuda()
    buf, view, stride = operands(z)
    run(EXACT_ROW, xd, out, view, stride, None, 0)
    assert_bitexact(out, prev, what=f"x_prev without a pack tensor, {what}")
    if mode == DPM:
        assert_bitexact(buf, x0_ref, what=f"x0 history without a pack tensor, {what}")


# ---- the stand-alone entry points on the same operands ----------------------------------------------------------------------------------
def _standalone(mode, ptype, row, e, x, noise, out):
    """rldm_sched_step / rldm_sched_dpmsolver_step on device tensors, in place (noise: the history in multistep mode)"""
    cf = (C.c_float * 5)(*[float(v) for v in row])

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    dev = torch.device("cuda")
    if mode == DPM:
        _lib.check(_lib.lib().rldm_sched_dpmsolver_step(ptype, cf, p(e), p(x), p(noise), p(out), x.numel(), _lib.stream_ptr(dev)),
                   "rldm_sched_dpmsolver_step")
    else:
        _lib.check(_lib.lib().rldm_sched_step(mode, ptype, cf, p(e), p(x), p(noise), p(out), x.numel(), _lib.stream_ptr(dev)),
                   "rldm_sched_step")
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 257, 2048 * 256 + 77], ids=["n1", "n257", "past-the-grid-cap"])
@pytest.mark.parametrize("ptype", range(3), ids=PTYPES)
@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_standalone_step_exact(mode, ptype, n):
    """sched_step_kernel alone, exact operands; 2048 * 256 + 77 elements is past the launch's grid cap, so its stride loop runs"""
    e, x, z = _refs.get(("S", n), lambda: (grid_draw(n, E_UNIT, E_MAX, 421), grid_draw(n, X_UNIT, X_MAX, 422),
                                           grid_draw(n, Z_UNIT, Z_MAX, 423)))
    what = f"stand-alone {MODE_NAMES[mode]} {PTYPES[ptype]} n={n}"
    for row, zz in ((EXACT_ROW, z), (EXACT_ROW_C4_ZERO, torch.full_like(z, NAN))):
        trace = []
        prev, x0_ref = sched_tail_reference(mode, ptype, row, e.numpy(), x.numpy(), zz.numpy(), trace)
        assert_trace_exact(trace + [prev, x0_ref], what)
        ed, xd, zd = e.cuda(), x.cuda(), zz.cuda()
        out = torch.full_like(xd, NAN)
        _standalone(mode, ptype, row, ed, xd, zd, out)
        assert_bitexact(out, torch.from_numpy(prev).float(), names=("element",), what=f"x_prev, {what}, c4 {row[4]}")
        assert torch.equal(_i32(ed), _i32(e)) and torch.equal(_i32(xd), _i32(x))
        if mode == DPM:
            assert_bitexact(zd, torch.from_numpy(np.broadcast_to(x0_ref, prev.shape).copy()).float(), names=("element",),
                            what=f"x0 history, {what}, c4 {row[4]}")
        else:
            assert torch.equal(_i32(zd), _i32(zz))
        xa = x.cuda()                                                  # ... and in place
        _standalone(mode, ptype, row, ed, xa, zz.cuda(), xa)
        assert_bitexact(xa, torch.from_numpy(prev).float(), names=("element",), what=f"x_prev aliasing x, {what}, c4 {row[4]}")


# ---- group B ------------------------------------------------------------------------------------------------------------------------
def _real_case(shape):
    B, Cin, W, H, N = shape
    key = "x".join(map(str, shape))

    def t(name, s):
        return torch.from_numpy(normal(43, f"schedtail/{key}/{name}", s))

    x0 = t("x0", (B, Cin, W, H))
    w = t("w", (N, Cin, 3, 3)) / (9 * Cin) ** 0.5 * 2
    b, gamma, beta = t("b", (N,)) * 0.1, 1 + 0.1 * t("gamma", (Cin,)), 0.1 * t("beta", (Cin,))
    return x0, w, b, gamma, beta, t("x", (B, N, W, H)), t("z", (B, N, W, H)), t("hist", (B, N, W, H))


def _real_rows(mode, ptype):
    """(label, row) pairs of the scheduler's own coefficient rows: a middle row and the last one (DDIM: the middle row with and
    without its noise term)"""
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP
    cfg = SchedulerConfig(prediction_type=PTYPES[ptype])
    if mode == DPM:
        s = DPMSolverMultistepSchedulerHIP(cfg)
        s.set_timesteps(20)
        rows = s.coefficients()
        assert rows[10][4] != 0 and rows[19][4] == 0
        return [("row 10 of 20", rows[10]), ("last row", rows[19])]
    s = (DDIMSchedulerHIP if mode == _lib.RLDM_SAMPLER_DDIM else DDPMSchedulerHIP)(cfg)
    s.set_timesteps(50)
    mid, last = int(s.timesteps[25]), int(s.timesteps[-1])
    if mode == _lib.RLDM_SAMPLER_DDIM:
        return [("middle row, eta 0", s.coefficients(mid, 0.0)), ("middle row, eta 0.5", s.coefficients(mid, 0.5)),
                ("last row", s.coefficients(last, 0.0))]
    return [("middle row", s.coefficients(mid)), ("last row", s.coefficients(last))]


@pytest.mark.parametrize("ptype", range(3), ids=PTYPES)
@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
@pytest.mark.parametrize("route,flags,shape", CASES, ids=CASE_IDS)
def test_fused_tail_bits_equal_standalone_launch(route, flags, shape, mode, ptype):
    """normal operands, a real gamma, the schedulers' own rows: x_prev (and the x0 history) of the fused tail against sched_step_kernel
    on the eps the fused launch wrote.  Before sched_prev stated its roundings, conv_o4_kernel agreed in every mode and the generic
    kernel in every mode but DDIM x v_prediction, where 16-19 % of the elements differed in their bits (and with them a captured
    sampler on the reduced network from the same sampler under Flag.SCHED_LAUNCH)."""
    B, Cin, W, H, N = shape
    x0, w, b, gamma, beta, x, z, hist0 = _refs.get(("B", shape), lambda: _real_case(shape))
    for label, row in _real_rows(mode, ptype):
        what = f"{route} {shape} {MODE_NAMES[mode]} {PTYPES[ptype]} {label}"
        tab, step = _table(row)
        xd, out = x.cuda(), torch.full_like(x, NAN).cuda()
        if mode == DPM:
            buf = hist0.clone().cuda()
            view, stride = buf, 0
        else:
            buf, view, stride = _lane_noise(z, B)
        eps, name = _with_flags(flags, lambda: hip_conv_sched(x0, w, b, gamma, beta, mode, ptype, tab, step, xd, view, stride, out))
        assert name.startswith(route + "<"), f"{what}: the step rode on {name}, not on {route}"
        assert torch.isfinite(eps).all() and torch.isfinite(out).all(), what
        ref_out = torch.full_like(out, NAN)
        ref_noise = hist0.clone().cuda() if mode == DPM else z.cuda()
        _standalone(mode, ptype, row, eps, xd, ref_noise if (mode == DPM or float(np.float32(row[4])) != 0.0) else None, ref_out)
        differ = int((_i32(out) != _i32(ref_out)).sum())
        assert differ == 0, f"{what}: {differ} of {out.numel()} x_prev differ in bits between the fused tail and sched_step_kernel"
        if mode == DPM:
            differ = int((_i32(buf) != _i32(ref_noise)).sum())
            assert differ == 0, f"{what}: {differ} x0 history elements differ in bits"


# ---- sampler level ------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _unet(cfg, prefix):
    from tests.test_dpmsolver_gpu import hip_unet
    if prefix not in _NETS:
        _NETS[prefix] = hip_unet(cfg, prefix)[0]
    return _NETS[prefix]


def _scheduler(mode, ptype):
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP
    cls = {_lib.RLDM_SAMPLER_DDIM: DDIMSchedulerHIP, _lib.RLDM_SAMPLER_DDPM: DDPMSchedulerHIP, DPM: DPMSolverMultistepSchedulerHIP}[mode]
    return cls(SchedulerConfig(prediction_type=PTYPES[ptype]))


def _fused_vs_separate(unet, mode, ptype, lat_shape, steps, seed):
    """-> [(latents, images) of the captured sampler with the fused tail, ... of the same sampler created under Flag.SCHED_LAUNCH], the
    two handles, and what they point into (the pipeline that owns them, x_T, the step noise): alive as long as the caller holds it"""
    from rangeldm_amd.pipelines import LDMPipelineRange
    from tests.test_dpmsolver_gpu import hip_vae
    vae, _ = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=_scheduler(mode, ptype), pos_encoding=True)
    x_T = torch.from_numpy(normal(seed, "schedtail/xT", lat_shape)).cuda()
    zs = torch.from_numpy(normal(seed, "schedtail/zs", (steps, *lat_shape))).cuda() if mode == _lib.RLDM_SAMPLER_DDPM else None
    img_shape = (lat_shape[0], 2, lat_shape[2] * 4, lat_shape[3] * 4)
    res, handles = [], []
    for plan_flags in (0, int(Flag.SCHED_LAUNCH)):
        h = pipe._fused.get(unet, vae, pipe.scheduler, lat_shape[0], steps, mode, True, 0, plan_flags=plan_flags)
        img, lat = torch.empty(img_shape, device="cuda"), torch.empty(lat_shape, device="cuda")
        pipe._fused.run(h, x_T, zs, None, img, latents_out=lat)
        res.append((lat.cpu(), img.cpu()))
        handles.append(h)
    return res, handles, (pipe, x_T, zs)


def _assert_samplers_equal(res, what):
    (lat_f, img_f), (lat_s, img_s) = res
    assert torch.isfinite(lat_f).all() and torch.isfinite(img_f).all(), what
    n = int((_i32(lat_f) != _i32(lat_s)).sum())
    # (the tails themselves are bit-equal on one step's operands -- test_fused_tail_bits_equal_standalone_launch; what is left between
    #  the two samplers is the bf16 input the fused tail packs for the next conv_in, and the step counter that conv_in advances)
    assert n == 0, (f"{what}: {n} of {lat_f.numel()} final latents differ between the fused tail and Flag.SCHED_LAUNCH: with the kernel-level "
                    "tests passing, the fused pack store or the step counter")
    assert torch.equal(img_f, img_s), f"{what}: decoded images differ"


@pytest.mark.parametrize("ptype", range(3), ids=PTYPES)
@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_captured_sampler_equals_separate_launch_sampler(mode, ptype):
    cfg = UNetConfig(sample_size=(32, 8), in_channels=5, out_channels=4, block_out_channels=(32, 32, 64, 64))
    res, _, _ = _fused_vs_separate(_unet(cfg, "dpm/small."), mode, ptype, (2, 4, 32, 8), 4, 44)
    _assert_samplers_equal(res, f"reduced network, {MODE_NAMES[mode]} {PTYPES[ptype]}")


@pytest.mark.parametrize("mode,ptype", [(_lib.RLDM_SAMPLER_DDIM, 1), (_lib.RLDM_SAMPLER_DDPM, 2), (DPM, 0)],
                         ids=["ddim-v_prediction", "ddpm-sample", "dpmsolver-epsilon"])
def test_captured_sampler_equals_separate_launch_sampler_on_conv_o4(mode, ptype):
    """a 128-channel first level at 256 x 16: the output layer is conv_o4_kernel (asserted from the sampler's own profile)"""
    res, handles, alive = _fused_vs_separate(_unet(UNetConfig(), ""), mode, ptype, (2, 4, 256, 16), 3, 45)
    _assert_samplers_equal(res, f"headline network, {MODE_NAMES[mode]} {PTYPES[ptype]}")
    buf = C.create_string_buffer(1 << 16)
    _lib.check(_lib.lib().rldm_sampler_profile(handles[0], C.c_void_p(alive[1].data_ptr()), buf, len(buf)), "rldm_sampler_profile")
    kernels = json.loads(buf.value.decode())["unet_step"]
    assert any(k.startswith("conv_o4_kernel<") for k in kernels), sorted(kernels)
