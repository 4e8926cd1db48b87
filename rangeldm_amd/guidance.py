"""Decoder guidance: completion of ANY pixel mask -- every 4th beam included -- with the released, unconditional RangeLDM.

Known-region replacement works on latents, so it needs latent pixels whose whole footprint is known (pipelines.latent_known_mask).
Here the known pixels guide the clean estimate instead (the DPS / MPGD family's guidance on x0, no UNet backward).  DDIM, eta = 0;
a_t = sqrt(abar_t), s_t = sqrt(1 - abar_t), (a_p, s_p) the same of the previous timestep ((1, 0) behind the last one), sf the VAE's
scaling_factor, y the known image (B, 2, W, H), m the pixel mask (B, 1, W, H), wc the channel weights.  Step i at latent z_t:

  1. eps = unet(z_t, t); z0 = the scheduler's own x0 conversion; z_plain = the scheduler's own step -- both by the code of the unguided
     loop (z0 is rldm_sched_step with the row (a_t, s_t, 1, 0, 0): 1 * x0 + 0 * eps).
  2. delta = 0; `guidance_iters` times:  xhat = D(z0 * (1 / sf)) on the training tape;  L_b = sum m wc[c] (xhat - y)^2 per image (fp64);
     g_x = m (2 wc[c]) (xhat - y);  g = D^T g_x by the tape's input-gradient-only replay;  rho_b = guidance_scale / max(sqrt(L_b), 1e-8)
     (fp64 from the device's L_b, no host sync, rounded to fp32);  u = rho_b (g (1 / sf));  z0 -= u;  delta += u.
     The update is guidance_scale * grad sqrt(L_b): DPS's normalisation.
  3. z_{t-1} = z_plain - c_i delta,  c_i = a_p - s_p a_t / s_t (host, fp64, rounded to fp32): the DDIM step taken with the corrected z0 and
     the eps consistent with it, written as a correction of the plain step -- so guidance_scale = 0 gives the bits of the unguided loop.

Steps outside [guidance_start, guidance_stop) (fractions of the schedule) are plain steps.  The final decode runs on the inference
kernels and the known pixels are pasted over it: they come back bit for bit.

`DecoderGuide` owns the decoder on the tape; `residual_host` / `latent_host` / `update_host` / `correct_host` restate csrc/guide.hip in
numpy, one rounding per line; `decoder_guided_sample_host` is the whole loop in torch on the oracle decoder with autograd (fp64, or
fp32 with the convs' operands rounded to bf16 as the tape's kernels round them) -- the reference has nothing like this step, so that
host statement is its contract.  No torch autograd and no torch compute op on the device path; no CPU fallback."""
import contextlib
from collections import OrderedDict

import numpy as np
import torch

from . import train_ops as T
from .params import vae_param_shapes
from .pipelines import _pos_channel
from .vae_training import _VAETape, decoder_param_names


def inverse_scale(scaling_factor):
    """1 / scaling_factor evaluated in fp64 and rounded to fp32, as a Python float: the factor of the decoder's input and of its gradient."""
    return float(np.float32(1.0 / float(scaling_factor)))


def _alpha_pair(scheduler, t):
    """(abar_t, abar_prev) as Python floats, abar_prev the one the scheduler's own step uses (1 behind the last timestep with
    set_alpha_to_one); for DDIMSchedulerHIP and the oracle's DDIM scheduler."""
    t = int(t)
    prev_t = scheduler._prev_t(t)
    if prev_t >= 0:
        a_prev = scheduler.alphas_cumprod[prev_t]
    else:
        a_prev = scheduler._alpha_final() if hasattr(scheduler, "_alpha_final") else scheduler.one
    return float(scheduler.alphas_cumprod[t]), float(a_prev)


def guidance_coefficient(scheduler, t, rounded=True):
    """c_i = a_p - s_p a_t / s_t of timestep t in fp64 (from the scheduler's fp32 alphas_cumprod); rounded: to fp32, what the device
    multiplies by.  1 on the last step."""
    at, ap = _alpha_pair(scheduler, t)
    c = np.sqrt(np.float64(ap)) - np.sqrt(np.float64(1.0 - ap)) * np.sqrt(np.float64(at)) / np.sqrt(np.float64(1.0 - at))
    return float(np.float32(c)) if rounded else float(c)


def guided_steps(num_steps, start=0.0, stop=1.0):
    """The step indices inside the window: i with start * N <= i < stop * N."""
    if not (0.0 <= start <= stop <= 1.0):
        raise ValueError(f"the guidance window must satisfy 0 <= start <= stop <= 1; got ({start}, {stop})")
    return [i for i in range(num_steps) if start * num_steps <= i < stop * num_steps]


# ---- host statements of csrc/guide.hip (numpy; every line is one rounding per element) ----------------------------------------------
def residual_host(xhat_nhwc, y_nchw, mask, channel_weights):
    """rldm_guide_residual -> (gx (B, W, H, C) fp32, L (B,) fp64).  d = fp32(xhat - y); known (mask > 0.5): gx = (2 wc[c]) d, one
    product (2 wc[c] is exact); unknown: +0.  L_b: element 256 i + t of image b (NHWC order) contributes (wc[c] d) d in fp64 (wc[c] d
    is exact there) or +0 as lane t of partial i (train_ops._block_sum); the image's partials are folded by train_ops._fold_double."""
    x = np.asarray(xhat_nhwc, np.float32)
    y = np.asarray(y_nchw, np.float32).transpose(0, 2, 3, 1)
    known = np.broadcast_to(np.asarray(mask, np.float32).transpose(0, 2, 3, 1) > 0.5, x.shape)
    wc = np.asarray(channel_weights, np.float32).reshape(-1)
    d = x - y
    w2 = np.float32(2.0) * wc
    gx = np.where(known, w2 * d, np.float32(0.0)).astype(np.float32)
    d64 = d.astype(np.float64)
    v = np.where(known, (wc.astype(np.float64) * d64) * d64, 0.0)
    B = x.shape[0]
    n = v[0].size
    nb = (n + 255) // 256
    L = np.empty(B, np.float64)
    for b in range(B):
        part = np.concatenate([v[b].reshape(-1), np.zeros(nb * 256 - n, np.float64)]).reshape(nb, 256)
        L[b] = T._fold_double(T._block_sum(part))
    return gx, L


def latent_host(z0_nchw, inv_sf):
    """rldm_guide_latent: the decoder's input (B, W, H, C) = z0 * inv_sf, one product."""
    return np.asarray(z0_nchw, np.float32).transpose(0, 2, 3, 1) * np.float32(inv_sf)


def update_host(g_nhwc, L, scale, inv_sf, z0_nchw, delta_nchw):
    """rldm_guide_update -> (z0', delta').  rho_b = fp32(scale / max(sqrt(L_b), 1e-8)) evaluated in fp64 (L None: 1); t = g * inv_sf;
    u = rho_b * t; z0' = z0 - u; delta' = delta + u."""
    g = np.asarray(g_nhwc, np.float32)
    B = g.shape[0]
    if L is None:
        rho = np.ones(B, np.float32)
    else:
        rho = (np.float64(scale) / np.maximum(np.sqrt(np.asarray(L, np.float64)), 1e-8)).astype(np.float32)
    t = g * np.float32(inv_sf)
    u = (rho.reshape(B, 1, 1, 1) * t).transpose(0, 3, 1, 2)
    return np.asarray(z0_nchw, np.float32) - u, np.asarray(delta_nchw, np.float32) + u


def correct_host(z_plain, delta, c):
    """rldm_guide_correct: p = c * delta; z_plain - p, and z_plain's own bits (a -0 included) where p is a zero of either sign."""
    z = np.asarray(z_plain, np.float32)
    p = np.float32(c) * np.asarray(delta, np.float32)
    return np.where(p == 0, z, z - p).astype(np.float32)


# ---- the decoder on the tape --------------------------------------------------------------------------------------------------------
class DecoderGuide(_VAETape):
    """The decoder of an AutoencoderKLHIP on the training tape, for its input gradient alone: no optimizer, no discriminator, no BEV
    term.  It holds the decoder's fp32 parameters with their bf16 operand copies and one flat gradient buffer of the same size (which
    the input-gradient-only replay never touches: it is there for a full replay of the tape); no AdamW moments.
    deterministic: every tape kernel runs in the library's deterministic mode, so the same inputs give the same bits (the kernels of
    csrc/guide.hip are order-fixed in either mode)."""

    def __init__(self, vae, channel_weights=(40.0, 10.0), deterministic=False):
        self.cfg = vae._cfg
        if len(channel_weights) != self.cfg.out_channels:
            raise ValueError(f"{len(channel_weights)} channel weights for {self.cfg.out_channels} output channels")
        if not vae._finalized:
            raise RuntimeError("DecoderGuide: the VAE has no weights yet (load_state_dict has not been called)")
        shapes = vae_param_shapes(self.cfg)
        names = decoder_param_names(self.cfg, shapes)
        # the host arrays the VAE was loaded from, kept: load_state_dict replaces them, which is how `stale` sees a reload
        self._vae, self._loaded = vae, {n: vae._state[n] for n in names}
        self._init_parameters(OrderedDict((n, shapes[n]) for n in names), names, self._loaded, vae.device, deterministic=deterministic,
                              moments=False)
        self.scaling_factor = float(vae.config.scaling_factor)
        self.inv_sf = inverse_scale(self.scaling_factor)
        self.channel_weights = torch.tensor([float(w) for w in channel_weights], dtype=torch.float32, device=self.device)
        self._conv_out_in = self._out = self._zin = self._gz = None

    def stale(self, vae):
        """True when this guide no longer holds `vae`'s decoder: another VAE, or weights loaded since it was built."""
        return vae is not self._vae or any(vae._state.get(n) is not a for n, a in self._loaded.items())

    def _latent_shape(self, z):
        f = self.cfg.downscale
        if z.dim() != 4 or z.shape[1] != self.cfg.z_channels:
            raise ValueError(f"latent {tuple(z.shape)}: the decoder expects (B, {self.cfg.z_channels}, W / {f}, H / {f})")
        return (z.shape[0], self.cfg.out_channels, z.shape[2] * f, z.shape[3] * f)

    def prepare(self, y, mask, batch):
        """-> (y (B, C, W, H) fp32 contiguous on the device, m (B, 1, W, H) fp32 0 / 1 contiguous): what the kernels read."""
        y = y.to(self.device, torch.float32).contiguous()
        m = (mask.to(self.device, torch.float32) > 0.5).to(torch.float32)
        if m.dim() != 4 or m.shape[1] != 1 or y.dim() != 4 or y.shape[0] != batch or m.shape[2:] != y.shape[2:] or m.shape[0] not in (1, batch):
            raise ValueError(f"known {tuple(y.shape)} / known_mask {tuple(m.shape)}: expected (B, C, W, H) and (B, 1, W, H) with B = {batch}")
        return y, m.expand(batch, 1, *m.shape[2:]).contiguous()

    def forward(self, z0hat):
        """z0hat (B, z_channels, W / f, H / f), a latent as the sampler holds it (scaled by scaling_factor) -> the reconstruction
        D(z0hat * (1 / sf)) (B, W, H, C) NHWC; records the tape."""
        z0hat = z0hat.to(self.device, torch.float32).contiguous()
        self._latent_shape(z0hat)
        with self._mode():
            self._begin_tape()
            zin = T.guide_latent(z0hat, self.inv_sf)

            def grab():                                     # (replayed last: the gradient that reached the decoder's input)
                self._gz = self._pop(zin)
            self._tape.append(grab)
            self._zin = zin
            return self._decode(zin, dz=True)

    def input_gradient(self, gx_nhwc, params=False):
        """Replays the tape from d(loss) / d(xhat) = gx -> d(loss) / d(decoder input) (B, W / f, H / f, z_channels) NHWC.
        params=True: the trainers' full replay (the flat gradient buffer += the parameter gradients too)."""
        self._gz = None
        with self._mode():
            self._run_tape(self._out, gx_nhwc, params=params)
        return self._gz

    def loss_and_grad(self, z0hat, y, m):
        """-> (L (B,) fp64 device = sum m wc[c] (D(z0hat / sf) - y)^2 per image, g_z (B, z_channels, W / f, H / f) = d L_b / d z0hat).
        y, m as `prepare` returns them."""
        gx, L = T.guide_residual(self.forward(z0hat), y, m, self.channel_weights)
        g = self.input_gradient(gx)
        gz = torch.zeros(self._nchw(g), dtype=torch.float32, device=self.device)
        T.guide_update(g, None, 1.0, self.inv_sf, torch.zeros_like(gz), gz)      # (rho = 1: delta = 0 + g * (1 / sf))
        return L, gz

    @staticmethod
    def _nchw(g_nhwc):
        B, W, H, Cc = g_nhwc.shape
        return (B, Cc, W, H)

    def refine(self, z0hat, y, m, scale, iters):
        """`iters` guidance iterations from z0hat -> (z0hat', delta = z0hat - z0hat' as the sum of the updates, L (iters, B) fp64: the
        loss each iteration measured before its update).  z0hat is not modified.  No host sync."""
        z = z0hat.to(self.device, torch.float32).clone(memory_format=torch.contiguous_format)
        delta = torch.zeros_like(z)
        Ls = []
        for _ in range(int(iters)):
            gx, L = T.guide_residual(self.forward(z), y, m, self.channel_weights)
            T.guide_update(self.input_gradient(gx), L, float(scale), self.inv_sf, z, delta)
            Ls.append(L)
        L = torch.stack(Ls) if Ls else torch.empty((0, z.shape[0]), dtype=torch.float64, device=self.device)
        return z, delta, L


# ---- the sampling loop on the device ------------------------------------------------------------------------------------------------
def refuse_unsupported(scheduler, eta, jump_length, jump_n_sample, final_only):
    """What decoder guidance does not run (NotImplementedError), checked before anything is computed."""
    from .schedulers import DDIMSchedulerHIP
    if not isinstance(scheduler, DDIMSchedulerHIP):
        raise NotImplementedError(f"decoder guidance corrects the DDIM step (eta = 0): pass a DDIMSchedulerHIP, not {type(scheduler).__name__}")
    if eta != 0.0:
        raise NotImplementedError("decoder guidance is DDIM with eta = 0")
    if jump_length != 1 or jump_n_sample != 1:
        raise NotImplementedError("decoder guidance does not resample (jump_length / jump_n_sample are RePaint's, of the latent replacement)")
    if not final_only:
        raise NotImplementedError("decoder-guided sampling returns the final image only")


def decoder_guided_call(pipe, guide, latents, num_inference_steps, known, known_mask, scale, iters, start, stop, trace=None):
    """The guided loop of LDMPipelineRange (module docstring) from x_T = latents, on the pipeline's scheduler with its timesteps set.
    -> (image with the known pixels pasted over it, final latents, L (B,) of the last guided iteration or None).  trace: a list that
    receives every step's latents."""
    sch, dev = pipe.scheduler, pipe.device
    if known is None or known_mask is None:
        raise ValueError("decoder guidance needs `known` and `known_mask`")
    if int(iters) < 0:
        raise ValueError("guidance_iters must not be negative")
    z = latents.to(dev, torch.float32)
    B = z.shape[0]
    y, m = guide.prepare(known, known_mask, B)
    if tuple(y.shape) != guide._latent_shape(z):
        raise ValueError(f"known {tuple(y.shape)} is not the image of a latent {tuple(z.shape)}: expected {guide._latent_shape(z)}")
    inside = set(guided_steps(num_inference_steps, start, stop)) if int(iters) > 0 else set()
    if pipe.pos_encoding:
        pos_encoding = _pos_channel(B, z.shape[2], z.shape[3], dev)
    last = None
    for i, t in enumerate(pipe.progress_bar(sch.timesteps)):
        model_input = sch.scale_model_input(z, t)
        if pipe.pos_encoding:
            model_input = torch.cat([model_input, pos_encoding], dim=1)
        eps = pipe.unet(model_input, t).sample
        z_plain = sch.step(eps, t, z, eta=0.0).prev_sample
        if i in inside:
            c = sch.coefficients(t, 0.0)
            z0hat = sch._launch(0, [c[0], c[1], 1.0, 0.0, 0.0], eps, z, None)       # the step's own x0: 1 * x0 + 0 * eps
            _, delta, L = guide.refine(z0hat, y, m, scale, iters)
            last = L[-1]
            z = T.guide_correct(z_plain, delta, guidance_coefficient(sch, t))
        else:
            z = z_plain
        if trace is not None:
            trace.append(z)
    image = pipe.vae.decode(z / pipe.vae.config.scaling_factor).sample
    image = torch.where(m > 0.5, y, image)
    return image, z, last


# ---- the host statement of the whole loop -------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


@contextlib.contextmanager
def bf16_operand_convs():
    """Inside: every oracle.ops.circ_conv2d rounds x, w (forward), dy, w (data gradient) and dy, x (weight gradient) to bf16 and
    accumulates in the tensors' own precision -- the operand rounding of the tape's conv kernels, everything else left as it is."""
    from oracle import ops as o_ops
    plain = o_ops.circ_conv2d

    class Conv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b, stride, padding):
            ctx.save_for_backward(x, w)
            ctx.geometry = (stride, padding)
            return plain(_bf16(x), _bf16(w), b, stride, padding)

        @staticmethod
        def backward(ctx, dy):
            x, w = ctx.saved_tensors
            stride, padding = ctx.geometry
            with torch.enable_grad():
                xr, wr = _bf16(x).detach().requires_grad_(), _bf16(w).detach().requires_grad_()
                dx, dw = torch.autograd.grad(plain(xr, wr, None, stride, padding), [xr, wr], _bf16(dy))
            return dx, dw, dy.sum((0, 2, 3)), None, None

    o_ops.circ_conv2d = lambda x, w, b, stride=1, padding=1: Conv.apply(x, w, b, stride, padding)
    try:
        yield
    finally:
        o_ops.circ_conv2d = plain


def _host_setup(state_dict, dtype):
    return {k: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(dtype) for k, v in state_dict.items()
            if k.startswith("decoder.")}


def loss_and_grad_host(state_dict, cfg, z0hat, y, m, channel_weights=(40.0, 10.0), scaling_factor=None, dtype=torch.float64,
                       bf16_operands=False):
    """DecoderGuide.loss_and_grad on the host: torch autograd through oracle.vae.vae_decode in `dtype` (bf16_operands: the convs' operands
    rounded as the tape rounds them) -> (L (B,), g_z = d L_b / d z0hat)."""
    from oracle import vae as o_vae
    sf = float(cfg.scaling_factor if scaling_factor is None else scaling_factor)
    sd = _host_setup(state_dict, dtype)
    wc = torch.tensor([float(w) for w in channel_weights], dtype=dtype).view(1, -1, 1, 1)
    mk = (m.to(dtype) > 0.5).to(dtype)
    with (bf16_operand_convs() if bf16_operands else contextlib.nullcontext()), torch.enable_grad():
        zz = z0hat.detach().to(dtype).clone().requires_grad_()
        xhat = o_vae.vae_decode.__wrapped__(sd, cfg, zz / sf)
        L = (mk * wc * (xhat - y.to(dtype)) ** 2).sum((1, 2, 3))
        g, = torch.autograd.grad(L.sum(), zz)
    return L.detach(), g.detach()


def refine_host(state_dict, cfg, z0hat, y, m, scale, iters, **kw):
    """DecoderGuide.refine on the host (loss_and_grad_host's arguments) -> (z0hat', delta, L (iters, B))."""
    z = z0hat.detach().to(kw.get("dtype", torch.float64)).clone()
    delta = torch.zeros_like(z)
    Ls = []
    for _ in range(int(iters)):
        L, g = loss_and_grad_host(state_dict, cfg, z, y, m, **kw)
        rho = float(scale) / torch.clamp(L.double().sqrt(), min=1e-8)
        u = rho.to(z.dtype).view(-1, 1, 1, 1) * g
        z, delta = z - u, delta + u
        Ls.append(L)
    return z, delta, (torch.stack(Ls) if Ls else torch.empty((0, z.shape[0]), dtype=z.dtype))


def decoder_guided_sample_host(unet, scheduler, state_dict, cfg, x_T, known, known_mask, num_inference_steps, guidance_scale=1.0,
                               guidance_iters=1, guidance_start=0.0, guidance_stop=1.0, channel_weights=(40.0, 10.0),
                               scaling_factor=None, dtype=torch.float64, bf16_operands=False, pos_encoding=False, trace=None):
    """The whole guided loop on the host.  unet: a callable (model_input, t) -> eps (the oracle's UNet, or any other -- its output is cast
    to `dtype`); scheduler: the oracle's DDIM scheduler (oracle.schedulers.OracleDDIMScheduler), whose own x0 conversion and step are
    used; the decoder is oracle.vae.vae_decode under torch autograd.  dtype / bf16_operands: fp64, or fp32 with the convs' operands
    rounded to bf16 (and c_i rounded to fp32, as the device takes it).  -> (final latents, L (B,) of the last guided iteration or None).
    guidance_scale = 0 is the scheduler's plain loop exactly."""
    kw = dict(channel_weights=channel_weights, scaling_factor=scaling_factor, dtype=dtype, bf16_operands=bf16_operands)
    scheduler.set_timesteps(num_inference_steps)
    inside = set(guided_steps(num_inference_steps, guidance_start, guidance_stop)) if int(guidance_iters) > 0 else set()
    z = x_T.detach().to(dtype) * scheduler.init_noise_sigma
    y, m = known.detach().to(dtype), known_mask.detach().to(dtype)
    if pos_encoding:
        pe = _pos_channel(z.shape[0], z.shape[2], z.shape[3], "cpu", dtype)
    last = None
    for i, t in enumerate(scheduler.timesteps):
        inp = scheduler.scale_model_input(z, t)
        eps = unet(torch.cat([inp, pe], 1) if pos_encoding else inp, t).to(dtype)
        out = scheduler.step(eps, t, z, eta=0.0)
        z_plain = out.prev_sample
        if i in inside:
            _, delta, L = refine_host(state_dict, cfg, out.pred_original_sample, y, m, guidance_scale, guidance_iters, **kw)
            last = L[-1]
            p = guidance_coefficient(scheduler, t, rounded=dtype != torch.float64) * delta
            z = torch.where(p == 0, z_plain, z_plain - p)
        else:
            z = z_plain
        if trace is not None:
            trace.append(z)
    return z, last
