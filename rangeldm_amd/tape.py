"""The model-independent half of the HIP training steps, in two classes.

`FlatParameters` is the parameter store: the flat fp32 buffers (parameters, gradients, AdamW moments, optional EMA copy; state-dict
views into them), the bf16 operand copies of the conv / linear weights it is told to pack, the deterministic switch, the clip + AdamW
call and the training state every owner of parameters saves and loads (`state_payload` / `load_payload`).  The discriminators
(discriminator.py, metakernel.py) sit on it directly: they walk their layers themselves and record no tape.

`TapeTrainer` adds the host-side tape (`forward` of a subclass records one backward closure per op, `_run_tape` replays them in
reverse) with its gradient slots, the queue of grouped weight gradients, the zero arena of the split-K convs and the conv / GroupNorm /
SiLU ops.  `UNetTrainer` (training.py), `VAEDecoderTrainer` and `VAETrainer` (vae_training.py) add their networks, losses and
schedules on top.  No torch autograd, no torch compute ops on the path; no CPU fallback."""
import contextlib
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from . import train_ops as T


class FlatParameters:
    _state_name = "training state"                      # (what load_payload calls a file it refuses)

    def _init_parameters(self, shapes, names, state_dict, device, fused=None, no_dx=(), use_ema=False, deterministic=False,
                         packed=None, tiled=True, moments=True):
        """shapes: name -> shape; names: the order of the parameters inside the flat buffers; fused: plan_parameter_order's layer
        groups (consecutive parameters run as ONE layer); no_dx: weights whose layer never computes a data gradient (no transposed
        operand copy).  packed: the weights that get bf16 operand copies (None: every `*.weight` of two or more dimensions outside a
        fused group, and every fused group); tiled: the packer `repack()` uses when it is not told (True: the 64 x 64 tile
        transpose).  moments=False: no AdamW moments are allocated (an owner that never takes an optimizer step: guidance.DecoderGuide);
        `_clip_adamw`, `state_payload` and `load_payload` are then not to be called."""
        _lib.require_gpu()
        self.device = torch.device(device)
        self.shapes, self.names, self.fused = shapes, list(names), fused if fused is not None else OrderedDict()
        sizes = [int(np.prod(self.shapes[n])) for n in self.names]
        self.offsets = dict(zip(self.names, np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()))
        self.sizes = dict(zip(self.names, sizes))
        self.numel = int(sum(sizes))
        z = lambda: torch.zeros(self.numel, dtype=torch.float32, device=self.device)      # noqa: E731
        self.params, self.grads = z(), z()
        self.exp_avg, self.exp_avg_sq = (z(), z()) if moments else (None, None)
        self.ema = z() if use_ema else None
        host = np.empty(self.numel, np.float32)
        for n in self.names:
            a = state_dict[n]
            a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
            if tuple(a.shape) != tuple(self.shapes[n]):
                raise RuntimeError(f"size mismatch for {n}: {tuple(a.shape)} vs {tuple(self.shapes[n])}")
            host[self.offsets[n]:self.offsets[n] + self.sizes[n]] = a.reshape(-1)
        self.params.copy_(torch.from_numpy(host))
        if self.ema is not None:
            self.ema.copy_(self.params)
        self.p = {n: self._view(self.params, n) for n in self.names}
        self.g = {n: self._view(self.grads, n) for n in self.names}
        # bf16 operand copies of the packed conv / linear weights: forward [N][taps][Cin], data gradient [Cin][taps][N].
        # layers: key -> (N, Cin, taps, offset of the fp32 weight in the flat buffer).  A fused group (all time_emb_proj
        # layers; to_q / to_k / to_v of an attention block) is ONE layer over its members' contiguous parameters.
        self.layers, self.wf, self.wt = OrderedDict(), {}, {}
        members = {m for grp in self.fused.values() for m in grp["weights"] + grp["biases"]}
        if packed is None:
            packed = [n for n in self.names if n.endswith(".weight") and len(self.shapes[n]) >= 2 and n not in members]
        packed = set(packed)
        for n in self.names:
            if n in packed:
                N, Cin = self.shapes[n][:2]
                taps = self.shapes[n][2] * self.shapes[n][3] if len(self.shapes[n]) == 4 else 1      # (k x k: 9, 1; 16 in the discriminator)
                self.layers[n] = (N, Cin, taps, self.offsets[n], n not in no_dx)
        for key, grp in self.fused.items():
            N = sum(self.shapes[m][0] for m in grp["weights"])
            Cin = self.shapes[grp["weights"][0]][1]
            ow, ob = self.offsets[grp["weights"][0]], self.offsets[grp["biases"][0]]
            self.layers[key + ".weight"] = (N, Cin, 1, ow, True)
            self.p[key + ".bias"] = self.params[ob:ob + N]
            self.g[key + ".bias"] = self.grads[ob:ob + N]
            self.g[key + ".weight"] = self.grads[ow:ow + N * Cin].view(N, Cin)
        for n, (N, Cin, taps, _, need_t) in self.layers.items():
            self.wf[n] = torch.empty((N, taps, (Cin + 15) // 16 * 16), dtype=torch.bfloat16, device=self.device)
            self.wt[n] = torch.empty((Cin, taps, (N + 15) // 16 * 16), dtype=torch.bfloat16, device=self.device) if need_t else None
        self._tiled, self._pack_table = bool(tiled), None
        self.repack()
        self.global_step = 0
        self.last_grad_norm = None
        self._deterministic = bool(deterministic)

    @property
    def deterministic(self):
        return self._deterministic

    @contextlib.contextmanager
    def _mode(self):
        """The library's deterministic switch set to this trainer's mode for the duration of a call, the previous value restored
        afterwards (also when the call raises)."""
        prev = T.deterministic_enabled()
        T.deterministic(self._deterministic)
        try:
            yield
        finally:
            T.deterministic(prev)

    # ---- parameters -------------------------------------------------------------------------------------------
    def _view(self, flat, n):
        return flat[self.offsets[n]:self.offsets[n] + self.sizes[n]].view(self.shapes[n])

    def repack(self, tiled=None):
        """Refresh the bf16 operand copies of the packed weights from the fp32 masters: one launch (tiled: a 64 x 64 tile
        transpose per workgroup; False: the element-wise kernel, kept as the cross-check; None: the store's default), none when
        no weight is packed."""
        import ctypes as C
        if not self.wf:
            return
        tiled = self._tiled if tiled is None else tiled
        if self._pack_table is None:
            tables = []
            for per_tile in (False, True):
                descs = (_lib.PackDescC * len(self.wf))()
                first = 0
                for i, (n, wf) in enumerate(self.wf.items()):
                    N, Cin, _, offset, _ = self.layers[n]
                    wt = self.wt[n]
                    d = descs[i]
                    d.first, d.param_offset = first, offset
                    d.w_forward = wf.data_ptr()
                    d.w_transposed = wt.data_ptr() if wt is not None else None
                    d.N, d.Cin, d.taps = N, Cin, wf.shape[1]
                    first += (((N + 63) // 64) * ((Cin + 63) // 64)) if per_tile else max(wf.numel(), wt.numel() if wt is not None else 0)
                tables.append((torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(self.device), first))
            self._pack_table = tables
        table, total = self._pack_table[1 if tiled else 0]
        fn = _lib.lib().rldm_train_pack_weights_tiled if tiled else _lib.lib().rldm_train_pack_weights_all
        _lib.check(fn(C.c_void_p(self.params.data_ptr()), C.c_void_p(table.data_ptr()), len(self.wf), total,
                      _lib.stream_ptr(self.device)), "rldm_train_pack_weights")

    def state_dict(self, ema=False):
        flat = (self.ema if ema else self.params).cpu()
        return OrderedDict((n, flat[self.offsets[n]:self.offsets[n] + self.sizes[n]].view(self.shapes[n]).clone())
                           for n in self.names)

    # ---- training state ---------------------------------------------------------------------------------------
    def state_payload(self):
        """What every owner of parameters saves: the fp32 masters, the Adam moments, the step counter and the parameter layout
        (host tensors).  A subclass adds its own entries to the dict."""
        return {"params": self.params.cpu(), "exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu(),
                "global_step": self.global_step, "names": list(self.names)}

    def load_payload(self, st):
        """Restores state_payload's entries IN PLACE (views, operand copies and captured graphs keep pointing at the buffers), zeroes
        the gradients and refreshes the bf16 operand copies."""
        if list(st["names"]) != list(self.names):
            raise RuntimeError(f"{self._state_name} was saved for a different parameter layout")
        self.params.copy_(st["params"])
        self.exp_avg.copy_(st["exp_avg"])
        self.exp_avg_sq.copy_(st["exp_avg_sq"])
        self.global_step = int(st["global_step"])
        self.grads.zero_()
        self.repack()

    def save_state(self, path):
        torch.save(self.state_payload(), path)

    def load_state(self, path):
        self.load_payload(torch.load(path, map_location="cpu", weights_only=True))     # tensors, lists, dicts, numbers: nothing to unpickle

    # ---- optimizer --------------------------------------------------------------------------------------------
    def _clip_adamw(self, lr, ema_decay=0.0):
        """clip_grad_norm_ (hp["max_grad_norm"]; None / <= 0: off) folded into torch.optim.AdamW on the flat buffers (+ the EMA copy's
        step), then the bf16 operand copies refreshed and the gradients zeroed.  `global_step` is the 1-based step being taken."""
        hp = self.hp
        sq = T.sqnorm(self.grads)
        T.adamw(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.global_step, lr, hp["betas"], hp["eps"],
                hp["weight_decay"], ema=self.ema, ema_decay=ema_decay, sqnorm_dev=sq, max_grad_norm=hp["max_grad_norm"] or 0.0)
        self.last_grad_norm = sq
        self.repack()
        self.grads.zero_()


class TapeTrainer(FlatParameters):
    def _init_parameters(self, shapes, names, state_dict, device, fused=None, no_dx=(), use_ema=False, deterministic=False,
                         arena_bytes=256 << 20, moments=True):
        """FlatParameters' arguments (every weight packed, the tiled packer) and arena_bytes: the size of the zero arena."""
        super()._init_parameters(shapes, names, state_dict, device, fused=fused, no_dx=no_dx, use_ema=use_ema,
                                 deterministic=deterministic, moments=moments)
        self._tape, self._grad, self._keep = [], {}, []
        self._rows, self._row_parent = {}, {}
        self._arena = T.ZeroArena(self.device, arena_bytes)
        # the weight gradients of the step are queued and run as a few grouped launches (rldm_train_wgrad_group: nothing in backward
        # waits for a weight gradient, and ~85 launches of them each sat at its launch floor); wgrad_group = False: launched where the
        # tape reaches them, the cross-check.  _wg_keep: the queued launches' operands (dy, inputs, statistics), alive until the flush
        self.wgrad_group = True
        self._wg_on, self._wg_keep = False, []
        self._cs = {}
        # _params_on: False only inside _run_tape(params=False), the replay for the input gradient alone; _dy_shared: a conv's dy is
        # (or, in that replay, counts as) an operand of a queued weight gradient, so a residual branch takes a buffer of its own
        self._params_on, self._dy_shared, self._sink_buf = True, False, None

    # ---- tape -------------------------------------------------------------------------------------------------
    def _acc(self, t, g, owned):
        """Add gradient g to tensor t's slot; `owned`: g is a fresh buffer nobody else reads."""
        if t is None:
            return
        k = id(t)
        if k not in self._grad:
            self._grad[k] = (g, owned)
        else:
            cur, cur_owned = self._grad[k]
            self._grad[k] = (T.add(cur, g, out=cur), True) if cur_owned else (T.add(cur, g), True)

    def _pop(self, t):
        g = self._grad.pop(id(t), None)
        self._popped_owned = bool(g is not None and g[1])
        return None if g is None else g[0]

    def _slot(self, t):
        """The gradient buffer tensor t already has, if this tape owns it: kernels that can accumulate write into it directly
        (no separate add launch)."""
        g = self._grad.get(id(t))
        return g[0] if g is not None and g[1] else None

    def _pin(self, *tensors):
        """Operands of a (possibly queued) weight-gradient launch: kept alive until the queue is flushed."""
        if self._wg_on:
            self._wg_keep.extend(t for t in tensors if t is not None)

    def _wg_flush(self):
        """Run the queued weight gradients (their dw / bias / time-embedding-row outputs are final behind this)."""
        if self._wg_on:
            T.wgrad_group_flush()
            self._wg_keep.clear()

    def _done(self, *names):
        """The gradients of these parameters are final (a trainer that exchanges gradients launches its collectives from here)."""

    def _cs_set(self, t, cs):
        """The (sum, sumsq) pairs of tensor t, keyed by id(t) WITH a reference to t: the id cannot be recycled while the entry lives."""
        self._cs[id(t)] = (t, cs)

    def _cs_get(self, t):
        e = self._cs.get(id(t))
        return e[1] if e is not None and e[0] is t else None

    def _end_queues(self, report=True):
        """Run the queued weight gradients and the deferred reduction, and switch both queues off: every gradient is final from here
        on.  The switches are reset whatever fails; report=False drops the flush's own error."""
        try:
            try:
                T.wgrad_group(False)                    # (runs what is still queued)
            finally:
                self._wg_on = False
                self._wg_keep.clear()
                T.defer_reduce(False)                   # (flushes)
        except Exception:
            if report:
                raise

    def _begin_tape(self):
        """A new forward pass: empty tape and gradient slots, the zero arena rewound."""
        self._tape, self._grad, self._cs = [], {}, {}
        T.set_zero_arena(self._arena)                   # split-K conv outputs of this step: pre-zeroed slices, one fill
        self._arena.begin()

    def _sink(self, n):
        """n floats nobody reads: where the input-gradient-only replay lets the GroupNorm backward put d gamma / d beta."""
        if self._sink_buf is None or self._sink_buf.numel() < n:
            self._sink_buf = torch.zeros(max(n, 4096), dtype=torch.float32, device=self.device)
        return self._sink_buf[:n]

    def _run_tape(self, out, dpred, params=True):
        """Replays the tape in reverse from d(loss) / d(out) = dpred; every gradient is final when it returns.
        params=False: the data gradients alone -- the same launches in the same order with the same operands as the default replay, so the
        gradient that reaches the tape's input has the same bits; no weight-gradient / bias launch, nothing queued or pinned, no
        weight-gradient group or deferred reduction opened, the flat gradient buffer untouched (the GroupNorm backward's d gamma /
        d beta go to `_sink`), `_done` not called."""
        self._acc(out, dpred, False)
        if not params:
            self._params_on, self._dy_shared = False, bool(self.wgrad_group)
            try:
                for fn in reversed(self._tape):
                    fn()
            finally:
                self._params_on, self._dy_shared = True, False
            self._tape, self._grad, self._cs = [], {}, {}
            T.set_zero_arena(None)
            return
        # the reduction of a weight gradient's partial tiles rides on the layer's data-gradient launch
        T.defer_reduce(True)
        self._wg_on = self._dy_shared = bool(self.wgrad_group)
        try:
            T.wgrad_group(self._wg_on)
            for fn in reversed(self._tape):
                fn()
        except BaseException:
            self._dy_shared = False
            self._end_queues(report=False)              # (the tape's error is the one to report)
            raise
        self._dy_shared = False
        self._end_queues()
        self._tape, self._grad, self._cs = [], {}, {}
        T.set_zero_arena(None)

    # ---- ops --------------------------------------------------------------------------------------------------
    def _conv(self, x, name, stride=1, mode=0, rowadd=None, res=None, need_dx=True, done=None, stats=False, pad=0):
        """pad = 1 (a stride-2 layer only): end-only padding in the forward, the weight gradient and the data gradient
        (train_ops.conv_desc)."""
        if pad and (stride != 2 or mode != 0 or stats):
            raise ValueError("end-only padding belongs to a plain stride-2 conv")
        w = name + ".weight"
        N, _, taps = self.layers[w][:3]
        done = done or (w, name + ".bias")
        if stats and rowadd is None and res is None and T.conv_fused_ok([T.Src(x)], N, taps, stride, mode, want_stats=True):
            y, cs_y = T.conv_fused([T.Src(x)], self.wf[w], N, taps, stride, mode, bias=self.p[name + ".bias"], want_stats=True)
            self._cs_set(y, cs_y)
        else:
            y = T.conv(x, self.wf[w], N, taps, stride, mode, bias=self.p[name + ".bias"], rowadd=rowadd, res=res, pad=pad)

        def bwd():
            dy = self._pop(y)
            dy_owned = self._popped_owned
            drow = None
            if rowadd is not None and not self._params_on:     # (drow is the weight-gradient launch's output)
                raise NotImplementedError("the input-gradient-only replay does not carry a conv's row term (time embedding)")
            if rowadd is not None:
                parent = self._row_parent.get(id(rowadd))
                if parent is None:
                    drow = T.empty(rowadd.shape, rowadd)
                else:                                   # a slice of the fused time_emb_proj output: write its slice of the gradient
                    rows, off = parent
                    if id(rows) not in self._grad:       # zeroed once for all 22 slices (they accumulate into it)
                        self._grad[id(rows)] = (torch.zeros(rows.shape, dtype=torch.float32, device=rows.device), True)
                    drow = self._grad[id(rows)][0][:, off:off + rowadd.shape[1]]
            if self._params_on:
                T.wgrad_bias(dy, x, self.g[w], taps, stride, mode, rows=drow, total=self.g[name + ".bias"],
                             rows_accumulate=rowadd is not None and self._row_parent.get(id(rowadd)) is not None, pad=pad)
                self._pin(dy, x, drow)
                self._done(*done)
            if rowadd is not None and self._row_parent.get(id(rowadd)) is None:
                self._acc(rowadd, drow, True)
            if res is not None:
                # (everything below that reads dy is enqueued before anyone adds to it -- unless the weight gradient above is
                #  queued: then dy must stay as it is until the flush, and later gradients of `res` go to a buffer of their own)
                self._acc(res, dy, dy_owned and not self._dy_shared)
            if need_dx:
                wt = self.wt[w]
                Cin = x.shape[3]
                cur = self._slot(x) if mode != 1 else None
                if stride == 2:
                    dx = T.conv(dy, wt, Cin, taps, 1, 2, out=cur, accumulate=cur is not None, pad=pad)
                elif mode == 1:
                    dx = T.sum2x2(T.conv(dy, wt, Cin, taps, 1, 0))
                else:
                    dx = T.conv(dy, wt, Cin, taps, 1, 0, out=cur, accumulate=cur is not None)
                if cur is None:
                    self._acc(x, dx, True)
        self._tape.append(bwd)
        return y

    def _gn(self, x, name, silu):
        cfg = self.cfg
        gamma, beta = self.p[name + ".weight"], self.p[name + ".bias"]
        y, stats = T.gn_forward(x, gamma, beta, cfg.norm_num_groups, cfg.norm_eps, silu)

        def bwd():
            dy = self._pop(y)
            cur = self._slot(x)
            dg, db = (self.g[name + ".weight"], self.g[name + ".bias"]) if self._params_on else self._sink(2 * gamma.numel()).chunk(2)
            dx = T.gn_backward(x, dy, stats, gamma, beta, cfg.norm_num_groups, silu, dg, db, dx=cur, accumulate=cur is not None)
            if self._params_on:
                self._done(name + ".weight", name + ".bias")
            if cur is None:
                self._acc(x, dx, True)
        self._tape.append(bwd)
        return y

    def _silu(self, x):
        y = T.silu(x)

        def bwd():
            dy = self._pop(y)
            self._acc(x, T.silu_backward(x, dy), True)
        self._tape.append(bwd)
        return y
