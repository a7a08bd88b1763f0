"""step_amd/optim.py -- FlatAdam / FlatSGD: the optimizers of the training step.

The reference builds `optim.Adam(params, lr=args.det_lr)` (train.py:126) over the single-tensor parameter groups of
utils/solver.py:12-93 (each with its own lr / weight_decay) and calls `optimizer.step()` once per iteration
(train.py:348); its schedulers (solver.py:96-180) rewrite `group['lr']` between steps.  Same constructor, same
`param_groups` / `zero_grad` / `step` / `state_dict` surface here, but MI355X-first underneath:

* every trainable parameter is re-homed into ONE flat fp32 arena (`p.data` becomes a view of it), its gradient into
  a second arena (`p.grad` is a view; autograd accumulates in place), the two Adam moments into two more;
* `step()` is ONE launch of `step_adam_flat` (include/step_amd.h) over the arenas -- pure HBM streaming, 28 B/element;
* the gradient arena is one contiguous buffer, so the data-parallel exchange is a single large RCCL all-reduce
  (`step_amd.dist.allreduce_flat`, no bucket copies: xGMI rings are per-link bound, few large messages win), and the
  1/world_size of the average and the gradient clear are folded into the Adam pass (`grad_scale`, `zero_grad`).

The reference's DEFAULT optimizer is `optim.SGD(params, lr=args.det_lr, momentum=args.momentum, weight_decay=args.weight_decay)`
(train.py:123-124, config.py:51-57): FlatSGD is the same scheme on three arenas (one momentum buffer) and `step_sgd_flat`, 20 B/element.
Both share the arena layer `_FlatOptimizer`, which is all that step_amd.dist and step_amd.workloads read.
"""
import torch

from . import _capi, _lib, wgrad

_ALIGN = 64          # elements (256 B): every tensor starts on its own cache line; segment ends stay multiples of 4


class LossScaler:
    """Dynamic loss scaling of mixed-precision (fp16) training -- what `amp.initialize(..., opt_level="O1")` + `with amp.scale_loss(loss,
    optimizer) as scaled_loss: scaled_loss.backward()` do in the reference (train.py:136-139,342-345) -- with the whole state on the device:
    `state` = {scale, growth_tracker, found_inf, -}.  Defaults are apex's DynamicLossScaler (2^16, x2 after 2000 clean steps, /2 on overflow),
    the same rule as torch.amp.GradScaler.  Use:

        scaler = LossScaler(device)
        scaler.scale_loss(loss).backward()          # a device multiply: nothing here reads the scale on the host
        opt.step(scaler=scaler, zero_grad=True)     # overflow scan + unscale + skip-or-step + scale update: step_adam_flat_amp

    The optimizer must be FlatAdam / FlatSGD(capturable=True): a skipped step must not advance the step count, and only the device knows
    (for FlatSGD the count also decides which step initialises the momentum buffer)."""

    def __init__(self, device, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.state = torch.tensor([float(init_scale), 0.0, 0.0, 0.0], dtype=torch.float32, device=device)

    def scale_loss(self, loss):
        return loss * self.state[0].to(loss.dtype)

    @property
    def scale(self):
        return float(self.state[0].item())

    def state_dict(self):
        s = self.state.tolist()
        return {"scale": s[0], "growth_tracker": int(s[1]), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval}

    def load_state_dict(self, sd):
        self.growth_factor, self.backoff_factor, self.growth_interval = float(sd["growth_factor"]), float(sd["backoff_factor"]), int(sd["growth_interval"])
        self.state.copy_(torch.tensor([float(sd["scale"]), float(sd["growth_tracker"]), 0.0, 0.0]))


class _FlatOptimizer(torch.optim.Optimizer):
    """The arena layer FlatAdam and FlatSGD share: parameters and gradients re-homed into `flat_param` / `flat_grad`, one zeroed arena
    per name in `state_arenas`, the `_entries` / `numel` / `_seg_*` tables the kernels, step_amd.dist and step_amd.workloads read, the
    host / device step count, and everything of step() around the subclass's launch (`_launch`)."""

    grad_wire = None                                             # a step_amd.dist.GradWire registers itself here (on the instance)
    lr_scheduler = None                                          # a DeviceWarmupCosineLR / DeviceWarmupStepLR attaches itself here: it owns _seg_lr
    grad_norm = None                                             # clip_grad_norm_ leaves {total_norm, clip_coef, nonfinite, 0} (device) here ...
    seg_grad_norm = None                                         # ... and the per-tensor norms, in the order of _entries, here
    _norm_ws = None

    def _check_groups(self):
        """hyper-parameters that one launch cannot vary must agree across the groups"""

    def _launch(self, L, grad_scale, zero_grad, scaler):
        raise NotImplementedError

    def __init__(self, params, defaults, state_arenas, capturable):
        # the base class normalises `params` into self.param_groups (fills the defaults, rejects duplicates) exactly as it does for
        # torch's own optimizers
        super().__init__(params, defaults)
        name = type(self).__name__
        self._check_groups()
        self._entries = []                                       # (group index, parameter, offset, numel)
        off = 0
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if not p.requires_grad:
                    continue
                if p.dtype != torch.float32:
                    raise RuntimeError("%s: fp32 master parameters expected, got %s" % (name, p.dtype))
                self._entries.append((gi, p, off, p.numel()))
                off += -(-p.numel() // _ALIGN) * _ALIGN
        if not self._entries:
            raise ValueError("%s: no trainable parameter" % name)
        if len(self._entries) > 4096:
            raise RuntimeError("%s: more than 4096 tensors" % name)
        dev = self._entries[0][1].device
        if any(p.device != dev for _, p, _, _ in self._entries):
            raise RuntimeError("%s: all parameters must live on one device (one process per GPU)" % name)
        _lib.dptr(self._entries[0][1].data)                      # refuses non-device tensors: there is no CPU fallback
        self.device, self.numel = dev, off
        self.flat_param = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(off, dtype=torch.float32, device=dev)
        for a in state_arenas:
            setattr(self, a, torch.zeros(off, dtype=torch.float32, device=dev))
        with torch.no_grad():
            for _, p, o, n in self._entries:
                self.flat_param[o:o + n].copy_(p.data.reshape(-1))
                p.data = self.flat_param[o:o + n].view(p.shape)
                if p.grad is not None:
                    self.flat_grad[o:o + n].copy_(p.grad.reshape(-1))
                p.grad = self.flat_grad[o:o + n].view(p.shape)
        ends = [o + -(-n // _ALIGN) * _ALIGN for _, _, o, n in self._entries]
        self._seg_end = torch.tensor(ends, dtype=torch.int64, device=dev)
        self._seg_lr = torch.zeros(len(ends), dtype=torch.float32, device=dev)
        self._seg_wd = torch.zeros(len(ends), dtype=torch.float32, device=dev)
        self._tables = None
        # capturable (as torch.optim.Adam's flag): the step counter lives on the device and step() is free of host scalars, so a
        # whole training step can be captured in a HIP graph and replayed (step_adam_flat_dev / step_sgd_flat_dev)
        self.capturable = bool(capturable)
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._step_host = 0

    @property
    def step_count(self):
        return int(self._step_dev.item()) if self.capturable else self._step_host

    @step_count.setter
    def step_count(self, v):
        self._step_host = int(v)
        self._step_dev.fill_(int(v))

    # -- torch.optim.Optimizer surface ---------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        """optimizer.zero_grad() (train.py:287).  Gradients stay views of the arena (set_to_none is ignored)."""
        self.flat_grad.zero_()
        for _, p, o, n in self._entries:
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * o:
                p.grad = self.flat_grad[o:o + n].view(p.shape)

    def _gather_stray_grads(self):
        # a caller that replaced p.grad (set_to_none, grad = tensor): fold it back into the arena.
        # Known divergence from torch.optim.Adam / SGD (documented, not emulated): torch SKIPS a parameter whose .grad is None -- no
        # moment decay, no step count -- while the one launch here treats it as a zero gradient at the shared step count (its
        # moments decay and the parameter keeps moving along exp_avg / the momentum buffer).  The reference's loop never produces that
        # case: every parameter of get_params() receives a gradient in every iteration (train.py:318-348), and zero_grad() here keeps
        # the gradients as views of the arena instead of dropping them.
        base = self.flat_grad.data_ptr()
        for _, p, o, n in self._entries:
            g = p.grad
            if g is None:
                self.flat_grad[o:o + n].zero_()
                p.grad = self.flat_grad[o:o + n].view(p.shape)
            elif g.data_ptr() != base + 4 * o:
                self.flat_grad[o:o + n].copy_(g.reshape(-1))
                p.grad = self.flat_grad[o:o + n].view(p.shape)

    def _refresh_tables(self):
        lr = [float(self.param_groups[gi]["lr"]) for gi, _, _, _ in self._entries]
        wd = [float(self.param_groups[gi]["weight_decay"]) for gi, _, _, _ in self._entries]
        if self.lr_scheduler is not None:                        # a device scheduler writes _seg_lr itself (step_lr_schedule): only the decay
            if self._tables != (None, wd):
                self._seg_wd.copy_(torch.tensor(wd, dtype=torch.float32))
                self._tables = (None, wd)
            return
        if self._tables != (lr, wd):                             # the schedulers rewrite group['lr'] every iteration
            self._seg_lr.copy_(torch.tensor(lr, dtype=torch.float32))
            self._seg_wd.copy_(torch.tensor(wd, dtype=torch.float32))
            self._tables = (lr, wd)

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm, grad_scale=1.0, scaler=None, norm_type=2.0):
        """torch.nn.utils.clip_grad_norm_(params, max_norm) over the gradient arena, on the device: one streaming pass and a finishing launch
        (step_grad_norm_flat), then the in-place multiply (step_grad_clip_flat), which touches nothing on a step that is not clipped.
        Returns the total norm as a DEVICE scalar -- nothing here synchronises, so the call can be recorded in a captured step -- and leaves
        `self.grad_norm` = {total_norm, clip_coef, nonfinite, 0} and `self.seg_grad_norm` (one norm per tensor, the order of `_entries`)
        behind.  The workspace is allocated on the first call: the warm-up steps ahead of a capture create it.

        Units: the norm is that of grad * |grad_scale| (the factor step() takes: 1 / world after a SUM all-reduce), divided by the loss
        scale when `scaler` is given -- a LossScaler step is clipped in UN-scaled units.  Only the L2 norm is supported.
        GradWire: call this after the exchange (step(max_grad_norm=) does): it acts on the exchanged gradient, the wire's residual is not
        involved.  LossScaler: an inf / NaN gradient (or a norm beyond fp32) gives nonfinite = 1 and a coefficient of 1 -- the gradient
        is left as it is, where torch would multiply it by 0 or NaN, so that the scaler's own scan in step() still skips the step."""
        if float(norm_type) != 2.0:
            raise ValueError("%s.clip_grad_norm_: only the L2 norm (norm_type=2) is supported, got %r" % (type(self).__name__, norm_type))
        from . import ops
        if self.grad_norm is None:
            self._norm_ws = ops.grad_norm_workspace(self.numel, len(self._entries), self.device)
            self.grad_norm = torch.zeros(4, dtype=torch.float32, device=self.device)
            self.seg_grad_norm = torch.zeros(len(self._entries), dtype=torch.float32, device=self.device)
        ops.grad_norm_flat(self.flat_grad, self._seg_end, max_norm, grad_scale=grad_scale, amp_state=None if scaler is None else scaler.state,
                           workspace=self._norm_ws, seg_norm=self.seg_grad_norm, stats=self.grad_norm)
        ops.grad_clip_flat(self.flat_grad, self.grad_norm)
        return self.grad_norm[0]

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, zero_grad=False, scaler=None, max_grad_norm=None, norm_type=2.0):
        """optimizer.step() (train.py:348): one kernel launch.  grad_scale multiplies every gradient on the way in
        (1/world_size after a SUM all-reduce, 1/loss_scale); zero_grad=True clears the gradient arena in the same pass.
        scaler = a LossScaler whose scale the loss was multiplied by: the gradients are scanned for inf / nan, unscaled, and the
        step is skipped on overflow (apex O1 / GradScaler semantics), all on the device (step_adam_flat_amp / step_sgd_flat_amp).
        max_grad_norm = a positive number: clip_grad_norm_(max_grad_norm, grad_scale, scaler) runs ahead of the update -- behind the
        side-stream weight gradients and the stray-gradient fold, hence on the exchanged gradient (a GradWire's residual is not involved),
        in un-scaled units under a LossScaler, whose skip an overflow still reaches (see clip_grad_norm_).  None launches nothing."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        wgrad.STATE.sync()                                       # weight gradients still in flight on the side stream
        self._gather_stray_grads()
        self._refresh_tables()
        if scaler is not None and not self.capturable:
            raise RuntimeError("%s.step(scaler=...): build the optimizer with capturable=True (a skipped step must not count, "
                               "and only the device knows whether it was skipped)" % type(self).__name__)
        if scaler is not None and self.grad_wire is not None and self.grad_wire.error_feedback:
            raise RuntimeError("%s.step(scaler=...): the gradient wire keeps an error-feedback residual, which would be in units of a loss "
                               "scale that changes on overflow -- use GradWire(error_feedback=False) with a LossScaler" % type(self).__name__)
        if max_grad_norm is not None:
            self.clip_grad_norm_(max_grad_norm, grad_scale=grad_scale, scaler=scaler, norm_type=norm_type)
        self._launch(_lib.lib(), float(grad_scale), int(bool(zero_grad)), scaler)
        # the kernel wrote through raw pointers: bump the autograd version counters (the packed-weight caches of
        # backbone.py / heads.py are keyed on them)
        torch.autograd.graph.increment_version([p for _, p, _, _ in self._entries])
        return loss

    # -- checkpoints: torch's own structure ({"state": {index: {...}}, "param_groups": [... "params": [indices]]}) ------------------
    def _pack_groups(self):
        idx, k, packed_groups = {}, 0, []
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                idx[id(p)] = k
                ids.append(k)
                k += 1
            pg = {kk: vv for kk, vv in g.items() if kk != "params"}
            pg["params"] = ids
            packed_groups.append(pg)
        return packed_groups, idx

    def _unpack_groups(self, sd):
        groups = sd["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("%s.load_state_dict: parameter groups do not match" % type(self).__name__)
        idx = {}
        for a, b in zip(groups, self.param_groups):
            for k, p in zip(a["params"], b["params"]):
                idx[id(p)] = k
            for kk, vv in a.items():
                if kk != "params":
                    b[kk] = vv
        self._tables = None
        return idx


class FlatAdam(_FlatOptimizer):
    """A torch.optim.Optimizer (the reference's schedulers subclass torch's _LRScheduler, which insists on one:
    utils/solver.py:96,141) whose whole state lives in four flat arenas."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False):
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), ("exp_avg", "exp_avg_sq"), capturable)
        self._bias_corr = torch.zeros(2, dtype=torch.float32, device=self.device)

    def _check_groups(self):
        b, e = self.param_groups[0]["betas"], self.param_groups[0]["eps"]
        if any(tuple(g["betas"]) != tuple(b) or g["eps"] != e for g in self.param_groups):
            raise ValueError("FlatAdam: betas / eps must be the same for every group (one launch)")

    def _launch(self, L, grad_scale, zero_grad, scaler):
        g0 = self.param_groups[0]
        head = (_lib.dptr(self.flat_param), _lib.dptr(self.flat_grad), _lib.dptr(self.exp_avg), _lib.dptr(self.exp_avg_sq), self.numel,
                _lib.dptr(self._seg_end), _lib.dptr(self._seg_lr), _lib.dptr(self._seg_wd), len(self._entries), float(g0["betas"][0]),
                float(g0["betas"][1]), float(g0["eps"]))
        if scaler is not None:
            _capi.check(L.step_adam_flat_amp(*head, _lib.dptr(self._step_dev), _lib.dptr(self._bias_corr), grad_scale, zero_grad,
                                             _lib.dptr(scaler.state), scaler.growth_factor, scaler.backoff_factor, scaler.growth_interval,
                                             _lib.stream_ptr(self.device)), "step_adam_flat_amp")
        elif self.capturable:
            _capi.check(L.step_adam_flat_dev(*head, _lib.dptr(self._step_dev), _lib.dptr(self._bias_corr), grad_scale, zero_grad,
                                             _lib.stream_ptr(self.device)), "step_adam_flat_dev")
        else:
            self._step_host += 1
            _capi.check(L.step_adam_flat(*head, self._step_host, grad_scale, zero_grad, _lib.stream_ptr(self.device)), "step_adam_flat")

    def state_dict(self):
        """Same structure as torch.optim.Adam.state_dict() (checkpoints: train.py:382,437)."""
        packed_groups, idx = self._pack_groups()
        state = {}
        if self.step_count:
            for _, p, o, n in self._entries:
                state[idx[id(p)]] = {"step": torch.tensor(float(self.step_count)),
                                     "exp_avg": self.exp_avg[o:o + n].view(p.shape).clone(),
                                     "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).clone()}
        return {"state": state, "param_groups": packed_groups}

    def load_state_dict(self, sd):
        """optimizer.load_state_dict(checkpoint['optimizer']) (train.py:205); accepts torch.optim.Adam's own dicts."""
        idx = self._unpack_groups(sd)
        steps = set()
        with torch.no_grad():
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            for _, p, o, n in self._entries:
                st = sd["state"].get(idx[id(p)])
                if st is None:
                    steps.add(0)
                    continue
                steps.add(int(float(st["step"])))
                self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
        if len(steps) != 1:
            raise ValueError("FlatAdam.load_state_dict: parameters are at different step counts %s" % sorted(steps))
        self.step_count = steps.pop()


class FlatSGD(_FlatOptimizer):
    """The reference's default optimizer -- `optim.SGD(params, lr=args.det_lr, momentum=args.momentum, weight_decay=args.weight_decay)`
    (train.py:123-124; config.py:51-57: momentum 0.9, weight decay 1e-7) -- on three flat arenas: same constructor arguments, same
    `param_groups` / `zero_grad` / `step` / `state_dict` surface, accepted by the reference's _LRScheduler subclasses (utils/solver.py:96,141);
    step() is ONE launch of `step_sgd_flat` (include/step_amd.h), 12 B read + 8 B written per element.  `momentum`, `dampening` and
    `nesterov` must agree across the groups (one launch); `lr` and `weight_decay` are per group.  momentum == 0 keeps no buffer
    (`momentum_buffer` is None), as torch keeps no state then.

    torch's SGD has no step number: a parameter's "momentum_buffer" being present means "past the first step", which only decides whether
    the buffer is initialised (buf = g) or updated.  Here `step_count` plays that role for all parameters at once, on the device when
    capturable=True -- a step skipped by the loss scaler does not count, so the first clean step still initialises the buffer.
    The divergence documented in `_gather_stray_grads` (a parameter whose .grad is None is treated as a zero gradient instead of
    being skipped) applies here as it does to FlatAdam."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, capturable=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %r" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        # (maximize / foreach / differentiable / fused: torch.optim.SGD's remaining group keys at their defaults, so that a state_dict
        # of this class loads into torch's and the loaded optimizer can step)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False,
                        foreach=None, differentiable=False, fused=None)
        groups = list(params)
        first = groups[0] if groups and isinstance(groups[0], dict) else {}
        state = ("momentum_buffer",) if first.get("momentum", momentum) != 0 else ()
        super().__init__(groups, defaults, state, capturable)
        if not state:
            self.momentum_buffer = None

    def _check_groups(self):
        g0 = self.param_groups[0]
        key = lambda g: (g["momentum"], g["dampening"], bool(g["nesterov"]))
        if any(key(g) != key(g0) for g in self.param_groups):
            raise ValueError("FlatSGD: momentum / dampening / nesterov must be the same for every group (one launch)")
        if g0["momentum"] < 0.0:
            raise ValueError("Invalid momentum value: %r" % (g0["momentum"],))
        if g0["nesterov"] and (g0["momentum"] <= 0 or g0["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if any(g.get("maximize") for g in self.param_groups):
            raise ValueError("FlatSGD: maximize is not supported")

    def _launch(self, L, grad_scale, zero_grad, scaler):
        g0 = self.param_groups[0]
        if (g0["momentum"] != 0) != (self.momentum_buffer is not None):
            raise RuntimeError("FlatSGD: momentum changed between zero and non-zero after construction (the buffer arena is fixed)")
        head = (_lib.dptr(self.flat_param), _lib.dptr(self.flat_grad), _lib.dptr(self.momentum_buffer), self.numel, _lib.dptr(self._seg_end),
                _lib.dptr(self._seg_lr), _lib.dptr(self._seg_wd), len(self._entries), float(g0["momentum"]), float(g0["dampening"]),
                int(bool(g0["nesterov"])))
        if scaler is not None:
            _capi.check(L.step_sgd_flat_amp(*head, _lib.dptr(self._step_dev), grad_scale, zero_grad, _lib.dptr(scaler.state),
                                            scaler.growth_factor, scaler.backoff_factor, scaler.growth_interval,
                                            _lib.stream_ptr(self.device)), "step_sgd_flat_amp")
        elif self.capturable:
            _capi.check(L.step_sgd_flat_dev(*head, _lib.dptr(self._step_dev), grad_scale, zero_grad, _lib.stream_ptr(self.device)),
                        "step_sgd_flat_dev")
        else:
            self._step_host += 1
            _capi.check(L.step_sgd_flat(*head, self._step_host, grad_scale, zero_grad, _lib.stream_ptr(self.device)), "step_sgd_flat")

    def state_dict(self):
        """Same structure as torch.optim.SGD.state_dict() (checkpoints: train.py:382,437): state[k] = {"momentum_buffer": tensor} once a
        step was taken with momentum != 0, nothing before (and nothing at all with momentum == 0)."""
        packed_groups, idx = self._pack_groups()
        state = {}
        if self.momentum_buffer is not None and self.step_count:
            for _, p, o, n in self._entries:
                state[idx[id(p)]] = {"momentum_buffer": self.momentum_buffer[o:o + n].view(p.shape).clone()}
        return {"state": state, "param_groups": packed_groups}

    def load_state_dict(self, sd):
        """optimizer.load_state_dict(checkpoint['optimizer']) (train.py:205); accepts torch.optim.SGD's own dicts.  No buffers in the
        dict: the step count is reset to 0 (the next step initialises the buffer); buffers present: the count becomes >= 1 (it is kept
        when it already is, torch's dicts carry no step number)."""
        idx = self._unpack_groups(sd)
        self._check_groups()
        have = set()
        with torch.no_grad():
            if self.momentum_buffer is not None:
                self.momentum_buffer.zero_()
            for _, p, o, n in self._entries:
                st = sd["state"].get(idx[id(p)])
                buf = None if st is None else st.get("momentum_buffer")
                have.add(buf is not None)
                if buf is not None:
                    if self.momentum_buffer is None:
                        raise ValueError("FlatSGD.load_state_dict: the checkpoint holds momentum buffers, this optimizer was built with momentum == 0")
                    self.momentum_buffer[o:o + n].copy_(buf.reshape(-1))
        if len(have) != 1:
            raise ValueError("FlatSGD.load_state_dict: some parameters have a momentum buffer and some do not")
        self.step_count = max(self.step_count, 1) if have.pop() else 0


class _DeviceLRScheduler:
    """The reference's per-iteration learning-rate schedules (utils/solver.py:96-172; `scheduler.step()` at train.py:262) with the iteration
    counter and the arithmetic on the device: `.step()` is ONE launch of step_lr_schedule, which advances `last_epoch` (an int64 on the
    device) and writes the optimizer's `seg_lr` table, so it can be recorded in a captured training step ahead of `optimizer.step()` and
    a replayed iteration takes no learning rate from the host.  For FlatAdam / FlatSGD built with capturable=True.

    As torch's _LRScheduler: the base lrs are the groups' `initial_lr` (set from `lr` at construction when last_epoch == -1, required
    otherwise), and construction takes the first step (last_epoch -1 -> 0).  The schedule's counter is its own: a step the LossScaler
    skips for overflow still advances it, as the reference's loop does.  While a scheduler is attached the optimizer's `_refresh_tables`
    keeps writing the weight decay but leaves `seg_lr` alone; `param_groups[i]['lr']` is refreshed by get_last_lr() (which synchronises),
    for logging."""

    _kind = None

    def __init__(self, optimizer, milestones, warmup_iters, warmup_factor, last_epoch, p0, p1):
        if not isinstance(optimizer, _FlatOptimizer) or not optimizer.capturable:
            raise RuntimeError("%s: wants a FlatAdam / FlatSGD built with capturable=True" % type(self).__name__)
        milestones = [int(m) for m in milestones]
        if milestones != sorted(milestones):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(milestones))
        table = self._table(milestones, int(warmup_iters))
        if len(table) > 64:
            raise ValueError("%s: at most 64 milestones" % type(self).__name__)
        if any(b <= a for a, b in zip(table, table[1:])) and self._kind == "cosine":
            raise ValueError("%s: warmup_iters and the milestones must be strictly increasing, got %s" % (type(self).__name__, table))
        if optimizer.lr_scheduler is not None:
            raise RuntimeError("%s: the optimizer already has a device scheduler" % type(self).__name__)
        self.optimizer, self.milestones = optimizer, milestones
        self.warmup_iters, self.warmup_factor = int(warmup_iters), float(warmup_factor)
        self._p0, self._p1 = float(p0), float(p1)
        if last_epoch == -1:
            for g in optimizer.param_groups:
                g.setdefault("initial_lr", g["lr"])
        elif any("initial_lr" not in g for g in optimizer.param_groups):
            raise KeyError("param 'initial_lr' is not specified in param_groups when resuming an optimizer")
        self.base_lrs = [float(g["initial_lr"]) for g in optimizer.param_groups]
        dev = optimizer.device
        self._base = torch.tensor([self.base_lrs[gi] for gi, _, _, _ in optimizer._entries], dtype=torch.float64).to(dev)
        self._ms = torch.tensor(table, dtype=torch.int64).to(dev)
        self._iter = torch.full((1,), int(last_epoch), dtype=torch.int64).to(dev)
        optimizer.lr_scheduler = self
        optimizer._tables = None
        self.step()                                              # torch's _initial_step

    def _table(self, milestones, warmup_iters):
        return milestones

    def step(self):
        from . import ops
        ops.lr_schedule(self._kind, self._iter, self._base, self.optimizer._seg_lr, self._ms, self.warmup_iters, self.warmup_factor, self._p0, self._p1)

    @property
    def last_epoch(self):
        return int(self._iter.item())

    def get_last_lr(self):
        """the learning rates the last step() wrote, one per group (reads the device table: synchronises); also refreshes
        param_groups[i]['lr'] for logging"""
        table = self.optimizer._seg_lr.tolist()
        lrs = list(self.base_lrs)
        for k, (gi, _, _, _) in enumerate(self.optimizer._entries):
            lrs[gi] = table[k]
        for g, lr in zip(self.optimizer.param_groups, lrs):
            g["lr"] = lr
        return lrs

    def state_dict(self):
        return {"last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        """resume: the counter is set to last_epoch and seg_lr re-evaluated for it (no step is taken)"""
        self._iter.fill_(int(sd["last_epoch"]) - 1)
        self.step()


class DeviceWarmupCosineLR(_DeviceLRScheduler):
    """utils/solver.py:96-138 WarmupCosineLR -- linear warm-up, then cosine annealing with restarts at `milestones`, the peak decayed by
    `cycle_decay` per cycle, the floor at `min_ratio` x base -- on the device (see _DeviceLRScheduler)."""
    _kind = "cosine"

    def __init__(self, optimizer, milestones, min_ratio=0., cycle_decay=1., warmup_iters=1000, warmup_factor=1. / 10, last_epoch=-1):
        self.min_ratio, self.cycle_decay = min_ratio, cycle_decay
        super().__init__(optimizer, milestones, warmup_iters, warmup_factor, last_epoch, min_ratio, cycle_decay)

    def _table(self, milestones, warmup_iters):
        return [warmup_iters] + milestones                       # the reference's own table (solver.py:116)


class DeviceWarmupStepLR(_DeviceLRScheduler):
    """utils/solver.py:140-172 WarmupStepLR -- linear warm-up, then base x gamma^(milestones passed) -- on the device (see
    _DeviceLRScheduler)."""
    _kind = "step"

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_iters=1000, warmup_factor=1. / 10, last_epoch=-1):
        self.gamma = gamma
        super().__init__(optimizer, milestones, warmup_iters, warmup_factor, last_epoch, gamma, 1.0)
