"""Fused optimisers over the engine's flat fp32 parameter / gradient buffers (one kernel per step).

Same update rules and defaults as the torch.optim classes the reference wires up
(/root/reference/chexpert.py:470 Adam(lr); :479 SGD(momentum=0.9, nesterov=True); :499
RMSprop(momentum=0.9, eps=1e-3)), with the schedulers of :480 (MultiStepLR[40000, 60000]) and :500
(ExponentialLR(gamma)) folded in as `scheduler_step()`.
"""
import contextlib

import torch

from . import ops


class _Flat:
    """Options shared by the three optimisers (all off by default: `step()` / `step_dev()` then launch the plain one-kernel update):

      max_grad_norm   clip the gradient to this global L2 norm (torch.nn.utils.clip_grad_norm_'s rule), on the device
      skip_nonfinite  drop the whole update of a step whose gradient norm is inf or NaN (no parameter, state or EMA element written)
      ema_decay       keep an exponential moving average of the parameters, written by the optimiser kernel itself
      ema_warmup      decay = min(ema_decay, (1 + t) / (10 + t)) at step t, so the average forgets its start quickly

    With any of them on the step is `cx_grad_norm` (when clipping or skipping) + the `_ex` update.  The scheduler and Adam's bias
    correction count minibatches, skipped ones included."""
    NSTATE = 0

    def __init__(self, model, lr, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=True):
        self.model = model
        self.lr = float(lr)
        self.base_lr = float(lr)
        self.step_count = 0
        self.sched_steps = 0
        self._state = None
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be > 0 (got %r)" % (max_grad_norm,))
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError("ema_decay must lie in (0, 1) (got %r)" % (ema_decay,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._ws = self._clip = self._ema = None
        self._pending_ex = None

    def _norm_on(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _ex_on(self):
        return self._norm_on() or self.ema_decay is not None

    def _bufs(self, n):
        eng = self.model._eng()
        if eng.flat is None:
            raise RuntimeError("run a forward pass first (parameters are bound to the flat buffer lazily)")
        if self._state is None or self._state[0].numel() != eng.flat.numel() or self._state[0].device != eng.flat.device:
            self._state = [torch.zeros_like(eng.flat) for _ in range(n)]
            pend = getattr(self, "_pending_state", None)
            if pend is not None:
                for dst, src in zip(self._state, pend):
                    dst.copy_(src)
                self._pending_state = None
        if self._ex_on() and (self._clip is None or self._clip.device != eng.flat.device
                              or (self._ema is not None and self._ema.numel() != eng.flat.numel())):
            # beside the states, so that nothing is allocated while a graph is being captured
            self._ws = torch.zeros(max(1, ops.grad_norm_partials(eng.flat.numel())), dtype=torch.float32, device=eng.flat.device)
            self._clip = torch.zeros(4, dtype=torch.float32, device=eng.flat.device)
            self._clip[1] = 1.0
            self._ema = eng.flat.detach().clone() if self.ema_decay is not None else None
            pend, self._pending_ex = self._pending_ex, None
            if pend is not None:
                self._clip[3] = float(pend.get("skipped", 0))
                if self._ema is not None and pend.get("ema") is not None:
                    self._ema.copy_(pend["ema"])
        return eng.flat, eng.flat_grad, self._state

    def _ex_args(self, g, grad_scale):
        """Launches the norm when clipping or skipping is on; keyword arguments of the `_ex` update that follows."""
        if self._norm_on():
            ops.grad_norm(g, self._ws, self._clip, grad_scale, self.max_grad_norm or 0.0, self.skip_nonfinite)
        return {"clip": self._clip if self._norm_on() else None, "ema": self._ema, "ema_decay": self.ema_decay or 0.0,
                "ema_warmup": self.ema_warmup, "skip_nonfinite": self.skip_nonfinite}

    def _clip_host(self):
        if not self._norm_on():
            raise RuntimeError("the gradient norm is computed only with max_grad_norm or skip_nonfinite")
        return None if self._clip is None else self._clip.cpu()

    def grad_norm(self):
        """L2 norm of the (unscaled) gradient of the most recent step, before clipping.  Reads the device: synchronises."""
        c = self._clip_host()
        return 0.0 if c is None else float(c[0])

    def skipped_steps(self):
        """Steps dropped so far because their gradient was not finite.  Reads the device: synchronises."""
        c = self._clip_host()
        if c is None:
            return int((self._pending_ex or {}).get("skipped", 0))
        return int(c[3])

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model computes with the averaged weights: the contents of the flat parameter buffer and of the EMA
        are swapped on entry and swapped back on exit.  BatchNorm running statistics are not averaged (they already are moving
        averages)."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weights() needs an optimiser built with ema_decay")
        eng = self.model._eng()
        p, _, _ = self._bufs(self.NSTATE)

        def swap():
            tmp = p.detach().clone()
            p.detach().copy_(self._ema)
            self._ema.copy_(tmp)
            eng.packed_version = None          # the packed bf16 weights are rebuilt from the flat buffer on the next forward
        swap()
        try:
            yield self
        finally:
            swap()

    def zero_grad(self, set_to_none=True):
        self.model.zero_grad(set_to_none=set_to_none)

    # ---- device-resident hyper-parameters (graph replay: chexpert_amd/graph.py)
    SCHED = (0, 1.0, (0, 0))        # (kind, gamma, milestones): 0 none, 1 ExponentialLR, 2 MultiStepLR

    def hyper(self, warmup_steps=0):
        """float[8] on the device: {lr, steps_done, sched_kind, gamma, lr_warmup_steps, milestone0, milestone1, base_lr}
        (include/chexpert_hip.h, cx_optim_tick).  Created from the host-side state on first use; from then on the device
        copy is the truth for `step_dev()` / `tick()` and `sync_from_device()` reads it back."""
        if getattr(self, "_hyper", None) is None:
            kind, gamma, ms = self.SCHED if not hasattr(self, "_sched") else self._sched
            eng = self.model._eng()
            self._hyper = torch.tensor([self.lr, float(self.step_count), float(kind), float(gamma), float(warmup_steps),
                                        float(ms[0]), float(ms[1]), self.base_lr], dtype=torch.float32, device=eng.flat.device)
        return self._hyper

    def tick(self):
        """steps_done += 1 and the scheduler step of chexpert.py:165, on the device."""
        ops.optim_tick(self.hyper())

    def state_dict(self):
        """What the reference saves as `optim_checkpoint_latest.pt` (chexpert.py:188-189), for the flat-buffer state."""
        self.sync_from_device()
        sd = {"kind": type(self).__name__, "lr": self.lr, "base_lr": self.base_lr, "step_count": self.step_count,
              "sched_steps": self.sched_steps, "state": None if self._state is None else [t.detach().cpu().clone() for t in self._state]}
        if self._ex_on():
            pend = self._pending_ex or {}
            sd.update({"max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite, "ema_decay": self.ema_decay,
                       "ema_warmup": self.ema_warmup,
                       "skipped": int(self._clip[3]) if self._clip is not None else int(pend.get("skipped", 0)),
                       "ema": self._ema.detach().cpu().clone() if self._ema is not None else pend.get("ema")})
        return sd

    def load_state_dict(self, sd):
        if sd.get("kind") != type(self).__name__:
            raise RuntimeError("optimizer checkpoint was written by %s, this is %s" % (sd.get("kind"), type(self).__name__))
        self.lr, self.base_lr, self.step_count, self.sched_steps = sd["lr"], sd["base_lr"], sd["step_count"], sd["sched_steps"]
        self._pending_state = sd["state"]              # copied into the flat-buffer state once the engine is bound
        self._hyper = None
        if "max_grad_norm" in sd:                      # (a checkpoint written without these options leaves them as constructed)
            self.max_grad_norm, self.skip_nonfinite = sd["max_grad_norm"], bool(sd["skip_nonfinite"])
            self.ema_decay, self.ema_warmup = sd["ema_decay"], bool(sd["ema_warmup"])
            self._pending_ex = {"skipped": int(sd.get("skipped", 0)), "ema": sd.get("ema")}
            self._ws = self._clip = self._ema = None

    def sync_from_device(self):
        if getattr(self, "_hyper", None) is not None:
            h = self._hyper.cpu()
            self.lr, self.step_count = float(h[0]), int(h[1])
            # cx_optim_tick steps the scheduler inside the graph: after minibatch number `step` it has been stepped
            # step - max(warm-up, 1) + 1 times (chexpert.py:157-165), which is what an eager resume continues from
            if int(h[2]) != 0:
                self.sched_steps = max(0, int(h[1]) - max(int(h[4]), 1) + 1)


class FusedAdam(_Flat):
    NSTATE = 2

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **options):
        super().__init__(model, lr, **options)
        self.betas, self.eps, self.wd = betas, eps, weight_decay

    def step(self, grad_scale=1.0):
        p, g, (m, v) = self._bufs(2)
        self.step_count += 1
        if self._ex_on():
            ops.adam_step_ex(p, g, m, v, self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.step_count, grad_scale,
                             **self._ex_args(g, grad_scale))
            return
        ops.adam_step(p, g, m, v, self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.step_count, grad_scale)

    def step_dev(self, grad_scale=1.0):
        p, g, (m, v) = self._bufs(2)
        if self._ex_on():
            ops.adam_step_dev_ex(p, g, m, v, self.hyper(), self.betas[0], self.betas[1], self.eps, self.wd, grad_scale,
                                 **self._ex_args(g, grad_scale))
            return
        ops.adam_step_dev(p, g, m, v, self.hyper(), self.betas[0], self.betas[1], self.eps, self.wd, grad_scale)


class FusedSGDNesterov(_Flat):
    NSTATE = 1

    def __init__(self, model, lr, momentum=0.9, weight_decay=0.0, milestones=(40000, 60000), gamma=0.1, **options):
        super().__init__(model, lr, **options)
        self.momentum, self.wd, self.milestones, self.gamma = momentum, weight_decay, tuple(milestones), gamma
        ms = (tuple(milestones) + (1 << 30, 1 << 30))[:2]
        self._sched = (2, gamma, ms)

    def step_dev(self, grad_scale=1.0):
        p, g, (buf,) = self._bufs(1)
        if self._ex_on():
            ops.sgd_nesterov_step_dev_ex(p, g, buf, self.hyper(), self.momentum, self.wd, grad_scale, **self._ex_args(g, grad_scale))
            return
        ops.sgd_nesterov_step_dev(p, g, buf, self.hyper(), self.momentum, self.wd, grad_scale)

    def step(self, grad_scale=1.0):
        p, g, (buf,) = self._bufs(1)
        if self._ex_on():
            ops.sgd_nesterov_step_ex(p, g, buf, self.lr, self.momentum, self.wd, self.step_count == 0, self.step_count + 1, grad_scale,
                                     **self._ex_args(g, grad_scale))
        else:
            ops.sgd_nesterov_step(p, g, buf, self.lr, self.momentum, self.wd, self.step_count == 0, grad_scale)
        self.step_count += 1

    def scheduler_step(self):
        self.sched_steps += 1
        self.lr = self.base_lr * self.gamma ** sum(self.sched_steps >= m for m in self.milestones)


class FusedRMSprop(_Flat):
    NSTATE = 2

    def __init__(self, model, lr, alpha=0.99, eps=1e-3, momentum=0.9, weight_decay=0.0, decay=0.97, **options):
        super().__init__(model, lr, **options)
        self.alpha, self.eps, self.momentum, self.wd, self.decay = alpha, eps, momentum, weight_decay, decay
        self._sched = (1, decay, (0, 0))

    def step_dev(self, grad_scale=1.0):
        p, g, (sq, buf) = self._bufs(2)
        if self._ex_on():
            ops.rmsprop_step_dev_ex(p, g, sq, buf, self.hyper(), self.alpha, self.eps, self.momentum, self.wd, grad_scale,
                                    **self._ex_args(g, grad_scale))
            return
        ops.rmsprop_step_dev(p, g, sq, buf, self.hyper(), self.alpha, self.eps, self.momentum, self.wd, grad_scale)

    def step(self, grad_scale=1.0):
        p, g, (sq, buf) = self._bufs(2)
        if self._ex_on():
            ops.rmsprop_step_ex(p, g, sq, buf, self.lr, self.alpha, self.eps, self.momentum, self.wd, self.step_count + 1, grad_scale,
                                **self._ex_args(g, grad_scale))
        else:
            ops.rmsprop_step(p, g, sq, buf, self.lr, self.alpha, self.eps, self.momentum, self.wd, grad_scale)
        self.step_count += 1

    def scheduler_step(self):
        self.sched_steps += 1
        self.lr = self.base_lr * self.decay ** self.sched_steps
