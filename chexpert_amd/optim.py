"""Fused optimisers over the engine's flat fp32 parameter / gradient buffers (one kernel per step).

Same update rules and defaults as the torch.optim classes the reference wires up
(/root/reference/chexpert.py:470 Adam(lr); :479 SGD(momentum=0.9, nesterov=True); :499
RMSprop(momentum=0.9, eps=1e-3)), with the schedulers of :480 (MultiStepLR[40000, 60000]) and :500
(ExponentialLR(gamma)) folded in as `scheduler_step()`.

Beside them, for large global batches, the layer-wise trust-ratio rules the reference does not have: `FusedLAMB` (on Adam's moments)
and `FusedLARS` (on SGD with Nesterov momentum), stated in float64 as `reference_trust_step`.

Around any of them, `FusedSAM`: sharpness-aware minimisation (SAM / ASAM), two forward/backward passes per step, its ascent step
stated in float64 as `reference_sam_step`.
"""
import contextlib
import math

import torch

from . import ops

MAX_GROUPS = 256


def item_table(numels, group_of, vec4=None):
    """The work items of the grouped kernels (csrc/optim.hip) for tensors of `numels` floats laid out as `_fused.flatten`
    lays them out (each at a multiple of 4 floats, zero-padded to one), tensor k in group group_of[k]: a list of
    (start4, len4, group, tensor) in 16-byte units.  Every tensor, padding included, is cut into consecutive items of at most
    `vec4` units (default: the library's constant); items come in buffer order and none crosses a tensor.  A function of the
    shapes and the group assignment alone."""
    V = int(ops.optim_item_vec4() if vec4 is None else vec4)
    if V < 1:
        raise ValueError("an item holds at least one 16-byte unit")
    items, at = [], 0
    for k, (n, grp) in enumerate(zip(numels, group_of)):
        left = (int(n) + 3) // 4
        while left > 0:
            take = min(left, V)
            items.append((at, take, int(grp), k))
            at += take
            left -= take
    return items


def reference_step(kind, p, g, state, lr, t, lr_mult=1.0, weight_decay=0.0, frozen=False, t0=0, decoupled=False,
                   betas=(0.9, 0.999), eps=None, momentum=0.9, alpha=0.99):
    """float64 restatement of one grouped step for the tensors of ONE group (what cx_*_step_items computes per element, and what
    torch.optim.Adam / AdamW / SGD(nesterov) / RMSprop compute for a param_group): returns the new p, updates `state` (a list of
    two tensors shaped like p, zeros before the first step) in place.  t is the 1-based number of the minibatch, t0 the number of
    minibatches the group sat out before its first step (torch keeps one step count per parameter and starts it when the
    parameter first has a gradient): Adam's bias corrections use t - t0.  frozen: nothing changes.
    decoupled: p <- p * (1 - lr_g * wd) first, then the rule without decay (AdamW's order); else g <- g + wd * p."""
    if frozen:
        return p
    p, g = p.double(), g.double()
    lr_g = float(lr) * float(lr_mult)
    if decoupled:
        p = p * (1.0 - lr_g * weight_decay)
    elif weight_decay != 0:
        g = g + weight_decay * p
    if kind == "adam":
        tg = t - t0
        e = 1e-8 if eps is None else eps
        state[0] = betas[0] * state[0] + (1 - betas[0]) * g
        state[1] = betas[1] * state[1] + (1 - betas[1]) * g * g
        return p - lr_g / (1 - betas[0] ** tg) * (state[0] / (state[1].sqrt() / math.sqrt(1 - betas[1] ** tg) + e))
    if kind == "sgd_nesterov":
        state[0] = momentum * state[0] + g                  # zeros before the group's first step: the buffer starts as g
        return p - lr_g * (g + momentum * state[0])
    if kind == "rmsprop":
        e = 1e-3 if eps is None else eps
        state[0] = alpha * state[0] + (1 - alpha) * g * g
        state[1] = momentum * state[1] + g / (state[0].sqrt() + e)
        return p - lr_g * state[1]
    raise ValueError("unknown optimiser kind %r" % (kind,))


def tensor_items(items, n_tensors):
    """The first item of every tensor in an `item_table`, then the number of items: T + 1 entries (what cx_lamb_step_items and
    cx_lars_step_items take as `tensor_items`).  Items come in buffer order and none crosses a tensor, so tensor k owns the items
    [out[k], out[k + 1]); a tensor without elements owns none."""
    out, at = [], 0
    for k in range(int(n_tensors)):
        out.append(at)
        while at < len(items) and items[at][3] == k:
            at += 1
    if at != len(items):
        raise ValueError("the items are not in tensor order, or name a tensor >= %d" % n_tensors)
    return out + [at]


def reference_trust_step(kind, tensors, grads, states, lr, t, group_rows, group_of, grad_scale=1.0, clip_coef=1.0, betas=(0.9, 0.999),
                         eps=None, momentum=0.9, trust_coef=0.001, always_adapt=False, trust_clip=False):
    """float64 statement of one LAMB / LARS step (what cx_lamb_step_items / cx_lars_step_items compute) over a LIST of tensors,
    because the rule is per tensor: tensor k is in group group_of[k] with the row group_rows[j] = {lr_mult, weight_decay, frozen, t0}
    (a sequence of four, or a dict with those keys).  t is the 1-based number of the minibatch.  Returns (new tensors, ratios) with
    ratios[k] = (r, |p|, |u|, adapted) (LARS: |g| for |u|); `states[k]` (two float64 tensors shaped like tensor k, zeros before the
    first step: m and v, or buf and an unused one) is updated in place.  A frozen group writes nothing (r = 1, norms 0).

      lamb   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  u = (m / (1 - b1^tg)) / (sqrt(v / (1 - b2^tg)) + eps) + wd p
             r = |p| / |u|;  p <- p - lr_g r u                                            (timm's Lamb, apex's FusedLAMB)
      lars   r = coef |p| / (|g| + wd |p| + eps);  g' = r (g + wd p);  buf = momentum buf + g';  p <- p - lr_g (g' + momentum buf)
                                                                                          (timm's Lars with nesterov=True)

    with g = grad_scale * clip_coef * grad, lr_g = lr * lr_mult, tg = t - t0.  r is 1 unless the tensor is adapted (its group has
    wd != 0, or always_adapt) and both norms are > 0; trust_clip: r = min(r, 1)."""
    if kind not in ("lamb", "lars"):
        raise ValueError("unknown trust-ratio optimiser kind %r" % (kind,))
    e = (1e-6 if kind == "lamb" else 1e-8) if eps is None else float(eps)
    out, ratios = [], []
    for k, (p, grad) in enumerate(zip(tensors, grads)):
        row = group_rows[group_of[k]]
        if isinstance(row, dict):
            row = [row.get("lr_mult", 1.0), row.get("weight_decay", 0.0), row.get("frozen", False), row.get("t0", 0)]
        lr_mult, wd, frozen, t0 = float(row[0]), float(row[1]), bool(row[2]), row[3]
        if frozen:
            out.append(p)
            ratios.append((1.0, 0.0, 0.0, False))
            continue
        p = p.double()
        g = float(grad_scale) * float(clip_coef) * grad.double()
        lr_g, tg = float(lr) * lr_mult, t - t0
        adapted = wd != 0 or bool(always_adapt)
        wn = float(p.pow(2).sum().sqrt())
        if kind == "lamb":
            states[k][0] = betas[0] * states[k][0] + (1 - betas[0]) * g
            states[k][1] = betas[1] * states[k][1] + (1 - betas[1]) * g * g
            u = (states[k][0] / (1 - betas[0] ** tg)) / ((states[k][1] / (1 - betas[1] ** tg)).sqrt() + e) + wd * p
            un = float(u.pow(2).sum().sqrt())
            r = wn / un if adapted and wn > 0 and un > 0 else 1.0
            if trust_clip:
                r = min(r, 1.0)
            out.append(p - lr_g * r * u)
        else:
            un = float(g.pow(2).sum().sqrt())
            r = trust_coef * wn / (un + wd * wn + e) if adapted and wn > 0 and un > 0 else 1.0
            if trust_clip:
                r = min(r, 1.0)
            g2 = r * (g + wd * p)
            states[k][0] = momentum * states[k][0] + g2
            out.append(p - lr_g * (g2 + momentum * states[k][0]))
        ratios.append((r, wn, un, adapted))
    return out, ratios


def reference_sam_step(tensors, grads, group_rows, group_of, rho, adaptive=False, eps=1e-12, grad_scale=1.0):
    """float64 statement of the ascent step of sharpness-aware minimisation (what cx_sam_norm_items + cx_sam_perturb_items compute)
    over a LIST of tensors: tensor k is in group group_of[k] with the row group_rows[j] = {lr_mult, weight_decay, frozen, t0} (a
    sequence of four, or a dict with those keys), of which only `frozen` is read.  With g = grad_scale * grad and s = 1 (SAM, Foret et
    al.) or s = |p| elementwise (ASAM, Kwon et al.):

      norm = sqrt(sum over the unfrozen tensors of (s g)^2);  p <- p + rho / (norm + eps) * s^2 g

    Returns (perturbed tensors, norm).  A tensor of a frozen group is returned as it came and is absent from the norm."""
    def frozen(k):
        row = group_rows[group_of[k]]
        return bool(row.get("frozen", False)) if isinstance(row, dict) else bool(row[2])
    live = [k for k in range(len(tensors)) if not frozen(k)]
    sg = {}
    for k in live:
        p, g = tensors[k].double(), float(grad_scale) * grads[k].double()
        sg[k] = (p, g, p.abs() if adaptive else torch.ones_like(p))
    norm = math.sqrt(sum(float((s * g).pow(2).sum()) for _, g, s in sg.values()))
    scale = float(rho) / (norm + float(eps))
    out = [sg[k][0] + scale * sg[k][2].pow(2) * sg[k][1] if k in sg else tensors[k] for k in range(len(tensors))]
    return out, norm


def finetune_groups(model, weight_decay=0.0, no_decay_norm_bias=False, head_lr_mult=1.0, backbone_lr_mult=1.0, freeze_backbone=False):
    """The `groups` list of a fine-tuning run: the head (the last nn.Linear in named_modules() order: `classifier` of DenseNet, `fc`
    of ResNet, the final layer of EfficientNet's head; GeM's exponent `pool_p` of FusedNet.set_pool goes with it) against
    everything else, each split once more when no_decay_norm_bias exempts every 1-D parameter (BatchNorm weights and biases, all
    biases, `pool_p`) from weight decay.  Dicts carry a "name": "backbone",
    "backbone_no_decay", "head", "head_no_decay"; an empty group is left out."""
    head = None
    for _, mod in model.named_modules():
        if isinstance(mod, torch.nn.Linear):
            head = mod
    if head is None:
        raise ValueError("finetune_groups: the model has no nn.Linear to call its head")
    head_ids = {id(q) for q in head.parameters()}
    if getattr(model, "pool_p", None) is not None:          # GeM's exponent (set_pool) belongs to the head; 1-D: no decay
        head_ids.add(id(model.pool_p))
    parts = {"backbone": [], "backbone_no_decay": [], "head": [], "head_no_decay": []}
    for q in model.parameters():
        key = "head" if id(q) in head_ids else "backbone"
        if no_decay_norm_bias and q.dim() <= 1:
            key += "_no_decay"
        parts[key].append(q)
    out = []
    for key, params in parts.items():
        if params:
            is_head = key.startswith("head")
            out.append({"name": key, "params": params, "lr_mult": float(head_lr_mult if is_head else backbone_lr_mult),
                        "weight_decay": 0.0 if key.endswith("_no_decay") else float(weight_decay),
                        "frozen": bool(freeze_backbone) and not is_head})
    return out


class _Flat:
    """Options shared by the three optimisers (all off by default: `step()` / `step_dev()` then launch the plain one-kernel update):

      max_grad_norm   clip the gradient to this global L2 norm (torch.nn.utils.clip_grad_norm_'s rule), on the device
      skip_nonfinite  drop the whole update of a step whose gradient norm is inf or NaN (no parameter, state or EMA element written)
      ema_decay       keep an exponential moving average of the parameters, written by the optimiser kernel itself
      ema_warmup      decay = min(ema_decay, (1 + t) / (10 + t)) at step t, so the average forgets its start quickly

    With any of them on the step is `cx_grad_norm` (when clipping or skipping) + the `_ex` update.  The scheduler and Adam's bias
    correction count minibatches, skipped ones included.

    Parameter groups (`groups`, `decoupled`; both off by default, and then nothing here runs):

      groups      list of {"params": iterable of the model's Parameters, "lr_mult": 1.0, "weight_decay": <the constructor's>,
                  "frozen": False, "name": optional}.  Dict j is group j + 1; parameters named in no dict form group 0 (the
                  constructor's weight_decay, lr_mult 1).  A frozen group is skipped by the kernels: no byte of its parameters,
                  states or EMA is written, and its gradient counts neither for the clip norm nor as non-finite.
      decoupled   weight decay as p <- p * (1 - lr_g * wd_g) ahead of the rule (AdamW's order) instead of g += wd_g * p

    The step is then `cx_grad_norm_items` (when clipping or skipping) + `cx_*_step_items`, walking a per-tensor item table and
    the group rows {lr_mult, weight_decay, frozen, t0} in device memory (`set_group` rewrites a row, between graph replays too)."""
    NSTATE = 0
    PASSES = 1                      # forward/backward passes of one train_step (FusedSAM: 2)
    KIND = None
    SCHED = (0, 1.0, (0, 0))        # (kind, gamma, milestones): 0 none, 1 ExponentialLR, 2 MultiStepLR
    # what the host-lr entry point of each family takes beside the rule's own arguments, by the family's suffix
    HOST_ARGS = {"": ("lr",), "_ex": ("lr", "step"), "_items": ("lr", "step")}

    def __init__(self, model, lr, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=True, weight_decay=0.0,
                 decoupled=False, groups=None):
        self.model = model
        if hasattr(model, "set_pool"):                      # the parameter list is this optimiser's from here on (FusedNet.set_pool)
            model._pool_locked = True
        self.lr = float(lr)
        self.base_lr = float(lr)
        self.wd = float(weight_decay)                       # the ungrouped steps' decay; with groups: group 0's row
        self.step_count = 0
        self.sched_steps = 0
        self._state = self._pending_state = self._hyper = None
        self._sched = self.SCHED
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
        self.decoupled = bool(decoupled)
        self._grouped = groups is not None or self.decoupled
        self._items = self._gtab = self._gpart = self._gsq = self._gnorm = None
        if self._grouped:
            self._init_groups(groups or [], self.wd)

    # ---- parameter groups
    def _init_groups(self, groups, weight_decay):
        named = list(self.model.named_parameters())
        name_of = {id(q): n for n, q in named}
        if 1 + len(groups) > MAX_GROUPS:
            raise ValueError("at most %d parameter groups (got %d dicts + the default group)" % (MAX_GROUPS, len(groups)))
        self._group_of = {}                                 # id(parameter) -> group
        self.group_names = ["default"]
        self._grows = [[1.0, weight_decay, 0.0, 0.0]]       # {lr_mult, weight_decay, frozen, t0}, the host copy of the device table
        for j, d in enumerate(groups):
            extra = set(d) - {"params", "lr_mult", "weight_decay", "frozen", "name"}
            if "params" not in d or extra:
                raise ValueError("group %d: a dict with 'params' and optionally lr_mult, weight_decay, frozen, name (got %s)" % (j, sorted(d)))
            lr_mult, wd = float(d.get("lr_mult", 1.0)), float(d.get("weight_decay", weight_decay))
            if not (math.isfinite(lr_mult) and lr_mult >= 0.0):
                raise ValueError("group %d: lr_mult must be finite and >= 0 (got %r)" % (j, d.get("lr_mult")))
            if not math.isfinite(wd):
                raise ValueError("group %d: weight_decay must be finite (got %r)" % (j, d.get("weight_decay")))
            for q in d["params"]:
                if id(q) not in name_of:
                    raise ValueError("group %d names a parameter that is not the model's" % j)
                if id(q) in self._group_of:
                    raise ValueError("parameter %s appears twice in the groups" % name_of[id(q)])
                self._group_of[id(q)] = j + 1
            self.group_names.append(str(d.get("name", "group%d" % (j + 1))))
            self._grows.append([lr_mult, wd, 1.0 if d.get("frozen", False) else 0.0, 0.0])
        self._gparams = [[] for _ in self._grows]           # parameter names of each group, in the model's order
        for n, q in named:
            self._gparams[self._group_of.get(id(q), 0)].append(n)
        self._frozen_at = [0] * len(self._grows)            # steps done when the group was frozen

    def _group_bufs(self, eng):
        dev = eng.flat.device
        if self._items is not None and self._items.device == dev and self._gnumel == eng.flat.numel():
            return
        if len(eng.params) != sum(len(v) for v in self._gparams):
            raise RuntimeError("the engine holds %d parameters, the groups were built over %d" % (len(eng.params), sum(len(v) for v in self._gparams)))
        items = item_table([q.numel() for q in eng.params], [self._group_of.get(id(q), 0) for q in eng.params])
        # the kernels trust the table: check it against the buffer it will walk
        tensor_start = {}
        for it in items:
            tensor_start.setdefault(it[3], it[0])
        if any(4 * tensor_start[k] != off for k, off in enumerate(eng.offsets)) or \
                (items and 4 * (items[-1][0] + items[-1][1]) != eng.flat.numel()) or (not items and eng.flat.numel()):
            raise RuntimeError("the item table does not match the layout of the flat parameter buffer")
        self._items = torch.tensor(items, dtype=torch.int32).reshape(-1, 4).to(dev)
        self._gtab = torch.tensor(self._grows, dtype=torch.float32).to(dev)
        self._gpart = torch.zeros(max(1, len(items)), dtype=torch.float32, device=dev)
        self._gsq = torch.zeros(len(self._grows), dtype=torch.float32, device=dev)
        self._gnorm = torch.zeros(len(self._grows), dtype=torch.float32, device=dev)
        self._gnumel = eng.flat.numel()

    def set_group(self, i, lr_mult=None, weight_decay=None, frozen=None):
        """Rewrites row i of the group table (None: keep) with one small host-to-device copy on the current stream, so the next
        step -- a replay of a captured one included -- sees it.  Freezing notes the steps done; thawing adds the steps the group
        sat out to its t0 (for a group frozen from the start: t0 = the steps done), so that Adam's bias corrections count the
        group's own steps, as torch does for a parameter whose gradient was None until then.  Thawing reads the device step count
        (`sync_from_device`: synchronises)."""
        if not self._grouped:
            raise RuntimeError("set_group() needs an optimiser built with groups (or decoupled=True)")
        row = self._grows[i]
        if lr_mult is not None:
            if not (math.isfinite(float(lr_mult)) and float(lr_mult) >= 0.0):
                raise ValueError("lr_mult must be finite and >= 0 (got %r)" % (lr_mult,))
            row[0] = float(lr_mult)
        if weight_decay is not None:
            if not math.isfinite(float(weight_decay)):
                raise ValueError("weight_decay must be finite (got %r)" % (weight_decay,))
            row[1] = float(weight_decay)
        if frozen is not None and bool(frozen) != (row[2] != 0.0):
            self.sync_from_device()
            if frozen:
                self._frozen_at[i] = self.step_count
            else:
                row[3] += float(self.step_count - self._frozen_at[i])
            row[2] = 1.0 if frozen else 0.0
        if self._gtab is not None:
            self._gtab[i].copy_(torch.tensor(row, dtype=torch.float32))

    def group_grad_norms(self):
        """L2 norm of the (unscaled) gradient of every group at the most recent step, frozen groups included.  Reads the device:
        synchronises."""
        if not self._grouped:
            raise RuntimeError("group_grad_norms() needs an optimiser built with groups")
        self._clip_host()
        return [0.0] * len(self._grows) if self._gnorm is None else [float(v) for v in self._gnorm.cpu()]

    # ---- the step
    def _step(self, grad_scale, dev):
        """One step through the family the options select: grouped -> `_items`, clip / skip / EMA on -> `_ex`, else the plain entry
        point; `dev`: the learning rate and the step count are the device's (`hyper()`), else the host's.  The norm goes first when
        clipping or skipping is on."""
        p, g, st = self._bufs(self.NSTATE)
        family = "_items" if self._grouped else "_ex" if self._ex_on() else ""
        args = {"grad_scale": grad_scale}
        if self._grouped:
            args.update(items=self._items, groups=self._gtab, decoupled=self.decoupled)
        else:
            args.update(weight_decay=self.wd)
        if family:
            if self._grouped and self._norm_on():
                ops.grad_norm_items(g, self._items, self._gtab, self._gpart, self._gsq, self._gnorm, self._clip, grad_scale,
                                    self.max_grad_norm or 0.0, self.skip_nonfinite)
            elif self._norm_on():
                ops.grad_norm(g, self._ws, self._clip, grad_scale, self.max_grad_norm or 0.0, self.skip_nonfinite)
            args.update(clip=self._clip if self._norm_on() else None, ema=self._ema, ema_decay=self.ema_decay or 0.0,
                        ema_warmup=self.ema_warmup, skip_nonfinite=self.skip_nonfinite)
        if dev:
            args.update(hyper=self.hyper())
        else:
            host = {"lr": self.lr, "first_step": self.step_count == 0, "step": self.step_count + 1}
            args.update({k: host[k] for k in self.HOST_ARGS[family]})
        name = self.KIND + ("_step_dev" if dev and not self._grouped else "_step") + family
        getattr(ops, name)(p, g, *st, **self._rule(), **args)
        if not dev:                                         # (the device's count is cx_optim_tick's: `tick()`)
            self.step_count += 1

    def step(self, grad_scale=1.0):
        self._step(grad_scale, False)

    def step_dev(self, grad_scale=1.0):
        self._step(grad_scale, True)

    def train_step(self, model, x, target, dev=False):
        """One training step on the minibatch (chexpert.py:159-164), the statement of it that the command line and the captured
        steps of graph.py share; returns (loss, logits) of the forward pass.  zero_grad, forward_backward, then step() or, `dev`
        (learning rate, step count and scheduler in device memory), step_dev(), tick() and the engine's packed weights marked
        stale: the device-side update leaves the tensor versions as they were.  The host-side scheduler_step() stays with the
        caller, who knows the warm-up and the global step."""
        if model is not self.model:
            raise RuntimeError("train_step: the model is not the one the optimiser was built over")
        self.zero_grad()
        loss, logits = model.forward_backward(x, target)
        if dev:
            self.step_dev()
            self.tick()
            model._eng().packed_version = None
        else:
            self.step()
        return loss, logits

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
            pend, self._pending_state = self._pending_state, None
            if pend is not None:
                for dst, src in zip(self._state, pend):
                    dst.copy_(src)
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
        if self._grouped:
            self._group_bufs(eng)
        return eng.flat, eng.flat_grad, self._state

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
    def hyper(self, warmup_steps=0):
        """float[8] on the device: {lr, steps_done, sched_kind, gamma, lr_warmup_steps, milestone0, milestone1, base_lr}
        (include/chexpert_hip.h, cx_optim_tick).  Created from the host-side state on first use; from then on the device
        copy is the truth for `step_dev()` / `tick()` and `sync_from_device()` reads it back."""
        if self._hyper is None:
            kind, gamma, ms = self._sched
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
        if self._grouped:
            sd["groups"] = {"rows": [list(r) for r in self._grows], "decoupled": self.decoupled, "names": list(self.group_names),
                            "params": [list(v) for v in self._gparams], "frozen_at": list(self._frozen_at)}
        return sd

    def load_state_dict(self, sd):
        if sd.get("kind") != type(self).__name__:
            raise RuntimeError("optimizer checkpoint was written by %s, this is %s" % (sd.get("kind"), type(self).__name__))
        if "groups" in sd:                             # (a checkpoint written without groups leaves them as constructed)
            self._load_groups(sd["groups"])
        self.lr, self.base_lr, self.step_count, self.sched_steps = sd["lr"], sd["base_lr"], sd["step_count"], sd["sched_steps"]
        self._pending_state = sd["state"]              # copied into the flat-buffer state once the engine is bound
        self._hyper = None
        if "max_grad_norm" in sd:                      # (a checkpoint written without these options leaves them as constructed)
            self.max_grad_norm, self.skip_nonfinite = sd["max_grad_norm"], bool(sd["skip_nonfinite"])
            self.ema_decay, self.ema_warmup = sd["ema_decay"], bool(sd["ema_warmup"])
            self._pending_ex = {"skipped": int(sd.get("skipped", 0)), "ema": sd.get("ema")}
            self._ws = self._clip = self._ema = None

    def _load_groups(self, gs):
        if not self._grouped:
            raise RuntimeError("the optimizer checkpoint was written with parameter groups: build the optimiser with the same groups "
                               "(decoupled=%r) before loading it" % bool(gs["decoupled"]))
        mine = {n: k for k, names in enumerate(self._gparams) for n in names}
        theirs = {n: k for k, names in enumerate(gs["params"]) for n in names}
        for n, k in mine.items():
            if theirs.get(n) != k:
                raise RuntimeError("the optimizer checkpoint partitions the parameters differently: %s is in group %s there, in group "
                                   "%d here" % (n, theirs.get(n, "none"), k))
        for n in theirs:
            if n not in mine:
                raise RuntimeError("the optimizer checkpoint partitions the parameters differently: %s is not a parameter here" % n)
        if len(gs["rows"]) != len(self._grows):
            raise RuntimeError("the optimizer checkpoint has %d parameter groups, this optimiser %d" % (len(gs["rows"]), len(self._grows)))
        if bool(gs["decoupled"]) != self.decoupled:
            raise RuntimeError("the optimizer checkpoint was written with decoupled=%r, this optimiser has decoupled=%r"
                               % (bool(gs["decoupled"]), self.decoupled))
        self._grows = [[float(v) for v in r] for r in gs["rows"]]
        self._frozen_at = [int(v) for v in gs.get("frozen_at", [0] * len(self._grows))]
        if self._gtab is not None:
            self._gtab.copy_(torch.tensor(self._grows, dtype=torch.float32))

    def sync_from_device(self):
        if self._hyper is not None:
            h = self._hyper.cpu()
            self.lr, self.step_count = float(h[0]), int(h[1])
            # cx_optim_tick steps the scheduler inside the graph: after minibatch number `step` it has been stepped
            # step - max(warm-up, 1) + 1 times (chexpert.py:157-165), which is what an eager resume continues from
            if int(h[2]) != 0:
                self.sched_steps = max(0, int(h[1]) - max(int(h[4]), 1) + 1)


class FusedAdam(_Flat):
    NSTATE = 2
    KIND = "adam"
    HOST_ARGS = dict(_Flat.HOST_ARGS, **{"": ("lr", "step")})              # the host's powf makes the bias corrections

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, groups=None, **options):
        super().__init__(model, lr, weight_decay=weight_decay, decoupled=decoupled, groups=groups, **options)
        self.betas, self.eps = betas, eps

    def _rule(self):
        return {"beta1": self.betas[0], "beta2": self.betas[1], "eps": self.eps}


class FusedSGDNesterov(_Flat):
    NSTATE = 1
    KIND = "sgd_nesterov"
    # on its first step the momentum buffer becomes the gradient (the grouped kernels start from a zeroed buffer instead)
    HOST_ARGS = dict(_Flat.HOST_ARGS, **{"": ("lr", "first_step"), "_ex": ("lr", "first_step", "step")})

    def __init__(self, model, lr, momentum=0.9, weight_decay=0.0, milestones=(40000, 60000), gamma=0.1, decoupled=False, groups=None,
                 **options):
        super().__init__(model, lr, weight_decay=weight_decay, decoupled=decoupled, groups=groups, **options)
        self.momentum, self.milestones, self.gamma = momentum, tuple(milestones), gamma
        ms = (tuple(milestones) + (1 << 30, 1 << 30))[:2]
        self._sched = (2, gamma, ms)

    def _rule(self):
        return {"momentum": self.momentum}

    def scheduler_step(self):
        self.sched_steps += 1
        self.lr = self.base_lr * self.gamma ** sum(self.sched_steps >= m for m in self.milestones)


class _Trust:
    """What FusedLAMB and FusedLARS share: the layer-wise trust ratio r_k = |p_k| / |update_k| of every parameter tensor, computed
    on the device inside the step (csrc/optim.hip: per-item partial sums, one workgroup that adds them per tensor, the update).
    Both always take the grouped path (`groups=None`: one default group) and refuse `decoupled`.  A tensor is adapted when its
    group's weight decay is not 0, or when `always_adapt` is set (timm's rule): with finetune_groups(no_decay_norm_bias=True)
    BatchNorm weights, biases and `pool_p` get neither decay nor adaptation.  `trust_clip`: r = min(r, 1)."""
    USCRATCH = False                # LAMB: n floats that hold the update between the norm and the apply

    def _init_trust(self, coef, eps, trust_clip, always_adapt):
        if not (math.isfinite(float(coef)) and float(coef) > 0.0):
            raise ValueError("trust_coef must be finite and > 0 (got %r)" % (coef,))
        self.trust_coef, self.trust_eps = float(coef), float(eps)
        self.trust_clip, self.always_adapt = bool(trust_clip), bool(always_adapt)
        self._titems = self._tpart = self._trust = self._u = None

    @staticmethod
    def _refuse_decoupled(decoupled, why):
        if decoupled:
            raise ValueError("decoupled=True is refused: " + why)

    def _bufs(self, n):
        out = super()._bufs(self.NSTATE)
        eng = self.model._eng()
        dev, numel = eng.flat.device, eng.flat.numel()
        if self._titems is None or self._titems.device != dev or self._tnumel != numel:
            # beside the states: nothing is allocated while a graph is being captured.  Not state: every step rewrites them
            T = len(eng.params)
            starts = tensor_items(self._items.cpu().tolist(), T)
            self._titems = torch.tensor(starts, dtype=torch.int32).to(dev)
            self._tpart = (torch.zeros(max(1, self._items.shape[0]), dtype=torch.float32, device=dev),
                           torch.zeros(max(1, self._items.shape[0]), dtype=torch.float32, device=dev))
            self._trust = torch.zeros(max(1, T), 4, dtype=torch.float32, device=dev)
            self._trust[:, 0] = 1.0
            self._u = torch.zeros_like(eng.flat) if self.USCRATCH else None
            self._tnumel = numel
        return out

    def _trust_args(self):
        return {"tensor_items": self._titems, "partials": self._tpart, "trust": self._trust, "trust_clip": self.trust_clip,
                "always_adapt": self.always_adapt}

    def trust_ratios(self):
        """{parameter name: (r, |p|, |u|)} of the most recent step that was not skipped (LARS: |g|, the scaled gradient's norm, for
        |u|); r = 1 for a tensor that is not adapted or belongs to a frozen group.  Reads the device: synchronises."""
        if self._trust is None:
            return {}
        name_of = {id(q): n for n, q in self.model.named_parameters()}
        rows = self._trust.cpu().tolist()
        return {name_of[id(q)]: tuple(rows[k][:3]) for k, q in enumerate(self.model._eng().params)}

    def adapted_ratios(self):
        """The ratios of the adapted tensors of the most recent step, as a list.  Reads the device: synchronises."""
        return [] if self._trust is None else [r[0] for r in self._trust.cpu().tolist() if r[3] != 0.0]

    def state_dict(self):
        sd = super().state_dict()
        sd["trust"] = {"coef": self.trust_coef, "eps": self.trust_eps, "trust_clip": self.trust_clip, "always_adapt": self.always_adapt}
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        tr = sd.get("trust")
        if tr is not None:
            self._set_trust(tr)

    def _set_trust(self, tr):
        self.trust_coef, self.trust_eps = float(tr["coef"]), float(tr["eps"])
        self.trust_clip, self.always_adapt = bool(tr["trust_clip"]), bool(tr["always_adapt"])


class FusedLAMB(_Trust, _Flat):
    """LAMB (You et al., ICLR 2020) in the bias-corrected form of timm's `Lamb` and apex's `FusedLAMB`: Adam's moments, the weight
    decay added to the update outside them, the update of every tensor rescaled to lr * |p| (reference_trust_step).  `eps` is Adam's
    (the ratio itself has none)."""
    NSTATE = 2
    KIND = "lamb"
    USCRATCH = True

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, always_adapt=False, trust_clip=False, groups=None,
                 decoupled=False, **options):
        self._refuse_decoupled(decoupled, "LAMB's weight decay already sits outside the moments")
        if not float(eps) > 0.0:
            raise ValueError("eps must be > 0 (got %r): it keeps the update of the zero padding at 0" % (eps,))
        super().__init__(model, lr, weight_decay=weight_decay, groups=groups or [], **options)
        self.betas, self.eps = betas, float(eps)
        self._init_trust(1.0, eps, trust_clip, always_adapt)

    def _rule(self):
        return dict(self._trust_args(), beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, u=self._u)

    def _set_trust(self, tr):
        super()._set_trust(tr)
        self.eps = self.trust_eps


class FusedLARS(_Trust, FusedSGDNesterov):
    """LARS (You, Gitman, Ginsburg 2017) on SGD with Nesterov momentum, timm's `Lars` with nesterov=True (without its
    trust_clip / lr quirk): r = trust_coef |p| / (|g| + wd |p| + eps) scales the decayed gradient ahead of the momentum
    (reference_trust_step).  Keeps FusedSGDNesterov's MultiStepLR."""
    KIND = "lars"

    def __init__(self, model, lr, momentum=0.9, weight_decay=0.0, trust_coef=0.001, eps=1e-8, always_adapt=False, trust_clip=False,
                 milestones=(40000, 60000), gamma=0.1, groups=None, decoupled=False, **options):
        self._refuse_decoupled(decoupled, "LARS's weight decay is part of the trust ratio")
        if not float(eps) >= 0.0:
            raise ValueError("eps must be >= 0 (got %r)" % (eps,))
        self._init_trust(trust_coef, eps, trust_clip, always_adapt)
        super().__init__(model, lr, momentum=momentum, weight_decay=weight_decay, milestones=milestones, gamma=gamma, groups=groups or [],
                         **options)

    def _rule(self):
        return dict(self._trust_args(), momentum=self.momentum, coef=self.trust_coef, eps=self.trust_eps)


class FusedRMSprop(_Flat):
    NSTATE = 2
    KIND = "rmsprop"

    def __init__(self, model, lr, alpha=0.99, eps=1e-3, momentum=0.9, weight_decay=0.0, decay=0.97, decoupled=False, groups=None,
                 **options):
        super().__init__(model, lr, weight_decay=weight_decay, decoupled=decoupled, groups=groups, **options)
        self.alpha, self.eps, self.momentum, self.decay = alpha, eps, momentum, decay
        self._sched = (1, decay, (0, 0))

    def _rule(self):
        return {"alpha": self.alpha, "eps": self.eps, "momentum": self.momentum}

    def scheduler_step(self):
        self.sched_steps += 1
        self.lr = self.base_lr * self.decay ** self.sched_steps


class FusedSAM:
    """Sharpness-aware minimisation (Foret et al., ICLR 2021) and, with `adaptive`, its scale-invariant form ASAM (Kwon et al., ICML
    2021) around any fused optimiser `base` (Adam, SGDNesterov, RMSprop, LAMB, LARS; grouped or not).  One step is two
    forward/backward passes: the first gradient g gives the ascent step p + rho * s^2 g / |s g| (s = 1, or |p| elementwise;
    reference_sam_step), the gradient at the perturbed weights is what the base optimiser then applies to the restored weights.
    Three kernels on the flat buffers (csrc/optim.hip: cx_sam_norm_items, cx_sam_perturb_items, cx_sam_restore_items); rho lives in
    device memory (`set_rho`), so a captured step follows a schedule.  A grouped base shares its item table and group rows: frozen
    groups are neither perturbed nor counted in the norm, and `set_group` is honoured; an ungrouped base gets a table with every
    tensor in group 0.

    Decided semantics:
      - the base's clipping, non-finite skip and EMA act on the second pass's gradient;
      - a non-finite first gradient leaves the weights unperturbed (no byte written); the second pass then recomputes the same
        gradient and the base treats it as it always does;
      - the EMA never sees perturbed weights (the base's kernel writes it after the weights are restored);
      - the second pass computes with batch statistics but moves no BatchNorm running statistic and counts no batch;
      - Dropout and DropConnect draw fresh masks in the second pass (their device counter advances per forward), as in the usual
        SAM implementations;
      - the scheduler and Adam's step count advance once per SAM step;
      - refused: set_loss(kind="aucm") (its auxiliary update runs inside forward_backward and would run twice), an engine with a
        data-parallel reducer (the first pass would have to skip the all-reduce), a model in eval mode, SegmentedTrainStep.

    Every attribute and method this class does not define (grad_norm, skipped_steps, ema_weights, set_group, hyper, tick,
    sync_from_device, scheduler_step, trust_ratios, lr, ...) is the base's, for reading and for writing."""
    PASSES = 2                      # (on this class itself: __getattr__ would answer with the base's 1)
    _OWN = ("base", "rho", "adaptive", "eps", "_sam", "_rho_dev", "_backup", "_spart", "_sitems", "_sgtab", "_sitems_host", "_snumel")

    def __init__(self, base, rho=0.05, adaptive=False, eps=1e-12):
        if not isinstance(base, _Flat):
            raise TypeError("FusedSAM wraps a fused optimiser (FusedAdam, FusedSGDNesterov, FusedRMSprop, FusedLAMB, FusedLARS), got %s"
                            % type(base).__name__)
        if not (math.isfinite(float(rho)) and float(rho) >= 0.0):
            raise ValueError("rho must be finite and >= 0 (got %r)" % (rho,))
        if not (math.isfinite(float(eps)) and float(eps) > 0.0):
            raise ValueError("eps must be finite and > 0 (got %r): it keeps the perturbation of a zero gradient at 0" % (eps,))
        self.base = base
        self.rho, self.adaptive, self.eps = float(rho), bool(adaptive), float(eps)
        self._sam = self._rho_dev = self._backup = self._spart = self._sitems = self._sgtab = self._sitems_host = None
        self._snumel = -1

    def __getattr__(self, name):                            # (only for names this object does not hold)
        if name == "base":
            raise AttributeError(name)
        return getattr(self.base, name)

    def __setattr__(self, name, value):
        if name in self._OWN:
            object.__setattr__(self, name, value)
        else:
            setattr(self.base, name, value)

    # ---- buffers: beside the base's states, so that nothing is allocated while a graph is being captured
    def _bufs(self, n=None):
        base = self.base
        out = base._bufs(base.NSTATE)
        eng = base.model._eng()
        dev, numel = eng.flat.device, eng.flat.numel()
        if self._sam is None or self._sam.device != dev or self._snumel != numel:
            if base._grouped:
                self._sitems_host = base._items.cpu().contiguous()
            else:
                items = item_table([q.numel() for q in eng.params], [0] * len(eng.params))
                if (items and 4 * (items[-1][0] + items[-1][1]) != numel) or (not items and numel):
                    raise RuntimeError("the item table does not match the layout of the flat parameter buffer")
                self._sitems_host = torch.tensor(items, dtype=torch.int32).reshape(-1, 4)
                self._sitems = self._sitems_host.to(dev)
                self._sgtab = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float32).to(dev)
            self._backup = torch.zeros_like(eng.flat)
            self._spart = torch.zeros(max(1, self._sitems_host.shape[0]), dtype=torch.float32, device=dev)
            self._sam = torch.zeros(4, dtype=torch.float32, device=dev)
            self._rho_dev = torch.tensor([self.rho, self.eps], dtype=torch.float32).to(dev)
            self._snumel = numel
        return out

    def _tables(self):
        base = self.base
        return (base._items, base._gtab) if base._grouped else (self._sitems, self._sgtab)

    def _refuse(self):
        model = self.base.model
        if getattr(model, "loss_kind", None) == "aucm":
            raise RuntimeError("FusedSAM refuses set_loss(kind='aucm'): its auxiliary update runs inside forward_backward and would run "
                               "twice per step")
        if getattr(model._eng(), "reducer", None) is not None:
            raise RuntimeError("FusedSAM is not supported data-parallel: the first pass would have to skip the all-reduce "
                               "(DESIGN.md: leftovers of the SAM section)")

    # ---- the two halves of a step
    def first_step(self, dev=False, grad_scale=1.0):
        """The norm of the gradient in the flat gradient buffer and the ascent step: backup = p, p += rho * s^2 g / |s g| on the
        unfrozen groups.  Marks the engine's packed weights stale, as GraphedTrainStep.replay does.  (`dev` changes nothing here:
        rho is always the device's.)"""
        self._refuse()
        p, g, _ = self._bufs()
        items, gtab = self._tables()
        ops.sam_norm_items(p, g, items, gtab, self._rho_dev, self._spart, self._sam, grad_scale, self.adaptive, self._sitems_host)
        ops.sam_perturb_items(p, g, self._backup, items, gtab, self._sam, grad_scale, self.adaptive, self._sitems_host)
        self.base.model._eng().packed_version = None

    def second_step(self, dev=False, grad_scale=1.0):
        """p = backup (a copy: the weights come back with their own bits), packed weights stale, then the base's step() or, `dev`,
        step_dev() on the gradient now in the flat gradient buffer."""
        p, _, _ = self._bufs()
        items, gtab = self._tables()
        ops.sam_restore_items(p, self._backup, items, gtab, self._sam, self._sitems_host)
        self.base.model._eng().packed_version = None
        if dev:
            self.base.step_dev(grad_scale)
        else:
            self.base.step(grad_scale)

    def step(self, grad_scale=1.0):
        raise RuntimeError("FusedSAM needs two gradients per step: call train_step(model, x, target), or first_step() / second_step() "
                           "around a second forward_backward(..., track_stats=False)")

    step_dev = step

    def train_step(self, model, x, target, dev=False):
        """One SAM step on the minibatch; returns (loss, logits) of the first pass, at the unperturbed weights.  zero_grad,
        forward_backward, first_step, zero_grad, a second forward_backward that leaves the BatchNorm running statistics and the
        count of batches alone, second_step and, `dev`, the base's tick()."""
        if model is not self.base.model:
            raise RuntimeError("train_step: the model is not the one the base optimiser was built over")
        if not model.training:
            raise RuntimeError("FusedSAM needs the model in training mode (eval-mode SAM with frozen BatchNorm is not supported)")
        self._refuse()
        self.zero_grad()
        loss, logits = model.forward_backward(x, target)
        self.first_step(dev)
        self.zero_grad()
        model.forward_backward(x, target, track_stats=False)
        self.second_step(dev)
        if dev:
            self.base.tick()
        return loss, logits

    # ---- what the wrapper adds to the base's surface
    def perturbation_norm(self):
        """|s g| of the most recent first_step (the norm the ascent step was divided by).  Reads the device: synchronises."""
        return 0.0 if self._sam is None else float(self._sam.cpu()[0])

    def set_rho(self, rho):
        """One small host-to-device copy on the current stream, so the next step -- a replay of a captured one included -- sees it."""
        if not (math.isfinite(float(rho)) and float(rho) >= 0.0):
            raise ValueError("rho must be finite and >= 0 (got %r)" % (rho,))
        self.rho = float(rho)
        if self._rho_dev is not None:
            self._rho_dev.copy_(torch.tensor([self.rho, self.eps], dtype=torch.float32))

    def state_dict(self):
        """The base's state (a checkpoint of a SAM run restores into the bare base optimiser, and the reverse) plus the `sam` entry."""
        sd = self.base.state_dict()
        sd["sam"] = {"rho": self.rho, "adaptive": self.adaptive, "eps": self.eps}
        return sd

    def load_state_dict(self, sd):
        self.base.load_state_dict(sd)
        s = sd.get("sam")
        if s is not None:                              # (a checkpoint written without SAM leaves it as constructed)
            self.adaptive, self.eps = bool(s["adaptive"]), float(s["eps"])
            self.set_rho(s["rho"])
