"""Call trace of the DenseNet / ResNet / WideResNet / EfficientNet engines and of Grad-CAM on the CPU, without the library: the
functions of chexpert_amd.ops and the `lib` / `ptr` / `stream_ptr` / `check` names of the modules that use them are replaced by
recorders, so `eng.forward` / `eng.backward` run on CPU tensors and leave the list of calls they would have issued.  A host-side
refactor of an engine is right when this list is EQUAL before and after, for every configuration below.

The wrappers of ops named in REAL run for real (on the recorders' `lib`): what they log is the C call they make, so a tree whose
engine calls `lib.cx_*` itself and a tree that goes through those wrappers leave the same list.  The library stand-in knows the
names of `_lib.SIGNATURES` and no other, as the library does.

    python scratch/record_calls.py [TREE] [--dump DIR] [--rank-offsets]
    python scratch/record_calls.py [TREE] --time

TREE: the checkout to import chexpert_amd from (default: this one), so the script can be pointed at a checkout of another commit.
Prints one line per configuration: name, number of calls, sha256 of the list.  --dump writes each list to DIR/<name>.txt (diff them).
--rank-offsets logs a tensor's storage offset as its rank among the distinct offsets seen for that storage in that list, so a monotone
re-packing of a vector (slots dropped, the others in their order) leaves the list as it is; the offsets of `zero_` calls do not
count (a fill of a range of slots is what such a re-packing shortens or removes): they are ranked by the offsets below them.
--time runs no configuration: it prints the median host time of one DenseNet121 step (forward + backward under the recorders, 20
steps after 3) -- what the engine's Python costs per step, to compare two trees.

What a call logs: the function's name and its arguments; a tensor as (index of its storage by first appearance, storage offset,
shape, strides, dtype), anything else by repr.  Calls made directly on tensors are logged too when they write: `zero_`, `fill_`,
`copy_`, `add_` and `torch.add(..., out=)` (a TorchFunctionMode), and so are the reducer's `begin` / `ready(offset)` / `finish`.
Every recorder returns ROWS where the real function returns a statistic-row count."""
import bisect
import hashlib
import inspect
import os
import sys

import torch
from torch.overrides import TorchFunctionMode

ROWS = 7
SWITCHES = ("CHEXPERT_JOIN_FUSE", "CHEXPERT_FWD_JOIN_FUSE", "CHEXPERT_STREAM_LO", "CHEXPERT_PAIR_BWD")
# functions of ops that run for real: the helpers every wrapper uses, and the wrappers of the entry points the engines once called raw
REAL = {"_nhwc", "_fn", "_dense", "_f32", "_out_hw", "dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad", "gap_se_fwd", "scale_act_bc", "gap_affine_act",
        "se_bwd_fused", "se_act_bwd", "bn_lin_bwd_stats", "affine2_out", "scale_rows", "dropout_mask_dev", "counter_add", "mul_f32",
        "linear_fwd", "u8_to_nhwc8", "nchw3_to_nhwc8", "chan_map_table", "affine_to_f32_nchw", "gradcam_map", "cam_norm_upsample"}


class Trace:
    def __init__(self):
        self.calls, self.storages, self.keep = [], {}, []

    def describe(self, a):
        if isinstance(a, _Ptr):
            return ("ptr", self.describe(a.t))
        if isinstance(a, torch.Tensor):
            self.keep.append(a)                          # (alive to the end: no storage address is handed out twice)
            sid = self.storages.setdefault(a.untyped_storage().data_ptr(), len(self.storages))
            return ("T", sid, a.storage_offset(), tuple(a.shape), tuple(a.stride()), str(a.dtype))
        if isinstance(a, (list, tuple)):
            return tuple(self.describe(x) for x in a)
        if isinstance(a, dict):
            return tuple((k, self.describe(a[k])) for k in sorted(a))
        if a is None or isinstance(a, (bool, int, float, str)):
            return repr(a)
        return "<%s>" % type(a).__name__

    def log(self, name, args, kwargs):
        self.calls.append((name, self.describe(args), self.describe(kwargs)))

    def ranked(self):
        """The calls with every tensor's storage offset replaced by its rank (--rank-offsets)."""
        def walk(a, f):
            if isinstance(a, tuple):
                return f(a) if len(a) == 6 and a[0] == "T" else tuple(walk(x, f) for x in a)
            return a
        seen = {}
        walk(tuple(c for c in self.calls if c[0] != "torch.zero_"), lambda t: seen.setdefault(t[1], set()).add(t[2]))
        order = {sid: sorted(offs) for sid, offs in seen.items()}
        return walk(tuple(self.calls), lambda t: t[:2] + (bisect.bisect_left(order.get(t[1], ()), t[2]),) + t[3:])

    def lines(self):
        return [repr(c) for c in (self.ranked() if RANK else self.calls)]

    def digest(self):
        return hashlib.sha256("\n".join(self.lines()).encode()).hexdigest()[:16]


TRACE = Trace()


class _Ptr:
    def __init__(self, t):
        self.t = t


def _recorder(name, ret=ROWS, sig=None):
    """sig: the replaced function's signature -- its arguments are logged by parameter name with the defaults filled in, so that
    an argument left out and the same value written out are one call"""
    def f(*args, **kwargs):
        if sig is not None:
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            args, kwargs = (), dict(bound.arguments)
        TRACE.log(name, args, kwargs)
        return ret
    return f


class _Lib:
    def __init__(self, names):
        self._names = names

    def __getattr__(self, name):
        if name not in self._names:
            raise AttributeError(name)
        return _recorder("lib." + name, ROWS if name == "cx_last_stat_rows" else 0)


class _OnGpu(torch.Tensor):
    is_cuda = True


class _Reducer:
    begin, ready, finish = _recorder("reducer.begin"), _recorder("reducer.ready"), _recorder("reducer.finish")


class _TensorWrites(TorchFunctionMode):
    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name in ("zero_", "fill_", "copy_", "add_") or (name == "add" and "out" in kwargs):
            TRACE.log("torch." + name, args, kwargs)
        return func(*args, **kwargs)


def patch(pkg):
    ops = pkg.ops
    special = {"_wgrad_ws": (None, None, False), "wgrad_defer_begin": True, "kernel_hint": 0}
    for name, fn in list(vars(ops).items()):
        if callable(fn) and getattr(fn, "__module__", None) == ops.__name__ and not isinstance(fn, type) and name not in REAL:
            setattr(ops, name, _recorder("ops." + name, special.get(name, ROWS), inspect.signature(fn)))
    from chexpert_amd import _lib, gradcam
    from chexpert_amd.models import densenet, efficientnet, resnet
    the_lib = _Lib(set(_lib.SIGNATURES))
    stand_ins = dict(lib=lambda: the_lib, ptr=lambda t: None if t is None else _Ptr(t), stream_ptr=lambda: 0, check=lambda rc, what: None,
                     require_cuda=lambda *tensors: None)
    for mod in (ops, densenet, resnet, efficientnet):
        for name, f in stand_ins.items():
            if hasattr(mod, name):
                setattr(mod, name, f)
    if hasattr(gradcam, "L"):                  # (a tree whose Grad-CAM calls the library through its `_lib as L`)
        gradcam.L = type("L", (), {k: staticmethod(f) for k, f in stand_ins.items()})


def run(name, make, x, *, train=True, dx=False, reducer=False, fp32=False, env=None, steps=2, eval_first=False, hooked=False, cam=False,
        pool=None):
    global TRACE
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    TRACE = Trace()
    torch.manual_seed(0)
    model = make()
    if pool:
        model.set_pool(pool)
    if fp32:
        model.storage_dtype(torch.float32)
    model.train(train)
    eng = model._eng()
    if reducer:
        eng.reducer = _Reducer()
    with _TensorWrites():
        if eval_first:                         # a plain eval forward before the training steps (its workspace is the one they take)
            eng.release(eng.forward(x, False))
        if hooked:                             # Grad-CAM's hook protocol: the eval forward and the feature-map launches
            from chexpert_amd.gradcam import hooked_eval_forward
            with torch.no_grad():
                hooked_eval_forward(model, x)
            steps = 0
        if cam:                                # grad_cam itself (it insists on a GPU tensor: a CPU one that says it is)
            from chexpert_amd.gradcam import grad_cam
            grad_cam(model, x.as_subclass(_OnGpu))
            steps = 0
        for _ in range(steps):                 # the second step takes the pooled workspace and its backward buffers
            ws = eng.forward(x, train, record=True)
            dl = torch.ones(ws.logits.shape, dtype=torch.float32)
            eng.backward(ws, dl, dx=torch.empty(x.shape[0], 3, *x.shape[2:], dtype=torch.float32) if dx else None)
            eng.release(ws)
    print("%-28s %5d calls  %s" % (name, len(TRACE.calls), TRACE.digest()), flush=True)
    if DUMP:
        with open(os.path.join(DUMP, name + ".txt"), "w") as f:
            f.writelines(line + "\n" for line in TRACE.lines())


def main():
    from chexpert_amd.models import BasicBlock, Bottleneck, DenseNet, ResNet, WideResNet
    from chexpert_amd.models.efficientnet import construct_model
    x64, x32 = torch.randn(2, 3, 64, 64), torch.randn(2, 3, 32, 32)
    u8 = torch.randint(0, 255, (2, 1, 64, 64), dtype=torch.uint8)
    ap = lambda S: {"k": .2, "v": .1, "nh": 8, "relative": True, "input_dims": (S, S)}
    bott = lambda **kw: (lambda: ResNet(Bottleneck, [1, 6, 2, 1], num_classes=5, **kw))      # a stage of 6: fuse_fwd, keep_lo, EPI_JOIN
    basic = lambda **kw: (lambda: ResNet(BasicBlock, [2, 2, 1, 1], num_classes=5, **kw))
    wrn = lambda d=10, k=2, **kw: (lambda: WideResNet(BasicBlock, d, k, num_classes=5, **kw))
    eff = lambda: construct_model("efficientnet-b0", 5)
    run("bottleneck_det", bott(), x64)
    for sw in ("CHEXPERT_JOIN_FUSE", "CHEXPERT_FWD_JOIN_FUSE", "CHEXPERT_STREAM_LO"):
        run("bottleneck_%s0_det" % sw[9:].lower(), bott(), x64, env={sw: "0"})
    run("bottleneck_fp32_det", bott(), x64, fp32=True)
    run("bottleneck_frozen_det", bott(), x64, train=False)
    run("bottleneck_dx_det", bott(), x64, dx=True)
    run("bottleneck_u8_det", bott(), u8)
    run("bottleneck_reducer_det", bott(), x64, reducer=True)
    run("bottleneck_lse_det", bott(), x64, pool="lse")
    for tag, kw in (("grouped", dict(groups=4, width_per_group=16)), ("dilated", dict(replace_stride_with_dilation=[False, True, True])),
                    ("wide128", dict(width_per_group=128)), ("aa", dict(attn_params=ap(64)))):
        run("bottleneck_%s_det" % tag, bott(**kw), x64)
    run("bottleneck_aa_fp32_det", bott(attn_params=ap(64)), x64, fp32=True)
    run("bottleneck_aa_frozen_det", bott(attn_params=ap(64)), x64, train=False)
    for tag, mk, x in (("basic", basic(), x64), ("basic_aa", basic(attn_params=ap(64)), x64), ("wrn", wrn(), x32),
                       ("wrn16_4_aa", wrn(16, 4, attn_params=ap(32)), x32)):
        run(tag + "_det", mk, x)
        run(tag + "_dx_det", mk, x, dx=True)
        run(tag + "_reducer_det", mk, x, reducer=True)
    run("basic_fp32_det", basic(), x64, fp32=True)
    run("efficientnet_b0_det", eff, x64)
    run("efficientnet_b0_frozen_det", eff, x64, train=False)
    run("efficientnet_b0_dx_reducer_det", eff, x64, dx=True, reducer=True)
    run("efficientnet_b0_fp32_det", eff, x64, fp32=True)
    run("efficientnet_b0_u8_det", eff, u8)
    run("efficientnet_b0_fp32_after_eval_det", eff, x64, fp32=True, eval_first=True)
    run("efficientnet_b0_dx_det", eff, x64, dx=True)
    run("efficientnet_b0_gem_det", eff, x64, pool="gem")
    run("efficientnet_b1_det", lambda: construct_model("efficientnet-b1", 5), x64)
    bc = lambda: DenseNet(12, (2, 2, 2), 24, num_classes=5)          # growth 12: the channel-padded twin with the CIFAR stem
    run("densenet_bc_padded_det", bc, x32)
    run("densenet_bc_padded_fp32_det", bc, x32, fp32=True)
    dense = lambda cfg=(2, 2, 2, 2), **kw: (lambda: DenseNet(32, cfg, 64, num_classes=5, **kw))
    run("densenet_det", dense(), x64)
    run("densenet_fp32_det", dense(), x64, fp32=True)
    run("densenet_frozen_det", dense(), x64, train=False)
    run("densenet_dx_det", dense(), x64, dx=True)
    run("densenet_u8_det", dense(), u8)
    run("densenet_reducer_det", dense(), x64, reducer=True)
    run("densenet_after_eval_det", dense(), x64, eval_first=True)
    run("densenet_max_det", dense(), x64, pool="max")
    run("densenet_drop_det", dense(drop_rate=0.25), x64)
    run("densenet_drop_frozen_det", dense(drop_rate=0.25), x64, train=False)
    run("densenet121_det", dense((6, 12, 24, 16)), x64)
    run("densenet121_pair_all_det", dense((6, 12, 24, 16)), x64, env={"CHEXPERT_PAIR_BWD": "all"})
    run("densenet4352_pair_all_det", dense((4, 3, 5, 2)), x64, env={"CHEXPERT_PAIR_BWD": "all"})      # odd layer counts
    run("densenet4352_pair_1_det", dense((4, 3, 5, 2)), x64, env={"CHEXPERT_PAIR_BWD": "1"})
    apv = lambda S, v: dict(ap(S), v=v)        # (a share of attention channels that leaves these narrow transitions some)
    run("densenet_aa_det", dense(attn_params=apv(64, .25)), x64)
    run("densenet_aa_fp32_det", dense(attn_params=apv(64, .25)), x64, fp32=True)
    run("densenet_aa_frozen_det", dense(attn_params=apv(64, .25)), x64, train=False)
    run("densenet_aa_dx_det", dense(attn_params=apv(64, .25)), x64, dx=True)
    bc3 = lambda **kw: (lambda: DenseNet(12, (3, 3, 3), 24, num_classes=5, **kw))
    run("densenet_bc333_det", bc3(), x32)
    run("densenet_bc333_fp32_det", bc3(), x32, fp32=True)
    run("densenet_bc333_drop_det", bc3(drop_rate=0.2), x32)
    run("densenet_bc333_aa_det", bc3(attn_params=apv(32, .7)), x32)
    run("densenet_bc333_dx_frozen_det", bc3(), x32, dx=True, train=False)
    run("gradcam_hooks_efficientnet_b0", eff, x64, train=False, hooked=True)
    run("gradcam_maps_efficientnet_b0", eff, x64, train=False, cam=True)
    run("gradcam_maps_bottleneck", bott(), x64, train=False, cam=True)
    run("gradcam_maps_densenet", lambda: DenseNet(32, (2, 2, 2, 2), 64, num_classes=5), x64, train=False, cam=True)
    run("gradcam_hooks_bottleneck", bott(), x64, train=False, hooked=True)
    run("gradcam_hooks_densenet", lambda: DenseNet(32, (2, 2, 2, 2), 64, num_classes=5), x64, train=False, hooked=True)


def time_steps(steps=20, warmup=3):
    """Median host seconds of one DenseNet121 step (B = 2, 64x64) under the recorders."""
    global TRACE
    import time
    from chexpert_amd.models import DenseNet
    for k in SWITCHES:
        os.environ.pop(k, None)
    torch.manual_seed(0)
    model = DenseNet(32, (6, 12, 24, 16), 64, num_classes=5).train()
    eng = model._eng()
    x, times = torch.randn(2, 3, 64, 64), []
    for i in range(warmup + steps):
        TRACE = Trace()                        # (a fresh list per step: the log does not grow)
        t0 = time.perf_counter()
        ws = eng.forward(x, True, record=True)
        eng.backward(ws, torch.ones(ws.logits.shape, dtype=torch.float32))
        eng.release(ws)
        times.append(time.perf_counter() - t0)
    times = sorted(times[warmup:])
    print("densenet121 host step: median %.2f ms of %d" % (1e3 * times[len(times) // 2], steps), flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    DUMP = None
    RANK = "--rank-offsets" in argv
    if RANK:
        argv.remove("--rank-offsets")
    TIME = "--time" in argv
    if TIME:
        argv.remove("--time")
    if "--dump" in argv:
        i = argv.index("--dump")
        DUMP = argv[i + 1]
        del argv[i:i + 2]
        os.makedirs(DUMP, exist_ok=True)
    tree = os.path.abspath(argv[0]) if argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path.insert(0, tree)
    import chexpert_amd
    assert os.path.abspath(chexpert_amd.__file__).startswith(os.path.abspath(tree)), chexpert_amd.__file__
    import chexpert_amd.ops
    patch(chexpert_amd)
    time_steps() if TIME else main()
