"""Call trace of the ResNet / WideResNet / EfficientNet engines on the CPU, without the library: every function of chexpert_amd.ops
and the `lib` / `ptr` / `stream_ptr` / `check` names of models/resnet.py and models/efficientnet.py are replaced by recorders, so
`eng.forward` / `eng.backward` run on CPU tensors and leave the list of calls they would have issued.  A host-side refactor of an
engine is right when this list is EQUAL before and after, for every configuration below.

    python scratch/record_calls.py [TREE] [--dump DIR]

TREE: the checkout to import chexpert_amd from (default: this one), so the script can be pointed at a checkout of another commit.
Prints one line per configuration: name, number of calls, sha256 of the list.  --dump writes each list to DIR/<name>.txt (diff them).

What a call logs: the function's name and its arguments; a tensor as (index of its storage by first appearance, storage offset,
shape, strides, dtype), anything else by repr.  Calls made directly on tensors are logged too when they write: `zero_`, `fill_`,
`copy_`, `add_` and `torch.add(..., out=)` (a TorchFunctionMode), and so are the reducer's `begin` / `ready(offset)` / `finish`.
Every recorder returns ROWS where the real function returns a statistic-row count."""
import hashlib
import inspect
import os
import sys

import torch
from torch.overrides import TorchFunctionMode

ROWS = 7
SWITCHES = ("CHEXPERT_DET", "CHEXPERT_JOIN_FUSE", "CHEXPERT_FWD_JOIN_FUSE", "CHEXPERT_STREAM_LO")


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

    def digest(self):
        return hashlib.sha256("\n".join(repr(c) for c in self.calls).encode()).hexdigest()[:16]


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
    def __getattr__(self, name):
        return _recorder("lib." + name, ROWS if name == "cx_last_stat_rows" else 0)


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
        if callable(fn) and getattr(fn, "__module__", None) == ops.__name__ and not isinstance(fn, type):
            setattr(ops, name, _recorder("ops." + name, special.get(name, ROWS), inspect.signature(fn)))
    from chexpert_amd.models import efficientnet, resnet
    for mod in (resnet, efficientnet):
        mod.lib, mod.ptr, mod.stream_ptr, mod.check = (lambda: _Lib()), (lambda t: None if t is None else _Ptr(t)), (lambda: 0), \
            (lambda rc, what: None)


def run(name, make, x, *, train=True, dx=False, reducer=False, fp32=False, env=None, steps=2):
    global TRACE
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    TRACE = Trace()
    torch.manual_seed(0)
    model = make()
    if fp32:
        model.storage_dtype(torch.float32)
    model.train(train)
    eng = model._eng()
    if reducer:
        eng.reducer = _Reducer()
    with _TensorWrites():
        for _ in range(steps):                 # the second step takes the pooled workspace and its backward buffers
            ws = eng.forward(x, train, record=True)
            dl = torch.ones(ws.logits.shape, dtype=torch.float32)
            eng.backward(ws, dl, dx=torch.empty(x.shape[0], 3, *x.shape[2:], dtype=torch.float32) if dx else None)
            eng.release(ws)
    print("%-28s %5d calls  %s" % (name, len(TRACE.calls), TRACE.digest()), flush=True)
    if DUMP:
        with open(os.path.join(DUMP, name + ".txt"), "w") as f:
            f.writelines(repr(c) + "\n" for c in TRACE.calls)


def main():
    from chexpert_amd.models import BasicBlock, Bottleneck, ResNet, WideResNet
    from chexpert_amd.models.efficientnet import construct_model
    x64, x32 = torch.randn(2, 3, 64, 64), torch.randn(2, 3, 32, 32)
    u8 = torch.randint(0, 255, (2, 1, 64, 64), dtype=torch.uint8)
    ap = lambda S: {"k": .2, "v": .1, "nh": 8, "relative": True, "input_dims": (S, S)}
    bott = lambda **kw: (lambda: ResNet(Bottleneck, [1, 6, 2, 1], num_classes=5, **kw))      # a stage of 6: fuse_fwd, keep_lo, EPI_JOIN
    basic = lambda **kw: (lambda: ResNet(BasicBlock, [2, 2, 1, 1], num_classes=5, **kw))
    wrn = lambda d=10, k=2, **kw: (lambda: WideResNet(BasicBlock, d, k, num_classes=5, **kw))
    eff = lambda: construct_model("efficientnet-b0", 5)
    atomic = {"CHEXPERT_DET": "0"}
    run("bottleneck_det", bott(), x64)
    run("bottleneck_atomic", bott(), x64, env=atomic)
    for sw in ("CHEXPERT_JOIN_FUSE", "CHEXPERT_FWD_JOIN_FUSE", "CHEXPERT_STREAM_LO"):
        run("bottleneck_%s0_det" % sw[9:].lower(), bott(), x64, env={sw: "0"})
        run("bottleneck_%s0_atomic" % sw[9:].lower(), bott(), x64, env={sw: "0", **atomic})
    run("bottleneck_fp32_det", bott(), x64, fp32=True)
    run("bottleneck_fp32_atomic", bott(), x64, fp32=True, env=atomic)
    run("bottleneck_frozen_det", bott(), x64, train=False)
    run("bottleneck_frozen_atomic", bott(), x64, train=False, env=atomic)
    run("bottleneck_dx_det", bott(), x64, dx=True)
    run("bottleneck_dx_frozen_atomic", bott(), x64, dx=True, train=False, env=atomic)
    run("bottleneck_u8_det", bott(), u8)
    run("bottleneck_reducer_det", bott(), x64, reducer=True)
    run("bottleneck_reducer_atomic", bott(), x64, reducer=True, env=atomic)
    for tag, kw in (("grouped", dict(groups=4, width_per_group=16)), ("dilated", dict(replace_stride_with_dilation=[False, True, True])),
                    ("wide128", dict(width_per_group=128)), ("aa", dict(attn_params=ap(64)))):
        run("bottleneck_%s_det" % tag, bott(**kw), x64)
        run("bottleneck_%s_atomic" % tag, bott(**kw), x64, env=atomic)
    run("bottleneck_aa_fp32_det", bott(attn_params=ap(64)), x64, fp32=True)
    run("bottleneck_aa_frozen_det", bott(attn_params=ap(64)), x64, train=False)
    for tag, mk, x in (("basic", basic(), x64), ("basic_aa", basic(attn_params=ap(64)), x64), ("wrn", wrn(), x32),
                       ("wrn16_4_aa", wrn(16, 4, attn_params=ap(32)), x32)):
        run(tag + "_det", mk, x)
        run(tag + "_atomic", mk, x, env=atomic)
        run(tag + "_dx_det", mk, x, dx=True)
        run(tag + "_frozen_atomic", mk, x, train=False, env=atomic)
        run(tag + "_reducer_det", mk, x, reducer=True)
    run("basic_fp32_det", basic(), x64, fp32=True)
    for tag, kw in (("det", {}), ("atomic", dict(env=atomic))):
        run("efficientnet_b0_" + tag, eff, x64, **kw)
        run("efficientnet_b0_frozen_" + tag, eff, x64, train=False, **kw)
        run("efficientnet_b0_dx_reducer_" + tag, eff, x64, dx=True, reducer=True, **kw)
    run("efficientnet_b0_fp32_det", eff, x64, fp32=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    DUMP = None
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
    main()
