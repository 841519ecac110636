"""CPU: the one statement of the fused training step (optim._Flat.train_step, optim.FusedSAM.train_step) as an order of calls, with
fakes and no device; and the command line's training loader, which is closed however the run ends."""
import pytest
import torch

from test_sam_cpu import Net

LOSS, LOGITS = object(), object()


class StepNet(Net):
    """test_sam_cpu's flat-buffer fake with a forward_backward that only notes how it was called."""

    def __init__(self, calls):
        super().__init__([5, 8, 3])
        self.calls = calls
        self.passes = 0

    def forward_backward(self, x, target, **kw):
        self.calls.append(("forward_backward", x, target, kw))
        self.passes += 1
        return (LOSS, LOGITS) if self.passes == 1 else (object(), object())      # a second pass's results are not the step's


def _recorded(opt, calls, names):
    for name in names:
        setattr(opt, name, lambda *a, _n=name, **kw: calls.append((_n,) + a))
    return opt


def _flat(calls):
    from chexpert_amd.optim import FusedAdam
    net = StepNet(calls)
    return net, _recorded(FusedAdam(net, lr=1e-3), calls, ("zero_grad", "step", "step_dev", "tick"))


def test_flat_train_step_host_form():
    calls = []
    net, opt = _flat(calls)
    net.eng.packed_version = 41
    assert opt.PASSES == 1
    out = opt.train_step(net, "x", "t")
    assert calls == [("zero_grad",), ("forward_backward", "x", "t", {}), ("step",)]
    assert out[0] is LOSS and out[1] is LOGITS
    assert net.eng.packed_version == 41                                          # the host step bumps tensor versions itself


def test_flat_train_step_dev_form():
    calls = []
    net, opt = _flat(calls)
    net.eng.packed_version = 41
    opt.tick = lambda: calls.append(("tick", net.eng.packed_version))          # the stale mark comes after tick()
    out = opt.train_step(net, "x", "t", dev=True)
    assert calls == [("zero_grad",), ("forward_backward", "x", "t", {}), ("step_dev",), ("tick", 41)]
    assert out[0] is LOSS and out[1] is LOGITS
    assert net.eng.packed_version is None


@pytest.mark.parametrize("dev", [False, True])
def test_sam_train_step_is_two_passes_the_second_without_statistics(monkeypatch, dev):
    from chexpert_amd.optim import FusedAdam, FusedSAM
    calls = []
    net = StepNet(calls)
    base = _recorded(FusedAdam(net, lr=1e-3), calls, ("zero_grad", "tick"))
    s = FusedSAM(base)
    # (FusedSAM writes unknown attributes through to its base: its own methods are patched on the class)
    monkeypatch.setattr(FusedSAM, "first_step", lambda self, dev=False: calls.append(("first_step", dev)))
    monkeypatch.setattr(FusedSAM, "second_step", lambda self, dev=False: calls.append(("second_step", dev)))
    assert s.PASSES == 2 and base.PASSES == 1 and "PASSES" in vars(FusedSAM)
    out = s.train_step(net, "x", "t", dev=dev)
    assert calls == [("zero_grad",), ("forward_backward", "x", "t", {}), ("first_step", dev),
                     ("zero_grad",), ("forward_backward", "x", "t", {"track_stats": False}), ("second_step", dev)] + ([("tick",)] if dev else [])
    assert out[0] is LOSS and out[1] is LOGITS


def test_a_foreign_model_is_refused_before_anything_runs():
    from chexpert_amd.optim import FusedSAM
    calls = []
    net, opt = _flat(calls)
    for o in (opt, FusedSAM(opt)):
        for dev in (False, True):
            with pytest.raises(RuntimeError, match="not the one"):
                o.train_step(StepNet(calls), "x", "t", dev=dev)
    assert calls == []


def test_every_fused_optimiser_states_its_passes_and_states():
    from chexpert_amd import optim as O
    for cls, nstate in ((O.FusedAdam, 2), (O.FusedSGDNesterov, 1), (O.FusedRMSprop, 2), (O.FusedLAMB, 2), (O.FusedLARS, 1)):
        assert cls.PASSES == 1 and cls.NSTATE == nstate, cls
        assert cls.train_step is O._Flat.train_step
    assert O.FusedSAM.PASSES == 2


def test_the_training_loader_is_closed_when_the_run_is_refused_after_it_started(monkeypatch, tmp_path):
    """The loader's workers exist from before the first GPU call on; a refusal after that (here: no GPU) must not leave them to
    __del__."""
    from chexpert_amd import cli, loader
    made = []

    class Recorder:
        def __init__(self, dataset, batch_size, **kw):
            self.closed = False
            made.append(self)

        def close(self):
            self.closed = True

    monkeypatch.setattr(loader, "RingLoader", Recorder)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        cli.main(["--train", "--synthetic", "8", "--batch_size", "4", "--resize", "64", "--num_workers", "1",
                  "--output_dir", str(tmp_path / "run")])
    assert len(made) == 1 and made[0].closed
