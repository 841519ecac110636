"""CPU (no GPU): host side of the clipping / non-finite skip / EMA options of the fused optimisers: state_dict round trip, old
checkpoints, constructor and command-line validation, argument checks of the new entry points before any launch."""
import pytest
import torch


class _Eng:
    flat = torch.arange(10.0)
    flat_grad = torch.zeros(10)
    packed_version = 0


class _M:
    def _eng(self):
        return _Eng


def test_state_dict_round_trip_carries_the_options_ema_and_skipped():
    from chexpert_amd.optim import FusedAdam, FusedRMSprop, FusedSGDNesterov
    a = FusedAdam(_M(), lr=1e-3, max_grad_norm=2.5, skip_nonfinite=True, ema_decay=0.99, ema_warmup=False)
    a.step_count = 7
    _, _, st = a._bufs(2)                                     # workspace, clip and the EMA are allocated beside the states
    assert torch.equal(a._ema, _Eng.flat) and a._ema.data_ptr() != _Eng.flat.data_ptr()
    assert a._clip.tolist() == [0.0, 1.0, 0.0, 0.0] and a._ws.numel() >= 1
    a._ema.mul_(3.0)
    a._clip[3] = 2.0
    st[1].copy_(torch.arange(10.0) * 2)
    sd = a.state_dict()
    assert (sd["max_grad_norm"], sd["skip_nonfinite"], sd["ema_decay"], sd["ema_warmup"], sd["skipped"]) == (2.5, True, 0.99, False, 2)
    b = FusedAdam(_M(), lr=1.0)
    b.load_state_dict(sd)
    assert (b.max_grad_norm, b.skip_nonfinite, b.ema_decay, b.ema_warmup, b.step_count) == (2.5, True, 0.99, False, 7)
    assert b.skipped_steps() == 2                             # known before the buffers are bound
    _, _, st = b._bufs(2)
    assert torch.equal(st[1], torch.arange(10.0) * 2)
    assert torch.equal(b._ema, torch.arange(10.0) * 3) and b.skipped_steps() == 2
    sd2 = b.state_dict()
    assert torch.equal(sd2["ema"], sd["ema"]) and sd2["skipped"] == 2
    # a second round trip before anything is bound keeps what was loaded
    c = FusedAdam(_M(), lr=1.0)
    c.load_state_dict(sd)
    assert torch.equal(c.state_dict()["ema"], sd["ema"]) and c.state_dict()["skipped"] == 2
    for cls in (FusedSGDNesterov, FusedRMSprop):
        o = cls(_M(), lr=0.1, ema_decay=0.5)
        assert o.state_dict()["ema_decay"] == 0.5 and o.state_dict()["max_grad_norm"] is None


def test_old_format_state_dict_leaves_the_options_off():
    from chexpert_amd.optim import FusedAdam
    a = FusedAdam(_M(), lr=1e-3)
    a._state = [torch.arange(10.0), torch.arange(10.0) * 2]
    sd = a.state_dict()
    assert set(sd) == {"kind", "lr", "base_lr", "step_count", "sched_steps", "state"}       # options off: the keys of before
    b = FusedAdam(_M(), lr=1.0)
    b.load_state_dict(sd)
    assert (b.max_grad_norm, b.skip_nonfinite, b.ema_decay, b.ema_warmup) == (None, False, None, True)
    assert not b._ex_on()
    _, _, st = b._bufs(2)
    assert b._ema is None and b._clip is None and b._ws is None
    with pytest.raises(RuntimeError, match="ema_decay"):
        with b.ema_weights():
            pass
    with pytest.raises(RuntimeError):
        b.grad_norm()


def test_ema_weights_swaps_and_restores():
    from chexpert_amd.optim import FusedSGDNesterov

    class Eng:
        flat = torch.arange(6.0)
        flat_grad = torch.zeros(6)
        packed_version = 5

    class M:
        def _eng(self):
            return Eng
    o = FusedSGDNesterov(M(), lr=0.1, ema_decay=0.9)
    o._bufs(1)
    o._ema.fill_(7.0)
    with o.ema_weights():
        assert Eng.packed_version is None
        assert torch.equal(Eng.flat, torch.full((6,), 7.0)) and torch.equal(o._ema, torch.arange(6.0))
        Eng.packed_version = 9
    assert Eng.packed_version is None
    assert torch.equal(Eng.flat, torch.arange(6.0)) and torch.equal(o._ema, torch.full((6,), 7.0))


def test_constructor_validation():
    from chexpert_amd.optim import FusedAdam, FusedRMSprop
    for kw in ({"max_grad_norm": 0.0}, {"max_grad_norm": -1.0}, {"ema_decay": 0.0}, {"ema_decay": 1.0}, {"max_grad_norm": float("nan")}):
        with pytest.raises(ValueError):
            FusedAdam(_M(), lr=1e-3, **kw)
    o = FusedRMSprop(_M(), lr=1e-3)
    assert (o.max_grad_norm, o.skip_nonfinite, o.ema_decay, o.ema_warmup) == (None, False, None, True)


def test_cli_flags_validation_and_defaults():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    # the namespace of before is unchanged ...
    assert (a.batch_size, a.lr, a.n_epochs, a.log_interval, a.eval_interval, a.lr_decay_factor, a.model, a.fused_optimizer, a.graph) == \
        (16, 1e-4, 1, 50, 300, 0.97, "densenet121", False, False)
    # ... and the new flags are off
    assert (a.clip_grad_norm, a.skip_nonfinite, a.ema_decay, a.no_ema_warmup, a.use_ema) == (None, False, None, False, False)
    assert cli.optimizer_options(a) == {}
    for argv in (["--clip_grad_norm", "1.0"], ["--skip_nonfinite"], ["--ema_decay", "0.999"], ["--no_ema_warmup"]):
        with pytest.raises(ValueError, match="--fused_optimizer"):
            cli.main(argv)                                    # raised before anything touches data or the GPU
    for argv, word in ((["--clip_grad_norm", "0"], "--clip_grad_norm"), (["--clip_grad_norm", "-2"], "--clip_grad_norm"),
                       (["--ema_decay", "0"], "--ema_decay"), (["--ema_decay", "1"], "--ema_decay"), (["--ema_decay", "1.5"], "--ema_decay")):
        with pytest.raises(ValueError, match=word):
            cli.main(["--fused_optimizer"] + argv)
    b = cli.build_parser().parse_args(["--fused_optimizer", "--clip_grad_norm", "3", "--skip_nonfinite", "--ema_decay", "0.999",
                                       "--no_ema_warmup"])
    assert cli.optimizer_options(b) == {"max_grad_norm": 3.0, "skip_nonfinite": True, "ema_decay": 0.999, "ema_warmup": False}
    c = cli.build_parser().parse_args(["--fused_optimizer", "--ema_decay", "0.9"])
    assert cli.optimizer_options(c) == {"max_grad_norm": None, "skip_nonfinite": False, "ema_decay": 0.9, "ema_warmup": True}
    # --use_ema reads ema_state_dict and says so when a checkpoint has none
    e = cli.build_parser().parse_args(["--evaluate", "--use_ema"])
    assert cli.model_weights({"state_dict": 1, "ema_state_dict": 2}, e) == 2
    assert cli.model_weights({"state_dict": 1, "ema_state_dict": 2}, a) == 1
    with pytest.raises(RuntimeError, match="ema_state_dict"):
        cli.model_weights({"state_dict": 1}, e, "checkpoint_latest.pt")


def test_new_entry_points_validate_before_launching():
    """Argument validation happens before any launch, so it can be exercised without a GPU."""
    import ctypes
    from chexpert_amd import _lib
    l = _lib.lib()
    assert [l.cx_grad_norm_partials(n) for n in (0, 1, 3, 4096, 4097, 4100, 5000003, 58154053)] == [0, 1, 1, 1, 1, 2, 1221, 2048]
    buf = (ctypes.c_float * 16)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    assert l.cx_grad_norm(None, 8, 1.0, 0.0, 0, base, 4, base, None) == -1                # CX_EINVAL: no gradient
    assert l.cx_grad_norm(base, 8, 1.0, 0.0, 0, base, 0, base, None) == -1                # workspace too small
    assert l.cx_grad_norm(base + 4, 8, 1.0, 0.0, 0, base, 4, base, None) == -2            # CX_EALIGN, before any launch
    assert l.cx_adam_step_ex(None, None, None, None, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, 1.0, None, None, 0.0, 0, 0, None) == -1
    assert l.cx_adam_step_ex(base, base, base, base, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 1.0, None, None, 0.0, 0, 0, None) == -1    # step < 1
    assert l.cx_sgd_nesterov_step_dev_ex(base, base, base, 4, None, 0.9, 0.0, 1.0, None, None, 0.0, 0, 0, None) == -1          # no hyper
    assert l.cx_rmsprop_step_ex(base, base, base, base, 4, 0.1, 0.99, 1e-3, 0.9, 0.0, 1, 1.0, None, base, 1.5, 0, 0, None) == -1  # decay > 1
