"""One training step (chexpert.py:159-165: forward, BCE loss, backward, optimiser step, scheduler step) captured once as a
hipGraph and replayed per minibatch.

Why: a DenseNet121 step is ~900 kernel launches; enqueued one by one through ctypes they cost ~18 ms of host time, which
becomes the floor once the GPU side of the step is faster than that.  A replay costs ~10-20 us of host time (one
`hipGraphLaunch`).  Shapes are static: the caller copies each minibatch into `x` / `target` (device tensors owned by this
object) and calls `replay()`.  Learning rate and step count live in device memory (`optim._Flat.hyper`), so the optimiser and
the scheduler advance inside the graph.

What is captured is the optimiser's own statement of the step, `optimizer.train_step(model, x, target, dev=True)`
(optim._Flat.train_step; optim.FusedSAM.train_step for its two passes), the one the command line launches eagerly as well.
"""
import torch


def _step_state(model):
    """What a training step changes beside the parameters: the module buffers and the state of the model's loss."""
    return list(model.buffers()) + list(getattr(model, "loss_step_state", lambda: [])())


class _CapturedStep:
    """What GraphedTrainStep and SegmentedTrainStep share: the tensors a replay reads, the eager warm-up on a side stream, the
    step that is captured, putting back what the warm-up changed, and the two ends of `replay()`."""

    def _warm_up(self, model, optimizer, x, target, warmup_steps, warmup_iters):
        """Binds the object to `model` / `optimizer` and clones of `x` / `target`, then runs the step eagerly on the side stream
        it returns: that binds the engine, allocates the workspaces, sets kernel attributes and creates the optimiser state, none
        of which may happen during capture.  It runs every kind of pass the step has but no optimiser, so the parameters stay as
        they are (an optimiser of two passes, optim.FusedSAM, gets its second pass's path through the engine warmed up too)."""
        self.model, self.opt = model, optimizer
        self.x, self.target = x.clone(), target.clone()
        # (Dropout / DropConnect masks: their step counter lives in device memory and is bumped inside the captured step --
        # efficientnet.py, cx_dropout_mask_dev -- so every replay draws new masks)
        model.train()
        # construction is free of side effects on the model: the warm-up steps really run (they update BatchNorm running
        # statistics), so the module buffers and the num_batches_tracked bookkeeping are put back afterwards (`_restore`)
        # (so are the auxiliary scalars of set_loss(kind="aucm"), which a train-mode step updates: loss_step_state)
        self._saved = [(b, b.detach().clone()) for b in _step_state(model)]
        self._nbt = getattr(model, "_nbt_pending", 0)
        s = torch.cuda.Stream(device=x.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(max(1, warmup_iters)):                  # (data-parallel: real collectives, every rank alike)
                model.zero_grad()
                self.loss, self.logits = model.forward_backward(self.x, self.target)
            if optimizer is not None and optimizer.PASSES == 2:
                model.zero_grad()
                model.forward_backward(self.x, self.target, track_stats=False)
            if optimizer is not None:
                optimizer._bufs(optimizer.NSTATE)
                optimizer.hyper(warmup_steps)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        return s

    def _step(self):
        """The step under capture: the optimiser's train_step on the device-resident learning rate and step count."""
        if self.opt is None:
            self.model.zero_grad()
            self.loss, self.logits = self.model.forward_backward(self.x, self.target)
        else:
            self.loss, self.logits = self.opt.train_step(self.model, self.x, self.target, dev=True)

    def _restore(self, s):
        """Joins the side stream and puts the buffers the warm-up steps changed back (they really ran)."""
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        with torch.no_grad():
            for b, v in self._saved:
                b.copy_(v)
        if hasattr(self.model, "_nbt_pending"):
            self.model._nbt_pending = self._nbt
        self._saved = None

    def _copy_in(self, x, target):
        if x is not None:
            self.x.copy_(x, non_blocking=True)
        if target is not None:
            self.target.copy_(target, non_blocking=True)

    def _replayed(self):
        self.replays += 1
        # the captured optimiser kernel has just changed the fp32 masters without touching tensor versions: an eval forward that
        # follows must repack the weights (Engine.pack(train=False) compares versions)
        self.model._eng().packed_version = None
        self.model._nbt_pending += 1           # BatchNorm num_batches_tracked is host-side bookkeeping (flushed by state_dict())
        return self.loss, self.logits


class GraphedTrainStep(_CapturedStep):
    def __init__(self, model, optimizer, x, target, warmup_steps=0, warmup_iters=2):
        if not x.is_cuda:
            raise RuntimeError("GraphedTrainStep needs device tensors (no CPU path)")
        if getattr(model._eng(), "reducer", None) is not None:
            raise RuntimeError("graph capture of the data-parallel step is not supported (collectives are enqueued eagerly)")
        s = self._warm_up(model, optimizer, x, target, warmup_steps, warmup_iters)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._step()
        self._restore(s)
        self.replays = 0

    def replay(self, x=None, target=None):
        """Run one step; returns (loss, logits) device tensors that the NEXT replay overwrites."""
        self._copy_in(x, target)
        self.graph.replay()
        return self._replayed()


_TEST_FAIL_CAPTURE = 0          # tests/test_dp_gpu.py: N > 0 raises at the N-th cut, i.e. in the middle of a captured backward pass


class SegmentedTrainStep(_CapturedStep):
    """The data-parallel training step as a CHAIN of hipGraphs.

    Collectives are enqueued from Python (parallel.GradReducer), so the whole step cannot be one graph.  Enqueued launch by
    launch it pays a dependent-launch gap at every kernel boundary that a graph does not have: 37.7 ms instead of 30.3 ms per
    DenseNet121 step on one MI355X, 66.5 instead of 56.6 for ResNet152 (bench.py's eager replica against its graph replay).
    Here the step is captured once with the reducer in capture mode: wherever backward completes a gradient bucket
    (`GradReducer.ready`) the capture is cut, so a replay is

        segment 0 (zero_grad, forward, loss, backward up to bucket 0) -> all-reduce(bucket 0) on the reducer's stream
        segment 1 (backward up to bucket 1)                            -> all-reduce(bucket 1) ...
        ...                                                            -> wait for the collectives
        last segment (whatever backward does after the join, optimiser step, scheduler tick)

    with the same launches, the same order and the same collectives as the eager data-parallel step: the kernels between two
    cuts run as a graph, the all-reduces overlap the following segments as before.  All segments share one memory pool."""

    def __init__(self, model, optimizer, x, target, warmup_steps=0, warmup_iters=2):
        if not x.is_cuda:
            raise RuntimeError("SegmentedTrainStep needs device tensors (no CPU path)")
        if optimizer is not None and optimizer.PASSES == 2:
            raise RuntimeError("SegmentedTrainStep refuses FusedSAM: data-parallel SAM is not supported (the first pass would have to "
                               "skip the all-reduce)")
        red = getattr(model._eng(), "reducer", None)
        if red is None:
            raise RuntimeError("SegmentedTrainStep is the data-parallel form (engine.enable_data_parallel() first); a single process uses GraphedTrainStep")
        self.red = red
        s = self._warm_up(model, optimizer, x, target, warmup_steps, warmup_iters)
        self.segs = []                                              # [(graph, actions)]; an action: ("launch", lo, hi) | ("finish",)
        self._pool = torch.cuda.graph_pool_handle()
        self._g = None
        red.capture = self
        try:
            with torch.cuda.stream(s):
                try:
                    self._begin()
                    self._step()
                    self._g.capture_end()
                    self.segs.append((self._g, ()))
                    self._g = None
                except BaseException:
                    # A capture must be ended on the stream (and thread) that began it, and BEFORE its graph object dies: ending
                    # it after `with torch.cuda.stream(s)` had restored the caller's stream failed torch's stream check, the
                    # stream stayed in capture mode, and tearing the objects down later aborted the process (round 3 parked them
                    # and left through os._exit).  Here the open segment is closed while `s` is still current; a capture the
                    # runtime has invalidated raises from capture_end too, but hipStreamEndCapture has then already taken the
                    # stream out of capture mode.
                    if self._g is not None:
                        try:
                            self._g.capture_end()
                        except Exception:
                            pass
                    self._g, self.segs = None, []
                    raise
        except BaseException as capture_error:
            # the clean-up below touches the GPU; if the failed capture left the device in a state where that raises too, the caller
            # must still see the ORIGINAL error (bench.py logs it and falls back to the eager step), chained, not replaced
            red.capture = None
            try:
                self._restore(s)
            except Exception as cleanup_error:
                raise capture_error from cleanup_error
            raise
        red.capture = None
        self._restore(s)
        self.replays = 0

    def _begin(self):
        self._g = torch.cuda.CUDAGraph()
        # thread_local: the process group's watchdog / proxy threads may query events while this thread captures
        self._g.capture_begin(pool=self._pool, capture_error_mode="thread_local")

    def cut(self, *actions):
        """Called by the reducer in capture mode: end the current segment here; `actions` run at this point of every replay."""
        self._g.capture_end()
        self.segs.append((self._g, actions))
        self._begin()
        if _TEST_FAIL_CAPTURE and len(self.segs) == _TEST_FAIL_CAPTURE:
            raise RuntimeError("forced capture failure (test hook)")

    def replay(self, x=None, target=None):
        self._copy_in(x, target)
        red = self.red
        red.begin()
        for g, actions in self.segs:
            g.replay()
            for action in actions:
                if action[0] == "launch":
                    red._launch(action[1], action[2])
                else:
                    red.wait()
        return self._replayed()
