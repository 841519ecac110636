"""The fused training step written out by the tests themselves (not collected: no test_ prefix).

It does NOT go through `optimizer.train_step`: the graph-against-eager tests compare a replay of the captured train_step with
this independent statement of the same five lines, and test_train_step_gpu.py compares train_step itself with it."""


def _eager_dev_step(model, opt, x, t):
    """The step GraphedTrainStep captures, launched one by one (the command line's partial-minibatch step)."""
    opt.zero_grad()
    loss, _ = model.forward_backward(x, t)
    opt.step_dev()
    opt.tick()
    model._eng().packed_version = None
    return loss.clone()
