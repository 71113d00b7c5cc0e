"""resnet18_gn on the GPU with stock kernels refused: an eager ASGD step leaves a
finite, non-zero gradient in every parameter; the captured step replays with the
eager run's losses bit for bit; and an eval-mode forward under ``no_grad`` is the
train-mode forward bit for bit (GroupNorm has no mode: no eval fold is taken)."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.strict_native]


def _worker():
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    torch.manual_seed(0)
    cfg = TrainConfig(model="resnet18_gn", batch_size=8, mode="asgd", ps="local", n_push=5,
                      n_pull=5, lr=0.01, evaluate=False, verbose=False)
    w = Worker(cfg, DistInfo(device=torch.device("cuda", 0)))
    g = torch.Generator().manual_seed(0)
    x = torch.randn(8, *w.input_shape, generator=g)
    y = torch.randint(0, w.num_classes, (8,), generator=g)
    return w, w.prepare(x, y)


def test_step_gradients_graph_replay_and_no_mode():
    w, (x, y) = _worker()
    assert not list(w.model.buffers())
    eager = [w.train_step(x, y)[0].float().item()]
    for name, p in w.model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert bool((p.grad != 0).any()), name
    eager += [w.train_step(x, y)[0].float().item() for _ in range(3)]
    with torch.no_grad():
        train_out = w.model(x)
        eval_out = w.model.eval()(x)
        w.model.train()
    assert torch.equal(train_out, eval_out)
    w.finish()

    w, (x, y) = _worker()
    assert w.enable_graph()
    graph = [w.train_step(x, y)[0].float().item() for _ in range(4)]   # warm-up, capture, replays
    assert w.graph is not None
    w.finish()
    assert all(v == v and v > 0 for v in eager)
    assert graph == eager, (graph, eager)
