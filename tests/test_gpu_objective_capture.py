"""The masked objective inside a captured step (ddr_amd.capture.CapturedStep): the observation window and the drop mask
change in place between replays -- other missing days, another number of kept gauges -- without a new shape or a host
sync, and every replay's loss and gradient are bit-identical to the eager call on the same data."""

import numpy as np
import pytest
import torch

import objective_cases as oc
from ddr_amd.capture import CapturedStep
from ddr_amd.train import daily_objective

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["l1", "kge"])
def test_replays_follow_the_buffers(cuda, kind):
    G, D, warmup = 64, 89, 3
    pred, obs_a, _ = oc.make_inputs(G, D, warmup, seed=1)
    _, obs_b, _ = oc.make_inputs(G, D, warmup, seed=2)
    drop_a = np.isnan(obs_a).sum(1) > 9
    drop_b = np.isnan(obs_b).sum(1) > 7
    assert 0 < drop_a.sum() < drop_b.sum() < G  # the number of kept gauges differs
    windows = [(torch.from_numpy(o).to(cuda), torch.from_numpy(d).to(cuda)) for o, d in ((obs_a, drop_a), (obs_b, drop_b))]

    leaf = torch.from_numpy(pred).to(cuda).requires_grad_(True)
    obs_buf = windows[0][0].clone()
    drop_buf = windows[0][1].clone()
    out = {}

    def step():
        leaf.grad = None
        loss = daily_objective(leaf, obs_buf, warmup, kind, drop=drop_buf)
        loss.backward()
        out["loss"] = loss

    captured = CapturedStep(step)
    losses = []
    for obs, drop in (windows[1], windows[0], windows[1]):
        obs_buf.copy_(obs)
        drop_buf.copy_(drop)
        captured()
        torch.cuda.synchronize()
        got_loss, got_grad = out["loss"].item(), leaf.grad.cpu().numpy().copy()
        eager = torch.from_numpy(pred).to(cuda).requires_grad_(True)
        want = daily_objective(eager, obs, warmup, kind, drop=drop)
        want.backward()
        assert np.isfinite(got_loss) and oc.bits(got_loss) == oc.bits(want.item())
        assert (oc.bits(got_grad) == oc.bits(eager.grad.cpu().numpy())).all()
        assert not oc.bits(got_grad)[drop.cpu().numpy()].any() and got_grad[~drop.cpu().numpy()].any()
        losses.append(got_loss)
    assert losses[0] == losses[2] and losses[0] != losses[1]
