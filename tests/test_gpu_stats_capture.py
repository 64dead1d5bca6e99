"""summarize and step_summary inside a captured step (ddr_amd.capture.CapturedStep: warm-up on a side stream, then
torch.cuda.graph): the inputs change in place between replays, and every replay's record is bit-identical to the
eager call on the same data.  Capture fails on a host synchronisation, so passing shows there is none.  The captured
graph is a single chain of launches."""

import numpy as np
import pytest
import torch

from ddr_amd.capture import CapturedStep
from ddr_amd.stats import TILE, summarize
from ddr_amd.train import step_summary
from ddr_amd.validation import METRIC_NAMES

pytestmark = pytest.mark.gpu


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int64)


def test_replays_follow_the_buffers(cuda):
    N, G, P = 3 * TILE + 1, 37, 4099
    i_nse = METRIC_NAMES.index("nse")

    def data(seed):
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((2, N)).astype(np.float32) * (seed + 1)
        x[1, rng.permutation(N)[:N // 50]] = np.nan
        mv = rng.standard_normal((len(METRIC_NAMES), G))
        mv[i_nse, [seed, 20]] = (np.nan, -np.inf)
        params = [rng.uniform(0.0, 1.0 + seed, P).astype(np.float32) for _ in range(3)]
        params[1][[5, 6 + seed]] = np.nan
        return [torch.from_numpy(a).to(cuda) for a in (x, mv, *params)]

    x, mv, *params = data(0)
    names = ("n", "q_spatial", "p_spatial")
    buf = torch.zeros(2, 7, device=cuda, dtype=torch.float64)
    rec = torch.zeros(6, 6, device=cuda, dtype=torch.float64)

    def step():
        summarize(x, q=(0.1, 0.5), out=buf)
        step_summary(mv, dict(zip(names, params)), out=rec)

    captured = CapturedStep(step)
    seen = []
    for seed in (1, 2, 1):
        fresh = data(seed)
        for dst, src in zip((x, mv, *params), fresh):
            dst.copy_(src)
        captured()
        torch.cuda.synchronize()
        want_buf = summarize(fresh[0], q=(0.1, 0.5)).table
        want_rec = step_summary(fresh[1], dict(zip(names, fresh[2:]))).record
        assert torch.equal(bits(buf), bits(want_buf))
        assert torch.equal(bits(rec), bits(want_rec))
        assert buf[1, 0].item() == N - N // 50 and rec[4, 0].item() == P - 2
        seen.append((buf.clone(), rec.clone()))
    assert torch.equal(bits(seen[0][0]), bits(seen[2][0])) and not torch.equal(bits(seen[0][0]), bits(seen[1][0]))
    assert torch.equal(bits(seen[0][1]), bits(seen[2][1])) and not torch.equal(bits(seen[0][1]), bits(seen[1][1]))
