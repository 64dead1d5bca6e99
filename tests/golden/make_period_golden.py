"""Generate ``period.npz``: the reference's whole-period inference loop.  BUILD-CONTAINER ONLY.

Like ``make_golden.py`` (whose loaders it reuses) this imports the reference's routing modules at run time
and stores arrays only.  The loop is ``scripts/router.py:152-167`` / ``scripts/test.py:57-112``: the period is
walked in ``batch_size``-day chunks (``DataLoader(SequentialSampler, batch_size)``), every chunk after the
first gets the previous day prepended (``base_geodataset.py:44-49``) and runs with ``carry_state=True`` on
the same engine object, each chunk's hourly output lands in ``predictions[:, first * 24 : last * 24]``, and
the whole is trimmed to ``[13 + tau : -11 + tau]`` and pooled to daily means
(``scripts_utils.compute_daily_runoff`` -> ``io/functions.py`` ``downsample``).

Case: ``synthetic.random_binary_tree(300, seed=41)``, attributes and unit parameters of seed 41, the daily
store ``synthetic.lateral_inflow(300, 8, 41)`` (8 days), all-reach and gauge mode.

Stored: ``daily_B{B}_tau{tau}_{all,gauge}`` for B in {2, 3, 8} x tau in {0, 3}; ``hourly_B3_{all,gauge}``,
the full hourly predictions of B = 3; ``chunks_B{B}`` the (first_day, last_day) of every routed chunk;
the gauges (``outflow_flat`` / ``outflow_offsets``) and a checksum of the store.

Run:  python tests/golden/make_period_golden.py
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as MG  # noqa: E402
from ddr_amd import synthetic  # noqa: E402

N, SEED, N_DAYS = 300, 41, 8
OUTFLOW = [[-1], [10, 20, 31], [44], [5, 59, 60]]
CHUNK_DAYS, TAUS = (2, 3, 8), (0, 3)


def batches(n_days: int, batch: int) -> list[list[int]]:
    """Day indices of every batch: the sequential sampler's, the previous day prepended from the second on."""
    out = []
    for s in range(0, n_days, batch):
        idx = list(range(s, min(s + batch, n_days)))
        if 0 not in idx:
            idx.insert(0, idx[0] - 1)
        out.append(idx)
    return out


def run(mmc, fun, net, attrs, u, daily_q, batch: int, tau: int, outflow):
    ofl = None if outflow is None else [np.asarray(i) for i in outflow]
    dc = MG.routing_dc(net.n, net.rows, net.cols, attrs, ofl)
    mc = mmc.MuskingumCunge(MG.cfg_of(MG.PARAMS_DEFAULT), device="cpu")
    R = net.n if ofl is None else len(ofl)
    pred = np.zeros((R, (N_DAYS - 1) * 24), np.float32)
    routed = []
    with torch.no_grad():
        for i, idx in enumerate(batches(N_DAYS, batch)):
            qp = np.repeat(daily_q[idx[0]:idx[-1] + 1], 24, axis=0)[:(len(idx) - 1) * 24]
            if qp.shape[0] == 0:
                continue
            sp = {k: torch.from_numpy(v) for k, v in u.items()}
            mc.setup_inputs(dc, torch.from_numpy(qp.copy()), sp, carry_state=i > 0)
            pred[:, idx[0] * 24: idx[-1] * 24] = mc.forward().numpy()
            routed.append((idx[0], idx[-1]))
    sl = torch.from_numpy(pred)[:, 13 + tau: -11 + tau]
    return fun.downsample(sl, rho=sl.shape[1] // 24).numpy(), pred, np.asarray(routed, np.int64)


def main():
    _, mmc = MG.load_reference()
    _, fun = MG.load_objective_modules()
    net = synthetic.random_binary_tree(N, seed=SEED)
    attrs = synthetic.reach_attributes(net.n, SEED)
    u = synthetic.unit_parameters(net.n, SEED)
    daily_q = synthetic.lateral_inflow(net.n, N_DAYS, SEED)
    out = dict(n=np.int64(N), seed=np.int64(SEED), n_days=np.int64(N_DAYS),
               store_sum=np.float64(daily_q.astype(np.float64).sum()),
               outflow_flat=np.concatenate([np.asarray(i, np.int64) for i in OUTFLOW]),
               outflow_offsets=np.cumsum([0] + [len(i) for i in OUTFLOW]).astype(np.int64))
    for B in CHUNK_DAYS:
        for tau in TAUS:
            for mode, ofl in (("all", None), ("gauge", OUTFLOW)):
                daily, pred, routed = run(mmc, fun, net, attrs, u, daily_q, B, tau, ofl)
                assert daily.shape[1] == N_DAYS - 2
                out[f"daily_B{B}_tau{tau}_{mode}"] = daily
                out[f"chunks_B{B}"] = routed
                if B == 3 and tau == TAUS[0]:
                    out[f"hourly_B3_{mode}"] = pred
    np.savez_compressed(HERE / "period.npz", **out)
    print("period.npz", (HERE / "period.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
