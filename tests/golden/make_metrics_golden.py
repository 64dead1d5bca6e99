"""Generate ``metrics.npz`` (F14) from the reference's own ``Metrics`` class.  BUILD-CONTAINER ONLY.

Loads ``/root/reference/src/ddr/validation/metrics.py`` by path at run time (it needs numpy, scipy and pydantic
only) and stores, per case, the fp32 inputs and the reference's 18 outputs computed on *the same inputs cast to
fp64*: on fp32 inputs the reference accumulates in fp32 and sits 1-3e-7 from its own fp64 result, which could
not pin the device's fp64 arithmetic.  The reference never travels to the GPU box: only the fixture does.

Inputs: a log-normal random walk per gauge; pred is the walk times log-normal noise, target the walk rounded
to 0.1 (gauge records are quantised: ties, and zeros at low flow) with 10 % NaN sprinkled in.  Special rows,
where the case has room: a target that is all NaN, one with a single valid day, a constant one, one without
NaN, and a pred rounded to 0.1 (ties in pred too).

Keys: ``cases`` (N, 2) of (G, D); ``names`` the 18 metric names in stored row order; per case ``pred_GxD``,
``target_GxD`` (G, D) fp32, ``ref_GxD`` (18, G) fp64, ``special_GxD`` (G,) the special-row code of each gauge
(index into ``special_names``, -1 ordinary); ``json_7x89`` the reference's ``model_dump_json()`` of that case.

Run:  python tests/golden/make_metrics_golden.py
"""

from __future__ import annotations

import importlib.util
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference/src/ddr/validation/metrics.py")

NAMES = ("bias", "mae", "rmse", "ub_rmse", "fdc_rmse", "corr", "corr_spearman", "r2", "nse", "flv", "fhv", "pbias",
         "pbias_mid", "kge", "kge_12", "rmse_low", "rmse_high", "rmse_mid")
SPECIAL = ("target_all_nan", "single_valid_day", "constant_target", "no_nan", "pred_ties")
# (G, D, first special row's code): the listed sizes, and 512 / 513 either side of the one-wave / one-workgroup
# dispatch boundary of csrc/metrics.hip; cases with fewer than five gauges take the specials in turn
CASES = ((5, 1, 0), (5, 2, 0), (6, 3, 0), (7, 89, 0), (7, 100, 0), (5, 365, 0), (4, 1000, 0), (3, 5479, 4),
         (2, 8192, 2), (6, 512, 0), (6, 513, 0))


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_validation_metrics", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Metrics


def make_inputs(rng: np.random.Generator, G: int, D: int, first: int):
    walk = np.exp(rng.normal(0.0, 1.0, (G, 1)) + np.cumsum(rng.normal(0.0, 0.1, (G, D)), axis=1))
    pred = (walk * np.exp(rng.normal(0.0, 0.15, (G, D)))).astype(np.float32)
    target = np.round(walk, 1).astype(np.float32)
    target[rng.uniform(size=(G, D)) < 0.1] = np.nan
    special = np.full(G, -1, np.int32)
    for k in range(min(G, len(SPECIAL))):
        code = (first + k) % len(SPECIAL)
        special[k] = code
        if code == 0:
            target[k] = np.nan
        elif code == 1:
            day = int(rng.integers(D))
            keep = np.round(walk[k, day], 1).astype(np.float32)
            target[k] = np.nan
            target[k, day] = keep
        elif code == 2:
            target[k, ~np.isnan(target[k])] = np.float32(1.7)
        elif code == 3:
            target[k] = np.round(walk[k], 1).astype(np.float32)
        else:
            pred[k] = np.round(pred[k], 1)
    return pred, target, special


def reference_table(Metrics, pred: np.ndarray, target: np.ndarray) -> np.ndarray:
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        m = Metrics(pred=pred.astype(np.float64), target=target.astype(np.float64))
    return np.stack([np.asarray(getattr(m, name), np.float64) for name in NAMES])


def main() -> None:
    Metrics = load_reference()
    rng = np.random.default_rng(20140)
    out = {"cases": np.array([(g, d) for g, d, _ in CASES], np.int64), "names": np.array(NAMES),
           "special_names": np.array(SPECIAL)}
    for G, D, first in CASES:
        pred, target, special = make_inputs(rng, G, D, first)
        ref = reference_table(Metrics, pred, target)
        assert ref.shape == (len(NAMES), G)
        tag = f"{G}x{D}"
        out[f"pred_{tag}"], out[f"target_{tag}"], out[f"ref_{tag}"], out[f"special_{tag}"] = pred, target, ref, special
        print(tag, "non-finite entries:", int((~np.isfinite(ref)).sum()), "of", ref.size)
        if (G, D) == (7, 89):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                m = Metrics(pred=pred.astype(np.float64), target=target.astype(np.float64))
                out[f"json_{tag}"] = np.array(m.model_dump_json())
    path = HERE / "metrics.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
