"""The float64 reference of the masked objectives (objective_cases.reference) checked without a GPU: its per-gauge
terms against the reference's own ``Metrics`` (tests/golden/metrics.npz), its closed-form gradient against float64
autograd of the same objective composed from PyTorch ops, and the equivalence with the reference loop's filter."""

import numpy as np
import pytest
import torch

import objective_cases as oc
from conftest import load_golden
from ddr_amd.train import OBJECTIVE_KINDS, daily_objective  # noqa: F401  (the feature under test is there)

GOLDEN_CASES = [(5, 1), (5, 2), (6, 3), (7, 89), (7, 100), (5, 365), (4, 1000), (3, 5479), (2, 8192), (6, 512), (6, 513)]
# Float64 autograd and the closed form differ by rounding alone: 1.1e-16 per operation, through sums of up to 8192
# terms (x 1e4 at worst) and the division by E, r - 1, alpha - 1, beta - 1 of the KGE, which these inputs keep above
# 1e-3 (x 1e3): 1e-9 of the row's largest entry is two orders above that product's typical value.
GRAD_BAR = 1e-9


def golden_terms(d: dict, tag: str) -> dict:
    names = list(d["names"])
    ref = d[f"ref_{tag}"]
    row = lambda name: ref[names.index(name)]  # noqa: E731
    return {"l1": row("mae"), "mse": row("rmse") ** 2, "nse": 1.0 - row("nse"), "kge": 1.0 - row("kge")}


@pytest.fixture(scope="module")
def golden():
    return load_golden("metrics")


def test_kinds_are_the_exported_list():
    assert tuple(OBJECTIVE_KINDS) == oc.KINDS


@pytest.mark.parametrize("G,D", GOLDEN_CASES)
def test_terms_against_reference_metrics(golden, G, D):
    """warmup 0, eps 0: l1 term = mae, mse term = rmse^2, nse term = 1 - nse, kge term = 1 - kge to
    1e-10 max(1, |ref|) (the bar of test_gpu_metrics.py), and a gauge is unused exactly where the golden value is
    NaN or +-inf."""
    tag = f"{G}x{D}"
    pred, target = golden[f"pred_{tag}"], golden[f"target_{tag}"]
    want = golden_terms(golden, tag)
    valid_days = (~np.isnan(target)).sum(1)
    for kind in oc.KINDS:
        r = oc.reference(pred, target, 0, kind)
        fin = np.isfinite(want[kind])
        assert (r["used"] == fin).all(), (kind, r["used"], want[kind])
        assert (np.isnan(r["term"]) == ~fin).all()
        assert (r["days"] == valid_days).all()
        err = np.abs(r["term"][fin] - want[kind][fin]) / np.maximum(1.0, np.abs(want[kind][fin]))
        assert (err <= 1e-10).all(), (kind, err.max())


@pytest.mark.parametrize("kind", oc.KINDS)
@pytest.mark.parametrize("G,D,warmup", [(5, 1, 0), (5, 2, 0), (7, 3, 1), (8, 89, 3), (9, 130, 40), (4, 600, 0), (3, 2000, 1999)])
def test_gradient_against_float64_autograd(kind, G, D, warmup):
    pred, target, codes = oc.make_inputs(G, D, warmup)
    variants = [dict(), dict(weight=oc.make_weights(G)), dict(drop=oc.make_drop(G)), dict(count=123.0)]
    if kind == "nse":
        variants.append(dict(eps=0.1))
    for kw in variants:
        r = oc.reference(pred, target, warmup, kind, **kw)
        p = torch.from_numpy(pred).double().requires_grad_(True)
        tkw = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        if "weight" in tkw:
            tkw["weight"] = tkw["weight"].double()
        loss = oc.torch_objective(p, torch.from_numpy(target).double(), warmup, kind, **tkw)
        if loss.requires_grad:
            loss.backward()
        got = p.grad.numpy() if p.grad is not None else np.zeros((G, D))
        assert oc.loss_error(float(loss.detach()), r["loss"]) <= 1e-12, (kw, float(loss.detach()), r["loss"])
        e, at = oc.row_error(got, r["grad"])
        assert e <= GRAD_BAR, (kw, e, at, codes[at])
        # exactly zero outside V_g and for unused gauges
        valid = ~np.isnan(target)
        valid[:, :warmup] = False
        assert not r["grad"][~valid].any() and not r["grad"][~r["used"]].any()


def test_special_rows_are_used_as_defined():
    G, D, warmup = 8, 89, 3
    pred, target, codes = oc.make_inputs(G, D, warmup)
    assert sorted(codes[1:7].tolist()) == list(range(len(oc.SPECIAL)))
    used = {k: oc.reference(pred, target, warmup, k)["used"] for k in oc.KINDS}
    by = {oc.SPECIAL[c]: g for g, c in enumerate(codes) if c >= 0}
    expect = {  # (l1 / mse, nse, kge)
        "target_all_nan": (False, False, False), "single_valid_day": (True, False, False),
        "constant_target": (True, False, False), "constant_pred": (True, True, False),
        "zero_mean_target": (True, True, False), "exact_zero_difference": (True, True, True)}
    for name, (a, b, c) in expect.items():
        g = by[name]
        assert (used["l1"][g], used["mse"][g], used["nse"][g], used["kge"][g]) == (a, a, b, c), name
    assert all(used[k][0] for k in oc.KINDS)
    # eps > 0 brings the constant target back into the NSE
    assert oc.reference(pred, target, warmup, "nse", eps=0.1)["used"][by["constant_target"]]
    # the exact zero differences: sign(0) = 0 in the L1 gradient
    g = by["exact_zero_difference"]
    zero = (pred[g] == target[g]) & (np.arange(D) >= warmup)
    assert zero.sum() == 3 and not oc.reference(pred, target, warmup, "l1")["grad"][g][zero].any()


def test_every_special_row_occurs_in_the_gpu_shapes():
    for lo, hi in ((1, oc.SHORT), (oc.SHORT + 1, oc.MAX_DAYS)):
        seen = set()
        for G, D, w in oc.SHAPES:
            if lo <= D <= hi:
                seen |= set(oc.make_inputs(G, D, w)[2].tolist())
        assert seen >= set(range(len(oc.SPECIAL))), (lo, hi, seen)


@pytest.mark.parametrize("G,D,warmup", [(9, 30, 3), (64, 89, 3)])
def test_l1_with_drop_equals_the_reference_filter(G, D, warmup):
    """drop = has_nan reproduces scripts/train.py:84-94: l1_loss over the gauges without a NaN in their window."""
    pred, target, _ = oc.make_inputs(G, D, warmup, special=False)
    target = target.copy()
    target[::2] = np.round(pred[::2] * 1.1, 1)  # half of the gauges have a full record
    has_nan = np.isnan(target).any(1)
    assert 0 < has_nan.sum() < G
    r = oc.reference(pred, target, warmup, "l1", drop=has_nan)
    p = torch.from_numpy(pred).double().requires_grad_(True)
    ref = oc.boolean_index_l1(p, torch.from_numpy(target).double(), warmup)
    ref.backward()
    assert abs(r["loss"] - ref.item()) <= 1e-14 * abs(ref.item())
    assert np.abs(r["grad"] - p.grad.numpy()).max() <= 1e-17
    assert (r["used"] == ~has_nan).all() and r["W"] == (~has_nan).sum() * (D - warmup)


def test_nothing_used_gives_zero():
    pred, target, _ = oc.make_inputs(4, 20, 2)
    for kind in oc.KINDS:
        for kw in (dict(drop=np.ones(4, bool)), dict()):
            t = target if kw else np.full_like(target, np.nan)
            r = oc.reference(pred, t, 2, kind, **kw)
            assert r["loss"] == 0.0 and not r["grad"].any() and not r["used"].any() and r["W"] == 0.0
            loss = oc.torch_objective(torch.from_numpy(pred).double().requires_grad_(True),
                                      torch.from_numpy(t).double(), 2, kind,
                                      **{k: torch.from_numpy(v) for k, v in kw.items()})
            assert float(loss) == 0.0
