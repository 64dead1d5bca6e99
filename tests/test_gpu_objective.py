"""GPU checks of the masked daily objectives (ddr_amd.train.daily_objective, csrc/objective.hip): the kernels K
against the float64 reference R of objective_cases.py.

Error rule: the project's own, ``tail_cases.bound(err(T, R), 1e-6)`` with ``tail_cases.MARGIN``, T the same objective
composed from PyTorch fp32 ops on the device (``objective_cases.torch_objective``).  It applies to the loss (relative)
and to the gradient per gauge row: the max-abs error of the row over the row's largest reference entry, the worst row
reported -- a large river's small gradients are not hidden behind a small one's.  Where T's error is not finite the
bound is the fixed 1e-6.  The loss also keeps |K - R| <= 1e-6 |R| (the bar of test_daily_l1_against_float64).  K forms
every element in fp64 and rounds once, so its error is expected near one fp32 ulp (6e-8).

Shapes (objective_cases.SHAPES): G in {1, 3, 4, 5, 1025} -- 5 is one more than the four gauges of a workgroup --; D in
{1, 2, 3, 63, 64, 65}, both sides of every dispatch boundary -- 512 | 513 (a wave | a workgroup per gauge), 256 | 257
and 513 (one | two | three chunks of the gradient launch) -- and 8192; warm-up 0, D // 3 and D - 1.

Measured on an MI355X, worst case of SHAPES per kind, err(T, R) / err(K, R):
l1: loss 1.337e-07 / 5.926e-08; gradient rows 5.122e-08 / 5.122e-08
mse: loss 1.315e-07 / 4.668e-08; gradient rows 1.185e-07 / 5.846e-08
nse: loss 2.695e-07 / 5.307e-08; gradient rows 4.147e-07 / 5.887e-08
kge: loss 3.249e-06 / 4.638e-08; gradient rows 1.984e-05 / 5.900e-08
(worst cases: T's KGE loss at 5 x 8192, its KGE rows at 1025 x 513; K's all near one fp32 rounding, 6e-8, as expected.
On 3000 x 5113 series T's KGE loss is 3.4e-2 off its float64 value, K's 3e-9: tools/objective_time.py.)
"""

import numpy as np
import pytest
import torch

import objective_cases as oc
import tail_cases as tc
from conftest import load_golden
from ddr_amd.train import daily_l1_loss, daily_objective

pytestmark = pytest.mark.gpu

FIXED = 1e-6
GOLDEN_CASES = [(5, 1), (5, 2), (6, 3), (7, 89), (7, 100), (5, 365), (4, 1000), (3, 5479), (2, 8192), (6, 512), (6, 513)]


def dev(a, cuda):
    return None if a is None else torch.tensor(np.asarray(a)).to(cuda)


def run_k(cuda, pred, target, warmup, kind, drop=None, weight=None, eps=0.0, count=None, upstream=None):
    """K on the device: (loss, grad, ObjectiveTerms as NumPy) of one call + backward."""
    p = dev(pred, cuda).requires_grad_(True)
    loss, t = daily_objective(p, dev(target, cuda), warmup, kind, drop=dev(drop, cuda), weight=dev(weight, cuda),
                              eps=eps, count=count, terms=True)
    assert loss.shape == () and loss.dtype == torch.float32
    (loss if upstream is None else loss * upstream).backward()
    assert p.grad.shape == p.shape
    return loss.item(), p.grad.cpu().numpy(), {k: getattr(t, k).cpu().numpy() for k in ("term", "days", "used")}


def run_t(cuda, pred, target, warmup, kind, drop=None, weight=None, eps=0.0, count=None):
    p = dev(pred, cuda).requires_grad_(True)
    loss = oc.torch_objective(p, dev(target, cuda), warmup, kind, drop=dev(drop, cuda), weight=dev(weight, cuda),
                              eps=eps, count=count)
    if loss.requires_grad:
        loss.backward()
    return loss.item(), (p.grad.cpu().numpy() if p.grad is not None else np.zeros(pred.shape, np.float32))


def limit(t: float) -> float:
    return tc.bound(t, FIXED) if np.isfinite(t) else FIXED


def check_against_reference(cuda, pred, target, warmup, kind, ref, label, **kw):
    """The error rule, the exact zeros and the terms of one case; returns the four errors."""
    tl, tg = run_t(cuda, pred, target, warmup, kind, **kw)
    kl, kg, terms = run_k(cuda, pred, target, warmup, kind, **kw)
    etl, ekl = oc.loss_error(tl, ref["loss"]), oc.loss_error(kl, ref["loss"])
    (etg, _), (ekg, at) = oc.row_error(tg, ref["grad"]), oc.row_error(kg, ref["grad"])
    print(f"objective {label} {kind}: loss T {etl:.3e} K {ekl:.3e}; grad rows T {etg:.3e} K {ekg:.3e} (row {at})")
    assert ekl <= limit(etl), (label, kind, "loss", etl, ekl)
    assert abs(kl - ref["loss"]) <= 1e-6 * abs(ref["loss"]), (label, kind, kl, ref["loss"])
    assert ekg <= limit(etg), (label, kind, "grad", etg, ekg, at)
    # exactly +0.0 before the warm-up, on missing days, on dropped and unused gauges
    valid = ~np.isnan(target)
    valid[:, :warmup] = False
    if kw.get("drop") is not None:
        valid &= ~kw["drop"][:, None]
    valid &= ref["used"][:, None]
    assert not oc.bits(kg)[~valid].any(), (label, kind)
    assert (terms["used"] == ref["used"]).all() and (terms["days"] == ref["days"]).all(), (label, kind)
    assert (np.isnan(terms["term"]) == ~ref["used"]).all()
    u = ref["used"]
    assert (np.abs(terms["term"][u] - ref["term"][u]) <= 1e-10 * np.maximum(1.0, np.abs(ref["term"][u]))).all()
    return etl, ekl, etg, ekg


@pytest.mark.parametrize("G,D,warmup", oc.SHAPES)
def test_against_float64(cuda, G, D, warmup):
    for kind in oc.KINDS:
        pred, target, _, _, ref = oc.case(G, D, warmup, kind)
        check_against_reference(cuda, pred, target, warmup, kind, ref, f"{G}x{D} w{warmup}")


@pytest.mark.parametrize("G,D,warmup", [(5, 89, 3), (6, 513, 171), (1025, 65, 0)])
def test_weights_drop_eps_and_count_against_float64(cuda, G, D, warmup):
    for kind in oc.KINDS:
        for weighted, dropped in ((True, False), (False, True), (True, True)):
            pred, target, drop, weight, ref = oc.case(G, D, warmup, kind, weighted, dropped)
            check_against_reference(cuda, pred, target, warmup, kind, ref, f"{G}x{D} weighted={weighted} "
                                    f"dropped={dropped}", drop=drop, weight=weight)
            if weighted and not dropped and ref["used"][1]:
                # weight 0: the gauge is used (its term is reported) but has no influence
                kl, kg, terms = run_k(cuda, pred, target, warmup, kind, weight=weight)
                assert weight[1] == 0.0 and terms["used"][1] == 1.0 and not kg[1].any()
                w2 = weight.copy()
                w2[1] = 0.0
                p2 = pred.copy()
                p2[1] *= 3.0
                kl2, kg2, _ = run_k(cuda, p2, target, warmup, kind, weight=w2)
                assert kl2 == kl and (oc.bits(np.delete(kg2, 1, 0)) == oc.bits(np.delete(kg, 1, 0))).all()
    pred, target, _, _, _ = oc.case(G, D, warmup, "nse")
    ref = oc.reference(pred, target, warmup, "nse", eps=0.25)
    check_against_reference(cuda, pred, target, warmup, "nse", ref, f"{G}x{D} eps=0.25", eps=0.25)
    for kind in oc.KINDS:
        ref = oc.reference(pred, target, warmup, kind, count=777.0)
        check_against_reference(cuda, pred, target, warmup, kind, ref, f"{G}x{D} count=777", count=777.0)


@pytest.mark.parametrize("G,D", GOLDEN_CASES)
def test_terms_against_reference_metrics(cuda, G, D):
    """``terms`` against the reference's own Metrics (tests/golden/metrics.npz): l1 = mae, mse = rmse^2, nse = 1 - nse,
    kge = 1 - kge to 1e-10 max(1, |ref|); unused exactly where the golden value is NaN or +-inf."""
    d = load_golden("metrics")
    tag = f"{G}x{D}"
    names = list(d["names"])
    row = lambda name: d[f"ref_{tag}"][names.index(name)]  # noqa: E731
    want = {"l1": row("mae"), "mse": row("rmse") ** 2, "nse": 1.0 - row("nse"), "kge": 1.0 - row("kge")}
    pred, target = dev(d[f"pred_{tag}"], cuda), dev(d[f"target_{tag}"], cuda)
    for kind in oc.KINDS:
        _, t = daily_objective(pred, target, 0, kind, terms=True)
        term, used = t.term.cpu().numpy(), t.used.cpu().numpy()
        fin = np.isfinite(want[kind])
        assert (used == fin).all() and (np.isnan(term) == ~fin).all(), (kind, used, want[kind])
        assert (t.days.cpu().numpy() == (~np.isnan(d[f"target_{tag}"])).sum(1)).all()
        err = np.abs(term[fin] - want[kind][fin]) / np.maximum(1.0, np.abs(want[kind][fin]))
        assert (err <= 1e-10).all(), (kind, err.max())


@pytest.mark.parametrize("G,D,warmup", [(5, 89, 3), (3, 600, 0)])
def test_nothing_used(cuda, G, D, warmup):
    """W = 0 -- every gauge dropped, or every observation NaN: the loss is 0 and the gradient +0.0."""
    pred, target, _ = oc.make_inputs(G, D, warmup)
    for kind in oc.KINDS:
        for t, drop in ((target, np.ones(G, bool)), (np.full_like(target, np.nan), None)):
            kl, kg, terms = run_k(cuda, pred, t, warmup, kind, drop=drop)
            assert kl == 0.0 and not oc.bits(kg).any() and not terms["used"].any() and not terms["days"].any()
            assert np.isnan(terms["term"]).all()


@pytest.mark.parametrize("G,D,warmup", [(4, 256, 1), (256, 89, 3), (37, 600, 4)])
def test_l1_agrees_with_daily_l1_loss(cuda, G, D, warmup):
    """Nothing missing, no weights, no drop: the gradient bits are ``daily_l1_loss``'s, also under an upstream factor
    of 3; the loss agrees to 1e-6."""
    daily, obs = tc.l1_inputs(G, D, warmup)
    for upstream in (None, 3.0):
        a = daily.to(cuda).requires_grad_(True)
        la = daily_l1_loss(a, obs.to(cuda), warmup)
        (la if upstream is None else la * upstream).backward()
        kl, kg, _ = run_k(cuda, daily.numpy(), obs.numpy(), warmup, "l1", upstream=upstream)
        assert (oc.bits(kg) == oc.bits(a.grad.cpu().numpy())).all()
        assert abs(kl - la.item()) <= 1e-6 * abs(la.item())


@pytest.mark.parametrize("G,D,warmup", [(9, 89, 3), (6, 129, 5), (7, 700, 0)])
def test_drop_equals_physical_filtering(cuda, G, D, warmup):
    """With ``drop=mask`` the gradient rows of the kept gauges are bit-identical to a call on ``daily[keep]``,
    ``obs[keep]``; the loss agrees to 1e-6 relative (its sum runs over other positions)."""
    pred, target, _ = oc.make_inputs(G, D, warmup)
    drop = oc.make_drop(G)
    keep = ~drop
    assert 0 < keep.sum() < G
    for kind in oc.KINDS:
        ml, mg, mt = run_k(cuda, pred, target, warmup, kind, drop=drop)
        fl, fg, ft = run_k(cuda, pred[keep], target[keep], warmup, kind)
        assert (oc.bits(mg[keep]) == oc.bits(fg)).all(), kind
        assert not oc.bits(mg[drop]).any()
        assert abs(ml - fl) <= 1e-6 * abs(fl), (kind, ml, fl)
        assert (mt["used"][keep] == ft["used"]).all() and not mt["used"][drop].any()
        assert (oc.bits(mt["term"][keep].astype(np.float32)) == oc.bits(ft["term"].astype(np.float32))).all()
    # drop = has_nan is the reference loop's filter (scripts/train.py:84-94)
    t2 = target.copy()
    t2[::2] = np.round(pred[::2] * 1.1, 1)
    has_nan = np.isnan(t2).any(1)
    ml, mg, _ = run_k(cuda, pred, t2, warmup, "l1", drop=has_nan)
    p = dev(pred, cuda).requires_grad_(True)
    ref = oc.boolean_index_l1(p, dev(t2, cuda), warmup)
    ref.backward()
    assert abs(ml - ref.item()) <= 1e-6 * abs(ref.item())
    assert oc.row_error(mg, p.grad.double().cpu().numpy())[0] <= FIXED and not oc.bits(mg[has_nan]).any()


def test_count_by_value_and_by_pointer(cuda):
    G, D, warmup = 6, 89, 3
    pred, target, _ = oc.make_inputs(G, D, warmup)
    for kind in oc.KINDS:
        vl, vg, _ = run_k(cuda, pred, target, warmup, kind, count=1234.0)
        count = torch.tensor(1234.0, device=cuda)
        pl, pg, _ = run_k(cuda, pred, target, warmup, kind, count=count)
        assert oc.bits(vl) == oc.bits(pl) and (oc.bits(vg) == oc.bits(pg)).all()
        count.fill_(617.0)  # read at launch time: the same tensor, a new value
        hl, hg, _ = run_k(cuda, pred, target, warmup, kind, count=count)
        ref = oc.reference(pred, target, warmup, kind, count=617.0)
        assert abs(hl - ref["loss"]) <= 1e-6 * abs(ref["loss"]) and oc.row_error(hg, ref["grad"])[0] <= FIXED


@pytest.mark.parametrize("D", [89, 600])
def test_nan_prediction(cuda, D):
    """A NaN prediction on a counted day: the loss is NaN, the gradient NaN at that element at least (kge: possibly
    the gauge's row), every other gauge's row bit-identical to the clean run.  On a missing day, inside the warm-up or
    on a dropped gauge it changes nothing."""
    G, warmup = 6, 3
    pred, target, _ = oc.make_inputs(G, D, warmup, special=False)
    target = target.copy()
    target[2, 40] = 1.0
    target[2, 41] = np.nan
    drop = np.zeros(G, bool)
    drop[4] = True
    others = np.arange(G) != 2
    for kind in oc.KINDS:
        cl, cg, ct = run_k(cuda, pred, target, warmup, kind, drop=drop)
        assert np.isfinite(cl) and np.isfinite(cg).all()
        bad = pred.copy()
        bad[2, 40] = np.nan
        nl, ng, nt = run_k(cuda, bad, target, warmup, kind, drop=drop)
        assert np.isnan(nl) and np.isnan(ng[2, 40]), kind
        assert (oc.bits(ng[others]) == oc.bits(cg[others])).all(), kind
        assert (nt["used"] == ct["used"]).all() and (nt["days"] == ct["days"]).all()
        if kind != "kge":
            rest = np.arange(D) != 40
            assert (oc.bits(ng[2, rest]) == oc.bits(cg[2, rest])).all(), kind
        for at in ((2, 41), (2, warmup - 1), (4, 40)):
            quiet = pred.copy()
            quiet[at] = np.nan
            ql, qg, _ = run_k(cuda, quiet, target, warmup, kind, drop=drop)
            assert oc.bits(ql) == oc.bits(cl) and (oc.bits(qg) == oc.bits(cg)).all(), (kind, at)


@pytest.mark.parametrize("G,D,warmup", [(256, 89, 3), (5, 513, 0), (1025, 257, 7)])
def test_repeatable(cuda, G, D, warmup):
    pred, target, _ = oc.make_inputs(G, D, warmup)
    weight = oc.make_weights(G)
    for kind in oc.KINDS:
        al, ag, at = run_k(cuda, pred, target, warmup, kind, weight=weight)
        bl, bg, bt = run_k(cuda, pred, target, warmup, kind, weight=weight)
        assert oc.bits(al) == oc.bits(bl) and (oc.bits(ag) == oc.bits(bg)).all()
        for k in at:
            assert (at[k].view(np.int64) == bt[k].view(np.int64)).all(), (kind, k)


def test_interfaces(cuda):
    """Strided views, a transposed leaf, a call without a gradient and without terms: as test_daily_l1_interfaces."""
    G, D, warmup = 37, 53, 4
    pred, target, _ = oc.make_inputs(G, D, warmup)
    obs_d = dev(target, cuda)
    for kind in oc.KINDS:
        bl, bg, _ = run_k(cuda, pred, target, warmup, kind)
        # no gradient wanted: the same loss, no terms
        base = daily_objective(dev(pred, cuda), obs_d, warmup, kind)
        assert isinstance(base, torch.Tensor) and not base.requires_grad and oc.bits(base.item()) == oc.bits(bl)
        # row-strided views of wider buffers (innermost stride 1: read in place)
        wide_p = torch.full((G, D + 20), float("nan"), device=cuda)
        wide_o = torch.full((G, D + 7), 5.0, device=cuda)
        wide_p[:, 5:5 + D] = dev(pred, cuda)
        wide_o[:, 7:] = obs_d
        leaf = wide_p.requires_grad_(True)
        loss = daily_objective(leaf[:, 5:5 + D], wide_o[:, 7:], warmup, kind)
        loss.backward()
        assert oc.bits(loss.item()) == oc.bits(bl)
        got = leaf.grad.cpu().numpy()
        assert (oc.bits(got[:, 5:5 + D]) == oc.bits(bg)).all() and not got[:, :5].any() and not got[:, 5 + D:].any()
        # a transposed view as the leaf: the gradient arrives in its layout
        dt = dev(np.ascontiguousarray(pred.T), cuda).t().requires_grad_(True)
        assert dt.shape == (G, D) and not dt.is_contiguous() and dt.is_leaf
        loss = daily_objective(dt, dev(np.ascontiguousarray(target.T), cuda).t(), warmup, kind)
        loss.backward()
        assert oc.bits(loss.item()) == oc.bits(bl) and (oc.bits(dt.grad.cpu().numpy()) == oc.bits(bg)).all()
        # ... and a transposed view of a leaf
        leaf = dev(np.ascontiguousarray(pred.T), cuda).requires_grad_(True)  # (D, G)
        daily_objective(leaf.t(), obs_d, warmup, kind).backward()
        assert (oc.bits(leaf.grad.cpu().numpy()) == oc.bits(bg.T)).all()
