"""Shared by test_objective_cases.py, test_objective_api.py, test_gpu_objective.py and test_gpu_objective_capture.py
(a helper, not a test): the masked daily objectives of ``ddr_amd.train.daily_objective`` (csrc/objective.hip) as

* ``reference`` -- R, float64 NumPy, written from the definitions in ``include/ddr_mc.h`` (loss, closed-form gradient,
  per-gauge term / days / used);
* ``torch_objective`` -- T, the same objective as a sync-free PyTorch composition (``torch.where`` masks, autograd)
  in the dtype and on the device of its inputs;

and input generators after the recipe of ``tests/golden/make_metrics_golden.py`` (a log-normal walk per gauge, the
prediction the walk times log-normal noise, the target the walk quantised to 0.1 with 10 % NaN) with special rows,
and the shape list of the GPU tests."""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

KINDS = ("l1", "mse", "nse", "kge")
SPECIAL = ("target_all_nan", "single_valid_day", "constant_target", "constant_pred", "zero_mean_target",
           "exact_zero_difference")

# dispatch of csrc/objective.hip (objective.h): a wave per gauge up to SHORT days, four gauges per workgroup; a
# workgroup per gauge above; the gradient launch writes CHUNK days of a gauge per wave
SHORT, CHUNK, GAUGES_PER_WG, MAX_DAYS = 512, 256, 4, 8192


def _warmups(D: int):
    return sorted({0, D // 3, D - 1})


def _shapes():
    out = []
    # every D at one more gauge than a workgroup holds, every warm-up
    for D in (1, 2, 3, 63, 64, 65, CHUNK, CHUNK + 1, SHORT, SHORT + 1, MAX_DAYS):
        out += [(GAUGES_PER_WG + 1, D, w) for w in _warmups(D)]
    # every G at one D of each kernel, a warm-up in between
    for G in (1, 3, 4, 1025):
        out += [(G, D, D // 3) for D in (3, 89, CHUNK + 1, SHORT + 1)]
    out += [(1025, 65, 0), (3, MAX_DAYS, MAX_DAYS - 1)]
    return sorted(set(out))


SHAPES = _shapes()


# ------------------------------------------------------------------------------------------------------- inputs


def make_inputs(G: int, D: int, warmup: int = 0, seed: int = 0, special: bool = True):
    """(pred, target, codes): (G, D) fp32 arrays and the special-row code of each gauge (index into ``SPECIAL``, -1
    ordinary).  Row 0 is ordinary; the rows after it take the special kinds in turn, starting at one that depends on
    the shape, so that a list of small shapes covers them all."""
    rng = np.random.default_rng(1_000_003 * seed + 8209 * G + 17 * D + warmup)
    walk = np.exp(rng.normal(0.0, 1.0, (G, 1)) + np.cumsum(rng.normal(0.0, 0.1, (G, D)), axis=1))
    pred = (walk * np.exp(rng.normal(0.0, 0.15, (G, D)))).astype(np.float32)
    target = np.round(walk, 1).astype(np.float32)
    target[rng.uniform(size=(G, D)) < 0.1] = np.nan
    codes = np.full(G, -1, np.int32)
    if not special:
        return pred, target, codes
    first = (G + D + warmup) % len(SPECIAL)
    for k in range(1, min(G, len(SPECIAL) + 1)):
        code = (first + k - 1) % len(SPECIAL)
        codes[k] = code
        live = np.arange(warmup, D)
        if code == 0:
            target[k] = np.nan
        elif code == 1:
            day = int(rng.integers(warmup, D))
            keep = np.float32(np.round(walk[k, day], 1))
            target[k] = np.nan
            target[k, day] = keep
        elif code == 2:
            target[k, ~np.isnan(target[k])] = np.float32(1.7)
        elif code == 3:
            pred[k] = np.float32(2.3)
        elif code == 4:
            target[k, live] = np.where(np.arange(len(live)) % 2 == 0, np.float32(1.5), np.float32(-1.5))
            if len(live) % 2:
                target[k, live[-1]] = np.float32(0.0)
        else:
            days = live[~np.isnan(target[k, live])][:3]
            target[k, days] = pred[k, days]
    return pred, target, codes


def make_weights(G: int, seed: int = 0) -> np.ndarray:
    """(G,) fp32 weights in [0.25, 4), the second gauge's (where there is one) exactly 0."""
    w = np.random.default_rng(7 + seed + G).uniform(0.25, 4.0, G).astype(np.float32)
    if G > 1:
        w[1] = 0.0
    return w


def make_drop(G: int, seed: int = 0) -> np.ndarray:
    """(G,) bool, about a third set, never all (where G > 1) and never none (where G > 2)."""
    d = np.random.default_rng(11 + seed + G).uniform(size=G) < 0.33
    if G > 1:
        d[0] = False
    if G > 2:
        d[2] = True
    return d


# ---------------------------------------------------------------------------------------------------- R, float64


def reference(daily, obs, warmup: int, kind: str, drop=None, weight=None, eps: float = 0.0, count=None) -> dict:
    """float64: ``loss``, ``grad`` (G, D), ``term`` (NaN where the gauge is not used), ``days``, ``used`` (bool) and
    the normaliser ``W``, from the fp32 inputs widened."""
    p = np.asarray(daily, np.float64)
    o = np.asarray(obs, np.float64)
    G, D = p.shape
    valid = ~np.isnan(o)
    valid[:, :warmup] = False
    if drop is not None:
        valid &= ~np.asarray(drop, bool)[:, None]
    w = np.ones(G) if weight is None else np.asarray(weight, np.float64)
    term = np.full(G, np.nan)
    days = valid.sum(1).astype(np.float64)
    used = np.zeros(G, bool)
    grad = np.zeros((G, D))  # d(term_g) / d(p) for l1, mse: of n_g term_g
    with np.errstate(all="ignore"):
        for g in range(G):
            v = valid[g]
            n = int(v.sum())
            if n == 0:
                continue
            pg, og = p[g, v], o[g, v]
            d = pg - og
            if kind == "l1":
                used[g], term[g] = True, np.abs(d).sum() / n
                gv = np.sign(d)
                gv[np.isnan(d)] = np.nan
                grad[g, v] = gv
                continue
            S = (d * d).sum()
            if kind == "mse":
                used[g], term[g] = True, S / n
                grad[g, v] = 2.0 * d
                continue
            mp, mo = pg.sum() / n, og.sum() / n
            cp, co = pg - mp, og - mo
            Spp, Soo, Spo = (cp * cp).sum(), (co * co).sum(), (cp * co).sum()
            if n < 2:
                continue
            if kind == "nse":
                if not (Soo != 0.0 or eps > 0.0):
                    continue
                den = n * (math.sqrt(Soo / n) + eps) ** 2
                used[g], term[g] = True, S / den
                grad[g, v] = 2.0 * d / den
                continue
            assert kind == "kge", kind
            if Soo == 0.0 or mo == 0.0 or Spp == 0.0:
                continue
            sp, so, rt = np.sqrt(Spp / n), np.sqrt(Soo / n), np.sqrt(Spp * Soo)
            r, al, be = Spo / rt, sp / so, mp / mo
            E = np.sqrt((r - 1.0) ** 2 + (al - 1.0) ** 2 + (be - 1.0) ** 2)
            used[g], term[g] = True, E
            if E == 0.0:
                continue
            dr = (co - r * np.sqrt(Soo / Spp) * cp) / rt
            da = cp / (n * sp * so)
            db = 1.0 / (n * mo)
            grad[g, v] = ((r - 1.0) * dr + (al - 1.0) * da + (be - 1.0) * db) / E
    per_day = kind in ("l1", "mse")
    t = np.where(used, term, 0.0)
    num = float((w * (days if per_day else 1.0) * t)[used].sum())
    W = float((w * (days if per_day else 1.0))[used].sum()) if count is None else float(count)
    if W == 0.0:
        return dict(loss=0.0, grad=np.zeros((G, D)), term=term, days=days, used=used, W=W)
    grad *= (w / W)[:, None]
    grad[~used] = 0.0
    return dict(loss=num / W, grad=grad, term=term, days=days, used=used, W=W)


# ------------------------------------------------------------------------------------- T, a PyTorch composition


def torch_objective(daily: torch.Tensor, obs: torch.Tensor, warmup: int, kind: str, drop=None, weight=None,
                    eps: float = 0.0, count=None) -> torch.Tensor:
    """The same objective from PyTorch ops in ``daily``'s dtype, without boolean indexing or a host sync:
    ``torch.where`` masks with harmless stand-ins where a gauge is not used, differentiable through autograd.
    Whether a row is constant is decided from its extremes, so that fp32 takes the same gauges as float64 does.
    (For inputs without NaN predictions.)"""
    G, D = daily.shape
    valid = ~obs.isnan()
    if warmup:
        valid = valid & (torch.arange(D, device=obs.device) >= warmup)[None, :]
    if drop is not None:
        valid = valid & ~drop[:, None]
    zero = torch.zeros((), dtype=daily.dtype, device=daily.device)
    one = torch.ones((), dtype=daily.dtype, device=daily.device)
    m = valid.to(daily.dtype)
    n = m.sum(1)
    ns = n.clamp_min(1.0)
    o = torch.where(valid, obs, zero)
    p = torch.where(valid, daily, zero)
    d = p - o
    w = torch.ones(G, dtype=daily.dtype, device=daily.device) if weight is None else weight

    def varies(x):
        # S_xx != 0 decided exactly (in fp32 the mean of a constant row is rounded, and its centred sum is not 0): the
        # counted values are not all equal
        inf = torch.full((), math.inf, dtype=x.dtype, device=x.device)
        return torch.where(valid, x, inf).amin(1) != torch.where(valid, x, -inf).amax(1)

    if kind in ("l1", "mse"):
        per_gauge = (d.abs() if kind == "l1" else d * d).sum(1)  # n_g term_g
        used = n >= 1
        num = (w * per_gauge).sum()
        den = (w * n).sum()
    else:
        mp, mo = p.sum(1) / ns, o.sum(1) / ns
        cp = torch.where(valid, p - mp[:, None], zero)
        co = torch.where(valid, o - mo[:, None], zero)
        Spp, Soo, Spo = (cp * cp).sum(1), (co * co).sum(1), (cp * co).sum(1)
        if kind == "nse":
            used = (n >= 2) & (varies(obs) | bool(eps > 0.0))
            den_g = torch.where(used, ns * (torch.sqrt(Soo / ns) + eps) ** 2, one)
            term = (d * d).sum(1) / den_g
        else:
            used = (n >= 2) & varies(obs) & (mo != 0) & varies(daily)
            Spp_s, Soo_s, mo_s = torch.where(used, Spp, one), torch.where(used, Soo, one), torch.where(used, mo, one)
            r = Spo / torch.sqrt(Spp_s * Soo_s)
            al = torch.sqrt(Spp_s / ns) / torch.sqrt(Soo_s / ns)
            be = mp / mo_s
            E2 = (r - 1.0) ** 2 + (al - 1.0) ** 2 + (be - 1.0) ** 2
            used_e = used & (E2 != 0)
            term = torch.where(used_e, torch.sqrt(torch.where(used_e, E2, one)), zero)
        num = (w * torch.where(used, term, zero)).sum()
        den = (w * used.to(daily.dtype)).sum()
    if count is not None:
        den = torch.as_tensor(count, dtype=daily.dtype, device=daily.device)
    safe = torch.where(den != 0, den, one)
    return torch.where(den != 0, num / safe, zero)


def boolean_index_l1(daily: torch.Tensor, obs: torch.Tensor, warmup: int) -> torch.Tensor:
    """The reference's form (scripts/train.py:84-94): drop the gauges whose window holds a NaN by boolean indexing
    (a host sync and a new shape), then ``l1_loss`` after the warm-up."""
    keep = ~obs.isnan().any(dim=1)
    return torch.nn.functional.l1_loss(daily[keep][:, warmup:], obs[keep][:, warmup:])


# ------------------------------------------------------------------------------------------------------- errors


def loss_error(a: float, ref: float) -> float:
    if ref == 0.0:
        return 0.0 if a == 0.0 else math.inf
    if not math.isfinite(a):
        return math.inf
    return abs(a - ref) / abs(ref)


def row_error(a, ref) -> tuple[float, int]:
    """The gradient's error per gauge row, max |a - ref| of the row over the row's largest |ref| (a row whose
    reference is identically zero must be met exactly): the worst row's value and its index."""
    a = np.asarray(a, np.float64)
    ref = np.asarray(ref, np.float64)
    assert a.shape == ref.shape and a.ndim == 2, (a.shape, ref.shape)
    worst, at = 0.0, -1
    for g in range(a.shape[0]):
        top = np.abs(ref[g]).max() if ref.shape[1] else 0.0
        if not np.isfinite(a[g]).all():
            e = math.inf
        elif top == 0.0:
            e = 0.0 if not a[g].any() else math.inf
        else:
            e = float(np.abs(a[g] - ref[g]).max() / top)
        if e > worst:
            worst, at = e, g
    return worst, at


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def case(G: int, D: int, warmup: int, kind: str, weighted: bool = False, dropped: bool = False, eps: float = 0.0):
    """Inputs and R of one case, computed once per session: (pred, target, drop, weight, R) -- read-only."""
    pred, target, _ = make_inputs(G, D, warmup)
    drop = make_drop(G) if dropped else None
    weight = make_weights(G) if weighted else None
    ref = reference(pred, target, warmup, kind, drop, weight, eps)
    for a in (pred, target, drop, weight, *(v for v in ref.values() if isinstance(v, np.ndarray))):
        if a is not None:
            a.setflags(write=False)
    return pred, target, drop, weight, ref
