"""The geometry-statistics kernels (csrc/geometry.hip) at every window length, valid count and edge.

``launch_geometry_stats`` dispatches on the day count D to eight instantiations of the wave kernel
(``<KD, KE>`` = <1,1> <2,2> <4,3> <4,4> <8,5> <8,6> <8,7> <8,8>: 64 KE days per wave) and, beyond 512 days, to
the workgroup-per-reach LDS sort.  Every case here is compared with ``oracle.geometry_statistics`` on the same
fp32 inputs:

* the NaN pattern of all 24 outputs is identical, and so is every +-inf;
* min, max and median are equal, tolerance 0;
* the mean is within 1 fp32 ulp of ``float32(fp64 mean of the oracle's fp32 per-day valid values)``: the
  kernel sums the fp32 values in fp64 and rounds once, so the two are roundings of fp64 numbers ~1e-16 apart.

The conditions a case has to meet to reach a branch of the kernel (a variable not monotone along sorted Q, a
decreasing one, valid counts at the slot boundaries, NaN geometry under a valid discharge) are asserted in the
test that needs them, from oracle values alone.
"""

import warnings

import numpy as np
import pytest
import torch

from ddr_amd import _lib
from ddr_amd.geometry.statistics import GEOMETRY_VARS, STATS, _as_dict, _stats_device, compute_geometry_statistics
from oracle import mc_oracle as O

pytestmark = pytest.mark.gpu

F = np.float32


def _params(rng, N):
    """Per-reach parameters, drawn as test_geometry_statistics_long_window draws them."""
    n = rng.uniform(0.015, 0.25, N).astype(F)
    p = rng.uniform(1.0, 200.0, N).astype(F)
    q = rng.uniform(0.0, 1.0, N).astype(F)
    slope = rng.uniform(1e-3, 0.05, N).astype(F)
    return n, p, q, slope


def _discharge(rng, D, N, nan_frac=0.01):
    qd = rng.lognormal(0.0, 3.0, (D, N)).astype(F)
    if nan_frac:
        qd[rng.random((D, N)) < nan_frac] = np.nan
    return qd


def _oracle(par, qd, mins=None):
    mins = mins or {}
    bd = O.Bounds(depth=mins.get("depth", 0.01), bottom_width=mins.get("bottom_width", 0.01))
    n, p, q, slope = par
    return O.geometry_statistics(n, np.broadcast_to(p, n.shape), q, slope, qd, bd, return_days=True)


def _kernel(par, qd, mins=None):
    n, p, q, slope = par
    return compute_geometry_statistics(torch.from_numpy(n), torch.from_numpy(np.atleast_1d(p)), torch.from_numpy(q),
                                       torch.from_numpy(slope), qd, mins)


def _mean_reference(days):
    """float32 of the fp64 mean of the valid fp32 per-day values, per variable: (N,) each."""
    out = {}
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for var in GEOMETRY_VARS:
            out[var] = np.nanmean(days[var].astype(np.float64), axis=0).astype(F)
    return out


def _compare(got, orc, days, tag):
    """The bars of the module docstring; prints the worst mean error (in ulp and relative) before asserting."""
    assert set(got) == {f"{v}_{s}" for v in GEOMETRY_VARS for s in STATS}
    means = _mean_reference(days)
    worst_ulp, worst_rel = 0.0, 0.0
    failures = []
    for var in GEOMETRY_VARS:
        for s in STATS:
            k = f"{var}_{s}"
            g, ref = got[k], (means[var] if s == "mean" else orc[k])
            assert g.dtype == F and g.shape == ref.shape, k
            if not np.array_equal(np.isnan(g), np.isnan(ref)):
                failures.append(f"{k}: NaN pattern differs at reaches {np.flatnonzero(np.isnan(g) != np.isnan(ref))[:8]}")
                continue
            inf = np.isinf(ref) | np.isinf(g)
            if not np.array_equal(g[inf], ref[inf]):
                failures.append(f"{k}: infinities differ at reaches {np.flatnonzero(inf)[:8]}")
                continue
            ok = np.isfinite(ref)
            if s != "mean":
                bad = np.flatnonzero(ok & (g != ref))
                if bad.size:
                    failures.append(f"{k}: {bad.size} reaches differ, first {bad[:5]}: got {g[bad[:5]]} want {ref[bad[:5]]}")
            elif ok.any():
                err = np.abs(g[ok].astype(np.float64) - ref[ok].astype(np.float64))
                ulp = err / np.spacing(np.abs(ref[ok])).astype(np.float64)
                rel = err / np.maximum(np.abs(ref[ok].astype(np.float64)), np.finfo(np.float64).tiny)
                worst_ulp, worst_rel = max(worst_ulp, float(ulp.max())), max(worst_rel, float(rel[err > 0].max(initial=0.0)))
                if ulp.max() > 1.0:
                    failures.append(f"{k}: mean {ulp.max():.1f} ulp ({rel.max():.2e} relative) from the fp64 mean")
    print(f"geostats {tag}: worst mean error {worst_ulp:.0f} ulp, {worst_rel:.2e} relative")
    assert not failures, (tag, failures)


def _run(par, qd, tag, mins=None):
    orc, days = _oracle(par, qd, mins)
    _compare(_kernel(par, qd, mins), orc, days, tag)
    return orc, days


def _monotonicity(days):
    """Per reach and variable, along the reach's valid days in ascending discharge: (non-decreasing,
    non-increasing, decreasing), each (6, N) bool.  Decreasing is never rising and falling at least once -- what
    sends the kernel to its mirrored positions; a side slope that falls onto its bound and stays there
    counts, a constant does not.  Only reaches whose six variables are valid on every valid-discharge day
    are classified (others are False everywhere: they take the kernel's NaN fallback)."""
    Q = days["discharge"]
    D, N = Q.shape
    inc = np.zeros((len(GEOMETRY_VARS), N), bool)
    dec = np.zeros_like(inc)
    sdec = np.zeros_like(inc)
    for r in range(N):
        valid = np.flatnonzero(~np.isnan(Q[:, r]))
        order = valid[np.argsort(Q[valid, r], kind="stable")]
        if order.size < 3 or any(np.isnan(days[v][order, r]).any() for v in GEOMETRY_VARS):
            continue
        for i, v in enumerate(GEOMETRY_VARS):
            d = np.diff(days[v][order, r].astype(np.float64))
            inc[i, r], dec[i, r], sdec[i, r] = (d >= 0).all(), (d <= 0).all(), (d <= 0).all() and (d < 0).any()
    return inc, dec, sdec


# ---- every instantiation and its boundaries -----------------------------------------------------

WAVE_D = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 365, 366, 383, 384, 385, 447,
          448, 449, 511, 512]


@pytest.mark.parametrize("D", WAVE_D)
def test_every_instantiation_and_boundary(cuda, D):
    """131 reaches (33 groups: more than one per XCD, the last one partial) x D days at both sides of every
    64-day slot boundary, 1 % NaN days.  From 33 days on the inputs reach all three branches of the order
    statistics: the fixed positions of an increasing variable, the mirrored ones of a decreasing variable, and
    the sort of a variable that is neither."""
    rng = np.random.default_rng(47000 + D)  # (a seed base at which every D meets the three conditions below)
    N = 131
    par = _params(rng, N)
    qd = _discharge(rng, D, N)
    orc, days = _run(par, qd, f"D={D}")
    if D >= 33:
        inc, dec, sdec = _monotonicity(days)
        neither = (~inc & ~dec).any(axis=0) & (inc | dec).any(axis=0)  # (classified reaches only)
        print(f"geostats D={D}: {neither.sum()} reaches with a non-monotone variable, {sdec.any(axis=0).sum()} with a "
              f"decreasing one, {inc.all(axis=0).sum()} all non-decreasing")
        assert neither.sum() >= 5
        assert sdec.any(axis=0).sum() >= 50
        assert inc.all(axis=0).sum() >= 5


# ---- valid-count edges ---------------------------------------------------------------------------


@pytest.mark.parametrize("D", [129, 365, 512])
def test_valid_count_edges(cuda, D):
    """Reaches with exactly c valid days at random positions, c at 0, the first values, both sides of the
    64-day slot boundaries (the wave-uniform skip of a slot without a valid day) and the window's end; a constant
    reach (every pair a tie: both monotone flags hold), a reach of two repeated values, and a reach whose valid
    days are all in the last slot."""
    rng = np.random.default_rng(8000 + D)
    counts = sorted({c for c in (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, D - 1, D) if c <= D})
    extra = 3
    N = len(counts) + extra + 6  # and six plain reaches
    par = _params(rng, N)
    qd = _discharge(rng, D, N, nan_frac=0.0)
    for r, c in enumerate(counts):
        qd[rng.permutation(D)[c:], r] = np.nan
    k = len(counts)
    qd[:, k] = F(3.25)
    qd[:, k + 1] = np.where(rng.random(D) < 0.5, F(0.75), F(41.0)).astype(F)
    last = 64 * ((D - 1) // 64)
    qd[:last, k + 2] = np.nan
    orc, days = _run(par, qd, f"counts D={D}")
    valid = (~np.isnan(days["discharge"])).sum(axis=0)
    assert list(valid[:k]) == counts
    for v in GEOMETRY_VARS:  # the counts hold for every variable: no NaN geometry on a valid day here
        assert np.array_equal((~np.isnan(days[v])).sum(axis=0), valid), v
        assert len(np.unique(days[v][:, k])) == 1
        assert np.isnan(orc[f"{v}_min"][0]) and orc[f"{v}_min"][1] == orc[f"{v}_max"][1]
    assert len(np.unique(days["discharge"][:, k + 1])) == 2
    assert valid[k + 2] == D - last and not np.isnan(days["discharge"][last:, k + 2]).any()


# ---- NaN geometry under a valid discharge -------------------------------------------------------


@pytest.mark.parametrize("D", [65, 365, 449])
def test_variables_nan_where_discharge_is_valid(cuda, D):
    """A negative discharge is a valid discharge with NaN geometry (a negative base under a fractional exponent),
    so the five geometry variables count fewer valid days than the sort of Q placed: the kernel's cnt != cq
    fallback.  Zero days sit on the depth bound; a +inf day has infinite depth and top width and NaN side slope,
    bottom width and hydraulic radius.  The oracle defines every value (tests/golden/geostats_edges.npz pins
    it to the reference on these classes)."""
    rng = np.random.default_rng(9000 + D)
    N = 131
    par = _params(rng, N)
    qd = _discharge(rng, D, N)
    for r in range(0, N, 3):
        d = rng.choice(D, int(rng.integers(1, D // 2 + 1)), replace=False)
        qd[d, r] = -np.abs(qd[d, r])
    qd[rng.random((D, N)) < 0.01] = 0.0
    qd[:, 10] = -rng.lognormal(0.0, 1.0, D).astype(F)  # valid discharge, no valid geometry at all
    qd[:, 11] = 0.0
    inf_reaches = (4, 12, 21, 130)
    for r in inf_reaches:
        qd[int(rng.integers(D)), r] = np.inf
    orc, days = _run(par, qd, f"nan-under-valid D={D}")
    vq = (~np.isnan(days["discharge"])).sum(axis=0)
    vd = (~np.isnan(days["depth"])).sum(axis=0)
    neg = (days["discharge"] < 0).sum(axis=0)
    assert np.array_equal(vq - vd, neg) and (neg > 0).sum() >= N // 4 and (neg == 0).sum() >= N // 4
    assert vd[10] == 0 and vq[10] == D and np.isnan(orc["depth_mean"][10]) and orc["discharge_max"][10] < 0
    assert (days["discharge"] == 0).sum() >= D and (orc["depth_min"][11] == F(0.01))
    for r in inf_reaches:
        assert np.isposinf(orc["depth_max"][r]) and np.isposinf(orc["top_width_mean"][r])
        assert (~np.isnan(days["side_slope"][:, r])).sum() < vd[r]


# ---- launch geometry ----------------------------------------------------------------------------


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 31, 33])
def test_fewer_groups_than_workgroups(cuda, N):
    """Fewer groups of four reaches than the eight-workgroup minimum, XCD spans that are empty, and a last
    group of 1, 2 or 3 reaches (D = 65: two slots, the second with one day)."""
    rng = np.random.default_rng(10000 + N)
    _run(_params(rng, N), _discharge(rng, 65, N), f"N={N}")


def test_persistent_workgroups_walk_several_groups(cuda):
    """40001 reaches are 10001 groups; at most 8 workgroups of 256 threads x 256 CUs = 2048 are resident, so
    every workgroup walks at least 4 groups (and the last group holds one reach)."""
    rng = np.random.default_rng(10500)
    N = 40001
    assert (N + 3) // 4 >= 4 * 2048 and N % 4 == 1
    _run(_params(rng, N), _discharge(rng, 65, N), f"N={N}")


def test_reach_permutation_permutes_rows(cuda):
    """The four waves of a workgroup work on four reaches independently: permuting the reaches permutes the
    24 output rows bitwise."""
    rng = np.random.default_rng(10600)
    N, D = 131, 257
    n, p, q, slope = _params(rng, N)
    qd = _discharge(rng, D, N)
    perm = rng.permutation(N)
    assert not np.array_equal(perm // 4, np.arange(N) // 4)
    a = _kernel((n, p, q, slope), qd)
    b = _kernel((n[perm], p[perm], q[perm], slope[perm]), np.ascontiguousarray(qd[:, perm]))
    for k in a:
        assert np.array_equal(a[k][perm].view(np.uint32), b[k].view(np.uint32)), k


# ---- layout and arguments -----------------------------------------------------------------------


@pytest.mark.parametrize("D", [129, 365, 1025])
def test_reach_major_layout_equals_day_major(cuda, D):
    """geometry_statistics_from_inflow hands the kernel a reach-major (N, D) discharge (strides D, 1);
    compute_geometry_statistics a day-major one (strides 1, N): the same bits, and the oracle's values."""
    rng = np.random.default_rng(11000 + D)
    N = 37
    par = _params(rng, N)
    qd = _discharge(rng, D, N)
    orc, days = _oracle(par, qd)
    dev_q = torch.from_numpy(qd).to(cuda)
    day_major = _stats_device(dev_q, 1, N, N, D, *par, 0.01, 0.01)
    reach_major = _stats_device(dev_q.T.contiguous(), D, 1, N, D, *par, 0.01, 0.01)
    assert torch.equal(day_major.view(torch.int32), reach_major.view(torch.int32))
    _compare(_as_dict(reach_major), orc, days, f"reach-major D={D}")


@pytest.mark.parametrize("D", [65, 365, 600])
def test_scalar_p_spatial(cuda, D):
    """A one-element p_spatial (stride 0) is the same p for every reach."""
    rng = np.random.default_rng(11500 + D)
    n, _, q, slope = _params(rng, 29)
    _run((n, F(21.0), q, slope), _discharge(rng, D, 29), f"scalar p D={D}")


@pytest.mark.parametrize("D", [129, 365, 600])
def test_attribute_minimums_make_tie_runs(cuda, D):
    """depth >= 0.5 and bottom_width >= 0.1: the low-flow days of a reach share the depth bound (and everything
    computed from it), long runs of ties along sorted Q."""
    rng = np.random.default_rng(12000 + D)
    N = 61
    mins = {"depth": 0.5, "bottom_width": 0.1}
    orc, days = _run(_params(rng, N), _discharge(rng, D, N), f"minimums D={D}", mins)
    on_bound = (days["depth"] == F(0.5)).sum(axis=0)
    assert (on_bound >= D // 4).sum() >= N // 2 and (orc["depth_min"] >= F(0.5)).all()
    assert (days["bottom_width"] == F(0.1)).any() and (orc["bottom_width_min"] >= F(0.1)).all()


# ---- long windows -------------------------------------------------------------------------------


def _long_case(D):
    rng = np.random.default_rng(13000 + D)
    N = 5
    par = _params(rng, N)
    qd = _discharge(rng, D, N)
    qd[:, 1] = np.nan  # a reach without a valid day
    d = rng.choice(D, D // 3, replace=False)
    qd[d, 3] = -np.abs(qd[d, 3])
    return par, qd


@pytest.mark.parametrize("D", [1023, 1024, 1025, 2048, 2049, 32768])
def test_long_window_boundaries(cuda, D):
    """The LDS sort over P = the next power of two >= D: P exactly full (1024, 2048), one short (1023), just
    exceeded (1025, 2049) and the documented cap of 32768 days; 1 % NaN days, an all-NaN reach and a reach with
    negative days."""
    par, qd = _long_case(D)
    orc, days = _run(par, qd, f"long D={D}")
    assert np.isnan(days["discharge"][:, 1]).all() and np.isnan(orc["discharge_mean"][1])
    assert (days["discharge"][:, 3] < 0).sum() >= D // 4
    assert (~np.isnan(days["depth"][:, 3])).sum() < (~np.isnan(days["discharge"][:, 3])).sum()


@pytest.mark.parametrize("D", [32769, 0])
def test_day_count_outside_the_window_is_refused(cuda, D):
    rng = np.random.default_rng(14000)
    par = _params(rng, 5)
    with pytest.raises(_lib.DDRError) as e:
        _kernel(par, np.ones((D, 5), F))
    assert e.value.code == _lib.DDR_ERR_ARG
