"""The parameter box of tests/physics_box.py on the CPU: that the box is what the device tests take it for (every
clamp and both negative coefficients well populated, the edge planes on their targets, the two exclusion masks
small), that the checker -- the fp64 oracle's hand adjoint -- equals autograd over the whole box, and that the
committed reduction tables of the fp32 pow (ddr_amd/csrc/mathtab.h) are what fastmath.h says they are.

Census of the box, share of the 60 000 points (fp32 evaluation; isolated / chains differ only in x < q_lb):

             depth  ss low  ss high  bw     v low  v high  x1 < q_lb     q' < q_lb  c1 < 0  c3 < 0
  default    0.098  0.228   0.158    0.149  0.026  0.040   0.394 / 0.350  0.201      0.290   0.553
  mock       0.095  0.228   0.158    0.196  0.240  0.040   0.423 / 0.361  0.300      0.255   0.589

Pow-tie mask: 0 points.  Near-bound mask: 1.2e-4 to 3.2e-4 of the 50 500 sampled points (the chains mask a pair as a
unit); the 1 500 points of the pw planes sit on depth_lb by construction and are all masked (2.7 % with them).
"""

import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import physics_box as PB

ROOT = Path(__file__).resolve().parents[1]
MATHTAB = ROOT / "ddr_amd" / "csrc" / "mathtab.h"
CASES = [(p, g) for p in PB.PARAMS for g in PB.GRAPHS]
f32 = np.float32


@pytest.mark.parametrize("pname", list(PB.PARAMS))
def test_edge_planes_are_on_their_targets(pname):
    b = PB.box(pname)
    assert b.n.shape == (PB.N,) and all(getattr(b, k).dtype == f32 for k in PB.FIELDS)
    for k in PB.FIELDS:
        lo, hi = PB.RANGES[k]
        v = getattr(b, k)
        assert v.min() >= f32(lo) and v.max() <= f32(hi), k
    pl = b.planes
    assert all(s.stop - s.start >= 500 and s.start % 2 == 0 for s in pl.values())
    assert b.interior.stop == min(s.start for s in pl.values()) and b.interior.stop + b.n_edge == PB.N
    for name, key, val in (("q0", "q", 0.0), ("q1", "q", 1.0), ("p_lo", "p", 1.0 + 1e-6), ("p_hi", "p", 200.0),
                           ("n_lo", "n", 0.015), ("n_hi", "n", 0.25), ("slope_lo", "slope", 1e-4),
                           ("slope_hi", "slope", 1.0), ("X0", "X", 0.0), ("X_half", "X", 0.5),
                           ("Q_qlb", "Q", b.bounds.discharge)):
        assert np.all(getattr(b, key)[pl[name]] == f32(val)), name
    d = PB.reference(pname, "isolated").s32["d"]
    for k in range(-2, 3):
        r = d["ratio"][pl[f"ratio_{k:+d}"]]
        m, e = np.frexp(PB._ulps(r, -k))
        assert np.all(m == 0.5), k                      # k ulp from a power of two
        assert np.sum(e == 1) >= 50                     # ... of 1 itself
        assert len(np.unique(e)) >= 10
    for k in range(-1, 2):
        assert np.all(d["pw"][pl[f"pw_{k:+d}"]] == PB._ulps(np.full(1, f32(b.bounds.depth)), k)[0]), k


@pytest.mark.parametrize("pname,graph", CASES)
def test_box_preconditions(pname, graph):
    """All seven clamps (the routed state's and q' one's counted separately), c1 < 0 and c3 < 0 each on at least 1 %
    of the points; the pow-tie mask on at most 1e-5 of them; the near-bound mask on at most 1e-3 of the sampled
    points (the planes built onto a bound are masked by design).  The two caps are conditions of the seed."""
    ref = PB.reference(pname, graph)
    cen = ref.census()
    print(pname, graph, {k: round(float(v), 4) for k, v in cen.items()})
    for k, v in cen.items():
        assert v >= 0.01, (k, v)
    tie, near = float(ref.tie.mean()), float(ref.near[ref.box.interior].mean())
    print(f"{pname} {graph}: pow-tie {tie:.2e}, near-bound (sampled) {near:.2e}, (all) {ref.near.mean():.2e}")
    assert tie <= 1e-5
    assert near <= 1e-3
    # what the forward comparisons divide by never vanishes, and the references are finite
    assert np.all(ref.s64["scale"] > 0) and np.all(np.isfinite(ref.s32["x1"])) and np.all(np.isfinite(ref.s64["x1"]))


@pytest.mark.parametrize("pname,graph", CASES)
def test_oracle_adjoint_equals_autograd_on_the_box(pname, graph):
    """The checker, checked: ``O.route_backward`` against torch's fp64 autograd of T's formulas (the reference's
    own geometry function and Muskingum step), every element of dL/d(n, q, p, Q0, q') to 1e-9 relative outside the
    near-bound mask, exact zeros equal (a velocity-clamped reach, a routed state below q_lb, q' below q_lb).
    The forwards agree to 1e-12 of the scale that does not cancel."""
    ref = PB.reference(pname, graph)
    t64 = PB.torch_step(ref.box, graph, "float64")
    s = ref.s64
    assert np.max(np.abs(t64["x1"] - s["x1"]) / s["scale"]) <= 1e-12
    for k in ("top_width", "side_slope"):
        assert np.max(np.abs(t64[k] / s["fw"][k] - 1.0)) <= 1e-12, k
    keep = ~ref.near
    for k, v in ref.vjp64.items():
        g = t64[k]
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(g)), k
        assert np.array_equal(g[keep] == 0.0, v[keep] == 0.0), k
        nz = keep & (v != 0.0)
        assert nz.mean() >= 0.3, k
        err = float(np.max(np.abs(g[nz] - v[nz]) / np.abs(v[nz])))
        print(f"{pname} {graph} d/d{k}: max element-wise {err:.2e} over {int(nz.sum())} nonzero elements")
        assert err <= 1e-9, k


# ---- mathtab.h ------------------------------------------------------------------------------------------

def _tables():
    lits = re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+", MATHTAB.read_text())
    assert len(lits) == 3 * 128
    v = [float.fromhex(x) for x in lits]
    return v[0:256:2], v[1:256:2], v[256:]


def _is_correctly_rounded(x: float, exact) -> bool:
    """x is the binary64 nearest to the mpmath value ``exact``: the exact value lies strictly between the
    midpoints to x's neighbours (no table entry is a tie: they are irrational)."""
    import mpmath

    lo, hi = np.nextafter(x, -np.inf), np.nextafter(x, np.inf)
    return (mpmath.mpf(float(lo)) + mpmath.mpf(x)) / 2 < exact < (mpmath.mpf(x) + mpmath.mpf(float(hi))) / 2


def test_mathtab_reduction_constants():
    """c_j has at most 21 significant bits (m c_j is then exact in fp64 for a 24-bit m), and |m c_j - 1| < 2^-8 at
    both ends of interval j = [1 + j / 128, 1 + (j + 1) / 128) -- at the last float32 below the upper end and, since
    the product is linear in m, at the end itself."""
    c, _, _ = _tables()
    for j, cj in enumerate(c):
        m, _ = np.frexp(cj)
        assert (m * 2.0 ** 21) % 1.0 == 0.0, j
        lo, hi = 1.0 + j / 128.0, 1.0 + (j + 1) / 128.0
        for mm in (lo, float(np.nextafter(f32(hi), f32(0))), hi):
            r = mm * cj - 1.0  # exact: 24 + 21 bits
            assert abs(r) < 2.0 ** -8, (j, mm, r)


def test_mathtab_values_are_correctly_rounded():
    """-ln c_j and 2^(j / 128) are the binary64 values nearest the true ones (mpmath, 80 digits)."""
    import mpmath

    c, L, E = _tables()
    with mpmath.workdps(80):
        for j in range(128):
            assert _is_correctly_rounded(L[j], -mpmath.log(mpmath.mpf(c[j]))), j
            if j == 0:
                assert E[0] == 1.0
            else:
                assert _is_correctly_rounded(E[j], mpmath.power(2, mpmath.mpf(j) / 128)), j


def test_mathtab_is_what_the_generator_emits(tmp_path):
    spec = importlib.util.spec_from_file_location("gen_mathtab", ROOT / "tools" / "gen_mathtab.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = tmp_path / "mathtab.h"
    gen.main([str(out)])
    assert out.read_bytes() == MATHTAB.read_bytes()
