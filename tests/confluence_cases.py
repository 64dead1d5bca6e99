"""Shared by test_confluence_cases.py and test_gpu_confluences.py: seeded networks whose reaches take more than
two inflows, and a classifier of what a built graph made of them.

``ddr_amd.synthetic`` caps the in-degree at 2 (``random_binary_tree`` by construction, ``hack_basin`` with one
tributary per spine joint), so none of its networks reaches the routing kernels' confluence list (csrc/route_device.h
``pack_up`` / ``up_1`` and the ``j = 2..c`` tails; csrc/graph.cpp and csrc/devgraph.hip ``xoff`` / ``xlist``).  Real
MERIT and Lynker networks do.  The builders here are deterministic, numbered upstream first, and return
``synthetic.SyntheticNetwork`` with the COO of ``synthetic._down_to_coo``.

  bushy(n, seed)           random tree, fan-ins from FANINS (both sides of the packed word's 15 cap)
  hub_of_subtrees(k, m)    one outlet with k inflows, each the root of an m-reach random binary tree
  star(k)                  an outlet with k leaf inflows;  STAR_KS the sweep
  mix40()                  hand-written: a 9-star feeding a 5-chain, joining a 20-star under a 5-way outlet
  confetti(n_basins, seed) basins of 1 to 3 reaches (many distinct basin keys per 64 consecutive reaches)
  classify(block, net)     per confluence: local / cut inflow counts and the list positions of the cut ones
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from ddr_amd import synthetic
from ddr_amd.synthetic import SyntheticNetwork, _down_to_coo

FANINS = (1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 6, 9, 14, 15, 16, 17, 20)
STAR_KS = (3, 14, 15, 16, 17, 63, 64, 65)
T = 48  # steps of the GPU tests: every case keeps max_depth + 2 < T (steady ticks exist)
CUT64 = {"max_block_reaches": 64, "target_blocks": 1 << 20}
CUT160 = {"max_block_reaches": 160, "target_blocks": 1 << 20}
WHOLE = {"target_blocks": 1}
# the largest star whose default-options build succeeds: its hub keeps 180 leaves and takes 1024 inflows over cut
# edges, the most one workgroup imports (found by bisection over 3..2100, where success is monotonic in k)
LARGEST_STAR = 1204


def _upstream_first(down_created: np.ndarray) -> np.ndarray:
    """Parent pointers in creation order (a parent is created before its children) -> the same tree numbered
    upstream first (reversed creation order)."""
    n = len(down_created)
    new = (n - 1) - np.arange(n, dtype=np.int64)
    down = np.full(n, -1, dtype=np.int64)
    has = down_created >= 0
    down[new[has]] = new[down_created[has]]
    return down


def _net(down: np.ndarray, basin_sizes=None) -> SyntheticNetwork:
    n = len(down)
    assert np.all((down < 0) | (down > np.arange(n))), "not numbered upstream first"
    rows, cols = _down_to_coo(down)
    sizes = np.array([n] if basin_sizes is None else basin_sizes, dtype=np.int64)
    return SyntheticNetwork(n, rows, cols, sizes)


def bushy(n: int, seed: int = 0) -> SyntheticNetwork:
    """A random tree of n reaches: a uniformly chosen open reach takes a fan-in from FANINS (each value once,
    in order, before the draws become random, so every listed in-degree occurs when n allows) and its inflows
    become open reaches."""
    rng = np.random.default_rng(seed)
    down = np.full(n, -1, dtype=np.int64)
    frontier = [0]
    nxt = 1
    once = [f for f in sorted(set(FANINS)) if f > 2]
    while nxt < n and frontier:
        k = int(rng.integers(len(frontier)))
        v = frontier[k]
        frontier[k] = frontier[-1]
        frontier.pop()
        f = once.pop() if once and n - nxt >= once[-1] else int(FANINS[int(rng.integers(len(FANINS)))])
        f = min(f, n - nxt)
        down[nxt:nxt + f] = v
        frontier.extend(range(nxt, nxt + f))
        nxt += f
    assert nxt == n
    return _net(_upstream_first(down))


def hub_of_subtrees(k: int, m: int, seed: int = 0) -> SyntheticNetwork:
    """k random binary trees of m reaches each, numbered one after another, whose outlets all drain into one
    last reach.  With m near the block cap each tree fills a block of its own and every inflow of the hub is a
    cut edge."""
    n = k * m + 1
    down = np.full(n, -1, dtype=np.int64)
    for s in range(k):
        d = synthetic.random_binary_tree(m, seed=seed + s).down
        seg = down[s * m:(s + 1) * m]
        seg[d >= 0] = d[d >= 0] + s * m
        seg[m - 1] = n - 1
    return _net(down)


def star(k: int) -> SyntheticNetwork:
    down = np.full(k + 1, k, dtype=np.int64)
    down[k] = -1
    return _net(down)


# mix40: reaches 0..8 -> 9 (a 9-star), 9 -> 10 -> ... -> 14 (a chain), 15..34 -> 35 (a 20-star),
# and 14, 35, 36, 37, 38 -> 39 (a 5-way outlet)
MIX40_HUB9, MIX40_HUB20, MIX40_OUTLET, MIX40_LEAF20 = 9, 35, 39, 20


def mix40() -> SyntheticNetwork:
    down = np.full(40, -1, dtype=np.int64)
    down[0:9] = 9
    down[9:14] = np.arange(10, 15)
    down[14] = 39
    down[15:35] = 35
    down[35:39] = 39
    return _net(down)


def confetti(n_basins: int, seed: int = 0) -> SyntheticNetwork:
    """n_basins basins of one reach, a two-chain, a three-chain or a two-inflow confluence, in random order."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, n_basins)
    sizes = np.array([1, 2, 3, 3])[kind]
    start = np.concatenate([[0], np.cumsum(sizes)])
    down = np.full(int(start[-1]), -1, dtype=np.int64)
    for b in np.flatnonzero(kind == 1):
        down[start[b]] = start[b] + 1
    for b in np.flatnonzero(kind == 2):
        down[start[b]] = start[b] + 1
        down[start[b] + 1] = start[b] + 2
    for b in np.flatnonzero(kind == 3):
        down[start[b]] = start[b] + 2
        down[start[b] + 1] = start[b] + 2
    return _net(down, sizes)


# tests/golden/confluence.npz (make_golden.py make_confluence): the reference on bushy(GOLDEN_N, GOLDEN_SEED)
GOLDEN_N, GOLDEN_SEED, GOLDEN_W2_SEED = 300, 0, 99


def golden_gauges(net: SyntheticNetwork) -> list:
    """Gauge groups of the golden gauge-mode run: the outlet (a 20-way confluence) by negative index, three
    confluences summed, one headwater, and a confluence with a reach of one or two inflows."""
    indeg = np.bincount(net.rows, minlength=net.n)
    conf = np.flatnonzero(indeg > 2)
    head = np.flatnonzero(indeg == 0)
    plain = np.flatnonzero((indeg == 1) | (indeg == 2))
    return [np.array([-1]), conf[[0, len(conf) // 2, len(conf) - 2]], head[[len(head) // 3]],
            np.array([conf[3], plain[0]])]


def golden_confluence():
    """(first leg, second leg, gauge-mode case, fixture dict).  q' and W come from their seeds as
    make_confluence drew them; the stored float64 sums pin them."""
    from conftest import PARAMS_DEFAULT, Case, load_golden

    d = load_golden("confluence")
    n, steps = int(d["n"]), int(d["T"])
    assert (n, steps) == (GOLDEN_N, T)
    net = bushy(n, GOLDEN_SEED)
    np.testing.assert_array_equal(net.rows, d["rows"])
    np.testing.assert_array_equal(net.cols, d["cols"])
    offs = d["outflow_offsets"]
    outflow = [d["outflow_flat"][offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    u = {k: d[f"u_{k}"] for k in ("n", "q_spatial", "p_spatial")}
    q1 = synthetic.lateral_inflow(n, steps, GOLDEN_SEED)
    q2 = synthetic.lateral_inflow(n, steps, GOLDEN_SEED, t0=steps)
    W1 = np.random.default_rng(GOLDEN_SEED + 4000).uniform(0, 1, (n, steps)).astype(np.float32)
    W2 = np.random.default_rng(GOLDEN_W2_SEED).uniform(0, 1, (n, steps)).astype(np.float32)
    Wg = np.random.default_rng(GOLDEN_SEED + 4000).uniform(0, 1, (len(outflow), steps)).astype(np.float32)
    for a, key in ((q1, "qprime_sum"), (W1, "W_sum"), (q2, "qprime2_sum"), (W2, "W2_sum"), (Wg, "Wg_sum")):
        assert float(a.astype(np.float64).sum()) == float(d[key]), f"{key}: the seeded input changed"
    mk = lambda q, W: Case(n, d["rows"], d["cols"], d["length"], d["slope"], d["x"], q, W, u, PARAMS_DEFAULT)  # noqa: E731
    return mk(q1, W1), mk(q2, W2), mk(q1, Wg), dict(d, outflow=outflow)


@functools.lru_cache(maxsize=None)
def network(name: str) -> SyntheticNetwork:
    """The networks of the GPU tests, by name (built once; treat as read-only)."""
    if name == "golden300":
        return bushy(GOLDEN_N, GOLDEN_SEED)
    if name.startswith("bushy"):
        return bushy(int(name[5:]), 0)
    if name == "hub":
        return hub_of_subtrees(20, 51)  # 51-reach trees: at cap 64 the packer leaves the hub a block of its own
    if name == "mix40":
        return mix40()
    if name.startswith("star"):
        return star(int(name[4:]))
    if name == "confetti":
        return confetti(5000, 1)
    raise KeyError(name)


_DEGS = {"deg3", "deg14", "deg15", "deg16", "deg17plus"}
_BUSHY_WHOLE = {"all_local", "two_in_block"} | _DEGS
_BUSHY_CUT = _BUSHY_WHOLE | {"mixed", "cut_pos0", "cut_pos1", "cut_pos2plus"}
_HUB_CUT = {"all_cut", "cut_pos0", "cut_pos1", "cut_pos2plus", "deg17plus"}
ALL_CLASSES = _BUSHY_CUT | _HUB_CUT
GEN4 = {**CUT160, "max_resident": 4}
# (network, partition name, builder arguments, classes of confluence the pair must hold, reaches per thread or
# None): every (network, partition) the GPU tests route.  test_confluence_cases.py asserts each row with
# classify() on the host build, so no GPU test silently tests nothing.
PAIRS = [
    ("golden300", "whole", WHOLE, _BUSHY_WHOLE, 1),
    ("golden300", "cut64", CUT64, _BUSHY_CUT, None),
    ("bushy600", "whole", WHOLE, _BUSHY_WHOLE, 1),
    ("bushy600", "cut64", CUT64, _BUSHY_CUT, None),
    ("bushy600", "cut160", CUT160, _BUSHY_CUT, None),
    ("bushy600", "gen4", GEN4, _BUSHY_CUT, None),
    ("bushy1500", "whole", WHOLE, _BUSHY_WHOLE, 2),
    ("bushy2600", "whole", WHOLE, _BUSHY_WHOLE, 4),
    ("bushy2600", "cut64", CUT64, _BUSHY_CUT, None),
    ("bushy2600", "cap500", {"max_block_reaches": 500, "target_blocks": 1 << 20}, _BUSHY_CUT, 1),
    ("bushy2600", "cap1500", {"max_block_reaches": 1500, "target_blocks": 2}, _BUSHY_CUT, 2),
    ("hub", "whole", WHOLE, {"all_local", "deg17plus"}, 1),
    ("hub", "cut64", CUT64, _HUB_CUT, None),
    ("mix40", "whole", WHOLE, {"all_local", "two_in_block", "deg17plus"}, 1),
]


def pair(net_name: str, part: str):
    """(network, builder arguments) of a PAIRS row."""
    for nm, p, gkw, _, _ in PAIRS:
        if (nm, p) == (net_name, part):
            return network(nm), dict(gkw)
    raise KeyError((net_name, part))


@dataclass
class Confluences:
    ids: np.ndarray        # reaches with more than two inflows, ascending
    indeg: np.ndarray      # their in-degrees
    n_local: np.ndarray    # inflows from the reach's own block
    n_cut: np.ndarray      # inflows over cut edges (virtual slots in the block)
    cut_pos: list          # per confluence: positions of the cut inflows among its inflows in ascending column
    #                        order (position 0 is the packed word's slot, 1.. are the list entries u1, u2, ...)
    per_block: np.ndarray  # confluences per block
    list_len: np.ndarray   # int32 entries of each block's confluence lists (a list [c, u1, ..] holds c)

    def classes(self) -> set:
        """Names of the classes of confluence this partition holds (test_confluence_cases.py asserts them)."""
        out = set()
        if np.any(self.n_cut == 0):
            out.add("all_local")
        if np.any((self.n_cut > 0) & (self.n_local > 0)):
            out.add("mixed")
        if np.any(self.n_local == 0):
            out.add("all_cut")
        pos = np.concatenate(self.cut_pos) if self.cut_pos else np.zeros(0, np.int64)
        for name, hit in (("cut_pos0", pos == 0), ("cut_pos1", pos == 1), ("cut_pos2plus", pos >= 2)):
            if np.any(hit):
                out.add(name)
        if self.per_block.size and self.per_block.max() >= 2:
            out.add("two_in_block")
        for d in (3, 14, 15, 16):
            if np.any(self.indeg == d):
                out.add(f"deg{d}")
        if np.any(self.indeg >= 17):
            out.add("deg17plus")
        return out


def classify(block: np.ndarray, net: SyntheticNetwork) -> Confluences:
    """What the partition ``block`` (``RiverGraph.structure()["block"]``) makes of the network's confluences."""
    block = np.asarray(block)
    indeg = np.bincount(net.rows, minlength=net.n)
    ids = np.flatnonzero(indeg > 2)
    order = np.lexsort((net.cols, net.rows))  # ascending column within a row, as csrc/graph.cpp emits
    rows, cols = net.rows[order], net.cols[order]
    start = np.concatenate([[0], np.cumsum(indeg)])
    n_local, n_cut, cut_pos = [], [], []
    for i in ids:
        ups = cols[start[i]:start[i + 1]]
        assert np.all(rows[start[i]:start[i + 1]] == i)
        cut = block[ups] != block[i]
        n_local.append(int(np.sum(~cut)))
        n_cut.append(int(np.sum(cut)))
        cut_pos.append(np.flatnonzero(cut))
    per_block = np.bincount(block[ids], minlength=int(block.max()) + 1) if len(block) else np.zeros(0, np.int64)
    list_len = np.bincount(block[ids], weights=indeg[ids], minlength=len(per_block)).astype(np.int64)
    return Confluences(ids, indeg[ids], np.array(n_local, np.int64), np.array(n_cut, np.int64), cut_pos, per_block,
                       list_len)
