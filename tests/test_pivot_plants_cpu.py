"""Pins the planted pivot failures of test_ldl_pivot_failure_gpu.py on the oracle, in the analysis' pivot
order: the GPU file asserts `factorize(planted) == k + 1`, so a plant must make pivot k — and no earlier
one — fail in the reference, with margins that make pivot_tol = helpers.PLANT_TOL = 1e-8 a condition and
not a measurement.

For every (tree, plant) the GPU file uses (helpers.plant_tree_names, tree_plant_pivots, exact_plant_pivots,
pair_plant_pivots, flip_plant_pivots, batched_leaf_problem):
  * tiny and exact plants: the oracle's first index with !(|d| > tol) or |d| = inf is k (k1 for a pair),
    and d[:k] is BITWISE the good factorisation's d[:k];
  * tiny plants: the planted |d_k| <= 1e-12;
  * the good matrix: min |d| >= 0.1;
  * flip plants: the oracle agrees with helpers.dense_ldlt_longdouble within 1e-13 (test_front_tree_cpu.py's
    bound) on the planted matrix, which has no |d| < 0.1, and pivot k changes sign;
  * Cholesky semantics: the quasi-definite trees have a first non-positive pivot, past pivot 0;
  * the configurations between them reach every front class of helpers.PLANT_CLASSES, by the planner
    model that each GPU configuration asserts against info().
A plant that fails a pin is replaced; the bounds stay.
"""
import numpy as np
import pytest

from helpers import (EXACT_LEAF_SHAPES, EXACT_VALUES, FLIP_TREES, FRONT_TREE_OPTS, PLANT_CLASSES, PLANT_TOL,
                     batched_leaf_problem, dense_ldlt_longdouble, exact_plant_pivots, first_bad_pivot,
                     flip_plant_pivots, front_tree_k2, front_tree_nodes, oracle_plant, pair_plant_pivots,
                     plant_configs, plant_pivot, plant_required_classes, plant_tree, plant_tree_names,
                     root_plant_tree_names, signed_diagonal, symmetric_from_lower, tree_plant_pivots)
from oracle.ldl import OracleLDL

TINY_MAX = 1e-12
GOOD_MIN = 0.1


class _Tree:
    def __init__(self, name, monkeypatch):
        from madipm_amd._lib import Symbolic, default_ldl_opts
        monkeypatch.setenv("MADIPM_BIG_MERGE", "0")
        root, seed = plant_tree(name)
        self.K, self.Lw, self.nodes = front_tree_k2(root, seed)
        self.N = self.K.shape[0]
        S = Symbolic(self.N, self.Lw.indptr, self.Lw.indices, default_ldl_opts(small_front_max=128, **FRONT_TREE_OPTS))
        self.perm = S.perm()
        self.sn = S.supernodes()
        for sfm in (128, 192):      # the plants are placed by pivot index: one order for every configuration
            for tf in ("1", "0"):
                monkeypatch.setenv("MADIPM_TREE_FACT", tf)
                S2 = Symbolic(self.N, self.Lw.indptr, self.Lw.indices, default_ldl_opts(small_front_max=sfm, **FRONT_TREE_OPTS))
                assert np.array_equal(S2.perm(), self.perm)
        o = OracleLDL(self.K, self.perm)
        assert o.factorize() == self.N
        self.d = o.diag()
        assert np.min(np.abs(self.d)) >= GOOD_MIN, (name, np.min(np.abs(self.d)))

    def pin_failure(self, vals, k, tol, what):
        kbad, d, nv = oracle_plant(self.Lw, vals, self.perm, tol)
        assert kbad == k, f"{what}: the oracle's first bad pivot is {kbad}, planted {k}"
        assert nv > k and np.array_equal(d[:k].view(np.uint64), self.d[:k].view(np.uint64)), \
            f"{what}: the pivots before the plant changed"
        return d[k]


@pytest.mark.parametrize("name", root_plant_tree_names())
def test_tiny_plants_pinned(name, monkeypatch):
    t = _Tree(name, monkeypatch)
    worst = 0.0
    plants = tree_plant_pivots(t.nodes, t.perm, *t.sn)
    assert len({k for k, _, _ in plants}) == len(plants)
    for k, i, c in plants:
        vals = plant_pivot(t.Lw, t.Lw.data, t.perm, k, "tiny", t.d)
        dk = t.pin_failure(vals, k, PLANT_TOL, f"{name} tiny k={k} (front {i}, column {c})")
        assert abs(dk) <= TINY_MAX, (name, k, dk)
        worst = max(worst, abs(dk))
    print(f"{name}: {len(plants)} tiny plants, worst planted |d_k| {worst:.2e}, min good |d| {np.min(np.abs(t.d)):.3f}")


@pytest.mark.parametrize("rw", EXACT_LEAF_SHAPES, ids=lambda rw: "leaf_%d_%d" % rw)
def test_exact_plants_pinned(rw, monkeypatch):
    name = "leaf_%d_%d" % rw
    t = _Tree(name, monkeypatch)
    plants = exact_plant_pivots(t.nodes, t.perm, *t.sn)
    assert len(plants) == 3
    for k, i in plants:
        for v in EXACT_VALUES:
            vals = plant_pivot(t.Lw, t.Lw.data, t.perm, k, "exact", value=v)
            dk = t.pin_failure(vals, k, 0.0, f"{name} exact {v!r} k={k} (front {i})")
            assert np.array_equal(np.float64(dk).view(np.uint64), np.float64(v).view(np.uint64)) or (v == 0.0 and dk == 0.0)


@pytest.mark.parametrize("name", ["big_mixed", "leaf_128_65"])
def test_pair_plants_pinned(name, monkeypatch):
    t = _Tree(name, monkeypatch)
    pairs = pair_plant_pivots(name, t.nodes, t.perm, *t.sn)
    first_holds = set()
    for k1, k2, (i1, i2) in pairs:
        assert k1 < k2 and i1 != i2
        vals = plant_pivot(t.Lw, plant_pivot(t.Lw, t.Lw.data, t.perm, k1, "tiny", t.d), t.perm, k2, "tiny", t.d)
        dk = t.pin_failure(vals, k1, PLANT_TOL, f"{name} pair ({k1}, {k2})")
        assert abs(dk) <= TINY_MAX
        # the second plant fails on its own too: the pair races two failing fronts, not one
        only2 = plant_pivot(t.Lw, t.Lw.data, t.perm, k2, "tiny", t.d)
        assert abs(t.pin_failure(only2, k2, PLANT_TOL, f"{name} second of pair ({k1}, {k2})")) <= TINY_MAX
        first_holds.add((t.nodes[i1]["w"], t.nodes[i1]["r"]))
    assert len(first_holds) == 2, f"both subtrees must hold the smaller index once: {first_holds}"


@pytest.mark.parametrize("name", FLIP_TREES)
def test_flip_plants_and_cholesky_pinned(name, monkeypatch):
    t = _Tree(name, monkeypatch)
    nonpos = np.flatnonzero(t.d <= 0)
    assert len(nonpos) and nonpos[0] > 0, "Cholesky semantics need a first non-positive pivot past pivot 0"
    for k, i in flip_plant_pivots(name, t.nodes, t.perm, *t.sn):
        vals = plant_pivot(t.Lw, t.Lw.data, t.perm, k, "flip", t.d)
        K2 = symmetric_from_lower(t.Lw, vals)
        o = OracleLDL(K2, t.perm)
        assert o.factorize() == t.N
        d = o.diag()
        dl = dense_ldlt_longdouble(K2[t.perm][:, t.perm])
        worst = float(np.max(np.abs(d - dl) / np.abs(dl)))
        assert worst <= 1e-13, (name, k, worst)
        assert np.min(np.abs(d)) >= GOOD_MIN, (name, k, np.min(np.abs(d)))
        assert np.sign(d[k]) == -np.sign(t.d[k]) and abs(d[k] + 0.5 * t.d[k]) <= 1e-12 * abs(t.d[k])
        assert np.array_equal(d[:k], t.d[:k])
        print(f"{name} flip k={k} (front {i}): oracle vs longdouble {worst:.2e}, inertia "
              f"{(int(np.sum(d > 0)), int(np.sum(d < 0)))} from {(int(np.sum(t.d > 0)), int(np.sum(t.d < 0)))}")


def test_root_plants_are_in_the_tiny_set(monkeypatch):
    """The root cases of the GPU file plant the first and last column of the root: both are tiny plants
    pinned above (the last one is pivot N - 1)."""
    for name in root_plant_tree_names():
        t = _Tree(name, monkeypatch)
        ks = {k for k, i, _ in tree_plant_pivots(t.nodes, t.perm, *t.sn) if i == len(t.nodes) - 1}
        w = t.nodes[-1]["w"]
        assert {t.N - w, t.N - 1} <= ks


def test_batched_leaf_plants_pinned():
    from madipm_amd._lib import Symbolic, default_ldl_opts
    K, Lw, members = batched_leaf_problem()
    N = K.shape[0]
    S = Symbolic(N, Lw.indptr, Lw.indices, default_ldl_opts(ordering=0))
    info = S.info()
    assert (info["lb_groups"], info["lb_members"]) == (1, 200)
    first, parent, nrows = S.supernodes()
    mem = np.flatnonzero((nrows == 1) & (parent >= 0))
    assert len(mem) == 200 and np.array_equal(first[mem], np.arange(200)), "the members are pivots 0 .. 199"
    perm = S.perm()
    o = OracleLDL(K, perm)
    assert o.factorize() == N
    d0 = o.diag()
    assert np.min(np.abs(d0)) >= GOOD_MIN, np.min(np.abs(d0))

    def pin(vals, k, tol):
        kbad, d, nv = oracle_plant(Lw, vals, perm, tol)
        assert kbad == k and nv > k and np.array_equal(d[:k].view(np.uint64), d0[:k].view(np.uint64)), (kbad, k)
        return d[k]

    for k in members:
        assert abs(pin(plant_pivot(Lw, Lw.data, perm, k, "tiny", d0), k, PLANT_TOL)) <= TINY_MAX
        for v in EXACT_VALUES:
            pin(plant_pivot(Lw, Lw.data, perm, k, "exact", value=v), k, 0.0)
    a, b = members[1], members[2]
    pin(plant_pivot(Lw, plant_pivot(Lw, Lw.data, perm, b, "tiny", d0), perm, a, "tiny", d0), a, PLANT_TOL)


def test_signed_diagonal_is_beyond_one_grid_pass():
    Lw, d = signed_diagonal()
    assert Lw.shape[0] == len(d) == 20001 > 64 * 256 and Lw.nnz == 20001
    assert np.all((np.abs(d) >= 0.5) & (np.abs(d) <= 2.0)) and 0 < np.sum(d > 0) < len(d)
    assert first_bad_pivot(d, len(d), 0.0) == -1


def test_plants_reach_every_class():
    seen = set()
    for name in plant_tree_names():
        nodes = front_tree_nodes(plant_tree(name)[0])
        for tf in (True, False):
            for sfm, dag, _ in plant_configs(name, nodes, tf):
                seen |= plant_required_classes(nodes, sfm, tf, dag != "0")
    assert seen == set(PLANT_CLASSES), sorted(set(PLANT_CLASSES) ^ seen)
