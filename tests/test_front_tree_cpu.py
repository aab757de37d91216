"""Pins helpers.front_tree_k2 on the host, for every tree of the GPU shape sweep
(test_ldl_shapes_gpu.py): the sweep names its cases after front shapes, so the analysis must return
exactly the prescribed fronts, the planner model that the sweep asserts its classes with must agree with
the analysis, and the matrices must be as well conditioned as the sweep's 1e-12 pivot gate assumes.

  * supernodes: Symbolic(ordering=0, relax=0) with MADIPM_BIG_MERGE=0 returns the nodes, (w, r) = (w, w + b),
    with the prescribed parents (the analysis postorders the tree again, so siblings may swap: the
    supernodes are matched to the nodes through the permutation, helpers.fronts_in_pivot_order);
  * classes: info()'s nbig / tree_fronts / tree_medium / max_front / fold_fronts / fold_leaves equal
    helpers.front_tree_classes for small_front_max in {128, 192} and MADIPM_TREE_FACT in {1, 0};
  * conditioning: the oracle's pivots agree with a dense np.longdouble no-pivot LDL^T to 1e-13 relative
    (5e-15 observed when the generator was designed: two float64 summation orders then differ by ~1e-14,
    100x inside the GPU gate).  A shape that exceeds it is replaced, the bound stays;
  * inertia of the oracle's D: (columns of positive blocks, 0, columns of negative blocks), for the
    matrix and for the refactorisation's perturbed values.
"""
import numpy as np
import pytest

from helpers import (ASSEMBLY_TREES, FRONT_TREE_OPTS, LEAF_SHAPE_R, assembly_tree, dense_ldlt_longdouble,
                     front_tree_classes, front_tree_k2, front_tree_nodes, fronts_in_pivot_order, leaf_shape_tree,
                     leaf_shape_widths, perturbed_values)
from oracle.ldl import OracleLDL


def _pin(root, seed, monkeypatch):
    from madipm_amd._lib import Symbolic, default_ldl_opts
    monkeypatch.setenv("MADIPM_BIG_MERGE", "0")
    K, Lw, nodes = front_tree_k2(root, seed)
    N = K.shape[0]
    for sfm in (128, 192):
        for tf in ("1", "0"):
            monkeypatch.setenv("MADIPM_TREE_FACT", tf)
            S = Symbolic(N, Lw.indptr, Lw.indices, default_ldl_opts(small_front_max=sfm, **FRONT_TREE_OPTS))
            perm = S.perm()
            node_of, _ = fronts_in_pivot_order(nodes, perm, *S.supernodes())
            assert sorted(node_of) == list(range(len(nodes))), (root, node_of)
            want, _ = front_tree_classes(nodes, sfm, tf == "1")
            info = S.info()
            assert {k: info[k] for k in want} == want, (root, sfm, tf)
            assert info["lb_groups"] == 0
    pos = sum(nd["w"] for nd in nodes if nd["depth"] % 2 == 0)
    assert sorted(perm) == list(range(N))
    _, K2 = perturbed_values(Lw, seed + 1)
    assert np.array_equal(K2.indices, K.indices) and np.array_equal(K2.indptr, K.indptr)
    assert abs(K2 - K2.T).max() == 0.0
    worst = 0.0
    for M in (K, K2):
        ref = OracleLDL(M, perm)
        assert ref.factorize() == N
        d = ref.diag()
        assert (int(np.sum(d > 0)), int(np.sum(d == 0)), int(np.sum(d < 0))) == (pos, 0, N - pos)
        dl = dense_ldlt_longdouble(M[perm][:, perm])
        worst = max(worst, float(np.max(np.abs(d - dl) / np.abs(dl))))
    assert worst <= 1e-13, (root, worst)
    return worst


@pytest.mark.parametrize("r", LEAF_SHAPE_R)
def test_leaf_shape_trees_pinned(r, monkeypatch):
    worst = max(_pin(leaf_shape_tree(r, w), 1000 * r + w, monkeypatch) for w in leaf_shape_widths(r))
    print(f"r={r}: oracle vs longdouble pivots, worst {worst:.2e}")


@pytest.mark.parametrize("name", sorted(ASSEMBLY_TREES))
def test_assembly_trees_pinned(name, monkeypatch):
    worst = _pin(assembly_tree(name), sorted(ASSEMBLY_TREES).index(name), monkeypatch)
    print(f"{name}: oracle vs longdouble pivots, worst {worst:.2e}")


def test_sweep_reaches_every_class():
    """The sweep's trees between them reach every class its boundaries separate (so a tree list that
    drifts off a class fails here, before any GPU run)."""
    seen = set()
    for name in ASSEMBLY_TREES:
        nodes = front_tree_nodes(assembly_tree(name))
        _, ftree = front_tree_classes(nodes)
        for s, nd in enumerate(nodes):
            kids = [nodes[c] for c in nd["children"]]
            if not kids or nd["parent"] < 0:
                continue
            tree_kids = sum(ftree[c] for c in nd["children"])
            seen.add(("fanin", min(tree_kids, 9), ftree[s]))
            if all(k["w"] <= 2 and k["r"] <= 32 for k in kids):
                seen.add("micro_fold")
            elif all(k["r"] <= 32 for k in kids):
                seen.add("preleaf_gather")
            seen.update(("child_rows", k["b"]) for k in kids if k["b"] in (128, 129))
            if nd["b"] in (128, 129):
                seen.add(("mid_rows", nd["b"]))
    for need in (("fanin", 8, True), ("fanin", 9, False), ("fanin", 2, True), "micro_fold", "preleaf_gather",
                 ("child_rows", 129), ("mid_rows", 129)):
        assert need in seen, (need, sorted(map(str, seen)))
