"""Front shapes across the kernel boundaries of csrc/ldl.hip and csrc/ldl_solve.hip, against
the oracle's LDL^T in the same pivot order.

helpers.front_tree_k2 prescribes the fronts (pinned on the host in test_front_tree_cpu.py), so a case
places fronts exactly on a boundary: r = 32/33, 64/65, 128/129, 192/193, 256/257 rows, w <= 2 (micro
path), w = 15/16/17 (in-LDS pivot blocks), 63/64/65 (HBM panels, assembly tiles), update blocks of
128/129 rows (gathered / block-wise children), 8/9 tree children (fan-in of the tree launch).

Configurations: MADIPM_TREE_FACT in {1, 0} x small_front_max in {128, 192} (the test items), and inside
an item MADIPM_BIG_DAG in {1, 0} x MADIPM_BIG_KPAN in {1, 4} for the trees with a front of r >= 129, plus
once per tree the level-by-level solve kernels (MADIPM_TREE_SOLVE=0).

Every (tree, configuration) asserts first, through info(), that the plan has the classes its shapes
stand for (nbig, tree_fronts, tree_medium, max_front, fold_fronts, fold_leaves from
helpers.front_tree_classes): a sweep that no longer reaches a path fails.  Then, for the matrix and again — on the SAME solver, whose arena is zeroed
only at creation — for values perturbed entrywise by 1 + 0.3 U(0, 1):
  * every pivot within 1e-12 |d_ref| of the oracle's (the matrices are well conditioned: the oracle and
    a longdouble LDL^T agree to 5e-15, two float64 summation orders to ~1e-14);
  * one solve of a contiguous (3, N) block — a random b, e_j of the first leaf's first pivot, e_{N-1} —
    whose columns equal single-column solves BITWISE and the oracle's within 1e-12 in max-norm
    (relative to max |x_ref|), with berr_gpu <= 10 berr_ref + 1e-15;
  * the inertia (columns of positive blocks, 0, columns of negative blocks).
A failure names the front (node index, w, r) that owns the worst pivot.  Each test item prints the number
of cases and the largest pivot / solution differences it saw (pytest -s)."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from helpers import (ASSEMBLY_TREES, FRONT_TREE_OPTS, LEAF_SHAPE_R, FrontTreeCase, assembly_tree,
                     assert_front_tree_plan, leaf_shape_tree, leaf_shape_widths, perturbed_values)
from oracle.ldl import OracleLDL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PIVOT_TOL = SOL_TOL = 1e-12


def _berr(K, x, b):
    return np.max(np.abs(K @ x - b)) / (spla.norm(K, np.inf) * np.max(np.abs(x)) + np.max(np.abs(b)))


class _Case(FrontTreeCase):
    """A tree's matrices, right-hand sides and oracle results: computed once, shared by its configurations."""

    def __init__(self, root, seed):
        super().__init__(root, seed)
        vals2, K2 = perturbed_values(self.Lw, seed + 1)
        self.mats = [(self.K, self.Lw.data.copy()), (K2, vals2)]
        self._ref = {}

    def ref(self, perm):
        """[(d_ref, X_ref (3, N), berr_ref (3,))] for the two matrices, in the solver's pivot order."""
        key = perm.tobytes()
        if key not in self._ref:
            out = []
            for M, _ in self.mats:
                o = OracleLDL(M, perm)
                assert o.factorize() == self.N
                X = np.stack([o.solve(b) for b in self.B])
                out.append((o.diag(), X, np.array([_berr(M, x, b) for x, b in zip(X, self.B)])))
            self._ref[key] = out
        return self._ref[key]


_CASES = {}


def _case(root, seed):
    key = (_hashable(root), seed)
    if key not in _CASES:
        _CASES[key] = _Case(key[0], seed)
    return _CASES[key]


def _hashable(root):
    w, b, ch = root
    return (w, b, tuple(_hashable(c) for c in ch))


def _run(case, sfm, tree_fact, stats, tag):
    """One configuration (the environment is the caller's): class assertions, then factorise / solve /
    refactorise.  Returns the failures as strings; HIP errors propagate."""
    from madipm_amd.linear_solver import HIPLDLSolver
    N, Lw = case.N, case.Lw
    ls = HIPLDLSolver(N, Lw.indptr, Lw.indices, small_front_max=sfm, **FRONT_TREE_OPTS)
    assert_front_tree_plan(ls.info(), case.nodes, sfm, tree_fact, tag)
    perm = ls.perm()
    dev = torch.device("cuda:0")
    fails = []
    for which, ((M, vals), (d_ref, X_ref, berr_ref)) in enumerate(zip(case.mats, case.ref(perm))):
        what = f"{tag} {'refactorised' if which else 'first'}"
        rc = ls.factorize(torch.from_numpy(vals.copy()).to(dev))
        if rc != 0 or not ls.is_factorized():
            fails.append(f"{what}: factorize returned {rc}")
            continue
        d = ls.diag()
        rel = np.abs(d - d_ref) / np.abs(d_ref)
        rel[~np.isfinite(rel)] = np.inf
        k = int(np.argmax(rel))
        stats["pivot"] = max(stats["pivot"], float(rel[k]))
        if rel[k] > PIVOT_TOL:
            fails.append(f"{what}: {int(np.sum(rel > PIVOT_TOL))} pivots off, worst {rel[k]:.3e} at k={k} in "
                         f"{case.front_of_pivot(perm, k)}: gpu {d[k]:.17e} oracle {d_ref[k]:.17e}")
        if ls.inertia() != (case.pos, 0, N - case.pos):
            fails.append(f"{what}: inertia {ls.inertia()}, expected {(case.pos, 0, N - case.pos)}")
        X = torch.from_numpy(case.B.copy()).to(dev)
        assert X.is_contiguous() and X.shape == (3, N)
        ls.solve(X)
        torch.cuda.synchronize()
        X = X.cpu().numpy()
        for j in range(3):
            x1 = torch.from_numpy(case.B[j].copy()).to(dev)
            ls.solve(x1)
            torch.cuda.synchronize()
            x1 = x1.cpu().numpy()
            if not np.array_equal(X[j].view(np.uint64), x1.view(np.uint64)):
                with np.errstate(invalid="ignore"):
                    fails.append(f"{what}: column {j} of the 3-column solve differs from its single solve at "
                                 f"{int(np.sum(X[j] != x1))} entries, max {np.nanmax(np.abs(X[j] - x1)):.3e}")
            err = np.max(np.abs(X[j] - X_ref[j])) / np.max(np.abs(X_ref[j]))
            if not np.isfinite(err):
                err = np.inf
            stats["sol"] = max(stats["sol"], float(err))
            if err > SOL_TOL:
                fails.append(f"{what}: column {j} solution off by {err:.3e}")
            bg = _berr(M, X[j], case.B[j])
            if not bg <= 10 * berr_ref[j] + 1e-15:
                fails.append(f"{what}: column {j} backward error gpu {bg:.3e} vs oracle {berr_ref[j]:.3e}")
    stats["cases"] += 1
    return fails


def _configs(rmax):
    """(MADIPM_BIG_DAG, MADIPM_BIG_KPAN): swept only where a front can be big (r >= 129)."""
    return [("1", "1"), ("1", "4"), ("0", "1"), ("0", "4")] if rmax >= 129 else [(None, None)]


def _sweep(cases, sfm, tree_fact, monkeypatch, label):
    monkeypatch.setenv("MADIPM_BIG_MERGE", "0")
    monkeypatch.setenv("MADIPM_TREE_FACT", tree_fact)
    stats = dict(cases=0, pivot=0.0, sol=0.0)
    fails = []
    for name, case in cases:
        configs = [(dag, kpan, "1") for dag, kpan in _configs(max(nd["r"] for nd in case.nodes))]
        for dag, kpan, tree_solve in configs + [configs[0][:2] + ("0",)]:
            # the level-by-level solve kernels (MADIPM_TREE_SOLVE=0) once per tree, on the first configuration
            monkeypatch.setenv("MADIPM_TREE_SOLVE", tree_solve)
            tag = f"{name} sfm={sfm} tree_fact={tree_fact} tree_solve={tree_solve}"
            if dag is not None:
                monkeypatch.setenv("MADIPM_BIG_DAG", dag)
                monkeypatch.setenv("MADIPM_BIG_KPAN", kpan)
                tag += f" dag={dag} kpan={kpan}"
            fails += _run(case, sfm, tree_fact == "1", stats, tag)
    print(f"\nSHAPES {label} sfm={sfm} tree_fact={tree_fact}: cases={stats['cases']} "
          f"max_pivot_diff={stats['pivot']:.3e} max_solution_diff={stats['sol']:.3e}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails)


@pytest.mark.parametrize("sfm", [128, 192])
@pytest.mark.parametrize("tree_fact", ["1", "0"])
@pytest.mark.parametrize("r", LEAF_SHAPE_R)
def test_leaf_shapes(r, tree_fact, sfm, monkeypatch):
    """Three leaves (two of (w, r), one of (w / 2, r - w + w / 2)) under a dense root of r - w + 3 columns,
    for every w of helpers.leaf_shape_widths(r)."""
    cases = [(f"leaf w={w} r={r}", _case(leaf_shape_tree(r, w), 1000 * r + w)) for w in leaf_shape_widths(r)]
    _sweep(cases, sfm, tree_fact, monkeypatch, f"leaf r={r}")


@pytest.mark.parametrize("sfm", [128, 192])
@pytest.mark.parametrize("tree_fact", ["1", "0"])
@pytest.mark.parametrize("name", sorted(ASSEMBLY_TREES))
def test_assembly_and_fan_in(name, tree_fact, sfm, monkeypatch):
    """Three-level trees (helpers.ASSEMBLY_TREES): pre-leaf versus tree children, fan-in 8 versus 9,
    gathered versus block-wise update blocks, the micro-leaf fold."""
    case = _case(assembly_tree(name), sorted(ASSEMBLY_TREES).index(name))
    _sweep([(name, case)], sfm, tree_fact, monkeypatch, f"assembly {name}")
