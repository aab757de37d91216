"""Failed pivots in every front class of csrc/ldl.hip: reported, with the smallest failing index, and
leaving nothing behind.

The interior-point loop retries a failed factorisation on the same solver after it has already enqueued
speculative solves on the failed factor (full of inf / NaN).  So, for every pivot-check site:
  1. a bad pivot is reported;
  2. factorize() returns the smallest failing pivot index + 1, whichever kernels race on the status word;
  3. a failed factorisation and a solve on it change nothing in the next good factorisation and solve.

helpers.plant_pivot changes one diagonal entry of a prescribed-front matrix (helpers.front_tree_k2, the
shape sweep's trees and seeds) so that pivot k fails; test_pivot_plants_cpu.py pins every plant on the
oracle (first bad index k, earlier pivots bitwise the good ones, planted |d_k| <= 1e-12, good |d| >= 0.1:
pivot_tol = 1e-8 is a condition, not a measurement).  Plants sit in columns 0, 16, 17, 64, 65 and w - 1 of
every front: pivot-block and panel boundaries, where an index offset would go wrong.

Per configuration (MADIPM_TREE_FACT x small_front_max x MADIPM_BIG_DAG x MADIPM_BIG_KPAN, the classes
asserted through info() against helpers.front_tree_classes) a fresh solver A factorises the good values
once: its diag() and 3-column solve are the reference BITS.  One solver B takes every plant in turn:
  * factorize(planted) == k + 1, is_factorized() false;
  * diag()[:k] within 1e-12 (relative) of the oracle's good pivots; not |diag()[k]| > 1e-8;
  * one solve on the failed factor returns (the MPC's speculated solve; values unchecked; a lost
    hand-off would raise from the next factorize);
  * factorize(good) == 0, is_factorized(), the prescribed inertia;
  * diag() bitwise A's; the 3-column solve bitwise A's and within 1e-12 of the oracle's.
A failure names the plant and its front (node, w, r).  Each item prints its number of plants and the
largest diag()[:k] difference (pytest -s)."""
import numpy as np
import pytest

from helpers import (EXACT_LEAF_SHAPES, EXACT_VALUES, FLIP_TREES, FRONT_TREE_OPTS, PLANT_TOL, batched_leaf_problem,
                     FrontTreeCase, assert_front_tree_plan, exact_plant_pivots, flip_plant_pivots, oracle_plant,
                     pair_plant_pivots, plant_configs, plant_pivot, plant_required_classes, plant_tree,
                     plant_tree_names, root_plant_tree_names, signed_diagonal, tree_plant_pivots)
from oracle.ldl import OracleLDL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PIVOT_TOL = SOL_TOL = 1e-12


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class _Case(FrontTreeCase):
    """A tree's matrix, right-hand sides (the shape sweep's) and oracle results, shared by its configurations."""

    def __init__(self, name):
        super().__init__(*plant_tree(name))
        self.name = name
        self.good = self.Lw.data.copy()
        self.inertia = (self.pos, 0, self.N - self.pos)
        self._ref = {}

    def ref(self, perm):
        """(d_ref, X_ref (3, N)) of the good matrix in the solver's pivot order."""
        key = perm.tobytes()
        if key not in self._ref:
            o = OracleLDL(self.K, perm)
            assert o.factorize() == self.N
            self._ref[key] = (o.diag(), np.stack([o.solve(b) for b in self.B]))
        return self._ref[key]

    def front_of_pivot(self, perm, k):
        i = self.node_of_pivot(perm, k)
        return super().front_of_pivot(perm, k)[:-1] + f", column {int(perm[k]) - self.nodes[i]['first']})"


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = _Case(name)
    return _CASES[name]


def _dev(vals):
    return torch.from_numpy(np.array(vals, dtype=np.float64, copy=True)).to(torch.device("cuda:0"))


def _solve(ls, rhs):
    X = _dev(rhs)
    assert X.is_contiguous()
    ls.solve(X)
    torch.cuda.synchronize()
    return X.cpu().numpy()


class _Pair:
    """Solver B of the module docstring (self.ls: it takes the plants) and the reference bits of a fresh
    solver A with the same options."""

    def __init__(self, N, Lw, good, rhs, inertia, X_ref, **opts):
        """X_ref: the oracle's solutions of rhs in the solvers' pivot order (may be set after construction,
        from self.perm)."""
        from madipm_amd.linear_solver import HIPLDLSolver
        self.N, self.Lw, self.good, self.rhs, self.inertia, self.X_ref = N, Lw, good, rhs, inertia, X_ref
        A = HIPLDLSolver(N, Lw.indptr, Lw.indices, **opts)
        assert A.factorize(_dev(good)) == 0 and A.is_factorized()
        assert inertia is None or A.inertia() == inertia, (A.inertia(), inertia)
        self.dA = A.diag().copy()
        self.XA = _solve(A, rhs)
        self.ls = HIPLDLSolver(N, Lw.indptr, Lw.indices, **opts)
        self.perm = self.ls.perm()
        assert np.array_equal(self.perm, A.perm())
        del A
        self.bitwise = True

    def fail(self, vals, k, d_ref, what, stats, check_dk=True):
        """factorize(planted) on B must report pivot k; then B must recover bitwise.  Returns failures."""
        ls, out = self.ls, []
        rc = ls.factorize(_dev(vals))
        if rc != k + 1:
            out.append(f"{what}: factorize returned {rc}, expected {k + 1}")
        if ls.is_factorized():
            out.append(f"{what}: is_factorized() after a failed factorisation")
        d = ls.diag()
        if k:
            rel = np.abs(d[:k] - d_ref[:k]) / np.abs(d_ref[:k])
            rel[~np.isfinite(rel)] = np.inf
            stats["pivot"] = max(stats["pivot"], float(rel.max()))
            if rel.max() > PIVOT_TOL:
                out.append(f"{what}: pivots before the plant off by {rel.max():.3e} at k={int(np.argmax(rel))}")
        if check_dk and abs(d[k]) > PLANT_TOL:
            out.append(f"{what}: planted pivot {d[k]:.3e} is above pivot_tol")
        _solve(ls, self.rhs[0])                      # the speculated solve on the failed factor
        stats["plants"] += 1
        return out + self.recover(what, stats)

    def recover(self, what, stats):
        ls, out = self.ls, []
        rc = ls.factorize(_dev(self.good))
        if rc != 0 or not ls.is_factorized():
            return [f"{what}: the good values returned {rc} afterwards (is_factorized {ls.is_factorized()})"]
        if self.inertia is not None and ls.inertia() != self.inertia:
            out.append(f"{what}: inertia {ls.inertia()} afterwards, expected {self.inertia}")
        d = ls.diag()
        if not np.array_equal(_bits(d), _bits(self.dA)):
            self.bitwise = stats["bitwise"] = False
            out.append(f"{what}: {int(np.sum(_bits(d) != _bits(self.dA)))} pivots differ afterwards from a fresh solver's")
        X = _solve(ls, self.rhs)
        if not np.array_equal(_bits(X), _bits(self.XA)):
            self.bitwise = stats["bitwise"] = False
            with np.errstate(invalid="ignore"):
                out.append(f"{what}: the 3-column solve differs afterwards from a fresh solver's at "
                           f"{int(np.sum(_bits(X) != _bits(self.XA)))} entries, max {np.nanmax(np.abs(X - self.XA)):.3e}")
        for j in range(len(self.rhs)):
            err = np.max(np.abs(X[j] - self.X_ref[j])) / np.max(np.abs(self.X_ref[j]))
            if not err <= SOL_TOL:
                out.append(f"{what}: column {j} of the solve afterwards is off the oracle's by {err:.3e}")
        return out


def _stats():
    return dict(plants=0, pivot=0.0, bitwise=True)


def _report(label, stats, fails):
    print(f"\nPLANTS {label}: plants={stats['plants']} max_diag_before_plant_diff={stats['pivot']:.3e} "
          f"bitwise_recovery={stats['bitwise']}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails)


def _opts(sfm, pivot_tol=PLANT_TOL, cholesky=False):
    return dict(small_front_max=sfm, pivot_tol=pivot_tol, cholesky=cholesky, **FRONT_TREE_OPTS)


def _assert_big_path(ls, case, sfm, tree_fact, dag, tag):
    """MADIPM_BIG_DAG is honoured: with big fronts outside the tree launch, one good factorisation under
    kernel timing launches k_big_dag and no k_big_diag (dag), or the reverse (per step)."""
    classes = plant_required_classes(case.nodes, sfm, tree_fact, dag != "0")
    if not classes & {"big_dag", "big_step"}:
        return
    ls.set_kernel_timing()
    assert ls.factorize(_dev(case.good)) == 0
    n = {k["name"]: k["launches"] for k in ls.kernel_stats()}
    ls.set_kernel_timing(0)
    if "big_dag" in classes:
        assert n["k_big_dag"] > 0 and n["k_big_diag"] == 0, f"{tag}: big fronts not in k_big_dag: {n}"
    else:
        assert n["k_big_dag"] == 0 and n["k_big_diag"] > 0, f"{tag}: big fronts not factorised per step: {n}"


def _tree_pair(case, sfm, tree_fact, tag, dag=None, pivot_tol=PLANT_TOL):
    """Solvers of one configuration (the environment is the caller's), its classes and launch path
    asserted first.  Returns (perm, d_ref, the _Pair)."""
    pair = _Pair(case.N, case.Lw, case.good, case.B, case.inertia, None, **_opts(sfm, pivot_tol))
    perm = pair.perm
    d_ref, pair.X_ref = case.ref(perm)
    assert_front_tree_plan(pair.ls.info(), case.nodes, sfm, tree_fact, tag)
    _assert_big_path(pair.ls, case, sfm, tree_fact, dag, tag)
    return perm, d_ref, pair


def _supernodes(case, perm, sfm):
    """(first, parent, nrows) of the analysis in pivot order, from the solver's own permutation."""
    from madipm_amd._lib import Symbolic, default_ldl_opts
    S = Symbolic(case.N, case.Lw.indptr, case.Lw.indices, default_ldl_opts(small_front_max=sfm, **FRONT_TREE_OPTS))
    assert np.array_equal(S.perm(), perm)
    return S.supernodes()


def _setenv(monkeypatch, tree_fact, dag=None, kpan=None):
    monkeypatch.setenv("MADIPM_BIG_MERGE", "0")
    monkeypatch.setenv("MADIPM_TREE_FACT", tree_fact)
    tag = f"tree_fact={tree_fact}"
    if dag is not None:
        monkeypatch.setenv("MADIPM_BIG_DAG", dag)
        monkeypatch.setenv("MADIPM_BIG_KPAN", kpan)
        tag += f" dag={dag} kpan={kpan}"
    return tag


@pytest.mark.parametrize("tree_fact", ["1", "0"])
@pytest.mark.parametrize("name", plant_tree_names())
def test_tiny_plants(name, tree_fact, monkeypatch):
    """A rounding-noise pivot in columns 0, 16, 17, 64, 65, w - 1 of every front, pivot_tol = 1e-8."""
    case = _case(name)
    stats, fails = _stats(), []
    for sfm, dag, kpan in plant_configs(name, case.nodes, tree_fact == "1"):
        tag = f"{name} sfm={sfm} " + _setenv(monkeypatch, tree_fact, dag, kpan)
        perm, d_ref, pair = _tree_pair(case, sfm, tree_fact == "1", tag, dag)
        for k, i, c in tree_plant_pivots(case.nodes, perm, *_supernodes(case, perm, sfm)):
            vals = plant_pivot(case.Lw, case.good, perm, k, "tiny", d_ref)
            fails += pair.fail(vals, k, d_ref, f"{tag} tiny k={k} in {case.front_of_pivot(perm, k)}", stats)
    _report(f"tiny {name} tree_fact={tree_fact}", stats, fails)


@pytest.mark.parametrize("tree_fact", ["1", "0"])
@pytest.mark.parametrize("rw", EXACT_LEAF_SHAPES, ids=lambda rw: "leaf_%d_%d" % rw)
def test_exact_plants(rw, tree_fact, monkeypatch):
    """0.0, -0.0, NaN and +inf as the first pivot of every childless front, pivot_tol = 0 (the IPM's default)."""
    name = "leaf_%d_%d" % rw
    case = _case(name)
    stats, fails = _stats(), []
    for sfm, dag, kpan in plant_configs(name, case.nodes, tree_fact == "1"):
        tag = f"{name} sfm={sfm} " + _setenv(monkeypatch, tree_fact, dag, kpan)
        perm, d_ref, pair = _tree_pair(case, sfm, tree_fact == "1", tag, dag, pivot_tol=0.0)
        for k, i in exact_plant_pivots(case.nodes, perm, *_supernodes(case, perm, sfm)):
            for v in EXACT_VALUES:
                vals = plant_pivot(case.Lw, case.good, perm, k, "exact", value=v)
                what = f"{tag} exact {v!r} k={k} in {case.front_of_pivot(perm, k)}"
                fails += pair.fail(vals, k, d_ref, what, stats, check_dk=False)
    _report(f"exact {name} tree_fact={tree_fact}", stats, fails)


@pytest.mark.parametrize("tree_fact", ["1", "0"])
@pytest.mark.parametrize("name", ["big_mixed", "leaf_128_65"])
def test_two_plants_report_the_smaller_index(name, tree_fact, monkeypatch):
    """Two fronts of different subtrees fail in one factorisation (different kernels on big_mixed: a micro
    leaf and a big mid): the code is the smaller index + 1, whichever subtree holds it."""
    case = _case(name)
    stats, fails = _stats(), []
    for sfm, dag, kpan in plant_configs(name, case.nodes, tree_fact == "1"):
        tag = f"{name} sfm={sfm} " + _setenv(monkeypatch, tree_fact, dag, kpan)
        perm, d_ref, pair = _tree_pair(case, sfm, tree_fact == "1", tag, dag)
        for k1, k2, _ in pair_plant_pivots(name, case.nodes, perm, *_supernodes(case, perm, sfm)):
            vals = plant_pivot(case.Lw, plant_pivot(case.Lw, case.good, perm, k1, "tiny", d_ref), perm, k2, "tiny", d_ref)
            what = (f"{tag} pair k1={k1} in {case.front_of_pivot(perm, k1)}, k2={k2} in {case.front_of_pivot(perm, k2)}")
            fails += pair.fail(vals, k1, d_ref, what, stats)
    _report(f"pairs {name} tree_fact={tree_fact}", stats, fails)


@pytest.mark.parametrize("root_async", ["1", "0"])
def test_root_plants(root_async, monkeypatch):
    """The first and last column of the root (the last pivot of all), with the root tail on the side
    stream where the plan has one (info()['root_tail_async'], printed per tree) and without."""
    monkeypatch.setenv("MADIPM_ROOT_ASYNC", root_async)
    stats, fails = _stats(), []
    for name in root_plant_tree_names():
        case = _case(name)
        tag = f"{name} root_async={root_async} " + _setenv(monkeypatch, "1")
        perm, d_ref, pair = _tree_pair(case, 128, True, tag)
        tail = pair.ls.info()["root_tail_async"]
        print(f"\n{name}: root_tail_async={tail} (MADIPM_ROOT_ASYNC={root_async})")
        if name == "root_tail":     # helpers.ROOT_TAIL_TREE: the root alone follows the tree launch
            assert tail == int(root_async), f"{tag}: root_tail_async={tail}"
        for k in (case.N - case.nodes[-1]["w"], case.N - 1):
            assert perm[k] >= case.nodes[-1]["first"]
            vals = plant_pivot(case.Lw, case.good, perm, k, "tiny", d_ref)
            fails += pair.fail(vals, k, d_ref, f"{tag} root k={k} in {case.front_of_pivot(perm, k)}", stats)
    _report(f"root root_async={root_async}", stats, fails)


def test_batched_leaf_column_plants():
    """k_lb_build's check: exact and tiny plants at the first, a middle and the last member of the one
    batched-leaf group of dense_k2(128, 200, 3), and two members at once."""
    K, Lw, members = batched_leaf_problem()
    N = K.shape[0]
    rng = np.random.default_rng(5)
    rhs = np.zeros((3, N))
    rhs[0] = rng.standard_normal(N)
    rhs[1, 0] = 1.0
    rhs[2, N - 1] = 1.0
    stats, fails = _stats(), []
    for tol in (PLANT_TOL, 0.0):
        pair = _Pair(N, Lw, Lw.data.copy(), rhs, (200, 0, 128), None, ordering=0, pivot_tol=tol)
        info = pair.ls.info()
        assert (info["lb_groups"], info["lb_members"]) == (1, 200), info
        perm = pair.perm
        ref = OracleLDL(K, perm)
        assert ref.factorize() == N
        d_ref = ref.diag()
        pair.X_ref = np.stack([ref.solve(b) for b in rhs])
        if tol:
            plants = [(f"tiny member {k}", k, plant_pivot(Lw, Lw.data, perm, k, "tiny", d_ref)) for k in members]
            a, b = members[1], members[2]
            plants.append((f"tiny members {a} and {b}", a,
                           plant_pivot(Lw, plant_pivot(Lw, Lw.data, perm, b, "tiny", d_ref), perm, a, "tiny", d_ref)))
        else:
            plants = [(f"exact {v!r} member {k}", k, plant_pivot(Lw, Lw.data, perm, k, "exact", value=v))
                      for k in members for v in EXACT_VALUES]
        for what, k, vals in plants:
            assert oracle_plant(Lw, vals, perm, tol)[0] == k
            fails += pair.fail(vals, k, d_ref, f"batched leaves pivot_tol={tol}: {what}", stats, check_dk=bool(tol))
    _report("batched leaf columns", stats, fails)


@pytest.mark.parametrize("name", FLIP_TREES)
def test_cholesky_semantics_and_flipped_pivots(name, monkeypatch):
    """Cholesky mode on a quasi-definite tree fails at the first non-positive pivot (k_inertia's check);
    in LDL^T mode a pivot of flipped sign does not fail, and the inertia counts it."""
    from madipm_amd.linear_solver import HIPLDLSolver
    case = _case(name)
    tag = f"{name} " + _setenv(monkeypatch, "1")
    ls = HIPLDLSolver(case.N, case.Lw.indptr, case.Lw.indices, **_opts(128, 0.0, cholesky=True))
    assert_front_tree_plan(ls.info(), case.nodes, 128, True, tag + " cholesky")
    perm = ls.perm()
    d_ref, _ = case.ref(perm)
    kneg = int(np.flatnonzero(d_ref <= 0)[0])
    rc = ls.factorize(_dev(case.good))
    assert rc == kneg + 1, f"{tag}: Cholesky mode returned {rc}, first non-positive pivot {kneg} in {case.front_of_pivot(perm, kneg)}"
    assert not ls.is_factorized()
    d = ls.diag()
    assert np.all(np.abs(d - d_ref) <= PIVOT_TOL * np.abs(d_ref)), "LDL^T goes on past the pivot: all pivots as the oracle's"
    perm2, d_ref2, pair = _tree_pair(case, 128, True, tag, pivot_tol=0.0)
    assert np.array_equal(perm2, perm)
    stats, fails = _stats(), []
    for k, i in flip_plant_pivots(name, case.nodes, perm, *_supernodes(case, perm, 128)):
        what = f"{tag} flip k={k} in {case.front_of_pivot(perm, k)}"
        vals = plant_pivot(case.Lw, case.good, perm, k, "flip", d_ref)
        kbad, d_o, nv = oracle_plant(case.Lw, vals, perm, 0.0)
        assert kbad == -1 and nv == case.N
        rc = pair.ls.factorize(_dev(vals))
        if rc != 0 or not pair.ls.is_factorized():
            fails.append(f"{what}: factorize returned {rc}")
            continue
        d = pair.ls.diag()
        rel = np.abs(d - d_o) / np.abs(d_o)
        if not rel.max() <= PIVOT_TOL:
            kk = int(np.argmax(rel))
            fails.append(f"{what}: pivot {kk} in {case.front_of_pivot(perm, kk)} off the oracle's by {rel.max():.3e}")
        want = (int(np.sum(d_o > 0)), 0, int(np.sum(d_o < 0)))
        assert want != case.inertia
        if pair.ls.inertia() != want:
            fails.append(f"{what}: inertia {pair.ls.inertia()}, the oracle's D has {want}")
        stats["plants"] += 1
        fails += pair.recover(what, stats)
    _report(f"flip {name}", stats, fails)


def test_inertia_beyond_one_grid_pass():
    """N = 20,001 columns: k_inertia's 64 blocks stride over them more than once."""
    from madipm_amd.linear_solver import HIPLDLSolver
    Lw, dvals = signed_diagonal()
    N = Lw.shape[0]
    ls = HIPLDLSolver(N, Lw.indptr, Lw.indices, ordering=0)
    assert ls.factorize(_dev(Lw.data)) == 0 and ls.is_factorized()
    assert ls.inertia() == (int(np.sum(dvals > 0)), 0, int(np.sum(dvals < 0)))
    assert np.array_equal(_bits(ls.diag()), _bits(dvals[ls.perm()]))
