"""MPCSolver.update: new numbers on an existing solver, without re-analysis.

The oracle of every test is a freshly constructed MPCSolver on the updated problem: same pattern, hence
same ordering, same factorisation schedule and same order of every sum, so every comparison is exact
(np.array_equal on the returned vectors, == on status / iter / objective / dual_objective, and the whole
iteration trace).  test_fresh_solvers_and_second_solve_repeat pins the two facts that rests on."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

from helpers import box_qp, free_eq_qp, scaled_general

pytestmark = pytest.mark.gpu

VECTORS = ("solution", "multipliers", "multipliers_L", "multipliers_U", "constraints")
SCALARS = ("status", "iter", "objective", "dual_objective")
VALUE_FIELDS = ("c", "c0", "Hvals", "Avals", "lcon", "ucon", "lvar", "uvar", "x0", "y0")


def _kw(**extra):
    from madipm_amd import FixedRegularization
    return dict(regularization=FixedRegularization(1e-8, -1e-8), max_iter=300, **extra)


def _kkt(name):
    from madipm_amd import solver as S
    return {"K2": S.SparseKKTSystem, "K25": S.ScaledSparseKKTSystem, "normal": S.NormalKKTSystem}[name]


def _trace_bits(tr):
    return [(t["k"],) + tuple(np.float64(v).tobytes() for k, v in t.items() if k != "k") for t in tr]


def assert_same(a, b):
    for f in VECTORS:                        # equal_nan: a failed solve's NaN is the same NaN on both sides
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    for f in SCALARS:
        x, y = getattr(a, f), getattr(b, f)
        assert x == y or (x != x and y != y), (f, x, y)
    assert len(a.trace) == len(b.trace) and _trace_bits(a.trace) == _trace_bits(b.trace)


def _fresh(qp, **kw):
    from madipm_amd import MPCSolver
    return MPCSolver(qp, **kw).solve()


def _values(qp):
    return {k: getattr(qp, k) for k in VALUE_FIELDS}


def _con_scale(qp, Avals):
    rowmax = np.zeros(qp.ncon)
    np.maximum.at(rowmax, qp.Arows, np.abs(Avals))
    with np.errstate(divide="ignore"):
        return np.minimum(1.0, 100.0 / rowmax)


def perturbed(qp, seed, rows=True):
    """P1 from P0: c, Hvals, Avals times seeded factors in [0.5, 2]; every row of A (and its bounds) times a
    row factor in 10**[-3, 3] that carries con_scale across 1 in both directions; finite bounds shifted
    (lower and upper by the same amount, so a fixed variable stays fixed and an equality row an equality);
    new c0, x0, y0.  The classification of every bound is P0's."""
    rng = np.random.default_rng(seed)
    n, m = qp.nvar, qp.ncon
    rowf = 10.0 ** rng.uniform(-3.0, 3.0, m) if rows else np.ones(m)
    dv, dc = rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, m)
    fixed = qp.lvar == qp.uvar
    dv[fixed] = 0.25                         # the fixed values change, and stay fixed
    new = dict(c=qp.c * rng.uniform(0.5, 2.0, n), c0=-3.25, Hvals=qp.Hvals * rng.uniform(0.5, 2.0, qp.nnzh),
               Avals=qp.Avals * rng.uniform(0.5, 2.0, qp.nnzj) * rowf[qp.Arows],
               lcon=(qp.lcon + dc) * rowf, ucon=(qp.ucon + dc) * rowf, lvar=qp.lvar + dv, uvar=qp.uvar + dv,
               x0=rng.uniform(0.1, 1.0, n), y0=0.1 * rng.standard_normal(m))
    p1 = dataclasses.replace(qp, **new)
    assert np.array_equal(p1.lvar == p1.uvar, fixed) and np.array_equal(p1.lcon == p1.ucon, qp.lcon == qp.ucon)
    assert np.array_equal(np.isfinite(p1.lvar), np.isfinite(qp.lvar))
    assert np.array_equal(np.isfinite(p1.ucon), np.isfinite(qp.ucon))
    return p1


# ------------------------------------------------------------------ what exact comparison rests on
def test_fresh_solvers_and_second_solve_repeat():
    from madipm_amd import MPCSolver
    for kind, kkt in (("lp", "K2"), ("qp", "K25"), ("lp", "normal")):
        qp = scaled_general(kind)
        kw = _kw(kkt_system=_kkt(kkt))
        s = MPCSolver(qp, **kw)
        a = s.solve()
        assert a.status == 1, (kind, kkt, a.status)
        assert_same(a, _fresh(qp, **kw))     # two fresh solvers agree to the bits
        assert_same(a, s.solve())            # a second solve() repeats the first
        assert s.counters() == {"n_analyses": 1, "n_updates": 0, "last_update_s": 0.0}


# ------------------------------------------------------------------ 1. full update, every formulation
@pytest.mark.parametrize("minimize", [True, False], ids=["min", "max"])
@pytest.mark.parametrize("kind,kkt", [("lp", "K2"), ("lp", "K25"), ("lp", "normal"), ("qp", "K2"), ("qp", "K25")])
def test_full_update_matches_fresh_solver(kind, kkt, minimize):
    from madipm_amd import MPCSolver
    p0 = scaled_general(kind, minimize)
    p1 = perturbed(p0, 101)
    cs0, cs1 = _con_scale(p0, p0.Avals), _con_scale(p1, p1.Avals)
    assert np.any((cs0 == 1.0) & (cs1 < 1.0)) and np.any((cs0 < 1.0) & (cs1 == 1.0))
    kw = _kw(kkt_system=_kkt(kkt))
    s = MPCSolver(p0, **kw)
    perm, info = s.kkt_perm(), s.ldl_info()
    a0 = s.solve()
    assert_same(a0, _fresh(p0, **kw))
    given = {k: (np.array(v, copy=True) if k != "c0" else v) for k, v in _values(p1).items()}
    s.update(**given)
    for k in VALUE_FIELDS:                   # the caller's arrays are untouched, self.qp is an updated copy
        assert np.array_equal(given[k], getattr(p1, k)) and np.array_equal(getattr(s.qp, k), getattr(p1, k))
        assert k == "c0" or not np.shares_memory(getattr(s.qp, k), given[k])
    a1 = s.solve()
    assert_same(a1, _fresh(p1, **kw))
    assert not np.array_equal(a1.solution, a0.solution)
    c = s.counters()
    assert c["n_analyses"] == 1 and c["n_updates"] == 1 and c["last_update_s"] > 0.0
    assert np.array_equal(s.kkt_perm(), perm) and s.ldl_info() == info


# ------------------------------------------------------------------ 2. csr_from_coo's corner cases
def corner_qp(fix):
    """12 x 20, written out: A's COO in a shuffled order (neither row- nor column-major) with (2, 4) three
    times (1e3, 1e-14, -1e3: the sum depends on the order), (7, 11) three times (0.1, 0.2, 0.3: it does
    too) and (5, 9) twice — column 9
    being the fixed one when fix; H = I + a diagonal entry given three times + an off-diagonal one given
    twice + entries in row / column 9.  Feasible: the right-hand sides come from a point inside the box."""
    from madipm_amd.qp import QuadraticModel
    m, n = 12, 20
    rows, cols, vals = [], [], []
    for i in range(m):
        for t, j in enumerate(sorted({i, i + 5, (3 * i + 1) % n, 19 - i, (7 * i + 2) % n})):
            if (i, j) in ((2, 4), (7, 11), (5, 9)):
                continue
            rows.append(i), cols.append(j), vals.append(1.0 + 0.25 * t - 0.125 * (i % 3))
    dup = [(2, 4, 1e3), (2, 4, 1e-14), (2, 4, -1e3), (7, 11, 0.1), (7, 11, 0.2), (7, 11, 0.3), (5, 9, 0.3),
           (5, 9, 0.6)]
    assert (1e3 + 1e-14) + -1e3 != (1e3 + -1e3) + 1e-14 and (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
    for i, j, v in dup:
        rows.append(i), cols.append(j), vals.append(v)
    order = np.random.default_rng(4).permutation(len(rows))
    rows, cols, vals = np.array(rows)[order], np.array(cols)[order], np.array(vals)[order]
    assert np.any(np.diff(rows) < 0) and np.any(np.diff(cols) < 0)
    hr = list(range(n)) + [4, 4, 6, 6, 9, 12, 9]
    hc = list(range(n)) + [4, 4, 2, 2, 3, 9, 9]
    hv = [1.0] * n + [0.1, 0.2, 0.3, -0.1, 0.25, 0.5, 0.75]
    rng = np.random.default_rng(8)
    xs = rng.uniform(0.5, 1.5, n)
    b = np.zeros(m)
    np.add.at(b, rows, vals * xs[cols])
    lcon, ucon = b.copy(), b.copy()
    lcon[[1, 6, 10]] -= 1.0
    ucon[[1, 6]] += 1.0
    ucon[10] = np.inf
    lvar, uvar = np.zeros(n), np.full(n, 3.0)
    uvar[[0, 13]] = np.inf
    lvar[14], uvar[14] = -np.inf, np.inf
    if fix:
        lvar[9] = uvar[9] = xs[9]
    return QuadraticModel(c=rng.standard_normal(n), Hrows=hr, Hcols=hc, Hvals=hv, Arows=rows, Acols=cols, Avals=vals,
                          lcon=lcon, ucon=ucon, lvar=lvar, uvar=uvar, c0=1.5, x0=rng.uniform(0.2, 1.0, n),
                          name=f"corner_{'fixed' if fix else 'free'}")


@pytest.mark.parametrize("kkt", ["K2", "K25"])
@pytest.mark.parametrize("fix", [True, False], ids=["fixed_column", "no_fixed"])
def test_duplicates_shuffled_coo_and_fixed_column(fix, kkt):
    from madipm_amd import MPCSolver
    p0 = corner_qp(fix)
    p1 = perturbed(p0, 7, rows=False)
    kw = _kw(kkt_system=_kkt(kkt))
    s = MPCSolver(p0, **kw)
    a0 = s.solve()
    assert_same(a0, _fresh(p0, **kw))
    s.update(**_values(p1))
    assert_same(s.solve(), _fresh(p1, **kw))
    s.update(**_values(p0))                  # back: the cancelling triple and the lone entries as created
    assert_same(s.solve(), a0)
    assert s.counters()["n_analyses"] == 1 and s.counters()["n_updates"] == 2


# ------------------------------------------------------------------ 3. partial updates, round trip
@pytest.mark.parametrize("kind", ["lp", "qp"])
def test_partial_updates_and_round_trip(kind):
    from madipm_amd import MPCSolver
    p0 = scaled_general(kind)
    p1 = perturbed(p0, 23)
    kw = _kw()
    s = MPCSolver(p0, **kw)
    first = s.solve()
    cur = p0
    steps = [("c",), ("lcon", "ucon", "lvar", "uvar"), ("Avals",), ("Hvals",)]
    for fields in steps:
        part = {k: getattr(p1, k) for k in fields}
        cur = dataclasses.replace(cur, **part)
        s.update(**part)
        assert_same(s.solve(), _fresh(cur, **kw))
    s.update(**_values(p0))
    assert_same(s.solve(), first)
    assert s.counters()["n_updates"] == len(steps) + 1 and s.counters()["n_analyses"] == 1


# ------------------------------------------------------------------ 4. rejections leave the solver intact
def test_rejected_updates_leave_the_solver_intact():
    from madipm_amd import MPCSolver
    from madipm_amd._lib import MadIPMError
    qp = scaled_general("lp")
    s = MPCSolver(qp, **_kw())
    ref = s.solve()
    fixed = qp.lvar == qp.uvar
    ineq = qp.lcon != qp.ucon
    j_lo = int(np.flatnonzero(np.isfinite(qp.lvar) & ~fixed)[0])
    j_noup = int(np.flatnonzero(np.isinf(qp.uvar))[0])
    j_free = int(np.flatnonzero(~fixed)[5])
    i_eq, i_rng = int(np.flatnonzero(~ineq)[2]), int(np.flatnonzero(ineq)[1])

    def changed(field, idx, val):
        a = getattr(qp, field).copy()
        a[idx] = val
        return {field: a}

    cases = [("variable", j_lo, changed("lvar", j_lo, -np.inf), "infinite"),      # a finite bound made infinite
             ("variable", j_noup, changed("uvar", j_noup, 1e3), "finite"),        # an infinite bound made finite
             ("variable", 17, changed("uvar", 17, qp.uvar[17] + 1.0), "free"),    # a fixed variable freed
             ("variable", j_free, {"lvar": changed("lvar", j_free, 0.25)["lvar"],
                                   "uvar": changed("uvar", j_free, 0.25)["uvar"]}, "fixed"),  # a free one fixed
             ("constraint", i_eq, changed("ucon", i_eq, qp.ucon[i_eq] + 1.0), "ranged"),
             ("constraint", i_rng, changed("ucon", i_rng, qp.lcon[i_rng]), "equality")]
    for what, idx, upd, word in cases:
        with pytest.raises(MadIPMError) as e:
            s.update(c=2.0 * qp.c, **upd)   # the accepted part of the call must not be installed either
        assert f"{what} {idx} " in str(e.value) and word in str(e.value), str(e.value)
        assert np.array_equal(s.qp.c, qp.c)
        assert_same(s.solve(), ref)
    assert s.counters()["n_updates"] == 0
    for k, bad in (("c", qp.c[:-1]), ("Avals", np.append(qp.Avals, 1.0)), ("lcon", qp.lcon[1:]), ("x0", np.zeros(3))):
        with pytest.raises(ValueError):
            s.update(**{k: bad})
    assert_same(s.solve(), ref)
    s.update(c=qp.c)                         # and a valid one still goes through
    assert_same(s.solve(), ref)


# ------------------------------------------------------------------ 5. degenerate shapes
@pytest.mark.parametrize("name", ["box_qp", "free_eq_qp", "simple_lp"])
def test_degenerate_shapes(name):
    from madipm_amd import MPCSolver, simple_lp
    p0 = {"box_qp": box_qp, "free_eq_qp": lambda: free_eq_qp()[0], "simple_lp": simple_lp}[name]()
    rng = np.random.default_rng(2)
    new = dict(c=p0.c * rng.uniform(0.5, 2.0, p0.nvar), Hvals=p0.Hvals * rng.uniform(0.9, 1.1, p0.nnzh),
               Avals=p0.Avals * rng.uniform(0.5, 2.0, p0.nnzj))
    p1 = dataclasses.replace(p0, **new)
    s = MPCSolver(p0, **_kw())
    a0 = s.solve()
    assert_same(a0, _fresh(p0, **_kw()))
    s.update(**new)
    a1 = s.solve()
    assert_same(a1, _fresh(p1, **_kw()))
    assert a1.objective != a0.objective
    assert s.counters()["n_analyses"] == 1


# ------------------------------------------------------------------ 6. shards on one device
def test_update_on_sharded_solver():
    from madipm_amd import MPCSolver
    from madipm_amd.instances import random_lp
    p0 = random_lp(200, 400, 0.02, 3, ineq_frac=0.3)
    p1 = perturbed(p0, 5, rows=False)
    kw = _kw(nshards=2)
    s = MPCSolver(p0, **kw)
    a0 = s.solve()
    assert a0.status == 1
    assert_same(a0, _fresh(p0, **kw))        # the sharded solve itself repeats
    s.update(**_values(p1))
    assert_same(s.solve(), _fresh(p1, **kw))
    assert s.counters()["n_analyses"] == 1


# ------------------------------------------------------------------ 7. the C entry points, and no cost when unused
def test_entry_points_and_unused_solver():
    from madipm_amd import MPCSolver, _lib as L
    from madipm_amd.solver import QPUpdate, QPStruct
    qp = scaled_general("qp")
    s = MPCSolver(qp, **_kw())
    assert s.counters() == {"n_analyses": 1, "n_updates": 0, "last_update_s": 0.0}
    ref = s.solve()
    # update before prepare_update: an error that names the missing call
    u = QPUpdate()
    assert L.lib.madipm_solver_update(s.h, C.byref(u)) < 0
    assert "madipm_solver_prepare_update" in L.madipm_last_error().decode()
    # other dimensions are refused; the right ones are accepted, twice
    q = QPStruct()
    C.memmove(C.byref(q), C.byref(s._q), C.sizeof(QPStruct))
    q.nnzj -= 1
    assert L.lib.madipm_solver_prepare_update(s.h, C.byref(q)) < 0
    assert L.lib.madipm_solver_prepare_update(s.h, C.byref(s._q)) == 0
    assert L.lib.madipm_solver_prepare_update(s.h, C.byref(s._q)) == 0
    # an update of nothing (every pointer NULL) keeps the problem
    assert L.lib.madipm_solver_update(s.h, C.byref(u)) == 0
    assert_same(s.solve(), ref)
    assert s.counters()["n_updates"] == 1 and s.counters()["n_analyses"] == 1
