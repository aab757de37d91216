"""The generators and the general-form certificate of tests/helpers.py, pinned on the CPU oracle (no
GPU): what tests/test_mpc_point_gpu.py relies on must hold for the reference's own points first.

  * scaled_general: set_scaling! really scales (obj_scale < 1, >= 10 rows with con_scale < 1); the
    oracle solves it with scaling on and off, minimising and maximising; the LP optimum is HiGHS';
  * rowlen_qp: the row-length multiset and the lane-group width class of the mean row;
  * kkt_properties_general: the oracle's points meet the thresholds the GPU points are held to, and
    four corrupted points (each a plausible un-scaling mistake of get_solution) do not.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import (ROWLEN_LENGTHS, assert_certificate, box_qp, free_eq_qp, rowlen_qp, scaled_general,
                     spmv_mean_row)
from oracle.mpc import OracleMPC, OracleOptions, SOLVE_SUCCEEDED

CASES = [(kind, mn, sc) for kind in ("lp", "qp") for mn in (True, False) for sc in (True, False)]


@functools.lru_cache(maxsize=None)
def _oracle(kind, minimize, scaling):
    qp = scaled_general(kind, minimize)
    o = OracleMPC(qp, OracleOptions(regularization=("fixed", 1e-8, -1e-8), max_iter=300, scaling=scaling))
    return qp, o, o.solve()


@pytest.mark.parametrize("kind", ["lp", "qp"])
def test_scaled_general_scales(kind):
    qp, o, st = _oracle(kind, True, True)
    assert o.obj_scale < 1.0
    assert np.sum(o.con_scale < 1.0) >= 10
    assert len(o.ind_fixed) == 2 and qp.c0 == 7.5 and np.any(qp.x0 != 0.0)
    if kind == "lp":    # one-sided and ranged rows, free variables (the QP's rows are equalities, its x boxed)
        assert np.any(np.isinf(qp.ucon)) and np.any(np.isfinite(qp.ucon) & (qp.lcon < qp.ucon))
        assert np.any(np.isinf(qp.lvar)) and np.any(np.isinf(qp.uvar) & np.isfinite(qp.lvar))
    _, o1, _ = _oracle(kind, True, False)
    assert o1.obj_scale == 1.0 and np.all(o1.con_scale == 1.0)


@pytest.mark.parametrize("kind,minimize,scaling", CASES)
def test_scaled_general_solves_and_certifies(kind, minimize, scaling):
    qp, o, st = _oracle(kind, minimize, scaling)
    assert st.status == SOLVE_SUCCEEDED, st.status
    assert_certificate(qp, st, st.objective)
    # maximising the negated objective is the same problem: objective c0 - (min - c0)
    _, _, smin = _oracle(kind, True, scaling)
    want = smin.objective if minimize else 2 * qp.c0 - smin.objective
    assert abs(st.objective - want) <= 1e-9 * abs(want)


def test_scaled_lp_optimum_is_highs():
    from scipy.optimize import linprog
    qp, _, st = _oracle("lp", True, True)
    A = sp.csr_matrix((qp.Avals, (qp.Arows, qp.Acols)), shape=(qp.ncon, qp.nvar))
    eq = qp.lcon == qp.ucon
    up, lo = ~eq & np.isfinite(qp.ucon), ~eq & np.isfinite(qp.lcon)
    r = linprog(qp.c, A_ub=sp.vstack([A[up], -A[lo]]), b_ub=np.concatenate([qp.ucon[up], -qp.lcon[lo]]),
                A_eq=A[eq], b_eq=qp.lcon[eq], method="highs",
                bounds=[(None if np.isinf(l) else l, None if np.isinf(u) else u) for l, u in zip(qp.lvar, qp.uvar)])
    assert r.status == 0
    assert abs(st.objective - (r.fun + qp.c0)) <= 1e-6 * abs(r.fun + qp.c0), (st.objective, r.fun + qp.c0)
    for scaling in (True, False):
        s = _oracle("lp", True, scaling)[2]
        assert abs(s.objective - (r.fun + qp.c0)) <= 1e-6 * abs(r.fun + qp.c0)


@pytest.mark.parametrize("hess,width", [(True, 32), (False, 8)])
def test_rowlen_qp_shape(hess, width):
    qp = rowlen_qp(hess=hess)
    assert (qp.nvar, qp.ncon) == (200, 39)
    A = sp.csr_matrix((qp.Avals, (qp.Arows, qp.Acols)), shape=(39, 200))
    assert sorted(np.diff(A.indptr)) == sorted(ROWLEN_LENGTHS * 3)
    assert np.all(A[:, 0].toarray() != 0.0) and A.T.tocsr().indptr[1] == 39      # column 0: a J^T row of 39
    assert not np.any(qp.lvar == qp.uvar) and np.any(np.isinf(qp.lvar)) and np.any(qp.lcon != qp.ucon)
    mean, g = spmv_mean_row(qp)
    assert g == width and width * 1.02 < mean <= 2 * width / 1.02, (mean, g)   # inside G < mean <= 2 G by 2 %
    if hess:
        H = sp.coo_matrix((qp.Hvals, (qp.Hrows, qp.Hcols)), shape=(200, 200)).tocsr()
        assert np.max(np.diff((H + H.T).tocsr().indptr)) >= 70
    st = OracleMPC(qp, OracleOptions(regularization=("fixed", 1e-4, -1e-4))).solve()
    assert st.status == SOLVE_SUCCEEDED
    assert_certificate(qp, st, st.objective)


def test_degenerate_generators():
    qp, x, y, obj = free_eq_qp()
    for reg in (("none",), ("fixed", 1e-8, -1e-8)):
        o = OracleMPC(qp, OracleOptions(regularization=reg))
        with np.errstate(invalid="ignore"):                       # delta_x2 = 0 / 0 without a bound
            st = o.solve()
        assert o.nlb == o.nub == 0
        assert st.status == SOLVE_SUCCEEDED and st.iter == 2
        assert abs(st.objective - obj) <= 1e-9 * abs(obj)
        assert np.max(np.abs(st.solution - x)) <= 1e-6 and np.max(np.abs(st.multipliers - y)) <= 1e-6
    qb = box_qp()
    st = OracleMPC(qb, OracleOptions(regularization=("fixed", 1e-8, -1e-8), max_iter=300)).solve()
    assert st.status == SOLVE_SUCCEEDED and len(st.multipliers) == len(st.constraints) == 0
    assert_certificate(qb, st, st.objective)


class _Point:
    def __init__(self, st, **kw):
        for f in ("solution", "multipliers", "multipliers_L", "multipliers_U", "constraints"):
            setattr(self, f, np.array(kw.get(f, getattr(st, f)), float))


def _fails(qp, pt, objective):
    try:
        assert_certificate(qp, pt, objective)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("kind,minimize", [("lp", True), ("qp", False)])
def test_certificate_rejects_corrupted_points(kind, minimize):
    qp, o, st = _oracle(kind, minimize, True)
    assert not _fails(qp, _Point(st), st.objective)
    # one multipliers_U entry with the wrong sign
    zu = st.multipliers_U.copy()
    j = int(np.argmax(zu))
    assert zu[j] > 1e-3
    zu[j] = -zu[j]
    assert _fails(qp, _Point(st, multipliers_U=zu), st.objective)
    # y left in the scaled space: one more (or one less) factor con_scale
    assert _fails(qp, _Point(st, multipliers=st.multipliers * o.con_scale), st.objective)
    assert _fails(qp, _Point(st, multipliers=st.multipliers / o.con_scale), st.objective)
    # y without the objective scale
    assert _fails(qp, _Point(st, multipliers=st.multipliers * o.obj_scale), st.objective)
    # zl and zu swapped
    assert _fails(qp, _Point(st, multipliers_L=st.multipliers_U, multipliers_U=st.multipliers_L), st.objective)
    # constraints without the fixed columns' term
    A = sp.csr_matrix((qp.Avals, (qp.Arows, qp.Acols)), shape=(qp.ncon, qp.nvar))
    xf = np.where(qp.lvar == qp.uvar, st.solution, 0.0)
    assert np.max(np.abs(A @ xf)) > 0.0
    assert _fails(qp, _Point(st, constraints=st.constraints - A @ xf), st.objective)
    # constraints left in the scaled space
    assert _fails(qp, _Point(st, constraints=st.constraints * o.con_scale), st.objective)


@pytest.mark.parametrize("reg", [("none",), ("fixed", 1e-8, -1e-8)])
def test_free_eq_qp_pivot_order(reg):
    """free_eq_qp's K2 is dense: the reference's static-pivot LDL^T (the oracle's LDL^T backend) meets the
    pivoting oracle's 2 iterations when x is eliminated before y, and with y first takes pivots of
    delta_d: a third iteration at -1e-8 (solve residuals ~1e-7), no factorization at all at 0."""
    from oracle.mpc import INTERNAL_ERROR, EXC_UNFACTORIZED
    qp, x, y, obj = free_eq_qp()
    n, m = qp.nvar, qp.ncon
    out = {}
    for name, perm in (("x_first", np.arange(n + m)), ("y_first", np.r_[np.arange(n, n + m), np.arange(n)])):
        o = OracleMPC(qp, OracleOptions(regularization=reg))
        o.linear_solver = "ldl"
        o.ldl_perm = perm
        with np.errstate(invalid="ignore"):
            out[name] = (o.solve(), o)
    st, o = out["x_first"]
    assert st.status == SOLVE_SUCCEEDED and st.iter == 2 and max(o.residuals) <= 1e-14
    assert np.max(np.abs(st.solution - x)) <= 1e-6 and abs(st.objective - obj) <= 1e-9 * abs(obj)
    st, o = out["y_first"]
    if reg[0] == "none":
        assert st.status == INTERNAL_ERROR and st.exception == EXC_UNFACTORIZED and st.iter == 0
    else:
        assert st.status == SOLVE_SUCCEEDED and st.iter == 3 and max(o.residuals) >= 1e-8
        assert np.max(np.abs(st.solution - x)) <= 1e-6 and abs(st.objective - obj) <= 1e-9 * abs(obj)
