"""The warm-start rule, pinned on the CPU oracle (tests/warm_oracle.py).

FixedRegularization(1e-8, -1e-8), weight 0.99, warm point = the public solution of a cold solve.  Iteration
counts of the oracle (cold | warm on the same data | warm after nudged(qp, 1e-3), a 1e-3 relative
perturbation of c, H, A and the finite bounds, with the cold count of the perturbed problem in brackets):

    AFIRO                          8 | 3 | 6 (10)
    scaled_general lp, min / max  10 | 3 | 3 (10)
    scaled_general qp, min / max   8 | 3 | 3 (8)
    rowlen_qp                     14 | 4 | 5 (14)
    box_qp (m = 0)                 7 | 2
    free_eq_qp (no bounds)         2 | 1
    ex10_standin(0, 0.02)         18 | 10                   [slow]
    supportcase10_standin(0, .05) 20 | 11                   [slow]

The assertion is warm.iter < cold.iter, never the counts themselves.
"""
from __future__ import annotations

import dataclasses
import functools
import os

import numpy as np
import pytest

from helpers import box_qp, free_eq_qp, rowlen_qp, scaled_general
from oracle.mpc import OracleMPC, OracleOptions, SOLVE_SUCCEEDED
from warm_oracle import WarmOracleMPC, warm_point, warm_solve

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHT = 0.99


def _opt(**kw):
    return OracleOptions(regularization=("fixed", 1e-8, -1e-8), max_iter=300, **kw)


def _afiro():
    from madipm_amd import read_mps, standard_form_qp
    return standard_form_qp(read_mps(os.path.join(GOLDEN, "afiro.mps")))


def _ex10():
    from madipm_amd.instances import ex10_standin
    return ex10_standin(0, 0.02)


def _sc10():
    from madipm_amd.instances import supportcase10_standin
    return supportcase10_standin(0, 0.05)


PROBLEMS = {"afiro": _afiro,
            "scaled_lp_min": lambda: scaled_general("lp", True), "scaled_lp_max": lambda: scaled_general("lp", False),
            "scaled_qp_min": lambda: scaled_general("qp", True), "scaled_qp_max": lambda: scaled_general("qp", False),
            "rowlen_qp": rowlen_qp, "box_qp": box_qp, "free_eq_qp": lambda: free_eq_qp()[0],
            "ex10_standin": _ex10, "supportcase10_standin": _sc10}
SLOW = ("ex10_standin", "supportcase10_standin")
PERTURBED = ("afiro", "scaled_lp_min", "scaled_lp_max", "scaled_qp_min", "scaled_qp_max", "rowlen_qp")


def _params(names):
    return [pytest.param(n, marks=pytest.mark.slow) if n in SLOW else n for n in names]


@functools.lru_cache(maxsize=None)
def _problem(name):
    return PROBLEMS[name]()


def _cold(qp):
    with np.errstate(invalid="ignore"):
        return OracleMPC(qp, _opt()).solve()


@functools.lru_cache(maxsize=None)
def _cold_of(name):
    return _cold(_problem(name))


def nudged(qp, eps, seed=1):
    """The data of qp moved by a relative eps: c, Hvals, Avals times (1 + eps U[-1, 1]) and every finite
    bound shifted by eps U[-1, 1] max(1, |bound|), lower and upper of one variable / row by the same amount
    (a fixed variable stays fixed, an equality row an equality)."""
    rng = np.random.default_rng(seed)
    n, m = qp.nvar, qp.ncon
    f = lambda k: 1.0 + eps * rng.uniform(-1.0, 1.0, k)
    dv = eps * rng.uniform(-1.0, 1.0, n)
    dc = eps * rng.uniform(-1.0, 1.0, m)
    with np.errstate(invalid="ignore"):
        sv = np.maximum(1.0, np.where(np.isfinite(qp.lvar), np.abs(qp.lvar), np.abs(qp.uvar)))
        sc = np.maximum(1.0, np.where(np.isfinite(qp.lcon), np.abs(qp.lcon), np.abs(qp.ucon)))
    sv, sc = np.where(np.isfinite(sv), sv, 1.0), np.where(np.isfinite(sc), sc, 1.0)
    return dataclasses.replace(qp, c=qp.c * f(n), Hvals=qp.Hvals * f(qp.nnzh), Avals=qp.Avals * f(qp.nnzj),
                               lvar=qp.lvar + dv * sv, uvar=qp.uvar + dv * sv, lcon=qp.lcon + dc * sc,
                               ucon=qp.ucon + dc * sc)


def perturbed(qp, seed, rows=True):
    """tests/test_update_gpu.py's bound-shifting construction: c, Hvals, Avals times seeded factors in
    [0.5, 2]; every row of A (and its bounds) times a row factor in 10**[-3, 3]; finite bounds shifted (lower
    and upper by the same amount); new c0, x0, y0.  The classification of every bound is qp's."""
    rng = np.random.default_rng(seed)
    n, m = qp.nvar, qp.ncon
    rowf = 10.0 ** rng.uniform(-3.0, 3.0, m) if rows else np.ones(m)
    dv, dc = rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, m)
    fixed = qp.lvar == qp.uvar
    dv[fixed] = 0.25
    new = dict(c=qp.c * rng.uniform(0.5, 2.0, n), c0=-3.25, Hvals=qp.Hvals * rng.uniform(0.5, 2.0, qp.nnzh),
               Avals=qp.Avals * rng.uniform(0.5, 2.0, qp.nnzj) * rowf[qp.Arows],
               lcon=(qp.lcon + dc) * rowf, ucon=(qp.ucon + dc) * rowf, lvar=qp.lvar + dv, uvar=qp.uvar + dv,
               x0=rng.uniform(0.1, 1.0, n), y0=0.1 * rng.standard_normal(m))
    p1 = dataclasses.replace(qp, **new)
    assert np.array_equal(p1.lvar == p1.uvar, fixed) and np.array_equal(p1.lcon == p1.ucon, qp.lcon == qp.ucon)
    return p1


def _same_objective(a, b):
    assert abs(a.objective - b.objective) <= 1e-6 * max(1.0, abs(b.objective)), (a.objective, b.objective)


@pytest.mark.parametrize("name", _params(PROBLEMS))
def test_warm_resolve_same_data_takes_fewer_iterations(name):
    qp, cold = _problem(name), _cold_of(name)
    assert cold.status == SOLVE_SUCCEEDED
    o, warm = warm_solve(qp, _opt(), warm_point(cold), WEIGHT)
    print(f"{name}: cold {cold.iter} warm {warm.iter}")
    assert o.n_warm_inits == 1
    assert warm.status == SOLVE_SUCCEEDED
    _same_objective(warm, cold)
    assert warm.iter < cold.iter, (warm.iter, cold.iter)


@pytest.mark.parametrize("name", _params(PERTURBED))
def test_warm_resolve_after_a_small_perturbation(name):
    """The previous solution as the warm point of the problem moved by 1e-3: fewer iterations than the cold
    solve of that problem."""
    qp, cold0 = _problem(name), _cold_of(name)
    p1 = nudged(qp, 1e-3)
    cold1 = _cold(p1)
    assert cold1.status == SOLVE_SUCCEEDED
    _, warm = warm_solve(p1, _opt(), warm_point(cold0), WEIGHT)
    print(f"{name} 1e-3: cold {cold1.iter} warm {warm.iter}")
    assert warm.status == SOLVE_SUCCEEDED
    _same_objective(warm, cold1)
    assert warm.iter < cold1.iter, (warm.iter, cold1.iter)


def _initialized(qp, warm, weight=WEIGHT, **kw):
    o = WarmOracleMPC(qp, _opt(**kw), warm, weight)
    with np.errstate(invalid="ignore"):
        o.initialize()
    return o


@pytest.mark.parametrize("weight", [0.5, 0.99])
@pytest.mark.parametrize("name", ["scaled_lp_min", "scaled_qp_max", "rowlen_qp", "box_qp", "free_eq_qp"])
def test_blended_point_is_strictly_interior_and_blended(name, weight):
    qp, cold = _problem(name), _cold_of(name)
    w = warm_point(cold)        # a converged point: x on its bounds, multipliers at 0 — the guard's ground
    o = _initialized(qp, w, weight)
    assert o.strictly_interior()
    xc, yc, zlc, zuc = o.cold_point
    # y has no interior condition: the blend itself, in the rule's own expression
    yt = w["y"] * o.obj_scale / o.con_scale
    assert np.array_equal(o.y, weight * yt + (1.0 - weight) * yc)
    assert np.array_equal(o.x[o.ind_fixed], o.xl[o.ind_fixed])
    moved = ~np.isclose(o.x, xc, rtol=0, atol=0)
    assert moved.any()
    # evaluate_model! ran at the blended point
    assert np.array_equal(o.c, o.eval_cons(o.x)) and np.array_equal(o.f, o.eval_grad(o.x))
    assert o.obj_val == o.eval_f(o.x)


def test_no_warm_point_is_the_cold_oracle():
    qp = _problem("scaled_qp_min")
    cold = _cold_of("scaled_qp_min")
    o, st = warm_solve(qp, _opt(), None)
    assert o.n_warm_inits == 0 and st.iter == cold.iter and st.objective == cold.objective
    assert np.array_equal(st.solution, cold.solution) and np.array_equal(st.multipliers, cold.multipliers)
    assert [t["inf_du"] for t in st.trace] == [t["inf_du"] for t in cold.trace]


@pytest.mark.parametrize("block", ["x", "y", "zl", "zu"])
def test_absent_blocks_keep_their_cold_values(block):
    qp = _problem("scaled_lp_min")
    w = warm_point(_cold_of("scaled_lp_min"))
    o = _initialized(qp, {block: w[block]})
    xc, yc, zlc, zuc = o.cold_point
    nx = o.nx
    same = dict(x=np.array_equal(o.x, xc), y=np.array_equal(o.y, yc),
                zl=np.array_equal(o.zl[:nx], zlc[:nx]), zu=np.array_equal(o.zu[:nx], zuc[:nx]),
                zs=np.array_equal(o.zl[nx:], zlc[nx:]) and np.array_equal(o.zu[nx:], zuc[nx:]))
    changed = {"x": {"x"}, "y": {"y", "zs"}, "zl": {"zl"}, "zu": {"zu"}}[block]
    for k, v in same.items():
        assert v == (k not in changed), (block, k)
    assert o.strictly_interior() and o.n_warm_inits == 1


def test_warm_x_outside_shifted_bounds_is_clamped():
    """The solution of P0 as the warm point of P1 = perturbed(P0): bounds shifted by up to 0.05 (fixed values
    by 0.25), rows rescaled by 10**[-3, 3].  Every x at a bound of P0 is outside or on P1's."""
    p0 = _problem("scaled_lp_min")
    p1 = perturbed(p0, 101)
    w = warm_point(_cold_of("scaled_lp_min"))
    assert np.any(w["x"] < p1.lvar) and np.any(w["x"] > p1.uvar)
    for weight in (0.5, 0.99):
        o = _initialized(p1, w, weight)
        assert o.strictly_interior()
        nx = o.nx
        xc = o.cold_point[0]
        xt = np.clip(w["x"], o.xl[:nx], o.xu[:nx])
        out = (w["x"] < o.xl[:nx]) | (w["x"] > o.xu[:nx])
        free = ~o._fixed_mask[:nx]
        exp = weight * xt + (1.0 - weight) * xc[:nx]
        assert np.array_equal(o.x[:nx][free], exp[free])
        assert np.all(np.abs(o.x[:nx][out & free] - xt[out & free]) <= (1.0 - weight) * np.abs(xc[:nx] - xt)[out & free] + 1e-15)
        fx = np.flatnonzero(p1.lvar == p1.uvar)
        assert np.array_equal(o.x[fx], p1.lvar[fx])
    cold1 = _cold(p1)
    _, warm = warm_solve(p1, _opt(), w, WEIGHT)
    assert warm.status == cold1.status == SOLVE_SUCCEEDED
    _same_objective(warm, cold1)
