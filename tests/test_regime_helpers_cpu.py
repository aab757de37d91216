"""What the reduction-regime GPU tests (test_step_gpu.py::test_step_regimes and companions,
test_mpc_regimes_gpu.py) rest on, pinned without a GPU:

  * the launch constants of csrc/mpc_kernels.hpp, csrc/mpc.hip and csrc/mpc.hpp are helpers.MPC_CONSTANTS, from which those tests
    derive every boundary: a changed source fails here by name;
  * every size of the tables reaches the regime it is listed for (blocks, finaliser path, stride);
  * regime_problem has n_ + m_ = 3 m + n_ineq rows on the oracle, and its planted row and coordinate are
    the unique extremes: |c_r| after initialize() by a factor >= 4, the only primal ratio below 1 in
    update_step at iteration 1 (and the oracle's i_xl); the dual residual after initialize() takes three
    values only, so no column can be planted;
  * the oracle's own spread s (SuperLU against its LDL^T backend) is <= 3e-9 on every case and k the GPU
    tests compare (asserted by test_mpc_point_gpu._oracle_iterate; printed here);
  * three float64 summation orders of MehrotraAdaptiveStep's mu_full terms for the step test's inputs
    agree within 1e-13, so its 1e-12 bound on the alphas stands at 2.6 M terms.
"""
import math
import os
import re

import numpy as np
import pytest

import oracle.mpc as M
from helpers import (MPC_CONSTANTS, REGIME_FLAT_SIZES, REGIME_G, REGIME_G64_SIZES, REGIME_KS, REGIME_STEP_SIZES,
                     mpc_regime, regime_bounds, regime_case, regime_flat_cases, regime_g64_cases, regime_launches,
                     regime_step_ties, spmv_mean_row)
from oracle.mpc import OracleMPC, OracleOptions, step_on_vectors
from test_mpc_point_gpu import _oracle_iterate
from test_step_gpu import RULES, SIDES, regime_step_vectors

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "madipm.jl_amd", "csrc")
WHO = ("the reduction-regime tests (tests/test_step_gpu.py::test_step_regimes, tests/test_mpc_regimes_gpu.py) "
       "derive their boundaries from helpers.MPC_CONSTANTS: move both together")


def test_source_constants():
    """Each launch constant is defined once, in the file named here: once among the MPC driver's sources
    (csrc/mpc*.hip, csrc/mpc*.hpp) and, but for NT, once in all of csrc/*.hip and csrc/*.hpp (the LDL^T and
    the KKT units have an NT of their own, ldl_plan.hpp and kkt.hip, which the MPC kernels never see)."""
    home = {"NT": "mpc_kernels.hpp", "MAXB": "mpc_kernels.hpp", "FT1": "mpc.hip", "FG": "mpc.hip", "FT": "mpc.hip"}
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp"))}
    for name, where in home.items():
        found = {f: re.findall(r"constexpr int (?:\w+ = \d+, )*%s = (\d+)" % name, text) for f, text in src.items()}
        found = {f: v for f, v in found.items() if v and (f.startswith("mpc") or name != "NT")}
        assert found == {where: [str(MPC_CONSTANTS[name])]}, (
            f"csrc: {name} = {found}, pinned {MPC_CONSTANTS[name]} in {where}; {WHO}")
    found = re.findall(r"\bint maxb_ = (\d+);", src["mpc.hpp"])
    assert found == [str(MPC_CONSTANTS["maxb_"])], f"csrc/mpc.hpp: maxb_ = {found}; {WHO}"
    assert MPC_CONSTANTS["MAXB"] == MPC_CONSTANTS["FG"] * MPC_CONSTANTS["FT"] >= MPC_CONSTANTS["maxb_"]


def test_sizes_reach_their_regimes():
    for n, want in REGIME_STEP_SIZES.items():
        assert mpc_regime(n) == want, (n, mpc_regime(n))
        for a, b in regime_step_ties(n):
            assert 0 <= a < b < n
    assert [v[1:] for v in REGIME_STEP_SIZES.values()] == [("one", False), ("two", False), ("two", False),
                                                           ("two", True), ("two", True)]
    for (m, ni), (rows, fin, strided) in REGIME_G64_SIZES.items():
        assert rows == 3 * m + ni and mpc_regime(rows, REGIME_G)[1:] == (fin, strided)
        assert mpc_regime(rows)[0] < 100                      # the flat kernels: the mixed-count case
    assert [v[0] for v in REGIME_G64_SIZES.values()] == [4096, 4097, 8192, 8193, 20001]
    for (m, ni), (rows, fin, strided, *_) in REGIME_FLAT_SIZES.items():
        assert rows == 3 * m + ni and mpc_regime(rows)[1:] == (fin, strided)
    assert [v[0] for v in REGIME_FLAT_SIZES.values()] == [262144, 262145, 524588]


PROBLEMS = sorted({p for p, _, _ in regime_g64_cases()} | {p for p, _ in regime_flat_cases()})


def _first_step(qp):
    """The oracle's update_step operands and result at iteration 1."""
    rec = []
    orig = M.step_on_vectors

    def spy(rule, mu, *v):
        rec.append((orig(rule, mu, *v), v))
        return rec[-1][0]

    M.step_on_vectors = spy
    try:
        OracleMPC(qp, OracleOptions(regularization=("fixed", 1e-4, -1e-4), max_iter=1)).solve()
    finally:
        M.step_on_vectors = orig
    return rec[0]


@pytest.mark.parametrize("problem", PROBLEMS)
def test_regime_problem_rows_and_plants(problem):
    qp = regime_case(problem)
    _, m, ni, hess, where, _ = problem.split(":")
    m, ni = int(m), int(ni)
    o = OracleMPC(qp, OracleOptions(regularization=("fixed", 1e-4, -1e-4), max_iter=0))
    o.initialize()
    assert o.n + o.m == 3 * m + ni == regime_bounds(qp)[0]
    assert (o.nlb, o.nub) == regime_bounds(qp)[1:] and o.nlb > o.nub and len(o.ind_fixed) == 0
    assert not np.array_equal(o.ind_lb, np.arange(o.nlb)) and not np.array_equal(o.ind_ub, np.arange(o.nub))
    assert o.obj_scale == 1.0 and np.all(o.con_scale == 1.0)
    if int(hess) == 0:
        assert spmv_mean_row(qp)[1] == 4
    # the planted row: the unique largest |c| by a factor >= 4
    hot = qp.hot
    c = np.abs(o.c)
    r = hot["row"]
    assert r == {"first": 0, "last": m - 1}.get(where, r)
    others = float(np.max(np.delete(c, r)))
    assert c[r] >= 4.0 * others > 0.0, (c[r], others)
    # the dual residual after init_starting_point!: three values, nothing to plant
    rd = o.f - o.zl + o.zu + o.jacl
    sh = float(np.max(np.abs(rd)))
    lo_only = np.flatnonzero(np.isfinite(o.xl) & ~np.isfinite(o.xu))
    assert sh > 1.0 and np.all(np.abs(np.abs(rd[lo_only]) - sh) <= 1e-9 * sh)
    assert np.all((np.abs(rd) <= 1e-9 * sh) | (np.abs(np.abs(rd) - sh) <= 1e-9 * sh))
    # the planted coordinate: the only primal ratio below 1 at iteration 1 (no other one binds), by a factor >= 1.5
    res, v = _first_step(qp)
    x_l, xl, _, dx_l, _, x_u, xu, _, dx_u, _ = v
    with np.errstate(divide="ignore", invalid="ignore"):
        rl = np.where(dx_l < 0, (-x_l + xl) / dx_l, np.inf)
        ru = np.where(dx_u > 0, (-x_u + xu) / dx_u, np.inf)
    t = hot["coord"]
    print(f"{problem}: rows {o.n + o.m} nlb {o.nlb} nub {o.nub} launches {regime_launches(qp, REGIME_G)} hot {hot} "
          f"|c_r| {c[r]:.3g} others {others:.3g}; ratio {rl[t] if t is not None else float('nan'):.3f}, others >= "
          f"{min(np.min(np.delete(rl, t)) if t is not None else rl.min(), ru.min()):.3f}")
    if t is None:
        assert where == "first" and ni > 0 and res["i_xl"] == res["i_xu"] == -1
        return
    assert o.ind_lb[t] == hot["col"] and hot["col"] // 2 >= ni
    if where == "last":
        assert hot["col"] == 2 * m - 1 and t == o.nlb - ni - 1       # the last column; the slacks follow
    rest = min(np.min(np.delete(rl, t)), ru.min())
    assert rl[t] <= 0.8 and rest > 1.0 and rest >= 1.5 * rl[t], (rl[t], rest)
    assert res["i_xl"] == t and res["i_xu"] == -1 and res["alpha_p"] < 0.8


@pytest.mark.parametrize("problem,kkt,variant", regime_g64_cases())
def test_oracle_spread_g64(problem, kkt, variant):
    for k in REGIME_KS:
        _, _, spread, tol = _oracle_iterate(problem, kkt, variant, k)      # asserts s <= 3e-9
        print(f"{problem} {kkt} {variant} k={k}: s = {max(spread.values()):.1e}, tol {tol:.1e}")
        assert tol == 1e-9


@pytest.mark.parametrize("problem,ks", regime_flat_cases())
def test_oracle_spread_flat(problem, ks):
    for k in ks:
        _, _, spread, tol = _oracle_iterate(problem, "K2", "default", k)
        print(f"{problem} K2 default k={k}: s = {max(spread.values()):.1e}, tol {tol:.1e}")
        assert tol == 1e-9


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("n", sorted(REGIME_STEP_SIZES))
def test_mu_full_summation_orders(n, side):
    """MehrotraAdaptiveStep's mu_full = sum of (x + a_p dx - xl)(zl + a_d dzl) and its upper twin over the
    step test's own inputs: math.fsum (exact), numpy's pairwise sum and a sequential cumsum agree within
    1e-13 relative, so no summation order of the GPU can use up the alphas' 1e-12."""
    rule, tau, mu = RULES[2]
    vecs, _, _, _ = regime_step_vectors(n, side, 2)
    x_l, xl, zl, dx_l, dzl, x_u, xu, zu, dx_u, dzu = vecs
    ref = step_on_vectors((rule, tau), mu, *vecs)
    ap, ad = min(ref["alpha_xl"], ref["alpha_xu"]), min(ref["alpha_zl"], ref["alpha_zu"])
    terms = np.concatenate([((x_l + ap * dx_l) - xl) * (zl + ad * dzl), (xu - (x_u + ap * dx_u)) * (zu + ad * dzu)])
    exact, pair, seq = math.fsum(terms), float(np.sum(terms)), float(np.cumsum(terms)[-1])
    rel = max(abs(pair - exact), abs(seq - exact), abs(pair - seq)) / abs(exact)
    print(f"mu_full n={n} {side}: {len(terms)} terms, sum {exact:.6e}, spread of three orders {rel:.1e}")
    assert rel <= 1e-13
