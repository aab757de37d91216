"""The oracle of the sensitivities at the polished point (polished_sens_oracle.py) against central
differences of polish_oracle.exact with the set held fixed, its transpose identity, the restated device
algorithm against the dense derivative (the condition under which the GPU's cap is fair), the coverage the
fixtures of test_polished_sens_gpu.py must give, and the argument checks and C interface of polished=True —
all without a GPU."""
from __future__ import annotations

import numpy as np
import pytest

import adjoint_full_oracle as F
import adjoint_oracle as O
import polish_oracle as P
import polished_sens_oracle as Q
import tangent_oracle as T
from helpers import box_qp, free_eq_qp

MU_IPM = 1e-9            # the end point the solver returns sits at about this mu

# The problems test_polished_sens_gpu.py solves (test_polish_gpu.FIXTURES), with the largest err over the five
# blocks of the oracle's tangent along directions(qp, 0), all seven blocks together and each alone (the sparse
# QP: together only), against central differences (h = 1e-6) of polish_oracle.exact on the guessed set, as
# measured with this file: rounding of the difference quotient (the scaled family's entries are 1e3).  The
# bound is 10 x the value, capped at 1e-6.
GPU_FIXTURES = {
    "family_0": (lambda: O.family(0)[0], 3.9e-10),
    "family_1": (lambda: O.family(1)[0], 4.3e-10),
    "family_2": (lambda: O.family(2)[0], 3.3e-10),
    "family_3": (lambda: O.family(3)[0], 5.3e-10),
    "family_max": (lambda: O.family(0, minimize=False)[0], 3.9e-10),
    "family_dup": (lambda: O.duplicated_family(0)[0], 2.8e-10),
    "family_scaled": (lambda: O.scaled_family(0)[0], 7.2e-8),
    "lp": (lambda: O.lp_fixture()[0], 2.8e-10),
    "sparse_g64": (lambda: O.sparse_fixture()[0], 8.0e-11),
    "rowlength_g4": (lambda: F.rowlength_fixture()[0], 4.2e-10),
    "no_bounds": (lambda: free_eq_qp()[0], 5.1e-10),
    "no_rows": (box_qp, 3.9e-10),
}
FD_CAP = 1e-6
RESTATED_TOL = 1e-11     # the restated device algorithm against the dense derivative
_solved = {}


def solved(name):
    """(qp, guessed set, directions, cotangents) of a fixture, computed once and never modified."""
    if name not in _solved:
        qp = GPU_FIXTURES[name][0]()
        av, ar = P.guess(qp, O.reference_ipm(qp, mu_end=MU_IPM))
        gx = np.random.default_rng(4100).uniform(0.5, 1.5, qp.nvar)
        _solved[name] = (qp, (av, ar), T.directions(qp, 0), F.cotangents(qp, gx))
    return _solved[name]


def test_fixtures_are_the_gpu_tests():
    pytest.importorskip("torch")
    import test_polish_gpu as G
    assert set(GPU_FIXTURES) == set(G.FIXTURES)
    for name in ("family_3", "rowlength_g4", "no_rows"):
        a, b = GPU_FIXTURES[name][0](), G.FIXTURES[name][0]()[0]
        assert np.array_equal(a.c, b.c) and np.array_equal(a.Avals, b.Avals) and np.array_equal(a.lvar, b.lvar)


@pytest.mark.parametrize("name", list(GPU_FIXTURES))
def test_tangent_matches_central_differences(name):
    qp, st, d, _ = solved(name)
    measured = GPU_FIXTURES[name][1]
    t, fd = Q.tangent(qp, *st, d), Q.finite_difference(qp, *st, d, h=1e-6)
    e = {k: O.err(t[k], fd[k]) for k in T.OUTS}
    print(name, "fd", {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e.values()) <= min(10.0 * measured, FD_CAP), e
    if name != "sparse_g64":      # each direction block alone (two dense solves of 2180 unknowns per block there)
        for k in T.NAMES:
            tk, fk = Q.tangent(qp, *st, T.only(d, k)), Q.finite_difference(qp, *st, T.only(d, k), h=1e-6)
            assert Q.max_err(tk, fk, T.OUTS) <= min(10.0 * measured, FD_CAP), k


@pytest.mark.parametrize("name", ["family_0", "family_1", "family_3", "family_scaled", "lp", "sparse_g64"])
def test_face_derivative_is_the_limit_of_the_interior_point_tangent(name):
    """The existing tangent at reference_ipm's optimum (mu = 1e-11) approximates the face derivative: measured
    <= 4.8e-8 (family_1), the distance of that central-path point from the face."""
    qp, st, d, _ = solved(name)
    e = Q.max_err(Q.tangent(qp, *st, d), T.reference_tangent(qp, O.reference_ipm(qp), d), T.OUTS)
    print(name, "ipm", f"{e:.1e}")
    assert e <= 4.8e-7


@pytest.mark.parametrize("name", list(GPU_FIXTURES))
def test_tangent_is_the_transpose_of_the_adjoint(name):
    """<cot, tangent(d)> = <adjoint(cot), d>: two dense solves with the same matrix, rounding only (measured
    <= 6.1e-16)."""
    qp, st, d, cot = solved(name)
    t, g = Q.tangent(qp, *st, d), Q.adjoint(qp, *st, cot)
    a, b = T.dot(cot, t), T.dot_data(g, qp, d)
    print(name, a, b, f"{abs(a - b) / max(1.0, abs(a)):.1e}")
    assert abs(a - b) <= 1e-12 * max(1.0, abs(a))
    if name == "family_3":        # each cotangent alone against each direction block alone
        for c in F.COTS:
            gc = Q.adjoint(qp, *st, F.only(cot, c))
            for k in T.NAMES:
                tk = Q.tangent(qp, *st, T.only(d, k))
                a, b = T.dot(F.only(cot, c), tk), T.dot_data(gc, qp, T.only(d, k))
                assert abs(a - b) <= 1e-12 * max(1.0, abs(a)), (c, k)


@pytest.mark.parametrize("name", list(GPU_FIXTURES))
def test_restated_algorithm_meets_the_dense_derivative(name):
    """The penalised factor as a preconditioner, the masked residual, 1 + refine_steps solves: within 1e-11 of
    the dense derivative on every fixture the GPU tests use (measured: <= 7.1e-14, the scaled family; <= 2.7e-15
    on the others), with a final residual <= 1.2e-12 in the public space."""
    qp, st, d, cot = solved(name)
    it, ia = {}, {}
    et = Q.max_err(Q.tangent(qp, *st, d, dense=False, info=it), Q.tangent(qp, *st, d), T.OUTS)
    ea = Q.max_err(Q.adjoint(qp, *st, cot, dense=False, info=ia), Q.adjoint(qp, *st, cot), O.NAMES)
    print(name, "restated", f"{et:.1e} {ea:.1e}", "residual", f"{it['residual']:.1e} {ia['residual']:.1e}")
    assert et <= RESTATED_TOL and ea <= RESTATED_TOL
    assert it["residual"] <= 1e-11 and ia["residual"] <= 1e-11
    # one solve is not enough (the penalty's 1 / sigma and the regularisation remain), which is what the count is for
    if name == "family_3":
        one = Q.max_err(Q.tangent(qp, *st, d, dense=False, refine_steps=0), Q.tangent(qp, *st, d), T.OUTS)
        assert one > 1e-11


def test_every_direction_reaches_every_output_and_every_cotangent_every_gradient():
    """For every direction block and every output block some fixture has that block's contribution alone >= 1e-2
    of the output's largest entry (all seven given), and likewise every cotangent and every gradient: a dropped
    block or term cannot hide under the cap of 1e-10."""
    best = {(k, o): 0.0 for k in T.NAMES for o in T.OUTS}
    bestg = {(c, k): 0.0 for c in F.COTS for k in O.NAMES}
    for name in ("family_3", "sparse_g64", "family_1", "rowlength_g4"):
        qp, st, d, cot = solved(name)
        full, fullg = Q.tangent(qp, *st, d), Q.adjoint(qp, *st, cot)
        for k in T.NAMES:
            t = Q.tangent(qp, *st, T.only(d, k))
            for o in T.OUTS:
                if np.any(full[o]):
                    best[(k, o)] = max(best[(k, o)], float(np.max(np.abs(t[o])) / np.max(np.abs(full[o]))))
        for c in F.COTS:
            g = Q.adjoint(qp, *st, F.only(cot, c))
            for k in O.NAMES:
                if np.any(fullg[k]):
                    bestg[(c, k)] = max(bestg[(c, k)], float(np.max(np.abs(g[k])) / np.max(np.abs(fullg[k]))))
    print({f"{k}->{o}": f"{v:.1e}" for (k, o), v in best.items()})
    print({f"{c}->{k}": f"{v:.1e}" for (c, k), v in bestg.items()})
    assert min(best.values()) >= 1e-2, {k: v for k, v in best.items() if v < 1e-2}
    assert min(bestg.values()) >= 1e-2, {k: v for k, v in bestg.items() if v < 1e-2}


def test_exact_properties_and_what_is_not_read():
    qp, (av, ar), d, cot = solved("family_3")
    fixed, eq = qp.lvar == qp.uvar, qp.lcon == qp.ucon
    assert fixed.any() and eq.any() and np.any(av != 0) and np.any(ar != 0)
    t = Q.tangent(qp, av, ar, d)
    assert np.array_equal(t["x"][av < 0], d["lvar"][av < 0]) and np.array_equal(t["x"][av > 0], d["uvar"][av > 0])
    assert np.array_equal(t["x"][fixed], d["lvar"][fixed])
    assert np.array_equal(t["cons"][ar < 0], d["lcon"][ar < 0]) and np.array_equal(t["cons"][ar > 0], d["ucon"][ar > 0])
    assert np.max(np.abs(t["cons"][eq] - d["lcon"][eq])) <= 1e-12
    assert not np.any(t["zl"][av >= 0]) and not np.any(t["zu"][av <= 0])
    tn = Q.tangent(qp, av, ar, T.with_nan(qp, d))
    for k in T.OUTS:
        assert np.array_equal(t[k], tn[k]), k
    g = Q.adjoint(qp, av, ar, cot)
    assert not np.any(g["lvar"][(av >= 0) & ~fixed]) and not np.any(g["uvar"][av <= 0])
    assert not np.any(g["lcon"][(ar >= 0) & ~eq]) and not np.any(g["ucon"][ar <= 0])


# ------------------------------------------------------------------ the argument checks and the C interface
def test_abi():
    import ctypes as C
    from madipm_amd import _lib as L
    assert L.madipm_version() == 203       # additive: the version number of the 0.2 line stays
    for f in ("madipm_solver_tangent_polished", "madipm_solver_tangent_polished_device",
              "madipm_solver_adjoint_polished", "madipm_solver_adjoint_polished_device",
              "madipm_solver_polished_sens_info"):
        assert hasattr(L.lib, f), f
    assert L.lib.madipm_solver_tangent_polished(None, C.byref(L.QPDir()), C.byref(L.QPTan())) < 0
    assert b"null handle" in L.madipm_last_error()
    assert L.lib.madipm_solver_adjoint_polished_device(None, C.byref(L.QPCot()), C.byref(L.QPGrad()), None) < 0
    assert b"null handle" in L.madipm_last_error()
    assert L.lib.madipm_solver_polished_sens_info(None, None, None, None, None) < 0
    assert b"null handle" in L.madipm_last_error()


class _NoLibrary:
    """MPCSolver's methods on an object without a handle: an argument check that let a call through would fail
    on `h`, not return."""

    def __init__(self, qp):
        self.qp = qp
        self._device = None


def test_polished_argument_checks_come_before_the_library():
    import inspect
    from madipm_amd import MPCSolver
    qp, _, d, cot = solved("family_3")
    s = _NoLibrary(qp)
    s._adjoint_sizes = lambda: MPCSolver._adjoint_sizes(s)
    s._tangent_sizes = lambda: MPCSolver._tangent_sizes(s)
    for fn in (MPCSolver.tangent, MPCSolver.tangent_device, MPCSolver.adjoint, MPCSolver.adjoint_device):
        p = inspect.signature(fn).parameters["polished"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    with pytest.raises(ValueError, match="tangent: no direction given"):
        MPCSolver.tangent(s, polished=True)
    with pytest.raises(ValueError, match="unknown name"):
        MPCSolver.tangent(s, want=["s"], polished=True, c=d["c"])
    with pytest.raises(ValueError, match=r"Avals has shape \(3,\)"):
        MPCSolver.tangent(s, polished=True, Avals=np.ones(3))
    with pytest.raises(TypeError, match="torch tensor"):
        MPCSolver.tangent_device(s, polished=True, c=d["c"])
    with pytest.raises(ValueError, match="adjoint: no cotangent given"):
        MPCSolver.adjoint(s, polished=True)
    with pytest.raises(ValueError, match="want is empty"):
        MPCSolver.adjoint(s, cot["gx"], want=[], polished=True)
    with pytest.raises(ValueError, match="gy has shape"):
        MPCSolver.adjoint(s, polished=True, gy=np.ones(qp.ncon + 1))
    with pytest.raises(TypeError, match="torch tensor"):
        MPCSolver.adjoint_device(s, cot["gx"], polished=True)


def test_layer_with_a_stand_in_solver():
    """QPLayer(polish=True) polishes after the solve, returns the polished blocks, raises on another verdict and
    passes polished=True to backward's and jvp's calls; the default layer passes no such keyword."""
    torch = pytest.importorskip("torch")
    import torch.autograd.forward_ad as fw
    from madipm_amd import MadIPMError, PolishVerdict, QPLayer
    from madipm_amd import solver as S
    n = {"x": 3, "y": 2, "zl": 3, "zu": 3, "cons": 2}

    class Stats:
        status = S.SOLVE_SUCCEEDED

    class StandIn:
        verdict = PolishVerdict.POLISHED

        def __init__(self):
            self.calls = []

        def update_device(self, **kw):
            self.calls.append(("update", sorted(kw)))

        def solve(self, fetch_solution=False):
            self.calls.append(("solve",))
            return Stats

        def solution_device(self):
            self.calls.append(("solution",))
            return {k: torch.zeros(v, dtype=torch.float64) for k, v in
                    zip(("solution", "multipliers", "multipliers_L", "multipliers_U", "constraints"), n.values())}

        def polish_device(self, want=None):
            self.calls.append(("polish", tuple(want)))
            out = {k: torch.full((n[k],), 1.0 + i, dtype=torch.float64) for i, k in enumerate(n) if k in want}
            out["info"] = {"verdict": self.verdict}
            return out

        def tangent_device(self, want=None, **d):
            self.calls.append(("tangent", tuple(want), sorted(d)))
            return {k: torch.full((n[k],), 10.0 + i, dtype=torch.float64) for i, k in enumerate(n) if k in want}

        def adjoint_device(self, gx=None, want=None, **kw):
            self.calls.append(("adjoint", gx is not None, tuple(want), sorted(kw)))
            return {k: torch.full((3,), 20.0, dtype=torch.float64) for k in want}

    s = StandIn()
    c = torch.arange(3, dtype=torch.float64).requires_grad_(True)
    x, zl = QPLayer(s, outputs=("x", "zl"), polish=True)(c=c)
    assert s.calls == [("update", ["c"]), ("solve",), ("polish", ("x", "zl"))]
    assert float(x.detach()[0]) == 1.0 and float(zl.detach()[0]) == 3.0
    (x.sum() + zl.sum()).backward()
    assert s.calls[-1] == ("adjoint", True, ("c",), ["gzl", "polished"]) and float(c.grad[0]) == 20.0
    s.calls.clear()
    with fw.dual_level():
        x = QPLayer(s, polish=True)(c=fw.make_dual(c.detach(), torch.ones(3, dtype=torch.float64)))
        assert s.calls == [("update", ["c"]), ("solve",), ("polish", ("x",)), ("tangent", ("x",), ["c", "polished"])]
        assert float(fw.unpack_dual(x).tangent[0]) == 10.0
    for verdict in (PolishVerdict.WRONG_SET, PolishVerdict.NO_CONVERGENCE, PolishVerdict.FACTORIZATION_FAILED):
        s.verdict = verdict
        with pytest.raises(MadIPMError, match=f"verdict {verdict.name}, not POLISHED"):
            QPLayer(s, polish=True)(c=c)
    # the default layer: no polish, no keyword
    s = StandIn()
    c = torch.arange(3, dtype=torch.float64).requires_grad_(True)
    for layer in (QPLayer(s, outputs=("x", "zl")), QPLayer(s, outputs=("x", "zl"), polish=False)):
        s.calls.clear()
        x, zl = layer(c=c)
        (x.sum() + zl.sum()).backward()
        assert s.calls == [("update", ["c"]), ("solve",), ("solution",), ("adjoint", True, ("c",), ["gzl"])]
