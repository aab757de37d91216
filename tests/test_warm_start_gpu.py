"""Warm start on the GPU: MPCSolver.warm_start / warm_start_device / warm_start_last / clear_warm_start /
warm_info.

Two oracles.  Where the statement is "the same computation by another route" (a cleared point against a
fresh solver, the host route against the device route against warm_start_last, two runs) the comparison is
exact: test_update_gpu's assert_same, the five vectors, the scalars and the whole trace, bit for bit.  Where
it is "the rule", the reference is tests/warm_oracle.py (the CPU oracle with the rule restated), under
test_mpc_point_gpu's tolerance: |gpu - ref| <= tol max(1, |ref|_inf) per vector and statistic with
tol = max(1e-9, 30 s), s the oracle's own spread on that case (SuperLU against its LDL^T backend), s <= 3e-9
required.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

from helpers import box_qp, free_eq_qp, rowlen_qp, scaled_general  # noqa: E402
from test_mpc_gpu import _oracle_opts  # noqa: E402
from test_mpc_point_gpu import SCALARS, VECTORS, _diff, _point, _reg  # noqa: E402
from test_update_gpu import _kkt, _kw, _values, assert_same, perturbed  # noqa: E402
from warm_oracle import WarmOracleMPC, warm_point  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCKS = ("x", "y", "zl", "zu")


def tiny_lp():
    """One variable, one (ranged) row: min x, 1 <= 2 x <= 3, 0 <= x <= 4."""
    from madipm_amd.qp import QuadraticModel
    return QuadraticModel(c=[1.0], Hrows=[], Hcols=[], Hvals=[], Arows=[0], Acols=[0], Avals=[2.0], lcon=[1.0],
                          ucon=[3.0], lvar=[0.0], uvar=[4.0], x0=[1.0], name="tiny_lp")


PROBLEMS = {"scaled_lp_min": lambda: scaled_general("lp", True), "scaled_lp_max": lambda: scaled_general("lp", False),
            "scaled_qp_min": lambda: scaled_general("qp", True), "scaled_qp_max": lambda: scaled_general("qp", False),
            "rowlen_qp": rowlen_qp, "box_qp": box_qp, "free_eq_qp": lambda: free_eq_qp()[0], "tiny_lp": tiny_lp}
LPS = ("scaled_lp_min", "scaled_lp_max", "tiny_lp")
# free_eq_qp's K2 is dense: every fill-reducing order ties, and the oracle's answer is the natural order's
# (test_mpc_point_gpu.test_degenerate_shapes)
EXTRA = {"free_eq_qp": dict(ordering=0)}


@functools.lru_cache(maxsize=None)
def _problem(name):
    return PROBLEMS[name]()


def _dev(v):
    return torch.as_tensor(np.ascontiguousarray(v, np.float64), device="cuda")


def _solver(qp, **kw):
    from madipm_amd import MPCSolver
    return MPCSolver(qp, **kw)


def _gpu_kw(name, **kw):
    return dict(kw, **EXTRA.get(name, {}))


def _oracle_run(qp, kw, warm, weight, backend="superlu"):
    o = WarmOracleMPC(qp, _oracle_opts(kw), warm, weight)
    o.linear_solver = backend
    with np.errstate(invalid="ignore"):
        st = o.solve()
    t = st.trace[-1]
    assert t["k"] == st.iter
    return o, st, _point(st, dict(objective=st.objective, dual_objective=o.dual_objective() / o.obj_scale,
                                  inf_pr=t["inf_pr"], inf_du=t["inf_du"], inf_compl=t["inf_compl"], mu=t["mu"]))


def _gpu_stats_point(st):
    t = st.trace[-1]
    assert t["k"] == st.iter
    return _point(st, dict(objective=st.objective, dual_objective=st.dual_objective, inf_pr=st.primal_feas,
                           inf_du=st.dual_feas, inf_compl=st.inf_compl, mu=t["mu"]))


@functools.lru_cache(maxsize=None)
def _oracle_solution(name, delta):
    """The oracle's cold converged point of the problem: the warm point of the parity tests (computed without
    the GPU)."""
    kw = dict(regularization=_reg(delta), max_iter=300)
    _, st, _ = _oracle_run(_problem(name), kw, None, 0.5)
    assert st.status == 1, (name, st.status)
    return warm_point(st)


@functools.lru_cache(maxsize=None)
def _oracle_start(name, kkt, weight, blocks):
    """The warm oracle's starting point (max_iter = 0), its own spread and the tolerance from it."""
    qp = _problem(name)
    kw = dict(regularization=_reg(1e-4), kkt_system=_kkt(kkt), max_iter=0)
    full = _oracle_solution(name, 1e-4)
    warm = {k: full[k] for k in blocks}
    o, st, ref = _oracle_run(qp, kw, warm, weight)
    _, st2, alt = _oracle_run(qp, kw, warm, weight, backend="ldl")
    assert o.n_warm_inits == 1 and st.iter == st2.iter == 0 and o.strictly_interior()
    spread = _diff(alt, ref)
    s = max(spread.values())
    assert s <= 3e-9, (name, kkt, weight, blocks, spread)
    return warm, ref, spread, max(1e-9, 30.0 * s)


def _check_start(name, kkt, weight, blocks):
    from madipm_amd import MAXIMUM_ITERATIONS_EXCEEDED
    warm, ref, spread, tol = _oracle_start(name, kkt, weight, blocks)
    s = _solver(_problem(name), **_gpu_kw(name, regularization=_reg(1e-4), kkt_system=_kkt(kkt), max_iter=300))
    s.warm_start(weight=weight, **warm)
    s.set_max_iter(0)
    st = s.solve()
    assert st.status == MAXIMUM_ITERATIONS_EXCEEDED and st.iter == 0 and len(st.trace) == 1
    assert s.warm_info() == {"active": True, "weight": weight, "n_warm_inits": 1}
    d = _diff(_gpu_stats_point(st), ref)
    print(f"warm start {name} {kkt} w={weight} blocks={''.join(b[-1] for b in blocks)} tol={tol:.1e} | " +
          " ".join(f"{f}={d[f]:.1e}/{spread[f]:.1e}" for f in VECTORS + SCALARS))
    for f in VECTORS + SCALARS:
        assert d[f] <= tol, (name, kkt, weight, blocks, f, d[f], tol, spread[f])
    return st, ref


# ------------------------------------------------------------------ 1. cold is untouched
@pytest.mark.parametrize("name,kkt", [("scaled_lp_min", "K2"), ("scaled_qp_max", "K25"), ("scaled_lp_max", "normal"),
                                      ("box_qp", "K2"), ("free_eq_qp", "K2")])
def test_set_then_cleared_is_the_cold_solver(name, kkt):
    qp = _problem(name)
    kw = _gpu_kw(name, **_kw(kkt_system=_kkt(kkt)))
    ref = _solver(qp, **kw).solve()
    s = _solver(qp, **kw)
    assert s.warm_info() == {"active": False, "weight": 0.0, "n_warm_inits": 0}
    s.warm_start(weight=0.9, **warm_point(ref))
    assert s.warm_info() == {"active": True, "weight": 0.9, "n_warm_inits": 0}
    s.clear_warm_start()
    assert s.warm_info() == {"active": False, "weight": 0.0, "n_warm_inits": 0}
    assert_same(s.solve(), ref)
    # and after a warm solve as well: the point is gone with clear, nothing of it stays in the solver
    s.warm_start_last()
    w = s.solve()
    assert w.status == 1 and s.warm_info()["n_warm_inits"] == 1
    s.clear_warm_start()
    assert_same(s.solve(), ref)
    assert s.warm_info() == {"active": False, "weight": 0.0, "n_warm_inits": 1}
    assert s.counters()["n_analyses"] == 1


# ------------------------------------------------------------------ 2. start-point parity with the warm oracle
@pytest.mark.parametrize("weight", [0.5, 0.99])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_start_point_matches_warm_oracle(name, weight, monkeypatch):
    """set_max_iter(0): x, y, zl, zu, the constraint values and the iteration-0 record of a warm start from the
    oracle's converged point, element-wise against the warm oracle."""
    monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    st, ref = _check_start(name, "K2", weight, BLOCKS)
    # the blend did move the start: the cold one is further than the tolerance from it
    cold = _solver(_problem(name), **_gpu_kw(name, regularization=_reg(1e-4), max_iter=0)).solve()
    assert any(np.max(np.abs(getattr(cold, f) - getattr(st, f)), initial=0.0) > 1e-6 for f in VECTORS)


@pytest.mark.parametrize("kkt", ["K25", "normal"])
def test_start_point_other_formulations(kkt, monkeypatch):
    monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    for name in ("scaled_lp_max", "tiny_lp") + (("rowlen_qp",) if kkt == "K25" else ()):
        _check_start(name, kkt, 0.99, BLOCKS)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("name", ["scaled_lp_min", "rowlen_qp"])
def test_start_point_single_block(name, block, monkeypatch):
    """One block alone: the others keep their cold values (the slack values follow x, the slack multipliers y)."""
    monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    st, _ = _check_start(name, "K2", 0.5, (block,))
    cold = _solver(_problem(name), regularization=_reg(1e-4), max_iter=0).solve()
    field = dict(x="solution", y="multipliers", zl="multipliers_L", zu="multipliers_U")
    for b, f in field.items():
        same = np.array_equal(getattr(st, f), getattr(cold, f))
        assert same == (b != block), (block, f)


@pytest.mark.parametrize("G", [4, 16, 64])
def test_start_point_row_kernel_widths(G, monkeypatch):
    """k_warm_rows at other lane-group widths than the heuristic's, on rowlen_qp's rows of 1 .. 131 entries."""
    monkeypatch.setenv("MADIPM_SPMV_G", str(G))
    _check_start("rowlen_qp", "K2", 0.99, BLOCKS)


# ------------------------------------------------------------------ 3. convergence
def _conv_cases():
    out = []
    for name in PROBLEMS:
        kinds = ("K2", "K25", "normal") if name in LPS else ("K2", "K25")
        out += [(name, k) for k in kinds]
    return out


@pytest.mark.parametrize("name,kkt", _conv_cases())
def test_warm_resolve_converges_in_fewer_iterations(name, kkt):
    qp = _problem(name)
    kw = _gpu_kw(name, **_kw(kkt_system=_kkt(kkt)))
    s = _solver(qp, **kw)
    cold = s.solve()
    assert cold.status == 1
    w = warm_point(cold)
    s.warm_start(**w)                        # weight 0.99, the default
    warm = s.solve()
    _, ost, _ = _oracle_run(qp, kw, w, 0.99)
    print(f"{name} {kkt}: cold {cold.iter} warm {warm.iter} warm oracle {ost.iter}")
    assert warm.status == 1 and ost.status == 1
    assert abs(warm.objective - cold.objective) <= 1e-6 * max(1.0, abs(cold.objective))
    assert abs(warm.iter - ost.iter) <= 1, (warm.iter, ost.iter)
    assert warm.iter < cold.iter, (warm.iter, cold.iter)
    assert s.warm_info()["n_warm_inits"] == 1 and s.counters()["n_analyses"] == 1


# ------------------------------------------------------------------ 4. the loop: three routes, one result
def _dvalues(qp):
    from test_update_gpu import VALUE_FIELDS
    return {k: (float(qp.c0) if k == "c0" else _dev(getattr(qp, k))) for k in VALUE_FIELDS}


@pytest.mark.parametrize("nshards", [1, 2])
@pytest.mark.parametrize("kind", ["lp", "qp"])
def test_resolve_loop_routes_agree(kind, nshards):
    """update_device(perturbed(p0)) -> warm_start_last() -> solve() on one solver, against a fresh solver on
    the perturbed problem that is given the same point through the host warm_start, and a third that gets
    it through warm_start_device: exactly equal."""
    p0 = scaled_general(kind)
    p1 = perturbed(p0, 101)
    kw = _kw(**({"nshards": nshards} if nshards > 1 else {}))
    s = _solver(p0, **kw)
    assert s.solve().status == 1
    s.update_device(**_dvalues(p1))
    pt = s.solution_device()                 # the bits warm_start_last takes
    s.warm_start_last()
    a = s.solve()
    assert a.status == 1 and s.warm_info()["n_warm_inits"] == 1
    host = {k: pt[f].cpu().numpy() for k, f in (("x", "solution"), ("y", "multipliers"), ("zl", "multipliers_L"),
                                                ("zu", "multipliers_U"))}
    f = _solver(p1, **kw)
    f.warm_start(**host)
    assert_same(a, f.solve())
    g = _solver(p1, **kw)
    g.warm_start_device(**{k: _dev(v) for k, v in host.items()})
    assert_same(a, g.solve())
    assert s.counters()["n_analyses"] == 1


def test_warm_start_last_before_the_update_keeps_the_solved_scaling():
    """solve -> warm_start_last -> update -> solve: the point is the first solve's public solution (taken
    with the scaling it was solved in) and survives the update: equal to a fresh solver on the new problem
    given the first solve's returned vectors."""
    p0 = scaled_general("lp")
    p1 = perturbed(p0, 101)
    s = _solver(p0, **_kw())
    a0 = s.solve()
    s.warm_start_last(0.9)
    s.update(**_values(p1))
    a1 = s.solve()
    f = _solver(p1, **_kw())
    f.warm_start(weight=0.9, **warm_point(a0))
    assert_same(a1, f.solve())
    assert a1.status == 1


# ------------------------------------------------------------------ 5. streams, memory, determinism
def test_point_produced_on_the_callers_stream_and_no_later_allocation():
    qp = _problem("scaled_qp_min")
    kw = _kw()
    cold = _solver(qp, **kw).solve()
    w = warm_point(cold)
    ref_s = _solver(qp, **kw)
    ref_s.warm_start(**w)
    ref = ref_s.solve()
    assert ref.iter < cold.iter

    def run():
        s = _solver(qp, **kw)
        half = {k: _dev(0.5 * v) for k, v in w.items()}
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            filler = torch.ones(1 << 22, dtype=torch.float64, device="cuda")
            for _ in range(8):               # work in front of the products, so that they are still pending
                filler = filler * 1.0000001
            t = {k: v * 2.0 for k, v in half.items()}      # exact: the point itself
        s.warm_start_device(stream=st, **t)  # no synchronisation of st before the call
        with torch.cuda.stream(st):
            for v in t.values():             # overwritten right after the call returns
                v.fill_(float("nan"))
        out = s.solve()
        st.synchronize()
        for _ in range(2):                   # the second and third calls allocate nothing
            t2 = {k: _dev(v) for k, v in w.items()}
            torch.cuda.synchronize()
            free = torch.cuda.mem_get_info()[0]
            s.warm_start_device(**t2)
            s.warm_start_last()
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free
        return out

    a, b = run(), run()
    assert_same(a, ref)
    assert_same(a, b)


# ------------------------------------------------------------------ 6. refusals leave the solver cold and intact
def test_refusals():
    from madipm_amd import _lib as L
    from madipm_amd._lib import MadIPMError
    qp = _problem("scaled_lp_min")
    s = _solver(qp, **_kw())
    with pytest.raises(MadIPMError, match="no solve has run"):
        s.warm_start_last()
    ref = s.solve()
    w = warm_point(ref)

    def refused(exc, call, match=None):
        """The call raises, and the solver still solves cold, bit for bit."""
        with pytest.raises(exc, match=match):
            call()
        assert s.warm_info() == {"active": False, "weight": 0.0, "n_warm_inits": 0}
        assert_same(s.solve(), ref)

    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        refused(MadIPMError, lambda: s.warm_start(weight=bad, **w), "weight")
        refused(MadIPMError, lambda: s.warm_start_last(bad), "weight")
        refused(MadIPMError, lambda: s.warm_start_device(weight=bad, x=_dev(w["x"])), "weight")
    refused(MadIPMError, lambda: s.warm_start(), "NULL")
    refused(MadIPMError, lambda: s.warm_start_device(), "NULL")
    assert L.lib.madipm_solver_set_warm_start(s.h, None, None, None, None, 0.5) < 0
    assert "NULL" in L.madipm_last_error().decode()
    assert L.lib.madipm_solver_set_warm_start_device(s.h, None, None, None, None, 0.5, None) < 0
    for k, v in (("x", w["x"][:-1]), ("y", np.append(w["y"], 0.0)), ("zl", np.zeros(3))):
        refused(ValueError, lambda: s.warm_start(**{k: v}))
    for v, exc in ((_dev(w["x"][:-1]), ValueError), (w["x"], TypeError), (torch.as_tensor(w["x"]), TypeError),
                   (_dev(w["x"]).float(), TypeError), (_dev(np.repeat(w["x"], 2))[::2], ValueError)):
        refused(exc, lambda: s.warm_start_device(x=v))
    assert s.warm_info() == {"active": False, "weight": 0.0, "n_warm_inits": 0}
    assert_same(s.solve(), ref)              # still cold, bit for bit
    assert_same(s.solve(), _solver(qp, **_kw()).solve())
    s.warm_start(**w)                        # and a valid one still goes through
    assert s.solve().iter < ref.iter
    # a refused call does not disturb the point that is set
    with pytest.raises(MadIPMError):
        s.warm_start(weight=2.0, **w)
    assert s.warm_info() == {"active": True, "weight": 0.99, "n_warm_inits": 1}


# ------------------------------------------------------------------ 7. the grid-stride pass of both kernels
def test_second_grid_pass_on_a_large_diagonal_lp():
    """k_warm_blend's grid is capped at 2048 blocks of 256 threads and k_warm_rows' at the same number of
    lane groups: n + m = 3 x 176000 coordinates and 176000 inequality rows at 4 lanes each need a second pass.
    min c'x, 0.5 <= x_i <= 1.5 (ranged rows of A = I), 0 <= x <= 2, scaling off: obj_scale = con_scale = 1,
    so the public blocks have the closed form w v~ + (1 - w) v_cold, compared exactly with the cold start
    of a second solver; the slack part (not returned) is in the iteration-0 record, compared with the warm
    oracle."""
    from madipm_amd.qp import QuadraticModel
    n, lam = 176000, 0.75
    i = np.arange(n)
    qp = QuadraticModel(c=0.25 + (i % 7) / 8.0, Hrows=[], Hcols=[], Hvals=[], Arows=i, Acols=i, Avals=np.ones(n),
                        lcon=np.full(n, 0.5), ucon=np.full(n, 1.5), lvar=np.zeros(n), uvar=np.full(n, 2.0),
                        x0=np.ones(n), name="diag_lp")
    kw = dict(regularization=_reg(1e-4), max_iter=0, scaling=False)
    cold = _solver(qp, **kw).solve()
    rng = np.random.default_rng(3)
    w = dict(x=np.linspace(-1.0, 3.0, n), y=rng.standard_normal(n), zl=rng.uniform(-0.5, 2.0, n),
             zu=rng.uniform(-0.5, 2.0, n))
    s = _solver(qp, **kw)
    s.warm_start(weight=lam, **w)
    st = s.solve()
    rest = 1.0 - lam
    xl, xu = 0.0 - 1e-12 * 1.0, 2.0 + 1e-12 * 2.0       # the relaxed bounds (bound_relax_factor)
    assert np.array_equal(st.solution, lam * np.clip(w["x"], xl, xu) + rest * cold.solution)
    assert np.array_equal(st.multipliers, lam * w["y"] + rest * cold.multipliers)
    assert np.array_equal(st.multipliers_L, lam * np.maximum(w["zl"], 0.0) + rest * cold.multipliers_L)
    assert np.array_equal(st.multipliers_U, lam * np.maximum(w["zu"], 0.0) + rest * cold.multipliers_U)
    _, ost, ref = _oracle_run(qp, kw, w, lam)
    d = _diff(_gpu_stats_point(st), ref)
    print("diag_lp second pass | " + " ".join(f"{f}={d[f]:.1e}" for f in VECTORS + SCALARS))
    for f in VECTORS + SCALARS:              # 1e-9: test_mpc_point_gpu's floor (a diagonal system: no spread)
        assert d[f] <= 1e-9, (f, d[f])
