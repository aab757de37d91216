"""The returned point and statistics of the GPU solver, element by element against the oracle.

These problems have at most 200 variables: every reduction here has at most about 50 partial blocks, so
k_final stays in its one-workgroup instance and no producer loop strides.  The same comparison past 1024
partial blocks and past the 2048-block cap is tests/test_mpc_regimes_gpu.py.

test_mpc_gpu.py compares status, iteration count, the objective and six scalars of the early trace:
max-norms and sums, which hide a wrong element, behind an interior-point loop that corrects small kernel
errors on later iterations.  Here (problems of <= 200 variables, tests/helpers.py, pinned on the oracle
in test_point_helpers_cpu.py):

  * test_iterates_match_oracle        iterates 0, 1, 3 (x, y, zl, zu, constraints and the statistics) on
                                      problems where set_scaling! scales and on the edge row lengths;
  * test_final_point_and_certificate  converged points, scaling on and off, min and max, with a
                                      general-form optimality certificate of the returned vectors;
  * test_spmv_widths                  every lane-group width G of the SpMV kernels (MADIPM_SPMV_G) on
                                      rows of 1, G - 1, G, G + 1, 2G, 2G + 1, > 4G entries;
  * test_degenerate_shapes            no bounded coordinate at all (nlb = nub = 0);
  * test_box_qp_no_constraints        no constraint (m = 0).

Tolerance of an iterate (FixedRegularization(1e-4, -1e-4), the well-conditioned setting of
test_tight_trace): |gpu - ref| <= tol max(1, |ref|_inf) per vector, tol = max(1e-9, 30 s), where s is the
oracle's own spread on that case and k — the same oracle solve with its LDL^T backend instead of
SuperLU — and s <= 3e-9 is required, so tol <= 1e-7 cannot hide a wrong element.
"""
import functools

import numpy as np
import pytest

from helpers import assert_certificate, box_qp, free_eq_qp, regime_case, rowlen_qp, scaled_general
from oracle.mpc import OracleMPC
from test_mpc_gpu import _oracle_opts

pytestmark = pytest.mark.gpu

VECTORS = ("solution", "multipliers", "multipliers_L", "multipliers_U", "constraints")
SCALARS = ("objective", "dual_objective", "inf_pr", "inf_du", "inf_compl", "mu")

PROBLEMS = {"rowlen_qp": lambda: rowlen_qp(hess=True), "rowlen_lp": lambda: rowlen_qp(hess=False)}
PROBLEMS.update({f"scaled_{kind}_{'min' if mn else 'max'}": (lambda kind=kind, mn=mn: scaled_general(kind, mn))
                 for kind in ("lp", "qp") for mn in (True, False)})


@functools.lru_cache(maxsize=None)
def _problem(name):
    """A named problem; 'regime:...' names are the sized family of helpers.regime_problem."""
    return regime_case(name) if name.startswith("regime:") else PROBLEMS[name]()


def _kkt(name):
    from madipm_amd import solver as S
    return {"K2": S.SparseKKTSystem, "K25": S.ScaledSparseKKTSystem, "normal": S.NormalKKTSystem}[name]


def _variant(name):
    from madipm_amd import MehrotraAdaptiveStep
    return {"default": {}, "mehrotra": dict(step_rule=MehrotraAdaptiveStep(0.99)), "ncorr3": dict(max_ncorr=3)}[name]


def _reg(delta):
    from madipm_amd import FixedRegularization
    return FixedRegularization(delta, -delta)


def _point(st, scalars):
    d = {f: np.asarray(getattr(st, f), float) for f in VECTORS}
    d.update(scalars)
    return d


def _oracle_point(qp, kw, backend="superlu"):
    """The oracle's returned point and the statistics of its last termination test."""
    o = OracleMPC(qp, _oracle_opts(kw))
    o.linear_solver = backend
    with np.errstate(invalid="ignore"):          # init_starting_point!'s 0 / 0 without a bounded coordinate
        st = o.solve()
    t = st.trace[-1]
    assert t["k"] == st.iter
    return st, _point(st, dict(objective=st.objective, dual_objective=o.dual_objective() / o.obj_scale,
                               inf_pr=t["inf_pr"], inf_du=t["inf_du"], inf_compl=t["inf_compl"], mu=t["mu"]))


def _gpu_point(qp, kw):
    from madipm_amd import MPCSolver
    s = MPCSolver(qp, **kw)
    st = s.solve()
    t = st.trace[-1]
    assert t["k"] == st.iter
    return s, st, _point(st, dict(objective=st.objective, dual_objective=st.dual_objective, inf_pr=st.primal_feas,
                                  inf_du=st.dual_feas, inf_compl=st.inf_compl, mu=t["mu"]))


def _diff(a, b):
    """Per field: |a - b|_inf / max(1, |b|_inf)."""
    out = {}
    for f in VECTORS + SCALARS:
        x, y = np.atleast_1d(a[f]), np.atleast_1d(b[f])
        assert x.shape == y.shape, (f, x.shape, y.shape)
        out[f] = float(np.max(np.abs(x - y), initial=0.0) / max(1.0, np.max(np.abs(y), initial=0.0)))
        assert np.all(np.isfinite(x)), f
    return out


@functools.lru_cache(maxsize=None)
def _oracle_iterate(problem, kkt, variant, k):
    """Oracle iterate k with its own spread s (SuperLU vs the LDL^T backend) and the tolerance from it."""
    qp = _problem(problem)
    kw = dict(regularization=_reg(1e-4), kkt_system=_kkt(kkt), max_iter=k, **_variant(variant))
    st, ref = _oracle_point(qp, kw)
    st2, alt = _oracle_point(qp, kw, backend="ldl")
    assert st.status == st2.status and st.iter == st2.iter == k
    spread = _diff(alt, ref)
    s = max(spread.values())
    assert s <= 3e-9, (problem, kkt, variant, k, spread)
    return st, ref, spread, max(1e-9, 30.0 * s)


def _check_iterate(qp, problem, kkt, variant, k, label="", seen=None):
    """seen: a dict that collects the largest difference per field."""
    from madipm_amd import MAXIMUM_ITERATIONS_EXCEEDED
    st, ref, spread, tol = _oracle_iterate(problem, kkt, variant, k)
    kw = dict(regularization=_reg(1e-4), kkt_system=_kkt(kkt), max_iter=k, **_variant(variant))
    s, gst, gpu = _gpu_point(qp, kw)
    assert gst.status == st.status == MAXIMUM_ITERATIONS_EXCEEDED and gst.iter == k
    d = _diff(gpu, ref)
    print(f"iterate {problem} {kkt} {variant}{label} k={k} G={s.spmv_group()} tol={tol:.1e} | " +
          " ".join(f"{f}={d[f]:.1e}/{spread[f]:.1e}" for f in VECTORS + SCALARS))
    for f in VECTORS + SCALARS:
        if seen is not None:
            seen[f] = max(seen.get(f, 0.0), d[f])
        assert d[f] <= tol, (problem, kkt, variant, k, f, d[f], tol, spread[f])
    return s


ITERATE_CASES = ([(p, kkt, "default") for p in ("scaled_lp_min", "scaled_qp_max", "rowlen_qp", "rowlen_lp")
                  for kkt in ("K2", "K25")] +
                 [(p, "normal", "default") for p in ("scaled_lp_min", "rowlen_lp")] +
                 [("scaled_qp_max", "K2", "mehrotra"), ("scaled_qp_max", "K2", "ncorr3")])


@pytest.mark.parametrize("problem,kkt,variant", ITERATE_CASES)
def test_iterates_match_oracle(problem, kkt, variant, monkeypatch):
    """Iterates k = 0 (the starting point after initialize!), 1 and 3: the five returned vectors and
    objective, dual_objective, inf_pr, inf_du, inf_compl, mu against the oracle, within
    max(1e-9, 30 x the oracle's own spread).

    Largest GPU-vs-oracle difference observed on the MI355X over all cases, k and (test_spmv_widths) all
    widths, relative to max(1, |ref|_inf), next to the oracle's own largest spread (SuperLU vs LDL^T):

        field            gpu vs oracle   oracle spread
        solution            1.5e-11         1.5e-11
        multipliers         4.2e-11         3.7e-11
        multipliers_L       1.6e-11         2.0e-11
        multipliers_U       1.7e-11         1.6e-11
        constraints         5.7e-12         4.7e-12
        objective           5.5e-11         3.6e-11
        dual_objective      1.0e-11         5.5e-12
        inf_pr              2.8e-12         1.6e-12
        inf_du              6.7e-13         5.9e-13
        inf_compl           9.8e-12         8.7e-12
        mu                  2.0e-11         1.7e-11

    (the tolerance was 1e-9 everywhere but the normal equations on scaled_lp_min, 1.1e-9); converged
    runs at delta = 1e-4 agreed to 7.9e-14 (multipliers) or better."""
    monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    qp = _problem(problem)
    for k in (0, 1, 3):
        _check_iterate(qp, problem, kkt, variant, k)


@functools.lru_cache(maxsize=None)
def _oracle_converged(problem, kkt, delta, scaling=True):
    kw = dict(regularization=_reg(delta), kkt_system=_kkt(kkt), max_iter=300, scaling=scaling)
    return _oracle_point(_problem(problem), kw)


def _check_converged_1e4(qp, problem, kkt, label=""):
    """Converged run with FixedRegularization(1e-4, -1e-4): the GPU takes the oracle's iteration count
    and returns its vectors to 1e-6 max(1, |ref|_inf) (test_kkt_formulation_parity's rule); the returned
    point carries its own optimality certificate."""
    st, ref = _oracle_converged(problem, kkt, 1e-4)
    s, gst, gpu = _gpu_point(qp, dict(regularization=_reg(1e-4), kkt_system=_kkt(kkt), max_iter=300))
    assert gst.status == st.status == 1, (gst.status_name, st.status)
    assert gst.iter == st.iter, (gst.iter, st.iter)
    d = _diff(gpu, ref)
    print(f"converged(1e-4) {problem} {kkt}{label} it={gst.iter} | " + " ".join(f"{f}={d[f]:.1e}" for f in VECTORS))
    for f in VECTORS:
        assert d[f] <= 1e-6, (problem, kkt, f, d[f])
    assert abs(gst.objective - st.objective) <= 1e-6 * max(1.0, abs(st.objective))
    assert_certificate(qp, gst, gst.objective)
    return s


@pytest.mark.parametrize("scaling", [True, False])
@pytest.mark.parametrize("minimize", [True, False])
@pytest.mark.parametrize("kind", ["lp", "qp"])
def test_final_point_and_certificate(kind, minimize, scaling, monkeypatch):
    """Converged points of the problems on which obj_scale and con_scale are not 1 (and, scaling=False,
    the same problems unscaled), with fixed variables, c0, free variables, one-sided and ranged rows,
    minimised and maximised: the existing parity rules against the oracle at delta = 1e-8, the optimality
    certificate of the returned vectors on the unscaled problem, and at delta = 1e-4 the vectors
    themselves against the oracle."""
    monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    problem = f"scaled_{kind}_{'min' if minimize else 'max'}"
    qp = _problem(problem)
    st, ref = _oracle_converged(problem, "K2", 1e-8, scaling)
    _, gst, gpu = _gpu_point(qp, dict(regularization=_reg(1e-8), max_iter=300, scaling=scaling))
    assert gst.status == st.status == 1, (gst.status_name, st.status)
    assert abs(gst.iter - st.iter) <= 1, (gst.iter, st.iter)
    assert abs(gst.objective - st.objective) <= 1e-6 * max(1.0, abs(st.objective)), (gst.objective, st.objective)
    p = assert_certificate(qp, gst, gst.objective)
    print(f"final {problem} scaling={scaling} it={gst.iter}/{st.iter} certificate", {k: float(f"{v:.3g}") for k, v in p.items()})
    if scaling:
        _check_converged_1e4(qp, problem, "K2")


WIDTH_CASES = [("rowlen_qp", "K2"), ("rowlen_qp", "K25"), ("rowlen_lp", "K2"), ("rowlen_lp", "normal")]
DEFAULT_WIDTH = {"rowlen_qp": 32, "rowlen_lp": 8}


@pytest.mark.parametrize("G", [None, 4, 8, 16, 32, 64])
def test_spmv_widths(G, monkeypatch):
    """gdot<G>, gdot2<G>, k_residual<G>, k_eval<G>, k_normal_rhs<G>, k_normal_back<G> at every G, on A rows
    of 1, 3, 4, 5, 8, 9, 19, 32, 33, 64, 65, 129, 131 entries, a J^T row of 39 and (rowlen_qp) H rows of
    ~70: iterate 3 and the converged point against the oracle.  G = None: the heuristic's own choice."""
    if G is None:
        monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    else:
        monkeypatch.setenv("MADIPM_SPMV_G", str(G))
    for problem, kkt in WIDTH_CASES:
        qp = _problem(problem)
        want = DEFAULT_WIDTH[problem] if G is None else G
        s = _check_iterate(qp, problem, kkt, "default", 3, label=f" G={want}")
        assert s.spmv_group() == want, (problem, kkt, s.spmv_group(), want)
        s = _check_converged_1e4(qp, problem, kkt, label=f" G={want}")
        assert s.spmv_group() == want


def test_spmv_width_knob_ignores_other_values(monkeypatch):
    from madipm_amd import MPCSolver
    qp = _problem("rowlen_lp")
    for v in ("0", "2", "12", "128", "-8", "x", ""):
        monkeypatch.setenv("MADIPM_SPMV_G", v)
        assert MPCSolver(qp).spmv_group() == DEFAULT_WIDTH["rowlen_lp"], v


def test_box_qp_no_constraints(monkeypatch):
    """m = 0 (no constraint, 0 <= x <= 1): every m-sized launch and allocation is empty."""
    monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    qp = box_qp()
    kw = dict(regularization=_reg(1e-8), max_iter=300)
    st, ref = _oracle_point(qp, kw)
    _, gst, gpu = _gpu_point(qp, kw)
    assert gst.status == st.status == 1, (gst.status_name, st.status)
    assert abs(gst.iter - st.iter) <= 1, (gst.iter, st.iter)
    assert abs(gst.objective - st.objective) <= 1e-6 * max(1.0, abs(st.objective))
    assert len(gst.multipliers) == len(gst.constraints) == 0
    assert_certificate(qp, gst, gst.objective)


@pytest.mark.parametrize("order", ["natural", "default"])
@pytest.mark.parametrize("reg", ["noreg", "fixedreg"])
def test_degenerate_shapes(reg, order, monkeypatch):
    """nlb = nub = 0: every variable free, every row an equality, H dense positive definite.
    init_starting_point!'s delta_x2 and delta_s2 are 0 / 0 in the reference, the barrier is empty, and one
    Newton step solves the problem: the oracle (SuperLU, partial pivoting) stops after exactly 2
    iterations at the solution of one dense solve of [H A^T; A 0].

    K2 is dense here, so every fill-reducing order ties, and a static-pivot LDL^T depends on which block
    goes first.  order="natural" (ordering=0, the option the dense-QP tests pass: x before y) is held to
    the oracle's answer: same status, exactly 2 iterations, x and y within 1e-6 of the dense solve, the
    objective within 1e-9, zl = zu = 0.  Under the default ordering the y block is eliminated first: its
    pivots are delta_d = -1e-8 (FixedRegularization: solve residuals ~2e-7, a third iteration) or exactly 0
    (NoRegularization: no factorization, INTERNAL_ERROR) — the behaviour of the reference's own LDL^T in
    that order, pinned on the CPU in test_point_helpers_cpu.py::test_free_eq_qp_pivot_order.  There the
    GPU is compared with the oracle running its LDL^T backend in the GPU's own pivot order."""
    from madipm_amd import NoRegularization, MPCSolver
    monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    qp, x, y, obj = free_eq_qp()
    kw = dict(regularization=NoRegularization() if reg == "noreg" else _reg(1e-8))
    if order == "natural":
        st, ref = _oracle_point(qp, kw)
        _, gst, gpu = _gpu_point(qp, dict(kw, ordering=0))
        assert gst.status == st.status == 1, (gst.status_name, st.status)
        assert gst.iter == st.iter == 2, (gst.iter, st.iter)
    else:
        s = MPCSolver(qp, **kw)
        o = OracleMPC(qp, _oracle_opts(kw))
        o.linear_solver = "ldl"
        o.ldl_perm = s.kkt_perm()
        with np.errstate(invalid="ignore"):
            st = o.solve()
        gst = s.solve()
        print(f"free_eq_qp {reg} default order: gpu {gst.status_name} it {gst.iter}, oracle LDL^T in that order "
              f"{st.status} it {st.iter}; first pivots {o.ldl_perm[:4].tolist()} (y = 30..39)")
        assert gst.status == st.status, (gst.status_name, st.status)
        assert gst.iter == st.iter, (gst.iter, st.iter)
        if gst.status != 1:
            return
    assert np.max(np.abs(gst.solution - x)) <= 1e-6 * max(1.0, np.max(np.abs(x)))
    assert np.max(np.abs(gst.multipliers - y)) <= 1e-6 * max(1.0, np.max(np.abs(y)))
    assert abs(gst.objective - obj) <= 1e-9 * abs(obj), (gst.objective, obj)
    assert np.all(gst.multipliers_L == 0.0) and np.all(gst.multipliers_U == 0.0)
    assert_certificate(qp, gst, gst.objective)
