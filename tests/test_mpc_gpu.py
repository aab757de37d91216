"""End-to-end GPU parity: the native HIP MPC solver vs the oracle restatement of MadIPM.

Both run the same algorithm (src/solver.jl mpc!) from the same data; they differ in the linear
algebra (GPU supernodal LDL^T vs SuperLU in the oracle) and in summation order.  Tolerances:
  * status equal, iteration count within 1 (late iterates are ill-conditioned: mu -> 1e-9);
  * final objective: |obj_gpu - obj_ref| <= 1e-6 max(1, |obj_ref|)  (BASELINE.md parity rule);
  * early trace (k <= 2): obj, inf_pr, inf_du, mu, alpha_p, alpha_d within `early_tol` relative
    (+1e-12 absolute).  With the benchmark regularization delta = 1e-8 the K2 solves carry relative
    errors ~eps*kappa ~ 1e-8..1e-7 in ANY factorisation (oracle SuperLU vs GPU LDL^T already differ
    by 7e-10 at k = 1 on AFIRO), so early_tol = 1e-6 there; with delta = 1e-4 (kappa ~1e4) the
    trajectories must agree to early_tol = 1e-9 (test_tight_trace_*).
Reference-pinned answers: simple_lp objective == 1 (test/runtests.jl:29-60), AFIRO -464.75314286.
"""
import math

import numpy as np
import pytest

from oracle.mpc import OracleMPC, OracleOptions

pytestmark = pytest.mark.gpu


def _oracle_opts(kw):
    from madipm_amd import solver as S
    o = {}
    reg = kw.get("regularization")
    if isinstance(reg, S.NoRegularization):
        o["regularization"] = ("none",)
    elif isinstance(reg, S.FixedRegularization):
        o["regularization"] = ("fixed", reg.delta_p, reg.delta_d)
    elif isinstance(reg, S.AdaptiveRegularization):
        o["regularization"] = ("adaptive", reg.delta_p, reg.delta_d, reg.delta_min)
    rule = kw.get("step_rule")
    if isinstance(rule, S.AdaptiveStep):
        o["step_rule"] = ("adaptive", rule.tau_min)
    elif isinstance(rule, S.ConservativeStep):
        o["step_rule"] = ("conservative", rule.tau)
    elif isinstance(rule, S.MehrotraAdaptiveStep):
        o["step_rule"] = ("mehrotra", rule.gamma_f)
    for k in ("max_iter", "tol", "max_ncorr", "scaling"):
        if k in kw:
            o[k] = kw[k]
    kkt = kw.get("kkt_system")
    if kkt is not None:
        o["kkt_system"] = {S.SparseKKTSystem: "K2", S.ScaledSparseKKTSystem: "K25", S.NormalKKTSystem: "normal"}[kkt]
    return OracleOptions(**o)


def _compare(qp, early=2, iter_slack=1, early_tol=1e-6, **kw):
    from madipm_amd import MPCSolver
    gpu = MPCSolver(qp, **kw).solve()
    ref = OracleMPC(qp, _oracle_opts(kw)).solve()
    assert gpu.status == ref.status, (gpu.status_name, ref.status)
    assert abs(gpu.iter - ref.iter) <= iter_slack, (gpu.iter, ref.iter)
    assert abs(gpu.objective - ref.objective) <= 1e-6 * max(1.0, abs(ref.objective)), (gpu.objective, ref.objective)
    for tg, tr in list(zip(gpu.trace, ref.trace))[: early + 1]:
        for key in ("obj", "inf_pr", "inf_du", "mu", "alpha_p", "alpha_d"):
            a, b = tg[key], tr[key]
            assert abs(a - b) <= early_tol * abs(b) + 1e-12, (tg["k"], key, a, b)
    return gpu, ref


def test_simple_lp_reference_answer():
    from madipm_amd import simple_lp, MPCSolver, NoRegularization, SOLVE_SUCCEEDED
    gpu, ref = _compare(simple_lp(), regularization=NoRegularization())
    assert gpu.status == SOLVE_SUCCEEDED
    assert abs(gpu.objective - 1.0) <= 1e-8                  # analytic answer of the reference test


def test_simple_lp_standard_form_equal():
    """test/runtests.jl:159-164: standard_form_qp gives the same objective."""
    from madipm_amd import simple_lp, standard_form_qp, MPCSolver, NoRegularization
    a = MPCSolver(simple_lp(), regularization=NoRegularization()).solve()
    b = MPCSolver(standard_form_qp(simple_lp())).solve()
    assert abs(a.objective - b.objective) <= 1e-8


@pytest.mark.parametrize("std", [False, True])
def test_afiro(std):
    import os
    from madipm_amd import read_mps, standard_form_qp, FixedRegularization
    qp = read_mps(os.path.join(os.path.dirname(__file__), "golden", "afiro.mps"))
    if std:
        qp = standard_form_qp(qp)
    gpu, ref = _compare(qp, regularization=FixedRegularization(1e-8, -1e-8), max_iter=300)
    assert abs(gpu.objective - (-464.75314286)) <= 1e-6 * 464.75


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_lp(seed):
    from madipm_amd import FixedRegularization
    from madipm_amd.instances import random_lp
    qp = random_lp(120, 250, 0.03, seed, ineq_frac=0.3, free_frac=0.05)
    _compare(qp, regularization=FixedRegularization(1e-8, -1e-8))


@pytest.mark.parametrize("rule", ["adaptive", "conservative", "mehrotra"])
def test_step_rules_dense_dummy(rule):
    """test/runtests.jl:85-97 (status only there; here also parity with the oracle)."""
    from madipm_amd import AdaptiveStep, ConservativeStep, MehrotraAdaptiveStep, SOLVE_SUCCEEDED
    from madipm_amd.instances import dense_dummy_qp
    r = {"adaptive": AdaptiveStep(0.99), "conservative": ConservativeStep(0.99),
         "mehrotra": MehrotraAdaptiveStep(0.99)}[rule]
    gpu, ref = _compare(dense_dummy_qp(10, 5), step_rule=r)
    assert gpu.status == SOLVE_SUCCEEDED


@pytest.mark.parametrize("reg", ["none", "fixed", "adaptive"])
def test_regularizations_qp(reg):
    """test/runtests.jl:122-140."""
    from madipm_amd import NoRegularization, FixedRegularization, AdaptiveRegularization
    from madipm_amd.instances import random_qp
    r = {"none": NoRegularization(), "fixed": FixedRegularization(1e-8, -1e-9),
         "adaptive": AdaptiveRegularization(1e-8, -1e-9, 1e-9)}[reg]
    _compare(random_qp(40, 90, 0.08, 3), regularization=r)


def test_equality_and_fixed_variables():
    """test/runtests.jl:67-78 cases (equality rows, fixed variables), incl. Gondzio max_ncorr=5."""
    from madipm_amd.instances import dense_dummy_qp
    _compare(dense_dummy_qp(20, 15, eq=[1, 2, 3, 8]))
    _compare(dense_dummy_qp(20, 15, eq=[1, 2, 3, 8]), max_ncorr=5)
    _compare(dense_dummy_qp(20, 15, fixed=[1, 2]))
    _compare(dense_dummy_qp(20, 15, fixed=[1, 2], eq=[1, 2, 3, 8]))


def test_ex10_standin_small():
    from madipm_amd import standard_form_qp, FixedRegularization
    from madipm_amd.instances import ex10_standin
    qp = standard_form_qp(ex10_standin(scale=0.05))
    gpu, ref = _compare(qp, regularization=FixedRegularization(1e-8, -1e-8), max_iter=300)
    assert gpu.status == 1


@pytest.mark.parametrize("which", ["afiro", "random_lp", "random_qp"])
def test_tight_trace(which):
    """Well-conditioned regularization (1e-4, -1e-4): the GPU trajectory equals the oracle's to 1e-9."""
    import os
    from madipm_amd import read_mps, FixedRegularization
    from madipm_amd.instances import random_lp, random_qp
    qp = {"afiro": lambda: read_mps(os.path.join(os.path.dirname(__file__), "golden", "afiro.mps")),
          "random_lp": lambda: random_lp(120, 250, 0.03, 5, ineq_frac=0.3),
          "random_qp": lambda: random_qp(40, 90, 0.08, 6)}[which]()
    _compare(qp, early=3, early_tol=1e-9, regularization=FixedRegularization(1e-4, -1e-4))


# ---------------------------------------------------------------- KKT formulations on the GPU
# K2.5 (ScaledSparseKKTSystem) and NormalKKTSystem (LP only, Cholesky semantics): each vs the
# oracle of the same formulation, and vs the GPU K2 solution within the reference's 1e-6
# (test/runtests.jl:107-120, 182-196; test/test_gpu.jl:9-19 runs all three on the GPU).
def _kkt_cases():
    import os
    from madipm_amd import read_mps, simple_lp, standard_form_qp
    from madipm_amd.instances import random_lp
    gold = os.path.join(os.path.dirname(__file__), "golden", "afiro.mps")
    return {"simple_lp": simple_lp, "afiro": lambda: read_mps(gold),
            "afiro_std": lambda: standard_form_qp(read_mps(gold)),
            "random_lp": lambda: random_lp(60, 120, 0.05, 0, ineq_frac=0.3, free_frac=0.05)}


@pytest.mark.parametrize("kkt_name", ["ScaledSparseKKTSystem", "NormalKKTSystem"])
@pytest.mark.parametrize("case", ["simple_lp", "afiro", "afiro_std", "random_lp"])
def test_kkt_formulation_parity(kkt_name, case):
    from madipm_amd import MPCSolver, FixedRegularization, SparseKKTSystem
    from madipm_amd import solver as S
    kkt = getattr(S, kkt_name)
    qp = _kkt_cases()[case]()
    kw = dict(regularization=FixedRegularization(1e-8, -1e-8), max_iter=300)
    gpu, ref = _compare(qp, kkt_system=kkt, **kw)
    k2 = MPCSolver(qp, kkt_system=SparseKKTSystem, **kw).solve()
    assert gpu.status == k2.status
    assert abs(gpu.objective - k2.objective) <= 1e-6 * max(1.0, abs(k2.objective))
    assert np.max(np.abs(gpu.solution - k2.solution)) <= 1e-6 * max(1.0, np.max(np.abs(k2.solution)))
    ytol = 1e-6 if case == "simple_lp" else 1e-5  # degenerate dual faces (see test_oracle_cpu)
    assert np.max(np.abs(gpu.multipliers - k2.multipliers)) <= ytol * max(1.0, np.max(np.abs(k2.multipliers)))


def test_k25_qp_parity():
    from madipm_amd import ScaledSparseKKTSystem, FixedRegularization
    from madipm_amd.instances import random_qp
    _compare(random_qp(40, 80, 0.08, 3), kkt_system=ScaledSparseKKTSystem, max_iter=300,
             regularization=FixedRegularization(1e-8, -1e-8))


def test_normal_kkt_rejects_qp():
    from madipm_amd import MPCSolver, NormalKKTSystem
    from madipm_amd.instances import random_qp
    with pytest.raises(Exception, match="only linear programs"):
        MPCSolver(random_qp(10, 20, 0.2, 0), kkt_system=NormalKKTSystem)


# ---------------------------------------------------------------- BASELINE.json configs 4 / 5
# The supportcase10 (many short rows) and neos-5052403 (dense rows, wide separators) stand-ins at a
# scale the oracle solves in seconds; bench.py --config supportcase10 / neos runs the full sizes.
@pytest.mark.parametrize("name,kw", [("supportcase10_standin", dict(scale=0.1, block_scale=0.3)),
                                     ("supportcase10_standin", dict(scale=0.05, block_scale=1.0)),  # r ~ 230 fronts
                                     ("neos5052403_standin", dict(scale=0.25, block_scale=0.15))])
def test_config_standins_parity(name, kw):
    from madipm_amd import FixedRegularization, standard_form_qp, MPCSolver
    from madipm_amd import instances as I
    qp = standard_form_qp(getattr(I, name)(**kw))
    opts = dict(regularization=FixedRegularization(1e-8, -1e-8), max_iter=300)
    gpu, ref = _compare(qp, **opts)
    # the subtree-sharded factorisation (4 shards on this device) follows the same trajectory
    sh = MPCSolver(qp, nshards=4, **opts).solve()
    assert sh.status == gpu.status and abs(sh.iter - gpu.iter) <= 1
    assert abs(sh.objective - gpu.objective) <= 1e-8 * max(1.0, abs(gpu.objective))


def test_dense_qp_batched_leaves():
    """BASELINE.json configs[2] (dense convex QP) at a size the oracle solves in seconds: the x
    columns are eliminated as batched leaves (MFMA SYRK)."""
    from madipm_amd import FixedRegularization, MPCSolver
    from madipm_amd.instances import dense_qp
    qp = dense_qp(n=1200, m=200, seed=0)
    opts = dict(regularization=FixedRegularization(1e-8, -1e-8), max_iter=300, ordering=0)
    s = MPCSolver(qp, **opts)
    assert s.ldl_info()["lb_members"] >= 600
    gpu = s.solve()
    ref = OracleMPC(qp, _oracle_opts(opts)).solve()
    assert gpu.status == ref.status == 1
    assert abs(gpu.iter - ref.iter) <= 1
    assert abs(gpu.objective - ref.objective) <= 1e-6 * max(1.0, abs(ref.objective))


@pytest.mark.parametrize("max_iter", [0, 1, 4])
def test_max_iter_stop(max_iter):
    """MAXIMUM_ITERATIONS_EXCEEDED after exactly max_iter steps (the last termination test enqueues no
    speculative factorisation), same iterate as the oracle: objective and trace agree early."""
    import os
    from madipm_amd import read_mps, FixedRegularization, MAXIMUM_ITERATIONS_EXCEEDED
    qp = read_mps(os.path.join(os.path.dirname(__file__), "golden", "afiro.mps"))
    gpu, ref = _compare(qp, early=min(max_iter, 2), iter_slack=0,
                        regularization=FixedRegularization(1e-8, -1e-8), max_iter=max_iter)
    assert gpu.status == MAXIMUM_ITERATIONS_EXCEEDED and gpu.iter == max_iter
    assert len(gpu.trace) == max_iter + 1
