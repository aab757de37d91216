"""MPCSolver.adjoint / adjoint_device / QPLayer on the GPU against the CPU oracle (adjoint_oracle.py).

Two comparisons per fixture, both with err = max |g_gpu - g_ref| / max(1, max |g_ref|) per block:
  formula  the oracle's formulas evaluated at the point the GPU solve returned: what the kernels compute
  truth    the oracle's gradients at its own optimum (mu = 1e-11): what the caller wants
and the routes (host / device / repeated / subsets give the same bits), the solver's state, the residual,
the refusals and the torch layer."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import adjoint_oracle as O  # noqa: E402
from helpers import box_qp, free_eq_qp  # noqa: E402
from test_update_gpu import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

# Largest err measured on the MI355X over all fixtures; each bound is 10 x it (floor 1e-9),
# and neither may exceed 1e-4: every term of every formula is >= 1e-2 of its block (test_adjoint_cpu.py).
FORMULA_MEASURED = 6.9e-10     # ucon of the 7 x 5 family; the sparse QP 9.1e-11, the scaled family 5.6e-11
TRUTH_MEASURED = 6.3e-8        # ucon of the 7 x 5 family (the end point's mu); the sparse QP 1.2e-8, the LP 3.7e-9
FORMULA_TOL = max(1e-9, 10.0 * FORMULA_MEASURED)
TRUTH_TOL = max(1e-9, 10.0 * TRUTH_MEASURED)
CAP = 1e-4

TOL_LINEAR_SOLVE = 1e-8   # the solver's default tol_linear_solve (madipm_default_options)


def _kw(**extra):
    from madipm_amd import FixedRegularization
    return dict(regularization=FixedRegularization(1e-8, -1e-8), max_iter=300, tol=1e-9, **extra)


def _free_eq():
    qp = free_eq_qp()[0]
    return qp, np.random.default_rng(17).uniform(0.5, 1.5, qp.nvar)


def _box():
    qp = box_qp()
    return qp, np.random.default_rng(18).uniform(0.5, 1.5, qp.nvar) * np.random.default_rng(19).choice([-1.0, 1.0], qp.nvar)


FIXTURES = {
    "family_min": (lambda: O.family(1), {}),
    "family_max": (lambda: O.family(1, minimize=False), {}),
    "family_scaled": (lambda: O.scaled_family(1), {}),
    "family_dup": (lambda: O.duplicated_family(1)[:2], {}),
    "family_seed3": (lambda: O.family(3), {}),
    "box": (_box, {}),
    "free_eq": (_free_eq, {}),
    "lp": (O.lp_fixture, {}),
    "sparse": (O.sparse_fixture, {}),
    "sparse_2shards": (O.sparse_fixture, {"nshards": 2}),
}
_cache, _refs = {}, {}


def _reference(make):
    """(qp, gx, reference point, reference gradients): computed once per problem, never modified."""
    if make not in _refs:
        qp, gx = make()
        pt = O.reference_ipm(qp)
        _refs[make] = (qp, gx, pt, O.reference_adjoint(qp, pt, gx))
    return _refs[make]


def case(name):
    """The fixture solved on the GPU once: solver, stats and the host route's gradients of all seven blocks."""
    if name not in _cache:
        from madipm_amd import MPCSolver
        make, extra = FIXTURES[name]
        qp, gx, pt, gref = _reference(make)
        s = MPCSolver(qp, **_kw(**extra))
        st = s.solve()
        assert st.status == 1, (name, st.status_name)
        g = s.adjoint(gx)
        _cache[name] = dict(qp=qp, gx=gx, pt=pt, gref=gref, solver=s, stats=st, g=g, info=s.adjoint_info())
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _cache.clear()          # the solvers go while the library is still loaded


def _errs(g, ref):
    return {k: O.err(g[k], ref[k]) for k in O.NAMES}


def test_tolerances_fit_the_condition():
    assert FORMULA_TOL <= CAP and TRUTH_TOL <= CAP


# ------------------------------------------------------------------ 1, 2, 3. formula and truth
@pytest.mark.parametrize("name", list(FIXTURES))
def test_formula_at_the_returned_point(name):
    c = case(name)
    st = c["stats"]
    point = {"x": st.solution, "y": st.multipliers, "zl": st.multipliers_L, "zu": st.multipliers_U}
    e = _errs(c["g"], O.reference_adjoint(c["qp"], point, c["gx"]))
    print("formula", name, {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= FORMULA_TOL, e


@pytest.mark.parametrize("name", list(FIXTURES))
def test_truth_at_the_reference_optimum(name):
    c = case(name)
    assert O.err(c["stats"].solution, c["pt"]["x"]) <= 1e-6        # the same optimum
    e = _errs(c["g"], c["gref"])
    print("truth", name, {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= TRUTH_TOL, e


def test_scaling_and_sign_fixtures_do_what_they_are_for():
    assert not case("family_max")["qp"].minimize
    # the scaled fixture: set_scaling! scales row 1 (an entry above 100) and the objective (x0 = 0: |c| above 100)
    qs = case("family_scaled")["qp"]
    assert np.abs(qs.Avals[qs.Arows == 1]).max() > 100.0 and np.abs(qs.Avals[qs.Arows != 1]).max() <= 1.0
    assert np.abs(qs.c).max() > 100.0 and not np.any(qs.x0)
    # the duplicated entries receive the full gradient of their entry
    qp, _, hk, ak = O.duplicated_family(1)
    g = case("family_dup")["g"]
    nh, na = qp.nnzh - len(hk), qp.nnzj - len(ak)
    assert np.array_equal(g["Hvals"][nh:], g["Hvals"][hk]) and np.array_equal(g["Avals"][na:], g["Avals"][ak])
    assert np.max(np.abs(g["Hvals"][hk])) > 1e-3 and np.max(np.abs(g["Avals"][ak])) > 1e-3
    assert case("lp")["g"]["Hvals"].shape == (0,) and case("box")["g"]["Avals"].shape == (0,)
    assert case("box")["g"]["lcon"].shape == (0,)
    assert case("sparse")["qp"].nvar == 1000 and (case("sparse")["qp"].lvar == case("sparse")["qp"].uvar).sum() == 20


# ------------------------------------------------------------------ 4. routes
@pytest.mark.parametrize("name", ["family_min", "family_scaled", "box", "lp", "sparse", "sparse_2shards"])
def test_routes_give_identical_bits(name):
    import torch
    c = case(name)
    s, gx, g = c["solver"], c["gx"], c["g"]
    nf = s.adjoint_info()["n_adjoint_factorizations"]
    again = s.adjoint(gx)
    dev = s.adjoint_device(torch.as_tensor(gx, device="cuda"))
    torch.cuda.synchronize()
    for k in O.NAMES:
        assert np.array_equal(again[k], g[k]), k
        assert np.array_equal(dev[k].cpu().numpy(), g[k]), k
    for want in (["c"], ["lvar", "uvar"], ["Avals"], ["Hvals", "lcon"], ["ucon"]):
        sub = s.adjoint(gx, want=want)
        assert sorted(sub) == sorted(want)
        for k in want:
            assert np.array_equal(sub[k], g[k]), (want, k)
        subd = s.adjoint_device(torch.as_tensor(gx, device="cuda"), want=want)
        for k in want:
            assert np.array_equal(subd[k].cpu().numpy(), g[k]), (want, k)
    # another gx on the same point: no new factorisation, and linear in gx
    g2 = s.adjoint(-2.0 * gx)
    info = s.adjoint_info()
    assert info["n_adjoint_factorizations"] == nf
    for k in O.NAMES:
        assert O.err(g2[k], -2.0 * g[k]) <= 1e-9, k


def test_device_route_honours_the_stream():
    import torch
    c = case("family_min")
    s = c["solver"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gx = torch.as_tensor(c["gx"], device="cuda") * 1.0       # produced on the side stream
        out = s.adjoint_device(gx, stream=side)
        doubled = {k: 2.0 * v for k, v in out.items()}            # consumed on it, without a host wait
    side.synchronize()
    for k in O.NAMES:
        assert np.array_equal(doubled[k].cpu().numpy(), 2.0 * c["g"][k]), k


# ------------------------------------------------------------------ 5. solver state
@pytest.mark.parametrize("name", ["family_min", "family_scaled", "sparse"])
def test_adjoint_leaves_the_next_solve_alone(name):
    from madipm_amd import MPCSolver
    make, extra = FIXTURES[name]
    qp, gx, _, _ = _reference(make)
    a = MPCSolver(qp, **_kw(**extra))
    first = a.solve()
    a.adjoint(gx)
    a.adjoint(gx, want=["c"])
    with_adjoint = a.solve()
    b = MPCSolver(qp, **_kw(**extra))
    assert_same(first, b.solve())
    assert_same(with_adjoint, b.solve())
    # and an adjoint after the second solve factorises again, with the first one's bits
    g = a.adjoint(gx)
    assert a.adjoint_info()["n_adjoint_factorizations"] == 2
    for k in O.NAMES:
        assert np.array_equal(g[k], case(name)["g"][k]), k


def test_warm_start_last_after_an_adjoint():
    from madipm_amd import MPCSolver
    qp, gx, _, _ = _reference(FIXTURES["family_min"][0])
    a, b = MPCSolver(qp, **_kw()), MPCSolver(qp, **_kw())
    a.solve(), b.solve()
    a.adjoint(gx)
    a.warm_start_last(0.99)
    b.warm_start_last(0.99)
    assert_same(a.solve(), b.solve())


# ------------------------------------------------------------------ 6. residual
@pytest.mark.parametrize("name", list(FIXTURES))
def test_residual_is_small(name):
    info = case(name)["info"]
    print("residual", name, info["last_residual"])
    assert np.isfinite(info["last_residual"]) and info["last_residual"] < TOL_LINEAR_SOLVE
    assert info["n_adjoints"] == 1 and info["n_adjoint_factorizations"] == 1


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    import torch
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    from madipm_amd import solver as S
    import ctypes as C
    qp, gx, _, _ = _reference(FIXTURES["family_min"][0])
    s = MPCSolver(qp, **_kw())
    with pytest.raises(MadIPMError, match="no solve has run"):
        s.adjoint(gx)
    with pytest.raises(MadIPMError, match="no solve has run"):
        s.adjoint_device(torch.as_tensor(gx, device="cuda"))
    s.set_max_iter(2)
    assert s.solve().status == S.MAXIMUM_ITERATIONS_EXCEEDED
    with pytest.raises(MadIPMError, match="not SOLVE_SUCCEEDED"):
        s.adjoint(gx)
    s.set_max_iter(300)
    assert s.solve().status == 1
    good = s.adjoint(gx)
    s.update(c=qp.c * 1.01)
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.adjoint(gx)
    assert s.solve().status == 1
    s.adjoint(gx)
    s.update_device(c=torch.as_tensor(qp.c, device="cuda"))
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.adjoint(gx)
    assert s.solve().status == 1
    s.initialize()
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.adjoint(gx)
    assert s.solve().status == 1
    # NULL gx, and no output at all, at the C interface
    g = L.QPGrad()
    buf = np.empty(qp.nvar)
    g.c = L.ptr(buf, C.c_double)
    assert L.lib.madipm_solver_adjoint(s.h, None, C.byref(g)) < 0
    assert b"gx is NULL" in L.madipm_last_error()
    assert L.lib.madipm_solver_adjoint(s.h, L.ptr(gx, C.c_double), C.byref(L.QPGrad())) < 0
    assert b"all seven outputs are NULL" in L.madipm_last_error()
    assert L.lib.madipm_solver_adjoint_device(s.h, None, C.byref(g), None) < 0
    assert b"gx is NULL" in L.madipm_last_error()
    # after all that a successful adjoint still works, with the bits of the first
    again = s.adjoint(gx)
    for k in O.NAMES:
        assert np.array_equal(again[k], good[k]), k
    # the other formulations, with a message that says they are still to come
    lp, glp = O.lp_fixture()
    for kkt in (S.ScaledSparseKKTSystem, S.NormalKKTSystem):
        t = MPCSolver(lp, **_kw(kkt_system=kkt))
        assert t.solve().status == 1
        with pytest.raises(MadIPMError, match="later release"):
            t.adjoint(glp)
        assert t.adjoint_info() == {"n_adjoints": 0, "n_adjoint_factorizations": 0, "last_residual": 0.0}


def test_refused_on_a_solver_with_a_communicator():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    qp, gx, _, _ = _reference(FIXTURES["family_min"][0])
    cb = L.ALLREDUCE_FN(lambda p, n, ctx: 0)          # one rank: the sum over the ranks is the buffer itself
    comm = L.vp()
    L.check(L.lib.madipm_comm_create_host(1, 0, cb, None, C.byref(comm)), "comm_create_host")
    s = MPCSolver(qp, **_kw())
    # MPCSolver takes the distributed constructor only for comm.size > 1: call it directly
    h = L.vp()
    L.check(L.lib.madipm_solver_create_dist(C.byref(s._q), C.byref(s.options), comm, C.byref(h)), "create_dist")
    L.lib.madipm_solver_destroy(s.h)
    s.h = h
    try:
        assert s.solve().status == 1
        with pytest.raises(MadIPMError, match="communicator"):
            s.adjoint(gx)
    finally:
        L.lib.madipm_solver_destroy(s.h)
        s.h = None
        L.lib.madipm_comm_destroy(comm)


# ------------------------------------------------------------------ 8. the torch layer
def test_layer_backward_is_adjoint_device():
    import torch
    from madipm_amd import MPCSolver, QPLayer
    qp, gx, _, _ = _reference(FIXTURES["family_min"][0])
    dev = torch.device("cuda")
    t = {k: torch.as_tensor(np.asarray(getattr(qp, k), float), device=dev) for k in O.NAMES}
    s = MPCSolver(qp, **_kw())
    layer = QPLayer(s)
    # all seven
    leaf = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    x = layer(**leaf)
    n0 = s.adjoint_info()["n_adjoints"]
    x.backward(torch.as_tensor(gx, device=dev))
    ref = s.adjoint_device(torch.as_tensor(gx, device=dev))
    assert s.adjoint_info()["n_adjoints"] == n0 + 2
    for k in O.NAMES:
        assert torch.equal(leaf[k].grad, ref[k]), k
    assert torch.equal(x.detach(), s.solution_device()["solution"])
    # the same bits as a solver that was never updated: update_device installed the same numbers
    plain = case("family_min")
    for k in O.NAMES:
        assert np.array_equal(ref[k].cpu().numpy(), plain["g"][k]), k
    # one tensor as both bounds of the equality rows receives ay once
    eq = np.flatnonzero(qp.lcon == qp.ucon)
    assert list(eq) == [0, 1]
    b = t["lcon"][:2].clone().requires_grad_(True)
    c = t["c"].clone().requires_grad_(True)
    lcon, ucon = torch.cat([b, t["lcon"][2:]]), torch.cat([b, t["ucon"][2:]])
    x = layer(c=c, lcon=lcon, ucon=ucon, lvar=t["lvar"])         # lvar: no requires_grad
    (x * torch.as_tensor(gx, device=dev)).sum().backward()
    assert torch.equal(b.grad, ref["lcon"][:2]) and torch.equal(c.grad, ref["c"])
    assert torch.equal(ref["ucon"][:2], torch.zeros(2, dtype=torch.float64, device=dev))
    assert t["lvar"].grad is None
    # exactly the gradients of the tensors that require grad are computed
    seen = {}
    orig = s.adjoint_device

    def spy(gx_, want=None, stream=None):
        seen["want"] = tuple(want)
        seen["out"] = orig(gx_, want=want, stream=stream)
        return seen["out"]
    s.adjoint_device = spy
    only = t["uvar"].clone().requires_grad_(True)
    x = layer(uvar=only, lvar=t["lvar"], c=t["c"])
    n1 = s.adjoint_info()["n_adjoints"]
    x.backward(torch.as_tensor(gx, device=dev))
    assert seen["want"] == ("uvar",) and sorted(seen["out"]) == ["uvar"]
    assert s.adjoint_info()["n_adjoints"] == n1 + 1
    assert torch.equal(only.grad, ref["uvar"])
    # nothing requires grad: backward is never asked for, the adjoint never runs
    x = layer(c=t["c"])
    assert not x.requires_grad and s.adjoint_info()["n_adjoints"] == n1 + 1


def test_layer_raises_when_the_solve_fails():
    import torch
    from madipm_amd import MPCSolver, QPLayer, MadIPMError
    qp, _, _, _ = _reference(FIXTURES["family_min"][0])
    s = MPCSolver(qp, **_kw())
    s.set_max_iter(2)
    with pytest.raises(MadIPMError, match="MAXIMUM_ITERATIONS_EXCEEDED"):
        QPLayer(s)(c=torch.as_tensor(qp.c, device="cuda").requires_grad_(True))
