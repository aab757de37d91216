"""MPCSolver.polish / polish_device on the GPU against the CPU oracle (polish_oracle.py): the
verdict and the set, the polished point against a dense exact solve on the returned set, the exact properties
(bounds attained bitwise, inactive multipliers 0), the KKT certificate on the unscaled problem, the routes
(host / device / repeated / subsets / a supplied set / a side stream give the same bits), the factor's tags and
the solver's state, the failure modes and the refusals.  Fixtures and solver options are
test_adjoint_full_gpu.py's, plus a problem without bounds and one without rows."""
from __future__ import annotations

import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import adjoint_full_oracle as F  # noqa: E402
import adjoint_oracle as O  # noqa: E402
import polish_oracle as P  # noqa: E402
from helpers import box_qp, free_eq_qp, kkt_properties_general  # noqa: E402
from test_adjoint_full_gpu import spmv_width  # noqa: E402
from test_adjoint_gpu import _kw  # noqa: E402
from test_update_gpu import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

# Largest figures measured on the MI355X; each bound is 10 x the largest, under its cap.
# err against the dense exact solve on the returned set, by fixture (largest block): the 7 x 5 family seeds 0-3
# 1.1e-15 / 1.5e-15 / 3.1e-16 / 1.8e-15, maximise 1.1e-15, duplicated 1.8e-15, scaled 4.7e-15 (y), the LP 1.7e-16,
# the sparse QP at G = 64 5.6e-15 (y), the row-length fixture at G = 4 1.6e-15, no bounds 8.3e-16, no rows 2.2e-16.
# The interior point the solver returned was 1.2e-11 ... 6.2e-8 from the same exact solution.
EXACT_MEASURED = 5.61e-15
EXACT_TOL = 10.0 * EXACT_MEASURED
EXACT_CAP = 1e-10              # two orders below the interior point's own distance
# the certificate of the polished point: pr <= 2.25e-16 (the sparse QP), du <= 3.90e-16 (no bounds), compl <=
# 5.76e-14 (the scaled family, whose multipliers are 1e3 times the family's; 1.5e-16 on the others); the interior
# point gives up to 6.0e-12, 9.1e-13 and 2.2e-9
KKT_MEASURED = {"pr": 2.25e-16, "du": 3.90e-16, "compl": 5.76e-14}
KKT_TOL = {k: 10.0 * v for k, v in KKT_MEASURED.items()}
KKT_CAP = 1e-11

BLOCKS = ("x", "y", "zl", "zu", "cons")


def _free_eq():
    return free_eq_qp()[0], None


def _box():
    return box_qp(), None


# name -> (problem, MADIPM_SPMV_G during construction or None)
FIXTURES = {
    "family_0": (lambda: O.family(0), None),
    "family_1": (lambda: O.family(1), None),
    "family_2": (lambda: O.family(2), None),
    "family_3": (lambda: O.family(3), None),
    "family_max": (lambda: O.family(0, minimize=False), None),
    "family_dup": (lambda: O.duplicated_family(0)[:2], None),
    "family_scaled": (lambda: O.scaled_family(0), None),
    "lp": (O.lp_fixture, None),
    "sparse_g64": (O.sparse_fixture, 64),
    "rowlength_g4": (F.rowlength_fixture, 4),
    "no_bounds": (_free_eq, None),
    "no_rows": (_box, None),
}
_cache, _qps = {}, {}


def problem(name):
    if name not in _qps:
        _qps[name] = FIXTURES[name][0]()[0]
    return _qps[name]


def new_solver(name, **extra):
    from madipm_amd import MPCSolver
    G = FIXTURES[name][1]
    with spmv_width(G):
        s = MPCSolver(problem(name), **_kw(**extra))
    if G is not None:
        assert s.spmv_group() == G
    return s


def case(name):
    """The fixture solved and polished on the GPU once (host route, all seven blocks), and the oracle's dense
    exact solve on the returned set: computed once, never modified."""
    if name not in _cache:
        qp = problem(name)
        s = new_solver(name)
        st = s.solve()
        assert st.status == 1, (name, st.status_name)
        pol = s.polish()
        ex = P.exact(qp, pol["active_var"], pol["active_row"])
        _cache[name] = dict(qp=qp, solver=s, stats=st, pol=pol, exact=ex)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _cache.clear()          # the solvers go while the library is still loaded


def _point(st):
    return {"x": st.solution, "y": st.multipliers, "zl": st.multipliers_L, "zu": st.multipliers_U}


def _same(a, b, keys=None):
    for k in keys or [k for k in a if k != "info"]:
        x = a[k].cpu().numpy() if isinstance(a[k], torch.Tensor) else a[k]
        y = b[k].cpu().numpy() if isinstance(b[k], torch.Tensor) else b[k]
        assert x.dtype == y.dtype and np.array_equal(x, y), k


def test_tolerances_fit_the_caps():
    assert EXACT_TOL <= EXACT_CAP and max(KKT_TOL.values()) <= KKT_CAP


# ------------------------------------------------------------------ 1-4: the polished point
@pytest.mark.parametrize("name", list(FIXTURES))
def test_verdict_and_set(name):
    from madipm_amd import PolishVerdict
    c = case(name)
    info = c["pol"]["info"]
    print("info", name, info)
    assert info["verdict"] == PolishVerdict.POLISHED, info
    av, ar = P.guess(c["qp"], _point(c["stats"]))
    assert np.array_equal(c["pol"]["active_var"], av) and np.array_equal(c["pol"]["active_row"], ar)
    assert c["pol"]["active_var"].dtype == np.int8 and c["pol"]["active_row"].dtype == np.int8
    assert info["n_active"] == np.count_nonzero(av) + np.count_nonzero(ar)
    assert info["residual"] <= 1e-10 and info["n_polishes"] >= 1 and info["n_polish_factorizations"] == 1
    if name == "no_bounds":
        assert info["n_active"] == 0 and info["min_multiplier"] == np.inf and info["min_gap"] == np.inf
    if name == "no_rows":
        assert c["pol"]["y"].shape == c["pol"]["cons"].shape == c["pol"]["active_row"].shape == (0,)
    if name == "sparse_g64":
        assert info["n_active"] == 180


@pytest.mark.parametrize("name", list(FIXTURES))
def test_against_the_exact_solve(name):
    c = case(name)
    e = {k: P.err(c["pol"][k], c["exact"][k]) for k in BLOCKS}
    d = P.distance(_point(c["stats"]), c["exact"])
    print("exact", name, {k: f"{v:.2e}" for k, v in e.items()}, f"interior point {d:.1e}")
    assert max(e.values()) <= EXACT_TOL, e


@pytest.mark.parametrize("name", list(FIXTURES))
def test_exact_properties(name):
    c = case(name)
    qp, pol = c["qp"], c["pol"]
    av, ar = pol["active_var"], pol["active_row"]
    assert np.array_equal(pol["x"][av < 0], qp.lvar[av < 0]) and np.array_equal(pol["x"][av > 0], qp.uvar[av > 0])
    assert not np.any(pol["zl"][av >= 0]) and not np.any(pol["zu"][av <= 0])
    assert np.array_equal(pol["cons"][ar < 0], qp.lcon[ar < 0]) and np.array_equal(pol["cons"][ar > 0], qp.ucon[ar > 0])
    fixed = qp.lvar == qp.uvar
    assert np.array_equal(pol["x"][fixed], qp.lvar[fixed]) and not np.any(av[fixed]) and not np.any(ar[qp.lcon == qp.ucon])


@pytest.mark.parametrize("name", list(FIXTURES))
def test_kkt_certificate(name):
    c = case(name)
    pol = c["pol"]
    st = types.SimpleNamespace(solution=pol["x"], multipliers=pol["y"], multipliers_L=pol["zl"],
                               multipliers_U=pol["zu"], constraints=pol["cons"])
    p = kkt_properties_general(c["qp"], st)
    q = kkt_properties_general(c["qp"], c["stats"])
    print("kkt", name, {k: f"{p[k]:.2e}" for k in KKT_TOL}, "interior point", {k: f"{q[k]:.2e}" for k in KKT_TOL})
    for k, tol in KKT_TOL.items():
        assert p[k] <= tol, (k, p[k])
    assert p["zoff"] == 0.0 and p["bounds"] <= 0.0 and p["zmin"] >= 0.0, p


# ------------------------------------------------------------------ 5: bits
@pytest.mark.parametrize("name", ["family_0", "family_scaled", "lp", "sparse_g64", "rowlength_g4", "no_bounds",
                                  "no_rows"])
def test_routes_give_identical_bits(name):
    c = case(name)
    s, pol = c["solver"], c["pol"]
    nf = s.polish_info()["n_polish_factorizations"]
    again = s.polish()
    _same(again, pol)
    dev = s.polish_device()
    torch.cuda.synchronize()
    _same(dev, pol)
    assert dev["info"]["verdict"] == pol["info"]["verdict"] and dev["info"]["residual"] == pol["info"]["residual"]
    for want in (["x"], ["zl", "zu"], ["cons", "active_row"], ["y", "active_var"]):
        sub = s.polish(want=want)
        assert sorted(k for k in sub if k != "info") == sorted(want)
        _same(sub, pol, want)
        _same(s.polish_device(want=want), pol, want)
    # the guessed set supplied: the same bits, on both routes, and no new factor
    sup = s.polish(active_var=pol["active_var"], active_row=pol["active_row"])
    _same(sup, pol)
    dsup = s.polish_device(active_var=torch.as_tensor(pol["active_var"], device="cuda"),
                           active_row=torch.as_tensor(pol["active_row"], device="cuda"))
    _same(dsup, pol)
    assert s.polish_info()["n_polish_factorizations"] == nf
    assert s.polish_info() == dsup["info"]


def test_device_route_honours_the_stream():
    c = case("family_0")
    s, pol = c["solver"], c["pol"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        av = torch.as_tensor(pol["active_var"], device="cuda") * 1          # produced on the side stream
        ar = torch.as_tensor(pol["active_row"], device="cuda") * 1
        out = s.polish_device(stream=side, active_var=av, active_row=ar)
        doubled = {k: 2 * out[k] for k in P_NAMES}                          # consumed on it, without a host wait
    side.synchronize()
    for k in P_NAMES:
        assert np.array_equal(doubled[k].cpu().numpy(), 2 * pol[k]), k


P_NAMES = BLOCKS + ("active_var", "active_row")


# ------------------------------------------------------------------ 6: the factor's tags, the solver's state
@pytest.mark.parametrize("name", ["family_0", "family_scaled", "sparse_g64"])
def test_factor_tags_and_the_next_solve(name):
    gx = np.random.default_rng(5).uniform(0.5, 1.5, problem(name).nvar)
    a = new_solver(name)
    first = a.solve()
    g0 = a.adjoint(gx)
    assert a.adjoint_info()["n_adjoint_factorizations"] == 1
    p1 = a.polish()
    p2 = a.polish()
    assert p2["info"]["n_polish_factorizations"] == 1 and p2["info"]["n_polishes"] == 2
    _same(p1, case(name)["pol"])
    _same(p2, p1)
    g1 = a.adjoint(gx)                    # the polish overwrote the factor: the adjoint factorises again
    assert a.adjoint_info()["n_adjoint_factorizations"] == 2
    p3 = a.polish()                       # and so does the polish after it
    assert p3["info"]["n_polish_factorizations"] == 2
    _same(p3, p1)
    second = a.solve()
    p4 = a.polish()
    assert p4["info"]["n_polish_factorizations"] == 3
    # solve(); polish(); solve() against solve(); solve(), and solve(); polish(); adjoint() against solve(); adjoint()
    b = new_solver(name)
    assert_same(first, b.solve())
    gb = b.adjoint(gx)
    assert_same(second, b.solve())
    for k in O.NAMES:
        assert np.array_equal(g0[k], gb[k]) and np.array_equal(g1[k], gb[k]), k
    # a different sigma is a different factor
    p5 = a.polish(sigma=1e8)
    assert p5["info"]["n_polish_factorizations"] == 4 and p5["info"]["verdict"] == 0
    assert P.distance(p5, p4, BLOCKS) <= EXACT_TOL


# ------------------------------------------------------------------ 7: the failure modes
def test_failure_modes():
    from madipm_amd import PolishVerdict
    c = case("family_0")
    s, pol = c["solver"], c["pol"]
    sol = s.solution_device()
    keys = {"x": "solution", "y": "multipliers", "zl": "multipliers_L", "zu": "multipliers_U", "cons": "constraints"}

    def check(res, verdict, sol):
        assert res["info"]["verdict"] == verdict, res["info"]
        for k, kk in keys.items():
            got = res[k].cpu().numpy() if isinstance(res[k], torch.Tensor) else res[k]
            assert np.array_equal(got, sol[kk].cpu().numpy()), k

    forced = (pol["active_var"].copy(), pol["active_row"].copy())
    forced[0][1] = 1                                      # variable 1's inactive upper bound
    a = s.polish(active_var=forced[0], active_row=forced[1])
    print("forced upper", a["info"])
    check(a, PolishVerdict.WRONG_SET, sol)
    assert abs(a["info"]["min_multiplier"] + 1.03) <= 0.01 and a["info"]["residual"] <= 1e-10
    assert np.array_equal(a["active_var"], forced[0]) and np.array_equal(a["active_row"], forced[1])
    ad = s.polish_device(active_var=torch.as_tensor(forced[0], device="cuda"),
                         active_row=torch.as_tensor(forced[1], device="cuda"))
    check(ad, PolishVerdict.WRONG_SET, sol)
    empty = (np.zeros_like(forced[0]), np.zeros_like(forced[1]))
    b = s.polish(active_var=empty[0], active_row=empty[1])
    print("empty set", b["info"])
    check(b, PolishVerdict.WRONG_SET, sol)
    assert abs(b["info"]["min_gap"] + 0.13) <= 0.01 and b["info"]["n_active"] == 0
    # after the failures the guess still gives the bits of the first call
    _same(s.polish(), pol)
    lp = case("lp")
    four = (lp["pol"]["active_var"].copy(), lp["pol"]["active_row"].copy())
    four[0][3] = -1                                       # a fourth variable at a bound under three equality rows
    d = lp["solver"].polish(active_var=four[0], active_row=four[1])
    print("lp, four active", d["info"])
    check(d, PolishVerdict.NO_CONVERGENCE, lp["solver"].solution_device())
    assert not d["info"]["residual"] <= 1e-3
    _same(lp["solver"].polish(), lp["pol"])


# ------------------------------------------------------------------ 8: the refusals
def test_refusals():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    from madipm_amd import solver as S
    qp = problem("family_0")
    s = MPCSolver(qp, **_kw())
    with pytest.raises(MadIPMError, match="madipm_solver_polish: no solve has run"):
        s.polish()
    with pytest.raises(MadIPMError, match="madipm_solver_polish_device: no solve has run"):
        s.polish_device()
    assert s.polish_info()["verdict"] is None and s.polish_info()["n_polishes"] == 0
    s.set_max_iter(2)
    assert s.solve().status == S.MAXIMUM_ITERATIONS_EXCEEDED
    with pytest.raises(MadIPMError, match="not SOLVE_SUCCEEDED"):
        s.polish()
    s.set_max_iter(300)
    assert s.solve().status == 1
    good = s.polish()
    s.update(c=qp.c * 1.01)
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.polish()
    assert s.solve().status == 1
    s.update(c=qp.c)
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.polish_device()
    assert s.solve().status == 1
    # the supplied set: one pointer only, and codes the problem has no bound for, on both routes
    av, ar = good["active_var"], good["active_row"]
    out = L.PolishOut()
    xbuf = np.empty(qp.nvar)
    out.x = L.ptr(xbuf, C.c_double)
    for fn, tail in ((L.lib.madipm_solver_polish, ()), (L.lib.madipm_solver_polish_device, (None,))):
        assert fn(s.h, None, L.ptr(av, C.c_int8), None, C.byref(out), None, *tail) < 0
        assert b"exactly one of active_var and active_row" in L.madipm_last_error()
        assert fn(s.h, None, None, L.ptr(ar, C.c_int8), C.byref(out), None, *tail) < 0
        assert b"exactly one of active_var and active_row" in L.madipm_last_error()
        assert fn(s.h, None, None, None, C.byref(L.PolishOut()), None, *tail) < 0
        assert b"all seven outputs are NULL" in L.madipm_last_error()
        assert fn(s.h, None, None, None, None, None, *tail) < 0
        assert b"null output struct" in L.madipm_last_error()
        for steps in (-1, 9):
            assert fn(s.h, C.byref(L.PolishOpts(1e10, 1e-10, 1e-9, 1e-9, steps)), None, None, C.byref(out), None,
                      *tail) < 0
            assert b"refine_steps must be in 0..8" in L.madipm_last_error()
        assert fn(s.h, C.byref(L.PolishOpts(0.0, 1e-10, 1e-9, 1e-9, 2)), None, None, C.byref(out), None, *tail) < 0
        assert b"sigma must be positive" in L.madipm_last_error()
    for var, row, code in ((0, None, 1), (3, None, -1), (None, 0, -1), (None, 2, 1), (4, None, -1), (1, None, 2)):
        bv, br = av.copy(), ar.copy()     # variable 0: no upper bound; 3: fixed; 4: free; row 0: equality; row 2: no upper side
        if var is not None:
            bv[var] = code
        else:
            br[row] = code
        with pytest.raises(MadIPMError, match="madipm_solver_polish: the supplied set has a code"):
            s.polish(active_var=bv, active_row=br)
        with pytest.raises(MadIPMError, match="madipm_solver_polish_device: the supplied set has a code"):
            s.polish_device(active_var=torch.as_tensor(bv, device="cuda"), active_row=torch.as_tensor(br, device="cuda"))
    # the device route's arguments, before any library call
    dav, dar = torch.as_tensor(av, device="cuda"), torch.as_tensor(ar, device="cuda")
    with pytest.raises(TypeError, match="expected torch.int8"):
        s.polish_device(active_var=dav.double(), active_row=dar)
    with pytest.raises(TypeError, match="expected a GPU tensor"):
        s.polish_device(active_var=dav.cpu(), active_row=dar)
    with pytest.raises(ValueError, match="shape"):
        s.polish_device(active_var=dav[:-1], active_row=dar)
    with pytest.raises(TypeError, match="must be a torch tensor"):
        s.polish_device(active_var=av, active_row=ar)
    with pytest.raises(TypeError, match="stream must be a torch.cuda.Stream"):
        s.polish_device(stream=0)
    # after all that a successful call still works, with the bits of the first
    _same(s.polish(), good)
    # the other formulations
    lp = problem("lp")
    for kkt in (S.ScaledSparseKKTSystem, S.NormalKKTSystem):
        t = MPCSolver(lp, **_kw(kkt_system=kkt))
        assert t.solve().status == 1
        with pytest.raises(MadIPMError, match="later release"):
            t.polish()
        assert t.polish_info()["n_polishes"] == 0


def test_refused_on_a_solver_with_a_communicator():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    qp = problem("family_0")
    cb = L.ALLREDUCE_FN(lambda p, n, ctx: 0)          # one rank: the sum over the ranks is the buffer itself
    comm = L.vp()
    L.check(L.lib.madipm_comm_create_host(1, 0, cb, None, C.byref(comm)), "comm_create_host")
    s = MPCSolver(qp, **_kw())
    h = L.vp()
    L.check(L.lib.madipm_solver_create_dist(C.byref(s._q), C.byref(s.options), comm, C.byref(h)), "create_dist")
    L.lib.madipm_solver_destroy(s.h)
    s.h = h
    try:
        assert s.solve().status == 1
        with pytest.raises(MadIPMError, match="communicator"):
            s.polish()
    finally:
        L.lib.madipm_solver_destroy(s.h)
        s.h = None
        L.lib.madipm_comm_destroy(comm)
