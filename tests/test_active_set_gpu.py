"""MPCSolver.active_set_solve / active_set_solve_device on the GPU against the CPU oracle (active_set_oracle.py,
DESIGN §13h): verdict, rounds, changed codes and the final set of every case test_active_set_cpu.py accepted; the
POLISHED point against a dense exact solve on the final set, its KKT certificate on the updated problem and the
exact properties; a twin solver's update -> solve -> polish; the cold start; the routes (multi-round / one round
from the final set / host / device / a side stream / subsets give the same bits, a repeated call does not
factorise); the failing cases; the solver's state after the call (the next solve, the polished sensitivities, the
refusals); the refusals of the call itself; the torch layer's active-set route.  Solver options are
test_polish_gpu.py's."""
from __future__ import annotations

import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import active_set_oracle as A  # noqa: E402
import adjoint_full_oracle as F  # noqa: E402
import adjoint_oracle as O  # noqa: E402
import polish_oracle as P  # noqa: E402
import polished_sens_oracle as Q  # noqa: E402
import tangent_oracle as T  # noqa: E402
import test_active_set_cpu as K  # noqa: E402
import test_polish_gpu as G  # noqa: E402
import test_polished_sens_gpu as GS  # noqa: E402
from helpers import kkt_properties_general  # noqa: E402
from test_adjoint_gpu import _kw  # noqa: E402
from test_update_gpu import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

# Largest figures measured on the MI355X over all POLISHED cases; each bound is 10 x the largest,
# under the cap test_polish_gpu.py uses.  err against the dense exact solve on the final set (largest block):
# the scaled family 8.9e-15 (y, shifted seed 4), the sparse QP 4.3e-15 (y), family seed 1 4.0e-15 (zu), seeds 0 and 3
# 1.9e-15 / 2.1e-15 (zl, cold), the row-length fixture at G = 4 1.0e-15, no bounds 6.7e-16, no rows 4.4e-16, seed 2,
# maximise and duplicated <= 3.6e-16.  A twin's update -> solve -> polish is within 3.9e-15 of the same points.
EXACT_MEASURED = 8.89e-15
EXACT_TOL = 10.0 * EXACT_MEASURED
# the certificate on the updated problem: pr <= 3.91e-16 (the sparse QP), du <= 2.85e-15 (family seed 1), compl <=
# 9.19e-14 (the scaled family, whose multipliers are 1e3 times the family's)
KKT_MEASURED = {"pr": 3.91e-16, "du": 2.85e-15, "compl": 9.19e-14}
KKT_TOL = {k: 10.0 * v for k, v in KKT_MEASURED.items()}
# the polished sensitivities at the active-set point against the dense derivative on the updated problem and the
# final set (err of polished_sens_oracle, largest block): tangent 3.1e-15 (the scaled family's cons), adjoint 4.5e-16
# (the sparse QP's ucon)
TANGENT_MEASURED, ADJOINT_MEASURED = 3.10e-15, 4.49e-16
TANGENT_TOL, ADJOINT_TOL = 10.0 * TANGENT_MEASURED, 10.0 * ADJOINT_MEASURED

BLOCKS = G.BLOCKS
NAMES7 = BLOCKS + ("active_var", "active_row")
CASES = {c.id: c for c in K.CASES}
KEPT_POLISHED = [c for c in K.POLISHED_CASES if c.start == "kept"]
COLD = [c for c in K.CASES if c.start == "zero"]
FAILING = [c for c in K.CASES if c.verdict != P.POLISHED]
_cache = {}


def fields(case):
    """update()'s arguments of the case: what its generator changed."""
    qp = K.updated(case)
    names = O.NAMES if case.gen[0] == "perturb" else ("c", "lcon", "ucon", "lvar", "uvar")
    return {k: np.asarray(getattr(qp, k), float) for k in names}


def kept_solver(case):
    """A solver that solved and polished the base problem (so it keeps the base set) and took the case's update."""
    from madipm_amd import PolishVerdict
    s = G.new_solver(case.fixture)
    assert s.solve().status == 1
    pol = s.polish(want=["active_var", "active_row"])
    assert pol["info"]["verdict"] == PolishVerdict.POLISHED
    av, ar = K.start_set(case)
    assert np.array_equal(pol["active_var"], av) and np.array_equal(pol["active_row"], ar)
    s.update(**fields(case))
    return s


def twin_solver(case):
    s = G.new_solver(case.fixture)
    if case.gen:
        s.update(**fields(case))
    return s


def run(case):
    """The case on the GPU once (host route, all seven blocks, from the kept set or, cold, on a fresh solver from
    the all-zero set), with the oracle's run and the dense exact solve on the final set: never modified."""
    if case.id not in _cache:
        qp, ref = K.solved(case)
        if case.start == "kept":
            s = kept_solver(case)
            res = s.active_set_solve()
        else:
            s = G.new_solver(case.fixture)
            res = s.active_set_solve(active_var=np.zeros(qp.nvar, np.int8), active_row=np.zeros(qp.ncon, np.int8))
        ex = P.exact(qp, res["active_var"], res["active_row"]) if res["info"]["verdict"] == 0 else None
        _cache[case.id] = dict(qp=qp, solver=s, res=res, ref=ref, exact=ex)
    return _cache[case.id]


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _cache.clear()          # the solvers go while the library is still loaded


def _same(a, b, keys=None):
    for k in keys or [k for k in a if k != "info"]:
        x = a[k].cpu().numpy() if isinstance(a[k], torch.Tensor) else a[k]
        y = b[k].cpu().numpy() if isinstance(b[k], torch.Tensor) else b[k]
        assert x.dtype == y.dtype and np.array_equal(x, y), k


def _check_info(info, ref):
    assert info["verdict"] == ref["verdict"], (info, ref["verdict"])
    assert (info["rounds"], info["n_changed"], info["n_active"]) == (ref["rounds"], ref["n_changed"], ref["n_active"])


def _check_point(c, res):
    """The polished blocks against the exact solve, the certificate on the updated problem, the exact properties."""
    qp, ex = c["qp"], c["exact"]
    e = {k: P.err(res[k], ex[k]) for k in BLOCKS}
    st = types.SimpleNamespace(solution=res["x"], multipliers=res["y"], multipliers_L=res["zl"],
                               multipliers_U=res["zu"], constraints=res["cons"])
    p = kkt_properties_general(qp, st)
    print("exact", {k: f"{v:.2e}" for k, v in e.items()}, "kkt", {k: f"{p[k]:.2e}" for k in KKT_TOL})
    assert max(e.values()) <= EXACT_TOL, e
    for k, tol in KKT_TOL.items():
        assert p[k] <= tol, (k, p[k])
    assert p["zoff"] == 0.0 and p["bounds"] <= 0.0 and p["zmin"] >= 0.0, p
    av, ar = res["active_var"], res["active_row"]
    assert np.array_equal(res["x"][av < 0], qp.lvar[av < 0]) and np.array_equal(res["x"][av > 0], qp.uvar[av > 0])
    assert not np.any(res["zl"][av >= 0]) and not np.any(res["zu"][av <= 0])
    assert np.array_equal(res["cons"][ar < 0], qp.lcon[ar < 0]) and np.array_equal(res["cons"][ar > 0], qp.ucon[ar > 0])
    fixed = qp.lvar == qp.uvar
    assert np.array_equal(res["x"][fixed], qp.lvar[fixed]) and not np.any(av[fixed]) and not np.any(ar[qp.lcon == qp.ucon])


def test_tolerances_fit_the_caps():
    assert EXACT_TOL <= G.EXACT_CAP and max(KKT_TOL.values()) <= G.KKT_CAP
    assert TANGENT_TOL <= GS.ACCURACY_CAP and ADJOINT_TOL <= GS.ACCURACY_CAP
    # every fixture the issue names has a case, and every case passed the CPU conditions (test_active_set_cpu.py)
    assert {c.fixture for c in K.CASES} == set(G.FIXTURES)


# ------------------------------------------------------------------ 1: the table, from the kept set after an update
@pytest.mark.parametrize("case", KEPT_POLISHED, ids=lambda c: c.id)
def test_kept_set_after_an_update(case):
    from madipm_amd import PolishVerdict
    c = run(case)
    res, ref = c["res"], c["ref"]
    info = res["info"]
    print("info", case.id, info)
    assert info["verdict"] == PolishVerdict.POLISHED
    _check_info(info, ref)
    assert np.array_equal(res["active_var"], ref["active_var"]) and np.array_equal(res["active_row"], ref["active_row"])
    assert res["active_var"].dtype == np.int8 and res["active_row"].dtype == np.int8
    assert info["residual"] <= 1e-10 and info["n_calls"] == 1 and info["n_factorizations"] == info["rounds"]
    if case.fixture == "no_bounds":
        assert info["n_active"] == 0 and info["min_multiplier"] == np.inf and info["min_gap"] == np.inf
    if case.fixture == "no_rows":
        assert res["y"].shape == res["cons"].shape == res["active_row"].shape == (0,)
    _check_point(c, res)


# ------------------------------------------------------------------ 2: a twin's update -> solve -> polish
@pytest.mark.parametrize("case", [c for c in KEPT_POLISHED if c.gen[1] in (0, 3)], ids=lambda c: c.id)
def test_twin_solve_and_polish_agrees(case):
    from madipm_amd import PolishVerdict
    c = run(case)
    t = twin_solver(case)
    assert t.solve().status == 1
    pol = t.polish()
    assert pol["info"]["verdict"] == PolishVerdict.POLISHED
    assert np.array_equal(pol["active_var"], c["res"]["active_var"])
    assert np.array_equal(pol["active_row"], c["res"]["active_row"])
    e = {k: P.err(pol[k], c["exact"][k]) for k in BLOCKS}
    d = {k: P.err(c["res"][k], pol[k]) for k in BLOCKS}
    print("twin vs exact", {k: f"{v:.2e}" for k, v in e.items()}, "active set vs twin", {k: f"{v:.2e}" for k, v in d.items()})
    assert max(e.values()) <= EXACT_TOL and max(d.values()) <= 2 * EXACT_TOL


# ------------------------------------------------------------------ 3: cold
@pytest.mark.parametrize("case", COLD, ids=lambda c: c.id)
def test_cold_solver_from_the_zero_set(case):
    from madipm_amd import MadIPMError, PolishVerdict
    c = run(case)
    s, res = c["solver"], c["res"]
    print("info", case.id, res["info"])
    assert res["info"]["verdict"] == PolishVerdict.POLISHED
    _check_info(res["info"], c["ref"])
    assert np.array_equal(res["active_var"], c["ref"]["active_var"]) and np.array_equal(res["active_row"], c["ref"]["active_row"])
    _check_point(c, res)
    assert s.polish_info()["verdict"] is None and s.counters()["n_updates"] == 0
    for call in (lambda: s.adjoint(np.ones(c["qp"].nvar)), s.polish, s.warm_start_last):
        with pytest.raises(MadIPMError, match="no solve has run"):      # nothing of the interior-point state exists
            call()
    # the kept set is the final one now: the next call starts from it and holds its factor
    nf = res["info"]["n_factorizations"]
    again = s.active_set_solve()
    _same(again, res)
    assert again["info"]["rounds"] == 1 and again["info"]["n_changed"] == 0 and again["info"]["n_factorizations"] == nf
    # the first solve of this solver is a fresh solver's
    assert_same(s.solve(), G.new_solver(case.fixture).solve())


# ------------------------------------------------------------------ 4: bits
BITS = ["family_3-kept-shifted-2-0.1", "family_scaled-kept-shifted-3-0.1", "sparse_g64-kept-shifted-0-0.01",
        "sparse_g64-kept-perturb-0-0.03", "rowlength_g4-kept-shifted-3-0.1", "no_rows-kept-shifted-0-0.3",
        "no_bounds-kept-shifted-0-0.1"]


@pytest.mark.parametrize("cid", BITS)
def test_routes_give_identical_bits(cid):
    c = run(CASES[cid])
    s, res = c["solver"], c["res"]
    nf, calls = s.active_set_info()["n_factorizations"], s.active_set_info()["n_calls"]
    av, ar = res["active_var"], res["active_row"]
    one = s.active_set_solve(active_var=av, active_row=ar, max_rounds=1)      # the final set supplied: one round
    _same(one, res)
    assert one["info"]["rounds"] == 1 and one["info"]["n_changed"] == 0
    for k in ("verdict", "n_active", "residual", "min_multiplier", "min_gap"):
        assert one["info"][k] == res["info"][k], k
    _same(s.active_set_solve(), res)                                           # the kept set is the final one
    dev = s.active_set_solve_device()
    torch.cuda.synchronize()
    _same(dev, res)
    assert dev["info"]["residual"] == res["info"]["residual"]
    dav, dar = torch.as_tensor(av, device="cuda"), torch.as_tensor(ar, device="cuda")
    _same(s.active_set_solve_device(active_var=dav, active_row=dar), res)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sav, sar = dav * 1, dar * 1                                            # produced on the side stream
        out = s.active_set_solve_device(stream=side, active_var=sav, active_row=sar)
        doubled = {k: 2 * out[k] for k in NAMES7}                              # consumed on it, without a host wait
    side.synchronize()
    for k in NAMES7:
        assert np.array_equal(doubled[k].cpu().numpy(), 2 * res[k]), k
    for want in (["x"], ["zl", "zu"], ["cons", "active_row"], ["y", "active_var"]):
        sub = s.active_set_solve(want=want)
        assert sorted(k for k in sub if k != "info") == sorted(want)
        _same(sub, res, want)
        _same(s.active_set_solve_device(want=want), res, want)
    info = s.active_set_info()
    assert info["n_factorizations"] == nf and info["n_calls"] == calls + 13    # the factor of the last round served all
    assert s.active_set_solve(sigma=1e8)["info"]["n_factorizations"] == nf + 1  # another sigma is another factor


def test_polish_and_active_set_share_the_factor():
    """solve(); polish(); active_set_solve() on the same data: the kept set is the polish's, its factor is held."""
    from madipm_amd import PolishVerdict
    for name in ("family_0", "sparse_g64"):
        s = G.new_solver(name)
        assert s.solve().status == 1
        pol = s.polish()
        res = s.active_set_solve()
        assert res["info"]["verdict"] == PolishVerdict.POLISHED and res["info"]["rounds"] == 1
        assert res["info"]["n_factorizations"] == 0 and res["info"]["n_changed"] == 0
        _same(res, pol, ["active_var", "active_row"])
        assert max(P.err(res[k], pol[k]) for k in BLOCKS) <= 2 * EXACT_TOL
        again = s.polish()                                    # and the polish after it finds its own factor again
        assert again["info"]["n_polish_factorizations"] == 1
        _same(again, pol)
        s.adjoint(np.ones(G.problem(name).nvar))              # takes the LDL^T: the next call factorises
        assert s.active_set_solve()["info"]["n_factorizations"] == 1


# ------------------------------------------------------------------ 5: failures
@pytest.mark.parametrize("case", FAILING, ids=lambda c: c.id)
def test_failing_cases(case):
    import ctypes as C
    from madipm_amd import MadIPMError
    from madipm_amd import _lib as L
    c = run(case)
    s, res, ref, qp = c["solver"], c["res"], c["ref"], c["qp"]
    info = res["info"]
    print("info", case.id, info, "oracle", {k: ref[k] for k in ("residual", "min_multiplier", "min_gap")})
    _check_info(info, ref)
    assert np.array_equal(res["active_var"], ref["active_var"]) and np.array_equal(res["active_row"], ref["active_row"])
    assert all(res[k] is None for k in BLOCKS)
    if case.verdict == P.NO_CONVERGENCE:
        assert not info["residual"] <= K.RESID_MIN
    else:
        assert info["residual"] <= 1e-10
        assert min(abs(info["min_multiplier"] - ref["min_multiplier"]), abs(info["min_gap"] - ref["min_gap"])) <= 1e-9
    dres = s.active_set_solve_device(active_var=torch.as_tensor(K.start_set(case)[0], device="cuda"),
                                     active_row=torch.as_tensor(K.start_set(case)[1], device="cuda"))
    assert dres["info"]["verdict"] == info["verdict"] and all(dres[k] is None for k in BLOCKS)
    _same(dres, res, ["active_var", "active_row"])
    # the caller's arrays are not written: a sentinel survives, on the host route and on the device route
    sent = {k: np.full(max(n, 1), -7.25) for k, n in zip(BLOCKS, (qp.nvar, qp.ncon, qp.nvar, qp.nvar, qp.ncon))}
    out = L.PolishOut()
    for k in BLOCKS:
        setattr(out, k, L.ptr(sent[k], C.c_double))
    av, ar = K.start_set(case)
    ai = L.ActiveSetInfo()
    L.check(L.lib.madipm_solver_active_set_solve(s.h, None, L.ptr(av, C.c_int8), L.ptr(ar, C.c_int8), C.byref(out),
                                                 C.byref(ai)), "active_set_solve")
    assert ai.verdict == info["verdict"] and ai.rounds == info["rounds"]
    assert all(np.all(v == -7.25) for v in sent.values())
    dsent = {k: torch.full((len(v),), -7.25, dtype=torch.float64, device="cuda") for k, v in sent.items()}
    for k in BLOCKS:
        setattr(out, k, C.cast(dsent[k].data_ptr(), L.f64p))
    dav, dar = torch.as_tensor(av, device="cuda"), torch.as_tensor(ar, device="cuda")
    L.check(L.lib.madipm_solver_active_set_solve_device(
        s.h, None, C.cast(dav.data_ptr(), L.i8p), C.cast(dar.data_ptr(), L.i8p), C.byref(out), C.byref(ai),
        L.vp(torch.cuda.current_stream().cuda_stream)), "active_set_solve_device")
    torch.cuda.synchronize()
    assert ai.verdict == info["verdict"] and all(bool(torch.all(v == -7.25)) for v in dsent.values())
    # no current polished point; the interior-point calls are refused as after any update
    for call in (lambda: s.adjoint(np.ones(qp.nvar), polished=True), lambda: s.tangent(c=np.ones(qp.nvar), polished=True),
                 lambda: s.adjoint(np.ones(qp.nvar)), s.polish):
        with pytest.raises(MadIPMError, match="since the last solve"):
            call()
    # update; active-set solve; solve against update; solve
    assert_same(s.solve(), twin_solver(case).solve())


# ------------------------------------------------------------------ 6: the state after POLISHED
STATE = ["family_3-kept-shifted-2-0.1", "family_scaled-kept-shifted-3-0.1", "family_max-kept-shifted-3-0.1",
         "sparse_g64-kept-perturb-1-0.03", "rowlength_g4-kept-shifted-0-0.1"]


@pytest.mark.parametrize("cid", STATE)
def test_state_after_a_polished_call(cid):
    from madipm_amd import MadIPMError, PolishVerdict
    case = CASES[cid]
    qp = K.updated(case)
    s = kept_solver(case)                    # this test's own: it goes on to solve and update it
    res = s.active_set_solve()
    assert res["info"]["verdict"] == PolishVerdict.POLISHED
    av, ar = res["active_var"], res["active_row"]
    gx = np.random.default_rng(4100).uniform(0.5, 1.5, qp.nvar) * np.random.default_rng(4101).choice([-1.0, 1.0], qp.nvar)
    d, cot = T.directions(qp, 0), F.cotangents(qp, gx)
    before = s.polished_sens_info()
    tan = s.tangent(polished=True, **d)
    adj = s.adjoint(polished=True, **cot)
    et = {k: O.err(tan[k], v) for k, v in Q.tangent(qp, av, ar, d).items() if k in T.OUTS}
    ea = {k: O.err(adj[k], v) for k, v in Q.adjoint(qp, av, ar, cot).items() if k in O.NAMES}
    print("polished sens", cid, "tangent", {k: f"{v:.2e}" for k, v in et.items()}, "adjoint",
          {k: f"{v:.2e}" for k, v in ea.items()})
    assert max(et.values()) <= TANGENT_TOL and max(ea.values()) <= ADJOINT_TOL
    after = s.polished_sens_info()
    assert after["n_tangents"] == before["n_tangents"] + 1 and after["n_adjoints"] == before["n_adjoints"] + 1
    assert after["n_factorizations"] == before["n_factorizations"]          # the call's own factor was still held
    dt = {k: torch.as_tensor(v, device="cuda") for k, v in d.items()}
    _same(s.tangent_device(polished=True, **dt), tan)
    # the interior-point calls belong to the solve before the update: refused with their own texts
    for call in (lambda: s.adjoint(gx), lambda: s.tangent(**d), s.polish, s.polish_device):
        with pytest.raises(MadIPMError, match="since the last solve"):
            call()
    assert s.polish_info()["n_polishes"] == 1                                # polish_info reports the last polish()
    _same(s.active_set_solve(), res)                                         # none of that touched the point or the set
    # the next solve is the twin's update; solve
    t = twin_solver(case)
    assert_same(s.solve(), t.solve())
    # a solve ends the active-set point; polish() on the new end point gives a polished point again
    assert s.polish()["info"]["verdict"] == PolishVerdict.POLISHED
    # another update: the kept set serves, and after one more update no polished point is current
    s.update(**fields(case))
    assert s.active_set_solve(want=["x"])["info"]["verdict"] == PolishVerdict.POLISHED
    s.tangent(polished=True, want=["x"], c=d["c"])
    s.update(c=np.asarray(qp.c, float))
    for call in (lambda: s.tangent(polished=True, **d), lambda: s.adjoint(polished=True, **cot)):
        with pytest.raises(MadIPMError, match="since the last solve"):
            call()


# ------------------------------------------------------------------ 7: the refusals
def test_refusals():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    from madipm_amd import solver as S
    qp = G.problem("family_0")
    s = MPCSolver(qp, **_kw())
    with pytest.raises(MadIPMError, match="madipm_solver_active_set_solve: no set is given and none is kept"):
        s.active_set_solve()
    with pytest.raises(MadIPMError, match="madipm_solver_active_set_solve_device: no set is given and none is kept"):
        s.active_set_solve_device()
    assert s.active_set_info()["verdict"] is None and s.active_set_info()["n_calls"] == 0
    av, ar = P.family_pattern(qp, 0)
    good = s.active_set_solve(active_var=av, active_row=ar)
    assert good["info"]["verdict"] == 0 and good["info"]["rounds"] == 1
    out = L.PolishOut()
    xbuf = np.empty(qp.nvar)
    out.x = L.ptr(xbuf, C.c_double)
    opts = lambda rounds, steps=2, sigma=1e10: C.byref(L.ActiveSetOpts(L.PolishOpts(sigma, 1e-10, 1e-9, 1e-9, steps), rounds))  # noqa: E731
    for fn, tail in ((L.lib.madipm_solver_active_set_solve, ()), (L.lib.madipm_solver_active_set_solve_device, (None,))):
        assert fn(s.h, None, L.ptr(av, C.c_int8), None, C.byref(out), None, *tail) < 0
        assert b"exactly one of active_var and active_row" in L.madipm_last_error()
        assert fn(s.h, None, None, L.ptr(ar, C.c_int8), C.byref(out), None, *tail) < 0
        assert b"exactly one of active_var and active_row" in L.madipm_last_error()
        assert fn(s.h, None, None, None, C.byref(L.PolishOut()), None, *tail) < 0
        assert b"all seven outputs are NULL" in L.madipm_last_error()
        assert fn(s.h, None, None, None, None, None, *tail) < 0
        assert b"null output struct" in L.madipm_last_error()
        for rounds in (0, 17):
            assert fn(s.h, opts(rounds), None, None, C.byref(out), None, *tail) < 0
            assert b"max_rounds must be in 1..16" in L.madipm_last_error()
        assert fn(s.h, opts(4, 9), None, None, C.byref(out), None, *tail) < 0
        assert b"refine_steps must be in 0..8" in L.madipm_last_error()
        assert fn(s.h, opts(4, 2, 0.0), None, None, C.byref(out), None, *tail) < 0
        assert b"sigma must be positive" in L.madipm_last_error()
    assert s.active_set_info() == good["info"]                                # none of them counted or changed anything
    s.tangent(polished=True, want=["x"], c=np.ones(qp.nvar))                  # the polished point is still current
    for var, row, code in ((0, None, 1), (3, None, -1), (None, 0, -1), (None, 2, 1), (4, None, -1), (1, None, 2)):
        bv, br = av.copy(), ar.copy()     # variable 0: no upper bound; 3: fixed; 4: free; row 0: equality; row 2: no upper side
        if var is not None:
            bv[var] = code
        else:
            br[row] = code
        with pytest.raises(MadIPMError, match="madipm_solver_active_set_solve: the supplied set has a code"):
            s.active_set_solve(active_var=bv, active_row=br)
        with pytest.raises(MadIPMError, match="madipm_solver_active_set_solve_device: the supplied set has a code"):
            s.active_set_solve_device(active_var=torch.as_tensor(bv, device="cuda"),
                                      active_row=torch.as_tensor(br, device="cuda"))
    # after all that the kept set still gives the bits of the first call
    G._same(s.active_set_solve(), good)
    lp = G.problem("lp")
    for kkt in (S.ScaledSparseKKTSystem, S.NormalKKTSystem):
        t = MPCSolver(lp, **_kw(kkt_system=kkt))
        with pytest.raises(MadIPMError, match="later release"):
            t.active_set_solve(active_var=np.zeros(lp.nvar, np.int8), active_row=np.zeros(lp.ncon, np.int8))
        assert t.active_set_info()["n_calls"] == 0


def test_refused_on_a_solver_with_a_communicator():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    qp = G.problem("family_0")
    cb = L.ALLREDUCE_FN(lambda p, n, ctx: 0)          # one rank: the sum over the ranks is the buffer itself
    comm = L.vp()
    L.check(L.lib.madipm_comm_create_host(1, 0, cb, None, C.byref(comm)), "comm_create_host")
    s = MPCSolver(qp, **_kw())
    h = L.vp()
    L.check(L.lib.madipm_solver_create_dist(C.byref(s._q), C.byref(s.options), comm, C.byref(h)), "create_dist")
    L.lib.madipm_solver_destroy(s.h)
    s.h = h
    try:
        with pytest.raises(MadIPMError, match="communicator"):
            s.active_set_solve(active_var=np.zeros(qp.nvar, np.int8), active_row=np.zeros(qp.ncon, np.int8))
    finally:
        L.lib.madipm_solver_destroy(s.h)
        s.h = None
        L.lib.madipm_comm_destroy(comm)


# ------------------------------------------------------------------ 8: the torch layer
def test_layer_with_the_active_set_route():
    import torch.autograd.forward_ad as fw
    from madipm_amd import QPLayer
    name = "family_3"
    qp = G.problem(name)
    seq = [qp] + [K.updated(CASES[f"family_3-kept-shifted-{s}-0.1"]) for s in (4, 1, 3)]   # POLISHED in the oracle
    dev = torch.device("cuda")
    keys = ("x", "y", "zl", "zu", "cons")
    gx = np.random.default_rng(4100).uniform(0.5, 1.5, qp.nvar)
    ct = {k: torch.as_tensor(v, device=dev) for k, v in F.cotangents(qp, gx).items()}
    dc = torch.as_tensor(T.directions(qp, 0)["c"], device=dev)
    av, ar = K.base(name)[1]
    rounds = []
    for q in seq[1:]:                          # each forward starts from the set the one before kept
        r = A.active_set_solve(q, av, ar)
        assert r["verdict"] == P.POLISHED and r["margin"] >= K.MARGIN_MIN
        av, ar = r["active_var"], r["active_row"]
        rounds.append(r["rounds"])
    a, b = G.new_solver(name), G.new_solver(name)
    la, lb = QPLayer(a, outputs=keys, polish=True, active_set=True), QPLayer(b, outputs=keys, polish=True)
    assert la.last_route is None
    for k, q in enumerate(seq):
        data = {n: torch.as_tensor(np.asarray(getattr(q, n), float), device=dev) for n in ("c", "lcon", "ucon", "lvar", "uvar")}
        leaf = [{n: t.clone().requires_grad_(True) for n, t in data.items()} for _ in range(2)]
        oa, ob = la(**leaf[0]), lb(**leaf[1])
        assert la.last_route == ("ipm" if k == 0 else "active_set")
        assert k == 0 or a.active_set_info()["rounds"] == rounds[k - 1]
        for x, y, n in zip(oa, ob, keys):
            assert P.err(x.detach().cpu().numpy(), y.detach().cpu().numpy()) <= 2 * EXACT_TOL, n
        sum((o * ct["g" + n]).sum() for o, n in zip(oa, keys)).backward()
        sum((o * ct["g" + n]).sum() for o, n in zip(ob, keys)).backward()
        eg = {n: O.err(leaf[0][n].grad.cpu().numpy(), leaf[1][n].grad.cpu().numpy()) for n in data}
        print("layer", k, la.last_route, "gradients against the plain layer's", {n: f"{v:.2e}" for n, v in eg.items()})
        assert max(eg.values()) <= 2 * ADJOINT_TOL, eg       # both sides are within ADJOINT_TOL of the same derivative
    assert a.active_set_info()["n_calls"] == 3 and a.polish_info()["n_polishes"] == 1
    assert b.active_set_info()["n_calls"] == 0 and b.polish_info()["n_polishes"] == 4
    with fw.dual_level():
        ja = la(c=fw.make_dual(data["c"], dc))
        jb = lb(c=fw.make_dual(data["c"], dc))
        assert la.last_route == "active_set"
        for x, y, n in zip(ja, jb, keys):
            ta, tb = fw.unpack_dual(x).tangent, fw.unpack_dual(y).tangent
            print("layer jvp", n, f"{O.err(ta.cpu().numpy(), tb.cpu().numpy()):.2e}")
            assert O.err(ta.cpu().numpy(), tb.cpu().numpy()) <= 2 * TANGENT_TOL, n
