"""MPCSolver.tangent / adjoint with polished=True, polished_sens_info and QPLayer(polish=True) on the GPU
against the CPU oracle (polished_sens_oracle.py): the derivatives of the polished point against the
dense derivative of the face on the returned set, the transpose identity between the two calls, the exact
properties (copies and zeros, bitwise), the gain over the interior-point sensitivities, the routes, the
factor's tags and the solver's state, the refusals and the torch layer.  Fixtures, solver options and the
polish are test_polish_gpu.py's; directions and cotangents are tangent_oracle's and adjoint_full_oracle's."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import adjoint_full_oracle as F  # noqa: E402
import adjoint_oracle as O  # noqa: E402
import polish_oracle as P  # noqa: E402
import polished_sens_oracle as Q  # noqa: E402
import tangent_oracle as T  # noqa: E402
import test_polish_gpu as G  # noqa: E402
from test_adjoint_gpu import _kw  # noqa: E402
from test_polished_sens_cpu import GPU_FIXTURES as CPU_CHECKED  # noqa: E402
from test_update_gpu import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

# Largest figures measured on the MI355X over all fixtures and selections; each bound is 10 x the
# largest, under its cap.  err = max |gpu - oracle| / max(1, max |oracle|) per block, the oracle's dense
# derivative on the returned set.
# tangent (all seven directions and each alone), largest block by fixture: the 7 x 5 family seeds 0-3 4.8e-16 /
# 1.2e-15 / 5.4e-16 / 2.0e-15, maximise 4.8e-16, duplicated 2.1e-15, scaled 1.2e-13 (cons with lvar alone: entries
# of 1e3), the LP 3.8e-15, the sparse QP at G = 64 5.1e-16, the row-length fixture at G = 4 4.7e-16, no bounds
# 2.3e-15, no rows 8.7e-16.
TANGENT_MEASURED = 1.24e-13
# adjoint (all five cotangents and each alone): the family 4.9e-16 / 1.4e-15 (lcon with gy alone) / 5.0e-16 / 8.8e-16,
# maximise 4.9e-16, duplicated 6.5e-16, scaled 7.5e-16, the LP 5.1e-16, the sparse QP 8.6e-16, the row-length
# fixture 7.8e-16, no bounds 3.3e-16, no rows 4.0e-16.
ADJOINT_MEASURED = 1.36e-15
# |<cot, tangent(d)> - <adjoint(cot), d>| / max(1, |<cot, tangent(d)>|): 1.1e-14 on the LP (W = 0: the reduced matrix is
# [0 J'; J 0]), <= 1.5e-15 on the others (the sparse QP: 1.5e-15)
TRANSPOSE_MEASURED = 1.09e-14
# last_residual, the max-norm of the final masked residual in the scaled space: 9.1e-13 on the scaled family
# (entries of 1e3), <= 7.6e-15 on the others
RESIDUAL_MEASURED = 9.09e-13
# the interior-point tangent() of the same solver and point against the same oracle: 2.3e-10 ... 1.2e-7 (row-length
# fixture; scaled 9.5e-8, family seed 1 4.9e-9, the sparse QP 1.4e-9), the polished one 1.8e-16 ... 2.6e-14
TANGENT_TOL, ADJOINT_TOL = 10.0 * TANGENT_MEASURED, 10.0 * ADJOINT_MEASURED
TRANSPOSE_TOL, RESIDUAL_TOL = 10.0 * TRANSPOSE_MEASURED, 10.0 * RESIDUAL_MEASURED
ACCURACY_CAP = 1e-10           # test_polish_gpu.EXACT_CAP: the derivative is solved to the same masked-residual level
TRANSPOSE_CAP = 1e-12

FIXTURES = G.FIXTURES
D_SELECTIONS = ("all",) + T.NAMES
C_SELECTIONS = ("all",) + F.COTS
_cache = {}


def _inputs(name):
    qp = G.problem(name)
    gx = np.random.default_rng(4100).uniform(0.5, 1.5, qp.nvar) * np.random.default_rng(4101).choice([-1.0, 1.0], qp.nvar)
    return T.directions(qp, 0), F.cotangents(qp, gx)


def _dsel(d, sel):
    return dict(d) if sel == "all" else T.only(d, sel)


def _csel(cot, sel):
    return dict(cot) if sel == "all" else F.only(cot, sel)


def _tensors(v):
    return {k: torch.as_tensor(a, device="cuda") for k, a in v.items()}


def case(name):
    """The fixture solved and polished on the GPU once, then the host route's polished tangents and gradients
    for every selection (all first: the calls whose residuals are kept), and last the interior-point tangent of
    the same point: computed once, never modified."""
    if name not in _cache:
        from madipm_amd import PolishVerdict
        qp = G.problem(name)
        d, cot = _inputs(name)
        s = G.new_solver(name)
        st = s.solve()
        assert st.status == 1, (name, st.status_name)
        pol = s.polish()
        assert pol["info"]["verdict"] == PolishVerdict.POLISHED, pol["info"]
        t, g, res = {}, {}, {}
        for sel in D_SELECTIONS:
            t[sel] = s.tangent(polished=True, **_dsel(d, sel))
            res["t_" + sel] = s.polished_sens_info()["last_residual"]
        for sel in C_SELECTIONS:
            g[sel] = s.adjoint(polished=True, **_csel(cot, sel))
            res["g_" + sel] = s.polished_sens_info()["last_residual"]
        info = s.polished_sens_info()
        ipm = s.tangent(**d)              # takes the LDL^T: the next polished call restores the polish's factor
        _cache[name] = dict(qp=qp, solver=s, stats=st, pol=pol, d=d, cot=cot, t=t, g=g, res=res, info=info, ipm=ipm)
    return _cache[name]


def _set(c):
    return c["pol"]["active_var"], c["pol"]["active_row"]


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _cache.clear()          # the solvers go while the library is still loaded


def test_tolerances_fit_the_caps():
    assert TANGENT_TOL <= ACCURACY_CAP and ADJOINT_TOL <= ACCURACY_CAP and RESIDUAL_TOL <= ACCURACY_CAP
    assert TRANSPOSE_TOL <= TRANSPOSE_CAP
    # every fixture's restated algorithm meets the dense derivative within 1e-11 on the CPU (test_polished_sens_cpu.py)
    assert set(CPU_CHECKED) == set(FIXTURES)


# ------------------------------------------------------------------ 1-3: against the oracle
@pytest.mark.parametrize("sel", D_SELECTIONS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_tangent_against_the_oracle(name, sel):
    c = case(name)
    ref = Q.tangent(c["qp"], *_set(c), _dsel(c["d"], sel))
    e = {k: O.err(c["t"][sel][k], ref[k]) for k in T.OUTS}
    print("tangent", name, sel, {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= TANGENT_TOL, e


@pytest.mark.parametrize("sel", C_SELECTIONS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_adjoint_against_the_oracle(name, sel):
    c = case(name)
    ref = Q.adjoint(c["qp"], *_set(c), _csel(c["cot"], sel))
    e = {k: O.err(c["g"][sel][k], ref[k]) for k in O.NAMES}
    print("adjoint", name, sel, {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= ADJOINT_TOL, e


@pytest.mark.parametrize("name", list(FIXTURES))
def test_transpose_identity(name):
    c = case(name)
    a, b = T.dot(c["cot"], c["t"]["all"]), T.dot_data(c["g"]["all"], c["qp"], c["d"])
    worst = abs(a - b) / max(1.0, abs(a))
    if name == "family_3":        # and each cotangent alone against each direction block alone
        for cs in F.COTS:
            for k in T.NAMES:
                a, b = T.dot(F.only(c["cot"], cs), c["t"][k]), T.dot_data(c["g"][cs], c["qp"], T.only(c["d"], k))
                worst = max(worst, abs(a - b) / max(1.0, abs(a)))
    print("transpose", name, f"{worst:.2e}")
    assert worst <= TRANSPOSE_TOL


@pytest.mark.parametrize("name", list(FIXTURES))
def test_residual_and_counters(name):
    c = case(name)
    print("residual", name, f"{max(c['res'].values()):.2e}")
    assert all(np.isfinite(r) and r <= RESIDUAL_TOL for r in c["res"].values()), c["res"]
    assert c["info"]["n_tangents"] == len(D_SELECTIONS) and c["info"]["n_adjoints"] == len(C_SELECTIONS)
    assert c["info"]["n_factorizations"] == 0         # the polish's factor was still in the LDL^T


# ------------------------------------------------------------------ 4: exact properties, bitwise
@pytest.mark.parametrize("name", list(FIXTURES))
def test_exact_properties(name):
    c = case(name)
    qp, d, s = c["qp"], c["d"], c["solver"]
    av, ar = _set(c)
    fixed = qp.lvar == qp.uvar
    for sel in D_SELECTIONS:
        t, ds = c["t"][sel], _dsel(d, sel)
        z = lambda k: ds.get(k, np.zeros_like(d[k]))  # noqa: E731
        assert np.array_equal(t["x"][av < 0], z("lvar")[av < 0]) and np.array_equal(t["x"][av > 0], z("uvar")[av > 0])
        assert np.array_equal(t["x"][fixed], z("lvar")[fixed])
        assert np.array_equal(t["cons"][ar < 0], z("lcon")[ar < 0]) and np.array_equal(t["cons"][ar > 0], z("ucon")[ar > 0])
        assert np.all(t["zl"][av >= 0] == 0.0) and np.all(t["zu"][av <= 0] == 0.0)
    for sel in C_SELECTIONS:
        g = c["g"][sel]
        assert np.all(g["lvar"][(av >= 0) & ~fixed] == 0.0) and np.all(g["uvar"][av <= 0] == 0.0)
        eq = qp.lcon == qp.ucon
        assert np.all(g["lcon"][(ar >= 0) & ~eq] == 0.0) and np.all(g["ucon"][ar <= 0] == 0.0)
    if name == "family_3":
        assert fixed.any() and np.any(av < 0) and np.any(ar != 0) and np.any(np.abs(c["t"]["all"]["zl"][av < 0]) > 1e-3)
    # NaN in the entries that are not read changes no bit; nor does it on the bounds of inactive coordinates
    dn = T.with_nan(qp, d)
    dn["lvar"][(av >= 0) & ~fixed], dn["uvar"][av <= 0] = np.nan, np.nan
    dn["lcon"][(ar >= 0) & (qp.lcon != qp.ucon)], dn["ucon"][ar <= 0] = np.nan, np.nan
    h, dv = s.tangent(polished=True, **dn), s.tangent_device(polished=True, **_tensors(dn))
    for k in T.OUTS:
        assert np.array_equal(h[k], c["t"]["all"][k]) and np.array_equal(dv[k].cpu().numpy(), c["t"]["all"][k]), k
    # the cotangents of constant multipliers are not read either
    cn = dict(c["cot"], gzl=np.where(av < 0, c["cot"]["gzl"], np.nan), gzu=np.where(av > 0, c["cot"]["gzu"], np.nan))
    gn = s.adjoint(polished=True, **cn)
    for k in O.NAMES:
        assert np.array_equal(gn[k], c["g"]["all"][k]), k


# ------------------------------------------------------------------ 5: the gain over the interior-point tangent
@pytest.mark.parametrize("name", list(FIXTURES))
def test_improvement_over_the_interior_point_tangent(name):
    c = case(name)
    ref = Q.tangent(c["qp"], *_set(c), c["d"])
    e_ipm, e_pol = T.max_err(c["ipm"], ref), T.max_err(c["t"]["all"], ref)
    print("gain", name, f"tangent() {e_ipm:.2e} polished {e_pol:.2e}")
    if e_ipm >= 1e-9:         # below it tangent() is exempt, as §13f exempts the scaled family
        assert e_pol <= 1e-2 * e_ipm
    if name in ("family_scaled", "rowlength_g4"):
        assert e_ipm >= 1e-9, "the gain is not shown on the fixtures it was measured on"


# ------------------------------------------------------------------ 6: routes and state
@pytest.mark.parametrize("name", ["family_0", "family_3", "family_scaled", "lp", "sparse_g64", "rowlength_g4",
                                  "no_bounds", "no_rows"])
def test_routes_give_identical_bits(name):
    c = case(name)
    s, d, cot, t, g = c["solver"], c["d"], c["cot"], c["t"]["all"], c["g"]["all"]
    again, dev = s.tangent(polished=True, **d), s.tangent_device(polished=True, **_tensors(d))
    gagain, gdev = s.adjoint(polished=True, **cot), s.adjoint_device(polished=True, **_tensors(cot))
    torch.cuda.synchronize()
    for k in T.OUTS:
        assert np.array_equal(again[k], t[k]) and np.array_equal(dev[k].cpu().numpy(), t[k]), k
    for k in O.NAMES:
        assert np.array_equal(gagain[k], g[k]) and np.array_equal(gdev[k].cpu().numpy(), g[k]), k
    for want in (["x"], ["zl", "zu"], ["cons"], ["cons", "y"]):
        sub, subd = s.tangent(want=want, polished=True, **d), s.tangent_device(want=want, polished=True, **_tensors(d))
        assert sorted(sub) == sorted(want)
        for k in want:
            assert np.array_equal(sub[k], t[k]) and np.array_equal(subd[k].cpu().numpy(), t[k]), (want, k)
    for want in (["c"], ["lvar", "uvar"], ["Avals", "lcon"], ["Hvals", "ucon"]):
        sub, subd = s.adjoint(want=want, polished=True, **cot), s.adjoint_device(want=want, polished=True, **_tensors(cot))
        assert sorted(sub) == sorted(want)
        for k in want:
            assert np.array_equal(sub[k], g[k]) and np.array_equal(subd[k].cpu().numpy(), g[k]), (want, k)
    # an absent block is that block given as zeros
    for sel in ("c", "lvar"):
        z = {k: (v if k == sel else np.zeros_like(v)) for k, v in d.items()}
        h = s.tangent(polished=True, **z)
        for k in T.OUTS:
            assert np.array_equal(h[k], c["t"][sel][k]), (sel, k)


def test_device_route_honours_the_stream():
    c = case("family_0")
    s = c["solver"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d = {k: v * 1.0 for k, v in _tensors(c["d"]).items()}        # produced on the side stream
        out = s.tangent_device(stream=side, polished=True, **d)
        ct = {k: v * 1.0 for k, v in _tensors(c["cot"]).items()}
        gout = s.adjoint_device(stream=side, polished=True, **ct)
        doubled = {k: 2.0 * v for k, v in out.items()}               # consumed on it, without a host wait
        gdoubled = {k: 2.0 * v for k, v in gout.items()}
    side.synchronize()
    for k in T.OUTS:
        assert np.array_equal(doubled[k].cpu().numpy(), 2.0 * c["t"]["all"][k]), k
    for k in O.NAMES:
        assert np.array_equal(gdoubled[k].cpu().numpy(), 2.0 * c["g"]["all"][k]), k


@pytest.mark.parametrize("name", ["family_0", "family_scaled", "sparse_g64"])
def test_factor_tags_and_the_next_solve(name):
    c = case(name)
    d, cot = c["d"], c["cot"]
    a = G.new_solver(name)
    first = a.solve()
    a.polish()
    t1, g1 = a.tangent(polished=True, **d), a.adjoint(polished=True, **cot)
    assert a.polished_sens_info()["n_factorizations"] == 0 and a.polish_info()["n_polish_factorizations"] == 1
    ga = a.adjoint(**cot)                 # takes the LDL^T
    assert a.adjoint_info()["n_adjoint_factorizations"] == 1
    t2 = a.tangent(polished=True, **d)    # restores the polish's factor, once
    g2 = a.adjoint(polished=True, **cot)
    assert a.polished_sens_info()["n_factorizations"] == 1
    ga2 = a.adjoint(**cot)                # and the adjoint factorises again
    assert a.adjoint_info()["n_adjoint_factorizations"] == 2
    again = a.polish()                    # the polish finds its factor gone, too
    assert again["info"]["n_polish_factorizations"] == 2
    for k in T.OUTS:
        assert np.array_equal(t1[k], c["t"]["all"][k]) and np.array_equal(t2[k], t1[k]), k
        assert np.array_equal(again[k], c["pol"][k]), k
    for k in O.NAMES:
        assert np.array_equal(g1[k], c["g"]["all"][k]) and np.array_equal(g2[k], g1[k]), k
    second = a.solve()
    # against a solver that never polished: solve(); adjoint(); solve()
    b = G.new_solver(name)
    assert_same(first, b.solve())
    gb = b.adjoint(**cot)
    assert_same(second, b.solve())
    for k in O.NAMES:
        assert np.array_equal(ga[k], gb[k]) and np.array_equal(ga2[k], gb[k]), k
    assert b.polished_sens_info() == {"n_tangents": 0, "n_adjoints": 0, "n_factorizations": 0, "last_residual": 0.0}


# ------------------------------------------------------------------ 7: the refusals
def test_refusals():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError, PolishVerdict
    from madipm_amd import _lib as L
    qp = G.problem("family_0")
    d, cot = _inputs("family_0")
    some, csome = T.only(d, "c", "lcon"), F.only(cot, "gx", "gy")
    s = MPCSolver(qp, **_kw())
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_polished: no solve has run"):
        s.tangent(polished=True, **some)
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_polished_device: no solve has run"):
        s.adjoint_device(polished=True, **_tensors(csome))
    assert s.solve().status == 1
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_polished_device: no polish has run on the point"):
        s.tangent_device(polished=True, **_tensors(some))
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_polished: no polish has run on the point"):
        s.adjoint(polished=True, **csome)
    good = s.polish()
    t0, g0 = s.tangent(polished=True, **some), s.adjoint(polished=True, **csome)
    # the last polish's verdict: §13f's supplied set with variable 1's inactive upper bound
    forced = (good["active_var"].copy(), good["active_row"].copy())
    forced[0][1] = 1
    assert s.polish(active_var=forced[0], active_row=forced[1])["info"]["verdict"] == PolishVerdict.WRONG_SET
    with pytest.raises(MadIPMError, match="the last polish ended with verdict WRONG_SET, not POLISHED"):
        s.tangent(polished=True, **some)
    with pytest.raises(MadIPMError, match="the last polish ended with verdict WRONG_SET, not POLISHED"):
        s.adjoint_device(polished=True, **_tensors(csome))
    # a polish that was refused half-way (a code on a bound that does not exist) leaves no polished point
    s.polish()
    bad = good["active_var"].copy()
    bad[0] = 1
    with pytest.raises(MadIPMError, match="the supplied set has a code"):
        s.polish(active_var=bad, active_row=good["active_row"])
    with pytest.raises(MadIPMError, match="no polish has run on the point"):
        s.tangent(polished=True, **some)
    s.polish()
    # an update since the solve; a new solve without a polish
    s.update(c=qp.c * 1.01)
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.tangent(polished=True, **some)
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.adjoint(polished=True, **csome)
    s.update(c=qp.c)
    assert s.solve().status == 1
    with pytest.raises(MadIPMError, match="no polish has run on the point"):
        s.adjoint(polished=True, **csome)
    s.polish()
    # all inputs or all outputs absent, null structs: at the C interface
    o, gr = L.QPTan(), L.QPGrad()
    buf = np.empty(qp.nvar)
    o.x = gr.c = L.ptr(buf, C.c_double)
    dr, ct = L.QPDir(c=L.ptr(d["c"], C.c_double)), L.QPCot(x=L.ptr(cot["gx"], C.c_double))
    for fn, tail in ((L.lib.madipm_solver_tangent_polished, ()), (L.lib.madipm_solver_tangent_polished_device, (None,))):
        assert fn(s.h, C.byref(L.QPDir()), C.byref(o), *tail) < 0
        assert b"all seven directions are NULL" in L.madipm_last_error()
        assert fn(s.h, C.byref(dr), C.byref(L.QPTan()), *tail) < 0
        assert b"all five outputs are NULL" in L.madipm_last_error()
        assert fn(s.h, None, C.byref(o), *tail) < 0 and b"null direction struct" in L.madipm_last_error()
        assert fn(s.h, C.byref(dr), None, *tail) < 0 and b"null output struct" in L.madipm_last_error()
    for fn, tail in ((L.lib.madipm_solver_adjoint_polished, ()), (L.lib.madipm_solver_adjoint_polished_device, (None,))):
        assert fn(s.h, C.byref(L.QPCot()), C.byref(gr), *tail) < 0
        assert b"all five cotangents are NULL" in L.madipm_last_error()
        assert fn(s.h, C.byref(ct), C.byref(L.QPGrad()), *tail) < 0
        assert b"all seven outputs are NULL" in L.madipm_last_error()
        assert fn(s.h, None, C.byref(gr), *tail) < 0 and b"null cotangent struct" in L.madipm_last_error()
        assert fn(s.h, C.byref(ct), None, *tail) < 0 and b"null output struct" in L.madipm_last_error()
    # Hvals / Avals, and lvar with a fixed variable, without prepare_update, on a fresh solver
    f = MPCSolver(qp, **_kw())
    assert f.solve().status == 1
    f.polish()
    for field in ("Hvals", "Avals", "lvar"):
        dd = L.QPDir(**{field: L.ptr(d[field], C.c_double)})
        assert L.lib.madipm_solver_tangent_polished(f.h, C.byref(dd), C.byref(o)) < 0, field
        assert b"madipm_solver_prepare_update first" in L.madipm_last_error(), field
        gg = L.QPGrad(**{field: L.ptr(np.empty(d[field].size), C.c_double)})
        assert L.lib.madipm_solver_adjoint_polished(f.h, C.byref(ct), C.byref(gg)) < 0, field
        assert b"madipm_solver_prepare_update first" in L.madipm_last_error(), field
    assert L.lib.madipm_solver_tangent_polished(f.h, C.byref(dr), C.byref(o)) == 0       # c needs nothing
    assert f.polished_sens_info()["n_tangents"] == 1
    # the python checks are those of the plain calls, before any library call
    n0 = s.polished_sens_info()
    with pytest.raises(ValueError, match="no direction given"):
        s.tangent(polished=True)
    with pytest.raises(ValueError, match="unknown name"):
        s.tangent(want=["s"], polished=True, **some)
    with pytest.raises(ValueError, match="c has shape"):
        s.tangent_device(polished=True, c=_tensors(some)["c"][:-1])
    with pytest.raises(TypeError, match="torch.cuda.Stream"):
        s.adjoint_device(stream=0, polished=True, **_tensors(csome))
    assert s.polished_sens_info() == n0
    # after all that a successful call still works, with the bits of the first
    t1, g1 = s.tangent(polished=True, **some), s.adjoint(polished=True, **csome)
    for k in T.OUTS:
        assert np.array_equal(t1[k], t0[k]), k
    for k in O.NAMES:
        assert np.array_equal(g1[k], g0[k]), k


# ------------------------------------------------------------------ 8: the torch layer
def test_layer_with_polish():
    import torch.autograd.forward_ad as fw
    from madipm_amd import QPLayer
    name = "family_3"
    c = case(name)
    qp, d, cot = c["qp"], c["d"], c["cot"]
    dev = torch.device("cuda")
    data = {k: torch.as_tensor(np.asarray(getattr(qp, k), float), device=dev) for k in O.NAMES}
    dt, ct = _tensors(d), _tensors(cot)
    s = G.new_solver(name)
    keys = ("x", "y", "zl", "zu", "cons")
    av, ar = _set(c)
    # reverse mode: all seven data tensors, all five outputs
    leaf = {k: data[k].clone().requires_grad_(True) for k in O.NAMES}
    out = QPLayer(s, outputs=keys, polish=True)(**leaf)
    pol = s.polish_device()
    assert np.array_equal(pol["active_var"].cpu().numpy(), av) and np.array_equal(pol["active_row"].cpu().numpy(), ar)
    for o, k in zip(out, keys):
        assert torch.equal(o.detach(), pol[k]), k
    sum((o * ct["g" + k]).sum() for o, k in zip(out, keys)).backward()
    direct = s.adjoint_device(polished=True, **ct)
    ref = Q.adjoint(qp, av, ar, cot)
    for k in O.NAMES:
        assert torch.equal(leaf[k].grad, direct[k]), k
        assert O.err(leaf[k].grad.cpu().numpy(), ref[k]) <= ADJOINT_TOL, k
    # forward mode
    ref = Q.tangent(qp, av, ar, d)
    with fw.dual_level():
        out = QPLayer(s, outputs=keys, polish=True)(**{k: fw.make_dual(data[k], dt[k]) for k in O.NAMES})
        direct = s.tangent_device(polished=True, **dt)
        for o, k in zip(out, keys):
            p, t = fw.unpack_dual(o)
            assert torch.equal(p, pol[k]) and torch.equal(t, direct[k]), k
            assert O.err(t.cpu().numpy(), ref[k]) <= TANGENT_TOL, k
        x = QPLayer(s, polish=True)(c=fw.make_dual(data["c"], dt["c"]))
        p, t = fw.unpack_dual(x)
        assert isinstance(x, torch.Tensor) and torch.equal(p, pol["x"])
        assert torch.equal(t, s.tangent_device(want=["x"], polished=True, c=dt["c"])["x"])
    # the default layer with polish: x alone, gx alone
    lc = data["c"].clone().requires_grad_(True)
    x = QPLayer(s, polish=True)(c=lc)
    (x * ct["gx"]).sum().backward()
    assert torch.equal(lc.grad, s.adjoint_device(ct["gx"], want=["c"], polished=True)["c"])
    assert O.err(lc.grad.cpu().numpy(), Q.adjoint(qp, av, ar, F.only(cot, "gx"))["c"]) <= ADJOINT_TOL
    assert s.adjoint_info()["n_adjoints"] == 0 and s.tangent_info()["n_tangents"] == 0


def test_layer_raises_on_a_face_without_a_polished_point():
    from madipm_amd import MadIPMError, MPCSolver, QPLayer

    class Degenerate(MPCSolver):          # §13f's LP case: a fourth variable at a bound under three equality rows
        def polish_device(self, want=None, stream=None, **kw):
            av, ar = P.lp_pattern(G.problem("lp"))
            av[3] = -1
            return super().polish_device(want, stream, active_var=torch.as_tensor(av, device="cuda"),
                                         active_row=torch.as_tensor(ar, device="cuda"), **kw)

    s = Degenerate(G.problem("lp"), **_kw())
    c = torch.as_tensor(np.asarray(G.problem("lp").c, float), device="cuda")
    with pytest.raises(MadIPMError, match="QPLayer: the polish ended with verdict (NO_CONVERGENCE|WRONG_SET), not POLISHED"):
        QPLayer(s, polish=True)(c=c)


def test_layer_without_polish_is_unchanged():
    from madipm_amd import QPLayer
    name = "family_1"
    qp = G.problem(name)
    _, cot = _inputs(name)
    dev = torch.device("cuda")
    data = {k: torch.as_tensor(np.asarray(getattr(qp, k), float), device=dev) for k in O.NAMES}
    ct = _tensors(cot)
    keys = ("x", "y", "cons")
    res = []
    for layer in (lambda s: QPLayer(s, outputs=keys), lambda s: QPLayer(s, outputs=keys, polish=False)):
        s = G.new_solver(name)
        leaf = {k: data[k].clone().requires_grad_(True) for k in ("c", "lvar", "Avals")}
        out = layer(s)(**leaf)
        sum((o * ct["g" + k]).sum() for o, k in zip(out, keys)).backward()
        ref = s.adjoint_device(ct["gx"], want=list(leaf), gy=ct["gy"], gcons=ct["gcons"])
        sol = s.solution_device()
        for o, k in zip(out, ("solution", "multipliers", "constraints")):
            assert torch.equal(o.detach(), sol[k]), k
        for k in leaf:
            assert torch.equal(leaf[k].grad, ref[k]), k
        assert s.polish_info()["n_polishes"] == 0 and s.polished_sens_info()["n_adjoints"] == 0
        res.append([o.detach().cpu().numpy() for o in out] + [leaf[k].grad.cpu().numpy() for k in leaf])
    for a, b in zip(*res):
        assert np.array_equal(a, b)
