"""MPCSolver.adjoint / adjoint_device / QPLayer with the cotangents of all five solution blocks
on the GPU against the CPU oracle (adjoint_full_oracle.py): the loss is l(x, y, zl, zu, A x).

Two comparisons per fixture and per selection of cotangents (all five, and each alone), both with
err = max |g_gpu - g_ref| / max(1, max |g_ref|) per block:
  formula  the oracle's shifted formulas evaluated at the point the GPU solve returned: what the kernels compute
  truth    the oracle's gradients at its own optimum (mu = 1e-11): what the caller wants
and the routes (gx alone is adjoint(gx); host / device / repeated / subsets give the same bits), the solver's
state, the residual, the refusals and the torch layer."""
from __future__ import annotations

import contextlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import adjoint_full_oracle as F  # noqa: E402
import adjoint_oracle as O  # noqa: E402
from test_adjoint_gpu import TOL_LINEAR_SOLVE, _kw  # noqa: E402
from test_update_gpu import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

# Largest err measured on the MI355X over all fixtures and selections; each bound is 10 x it
# (floor 1e-9), and neither may exceed 1e-4: every cotangent's contribution to every block is >= 1e-2 of the
# block on some fixture (test_adjoint_full_cpu.py).  By fixture, formula / truth: the 7 x 5 family (min, max,
# duplicated) 6.9e-10 / 6.3e-8, scaled 4.1e-10 / 3.2e-9, seed 3 1.4e-10 / 5.3e-9, the LP 2.6e-10 / 3.7e-9, the
# sparse QP (1 and 2 shards, G = 64) 1.6e-10 / 2.0e-8, the row-length fixture at G = 4 1.1e-10 / 8.1e-7.
# The plain form's lvar / uvar at the same returned points (oracle, plain against shifted) is off by 3.0e-7
# (family) ... 1.2e-5 (LP) ... 3.4e-4 (sparse QP): what the shift stays below by three to six orders.
# last_residual: <= 1.7e-14 everywhere.
FORMULA_MEASURED = 6.9e-10     # ucon of the 7 x 5 family with gx alone; with all five cotangents 5.1e-10 (c, Hvals)
TRUTH_MEASURED = 8.1e-7        # c of the row-length fixture with gzl alone (the end point's mu); the family 6.3e-8
FORMULA_TOL = max(1e-9, 10.0 * FORMULA_MEASURED)
TRUTH_TOL = max(1e-9, 10.0 * TRUTH_MEASURED)
CAP = 1e-4

# name -> (problem, solver options, MADIPM_SPMV_G during construction or None)
FIXTURES = {
    "family_min": (lambda: O.family(1), {}, None),
    "family_max": (lambda: O.family(1, minimize=False), {}, None),
    "family_scaled": (lambda: O.scaled_family(1), {}, None),
    "family_dup": (lambda: O.duplicated_family(1)[:2], {}, None),
    "family_seed3": (lambda: O.family(3), {}, None),
    "lp": (O.lp_fixture, {}, None),
    "sparse": (O.sparse_fixture, {}, None),
    "sparse_2shards": (O.sparse_fixture, {"nshards": 2}, None),
    "rowlength_g4": (F.rowlength_fixture, {}, 4),
    "sparse_g64": (O.sparse_fixture, {}, 64),
}
SELECTIONS = ("all",) + F.COTS
_cache, _refs, _truth = {}, {}, {}


@contextlib.contextmanager
def spmv_width(G):
    """MADIPM_SPMV_G = G (None: unset) while a solver is constructed: the variable is read once, there."""
    old = os.environ.pop("MADIPM_SPMV_G", None)
    if G is not None:
        os.environ["MADIPM_SPMV_G"] = str(G)
    try:
        yield
    finally:
        os.environ.pop("MADIPM_SPMV_G", None)
        if old is not None:
            os.environ["MADIPM_SPMV_G"] = old


def _reference(make):
    """(qp, cotangents, reference point): computed once per problem, never modified."""
    if make not in _refs:
        qp, gx = make()
        _refs[make] = (qp, F.cotangents(qp, gx), O.reference_ipm(qp))
    return _refs[make]


def _select(cot, sel):
    return dict(cot) if sel == "all" else F.only(cot, sel)


def _call(cot):
    """The oracle's cotangent dict as adjoint()'s arguments: its keys are the keywords."""
    return dict(cot)


def _truth_of(make, sel):
    if (make, sel) not in _truth:
        qp, cot, pt = _reference(make)
        _truth[(make, sel)] = F.reference_adjoint_full(qp, pt, _select(cot, sel))
    return _truth[(make, sel)]


def new_solver(name):
    from madipm_amd import MPCSolver
    make, extra, G = FIXTURES[name]
    with spmv_width(G):
        s = MPCSolver(_reference(make)[0], **_kw(**extra))
    if G is not None:
        assert s.spmv_group() == G
    return s


def case(name):
    """The fixture solved on the GPU once: solver, stats, and the host route's gradients of all seven blocks for
    every selection of cotangents (all five first: the call whose counters and residual are kept)."""
    if name not in _cache:
        make = FIXTURES[name][0]
        qp, cot, pt = _reference(make)
        s = new_solver(name)
        st = s.solve()
        assert st.status == 1, (name, st.status_name)
        g = {"all": s.adjoint(**_call(cot))}
        info = s.adjoint_info()
        res = {"all": info["last_residual"]}
        for sel in F.COTS:
            g[sel] = s.adjoint(**_call(_select(cot, sel)))
            res[sel] = s.adjoint_info()["last_residual"]
        _cache[name] = dict(qp=qp, cot=cot, pt=pt, make=make, solver=s, stats=st, g=g, info=info, res=res)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _cache.clear()          # the solvers go while the library is still loaded


def _errs(g, ref):
    return {k: O.err(g[k], ref[k]) for k in O.NAMES}


def _tensors(cot):
    return {k: torch.as_tensor(v, device="cuda") for k, v in cot.items()}


def test_tolerances_fit_the_condition():
    assert FORMULA_TOL <= CAP and TRUTH_TOL <= CAP


# ------------------------------------------------------------------ formula and truth
@pytest.mark.parametrize("sel", SELECTIONS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_formula_at_the_returned_point(name, sel):
    c = case(name)
    st = c["stats"]
    point = {"x": st.solution, "y": st.multipliers, "zl": st.multipliers_L, "zu": st.multipliers_U}
    cot = _select(c["cot"], sel)
    e = _errs(c["g"][sel], F.reference_adjoint_full(c["qp"], point, cot, "shifted"))
    # what the plain form would have cost in the bound gradients at this point (not asserted: for the record)
    p = _errs(F.reference_adjoint_full(c["qp"], point, cot, "plain"),
              F.reference_adjoint_full(c["qp"], point, cot, "shifted"))
    print("formula", name, sel, {k: f"{v:.2e}" for k, v in e.items()}, "plain-shifted lvar/uvar",
          f"{p['lvar']:.1e}/{p['uvar']:.1e}")
    assert max(e.values()) <= FORMULA_TOL, e


@pytest.mark.parametrize("sel", SELECTIONS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_truth_at_the_reference_optimum(name, sel):
    c = case(name)
    assert O.err(c["stats"].solution, c["pt"]["x"]) <= 1e-6        # the same optimum
    e = _errs(c["g"][sel], _truth_of(c["make"], sel))
    print("truth", name, sel, {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= TRUTH_TOL, e


def test_constant_multipliers_are_zero_and_their_cotangents_ignored():
    """zl / zu of a variable without that bound and of a fixed variable come back as 0, and whatever stands in
    their cotangents changes no bit."""
    c = case("family_seed3")
    qp, s, st = c["qp"], c["solver"], c["stats"]
    fixed = qp.lvar == qp.uvar
    nol, nou = ~np.isfinite(qp.lvar) | fixed, ~np.isfinite(qp.uvar) | fixed
    assert fixed.any() and not np.any(st.multipliers_L[nol]) and not np.any(st.multipliers_U[nou])
    other = dict(c["cot"], gzl=np.where(nol, 7.0, c["cot"]["gzl"]), gzu=np.where(nou, -7.0, c["cot"]["gzu"]))
    g = s.adjoint(**_call(other))
    for k in O.NAMES:
        assert np.array_equal(g[k], c["g"]["all"][k]), k
    sp = case("sparse")
    fx = sp["qp"].lvar == sp["qp"].uvar
    assert fx.sum() == 20 and not np.any(sp["stats"].multipliers_L[fx]) and not np.any(sp["stats"].multipliers_U[fx])


def test_fixtures_do_what_they_are_for():
    assert not case("family_max")["qp"].minimize
    assert case("rowlength_g4")["solver"].spmv_group() == 4 and case("sparse_g64")["solver"].spmv_group() == 64
    assert case("lp")["g"]["all"]["Hvals"].shape == (0,)
    # the duplicated entries receive the full gradient of their entry, the direct term of Avals included
    qp, _, hk, ak = O.duplicated_family(1)
    g = case("family_dup")["g"]["gcons"]
    nh, na = qp.nnzh - len(hk), qp.nnzj - len(ak)
    assert np.array_equal(g["Hvals"][nh:], g["Hvals"][hk]) and np.array_equal(g["Avals"][na:], g["Avals"][ak])
    assert np.max(np.abs(g["Avals"][ak])) > 1e-3


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("name", ["family_min", "family_scaled", "lp", "sparse", "sparse_2shards", "rowlength_g4"])
def test_gx_alone_is_the_adjoint_of_x(name):
    """The C entry points themselves with x alone in the struct, against madipm_solver_adjoint(gx)."""
    import ctypes as C
    from madipm_amd import _lib as L
    c = case(name)
    s, gx = c["solver"], c["cot"]["gx"]
    old = s.adjoint(gx)
    for k in O.NAMES:
        assert np.array_equal(c["g"]["gx"][k], old[k]), k
    size = s._adjoint_sizes()
    buf = {k: np.empty(max(size[k], 1)) for k in O.NAMES}
    g = L.QPGrad(**{k: L.ptr(buf[k], C.c_double) for k in O.NAMES})
    ct = L.QPCot(x=L.ptr(np.ascontiguousarray(gx), C.c_double))
    L.check(L.lib.madipm_solver_adjoint_full(s.h, C.byref(ct), C.byref(g)), "adjoint_full")
    for k in O.NAMES:
        assert np.array_equal(buf[k][:size[k]], old[k]), k
    dbuf = {k: torch.empty(max(size[k], 1), dtype=torch.float64, device="cuda") for k in O.NAMES}
    dgx = torch.as_tensor(gx, device="cuda")
    g = L.QPGrad(**{k: C.cast(dbuf[k].data_ptr(), L.f64p) for k in O.NAMES})
    ct = L.QPCot(x=C.cast(dgx.data_ptr(), L.f64p))
    L.check(L.lib.madipm_solver_adjoint_full_device(s.h, C.byref(ct), C.byref(g),
                                                    L.vp(torch.cuda.current_stream().cuda_stream)), "adjoint_full_device")
    torch.cuda.synchronize()
    for k in O.NAMES:
        assert np.array_equal(dbuf[k][:size[k]].cpu().numpy(), old[k]), k


@pytest.mark.parametrize("name", ["family_min", "family_scaled", "lp", "sparse", "sparse_2shards", "rowlength_g4",
                                  "sparse_g64"])
def test_routes_give_identical_bits(name):
    c = case(name)
    s, cot, g = c["solver"], c["cot"], c["g"]["all"]
    nf = s.adjoint_info()["n_adjoint_factorizations"]
    assert nf == 1                       # adjoint(gx) and every full call so far: one factor for the point
    again = s.adjoint(**_call(cot))
    dev = s.adjoint_device(**_tensors(cot))
    torch.cuda.synchronize()
    for k in O.NAMES:
        assert np.array_equal(again[k], g[k]), k
        assert np.array_equal(dev[k].cpu().numpy(), g[k]), k
    for want in (["c"], ["lvar", "uvar"], ["Avals"], ["Hvals", "lcon"], ["ucon"]):
        sub = s.adjoint(want=want, **_call(cot))
        assert sorted(sub) == sorted(want)
        for k in want:
            assert np.array_equal(sub[k], g[k]), (want, k)
        subd = s.adjoint_device(want=want, **_tensors(cot))
        for k in want:
            assert np.array_equal(subd[k].cpu().numpy(), g[k]), (want, k)
    # each cotangent alone on the device route, and the call is linear in the cotangents
    for sel in F.COTS:
        d = s.adjoint_device(**_tensors(_select(cot, sel)))
        for k in O.NAMES:
            assert np.array_equal(d[k].cpu().numpy(), c["g"][sel][k]), (sel, k)
    g2 = s.adjoint(**_call({k: -2.0 * v for k, v in cot.items()}))
    total = {k: sum(c["g"][sel][k] for sel in F.COTS) for k in O.NAMES}
    for k in O.NAMES:
        assert O.err(g2[k], -2.0 * g[k]) <= 1e-9, k
        assert O.err(total[k], g[k]) <= 1e-9, k
    assert s.adjoint_info()["n_adjoint_factorizations"] == nf


def test_device_route_honours_the_stream():
    c = case("family_min")
    s = c["solver"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cot = {k: v * 1.0 for k, v in _tensors(c["cot"]).items()}     # produced on the side stream
        out = s.adjoint_device(stream=side, **cot)
        doubled = {k: 2.0 * v for k, v in out.items()}                # consumed on it, without a host wait
    side.synchronize()
    for k in O.NAMES:
        assert np.array_equal(doubled[k].cpu().numpy(), 2.0 * c["g"]["all"][k]), k


# ------------------------------------------------------------------ solver state
@pytest.mark.parametrize("name", ["family_min", "family_scaled", "sparse"])
def test_full_adjoint_leaves_the_next_solve_alone(name):
    cot = _reference(FIXTURES[name][0])[1]
    a = new_solver(name)
    first = a.solve()
    a.adjoint(cot["gx"])
    assert a.adjoint_info()["n_adjoint_factorizations"] == 1
    g = a.adjoint(**_call(cot))
    assert a.adjoint_info()["n_adjoint_factorizations"] == 1      # adjoint(gx), then a full call: one factor
    with_adjoint = a.solve()
    b = new_solver(name)
    assert_same(first, b.solve())
    assert_same(with_adjoint, b.solve())
    for k in O.NAMES:
        assert np.array_equal(g[k], case(name)["g"]["all"][k]), k
    # a full call first on the new point factorises once, and adjoint(gx) after it does not again
    g = a.adjoint(**_call(cot))
    old = a.adjoint(cot["gx"])
    assert a.adjoint_info()["n_adjoint_factorizations"] == 2
    for k in O.NAMES:
        assert np.array_equal(g[k], case(name)["g"]["all"][k]), k
        assert np.array_equal(old[k], case(name)["g"]["gx"][k]), k


# ------------------------------------------------------------------ residual
@pytest.mark.parametrize("name", list(FIXTURES))
def test_residual_is_small(name):
    c = case(name)
    print("residual", name, {k: f"{v:.1e}" for k, v in c["res"].items()})
    for sel, r in c["res"].items():
        assert np.isfinite(r) and r <= TOL_LINEAR_SOLVE, (sel, r)
    assert c["info"]["n_adjoints"] == 1 and c["info"]["n_adjoint_factorizations"] == 1


# ------------------------------------------------------------------ refusals
def test_refusals():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    from madipm_amd import solver as S
    qp, cot, _ = _reference(FIXTURES["family_min"][0])
    full, dfull = _call(F.only(cot, "gy", "gcons")), _tensors(F.only(cot, "gy", "gcons"))
    s = MPCSolver(qp, **_kw())
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_full: no solve has run"):
        s.adjoint(**full)
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_full_device: no solve has run"):
        s.adjoint_device(**dfull)
    s.set_max_iter(2)
    assert s.solve().status == S.MAXIMUM_ITERATIONS_EXCEEDED
    with pytest.raises(MadIPMError, match="not SOLVE_SUCCEEDED"):
        s.adjoint(**full)
    s.set_max_iter(300)
    assert s.solve().status == 1
    good = s.adjoint(**full)
    s.update(c=qp.c * 1.01)
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.adjoint(**full)
    assert s.solve().status == 1
    s.adjoint(**full)
    s.update_device(c=torch.as_tensor(qp.c, device="cuda"))
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.adjoint_device(**dfull)
    assert s.solve().status == 1
    s.initialize()
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.adjoint(**full)
    assert s.solve().status == 1
    # all five cotangents NULL, no output at all, a null struct: at the C interface
    g = L.QPGrad()
    buf = np.empty(qp.nvar)
    g.c = L.ptr(buf, C.c_double)
    ct = L.QPCot(y=L.ptr(cot["gy"], C.c_double))
    for fn, tail in ((L.lib.madipm_solver_adjoint_full, ()), (L.lib.madipm_solver_adjoint_full_device, (None,))):
        assert fn(s.h, C.byref(L.QPCot()), C.byref(g), *tail) < 0
        assert b"all five cotangents are NULL" in L.madipm_last_error()
        assert fn(s.h, C.byref(ct), C.byref(L.QPGrad()), *tail) < 0
        assert b"all seven outputs are NULL" in L.madipm_last_error()
        assert fn(s.h, None, C.byref(g), *tail) < 0
        assert b"null cotangent struct" in L.madipm_last_error()
        assert fn(s.h, C.byref(ct), None, *tail) < 0
        assert b"null output struct" in L.madipm_last_error()
    # Avals without prepare_update, on a fresh solver
    t = MPCSolver(qp, **_kw())
    assert t.solve().status == 1
    ga = L.QPGrad()
    abuf = np.empty(qp.nnzj)
    ga.Avals = L.ptr(abuf, C.c_double)
    assert L.lib.madipm_solver_adjoint_full(t.h, C.byref(ct), C.byref(ga)) < 0
    assert b"madipm_solver_prepare_update first" in L.madipm_last_error()
    # after all that a successful call still works, with the bits of the first
    again = s.adjoint(**full)
    for k in O.NAMES:
        assert np.array_equal(again[k], good[k]), k
    # the other formulations, with a message that says they are still to come
    lp, glp = O.lp_fixture()
    for kkt in (S.ScaledSparseKKTSystem, S.NormalKKTSystem):
        t = MPCSolver(lp, **_kw(kkt_system=kkt))
        assert t.solve().status == 1
        with pytest.raises(MadIPMError, match="later release"):
            t.adjoint(glp, gy=np.ones(lp.ncon))
        assert t.adjoint_info() == {"n_adjoints": 0, "n_adjoint_factorizations": 0, "last_residual": 0.0}


def test_refused_on_a_solver_with_a_communicator():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    qp, cot, _ = _reference(FIXTURES["family_min"][0])
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
            s.adjoint(gy=cot["gy"])
    finally:
        L.lib.madipm_solver_destroy(s.h)
        s.h = None
        L.lib.madipm_comm_destroy(comm)


# ------------------------------------------------------------------ the torch layer
def _spy(s, seen):
    orig = s.adjoint_device

    def spy(*a, **kw):
        seen["args"], seen["kw"] = a, dict(kw)
        seen["out"] = orig(*a, **kw)
        return seen["out"]
    s.adjoint_device = spy


def test_default_layer_is_unchanged():
    from madipm_amd import QPLayer
    qp, cot, _ = _reference(FIXTURES["family_min"][0])
    dev = torch.device("cuda")
    t = {k: torch.as_tensor(np.asarray(getattr(qp, k), float), device=dev) for k in O.NAMES}
    s = new_solver("family_min")
    layer = QPLayer(s)
    assert layer.outputs == ("x",)
    leaf = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    x = layer(**leaf)
    assert isinstance(x, torch.Tensor) and torch.equal(x.detach(), s.solution_device()["solution"])
    seen = {}
    _spy(s, seen)
    x.backward(torch.as_tensor(cot["gx"], device=dev))
    assert len(seen["args"]) == 1 and sorted(seen["kw"]) == ["want"]      # the call of before: gx and want alone
    plain = case("family_min")["g"]["gx"]                                  # = adjoint(gx), test_gx_alone_...
    for k in O.NAMES:
        assert np.array_equal(leaf[k].grad.cpu().numpy(), plain[k]), k


def test_layer_with_all_outputs():
    from madipm_amd import QPLayer
    qp, cot, _ = _reference(FIXTURES["family_min"][0])
    dev = torch.device("cuda")
    t = {k: torch.as_tensor(np.asarray(getattr(qp, k), float), device=dev) for k in O.NAMES}
    s = new_solver("family_min")
    layer = QPLayer(s, outputs=("x", "y", "zl", "zu", "cons"))
    leaf = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    out = layer(**leaf)
    sol = s.solution_device()
    assert isinstance(out, tuple) and len(out) == 5
    for o, k in zip(out, ("solution", "multipliers", "multipliers_L", "multipliers_U", "constraints")):
        assert torch.equal(o.detach(), sol[k]), k
    x, y, zl, zu, cons = out
    # a loss of y and cons alone: backward is the direct call with gy and gcons, bit for bit, and passes no other
    gy, gcons = torch.as_tensor(cot["gy"], device=dev), torch.as_tensor(cot["gcons"], device=dev)
    seen = {}
    _spy(s, seen)
    ((y * gy).sum() + (cons * gcons).sum()).backward()
    assert seen["args"] == (None,) and sorted(seen["kw"]) == ["gcons", "gy", "want"]
    assert tuple(seen["kw"]["want"]) == O.NAMES
    ref = s.adjoint_device(gy=gy, gcons=gcons)
    direct = case("family_min")["solver"].adjoint(gy=cot["gy"], gcons=cot["gcons"])
    for k in O.NAMES:
        assert torch.equal(leaf[k].grad, ref[k]), k
        assert np.array_equal(ref[k].cpu().numpy(), direct[k]), k      # update_device installed the same numbers
    # all five used, only uvar requires grad: exactly that gradient is computed
    only = t["uvar"].clone().requires_grad_(True)
    out = QPLayer(s, outputs=("zu", "x", "cons", "y", "zl"))(uvar=only, c=t["c"])     # any order
    w = {"zu": "gzu", "x": "gx", "cons": "gcons", "y": "gy", "zl": "gzl"}
    n1 = s.adjoint_info()["n_adjoints"]
    sum((o * torch.as_tensor(cot[w[k]], device=dev)).sum() for o, k in zip(out, w)).backward()
    assert tuple(seen["kw"]["want"]) == ("uvar",) and sorted(seen["out"]) == ["uvar"]
    assert sorted(seen["kw"]) == ["gcons", "gy", "gzl", "gzu", "want"] and len(seen["args"]) == 1
    assert s.adjoint_info()["n_adjoints"] == n1 + 1
    assert np.array_equal(only.grad.cpu().numpy(), case("family_min")["g"]["all"]["uvar"])
    # x alone used out of several outputs: the call of the default layer
    c = t["c"].clone().requires_grad_(True)
    x, y = QPLayer(s, outputs=("x", "y"))(c=c)
    (x * torch.as_tensor(cot["gx"], device=dev)).sum().backward()
    assert len(seen["args"]) == 1 and sorted(seen["kw"]) == ["want"]
    assert np.array_equal(c.grad.cpu().numpy(), case("family_min")["g"]["gx"]["c"])
    # nothing requires grad: backward is never asked for
    out = QPLayer(s, outputs=("y", "cons"))(c=t["c"])
    assert not any(o.requires_grad for o in out)
