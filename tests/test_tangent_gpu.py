"""MPCSolver.tangent / tangent_device / QPFunction.jvp on the GPU against the CPU oracle
(tangent_oracle.py): the directional derivative (dx, dy, dzl, dzu, dcons) of the solution along a direction of
the seven data blocks.

Two comparisons per fixture and per selection of directions (all seven, and each block alone), both with
err = max |t_gpu - t_ref| / max(1, max |t_ref|) per output block:
  formula  the oracle's shifted formulas evaluated at the point the GPU solve returned: what the kernels compute
  truth    the oracle's tangent at its own optimum (mu = 1e-11): what the caller wants
then the shift (the formula error stays far below what the plain form loses at the same point), the transpose
identity with adjoint() on the GPU, the routes (host / device / repeated / subsets / absent blocks / not-read
entries give the same bits), the solver's state, the residual, the refusals and the torch layer."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import adjoint_oracle as O  # noqa: E402
import tangent_oracle as T  # noqa: E402
import test_adjoint_full_gpu as G  # noqa: E402  (its fixtures, solver options and reference points)
from test_adjoint_gpu import TOL_LINEAR_SOLVE, _kw  # noqa: E402
from test_update_gpu import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

# Largest err measured on the MI355X over all fixtures and selections; each bound is 10 x it
# (floor 1e-9), and neither may exceed 1e-4: every direction block's contribution to every output block is
# >= 1e-2 of the block on some fixture (test_tangent_cpu.py).  By fixture, formula / truth: the 7 x 5 family
# (min, max) 7.3e-10 / 6.2e-8, duplicated 5.7e-10 / 5.2e-8, scaled 3.2e-10 / 8.7e-9, seed 3 1.7e-10 / 5.1e-9, the
# LP 1.6e-10 / 2.4e-9, the sparse QP (1 and 2 shards, G = 64) 2.4e-10 / 3.5e-8, the row-length fixture at G = 4
# 1.1e-10 / 9.1e-7.  The oracle's plain form at the same returned points is off the shifted one by 2.7e-7
# (family) ... 5.3e-6 (seed 3) ... 3.2e-4 (sparse QP): what the shift stays below by three to six orders.
# last_residual: <= 9.9e-14 (the scaled family with lcon alone; <= 4.1e-15 elsewhere).
FORMULA_MEASURED = 7.3e-10      # cons of the 7 x 5 family with Hvals alone; with all seven directions 4.9e-10
TRUTH_MEASURED = 9.2e-7         # x of the row-length fixture with lvar alone (the end point's mu); the family 6.2e-8
TRANSPOSE_MEASURED = 2.3e-15    # |<cot, t> - <g, d>| / max(1, |<cot, t>|): the sparse QP; the families <= 6.0e-16
FORMULA_TOL = max(1e-9, 10.0 * FORMULA_MEASURED)
TRUTH_TOL = max(1e-9, 10.0 * TRUTH_MEASURED)
TRANSPOSE_TOL = 10.0 * TRANSPOSE_MEASURED
CAP = 1e-4

FIXTURES = G.FIXTURES
SELECTIONS = ("all",) + T.NAMES
_cache, _truth = {}, {}


def _reference(make):
    """(qp, directions, cotangents, reference point): test_adjoint_full_gpu's, computed once per problem."""
    qp, cot, pt = G._reference(make)
    return qp, T.directions(qp, 0), cot, pt


def _select(d, sel):
    return dict(d) if sel == "all" else T.only(d, sel)


def _truth_of(make, sel):
    if (make, sel) not in _truth:
        qp, d, _, pt = _reference(make)
        _truth[(make, sel)] = T.reference_tangent(qp, pt, _select(d, sel))
    return _truth[(make, sel)]


def case(name):
    """The fixture solved on the GPU once: solver, stats, and the host route's tangents of all five blocks for
    every selection of directions (all seven first: the call whose counters and residual are kept)."""
    if name not in _cache:
        make = FIXTURES[name][0]
        qp, d, cot, pt = _reference(make)
        s = G.new_solver(name)
        st = s.solve()
        assert st.status == 1, (name, st.status_name)
        t = {"all": s.tangent(**d)}
        info = dict(s.adjoint_info(), **s.tangent_info())     # last_residual: the tangent's
        res = {"all": info["last_residual"]}
        for sel in T.NAMES:
            t[sel] = s.tangent(**_select(d, sel))
            res[sel] = s.tangent_info()["last_residual"]
        point = {"x": st.solution, "y": st.multipliers, "zl": st.multipliers_L, "zu": st.multipliers_U}
        _cache[name] = dict(qp=qp, d=d, cot=cot, pt=pt, make=make, solver=s, stats=st, t=t, info=info, res=res,
                            point=point)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _cache.clear()          # the solvers go while the library is still loaded


def _errs(t, ref):
    return {k: O.err(t[k], ref[k]) for k in T.OUTS}


def _tensors(d):
    return {k: torch.as_tensor(v, device="cuda") for k, v in d.items()}


def figures(name, sel):
    """(formula errors, truth errors, the oracle's plain-minus-shifted difference at the returned point)."""
    c = case(name)
    d = _select(c["d"], sel)
    shifted = T.reference_tangent(c["qp"], c["point"], d, "shifted")
    plain = T.reference_tangent(c["qp"], c["point"], d, "plain")
    return _errs(c["t"][sel], shifted), _errs(c["t"][sel], _truth_of(c["make"], sel)), T.max_err(plain, shifted)


def test_tolerances_fit_the_condition():
    assert FORMULA_TOL <= CAP and TRUTH_TOL <= CAP


# ------------------------------------------------------------------ formula, truth, shift
@pytest.mark.parametrize("sel", SELECTIONS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_formula_at_the_returned_point(name, sel):
    e, _, gap = figures(name, sel)
    print("formula", name, sel, {k: f"{v:.2e}" for k, v in e.items()}, "plain-shifted", f"{gap:.1e}")
    assert max(e.values()) <= FORMULA_TOL, e


@pytest.mark.parametrize("sel", SELECTIONS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_truth_at_the_reference_optimum(name, sel):
    c = case(name)
    assert O.err(c["stats"].solution, c["pt"]["x"]) <= 1e-6        # the same optimum
    _, e, _ = figures(name, sel)
    print("truth", name, sel, {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= TRUTH_TOL, e


@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_shifted_form_is_what_runs(name):
    """Where the oracle's two forms differ by more than 1e-7 at the returned point, the GPU is within a tenth of
    that difference of the shifted one (§13d measured three to six orders of separation)."""
    seen = 0
    for sel in SELECTIONS:
        e, _, gap = figures(name, sel)
        if gap > 1e-7:
            seen += 1
            assert max(e.values()) < 0.1 * gap, (sel, e, gap)
    print("shift", name, "selections with a visible difference:", seen)
    assert seen >= 1       # measured: 1 (the LP) to 3 of the 8 selections on every fixture


def test_fixtures_do_what_they_are_for():
    assert not case("family_max")["qp"].minimize
    assert case("rowlength_g4")["solver"].spmv_group() == 4 and case("sparse_g64")["solver"].spmv_group() == 64
    lp = case("lp")
    assert lp["d"]["Hvals"].shape == (0,) and not any(np.any(lp["t"]["Hvals"][k]) for k in T.OUTS)
    # the copies of a duplicated entry are separate parameters that add: a direction in the copy alone is the
    # same direction in the original alone
    qp, _, hk, ak = O.duplicated_family(1)
    s = case("family_dup")["solver"]
    nh, na = qp.nnzh - len(hk), qp.nnzj - len(ak)
    dH, dA = np.zeros(qp.nnzh), np.zeros(qp.nnzj)
    dH[nh:], dA[na:] = 1.0, -0.5
    a = s.tangent(Hvals=dH, Avals=dA)
    dH, dA = np.zeros(qp.nnzh), np.zeros(qp.nnzj)
    dH[hk], dA[ak] = 1.0, -0.5
    b = s.tangent(Hvals=dH, Avals=dA)
    for k in T.OUTS:
        assert O.err(a[k], b[k]) <= 1e-9 and np.max(np.abs(a["x"])) > 1e-3, k
    # a fixed variable moves with dlvar, its multipliers stay 0
    c = case("family_seed3")
    fixed = c["qp"].lvar == c["qp"].uvar
    assert fixed.any() and np.array_equal(c["t"]["all"]["x"][fixed], c["d"]["lvar"][fixed])
    assert not np.any(c["t"]["all"]["zl"][fixed]) and not np.any(c["t"]["all"]["zu"][fixed])


# ------------------------------------------------------------------ transpose
@pytest.mark.parametrize("name", ["family_seed3", "family_scaled", "sparse"])
def test_tangent_is_the_transpose_of_the_adjoint(name):
    """<cot, tangent(d)> against <adjoint(all five cot), d>, both from the GPU on one solved point, and one
    factorisation for the two calls in either order."""
    c = case(name)
    s, qp, d, cot = c["solver"], c["qp"], c["d"], c["cot"]
    g = s.adjoint(**cot)
    a, b = T.dot(cot, c["t"]["all"]), T.dot_data(g, qp, d)
    rel = abs(a - b) / max(1.0, abs(a))
    print("transpose", name, a, b, f"{rel:.2e}")
    assert s.adjoint_info()["n_adjoint_factorizations"] == 1          # tangent first, then adjoint
    assert rel <= TRANSPOSE_TOL
    r = G.new_solver(name)
    assert r.solve().status == 1
    g2 = r.adjoint(**cot)                                             # adjoint first, then tangent
    t2 = r.tangent(**d)
    assert r.adjoint_info()["n_adjoint_factorizations"] == 1 and r.tangent_info()["n_tangents"] == 1
    for k in O.NAMES:
        assert np.array_equal(g2[k], g[k]), k
    for k in T.OUTS:
        assert np.array_equal(t2[k], c["t"]["all"][k]), k


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("name", ["family_min", "family_scaled", "family_seed3", "lp", "sparse", "sparse_2shards",
                                  "rowlength_g4", "sparse_g64"])
def test_routes_give_identical_bits(name):
    c = case(name)
    s, qp, d, t = c["solver"], c["qp"], c["d"], c["t"]["all"]
    again = s.tangent(**d)
    dev = s.tangent_device(**_tensors(d))
    torch.cuda.synchronize()
    for k in T.OUTS:
        assert np.array_equal(again[k], t[k]), k
        assert np.array_equal(dev[k].cpu().numpy(), t[k]), k
    for want in (["x"], ["zl", "zu"], ["cons"], ["y", "x"], ["cons", "y"]):
        sub = s.tangent(want=want, **d)
        assert sorted(sub) == sorted(want)
        for k in want:
            assert np.array_equal(sub[k], t[k]), (want, k)
        subd = s.tangent_device(want=want, **_tensors(d))
        for k in want:
            assert np.array_equal(subd[k].cpu().numpy(), t[k]), (want, k)
    # an absent block is that block given as zeros, on both routes
    for sel in T.NAMES:
        z = {k: (v if k == sel else np.zeros_like(v)) for k, v in d.items()}
        h, dv = s.tangent(**z), s.tangent_device(**_tensors(z))
        for k in T.OUTS:
            assert np.array_equal(h[k], c["t"][sel][k]), (sel, k)
            assert np.array_equal(dv[k].cpu().numpy(), c["t"][sel][k]), (sel, k)
    # NaN in the entries that are not read changes nothing
    dn = T.with_nan(qp, d)
    h, dv = s.tangent(**dn), s.tangent_device(**_tensors(dn))
    for k in T.OUTS:
        assert np.array_equal(h[k], t[k]), k
        assert np.array_equal(dv[k].cpu().numpy(), t[k]), k
    # linear in the direction
    t2 = s.tangent(**{k: -2.0 * v for k, v in d.items()})
    total = {k: sum(c["t"][sel][k] for sel in T.NAMES) for k in T.OUTS}
    for k in T.OUTS:
        assert O.err(t2[k], -2.0 * t[k]) <= 1e-9, k
        assert O.err(total[k], t[k]) <= 1e-9, k
    assert s.adjoint_info()["n_adjoint_factorizations"] == 1


def test_device_route_honours_the_stream():
    c = case("family_min")
    s = c["solver"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d = {k: v * 1.0 for k, v in _tensors(c["d"]).items()}        # produced on the side stream
        out = s.tangent_device(stream=side, **d)
        doubled = {k: 2.0 * v for k, v in out.items()}               # consumed on it, without a host wait
    side.synchronize()
    for k in T.OUTS:
        assert np.array_equal(doubled[k].cpu().numpy(), 2.0 * c["t"]["all"][k]), k


@pytest.mark.parametrize("name", ["family_min", "family_scaled", "sparse"])
def test_tangent_leaves_the_next_solve_alone(name):
    d = _reference(FIXTURES[name][0])[1]
    a = G.new_solver(name)
    first = a.solve()
    t = a.tangent(**d)
    with_tangent = a.solve()
    b = G.new_solver(name)
    assert_same(first, b.solve())
    assert_same(with_tangent, b.solve())
    for k in T.OUTS:
        assert np.array_equal(t[k], case(name)["t"]["all"][k]), k
    # the new point has its own factor
    a.tangent(**d)
    assert a.adjoint_info()["n_adjoint_factorizations"] == 2 and a.tangent_info()["n_tangents"] == 2


@pytest.mark.parametrize("name", list(FIXTURES))
def test_residual_is_small(name):
    c = case(name)
    print("residual", name, {k: f"{v:.1e}" for k, v in c["res"].items()})
    for sel, r in c["res"].items():
        assert np.isfinite(r) and r <= TOL_LINEAR_SOLVE, (sel, r)
    assert c["info"]["n_tangents"] == 1 and c["info"]["n_adjoint_factorizations"] == 1
    assert c["info"]["n_adjoints"] == 0            # the tangent's counter and residual are its own


def test_first_order_prediction_of_a_resolve():
    """x* + t dx against the re-solved optimum of the data moved by t d (t = 1e-4): second order, far below the
    movement itself."""
    from madipm_amd import MPCSolver
    c = case("family_min")
    step = 1e-4
    new = MPCSolver(T.moved(c["qp"], c["d"], step), **_kw()).solve()
    assert new.status == 1
    move = np.max(np.abs(new.solution - c["stats"].solution))
    miss = np.max(np.abs(new.solution - c["stats"].solution - step * c["t"]["all"]["x"]))
    print("prediction", move, miss)
    assert move > 1e-5 and miss <= 1e-2 * move


# ------------------------------------------------------------------ refusals
def test_refusals():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    from madipm_amd import solver as S
    qp, d, _, _ = _reference(FIXTURES["family_min"][0])
    some, dsome = T.only(d, "c", "lcon"), _tensors(T.only(d, "c", "lcon"))
    s = MPCSolver(qp, **_kw())
    with pytest.raises(MadIPMError, match="madipm_solver_tangent: no solve has run"):
        s.tangent(**some)
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_device: no solve has run"):
        s.tangent_device(**dsome)
    s.set_max_iter(2)
    assert s.solve().status == S.MAXIMUM_ITERATIONS_EXCEEDED
    with pytest.raises(MadIPMError, match="not SOLVE_SUCCEEDED"):
        s.tangent(**some)
    s.set_max_iter(300)
    assert s.solve().status == 1
    good = s.tangent(**some)
    s.update(c=qp.c * 1.01)
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.tangent(**some)
    assert s.solve().status == 1
    s.tangent(**some)
    s.update_device(c=torch.as_tensor(qp.c, device="cuda"))
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.tangent_device(**dsome)
    assert s.solve().status == 1
    s.initialize()
    with pytest.raises(MadIPMError, match="since the last solve"):
        s.tangent(**some)
    assert s.solve().status == 1
    # all seven directions NULL, no output at all, a null struct: at the C interface
    o = L.QPTan()
    buf = np.empty(qp.nvar)
    o.x = L.ptr(buf, C.c_double)
    dr = L.QPDir(c=L.ptr(d["c"], C.c_double))
    for fn, tail in ((L.lib.madipm_solver_tangent, ()), (L.lib.madipm_solver_tangent_device, (None,))):
        assert fn(s.h, C.byref(L.QPDir()), C.byref(o), *tail) < 0
        assert b"all seven directions are NULL" in L.madipm_last_error()
        assert fn(s.h, C.byref(dr), C.byref(L.QPTan()), *tail) < 0
        assert b"all five outputs are NULL" in L.madipm_last_error()
        assert fn(s.h, None, C.byref(o), *tail) < 0
        assert b"null direction struct" in L.madipm_last_error()
        assert fn(s.h, C.byref(dr), None, *tail) < 0
        assert b"null output struct" in L.madipm_last_error()
    # Hvals / Avals directions, and lvar with a fixed variable, without prepare_update, on a fresh solver
    t = MPCSolver(qp, **_kw())
    assert t.solve().status == 1
    for field in ("Hvals", "Avals", "lvar"):
        dd = L.QPDir(**{field: L.ptr(d[field], C.c_double)})
        assert L.lib.madipm_solver_tangent(t.h, C.byref(dd), C.byref(o)) < 0, field
        assert b"madipm_solver_prepare_update first" in L.madipm_last_error(), field
    assert L.lib.madipm_solver_tangent(t.h, C.byref(dr), C.byref(o)) == 0       # c needs nothing
    assert t.tangent_info()["n_tangents"] == 1
    # wrong shape / dtype / device on the device route: before any library call
    n0 = s.tangent_info()["n_tangents"]
    with pytest.raises(ValueError, match="c has shape"):
        s.tangent_device(c=dsome["c"][:-1])
    with pytest.raises(TypeError, match="float64"):
        s.tangent_device(c=dsome["c"].float())
    with pytest.raises(TypeError, match="expected a GPU tensor"):
        s.tangent_device(c=dsome["c"].cpu())
    with pytest.raises(ValueError, match="not contiguous"):
        s.tangent_device(c=torch.zeros(2 * qp.nvar, dtype=torch.float64, device="cuda")[::2])
    with pytest.raises(TypeError, match="torch.cuda.Stream"):
        s.tangent_device(stream=0, **dsome)
    with pytest.raises(ValueError, match="no direction given"):
        s.tangent()
    with pytest.raises(ValueError, match="unknown name"):
        s.tangent(want=["s"], **some)
    assert s.tangent_info()["n_tangents"] == n0
    # after all that a successful call still works, with the bits of the first
    again = s.tangent(**some)
    for k in T.OUTS:
        assert np.array_equal(again[k], good[k]), k
    # the other formulations, with a message that says they are still to come
    lp, _ = O.lp_fixture()
    for kkt in (S.ScaledSparseKKTSystem, S.NormalKKTSystem):
        t = MPCSolver(lp, **_kw(kkt_system=kkt))
        assert t.solve().status == 1
        with pytest.raises(MadIPMError, match="later release"):
            t.tangent(c=np.ones(lp.nvar))
        assert t.tangent_info() == {"n_tangents": 0, "last_residual": 0.0}


def test_refused_on_a_solver_with_a_communicator():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    qp, d, _, _ = _reference(FIXTURES["family_min"][0])
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
            s.tangent(c=d["c"])
    finally:
        L.lib.madipm_solver_destroy(s.h)
        s.h = None
        L.lib.madipm_comm_destroy(comm)


# ------------------------------------------------------------------ the torch layer
def test_layer_forward_mode():
    import torch.autograd.forward_ad as fw
    from madipm_amd import QPLayer
    qp, d, cot, _ = _reference(FIXTURES["family_min"][0])
    dev = torch.device("cuda")
    data = {k: torch.as_tensor(np.asarray(getattr(qp, k), float), device=dev) for k in O.NAMES}
    dt = _tensors(d)
    s = G.new_solver("family_min")
    keys = ("x", "y", "cons")
    sol_key = {"x": "solution", "y": "multipliers", "cons": "constraints"}
    with fw.dual_level():
        out = QPLayer(s, outputs=keys)(c=fw.make_dual(data["c"], dt["c"]), lvar=fw.make_dual(data["lvar"], dt["lvar"]),
                                      uvar=data["uvar"])
        ref = s.tangent_device(want=keys, c=dt["c"], lvar=dt["lvar"])
        sol = s.solution_device()
        assert isinstance(out, tuple) and len(out) == 3
        for o, k in zip(out, keys):
            p, t = fw.unpack_dual(o)
            assert torch.equal(p, sol[sol_key[k]]), k
            assert torch.equal(t, ref[k]), k
        # update_device installed the same numbers: the direct call on the cached solver, bit for bit
        direct = case("family_min")["solver"].tangent(want=keys, c=d["c"], lvar=d["lvar"])
        for k in keys:
            assert np.array_equal(ref[k].cpu().numpy(), direct[k]), k
        # the default layer: one tensor with its tangent
        x = QPLayer(s)(c=fw.make_dual(data["c"], dt["c"]))
        p, t = fw.unpack_dual(x)
        assert isinstance(x, torch.Tensor) and torch.equal(p, s.solution_device()["solution"])
        assert torch.equal(t, s.tangent_device(want=["x"], c=dt["c"])["x"])
    # reverse mode on the same layer is what it was: the gradients of adjoint_device
    leaf = {k: data[k].clone().requires_grad_(True) for k in ("c", "lvar")}
    x, y, cons = QPLayer(s, outputs=keys)(**leaf)
    gx, gy = torch.as_tensor(cot["gx"], device=dev), torch.as_tensor(cot["gy"], device=dev)
    ((x * gx).sum() + (y * gy).sum()).backward()
    g = s.adjoint_device(gx, want=["c", "lvar"], gy=gy)
    for k in leaf:
        assert torch.equal(leaf[k].grad, g[k]), k
    # and the two modes agree on this point: <(gx, gy), jvp(dc, dlvar)> = <vjp(gx, gy), (dc, dlvar)>
    t = s.tangent_device(want=["x", "y"], c=dt["c"], lvar=dt["lvar"])
    a = float((gx * t["x"]).sum() + (gy * t["y"]).sum())
    b = T.dot_data({k: v.cpu().numpy() for k, v in g.items()}, qp, T.only(d, "c", "lvar"))
    assert abs(a - b) <= TRANSPOSE_TOL * max(1.0, abs(a)), (a, b)
