"""Batched sensitivities on the GPU: MPCSolver.tangent_batch / adjoint_batch / jacobian and
QPLayer.jacobian.  The claim is one of bits: row j of every block a batched call returns is what the single call
returns for column j, on every route, for every k around the chunk width W, at the interior point and at the
polished point; the counters, the solver's state and the refusals are the single calls'.

Fixtures and solver options are test_adjoint_full_gpu.py's (the 7 x 5 family with a fixed variable, the LP with
nnzh = 0, the row-length fixture at G = 4, the sparse 1000 x 600 QP at G = 64 and on two shards) plus the
problems without bounds and without rows of test_polish_gpu.py.  Column j is tangent_oracle.directions(qp, seed=j)
and adjoint_full_oracle.cotangents(qp, gx rotated by j, seed=j).

Forward- against reverse-mode Jacobians: both are within FORMULA_TOL of the same formulas (test_tangent_gpu.py,
test_adjoint_full_gpu.py), so they may differ by 2 x FORMULA_TOL at most (the cap).  Largest difference measured on
the MI355X, max |J_fwd - J_rev| / max(1, max |J|) per block: JACOBIAN_MEASURED below (by fixture in DESIGN §13i);
the bound is 10 x it, and may not exceed the cap."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import adjoint_full_oracle as F  # noqa: E402
import adjoint_oracle as O  # noqa: E402
import tangent_oracle as T  # noqa: E402
import test_adjoint_full_gpu as A  # noqa: E402  (its fixtures and solver options)
import test_polish_gpu as G  # noqa: E402  (the problems without bounds and without rows)
from test_adjoint_gpu import _kw  # noqa: E402
from test_tangent_gpu import FORMULA_TOL  # noqa: E402
from test_update_gpu import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

JACOBIAN_MEASURED = 4.5e-16     # the LP (4.44e-16); the 7 x 5 family 3.85e-16, the sparse QP's 12 x 12 selection 2.8e-17
JACOBIAN_TOL = 10.0 * JACOBIAN_MEASURED
JACOBIAN_CAP = 2.0 * FORMULA_TOL

NAMES = ("family_min", "lp", "rowlength_g4", "sparse_g64", "sparse_2shards", "no_bounds", "no_rows")
POLISHED_NAMES = ("family_3", "lp", "rowlength_g4", "no_bounds", "no_rows")     # test_polish_gpu's fixtures
_cache, _pcache = {}, {}


def W():
    from madipm_amd import MPCSolver
    return MPCSolver.sens_batch_cols()


def KS():
    w = W()
    return (1, w - 1, w, w + 1, 2 * w + 1)


def _problem(name):
    """(qp, gx, solver options, lane-group width): nothing here computes a CPU reference point."""
    if name in A.FIXTURES:
        make, extra, width = A.FIXTURES[name]
        qp, gx = make()[:2]
        return qp, np.asarray(gx, float), extra, width
    qp = G.problem(name)
    rng = np.random.default_rng(4100)
    return qp, rng.uniform(0.5, 1.5, qp.nvar) * rng.choice([-1.0, 1.0], qp.nvar), {}, G.FIXTURES[name][1]


def _new_solver(qp, extra, width):
    from madipm_amd import MPCSolver
    with A.spmv_width(width):
        s = MPCSolver(qp, **_kw(**extra))
    if width is not None:
        assert s.spmv_group() == width
    return s


def _columns(qp, gx, k):
    """The first k seeded columns as lists of the single calls' keyword dicts."""
    d = [T.directions(qp, seed=j) for j in range(k)]
    cot = [F.cotangents(qp, np.roll(gx, j), seed=j) for j in range(k)]
    return d, cot


def _stack(cols, k, keys=None):
    return {key: np.array([c[key] for c in cols[:k]]).reshape(k, len(cols[0][key])) for key in (keys or cols[0])}


def case(name):
    """The fixture solved on the GPU once, then the SINGLE calls of the 2 W + 1 seeded columns on the host route
    (tangent of all seven blocks, adjoint of all five cotangents, adjoint of gx alone) with each call's
    residual: computed before any batched call, never modified."""
    if name not in _cache:
        qp, gx, extra, width = _problem(name)
        kmax = 2 * W() + 1
        d, cot = _columns(qp, gx, kmax)
        s = _new_solver(qp, extra, width)
        st = s.solve()
        assert st.status == 1, (name, st.status_name)
        t, g, gxo, rt, rg, rx = [], [], [], [], [], []
        for j in range(kmax):
            t.append(s.tangent(**d[j]))
            rt.append(s.tangent_info()["last_residual"])
            g.append(s.adjoint(**cot[j]))
            rg.append(s.adjoint_info()["last_residual"])
            gxo.append(s.adjoint(cot[j]["gx"]))
            rx.append(s.adjoint_info()["last_residual"])
        _cache[name] = dict(qp=qp, gx=gx, extra=extra, width=width, d=d, cot=cot, solver=s, stats=st, t=t, g=g,
                            gxo=gxo, rt=rt, rg=rg, rx=rx)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _cache.clear()          # the solvers go while the library is still loaded
    _pcache.clear()


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def _rows_equal(batch, singles, keys, what):
    """Row j of every block of `batch` has the bits of singles[j]."""
    for key in keys:
        b = _np(batch[key])
        assert b.shape == (len(singles), singles[0][key].shape[0]), (what, key, b.shape)
        for j, one in enumerate(singles):
            assert np.array_equal(b[j], _np(one[key]), equal_nan=True), (what, key, j)


def _tensors(v):
    return {k: torch.as_tensor(a, device="cuda") for k, a in v.items()}


def test_tolerance_fits_the_cap():
    assert JACOBIAN_TOL <= JACOBIAN_CAP


# ------------------------------------------------------------------ 1: the columns are the single calls
@pytest.mark.parametrize("name", NAMES)
def test_columns_are_the_single_calls(name):
    c = case(name)
    s, qp = c["solver"], c["qp"]
    for k in KS():
        tb = s.tangent_batch(**_stack(c["d"], k))
        _rows_equal(tb, c["t"][:k], T.OUTS, ("tangent", k))
        gb = s.adjoint_batch(**_stack(c["cot"], k))
        _rows_equal(gb, c["g"][:k], O.NAMES, ("adjoint", k))
        xb = s.adjoint_batch(_stack(c["cot"], k, ("gx",))["gx"])
        _rows_equal(xb, c["gxo"][:k], O.NAMES, ("adjoint of gx", k))
    # whatever stands in the entries the conventions do not read changes no bit
    k = W() + 1
    nan = [T.with_nan(qp, d) for d in c["d"][:k]]
    if name == "family_min":
        assert all(np.isnan(nan[0][key]).any() for key in ("lvar", "uvar", "lcon", "ucon"))
    _rows_equal(s.tangent_batch(**_stack(nan, k)), c["t"][:k], T.OUTS, "not-read entries")
    assert s.adjoint_info()["n_adjoint_factorizations"] == 1


# ------------------------------------------------------------------ 2: the routes
@pytest.mark.parametrize("name", ["family_min", "lp", "sparse_g64", "no_bounds", "no_rows"])
def test_routes_give_identical_bits(name):
    c = case(name)
    s = c["solver"]
    k = W() + 1
    d, cot = _stack(c["d"], k), _stack(c["cot"], k)
    # a single call before the batches, and the same call after them
    one_t, one_g = s.tangent(**c["d"][2]), s.adjoint(**c["cot"][2])
    # device route, default and side stream
    _rows_equal(s.tangent_batch_device(**_tensors(d)), c["t"][:k], T.OUTS, "tangent, device")
    _rows_equal(s.adjoint_batch_device(**_tensors(cot)), c["g"][:k], O.NAMES, "adjoint, device")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dt = {key: v * 1.0 for key, v in _tensors(d).items()}          # produced on the side stream
        tb = s.tangent_batch_device(stream=side, **dt)
        ct = {key: v * 1.0 for key, v in _tensors(cot).items()}
        gb = s.adjoint_batch_device(stream=side, **ct)
        doubled = {key: 2.0 * v for key, v in tb.items()}              # consumed on it, without a host wait
    side.synchronize()
    _rows_equal(gb, c["g"][:k], O.NAMES, "adjoint, side stream")
    _rows_equal({key: 0.5 * v for key, v in doubled.items()}, c["t"][:k], T.OUTS, "tangent, side stream")
    # subsets of the outputs
    sub = s.tangent_batch(want=["cons", "x"], **d)
    assert list(sub) == ["x", "cons"]
    _rows_equal(sub, c["t"][:k], ("x", "cons"), "tangent, want")
    sub = s.adjoint_batch(want=["lvar", "Avals"], **cot)
    assert list(sub) == ["Avals", "lvar"]
    _rows_equal(sub, c["g"][:k], ("Avals", "lvar"), "adjoint, want")
    # absent blocks: the single calls with the same blocks absent
    some = [T.only(x, "c", "lcon") for x in c["d"][:k]]
    _rows_equal(s.tangent_batch(**_stack(some, k)), [s.tangent(**x) for x in some], T.OUTS, "tangent, absent")
    csome = [F.only(x, "gy", "gzu") for x in c["cot"][:k]]
    _rows_equal(s.adjoint_batch(**_stack(csome, k)), [s.adjoint(**x) for x in csome], O.NAMES, "adjoint, absent")
    # one batch split by the caller into two
    for lo, hi in ((0, 3), (3, k)):
        part = {key: v[lo:hi] for key, v in d.items()}
        _rows_equal(s.tangent_batch(**part), c["t"][lo:hi], T.OUTS, ("tangent, split", lo))
        part = {key: v[lo:hi] for key, v in cot.items()}
        _rows_equal(s.adjoint_batch(**part), c["g"][lo:hi], O.NAMES, ("adjoint, split", lo))
    again_t, again_g = s.tangent(**c["d"][2]), s.adjoint(**c["cot"][2])
    for key in T.OUTS:
        assert np.array_equal(one_t[key], c["t"][2][key]) and np.array_equal(again_t[key], one_t[key]), key
    for key in O.NAMES:
        assert np.array_equal(one_g[key], c["g"][2][key]) and np.array_equal(again_g[key], one_g[key]), key
    assert s.adjoint_info()["n_adjoint_factorizations"] == 1


# ------------------------------------------------------------------ 3: counters and the residual
@pytest.mark.parametrize("name", ["family_min", "sparse_g64"])
def test_counters_and_residual(name):
    c = case(name)
    s, w = c["solver"], W()
    for k in KS():
        b0, t0, a0 = s.sens_batch_info(), s.tangent_info(), s.adjoint_info()
        s.tangent_batch(want=["x"], **_stack(c["d"], k))
        b1, t1 = s.sens_batch_info(), s.tangent_info()
        assert b1["n_batches"] == b0["n_batches"] + 1 and b1["n_columns"] == b0["n_columns"] + k
        assert b1["n_chunks"] == b0["n_chunks"] + -(-k // w)
        assert t1["n_tangents"] == t0["n_tangents"] + k and t1["last_residual"] == max(c["rt"][:k])
        s.adjoint_batch(want=["c"], **_stack(c["cot"], k))
        b2, a1 = s.sens_batch_info(), s.adjoint_info()
        assert b2["n_chunks"] == b1["n_chunks"] + -(-k // w) and b2["n_columns"] == b1["n_columns"] + k
        assert a1["n_adjoints"] == a0["n_adjoints"] + k and a1["last_residual"] == max(c["rg"][:k])
        s.adjoint_batch(_stack(c["cot"], k, ("gx",))["gx"], want=["c"])
        assert s.adjoint_info()["last_residual"] == max(c["rx"][:k])
        assert s.tangent_info() == t1              # the adjoint's batches leave the tangent's figures alone
    s.tangent(**c["d"][0])
    s.adjoint(**c["cot"][0])
    assert s.adjoint_info()["n_adjoint_factorizations"] == 1     # one factor for every mix of calls on the point
    assert max(c["rt"] + c["rg"] + c["rx"]) < 1e-10


# ------------------------------------------------------------------ 4: the solver's state
@pytest.mark.parametrize("name", ["family_min", "sparse_g64"])
def test_batches_leave_the_next_solve_alone(name):
    c = case(name)
    k = W() + 1
    a = _new_solver(c["qp"], c["extra"], c["width"])
    first = a.solve()
    tb = a.tangent_batch(**_stack(c["d"], k))
    gb = a.adjoint_batch(**_stack(c["cot"], k))
    with_batches = a.solve()
    b = _new_solver(c["qp"], c["extra"], c["width"])
    assert_same(first, b.solve())
    assert_same(with_batches, b.solve())
    _rows_equal(tb, c["t"][:k], T.OUTS, "a fresh solver's first call")     # the scratch's first use
    _rows_equal(gb, c["g"][:k], O.NAMES, "a fresh solver's first call")
    # the new point has its own factor
    a.adjoint_batch(_stack(c["cot"], 2, ("gx",))["gx"])
    assert a.adjoint_info()["n_adjoint_factorizations"] == 2


# ------------------------------------------------------------------ 5: the polished point
def pcase(name):
    if name not in _pcache:
        from madipm_amd import PolishVerdict
        qp = G.problem(name)
        rng = np.random.default_rng(4100)
        gx = rng.uniform(0.5, 1.5, qp.nvar) * rng.choice([-1.0, 1.0], qp.nvar)
        s = G.new_solver(name)
        assert s.solve().status == 1
        assert s.polish()["info"]["verdict"] == PolishVerdict.POLISHED
        _pcache[name] = dict(qp=qp, gx=gx, solver=s)
    return _pcache[name]


@pytest.mark.parametrize("name", POLISHED_NAMES)
def test_polished_batches_are_the_single_polished_calls(name):
    c = pcase(name)
    s, k = c["solver"], W() + 1
    d, cot = _columns(c["qp"], c["gx"], k)
    t = [s.tangent(polished=True, **x) for x in d]
    g = [s.adjoint(polished=True, **x) for x in cot]
    i0, b0 = s.polished_sens_info(), s.sens_batch_info()
    _rows_equal(s.tangent_batch(polished=True, **_stack(d, k)), t, T.OUTS, "tangent")
    _rows_equal(s.adjoint_batch(polished=True, **_stack(cot, k)), g, O.NAMES, "adjoint")
    _rows_equal(s.tangent_batch_device(polished=True, **_tensors(_stack(d, k))), t, T.OUTS, "tangent, device")
    _rows_equal(s.adjoint_batch_device(polished=True, **_tensors(_stack(cot, k))), g, O.NAMES, "adjoint, device")
    i1, b1 = s.polished_sens_info(), s.sens_batch_info()
    assert i1["n_tangents"] == i0["n_tangents"] + 2 * k and i1["n_adjoints"] == i0["n_adjoints"] + 2 * k
    assert b1["n_batches"] == b0["n_batches"] + 4 and b1["n_columns"] == b0["n_columns"] + 4 * k
    assert b1["n_chunks"] == b0["n_chunks"]
    # an interior-point batch takes the LDL^T; the next polished batch restores the polish's factor
    s.tangent_batch(**_stack(d, 2))
    _rows_equal(s.adjoint_batch(polished=True, **_stack(cot, 2)), g[:2], O.NAMES, "after an interior-point batch")
    assert s.polished_sens_info()["n_factorizations"] == i1["n_factorizations"] + 1


def test_polished_refusals():
    from madipm_amd import MadIPMError, PolishVerdict
    qp = G.problem("family_0")
    d, cot = _columns(qp, np.ones(qp.nvar), 2)
    some, csome = _stack([T.only(x, "c", "lcon") for x in d], 2), _stack([F.only(x, "gx", "gy") for x in cot], 2)
    s = G.new_solver("family_0")
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_batch: no solve has run"):
        s.tangent_batch(polished=True, **some)
    assert s.solve().status == 1
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_batch_device: no polish has run on the point"):
        s.tangent_batch_device(polished=True, **_tensors(some))
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_batch: no polish has run on the point"):
        s.adjoint_batch(polished=True, **csome)
    good = s.polish()
    t0 = s.tangent_batch(polished=True, **some)
    forced = (good["active_var"].copy(), good["active_row"].copy())
    forced[0][1] = 1            # §13f's supplied set with variable 1's inactive upper bound
    assert s.polish(active_var=forced[0], active_row=forced[1])["info"]["verdict"] == PolishVerdict.WRONG_SET
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_batch: the last polish ended with verdict WRONG_SET"):
        s.tangent_batch(polished=True, **some)
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_batch_device: the last polish ended with verdict "
                                          "WRONG_SET, not POLISHED"):
        s.adjoint_batch_device(polished=True, **_tensors(csome))
    assert s.sens_batch_info()["n_batches"] == 1
    s.polish()
    _rows_equal(s.tangent_batch(polished=True, **some), [{k: v[j] for k, v in t0.items()} for j in range(2)], T.OUTS,
                "after the refusals")


# ------------------------------------------------------------------ 6: Jacobians
def _jac_selection(name, qp):
    """(outputs, wrt): every coordinate on the small fixtures, 12 parameters and 12 output coordinates
    spread over two blocks each on the sparse QP."""
    if name != "sparse":
        return ("x", "y", "cons"), ("c", "lcon", "lvar")
    pick = lambda n: np.linspace(0, n - 1, 6).astype(np.int64)     # noqa: E731
    return {"x": pick(qp.nvar), "y": pick(qp.ncon)}, {"c": pick(qp.nvar), "lcon": pick(qp.ncon)}


@pytest.mark.parametrize("name", ["family_min", "lp", "sparse"])
def test_jacobians(name):
    from madipm_amd import solver as S
    qp, gx, extra, width = _problem(name)
    s = _new_solver(qp, extra, width)
    assert s.solve().status == 1
    outputs, wrt = _jac_selection(name, qp)
    osel = S.check_jacobian_selection(outputs, s._tangent_sizes(), "outputs")
    psel = S.check_jacobian_selection(wrt, s._adjoint_sizes(), "wrt")
    n_par, n_out = sum(map(len, psel.values())), sum(map(len, osel.values()))
    b0 = s.sens_batch_info()
    fwd = s.jacobian(outputs, wrt, mode="forward")
    b1 = s.sens_batch_info()
    assert b1["n_columns"] == b0["n_columns"] + n_par
    rev = s.jacobian(outputs, wrt, mode="reverse")
    b2 = s.sens_batch_info()
    assert b2["n_columns"] == b1["n_columns"] + n_out
    assert set(fwd) == set(rev) == {(o, p) for o in osel for p in psel}
    # forward columns are tangent(par = e_i), reverse rows adjoint() of the unit cotangent: bit for bit
    for p, idx in psel.items():
        for col, i in list(enumerate(idx))[:: max(1, len(idx) // 4)]:
            e = np.zeros(s._adjoint_sizes()[p])
            e[i] = 1.0
            t = s.tangent(want=list(osel), **{p: e})
            for o, oi in osel.items():
                assert np.array_equal(fwd[(o, p)][:, col], t[o][oi]), (o, p, i)
    for o, idx in osel.items():
        for row, i in list(enumerate(idx))[:: max(1, len(idx) // 4)]:
            e = np.zeros(s._tangent_sizes()[o])
            e[i] = 1.0
            g = s.adjoint(want=list(psel), **{"g" + o: e})
            for p, pi in psel.items():
                assert np.array_equal(rev[(o, p)][row], g[p][pi]), (o, p, i)
    # the two modes agree
    worst = 0.0
    for key in fwd:
        assert fwd[key].shape == rev[key].shape == (len(osel[key[0]]), len(psel[key[1]])), key
        e = O.err(fwd[key], rev[key])
        worst = max(worst, e)
    print("jacobian", name, f"forward against reverse {worst:.2e}")
    assert worst <= JACOBIAN_TOL, worst
    # mode=None takes the side with fewer columns (forward on a tie), seen through the counters
    auto = s.jacobian(outputs, wrt)
    b3 = s.sens_batch_info()
    assert b3["n_columns"] == b2["n_columns"] + min(n_par, n_out)
    side = fwd if n_par <= n_out else rev
    for key in side:
        assert np.array_equal(auto[key], side[key]), key
    one_sided = s.jacobian(("x",), {"c": [0, 1]})               # 2 parameters against nvar outputs: forward
    assert s.sens_batch_info()["n_columns"] == b3["n_columns"] + 2
    assert np.array_equal(one_sided[("x", "c")], s.jacobian(("x",), {"c": [0, 1]}, mode="forward")[("x", "c")])
    # the device route returns the same bits
    dj = s.jacobian_device(outputs, wrt, mode="forward")
    for key in fwd:
        assert np.array_equal(dj[key].cpu().numpy(), fwd[key]), key
    assert s.adjoint_info()["n_adjoint_factorizations"] == 1


@pytest.mark.parametrize("polish", [False, True])
def test_layer_jacobian(polish):
    from madipm_amd import QPLayer
    qp = G.problem("family_3")
    s = G.new_solver("family_3")
    data = {k: torch.as_tensor(np.asarray(getattr(qp, k), float), device="cuda") for k in O.NAMES}
    layer = QPLayer(s, outputs=("x", "y"), polish=polish)
    layer(**data)
    wrt = {"c": None, "lcon": [0, 2]}
    J = layer.jacobian(wrt)
    ref = s.jacobian_device(outputs=("x", "y"), wrt=wrt, polished=polish)
    assert set(J) == set(ref) == {("x", "c"), ("x", "lcon"), ("y", "c"), ("y", "lcon")}
    for key in ref:
        assert isinstance(J[key], torch.Tensor) and J[key].is_cuda and torch.equal(J[key], ref[key]), key
    assert J[("y", "lcon")].shape == (qp.ncon, 2)
    # a column is the single call at the layer's point
    e = torch.zeros(qp.nvar, dtype=torch.float64, device="cuda")
    e[1] = 1.0
    t = s.tangent_device(want=["x", "y"], c=e, polished=polish)
    assert torch.equal(J[("x", "c")][:, 1], t["x"]) and torch.equal(J[("y", "c")][:, 1], t["y"])
    other = layer.jacobian(("c",), outputs=("cons",), mode="reverse")
    assert other[("cons", "c")].shape == (qp.ncon, qp.nvar)
    info = s.polished_sens_info()
    assert (info["n_tangents"] + info["n_adjoints"] > 0) == polish


# ------------------------------------------------------------------ 7: refusals
def _unchanged(s, before):
    assert (s.sens_batch_info(), s.tangent_info(), s.adjoint_info()) == before


def test_refusals():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    qp, gx, extra, width = _problem("family_min")
    d, cot = _columns(qp, gx, 2)
    some, csome = _stack([T.only(x, "c", "lcon") for x in d], 2), _stack([F.only(x, "gx", "gy") for x in cot], 2)
    s = MPCSolver(qp, **_kw())
    # before a solve
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_batch: no solve has run"):
        s.tangent_batch(**some)
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_batch_device: no solve has run"):
        s.tangent_batch_device(**_tensors(some))
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_batch: no solve has run"):
        s.adjoint_batch(**csome)
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_batch_device: no solve has run"):
        s.adjoint_batch_device(**_tensors(csome))
    assert s.solve().status == 1
    t0, g0 = s.tangent_batch(**some), s.adjoint_batch(**csome)
    before = (s.sens_batch_info(), s.tangent_info(), s.adjoint_info())
    assert before[0] == {"n_batches": 2, "n_columns": 4, "n_chunks": 2}
    # after an update
    s.update(c=qp.c * 1.01)
    with pytest.raises(MadIPMError, match="madipm_solver_tangent_batch: an update, update_device or initialize"):
        s.tangent_batch(**some)
    with pytest.raises(MadIPMError, match="madipm_solver_adjoint_batch_device: an update, update_device or initialize"):
        s.adjoint_batch_device(**_tensors(csome))
    s.update(c=qp.c)
    assert s.solve().status == 1
    # k = 0 and k < 0, all blocks NULL, all outputs NULL, null structs: at the C interface
    o, gr = L.QPTan(), L.QPGrad()
    buf = np.empty(2 * qp.nvar)
    o.x = gr.c = L.ptr(buf, C.c_double)
    dr, ct = L.QPDir(c=L.ptr(some["c"], C.c_double)), L.QPCot(x=L.ptr(csome["gx"], C.c_double))
    for fn, tail, who in ((L.lib.madipm_solver_tangent_batch, (), b"madipm_solver_tangent_batch: "),
                          (L.lib.madipm_solver_tangent_batch_device, (None,), b"madipm_solver_tangent_batch_device: ")):
        for k in (0, -3):
            assert fn(s.h, k, C.byref(dr), C.byref(o), 0, *tail) < 0
            assert who + b"k = " + str(k).encode() in L.madipm_last_error()
            assert fn(s.h, k, C.byref(dr), C.byref(o), 1, *tail) < 0 and who + b"k = " in L.madipm_last_error()
        assert fn(s.h, 2, C.byref(L.QPDir()), C.byref(o), 0, *tail) < 0
        assert who + b"all seven directions are NULL" in L.madipm_last_error()
        assert fn(s.h, 2, C.byref(dr), C.byref(L.QPTan()), 0, *tail) < 0
        assert who + b"all five outputs are NULL" in L.madipm_last_error()
        assert fn(s.h, 2, None, C.byref(o), 0, *tail) < 0 and b"null direction struct" in L.madipm_last_error()
        assert fn(s.h, 2, C.byref(dr), None, 0, *tail) < 0 and b"null output struct" in L.madipm_last_error()
    for fn, tail, who in ((L.lib.madipm_solver_adjoint_batch, (), b"madipm_solver_adjoint_batch: "),
                          (L.lib.madipm_solver_adjoint_batch_device, (None,), b"madipm_solver_adjoint_batch_device: ")):
        assert fn(s.h, 0, C.byref(ct), C.byref(gr), 0, *tail) < 0 and who + b"k = 0" in L.madipm_last_error()
        assert fn(s.h, 2, C.byref(L.QPCot()), C.byref(gr), 0, *tail) < 0
        assert who + b"all five cotangents are NULL" in L.madipm_last_error()
        assert fn(s.h, 2, C.byref(ct), C.byref(L.QPGrad()), 0, *tail) < 0
        assert who + b"all seven outputs are NULL" in L.madipm_last_error()
        assert fn(s.h, 2, None, C.byref(gr), 0, *tail) < 0 and b"null cotangent struct" in L.madipm_last_error()
        assert fn(s.h, 2, C.byref(ct), None, 0, *tail) < 0 and b"null output struct" in L.madipm_last_error()
    # blocks that need prepare_update, on a solver that never prepared
    t = MPCSolver(qp, **_kw())
    assert t.solve().status == 1
    full = _stack(d, 2)
    for field in ("Hvals", "Avals", "lvar"):
        dd = L.QPDir(**{field: L.ptr(full[field], C.c_double)})
        assert L.lib.madipm_solver_tangent_batch(t.h, 2, C.byref(dd), C.byref(o), 0) < 0, field
        assert b"madipm_solver_tangent_batch: Avals, Hvals" in L.madipm_last_error(), field
    ga = L.QPGrad(Avals=L.ptr(np.empty(2 * qp.nnzj), C.c_double))
    assert L.lib.madipm_solver_adjoint_batch(t.h, 2, C.byref(ct), C.byref(ga), 0) < 0
    assert b"madipm_solver_adjoint_batch: Avals, Hvals" in L.madipm_last_error()
    assert t.sens_batch_info() == {"n_batches": 0, "n_columns": 0, "n_chunks": 0}
    assert t.adjoint_info()["n_adjoint_factorizations"] == 0
    # the Python checks come before the library
    with pytest.raises(ValueError, match="c has shape"):
        s.tangent_batch(c=some["c"][0])
    with pytest.raises(ValueError, match="holds k = 1 columns"):
        s.adjoint_batch(csome["gx"], gy=csome["gy"][:1])
    with pytest.raises(TypeError, match="torch.cuda.Stream"):
        s.tangent_batch_device(stream=0, **_tensors(some))
    # nothing above counted or changed anything: the same calls give the same bits
    _unchanged(s, before)
    t1, g1 = s.tangent_batch(**some), s.adjoint_batch(**csome)
    for k in T.OUTS:
        assert np.array_equal(t1[k], t0[k]), k
    for k in O.NAMES:
        assert np.array_equal(g1[k], g0[k]), k


def test_refused_on_a_solver_with_a_communicator():
    import ctypes as C
    from madipm_amd import MPCSolver, MadIPMError
    from madipm_amd import _lib as L
    qp, gx, _, _ = _problem("family_min")
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
        with pytest.raises(MadIPMError, match="madipm_solver_tangent_batch: a solver created with a communicator"):
            s.tangent_batch(c=np.ones((2, qp.nvar)))
        with pytest.raises(MadIPMError, match="madipm_solver_adjoint_batch: a solver created with a communicator"):
            s.adjoint_batch(np.ones((2, qp.nvar)))
        assert s.sens_batch_info() == {"n_batches": 0, "n_columns": 0, "n_chunks": 0}
    finally:
        L.lib.madipm_solver_destroy(s.h)
        s.h = None
        L.lib.madipm_comm_destroy(comm)
