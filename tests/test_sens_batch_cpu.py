"""Batched sensitivities and Jacobians without a GPU: the argument checks of
MPCSolver.tangent_batch / adjoint_batch / jacobian, which run before any library call, the C interface, and the
premise of the GPU Jacobian tests: on the CPU oracle the forward-mode Jacobian (one tangent per parameter) and
the reverse-mode Jacobian (one adjoint per output coordinate) of the same point are the same matrix."""
from __future__ import annotations

import numpy as np
import pytest

import adjoint_full_oracle as F
import adjoint_oracle as O
import tangent_oracle as T

OUTS = ("x", "y", "cons")
PARS = ("c", "lcon", "lvar")
PREMISE_TOL = 1e-9            # relative to max(1, max |J|): two dense solves of one well-scaled system


# ------------------------------------------------------------------ the oracle premise
def _unit(n, i):
    e = np.zeros(n)
    e[i] = 1.0
    return e


def _forward(qp, pt):
    size = T.sizes(qp)
    cols = {p: [T.reference_tangent(qp, pt, {p: _unit(size[p], i)}) for i in range(size[p])] for p in PARS}
    return {(o, p): np.array([t[o] for t in cols[p]]).T for o in OUTS for p in PARS}


def _reverse(qp, pt, gx_only):
    osize = {"x": qp.nvar, "y": qp.ncon, "cons": qp.ncon}
    J = {}
    for o in OUTS:
        rows = []
        for i in range(osize[o]):
            e = _unit(osize[o], i)
            if o == "x" and gx_only:
                rows.append(O.reference_adjoint(qp, pt, e))
            else:
                rows.append(F.reference_adjoint_full(qp, pt, {"g" + o: e}))
        for p in PARS:
            J[(o, p)] = np.array([r[p] for r in rows]).reshape(osize[o], T.sizes(qp)[p])
    return J


@pytest.mark.parametrize("make", [lambda: O.family(1), O.lp_fixture], ids=["family_1", "lp"])
def test_forward_and_reverse_jacobians_agree_on_the_oracle(make):
    qp = make()[0]
    pt = O.reference_ipm(qp)
    fwd = _forward(qp, pt)
    worst = 0.0
    for gx_only in (True, False):       # the gx-only form and the five-cotangent form of the adjoint
        rev = _reverse(qp, pt, gx_only)
        for key in fwd:
            assert fwd[key].shape == rev[key].shape, key
            scale = max(1.0, float(np.max(np.abs(fwd[key]), initial=0.0)))
            e = float(np.max(np.abs(fwd[key] - rev[key]), initial=0.0)) / scale
            worst = max(worst, e)
            assert e <= PREMISE_TOL, (key, gx_only, e)
    # the comparison is not one of zeros: every output moves with the data (at an LP's vertex x does not move
    # with c, so the blocks are taken together)
    for o in OUTS:
        assert max(np.max(np.abs(fwd[(o, p)])) for p in PARS) > 1e-3, o
    print("forward against reverse on the oracle:", f"{worst:.2e}")


# ------------------------------------------------------------------ the argument checks
def test_check_batch_blocks_accepts_and_refuses():
    from madipm_amd import check_batch_blocks
    sizes = {"c": 4, "Hvals": 0, "lcon": 3}
    k, given = check_batch_blocks(sizes, {"c": np.ones((5, 4)), "lcon": [[1, 2, 3]] * 5})
    assert k == 5 and list(given) == ["c", "lcon"]
    assert given["lcon"].dtype == np.float64 and given["lcon"].flags["C_CONTIGUOUS"] and given["lcon"].shape == (5, 3)
    k, given = check_batch_blocks(sizes, {"Hvals": np.zeros((2, 0)), "c": None})     # an empty block still says k
    assert k == 2 and given["Hvals"].shape == (2, 0)
    k, given = check_batch_blocks(sizes, {"c": np.asfortranarray(np.arange(8.0).reshape(2, 4))})
    assert k == 2 and given["c"].flags["C_CONTIGUOUS"] and given["c"][1, 0] == 4.0
    with pytest.raises(ValueError, match=r"c has shape \(4,\), expected \(k, 4\)"):
        check_batch_blocks(sizes, {"c": np.ones(4)})
    with pytest.raises(ValueError, match=r"c has shape \(1, 2, 4\)"):
        check_batch_blocks(sizes, {"c": np.ones((1, 2, 4))})
    with pytest.raises(ValueError, match=r"lcon has shape \(2, 4\), expected \(k, 3\)"):
        check_batch_blocks(sizes, {"lcon": np.ones((2, 4))})
    with pytest.raises(ValueError, match="lcon holds k = 3 columns, c holds 2"):
        check_batch_blocks(sizes, {"c": np.ones((2, 4)), "lcon": np.ones((3, 3))})
    with pytest.raises(ValueError, match="k = 0 columns"):
        check_batch_blocks(sizes, {"c": np.ones((0, 4))})
    with pytest.raises(ValueError, match="tangent_batch: no block given"):
        check_batch_blocks(sizes, {"c": None})
    with pytest.raises(ValueError, match="gy has shape"):
        check_batch_blocks({"x": 4, "y": 3}, {"y": np.ones(3)}, labels={"x": "gx", "y": "gy"}, who="adjoint_batch")


def test_check_batch_blocks_on_the_device_route():
    torch = pytest.importorskip("torch")
    from madipm_amd import check_batch_blocks
    sizes = {"c": 4}
    with pytest.raises(TypeError, match="c must be a torch tensor on the GPU, not ndarray"):
        check_batch_blocks(sizes, {"c": np.ones((2, 4))}, on_device=True, who="tangent_batch_device")
    with pytest.raises(TypeError, match="float64"):
        check_batch_blocks(sizes, {"c": torch.ones((2, 4), dtype=torch.float32)}, on_device=True)
    with pytest.raises(TypeError, match="expected a GPU tensor"):
        check_batch_blocks(sizes, {"c": torch.ones((2, 4), dtype=torch.float64)}, on_device=True)
    with pytest.raises(ValueError, match="not contiguous"):
        check_batch_blocks(sizes, {"c": torch.ones((4, 2), dtype=torch.float64).T}, on_device=True)


class _NoLibrary:
    """MPCSolver's methods on an object without a handle: an argument check that let a call through would fail
    on `h`, not return."""

    def __init__(self, qp):
        self.qp = qp
        self._device = None


def _no_library(qp):
    from madipm_amd import MPCSolver
    s = _NoLibrary(qp)
    s._adjoint_sizes = lambda: MPCSolver._adjoint_sizes(s)
    s._tangent_sizes = lambda: MPCSolver._tangent_sizes(s)
    s._COT_LABELS = MPCSolver._COT_LABELS
    s.sens_batch_cols = MPCSolver.sens_batch_cols
    return s


def test_batch_argument_checks_come_before_the_library():
    from madipm_amd import MPCSolver
    qp = O.family(1)[0]
    s = _no_library(qp)
    n, m = qp.nvar, qp.ncon
    with pytest.raises(ValueError, match="tangent_batch: no block given"):
        MPCSolver.tangent_batch(s)
    with pytest.raises(ValueError, match=r"c has shape \(%d,\)" % n):
        MPCSolver.tangent_batch(s, c=np.ones(n))
    with pytest.raises(ValueError, match="unknown name"):
        MPCSolver.tangent_batch(s, want=["s"], c=np.ones((2, n)))
    with pytest.raises(TypeError, match="not the string"):
        MPCSolver.tangent_batch(s, want="x", c=np.ones((2, n)))
    with pytest.raises(ValueError, match="ucon holds k = 3 columns, c holds 2"):
        MPCSolver.tangent_batch(s, c=np.ones((2, n)), ucon=np.ones((3, m)))
    with pytest.raises(TypeError, match="torch tensor"):
        MPCSolver.tangent_batch_device(s, c=np.ones((2, n)))
    with pytest.raises(ValueError, match="adjoint_batch: no block given"):
        MPCSolver.adjoint_batch(s)
    with pytest.raises(ValueError, match="want is empty"):
        MPCSolver.adjoint_batch(s, np.ones((2, n)), want=[])
    with pytest.raises(ValueError, match=r"gy has shape \(2, %d\), expected \(k, %d\)" % (m + 1, m)):
        MPCSolver.adjoint_batch(s, gy=np.ones((2, m + 1)))
    with pytest.raises(ValueError, match="gcons holds k = 0 columns"):
        MPCSolver.adjoint_batch(s, gcons=np.ones((0, m)))
    with pytest.raises(TypeError, match="torch tensor"):
        MPCSolver.adjoint_batch_device(s, np.ones((2, n)))


def test_jacobian_argument_checks_and_mode():
    from madipm_amd import MPCSolver
    from madipm_amd import solver as S
    sizes = {"x": 5, "y": 3}
    sel = S.check_jacobian_selection(("y", "x"), sizes, "outputs")
    assert list(sel) == ["y", "x"] and np.array_equal(sel["x"], np.arange(5)) and sel["y"].dtype == np.int64
    sel = S.check_jacobian_selection({"x": [4, 0], "y": None}, sizes, "outputs")
    assert np.array_equal(sel["x"], [4, 0]) and np.array_equal(sel["y"], [0, 1, 2])
    with pytest.raises(TypeError, match="not the string"):
        S.check_jacobian_selection("x", sizes, "outputs")
    with pytest.raises(ValueError, match="unknown name 'c' in outputs"):
        S.check_jacobian_selection(("c",), sizes, "outputs")
    with pytest.raises(ValueError, match="outputs is empty"):
        S.check_jacobian_selection((), sizes, "outputs")
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        S.check_jacobian_selection({"y": [3]}, sizes, "outputs")
    with pytest.raises(ValueError, match="1-D integer array"):
        S.check_jacobian_selection({"y": [0.5]}, sizes, "outputs")
    assert S.jacobian_mode(None, 3, 4) == "forward" and S.jacobian_mode(None, 4, 4) == "forward"
    assert S.jacobian_mode(None, 5, 4) == "reverse" and S.jacobian_mode("reverse", 1, 9) == "reverse"
    with pytest.raises(ValueError, match="mode must be"):
        S.jacobian_mode("both", 1, 1)
    s = _no_library(O.family(1)[0])
    s._jacobian = lambda *a: MPCSolver._jacobian(s, *a)
    with pytest.raises(ValueError, match="jacobian: unknown name 'x' in wrt"):
        MPCSolver.jacobian(s, wrt=("x",))
    with pytest.raises(ValueError, match="mode must be"):
        MPCSolver.jacobian(s, mode="both")


def test_abi():
    import ctypes as C
    from madipm_amd import _lib as L
    assert L.madipm_version() == 203       # additive: the version number of the 0.2 line stays
    for f in ("madipm_sens_batch_cols", "madipm_solver_tangent_batch", "madipm_solver_tangent_batch_device",
              "madipm_solver_adjoint_batch", "madipm_solver_adjoint_batch_device", "madipm_solver_sens_batch_info"):
        assert hasattr(L.lib, f), f
    assert L.lib.madipm_sens_batch_cols() == 8
    assert L.lib.madipm_solver_tangent_batch(None, 1, C.byref(L.QPDir()), C.byref(L.QPTan()), 0) < 0
    assert b"null handle" in L.madipm_last_error()
    assert L.lib.madipm_solver_adjoint_batch_device(None, 1, C.byref(L.QPCot()), C.byref(L.QPGrad()), 0, None) < 0
    assert b"null handle" in L.madipm_last_error()
    assert L.lib.madipm_solver_sens_batch_info(None, None, None, None) < 0
    assert b"null handle" in L.madipm_last_error()


def test_layer_jacobian_with_a_stand_in_solver():
    pytest.importorskip("torch")
    from madipm_amd import QPLayer

    class StandIn:
        def jacobian_device(self, **kw):
            return kw

    for polish in (False, True):
        layer = QPLayer(StandIn(), outputs=("x", "y"), polish=polish)
        assert layer.jacobian(("c",)) == {"outputs": ("x", "y"), "wrt": ("c",), "mode": None, "polished": polish}
        assert layer.jacobian({"lcon": [0]}, outputs=("cons",), mode="reverse") == {
            "outputs": ("cons",), "wrt": {"lcon": [0]}, "mode": "reverse", "polished": polish}
