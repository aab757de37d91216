"""The oracle of the five-cotangent adjoint (adjoint_full_oracle.py) against central differences,
its two forms against each other, the conditions the fixtures of test_adjoint_full_gpu.py must meet, and the
argument checks of MPCSolver.adjoint / adjoint_device / QPLayer — all without a GPU."""
from __future__ import annotations

import numpy as np
import pytest

import adjoint_full_oracle as F
import adjoint_oracle as O

# Central differences (h = 1e-6) of l = gx'x + gy'y + gzl'zl + gzu'zu + gcons'(A x) against the shifted formulas
# at reference_ipm's optimum, largest err over the seven blocks as measured with this file; each bound is
# 10 x it.  The plain form on the same fixtures: 2.8e-7, 8.4e-9, 8.5e-9, 9.7e-9, 2.8e-7, 2.8e-7, 1.1e-7, 1.4e-4.
FD_FIXTURES = {
    "family0": (lambda: O.family(0), 9.8e-10),
    "family1": (lambda: O.family(1), 8.9e-10),
    "family2": (lambda: O.family(2), 7.6e-10),
    "family3": (lambda: O.family(3), 1.1e-9),
    "family0_max": (lambda: O.family(0, minimize=False), 9.8e-10),
    "family0_dup": (lambda: O.duplicated_family(0)[:2], 9.8e-10),
    "lp": (O.lp_fixture, 4.1e-10),
    "family0_scaled": (lambda: O.scaled_family(0), 8.0e-7),   # gradients around 1e3: the differences are the coarser side
}
# the problems test_adjoint_full_gpu.py solves
GPU_FIXTURES = {
    "family_min": lambda: O.family(1),
    "family_max": lambda: O.family(1, minimize=False),
    "family_scaled": lambda: O.scaled_family(1),
    "family_dup": lambda: O.duplicated_family(1)[:2],
    "family_seed3": lambda: O.family(3),
    "lp": O.lp_fixture,
    "sparse": O.sparse_fixture,
    "rowlength": F.rowlength_fixture,
}
NO_CANCEL = ("c", "Hvals", "Avals", "lcon", "ucon")
_solved = {}


def solved(make):
    """(qp, cotangents, reference point) of a fixture, computed once and never modified."""
    if make not in _solved:
        qp, gx = make()
        _solved[make] = (qp, F.cotangents(qp, gx), O.reference_ipm(qp))
    return _solved[make]


@pytest.mark.parametrize("name", list(FD_FIXTURES))
def test_shifted_form_matches_central_differences(name):
    make, measured = FD_FIXTURES[name]
    qp, cot, pt = solved(make)
    fd = F.finite_difference(qp, cot, h=1e-6)
    gs, gp = F.reference_adjoint_full(qp, pt, cot, "shifted"), F.reference_adjoint_full(qp, pt, cot, "plain")
    es = {k: O.err(gs[k], fd[k]) for k in O.NAMES}
    ep = {k: O.err(gp[k], fd[k]) for k in O.NAMES}
    print(name, "shifted", f"{max(es.values()):.2e}", "plain", f"{max(ep.values()):.2e}")
    assert max(es.values()) <= 10.0 * measured, es


@pytest.mark.parametrize("name", list(FD_FIXTURES) + ["rowlength", "sparse"])
def test_gx_alone_is_the_adjoint_of_x(name):
    make = FD_FIXTURES[name][0] if name in FD_FIXTURES else GPU_FIXTURES[name]
    qp, cot, pt = solved(make)
    ref = O.reference_adjoint(qp, pt, cot["gx"])
    for form in ("shifted", "plain"):
        g = F.reference_adjoint_full(qp, pt, F.only(cot, "gx"), form)
        assert max(O.err(g[k], ref[k]) for k in O.NAMES) <= 1e-12, form


@pytest.mark.parametrize("name", list(FD_FIXTURES) + ["rowlength"])
def test_the_forms_differ_in_the_free_bounds_only(name):
    """On c, Hvals, Avals, lcon, ucon the two forms are the same numbers (measured: <= 1.3e-15).  lvar / uvar
    is where the plain form multiplies a rounding-level difference by Sigma: up to 2.8e-7 on the family,
    1.4e-4 on its scaled variant, 1.2e-7 on the row-length fixture.  (On sparse_fixture the plain form's
    right-hand side of 1e9 also spoils the sparse LU without refinement, 1e-5 on every block: not compared.)"""
    make = FD_FIXTURES[name][0] if name in FD_FIXTURES else GPU_FIXTURES[name]
    qp, cot, pt = solved(make)
    gs, gp = F.reference_adjoint_full(qp, pt, cot, "shifted"), F.reference_adjoint_full(qp, pt, cot, "plain")
    e = {k: O.err(gs[k], gp[k]) for k in O.NAMES}
    print(name, {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e[k] for k in NO_CANCEL) <= 1e-12, e
    fx = qp.lvar == qp.uvar             # a fixed variable's lvar has no Sigma in it
    assert O.err(gs["lvar"][fx], gp["lvar"][fx]) <= 1e-12


def test_every_cotangent_reaches_every_block():
    """For every cotangent and every data block some fixture of the GPU set has that cotangent's contribution
    alone >= 1e-2 of the block's largest entry (all five given): a dropped cotangent or direct term cannot
    hide under the cap of 1e-4.  Every pair is reachable: each cotangent moves a = K^-1 g, and a enters every
    block.  (Measured: the smallest best ratio is 7.1e-2, gcons -> uvar.)"""
    best = {(c, k): 0.0 for c in F.COTS for k in O.NAMES}
    for name, make in GPU_FIXTURES.items():
        qp, cot, pt = solved(make)
        full = F.reference_adjoint_full(qp, pt, cot)
        for c in F.COTS:
            g = F.reference_adjoint_full(qp, pt, F.only(cot, c))
            for k in O.NAMES:
                if full[k].size and np.any(full[k]):      # ucon of the LP is all 0: equality rows
                    best[(c, k)] = max(best[(c, k)], float(np.max(np.abs(g[k])) / np.max(np.abs(full[k]))))
    print({f"{c}->{k}": f"{v:.1e}" for (c, k), v in best.items()})
    assert min(best.values()) >= 1e-2, {k: v for k, v in best.items() if v < 1e-2}


def test_upper_bound_fixtures_are_chosen_accordingly():
    """family(0) has no active upper variable bound (gzu does next to nothing there); seeds 1 and 3, which the
    GPU set uses, have one."""
    for seed, expect in ((0, False), (1, True), (3, True)):
        qp, _, pt = solved({0: FD_FIXTURES["family0"][0], 1: GPU_FIXTURES["family_min"],
                            3: GPU_FIXTURES["family_seed3"]}[seed])
        active = np.isfinite(qp.uvar) & (qp.lvar != qp.uvar) & (pt["zu"] >= 1e-2)
        assert bool(active.any()) == expect, seed


def test_constant_multipliers_have_no_cotangent():
    """zl / zu of a variable without that bound and of a fixed variable are 0 at the reference point, and
    their cotangents change nothing."""
    qp, cot, pt = solved(GPU_FIXTURES["family_seed3"])
    fixed = qp.lvar == qp.uvar
    nol, nou = ~np.isfinite(qp.lvar) | fixed, ~np.isfinite(qp.uvar) | fixed
    assert fixed.any() and (nol & ~fixed).any() and (nou & ~fixed).any()
    assert not np.any(pt["zl"][nol]) and not np.any(pt["zu"][nou])
    other = dict(cot, gzl=np.where(nol, 7.0, cot["gzl"]), gzu=np.where(nou, -7.0, cot["gzu"]))
    for form in ("shifted", "plain"):
        a, b = F.reference_adjoint_full(qp, pt, cot, form), F.reference_adjoint_full(qp, pt, other, form)
        for k in O.NAMES:
            assert np.array_equal(a[k], b[k]), (form, k)


def test_rowlength_fixture_is_what_it_is_for():
    qp, _, pt = solved(F.rowlength_fixture)
    assert 50 <= qp.nvar <= 70 and not np.any(qp.lvar == qp.uvar)
    ra, rh = F.row_lengths(qp)
    assert sorted(set(ra)) == list(F.ROW_LENGTHS) and sorted(set(rh)) == list(F.ROW_LENGTHS)
    eq = qp.lcon == qp.ucon
    assert sorted(set(ra[eq])) == list(F.ROW_LENGTHS)        # the rows of J without a slack entry: every length
    O.check_strict(qp, pt, active=1e-2, inactive=5e-2)
    # row i holds the interior variable i
    A = O.dense(qp).A
    for i in range(qp.ncon):
        assert A[i, i] != 0.0
        assert pt["zl"][i] <= 1e-6 and pt["zu"][i] <= 1e-6
    # active bounds of both sides among the variables, active rows of both signs
    assert (pt["zl"] >= 1e-2).any() and (pt["zu"] >= 1e-2).any()
    assert (pt["y"][~eq] >= 1e-2).any() and (pt["y"][~eq] <= -1e-2).any()


# ------------------------------------------------------------------ argument checks, before any library call
def _bare_solver():
    from madipm_amd import MPCSolver
    s = MPCSolver.__new__(MPCSolver)
    s.qp = O.family(0)[0]
    s._device = None
    s._update_ready = False
    s.h = None                       # no handle: a library call would fail on it; __del__ has nothing to destroy
    return s


def test_full_entry_points_exist():
    import ctypes as C
    from madipm_amd import MPCSolver, _lib as L
    from madipm_amd import solver  # noqa: F401
    import inspect
    for name in ("madipm_solver_adjoint_full", "madipm_solver_adjoint_full_device"):
        f = getattr(L.lib, name)
        assert f.argtypes is not None and f.restype is C.c_int, name
    assert [k for k, _ in L.QPCot._fields_] == ["x", "y", "zl", "zu", "cons"]
    for meth in (MPCSolver.adjoint, MPCSolver.adjoint_device):
        p = inspect.signature(meth).parameters
        assert list(p)[:3] == ["self", "gx", "want"]
        for k in ("gy", "gzl", "gzu", "gcons"):
            assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None, k
    assert L.madipm_version() == 203       # additive: the version number of the 0.2 line stays


def test_cotangent_checks():
    from madipm_amd.solver import COTANGENT_NAMES, check_adjoint_cotangents
    n, m = 7, 5
    out = check_adjoint_cotangents(n, m, gcons=[1.0] * m, gx=np.ones(n, np.float32))
    assert list(out) == ["x", "cons"] and COTANGENT_NAMES == ("x", "y", "zl", "zu", "cons")
    assert all(a.dtype == np.float64 and a.flags.c_contiguous for a in out.values())
    assert list(check_adjoint_cotangents(n, m, None, np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(m))) == \
        ["y", "zl", "zu", "cons"]
    with pytest.raises(ValueError, match="no cotangent given"):
        check_adjoint_cotangents(n, m)
    for k, bad in (("gx", m), ("gy", n), ("gzl", m), ("gzu", m), ("gcons", n)):
        with pytest.raises(ValueError, match=f"adjoint: {k} has shape"):
            check_adjoint_cotangents(n, m, **{k: np.zeros(bad)})
    with pytest.raises(ValueError, match="gy has shape"):
        check_adjoint_cotangents(n, m, gx=np.zeros(n), gy=np.zeros((m, 1)))


def test_adjoint_argument_errors_come_before_the_library():
    import torch
    s = _bare_solver()
    n, m = s.qp.nvar, s.qp.ncon
    with pytest.raises(ValueError, match="no cotangent given"):
        s.adjoint()
    with pytest.raises(ValueError, match="no cotangent given"):
        s.adjoint_device()
    with pytest.raises(ValueError, match="gy has shape"):
        s.adjoint(np.zeros(n), gy=np.zeros(m + 1))
    with pytest.raises(ValueError, match="gzu has shape"):
        s.adjoint(gzu=np.zeros(m))
    with pytest.raises(ValueError, match="unknown name"):
        s.adjoint(gy=np.zeros(m), want=["y"])
    with pytest.raises(TypeError, match="gy must be a torch tensor"):
        s.adjoint_device(gy=np.zeros(m))                                       # a numpy array
    with pytest.raises(TypeError, match="gcons is on cpu"):
        s.adjoint_device(gcons=torch.zeros(m, dtype=torch.float64))            # a CPU tensor
    with pytest.raises(TypeError, match="gzl has dtype"):
        s.adjoint_device(gzl=torch.zeros(n, dtype=torch.float32))
    with pytest.raises(ValueError, match="gzu is not contiguous"):
        s.adjoint_device(gzu=torch.zeros(2 * n, dtype=torch.float64)[::2])
    with pytest.raises(TypeError):
        s.adjoint_device(torch.zeros(n, dtype=torch.float64, device="meta"), gy=torch.zeros(m, dtype=torch.float64))


def test_device_shapes_are_checked():
    """As test_adjoint_cpu.test_wrong_shape_is_reported_as_such: the shape test comes after the device's, so it
    needs a tensor that passes for a GPU tensor."""
    import torch
    from madipm_amd.solver import check_adjoint_cotangents

    class OnGpu(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    t = lambda k: torch.zeros(k, dtype=torch.float64).as_subclass(OnGpu)  # noqa: E731
    good = check_adjoint_cotangents(7, 5, gy=t(5), gzl=t(7), on_device=True, who="adjoint_device")
    assert list(good) == ["y", "zl"]
    with pytest.raises(ValueError, match="adjoint_device: gcons has shape"):
        check_adjoint_cotangents(7, 5, gy=t(5), gcons=t(7), on_device=True, who="adjoint_device")
    with pytest.raises(TypeError, match="the solver is on"):
        check_adjoint_cotangents(7, 5, gy=t(5), on_device=True, device=torch.device("cuda", 1), who="adjoint_device")


def test_layer_outputs_are_checked():
    from madipm_amd.solver import check_layer_outputs
    assert check_layer_outputs(("x",)) == ("x",)
    assert check_layer_outputs(["cons", "x", "zu"]) == ("cons", "x", "zu")       # the caller's order is kept
    with pytest.raises(ValueError, match="unknown name"):
        check_layer_outputs(("x", "s"))
    with pytest.raises(ValueError, match="repeated"):
        check_layer_outputs(("y", "y"))
    with pytest.raises(ValueError, match="empty"):
        check_layer_outputs(())
    with pytest.raises(TypeError):
        check_layer_outputs("x")
    from madipm_amd import QPLayer
    with pytest.raises(ValueError, match="unknown name"):
        QPLayer(None, outputs=("x", "multipliers"))
    assert QPLayer(None).outputs == ("x",) and QPLayer(None, outputs=["y", "x"]).outputs == ("y", "x")
