"""The adjoint oracle against finite differences, the conditions its fixtures must meet, and the argument
checks of MPCSolver.adjoint_device — all without a GPU."""
from __future__ import annotations

import numpy as np
import pytest

import adjoint_oracle as O

FD_TOL = 1e-8        # absolute, gradients of size 0.1 - 3 (measured: 8.2e-10 over the four seeds)


@pytest.fixture(scope="module")
def solved():
    """seed -> (qp, gx, point, gradients, terms) of the minimize family at its reference optimum."""
    out = {}
    for seed in O.FAMILY_SEEDS:
        qp, gx = O.family(seed)
        pt = O.reference_ipm(qp)
        g, t = O.reference_adjoint(qp, pt, gx, terms=True)
        out[seed] = (qp, gx, pt, g, t)
    return out


@pytest.mark.parametrize("seed", O.FAMILY_SEEDS)
def test_oracle_matches_central_differences(solved, seed):
    qp, gx, _, g, _ = solved[seed]
    fd = O.finite_difference(qp, gx, h=1e-6)
    worst = {k: float(np.max(np.abs(fd[k] - g[k]))) for k in O.NAMES}
    print(seed, worst)
    assert max(worst.values()) <= FD_TOL, worst


def test_family_is_what_the_issue_describes(solved):
    qp = solved[0][0]
    assert (qp.nvar, qp.ncon) == (7, 5)
    fixed = qp.lvar == qp.uvar
    assert fixed.sum() == 1 and (np.isfinite(qp.lvar) & np.isfinite(qp.uvar) & ~fixed).sum() == 1   # fixed, boxed
    assert (np.isfinite(qp.lvar) ^ np.isfinite(qp.uvar)).sum() == 2                                 # two bounded
    eq = qp.lcon == qp.ucon
    assert eq.sum() == 2 and (np.isfinite(qp.lcon) ^ np.isfinite(qp.ucon)).sum() == 2               # one-sided rows
    assert (np.isfinite(qp.lcon) & np.isfinite(qp.ucon) & ~eq).sum() == 1                           # ranged


def test_fixtures_are_strictly_complementary(solved):
    for seed in O.FAMILY_SEEDS:
        qp, _, pt, _, _ = solved[seed]
        O.check_strict(qp, pt, active=1e-2, inactive=5e-2)
        qm, _ = O.family(seed, minimize=False)
        pm = O.reference_ipm(qm)
        O.check_strict(qm, pm, active=1e-2, inactive=5e-2)
        assert np.max(np.abs(pm["x"] - pt["x"])) <= 1e-8       # the maximised negated objective: the same x*
    for make in (lambda: O.scaled_family(1), O.lp_fixture):
        qp = make()[0]
        O.check_strict(qp, O.reference_ipm(qp), active=1e-2, inactive=5e-2)


def test_every_block_and_every_term_is_visible(solved):
    """On at least one fixture each block has an entry >= 1e-2 of the largest gradient entry, and on such a
    fixture each single term of its formula is >= 1e-2 of the block's scale: a dropped term cannot hide
    under a tolerance of 1e-4."""
    nterms = {k: len(solved[0][4][k]) for k in O.NAMES}
    block_ok = {k: False for k in O.NAMES}
    term_ok = {(k, j): False for k in O.NAMES for j in range(nterms[k])}
    for seed in O.FAMILY_SEEDS:
        _, _, _, g, t = solved[seed]
        top = max(np.max(np.abs(v)) for v in g.values())
        for k in O.NAMES:
            scale = np.max(np.abs(g[k]))
            if scale < 1e-2 * top:
                continue
            block_ok[k] = True
            for j, term in enumerate(t[k]):
                if np.max(np.abs(term)) >= 1e-2 * scale:
                    term_ok[(k, j)] = True
    assert all(block_ok.values()), block_ok
    assert all(term_ok.values()), term_ok


def test_duplicated_entries_describe_the_same_problem():
    qp, gx, hk, ak = O.duplicated_family(1)
    base, _ = O.family(1)
    assert qp.nnzh == base.nnzh + len(hk) and qp.nnzj == base.nnzj + len(ak)
    a, b = O.dense(qp), O.dense(base)
    assert np.allclose(a.H, b.H, rtol=0, atol=1e-15) and np.allclose(a.A, b.A, rtol=0, atol=1e-15)
    pt = O.reference_ipm(base)
    g, gb = O.reference_adjoint(qp, pt, gx), O.reference_adjoint(base, pt, gx)
    assert np.allclose(g["Hvals"][base.nnzh:], gb["Hvals"][hk], rtol=0, atol=1e-13)   # each copy: the full value
    assert np.allclose(g["Hvals"][hk], gb["Hvals"][hk], rtol=0, atol=1e-13)
    assert np.allclose(g["Avals"][base.nnzj:], gb["Avals"][ak], rtol=0, atol=1e-13)


# ------------------------------------------------------------------ argument checks, before any library call
def _bare_solver():
    from madipm_amd import MPCSolver
    s = MPCSolver.__new__(MPCSolver)
    s.qp = O.family(0)[0]
    s._device = None
    s._update_ready = False
    s.h = None                       # no handle: a library call would fail on it; __del__ has nothing to destroy
    return s


def test_adjoint_entry_points_exist():
    from madipm_amd import MPCSolver, _lib as L
    from madipm_amd import solver  # noqa: F401
    for name in ("adjoint", "adjoint_device", "adjoint_info"):
        assert callable(getattr(MPCSolver, name)), name
    for name in ("madipm_solver_adjoint", "madipm_solver_adjoint_device", "madipm_solver_adjoint_info"):
        f = getattr(L.lib, name)
        assert f.argtypes is not None and f.restype is not None, name
    assert L.madipm_version() == 203


def test_adjoint_device_argument_errors():
    import torch
    s = _bare_solver()
    n = s.qp.nvar
    with pytest.raises(TypeError):
        s.adjoint_device(np.zeros(n))                                      # a numpy array
    with pytest.raises(TypeError):
        s.adjoint_device(torch.zeros(n, dtype=torch.float64))              # a CPU tensor
    with pytest.raises(TypeError):
        s.adjoint_device(torch.zeros(n, dtype=torch.float32))              # wrong dtype
    with pytest.raises(ValueError):
        s.adjoint_device(torch.zeros(2 * n, dtype=torch.float64)[::2])     # not contiguous
    with pytest.raises(ValueError, match="unknown name"):
        s.adjoint_device(torch.zeros(n, dtype=torch.float64), want=["c", "x0"])
    with pytest.raises(ValueError, match="unknown name"):
        s.adjoint(np.zeros(n), want=["Hval"])
    with pytest.raises(ValueError, match="shape"):
        s.adjoint(np.zeros(n + 1))
    with pytest.raises(ValueError):
        s.adjoint(np.zeros(n), want=[])
    with pytest.raises(TypeError):
        s.adjoint(np.zeros(n), want="c")


def test_wrong_shape_is_reported_as_such():
    """check_device_array tests the shape after the device, so the wrong-shape case needs a tensor that
    passes for a GPU tensor: the check itself, with the shape it is given."""
    import torch
    from madipm_amd.solver import check_device_array

    class OnGpu(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    t = torch.zeros(5, dtype=torch.float64).as_subclass(OnGpu)
    with pytest.raises(ValueError, match="adjoint_device: gx has shape"):
        check_device_array("gx", t, 7, who="adjoint_device")
    assert check_device_array("gx", t, 5, who="adjoint_device") is t


def test_want_is_normalised():
    from madipm_amd.solver import ADJOINT_NAMES, check_adjoint_want
    assert check_adjoint_want(None) == ADJOINT_NAMES == O.NAMES
    assert check_adjoint_want(["uvar", "c"]) == ("c", "uvar")
    assert check_adjoint_want({"Avals"}) == ("Avals",)
