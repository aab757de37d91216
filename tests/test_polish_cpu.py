"""The oracle of the polish (polish_oracle.py) on the adjoint oracle's fixtures, from the
interior-point end point reference_ipm(mu_end=1e-9): the guessed set against the construction's, the delta-form
solves against a dense solve of the exact reduced system, the residual history, the gain over the interior
point, the three failure modes, and the argument checks of MPCSolver.polish / polish_device — all without a
GPU."""
from __future__ import annotations

import numpy as np
import pytest

import adjoint_oracle as O
import polish_oracle as P

MU_IPM = 1e-9            # the end point the solver returns sits at about this mu

# name -> (problem, the construction's pattern or None: read from the reference optimum)
FIXTURES = {
    "family_0": (lambda: O.family(0)[0], lambda qp: P.family_pattern(qp, 0)),
    "family_1": (lambda: O.family(1)[0], lambda qp: P.family_pattern(qp, 1)),
    "family_2": (lambda: O.family(2)[0], lambda qp: P.family_pattern(qp, 2)),
    "family_3": (lambda: O.family(3)[0], lambda qp: P.family_pattern(qp, 3)),
    "family_0_max": (lambda: O.family(0, minimize=False)[0], lambda qp: P.family_pattern(qp, 0)),
    "scaled": (lambda: O.scaled_family(0)[0], lambda qp: P.family_pattern(qp, 0)),
    "duplicated": (lambda: O.duplicated_family(0)[0], lambda qp: P.family_pattern(qp, 0)),
    "lp": (lambda: O.lp_fixture()[0], P.lp_pattern),
    "sparse": (lambda: O.sparse_fixture()[0], None),
}
_solved = {}


def solved(name):
    """(qp, interior point, pattern, polished, exact), computed once and never modified."""
    if name not in _solved:
        make, pattern = FIXTURES[name]
        qp = make()
        pt = O.reference_ipm(qp, mu_end=MU_IPM)
        pat = pattern(qp) if pattern else P.strict_pattern(qp, O.reference_ipm(qp))
        _solved[name] = (qp, pt, pat, P.polish(qp, pt), P.exact(qp, *pat))
    return _solved[name]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_guess_is_the_constructions_pattern(name):
    qp, pt, pat, pol, _ = solved(name)
    av, ar = P.guess(qp, pt)
    assert np.array_equal(av, pat[0]) and np.array_equal(ar, pat[1])
    assert np.array_equal(pol["active_var"], pat[0]) and np.array_equal(pol["active_row"], pat[1])
    assert pol["n_active"] == int(np.count_nonzero(pat[0]) + np.count_nonzero(pat[1]))
    if name == "sparse":
        assert pol["n_active"] == 180


@pytest.mark.parametrize("name", list(FIXTURES))
def test_polished_point_is_the_exact_solve(name):
    qp, pt, pat, pol, ex = solved(name)
    assert pol["verdict"] == P.POLISHED, pol["verdict"]
    e = {k: P.err(pol[k], ex[k]) for k in ("x", "y", "zl", "zu", "cons")}
    print("polish vs exact", name, {k: f"{v:.1e}" for k, v in e.items()}, "history",
          [f"{h:.1e}" for h in pol["history"]])
    assert max(e.values()) <= 1e-13, e
    assert all(h <= 1e-13 for h in pol["history"][1:]), pol["history"]
    assert pol["residual"] == pol["history"][-1]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_polished_point_is_much_nearer_than_the_interior_point(name):
    qp, pt, pat, pol, ex = solved(name)
    d_ipm, d_pol = P.distance(pt, ex), P.distance(pol, ex)
    print("distance to the exact solution", name, f"interior {d_ipm:.1e} polished {d_pol:.1e}")
    if d_ipm > 1e-9:
        assert d_pol <= 1e-3 * d_ipm
    else:
        assert name == "scaled"          # starts at 7e-13: 1e3 c, H put the central path that much nearer


@pytest.mark.parametrize("name", list(FIXTURES))
def test_exact_properties(name):
    qp, pt, pat, pol, _ = solved(name)
    av, ar = pol["active_var"], pol["active_row"]
    assert np.array_equal(pol["x"][av < 0], qp.lvar[av < 0]) and np.array_equal(pol["x"][av > 0], qp.uvar[av > 0])
    assert not np.any(pol["zl"][av >= 0]) and not np.any(pol["zu"][av <= 0])
    assert np.array_equal(pol["cons"][ar < 0], qp.lcon[ar < 0]) and np.array_equal(pol["cons"][ar > 0], qp.ucon[ar > 0])


@pytest.mark.parametrize("sigma", [1e8, 1e10, 1e12])
def test_sigma_does_not_matter(sigma):
    qp, pt, pat, pol, ex = solved("family_0")
    q = P.polish(qp, pt, sigma=sigma)
    assert q["verdict"] == P.POLISHED and P.distance(q, ex) <= 1e-13


def failure_cases():
    """name -> (qp, interior point, supplied set): the three failure modes."""
    qp, pt, pat, _, _ = solved("family_0")
    forced = (pat[0].copy(), pat[1].copy())
    forced[0][1] = 1                                   # variable 1's inactive upper bound
    empty = (np.zeros(qp.nvar, np.int8), np.zeros(qp.ncon, np.int8))
    lp, lpt, lpat, _, _ = solved("lp")
    four = (lpat[0].copy(), lpat[1].copy())
    four[0][3] = -1                                    # a fourth variable at a bound under three equality rows
    return {"forced_upper": (qp, pt, forced), "empty": (qp, pt, empty), "lp_four": (lp, lpt, four)}


def test_failure_modes():
    c = failure_cases()
    a = P.polish(*c["forced_upper"][:2], *c["forced_upper"][2])
    print("forced upper", a["verdict"], a["min_multiplier"], a["residual"])
    assert a["verdict"] == P.WRONG_SET and abs(a["min_multiplier"] + 1.03) <= 0.01 and a["residual"] <= 1e-13
    b = P.polish(*c["empty"][:2], *c["empty"][2])
    print("empty set", b["verdict"], b["min_gap"], b["residual"])
    assert b["verdict"] == P.WRONG_SET and abs(b["min_gap"] + 0.13) <= 0.01 and b["residual"] <= 1e-13
    d = P.polish(*c["lp_four"][:2], *c["lp_four"][2])
    print("lp, four active", d["verdict"], d["residual"], d["history"])
    assert d["verdict"] == P.NO_CONVERGENCE and not d["residual"] <= 1e-3
    # a wrong but consistent set converges in two solves: the first leaves the penalty's 1 / sigma
    assert a["history"][1] <= 1e-7 and a["history"][2] <= 1e-13


def test_refused_codes():
    qp, pt, pat, _, _ = solved("family_0")
    for var, row in ((0, None), (3, None), (None, 0), (None, 2)):
        av, ar = pat[0].copy(), pat[1].copy()
        if var is not None:
            av[var] = 1          # variable 0 has no upper bound, variable 3 is fixed
        else:
            ar[row] = 1          # row 0 is an equality, row 2 has no upper side
        with pytest.raises(ValueError):
            P.polish(qp, pt, av, ar)


# ------------------------------------------------------------------ the argument checks and the C interface
def test_abi():
    import ctypes as C
    from madipm_amd import _lib as L
    assert L.madipm_version() == 203       # additive: the version number of the 0.2 line stays
    for f in ("madipm_polish_default_opts", "madipm_solver_polish", "madipm_solver_polish_device",
              "madipm_solver_polish_info"):
        assert hasattr(L.lib, f), f
    o = L.PolishOpts()
    L.lib.madipm_polish_default_opts(C.byref(o))
    assert (o.sigma, o.tol_resid, o.tol_sign, o.tol_feas, o.refine_steps) == (1e10, 1e-10, 1e-9, 1e-9, 2)
    assert (P.SIGMA, P.TOL_RESID, P.TOL_SIGN, P.TOL_FEAS, P.REFINE_STEPS) == (1e10, 1e-10, 1e-9, 1e-9, 2)
    assert C.sizeof(L.PolishOpts) == 40 and C.sizeof(L.PolishOut) == 56 and C.sizeof(L.PolishInfo) == 48
    out = L.PolishOut()
    assert L.lib.madipm_solver_polish(None, None, None, None, C.byref(out), None) < 0
    assert b"null handle" in L.madipm_last_error()


def test_argument_checks():
    from madipm_amd import POLISH_NAMES, PolishVerdict
    from madipm_amd.solver import check_polish_opts, check_polish_set, check_polish_want
    assert POLISH_NAMES == ("x", "y", "zl", "zu", "cons", "active_var", "active_row")
    assert [int(v) for v in PolishVerdict] == [0, 1, 2, 3] and PolishVerdict.NO_CONVERGENCE == P.NO_CONVERGENCE
    assert check_polish_want(None) == POLISH_NAMES and check_polish_want(["cons", "x"]) == ("x", "cons")
    with pytest.raises(TypeError, match="not the string"):
        check_polish_want("x")
    with pytest.raises(ValueError, match="unknown name"):
        check_polish_want(["x", "s"])
    with pytest.raises(ValueError, match="want is empty"):
        check_polish_want([])
    assert check_polish_opts() == (1e10, 1e-10, 1e-9, 1e-9, 2)
    assert check_polish_opts(1e8, 0.0, 1e-6, 1e-7, 8) == (1e8, 0.0, 1e-6, 1e-7, 8)
    for kw in (dict(sigma=0.0), dict(sigma=np.inf), dict(tol_resid=-1.0), dict(tol_sign=np.nan), dict(tol_feas=np.inf),
               dict(refine_steps=-1), dict(refine_steps=9)):
        with pytest.raises(ValueError):
            check_polish_opts(**kw)
    with pytest.raises(TypeError, match="refine_steps must be an integer"):
        check_polish_opts(refine_steps=2.0)
    assert check_polish_set(7, 5) == ()
    av, ar = check_polish_set(7, 5, [0, 1, -1, 0, 0, 0, 0], np.zeros(5, np.int64))
    assert av.dtype == ar.dtype == np.int8 and av.flags.c_contiguous and list(av[:3]) == [0, 1, -1]
    with pytest.raises(ValueError, match="go together"):
        check_polish_set(7, 5, np.zeros(7, np.int8))
    with pytest.raises(ValueError, match="go together"):
        check_polish_set(7, 5, None, np.zeros(5, np.int8))
    with pytest.raises(ValueError, match="shape"):
        check_polish_set(7, 5, np.zeros(6, np.int8), np.zeros(5, np.int8))
    with pytest.raises(TypeError, match="expected integers"):
        check_polish_set(7, 5, np.zeros(7), np.zeros(5, np.int8))
    with pytest.raises(ValueError, match="does not fit int8"):
        check_polish_set(7, 5, np.full(7, 300), np.zeros(5, np.int8))


def test_device_set_checks():
    torch = pytest.importorskip("torch")
    from madipm_amd.solver import check_polish_set
    with pytest.raises(TypeError, match="must be a torch tensor"):
        check_polish_set(7, 5, np.zeros(7, np.int8), np.zeros(5, np.int8), on_device=True)
    with pytest.raises(TypeError, match="expected torch.int8"):
        check_polish_set(7, 5, torch.zeros(7), torch.zeros(5, dtype=torch.int8), on_device=True)
    with pytest.raises(TypeError, match="expected a GPU tensor"):
        check_polish_set(7, 5, torch.zeros(7, dtype=torch.int8), torch.zeros(5, dtype=torch.int8), on_device=True)
    with pytest.raises(ValueError, match="not contiguous"):
        check_polish_set(7, 5, torch.zeros(14, dtype=torch.int8)[::2], torch.zeros(5, dtype=torch.int8), on_device=True)
