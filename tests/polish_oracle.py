"""A CPU oracle for MPCSolver.polish: the active-set guess, the projection, the delta-form solves
of the reduced system with the penalised dense factor as a preconditioner, the multipliers and the verdict,
restated with numpy in the public space; and a dense solve of the exact reduced system.  No GPU, no library
call.  Notation and fixtures are adjoint_oracle.py's: v = [x_F; s] with s = (A x)_I, W = diag(sgn H_FF, 0),
J = [A_:F, -E], the multipliers of a row are zl_s = max(-y, 0), zu_s = max(y, 0)."""
from __future__ import annotations

import dataclasses

import numpy as np

import adjoint_oracle as O

POLISHED, WRONG_SET, NO_CONVERGENCE, FACTORIZATION_FAILED = 0, 1, 2, 3
SIGMA, TOL_RESID, TOL_SIGN, TOL_FEAS, REFINE_STEPS = 1e10, 1e-10, 1e-9, 1e-9, 2
DELTA_W, DELTA_C = 1e-8, -1e-8       # the regularisation of the GPU tests' solver options


@dataclasses.dataclass
class Space:
    D: O.Dense
    nf: int
    ns: int
    lo: np.ndarray          # bounds of v
    hi: np.ndarray
    lb: np.ndarray          # bool: the bound exists
    ub: np.ndarray
    W: np.ndarray
    J: np.ndarray
    g: np.ndarray
    b: np.ndarray
    xfix: np.ndarray        # x with the fixed variables at their value, 0 elsewhere


def space(qp) -> Space:
    D = O.dense(qp)
    F, I = D.F, D.I
    nf, ns = len(F), len(I)
    lvar, uvar = np.asarray(qp.lvar, float), np.asarray(qp.uvar, float)
    lcon, ucon = np.asarray(qp.lcon, float), np.asarray(qp.ucon, float)
    lo, hi = np.concatenate([lvar[F], lcon[I]]), np.concatenate([uvar[F], ucon[I]])
    xfix = np.where(D.fixed, lvar, 0.0)
    E = np.zeros((D.m, ns))
    E[I, np.arange(ns)] = 1.0
    W = np.zeros((nf + ns, nf + ns))
    W[:nf, :nf] = D.sgn * D.H[np.ix_(F, F)]
    J = np.hstack([D.A[:, F], -E])
    g = np.concatenate([D.sgn * (np.asarray(qp.c, float) + D.H @ xfix)[F], np.zeros(ns)])
    b = np.where(D.eq, lcon, 0.0) - D.A @ xfix
    return Space(D, nf, ns, lo, hi, np.isfinite(lo), np.isfinite(hi), W, J, g, b, xfix)


def scaling(qp, bound_relax=1e-12, bound_push=1e-2, bound_fac=1e-2):
    """(obj_scale, con_scale) as the solver's set_scaling! gives them with its default options: obj_scale =
    min(1, 100 / |sgn (c + H x)|_inf) at the start x (x0, the fixed variables at their value, pushed inside the
    relaxed bounds), con_scale_i = min(1, 100 / max_j |A_ij|)."""
    D = O.dense(qp)
    lvar, uvar = np.asarray(qp.lvar, float), np.asarray(qp.uvar, float)
    x0 = getattr(qp, "x0", None)
    x = np.zeros(D.n) if x0 is None else np.array(x0, float)
    x[D.fixed] = lvar[D.fixed]
    for i in np.flatnonzero(~D.fixed):
        l, u = lvar[i], uvar[i]
        if np.isfinite(l):
            l -= bound_relax * max(1.0, abs(l))
        if np.isfinite(u):
            u += bound_relax * max(1.0, abs(u))
        lo, hi = -np.inf, np.inf
        if np.isfinite(l):
            lo = l + (min(bound_push * max(1.0, abs(l)), bound_fac * (u - l)) if np.isfinite(u)
                      else bound_push * max(1.0, abs(l)))
        if np.isfinite(u):
            hi = u - (min(bound_push * max(1.0, abs(u)), bound_fac * (u - l)) if np.isfinite(l)
                      else bound_push * max(1.0, abs(u)))
        x[i] = min(max(x[i], lo), hi)
    gmax = float(np.max(np.abs(np.asarray(qp.c, float) + D.H @ x), initial=0.0))
    os_ = min(1.0, 100.0 / gmax) if gmax > 0 else 1.0
    rowmax = np.zeros(D.m)
    np.maximum.at(rowmax, np.asarray(qp.Arows, int), np.abs(np.asarray(qp.Avals, float)))
    with np.errstate(divide="ignore"):
        cs = np.minimum(1.0, 100.0 / rowmax)
    return os_, cs


def _to_v(S: Space, point):
    """(v, y, zl_v, zu_v) of a public point (x, y, zl, zu)."""
    D = S.D
    x, y = np.asarray(point["x"], float), np.asarray(point["y"], float)
    v = np.concatenate([x[D.F], (D.A @ x)[D.I]])
    zl = np.concatenate([np.asarray(point["zl"], float)[D.F], np.maximum(-y[D.I], 0.0)])
    zu = np.concatenate([np.asarray(point["zu"], float)[D.F], np.maximum(y[D.I], 0.0)])
    return v, y.copy(), zl, zu


def _codes_of(S: Space, active_var, active_row):
    """The codes of v from one int8 per variable and one per row; ValueError for a code the library refuses."""
    D = S.D
    av, ar = np.asarray(active_var, int), np.asarray(active_row, int)
    if av.shape != (D.n,) or ar.shape != (D.m,):
        raise ValueError("shape")
    if np.any(av[D.fixed] != 0) or np.any(ar[D.eq] != 0):
        raise ValueError("a code on a fixed variable or an equality row")
    c = np.concatenate([av[D.F], ar[D.I]])
    if np.any((c != 0) & (c != 1) & (c != -1)) or np.any((c == -1) & ~S.lb) or np.any((c == 1) & ~S.ub):
        raise ValueError("a code on a bound that does not exist")
    return c


def _codes_out(S: Space, c):
    D = S.D
    av, ar = np.zeros(D.n, np.int8), np.zeros(D.m, np.int8)
    av[D.F], ar[D.I] = c[:S.nf], c[S.nf:]
    return av, ar


def guess(qp, point):
    """Step 1: (active_var, active_row) at a public point: lower-active when zl > v - lo, upper-active when
    zu > hi - v; both: the larger multiplier, lower on a tie."""
    S = space(qp)
    v, _, zl, zu = _to_v(S, point)
    with np.errstate(invalid="ignore"):
        la = S.lb & (zl > v - S.lo)
        ua = S.ub & (zu > S.hi - v)
    c = np.where(la & ua, np.where(zu > zl, 1, -1), np.where(la, -1, np.where(ua, 1, 0)))
    return _codes_out(S, c)


def _pack(S: Space, c, v, y):
    """The public blocks of (v, y) with the set c: x, y, zl, zu, cons."""
    D = S.D
    t = S.g + S.W @ v + S.J.T @ y
    zlv, zuv = np.where(c < 0, t, 0.0), np.where(c > 0, -t, 0.0)
    x = S.xfix.copy()
    x[D.F] = v[:S.nf]
    zl, zu = np.zeros(D.n), np.zeros(D.n)
    zl[D.F], zu[D.F] = zlv[:S.nf], zuv[:S.nf]
    cons = D.A @ x
    cs = c[S.nf:]
    cons[D.I] = np.where(cs < 0, S.lo[S.nf:], np.where(cs > 0, S.hi[S.nf:], cons[D.I]))
    return dict(x=x, y=y.copy(), zl=zl, zu=zu, cons=cons), zlv, zuv


def _lu(K):
    try:
        import scipy.linalg as sl
        f = sl.lu_factor(K)
        return lambda r: sl.lu_solve(f, r)
    except ImportError:
        return lambda r: np.linalg.solve(K, r)


def polish(qp, point, active_var=None, active_row=None, sigma=SIGMA, refine_steps=REFINE_STEPS, tol_resid=TOL_RESID,
           tol_sign=TOL_SIGN, tol_feas=TOL_FEAS, delta_w=DELTA_W, delta_c=DELTA_C):
    """Steps 1-6 at a public point.  Returns a dict: the polished blocks x, y, zl, zu, cons (whatever the
    verdict), active_var, active_row, verdict, residual, min_multiplier, min_gap, n_active, and history: the
    max-norm of the exact reduced residual, in the solver's scaled space, before each solve and at the final
    point."""
    S = space(qp)
    if active_var is None:
        active_var, active_row = guess(qp, point)
    c = _codes_of(S, active_var, active_row)
    act = c != 0
    v, y, _, _ = _to_v(S, point)
    v = np.where(c < 0, S.lo, np.where(c > 0, S.hi, v))                 # step 2
    nv, m = S.nf + S.ns, S.D.m
    K = np.block([[S.W + np.diag(delta_w + np.where(act, sigma, 0.0)), S.J.T], [S.J, delta_c * np.eye(m)]])  # step 4
    verdict = POLISHED
    try:
        solve = _lu(K)
    except Exception:            # a singular penalised matrix
        solve, verdict = None, FACTORIZATION_FAILED

    os_, cs = scaling(qp)
    scale = np.concatenate([np.full(S.nf, os_), os_ / cs[S.D.I], cs])   # the residual's rows in the scaled space

    def resid(v, y):
        r1 = -(S.g + S.W @ v + S.J.T @ y)
        r1[act] = 0.0
        return np.concatenate([r1, -(S.J @ v - S.b)])

    hist = []
    if solve is not None:
        for _ in range(refine_steps + 1):                                # step 3
            r = resid(v, y)
            hist.append(float(np.max(np.abs(scale * r), initial=0.0)))
            with np.errstate(all="ignore"):
                d = solve(r)
            d[:nv][act] = 0.0
            v, y = v + d[:nv], y + d[nv:]
    with np.errstate(all="ignore"):
        r = resid(v, y)
        res = float(np.max(np.abs(scale * r), initial=0.0)) if np.all(np.isfinite(r)) else float("nan")
        hist.append(res)
        out, zlv, zuv = _pack(S, c, v, y)                                # step 5
        mult = np.concatenate([zlv[c < 0], zuv[c > 0]])
        min_mult = float(np.min(mult, initial=np.inf))
        max_abs = float(np.max(np.abs(mult), initial=0.0))
        gl = ((v - S.lo) / np.maximum(1.0, np.abs(S.lo)))[S.lb & (c != -1)]
        gu = ((S.hi - v) / np.maximum(1.0, np.abs(S.hi)))[S.ub & (c != 1)]
        rel_gap = float(np.min(np.concatenate([gl, gu]), initial=np.inf))
        min_gap = float(np.min(np.concatenate([(v - S.lo)[S.lb & (c != -1)], (S.hi - v)[S.ub & (c != 1)]]),
                               initial=np.inf))
    if min_mult < -tol_sign * max(1.0, max_abs) or rel_gap < -tol_feas:   # step 6
        verdict = max(verdict, WRONG_SET)
    if not res <= tol_resid:
        verdict = max(verdict, NO_CONVERGENCE)
    av, ar = _codes_out(S, c)
    out.update(active_var=av, active_row=ar, verdict=verdict, residual=res, min_multiplier=min_mult, min_gap=min_gap,
               n_active=int(act.sum()), history=hist)
    return out


def exact(qp, active_var, active_row):
    """A dense solve of the exact reduced system on the given set: the public blocks x, y, zl, zu, cons."""
    S = space(qp)
    c = _codes_of(S, active_var, active_row)
    act = c != 0
    N = np.flatnonzero(~act)
    nv, m = S.nf + S.ns, S.D.m
    v = np.where(c < 0, S.lo, np.where(c > 0, S.hi, 0.0))
    K = np.block([[S.W[np.ix_(N, N)], S.J[:, N].T], [S.J[:, N], np.zeros((m, m))]])
    rhs = np.concatenate([-(S.g + S.W @ v)[N], S.b - S.J @ v])
    sol = np.linalg.solve(K, rhs)
    r = rhs - K @ sol                    # one step of refinement: the reference is at rounding level itself
    sol = sol + np.linalg.solve(K, r)
    v[N] = sol[:len(N)]
    assert nv == len(v)
    return _pack(S, c, v, sol[len(N):])[0]


def err(a, ref):
    return O.err(a, ref)


def distance(a, ref, keys=("x", "y", "zl", "zu")):
    """The largest err over the blocks."""
    return max(err(a[k], ref[k]) for k in keys)


# ------------------------------------------------------------------ the construction's patterns
def family_pattern(qp, seed):
    """(active_var, active_row) of family(seed) and its variants, from PATTERNS."""
    pat = O.PATTERNS[seed % 4]
    av, ar = np.zeros(qp.nvar, np.int8), np.zeros(qp.ncon, np.int8)
    av[list(pat["var_l"])], av[list(pat["var_u"])] = -1, 1
    ar[list(pat["row_l"])], ar[list(pat["row_u"])] = -1, 1
    return av, ar


def lp_pattern(qp):
    """lp_fixture: variables 0 and 2 at 0, variable 1 at 2."""
    av = np.zeros(qp.nvar, np.int8)
    av[[0, 2]], av[1] = -1, 1
    return av, np.zeros(qp.ncon, np.int8)


def strict_pattern(qp, point, near=1e-6):
    """The set a strictly complementary construction put at its optimum, read from a point within `near` of
    that optimum: a bound closer than `near` is one the construction made active (the inactive ones are 0.1 and
    more away: check_strict)."""
    O.check_strict(qp, point)
    S = space(qp)
    v = _to_v(S, point)[0]
    with np.errstate(invalid="ignore"):
        c = np.where(S.lb & (v - S.lo <= near), -1, np.where(S.ub & (S.hi - v <= near), 1, 0))
    return _codes_out(S, c)
