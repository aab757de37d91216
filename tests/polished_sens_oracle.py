"""A CPU oracle for the sensitivities at the polished point (MPCSolver.tangent / adjoint with polished=True,
DESIGN §13g): the derivatives of the equality-constrained QP of the face an active set defines, with numpy in
the public space.  No GPU, no library call.  Notation is polish_oracle.py's: v = [x_F; s], W = diag(sgn H_FF, 0),
J = [A_:F, -E], K0 = [[W, J'], [J, 0]] (no Sigma, no regularisation), the set's codes split v into active A and
inactive N; w = [v; y] is polish_oracle.exact's point, t = g + W v + J'y, zl = t on a lower-active coordinate,
zu = -t on an upper-active one.  The conventions of what is read are tangent_oracle's.

    tangent   dw_A = dbound_A;  M dz = -dD_N - K0_NA dbound_A  (M = K0 on (N + rows)^2, dz = [dv_N; dy]);
              dt_A = dD_A + (K0 dw)_A;   dD = [sgn (dc + dH x + H dxfix)_F + (dA'y)_F; 0; dA x + A dxfix - db]
    adjoint   ghat = [gx_F; gcons_I; gy] (cons_r = s_r on an inequality row, lcon_r on an equality row);
              taubar = gzl on a lower-active variable, -gzu on an upper-active one;  h = ghat + K0 taubar;
              M a = h_N;  e = taubar - abar;  beta = (h - K0 abar)_A;  dl = e'dD + beta'dbound_A

dense=False restates the device algorithm instead of the dense reduced solve: the penalised factor of
polish_oracle.polish as a preconditioner, the exact masked residual, 1 + refine_steps solves in delta form.
"""
from __future__ import annotations

import numpy as np

import adjoint_oracle as O
import polish_oracle as P
import tangent_oracle as T

OUTS = T.OUTS
NAMES = O.NAMES
COTS = ("gx", "gy", "gzl", "gzu", "gcons")


_faces = {}


def _face(qp, active_var, active_row):
    """The space, the codes, K0, the polished point of the set and the factors, kept per problem and set."""
    key = (id(qp), np.asarray(active_var, np.int8).tobytes(), np.asarray(active_row, np.int8).tobytes())
    if key not in _faces:
        S = P.space(qp)
        c = P._codes_of(S, active_var, active_row)
        m = S.D.m
        K0 = np.block([[S.W, S.J.T], [S.J, np.zeros((m, m))]])
        _faces[key] = (qp, S, c, K0, P.exact(qp, active_var, active_row), {})
    return _faces[key][1:]


def _masked_solve(S, c, K0, lu, u, rhs, dense, sigma=P.SIGMA, refine_steps=P.REFINE_STEPS, delta_w=P.DELTA_W,
                  delta_c=P.DELTA_C):
    """u with (K0 u)_i = rhs_i on the inactive coordinates and the rows, u_A as given; K0 u - rhs on A; the
    max-norm of the final masked residual (dense: of the refined dense solve).  lu: the face's factors."""
    nv = S.nf + S.ns
    m = S.D.m
    act = np.concatenate([c != 0, np.zeros(m, bool)])
    free = np.flatnonzero(~act)
    u = u.copy()

    def resid(u):
        r = rhs - K0 @ u
        r[act] = 0.0
        return r

    if dense:
        if "M" not in lu:
            lu["M"] = P._lu(K0[np.ix_(free, free)])
        for _ in range(2):                 # one step of refinement, as polish_oracle.exact
            u[free] += lu["M"](resid(u)[free])
    else:
        key = (sigma, delta_w, delta_c)
        if key not in lu:
            lu[key] = P._lu(K0 + np.diag(np.concatenate([delta_w + np.where(c != 0, sigma, 0.0),
                                                         np.full(m, delta_c)])))
        for _ in range(refine_steps + 1):
            d = lu[key](resid(u))
            d[act] = 0.0
            u = u + d
    keep = (K0 @ u - rhs)[:nv]
    return u, np.where(c != 0, keep, 0.0), float(np.max(np.abs(resid(u)), initial=0.0))


def _dbound(S, c, v):
    """The direction of the active bound of every coordinate of [x_F; s] (0 on an inactive one)."""
    D = S.D
    lo = np.concatenate([v["lvar"][D.F], v["lcon"][D.I]])
    hi = np.concatenate([v["uvar"][D.F], v["ucon"][D.I]])
    return np.where(c < 0, lo, np.where(c > 0, hi, 0.0))


def tangent(qp, active_var, active_row, d, dense=True, info=None, **kw):
    """(dx, dy, dzl, dzu, dcons) of polish_oracle.exact(qp, set) along `d` (keys out of NAMES), the set held."""
    S, c, K0, ex, lu = _face(qp, active_var, active_row)
    D = S.D
    nv, m = S.nf + S.ns, D.m
    x, y = ex["x"], ex["y"]
    v, dH, dA = T._blocks(qp, d)
    dxfix = np.where(D.fixed, v["lvar"], 0.0)
    db = np.where(D.eq, v["lcon"], 0.0)
    dD = np.concatenate([(D.sgn * (v["c"] + dH @ x + D.H @ dxfix) + dA.T @ y)[D.F], np.zeros(S.ns),
                         dA @ x + D.A @ dxfix - db])
    u0 = np.concatenate([_dbound(S, c, v), np.zeros(m)])
    u, dt, res = _masked_solve(S, c, K0, lu, u0, -dD, dense, **kw)
    if info is not None:
        info["residual"] = res
    dx = dxfix.copy()
    dx[D.F] = u[:S.nf]
    dzl, dzu = np.zeros(D.n), np.zeros(D.n)
    dzl[D.F] = np.where(c < 0, dt, 0.0)[:S.nf]
    dzu[D.F] = np.where(c > 0, -dt, 0.0)[:S.nf]
    dcons = D.A @ dx + dA @ x
    cr = c[S.nf:]
    dcons[D.I] = np.where(cr != 0, u0[S.nf:nv], dcons[D.I])
    return {"x": dx, "y": u[nv:], "zl": dzl, "zu": dzu, "cons": dcons}


def adjoint(qp, active_var, active_row, cot, dense=True, info=None, **kw):
    """The gradients of l(x, y, zl, zu, cons) of the polished point with respect to the seven data blocks, given
    the cotangents in `cot` (keys out of COTS; a missing one is 0), the set held."""
    assert set(cot) <= set(COTS), sorted(cot)
    S, c, K0, ex, lu = _face(qp, active_var, active_row)
    D = S.D
    n, m, sgn, F, I = D.n, D.m, D.sgn, D.F, D.I
    nv = S.nf + S.ns
    x, y = ex["x"], ex["y"]
    z = lambda k, size: np.asarray(cot[k], float) if cot.get(k) is not None else np.zeros(size)  # noqa: E731
    gx, gy, gzl, gzu, gcons = z("gx", n), z("gy", m), z("gzl", n), z("gzu", n), z("gcons", m)
    ghat = np.concatenate([gx[F], gcons[I], gy])
    cv = c[:S.nf]
    tau = np.concatenate([np.where(cv < 0, gzl[F], np.where(cv > 0, -gzu[F], 0.0)), np.zeros(S.ns + m)])
    # u = abar - taubar solves the masked system with right-hand side ghat: (ghat - K0 u)_N = (h - K0 abar)_N = 0
    u, keep, res = _masked_solve(S, c, K0, lu, -tau, ghat, dense, **kw)
    if info is not None:
        info["residual"] = res
    e, beta = -u, -keep
    ex_, ey = np.zeros(n), e[nv:]
    ex_[F] = e[:S.nf]
    r, cc = np.asarray(qp.Hrows, int), np.asarray(qp.Hcols, int)
    ar, ac = np.asarray(qp.Arows, int), np.asarray(qp.Acols, int)
    lv, uv = np.zeros(n), np.zeros(n)
    lv[F], uv[F] = np.where(cv < 0, beta[:S.nf], 0.0), np.where(cv > 0, beta[:S.nf], 0.0)
    lv = np.where(D.fixed, gx + sgn * (D.H @ ex_) + D.A.T @ ey, lv)
    cr = c[S.nf:]
    lc, uc = np.where(D.eq, gcons - ey, 0.0), np.zeros(m)
    lc[I], uc[I] = np.where(cr < 0, beta[S.nf:], 0.0), np.where(cr > 0, beta[S.nf:], 0.0)
    return {"c": sgn * ex_,
            "Hvals": sgn * ex_[r] * x[cc] + np.where(r == cc, 0.0, sgn * ex_[cc] * x[r]),
            "Avals": ex_[ac] * y[ar] + ey[ar] * x[ac],
            "lcon": lc, "ucon": uc, "lvar": lv, "uvar": uv}


def finite_difference(qp, active_var, active_row, d, h=1e-6):
    """Central differences of polish_oracle.exact along `d` with the set held fixed."""
    a = P.exact(T.moved(qp, d, h), active_var, active_row)
    b = P.exact(T.moved(qp, d, -h), active_var, active_row)
    return {k: (a[k] - b[k]) / (2 * h) for k in OUTS}


def max_err(a, ref, keys):
    return max(O.err(a[k], ref[k]) for k in keys)
