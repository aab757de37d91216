"""A CPU oracle for MPCSolver.active_set_solve: the rounds of start, penalised delta-form solves,
verdict and repaired set, restated with numpy on top of polish_oracle.py in the public space; and the two
generators of updated problems the tests use.  No GPU, no library call.  Notation is polish_oracle.py's:
codes c_j in {-1, 0, +1} on v = [x_F; s]."""
from __future__ import annotations

import dataclasses

import numpy as np

import polish_oracle as P

MAX_ROUNDS = 4


# ------------------------------------------------------------------ updated problems
def shifted(qp, seed, eps):
    """qp with c shifted by eps N(0, 1), both bounds of every variable by one eps N(0, 1) and both sides of every
    row by one eps N(0, 1), drawn in that order from default_rng(seed): every classification survives (a fixed
    variable stays fixed, an equality row an equality row, an absent bound absent)."""
    rng = np.random.default_rng(seed)
    dc = eps * rng.standard_normal(qp.nvar)
    dv = eps * rng.standard_normal(qp.nvar)
    dr = eps * rng.standard_normal(qp.ncon)
    return dataclasses.replace(qp, c=qp.c + dc, lvar=qp.lvar + dv, uvar=qp.uvar + dv, lcon=qp.lcon + dr,
                               ucon=qp.ucon + dr)


def perturb(qp, rng, rel):
    """tools/resolve_bench.py's perturb at relative noise `rel`: the value fields of qp times 1 + rel U(-1, 1),
    both bounds of a coordinate by the same factor."""
    def f(k):
        return 1.0 + rel * rng.uniform(-1.0, 1.0, k)
    fv, fc = f(qp.nvar), f(qp.ncon)
    return dict(c=qp.c * f(qp.nvar), Avals=qp.Avals * f(qp.nnzj), Hvals=qp.Hvals * f(qp.nnzh),
                lvar=qp.lvar * fv, uvar=qp.uvar * fv, lcon=qp.lcon * fc, ucon=qp.ucon * fc)


def update_fields(qp):
    """The fields MPCSolver.update takes, from a problem."""
    return {k: np.asarray(getattr(qp, k), float) for k in ("c", "Hvals", "Avals", "lcon", "ucon", "lvar", "uvar")}


# ------------------------------------------------------------------ one round
def _round(S, c, os_, cs, sigma, refine_steps, tol_resid, tol_sign, tol_feas, delta_w, delta_c):
    """Steps 1-3 on the codes c: the start (the raw bound on an active coordinate, 0 on an inactive one, y = 0),
    P.polish's penalised factor and 1 + refine_steps delta-form solves, the measures and the verdict.  Returns a
    dict with v, y, the multipliers of the active coordinates and the verdict's figures."""
    act = c != 0
    nv, m = S.nf + S.ns, S.D.m
    v = np.where(c < 0, S.lo, np.where(c > 0, S.hi, 0.0))
    y = np.zeros(m)
    K = np.block([[S.W + np.diag(delta_w + np.where(act, sigma, 0.0)), S.J.T], [S.J, delta_c * np.eye(m)]])
    verdict = P.POLISHED
    try:
        solve = P._lu(K)
    except Exception:
        solve, verdict = None, P.FACTORIZATION_FAILED
    scale = np.concatenate([np.full(S.nf, os_), os_ / cs[S.D.I], cs])

    def resid(v, y):
        r1 = -(S.g + S.W @ v + S.J.T @ y)
        r1[act] = 0.0
        return np.concatenate([r1, -(S.J @ v - S.b)])

    hist = []
    if solve is not None:
        for _ in range(refine_steps + 1):
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
        t = S.g + S.W @ v + S.J.T @ y
        mult = np.where(c < 0, t, np.where(c > 0, -t, 0.0))          # of the active coordinates
        M = max(1.0, float(np.max(np.abs(mult[act]), initial=0.0)))
        gl = (v - S.lo) / np.maximum(1.0, np.abs(S.lo))               # relative gaps, where the bound exists
        gu = (S.hi - v) / np.maximum(1.0, np.abs(S.hi))
        inl, inu = S.lb & (c != -1), S.ub & (c != 1)
        min_mult = float(np.min(mult[act], initial=np.inf))
        rel_gap = float(np.min(np.concatenate([gl[inl], gu[inu]]), initial=np.inf))
        min_gap = float(np.min(np.concatenate([(v - S.lo)[inl], (S.hi - v)[inu]]), initial=np.inf))
        margin = float(np.min(np.concatenate([np.abs(mult[act]) / M, np.abs(gl[inl]), np.abs(gu[inu])]),
                              initial=np.inf))
    if min_mult < -tol_sign * M or rel_gap < -tol_feas:
        verdict = max(verdict, P.WRONG_SET)
    if not res <= tol_resid:
        verdict = max(verdict, P.NO_CONVERGENCE)
    return dict(v=v, y=y, mult=mult, M=M, gl=gl, gu=gu, verdict=verdict, residual=res, min_multiplier=min_mult,
                min_gap=min_gap, n_active=int(act.sum()), margin=margin, history=hist)


def _next(S, c, rd, tol_sign, tol_feas):
    """Step 4: the next codes from the round's violations.  An inactive coordinate whose lower and upper bound
    are both violated goes to the lower one; a coordinate dropped here is not added."""
    new = c.copy()
    act = c != 0
    new[act & (rd["mult"] < -tol_sign * rd["M"])] = 0
    with np.errstate(invalid="ignore"):
        up = ~act & S.ub & (rd["gu"] < -tol_feas)
        lo = ~act & S.lb & (rd["gl"] < -tol_feas)
    new[up] = 1
    new[lo] = -1
    return new


def active_set_solve(qp, active_var, active_row, max_rounds=MAX_ROUNDS, sigma=P.SIGMA, refine_steps=P.REFINE_STEPS,
                     tol_resid=P.TOL_RESID, tol_sign=P.TOL_SIGN, tol_feas=P.TOL_FEAS, delta_w=P.DELTA_W,
                     delta_c=P.DELTA_C):
    """Rounds 1 .. max_rounds from the given set.  Returns a dict: the blocks x, y, zl, zu, cons of the last
    round (the library writes them on POLISHED only), active_var / active_row (the last set tried), verdict,
    rounds, n_active, n_changed, residual, min_multiplier, min_gap, margin (the smallest decision margin over
    all rounds: |multiplier| / M over the active coordinates, |gap| / max(1, |bound|) over the inactive bounds)
    and histories (the residual history of each round)."""
    S = P.space(qp)
    c0 = P._codes_of(S, active_var, active_row)
    os_, cs = P.scaling(qp)
    c, margin, hists = c0.copy(), np.inf, []
    for k in range(1, max_rounds + 1):
        rd = _round(S, c, os_, cs, sigma, refine_steps, tol_resid, tol_sign, tol_feas, delta_w, delta_c)
        margin = min(margin, rd["margin"])
        hists.append(rd["history"])
        if rd["verdict"] != P.WRONG_SET or k == max_rounds:
            break
        c = _next(S, c, rd, tol_sign, tol_feas)
    out = P._pack(S, c, rd["v"], rd["y"])[0]
    av, ar = P._codes_out(S, c)
    out.update(active_var=av, active_row=ar, verdict=rd["verdict"], rounds=k, n_active=rd["n_active"],
               n_changed=int(np.count_nonzero(c != c0)), residual=rd["residual"],
               min_multiplier=rd["min_multiplier"], min_gap=rd["min_gap"], margin=margin, histories=hists)
    return out
