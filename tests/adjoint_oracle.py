"""A CPU oracle for MPCSolver.adjoint: problem fixtures, a dense reference interior-point method and the
adjoint formulas of DESIGN §13c evaluated with a dense solve.  No GPU, no library call.

The public space throughout: (x, y, zl, zu) as solve() returns them, sgn = +1 for minimize and -1 for
maximize, the multipliers those of min sgn f:

    sgn (H x + c) + A'y - zl + zu = 0 on the free variables,     y_i = zu_s - zl_s on an inequality row i,

with the slack s_I = (A x)_I of the inequality rows I (lcon != ucon), zl_s = max(-y, 0), zu_s = max(y, 0).
"""
from __future__ import annotations

import dataclasses

import numpy as np

NAMES = ("c", "Hvals", "Avals", "lcon", "ucon", "lvar", "uvar")
MU_END = 1e-11


def _qm():
    from madipm_amd.qp import QuadraticModel
    return QuadraticModel


# ------------------------------------------------------------------ dense views
@dataclasses.dataclass
class Dense:
    n: int
    m: int
    sgn: float
    H: np.ndarray          # full symmetric, duplicates summed
    A: np.ndarray          # duplicates summed
    fixed: np.ndarray      # bool (n)
    F: np.ndarray          # free variables
    I: np.ndarray          # inequality rows
    eq: np.ndarray         # bool (m)


def dense(qp) -> Dense:
    n, m = qp.nvar, qp.ncon
    H = np.zeros((n, n))
    r, c = np.asarray(qp.Hrows, int), np.asarray(qp.Hcols, int)
    np.add.at(H, (r, c), qp.Hvals)
    off = r != c
    np.add.at(H, (c[off], r[off]), np.asarray(qp.Hvals)[off])
    A = np.zeros((m, n))
    np.add.at(A, (np.asarray(qp.Arows, int), np.asarray(qp.Acols, int)), qp.Avals)
    lvar, uvar = np.asarray(qp.lvar, float), np.asarray(qp.uvar, float)
    lcon, ucon = np.asarray(qp.lcon, float), np.asarray(qp.ucon, float)
    fixed = lvar == uvar
    eq = lcon == ucon
    return Dense(n, m, 1.0 if qp.minimize else -1.0, H, A, fixed, np.flatnonzero(~fixed), np.flatnonzero(~eq), eq)


BIG = 400   # unknowns above which the Newton matrices are kept sparse (a dense LU would take seconds per step)


def _solve(K, rhs):
    if K.shape[0] > BIG:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        return spl.splu(sp.csc_matrix(K), permc_spec="MMD_AT_PLUS_A").solve(rhs)
    return np.linalg.solve(K, rhs)


# ------------------------------------------------------------------ reference interior-point method
def reference_ipm(qp, mu_end=MU_END, max_iter=200):
    """Mehrotra predictor-corrector on the reduced K2 Newton system down to mu_end, then Newton steps on the
    central-path equations at mu = mu_end until their residual is at rounding level: the returned point is
    the central-path point of mu_end, which is what the adjoint formulas differentiate.  Returns a dict
    with x, y, zl, zu (public space) and mu."""
    D = dense(qp)
    n, m, sgn, F, I = D.n, D.m, D.sgn, D.F, D.I
    nf, ns = len(F), len(I)
    lvar, uvar = np.asarray(qp.lvar, float), np.asarray(qp.uvar, float)
    lcon, ucon = np.asarray(qp.lcon, float), np.asarray(qp.ucon, float)
    lo = np.concatenate([lvar[F], lcon[I]])
    hi = np.concatenate([uvar[F], ucon[I]])
    lb, ub = np.isfinite(lo), np.isfinite(hi)
    x = np.zeros(n)
    x[D.fixed] = lvar[D.fixed]
    b = np.where(D.eq, lcon, 0.0)
    E = np.zeros((m, ns))
    E[I, np.arange(ns)] = 1.0
    Jv = np.hstack([D.A[:, F], -E])
    W = np.zeros((nf + ns, nf + ns))
    W[:nf, :nf] = sgn * D.H[np.ix_(F, F)]
    K0 = np.block([[W, Jv.T], [Jv, np.zeros((m, m))]])
    big = K0.shape[0] > BIG
    if big:
        import scipy.sparse as sp
        K0 = sp.csc_matrix(K0)

    def interior(v):
        v = v.copy()
        both = lb & ub
        v[both] = np.clip(v[both], lo[both] + 0.25 * (hi - lo)[both], hi[both] - 0.25 * (hi - lo)[both])
        ol, ou = lb & ~ub, ub & ~lb
        v[ol] = np.maximum(v[ol], lo[ol] + 1.0)
        v[ou] = np.minimum(v[ou], hi[ou] - 1.0)
        return v

    v = interior(np.concatenate([np.zeros(nf), (D.A @ x)[I]]))
    y = np.zeros(m)
    zl, zu = np.where(lb, 1.0, 0.0), np.where(ub, 1.0, 0.0)
    nb = max(int(lb.sum() + ub.sum()), 1)

    def resid(v, y, zl, zu):
        x[F] = v[:nf]
        g = np.concatenate([sgn * (D.H @ x + qp.c)[F], np.zeros(ns)]) + Jv.T @ y
        return g - zl + zu, D.A @ x - E @ v[nf:] - b

    def gaps(v):
        return np.where(lb, v - lo, 1.0), np.where(ub, hi - v, 1.0)

    def factor(v, zl, zu):
        """The solver of the reduced Newton matrix at (v, zl, zu): one factorisation, shared by the
        predictor and the corrector."""
        gl, gu = gaps(v)
        sig = np.where(lb, zl / gl, 0.0) + np.where(ub, zu / gu, 0.0)
        dg = np.concatenate([sig, np.zeros(m)])
        if big:
            import scipy.sparse.linalg as spl
            return spl.splu(K0 + sp.diags(dg, format="csc"), permc_spec="MMD_AT_PLUS_A").solve
        K = K0 + np.diag(dg)
        return lambda rhs: np.linalg.solve(K, rhs)

    def newton(solve, v, zl, zu, rd, rp, cl, cu):
        gl, gu = gaps(v)
        rhs = np.concatenate([-rd + np.where(lb, cl / gl, 0.0) - np.where(ub, cu / gu, 0.0), -rp])
        d = solve(rhs)
        dv, dy = d[:nf + ns], d[nf + ns:]
        dzl = np.where(lb, (cl - zl * dv) / gl, 0.0)
        dzu = np.where(ub, (cu + zu * dv) / gu, 0.0)
        return dv, dy, dzl, dzu

    def maxstep(v, dv, zl, dzl, zu, dzu, tau):
        gl, gu = gaps(v)
        ap = ad = 1.0
        for gap, dgap, msk in ((gl, dv, lb), (gu, -dv, ub)):
            neg = msk & (dgap < 0)
            if neg.any():
                ap = min(ap, float(np.min(-tau * gap[neg] / dgap[neg])))
        for z, dz, msk in ((zl, dzl, lb), (zu, dzu, ub)):
            neg = msk & (dz < 0)
            if neg.any():
                ad = min(ad, float(np.min(-tau * z[neg] / dz[neg])))
        return ap, ad

    def mu_of(v, zl, zu):
        gl, gu = gaps(v)
        return float((zl[lb] @ gl[lb] + zu[ub] @ gu[ub]) / nb)

    for _ in range(max_iter):
        rd, rp = resid(v, y, zl, zu)
        mu = mu_of(v, zl, zu) if lb.any() or ub.any() else 0.0
        if mu <= mu_end and max(np.abs(rd).max(initial=0), np.abs(rp).max(initial=0)) <= 1e-9:
            break
        gl, gu = gaps(v)
        solve = factor(v, zl, zu)
        dv, dy, dzl, dzu = newton(solve, v, zl, zu, rd, rp, -zl * gl, -zu * gu)
        ap, ad = maxstep(v, dv, zl, dzl, zu, dzu, 1.0)
        mu_aff = mu_of(v + ap * dv, zl + ad * dzl, zu + ad * dzu) if mu > 0 else 0.0
        mut = max((mu_aff / mu) ** 3 * mu if mu > 0 else 0.0, 0.1 * mu_end if mu <= 10 * mu_end else 0.0)
        dv, dy, dzl, dzu = newton(solve, v, zl, zu, rd, rp, mut - zl * gl - dv * dzl, mut - zu * gu + dv * dzu)
        ap, ad = maxstep(v, dv, zl, dzl, zu, dzu, 0.995)
        v, y, zl, zu = v + ap * dv, y + ad * dy, zl + ad * dzl, zu + ad * dzu
    else:
        raise RuntimeError("reference_ipm: no convergence")
    if lb.any() or ub.any():      # onto the central path of mu_end
        for _ in range(60):
            rd, rp = resid(v, y, zl, zu)
            gl, gu = gaps(v)
            cl, cu = np.where(lb, mu_end - zl * gl, 0.0), np.where(ub, mu_end - zu * gu, 0.0)
            err = max(np.abs(rd).max(initial=0), np.abs(rp).max(initial=0),
                      np.abs(cl).max(initial=0) / mu_end * 1e-13, np.abs(cu).max(initial=0) / mu_end * 1e-13)
            if err <= 2e-14 * max(1.0, np.abs(y).max(initial=0), np.abs(v).max(initial=0)):
                break
            dv, dy, dzl, dzu = newton(factor(v, zl, zu), v, zl, zu, rd, rp, cl, cu)
            ap, ad = maxstep(v, dv, zl, dzl, zu, dzu, 0.999)
            v, y, zl, zu = v + ap * dv, y + ad * dy, zl + ad * dzl, zu + ad * dzu
    x[F] = v[:nf]
    ZL, ZU = np.zeros(n), np.zeros(n)
    ZL[F], ZU[F] = zl[:nf], zu[:nf]
    return {"x": x.copy(), "y": y, "zl": ZL, "zu": ZU, "mu": mu_end}


# ------------------------------------------------------------------ the adjoint formulas
def reference_adjoint(qp, point, gx, terms=False):
    """The gradients of l with dl/dx* = gx with respect to the seven data blocks, by the formulas of DESIGN
    §13c evaluated at `point` (a dict with x, y, zl, zu of the public space) with one dense solve.
    terms=True: also the single terms of every formula, {block: [arrays]}, for the fixture checks."""
    D = dense(qp)
    n, m, sgn, F, I = D.n, D.m, D.sgn, D.F, D.I
    nf, ns = len(F), len(I)
    x, y = np.asarray(point["x"], float), np.asarray(point["y"], float)
    zl, zu = np.asarray(point["zl"], float), np.asarray(point["zu"], float)
    lvar, uvar = np.asarray(qp.lvar, float), np.asarray(qp.uvar, float)
    lcon, ucon = np.asarray(qp.lcon, float), np.asarray(qp.ucon, float)
    gx = np.asarray(gx, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        sl = np.where(np.isfinite(lvar) & ~D.fixed, zl / (x - lvar), 0.0)
        su = np.where(np.isfinite(uvar) & ~D.fixed, zu / (uvar - x), 0.0)
        s = (D.A @ x)[I]
        sls = np.where(np.isfinite(lcon[I]), np.maximum(-y[I], 0.0) / (s - lcon[I]), 0.0)
        sus = np.where(np.isfinite(ucon[I]), np.maximum(y[I], 0.0) / (ucon[I] - s), 0.0)
    E = np.zeros((m, ns))
    E[I, np.arange(ns)] = 1.0
    K = np.zeros((nf + ns + m, nf + ns + m))
    K[:nf, :nf] = sgn * D.H[np.ix_(F, F)] + np.diag((sl + su)[F])
    K[nf:nf + ns, nf:nf + ns] = np.diag(sls + sus)
    K[nf + ns:, :nf] = D.A[:, F]
    K[nf + ns:, nf:nf + ns] = -E
    K[:nf + ns, nf + ns:] = K[nf + ns:, :nf + ns].T
    a = _solve(K, np.concatenate([gx[F], np.zeros(ns + m)]))
    ax = np.zeros(n)
    ax[F] = a[:nf]
    as_, ay = a[nf:nf + ns], a[nf + ns:]
    r, c = np.asarray(qp.Hrows, int), np.asarray(qp.Hcols, int)
    ar, ac = np.asarray(qp.Arows, int), np.asarray(qp.Acols, int)
    t = {}
    t["c"] = [-sgn * ax]
    h1, h2 = -sgn * ax[r] * x[c], np.where(r == c, 0.0, -sgn * ax[c] * x[r])
    t["Hvals"] = [h1, h2]
    t["Avals"] = [-ax[ac] * y[ar], -ay[ar] * x[ac]]
    fx = D.fixed
    t["lvar"] = [np.where(fx, 0.0, sl * ax), np.where(fx, gx, 0.0), np.where(fx, -sgn * (D.H @ ax), 0.0),
                 np.where(fx, -(D.A.T @ ay), 0.0)]
    t["uvar"] = [np.where(fx, 0.0, su * ax)]
    lc, uc = np.where(D.eq, ay, 0.0), np.zeros(m)
    lc[I], uc[I] = sls * as_, sus * as_
    t["lcon"], t["ucon"] = [lc], [uc]
    g = {k: np.sum(v, axis=0) for k, v in t.items()}
    return (g, t) if terms else g


def err(g, ref):
    """max |g - ref| / max(1, max |ref|), the measure of every comparison (0 for an empty block)."""
    g, ref = np.asarray(g, float), np.asarray(ref, float)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(g - ref)) / max(1.0, np.max(np.abs(ref))))


def finite_difference(qp, gx, h=1e-6):
    """Central differences of l = gx'x*(data) through reference_ipm, block by block, with the conventions of
    the formulas: a fixed variable's / equality row's common value is moved as one and reported in lvar /
    lcon; infinite bounds are not moved (0)."""
    def loss(q):
        return float(gx @ reference_ipm(q)["x"])

    def moved(field, idx, d, also=None):
        new = {field: np.array(getattr(qp, field), float)}
        new[field][idx] += d
        if also:
            new[also] = np.array(getattr(qp, also), float)
            new[also][idx] += d
        return dataclasses.replace(qp, **new)

    out = {}
    fixed = np.asarray(qp.lvar) == np.asarray(qp.uvar)
    eq = np.asarray(qp.lcon) == np.asarray(qp.ucon)
    for k in NAMES:
        base = np.asarray(getattr(qp, k), float)
        g = np.zeros(base.size)
        for i in range(base.size):
            if not np.isfinite(base[i]):
                continue
            also = None
            if k in ("lvar", "uvar") and fixed[i]:
                if k == "uvar":
                    continue
                also = "uvar"
            if k in ("lcon", "ucon") and eq[i]:
                if k == "ucon":
                    continue
                also = "ucon"
            g[i] = (loss(moved(k, i, h, also)) - loss(moved(k, i, -h, also))) / (2 * h)
        out[k] = g
    return out


# ------------------------------------------------------------------ fixtures
# Active sets of the 7 x 5 family (variables 0: lower bound, 1: upper bound, 2: boxed, 3: fixed, 4-6 free;
# rows 0-1: equalities, 2: lower side only, 3: upper side only, 4: ranged), by pattern: which bounds are
# active at the optimum.  Every block of the gradient is exercised by one of them.
PATTERNS = {
    0: dict(var_l=(0,), var_u=(), row_l=(2,), row_u=()),
    1: dict(var_l=(), var_u=(1, 2), row_l=(), row_u=(3,)),
    2: dict(var_l=(2,), var_u=(), row_l=(4,), row_u=()),
    3: dict(var_l=(0,), var_u=(1,), row_l=(), row_u=(4,)),
}
FAMILY_SEEDS = (0, 1, 2, 3)


def family(seed, minimize=True):
    """One problem of the 7 x 5 family, built from its optimum: x*, the active set PATTERNS[seed % 4] and
    multipliers in [0.05, 0.45] are drawn (minimize=False: the objective is negated, so x* is the same), the bounds are put at x* (active) or 0.1-0.3 away (inactive) and
    c is solved from stationarity, so the problem is strictly complementary by construction (asserted in
    check_strict).  Returns (qp, gx)."""
    rng = np.random.default_rng(1000 + seed)
    pat = PATTERNS[seed % 4]
    n, m = 7, 5
    sgn = 1.0 if minimize else -1.0
    P = rng.standard_normal((n, n))
    H = sgn * (P @ P.T / n + np.eye(n))      # maximize: the negated (concave) objective, the same optimum
    A = rng.uniform(0.3, 1.0, (m, n)) * rng.choice([-1.0, 1.0], (m, n))
    x = rng.uniform(0.4, 1.2, n) * rng.choice([-1.0, 1.0], n)
    gap = lambda: rng.uniform(0.1, 0.3)  # noqa: E731
    mult = lambda: rng.uniform(0.05, 0.45)  # noqa: E731
    lvar, uvar = np.full(n, -np.inf), np.full(n, np.inf)
    zl, zu = np.zeros(n), np.zeros(n)
    lvar[0] = x[0] - (0.0 if 0 in pat["var_l"] else gap())
    uvar[1] = x[1] + (0.0 if 1 in pat["var_u"] else gap())
    lvar[2] = x[2] - (0.0 if 2 in pat["var_l"] else gap())
    uvar[2] = x[2] + (0.0 if 2 in pat["var_u"] else gap())
    lvar[3] = uvar[3] = x[3]
    for i in pat["var_l"]:
        zl[i] = mult()
    for i in pat["var_u"]:
        zu[i] = mult()
    ax = A @ x
    lcon, ucon = np.full(m, -np.inf), np.full(m, np.inf)
    y = np.zeros(m)
    lcon[:2] = ucon[:2] = ax[:2]
    y[:2] = rng.uniform(0.1, 0.5, 2) * rng.choice([-1.0, 1.0], 2)
    lcon[2] = ax[2] - (0.0 if 2 in pat["row_l"] else gap())
    ucon[3] = ax[3] + (0.0 if 3 in pat["row_u"] else gap())
    lcon[4] = ax[4] - (0.0 if 4 in pat["row_l"] else gap())
    ucon[4] = ax[4] + (0.0 if 4 in pat["row_u"] else gap())
    for i in pat["row_l"]:
        y[i] = -mult()
    for i in pat["row_u"]:
        y[i] = mult()
    c = -H @ x - sgn * (A.T @ y - zl + zu)
    r, cc = np.tril_indices(n)
    ar, ac = np.nonzero(A)
    qp = _qm()(c=c, Hrows=r.astype(np.int32), Hcols=cc.astype(np.int32), Hvals=H[r, cc], Arows=ar.astype(np.int32),
               Acols=ac.astype(np.int32), Avals=A[ar, ac], lcon=lcon, ucon=ucon, lvar=lvar, uvar=uvar, c0=0.5,
               x0=np.zeros(n), minimize=minimize, name=f"adjoint_family_{seed}_{'min' if minimize else 'max'}")
    gx = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    return qp, gx


def check_strict(qp, point, active=1e-2, inactive=5e-2):
    """Strict complementarity of `point` with margins: every bound (of a free variable or an inequality
    row) is either active with a multiplier >= `active` (and a gap below 1e-6), or inactive with a gap >=
    `inactive` (and a multiplier below 1e-6).  Raises AssertionError otherwise."""
    D = dense(qp)
    x, y = point["x"], point["y"]
    s = (D.A @ x)[D.I]
    lo = np.concatenate([np.asarray(qp.lvar, float)[D.F], np.asarray(qp.lcon, float)[D.I]])
    hi = np.concatenate([np.asarray(qp.uvar, float)[D.F], np.asarray(qp.ucon, float)[D.I]])
    v = np.concatenate([x[D.F], s])
    zl = np.concatenate([point["zl"][D.F], np.maximum(-y[D.I], 0.0)])
    zu = np.concatenate([point["zu"][D.F], np.maximum(y[D.I], 0.0)])
    for gap, z in ((v - lo, zl), (hi - v, zu)):
        for g, zz in zip(gap, z):
            if not np.isfinite(g):
                continue
            assert (zz >= active and g <= 1e-6) or (g >= inactive and zz <= 1e-6), (qp.name, g, zz)


def scaled_family(seed=0):
    """family(seed) with row 1 (and its bounds) times 1e3 and c, H times 1e3: set_scaling! gives con_scale < 1
    on that row and obj_scale < 1.  The optimum x* is the family's."""
    qp, gx = family(seed)
    rf = np.ones(qp.ncon)
    rf[1] = 1e3
    return dataclasses.replace(qp, c=1e3 * qp.c, Hvals=1e3 * qp.Hvals, Avals=qp.Avals * rf[qp.Arows],
                               lcon=qp.lcon * rf, ucon=qp.ucon * rf, name=qp.name + "_scaled"), gx


def duplicated_family(seed=0):
    """family(seed) with COO entries of H and A split in two (0.3 v + 0.7 v, the copy appended at the end): the
    same problem; each copy must receive the full gradient of its entry."""
    qp, gx = family(seed)
    hk, ak = np.array([0, 4, 9, 20]), np.array([1, 8, 17, 30])

    def split(rows, cols, vals, k):
        v = np.array(vals, float)
        extra = 0.7 * v[k]
        v[k] *= 0.3
        return (np.concatenate([rows, rows[k]]).astype(np.int32), np.concatenate([cols, cols[k]]).astype(np.int32),
                np.concatenate([v, extra]))
    hr, hc, hv = split(qp.Hrows, qp.Hcols, qp.Hvals, hk)
    ar, ac, av = split(qp.Arows, qp.Acols, qp.Avals, ak)
    return dataclasses.replace(qp, Hrows=hr, Hcols=hc, Hvals=hv, Arows=ar, Acols=ac, Avals=av,
                               name=qp.name + "_dup"), gx, hk, ak


def lp_fixture(seed=7):
    """An LP (empty H) with a unique, strictly complementary vertex: 6 variables in [0, 2], 3 equality rows,
    built from its optimum (3 variables at a bound with reduced costs in [0.1, 0.5])."""
    rng = np.random.default_rng(seed)
    n, m = 6, 3
    A = rng.uniform(0.3, 1.0, (m, n)) * rng.choice([-1.0, 1.0], (m, n))
    x = np.array([0.0, 2.0, 0.0, 0.7, 1.1, 1.4])
    zl, zu = np.zeros(n), np.zeros(n)
    zl[[0, 2]] = rng.uniform(0.1, 0.5, 2)
    zu[1] = rng.uniform(0.1, 0.5)
    y = rng.uniform(0.1, 0.5, m) * rng.choice([-1.0, 1.0], m)
    c = -(A.T @ y - zl + zu)
    ar, ac = np.nonzero(A)
    e = np.zeros(0, np.int32)
    qp = _qm()(c=c, Hrows=e, Hcols=e, Hvals=np.zeros(0), Arows=ar.astype(np.int32), Acols=ac.astype(np.int32),
               Avals=A[ar, ac], lcon=A @ x, ucon=A @ x, lvar=np.zeros(n), uvar=np.full(n, 2.0), x0=np.ones(n),
               name="adjoint_lp")
    return qp, rng.uniform(0.5, 1.5, n)


def sparse_fixture(n=1000, m=600, nfix=20, seed=3):
    """A random sparse QP built from its optimum: n variables (nfix fixed, a third each lower-bounded, boxed
    and free), m rows (half equalities, the rest one-sided or ranged), about 4 entries per row of A, H =
    diagonal + a sparse lower triangle (diagonally dominant), a third of the bounds active with multipliers
    in [0.05, 0.45] and the others 0.1-0.3 away.  Row i holds variable i, and variables 0 .. m-1 are neither
    fixed nor at a bound, so the active constraints are linearly independent (a row whose variables all sit
    at bounds would leave its multiplier, and the gradients through it, undefined)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.4, 1.2, n) * rng.choice([-1.0, 1.0], n)
    # H
    k = 2 * n
    r, c = rng.integers(0, n, k), rng.integers(0, n, k)
    keep = r > c
    r, c = r[keep], c[keep]
    hv = rng.uniform(-0.3, 0.3, r.size)
    hr = np.concatenate([np.arange(n), r]).astype(np.int32)
    hc = np.concatenate([np.arange(n), c]).astype(np.int32)
    hvals = np.concatenate([rng.uniform(2.5, 3.5, n), hv])
    # A: 4 entries per row, distinct columns
    ar = np.repeat(np.arange(m), 4).astype(np.int32)
    # row i holds variable i, which stays off its bounds: the active rows are independent on those columns
    ac = np.concatenate([np.concatenate([[i], rng.choice(np.delete(np.arange(n), i), 3, replace=False)])
                         for i in range(m)]).astype(np.int32)
    av = rng.uniform(0.3, 1.0, ar.size) * rng.choice([-1.0, 1.0], ar.size)
    A = np.zeros((m, n))
    A[ar, ac] = av
    H = np.zeros((n, n))
    np.add.at(H, (hr, hc), hvals)
    H = H + np.tril(H, -1).T
    # bounds of the variables
    kind = rng.integers(0, 3, n)               # 0 lower-bounded, 1 boxed, 2 free
    fix = m + rng.choice(n - m, nfix, replace=False)
    lvar, uvar = np.full(n, -np.inf), np.full(n, np.inf)
    zl, zu = np.zeros(n), np.zeros(n)
    act = rng.random(n) < 1.0 / 3.0
    act[:m] = False
    side = rng.random(n) < 0.5
    for i in range(n):
        if kind[i] == 2:
            continue
        g = rng.uniform(0.1, 0.3, 2)
        lvar[i] = x[i] - g[0]
        if kind[i] == 1:
            uvar[i] = x[i] + g[1]
        if act[i]:
            if kind[i] == 1 and side[i]:
                uvar[i], zu[i] = x[i], rng.uniform(0.05, 0.45)
            else:
                lvar[i], zl[i] = x[i], rng.uniform(0.05, 0.45)
    lvar[fix], uvar[fix] = x[fix], x[fix]
    zl[fix] = zu[fix] = 0.0
    # rows
    ax = A @ x
    lcon, ucon = ax.copy(), ax.copy()
    y = rng.uniform(0.1, 0.5, m) * rng.choice([-1.0, 1.0], m)
    for i in range(m // 2, m):
        t = rng.integers(0, 3)                 # 0 lower side, 1 upper side, 2 ranged
        g = rng.uniform(0.1, 0.3, 2)
        lcon[i] = ax[i] - g[0] if t != 1 else -np.inf
        ucon[i] = ax[i] + g[1] if t != 0 else np.inf
        y[i] = 0.0
        if rng.random() < 1.0 / 3.0:
            if t == 1 or (t == 2 and rng.random() < 0.5):
                ucon[i], y[i] = ax[i], rng.uniform(0.05, 0.45)
            else:
                lcon[i], y[i] = ax[i], -rng.uniform(0.05, 0.45)
    c = -H @ x - (A.T @ y - zl + zu)
    qp = _qm()(c=c, Hrows=hr, Hcols=hc, Hvals=hvals, Arows=ar, Acols=ac, Avals=av, lcon=lcon, ucon=ucon, lvar=lvar,
               uvar=uvar, x0=np.zeros(n), name="adjoint_sparse")
    return qp, rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
