"""A CPU oracle for MPCSolver.adjoint with all five cotangents: the loss is l(x, y, zl, zu, cons)
with cons = A x.  The plain and the shifted formulas with a dense solve, central differences of the five-block
loss through adjoint_oracle.reference_ipm, the cotangents of the tests and the row-length fixture.
No GPU, no library call.  Notation, fixtures and the measure `err` are adjoint_oracle's.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import adjoint_oracle as O

COTS = ("gx", "gy", "gzl", "gzu", "gcons")
NAMES = O.NAMES


def cotangents(qp, gx, seed=0):
    """The five cotangents of the tests: the fixture's gx and seeded gy, gzl, gzu, gcons, every entry of
    magnitude 0.5 - 1.5 with a random sign."""
    rng = np.random.default_rng(4000 + seed)
    draw = lambda k: rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)  # noqa: E731
    return {"gx": np.asarray(gx, float), "gy": draw(qp.ncon), "gzl": draw(qp.nvar), "gzu": draw(qp.nvar),
            "gcons": draw(qp.ncon)}


def only(cot, *keep):
    """The cotangents of `keep` alone (the others absent)."""
    return {k: v for k, v in cot.items() if k in keep}


def _sigmas(qp, D, point):
    x, y = np.asarray(point["x"], float), np.asarray(point["y"], float)
    zl, zu = np.asarray(point["zl"], float), np.asarray(point["zu"], float)
    lvar, uvar = np.asarray(qp.lvar, float), np.asarray(qp.uvar, float)
    lcon, ucon = np.asarray(qp.lcon, float), np.asarray(qp.ucon, float)
    I = D.I
    with np.errstate(divide="ignore", invalid="ignore"):
        hasl, hasu = np.isfinite(lvar) & ~D.fixed, np.isfinite(uvar) & ~D.fixed
        sl = np.where(hasl, zl / (x - lvar), 0.0)
        su = np.where(hasu, zu / (uvar - x), 0.0)
        s = (D.A @ x)[I]
        sls = np.where(np.isfinite(lcon[I]), np.maximum(-y[I], 0.0) / (s - lcon[I]), 0.0)
        sus = np.where(np.isfinite(ucon[I]), np.maximum(y[I], 0.0) / (ucon[I] - s), 0.0)
    return hasl, hasu, sl, su, sls, sus


def reference_adjoint_full(qp, point, cot, form="shifted"):
    """The gradients of l(x, y, zl, zu, A x) with respect to the seven data blocks at `point` (x, y, zl, zu of
    the public space), given the cotangents in `cot` (keys out of COTS; a missing one is 0).
    form = "plain": K a = [(gxe - Sigma_l gzl + Sigma_u gzu)_F; 0; gy] and lvar = Sigma_l (ax + gzl),
    uvar = Sigma_u (ax - gzu) on the free variables.  form = "shifted": the same system moved by q, whose
    right-hand side and bound gradients carry no product of Sigma with a cotangent."""
    assert form in ("plain", "shifted") and set(cot) <= set(COTS), (form, sorted(cot))
    D = O.dense(qp)
    n, m, sgn, F, I = D.n, D.m, D.sgn, D.F, D.I
    nf, ns = len(F), len(I)
    x, y = np.asarray(point["x"], float), np.asarray(point["y"], float)
    z = lambda k, size: np.asarray(cot[k], float) if cot.get(k) is not None else np.zeros(size)  # noqa: E731
    gx, gy, gzl, gzu, gcons = z("gx", n), z("gy", m), z("gzl", n), z("gzu", n), z("gcons", m)
    hasl, hasu, sl, su, sls, sus = _sigmas(qp, D, point)
    gzl, gzu = np.where(hasl, gzl, 0.0), np.where(hasu, gzu, 0.0)   # a multiplier without its bound is a constant
    gxe = gx + D.A.T @ gcons
    E = np.zeros((m, ns))
    E[I, np.arange(ns)] = 1.0
    K = np.zeros((nf + ns + m, nf + ns + m))
    K[:nf, :nf] = sgn * D.H[np.ix_(F, F)] + np.diag((sl + su)[F])
    K[nf:nf + ns, nf:nf + ns] = np.diag(sls + sus)
    K[nf + ns:, :nf] = D.A[:, F]
    K[nf + ns:, nf:nf + ns] = -E
    K[:nf + ns, nf + ns:] = K[nf + ns:, :nf + ns].T
    ax = np.zeros(n)
    if form == "plain":
        a = O._solve(K, np.concatenate([(gxe - sl * gzl + su * gzu)[F], np.zeros(ns), gy]))
        ax[F] = a[:nf]
        lv, uv = sl * (ax + gzl), su * (ax - gzu)
    else:
        # "has a bound" is asked of the bounds, not of the sign of Sigma: at a point the solver returned, x may
        # lie 1e-8 beyond an active bound (the solver's own bounds are the relaxed ones, bound_relax_factor),
        # which makes the public gap, and this Sigma, negative.  The formulas hold for either sign.
        sm = sl + su
        bounded = (hasl | hasu) & (sm != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(bounded, (sl * gzl - su * gzu) / sm, 0.0)
            h = np.where(bounded, sl * su / sm, 0.0)
        a = O._solve(K, np.concatenate([(gxe + sgn * (D.H @ q))[F], np.zeros(ns), gy + D.A @ q]))
        apx = np.zeros(n)
        apx[F] = a[:nf]
        ax = apx - q                      # q is 0 on the fixed variables
        lv, uv = sl * apx + h * (gzl + gzu), su * apx - h * (gzl + gzu)
    as_, ay = a[nf:nf + ns], a[nf + ns:]
    r, c = np.asarray(qp.Hrows, int), np.asarray(qp.Hcols, int)
    ar, ac = np.asarray(qp.Arows, int), np.asarray(qp.Acols, int)
    fx = D.fixed
    g = {"c": -sgn * ax,
         "Hvals": -sgn * ax[r] * x[c] + np.where(r == c, 0.0, -sgn * ax[c] * x[r]),
         "Avals": -ax[ac] * y[ar] - ay[ar] * x[ac] + gcons[ar] * x[ac],
         "lvar": np.where(fx, gxe - sgn * (D.H @ ax) - D.A.T @ ay, lv),
         "uvar": np.where(fx, 0.0, uv)}
    lc, uc = np.where(D.eq, ay, 0.0), np.zeros(m)
    lc[I], uc[I] = sls * as_, sus * as_
    g["lcon"], g["ucon"] = lc, uc
    return g


def loss(qp, point, cot):
    """l = gx'x + gy'y + gzl'zl + gzu'zu + gcons'(A x) at `point`, with qp's A."""
    v = {"gx": point["x"], "gy": point["y"], "gzl": point["zl"], "gzu": point["zu"],
         "gcons": O.dense(qp).A @ point["x"]}
    return float(sum(np.asarray(cot[k], float) @ v[k] for k in cot))


def finite_difference(qp, cot, h=1e-6):
    """Central differences of the five-block loss through reference_ipm, block by block, with
    adjoint_oracle.finite_difference's conventions: a fixed variable's / an equality row's common value is
    moved as one and reported in lvar / lcon; infinite bounds are not moved (0)."""
    def at(q):
        return loss(q, O.reference_ipm(q), cot)

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
            g[i] = (at(moved(k, i, h, also)) - at(moved(k, i, -h, also))) / (2 * h)
        out[k] = g
    return out


# ------------------------------------------------------------------ the row-length fixture
ROW_LENGTHS = (1, 3, 4, 5, 9)   # below, at and above one and two trips of a lane group of width 4


def rowlength_fixture(n=60, m=30, seed=11):
    """A QP built from its optimum, as adjoint_oracle.sparse_fixture is, whose rows of A and rows of the full
    symmetric H have 1, 3, 4, 5 and 9 entries (row i of A: ROW_LENGTHS[i % 5]; H: the diagonal and disjoint
    cliques of 3, 4, 5 and 9 variables, the other variables diagonal only).  No fixed variable (the solver leaves
    a fixed column out of its rows, which would change their lengths).  Rows 0 .. m/2-1 are equalities, the
    others one-sided or ranged, so their rows of J carry a slack entry besides.  Row i holds variable i, and
    variables 0 .. m-1 stay off their bounds: the active constraints are independent.  Returns (qp, gx)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.4, 1.2, n) * rng.choice([-1.0, 1.0], n)
    # H: diagonal + cliques over a random selection of the variables
    perm = rng.permutation(n)
    hr, hc = list(range(n)), list(range(n))
    at = 0
    for size in (3, 4, 5, 9):
        mem = np.sort(perm[at:at + size])
        at += size
        for a in range(size):
            for b in range(a):
                hr.append(int(mem[a]))
                hc.append(int(mem[b]))
    hr, hc = np.array(hr, np.int32), np.array(hc, np.int32)
    hvals = np.concatenate([rng.uniform(2.5, 3.5, n), rng.uniform(-0.3, 0.3, hr.size - n)])
    H = np.zeros((n, n))
    H[hr, hc] = hvals
    H = H + np.tril(H, -1).T
    # A: row i holds variable i and ROW_LENGTHS[i % 5] - 1 others
    ar, ac = [], []
    for i in range(m):
        k = ROW_LENGTHS[i % 5]
        cols = np.concatenate([[i], rng.choice(np.delete(np.arange(n), i), k - 1, replace=False)])
        ar += [i] * k
        ac += [int(c) for c in cols]
    ar, ac = np.array(ar, np.int32), np.array(ac, np.int32)
    av = rng.uniform(0.3, 1.0, ar.size) * rng.choice([-1.0, 1.0], ar.size)
    A = np.zeros((m, n))
    A[ar, ac] = av
    # bounds of the variables: as sparse_fixture
    kind = rng.integers(0, 3, n)               # 0 lower-bounded, 1 boxed, 2 free
    lvar, uvar = np.full(n, -np.inf), np.full(n, np.inf)
    zl, zu = np.zeros(n), np.zeros(n)
    act = rng.random(n) < 0.5
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
    qp = O._qm()(c=c, Hrows=hr, Hcols=hc, Hvals=hvals, Arows=ar, Acols=ac, Avals=av, lcon=lcon, ucon=ucon,
                 lvar=lvar, uvar=uvar, x0=np.zeros(n), name="adjoint_rowlength")
    return qp, rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)


def row_lengths(qp):
    """(entries per row of A, entries per row of the full symmetric H) of the COO input."""
    D = O.dense(qp)
    return np.count_nonzero(D.A, axis=1), np.count_nonzero(D.H, axis=1)
