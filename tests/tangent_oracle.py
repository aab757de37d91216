"""A CPU oracle for MPCSolver.tangent: the directional derivative (dx, dy, dzl, dzu, dcons) of the
solution along a direction (dc, dHvals, dAvals, dlcon, ducon, dlvar, duvar) of the data.  The plain and the
shifted formulas with a dense solve, central differences through adjoint_oracle.reference_ipm, and the
directions of the tests.  No GPU, no library call.  Notation, fixtures and the measure `err` are
adjoint_oracle's; the Sigmas are adjoint_full_oracle's.

Conventions (the transposes of the adjoint's): a direction entry on an infinite bound is not read; a fixed
variable's common value moves by dlvar (duvar is not read); an equality row's by dlcon (ducon is not read);
a missing block is 0.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import adjoint_full_oracle as OF
import adjoint_oracle as O

NAMES = O.NAMES                                # the seven direction blocks
OUTS = ("x", "y", "zl", "zu", "cons")          # the five output blocks


def sizes(qp) -> dict:
    return {"c": qp.nvar, "Hvals": len(qp.Hvals), "Avals": len(qp.Avals), "lcon": qp.ncon, "ucon": qp.ncon,
            "lvar": qp.nvar, "uvar": qp.nvar}


def directions(qp, seed=0):
    """A direction in all seven blocks, every entry of magnitude 0.5 - 1.5 with a random sign."""
    rng = np.random.default_rng(7000 + seed)
    draw = lambda k: rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)  # noqa: E731
    return {k: draw(n) for k, n in sizes(qp).items()}


def only(d, *keep):
    """The direction blocks of `keep` alone (the others absent)."""
    return {k: v for k, v in d.items() if k in keep}


def not_read(qp) -> dict:
    """Per bound block, the mask of the entries the conventions do not read."""
    lvar, uvar = np.asarray(qp.lvar, float), np.asarray(qp.uvar, float)
    lcon, ucon = np.asarray(qp.lcon, float), np.asarray(qp.ucon, float)
    return {"lvar": ~np.isfinite(lvar), "uvar": ~np.isfinite(uvar) | (lvar == uvar),
            "lcon": ~np.isfinite(lcon), "ucon": ~np.isfinite(ucon) | (lcon == ucon)}


def with_nan(qp, d):
    """`d` with NaN in every entry that is not read."""
    out = {k: np.array(v, float) for k, v in d.items()}
    for k, mask in not_read(qp).items():
        if k in out:
            out[k][mask] = np.nan
    return out


def _blocks(qp, d):
    """The seven blocks of `d` (absent: 0) with every not-read entry replaced by 0, and dH, dA dense."""
    assert set(d) <= set(NAMES), sorted(d)
    v = {k: (np.array(d[k], float) if d.get(k) is not None else np.zeros(n)) for k, n in sizes(qp).items()}
    for k, mask in not_read(qp).items():
        v[k] = np.where(mask, 0.0, v[k])
    n, m = qp.nvar, qp.ncon
    r, c = np.asarray(qp.Hrows, int), np.asarray(qp.Hcols, int)
    dH = np.zeros((n, n))
    np.add.at(dH, (r, c), v["Hvals"])
    off = r != c
    np.add.at(dH, (c[off], r[off]), v["Hvals"][off])
    dA = np.zeros((m, n))
    np.add.at(dA, (np.asarray(qp.Arows, int), np.asarray(qp.Acols, int)), v["Avals"])
    return v, dH, dA


def reference_tangent(qp, point, d, form="shifted"):
    """(dx, dy, dzl, dzu, dcons) at `point` (x, y, zl, zu of the public space) along `d` (keys out of NAMES).
    form = "plain": K dw = [base1 + (Sigma_l dlvar + Sigma_u duvar)_F; Sigma_l,s dlcon_I + Sigma_u,s ducon_I;
    base3], dzl = -Sigma_l (dx - dlvar), dzu = Sigma_u (dx - duvar).  form = "shifted": the same system moved
    by p, p_s, whose right-hand side and outputs carry no product of Sigma with a direction."""
    assert form in ("plain", "shifted"), form
    D = O.dense(qp)
    n, m, sgn, F, I = D.n, D.m, D.sgn, D.F, D.I
    nf, ns = len(F), len(I)
    x, y = np.asarray(point["x"], float), np.asarray(point["y"], float)
    v, dH, dA = _blocks(qp, d)
    hasl, hasu, sl, su, sls, sus = OF._sigmas(qp, D, point)
    dl, du = np.where(hasl, v["lvar"], 0.0), np.where(hasu, v["uvar"], 0.0)
    dxfix = np.where(D.fixed, v["lvar"], 0.0)
    db = np.where(D.eq, v["lcon"], 0.0)
    dlc, duc = v["lcon"][I], v["ucon"][I]
    base1 = -(sgn * (dH @ x + v["c"] + D.H @ dxfix) + dA.T @ y)
    base3 = -(dA @ x + D.A @ dxfix) + db
    E = np.zeros((m, ns))
    E[I, np.arange(ns)] = 1.0
    K = np.zeros((nf + ns + m, nf + ns + m))
    K[:nf, :nf] = sgn * D.H[np.ix_(F, F)] + np.diag((sl + su)[F])
    K[nf:nf + ns, nf:nf + ns] = np.diag(sls + sus)
    K[nf + ns:, :nf] = D.A[:, F]
    K[nf + ns:, nf:nf + ns] = -E
    K[:nf + ns, nf + ns:] = K[nf + ns:, :nf + ns].T
    dx = np.zeros(n)
    if form == "plain":
        w = O._solve(K, np.concatenate([(base1 + sl * dl + su * du)[F], sls * dlc + sus * duc, base3]))
        dx[F] = w[:nf]
        dzl, dzu = -sl * (dx - dl), su * (dx - du)
        dx = dx + dxfix
    else:
        # "has a bound" is asked of the bounds, not of the sign of Sigma (adjoint_full_oracle)
        sm, sms = sl + su, sls + sus
        with np.errstate(divide="ignore", invalid="ignore"):
            bounded = (hasl | hasu) & (sm != 0)
            p = np.where(bounded, (sl * dl + su * du) / sm, 0.0)
            h = np.where(bounded, sl * su / sm, 0.0)
            ps = np.where(sms != 0, (sls * dlc + sus * duc) / sms, 0.0)
        w = O._solve(K, np.concatenate([(base1 - sgn * (D.H @ p))[F], np.zeros(ns), base3 - D.A @ p + E @ ps]))
        dxp = np.zeros(n)
        dxp[F] = w[:nf]
        dx = dxp + p + dxfix
        dzl, dzu = -sl * dxp + h * (dl - du), su * dxp + h * (dl - du)
    dzl, dzu = np.where(hasl, dzl, 0.0), np.where(hasu, dzu, 0.0)
    return {"x": dx, "y": w[nf + ns:], "zl": dzl, "zu": dzu, "cons": D.A @ dx + dA @ x}


def moved(qp, d, t):
    """qp with its data moved by t * d under the conventions above."""
    v, _, _ = _blocks(qp, d)
    fixed = np.asarray(qp.lvar) == np.asarray(qp.uvar)
    eq = np.asarray(qp.lcon) == np.asarray(qp.ucon)
    v["uvar"] = np.where(fixed, v["lvar"], v["uvar"])
    v["ucon"] = np.where(eq, v["lcon"], v["ucon"])
    new = {}
    for k in NAMES:
        base = np.array(getattr(qp, k), float)
        fin = np.isfinite(base)
        base[fin] += t * v[k][fin]
        new[k] = base
    return dataclasses.replace(qp, **new)


def finite_difference(qp, d, h=1e-6):
    """Central differences of (x, y, zl, zu, A x) through reference_ipm along `d`."""
    def at(t):
        q = moved(qp, d, t)
        pt = O.reference_ipm(q)
        return {"x": pt["x"], "y": pt["y"], "zl": pt["zl"], "zu": pt["zu"], "cons": O.dense(q).A @ pt["x"]}
    a, b = at(h), at(-h)
    return {k: (a[k] - b[k]) / (2 * h) for k in OUTS}


def max_err(t, ref, keys=OUTS):
    return max(O.err(t[k], ref[k]) for k in keys)


def dot(cot, t):
    """<cot, t> over the five output blocks (cot keyed gx, gy, gzl, gzu, gcons)."""
    pair = {"gx": "x", "gy": "y", "gzl": "zl", "gzu": "zu", "gcons": "cons"}
    return float(sum(np.asarray(cot[k], float) @ np.asarray(t[pair[k]], float) for k in cot))


def dot_data(g, qp, d):
    """<g, d> over the seven data blocks, the not-read entries of d left out."""
    v, _, _ = _blocks(qp, d)
    return float(sum(np.asarray(g[k], float) @ v[k] for k in NAMES if k in d))
