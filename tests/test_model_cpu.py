"""The MPC's problem model on the host (csrc/qp_model.cpp through build/model_check, no GPU).

model_check builds what setup_host, prepare_update, build_device_route and the adjoint upload, checks the
invariants between the arrays and prints / dumps them.  Here every array of small problems is compared
with a restatement in plain Python that walks the COO in input order (index arrays exactly, value arrays
bit for bit); a 2^22-entry problem gives the same digests on 1 and 8 analysis threads; the refusals of the
intake and the class-change checks of update() keep their texts.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_CHECK = os.path.join(ROOT, "build", "model_check")
INF = float("inf")
OPTS = dict(scaling=1, kkt_system=0, bound_relax_factor=1e-8, bound_push=1e-2, bound_fac=1e-2)

I64 = {"Hrp", "Jrp", "JTrp", "Kcp", "diag_pos", "Ccp", "cpp"}
U8 = {"fixed", "vcls", "ccls"}
F64 = {"x", "xl", "xu", "y", "rhs", "con_scale", "obj_scale", "c0s", "norm_b", "gfix", "cfix", "cs", "Hdiag", "Hv", "Jv",
       "JTv", "Kv"}
PAIRS = {"ae", "fe", "ge", "xe", "bfrc", "fh", "fa"}


def _dtype(name):
    return np.int64 if name in I64 else np.uint8 if name in U8 else np.float64 if name in F64 else np.int32


def qp(nx, m, A, H, c, lvar, uvar, lcon, ucon, x0=None, y0=None, c0=0.25, minimize=1):
    """A problem from lists of (row, col, value) triplets in input order."""
    A, H = list(A), list(H)
    f, i = (lambda v: np.asarray(v, dtype=np.float64)), (lambda v: np.asarray(v, dtype=np.int32))
    return dict(nx=nx, m=m, c0=float(c0), minimize=int(minimize), c=f(c), lvar=f(lvar), uvar=f(uvar), lcon=f(lcon),
                ucon=f(ucon), x0=f(np.zeros(nx) if x0 is None else x0), y0=f(np.zeros(m) if y0 is None else y0),
                Ar=i([t[0] for t in A]), Ac=i([t[1] for t in A]), Av=f([t[2] for t in A]),
                Hr=i([t[0] for t in H]), Hc=i([t[1] for t in H]), Hv=f([t[2] for t in H]))


def write_problem(path, p):
    with open(path, "wb") as f:
        f.write(f"madipm_qp {p['nx']} {p['m']} {len(p['Av'])} {len(p['Hv'])} {p['minimize']}\n".encode())
        np.float64(p["c0"]).tofile(f)
        for k in ("c", "lvar", "uvar", "x0", "lcon", "ucon", "y0", "Ar", "Ac", "Av", "Hr", "Hc", "Hv"):
            p[k].tofile(f)


def run(path, opts=OPTS, threads=1, dump=None, update=None):
    assert os.path.exists(MODEL_CHECK), "build/model_check is built by `make -C madipm.jl_amd/csrc` (build())"
    cmd = [MODEL_CHECK, str(path)] + [s for k, v in opts.items() for s in (f"--{k}", repr(v))]
    if dump:
        os.makedirs(dump, exist_ok=True)
        cmd += ["--dump", str(dump)]
    if update:
        cmd += ["--update", str(update)]
    e = {k: v for k, v in os.environ.items() if not k.startswith("MADIPM_")}
    e["MADIPM_ANALYSIS_THREADS"] = str(threads)
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=300)
    digests = {ln.split()[0]: tuple(ln.split()[1:]) for ln in p.stdout.splitlines()}
    return p.returncode, digests, p.stderr.strip()


# ----------------------------------------------------------------------------- the restatement
def _merge(nrow, coo):
    """CSR of a COO given as (row, col, value or None, source id) in input order: entries sorted by (row, col),
    duplicates summed in input order starting from the first; per entry the list of its source ids."""
    cells = {}
    for r, c, v, k in coo:
        if (r, c) in cells:
            cells[r, c][0] = cells[r, c][0] + v
            cells[r, c][1].append(k)
        else:
            cells[r, c] = [v, [k]]
    keys = sorted(cells)
    rp = np.zeros(nrow + 1, dtype=np.int64)
    for r, _ in keys:
        rp[r + 1] += 1
    return keys, np.cumsum(rp), [cells[k][0] for k in keys], [cells[k][1] for k in keys]


def _lists(nd, items):
    """(destination, (input index, other)) in input order -> list starts and the pairs, input order kept."""
    per = [[] for _ in range(nd)]
    for d, e in items:
        per[d].append(e)
    sp = np.cumsum([0] + [len(x) for x in per])
    return sp, [e for x in per for e in x]


def reference(p, o):
    nx, m = p["nx"], p["m"]
    c, lvar, uvar, lcon, ucon = p["c"], p["lvar"], p["uvar"], p["lcon"], p["ucon"]
    A = list(zip(p["Ar"].tolist(), p["Ac"].tolist(), [np.float64(v) for v in p["Av"]]))
    H = list(zip(p["Hr"].tolist(), p["Hc"].tolist(), [np.float64(v) for v in p["Hv"]]))
    sgn = np.float64(1.0 if p["minimize"] else -1.0)
    R = {}
    ineq = [i for i in range(m) if lcon[i] != ucon[i]]
    ns, n = len(ineq), nx + len(ineq)
    xl = np.concatenate([lvar, lcon[ineq]]).astype(np.float64)
    xu = np.concatenate([uvar, ucon[ineq]]).astype(np.float64)
    fixed = (xl == xu)
    ind_lb = [i for i in range(n) if not fixed[i] and xl[i] != -INF]
    ind_ub = [i for i in range(n) if not fixed[i] and xu[i] != INF]
    R.update(ind_ineq=ineq, ind_fixed=np.flatnonzero(fixed), ind_lb=ind_lb, ind_ub=ind_ub, fixed=fixed.astype(np.uint8))
    lbpos, ubpos = np.full(n, -1), np.full(n, -1)
    lbpos[ind_lb], ubpos[ind_ub] = np.arange(len(ind_lb)), np.arange(len(ind_ub))
    R.update(lbpos=lbpos, ubpos=ubpos)
    # ---- initialize: start, relaxed bounds, slack start A x (input order), bound push
    x = np.zeros(n)
    x[:nx] = p["x0"]
    x[fixed] = xl[fixed]
    rhs = np.where(lcon == ucon, lcon, 0.0)
    tol = o["bound_relax_factor"]
    for i in range(n):
        if fixed[i]:
            continue
        if np.isfinite(xl[i]):
            xl[i] = xl[i] - tol * max(1.0, abs(xl[i]))
        if np.isfinite(xu[i]):
            xu[i] = xu[i] + tol * max(1.0, abs(xu[i]))
    if ns:
        ax = np.zeros(m)
        for r, cc, v in A:
            ax[r] += v * x[cc]
        x[nx:] = ax[ineq]
    bp, bf = o["bound_push"], o["bound_fac"]
    for i in range(n):
        if fixed[i]:
            continue
        l, u, lo, hi = xl[i], xu[i], -INF, INF
        if np.isfinite(l):
            pl = bp * max(1.0, abs(l))
            lo = l + (min(pl, bf * (u - l)) if np.isfinite(u) else pl)
        if np.isfinite(u):
            pu = bp * max(1.0, abs(u))
            hi = u - (min(pu, bf * (u - l)) if np.isfinite(l) else pu)
        x[i] = min(max(x[i], lo), hi)
    # ---- set_scaling!
    obj_scale, cscale = np.float64(1.0), np.ones(m)
    if o["scaling"]:
        g = sgn * c
        for r, cc, v in H:
            w = sgn * v
            g[r] += w * x[cc]
            if r != cc:
                g[cc] += w * x[r]
        gmax = max([0.0] + [abs(v) for v in g])
        obj_scale = np.float64(min(1.0, 100.0 / gmax) if gmax > 0 else 1.0)
        rowmax = np.zeros(m)
        for r, cc, v in A:
            rowmax[r] = max(rowmax[r], abs(v))
        with np.errstate(divide="ignore"):
            cscale = np.minimum(1.0, 100.0 / rowmax)
        for k, r in enumerate(ineq):
            xl[nx + k] *= cscale[r]
            xu[nx + k] *= cscale[r]
            x[nx + k] *= cscale[r]
        rhs = rhs * cscale
    R.update(x=x, xl=xl, xu=xu, y=p["y0"], rhs=rhs, con_scale=cscale, obj_scale=[obj_scale])
    # ---- fixed variables' terms
    gfix, cfix, const_fixed = np.zeros(n), np.zeros(m), np.float64(0.0)
    for r, cc, v in H:
        fr, fc = fixed[r], fixed[cc]
        if not fr and not fc:
            continue
        w = obj_scale * sgn * v
        if fr and fc:
            const_fixed += np.float64(0.5 if r == cc else 1.0) * w * x[r] * x[cc]
            continue
        if not fr:
            gfix[r] += w * x[cc]
        if not fc:
            gfix[cc] += w * x[r]
    for r, cc, v in A:
        if fixed[cc]:
            cfix[r] += (cscale[r] * v) * x[cc]
    cs = np.zeros(n)
    cs[:nx] = obj_scale * sgn * c
    R.update(gfix=gfix, cfix=cfix, cs=cs, c0s=[obj_scale * (sgn * np.float64(p["c0"])) + const_fixed],
             norm_b=[max([0.0] + [abs(v) for v in rhs])])
    # ---- H (symmetric CSR of the free part), J, J^T
    hcoo, Hdiag = [], np.zeros(n)
    for k, (r, cc, v) in enumerate(H):
        if fixed[r] or fixed[cc]:
            continue
        w = obj_scale * sgn * v
        hcoo.append((r, cc, w, k))
        if r == cc:
            Hdiag[r] += w
        else:
            hcoo.append((cc, r, w, k))
    hkeys, Hrp, Hval, Hsrc = _merge(n, hcoo)
    jcoo = [(r, cc, cscale[r] * v, k) for k, (r, cc, v) in enumerate(A) if not fixed[cc]]
    jcoo += [(r, nx + k, np.float64(-1.0), -1) for k, r in enumerate(ineq)]
    jkeys, Jrp, Jval, _ = _merge(m, jcoo)
    tkeys, JTrp, JTval, Tsrc = _merge(n, [(cc, r, v, k) for r, cc, v, k in jcoo])
    R.update(Hdiag=Hdiag, Hrp=Hrp, Hci=[k[1] for k in hkeys], Hv=Hval, Jrp=Jrp, Jci=[k[1] for k in jkeys], Jv=Jval,
             JTrp=JTrp, JTci=[k[1] for k in tkeys], JTv=JTval)
    # ---- K2 lower CSC and the slots of H's and J^T's entries
    Kcp, Kri, Kv, hk, jtk = [0], [], [], [-1] * len(hkeys), [0] * len(tkeys)
    for j in range(n + m):
        Kri.append(j)
        Kv.append(0.0)
        if j < n:
            for t in range(Hrp[j], Hrp[j + 1]):
                if hkeys[t][1] > j:
                    hk[t] = len(Kri)
                    Kri.append(hkeys[t][1])
                    Kv.append(Hval[t])
            for t in range(JTrp[j], JTrp[j + 1]):
                jtk[t] = len(Kri)
                Kri.append(n + tkeys[t][1])
                Kv.append(JTval[t])
        Kcp.append(len(Kri))
    R.update(Kcp=Kcp, Kri=Kri, Kv=Kv, diag_pos=Kcp[:-1])
    if o["kkt_system"] == 1:
        R["kcol"] = [j for j in range(n + m) for _ in range(Kcp[j], Kcp[j + 1])]
    # ---- the refresh plan
    tpos = {k: t for t, k in enumerate(tkeys)}
    hdpos = np.full(n, -1)
    for t, (r, cc) in enumerate(hkeys):
        if r == cc:
            hdpos[r] = t
    R.update(tsp=np.cumsum([0] + [sum(k >= 0 for k in s) for s in Tsrc]), tsrc=[k for s in Tsrc for k in s if k >= 0],
             jtk=jtk, j2jt=[tpos[cc, r] for r, cc in jkeys], hsp=np.cumsum([0] + [len(s) for s in Hsrc]),
             hsrc=[k for s in Hsrc for k in s], hk=hk, hdpos=hdpos)
    # ---- the device route's lists and the adjoint's
    asp, ae = _lists(m, [(r, (k, cc)) for k, (r, cc, _) in enumerate(A)])
    fsp, fe = _lists(m, [(r, (k, cc)) for k, (r, cc, _) in enumerate(A) if fixed[cc]])
    gsp, ge = _lists(nx, [it for k, (r, cc, _) in enumerate(H)
                          for it in ([(r, (k, cc))] + ([(cc, (k, r))] if r != cc else []))])
    cross = [(k, (r, cc) if fixed[r] else (cc, r)) for k, (r, cc, _) in enumerate(H) if fixed[r] != fixed[cc]]
    xsp, xe = _lists(nx, [(fr, (k, fx)) for k, (fx, fr) in cross])
    both = [(k, r, cc) for k, (r, cc, _) in enumerate(H) if fixed[r] and fixed[cc]]
    cls = lambda l, u: 1 if l == u else (2 if l != -INF else 0) | (4 if u != INF else 0)
    R.update(asp=asp, ae=ae, fsp=fsp, fe=fe, gsp=gsp, ge=ge, xsp=xsp, xe=xe, bfk=[b[0] for b in both],
             bfrc=[b[1:] for b in both], vcls=[cls(l, u) for l, u in zip(lvar, uvar)],
             ccls=[cls(l, u) for l, u in zip(lcon, ucon)])
    rowslack = np.full(max(m, 1), -1)
    rowslack[ineq] = nx + np.arange(ns)
    fix = [i for i in range(nx) if fixed[i]]
    fhsp, fh = _lists(len(fix), [(fix.index(fx), (k, fr)) for k, (fx, fr) in cross])
    fasp, fa = _lists(len(fix), [(fix.index(cc), (k, r)) for k, (r, cc, _) in enumerate(A) if fixed[cc]])
    R.update(rowslack=rowslack, fix=fix, fhsp=fhsp, fh=fh, fasp=fasp, fa=fa)
    # ---- normal equations: tril(J J^T)'s pattern by columns, each entry's products in ascending k
    Ccp, Cri, cpp, cprod = [], [], [], []
    if o["kkt_system"] == 2:
        jpos = {k: t for t, k in enumerate(jkeys)}
        Jd = np.zeros((m, n), dtype=bool)
        for r, cc in jkeys:
            Jd[r, cc] = True
        Cd = (Jd.astype(np.int64) @ Jd.T.astype(np.int64)) > 0
        Ccp, cpp = [0], [0]
        for i in range(m):
            rows = [j for j in range(i, m) if Cd[j, i]] or [i]   # an empty row of A keeps its diagonal
            for j in rows:
                Cri.append(j)
                cprod += [(jpos[i, k], jpos[j, k]) for k in range(n) if Jd[i, k] and Jd[j, k]]
                cpp.append(len(cprod))
            Ccp.append(len(Cri))
    R.update(Ccp=Ccp, Cri=Cri, cpp=cpp, cprod=cprod)
    return R


def compare(p, tmp_path, name, **over):
    o = dict(OPTS, **over)
    path = tmp_path / f"{name}.qp"
    write_problem(path, p)
    rc, digests, err = run(path, o, dump=tmp_path / name)
    assert rc == 0, err
    want = reference(p, o)
    assert set(want) == set(digests), set(want) ^ set(digests)
    for k, w in want.items():
        got = np.fromfile(tmp_path / name / f"{k}.bin", dtype=_dtype(k))
        w = np.asarray(w, dtype=_dtype(k)).reshape(-1)
        assert got.shape == w.shape, (k, got, w)
        assert got.tobytes() == w.tobytes(), (k, got, w)   # indices exactly, values bit for bit
    return digests


# ----------------------------------------------------------------------------- the problems
# variables: free, lower-only, upper-only, boxed, fixed, fixed; rows: equality, ranged, one infinite side,
# empty ranged row, equality.  Row 0 of A arrives sorted, rows 1, 2 and 4 unsorted; (1, 3) and (4, 0) are
# duplicated.  H: duplicated diagonal (0, 0), duplicated (1, 0), free / free, fixed / fixed on and off the
# diagonal, fixed / free with the fixed variable as row and as column.  The values are no dyadic fractions,
# so that every sum depends on its order; 250 and 300 make both scalings bite.
A_MIX = [(0, 0, 1.1), (0, 1, 250.0), (0, 4, 0.5), (1, 3, 1.3), (1, 0, -2.7), (1, 3, 0.1), (1, 5, 3.3), (2, 2, 1.7),
         (2, 1, -0.3), (4, 5, 2.1), (4, 0, 0.7), (4, 0, 0.3), (2, 4, -0.7), (1, 3, 1e-17)]
H_MIX = [(0, 0, 2.3), (0, 0, 0.1), (1, 0, 0.3), (1, 0, 0.7), (3, 1, -0.2), (4, 4, 1.1), (5, 4, 0.4), (4, 0, 0.6),
         (5, 3, 0.9), (3, 3, 1.9), (4, 2, 0.35), (1, 0, 1e-17), (5, 0, -0.45)]
C_MIX = [300.0, -1.3, 0.7, 2.1, 1.1, -3.3]
X0_MIX, Y0_MIX = [0.3, -0.2, 5.0, 0.1, 9.0, 9.0], [0.1, -0.2, 0.3, 0.0, 0.7]
LCON, UCON = [2.1, -1.3, -INF, 0.1, 0.0], [2.1, 4.7, 5.3, 1.1, 0.0]


def mix(fixed=True, **kw):
    hi = [1.7, -0.6] if fixed else [1.9, 0.6]
    return qp(6, 5, A_MIX, H_MIX, C_MIX, [-INF, 0.3, -INF, -1.1, 1.7, -0.6], [INF, INF, 3.3, 2.3] + hi, LCON, UCON,
              X0_MIX, Y0_MIX, **kw)


def lp(fixed=False):
    p = mix(fixed)
    return dict(p, Hr=p["Hr"][:0], Hc=p["Hc"][:0], Hv=p["Hv"][:0])


def seeded(seed, nx=12, m=8, nfix=2):
    r = np.random.default_rng(seed)
    lvar, uvar = np.full(nx, -INF), np.full(nx, INF)
    kinds = r.integers(0, 4, nx)
    lvar[kinds % 2 == 1] = r.uniform(-2, 0, nx)[kinds % 2 == 1]
    uvar[kinds >= 2] = r.uniform(1, 3, nx)[kinds >= 2]
    for i in r.choice(nx, nfix, replace=False):
        lvar[i] = uvar[i] = r.uniform(-1, 1)
    lcon, ucon = r.uniform(-2, 0, m), r.uniform(1, 3, m)
    eq = r.random(m) < 0.4
    ucon[eq] = lcon[eq]
    lcon[~eq & (r.random(m) < 0.3)] = -INF
    na, nh = 40, 30
    A = list(zip(r.integers(0, m, na).tolist(), r.integers(0, nx, na).tolist(), r.uniform(-150, 150, na).tolist()))
    hr, hc = r.integers(0, nx, nh), r.integers(0, nx, nh)
    H = list(zip(np.maximum(hr, hc).tolist(), np.minimum(hr, hc).tolist(), r.uniform(-1, 1, nh).tolist()))
    return qp(nx, m, A, H, r.uniform(-200, 200, nx), lvar, uvar, lcon, ucon, r.uniform(-1, 1, nx), r.uniform(-1, 1, m))


CASES = {
    "mix_fixed": (lambda: mix(True), {}),                  # J from the filtered COO
    "mix_free": (lambda: mix(False), {}),                  # J read through the accessors
    "mix_fixed_noscale": (lambda: mix(True), dict(scaling=0)),
    "mix_free_noscale": (lambda: mix(False), dict(scaling=0)),
    "mix_fixed_max": (lambda: mix(True, minimize=0), {}),
    "mix_free_k25": (lambda: mix(False), dict(kkt_system=1)),
    "mix_fixed_k25": (lambda: mix(True), dict(kkt_system=1)),
    "lp_free_normal": (lambda: lp(False), dict(kkt_system=2)),
    "lp_fixed_normal": (lambda: lp(True), dict(kkt_system=2)),
    "lp_free": (lambda: lp(False), {}),                    # nnzh = 0
    "no_rows": (lambda: qp(3, 0, [], [(1, 0, 0.3), (2, 2, 1.1)], [1.0, 2.0, -0.5], [0.1, -INF, 1.0], [0.9, INF, 1.0], [], []),
                {}),                                       # m = 0, nnzj = 0
    "no_slack": (lambda: qp(3, 2, [(1, 2, 0.3), (0, 0, 1.1), (1, 0, 0.7)], [(1, 1, 0.9)], [1.0, 2.0, -0.5],
                            [0.1, -INF, -1.0], [0.9, INF, INF], [1.1, -0.3], [1.1, -0.3]), {}),   # ns = 0
    "empty_A": (lambda: qp(2, 2, [], [(1, 0, 0.3)], [1.0, 2.0], [0.1, -INF], [0.9, 2.0], [0.0, -1.0], [0.0, 1.0]),
                dict(kkt_system=1)),                       # nnzj = 0 with rows
    "empty_A_normal": (lambda: qp(2, 2, [], [], [1.0, 2.0], [0.1, -INF], [0.9, 2.0], [0.0, -1.0], [0.0, 1.0]),
                       dict(kkt_system=2)),
    "seeded_1": (lambda: seeded(1), {}),
    "seeded_2": (lambda: seeded(2, nfix=0), dict(kkt_system=1)),
    "seeded_3": (lambda: seeded(3, nx=9, m=5, nfix=3), dict(scaling=0, bound_relax_factor=1e-12)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_model_arrays_match_the_restatement(name, tmp_path):
    make, over = CASES[name]
    compare(make(), tmp_path, name, **over)


def test_refusals_keep_their_texts(tmp_path):
    def refused(p, **over):
        write_problem(tmp_path / "bad.qp", p)
        rc, _, err = run(tmp_path / "bad.qp", dict(OPTS, **over))
        assert rc == 2, (rc, err)
        return err

    assert refused(mix(True), kkt_system=2) == ("error: The KKT system NormalKKTSystem supports only linear programs. "
                                                "The problem has a positive number of nonzero in its Hessian.")
    p = mix(True)
    p["Ac"][3] = 6
    assert refused(p) == "error: A index out of range"
    p = mix(True)
    p["Ar"][0] = -1
    assert refused(p) == "error: A index out of range"
    p = mix(True)
    p["Hr"][2], p["Hc"][2] = 0, 1
    assert refused(p) == "error: H must be lower-triangular COO in range"
    assert refused(mix(True), kkt_system=3) == "error: unknown kkt_system"


TAIL = " (the classification of every bound is fixed at creation; nothing was changed)"
# (field, index, new value) -> message; variable 1 is lower-only, 2 upper-only, 0 free, 4 fixed; row 0 is an
# equality, row 1 ranged, row 2 has an infinite lower side
CLASS_CHANGES = {
    "eq_to_ranged": (("ucon", 0, 2.5), "constraint 0 was an equality (lcon == ucon) and would become ranged"),
    "ranged_to_eq": (("ucon", 1, -1.3), "constraint 1 was ranged (lcon != ucon) and would become an equality"),
    "fixed_to_free": (("uvar", 4, 1.9), "variable 4 was fixed (lower == upper bound) and would become free"),
    "free_to_fixed": (("uvar", 3, -1.1), "variable 3 was free (lower != upper bound) and would become fixed"),
    "lower_to_inf": (("lvar", 1, -INF), "variable 1 had a finite lower bound that would become infinite"),
    "lower_to_finite": (("lvar", 2, -4.0), "variable 2 had an infinite lower bound that would become finite"),
    "upper_to_inf": (("uvar", 2, INF), "variable 2 had a finite upper bound that would become infinite"),
    "upper_to_finite": (("uvar", 1, 4.0), "variable 1 had an infinite upper bound that would become finite"),
    "row_lower_to_finite": (("lcon", 2, -4.0), "constraint 2 had an infinite lower bound that would become finite"),
    "row_upper_to_inf": (("ucon", 1, INF), "constraint 1 had a finite upper bound that would become infinite"),
}


@pytest.mark.parametrize("name", list(CLASS_CHANGES))
def test_class_changes_are_refused(name, tmp_path):
    p = mix(True)
    write_problem(tmp_path / "p.qp", p)
    (field, idx, value), text = CLASS_CHANGES[name]
    new = {k: p[k].copy() for k in ("lvar", "uvar", "lcon", "ucon")}
    new[field][idx] = value
    with open(tmp_path / "u.bin", "wb") as f:
        for k in ("lvar", "uvar", "lcon", "ucon"):
            new[k].tofile(f)
    rc, _, err = run(tmp_path / "p.qp", update=tmp_path / "u.bin")
    assert (rc, err) == (2, "error: madipm_solver_update: " + text + TAIL)


def test_same_classes_are_accepted(tmp_path):
    p = mix(True)
    write_problem(tmp_path / "p.qp", p)
    with open(tmp_path / "u.bin", "wb") as f:   # other numbers, the same classes
        for k, d in (("lvar", 0.05), ("uvar", 0.05), ("lcon", -0.05), ("ucon", -0.05)):
            (p[k] + d).tofile(f)
    rc, _, err = run(tmp_path / "p.qp", update=tmp_path / "u.bin")
    assert rc == 0, err


@pytest.mark.parametrize("nfix", [0, 3])
def test_digests_do_not_depend_on_the_thread_count(nfix, tmp_path):
    """2^22 entries of A on 64 rows: par_range (grain 2^20) and csr_from_coo thread; the columns arrive in
    random order and every cell is hit about 20 times."""
    r = np.random.default_rng(7)
    nx, m, na, nh = 3000, 64, 1 << 22, 5000
    lvar, uvar = np.full(nx, -1.0), np.full(nx, 2.0)
    lvar[::7] = -INF
    uvar[::5] = INF
    uvar[:nfix] = lvar[:nfix] = 0.5
    lcon, ucon = np.full(m, -1.0), np.full(m, 1.0)
    ucon[::4] = -1.0
    hr, hc = r.integers(0, nx, nh), r.integers(0, nx, nh)
    p = dict(nx=nx, m=m, c0=0.0, minimize=1, c=r.uniform(-1, 1, nx), lvar=lvar, uvar=uvar, lcon=lcon, ucon=ucon,
             x0=r.uniform(-1, 1, nx), y0=np.zeros(m), Ar=r.integers(0, m, na).astype(np.int32),
             Ac=r.integers(0, nx, na).astype(np.int32), Av=r.uniform(-1, 1, na), Hr=np.maximum(hr, hc).astype(np.int32),
             Hc=np.minimum(hr, hc).astype(np.int32), Hv=r.uniform(-1, 1, nh))
    write_problem(tmp_path / "big.qp", p)
    rc1, d1, err1 = run(tmp_path / "big.qp", threads=1)
    rc8, d8, err8 = run(tmp_path / "big.qp", threads=8)
    assert (rc1, rc8) == (0, 0), (err1, err8)      # the invariants hold
    assert d1 and d1 == d8, {k: (d1[k], d8.get(k)) for k in d1 if d1[k] != d8.get(k)}
    assert int(d1["Jci"][0]) < na                  # duplicates were merged
