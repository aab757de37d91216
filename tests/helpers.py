"""Shared test helpers: seeded KKT matrices and problem generators (test data only)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def random_k2(m, n, density, seed, delta=1e-8, qp=False, well=False):
    """K2 = [H + Sigma, A^T; A, -delta I] with Sigma in [1e-2, 1e2]: quasi-definite.
    well=True: delta = 1e-2, Sigma in [0.1, 10] (O(1) element growth)."""
    rng = np.random.default_rng(seed)
    A = sp.random(m, n, density=density, random_state=rng, format="csr")
    A.data[:] = rng.standard_normal(A.nnz)
    sig = 10.0 ** rng.uniform(-1, 1, n) if well else 10.0 ** rng.uniform(-2, 2, n)
    if well:
        delta = 1e-2
    H = sp.diags(sig)
    if qp:
        B = sp.random(n, n, density=min(1.0, 3.0 / n), random_state=rng)
        H = H + B @ B.T
    K = sp.bmat([[H, A.T], [A, -delta * sp.eye(m)]]).tocsc()
    K.sum_duplicates()
    Lw = sp.tril(K).tocsc()
    Lw.sort_indices()
    return K, Lw


def block_angular_k2(m, n, nblocks, seed, coupling=0.02, delta=1e-8, well=False):
    """Structured stand-in: block-angular A with a few coupling rows."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    bn = n // nblocks
    for i in range(m):
        b = (i * nblocks) // m
        c = rng.integers(b * bn, (b + 1) * bn, size=6)
        if rng.random() < coupling:
            c = np.concatenate([c, rng.integers(0, n, size=20)])
        rows += [i] * len(c)
        cols += list(c)
    A = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(m, n))
    A.sum_duplicates()
    sig = 10.0 ** rng.uniform(-1, 1, n) if well else 10.0 ** rng.uniform(-2, 2, n)
    if well:
        delta = 1e-2
    K = sp.bmat([[sp.diags(sig), A.T], [A, -delta * sp.eye(m)]]).tocsc()
    K.sum_duplicates()
    Lw = sp.tril(K).tocsc()
    Lw.sort_indices()
    return K, Lw


def dense_k2(m, n, seed, delta=1e-2):
    """K2 of a QP with diagonal H and dense A (m x n): the x_j are single-column leaves with m-row
    updates (batched leaves); returns (K, lower CSC with sorted indices)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    sig = 10.0 ** rng.uniform(-1, 1, n)
    K = sp.bmat([[sp.diags(sig), sp.csr_matrix(A.T)], [sp.csr_matrix(A), -delta * sp.eye(m)]]).tocsc()
    K.sum_duplicates()
    Lw = sp.tril(K).tocsc()
    Lw.sort_indices()
    return K, Lw


def lp_k2(qp, seed, well=False, delta=1e-8):
    """K2 = [Sigma, A^T; A, -delta I] on the constraint matrix of a QuadraticModel (the benchmark
    stand-ins' structure: their fronts), Sigma as random_k2; returns (K, lower CSC sorted)."""
    rng = np.random.default_rng(seed)
    m, n = qp.ncon, qp.nvar
    A = sp.csr_matrix((np.asarray(qp.Avals, float), (np.asarray(qp.Arows), np.asarray(qp.Acols))), shape=(m, n))
    A.sum_duplicates()
    sig = 10.0 ** rng.uniform(-1, 1, n) if well else 10.0 ** rng.uniform(-2, 2, n)
    if well:
        delta = 1e-2
    K = sp.bmat([[sp.diags(sig), A.T], [A, -delta * sp.eye(m)]]).tocsc()
    K.sum_duplicates()
    Lw = sp.tril(K).tocsc()
    Lw.sort_indices()
    return K, Lw


def kkt_properties(qp, st):
    """Optimality measures of (x, y, zl, zu) for min/max c'x + x'Hx/2 + c0, Ax = b, l <= x <= u
    (unscaled).  The multipliers are those of the problem the solver minimises, sigma f with
    sigma = +1 (minimise) / -1 (maximise) (MadNLP's objective sign [EXT]; the reference flips only the
    reported objective back, /root/reference/src/utils.jl:150-156): stationarity
    sigma (c + Hx) + A'y - zl + zu = 0, and the dual bound of min sigma f,
    sigma c0 - y'b + zl'l - zu'u - sigma x'Hx/2 (src/kernels.jl:408-430), is reported in the
    problem's own sense (times sigma) so that it compares with the primal objective."""
    import scipy.sparse as sp
    n, m = qp.nvar, qp.ncon
    sg = 1.0 if getattr(qp, "minimize", True) else -1.0
    A = sp.csr_matrix((qp.Avals, (qp.Arows, qp.Acols)), shape=(m, n))
    x, y, zl, zu = st.solution, st.multipliers, st.multipliers_L, st.multipliers_U
    hx = np.zeros(n)
    np.add.at(hx, qp.Hrows, qp.Hvals * x[qp.Hcols])
    off = qp.Hrows != qp.Hcols
    np.add.at(hx, qp.Hcols[off], qp.Hvals[off] * x[qp.Hrows[off]])
    b = qp.lcon
    pr = np.max(np.abs(A @ x - b)) / (1.0 + np.max(np.abs(b)))
    g = sg * (qp.c + hx)
    du = np.max(np.abs(g + A.T @ y - zl + zu)) / (1.0 + np.max(np.abs(qp.c)))
    lo, hi = np.isfinite(qp.lvar), np.isfinite(qp.uvar)
    compl = max(np.max(np.abs((x - qp.lvar)[lo] * zl[lo]), initial=0.0),
                np.max(np.abs((qp.uvar - x)[hi] * zu[hi]), initial=0.0))
    pobj = qp.c0 + qp.c @ x + 0.5 * x @ hx
    dobj = sg * (sg * qp.c0 - y @ b + zl[lo] @ qp.lvar[lo] - zu[hi] @ qp.uvar[hi] - sg * 0.5 * x @ hx)
    return dict(pr=pr, du=du, compl=compl, pobj=pobj, dobj=dobj,
                bounds=max(np.max((qp.lvar - x)[lo], initial=-1.0), np.max((x - qp.uvar)[hi], initial=-1.0)),
                zmin=min(np.min(zl[lo], initial=0.0), np.min(zu[hi], initial=0.0)))


def many_leaf_k2(n, seed=0):
    """K2 of an LP with one constraint row over n columns (delta = 1e-2, well conditioned): every x_j is
    a two-row micro leaf (x_j, y) under the one tree front y, which folds all n of them — more than
    k_fact_tree's fold_leaves holds per batch (2 x 512 leaf-table registers) once n > 1024."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    A = sp.csr_matrix(rng.uniform(0.5, 1.5, (1, n)))
    K = sp.bmat([[sp.diags(10.0 ** rng.uniform(-1, 1, n)), A.T], [A, -1e-2 * sp.eye(1)]]).tocsc()
    K.sum_duplicates()
    Lw = sp.tril(K).tocsc()
    Lw.sort_indices()
    return K, Lw


# ---------------------------------------------------------------- general-form problems for the
# returned-point tests (test_mpc_point_gpu.py; pinned on the oracle in test_point_helpers_cpu.py)
def scaled_general(kind, minimize=True):
    """A general-form LP / QP on which set_scaling! does scale (obj_scale < 1, con_scale < 1 on some
    rows), with fixed variables, an objective constant, a non-zero x0 and, for minimize=False, the
    maximisation of the negated objective (the same point; objective c0 - (min - c0)).

    Base: random_lp(60, 120, 0.05, 0, ineq_frac=0.3, free_frac=0.05) / random_qp(40, 90, 0.08, 3).
    Rows are multiplied by 10**U(0, 4) (30 % of them kept at 1), c and H by 1e3, c0 = 7.5, variables 3
    and 17 are fixed (at 0.5 when their upper bound was finite, else at 1)."""
    from madipm_amd.instances import random_lp, random_qp
    from madipm_amd.qp import QuadraticModel
    base = {"lp": lambda: random_lp(60, 120, 0.05, 0, ineq_frac=0.3, free_frac=0.05),
            "qp": lambda: random_qp(40, 90, 0.08, 3)}[kind]()
    rng = np.random.default_rng(11)
    m, n = base.ncon, base.nvar
    fac = 10.0 ** rng.uniform(0.0, 4.0, m)
    fac[rng.random(m) < 0.3] = 1.0
    lvar, uvar = base.lvar.copy(), base.uvar.copy()
    for j in (3, 17):
        lvar[j] = uvar[j] = 0.5 if np.isfinite(base.uvar[j]) else 1.0
    sg = 1.0 if minimize else -1.0
    return QuadraticModel(c=sg * 1e3 * base.c, Hrows=base.Hrows, Hcols=base.Hcols, Hvals=sg * 1e3 * base.Hvals,
                          Arows=base.Arows, Acols=base.Acols, Avals=base.Avals * fac[base.Arows],
                          lcon=base.lcon * fac, ucon=base.ucon * fac, lvar=lvar, uvar=uvar,
                          c0=7.5, x0=rng.uniform(0.1, 1.0, n), minimize=minimize,
                          name=f"scaled_{kind}_{'min' if minimize else 'max'}")


ROWLEN_LENGTHS = (1, 3, 4, 5, 8, 9, 19, 32, 33, 64, 65, 129, 131)


def rowlen_qp(seed=0, hess=True):
    """n = 200, m = 39: A's row lengths are ROWLEN_LENGTHS x 3 — around every lane-group width G of the
    SpMV kernels (1, G - 1, G, G + 1, 2G, 2G + 1, > 4G for G = 4 .. 64).  Column 0 is in every row (a
    J^T row of 39 entries), the other columns of a row are drawn without replacement.  Bounds, free
    variables, inequality / ranged rows and the feasible, bounded construction are random_lp's
    (b = A x0, c = A^T y0 + z0 - H x0).  hess=True: H = diag(U[1e-2, 1]) + sparse B B^T + v v^T with v on
    70 variables (H rows of ~70 entries; the mean row of [H A^T; A] then selects G = 32, without H 8)."""
    from madipm_amd.qp import QuadraticModel
    rng = np.random.default_rng(seed)
    n, lens = 200, np.tile(ROWLEN_LENGTHS, 3)
    m = len(lens)
    rows, cols = [], []
    for i, ln in enumerate(lens):
        rows += [i] * int(ln)
        cols += [0] + list(1 + rng.choice(n - 1, int(ln) - 1, replace=False))
    vals = rng.standard_normal(len(rows))
    vals[np.abs(vals) < 0.1] = 0.5
    A = sp.coo_matrix((vals, (rows, cols)), shape=(m, n)).tocsr()
    lvar = np.zeros(n)
    uvar = np.where(rng.random(n) < 0.5, rng.uniform(1.0, 5.0, n), np.inf)
    free = rng.random(n) < 0.05
    lvar[free], uvar[free] = -np.inf, np.inf
    x0 = np.where(np.isfinite(uvar), uvar * rng.uniform(0.2, 0.8, n), rng.uniform(0.5, 2.0, n))
    x0[free] = rng.standard_normal(free.sum())
    b = A @ x0
    y0 = rng.standard_normal(m)
    z0 = rng.uniform(0.0, 1.0, n)
    z0[free] = 0.0
    c = A.T @ y0 + z0
    lcon, ucon = b.copy(), b.copy()
    ineq = rng.random(m) < 0.3
    lcon[ineq] = b[ineq] - rng.uniform(0.1, 1.0, ineq.sum())
    ucon[ineq] = np.where(rng.random(ineq.sum()) < 0.5, np.inf, b[ineq] + rng.uniform(0.1, 1.0, ineq.sum()))
    Hr = Hc = Hv = []
    if hess:
        B = sp.random(n, n // 4, density=3.0 / n, random_state=rng)
        v = np.zeros(n)
        v[rng.choice(n, 70, replace=False)] = rng.uniform(0.1, 0.5, 70)
        H = sp.diags(rng.uniform(1e-2, 1.0, n)) + B @ B.T + sp.csr_matrix(np.outer(v, v))
        c = c - H @ x0
        Hl = sp.tril(H).tocoo()
        Hr, Hc, Hv = Hl.row, Hl.col, Hl.data
    Ac = A.tocoo()
    return QuadraticModel(c=c, Hrows=Hr, Hcols=Hc, Hvals=Hv, Arows=Ac.row, Acols=Ac.col, Avals=Ac.data,
                          lcon=lcon, ucon=ucon, lvar=lvar, uvar=uvar, x0=rng.uniform(0.1, 1.0, n),
                          name=f"rowlen_{'qp' if hess else 'lp'}_s{seed}")


def spmv_mean_row(qp):
    """Mean row length of [H A^T; A] (H symmetric in full, A with its slack columns): the figure
    MPCSolver picks the SpMV lane-group width from, and that width (4 doubled while 2 G < mean, <= 64).
    For problems without fixed variables (their rows and columns would leave H and A)."""
    assert not np.any(qp.lvar == qp.uvar)
    H = sp.coo_matrix((np.ones(qp.nnzh), (qp.Hrows, qp.Hcols)), shape=(qp.nvar, qp.nvar)).tocsr()
    nnzh = (H + H.T).nnz
    A = sp.coo_matrix((np.ones(qp.nnzj), (qp.Arows, qp.Acols)), shape=(qp.ncon, qp.nvar)).tocsr()
    ns = int(np.sum(qp.lcon != qp.ucon))
    mean = (nnzh + 2.0 * (A.nnz + ns)) / max(1, qp.nvar + ns + qp.ncon)
    g = 4
    while g < 64 and 2 * g < mean:
        g *= 2
    return mean, g


def _dense_pd(n, rng):
    P = rng.standard_normal((n, n))
    H = P @ P.T / n + np.eye(n)
    r, c = np.tril_indices(n)
    return H, r, c, H[r, c]


def free_eq_qp():
    """n = 30 free variables, m = 10 equality rows, dense positive definite H = P P^T / n + I: no bounded
    coordinate at all (nlb = nub = 0).  Returns (qp, x, y, objective) with the exact solution of
    [H A^T; A 0] [x; y] = [-c; b] (the solver's sign of y: c + H x + A^T y = 0)."""
    from madipm_amd.qp import QuadraticModel
    rng = np.random.default_rng(5)
    n, m = 30, 10
    H, r, c_, hv = _dense_pd(n, rng)
    c = rng.standard_normal(n)
    A = rng.standard_normal((m, n))
    b = rng.standard_normal(m)
    K = np.block([[H, A.T], [A, np.zeros((m, m))]])
    sol = np.linalg.solve(K, np.concatenate([-c, b]))
    x, y = sol[:n], sol[n:]
    ar, ac = np.nonzero(A)
    qp = QuadraticModel(c=c, Hrows=r, Hcols=c_, Hvals=hv, Arows=ar, Acols=ac, Avals=A[ar, ac], lcon=b, ucon=b.copy(),
                        lvar=np.full(n, -np.inf), uvar=np.full(n, np.inf), name="free_eq_qp")
    return qp, x, y, float(c @ x + 0.5 * x @ H @ x)


def box_qp():
    """free_eq_qp's H and c with no constraint at all (m = 0) and 0 <= x <= 1."""
    from madipm_amd.qp import QuadraticModel
    rng = np.random.default_rng(5)
    n = 30
    H, r, c_, hv = _dense_pd(n, rng)
    c = rng.standard_normal(n)
    return QuadraticModel(c=c, Hrows=r, Hcols=c_, Hvals=hv, Arows=[], Acols=[], Avals=[], lcon=[], ucon=[],
                          lvar=np.zeros(n), uvar=np.ones(n), name="box_qp")


def kkt_properties_general(qp, st):
    """Optimality certificate of a returned point (x, y, zl, zu, constraints) on the unscaled
    general-form problem min/max c0 + c'x + x'Hx/2, lcon <= Ax <= ucon, lvar <= x <= uvar, in the solver's
    sign convention (kkt_properties: the multipliers are those of min sigma f, sigma = -1 for
    maximisation).  An inequality row i has the slack s_i = (Ax)_i in [lcon_i, ucon_i], whose
    stationarity gives y_i = z_upper - z_lower: y_i >= 0 without a lower side, <= 0 without an upper.

      du      |sigma (c + Hx) + A'y - zl + zu| over the non-fixed variables / (1 + |c|_inf)
      cons    |constraints - Ax|_i / (|A||x|)_i, the worst row
      pr      the worst row violation of lcon <= Ax <= ucon / max(1, (|A||x|)_i)
      bounds  the worst violation of lvar <= x <= uvar (negative inside)
      zmin    the smallest of zl, zu on their bounded coordinates
      ysign   the wrong-signed part of y on the one-sided rows / (1 + |c|_inf)  (the slack's part of du)
      zoff    the largest |zl|, |zu| where they must vanish: fixed variables and absent bounds
      compl   the largest product multiplier x distance, over variable bounds and row sides
      pobj    the objective at x;  dobj: the dual bound (fixed variables enter with their reduced cost)
    """
    n, m = qp.nvar, qp.ncon
    sg = 1.0 if getattr(qp, "minimize", True) else -1.0
    A = sp.csr_matrix((qp.Avals, (qp.Arows, qp.Acols)), shape=(m, n))
    x, y, zl, zu = st.solution, st.multipliers, st.multipliers_L, st.multipliers_U
    assert len(x) == len(zl) == len(zu) == n and len(y) == len(st.constraints) == m
    hx = np.zeros(n)
    np.add.at(hx, qp.Hrows, qp.Hvals * x[qp.Hcols])
    off = qp.Hrows != qp.Hcols
    np.add.at(hx, qp.Hcols[off], qp.Hvals[off] * x[qp.Hrows[off]])
    fixed = qp.lvar == qp.uvar
    lo = np.isfinite(qp.lvar) & ~fixed
    hi = np.isfinite(qp.uvar) & ~fixed
    r = sg * (qp.c + hx) + A.T @ y - zl + zu
    du = np.max(np.abs(r[~fixed]), initial=0.0) / (1.0 + np.max(np.abs(qp.c), initial=0.0))
    ax = A @ x
    absax = abs(A) @ np.abs(x)
    cons = np.max(np.abs(st.constraints - ax) / np.where(absax > 0, absax, 1.0), initial=0.0)
    with np.errstate(invalid="ignore"):
        viol = np.maximum(np.maximum(qp.lcon - ax, ax - qp.ucon), 0.0)
    pr = np.max(viol / np.maximum(1.0, absax), initial=0.0)
    bounds = max(np.max((qp.lvar - x)[lo | fixed], initial=-1.0), np.max((x - qp.uvar)[hi | fixed], initial=-1.0))
    ineq = qp.lcon != qp.ucon
    rlo, rhi = ineq & np.isfinite(qp.lcon), ineq & np.isfinite(qp.ucon)
    zrl, zru = np.maximum(-y, 0.0), np.maximum(y, 0.0)            # the slack's z_lower / z_upper
    zmin = min(np.min(zl[lo], initial=0.0), np.min(zu[hi], initial=0.0))
    # y is stepped on its own, so its sign on a one-sided row holds to the slack's dual residual: as du
    ysign = max(np.max(-y[ineq & ~rlo], initial=0.0), np.max(y[ineq & ~rhi], initial=0.0)) \
        / (1.0 + np.max(np.abs(qp.c), initial=0.0))
    zoff = max(np.max(np.abs(zl[~lo]), initial=0.0), np.max(np.abs(zu[~hi]), initial=0.0))
    compl = max(np.max(np.abs((x - qp.lvar)[lo] * zl[lo]), initial=0.0),
                np.max(np.abs((qp.uvar - x)[hi] * zu[hi]), initial=0.0),
                np.max(np.abs(zrl[rlo] * (ax - qp.lcon)[rlo]), initial=0.0),
                np.max(np.abs(zru[rhi] * (qp.ucon - ax)[rhi]), initial=0.0))
    pobj = qp.c0 + qp.c @ x + 0.5 * x @ hx
    dmin = (sg * qp.c0 - y[~ineq] @ qp.lcon[~ineq] + zrl[rlo] @ qp.lcon[rlo] - zru[rhi] @ qp.ucon[rhi]
            + zl[lo] @ qp.lvar[lo] - zu[hi] @ qp.uvar[hi] + r[fixed] @ x[fixed] - sg * 0.5 * x @ hx)
    return dict(pr=pr, du=du, cons=cons, bounds=bounds, zmin=zmin, ysign=ysign, zoff=zoff, compl=compl, pobj=pobj, dobj=sg * dmin)


def assert_certificate(qp, st, objective):
    """The thresholds of test_fullsize_vs_oracle on the general-form certificate.  cons: a row of <= 131
    entries summed in any order, scaled and un-scaled by con_scale, is within (131 + 3) eps ~ 3e-14 of
    |A||x|; ysign is the slack's share of the dual residual (as du); zoff is exact."""
    p = kkt_properties_general(qp, st)
    assert p["pr"] <= 1e-6 and p["du"] <= 1e-6 and p["ysign"] <= 1e-6, p
    assert p["cons"] <= 1e-13, p
    assert p["bounds"] <= 1e-8 and p["zmin"] >= -1e-10 and p["zoff"] == 0.0, p
    assert abs(p["pobj"] - p["dobj"]) <= 1e-6 * max(1.0, abs(p["pobj"])), p
    assert abs(p["pobj"] - objective) <= 1e-9 * max(1.0, abs(p["pobj"])), (p["pobj"], objective)
    return p


# ---------------------------------------------------------------- prescribed front trees for the
# LDL^T shape sweep (test_ldl_shapes_gpu.py; pinned on the host in test_front_tree_cpu.py)
FRONT_TREE_OPTS = dict(ordering=0, relax=0)   # with MADIPM_BIG_MERGE=0: the supernodes are the nodes


def front_tree_nodes(root):
    """The nodes of a front tree (w, b, children) in postorder, the numbering of front_tree_k2: dicts
    with first (the node's first column), w, r = w + b, parent (postorder index, -1 at the root),
    depth, children (indices) and rows (the b global indices of its rows below the diagonal block)."""
    nodes = []

    def visit(node, depth):
        w, b, children = node
        kids = [visit(c, depth + 1) for c in children]
        me = len(nodes)
        first = nodes[-1]["first"] + nodes[-1]["w"] if nodes else 0
        nodes.append(dict(first=first, w=int(w), b=int(b), r=int(w + b), parent=-1, depth=depth, children=kids))
        for k in kids:
            nodes[k]["parent"] = me
        return me

    visit(root, 0)
    assert nodes[-1]["b"] == 0, "the root has no rows below it"
    for nd in nodes:
        if nd["parent"] < 0:
            nd["rows"] = np.zeros(0, np.int64)
            continue
        p, b = nodes[nd["parent"]], nd["b"]
        assert 1 <= b <= p["w"], (nd, p)
        assert len(p["children"]) >= 2, "a non-leaf needs two children on its column 0 to stay a supernode"
        # the parent's column 0 and an even spread of its other columns: distinct because b - 1 <= w_p - 1
        local = np.r_[0, 1 + (np.arange(b - 1) * (p["w"] - 1)) // max(1, b - 1)].astype(np.int64)
        assert len(np.unique(local)) == b and local.max() < p["w"]
        nd["rows"] = p["first"] + local
    return nodes


def front_tree_k2(root, seed):
    """A quasi-definite matrix whose multifrontal fronts are prescribed.  A node is (w, b, children): a
    dense w x w diagonal block +-(B B^T / w + I) 10^U(-0.5, 0.5), the sign alternating by depth (+ at
    the root), and, for a non-root node, a dense b x w coupling block N(0, 1) / sqrt(w + b) in b of its
    parent's w columns (column 0 and an even spread of the others: relative indices with gaps).
    Postorder numbering.  Every non-leaf has >= 2 children, all reaching its column 0, so with
    FRONT_TREE_OPTS and MADIPM_BIG_MERGE=0 the supernodes are the nodes: (w, r) = (w, w + b).
    Returns (K, lower CSC with sorted indices, nodes of front_tree_nodes)."""
    nodes = front_tree_nodes(root)
    rng = np.random.default_rng(seed)
    N = nodes[-1]["first"] + nodes[-1]["w"]
    Kd = np.zeros((N, N))
    for nd in nodes:
        f, w, b = nd["first"], nd["w"], nd["b"]
        B = rng.standard_normal((w, w))
        sign = 1.0 if nd["depth"] % 2 == 0 else -1.0
        Kd[f:f + w, f:f + w] = sign * (B @ B.T / w + np.eye(w)) * 10.0 ** rng.uniform(-0.5, 0.5)
        if b:
            Cb = rng.standard_normal((b, w)) / np.sqrt(w + b)
            Kd[nd["rows"], f:f + w] = Cb
            Kd[f:f + w, nd["rows"]] = Cb.T
    K = sp.csc_matrix(Kd)
    K.sort_indices()
    Lw = sp.tril(K).tocsc()
    Lw.sort_indices()
    return K, Lw, nodes


def fronts_in_pivot_order(nodes, perm, first, parent, nrows):
    """Matches the analysis' supernodes (first, parent, nrows in pivot order; perm[k] = the column
    eliminated k-th) to the prescribed nodes and asserts that they ARE the nodes: each supernode holds
    exactly one node's columns in order, with its r and its parent.  Returns (node_of[s], front_of[k]):
    the node of supernode s and the supernode of pivot k."""
    by_first = {nd["first"]: i for i, nd in enumerate(nodes)}
    ns = len(nrows)
    assert ns == len(nodes), (ns, len(nodes))
    node_of = []
    for s in range(ns):
        cols = np.asarray(perm[first[s]:first[s + 1]])
        i = by_first.get(int(cols[0]), -1)
        assert i >= 0, f"supernode {s} starts at column {cols[0]}, inside a node"
        nd = nodes[i]
        assert np.array_equal(cols, nd["first"] + np.arange(nd["w"])) and nrows[s] == nd["r"], \
            f"supernode {s}: w={len(cols)} r={nrows[s]}, node {i} has w={nd['w']} r={nd['r']}"
        node_of.append(i)
    for s in range(ns):
        want = nodes[node_of[s]]["parent"]
        assert (parent[s] < 0 and want < 0) or (parent[s] >= 0 and node_of[parent[s]] == want), (s, parent[s], want)
    return node_of, np.repeat(np.arange(ns), np.diff(first))


def front_tree_classes(nodes, small_front_max=128, tree_fact=True):
    """info()'s nbig, tree_fronts, tree_medium and max_front for prescribed fronts, restating the
    unsharded planner without batched leaf columns (csrc/symbolic.hpp thresholds, symbolic.cpp's storage
    and factorisation-tree passes): a front is big when r > small_front_max; a tree front has r <= 256, is
    no childless front of r <= 32 (a pre-leaf), has only pre-leaves and tree fronts as children and at
    most 8 tree children; medium tree fronts have r > 192.  fold_fronts / fold_leaves: the tree fronts of
    r <= 192 whose pre-leaf children are all micro leaves (w <= 2, r <= 32), which they fold, and those
    leaves (few enough here to fit the LDS carve).  Also returns the per-node tree flags."""
    ftree = [False] * len(nodes)
    for s, nd in enumerate(nodes):       # postorder: children first
        if not tree_fact or nd["r"] > 256 or (not nd["children"] and nd["r"] <= 32):
            continue
        ok = all(ftree[c] or (not nodes[c]["children"] and nodes[c]["r"] <= 32) for c in nd["children"])
        ftree[s] = ok and sum(ftree[c] for c in nd["children"]) <= 8
    fold_fronts = fold_leaves = 0
    for s, nd in enumerate(nodes):
        pre = [nodes[c] for c in nd["children"] if not ftree[c]]
        if ftree[s] and nd["r"] <= 192 and pre and all(c["w"] <= 2 and c["r"] <= 32 for c in pre):
            fold_fronts += 1
            fold_leaves += len(pre)
    return dict(nbig=sum(nd["r"] > small_front_max for nd in nodes), tree_fronts=sum(ftree),
                tree_medium=sum(f and nd["r"] > 192 for f, nd in zip(ftree, nodes)),
                max_front=max(nd["r"] for nd in nodes), fold_fronts=fold_fronts, fold_leaves=fold_leaves), ftree


class FrontTreeCase:
    """A prescribed-front matrix (front_tree_k2), the right-hand sides of the GPU sweeps — a random b,
    e_j of the first leaf's first pivot, e_{N-1}, as one contiguous (3, N) block — and the prescribed
    count of positive pivots (the columns of the blocks at even depth)."""

    def __init__(self, root, seed):
        self.root = root
        self.K, self.Lw, self.nodes = front_tree_k2(root, seed)
        self.N = self.K.shape[0]
        rng = np.random.default_rng(seed + 2)
        self.B = np.zeros((3, self.N))
        self.B[0] = rng.standard_normal(self.N)
        self.B[1, self.nodes[0]["first"]] = 1.0
        self.B[2, self.N - 1] = 1.0
        self.pos = sum(nd["w"] for nd in self.nodes if nd["depth"] % 2 == 0)
        self.firsts = np.array([nd["first"] for nd in self.nodes])

    def node_of_pivot(self, perm, k):
        return int(np.searchsorted(self.firsts, perm[k], side="right") - 1)

    def front_of_pivot(self, perm, k):
        i = self.node_of_pivot(perm, k)
        return f"front {i} (w={self.nodes[i]['w']}, r={self.nodes[i]['r']})"


def assert_front_tree_plan(info, nodes, sfm, tree_fact, tag):
    """A solver's info() has the classes that the prescribed fronts stand for (front_tree_classes), one
    supernode per node and no batched leaf columns: a case that no longer reaches its path fails."""
    want, _ = front_tree_classes(nodes, sfm, tree_fact)
    got = {k: info[k] for k in want}
    assert got == want and info["nsuper"] == len(nodes) and info["lb_groups"] == 0, \
        f"{tag}: the plan misses its classes: {got} (nsuper {info['nsuper']}), prescribed {want}"


LEAF_SHAPE_R = (2, 3, 17, 32, 33, 48, 64, 65, 96, 128, 129, 160, 191, 192, 193, 224, 256, 257, 300)


def leaf_shape_widths(r):
    """The pivot-column counts swept at r front rows: around the micro path (w <= 2), the 16-column
    in-LDS pivot blocks, the 64-column panels and tiles, 128, and update blocks of 1, 16 and 17 rows."""
    return sorted({w for w in (1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 127, 128, 129, r - 17, r - 16, r - 1)
                   if 1 <= w <= r - 1})


def leaf_shape_tree(r, w):
    """Three leaves under one dense root: two of (w, r), one with half the columns and the same update
    rows; the root has max b + 3 columns (r = w)."""
    b = r - w
    return (b + 3, 0, [(w, b, []), (w, b, []), (max(1, w // 2), b, [])])


# (w_m, b_m) of the mids, k leaves each of (w, b): three mids per tree under a root of max b_m + 3 columns
ASSEMBLY_TREES = {
    # every child a micro leaf (w <= 2, r <= 32): the fold; k = 9 pre-leaves are no fan-in
    "micro_fold": [((16, 8), 2, (1, 1)), ((40, 33), 8, (2, 7)), ((64, 64), 9, (1, 1))],
    # pre-leaves that are no micro leaves (w = 3) next to r = 33 tree children, fan-in 8 and 9
    "preleaf_vs_tree": [((16, 8), 9, (3, 16)), ((40, 33), 8, (17, 16)), ((40, 33), 9, (17, 16))],
    "fanin_lds": [((64, 64), 8, (33, 40)), ((64, 64), 9, (33, 40)), ((100, 30), 2, (64, 64))],
    "fanin_packed": [((100, 30), 8, (17, 16)), ((100, 30), 9, (65, 100)), ((130, 129), 2, (65, 100))],
    # 128 / 129 update rows: gathered versus block-wise children, at the leaves and at the mids
    "gather_128_129": [((130, 129), 2, (129, 129)), ((130, 129), 8, (64, 64)), ((200, 57), 2, (129, 129))],
    "medium_mids": [((200, 57), 8, (33, 40)), ((200, 57), 9, (17, 16)), ((130, 129), 9, (3, 16))],
    "big_mids": [((257, 100), 2, (65, 100)), ((257, 100), 8, (2, 7)), ((257, 100), 9, (33, 40))],
    "big_mixed": [((257, 100), 2, (129, 129)), ((200, 57), 2, (64, 64)), ((16, 8), 8, (1, 1))],
}


def assembly_tree(name):
    mids = ASSEMBLY_TREES[name]
    for (wm, bm), k, (w, b) in mids:
        assert b <= wm and k in (2, 8, 9)
    return (max(bm for (_, bm), _, _ in mids) + 3, 0, [(wm, bm, [(w, b, [])] * k) for (wm, bm), k, (w, b) in mids])


def perturbed_values(Lw, seed):
    """vals * (1 + 0.3 U(0, 1)) per stored lower entry (the refactorisation's new matrix) and the
    symmetric K of those values."""
    vals2 = Lw.data * (1.0 + 0.3 * np.random.default_rng(seed).uniform(0.0, 1.0, Lw.nnz))
    L2 = sp.csc_matrix((vals2, Lw.indices, Lw.indptr), shape=Lw.shape)
    K2 = (L2 + sp.tril(L2, -1).T).tocsc()
    K2.sort_indices()
    return vals2, K2


def dense_ldlt_longdouble(K):
    """Pivots of the no-pivot LDL^T of a symmetric matrix in np.longdouble, right-looking on dense
    storage (a column's structural zeros are skipped: their updates are exact zeros)."""
    A = np.asarray(K.todense() if sp.issparse(K) else K).astype(np.longdouble)
    n = A.shape[0]
    d = np.empty(n, np.longdouble)
    for k in range(n):
        d[k] = A[k, k]
        idx = k + 1 + np.flatnonzero(A[k + 1:, k])
        if idx.size:
            a = A[idx, k]
            A[np.ix_(idx, idx)] -= np.outer(a / d[k], a)
    return d


# ---------------------------------------------------------------- planted pivot failures
# (test_ldl_pivot_failure_gpu.py; pinned on the oracle in test_pivot_plants_cpu.py)
PLANT_TOL = 1e-8          # the solvers' pivot_tol for tiny plants: six decades above the planted |d_k|
                          # (<= 1e-12, pinned), seven below the smallest good pivot (>= 0.1, pinned)
PLANT_COLUMNS = (0, 16, 17, 64, 65)   # and w - 1: pivot-block and panel boundaries of a front
EXACT_VALUES = (0.0, -0.0, float("nan"), float("inf"))

# the trees of the failed-pivot tests: (name, root, seed), the shape sweep's matrices (same seeds)
PLANT_LEAF_SHAPES = ((32, 2), (32, 16), (64, 17), (128, 65), (192, 64), (224, 65), (300, 129))
PLANT_ASSEMBLY = ("micro_fold", "big_mixed", "medium_mids")
EXACT_LEAF_SHAPES = ((32, 2), (32, 16), (128, 65), (300, 129))
# root plants only: nine tree children exceed the tree launch's fan-in of 8, so the root (43 rows) is
# factorised after it by one in-LDS launch of roots — the plan that puts the root tail on a side stream
ROOT_TAIL_TREE = (43, 0, [(33, 40, [])] * 9)


def plant_tree(name):
    """(root, seed) of a failed-pivot tree: 'leaf_R_W', 'root_tail' or an ASSEMBLY_TREES name."""
    if name.startswith("leaf_"):
        r, w = (int(t) for t in name.split("_")[1:])
        return leaf_shape_tree(r, w), 1000 * r + w
    if name == "root_tail":
        return ROOT_TAIL_TREE, 77
    return assembly_tree(name), sorted(ASSEMBLY_TREES).index(name)


def plant_tree_names():
    return [f"leaf_{r}_{w}" for r, w in PLANT_LEAF_SHAPES] + list(PLANT_ASSEMBLY)


def root_plant_tree_names():
    return plant_tree_names() + ["root_tail"]


def plant_sfms(name):
    """small_front_max values of a tree's configurations: 128, plus 192 for leaf_192_64."""
    return (128, 192) if name == "leaf_192_64" else (128,)


def plant_pivot(Lw, vals, perm, k, kind, d_ref=None, value=None):
    """New lower-CSC values (same pattern as Lw, sorted indices) in which only the diagonal entry of
    column j = perm[k] differs from vals:
      'tiny'   K[j,j] -= d_ref[k]         pivot k becomes rounding noise (fails pivot_tol = PLANT_TOL)
      'flip'   K[j,j] -= 1.5 d_ref[k]     pivot k becomes about -d_ref[k] / 2 (no failure, other inertia)
      'exact'  K[j,j]  = value            (k the first column of a childless front: d_k = K[j,j] exactly)
    d_ref: the oracle's pivots of the good matrix in the order perm."""
    j = int(perm[k])
    p = int(Lw.indptr[j])
    assert Lw.indices[p] == j, "the diagonal entry leads its lower-CSC column"
    out = np.array(vals, dtype=np.float64, copy=True)
    if kind == "tiny":
        out[p] -= d_ref[k]
    elif kind == "flip":
        out[p] -= 1.5 * d_ref[k]
    elif kind == "exact":
        out[p] = value
    else:
        raise ValueError(kind)
    return out


def symmetric_from_lower(Lw, vals):
    """The symmetric CSC matrix of lower-CSC values on Lw's pattern (as perturbed_values builds it: the
    diagonal is taken once, so a planted NaN or inf stays what it is)."""
    L2 = sp.csc_matrix((np.asarray(vals, np.float64), Lw.indices, Lw.indptr), shape=Lw.shape)
    K2 = (L2 + sp.tril(L2, -1).T).tocsc()
    K2.sort_indices()
    return K2


def first_bad_pivot(d, nvalid, tol):
    """The solver's failure rule on a pivot vector of which d[:nvalid + 1] is computed (the oracle stops
    at an exact zero pivot, which it stores): the smallest k with !(|d_k| > tol) or |d_k| = inf; -1 if none."""
    d = np.asarray(d)[:min(len(d), nvalid + 1)]
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(d) > tol) | np.isinf(d)
    return int(np.argmax(bad)) if bad.any() else -1


def oracle_plant(Lw, vals, perm, tol):
    """(first bad pivot index or -1, the oracle's pivots, how many of them are computed) for lower-CSC
    values in the pivot order perm."""
    from oracle.ldl import OracleLDL
    o = OracleLDL(symmetric_from_lower(Lw, vals), perm)
    n = int(o.factorize())
    d = o.diag()
    nv = min(n + 1, Lw.shape[0])
    return first_bad_pivot(d, n, tol), d, nv


def front_plant_columns(w):
    return sorted({c for c in PLANT_COLUMNS + (w - 1,) if 0 <= c < w})


def tree_plant_pivots(nodes, perm, first, parent, nrows):
    """[(pivot index k, node index, local column)] of the plants of a tree: front_plant_columns of every
    front, in the analysis' pivot order (through fronts_in_pivot_order)."""
    node_of, _ = fronts_in_pivot_order(nodes, perm, first, parent, nrows)
    out = []
    for s, i in enumerate(node_of):
        out += [(int(first[s]) + c, i, c) for c in front_plant_columns(nodes[i]["w"])]
    return out


def plant_required_classes(nodes, sfm, tree_fact, big_dag):
    """The front classes (names of the issue's list) that a configuration's plants reach, from the
    planner model front_tree_classes, which every GPU configuration asserts against info()."""
    want, ftree = front_tree_classes(nodes, sfm, tree_fact)
    seen = {"root"}
    for s, nd in enumerate(nodes):
        leaf, w, r = not nd["children"], nd["w"], nd["r"]
        if leaf and w <= 2 and r <= 32:
            p = nd["parent"]       # folded: the parent is a fold front of front_tree_classes
            pre = [nodes[q] for q in nodes[p]["children"] if not ftree[q]]
            folded = ftree[p] and nodes[p]["r"] <= 192 and all(c["w"] <= 2 and c["r"] <= 32 for c in pre)
            assert not folded or want["fold_leaves"] > 0
            seen.add("micro_folded" if folded else "micro_unfolded")
        elif leaf and r <= 32:
            seen.add("tiny")
        elif ftree[s] and r > 192:
            seen.add("tree_medium")
        elif ftree[s]:
            seen.add("lds_tree")
        elif r <= sfm:
            seen.add("lds_level")
        else:
            seen.add("big_dag" if big_dag else "big_step")
    return seen


PLANT_CLASSES = ("micro_unfolded", "micro_folded", "tiny", "lds_level", "lds_tree", "tree_medium", "big_dag",
                 "big_step", "root")


def plant_configs(name, nodes, tree_fact):
    """[(small_front_max, MADIPM_BIG_DAG, MADIPM_BIG_KPAN)] of a tree under one MADIPM_TREE_FACT: the
    DAG / per-step and panel-depth sweep only where a front can be big (r >= 129)."""
    big = max(nd["r"] for nd in nodes) >= 129
    dk = [("1", "1"), ("1", "4"), ("0", "1"), ("0", "4")] if big else [(None, None)]
    return [(sfm, dag, kpan) for sfm in plant_sfms(name) for dag, kpan in dk]


def _pivot_of(nodes, perm, first, parent, nrows):
    node_of, _ = fronts_in_pivot_order(nodes, perm, first, parent, nrows)
    sup_of = {i: s for s, i in enumerate(node_of)}
    return lambda i, c: int(first[sup_of[i]]) + c


def pair_plant_pivots(name, nodes, perm, first, parent, nrows):
    """[(k1, k2, nodes (i1, i2))], k1 < k2 in different subtrees, for the two-plants-at-once cases.
    big_mixed: a micro leaf with a column of the 257-column mid (the analysis orders that mid's subtree
    last, so the micro leaf holds the smaller index) and with a column of the 200-column mid (r = 257,
    ordered before the micro leaves: the big front holds the smaller index).  leaf_128_65: the first
    leaf with the third, and the third with the second (eliminated in the order first, third, second)."""
    k = _pivot_of(nodes, perm, first, parent, nrows)
    if name == "big_mixed":
        micro = [i for i, nd in enumerate(nodes) if nd["w"] == 1 and nd["r"] == 2]
        m257 = next(i for i, nd in enumerate(nodes) if nd["w"] == 257)
        m200 = next(i for i, nd in enumerate(nodes) if nd["w"] == 200)
        raw = [(micro[0], 0, m257, c) for c in (0, 64, 256)] + [(micro[-1], 0, m200, c) for c in (0, 65, 199)]
    elif name == "leaf_128_65":
        raw = [(0, 0, 2, 0), (0, 64, 2, 31), (0, 17, 2, 16), (2, 0, 1, 0), (2, 31, 1, 64), (2, 16, 1, 65)]
    else:
        raise ValueError(name)
    out = []
    for ia, ca, ib, cb in raw:
        (k1, i1), (k2, i2) = sorted([(k(ia, ca), ia), (k(ib, cb), ib)])
        out.append((k1, k2, (i1, i2)))
    return out


FLIP_TREES = ("big_mixed", "medium_mids")   # also the Cholesky-semantics trees (quasi-definite)


def flip_plant_pivots(name, nodes, perm, first, parent, nrows):
    """[(k, node)] of the flip plants: a column of a small leaf and a column of a big mid."""
    k = _pivot_of(nodes, perm, first, parent, nrows)
    leaf_w, leaf_c, mid_w, mid_c = {"big_mixed": (64, 17, 257, 65), "medium_mids": (33, 16, 200, 64)}[name]
    leaf = next(i for i, nd in enumerate(nodes) if nd["w"] == leaf_w and not nd["children"])
    mid = next(i for i, nd in enumerate(nodes) if nd["w"] == mid_w and nd["children"])
    return [(k(leaf, leaf_c), leaf), (k(mid, mid_c), mid)]


def exact_plant_pivots(nodes, perm, first, parent, nrows):
    """[(k, node)]: the first column of every childless front (d_k = K[j,j] exactly there)."""
    k = _pivot_of(nodes, perm, first, parent, nrows)
    return [(k(i, 0), i) for i, nd in enumerate(nodes) if not nd["children"]]


def batched_leaf_problem():
    """dense_k2(128, 200, 3), natural order (N = 328): one batched-leaf group whose 200 members are the
    single-column leaves x_j.  Returns (K, Lw, member pivots planted: first, a middle one, last)."""
    K, Lw = dense_k2(128, 200, 3)
    return K, Lw, (0, 101, 199)


def signed_diagonal(n=20001, seed=7):
    """A diagonal matrix with random signs and magnitudes in [0.5, 2]: more columns than one grid pass
    of the inertia kernel (64 blocks) covers.  Returns (lower CSC, the diagonal)."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    Lw = sp.diags(d).tocsc()
    Lw.sort_indices()
    return Lw, d


# ---------------------------------------------------------------- MPC reduction regimes
# (test_step_gpu.py, test_mpc_regimes_gpu.py; pinned on the sources and the oracle in
# test_regime_helpers_cpu.py)
# The launch constants of csrc/mpc_kernels.hpp (NT, MAXB), csrc/mpc.hip (FT1, FG, FT) and csrc/mpc.hpp (maxb_)
# that decide which path a reduction takes: the regime tests derive every boundary from these and
# test_regime_helpers_cpu.py fails when a source changes.
MPC_CONSTANTS = {"NT": 256, "FT1": 1024, "MAXB": 2048, "FG": 16, "FT": 128, "maxb_": 2048}
MPC_NT, MPC_FT1, MPC_MAXB = MPC_CONSTANTS["NT"], MPC_CONSTANTS["FT1"], MPC_CONSTANTS["maxb_"]


def mpc_blocks(n):
    """MPCSolver::blocks: the producer blocks of a flat kernel over n elements."""
    return max(1, min(MPC_MAXB, -(-int(n) // MPC_NT)))


def mpc_spmv_blocks(rows, G):
    """MPCSolver::spmv_blocks: the producer blocks of an SpMV-shaped kernel, one row per G lanes."""
    return mpc_blocks(int(rows) * G)


def mpc_regime(n, G=1):
    """(producer blocks, finaliser 'one' | 'two', strided) of a kernel over n elements, G lanes each:
    k_final's one-workgroup instance up to FT1 partial blocks, the two-level one past it; the producer's
    loop strides once n G exceeds MAXB NT threads."""
    nb = mpc_blocks(int(n) * G)
    return nb, ("one" if nb <= MPC_FT1 else "two"), int(n) * G > MPC_MAXB * MPC_NT


def regime_hot(m, n_ineq, where, boundary=None):
    """The planted positions of regime_problem for a placement:
      'first'     row 0 (a range row whenever n_ineq > 0: no coordinate can be planted beside it);
      'last'      row m - 1, the last of n_ + m_, and its second column, the last lower-bounded column;
      'boundary'  flat element `boundary` of [0, n_ + m_) — the first element of the block or of the
                  stride trip under test, clamped to the last element — as a constraint row (an element
                  below n_ wraps into the rows) and, as a position of ind_lb, as a coordinate."""
    n_ = 2 * m + n_ineq
    if where == "first":
        return dict(row=0, coord=None if n_ineq > 0 else 0)
    if where == "last":
        return dict(row=m - 1, coord=-1)
    assert where == "boundary" and boundary is not None
    e = min(int(boundary), n_ + m - 1)
    return dict(row=e - n_ if e >= n_ else e % m, coord=e)


def regime_problem(m, n_ineq, seed, hess=False, hot=None):
    """A separable LP / QP of any size for the reduction-regime tests: nx = 2 m columns, row i couples
    columns 2 i and 2 i + 1 only (two entries of magnitude in [0.5, 2], random sign); the first n_ineq rows
    are ranges (ucon = lcon + 1), the others equalities; no fixed and no free variable, so the solver has
    n_ + m_ = 3 m + n_ineq rows.  Bounds: lower-only (50 %), both (40 %), upper-only (10 %, with c < 0
    there), so nlb != nub and ind_lb, ind_ub are no identity.  lcon = A xint (ranges: a band around it)
    for a strictly interior xint, and c = A^T y0 + zl0 - zu0 (- H xint) with zl0, zu0 >= 0 on their
    bounds: feasible and bounded.  The start x0 = xint + 0.02 U(-1, 1).  hess=True: H = a positive
    diagonal plus the off-diagonal of each pair (2 i, 2 i + 1), diagonally dominant: still separable.

    hot = dict(row=r, coord=t or None) (regime_hot) plants the extreme element of the max-type reductions
    through the start alone.  The reference's first Newton step uses the constraint residual c of x0
    (initialize! evaluates the model before init_starting_point! moves x), so a column started away from
    xint is moved by about that distance twice: by the starting point's projection and by the step.
      coord  the lower-bounded column j of an equality row nearest to position t of ind_lb (t < 0: from the
             end of the columns): lower-only, 0.5 above its bound, entry +-2 beside a partner entry -+0.5
             whose sign moves the partner away from its bound, started 4 above xint_j (|c| = 8): the only
             primal ratio below 1 at iteration 1.  Measured on the oracle, a larger offset is undone by the
             Mehrotra corrector, and in a range row the projection pushes the slack out of its band (one
             wide), whose repair (delta_x) lifts every coordinate off its bound: no column of a range row
             and no slack can be planted this way, so positions there move to the next equality row.
      row    |c_r| of x0 is the largest by a factor >= 4.  An equality row: the coordinate's row when t
             lies in it; else both columns are lower-only, 50 above their bound, entries +-2 of one sign,
             started 40 below xint (|c_r| = 160; they move away from their bounds).  A range row (no
             coordinate then): one column started 4 above xint with entry +-2, |c_r| >= 6.8.
    qp.hot = dict(row, coord: position in ind_lb or None, col: that column).
    (The dual residual after init_starting_point! is -(1 + delta_s + delta_s2) on every lower-only
    column, the same with + on every upper-only one and 0 on the boxed columns and slacks, and an LP's
    stays a multiple of that: it has no unique maximum to plant; test_regime_helpers_cpu.py pins this.)"""
    from madipm_amd.qp import QuadraticModel
    rng = np.random.default_rng(seed)
    nx = 2 * m
    a = rng.uniform(0.5, 2.0, (m, 2)) * rng.choice([-1.0, 1.0], (m, 2))
    u = rng.random(nx)
    up_only, both = u < 0.1, (u >= 0.1) & (u < 0.5)
    lvar = rng.uniform(-1.0, 1.0, nx)
    uvar = np.where(both, lvar + rng.uniform(1.0, 5.0, nx), np.inf)
    uvar[up_only] = lvar[up_only]
    lvar[up_only] = -np.inf
    pos = rng.uniform(0.2, 0.8, nx)
    gap = rng.uniform(0.5, 2.0, nx)
    noise = 0.02 * rng.uniform(-1.0, 1.0, nx)
    start = {}                                          # column -> x0 - xint of the plants
    if hot is not None:
        r, t = int(hot["row"]), hot["coord"]
        assert 0 <= r < m
        for j in (2 * r, 2 * r + 1):
            lvar[j], uvar[j], up_only[j], both[j] = 0.0, np.inf, False, False
        q = j = None
        if t is not None:
            assert r >= n_ineq, "no coordinate can be planted beside a planted range row"
            lb_cols = np.flatnonzero(np.isfinite(lvar))     # ind_lb: these columns, then the slacks
            t = min(int(t), len(lb_cols) - 1) if t >= 0 else max(0, len(lb_cols) + int(t))
            ok = np.flatnonzero(lb_cols // 2 >= n_ineq)     # positions in equality rows
            t = int(ok[min(np.searchsorted(ok, t), len(ok) - 1)])
            j = int(lb_cols[t])
            p, q = j ^ 1, j // 2
            uvar[j], both[j], gap[j] = np.inf, False, 0.5   # lower-only; lb_cols keeps its members
            if np.isfinite(lvar[p]):
                uvar[p], both[p] = np.inf, False
            sj = np.sign(a[q, j & 1])
            a[q, j & 1] = 2.0 * sj
            a[q, p & 1] = (0.5 if up_only[p] else -0.5) * sj   # the partner moves away from its one bound
            start[j] = 4.0
        if r < n_ineq:
            a[r, 0] = 2.0 * np.sign(a[r, 0])
            start[2 * r] = 4.0
        elif q != r:
            a[r] = 2.0 * np.sign(a[r, 0])
            gap[2 * r] = gap[2 * r + 1] = 50.0
            start[2 * r] = start[2 * r + 1] = -40.0
        hot = dict(row=r, coord=t, col=j)
    with np.errstate(invalid="ignore"):
        xint = np.where(both, lvar + pos * (uvar - lvar), np.where(up_only, uvar - gap, lvar + gap))
    b = a[:, 0] * xint[0::2] + a[:, 1] * xint[1::2]
    lcon, ucon = b.copy(), b.copy()
    lcon[:n_ineq] = b[:n_ineq] - rng.uniform(0.2, 0.8, n_ineq)
    ucon[:n_ineq] = lcon[:n_ineq] + 1.0
    y0 = rng.uniform(-1.0, 1.0, m)
    aty = (a * y0[:, None]).ravel()
    zl0 = np.where(np.isfinite(lvar), rng.uniform(0.0, 1.0, nx), 0.0)
    zu0 = np.where(both, rng.uniform(0.0, 1.0, nx), 0.0)
    zu0[up_only] = np.abs(aty[up_only]) + rng.uniform(0.5, 1.5, int(up_only.sum()))
    c = aty + zl0 - zu0
    assert np.all(c[up_only] < 0.0)
    Hr = Hc = Hv = []
    if hess:
        hd = rng.uniform(0.5, 2.0, nx)
        ho = rng.uniform(-0.4, 0.4, m)
        Hr = np.r_[np.arange(nx), np.arange(1, nx, 2)]
        Hc = np.r_[np.arange(nx), np.arange(0, nx, 2)]
        Hv = np.r_[hd, ho]
        hx = hd * xint
        hx[0::2] += ho * xint[1::2]
        hx[1::2] += ho * xint[0::2]
        c = c - hx
        c[up_only] = np.minimum(c[up_only], -0.5)
    x0 = xint + noise
    for j, d in start.items():
        x0[j] = xint[j] + d
    qp = QuadraticModel(c=c, Hrows=Hr, Hcols=Hc, Hvals=Hv, Arows=np.repeat(np.arange(m), 2), Acols=np.arange(nx),
                        Avals=a.ravel(), lcon=lcon, ucon=ucon, lvar=lvar, uvar=uvar, x0=x0,
                        name=f"regime_{m}_{n_ineq}_s{seed}_{'qp' if hess else 'lp'}")
    qp.hot = hot
    return qp


def regime_bounds(qp):
    """(rows, nlb, nub) of the solver on a regime problem: n_ + m_ and the bounded coordinates, slacks
    included (a range row's slack has both bounds)."""
    ns = int(np.sum(qp.lcon != qp.ucon))
    return (qp.nvar + ns + qp.ncon, int(np.sum(np.isfinite(qp.lvar))) + ns, int(np.sum(np.isfinite(qp.uvar))) + ns)


def regime_name(m, n_ineq, hess, where, boundary=0):
    """The cache key of a regime problem (seed = m + n_ineq): test_mpc_point_gpu._problem builds it."""
    return f"regime:{m}:{n_ineq}:{int(hess)}:{where}:{boundary}"


def regime_case(name):
    tag, m, n_ineq, hess, where, boundary = name.split(":")
    assert tag == "regime"
    m, n_ineq = int(m), int(n_ineq)
    return regime_problem(m, n_ineq, m + n_ineq, bool(int(hess)), regime_hot(m, n_ineq, where, int(boundary)))


# SpMV-shaped kernels at G = 64 (NT / 64 = 4 rows per block): (m, n_ineq) -> rows = 3 m + n_ineq, with the
# finaliser path and whether the row loop strides; `boundary` is the first row element of block FT1
# (4 FT1) before the cap and of the second stride trip (4 MAXB) past it
REGIME_G = 64
REGIME_G64_SIZES = {(1300, 196): (4096, "one", False), (1300, 197): (4097, "two", False),
                    (2600, 392): (8192, "two", False), (2600, 393): (8193, "two", True),
                    (6000, 2001): (20001, "two", True)}
REGIME_PLACES = ("first", "last", "boundary")
REGIME_KS = (0, 1, 3)


def regime_g64_boundary(rows):
    per = MPC_NT // REGIME_G
    return per * MPC_MAXB if rows > per * MPC_MAXB else per * MPC_FT1


def regime_g64_cases():
    """[(problem name, kkt, variant)] of the G = 64 sweep: per size the LP under K2, K2.5 and the normal
    equations and the QP under K2 and K2.5 (default variant), MehrotraAdaptiveStep and max_ncorr = 3 on the
    4097- and 8193-row LPs under K2; the placement of the plants cycles over the cases."""
    out = []
    for si, ((m, ni), (rows, _, _)) in enumerate(REGIME_G64_SIZES.items()):
        combos = [(False, "K2", "default"), (False, "K25", "default"), (False, "normal", "default"),
                  (True, "K2", "default"), (True, "K25", "default")]
        if rows in (4097, 8193):
            combos += [(False, "K2", "mehrotra"), (False, "K2", "ncorr3")]
        for ci, (hess, kkt, variant) in enumerate(combos):
            where = REGIME_PLACES[(si + ci) % 3]
            out.append((regime_name(m, ni, hess, where, regime_g64_boundary(rows)), kkt, variant))
    return out


# flat kernels at the heuristic's own G: (m, n_ineq) -> (rows, finaliser, strided, placement, boundary, ks)
REGIME_FLAT_SIZES = {(80000, 22144): (262144, "one", False, "last", 0, (2,)),
                     (80000, 22145): (262145, "two", False, "last", 0, (2,)),
                     (160000, 44588): (524588, "two", True, "boundary", MPC_MAXB * MPC_NT, (0, 2))}


def regime_flat_cases():
    return [(regime_name(m, ni, False, where, b), ks) for (m, ni), (_, _, _, where, b, ks) in REGIME_FLAT_SIZES.items()]


def regime_launches(qp, G):
    """The producer block counts of one MPC iteration on a regime problem, as (blocks, finaliser,
    strided) per kernel family: 'flat' (k_rhs, k_term, k_apply, ... over n_ + m_), 'spmv' (k_residual,
    k_eval, the normal-equation kernels: one row per G lanes) and 'step' (k_alpha, k_mu, the step-test
    blocks of k_residual over max(nlb, nub))."""
    rows, nlb, nub = regime_bounds(qp)
    return dict(flat=mpc_regime(rows), spmv=mpc_regime(rows, G), step=mpc_regime(max(nlb, nub)))


# the step test alone (madipm_update_step): max(nlb, nub) -> (blocks, finaliser, strided)
REGIME_STEP_SIZES = {262144: (1024, "one", False), 262145: (1025, "two", False), 524288: (2048, "two", False),
                     524289: (2048, "two", True), 1310797: (2048, "two", True)}


def regime_step_ties(n):
    """The tied index pairs of the step test at max(nlb, nub) = n, each of which must yield its last
    index: across workgroups 0 and 1 of the two-level finaliser (FT blocks each), across blocks FT1 - 1
    and FT1, the first and the last element, and past the cap one thread's two trips and the pair around
    the first trip's end (the later index sits in block 0, which the finaliser combines first)."""
    wg = MPC_CONSTANTS["FT"] * MPC_NT
    ties = [(wg - 1, wg), (0, n - 1), (MPC_NT - 1, MPC_NT)]      # the last: blocks 0 | 1
    if n > MPC_FT1 * MPC_NT:
        ties.append((MPC_FT1 * MPC_NT - 1, MPC_FT1 * MPC_NT))
    trip = MPC_MAXB * MPC_NT
    if n > trip:
        t = min(5, n - trip - 1)
        ties += [(t, t + trip), (trip - 1, trip)]
    return list(dict.fromkeys(ties))      # at n = MAXB NT + 1 the two-trip pair is (0, n - 1)
