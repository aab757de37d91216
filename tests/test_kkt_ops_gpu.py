"""Array-type overrides (csrc/kkt.hip, the ROCArray counterparts of ext/MadIPMCUDAExt) through the
C-ABI against the oracle's restatement of the reference's CPU methods (oracle/kkt_ops.py).

Tolerances: transfer!, compress_jacobian!, coo_to_csr, fill_structure and assemble_normal_system!
follow the reference CPU loops' order and rounding: BIT-EXACT.  The SpMV operator and the QP
evaluators sum rows in a fixed order of their own (cuSPARSE's order is unspecified in the
reference): 1e-14 relative to the row's absolute sum.
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")


def _t(a, dtype=None):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.copy())
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _random_csr(m, n, dens, seed):
    rng = np.random.default_rng(seed)
    A = sp.random(m, n, density=dens, format="csr", random_state=rng, data_rvs=rng.standard_normal)
    A.sort_indices()
    return A


@pytest.mark.parametrize("nsrc,ndest,seed", [(0, 5, 0), (1, 1, 1), (1000, 300, 2), (200_000, 50_000, 3)])
def test_transfer_bitexact(nsrc, ndest, seed):
    from madipm_amd.rocm_wrapper import Transfer
    from oracle import kkt_ops as O
    rng = np.random.default_rng(seed)
    mp = rng.integers(0, ndest, nsrc).astype(np.int64)        # duplicates: scatter-ADD
    src = rng.standard_normal(nsrc) * 10.0 ** rng.integers(-8, 8, nsrc)
    ref = O.transfer(ndest, src, mp.tolist()) if nsrc <= 1000 else None
    if ref is None:  # large case: the same ascending-k sums, vectorised per destination
        order = np.argsort(mp, kind="stable")
        ref = np.zeros(ndest)
        for k in order:
            ref[mp[k]] += src[k]
    dest = torch.full((ndest,), 7.0, dtype=torch.float64, device=DEV)   # stale values are overwritten
    for dev_map in (False, True):
        T = Transfer(_t(mp) if dev_map else mp, ndest)
        T(dest, _t(src))
        assert np.array_equal(_np(dest), ref)


def test_compress_jacobian_bitexact():
    from madipm_amd.rocm_wrapper import compress_jacobian
    from oracle import kkt_ops as O
    rng = np.random.default_rng(0)
    nnz, ns = 5000, 300
    AV = rng.standard_normal(nnz)
    cmap = rng.permutation(nnz).astype(np.int64)
    refAV, refAT = O.compress_jacobian(AV, ns, cmap)
    dAV, dAT = _t(AV), torch.zeros(nnz, dtype=torch.float64, device=DEV)
    compress_jacobian(dAV, ns, _t(cmap), dAT)
    assert np.array_equal(_np(dAV), refAV) and np.array_equal(_np(dAT), refAT)


@pytest.mark.parametrize("m,n,nnz,seed", [(1, 1, 0, 0), (5, 7, 12, 1), (300, 200, 4000, 2), (20000, 30000, 400_000, 3)])
def test_coo_to_csr_bitexact(m, n, nnz, seed):
    from madipm_amd.rocm_wrapper import coo_to_csr
    from oracle import kkt_ops as O
    rng = np.random.default_rng(seed)
    Ai = rng.integers(0, m, nnz).astype(np.int32)
    Aj = rng.integers(0, n, nnz).astype(np.int32)
    Ax = rng.standard_normal(nnz)
    if nnz <= 4000:
        Rp, Rj, Rx = O.coo_to_csr(m, n, Ai.tolist(), Aj.tolist(), Ax)
    else:  # stable counting sort by row == a stable argsort by row
        o = np.argsort(Ai, kind="stable")
        Rp = np.r_[0, np.cumsum(np.bincount(Ai, minlength=m))].astype(np.int32)
        Rj, Rx = Aj[o], Ax[o]
    Bp, Bj, Bx = coo_to_csr(m, n, _t(Ai), _t(Aj), _t(Ax))
    assert np.array_equal(_np(Bp), Rp) and np.array_equal(_np(Bj), Rj) and np.array_equal(_np(Bx), Rx)
    # sort_cols: the rows' entries by ascending column, ties in input order (cuSPARSE layout)
    o = np.lexsort((np.arange(nnz), Aj, Ai))
    Bp, Bj, Bx = coo_to_csr(m, n, _t(Ai), _t(Aj), _t(Ax), sort_cols=True)
    assert np.array_equal(_np(Bp), Rp) and np.array_equal(_np(Bj), Aj[o]) and np.array_equal(_np(Bx), Ax[o])


def test_coo_to_csr_rejects_out_of_range():
    """An index outside [0, n_rows) x [0, n_cols) is reported, not turned into a corrupt CSR."""
    from madipm_amd.rocm_wrapper import coo_to_csr
    Ax = np.ones(3)
    for Ai, Aj in (([0, 5, 1], [0, 1, 2]), ([0, 1, 1], [0, -1, 2]), ([0, 1, 1], [0, 1, 3])):
        with pytest.raises(Exception, match="out of range"):
            coo_to_csr(4, 3, _t(np.array(Ai, np.int32)), _t(np.array(Aj, np.int32)), _t(Ax))


def test_fill_structure_exact():
    from madipm_amd.rocm_wrapper import fill_structure
    from oracle import kkt_ops as O
    A = _random_csr(500, 300, 0.02, 1)
    rows = torch.zeros(A.nnz, dtype=torch.int32, device=DEV)
    cols = torch.zeros(A.nnz, dtype=torch.int32, device=DEV)
    fill_structure(500, _t(A.indptr.astype(np.int32)), _t(A.indices.astype(np.int32)), rows, cols)
    rr, rc = O.fill_structure(500, A.indptr, A.indices)
    assert np.array_equal(_np(rows), rr) and np.array_equal(_np(cols), rc)


@pytest.mark.parametrize("m,n,dens,seed", [(40, 60, 0.1, 0), (400, 900, 0.01, 1), (3000, 8000, 0.002, 2)])
def test_assemble_normal_system_bitexact(m, n, dens, seed):
    from madipm_amd.rocm_wrapper import build_normal_system, assemble_normal_system
    from oracle import kkt_ops as O
    A = _random_csr(m, n, dens, seed)
    Cp, Cj = build_normal_system(m, n, A.indptr, A.indices)
    D = np.random.default_rng(seed).uniform(0.1, 10.0, n)
    Cx = torch.full((len(Cj),), np.nan, dtype=torch.float64, device=DEV)
    assemble_normal_system(m, n, _t(A.indptr.astype(np.int32)), _t(A.indices.astype(np.int32)), _t(A.data),
                           _t(Cp), _t(Cj), Cx, _t(D))
    got = _np(Cx)
    if m <= 400:
        ref = O.assemble_normal_system(m, n, A.indptr.tolist(), A.indices.tolist(), A.data.tolist(),
                                       Cp.tolist(), Cj.tolist(), D)
        assert np.array_equal(got, ref)
    # and it is A D A' on the lower pattern
    C = sp.tril(A @ sp.diags(D) @ A.T).tocsc()
    ref2 = np.asarray(C[Cj, np.repeat(np.arange(m), np.diff(Cp))]).ravel()
    assert np.allclose(got, ref2, rtol=1e-13, atol=1e-13 * np.abs(ref2).max())


def _spmv_group(mean_row):
    """spmv_group of csrc/kkt.hip: the lanes per row chosen from the operator's mean row length."""
    for g, top in ((2, 3), (4, 6), (8, 12), (16, 24), (32, 48)):
        if mean_row <= top:
            return g
    return 64


def _check_operator(m, n, A, transa, symmetric, group=None, lengths=(), live=True, exact_ref=True):
    """mul! of the operator on the CSR arrays of A (as stored: unsorted / duplicate entries stay) against
    oracle.kkt_ops.operator_matrix, to 1e-14 x the row's absolute sum.  group: the lane-group width the
    operator's mean row length must select; lengths: row lengths the operator matrix must contain.
    exact_ref: the reference product is summed in longdouble (dense: small cases only)."""
    from madipm_amd.rocm_wrapper import MadIPMOperator
    from oracle import kkt_ops as O
    rng = np.random.default_rng(3)
    dp, dj, dx = _t(A.indptr.astype(np.int32)), _t(A.indices.astype(np.int32)), _t(A.data)
    op = MadIPMOperator(m, n, dp, dj, dx, transa=transa, symmetric=symmetric)
    assert op.shape == (m, n) and op.nnz() == A.nnz
    M = O.operator_matrix(m, n, A.indptr, A.indices, A.data, transa, symmetric)
    M.sum_duplicates()
    rowlen = np.diff(M.indptr)
    if group is not None:
        assert _spmv_group(M.nnz / M.shape[0]) == group, (M.nnz / M.shape[0], group)
    assert set(lengths) <= set(rowlen.tolist()), sorted(set(lengths) - set(rowlen.tolist()))
    x = rng.standard_normal(M.shape[1])
    y0 = rng.standard_normal(M.shape[0])
    if exact_ref:
        Mx = M.toarray().astype(np.longdouble) @ x.astype(np.longdouble)
    else:
        Mx = M @ x
    absMx = abs(M) @ abs(x)
    scale = absMx + abs(y0) + 1e-300
    for alpha, beta in ((1.0, 0.0), (1.0, -1.0), (-0.5, 2.0)):
        y = _t(y0)
        op.mul(y, _t(x), alpha, beta)
        ref = alpha * Mx + beta * y0
        err = np.abs(_np(y) - ref)
        assert np.all(err <= 1e-14 * scale * max(1.0, abs(alpha), abs(beta))), \
            (alpha, beta, int(np.argmax(err / scale)), int(rowlen[np.argmax(err / scale)]), float(np.max(err / scale)))
    # beta = 0 overwrites: stale NaN in y must not reach the result (rows of 0 entries included)
    y = torch.full((M.shape[0],), float("nan"), dtype=torch.float64, device=DEV)
    op.mul(y, _t(x), 2.0, 0.0)
    got = _np(y)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - 2.0 * Mx) <= 2e-14 * (absMx + 1e-300))
    if live and not symmetric:  # 'N' and 'T' read the caller's values live (cuSPARSE descriptors do too)
        dx.mul_(2.0)
        y = torch.zeros(M.shape[0], dtype=torch.float64, device=DEV)
        op.mul(y, _t(x))
        assert np.all(np.abs(_np(y) - 2.0 * Mx) <= 2e-14 * scale)
    return M


@pytest.mark.parametrize("transa,symmetric", [("N", False), ("T", False), ("N", True)])
def test_operator_mul(transa, symmetric):
    m, n = (700, 700) if symmetric else (700, 1100)
    A = _random_csr(m, n, 0.01, 4)
    if symmetric:
        A = sp.tril(A).tocsr()
        A.sort_indices()
    _check_operator(m, n, A, transa, symmetric, group=8)


def _special_lengths(G):
    return (0, 1, G - 1, G, G + 1, 2 * G + 1, 4 * G + 3)


def _rowlen_csr(nrows, ncols, G, mean, seed):
    """nrows x ncols CSR with nrows * mean entries: two rows each of 0, 1, G - 1, G, G + 1, 2 G + 1 and
    4 G + 3 entries (the first and the last row among them), the others of floor / ceil of what is left;
    columns drawn without replacement, values N(0, 1)."""
    rng = np.random.default_rng(seed)
    special = list(_special_lengths(G)) * 2
    where = np.r_[0, nrows - 1, rng.choice(np.arange(1, nrows - 1), len(special) - 2, replace=False)]
    lens = np.full(nrows, -1)
    lens[where] = special
    rest = np.flatnonzero(lens < 0)
    left = int(round(mean * nrows)) - sum(special)
    lens[rest] = left // len(rest) + (np.arange(len(rest)) < left % len(rest))
    assert lens.min() >= 0 and lens.max() <= ncols and lens.sum() == int(round(mean * nrows))
    cols = np.concatenate([np.sort(rng.choice(ncols, ln, replace=False)) for ln in lens])
    A = sp.csr_matrix((rng.standard_normal(len(cols)), cols, np.r_[0, np.cumsum(lens)]), shape=(nrows, ncols))
    return A


def _rowlen_lower(n, G, mean, seed):
    """Lower-triangular n x n CSR whose symmetric operator tril(A, -1) + A' has ~n * mean entries and
    rows of the special lengths: the last 14 rows hold exactly those many entries, in columns of the
    first n - 14 rows, and no diagonal; the first n - 14 rows hold their diagonal and random strictly
    lower entries."""
    rng = np.random.default_rng(seed)
    special = list(_special_lengths(G)) * 2
    nq = n - len(special)
    target = (int(round(mean * n)) - nq) // 2 - sum(special)   # strictly lower entries among the first nq rows
    t = 0
    while np.minimum(np.arange(nq), t).sum() < target:
        t += 1
    cnt = np.minimum(np.arange(nq), t)
    over = int(cnt.sum() - target)
    cnt[nq - over:] -= 1
    assert cnt.min() >= 0 and cnt.sum() == target
    rows, cols = [], []
    for i in range(nq):
        c = np.sort(rng.choice(i, cnt[i], replace=False)) if cnt[i] else np.zeros(0, int)
        rows += [i] * (len(c) + 1)
        cols += list(c) + [i]
    for k, ln in enumerate(rng.permutation(special)):
        rows += [nq + k] * int(ln)
        cols += list(np.sort(rng.choice(nq, int(ln), replace=False)))
    A = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


@pytest.mark.parametrize("transa,symmetric", [("N", False), ("T", False), ("N", True)])
@pytest.mark.parametrize("G,mean", [(2, 2), (4, 5), (8, 10), (16, 20), (32, 40), (64, 60)])
def test_operator_mul_widths(G, mean, transa, symmetric):
    """Every lane-group width of k_spmv_rows32 ('N'), k_spmv_rows with the value map ('T') and
    k_spmv_rows on the owned copy (symmetric), selected by the operator's mean row length, on rows of
    0, 1, G - 1, G, G + 1, 2 G + 1 and 4 G + 3 entries; m = 701 and n = 1103 are odd (no multiple of
    256 / G rows: the last workgroup is partial, and the first and last rows are special ones)."""
    m, n = 701, 1103
    if symmetric:
        A = _rowlen_lower(m, G, mean, 10 + G)
        n = m
    elif transa == "N":
        A = _rowlen_csr(m, n, G, mean, 20 + G)
    else:  # the operator's rows are A's columns
        A = _rowlen_csr(n, m, G, mean, 30 + G).T.tocsr()
        A.sort_indices()
    _check_operator(m, n, A, transa, symmetric, group=G, lengths=_special_lengths(G))


def test_operator_mul_general_symmetric_input():
    """symmetric=True on an A that is no lower triangle: strictly upper entries (which enter through A'
    only) and duplicate entries (summed), in unsorted rows — against scipy's tril(A, -1) + A'."""
    rng = np.random.default_rng(8)
    n, nnz = 333, 4000
    ri = np.sort(rng.integers(0, n, nnz))
    cj = rng.integers(0, n, nnz)
    cj[1::7] = cj[0:-1:7][:len(cj[1::7])]           # duplicates of (row, column) where the rows agree
    A = sp.csr_matrix((rng.standard_normal(nnz), cj, np.r_[0, np.cumsum(np.bincount(ri, minlength=n))]), shape=(n, n))
    assert A.nnz == nnz and not A.has_canonical_format
    B = A.copy()
    B.sum_duplicates()
    assert B.nnz < nnz and sp.triu(B, 1).nnz > 100 and sp.tril(B, -1).nnz > 100
    M = _check_operator(n, n, A, "N", True)
    ref = (sp.tril(B, -1) + B.T).tocsr()
    assert abs(M - ref).max() <= 1e-15 * abs(ref).max()


@pytest.mark.parametrize("transa,symmetric", [("N", False), ("T", False), ("N", True)])
def test_operator_mul_empty(transa, symmetric):
    """An operator without entries: y = beta y (and zero for beta = 0, whatever y held)."""
    from madipm_amd.rocm_wrapper import MadIPMOperator
    m, n = (6, 6) if symmetric else (5, 7)
    op = MadIPMOperator(m, n, torch.zeros(m + 1, dtype=torch.int32, device=DEV),
                        torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV),
                        transa=transa, symmetric=symmetric)
    assert op.shape == (m, n) and op.nnz() == 0
    rows, cols = (n, m) if transa == "T" else (m, n)
    y0 = np.arange(1.0, rows + 1)
    x = _t(np.ones(cols))
    y = _t(y0)
    op.mul(y, x, 2.0, -1.5)
    assert np.array_equal(_np(y), -1.5 * y0)
    y = torch.full((rows,), float("nan"), dtype=torch.float64, device=DEV)
    op.mul(y, x, 2.0, 0.0)
    assert np.array_equal(_np(y), np.zeros(rows))


def test_operator_mul_grid_stride():
    """300,000 rows of exactly 49 entries: mean 49 selects G = 64, and rows x G = 19.2 M lanes exceed
    the launch's cap of 65,536 workgroups x 256 threads, so every lane group strides to a second row."""
    m, n, L = 300_000, 1009, 49
    assert m * 64 > 65536 * 256
    i = np.arange(m, dtype=np.int64)[:, None]
    k = np.arange(L, dtype=np.int64)[None, :]
    cols = ((7 * i + 13 * k) % n).astype(np.int32).ravel()     # 13 k < n: distinct within a row
    vals = (((31 * i + 17 * k) % 101) - 50.0).ravel() / 64.0
    A = sp.csr_matrix((vals, cols, np.arange(0, m * L + 1, L)), shape=(m, n))
    _check_operator(m, n, A, "N", False, group=64, lengths=(L,), live=False, exact_ref=False)


def _long_thin_csr(m, n):
    """m rows of 1 - 2 entries (ascending columns), arithmetically; values in [-1, 1]."""
    i = np.arange(m, dtype=np.int64)
    two = i % 3 != 0
    c0 = (5 * i) % n
    c1 = (5 * i + 1 + i % 7) % n
    lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)
    lens = 1 + two.astype(np.int64)
    rp = np.r_[0, np.cumsum(lens)]
    cols = np.empty(rp[-1], np.int32)
    cols[rp[:-1]] = np.where(two, lo, c0)
    cols[rp[:-1][two] + 1] = hi[two]
    assert np.all(lo[two] < hi[two])
    vals = ((np.arange(rp[-1]) * 37) % 201 - 100.0) / 100.0 + 0.005
    return sp.csr_matrix((vals, cols, rp), shape=(m, n))


def test_fill_structure_grid_stride():
    """300,000 rows (one wave each: 19.2 M lanes, above the 65,536 x 256 launch cap) of 1 - 2 entries."""
    from madipm_amd.rocm_wrapper import fill_structure
    m, n = 300_000, 299_993
    A = _long_thin_csr(m, n)
    rows = torch.full((A.nnz,), -1, dtype=torch.int32, device=DEV)
    cols = torch.full((A.nnz,), -1, dtype=torch.int32, device=DEV)
    fill_structure(m, _t(A.indptr.astype(np.int32)), _t(A.indices.astype(np.int32)), rows, cols)
    assert np.array_equal(_np(rows), np.repeat(np.arange(m, dtype=np.int32), np.diff(A.indptr)))
    assert np.array_equal(_np(cols), A.indices)


def test_assemble_normal_system_grid_stride():
    """assemble_normal_system! on 300,000 rows of 1 - 2 entries (one wave per row, above the launch
    cap): BIT-EXACT — an entry is 0 + (a_ik d_k) a_jk (+ a second product), no order to choose."""
    from madipm_amd.rocm_wrapper import build_normal_system, assemble_normal_system
    m, n = 300_000, 299_993
    A = _long_thin_csr(m, n)
    Cp, Cj = build_normal_system(m, n, A.indptr, A.indices)
    D = 0.5 + (np.arange(n) % 13) / 4.0
    Cx = torch.full((len(Cj),), np.nan, dtype=torch.float64, device=DEV)
    assemble_normal_system(m, n, _t(A.indptr.astype(np.int32)), _t(A.indices.astype(np.int32)), _t(A.data),
                           _t(Cp), _t(Cj), Cx, _t(D))
    got = _np(Cx)
    ci = np.repeat(np.arange(m), np.diff(Cp))                 # entry c = (row Cj[c], column ci[c])
    AD = A.copy()
    AD.data = A.data * D[A.indices]                           # a_ik d_k, rounded once
    ref = np.asarray(AD[ci].multiply(A[Cj]).sum(axis=1)).ravel()
    assert len(Cj) > m and np.array_equal(got, ref)


@pytest.mark.parametrize("n_slack", [0, 5000])
def test_compress_jacobian_slack_edges(n_slack):
    """n_slack = 0 (nothing overwritten) and n_slack = nnz (every entry becomes -1)."""
    from madipm_amd.rocm_wrapper import compress_jacobian
    from oracle import kkt_ops as O
    rng = np.random.default_rng(1)
    nnz = 5000
    AV = rng.standard_normal(nnz)
    cmap = rng.permutation(nnz).astype(np.int64)
    refAV, refAT = O.compress_jacobian(AV, n_slack, cmap)
    dAV, dAT = _t(AV), torch.full((nnz,), np.nan, dtype=torch.float64, device=DEV)
    compress_jacobian(dAV, n_slack, _t(cmap), dAT)
    assert np.array_equal(_np(dAV), refAV) and np.array_equal(_np(dAT), refAT)
    assert np.all(refAT == -1.0) if n_slack else np.array_equal(refAV, AV)


def test_qp_obj_grad():
    from madipm_amd.rocm_wrapper import MadIPMOperator, qp_obj, qp_grad
    from oracle import kkt_ops as O
    rng = np.random.default_rng(5)
    n = 5000
    H = sp.tril(_random_csr(n, n, 0.001, 6) + sp.eye(n)).tocsr()
    H.sort_indices()
    Hop = MadIPMOperator(n, n, _t(H.indptr.astype(np.int32)), _t(H.indices.astype(np.int32)), _t(H.data),
                         symmetric=True)
    Hm = O.operator_matrix(n, n, H.indptr, H.indices, H.data, "N", True)
    c, x = rng.standard_normal(n), rng.standard_normal(n)
    v = torch.zeros(n, dtype=torch.float64, device=DEV)
    obj = qp_obj(Hop, _t(c), 1.25, _t(x), v)
    ref = O.qp_obj(Hm, c, 1.25, x)
    assert abs(obj - ref) <= 1e-13 * (abs(c) @ abs(x) + abs(Hm) @ abs(x) @ abs(x) + 1.25)
    g = torch.zeros(n, dtype=torch.float64, device=DEV)
    qp_grad(Hop, _t(c), _t(x), g)
    assert np.allclose(_np(g), O.qp_grad(Hm, c, x), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("n", [1, 255, 257, 70_001])
def test_qp_obj_grad_sizes(n):
    """n = 1, one short of / one past a 256-thread workgroup, and 70,001 (> 256 x 256: k_dot2's 256
    workgroups stride twice, the last pass partial).  Same references and bounds as test_qp_obj_grad."""
    from madipm_amd.rocm_wrapper import MadIPMOperator, qp_obj, qp_grad
    from oracle import kkt_ops as O
    rng = np.random.default_rng(n)
    H = sp.tril(_random_csr(n, n, min(1.0, 5.0 / n), 6) + sp.eye(n)).tocsr()
    H.sort_indices()
    Hop = MadIPMOperator(n, n, _t(H.indptr.astype(np.int32)), _t(H.indices.astype(np.int32)), _t(H.data),
                         symmetric=True)
    Hm = O.operator_matrix(n, n, H.indptr, H.indices, H.data, "N", True)
    c, x = rng.standard_normal(n), rng.standard_normal(n)
    v = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    obj = qp_obj(Hop, _t(c), 1.25, _t(x), v)
    ref = O.qp_obj(Hm, c, 1.25, x)
    assert abs(obj - ref) <= 1e-13 * (abs(c) @ abs(x) + abs(Hm) @ abs(x) @ abs(x) + 1.25)
    assert np.allclose(_np(v), Hm @ x, rtol=1e-13, atol=1e-13)
    g = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    qp_grad(Hop, _t(c), _t(x), g)
    assert np.allclose(_np(g), O.qp_grad(Hm, c, x), rtol=1e-13, atol=1e-13)


def test_normal_kkt_constructor_pipeline():
    """NormalKKTSystem's construction on device arrays (src/KKT/normalkkt.jl:69-111): A_coo with
    values 1..nnz -> coo_to_csr -> A_csr_map; build_normal_system; compress_jacobian!; build_kkt!
    (assemble_normal_system! with D = 1 ./ pr_diag); then the LDL^T of C through the plugin
    boundary — the normal-equations solve equals the dense one."""
    from madipm_amd.rocm_wrapper import (coo_to_csr, build_normal_system, compress_jacobian,
                                         assemble_normal_system)
    from madipm_amd.linear_solver import HIPLDLSolver
    rng = np.random.default_rng(7)
    m, nx, ns = 300, 700, 40
    A = sp.random(m, nx, density=0.02, format="coo", random_state=rng, data_rvs=rng.standard_normal)
    ind_ineq = np.sort(rng.choice(m, ns, replace=False)).astype(np.int32)
    I = np.r_[A.row, ind_ineq].astype(np.int32)
    J = np.r_[A.col, nx + np.arange(ns)].astype(np.int32)
    ntot, nnz = nx + ns, A.nnz + ns
    # A_coo.V .= 1:nnz (0-based here); coo_to_csr; A_csr_map = convert.(Int, Ax)
    Ap, Aj, Ax = coo_to_csr(m, ntot, _t(I), _t(J), _t(np.arange(nnz, dtype=np.float64)), sort_cols=True)
    csr_map = Ax.to(torch.int64)
    Cp, Cj = build_normal_system(m, ntot, _np(Ap), _np(Aj))
    # jac values + compress_jacobian! (slack entries -1)
    V = _t(np.r_[A.data, np.zeros(ns)])
    ATnz = torch.zeros(nnz, dtype=torch.float64, device=DEV)
    compress_jacobian(V, ns, csr_map, ATnz)
    pr = rng.uniform(0.5, 5.0, ntot)
    Cx = torch.zeros(len(Cj), dtype=torch.float64, device=DEV)
    assemble_normal_system(m, ntot, Ap, Aj, ATnz, _t(Cp), _t(Cj), Cx, _t(1.0 / pr))
    Afull = sp.csr_matrix((np.r_[A.data, -np.ones(ns)], (I, J)), shape=(m, ntot))
    Cd = (Afull @ sp.diags(1.0 / pr) @ Afull.T).toarray()
    ls = HIPLDLSolver(m, Cp.astype(np.int64), Cj)
    assert ls.factorize(Cx) == 0
    b = rng.standard_normal(m)
    xb = _t(b)
    ls.solve(xb)
    xr = np.linalg.solve(Cd, b)
    assert np.max(np.abs(_np(xb) - xr)) <= 1e-10 * np.max(np.abs(xr))


@pytest.mark.parametrize("which", ["upper", "mixed"])
def test_ldl_either_triangle(which):
    """madipm_ldl_analyze / factorize on the upper triangle (LDLFactorizations' input) or a mixed
    one gives the lower-triangle factorisation's pivots and solution."""
    from helpers import random_k2
    from madipm_amd.linear_solver import HIPLDLSolver
    K, Lw = random_k2(200, 300, 0.02, 9, well=True)
    N = K.shape[0]
    if which == "upper":
        M = sp.triu(K).tocsc()
    else:
        T = sp.tril(K, -1).tocoo()
        flip = np.arange(T.nnz) % 3 == 0
        M = sp.csc_matrix((np.r_[T.data, K.diagonal()],
                           (np.r_[np.where(flip, T.col, T.row), np.arange(N)],
                            np.r_[np.where(flip, T.row, T.col), np.arange(N)])), shape=(N, N))
    M.sort_indices()
    low = HIPLDLSolver(N, Lw.indptr, Lw.indices)
    oth = HIPLDLSolver(N, M.indptr, M.indices)
    assert low.factorize(_t(Lw.data)) == 0 and oth.factorize(_t(M.data)) == 0
    if which == "upper":  # same adjacency order -> same ordering and pivots (a mixed input may break
        assert np.array_equal(low.perm(), oth.perm())  # AMD's ties differently: same solution only)
        assert np.allclose(low.diag(), oth.diag(), rtol=1e-13, atol=0)
    b = np.random.default_rng(1).standard_normal(N)
    x1, x2 = _t(b), _t(b)
    low.solve(x1)
    oth.solve(x2)
    r1, r2 = _np(x1), _np(x2)
    if which == "upper":
        assert np.max(np.abs(r1 - r2)) <= 1e-12 * np.max(np.abs(r1))
    # both are backward stable solves of K x = b (a different pivot order rounds differently)
    nK = abs(K).sum(axis=1).max()
    for r_ in (r1, r2):
        assert np.max(np.abs(K @ r_ - b)) <= 1e-13 * nK * np.max(np.abs(r_))
    assert low.inertia() == oth.inertia()
