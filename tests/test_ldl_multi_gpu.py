"""The multi-right-hand-side LDL^T solve (HIPLDLSolver.solve_multi) on the GPU.

Fixtures, the smallest shapes that reach each class of the multi-column levels (mlev):
  micro_tiny    random_k2(5, 8, 0.3, 0)                  micro / tiny fronts only
  tiny_small    random_k2(400, 900, 0.004, 4)            tiny + small
  block         block_angular_k2(3000, 4000, 20, 7)      small fronts of 16-150 columns and the 120-column root, all
                                                         of which the default plan solves in tree tasks
  dense         dense_k2(150, 1000, 5)                   its x columns form a batched-leaf group under every ordering
                                                         (lb_groups = 1, largest front 151 rows), so solve_multi is the
                                                         loop of single solves there: native == 0
  medium        test_ldl_medium_tree_fronts' fixture     medium tree fronts (192 < r <= 256), big in mlev
  qp_big        random_k2(150, 400, 0.05, 11, qp=True)   test_ldl_qp_dense_front's: fronts up to 279 rows and no
                                                         batched-leaf group, the per-column big route inside mlev
  batched_leaf  test_batched_leaf_columns_parity's (150, 1000, ordering 0): native == 0, the loop
Both `well` settings where the helper has them.  The criteria against the oracle factor's solve of the same column
are test_ldl_gpu._check_case's: forward difference <= 1e-12 (well) or 1e-6 (IPM-conditioned), backward error
<= 10 x the oracle's + 1e-15.
"""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from helpers import block_angular_k2, dense_k2, lp_k2, random_k2
from oracle.ldl import OracleLDL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W = 8
KS = (1, 7, 8, 9, 17)
NCOL = 17


def _medium(well):
    from madipm_amd import standard_form_qp
    from madipm_amd.instances import supportcase10_standin
    return lp_k2(standard_form_qp(supportcase10_standin(scale=0.05, block_scale=1.0)), 3, well=well)


# name -> (K2 maker(well), solver options, has an IPM-conditioned variant, native route expected)
CASES = {
    "micro_tiny": (lambda well: random_k2(5, 8, 0.3, 0, well=well), {}, True, 1),
    "tiny_small": (lambda well: random_k2(400, 900, 0.004, 4, well=well), {}, True, 1),
    "block": (lambda well: block_angular_k2(3000, 4000, 20, 7, well=well), {}, True, 1),
    "dense": (lambda well: dense_k2(150, 1000, 5), {}, False, 0),
    "medium": (_medium, {}, True, 1),
    "qp_big": (lambda well: random_k2(150, 400, 0.05, 11, qp=True, well=well), {}, True, 1),
    "batched_leaf": (lambda well: dense_k2(150, 1000, 3), {"ordering": 0}, False, 0),
}
PARAMS = [(c, w) for c, v in CASES.items() for w in ((True, False) if v[2] else (True,))]


class _State:
    pass


@functools.lru_cache(maxsize=None)
def _state(case, well):
    """One factorised solver, the oracle's factor in the same order, 17 distinct right-hand sides, the oracle's
    solutions and each column's solve_multi alone: computed once per fixture, shared, never changed."""
    from madipm_amd.linear_solver import HIPLDLSolver
    make, opts, _, native = CASES[case]
    K, Lw = make(well)
    st = _State()
    st.K, st.Lw, st.N, st.native = K, Lw, K.shape[0], native
    st.ls = HIPLDLSolver(st.N, Lw.indptr, Lw.indices, **opts)
    assert st.ls.factorize(torch.from_numpy(Lw.data.copy()).cuda()) == 0 and st.ls.is_factorized()
    st.ref = OracleLDL(K, st.ls.perm())
    assert st.ref.factorize() == st.N
    st.B = np.random.default_rng(17).standard_normal((NCOL, st.N))
    st.Xref = np.stack([st.ref.solve(st.B[j].copy()) for j in range(NCOL)])
    st.normK = spla.norm(K, np.inf)
    st.alone = np.stack([_multi(st.ls, st.B[j:j + 1])[0] for j in range(NCOL)])
    return st


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _state.cache_clear()      # the solvers go while the library is still loaded


def _multi(ls, B, stream=None):
    X = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    torch.cuda.synchronize()
    out = ls.solve_multi(X, stream=stream)
    assert out is X
    torch.cuda.synchronize()
    return X.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _berr(st, x, b):
    return np.max(np.abs(st.K @ x - b)) / (st.normK * np.max(np.abs(x)) + np.max(np.abs(b)))


@pytest.mark.parametrize("case,well", PARAMS)
def test_rows_do_not_depend_on_k_or_position(case, well):
    """Row j of solve_multi on k columns equals, bit for bit, solve_multi on that column alone, for k in
    {1, 7, 8, 9, 17} (a partial chunk, a full one, a chunk of one column after a full one, two full chunks and
    one column); multi_info() counts ceil(k / 8) chunks per call and reports the route."""
    st = _state(case, well)
    for k in KS:
        i0 = st.ls.multi_info()
        X = _multi(st.ls, st.B[:k])
        i1 = st.ls.multi_info()
        bad = np.flatnonzero((_bits(X) != _bits(st.alone[:k])).any(axis=1))
        assert bad.size == 0, f"k={k}: rows {bad[:8]} differ from the column alone"
        assert i1["n_calls"] - i0["n_calls"] == 1 and i1["n_columns"] - i0["n_columns"] == k
        assert i1["n_chunks"] - i0["n_chunks"] == -(-k // W)
    info = st.ls.multi_info()
    assert info["width"] == W and info["native"] == st.native, info
    assert info["native"] == int(st.ls.info()["lb_groups"] == 0)
    if case in ("medium", "qp_big"):
        assert info["n_big_fronts"] >= 1, info
    if case in ("micro_tiny", "tiny_small") or not info["native"]:
        assert info["n_big_fronts"] == 0, info
    if not info["native"]:  # the loop: the single solve's bits
        x = torch.from_numpy(st.B[3].copy()).cuda()
        st.ls.solve(x)
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(st.alone[3]))


@pytest.mark.parametrize("case,well", PARAMS)
def test_rows_match_the_oracle(case, well):
    st = _state(case, well)
    X = _multi(st.ls, st.B)
    for j in range(NCOL):
        x, xr, b = X[j], st.Xref[j], st.B[j]
        ferr = np.max(np.abs(x - xr)) / np.max(np.abs(xr))
        assert ferr <= (1e-12 if well else 1e-6), f"row {j}: forward difference {ferr:.3e}"
        bg, br = _berr(st, x, b), _berr(st, xr, b)
        assert bg <= 10 * br + 1e-15, f"row {j}: backward error gpu {bg:.3e} vs oracle {br:.3e}"


@pytest.mark.parametrize("case,well", [(c, True) for c in CASES])
def test_single_solve_keeps_its_bits_around_a_multi_solve(case, well):
    """solve(x) before and after a solve_multi returns the same bits (tree-path state, epochs, counters)."""
    st = _state(case, well)

    def single():
        x = torch.from_numpy(st.B[0].copy()).cuda()
        st.ls.solve(x)
        torch.cuda.synchronize()
        return x.cpu().numpy()
    before = single()
    _multi(st.ls, st.B[:9])
    after = single()
    assert np.array_equal(_bits(before), _bits(after))
    _multi(st.ls, st.B[:1])
    assert np.array_equal(_bits(before), _bits(single()))


def test_multi_solve_right_after_a_refactorisation():
    """A refactorisation with new values followed at once by solve_multi (the factorisation's root tail may still
    be on its side stream: the route joins it) is correct, for every new factor, and the single solve after it
    is the single solve's."""
    from madipm_amd.linear_solver import HIPLDLSolver
    for make in (lambda: random_k2(200, 300, 0.01, 5, well=True), lambda: block_angular_k2(3000, 4000, 20, 7, well=True)):
        K, Lw = make()
        N = K.shape[0]
        ls = HIPLDLSolver(N, Lw.indptr, Lw.indices)
        perm = ls.perm()
        B = np.random.default_rng(2).standard_normal((9, N))
        for it in range(3):
            vals = Lw.data.copy()
            diag = Lw.indices == np.repeat(np.arange(N), np.diff(Lw.indptr))
            vals[diag] *= (1.0 + it)
            Kn = K.copy().tolil()
            Kn.setdiag(K.diagonal() * (1.0 + it))
            Kn = Kn.tocsc()
            X = torch.from_numpy(B.copy()).cuda()
            assert ls.factorize(torch.from_numpy(vals).cuda()) == 0
            ls.solve_multi(X)
            x1 = torch.from_numpy(B[0].copy()).cuda()
            ls.solve(x1)
            torch.cuda.synchronize()
            ref = OracleLDL(Kn, perm)
            assert ref.factorize() == N
            for j in range(9):
                xr = ref.solve(B[j].copy())
                for x in ((X[j].cpu().numpy(),) if j else (X[0].cpu().numpy(), x1.cpu().numpy())):
                    assert np.max(np.abs(x - xr)) <= 1e-12 * np.max(np.abs(xr)), (it, j)


@pytest.mark.parametrize("case", ["tiny_small", "block", "medium", "qp_big"])
def test_zero_and_nan_columns_stay_in_their_column(case):
    st = _state(case, True)
    for k, j in ((9, 4), (9, 8), (3, 0)):
        B = st.B[:k].copy()
        B[j] = 0.0
        X = _multi(st.ls, B)
        assert not X[j].any(), "a column of zeros gives zeros"
        others = [i for i in range(k) if i != j]
        assert np.array_equal(_bits(X[others]), _bits(st.alone[others]))
        B[j] = st.B[j]
        B[j, st.N // 2] = np.nan
        X = _multi(st.ls, B)
        assert np.isnan(X[j]).any()
        assert np.array_equal(_bits(X[others]), _bits(st.alone[others])), "NaN leaked into another column"


@pytest.mark.parametrize("case", ["block", "qp_big", "batched_leaf"])
def test_side_stream_gives_the_same_bits(case):
    st = _state(case, True)
    side = torch.cuda.Stream()
    X = _multi(st.ls, st.B[:9], stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(_bits(X), _bits(st.alone[:9]))


def test_refusals_before_any_library_call():
    st = _state("micro_tiny", True)
    ls, N = st.ls, st.N
    good = torch.zeros((3, N), dtype=torch.float64, device="cuda")
    before = ls.multi_info()
    with pytest.raises(TypeError):
        ls.solve_multi(torch.zeros((3, N), dtype=torch.float64))            # a CPU tensor
    with pytest.raises(TypeError):
        ls.solve_multi(np.zeros((3, N)))                                   # not a tensor
    with pytest.raises(TypeError):
        ls.solve_multi(good.to(torch.float32))
    with pytest.raises(ValueError):
        ls.solve_multi(good[0])                                            # 1-D
    with pytest.raises(ValueError):
        ls.solve_multi(torch.zeros((3, N + 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ls.solve_multi(torch.zeros((0, N), dtype=torch.float64, device="cuda"))   # k = 0
    with pytest.raises(ValueError):
        ls.solve_multi(torch.zeros((N, 3), dtype=torch.float64, device="cuda").t())  # (3, N), not contiguous
    assert ls.multi_info() == before, "a refused call reached the library"
