"""The big fronts of the multi-right-hand-side LDL^T solve carry a chunk's columns in one pass.

HIPLDLSolver.set_multi_big(True) (the default) solves the big fronts of solve_multi's levels with the multi-column
task-queue kernels, one pass per level and direction for a chunk of up to 8 columns; set_multi_big(False) keeps
the single-column kernels, column after column.  The claim is that both give the same bits.

Fixtures; (w, b, children) is a front of w pivots and r = w + b rows (helpers.front_tree_k2, FRONT_TREE_OPTS,
MADIPM_BIG_MERGE=0):
  deep    root (300, 0, [A, A, (2, 5, []), (20, 30, [])]), A = (130, 290, []), N = 582.  A: r = 420, 7 forward row
          blocks (the last of 36 rows), 3 pivot panels (the last of 2 columns: the hand-off is read twice in each
          direction), 2 chunks of 256 rows below the pivots (the second of 34 rows).  Root: r = w = 300, 5 panels
          (the last of 44 columns), no rows below; it gathers from two big children, a micro and a small one.  Big
          fronts at two levels.
  edges   root (129, 0, [(64, 129, []), (65, 129, []), (128, 129, [])]): r = 193 (the smallest big front, one full
          panel, a last row block of 1 row), r = 194 (a second panel of 1 column), r = 257 (two full panels, a last
          row block of 1 row); the root is small in the multi levels (129 x 129) and reads the big children's
          update vectors.
  medium, qp_big   the makers of test_ldl_multi_gpu.py: a real ordering's medium tree fronts and 279-row fronts,
          well conditioned and IPM-conditioned.
Criteria against the oracle's solve in the solver's order: forward difference <= 1e-12 (well conditioned) or 1e-6
(IPM-conditioned), backward error <= 10 x the oracle's + 1e-15 (test_ldl_multi_gpu.test_rows_match_the_oracle's).
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from helpers import FRONT_TREE_OPTS, front_tree_k2, lp_k2, perturbed_values, random_k2
from oracle.ldl import OracleLDL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W = 8
KS = (1, 7, 8, 9, 17)
NCOL = 17

_A = (130, 290, [])
DEEP = (300, 0, [_A, _A, (2, 5, []), (20, 30, [])])
EDGES = (129, 0, [(64, 129, []), (65, 129, []), (128, 129, [])])


def _tree(root, seed):
    K, Lw, _ = front_tree_k2(root, seed)
    return K, Lw


def _medium(well):
    from madipm_amd import standard_form_qp
    from madipm_amd.instances import supportcase10_standin
    return lp_k2(standard_form_qp(supportcase10_standin(scale=0.05, block_scale=1.0)), 3, well=well)


# name -> (K2 maker(well), solver options, prescribed fronts, n_big_fronts (None: >= 1), n_big_levels or None)
CASES = {
    "deep": (lambda well: _tree(DEEP, 31), FRONT_TREE_OPTS, True, 3, 2),
    "edges": (lambda well: _tree(EDGES, 32), FRONT_TREE_OPTS, True, 3, None),
    "medium": (_medium, {}, False, None, None),
    "qp_big": (lambda well: random_k2(150, 400, 0.05, 11, qp=True, well=well), {}, False, None, None),
}
PARAMS = [("deep", True), ("edges", True), ("medium", True), ("medium", False), ("qp_big", True), ("qp_big", False)]
WELL = [(c, True) for c in CASES]


class _State:
    pass


_STATES = {}


def _state(case, well, monkeypatch):
    """One factorised solver, the oracle's factor in the same order, 17 distinct right-hand sides and the oracle's
    solutions: computed once per fixture, shared, never changed (a test that refactorises builds its own)."""
    if (case, well) not in _STATES:
        st = _new(case, well, monkeypatch)
        st.ref = OracleLDL(st.K, st.ls.perm())
        assert st.ref.factorize() == st.N
        st.Xref = np.stack([st.ref.solve(st.B[j].copy()) for j in range(NCOL)])
        st.normK = spla.norm(st.K, np.inf)
        _STATES[(case, well)] = st
    st = _STATES[(case, well)]
    st.ls.set_multi_big(True)
    return st


def _new(case, well, monkeypatch):
    from madipm_amd.linear_solver import HIPLDLSolver
    make, opts, prescribed, nbig, nlev = CASES[case]
    if prescribed:
        monkeypatch.setenv("MADIPM_BIG_MERGE", "0")
    K, Lw = make(well)
    st = _State()
    st.K, st.Lw, st.N = K, Lw, K.shape[0]
    st.ls = HIPLDLSolver(st.N, Lw.indptr, Lw.indices, **opts)
    info = st.ls.multi_info()
    assert info["native"] == 1 and info["width"] == W and info["multi_big"] == 1, info
    assert info["n_big_fronts"] == nbig if nbig is not None else info["n_big_fronts"] >= 1, info
    assert info["n_big_levels"] == nlev if nlev is not None else info["n_big_levels"] >= 1, info
    assert st.ls.factorize(torch.from_numpy(Lw.data.copy()).cuda()) == 0 and st.ls.is_factorized()
    st.B = np.random.default_rng(17).standard_normal((NCOL, st.N))
    return st


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _STATES.clear()           # the solvers go while the library is still loaded


def _multi(ls, B, stream=None):
    X = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    torch.cuda.synchronize()
    out = ls.solve_multi(X, stream=stream)
    assert out is X
    torch.cuda.synchronize()
    return X.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _berr(K, normK, x, b):
    return np.max(np.abs(K @ x - b)) / (normK * np.max(np.abs(x)) + np.max(np.abs(b)))


def _check_oracle(K, normK, X, Xref, B, well, what):
    for j in range(len(X)):
        x, xr, b = X[j], Xref[j], B[j]
        ferr = np.max(np.abs(x - xr)) / np.max(np.abs(xr))
        assert ferr <= (1e-12 if well else 1e-6), f"{what} row {j}: forward difference {ferr:.3e}"
        bg, br = _berr(K, normK, x, b), _berr(K, normK, xr, b)
        assert bg <= 10 * br + 1e-15, f"{what} row {j}: backward error gpu {bg:.3e} vs oracle {br:.3e}"


@pytest.mark.parametrize("case,well", PARAMS)
def test_rows_have_the_bits_of_the_per_column_route(case, well, monkeypatch):
    """solve_multi of the same 17 columns with set_multi_big(False) and with set_multi_big(True), for k in
    {1, 7, 8, 9, 17}: every row bit for bit the per-column route's row of the 17-column call (so a row depends
    neither on k nor on its position, on either route); again after a refactorisation with perturbed values."""
    st = _new(case, well, monkeypatch)
    ls = st.ls
    for which in range(2):
        if which:
            vals2, _ = perturbed_values(st.Lw, 5)
            assert ls.factorize(torch.from_numpy(vals2).cuda()) == 0
        ls.set_multi_big(False)
        ref = _multi(ls, st.B)
        assert np.isfinite(ref).all()
        for on in (True, False):
            ls.set_multi_big(on)
            assert ls.multi_info()["multi_big"] == int(on)
            for k in KS:
                X = _multi(ls, st.B[:k])
                bad = np.flatnonzero((_bits(X) != _bits(ref[:k])).any(axis=1))
                assert bad.size == 0, (f"{'refactorised' if which else 'first'} multi_big={int(on)} k={k}: rows "
                                       f"{bad[:8]} differ from the per-column route, max "
                                       f"{np.max(np.abs(X[bad] - ref[bad])):.3e}")


@pytest.mark.parametrize("case,well", WELL)
def test_counters(case, well, monkeypatch):
    """n_big_passes grows by 2 n_big_levels ceil(k / 8) per call with the route on and by 2 n_big_levels k with it
    off; big_bytes is 0 before the first on-call and positive after it."""
    st = _new(case, well, monkeypatch)
    ls = st.ls
    nlev = ls.multi_info()["n_big_levels"]
    assert ls.multi_info()["big_bytes"] == 0 and ls.multi_info()["n_big_passes"] == 0
    ls.set_multi_big(False)
    for k in (1, 9):
        i0 = ls.multi_info()
        _multi(ls, st.B[:k])
        i1 = ls.multi_info()
        assert i1["n_big_passes"] - i0["n_big_passes"] == 2 * nlev * k, (k, i0, i1)
        assert i1["big_bytes"] == 0 and i1["multi_big"] == 0
    ls.set_multi_big(True)
    for k in KS:
        i0 = ls.multi_info()
        _multi(ls, st.B[:k])
        i1 = ls.multi_info()
        assert i1["n_big_passes"] - i0["n_big_passes"] == 2 * nlev * -(-k // W), (k, i0, i1)
        assert i1["big_bytes"] > 0 and i1["multi_big"] == 1
        assert i1["n_big_fronts"] == i0["n_big_fronts"] and i1["n_big_levels"] == nlev


def test_counters_without_big_fronts():
    from madipm_amd.linear_solver import HIPLDLSolver
    K, Lw = random_k2(5, 8, 0.3, 0, well=True)
    ls = HIPLDLSolver(K.shape[0], Lw.indptr, Lw.indices)
    assert ls.factorize(torch.from_numpy(Lw.data.copy()).cuda()) == 0
    B = np.random.default_rng(1).standard_normal((9, K.shape[0]))
    for on in (True, False):
        ls.set_multi_big(on)
        _multi(ls, B)
        info = ls.multi_info()
        assert info["native"] == 1 and info["n_big_fronts"] == 0 and info["n_big_levels"] == 0, info
        assert info["n_big_passes"] == 0 and info["big_bytes"] == 0 and info["multi_big"] == int(on), info


@pytest.mark.parametrize("case,well", PARAMS)
def test_rows_match_the_oracle(case, well, monkeypatch):
    st = _state(case, well, monkeypatch)
    X = _multi(st.ls, st.B)
    _check_oracle(st.K, st.normK, X, st.Xref, st.B, well, case)


@pytest.mark.parametrize("case,well", WELL)
def test_columns_stay_apart_and_in_bounds(case, well, monkeypatch):
    """A zero column gives zeros; a NaN in column j stays in row j and the other rows keep their bits; X is the
    leading k rows of a (k + 2, N) tensor whose last two rows hold a sentinel that the call leaves alone."""
    st = _state(case, well, monkeypatch)
    alone = _multi(st.ls, st.B)
    for k, j in ((9, 4), (9, 8), (3, 0)):
        B = st.B[:k].copy()
        B[j] = 0.0
        X = _multi(st.ls, B)
        assert not X[j].any(), "a column of zeros gives zeros"
        others = [i for i in range(k) if i != j]
        assert np.array_equal(_bits(X[others]), _bits(alone[others]))
        B[j] = st.B[j]
        B[j, st.N // 2] = np.nan
        X = _multi(st.ls, B)
        assert np.isnan(X[j]).any()
        assert np.array_equal(_bits(X[others]), _bits(alone[others])), "NaN leaked into another column"
        full = torch.full((k + 2, st.N), -12345.678, dtype=torch.float64, device="cuda")
        full[:k] = torch.from_numpy(st.B[:k]).cuda()
        torch.cuda.synchronize()
        st.ls.solve_multi(full[:k])
        torch.cuda.synchronize()
        full = full.cpu().numpy()
        assert np.array_equal(_bits(full[:k]), _bits(alone[:k]))
        assert (full[k:] == -12345.678).all(), "the call wrote past its k rows"


@pytest.mark.parametrize("case,well", WELL)
def test_neighbours(case, well, monkeypatch):
    """solve(x) keeps its bits around an on-call; an on-call on a side stream returns the default stream's bits."""
    st = _state(case, well, monkeypatch)

    def single():
        x = torch.from_numpy(st.B[0].copy()).cuda()
        st.ls.solve(x)
        torch.cuda.synchronize()
        return x.cpu().numpy()
    before = single()
    X = _multi(st.ls, st.B[:9])
    assert np.array_equal(_bits(before), _bits(single()))
    _multi(st.ls, st.B[:1])
    assert np.array_equal(_bits(before), _bits(single()))
    side = torch.cuda.Stream()
    Xs = _multi(st.ls, st.B[:9], stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(_bits(Xs), _bits(X))


@pytest.mark.parametrize("case", ["deep", "qp_big"])
def test_on_call_right_after_a_factorisation(case, monkeypatch):
    """factorize with new values followed at once by solve_multi (the factorisation's root tail may still be on its
    side stream: the route joins it) passes the oracle check for the new factor."""
    st = _new(case, True, monkeypatch)
    vals2, K2 = perturbed_values(st.Lw, 9)
    X = torch.from_numpy(st.B[:9].copy()).cuda()
    assert st.ls.factorize(torch.from_numpy(vals2).cuda()) == 0
    st.ls.solve_multi(X)
    torch.cuda.synchronize()
    ref = OracleLDL(K2, st.ls.perm())
    assert ref.factorize() == st.N
    Xref = np.stack([ref.solve(st.B[j].copy()) for j in range(9)])
    _check_oracle(K2, spla.norm(K2, np.inf), X.cpu().numpy(), Xref, st.B, True, case)
