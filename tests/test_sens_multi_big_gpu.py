"""Batched sensitivities on a QP whose KKT factor has big fronts, with the multi-right-hand-side solve on (DESIGN
§13k): the rows of tangent_batch / adjoint_batch have the bits of a solver built under MADIPM_MULTI_BIG=0 (the big
fronts column after column), agree with the single calls within test_sens_multi_gpu's bound, and the big-pass
counter follows 2 n_big_levels per chunk (times the chunk's columns under MADIPM_MULTI_BIG=0).

The QP: 200 variables with a dense 200 x 200 Hessian block, 40 sparse rows of four entries, box bounds.  Its KKT
factor has no batched-leaf group and a front past 192 rows (asserted).  Largest difference of a row to the single
call's measured on the MI355X: 1.78e-15, under test_sens_multi_gpu's bound of 5.7e-15."""
from __future__ import annotations

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import adjoint_oracle as O  # noqa: E402
import tangent_oracle as T  # noqa: E402
import test_sens_batch_gpu as B  # noqa: E402  (its columns, stacking and solver options)
from test_sens_multi_gpu import MULTI_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 9)
_cache = {}


def dense_block_qp(n=200, m=40, seed=5):
    from madipm_amd.qp import QuadraticModel
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, n))
    H = np.tril(P @ P.T / n + np.eye(n))
    hr, hc = np.nonzero(H)
    rows = np.repeat(np.arange(m), 4)
    cols = np.concatenate([rng.choice(n, 4, replace=False) for _ in range(m)])
    A = sp.coo_matrix((rng.standard_normal(4 * m), (rows, cols)), shape=(m, n)).tocsr().tocoo()
    x0 = rng.uniform(0.2, 0.8, n)
    b = A @ x0
    return QuadraticModel(c=rng.standard_normal(n), Hrows=hr, Hcols=hc, Hvals=H[hr, hc], Arows=A.row, Acols=A.col,
                          Avals=A.data, lcon=b, ucon=b.copy(), lvar=np.zeros(n), uvar=np.ones(n),
                          name="dense_block_200_40")


def _case(monkeypatch):
    """The QP solved by two solvers, the default one and one built under MADIPM_MULTI_BIG=0, and the single calls
    of the nine seeded columns on the first: computed once."""
    if not _cache:
        qp = dense_block_qp()
        gx = np.random.default_rng(41).uniform(0.5, 1.5, qp.nvar)
        d, cot = B._columns(qp, gx, max(KS))
        on = B._new_solver(qp, {}, None)
        monkeypatch.setenv("MADIPM_MULTI_BIG", "0")
        off = B._new_solver(qp, {}, None)
        monkeypatch.delenv("MADIPM_MULTI_BIG")
        for s in (on, off):
            st = s.solve()
            assert st.status == 1, st.status_name
        t = [on.tangent(**d[j]) for j in range(max(KS))]
        g = [on.adjoint(**cot[j]) for j in range(max(KS))]
        _cache.update(qp=qp, d=d, cot=cot, on=on, off=off, t=t, g=g)
    return _cache


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    _cache.clear()            # the solvers go while the library is still loaded


def test_the_qp_has_big_fronts_on_the_native_route(monkeypatch):
    c = _case(monkeypatch)
    on, off = c["on"].multi_solve_info(), c["off"].multi_solve_info()
    assert on["native"] == 1 and on["n_big_fronts"] >= 1 and on["n_big_levels"] >= 1, on
    assert on["multi_big"] == 1 and off["multi_big"] == 0, (on, off)
    assert {k: on[k] for k in ("native", "n_big_fronts", "n_big_levels")} == \
        {k: off[k] for k in ("native", "n_big_fronts", "n_big_levels")}


def test_rows_have_the_bits_of_the_per_column_route_and_match_the_single_calls(monkeypatch):
    c = _case(monkeypatch)
    on, off = c["on"], c["off"]
    nlev = on.multi_solve_info()["n_big_levels"]
    worst = 0.0
    for s in (on, off):
        s.set_multi_solve(True)
    try:
        for k in KS:
            i0, j0 = on.multi_solve_info(), off.multi_solve_info()
            tb, to = on.tangent_batch(**B._stack(c["d"], k)), off.tangent_batch(**B._stack(c["d"], k))
            gb, go = on.adjoint_batch(**B._stack(c["cot"], k)), off.adjoint_batch(**B._stack(c["cot"], k))
            i1, j1 = on.multi_solve_info(), off.multi_solve_info()
            for got, ref, keys, what in ((tb, to, T.OUTS, "tangent"), (gb, go, O.NAMES, "adjoint")):
                for key in keys:
                    x, y = B._np(got[key]), B._np(ref[key])
                    assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, k, key)
            for batch, singles, keys, what in ((tb, c["t"], T.OUTS, "tangent"), (gb, c["g"], O.NAMES, "adjoint")):
                for key in keys:
                    for j in range(k):
                        e = O.err(B._np(batch[key])[j], B._np(singles[j][key]))
                        worst = max(worst, e)
                        assert e <= MULTI_TOL, (what, k, key, j, e)
            assert i1["n_chunks"] > i0["n_chunks"] and i1["n_columns"] - i0["n_columns"] == j1["n_columns"] - j0["n_columns"]
            assert i1["n_big_passes"] - i0["n_big_passes"] == 2 * nlev * (i1["n_chunks"] - i0["n_chunks"]), (k, i0, i1)
            assert j1["n_big_passes"] - j0["n_big_passes"] == 2 * nlev * (j1["n_columns"] - j0["n_columns"]), (k, j0, j1)
            assert i1["big_bytes"] > 0 and j1["big_bytes"] == 0
    finally:
        for s in (on, off):
            s.set_multi_solve(False)
    print("sens multi big", f"largest difference to the single calls {worst:.2e}")
