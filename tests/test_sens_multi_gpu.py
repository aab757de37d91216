"""Batched sensitivities on the multi-right-hand-side LDL^T solve (MPCSolver.set_multi_solve).

With the switch on, tangent_batch / adjoint_batch at the interior point solve every chunk of columns, a chunk of
one column included, in one pass over the factor.  The claims: a row's bits do not depend on k; every block of
every row is within 2 x FORMULA_TOL of the single call's (both are within FORMULA_TOL of the same formulas:
test_tangent_gpu.FORMULA_TOL), relative to max(1, max |block|); the residual, the counters and the solver's
state are the single calls'; with the switch off again every bit is back; on a sharded solver the switch falls
back to the loop.  Fixtures, columns and the single calls are test_sens_batch_gpu's.

Largest difference to the single calls measured on the MI355X, over every block of every row of tangent_batch,
adjoint_batch (all cotangents, and gx alone) and the QPLayer Jacobian on the six fixtures: MULTI_MEASURED below;
the bound is 10 x it and may not exceed the cap."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

import adjoint_oracle as O  # noqa: E402
import tangent_oracle as T  # noqa: E402
import test_polish_gpu as G  # noqa: E402
import test_sens_batch_gpu as B  # noqa: E402  (its fixtures, columns and single calls)
from test_tangent_gpu import FORMULA_TOL  # noqa: E402
from test_update_gpu import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

MULTI_MEASURED = 5.7e-16     # rowlength_g4 (5.65e-16); sparse_g64 4.36e-16; the other four fixtures and the layer: 0
MULTI_TOL = 10.0 * MULTI_MEASURED
MULTI_CAP = 2.0 * FORMULA_TOL
RESIDUAL_FACTOR = 10.0       # the batch's last_residual against the single calls' largest: the same factor

NAMES = ("family_min", "lp", "rowlength_g4", "sparse_g64", "no_bounds", "no_rows")
KS = (1, 8, 9)


@pytest.fixture(scope="module", autouse=True)
def _release_solvers():
    yield
    B._cache.clear()          # the solvers go while the library is still loaded


@contextlib.contextmanager
def multi(s):
    s.set_multi_solve(True)
    try:
        yield s
    finally:
        s.set_multi_solve(False)


def _bits_equal(a, b, keys, what):
    for key in keys:
        x, y = B._np(a[key]), B._np(b[key])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, key)


def _close(batch, singles, keys, what):
    """Every block of every row within MULTI_TOL of the single call's; returns the largest difference."""
    worst = 0.0
    for key in keys:
        b = B._np(batch[key])
        assert b.shape == (len(singles), singles[0][key].shape[0]), (what, key, b.shape)
        for j, one in enumerate(singles):
            e = O.err(b[j], B._np(one[key]))
            worst = max(worst, e)
            assert e <= MULTI_TOL, (what, key, j, e)
    return worst


def test_tolerance_fits_the_cap():
    assert B.W() == 8 and MULTI_TOL <= MULTI_CAP


@pytest.mark.parametrize("name", NAMES)
def test_rows_do_not_depend_on_k_and_match_the_single_calls(name):
    c = B.case(name)
    s = c["solver"]
    kmax = max(KS)
    worst = 0.0
    with multi(s):
        i0 = s.multi_solve_info()
        assert i0["native"] == 1 and i0["width"] == 8, i0
        ref = None
        for k in sorted(KS, reverse=True):
            tb = s.tangent_batch(**B._stack(c["d"], k))
            rt = s.tangent_info()["last_residual"]
            gb = s.adjoint_batch(**B._stack(c["cot"], k))
            rg = s.adjoint_info()["last_residual"]
            xb = s.adjoint_batch(B._stack(c["cot"], k, ("gx",))["gx"])
            rx = s.adjoint_info()["last_residual"]
            if ref is None:
                ref = (tb, gb, xb)
            for got, want, keys, what in ((tb, ref[0], T.OUTS, "tangent"), (gb, ref[1], O.NAMES, "adjoint"),
                                          (xb, ref[2], O.NAMES, "adjoint of gx")):
                _bits_equal(got, {key: B._np(want[key])[:k] for key in keys}, keys, (what, k, "against k = 9"))
            worst = max(worst, _close(tb, c["t"][:k], T.OUTS, ("tangent", k)),
                        _close(gb, c["g"][:k], O.NAMES, ("adjoint", k)),
                        _close(xb, c["gxo"][:k], O.NAMES, ("adjoint of gx", k)))
            assert rt <= RESIDUAL_FACTOR * max(c["rt"][:k]), (k, rt, max(c["rt"][:k]))
            assert rg <= RESIDUAL_FACTOR * max(c["rg"][:k]), (k, rg, max(c["rg"][:k]))
            assert rx <= RESIDUAL_FACTOR * max(c["rx"][:k]), (k, rx, max(c["rx"][:k]))
        i1 = s.multi_solve_info()
        assert i1["n_calls"] > i0["n_calls"] and i1["n_chunks"] - i0["n_chunks"] == i1["n_calls"] - i0["n_calls"]
        # the single calls do not take the switch
        for key in T.OUTS:
            assert np.array_equal(s.tangent(**c["d"][1])[key], c["t"][1][key]), key
        for key in O.NAMES:
            assert np.array_equal(s.adjoint(**c["cot"][1])[key], c["g"][1][key]), key
        assert s.multi_solve_info() == i1
    print("multi-solve", name, f"largest difference to the single calls {worst:.2e}")
    assert s.adjoint_info()["n_adjoint_factorizations"] == 1
    # with the switch off again the batch returns the single calls' bits
    B._rows_equal(s.tangent_batch(**B._stack(c["d"], kmax)), c["t"][:kmax], T.OUTS, "tangent, switch off")
    B._rows_equal(s.adjoint_batch(**B._stack(c["cot"], kmax)), c["g"][:kmax], O.NAMES, "adjoint, switch off")
    assert s.multi_solve_info() == i1


@pytest.mark.parametrize("name", ["family_min", "sparse_g64"])
def test_the_switch_leaves_the_next_solve_alone(name):
    c = B.case(name)
    a = B._new_solver(c["qp"], c["extra"], c["width"])
    first = a.solve()
    a.set_multi_solve(True)
    a.tangent_batch(**B._stack(c["d"], 9))
    a.adjoint_batch(**B._stack(c["cot"], 9))
    assert a.multi_solve_info()["n_calls"] > 0
    second = a.solve()
    b = B._new_solver(c["qp"], c["extra"], c["width"])
    assert_same(first, b.solve())
    assert_same(second, b.solve())


def test_sharded_solver_takes_the_loop():
    c = B.case("sparse_2shards")
    s, k = c["solver"], 9
    with multi(s):
        info = s.multi_solve_info()
        assert info["native"] == 0, info
        B._rows_equal(s.tangent_batch(**B._stack(c["d"], k)), c["t"][:k], T.OUTS, "tangent, two shards")
        B._rows_equal(s.adjoint_batch(**B._stack(c["cot"], k)), c["g"][:k], O.NAMES, "adjoint, two shards")
        after = s.multi_solve_info()
        assert after["native"] == 0 and after["n_columns"] > info["n_columns"]


def test_layer_jacobian_with_the_switch():
    from madipm_amd import QPLayer
    qp = G.problem("family_3")
    s = G.new_solver("family_3")
    data = {k: torch.as_tensor(np.asarray(getattr(qp, k), float), device="cuda") for k in O.NAMES}
    layer = QPLayer(s, outputs=("x", "y"))
    layer(**data)
    wrt = {"c": None, "lcon": [0, 2]}
    off, off_rev = layer.jacobian(wrt), layer.jacobian(wrt, mode="reverse")
    with multi(s):
        on, on_rev = layer.jacobian(wrt), layer.jacobian(wrt, mode="reverse")
        assert s.multi_solve_info()["n_calls"] > 0
    worst = 0.0
    for key in off:
        for J, ref in ((on, off), (on_rev, off_rev)):
            worst = max(worst, O.err(J[key].cpu().numpy(), ref[key].cpu().numpy()))
    print("multi-solve layer jacobian", f"largest difference to the switch off {worst:.2e}")
    assert worst <= MULTI_TOL, worst
    again = layer.jacobian(wrt)
    for key in off:
        assert torch.equal(again[key], off[key]), key
