"""The oracle of the forward-mode sensitivities (tangent_oracle.py) against central differences,
its two forms against each other, the transpose identity with the adjoint's oracle, the entries that are not
read, the conditions the fixtures of test_tangent_gpu.py must meet, and the argument checks of
MPCSolver.tangent / tangent_device and QPFunction.jvp — all without a GPU."""
from __future__ import annotations

import numpy as np
import pytest

import adjoint_full_oracle as F
import adjoint_oracle as O
import tangent_oracle as T

# Central differences (h = 1e-6) of (x, y, zl, zu, A x) through reference_ipm along directions(qp, 0) against the
# two forms at reference_ipm's optimum, largest err over the five blocks as measured with this file:
# name -> (problem, shifted vs differences, plain vs differences, plain vs shifted).  The bound of the shifted
# form is 10 x its value.
FD_FIXTURES = {
    "family0": (lambda: O.family(0), 1.8e-10, 1.4e-7, 1.4e-7),
    "family1": (lambda: O.family(1), 2.2e-10, 5.7e-10, 7.6e-10),
    "family2": (lambda: O.family(2), 8.2e-11, 1.5e-7, 1.4e-7),
    "family3": (lambda: O.family(3), 1.2e-9, 6.2e-7, 6.1e-7),
    "family0_max": (lambda: O.family(0, minimize=False), 1.5e-10, 6.3e-8, 6.3e-8),
    "family0_dup": (lambda: O.duplicated_family(0)[:2], 4.1e-10, 5.0e-8, 4.9e-8),
    "lp": (O.lp_fixture, 2.8e-10, 5.4e-7, 5.4e-7),
    "family0_scaled": (lambda: O.scaled_family(0), 2.2e-9, 1.1e-4, 1.1e-4),
    "rowlength": (F.rowlength_fixture, 6.5e-10, 2.4e-7, 2.3e-7),
}
# the problems test_tangent_gpu.py solves (test_adjoint_full_gpu.py's)
GPU_FIXTURES = {
    "family_min": lambda: O.family(1),
    "family_max": lambda: O.family(1, minimize=False),
    "family_scaled": lambda: O.scaled_family(1),
    "family_dup": lambda: O.duplicated_family(1)[:2],
    "family_seed3": lambda: O.family(3),
    "lp": O.lp_fixture,
    "sparse": O.sparse_fixture,
    "rowlength": F.rowlength_fixture,
}
_solved = {}


def solved(make):
    """(qp, directions, cotangents, reference point) of a fixture, computed once and never modified."""
    if make not in _solved:
        qp, gx = make()
        _solved[make] = (qp, T.directions(qp, 0), F.cotangents(qp, gx), O.reference_ipm(qp))
    return _solved[make]


def _all_fixtures():
    out = {k: v[0] for k, v in FD_FIXTURES.items()}
    out.update({"gpu_" + k: v for k, v in GPU_FIXTURES.items()})
    return out


@pytest.mark.parametrize("name", list(FD_FIXTURES))
def test_shifted_form_matches_central_differences(name):
    make, measured, _, _ = FD_FIXTURES[name]
    qp, d, _, pt = solved(make)
    fd = T.finite_difference(qp, d, h=1e-6)
    ts, tp = T.reference_tangent(qp, pt, d, "shifted"), T.reference_tangent(qp, pt, d, "plain")
    es = {k: O.err(ts[k], fd[k]) for k in T.OUTS}
    ep = {k: O.err(tp[k], fd[k]) for k in T.OUTS}
    gap = T.max_err(tp, ts)
    print(name, "shifted", f"{max(es.values()):.2e}", "plain", f"{max(ep.values()):.2e}", "plain-shifted", f"{gap:.2e}")
    assert max(es.values()) <= 10.0 * measured, es
    if gap > 1e-7:       # where the forms differ visibly, the plain one is the worse
        assert max(ep.values()) > max(es.values()), (es, ep)


@pytest.mark.parametrize("name", list(_all_fixtures()))
def test_tangent_is_the_transpose_of_the_adjoint(name):
    """<cot, tangent(d)> = <adjoint(cot), d> for all five cotangents and all seven directions: two dense solves
    with the same 17 x 17 ... 90 x 90 matrix (the sparse fixture: a sparse LU of 2180 unknowns), rounding only.
    Measured: <= 1.5e-14 (the sparse fixture), <= 1.8e-15 on the dense ones."""
    qp, d, cot, pt = solved(_all_fixtures()[name])
    t = T.reference_tangent(qp, pt, d)
    g = F.reference_adjoint_full(qp, pt, cot)
    a, b = T.dot(cot, t), T.dot_data(g, qp, d)
    print(name, a, b, f"{abs(a - b) / max(1.0, abs(a)):.1e}")
    assert abs(a - b) <= 1e-12 * max(1.0, abs(a))
    # and for each cotangent alone against each direction block alone on one fixture
    if name == "gpu_family_seed3":
        for c in F.COTS:
            gc = F.reference_adjoint_full(qp, pt, F.only(cot, c))
            for k in T.NAMES:
                tk = T.reference_tangent(qp, pt, T.only(d, k))
                a, b = T.dot(F.only(cot, c), tk), T.dot_data(gc, qp, T.only(d, k))
                assert abs(a - b) <= 1e-12 * max(1.0, abs(a)), (c, k)


@pytest.mark.parametrize("name", list(_all_fixtures()))
def test_not_read_entries_are_not_read(name):
    """NaN on the infinite bounds, in duvar of the fixed variables and in ducon of the equality rows leaves
    every bit as it is, in both forms."""
    qp, d, _, pt = solved(_all_fixtures()[name])
    dn = T.with_nan(qp, d)
    if name in ("family3", "gpu_family_min", "gpu_sparse"):
        assert sum(int(np.isnan(v).sum()) for v in dn.values()) >= 4, name
    for form in ("shifted", "plain"):
        a, b = T.reference_tangent(qp, pt, d, form), T.reference_tangent(qp, pt, dn, form)
        for k in T.OUTS:
            assert np.array_equal(a[k], b[k]), (form, k)
    m = T.moved(qp, dn, 1e-3)
    for k in T.NAMES:
        assert not np.any(np.isnan(getattr(m, k))), k


def test_every_direction_reaches_every_output():
    """For every direction block and every output block some fixture of the GPU set has that block's
    contribution alone >= 1e-2 of the output's largest entry (all seven given): a dropped block or term cannot
    hide under the cap of 1e-4.  (Measured: the smallest best ratio is 1.1e-1, c -> cons.)"""
    best = {(k, o): 0.0 for k in T.NAMES for o in T.OUTS}
    for name, make in GPU_FIXTURES.items():
        qp, d, _, pt = solved(make)
        full = T.reference_tangent(qp, pt, d)
        for k in T.NAMES:
            if d[k].size == 0:
                continue
            t = T.reference_tangent(qp, pt, T.only(d, k))
            for o in T.OUTS:
                if np.any(full[o]):
                    best[(k, o)] = max(best[(k, o)], float(np.max(np.abs(t[o])) / np.max(np.abs(full[o]))))
    print({f"{k}->{o}": f"{v:.1e}" for (k, o), v in best.items()})
    assert min(best.values()) >= 1e-2, {k: v for k, v in best.items() if v < 1e-2}


def test_conventions_of_the_fixed_and_the_equality():
    """A fixed variable moves with dlvar one to one, its multipliers stay 0; an equality row's value moves with
    dlcon one to one."""
    qp, d, _, pt = solved(GPU_FIXTURES["family_seed3"])
    fixed, eq = qp.lvar == qp.uvar, qp.lcon == qp.ucon
    assert fixed.any() and eq.any()
    t = T.reference_tangent(qp, pt, d)
    assert np.array_equal(t["x"][fixed], d["lvar"][fixed])
    assert not np.any(t["zl"][fixed]) and not np.any(t["zu"][fixed])
    only = T.reference_tangent(qp, pt, T.only(d, "lcon"))
    assert np.max(np.abs(only["cons"][eq] - d["lcon"][eq])) <= 1e-12


def test_first_order_prediction():
    """x* + t dx predicts the optimum of the moved problem to second order for steps of 1e-4 and 1e-5 with
    directions around 1 (measured: 2.2e-7 and 2.2e-9 against movements of 9.7e-4 and 9.7e-5; at 1e-3 the
    prediction is already off by a third of the movement on this fixture): the error falls by 100 when t falls
    by 10 (within a factor 3), and is far below the zeroth-order error."""
    qp, d, _, pt = solved(GPU_FIXTURES["family_min"])
    t = T.reference_tangent(qp, pt, d)
    e = []
    for step in (1e-4, 1e-5):
        new = O.reference_ipm(T.moved(qp, d, step))
        e.append((np.max(np.abs(new["x"] - pt["x"] - step * t["x"])), np.max(np.abs(new["x"] - pt["x"]))))
    print(e)
    assert e[0][0] <= 1e-2 * e[0][1] and e[1][0] <= 1e-3 * e[1][1]
    assert e[1][0] <= e[0][0] / 30.0


# ------------------------------------------------------------------ the argument checks (no library call behind them)
def test_want_and_direction_checks():
    from madipm_amd import solver as S
    assert S.TANGENT_NAMES == ("x", "y", "zl", "zu", "cons")
    assert S.check_tangent_want(None) == S.TANGENT_NAMES
    assert S.check_tangent_want(["cons", "x"]) == ("x", "cons")
    with pytest.raises(TypeError, match="not the string"):
        S.check_tangent_want("x")
    with pytest.raises(ValueError, match="unknown name"):
        S.check_tangent_want(["x", "s"])
    with pytest.raises(ValueError, match="want is empty"):
        S.check_tangent_want([])
    qp, d, _, _ = solved(GPU_FIXTURES["family_min"])
    size = T.sizes(qp)
    got = S.check_tangent_directions(size, {"uvar": d["uvar"], "c": list(d["c"])})
    assert list(got) == ["c", "uvar"] and got["c"].dtype == np.float64 and got["c"].flags.c_contiguous
    with pytest.raises(ValueError, match="no direction given"):
        S.check_tangent_directions(size, {})
    with pytest.raises(ValueError, match=r"Avals has shape \(3,\)"):
        S.check_tangent_directions(size, {"Avals": np.ones(3)})
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="float64"):
        S.check_tangent_directions(size, {"c": torch.ones(qp.nvar, dtype=torch.float32)}, on_device=True,
                                   who="tangent_device")
    with pytest.raises(TypeError, match="expected a GPU tensor"):
        S.check_tangent_directions(size, {"c": torch.ones(qp.nvar, dtype=torch.float64)}, on_device=True,
                                   who="tangent_device")
    with pytest.raises(TypeError, match="torch tensor"):
        S.check_tangent_directions(size, {"c": d["c"]}, on_device=True, who="tangent_device")


def test_jvp_of_the_layer_with_a_stand_in_solver():
    """QPFunction.jvp hands tangent_device exactly the tangents autograd has, asks for the layer's outputs and
    returns them in the layer's order; a data tensor without a tangent is absent (the multi-output layer) or
    zeros (the default layer, whose forward materialises them)."""
    torch = pytest.importorskip("torch")
    import torch.autograd.forward_ad as fw
    from madipm_amd import QPLayer
    from madipm_amd import solver as S
    n = {"x": 3, "y": 2, "zl": 3, "zu": 3, "cons": 2}
    key = {"x": "solution", "y": "multipliers", "zl": "multipliers_L", "zu": "multipliers_U", "cons": "constraints"}

    class Stats:
        status = S.SOLVE_SUCCEEDED

    class StandIn:
        calls = []

        def update_device(self, **kw):
            self.data = kw

        def solve(self, fetch_solution=False):
            return Stats

        def solution_device(self):
            return {key[k]: torch.full((n[k],), 1.0 + i, dtype=torch.float64) for i, k in enumerate(n)}

        def tangent_device(self, want=None, **d):
            self.calls.append((tuple(want), d))
            return {k: torch.full((n[k],), 10.0 + i, dtype=torch.float64) for i, k in enumerate(n) if k in want}

    s = StandIn()
    c, lvar, uvar = (torch.arange(3, dtype=torch.float64) + k for k in range(3))
    dc, dl = torch.ones(3, dtype=torch.float64), torch.full((6,), 2.0, dtype=torch.float64)[::2]
    with fw.dual_level():
        out = QPLayer(s, outputs=("cons", "x", "y"))(c=fw.make_dual(c, dc), lvar=fw.make_dual(lvar, dl), uvar=uvar)
        want, d = s.calls[-1]
        assert want == ("cons", "x", "y") and sorted(d) == ["c", "lvar"]
        assert torch.equal(d["c"], dc) and torch.equal(d["lvar"], dl) and d["lvar"].is_contiguous()
        for o, k in zip(out, ("cons", "x", "y")):
            p, t = fw.unpack_dual(o)
            assert torch.equal(p, s.solution_device()[key[k]]) and float(t[0]) == 10.0 + list(n).index(k)
        x = QPLayer(s)(c=fw.make_dual(c, dc), uvar=uvar)
        want, d = s.calls[-1]
        assert want == ("x",) and isinstance(x, torch.Tensor) and float(fw.unpack_dual(x).tangent[0]) == 10.0
        assert torch.equal(d["c"], dc) and not torch.any(d.get("uvar", torch.zeros(1)))
        k = len(s.calls)
        y = QPLayer(s, outputs=("y", "x"))(c=c)          # no tangent anywhere: jvp is not asked, or returns none
        assert len(s.calls) == k and all(fw.unpack_dual(o).tangent is None for o in y)
