"""The MPC loop's reductions past one finaliser workgroup and past the block cap: iterates element by
element against the oracle, with test_mpc_point_gpu.py's comparison (_check_iterate: the five returned
vectors in max-norm and objective, dual_objective, inf_pr, inf_du, inf_compl, mu against the oracle at the
same max_iter = k with FixedRegularization(1e-4, -1e-4), within max(1e-9, 30 s), s the oracle's own
SuperLU-vs-LDL^T spread, <= 3e-9 required) on the sized separable family helpers.regime_problem.

Every scalar the loop steers by is a multi-block reduction of csrc/mpc.hip (block_partials is in
csrc/mpc_kernels.hpp): producers write one partial per block, k_final combines them.  Up to FT1 = 1024
partial blocks one workgroup combines them; past that, FG workgroups, level-2 partials and a ticket.
Producers launch at most MAXB = 2048 blocks and stride past that.  The constants are helpers.MPC_CONSTANTS, pinned on the sources by test_regime_helpers_cpu.py, which
also pins the family's row counts, its planted extremes and every case's oracle spread on the CPU.  Every
test first asserts (assert_regime) that its launches lie on the side of 1024 and 2048 it is named for.

  * test_spmv_regimes_g64   MADIPM_SPMV_G=64 (4 rows per block): n_ + m_ = 4096 (1024 blocks: the last
                            one-workgroup case), 4097, 8192 (2048 blocks, no stride), 8193, 20001 (2.4
                            trips) for k_residual with its fused step-test blocks, k_eval and the
                            normal-equation kernels, while the flat kernels stay below 80 blocks: the
                            mixed counts of FIN_RESID (nb against nb_alpha) and FIN_TERM (nb against
                            nb_eval).  LP under K2, K2.5, normal; QP under K2, K2.5; MehrotraAdaptiveStep
                            and max_ncorr = 3 at 4097 and 8193; iterates 0, 1, 3.
  * test_g16_same_numbers   the 8193-row K2 case at G = 16 (513 blocks, no boundary) against the same
                            oracle numbers: the comparison is about the problem, not about G.
  * test_reused_solver_repeats_bitwise
                            two solves on one 8193-row solver, update() with the same data and a second,
                            4096-row solver in between: bit-identical (the ticket's reset).
  * test_flat_regimes       the heuristic's own G (4) on 262144, 262145 and 524588 rows: the flat kernels
                            (k_rhs, k_term, k_apply, k_zinit, ...) at 1024, 1025 and 2048 strided blocks,
                            the step test at 1299 blocks on the last.  LP, K2, k = 2 (and 0 on the last).
                            Wall time of the GPU side of one iterate on the MI355X (solver construction
                            with the default ordering, solve, comparison; printed as flat_wall):
                                262144 rows  k = 2      0.06 s   (the test with its two oracle solves 0.6 s)
                                262145 rows  k = 2      0.07 s   (0.6 s)
                                524588 rows  k = 0, 2   0.13 s, 0.14 s   (1.7 s)
                            Symbolic analysis does not dominate: constructing the solver took 0.08 s
                            (262145 rows) and 0.12 s (524588) with the default ordering and 0.30 s / 0.12 s
                            with ordering=0, at the same fill (nnz(L) 444290 / 889176), so the default stays.

Largest GPU-vs-oracle difference per field on the MI355X, relative to max(1, |ref|_inf), over all cases and
k of a group (the tolerance was 1e-9 in every case; every test prints its own):

    field            G = 64 sizes   flat sizes
    solution           9.0e-15        1.5e-15
    multipliers        1.0e-14        9.1e-16
    multipliers_L      8.6e-15        1.3e-15
    multipliers_U      2.1e-15        6.0e-16
    constraints        3.0e-15        9.4e-16
    objective          1.3e-14        2.7e-15
    dual_objective     9.4e-15        7.8e-16
    inf_pr             1.7e-15        2.8e-16
    inf_du             5.5e-15        1.4e-16
    inf_compl          1.7e-14        8.9e-16
    mu                 4.2e-15        7.2e-16
"""
import time

import pytest

from helpers import (REGIME_FLAT_SIZES, REGIME_G, REGIME_G64_SIZES, REGIME_KS, regime_bounds, regime_flat_cases,
                     regime_g64_boundary, regime_g64_cases, regime_launches, regime_name, spmv_mean_row)
from test_mpc_point_gpu import SCALARS, VECTORS, _check_iterate, _kkt, _oracle_iterate, _problem, _reg
from test_update_gpu import VALUE_FIELDS, assert_same

pytestmark = pytest.mark.gpu

SEEN = {"g64": {}, "flat": {}}      # the largest difference per field and group (printed by every test)


def _size(problem):
    _, m, n_ineq = problem.split(":")[:3]
    return int(m), int(n_ineq)


def assert_regime(qp, G, spmv=None, flat=None, step=None):
    """The launches of this problem at lane-group width G are in the named regimes ((finaliser,
    strided) per kernel family, helpers.regime_launches): a case that no longer reaches its path fails."""
    got = regime_launches(qp, G)
    for fam, want in (("spmv", spmv), ("flat", flat), ("step", step)):
        if want is not None:
            assert got[fam][1:] == tuple(want), (fam, got[fam], want, regime_bounds(qp), G)
    return got


def _report(group):
    print(f"largest differences so far ({group}): " + " ".join(f"{f}={SEEN[group].get(f, 0.0):.1e}" for f in VECTORS + SCALARS))


@pytest.mark.parametrize("problem,kkt,variant", regime_g64_cases())
def test_spmv_regimes_g64(problem, kkt, variant, monkeypatch):
    """The SpMV-shaped kernels on each side of 1024 and 2048 blocks, the flat ones far below."""
    monkeypatch.setenv("MADIPM_SPMV_G", str(REGIME_G))
    qp = _problem(problem)
    rows, fin, strided = REGIME_G64_SIZES[_size(problem)]
    assert regime_bounds(qp)[0] == rows
    # SpMV-shaped kernels on their side of 1024 and 2048 blocks; the flat ones and the step test far below
    got = assert_regime(qp, REGIME_G, spmv=(fin, strided), flat=("one", False), step=("one", False))
    assert got["flat"][0] < 100 and got["step"][0] < 100
    for k in REGIME_KS:
        s = _check_iterate(qp, problem, kkt, variant, k, label=f" {got['spmv']}", seen=SEEN["g64"])
        assert s.spmv_group() == REGIME_G
    _report("g64")


def test_g16_same_numbers(monkeypatch):
    """The 8193-row K2 LP at G = 16: 513 SpMV blocks, one finaliser workgroup, no stride; the same
    oracle numbers as at G = 64 (the oracle's cache key has no G)."""
    monkeypatch.setenv("MADIPM_SPMV_G", "16")
    problem = regime_name(2600, 393, False, "boundary", regime_g64_boundary(8193))
    qp = _problem(problem)
    got = assert_regime(qp, 16, spmv=("one", False), flat=("one", False), step=("one", False))
    assert got["spmv"][0] == 513
    for k in REGIME_KS:
        s = _check_iterate(qp, problem, "K2", "default", k, label=f" {got['spmv']}", seen=SEEN["g64"])
        assert s.spmv_group() == 16


def test_reused_solver_repeats_bitwise(monkeypatch):
    """k_final's ticket is reset by the last workgroup of every two-level launch: a missed reset shows
    in the NEXT launch.  One 8193-row solver (two-level, strided) solves, is updated with unchanged data
    while a 4096-row solver (one workgroup) is created and solves in the same process, and solves again:
    the second result equals the first bit for bit, vectors, scalars and the whole trace."""
    from madipm_amd import MAXIMUM_ITERATIONS_EXCEEDED, MPCSolver
    monkeypatch.setenv("MADIPM_SPMV_G", str(REGIME_G))
    qp = _problem(regime_name(2600, 393, False, "boundary", regime_g64_boundary(8193)))
    small = _problem(regime_name(1300, 196, False, "first", regime_g64_boundary(4096)))
    assert_regime(qp, REGIME_G, spmv=("two", True))
    assert_regime(small, REGIME_G, spmv=("one", False))
    kw = dict(regularization=_reg(1e-4), kkt_system=_kkt("K2"), max_iter=3)
    s = MPCSolver(qp, **kw)
    assert s.spmv_group() == REGIME_G
    first = s.solve()
    assert first.status == MAXIMUM_ITERATIONS_EXCEEDED and first.iter == 3      # a solve, not the same failure twice
    other = MPCSolver(small, **kw)
    o1 = other.solve()
    assert o1.status == MAXIMUM_ITERATIONS_EXCEEDED and o1.iter == 3
    s.update(**{k: getattr(qp, k) for k in VALUE_FIELDS})
    second = s.solve()
    assert_same(second, first)
    assert s.counters()["n_updates"] == 1
    assert_same(other.solve(), o1)
    assert_same(s.solve(), first)


@pytest.mark.parametrize("problem,ks", regime_flat_cases())
def test_flat_regimes(problem, ks, monkeypatch):
    """The flat kernels across both boundaries at the heuristic's own lane-group width."""
    monkeypatch.delenv("MADIPM_SPMV_G", raising=False)
    qp = _problem(problem)
    rows, fin, strided = REGIME_FLAT_SIZES[_size(problem)][:3]
    G = spmv_mean_row(qp)[1]
    assert regime_bounds(qp)[0] == rows and G == 4
    got = assert_regime(qp, G, flat=(fin, strided), spmv=("two", True),
                        step=("two", False) if rows > 500000 else ("one", False))
    assert got["flat"][0] == {262144: 1024, 262145: 1025, 524588: 2048}[rows]
    for k in ks:
        _oracle_iterate(problem, "K2", "default", k)      # cached: the time below is the GPU side's
        t0 = time.perf_counter()
        s = _check_iterate(qp, problem, "K2", "default", k, label=f" {got}", seen=SEEN["flat"])
        print(f"flat_wall rows={rows} k={k}: {time.perf_counter() - t0:.2f} s")
        assert s.spmv_group() == G
    _report("flat")
