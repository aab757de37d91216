"""GPU tests of the step-length rules (update_step!, src/kernels.jl:291-358) through the C-ABI
`madipm_update_step`, which runs the MPC loop's own step-test kernels (k_alpha + k_final, and k_mu +
k_final for MehrotraAdaptiveStep), against the oracle's restatement (oracle/mpc.py step_on_vectors).

The reference's max-ratio test is `mapreduce(f, (e1, e2) -> e1[1] < e2[1] ? e1 : e2, ...; init =
(1.0, 0))` (kernels.jl:226-272), a left fold: among EXACTLY equal ratios the LAST index wins, and an
element whose ratio is exactly 1.0 replaces the init element.  Only MehrotraAdaptiveStep reads the
index (kernels.jl:335-352), so the tied entries below carry different multipliers: the first-index
rule would give a different step, which the test checks too (it discriminates).
Tolerance: indices exact; alphas 1e-12 relative (the Mehrotra mu_full sum is reduced in a different
order on the GPU).

The tests down to test_empty_sides use 3000 bounded coordinates: 12 partial blocks, k_final's
one-workgroup instance, no strided loop.  test_step_regimes and its two companions repeat them at
max(nlb, nub) = 262144 (1024 blocks: the last one-workgroup case), 262145, 524288 (2048 blocks, no
stride), 524289 and 1310797 (2.5 trips of the capped grid), with ties across the finaliser's workgroups,
across blocks 1023 | 1024, across one thread's two trips and around the first trip's end
(helpers.regime_step_ties), full and with one side of 3 elements.  The mu_full sum then has up to 2.6 M
terms; test_regime_helpers_cpu.py shows that three float64 summation orders of the oracle's terms for
exactly these inputs agree within 1e-13, so the 1e-12 bound stands.  The MPC loop's own reductions at
these sizes: test_mpc_regimes_gpu.py.  On the MI355X every index was exact and every alpha of every
regime case equal to the oracle's bit for bit (each case prints its largest difference).
"""
import numpy as np
import pytest

from helpers import REGIME_STEP_SIZES, mpc_regime, regime_step_ties
from oracle.mpc import step_on_vectors

pytestmark = pytest.mark.gpu


def _vectors(seed, nlb=3000, nub=2500, tie_l=(5, 700, 2999), tie_lz=(11, 1500, 2998), tie_u=(17, 300, 2400),
             tie_uz=(40, 1000, 2499), ratio=0.5, lo=0.8):
    """Random interior point + direction whose smallest ratios are EXACT ties (the tied entries have
    bit-identical operands, so every tau gives identical quotients) at the given indices:
    primal ties (tie_l / tie_u) carry distinct multipliers, dual ties (tie_lz / tie_uz) distinct
    primal values — the quantities MehrotraAdaptiveStep reads at the chosen index.  The other entries'
    ratios are >= lo (primal) and >= 1.25 (dual)."""
    rng = np.random.default_rng(seed)
    xl = rng.uniform(-1, 1, nlb)
    x_l = xl + rng.uniform(lo, lo + 1.2, nlb)
    dx_l = rng.uniform(-1.0, 1.0, nlb)
    zl = rng.uniform(0.5, 2.0, nlb)
    dzl = rng.uniform(-1.0, 1.0, nlb) * 0.4
    xu = rng.uniform(-1, 1, nub)
    x_u = xu - rng.uniform(lo, lo + 1.2, nub)
    dx_u = rng.uniform(-1.0, 1.0, nub)
    zu = rng.uniform(0.5, 2.0, nub)
    dzu = -rng.uniform(0.0, 1.0, nub) * 0.4          # zu + dzu > 0: no upper dual candidate
    for k, i in enumerate(tie_l):
        xl[i], x_l[i], dx_l[i] = 0.0, ratio, -1.0     # (-x + xl) tau / dx = ratio tau
        zl[i] = 1.0 + 0.25 * k
    for i in tie_lz:
        zl[i], dzl[i] = 1.0, -2.0                     # -zl tau / dzl = tau / 2
    for k, i in enumerate(tie_u):
        xu[i], x_u[i], dx_u[i] = 0.0, -ratio, 1.0
        zu[i] = 1.5 + 0.25 * k
    for i in tie_uz:
        zu[i], dzu[i] = 1.0, -2.0                     # zu + dzu < 0 holds
    return [x_l, xl, zl, dx_l, dzl, x_u, xu, zu, dx_u, dzu]


def _gpu(rule, tau, mu, vecs):
    import torch
    from madipm_amd.rocm_wrapper import update_step
    dv = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in vecs]
    return update_step(rule, tau, mu, *dv)


def _close(a, b, rtol=1e-12):
    return abs(a - b) <= rtol * max(1.0, abs(b))


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("rule,tau,mu", [("conservative", 0.995, 0.0), ("adaptive", 0.99, 1e-3),
                                         ("mehrotra", 0.99, 0.0)])
def test_step_rule_ties_match_oracle(seed, rule, tau, mu):
    vecs = _vectors(seed)
    got = _gpu(rule, tau, mu, vecs)
    ref = step_on_vectors((rule, tau), mu, *vecs)
    for k in ("i_xl", "i_xu", "i_zl", "i_zu"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    # the left fold keeps the LAST of the tied indices
    assert (ref["i_xl"], ref["i_xu"], ref["i_zl"], ref["i_zu"]) == (2999, 2400, 2998, 2499)
    for k in ("alpha_p", "alpha_d", "alpha_xl", "alpha_xu", "alpha_zl", "alpha_zu"):
        assert _close(got[k], ref[k]), (k, got[k], ref[k])


def test_mehrotra_tie_choice_changes_the_step():
    """The tie-break is observable: with the first tied index instead, MehrotraAdaptiveStep's alpha_p
    and alpha_d differ from the reference's (and from the GPU's)."""
    vecs = _vectors(3)
    got = _gpu("mehrotra", 0.99, 0.0, vecs)
    ref = step_on_vectors(("mehrotra", 0.99), 0.0, *vecs)
    assert _close(got["alpha_p"], ref["alpha_p"]) and _close(got["alpha_d"], ref["alpha_d"])
    # first-index variant: move the first tie's entry to the end (then it is the last one)
    first = _vectors(3, tie_l=(5,), tie_lz=(11,), tie_u=(17,), tie_uz=(40,))
    alt = step_on_vectors(("mehrotra", 0.99), 0.0, *first)
    assert not _close(alt["alpha_p"], ref["alpha_p"], 1e-9) or not _close(alt["alpha_d"], ref["alpha_d"], 1e-9)


def test_ratio_exactly_one_replaces_init():
    """A ratio of exactly 1.0 is not strictly larger than init (1.0, 0): the element's index is kept;
    ratios above 1 keep the init element (index -1, alpha 1)."""
    vecs = _vectors(4, ratio=1.0, lo=1.5)
    got = _gpu("conservative", 1.0, 0.0, vecs)
    ref = step_on_vectors(("conservative", 1.0), 0.0, *vecs)
    assert got["alpha_xl"] == ref["alpha_xl"] == 1.0
    assert got["i_xl"] == ref["i_xl"] == 2999
    # no candidate at all below or at 1: the init element
    vecs = _vectors(5, ratio=2.0, lo=1.5)
    got = _gpu("conservative", 1.0, 0.0, vecs)
    ref = step_on_vectors(("conservative", 1.0), 0.0, *vecs)
    assert (got["i_xl"], got["alpha_xl"]) == (ref["i_xl"], ref["alpha_xl"]) == (-1, 1.0)


def test_empty_sides():
    """nub = 0 (only lower bounds) and nlb = 0: the empty side is the init element."""
    v = _vectors(6)
    for keep in ("lb", "ub"):
        vecs = [a if (k < 5) == (keep == "lb") else a[:0] for k, a in enumerate(v)]
        got = _gpu("mehrotra", 0.99, 0.0, vecs)
        ref = step_on_vectors(("mehrotra", 0.99), 0.0, *vecs)
        for k in ("i_xl", "i_xu", "i_zl", "i_zu"):
            assert got[k] == ref[k]
        assert _close(got["alpha_p"], ref["alpha_p"]) and _close(got["alpha_d"], ref["alpha_d"])


# ------------------------------------------------------------------ past one finaliser workgroup, past the cap
RULES = [("conservative", 0.995, 0.0), ("adaptive", 0.99, 1e-3), ("mehrotra", 0.99, 0.0)]
SIDES = ("full", "tiny_ub", "tiny_lb")


def _unclamped(vecs, tie_l, tie_lz):
    """MehrotraAdaptiveStep's alphas are max(candidate, gamma_f alpha_max), and with _vectors' multipliers
    of ~1 the clamp wins whatever index was chosen.  Multipliers of 8, 16 on the primal tie and primal
    gaps of 8, 16 (dx = 0: no primal candidate) on the dual tie put both candidates above the clamp, at
    values that differ by ~1e-3 between the first and the last tied index."""
    x_l, xl, zl, dx_l = vecs[0], vecs[1], vecs[2], vecs[3]
    for k, i in enumerate(tie_l):
        zl[i] = 8.0 * (k + 1)
    for k, i in enumerate(tie_lz):
        x_l[i], dx_l[i] = xl[i] + 8.0 * (k + 1), 0.0
    return vecs


def regime_step_vectors(n, side, rot, ratio=0.5, lo=0.8):
    """_vectors at max(nlb, nub) = n: 'full' has nub = n - 777, 'tiny_ub' nub = 3, 'tiny_lb' nlb = 3 (most
    blocks then hold only the init element on that side).  The four reductions (primal / dual, lower /
    upper) each carry one tied pair of regime_step_ties(n), the assignment rotated by 2 rot; a pair that
    does not fit a side is replaced by that side's first and last element (primal) or second and last but
    one (dual; a side of 3 has the single candidate 1).
    The lower ties are _unclamped, so MehrotraAdaptiveStep's alphas depend on the chosen indices and on the
    mu_full sum.  Returns (vectors, (nlb, nub), the last index of each tie in the order i_xl, i_xu, i_zl, i_zu, the
    ties in the order lower primal, upper primal, lower dual, upper dual)."""
    nlb, nub = {"full": (n, n - 777), "tiny_ub": (n, 3), "tiny_lb": (3, n)}[side]
    ties = regime_step_ties(n)
    order = ties[2 * rot % len(ties):] + ties[:2 * rot % len(ties)]   # rot = 0, 1, 2 reach all of <= 6 pairs
    pick = [order[0], order[1 % len(order)]]             # primal lower, primal upper; the dual ones: the next
    pick += [next(p for p in order[2:] + order[:2] if not set(p) & set(q)) for q in pick]   # disjoint pairs
    spare = [(0, -1), (0, -1), (1, -2), (1, -2)]         # primal and dual ties of a side share no index:
    fit = [p if max(p) < size else (a, max(a, size + b))  # an index tied in both has a zero denominator
           for p, size, (a, b) in zip(pick, (nlb, nub, nlb, nub), spare)]
    assert not set(fit[0]) & set(fit[2]) and not set(fit[1]) & set(fit[3]), fit
    vecs = _vectors(n % 1000 + rot, nlb=nlb, nub=nub, tie_l=fit[0], tie_u=fit[1], tie_lz=fit[2], tie_uz=fit[3],
                    ratio=ratio, lo=lo)
    return _unclamped(vecs, fit[0], fit[2]), (nlb, nub), tuple(max(p) for p in fit), fit


def assert_step_regime(n, nlb, nub):
    """The step test's launch at this size is in the regime the size is listed for."""
    assert max(nlb, nub) == n and mpc_regime(n) == REGIME_STEP_SIZES[n], (n, mpc_regime(n))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("n", sorted(REGIME_STEP_SIZES))
def test_step_regimes(n, side):
    """test_step_rule_ties_match_oracle across the regimes: every rule, the tied pairs rotated over the
    four reductions by the rule's number, indices exact (the last of each tie), alphas to 1e-12."""
    worst = 0.0
    for rot, (rule, tau, mu) in enumerate(RULES):
        vecs, (nlb, nub), last, _ = regime_step_vectors(n, side, rot)
        assert_step_regime(n, nlb, nub)
        got = _gpu(rule, tau, mu, vecs)
        ref = step_on_vectors((rule, tau), mu, *vecs)
        for k in ("i_xl", "i_xu", "i_zl", "i_zu"):
            assert got[k] == ref[k], (rule, k, got[k], ref[k])
        assert (ref["i_xl"], ref["i_xu"], ref["i_zl"], ref["i_zu"]) == last
        for k in ("alpha_p", "alpha_d", "alpha_xl", "alpha_xu", "alpha_zl", "alpha_zu"):
            worst = max(worst, abs(got[k] - ref[k]) / max(1.0, abs(ref[k])))
            assert _close(got[k], ref[k]), (rule, k, got[k], ref[k])
    print(f"step regimes n={n} {side} {mpc_regime(n)}: largest alpha difference {worst:.1e}")


def test_step_regime_tie_choice_changes_the_step():
    """test_mehrotra_tie_choice_changes_the_step at 524289 (two-level finaliser, strided): the tie-break
    is observable there too, in alpha_p and in alpha_d (neither is clamped, _unclamped)."""
    n = 524289
    vecs, (nlb, nub), last, fit = regime_step_vectors(n, "full", 0)
    assert_step_regime(n, nlb, nub)
    got = _gpu("mehrotra", 0.99, 0.0, vecs)
    ref = step_on_vectors(("mehrotra", 0.99), 0.0, *vecs)
    assert (got["i_xl"], got["i_xu"], got["i_zl"], got["i_zu"]) == last
    assert _close(got["alpha_p"], ref["alpha_p"]) and _close(got["alpha_d"], ref["alpha_d"])
    assert ref["alpha_p"] > 0.99 * ref["alpha_xl"] and ref["alpha_d"] > 0.99 * ref["alpha_zl"]      # unclamped
    # first-index variant: only the first entry of each tie (then it is the chosen one)
    first = _vectors(n % 1000, nlb=nlb, nub=nub, tie_l=fit[0][:1], tie_u=fit[1][:1], tie_lz=fit[2][:1], tie_uz=fit[3][:1])
    alt = step_on_vectors(("mehrotra", 0.99), 0.0, *_unclamped(first, fit[0][:1], fit[2][:1]))
    assert (alt["i_xl"], alt["i_zl"]) == (fit[0][0], fit[2][0])
    assert not _close(alt["alpha_p"], ref["alpha_p"], 1e-9) and not _close(alt["alpha_d"], ref["alpha_d"], 1e-9)


def test_step_regime_ratio_exactly_one_and_no_candidate():
    """test_ratio_exactly_one_replaces_init at the largest size: a tie at exactly 1.0 across one thread's
    two trips keeps the later index; without a candidate at or below 1 the init element survives 2048
    blocks and 2.5 trips."""
    n = max(REGIME_STEP_SIZES)
    vecs, (nlb, nub), last, _ = regime_step_vectors(n, "full", 2, ratio=1.0, lo=1.5)
    assert_step_regime(n, nlb, nub)
    got = _gpu("conservative", 1.0, 0.0, vecs)
    ref = step_on_vectors(("conservative", 1.0), 0.0, *vecs)
    assert got["alpha_xl"] == ref["alpha_xl"] == 1.0 and got["alpha_xu"] == ref["alpha_xu"] == 1.0
    assert (got["i_xl"], got["i_xu"]) == (ref["i_xl"], ref["i_xu"]) == last[:2]
    vecs, _, _, _ = regime_step_vectors(n, "full", 2, ratio=2.0, lo=1.5)
    got = _gpu("conservative", 1.0, 0.0, vecs)
    ref = step_on_vectors(("conservative", 1.0), 0.0, *vecs)
    assert (got["i_xl"], got["alpha_xl"]) == (ref["i_xl"], ref["alpha_xl"]) == (-1, 1.0)
    assert (got["i_xu"], got["alpha_xu"]) == (ref["i_xu"], ref["alpha_xu"]) == (-1, 1.0)
