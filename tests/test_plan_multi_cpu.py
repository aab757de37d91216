"""The multi-right-hand-side solve levels of the launch planner (LaunchPlan::mlev) on the host:
build/plan_check, no GPU.

plan_check checks, and exits 1 on the first violation: every front of the plan appears exactly once over all
levels and classes of mlev, in the class its shape asks for (micro: r <= 32 and w <= 2; tiny / small: solve_small,
the small class with its panel and the 8 staged columns inside a workgroup's LDS; big: the rest); every front's
children are at strictly lower levels; the gather / below / task lists of a level cover exactly its big fronts,
each of which has flags and a bpart range.  Here: it exits 0 on a plan with tree fronts and on the same pattern
with MADIPM_TREE_SOLVE=0, the report lists every front once, and the two plans give the same mlev front for
front (the list does not depend on the knob), while the single solve's levels do depend on it.  A sharded plan
has no mlev.
"""
import os

import pytest

from test_plan_cpu import PATTERNS, PLAN_CHECK, _run, _write

# tree fronts of every kind (small, medium, big roots, folded micro leaves), batched-free dense fronts, and leaf
# shapes on both sides of the small / big boundary (r = 193: big by its rows; r = 129, w = 128: small)
NAMES = ["block_angular_k2", "ex10_k2", "dense_k2", "many_leaf_k2", "asm_medium_mids", "asm_big_mixed", "asm_micro_fold",
         "leaf_193_16", "leaf_257_256", "leaf_129_128"]


def _mlev(path, env):
    """{(level, class): [fronts]} and the class totals of plan_check's mlev report."""
    import subprocess
    e = {k: v for k, v in os.environ.items() if not k.startswith("MADIPM_")}
    e.update(env, MADIPM_ANALYSIS_THREADS="1")
    p = subprocess.run([PLAN_CHECK, path], env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (path, env, p.stderr[-2000:])
    fronts, totals = {}, None
    for ln in p.stdout.splitlines():
        f = ln.split()
        if f[:2] == ["info", "mlev_fronts"]:
            fronts[int(f[2]), f[3]] = [int(v) for v in f[4:]]
        elif f[:2] == ["info", "mlev_classes"]:
            totals = {f[i]: int(f[i + 1]) for i in range(2, len(f), 2)}
    return fronts, totals


@pytest.mark.parametrize("name", NAMES)
def test_mlev_invariants_and_knob_independence(name, tmp_path):
    assert os.path.exists(PLAN_CHECK), "build/plan_check is built by `make -C madipm.jl_amd/csrc` (build())"
    make, opts = PATTERNS[name]
    _, Lw = make()
    extra = {"MADIPM_BIG_MERGE": "0"} if name.startswith(("asm_", "leaf_")) else {}
    path = str(tmp_path / "p.txt")
    _write(path, Lw, opts, 1, 0)
    tree, tot = _mlev(path, dict(extra))                              # plan_check's own invariants passed (exit 0)
    level, tot0 = _mlev(path, dict(extra, MADIPM_TREE_SOLVE="0"))
    assert tot is not None and tot == tot0
    allf = sorted(f for v in tree.values() for f in v)
    assert allf == list(range(tot["fronts"])), "every front exactly once"   # (none of these plans has batched leaves)
    assert tot["micro"] + tot["tiny"] + tot["small"] + tot["big"] == len(allf)
    assert tree == level, "mlev depends on MADIPM_TREE_SOLVE"
    d1 = _run(path, dict(extra), 1)
    d0 = _run(path, dict(extra, MADIPM_TREE_SOLVE="0"), 1)
    assert int(d1["launch", "mlev"][0]) == tot["levels"] == int(d0["launch", "mlev"][0])
    if int(d1["tree", "tc_list"][0]) > 0:    # the plan has tree fronts: the single solve's levels lose them
        assert d1["launch", "slev1"] != d0["launch", "slev1"]
    # what the single solve reads keeps its place: mlev's lists only follow it in sched / tasks
    for key in (("solve", "flag_off"), ("solve", "bp_off"), ("solve", "scalars")):
        assert d1[key][0] == d0[key][0]


def test_mlev_reaches_every_class(tmp_path):
    """Between them the patterns put fronts into all four classes, the ex10 stand-in has tree fronts that are
    small in mlev, and leaf_257_256 a front past 192 rows (big)."""
    seen = {}
    for name in ("ex10_k2", "leaf_257_256", "many_leaf_k2"):
        make, opts = PATTERNS[name]
        _, Lw = make()
        path = str(tmp_path / f"{name}.txt")
        _write(path, Lw, opts, 1, 0)
        _, tot = _mlev(path, {"MADIPM_BIG_MERGE": "0"} if name.startswith("leaf_") else {})
        seen[name] = tot
    assert seen["ex10_k2"]["small"] > 0 and seen["ex10_k2"]["micro"] > 0, seen
    assert seen["leaf_257_256"]["big"] > 0, seen
    assert sum(t["tiny"] for t in seen.values()) > 0, seen


def test_sharded_plan_has_no_mlev(tmp_path):
    make, opts = PATTERNS["block_angular_k2"]
    _, Lw = make()
    for shard in range(2):
        path = str(tmp_path / f"s{shard}.txt")
        _write(path, Lw, opts, 2, shard)
        fronts, tot = _mlev(path, {})
        assert fronts == {} and tot["levels"] == 0
        assert int(_run(path, {}, 1)["launch", "mlev"][0]) == 0
