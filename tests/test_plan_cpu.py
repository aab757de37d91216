"""The LDL^T launch planner on the host (csrc/ldl_plan.cpp through build/plan_check, no GPU).

plan_check runs symbolic_analyze + read_ldl_knobs + build_launch_plan on a pattern, checks the plan's
invariants (DAG dependencies earlier, sorted and distinct; launch lists inside sched; every front
factorised and solved exactly once; ticket orders of the tree kernels; upos inside the parent's gather
range and distinct; sv_nt within the row; LDS-source tiles and chunk ids) and prints one FNV-1a digest
per LaunchPlan array.  Here, per pattern and setting: it exits 0, its digests do not depend on
MADIPM_ANALYSIS_THREADS, and MADIPM_BIG_DAG=0 changes only the launch lists.
"""
import os
import subprocess

import pytest

from helpers import (ASSEMBLY_TREES, FRONT_TREE_OPTS, assembly_tree, block_angular_k2, dense_k2, front_tree_k2,
                     leaf_shape_tree, lp_k2, many_leaf_k2)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_CHECK = os.path.join(ROOT, "build", "plan_check")

K2_OPTS = dict(ordering=1, relax=1)


def _ex10():
    from madipm_amd import standard_form_qp
    from madipm_amd.instances import ex10_standin
    return lp_k2(standard_form_qp(ex10_standin(scale=0.05)), 0, well=True)


PATTERNS = {f"asm_{name}": (lambda name=name: front_tree_k2(assembly_tree(name), sorted(ASSEMBLY_TREES).index(name))[:2],
                            FRONT_TREE_OPTS) for name in sorted(ASSEMBLY_TREES)}
PATTERNS.update({f"leaf_{r}_{w}": (lambda r=r, w=w: front_tree_k2(leaf_shape_tree(r, w), 1000 * r + w)[:2], FRONT_TREE_OPTS)
                 for r in (33, 129, 193, 257) for w in (16, r - 1)})
PATTERNS.update({"dense_k2": (lambda: dense_k2(100, 800, 3), K2_OPTS),
                 "many_leaf_k2": (lambda: many_leaf_k2(1500), K2_OPTS),
                 "block_angular_k2": (lambda: block_angular_k2(1200, 2400, 24, 3, well=True), K2_OPTS),
                 "ex10_k2": (_ex10, K2_OPTS)})

# (environment, nshards): the defaults, every A/B switch of the planner, a forced window count, 2 shards
SETTINGS = {"default": ({}, 1), "big_dag0": ({"MADIPM_BIG_DAG": "0"}, 1), "big_kpan1": ({"MADIPM_BIG_KPAN": "1"}, 1),
            "tree_solve0": ({"MADIPM_TREE_SOLVE": "0"}, 1), "fold_help0": ({"MADIPM_FOLD_HELP": "0"}, 1),
            "asm_lds_win12": ({"MADIPM_ASM_LDS_WIN": "12"}, 1), "shards2": ({}, 2)}


def _write(path, Lw, opts, nshards, shard):
    with open(path, "w") as f:
        f.write(f"{Lw.shape[0]} {Lw.nnz}\n")
        f.write(" ".join(map(str, Lw.indptr.tolist())) + "\n")
        f.write(" ".join(map(str, Lw.indices.tolist())) + "\n")
        f.write(f"{opts['ordering']} {opts['relax']} 128 {nshards} {shard}\n")


def _run(path, env, threads):
    e = {k: v for k, v in os.environ.items() if not k.startswith("MADIPM_")}
    e.update(env, MADIPM_ANALYSIS_THREADS=str(threads))
    p = subprocess.run([PLAN_CHECK, path], env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (path, env, p.stderr[-2000:])
    lines = [ln.split() for ln in p.stdout.splitlines()]
    return {(c, n): (cnt, h) for c, n, cnt, h in (ln for ln in lines if ln[0] != "info")}


@pytest.mark.parametrize("name", list(PATTERNS))
def test_launch_plan_invariants_and_digests(name, tmp_path):
    assert os.path.exists(PLAN_CHECK), "build/plan_check is built by `make -C madipm.jl_amd/csrc` (build())"
    make, opts = PATTERNS[name]
    _, Lw = make()
    extra = {"MADIPM_BIG_MERGE": "0"} if opts is FRONT_TREE_OPTS else {}   # prescribed fronts: no cost-based merging
    digests = {}
    for sname, (env, nshards) in SETTINGS.items():
        env = dict(env, **extra)
        for shard in range(nshards):
            path = str(tmp_path / f"{sname}_{shard}.txt")
            _write(path, Lw, opts, nshards, shard)
            d1 = _run(path, env, 1)
            d8 = _run(path, env, 8)
            assert d1 == d8, (sname, shard, {k: (d1[k], d8[k]) for k in d1 if d1[k] != d8[k]})
            digests[sname, shard] = d1
    base, nodag = digests["default", 0], digests["big_dag0", 0]
    differ = {k for k in base if base[k] != nodag[k]}
    assert all(k[0] == "launch" for k in differ), differ
    # a plan with k_big_dag launches has DAG tasks; without them the launch lists must change
    if int(base["launch", "dag_tasks"][0]) > 0:
        assert ("launch", "fact1") in differ and int(nodag["launch", "dag_tasks"][0]) == 0, differ
    else:
        assert not differ, differ
