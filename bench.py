#!/usr/bin/env python3
"""Benchmark: MadIPM's Mehrotra predictor-corrector on MI355X (BASELINE.json metric).

metric  : IPM iterations/sec (+ wall-clock-to-optimality), MIPLIB LP
workload: BASELINE.json configs[1] — MIPLIB ex10 LP relaxation, fp64, 1 GPU.  No MPS files exist
          offline, so a seeded structured stand-in with ex10's catalogue shape is used
          (madipm_amd.instances.ex10_standin; 69.6k rows x 17.7k [0,1] columns, ~1.1M nnz), run
          through presolve_qp -> scale_qp -> standard_form_qp exactly as scripts/benchmarks_*.jl do
          (reformulate = true), with the benchmark's solver
          settings: max_iter=300, FixedRegularization(1e-8, -1e-8), AdaptiveStep(0.99), tol 1e-8.
step    : one MPC iteration (factorize + predictor/corrector solves + step), inputs resident in HBM.
          W warmup iterations (untimed solve), then EXACTLY K iterations of a fresh solve after
          initialize! (the MPC loop only, as cnt.total_time in src/solver.jl:181,407).  A solve that
          reaches optimality before K iterations (ex10: 22) is followed by further solves, each from
          an untimed initialize!, until K iterations are timed.
plain   : without --full the run sets up, warms up, times the K steps and prints the line (value,
          ms_per_step, the timed leg's own figures); --dump-outputs DIR writes the point the last
          timed step left (x, y, z_L, z_U, constraint values, summary) as DIR/<name>.npy.
--full  : adds everything else, as below: the solve to optimality with its parity object, the legs
          of the other configs, the CPU baseline and HiGHS (--no-opt, --legs, --no-cpu, --no-highs
          trim it).
legs    : every other BASELINE config gets a leg of the same schema under its own key of the line
          ("supportcase10" configs[3], "dense_qp" configs[2], "neos" configs[4]): iters/s over a timed
          run, the dominant kernel's roofline (HIP events on the launch stream; PMC traffic from the
          newest committed profiles/*_<config>_pmc_traffic.json), the iteration roofline, analysis /
          end-to-end time to optimality and a parity object (the HiGHS optimum of the same stand-in,
          tests/golden/fullsize_highs.json, plus the returned point's KKT measures).  N > 1: the neos
          leg only (subtree-sharded; the dense QP's 12 GB host instance per rank is not replicated).
multi-GPU: (N > 1, launched by torch.distributed.run) ONE solve of the workload with the LDL^T
          subtree-sharded across the N GPUs (SURVEY §8 e): one process per GPU, each owns
          a set of elimination-tree subtrees, the common ancestors ("top" fronts) are factorised
          redundantly after an RCCL all-reduce of their external contributions (+ 2 all-reduces per
          solve); the MPC vector work is replicated.  value = MPC iterations / max-over-ranks time of
          that single solve ("strong" scaling).  --mode replicas runs N independent solves instead
          (value = total iterations / max time, "weak").
"""
from __future__ import annotations

import argparse
import re
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "madipm.jl_amd"))
sys.path.insert(0, ROOT)


def reference_pipeline(qp):
    """scripts/benchmarks_gpu.jl:29-32 (reformulate = true, l.88): presolve_qp -> scale_qp ->
    standard_form_qp."""
    from madipm_amd import presolve_qp, scale_qp, standard_form_qp
    pq, flag = presolve_qp(qp)
    if not flag:
        raise RuntimeError("presolve: problem solved, infeasible or unbounded")
    return standard_form_qp(scale_qp(pq))


def build_problem(config: str, seed: int = 0):
    """BASELINE.json configs as concrete inputs (SURVEY §8 d).  `name@s` scales the stand-in by s.
    MIPLIB configs go through the reference benchmark's preprocessing (reference_pipeline)."""
    from madipm_amd import instances as I
    standard_form_qp = reference_pipeline
    name, _, sc = config.partition("@")
    s = float(sc) if sc else 1.0
    tag = f" scaled x{s}" if sc else ""
    if name == "ex10":       # configs[1] (the bench workload)
        return standard_form_qp(I.ex10_standin(seed=seed, scale=s)), "MIPLIB ex10 LP relaxation (structured stand-in)" + tag
    if name == "supportcase10":  # configs[3]
        return (standard_form_qp(I.supportcase10_standin(seed=seed, scale=s)),
                "MIPLIB supportcase10 LP relaxation (structured stand-in)" + tag)
    if name == "dense_qp":   # configs[2]: already in standard form (equalities + bounds), natural order
        n, m = int(round(50_000 * s)), int(round(10_000 * s))
        return I.dense_qp(n=n, m=m, seed=seed), f"random dense convex QP n={n} m={m}"
    if name == "neos":       # configs[4]
        return (standard_form_qp(I.neos5052403_standin(seed=seed, scale=s)),
                "MIPLIB neos-5052403-cygnet LP relaxation (structured stand-in)" + tag)
    raise ValueError(config)


SOLVER_OPTS = None


def solver_opts():
    from madipm_amd import FixedRegularization, AdaptiveStep
    return dict(max_iter=300, regularization=FixedRegularization(1e-8, -1e-8), step_rule=AdaptiveStep(0.99),
                tol=1e-8)


def host_cpu_info() -> dict:
    """nproc / lscpu of the host the baseline ran on (core count stated)."""
    info = {"nproc": os.cpu_count(), "affinity": len(os.sched_getaffinity(0))}
    try:
        import subprocess
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            k, _, v = line.partition(":")
            if k.strip() in ("Model name", "Socket(s)", "Core(s) per socket", "Thread(s) per core", "CPU max MHz"):
                info[k.strip()] = v.strip()
    except Exception:
        pass
    return info


def baseline_threads() -> int:
    """The host cores this process may use: its affinity set, capped by OMP_NUM_THREADS (16 per GPU
    on the gpurun boxes, whose nproc counts the whole machine)."""
    n = len(os.sched_getaffinity(0))
    env = os.environ.get("OMP_NUM_THREADS")
    if env and env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    return max(1, n)


def cpu_baseline(config: str, perm, max_threads: int, timeout_s: float = 240.0):
    """CPU baseline on this host (SURVEY §8 d): oracle/cpu_baseline.py in a process of its own (no torch,
    no HIP runtime; MKL's Intel OpenMP with idle threads sleeping; pinned to `max_threads` CPUs), the
    oracle's MPC loop with MKL PARDISO to optimality at 1, 2, 4, 8, 16 threads (capped at the host share);
    value = iterations / PARDISO factor+solve time of the fastest thread count.  Returns (ref, record):
    ref = (status, objective, iterations) of the CPU solve for the parity check."""
    import subprocess
    import tempfile
    import numpy as np
    with tempfile.TemporaryDirectory() as td:
        pf = os.path.join(td, "perm.npy")
        np.save(pf, np.asarray(perm, np.int32))
        env = {k: v for k, v in os.environ.items() if not k.startswith(("OMP_", "MKL_", "KMP_", "GOMP_"))}
        env["PYTHONPATH"] = ROOT
        cmd = [sys.executable, "-m", "oracle.cpu_baseline", "--config", config, "--perm", pf,
               "--max-threads", str(max_threads), "--threads", "1,2,4,8,16"]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout_s)
    if r.returncode != 0:
        raise RuntimeError(f"cpu_baseline exited {r.returncode}: {r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    rec["host"] = host_cpu_info()
    return (rec.pop("ref_status"), rec.pop("ref_objective"), rec.pop("ref_iter")), rec


def highs_baseline(qp, time_limit: float = 120.0):
    """Third-party CPU datapoint: HiGHS 1.x interior point (scipy.optimize.linprog 'highs-ipm', presolve
    off, crossover as scipy runs it) on the same standard-form LP; wall time and objective."""
    import numpy as np
    import scipy.sparse as sp
    from scipy.optimize import linprog
    if qp.nnzh or not np.all(qp.lcon == qp.ucon):
        return None
    A = sp.csr_matrix((qp.Avals, (qp.Arows, qp.Acols)), shape=(qp.ncon, qp.nvar))
    bnds = [(a if np.isfinite(a) else None, b if np.isfinite(b) else None) for a, b in zip(qp.lvar, qp.uvar)]
    sg = 1.0 if qp.minimize else -1.0
    t0 = time.perf_counter()
    r = linprog(sg * qp.c, A_eq=A, b_eq=qp.lcon, bounds=bnds, method="highs-ipm",
                options=dict(presolve=False, disp=False, time_limit=time_limit))
    dt = time.perf_counter() - t0
    return {"status": int(r.status), "message": r.message, "objective": sg * float(r.fun) + qp.c0 if r.fun is not None else None,
            "ipm_iterations": int(getattr(r, "nit", 0) or 0), "wall_s": dt}


# Peaks (MI355X): HBM3E 8.0 TB/s spec (/opt/skills/guides/MI355X_MICROARCH.md); f64 MFMA
# (v_mfma_f64_16x16x4f64) 78.6 TFLOP/s dense, AMD spec (the guide tabulates no f64 row;
# profiles/r1_mfma_f64_peak.txt holds our own measurement of the instruction's rate).
PEAK_HBM_GBS = 8000.0
STATUS = {1: "SOLVE_SUCCEEDED", 2: "INFEASIBLE_PROBLEM_DETECTED", -1: "MAXIMUM_ITERATIONS_EXCEEDED",
          -2: "MAXIMUM_WALLTIME_EXCEEDED", -3: "DIVERGING_ITERATES", -4: "ERROR_IN_STEP_COMPUTATION",
          -5: "INTERNAL_ERROR"}
PEAK_F64_TFS = 78.6


def roofline(stats: list, dominant: str, config: str = "ex10"):
    """Roofline object for the dominant kernel from the live HIP-event statistics of the timed region.
    achieved = SURVEY 8(d)'s algorithmic bytes per launch (8 nnzL + 12 nnzK of the columns the launch
    factorises, exact column counts of the symbolic analysis; 8 nnzL of the columns a solve launch
    substitutes) / the event-timed average launch; the kernel's own staging-traffic model is reported
    beside it as `staging_bytes_per_launch`, the PMC-measured HBM bytes as `traffic`."""
    k = next(x for x in stats if x["name"] == dominant)
    if k["launches"] == 0 or k["time_ms"] <= 0:
        return None
    avg_s = k["time_ms"] / k["launches"] * 1e-3
    flops, nbytes = k["flops"] / k["launches"], k["alg_bytes"] / k["launches"]
    staging = k["bytes"] / k["launches"]
    mfma = flops / (PEAK_F64_TFS * 1e12) > nbytes / (PEAK_HBM_GBS * 1e9)
    if mfma:
        ach, peak, unit = flops / avg_s / 1e12, PEAK_F64_TFS, "TFLOP/s"
    else:
        ach, peak, unit = nbytes / avg_s / 1e9, PEAK_HBM_GBS, "GB/s"
    traffic, src, traffic_lo = None, None, None
    def _rv(path):  # r<round>_v<n> (numeric: r2_v10 after r2_v3) or r<round>_<letters> (r4_i after r4_h)
        m = re.search(r"r(\d+)_(?:v(\d+)|([a-z]+))_", os.path.basename(path))
        if not m:
            return (-1, -1)
        return (int(m.group(1)), int(m.group(2)) if m.group(2) else sum(ord(ch) * 128 ** -k for k, ch in enumerate(m.group(3))))

    # the newest PMC pass of THIS workload: files tagged r<round>_<letter>_<config>_pmc_traffic.json, or
    # untagged ones (r<round>_<v>_pmc_traffic.json: ex10, the bench workload)
    cfgs = ("ex10", "supportcase10", "neos", "dense_qp")
    def _mine(path):
        b = os.path.basename(path)
        tagged = [c for c in cfgs if f"_{c}_pmc_traffic" in b]
        return (config in tagged) if tagged else config == "ex10"
    pmc = sorted((f for f in glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json")) if _mine(f)), key=_rv)
    if pmc:  # PMC counters can not be read inside the timed run: the latest committed pass of this workload
        ent = json.load(open(pmc[-1]))["kernels"].get(dominant)
        if ent:
            traffic, src = ent["hbm_bytes_per_launch"], os.path.relpath(pmc[-1], ROOT)
            traffic_lo = ent.get("hbm_bytes_lo_per_launch")
    return {"bound": "mfma" if mfma else "hbm", "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak,
            "traffic": traffic, "traffic_lo": traffic_lo, "traffic_source": src,
            "traffic_definition": "PMC bytes per launch: 2 FETCH_SIZE + WRITE_SIZE (upper bound; traffic_lo = "
                                  "FETCH_SIZE + WRITE_SIZE, exact for 8-B gathers; profiles/r3_e1_fetch_calib.txt)", "kernel": dominant, "launches": k["launches"],
            "avg_launch_us": avg_s * 1e6, "alg_bytes_per_launch": nbytes, "alg_flops_per_launch": flops,
            "alg_bytes_definition": "SURVEY 8(d): 8 nnzL + 12 nnzK of the columns the launch factorises",
            "staging_bytes_per_launch": staging}


def iteration_roofline(info: dict, ms_per_step: float, vec_passes: int = 60) -> dict:
    """Whole-iteration roofline from SURVEY 8(d)'s per-phase algorithmic counts: factorisation
    B = 8 nnzL + 12 nnzK, F = the analysis' flop count; 2 solves B = 2 x 16 nnzL, F = 2 x 4 nnzL;
    2 residual SpMVs B = 2 x (12 nnzK + 16 N); vector kernels B ~ vec_passes x 8 N (an estimate of
    the ~60 length-N vector reads/writes of the RHS / step / barrier / evaluation kernels).  Each
    phase is bounded by max(B / 8 TB/s, F / 78.6 TF/s); frac = sum of the bounds / measured step."""
    nnzL, nnzK, N, F = float(info["nnzL"]), float(info["nnzK"]), float(info["n"]), float(info["flops"])
    phases = {"factorization": (8 * nnzL + 12 * nnzK, F), "solves": (32 * nnzL, 8 * nnzL),
              "residuals": (2 * (12 * nnzK + 16 * N), 4 * nnzK), "vector_kernels": (vec_passes * 8 * N, 0.0)}
    bound = {k: max(b / (PEAK_HBM_GBS * 1e9), f / (PEAK_F64_TFS * 1e12)) * 1e6 for k, (b, f) in phases.items()}
    t_roof = sum(bound.values())
    return {"alg_bytes": sum(b for b, _ in phases.values()), "alg_flops": sum(f for _, f in phases.values()),
            "bound_us": {k: round(v, 2) for k, v in bound.items()}, "time_at_roofline_us": t_roof,
            "measured_us": ms_per_step * 1e3, "frac": t_roof / (ms_per_step * 1e3)}


def rocm_version() -> str | None:
    try:
        with open("/opt/rocm/.info/version") as f:
            return f.read().strip()
    except OSError:
        return None


def aggregate(dt, iters, dist, sharded):
    """Whole-job numbers: max time over ranks; iterations = those of the one sharded solve, or the
    sum over ranks (replicas).  Also returns every rank's own time (s)."""
    if dist is None:
        return dt, float(iters), [dt]
    import torch
    ts = [torch.zeros(1, dtype=torch.float64) for _ in range(dist.get_world_size())]
    dist.all_gather(ts, torch.tensor([dt], dtype=torch.float64))
    per_rank = [float(t.item()) for t in ts]
    it = torch.tensor([float(iters)], dtype=torch.float64)
    dist.all_reduce(it, op=dist.ReduceOp.MAX if sharded else dist.ReduceOp.SUM)
    return max(per_rank), float(it.item()), per_rank


def collective_volume(info, warm, world=None):
    """Sharded factorisation: doubles exchanged per factorisation (all-reduce of the top fronts) and per
    solve (all-reduce of the top rows + in-place all-gather of the subtree solution slices; ldl_info
    xch_*), per MPC iteration with the solves-per-factorisation ratio seen in the warm-up launch
    counts; with `world`, the ring model's bytes each rank sends per iteration (all-reduce of m
    doubles: 2 (P-1)/P 8m; all-gather of G doubles in P slices: (P-1)/P 8G)."""
    if not info.get("xch_fact"):
        return None
    launches = {k["name"]: k["launches"] for k in warm}
    nfact = launches.get("k_fact_tree") or launches.get("k_small_blocked") or 1
    nsolve = launches.get("k_bwd_tree") or launches.get("k_bwd_tiny") or 2 * nfact
    spf = nsolve / nfact
    gat = info.get("xch_gather", 0)
    out = {"fact_bytes": 8 * info["xch_fact"], "solve_bytes": 8 * (info["xch_solve"] + gat),
           "solve_allreduce_bytes": 8 * info["xch_solve"], "solve_allgather_bytes": 8 * gat,
           "solves_per_fact": spf, "collectives_per_iter": 1 + 2 * spf,
           "bytes_per_iter": 8 * (info["xch_fact"] + spf * (info["xch_solve"] + gat))}
    if world and world > 1:
        f = (world - 1) / world
        out["wire_bytes_per_rank_per_iter"] = 8 * f * (2 * info["xch_fact"] + spf * (2 * info["xch_solve"] + gat))
    return out


def kkt_measures(qp, st) -> dict:
    """Optimality measures of the returned unscaled point (x, y, zl, zu) of min/max c'x + x'Hx/2 + c0,
    Ax = b, l <= x <= u, in the solver's sign convention (sigma = -1 for a maximisation: the reference
    flips only the reported objective, src/utils.jl:150-156): relative primal residual, relative
    stationarity sigma (c + Hx) + A'y - zl + zu, the bound violation, and the duality gap between the
    primal objective and the Lagrangian dual bound (src/kernels.jl:408-430).  The dense QP instance
    (column-major A, madipm_amd.instances.dense_qp) is applied as a dense (n x m) view: no 5e8-entry
    sparse matrix on the host."""
    import numpy as np
    n, m = qp.nvar, qp.ncon
    sg = 1.0 if getattr(qp, "minimize", True) else -1.0
    x, y, zl, zu = st.solution, st.multipliers, st.multipliers_L, st.multipliers_U
    if qp.nnzj == n * m and qp.name.startswith("dense_qp"):
        V = np.asarray(qp.Avals).reshape(n, m)  # row j = column j of A
        Ax, Aty = V.T @ x, V @ y
    else:
        import scipy.sparse as sp
        A = sp.csr_matrix((qp.Avals, (qp.Arows, qp.Acols)), shape=(m, n))
        Ax, Aty = A @ x, A.T @ y
    hx = np.zeros(n)
    np.add.at(hx, qp.Hrows, qp.Hvals * x[qp.Hcols])
    off = qp.Hrows != qp.Hcols
    np.add.at(hx, qp.Hcols[off], qp.Hvals[off] * x[qp.Hrows[off]])
    b = qp.lcon
    lo, hi = np.isfinite(qp.lvar), np.isfinite(qp.uvar)
    pobj = qp.c0 + qp.c @ x + 0.5 * x @ hx
    dobj = sg * (sg * qp.c0 - y @ b + zl[lo] @ qp.lvar[lo] - zu[hi] @ qp.uvar[hi] - sg * 0.5 * x @ hx)
    return {"pr": float(np.max(np.abs(Ax - b)) / (1.0 + np.max(np.abs(b)))),
            "du": float(np.max(np.abs(sg * (qp.c + hx) + Aty - zl + zu)) / (1.0 + np.max(np.abs(qp.c)))),
            "bounds": float(max(np.max((qp.lvar - x)[lo], initial=-1.0), np.max((x - qp.uvar)[hi], initial=-1.0))),
            "pobj": float(pobj), "dobj": float(dobj), "gap_rel": float(abs(pobj - dobj) / max(1.0, abs(pobj)))}


def golden_parity(config: str, qp, so) -> dict:
    """Parity of a solve to optimality: the HiGHS 1.x IPM + crossover optimum of the same seeded
    stand-in (tests/golden/fullsize_highs.json, tools/make_golden_fullsize.py; full-size configs only)
    at BASELINE.md's |dobj| <= 1e-6 max(1, |obj|), and the point's own KKT measures (absolute
    thresholds pr, du <= 1e-6, gap <= 1e-6 relative).  A config with no HiGHS optimum (the dense QP:
    scipy's HiGHS has no QP) rests on the KKT certificate alone (convex: feasible + zero gap =
    optimal) — parity unpinned against any reference fixture."""
    out = {"status": so.status_name, "iters": so.iter, "objective": so.objective}
    try:
        k = kkt_measures(qp, so)
    except Exception as e:  # pragma: no cover - reported, not hidden
        k = {"error": repr(e)}
    out["kkt"] = k
    ok = so.status_name == "SOLVE_SUCCEEDED" and "error" not in k and k["pr"] <= 1e-6 and k["du"] <= 1e-6 \
        and k["gap_rel"] <= 1e-6 and k["bounds"] <= 1e-8
    name, _, sc = config.partition("@")
    try:
        g = json.load(open(os.path.join(ROOT, "tests", "golden", "fullsize_highs.json"))).get(name) if not sc else None
    except OSError:
        g = None
    if g and g.get("nvar") == qp.nvar and g.get("ncon") == qp.ncon:
        rel = abs(so.objective - g["objective"]) / max(1.0, abs(g["objective"]))
        out.update({"reference": "HiGHS IPM + crossover optimum of the same stand-in (tests/golden/fullsize_highs.json)",
                    "objective_ref": g["objective"], "rel_obj_diff": rel})
        ok = ok and rel <= 1e-6
    else:
        out["reference"] = "KKT certificate of the returned point only (no reference fixture: parity unpinned)"
    out["ok"] = bool(ok)
    return out


def timed_leg(solver, steps, warmup, dist, sharded, barrier, config="ex10"):
    """The timed part of a leg: `warmup` untimed iterations with every LDL^T kernel kind event-timed
    (the dominant kind), then EXACTLY `steps` iterations after initialize!, bracketed by barriers
    (barrier() also synchronises the device), HIP events around the dominant kind only (its roofline);
    whole-job numbers by `aggregate` (max time over ranks).  A solve that ends before its share of the
    iterations (optimality) is followed by another from initialize! (outside the clock) for the rest.
    Returns (leg, warm stats, stats of the last timed solve)."""
    import torch
    solver.set_kernel_timing()
    solver.set_max_iter(max(warmup, 1))
    done = solver.solve().iter
    while 0 < done < warmup:
        solver.set_max_iter(warmup - done)
        k = solver.solve().iter
        if k <= 0:
            break
        done += k
    warm = solver.kernel_stats()
    dominant = max(warm, key=lambda k: k["time_ms"])["name"]
    breakdown = {k["name"]: round(k["time_ms"], 3) for k in sorted(warm, key=lambda k: -k["time_ms"]) if k["launches"]}
    solver.set_kernel_timing(1 << [k["name"] for k in warm].index(dominant))
    dt, iters, sts = 0.0, 0, []
    while iters < steps:
        solver.set_max_iter(steps - iters)
        solver.initialize()
        barrier()
        t0 = time.perf_counter()
        # the MPC loop only: update_solution!'s host copies of the solution vectors come after the
        # reference's cnt.total_time (src/solver.jl:406-413) and are not part of an iteration
        st = solver.solve(fetch_solution=False)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        barrier()
        dt += time.perf_counter() - t0
        sts.append(st)
        if st.iter <= 0:  # a solve that makes no iteration would never fill the count
            break
        iters += st.iter
    roof = roofline(solver.kernel_stats(), dominant, config)
    solver.set_kernel_timing(0)
    dt, total_iters, per_rank = aggregate(dt, iters, dist, sharded)
    # the library's own clock around the timed iterations (every timed solve's cnt.total_time)
    lib_s = sum(s.counters.total_time for s in sts) if all(hasattr(s, "counters") for s in sts) else None
    return ({"iters_per_s": total_iters / dt, "ms_per_iter": 1e3 * dt / max(iters, 1), "steps": steps,
             "warmup": warmup, "iters_timed": iters, "timed_solves": len(sts), "roofline": roof,
             "kernel_ms_warmup": breakdown, "per_rank_s": per_rank, "loop_total_time_s": lib_s}, warm, st)


def dump_outputs(solver, st, out_dir, cap_bytes=64 << 20):
    """--dump-outputs: what a caller of the timed path receives after its last step, as
    <out_dir>/<name>.npy (float64): the unscaled point update_solution! returns (solution, multipliers,
    multipliers_L, multipliers_U, constraints) read back from the device as the timed solve left it,
    and `summary` = [status, iterations of the last timed solve, objective, dual objective, inf_pr,
    inf_du, inf_compl].  An array that would take the files past `cap_bytes` in all is cut to a fixed
    seeded sample of its entries (in index order)."""
    import ctypes as C
    import numpy as np
    from madipm_amd import _lib as L
    nx, m = solver.qp.nvar, solver.qp.ncon
    x, zl, zu, y, cons = np.empty(nx), np.empty(nx), np.empty(nx), np.empty(m), np.empty(m)
    L.check(L.lib.madipm_solver_get_solution(solver.h, L.ptr(x, C.c_double), L.ptr(y, C.c_double),
                                             L.ptr(zl, C.c_double), L.ptr(zu, C.c_double), L.ptr(cons, C.c_double)),
            "get_solution")
    arrays = {"solution": x, "multipliers": y, "multipliers_L": zl, "multipliers_U": zu, "constraints": cons,
              "summary": np.array([st.status, st.iter, st.objective, st.dual_objective, st.primal_feas,
                                   st.dual_feas, st.inf_compl], np.float64)}
    cap = cap_bytes // 8 // len(arrays)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        if a.size > cap:
            a = a[np.sort(np.random.default_rng(0).choice(a.size, cap, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def run_leg(config, steps, warmup, comm=None, dist=None, sharded=False, barrier=None, world=1, opt=True,
            ordering=None, dump=None):
    """One BASELINE config end to end: build (the reference pipeline), analysis + upload (timed), W
    warmup iterations with every LDL^T kernel kind event-timed (the dominant kind), EXACTLY `steps`
    iterations after initialize! with HIP events around the dominant kind only, whole-job numbers
    (max time over ranks), then (dump) the timed solve's outputs to that folder and (opt) a solve to optimality: status, iterations, loop time, end to end
    = analysis + initialisation + loop, and golden_parity.  Returns (leg dict, solver, qp)."""
    import torch
    from madipm_amd import MPCSolver
    if barrier is None:
        def barrier():
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()
    qp, name = build_problem(config)
    extra = {}
    if config.startswith("dense_qp"):
        # x first (natural order): the x columns are batched leaves eliminated by one MFMA SYRK; AMD/ND
        # on the complete bipartite graph of a dense A would only rediscover this order, slowly
        extra["ordering"] = 0
    if ordering is not None:
        extra["ordering"] = ordering
    t_an = time.perf_counter()
    solver = MPCSolver(qp, comm=comm, **solver_opts(), **extra)
    t_analysis = time.perf_counter() - t_an
    info = solver.ldl_info()
    leg, warm, st = timed_leg(solver, steps, warmup, dist, sharded, barrier, config.partition("@")[0])
    ms = leg["ms_per_iter"]
    leg.update({"workload": name, "nvar": qp.nvar, "ncon": qp.ncon, "nnzj": qp.nnzj, "kkt_n": info["n"],
                "nnzL": info["nnzL"], "nnzL_stored": info["nnzL_stored"], "fact_flops": info["flops"],
                "fronts": info["nsuper"], "levels": info["nlevels"], "leaf_batch_members": info["lb_members"],
                "parallelism": f"subtree-shard{world}" if sharded else f"replicas{world}",
                "analysis_s": t_analysis, "iteration_roofline": iteration_roofline(info, ms),
                "collectives": collective_volume(info, warm, world)})
    if dump and (dist is None or dist.get_rank() == 0):
        dump_outputs(solver, st, dump)
    if opt:
        solver.set_max_iter(300)
        t1 = time.perf_counter()
        so = solver.solve()
        e2e = time.perf_counter() - t1
        leg.update({"status": so.status_name, "iters_to_opt": so.iter, "wall_clock_to_opt_s": so.counters.total_time,
                    "init_plus_loop_s": e2e, "objective": so.objective,
                    "linear_solver_time_s": so.counters.linear_solver_time,
                    # end-to-end = symbolic analysis + initialisation + loop to optimality
                    "end_to_end_s": t_analysis + e2e})
        if dist is None or dist.get_rank() == 0:
            leg["parity"] = golden_parity(config, qp, so)
    return leg, solver, qp


LEG_STEPS = {"supportcase10": (20, 2), "dense_qp": (3, 1), "neos": (8, 2)}  # (timed steps, warmup) per leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="ex10")
    ap.add_argument("--full", action="store_true",
                    help="beside the timed steps: the solve to optimality with its parity, the legs of the other "
                         "BASELINE configs, the CPU baseline and HiGHS (trimmed by --no-opt, --legs, --no-cpu, "
                         "--no-highs); without it the run times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step left (solution, multipliers, multipliers_L, "
                         "multipliers_U, constraints, summary) as DIR/<name>.npy")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--highs", action=argparse.BooleanOptionalAction, default=True,
                    help="time HiGHS-IPM (scipy) on the same LP as a third-party CPU datapoint")
    ap.add_argument("--no-opt", action="store_true", help="skip the wall-clock-to-optimality solve")
    ap.add_argument("--ordering", type=int, default=None, help="LDL ordering override (0 natural, 1 AMD, 3 ND, 4 auto)")
    ap.add_argument("--mode", choices=["shard", "replicas"], default="shard",
                    help="N > 1: one subtree-sharded solve (RCCL) or N independent replicas")
    ap.add_argument("--legs", default=None,
                    help="comma list of extra BASELINE configs timed under their own keys (default: "
                         "supportcase10,dense_qp,neos at N = 1, neos at N > 1; 'none' for none)")
    ap.add_argument("--neos", action=argparse.BooleanOptionalAction, default=True,
                    help="--no-neos drops the neos leg")
    ap.add_argument("--neos-steps", type=int, default=LEG_STEPS["neos"][0])
    args = ap.parse_args()

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    torch.cuda.set_device(local)
    from madipm_amd import _lib
    _lib.check(_lib.madipm_set_device(local), "madipm_set_device")  # the library's own HIP runtime
    if world > 1:
        import torch.distributed as dist
        # host-side process group for the id broadcast, barriers and the timing max; the data-path
        # collectives of the sharded factorisation are RCCL, issued by the library on its stream
        dist.init_process_group("gloo")
    sharded = world > 1 and args.mode == "shard"

    from madipm_amd import RCCLComm
    comm = RCCLComm.from_torch(dist) if sharded else None

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    main_leg, solver, qp = run_leg(args.config, args.steps, args.warmup, comm, dist, sharded, barrier, world,
                                   opt=args.full and not args.no_opt, ordering=args.ordering,
                                   dump=args.dump_outputs)
    kperm = solver.kkt_perm() if rank == 0 else None
    del solver

    base = args.config.partition("@")[0]
    if not args.full:
        legs = []
    elif args.legs is None:
        legs = ["supportcase10", "dense_qp", "neos"] if world == 1 else ["neos"]
    else:
        legs = [] if args.legs == "none" else [c for c in args.legs.split(",") if c]
    if not args.neos:
        legs = [c for c in legs if c != "neos"]
    legs = [c for c in legs if c.partition("@")[0] != base]
    extra = {}
    for c in legs:
        steps, warm = LEG_STEPS.get(c.partition("@")[0], (8, 2))
        if c.startswith("neos"):
            steps = args.neos_steps
        try:
            leg, s2, q2 = run_leg(c, steps, warm, comm, dist, sharded, barrier, world, opt=True)
            del s2, q2
        except Exception as e:  # pragma: no cover - reported, not hidden
            leg = {"error": repr(e)}
        extra[c] = leg
        import gc
        gc.collect()

    if rank == 0:
        it = main_leg
        opt_keys = ("status", "iters_to_opt", "wall_clock_to_opt_s", "init_plus_loop_s", "analysis_s", "objective",
                    "linear_solver_time_s", "end_to_end_s")
        cfg = {k: it[k] for k in ("workload", "nvar", "ncon", "nnzj", "kkt_n", "nnzL", "nnzL_stored", "fact_flops",
                                  "fronts", "levels", "leaf_batch_members", "parallelism")}
        cfg.update({k: it[k] for k in opt_keys if k in it})
        cfg["analysis_s"] = it["analysis_s"]
        out = {
            "metric": "IPM iters/sec + wall-clock-to-opt, MIPLIB LP, 1/2/4/8 MI355X vs host CPU",
            "value": it["iters_per_s"],
            "unit": "iters/s",
            "n_gpus": world,
            "steps": it["iters_timed"],  # the iterations under the clock: --steps
            "timed_solves": it["timed_solves"],
            "warmup": args.warmup,
            "ms_per_step": it["ms_per_iter"],
            "higher_is_better": True,
            "scaling": "strong" if sharded else "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "rocm": rocm_version(),
            "data": "synthetic (seeded structured stand-ins; no MIPLIB MPS offline)",
            "config": cfg,
            "roofline": it["roofline"],
            "iteration_roofline": it["iteration_roofline"],
            "kernel_ms_warmup": it["kernel_ms_warmup"],
            "per_rank_s": it["per_rank_s"],
            "loop_total_time_s": it["loop_total_time_s"],
            "collectives": it["collectives"],
            **extra,
            "cpu_baseline": None,
            "parity": it.get("parity"),
        }
        if args.full and not args.no_cpu and world == 1 and not base.startswith(("dense_qp", "neos")):
            try:
                (r_status, r_obj, r_iter), out["cpu_baseline"] = cpu_baseline(args.config, kperm,
                                                                               baseline_threads())
                if "objective" in it:
                    # parity at the benchmarked size: the GPU solve to optimality vs the oracle's (same
                    # problem, same settings; BASELINE.md parity rule |dobj| <= 1e-6 max(1, |obj|)),
                    # beside the HiGHS optimum and the KKT measures of golden_parity
                    rel = abs(it["objective"] - r_obj) / max(1.0, abs(r_obj))
                    p = out["parity"] or {}
                    p["oracle"] = {"reference": "oracle/mpc.py + MKL PARDISO (CPU)",
                                   "status_gpu": it["status"], "status_ref": STATUS.get(r_status, r_status),
                                   "status_equal": STATUS.get(r_status) == it["status"],
                                   "objective_gpu": it["objective"], "objective_ref": r_obj,
                                   "rel_obj_diff": rel, "iters_gpu": it["iters_to_opt"], "iters_ref": r_iter,
                                   "ok": bool(STATUS.get(r_status) == it["status"] and rel <= 1e-6
                                              and abs(it["iters_to_opt"] - r_iter) <= 1)}
                    p["ok"] = bool(p.get("ok", True) and p["oracle"]["ok"])
                    out["parity"] = p
            except Exception as e:  # pragma: no cover - reported, not hidden
                out["cpu_baseline"] = {"error": repr(e)}
            if args.highs:
                try:
                    out["cpu_baseline"]["highs_ipm"] = highs_baseline(qp)
                except Exception as e:  # pragma: no cover
                    out["cpu_baseline"]["highs_ipm"] = {"error": repr(e)}
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
