"""Re-solve with new numbers against re-construction, on the ex10 and supportcase10 stand-ins
(python tools/resolve_bench.py [ex10 supportcase10 ...]; MADIPM_SYMBOLIC_TIMING=1 adds update()'s phases
on stderr).

Per instance: construct_s (MPCSolver(qp), bench.py's analysis_s), prepare_update_s (the refresh plan, once),
update_s (counters()["last_update_s"]: host wall time of one update, its stream synchronisation included;
median of 10 after 2 warm-ups) and solve_s (initialize! + the MPC loop on the updated problem, same
median).  Every update installs c, the finite bounds and the values of A (and H) times 1 + 1e-3 U(-1, 1),
seeded — lower and upper bound of a coordinate by the same factor, so the classification of every bound is
the creation-time one.  The last updated solve is compared with a fresh solver on the same data
(matches_fresh: same status, iterations, objective bits).

The device route runs in the same process on the same sequence of perturbed data, held in torch tensors:
update_device_s (counters()["last_update_s"] of MPCSolver.update_device, same median) beside the host
update_s, and update + solve + solution_device() (the results left in device tensors, stream synchronised)
against host update + solve with the host fetch; device_matches_fresh compares the last device-updated
solve with the same fresh solver.  Ends with one JSON line.

--warm WEIGHT adds the warm-started device loop on the same sequence of data, in the same process:
warm_start_last(WEIGHT) after each solve (the previous solution, taken before the update), then update_device
+ solve + solution_device: warm_iters and warm_device_loop_s beside iters and device_loop_s, warm_status,
and warm_obj_rel, the largest relative difference of a warm solve's objective from the cold solve's on the
same data.  Without the option nothing of it runs and the output is as before.

--adjoint adds, on the same sequence of data and in the same process, one adjoint per re-solve: after each
update_device + solve, adjoint_device of a seeded gx for all seven gradients, stream synchronised:
adjoint_s (the first adjoint on a point: the factorisation of its KKT matrix + one solve + the gradient
kernels) beside adjoint_solve_s (the solve before it) and adjoint_again_s (a second gx on the same point,
which reuses the factor), adjoint_residual (the largest last_residual) and adjoint_status.

--adjoint-full is --adjoint with one more call per point, after the two above and on the same factor:
adjoint_device with seeded cotangents of all five solution blocks (gx, gy, gzl, gzu, gcons), for all seven
gradients: adjoint_full_s beside adjoint_again_s, and adjoint_full_residual, the largest last_residual of
those calls (the residual of the shifted system).

--tangent adds, on the same sequence of data and in the same process, the forward-mode call: after each
update_device + solve, tangent_device of a seeded direction in all seven data blocks for all five outputs,
stream synchronised: tangent_s (the first call on a point: the factorisation + the solves) beside
tangent_solve_s (the solve before it) and tangent_again_s (a second direction on the same point),
tangent_residual (the largest last_residual) and tangent_status.  With --warm WEIGHT it also runs the
sequence twice more, warm-started from the previous solution (warm_start_last) and from the first-order
prediction solution + tangent along the actual next perturbation (warm_start_device):
tangent_warm_iters_last and tangent_warm_iters_predicted.

--polish adds, on the same sequence of data and in the same process, the exact active-set solve: after each
update_device + solve, polish_device for all seven blocks, stream synchronised: polish_s (the first call on a
point: classification, factorisation, three solves, the verdict's read-back) beside polish_solve_s (the solve
before it) and polish_again_s (a second call with the returned set supplied: no factorisation), polish_verdicts
(how often each verdict came back), polish_residual (the largest) and the counters.

--polished-sens adds the sensitivities at the polished point: after each update_device + solve +
polish_device, one tangent_device(polished=True) of a seeded direction in all seven data blocks for all five
outputs and one adjoint_device(polished=True) of seeded cotangents of all five blocks for all seven gradients,
each with the stream synchronised: polished_tangent_s, polished_adjoint_s (medians), polished_sens_residual (the
largest), polished_sens_verdicts and polished_sens_refused (the points whose polish did not end POLISHED: the
calls are refused there, by design: the LP stand-ins are degenerate).  The instance name sparse_qp is the
strictly complementary 1000 x 600 sparse QP of the tests (tests/adjoint_oracle.py), on which every point is
polished.

--active-set adds the active-set re-solve: after one update_device + solve + polish_device (which
leaves a kept set when it ends POLISHED), per updated problem of the same sequence update_device +
active_set_solve_device from the kept set, stream synchronised (active_set_loop_s; active_set_s without the
update), beside update_device + solve + polish_device on the same data (active_set_ipm_loop_s): the verdicts, the
rounds, active_set_share (the part of the problems the active-set route solved: POLISHED) and the counters.  A
problem whose attempt does not end POLISHED is solved by the interior-point route, whose polish renews the kept set
when it can; active_set_failed_s is the cost of such an attempt.  While the solver keeps no set (no polish has ended
POLISHED: the degenerate LP stand-ins) the attempt starts from the set the last polish guessed, supplied.  --rel REL sets the relative noise of every
sequence (default 1e-3).

--sens-batch K adds the batched sensitivities: after each update_device + solve, and after one single
tangent_device that factorises the point, one tangent_batch_device and one adjoint_batch_device of K seeded
columns (all seven direction blocks / all five cotangents given, all outputs), each against K single tangent_device /
adjoint_device calls of the same columns on the same point, stream synchronised, medians of 10:
sens_batch_tangent_s / sens_loop_tangent_s, sens_batch_adjoint_s / sens_loop_adjoint_s, and sens_batch_same_bits (every
row of the batches is the single call's).  --multi-solve (with --sens-batch) times the two batched calls once more with
MPCSolver.set_multi_solve on: sens_multi_tangent_s / sens_multi_adjoint_s beside the batched and looped
columns, sens_multi_rel_diff (the rows' largest difference to the switch off, relative to max(1, max |block|)), the
spread (max - min) of the ten looped samples and multi_solve_info(), which says how the big fronts were solved (DESIGN
§13k: a chunk's columns in one pass; with MADIPM_MULTI_BIG=0 in the environment column after column).  The instance name random_qp:N is instances.random_qp with N variables, N / 4 rows and about 8 entries per row."""
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "madipm.jl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from madipm_amd import MPCSolver  # noqa: E402
from madipm_amd import _lib  # noqa: E402

WARMUP, REPS, REL = 2, 10, 1e-3


def perturb(qp, rng):
    """The value fields of qp under relative noise REL that keeps every classification."""
    def f(k):
        return 1.0 + REL * rng.uniform(-1.0, 1.0, k)
    fv, fc = f(qp.nvar), f(qp.ncon)
    return dict(c=qp.c * f(qp.nvar), Avals=qp.Avals * f(qp.nnzj), Hvals=qp.Hvals * f(qp.nnzh),
                lvar=qp.lvar * fv, uvar=qp.uvar * fv, lcon=qp.lcon * fc, ucon=qp.ucon * fc)


def build_problem(name):
    if name == "sparse_qp":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import adjoint_oracle
        return adjoint_oracle.sparse_fixture()[0], "strictly complementary sparse QP of the tests, 1000 x 600"
    if name.startswith("random_qp:"):
        from madipm_amd import instances
        n = int(name.split(":")[1])
        return (instances.random_qp(n // 4, n, density=8.0 / n, seed=0),
                f"instances.random_qp, {n} box-bounded variables, {n // 4} equality rows, about 8 entries per row")
    return bench.build_problem(name)


def run(name, warm=None, adjoint=False, adjoint_full=False, tangent=False, polish=False, polished_sens=False,
        active_set=False, sens_batch=None, multi_solve=False):
    qp, desc = build_problem(name)
    opts = bench.solver_opts()
    MPCSolver(qp, **opts)                      # the first construction of a process pays one-off set-up
    t = time.perf_counter()
    s = MPCSolver(qp, **opts)
    construct_s = time.perf_counter() - t
    t = time.perf_counter()
    st0 = s.solve(fetch_solution=False)
    solve0_s = time.perf_counter() - t
    rng = np.random.default_rng(0)
    new = perturb(qp, rng)
    t = time.perf_counter()
    s.update(**new)                            # the first update builds the plan
    first_update_s = time.perf_counter() - t
    prepare_update_s = first_update_s - s.counters()["last_update_s"]
    upd, call, sol, its, hostloop = [], [], [], [], []
    for rep in range(WARMUP + REPS):
        new = perturb(qp, rng)
        t = time.perf_counter()
        s.update(**new)
        t_call = time.perf_counter() - t
        t = time.perf_counter()
        st = s.solve(fetch_solution=False)
        t_solve = time.perf_counter() - t
        t = time.perf_counter()
        s.update(**new)
        s.solve()                              # the whole host loop: update + solve + the host fetch
        t_loop = time.perf_counter() - t
        if rep >= WARMUP:
            upd.append(s.counters()["last_update_s"])
            call.append(t_call)
            sol.append(t_solve)
            its.append(st.iter)
            hostloop.append(t_loop)
    fresh = MPCSolver(dataclasses.replace(qp, **new), **opts).solve(fetch_solution=False)
    # ---- the device route: the same sequence of data, in torch tensors
    rng = np.random.default_rng(0)
    perturb(qp, rng)                           # the first update's draw
    s.update_device(**{k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()})  # allocates
    rng = np.random.default_rng(0)
    perturb(qp, rng)
    dupd, dcall, devloop, dobj = [], [], [], []
    for rep in range(WARMUP + REPS):
        dnew = {k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()}
        torch.cuda.synchronize()
        t = time.perf_counter()
        s.update_device(**dnew)
        t_call = time.perf_counter() - t
        dst = s.solve(fetch_solution=False)
        t = time.perf_counter()
        s.update_device(**dnew)
        s.solve(fetch_solution=False)
        s.solution_device()
        torch.cuda.current_stream().synchronize()
        t_loop = time.perf_counter() - t
        dobj.append(dst.objective)
        if rep >= WARMUP:
            dupd.append(s.counters()["last_update_s"])
            dcall.append(t_call)
            devloop.append(t_loop)
    c = s.counters()
    wres = {}
    if warm is not None:   # the same data again, each solve started from the previous solution
        rng = np.random.default_rng(0)
        perturb(qp, rng)
        wits, wloop, wstat, wrel = [], [], set(), 0.0
        for rep in range(WARMUP + REPS):
            dnew = {k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()}
            torch.cuda.synchronize()
            t = time.perf_counter()
            s.warm_start_last(warm)
            s.update_device(**dnew)
            wst = s.solve(fetch_solution=False)
            s.solution_device()
            torch.cuda.current_stream().synchronize()
            t_loop = time.perf_counter() - t
            wrel = max(wrel, abs(wst.objective - dobj[rep]) / max(1.0, abs(dobj[rep])))
            if rep >= WARMUP:
                wits.append(wst.iter)
                wloop.append(t_loop)
                wstat.add(wst.status)
        s.clear_warm_start()
        wres = {"warm_weight": warm, "warm_iters": wits, "warm_device_loop_s": statistics.median(wloop),
                "warm_status": sorted(wstat), "warm_obj_rel": wrel, "n_warm_inits": s.warm_info()["n_warm_inits"]}
        c = s.counters()
    if adjoint:   # the same data again: one adjoint (all seven gradients) per re-solve
        rng = np.random.default_rng(0)
        perturb(qp, rng)
        grng = np.random.default_rng(1)
        asol, afirst, aagain, astat, ares = [], [], [], set(), 0.0
        afull, afres = [], 0.0
        for rep in range(WARMUP + REPS):
            dnew = {k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()}
            gx = torch.as_tensor(grng.standard_normal(qp.nvar), device="cuda")
            gx2 = torch.as_tensor(grng.standard_normal(qp.nvar), device="cuda")
            s.update_device(**dnew)
            torch.cuda.synchronize()
            t = time.perf_counter()
            ast = s.solve(fetch_solution=False)
            t_solve = time.perf_counter() - t
            astat.add(ast.status)
            if ast.status != 1:
                continue
            t = time.perf_counter()
            s.adjoint_device(gx)
            torch.cuda.current_stream().synchronize()
            t_first = time.perf_counter() - t
            t = time.perf_counter()
            s.adjoint_device(gx2)
            torch.cuda.current_stream().synchronize()
            t_again = time.perf_counter() - t
            ares = max(ares, s.adjoint_info()["last_residual"])
            if adjoint_full:
                draw = lambda k: torch.as_tensor(grng.standard_normal(k), device="cuda")  # noqa: E731
                cot = dict(gy=draw(qp.ncon), gzl=draw(qp.nvar), gzu=draw(qp.nvar), gcons=draw(qp.ncon))
                torch.cuda.synchronize()
                t = time.perf_counter()
                s.adjoint_device(gx, **cot)
                torch.cuda.current_stream().synchronize()
                t_full = time.perf_counter() - t
                afres = max(afres, s.adjoint_info()["last_residual"])
                if rep >= WARMUP:
                    afull.append(t_full)
            if rep >= WARMUP:
                asol.append(t_solve)
                afirst.append(t_first)
                aagain.append(t_again)
        med = lambda v: statistics.median(v) if v else float("nan")  # noqa: E731
        wres.update({"adjoint_s": med(afirst), "adjoint_again_s": med(aagain), "adjoint_solve_s": med(asol),
                     "adjoint_residual": ares, "adjoint_status": sorted(astat), **s.adjoint_info()})
        if adjoint_full:
            wres.update({"adjoint_full_s": med(afull), "adjoint_full_residual": afres})
        c = s.counters()
    if tangent:   # the same data again: the forward-mode call (all seven blocks, all five outputs) per re-solve
        rng = np.random.default_rng(0)
        perturb(qp, rng)
        seq = [perturb(qp, rng) for _ in range(WARMUP + REPS + 1)]
        drng = np.random.default_rng(2)
        size = dict(c=qp.nvar, Hvals=qp.nnzh, Avals=qp.nnzj, lcon=qp.ncon, ucon=qp.ncon, lvar=qp.nvar, uvar=qp.nvar)
        dev = lambda d: {k: torch.as_tensor(v, device="cuda") for k, v in d.items()}  # noqa: E731
        draw = lambda: dev({k: drng.standard_normal(n) for k, n in size.items()})  # noqa: E731
        tsol, tfirst, tagain, tstat, tres = [], [], [], set(), 0.0
        for rep in range(WARMUP + REPS):
            s.update_device(**dev(seq[rep]))
            d1, d2 = draw(), draw()
            torch.cuda.synchronize()
            t = time.perf_counter()
            tst = s.solve(fetch_solution=False)
            t_solve = time.perf_counter() - t
            tstat.add(tst.status)
            if tst.status != 1:
                continue
            t = time.perf_counter()
            s.tangent_device(**d1)
            torch.cuda.current_stream().synchronize()
            t_first = time.perf_counter() - t
            t = time.perf_counter()
            s.tangent_device(**d2)
            torch.cuda.current_stream().synchronize()
            t_again = time.perf_counter() - t
            tres = max(tres, s.tangent_info()["last_residual"])
            if rep >= WARMUP:
                tsol.append(t_solve)
                tfirst.append(t_first)
                tagain.append(t_again)
        med = lambda v: statistics.median(v) if v else float("nan")  # noqa: E731
        wres.update({"tangent_s": med(tfirst), "tangent_again_s": med(tagain), "tangent_solve_s": med(tsol),
                     "tangent_residual": tres, "tangent_status": sorted(tstat), **s.tangent_info()})
        if warm is not None:   # the next solve started from the last solution, or from solution + tangent
            for mode in ("last", "predicted"):
                its_, stat_ = [], set()
                s.clear_warm_start()
                s.update_device(**dev(seq[0]))
                ok = s.solve(fetch_solution=False).status == 1
                for rep in range(1, WARMUP + REPS + 1):
                    cur, nxt = dev(seq[rep - 1]), dev(seq[rep])
                    if not ok:
                        s.clear_warm_start()
                    elif mode == "last":
                        s.warm_start_last(warm)
                    else:   # an infinite bound gives inf - inf = NaN, in an entry that is not read
                        pt = s.solution_device()
                        tg = s.tangent_device(want=("x", "y", "zl", "zu"), **{k: nxt[k] - cur[k] for k in nxt})
                        s.warm_start_device(x=pt["solution"] + tg["x"], y=pt["multipliers"] + tg["y"],
                                            zl=pt["multipliers_L"] + tg["zl"], zu=pt["multipliers_U"] + tg["zu"],
                                            weight=warm)
                    s.update_device(**nxt)
                    wst = s.solve(fetch_solution=False)
                    ok = wst.status == 1
                    stat_.add(wst.status)
                    if rep > WARMUP:
                        its_.append(wst.iter)
                wres.update({f"tangent_warm_iters_{mode}": its_, f"tangent_warm_status_{mode}": sorted(stat_)})
            s.clear_warm_start()
        c = s.counters()
    if polish:   # the same data again: the exact active-set solve per re-solve, then again with its set supplied
        rng = np.random.default_rng(0)
        perturb(qp, rng)
        psol, pfirst, pagain, pstat, pverd, pres = [], [], [], set(), {}, 0.0
        for rep in range(WARMUP + REPS):
            s.update_device(**{k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()})
            torch.cuda.synchronize()
            t = time.perf_counter()
            pst = s.solve(fetch_solution=False)
            t_solve = time.perf_counter() - t
            pstat.add(pst.status)
            if pst.status != 1:
                continue
            t = time.perf_counter()
            p1 = s.polish_device()
            torch.cuda.current_stream().synchronize()
            t_first = time.perf_counter() - t
            t = time.perf_counter()
            p2 = s.polish_device(active_var=p1["active_var"], active_row=p1["active_row"])
            torch.cuda.current_stream().synchronize()
            t_again = time.perf_counter() - t
            v = p1["info"]["verdict"].name
            pverd[v] = pverd.get(v, 0) + 1
            if np.isfinite(p1["info"]["residual"]):
                pres = max(pres, p1["info"]["residual"])
            assert p2["info"]["verdict"] == p1["info"]["verdict"]
            if rep >= WARMUP:
                psol.append(t_solve)
                pfirst.append(t_first)
                pagain.append(t_again)
        med = lambda v: statistics.median(v) if v else float("nan")  # noqa: E731
        info = s.polish_info()
        wres.update({"polish_s": med(pfirst), "polish_again_s": med(pagain), "polish_solve_s": med(psol),
                     "polish_verdicts": pverd, "polish_residual": pres, "polish_status": sorted(pstat),
                     "polish_n_active": info["n_active"], "n_polishes": info["n_polishes"],
                     "n_polish_factorizations": info["n_polish_factorizations"]})
        c = s.counters()
    if polished_sens:   # the same data again: one polished tangent and one polished adjoint per polished point
        from madipm_amd import MadIPMError, PolishVerdict
        rng = np.random.default_rng(0)
        perturb(qp, rng)
        drng = np.random.default_rng(3)
        size = dict(c=qp.nvar, Hvals=qp.nnzh, Avals=qp.nnzj, lcon=qp.ncon, ucon=qp.ncon, lvar=qp.nvar, uvar=qp.nvar)
        csize = dict(gx=qp.nvar, gy=qp.ncon, gzl=qp.nvar, gzu=qp.nvar, gcons=qp.ncon)
        draw = lambda sz: {k: torch.as_tensor(drng.standard_normal(n), device="cuda") for k, n in sz.items()}  # noqa: E731
        qtan, qadj, qverd, qres, refused = [], [], {}, 0.0, 0
        for rep in range(WARMUP + REPS):
            s.update_device(**{k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()})
            if s.solve(fetch_solution=False).status != 1:
                continue
            verdict = s.polish_device()["info"]["verdict"]
            qverd[verdict.name] = qverd.get(verdict.name, 0) + 1
            d, cot = draw(size), draw(csize)
            torch.cuda.synchronize()
            if verdict != PolishVerdict.POLISHED:
                try:
                    s.tangent_device(polished=True, **d)
                except MadIPMError:
                    refused += 1
                continue
            t = time.perf_counter()
            s.tangent_device(polished=True, **d)
            torch.cuda.current_stream().synchronize()
            t_tan = time.perf_counter() - t
            qres = max(qres, s.polished_sens_info()["last_residual"])
            t = time.perf_counter()
            s.adjoint_device(cot.pop("gx"), polished=True, **cot)
            torch.cuda.current_stream().synchronize()
            t_adj = time.perf_counter() - t
            qres = max(qres, s.polished_sens_info()["last_residual"])
            if rep >= WARMUP:
                qtan.append(t_tan)
                qadj.append(t_adj)
        med = lambda v: statistics.median(v) if v else float("nan")  # noqa: E731
        wres.update({"polished_tangent_s": med(qtan), "polished_adjoint_s": med(qadj), "polished_sens_residual": qres,
                     "polished_sens_verdicts": qverd, "polished_sens_refused": refused,
                     **{"polished_" + k: v for k, v in s.polished_sens_info().items() if k != "last_residual"}})
        c = s.counters()
    if active_set:   # the same data again: the active-set re-solve from the kept set against solve + polish
        from madipm_amd import PolishVerdict
        rng = np.random.default_rng(0)
        s.update_device(**{k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()})
        first, last_set = "not solved", None   # last_set: the set the last polish tried, whatever its verdict
        if s.solve(fetch_solution=False).status == 1:
            pol = s.polish_device()
            first, last_set = pol["info"]["verdict"].name, (pol["active_var"], pol["active_row"])
        aloop, acall, afail, iloop, averd, arounds, share = [], [], [], [], {}, [], 0
        for rep in range(WARMUP + REPS):
            dnew = {k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()}
            torch.cuda.synchronize()
            verdict = None
            t_loop = t_call = float("nan")
            if s.has_kept_set() or last_set is not None:
                # no kept set (no polish has ended POLISHED yet: the degenerate LP stand-ins): the last polish's guess
                start = {} if s.has_kept_set() else dict(active_var=last_set[0], active_row=last_set[1])
                t = time.perf_counter()
                s.update_device(**dnew)
                t1 = time.perf_counter()
                res = s.active_set_solve_device(**start)
                torch.cuda.current_stream().synchronize()
                t_loop, t_call = time.perf_counter() - t, time.perf_counter() - t1
                verdict = res["info"]["verdict"]
            t = time.perf_counter()
            s.update_device(**dnew)
            ist = s.solve(fetch_solution=False)
            if ist.status == 1:
                pol = s.polish_device()
                last_set = (pol["active_var"], pol["active_row"])
            torch.cuda.current_stream().synchronize()
            t_ipm = time.perf_counter() - t
            if rep >= WARMUP:
                v = verdict.name if verdict is not None else "no kept set"
                averd[v] = averd.get(v, 0) + 1
                iloop.append(t_ipm)
                if verdict == PolishVerdict.POLISHED:
                    share += 1
                    aloop.append(t_loop)
                    acall.append(t_call)
                    arounds.append(res["info"]["rounds"])
                elif verdict is not None:
                    afail.append(t_call)
                    arounds.append(res["info"]["rounds"])
        med = lambda v: statistics.median(v) if v else float("nan")  # noqa: E731
        wres.update({"active_set_first_polish": first, "active_set_loop_s": med(aloop), "active_set_s": med(acall),
                     "active_set_failed_s": med(afail), "active_set_ipm_loop_s": med(iloop),
                     "active_set_verdicts": averd, "active_set_rounds": arounds, "active_set_share": share / REPS,
                     **{"active_set_" + k: v for k, v in s.active_set_info().items()
                        if k in ("n_calls", "n_factorizations")}})
        c = s.counters()
    if sens_batch:   # the same data again: K columns in one batched call against K single calls on the same point
        K = int(sens_batch)
        rng = np.random.default_rng(0)
        perturb(qp, rng)
        drng = np.random.default_rng(4)
        size = dict(c=qp.nvar, Hvals=qp.nnzh, Avals=qp.nnzj, lcon=qp.ncon, ucon=qp.ncon, lvar=qp.nvar, uvar=qp.nvar)
        csize = dict(gx=qp.nvar, gy=qp.ncon, gzl=qp.nvar, gzu=qp.nvar, gcons=qp.ncon)
        draw = lambda sz: {k: torch.as_tensor(drng.standard_normal((K, n)), device="cuda") for k, n in sz.items()}  # noqa: E731
        sync = lambda: torch.cuda.current_stream().synchronize()  # noqa: E731
        bt, lt, ba, la, same, bstat = [], [], [], [], True, set()
        mt, ma, mrel = [], [], 0.0   # --multi-solve: the batched calls again with set_multi_solve on
        rel = lambda a, b: float((a - b).abs().max() / max(1.0, float(b.abs().max()))) if b.numel() else 0.0  # noqa: E731
        for rep in range(WARMUP + REPS):
            s.update_device(**{k: torch.as_tensor(v, device="cuda") for k, v in perturb(qp, rng).items()})
            st_ = s.solve(fetch_solution=False).status
            bstat.add(st_)
            if st_ != 1:
                continue
            d, cot = draw(size), draw(csize)
            s.tangent_device(**{k: v[0] for k, v in d.items()})      # the point's factorisation
            torch.cuda.synchronize()
            t = time.perf_counter()
            tb = s.tangent_batch_device(**d)
            sync()
            t_bt = time.perf_counter() - t
            t = time.perf_counter()
            ts = [s.tangent_device(**{k: v[j] for k, v in d.items()}) for j in range(K)]
            sync()
            t_lt = time.perf_counter() - t
            t = time.perf_counter()
            gb = s.adjoint_batch_device(**cot)
            sync()
            t_ba = time.perf_counter() - t
            t = time.perf_counter()
            gs = [s.adjoint_device(**{k: v[j] for k, v in cot.items()}) for j in range(K)]
            sync()
            t_la = time.perf_counter() - t
            same = same and all(torch.equal(tb[k][j], ts[j][k]) for j in range(K) for k in tb) \
                and all(torch.equal(gb[k][j], gs[j][k]) for j in range(K) for k in gb)
            if multi_solve:
                s.set_multi_solve(True)
                t = time.perf_counter()
                tm = s.tangent_batch_device(**d)
                sync()
                t_mt = time.perf_counter() - t
                t = time.perf_counter()
                gm = s.adjoint_batch_device(**cot)
                sync()
                t_ma = time.perf_counter() - t
                s.set_multi_solve(False)
                mrel = max([mrel] + [rel(tm[k], tb[k]) for k in tb] + [rel(gm[k], gb[k]) for k in gb])
                if rep >= WARMUP:
                    mt.append(t_mt)
                    ma.append(t_ma)
            if rep >= WARMUP:
                bt.append(t_bt)
                lt.append(t_lt)
                ba.append(t_ba)
                la.append(t_la)
        med = lambda v: statistics.median(v) if v else float("nan")  # noqa: E731
        wres.update({"sens_batch_k": K, "sens_batch_cols": s.sens_batch_cols(), "sens_batch_tangent_s": med(bt),
                     "sens_loop_tangent_s": med(lt), "sens_batch_adjoint_s": med(ba), "sens_loop_adjoint_s": med(la),
                     "sens_batch_same_bits": bool(same), "sens_batch_status": sorted(bstat), **s.sens_batch_info()})
        spread = lambda v: (max(v) - min(v)) if v else float("nan")  # noqa: E731
        wres.update({"sens_loop_tangent_spread_s": spread(lt), "sens_loop_adjoint_spread_s": spread(la)})
        if multi_solve:
            wres.update({"sens_multi_tangent_s": med(mt), "sens_multi_adjoint_s": med(ma), "sens_multi_rel_diff": mrel,
                         "sens_multi_info": s.multi_solve_info()})
        c = s.counters()
    update_s, solve_s = statistics.median(upd), statistics.median(sol)
    return {**wres, "instance": name, "description": desc, "nvar": qp.nvar, "ncon": qp.ncon, "nnzj": qp.nnzj, "nnzh": qp.nnzh,
            "construct_s": construct_s, "prepare_update_s": prepare_update_s, "update_s": update_s,
            "update_call_s": statistics.median(call),   # MPCSolver.update: + the Python copies of the arrays
            "solve_s": solve_s, "first_solve_s": solve0_s, "status": st.status, "first_status": st0.status,
            "iters": its, "first_iters": st0.iter,
            "update_plus_solve_s": update_s + solve_s, "construct_plus_solve_s": construct_s + solve_s,
            "speedup": (construct_s + solve_s) / (update_s + solve_s),
            "matches_fresh": bool(fresh.status == st.status and fresh.iter == st.iter
                                  and np.float64(fresh.objective).tobytes() == np.float64(st.objective).tobytes()),
            "update_device_s": statistics.median(dupd), "update_device_call_s": statistics.median(dcall),
            "host_loop_s": statistics.median(hostloop),       # update + solve + get_solution (host arrays)
            "device_loop_s": statistics.median(devloop),      # update_device + solve + solution_device + sync
            "device_matches_fresh": bool(fresh.status == dst.status and fresh.iter == dst.iter
                                         and np.float64(fresh.objective).tobytes()
                                         == np.float64(dst.objective).tobytes()),
            "n_analyses": c["n_analyses"], "n_updates": c["n_updates"]}


def main():
    torch.cuda.set_device(0)
    _lib.check(_lib.madipm_set_device(0), "madipm_set_device")
    torch.zeros(1, device="cuda")
    out = []
    args, warm = sys.argv[1:], None
    if "--warm" in args:
        k = args.index("--warm")
        warm = float(args[k + 1])
        del args[k:k + 2]
    adjoint_full = "--adjoint-full" in args
    if adjoint_full:
        args.remove("--adjoint-full")
    adjoint = "--adjoint" in args or adjoint_full
    if "--adjoint" in args:
        args.remove("--adjoint")
    tangent = "--tangent" in args
    if tangent:
        args.remove("--tangent")
    polish = "--polish" in args
    if polish:
        args.remove("--polish")
    polished_sens = "--polished-sens" in args
    if polished_sens:
        args.remove("--polished-sens")
    active_set = "--active-set" in args
    if active_set:
        args.remove("--active-set")
    sens_batch = None
    if "--sens-batch" in args:
        k = args.index("--sens-batch")
        sens_batch = int(args[k + 1])
        del args[k:k + 2]
    multi_solve = "--multi-solve" in args
    if multi_solve:
        args.remove("--multi-solve")
    if "--rel" in args:
        global REL
        k = args.index("--rel")
        REL = float(args[k + 1])
        del args[k:k + 2]
    for name in args or ["ex10", "supportcase10"]:
        r = run(name, warm, adjoint, adjoint_full, tangent, polish, polished_sens, active_set, sens_batch, multi_solve)
        print(f"{name}: construct_s {r['construct_s']:.4f}  prepare_update_s {r['prepare_update_s']:.4f}  "
              f"update_s {r['update_s']:.5f}  solve_s {r['solve_s']:.4f}  ->  update + solve "
              f"{r['update_plus_solve_s']:.4f} s against construct + solve {r['construct_plus_solve_s']:.4f} s "
              f"(x{r['speedup']:.1f}), matches_fresh {r['matches_fresh']}", flush=True)
        print(f"{name}: device route: update_device_s {r['update_device_s']:.5f} (host update_s {r['update_s']:.5f})  "
              f"update_device + solve + solution_device {r['device_loop_s']:.4f} s against update + solve + host "
              f"fetch {r['host_loop_s']:.4f} s, device_matches_fresh {r['device_matches_fresh']}", flush=True)
        if warm is not None:
            print(f"{name}: warm start {warm}: iterations {statistics.median(r['warm_iters'])} (cold "
                  f"{statistics.median(r['iters'])})  warm_start_last + update_device + solve + solution_device "
                  f"{r['warm_device_loop_s']:.4f} s (cold {r['device_loop_s']:.4f} s), status {r['warm_status']}, "
                  f"objective within {r['warm_obj_rel']:.1e} of the cold solve's", flush=True)
        if adjoint:
            print(f"{name}: adjoint (seven gradients): {r['adjoint_s']:.4f} s after a solve of "
                  f"{r['adjoint_solve_s']:.4f} s; a second gx on the same point {r['adjoint_again_s']:.4f} s; "
                  f"residual <= {r['adjoint_residual']:.1e}, status {r['adjoint_status']}", flush=True)
        if adjoint_full:
            print(f"{name}: adjoint with all five cotangents on the same point {r['adjoint_full_s']:.4f} s, "
                  f"residual <= {r['adjoint_full_residual']:.1e}", flush=True)
        if tangent:
            print(f"{name}: tangent (seven direction blocks, five outputs): {r['tangent_s']:.4f} s after a solve of "
                  f"{r['tangent_solve_s']:.4f} s; a second direction on the same point {r['tangent_again_s']:.4f} s; "
                  f"residual <= {r['tangent_residual']:.1e}, status {r['tangent_status']}", flush=True)
            if warm is not None:
                med = lambda v: statistics.median(v) if v else float("nan")  # noqa: E731
                print(f"{name}: warm start {warm} from solution + tangent: iterations "
                      f"{med(r['tangent_warm_iters_predicted'])} (status {r['tangent_warm_status_predicted']}), "
                      f"from the last solution alone {med(r['tangent_warm_iters_last'])} (status "
                      f"{r['tangent_warm_status_last']}), cold {med(r['iters'])}", flush=True)
        if polish:
            print(f"{name}: polish (seven blocks): {r['polish_s']:.4f} s after a solve of {r['polish_solve_s']:.4f} s; "
                  f"again with the returned set supplied {r['polish_again_s']:.4f} s; verdicts {r['polish_verdicts']}, "
                  f"residual <= {r['polish_residual']:.1e}, {r['polish_n_active']} active in the last set, "
                  f"{r['n_polish_factorizations']} factorisations in {r['n_polishes']} calls", flush=True)
        if polished_sens:
            print(f"{name}: at the polished point: tangent (seven direction blocks, five outputs) "
                  f"{r['polished_tangent_s']:.4f} s, adjoint (five cotangents, seven gradients) "
                  f"{r['polished_adjoint_s']:.4f} s; verdicts {r['polished_sens_verdicts']}, refused "
                  f"{r['polished_sens_refused']}, residual <= {r['polished_sens_residual']:.1e}, "
                  f"{r['polished_n_factorizations']} factorisations of their own", flush=True)
        if active_set:
            print(f"{name}: active-set re-solve: update_device + active_set_solve_device {r['active_set_loop_s']:.4f} s "
                  f"(the call alone {r['active_set_s']:.4f} s) against update_device + solve + polish_device "
                  f"{r['active_set_ipm_loop_s']:.4f} s; verdicts {r['active_set_verdicts']}, rounds "
                  f"{r['active_set_rounds']}, share {r['active_set_share']:.2f}; a failed attempt "
                  f"{r['active_set_failed_s']:.4f} s; first polish {r['active_set_first_polish']}; "
                  f"{r['active_set_n_factorizations']} factorisations in {r['active_set_n_calls']} calls", flush=True)
        if sens_batch:
            K = r["sens_batch_k"]
            print(f"{name}: {K} columns (chunks of {r['sens_batch_cols']}): tangent_batch_device "
                  f"{r['sens_batch_tangent_s'] * 1e3:.3f} ms against {K} tangent_device calls "
                  f"{r['sens_loop_tangent_s'] * 1e3:.3f} ms (x{r['sens_loop_tangent_s'] / r['sens_batch_tangent_s']:.2f}); "
                  f"adjoint_batch_device {r['sens_batch_adjoint_s'] * 1e3:.3f} ms against {K} adjoint_device calls "
                  f"{r['sens_loop_adjoint_s'] * 1e3:.3f} ms (x{r['sens_loop_adjoint_s'] / r['sens_batch_adjoint_s']:.2f}); "
                  f"same bits {r['sens_batch_same_bits']}, status {r['sens_batch_status']}", flush=True)
            if multi_solve:
                mi = r["sens_multi_info"]
                big = (f"{mi['n_big_fronts']} big fronts at {mi['n_big_levels']} levels, "
                       + ("a chunk's columns in one pass" if mi["multi_big"] else "column after column")
                       + f", {mi['n_big_passes']} big passes, {mi['big_bytes']} B of multi-column big-front buffers")
                print(f"{name}: multi-solve on ({'native' if mi['native'] else 'the loop'}, {big}): "
                      f"tangent_batch_device {r['sens_multi_tangent_s'] * 1e3:.3f} ms "
                      f"(x{r['sens_loop_tangent_s'] / r['sens_multi_tangent_s']:.2f} of the loop, whose samples spread "
                      f"{r['sens_loop_tangent_spread_s'] * 1e3:.3f} ms); adjoint_batch_device "
                      f"{r['sens_multi_adjoint_s'] * 1e3:.3f} ms (x{r['sens_loop_adjoint_s'] / r['sens_multi_adjoint_s']:.2f}, "
                      f"spread {r['sens_loop_adjoint_spread_s'] * 1e3:.3f} ms); rows within "
                      f"{r['sens_multi_rel_diff']:.1e} of the switch off", flush=True)
        out.append(r)
    print(json.dumps({"resolve_bench": out, "warmup": WARMUP, "reps": REPS, "rel_noise": REL}))


if __name__ == "__main__":
    main()
