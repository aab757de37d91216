"""Host-side mirror of MadIPM's public interface over the native (HIP) solver.

Same names and argument meaning as the reference (src/MadIPM.jl exports `MPCSolver`, `madipm`;
options are IPMOptions fields, src/utils.jl:69-105; types src/utils.jl:10-48):

    solver = MPCSolver(qp; tol=1e-8, max_iter=300, linear_solver=HIPLDLSolver,
                       regularization=FixedRegularization(1e-8, -1e-8), step_rule=AdaptiveStep(0.99))
    stats = solver.solve()          # solve!(solver)
    stats = madipm(qp; kwargs...)   # madipm(m; kwargs...)

Every computation of the solve runs in libmadipm_hip on the GPU; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from .linear_solver import HIPLDLSolver
from .qp import QuadraticModel


# ---------------------------------------------------------------- option types (src/utils.jl:10-48)
class AbstractBarrierUpdate: ...


class Mehrotra(AbstractBarrierUpdate): ...


@dataclass
class ConservativeStep:
    tau: float = 0.995


@dataclass
class AdaptiveStep:
    tau_min: float = 0.99


@dataclass
class MehrotraAdaptiveStep:
    gamma_f: float = 0.99


@dataclass
class NoRegularization: ...


@dataclass
class FixedRegularization:
    delta_p: float
    delta_d: float


@dataclass
class AdaptiveRegularization:
    delta_p: float
    delta_d: float
    delta_min: float


class SparseKKTSystem: ...          # K2 (MadNLP.SparseKKTSystem)


class ScaledSparseKKTSystem: ...    # K2.5 (MadNLP.ScaledSparseKKTSystem; src/kernels.jl:139-149)


class NormalKKTSystem: ...          # src/KKT/normalkkt.jl (LPs only; A Sigma^-1 A^T, Cholesky semantics)


_KKT_CODES = {SparseKKTSystem: 0, ScaledSparseKKTSystem: 1, NormalKKTSystem: 2}


# MadNLP.Status
STATUS_NAMES = {
    0: "REGULAR", 1: "SOLVE_SUCCEEDED", 2: "INFEASIBLE_PROBLEM_DETECTED",
    -1: "MAXIMUM_ITERATIONS_EXCEEDED", -2: "MAXIMUM_WALLTIME_EXCEEDED", -3: "DIVERGING_ITERATES",
    -4: "ERROR_IN_STEP_COMPUTATION", -5: "INTERNAL_ERROR",
}
SOLVE_SUCCEEDED = 1
INFEASIBLE_PROBLEM_DETECTED = 2
MAXIMUM_ITERATIONS_EXCEEDED = -1
MAXIMUM_WALLTIME_EXCEEDED = -2
DIVERGING_ITERATES = -3
ERROR_IN_STEP_COMPUTATION = -4
INTERNAL_ERROR = -5


class Options(C.Structure):
    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int32), ("max_wall_time", C.c_double),
                ("divergence_tol", C.c_double), ("scaling", C.c_int32), ("bound_push", C.c_double),
                ("bound_fac", C.c_double), ("bound_relax_factor", C.c_double), ("regularization", C.c_int32),
                ("delta_p", C.c_double), ("delta_d", C.c_double), ("delta_min", C.c_double),
                ("step_rule", C.c_int32), ("step_tau", C.c_double), ("max_ncorr", C.c_int32),
                ("mu_init", C.c_double), ("mu_min", C.c_double), ("tol_linear_solve", C.c_double),
                ("check_residual", C.c_int32), ("kkt_system", C.c_int32), ("print_level", C.c_int32),
                ("ldl", L.LDLOpts)]


class QPStruct(C.Structure):
    _fields_ = [("nvar", C.c_int32), ("ncon", C.c_int32), ("nnzh", C.c_int64), ("nnzj", C.c_int64),
                ("c", L.f64p), ("c0", C.c_double), ("Hrows", L.i32p), ("Hcols", L.i32p), ("Hvals", L.f64p),
                ("Arows", L.i32p), ("Acols", L.i32p), ("Avals", L.f64p), ("lcon", L.f64p), ("ucon", L.f64p),
                ("lvar", L.f64p), ("uvar", L.f64p), ("x0", L.f64p), ("y0", L.f64p), ("minimize", C.c_int32)]


class QPUpdate(C.Structure):
    """madipm_qp_update: new numbers for an existing solver's problem; a NULL pointer keeps the current data."""
    _fields_ = [("c", L.f64p), ("c0", L.f64p), ("Hvals", L.f64p), ("Avals", L.f64p), ("lcon", L.f64p),
                ("ucon", L.f64p), ("lvar", L.f64p), ("uvar", L.f64p), ("x0", L.f64p), ("y0", L.f64p)]


class Stats(C.Structure):
    _fields_ = [("status", C.c_int32), ("iter", C.c_int32), ("objective", C.c_double),
                ("dual_objective", C.c_double), ("inf_pr", C.c_double), ("inf_du", C.c_double),
                ("inf_compl", C.c_double), ("mu", C.c_double), ("total_time", C.c_double),
                ("linear_solver_time", C.c_double), ("init_time", C.c_double), ("exception", C.c_int32)]


# The exceptions solve!'s catch-all turns into INTERNAL_ERROR (src/solver.jl:398-403) and rethrows
# when rethrow_error = true (the reference benchmark sets it, scripts/benchmarks_cpu.jl:39).
class SolveException(Exception):
    """MadNLP.SolveException, thrown (as a type) by solve_system! (src/linear_solver.jl:40-41)."""


class UnfactorizedSolveException(Exception):
    """The linear solver refusing a solve after every trial of factorize_regularized_system!
    (src/linear_solver.jl:6-17) failed (LDLFactorizations' ldiv! on an unfactorized object [EXT])."""


MadIPMError = L.MadIPMError  # a refused library call (MPCSolver.update on a change of classification)
EXC_NONE, EXC_SOLVE, EXC_UNFACTORIZED = 0, 1, 2
_EXCEPTIONS = {EXC_SOLVE: SolveException, EXC_UNFACTORIZED: UnfactorizedSolveException}


class IterTrace(C.Structure):
    _fields_ = [("k", C.c_int32), ("obj", C.c_double), ("inf_pr", C.c_double), ("inf_du", C.c_double),
                ("inf_compl", C.c_double), ("mu", C.c_double), ("alpha_p", C.c_double),
                ("alpha_d", C.c_double), ("del_w", C.c_double), ("dx_inf", C.c_double),
                ("residual", C.c_double)]


L._sig("madipm_default_options", None, [C.POINTER(Options)])
L._sig("madipm_solver_create", C.c_int, [C.POINTER(QPStruct), C.POINTER(Options), C.POINTER(L.vp)])
L._sig("madipm_solver_create_dist", C.c_int, [C.POINTER(QPStruct), C.POINTER(Options), L.vp, C.POINTER(L.vp)])
L._sig("madipm_solver_solve", C.c_int, [L.vp, C.POINTER(Stats)])
L._sig("madipm_solver_initialize", C.c_int, [L.vp])
L._sig("madipm_solver_set_max_iter", C.c_int, [L.vp, C.c_int32])
L._sig("madipm_solver_get_solution", C.c_int, [L.vp, L.f64p, L.f64p, L.f64p, L.f64p, L.f64p])
L._sig("madipm_solver_trace", C.c_int, [L.vp, C.POINTER(IterTrace), C.c_int32])
L._sig("madipm_solver_ldl_info", C.c_int, [L.vp, C.POINTER(L.LDLInfo)])
L._sig("madipm_solver_ldl_perm", C.c_int, [L.vp, L.i32p])
L._sig("madipm_solver_spmv_group", C.c_int, [L.vp])
L._sig("madipm_solver_set_timing", C.c_int, [L.vp, C.c_uint32])
L._sig("madipm_solver_kernel_stats", C.c_int, [L.vp, C.POINTER(L.KStat)])
L._sig("madipm_solver_destroy", None, [L.vp])
L._sig("madipm_solver_prepare_update", C.c_int, [L.vp, C.POINTER(QPStruct)])
L._sig("madipm_solver_update", C.c_int, [L.vp, C.POINTER(QPUpdate)])
L._sig("madipm_solver_counters", C.c_int, [L.vp, L.i64p, L.i64p, L.f64p])
L._sig("madipm_solver_update_device", C.c_int, [L.vp, C.POINTER(QPUpdate), L.vp])
L._sig("madipm_solver_get_solution_device", C.c_int, [L.vp, L.f64p, L.f64p, L.f64p, L.f64p, L.f64p, L.vp])
L._sig("madipm_solver_get_data", C.c_int, [L.vp] + [L.f64p] * 10)


def check_device_array(name: str, a, length: int, device=None, who: str = "update_device"):
    """The argument check of MPCSolver.update_device, before any library call: `a` must be a torch tensor on
    the GPU (on `device` when given), float64, contiguous, of shape (length,).  TypeError for a numpy array,
    a CPU tensor or another dtype; ValueError for a non-contiguous tensor or another shape.  Returns `a`.
    `who` names the calling method in the message."""
    import torch
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch tensor on the GPU, not {type(a).__name__}")
    if a.dtype != torch.float64:
        raise TypeError(f"{who}: {name} has dtype {a.dtype}, expected torch.float64")
    if not a.is_contiguous():  # a property of the tensor alone: checked before where it lives
        raise ValueError(f"{who}: {name} is not contiguous")
    if a.device.type != "cuda":
        raise TypeError(f"{who}: {name} is on {a.device}, expected a GPU tensor")
    if device is not None and a.device != device:
        raise TypeError(f"{who}: {name} is on {a.device}, the solver is on {device}")
    if tuple(a.shape) != (int(length),):
        raise ValueError(f"{who}: {name} has shape {tuple(a.shape)}, expected ({int(length)},)")
    return a


ADJOINT_NAMES = ("c", "Hvals", "Avals", "lcon", "ucon", "lvar", "uvar")


def check_adjoint_want(want) -> tuple:
    """The `want` argument of MPCSolver.adjoint / adjoint_device: None (all seven) or an iterable of names out
    of ADJOINT_NAMES.  Returns the names in ADJOINT_NAMES order; ValueError for an unknown name or an empty
    selection, TypeError for a bare string."""
    if want is None:
        return ADJOINT_NAMES
    if isinstance(want, str):
        raise TypeError(f"adjoint: want must be a collection of names, not the string {want!r}")
    want = list(want)
    unknown = [k for k in want if k not in ADJOINT_NAMES]
    if unknown:
        raise ValueError(f"adjoint: unknown name(s) {unknown} in want; the gradients are {list(ADJOINT_NAMES)}")
    if not want:
        raise ValueError("adjoint: want is empty")
    return tuple(k for k in ADJOINT_NAMES if k in want)


COTANGENT_NAMES = ("x", "y", "zl", "zu", "cons")   # madipm_qp_cotangents' fields; gx, gy, gzl, gzu, gcons


def check_adjoint_cotangents(nvar: int, ncon: int, gx=None, gy=None, gzl=None, gzu=None, gcons=None, *,
                             on_device: bool = False, device=None, who: str = "adjoint") -> dict:
    """The cotangent arguments of MPCSolver.adjoint / adjoint_device, before any library call: gx, gzl, gzu of
    shape (nvar,), gy, gcons of shape (ncon,), each optional (None: 0) but not all five.  Host route: each is
    converted to a C-contiguous float64 array.  Device route (on_device): each must pass check_device_array.
    Returns {field of madipm_qp_cotangents: array} of those given, in COTANGENT_NAMES order."""
    given = {}
    for field, name, a, length in (("x", "gx", gx, nvar), ("y", "gy", gy, ncon), ("zl", "gzl", gzl, nvar),
                                   ("zu", "gzu", gzu, nvar), ("cons", "gcons", gcons, ncon)):
        if a is None:
            continue
        if on_device:
            check_device_array(name, a, length, device, who=who)
        else:
            a = np.array(a, dtype=np.float64, order="C", ndmin=1)
            if a.shape != (int(length),):
                raise ValueError(f"{who}: {name} has shape {a.shape}, expected ({int(length)},)")
        given[field] = a
    if not given:
        raise ValueError(f"{who}: no cotangent given; pass at least one of gx, gy, gzl, gzu, gcons")
    return given


TANGENT_NAMES = COTANGENT_NAMES   # MPCSolver.tangent's output blocks; its directions' blocks are ADJOINT_NAMES


def check_tangent_want(want) -> tuple:
    """The `want` argument of MPCSolver.tangent / tangent_device: None (all five) or an iterable of names out
    of TANGENT_NAMES.  Returns the names in TANGENT_NAMES order; ValueError for an unknown name or an empty
    selection, TypeError for a bare string."""
    if want is None:
        return TANGENT_NAMES
    if isinstance(want, str):
        raise TypeError(f"tangent: want must be a collection of names, not the string {want!r}")
    want = list(want)
    unknown = [k for k in want if k not in TANGENT_NAMES]
    if unknown:
        raise ValueError(f"tangent: unknown name(s) {unknown} in want; the blocks are {list(TANGENT_NAMES)}")
    if not want:
        raise ValueError("tangent: want is empty")
    return tuple(k for k in TANGENT_NAMES if k in want)


def check_tangent_directions(sizes: dict, directions: dict, *, on_device: bool = False, device=None,
                             who: str = "tangent") -> dict:
    """The direction arguments of MPCSolver.tangent / tangent_device, before any library call: `directions`
    maps names out of ADJOINT_NAMES to arrays (None: 0) of the lengths in `sizes`, not all seven None.  Host
    route: each is converted to a C-contiguous float64 array.  Device route (on_device): each must pass
    check_device_array.  Returns {name: array} of those given, in ADJOINT_NAMES order."""
    given = {}
    for name in ADJOINT_NAMES:
        a = directions.get(name)
        if a is None:
            continue
        if on_device:
            check_device_array(name, a, sizes[name], device, who=who)
        else:
            a = np.array(a, dtype=np.float64, order="C", ndmin=1)
            if a.shape != (int(sizes[name]),):
                raise ValueError(f"{who}: {name} has shape {a.shape}, expected ({int(sizes[name])},)")
        given[name] = a
    if not given:
        raise ValueError(f"{who}: no direction given; pass at least one of {', '.join(ADJOINT_NAMES)}")
    return given


def check_batch_blocks(sizes: dict, blocks: dict, *, labels: dict | None = None, on_device: bool = False,
                       device=None, who: str = "tangent_batch") -> tuple:
    """The direction / cotangent arguments of MPCSolver.tangent_batch / adjoint_batch (and the device routes),
    before any library call: `blocks` maps the names in `sizes` to arrays of shape (k, sizes[name]) (None: 0 in
    every column), not all None, all with the same k >= 1.  Host route: each is converted to a C-contiguous
    float64 array.  Device route (on_device): each must be a contiguous float64 tensor on the GPU, checked by
    check_device_array (its TypeErrors and its ValueError for a non-contiguous tensor).  ValueError for a block
    that is not 2-D, a wrong second dimension, k == 0 and blocks whose k disagree.  `labels` maps a name to the
    keyword the messages use (the cotangents: x -> gx, ...).  Returns (k, {name: array} of those given, in the
    order of `sizes`)."""
    labels = labels or {}
    given, k, first = {}, None, None
    for name, length in sizes.items():
        a = blocks.get(name)
        if a is None:
            continue
        label = labels.get(name, name)
        if on_device:
            import torch
            flat = a.reshape(-1) if isinstance(a, torch.Tensor) and a.is_contiguous() else a
            check_device_array(label, flat, flat.numel() if isinstance(flat, torch.Tensor) else 0, device, who=who)
        else:
            a = np.array(a, dtype=np.float64, order="C")
        if a.ndim != 2:
            raise ValueError(f"{who}: {label} has shape {tuple(a.shape)}, expected (k, {int(length)}): one row per "
                             "column of the batch")
        if a.shape[1] != int(length):
            raise ValueError(f"{who}: {label} has shape {tuple(a.shape)}, expected (k, {int(length)})")
        if a.shape[0] == 0:
            raise ValueError(f"{who}: {label} holds k = 0 columns; a batch holds at least one")
        if k is None:
            k, first = int(a.shape[0]), label
        elif int(a.shape[0]) != k:
            raise ValueError(f"{who}: {label} holds k = {int(a.shape[0])} columns, {first} holds {k}")
        given[name] = a
    if not given:
        raise ValueError(f"{who}: no block given; pass at least one of "
                         f"{', '.join(labels.get(n, n) for n in sizes)}")
    return k, given


JACOBIAN_BATCHES = 8   # Jacobian columns per library call, in units of sens_batch_cols(): bounds the unit blocks


def check_jacobian_selection(sel, sizes: dict, what: str, who: str = "jacobian") -> dict:
    """The `outputs` / `wrt` argument of MPCSolver.jacobian: an iterable of names out of `sizes`, or a dict
    name -> index array (None: every coordinate).  Returns {name: int64 index array} in the order given.
    TypeError for a bare string, ValueError for an unknown name, an empty selection, an index array that is not
    1-D or an index out of range."""
    if isinstance(sel, str):
        raise TypeError(f"{who}: {what} must be a collection of names or a dict name -> indices, not the string "
                        f"{sel!r}")
    items = list(sel.items()) if isinstance(sel, dict) else [(k, None) for k in sel]
    if not items:
        raise ValueError(f"{who}: {what} is empty")
    out = {}
    for name, idx in items:
        if name not in sizes:
            raise ValueError(f"{who}: unknown name {name!r} in {what}; the blocks are {list(sizes)}")
        if name in out:
            raise ValueError(f"{who}: {name!r} appears twice in {what}")
        n = int(sizes[name])
        if idx is None:
            idx = np.arange(n, dtype=np.int64)
        else:
            idx = np.array(idx.cpu() if hasattr(idx, "cpu") else idx)
            if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
                raise ValueError(f"{who}: the indices of {name!r} in {what} must be a 1-D integer array")
            idx = idx.astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= n):
                raise ValueError(f"{who}: an index of {name!r} in {what} is outside [0, {n})")
        out[name] = idx
    return out


def jacobian_mode(mode, n_parameters: int, n_outputs: int, who: str = "jacobian") -> str:
    """"forward" (one tangent column per selected parameter) or "reverse" (one adjoint column per selected
    output coordinate); None picks the one with fewer columns, forward on a tie."""
    if mode is None:
        return "forward" if n_parameters <= n_outputs else "reverse"
    if mode not in ("forward", "reverse"):
        raise ValueError(f"{who}: mode must be None, 'forward' or 'reverse', not {mode!r}")
    return mode


POLISH_NAMES = ("x", "y", "zl", "zu", "cons", "active_var", "active_row")   # madipm_polish_out's fields


class PolishVerdict(enum.IntEnum):
    """madipm_polish_info.verdict: the larger number wins."""
    POLISHED = 0
    WRONG_SET = 1
    NO_CONVERGENCE = 2
    FACTORIZATION_FAILED = 3


def check_polish_want(want) -> tuple:
    """The `want` argument of MPCSolver.polish / polish_device: None (all seven) or an iterable of names out of
    POLISH_NAMES.  Returns the names in POLISH_NAMES order; ValueError for an unknown name or an empty
    selection, TypeError for a bare string."""
    if want is None:
        return POLISH_NAMES
    if isinstance(want, str):
        raise TypeError(f"polish: want must be a collection of names, not the string {want!r}")
    want = list(want)
    unknown = [k for k in want if k not in POLISH_NAMES]
    if unknown:
        raise ValueError(f"polish: unknown name(s) {unknown} in want; the blocks are {list(POLISH_NAMES)}")
    if not want:
        raise ValueError("polish: want is empty")
    return tuple(k for k in POLISH_NAMES if k in want)


def check_polish_opts(sigma=None, tol_resid=None, tol_sign=None, tol_feas=None, refine_steps=None) -> tuple:
    """The options of MPCSolver.polish / polish_device, before any library call; None is the library's default
    (madipm_polish_default_opts: 1e10, 1e-10, 1e-9, 1e-9, 2).  sigma must be positive and finite, the
    tolerances finite and not negative, refine_steps an integer in 0..8.  Returns the five values in
    madipm_polish_opts' order."""
    d = L.PolishOpts()
    L.lib.madipm_polish_default_opts(C.byref(d))
    sigma = d.sigma if sigma is None else float(sigma)
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError(f"polish: sigma must be positive and finite, got {sigma}")
    tols = []
    for name, v, dv in (("tol_resid", tol_resid, d.tol_resid), ("tol_sign", tol_sign, d.tol_sign),
                        ("tol_feas", tol_feas, d.tol_feas)):
        v = dv if v is None else float(v)
        if not (v >= 0.0 and np.isfinite(v)):
            raise ValueError(f"polish: {name} must be finite and not negative, got {v}")
        tols.append(v)
    if refine_steps is None:
        refine_steps = d.refine_steps
    if isinstance(refine_steps, bool) or not isinstance(refine_steps, (int, np.integer)):
        raise TypeError(f"polish: refine_steps must be an integer, not {type(refine_steps).__name__}")
    if not 0 <= int(refine_steps) <= 8:
        raise ValueError(f"polish: refine_steps must be in 0..8, got {int(refine_steps)}")
    return (sigma, *tols, int(refine_steps))


def check_polish_set(nvar: int, ncon: int, active_var=None, active_row=None, *, on_device: bool = False,
                     device=None) -> tuple:
    """The supplied active set of MPCSolver.polish / polish_device, before any library call: both None (the
    guess: returns ()) or both given, of shapes (nvar,) and (ncon,).  Host route: integer arrays with values
    that fit int8, converted to C-contiguous int8.  Device route (on_device): contiguous torch.int8 tensors on
    the GPU (on `device` when given).  Which codes a variable or a row may carry is the library's check."""
    who = "polish_device" if on_device else "polish"
    if active_var is None and active_row is None:
        return ()
    if active_var is None or active_row is None:
        raise ValueError(f"{who}: active_var and active_row go together; pass both, or neither for the guess")
    out = []
    for name, a, length in (("active_var", active_var, nvar), ("active_row", active_row, ncon)):
        if on_device:
            import torch
            if not isinstance(a, torch.Tensor):
                raise TypeError(f"{who}: {name} must be a torch tensor on the GPU, not {type(a).__name__}")
            if a.dtype != torch.int8:
                raise TypeError(f"{who}: {name} has dtype {a.dtype}, expected torch.int8")
            if not a.is_contiguous():
                raise ValueError(f"{who}: {name} is not contiguous")
            if a.device.type != "cuda":
                raise TypeError(f"{who}: {name} is on {a.device}, expected a GPU tensor")
            if device is not None and a.device != device:
                raise TypeError(f"{who}: {name} is on {a.device}, the solver is on {device}")
            if tuple(a.shape) != (int(length),):
                raise ValueError(f"{who}: {name} has shape {tuple(a.shape)}, expected ({int(length)},)")
        else:
            a = np.array(a, ndmin=1)
            if a.size and a.dtype.kind not in "iu":
                raise TypeError(f"{who}: {name} has dtype {a.dtype}, expected integers (-1, 0, +1)")
            if a.shape != (int(length),):
                raise ValueError(f"{who}: {name} has shape {a.shape}, expected ({int(length)},)")
            if a.size and (a.min() < -128 or a.max() > 127):
                raise ValueError(f"{who}: {name} has a value that does not fit int8")
            a = np.ascontiguousarray(a, dtype=np.int8)
        out.append(a)
    return tuple(out)


def _polish_info_dict(info) -> dict:
    v = int(info.verdict)
    return {"verdict": PolishVerdict(v) if v >= 0 else None, "n_active": int(info.n_active),
            "residual": float(info.residual), "min_multiplier": float(info.min_multiplier),
            "min_gap": float(info.min_gap), "n_polishes": int(info.n_polishes),
            "n_polish_factorizations": int(info.n_polish_factorizations)}


def check_active_set_opts(max_rounds=None, sigma=None, tol_resid=None, tol_sign=None, tol_feas=None,
                          refine_steps=None) -> tuple:
    """The options of MPCSolver.active_set_solve / active_set_solve_device, before any library call: the
    polish's (check_polish_opts) and max_rounds, an integer in 1..16 (None: madipm_active_set_default_opts'
    4).  Returns (the five polish values, max_rounds)."""
    opts = check_polish_opts(sigma, tol_resid, tol_sign, tol_feas, refine_steps)
    if max_rounds is None:
        d = L.ActiveSetOpts()
        L.lib.madipm_active_set_default_opts(C.byref(d))
        max_rounds = d.max_rounds
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)):
        raise TypeError(f"active_set_solve: max_rounds must be an integer, not {type(max_rounds).__name__}")
    if not 1 <= int(max_rounds) <= 16:
        raise ValueError(f"active_set_solve: max_rounds must be in 1..16, got {int(max_rounds)}")
    return opts, int(max_rounds)


def _active_set_info_dict(info) -> dict:
    v = int(info.verdict)
    return {"verdict": PolishVerdict(v) if v >= 0 else None, "rounds": int(info.rounds),
            "n_active": int(info.n_active), "n_changed": int(info.n_changed), "residual": float(info.residual),
            "min_multiplier": float(info.min_multiplier), "min_gap": float(info.min_gap),
            "n_calls": int(info.n_calls), "n_factorizations": int(info.n_factorizations)}


def _active_set_result(buf: dict, size: dict, names, info) -> dict:
    """The blocks of an active-set solve: the five point blocks are None unless the verdict is POLISHED (the
    library did not write them); the set is the last one tried."""
    ok = int(info.verdict) == PolishVerdict.POLISHED
    res = {k: (buf[k][:size[k]] if ok or _is_code(k) else None) for k in names}
    res["info"] = _active_set_info_dict(info)
    return res


def check_layer_outputs(outputs) -> tuple:
    """The `outputs` argument of QPLayer: an ordered selection out of COTANGENT_NAMES without repeats.
    Returns it as a tuple; TypeError for a bare string, ValueError for an unknown or repeated name or an
    empty selection."""
    if isinstance(outputs, str):
        raise TypeError(f"QPLayer: outputs must be a collection of names, not the string {outputs!r}")
    outputs = tuple(outputs)
    unknown = [k for k in outputs if k not in COTANGENT_NAMES]
    if unknown:
        raise ValueError(f"QPLayer: unknown name(s) {unknown} in outputs; the blocks are {list(COTANGENT_NAMES)}")
    if len(set(outputs)) != len(outputs):
        raise ValueError(f"QPLayer: a name is repeated in outputs {list(outputs)}")
    if not outputs:
        raise ValueError("QPLayer: outputs is empty")
    return outputs


class RCCLComm:
    """RCCL communicator of the sharded factorisation (one process per GPU; madipm_comm_*).

    `RCCLComm.from_torch(dist)` makes rank 0's 128-byte unique id, broadcasts it with the
    torch.distributed process group (any backend), and joins the communicator."""

    def __init__(self, rank: int, size: int, uid: bytes):
        assert len(uid) == 128
        self.rank, self.size = int(rank), int(size)
        h = L.vp()
        L.check(L.lib.madipm_comm_create(self.size, self.rank, uid, C.byref(h)), "madipm_comm_create")
        self.h = h

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        L.check(L.lib.madipm_comm_unique_id(buf), "madipm_comm_unique_id")
        return buf.raw

    @classmethod
    def from_torch(cls, dist) -> "RCCLComm":
        rank, size = dist.get_rank(), dist.get_world_size()
        box = [cls.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        return cls(rank, size, box[0])

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            L.lib.madipm_comm_destroy(h)
            self.h = None


class HostComm:
    """Host-staged communicator over a torch.distributed process group (e.g. gloo): every all-reduce
    goes device -> pinned host -> dist.all_reduce -> device.  For exercising the multi-process
    sharded path where RCCL cannot run (several ranks on one GPU); RCCLComm is the data path."""

    def __init__(self, dist):
        import torch
        self.rank, self.size = dist.get_rank(), dist.get_world_size()

        def _fn(p, n, _ctx):
            try:
                a = np.ctypeslib.as_array(p, shape=(int(n),))
                t = torch.from_numpy(a)
                dist.all_reduce(t)
                return 0
            except Exception:  # pragma: no cover - reported as a C error
                return -1
        self._cb = L.ALLREDUCE_FN(_fn)
        h = L.vp()
        L.check(L.lib.madipm_comm_create_host(self.size, self.rank, self._cb, None, C.byref(h)), "madipm_comm_create_host")
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            L.lib.madipm_comm_destroy(h)
            self.h = None


@dataclass
class Counters:
    """MadNLP.MadNLPCounters subset reported by the reference benchmarks (scripts/benchmarks_cpu.jl:49-50)."""
    k: int = 0
    total_time: float = 0.0
    linear_solver_time: float = 0.0
    init_time: float = 0.0


@dataclass
class ExecutionStats:
    """MadNLP.MadNLPExecutionStats as filled by update_solution! (src/utils.jl:150-156)."""
    status: int
    iter: int
    objective: float
    dual_objective: float
    solution: np.ndarray
    constraints: np.ndarray
    multipliers: np.ndarray
    multipliers_L: np.ndarray
    multipliers_U: np.ndarray
    primal_feas: float
    dual_feas: float
    inf_compl: float
    counters: Counters
    trace: list = field(default_factory=list)

    @property
    def status_name(self) -> str:
        return STATUS_NAMES.get(self.status, str(self.status))


_KNOWN = {"tol", "max_iter", "max_wall_time", "divergence_tol", "scaling", "bound_push", "bound_fac",
          "bound_relax_factor", "regularization", "step_rule", "barrier_update", "max_ncorr", "mu_init",
          "mu_min", "tol_linear_solve", "check_residual", "kkt_system", "linear_solver", "print_level",
          "rethrow_error", "ordering", "relax", "pivot_tol", "small_front_max", "dense_alpha",
          "output_file", "file_print_level", "kappa_d", "s_max", "mu_superlinear_decrease_power", "tau_min",
          "fixed_variable_treatment", "equality_treatment", "nshards", "comm"}


def load_options(**kw) -> Options:
    """load_options (src/utils.jl:121-148): IPM options + linear-solver options."""
    unknown = set(kw) - _KNOWN
    if unknown:
        # MadNLP.print_ignored_options (src/utils.jl:140-142): unsupported options are reported, not fatal
        import sys
        print("The following options are ignored: " + ", ".join(f"{k} = {kw[k]!r}" for k in sorted(unknown)),
              file=sys.stderr)
    o = Options()
    L.lib.madipm_default_options(C.byref(o))
    for k in ("tol", "max_iter", "max_wall_time", "divergence_tol", "bound_push", "bound_fac",
              "bound_relax_factor", "max_ncorr", "mu_init", "mu_min", "tol_linear_solve"):
        if k in kw:
            setattr(o, k, kw[k])
    if "scaling" in kw:
        o.scaling = int(bool(kw["scaling"]))
    if "check_residual" in kw:
        o.check_residual = int(bool(kw["check_residual"]))
    reg = kw.get("regularization", FixedRegularization(1e-10, 1e-10))
    if isinstance(reg, NoRegularization):
        o.regularization = 0
    elif isinstance(reg, FixedRegularization):
        o.regularization, o.delta_p, o.delta_d = 1, reg.delta_p, reg.delta_d
    elif isinstance(reg, AdaptiveRegularization):
        o.regularization, o.delta_p, o.delta_d, o.delta_min = 2, reg.delta_p, reg.delta_d, reg.delta_min
    else:
        raise TypeError(f"unsupported regularization {reg!r}")
    rule = kw.get("step_rule", AdaptiveStep(0.99))
    if isinstance(rule, ConservativeStep):
        o.step_rule, o.step_tau = 0, rule.tau
    elif isinstance(rule, AdaptiveStep):
        o.step_rule, o.step_tau = 1, rule.tau_min
    elif isinstance(rule, MehrotraAdaptiveStep):
        o.step_rule, o.step_tau = 2, rule.gamma_f
    else:
        raise TypeError(f"unsupported step rule {rule!r}")
    kkt = kw.get("kkt_system", SparseKKTSystem)
    if kkt not in _KKT_CODES:
        raise TypeError(f"unsupported kkt_system {getattr(kkt, '__name__', kkt)!r}")
    o.kkt_system = _KKT_CODES[kkt]
    ls = kw.get("linear_solver", HIPLDLSolver)
    if ls is not HIPLDLSolver:
        raise NotImplementedError("linear_solver must be HIPLDLSolver (the GPU LDL^T)")
    o.print_level = int(kw.get("print_level", 0))
    for k in ("ordering", "relax", "small_front_max", "nshards"):
        if k in kw:
            setattr(o.ldl, k, int(kw[k]))
    for k in ("pivot_tol", "dense_alpha"):
        if k in kw:
            setattr(o.ldl, k, float(kw[k]))
    return o


def _is_code(name: str) -> bool:
    return name.startswith("active")   # the polish's set: int8 codes; every other block is float64


def _host_outputs(struct, size: dict, names) -> dict:
    """Host route of adjoint / tangent / polish: one numpy buffer per wanted output (an empty output still has
    a non-null address), its address in the C struct's field of the same name."""
    buf = {k: np.empty(max(size[k], 1), np.int8 if _is_code(k) else np.float64) for k in names}
    for k in names:
        setattr(struct, k, L.ptr(buf[k], C.c_int8 if _is_code(k) else C.c_double))
    return buf


def _host_inputs(given: dict) -> dict:
    """Addresses of the given host blocks.  An empty block (ncon = 0, nnzh = 0) has nothing to read: any
    non-null address says "given"."""
    return {k: L.ptr(a if a.size else np.zeros(1, a.dtype), C.c_int8 if a.dtype == np.int8 else C.c_double)
            for k, a in given.items()}


class MPCSolver:
    """`MPCSolver(nlp; kwargs...)` (src/structure.jl:79-178) on the GPU."""

    def __init__(self, qp: QuadraticModel, **kwargs):
        self.qp = qp
        self.options = load_options(**kwargs)
        self.rethrow_error = bool(kwargs.get("rethrow_error", False))
        self._keep = []
        self._update_ready = False  # madipm_solver_prepare_update has run (update() calls it on first use)
        self.qp_current = True      # self.qp's value arrays are the solver's (False after update_device)
        self._device = None         # the solver's torch device, looked up by the first device-route call
        self._kept_set = False      # a polish or an active-set solve ended POLISHED: the library keeps its set
        q = QPStruct()
        q.nvar, q.ncon = qp.nvar, qp.ncon
        q.nnzh, q.nnzj = qp.nnzh, qp.nnzj

        def f64(a):
            a = np.ascontiguousarray(a, np.float64)
            self._keep.append(a)
            return L.ptr(a, C.c_double)

        def i32(a):
            a = np.ascontiguousarray(a, np.int32)
            self._keep.append(a)
            return L.ptr(a, C.c_int32)

        q.c, q.c0 = f64(qp.c), float(qp.c0)
        q.Hrows, q.Hcols, q.Hvals = i32(qp.Hrows), i32(qp.Hcols), f64(qp.Hvals)
        q.Arows, q.Acols, q.Avals = i32(qp.Arows), i32(qp.Acols), f64(qp.Avals)
        q.lcon, q.ucon, q.lvar, q.uvar = f64(qp.lcon), f64(qp.ucon), f64(qp.lvar), f64(qp.uvar)
        q.x0, q.y0 = f64(qp.x0), f64(qp.y0)
        q.minimize = int(bool(qp.minimize))
        self._q = q
        h = L.vp()
        comm = kwargs.get("comm")
        if comm is not None and comm.size > 1:
            # subtree-sharded factorisation across the processes of `comm` (SURVEY §8 e)
            self._comm = comm
            L.check(L.lib.madipm_solver_create_dist(C.byref(q), C.byref(self.options), comm.h, C.byref(h)),
                    "MPCSolver")
        else:
            L.check(L.lib.madipm_solver_create(C.byref(q), C.byref(self.options), C.byref(h)), "MPCSolver")
        self.h = h

    def ldl_info(self) -> dict:
        inf = L.LDLInfo()
        L.check(L.lib.madipm_solver_ldl_info(self.h, C.byref(inf)), "ldl_info")
        return inf.as_dict()

    def kkt_perm(self) -> np.ndarray:
        """Pivot order of the K2 LDL^T (analysis output), over the K2 unknowns [x; s; y]."""
        n = self.ldl_info()["n"]
        p = np.empty(n, np.int32)
        L.check(L.lib.madipm_solver_ldl_perm(self.h, L.ptr(p, C.c_int32)), "kkt_perm")
        return p

    def spmv_group(self) -> int:
        """Lanes per row of the MPC loop's SpMV kernels (4..64): the mean-row heuristic's choice, or the
        value forced by MADIPM_SPMV_G at construction."""
        return L.check(L.lib.madipm_solver_spmv_group(self.h), "spmv_group")

    def set_kernel_timing(self, mask: int = (1 << L.NKERNELS) - 1):
        """Record HIP events around every launch of the LDL^T kernel kinds in `mask` (bit k = kind k,
        include/madipm_hip.h); clears the statistics.  mask=0 turns timing off."""
        L.check(L.lib.madipm_solver_set_timing(self.h, int(mask)), "set_timing")

    def kernel_stats(self) -> list:
        """Per kernel kind: launches, summed event time (ms), algorithmic bytes and flops."""
        arr = (L.KStat * L.NKERNELS)()
        L.check(L.lib.madipm_solver_kernel_stats(self.h, arr), "kernel_stats")
        return L.kstats_to_list(arr)

    def initialize(self):
        """initialize! alone (src/solver.jl:127-189); the next solve() runs only the MPC loop."""
        L.check(L.lib.madipm_solver_initialize(self.h), "initialize!")

    def set_max_iter(self, k: int):
        L.check(L.lib.madipm_solver_set_max_iter(self.h, int(k)), "set_max_iter")

    def solve(self, fetch_solution: bool = True) -> ExecutionStats:
        """solve!(solver) (src/solver.jl:362-418).  fetch_solution=False skips update_solution!'s
        device-to-host copies of x, y, z_L, z_U and the constraint values (the reference runs it after
        cnt.total_time is taken, solver.jl:406-413); the returned arrays are then None."""
        st = Stats()
        rc = L.lib.madipm_solver_solve(self.h, C.byref(st))
        if rc < 0:
            # solve!'s catch-all (src/solver.jl:398-403): INTERNAL_ERROR, rethrown only with rethrow_error
            if self.rethrow_error:
                L.check(rc, "solve!")
            st.status = INTERNAL_ERROR
            st.iter = len(self.trace()) - 1 if self.trace() else 0
        elif st.status == INTERNAL_ERROR and st.exception in _EXCEPTIONS and self.rethrow_error:
            raise _EXCEPTIONS[st.exception](
                "MPC loop: " + ("residual check of solve_system! (src/linear_solver.jl:40-41)"
                                if st.exception == EXC_SOLVE else "solve with an unfactorized KKT system"))
        if not fetch_solution:
            return ExecutionStats(status=st.status, iter=st.iter, objective=st.objective,
                                  dual_objective=st.dual_objective, solution=None, constraints=None,
                                  multipliers=None, multipliers_L=None, multipliers_U=None, primal_feas=st.inf_pr,
                                  dual_feas=st.inf_du, inf_compl=st.inf_compl,
                                  counters=Counters(k=st.iter, total_time=st.total_time,
                                                    linear_solver_time=st.linear_solver_time, init_time=st.init_time),
                                  trace=None)
        nx, m = self.qp.nvar, self.qp.ncon
        x, zl, zu = np.empty(nx), np.empty(nx), np.empty(nx)
        y, cons = np.empty(m), np.empty(m)
        rs = L.lib.madipm_solver_get_solution(self.h, L.ptr(x, C.c_double), L.ptr(y, C.c_double),
                                              L.ptr(zl, C.c_double), L.ptr(zu, C.c_double), L.ptr(cons, C.c_double))
        if rs < 0:
            if rc >= 0:
                L.check(rs, "get_solution")
            for a in (x, y, zl, zu, cons):
                a.fill(np.nan)
        return ExecutionStats(status=st.status, iter=st.iter, objective=st.objective,
                              dual_objective=st.dual_objective, solution=x, constraints=cons,
                              multipliers=y, multipliers_L=zl, multipliers_U=zu, primal_feas=st.inf_pr,
                              dual_feas=st.inf_du, inf_compl=st.inf_compl,
                              counters=Counters(k=st.iter, total_time=st.total_time,
                                                linear_solver_time=st.linear_solver_time, init_time=st.init_time),
                              trace=self.trace())

    def update(self, *, c=None, c0=None, Hvals=None, Avals=None, lcon=None, ucon=None, lvar=None, uvar=None,
               x0=None, y0=None):
        """New numbers for the same sparsity pattern: the next solve() runs on the updated problem from its
        x0 / y0, with the ordering, the symbolic factorisation, the device plan and every buffer of this
        solver kept (no re-analysis).  An argument left None keeps the current data; Hvals / Avals are in the
        creation-time COO order.  The classification of every bound is fixed at creation: turning an
        equality row into a ranged one, a fixed variable into a free one, or a finite bound into an infinite
        one (or back) raises MadIPMError and leaves the solver as it was.  self.qp becomes an updated copy;
        the caller's arrays are never modified and are kept alive for the call only."""
        qp = self.qp
        want = {"c": qp.nvar, "Hvals": qp.nnzh, "Avals": qp.nnzj, "lcon": qp.ncon, "ucon": qp.ncon,
                "lvar": qp.nvar, "uvar": qp.nvar, "x0": qp.nvar, "y0": qp.ncon}
        given = {"c": c, "Hvals": Hvals, "Avals": Avals, "lcon": lcon, "ucon": ucon, "lvar": lvar, "uvar": uvar,
                 "x0": x0, "y0": y0}
        u, new = QPUpdate(), {}
        for k, a in given.items():
            if a is None:
                continue
            a = np.array(a, dtype=np.float64, order="C", ndmin=1)  # a copy: self.qp never aliases the caller's
            if a.shape != (want[k],):
                raise ValueError(f"update: {k} has shape {a.shape}, expected ({want[k]},)")
            new[k] = a
            setattr(u, k, L.ptr(a, C.c_double))
        c0v = None
        if c0 is not None:
            c0v = C.c_double(float(c0))
            u.c0 = C.pointer(c0v)
            new["c0"] = float(c0)
        self._prepare_update()
        L.check(L.lib.madipm_solver_update(self.h, C.byref(u)), "update")
        if self.qp_current:
            self.qp = dataclasses.replace(qp, **new)
        else:  # after update_device: the kept fields are the device-installed ones
            self.fetch_qp()

    def _prepare_update(self):
        if not self._update_ready:
            # the refresh plan, once: the creation-time arrays of self._q are alive in self._keep
            L.check(L.lib.madipm_solver_prepare_update(self.h, C.byref(self._q)), "prepare_update")
            self._update_ready = True

    def update_device(self, *, c=None, c0=None, Hvals=None, Avals=None, lcon=None, ucon=None, lvar=None,
                      uvar=None, x0=None, y0=None, stream=None):
        """update() from torch tensors on the solver's GPU (float64, contiguous, the shapes update() expects;
        c0 is a Python number): nothing is copied to the host, and everything update() computes on the host
        is recomputed by kernels, with the same bits.  `stream` is the torch.cuda.Stream the tensors were
        produced on (None: the current stream); the reads are ordered after the work enqueued on it, and the
        call returns with all its reads done, so the tensors may be overwritten right after it.  The same
        changes of classification are refused, with the same message.  self.qp keeps its pattern and
        dimensions, but its value arrays are no longer current (qp_current is False) until fetch_qp().
        As wherever torch pointers or streams are handed to the library, `import torch` comes before this
        package in the process, so that both use one HIP runtime."""
        import torch
        qp = self.qp
        want = {"c": qp.nvar, "Hvals": qp.nnzh, "Avals": qp.nnzj, "lcon": qp.ncon, "ucon": qp.ncon,
                "lvar": qp.nvar, "uvar": qp.nvar, "x0": qp.nvar, "y0": qp.ncon}
        given = {"c": c, "Hvals": Hvals, "Avals": Avals, "lcon": lcon, "ucon": ucon, "lvar": lvar, "uvar": uvar,
                 "x0": x0, "y0": y0}
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        u, keep = QPUpdate(), []
        for k, a in given.items():
            if a is None:
                continue
            check_device_array(k, a, want[k], self._device)
            keep.append(a)
            setattr(u, k, C.cast(a.data_ptr(), L.f64p))  # an empty tensor's null pointer reads as "keep"
        c0v = None
        if c0 is not None:
            c0v = C.c_double(float(c0))
            u.c0 = C.pointer(c0v)
        if stream is not None and not isinstance(stream, torch.cuda.Stream):
            raise TypeError(f"update_device: stream must be a torch.cuda.Stream, not {type(stream).__name__}")
        st = stream if stream is not None else torch.cuda.current_stream(self._device)
        self._prepare_update()
        # labelled as update(): a refused change of classification reads the same on both routes
        L.check(L.lib.madipm_solver_update_device(self.h, C.byref(u), L.vp(st.cuda_stream)), "update")
        self.qp_current = False

    def fetch_qp(self) -> QuadraticModel:
        """The problem the solver currently holds (madipm_solver_get_data), as an updated copy of self.qp;
        self.qp is current again afterwards."""
        qp = self.qp
        self._prepare_update()  # the solver keeps A's values from then on
        new = {"c": np.empty(qp.nvar), "Hvals": np.empty(qp.nnzh), "Avals": np.empty(qp.nnzj),
               "lcon": np.empty(qp.ncon), "ucon": np.empty(qp.ncon), "lvar": np.empty(qp.nvar),
               "uvar": np.empty(qp.nvar), "x0": np.empty(qp.nvar), "y0": np.empty(qp.ncon)}
        c0 = C.c_double()
        p = {k: L.ptr(a, C.c_double) for k, a in new.items()}
        L.check(L.lib.madipm_solver_get_data(self.h, p["c"], C.byref(c0), p["Hvals"], p["Avals"], p["lcon"],
                                             p["ucon"], p["lvar"], p["uvar"], p["x0"], p["y0"]), "get_data")
        self.qp = dataclasses.replace(qp, c0=float(c0.value), **new)
        self.qp_current = True
        return self.qp

    def solution_device(self, stream=None) -> dict:
        """update_solution! into torch tensors on the GPU (madipm_solver_get_solution_device): the bits
        solve() returns in host arrays, without a copy through the host and without blocking it.  Work
        enqueued on `stream` (None: the current stream) afterwards sees the values."""
        import torch
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        if stream is not None and not isinstance(stream, torch.cuda.Stream):
            raise TypeError(f"solution_device: stream must be a torch.cuda.Stream, not {type(stream).__name__}")
        st = stream if stream is not None else torch.cuda.current_stream(self._device)
        nx, m = self.qp.nvar, self.qp.ncon
        with torch.cuda.stream(st):
            out = {"solution": torch.empty(nx, dtype=torch.float64, device=self._device),
                   "multipliers": torch.empty(m, dtype=torch.float64, device=self._device),
                   "multipliers_L": torch.empty(nx, dtype=torch.float64, device=self._device),
                   "multipliers_U": torch.empty(nx, dtype=torch.float64, device=self._device),
                   "constraints": torch.empty(m, dtype=torch.float64, device=self._device)}
        dp = {k: C.cast(t.data_ptr(), L.f64p) for k, t in out.items()}
        L.check(L.lib.madipm_solver_get_solution_device(self.h, dp["solution"], dp["multipliers"],
                                                        dp["multipliers_L"], dp["multipliers_U"],
                                                        dp["constraints"], L.vp(st.cuda_stream)),
                "get_solution_device")
        return out

    # ------------------------------------------------------------ warm start
    def warm_start(self, *, x=None, y=None, zl=None, zu=None, weight=0.99):
        """Start the following solves from a point of the public space — what solve() returns as solution,
        multipliers, multipliers_L, multipliers_U (lengths nvar, ncon, nvar, nvar) — instead of the cold
        start alone: initialize! runs unchanged, then every block given here is blended into the cold start,
        weight * warm + (1 - weight) * cold, after x is clamped into the bounds and the multipliers at 0; a
        coordinate that would leave the strict interior keeps its cold value.  A block left None keeps its
        cold values (the slack values follow x, the slack multipliers y).  The point replaces any earlier one
        and stays, across solves and updates, until clear_warm_start().  0 < weight < 1; entries are not
        checked for NaN / inf.  The arrays are read during the call only."""
        want = {"x": self.qp.nvar, "y": self.qp.ncon, "zl": self.qp.nvar, "zu": self.qp.nvar}
        p, keep = {}, []
        for k, a in (("x", x), ("y", y), ("zl", zl), ("zu", zu)):
            if a is None:
                p[k] = None
                continue
            a = np.array(a, dtype=np.float64, order="C", ndmin=1)
            if a.shape != (want[k],):
                raise ValueError(f"warm_start: {k} has shape {a.shape}, expected ({want[k]},)")
            # an empty block (ncon = 0) has nothing to read: any non-null address says "given"
            a = a if a.size else np.zeros(1)
            keep.append(a)
            p[k] = L.ptr(a, C.c_double)
        L.check(L.lib.madipm_solver_set_warm_start(self.h, p["x"], p["y"], p["zl"], p["zu"], float(weight)),
                "warm_start")

    def warm_start_device(self, *, x=None, y=None, zl=None, zu=None, weight=0.99, stream=None):
        """warm_start() from torch tensors on the solver's GPU (float64, contiguous, the shapes warm_start()
        expects), without a copy through the host.  `stream` is the torch.cuda.Stream the tensors were
        produced on (None: the current stream): the reads are ordered after the work enqueued on it, the
        host is not blocked, and work enqueued on it after the call is ordered after the copies, so the
        tensors may be overwritten from that stream right away."""
        import torch
        want = {"x": self.qp.nvar, "y": self.qp.ncon, "zl": self.qp.nvar, "zu": self.qp.nvar}
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        p, keep = {}, []
        for k, a in (("x", x), ("y", y), ("zl", zl), ("zu", zu)):
            if a is None:
                p[k] = None
                continue
            check_device_array(k, a, want[k], self._device)
            if a.numel() == 0:
                a = torch.zeros(1, dtype=torch.float64, device=self._device)
            keep.append(a)
            p[k] = C.cast(a.data_ptr(), L.f64p)
        if stream is not None and not isinstance(stream, torch.cuda.Stream):
            raise TypeError(f"warm_start_device: stream must be a torch.cuda.Stream, not {type(stream).__name__}")
        st = stream if stream is not None else torch.cuda.current_stream(self._device)
        L.check(L.lib.madipm_solver_set_warm_start_device(self.h, p["x"], p["y"], p["zl"], p["zu"], float(weight),
                                                          L.vp(st.cuda_stream)), "warm_start_device")

    def warm_start_last(self, weight=0.99):
        """The solver's own current iterate (the bits solution_device() would return now) as the warm point,
        without leaving the GPU.  In a re-solve loop: solve() -> warm_start_last() -> update_device() ->
        solve(), i.e. before the update, so that the solution is un-scaled with the scaling it was computed
        in.  MadIPMError before the first solve."""
        L.check(L.lib.madipm_solver_warm_start_last(self.h, float(weight)), "warm_start_last")

    def clear_warm_start(self):
        """Back to cold starts: the next solve() is bit for bit the one of a solver that never set a point."""
        L.check(L.lib.madipm_solver_clear_warm_start(self.h), "clear_warm_start")

    def warm_info(self) -> dict:
        """active: a warm point is set; weight: its weight (0.0 when none); n_warm_inits: initialisations of
        this solver that blended a warm point."""
        a, w, k = C.c_int32(), C.c_double(), C.c_int64()
        L.check(L.lib.madipm_solver_warm_info(self.h, C.byref(a), C.byref(w), C.byref(k)), "warm_info")
        return {"active": bool(a.value), "weight": float(w.value), "n_warm_inits": int(k.value)}

    # ------------------------------------------------------------ what the post-solve device calls share
    def _device_call(self, who, stream, recheck, struct, size, names, given):
        """`stream` validated; the device resolved (a solver that had none yet: recheck() repeats the argument
        check against it); on the stream, one tensor per wanted output (an empty output still has a non-null
        address), its address in the C struct's field of the same name, and every given block kept alive, an
        empty one as one element.  Returns the stream, the outputs, the given blocks' addresses and the blocks
        themselves, which the caller holds until the library call has returned."""
        import torch
        if stream is not None and not isinstance(stream, torch.cuda.Stream):
            raise TypeError(f"{who}: stream must be a torch.cuda.Stream, not {type(stream).__name__}")
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
            recheck()
        st = stream if stream is not None else torch.cuda.current_stream(self._device)
        with torch.cuda.stream(st):
            buf = {k: torch.empty(max(size[k], 1), dtype=torch.int8 if _is_code(k) else torch.float64,
                                  device=self._device) for k in names}
            keep = {k: a if a.numel() else torch.zeros(1, dtype=a.dtype, device=self._device)
                    for k, a in given.items()}
        for k in names:
            setattr(struct, k, C.cast(buf[k].data_ptr(), L.i8p if _is_code(k) else L.f64p))
        p = {k: C.cast(a.data_ptr(), L.i8p if a.dtype == torch.int8 else L.f64p) for k, a in keep.items()}
        return st, buf, p, keep

    # ------------------------------------------------------------ adjoint gradients
    def _adjoint_sizes(self) -> dict:
        qp = self.qp
        return {"c": qp.nvar, "Hvals": qp.nnzh, "Avals": qp.nnzj, "lcon": qp.ncon, "ucon": qp.ncon,
                "lvar": qp.nvar, "uvar": qp.nvar}

    def _adjoint_prepare(self, names):
        # Avals and Hvals read the index arrays and raw values prepare_update keeps, and so does lvar when a
        # variable is fixed; the other gradients cost nothing per entry of A
        if "Avals" in names or "Hvals" in names or ("lvar" in names and np.any(self.qp.lvar == self.qp.uvar)):
            self._prepare_update()

    def adjoint(self, gx=None, want=None, *, gy=None, gzl=None, gzu=None, gcons=None, polished=False) -> dict:
        """Gradients of a loss l(x*) with respect to the problem data, given gx = dl/dx* (length nvar) at the
        optimum the last solve() returned: a dict of numpy arrays over `want`, a subset of ADJOINT_NAMES
        (None: all seven), Hvals / Avals in the creation-time COO order.  An infinite bound gets 0; a fixed
        variable and an equality row carry their whole derivative in lvar / lcon (uvar / ucon are 0 there).
        The first call after a solve factorises the KKT matrix of the optimum once; further calls on the same
        point reuse the factor.  The solver's state is untouched: the next solve() is what it would have been.
        MadIPMError when the last solve did not succeed, when an update or initialize ran since, for the
        K2.5 / normal-equations formulations and for a solver created with `comm`.

        A loss l(x, y, zl, zu, cons) of everything solve() returns: gy, gzl, gzu and gcons are
        its derivatives with respect to multipliers, multipliers_L, multipliers_U and constraints (= A x),
        lengths ncon, nvar, nvar, ncon; any of the five may be None (0), not all.  Constants, whose
        cotangents are ignored: zl_i / zu_i of a variable without that bound and zl, zu of a fixed variable
        (solve() returns 0 there).  With gx alone the call is the one above, bit for bit.

        polished=True: the gradients at the point the last polish() returned, which must have
        ended POLISHED on this solved point: the exact derivatives of the face's equality-constrained QP.  The
        gradient of an inactive bound is exactly 0 and that of an active one is the whole sensitivity; zl / zu
        of an inactive bound are constants there.  Arguments and checks are the same."""
        names = check_adjoint_want(want)
        given = check_adjoint_cotangents(self.qp.nvar, self.qp.ncon, gx, gy, gzl, gzu, gcons)
        size = self._adjoint_sizes()
        g = L.QPGrad()
        buf = _host_outputs(g, size, names)
        self._adjoint_prepare(names)
        p = _host_inputs(given)
        if polished:
            ct = L.QPCot(**p)
            L.check(L.lib.madipm_solver_adjoint_polished(self.h, C.byref(ct), C.byref(g)), "adjoint")
        elif list(given) == ["x"]:
            L.check(L.lib.madipm_solver_adjoint(self.h, p["x"], C.byref(g)), "adjoint")
        else:
            ct = L.QPCot(**p)
            L.check(L.lib.madipm_solver_adjoint_full(self.h, C.byref(ct), C.byref(g)), "adjoint")
        return {k: buf[k][:size[k]] for k in names}

    def adjoint_device(self, gx=None, want=None, stream=None, *, gy=None, gzl=None, gzu=None, gcons=None,
                       polished=False) -> dict:
        """adjoint() from and into torch tensors on the solver's GPU (every cotangent: float64, contiguous, the
        shape adjoint() expects), without a copy through the host.  `stream` is the torch.cuda.Stream the
        cotangents were produced on (None: the current stream): they are read after the work enqueued on it,
        and work enqueued on it after the call sees the returned tensors.  The arguments are checked before
        any library call.  polished as in adjoint()."""
        names = check_adjoint_want(want)
        nvar, ncon = self.qp.nvar, self.qp.ncon
        given = check_adjoint_cotangents(nvar, ncon, gx, gy, gzl, gzu, gcons, on_device=True, device=self._device,
                                         who="adjoint_device")
        size = self._adjoint_sizes()
        g = L.QPGrad()
        st, buf, p, _alive = self._device_call(
            "adjoint_device", stream, lambda: check_adjoint_cotangents(
                nvar, ncon, gx, gy, gzl, gzu, gcons, on_device=True, device=self._device, who="adjoint_device"),
            g, size, names, given)
        self._adjoint_prepare(names)
        if polished:
            ct = L.QPCot(**p)
            L.check(L.lib.madipm_solver_adjoint_polished_device(self.h, C.byref(ct), C.byref(g),
                                                                L.vp(st.cuda_stream)), "adjoint_device")
        elif list(given) == ["x"]:
            L.check(L.lib.madipm_solver_adjoint_device(self.h, p["x"], C.byref(g), L.vp(st.cuda_stream)),
                    "adjoint_device")
        else:
            ct = L.QPCot(**p)
            L.check(L.lib.madipm_solver_adjoint_full_device(self.h, C.byref(ct), C.byref(g), L.vp(st.cuda_stream)),
                    "adjoint_device")
        return {k: buf[k][:size[k]] for k in names}

    def adjoint_info(self) -> dict:
        """n_adjoints: successful adjoint calls; n_adjoint_factorizations: those that factorised (one per
        solved point); last_residual: the last call's ||g - K a||_inf / max(1, ||g||_inf)."""
        na, nf, r = C.c_int64(), C.c_int64(), C.c_double()
        L.check(L.lib.madipm_solver_adjoint_info(self.h, C.byref(na), C.byref(nf), C.byref(r)), "adjoint_info")
        return {"n_adjoints": int(na.value), "n_adjoint_factorizations": int(nf.value),
                "last_residual": float(r.value)}

    # ------------------------------------------------------------ forward-mode sensitivities
    def tangent(self, want=None, *, c=None, Hvals=None, Avals=None, lcon=None, ucon=None, lvar=None,
                uvar=None, polished=False) -> dict:
        """The directional derivative of the solution the last solve() returned along a direction of the
        problem data: a dict of numpy arrays over `want`, a subset of TANGENT_NAMES (None: all five: x, y,
        zl, zu and cons = A x).  The direction blocks have the data's shapes (Hvals / Avals in the
        creation-time COO order); None is 0, not all seven.  An entry on an infinite bound is not read; a
        fixed variable moves by lvar's entry and an equality row by lcon's (uvar's / ucon's is not read), so
        one array passed as both bounds stays right.  x* + tangent is the first-order prediction of the
        optimum after the data moved by the direction.  The call shares adjoint()'s factor of the point (one
        factorisation serves both) and leaves the solver's state untouched.  MadIPMError as adjoint().

        polished=True: the derivative of the point the last polish() returned, which must have
        ended POLISHED on this solved point: an active variable moves with its bound and an active row's cons
        with the row's bound (copies of the direction), zl / zu of an inactive bound stay exactly 0, and the
        directions of inactive bounds are not read.  Arguments and checks are the same."""
        names = check_tangent_want(want)
        size = self._adjoint_sizes()
        given = check_tangent_directions(size, dict(c=c, Hvals=Hvals, Avals=Avals, lcon=lcon, ucon=ucon, lvar=lvar,
                                                    uvar=uvar))
        osize = self._tangent_sizes()
        o = L.QPTan()
        buf = _host_outputs(o, osize, names)
        self._adjoint_prepare(given)
        d = L.QPDir(**_host_inputs(given))
        fn = L.lib.madipm_solver_tangent_polished if polished else L.lib.madipm_solver_tangent
        L.check(fn(self.h, C.byref(d), C.byref(o)), "tangent")
        return {k: buf[k][:osize[k]] for k in names}

    def _tangent_sizes(self) -> dict:
        qp = self.qp
        return {"x": qp.nvar, "y": qp.ncon, "zl": qp.nvar, "zu": qp.nvar, "cons": qp.ncon}

    def tangent_device(self, want=None, stream=None, *, c=None, Hvals=None, Avals=None, lcon=None, ucon=None,
                       lvar=None, uvar=None, polished=False) -> dict:
        """tangent() from and into torch tensors on the solver's GPU (every direction: float64, contiguous, the
        shape tangent() expects), without a copy through the host.  `stream` is the torch.cuda.Stream the
        directions were produced on (None: the current stream): they are read after the work enqueued on it,
        and work enqueued on it after the call sees the returned tensors.  The arguments are checked before
        any library call.  polished as in tangent()."""
        names = check_tangent_want(want)
        size = self._adjoint_sizes()
        dirs = dict(c=c, Hvals=Hvals, Avals=Avals, lcon=lcon, ucon=ucon, lvar=lvar, uvar=uvar)
        given = check_tangent_directions(size, dirs, on_device=True, device=self._device, who="tangent_device")
        osize = self._tangent_sizes()
        o = L.QPTan()
        st, buf, p, _alive = self._device_call(
            "tangent_device", stream, lambda: check_tangent_directions(
                size, dirs, on_device=True, device=self._device, who="tangent_device"),
            o, osize, names, given)
        self._adjoint_prepare(given)
        d = L.QPDir(**p)
        fn = L.lib.madipm_solver_tangent_polished_device if polished else L.lib.madipm_solver_tangent_device
        L.check(fn(self.h, C.byref(d), C.byref(o), L.vp(st.cuda_stream)), "tangent_device")
        return {k: buf[k][:osize[k]] for k in names}

    def tangent_info(self) -> dict:
        """n_tangents: successful tangent calls; last_residual: the last call's ||r - K w||_inf /
        max(1, ||r||_inf) of the shifted system."""
        nt, r = C.c_int64(), C.c_double()
        L.check(L.lib.madipm_solver_tangent_info(self.h, C.byref(nt), C.byref(r)), "tangent_info")
        return {"n_tangents": int(nt.value), "last_residual": float(r.value)}

    # ------------------------------------------------------------ batched sensitivities
    _COT_LABELS = {"x": "gx", "y": "gy", "zl": "gzl", "zu": "gzu", "cons": "gcons"}

    @staticmethod
    def sens_batch_cols() -> int:
        """W: the columns one chunk of a batched call runs together (a compile-time constant of the library)."""
        return int(L.lib.madipm_sens_batch_cols())

    def sens_batch_info(self) -> dict:
        """n_batches: successful batched calls; n_columns: the columns they held; n_chunks: the chunks of at most
        sens_batch_cols() columns the calls at the interior point ran (a polished batch adds none)."""
        nb, nc, nk = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib.madipm_solver_sens_batch_info(self.h, C.byref(nb), C.byref(nc), C.byref(nk)),
                "sens_batch_info")
        return {"n_batches": int(nb.value), "n_columns": int(nc.value), "n_chunks": int(nk.value)}

    def set_multi_solve(self, on: bool = True):
        """on: tangent_batch / adjoint_batch (and jacobian, QPLayer.jacobian) at the interior point solve every
        chunk of columns with the multi-right-hand-side LDL^T solve, a chunk of one column too.
        A row's bits then do not depend on k; they agree with the single calls' within the formulas' tolerance,
        not bit for bit.  Default off: every bit as before.  tangent() / adjoint() and polished=True calls are
        unchanged either way."""
        L.check(L.lib.madipm_solver_set_multi_solve(self.h, int(bool(on))), "set_multi_solve")

    def multi_solve_info(self) -> dict:
        """HIPLDLSolver.multi_info() of the solver's linear solver: native is 0 where the switch falls back to
        the loop of single solves (sharded, batched-leaf groups); multi_big, n_big_levels, n_big_passes and
        big_bytes say how the route solves its big fronts (MADIPM_MULTI_BIG=0 at construction takes
        them column after column, with the same bits)."""
        inf, big = L.LDLMultiInfo(), L.LDLMultiBigInfo()
        L.check(L.lib.madipm_solver_multi_solve_info(self.h, C.byref(inf)), "multi_solve_info")
        L.check(L.lib.madipm_solver_multi_big_info(self.h, C.byref(big)), "multi_big_info")
        return {**inf.as_dict(), **big.as_dict()}

    def tangent_batch(self, want=None, *, polished=False, c=None, Hvals=None, Avals=None, lcon=None, ucon=None,
                      lvar=None, uvar=None) -> dict:
        """k tangent() calls on one point in one library call: every direction block has shape (k, len) (row j
        is column j's block; None is 0 in every column), and the result is a dict of (k, len) arrays over
        `want`.  Row j of every block is, bit for bit, what tangent() returns for row j of the directions.  The
        columns run in chunks of sens_batch_cols() that share the passes over the KKT operator and the launches
        of everything but the solves; polished=True runs tangent(polished=True) per column inside the library.
        tangent_info() counts k more calls and reports the largest residual of the columns.  ValueError /
        TypeError as check_batch_blocks raises them, before any library call; MadIPMError as tangent()."""
        names = check_tangent_want(want)
        size = self._adjoint_sizes()
        k, given = check_batch_blocks(size, dict(c=c, Hvals=Hvals, Avals=Avals, lcon=lcon, ucon=ucon, lvar=lvar,
                                                 uvar=uvar), who="tangent_batch")
        osize = self._tangent_sizes()
        o = L.QPTan()
        buf = _host_outputs(o, {n: k * osize[n] for n in names}, names)
        self._adjoint_prepare(given)
        d = L.QPDir(**_host_inputs(given))
        L.check(L.lib.madipm_solver_tangent_batch(self.h, k, C.byref(d), C.byref(o), int(bool(polished))),
                "tangent_batch")
        return {n: buf[n][:k * osize[n]].reshape(k, osize[n]) for n in names}

    def tangent_batch_device(self, want=None, stream=None, *, polished=False, c=None, Hvals=None, Avals=None,
                             lcon=None, ucon=None, lvar=None, uvar=None) -> dict:
        """tangent_batch() from and into torch tensors on the solver's GPU (every direction block: float64,
        contiguous, shape (k, len)), with tangent_device()'s stream contract."""
        names = check_tangent_want(want)
        size = self._adjoint_sizes()
        dirs = dict(c=c, Hvals=Hvals, Avals=Avals, lcon=lcon, ucon=ucon, lvar=lvar, uvar=uvar)
        k, given = check_batch_blocks(size, dirs, on_device=True, device=self._device, who="tangent_batch_device")
        osize = self._tangent_sizes()
        o = L.QPTan()
        st, buf, p, _alive = self._device_call(
            "tangent_batch_device", stream, lambda: check_batch_blocks(
                size, dirs, on_device=True, device=self._device, who="tangent_batch_device"),
            o, {n: k * osize[n] for n in names}, names, given)
        self._adjoint_prepare(given)
        d = L.QPDir(**p)
        L.check(L.lib.madipm_solver_tangent_batch_device(self.h, k, C.byref(d), C.byref(o), int(bool(polished)),
                                                         L.vp(st.cuda_stream)), "tangent_batch_device")
        return {n: buf[n][:k * osize[n]].view(k, osize[n]) for n in names}

    def adjoint_batch(self, gx=None, want=None, *, gy=None, gzl=None, gzu=None, gcons=None, polished=False) -> dict:
        """k adjoint() calls on one point in one library call: every cotangent block has shape (k, len) (None is
        0 in every column), and the result is a dict of (k, len) arrays over `want`.  Row j of every gradient
        is, bit for bit, what adjoint() returns for row j of the cotangents: with gx alone the gx-only call's
        bits, with any other block given those of the five-cotangent call for every column.  Chunks, polished,
        counters (adjoint_info()) and errors as tangent_batch()."""
        names = check_adjoint_want(want)
        k, given = check_batch_blocks(self._tangent_sizes(), dict(x=gx, y=gy, zl=gzl, zu=gzu, cons=gcons),
                                      labels=self._COT_LABELS, who="adjoint_batch")
        size = self._adjoint_sizes()
        g = L.QPGrad()
        buf = _host_outputs(g, {n: k * size[n] for n in names}, names)
        self._adjoint_prepare(names)
        ct = L.QPCot(**_host_inputs(given))
        L.check(L.lib.madipm_solver_adjoint_batch(self.h, k, C.byref(ct), C.byref(g), int(bool(polished))),
                "adjoint_batch")
        return {n: buf[n][:k * size[n]].reshape(k, size[n]) for n in names}

    def adjoint_batch_device(self, gx=None, want=None, stream=None, *, gy=None, gzl=None, gzu=None, gcons=None,
                             polished=False) -> dict:
        """adjoint_batch() from and into torch tensors on the solver's GPU (every cotangent block: float64,
        contiguous, shape (k, len)), with adjoint_device()'s stream contract."""
        names = check_adjoint_want(want)
        cots = dict(x=gx, y=gy, zl=gzl, zu=gzu, cons=gcons)
        csize = self._tangent_sizes()
        k, given = check_batch_blocks(csize, cots, labels=self._COT_LABELS, on_device=True, device=self._device,
                                      who="adjoint_batch_device")
        size = self._adjoint_sizes()
        g = L.QPGrad()
        st, buf, p, _alive = self._device_call(
            "adjoint_batch_device", stream, lambda: check_batch_blocks(
                csize, cots, labels=self._COT_LABELS, on_device=True, device=self._device,
                who="adjoint_batch_device"),
            g, {n: k * size[n] for n in names}, names, given)
        self._adjoint_prepare(names)
        ct = L.QPCot(**p)
        L.check(L.lib.madipm_solver_adjoint_batch_device(self.h, k, C.byref(ct), C.byref(g), int(bool(polished)),
                                                         L.vp(st.cuda_stream)), "adjoint_batch_device")
        return {n: buf[n][:k * size[n]].view(k, size[n]) for n in names}

    def _jacobian(self, outputs, wrt, mode, polished, device, stream, who):
        # one batched call per JACOBIAN_BATCHES * W unit columns of one block: forward mode seeds the parameters,
        # reverse mode the output coordinates; the other side's selection is gathered from the returned blocks
        out_sel = check_jacobian_selection(outputs, self._tangent_sizes(), "outputs", who)
        par_sel = check_jacobian_selection(wrt, self._adjoint_sizes(), "wrt", who)
        n_par = sum(len(i) for i in par_sel.values())
        n_out = sum(len(i) for i in out_sel.values())
        mode = jacobian_mode(mode, n_par, n_out, who)
        seeds, reads = (par_sel, out_sel) if mode == "forward" else (out_sel, par_sel)
        seed_size = self._adjoint_sizes() if mode == "forward" else self._tangent_sizes()
        step = JACOBIAN_BATCHES * self.sens_batch_cols()
        if device:
            import torch
            if stream is not None and not isinstance(stream, torch.cuda.Stream):
                raise TypeError(f"{who}: stream must be a torch.cuda.Stream, not {type(stream).__name__}")
            if self._device is None:
                self._device = torch.device("cuda", torch.cuda.current_device())
            dev = self._device
            zeros = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device=dev)   # noqa: E731
            index = lambda i: torch.as_tensor(i, device=dev)                            # noqa: E731
            if stream is not None:     # the unit blocks and the gathers are enqueued where the calls read and write
                with torch.cuda.stream(stream):
                    return self._jacobian(outputs, wrt, mode, polished, True, None, who)
        else:
            zeros = lambda r, c: np.zeros((r, c))   # noqa: E731
            index = lambda i: i                     # noqa: E731
        read_idx = {name: index(i) for name, i in reads.items()}
        J = {(o, p): zeros(len(oi), len(pi)) for o, oi in out_sel.items() for p, pi in par_sel.items()}
        for seed, idx in seeds.items():
            for lo in range(0, len(idx), step):
                part = idx[lo:lo + step]
                E = zeros(len(part), seed_size[seed])
                E[index(np.arange(len(part))), index(part)] = 1.0
                if mode == "forward":
                    call = self.tangent_batch_device if device else self.tangent_batch
                    res = call(want=tuple(reads), polished=polished, **{seed: E})
                    for o in reads:      # row j: d out / d parameter part[j]
                        J[(o, seed)][:, lo:lo + len(part)] = res[o][:, read_idx[o]].T
                else:
                    call = self.adjoint_batch_device if device else self.adjoint_batch
                    res = call(want=tuple(reads), polished=polished, **{self._COT_LABELS[seed]: E})
                    for p in reads:      # row j: d output coordinate part[j] / d parameters
                        J[(seed, p)][lo:lo + len(part), :] = res[p][:, read_idx[p]]
        return J

    def jacobian(self, outputs=("x",), wrt=("c",), *, mode=None, polished=False) -> dict:
        """The Jacobian of solution blocks with respect to data blocks at the point of the last solve():
        {(out, par): array of shape (selected coordinates of out, selected entries of par)}.  `outputs` (names
        out of TANGENT_NAMES) and `wrt` (names out of ADJOINT_NAMES) are tuples of block names, or dicts
        name -> index array that select coordinates (None: all).  mode="forward" feeds unit directions through
        tangent_batch(), one column per selected parameter; mode="reverse" feeds unit cotangents through
        adjoint_batch(), one column per selected output coordinate; None picks the side with fewer columns,
        forward on a tie.  Either way at most 8 sens_batch_cols() columns go into one library call, which
        bounds the memory of the unit blocks.  A forward-mode column is tangent(par=e_i) and a reverse-mode row
        adjoint() of the unit cotangent, bit for bit.  polished and the errors as tangent() / adjoint()."""
        return self._jacobian(outputs, wrt, mode, polished, False, None, "jacobian")

    def jacobian_device(self, outputs=("x",), wrt=("c",), *, mode=None, polished=False, stream=None) -> dict:
        """jacobian() with the unit blocks built and the Jacobian blocks returned as torch tensors on the
        solver's GPU; `stream` as in tangent_device()."""
        return self._jacobian(outputs, wrt, mode, polished, True, stream, "jacobian_device")

    # ------------------------------------------------------------ polish
    def _polish_sizes(self) -> dict:
        qp = self.qp
        return {"x": qp.nvar, "y": qp.ncon, "zl": qp.nvar, "zu": qp.nvar, "cons": qp.ncon, "active_var": qp.nvar,
                "active_row": qp.ncon}

    def polish(self, want=None, *, active_var=None, active_row=None, sigma=None, tol_resid=None, tol_sign=None,
               tol_feas=None, refine_steps=None) -> dict:
        """The exact solution on the active set the last solve()'s end point identifies: active bounds
        attained bitwise, inactive multipliers exactly 0, the KKT conditions at rounding level.  Returns a
        dict over `want`, a subset of POLISH_NAMES (None: all seven: x, y, zl, zu, cons and the set as
        active_var / active_row, int8: -1 lower-active, +1 upper-active, 0 inactive), plus "info": verdict (a
        PolishVerdict), n_active, residual, min_multiplier, min_gap and the two counters.  active_var and
        active_row (both or neither) supply the set instead of the guess.  With a verdict other than POLISHED
        the blocks are solve()'s, bit for bit.  The call overwrites the factor adjoint() / tangent() share (they
        factorise again), and leaves the next solve() untouched.  MadIPMError as adjoint(), and for a code on
        a bound that does not exist, on a fixed variable or on an equality row."""
        names = check_polish_want(want)
        opts = check_polish_opts(sigma, tol_resid, tol_sign, tol_feas, refine_steps)
        size = self._polish_sizes()
        sets = check_polish_set(size["active_var"], size["active_row"], active_var, active_row)
        o = L.PolishOut()
        buf = _host_outputs(o, size, names)
        po = L.PolishOpts(*opts)
        info = L.PolishInfo()
        p = _host_inputs(dict(zip(("active_var", "active_row"), sets)))
        L.check(L.lib.madipm_solver_polish(self.h, C.byref(po), p.get("active_var"), p.get("active_row"), C.byref(o),
                                           C.byref(info)), "polish")
        res = {k: buf[k][:size[k]] for k in names}
        res["info"] = _polish_info_dict(info)
        self._kept_set |= info.verdict == PolishVerdict.POLISHED
        return res

    def polish_device(self, want=None, stream=None, *, active_var=None, active_row=None, sigma=None, tol_resid=None,
                      tol_sign=None, tol_feas=None, refine_steps=None) -> dict:
        """polish() into torch tensors on the solver's GPU (float64; the set's codes int8), without a copy
        through the host; a supplied set is a pair of contiguous int8 tensors on that GPU.  `stream` is the
        torch.cuda.Stream the set was produced on (None: the current stream): it is read after the work
        enqueued on it, and work enqueued on it after the call sees the returned tensors.  "info" is a host
        dict.  The arguments are checked before any library call."""
        names = check_polish_want(want)
        opts = check_polish_opts(sigma, tol_resid, tol_sign, tol_feas, refine_steps)
        size = self._polish_sizes()
        sets = check_polish_set(size["active_var"], size["active_row"], active_var, active_row, on_device=True,
                                device=self._device)
        o = L.PolishOut()
        st, buf, p, _alive = self._device_call(
            "polish_device", stream, lambda: check_polish_set(
                size["active_var"], size["active_row"], active_var, active_row, on_device=True, device=self._device),
            o, size, names, dict(zip(("active_var", "active_row"), sets)))
        po = L.PolishOpts(*opts)
        info = L.PolishInfo()
        L.check(L.lib.madipm_solver_polish_device(self.h, C.byref(po), p.get("active_var"), p.get("active_row"),
                                                  C.byref(o), C.byref(info), L.vp(st.cuda_stream)), "polish_device")
        res = {k: buf[k][:size[k]] for k in names}
        res["info"] = _polish_info_dict(info)
        self._kept_set |= info.verdict == PolishVerdict.POLISHED
        return res

    # ------------------------------------------------------------ active-set solve
    def active_set_solve(self, want=None, *, active_var=None, active_row=None, max_rounds=None, sigma=None,
                         tol_resid=None, tol_sign=None, tol_feas=None, refine_steps=None) -> dict:
        """The exact solution of the problem the solver holds (after update(), or on a fresh solver) from a
        starting active set, without the interior-point method: up to max_rounds (None: 4) rounds of the
        polish's factor, solves and verdict from a start that reads nothing of the iterate, the set repaired
        between them from the violations found.  active_var / active_row (both or neither) are the starting
        set; neither: the kept set, the codes of the last polish() or active-set solve on this solver that
        ended POLISHED.  Returns a dict over `want` as polish() does; with a verdict other than POLISHED the
        five point blocks are None and active_var / active_row the last set tried.  "info": verdict (a
        PolishVerdict), rounds, n_active, n_changed, residual, min_multiplier, min_gap, n_calls,
        n_factorizations.  A POLISHED call makes its point the one adjoint(polished=True) and
        tangent(polished=True) differentiate; solve() is untouched.  The arguments are checked before any
        library call."""
        names = check_polish_want(want)
        opts, rounds = check_active_set_opts(max_rounds, sigma, tol_resid, tol_sign, tol_feas, refine_steps)
        size = self._polish_sizes()
        sets = check_polish_set(size["active_var"], size["active_row"], active_var, active_row)
        o = L.PolishOut()
        buf = _host_outputs(o, size, names)
        ao = L.ActiveSetOpts(L.PolishOpts(*opts), rounds)
        info = L.ActiveSetInfo()
        p = _host_inputs(dict(zip(("active_var", "active_row"), sets)))
        L.check(L.lib.madipm_solver_active_set_solve(self.h, C.byref(ao), p.get("active_var"), p.get("active_row"),
                                                     C.byref(o), C.byref(info)), "active_set_solve")
        self._kept_set |= info.verdict == PolishVerdict.POLISHED
        return _active_set_result(buf, size, names, info)

    def active_set_solve_device(self, want=None, stream=None, *, active_var=None, active_row=None, max_rounds=None,
                                sigma=None, tol_resid=None, tol_sign=None, tol_feas=None, refine_steps=None) -> dict:
        """active_set_solve() into torch tensors on the solver's GPU, with polish_device()'s arguments and
        stream contract; "info" is a host dict.  The arguments are checked before any library call."""
        names = check_polish_want(want)
        opts, rounds = check_active_set_opts(max_rounds, sigma, tol_resid, tol_sign, tol_feas, refine_steps)
        size = self._polish_sizes()
        sets = check_polish_set(size["active_var"], size["active_row"], active_var, active_row, on_device=True,
                                device=self._device)
        o = L.PolishOut()
        st, buf, p, _alive = self._device_call(
            "active_set_solve_device", stream, lambda: check_polish_set(
                size["active_var"], size["active_row"], active_var, active_row, on_device=True, device=self._device),
            o, size, names, dict(zip(("active_var", "active_row"), sets)))
        ao = L.ActiveSetOpts(L.PolishOpts(*opts), rounds)
        info = L.ActiveSetInfo()
        L.check(L.lib.madipm_solver_active_set_solve_device(
            self.h, C.byref(ao), p.get("active_var"), p.get("active_row"), C.byref(o), C.byref(info),
            L.vp(st.cuda_stream)), "active_set_solve_device")
        self._kept_set |= info.verdict == PolishVerdict.POLISHED
        return _active_set_result(buf, size, names, info)

    def has_kept_set(self) -> bool:
        """A polish() or an active-set solve on this solver has ended POLISHED, so active_set_solve() can start
        from the set the library kept."""
        return bool(self._kept_set)

    def active_set_info(self) -> dict:
        """The last active-set solve's info (verdict None before the first); no device access."""
        info = L.ActiveSetInfo()
        L.check(L.lib.madipm_solver_active_set_info(self.h, C.byref(info)), "active_set_info")
        return _active_set_info_dict(info)

    def polish_info(self) -> dict:
        """The last polish()'s info (verdict None before the first); no device access."""
        info = L.PolishInfo()
        L.check(L.lib.madipm_solver_polish_info(self.h, C.byref(info)), "polish_info")
        return _polish_info_dict(info)

    def polished_sens_info(self) -> dict:
        """n_tangents / n_adjoints: successful calls with polished=True; n_factorizations: those that rebuilt the
        polish's factor (an adjoint or a tangent had taken it); last_residual: the max-norm of the last call's
        final masked residual (scaled space)."""
        nt, na, nf, r = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        L.check(L.lib.madipm_solver_polished_sens_info(self.h, C.byref(nt), C.byref(na), C.byref(nf), C.byref(r)),
                "polished_sens_info")
        return {"n_tangents": int(nt.value), "n_adjoints": int(na.value), "n_factorizations": int(nf.value),
                "last_residual": float(r.value)}

    def counters(self) -> dict:
        """n_analyses: linear-solver analyses run for this solver (stays 1); n_updates: successful update()
        calls; last_update_s: host wall time of the last one (its stream synchronisation included)."""
        na, nu, t = C.c_int64(), C.c_int64(), C.c_double()
        L.check(L.lib.madipm_solver_counters(self.h, C.byref(na), C.byref(nu), C.byref(t)), "counters")
        return {"n_analyses": int(na.value), "n_updates": int(nu.value), "last_update_s": float(t.value)}

    def trace(self) -> list:
        n = L.check(L.lib.madipm_solver_trace(self.h, None, 0), "trace")
        buf = (IterTrace * max(n, 1))()
        L.lib.madipm_solver_trace(self.h, buf, n)
        return [{k: getattr(buf[i], k) for k, _ in IterTrace._fields_} for i in range(n)]

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            L.lib.madipm_solver_destroy(h)
            self.h = None


def solve(solver: MPCSolver) -> ExecutionStats:
    """`solve!(solver)` as a free function."""
    return solver.solve()


def madipm(qp: QuadraticModel, **kwargs) -> ExecutionStats:
    """`madipm(m; kwargs...)` (src/solver.jl:425-428)."""
    return MPCSolver(qp, **kwargs).solve()
