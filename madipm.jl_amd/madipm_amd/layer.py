"""The solver as a differentiable torch layer: x*(c, Hvals, Avals, lcon, ucon, lvar, uvar).

    layer = QPLayer(MPCSolver(qp, tol=1e-9))
    x = layer(c=c, lvar=lvar)        # update_device -> solve -> solution_device, all on the GPU
    loss(x).backward()               # adjoint_device: one factorisation + one solve with the LDL^T on the device

    layer = QPLayer(solver, outputs=("x", "y", "cons"))
    x, y, cons = layer(c=c)          # the row multipliers and A x* are differentiable too

Forward and backward stay on the device (MPCSolver.update_device / solution_device / adjoint_device); the
gradients are those of MPCSolver.adjoint, K2 formulation.  Forward-mode autograd
(torch.autograd.forward_ad) goes through MPCSolver.tangent_device; the torch.func transforms
ask a Function for the setup_context form of forward, which QPFunction does not have.

    layer = QPLayer(solver, outputs=("x", "zl"), polish=True)
    x, zl = layer(c=c)               # ... -> solve -> polish_device: the exact point of the active face

With polish=True forward returns the polished point and backward / jvp differentiate it exactly
(adjoint_device / tangent_device with polished=True): what an active-set QP layer gives.

    layer = QPLayer(solver, outputs=("x", "zl"), polish=True, active_set=True)
    x, zl = layer(c=c)               # update_device -> active_set_solve_device from the kept set; the
    layer.last_route                 # interior-point path above when that does not end POLISHED ("active_set" / "ipm")

    J = layer.jacobian(("c", "lcon"))  # {(out, par): tensor} at the last forward's point, from batched
                                       # tangents or adjoints, whichever needs fewer columns

`import torch` comes before this package in the process, as for every device-route call.
"""
from __future__ import annotations

import torch

from .solver import (ADJOINT_NAMES, SOLVE_SUCCEEDED, STATUS_NAMES, MadIPMError, PolishVerdict,
                     check_layer_outputs)

# output name -> (key of MPCSolver.solution_device(), cotangent keyword of MPCSolver.adjoint_device())
_OUTPUTS = {"x": ("solution", "gx"), "y": ("multipliers", "gy"), "zl": ("multipliers_L", "gzl"),
            "zu": ("multipliers_U", "gzu"), "cons": ("constraints", "gcons")}


class QPFunction(torch.autograd.Function):
    """forward(solver, c, Hvals, Avals, lcon, ucon, lvar, uvar) -> x; a tensor left None keeps the solver's
    current data.  backward asks adjoint_device for exactly the gradients of the tensors that require grad,
    and must run before the solver is updated or solved again (the adjoint belongs to the last solve).
    A tuple of names from ("x", "y", "zl", "zu", "cons") as a ninth argument selects the outputs: forward then
    returns that tuple of tensors, and backward passes on the cotangents of those the loss used.
    jvp hands tangent_device the tangents of the data tensors that carry one and returns the tangents of the
    selected outputs; like backward it must run before the solver is updated or solved again,
    which forward-mode autograd does by calling it right after forward.
    True as a tenth argument (the ninth may be None) polishes: forward returns polish_device's blocks and raises
    MadIPMError unless the verdict is POLISHED, backward and jvp pass polished=True.
    A QPLayer as an eleventh argument (with the polish) tries the active-set solve first: after
    update_device, when the solver keeps a set, active_set_solve_device from it; POLISHED returns its blocks,
    anything else goes on with the solve and the polish as without it.  The layer's last_route says which."""

    @staticmethod
    def forward(ctx, solver, *data):
        outputs, polish, layer = None, False, None
        if len(data) > len(ADJOINT_NAMES) + 2:
            layer = data[len(ADJOINT_NAMES) + 2]
        if len(data) > len(ADJOINT_NAMES) + 1:
            polish = bool(data[len(ADJOINT_NAMES) + 1])
        if len(data) > len(ADJOINT_NAMES):
            data, outputs = data[:len(ADJOINT_NAMES)], data[len(ADJOINT_NAMES)]
        given = {k: t.detach() for k, t in zip(ADJOINT_NAMES, data) if t is not None}
        if given:
            solver.update_device(**given)
        if layer is not None:
            layer.last_route = "ipm"
            if polish and solver.has_kept_set():
                res = solver.active_set_solve_device(want=("x",) if outputs is None else outputs)
                if res["info"]["verdict"] == PolishVerdict.POLISHED:
                    layer.last_route = "active_set"
                    ctx.solver = solver
                    ctx.names = ADJOINT_NAMES
                    ctx.outputs = outputs
                    ctx.sens = {"polished": True}
                    if outputs is None:
                        return res["x"]
                    ctx.set_materialize_grads(False)
                    return tuple(res[k] for k in outputs)
        st = solver.solve(fetch_solution=False)
        if st.status != SOLVE_SUCCEEDED:
            raise MadIPMError(f"QPLayer: the solve ended with status {STATUS_NAMES.get(st.status, st.status)}, "
                              "not SOLVE_SUCCEEDED: no solution to differentiate")
        ctx.solver = solver
        ctx.names = ADJOINT_NAMES
        ctx.outputs = outputs
        ctx.sens = {"polished": True} if polish else {}   # no keyword at all without the polish: today's calls
        if polish:
            pol = solver.polish_device(want=("x",) if outputs is None else outputs)
            verdict = pol["info"]["verdict"]
            if verdict != PolishVerdict.POLISHED:
                raise MadIPMError(f"QPLayer: the polish ended with verdict {PolishVerdict(verdict).name}, not "
                                  "POLISHED: the face has no unique derivative")
            if outputs is None:
                return pol["x"]
            ctx.set_materialize_grads(False)
            return tuple(pol[k] for k in outputs)
        if outputs is None:
            return solver.solution_device()["solution"]
        ctx.set_materialize_grads(False)   # an output the loss did not use arrives as None and stays absent
        sol = solver.solution_device()
        return tuple(sol[_OUTPUTS[k][0]] for k in outputs)

    @staticmethod
    def backward(ctx, *grads):
        # needs_input_grad[0] is the solver's; one entry per data tensor follows (then the outputs' tuple)
        nin = len(ctx.needs_input_grad)
        want = [k for k, need in zip(ctx.names, ctx.needs_input_grad[1:]) if need]
        if not want:
            return (None,) * nin
        if ctx.outputs is None:
            g = ctx.solver.adjoint_device(grads[0].contiguous(), want=want, **ctx.sens)
        else:
            cot = {_OUTPUTS[k][1]: t.contiguous() for k, t in zip(ctx.outputs, grads) if t is not None}
            if not cot:
                return (None,) * nin
            g = ctx.solver.adjoint_device(cot.pop("gx", None), want=want, **cot, **ctx.sens)
        return ((None,) + tuple(g.get(k) for k in ctx.names) + (None,) * nin)[:nin]

    @staticmethod
    def jvp(ctx, *tangents):
        # forward mode (torch.autograd.forward_ad): tangents[0] is the solver's (None); one
        # entry per data tensor follows, None for a tensor without a tangent (then the outputs' tuple: None)
        d = {k: t.contiguous() for k, t in zip(ctx.names, tangents[1:]) if t is not None}
        keys = ("x",) if ctx.outputs is None else ctx.outputs
        if not d:
            return None if ctx.outputs is None else (None,) * len(keys)
        t = ctx.solver.tangent_device(want=keys, **d, **ctx.sens)
        return t["x"] if ctx.outputs is None else tuple(t[k] for k in keys)


class QPLayer(torch.nn.Module):
    """x* of the solver's problem as a function of its data.  forward's arguments are float64 tensors on the
    solver's GPU with the shapes MPCSolver.update_device expects; an argument left None keeps the solver's
    current numbers.  One tensor may be passed as both bounds of the equality rows (lcon and ucon) or of the
    fixed variables: the whole derivative arrives through the lower one and the upper one adds 0.  Raises
    MadIPMError when the solve does not end with SOLVE_SUCCEEDED.

    outputs: the default ("x",) returns the one tensor x*.  Any other ordered selection out of ("x", "y",
    "zl", "zu", "cons") returns that tuple of MPCSolver.solution_device()'s solution, multipliers,
    multipliers_L, multipliers_U and constraints, all differentiable; backward hands the solver the
    cotangents of the outputs the loss used and no others.  zl / zu of a variable without that bound, and of
    a fixed variable, are constants (0).

    polish=True: forward runs update_device -> solve -> polish_device and returns the polished blocks (active
    bounds attained bitwise, inactive multipliers exactly 0); backward and forward-mode autograd differentiate
    that point exactly.  Raises MadIPMError, naming the verdict, when the polish does not end
    POLISHED: a degenerate face has no unique derivative.  The default is the layer without it, bit for bit.

    active_set=True (needs polish=True): after update_device, when the solver keeps the set of an earlier
    POLISHED polish or active-set solve, forward first runs active_set_solve_device from it and
    returns its blocks when it ends POLISHED: no interior-point solve.  Otherwise the path above runs
    unchanged.  last_route is "active_set" or "ipm" after each forward (None before the first); backward and
    jvp are the polished ones either way."""

    def __init__(self, solver, outputs=("x",), polish=False, active_set=False):
        super().__init__()
        self.solver = solver
        self.outputs = check_layer_outputs(outputs)
        self.polish = bool(polish)
        self.active_set = bool(active_set)
        if self.active_set and not self.polish:
            raise ValueError("QPLayer: active_set=True requires polish=True")
        self.last_route = None

    def forward(self, c=None, Hvals=None, Avals=None, lcon=None, ucon=None, lvar=None, uvar=None):
        if self.polish:
            outputs = None if self.outputs == ("x",) else self.outputs
            if self.active_set:
                return QPFunction.apply(self.solver, c, Hvals, Avals, lcon, ucon, lvar, uvar, outputs, True, self)
            return QPFunction.apply(self.solver, c, Hvals, Avals, lcon, ucon, lvar, uvar, outputs, True)
        if self.outputs == ("x",):
            return QPFunction.apply(self.solver, c, Hvals, Avals, lcon, ucon, lvar, uvar)
        return QPFunction.apply(self.solver, c, Hvals, Avals, lcon, ucon, lvar, uvar, self.outputs)

    def jacobian(self, wrt, outputs=None, mode=None):
        """The Jacobian of the layer's outputs (or of `outputs`) with respect to the data blocks `wrt` at the
        point of the last forward: MPCSolver.jacobian_device's dict {(out, par): tensor}, of the polished point
        with polish=True.  Like backward it must run before the solver is updated or solved
        again."""
        return self.solver.jacobian_device(outputs=self.outputs if outputs is None else outputs, wrt=wrt, mode=mode,
                                           polished=self.polish)
