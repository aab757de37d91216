"""The solver as a differentiable torch layer: x*(c, Hvals, Avals, lcon, ucon, lvar, uvar).

    layer = QPLayer(MPCSolver(qp, tol=1e-9))
    x = layer(c=c, lvar=lvar)        # update_device -> solve -> solution_device, all on the GPU
    loss(x).backward()               # adjoint_device: one factorisation + one solve with the LDL^T on the device

Forward and backward stay on the device (MPCSolver.update_device / solution_device / adjoint_device); the
gradients are those of MPCSolver.adjoint: of a loss that depends on x alone, K2 formulation.
`import torch` comes before this package in the process, as for every device-route call.
"""
from __future__ import annotations

import torch

from .solver import ADJOINT_NAMES, SOLVE_SUCCEEDED, STATUS_NAMES, MadIPMError


class QPFunction(torch.autograd.Function):
    """forward(solver, c, Hvals, Avals, lcon, ucon, lvar, uvar) -> x; a tensor left None keeps the solver's
    current data.  backward asks adjoint_device for exactly the gradients of the tensors that require grad,
    and must run before the solver is updated or solved again (the adjoint belongs to the last solve)."""

    @staticmethod
    def forward(ctx, solver, *data):
        given = {k: t.detach() for k, t in zip(ADJOINT_NAMES, data) if t is not None}
        if given:
            solver.update_device(**given)
        st = solver.solve(fetch_solution=False)
        if st.status != SOLVE_SUCCEEDED:
            raise MadIPMError(f"QPLayer: the solve ended with status {STATUS_NAMES.get(st.status, st.status)}, "
                              "not SOLVE_SUCCEEDED: no solution to differentiate")
        ctx.solver = solver
        ctx.names = ADJOINT_NAMES
        return solver.solution_device()["solution"]

    @staticmethod
    def backward(ctx, gx):
        # needs_input_grad[0] is the solver's; one entry per data tensor follows
        want = [k for k, need in zip(ctx.names, ctx.needs_input_grad[1:]) if need]
        if not want:
            return (None,) * (1 + len(ctx.names))
        g = ctx.solver.adjoint_device(gx.contiguous(), want=want)
        return (None,) + tuple(g.get(k) for k in ctx.names)


class QPLayer(torch.nn.Module):
    """x* of the solver's problem as a function of its data.  forward's arguments are float64 tensors on the
    solver's GPU with the shapes MPCSolver.update_device expects; an argument left None keeps the solver's
    current numbers.  One tensor may be passed as both bounds of the equality rows (lcon and ucon) or of the
    fixed variables: the whole derivative arrives through the lower one and the upper one adds 0.  Raises
    MadIPMError when the solve does not end with SOLVE_SUCCEEDED."""

    def __init__(self, solver):
        super().__init__()
        self.solver = solver

    def forward(self, c=None, Hvals=None, Avals=None, lcon=None, ucon=None, lvar=None, uvar=None):
        return QPFunction.apply(self.solver, c, Hvals, Avals, lcon, ucon, lvar, uvar)
