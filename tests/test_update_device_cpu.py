"""The device route's entry points and argument checks, without a GPU."""
from __future__ import annotations

import numpy as np
import pytest


def test_device_route_symbols_resolve():
    from madipm_amd import _lib as L
    from madipm_amd import solver  # noqa: F401  (binds the signatures)
    for name in ("madipm_solver_update_device", "madipm_solver_get_solution_device", "madipm_solver_get_data"):
        f = getattr(L.lib, name)
        assert f.argtypes is not None and f.restype is not None, name
    assert L.madipm_version() == 203


def test_python_entry_points_exist():
    from madipm_amd import MPCSolver
    for name in ("update_device", "solution_device", "fetch_qp"):
        assert callable(getattr(MPCSolver, name)), name


def test_argument_checks_are_pure():
    import torch
    from madipm_amd.solver import check_device_array
    with pytest.raises(TypeError):
        check_device_array("c", np.zeros(4), 4)
    with pytest.raises(TypeError):
        check_device_array("c", [0.0] * 4, 4)
    with pytest.raises(TypeError):
        check_device_array("c", torch.zeros(4, dtype=torch.float64), 4)           # a CPU tensor
    with pytest.raises(TypeError):
        check_device_array("c", torch.zeros(4, dtype=torch.float32), 4)
    with pytest.raises(ValueError):
        check_device_array("c", torch.zeros(8, dtype=torch.float64)[::2], 4)      # not contiguous
