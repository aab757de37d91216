"""bench.py's timed leg on the GPU at a small size (the ex10 stand-in scaled by 0.05): --steps sets the
number of timed iterations even past optimality, and --dump-outputs writes the point the last timed
solve left, which a replay of that solve returns again."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("solution", "multipliers", "multipliers_L", "multipliers_U", "constraints")


def test_timed_steps_and_dumped_outputs(tmp_path):
    import bench
    out = str(tmp_path / "dump")
    steps = 40
    leg, solver, qp = bench.run_leg("ex10@0.05", steps, 2, opt=True, dump=out)
    n_opt = leg["iters_to_opt"]  # the iterations one solve takes: every timed solve but the last ran as many
    assert leg["status"] == "SOLVE_SUCCEEDED" and 4 < n_opt < steps
    solves, last = -(-steps // n_opt), steps - n_opt * ((steps - 1) // n_opt)
    assert leg["steps"] == steps and leg["iters_timed"] == steps and leg["timed_solves"] == solves
    assert leg["ms_per_iter"] == pytest.approx(1e3 * leg["per_rank_s"][0] / steps)
    assert 0 < leg["loop_total_time_s"] <= leg["per_rank_s"][0]  # the library's clock sits inside the bench's

    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in FIELDS + ("summary",))
    arrays = {n: np.load(os.path.join(out, n + ".npy")) for n in FIELDS + ("summary",)}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["solution"].shape == (qp.nvar,) and arrays["multipliers"].shape == (qp.ncon,)
    # the replay of the last timed solve (`last` iterations from initialize!) returns the dumped point
    solver.set_max_iter(last)
    st = solver.solve()
    assert st.iter == last == int(arrays["summary"][1]) and st.status == int(arrays["summary"][0])
    assert st.objective == arrays["summary"][2]
    for name in FIELDS:
        np.testing.assert_array_equal(arrays[name], getattr(st, name), err_msg=name)
