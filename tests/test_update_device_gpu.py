"""MPCSolver.update_device / solution_device / fetch_qp: the re-solve loop without the host.

As in test_update_gpu, the oracle of every test is a freshly constructed MPCSolver on the updated problem,
compared exactly (assert_same: the five vectors, status, iterations, both objectives and the whole trace,
bit for bit): the device route recomputes on the GPU everything the host update computes on the host, with
the host loops' order and rounding."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the library loads: tensors and streams are shared with it

from helpers import box_qp, free_eq_qp, scaled_general  # noqa: E402
from test_update_gpu import VALUE_FIELDS, VECTORS, _kkt, _kw, assert_same, corner_qp, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(v):
    return torch.as_tensor(np.ascontiguousarray(v, np.float64), device="cuda")


def _dvalues(qp, fields=VALUE_FIELDS):
    """qp's value fields as update_device arguments: tensors on the GPU, c0 a number."""
    return {k: (float(qp.c0) if k == "c0" else _dev(getattr(qp, k))) for k in fields}


def _fresh(qp, **kw):
    from madipm_amd import MPCSolver
    return MPCSolver(qp, **kw).solve()


def _same_data(a, b):
    for k in VALUE_FIELDS:
        assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k


# ------------------------------------------------------------------ 1. full device update, every formulation
@pytest.mark.parametrize("minimize", [True, False], ids=["min", "max"])
@pytest.mark.parametrize("kind,kkt", [("lp", "K2"), ("lp", "K25"), ("lp", "normal"), ("qp", "K2"), ("qp", "K25")])
def test_full_device_update_matches_fresh_solver(kind, kkt, minimize):
    from madipm_amd import MPCSolver
    p0 = scaled_general(kind, minimize)
    p1 = perturbed(p0, 101)
    kw = _kw(kkt_system=_kkt(kkt))
    s = MPCSolver(p0, **kw)
    perm, info = s.kkt_perm(), s.ldl_info()
    a0 = s.solve()
    assert s.qp_current
    s.update_device(**_dvalues(p1))
    assert not s.qp_current
    a1 = s.solve()
    assert_same(a1, _fresh(p1, **kw))
    assert not np.array_equal(a1.solution, a0.solution)
    c = s.counters()
    assert c["n_analyses"] == 1 and c["n_updates"] == 1 and c["last_update_s"] > 0.0
    assert np.array_equal(s.kkt_perm(), perm) and s.ldl_info() == info
    got = s.fetch_qp()
    assert s.qp_current and got is s.qp
    _same_data(got, p1)


# ------------------------------------------------------------------ 2. csr_from_coo's corner cases
@pytest.mark.parametrize("fix", [True, False], ids=["fixed_column", "no_fixed"])
def test_duplicates_shuffled_coo_and_fixed_column(fix):
    from madipm_amd import MPCSolver
    p0 = corner_qp(fix)
    p1 = perturbed(p0, 7, rows=False)
    s = MPCSolver(p0, **_kw())
    a0 = s.solve()
    s.update_device(**_dvalues(p1))
    assert_same(s.solve(), _fresh(p1, **_kw()))
    s.update_device(**_dvalues(p0))
    assert_same(s.solve(), a0)
    assert s.counters()["n_analyses"] == 1 and s.counters()["n_updates"] == 2


# ------------------------------------------------------------------ 3. the host sums whose order matters
F1, F2, JX, GROW = 10, 20, 15, 50         # two fixed variables, the free one their cross terms feed, gmax's row


def order_qp(seed=0):
    """3 x 200.  Row 0 is ranged (its slack starts at (A x0)_0) with one entry per column in a shuffled input
    order, among them 1e16, -1e16 and O(1) values, and the fixed column F1 three times (1e3, -1e3, 1e-14).
    H: several entries between the fixed variables F1 and F2 (const_fixed), cross terms from both into
    the free variable JX (gfix), and a row GROW whose scaling gradient mixes 1e13-sized and O(1) terms and
    is the largest (gmax).  Rows 1, 2 are plain equality rows."""
    from madipm_amd.qp import QuadraticModel
    rng = np.random.default_rng(seed)
    m, n = 3, 200
    x0 = rng.uniform(0.5, 1.5, n)
    lvar, uvar = np.zeros(n), np.full(n, 3.0)
    lvar[F1] = uvar[F1] = 0.7
    lvar[F2] = uvar[F2] = 1.3
    v0 = rng.uniform(0.5, 2.0, n)
    v0[3], v0[150] = 1e16, -1e16
    v0[77], v0[120] = 3e15, -3e15
    free0 = [j for j in range(n) if j not in (F1, F2)]
    rows = [0] * len(free0) + [0, 0, 0]
    cols = free0 + [F1, F1, F1]
    vals = [v0[j] for j in free0] + [0.0, 0.0, 0.0]
    for r in (1, 2):
        for j in range(r, n, 2):
            rows.append(r), cols.append(j), vals.append(1.0 + 0.01 * (j % 7))
    order = rng.permutation(len(rows))
    rows, cols, vals = np.array(rows)[order], np.array(cols)[order], np.array(vals)[order]
    # the fixed column's three entries of row 0, wherever the shuffle put them, in this input order:
    # (1e3 x - 1e3 x) + 1e-14 x keeps the small term, every order that adds it earlier loses it
    vals[np.flatnonzero((rows == 0) & (cols == F1))] = [1e3, -1e3, 1e-14]
    hr = list(range(n))
    hc = list(range(n))
    hv = [1.0] * n
    for r, c, v in ((F2, F1, 1e8), (F2, F1, 1.0 / 3.0), (F1, F1, 0.1), (F2, F1, -1e8), (F2, F2, 0.7), (F2, F1, 0.3),
                    (JX, F1, 1e8), (F2, JX, 1.0 / 7.0), (JX, F1, -1e8), (F2, JX, 0.9), (JX, F1, 0.3),
                    (GROW, 30, 1e13), (GROW, 31, 0.1234567), (GROW, 32, -1e13), (GROW, 33, 1.0 / 3.0), (GROW, 34, 1e13),
                    (GROW, 35, 0.7654321), (GROW, 36, -1e13), (60, GROW, 1.0 / 9.0)):
        hr.append(r), hc.append(c), hv.append(v)
    horder = rng.permutation(len(hr))
    hr, hc, hv = np.array(hr)[horder], np.array(hc)[horder], np.array(hv)[horder]
    x0[30], x0[32], x0[34], x0[36], x0[GROW] = 1.5, 0.5, 1.25, 0.75, 0.5
    xs = np.where(lvar == uvar, lvar, rng.uniform(0.5, 1.5, n))
    b = np.zeros(m)
    np.add.at(b, rows, vals * xs[cols])
    lcon, ucon = b.copy(), b.copy()
    lcon[0], ucon[0] = b[0] - 1e15, b[0] + 1e15
    c = rng.standard_normal(n)
    c[GROW] = 1e3
    return QuadraticModel(c=c, Hrows=hr, Hcols=hc, Hvals=hv, Arows=rows, Acols=cols, Avals=vals, lcon=lcon, ucon=ucon,
                          lvar=lvar, uvar=uvar, c0=0.5, x0=x0, name="order_qp")


def _seq(terms, start=0.0):
    acc = np.float64(start)
    for t in terms:
        acc = acc + np.float64(t)
    return acc


def _order_sums(qp, by_value):
    """The five order-sensitive host sums of numeric_host: ax[0], cfix[0], g[GROW] (which must be gmax),
    gfix[JX], const_fixed, with their terms taken in input order, or (by_value) in ascending order of the
    matrix values (obj_scale and con_scale left at 1: the order is what is compared)."""
    fixed = qp.lvar == qp.uvar
    x = np.where(fixed, qp.lvar, qp.x0)            # x0 is inside the pushed bounds: the push leaves it
    Ar, Ac, Av = np.asarray(qp.Arows), np.asarray(qp.Acols), np.asarray(qp.Avals)
    Hr, Hc, Hv = np.asarray(qp.Hrows), np.asarray(qp.Hcols), np.asarray(qp.Hvals)
    ka = np.flatnonzero(Ar == 0)
    kh = np.arange(len(Hr))
    if by_value:
        ka, kh = ka[np.argsort(Av[ka], kind="stable")], kh[np.argsort(Hv, kind="stable")]
    ax0 = _seq(Av[k] * x[Ac[k]] for k in ka)
    cfix0 = _seq(Av[k] * x[Ac[k]] for k in ka if fixed[Ac[k]])
    g = {i: [qp.c[i]] for i in range(qp.nvar)}
    gf, cfx = [], []
    for k in kh:
        r, c, v = Hr[k], Hc[k], Hv[k]
        g[r].append(v * x[c])
        if r != c:
            g[c].append(v * x[r])
        if fixed[r] and fixed[c]:
            cfx.append((0.5 if r == c else 1.0) * v * x[r] * x[c])
        elif fixed[c] and r == JX:
            gf.append(v * x[c])
        elif fixed[r] and c == JX:
            gf.append(v * x[r])
    gs = {i: _seq(t[1:], t[0]) for i, t in g.items()}
    imax = max(gs, key=lambda i: abs(gs[i]))
    return dict(ax0=ax0, cfix0=cfix0, g=gs[GROW], gfix=_seq(gf), const_fixed=_seq(cfx)), imax


def _assert_order_matters(qp):
    inp, imax = _order_sums(qp, False)
    srt, _ = _order_sums(qp, True)
    assert imax == GROW
    for k in inp:
        assert np.float64(inp[k]).tobytes() != np.float64(srt[k]).tobytes(), (k, inp[k], srt[k])
    return inp, srt


def test_order_qp_sums_depend_on_the_order():
    """No GPU work: numpy shows that each of the five sums has other bits in sorted order than in input
    order, so a kernel that sums in another order cannot reproduce the fresh solver."""
    _assert_order_matters(order_qp())


@pytest.mark.parametrize("scaling", [True, False], ids=["scaling", "no_scaling"])
def test_order_sensitive_sums_match_fresh_solver(scaling):
    from madipm_amd import MPCSolver
    p0 = order_qp()
    # powers of two: every product and sum of p0 scales exactly, so p1's sums depend on the order as p0's do
    p1 = dataclasses.replace(p0, Avals=p0.Avals * 0.5, Hvals=p0.Hvals * 0.5, c=p0.c * 0.5, c0=-1.25)
    _assert_order_matters(p0)
    _assert_order_matters(p1)
    kw = _kw(scaling=scaling)
    s = MPCSolver(p0, **kw)
    a0 = s.solve()
    s.update_device(**_dvalues(p1))
    a1 = s.solve()
    assert_same(a1, _fresh(p1, **kw))
    assert len(a1.trace) > 1                 # the comparison covers iterations, not a failed start
    s.update_device(**_dvalues(p0))
    assert_same(s.solve(), a0)


# ------------------------------------------------------------------ 4. more than one workgroup, tails
def wide_lp():
    """m = 2 * 256 + 3 rows, n = 3 * 256 + 5 variables: a shifted diagonal plus one more entry per row, one
    empty ranged row (rowmax = 0: con_scale = min(1, 100 / 0) = 1) and one row of 70 entries."""
    from madipm_amd.qp import QuadraticModel
    rng = np.random.default_rng(12)
    m, n = 2 * 256 + 3, 3 * 256 + 5
    empty, long_ = 300, 41
    rows, cols, vals = [], [], []
    for r in range(m):
        if r == empty:
            continue
        js = [(r + 5) % n, (r + 261) % n] if r != long_ else [(11 * t + 2) % n for t in range(70)]
        for j in js:
            rows.append(r), cols.append(j), vals.append(rng.uniform(0.5, 2.0) * 10.0 ** rng.integers(-1, 4))
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
    assert len(set(zip(rows.tolist(), cols.tolist()))) == len(rows)
    xs = rng.uniform(0.5, 1.5, n)
    b = np.zeros(m)
    np.add.at(b, rows, vals * xs[cols])
    lcon, ucon = b.copy(), b.copy()
    rng_rows = np.arange(7, m, 9)
    lcon[rng_rows] -= 1.0
    ucon[rng_rows[::2]] += 1.0
    ucon[rng_rows[1::2]] = np.inf
    lcon[empty], ucon[empty] = -1.0, 1.0
    return QuadraticModel(c=rng.uniform(0.1, 1.0, n), Hrows=[], Hcols=[], Hvals=[], Arows=rows, Acols=cols, Avals=vals,
                          lcon=lcon, ucon=ucon, lvar=np.zeros(n), uvar=np.full(n, 4.0), x0=rng.uniform(0.2, 1.0, n),
                          name="wide_lp")


def test_several_workgroups_tails_empty_and_long_rows():
    from madipm_amd import MPCSolver
    p0 = wide_lp()
    assert p0.ncon == 515 and p0.nvar == 773
    p1 = perturbed(p0, 31)
    s = MPCSolver(p0, **_kw())
    s.solve()
    s.update_device(**_dvalues(p1))
    assert_same(s.solve(), _fresh(p1, **_kw()))
    _same_data(s.fetch_qp(), p1)


# ------------------------------------------------------------------ 5. partial updates, round trip
@pytest.mark.parametrize("kind", ["lp", "qp"])
def test_partial_device_updates_and_round_trip(kind):
    from madipm_amd import MPCSolver
    p0 = scaled_general(kind)
    p1 = perturbed(p0, 23)
    kw = _kw()
    s = MPCSolver(p0, **kw)
    first = s.solve()
    cur = p0
    steps = [(k,) for k in VALUE_FIELDS] + [("c", "lcon", "ucon", "lvar", "uvar"), ("Avals",)]
    p2 = perturbed(p0, 29)

    def one_side(field):
        """One bound array alone: the finite bounds of the ranged rows / free variables move outwards, the
        equality rows and fixed variables (whose two sides must move together) stay."""
        a = getattr(cur, field)
        tied = a == getattr(cur, {"lcon": "ucon", "ucon": "lcon", "lvar": "uvar", "uvar": "lvar"}[field])
        step = 0.01 * (1.0 + np.abs(np.where(np.isfinite(a), a, 0.0)))
        return np.where(tied, a, a - step if field[0] == "l" else a + step)

    for i, fields in enumerate(steps):
        if fields[0] in ("lcon", "ucon", "lvar", "uvar") and len(fields) == 1:
            part = {fields[0]: one_side(fields[0])}   # (the QP has equality rows only: its row bounds stay)
        else:
            part = {k: getattr(p1 if i < len(VALUE_FIELDS) else p2, k) for k in fields}
        cur = dataclasses.replace(cur, **part)
        s.update_device(**_dvalues(cur, fields))
        assert_same(s.solve(), _fresh(cur, **kw))
    s.update_device(**_dvalues(p0))
    assert_same(s.solve(), first)
    assert s.counters()["n_updates"] == len(steps) + 1 and s.counters()["n_analyses"] == 1
    _same_data(s.fetch_qp(), p0)


# ------------------------------------------------------------------ 6. rejections: the host's text, solver intact
def test_rejected_device_updates_carry_the_host_message():
    from madipm_amd import MPCSolver
    from madipm_amd._lib import MadIPMError
    qp = scaled_general("lp")
    s, h = MPCSolver(qp, **_kw()), MPCSolver(qp, **_kw())
    ref = s.solve()
    fixed = qp.lvar == qp.uvar
    ineq = qp.lcon != qp.ucon
    j_lo = int(np.flatnonzero(np.isfinite(qp.lvar) & ~fixed)[0])
    j_noup = int(np.flatnonzero(np.isinf(qp.uvar))[0])
    j_free = int(np.flatnonzero(~fixed)[5])
    i_eq, i_rng = int(np.flatnonzero(~ineq)[2]), int(np.flatnonzero(ineq)[1])

    def changed(field, idx, val):
        a = getattr(qp, field).copy()
        a[idx] = val
        return {field: a}

    cases = [changed("lvar", j_lo, -np.inf), changed("uvar", j_noup, 1e3), changed("uvar", 17, qp.uvar[17] + 1.0),
             {**changed("lvar", j_free, 0.25), **changed("uvar", j_free, 0.25)},
             changed("ucon", i_eq, qp.ucon[i_eq] + 1.0), changed("ucon", i_rng, qp.lcon[i_rng])]
    for upd in cases:
        with pytest.raises(MadIPMError) as eh:
            h.update(c=2.0 * qp.c, **upd)
        with pytest.raises(MadIPMError) as ed:
            s.update_device(c=_dev(2.0 * qp.c), **{k: _dev(v) for k, v in upd.items()})
        assert str(ed.value) == str(eh.value)
        assert_same(s.solve(), ref)          # the accepted part of the call was not installed either
    assert s.counters()["n_updates"] == 0 and s.qp_current
    import torch
    for bad, exc in ((_dev(qp.c[:-1]), ValueError), (_dev(np.repeat(qp.c, 2))[::2], ValueError), (qp.c, TypeError),
                     (torch.as_tensor(qp.c), TypeError), (_dev(qp.c).float(), TypeError)):
        with pytest.raises(exc):
            s.update_device(c=bad)
    assert s.counters()["n_updates"] == 0
    s.update_device(c=_dev(qp.c))            # and a valid one still goes through
    assert_same(s.solve(), ref)


# ------------------------------------------------------------------ 7. degenerate shapes
@pytest.mark.parametrize("name", ["box_qp", "free_eq_qp", "simple_lp"])
def test_degenerate_shapes(name):
    from madipm_amd import MPCSolver, simple_lp
    p0 = {"box_qp": box_qp, "free_eq_qp": lambda: free_eq_qp()[0], "simple_lp": simple_lp}[name]()
    rng = np.random.default_rng(2)
    new = dict(c=p0.c * rng.uniform(0.5, 2.0, p0.nvar), Hvals=p0.Hvals * rng.uniform(0.9, 1.1, p0.nnzh),
               Avals=p0.Avals * rng.uniform(0.5, 2.0, p0.nnzj))
    p1 = dataclasses.replace(p0, **new)
    s = MPCSolver(p0, **_kw())
    a0 = s.solve()
    s.update_device(**_dvalues(p1))
    a1 = s.solve()
    assert_same(a1, _fresh(p1, **_kw()))
    assert a1.objective != a0.objective and s.counters()["n_analyses"] == 1
    d = s.solution_device()
    for f in VECTORS:
        assert np.array_equal(d[f].cpu().numpy(), getattr(a1, f), equal_nan=True), f


# ------------------------------------------------------------------ 8. two shards on one device
def test_device_update_on_sharded_solver():
    from madipm_amd import MPCSolver
    p0 = scaled_general("lp")
    p1 = perturbed(p0, 101)
    kw = _kw(nshards=2)
    s = MPCSolver(p0, **kw)
    perm, info = s.kkt_perm(), s.ldl_info()
    s.solve()
    s.update_device(**_dvalues(p1))
    assert_same(s.solve(), _fresh(p1, **kw))
    assert s.counters()["n_analyses"] == 1
    assert np.array_equal(s.kkt_perm(), perm) and s.ldl_info() == info
    _same_data(s.fetch_qp(), p1)


# ------------------------------------------------------------------ 9. host and device updates mixed
@pytest.mark.parametrize("kind", ["lp", "qp"])
def test_mixing_host_and_device_updates(kind):
    from madipm_amd import MPCSolver
    p0 = scaled_general(kind)
    p1, p2 = perturbed(p0, 101), perturbed(p0, 55)
    kw = _kw()
    s = MPCSolver(p0, **kw)
    s.update_device(**_dvalues(p1))          # device (all fields), then the host with c only
    s.update(c=p2.c)
    m1 = dataclasses.replace(p1, c=p2.c)
    assert s.qp_current
    _same_data(s.qp, m1)
    assert_same(s.solve(), _fresh(m1, **kw))
    s.update(**{k: getattr(p2, k) for k in VALUE_FIELDS})   # host (all fields), then the device with Avals only
    s.update_device(Avals=_dev(p1.Avals))
    m2 = dataclasses.replace(p2, Avals=p1.Avals)
    assert_same(s.solve(), _fresh(m2, **kw))
    _same_data(s.fetch_qp(), m2)
    assert s.counters()["n_updates"] == 4 and s.counters()["n_analyses"] == 1


# ------------------------------------------------------------------ 10. the solution on the device
def test_solution_device_matches_the_host_arrays():
    import torch
    from madipm_amd import MPCSolver, _lib as L
    p0 = scaled_general("qp")
    p1 = perturbed(p0, 101)
    s = MPCSolver(p0, **_kw())
    a0 = s.solve()
    assert a0.status == 1
    d0 = s.solution_device()
    for f in VECTORS:
        assert d0[f].dtype == torch.float64 and d0[f].is_cuda
        assert np.array_equal(d0[f].cpu().numpy(), getattr(a0, f)), f
    s.update_device(**_dvalues(p1))
    a1 = s.solve(fetch_solution=False)
    assert a1.solution is None
    d1 = s.solution_device()
    ref = _fresh(p1, **_kw())
    for f in VECTORS:
        assert np.array_equal(d1[f].cpu().numpy(), getattr(ref, f)), f
    # NULL outputs at the C level: only x is asked for
    x = torch.empty(p0.nvar, dtype=torch.float64, device="cuda")
    rc = L.lib.madipm_solver_get_solution_device(s.h, C.cast(x.data_ptr(), L.f64p), None, None, None, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), ref.solution)


# ------------------------------------------------------------------ 11. the caller's stream
def test_arrays_produced_on_the_callers_stream():
    import torch
    from madipm_amd import MPCSolver
    p0 = scaled_general("lp")
    rng = np.random.default_rng(9)
    fa, fc = rng.uniform(0.5, 2.0, p0.nnzj), rng.uniform(0.5, 2.0, p0.nvar)
    p1 = dataclasses.replace(p0, Avals=p0.Avals * fa, c=p0.c * fc)
    s = MPCSolver(p0, **_kw())
    s.solve()
    base_a, base_c, dfa, dfc = _dev(p0.Avals), _dev(p0.c), _dev(fa), _dev(fc)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        filler = torch.ones(1 << 22, dtype=torch.float64, device="cuda")
        for _ in range(8):                   # work in front of the products, so that they are still pending
            filler = filler * 1.0000001
        av, cv = base_a * dfa, base_c * dfc
    s.update_device(Avals=av, c=cv, stream=st)   # no synchronisation of st before the call
    with torch.cuda.stream(st):
        av.zero_()                           # the call returned with its reads done
        cv.fill_(float("nan"))
    assert_same(s.solve(), _fresh(p1, **_kw()))
    st.synchronize()


# ------------------------------------------------------------------ 12. no allocation after the first call
def test_no_device_allocation_after_the_first_call():
    import torch
    from madipm_amd import MPCSolver
    p0 = scaled_general("qp")
    p1 = perturbed(p0, 101)
    d0, d1 = _dvalues(p0), _dvalues(p1)
    s = MPCSolver(p0, **_kw())
    s.solve()
    s.update_device(**d1)                    # the first call allocates the device route
    torch.cuda.synchronize()
    for d in (d0, d1):
        free = torch.cuda.mem_get_info()[0]
        s.update_device(**d)
        assert torch.cuda.mem_get_info()[0] == free
    assert_same(s.solve(), _fresh(p1, **_kw()))
