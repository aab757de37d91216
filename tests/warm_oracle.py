"""Test-side restatement of the warm-start rule on top of the CPU oracle.

WarmOracleMPC is oracle.mpc.OracleMPC with one override: init_starting_point runs the cold start unchanged,
then blends it with a caller-given point (x, y, zl, zu) of the PUBLIC, unscaled space (what solve() returns
as solution / multipliers / multipliers_L / multipliers_U; any of the four may be None):

  1. x~  = clamp(x, xl, xu) on the variables (the relaxed bounds; a fixed variable gives its fixed value);
  2. s~  = clamp(con_scale (A x~) on the inequality rows, xl_s, xu_s);
  3. y~  = y obj_scale / con_scale, zl~ = max(zl obj_scale, 0), zu~ = max(zu obj_scale, 0),
     slack multipliers zl_s~ = max(-y~, 0), zu_s~ = max(y~, 0);
  4. v = w v~ + (1 - w) v_cold for x and s (free coordinates), y, zl on ind_lb, zu on ind_ub; a block whose
     input is absent keeps its cold values (slack values need x, slack multipliers need y); a coordinate
     whose blended value is not strictly interior keeps its cold value;
  5. evaluate_model! at the blended point.

norm_c stays the cold one (initialize! computes it before the start point exists).
"""
from __future__ import annotations

import numpy as np

from oracle.mpc import OracleMPC


def clip_nan(v, lo, hi):
    """clamp that lets a NaN through (np.clip does; written out so that the rule is visible)."""
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


class WarmOracleMPC(OracleMPC):
    def __init__(self, qp, opt=None, warm=None, weight=0.99, record_trace=True):
        super().__init__(qp, opt, record_trace)
        assert 0.0 < weight < 1.0
        self.warm = dict(warm or {})
        self.weight = float(weight)
        self.cold_point = None       # (x, y, zl, zu) of the cold start, scaled space
        self.n_warm_inits = 0

    def _get(self, key, length):
        v = self.warm.get(key)
        if v is None:
            return None
        v = np.asarray(v, float)
        assert v.shape == (length,), (key, v.shape, length)
        return v

    def init_starting_point(self):
        super().init_starting_point()
        self.cold_point = (self.x.copy(), self.y.copy(), self.zl.copy(), self.zu.copy())
        wx, wy = self._get("x", self.nx), self._get("y", self.m)
        wzl, wzu = self._get("zl", self.nx), self._get("zu", self.nx)
        if wx is None and wy is None and wzl is None and wzu is None:
            return
        lam = self.weight
        one_m = 1.0 - lam
        nx, n = self.nx, self.n
        xl, xu = self.xl, self.xu
        free = ~self._fixed_mask
        in_lb = np.zeros(n, bool)
        in_ub = np.zeros(n, bool)
        in_lb[self.ind_lb] = True
        in_ub[self.ind_ub] = True
        os_ = self.obj_scale
        with np.errstate(invalid="ignore"):
            if wx is not None:
                xt = np.empty(n)
                xt[:nx] = clip_nan(wx, xl[:nx], xu[:nx])
                rows = self.con_scale * (self._A @ xt[:nx])
                xt[nx:] = clip_nan(rows[self.ind_ineq], xl[nx:], xu[nx:])
                v = lam * xt + one_m * self.x
                bad = (in_lb & (v <= xl)) | (in_ub & (v >= xu))
                take = free & ~bad
                self.x = np.where(take, v, self.x)
            yt = None
            if wy is not None:
                yt = wy * os_ / self.con_scale
                self.y = lam * yt + one_m * self.y
            zlt = np.full(n, np.nan)
            zut = np.full(n, np.nan)
            has_l = np.zeros(n, bool)
            has_u = np.zeros(n, bool)
            if wzl is not None:
                zlt[:nx] = np.maximum(wzl * os_, 0.0)
                has_l[:nx] = True
            if wzu is not None:
                zut[:nx] = np.maximum(wzu * os_, 0.0)
                has_u[:nx] = True
            if yt is not None and self.ns:
                ys = yt[self.ind_ineq]
                zlt[nx:] = np.maximum(-ys, 0.0)
                zut[nx:] = np.maximum(ys, 0.0)
                has_l[nx:] = True
                has_u[nx:] = True
            v = lam * zlt + one_m * self.zl
            self.zl = np.where(in_lb & has_l & ~(v <= 0.0), v, self.zl)
            v = lam * zut + one_m * self.zu
            self.zu = np.where(in_ub & has_u & ~(v <= 0.0), v, self.zu)
        # step 5: evaluate_model! at the blended point (initialize! adds jacl right after)
        self.obj_val = self.eval_f(self.x)
        self.c = self.eval_cons(self.x)
        self.f = self.eval_grad(self.x)
        self.n_warm_inits += 1

    def strictly_interior(self):
        lb, ub = self.ind_lb, self.ind_ub
        return bool(np.all(self.x[lb] > self.xl[lb]) and np.all(self.x[ub] < self.xu[ub])
                    and np.all(self.zl[lb] > 0.0) and np.all(self.zu[ub] > 0.0))


def warm_point(st):
    """The public point of a finished solve (an OracleStats or an ExecutionStats) as a warm point."""
    return dict(x=np.array(st.solution, float), y=np.array(st.multipliers, float),
                zl=np.array(st.multipliers_L, float), zu=np.array(st.multipliers_U, float))


def warm_solve(qp, opt, warm, weight=0.99):
    o = WarmOracleMPC(qp, opt, warm, weight)
    with np.errstate(invalid="ignore"):
        st = o.solve()
    return o, st
