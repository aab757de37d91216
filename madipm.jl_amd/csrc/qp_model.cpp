// The problem model of MPCSolver (qp_model.hpp): plain arithmetic over the caller's QP, no HIP call.
#include "qp_model.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "common.hpp"  // Error, MADIPM_REQUIRE, PhaseClock
#include "symbolic.hpp"  // analysis_threads

namespace madipm {

namespace {

constexpr double INF = std::numeric_limits<double>::infinity();

// ---- host construction helpers, threaded for the dense-QP config (5e8 entries in A): every O(nnz) pass
// runs on analysis_threads() host threads over contiguous input chunks, with per-thread counts and
// offsets in thread order, so the result is the one-thread result bit for bit (r3: 38 s of analysis_s
// on the box, mostly single-threaded passes and growing vectors over the 5e8 entries).
template <class F>
void par_range(int64_t n, F f, int64_t grain = (int64_t)1 << 20) {
  const int T = (int)std::min<int64_t>(analysis_threads(), std::max<int64_t>(1, n / grain));
  if (T <= 1) {
    f(0, (int64_t)0, n);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back(f, t, n * t / T, n * (t + 1) / T);
  for (auto& x : th) x.join();
}
int par_threads(int64_t n, int64_t grain = (int64_t)1 << 20) {
  return (int)std::min<int64_t>(analysis_threads(), std::max<int64_t>(1, n / grain));
}

// CSR (sorted by (row, col), duplicates summed in input order) of the COO (r, c, v): a stable counting
// sort by row — per-thread row counts over input chunks, offsets in thread order — then each row's
// run sorted by column only when it is not already (O(nnz) for the usual column- or row-major input;
// a comparison sort of 1e9 dense-QP entries took minutes) and duplicates merged
// entry k of the COO: row R(k), column C(k), value V(k) (accessors: the scaled Jacobian is read
// straight from the caller's A, no COO copy); the CSR arrays are filled in full by the threads
template <class R, class C, class V>
void csr_from_coo(int nrow, int64_t nnz, R r, C c, V v, std::vector<int64_t>& rp, hvec<int32_t>& ci,
                  hvec<double>& cv) {
  // per-thread row counts cost T (nrow + 1) int64: bound T so that they stay within the entries' own
  // size (a tall sparse matrix with millions of rows would otherwise take gigabytes of scratch)
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(par_threads(nnz), nnz / (4 * ((int64_t)nrow + 1))));
  std::vector<std::vector<int64_t>> cnt(T, std::vector<int64_t>(nrow + 1, 0));
  auto chunk = [&](int t) { return std::make_pair(nnz * t / T, nnz * (t + 1) / T); };
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t] {
        auto [k0, k1] = chunk(t);
        int64_t* cn = cnt[t].data();
        for (int64_t k = k0; k < k1; ++k) cn[r(k)]++;
      });
    for (auto& x : th) x.join();
  }
  std::vector<int64_t> start(nrow + 1, 0);
  for (int i = 0; i < nrow; ++i) {
    int64_t acc = start[i];
    for (int t = 0; t < T; ++t) {
      const int64_t c_ = cnt[t][i];
      cnt[t][i] = acc;  // this thread's first slot in row i
      acc += c_;
    }
    start[i + 1] = acc;
  }
  hvec<int32_t> tc(nnz);
  hvec<double> tv(nnz);
  {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t] {
        auto [k0, k1] = chunk(t);
        int64_t* off = cnt[t].data();
        for (int64_t k = k0; k < k1; ++k) {
          const int64_t q = off[r(k)]++;
          tc[q] = c(k);
          tv[q] = v(k);
        }
      });
    for (auto& x : th) x.join();
  }
  // per row: sort if needed (stable: duplicates keep input order), count the distinct columns
  std::vector<int64_t> uniq(nrow + 1, 0);
  par_range(nrow, [&](int, int64_t i0, int64_t i1) {
    std::vector<std::pair<int32_t, double>> buf;
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t b = start[i], e = start[i + 1];
      bool sorted = true;
      for (int64_t q = b; q + 1 < e && sorted; ++q) sorted = tc[q] <= tc[q + 1];
      if (!sorted) {
        buf.clear();
        for (int64_t q = b; q < e; ++q) buf.emplace_back(tc[q], tv[q]);
        std::stable_sort(buf.begin(), buf.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
        for (int64_t q = b; q < e; ++q) tc[q] = buf[q - b].first, tv[q] = buf[q - b].second;
      }
      int64_t u = 0;
      for (int64_t q = b; q < e; ++q) u += (q == b || tc[q] != tc[q - 1]);
      uniq[i + 1] = u;
    }
  }, 4096);
  for (int i = 0; i < nrow; ++i) uniq[i + 1] += uniq[i];
  if (uniq[nrow] == nnz) {  // no duplicates: the sorted runs are the CSR
    rp = std::move(start);
    ci = std::move(tc);
    cv = std::move(tv);
    return;
  }
  rp = uniq;
  ci.resize(uniq[nrow]);
  cv.resize(uniq[nrow]);
  par_range(nrow, [&](int, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      int64_t o = rp[i] - 1;
      for (int64_t q = start[i]; q < start[i + 1]; ++q) {
        if (q == start[i] || tc[q] != tc[q - 1]) {
          ++o;
          ci[o] = tc[q];
          cv[o] = tv[q];
        } else {
          cv[o] += tv[q];
        }
      }
    }
  }, 4096);
}
void csr_from_coo(int nrow, const std::vector<int32_t>& r, const std::vector<int32_t>& c,
                  const std::vector<double>& v, std::vector<int64_t>& rp, hvec<int32_t>& ci, hvec<double>& cv) {
  const int32_t *rr = r.data(), *cc = c.data();
  const double* vv = v.data();
  csr_from_coo(
      nrow, (int64_t)r.size(), [=](int64_t k) { return rr[k]; }, [=](int64_t k) { return cc[k]; },
      [=](int64_t k) { return vv[k]; }, rp, ci, cv);
}

// xl / xu of [x; s] as given: the variables' bounds, then the ranged rows' (before relaxation and scaling)
void raw_bounds(QPHost& P) {
  const int nx = P.nx;
  P.xl.resize(P.n);
  P.xu.resize(P.n);
  for (int i = 0; i < nx; ++i) {
    P.xl[i] = P.lvar[i];
    P.xu[i] = P.uvar[i];
  }
  for (int k = 0; k < P.ns; ++k) {
    P.xl[nx + k] = P.lcon[P.ind_ineq[k]];
    P.xu[nx + k] = P.ucon[P.ind_ineq[k]];
  }
}

// Stable counting sort of the entries ent[t] by their destinations dest[t] (given in input order):
// sp[d] .. sp[d + 1] lists destination d's entries, input order kept.  The one bucketing behind the device
// route's lists and the adjoint's.
void bucket(int nd, const std::vector<int32_t>& dest, const std::vector<I2>& ent, std::vector<int32_t>& sp,
            std::vector<I2>& out) {
  sp.assign(nd + 1, 0);
  for (int32_t d : dest) sp[d + 1]++;
  for (int i = 0; i < nd; ++i) sp[i + 1] += sp[i];
  out.resize(ent.size());
  std::vector<int32_t> fill(sp.begin(), sp.end() - 1);
  for (size_t t = 0; t < dest.size(); ++t) out[fill[dest[t]]++] = ent[t];
}
// Entries k of A in a fixed column, bucketed by dst(row, col) as (k, oth(row, col)): by row for the device
// route's cfix sum, by fixed variable for the adjoint's lvar gradient
template <class D, class O>
void fixed_column_lists(const QPHost& P, int nd, D dst, O oth, std::vector<int32_t>& sp, std::vector<I2>& out) {
  std::vector<int32_t> dest;
  std::vector<I2> ent;
  for (int64_t k = 0; k < P.nnzA; ++k)
    if (P.fixed[P.Ac[k]]) {
      dest.push_back(dst(P.Ar[k], P.Ac[k]));
      ent.push_back({(int32_t)k, oth(P.Ar[k], P.Ac[k])});
    }
  bucket(nd, dest, ent, sp, out);
}
// Entries k of H between a fixed and a free variable, bucketed by dst(fixed, free) as (k, oth(fixed, free)):
// by free endpoint for the device route's gfix sum, by fixed variable for the adjoint's lvar gradient
template <class D, class O>
void fixed_free_lists(const QPHost& P, int nd, D dst, O oth, std::vector<int32_t>& sp, std::vector<I2>& out) {
  std::vector<int32_t> dest;
  std::vector<I2> ent;
  for (size_t k = 0; k < P.Hv.size(); ++k) {
    const int r = P.Hr[k], c = P.Hc[k];
    if (P.fixed[r] == P.fixed[c]) continue;
    const int fx = P.fixed[r] ? r : c, fr = P.fixed[r] ? c : r;
    dest.push_back(dst(fx, fr));
    ent.push_back({(int32_t)k, oth(fx, fr)});
  }
  bucket(nd, dest, ent, sp, out);
}

}  // namespace

int bound_class(double l, double u) { return l == u ? 1 : (l != -INF ? 2 : 0) | (u != INF ? 4 : 0); }

[[noreturn]] void throw_kind_change(int idx, bool was_equality) {
  throw Error("madipm_solver_update: constraint " + std::to_string(idx) +
                  (was_equality ? " was an equality (lcon == ucon) and would become ranged"
                                : " was ranged (lcon != ucon) and would become an equality") +
                  " (the classification of every bound is fixed at creation; nothing was changed)",
              -3);
}
void require_same_class(const char* what, int idx, int a, int b) {
  if (a == b) return;
  std::string how;
  if ((a == 1) != (b == 1))
    how = a == 1 ? "was fixed (lower == upper bound) and would become free"
                 : "was free (lower != upper bound) and would become fixed";
  else if ((a & 2) != (b & 2))
    how = (a & 2) ? "had a finite lower bound that would become infinite"
                  : "had an infinite lower bound that would become finite";
  else
    how = (a & 4) ? "had a finite upper bound that would become infinite"
                  : "had an infinite upper bound that would become finite";
  throw Error(std::string("madipm_solver_update: ") + what + " " + std::to_string(idx) + " " + how +
                  " (the classification of every bound is fixed at creation; nothing was changed)",
              -3);
}
void require_same_class(const char* what, int idx, double l0, double u0, double l1, double u1) {
  require_same_class(what, idx, bound_class(l0, u0), bound_class(l1, u1));
}

void require_same_classes(const QPHost& P, const double* lv, const double* uv, const double* lc,
                          const double* uc) {
  for (int i = 0; i < P.m; ++i) {
    const bool was = P.lcon[i] == P.ucon[i], is = lc[i] == uc[i];
    if (was != is) throw_kind_change(i, was);
  }
  for (int i = 0; i < P.nx; ++i) require_same_class("variable", i, P.lvar[i], P.uvar[i], lv[i], uv[i]);
  for (int k = 0; k < P.ns; ++k) {
    const int r = P.ind_ineq[k];
    require_same_class("constraint", r, P.lcon[r], P.ucon[r], lc[r], uc[r]);
  }
}

void qp_intake(QPHost& P, const madipm_qp& q, PhaseClock* clk) {
  MADIPM_REQUIRE(q.nvar >= 0 && q.ncon >= 0, "negative dimensions");
  P.nx = q.nvar;
  P.m = q.ncon;
  const int nx = P.nx, m = P.m;
  auto cp = [](const double* a, int64_t n, double dflt = 0.0) {
    std::vector<double> v(n, dflt);
    if (a) std::copy(a, a + n, v.begin());
    return v;
  };
  P.c = cp(q.c, nx);
  P.lvar = cp(q.lvar, nx, -INF);
  P.uvar = cp(q.uvar, nx, INF);
  P.lcon = cp(q.lcon, m, -INF);
  P.ucon = cp(q.ucon, m, INF);
  P.x0 = cp(q.x0, nx);
  P.y0 = cp(q.y0, m);
  P.c0 = q.c0;
  P.minimize = q.minimize != 0;
  P.sgn = P.minimize ? 1.0 : -1.0;
  P.Hr.assign(q.Hrows, q.Hrows + q.nnzh);
  P.Hc.assign(q.Hcols, q.Hcols + q.nnzh);
  P.Hv.assign(q.Hvals, q.Hvals + q.nnzh);
  P.Ar = q.Arows;
  P.Ac = q.Acols;
  P.Av = q.Avals;
  P.nnzA = q.nnzj;
  for (int64_t k = 0; k < q.nnzh; ++k)
    MADIPM_REQUIRE(P.Hr[k] >= P.Hc[k] && P.Hr[k] < nx && P.Hc[k] >= 0, "H must be lower-triangular COO in range");
  {
    std::atomic<bool> bad{false};
    par_range(q.nnzj, [&](int, int64_t a, int64_t b) {
      bool ok = true;
      for (int64_t k = a; k < b; ++k) ok &= P.Ar[k] >= 0 && P.Ar[k] < m && P.Ac[k] >= 0 && P.Ac[k] < nx;
      if (!ok) bad = true;
    });
    MADIPM_REQUIRE(!bad, "A index out of range");
  }
  if (clk) (*clk)("copy + validate");
  // ---- index sets: MadNLP.get_index_constraints (EnforceEquality, MakeParameter) [EXT]
  for (int i = 0; i < m; ++i)
    if (P.lcon[i] != P.ucon[i]) P.ind_ineq.push_back(i);
  P.ns = (int)P.ind_ineq.size();
  const int n = nx + P.ns;
  P.n = n;
  raw_bounds(P);
  P.fixed.assign(n, 0);
  for (int i = 0; i < n; ++i) {
    if (P.xl[i] == P.xu[i]) {
      P.ind_fixed.push_back(i);
      P.fixed[i] = 1;
    } else {
      if (P.xl[i] != -INF) P.ind_lb.push_back(i);
      if (P.xu[i] != INF) P.ind_ub.push_back(i);
    }
  }
  // structure.jl:172-173 field swap => update_barrier! tests nlb + nub > 0
  P.has_ineq = (P.ind_lb.size() + P.ind_ub.size()) > 0;
  for (int i = 0; i < nx && !P.anyfix; ++i) P.anyfix = P.fixed[i];
}

void numeric_host(QPHost& P, const madipm_options& opt, HostNumeric& o, JCoo* jcoo) {
  PhaseClock clk("numeric_host");
  const int nx = P.nx, m = P.m, n = P.n;
  raw_bounds(P);
  // ---- MadNLP.initialize!(cb, ...) [EXT]
  P.x.assign(n, 0.0);
  for (int i = 0; i < nx; ++i) P.x[i] = P.x0[i];
  for (int i : P.ind_fixed) P.x[i] = P.xl[i];
  P.y = P.y0;
  P.rhs.assign(m, 0.0);
  for (int i = 0; i < m; ++i) P.rhs[i] = (P.lcon[i] == P.ucon[i]) ? P.lcon[i] : 0.0;
  const double tol = opt.bound_relax_factor;
  for (int i = 0; i < n; ++i) {
    if (P.fixed[i]) continue;
    if (std::isfinite(P.xl[i])) P.xl[i] = P.xl[i] - tol * std::max(1.0, std::fabs(P.xl[i]));
    if (std::isfinite(P.xu[i])) P.xu[i] = P.xu[i] + tol * std::max(1.0, std::fabs(P.xu[i]));
  }
  if (P.ns) {
    std::vector<double> ax(m, 0.0);
    for (int64_t k = 0; k < P.nnzA; ++k) ax[P.Ar[k]] += P.Av[k] * P.x[P.Ac[k]];
    for (int k = 0; k < P.ns; ++k) P.x[nx + k] = ax[P.ind_ineq[k]];
  }
  clk("bounds + slack start A x");
  // initialize_variables! (Ipopt bound push) [EXT]
  const double bp = opt.bound_push, bf = opt.bound_fac;
  for (int i = 0; i < n; ++i) {
    if (P.fixed[i]) continue;
    const double l = P.xl[i], u = P.xu[i];
    double lo = -INF, hi = INF;
    if (std::isfinite(l)) {
      double pl = bp * std::max(1.0, std::fabs(l));
      if (std::isfinite(u)) pl = std::min(pl, bf * (u - l));
      lo = l + pl;
    }
    if (std::isfinite(u)) {
      double pu = bp * std::max(1.0, std::fabs(u));
      if (std::isfinite(l)) pu = std::min(pu, bf * (u - l));
      hi = u - pu;
    }
    P.x[i] = std::min(std::max(P.x[i], lo), hi);
  }
  // ---- set_scaling!(..., 100) [EXT] (solver.jl:148-159)
  P.obj_scale = 1.0;
  P.con_scale.assign(m, 1.0);
  if (opt.scaling) {
    std::vector<double> g(nx);
    for (int i = 0; i < nx; ++i) g[i] = P.sgn * P.c[i];
    for (size_t k = 0; k < P.Hv.size(); ++k) {
      const int r = P.Hr[k], c = P.Hc[k];
      const double v = P.sgn * P.Hv[k];
      g[r] += v * P.x[c];
      if (r != c) g[c] += v * P.x[r];
    }
    double gmax = 0;
    for (double v : g) gmax = std::max(gmax, std::fabs(v));
    P.obj_scale = gmax > 0 ? std::min(1.0, 100.0 / gmax) : 1.0;
    std::vector<double> rowmax(m, 0.0);
    {  // per-thread row maxima, then their maximum (order-free)
      const int64_t nz = P.nnzA;
      // at most nz / (4 m) threads: their m-long maxima stay within the entries' own size
      const int64_t tc = std::max<int64_t>(1, std::min<int64_t>(par_threads(nz), nz / (4 * std::max(m, 1))));
      std::vector<std::vector<double>> rm(tc, std::vector<double>(m, 0.0));
      par_range(nz, [&](int t, int64_t a, int64_t b) {
        double* x = rm[t].data();
        for (int64_t k = a; k < b; ++k) x[P.Ar[k]] = std::max(x[P.Ar[k]], std::fabs(P.Av[k]));
      }, std::max<int64_t>((int64_t)1 << 20, (nz + tc - 1) / tc));
      for (const auto& x : rm)
        for (int i = 0; i < m; ++i) rowmax[i] = std::max(rowmax[i], x[i]);
    }
    for (int i = 0; i < m; ++i) P.con_scale[i] = std::min(1.0, 100.0 / rowmax[i]);
    for (int k = 0; k < P.ns; ++k) {
      const double cs = P.con_scale[P.ind_ineq[k]];
      P.xl[nx + k] *= cs;
      P.xu[nx + k] *= cs;
      P.x[nx + k] *= cs;
    }
    for (int i = 0; i < m; ++i) P.rhs[i] *= P.con_scale[i];
  }
  o.obj_scale = P.obj_scale;
  clk("bound push + scaling");
  // fixed variables (MakeParameter): their Hessian terms -> objective constant / gradient shift ...
  o.gfix.assign(n, 0.0);
  o.cfix.assign(m, 0.0);
  double const_fixed = 0.0;
  for (size_t k = 0; k < P.Hv.size(); ++k) {
    const int r = P.Hr[k], c = P.Hc[k];
    const bool fr = P.fixed[r], fc = P.fixed[c];
    if (!fr && !fc) continue;
    const double v = P.obj_scale * P.sgn * P.Hv[k];
    if (fr && fc) {
      const_fixed += (r == c ? 0.5 : 1.0) * v * P.x[r] * P.x[c];
      continue;
    }
    // cross term with a fixed variable -> constant gradient shift
    if (!fr) o.gfix[r] += v * P.x[c];
    if (!fc) o.gfix[c] += v * P.x[r];
  }
  // ... and their Jacobian columns -> cfix, summed in input order: the sequential pass (which, at
  // construction, also collects the COO of the columns that stay)
  if (P.anyfix) {
    const int64_t nz = P.nnzA;
    for (int64_t k = 0; k < nz; ++k) {
      const int r = P.Ar[k], c = P.Ac[k];
      const double v = P.con_scale[r] * P.Av[k];
      if (P.fixed[c]) {
        o.cfix[r] += v * P.x[c];
        continue;
      }
      if (jcoo) {
        jcoo->r.push_back(r);
        jcoo->c.push_back(c);
        jcoo->v.push_back(v);
      }
    }
  }
  o.cs.assign(n, 0.0);
  for (int i = 0; i < nx; ++i) o.cs[i] = P.obj_scale * P.sgn * P.c[i];
  o.c0s = P.obj_scale * (P.sgn * P.c0) + const_fixed;
  // norm_b (solver.jl:173) on host
  o.norm_b = 0;
  for (double v : P.rhs) o.norm_b = std::max(o.norm_b, std::fabs(v));
  clk("fixed terms, cs, norms");
}

std::vector<int64_t> k2_colptr(int n, int m, const int64_t* Hrp, const int32_t* Hci, const int64_t* JTrp) {
  std::vector<int64_t> hup(n, 0), Kcp(n + m + 1, 0);  // hup: per column, H entries below the diagonal
  for (int i = 0; i < n; ++i)
    for (int64_t q = Hrp[i]; q < Hrp[i + 1]; ++q) hup[i] += Hci[q] > i;
  for (int j = 0; j < n + m; ++j) Kcp[j + 1] = Kcp[j] + 1 + (j < n ? hup[j] + (JTrp[j + 1] - JTrp[j]) : 0);
  return Kcp;
}

// Structural part of the construction: MPCSolver(...) (structure.jl:79-178) and the K2 pattern of
// SparseKKTSystem [EXT].
QPStructure build_structure(QPHost& P, const madipm_options& opt, JCoo& jcoo, PhaseClock* clkp) {
  auto clk = [&](const char* what) {
    if (clkp) (*clkp)(what);
  };
  QPStructure S;
  const int nx = P.nx, m = P.m, n = P.n;
  // scaled Hessian (full symmetric CSR over n; MakeParameter zeroes fixed rows/cols), diagonal apart
  std::vector<int32_t> hr, hc;
  std::vector<double> hv;
  S.Hdiag.assign(n, 0.0);
  for (size_t k = 0; k < P.Hv.size(); ++k) {
    const int r = P.Hr[k], c = P.Hc[k];
    const double v = P.obj_scale * P.sgn * P.Hv[k];
    if (P.fixed[r] || P.fixed[c]) continue;  // numeric_host: const_fixed / gfix
    if (r == c) {
      S.Hdiag[r] += v;
      hr.push_back(r);
      hc.push_back(c);
      hv.push_back(v);
    } else {
      hr.push_back(r);
      hc.push_back(c);
      hv.push_back(v);
      hr.push_back(c);
      hc.push_back(r);
      hv.push_back(v);
    }
  }
  csr_from_coo(n, hr, hc, hv, S.Hrp, S.Hci, S.Hcv);
  // scaled Jacobian with slack columns (m x n); fixed columns zeroed (their term -> cfix).  Without a
  // fixed column every entry is kept in input order and read straight from the caller's A; with one,
  // numeric_host's cfix pass has filled the COO
  const bool anyfix = P.anyfix;
  std::vector<int32_t>&jr = jcoo.r, &jc = jcoo.c;
  std::vector<double>& jv = jcoo.v;
  if (anyfix)
    for (int k = 0; k < P.ns; ++k) {
      jr.push_back(P.ind_ineq[k]);
      jc.push_back(nx + k);
      jv.push_back(-1.0);
    }
  clk("H CSR + J COO");
  if (anyfix) {
    csr_from_coo(m, jr, jc, jv, S.Jrp, S.Jci, S.Jcv);
    csr_from_coo(n, jc, jr, jv, S.JTrp, S.JTci, S.JTcv);
    std::vector<int32_t>().swap(jr);
    std::vector<int32_t>().swap(jc);
    std::vector<double>().swap(jv);
  } else {  // entries k < nnzA: A's (scaled); then one -1 per slack column
    const int64_t na = P.nnzA, nj = na + P.ns;
    const int32_t *Ar = P.Ar, *Ac = P.Ac, *ineq = P.ind_ineq.data();
    const double *Av = P.Av, *cs = P.con_scale.data();
    auto row = [=](int64_t k) { return k < na ? Ar[k] : ineq[k - na]; };
    auto col = [=](int64_t k) { return k < na ? Ac[k] : (int32_t)(nx + (k - na)); };
    auto val = [=](int64_t k) { return k < na ? cs[Ar[k]] * Av[k] : -1.0; };
    csr_from_coo(m, nj, row, col, val, S.Jrp, S.Jci, S.Jcv);
    csr_from_coo(n, nj, col, row, val, S.JTrp, S.JTci, S.JTcv);
  }
  clk("J, J^T CSR");
  // K2 lower CSC: diag(n+m) + H strictly-lower + J at rows n+r  (SparseKKTSystem [EXT]), built by
  // columns in k2_colptr's layout
  S.Kcp = k2_colptr(n, m, S.Hrp.data(), S.Hci.data(), S.JTrp.data());
  {
    const std::vector<int64_t>&Kcp = S.Kcp, &Hrp = S.Hrp, &JTrp = S.JTrp;
    hvec<int32_t>&Kri = S.Kri, &Hci = S.Hci, &JTci = S.JTci;
    hvec<double>&Kv = S.Kv, &Hcv = S.Hcv, &JTcv = S.JTcv;
    Kri.resize(Kcp[n + m]);
    Kv.resize(Kcp[n + m]);
    par_range(n + m, [&](int, int64_t j0, int64_t j1) {
      for (int64_t j = j0; j < j1; ++j) {
        int64_t o = Kcp[j];
        Kri[o] = (int32_t)j;
        Kv[o++] = 0.0;
        if (j >= n) continue;
        for (int64_t q = Hrp[j]; q < Hrp[j + 1]; ++q)
          if (Hci[q] > j) {
            Kri[o] = Hci[q];
            Kv[o++] = Hcv[q];
          }
        for (int64_t q = JTrp[j]; q < JTrp[j + 1]; ++q) {
          Kri[o] = n + JTci[q];
          Kv[o++] = JTcv[q];
        }
      }
    }, 1024);
  }
  S.diag_pos.assign(S.Kcp.begin(), S.Kcp.end() - 1);  // the diagonal leads every column
  P.nJ = (int64_t)S.Jci.size();
  P.nH = (int64_t)S.Hci.size();
  P.nnzK = (int64_t)S.Kri.size();
  clk("K2 CSC");
  S.lbpos.assign(n, -1);
  S.ubpos.assign(n, -1);
  for (size_t k = 0; k < P.ind_lb.size(); ++k) S.lbpos[P.ind_lb[k]] = (int32_t)k;
  for (size_t k = 0; k < P.ind_ub.size(); ++k) S.ubpos[P.ind_ub[k]] = (int32_t)k;

  const int kkt = opt.kkt_system;
  MADIPM_REQUIRE(kkt == KKT_K2 || kkt == KKT_K25 || kkt == KKT_NORMAL, "unknown kkt_system");
  if (kkt == KKT_NORMAL) {
    // NormalKKTSystem constructor (normalkkt.jl:29-140): LP only; pattern of tril(A A^T) with A the
    // scaled Jacobian with slack columns (build_normal_system, utils.jl:209-274), plus the product
    // list of every entry for the assembly kernel (positions into J's CSR values).
    MADIPM_REQUIRE(P.Hv.empty(),
                   "The KKT system NormalKKTSystem supports only linear programs. "
                   "The problem has a positive number of nonzero in its Hessian.");
    const std::vector<int64_t>& Jrp = S.Jrp;
    const hvec<int32_t>& Jci = S.Jci;
    std::vector<int64_t>&Ccp = S.Ccp, &cpp = S.cpp;
    std::vector<int32_t>&Cri = S.Cri, &cprod = S.cprod;
    std::vector<int64_t> colp(n + 1, 0);
    for (int32_t k : Jci) colp[k + 1]++;
    for (int k = 0; k < n; ++k) colp[k + 1] += colp[k];
    std::vector<int32_t> crow(Jci.size()), cpos(Jci.size());
    {
      std::vector<int64_t> fill(colp.begin(), colp.end() - 1);
      for (int i = 0; i < m; ++i)
        for (int64_t p = Jrp[i]; p < Jrp[i + 1]; ++p) {
          const int64_t t = fill[Jci[p]]++;
          crow[t] = i;
          cpos[t] = (int32_t)p;
        }
    }
    Ccp.assign(m + 1, 0);
    cpp.push_back(0);
    struct Prod {
      int32_t j, a, b;
    };
    std::vector<Prod> pr;
    for (int i = 0; i < m; ++i) {
      pr.clear();
      for (int64_t p = Jrp[i]; p < Jrp[i + 1]; ++p) {
        const int k = Jci[p];
        for (int64_t t = colp[k]; t < colp[k + 1]; ++t)
          if (crow[t] >= i) pr.push_back({crow[t], (int32_t)p, cpos[t]});
      }
      std::stable_sort(pr.begin(), pr.end(), [](const Prod& x, const Prod& y) { return x.j < y.j; });
      for (size_t t = 0; t < pr.size(); ++t) {
        if (t == 0 || pr[t].j != pr[t - 1].j) {
          if (t) cpp.push_back((int64_t)cprod.size() / 2);
          Cri.push_back(pr[t].j);
        }
        cprod.push_back(pr[t].a);
        cprod.push_back(pr[t].b);
      }
      if (!pr.empty()) {
        cpp.push_back((int64_t)cprod.size() / 2);
      } else {  // empty row of A: structurally singular C; keep the (zero) diagonal entry
        Cri.push_back(i);
        cpp.push_back((int64_t)cprod.size() / 2);
      }
      Ccp[i + 1] = (int64_t)Cri.size();
    }
  }
  return S;
}

hvec<int32_t> k2_slot_columns(const std::vector<int64_t>& Kcp) {
  const int64_t nc = (int64_t)Kcp.size() - 1;
  hvec<int32_t> kcol(Kcp[nc]);
  par_range(nc, [&](int, int64_t j0, int64_t j1) {
    for (int64_t j = j0; j < j1; ++j)
      for (int64_t q = Kcp[j]; q < Kcp[j + 1]; ++q) kcol[q] = (int32_t)j;
  }, 1024);
  return kcol;
}

CooPlan coo_plan(int nrow, const std::vector<int32_t>& r, const std::vector<int32_t>& c,
                 const std::vector<int32_t>& id) {
  const int64_t N = (int64_t)r.size();
  std::vector<int64_t> start(nrow + 1, 0);
  for (int64_t k = 0; k < N; ++k) start[r[k] + 1]++;
  for (int i = 0; i < nrow; ++i) start[i + 1] += start[i];
  std::vector<int32_t> ord(N);
  {
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t k = 0; k < N; ++k) ord[fill[r[k]]++] = (int32_t)k;
  }
  CooPlan P;
  P.sp.reserve(N + 1);
  P.src.reserve(N);
  P.drow.reserve(N);
  P.dcol.reserve(N);
  P.rp.assign(nrow + 1, 0);
  for (int i = 0; i < nrow; ++i) {
    const auto b = ord.begin() + start[i], e = ord.begin() + start[i + 1];
    if (!std::is_sorted(b, e, [&](int32_t x, int32_t y) { return c[x] < c[y]; }))
      std::stable_sort(b, e, [&](int32_t x, int32_t y) { return c[x] < c[y]; });
    for (auto it = b; it != e; ++it) {
      if (it == b || c[*it] != c[*(it - 1)]) {
        P.sp.push_back((int32_t)P.src.size());
        P.drow.push_back(i);
        P.dcol.push_back(c[*it]);
      }
      if (id[*it] >= 0) P.src.push_back(id[*it]);
    }
    P.rp[i + 1] = (int64_t)P.drow.size();
  }
  P.sp.push_back((int32_t)P.src.size());
  return P;
}

RefreshPlan build_refresh_plan(const QPHost& P, const madipm_qp& q) {
  const int nx = P.nx, m = P.m, n = P.n;
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  MADIPM_REQUIRE(q.nvar == nx && q.ncon == m && q.nnzj == na && q.nnzh == nh,
                 "madipm_solver_prepare_update: nvar / ncon / nnzj / nnzh differ from the problem the solver was "
                 "created with");
  MADIPM_REQUIRE(na == 0 || (q.Arows && q.Acols && q.Avals), "madipm_solver_prepare_update: null A arrays");
  MADIPM_REQUIRE(na + P.ns < INT32_MAX && 2 * nh < INT32_MAX && P.nnzK < INT32_MAX,
                 "madipm_solver_prepare_update: the refresh plan has 32-bit indices (nnz < 2^31)");
  RefreshPlan R;
  R.Ar.assign(q.Arows, q.Arows + na);
  R.Ac.assign(q.Acols, q.Acols + na);
  R.Av.assign(q.Avals, q.Avals + na);
  for (int64_t k = 0; k < na; ++k)
    MADIPM_REQUIRE(R.Ar[k] >= 0 && R.Ar[k] < m && R.Ac[k] >= 0 && R.Ac[k] < nx,
                   "madipm_solver_prepare_update: A index out of range");
  // ---- J^T (n x m): the COO build_structure reads (fixed columns dropped, one -1 per slack column), transposed
  std::vector<int32_t> er, ec, id;
  er.reserve(na + P.ns);
  ec.reserve(na + P.ns);
  id.reserve(na + P.ns);
  for (int64_t k = 0; k < na; ++k) {
    if (P.fixed[R.Ac[k]]) continue;
    er.push_back(R.Ar[k]);
    ec.push_back(R.Ac[k]);
    id.push_back((int32_t)k);
  }
  for (int k = 0; k < P.ns; ++k) {
    er.push_back(P.ind_ineq[k]);
    ec.push_back(nx + k);
    id.push_back(-1);
  }
  CooPlan T = coo_plan(n, ec, er, id);
  const int64_t nJ = (int64_t)T.drow.size();
  std::vector<int32_t>().swap(er);
  std::vector<int32_t>().swap(ec);
  std::vector<int32_t>().swap(id);
  // J's entries sorted by (row, column) = J^T's, bucketed by their column index in ascending order
  R.j2jt.resize(nJ);
  {
    std::vector<int64_t> rs(m + 1, 0);
    for (int64_t t = 0; t < nJ; ++t) rs[T.dcol[t] + 1]++;
    for (int i = 0; i < m; ++i) rs[i + 1] += rs[i];
    for (int64_t t = 0; t < nJ; ++t) R.j2jt[rs[T.dcol[t]]++] = (int32_t)t;
  }
  // ---- H (n x n, symmetric): an off-diagonal source feeds (r, c) and (c, r); fixed rows / columns feed none
  std::vector<int32_t> hr, hc, hid;
  for (int64_t k = 0; k < nh; ++k) {
    const int r = P.Hr[k], c = P.Hc[k];
    if (P.fixed[r] || P.fixed[c]) continue;
    hr.push_back(r);
    hc.push_back(c);
    hid.push_back((int32_t)k);
    if (r != c) {
      hr.push_back(c);
      hc.push_back(r);
      hid.push_back((int32_t)k);
    }
  }
  CooPlan Hp = coo_plan(n, hr, hc, hid);
  const int64_t nH = (int64_t)Hp.drow.size();
  // the plan must address exactly the arrays the constructor laid out
  MADIPM_REQUIRE(nJ == P.nJ && nH == P.nH,
                 "madipm_solver_prepare_update: the index arrays are not the ones the solver was created with");
  const std::vector<int64_t> Kcp = k2_colptr(n, m, Hp.rp.data(), Hp.dcol.data(), T.rp.data());
  MADIPM_REQUIRE(Kcp[n + m] == P.nnzK,
                 "madipm_solver_prepare_update: the index arrays are not the ones the solver was created with");
  R.hk.assign(nH, -1);
  R.hdpos.assign(n, -1);
  R.jtk.resize(nJ);
  {
    std::vector<int64_t> nxt(n);
    for (int j = 0; j < n; ++j) nxt[j] = Kcp[j] + 1;
    for (int64_t t = 0; t < nH; ++t) {
      const int i = Hp.drow[t], j = Hp.dcol[t];
      if (j > i) R.hk[t] = (int32_t)nxt[i]++;
      if (j == i) R.hdpos[i] = (int32_t)t;
    }
    for (int64_t t = 0; t < nJ; ++t) R.jtk[t] = (int32_t)nxt[T.drow[t]]++;
  }
  R.tsp = std::move(T.sp);
  R.tsrc = std::move(T.src);
  R.hsp = std::move(Hp.sp);
  R.hsrc = std::move(Hp.src);
  R.nJ = nJ;
  R.nH = nH;
  return R;
}

RouteLists build_route_lists(const QPHost& P) {
  const int nx = P.nx, m = P.m;
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  RouteLists L;
  {
    std::vector<int32_t> dest(na);
    std::vector<I2> ent(na);
    for (int64_t k = 0; k < na; ++k) {
      dest[k] = P.Ar[k];
      ent[k] = {(int32_t)k, P.Ac[k]};
    }
    bucket(m, dest, ent, L.asp, L.ae);
  }
  fixed_column_lists(P, m, [](int r, int) { return r; }, [](int, int c) { return c; }, L.fsp, L.fe);
  {
    std::vector<int32_t> gdest;
    std::vector<I2> gent;
    for (int64_t k = 0; k < nh; ++k) {
      const int r = P.Hr[k], c = P.Hc[k];
      gdest.push_back(r);
      gent.push_back({(int32_t)k, c});
      if (r != c) {
        gdest.push_back(c);
        gent.push_back({(int32_t)k, r});
      }
      if (P.fixed[r] && P.fixed[c]) {
        L.bfk.push_back((int32_t)k);
        L.bfrc.push_back({r, c});
      }
    }
    bucket(nx, gdest, gent, L.gsp, L.ge);
  }
  fixed_free_lists(P, nx, [](int, int fr) { return fr; }, [](int fx, int) { return fx; }, L.xsp, L.xe);
  L.vcls.resize(nx);
  L.ccls.resize(m);
  for (int i = 0; i < nx; ++i) L.vcls[i] = (uint8_t)bound_class(P.lvar[i], P.uvar[i]);
  for (int i = 0; i < m; ++i) L.ccls[i] = (uint8_t)bound_class(P.lcon[i], P.ucon[i]);
  return L;
}

std::vector<int32_t> adjoint_rowslack(const QPHost& P) {
  std::vector<int32_t> rs(std::max(P.m, 1), -1);
  for (int k = 0; k < P.ns; ++k) rs[P.ind_ineq[k]] = P.nx + k;
  return rs;
}

AdjointLists build_adjoint_lists(const QPHost& P) {
  AdjointLists L;
  std::vector<int32_t> tof(P.nx, -1);  // variable -> its place in fix
  for (int i = 0; i < P.nx; ++i)
    if (P.fixed[i]) {
      tof[i] = (int32_t)L.fix.size();
      L.fix.push_back(i);
    }
  const int nf = (int)L.fix.size();
  fixed_free_lists(P, nf, [&](int fx, int) { return tof[fx]; }, [](int, int fr) { return fr; }, L.fhsp, L.fh);
  fixed_column_lists(P, nf, [&](int, int c) { return tof[c]; }, [](int r, int) { return r; }, L.fasp, L.fa);
  return L;
}

TangentLists build_tangent_lists(const QPHost& P) {
  const int nx = P.nx, m = P.m;
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  TangentLists L;
  {
    std::vector<int32_t> rdest(na), cdest(na);
    std::vector<I2> rent(na), cent(na);
    for (int64_t k = 0; k < na; ++k) {
      rdest[k] = P.Ar[k];
      rent[k] = {(int32_t)k, P.Ac[k]};
      cdest[k] = P.Ac[k];
      cent[k] = {(int32_t)k, P.Ar[k]};
    }
    bucket(m, rdest, rent, L.asp, L.ae);
    bucket(nx, cdest, cent, L.csp, L.ce);
  }
  std::vector<int32_t> gdest;
  std::vector<I2> gent;
  for (int64_t k = 0; k < nh; ++k) {
    const int r = P.Hr[k], c = P.Hc[k];
    gdest.push_back(r);
    gent.push_back({(int32_t)k, c});
    if (r != c) {
      gdest.push_back(c);
      gent.push_back({(int32_t)k, r});
    }
  }
  bucket(nx, gdest, gent, L.gsp, L.ge);
  return L;
}

}  // namespace madipm
