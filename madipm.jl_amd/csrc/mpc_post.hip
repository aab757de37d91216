// The post-solve calls of the MPC driver: adjoint gradients, forward-mode tangents and the active-set polish
// (DESIGN §13c-§13g).  Each reads the end point of a finished solve, factorises once per point and leaves
// alone everything a later initialize / solve / warm_start_last reads; the interior-point loop (mpc.hip)
// knows nothing of the state kept here.  The active-set solve (§13h) runs the polish's kernels on the data the
// solver holds, from a start that reads no end point, and so needs no solve at all.  The adjoint's and the
// tangent's kernels take a column from blockIdx.y: a single call is one column, a batched call (§13i) up to
// SENS_W of them, and both run the one host path at the end of the file.  Kernels and what they share with the
// loop's: mpc_kernels.hpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "mpc_kernels.hpp"

namespace madipm {

// The host route's staging of a group of optional blocks (null: not given / not wanted).  bind() gives the
// pointers the kernels use: the caller's own on the device route, else a staging buffer, allocated by the
// first call that passes the block and never empty, so a second call with the same blocks allocates nothing.
template <class T, int N>
struct Staged {
  DBuf<T> buf[N];
  template <class P>  // const T* (inputs) or T* (outputs)
  void bind(P const (&user)[N], const int64_t (&len)[N], bool device, P (&dev)[N]) {
    for (int j = 0; j < N; ++j) {
      dev[j] = user[j];
      if (!device && user[j]) {
        if (!buf[j].p) buf[j].alloc(std::max<int64_t>(len[j], 1));
        dev[j] = buf[j].p;
      }
    }
  }
  void upload(const T* const (&user)[N], const int64_t (&len)[N], hipStream_t s) {
    for (int j = 0; j < N; ++j)
      if (user[j] && len[j]) buf[j].upload(user[j], len[j], s);
  }
  // sync = false: the caller enqueues more copies and synchronises after the last
  void download(T* const (&user)[N], const int64_t (&len)[N], hipStream_t s, bool sync = true) {
    for (int j = 0; j < N; ++j)
      if (user[j] && len[j]) MADIPM_HIP(hipMemcpyAsync(user[j], buf[j].p, len[j] * sizeof(T), hipMemcpyDeviceToHost, s));
    if (sync) MADIPM_HIP(hipStreamSynchronize(s));
  }
};

// The adjoint gradients (madipm_solver_adjoint*).  Everything here is allocated by the first
// call that needs it: the right-hand side copy, the solution, the per-row residuals and the scalar block by
// the first call (8 B x (nvar + 2 (n + m) + 2)); rowslack (4 B per row) with lcon / ucon; A's COO indices (8 B per entry)
// with Avals; H's (8 B per entry) with Hvals; the fixed variables' entry lists (8 B per entry of A in a
// fixed column and per entry of H between a fixed and a free variable, 4 B per fixed variable for each
// list start) with lvar on a problem that has fixed variables; the host route's output staging (8 B per
// output entry) with each output it is asked for.
struct Adjoint {
  DBuf<double> sol, rowres, scal;         // a~ (refined); |g - K a~| per row; [residual ratio, the single view's scal]
  DBuf<int32_t> rowslack;                 // row -> its slack (index into [nx, n)) or -1 (equality row)
  DBuf<int32_t> Ar, Ac, Hr, Hc;           // COO indices, creation-time entry order
  DBuf<int32_t> fix, fhsp, fasp;          // fixed variables; their list starts into fh / fa
  DBuf<int2> fh, fa;                      // (entry of Hvals, free endpoint), (entry of Avals, row)
  int nfix = -1;                          // -1: lists not built yet
  Staged<double, 7> out;                  // host route: c, Hvals, Avals, lcon, ucon, lvar, uvar
  // the loss of all five blocks (§13d), by the first call with a cotangent other than gx: 8 B x (n + m + nvar)
  DBuf<double> shift, apx;                // v = [q~; 0; gcons / con_scale]; a~'x of the shifted system
  Staged<double, 5> ct;                   // host route's gx, gy, gzl, gzu, gcons
  int64_t n_adjoints = 0, n_fact = 0;
  int64_t fact_solve = -1;                // n_solves_ of the point the LDL^T currently holds the factor of
};

// The tangent (madipm_solver_tangent*) shares the adjoint's factor, solution and residual
// rows.  Its own, each allocated by the first call that needs it: the data terms and the full dx
// (8 B x (2 n + m + 1)); the shift vector is the adjoint's `shift`; rowslack as there; with Hvals / Avals (or
// lvar on a problem with fixed variables) the entry lists of build_tangent_lists: 16 B per entry of A, 8 B per
// endpoint of a stored entry of H, 4 B x (2 nvar + ncon) list starts; the host route's staging of the
// directions given and the outputs wanted (8 B per entry).
struct Tangent {
  DBuf<double> base, dx, scal;            // data terms of the right-hand side; [dx; 0]; residual ratio
  DBuf<int32_t> asp, csp, gsp;            // list starts: A per row, A per column, H per endpoint
  DBuf<int2> ae, ce, ge;                  // (entry, column), (entry, row), (entry, other endpoint)
  bool lists = false;
  Staged<double, 7> dir;                  // host route: c, Hvals, Avals, lcon, ucon, lvar, uvar
  Staged<double, 5> out;                  // host route: x, y, zl, zu, cons
  int64_t n_tangents = 0;
};

// The polish (madipm_solver_polish*) shares the adjoint's residual rows and rowslack (and
// overwrites its factor: sens_factor and polish() clear each other's tag).  Its own, allocated by the first
// call: the scratch point [v; y], the gradient of the Lagrangian on [x; s], the raw bounds of [x; s] in the
// public space, the partial measures and the row values (8 B x (4 n + 2 m)); the codes of this call and of the
// factor held (2 n B); the slack -> row map (4 B per slack); the host route's staging of the set and the
// outputs.
struct PolMeasures {  // k_pol_verdict's result, read back with one copy
  int32_t verdict, n_active;
  double residual, min_multiplier, min_gap;
  double max_multiplier;                  // the largest |active multiplier|: the active-set solve's M (§13h)
};
struct Polish {
  DBuf<double> w, grad, lo, hi, part, ax;
  DBuf<int8_t> codes, codes_fact;
  DBuf<int32_t> ineq, flags;              // flags: [a bad code was supplied, the codes differ from the factor's]
  DBuf<PolMeasures> meas;
  Staged<double, 5> out;                  // host route: x, y, zl, zu, cons
  Staged<int8_t, 2> set_in, set_out;      // host route: the codes per variable and per row, supplied / returned
  int64_t bounds_updates = -1;            // n_updates_ of the bounds in lo / hi
  int64_t fact_solve = -1;                // n_solves_ of the point the LDL^T holds the polish factor of
  double fact_sigma = 0.0;
  int64_t point_solve = -1;               // n_solves_ of the point w / codes / grad belong to (-1: none, or a polish threw)
  int refine_steps = 0;                   // of that polish
  madipm_polish_info last{-1, 0, 0.0, 0.0, 0.0, 0, 0};
  // the rest of the factor's tag: the data (n_updates_) it was made of, and its place among the factorisations
  // enqueued (n_factor_calls_: nothing has taken the LDL^T since)
  int64_t fact_updates = -1, fact_calls = -1;
  // The active-set solve (madipm_solver_active_set_solve*), allocated with the rest: the kept set
  // (the codes of the last polish or active-set solve that ended POLISHED) and the starting set of the call
  // (2 n B), the count of changed codes.  as_*: the data and the state the current active-set point belongs to.
  DBuf<int8_t> codes_kept, codes0;
  DBuf<int32_t> changed;
  bool kept = false, as_point = false;
  int64_t as_updates = -1, as_solves = -1, as_inits = -1;
  madipm_active_set_info as_last{-1, 0, 0, 0, 0.0, 0.0, 0.0, 0, 0};
};

// The sensitivities at the polished point (madipm_solver_tangent_polished* / _adjoint_polished*)
// read the polish's scratch point, codes and factor and share the tangent's data terms and lists, the adjoint's
// index lists and residual rows.  Their own, allocated by the first call: the solution u and the right-hand
// side (8 B x 2 (n + m)), K0 u - rhs on the active coordinates (8 B x n), the residual scalar; the host route's
// staging of the blocks given and wanted.
struct PolSens {
  DBuf<double> u, rhs, keep, scal;
  Staged<double, 7> dir, grad;            // host route: c, Hvals, Avals, lcon, ucon, lvar, uvar
  Staged<double, 5> out, ct;              // host route: x, y, zl, zu, cons
  int64_t n_tangents = 0, n_adjoints = 0, n_fact = 0;
};

// The batched sensitivities (madipm_solver_tangent_batch / _adjoint_batch) keep SENS_W columns of
// the single calls' scratch (SensView names which buffer stands for which), column-contiguous (column j of a buffer of vectors of length len starts at j len), so
// that the LDL^T solves one column in place.  Each part by the first batched call that needs it: the solve's
// vector, the kept right-hand side, the solution, the residual rows and the columns' ratios (8 B x W x (4 (n + m)
// + 1)); the shift vector and a~'x with the tangent or a cotangent other than gx (8 B x W x (n + m + nvar)); the
// data terms and the full dx with the tangent (8 B x W x (2 n + m)); the host route's staging of one chunk.
constexpr int SENS_W = 8;
struct SensBatch {
  DBuf<double> d, p, sol, rowres, scal;
  DBuf<double> shift, apx, base, dx;
  Staged<double, 7> dir, grad;            // host route: c, Hvals, Avals, lcon, ucon, lvar, uvar
  Staged<double, 5> out, ct;              // host route: x, y, zl, zu, cons
  int64_t n_batches = 0, n_columns = 0, n_chunks = 0;
  void count(int64_t k, int64_t chunks) { ++n_batches, n_columns += k, n_chunks += chunks; }
  // N = n + m.  shifted: the tangent, or a cotangent other than gx; tangent: its data terms and dx
  void need(int64_t N, int nx, int n, bool shifted, bool tangent) {
    const auto cols = [](int64_t len) { return std::max<int64_t>(SENS_W * len, 1); };
    if (!d.p) {
      d.alloc(cols(N));
      p.alloc(cols(N));
      sol.alloc(cols(N));
      rowres.alloc(cols(N));
      scal.alloc(SENS_W);
    }
    if (shifted && !shift.p) {
      shift.alloc(cols(N));
      apx.alloc(cols(nx));
    }
    if (tangent && !base.p) {
      base.alloc(cols(N));
      dx.alloc(cols(n));
    }
  }
};

// The scratch one tangent or adjoint call runs on: W columns of each vector, column j of a vector of length len
// at j len, and the host route's staging of a chunk.  A single call's view (W = 1) is over the solver's own d / p
// and the Adjoint's and Tangent's buffers, so it writes exactly the vectors it always wrote; a batched call's is
// over SensBatch.  scal: the columns' residual ratios of a chunk that is folded (never the single call's).
struct SensView {
  int W;
  double *d, *p, *sol, *rowres, *scal;    // the solves' vectors; the kept right-hand sides; a~; |g - K a~|; ratios
  double *shift, *apx, *base, *dx;        // null where the call has no use for them
  Staged<double, 7>*dir, *grad;           // the tangent's directions, the adjoint's gradients
  Staged<double, 5>*out, *ct;             // the tangent's outputs, the adjoint's cotangents
};

// What the calls keep between them, created by the first of them; the tangent, the polish and the polished
// sensitivities allocate their own parts in their first call.
struct AdjArgs;
struct PostSolve {
  Adjoint adj;
  Tangent tan;
  Polish pol;
  PolSens sens;
  SensBatch bat;
  StreamHandoff sync;  // the device routes of all of them
  AdjArgs args(MPCSolver& S);
  // the adjoint's COO indices and fixed-variable lists, the tangent's data terms and entry lists: each by the
  // first call that needs it
  void adjoint_lists(MPCSolver& S, bool needA, bool needH, bool needFix);
  void tangent_scratch(MPCSolver& S, bool needLists);
  // row -> slack; the shift vector and a~'x: by the first call that needs them
  const int32_t* rowslack(const QPHost& P, hipStream_t s) {
    if (!adj.rowslack.p) {
      adj.rowslack.upload(adjoint_rowslack(P), s);
      MADIPM_HIP(hipStreamSynchronize(s));
    }
    return adj.rowslack.p;
  }
  void need_shift(int N, int nx) {
    if (adj.shift.p) return;
    adj.shift.alloc(std::max(N, 1));
    adj.apx.alloc(std::max(nx, 1));
  }
  // shifted: the tangent, or a cotangent other than gx; tangent: after tangent_scratch.  Allocates what the
  // view lacks: the shift vector and a~'x of a single call, the parts of SensBatch of a batched one.
  SensView sens_view(MPCSolver& S, bool batch, bool shifted, bool tangent);
};
void PostSolveDelete::operator()(PostSolve* p) const { delete p; }

}  // namespace madipm

// ======================================================================= adjoint gradients
// madipm_solver_adjoint / _adjoint_device: with gx = dl/dx* at the end point of a successful solve, one
// solve with the K2 matrix of that point, K a~ = [gx on the free variables; 0; 0] in the solver's scaled
// space, gives a = (ax, as, ay) = (obj_scale a~x, obj_scale a~s / con_scale, con_scale a~y) of the public
// space, and every gradient is a product of entries of a with entries of the solution.  One thread (the
// residual: one lane group) per output, every sum in a fixed order, no atomics: the same bits run to run.
// madipm_solver_adjoint_full / _full_device: the loss also depends on y, zl, zu and A x.  The
// same factor and refinement with the shifted right-hand side K a~' = g' (k_adj_shift, k_adj_rhs_full),
// a~ = a~' - [q~; 0; 0] (k_adj_unshift), and the <true> instantiations of the gradient kernels.
namespace madipm {

struct AdjArgs {
  int n, m, nx;
  double os, sgn;                                  // obj_scale; +1 minimize, -1 maximize
  const double *d, *x, *xl, *xu, *zl, *zu, *y;     // a~ = [a~x; a~s; a~y]; the iterate (scaled space)
  const double* cscale;                            // con_scale
  const int32_t *lbpos, *ubpos;
  const uint8_t* fixed;
};

namespace {

__device__ __forceinline__ double adj_ax(const AdjArgs& A, int i) { return A.fixed[i] ? 0.0 : A.os * A.d[i]; }
__device__ __forceinline__ double adj_ay(const AdjArgs& A, int r) { return A.cscale[r] * A.d[A.n + r]; }
// Sigma_l, Sigma_u of coordinate i of [x; s] in the scaled space (k_diag's terms of pr_diag); 0 without the bound
__device__ __forceinline__ double adj_sig_l(const AdjArgs& A, int i) {
  return A.lbpos[i] >= 0 ? A.zl[i] / (A.x[i] - A.xl[i]) : 0.0;
}
__device__ __forceinline__ double adj_sig_u(const AdjArgs& A, int i) {
  return A.ubpos[i] >= 0 ? A.zu[i] / (A.xu[i] - A.x[i]) : 0.0;
}

// The loss of all five blocks: the cotangents besides gx (any may be null: 0), and a~'x, the
// x part of the shifted system's solution, which the bound gradients of the free variables are formed from.
struct AdjFull {
  const double *gzl, *gzu, *gcons;
  const double* apx;
};
// a bound the variable does not have makes its multiplier a constant: that cotangent is not read
__device__ __forceinline__ double adj_gzl(const AdjArgs& A, const AdjFull& F, int i) {
  return (F.gzl && A.lbpos[i] >= 0) ? F.gzl[i] : 0.0;
}
__device__ __forceinline__ double adj_gzu(const AdjArgs& A, const AdjFull& F, int i) {
  return (F.gzu && A.ubpos[i] >= 0) ? F.gzu[i] : 0.0;
}

// The kernels below and the tangent's (§13e) work on column blockIdx.y of a call's blocks and scratch (§13i): a
// single call launches them with gridDim.y == 1, a batched one with a chunk's columns.  Arguments named ...b and
// the structs named ...0 hold the first column; column j of a block of vectors of length len starts at j len.
struct BLen {  // entries of Hvals / Avals: the column strides the kernels cannot read from AdjArgs
  int64_t nh, na;
};
// column j of a block of vectors of length len (null stays null)
__device__ __forceinline__ const double* bcol(const double* p, int j, int64_t len) { return p ? p + j * len : nullptr; }
__device__ __forceinline__ double* bcol(double* p, int j, int64_t len) { return p ? p + j * len : nullptr; }
__device__ __forceinline__ AdjArgs adj_col(AdjArgs A, int j) {  // a~ of column j
  A.d = A.d + j * ((int64_t)A.n + A.m);
  return A;
}
__device__ __forceinline__ AdjFull full_col(const AdjFull& F, const AdjArgs& A, int j) {
  return AdjFull{bcol(F.gzl, j, A.nx), bcol(F.gzu, j, A.nx), bcol(F.gcons, j, A.m), bcol(F.apx, j, A.nx)};
}

// v = [q~; 0; gcons / con_scale], the vector the shifted right-hand side applies K's blocks to:
// q_i = (Sigma_l gzl - Sigma_u gzu)_i / (Sigma_l + Sigma_u)_i on a free variable with a bound, else 0 (the
// scalings cancel in q), q~ = q / obj_scale.  The slack entries are written 0: their J~^T row is not empty.
__global__ __launch_bounds__(NT) void k_adj_shift(AdjArgs A, AdjFull F0, double* __restrict__ vb, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ldl_status_end(t1);
  const int col = blockIdx.y;
  const AdjFull F = full_col(F0, A, col);
  double* __restrict__ v = vb + col * ((int64_t)A.n + A.m);
  GRID_LOOP(i, A.n + A.m) {
    double o = 0.0;
    if (i < A.nx) {
      if (!A.fixed[i]) {
        const double sl = adj_sig_l(A, (int)i), su = adj_sig_u(A, (int)i), sm = sl + su;
        if (sm > 0.0) o = ((sl * adj_gzl(A, F, (int)i) - su * adj_gzu(A, F, (int)i)) / sm) / A.os;
      }
    } else if (i >= A.n && F.gcons) {
      o = F.gcons[i - A.n] / A.cscale[i - A.n];
    }
    v[i] = o;
  }
}

// The shifted right-hand side into bd (the solve's vector: the solver's d in a single call) and bp (which keeps
// it for the residual: the solver's p), k_adj_resid's access pattern applied to v: gx + H~ q~ +
// J~^T (gcons / con_scale) on a free variable, 0 on a fixed one and on a slack, con_scale_r gy_r / obj_scale +
// J~_r q~ on row r.  Every entry is of the cotangents' magnitude: the Sigma terms of the plain form, 1e8 and more
// at an active bound, have cancelled in the algebra.
template <int G>
__global__ __launch_bounds__(NT) void k_adj_rhs_full(DV D, AdjArgs A, const double* __restrict__ gxb,
                                                     const double* __restrict__ gyb, const double* __restrict__ vb,
                                                     double* __restrict__ bd, double* __restrict__ bp) {
#pragma clang fp contract(off)
  const int n = D.n, m = D.m;
  const int col = blockIdx.y;
  const int64_t off = col * ((int64_t)n + m);
  const double* __restrict__ gx = bcol(gxb, col, D.nx);
  const double* __restrict__ gy = bcol(gyb, col, m);
  const double* __restrict__ v = vb + off;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  GROUP_LOOP(i, n + m, G) {
    double g = 0.0;
    if (i < n) {
      if (i < D.nx && !D.fixed[i]) {
        double hd, jd;
        gdot2<G>(D.H, i, v, D.JT, i, v + n, hd, jd);
        g = (gx ? gx[i] : 0.0) + (hd + jd);
      }
    } else {
      const double jq = gdot<G>(D.J, i - n, v);
      g = (gy ? A.cscale[i - n] * gy[i - n] / A.os : 0.0) + jq;
    }
    if (lead) {
      bd[off + i] = g;
      bp[off + i] = g;
    }
  }
}

// a~ = a~' - [q~; 0; 0], with a~'x kept for the bound gradients
__global__ __launch_bounds__(NT) void k_adj_unshift(int nx, int64_t N, const double* __restrict__ vb,
                                                    double* __restrict__ solb, double* __restrict__ apxb) {
  const int col = blockIdx.y;
  const double* __restrict__ v = vb + col * N;
  double* __restrict__ sol = solb + col * N;
  double* __restrict__ apx = apxb + col * (int64_t)nx;
  GRID_LOOP(i, nx) {
    const double ap = sol[i];
    apx[i] = ap;
    sol[i] = ap - v[i];
  }
}

// gx into bd's K2 layout (and into bp, which keeps it for the residual): zero on fixed variables, slacks, rows
// t1 != nullptr: the factorisation before this launch ended (LinSolver::lazy_inertia), as in k_rhs
__global__ __launch_bounds__(NT) void k_adj_rhs(DV D, const double* __restrict__ gxb, double* __restrict__ bd,
                                                double* __restrict__ bp, LDLStatus* t1) {
  if (t1 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ldl_status_end(t1);
  const int col = blockIdx.y;
  const int64_t off = col * ((int64_t)D.n + D.m);
  const double* __restrict__ gx = gxb + col * (int64_t)D.nx;
  GRID_LOOP(i, D.n + D.m) {
    const double v = (i < D.nx && !D.fixed[i]) ? gx[i] : 0.0;
    bd[off + i] = v;
    bp[off + i] = v;
  }
}

// r = g - K v and |r| of every row, K the K2 matrix of the point WITHOUT the regularisation the factor carries:
// H, J^T and Sigma_l + Sigma_u on a primal row, J on a dual row (k_residual's operator with the bound blocks
// folded into Sigma).  g = the kept right-hand side; v = the current a~; r (may be null) becomes the right-hand
// side of a refinement solve.  One column: a chunk of more runs k_adj_resid_b (§13i, at the end of the file).
template <int G>
__global__ __launch_bounds__(NT) void k_adj_resid(DV D, AdjArgs A, const double* __restrict__ g,
                                                  const double* __restrict__ v, double* __restrict__ r,
                                                  double* __restrict__ rowres) {
  const int n = D.n, m = D.m;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  GROUP_LOOP(i, n + m, G) {
    const double gi = g[i];
    double kv;
    if (i < n) {
      double hd, jd;
      gdot2<G>(D.H, i, v, D.JT, i, v + n, hd, jd);
      kv = (hd + jd) + (adj_sig_l(A, (int)i) + adj_sig_u(A, (int)i)) * v[i];
    } else {
      kv = gdot<G>(D.J, i - n, v);
    }
    if (lead) {
      const double ri = gi - kv;
      if (r) r[i] = ri;
      rowres[i] = fabs(ri);
    }
  }
}

// a~ = d (first) or a~ += d: the solve's result, then each refinement's correction
__global__ __launch_bounds__(NT) void k_adj_acc(double* __restrict__ acc, const double* __restrict__ d, int64_t N,
                                                int first) {
  GRID_LOOP(i, N) acc[i] = first ? d[i] : acc[i] + d[i];
}

// Column blockIdx.x: out[column] = max_i rowres[i] / max(1, max_i |g_i|): one block, each thread a strided slice,
// then an LDS tree (a maximum does not depend on the order; a NaN is kept).  gb == null: the plain maximum.
__global__ __launch_bounds__(NT) void k_adj_resmax(const double* __restrict__ rowresb, const double* __restrict__ gb,
                                                   int64_t N, double* __restrict__ out) {
  __shared__ double sw[NT], sg[NT];
  const int t = threadIdx.x;
  const double* __restrict__ rowres = rowresb + blockIdx.x * N;
  const double* __restrict__ g = bcol(gb, blockIdx.x, N);
  double w = 0.0, gm = 0.0;
  if (g) {  // tested outside the loop, which is a third of a call's time on a large problem (one block, N trips / NT)
    for (int64_t i = t; i < N; i += NT) {
      w = nmax(w, rowres[i]);
      gm = nmax(gm, fabs(g[i]));
    }
  } else {
    for (int64_t i = t; i < N; i += NT) w = nmax(w, rowres[i]);
  }
  sw[t] = w;
  sg[t] = gm;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (t < o) {
      sw[t] = nmax(sw[t], sw[t + o]);
      sg[t] = nmax(sg[t], sg[t + o]);
    }
    __syncthreads();
  }
  if (t == 0) out[blockIdx.x] = sw[0] / (sg[0] > 1.0 ? sg[0] : 1.0);
}

// The vector gradients (any output may be null).  Variable i: c_i = -sgn ax_i; a free one:
// lvar_i = Sigma_l,i ax_i = Sigma~_l,i a~x_i and uvar_i likewise (the scalings cancel); a fixed one: uvar_i = 0
// (lvar_i is k_adj_fix's).  Row i: an equality row lcon_i = ay_i, ucon_i = 0; a row with slack k:
// lcon_i = Sigma_l,k as_k = con_scale_i Sigma~_l,k a~s_k and ucon_i likewise.
// FULL (§13d; A.d is the un-shifted a~): a free variable's bounds in the shifted form,
// lvar_i = Sigma~_l,i a~'x_i + h_i (gzl_i + gzu_i), uvar_i = Sigma~_u,i a~'x_i - h_i (gzl_i + gzu_i),
// h_i = Sigma~_l Sigma~_u / (Sigma~_l + Sigma~_u) / obj_scale (0 where the sum is 0).
template <bool FULL>
__global__ __launch_bounds__(NT) void k_adj_vec(AdjArgs A0, AdjFull F0, const int32_t* __restrict__ rowslack,
                                                double* __restrict__ gcb, double* __restrict__ glvb,
                                                double* __restrict__ guvb, double* __restrict__ glcb,
                                                double* __restrict__ gucb) {
#pragma clang fp contract(off)
  const int col = blockIdx.y;
  const AdjArgs A = adj_col(A0, col);
  const AdjFull F = full_col(F0, A, col);
  double* __restrict__ gc = bcol(gcb, col, A.nx);
  double* __restrict__ glv = bcol(glvb, col, A.nx);
  double* __restrict__ guv = bcol(guvb, col, A.nx);
  double* __restrict__ glc = bcol(glcb, col, A.m);
  double* __restrict__ guc = bcol(gucb, col, A.m);
  GRID_LOOP(i, (A.nx > A.m ? A.nx : A.m)) {
    if (i < A.nx) {
      const bool fx = A.fixed[i];
      const double at = fx ? 0.0 : A.d[i];
      if (gc) gc[i] = -(A.sgn * (A.os * at));
      if (!fx) {
        if constexpr (FULL) {
          const double sl = adj_sig_l(A, (int)i), su = adj_sig_u(A, (int)i), sm = sl + su;
          const double ap = F.apx[i];
          const double hg = sm > 0.0 ? (sl * su / sm) / A.os * (adj_gzl(A, F, (int)i) + adj_gzu(A, F, (int)i)) : 0.0;
          if (glv) glv[i] = sl * ap + hg;
          if (guv) guv[i] = su * ap - hg;
        } else {
          if (glv) glv[i] = adj_sig_l(A, (int)i) * at;
          if (guv) guv[i] = adj_sig_u(A, (int)i) * at;
        }
      } else if (guv) {
        guv[i] = 0.0;
      }
    }
    if (i < A.m && (glc || guc)) {
      const int k = rowslack[i];
      const double cs = A.cscale[i];
      if (k < 0) {
        if (glc) glc[i] = cs * A.d[A.n + i];
        if (guc) guc[i] = 0.0;
      } else {
        const double as = A.d[k];
        if (glc) glc[i] = cs * (adj_sig_l(A, k) * as);
        if (guc) guc[i] = cs * (adj_sig_u(A, k) * as);
      }
    }
  }
}

// Avals[k], entry (r, c): -(ax_c y_r + ay_r x_c), y the public multiplier (k_unscale's rounding)
// FULL: + gcons_r x_c, the entry's own part of (A x)_r
template <bool FULL>
__global__ __launch_bounds__(NT) void k_adj_avals(AdjArgs A0, AdjFull F0, int64_t nnz, const int32_t* __restrict__ Ar,
                                                  const int32_t* __restrict__ Ac, double* __restrict__ outb) {
#pragma clang fp contract(off)
  const int col = blockIdx.y;
  const AdjArgs A = adj_col(A0, col);
  const AdjFull F = full_col(F0, A, col);
  double* __restrict__ out = outb + col * nnz;
  GRID_LOOP(k, nnz) {
    const int r = Ar[k], c = Ac[k];
    const double yr = A.y[r] * A.cscale[r] / A.os;
    const double v = -(adj_ax(A, c) * yr + adj_ay(A, r) * A.x[c]);
    if constexpr (FULL)
      out[k] = F.gcons ? v + F.gcons[r] * A.x[c] : v;
    else
      out[k] = v;
  }
}

// Hvals[k], entry (r, c) of the lower triangle: -sgn ax_r x_r on the diagonal, -sgn (ax_r x_c + ax_c x_r) off it
__global__ __launch_bounds__(NT) void k_adj_hvals(AdjArgs A0, int64_t nnz, const int32_t* __restrict__ Hr,
                                                  const int32_t* __restrict__ Hc, double* __restrict__ outb) {
#pragma clang fp contract(off)
  const int col = blockIdx.y;
  const AdjArgs A = adj_col(A0, col);
  double* __restrict__ out = outb + col * nnz;
  GRID_LOOP(k, nnz) {
    const int r = Hr[k], c = Hc[k];
    const double ar = adj_ax(A, r);
    const double v = r == c ? ar * A.x[r] : ar * A.x[c] + adj_ax(A, c) * A.x[r];
    out[k] = -(A.sgn * v);
  }
}

// lvar_f of fixed variable f = gx_f - sgn (H ax)_f - (A^T ay)_f, from the raw values: the entries of Hvals
// between f and a free variable, then the entries of Avals in column f, each list in input order
// FULL: gxe_f = gx_f + (A^T gcons)_f in the place of gx_f, over the same list of column f (J~^T has no row
// of a fixed variable), and gx may be null
template <bool FULL>
__global__ __launch_bounds__(NT) void k_adj_fix(AdjArgs A0, AdjFull F0, int nfix, const int32_t* __restrict__ fix,
                                                const int32_t* __restrict__ fhsp, const int2* __restrict__ fh,
                                                const int32_t* __restrict__ fasp, const int2* __restrict__ fa,
                                                const double* __restrict__ Hraw, const double* __restrict__ Araw,
                                                const double* __restrict__ gxb, double* __restrict__ glvb) {
#pragma clang fp contract(off)
  const int col = blockIdx.y;
  const AdjArgs A = adj_col(A0, col);
  const AdjFull F = full_col(F0, A, col);
  const double* __restrict__ gx = bcol(gxb, col, A.nx);
  double* __restrict__ glv = glvb + col * (int64_t)A.nx;
  GRID_LOOP(t, nfix) {
    double hs = 0.0, as = 0.0;
    for (int q = fhsp[t]; q < fhsp[t + 1]; ++q) {
      const int2 e = fh[q];
      hs = hs + Hraw[e.x] * (A.os * A.d[e.y]);
    }
    for (int q = fasp[t]; q < fasp[t + 1]; ++q) {
      const int2 e = fa[q];
      as = as + Araw[e.x] * adj_ay(A, e.y);
    }
    const int f = fix[t];
    if constexpr (FULL) {
      double gs = 0.0;
      if (F.gcons)
        for (int q = fasp[t]; q < fasp[t + 1]; ++q) {
          const int2 e = fa[q];
          gs = gs + Araw[e.x] * F.gcons[e.y];
        }
      glv[f] = ((gx ? gx[f] : 0.0) + gs) - A.sgn * hs - as;
    } else {
      glv[f] = gx[f] - A.sgn * hs - as;
    }
  }
}

}  // namespace

// refinement solves per adjoint: 2, or MADIPM_ADJ_REFINE (0..8; A/B measurements of the refinement)
static int adj_refine_steps() {
  static const int k = [] {
    const char* e = std::getenv("MADIPM_ADJ_REFINE");
    const int v = e ? std::atoi(e) : 2;
    return v < 0 ? 0 : (v > 8 ? 8 : v);
  }();
  return k;
}

// ---- what the adjoint and the tangent (§13e) share: the refusals, the scratch, the factor, the solves
void MPCSolver::sens_refuse(const std::string& who) const {
  MADIPM_REQUIRE(solved_, who + "no solve has run on this solver yet");
  MADIPM_REQUIRE(point_ok_ && !initialized_ && solve_updates_ == n_updates_,
                 who + "an update, update_device or initialize ran since the last solve, so the iterate no longer "
                       "belongs to the problem data (solve first)");
  MADIPM_REQUIRE(status_ == MADIPM_SOLVE_SUCCEEDED, who + "the last solve ended with status " +
                                                        std::to_string(status_) + ", not SOLVE_SUCCEEDED");
  MADIPM_REQUIRE(kkt_ == KKT_K2, who + "only kkt_system = SparseKKTSystem (K2) is supported; the K2.5 and "
                                       "normal-equations formulations are left to a later release");
  MADIPM_REQUIRE(!comm_, who + "a solver created with a communicator (madipm_solver_create_dist) is not supported");
}

PostSolve& MPCSolver::post_state() {
  if (!post_) {
    std::unique_ptr<PostSolve, PostSolveDelete> ps(new PostSolve);
    Adjoint& a = ps->adj;
    a.rowres.alloc(std::max(n_ + m_, 1));
    a.sol.alloc(std::max(n_ + m_, 1));
    a.scal.alloc(2);
    a.scal.zero(stream_);
    post_ = std::move(ps);
  }
  return *post_;
}

// The adjoint kernels' view of the end point and of the solution a~ (adj.sol)
AdjArgs PostSolve::args(MPCSolver& S) {
  return AdjArgs{S.n_,    S.m_,    S.nx_,   S.obj_scale_,         S.H_->sgn,  adj.sol.p,  S.x_.p,    S.xl_.p, S.xu_.p,
                 S.zl_.p, S.zu_.p, S.y_.p,  S.device_con_scale(), S.lbpos_.p, S.ubpos_.p, S.fixed_.p};
}

SensView PostSolve::sens_view(MPCSolver& S, bool batch, bool shifted, bool tangent) {
  if (!batch) {  // adj.scal's second entry is never read: a single call is its own first chunk of one column
    if (shifted) need_shift(S.n_ + S.m_, S.nx_);
    return SensView{1,           S.d_.p,    S.p_.p,     adj.sol.p, adj.rowres.p, adj.scal.p + 1, adj.shift.p,
                    adj.apx.p,   tan.base.p, tan.dx.p,  &tan.dir,  &adj.out,     &tan.out,       &adj.ct};
  }
  SensBatch& b = bat;
  b.need((int64_t)S.n_ + S.m_, S.nx_, S.n_, shifted, tangent);
  return SensView{SENS_W,  b.d.p,    b.p.p,  b.sol.p, b.rowres.p, b.scal.p, b.shift.p,
                  b.apx.p, b.base.p, b.dx.p, &b.dir,  &b.grad,    &b.out,   &b.ct};
}

void PostSolve::adjoint_lists(MPCSolver& S, bool needA, bool needH, bool needFix) {
  Adjoint& a = adj;
  QPHost& P = *S.H_;
  hipStream_t s = S.stream_;
  if (needA && !a.Ar.p) {
    a.Ar.upload(S.plan_->Ar, s);
    a.Ac.upload(S.plan_->Ac, s);
  }
  if (needH && !a.Hr.p) {
    a.Hr.upload(P.Hr, s);
    a.Hc.upload(P.Hc, s);
  }
  if (needFix && a.nfix < 0) {  // the fixed variables' entry lists, from the host COO copies
    AdjointLists L = build_adjoint_lists(P);
    L.fh.resize(std::max<size_t>(L.fh.size(), 1));  // the allocations are never empty
    L.fa.resize(std::max<size_t>(L.fa.size(), 1));
    a.fix.upload(L.fix, s);
    a.fhsp.upload(L.fhsp, s);
    a.fasp.upload(L.fasp, s);
    a.fh.upload(as_int2(L.fh), L.fh.size(), s);
    a.fa.upload(as_int2(L.fa), L.fa.size(), s);
    MADIPM_HIP(hipStreamSynchronize(s));
    a.nfix = (int)L.fix.size();
  }
}

void PostSolve::tangent_scratch(MPCSolver& S, bool needLists) {
  Tangent& t = tan;
  hipStream_t s = S.stream_;
  if (!t.base.p) {
    t.base.alloc(std::max(S.n_ + S.m_, 1));
    t.dx.alloc(std::max(S.n_, 1));
    t.scal.alloc(1);
    t.scal.zero(s);
  }
  if (needLists && !t.lists) {  // the entry lists, from the host COO copies
    TangentLists L = build_tangent_lists(*S.H_);
    L.ae.resize(std::max<size_t>(L.ae.size(), 1));  // the allocations are never empty
    L.ce.resize(std::max<size_t>(L.ce.size(), 1));
    L.ge.resize(std::max<size_t>(L.ge.size(), 1));
    t.asp.upload(L.asp, s);
    t.csp.upload(L.csp, s);
    t.gsp.upload(L.gsp, s);
    t.ae.upload(as_int2(L.ae), L.ae.size(), s);
    t.ce.upload(as_int2(L.ce), L.ce.size(), s);
    t.ge.upload(as_int2(L.ge), L.ge.size(), s);
    MADIPM_HIP(hipStreamSynchronize(s));
    t.lists = true;
  }
}

// factorize_regularized_system!'s trials at the end point: the options' regularisation (Adaptive: the current
// pair, not decayed), x 100 after each failure.  enqueue(dw, dc) writes the KKT diagonal and enqueues one
// factorisation.  false: all three failed.
template <class Enqueue>
bool MPCSolver::factor_trials(Enqueue&& enqueue) {
  double dw = 0.0, dc = 0.0;
  if (opt_.regularization == 1 || (opt_.regularization != 0 && n_inits_ == 0)) {
    dw = opt_.delta_p;  // Adaptive before the first initialize (an active-set solve on a fresh solver): its first pair
    dc = opt_.delta_d;
  } else if (opt_.regularization != 0) {
    dw = adapt_dp_;
    dc = adapt_dd_;
  }
  for (int trial = 0; trial < 3; ++trial) {
    if (trial) {
      dw *= 100.0;
      dc *= 100.0;
    }
    enqueue(dw, dc);
    if (ldl_->status(stream_) == 0) return true;
  }
  return false;
}

// the factor of the K2 matrix at the final iterate: once per solve
void MPCSolver::sens_factor(const std::string& who) {
  Adjoint& a = post_->adj;
  if (a.fact_solve == n_solves_) return;
  a.fact_solve = -1;
  post_->pol.fact_solve = -1;  // the polish's factor (§13f) is overwritten
  if (!factor_trials([&](double dw, double dc) { factor_enqueue(dw, dc); }))
    throw Error(who + "the factorisation of the KKT system at the solution failed in all three trials", -4);
  a.fact_solve = n_solves_;
  ++a.n_fact;
}

void MPCSolver::adjoint(const double* gx, const madipm_qp_gradients& g, bool device, hipStream_t caller) {
  adjoint(madipm_qp_cotangents{gx, nullptr, nullptr, nullptr, nullptr}, g, device, caller, nullptr);
}

// name == nullptr: madipm_solver_adjoint / _adjoint_device (gx alone, which must be given).  One column on the
// single call's scratch (adjoint_cols, §13i).
void MPCSolver::adjoint(const madipm_qp_cotangents& ct, const madipm_qp_gradients& g, bool device,
                        hipStream_t caller, const char* name) {
  const std::string who =
      name ? std::string(name) + ": " : (device ? "madipm_solver_adjoint_device: " : "madipm_solver_adjoint: ");
  adjoint_cols(who, 1, false, false, !name, ct, g, device, caller);
}

// the residual ratio the last call left on the device (0 before the first call)
static void read_residual(double* out, int64_t calls, const double* dev, hipStream_t s) {
  if (!out) return;
  *out = 0.0;
  if (calls) {
    MADIPM_HIP(hipMemcpyAsync(out, dev, sizeof(double), hipMemcpyDeviceToHost, s));
    MADIPM_HIP(hipStreamSynchronize(s));
  }
}

void MPCSolver::adjoint_info(int64_t* n_adjoints, int64_t* n_adjoint_factorizations, double* last_residual) {
  const int64_t calls = post_ ? post_->adj.n_adjoints : 0;
  if (n_adjoints) *n_adjoints = calls;
  if (n_adjoint_factorizations) *n_adjoint_factorizations = post_ ? post_->adj.n_fact : 0;
  read_residual(last_residual, calls, calls ? post_->adj.scal.p : nullptr, stream_);
}

}  // namespace madipm

// ======================================================================= tangent
// madipm_solver_tangent / _tangent_device: forward mode, the transpose of the adjoint.  A direction
// (dc, dHvals, dAvals, dlcon, ducon, dlvar, duvar) of the data moves w = (x_F, s, y) by K dw = -(dF/dtheta) dtheta
// with the K of §13c.  The system is solved in the shifted form, dx_F = dx' + p, ds = ds' + p_s, in which no
// product of Sigma with a direction remains, with the adjoint's factor, refinement and residual.
namespace madipm {
namespace {

struct TanDir {  // the direction blocks on the device (null: 0)
  const double *c, *Hv, *Av, *lcon, *ucon, *lvar, *uvar;
};
// a direction entry of a bound the coordinate does not have is not read
__device__ __forceinline__ double tan_dl(const AdjArgs& A, const TanDir& T, int i) {
  return (T.lvar && A.lbpos[i] >= 0) ? T.lvar[i] : 0.0;
}
__device__ __forceinline__ double tan_du(const AdjArgs& A, const TanDir& T, int i) {
  return (T.uvar && A.ubpos[i] >= 0) ? T.uvar[i] : 0.0;
}
// the directions of column j (the kernels below: column blockIdx.y, as the adjoint's)
__device__ __forceinline__ TanDir tan_col(const TanDir& T, const AdjArgs& A, const BLen& L, int j) {
  return TanDir{bcol(T.c, j, A.nx),   bcol(T.Hv, j, L.nh),  bcol(T.Av, j, L.na),  bcol(T.lcon, j, A.m),
                bcol(T.ucon, j, A.m), bcol(T.lvar, j, A.nx), bcol(T.uvar, j, A.nx)};
}

// v = [p; p~_s; 0]: p_i = (Sigma_l dlvar + Sigma_u duvar)_i / (Sigma_l + Sigma_u)_i on a free variable with a
// bound, else 0 (the scalings cancel in p); the slack k of row r: p~_s,k = con_scale_r (Sigma_l,k dlcon_r +
// Sigma_u,k ducon_r) / (Sigma_l,k + Sigma_u,k).  One thread per variable and per row; a row's thread writes
// its slack's entry.
__global__ __launch_bounds__(NT) void k_tan_shift(AdjArgs A, TanDir T0, BLen L, const int32_t* __restrict__ rowslack,
                                                  double* __restrict__ vb, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ldl_status_end(t1);
  const int col = blockIdx.y;
  const TanDir T = tan_col(T0, A, L, col);
  double* __restrict__ v = vb + col * ((int64_t)A.n + A.m);
  GRID_LOOP(i, A.n + A.m) {
    if (i < A.nx) {
      double o = 0.0;
      if (!A.fixed[i]) {
        const double sl = adj_sig_l(A, (int)i), su = adj_sig_u(A, (int)i), sm = sl + su;
        if (sm > 0.0) o = (sl * tan_dl(A, T, (int)i) + su * tan_du(A, T, (int)i)) / sm;
      }
      v[i] = o;
    } else if (i >= A.n) {
      const int r = (int)(i - A.n), k = rowslack[r];
      v[i] = 0.0;
      if (k >= 0) {
        const double sl = adj_sig_l(A, k), su = adj_sig_u(A, k), sm = sl + su;
        const double dl = (T.lcon && A.lbpos[k] >= 0) ? T.lcon[r] : 0.0;
        const double du = (T.ucon && A.ubpos[k] >= 0) ? T.ucon[r] : 0.0;
        v[k] = sm > 0.0 ? A.cscale[r] * ((sl * dl + su * du) / sm) : 0.0;
      }
    }
  }
}

// The data terms, one thread per destination, each list in ascending input index (build_tangent_lists).
// A free variable i: base_i = -[ os sgn (dc_i + (dH x)_i + (H dxfix)_i) + os (dA^T y)_i ], y the public
// multiplier, os y_r = con_scale_r y~_r; 0 on a fixed variable and a slack.  Row r (public space):
// base_r = (dA x)_r + (A dxfix)_r.  dxfix = dlvar on the fixed variables.  Without lists (gsp == null) the
// sums are empty: no Hvals / Avals direction and no fixed variable with an lvar direction.
__global__ __launch_bounds__(NT) void k_tan_data(AdjArgs A, TanDir T0, BLen L, const int32_t* __restrict__ gsp,
                                                 const int2* __restrict__ ge, const int32_t* __restrict__ csp,
                                                 const int2* __restrict__ ce, const int32_t* __restrict__ asp,
                                                 const int2* __restrict__ ae, const double* __restrict__ Hraw,
                                                 const double* __restrict__ Araw, double* __restrict__ baseb) {
#pragma clang fp contract(off)
  const int col = blockIdx.y;
  const TanDir T = tan_col(T0, A, L, col);
  double* __restrict__ base = baseb + col * ((int64_t)A.n + A.m);
  GRID_LOOP(i, A.n + A.m) {
    double o = 0.0;
    if (i < A.nx) {
      if (!A.fixed[i]) {
        double hs = 0.0, as = 0.0;
        if (gsp) {
          for (int q = gsp[i]; q < gsp[i + 1]; ++q) {
            const int2 e = ge[q];
            if (T.Hv) hs = hs + T.Hv[e.x] * A.x[e.y];
            if (T.lvar && A.fixed[e.y]) hs = hs + Hraw[e.x] * T.lvar[e.y];
          }
          if (T.Av)
            for (int q = csp[i]; q < csp[i + 1]; ++q) {
              const int2 e = ce[q];
              as = as + T.Av[e.x] * (A.cscale[e.y] * A.y[e.y]);
            }
        }
        const double dc = T.c ? T.c[i] : 0.0;
        o = -((A.os * A.sgn) * (dc + hs) + as);
      }
    } else if (i >= A.n) {
      const int r = (int)(i - A.n);
      if (asp)
        for (int q = asp[r]; q < asp[r + 1]; ++q) {
          const int2 e = ae[q];
          if (T.Av) o = o + T.Av[e.x] * A.x[e.y];
          if (T.lvar && A.fixed[e.y]) o = o + Araw[e.x] * T.lvar[e.y];
        }
    }
    base[i] = o;
  }
}

// The shifted right-hand side into bd (and bp, which keeps it for the residual), k_adj_rhs_full's access
// pattern applied to v: base_i - (H~ p)_i on a free variable (v's row part is 0: J~^T adds nothing), 0 on a
// fixed one and on a slack, con_scale_r (db_r - base_r) - (J~ p - p~_s)_r on row r, db = dlcon on an equality
// row.  Every entry is of the directions' magnitude.
template <int G>
__global__ __launch_bounds__(NT) void k_tan_rhs(DV D, AdjArgs A, TanDir T0, BLen L,
                                                const int32_t* __restrict__ rowslack, const double* __restrict__ vb,
                                                const double* __restrict__ baseb, double* __restrict__ bd,
                                                double* __restrict__ bp) {
#pragma clang fp contract(off)
  const int n = D.n, m = D.m;
  const int col = blockIdx.y;
  const int64_t off = col * ((int64_t)n + m);
  const TanDir T = tan_col(T0, A, L, col);
  const double* __restrict__ v = vb + off;
  const double* __restrict__ base = baseb + off;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  GROUP_LOOP(i, n + m, G) {
    double g = 0.0;
    if (i < n) {
      if (i < D.nx && !D.fixed[i]) g = base[i] - gdot<G>(D.H, i, v);
    } else {
      const int r = (int)(i - n);
      const double jq = gdot<G>(D.J, r, v);
      const double db = (T.lcon && rowslack[r] < 0) ? T.lcon[r] : 0.0;
      g = A.cscale[r] * (db - base[i]) - jq;
    }
    if (lead) {
      bd[off + i] = g;
      bp[off + i] = g;
    }
  }
}

// Un-shift and un-scale (A.d is the solution [dx'; ds~'; dy~] of the shifted system; any output may be null):
// dx = dx' + p on a free variable, dlvar on a fixed one (also into dxs, with zeros on the slacks, for
// k_tan_cons); dy = con_scale dy~ / obj_scale; dzl = -Sigma_l dx' + h (dlvar - duvar), dzu = Sigma_u dx' +
// h (dlvar - duvar) with the public Sigma = Sigma~ / obj_scale and h = Sigma_l Sigma_u / (Sigma_l + Sigma_u);
// 0 without that bound and on a fixed variable.
__global__ __launch_bounds__(NT) void k_tan_out(AdjArgs A0, TanDir T0, BLen L, const double* __restrict__ vb,
                                                double* __restrict__ dxsb, double* __restrict__ oxb,
                                                double* __restrict__ oyb, double* __restrict__ ozlb,
                                                double* __restrict__ ozub) {
#pragma clang fp contract(off)
  const int col = blockIdx.y;
  const AdjArgs A = adj_col(A0, col);
  const TanDir T = tan_col(T0, A, L, col);
  const double* __restrict__ v = vb + col * ((int64_t)A.n + A.m);
  double* __restrict__ dxs = dxsb + col * (int64_t)A.n;
  double* __restrict__ ox = bcol(oxb, col, A.nx);
  double* __restrict__ oy = bcol(oyb, col, A.m);
  double* __restrict__ ozl = bcol(ozlb, col, A.nx);
  double* __restrict__ ozu = bcol(ozub, col, A.nx);
  const int ns = A.n - A.nx;
  const int top = A.nx > A.m ? A.nx : A.m;
  GRID_LOOP(i, (top > ns ? top : ns)) {
    if (i < A.nx) {
      double dx, dzl = 0.0, dzu = 0.0;
      if (A.fixed[i]) {
        dx = T.lvar ? T.lvar[i] : 0.0;
      } else {
        const double dxp = A.d[i];
        dx = dxp + v[i];
        const double sl = adj_sig_l(A, (int)i), su = adj_sig_u(A, (int)i), sm = sl + su;
        const double hd = sm > 0.0 ? ((sl * su / sm) / A.os) * (tan_dl(A, T, (int)i) - tan_du(A, T, (int)i)) : 0.0;
        if (A.lbpos[i] >= 0) dzl = hd - (sl / A.os) * dxp;
        if (A.ubpos[i] >= 0) dzu = (su / A.os) * dxp + hd;
      }
      dxs[i] = dx;
      if (ox) ox[i] = dx;
      if (ozl) ozl[i] = dzl;
      if (ozu) ozu[i] = dzu;
    }
    if (i < ns) dxs[A.nx + i] = 0.0;
    if (i < A.m && oy) oy[i] = A.d[A.n + i] * A.cscale[i] / A.os;
  }
}

// dcons_r = (A dx)_r + (dA x)_r: J~'s structural columns times dx / con_scale_r (J~ has no fixed column, and
// dxs is 0 on the slacks), + base_r, which holds the fixed columns' part and dA x
template <int G>
__global__ __launch_bounds__(NT) void k_tan_cons(DV D, AdjArgs A, const double* __restrict__ dxsb,
                                                 const double* __restrict__ baseb, double* __restrict__ oconsb) {
#pragma clang fp contract(off)
  const int col = blockIdx.y;
  const double* __restrict__ dxs = dxsb + col * (int64_t)D.n;
  const double* __restrict__ base = baseb + col * ((int64_t)D.n + D.m);
  double* __restrict__ ocons = oconsb + col * (int64_t)D.m;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  GROUP_LOOP(r, D.m, G) {
    const double s = gdot<G>(D.J, r, dxs);
    if (lead) ocons[r] = s / A.cscale[r] + base[D.n + r];
  }
}

}  // namespace

void MPCSolver::tangent(const madipm_qp_directions& dr, const madipm_qp_point_tangents& o, bool device,
                        hipStream_t caller) {
  const std::string who = device ? "madipm_solver_tangent_device: " : "madipm_solver_tangent: ";
  tangent_cols(who, 1, false, false, dr, o, device, caller);  // one column on the single call's scratch (§13i)
}

void MPCSolver::tangent_info(int64_t* n_tangents, double* last_residual) {
  const int64_t calls = post_ ? post_->tan.n_tangents : 0;
  if (n_tangents) *n_tangents = calls;
  read_residual(last_residual, calls, calls ? post_->tan.scal.p : nullptr, stream_);
}

}  // namespace madipm

// ======================================================================= polish
// madipm_solver_polish / _polish_device: the active set the end point identifies (or the caller's), the active
// coordinates of v = [x; s] at their bounds, and the equality-constrained QP of that face solved in delta form:
// r = -[grad of the Lagrangian on the inactive coordinates; J v - b] at the scratch point w = [v; y], a solve
// with the factor of the K2 pattern whose diagonal is H~_ii + delta_w (+ sigma on an active coordinate; no
// Sigma), the correction masked on the active coordinates, a fixed number of times.  The factor is a
// preconditioner: the residual is the exact masked operator's.  One thread (the residual: one lane group) per
// output, every sum in a fixed order, no atomics but the integer maxima of the two flags.
namespace madipm {
namespace {

struct PolArgs {
  int n, m, nx;
  double os;                                   // obj_scale
  const double *x, *zl, *zu, *y;               // the iterate (scaled space); never written
  const double* cscale;                        // con_scale
  const int32_t *lbpos, *ubpos;
  const uint8_t* fixed;
  const double *lo, *hi;                       // raw bounds of [x; s], public space (lvar / lcon of the slack's row)
  const int32_t *ineq, *rowslack;              // slack -> row; row -> slack coordinate or -1
  int8_t* codes;                               // -1 lower-active, +1 upper-active, 0 inactive, per coordinate of [x; s]
  const int8_t* codes_fact;                    // the codes the factor held was made with
  double *w, *grad;                            // [v; y]; f + J~^T y on [x; s] at w
  int32_t* flags;
};

// con_scale of coordinate i's row (1 on a variable), and its bounds in the scaled space
__device__ __forceinline__ double pol_cs(const PolArgs& P, int i) { return i < P.nx ? 1.0 : P.cscale[P.ineq[i - P.nx]]; }
// a multiplier of coordinate i, scaled space -> public (k_unscale's roundings: z / os, y cs / os)
__device__ __forceinline__ double pol_mult(const PolArgs& P, int i, double z, double cs) {
  return i < P.nx ? z / P.os : z * cs / P.os;
}

// The codes and the projected point.  av == null: the guess, on the values get_solution returns (multiplier
// against gap, both un-scaled); else the supplied set, validated (flags[0]).  flags[1]: the codes differ from
// those of the factor held.  Writes only scratch.  t1 as in k_adj_shift.
__global__ __launch_bounds__(NT) void k_pol_classify(PolArgs P, const int8_t* __restrict__ av,
                                                     const int8_t* __restrict__ ar, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
  const int top = P.n > P.m ? P.n : P.m;
  GRID_LOOP(i, top) {
    if (i < P.n) {
      const bool fx = P.fixed[i], kl = P.lbpos[i] >= 0, ku = P.ubpos[i] >= 0;
      const double cs = pol_cs(P, (int)i);
      const double v = P.x[i];
      const double ls = i < P.nx ? P.lo[i] : cs * P.lo[i], us = i < P.nx ? P.hi[i] : cs * P.hi[i];
      int c = 0;
      if (av) {
        c = i < P.nx ? av[i] : ar[P.ineq[i - P.nx]];
        if (c != 0 && (fx || (c != -1 && c != 1) || (c == -1 && !kl) || (c == 1 && !ku))) {
          atomicMax(&P.flags[0], 1);
          c = 0;
        }
      } else if (!fx) {
        const double zl = kl ? pol_mult(P, (int)i, P.zl[i], cs) : 0.0, zu = ku ? pol_mult(P, (int)i, P.zu[i], cs) : 0.0;
        const bool la = kl && zl > (v - ls) / cs, ua = ku && zu > (us - v) / cs;
        c = (la && ua) ? (zu > zl ? 1 : -1) : (la ? -1 : (ua ? 1 : 0));
      }
      P.w[i] = c < 0 ? ls : (c > 0 ? us : v);
      if (P.codes_fact[i] != c) atomicMax(&P.flags[1], 1);
      P.codes[i] = (int8_t)c;
    }
    if (i < P.m) {
      P.w[P.n + i] = P.y[i];
      if (ar && P.rowslack[i] < 0 && ar[i] != 0) atomicMax(&P.flags[0], 1);
    }
  }
}

// The K2 diagonal of the polish factor: H~_ii + delta_w, + sigma on an active coordinate; delta_c on a row.
// Only Kx's diagonal is written.  rs as in k_diag.
__global__ __launch_bounds__(NT) void k_pol_diag(DV D, const int8_t* __restrict__ codes, double dw, double dc,
                                                 double sigma, LDLStatus* rs) {
#pragma clang fp contract(off)
  if (rs && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_start(rs);
  GRID_LOOP(i, D.n + D.m) {
    if (i < D.n) {
      const double h = D.Hdiag[i] + dw;
      D.Kx[D.diag_pos[i]] = codes[i] ? h + sigma : h;
    } else {
      D.Kx[D.diag_pos[i]] = dc;
    }
  }
}

// The exact masked residual at w: on a coordinate of [x; s], t = (H~ v + c~ + gfix) + J~^T y (k_eval's f and
// jacl), r = -t on an inactive free coordinate and 0 on an active or fixed one; on a row, r = -((J~ v - rhs) +
// cfix).  r (may be null) becomes the right-hand side of the next solve; grad (may be null) keeps t.
template <int G>
__global__ __launch_bounds__(NT) void k_pol_resid(DV D, PolArgs P, double* __restrict__ r, double* __restrict__ rowres,
                                                  double* __restrict__ grad, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
  const int n = D.n, m = D.m;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  const double* __restrict__ w = P.w;
  GROUP_LOOP(i, n + m, G) {
    double ri;
    if (i < n) {
      double hv, jy;
      gdot2<G>(D.H, i, w, D.JT, i, w + n, hv, jy);
      const double t = (hv + (D.cs[i] + D.gfix[i])) + jy;
      ri = (P.codes[i] != 0 || D.fixed[i]) ? 0.0 : -t;
      if (lead && grad) grad[i] = t;
    } else {
      const int64_t j = i - n;
      const double jv = gdot<G>(D.J, j, w);
      ri = -((jv - D.rhs[j]) + D.cfix[j]);
    }
    if (lead) {
      if (r) r[i] = ri;
      rowres[i] = fabs(ri);
    }
  }
}

// w += d, with the correction of an active or fixed coordinate dropped
__global__ __launch_bounds__(NT) void k_pol_acc(PolArgs P, const double* __restrict__ d) {
  GRID_LOOP(i, P.n + P.m) {
    if (i < P.n && (P.codes[i] != 0 || P.fixed[i])) continue;
    P.w[i] = P.w[i] + d[i];
  }
}

// The checks as block partials (value-major, pidx): the smallest active multiplier, the largest |active
// multiplier|, the smallest gap / max(1, |bound|) and the smallest gap over the inactive bounds, all in the
// public space
__global__ __launch_bounds__(NT) void k_pol_meas(PolArgs P, double* __restrict__ part) {
#pragma clang fp contract(off)
  double mn = INF, ma = 0.0, gp = INF, gr = INF;
  GRID_LOOP(i, P.n) {
    if (P.fixed[i]) continue;
    const int c = P.codes[i];
    const double cs = pol_cs(P, (int)i);
    if (c != 0) {
      const double t = pol_mult(P, (int)i, P.grad[i], cs);
      const double z = c < 0 ? t : -t;
      mn = fmin(mn, z);
      ma = nmax(ma, fabs(z));
    }
    const double v = P.w[i];
    if (P.lbpos[i] >= 0 && c != -1) {
      const double b = P.lo[i], bs = i < P.nx ? b : cs * b;
      const double g = (v - bs) / cs;
      gr = fmin(gr, g);
      gp = fmin(gp, g / fmax(1.0, fabs(b)));
    }
    if (P.ubpos[i] >= 0 && c != 1) {
      const double b = P.hi[i], bs = i < P.nx ? b : cs * b;
      const double g = (bs - v) / cs;
      gr = fmin(gr, g);
      gp = fmin(gp, g / fmax(1.0, fabs(b)));
    }
  }
  double v[4] = {mn, ma, gp, gr};
  const int ops[4] = {OP_MIN, OP_MAX, OP_MIN, OP_MIN};
  block_partials<4>(v, ops, part);
}

// The verdict: one block, each thread a strided slice, then an LDS tree (k_adj_resmax's shape; maxima and
// minima do not depend on the order, the count is an integer sum).  failed: all three factorisations failed.
__global__ __launch_bounds__(NT) void k_pol_verdict(const double* __restrict__ rowres, int64_t N,
                                                    const double* __restrict__ part, int nb,
                                                    const int8_t* __restrict__ codes, int n, double tol_resid,
                                                    double tol_sign, double tol_feas, int failed,
                                                    PolMeasures* __restrict__ out) {
  __shared__ double sr[NT], smn[NT], sma[NT], sgp[NT], sgr[NT];
  __shared__ int sc[NT];
  const int t = threadIdx.x;
  double r = 0.0, mn = INF, ma = 0.0, gp = INF, gr = INF;
  int cnt = 0;
  for (int64_t i = t; i < N; i += NT) r = nmax(r, rowres[i]);
  for (int b = t; b < nb; b += NT) {
    mn = fmin(mn, part[pidx(b, 0)]);
    ma = nmax(ma, part[pidx(b, 1)]);
    gp = fmin(gp, part[pidx(b, 2)]);
    gr = fmin(gr, part[pidx(b, 3)]);
  }
  for (int i = t; i < n; i += NT) cnt += codes[i] != 0;
  sr[t] = r, smn[t] = mn, sma[t] = ma, sgp[t] = gp, sgr[t] = gr, sc[t] = cnt;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (t < o) {
      sr[t] = nmax(sr[t], sr[t + o]);
      smn[t] = fmin(smn[t], smn[t + o]);
      sma[t] = nmax(sma[t], sma[t + o]);
      sgp[t] = fmin(sgp[t], sgp[t + o]);
      sgr[t] = fmin(sgr[t], sgr[t + o]);
      sc[t] += sc[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    int v = MADIPM_POLISHED;
    if (smn[0] < -tol_sign * (sma[0] > 1.0 ? sma[0] : 1.0) || sgp[0] < -tol_feas) v = MADIPM_POLISH_WRONG_SET;
    if (!(sr[0] <= tol_resid)) v = MADIPM_POLISH_NO_CONVERGENCE;  // a NaN lands here
    if (failed) v = MADIPM_POLISH_FACTORIZATION_FAILED;
    out->verdict = v;
    out->n_active = sc[0];
    out->residual = sr[0];
    out->min_multiplier = smn[0];
    out->min_gap = sgr[0];
    out->max_multiplier = sma[0];
  }
}

// The polished point, un-scaled (any output may be null): x = v; y = y~ cs / os; zl = t / os on a lower-active
// variable, zu = -t / os on an upper-active one, 0 elsewhere; cons = (A x) / cs from k_cons' row values, the
// bound itself on an active row
__global__ __launch_bounds__(NT) void k_pol_out(PolArgs P, const double* __restrict__ ax, double* __restrict__ ox,
                                                double* __restrict__ oy, double* __restrict__ ozl,
                                                double* __restrict__ ozu, double* __restrict__ ocons) {
#pragma clang fp contract(off)
  GRID_LOOP(i, (P.nx > P.m ? P.nx : P.m)) {
    if (i < P.nx) {
      const int c = P.codes[i];
      const double t = c != 0 ? P.grad[i] / P.os : 0.0;
      if (ox) ox[i] = P.w[i];
      if (ozl) ozl[i] = c < 0 ? t : 0.0;
      if (ozu) ozu[i] = c > 0 ? -t : 0.0;
    }
    if (i < P.m) {
      const double cs = P.cscale[i];
      if (oy) oy[i] = P.w[P.n + i] * cs / P.os;
      if (ocons) {
        const int k = P.rowslack[i], c = k >= 0 ? P.codes[k] : 0;
        ocons[i] = c < 0 ? P.lo[k] : (c > 0 ? P.hi[k] : ax[i] / cs);
      }
    }
  }
}

// The codes as the caller sees them: one per variable, one per row (0 on an equality row)
__global__ __launch_bounds__(NT) void k_pol_codes(PolArgs P, int8_t* __restrict__ ovar, int8_t* __restrict__ orow) {
  GRID_LOOP(i, (P.nx > P.m ? P.nx : P.m)) {
    if (i < P.nx && ovar) ovar[i] = P.codes[i];
    if (i < P.m && orow) {
      const int k = P.rowslack[i];
      orow[i] = k >= 0 ? P.codes[k] : (int8_t)0;
    }
  }
}

// ---- the active-set solve's own kernels; everything else it launches is the polish's
// The raw bounds of [x; s] from the device route's staging: lvar / uvar, lcon / ucon of the slack's row
__global__ __launch_bounds__(NT) void k_as_bounds(int nx, int n, const double* __restrict__ lvar,
                                                  const double* __restrict__ uvar, const double* __restrict__ lcon,
                                                  const double* __restrict__ ucon, const int32_t* __restrict__ ineq,
                                                  double* __restrict__ lo, double* __restrict__ hi) {
  GRID_LOOP(i, n) {
    if (i < nx) {
      lo[i] = lvar[i], hi[i] = uvar[i];
    } else {
      const int r = ineq[i - nx];
      lo[i] = lcon[r], hi[i] = ucon[r];
    }
  }
}

// The start of a round.  The codes: the supplied set, validated as k_pol_classify validates it (flags[0]); or
// `from` (the kept set); or, with neither, those k_as_next left in P.codes.  Then v = the raw bound on an active
// coordinate and 0 on an inactive one, a fixed variable at its value, y = 0: the iterate is not read, so the
// round's result depends on the data, the set and the options only.  flags[1] and t1 as in k_pol_classify;
// codes0 (may be null) keeps the set the call started from.
__global__ __launch_bounds__(NT) void k_as_start(PolArgs P, const int8_t* __restrict__ av,
                                                 const int8_t* __restrict__ ar, const int8_t* __restrict__ from,
                                                 int8_t* __restrict__ codes0, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
  const int top = P.n > P.m ? P.n : P.m;
  GRID_LOOP(i, top) {
    if (i < P.n) {
      const bool fx = P.fixed[i], kl = P.lbpos[i] >= 0, ku = P.ubpos[i] >= 0;
      int c;
      if (av) {
        c = i < P.nx ? av[i] : ar[P.ineq[i - P.nx]];
        if (c != 0 && (fx || (c != -1 && c != 1) || (c == -1 && !kl) || (c == 1 && !ku))) {
          atomicMax(&P.flags[0], 1);
          c = 0;
        }
      } else {
        c = from ? from[i] : P.codes[i];
      }
      double v = 0.0;
      if (fx) {
        v = P.lo[i];
      } else if (c != 0) {
        const double b = c < 0 ? P.lo[i] : P.hi[i];
        v = i < P.nx ? b : pol_cs(P, (int)i) * b;
      }
      P.w[i] = v;
      if (P.codes_fact[i] != c) atomicMax(&P.flags[1], 1);
      P.codes[i] = (int8_t)c;
      if (codes0) codes0[i] = (int8_t)c;
    }
    if (i < P.m) {
      P.w[P.n + i] = 0.0;
      if (ar && P.rowslack[i] < 0 && ar[i] != 0) atomicMax(&P.flags[0], 1);
    }
  }
}

// The next set after a round that ended WRONG_SET, from exactly the violations k_pol_verdict found (k_pol_meas'
// expressions, the verdict's thresholds, M = max(1, max |active multiplier|) of this round): an active
// coordinate whose multiplier is < -tol_sign M becomes inactive; an inactive one whose gap to a bound it has is
// < -tol_feas max(1, |bound|) becomes active there, the lower bound when both are violated.  One thread per
// coordinate, so a coordinate dropped here is not added again.
__global__ __launch_bounds__(NT) void k_as_next(PolArgs P, const PolMeasures* __restrict__ meas, double tol_sign,
                                                double tol_feas) {
#pragma clang fp contract(off)
  const double ma = meas->max_multiplier;
  const double M = ma > 1.0 ? ma : 1.0;
  GRID_LOOP(i, P.n) {
    if (P.fixed[i]) continue;
    const int c = P.codes[i];
    const double cs = pol_cs(P, (int)i);
    if (c != 0) {
      const double t = pol_mult(P, (int)i, P.grad[i], cs);
      const double z = c < 0 ? t : -t;
      if (z < -tol_sign * M) P.codes[i] = 0;
      continue;
    }
    const double v = P.w[i];
    int nc = 0;
    if (P.ubpos[i] >= 0) {
      const double b = P.hi[i], bs = i < P.nx ? b : cs * b;
      if ((bs - v) / cs / fmax(1.0, fabs(b)) < -tol_feas) nc = 1;
    }
    if (P.lbpos[i] >= 0) {
      const double b = P.lo[i], bs = i < P.nx ? b : cs * b;
      if ((v - bs) / cs / fmax(1.0, fabs(b)) < -tol_feas) nc = -1;
    }
    if (nc) P.codes[i] = (int8_t)nc;
  }
}

// The codes that differ between two sets: an integer sum per block (an LDS tree), one integer atomic per block
__global__ __launch_bounds__(NT) void k_as_changed(int n, const int8_t* __restrict__ a, const int8_t* __restrict__ b,
                                                   int32_t* __restrict__ count) {
  __shared__ int sc[NT];
  int cnt = 0;
  GRID_LOOP(i, n) cnt += a[i] != b[i];
  sc[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sc[threadIdx.x] += sc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sc[0]) atomicAdd(count, sc[0]);
}

}  // namespace

// The polish's and the active-set solve's scratch, by the first call of either, and the raw bounds of [x; s] as
// the last update left them.  device_bounds: the device route's staging holds them (k_as_bounds, no host copy).
void MPCSolver::polish_buffers(bool device_bounds) {
  QPHost& P = *H_;
  hipStream_t s = stream_;
  PostSolve& ps = post_state();
  Polish& p = ps.pol;
  ps.rowslack(P, s);
  const int ns = n_ - nx_;
  if (!p.w.p) {
    p.w.alloc(std::max(n_ + m_, 1));
    p.grad.alloc(std::max(n_, 1));
    p.lo.alloc(std::max(n_, 1));
    p.hi.alloc(std::max(n_, 1));
    p.part.alloc((size_t)4 * MAXB);
    p.ax.alloc(std::max(m_, 1));
    p.codes.alloc(std::max(n_, 1));
    p.codes_fact.alloc(std::max(n_, 1));
    p.codes_fact.zero(s);
    p.codes_kept.alloc(std::max(n_, 1));
    p.codes0.alloc(std::max(n_, 1));
    p.changed.alloc(1);
    p.ineq.alloc(std::max(ns, 1));
    p.ineq.upload(P.ind_ineq.data(), P.ind_ineq.size(), s);
    p.flags.alloc(2);
    p.meas.alloc(1);
  }
  if (p.bounds_updates == n_updates_) return;
  const double* raw[4];  // lvar, uvar, lcon, ucon of the device route's staging
  if (device_bounds && device_raw_bounds(raw)) {
    if (n_)
      k_as_bounds<<<blocks(n_), NT, 0, s>>>(nx_, n_, raw[0], raw[1], raw[2], raw[3], p.ineq.p, p.lo.p, p.hi.p);
    MADIPM_HIP(hipGetLastError());
  } else {
    refresh_host_mirrors();
    std::vector<double> lo(std::max(n_, 1)), hi(std::max(n_, 1));
    for (int i = 0; i < nx_; ++i) lo[i] = P.lvar[i], hi[i] = P.uvar[i];
    for (int k = 0; k < ns; ++k) lo[nx_ + k] = P.lcon[P.ind_ineq[k]], hi[nx_ + k] = P.ucon[P.ind_ineq[k]];
    p.lo.upload(lo, s);
    p.hi.upload(hi, s);
    MADIPM_HIP(hipStreamSynchronize(s));  // lo / hi are this scope's
  }
  p.bounds_updates = n_updates_;
}

// The LDL^T holds the polish factor of the current data: made at this solve and update count, and nothing has
// factorised since.  (Its codes and sigma are compared by the caller.)
bool MPCSolver::polish_factor_held() const {
  const Polish& p = post_->pol;
  return p.fact_solve == n_solves_ && p.fact_updates == n_updates_ && p.fact_calls == n_factor_calls_;
}

void MPCSolver::polish_factor_tag(double sigma) {
  Polish& p = post_->pol;
  if (n_) MADIPM_HIP(hipMemcpyAsync(p.codes_fact.p, p.codes.p, (size_t)n_, hipMemcpyDeviceToDevice, stream_));
  p.fact_solve = n_solves_;
  p.fact_updates = n_updates_;
  p.fact_calls = n_factor_calls_;
  p.fact_sigma = sigma;
}

// The current polished point is an active-set solve's: it ended POLISHED, and no update, initialize, solve,
// polish or active-set solve ran since
bool MPCSolver::active_set_point() const {
  if (!post_) return false;
  const Polish& p = post_->pol;
  return p.as_point && p.as_updates == n_updates_ && p.as_solves == n_solves_ && p.as_inits == n_inits_;
}

void MPCSolver::polish(const madipm_polish_opts& o, const int8_t* av, const int8_t* ar, const madipm_polish_out& po,
                       madipm_polish_info* info, bool device, hipStream_t caller) {
  const std::string who = device ? "madipm_solver_polish_device: " : "madipm_solver_polish: ";
  // ---- refusals, before anything is allocated or enqueued
  sens_refuse(who);
  MADIPM_REQUIRE((av == nullptr) == (ar == nullptr),
                 who + "exactly one of active_var and active_row is given (pass both, or neither for the guess)");
  double* const user[5] = {po.x, po.y, po.zl, po.zu, po.cons};
  MADIPM_REQUIRE(po.x || po.y || po.zl || po.zu || po.cons || po.active_var || po.active_row,
                 who + "all seven outputs are NULL");
  auto tol_ok = [](double t) { return t >= 0.0 && std::isfinite(t); };
  MADIPM_REQUIRE(o.sigma > 0.0 && std::isfinite(o.sigma), who + "sigma must be positive and finite");
  MADIPM_REQUIRE(tol_ok(o.tol_resid) && tol_ok(o.tol_sign) && tol_ok(o.tol_feas),
                 who + "tol_resid, tol_sign and tol_feas must be finite and not negative");
  MADIPM_REQUIRE(o.refine_steps >= 0 && o.refine_steps <= 8,
                 who + "refine_steps must be in 0..8, got " + std::to_string(o.refine_steps));
  hipStream_t s = stream_;
  // ---- allocations, by the first call
  polish_buffers(false);
  PostSolve& ps = *post_;
  Adjoint& a = ps.adj;
  Polish& p = ps.pol;
  const double* cscale = device_con_scale();
  const int64_t olen[5] = {nx_, m_, nx_, nx_, m_};
  double* out[5];
  p.out.bind(user, olen, device, out);
  const int8_t* const set[2] = {av, ar};
  int8_t* const uset[2] = {po.active_var, po.active_row};
  const int64_t slen[2] = {nx_, m_};
  const int8_t* dset[2];
  int8_t* oset[2];
  p.set_in.bind(set, slen, device, dset);
  p.set_out.bind(uset, slen, device, oset);
  if (device)  // the set is read, and the outputs written, after the work already enqueued on the caller's stream
    ps.sync.begin(caller, s);
  else
    p.set_in.upload(set, slen, s);
  // ---- the codes and the projected point
  const DV D = view();
  const PolArgs A{n_, m_, nx_, obj_scale_, x_.p, zl_.p, zu_.p, y_.p, cscale, lbpos_.p, ubpos_.p, fixed_.p,
                  p.lo.p, p.hi.p, p.ineq.p, a.rowslack.p, p.codes.p, p.codes_fact.p, p.w.p, p.grad.p, p.flags.p};
  const int nb = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_), nbn = blocks(std::max(n_, 1));
  const int64_t N = (int64_t)n_ + m_;
  p.point_solve = -1;  // w, codes and grad are overwritten from here on
  p.as_point = false;
  p.flags.zero(s);
  k_pol_classify<<<blocks(std::max(std::max(n_, m_), 1)), NT, 0, s>>>(A, dset[0], dset[1], take_fact_end());
  MADIPM_HIP(hipGetLastError());
  int32_t hflags[2] = {0, 0};
  MADIPM_HIP(hipMemcpyAsync(hflags, p.flags.p, sizeof(hflags), hipMemcpyDeviceToHost, s));
  MADIPM_HIP(hipStreamSynchronize(s));
  MADIPM_REQUIRE(!hflags[0], who + "the supplied set has a code other than -1, 0, +1, or a code on a bound that does "
                                   "not exist, on a fixed variable or on an equality row");
  // ---- the factor: once per point, set and sigma
  bool ok = true;
  if (!polish_factor_held() || p.fact_sigma != o.sigma || hflags[1]) {
    p.fact_solve = -1;
    a.fact_solve = -1;  // the adjoint's factor and KKT diagonal are overwritten
    ok = factor_trials([&](double dw, double dc) {
      k_pol_diag<<<nb, NT, 0, s>>>(D, p.codes.p, dw, dc, o.sigma, fact_reset());
      timed_factorize();
    });
    if (ok) {
      polish_factor_tag(o.sigma);
      ++p.last.n_polish_factorizations;
    }
  }
  // ---- 1 + refine_steps solves in delta form, the final residual, the verdict
  if (ok)
    for (int it = 0; it <= o.refine_steps; ++it) {
      SPMV_LAUNCH(k_pol_resid, nbs, s, D, A, d_.p, a.rowres.p, (double*)nullptr, take_fact_end());
      kkt_solve();
      k_pol_acc<<<nb, NT, 0, s>>>(A, d_.p);
    }
  SPMV_LAUNCH(k_pol_resid, nbs, s, D, A, (double*)nullptr, a.rowres.p, p.grad.p, take_fact_end());
  k_pol_meas<<<nbn, NT, 0, s>>>(A, p.part.p);
  k_pol_verdict<<<1, NT, 0, s>>>(a.rowres.p, N, p.part.p, nbn, p.codes.p, n_, o.tol_resid, o.tol_sign, o.tol_feas,
                                 ok ? 0 : 1, p.meas.p);
  MADIPM_HIP(hipGetLastError());
  PolMeasures hm{};
  MADIPM_HIP(hipMemcpyAsync(&hm, p.meas.p, sizeof(hm), hipMemcpyDeviceToHost, s));
  MADIPM_HIP(hipStreamSynchronize(s));
  // ---- outputs: the polished point, or get_solution's bits
  const bool any5 = out[0] || out[1] || out[2] || out[3] || out[4];
  if (any5 && std::max(nx_, m_)) {
    if (hm.verdict == MADIPM_POLISHED) {
      if (out[4]) cons_rows(p.w.p, p.ax.p);
      k_pol_out<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, p.ax.p, out[0], out[1], out[2], out[3], out[4]);
    } else {
      unscale_point(cscale, p.ax.p, out[0], out[1], out[2], out[3], out[4]);
    }
  }
  if ((oset[0] || oset[1]) && std::max(nx_, m_))
    k_pol_codes<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, oset[0], oset[1]);
  MADIPM_HIP(hipGetLastError());
  if (device) {  // work enqueued on the caller's stream from now on sees the outputs
    ps.sync.end(s, caller);
  } else {
    p.out.download(user, olen, s, false);
    p.set_out.download(uset, slen, s);
  }
  p.point_solve = n_solves_;
  p.refine_steps = o.refine_steps;
  if (hm.verdict == MADIPM_POLISHED) {  // the kept set of the active-set solve (§13h)
    if (n_) MADIPM_HIP(hipMemcpyAsync(p.codes_kept.p, p.codes.p, (size_t)n_, hipMemcpyDeviceToDevice, s));
    p.kept = true;
  }
  ++p.last.n_polishes;
  p.last.verdict = hm.verdict;
  p.last.n_active = hm.n_active;
  p.last.residual = hm.residual;
  p.last.min_multiplier = hm.min_multiplier;
  p.last.min_gap = hm.min_gap;
  if (info) *info = p.last;
}

void MPCSolver::polish_info(madipm_polish_info* info) const {
  if (!info) return;
  *info = post_ ? post_->pol.last : madipm_polish_info{-1, 0, 0.0, 0.0, 0.0, 0, 0};
}

// madipm_solver_active_set_solve / _device: up to max_rounds rounds of start (k_as_start), the
// polish's factor, 1 + refine_steps delta-form solves, final residual, measures and verdict; WRONG_SET before
// the last round repairs the set (k_as_next) and goes on, every other verdict ends the call.  It needs no
// solve: everything it reads is what the constructor or the last update left on the device.
void MPCSolver::active_set_solve(const madipm_active_set_opts& ao, const int8_t* av, const int8_t* ar,
                                 const madipm_polish_out& po, madipm_active_set_info* info, bool device,
                                 hipStream_t caller) {
  const std::string who = device ? "madipm_solver_active_set_solve_device: " : "madipm_solver_active_set_solve: ";
  const madipm_polish_opts& o = ao.polish;
  // ---- refusals, before anything is allocated or enqueued
  MADIPM_REQUIRE(kkt_ == KKT_K2, who + "only kkt_system = SparseKKTSystem (K2) is supported; the K2.5 and "
                                       "normal-equations formulations are left to a later release");
  MADIPM_REQUIRE(!comm_, who + "a solver created with a communicator (madipm_solver_create_dist) is not supported");
  MADIPM_REQUIRE((av == nullptr) == (ar == nullptr),
                 who + "exactly one of active_var and active_row is given (pass both, or neither for the kept set)");
  double* const user[5] = {po.x, po.y, po.zl, po.zu, po.cons};
  MADIPM_REQUIRE(po.x || po.y || po.zl || po.zu || po.cons || po.active_var || po.active_row,
                 who + "all seven outputs are NULL");
  auto tol_ok = [](double t) { return t >= 0.0 && std::isfinite(t); };
  MADIPM_REQUIRE(o.sigma > 0.0 && std::isfinite(o.sigma), who + "sigma must be positive and finite");
  MADIPM_REQUIRE(tol_ok(o.tol_resid) && tol_ok(o.tol_sign) && tol_ok(o.tol_feas),
                 who + "tol_resid, tol_sign and tol_feas must be finite and not negative");
  MADIPM_REQUIRE(o.refine_steps >= 0 && o.refine_steps <= 8,
                 who + "refine_steps must be in 0..8, got " + std::to_string(o.refine_steps));
  MADIPM_REQUIRE(ao.max_rounds >= 1 && ao.max_rounds <= 16,
                 who + "max_rounds must be in 1..16, got " + std::to_string(ao.max_rounds));
  MADIPM_REQUIRE(av || (post_ && post_->pol.kept),
                 who + "no set is given and none is kept: no polish or active-set solve on this solver has ended "
                       "POLISHED yet (pass active_var and active_row)");
  hipStream_t s = stream_;
  // ---- allocations, by the first call; the raw bounds of this data
  polish_buffers(true);
  PostSolve& ps = *post_;
  Adjoint& a = ps.adj;
  Polish& p = ps.pol;
  const double* cscale = device_con_scale();
  const int64_t olen[5] = {nx_, m_, nx_, nx_, m_};
  double* out[5];
  p.out.bind(user, olen, device, out);
  const int8_t* const set[2] = {av, ar};
  int8_t* const uset[2] = {po.active_var, po.active_row};
  const int64_t slen[2] = {nx_, m_};
  const int8_t* dset[2];
  int8_t* oset[2];
  p.set_in.bind(set, slen, device, dset);
  p.set_out.bind(uset, slen, device, oset);
  if (device)  // the set is read, and the outputs written, after the work already enqueued on the caller's stream
    ps.sync.begin(caller, s);
  else
    p.set_in.upload(set, slen, s);
  const DV D = view();
  // the iterate's place stays empty: no kernel launched here may read it
  const PolArgs A{n_, m_, nx_, obj_scale_, nullptr, nullptr, nullptr, nullptr, cscale, lbpos_.p, ubpos_.p, fixed_.p,
                  p.lo.p, p.hi.p, p.ineq.p, a.rowslack.p, p.codes.p, p.codes_fact.p, p.w.p, p.grad.p, p.flags.p};
  const int nb = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_), nbn = blocks(std::max(n_, 1));
  const int nbt = blocks(std::max(std::max(n_, m_), 1));
  const int64_t N = (int64_t)n_ + m_;
  p.point_solve = -1;  // w, codes and grad are overwritten from here on: no current polished point
  p.as_point = false;
  PolMeasures hm{};
  int rounds = 0;
  for (int k = 1; k <= ao.max_rounds; ++k) {
    rounds = k;
    // ---- the start; the first round's set is validated and kept for n_changed
    p.flags.zero(s);
    if (k == 1)
      k_as_start<<<nbt, NT, 0, s>>>(A, dset[0], dset[1], dset[0] ? nullptr : (const int8_t*)p.codes_kept.p,
                                    p.codes0.p, take_fact_end());
    else
      k_as_start<<<nbt, NT, 0, s>>>(A, nullptr, nullptr, nullptr, nullptr, take_fact_end());
    MADIPM_HIP(hipGetLastError());
    bool held = false;
    if (k == 1) {
      int32_t hflags[2] = {0, 0};
      MADIPM_HIP(hipMemcpyAsync(hflags, p.flags.p, sizeof(hflags), hipMemcpyDeviceToHost, s));
      MADIPM_HIP(hipStreamSynchronize(s));
      if (hflags[0] && device) ps.sync.end(s, caller);
      MADIPM_REQUIRE(!hflags[0], who + "the supplied set has a code other than -1, 0, +1, or a code on a bound that "
                                       "does not exist, on a fixed variable or on an equality row");
      held = polish_factor_held() && p.fact_sigma == o.sigma && !hflags[1];
    }
    // ---- the factor: the one held when data, set and sigma are its own; a repaired set is a new one
    bool ok = true;
    if (!held) {
      p.fact_solve = -1;
      a.fact_solve = -1;  // the adjoint's factor and KKT diagonal are overwritten
      ok = factor_trials([&](double dw, double dc) {
        k_pol_diag<<<nb, NT, 0, s>>>(D, p.codes.p, dw, dc, o.sigma, fact_reset());
        timed_factorize();
      });
      if (ok) {
        polish_factor_tag(o.sigma);
        ++p.as_last.n_factorizations;
      }
    }
    // ---- 1 + refine_steps solves in delta form, the final residual, the verdict
    if (ok)
      for (int it = 0; it <= o.refine_steps; ++it) {
        SPMV_LAUNCH(k_pol_resid, nbs, s, D, A, d_.p, a.rowres.p, (double*)nullptr, take_fact_end());
        kkt_solve();
        k_pol_acc<<<nb, NT, 0, s>>>(A, d_.p);
      }
    SPMV_LAUNCH(k_pol_resid, nbs, s, D, A, (double*)nullptr, a.rowres.p, p.grad.p, take_fact_end());
    k_pol_meas<<<nbn, NT, 0, s>>>(A, p.part.p);
    k_pol_verdict<<<1, NT, 0, s>>>(a.rowres.p, N, p.part.p, nbn, p.codes.p, n_, o.tol_resid, o.tol_sign, o.tol_feas,
                                   ok ? 0 : 1, p.meas.p);
    MADIPM_HIP(hipGetLastError());
    MADIPM_HIP(hipMemcpyAsync(&hm, p.meas.p, sizeof(hm), hipMemcpyDeviceToHost, s));
    MADIPM_HIP(hipStreamSynchronize(s));
    if (hm.verdict != MADIPM_POLISH_WRONG_SET || k == ao.max_rounds) break;
    // ---- the next set, from this round's violations
    k_as_next<<<nbn, NT, 0, s>>>(A, p.meas.p, o.tol_sign, o.tol_feas);
  }
  // ---- the codes of the last set that differ from the starting set
  int32_t changed = 0;
  if (rounds > 1) {
    p.changed.zero(s);
    k_as_changed<<<nbn, NT, 0, s>>>(n_, p.codes.p, p.codes0.p, p.changed.p);
    MADIPM_HIP(hipMemcpyAsync(&changed, p.changed.p, sizeof(changed), hipMemcpyDeviceToHost, s));
    MADIPM_HIP(hipStreamSynchronize(s));
  }
  // ---- outputs: the polished point, or nothing but the last set tried
  const bool polished = hm.verdict == MADIPM_POLISHED;
  const bool any5 = out[0] || out[1] || out[2] || out[3] || out[4];
  if (polished && any5 && std::max(nx_, m_)) {
    if (out[4]) cons_rows(p.w.p, p.ax.p);
    k_pol_out<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, p.ax.p, out[0], out[1], out[2], out[3], out[4]);
  }
  if ((oset[0] || oset[1]) && std::max(nx_, m_))
    k_pol_codes<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, oset[0], oset[1]);
  if (polished) {  // the kept set of the next call
    if (n_) MADIPM_HIP(hipMemcpyAsync(p.codes_kept.p, p.codes.p, (size_t)n_, hipMemcpyDeviceToDevice, s));
    p.kept = true;
  }
  MADIPM_HIP(hipGetLastError());
  if (device) {  // work enqueued on the caller's stream from now on sees the outputs
    ps.sync.end(s, caller);
  } else {
    if (polished) p.out.download(user, olen, s, false);
    p.set_out.download(uset, slen, s);
  }
  if (polished) {  // the current polished point: tangent_polished / adjoint_polished differentiate it
    p.as_point = true;
    p.as_updates = n_updates_;
    p.as_solves = n_solves_;
    p.as_inits = n_inits_;
    p.refine_steps = o.refine_steps;
  }
  madipm_active_set_info& L = p.as_last;
  ++L.n_calls;
  L.verdict = hm.verdict;
  L.rounds = rounds;
  L.n_active = hm.n_active;
  L.n_changed = changed;
  L.residual = hm.residual;
  L.min_multiplier = hm.min_multiplier;
  L.min_gap = hm.min_gap;
  if (info) *info = L;
}

void MPCSolver::active_set_info(madipm_active_set_info* info) const {
  if (!info) return;
  *info = post_ ? post_->pol.as_last : madipm_active_set_info{-1, 0, 0, 0, 0.0, 0.0, 0.0, 0, 0};
}

}  // namespace madipm

// ======================================================================= sensitivities at the polished point
// madipm_solver_tangent_polished / _adjoint_polished (and _device): the derivatives of the face's
// equality-constrained QP at the point the last polish() left in its scratch.  With K0 the K2 operator without
// Sigma and without regularisation (H~, J~^T on a primal row, J~ on a dual row), A the active coordinates of
// [x; s] and N the others, both calls solve one masked system
//     (K0 u)_i = rhs_i on N and on the rows,   u_A given,
// in delta form, exactly as the polish solves its own: r = rhs - K0 u with the rows of A and of the fixed
// variables written 0, a solve with the polish's factor (a preconditioner), the correction masked on A,
// 1 + refine_steps times; the last residual keeps K0 u - rhs on A.
//   tangent: u_A = the direction of the active bound (x cs on a slack), rhs = the data terms (k_tan_data at the
//     polished point); dw = u, and K0 u - rhs on A is the tangent of t = grad of the Lagrangian, so of zl / zu.
//   adjoint: u_A = -taubar~ (taubar = gzl on a lower-active variable, -gzu on an upper-active one), rhs = the
//     cotangents' image ghat~ on [x; s; y]; then u = a~ - taubar~ is -e of the derivation, the place §13c's a~
//     has in the gradient kernels, and rhs - K0 u on A is beta, the gradient of the active bound.
// No product with Sigma occurs.  One thread (the residual, dcons: one lane group) per output, fixed summation
// orders, no atomics: the same bits run to run.
namespace madipm {
namespace {

// u and rhs of the tangent; base: k_tan_data's terms at the polished point (0 on fixed variables and slacks)
__global__ __launch_bounds__(NT) void k_pst_rhs(AdjArgs A, TanDir T, const int8_t* __restrict__ codes,
                                                const int32_t* __restrict__ ineq, const int32_t* __restrict__ rowslack,
                                                const double* __restrict__ base, double* __restrict__ u,
                                                double* __restrict__ rhs, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
  GRID_LOOP(i, A.n + A.m) {
    double ui = 0.0, ri;
    if (i < A.n) {
      const int c = codes[i];
      if (c != 0) {
        if (i < A.nx) {
          const double* b = c < 0 ? T.lvar : T.uvar;
          ui = b ? b[i] : 0.0;
        } else {
          const int r = ineq[i - A.nx];
          const double* b = c < 0 ? T.lcon : T.ucon;
          ui = b ? A.cscale[r] * b[r] : 0.0;
        }
      }
      ri = base[i];
    } else {
      const int r = (int)(i - A.n);
      const double db = (T.lcon && rowslack[r] < 0) ? T.lcon[r] : 0.0;
      ri = A.cscale[r] * (db - base[i]);
    }
    u[i] = ui;
    rhs[i] = ri;
  }
}

// u and rhs of the adjoint (any cotangent may be null: 0): gx on a free variable, gcons_r / cs_r on the slack
// of row r (cons_r = s_r on the face), cs_r gy_r / os on row r; -taubar / os on an active variable
__global__ __launch_bounds__(NT) void k_psa_rhs(AdjArgs A, const double* __restrict__ gx, const double* __restrict__ gy,
                                                const double* __restrict__ gzl, const double* __restrict__ gzu,
                                                const double* __restrict__ gcons, const int8_t* __restrict__ codes,
                                                const int32_t* __restrict__ ineq, double* __restrict__ u,
                                                double* __restrict__ rhs, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
  GRID_LOOP(i, A.n + A.m) {
    double ui = 0.0, ri = 0.0;
    if (i < A.nx) {
      if (!A.fixed[i]) {
        const int c = codes[i];
        if (c < 0 && gzl) ui = -(gzl[i] / A.os);
        if (c > 0 && gzu) ui = gzu[i] / A.os;
        if (gx) ri = gx[i];
      }
    } else if (i < A.n) {
      const int r = ineq[i - A.nx];
      if (gcons) ri = gcons[r] / A.cscale[r];
    } else if (gy) {
      const int r = (int)(i - A.n);
      ri = A.cscale[r] * gy[r] / A.os;
    }
    u[i] = ui;
    rhs[i] = ri;
  }
}

// r = rhs - K0 u and |r| of every row, k_pol_resid's access pattern on an arbitrary u: the rows of active and
// fixed coordinates write 0.  r (may be null) becomes the right-hand side of the next solve; keep (may be null)
// gets K0 u - rhs on the active coordinates and 0 on the others.  t1 as in k_pol_resid.
template <int G>
__global__ __launch_bounds__(NT) void k_ps_resid(DV D, const int8_t* __restrict__ codes, const double* __restrict__ u,
                                                 const double* __restrict__ rhs, double* __restrict__ r,
                                                 double* __restrict__ rowres, double* __restrict__ keep,
                                                 LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
  const int n = D.n, m = D.m;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  GROUP_LOOP(i, n + m, G) {
    double ku;
    bool act = false, masked = false;
    if (i < n) {
      double hv, jy;
      gdot2<G>(D.H, i, u, D.JT, i, u + n, hv, jy);
      ku = hv + jy;
      act = codes[i] != 0;
      masked = act || D.fixed[i];
    } else {
      ku = gdot<G>(D.J, i - n, u);
    }
    if (lead) {
      const double ri = masked ? 0.0 : rhs[i] - ku;
      if (r) r[i] = ri;
      rowres[i] = fabs(ri);
      if (keep && i < n) keep[i] = act ? ku - rhs[i] : 0.0;
    }
  }
}

// Un-scale the tangent (A.d is u; any output may be null): dx = the bound's direction on an active variable,
// dlvar on a fixed one (copies), u elsewhere (also into dxs, zeros on the slacks, for k_pst_cons);
// dy = con_scale dy~ / obj_scale; dzl = keep / obj_scale on a lower-active variable, dzu = -keep / obj_scale
// on an upper-active one, the constant 0 everywhere else.
__global__ __launch_bounds__(NT) void k_pst_out(AdjArgs A, TanDir T, const int8_t* __restrict__ codes,
                                                const double* __restrict__ keep, double* __restrict__ dxs,
                                                double* __restrict__ ox, double* __restrict__ oy,
                                                double* __restrict__ ozl, double* __restrict__ ozu) {
#pragma clang fp contract(off)
  const int ns = A.n - A.nx;
  const int top = A.nx > A.m ? A.nx : A.m;
  GRID_LOOP(i, (top > ns ? top : ns)) {
    if (i < A.nx) {
      const int c = A.fixed[i] ? -1 : codes[i];
      double dx, dzl = 0.0, dzu = 0.0;
      if (c != 0) {
        const double* b = c < 0 ? T.lvar : T.uvar;
        dx = b ? b[i] : 0.0;
        if (!A.fixed[i]) {
          const double dt = keep[i] / A.os;
          if (c < 0) dzl = dt;
          else dzu = -dt;
        }
      } else {
        dx = A.d[i];
      }
      dxs[i] = dx;
      if (ox) ox[i] = dx;
      if (ozl) ozl[i] = dzl;
      if (ozu) ozu[i] = dzu;
    }
    if (i < ns) dxs[A.nx + i] = 0.0;
    if (i < A.m && oy) oy[i] = A.d[A.n + i] * A.cscale[i] / A.os;
  }
}

// dcons_r: the bound's direction itself on an active row (a copy), else k_tan_cons' (A dx)_r + (dA x)_r
template <int G>
__global__ __launch_bounds__(NT) void k_pst_cons(DV D, AdjArgs A, TanDir T, const int8_t* __restrict__ codes,
                                                 const int32_t* __restrict__ rowslack, const double* __restrict__ dxs,
                                                 const double* __restrict__ base, double* __restrict__ ocons) {
#pragma clang fp contract(off)
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  GROUP_LOOP(r, D.m, G) {
    const double s = gdot<G>(D.J, r, dxs);
    if (lead) {
      const int k = rowslack[r], c = k >= 0 ? codes[k] : 0;
      if (c != 0) {
        const double* b = c < 0 ? T.lcon : T.ucon;
        ocons[r] = b ? b[r] : 0.0;
      } else {
        ocons[r] = s / A.cscale[r] + base[D.n + r];
      }
    }
  }
}

// The vector gradients (A.d is u = a~ - taubar~; any output may be null).  Variable i: c_i = -sgn os u_i (0 on a
// fixed one, whose lvar is k_adj_fix's and whose uvar is 0); the bound of an active variable gets beta_i =
// -keep_i, every other bound the constant 0.  Row r: an equality row lcon_r = cs_r u_y,r + gcons_r (cons_r is
// lcon_r there), ucon_r = 0; a row with slack k: cs_r beta_k on the active side, 0 elsewhere.
__global__ __launch_bounds__(NT) void k_psa_vec(AdjArgs A, const int8_t* __restrict__ codes,
                                                const double* __restrict__ keep, const int32_t* __restrict__ rowslack,
                                                const double* __restrict__ gcons, double* __restrict__ gc,
                                                double* __restrict__ glv, double* __restrict__ guv,
                                                double* __restrict__ glc, double* __restrict__ guc) {
#pragma clang fp contract(off)
  GRID_LOOP(i, (A.nx > A.m ? A.nx : A.m)) {
    if (i < A.nx) {
      const bool fx = A.fixed[i];
      const double at = fx ? 0.0 : A.d[i];
      if (gc) gc[i] = -(A.sgn * (A.os * at));
      if (!fx) {
        const int c = codes[i];
        const double b = c != 0 ? -keep[i] : 0.0;
        if (glv) glv[i] = c < 0 ? b : 0.0;
        if (guv) guv[i] = c > 0 ? b : 0.0;
      } else if (guv) {
        guv[i] = 0.0;
      }
    }
    if (i < A.m && (glc || guc)) {
      const int k = rowslack[i];
      const double cs = A.cscale[i];
      if (k < 0) {
        const double ay = cs * A.d[A.n + i];
        if (glc) glc[i] = gcons ? ay + gcons[i] : ay;
        if (guc) guc[i] = 0.0;
      } else {
        const int c = codes[k];
        const double b = c != 0 ? cs * -keep[k] : 0.0;
        if (glc) glc[i] = c < 0 ? b : 0.0;
        if (guc) guc[i] = c > 0 ? b : 0.0;
      }
    }
  }
}

const char* polish_verdict_name(int v) {
  switch (v) {
    case MADIPM_POLISHED: return "POLISHED";
    case MADIPM_POLISH_WRONG_SET: return "WRONG_SET";
    case MADIPM_POLISH_NO_CONVERGENCE: return "NO_CONVERGENCE";
    case MADIPM_POLISH_FACTORIZATION_FAILED: return "FACTORIZATION_FAILED";
  }
  return "unknown";
}

}  // namespace

// sens_refuse's refusals, then: the last polish belongs to this solved point and ended POLISHED
void MPCSolver::polished_refuse(const std::string& who) const {
  if (active_set_point()) return;  // an active-set solve's point (§13h): it checked K2 and the communicator itself
  sens_refuse(who);
  MADIPM_REQUIRE(post_ && post_->pol.point_solve == n_solves_,
                 who + "no polish has run on the point of the last solve (madipm_solver_polish first)");
  const int v = post_->pol.last.verdict;
  MADIPM_REQUIRE(v == MADIPM_POLISHED, who + "the last polish ended with verdict " + polish_verdict_name(v) +
                                           ", not POLISHED: the face has no polished point to differentiate");
}

// The polish's factor back into the LDL^T when an adjoint / tangent overwrote it: the kept codes and sigma
void MPCSolver::polished_factor(const std::string& who) {
  Polish& p = post_->pol;
  if (polish_factor_held()) return;
  p.fact_solve = -1;
  post_->adj.fact_solve = -1;  // the adjoint's factor and KKT diagonal are overwritten
  const DV D = view();
  const int nb = blocks(n_ + m_);
  if (!factor_trials([&](double dw, double dc) {
        k_pol_diag<<<nb, NT, 0, stream_>>>(D, p.codes.p, dw, dc, p.fact_sigma, fact_reset());
        timed_factorize();
      }))
    throw Error(who + "the factorisation of the polish's KKT system failed in all three trials", -4);
  polish_factor_tag(p.fact_sigma);
  ++post_->sens.n_fact;
}

// With sens.u and sens.rhs set: the masked solves in delta form, K0 u - rhs on the active coordinates into
// sens.keep, the max-norm of the final masked residual into sens.scal
void MPCSolver::polished_solve() {
  PostSolve& ps = *post_;
  Polish& p = ps.pol;
  PolSens& q = ps.sens;
  const DV D = view();
  hipStream_t s = stream_;
  const int nb = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_);
  PolArgs M{};  // k_pol_acc's masking on u: it reads the sizes, the codes, the fixed flags and w
  M.n = n_, M.m = m_, M.nx = nx_, M.fixed = fixed_.p, M.codes = p.codes.p, M.w = q.u.p;
  const int8_t* codes = p.codes.p;
  for (int it = 0; it <= p.refine_steps; ++it) {
    SPMV_LAUNCH(k_ps_resid, nbs, s, D, codes, (const double*)q.u.p, (const double*)q.rhs.p, d_.p, ps.adj.rowres.p,
                (double*)nullptr, take_fact_end());
    kkt_solve();
    k_pol_acc<<<nb, NT, 0, s>>>(M, d_.p);
  }
  SPMV_LAUNCH(k_ps_resid, nbs, s, D, codes, (const double*)q.u.p, (const double*)q.rhs.p, (double*)nullptr,
              ps.adj.rowres.p, q.keep.p, take_fact_end());
  k_adj_resmax<<<1, NT, 0, s>>>(ps.adj.rowres.p, (const double*)nullptr, (int64_t)n_ + m_, q.scal.p);
}

static void polished_scratch(PolSens& q, int n, int m, hipStream_t s) {
  if (q.u.p) return;
  q.u.alloc(std::max(n + m, 1));
  q.rhs.alloc(std::max(n + m, 1));
  q.keep.alloc(std::max(n, 1));
  q.scal.alloc(1);
  q.scal.zero(s);
}

void MPCSolver::tangent_polished(const madipm_qp_directions& dr, const madipm_qp_point_tangents& o, bool device,
                                 hipStream_t caller) {
  const std::string who = device ? "madipm_solver_tangent_polished_device: " : "madipm_solver_tangent_polished: ";
  QPHost& P = *H_;
  // ---- refusals, before anything is allocated or enqueued
  polished_refuse(who);
  const double* const dir[7] = {dr.c, dr.Hvals, dr.Avals, dr.lcon, dr.ucon, dr.lvar, dr.uvar};
  double* const user[5] = {o.x, o.y, o.zl, o.zu, o.cons};
  MADIPM_REQUIRE(dr.c || dr.Hvals || dr.Avals || dr.lcon || dr.ucon || dr.lvar || dr.uvar,
                 who + "all seven directions are NULL");
  MADIPM_REQUIRE(o.x || o.y || o.zl || o.zu || o.cons, who + "all five outputs are NULL");
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  const bool needLists = (dr.Avals && na > 0) || (dr.Hvals && nh > 0) || (dr.lvar && P.anyfix);
  MADIPM_REQUIRE(plan_ || !needLists,
                 who + "Avals, Hvals (and lvar on a problem with fixed variables) need "
                       "madipm_solver_prepare_update first (it keeps the index arrays and the raw values)");
  hipStream_t s = stream_;
  // ---- allocations, each by the first call that needs it
  PostSolve& ps = *post_;
  Tangent& t = ps.tan;
  Polish& p = ps.pol;
  PolSens& q = ps.sens;
  polished_scratch(q, n_, m_, s);
  ps.tangent_scratch(*this, needLists);
  AdjArgs A = ps.args(*this);  // the polished point in the iterate's place, u in a~'s
  A.d = q.u.p, A.x = p.w.p, A.y = p.w.p + n_;
  const int64_t dlen[7] = {nx_, nh, na, m_, m_, nx_, nx_};
  const int64_t olen[5] = {nx_, m_, nx_, nx_, m_};
  const double* ddir[7];
  double* out[5];
  q.dir.bind(dir, dlen, device, ddir);
  q.out.bind(user, olen, device, out);
  // ---- the polish's factor, if an adjoint / tangent took the LDL^T since
  const DV D = view();
  polished_factor(who);
  if (device)
    ps.sync.begin(caller, s);  // the directions are read after the work already enqueued on the caller's stream
  else
    q.dir.upload(dir, dlen, s);
  // ---- right-hand side, solves, residual
  const int nb = blocks(n_ + m_);
  const TanDir T{ddir[0], ddir[1], ddir[2], ddir[3], ddir[4], ddir[5], ddir[6]};
  const bool ls = needLists;
  k_tan_data<<<nb, NT, 0, s>>>(A, T, BLen{nh, na}, ls ? t.gsp.p : nullptr, t.ge.p, t.csp.p, t.ce.p,
                               ls ? t.asp.p : nullptr, t.ae.p, plan_ ? plan_->Hraw.p : nullptr,
                               plan_ ? plan_->Araw.p : nullptr, t.base.p);
  k_pst_rhs<<<nb, NT, 0, s>>>(A, T, (const int8_t*)p.codes.p, (const int32_t*)p.ineq.p,
                              (const int32_t*)ps.adj.rowslack.p, (const double*)t.base.p, q.u.p, q.rhs.p,
                              take_fact_end());
  polished_solve();
  // ---- outputs
  k_pst_out<<<blocks(std::max(std::max(nx_, m_), std::max(n_ - nx_, 1))), NT, 0, s>>>(
      A, T, (const int8_t*)p.codes.p, (const double*)q.keep.p, t.dx.p, out[0], out[1], out[2], out[3]);
  if (out[4] && m_)
    SPMV_LAUNCH(k_pst_cons, spmv_blocks(m_), s, D, A, T, (const int8_t*)p.codes.p, (const int32_t*)ps.adj.rowslack.p,
                (const double*)t.dx.p, (const double*)t.base.p, out[4]);
  MADIPM_HIP(hipGetLastError());
  if (device)
    ps.sync.end(s, caller);  // work enqueued on the caller's stream from now on sees the outputs
  else
    q.out.download(user, olen, s);
  ++q.n_tangents;
}

void MPCSolver::adjoint_polished(const madipm_qp_cotangents& ct, const madipm_qp_gradients& g, bool device,
                                 hipStream_t caller) {
  const std::string who = device ? "madipm_solver_adjoint_polished_device: " : "madipm_solver_adjoint_polished: ";
  QPHost& P = *H_;
  // ---- refusals, before anything is allocated or enqueued
  polished_refuse(who);
  MADIPM_REQUIRE(ct.x || ct.y || ct.zl || ct.zu || ct.cons, who + "all five cotangents are NULL");
  double* const user[7] = {g.c, g.Hvals, g.Avals, g.lcon, g.ucon, g.lvar, g.uvar};
  MADIPM_REQUIRE(g.c || g.Hvals || g.Avals || g.lcon || g.ucon || g.lvar || g.uvar,
                 who + "all seven outputs are NULL");
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  const bool needA = g.Avals && na > 0, needH = g.Hvals && nh > 0, needFix = g.lvar && P.anyfix;
  MADIPM_REQUIRE(plan_ || !(needA || needH || needFix),
                 who + "Avals, Hvals (and lvar on a problem with fixed variables) need "
                       "madipm_solver_prepare_update first (it keeps the index arrays and the raw values)");
  hipStream_t s = stream_;
  // ---- allocations, each by the first call that needs it
  PostSolve& ps = *post_;
  Adjoint& a = ps.adj;
  Polish& p = ps.pol;
  PolSens& q = ps.sens;
  polished_scratch(q, n_, m_, s);
  ps.adjoint_lists(*this, needA, needH, needFix);
  AdjArgs A = ps.args(*this);  // the polished point in the iterate's place, u in a~'s
  A.d = q.u.p, A.x = p.w.p, A.y = p.w.p + n_;
  const double* const cot[5] = {ct.x, ct.y, ct.zl, ct.zu, ct.cons};
  const int64_t clen[5] = {nx_, m_, nx_, nx_, m_};
  const double* dct[5];  // gx, gy, gzl, gzu, gcons on the device
  q.ct.bind(cot, clen, device, dct);
  const int64_t len[7] = {nx_, nh, na, m_, m_, nx_, nx_};
  double* out[7];
  q.grad.bind(user, len, device, out);
  // ---- the polish's factor, if an adjoint / tangent took the LDL^T since
  polished_factor(who);
  if (device)
    ps.sync.begin(caller, s);  // the cotangents are read after the work already enqueued on the caller's stream
  else
    q.ct.upload(cot, clen, s);
  // ---- right-hand side, solves, residual
  k_psa_rhs<<<blocks(n_ + m_), NT, 0, s>>>(A, dct[0], dct[1], dct[2], dct[3], dct[4], (const int8_t*)p.codes.p,
                                           (const int32_t*)p.ineq.p, q.u.p, q.rhs.p, take_fact_end());
  polished_solve();
  // ---- gradients: §13c's kernels with u in a~'s place and the polished point in the iterate's
  const AdjFull F{nullptr, nullptr, nullptr, nullptr};
  if ((out[0] || out[3] || out[4] || out[5] || out[6]) && std::max(nx_, m_))
    k_psa_vec<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, (const int8_t*)p.codes.p, (const double*)q.keep.p,
                                                       (const int32_t*)a.rowslack.p, dct[4], out[0], out[5], out[6],
                                                       out[3], out[4]);
  if (needFix && a.nfix > 0)  // <true> with no gcons: gx may be null, and cons reaches a fixed column through u_y
    k_adj_fix<true><<<blocks(a.nfix), NT, 0, s>>>(A, F, a.nfix, a.fix.p, a.fhsp.p, a.fh.p, a.fasp.p, a.fa.p,
                                                  plan_->Hraw.p, plan_->Araw.p, dct[0], out[5]);
  if (needA) k_adj_avals<false><<<blocks(na), NT, 0, s>>>(A, F, na, a.Ar.p, a.Ac.p, out[2]);
  if (needH) k_adj_hvals<<<blocks(nh), NT, 0, s>>>(A, nh, a.Hr.p, a.Hc.p, out[1]);
  MADIPM_HIP(hipGetLastError());
  if (device)
    ps.sync.end(s, caller);  // work enqueued on the caller's stream from now on sees the outputs
  else
    q.grad.download(user, len, s);
  ++q.n_adjoints;
}

void MPCSolver::polished_sens_info(int64_t* n_tangents, int64_t* n_adjoints, int64_t* n_factorizations,
                                   double* last_residual) {
  const PolSens* q = post_ ? &post_->sens : nullptr;
  if (n_tangents) *n_tangents = q ? q->n_tangents : 0;
  if (n_adjoints) *n_adjoints = q ? q->n_adjoints : 0;
  if (n_factorizations) *n_factorizations = q ? q->n_fact : 0;
  const int64_t calls = q ? q->n_tangents + q->n_adjoints : 0;
  read_residual(last_residual, calls, calls ? q->scal.p : nullptr, stream_);
}

}  // namespace madipm

// ======================================================================= one column or k: the host path
// madipm_solver_tangent / _adjoint are one column on a SensView of the single calls' scratch,
// madipm_solver_tangent_batch / _adjoint_batch / _device k columns of one point in chunks of kc <= SENS_W on the
// view of SensBatch: one implementation of each (tangent_cols, adjoint_cols) and one refined solve (sens_solve),
// launching §13c-§13e's kernels with the chunk's columns in gridDim.y.  Only the residual has two kernels: a
// chunk of one column runs k_adj_resid, a chunk of more k_adj_resid_b below, whose lane groups load a row's
// entries and column indices once and gather from each column's vector.  The solves are ldl_->solve_async on one
// column after the other.
namespace madipm {
namespace {

// The refinement residual of the chunk's kc columns (k_adj_resid for each): a lane group per K2 row loads its
// entries of H~ and J~^T (or J~) and their column indices once per trip, two entries a trip as gdot / gdot2 issue
// them, and gathers from each column's vector; one fma chain per column in gdot's order, each with gdot's
// butterfly; Sigma_l + Sigma_u once per row.  g: the kept right-hand sides; v: the current a~; r (may be null):
// the next solves' right-hand sides.
template <int G>
__device__ __forceinline__ void gdot_b(const DCsr& A, int64_t row, const double* __restrict__ x, int64_t ld, int kc,
                                       double (&s)[SENS_W]) {
  const int gl = threadIdx.x & (G - 1);
#pragma unroll
  for (int j = 0; j < SENS_W; ++j) s[j] = 0.0;
  const int64_t q1 = A.rp[row + 1];
  for (int64_t q = A.rp[row] + gl; q < q1; q += 2 * G) {
    const int64_t qb = min(q + G, q1 - 1);
    const double va = A.v[q], vb = A.v[qb];
    const int64_t ca = A.ci[q], cb = A.ci[qb];
    const double vb0 = (q + G < q1) ? vb : 0.0;
    double xa[SENS_W], xb[SENS_W];
#pragma unroll
    for (int j = 0; j < SENS_W; ++j)
      if (j < kc) {
        xa[j] = x[ca + j * ld];
        xb[j] = x[cb + j * ld];
      }
#pragma unroll
    for (int j = 0; j < SENS_W; ++j)
      if (j < kc) {
        s[j] = fma(va, xa[j], s[j]);
        s[j] = fma(vb0, xb[j], s[j]);
      }
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < SENS_W; ++j)
      if (j < kc) s[j] += __shfl_xor(s[j], o, G);
  }
}

template <int G>
__device__ __forceinline__ void gdot2_b(const DCsr& A, int64_t ra, const double* __restrict__ xa, const DCsr& B,
                                        int64_t rb, const double* __restrict__ xb, int64_t ld, int kc,
                                        double (&sa)[SENS_W], double (&sb)[SENS_W]) {
  const int gl = threadIdx.x & (G - 1);
  const int64_t a1 = A.rp[ra + 1], b1 = B.rp[rb + 1];
  int64_t qa = A.rp[ra] + gl, qb = B.rp[rb] + gl;
#pragma unroll
  for (int j = 0; j < SENS_W; ++j) {
    sa[j] = 0.0;
    sb[j] = 0.0;
  }
  while (qa < a1 || qb < b1) {
    const bool ta = qa < a1, tb = qb < b1;
    double va = 0.0, va2 = 0.0, vb = 0.0, vb2 = 0.0;
    int64_t ia = 0, ia2 = 0, ib = 0, ib2 = 0;
    if (ta) {
      const int64_t q2 = min(qa + G, a1 - 1);
      va = A.v[qa];
      va2 = (qa + G < a1) ? A.v[q2] : 0.0;
      ia = A.ci[qa];
      ia2 = A.ci[q2];
    }
    if (tb) {
      const int64_t q2 = min(qb + G, b1 - 1);
      vb = B.v[qb];
      vb2 = (qb + G < b1) ? B.v[q2] : 0.0;
      ib = B.ci[qb];
      ib2 = B.ci[q2];
    }
    double ya[SENS_W], ya2[SENS_W], yb[SENS_W], yb2[SENS_W];
#pragma unroll
    for (int j = 0; j < SENS_W; ++j)
      if (j < kc) {
        if (ta) {
          ya[j] = xa[ia + j * ld];
          ya2[j] = xa[ia2 + j * ld];
        }
        if (tb) {
          yb[j] = xb[ib + j * ld];
          yb2[j] = xb[ib2 + j * ld];
        }
      }
#pragma unroll
    for (int j = 0; j < SENS_W; ++j)
      if (j < kc) {
        if (ta) {
          sa[j] = fma(va, ya[j], sa[j]);
          sa[j] = fma(va2, ya2[j], sa[j]);
        }
        if (tb) {
          sb[j] = fma(vb, yb[j], sb[j]);
          sb[j] = fma(vb2, yb2[j], sb[j]);
        }
      }
    if (ta) qa += 2 * G;
    if (tb) qb += 2 * G;
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < SENS_W; ++j)
      if (j < kc) {
        sa[j] += __shfl_xor(sa[j], o, G);
        sb[j] += __shfl_xor(sb[j], o, G);
      }
  }
}

template <int G>
__global__ __launch_bounds__(NT) void k_adj_resid_b(DV D, AdjArgs A, int kc, const double* __restrict__ g,
                                                    const double* __restrict__ v, double* __restrict__ r,
                                                    double* __restrict__ rowres) {
  const int n = D.n, m = D.m;
  const int64_t N = (int64_t)n + m;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  GROUP_LOOP(i, n + m, G) {
    double kv[SENS_W];
    if (i < n) {
      double hd[SENS_W], jd[SENS_W];
      gdot2_b<G>(D.H, i, v, D.JT, i, v + n, N, kc, hd, jd);
      const double sig = adj_sig_l(A, (int)i) + adj_sig_u(A, (int)i);
#pragma unroll
      for (int j = 0; j < SENS_W; ++j)
        if (j < kc) kv[j] = (hd[j] + jd[j]) + sig * v[i + j * N];
    } else {
      gdot_b<G>(D.J, i - n, v, N, kc, kv);
    }
    if (lead) {
#pragma unroll
      for (int j = 0; j < SENS_W; ++j)
        if (j < kc) {
          const double ri = g[i + j * N] - kv[j];
          if (r) r[i + j * N] = ri;
          rowres[i + j * N] = fabs(ri);
        }
    }
  }
}

// out[0] = the largest of the chunk's ratios and, after the call's first chunk, of out[0] (a NaN is kept)
__global__ void k_sens_fold(const double* __restrict__ col, int kc, int first, double* __restrict__ out) {
  if (blockIdx.x || threadIdx.x) return;
  double w = first ? col[0] : out[0];
  for (int j = first ? 1 : 0; j < kc; ++j) w = nmax(w, col[j]);
  out[0] = w;
}

// column c0 of a block of the caller's (null stays null)
template <class T>
T* at_col(T* p, int64_t c0, int64_t len) {
  return p ? p + c0 * len : nullptr;
}

// launch a GROUP_LOOP SpMV kernel over the chunk's columns (grid.y) with the problem's lane-group width
#define SPMV_LAUNCH_B(kern, grid, kc, strm, ...)                                             \
  do {                                                                                       \
    switch (spmv_g_) {                                                                       \
      case 4: kern<4><<<dim3((grid), (kc)), NT, 0, (strm)>>>(__VA_ARGS__); break;            \
      case 8: kern<8><<<dim3((grid), (kc)), NT, 0, (strm)>>>(__VA_ARGS__); break;            \
      case 16: kern<16><<<dim3((grid), (kc)), NT, 0, (strm)>>>(__VA_ARGS__); break;          \
      case 32: kern<32><<<dim3((grid), (kc)), NT, 0, (strm)>>>(__VA_ARGS__); break;          \
      default: kern<64><<<dim3((grid), (kc)), NT, 0, (strm)>>>(__VA_ARGS__); break;          \
    }                                                                                        \
  } while (0)

}  // namespace

int MPCSolver::sens_batch_cols() { return SENS_W; }

// With a chunk's kc right-hand sides in V.d (and in V.p, which keeps them): V.sol = K^-1 V.p column by column,
// refined; the largest residual ratio of the call so far into resid[0]
void MPCSolver::sens_solve(const SensView& V, int kc, double* resid, bool first_chunk) {
  AdjArgs A = post_->args(*this);
  A.d = V.sol;
  const DV D = view();
  hipStream_t s = stream_;
  const int64_t N = (int64_t)n_ + m_;
  const int nb = blocks(kc * N), nbs = spmv_blocks(n_ + m_);
  // kkt_solve() of the K2 formulation (sens_refuse admits no other), on each column; a batch with
  // set_multi_solve on: the chunk's columns in one multi-right-hand-side solve, a chunk of one column too
  const bool multi = multi_solve_ && V.W > 1;
  auto solves = [&] {
    if (multi) return ldl_->solve_multi_async(V.d, kc, s);
    for (int j = 0; j < kc; ++j) ldl_->solve_async(V.d + j * N, s);
  };
  auto residual = [&](double* r) {
    if (kc == 1)
      SPMV_LAUNCH(k_adj_resid, nbs, s, D, A, (const double*)V.p, (const double*)V.sol, r, V.rowres);
    else
      SPMV_LAUNCH(k_adj_resid_b, nbs, s, D, A, kc, (const double*)V.p, (const double*)V.sol, r, V.rowres);
  };
  solves();
  k_adj_acc<<<nb, NT, 0, s>>>(V.sol, V.d, kc * N, 1);  // the columns are contiguous: one flat pass
  // iterative refinement towards the system without the regularisation (the factor is the regularised
  // matrix's: each step gains about -log10(delta |K^-1|) digits); a fixed count, so nothing is read back
  for (int it = 0; it < adj_refine_steps(); ++it) {
    residual(V.d);
    solves();
    k_adj_acc<<<nb, NT, 0, s>>>(V.sol, V.d, kc * N, 0);
  }
  residual(nullptr);
  // a first chunk of one column (every single call) is the call's ratio itself: no fold
  const bool direct = first_chunk && kc == 1;
  k_adj_resmax<<<kc, NT, 0, s>>>(V.rowres, V.p, N, direct ? resid : V.scal);
  if (!direct) k_sens_fold<<<1, 1, 0, s>>>(V.scal, kc, first_chunk ? 1 : 0, resid);
}

// The tangents of k columns of directions (§13e), in chunks of the view's width.  batch: on SensBatch, else
// k = 1 on the single call's scratch; polished: one tangent_polished per column, with offset pointers (its bits
// by construction).  Returns the chunks run.
int64_t MPCSolver::tangent_cols(const std::string& who, int64_t k, bool batch, bool polished,
                                const madipm_qp_directions& dr, const madipm_qp_point_tangents& o, bool device,
                                hipStream_t caller) {
  QPHost& P = *H_;
  // ---- refusals, before anything is allocated or enqueued
  if (polished)
    polished_refuse(who);
  else
    sens_refuse(who);
  const double* const dir[7] = {dr.c, dr.Hvals, dr.Avals, dr.lcon, dr.ucon, dr.lvar, dr.uvar};
  double* const user[5] = {o.x, o.y, o.zl, o.zu, o.cons};
  MADIPM_REQUIRE(dr.c || dr.Hvals || dr.Avals || dr.lcon || dr.ucon || dr.lvar || dr.uvar,
                 who + "all seven directions are NULL");
  MADIPM_REQUIRE(o.x || o.y || o.zl || o.zu || o.cons, who + "all five outputs are NULL");
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  const bool needLists = (dr.Avals && na > 0) || (dr.Hvals && nh > 0) || (dr.lvar && P.anyfix);
  MADIPM_REQUIRE(plan_ || !needLists,
                 who + "Avals, Hvals (and lvar on a problem with fixed variables) need "
                       "madipm_solver_prepare_update first (it keeps the index arrays and the raw values)");
  const int64_t dlen[7] = {nx_, nh, na, m_, m_, nx_, nx_};
  const int64_t olen[5] = {nx_, m_, nx_, nx_, m_};
  if (polished) {
    for (int64_t j = 0; j < k; ++j) {
      const madipm_qp_directions dj{at_col(dir[0], j, dlen[0]), at_col(dir[1], j, dlen[1]), at_col(dir[2], j, dlen[2]),
                                    at_col(dir[3], j, dlen[3]), at_col(dir[4], j, dlen[4]), at_col(dir[5], j, dlen[5]),
                                    at_col(dir[6], j, dlen[6])};
      const madipm_qp_point_tangents oj{at_col(user[0], j, olen[0]), at_col(user[1], j, olen[1]),
                                        at_col(user[2], j, olen[2]), at_col(user[3], j, olen[3]),
                                        at_col(user[4], j, olen[4])};
      tangent_polished(dj, oj, device, caller);
    }
    return 0;
  }
  hipStream_t s = stream_;
  // ---- allocations, each by the first call that needs it
  PostSolve& ps = post_state();
  Adjoint& a = ps.adj;
  Tangent& t = ps.tan;
  ps.rowslack(P, s);
  ps.tangent_scratch(*this, needLists);
  const SensView V = ps.sens_view(*this, batch, true, true);  // shifted, as the five-cotangent adjoint
  int64_t dcap[7], ocap[5];  // a chunk's staging
  for (int q = 0; q < 7; ++q) dcap[q] = V.W * dlen[q];
  for (int q = 0; q < 5; ++q) ocap[q] = V.W * olen[q];
  const double* ddir[7];
  double* out[5];
  V.dir->bind(dir, dcap, device, ddir);
  V.out->bind(user, ocap, device, out);
  AdjArgs A = ps.args(*this);
  A.d = V.sol;
  const BLen L{nh, na};
  // ---- the factor of the K2 matrix at the final iterate: the adjoint's, once per solve
  const DV D = view();
  sens_factor(who);
  if (device) ps.sync.begin(caller, s);  // the directions are read after the work already enqueued on the caller's stream
  const bool ls = needLists;  // lists built by an earlier call are not walked when this one has no use for them
  const int nbv = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_);
  int64_t chunks = 0;
  for (int64_t c0 = 0; c0 < k; c0 += V.W, ++chunks) {
    const int kc = (int)std::min<int64_t>(V.W, k - c0);
    const int64_t co = device ? c0 : 0;  // the host route stages the chunk's columns from 0
    if (!device) {
      const double* uc[7];
      int64_t ul[7];
      for (int q = 0; q < 7; ++q) uc[q] = at_col(dir[q], c0, dlen[q]), ul[q] = kc * dlen[q];
      V.dir->upload(uc, ul, s);
    }
    // ---- right-hand sides, solves, residuals
    const TanDir T{at_col(ddir[0], co, dlen[0]), at_col(ddir[1], co, dlen[1]), at_col(ddir[2], co, dlen[2]),
                   at_col(ddir[3], co, dlen[3]), at_col(ddir[4], co, dlen[4]), at_col(ddir[5], co, dlen[5]),
                   at_col(ddir[6], co, dlen[6])};
    k_tan_shift<<<dim3(nbv, kc), NT, 0, s>>>(A, T, L, a.rowslack.p, V.shift, take_fact_end());
    k_tan_data<<<dim3(nbv, kc), NT, 0, s>>>(A, T, L, ls ? t.gsp.p : nullptr, t.ge.p, t.csp.p, t.ce.p,
                                           ls ? t.asp.p : nullptr, t.ae.p, plan_ ? plan_->Hraw.p : nullptr,
                                           plan_ ? plan_->Araw.p : nullptr, V.base);
    SPMV_LAUNCH_B(k_tan_rhs, nbs, kc, s, D, A, T, L, (const int32_t*)a.rowslack.p, (const double*)V.shift,
                  (const double*)V.base, V.d, V.p);
    sens_solve(V, kc, t.scal.p, c0 == 0);
    // ---- outputs
    k_tan_out<<<dim3(blocks(std::max(std::max(nx_, m_), std::max(n_ - nx_, 1))), kc), NT, 0, s>>>(
        A, T, L, V.shift, V.dx, at_col(out[0], co, olen[0]), at_col(out[1], co, olen[1]),
        at_col(out[2], co, olen[2]), at_col(out[3], co, olen[3]));
    if (out[4] && m_)
      SPMV_LAUNCH_B(k_tan_cons, spmv_blocks(m_), kc, s, D, A, (const double*)V.dx, (const double*)V.base,
                    at_col(out[4], co, olen[4]));
    MADIPM_HIP(hipGetLastError());
    if (!device) {
      double* uc[5];
      int64_t ul[5];
      for (int q = 0; q < 5; ++q) uc[q] = at_col(user[q], c0, olen[q]), ul[q] = kc * olen[q];
      V.out->download(uc, ul, s);  // synchronises: the next chunk reuses the staging
    }
  }
  if (device) ps.sync.end(s, caller);  // work enqueued on the caller's stream from now on sees the outputs
  t.n_tangents += k;
  return chunks;
}

// The adjoints of k columns of cotangents (§13c, §13d), as tangent_cols.  need_gx: the entry point takes gx alone,
// which must be given.  full: a cotangent block other than gx is given, and every column solves the shifted system
// of §13d; without one the kernels and their order are those of the gx-only call whichever entry point was taken.
int64_t MPCSolver::adjoint_cols(const std::string& who, int64_t k, bool batch, bool polished, bool need_gx,
                                const madipm_qp_cotangents& ct, const madipm_qp_gradients& g, bool device,
                                hipStream_t caller) {
  QPHost& P = *H_;
  // ---- refusals, before anything is allocated or enqueued
  if (polished)
    polished_refuse(who);
  else
    sens_refuse(who);
  const bool full = ct.y || ct.zl || ct.zu || ct.cons;
  if (need_gx)
    MADIPM_REQUIRE(ct.x, who + "gx is NULL");
  else
    MADIPM_REQUIRE(ct.x || full, who + "all five cotangents are NULL");
  double* const user[7] = {g.c, g.Hvals, g.Avals, g.lcon, g.ucon, g.lvar, g.uvar};
  MADIPM_REQUIRE(g.c || g.Hvals || g.Avals || g.lcon || g.ucon || g.lvar || g.uvar,
                 who + "all seven outputs are NULL");
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  const bool needA = g.Avals && na > 0, needH = g.Hvals && nh > 0, needFix = g.lvar && P.anyfix;
  MADIPM_REQUIRE(plan_ || !(needA || needH || needFix),
                 who + "Avals, Hvals (and lvar on a problem with fixed variables) need "
                       "madipm_solver_prepare_update first (it keeps the index arrays and the raw values)");
  const double* const cot[5] = {ct.x, ct.y, ct.zl, ct.zu, ct.cons};
  const int64_t clen[5] = {nx_, m_, nx_, nx_, m_};
  const int64_t len[7] = {nx_, nh, na, m_, m_, nx_, nx_};
  if (polished) {
    for (int64_t j = 0; j < k; ++j) {
      const madipm_qp_cotangents cj{at_col(cot[0], j, clen[0]), at_col(cot[1], j, clen[1]), at_col(cot[2], j, clen[2]),
                                    at_col(cot[3], j, clen[3]), at_col(cot[4], j, clen[4])};
      const madipm_qp_gradients gj{at_col(user[0], j, len[0]), at_col(user[1], j, len[1]), at_col(user[2], j, len[2]),
                                   at_col(user[3], j, len[3]), at_col(user[4], j, len[4]), at_col(user[5], j, len[5]),
                                   at_col(user[6], j, len[6])};
      adjoint_polished(cj, gj, device, caller);
    }
    return 0;
  }
  hipStream_t s = stream_;
  // ---- allocations, each by the first call that needs it
  PostSolve& ps = post_state();
  Adjoint& a = ps.adj;
  const SensView V = ps.sens_view(*this, batch, full, false);
  if (g.lcon || g.ucon) ps.rowslack(P, s);
  ps.adjoint_lists(*this, needA, needH, needFix);
  int64_t ccap[5], gcap[7];  // a chunk's staging
  for (int q = 0; q < 5; ++q) ccap[q] = V.W * clen[q];
  for (int q = 0; q < 7; ++q) gcap[q] = V.W * len[q];
  const double* dct[5];  // gx, gy, gzl, gzu, gcons on the device
  double* out[7];
  V.ct->bind(cot, ccap, device, dct);
  V.grad->bind(user, gcap, device, out);
  AdjArgs A = ps.args(*this);
  A.d = V.sol;
  const int64_t N = (int64_t)n_ + m_;
  // ---- the factor of the K2 matrix at the final iterate: once per solve
  const DV D = view();
  sens_factor(who);
  if (device) ps.sync.begin(caller, s);  // the cotangents are read after the work already enqueued on the caller's stream
  const int nbv = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_);
  const bool vec = (out[0] || out[3] || out[4] || out[5] || out[6]) && std::max(nx_, m_);
  const bool fix = needFix && a.nfix > 0;
  int64_t chunks = 0;
  for (int64_t c0 = 0; c0 < k; c0 += V.W, ++chunks) {
    const int kc = (int)std::min<int64_t>(V.W, k - c0);
    const int64_t co = device ? c0 : 0;  // the host route stages the chunk's columns from 0
    if (!device) {
      const double* uc[5];
      int64_t ul[5];
      for (int q = 0; q < 5; ++q) uc[q] = at_col(cot[q], c0, clen[q]), ul[q] = kc * clen[q];
      V.ct->upload(uc, ul, s);
    }
    const double* const gx = at_col(dct[0], co, clen[0]);
    const double* const gy = at_col(dct[1], co, clen[1]);
    const AdjFull F{at_col(dct[2], co, clen[2]), at_col(dct[3], co, clen[3]), at_col(dct[4], co, clen[4]), V.apx};
    double* oc[7];
    for (int q = 0; q < 7; ++q) oc[q] = at_col(out[q], co, len[q]);
    // ---- right-hand sides, solves, residuals
    if (full) {  // the shifted system K a~' = g' (§13d); V.p keeps g' for the residual
      k_adj_shift<<<dim3(nbv, kc), NT, 0, s>>>(A, F, V.shift, take_fact_end());
      SPMV_LAUNCH_B(k_adj_rhs_full, nbs, kc, s, D, A, gx, gy, (const double*)V.shift, V.d, V.p);
    } else {
      k_adj_rhs<<<dim3(nbv, kc), NT, 0, s>>>(D, gx, V.d, V.p, take_fact_end());
    }
    sens_solve(V, kc, a.scal.p, c0 == 0);
    if (full && nx_) k_adj_unshift<<<dim3(blocks(nx_), kc), NT, 0, s>>>(nx_, N, V.shift, V.sol, V.apx);
    // ---- gradients
    auto gradients = [&](auto is_full) {  // the <true> instantiations read F (§13d)
      constexpr bool FULL = decltype(is_full)::value;
      if (vec)
        k_adj_vec<FULL><<<dim3(blocks(std::max(nx_, m_)), kc), NT, 0, s>>>(A, F, a.rowslack.p, oc[0], oc[5], oc[6],
                                                                          oc[3], oc[4]);
      if (fix)
        k_adj_fix<FULL><<<dim3(blocks(a.nfix), kc), NT, 0, s>>>(A, F, a.nfix, a.fix.p, a.fhsp.p, a.fh.p, a.fasp.p,
                                                               a.fa.p, plan_->Hraw.p, plan_->Araw.p, gx, oc[5]);
      if (needA) k_adj_avals<FULL><<<dim3(blocks(na), kc), NT, 0, s>>>(A, F, na, a.Ar.p, a.Ac.p, oc[2]);
    };
    if (full)
      gradients(std::true_type{});
    else
      gradients(std::false_type{});
    if (needH) k_adj_hvals<<<dim3(blocks(nh), kc), NT, 0, s>>>(A, nh, a.Hr.p, a.Hc.p, oc[1]);
    MADIPM_HIP(hipGetLastError());
    if (!device) {
      double* uc[7];
      int64_t ul[7];
      for (int q = 0; q < 7; ++q) uc[q] = at_col(user[q], c0, len[q]), ul[q] = kc * len[q];
      V.grad->download(uc, ul, s);  // synchronises: the next chunk reuses the staging
    }
  }
  if (device) ps.sync.end(s, caller);  // work enqueued on the caller's stream from now on sees the outputs
  a.n_adjoints += k;
  return chunks;
}

void MPCSolver::tangent_batch(int32_t k, const madipm_qp_directions& dr, const madipm_qp_point_tangents& o,
                              bool polished, bool device, hipStream_t caller) {
  const std::string who = device ? "madipm_solver_tangent_batch_device: " : "madipm_solver_tangent_batch: ";
  MADIPM_REQUIRE(k >= 1, who + "k = " + std::to_string(k) + ", a batch holds at least one column");
  const int64_t chunks = tangent_cols(who, k, true, polished, dr, o, device, caller);
  post_->bat.count(k, chunks);
}

void MPCSolver::adjoint_batch(int32_t k, const madipm_qp_cotangents& ct, const madipm_qp_gradients& g, bool polished,
                              bool device, hipStream_t caller) {
  const std::string who = device ? "madipm_solver_adjoint_batch_device: " : "madipm_solver_adjoint_batch: ";
  MADIPM_REQUIRE(k >= 1, who + "k = " + std::to_string(k) + ", a batch holds at least one column");
  const int64_t chunks = adjoint_cols(who, k, true, polished, false, ct, g, device, caller);
  post_->bat.count(k, chunks);
}

void MPCSolver::sens_batch_info(int64_t* n_batches, int64_t* n_columns, int64_t* n_chunks) const {
  const SensBatch* b = post_ ? &post_->bat : nullptr;
  if (n_batches) *n_batches = b ? b->n_batches : 0;
  if (n_columns) *n_columns = b ? b->n_columns : 0;
  if (n_chunks) *n_chunks = b ? b->n_chunks : 0;
}

}  // namespace madipm
