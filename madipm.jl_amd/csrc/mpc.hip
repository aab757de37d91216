// Native MPC driver + fused IPM vector kernels (gfx950).
//
// Restates MadIPM's per-iteration path on the GPU (file:line relative to the reference root):
//   update_termination_criteria!  src/solver.jl:194-222  -> k_term + k_final(TERM)
//   set_aug_diagonal_reg! (K2)    src/kernels.jl:124-136 -> k_diag (also writes the K2 diagonal)
//   factorize_regularized_system! src/linear_solver.jl:6-17 -> LDLSolver::factorize_async (+retry)
//   set_predictive_rhs! / set_correction_rhs! / reduce_rhs!  src/kernels.jl:21-58 -> k_rhs
//   solve_system! + finish_aug_solve! + residual (mul!, _kktmul!)  src/linear_solver.jl:19-44 -> k_residual
//   get_fraction_to_boundary_step (max-ratio test)  src/kernels.jl:226-289 -> k_alpha (argmin)
//   get_(affine_)complementarity_measure, update_barrier!  src/kernels.jl:155-220 -> k_mu
//   update_step! (Adaptive/Conservative/MehrotraAdaptive)  src/kernels.jl:291-358 -> k_alpha/k_mu FINAL
//   apply_step! + adjust_boundary!  src/solver.jl:308-317 -> k_apply
//   evaluate_model!  src/solver.jl:319-326 -> k_eval (SpMV H x, J x, J^T y, objective)
//   init_starting_point!  src/solver.jl:6-125 -> k_init_kkt, k_rhs(INIT_*), k_zinit, k_zshift1/2
// Reductions are two-pass (per-block partials, then one finalising block in fixed order), so every
// scalar is bitwise reproducible run to run; all scalars stay on the device and the host reads one
// 200-byte state block per iteration (published by k_publish into coherent host memory; the host
// spins on its counter, overlapped with the factorisation and the speculated directions).
#include <algorithm>
#include <array>
#include <atomic>
#include <thread>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>

#include "mpc.hpp"
#include "qp_model.hpp"

namespace madipm {

// the model's index pairs are uploaded as the kernels' int2
static_assert(sizeof(I2) == sizeof(int2) && alignof(I2) <= alignof(int2) && offsetof(I2, x) == offsetof(int2, x) &&
                  offsetof(I2, y) == offsetof(int2, y),
              "qp_model.hpp's I2 must have int2's layout");
static const int2* as_int2(const std::vector<I2>& v) { return reinterpret_cast<const int2*>(v.data()); }

// The refresh plan on the device (prepare_update; the host arrays are qp_model.hpp's RefreshPlan)
struct UpdatePlan {
  std::vector<int32_t> Ar, Ac;  // host copy of A's COO for the host passes (slack start, row maxima, cfix)
  std::vector<double> Av;
  DBuf<double> Araw, Hraw, cscale;      // device staging: raw Avals / Hvals, con_scale
  DBuf<int32_t> tsp, tsrc, jtk, j2jt;   // J^T entry -> sources, -> its Kx_ slot; J entry -> J^T entry
  DBuf<int32_t> hsp, hsrc, hk, hdpos;   // H entry -> sources, -> its Kx_ slot (-1: upper triangle);
                                        // hdpos[i] = H's entry (i, i) or -1
  int64_t nJ = 0, nH = 0;               // destination entries of J (= J^T) and H
};

// The device route (update_device), allocated by its first call: the raw problem numbers as last installed
// (A's and H's are the plan's Araw / Hraw), the start vectors initialize() restarts from, and the lists
// that give every host sum of numeric_host its input order: per destination [sp[i], sp[i + 1]) of
// (input index, other index) pairs, 8 B each.  Per entry of A: 8 B (row lists) + 8 B per entry in a fixed
// column; per stored entry of H: 8 B per endpoint (16 B off the diagonal), + 8 B per fixed / free cross
// entry, + 12 B per entry between two fixed variables; 4 B per row and per variable for each sp.
struct DevUpdate {
  DBuf<double> c, lvar, uvar, lcon, ucon, x0, y0;  // raw staging (y0 is also the start y)
  DBuf<double> x, xl, xu;                          // start vectors of [x; s], scaled
  DBuf<double> xpre, ax, sc;                       // structural start before the push, A x, scalar block
  DBuf<int32_t> chk, ineq;                         // the check's result block; ind_ineq
  DBuf<uint8_t> vcls, ccls;                        // creation-time bound classes
  DBuf<int32_t> asp, fsp, gsp, xsp, bfk;
  DBuf<int2> ae, fe, ge, xe, bfrc;
  int nbf = 0;
  hipEvent_t ev = nullptr;
  double* hsc = nullptr;  // pinned: SC_LEN scalars + the check block behind them
  ~DevUpdate() {
    if (ev) (void)hipEventDestroy(ev);
    if (hsc) (void)hipHostFree(hsc);
  }
};

// The warm point (set_warm_start*), kept on the device in the public, un-scaled space: obj_scale and
// con_scale may change with the next update.  8 B x (3 nvar + ncon) + 12 B per inequality row (the row
// values of k_warm_rows and the slack -> row map), allocated by the first call that sets a point.
struct WarmStart {
  DBuf<double> x, y, zl, zu, rows;
  DBuf<int32_t> ineq;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool has[4] = {false, false, false, false};  // x, y, zl, zu of the current point
  bool active = false;
  double weight = 0.0;
  ~WarmStart() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
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
  DBuf<double> gx, sol, rowres, scal;     // host route's gx; a~ (refined); |g - K a~| per row; [residual ratio, unused]
  DBuf<int32_t> rowslack;                 // row -> its slack (index into [nx, n)) or -1 (equality row)
  DBuf<int32_t> Ar, Ac, Hr, Hc;           // COO indices, creation-time entry order
  DBuf<int32_t> fix, fhsp, fasp;          // fixed variables; their list starts into fh / fa
  DBuf<int2> fh, fa;                      // (entry of Hvals, free endpoint), (entry of Avals, row)
  int nfix = -1;                          // -1: lists not built yet
  DBuf<double> out[7];                    // host route: c, Hvals, Avals, lcon, ucon, lvar, uvar
  // the loss of all five blocks (§13d), by the first call with a cotangent other than gx: 8 B x (n + m + nvar)
  DBuf<double> shift, apx;                // v = [q~; 0; gcons / con_scale]; a~'x of the shifted system
  DBuf<double> ct[4];                     // host route's gy, gzl, gzu, gcons
  hipEvent_t ev[2] = {nullptr, nullptr};
  int64_t n_adjoints = 0, n_fact = 0;
  int64_t fact_solve = -1;                // n_solves_ of the point the LDL^T currently holds the factor of
  ~Adjoint() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// The tangent (madipm_solver_tangent*) shares the adjoint's factor, solution, residual rows and
// events.  Its own, each allocated by the first call that needs it: the data terms and the full dx
// (8 B x (2 n + m + 1)); the shift vector is the adjoint's `shift`; rowslack as there; with Hvals / Avals (or
// lvar on a problem with fixed variables) the entry lists of build_tangent_lists: 16 B per entry of A, 8 B per
// endpoint of a stored entry of H, 4 B x (2 nvar + ncon) list starts; the host route's staging of the
// directions given and the outputs wanted (8 B per entry).
struct Tangent {
  DBuf<double> base, dx, scal;            // data terms of the right-hand side; [dx; 0]; residual ratio
  DBuf<int32_t> asp, csp, gsp;            // list starts: A per row, A per column, H per endpoint
  DBuf<int2> ae, ce, ge;                  // (entry, column), (entry, row), (entry, other endpoint)
  bool lists = false;
  DBuf<double> dir[7], out[5];            // host route: c, Hvals, Avals, lcon, ucon, lvar, uvar; x, y, zl, zu, cons
  int64_t n_tangents = 0;
};

// The polish (madipm_solver_polish*) shares the adjoint's residual rows, rowslack and events (and
// overwrites its factor: sens_factor and polish() clear each other's tag).  Its own, allocated by the first
// call: the scratch point [v; y], the gradient of the Lagrangian on [x; s], the raw bounds of [x; s] in the
// public space, the partial measures and the row values (8 B x (4 n + 2 m)); the codes of this call and of the
// factor held (2 n B); the slack -> row map (4 B per slack); the host route's staging of the set and the
// outputs.
struct PolMeasures {  // k_pol_verdict's result, read back with one copy
  int32_t verdict, n_active;
  double residual, min_multiplier, min_gap;
};
struct Polish {
  DBuf<double> w, grad, lo, hi, part, ax;
  DBuf<int8_t> codes, codes_fact, in_var, in_row, out_var, out_row;
  DBuf<int32_t> ineq, flags;              // flags: [a bad code was supplied, the codes differ from the factor's]
  DBuf<PolMeasures> meas;
  DBuf<double> out[5];                    // host route: x, y, zl, zu, cons
  int64_t bounds_updates = -1;            // n_updates_ of the bounds in lo / hi
  int64_t fact_solve = -1;                // n_solves_ of the point the LDL^T holds the polish factor of
  double fact_sigma = 0.0;
  madipm_polish_info last{-1, 0, 0.0, 0.0, 0.0, 0, 0};
};

namespace {

constexpr int NT = 256;
constexpr int NPART = 16;
constexpr int MAXB = 2048;  // partial-reduction blocks (part_ holds NPART x MAXB, value-major)
// partial k of block b: value-major so k_final's loads of one value are coalesced
__device__ __forceinline__ int pidx(int b, int k) { return k * MAXB + b; }
constexpr double INF = std::numeric_limits<double>::infinity();

struct DCsr {
  const int64_t* rp;
  const int32_t* ci;
  const double* v;
};

struct DV {
  int n, m, nx, nlb, nub;
  double *x, *xl, *xu, *zl, *zu, *f, *jacl, *c, *y, *rhs;
  double *pr_diag, *l_diag, *u_diag, *l_lower, *u_lower;
  double *d, *p, *corr_lb, *corr_ub;
  double* Kx;
  const int64_t* diag_pos;
  const double *Hdiag, *cs, *gfix, *cfix;
  const int32_t *ind_lb, *ind_ub, *lbpos, *ubpos;
  const uint8_t* fixed;
  DCsr H, J, JT;
  double* part;
  DevState* st;
  // KKT formulation (madipm_options.kkt_system): K2 / K2.5 (scaled) / normal equations
  int kkt;
  double* sk;               // K2.5: primal scaling s_i = sqrt(dist_l * dist_u)
  const int32_t *Krow, *Kcol;
  const double* K0;         // K2.5: unscaled K2 values (off-diagonal entries are constant)
  int64_t nnzK;
  double* Dinv;             // normal: 1 ./ pr_diag
  double* bufm;             // normal: right-hand side / solution of the m x m system
  const int64_t* cpp;       // normal: C entry e = sum over products [cpp[e], cpp[e+1])
  const int2* cprod;        //   product = (position of A_ik, position of A_jk) in J's values
  double* Cx;               //   values of C = A Sigma^{-1} A^T (lower CSC)
  int64_t nnzC;
};

enum { OP_SUM = 0, OP_MAX = 1, OP_MIN = 2 };

__device__ __forceinline__ double nmax(double a, double b) { return ((b > a) | (b != b)) ? b : a; }
__device__ __forceinline__ double comb(double a, double b, int op) {
  return op == OP_SUM ? a + b : (op == OP_MAX ? nmax(a, b) : fmin(a, b));
}
__device__ __forceinline__ double csr_dot(const DCsr& A, int row, const double* __restrict__ x) {
  double s = 0.0;
  for (int64_t q = A.rp[row]; q < A.rp[row + 1]; ++q) s += A.v[q] * x[A.ci[q]];
  return s;
}

// Wave reductions with the pairing of the `for (o = 32; o; o >>= 1) a = op(a, __shfl_down(a, o))` tree
// (lane i combines lane i + o; lane 0 ends with the same value bit for bit), without the LDS crossbar:
// o = 32 / 16 by the gfx950 half-row swaps (v_permlane32_swap / v_permlane16_swap: the swapped-in half
// is lane i + o for the lanes the tree reads), o = 8, 4, 2, 1 by DPP row_shl:o inside each 16-lane row.
// (ds_bpermute costs an LDS round trip per step: k_final's level-1 tree took ~2 us, MADIPM_FINAL_DEBUG.)
template <int O>
__device__ __forceinline__ int lane_down_i32(int v) {
  if constexpr (O == 32) {
    const auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (int)p[1];
  } else if constexpr (O == 16) {
    const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (int)p[1];
  } else {
    return __builtin_amdgcn_update_dpp(v, v, 0x100 + O, 0xf, 0xf, false);  // row_shl:O
  }
}
template <int O>
__device__ __forceinline__ double lane_down(double v) {
  return __hiloint2double(lane_down_i32<O>(__double2hiint(v)), lane_down_i32<O>(__double2loint(v)));
}
template <int OP>
__device__ __forceinline__ double wave_reduce(double a) {
  a = comb(a, lane_down<32>(a), OP);
  a = comb(a, lane_down<16>(a), OP);
  a = comb(a, lane_down<8>(a), OP);
  a = comb(a, lane_down<4>(a), OP);
  a = comb(a, lane_down<2>(a), OP);
  return comb(a, lane_down<1>(a), OP);
}
template <int O>
__device__ __forceinline__ void argmin_step(double& a, int& b);
__device__ __forceinline__ double wave_reduce_op(double a, int op) {
  return op == OP_SUM ? wave_reduce<OP_SUM>(a) : (op == OP_MAX ? wave_reduce<OP_MAX>(a) : wave_reduce<OP_MIN>(a));
}

template <int NV>
__device__ void block_partials(double (&v)[NV], const int (&ops)[NV], double* part, int base = 0, int bid = -1) {
  __shared__ double sh[NV][NT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double a = wave_reduce_op(v[k], ops[k]);
    if (lane == 0) sh[k][wv] = a;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int k = threadIdx.x;
    double a = sh[k][0];
    for (int w = 1; w < NT / 64; ++w) a = comb(a, sh[k][w], ops[k]);
    part[pidx(bid >= 0 ? bid : (int)blockIdx.x, base + k)] = a;
  }
}

// (value, index) argmin in the order of the reference's left fold (kernels.jl:226-272:
// mapreduce(...; init = (1.0, 0)) with `elem1[1] < elem2[1] ? elem1 : elem2`): a later element
// replaces the accumulator unless the accumulator is strictly smaller, so among equal ratios the
// LAST index wins.  As a total order, (value ascending, index descending): associative, so any
// combine tree gives the fold's answer.  The init element is index -1 (below every real index).
__device__ __forceinline__ void amin_upd(double& v, int& ix, double nv, int ni) {
  const bool take = (nv < v) | ((nv == v) & (ni > ix));  // no short circuit: selects, not branches
  v = take ? nv : v;
  ix = take ? ni : ix;
}

template <int O>
__device__ __forceinline__ void argmin_step(double& a, int& b) {
  const double a2 = lane_down<O>(a);
  const int b2 = lane_down_i32<O>(b);
  amin_upd(a, b, a2, b2);
}
__device__ __forceinline__ void wave_argmin(double& a, int& b) {
  argmin_step<32>(a, b);
  argmin_step<16>(a, b);
  argmin_step<8>(a, b);
  argmin_step<4>(a, b);
  argmin_step<2>(a, b);
  argmin_step<1>(a, b);
}

#define GRID_LOOP(i, N) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (N); i += (int64_t)gridDim.x * blockDim.x)

// SpMV rows in groups of G lanes (G | 64): the group's lanes stride the row's entries (coalesced),
// then a G-wide butterfly sums them (every lane of the group holds the row sum).  G is chosen per
// problem from the mean row length (MPCSolver::spmv_group).
#define GROUP_LOOP(i, N, G) \
  for (int64_t i = (blockIdx.x * (int64_t)NT + threadIdx.x) / (G); i < (N); i += (int64_t)gridDim.x * (NT / (G)))
// the same loops over a sub-grid of nblk blocks (block bid of it): kernels whose blocks split into roles
#define GROUP_LOOP_B(i, N, G, bid, nblk) \
  for (int64_t i = ((bid) * (int64_t)NT + threadIdx.x) / (G); i < (N); i += (int64_t)(nblk) * (NT / (G)))
#define GRID_LOOP_B(i, N, bid, nblk) \
  for (int64_t i = (bid) * (int64_t)blockDim.x + threadIdx.x; i < (N); i += (int64_t)(nblk) * blockDim.x)

template <int G>
__device__ __forceinline__ double gdot(const DCsr& A, int64_t row, const double* __restrict__ x) {
  const int gl = threadIdx.x & (G - 1);
  double s = 0.0;
  const int64_t q1 = A.rp[row + 1];
  // two entries per lane and trip, both issued before either is summed (clamped index, the second
  // masked): the gathers of consecutive trips no longer wait for each other; same summation order
  for (int64_t q = A.rp[row] + gl; q < q1; q += 2 * G) {
    const int64_t qb = min(q + G, q1 - 1);
    const double va = A.v[q], vb = A.v[qb];
    const double xa = x[A.ci[q]], xb = x[A.ci[qb]];
    s = fma(va, xa, s);
    s = fma((q + G < q1) ? vb : 0.0, xb, s);
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, G);
  return s;
}

// gdot<G>(A, ra, xa) and gdot<G>(B, rb, xb) at once (a primal row's H and J^T parts): both rows'
// extents, then each trip's entries and gathers of both, issued before either is summed — one chain
// of dependent loads instead of two back to back.  Each sum in gdot's own order (same bits).
template <int G>
__device__ __forceinline__ void gdot2(const DCsr& A, int64_t ra, const double* __restrict__ xa, const DCsr& B,
                                      int64_t rb, const double* __restrict__ xb, double& sa, double& sb) {
  const int gl = threadIdx.x & (G - 1);
  const int64_t a1 = A.rp[ra + 1], b1 = B.rp[rb + 1];
  int64_t qa = A.rp[ra] + gl, qb = B.rp[rb] + gl;
  sa = 0.0;
  sb = 0.0;
  while (qa < a1 || qb < b1) {
    const bool ta = qa < a1, tb = qb < b1;
    double va = 0.0, va2 = 0.0, ya = 0.0, ya2 = 0.0, vb = 0.0, vb2 = 0.0, yb = 0.0, yb2 = 0.0;
    if (ta) {
      const int64_t q2 = min(qa + G, a1 - 1);
      va = A.v[qa];
      va2 = A.v[q2];
      ya = xa[A.ci[qa]];
      ya2 = xa[A.ci[q2]];
    }
    if (tb) {
      const int64_t q2 = min(qb + G, b1 - 1);
      vb = B.v[qb];
      vb2 = B.v[q2];
      yb = xb[B.ci[qb]];
      yb2 = xb[B.ci[q2]];
    }
    if (ta) {
      sa = fma(va, ya, sa);
      sa = fma((qa + G < a1) ? va2 : 0.0, ya2, sa);
      qa += 2 * G;
    }
    if (tb) {
      sb = fma(vb, yb, sb);
      sb = fma((qb + G < b1) ? vb2 : 0.0, yb2, sb);
      qb += 2 * G;
    }
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    sa += __shfl_xor(sa, o, G);
    sb += __shfl_xor(sb, o, G);
  }
}

// ------------------------------------------------------------------ KKT diagonal (kernels.jl:124-149)
// K2 (set_aug_diagonal! for SparseKKTSystem, kernels.jl:124-136): pr_diag into the K2 diagonal.
// K2.5 (kernels.jl:139-149 + MadNLP._set_aug_diagonal! [EXT]): the primal block is scaled
// symmetrically by S = diag(s), s_i = sqrt((x - xl)(xu - x)) (a missing bound contributes 1), so the
// diagonal is s^2 (dw + H_ii) + zl (xu - x) + zu (x - xl) — bounded as x approaches a bound.
// Normal equations (NormalKKTSystem.build_kkt!, normalkkt.jl:180-194): Dinv = 1 ./ pr_diag.
// l_diag / u_diag keep the K2 sign convention (xl - x, x - xu) in every mode: they feed the
// unreduced operator of the residual, which is the same for the three formulations.
__device__ __forceinline__ void diag_entry(const DV& D, int64_t i, double dw, double dc) {
  if (i < D.n) {
    double pr = dw;
    const int kl = D.lbpos[i], ku = D.ubpos[i];
    const double x = D.x[i];
    double dl = 1.0, du = 1.0, zlv = 0.0, zuv = 0.0;
    if (kl >= 0) {
      const double ld = D.xl[i] - x, zl = D.zl[i];
      D.l_diag[kl] = ld;
      D.l_lower[kl] = zl;
      pr -= zl / ld;
      dl = -ld;
      zlv = zl;
    }
    if (ku >= 0) {
      const double ud = x - D.xu[i], zu = D.zu[i];
      D.u_diag[ku] = ud;
      D.u_lower[ku] = zu;
      pr -= zu / ud;
      du = -ud;
      zuv = zu;
    }
    D.pr_diag[i] = pr;
    if (D.kkt == KKT_NORMAL) {
      D.Dinv[i] = 1.0 / pr;
    } else if (D.kkt == KKT_K25) {
      const double s2 = dl * du;
      D.sk[i] = sqrt(s2);
      D.Kx[D.diag_pos[i]] = s2 * (dw + D.Hdiag[i]) + zlv * du + zuv * dl;
    } else {
      D.Kx[D.diag_pos[i]] = pr + D.Hdiag[i];
    }
  } else if (D.kkt != KKT_NORMAL) {
    D.Kx[D.diag_pos[i]] = dc;
  }
}

// rs != nullptr: the factorisation that follows starts here (LinSolver::ext_reset)
__global__ __launch_bounds__(NT) void k_diag(DV D, double dw, double dc, LDLStatus* rs) {
  if (rs && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_start(rs);
  GRID_LOOP(i, D.n + D.m) diag_entry(D, i, dw, dc);
}

// MadNLP.initialize!(kkt) + init_starting_point! lines 16-18 (l_diag = u_diag = 1, l/u_lower = 0,
// pr_diag = dw; K2.5 scaling factor 1)
__global__ __launch_bounds__(NT) void k_init_kkt(DV D, double dw, double dc, LDLStatus* rs) {
  if (rs && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_start(rs);
  GRID_LOOP(i, D.n + D.m) {
    if (i < D.n) {
      const int kl = D.lbpos[i], ku = D.ubpos[i];
      if (kl >= 0) {
        D.l_diag[kl] = 1.0;
        D.l_lower[kl] = 0.0;
      }
      if (ku >= 0) {
        D.u_diag[ku] = 1.0;
        D.u_lower[ku] = 0.0;
      }
      D.pr_diag[i] = dw;
      if (D.kkt == KKT_NORMAL) {
        D.Dinv[i] = 1.0 / dw;
      } else {
        if (D.kkt == KKT_K25) D.sk[i] = 1.0;
        D.Kx[D.diag_pos[i]] = dw + D.Hdiag[i];
      }
    } else if (D.kkt != KKT_NORMAL) {
      D.Kx[D.diag_pos[i]] = dc;
    }
  }
}

// K2.5: off-diagonal entries K[e] = s_row s_col K0[e] (s = 1 on the dual block)
__global__ __launch_bounds__(NT) void k_k25_scale(DV D) {
  GRID_LOOP(e, D.nnzK) {
    const int r = D.Krow[e], c = D.Kcol[e];
    if (r == c) continue;
    const double sr = r < D.n ? D.sk[r] : 1.0, sc = c < D.n ? D.sk[c] : 1.0;
    D.Kx[e] = sr * sc * D.K0[e];
  }
}

// K2.5: dx = S (S^{-1} dx) after the scaled solve
__global__ __launch_bounds__(NT) void k_k25_unscale(DV D) {
  GRID_LOOP(i, D.n) D.d[i] *= D.sk[i];
}

// NormalKKTSystem.build_kkt! / assemble_normal_system! (normalkkt.jl:180-194, utils.jl:276-308):
// C_ij = sum_k A_ik Sigma_k^{-1} A_jk over the precomputed product list of entry (i, j) — one
// thread per entry of tril(C), fixed summation order, no atomics.
__global__ __launch_bounds__(NT) void k_normal_asm(DV D) {
  GRID_LOOP(e, D.nnzC) {
    double v = 0.0;
    const int64_t p1 = D.cpp[e + 1];
    for (int64_t p = D.cpp[e]; p < p1; ++p) {
      const int2 ab = D.cprod[p];
      v += D.J.v[ab.x] * D.Dinv[D.J.ci[ab.x]] * D.J.v[ab.y];
    }
    D.Cx[e] = v;
  }
}

// MadNLP.solve!(kkt::NormalKKTSystem, w) (normalkkt.jl:196-219), after reduce_rhs! (done by k_rhs):
// r2 = A Sigma^{-1} r1 - r2 (one thread per row of A)
template <int G>
__global__ __launch_bounds__(NT) void k_normal_rhs(DV D) {
  GROUP_LOOP(i, D.m, G) {
    const int gl = threadIdx.x & (G - 1);
    double s = 0.0;
    for (int64_t q = D.J.rp[i] + gl; q < D.J.rp[i + 1]; q += G) {
      const int k = D.J.ci[q];
      s += D.J.v[q] * (D.d[k] / D.pr_diag[k]);
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, G);
    if (gl == 0) D.bufm[i] = s - D.d[D.n + i];
  }
}

// ... dy = C^{-1} r2 (LDL^T solve on bufm), then dx = Sigma^{-1} (r1 - A^T dy), wy = dy
template <int G>
__global__ __launch_bounds__(NT) void k_normal_back(DV D) {
  GROUP_LOOP(i, D.n + D.m, G) {
    if (i < D.n) {
      const double s = gdot<G>(D.JT, i, D.bufm);
      if ((threadIdx.x & (G - 1)) == 0) D.d[i] = (D.d[i] - s) / D.pr_diag[i];
    } else if ((threadIdx.x & (G - 1)) == 0) {
      D.d[i] = D.bufm[i - D.n];
    }
  }
}

enum { RHS_INIT_PRIMAL = 0, RHS_INIT_DUAL = 1, RHS_PRED = 2, RHS_CORR = 3, RHS_GONDZIO = 4 };

// set_*_rhs! (kernels.jl:1-58) fused with reduce_rhs! [EXT]: writes the unreduced p and the
// reduced right-hand side d[0:n+m] handed to the LDL^T solve.
// reset: 1 = start of an iteration's directions (max_res_ratio), 2 = also clear the NaN flag (redo)
// publish the device state to the host mirror: payload with system-scope stores, drained and
// released, then the counter (the host spins on the counter, MPCSolver::wait_state)
static_assert(sizeof(DevState) % 8 == 0 && sizeof(DevState) <= 64 * 8, "k_publish: one word per lane");
__device__ __forceinline__ void publish_state(const DevState* __restrict__ st, DevState* host, uint32_t* hseq,
                                              uint32_t seq, bool fresh = false) {  // called by one whole wave
  // fresh: the state was just stored by lane 0 of this wave: read it back from L2 (agent-scope loads)
  const int i = threadIdx.x;
  if (i < (int)(sizeof(DevState) / 8)) {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(st) + i;
    const uint64_t v = fresh ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *src;
    __hip_atomic_store(reinterpret_cast<uint64_t*>(host) + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (i == 0) __hip_atomic_store(hseq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// FIN_MU_PRED folded into the corrector's k_rhs: every block reduces k_mu's nb partials (slots 0..3)
// in the same fixed order, so all blocks agree on mu bit for bit; block 0 records it in the state
struct MuFold {
  int nb;                         // 0: mu from the state (FIN_MU_PRED ran)
  double cnt, has_ineq, mu_min;   // nlb + nub, has_inequalities, mu_min (FIN_MU_PRED's parameters)
};

// host != nullptr: wave 0 of block 0 first publishes the state (k_publish's work: the speculated
// predictor's k_rhs is the first launch after the factorisation, one launch less per iteration)
// t1 != nullptr: the factorisation before this launch ended (LinSolver::lazy_inertia)
__global__ __launch_bounds__(NT) void k_rhs(DV D, int mode, double mu_g, int reset, DevState* host, uint32_t* hseq,
                                            uint32_t seq, MuFold mf, LDLStatus* t1) {
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
  const int n = D.n, m = D.m, nlb = D.nlb;
  double mu = (mode == RHS_CORR) ? D.st->mu : mu_g;
  if (mf.nb > 0) {  // prediction_step! + update_barrier! (kernels.jl:176-220), as k_final(FIN_MU_PRED)
    __shared__ double shm[4][NT / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < mf.nb; b += NT)
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += D.part[pidx(b, k)];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] = wave_reduce<OP_SUM>(a[k]);
      if (lane == 0) shm[k][wv] = a[k];
    }
    __syncthreads();
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r[k] = shm[k][0];
      for (int w = 1; w < NT / 64; ++w) r[k] += shm[k][w];
    }
    const double mu_aff = mf.cnt == 0 ? 0.0 : (r[2] + r[3]) / mf.cnt;
    const double mu_curr = mf.cnt == 0 ? 0.0 : (r[0] + r[1]) / mf.cnt;
    double sigma = 1.0;
    if (mf.has_ineq != 0.0) {
      const double q = mu_aff / mu_curr;
      sigma = fmin(fmax(q * q * q, 1e-6), 10.0);
    }
    mu = fmax(mf.mu_min, sigma * mu_curr);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      D.st->mu_aff = mu_aff;
      D.st->mu_curr = mu_curr;
      D.st->mu = mu;
    }
  }
  if (host && blockIdx.x == 0 && threadIdx.x < 64) publish_state(D.st, host, hseq, seq);
  if (reset && blockIdx.x == 0 && threadIdx.x == 0) {
    D.st->max_res_ratio = 0.0;
    if (reset == 2) D.st->nan_flag = 0;
  }
  // every operand of the row loaded first and unconditionally (clamped indices; the bound blocks'
  // entries right after the bound positions), the mode / bound tests applied afterwards: behind
  // `if (kl >= 0)` the loads were dependent round trips of their own
  const int nub = D.nub;
  GRID_LOOP(i, n + m) {
    if (i < n) {
      const int kl = D.lbpos[i], ku = D.ubpos[i];
      const double f = D.f[i], zl = D.zl[i], zu = D.zu[i], jl = D.jacl[i];
      const double x = D.x[i], xl = D.xl[i], xu = D.xu[i], di = D.d[i];
      const int kl0 = kl >= 0 ? kl : 0, ku0 = ku >= 0 ? ku : 0;
      const double ldg = D.l_diag[kl0], udg = D.u_diag[ku0], clb = D.corr_lb[kl0], cub = D.corr_ub[ku0];
      const double dzl = D.d[nlb > 0 ? n + m + kl0 : 0], dzu = D.d[nub > 0 ? n + m + nlb + ku0 : 0];
      double px;
      if (mode == RHS_INIT_PRIMAL)
        px = 0.0;
      else if (mode == RHS_INIT_DUAL)
        px = -f;
      else
        px = -f + zl - zu - jl;
      double dr = px;
      const bool full = mode >= RHS_PRED;
      if (kl >= 0) {
        double pz = 0.0;
        if (full) {
          pz = (xl - x) * zl;
          if (mode == RHS_CORR) {
            const double corr = di * dzl;
            D.corr_lb[kl] = corr;
            pz = pz + mu - corr;
          } else if (mode == RHS_GONDZIO) {
            pz = pz + mu - clb;
          }
        }
        D.p[n + m + kl] = pz;
        dr -= pz / ldg;
      }
      if (ku >= 0) {
        double pz = 0.0;
        if (full) {
          pz = (xu - x) * zu;
          if (mode == RHS_CORR) {
            const double corr = di * dzu;
            D.corr_ub[ku] = corr;
            pz = pz - mu - corr;
          } else if (mode == RHS_GONDZIO) {
            pz = pz - mu - cub;
          }
        }
        D.p[n + m + nlb + ku] = pz;
        dr -= pz / udg;
      }
      D.p[i] = px;
      D.d[i] = (D.kkt == KKT_K25) ? dr * D.sk[i] : dr;  // K2.5: right-hand side S r1
    } else {
      const double py = (mode == RHS_INIT_DUAL) ? 0.0 : -D.c[i - n];
      D.p[i] = py;
      D.d[i] = py;
    }
  }
}

// finish_aug_solve! [EXT] + residual w = p - K d (mul!/_kktmul! [EXT], linear_solver.jl:29-35)
enum { ALPHA_PRED = 0, ALPHA_CONSERVATIVE = 1, ALPHA_ADAPTIVE = 2, ALPHA_MEHROTRA = 3, ALPHA_GONDZIO = 4 };
// k_alpha may write its partials from slot PART_ALPHA (4 values, 4 indices) so that the residual's
// finaliser finalises both (one k_final less per direction).  Measured and reverted: the step test
// inside k_residual itself — its division-heavy tail then runs on one lane per SpMV lane group
// (k_residual 20.9 -> 32.2 us per launch, more than the two launches it saved).
constexpr int PART_ALPHA = 8;

__device__ __forceinline__ double alpha_tau(const DV& D, int mode, double tau_param) {
  double tau = 1.0;
  if (mode == ALPHA_CONSERVATIVE || mode == ALPHA_GONDZIO) tau = tau_param;
  if (mode == ALPHA_ADAPTIVE) tau = fmax(1.0 - D.st->mu, tau_param);
  return tau;
}

// block argmin of (v[k], ix[k]), k < 4, into part slots base + k (values) and base + 4 + k (indices)
__device__ void block_argmin4(const double (&v)[4], const int (&ix)[4], double* part, int base, int bid) {
  __shared__ double sv[4][NT / 64];
  __shared__ int si[4][NT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double a = v[k];
    int b = ix[k];
    wave_argmin(a, b);
    if (lane == 0) {
      sv[k][wv] = a;
      si[k][wv] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    double a = sv[k][0];
    int b = si[k][0];
    for (int w = 1; w < NT / 64; ++w) amin_upd(a, b, sv[k][w], si[k][w]);
    part[pidx(bid, base + k)] = a;
    part[pidx(bid, base + 4 + k)] = (double)b;
  }
}

template <bool FROM_P>
__device__ void alpha_body(const DV& D, int mode, double tau_param, int base, int bid, int nblk);

// nres < gridDim.x: blocks [nres, gridDim.x) run the step test of mode amode (alpha_body, partials
// from slot PART_ALPHA) beside the nres residual blocks — one launch for both
template <int G>
__global__ __launch_bounds__(NT) void k_residual(DV D, double dw, double dc, int nres, int amode, double atau) {
  const int n = D.n, m = D.m, nlb = D.nlb;
  if ((int)blockIdx.x >= nres) {
    alpha_body<true>(D, amode, atau, PART_ALPHA, (int)blockIdx.x - nres, (int)gridDim.x - nres);
    return;
  }
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  double wmax = 0.0, pmax = 0.0, dxmax = 0.0;
  GROUP_LOOP_B(i, n + m, G, (int)blockIdx.x, nres) {
    // the row's own entries and its bound blocks do not depend on the dot products: loaded first,
    // unconditionally (clamped indices; every lane of the group, one cache line), so their latency
    // overlaps the gathers — behind `if (!lead)` / `if (kl >= 0)` they were two more round trips
    const double dxi = D.d[i], pi = D.p[i];
    const int kl = (i < n) ? D.lbpos[i] : -1, ku = (i < n) ? D.ubpos[i] : -1;
    const int kl0 = kl >= 0 ? kl : 0, ku0 = ku >= 0 ? ku : 0;
    const double pl = D.p[kl >= 0 ? n + m + kl : i], llo = D.l_lower[kl0], ldi = D.l_diag[kl0];
    const double pu = D.p[ku >= 0 ? n + m + nlb + ku : i], ulo = D.u_lower[ku0], udi = D.u_diag[ku0];
    if (i < n) {
      double hd, jd;
      gdot2<G>(D.H, i, D.d, D.JT, i, D.d + n, hd, jd);
      const double hj = hd + jd;
      if (!lead) continue;
      const double dx = dxi;
      double kv = hj + dw * dx;
      if (kl >= 0) {
        const double dzl = (-pl + llo * dx) / ldi;
        D.d[n + m + kl] = dzl;
        kv -= dzl;
        const double wl = pl - (dx * llo - dzl * ldi);
        wmax = nmax(wmax, fabs(wl));
        pmax = nmax(pmax, fabs(pl));
      }
      if (ku >= 0) {
        const double dzu = (pu - ulo * dx) / udi;
        D.d[n + m + nlb + ku] = dzu;
        kv += dzu;
        const double wu = pu - (dx * ulo + dzu * udi);
        wmax = nmax(wmax, fabs(wu));
        pmax = nmax(pmax, fabs(pu));
      }
      wmax = nmax(wmax, fabs(pi - kv));
      pmax = nmax(pmax, fabs(pi));
      dxmax = nmax(dxmax, fabs(dx));
    } else {
      const double jd = gdot<G>(D.J, i - n, D.d);
      if (!lead) continue;
      const double kv = jd + dc * dxi;
      wmax = nmax(wmax, fabs(pi - kv));
      pmax = nmax(pmax, fabs(pi));
    }
  }
  double v[3] = {wmax, pmax, dxmax};
  const int ops[3] = {OP_MAX, OP_MAX, OP_MAX};
  block_partials<3>(v, ops, D.part, 0, (int)blockIdx.x);
}

// get_alpha_max_primal / get_alpha_max_dual (kernels.jl:226-272): min-ratio with argmin
// from_p: dz formed here from the reduced rhs p and dx, exactly as k_residual's finish_aug_solve
// forms it (the step-test blocks of a k_residual launch run beside the residual blocks that store it).
// The reduced-rhs operands (p, l_lower, l_diag, u_lower, u_diag) exist only in the FROM_P instance:
// madipm_update_step's standalone DV leaves them null.
template <bool FROM_P>
__device__ void alpha_body(const DV& D, int mode, double tau_param, int base, int bid, int nblk) {
  constexpr bool from_p = FROM_P;
  const int n = D.n, m = D.m, nlb = D.nlb, nub = D.nub;
  const double tau = alpha_tau(D, mode, tau_param);
  double v[4] = {INF, INF, INF, INF};
  int ix[4] = {-1, -1, -1, -1};
  // every operand loaded unconditionally (clamped indices) right after the bound's index, the tests
  // applied as selects: behind `if (dx < 0)` etc. the loads were dependent round trips of their own
  GRID_LOOP_B(t, (nlb > nub ? nlb : nub), bid, nblk) {
    const int tl = t < nlb ? (int)t : 0, tu = t < nub ? (int)t : 0;
    const int il = nlb > 0 ? D.ind_lb[tl] : 0, iu = nub > 0 ? D.ind_ub[tu] : 0;
    const double dxl = D.d[il], xl_x = D.x[il], xl_l = D.xl[il], zl = D.zl[il];
    const double pl = from_p ? D.p[nlb > 0 ? n + m + tl : 0] : D.d[nlb > 0 ? n + m + tl : 0];
    const double lo = from_p ? D.l_lower[tl] : 0.0, ldg = from_p ? D.l_diag[tl] : 1.0;
    const double dxu = D.d[iu], xu_x = D.x[iu], xu_u = D.xu[iu], zu = D.zu[iu];
    const int qu = nub > 0 ? n + m + nlb + tu : 0;  // in range
    const double pu = from_p ? D.p[qu] : D.d[qu];
    const double uo = from_p ? D.u_lower[tu] : 0.0, udg = from_p ? D.u_diag[tu] : 1.0;
    if (t < nlb) {
      const double dx = dxl;
      if (dx < 0) amin_upd(v[0], ix[0], (-xl_x + xl_l) * tau / dx, (int)t);
      const double dz = from_p ? (-pl + lo * dx) / ldg : pl;
      if (dz < 0) amin_upd(v[2], ix[2], (-zl) * tau / dz, (int)t);
    }
    if (t < nub) {
      const double dx = dxu;
      if (dx > 0) amin_upd(v[1], ix[1], (-xu_x + xu_u) * tau / dx, (int)t);
      const double dz = from_p ? (pu - uo * dx) / udg : pu;
      if (dz < 0 && zu + dz < 0) amin_upd(v[3], ix[3], (-zu) * tau / dz, (int)t);
    }
  }
  block_argmin4(v, ix, D.part, base, bid);
}

__global__ __launch_bounds__(NT) void k_alpha(DV D, int mode, double tau_param, int base) {
  alpha_body<false>(D, mode, tau_param, base, blockIdx.x, gridDim.x);
}

enum { MU_PRED = 0, MU_FULL = 1, MU_GONDZIO = 2 };

// complementarity sums (kernels.jl:155-208); step lengths from the device state (use_state) or args
__global__ __launch_bounds__(NT) void k_mu(DV D, int use_state, double ap_arg, double ad_arg) {
  const int n = D.n, m = D.m, nlb = D.nlb, nub = D.nub;
  const double ap = use_state ? D.st->alpha_aff_p : ap_arg;
  const double ad = use_state ? D.st->alpha_aff_d : ad_arg;
  double cl = 0, cu = 0, al = 0, au = 0;
  GRID_LOOP(t, (nlb > nub ? nlb : nub)) {
    if (t < nlb) {
      const int i = D.ind_lb[t];
      const double x = D.x[i], xl = D.xl[i], zl = D.zl[i];
      cl += (x - xl) * zl;
      al += ((x + ap * D.d[i]) - xl) * (zl + ad * D.d[n + m + t]);
    }
    if (t < nub) {
      const int i = D.ind_ub[t];
      const double x = D.x[i], xu = D.xu[i], zu = D.zu[i];
      cu += (xu - x) * zu;
      au += (xu - (x + ap * D.d[i])) * (zu + ad * D.d[n + m + nlb + t]);
    }
  }
  double v[4] = {cl, cu, al, au};
  const int ops[4] = {OP_SUM, OP_SUM, OP_SUM, OP_SUM};
  block_partials<4>(v, ops, D.part);
}

// apply_step! + adjust_boundary! [EXT] (solver.jl:308-317)
__global__ __launch_bounds__(NT) void k_apply(DV D) {
  if (D.st->nan_flag) return;  // SolveException raised in this iteration's directions: no step
  const int n = D.n, m = D.m, nlb = D.nlb;
  const double ap = D.st->alpha_p, ad = D.st->alpha_d, mu = D.st->mu;
  const double eps = 2.220446049250313e-16;
  const double c1 = eps * mu, c2 = 1.8189894035458617e-12;  // eps^(3/4)
  GRID_LOOP(i, n + m) {
    if (i < n) {
      const double x = D.x[i] + ap * D.d[i];
      D.x[i] = x;
      const int kl = D.lbpos[i], ku = D.ubpos[i];
      if (kl >= 0) {
        D.zl[i] += ad * D.d[n + m + kl];
        const double xl = D.xl[i];
        if (x - xl < c1) D.xl[i] = xl - c2 * fmax(1.0, fabs(x));
      }
      if (ku >= 0) {
        D.zu[i] += ad * D.d[n + m + nlb + ku];
        const double xu = D.xu[i];
        if (xu - x < c1) D.xu[i] = xu + c2 * fmax(1.0, fabs(x));
      }
    } else {
      D.y[i - n] += ad * D.d[i];
    }
  }
}

// evaluate_model! (solver.jl:319-326): obj, grad f = Hx + c, cons c = Jx - rhs, jacl = J^T y
template <int G>
__global__ __launch_bounds__(NT) void k_eval(DV D, int slot) {
  const int n = D.n;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  double op = 0.0;
  GROUP_LOOP(i, n + D.m, G) {
    if (i < n) {
      double hx, jy;
      gdot2<G>(D.H, i, D.x, D.JT, i, D.y, hx, jy);
      if (!lead) continue;
      const double x = D.x[i];
      const double g = D.cs[i] + D.gfix[i];
      D.f[i] = D.fixed[i] ? 0.0 : hx + g;
      D.jacl[i] = jy;
      op += x * g + 0.5 * x * hx;
    } else {
      const int64_t j = i - n;
      const double jx = gdot<G>(D.J, j, D.x);
      if (lead) D.c[j] = jx - D.rhs[j] + D.cfix[j];
    }
  }
  double v[1] = {op};
  const int ops[1] = {OP_SUM};
  block_partials<1>(v, ops, D.part, slot);
}

// jtprod!(jacl, kkt, y)
__global__ __launch_bounds__(NT) void k_jtprod(DV D) {
  GRID_LOOP(i, D.n) D.jacl[i] = csr_dot(D.JT, (int)i, D.y);
}

// update_termination_criteria! pieces (solver.jl:194-204; dual_objective kernels.jl:408-417;
// get_optimality_gap kernels.jl:419-430; get_inf_pr/get_inf_du [EXT])
// diag != 0: also k_diag's work for the next factorisation (same grid, same iterate reads; the
// regularisation is decided on the host before this launch), one launch less per iteration
__global__ __launch_bounds__(NT) void k_term(DV D, int diag, double dw, double dc) {
  const int n = D.n;
  double du = 0, gap = 0, pr = 0, sy = 0, sl = 0, su = 0;
  GRID_LOOP(i, n + D.m) {
    if (diag) diag_entry(D, i, dw, dc);
    if (i < n) {
      du = nmax(du, fabs(D.f[i] - D.zl[i] + D.zu[i] + D.jacl[i]));
      const int kl = D.lbpos[i], ku = D.ubpos[i];
      if (kl >= 0) {
        gap = nmax(gap, fabs((D.x[i] - D.xl[i]) * D.zl[i]));
        sl += D.zl[i] * D.xl[i];
      }
      if (ku >= 0) {
        gap = nmax(gap, fabs((D.xu[i] - D.x[i]) * D.zu[i]));
        su += D.zu[i] * D.xu[i];
      }
    } else {
      const int j = (int)(i - n);
      pr = nmax(pr, fabs(D.c[j]));
      sy += D.y[j] * D.rhs[j];
    }
  }
  double v[6] = {du, gap, pr, sy, sl, su};
  const int ops[6] = {OP_MAX, OP_MAX, OP_MAX, OP_SUM, OP_SUM, OP_SUM};
  block_partials<6>(v, ops, D.part);
}

// init_starting_point! Step 3 (solver.jl:37-78): z from r = A^T y + f, then min-reductions
__global__ __launch_bounds__(NT) void k_zinit(DV D) {
  const int n = D.n;
  double mxl = 0, mxu = 0, mzl = 0, mzu = 0;  // minimum(...; init=0.0)
  GRID_LOOP(i, n) {
    const double res = csr_dot(D.JT, (int)i, D.y) + D.f[i];
    const double l = D.xl[i], u = D.xu[i];
    const bool fl = isfinite(l), fu = isfinite(u);
    const double zl = (fl && fu) ? 0.5 * res : (fl ? res : D.zl[i]);
    const double zu = (fl && fu) ? -0.5 * res : (fu ? -res : D.zu[i]);
    D.zl[i] = zl;
    D.zu[i] = zu;
    const double x = D.x[i];
    if (D.lbpos[i] >= 0) {
      mxl = fmin(mxl, x - l);
      mzl = fmin(mzl, zl);
    }
    if (D.ubpos[i] >= 0) {
      mxu = fmin(mxu, u - x);
      mzu = fmin(mzu, zu);
    }
  }
  double v[4] = {mxl, mxu, mzl, mzu};
  const int ops[4] = {OP_MIN, OP_MIN, OP_MIN, OP_MIN};
  block_partials<4>(v, ops, D.part);
}

// solver.jl:80-99: first shift, then the sums defining mu, delta_x2, delta_s2
__global__ __launch_bounds__(NT) void k_zshift1(DV D) {
  const int n = D.n;
  const double dx = D.st->delta_x, ds = D.st->delta_s;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  GRID_LOOP(i, n) {
    const bool lb = D.lbpos[i] >= 0, ub = D.ubpos[i] >= 0;
    double x = D.x[i];
    if (lb) x = x + dx;
    if (ub) x = x - dx;
    D.x[i] = x;
    if (lb) {
      const double zl = D.zl[i] + 1.0 + ds;
      D.zl[i] = zl;
      const double l = D.xl[i];
      s[0] += x * zl;
      s[1] += l * zl;
      s[4] += zl;
      s[6] += x - l;
    }
    if (ub) {
      const double zu = D.zu[i] + 1.0 + ds;
      D.zu[i] = zu;
      const double u = D.xu[i];
      s[2] += u * zu;
      s[3] += x * zu;
      s[5] += zu;
      s[7] += u - x;
    }
  }
  const int ops[8] = {OP_SUM, OP_SUM, OP_SUM, OP_SUM, OP_SUM, OP_SUM, OP_SUM, OP_SUM};
  block_partials<8>(s, ops, D.part);
}

// solver.jl:96-123: second shift, Ipopt projection, interior assertions (violation count)
__global__ __launch_bounds__(NT) void k_zshift2(DV D, double kappa) {
  const int n = D.n;
  const double dx2 = D.st->delta_x2, ds2 = D.st->delta_s2;
  double viol = 0;
  GRID_LOOP(i, n) {
    const bool lb = D.lbpos[i] >= 0, ub = D.ubpos[i] >= 0;
    double x = D.x[i];
    if (lb) x = x + dx2;
    if (ub) x = x - dx2;
    if (lb) D.zl[i] = D.zl[i] + ds2;
    if (ub) D.zu[i] = D.zu[i] + ds2;
    const double l = D.xl[i], u = D.xu[i];
    if (x < l) {
      x = l + fmin(kappa * fmax(1.0, l), kappa * (u - l));
    } else if (u < x) {
      x = u - fmin(kappa * fmax(1.0, u), kappa * (u - l));
    }
    D.x[i] = x;
    if (lb && !(D.zl[i] > 0.0 && x > l)) viol += 1;
    if (ub && !(D.zu[i] > 0.0 && x < u)) viol += 1;
  }
  double v[1] = {viol};
  const int ops[1] = {OP_SUM};
  block_partials<1>(v, ops, D.part);
}

__global__ void k_set_mu(DevState* st, double mu) {
  st->mu = mu;
  st->alpha_p = st->alpha_d = 0.0;
  st->nan_flag = 0;
  st->max_res_ratio = 0.0;
  st->dx_inf = 0.0;
}

enum {
  FIN_RESID = 0,
  FIN_ALPHA = 1,
  FIN_MU_PRED = 2,
  FIN_MU_FULL = 3,
  FIN_EVAL = 4,
  FIN_TERM = 5,
  FIN_ZINIT = 6,
  FIN_ZSHIFT1 = 7,
  FIN_ZSHIFT2 = 8,
  FIN_MU_GONDZIO = 9
};

struct FinParams {
  int nb;          // number of partial blocks
  int alpha_mode;  // for FIN_ALPHA (and FIN_RESID with nb_alpha > 0)
  double a, b, c;  // kind-specific parameters
  int nb_alpha;    // FIN_RESID: > 0 -> also finalise k_alpha's nb_alpha partials (slots PART_ALPHA..)
  int nb_eval;     // FIN_TERM: > 0 -> also finalise evaluate_model!'s objective (k_eval's nb_eval
                   // partials in slot PART_EVAL, the previous iteration's; P.c = its constant)
  LDLStatus* rs;   // != nullptr: a factorisation follows this launch (LinSolver::ext_reset)
  int64_t* dbg = nullptr;  // diagnostics (MADIPM_FINAL_DEBUG): thread 0's wall clock at entry / reduced / end
  DevState* host = nullptr;  // != nullptr: wave 0 of the last workgroup publishes the state (sequence seq)
  uint32_t* hseq = nullptr;
  uint32_t seq = 0;
};
constexpr int PART_EVAL = 6;

// k_final combines the producers' block partials (nb <= MAXB per slot) in two levels inside ONE launch:
// FG workgroups of FT threads, thread t of workgroup g owning block g FT + t; each workgroup reduces its
// FT blocks (wave shuffles, then wave 0 before wave 1) and stores one partial per value write-through
// (sc1), and the last workgroup to take a ticket combines the FG partials in workgroup order and runs
// the scalar logic.  Fixed combine order: bitwise reproducible.  One workgroup reading every partial was
// bound by a single CU's memory parallelism (~1 us per 16-KB slot, 11 us for the residual + step test:
// MADIPM_FINAL_DEBUG stamps); spread over FG CUs each reads ~1/FG of it in one round trip.
// (Finalising inside the producing kernel instead — block 0 polling per-block flags, or a ticket —
// measured slower on ex10: the in-launch hand-off costs more than this launch.)
constexpr int FG = 16, FT = 128;  // workgroups, threads per workgroup (one partial block per thread)
static_assert(MAXB == FG * FT, "k_final: one partial block per thread");
constexpr int NL2 = 24;  // level-2 value slots: 8 generic + 4 alpha values + 4 alpha indices + eval

__device__ __forceinline__ double ld_sc1(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the step test's result (fraction-to-boundary ratios and their argmins) into the state
__device__ void fin_alpha_store(const DV& D, const FinParams& P, double (&a)[4], int (&ii)[4]) {
  DevState* st = D.st;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // mapreduce init (1.0, 0) is the fold's first element: an element whose ratio is exactly 1.0
    // comes later and replaces it (the index is the element's); larger ratios keep (1.0, init)
    if (!(a[k] <= 1.0)) {
      a[k] = 1.0;
      ii[k] = -1;
    }
  }
  st->a_xl = a[0];
  st->a_xu = a[1];
  st->a_zl = a[2];
  st->a_zu = a[3];
  st->i_xl = ii[0];
  st->i_xu = ii[1];
  st->i_zl = ii[2];
  st->i_zu = ii[3];
  const double ap = fmin(a[0], a[1]), ad = fmin(a[2], a[3]);
  if (P.alpha_mode == ALPHA_PRED) {
    st->alpha_aff_p = ap;
    st->alpha_aff_d = ad;
  } else if (P.alpha_mode == ALPHA_CONSERVATIVE || P.alpha_mode == ALPHA_ADAPTIVE) {
    st->alpha_p = ap;
    st->alpha_d = ad;
  } else {  // MEHROTRA / GONDZIO: keep in the aff slots for the follow-up pass
    st->alpha_aff_p = ap;
    st->alpha_aff_d = ad;
  }
}

// value slots and combine operation of each finaliser kind (compile time: the k_final instance's
// combines are branch-free)
constexpr int fin_nv(int kind) {
  return kind == FIN_RESID ? 3
         : kind == FIN_TERM ? 6
         : (kind == FIN_MU_PRED || kind == FIN_MU_FULL || kind == FIN_MU_GONDZIO || kind == FIN_ZINIT) ? 4
         : kind == FIN_ZSHIFT1 ? 8
         : (kind == FIN_EVAL || kind == FIN_ZSHIFT2) ? 1
                                                     : 0;
}
__host__ __device__ constexpr int fin_op(int kind, int k) {
  return (kind == FIN_RESID || (kind == FIN_TERM && k < 3)) ? OP_MAX : (kind == FIN_ZINIT ? OP_MIN : OP_SUM);
}

// the scalar logic of each finaliser kind on the reduced values res[] (thread 0 of the last workgroup)
__device__ void fin_tail(const DV& D, int kind, const FinParams& P, const double* res) {
  DevState* st = D.st;
  switch (kind) {
    case FIN_RESID: {
      const double ratio = res[0] / fmax(1.0, res[1]);  // linear_solver.jl:35
      st->res_ratio = ratio;
      st->max_res_ratio = nmax(st->max_res_ratio, ratio);
      st->dx_inf = res[2];
      if (ratio != ratio || (P.a > 0 && ratio > P.a)) st->nan_flag = 1;  // SolveException
      break;
    }
    case FIN_MU_PRED: {  // prediction_step! + update_barrier! (kernels.jl:176-220)
      const double cnt = P.a;  // nlb + nub
      const double mu_aff = cnt == 0 ? 0.0 : (res[2] + res[3]) / cnt;
      const double mu_curr = cnt == 0 ? 0.0 : (res[0] + res[1]) / cnt;
      double sigma = 1.0;
      if (P.b != 0.0) {  // has_inequalities
        const double q = mu_aff / mu_curr;
        sigma = fmin(fmax(q * q * q, 1e-6), 10.0);
      }
      st->mu_aff = mu_aff;
      st->mu_curr = mu_curr;
      st->mu = fmax(P.c, sigma * mu_curr);
      break;
    }
    case FIN_MU_FULL: {  // MehrotraAdaptiveStep (kernels.jl:309-358)
      const double cnt = P.a, gamma_f = P.b;
      const double gamma_a = 1.0 / (1.0 - gamma_f);
      double mu_full = cnt == 0 ? 0.0 : (res[2] + res[3]) / cnt;
      mu_full /= gamma_a;
      const double max_p = st->alpha_aff_p, max_d = st->alpha_aff_d;
      const int n = D.n, m = D.m, nlb = D.nlb;
      double ap = 1.0, ad = 1.0;
      if (max_p < 1.0) {
        if (st->a_xl <= st->a_xu) {
          const int k = st->i_xl, i = D.ind_lb[k];
          const double tmp = mu_full / (D.zl[i] + max_d * D.d[n + m + k]);
          ap = (D.x[i] - D.xl[i] - tmp) / (-D.d[i]);
        } else {
          const int k = st->i_xu, i = D.ind_ub[k];
          const double tmp = mu_full / (D.zu[i] + max_d * D.d[n + m + nlb + k]);
          ap = (D.xu[i] - D.x[i] - tmp) / (D.d[i]);
        }
      }
      if (max_d < 1.0) {
        if (st->a_zl <= st->a_zu) {
          const int k = st->i_zl, i = D.ind_lb[k];
          const double tmp = mu_full / (D.x[i] + max_p * D.d[i] - D.xl[i]);
          ad = -(D.zl[i] - tmp) / D.d[n + m + k];
        } else {
          const int k = st->i_zu, i = D.ind_ub[k];
          const double tmp = mu_full / (D.xu[i] - D.x[i] - max_p * D.d[i]);
          ad = -(D.zu[i] - tmp) / D.d[n + m + nlb + k];
        }
      }
      st->alpha_p = fmax(ap, gamma_f * max_p);
      st->alpha_d = fmax(ad, gamma_f * max_d);
      break;
    }
    case FIN_MU_GONDZIO: {
      const double cnt = P.a;
      st->mu_aff = cnt == 0 ? 0.0 : (res[2] + res[3]) / cnt;
      break;
    }
    case FIN_EVAL: st->obj_val = P.a + res[0]; break;
    case FIN_TERM:
      st->inf_du_raw = res[0];
      st->inf_compl_raw = res[1];
      st->inf_pr_raw = res[2];
      st->dobj = -res[3] + res[4] - res[5];
      break;
    case FIN_ZINIT:
      st->delta_x = fmax(fmax(0.0, -1.5 * res[0]), -1.5 * res[1]);
      st->delta_s = fmax(fmax(0.0, -1.5 * res[2]), -1.5 * res[3]);
      break;
    case FIN_ZSHIFT1: {
      double mu = 0.0;
      if (D.nlb > 0) mu += res[0] - res[1];
      if (D.nub > 0) mu += res[2] - res[3];
      st->delta_x2 = mu / (2 * (res[4] + res[5]));
      st->delta_s2 = mu / (2 * (res[6] + res[7]));
      break;
    }
    case FIN_ZSHIFT2: st->init_viol = res[0]; break;
  }
}

// Instantiated per (finaliser kind KIND, fused step test AL, fused objective EV) so that a thread holds
// exactly the partials of its launch and every combine is a compile-time operation (launch_final
// picks the instance).  Level-2 partials and the
// ticket live past the NPART x MAXB partials (part_): L2 = part + NPART MAXB, NL2 x FG doubles, then the
// ticket counter (reset by the last workgroup).
// NG == 1 (producers of at most FT1 blocks, MPCSolver::maxb_): ONE workgroup of FT1 threads reduces
// every partial in one round trip — no level-2 partials, no ticket.
template <int KIND, bool AL, bool EV, int NG = FG, int NTH = FT>
__global__ __launch_bounds__(NTH) void k_final(DV D, int kind, FinParams P) {
  constexpr int NV = fin_nv(KIND);
  __shared__ double res[NL2];
  __shared__ int s_last;
  DevState* st = D.st;
  double* L2 = D.part + NPART * MAXB;
  int32_t* ticket = reinterpret_cast<int32_t*>(L2 + NL2 * FG);
  const int g = blockIdx.x, b = g * NTH + threadIdx.x;
  if (P.dbg && threadIdx.x == 0 && g == 0) {
    P.dbg[0] = (int64_t)wall_clock64();
    P.dbg[3] = kind | (AL && NV > 0 ? 16 : 0) | (EV ? 32 : 0);
  }
  // every load first (unconditional: each slot holds MAXB partials, stale past nb), then the pins
  // (waits) and the selections — a predicated load compiles to a branch with a wait inside
  constexpr int NA = AL ? 8 : 0;
  double q[NV > 0 ? NV : 1], aq[AL ? 8 : 1], eq = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k) q[k] = D.part[pidx(b, k)];
#pragma unroll
  for (int k = 0; k < NA; ++k) aq[k] = D.part[pidx(b, (NV > 0 ? PART_ALPHA : 0) + k)];
  if (EV) eq = D.part[pidx(b, PART_EVAL)];
#pragma unroll
  for (int k = 0; k < NV; ++k) asm volatile("" : "+v"(q[k]));
#pragma unroll
  for (int k = 0; k < NA; ++k) asm volatile("" : "+v"(aq[k]));
  if (EV) asm volatile("" : "+v"(eq));
  if (P.dbg && threadIdx.x == 0 && g == 0) P.dbg[4] = (int64_t)wall_clock64();  // loads returned
  // level 1: this workgroup's blocks — every value's shuffle tree in lockstep (one latency chain for all
  // of them, not one per value), then the waves in order
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double w1[NV > 0 ? NV : 1], av[4];
  int ai[4];
#pragma unroll
  for (int k = 0; k < NV; ++k) w1[k] = b < P.nb ? q[k] : 0.0;
  const int nba = NV > 0 ? P.nb_alpha : P.nb;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    av[k] = (AL && b < nba) ? aq[k] : INF;
    ai[k] = (AL && b < nba) ? (int)aq[AL ? 4 + k : 0] : -1;
  }
  double e1 = (EV && b < P.nb_eval) ? eq : 0.0;
  // every value's tree in lockstep (one latency chain for all of them), the __shfl_down pairing
  auto stage = [&](auto otag) {
    constexpr int O = decltype(otag)::value;
#pragma unroll
    for (int k = 0; k < NV; ++k) w1[k] = comb(w1[k], lane_down<O>(w1[k]), fin_op(KIND, k));
    if (AL)
#pragma unroll
      for (int k = 0; k < 4; ++k) argmin_step<O>(av[k], ai[k]);
    if (EV) e1 += lane_down<O>(e1);
  };
  stage(std::integral_constant<int, 32>{});
  stage(std::integral_constant<int, 16>{});
  stage(std::integral_constant<int, 8>{});
  stage(std::integral_constant<int, 4>{});
  stage(std::integral_constant<int, 2>{});
  stage(std::integral_constant<int, 1>{});
  __shared__ double shv[NL2][NTH / 64];
  __shared__ int shx[4][NTH / 64];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) shv[k][wv] = w1[k];
    if (AL)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        shv[8 + k][wv] = av[k];
        shx[k][wv] = ai[k];
      }
    if (EV) shv[16][wv] = e1;
  }
  __syncthreads();
  if constexpr (NG == 1) {  // the waves in order, straight into res[]
    const int t = threadIdx.x;
    if (t < NV) {
      double a = shv[t][0];
#pragma unroll
      for (int w = 1; w < NTH / 64; ++w) a = comb(a, shv[t][w], fin_op(KIND, t));
      res[t] = a;
    } else if (AL && t >= 8 && t < 12) {
      double a = shv[t][0];
      int ix = shx[t - 8][0];
#pragma unroll
      for (int w = 1; w < NTH / 64; ++w) amin_upd(a, ix, shv[t][w], shx[t - 8][w]);
      res[t] = a;
      res[t + 4] = (double)ix;
    } else if (EV && t == 16) {
      double a = shv[16][0];
#pragma unroll
      for (int w = 1; w < NTH / 64; ++w) a += shv[16][w];
      res[16] = a;
    }
    if (P.dbg && t == 0) P.dbg[5] = P.dbg[6] = (int64_t)wall_clock64();
    __syncthreads();
  } else {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      double a = shv[k][0];
#pragma unroll
      for (int w = 1; w < FT / 64; ++w) a = comb(a, shv[k][w], fin_op(KIND, k));
      st_sc1(L2 + k * FG + g, a);
    }
    if (AL)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double a = shv[8 + k][0];
        int ix = shx[k][0];
#pragma unroll
        for (int w = 1; w < FT / 64; ++w) amin_upd(a, ix, shv[8 + k][w], shx[k][w]);
        st_sc1(L2 + (8 + k) * FG + g, a);
        st_sc1(L2 + (12 + k) * FG + g, (double)ix);
      }
    if (EV) {
      double a = shv[16][0];
#pragma unroll
      for (int w = 1; w < FT / 64; ++w) a += shv[16][w];
      st_sc1(L2 + 16 * FG + g, a);
    }
    if (P.dbg && g == 0) P.dbg[5] = (int64_t)wall_clock64();  // level 1 reduced
    // release: this workgroup's level-2 partials are visible before its ticket; the last
    // workgroup's acquire (below) pairs with every earlier release on the ticket's RMW chain
    s_last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == FG - 1;
    if (P.dbg && s_last) P.dbg[6] = (int64_t)wall_clock64();  // last ticket taken
  }
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // every thread of the last workgroup: see the partials
  // level 2 (last workgroup): every level-2 partial loaded at once (one per thread, sc1), then thread k
  // combines value slot k over the workgroups in order
  const int t = threadIdx.x;
  __shared__ double l2s[NL2 * FG];
  constexpr int NUSE = AL ? (EV ? 17 : 16) : (EV ? 17 : NV);  // slots in use: 0..NV-1, 8..15 (alpha), 16 (eval)
  static_assert(NUSE * FG <= 3 * FT, "level 2: at most three loads per thread");
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const int e = t + h * FT;
    if (e < NUSE * FG) l2s[e] = ld_sc1(L2 + e);
  }
  __syncthreads();
  if (t < NV) {
    double a = l2s[t * FG];
#pragma unroll
    for (int w = 1; w < FG; ++w) a = comb(a, l2s[t * FG + w], fin_op(KIND, t));
    res[t] = a;
  } else if (AL && t >= 8 && t < 12) {
    double a = l2s[t * FG];
    int ix = (int)l2s[(t + 4) * FG];
#pragma unroll
    for (int w = 1; w < FG; ++w) amin_upd(a, ix, l2s[t * FG + w], (int)l2s[(t + 4) * FG + w]);
    res[t] = a;
    res[t + 4] = (double)ix;
  } else if (EV && t == 16) {
    double a = l2s[16 * FG];
#pragma unroll
    for (int w = 1; w < FG; ++w) a += l2s[16 * FG + w];
    res[16] = a;
  }
  __syncthreads();
  }  // NG > 1
  const int t = threadIdx.x;
  if (t >= 64) return;
  if (t == 0) {
    if (NG > 1) *ticket = 0;  // every workgroup has taken its ticket: reset for the next launch
    if (P.dbg) P.dbg[1] = (int64_t)wall_clock64();
    if (AL) {
      double a[4];
      int ii[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] = res[8 + k];
        ii[k] = (int)res[12 + k];
      }
      fin_alpha_store(D, P, a, ii);
    }
    if (EV) st->obj_val = P.c + res[16];  // FIN_TERM: the previous iteration's FIN_EVAL, deferred here
    if (NV > 0) {
      if (P.rs) ldl_status_start(P.rs);
      fin_tail(D, kind, P, res);
    }
    if (P.dbg) {
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      P.dbg[2] = (int64_t)wall_clock64();
    }
  }
  if (P.host) {  // publish the state right here (the termination test's, before the factorisation):
    // lane 0's state stores drained to L2, the wave reads them back past L1 and publishes
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    publish_state(st, P.host, P.hseq, P.seq, true);
  }
}

// the k_final instance of a finaliser launch (slots, fused step test, fused objective)
constexpr int FT1 = 1024;  // the single-workgroup finaliser's threads (one partial block each)
void launch_final(const DV& D, int kind, const FinParams& P, hipStream_t s) {
  // one workgroup when every producer launch had at most FT1 blocks (maxb_ <= FT1), else FG of them
  const bool one = std::max(P.nb, std::max(P.nb_alpha, P.nb_eval)) <= FT1;
#define LF(K, AL, EV)                                                 \
  do {                                                                \
    if (one)                                                          \
      k_final<K, AL, EV, 1, FT1><<<1, FT1, 0, s>>>(D, kind, P);       \
    else                                                              \
      k_final<K, AL, EV><<<FG, FT, 0, s>>>(D, kind, P);               \
  } while (0)
  switch (kind) {
    case FIN_ALPHA: LF(FIN_ALPHA, true, false); break;
    case FIN_RESID:
      if (P.nb_alpha > 0)
        LF(FIN_RESID, true, false);
      else
        LF(FIN_RESID, false, false);
      break;
    case FIN_MU_PRED: LF(FIN_MU_PRED, false, false); break;
    case FIN_MU_FULL: LF(FIN_MU_FULL, false, false); break;
    case FIN_MU_GONDZIO: LF(FIN_MU_GONDZIO, false, false); break;
    case FIN_ZINIT: LF(FIN_ZINIT, false, false); break;
    case FIN_EVAL: LF(FIN_EVAL, false, false); break;
    case FIN_ZSHIFT2: LF(FIN_ZSHIFT2, false, false); break;
    case FIN_TERM:
      if (P.nb_eval > 0)
        LF(FIN_TERM, false, true);
      else
        LF(FIN_TERM, false, false);
      break;
    case FIN_ZSHIFT1: LF(FIN_ZSHIFT1, false, false); break;
    default: throw Error("k_final: unknown finaliser kind", -2);
  }
#undef LF
}

__global__ void k_publish(const DevState* __restrict__ st, DevState* host, uint32_t* hseq, uint32_t seq) {
  publish_state(st, host, hseq, seq);
}

__global__ void k_copy(double* __restrict__ dst, const double* __restrict__ src, int64_t n) {
  GRID_LOOP(i, n) dst[i] = src[i];
}
// get_solution's constraint values: one wave per row of J (CSR), the columns < nx (A's; the slack
// columns left out), a fixed-order wave sum, + cfix (the fixed columns' terms)
__global__ __launch_bounds__(NT) void k_cons(const int64_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                             const double* __restrict__ v, const double* __restrict__ x,
                                             const double* __restrict__ cfix, int m, int nx, double* __restrict__ out) {
  const int row = blockIdx.x * (NT / 64) + threadIdx.x / 64, l = threadIdx.x & 63;
  if (row >= m) return;
  double a = 0.0;
  for (int64_t p = rp[row] + l; p < rp[row + 1]; p += 64) {
    const int c = ci[p];
    if (c < nx) a = fma(v[p], x[c], a);
  }
  a = wave_reduce<OP_SUM>(a);
  if (l == 0) out[row] = a + cfix[row];
}
__global__ void k_axpy_x(DV D) {
  GRID_LOOP(i, D.n) D.x[i] += D.d[i];
}
__global__ void k_copy_y(DV D) {
  GRID_LOOP(j, D.m) D.y[j] = D.d[D.n + j];
}
// Gondzio: set_extra_correction! (kernels.jl:74-122)
__global__ void k_extra_corr(DV D, double ap, double ad, double tmin, double tmax) {
  const int n = D.n, m = D.m, nlb = D.nlb, nub = D.nub;
  GRID_LOOP(t, (nlb > nub ? nlb : nub)) {
    if (t < nlb) {
      const int i = D.ind_lb[t];
      const double xx = D.x[i] + ap * D.d[i] - D.xl[i];
      const double zz = D.zl[i] + ad * D.d[n + m + t];
      const double v = xx * zz;
      const double del = v < tmin ? tmin - v : (v > tmax ? tmax - v : 0.0);
      D.corr_lb[t] = D.corr_lb[t] - del;
    }
    if (t < nub) {
      const int i = D.ind_ub[t];
      const double xx = D.xu[i] - ap * D.d[i] - D.x[i];
      const double zz = D.zu[i] + ad * D.d[n + m + nlb + t];
      const double v = xx * zz;
      const double del = v < tmin ? tmin - v : (v > tmax ? tmax - v : 0.0);
      D.corr_ub[t] = D.corr_ub[t] + del;
    }
  }
}

double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

// ======================================================================= host side

MPCSolver::~MPCSolver() {
  if (fdbg_.p) {  // MADIPM_FINAL_DEBUG: per finaliser kind, thread 0's mean time to the reduced values / to the end
    std::vector<int64_t> h((size_t)8 * kFinDbg);
    (void)hipStreamSynchronize(stream_);
    (void)hipMemcpy(h.data(), fdbg_.p, h.size() * 8, hipMemcpyDeviceToHost);
    std::map<int64_t, std::array<double, 6>> acc;
    for (int64_t q = 0; q < std::min<int64_t>(fdbg_n_, kFinDbg); ++q) {
      const int64_t* e = &h[8 * q];
      auto& a = acc[e[3]];
      a[0] += 1;
      a[1] += (e[4] - e[0]) * 1e-2;  // 100 MHz ticks -> us
      a[2] += (e[5] - e[0]) * 1e-2;
      a[3] += (e[6] - e[0]) * 1e-2;
      a[4] += (e[1] - e[0]) * 1e-2;
      a[5] += (e[2] - e[0]) * 1e-2;
    }
    for (auto& kv : acc) {
      const double n = kv.second[0];
      std::fprintf(stderr,
                   "k_final kind %2lld (alpha %d eval %d): %6.0f launches  wg0 loads %6.2f  wg0 level-1 %6.2f  last ticket "
                   "%6.2f  reduced %6.2f  end %6.2f us\n",
                   (long long)(kv.first & 15), (int)((kv.first >> 4) & 1), (int)((kv.first >> 5) & 1), n,
                   kv.second[1] / n, kv.second[2] / n, kv.second[3] / n, kv.second[4] / n, kv.second[5] / n);
    }
  }
  if (hst_) (void)hipHostFree(hst_);
  for (hipEvent_t e : sol_ev_)
    if (e) (void)hipEventDestroy(e);
  if (stream_) (void)hipStreamDestroy(stream_);
}

int MPCSolver::blocks(int64_t n) const {
  int64_t b = (n + NT - 1) / NT;
  return (int)std::max<int64_t>(1, std::min<int64_t>(maxb_, b));
}

// GROUP_LOOP SpMV kernels: one row per lane group (spmv_g_ lanes), so a group walks one row instead
// of a dependent chain of rows (the row loads are latency-bound)
int MPCSolver::spmv_blocks(int64_t rows) const { return blocks(rows * spmv_g_); }

MPCSolver::MPCSolver(const madipm_qp& qp, const madipm_options& opt, Comm* comm) : opt_(opt), comm_(comm) {
  const double t0 = now();
  PhaseClock clk("MPCSolver");
  MADIPM_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  clk("stream");
  // state mirror + publication counter on their own line: coherent host memory, written by k_publish
  constexpr size_t seq_off = (sizeof(DevState) + 63) / 64 * 64;
  MADIPM_HIP(hipHostMalloc((void**)&hst_, seq_off + 64, hipHostMallocCoherent));
  std::memset((void*)hst_, 0, seq_off + 64);
  hseq_ = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(hst_) + seq_off);
  clk("host state");
  setup_host(qp);
  clk("setup_host (its locals freed)");
  t_init_ = now() - t0;
}

// The linear solver: one LDL^T, or a sharded one — across processes (comm, RCCL) or as a group of
// shards on this device (ldl.nshards > 1, ShardGroup)
std::unique_ptr<LinSolver> MPCSolver::make_linsolver(int n, const int64_t* cp, const int32_t* ri,
                                                     const SymbolicOptions& so) {
  ++n_analyses_;
  if (comm_ && comm_->size > 1) {
    SymbolicOptions o = so;
    o.nshards = comm_->size;
    o.shard = comm_->rank;
    return std::make_unique<LDLSolver>(n, cp, ri, o, opt_.ldl.pivot_tol, nullptr, comm_);
  }
  if (opt_.ldl.nshards > 1)
    return std::make_unique<ShardGroup>(opt_.ldl.nshards, n, cp, ri, so, opt_.ldl.pivot_tol);
  return std::make_unique<LDLSolver>(n, cp, ri, so, opt_.ldl.pivot_tol);
}

// Host-side construction: the problem model (qp_model.hpp) is built on the host, the linear solver is
// analysed, everything is uploaded and the stream synchronised.
void MPCSolver::setup_host(const madipm_qp& q) {
  PhaseClock clk("setup_host");
  H_ = std::make_unique<QPHost>();
  QPHost& P = *H_;
  qp_intake(P, q, &clk);
  // ---- everything that depends on the numbers and is O(n + m) long: shared with update()
  HostNumeric num;
  JCoo jcoo;
  numeric_host(P, opt_, num, &jcoo);
  obj_scale_ = num.obj_scale;
  c0s_ = num.c0s;
  norm_b_ = num.norm_b;
  clk("initialize + scaling");
  const int nx = P.nx, m = P.m, n = P.n;
  nx_ = nx;
  ns_ = P.ns;
  n_ = n;
  m_ = m;
  nlb_ = (int)P.ind_lb.size();
  nub_ = (int)P.ind_ub.size();
  L_ = (int64_t)n + m + nlb_ + nub_;
  // ---- H, J, J^T CSR, the K2 pattern and (kkt_system 2) the normal equations' pattern
  kkt_ = opt_.kkt_system;
  QPStructure S = build_structure(P, opt_, jcoo, &clk);
  nnzK_ = P.nnzK;
  if (const char* e = std::getenv("MADIPM_SPEC_NEAR")) spec_near_ = std::max(0.0, std::atof(e));
  if (const char* e = std::getenv("MADIPM_FINAL_DEBUG"); e && e[0] == '1') {
    fdbg_.alloc(8 * kFinDbg);
    MADIPM_HIP(hipMemset(fdbg_.p, 0, 8 * kFinDbg * sizeof(int64_t)));
  }
  {  // SpMV lane-group width: ~2 entries per lane on an average row of [H A^T; A]
    const double avg = (double)(P.nH + 2 * P.nJ) / std::max(1, n + m);
    spmv_g_ = 4;
    while (spmv_g_ < 64 && spmv_g_ * 2 < avg) spmv_g_ *= 2;
    if (const char* e = std::getenv("MADIPM_SPMV_G")) {  // tests / A-B: force the width (4..64, power of two)
      const int g = std::atoi(e);
      if (g == 4 || g == 8 || g == 16 || g == 32 || g == 64) spmv_g_ = g;
    }
  }
  // ---- LDL^T symbolic analysis + device plan (linear-solver constructor)
  SymbolicOptions so;
  so.ordering = opt_.ldl.ordering;
  so.dense_alpha = opt_.ldl.dense_alpha;
  so.relax = opt_.ldl.relax;
  so.small_front_max = opt_.ldl.small_front_max;
  if (kkt_ == KKT_NORMAL) {
    nnzC_ = (int64_t)S.Cri.size();
    ldl_ = make_linsolver(m, S.Ccp.data(), S.Cri.data(), so);
    ldl_->spd = true;  // Cholesky semantics (test/test_gpu.jl:11): a non-positive pivot fails
  } else {
    ldl_ = make_linsolver(n + m, S.Kcp.data(), S.Kri.data(), so);
  }

  clk("linear solver (analysis + plan)");
  // ---- uploads
  hipStream_t s = stream_;
  auto up = [&](auto& buf, const auto& vec, size_t minlen = 1) {
    using T = typename std::decay_t<decltype(vec)>::value_type;
    buf.alloc(std::max(vec.size(), minlen));
    if (!vec.empty()) MADIPM_HIP(hipMemcpyAsync(buf.p, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice, s));
  };
  up(x_, P.x);
  up(xl_, P.xl);
  up(xu_, P.xu);
  up(y_, P.y);
  up(rhs_, P.rhs);
  up(Hdiag_, S.Hdiag);
  up(cs_, num.cs);
  up(gfix_, num.gfix);
  up(cfix_, num.cfix);
  up(diag_pos_, S.diag_pos);
  up(Kx_, S.Kv);
  up(ind_lb_, P.ind_lb);
  up(ind_ub_, P.ind_ub);
  up(lbpos_, S.lbpos);
  up(ubpos_, S.ubpos);
  up(fixed_, P.fixed);
  up(Hrp_, S.Hrp);
  up(Hci_, S.Hci);
  up(Hv_, S.Hcv);
  up(Jrp_, S.Jrp);
  up(Jci_, S.Jci);
  up(Jv_, S.Jcv);
  up(JTrp_, S.JTrp);
  up(JTci_, S.JTci);
  up(JTv_, S.JTcv);
  auto zeros = [&](DBuf<double>& b, int64_t len) {
    b.alloc(std::max<int64_t>(len, 1));
    b.zero(s);
  };
  zeros(zl_, n);
  zeros(zu_, n);
  zeros(f_, n);
  zeros(jacl_, n);
  zeros(c_, m);
  zeros(pr_diag_, n);
  zeros(l_diag_, nlb_);
  zeros(u_diag_, nub_);
  zeros(l_lower_, nlb_);
  zeros(u_lower_, nub_);
  zeros(d_, L_);
  zeros(p_, L_);
  zeros(dsave_, L_);
  zeros(corr_lb_, nlb_);
  zeros(corr_ub_, nub_);
  if (kkt_ == KKT_NORMAL) {
    up(cpp_, S.cpp);
    up(cprod_, S.cprod, 2);
    zeros(Cx_, nnzC_);
    zeros(Dinv_, n);
    zeros(bufm_, m);
  } else if (kkt_ == KKT_K25) {
    const hvec<int32_t> kcol = k2_slot_columns(S.Kcp);
    up(Krow_, S.Kri);
    up(Kcol_, kcol);
    up(K0_, S.Kv);
    zeros(sk_, n);
  }
  part_.alloc(MAXB * NPART + NL2 * FG + 8);  // + k_final's level-2 partials and ticket
  MADIPM_HIP(hipMemset(part_.p, 0, (MAXB * NPART + NL2 * FG + 8) * sizeof(double)));
  st_.alloc(1);
  if (ldl_->external_status(&st_.p->ldl_status, &hst_->ldl_status)) {  // carried by read_state()
    // the MPC's own kernels start / end each factorisation: no k_status_init, no k_inertia (K2, K2.5:
    // the pivot check needs no inertia; the normal equations' Cholesky check keeps k_inertia)
    ldl_->ext_reset = true;
    ldl_->lazy_inertia = !ldl_->spd;
  }
  st_.zero(s);
  MADIPM_HIP(hipStreamSynchronize(s));
  clk("uploads");
  // the host copies of J, J^T and K2 (dense QP: ~18 GB) are released on a thread of their own: their
  // page-table teardown took 2.1 s of the construction on the box (r6) with nothing waiting for it
  free_async(std::move(S));
}

// ======================================================================= re-solve with new numbers
// madipm_solver_prepare_update / madipm_solver_update: the pattern, the ordering, the symbolic
// factorisation, the device plan and every allocation stay; the vectors are recomputed by numeric_host
// and the matrix values (Jv_, JTv_, Hv_, Hdiag_, the H and J entries of Kx_, K0_) by the kernels below.
namespace {

// The kernels round as the host construction does: each product con_scale[r] * Av[k] or
// (obj_scale * sgn) * Hv[k] is rounded before it is added (no FMA: contraction is off inside them), a
// destination's first source is taken as it is and the others are added in ascending input index.
// One thread per destination entry: the writes are coalesced, the sources are gathered; no atomics.
__global__ void k_refresh_jt(int64_t nd, const int32_t* __restrict__ sp, const int32_t* __restrict__ src,
                             const int32_t* __restrict__ row, const double* __restrict__ cs,
                             const double* __restrict__ raw, const int32_t* __restrict__ kpos,
                             double* __restrict__ JTv, double* __restrict__ Kx, double* __restrict__ K0) {
#pragma clang fp contract(off)
  GRID_LOOP(q, nd) {
    const int a = sp[q], b = sp[q + 1];
    if (a == b) continue;  // a slack column's -1.0 never changes
    const double s = cs[row[q]];
    double acc = s * raw[src[a]];
    for (int t = a + 1; t < b; ++t) {
      const double p = s * raw[src[t]];
      acc = acc + p;
    }
    JTv[q] = acc;
    const int kp = kpos[q];  // ascending in q: K2's column j holds row j of J^T contiguously
    Kx[kp] = acc;
    if (K0) K0[kp] = acc;
  }
}
__global__ void k_refresh_h(int64_t nd, const int32_t* __restrict__ sp, const int32_t* __restrict__ src, double os,
                            const double* __restrict__ raw, const int32_t* __restrict__ kpos,
                            double* __restrict__ Hv, double* __restrict__ Kx, double* __restrict__ K0) {
#pragma clang fp contract(off)
  GRID_LOOP(q, nd) {
    const int a = sp[q], b = sp[q + 1];
    if (a == b) continue;
    double acc = os * raw[src[a]];
    for (int t = a + 1; t < b; ++t) {
      const double p = os * raw[src[t]];
      acc = acc + p;
    }
    Hv[q] = acc;
    const int kp = kpos[q];  // -1: diagonal or upper triangle (K2 keeps H's strict lower part)
    if (kp >= 0) {
      Kx[kp] = acc;
      if (K0) K0[kp] = acc;
    }
  }
}
// Hdiag[i] is the host's 0.0 + v1 + v2 + ...; H's entry (i, i) is v1 + v2 + ...: they differ only where
// every source is -0.0, which adding 0.0 to the entry restores
__global__ void k_refresh_hdiag(int n, const int32_t* __restrict__ pos, const double* __restrict__ Hv,
                                double* __restrict__ Hdiag) {
#pragma clang fp contract(off)
  GRID_LOOP(i, n) {
    const int p = pos[i];
    Hdiag[i] = p >= 0 ? 0.0 + Hv[p] : 0.0;
  }
}
__global__ void k_refresh_gather(int64_t nd, const int32_t* __restrict__ map, const double* __restrict__ from,
                                 double* __restrict__ to) {
  GRID_LOOP(q, nd) to[q] = from[map[q]];
}

// ----------------------------------------------------------------- the device route (update_device)
// numeric_host restated as kernels over device-resident raw data.  One thread per destination; a
// destination's sources come from its list [sp[i], sp[i + 1]) of (input index, other index) pairs in
// ascending input index, so every sum has the host loop's order; contraction is off, so every product is
// rounded before it is added; the two maxima are integer maxima over the bit patterns of non-negative
// doubles (order-free, hence deterministic).  std::min / std::max are restated with their own comparisons
// (a NaN operand is kept or dropped exactly as on the host).
__device__ __forceinline__ double smax(double a, double b) { return a < b ? b : a; }  // std::max(a, b)
__device__ __forceinline__ double smin(double a, double b) { return b < a ? b : a; }  // std::min(a, b)
__device__ __forceinline__ int dev_bound_class(double l, double u) {
  return l == u ? 1 : (l != -INF ? 2 : 0) | (u != INF ? 4 : 0);
}
// after the loop every lane of the block is active again: one wave maximum, one integer atomic per wave
__device__ __forceinline__ void publish_max(double a, double* slot) {
  a = wave_reduce<OP_MAX>(a);
  if ((threadIdx.x & 63) == 0 && a > 0.0)
    atomicMax(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)__double_as_longlong(a));
}

enum { SC_OS = 0, SC_OBJ = 1, SC_C0S = 2, SC_NORMB = 3, SC_GMAX = 4, SC_LEN = 8 };

// The host's classification check on the merged data: out[0] = first row whose equality / ranged kind
// changed, out[1] = first variable, out[2] = first ranged row whose bound class changed (INT32_MAX: none).
// The classes were fixed at creation (vcls, ccls).
__global__ void k_upd_check(int nx, int m, const double* __restrict__ lv, const double* __restrict__ uv,
                            const double* __restrict__ lc, const double* __restrict__ uc,
                            const uint8_t* __restrict__ vcls, const uint8_t* __restrict__ ccls,
                            int32_t* __restrict__ out) {
  GRID_LOOP(i, (nx > m ? nx : m)) {
    if (i < m) {
      const int was = ccls[i], is = dev_bound_class(lc[i], uc[i]);
      if ((was == 1) != (is == 1))
        atomicMin(&out[0], (int)i);
      else if (was != is)
        atomicMin(&out[2], (int)i);
    }
    if (i < nx && dev_bound_class(lv[i], uv[i]) != vcls[i]) atomicMin(&out[1], (int)i);
  }
}

// raw_bounds + MadNLP.initialize!'s start and bound relaxation: xl / xu of [x; s], the structural start
// (x0, a fixed variable at its value) as it is before the bound push
__global__ void k_upd_bounds(int nx, int n, double tol, const double* __restrict__ lvar,
                             const double* __restrict__ uvar, const double* __restrict__ lcon,
                             const double* __restrict__ ucon, const double* __restrict__ x0,
                             const int32_t* __restrict__ ineq, const uint8_t* __restrict__ fixed,
                             double* __restrict__ xl, double* __restrict__ xu, double* __restrict__ xpre) {
#pragma clang fp contract(off)
  GRID_LOOP(i, n) {
    const bool fx = fixed[i];
    double l, u;
    if (i < nx) {
      l = lvar[i], u = uvar[i];
      xpre[i] = fx ? l : x0[i];
    } else {
      const int r = ineq[i - nx];
      l = lcon[r], u = ucon[r];
    }
    if (!fx) {
      if (__builtin_isfinite(l)) l = l - tol * smax(1.0, fabs(l));
      if (__builtin_isfinite(u)) u = u + tol * smax(1.0, fabs(u));
    }
    xl[i] = l;
    xu[i] = u;
  }
}

// per constraint row: the slack start (A x)_r over every entry of the row, the row maximum -> con_scale,
// cfix over the row's fixed-column entries, rhs (scaled) and its part of norm_b
__global__ __launch_bounds__(NT) void k_upd_rows(int m, int scaling, const int32_t* __restrict__ asp,
                                                 const int2* __restrict__ ae, const int32_t* __restrict__ fsp,
                                                 const int2* __restrict__ fe, const double* __restrict__ Av,
                                                 const double* __restrict__ xpre, const double* __restrict__ lcon,
                                                 const double* __restrict__ ucon, double* __restrict__ ax,
                                                 double* __restrict__ cscale, double* __restrict__ cfix,
                                                 double* __restrict__ rhs, double* __restrict__ sc) {
#pragma clang fp contract(off)
  double nb = 0.0;
  GRID_LOOP(r, m) {
    double s = 0.0, rm = 0.0;
    const int a = asp[r], b = asp[r + 1];
    for (int t = a; t < b; ++t) {
      const int2 e = ae[t];
      const double v = Av[e.x];
      const double p = v * xpre[e.y];
      s = s + p;
      rm = smax(rm, fabs(v));
    }
    ax[r] = s;
    const double cs = scaling ? smin(1.0, 100.0 / rm) : 1.0;
    cscale[r] = cs;
    double cf = 0.0;
    for (int t = fsp[r]; t < fsp[r + 1]; ++t) {
      const int2 e = fe[t];
      const double v = cs * Av[e.x];
      const double p = v * xpre[e.y];
      cf = cf + p;
    }
    cfix[r] = cf;
    const double l = lcon[r];
    double h = l == ucon[r] ? l : 0.0;
    if (scaling) h = h * cs;
    rhs[r] = h;
    nb = smax(nb, fabs(h));
  }
  publish_max(nb, sc + SC_NORMB);
}

// the slack start, initialize_variables!'s bound push, then the slack rows of x / xl / xu times con_scale
__global__ void k_upd_start(int nx, int n, int scaling, double bp, double bf, const double* __restrict__ xpre,
                            const double* __restrict__ ax, const double* __restrict__ cscale,
                            const int32_t* __restrict__ ineq, const uint8_t* __restrict__ fixed,
                            double* __restrict__ xl, double* __restrict__ xu, double* __restrict__ x) {
#pragma clang fp contract(off)
  GRID_LOOP(i, n) {
    const int r = i < nx ? -1 : ineq[i - nx];
    double v = i < nx ? xpre[i] : ax[r];
    double l = xl[i], u = xu[i];
    if (!fixed[i]) {
      double lo = -INF, hi = INF;
      if (__builtin_isfinite(l)) {
        double pl = bp * smax(1.0, fabs(l));
        if (__builtin_isfinite(u)) pl = smin(pl, bf * (u - l));
        lo = l + pl;
      }
      if (__builtin_isfinite(u)) {
        double pu = bp * smax(1.0, fabs(u));
        if (__builtin_isfinite(l)) pu = smin(pu, bf * (u - l));
        hi = u - pu;
      }
      v = smin(smax(v, lo), hi);
    }
    if (r >= 0 && scaling) {
      const double cs = cscale[r];
      xl[i] = l * cs;
      xu[i] = u * cs;
      v = v * cs;
    }
    x[i] = v;
  }
}

// set_scaling!'s objective gradient at the start: g[i] = sgn c[i] + the H terms of variable i in input
// order; its maximum magnitude -> sc[SC_GMAX]
__global__ __launch_bounds__(NT) void k_upd_g(int nx, double sgn, const int32_t* __restrict__ gsp,
                                              const int2* __restrict__ ge, const double* __restrict__ c,
                                              const double* __restrict__ Hv, const double* __restrict__ x,
                                              double* __restrict__ sc) {
#pragma clang fp contract(off)
  double gm = 0.0;
  GRID_LOOP(i, nx) {
    double g = sgn * c[i];
    for (int t = gsp[i]; t < gsp[i + 1]; ++t) {
      const int2 e = ge[t];
      const double v = sgn * Hv[e.x];
      const double p = v * x[e.y];
      g = g + p;
    }
    gm = smax(gm, fabs(g));
  }
  publish_max(gm, sc + SC_GMAX);
}

// one thread: obj_scale, obj_scale * sgn, and c0s with const_fixed summed over the both-fixed H entries
// (bf: input index, row, column) in input order
__global__ void k_upd_scalars(int scaling, double sgn, double c0, int nbf, const int32_t* __restrict__ bfk,
                              const int2* __restrict__ bfrc, const double* __restrict__ Hv,
                              const double* __restrict__ x, double* __restrict__ sc) {
#pragma clang fp contract(off)
  if (blockIdx.x || threadIdx.x) return;
  double os = 1.0;
  if (scaling) {
    const double gmax = sc[SC_GMAX];
    os = gmax > 0 ? smin(1.0, 100.0 / gmax) : 1.0;
  }
  const double oss = os * sgn;
  double cf = 0.0;
  for (int t = 0; t < nbf; ++t) {
    const int2 rc = bfrc[t];
    const double v = oss * Hv[bfk[t]];
    const double p = (((rc.x == rc.y ? 0.5 : 1.0) * v) * x[rc.x]) * x[rc.y];
    cf = cf + p;
  }
  const double sc0 = sgn * c0;
  const double t0 = os * sc0;
  sc[SC_OBJ] = os;
  sc[SC_OS] = oss;
  sc[SC_C0S] = t0 + cf;
}

// cs = (obj_scale sgn) c, and gfix: the cross terms of the fixed variables into the free ones
__global__ void k_upd_cs_gfix(int nx, int n, const int32_t* __restrict__ xsp, const int2* __restrict__ xe,
                              const double* __restrict__ c, const double* __restrict__ Hv,
                              const double* __restrict__ x, const double* __restrict__ sc, double* __restrict__ cs,
                              double* __restrict__ gfix) {
#pragma clang fp contract(off)
  const double oss = sc[SC_OS];
  GRID_LOOP(i, n) {
    double gf = 0.0, cv = 0.0;
    if (i < nx) {
      cv = oss * c[i];
      for (int t = xsp[i]; t < xsp[i + 1]; ++t) {
        const int2 e = xe[t];
        const double v = oss * Hv[e.x];
        const double p = v * x[e.y];
        gf = gf + p;
      }
    }
    cs[i] = cv;
    gfix[i] = gf;
  }
}

// k_refresh_h with obj_scale * sgn read from the device scalar block
__global__ void k_refresh_h_dev(int64_t nd, const int32_t* __restrict__ sp, const int32_t* __restrict__ src,
                                const double* __restrict__ sc, const double* __restrict__ raw,
                                const int32_t* __restrict__ kpos, double* __restrict__ Hv, double* __restrict__ Kx,
                                double* __restrict__ K0) {
#pragma clang fp contract(off)
  const double os = sc[SC_OS];
  GRID_LOOP(q, nd) {
    const int a = sp[q], b = sp[q + 1];
    if (a == b) continue;
    double acc = os * raw[src[a]];
    for (int t = a + 1; t < b; ++t) {
      const double p = os * raw[src[t]];
      acc = acc + p;
    }
    Hv[q] = acc;
    const int kp = kpos[q];
    if (kp >= 0) {
      Kx[kp] = acc;
      if (K0) K0[kp] = acc;
    }
  }
}

// update_solution! on the device: x, z_L / obj_scale, z_U / obj_scale, y con_scale / obj_scale, and the
// constraint values k_cons left in `ax`, / con_scale (any output may be null)
__global__ void k_unscale(int nx, int m, double os, const double* __restrict__ x, const double* __restrict__ y,
                          const double* __restrict__ zl, const double* __restrict__ zu,
                          const double* __restrict__ ax, const double* __restrict__ cscale, double* __restrict__ ox,
                          double* __restrict__ oy, double* __restrict__ ozl, double* __restrict__ ozu,
                          double* __restrict__ ocons) {
#pragma clang fp contract(off)
  GRID_LOOP(i, (nx > m ? nx : m)) {
    if (i < nx) {
      if (ox) ox[i] = x[i];
      if (ozl) ozl[i] = zl[i] / os;
      if (ozu) ozu[i] = zu[i] / os;
    }
    if (i < m) {
      const double cs = cscale[i];
      if (oy) oy[i] = y[i] * cs / os;
      if (ocons) ocons[i] = ax[i] / cs;
    }
  }
}

// ---- warm start (madipm_solver_set_warm_start*): initialize() blends the cold start with a
// caller-given point of the public, un-scaled space.  One thread (k_warm_rows: one lane group) per
// destination, every sum in a fixed order, no atomics: the same bits from run to run.
struct WarmArgs {
  const double *wx, *wy, *wzl, *wzu;  // the warm point (null: the block is absent and keeps its cold values)
  const double* cscale;               // con_scale
  const int32_t* ineq;                // slack k -> its constraint row
  double* rows;                       // per slack: the scaled row value of the clamped x (k_warm_rows)
  double lam, os;                     // weight, obj_scale
};

// comparisons, not fmin / fmax: a NaN of the warm point is not hidden
__device__ __forceinline__ double clampv(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// con_scale_i (A x~)_i of every inequality row, x~ = clamp(x, xl, xu) (a fixed variable: its value): J's
// scaled entries of the structural columns + cfix (the fixed columns' terms), as k_cons forms the row for
// get_solution.  A row per lane group of the solver's SpMV width; the lanes stride the row, then a butterfly.
template <int G>
__global__ __launch_bounds__(NT) void k_warm_rows(DV D, WarmArgs W) {
  const int nx = D.nx, ns = D.n - D.nx;
  const int gl = threadIdx.x & (G - 1);
  GROUP_LOOP(k, ns, G) {
    const int r = W.ineq[k];
    const int64_t q1 = D.J.rp[r + 1];
    double s = 0.0;
    for (int64_t q = D.J.rp[r] + gl; q < q1; q += G) {
      const int c = D.J.ci[q];
      if (c < nx) s = fma(D.J.v[q], clampv(W.wx[c], D.xl[c], D.xu[c]), s);
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, G);
    if (gl == 0) W.rows[k] = s + D.cfix[r];
  }
}

// v = lam v~ + (1 - lam) v_cold on x and s (free coordinates), y, zl on ind_lb, zu on ind_ub, where
//   x~ = clamp(x, xl, xu), s~ = clamp(row value, xl_s, xu_s), y~ = y obj_scale / con_scale,
//   zl~ = max(zl obj_scale, 0), zu~ = max(zu obj_scale, 0), and for the slack of row i (stationarity of the
//   slack coordinate, -y - zl_s + zu_s = 0) zl_s~ = max(-y~_i, 0), zu_s~ = max(y~_i, 0);
// a coordinate whose blended value is not strictly interior (x <= xl, x >= xu, z <= 0) keeps its cold value,
// so init_starting_point!'s interior assertions (solver.jl:120-123) still hold.  Each thread reads and
// writes its own coordinate of the iterate only.
__global__ __launch_bounds__(NT) void k_warm_blend(DV D, WarmArgs W) {
#pragma clang fp contract(off)
  const int n = D.n, nx = D.nx;
  const double lam = W.lam, rest = 1.0 - W.lam;
  GRID_LOOP(i, n + D.m) {
    if (i < n) {
      const bool lb = D.lbpos[i] >= 0, ub = D.ubpos[i] >= 0, slack = i >= nx;
      if (W.wx && !D.fixed[i]) {
        const double l = D.xl[i], u = D.xu[i];
        const double xt = clampv(slack ? W.rows[i - nx] : W.wx[i], l, u);
        const double v = lam * xt + rest * D.x[i];
        if (!((lb && v <= l) || (ub && v >= u))) D.x[i] = v;
      }
      double ys = 0.0;
      if (slack && W.wy) {
        const int r = W.ineq[i - nx];
        ys = W.wy[r] * W.os / W.cscale[r];
      }
      if (lb && (slack ? W.wy != nullptr : W.wzl != nullptr)) {
        const double t = slack ? -ys : W.wzl[i] * W.os;
        const double v = lam * (t < 0.0 ? 0.0 : t) + rest * D.zl[i];
        if (!(v <= 0.0)) D.zl[i] = v;
      }
      if (ub && (slack ? W.wy != nullptr : W.wzu != nullptr)) {
        const double t = slack ? ys : W.wzu[i] * W.os;
        const double v = lam * (t < 0.0 ? 0.0 : t) + rest * D.zu[i];
        if (!(v <= 0.0)) D.zu[i] = v;
      }
    } else if (W.wy) {
      const int64_t j = i - n;
      D.y[j] = lam * (W.wy[j] * W.os / W.cscale[j]) + rest * D.y[j];
    }
  }
}

}  // namespace

void MPCSolver::prepare_update(const madipm_qp& q) {
  if (plan_) return;
  QPHost& P = *H_;
  RefreshPlan R = build_refresh_plan(P, q);
  auto pl = std::make_unique<UpdatePlan>();
  pl->Ar = std::move(R.Ar);
  pl->Ac = std::move(R.Ac);
  pl->Av = std::move(R.Av);
  // ---- device side: plans + staging (the only allocations of the refresh path)
  hipStream_t s = stream_;
  auto up = [&](auto& buf, const auto& vec) {
    buf.alloc(std::max<size_t>(vec.size(), 1));
    buf.upload(vec.data(), vec.size(), s);
  };
  up(pl->tsp, R.tsp);
  up(pl->tsrc, R.tsrc);
  up(pl->jtk, R.jtk);
  up(pl->j2jt, R.j2jt);
  up(pl->hsp, R.hsp);
  up(pl->hsrc, R.hsrc);
  up(pl->hk, R.hk);
  up(pl->hdpos, R.hdpos);
  up(pl->Araw, pl->Av);
  up(pl->Hraw, P.Hv);
  pl->cscale.alloc(std::max(P.m, 1));
  pl->nJ = R.nJ;
  pl->nH = R.nH;
  MADIPM_HIP(hipStreamSynchronize(s));
  // the host passes of numeric_host read A from the plan's copy from now on
  P.Ar = pl->Ar.data();
  P.Ac = pl->Ac.data();
  P.Av = pl->Av.data();
  plan_ = std::move(pl);
}

void MPCSolver::update(const madipm_qp_update& u) {
  const double t0 = now();
  PhaseClock clk("update");
  MADIPM_REQUIRE(plan_, "madipm_solver_update: call madipm_solver_prepare_update on this solver first (it builds "
                        "the refresh plan)");
  QPHost& P = *H_;
  UpdatePlan& pl = *plan_;
  const int n = P.n;
  refresh_host_mirrors();  // after a device update: the "keep" fields are the device-installed ones
  // ---- the classification setup_host derived must hold for the merged data; checked before anything changes
  const double* lv = u.lvar ? u.lvar : P.lvar.data();
  const double* uv = u.uvar ? u.uvar : P.uvar.data();
  const double* lc = u.lcon ? u.lcon : P.lcon.data();
  const double* uc = u.ucon ? u.ucon : P.ucon.data();
  require_same_classes(P, lv, uv, lc, uc);
  clk("classification check");
  // ---- install
  auto put = [](std::vector<double>& dst, const double* src) {
    if (src && src != dst.data()) std::copy(src, src + dst.size(), dst.begin());
  };
  put(P.c, u.c);
  if (u.c0) P.c0 = *u.c0;
  put(P.Hv, u.Hvals);
  put(pl.Av, u.Avals);
  put(P.lvar, u.lvar);
  put(P.uvar, u.uvar);
  put(P.lcon, u.lcon);
  put(P.ucon, u.ucon);
  put(P.x0, u.x0);
  put(P.y0, u.y0);
  clk("copy");
  HostNumeric num;
  numeric_host(P, opt_, num);
  obj_scale_ = num.obj_scale;
  c0s_ = num.c0s;
  norm_b_ = num.norm_b;
  clk("numeric_host");
  hipStream_t s = stream_;
  auto send = [&](double* dst, const std::vector<double>& v) {
    if (!v.empty()) MADIPM_HIP(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, s));
  };
  send(rhs_.p, P.rhs);
  send(cs_.p, num.cs);
  send(gfix_.p, num.gfix);
  send(cfix_.p, num.cfix);
  send(pl.cscale.p, P.con_scale);
  if (u.Avals) send(pl.Araw.p, pl.Av);
  if (u.Hvals) send(pl.Hraw.p, P.Hv);
  // ---- matrix values on the device
  double* K0 = kkt_ == KKT_K25 ? K0_.p : nullptr;
  if (pl.nJ) {
    k_refresh_jt<<<blocks(pl.nJ), NT, 0, s>>>(pl.nJ, pl.tsp, pl.tsrc, JTci_, pl.cscale, pl.Araw, pl.jtk, JTv_, Kx_, K0);
    k_refresh_gather<<<blocks(pl.nJ), NT, 0, s>>>(pl.nJ, pl.j2jt, JTv_, Jv_);
  }
  if (pl.nH)
    k_refresh_h<<<blocks(pl.nH), NT, 0, s>>>(pl.nH, pl.hsp, pl.hsrc, P.obj_scale * P.sgn, pl.Hraw, pl.hk, Hv_, Kx_, K0);
  if (n) k_refresh_hdiag<<<blocks(n), NT, 0, s>>>(n, pl.hdpos, Hv_, Hdiag_);
  MADIPM_HIP(hipGetLastError());
  MADIPM_HIP(hipStreamSynchronize(s));
  clk("uploads + kernels");
  initialized_ = false;  // the next solve() initialises from the new x0 / y0
  start_on_device_ = false;
  cscale_host_stale_ = false;
  cscale_dev_ok_ = true;
  dev_raw_stale_ = dev_ != nullptr;  // the device route's copies of c / bounds / x0 / y0 are refreshed on its next call
  ++n_updates_;
  last_update_s_ = now() - t0;
}

// ---- the device route
enum { F_C = 1, F_H = 2, F_A = 4, F_LCON = 8, F_UCON = 16, F_LVAR = 32, F_UVAR = 64, F_X0 = 128, F_Y0 = 256 };

// Host mirrors of the raw fields a device update installed (QPHost's vectors, the plan's Avals), read
// back from the device staging; a no-op unless a device update ran since the last refresh.
void MPCSolver::refresh_host_mirrors() {
  if (!host_stale_) return;
  QPHost& P = *H_;
  DevUpdate& dv = *dev_;
  UpdatePlan& pl = *plan_;
  hipStream_t s = stream_;
  auto get = [&](int bit, std::vector<double>& dst, const double* src) {
    if ((host_stale_ & bit) && !dst.empty())
      MADIPM_HIP(hipMemcpyAsync(dst.data(), src, dst.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  };
  get(F_C, P.c, dv.c);
  get(F_H, P.Hv, pl.Hraw);
  get(F_A, pl.Av, pl.Araw);
  get(F_LCON, P.lcon, dv.lcon);
  get(F_UCON, P.ucon, dv.ucon);
  get(F_LVAR, P.lvar, dv.lvar);
  get(F_UVAR, P.uvar, dv.uvar);
  get(F_X0, P.x0, dv.x0);
  get(F_Y0, P.y0, dv.y0);
  MADIPM_HIP(hipStreamSynchronize(s));
  host_stale_ = 0;
}

void MPCSolver::get_data(double* c, double* c0, double* Hvals, double* Avals, double* lcon, double* ucon,
                         double* lvar, double* uvar, double* x0, double* y0) {
  QPHost& P = *H_;
  MADIPM_REQUIRE(!Avals || P.nnzA == 0 || plan_,
                 "madipm_solver_get_data: Avals needs madipm_solver_prepare_update first (the solver keeps no copy "
                 "of A otherwise)");
  refresh_host_mirrors();
  auto out = [](double* dst, const std::vector<double>& v) {
    if (dst) std::copy(v.begin(), v.end(), dst);
  };
  out(c, P.c);
  if (c0) *c0 = P.c0;
  out(Hvals, P.Hv);
  if (Avals && plan_) out(Avals, plan_->Av);
  out(lcon, P.lcon);
  out(ucon, P.ucon);
  out(lvar, P.lvar);
  out(uvar, P.uvar);
  out(x0, P.x0);
  out(y0, P.y0);
}

// The first device update: the lists of the host sums (from the COO copy prepare_update keeps), the
// staging of the raw fields (from the host mirrors, which are current: no device update ran yet), the
// start vectors and the scalar block.  Every device allocation of the device route happens here.
void MPCSolver::build_device_route() {
  PhaseClock clk("build_device_route");
  QPHost& P = *H_;
  const int nx = P.nx, m = P.m, n = P.n;
  auto dv = std::make_unique<DevUpdate>();
  hipStream_t s = stream_;
  const RouteLists L = build_route_lists(P);  // alive until the synchronisation below
  clk("lists");
  auto up = [&](auto& buf, const auto& vec, size_t len) {
    buf.alloc(std::max<size_t>(len, 1));
    buf.upload(vec.data(), vec.size(), s);
  };
  auto up2 = [&](DBuf<int2>& buf, const std::vector<I2>& vec) {
    buf.alloc(std::max<size_t>(vec.size(), 1));
    buf.upload(as_int2(vec), vec.size(), s);
  };
  up(dv->asp, L.asp, L.asp.size());
  up2(dv->ae, L.ae);
  up(dv->fsp, L.fsp, L.fsp.size());
  up2(dv->fe, L.fe);
  up(dv->gsp, L.gsp, L.gsp.size());
  up2(dv->ge, L.ge);
  up(dv->xsp, L.xsp, L.xsp.size());
  up2(dv->xe, L.xe);
  dv->nbf = (int)L.bfk.size();
  up(dv->bfk, L.bfk, L.bfk.size());
  up2(dv->bfrc, L.bfrc);
  up(dv->vcls, L.vcls, nx);
  up(dv->ccls, L.ccls, m);
  up(dv->ineq, P.ind_ineq, P.ns);
  up(dv->c, P.c, nx);
  up(dv->lvar, P.lvar, nx);
  up(dv->uvar, P.uvar, nx);
  up(dv->x0, P.x0, nx);
  up(dv->lcon, P.lcon, m);
  up(dv->ucon, P.ucon, m);
  up(dv->y0, P.y0, m);
  dv->x.alloc(std::max(n, 1));
  dv->xl.alloc(std::max(n, 1));
  dv->xu.alloc(std::max(n, 1));
  dv->xpre.alloc(std::max(nx, 1));
  dv->ax.alloc(std::max(m, 1));
  dv->sc.alloc(SC_LEN);
  dv->chk.alloc(4);
  MADIPM_HIP(hipEventCreateWithFlags(&dv->ev, hipEventDisableTiming));
  MADIPM_HIP(hipHostMalloc((void**)&dv->hsc, (SC_LEN + 2) * sizeof(double), hipHostMallocDefault));
  MADIPM_HIP(hipStreamSynchronize(s));
  dev_raw_stale_ = false;
  dev_ = std::move(dv);
  clk("staging + uploads");
}

void MPCSolver::update_device(const madipm_qp_update& u, hipStream_t caller) {
  const double t0 = now();
  PhaseClock clk("update_device");
  MADIPM_REQUIRE(plan_, "madipm_solver_update_device: call madipm_solver_prepare_update on this solver first (it "
                        "builds the refresh plan)");
  QPHost& P = *H_;
  UpdatePlan& pl = *plan_;
  const int nx = P.nx, m = P.m, n = P.n;
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  if (!dev_) build_device_route();
  DevUpdate& dv = *dev_;
  hipStream_t s = stream_;
  if (dev_raw_stale_) {  // a host update since: its c / bounds / x0 / y0 (Araw / Hraw it keeps itself)
    auto send = [&](double* dst, const std::vector<double>& v) {
      if (!v.empty()) MADIPM_HIP(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, s));
    };
    send(dv.c, P.c), send(dv.lvar, P.lvar), send(dv.uvar, P.uvar), send(dv.x0, P.x0);
    send(dv.lcon, P.lcon), send(dv.ucon, P.ucon), send(dv.y0, P.y0);
    dev_raw_stale_ = false;
  }
  // ---- the caller's arrays are read after the work already enqueued on its stream
  MADIPM_HIP(hipEventRecord(dv.ev, caller));
  MADIPM_HIP(hipStreamWaitEvent(s, dv.ev, 0));
  // ---- classification of the merged data, by a kernel, before anything is overwritten
  const double* lv = u.lvar ? u.lvar : dv.lvar.p;
  const double* uv = u.uvar ? u.uvar : dv.uvar.p;
  const double* lc = u.lcon ? u.lcon : dv.lcon.p;
  const double* uc = u.ucon ? u.ucon : dv.ucon.p;
  int32_t* hchk = reinterpret_cast<int32_t*>(dv.hsc + SC_LEN);
  if (u.lvar || u.uvar || u.lcon || u.ucon) {
    MADIPM_HIP(hipMemsetAsync(dv.chk.p, 0x7f, 4 * sizeof(int32_t), s));
    k_upd_check<<<blocks(std::max(nx, m)), NT, 0, s>>>(nx, m, lv, uv, lc, uc, dv.vcls, dv.ccls, dv.chk);
    MADIPM_HIP(hipGetLastError());
    MADIPM_HIP(hipMemcpyAsync(hchk, dv.chk.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MADIPM_HIP(hipStreamSynchronize(s));
    const int32_t none = 0x7f7f7f7f;
    auto fetch = [&](const double* d, int i) {
      double v = 0;
      MADIPM_HIP(hipMemcpy(&v, d + i, sizeof(double), hipMemcpyDeviceToHost));
      return v;
    };
    // the host path's order and text; the old class is the creation-time one, which the host mirrors
    // still show whatever their age
    if (hchk[0] != none) throw_kind_change(hchk[0], P.lcon[hchk[0]] == P.ucon[hchk[0]]);
    if (hchk[1] != none) {
      const int i = hchk[1];
      require_same_class("variable", i, bound_class(P.lvar[i], P.uvar[i]), bound_class(fetch(lv, i), fetch(uv, i)));
    }
    if (hchk[2] != none) {
      const int i = hchk[2];
      require_same_class("constraint", i, bound_class(P.lcon[i], P.ucon[i]), bound_class(fetch(lc, i), fetch(uc, i)));
    }
  }
  clk("classification check");
  // ---- install the given fields into the staging
  int given = 0;
  auto put = [&](int bit, double* dst, const double* src, int64_t len) {
    if (!src) return;
    given |= bit;
    if (src != dst && len) MADIPM_HIP(hipMemcpyAsync(dst, src, len * sizeof(double), hipMemcpyDeviceToDevice, s));
  };
  put(F_C, dv.c, u.c, nx);
  put(F_H, pl.Hraw, u.Hvals, nh);
  put(F_A, pl.Araw, u.Avals, na);
  put(F_LCON, dv.lcon, u.lcon, m);
  put(F_UCON, dv.ucon, u.ucon, m);
  put(F_LVAR, dv.lvar, u.lvar, nx);
  put(F_UVAR, dv.uvar, u.uvar, nx);
  put(F_X0, dv.x0, u.x0, nx);
  put(F_Y0, dv.y0, u.y0, m);
  if (u.c0) P.c0 = *u.c0;
  // ---- numeric_host, on the device
  const int scaling = opt_.scaling ? 1 : 0;
  MADIPM_HIP(hipMemsetAsync(dv.sc.p, 0, SC_LEN * sizeof(double), s));
  if (n)
    k_upd_bounds<<<blocks(n), NT, 0, s>>>(nx, n, opt_.bound_relax_factor, dv.lvar, dv.uvar, dv.lcon, dv.ucon, dv.x0,
                                          dv.ineq, fixed_, dv.xl, dv.xu, dv.xpre);
  if (m)
    k_upd_rows<<<blocks(m), NT, 0, s>>>(m, scaling, dv.asp, dv.ae, dv.fsp, dv.fe, pl.Araw, dv.xpre, dv.lcon, dv.ucon,
                                        dv.ax, pl.cscale, cfix_, rhs_, dv.sc);
  if (n)
    k_upd_start<<<blocks(n), NT, 0, s>>>(nx, n, scaling, opt_.bound_push, opt_.bound_fac, dv.xpre, dv.ax, pl.cscale,
                                         dv.ineq, fixed_, dv.xl, dv.xu, dv.x);
  if (scaling && nx) k_upd_g<<<blocks(nx), NT, 0, s>>>(nx, P.sgn, dv.gsp, dv.ge, dv.c, pl.Hraw, dv.x, dv.sc);
  k_upd_scalars<<<1, 64, 0, s>>>(scaling, P.sgn, P.c0, dv.nbf, dv.bfk, dv.bfrc, pl.Hraw, dv.x, dv.sc);
  if (n) k_upd_cs_gfix<<<blocks(n), NT, 0, s>>>(nx, n, dv.xsp, dv.xe, dv.c, pl.Hraw, dv.x, dv.sc, cs_, gfix_);
  // ---- matrix values, as the host route
  double* K0 = kkt_ == KKT_K25 ? K0_.p : nullptr;
  if (pl.nJ) {
    k_refresh_jt<<<blocks(pl.nJ), NT, 0, s>>>(pl.nJ, pl.tsp, pl.tsrc, JTci_, pl.cscale, pl.Araw, pl.jtk, JTv_, Kx_, K0);
    k_refresh_gather<<<blocks(pl.nJ), NT, 0, s>>>(pl.nJ, pl.j2jt, JTv_, Jv_);
  }
  if (pl.nH)
    k_refresh_h_dev<<<blocks(pl.nH), NT, 0, s>>>(pl.nH, pl.hsp, pl.hsrc, dv.sc, pl.Hraw, pl.hk, Hv_, Kx_, K0);
  if (n) k_refresh_hdiag<<<blocks(n), NT, 0, s>>>(n, pl.hdpos, Hv_, Hdiag_);
  MADIPM_HIP(hipGetLastError());
  // ---- the host's scalars, read with the final synchronisation
  MADIPM_HIP(hipMemcpyAsync(dv.hsc, dv.sc.p, SC_LEN * sizeof(double), hipMemcpyDeviceToHost, s));
  MADIPM_HIP(hipStreamSynchronize(s));
  clk("copies + kernels");
  P.obj_scale = obj_scale_ = dv.hsc[SC_OBJ];
  c0s_ = dv.hsc[SC_C0S];
  norm_b_ = dv.hsc[SC_NORMB];
  host_stale_ |= given;
  start_on_device_ = true;
  cscale_host_stale_ = true;
  cscale_dev_ok_ = true;
  initialized_ = false;
  ++n_updates_;
  last_update_s_ = now() - t0;
}

// con_scale on the device: the plan's once an update has written it, else a copy of the host's
const double* MPCSolver::device_con_scale() {
  if (plan_ && cscale_dev_ok_) return plan_->cscale.p;
  if (!sol_cs_.p) {
    sol_cs_.alloc(std::max(m_, 1));
    sol_cs_.upload(H_->con_scale.data(), H_->con_scale.size(), stream_);
  }
  return sol_cs_.p;
}

void MPCSolver::get_solution_device(double* x, double* y, double* zl, double* zu, double* cons, hipStream_t caller) {
  hipStream_t s = stream_;
  if (!sol_ev_[0]) {
    MADIPM_HIP(hipEventCreateWithFlags(&sol_ev_[0], hipEventDisableTiming));
    MADIPM_HIP(hipEventCreateWithFlags(&sol_ev_[1], hipEventDisableTiming));
    sol_ax_.alloc(std::max(m_, 1));
  }
  const double* cscale = device_con_scale();
  // the outputs are written after the caller's earlier work on them, and read by its later work
  MADIPM_HIP(hipEventRecord(sol_ev_[0], caller));
  MADIPM_HIP(hipStreamWaitEvent(s, sol_ev_[0], 0));
  if (cons && m_)
    k_cons<<<(unsigned)((m_ + NT / 64 - 1) / (NT / 64)), NT, 0, s>>>(Jrp_, Jci_, Jv_, x_, cfix_, m_, nx_, sol_ax_);
  if (std::max(nx_, m_))
    k_unscale<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(nx_, m_, obj_scale_, x_, y_, zl_, zu_, sol_ax_, cscale, x, y,
                                                        zl, zu, cons);
  MADIPM_HIP(hipGetLastError());
  MADIPM_HIP(hipEventRecord(sol_ev_[1], s));
  MADIPM_HIP(hipStreamWaitEvent(caller, sol_ev_[1], 0));
}

// Launch helpers (the DV view is rebuilt from member buffers; cheap, host-only)
#define DV_ARGS                                                                                         \
  DV D;                                                                                                 \
  D.n = n_;                                                                                             \
  D.m = m_;                                                                                             \
  D.nx = nx_;                                                                                           \
  D.nlb = nlb_;                                                                                         \
  D.nub = nub_;                                                                                         \
  D.x = x_;                                                                                             \
  D.xl = xl_;                                                                                           \
  D.xu = xu_;                                                                                           \
  D.zl = zl_;                                                                                           \
  D.zu = zu_;                                                                                           \
  D.f = f_;                                                                                             \
  D.jacl = jacl_;                                                                                       \
  D.c = c_;                                                                                             \
  D.y = y_;                                                                                             \
  D.rhs = rhs_;                                                                                         \
  D.pr_diag = pr_diag_;                                                                                 \
  D.l_diag = l_diag_;                                                                                   \
  D.u_diag = u_diag_;                                                                                   \
  D.l_lower = l_lower_;                                                                                 \
  D.u_lower = u_lower_;                                                                                 \
  D.d = d_;                                                                                             \
  D.p = p_;                                                                                             \
  D.corr_lb = corr_lb_;                                                                                 \
  D.corr_ub = corr_ub_;                                                                                 \
  D.Kx = Kx_;                                                                                           \
  D.diag_pos = diag_pos_;                                                                               \
  D.Hdiag = Hdiag_;                                                                                     \
  D.cs = cs_;                                                                                           \
  D.gfix = gfix_;                                                                                       \
  D.cfix = cfix_;                                                                                       \
  D.ind_lb = ind_lb_;                                                                                   \
  D.ind_ub = ind_ub_;                                                                                   \
  D.lbpos = lbpos_;                                                                                     \
  D.ubpos = ubpos_;                                                                                     \
  D.fixed = fixed_;                                                                                     \
  D.H = DCsr{Hrp_, Hci_, Hv_};                                                                          \
  D.J = DCsr{Jrp_, Jci_, Jv_};                                                                          \
  D.JT = DCsr{JTrp_, JTci_, JTv_};                                                                      \
  D.part = part_;                                                                                       \
  D.st = st_;                                                                                           \
  D.kkt = kkt_;                                                                                         \
  D.sk = sk_;                                                                                           \
  D.Krow = Krow_;                                                                                       \
  D.Kcol = Kcol_;                                                                                       \
  D.K0 = K0_;                                                                                           \
  D.nnzK = nnzK_;                                                                                       \
  D.Dinv = Dinv_;                                                                                       \
  D.bufm = bufm_;                                                                                       \
  D.cpp = cpp_;                                                                                         \
  D.cprod = reinterpret_cast<const int2*>(cprod_.p);                                                    \
  D.Cx = Cx_;                                                                                           \
  D.nnzC = nnzC_;

// launch a GROUP_LOOP SpMV kernel with the problem's lane-group width
#define SPMV_LAUNCH(kern, grid, strm, ...)                                        \
  do {                                                                            \
    switch (spmv_g_) {                                                            \
      case 4: kern<4><<<(grid), NT, 0, (strm)>>>(__VA_ARGS__); break;             \
      case 8: kern<8><<<(grid), NT, 0, (strm)>>>(__VA_ARGS__); break;             \
      case 16: kern<16><<<(grid), NT, 0, (strm)>>>(__VA_ARGS__); break;           \
      case 32: kern<32><<<(grid), NT, 0, (strm)>>>(__VA_ARGS__); break;           \
      default: kern<64><<<(grid), NT, 0, (strm)>>>(__VA_ARGS__); break;           \
    }                                                                             \
  } while (0)

// ---- warm start
static void check_weight(double w) {
  MADIPM_REQUIRE(w > 0.0 && w < 1.0, "warm start: weight must be in the open interval (0, 1), got " + std::to_string(w));
}

// the buffers, once (the first call that sets a point); nothing of the current point is touched
WarmStart& MPCSolver::warm_buffers() {
  if (!warm_) {
    auto w = std::make_unique<WarmStart>();
    w->x.alloc(std::max(nx_, 1));
    w->y.alloc(std::max(m_, 1));
    w->zl.alloc(std::max(nx_, 1));
    w->zu.alloc(std::max(nx_, 1));
    w->rows.alloc(std::max(ns_, 1));
    w->ineq.alloc(std::max(ns_, 1));
    w->ineq.upload(H_->ind_ineq.data(), H_->ind_ineq.size(), stream_);
    MADIPM_HIP(hipEventCreateWithFlags(&w->ev[0], hipEventDisableTiming));
    MADIPM_HIP(hipEventCreateWithFlags(&w->ev[1], hipEventDisableTiming));
    device_con_scale();  // its one-off device copy (a solver without an update) now, not in initialize()
    MADIPM_HIP(hipStreamSynchronize(stream_));
    warm_ = std::move(w);
  }
  return *warm_;
}

void MPCSolver::set_warm_start(const double* x, const double* y, const double* zl, const double* zu, double weight,
                               bool device, hipStream_t caller) {
  check_weight(weight);
  MADIPM_REQUIRE(x || y || zl || zu, "warm start: all four of x, y, zl, zu are NULL (madipm_solver_clear_warm_start "
                                     "removes a warm point)");
  WarmStart& w = warm_buffers();
  hipStream_t s = stream_;
  const auto kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (device) {  // the caller's arrays are read after the work already enqueued on its stream
    MADIPM_HIP(hipEventRecord(w.ev[0], caller));
    MADIPM_HIP(hipStreamWaitEvent(s, w.ev[0], 0));
  }
  const double* src[4] = {x, y, zl, zu};
  double* dst[4] = {w.x.p, w.y.p, w.zl.p, w.zu.p};
  const int64_t len[4] = {nx_, m_, nx_, nx_};
  for (int k = 0; k < 4; ++k) {
    w.has[k] = src[k] != nullptr;
    if (src[k] && len[k]) MADIPM_HIP(hipMemcpyAsync(dst[k], src[k], len[k] * sizeof(double), kind, s));
  }
  if (device) {  // the caller's later work on its stream (overwriting the arrays) comes after the copies
    MADIPM_HIP(hipEventRecord(w.ev[1], s));
    MADIPM_HIP(hipStreamWaitEvent(caller, w.ev[1], 0));
  } else {
    MADIPM_HIP(hipStreamSynchronize(s));  // host arrays are read during the call only
  }
  w.weight = weight;
  w.active = true;
  initialized_ = false;
}

void MPCSolver::warm_start_last(double weight) {
  check_weight(weight);
  MADIPM_REQUIRE(solved_, "madipm_solver_warm_start_last: no solve has run on this solver yet");
  WarmStart& w = warm_buffers();
  const double* cscale = device_con_scale();
  if (std::max(nx_, m_))
    k_unscale<<<blocks(std::max(nx_, m_)), NT, 0, stream_>>>(nx_, m_, obj_scale_, x_, y_, zl_, zu_, nullptr, cscale, w.x,
                                                              w.y, w.zl, w.zu, nullptr);
  MADIPM_HIP(hipGetLastError());
  for (bool& h : w.has) h = true;
  w.weight = weight;
  w.active = true;
  initialized_ = false;
}

void MPCSolver::clear_warm_start() {
  if (warm_ && warm_->active) initialized_ = false;
  if (warm_) warm_->active = false;
}

void MPCSolver::warm_info(int32_t* active, double* weight, int64_t* n_warm_inits) const {
  const bool on = warm_ && warm_->active;
  if (active) *active = on ? 1 : 0;
  if (weight) *weight = on ? warm_->weight : 0.0;
  if (n_warm_inits) *n_warm_inits = n_warm_inits_;
}

// initialize()'s warm part, after init_starting_point(): the blend, then evaluate_model! at the blended
// point (the cold path leaves the initial point's f, c and objective in place; the first termination test of
// a warm solve sees the blended point's residuals)
void MPCSolver::warm_blend() {
  DV_ARGS;
  hipStream_t s = stream_;
  WarmStart& w = *warm_;
  WarmArgs W{w.has[0] ? w.x.p : nullptr, w.has[1] ? w.y.p : nullptr, w.has[2] ? w.zl.p : nullptr,
             w.has[3] ? w.zu.p : nullptr, device_con_scale(), w.ineq.p, w.rows.p, w.weight, obj_scale_};
  if (W.wx && ns_) SPMV_LAUNCH(k_warm_rows, spmv_blocks(ns_), s, D, W);
  const int nb = blocks(n_ + m_);
  k_warm_blend<<<nb, NT, 0, s>>>(D, W);
  SPMV_LAUNCH(k_eval, nb, s, D, 0);
  launch_reduce_final(FIN_EVAL, nb);
  MADIPM_HIP(hipGetLastError());
  ++n_warm_inits_;
}

void MPCSolver::kkt_diag(double dw, double dc) {
  DV_ARGS;
  k_diag<<<blocks(n_ + m_), NT, 0, stream_>>>(D, dw, dc, fact_reset());
}

// set_aug_diagonal_reg! + build_kkt! of the chosen formulation (values consumed by the LDL^T)
void MPCSolver::assemble_kkt(double dw, double dc, bool diag_done) {
  DV_ARGS;
  if (!diag_done) kkt_diag(dw, dc);
  if (kkt_ == KKT_K25) k_k25_scale<<<blocks(nnzK_), NT, 0, stream_>>>(D);
  if (kkt_ == KKT_NORMAL) k_normal_asm<<<blocks(nnzC_), NT, 0, stream_>>>(D);
}

const double* MPCSolver::kvals() const { return kkt_ == KKT_NORMAL ? Cx_.p : Kx_.p; }

// factorize! between two pooled timing events (cnt.linear_solver_time, MadNLP.factorize_wrapper!);
// the pool grows only when a solve needs more pairs than any earlier one did
void MPCSolver::timed_factorize() {
  ldl_->factorize_async(kvals(), stream_);
  // the next k_rhs stamps the factorisation's end (an asynchronous tail stamps its own)
  fact_end_pending_ = ldl_->lazy_inertia && !ldl_->tail_async();
}

// the status block the kernel right before a factorisation resets (LinSolver::ext_reset), or nullptr
LDLStatus* MPCSolver::fact_reset() const { return ldl_->ext_reset ? &st_.p->ldl_status : nullptr; }
// the status block the first kernel after a factorisation stamps (LinSolver::lazy_inertia), or nullptr
LDLStatus* MPCSolver::take_fact_end() {
  LDLStatus* p = fact_end_pending_ ? &st_.p->ldl_status : nullptr;
  fact_end_pending_ = false;
  return p;
}

void MPCSolver::factor_enqueue(double dw, double dc) {
  assemble_kkt(dw, dc);
  timed_factorize();
}

// MadNLP.solve!(kkt, d) between reduce_rhs! (k_rhs) and finish_aug_solve! (k_residual)
void MPCSolver::kkt_solve() {
  DV_ARGS;
  if (kkt_ == KKT_NORMAL) {
    SPMV_LAUNCH(k_normal_rhs, spmv_blocks(m_), stream_, D);
    ldl_->solve_async(bufm_.p, stream_);
    SPMV_LAUNCH(k_normal_back, spmv_blocks(n_ + m_), stream_, D);
  } else {
    ldl_->solve_async(d_.p, stream_);
    if (kkt_ == KKT_K25) k_k25_unscale<<<blocks(n_), NT, 0, stream_>>>(D);
  }
}

void MPCSolver::launch_reduce_final(int kind, int nb, int amode, int nb_eval, LDLStatus* rs, bool publish) {
  DV_ARGS;
  FinParams P{nb, 0, 0, 0, 0, 0, nb_eval, rs};
  if (publish) {
    P.host = hst_;
    P.hseq = hseq_;
    P.seq = ++pub_seq_;
  }
  if (nb_eval > 0) P.c = c0s_;
  if (amode >= 0) {
    P.alpha_mode = amode;
    P.nb_alpha = blocks(std::max(nlb_, nub_));
  }
  if (kind == FIN_MU_PRED) {
    P.a = (double)(nlb_ + nub_);
    P.b = H_->has_ineq ? 1.0 : 0.0;
    P.c = opt_.mu_min;
  } else if (kind == FIN_MU_FULL) {
    P.a = (double)(nlb_ + nub_);
    P.b = opt_.step_tau;
  } else if (kind == FIN_MU_GONDZIO) {
    P.a = (double)(nlb_ + nub_);
  } else if (kind == FIN_EVAL) {
    P.a = c0s_;
  } else if (kind == FIN_RESID) {
    P.a = opt_.check_residual ? opt_.tol_linear_solve : 0.0;
  }
  if (fdbg_.p) P.dbg = fdbg_.p + 8 * (fdbg_n_++ % kFinDbg);
  launch_final(D, kind, P, stream_);
}

// solve_system! (linear_solver.jl:19-44): rhs (mode) -> LDL^T solve -> finish + residual
void MPCSolver::solve_system(int mode, double mu, int reset, int amode, double atau, int mu_nb) {
  DV_ARGS;
  const int nb = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_);
  DevState* host = nullptr;
  uint32_t seq = 0;
  bool late = false;  // published by the residual's finaliser instead: after the solve joined the
                      // factorisation's asynchronous tail, whose pivot check the state carries
  if (publish_next_ && ldl_->tail_async()) {
    late = true;
    publish_next_ = false;
  } else if (publish_next_) {  // read_state() folded into this launch
    host = hst_;
    seq = ++pub_seq_;
    publish_next_ = false;
  }
  MuFold mf{0, 0.0, 0.0, 0.0};
  if (mu_nb > 0) mf = MuFold{mu_nb, (double)(nlb_ + nub_), H_->has_ineq ? 1.0 : 0.0, opt_.mu_min};
  k_rhs<<<nb, NT, 0, stream_>>>(D, mode, mu, reset, host, hseq_, seq, mf, take_fact_end());
  kkt_solve();
  // amode >= 0: the step test of that mode on the new direction runs in the same launch (its own
  // blocks) and is finalised with the residual
  const int nbz = amode >= 0 ? blocks(std::max(nlb_, nub_)) : 0;
  SPMV_LAUNCH(k_residual, nbs + nbz, stream_, D, del_w_, del_c_, nbs, amode, atau);
  launch_reduce_final(FIN_RESID, nbs, amode, 0, nullptr, late);
}

// gondzio_correction_direction! (solver.jl:245-298): host-controlled loop, one read-back per solve
void MPCSolver::gondzio() {
  DV_ARGS;
  hipStream_t s = stream_;
  const double delta = 0.1, bmin = 0.1, bmax = 10.0, tau = 0.995;
  const int nbz = blocks(std::max(nlb_, nub_));
  auto ftb = [&](double& ap, double& ad) {  // get_fraction_to_boundary_step(solver, tau)
    k_alpha<<<nbz, NT, 0, s>>>(D, ALPHA_GONDZIO, tau, 0);
    FinParams P{nbz, ALPHA_GONDZIO, 0, 0, 0, 0, 0};
    launch_final(D, FIN_ALPHA, P, s);
    read_state();
    wait_state();
    ap = hst_->alpha_aff_p;
    ad = hst_->alpha_aff_d;
  };
  double ap, ad;
  ftb(ap, ad);
  for (int nc = 0; nc < opt_.max_ncorr; ++nc) {
    const double tap = std::min(ap + delta, 1.0), tad = std::min(ad + delta, 1.0);
    k_mu<<<nbz, NT, 0, s>>>(D, 0, tap, tad);
    launch_reduce_final(FIN_MU_GONDZIO, nbz);
    read_state();
    wait_state();
    const double ga = hst_->mu_aff, g = hst_->mu_curr;
    const double mu = (ga / g) * (ga / g) * ga;  // Eq. (12)
    k_extra_corr<<<nbz, NT, 0, s>>>(D, tap, tad, bmin * mu, bmax * mu);
    k_copy<<<blocks(L_), NT, 0, s>>>(dsave_, d_, L_);  // copyto!(dp, d.values) happens before the solve
    solve_system(RHS_GONDZIO, mu);
    double hap, had;
    ftb(hap, had);
    if (hap < 1.005 * ap || had < 1.005 * ad) {
      k_copy<<<blocks(L_), NT, 0, s>>>(d_, dsave_, L_);
      break;
    }
    ap = hap;
    ad = had;
  }
}

void MPCSolver::read_state() {
  k_publish<<<1, 64, 0, stream_>>>(st_, hst_, hseq_, ++pub_seq_);
  MADIPM_HIP(hipGetLastError());
}

// Host spin on the publication counter (no event record in the stream: each one costs a ~5 us
// bubble between kernels); bounded, and a failed stream surfaces as its HIP error.  The stream is
// queried only once a wait has lasted 2 ms: a query puts a marker into the stream, another ~6 us
// bubble at the point the host had enqueued to (r6_x: before the predictor's k_rhs and k_apply)
void MPCSolver::wait_state() {
  const double t0 = now();
  for (uint64_t spin = 0;; ++spin) {
    if (__atomic_load_n(hseq_, __ATOMIC_ACQUIRE) == pub_seq_) return;
    if ((spin & 1023) == 1023 && now() - t0 > 2e-3) {
      const hipError_t e = hipStreamQuery(stream_);
      if (e != hipSuccess && e != hipErrorNotReady) MADIPM_HIP(e);
      if (e == hipSuccess && __atomic_load_n(hseq_, __ATOMIC_ACQUIRE) != pub_seq_)
        throw Error("state publication lost (stream idle, counter not updated)", -5);
      if (now() - t0 > 600.0) throw Error("state publication: timed out", -5);
    }
  }
}

void MPCSolver::init_starting_point() {
  DV_ARGS;
  const int nb = blocks(n_ + m_), nbn = blocks(n_);
  hipStream_t s = stream_;
  k_init_kkt<<<nb, NT, 0, s>>>(D, del_w_, del_c_, fact_reset());
  if (kkt_ == KKT_NORMAL) k_normal_asm<<<blocks(nnzC_), NT, 0, s>>>(D);
  if (kkt_ == KKT_K25) k_k25_scale<<<blocks(nnzK_), NT, 0, s>>>(D);  // s = 1: K2.5 = K2
  timed_factorize();
  // init factorization: the reference does not retry here; a solve with an unfactorized LDL^T is a
  // step-computation failure (oracle/mpc.py solve_system)
  if (ldl_->status(s) != 0) {
    exception_ = MADIPM_EXC_UNFACTORIZED;
    throw Error("init_starting_point!: KKT factorization failed", -4);
  }
  // Step 1: least-squares primal correction
  k_rhs<<<nb, NT, 0, s>>>(D, RHS_INIT_PRIMAL, 0.0, 0, nullptr, nullptr, 0, MuFold{0, 0.0, 0.0, 0.0}, take_fact_end());
  kkt_solve();
  SPMV_LAUNCH(k_residual, nb, s, D, del_w_, del_c_, nb, -1, 1.0);
  launch_reduce_final(FIN_RESID, nb);
  k_axpy_x<<<nbn, NT, 0, s>>>(D);
  // Step 2: dual least squares
  k_rhs<<<nb, NT, 0, s>>>(D, RHS_INIT_DUAL, 0.0, 0, nullptr, nullptr, 0, MuFold{0, 0.0, 0.0, 0.0}, take_fact_end());
  kkt_solve();
  SPMV_LAUNCH(k_residual, nb, s, D, del_w_, del_c_, nb, -1, 1.0);
  launch_reduce_final(FIN_RESID, nb);
  k_copy_y<<<blocks(m_), NT, 0, s>>>(D);
  // Step 3: bound multipliers and shifts
  k_zinit<<<nbn, NT, 0, s>>>(D);
  launch_reduce_final(FIN_ZINIT, nbn);
  k_zshift1<<<nbn, NT, 0, s>>>(D);
  launch_reduce_final(FIN_ZSHIFT1, nbn);
  k_zshift2<<<nbn, NT, 0, s>>>(D, opt_.bound_fac);
  launch_reduce_final(FIN_ZSHIFT2, nbn);
  read_state();
  wait_state();
  if (hst_->nan_flag) {
    exception_ = MADIPM_EXC_SOLVE;
    throw Error("SolveException in init_starting_point!", -4);
  }
  MADIPM_REQUIRE(hst_->init_viol == 0.0, "init_starting_point!: interior assertion failed");
}

void MPCSolver::initialize() {
  DV_ARGS;
  hipStream_t s = stream_;
  {  // restart from the problem's initial point (solve! always restarts)
    const QPHost& P = *H_;
    if (start_on_device_) {  // the last update was a device update: its start vectors never left the device
      const DevUpdate& dv = *dev_;
      const auto d2d = hipMemcpyDeviceToDevice;
      if (n_) {
        MADIPM_HIP(hipMemcpyAsync(x_.p, dv.x.p, sizeof(double) * n_, d2d, s));
        MADIPM_HIP(hipMemcpyAsync(xl_.p, dv.xl.p, sizeof(double) * n_, d2d, s));
        MADIPM_HIP(hipMemcpyAsync(xu_.p, dv.xu.p, sizeof(double) * n_, d2d, s));
      }
      if (m_) MADIPM_HIP(hipMemcpyAsync(y_.p, dv.y0.p, sizeof(double) * m_, d2d, s));
    } else {
      MADIPM_HIP(hipMemcpyAsync(x_.p, P.x.data(), sizeof(double) * n_, hipMemcpyHostToDevice, s));
      MADIPM_HIP(hipMemcpyAsync(xl_.p, P.xl.data(), sizeof(double) * n_, hipMemcpyHostToDevice, s));
      MADIPM_HIP(hipMemcpyAsync(xu_.p, P.xu.data(), sizeof(double) * n_, hipMemcpyHostToDevice, s));
      if (m_) MADIPM_HIP(hipMemcpyAsync(y_.p, P.y.data(), sizeof(double) * m_, hipMemcpyHostToDevice, s));
    }
    zl_.zero(s);
    zu_.zero(s);
    d_.zero(s);
    p_.zero(s);
  }
  fs0_ = ldl_->fact_seconds(s);
  // init_regularization! (kernels.jl:364-392)
  switch (opt_.regularization) {
    case 0: del_w_ = 1.0; del_c_ = 0.0; break;
    case 1: del_w_ = 1.0; del_c_ = opt_.delta_d; break;
    default:
      adapt_dp_ = opt_.delta_p;
      adapt_dd_ = opt_.delta_d;
      adapt_dmin_ = opt_.delta_min;
      del_w_ = 1.0;
      del_c_ = opt_.delta_d;
  }
  k_set_mu<<<1, 1, 0, s>>>(st_, 0.0);
  // callbacks at the initial point (solver.jl:166-170)
  const int nb = blocks(n_ + m_);
  SPMV_LAUNCH(k_eval, nb, s, D, 0);
  launch_reduce_final(FIN_EVAL, nb);
  // norm_c = ||primal(f)||_inf (solver.jl:174)
  std::vector<double> fh(n_);
  if (n_) MADIPM_HIP(hipMemcpyAsync(fh.data(), f_.p, sizeof(double) * n_, hipMemcpyDeviceToHost, s));
  MADIPM_HIP(hipStreamSynchronize(s));
  norm_c_ = 0;
  for (double v : fh) norm_c_ = std::max(norm_c_, std::fabs(v));
  init_starting_point();
  if (warm_ && warm_->active) warm_blend();
  k_set_mu<<<1, 1, 0, s>>>(st_, opt_.mu_init);  // solver.jl:179
  k_jtprod<<<blocks(n_), NT, 0, s>>>(D);        // solver.jl:187
  best_compl_ = INF;
  status_ = MADIPM_REGULAR;
  k_ = 0;
  eval_pending_ = false;
}

void MPCSolver::initialize_public() {
  const double t0 = now();
  initialize();
  MADIPM_HIP(hipStreamSynchronize(stream_));
  t_init_ += now() - t0;
  initialized_ = true;
}

// prediction_step! (solver.jl:230-237) + mehrotra_correction_direction! (solver.jl:239-243)
void MPCSolver::directions(bool redo, bool fuse_step) {
  DV_ARGS;
  hipStream_t s = stream_;
  const int nbz = blocks(std::max(nlb_, nub_));
  // the affine step test (get_alpha_max_primal/dual with tau = 1) is finalised with the residual
  solve_system(RHS_PRED, 0.0, redo ? 2 : 1, ALPHA_PRED, 1.0);
  // mu_affine at (alpha_aff_p, alpha_aff_d) and mu_curr; the alphas never leave the device.  The
  // barrier update (FIN_MU_PRED) is finalised inside the corrector's k_rhs (no separate launch).
  k_mu<<<nbz, NT, 0, s>>>(D, 1, 0.0, 0.0);
  double tau = 1.0;
  const int amode = fuse_step ? step_alpha_mode(tau) : -1;
  solve_system(RHS_CORR, 0.0, 0, amode, tau, nbz);
}

// the step test update_step_size! runs for the configured rule (its mode and tau parameter)
int MPCSolver::step_alpha_mode(double& tau) const {
  if (opt_.step_rule == 2) {
    tau = 1.0;
    return ALPHA_MEHROTRA;
  }
  tau = opt_.step_tau;
  return opt_.step_rule == 0 ? ALPHA_CONSERVATIVE : ALPHA_ADAPTIVE;
}

// update_step_size! (solver.jl:304-307)
// fused: the corrector solve already ran the step test (directions(.., true))
void MPCSolver::step_size(bool fused) {
  DV_ARGS;
  hipStream_t s = stream_;
  const int nbz = blocks(std::max(nlb_, nub_));
  double tau = 1.0;
  const int mode = step_alpha_mode(tau);
  if (!fused) {
    k_alpha<<<nbz, NT, 0, s>>>(D, mode, tau, 0);
    FinParams P{nbz, mode, 0, 0, 0, 0, 0};
    launch_final(D, FIN_ALPHA, P, s);
  }
  if (opt_.step_rule == 2) {
    k_mu<<<nbz, NT, 0, s>>>(D, 1, 0.0, 0.0);
    launch_reduce_final(FIN_MU_FULL, nbz);
  }
}

int MPCSolver::solve(madipm_stats* stats) {
  DV_ARGS;
  hipStream_t s = stream_;
  trace_.clear();
  point_ok_ = false;
  int status = MADIPM_REGULAR;
  exception_ = MADIPM_EXC_NONE;
  double tstart = now();
  try {
    if (!initialized_) initialize_public();
    initialized_ = false;
    tstart = now();  // solver.jl:181
    const int nb = blocks(n_ + m_);
    while (true) {
      // ---- update_termination_criteria! (+ speculative factorization of this iteration)
      const double del_w_print = del_w_;
      // factorize_system! = update_regularization! + factorize_regularized_system!
      double save_w = del_w_, save_c = del_c_;
      switch (opt_.regularization) {
        case 0: del_w_ = 0.0; del_c_ = 0.0; break;
        case 1: del_w_ = opt_.delta_p; del_c_ = opt_.delta_d; break;
        default:
          adapt_dp_ = std::max(adapt_dp_ / 10.0, adapt_dmin_);
          adapt_dd_ = std::min(adapt_dd_ / 10.0, -adapt_dmin_);
          del_w_ = adapt_dp_;
          del_c_ = adapt_dd_;
      }
      // first trial enqueued together with the state read-back: ONE sync per iteration.  At
      // k >= max_iter the termination test ends the solve whatever it finds: nothing to speculate.
      const bool last = k_ >= opt_.max_iter;
      k_term<<<nb, NT, 0, s>>>(D, last ? 0 : 1, del_w_, del_c_);
      // the termination test's state is published by its own finaliser: the host decides while the GPU
      // runs this iteration's (speculative) factorisation, and a converged solve enqueues no directions
      launch_reduce_final(FIN_TERM, nb, -1, eval_pending_ ? spmv_blocks(n_ + m_) : 0, last ? nullptr : fact_reset(),
                          true);
      eval_pending_ = false;
      // the factorisation is enqueued before the host reads the termination test (speculatively),
      // except when the previous iteration's residuals were within spec_near_ x tol: there the solve
      // is likely to stop now, and a converged test would leave the whole factorisation as waste
      // (~0.3 ms on ex10) where holding it back costs one host turn-around (~20 us) otherwise
      const bool hold = !last && spec_near_ > 0 && k_ > 0 &&
                        std::max(inf_pr_, std::max(inf_du_, inf_compl_)) <= spec_near_ * opt_.tol;
      if (!last && !hold) {
        assemble_kkt(del_w_, del_c_, true);
        timed_factorize();
      }
      wait_state();
      const DevState h = *hst_;
      last_ = h;
      if (h.nan_flag) {
        // SolveException in the previous iteration's solve_system! (linear_solver.jl:40-41): the
        // reference throws before apply_step!, so k_apply skipped the step on the device and the
        // iteration is not counted (cnt.k += 1 is inside apply_step!, solver.jl:316).  It throws the
        // TYPE MadNLP.SolveException, which is not `isa MadNLP.LinearSolverException`, so solve!'s
        // catch-all maps it to INTERNAL_ERROR (solver.jl:398-403)
        status = MADIPM_INTERNAL_ERROR;
        exception_ = MADIPM_EXC_SOLVE;
        if (k_ > 0) --k_;
        break;
      }
      const double dobj = h.dobj;
      inf_pr_ = h.inf_pr_raw / std::max(1.0, norm_b_);
      inf_du_ = h.inf_du_raw / std::max(1.0, norm_c_);
      inf_compl_ = h.inf_compl_raw / std::max(1.0, norm_c_);
      best_compl_ = std::min(best_compl_, inf_compl_);
      const double obj_val = h.obj_val;
      madipm_iter_trace tr{k_, obj_val / obj_scale_, inf_pr_, inf_du_, inf_compl_, h.mu, h.alpha_p, h.alpha_d,
                           del_w_print, k_ == 0 ? 0.0 : h.dx_inf, h.max_res_ratio};
      trace_.push_back(tr);
      if (opt_.print_level > 0) {
        if (k_ % 10 == 0) std::printf("iter    objective    inf_pr   inf_du lg(mu)  ||d||  lg(rg) alpha_du alpha_pr\n");
        char rg[16];
        if (del_w_print == 0)
          std::snprintf(rg, sizeof rg, "   - ");
        else
          std::snprintf(rg, sizeof rg, "%5.1f", std::log10(del_w_print));
        std::printf("%4d % 10.7e %6.2e %6.2e %5.1f %6.2e %s %6.2e %6.2e\n", k_, obj_val / obj_scale_, inf_pr_,
                    inf_du_, std::log10(h.mu), tr.dx_inf, rg, h.alpha_d, h.alpha_p);
      }
      if (std::max(inf_pr_, std::max(inf_du_, inf_compl_)) <= opt_.tol) {
        status = MADIPM_SOLVE_SUCCEEDED;
      } else if (inf_compl_ > opt_.divergence_tol * best_compl_ && dobj > std::max(10.0 * std::fabs(obj_val), 1.0)) {
        status = MADIPM_INFEASIBLE_PROBLEM_DETECTED;
      } else if (obj_val < -opt_.divergence_tol * std::max(std::max(10.0, std::fabs(dobj)), 1.0)) {
        status = MADIPM_DIVERGING_ITERATES;
      } else if (k_ >= opt_.max_iter) {
        status = MADIPM_MAXIMUM_ITERATIONS_EXCEEDED;
      } else if (now() - tstart >= opt_.max_wall_time) {
        status = MADIPM_MAXIMUM_WALLTIME_EXCEEDED;
      }
      if (status != MADIPM_REGULAR) {
        del_w_ = save_w;
        del_c_ = save_c;
        break;
      }
      // speculation: this iteration's directions (prediction_step!, mehrotra_correction_direction!,
      // update_step_size!) are enqueued BEFORE the host reads the factorisation status, so the GPU is
      // busy while the host decides; they write scratch vectors and step scalars only (the iterate is
      // updated by k_apply, enqueued after the decision) and are recomputed after a failed
      // factorisation's retries.  Gondzio's loop synchronises internally: not speculated.
      if (hold) {
        assemble_kkt(del_w_, del_c_, true);
        timed_factorize();
      }
      const bool spec = opt_.max_ncorr == 0;
      if (spec) {  // the state read-back (with the factorisation status) rides on the predictor's first launch
        publish_next_ = true;
        directions(false, true);
        step_size(true);
      } else {
        ldl_->join(s);  // the factorisation's asynchronous tail (its pivot check) before the read-back
        read_state();
      }
      wait_state();
      const int frc = ldl_->status(s, false);
      if (frc != 0) {  // remaining trials of factorize_regularized_system!
        bool ok = false;
        for (int trial = 1; trial < 3 && !ok; ++trial) {
          del_w_ *= 100.0;
          del_c_ *= 100.0;
          factor_enqueue(del_w_, del_c_);
          ok = ldl_->status(s) == 0;
        }
        if (!ok) {  // every trial failed: prediction_step!'s solve would use an unfactorized LDL^T,
          // which the linear solver refuses with an exception that is no LinearSolverException
          // (LDLFactorizations' ldiv! [EXT]) -> solve!'s catch-all: INTERNAL_ERROR (solver.jl:398-403)
          del_w_ *= 100.0;
          del_c_ *= 100.0;
          status = MADIPM_INTERNAL_ERROR;
          exception_ = MADIPM_EXC_UNFACTORIZED;
          break;
        }
        if (spec) {  // the speculated directions used the failed factor: recompute
          directions(true, true);
          step_size(true);
        }
      }
      if (!spec) {
        directions(false, false);
        gondzio();  // gondzio_correction_direction! (solver.jl:245-298)
        step_size(false);
      }
      // ---- apply_step! + evaluate_model!
      k_apply<<<nb, NT, 0, s>>>(D);
      ++k_;
      // evaluate_model!: its objective is finalised by the next iteration's FIN_TERM (one launch
      // less; nothing reads obj_val before the termination test)
      SPMV_LAUNCH(k_eval, spmv_blocks(n_ + m_), s, D, PART_EVAL);
      eval_pending_ = true;
      MADIPM_HIP(hipGetLastError());
    }
  } catch (const Error& e) {
    // init_starting_point!'s failures (code -4): the same two exceptions, caught by solve!'s
    // catch-all (solver.jl:398-403)
    if (e.code == -4)
      status = MADIPM_INTERNAL_ERROR;
    else
      throw;
  }
  MADIPM_HIP(hipStreamSynchronize(s));
  solved_ = true;
  point_ok_ = true;
  ++n_solves_;
  solve_updates_ = n_updates_;
  t_total_ = now() - tstart;
  status_ = status;
  t_linsol_ = ldl_->fact_seconds(s) - fs0_;
  if (stats) {
    // the state read at the last termination test (the speculated directions after it changed only
    // step scalars, never the iterate)
    if (trace_.empty()) {
      read_state();
      wait_state();
      last_ = *hst_;
    }
    stats->status = status;
    stats->iter = k_;
    double obj = last_.obj_val / obj_scale_;
    if (!H_->minimize) obj = -obj;
    stats->objective = obj;
    stats->dual_objective = last_.dobj / obj_scale_;
    stats->inf_pr = inf_pr_;
    stats->inf_du = inf_du_;
    stats->inf_compl = inf_compl_;
    stats->mu = last_.mu;
    stats->total_time = t_total_;
    stats->linear_solver_time = t_linsol_;
    stats->init_time = t_init_;
    stats->exception = exception_;
  }
  return status;
}

}  // namespace madipm

namespace madipm {

// update_solution! (src/utils.jl:150-156) + MadNLP.update! [EXT]: un-scaled primal/dual solution
void MPCSolver::get_solution(double* x, double* y, double* zl, double* zu, double* cons) {
  MADIPM_HIP(hipStreamSynchronize(stream_));
  QPHost& P = *H_;
  if (cscale_host_stale_) {  // a device update computed con_scale on the device
    if (m_) MADIPM_HIP(hipMemcpy(P.con_scale.data(), plan_->cscale.p, sizeof(double) * m_, hipMemcpyDeviceToHost));
    cscale_host_stale_ = false;
  }
  std::vector<double> xh(n_), yh(m_), zlh(n_), zuh(n_);
  if (n_) {
    MADIPM_HIP(hipMemcpy(xh.data(), x_.p, sizeof(double) * n_, hipMemcpyDeviceToHost));
    MADIPM_HIP(hipMemcpy(zlh.data(), zl_.p, sizeof(double) * n_, hipMemcpyDeviceToHost));
    MADIPM_HIP(hipMemcpy(zuh.data(), zu_.p, sizeof(double) * n_, hipMemcpyDeviceToHost));
  }
  if (m_) MADIPM_HIP(hipMemcpy(yh.data(), y_.p, sizeof(double) * m_, hipMemcpyDeviceToHost));
  if (x) std::copy(xh.begin(), xh.begin() + nx_, x);
  if (zl)
    for (int i = 0; i < nx_; ++i) zl[i] = zlh[i] / obj_scale_;
  if (zu)
    for (int i = 0; i < nx_; ++i) zu[i] = zuh[i] / obj_scale_;
  if (y)
    for (int j = 0; j < m_; ++j) y[j] = yh[j] * P.con_scale[j] / obj_scale_;
  if (cons && m_) {  // A x = (J's columns < nx) x / con_scale + the fixed columns' part (cfix / con_scale)
    DBuf<double> ax;
    ax.alloc(m_);
    k_cons<<<(unsigned)((m_ + NT / 64 - 1) / (NT / 64)), NT, 0, stream_>>>(Jrp_, Jci_, Jv_, x_, cfix_, m_, nx_, ax);
    MADIPM_HIP(hipGetLastError());
    std::vector<double> h(m_);
    MADIPM_HIP(hipMemcpyAsync(h.data(), ax.p, sizeof(double) * m_, hipMemcpyDeviceToHost, stream_));
    MADIPM_HIP(hipStreamSynchronize(stream_));
    for (int j = 0; j < m_; ++j) cons[j] = h[j] / P.con_scale[j];
  }
}

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

struct AdjArgs {  // named in mpc.hpp (sens_solve)
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

// v = [q~; 0; gcons / con_scale], the vector the shifted right-hand side applies K's blocks to:
// q_i = (Sigma_l gzl - Sigma_u gzu)_i / (Sigma_l + Sigma_u)_i on a free variable with a bound, else 0 (the
// scalings cancel in q), q~ = q / obj_scale.  The slack entries are written 0: their J~^T row is not empty.
__global__ __launch_bounds__(NT) void k_adj_shift(AdjArgs A, AdjFull F, double* __restrict__ v, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
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

// The shifted right-hand side into d (and p, which keeps it for the residual), k_adj_resid's access pattern
// applied to v: gx + H~ q~ + J~^T (gcons / con_scale) on a free variable, 0 on a fixed one and on a slack,
// con_scale_r gy_r / obj_scale + J~_r q~ on row r.  Every entry is of the cotangents' magnitude: the
// Sigma terms of the plain form, 1e8 and more at an active bound, have cancelled in the algebra.
template <int G>
__global__ __launch_bounds__(NT) void k_adj_rhs_full(DV D, AdjArgs A, const double* __restrict__ gx,
                                                     const double* __restrict__ gy, const double* __restrict__ v) {
#pragma clang fp contract(off)
  const int n = D.n, m = D.m;
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
      D.d[i] = g;
      D.p[i] = g;
    }
  }
}

// a~ = a~' - [q~; 0; 0], with a~'x kept for the bound gradients
__global__ __launch_bounds__(NT) void k_adj_unshift(int nx, const double* __restrict__ v, double* __restrict__ sol,
                                                    double* __restrict__ apx) {
  GRID_LOOP(i, nx) {
    const double ap = sol[i];
    apx[i] = ap;
    sol[i] = ap - v[i];
  }
}

// gx into d's K2 layout (and into p, which keeps it for the residual): zero on fixed variables, slacks, rows
// t1 != nullptr: the factorisation before this launch ended (LinSolver::lazy_inertia), as in k_rhs
__global__ __launch_bounds__(NT) void k_adj_rhs(DV D, const double* __restrict__ gx, LDLStatus* t1) {
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
  GRID_LOOP(i, D.n + D.m) {
    const double v = (i < D.nx && !D.fixed[i]) ? gx[i] : 0.0;
    D.d[i] = v;
    D.p[i] = v;
  }
}

// r = g - K v and |r| of every row, K the K2 matrix of the point WITHOUT the regularisation the factor carries:
// H, J^T and Sigma_l + Sigma_u on a primal row, J on a dual row (k_residual's operator with the bound blocks
// folded into Sigma).  v = the current a~; r (may be null) becomes the right-hand side of a refinement solve.
template <int G>
__global__ __launch_bounds__(NT) void k_adj_resid(DV D, AdjArgs A, const double* __restrict__ v, double* __restrict__ r,
                                                  double* __restrict__ rowres) {
  const int n = D.n, m = D.m;
  const bool lead = (threadIdx.x & (G - 1)) == 0;
  GROUP_LOOP(i, n + m, G) {
    const double gi = D.p[i];
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

// out[0] = max_i rowres[i] / max(1, max_i |g_i|): one block, each thread a strided slice, then an LDS tree
// (a maximum does not depend on the order; a NaN is kept)
__global__ __launch_bounds__(NT) void k_adj_resmax(const double* __restrict__ rowres, const double* __restrict__ g,
                                                   int64_t N, double* __restrict__ out) {
  __shared__ double sw[NT], sg[NT];
  const int t = threadIdx.x;
  double w = 0.0, gm = 0.0;
  for (int64_t i = t; i < N; i += NT) {
    w = nmax(w, rowres[i]);
    gm = nmax(gm, fabs(g[i]));
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
  if (t == 0) out[0] = sw[0] / (sg[0] > 1.0 ? sg[0] : 1.0);
}

// The vector gradients (any output may be null).  Variable i: c_i = -sgn ax_i; a free one:
// lvar_i = Sigma_l,i ax_i = Sigma~_l,i a~x_i and uvar_i likewise (the scalings cancel); a fixed one: uvar_i = 0
// (lvar_i is k_adj_fix's).  Row i: an equality row lcon_i = ay_i, ucon_i = 0; a row with slack k:
// lcon_i = Sigma_l,k as_k = con_scale_i Sigma~_l,k a~s_k and ucon_i likewise.
// FULL (§13d; A.d is the un-shifted a~): a free variable's bounds in the shifted form,
// lvar_i = Sigma~_l,i a~'x_i + h_i (gzl_i + gzu_i), uvar_i = Sigma~_u,i a~'x_i - h_i (gzl_i + gzu_i),
// h_i = Sigma~_l Sigma~_u / (Sigma~_l + Sigma~_u) / obj_scale (0 where the sum is 0).
template <bool FULL>
__global__ __launch_bounds__(NT) void k_adj_vec(AdjArgs A, AdjFull F, const int32_t* __restrict__ rowslack,
                                                double* __restrict__ gc, double* __restrict__ glv,
                                                double* __restrict__ guv, double* __restrict__ glc,
                                                double* __restrict__ guc) {
#pragma clang fp contract(off)
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
__global__ __launch_bounds__(NT) void k_adj_avals(AdjArgs A, AdjFull F, int64_t nnz, const int32_t* __restrict__ Ar,
                                                  const int32_t* __restrict__ Ac, double* __restrict__ out) {
#pragma clang fp contract(off)
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
__global__ __launch_bounds__(NT) void k_adj_hvals(AdjArgs A, int64_t nnz, const int32_t* __restrict__ Hr,
                                                  const int32_t* __restrict__ Hc, double* __restrict__ out) {
#pragma clang fp contract(off)
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
__global__ __launch_bounds__(NT) void k_adj_fix(AdjArgs A, AdjFull F, int nfix, const int32_t* __restrict__ fix,
                                                const int32_t* __restrict__ fhsp, const int2* __restrict__ fh,
                                                const int32_t* __restrict__ fasp, const int2* __restrict__ fa,
                                                const double* __restrict__ Hraw, const double* __restrict__ Araw,
                                                const double* __restrict__ gx, double* __restrict__ glv) {
#pragma clang fp contract(off)
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

Adjoint& MPCSolver::sens_state() {
  if (!adj_) {
    auto a = std::make_unique<Adjoint>();
    a->rowres.alloc(std::max(n_ + m_, 1));
    a->sol.alloc(std::max(n_ + m_, 1));
    a->scal.alloc(2);
    a->scal.zero(stream_);
    MADIPM_HIP(hipEventCreateWithFlags(&a->ev[0], hipEventDisableTiming));
    MADIPM_HIP(hipEventCreateWithFlags(&a->ev[1], hipEventDisableTiming));
    adj_ = std::move(a);
  }
  return *adj_;
}

// the factor of the K2 matrix at the final iterate: once per solve
void MPCSolver::sens_factor(Adjoint& a, const std::string& who) {
  if (a.fact_solve == n_solves_) return;
  a.fact_solve = -1;
  if (pol_) pol_->fact_solve = -1;  // the polish's factor (§13f) is overwritten
  double dw = 0.0, dc = 0.0;  // the options' regularisation; Adaptive: the current pair, not decayed
  if (opt_.regularization == 1) {
    dw = opt_.delta_p;
    dc = opt_.delta_d;
  } else if (opt_.regularization != 0) {
    dw = adapt_dp_;
    dc = adapt_dd_;
  }
  bool ok = false;
  for (int trial = 0; trial < 3 && !ok; ++trial) {  // factorize_regularized_system!'s trials
    if (trial) {
      dw *= 100.0;
      dc *= 100.0;
    }
    factor_enqueue(dw, dc);
    ok = ldl_->status(stream_) == 0;
  }
  if (!ok) throw Error(who + "the factorisation of the KKT system at the solution failed in all three trials", -4);
  a.fact_solve = n_solves_;
  ++a.n_fact;
}

// With the right-hand side in d (and in p, which keeps it): a.sol = K^-1 p, refined; the residual ratio
// into resid[0]
void MPCSolver::sens_solve(Adjoint& a, const AdjArgs& A, double* resid) {
  DV_ARGS;
  hipStream_t s = stream_;
  const int nb = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_);
  const int64_t N = (int64_t)n_ + m_;
  kkt_solve();
  k_adj_acc<<<nb, NT, 0, s>>>(a.sol.p, d_.p, N, 1);
  // iterative refinement towards the system without the regularisation (the factor is the regularised
  // matrix's: each step gains about -log10(delta |K^-1|) digits); a fixed count, so nothing is read back
  for (int it = 0; it < adj_refine_steps(); ++it) {
    SPMV_LAUNCH(k_adj_resid, nbs, s, D, A, a.sol.p, d_.p, a.rowres.p);
    kkt_solve();
    k_adj_acc<<<nb, NT, 0, s>>>(a.sol.p, d_.p, N, 0);
  }
  SPMV_LAUNCH(k_adj_resid, nbs, s, D, A, a.sol.p, (double*)nullptr, a.rowres.p);
  k_adj_resmax<<<1, NT, 0, s>>>(a.rowres.p, p_.p, N, resid);
}

void MPCSolver::adjoint(const double* gx, const madipm_qp_gradients& g, bool device, hipStream_t caller) {
  adjoint(madipm_qp_cotangents{gx, nullptr, nullptr, nullptr, nullptr}, g, device, caller, nullptr);
}

// name == nullptr: madipm_solver_adjoint / _adjoint_device (gx alone, which must be given).  full: a
// cotangent other than gx is given, and the shifted system of §13d is solved; without one the kernels and
// their order are those of the gx-only call whichever entry point was taken.
void MPCSolver::adjoint(const madipm_qp_cotangents& ct, const madipm_qp_gradients& g, bool device,
                        hipStream_t caller, const char* name) {
  const std::string who =
      name ? std::string(name) + ": " : (device ? "madipm_solver_adjoint_device: " : "madipm_solver_adjoint: ");
  const double* const gx = ct.x;
  const bool full = ct.y || ct.zl || ct.zu || ct.cons;
  QPHost& P = *H_;
  // ---- refusals, before anything is allocated or enqueued
  sens_refuse(who);
  if (name)
    MADIPM_REQUIRE(gx || full, who + "all five cotangents are NULL");
  else
    MADIPM_REQUIRE(gx, who + "gx is NULL");
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
  Adjoint& a = sens_state();
  const double* cscale = device_con_scale();
  if (!device && gx && !a.gx.p) a.gx.alloc(std::max(nx_, 1));
  const double* const cot[4] = {ct.y, ct.zl, ct.zu, ct.cons};
  const int64_t clen[4] = {m_, nx_, nx_, m_};
  if (full) {
    if (!a.shift.p) {
      a.shift.alloc(std::max(n_ + m_, 1));
      a.apx.alloc(std::max(nx_, 1));
    }
    for (int j = 0; j < 4; ++j)
      if (!device && cot[j] && !a.ct[j].p) a.ct[j].alloc(std::max<int64_t>(clen[j], 1));
  }
  if ((g.lcon || g.ucon) && !a.rowslack.p) {
    a.rowslack.upload(adjoint_rowslack(P), s);
    MADIPM_HIP(hipStreamSynchronize(s));
  }
  if (needA && !a.Ar.p) {
    a.Ar.upload(plan_->Ar, s);
    a.Ac.upload(plan_->Ac, s);
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
  const int64_t len[7] = {nx_, nh, na, m_, m_, nx_, nx_};
  double* out[7];
  for (int j = 0; j < 7; ++j) {
    out[j] = user[j];
    if (!device && user[j]) {
      if (!a.out[j].p) a.out[j].alloc(std::max<int64_t>(len[j], 1));
      out[j] = a.out[j].p;
    }
  }
  // ---- the factor of the K2 matrix at the final iterate: once per solve
  DV_ARGS;
  sens_factor(a, who);
  // ---- right-hand side, solve, residual
  const double* dgx = gx;
  const double* dct[4] = {cot[0], cot[1], cot[2], cot[3]};  // gy, gzl, gzu, gcons on the device
  if (device) {  // the cotangents are read after the work already enqueued on the caller's stream
    MADIPM_HIP(hipEventRecord(a.ev[0], caller));
    MADIPM_HIP(hipStreamWaitEvent(s, a.ev[0], 0));
  } else {
    if (gx) {
      a.gx.upload(gx, nx_, s);
      dgx = a.gx.p;
    }
    for (int j = 0; j < 4; ++j)
      if (cot[j]) {
        if (clen[j]) a.ct[j].upload(cot[j], clen[j], s);
        dct[j] = a.ct[j].p;
      }
  }
  const int nb = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_);
  const AdjArgs A{n_, m_, nx_, obj_scale_, P.sgn, a.sol.p, x_.p, xl_.p, xu_.p, zl_.p, zu_.p, y_.p,
                  cscale, lbpos_.p, ubpos_.p, fixed_.p};
  const AdjFull F{dct[1], dct[2], dct[3], a.apx.p};
  if (full) {  // the shifted system K a~' = g' (§13d); p keeps g' for the residual
    k_adj_shift<<<nb, NT, 0, s>>>(A, F, a.shift.p, take_fact_end());
    SPMV_LAUNCH(k_adj_rhs_full, nbs, s, D, A, dgx, dct[0], (const double*)a.shift.p);
  } else {
    k_adj_rhs<<<nb, NT, 0, s>>>(D, dgx, take_fact_end());
  }
  sens_solve(a, A, a.scal.p);
  if (full && nx_) k_adj_unshift<<<blocks(nx_), NT, 0, s>>>(nx_, a.shift.p, a.sol.p, a.apx.p);
  // ---- gradients
  const bool vec = (out[0] || out[3] || out[4] || out[5] || out[6]) && std::max(nx_, m_);
  const bool fix = needFix && a.nfix > 0;
  if (full) {
    if (vec)
      k_adj_vec<true><<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, F, a.rowslack.p, out[0], out[5], out[6], out[3],
                                                                out[4]);
    if (fix)
      k_adj_fix<true><<<blocks(a.nfix), NT, 0, s>>>(A, F, a.nfix, a.fix.p, a.fhsp.p, a.fh.p, a.fasp.p, a.fa.p,
                                                     plan_->Hraw.p, plan_->Araw.p, dgx, out[5]);
    if (needA) k_adj_avals<true><<<blocks(na), NT, 0, s>>>(A, F, na, a.Ar.p, a.Ac.p, out[2]);
  } else {
    if (vec)
      k_adj_vec<false><<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, F, a.rowslack.p, out[0], out[5], out[6], out[3],
                                                                 out[4]);
    if (fix)
      k_adj_fix<false><<<blocks(a.nfix), NT, 0, s>>>(A, F, a.nfix, a.fix.p, a.fhsp.p, a.fh.p, a.fasp.p, a.fa.p,
                                                      plan_->Hraw.p, plan_->Araw.p, dgx, out[5]);
    if (needA) k_adj_avals<false><<<blocks(na), NT, 0, s>>>(A, F, na, a.Ar.p, a.Ac.p, out[2]);
  }
  if (needH) k_adj_hvals<<<blocks(nh), NT, 0, s>>>(A, nh, a.Hr.p, a.Hc.p, out[1]);
  MADIPM_HIP(hipGetLastError());
  if (device) {  // work enqueued on the caller's stream from now on sees the outputs
    MADIPM_HIP(hipEventRecord(a.ev[1], s));
    MADIPM_HIP(hipStreamWaitEvent(caller, a.ev[1], 0));
  } else {
    for (int j = 0; j < 7; ++j)
      if (user[j] && len[j])
        MADIPM_HIP(hipMemcpyAsync(user[j], out[j], len[j] * sizeof(double), hipMemcpyDeviceToHost, s));
    MADIPM_HIP(hipStreamSynchronize(s));
  }
  ++a.n_adjoints;
}

void MPCSolver::adjoint_info(int64_t* n_adjoints, int64_t* n_adjoint_factorizations, double* last_residual) {
  if (n_adjoints) *n_adjoints = adj_ ? adj_->n_adjoints : 0;
  if (n_adjoint_factorizations) *n_adjoint_factorizations = adj_ ? adj_->n_fact : 0;
  if (last_residual) {
    *last_residual = 0.0;
    if (adj_ && adj_->n_adjoints) {
      MADIPM_HIP(hipMemcpyAsync(last_residual, adj_->scal.p, sizeof(double), hipMemcpyDeviceToHost, stream_));
      MADIPM_HIP(hipStreamSynchronize(stream_));
    }
  }
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

// v = [p; p~_s; 0]: p_i = (Sigma_l dlvar + Sigma_u duvar)_i / (Sigma_l + Sigma_u)_i on a free variable with a
// bound, else 0 (the scalings cancel in p); the slack k of row r: p~_s,k = con_scale_r (Sigma_l,k dlcon_r +
// Sigma_u,k ducon_r) / (Sigma_l,k + Sigma_u,k).  One thread per variable and per row; a row's thread writes
// its slack's entry.
__global__ __launch_bounds__(NT) void k_tan_shift(AdjArgs A, TanDir T, const int32_t* __restrict__ rowslack,
                                                  double* __restrict__ v, LDLStatus* t1) {
#pragma clang fp contract(off)
  if (t1 && blockIdx.x == 0 && threadIdx.x == 0) ldl_status_end(t1);
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
__global__ __launch_bounds__(NT) void k_tan_data(AdjArgs A, TanDir T, const int32_t* __restrict__ gsp,
                                                 const int2* __restrict__ ge, const int32_t* __restrict__ csp,
                                                 const int2* __restrict__ ce, const int32_t* __restrict__ asp,
                                                 const int2* __restrict__ ae, const double* __restrict__ Hraw,
                                                 const double* __restrict__ Araw, double* __restrict__ base) {
#pragma clang fp contract(off)
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

// The shifted right-hand side into d (and p, which keeps it for the residual), k_adj_rhs_full's access
// pattern applied to v: base_i - (H~ p)_i on a free variable (v's row part is 0: J~^T adds nothing), 0 on a
// fixed one and on a slack, con_scale_r (db_r - base_r) - (J~ p - p~_s)_r on row r, db = dlcon on an equality
// row.  Every entry is of the directions' magnitude.
template <int G>
__global__ __launch_bounds__(NT) void k_tan_rhs(DV D, AdjArgs A, TanDir T, const int32_t* __restrict__ rowslack,
                                                const double* __restrict__ v, const double* __restrict__ base) {
#pragma clang fp contract(off)
  const int n = D.n, m = D.m;
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
      D.d[i] = g;
      D.p[i] = g;
    }
  }
}

// Un-shift and un-scale (A.d is the solution [dx'; ds~'; dy~] of the shifted system; any output may be null):
// dx = dx' + p on a free variable, dlvar on a fixed one (also into dxs, with zeros on the slacks, for
// k_tan_cons); dy = con_scale dy~ / obj_scale; dzl = -Sigma_l dx' + h (dlvar - duvar), dzu = Sigma_u dx' +
// h (dlvar - duvar) with the public Sigma = Sigma~ / obj_scale and h = Sigma_l Sigma_u / (Sigma_l + Sigma_u);
// 0 without that bound and on a fixed variable.
__global__ __launch_bounds__(NT) void k_tan_out(AdjArgs A, TanDir T, const double* __restrict__ v,
                                                double* __restrict__ dxs, double* __restrict__ ox,
                                                double* __restrict__ oy, double* __restrict__ ozl,
                                                double* __restrict__ ozu) {
#pragma clang fp contract(off)
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
__global__ __launch_bounds__(NT) void k_tan_cons(DV D, AdjArgs A, const double* __restrict__ dxs,
                                                 const double* __restrict__ base, double* __restrict__ ocons) {
#pragma clang fp contract(off)
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
  QPHost& P = *H_;
  // ---- refusals, before anything is allocated or enqueued
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
  hipStream_t s = stream_;
  // ---- allocations, each by the first call that needs it
  Adjoint& a = sens_state();
  if (!tan_) {
    auto t = std::make_unique<Tangent>();
    t->base.alloc(std::max(n_ + m_, 1));
    t->dx.alloc(std::max(n_, 1));
    t->scal.alloc(1);
    t->scal.zero(s);
    tan_ = std::move(t);
  }
  Tangent& t = *tan_;
  const double* cscale = device_con_scale();
  if (!a.shift.p) {  // as the five-cotangent adjoint allocates them
    a.shift.alloc(std::max(n_ + m_, 1));
    a.apx.alloc(std::max(nx_, 1));
  }
  if (!a.rowslack.p) {
    a.rowslack.upload(adjoint_rowslack(P), s);
    MADIPM_HIP(hipStreamSynchronize(s));
  }
  if (needLists && !t.lists) {  // the entry lists, from the host COO copies
    TangentLists L = build_tangent_lists(P);
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
  const int64_t dlen[7] = {nx_, nh, na, m_, m_, nx_, nx_};
  const int64_t olen[5] = {nx_, m_, nx_, nx_, m_};
  const double* ddir[7];
  double* out[5];
  for (int j = 0; j < 7; ++j) {
    ddir[j] = dir[j];
    if (!device && dir[j]) {
      if (!t.dir[j].p) t.dir[j].alloc(std::max<int64_t>(dlen[j], 1));
      ddir[j] = t.dir[j].p;
    }
  }
  for (int j = 0; j < 5; ++j) {
    out[j] = user[j];
    if (!device && user[j]) {
      if (!t.out[j].p) t.out[j].alloc(std::max<int64_t>(olen[j], 1));
      out[j] = t.out[j].p;
    }
  }
  // ---- the factor of the K2 matrix at the final iterate: the adjoint's, once per solve
  DV_ARGS;
  sens_factor(a, who);
  if (device) {  // the directions are read after the work already enqueued on the caller's stream
    MADIPM_HIP(hipEventRecord(a.ev[0], caller));
    MADIPM_HIP(hipStreamWaitEvent(s, a.ev[0], 0));
  } else {
    for (int j = 0; j < 7; ++j)
      if (dir[j] && dlen[j]) t.dir[j].upload(dir[j], dlen[j], s);
  }
  // ---- right-hand side, solve, residual
  const int nb = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_);
  const AdjArgs A{n_, m_, nx_, obj_scale_, P.sgn, a.sol.p, x_.p, xl_.p, xu_.p, zl_.p, zu_.p, y_.p,
                  cscale, lbpos_.p, ubpos_.p, fixed_.p};
  const TanDir T{ddir[0], ddir[1], ddir[2], ddir[3], ddir[4], ddir[5], ddir[6]};
  const bool ls = needLists;  // lists built by an earlier call are not walked when this one has no use for them
  k_tan_shift<<<nb, NT, 0, s>>>(A, T, a.rowslack.p, a.shift.p, take_fact_end());
  k_tan_data<<<nb, NT, 0, s>>>(A, T, ls ? t.gsp.p : nullptr, t.ge.p, t.csp.p, t.ce.p, ls ? t.asp.p : nullptr, t.ae.p,
                               plan_ ? plan_->Hraw.p : nullptr, plan_ ? plan_->Araw.p : nullptr, t.base.p);
  SPMV_LAUNCH(k_tan_rhs, nbs, s, D, A, T, (const int32_t*)a.rowslack.p, (const double*)a.shift.p,
              (const double*)t.base.p);
  sens_solve(a, A, t.scal.p);
  // ---- outputs
  k_tan_out<<<blocks(std::max(std::max(nx_, m_), std::max(n_ - nx_, 1))), NT, 0, s>>>(
      A, T, a.shift.p, t.dx.p, out[0], out[1], out[2], out[3]);
  if (out[4] && m_)
    SPMV_LAUNCH(k_tan_cons, spmv_blocks(m_), s, D, A, (const double*)t.dx.p, (const double*)t.base.p, out[4]);
  MADIPM_HIP(hipGetLastError());
  if (device) {  // work enqueued on the caller's stream from now on sees the outputs
    MADIPM_HIP(hipEventRecord(a.ev[1], s));
    MADIPM_HIP(hipStreamWaitEvent(caller, a.ev[1], 0));
  } else {
    for (int j = 0; j < 5; ++j)
      if (user[j] && olen[j])
        MADIPM_HIP(hipMemcpyAsync(user[j], out[j], olen[j] * sizeof(double), hipMemcpyDeviceToHost, s));
    MADIPM_HIP(hipStreamSynchronize(s));
  }
  ++t.n_tangents;
}

void MPCSolver::tangent_info(int64_t* n_tangents, double* last_residual) {
  if (n_tangents) *n_tangents = tan_ ? tan_->n_tangents : 0;
  if (last_residual) {
    *last_residual = 0.0;
    if (tan_ && tan_->n_tangents) {
      MADIPM_HIP(hipMemcpyAsync(last_residual, tan_->scal.p, sizeof(double), hipMemcpyDeviceToHost, stream_));
      MADIPM_HIP(hipStreamSynchronize(stream_));
    }
  }
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

}  // namespace

void MPCSolver::polish(const madipm_polish_opts& o, const int8_t* av, const int8_t* ar, const madipm_polish_out& po,
                       madipm_polish_info* info, bool device, hipStream_t caller) {
  const std::string who = device ? "madipm_solver_polish_device: " : "madipm_solver_polish: ";
  QPHost& P = *H_;
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
  Adjoint& a = sens_state();
  const double* cscale = device_con_scale();
  if (!a.rowslack.p) {
    a.rowslack.upload(adjoint_rowslack(P), s);
    MADIPM_HIP(hipStreamSynchronize(s));
  }
  const int ns = n_ - nx_;
  if (!pol_) {
    auto p = std::make_unique<Polish>();
    p->w.alloc(std::max(n_ + m_, 1));
    p->grad.alloc(std::max(n_, 1));
    p->lo.alloc(std::max(n_, 1));
    p->hi.alloc(std::max(n_, 1));
    p->part.alloc((size_t)4 * MAXB);
    p->ax.alloc(std::max(m_, 1));
    p->codes.alloc(std::max(n_, 1));
    p->codes_fact.alloc(std::max(n_, 1));
    p->codes_fact.zero(s);
    p->ineq.alloc(std::max(ns, 1));
    p->ineq.upload(P.ind_ineq.data(), P.ind_ineq.size(), s);
    p->flags.alloc(2);
    p->meas.alloc(1);
    pol_ = std::move(p);
  }
  Polish& p = *pol_;
  if (p.bounds_updates != n_updates_) {  // the raw bounds of [x; s], as the last update left them
    refresh_host_mirrors();
    std::vector<double> lo(std::max(n_, 1)), hi(std::max(n_, 1));
    for (int i = 0; i < nx_; ++i) lo[i] = P.lvar[i], hi[i] = P.uvar[i];
    for (int k = 0; k < ns; ++k) lo[nx_ + k] = P.lcon[P.ind_ineq[k]], hi[nx_ + k] = P.ucon[P.ind_ineq[k]];
    p.lo.upload(lo, s);
    p.hi.upload(hi, s);
    MADIPM_HIP(hipStreamSynchronize(s));  // lo / hi are this scope's
    p.bounds_updates = n_updates_;
  }
  const int64_t olen[5] = {nx_, m_, nx_, nx_, m_};
  double* out[5];
  for (int j = 0; j < 5; ++j) {
    out[j] = user[j];
    if (!device && user[j]) {
      if (!p.out[j].p) p.out[j].alloc(std::max<int64_t>(olen[j], 1));
      out[j] = p.out[j].p;
    }
  }
  int8_t *ovar = po.active_var, *orow = po.active_row;
  const int8_t *dav = av, *dar = ar;
  if (!device) {
    if (ovar && !p.out_var.p) p.out_var.alloc(std::max(nx_, 1));
    if (orow && !p.out_row.p) p.out_row.alloc(std::max(m_, 1));
    if (ovar) ovar = p.out_var.p;
    if (orow) orow = p.out_row.p;
    if (av) {
      if (!p.in_var.p) {
        p.in_var.alloc(std::max(nx_, 1));
        p.in_row.alloc(std::max(m_, 1));
      }
      p.in_var.upload(av, nx_, s);
      p.in_row.upload(ar, m_, s);
      dav = p.in_var.p;
      dar = p.in_row.p;
    }
  } else {  // the set is read, and the outputs written, after the work already enqueued on the caller's stream
    MADIPM_HIP(hipEventRecord(a.ev[0], caller));
    MADIPM_HIP(hipStreamWaitEvent(s, a.ev[0], 0));
  }
  // ---- the codes and the projected point
  DV_ARGS;
  const PolArgs A{n_, m_, nx_, obj_scale_, x_.p, zl_.p, zu_.p, y_.p, cscale, lbpos_.p, ubpos_.p, fixed_.p,
                  p.lo.p, p.hi.p, p.ineq.p, a.rowslack.p, p.codes.p, p.codes_fact.p, p.w.p, p.grad.p, p.flags.p};
  const int nb = blocks(n_ + m_), nbs = spmv_blocks(n_ + m_), nbn = blocks(std::max(n_, 1));
  const int64_t N = (int64_t)n_ + m_;
  p.flags.zero(s);
  k_pol_classify<<<blocks(std::max(std::max(n_, m_), 1)), NT, 0, s>>>(A, dav, dar, take_fact_end());
  MADIPM_HIP(hipGetLastError());
  int32_t hflags[2] = {0, 0};
  MADIPM_HIP(hipMemcpyAsync(hflags, p.flags.p, sizeof(hflags), hipMemcpyDeviceToHost, s));
  MADIPM_HIP(hipStreamSynchronize(s));
  MADIPM_REQUIRE(!hflags[0], who + "the supplied set has a code other than -1, 0, +1, or a code on a bound that does "
                                   "not exist, on a fixed variable or on an equality row");
  // ---- the factor: once per point, set and sigma
  bool ok = true;
  if (p.fact_solve != n_solves_ || p.fact_sigma != o.sigma || hflags[1]) {
    p.fact_solve = -1;
    a.fact_solve = -1;  // the adjoint's factor and KKT diagonal are overwritten
    double dw = 0.0, dc = 0.0;  // sens_factor's regularisation and trials
    if (opt_.regularization == 1) {
      dw = opt_.delta_p;
      dc = opt_.delta_d;
    } else if (opt_.regularization != 0) {
      dw = adapt_dp_;
      dc = adapt_dd_;
    }
    ok = false;
    for (int trial = 0; trial < 3 && !ok; ++trial) {
      if (trial) {
        dw *= 100.0;
        dc *= 100.0;
      }
      k_pol_diag<<<nb, NT, 0, s>>>(D, p.codes.p, dw, dc, o.sigma, fact_reset());
      timed_factorize();
      ok = ldl_->status(s) == 0;
    }
    if (ok) {
      if (n_) MADIPM_HIP(hipMemcpyAsync(p.codes_fact.p, p.codes.p, (size_t)n_, hipMemcpyDeviceToDevice, s));
      p.fact_solve = n_solves_;
      p.fact_sigma = o.sigma;
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
  const unsigned nbc = (unsigned)((m_ + NT / 64 - 1) / (NT / 64));
  if (any5 && std::max(nx_, m_)) {
    if (hm.verdict == MADIPM_POLISHED) {
      if (out[4] && m_) k_cons<<<nbc, NT, 0, s>>>(Jrp_, Jci_, Jv_, p.w.p, cfix_, m_, nx_, p.ax.p);
      k_pol_out<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, p.ax.p, out[0], out[1], out[2], out[3], out[4]);
    } else {
      if (out[4] && m_) k_cons<<<nbc, NT, 0, s>>>(Jrp_, Jci_, Jv_, x_, cfix_, m_, nx_, p.ax.p);
      k_unscale<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(nx_, m_, obj_scale_, x_, y_, zl_, zu_, p.ax.p, cscale, out[0],
                                                          out[1], out[2], out[3], out[4]);
    }
  }
  if ((ovar || orow) && std::max(nx_, m_)) k_pol_codes<<<blocks(std::max(nx_, m_)), NT, 0, s>>>(A, ovar, orow);
  MADIPM_HIP(hipGetLastError());
  if (device) {  // work enqueued on the caller's stream from now on sees the outputs
    MADIPM_HIP(hipEventRecord(a.ev[1], s));
    MADIPM_HIP(hipStreamWaitEvent(caller, a.ev[1], 0));
  } else {
    for (int j = 0; j < 5; ++j)
      if (user[j] && olen[j])
        MADIPM_HIP(hipMemcpyAsync(user[j], out[j], olen[j] * sizeof(double), hipMemcpyDeviceToHost, s));
    if (po.active_var && nx_) MADIPM_HIP(hipMemcpyAsync(po.active_var, ovar, (size_t)nx_, hipMemcpyDeviceToHost, s));
    if (po.active_row && m_) MADIPM_HIP(hipMemcpyAsync(po.active_row, orow, (size_t)m_, hipMemcpyDeviceToHost, s));
    MADIPM_HIP(hipStreamSynchronize(s));
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
  *info = pol_ ? pol_->last : madipm_polish_info{-1, 0, 0.0, 0.0, 0.0, 0, 0};
}

}  // namespace madipm

namespace madipm {

// update_step! (kernels.jl:291-358) on caller-given bounded-coordinate vectors, through the solver's
// own step-test kernels (k_alpha + k_final(FIN_ALPHA), and k_mu + k_final(FIN_MU_FULL) for
// MehrotraAdaptiveStep).  The vectors are laid out as a problem with n = nlb + nub primal
// coordinates, the lower-bounded ones first, no constraints: ind_lb = [0, nlb), ind_ub = [nlb, n).
void update_step_standalone(int rule, double tau_param, double mu, int nlb, int nub, const double* const* v,
                            madipm_step_result* out, hipStream_t s) {
  const int n = nlb + nub;
  MADIPM_REQUIRE(nlb >= 0 && nub >= 0 && n > 0, "update_step: no bounded coordinate");
  MADIPM_REQUIRE(rule >= 0 && rule <= 2, "update_step: rule must be 0, 1 or 2");
  DBuf<double> x(n), xl(n), xu(n), zl(n), zu(n), d(n + nlb + nub), part((size_t)NPART * MAXB + NL2 * FG + 8);
  DBuf<int32_t> ilb(std::max(nlb, 1)), iub(std::max(nub, 1));
  DBuf<DevState> st(1);
  std::vector<int32_t> io(n);
  for (int i = 0; i < n; ++i) io[i] = i;
  ilb.upload(io.data(), nlb, s);
  iub.upload(io.data() + nlb, nub, s);
  MADIPM_HIP(hipMemsetAsync(part.p, 0, sizeof(double) * part.n, s));  // k_final's ticket starts at 0
  MADIPM_HIP(hipMemsetAsync(x.p, 0, sizeof(double) * n, s));
  MADIPM_HIP(hipMemsetAsync(xl.p, 0, sizeof(double) * n, s));
  MADIPM_HIP(hipMemsetAsync(xu.p, 0, sizeof(double) * n, s));
  MADIPM_HIP(hipMemsetAsync(zl.p, 0, sizeof(double) * n, s));
  MADIPM_HIP(hipMemsetAsync(zu.p, 0, sizeof(double) * n, s));
  auto cp = [&](double* dst, const double* src, int cnt) {
    if (cnt) MADIPM_HIP(hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyDeviceToDevice, s));
  };
  // v: x_lr, xl_r, zl_r, dx_lr, dzl, x_ur, xu_r, zu_r, dx_ur, dzu
  cp(x.p, v[0], nlb), cp(xl.p, v[1], nlb), cp(zl.p, v[2], nlb), cp(d.p, v[3], nlb), cp(d.p + n, v[4], nlb);
  cp(x.p + nlb, v[5], nub), cp(xu.p + nlb, v[6], nub), cp(zu.p + nlb, v[7], nub), cp(d.p + nlb, v[8], nub);
  cp(d.p + n + nlb, v[9], nub);
  DV D{};
  D.n = n;
  D.m = 0;
  D.nx = n;
  D.nlb = nlb;
  D.nub = nub;
  D.x = x.p, D.xl = xl.p, D.xu = xu.p, D.zl = zl.p, D.zu = zu.p, D.d = d.p;
  D.ind_lb = ilb.p, D.ind_ub = iub.p;
  D.part = part.p;
  D.st = st.p;
  k_set_mu<<<1, 1, 0, s>>>(st.p, mu);
  const int nbz = (int)std::max<int64_t>(1, std::min<int64_t>(MAXB, (std::max(nlb, nub) + NT - 1) / NT));
  const int mode = rule == 0 ? ALPHA_CONSERVATIVE : (rule == 1 ? ALPHA_ADAPTIVE : ALPHA_MEHROTRA);
  const double tau = rule == 2 ? 1.0 : tau_param;
  k_alpha<<<nbz, NT, 0, s>>>(D, mode, tau, 0);
  FinParams P{nbz, mode, 0, 0, 0, 0, 0};
  launch_final(D, FIN_ALPHA, P, s);
  if (rule == 2) {
    k_mu<<<nbz, NT, 0, s>>>(D, 1, 0.0, 0.0);
    FinParams Q{nbz, 0, (double)(nlb + nub), tau_param, 0, 0, 0};
    launch_final(D, FIN_MU_FULL, Q, s);
  }
  MADIPM_HIP(hipGetLastError());
  DevState h{};
  MADIPM_HIP(hipMemcpyAsync(&h, st.p, sizeof(DevState), hipMemcpyDeviceToHost, s));
  MADIPM_HIP(hipStreamSynchronize(s));
  out->alpha_p = h.alpha_p;
  out->alpha_d = h.alpha_d;
  out->alpha_xl = h.a_xl, out->alpha_xu = h.a_xu, out->alpha_zl = h.a_zl, out->alpha_zu = h.a_zu;
  out->i_xl = h.i_xl, out->i_xu = h.i_xu, out->i_zl = h.i_zl, out->i_zu = h.i_zu;
}

}  // namespace madipm
