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

#include "mpc_kernels.hpp"

namespace madipm {

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
  StreamHandoff sync;
  bool has[4] = {false, false, false, false};  // x, y, zl, zu of the current point
  bool active = false;
  double weight = 0.0;
};

namespace {

__device__ __forceinline__ double csr_dot(const DCsr& A, int row, const double* __restrict__ x) {
  double s = 0.0;
  for (int64_t q = A.rp[row]; q < A.rp[row + 1]; ++q) s += A.v[q] * x[A.ci[q]];
  return s;
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

// lvar, uvar, lcon, ucon of the device route's staging, when they are what the solver holds (no host update
// ran since they were written)
bool MPCSolver::device_raw_bounds(const double* (&raw)[4]) const {
  if (!dev_ || dev_raw_stale_) return false;
  raw[0] = dev_->lvar.p, raw[1] = dev_->uvar.p, raw[2] = dev_->lcon.p, raw[3] = dev_->ucon.p;
  return true;
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
  stream_after(dv.ev, caller, s);
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
  if (!sol_ax_.p) sol_ax_.alloc(std::max(m_, 1));
  const double* cscale = device_con_scale();
  // the outputs are written after the caller's earlier work on them, and read by its later work
  sol_sync_.begin(caller, stream_);
  unscale_point(cscale, sol_ax_, x, y, zl, zu, cons);
  MADIPM_HIP(hipGetLastError());
  sol_sync_.end(stream_, caller);
}

// get_solution's constraint values of the scaled point xs, before the division by con_scale, into ax
void MPCSolver::cons_rows(const double* xs, double* ax) {
  const unsigned nb = (unsigned)((m_ + NT / 64 - 1) / (NT / 64));
  if (m_) k_cons<<<nb, NT, 0, stream_>>>(Jrp_, Jci_, Jv_, xs, cfix_, m_, nx_, ax);
}

// update_solution! of the iterate into device arrays (any may be null); ax: m_ doubles of scratch when cons is given
void MPCSolver::unscale_point(const double* cscale, double* ax, double* x, double* y, double* zl, double* zu,
                              double* cons) {
  if (cons) cons_rows(x_, ax);
  if (std::max(nx_, m_))
    k_unscale<<<blocks(std::max(nx_, m_)), NT, 0, stream_>>>(nx_, m_, obj_scale_, x_, y_, zl_, zu_, ax, cscale, x, y,
                                                              zl, zu, cons);
}

// The kernels' view of the member buffers (rebuilt per launch site; cheap, host-only)
DV MPCSolver::view() const {
  DV D;
  D.n = n_, D.m = m_, D.nx = nx_, D.nlb = nlb_, D.nub = nub_;
  D.x = x_, D.xl = xl_, D.xu = xu_, D.zl = zl_, D.zu = zu_, D.f = f_, D.jacl = jacl_, D.c = c_, D.y = y_, D.rhs = rhs_;
  D.pr_diag = pr_diag_, D.l_diag = l_diag_, D.u_diag = u_diag_, D.l_lower = l_lower_, D.u_lower = u_lower_;
  D.d = d_, D.p = p_, D.corr_lb = corr_lb_, D.corr_ub = corr_ub_;
  D.Kx = Kx_, D.diag_pos = diag_pos_, D.Hdiag = Hdiag_, D.cs = cs_, D.gfix = gfix_, D.cfix = cfix_;
  D.ind_lb = ind_lb_, D.ind_ub = ind_ub_, D.lbpos = lbpos_, D.ubpos = ubpos_, D.fixed = fixed_;
  D.H = DCsr{Hrp_, Hci_, Hv_}, D.J = DCsr{Jrp_, Jci_, Jv_}, D.JT = DCsr{JTrp_, JTci_, JTv_};
  D.part = part_, D.st = st_, D.kkt = kkt_;
  D.sk = sk_, D.Krow = Krow_, D.Kcol = Kcol_, D.K0 = K0_, D.nnzK = nnzK_;
  D.Dinv = Dinv_, D.bufm = bufm_, D.cpp = cpp_, D.cprod = reinterpret_cast<const int2*>(cprod_.p);
  D.Cx = Cx_, D.nnzC = nnzC_;
  return D;
}

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
  if (device) w.sync.begin(caller, s);  // the caller's arrays are read after the work already enqueued on its stream
  const double* src[4] = {x, y, zl, zu};
  double* dst[4] = {w.x.p, w.y.p, w.zl.p, w.zu.p};
  const int64_t len[4] = {nx_, m_, nx_, nx_};
  for (int k = 0; k < 4; ++k) {
    w.has[k] = src[k] != nullptr;
    if (src[k] && len[k]) MADIPM_HIP(hipMemcpyAsync(dst[k], src[k], len[k] * sizeof(double), kind, s));
  }
  if (device)
    w.sync.end(s, caller);  // the caller's later work on its stream (overwriting the arrays) comes after the copies
  else
    MADIPM_HIP(hipStreamSynchronize(s));  // host arrays are read during the call only
  w.weight = weight;
  w.active = true;
  initialized_ = false;
}

void MPCSolver::warm_start_last(double weight) {
  check_weight(weight);
  MADIPM_REQUIRE(solved_, "madipm_solver_warm_start_last: no solve has run on this solver yet");
  WarmStart& w = warm_buffers();
  unscale_point(device_con_scale(), nullptr, w.x, w.y, w.zl, w.zu, nullptr);
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
  const DV D = view();
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
  const DV D = view();
  k_diag<<<blocks(n_ + m_), NT, 0, stream_>>>(D, dw, dc, fact_reset());
}

// set_aug_diagonal_reg! + build_kkt! of the chosen formulation (values consumed by the LDL^T)
void MPCSolver::assemble_kkt(double dw, double dc, bool diag_done) {
  const DV D = view();
  if (!diag_done) kkt_diag(dw, dc);
  if (kkt_ == KKT_K25) k_k25_scale<<<blocks(nnzK_), NT, 0, stream_>>>(D);
  if (kkt_ == KKT_NORMAL) k_normal_asm<<<blocks(nnzC_), NT, 0, stream_>>>(D);
}

const double* MPCSolver::kvals() const { return kkt_ == KKT_NORMAL ? Cx_.p : Kx_.p; }

// factorize! between two pooled timing events (cnt.linear_solver_time, MadNLP.factorize_wrapper!);
// the pool grows only when a solve needs more pairs than any earlier one did
void MPCSolver::timed_factorize() {
  ldl_->factorize_async(kvals(), stream_);
  ++n_factor_calls_;
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
  const DV D = view();
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
  const DV D = view();
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
  const DV D = view();
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
  const DV D = view();
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
  const DV D = view();
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
  const DV D = view();
  hipStream_t s = stream_;
  ++n_inits_;
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
  const DV D = view();
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
  const DV D = view();
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
  const DV D = view();
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
    cons_rows(x_, ax);
    MADIPM_HIP(hipGetLastError());
    std::vector<double> h(m_);
    MADIPM_HIP(hipMemcpyAsync(h.data(), ax.p, sizeof(double) * m_, hipMemcpyDeviceToHost, stream_));
    MADIPM_HIP(hipStreamSynchronize(stream_));
    for (int j = 0; j < m_; ++j) cons[j] = h[j] / P.con_scale[j];
  }
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
