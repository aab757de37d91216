// What the two translation units of the MPC driver share (mpc.hip: the interior-point loop, updates, warm
// start; mpc_post.hip: adjoint, tangent, polish): the kernels' view of the solver's vectors, the launch
// constants, the loop macros, the SpMV row sums and the block reductions.  Private to csrc/; each unit
// launches only its own kernels.
#pragma once

#include <cstddef>
#include <limits>
#include <vector>

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

namespace {  // internal linkage, as when one file held everything: each unit compiles its own copy

constexpr int NT = 256;
constexpr int NPART = 16;
constexpr int MAXB = 2048;  // partial-reduction blocks (part_ holds NPART x MAXB, value-major)
// partial k of block b: value-major so k_final's loads of one value are coalesced
__device__ __forceinline__ int pidx(int b, int k) { return k * MAXB + b; }
constexpr double INF = std::numeric_limits<double>::infinity();

enum { OP_SUM = 0, OP_MAX = 1, OP_MIN = 2 };

__device__ __forceinline__ double nmax(double a, double b) { return ((b > a) | (b != b)) ? b : a; }
__device__ __forceinline__ double comb(double a, double b, int op) {
  return op == OP_SUM ? a + b : (op == OP_MAX ? nmax(a, b) : fmin(a, b));
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

}  // namespace

}  // namespace madipm

// launch a GROUP_LOOP SpMV kernel with the problem's lane-group width (inside a member of MPCSolver)
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
