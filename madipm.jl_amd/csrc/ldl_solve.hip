// Multifrontal supernodal LDL^T for gfx950: the triangular solves with the factor of ldl.hip.
// Multifrontal forward solve per front:  v = [b(own cols); 0] + extend-add of the children's update
// vectors;  v[0:w] <- L11^{-1} v[0:w];  v[w:] -= L21 v[0:w];  own part -> xi, rest -> update vector.
// Backward:  v[0:w] = D^{-1} xi(own) - L21^T x(below rows);  x_own = L11^{-T} v[0:w].
//  * fronts with r <= 128: one WAVE per front (wave-synchronous, v in LDS), 4 fronts per workgroup;
//  * bigger fronts: dependency-driven persistent kernels.  Tasks = 64-row blocks (forward) or 64-column
//    panels (backward), dequeued in dependency order from one atomic counter; block i waits for the
//    published x of panels < i (release/acquire flags tagged with a per-solve epoch), so the whole
//    level is ONE launch and the panel GEMVs of different blocks overlap.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstdio>

#include "ldl_device.hpp"

namespace madipm {
namespace {

constexpr int SW = 4;  // waves (= small fronts) per workgroup

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// initial forward value of row i of front s: own right-hand side entry, or (sharded top fronts) the
// exchanged sum of b and the other shards' subtree updates
__device__ __forceinline__ double fwd_init(const FrontTab& T, int s, int i, int w, int f0, const double* __restrict__ b) {
  // the caller's entry loaded unconditionally (clamped row): its two dependent loads issue beside the
  // xoff load instead of after it (a load under a branch waits for everything before it)
  const double bv = b[T.perm[f0 + min(i, max(w - 1, 0))]];
  const int64_t xo = T.xoff[s];
  if (xo >= 0) return T.xch[xo + i];
  return (i < w) ? bv : 0.0;
}

// Destination of update entry a of front s: its slot in the tree parent's contiguous gather range
// (T.upos >= 0) or the front's own update vector (read by the level kernels through sv_src).
__device__ __forceinline__ double* uvec_dst(const FrontTab& T, int s, int a, double* uvec) {
  const int64_t p = T.upos[T.rel_ptr[s] + a];
  return p >= 0 ? T.gbuf + p : uvec + T.uvec_off[s] + a;
}

// uvec_dst of the rows lane + 64 h (h < NH) of front s for a whole wave at once: the front's words
// once (uniform), every row's slot loaded unconditionally from a clamped row, then selected — uvec_dst
// per row under its row mask was three dependent round trips per row (k_fwd_tree: nine before the
// wait of every front, ~10 us of the level-1 fronts' start)
template <int NH>
__device__ __forceinline__ void uvec_dsts(const FrontTab& T, int s, int w, int r, int f0, bool act, int lane,
                                          double* uvec, double* xi, double* (&dst)[NH]) {
  const int64_t rp = T.rel_ptr[s], uo = T.uvec_off[s];
  const int amax = r - w - 1;  // (uniform) the front's last update row
  int64_t p[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) p[h] = amax >= 0 ? T.upos[rp + min(max(lane + 64 * h - w, 0), amax)] : -1;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const int i = lane + 64 * h;
    dst[h] = (act && i >= w && i < r) ? (p[h] >= 0 ? T.gbuf + p[h] : uvec + uo + (i - w)) : xi + f0 + min(i, max(w - 1, 0));
  }
}

// HBM panel (r x w, ld r) -> LDS (ld rl), all threads, 16 independent loads per thread per batch
// (one HBM round trip per 4096 doubles: a 128 x 128 front is 4 round trips)
__device__ __forceinline__ void stage_panel(const double* __restrict__ L, double* Ls, int r, int w, int rl) {
  const int nel = r * w;
  ColWalk wk(threadIdx.x, r);
  for (int base = 0; base < nel; base += NT * 16) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int q = base + k * NT + threadIdx.x;
      v[k] = (q < nel) ? L[q] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int q = base + k * NT + threadIdx.x;
      if (q < nel) Ls[wk.i + wk.j * rl] = v[k];
      wk.next();
    }
  }
}

// the producer's end of the hand-off (ldl_device.hpp): the storing wave, after its sc1 stores
__device__ __forceinline__ void publish_sc1(int32_t* f, int epoch) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(f, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ micro fronts (w <= 2, r <= 32)
// (MG lanes per front, lane l owns rows l and l + 16: k_micro_factor's layout, ldl.hip)
// forward / backward solves of micro fronts (same lane layout); x_0, x_1 broadcast within the group
__global__ __launch_bounds__(NT) void k_fwd_micro(FrontTab T, const int32_t* __restrict__ fronts, int nf,
                                                  const double* __restrict__ arena, const double* __restrict__ b,
                                                  double* __restrict__ xi, double* __restrict__ uvec) {
  const int g = threadIdx.x / MG, l = threadIdx.x & (MG - 1);
  const int q = blockIdx.x * (NT / MG) + g;
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  double v[2], c0[2], c1[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = l + 16 * h;
    double vi = 0.0, a0 = 0.0, a1 = 0.0;
    if (i < r) {
      vi = fwd_init(T, s, i, w, f0, b);
      const int64_t e = T.row_ptr[s] + i;
      const int64_t p1 = T.sv_ptr[e + 1];
      for (int64_t p = T.sv_ptr[e]; p < p1; ++p) vi += uvec[T.sv_src[p]];
      a0 = L[i];
      if (w == 2) a1 = L[i + r];
    }
    v[h] = vi;
    c0[h] = a0;
    c1[h] = a1;
  }
  const double x0 = __shfl(v[0], 0, MG);
  const double l10 = __shfl(c0[0], 1, MG);
  const double x1 = (w == 2) ? __shfl(v[0], 1, MG) - l10 * x0 : 0.0;
  if (!live) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = l + 16 * h;
    if (i < w) {
      xi[f0 + i] = (i == 0) ? x0 : x1;
    } else if (i < r) {
      *uvec_dst(T, s, i - w, uvec) = (v[h] - c0[h] * x0) - c1[h] * x1;
    }
  }
}

__global__ __launch_bounds__(NT) void k_bwd_micro(FrontTab T, const int32_t* __restrict__ fronts, int nf,
                                                  const double* __restrict__ arena, const double* __restrict__ D,
                                                  double* __restrict__ xi, double* __restrict__ out) {
  const int g = threadIdx.x / MG, l = threadIdx.x & (MG - 1);
  const int q = blockIdx.x * (NT / MG) + g;
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
  double a0 = 0.0, a1 = 0.0, l10 = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = l + 16 * h;
    if (i >= w && i < r) {
      const double x = xi[rows[i]];  // final: ancestors
      a0 = fma(L[i], x, a0);
      if (w == 2) a1 = fma(L[i + r], x, a1);
    }
    if (i == 1 && w == 2) l10 = L[1];
  }
#pragma unroll
  for (int o = MG / 2; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o, MG);
    a1 += __shfl_xor(a1, o, MG);
  }
  l10 = __shfl(l10, 1, MG);
  if (!live || l != 0) return;
  const double v1 = (w == 2) ? xi[f0 + 1] / D[f0 + 1] - a1 : 0.0;
  const double v0 = xi[f0] / D[f0] - a0 - l10 * v1;
  xi[f0] = v0;
  if (T.wout[s]) out[T.perm[f0]] = v0;
  if (w == 2) {
    xi[f0 + 1] = v1;
    if (T.wout[s]) out[T.perm[f0 + 1]] = v1;
  }
}

// forward: s_j = b(c_j) / d_j, t = W s (two passes: column chunks of LBF_COLS -> partials, then the
// chunks summed in order), the group's update vector = -t; the members' forward values are b(c_j)
__global__ __launch_bounds__(NT) void k_lb_fwd1(const double* __restrict__ W, const double* __restrict__ dlb,
                                                const int32_t* __restrict__ mem, const int32_t* __restrict__ perm,
                                                int m, int n, int64_t mem0, const double* __restrict__ b,
                                                double* __restrict__ xi, double* __restrict__ part) {
  __shared__ double sj[LBF_COLS];
  const int c0 = blockIdx.y * LBF_COLS;
  const int nc = min(LBF_COLS, n - c0);
  if (threadIdx.x < nc) {
    const int j = c0 + threadIdx.x;
    const int col = mem[mem0 + j];
    const double bj = b[perm[col]];
    sj[threadIdx.x] = bj / dlb[mem0 + j];
    if (blockIdx.x == 0) xi[col] = bj;
  }
  __syncthreads();
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= m) return;
  const double* __restrict__ Wc = W + (int64_t)c0 * m + i;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int j = 0;
  for (; j + 3 < nc; j += 4) {
    a0 = fma(Wc[(int64_t)j * m], sj[j], a0);
    a1 = fma(Wc[(int64_t)(j + 1) * m], sj[j + 1], a1);
    a2 = fma(Wc[(int64_t)(j + 2) * m], sj[j + 2], a2);
    a3 = fma(Wc[(int64_t)(j + 3) * m], sj[j + 3], a3);
  }
  for (; j < nc; ++j) a0 = fma(Wc[(int64_t)j * m], sj[j], a0);
  part[(int64_t)blockIdx.y * m + i] = (a0 + a1) + (a2 + a3);
}

__global__ __launch_bounds__(NT) void k_lb_fwd2(const double* __restrict__ part, int m, int nchunk,
                                                double* __restrict__ uv) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= m) return;
  double v = 0.0;
  for (int c = 0; c < nchunk; ++c) v += part[(int64_t)c * m + i];
  uv[i] = -v;
}

// backward: x_j = (y_j - W(:, j)^T x_P(gpos)) / d_j, one wave per member column
__global__ __launch_bounds__(NT) void k_lb_bwd(const double* __restrict__ W, const double* __restrict__ dlb,
                                               const int32_t* __restrict__ mem, const int32_t* __restrict__ perm,
                                               const int32_t* __restrict__ xrow, int m, int n, int64_t mem0,
                                               double* __restrict__ xi, double* __restrict__ out) {
  const int j = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= n) return;
  const double* __restrict__ Wc = W + (int64_t)j * m;
  double a = 0.0;
  for (int k = lane; k < m; k += 64) a = fma(Wc[k], xi[xrow[k]], a);
  a = wave_sum(a);
  if (lane == 0) {
    const int col = mem[mem0 + j];
    const double x = (xi[col] - a) / dlb[mem0 + j];
    xi[col] = x;
    out[perm[col]] = x;
  }
}

// Small-front solves (32 < r <= 128): one WORKGROUP per front.  The whole workgroup first copies the
// r x w L panel into LDS with every load in flight at once (the panel is contiguous in HBM, ld r; in
// LDS ld = r | 1 so that column-strided lane accesses of the backward solve are conflict-free), then
// wave 0 runs the substitution from LDS: lane l holds rows (forward) or pivot columns (backward) l and
// l + 64 in registers, the value of row/column t is broadcast with readlane.  Turning the panel read
// from a latency chain into one bandwidth burst is what bounds these levels.

// Blocked substitutions of ONE wave on a panel staged in LDS (col-major, ld rl), rows / columns
// i = lane + 64 h (h < 3) held in v[h].  Pivots are taken 16 at a time: the block's L entries of
// every row are loaded into registers up front (one LDS latency per block), then the 16-step
// dependency chain touches only v[HB] (readlane broadcast + one fma per step), and the rows of the
// other thirds get the block's contribution as 16 independent fmas.  HB (the third holding the
// block) is a template parameter so every register index is static.
template <int HB>
__device__ __forceinline__ void fwd_block16(double (&v)[3], const double* Ls, int rl, int r, int t0, int kb, int lane) {
  double lb[3][16];
#pragma unroll
  for (int h = HB; h < 3; ++h) {
    const int i = lane + 64 * h;
    const int ic = min(i, r - 1);
#pragma unroll
    for (int k = 0; k < 16; ++k) lb[h][k] = (k < kb && i > t0 + k && i < r) ? Ls[ic + (t0 + k) * rl] : 0.0;
  }
  double xs[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    xs[k] = 0.0;
    if (k < kb) {  // wave-uniform
      xs[k] = readlane_f64(v[HB], (t0 & 63) + k);
      v[HB] = fma(-lb[HB][k], xs[k], v[HB]);
    }
  }
#pragma unroll
  for (int h = HB + 1; h < 3; ++h)
#pragma unroll
    for (int k = 0; k < 16; ++k) v[h] = fma(-lb[h][k], xs[k], v[h]);
}

// forward: v[i] -= L(i, t) v[t] for i > t, t < w
__device__ __forceinline__ void fwd_subst16(double (&v)[3], const double* Ls, int rl, int r, int w, int lane) {
  for (int t0 = 0; t0 < w; t0 += 16) {
    const int kb = min(16, w - t0);
    if (t0 < 64)
      fwd_block16<0>(v, Ls, rl, r, t0, kb, lane);
    else if (t0 < 128)
      fwd_block16<1>(v, Ls, rl, r, t0, kb, lane);
    else
      fwd_block16<2>(v, Ls, rl, r, t0, kb, lane);
  }
}

template <int HB>
__device__ __forceinline__ void bwd_block16(double (&v)[3], const double* Ls, int rl, int w, int t0, int kb, int lane) {
  double lb[HB + 1][16];
#pragma unroll
  for (int h = 0; h <= HB; ++h) {
    const int j = lane + 64 * h;
    const int jc = min(j, w - 1);
#pragma unroll
    for (int k = 0; k < 16; ++k) lb[h][k] = (k < kb && j < t0 + k) ? Ls[(t0 + k) + jc * rl] : 0.0;
  }
  double xs[16];
#pragma unroll
  for (int k = 15; k >= 0; --k) {
    xs[k] = 0.0;
    if (k < kb) {  // wave-uniform
      xs[k] = readlane_f64(v[HB], (t0 & 63) + k);
      v[HB] = fma(-lb[HB][k], xs[k], v[HB]);
    }
  }
#pragma unroll
  for (int h = 0; h < HB; ++h)
#pragma unroll
    for (int k = 0; k < 16; ++k) v[h] = fma(-lb[h][k], xs[k], v[h]);
}

// backward (transposed): v[j] -= L(t, j) v[t] for j < t, t = w-1 .. 1
__device__ __forceinline__ void bwd_subst16(double (&v)[3], const double* Ls, int rl, int w, int lane) {
  for (int t0 = ((w - 1) >> 4) << 4; t0 >= 0; t0 -= 16) {
    const int kb = min(16, w - t0);
    if (t0 < 64)
      bwd_block16<0>(v, Ls, rl, w, t0, kb, lane);
    else if (t0 < 128)
      bwd_block16<1>(v, Ls, rl, w, t0, kb, lane);
    else
      bwd_block16<2>(v, Ls, rl, w, t0, kb, lane);
  }
}

// r <= SMALL_SOLVE_MAX rows (3 per lane of wave 0), panel r x w staged in LDS (ld r | 1)

__global__ __launch_bounds__(NT) void k_fwd_small(FrontTab T, const int32_t* __restrict__ fronts, int nf,
                                                  const double* __restrict__ arena, const double* __restrict__ b,
                                                  double* __restrict__ xi, double* __restrict__ uvec) {
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  __shared__ double v0s[SMALL_SOLVE_MAX];
  const int s = fronts[blockIdx.x];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int rl = r | 1;
  stage_panel(arena + T.l_off[s], Ls, r, w, rl);
  const int lane = threadIdx.x & 63;
  // initial vector (own b + children's update vectors): all 256 threads, rows strided, each row's
  // gather list walked with 4 loads in flight
  for (int i = threadIdx.x; i < r; i += NT) {
    const int64_t e = T.row_ptr[s] + i;
    const int64_t p1 = T.sv_ptr[e + 1];
    int64_t p = T.sv_ptr[e];
    double vi = 0.0;
    for (; p + 3 < p1; p += 4) {
      const int64_t q0 = T.sv_src[p], q1 = T.sv_src[p + 1], q2 = T.sv_src[p + 2], q3 = T.sv_src[p + 3];
      vi += (uvec[q0] + uvec[q1]) + (uvec[q2] + uvec[q3]);
    }
    for (; p < p1; ++p) vi += uvec[T.sv_src[p]];
    v0s[i] = vi + fwd_init(T, s, i, w, f0, b);
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  double v[3];
  int ci[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const int i = lane + 64 * h;
    v[h] = (i < r) ? v0s[i] : 0.0;
    ci[h] = min(i, r - 1);
  }
  fwd_subst16(v, Ls, rl, r, w, lane);  // v[i] -= L(i, t) v[t] for i > t, t < w
  (void)ci;
  double* __restrict__ uo = uvec + T.uvec_off[s];
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const int i = lane + 64 * h;
    if (i < w)
      xi[f0 + i] = v[h];
    else if (i < r)
      uo[i - w] = v[h];
  }
}

__global__ __launch_bounds__(NT) void k_bwd_small(FrontTab T, const int32_t* __restrict__ fronts, int nf,
                                                  const double* __restrict__ arena, const double* __restrict__ D,
                                                  double* __restrict__ xi, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  __shared__ double xbs[SMALL_SOLVE_MAX];
  const int s = fronts[blockIdx.x];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int rl = r | 1;
  stage_panel(arena + T.l_off[s], Ls, r, w, rl);
  const int lane = threadIdx.x & 63;
  const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
  const int nb = r - w;
  // x of the rows below the pivot block (ancestors: final), all threads
  for (int k = threadIdx.x; k < nb; k += NT) xbs[k] = xi[rows[w + k]];
  double own[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const int j = lane + 64 * h;
    own[h] = (threadIdx.x < 64 && j < w) ? xi[f0 + j] / D[f0 + j] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  int cj[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) cj[h] = min(lane + 64 * h, w - 1);
  // v[j] = x_j / d_j - sum_{i >= w} L(i, j) x_i
  double acc[3] = {0.0, 0.0, 0.0};
  for (int k8 = 0; k8 < nb; k8 += 8) {
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = k8 + kk;
      if (k < nb) {
        const double x = xbs[k];
#pragma unroll
        for (int h = 0; h < 3; ++h) acc[h] = fma(Ls[(w + k) + cj[h] * rl], x, acc[h]);
      }
    }
  }
  double v[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) v[h] = (lane + 64 * h < w) ? own[h] - acc[h] : 0.0;
  bwd_subst16(v, Ls, rl, w, lane);  // for t = w-1 .. 1: v[j] -= L(t, j) v[t] for j < t
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const int j = lane + 64 * h;
    if (j < w) {
      xi[f0 + j] = v[h];
      if (T.wout[s]) out[T.perm[f0 + j]] = v[h];
    }
  }
}

// Fronts with r <= 32 (the leaf level has ~10^5): HALF a wave per front, 8 fronts per workgroup;
// lane l & 31 holds row / pivot column l & 31, values exchanged with 32-wide shuffles.
__global__ __launch_bounds__(NT) void k_fwd_tiny(FrontTab T, const int32_t* __restrict__ fronts, int nf,
                                                 const double* __restrict__ arena, const double* __restrict__ b,
                                                 double* __restrict__ xi, double* __restrict__ uvec) {
  const int lane = threadIdx.x & 63, lr = lane & 31;
  const int q = (blockIdx.x * SW + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  double v = 0.0;
  if (lr < r) {
    v = fwd_init(T, s, lr, w, f0, b);
    const int64_t e = T.row_ptr[s] + lr;
    const int64_t p1 = T.sv_ptr[e + 1];
    for (int64_t p = T.sv_ptr[e]; p < p1; ++p) v += uvec[T.sv_src[p]];
  }
  const int wmax = max(__builtin_amdgcn_readlane(w, 0), __builtin_amdgcn_readlane(w, 32));
  const int cl = min(lr, r - 1);
  for (int t4 = 0; t4 < wmax; t4 += 4) {
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = L[cl + (int64_t)min(t4 + k, w - 1) * r];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = t4 + k;
      const double xt = __shfl(v, t & 31, 32);
      v = fma((t < w && lr > t) ? -c[k] : 0.0, xt, v);
    }
  }
  if (live && lr < r) {
    if (lr < w)
      xi[f0 + lr] = v;
    else
      *uvec_dst(T, s, lr - w, uvec) = v;
  }
}

__global__ __launch_bounds__(NT) void k_bwd_tiny(FrontTab T, const int32_t* __restrict__ fronts, int nf,
                                                 const double* __restrict__ arena, const double* __restrict__ D,
                                                 double* __restrict__ xi, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, lr = lane & 31;
  const int q = (blockIdx.x * SW + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
  const int nb = r - w;
  const double xb = (lr < nb) ? xi[rows[w + lr]] : 0.0;  // x of below row w + lr (final)
  const int cj = min(lr, w - 1);
  const int nbmax = max(__builtin_amdgcn_readlane(nb, 0), __builtin_amdgcn_readlane(nb, 32));
  double acc = 0.0;
  for (int k4 = 0; k4 < nbmax; k4 += 4) {
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = L[min(w + k4 + k, r - 1) + (int64_t)cj * r];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double x = __shfl(xb, (k4 + k) & 31, 32);
      acc = fma((k4 + k < nb) ? c[k] : 0.0, x, acc);
    }
  }
  double v = (lr < w) ? xi[f0 + lr] / D[f0 + lr] - acc : 0.0;
  const int wmax = max(__builtin_amdgcn_readlane(w, 0), __builtin_amdgcn_readlane(w, 32));
  for (int t4 = wmax - 1; t4 > 0; t4 -= 4) {
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = L[min(max(t4 - k, 0), w - 1) + (int64_t)cj * r];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = t4 - k;
      const double xt = __shfl(v, max(t, 0) & 31, 32);
      v = fma((t > 0 && t < w && lr < t) ? -c[k] : 0.0, xt, v);
    }
  }
  if (live && lr < w) {
    xi[f0 + lr] = v;
    if (T.wout[s]) out[T.perm[f0 + lr]] = v;
  }
}

// ------------------------------------------------------------------ multi-right-hand-side level kernels
// The level kernels above over kc <= MW columns (LDLSolver::solve_multi_async): column j of
// the right-hand side / solution at b + j n, of the internal vector at xi + j N, of the update vector at
// uvec + j ustride.  Every L entry, row index, gather index and pivot is loaded once per front and used for
// all kc columns.  A front's update entries always go to its own update vector (never through T.upos into
// T.gbuf) and the children's are read through sv_src, which indexes the update vector for every row of every
// front.  A column's operations and their order are those of the single-column kernel: kc is a uniform loop
// bound or guard only, so a column's bits depend neither on kc nor on its slot.  The plans that take this
// route are unsharded (T.xoff = -1 everywhere): the initial value is the caller's entry.
constexpr int MW = MULTI_W;

__global__ __launch_bounds__(NT) void k_fwd_micro_m(FrontTab T, const int32_t* __restrict__ fronts, int nf, int kc,
                                                    const double* __restrict__ arena, const double* __restrict__ b,
                                                    int64_t n, double* __restrict__ xi, int64_t N,
                                                    double* __restrict__ uvec, int64_t ustride) {
  const int g = threadIdx.x / MG, l = threadIdx.x & (MG - 1);
  const int q = blockIdx.x * (NT / MG) + g;
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  const int64_t uo = T.uvec_off[s];
  double v[2][MW], c0[2], c1[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = l + 16 * h;
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int j = 0; j < MW; ++j) v[h][j] = 0.0;
    if (i < r) {
      if (i < w) {
        const int64_t pi = T.perm[f0 + i];
#pragma unroll
        for (int j = 0; j < MW; ++j)
          if (j < kc) v[h][j] = b[j * n + pi];
      }
      const int64_t e = T.row_ptr[s] + i;
      const int64_t p1 = T.sv_ptr[e + 1];
      for (int64_t p = T.sv_ptr[e]; p < p1; ++p) {
        const int64_t src = T.sv_src[p];
#pragma unroll
        for (int j = 0; j < MW; ++j)
          if (j < kc) v[h][j] += uvec[j * ustride + src];
      }
      a0 = L[i];
      if (w == 2) a1 = L[i + r];
    }
    c0[h] = a0;
    c1[h] = a1;
  }
  const double l10 = __shfl(c0[0], 1, MG);
#pragma unroll
  for (int j = 0; j < MW; ++j) {
    if (j >= kc) break;  // uniform
    const double x0 = __shfl(v[0][j], 0, MG);
    const double x1 = (w == 2) ? __shfl(v[0][j], 1, MG) - l10 * x0 : 0.0;
    if (!live) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = l + 16 * h;
      if (i < w) {
        xi[j * N + f0 + i] = (i == 0) ? x0 : x1;
      } else if (i < r) {
        uvec[j * ustride + uo + (i - w)] = (v[h][j] - c0[h] * x0) - c1[h] * x1;
      }
    }
  }
}

__global__ __launch_bounds__(NT) void k_bwd_micro_m(FrontTab T, const int32_t* __restrict__ fronts, int nf, int kc,
                                                    const double* __restrict__ arena, const double* __restrict__ D,
                                                    double* __restrict__ xi, int64_t N, double* __restrict__ out,
                                                    int64_t n) {
  const int g = threadIdx.x / MG, l = threadIdx.x & (MG - 1);
  const int q = blockIdx.x * (NT / MG) + g;
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
  double a0[MW], a1[MW], l10 = 0.0;
#pragma unroll
  for (int j = 0; j < MW; ++j) a0[j] = a1[j] = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = l + 16 * h;
    if (i >= w && i < r) {
      const int64_t row = rows[i];  // final: ancestors
      const double c0 = L[i], c1 = (w == 2) ? L[i + r] : 0.0;
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) {
          const double x = xi[j * N + row];
          a0[j] = fma(c0, x, a0[j]);
          if (w == 2) a1[j] = fma(c1, x, a1[j]);
        }
    }
    if (i == 1 && w == 2) l10 = L[1];
  }
  l10 = __shfl(l10, 1, MG);
  const bool head = live && l == 0;
  const double d0 = D[f0], d1 = (w == 2) ? D[f0 + 1] : 1.0;
  const int64_t p0 = T.perm[f0], p1 = (w == 2) ? T.perm[f0 + 1] : 0;
  const bool wo = T.wout[s];
#pragma unroll
  for (int j = 0; j < MW; ++j) {
    if (j >= kc) break;  // uniform
    double s0 = a0[j], s1 = a1[j];
#pragma unroll
    for (int o = MG / 2; o > 0; o >>= 1) {
      s0 += __shfl_xor(s0, o, MG);
      s1 += __shfl_xor(s1, o, MG);
    }
    if (!head) continue;
    double* __restrict__ xj = xi + j * N;
    const double v1 = (w == 2) ? xj[f0 + 1] / d1 - s1 : 0.0;
    const double v0 = xj[f0] / d0 - s0 - l10 * v1;
    xj[f0] = v0;
    if (wo) out[j * n + p0] = v0;
    if (w == 2) {
      xj[f0 + 1] = v1;
      if (wo) out[j * n + p1] = v1;
    }
  }
}

__global__ __launch_bounds__(NT) void k_fwd_tiny_m(FrontTab T, const int32_t* __restrict__ fronts, int nf, int kc,
                                                   const double* __restrict__ arena, const double* __restrict__ b,
                                                   int64_t n, double* __restrict__ xi, int64_t N,
                                                   double* __restrict__ uvec, int64_t ustride) {
  const int lane = threadIdx.x & 63, lr = lane & 31;
  const int q = (blockIdx.x * SW + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  double v[MW];
#pragma unroll
  for (int j = 0; j < MW; ++j) v[j] = 0.0;
  if (lr < r) {
    if (lr < w) {
      const int64_t pi = T.perm[f0 + lr];
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) v[j] = b[j * n + pi];
    }
    const int64_t e = T.row_ptr[s] + lr;
    const int64_t p1 = T.sv_ptr[e + 1];
    for (int64_t p = T.sv_ptr[e]; p < p1; ++p) {
      const int64_t src = T.sv_src[p];
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) v[j] += uvec[j * ustride + src];
    }
  }
  const int wmax = max(__builtin_amdgcn_readlane(w, 0), __builtin_amdgcn_readlane(w, 32));
  const int cl = min(lr, r - 1);
  for (int t4 = 0; t4 < wmax; t4 += 4) {
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = L[cl + (int64_t)min(t4 + k, w - 1) * r];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = t4 + k;
      const double ck = (t < w && lr > t) ? -c[k] : 0.0;
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) {  // uniform
          const double xt = __shfl(v[j], t & 31, 32);
          v[j] = fma(ck, xt, v[j]);
        }
    }
  }
  if (live && lr < r) {
    const int64_t uo = T.uvec_off[s];
#pragma unroll
    for (int j = 0; j < MW; ++j)
      if (j < kc) {
        if (lr < w)
          xi[j * N + f0 + lr] = v[j];
        else
          uvec[j * ustride + uo + (lr - w)] = v[j];
      }
  }
}

__global__ __launch_bounds__(NT) void k_bwd_tiny_m(FrontTab T, const int32_t* __restrict__ fronts, int nf, int kc,
                                                   const double* __restrict__ arena, const double* __restrict__ D,
                                                   double* __restrict__ xi, int64_t N, double* __restrict__ out,
                                                   int64_t n) {
  const int lane = threadIdx.x & 63, lr = lane & 31;
  const int q = (blockIdx.x * SW + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
  const int nb = r - w;
  double xb[MW], acc[MW], v[MW];  // xb: x of below row w + lr (final)
  const int64_t brow = (lr < nb) ? rows[w + lr] : 0;
#pragma unroll
  for (int j = 0; j < MW; ++j) {
    xb[j] = (lr < nb && j < kc) ? xi[j * N + brow] : 0.0;
    acc[j] = 0.0;
  }
  const int cj = min(lr, w - 1);
  const int nbmax = max(__builtin_amdgcn_readlane(nb, 0), __builtin_amdgcn_readlane(nb, 32));
  for (int k4 = 0; k4 < nbmax; k4 += 4) {
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = L[min(w + k4 + k, r - 1) + (int64_t)cj * r];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double ck = (k4 + k < nb) ? c[k] : 0.0;
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) {  // uniform
          const double x = __shfl(xb[j], (k4 + k) & 31, 32);
          acc[j] = fma(ck, x, acc[j]);
        }
    }
  }
  const double dj = D[f0 + cj];
#pragma unroll
  for (int j = 0; j < MW; ++j) v[j] = (lr < w && j < kc) ? xi[j * N + f0 + lr] / dj - acc[j] : 0.0;
  const int wmax = max(__builtin_amdgcn_readlane(w, 0), __builtin_amdgcn_readlane(w, 32));
  for (int t4 = wmax - 1; t4 > 0; t4 -= 4) {
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = L[min(max(t4 - k, 0), w - 1) + (int64_t)cj * r];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = t4 - k;
      const double ck = (t > 0 && t < w && lr < t) ? -c[k] : 0.0;
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) {  // uniform
          const double xt = __shfl(v[j], max(t, 0) & 31, 32);
          v[j] = fma(ck, xt, v[j]);
        }
    }
  }
  if (live && lr < w) {
    const int64_t pi = T.perm[f0 + lr];
    const bool wo = T.wout[s];
#pragma unroll
    for (int j = 0; j < MW; ++j)
      if (j < kc) {
        xi[j * N + f0 + lr] = v[j];
        if (wo) out[j * n + pi] = v[j];
      }
  }
}

// Small fronts: the panel staged once by the whole workgroup, the kc initial vectors through LDS, then wave q
// substitutes columns q and q + 4 one after the other, each exactly as wave 0 of k_fwd_small / k_bwd_small
// does (one column per wave in two rounds: the registers of the single-column kernel, and four columns already
// keep all four waves busy).
__global__ __launch_bounds__(NT) void k_fwd_small_m(FrontTab T, const int32_t* __restrict__ fronts, int nf, int kc,
                                                    const double* __restrict__ arena, const double* __restrict__ b,
                                                    int64_t n, double* __restrict__ xi, int64_t N,
                                                    double* __restrict__ uvec, int64_t ustride) {
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  __shared__ double v0s[MW][SMALL_SOLVE_MAX];
  const int s = fronts[blockIdx.x];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int rl = r | 1;
  stage_panel(arena + T.l_off[s], Ls, r, w, rl);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < r; i += NT) {
    const int64_t e = T.row_ptr[s] + i;
    const int64_t p1 = T.sv_ptr[e + 1];
    int64_t p = T.sv_ptr[e];
    const int64_t pi = T.perm[f0 + min(i, w - 1)];
    double vi[MW];
#pragma unroll
    for (int j = 0; j < MW; ++j) vi[j] = 0.0;
    for (; p + 3 < p1; p += 4) {
      const int64_t q0 = T.sv_src[p], q1 = T.sv_src[p + 1], q2 = T.sv_src[p + 2], q3 = T.sv_src[p + 3];
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) {
          const double* __restrict__ u = uvec + j * ustride;
          vi[j] += (u[q0] + u[q1]) + (u[q2] + u[q3]);
        }
    }
    for (; p < p1; ++p) {
      const int64_t q0 = T.sv_src[p];
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) vi[j] += uvec[j * ustride + q0];
    }
#pragma unroll
    for (int j = 0; j < MW; ++j)
      if (j < kc) v0s[j][i] = vi[j] + ((i < w) ? b[j * n + pi] : 0.0);
  }
  __syncthreads();
  const int64_t uo = T.uvec_off[s];
  for (int j = wave; j < kc; j += NT / 64) {
    double v[3];
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int i = lane + 64 * h;
      v[h] = (i < r) ? v0s[j][i] : 0.0;
    }
    fwd_subst16(v, Ls, rl, r, w, lane);  // v[i] -= L(i, t) v[t] for i > t, t < w
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int i = lane + 64 * h;
      if (i < w)
        xi[j * N + f0 + i] = v[h];
      else if (i < r)
        uvec[j * ustride + uo + (i - w)] = v[h];
    }
  }
}

__global__ __launch_bounds__(NT) void k_bwd_small_m(FrontTab T, const int32_t* __restrict__ fronts, int nf, int kc,
                                                    const double* __restrict__ arena, const double* __restrict__ D,
                                                    double* __restrict__ xi, int64_t N, double* __restrict__ out,
                                                    int64_t n) {
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  // per column: [0, w) the own entries x_j / d_j, [w, r) x of the rows below the pivot block (ancestors: final)
  __shared__ double xbs[MW][SMALL_SOLVE_MAX];
  const int s = fronts[blockIdx.x];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int rl = r | 1;
  stage_panel(arena + T.l_off[s], Ls, r, w, rl);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
  const int nb = r - w;
  for (int i = threadIdx.x; i < r; i += NT) {
    if (i < w) {
      const double d = D[f0 + i];
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) xbs[j][i] = xi[j * N + f0 + i] / d;
    } else {
      const int64_t row = rows[i];
#pragma unroll
      for (int j = 0; j < MW; ++j)
        if (j < kc) xbs[j][i] = xi[j * N + row];
    }
  }
  __syncthreads();
  int cj[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) cj[h] = min(lane + 64 * h, w - 1);
  int64_t pj[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) pj[h] = T.perm[f0 + cj[h]];
  const bool wo = T.wout[s];
  for (int j = wave; j < kc; j += NT / 64) {
    const double* xb = xbs[j] + w;
    // v[j] = x_j / d_j - sum_{i >= w} L(i, j) x_i
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k8 = 0; k8 < nb; k8 += 8) {
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int k = k8 + kk;
        if (k < nb) {
          const double x = xb[k];
#pragma unroll
          for (int h = 0; h < 3; ++h) acc[h] = fma(Ls[(w + k) + cj[h] * rl], x, acc[h]);
        }
      }
    }
    double v[3];
#pragma unroll
    for (int h = 0; h < 3; ++h) v[h] = (lane + 64 * h < w) ? xbs[j][cj[h]] - acc[h] : 0.0;
    bwd_subst16(v, Ls, rl, w, lane);  // for t = w-1 .. 1: v[j] -= L(t, j) v[t] for j < t
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int c = lane + 64 * h;
      if (c < w) {
        xi[j * N + f0 + c] = v[h];
        if (wo) out[j * n + pj[h]] = v[h];
      }
    }
  }
}

// initial forward vector of a big front (own b entries + children's update vectors), in HBM;
// task = (front, chunk of GAT_ROWS rows), GAT_G lanes per row stride the row's gather list (children
// in list order per lane, lanes combined by a fixed butterfly: deterministic)
constexpr int GAT_G = 8;
static_assert(GAT_ROWS == NT / GAT_G, "rows of a gather task");
__global__ __launch_bounds__(NT) void k_fwd_gather(FrontTab T, const int32_t* __restrict__ list,
                                                   const double* __restrict__ b, const double* __restrict__ uvec,
                                                   double* __restrict__ vwork) {
  int s, chunk;
  task_of(list, s, chunk);
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int i = chunk * GAT_ROWS + threadIdx.x / GAT_G, gl = threadIdx.x & (GAT_G - 1);
  if (i >= r) return;  // whole groups leave together
  const int64_t e = T.row_ptr[s] + i;
  const int64_t p1 = T.sv_ptr[e + 1];
  double vi = 0.0;
  for (int64_t p = T.sv_ptr[e] + gl; p < p1; p += GAT_G) vi += uvec[T.sv_src[p]];
#pragma unroll
  for (int o = GAT_G / 2; o > 0; o >>= 1) vi += __shfl_xor(vi, o, GAT_G);
  if (gl == 0) vwork[e] = vi + fwd_init(T, s, i, w, f0, b);
}

// Triangular solves of a 64-pivot diagonal block by one wave, 16 pivots per batch: the batch's L
// entries are loaded first, then each pivot's value is broadcast by v_readlane (an SGPR, a few cycles)
// — a __shfl (ds_bpermute) per pivot put an LDS round trip on the chain: ~5 us per 64-pivot block.
// forward: a[lane] -= L(lane, t) a[t] for t < lane, t < kw; L(i, t) at Ld[t * 65 + i]
__device__ __forceinline__ double tri_fwd64(double a, const double* Ld, int kw, int lane) {
  for (int t0 = 0; t0 < kw; t0 += 16) {
    double lb[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) lb[k] = Ld[min(t0 + k, 63) * 65 + lane];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int tt = t0 + k;
      const double xt = readlane_f64(a, min(tt, 63));
      const double na = a - lb[k] * xt;
      a = (lane > tt && tt < kw) ? na : a;
    }
  }
  return a;
}
// backward (transposed): a[lane] -= L(t, lane) a[t] for t > lane, t < kw, from t = kw - 1 down;
// L(t, j) at Ld[t * 65 + j]
__device__ __forceinline__ double tri_bwd64(double a, const double* Ld, int kw, int lane) {
  for (int t1 = kw - 1; t1 > 0; t1 -= 16) {
    double lb[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) lb[k] = Ld[max(t1 - k, 0) * 65 + lane];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int tt = t1 - k;
      const double xt = readlane_f64(a, max(tt, 0));
      const double na = a - lb[k] * xt;
      a = (lane < tt && tt > 0) ? na : a;
    }
  }
  return a;
}

// Panel solutions handed between the big-front solve tasks as self-validating 8-byte words (the LL
// idea): value halves each stored with the solve's epoch in the upper 32 bits by single-copy-atomic
// 8-byte stores, so a consumer lane polls its two words until both carry the epoch — the data is the
// flag: no release fence and drain before a flag store, no acquire and second round trip after it.
__device__ __forceinline__ void ll_put(uint64_t* w, double v, int epoch) {
  const uint64_t tag = (uint64_t)(uint32_t)epoch << 32;
  __hip_atomic_store(w, tag | (uint32_t)__double2loint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(w + 1, tag | (uint32_t)__double2hiint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ll_get(const uint64_t* w, int epoch, int32_t* err) {
  uint64_t a, b;
  int spins = 0;
  for (;;) {
    a = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)(a >> 32) == (uint32_t)epoch && (uint32_t)(b >> 32) == (uint32_t)epoch) break;
    __builtin_amdgcn_s_sleep(1);
    if (++spins > (1 << 25)) {
      atomicOr(err, kErrHandoff);
      break;
    }
  }
  return __hiloint2double((int)(uint32_t)b, (int)(uint32_t)a);
}

// Forward, big fronts: task = (front, 64-row block i).  acc(rows) = v(rows) - sum_{panels p < i} L(rows,p) x_p,
// then (pivot block) x_i = L_ii^{-1} acc, handed to the later row blocks through T.xll (ll_put / ll_get).
__global__ __launch_bounds__(NT) void k_fwd_big(FrontTab T, const SolveTask* __restrict__ tasks, int ntasks,
                                                int32_t* counter, int32_t* flags, const int32_t* __restrict__ flag_off,
                                                int epoch, const double* __restrict__ arena,
                                                const double* __restrict__ vwork, double* __restrict__ xi,
                                                double* __restrict__ uvec, int32_t* err) {
  __shared__ int s_task;
  __shared__ double xs[64];
  __shared__ double part[4][64];
  __shared__ double Ld[64 * 65];
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  for (;;) {
    if (tid == 0) s_task = atomicAdd(counter, 1);
    __syncthreads();
    const int t = s_task;
    __syncthreads();
    if (t >= ntasks) return;
    const int s = tasks[t].front, i = tasks[t].blk;
    const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
    const double* __restrict__ L = arena + T.l_off[s];
    const int row0 = i * 64, nrow = min(64, r - row0);
    const int npan = (w + 63) >> 6;
    const int np = min(i, npan);
    const int row = row0 + lane;
    const bool pivot_blk = row0 < w;
    const int kw = pivot_blk ? min(64, w - row0) : 0;
    // every load below is issued unconditionally from a clamped address and masked after: a
    // predicated load compiles into a branch with a wait of its own (16 serial round trips per batch)
    const int rowc = row0 + min(lane, nrow - 1);
    // prefetch the diagonal block (columns row0 .. row0+kw-1 of this row block) into LDS
    if (kw > 0) {
      double v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = L[rowc + (int64_t)(row0 + min(g + 4 * e, kw - 1)) * r];
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (g + 4 * e < kw) Ld[(g + 4 * e) * 65 + lane] = (lane < nrow) ? v[e] : 0.0;
    }
    double acc = 0.0;
    // the panel pieces are final (factorisation): panel p + 1's loads are issued before panel p's flag
    // wait and x loads, so one L round trip per task is exposed instead of one per panel
    double lv[16], ln[16];
    auto load_panel = [&](double (&dst)[16], int p) {
      const int cb = p * 64 + g * 16;
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) dst[cc] = L[rowc + (int64_t)min(cb + cc, w - 1) * r];
    };
    if (np > 0) load_panel(lv, 0);
    for (int p = 0; p < np; ++p) {
      if (p + 1 < np) load_panel(ln, p + 1);  // wave-uniform
      const int cb = p * 64 + g * 16;
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) lv[cc] = (lane < nrow && cb + cc < w) ? lv[cc] : 0.0;
      if (tid < 64) {
        const double xv = ll_get(T.xll + ((int64_t)flag_off[s] + p) * 128 + 2 * tid, epoch, err);
        xs[tid] = (p * 64 + tid < w) ? xv : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) acc += lv[cc] * xs[g * 16 + cc];
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) lv[cc] = ln[cc];
      __syncthreads();
    }
    part[g][lane] = acc;
    __syncthreads();
    if (g == 0) {
      double a = (lane < nrow) ? vwork[T.row_ptr[s] + row] - ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]))
                               : 0.0;
      a = tri_fwd64(a, Ld, kw, lane);
      if (pivot_blk) ll_put(T.xll + ((int64_t)flag_off[s] + i) * 128 + 2 * lane, a, epoch);  // every lane: 0 past nrow
      if (lane < nrow) {
        if (row < w)
          xi[f0 + row] = a;
        else
          uvec[T.uvec_off[s] + row - w] = a;
      }
    }
    __syncthreads();
  }
}

// Backward, big fronts, rows below the pivot block (independent of the panel chain): task =
// (front, panel p, 256-row chunk); writes bpart[(bp_off[front] + p * nchunk + chunk) * 64 + col] =
// sum over the chunk's rows of L(row, col) x(row).  The chain kernel sums the chunks in order.
__global__ __launch_bounds__(NT) void k_bwd_below(FrontTab T, const int32_t* __restrict__ list,
                                                  const int32_t* __restrict__ bp_off, const double* __restrict__ arena,
                                                  const double* __restrict__ xi, double* __restrict__ bpart) {
  __shared__ double tile[64 * 65];
  __shared__ double xr[64];
  __shared__ double part[4][64];
  int s, pc;
  task_of(list, s, pc);
  const int p = pc & 0xffff, chunk = pc >> 16;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  (void)f0;
  const double* __restrict__ L = arena + T.l_off[s];
  const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
  const int c0 = p * 64, kw = min(64, w - c0);
  const int nch = (r - w + BWD_CHUNK - 1) / BWD_CHUNK;
  const int R0 = w + chunk * BWD_CHUNK, R1 = min(r, R0 + BWD_CHUNK);
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  double acc = 0.0;
  // unconditional loads from clamped addresses, masked at the LDS stores; the next row block's loads
  // are issued before this block's products (one round trip exposed per task, not per block)
  double v[16], vn[16], xv = 0.0, xvn = 0.0;
  auto load_blk = [&](double (&dst)[16], double& x, int rb) {
    const int nr = min(64, R1 - rb);
    const int rc = rb + min(lane, nr - 1);
#pragma unroll
    for (int e = 0; e < 16; ++e) dst[e] = L[rc + (int64_t)(c0 + min(g + 4 * e, kw - 1)) * r];
    x = (tid < 64) ? xi[rows[rb + min(tid, nr - 1)]] : 0.0;
  };
  if (R0 < R1) load_blk(v, xv, R0);
  for (int rb = R0; rb < R1; rb += 64) {
    const int nr = min(64, R1 - rb);
#pragma unroll
    for (int e = 0; e < 16; ++e) tile[lane * 65 + g + 4 * e] = (lane < nr && g + 4 * e < kw) ? v[e] : 0.0;
    if (tid < 64) xr[tid] = (tid < nr) ? xv : 0.0;
    __syncthreads();
    if (rb + 64 < R1) load_blk(vn, xvn, rb + 64);  // block-uniform
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc += tile[(g * 16 + rr) * 65 + lane] * xr[g * 16 + rr];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = vn[e];
    xv = xvn;
    __syncthreads();
  }
  part[g][lane] = acc;
  __syncthreads();
  if (g == 0)
    bpart[((int64_t)bp_off[s] + (int64_t)p * nch + chunk) * 64 + lane] =
        (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// Backward, big fronts: task = (front, 64-column pivot panel p), processed from the last panel down.
// acc(cols) = D^{-1} y(cols) - L(below,cols)^T x(below) - sum_{q > p} L(q-block,cols)^T x_q; x_p = L_pp^{-T} acc.
__global__ __launch_bounds__(NT) void k_bwd_big(FrontTab T, const SolveTask* __restrict__ tasks, int ntasks,
                                                int32_t* counter, int32_t* flags, const int32_t* __restrict__ flag_off,
                                                int epoch, const double* __restrict__ arena,
                                                const double* __restrict__ D, double* __restrict__ xi,
                                                double* __restrict__ out, const int32_t* __restrict__ bp_off,
                                                const double* __restrict__ bpart, int32_t* err) {
  __shared__ int s_task;
  __shared__ double tile[64 * 65];
  __shared__ double xr[64];
  __shared__ double part[4][64];
  __shared__ double Ld[64 * 65];
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  for (;;) {
    if (tid == 0) s_task = atomicAdd(counter, 1);
    __syncthreads();
    const int t = s_task;
    __syncthreads();
    if (t >= ntasks) return;
    const int s = tasks[t].front, p = tasks[t].blk;
    const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
    const double* __restrict__ L = arena + T.l_off[s];
    const int c0 = p * 64, kw = min(64, w - c0);
    const int npan = (w + 63) >> 6;
    // diagonal block L(c0+i, c0+j) -> Ld[i*65+j] (unconditional clamped loads, masked at the store)
    {
      double v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = L[(c0 + min(lane, kw - 1)) + (int64_t)(c0 + min(g + 4 * e, kw - 1)) * r];
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (g + 4 * e < kw) Ld[lane * 65 + g + 4 * e] = (lane < kw) ? v[e] : 0.0;
    }
    double acc = 0.0;  // partial for column c0+lane over this wave's rows of each tile
    // pivot panels q = npan-1 .. p+1 (wait for each); the rows below come from k_bwd_below.  A tile's
    // L values are final: they are loaded before the wait for its x (the next tile's during this
    // tile's products), only the x values wait for the flag
    const int nq = npan - 1 - p;
    double v[16], vn[16];
    auto load_tile = [&](double (&dst)[16], int q) {
      const int rb = q * 64, nr = min(64, w - rb);
      const int rc = rb + min(lane, nr - 1);
#pragma unroll
      for (int e = 0; e < 16; ++e) dst[e] = L[rc + (int64_t)(c0 + min(g + 4 * e, kw - 1)) * r];
    };
    if (nq > 0) load_tile(v, npan - 1);
    for (int k = 0; k < nq; ++k) {
      const int q = npan - 1 - k;
      const int rb = q * 64, nr = min(64, w - rb);
      // stage the 64 x 64 tile L(rb.., c0..) (coalesced over rows) and the x values of its rows (the
      // panel's solution words, ll_get: they are the hand-off)
      {
        const double xv = (tid < 64) ? ll_get(T.xll + ((int64_t)flag_off[s] + q) * 128 + 2 * tid, epoch, err) : 0.0;
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (g + 4 * e < kw) tile[lane * 65 + g + 4 * e] = (lane < nr) ? v[e] : 0.0;
        if (tid < 64) xr[tid] = (tid < nr) ? xv : 0.0;
      }
      __syncthreads();
      if (k + 1 < nq) load_tile(vn, q - 1);  // block-uniform
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) acc += tile[(g * 16 + rr) * 65 + lane] * xr[g * 16 + rr];
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = vn[e];
      __syncthreads();
    }
    if (g == 0 && r > w) {
      const int nch = (r - w + BWD_CHUNK - 1) / BWD_CHUNK;
      const double* __restrict__ bp = bpart + ((int64_t)bp_off[s] + (int64_t)p * nch) * 64 + lane;
      double below = 0.0;
      for (int c = 0; c < nch; ++c) below += bp[c * 64];
      acc += below;
    }
    part[g][lane] = acc;
    __syncthreads();
    if (g == 0) {
      double a = 0.0;
      if (lane < kw) {
        const int c = f0 + c0 + lane;
        a = xi[c] / D[c] - ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]));
      }
      a = tri_bwd64(a, Ld, kw, lane);
      ll_put(T.xll + ((int64_t)flag_off[s] + p) * 128 + 2 * lane, a, epoch);  // every lane (masked by the readers)
      if (lane < kw) {
        const int c = f0 + c0 + lane;
        xi[c] = a;
        if (T.wout[s]) out[T.perm[c]] = a;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ big fronts, multi-right-hand-side
// The four big-front kernels above over the kc <= MW columns of a chunk: same task lists, same ticket order, same
// grid.  Every L entry, row index and gather index is loaded once per task and used for all kc columns; column
// j's operations and their order are those of the single-column kernel (kc is a uniform bound only), so a
// column has the bits the single-column kernels give it.  Column j of the gathered vector is at vwork + j
// vstride, of the below-row partials at bpart + j bstride; the hand-off words of (front, panel, column j) are
// the 128 words at xllm + ((flag_off[front] + panel) MW + j) 128, a buffer of the multi route alone (T.xll and
// its epochs belong to the single-column kernels).  Wave q polls / substitutes / writes columns q and q + 4.
__global__ __launch_bounds__(NT) void k_fwd_gather_m(FrontTab T, const int32_t* __restrict__ list, int kc,
                                                     const double* __restrict__ b, int64_t n,
                                                     const double* __restrict__ uvec, int64_t ustride,
                                                     double* __restrict__ vwork, int64_t vstride) {
  int s, chunk;
  task_of(list, s, chunk);
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int i = chunk * GAT_ROWS + threadIdx.x / GAT_G, gl = threadIdx.x & (GAT_G - 1);
  if (i >= r) return;  // whole groups leave together
  const int64_t e = T.row_ptr[s] + i;
  const int64_t p1 = T.sv_ptr[e + 1];
  const int64_t pi = T.perm[f0 + min(i, max(w - 1, 0))];
  double vi[MW];
#pragma unroll
  for (int j = 0; j < MW; ++j) vi[j] = 0.0;
  for (int64_t p = T.sv_ptr[e] + gl; p < p1; p += GAT_G) {
    const int64_t src = T.sv_src[p];
#pragma unroll
    for (int j = 0; j < MW; ++j)
      if (j < kc) vi[j] += uvec[j * ustride + src];
  }
#pragma unroll
  for (int j = 0; j < MW; ++j) {
    if (j >= kc) break;  // uniform
    double v = vi[j];
#pragma unroll
    for (int o = GAT_G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GAT_G);
    if (gl == 0) vwork[j * vstride + e] = v + ((i < w) ? b[j * n + pi] : 0.0);
  }
}

__global__ __launch_bounds__(NT) void k_fwd_big_m(FrontTab T, const SolveTask* __restrict__ tasks, int ntasks, int kc,
                                                  int32_t* counter, uint64_t* xllm, const int32_t* __restrict__ flag_off,
                                                  int epoch, const double* __restrict__ arena,
                                                  const double* __restrict__ vwork, int64_t vstride,
                                                  double* __restrict__ xi, int64_t N, double* __restrict__ uvec,
                                                  int64_t ustride, int32_t* err) {
  __shared__ int s_task;
  __shared__ double xs[MW][64];
  __shared__ double part[MW][4][64];
  __shared__ double Ld[64 * 65];
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  for (;;) {
    if (tid == 0) s_task = atomicAdd(counter, 1);
    __syncthreads();
    const int t = s_task;
    __syncthreads();
    if (t >= ntasks) return;
    const int s = tasks[t].front, i = tasks[t].blk;
    const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
    const double* __restrict__ L = arena + T.l_off[s];
    const int row0 = i * 64, nrow = min(64, r - row0);
    const int npan = (w + 63) >> 6;
    const int np = min(i, npan);
    const int row = row0 + lane;
    const bool pivot_blk = row0 < w;
    const int kw = pivot_blk ? min(64, w - row0) : 0;
    const int rowc = row0 + min(lane, nrow - 1);  // (unconditional loads from clamped addresses, masked after)
    if (kw > 0) {
      double v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = L[rowc + (int64_t)(row0 + min(g + 4 * e, kw - 1)) * r];
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (g + 4 * e < kw) Ld[(g + 4 * e) * 65 + lane] = (lane < nrow) ? v[e] : 0.0;
    }
    double acc[MW];
#pragma unroll
    for (int j = 0; j < MW; ++j) acc[j] = 0.0;
    uint64_t* const xw = xllm + (int64_t)flag_off[s] * MW * 128 + 2 * lane;
    double lv[16], ln[16];
    auto load_panel = [&](double (&dst)[16], int p) {
      const int cb = p * 64 + g * 16;
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) dst[cc] = L[rowc + (int64_t)min(cb + cc, w - 1) * r];
    };
    if (np > 0) load_panel(lv, 0);
    for (int p = 0; p < np; ++p) {
      if (p + 1 < np) load_panel(ln, p + 1);  // wave-uniform
      const int cb = p * 64 + g * 16;
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) lv[cc] = (lane < nrow && cb + cc < w) ? lv[cc] : 0.0;
      for (int j = g; j < kc; j += 4) {  // wave-uniform
        const double xv = ll_get(xw + ((int64_t)p * MW + j) * 128, epoch, err);
        xs[j][lane] = (p * 64 + lane < w) ? xv : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < MW; ++j) {
        if (j >= kc) break;  // uniform
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) acc[j] += lv[cc] * xs[j][g * 16 + cc];
      }
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) lv[cc] = ln[cc];
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < MW; ++j)
      if (j < kc) part[j][g][lane] = acc[j];
    __syncthreads();
    const int64_t uo = T.uvec_off[s], e0 = T.row_ptr[s] + row0 + min(lane, nrow - 1);
    for (int j = g; j < kc; j += 4) {  // wave-uniform
      const double vj = vwork[j * vstride + e0];
      double a = (lane < nrow) ? vj - ((part[j][0][lane] + part[j][1][lane]) + (part[j][2][lane] + part[j][3][lane])) : 0.0;
      a = tri_fwd64(a, Ld, kw, lane);
      if (pivot_blk) ll_put(xw + ((int64_t)i * MW + j) * 128, a, epoch);  // every lane: 0 past nrow
      if (lane < nrow) {
        if (row < w)
          xi[j * N + f0 + row] = a;
        else
          uvec[j * ustride + uo + row - w] = a;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(NT) void k_bwd_below_m(FrontTab T, const int32_t* __restrict__ list, int kc,
                                                    const int32_t* __restrict__ bp_off,
                                                    const double* __restrict__ arena, const double* __restrict__ xi,
                                                    int64_t N, double* __restrict__ bpart, int64_t bstride) {
  __shared__ double tile[64 * 65];
  __shared__ double xr[MW][64];
  __shared__ double part[MW][4][64];
  int s, pc;
  task_of(list, s, pc);
  const int p = pc & 0xffff, chunk = pc >> 16;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
  const int c0 = p * 64, kw = min(64, w - c0);
  const int nch = (r - w + BWD_CHUNK - 1) / BWD_CHUNK;
  const int R0 = w + chunk * BWD_CHUNK, R1 = min(r, R0 + BWD_CHUNK);
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const bool c1on = g + 4 < kc;  // wave g carries the x of columns g and g + 4 (kc >= 1: wave 0 always has one)
  const int64_t o0 = (int64_t)min(g, kc - 1) * N, o1 = (int64_t)min(g + 4, kc - 1) * N;
  double acc[MW];
#pragma unroll
  for (int j = 0; j < MW; ++j) acc[j] = 0.0;
  double v[16], vn[16], xv[2] = {0.0, 0.0}, xvn[2] = {0.0, 0.0};
  auto load_blk = [&](double (&dst)[16], double (&x)[2], int rb) {
    const int nr = min(64, R1 - rb);
    const int rc = rb + min(lane, nr - 1);
#pragma unroll
    for (int e = 0; e < 16; ++e) dst[e] = L[rc + (int64_t)(c0 + min(g + 4 * e, kw - 1)) * r];
    const int64_t xrow = rows[rc];
    x[0] = xi[o0 + xrow];
    x[1] = xi[o1 + xrow];
  };
  if (R0 < R1) load_blk(v, xv, R0);
  for (int rb = R0; rb < R1; rb += 64) {
    const int nr = min(64, R1 - rb);
#pragma unroll
    for (int e = 0; e < 16; ++e) tile[lane * 65 + g + 4 * e] = (lane < nr && g + 4 * e < kw) ? v[e] : 0.0;
    if (g < kc) xr[g][lane] = (lane < nr) ? xv[0] : 0.0;
    if (c1on) xr[g + 4][lane] = (lane < nr) ? xv[1] : 0.0;
    __syncthreads();
    if (rb + 64 < R1) load_blk(vn, xvn, rb + 64);  // block-uniform
    double tv[16];
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) tv[rr] = tile[(g * 16 + rr) * 65 + lane];
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      if (j >= kc) break;  // uniform
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) acc[j] += tv[rr] * xr[j][g * 16 + rr];
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = vn[e];
    xv[0] = xvn[0];
    xv[1] = xvn[1];
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < MW; ++j)
    if (j < kc) part[j][g][lane] = acc[j];
  __syncthreads();
  for (int j = g; j < kc; j += 4)  // wave-uniform
    bpart[j * bstride + ((int64_t)bp_off[s] + (int64_t)p * nch + chunk) * 64 + lane] =
        (part[j][0][lane] + part[j][1][lane]) + (part[j][2][lane] + part[j][3][lane]);
  (void)f0;
}

// LDS of k_bwd_big_m (dynamic: past the 64 KiB of a static carve): the tile, the diagonal block, kc x 64 x values;
// the per-column partials reuse the tile once its last products are done
constexpr int BIGM_TILE = 64 * 65;
constexpr int kBwdBigMultiLds = 8 * (2 * BIGM_TILE + MW * 64);
static_assert(MW * 4 * 64 <= BIGM_TILE, "the partials fit the tile");
static_assert(kBwdBigMultiLds <= kWorkgroupLds, "k_bwd_big_m's LDS");
__global__ __launch_bounds__(NT) void k_bwd_big_m(FrontTab T, const SolveTask* __restrict__ tasks, int ntasks, int kc,
                                                  int32_t* counter, uint64_t* xllm, const int32_t* __restrict__ flag_off,
                                                  int epoch, const double* __restrict__ arena,
                                                  const double* __restrict__ D, double* __restrict__ xi, int64_t N,
                                                  double* __restrict__ out, int64_t n,
                                                  const int32_t* __restrict__ bp_off, const double* __restrict__ bpart,
                                                  int64_t bstride, int32_t* err) {
  extern __shared__ __attribute__((aligned(16))) double bigm_lds[];
  __shared__ int s_task;
  double* const tile = bigm_lds;
  double* const Ld = tile + BIGM_TILE;
  double(*const xr)[64] = reinterpret_cast<double(*)[64]>(Ld + BIGM_TILE);
  double(*const part)[4][64] = reinterpret_cast<double(*)[4][64]>(tile);
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  for (;;) {
    if (tid == 0) s_task = atomicAdd(counter, 1);
    __syncthreads();
    const int t = s_task;
    __syncthreads();
    if (t >= ntasks) return;
    const int s = tasks[t].front, p = tasks[t].blk;
    const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
    const double* __restrict__ L = arena + T.l_off[s];
    const int c0 = p * 64, kw = min(64, w - c0);
    const int npan = (w + 63) >> 6;
    {
      double v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = L[(c0 + min(lane, kw - 1)) + (int64_t)(c0 + min(g + 4 * e, kw - 1)) * r];
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (g + 4 * e < kw) Ld[lane * 65 + g + 4 * e] = (lane < kw) ? v[e] : 0.0;
    }
    double acc[MW];
#pragma unroll
    for (int j = 0; j < MW; ++j) acc[j] = 0.0;
    uint64_t* const xw = xllm + (int64_t)flag_off[s] * MW * 128 + 2 * lane;
    const int nq = npan - 1 - p;
    double v[16], vn[16];
    auto load_tile = [&](double (&dst)[16], int q) {
      const int rb = q * 64, nr = min(64, w - rb);
      const int rc = rb + min(lane, nr - 1);
#pragma unroll
      for (int e = 0; e < 16; ++e) dst[e] = L[rc + (int64_t)(c0 + min(g + 4 * e, kw - 1)) * r];
    };
    if (nq > 0) load_tile(v, npan - 1);
    for (int k = 0; k < nq; ++k) {
      const int q = npan - 1 - k;
      const int rb = q * 64, nr = min(64, w - rb);
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (g + 4 * e < kw) tile[lane * 65 + g + 4 * e] = (lane < nr) ? v[e] : 0.0;
      for (int j = g; j < kc; j += 4) {  // wave-uniform
        const double xv = ll_get(xw + ((int64_t)q * MW + j) * 128, epoch, err);
        xr[j][lane] = (lane < nr) ? xv : 0.0;
      }
      __syncthreads();
      if (k + 1 < nq) load_tile(vn, q - 1);  // block-uniform
      double tv[16];
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) tv[rr] = tile[(g * 16 + rr) * 65 + lane];
#pragma unroll
      for (int j = 0; j < MW; ++j) {
        if (j >= kc) break;  // uniform
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc[j] += tv[rr] * xr[j][g * 16 + rr];
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = vn[e];
      __syncthreads();
    }
    // wave q finishes columns q and q + 4: their below-row partials (k_bwd_below_m's chunks in chunk order) are
    // loaded before the barrier and added to wave 0's partial, as k_bwd_big adds them to wave 0's acc
    double below[2] = {0.0, 0.0};
    if (r > w) {
      const int nch = (r - w + BWD_CHUNK - 1) / BWD_CHUNK;
      const double* __restrict__ bp = bpart + ((int64_t)bp_off[s] + (int64_t)p * nch) * 64 + lane;
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (g + 4 * h < kc)
          for (int c = 0; c < nch; ++c) below[h] += bp[(g + 4 * h) * bstride + c * 64];
    }
#pragma unroll
    for (int j = 0; j < MW; ++j)
      if (j < kc) part[j][g][lane] = acc[j];
    __syncthreads();
    const int c = f0 + c0 + min(lane, kw - 1);
    const double dc = D[c];
    const int64_t pc = T.perm[c];
    const bool wo = T.wout[s];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = g + 4 * h;
      if (j >= kc) break;  // wave-uniform
      double a = 0.0;
      if (lane < kw) {
        const double p0 = (r > w) ? part[j][0][lane] + below[h] : part[j][0][lane];
        a = xi[j * N + c] / dc - ((p0 + part[j][1][lane]) + (part[j][2][lane] + part[j][3][lane]));
      }
      a = tri_bwd64(a, Ld, kw, lane);
      ll_put(xw + ((int64_t)p * MW + j) * 128, a, epoch);  // every lane (masked by the readers)
      if (lane < kw) {
        xi[j * N + c] = a;
        if (wo) out[j * n + pc] = a;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ tree solves (dependency-driven)
// ONE launch per direction covers every "tree" front (LDLSolver ctor: phase-1 fronts whose L panel
// fits LDS and whose children are leaves of <= 32 rows — done by the level-0 launches — or tree
// fronts).  A workgroup takes the next front in topological order from an atomic ticket (every
// front it waits on holds an earlier ticket, taken by a running workgroup: no deadlock at any grid
// size or residency), stages its L panel into LDS BEFORE waiting, then polls its dependencies'
// flags (forward: tree children; backward: the tree parent), substitutes and publishes.  Hand-off
// (MI355X_MICROARCH.md "inter-workgroup visibility", form R1): the payload (xi, uvec) is stored
// write-through (sc1) by the ONE publishing wave, which drains it (vmcnt 0) before its lane 0 stores
// the flag; every consumer load of handed-off bytes is an sc1 load behind the poll and a workgroup
// barrier — no agent-scope fences on the dependency chain.

// Tree-solve substitutions, one wave, 16 pivots per block, mask-free: the panels are staged with the
// upper triangle + diagonal zeroed and the pivot columns zero-padded to a multiple of 16, so every
// block loads its L entries unconditionally (16-byte LDS reads, immediate offsets) and the
// dependency chain is one readlane + one fma per pivot.
// dynamic LDS of the tree solves (+ ~2 KB static): two 256-thread workgroups per CU
__device__ __forceinline__ int tree_ldt(int w) { return ((w + 15) & ~15) + 2; }  // forward: row-major ld
__device__ __forceinline__ int tree_ldc(int r) { return ((r + 31) & ~31) + 2; }  // backward: col-major ld

// forward staging: LT[i * ldt + t] = L(i, t) for t < min(i, w), else 0 (t < w16)
template <int NTH = NT>
__device__ __forceinline__ void stage_rowmajor(const double* __restrict__ L, double* LT, int r, int w, int ldt) {
  const int w16 = (w + 15) & ~15;
  const int nel = r * w16;
  ColWalk wk(threadIdx.x, r, NTH);
  for (int base = 0; base < nel; base += NTH * 16) {
    double v[16];
    int dst[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int q = base + k * NTH + threadIdx.x;
      v[k] = (q < nel && wk.j < w && wk.i > wk.j) ? L[q] : 0.0;
      dst[k] = (q < nel) ? wk.i * ldt + wk.j : -1;
      wk.next();
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (dst[k] >= 0) LT[dst[k]] = v[k];
  }
}

// backward staging: LC[j * ldc + t] = L(t, j) for t > j, else 0 (j < w, t < r)
__device__ __forceinline__ void stage_colmajor(const double* __restrict__ L, double* LC, int r, int w, int ldc) {
  const int nel = r * w;
  ColWalk wk(threadIdx.x, r);
  for (int base = 0; base < nel; base += NT * 16) {
    double v[16];
    int dst[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int q = base + k * NT + threadIdx.x;
      v[k] = (q < nel && wk.i > wk.j) ? L[q] : 0.0;
      dst[k] = (q < nel) ? wk.j * ldc + wk.i : -1;
      wk.next();
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (dst[k] >= 0) LC[dst[k]] = v[k];
  }
  const int pad = ((w + 15) & ~15) - r;  // the last pivot block may reach past row r - 1: zero rows
  for (int q = threadIdx.x; q < w * pad; q += NT) LC[(q / pad) * ldc + r + q % pad] = 0.0;
}

template <int HB>
__device__ __forceinline__ void fwd_block_t(double (&v)[3], const double* LT, int ldt, int r, int t0, int lane) {
  double lb[3][16];
#pragma unroll
  for (int h = HB; h < 3; ++h) {
    const double2* rp = reinterpret_cast<const double2*>(LT + min(lane + 64 * h, r - 1) * ldt + t0);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const double2 q = rp[m];
      lb[h][2 * m] = q.x;
      lb[h][2 * m + 1] = q.y;
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const double xt = readlane_f64(v[HB], (t0 & 63) + k);
#pragma unroll
    for (int h = HB; h < 3; ++h) v[h] = fma(-lb[h][k], xt, v[h]);
  }
}

// forward: v[i] -= L(i, t) v[t] for i > t, t < w (columns >= w are zero)
__device__ __forceinline__ void fwd_subst_t(double (&v)[3], const double* LT, int ldt, int r, int w, int lane) {
  for (int t0 = 0; t0 < w; t0 += 16) {
    if (t0 < 64)
      fwd_block_t<0>(v, LT, ldt, r, t0, lane);
    else if (t0 < 128)
      fwd_block_t<1>(v, LT, ldt, r, t0, lane);
    else
      fwd_block_t<2>(v, LT, ldt, r, t0, lane);
  }
}

template <int HB>
__device__ __forceinline__ void bwd_block_c(double (&v)[3], const double* LC, int ldc, int w, int t0, int lane) {
  double lb[HB + 1][16];
#pragma unroll
  for (int h = 0; h <= HB; ++h) {
    const double2* cp = reinterpret_cast<const double2*>(LC + min(lane + 64 * h, w - 1) * ldc + t0);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const double2 q = cp[m];
      lb[h][2 * m] = q.x;
      lb[h][2 * m + 1] = q.y;
    }
  }
#pragma unroll
  for (int k = 15; k >= 0; --k) {  // lanes >= w hold 0 and stay 0 until k < kb
    const double xt = readlane_f64(v[HB], (t0 & 63) + k);
#pragma unroll
    for (int h = 0; h <= HB; ++h) v[h] = fma(-lb[h][k], xt, v[h]);
  }
}

// backward (transposed): v[j] -= L(t, j) v[t] for j < t, t = w-1 .. 1
__device__ __forceinline__ void bwd_subst_c(double (&v)[3], const double* LC, int ldc, int w, int lane) {
  for (int t0 = ((w - 1) >> 4) << 4; t0 >= 0; t0 -= 16) {
    if (t0 < 64)
      bwd_block_c<0>(v, LC, ldc, w, t0, lane);
    else if (t0 < 128)
      bwd_block_c<1>(v, LC, ldc, w, t0, lane);
    else
      bwd_block_c<2>(v, LC, ldc, w, t0, lane);
  }
}

// backward (transposed) on the forward's row-major panel: v[j] -= L(t, j) v[t] for j < t, t = w-1 .. 0,
// L(t, j) = LT[t ldt + j] — the same fma sequence as bwd_subst_c (bitwise the same x).  Used by the
// forward kernel for an elimination-tree root (r == w) whose panel it already holds in LDS.
template <int HB>
__device__ __forceinline__ void bwd_block_t(double (&v)[3], const double* LT, int ldt, int w, int t0, int lane) {
  double lb[HB + 1][16];
#pragma unroll
  for (int h = 0; h <= HB; ++h) {
    const int j = min(lane + 64 * h, w - 1);
#pragma unroll
    for (int k = 0; k < 16; ++k) lb[h][k] = LT[min(t0 + k, w - 1) * ldt + j];
  }
#pragma unroll
  for (int k = 15; k >= 0; --k) {
    const double xt = readlane_f64(v[HB], (t0 & 63) + k);
#pragma unroll
    for (int h = 0; h <= HB; ++h) v[h] = fma(-lb[h][k], xt, v[h]);
  }
}
__device__ __forceinline__ void bwd_subst_t(double (&v)[3], const double* LT, int ldt, int w, int lane) {
  for (int t0 = ((w - 1) >> 4) << 4; t0 >= 0; t0 -= 16) {
    if (t0 < 64)
      bwd_block_t<0>(v, LT, ldt, w, t0, lane);
    else if (t0 < 128)
      bwd_block_t<1>(v, LT, ldt, w, t0, lane);
    else
      bwd_block_t<2>(v, LT, ldt, w, t0, lane);
  }
}

// ---- Chunked tree-solve fronts: medium fronts (SMALL_SOLVE_MAX < r <= kFactTreeMedMax) and every
// front whose whole panel would not fit the tree solves' LDS budget (TREE_SOLVE_LDS: two workgroups per
// CU, so the 272 level-1/2 fronts of ex10 all start at once — with one per CU, 16 of them waited for
// a level-1 front to retire).  The L panel is streamed in 16-column chunks, double-buffered: wave 0
// substitutes chunk c while waves 1..3 stage chunk c +- 1.  v (forward) / x (backward) stay in wave 0's
// registers, 4 rows per lane.
constexpr int MCW = 16, MLDT = MCW + 2;           // forward chunk: pivot columns, row-major ld
constexpr int MFBUF = MED_SOLVE_MAX * MLDT;       // doubles per forward chunk buffer
constexpr int MLDC = MED_SOLVE_MAX + 2;           // backward chunk: col-major ld
constexpr int MBBUF = MCW * MLDC;                 // doubles per backward chunk buffer
constexpr int MED_FWD_LDS = 2 * MFBUF, MED_BWD_LDS = 2 * MBBUF + 2 * MED_SOLVE_MAX;  // doubles
static_assert(8 * MED_FWD_LDS <= TREE_SOLVE_LDS && 8 * MED_BWD_LDS <= TREE_SOLVE_LDS,
              "chunked tree-solve buffers fit the tree launches' LDS");

// rows [ra, r) x columns [c0, c0 + MCW) of L (ld r) -> LT[(i - ra) MLDT + (t - c0)] = L(i, t) for
// t < w and i > t, else 0; threads lt = 0 .. nthr - 1 of the caller's group
__device__ __forceinline__ void stage_fwd_chunk(const double* __restrict__ L, double* LT, int r, int w, int ra, int c0,
                                                int lt, int nthr) {
  const int nrow = r - ra, nel = nrow * MCW;
  ColWalk wk(lt, nrow, nthr);
  for (int base = 0; base < nel; base += nthr * 8) {
    double v[8];
    int dst[8];
    bool ok[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int q = base + k * nthr + lt, i = ra + wk.i, t = c0 + wk.j;
      ok[k] = t < w && i > t;
      v[k] = L[min(i, r - 1) + (int64_t)min(t, w - 1) * r];  // clamped, in range: masked below
      dst[k] = q < nel ? wk.i * MLDT + wk.j : -1;
      wk.next();
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (dst[k] >= 0) LT[dst[k]] = ok[k] ? v[k] : 0.0;
  }
}

template <int HB>
__device__ __forceinline__ void fwd_block_m(double (&v)[4], const double* LT, int r, int ra, int tc, int t0, int lane) {
  double lb[4][16];
#pragma unroll
  for (int h = HB; h < 4; ++h) {
    const double2* rp = reinterpret_cast<const double2*>(LT + (min(lane + 64 * h, r - 1) - ra) * MLDT + tc);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const double2 q = rp[m];
      lb[h][2 * m] = q.x;
      lb[h][2 * m + 1] = q.y;
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const double xt = readlane_f64(v[HB], (t0 & 63) + k);
#pragma unroll
    for (int h = HB; h < 4; ++h) v[h] = fma(-lb[h][k], xt, v[h]);
  }
}

// column chunk [c0, c0 + MCW) of L (ld r), rows [c0, r) -> LC[(j - c0) MLDC + (t - c0)] = L(t, j) for
// j < w and t > j, else 0
__device__ __forceinline__ void stage_bwd_chunk(const double* __restrict__ L, double* LC, int r, int w, int c0, int lt,
                                                int nthr) {
  const int nrow = r - c0, nel = nrow * MCW;
  ColWalk wk(lt, nrow, nthr);
  for (int base = 0; base < nel; base += nthr * 8) {
    double v[8];
    int dst[8];
    bool ok[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int q = base + k * nthr + lt, t = c0 + wk.i, j = c0 + wk.j;
      ok[k] = j < w && t > j;
      v[k] = L[min(t, r - 1) + (int64_t)min(j, w - 1) * r];
      dst[k] = q < nel ? wk.j * MLDC + wk.i : -1;
      wk.next();
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (dst[k] >= 0) LC[dst[k]] = ok[k] ? v[k] : 0.0;
  }
}

// forward solve of a medium tree front (all NT threads; v0: the gathered initial values of its rows)
__device__ __forceinline__ void fwd_med_front(const FrontTab& T, int s, const double* __restrict__ arena, double* Ls,
                                              const double* v0, double* xi, double* uvec, int32_t* tflags, int epoch) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const double* __restrict__ L = arena + T.l_off[s];
  const int nch = (((w + 15) & ~15) + MCW - 1) / MCW;
  double* buf[2] = {Ls, Ls + MFBUF};
  stage_fwd_chunk(L, buf[0], r, w, 0, 0, tid, NT);
  double v[4];
  double* dst[4];
  uvec_dsts<4>(T, s, w, r, f0, wv == 0, lane, uvec, xi, dst);
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int i = lane + 64 * h;
    v[h] = (i < r) ? v0[i] : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int c0 = c * MCW;
    if (wv == 0) {
      const int ra = (c0 >> 6) << 6;
      const double* LT = buf[c & 1];
      const int tend = min(c0 + MCW, (w + 15) & ~15);
      for (int t0 = c0; t0 < tend; t0 += 16) {
        const int tc = t0 - c0;
        switch (t0 >> 6) {
          case 0: fwd_block_m<0>(v, LT, r, ra, tc, t0, lane); break;
          case 1: fwd_block_m<1>(v, LT, r, ra, tc, t0, lane); break;
          case 2: fwd_block_m<2>(v, LT, r, ra, tc, t0, lane); break;
          default: fwd_block_m<3>(v, LT, r, ra, tc, t0, lane); break;
        }
      }
    } else if (c + 1 < nch) {
      const int c1 = c0 + MCW;
      stage_fwd_chunk(L, buf[(c + 1) & 1], r, w, (c1 >> 6) << 6, c1, tid - 64, NT - 64);
    }
    __syncthreads();
  }
  if (wv == 0) {
#pragma unroll
    for (int h = 0; h < 4; ++h)
      if (lane + 64 * h < r) st_sc1(dst[h], v[h]);
    publish_sc1(&tflags[s], epoch);
  }
  __syncthreads();
}

// backward solve of a medium tree front (all NT threads): chunks from the last to the first; xall holds
// the final x of every row below the current chunk (the ancestors' rows, then this front's later pivots)
__device__ __forceinline__ void bwd_med_front(const FrontTab& T, int s, const double* __restrict__ arena,
                                              const double* __restrict__ D, double* Ls, double* xi, double* out,
                                              const int32_t* __restrict__ pdep, int t, int32_t* tflags, int epoch,
                                              int32_t* err) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s], nb = r - w;
  const double* __restrict__ L = arena + T.l_off[s];
  double* buf[2] = {Ls, Ls + MBBUF};
  double* xall = Ls + 2 * MBBUF;            // r doubles
  double* ownv = xall + MED_SOLVE_MAX;      // w doubles: the forward values / d
  const int nch = (w + MCW - 1) / MCW;
  // symbolic / previous-launch data before the wait: the rows below, the own values, the last chunk
  const int rk = (tid < nb) ? T.rows[T.row_ptr[s] + w + tid] : 0;
  if (tid < w) ownv[tid] = xi[f0 + tid] / D[f0 + tid];
  stage_bwd_chunk(L, buf[(nch - 1) & 1], r, w, (nch - 1) * MCW, tid, NT);
  if (tid < 64 && pdep[t] >= 0) poll_deps(pdep, t, t + 1, tflags, epoch, err);
  __syncthreads();
  if (tid < nb) xall[w + tid] = ld_sc1(xi + rk);
  __syncthreads();
  const bool wo = T.wout[s];
  constexpr int NG = 64 / MCW;  // lane groups of the wave: group g sums the rows t = c1 + g (mod NG)
  const int jl = lane % MCW, grp = lane / MCW;
  for (int c = nch - 1; c >= 0; --c) {
    const int c0 = c * MCW, c1 = min(c0 + MCW, w), j = c0 + jl;
    if (wv == 0) {
      const double* LC = buf[c & 1] + jl * MLDC;
      // rows below the chunk (NG lane groups, interleaved rows), then the chunk's own triangle
      double a0 = 0.0, a1 = 0.0;
      int q = c1 + grp;
      for (; q + NG < r; q += 2 * NG) {
        a0 = fma(LC[q - c0], xall[q], a0);
        a1 = fma(LC[q + NG - c0], xall[q + NG], a1);
      }
      for (; q < r; q += NG) a0 = fma(LC[q - c0], xall[q], a0);
      const double part = a0 + a1;
      double p[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) p[g] = __shfl(part, jl + MCW * g, 64);
      static_assert(NG == 4, "bwd_med_front: four lane groups");
      const double acc = (p[0] + p[1]) + (p[2] + p[3]);  // the same fixed order in every lane group
      double x = (j < w) ? ownv[min(j, w - 1)] - acc : 0.0;
      for (int tt = c1 - 1; tt > c0; --tt) {  // x_j -= L(tt, j) x_tt, j < tt
        const double xt = readlane_f64(x, tt - c0);
        x = fma(-LC[tt - c0], xt, x);
      }
      if (grp == 0 && j < w) {
        xall[j] = x;
        st_sc1(xi + f0 + j, x);
        if (wo) out[T.perm[f0 + j]] = x;
      }
    } else if (c > 0) {
      stage_bwd_chunk(L, buf[(c - 1) & 1], r, w, (c - 1) * MCW, tid - 64, NT - 64);
    }
    __syncthreads();
  }
  if (tid < 64) publish_sc1(&tflags[s], epoch);
  __syncthreads();
}

// The micro leaves under tree fronts as flat launches: LPL lanes per leaf, each lane forms
// x0, x1 itself (the same loads) and takes rows a = j, j + LPL, ...; the leaf record carries every
// index, so a lane's loads are one dependent level deep (record -> b, L, row table).  Forward before
// k_fwd_tree (it gathers the update entries from gbuf), backward after k_bwd_tree (final ancestors).
constexpr int LPL = 4, LROWS = (32 + LPL - 1) / LPL;
__global__ __launch_bounds__(NT) void k_fwd_leaves(const SolveLeaf* __restrict__ lv, int nleaf,
                                                   const int2* __restrict__ lrow, const double* __restrict__ arena,
                                                   const double* __restrict__ b, double* __restrict__ xi,
                                                   double* __restrict__ gbuf) {
  const int gid = blockIdx.x * NT + threadIdx.x;
  const int k = gid / LPL, j = gid % LPL;
  if (k >= nleaf) return;
  const SolveLeaf L = lv[k];
  const int r = L.rw & 255, w = L.rw >> 8, u = r - w;
  const double* __restrict__ P = arena + L.loff;
  // unconditional loads from clamped in-range addresses (a leaf with no update rows reads its own
  // pivot entry; the row table is padded by one record), masked at the use
  double p[LROWS], q[LROWS];
  int d[LROWS];
#pragma unroll
  for (int m = 0; m < LROWS; ++m) {
    const int a = max(min(j + LPL * m, u - 1), 0);
    p[m] = P[min(w + a, r - 1)];
    q[m] = P[(w == 2) ? min(w + a, r - 1) + r : 0];
    d[m] = lrow[L.roff + a].x;
  }
  const double b0 = b[L.p0], b1r = b[(w == 2) ? L.p1 : L.p0], l10r = P[1 < r ? 1 : 0];
  const double b1 = (w == 2) ? b1r : 0.0, l10 = (w == 2) ? l10r : 0.0;
  const double x0 = b0, x1 = (w == 2) ? b1 - l10 * x0 : 0.0;
  if (j == 0) {
    xi[L.f0] = x0;
    if (w == 2) xi[L.f0 + 1] = x1;
  }
#pragma unroll
  for (int m = 0; m < LROWS; ++m)
    if (j + LPL * m < u) gbuf[d[m]] = (0.0 - p[m] * x0) - (w == 2 ? q[m] : 0.0) * x1;
}

__global__ __launch_bounds__(NT) void k_bwd_leaves(const SolveLeaf* __restrict__ lv, int nleaf,
                                                   const int2* __restrict__ lrow, const double* __restrict__ arena,
                                                   const double* __restrict__ D, double* __restrict__ xi,
                                                   double* __restrict__ out) {
  const int gid = blockIdx.x * NT + threadIdx.x;
  const int k = gid / LPL, j = gid % LPL;
  if (k >= nleaf) return;  // whole leaves only: the LPL lanes of a leaf exit together
  const SolveLeaf L = lv[k];
  const int r = L.rw & 255, w = L.rw >> 8, u = r - w;
  const double* __restrict__ P = arena + L.loff;
  // unconditional loads from clamped in-range addresses, masked at the use (as k_fwd_leaves)
  int src[LROWS];
#pragma unroll
  for (int m = 0; m < LROWS; ++m) src[m] = lrow[L.roff + max(min(j + LPL * m, u - 1), 0)].y;
  double p[LROWS], q[LROWS], x[LROWS];
#pragma unroll
  for (int m = 0; m < LROWS; ++m) {
    const int a = max(min(j + LPL * m, u - 1), 0);
    p[m] = P[min(w + a, r - 1)];
    q[m] = P[(w == 2) ? min(w + a, r - 1) + r : 0];
    x[m] = xi[src[m]];  // the tree fronts' final x (previous launch)
  }
  // the pivots' own entries, for lane 0's tail (loaded with the rest)
  const int f1 = L.f0 + (w == 2 ? 1 : 0);
  const double l10r = P[1 < r ? 1 : 0], xf0 = xi[L.f0], df0 = D[L.f0], xf1 = xi[f1], df1 = D[f1];
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int m = 0; m < LROWS; ++m)
    if (j + LPL * m < u) {
      a0 = fma(p[m], x[m], a0);
      a1 = fma(q[m], x[m], a1);
    }
  // ((lane 0 + lane 1) + (lane 2 + lane 3)): a fixed order
  a0 += __shfl_xor(a0, 1, LPL);
  a1 += __shfl_xor(a1, 1, LPL);
  a0 += __shfl_xor(a0, 2, LPL);
  a1 += __shfl_xor(a1, 2, LPL);
  if (j != 0) return;
  const double l10 = (w == 2) ? l10r : 0.0;
  const double v1 = (w == 2) ? xf1 / df1 - a1 : 0.0;
  const double v0 = xf0 / df0 - a0 - l10 * v1;
  xi[L.f0] = v0;
  out[L.p0] = v0;
  if (w == 2) {
    xi[L.f0 + 1] = v1;
    out[L.p1] = v1;
  }
}

// Tree solves over CHAIN tasks: a task is a maximal chain of tree fronts in which every front is the
// only tree child of the next (LDLSolver ctor), solved back to back by one workgroup (forward deepest
// first, backward top first) together with the folded micro leaves of its fronts: inside a chain no
// flag hand-off, no second workgroup start, and the leaves need no launch of their own.  Only the
// chain's ends talk to other workgroups (forward: the tree children of its deepest front, poll; its top
// publishes.  Backward: the top polls its tree parent; every front publishes for the tasks below).
// Inside the chain a front's stores (update entries, x) are drained (vmcnt 0) before the barrier that
// precedes the next front's sc1 loads of them.
// Dynamic LDS of the tree solve kernels: L panel | gather staging.
__global__ __launch_bounds__(NT) void k_fwd_tree(FrontTab T, const int32_t* __restrict__ cptr, const int32_t* __restrict__ clist,
                                                 int nt, const int32_t* __restrict__ dep_ptr, const int32_t* __restrict__ dep,
                                                 int32_t* counter, int32_t* tflags, int epoch, int lds_doubles,
                                                 const double* __restrict__ arena, const double* __restrict__ b,
                                                 double* xi, double* uvec, int32_t* err, int64_t* dbg,
                                                 const uint8_t* __restrict__ rootbwd, const double* __restrict__ Dg,
                                                 const uint8_t* __restrict__ tchunk, const uint8_t* __restrict__ tside,
                                                 const int32_t* rdone, int nrd, int repoch) {
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  __shared__ double v0s[MED_SOLVE_MAX];
  __shared__ int s_task;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_task = atomicAdd(counter, 1);
    if (s_task == nt - 1) atomicExch(counter, 0);  // every ticket taken: ready for the next launch
  }
  __syncthreads();
  const int t = s_task;
  if (t >= nt) return;
  int64_t* dg = dbg ? dbg + 8 * t : nullptr;
  if (dg && tid == 0) dg[0] = wall_clock64();
  const int q0 = cptr[t], q1 = cptr[t + 1];
  if (dg) {
    __syncthreads();
    if (tid == 0) dg[1] = wall_clock64();
  }
  for (int q = q0; q < q1; ++q) {
    const int s = clist[q];
    const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
    const bool med = tchunk[s];  // chunked front: panel streamed after the gather
    const int ldt = tree_ldt(w);
    double* stg = med ? Ls : Ls + r * ldt;
    const int cap = med ? (lds_doubles / NT) * NT : ((lds_doubles - r * ldt) / NT) * NT;
    // a root factorised on the side stream (LDLSolver::root_async_, first solve after the
    // factorisation): its panel and pivots only after the tail's done flags
    const bool sw = nrd > 0 && tside[t] && q == q1 - 1;
    if (!med && !sw) stage_rowmajor(arena + T.l_off[s], Ls, r, w, ldt);
    // everything that does not depend on the children is loaded before the wait: the gather range
    // (symbolic) and this front's own right-hand side entries (the input b)
    const int64_t e0 = T.row_ptr[s];
    const int64_t P0 = T.sv_ptr[e0], P1 = T.sv_ptr[e0 + r];
    const int64_t pr0 = (tid < r) ? T.sv_ptr[e0 + tid] : 0, pr1 = (tid < r) ? T.sv_ptr[e0 + tid + 1] : 0;
    const double init = (tid < r) ? fwd_init(T, s, tid, w, f0, b) : 0.0;
    double* udst[3];  // wave 0: where its rows' results go (x for pivots, the parent's gather slot below)
    uvec_dsts<3>(T, s, w, r, f0, tid < 64, tid & 63, uvec, xi, udst);
    // an elimination-tree root (r == w) also runs its backward substitution here:
    // its pivots and the caller's positions are loaded before the wait
    const bool rb = q == q1 - 1 && rootbwd[t];
    double dpiv[3];
    int pj[3];
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int j = min((tid & 63) + 64 * h, max(w - 1, 0));
      dpiv[h] = (rb && tid < 64) ? Dg[f0 + j] : 1.0;
      pj[h] = (rb && tid < 64) ? T.perm[f0 + j] : 0;
    }
    // initial vector: the children scattered their update entries into this front's contiguous range
    // gbuf[P0, P1) in row order, each row's entries from childless children (the leaves, solved by an
    // earlier launch) first and from its tree children (this launch) last (sv_nt, LDLSolver ctor).  The
    // leaf part is summed BEFORE the wait: staged through LDS (16 coalesced loads in flight per
    // thread), thread i sums row i's leaf entries in order (4 partial sums); after the wait only the
    // tree children's few entries per row are loaded (one round trip)
    const int ntr = (tid < r) ? (int)T.sv_nt[e0 + tid] : 0;
    const int64_t pl1 = pr1 - ntr;  // the row's leaf part: [pr0, pl1)
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    for (int64_t base = P0; base < P1; base += cap) {
      const int n = (int)min((int64_t)cap, P1 - base);
      for (int g0 = 0; g0 < n; g0 += NT * 16) {
        double tmp[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int g = g0 + k * NT + tid;
          tmp[k] = (g < n) ? ld_sc1(T.gbuf + base + g) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int g = g0 + k * NT + tid;
          if (g < n) stg[g] = tmp[k];
        }
      }
      __syncthreads();
      const int lo = (int)(max(pr0, base) - base), hi = (int)(min(pl1, base + n) - base);
      int p = lo;
      for (; p + 3 < hi; p += 4) {
        c0 += stg[p];
        c1 += stg[p + 1];
        c2 += stg[p + 2];
        c3 += stg[p + 3];
      }
      for (; p < hi; ++p) c0 += stg[p];
      __syncthreads();
    }
    if (q == q0 && tid < 64) poll_deps(dep, dep_ptr[t], dep_ptr[t + 1], tflags, epoch, err);
    __syncthreads();  // + the previous front's / the leaves' drained stores (vmcnt 0 before it)
    if (sw) {
      if (tid < 64) {
        const int lane = tid;
        int spins = 0;
        for (;;) {
          const bool ok = lane >= nrd ||
                          __hip_atomic_load(rdone + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == repoch;
          if (__all(ok)) break;
          __builtin_amdgcn_s_sleep(1);
          if (++spins > (1 << 25)) {
            if (lane == 0) atomicOr(err, kErrHandoff);
            break;
          }
        }
      }
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      if (!med) stage_rowmajor(arena + T.l_off[s], Ls, r, w, ldt);
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const int j = min((tid & 63) + 64 * h, max(w - 1, 0));
        dpiv[h] = (rb && tid < 64) ? Dg[f0 + j] : 1.0;
      }
      __syncthreads();
    }
    if (dg && tid == 0 && q == q0) dg[2] = wall_clock64();
    double ct = 0.0;  // the tree children's entries of this row, in order
    for (int k = 0; k < ntr; ++k) ct += ld_sc1(T.gbuf + pl1 + k);
    if (tid < r) v0s[tid] = (((c0 + c1) + (c2 + c3)) + ct) + init;
    __syncthreads();
    if (med) {
      fwd_med_front(T, s, arena, Ls, v0s, xi, uvec, tflags, epoch);
      continue;
    }
    if (dg && tid == 0 && q == q1 - 1) dg[3] = wall_clock64();
    if (tid < 64) {
      const int lane = tid;
      double v[3];
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const int i = lane + 64 * h;
        v[h] = (i < r) ? v0s[i] : 0.0;
      }
      fwd_subst_t(v, Ls, ldt, r, w, lane);
      if (dg && tid == 0 && q == q1 - 1) dg[4] = wall_clock64();
      if (rb) {  // k_bwd_tree's work for this root: x = L^-T (D^-1 y), published with the backward epoch
#pragma unroll
        for (int h = 0; h < 3; ++h) v[h] = (lane + 64 * h < w) ? v[h] / dpiv[h] : 0.0;
        bwd_subst_t(v, Ls, ldt, w, lane);
        double* out = const_cast<double*>(b);  // the caller's vector: x at this root's pivots (read by no other task)
#pragma unroll
        for (int h = 0; h < 3; ++h) {
          const int j = lane + 64 * h;
          if (j < w) {
            st_sc1(xi + f0 + j, v[h]);
            if (T.wout[s]) out[pj[h]] = v[h];
          }
        }
        publish_sc1(&tflags[s], epoch + 1);
      } else {
#pragma unroll
        for (int h = 0; h < 3; ++h) {
          const int i = lane + 64 * h;
          if (i < r) st_sc1(udst[h], v[h]);
        }
        if (q == q1 - 1)
          publish_sc1(&tflags[s], epoch);  // the chain's top: its tree parent is another task's
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    __syncthreads();  // wave 0 is done with Ls; its stores are drained
  }
  if (dg && tid == 0) {
    dg[5] = wall_clock64();
    dg[6] = clist[q1 - 1];
    dg[7] = T.nrows[clist[q1 - 1]];
  }
}

// The big elimination-tree roots of the tree solves (LDLSolver::nroot_task_: r == w, panel beyond the
// tree launches' 76 KB; ex10's 120-column coupling root), one 1024-thread workgroup each, after the
// forward tree launch (every child has scattered its update entries): the panel staged row-major in
// one round of loads, each row's gather segment summed by four threads (strided, all loads in
// flight), then the forward and backward substitutions on the staged panel (k_fwd_tree's root-backward
// path: the same fma sequences).  In k_fwd_tree the root's single 256-thread workgroup staged 125 KB
// of panel and its ~20k gather entries through the LDS left beside the panel: 26-34 us per solve.
constexpr int RSN = 1024;
__global__ __launch_bounds__(RSN) void k_root_solve(FrontTab T, const int32_t* __restrict__ fronts,
                                                    const double* __restrict__ arena, double* b, double* xi,
                                                    const double* __restrict__ Dg, int32_t* tflags, int epoch,
                                                    const int32_t* rdone, int nrd, int repoch, int64_t* dbg,
                                                    RootArgs RA) {
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  __shared__ double part[4 * SMALL_SOLVE_MAX], inits[SMALL_SOLVE_MAX];
  int64_t* dg = dbg ? dbg + 8 * blockIdx.x : nullptr;  // MADIPM_TREE_DEBUG: phase stamps
  if (dg && threadIdx.x == 0) dg[0] = wall_clock64();
  const int q = blockIdx.x;
  const bool ra = q < RA.n;  // (the shapes in the launch arguments; beyond kRootArgs, from the tables)
  const int s = ra ? RA.s[q] : fronts[q];
  const int f0 = ra ? RA.f0[q] : T.first[s], w = ra ? RA.w[q] : T.first[s + 1] - f0, r = ra ? RA.r[q] : T.nrows[s];
  const int64_t loff = ra ? RA.loff[q] : T.l_off[s];
  const int tid = threadIdx.x, lane = tid & 63;
  const int ldt = tree_ldt(w);
  // gather: row i = tid >> 2 summed by threads k = tid & 3 over the entries lo + 4 m + k of its segment
  // (the tail past the last full group of 4 by k = 0, in order: k_fwd_tree's summation)
  const int i = tid >> 2, k = tid & 3;
  const int64_t e0 = ra ? RA.e0[q] : T.row_ptr[s];
  int64_t lo = 0, len = 0;
  if (i < r) {
    lo = T.sv_ptr[e0 + i];
    len = T.sv_ptr[e0 + i + 1] - lo;
  }
  const double init = (i < r && k == 0) ? fwd_init(T, s, i, w, f0, b) : 0.0;
  // wave 0's pivots and the caller's positions, and the panel: loaded with everything else, except
  // right after a factorisation whose root tail ran on the side stream (nrd > 0: after the gather,
  // the tail's done flags and the acquire)
  double dpiv[3];
  int pj[3];
  auto factor_loads = [&]() {
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int j = min(lane + 64 * h, max(w - 1, 0));
      dpiv[h] = (tid < 64) ? Dg[f0 + j] : 1.0;
      pj[h] = (tid < 64) ? T.perm[f0 + j] : 0;
    }
    stage_rowmajor<RSN>(arena + loff, Ls, r, w, ldt);
  };
  if (nrd == 0) factor_loads();
  double c = 0.0;
  const int64_t q4 = len >> 2;
  for (int64_t m0 = 0; m0 < q4; m0 += 16) {  // 16 loads in flight (ex10's root rows: ~14 per thread)
    double x[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) x[u] = T.gbuf[lo + 4 * min(m0 + u, max(q4 - 1, (int64_t)0)) + k];
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (m0 + u < q4) c += x[u];
  }
  if (k == 0)
    for (int64_t p = 4 * q4; p < len; ++p) c += T.gbuf[lo + p];
  if (i < r) {
    part[4 * i + k] = c;
    if (k == 0) inits[i] = init;
  }
  if (dg && tid == 0) dg[1] = wall_clock64();
  if (nrd > 0) {  // the root tail on the side stream (LDLSolver::root_async_): every root factorised
    if (tid < 64) {
      int spins = 0;
      for (;;) {
        const bool ok = lane >= nrd ||
                        __hip_atomic_load(rdone + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == repoch;
        if (__all(ok)) break;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 25)) {
          if (lane == 0) atomicOr(T.err, kErrHandoff);
          break;
        }
      }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (dg && tid == 0) dg[2] = wall_clock64();
    factor_loads();
  }
  __syncthreads();  // the panel and the partial sums
  if (dg && tid == 0) {
    if (nrd == 0) dg[2] = dg[1];
    dg[3] = wall_clock64();
  }
  if (tid < 64) {
    double v[3];
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int ii = lane + 64 * h;
      v[h] = (ii < r) ? ((part[4 * ii] + part[4 * ii + 1]) + (part[4 * ii + 2] + part[4 * ii + 3])) + inits[ii] : 0.0;
    }
    fwd_subst_t(v, Ls, ldt, r, w, lane);
    if (dg && tid == 0) dg[4] = wall_clock64();
#pragma unroll
    for (int h = 0; h < 3; ++h) v[h] = (lane + 64 * h < w) ? v[h] / dpiv[h] : 0.0;
    bwd_subst_t(v, Ls, ldt, w, lane);
    if (dg && tid == 0) dg[5] = wall_clock64();
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int j = lane + 64 * h;
      if (j < w) {
        st_sc1(xi + f0 + j, v[h]);
        if (T.wout[s]) b[pj[h]] = v[h];
      }
    }
    publish_sc1(&tflags[s], epoch + 1);  // the backward epoch: k_bwd_tree's children of the root wait on it
    if (dg && tid == 0) dg[6] = wall_clock64();
  }
}

__global__ __launch_bounds__(NT) void k_bwd_tree(FrontTab T, const int32_t* __restrict__ cptr, const int32_t* __restrict__ clist,
                                                 int nt, const int32_t* __restrict__ pdep, int32_t* counter, int32_t* tflags,
                                                 int epoch, const double* __restrict__ arena,
                                                 const double* __restrict__ D, double* xi, double* __restrict__ out,
                                                 int32_t* err, const uint8_t* __restrict__ rootbwd,
                                                 const uint8_t* __restrict__ tchunk) {
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  __shared__ double xbs[SMALL_SOLVE_MAX];
  __shared__ double bpart[3][64];  // waves 1..3: their share of the update rows' products (w <= 64)
  __shared__ int s_task;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_task = atomicAdd(counter, 1);
    if (s_task == nt - 1) atomicExch(counter, 0);  // every ticket taken: ready for the next launch
  }
  __syncthreads();
  const int t = s_task;  // backward ticket t = forward task nt - 1 - t (reverse topological order)
  if (t >= nt) return;
  const int tf = nt - 1 - t;
  if (rootbwd[tf]) return;  // solved and published by k_fwd_tree
  const int q0 = cptr[tf], q1 = cptr[tf + 1];
  const int lane = tid & 63;
  for (int q = q1 - 1; q >= q0; --q) {  // top first
    const int s = clist[q];
    const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
    if (tchunk[s]) {  // chunked front: panel streamed, double-buffered
      bwd_med_front(T, s, arena, D, Ls, xi, out, pdep, t, tflags, epoch, err);
      continue;
    }
    const int ldc = tree_ldc(r);
    stage_colmajor(arena + T.l_off[s], Ls, r, w, ldc);
    const int32_t* __restrict__ rows = T.rows + T.row_ptr[s];
    const int nb = r - w;
    double own[3];  // this front's forward values (previous launch): plain loads, unconditional from
                    // clamped rows (loads under the mask compiled into a wait each), masked after
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int jc = min(lane + 64 * h, max(w - 1, 0));
      own[h] = xi[f0 + jc] / D[f0 + jc];
    }
#pragma unroll
    for (int h = 0; h < 3; ++h) own[h] = (tid < 64 && lane + 64 * h < w) ? own[h] : 0.0;
    static_assert(SMALL_SOLVE_MAX < NT, "k_bwd_tree: one update row per thread");
    const int rk = (tid < nb) ? rows[w + tid] : 0;  // symbolic: loaded before the wait
    int pj[3];  // wave 0: the caller's positions of its pivots
#pragma unroll
    for (int h = 0; h < 3; ++h) pj[h] = (tid < 64 && lane + 64 * h < w) ? T.perm[f0 + lane + 64 * h] : 0;
    const bool wo = T.wout[s];
    if (q == q1 - 1 && tid < 64 && pdep[t] >= 0) poll_deps(pdep, t, t + 1, tflags, epoch, err);
    __syncthreads();  // + the previous (parent) front's drained x stores
    if (tid < nb) xbs[tid] = ld_sc1(xi + rk);
    __syncthreads();
    // the update rows' products L(w + k, j) x_k: for a front of <= 64 pivots and >= 64 update rows the
    // four waves each take a quarter of the rows (ex10's level 1-3 fronts: 70-128 rows, one column per
    // lane) and wave 0 adds the parts in wave order; else wave 0 alone, three columns per lane
    const bool split = w <= 64 && nb >= 64;  // uniform
    double part = 0.0;
    if (split) {
      const int wv = tid >> 6, kb0 = (nb * wv) >> 2, kb1 = (nb * (wv + 1)) >> 2;
      const int cj = min(lane, w - 1);
      double a0 = 0.0, a1 = 0.0;
      int k = kb0;
      for (; k + 1 < kb1; k += 2) {
        a0 = fma(Ls[(w + k) + cj * ldc], xbs[k], a0);
        a1 = fma(Ls[(w + k + 1) + cj * ldc], xbs[k + 1], a1);
      }
      if (k < kb1) a0 = fma(Ls[(w + k) + cj * ldc], xbs[k], a0);
      part = a0 + a1;
      if (wv > 0) bpart[wv - 1][lane] = part;
      __syncthreads();
    }
    if (tid < 64) {
      int cj[3];
#pragma unroll
      for (int h = 0; h < 3; ++h) cj[h] = min(lane + 64 * h, w - 1);
      double acc[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
      if (split) {
        acc[0][0] = ((part + bpart[0][lane]) + bpart[1][lane]) + bpart[2][lane];
      } else {
        for (int k8 = 0; k8 < nb; k8 += 8) {
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) {
            const int k = k8 + kk;
            if (k < nb) {
              const double x = xbs[k];
#pragma unroll
              for (int h = 0; h < 3; ++h) acc[h][kk & 1] = fma(Ls[(w + k) + cj[h] * ldc], x, acc[h][kk & 1]);
            }
          }
        }
      }
      double v[3];
#pragma unroll
      for (int h = 0; h < 3; ++h) v[h] = (lane + 64 * h < w) ? own[h] - (acc[h][0] + acc[h][1]) : 0.0;
      bwd_subst_c(v, Ls, ldc, w, lane);
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const int j = lane + 64 * h;
        if (j < w) {
          st_sc1(xi + f0 + j, v[h]);
          if (wo) out[pj[h]] = v[h];
        }
      }
      publish_sc1(&tflags[s], epoch);  // tasks whose top hangs below s poll it
    }
    __syncthreads();  // wave 0 is done with Ls; its stores are drained
  }
}

// ------------------------------------------------------------------ sharding (SURVEY §8 e)
// External forward contribution of the top fronts: task = (top front, 256-row chunk); xch[xoff + i] =
// (shard 0: own right-hand side entry) + this shard's subtree-root update vectors, child order.
__global__ __launch_bounds__(NT) void k_ext_gather(FrontTab T, const int32_t* __restrict__ list, int shard0,
                                                   const int64_t* __restrict__ sx_ptr, const int64_t* __restrict__ sx_src,
                                                   const double* __restrict__ b, const double* __restrict__ uvec,
                                                   double* __restrict__ xch) {
  int s, chunk;
  task_of(list, s, chunk);
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int i = chunk * NT + threadIdx.x;
  if (i >= r) return;
  const int64_t e = T.xoff[s] + i;
  double v = (shard0 && i < w) ? b[T.perm[f0 + i]] : 0.0;
  for (int64_t p = sx_ptr[e]; p < sx_ptr[e + 1]; ++p) v += uvec[sx_src[p]];
  xch[e] = v;
}

// Sharded solve, solution exchange: slice `me` of g <- this shard's subtree x (caller positions
// gidx), every other slice <- 0 (so that a sum all-reduce can stand in for the all-gather) ...
__global__ __launch_bounds__(NT) void k_gather_pack(const int32_t* gidx, int64_t n, int64_t per, int me,
                                                    const double* b, double* g) {
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
    const int32_t p = gidx[i];
    g[i] = (i / per == me && p >= 0) ? b[p] : 0.0;
  }
}
// ... and after the gather, the other shards' x into the caller's vector
__global__ __launch_bounds__(NT) void k_gather_scatter(const int32_t* gidx, int64_t n, int64_t per, int me,
                                                       const double* g, double* b) {
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
    const int32_t p = gidx[i];
    if (i / per != me && p >= 0) b[p] = g[i];
  }
}

}  // namespace

void ldl_solve_kernel_attributes() {
  set_max_dyn_lds((const void*)k_fwd_small, kSolveSmallLds);
  set_max_dyn_lds((const void*)k_bwd_small, kSolveSmallLds);
  set_max_dyn_lds((const void*)k_fwd_small_m, kSolveSmallMultiLds);
  set_max_dyn_lds((const void*)k_bwd_small_m, kSolveSmallMultiLds);
  set_max_dyn_lds((const void*)k_bwd_big_m, kBwdBigMultiLds);
  set_max_dyn_lds((const void*)k_fwd_tree, TREE_SOLVE_LDS);
  set_max_dyn_lds((const void*)k_bwd_tree, TREE_SOLVE_LDS);
  set_max_dyn_lds((const void*)k_root_solve, TREE_ROOT_LDS);
}

void LDLSolver::lb_fwd(const double* b, hipStream_t s) {
  for (size_t g = 0; g < S_.lb.size(); ++g) {
    const auto& G = S_.lb[g];
    const int nch = (int)cdiv(G.n, LBF_COLS);
    int64_t poff = 0;
    for (size_t h = 0; h < g; ++h) poff += cdiv(S_.lb[h].n, LBF_COLS) * S_.lb[h].m;
    TIMED(KK_LB_GEMV, 8.0 * G.m * (double)G.n, lb_alg(S_, g), 2.0 * G.m * (double)G.n,
          (k_lb_fwd1<<<dim3((unsigned)cdiv(G.m, NT), (unsigned)nch), NT, 0, s>>>(
              lbW_.p + G.w_off, lbd_, lbmem_, perm_, G.m, G.n, G.mem_off, b, xi_, lbpart_.p + poff)));
    k_lb_fwd2<<<(unsigned)cdiv(G.m, NT), NT, 0, s>>>(lbpart_.p + poff, G.m, nch, uvec_.p + G.uvec_off);
  }
}

void LDLSolver::lb_bwd(int g, double* b, hipStream_t s) {
  const auto& G = S_.lb[g];
  int64_t xoff = 0;
  for (int h = 0; h < g; ++h) xoff += S_.lb[h].m;
  TIMED(KK_LB_GEMV, 8.0 * G.m * (double)G.n, lb_alg(S_, g), 2.0 * G.m * (double)G.n,
        (k_lb_bwd<<<(unsigned)cdiv(G.n, NT / 64), NT, 0, s>>>(lbW_.p + G.w_off, lbd_, lbmem_, perm_, lbxrow_.p + xoff,
                                                             G.m, G.n, G.mem_off, xi_, b)));
}

void LDLSolver::fwd_levels(const std::vector<SolveLevel>& V, int phase, double* b, hipStream_t s) {
  const SolveTask* tasks = reinterpret_cast<const SolveTask*>(tasks_.p);
  const int efwd = 2 * epoch_ - 1;
  int32_t* cnt = counters_.p + phase * 2 * S_.nlevels;
  if (phase == 0 && !S_.lb.empty()) lb_fwd(b, s);
  for (int lev = 0; lev < (int)V.size(); ++lev) {
    const SolveLevel& L = V[lev];
    if (L.nmicro)
      TIMED(KK_FWD_TINY, L.micro_bytes, L.micro_alg, L.micro_flops,
            (k_fwd_micro<<<(unsigned)cdiv(L.nmicro, NT / MG), NT, 0, s>>>(T_, sched_.p + L.micro_off, L.nmicro, arena_, b,
                                                                         xi_, uvec_)));
    if (L.ntiny)
      TIMED(KK_FWD_TINY, L.tiny_bytes, L.tiny_alg, L.tiny_flops,
            (k_fwd_tiny<<<(unsigned)cdiv(L.ntiny, 2 * SW), NT, 0, s>>>(T_, sched_.p + L.tiny_off, L.ntiny, arena_, b, xi_,
                                                                      uvec_)));
    if (L.nsmall)
      TIMED(KK_FWD_SMALL, L.small_bytes, L.small_alg, L.small_flops,
            (k_fwd_small<<<(unsigned)L.nsmall, NT, L.small_lds, s>>>(T_, sched_.p + L.small_off, L.nsmall, arena_, b, xi_,
                                                                    uvec_)));
    if (L.nbig) {
      TIMED(KK_FWD_GATHER, L.gat_bytes, 0.0, 0.0,
            (k_fwd_gather<<<L.ngat, NT, 0, s>>>(T_, sched_.p + L.gat_off, b, uvec_, vwork_)));
      TIMED(KK_FWD_BIG, L.big_bytes, L.big_alg + L.below_alg, L.big_flops,
            (k_fwd_big<<<std::min(L.nftask, knobs_.big_solve_wg), NT, 0, s>>>(T_, tasks + L.ftask_off, L.nftask, cnt + 2 * lev,
                                                               flags_, flag_off_, efwd, arena_, vwork_, xi_, uvec_, &st_->err)));
    }
    if (lev == 0 && phase == 0 && ntree_ && nsleaf_)
      TIMED(KK_FWD_TINY, leaf_bytes_, leaf_alg_, leaf_flops_,
            (k_fwd_leaves<<<(unsigned)cdiv(nsleaf_ * LPL, NT), NT, 0, s>>>(tleaf_, (int)nsleaf_, tlrow_, arena_, b, xi_,
                                                                         T_.gbuf)));
    if (lev == 0 && phase == 0 && ntree_)
    {
      const int nlo = ntask_ - nroot_task_;  // the big roots last, in their own launch (more LDS)
      if (nlo > 0)
        TIMED(KK_FWD_TREE, tree_bytes_, tree_alg_, tree_flops_,
              (k_fwd_tree<<<(unsigned)nlo, NT, tree_lds_, s>>>(
                  T_, tc_ptr_, tc_list_, nlo, tdep_ptr_, tdep_, counters_.p + 4 * S_.nlevels, tflags_, efwd, tree_lds_ / 8,
                  arena_, b, xi_, uvec_, &st_->err, tdbg_.p, trootbwd_, D_, tchunk_, tside_.p,
                  rflag_.p ? rflag_.p + 2 : nullptr, root_pending_ && side_tree_ ? nroot_side_ : 0, repoch_)));
      if (side_tree_) root_pending_ = false;  // (root_async_) its side roots waited for the tail
      if (nroot_task_)
        TIMED(KK_FWD_TREE, nlo > 0 ? 0.0 : tree_bytes_, nlo > 0 ? 0.0 : tree_alg_, nlo > 0 ? 0.0 : tree_flops_,
              (k_root_solve<<<(unsigned)nroot_task_, RSN, root_lds_, s>>>(
                  T_, tc_list_.p + nlo, arena_, b, xi_, D_, tflags_, efwd, rflag_.p ? rflag_.p + 2 : nullptr,
                  root_pending_ ? nroot_side_ : 0, repoch_, tdbg_.p ? tdbg_.p + 8 * nlo : nullptr, rargs_)));
      if (nroot_task_ && tdbg_.p) {  // MADIPM_TREE_DEBUG: the root solve's phases
        std::vector<int64_t> h(8 * nroot_task_);
        MADIPM_HIP(hipMemcpyAsync(h.data(), tdbg_.p + 8 * nlo, h.size() * 8, hipMemcpyDeviceToHost, s));
        MADIPM_HIP(hipMemsetAsync(tdbg_.p + 8 * nlo, 0, h.size() * 8, s));  // not tree tasks' stamps
        MADIPM_HIP(hipStreamSynchronize(s));
        for (int q = 0; q < nroot_task_; ++q) {
          const int64_t* d = &h[8 * q];
          fprintf(stderr, "root solve %d: gather %.2f  wait %.2f  panel %.2f  fwd %.2f  bwd %.2f  store %.2f us\n", q,
                  (d[1] - d[0]) * 0.01, (d[2] - d[1]) * 0.01, (d[3] - d[2]) * 0.01, (d[4] - d[3]) * 0.01,
                  (d[5] - d[4]) * 0.01, (d[6] - d[5]) * 0.01);
        }
      }
      root_pending_ = false;  // (root_async_) the first k_root_solve after a factorisation waited for its tail
    }
    if (lev == 0 && phase == 0 && ntree_ && tdbg_.p)
      tree_debug_dump(s, "fwd", tdbg_.p, ntask_, "leaves", "wait", "gather", "subst", "store", 8);
    if (lev == 0) join(s);  // (no-op: root_async_ has no fronts above the tree)
  }
}

void LDLSolver::bwd_levels(const std::vector<SolveLevel>& V, int phase, double* b, hipStream_t s) {
  const SolveTask* tasks = reinterpret_cast<const SolveTask*>(tasks_.p);
  const int ebwd = 2 * epoch_;
  int32_t* cnt = counters_.p + phase * 2 * S_.nlevels;
  for (int lev = (int)V.size() - 1; lev >= 0; --lev) {
    const SolveLevel& L = V[lev];
    if (lev == 0 && phase == 0 && ntree_)
      TIMED(KK_BWD_TREE, tree_bytes_, tree_alg_, tree_flops_,
            (k_bwd_tree<<<(unsigned)ntask_, NT, tree_lds_, s>>>(T_, tc_ptr_, tc_list_, ntask_, tpar_,
                                                                 counters_.p + 4 * S_.nlevels + 1, tflags_, ebwd, arena_, D_,
                                                                 xi_, b, &st_->err, trootbwd_, tchunk_)));
    if (lev == 0 && phase == 0 && ntree_ && nsleaf_)
      TIMED(KK_BWD_TINY, leaf_bytes_, leaf_alg_, leaf_flops_,
            (k_bwd_leaves<<<(unsigned)cdiv(nsleaf_ * LPL, NT), NT, 0, s>>>(tleaf_, (int)nsleaf_, tlrow_, arena_, D_, xi_,
                                                                         b)));
    if (L.nbelow)
      TIMED(KK_BWD_BELOW, L.below_bytes, L.below_alg, 0.25 * L.below_bytes,
            (k_bwd_below<<<L.nbelow, NT, 0, s>>>(T_, sched_.p + L.below_off, bp_off_, arena_, xi_, bpart_)));
    if (L.nbig)
      TIMED(KK_BWD_BIG, L.big_bytes - L.below_bytes, L.big_alg, L.big_flops - 0.25 * L.below_bytes,
            (k_bwd_big<<<std::min(L.nbtask, knobs_.big_solve_wg), NT, 0, s>>>(T_, tasks + L.btask_off, L.nbtask, cnt + 2 * lev + 1,
                                                               flags_, flag_off_, ebwd, arena_, D_, xi_, b, bp_off_, bpart_,
                                                               &st_->err)));
    if (L.nsmall)
      TIMED(KK_BWD_SMALL, L.small_bytes, L.small_alg, L.small_flops,
            (k_bwd_small<<<(unsigned)L.nsmall, NT, L.small_lds, s>>>(T_, sched_.p + L.small_off, L.nsmall, arena_, D_, xi_,
                                                                    b)));
    if (L.ntiny)
      TIMED(KK_BWD_TINY, L.tiny_bytes, L.tiny_alg, L.tiny_flops,
            (k_bwd_tiny<<<(unsigned)cdiv(L.ntiny, 2 * SW), NT, 0, s>>>(T_, sched_.p + L.tiny_off, L.ntiny, arena_, D_, xi_,
                                                                      b)));
    if (L.nmicro)
      TIMED(KK_BWD_TINY, L.micro_bytes, L.micro_alg, L.micro_flops,
            (k_bwd_micro<<<(unsigned)cdiv(L.nmicro, NT / MG), NT, 0, s>>>(T_, sched_.p + L.micro_off, L.nmicro, arena_, D_,
                                                                         xi_, b)));
    if (phase == 0)
      for (int g : lb_at_level_[lev]) lb_bwd(g, b, s);
  }
}

// Phase 1: forward over this shard's subtrees; unsharded it is the whole solve, sharded it ends with
// the top fronts' external forward contribution in solve_xbuf().
void LDLSolver::solve_phase1(double* b, hipStream_t s) {
  if (S_.N == 0) return;
  ++epoch_;
  // the big-front task queues need zeroed counters; the tree kernels reset their own tickets
  bool queues = false;
  for (const SolveLevel& L : slev1_) queues |= L.nbig > 0;
  for (const SolveLevel& L : slev2_) queues |= L.nbig > 0;
  if (queues) MADIPM_HIP(hipMemsetAsync(counters_.p, 0, counters_.n * sizeof(int32_t), s));
  fwd_levels(slev1_, 0, b, s);
  join(s);
  if (!sharded()) {
    bwd_levels(slev1_, 0, b, s);
  } else if (nxg_) {
    k_ext_gather<<<nxg_, NT, 0, s>>>(T_, sched_.p + xg_off_, S_.shard == 0 ? 1 : 0, sx_ptr_, sx_src_, b, uvec_, xch_);
  }
  MADIPM_HIP(hipGetLastError());
}

// Phase 2 (sharded): after the all-reduce of solve_xbuf(): top forward + backward (redundant on every
// shard, which each write the top x to b), then this shard's subtrees backward, and this shard's
// subtree x packed into its slice of solve_gbuf() (other slices zeroed) for the all-gather.
void LDLSolver::solve_phase2(double* b, hipStream_t s) {
  if (S_.N == 0 || !sharded()) return;
  fwd_levels(slev2_, 1, b, s);
  bwd_levels(slev2_, 1, b, s);
  bwd_levels(slev1_, 0, b, s);
  const int64_t n = S_.nshards * gper_;
  k_gather_pack<<<(unsigned)std::min<int64_t>(1024, cdiv(n, NT)), NT, 0, s>>>(gidx_, n, gper_, S_.shard, b, gsol_);
  MADIPM_HIP(hipGetLastError());
}

// Phase 3 (sharded): after the all-gather of solve_gbuf(): the other shards' subtree x into b (every
// entry of b is then this solve's x: top and own entries from phase 2, the rest from the gather).
void LDLSolver::solve_phase3(double* b, hipStream_t s) {
  if (S_.N == 0 || !sharded()) return;
  const int64_t n = S_.nshards * gper_;
  k_gather_scatter<<<(unsigned)std::min<int64_t>(1024, cdiv(n, NT)), NT, 0, s>>>(gidx_, n, gper_, S_.shard, gsol_,
                                                                                  b);
  MADIPM_HIP(hipGetLastError());
}

void LDLSolver::solve_async(double* b, hipStream_t s) {
  solve_phase1(b, s);
  if (!sharded() || S_.N == 0) return;
  MADIPM_REQUIRE(comm_ != nullptr, "sharded LDL^T without a communicator");
  MADIPM_REQUIRE(comm_->size == S_.nshards && comm_->rank == S_.shard, "communicator does not match the shards");
  comm_->allreduce_sum(solve_xbuf(), solve_xlen(), s);
  solve_phase2(b, s);
  comm_->allgather_inplace(solve_gbuf(), gper_, s);
  solve_phase3(b, s);
}

// ------------------------------------------------------------------ multi-right-hand-side solve
// k columns in place, column j at b + j n.  Native route (unsharded, no batched-leaf groups): chunks of kc <= MW
// columns, each forward over mlev_ level by level and backward in reverse, one multi-column launch per non-empty
// class of a level, ordered by the stream: no kernel of it waits on another workgroup of a different launch.  A
// level's big fronts go through the multi-column task-queue kernels (§13k: one zeroing of the level's two
// counters and one pass per direction for the chunk, hand-off words tagged with the chunk's epoch in a buffer
// of their own), or with set_multi_big(false) / MADIPM_MULTI_BIG=0 through the single-column ones, column after
// column inside the level, each pass with its own epoch and zeroed counters: bit for bit the same columns.
// Otherwise: the loop of solve_async.
void LDLSolver::set_multi_big(bool on) { mbig_.multi_big = on ? 1 : 0; }

void LDLSolver::solve_multi_async(double* b, int k, hipStream_t s) {
  if (k <= 0) return;
  ++mstat_.n_calls;
  mstat_.n_columns += k;
  mstat_.n_chunks += cdiv(k, MW);
  if (!mstat_.native) {
    for (int j = 0; j < k; ++j) solve_async(b + (int64_t)j * S_.N, s);
    return;
  }
  join(s);  // the factorisation's root tail may still be on the side stream
  const int64_t N = S_.N, us = std::max<int64_t>(S_.uvec_size, 1);
  if (!xim_.p) {  // the first multi call: MW columns of the internal and the update vector
    xim_.alloc(MW * N);
    uvm_.alloc(MW * us);
  }
  const bool mbig = mbig_.multi_big && mbig_.n_big_levels > 0;
  if (mbig && !xllm_.p) {  // the first multi-column big pass: MW columns of the hand-off words, vwork and bpart
    xllm_.alloc(MW * xll_.n);
    xllm_.zero(s);  // no epoch is 0
    vwm_.alloc(MW * vwork_.n);
    bpm_.alloc(MW * bpart_.n);
    mbig_.big_bytes = (int64_t)(xllm_.n * sizeof(uint64_t) + (vwm_.n + bpm_.n) * sizeof(double));
  }
  const int64_t vs = (int64_t)vwork_.n, bs = (int64_t)bpart_.n;
  const SolveTask* tasks = reinterpret_cast<const SolveTask*>(tasks_.p);
  const int NL = (int)mlev_.size();
  for (int c0 = 0; c0 < k; c0 += MW) {
    const int kc = std::min(MW, k - c0);
    double* bc = b + (int64_t)c0 * N;
    const int e0 = epoch_;  // column j's passes: the epochs of single solve e0 + 1 + j
    epoch_ += kc;
    for (int lev = 0; lev < NL; ++lev) {
      const SolveLevel& L = mlev_[lev];
      if (L.nmicro)
        TIMED(KK_FWD_TINY, L.micro_bytes, L.micro_alg, L.micro_flops,
              (k_fwd_micro_m<<<(unsigned)cdiv(L.nmicro, NT / MG), NT, 0, s>>>(T_, sched_.p + L.micro_off, L.nmicro, kc, arena_,
                                                                             bc, N, xim_, N, uvm_, us)));
      if (L.ntiny)
        TIMED(KK_FWD_TINY, L.tiny_bytes, L.tiny_alg, L.tiny_flops,
              (k_fwd_tiny_m<<<(unsigned)cdiv(L.ntiny, 2 * SW), NT, 0, s>>>(T_, sched_.p + L.tiny_off, L.ntiny, kc, arena_, bc,
                                                                          N, xim_, N, uvm_, us)));
      if (L.nsmall)
        TIMED(KK_FWD_SMALL, L.small_bytes, L.small_alg, L.small_flops,
              (k_fwd_small_m<<<(unsigned)L.nsmall, NT, L.small_lds, s>>>(T_, sched_.p + L.small_off, L.nsmall, kc, arena_, bc,
                                                                        N, xim_, N, uvm_, us)));
      if (L.nbig && mbig) {
        ++mbig_.n_big_passes;
        MADIPM_HIP(hipMemsetAsync(counters_.p + 2 * lev, 0, 2 * sizeof(int32_t), s));
        TIMED(KK_FWD_GATHER, L.gat_bytes, 0.0, 0.0,
              (k_fwd_gather_m<<<L.ngat, NT, 0, s>>>(T_, sched_.p + L.gat_off, kc, bc, N, uvm_, us, vwm_, vs)));
        TIMED(KK_FWD_BIG, L.big_bytes, L.big_alg + L.below_alg, L.big_flops,
              (k_fwd_big_m<<<std::min(L.nftask, knobs_.big_solve_wg), NT, 0, s>>>(
                  T_, tasks + L.ftask_off, L.nftask, kc, counters_.p + 2 * lev, xllm_, flag_off_, 2 * (e0 + 1) - 1, arena_,
                  vwm_, vs, xim_, N, uvm_, us, &st_->err)));
      }
      for (int j = 0; L.nbig && !mbig && j < kc; ++j) {
        ++mbig_.n_big_passes;
        MADIPM_HIP(hipMemsetAsync(counters_.p + 2 * lev, 0, 2 * sizeof(int32_t), s));
        TIMED(KK_FWD_GATHER, L.gat_bytes, 0.0, 0.0,
              (k_fwd_gather<<<L.ngat, NT, 0, s>>>(T_, sched_.p + L.gat_off, bc + j * N, uvm_.p + j * us, vwork_)));
        TIMED(KK_FWD_BIG, L.big_bytes, L.big_alg + L.below_alg, L.big_flops,
              (k_fwd_big<<<std::min(L.nftask, knobs_.big_solve_wg), NT, 0, s>>>(
                  T_, tasks + L.ftask_off, L.nftask, counters_.p + 2 * lev, flags_, flag_off_, 2 * (e0 + 1 + j) - 1, arena_,
                  vwork_, xim_.p + j * N, uvm_.p + j * us, &st_->err)));
      }
    }
    for (int lev = NL - 1; lev >= 0; --lev) {
      const SolveLevel& L = mlev_[lev];
      if (L.nbig && mbig) {
        ++mbig_.n_big_passes;
        MADIPM_HIP(hipMemsetAsync(counters_.p + 2 * lev, 0, 2 * sizeof(int32_t), s));
        if (L.nbelow)
          TIMED(KK_BWD_BELOW, L.below_bytes, L.below_alg, 0.25 * L.below_bytes,
                (k_bwd_below_m<<<L.nbelow, NT, 0, s>>>(T_, sched_.p + L.below_off, kc, bp_off_, arena_, xim_, N, bpm_, bs)));
        TIMED(KK_BWD_BIG, L.big_bytes - L.below_bytes, L.big_alg, L.big_flops - 0.25 * L.below_bytes,
              (k_bwd_big_m<<<std::min(L.nbtask, knobs_.big_solve_wg), NT, kBwdBigMultiLds, s>>>(
                  T_, tasks + L.btask_off, L.nbtask, kc, counters_.p + 2 * lev + 1, xllm_, flag_off_, 2 * (e0 + 1), arena_, D_,
                  xim_, N, bc, N, bp_off_, bpm_, bs, &st_->err)));
      }
      for (int j = 0; L.nbig && !mbig && j < kc; ++j) {
        ++mbig_.n_big_passes;
        MADIPM_HIP(hipMemsetAsync(counters_.p + 2 * lev, 0, 2 * sizeof(int32_t), s));
        if (L.nbelow)
          TIMED(KK_BWD_BELOW, L.below_bytes, L.below_alg, 0.25 * L.below_bytes,
                (k_bwd_below<<<L.nbelow, NT, 0, s>>>(T_, sched_.p + L.below_off, bp_off_, arena_, xim_.p + j * N, bpart_)));
        TIMED(KK_BWD_BIG, L.big_bytes - L.below_bytes, L.big_alg, L.big_flops - 0.25 * L.below_bytes,
              (k_bwd_big<<<std::min(L.nbtask, knobs_.big_solve_wg), NT, 0, s>>>(
                  T_, tasks + L.btask_off, L.nbtask, counters_.p + 2 * lev + 1, flags_, flag_off_, 2 * (e0 + 1 + j), arena_, D_,
                  xim_.p + j * N, bc + j * N, bp_off_, bpart_, &st_->err)));
      }
      if (L.nsmall)
        TIMED(KK_BWD_SMALL, L.small_bytes, L.small_alg, L.small_flops,
              (k_bwd_small_m<<<(unsigned)L.nsmall, NT, L.small_lds, s>>>(T_, sched_.p + L.small_off, L.nsmall, kc, arena_, D_,
                                                                        xim_, N, bc, N)));
      if (L.ntiny)
        TIMED(KK_BWD_TINY, L.tiny_bytes, L.tiny_alg, L.tiny_flops,
              (k_bwd_tiny_m<<<(unsigned)cdiv(L.ntiny, 2 * SW), NT, 0, s>>>(T_, sched_.p + L.tiny_off, L.ntiny, kc, arena_, D_,
                                                                          xim_, N, bc, N)));
      if (L.nmicro)
        TIMED(KK_BWD_TINY, L.micro_bytes, L.micro_alg, L.micro_flops,
              (k_bwd_micro_m<<<(unsigned)cdiv(L.nmicro, NT / MG), NT, 0, s>>>(T_, sched_.p + L.micro_off, L.nmicro, kc, arena_,
                                                                             D_, xim_, N, bc, N)));
    }
  }
  MADIPM_HIP(hipGetLastError());
}

}  // namespace madipm
