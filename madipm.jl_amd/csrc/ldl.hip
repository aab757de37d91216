// Multifrontal supernodal LDL^T for gfx950: the numeric factorisation (assembly, factorisation, status
// and packing kernels with the LDLSolver members that launch them).  The triangular solves are in
// ldl_solve.hip, LDLSolver's construction, timing and ShardGroup in ldl_solver.hip.
//
// Fronts are processed level by level (children before parents).  Per level:
//  * small fronts (r <= 128): ONE workgroup per front, the whole r x r front in LDS:
//    assemble (original entries + extend-add of the children's update blocks, children in a
//    fixed order -> deterministic), right-looking LDL^T of the w pivot columns, write the L panel,
//    D and the (r-w)^2 update block;
//  * big fronts (r > 128): the front lives in HBM (ld r).  Batched launches over all big fronts of
//    the level: column-block assembly, then per 64-column panel a panel kernel (diagonal block
//    factorised in LDS, rows below solved by forward substitution) and a trailing-update kernel
//    C -= (L D) L^T on 64x64 tiles with v_mfma_f64_16x16x4_f64.
// Quasi-definite KKT matrices (FixedRegularization(1e-8,-1e-8)) admit static
// pivoting in any symmetric order; zero / non-finite pivots are reported (is_factorized=false).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstdio>

#include "ldl_front_lds.hpp"

namespace madipm {
namespace {

__global__ void k_status_init(LDLStatus* st, int all = 0) {
  const uint64_t now = wall_clock64();
  if (all) {
    st->ticks = 0;
  } else if (st->t1 > st->t0) {
    st->ticks += st->t1 - st->t0;  // the previous factorisation
  }
  st->t0 = st->t1 = now;
  st->fail_pivot = INT_MAX;
  st->npos = st->nneg = st->nzero = 0;
  if (all) st->err = 0;
}

// ------------------------------------------------------------------ micro fronts (w <= 2, r <= 32)
// The leaf level of the K2 trees (~1e5 fronts: one or two x columns and their rows).  16 lanes per
// front, 16 fronts per workgroup, lane l owns rows l and l + 16; no frontal matrix: a leaf's original
// entries live in its pivot columns only, so L = F(:, 0:w) D^-1 (2 x 2 block at most) and the update
// block is U = -L D L^T (rows >= w), written column by column, coalesced over the group's lanes.
__global__ __launch_bounds__(NT) void k_micro_factor(FrontTab T, const int32_t* __restrict__ fronts, int nf,
                                                     const double* __restrict__ Kx, double* __restrict__ arena,
                                                     double* __restrict__ D, LDLStatus* st, double tol) {
  __shared__ double Fs[NT / MG][64];  // columns 0 / 1 of F (rows 0..31); later l_i0 d0 / l_i1 d1
  const int g = threadIdx.x / MG, l = threadIdx.x & (MG - 1);
  const int q = blockIdx.x * (NT / MG) + g;
  const bool live = q < nf;
  const int s = fronts[live ? q : nf - 1];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  double* F = Fs[g];
#pragma unroll
  for (int k = 0; k < 4; ++k) F[l + 16 * k] = 0.0;
  wave_sync();
  for (int64_t e = T.asm_ptr[s] + l; e < T.asm_ptr[s + 1]; e += MG) {
    // original entries lie in the front's own (w <= 2) columns: d < 2 r, no division
    const int d = (int)T.asm_dst[e];
    const int lc = d >= r ? 1 : 0, lr = d - lc * r;
    F[lr + 32 * lc] = Kx[T.asm_src[e]];
  }
  wave_sync();
  const double d0 = F[0];
  const double f10 = F[1];
  const double l10 = (w == 2) ? f10 / d0 : 0.0;
  const double d1 = (w == 2) ? F[33] - l10 * f10 : 0.0;
  double li0[2], li1[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = l + 16 * h;
    li0[h] = 0.0;
    li1[h] = 0.0;
    if (i >= w && i < r) {
      li0[h] = F[i] / d0;
      if (w == 2) li1[h] = (F[32 + i] - li0[h] * f10) / d1;
    }
  }
  wave_sync();
#pragma unroll
  for (int h = 0; h < 2; ++h) {  // scaled columns for the update: U_ab = -(l_a0 (d0 l_b0) + l_a1 (d1 l_b1))
    const int i = l + 16 * h;
    F[i] = li0[h] * d0;
    F[32 + i] = li1[h] * d1;
  }
  wave_sync();
  if (!live) return;
  double* __restrict__ L = arena + T.l_off[s];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = l + 16 * h;
    if (i < r) {
      L[i] = (i == 0) ? d0 : (i >= w ? li0[h] : l10);
      if (w == 2) L[i + r] = (i == 0) ? 0.0 : (i == 1 ? d1 : li1[h]);
    }
  }
  if (l == 0) {
    D[f0] = d0;
    if (bad_pivot(d0, tol)) atomicMin(&st->fail_pivot, f0 + 1);
    if (w == 2) {
      D[f0 + 1] = d1;
      if (bad_pivot(d1, tol)) atomicMin(&st->fail_pivot, f0 + 2);
    }
  }
  const int u = r - w;
  double* __restrict__ Uo = arena + T.u_off[s];
  for (int b = 0; b < u; ++b) {
    const double sb0 = F[w + b], sb1 = F[32 + w + b];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int a = l + 16 * h - w;  // U row of this lane's row
      if (a >= b && a < u) Uo[a + (int64_t)b * u] = -(li0[h] * sb0 + li1[h] * sb1);
    }
  }
}

// Fronts with r <= 32: one WAVE per front, 4 fronts per workgroup (the leaf level has ~10^5 of them).
// Lane l works on row l & 31 and the columns of parity l >> 5; wave-synchronous right-looking LDL^T.
constexpr int TINY = 32;
__global__ __launch_bounds__(NT) void k_tiny_factor(FrontTab T, const int32_t* __restrict__ fronts, int nf,
                                                    const double* __restrict__ Kx, double* __restrict__ arena,
                                                    const double* __restrict__ fscratch, double* __restrict__ D,
                                                    LDLStatus* st, double tol) {
  constexpr int LD = TINY + 1;
  __shared__ double Fs[4][TINY * LD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wv;
  if (q >= nf) return;
  const int s = fronts[q];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  double* F = Fs[wv];
  const int i = lane & 31, par = lane >> 5;
  for (int j = par; j < r; j += 2) F[i + j * LD] = 0.0;
  wave_sync();
  const int64_t fso = T.fs_off[s];
  if (fso < 0) {
    for (int64_t e = T.asm_ptr[s] + lane; e < T.asm_ptr[s + 1]; e += 64) {
      const int d = (int)T.asm_dst[e], dj = d / r;  // d < r^2: 32-bit division
      F[(d - dj * r) + dj * LD] = Kx[T.asm_src[e]];
    }
  } else {
    const double* __restrict__ Fg = fscratch + fso;
    for (int j = par; j < r; j += 2)
      if (i >= j && i < r) F[i + j * LD] = Fg[i + j * r];
  }
  wave_sync();
  for (int t = 0; t < w; ++t) {
    const double dinv = 1.0 / F[t + t * LD];
    const double lit = F[i + t * LD] * dinv;
    for (int j = t + 1 + par; j < r; j += 2)
      if (i >= j && i < r) F[i + j * LD] -= lit * F[j + t * LD];
    wave_sync();
  }
  double* __restrict__ L = arena + T.l_off[s];
  for (int t = par; t < w; t += 2) {
    const double d = F[t + t * LD];
    if (i < r) L[i + (int64_t)t * r] = (i > t) ? F[i + t * LD] / d : (i == t ? d : 0.0);
    if (i == 0) {
      D[f0 + t] = d;
      if (bad_pivot(d, tol)) atomicMin(&st->fail_pivot, f0 + t + 1);
    }
  }
  const int u = r - w;
  double* __restrict__ Uo = arena + T.u_off[s];
  for (int b = par; b < u; b += 2)
    if (i >= b && i < u) Uo[i + (int64_t)b * u] = F[(w + i) + (w + b) * LD];
}

// ------------------------------------------------------------------ assembly (all big fronts, small fronts with children)
// Phase 1 (flat, thread per chunk): part[c] = sum of the <= kChunk sources of chunk c, in order.
// Chunk sums: thread per chunk of <= kChunk sources, summed in source order.  Sources are int32
// when the arena and K fit (IDX = int32_t), else int64.
template <typename IDX>
__device__ __forceinline__ void asm_chunk_sum(const int64_t* __restrict__ ids, const int64_t* __restrict__ gchunk,
                                              const IDX* __restrict__ gsrc, int64_t c0, int64_t ci,
                                              const double* __restrict__ Kx, const double* __restrict__ arena,
                                              double* __restrict__ part, bool sc1) {
  const int64_t c = ids[c0 + ci];  // the chunks of the launch's chunk-path tiles (asm_chunks_lds)
  const int64_t p0 = gchunk[c], p1 = gchunk[c + 1];
  constexpr int KC = SymbolicPlan::kChunk;
  // every index, then every value operand in flight before the sum: unconditional loads (clamped
  // index, selected source pointer), masked at the sum — predicated loads compiled into branches
  // with a wait each
  int64_t q[KC];
#pragma unroll
  for (int u = 0; u < KC; ++u) q[u] = (int64_t)gsrc[min(p0 + u, max(p1 - 1, p0))];
  double x[KC];
#pragma unroll
  for (int u = 0; u < KC; ++u) x[u] = *((q[u] < 0) ? Kx + ~q[u] : arena + q[u]);
  double v = 0.0;
#pragma unroll
  for (int u = 0; u < KC; ++u)
    if (p0 + u < p1) v += x[u];
  if (sc1)
    __hip_atomic_store(part + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    part[c] = v;
}
template <typename IDX>
__global__ __launch_bounds__(NT) void k_asm_chunks(const int64_t* __restrict__ ids, const int64_t* __restrict__ gchunk,
                                                   const IDX* __restrict__ gsrc, int64_t c0, int64_t n,
                                                   const double* __restrict__ Kx, const double* __restrict__ arena,
                                                   double* __restrict__ part, int32_t* cflag, int epoch) {
  const int64_t ci = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (ci < n) asm_chunk_sum(ids, gchunk, gsrc, c0, ci, Kx, arena, part, cflag != nullptr);
  if (cflag) {  // the root tail (LDLSolver::root_async_): handed to its k_assemble on the side stream
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // form R1: write-through sums drained, one flag
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(cflag + blockIdx.x, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Phase 2: one workgroup (1024 threads) per 64x64 lower tile of F (SymbolicPlan step 10), assembled
// in an LDS tile: entry = sum of its chunk sums in chunk order (asm_chunks_lds), then the big
// children's update blocks record by record in child order (asm_children_lds); thread t writes out
// the entries (row t & 63, columns t >> 6 + 16 k), k < 4.  No atomics, deterministic.  The tile is written to the front (big: arena, ld r; small: scratch, ld r).
constexpr int ANT = 1024;
// tiles of at most kAsmLdsWin windows of kAsmLdsSrc sources (one window in launches of < 256 tiles:
// their few workgroups would carry a root's whole gather — ex10's 3 root tiles of 32k sources took
// 1816 -> 1645 iters/s through the LDS path; the chunk pass spreads it over the chip) gather them into
// LDS and sum them there (asm_chunks_lds), without k_asm_chunks.  (r5_zi: the source count rode in gchk's top 16 bits and was read back with a signed
// shift — a tile of >= 2^15 sources read a negative count and summed nothing; unsigned now)
// The windows straddle: an entry whose sources cross a window boundary carries its running chunk
// sum to the next (the straddle branch below); MADIPM_ASM_LDS_WIN=n (tests) puts every tile of up to
// n windows on this path, whatever its launch size.  kAsmLdsWinMax bounds n: the count rides in 16
// bits of gchk, and the kernel checks it against FrontTab::asm_src_cap (kErrAsmSrc).
static_assert(kAsmLdsSrc == 5 * ANT, "five sources per thread and window");
static_assert(kAsmLdsSrc * kAsmLdsWinMax < 65536, "the tile's source count rides in 16 bits");
// The tile's chunk sums into the LDS tile Ts (64 x 64, column-major, ld 64; zeroed first): the
// tile's nonempty entries (its g_ptr list: ne, then position | first chunk << 12 per entry, then the
// chunk count << 12; ne also in the device tile's gptr >> 48, bit 47: the source path below) spread
// over the threads, up to 4 per thread, each entry's chunk sums added in
// chunk order, CU per entry and round in flight.  A wave past the list issues no load.  Ends with a
// barrier.  (r3-r5 read a dense 4097-offset table per tile: 32 KB of offset loads for a tree front's
// tile of ~40 nonempty entries, neos.)
template <int CU, typename IDX, int WS = 5 * 1024>
__device__ __forceinline__ void asm_chunks_lds(const SymbolicPlan::AsmTile& tl, const int32_t* __restrict__ gent,
                                               const double* __restrict__ part, const IDX* __restrict__ gsrc,
                                               const double* __restrict__ Kx, const double* __restrict__ arena,
                                               double* Ts, double* vals, int32_t* err, int src_cap) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);
#pragma unroll
  for (int m = 0; m < 4; ++m) Ts[(wv + 16 * m) * 64 + lane] = 0.0;
  if (tl.gptr >= 0 && ((tl.gptr >> 47) & 1)) {  // uniform: a tile of <= kAsmLdsWin windows of sources
    // Its entry list holds source offsets (pos | first source << 12): the tile's sources are gathered
    // straight into LDS (thread per source, consecutive indices: coalesced), then each entry sums its
    // sources from LDS in 8-source chunks, in order — k_asm_chunks' partial sums, then their sum, as
    // the chunk path: the same bits, without the chunk launch and its partials in HBM.
    const int32_t* __restrict__ ge = gent + (tl.gptr & (((int64_t)1 << 47) - 1));
    const int ne = (int)(tl.gptr >> 48);
    const int64_t sb = tl.gchk & (((int64_t)1 << 48) - 1);
    int ns = (int)((uint64_t)tl.gchk >> 48);  // unsigned: a count >= 2^15 sets the sign bit
    if (ns > src_cap) {  // uniform: the plan promised at most kAsmLdsWinMax windows — never a silent sum
      if (tid == 0) __hip_atomic_fetch_or(err, kErrAsmSrc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ns = 0;
    }
    int pos[4], s0[4], s1[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      pos[m] = -1;
      s0[m] = s1[m] = 0;
      if (wbase + ANT * m < ne) {  // uniform
        const int k = tid + ANT * m, kk = min(k, ne - 1);
        const int e0 = ge[1 + kk], e1 = ge[2 + kk];
        s0[m] = e0 >> 12;
        s1[m] = k < ne ? e1 >> 12 : s0[m];
        pos[m] = k < ne ? (e0 & 4095) : -1;
      }
    }
    // windows of WS sources; an entry whose sources straddle a window carries its running
    // chunk sum to the next (the chunk boundaries stay every kChunk sources from the entry's first)
    double v[4] = {0.0, 0.0, 0.0, 0.0}, cs[4] = {0.0, 0.0, 0.0, 0.0};
    int nx[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) nx[m] = s0[m];
    for (int w0 = 0; w0 < ns; w0 += WS) {  // uniform
      const int wn = min(WS, ns - w0);
      int64_t q[WS / ANT];
#pragma unroll
      for (int u = 0; u < WS / ANT; ++u)
        q[u] = (wbase + ANT * u < wn) ? (int64_t)gsrc[sb + w0 + min(tid + ANT * u, wn - 1)] : 0;
      double x[WS / ANT];
#pragma unroll
      for (int u = 0; u < WS / ANT; ++u)
        x[u] = (wbase + ANT * u < wn) ? *((q[u] < 0) ? Kx + ~q[u] : arena + q[u]) : 0.0;
#pragma unroll
      for (int u = 0; u < WS / ANT; ++u)
        if (tid + ANT * u < wn) vals[tid + ANT * u] = x[u];
      __syncthreads();  // the window's sources (and the zeroed tile)
      const int we = w0 + wn;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (pos[m] < 0 || nx[m] >= s1[m] || nx[m] >= we) continue;
        if (nx[m] == s0[m] && s1[m] <= we) {  // the whole entry in this window (the common case)
          for (int c = s0[m]; c < s1[m]; c += SymbolicPlan::kChunk) {
            double ck = 0.0;
#pragma unroll
            for (int u = 0; u < SymbolicPlan::kChunk; ++u)
              if (c + u < s1[m]) ck += vals[c + u - w0];
            v[m] += ck;
          }
          nx[m] = s1[m];
        } else {
          const int e = min(s1[m], we);
          for (; nx[m] < e; ++nx[m]) {
            cs[m] += vals[nx[m] - w0];
            if (((nx[m] + 1 - s0[m]) % SymbolicPlan::kChunk) == 0 || nx[m] + 1 == s1[m]) {
              v[m] += cs[m];
              cs[m] = 0.0;
            }
          }
        }
      }
      __syncthreads();  // every entry done with the window before the next overwrites it
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (pos[m] >= 0) Ts[pos[m]] = v[m];
    __syncthreads();
    return;
  }
  __syncthreads();
  if (tl.gptr >= 0) {  // uniform
    const int32_t* __restrict__ ge = gent + (tl.gptr & (((int64_t)1 << 47) - 1));
    const double* __restrict__ pc = part + tl.gchk;
    const int ne = (int)(tl.gptr >> 48);
    int pos[4], c0[4], c1[4], len = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      pos[m] = -1;
      c0[m] = c1[m] = 0;
      if (wbase + ANT * m < ne) {  // uniform
        const int k = tid + ANT * m, kk = min(k, ne - 1);
        const int e0 = ge[1 + kk], e1 = ge[2 + kk];
        c0[m] = e0 >> 12;
        c1[m] = k < ne ? e1 >> 12 : c0[m];
        pos[m] = k < ne ? (e0 & 4095) : -1;
        len = max(len, c1[m] - c0[m]);
      }
    }
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < len; it += CU) {
      double x[4][CU];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int u = 0; u < CU; ++u) x[m][u] = pc[min(c0[m] + it + u, max(c1[m] - 1, c0[m]))];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int u = 0; u < CU; ++u)
          if (c0[m] + it + u < c1[m]) v[m] += x[m][u];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (pos[m] >= 0) Ts[pos[m]] = v[m];
  }
  __syncthreads();
}

// The big children's blocks added into the LDS tile Ts (64 x 64, column-major, ld 64), record by
// record in child order (BigChildRec: a child's hits on the tile are the na x nb block of its U at
// (a0, b0), <= 1024 entries per record): thread e takes the record's entry e — consecutive threads
// read consecutive rows of the child's column, and a wave past the record's entries issues nothing —
// and a barrier separates the records.  The loads of ABR records are in flight before the first
// add.  r3-r5 had every thread pull its own four entries from every child through row / column maps:
// ~5% of those loads hit (neos), and the address unit was the bound (TA busy 83%, r6_b).
template <int ABR>
__device__ __forceinline__ void asm_children_lds(int bt0, int bt1, const BigChildRec* __restrict__ brec,
                                                 const double* __restrict__ arena, double* Ts) {
  const int tid = threadIdx.x;
  const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);
  for (int kc = bt0; kc < bt1; kc += ABR) {  // uniform
    const int nk = min(ABR, bt1 - kc);
    // the batch's record headers first (scalar loads, none waited for alone), then its entry loads
    int4 h0[ABR], h1[ABR];
#pragma unroll
    for (int k = 0; k < ABR; ++k) {
      const int4* __restrict__ hp = reinterpret_cast<const int4*>(brec + kc + min(k, nk - 1));
      h0[k] = hp[0];
      h1[k] = hp[1];
    }
    // the loaded values are only combined at the adds: nothing inside the uniform branch waits
    double x[ABR];
    int rb[ABR], cbt[ABR];
    uint32_t ok = 0;
#pragma unroll
    for (int k = 0; k < ABR; ++k) {
      x[k] = 0.0;
      rb[k] = cbt[k] = 0;
      const int64_t uo = (int64_t)(((uint64_t)(uint32_t)h0[k].y << 32) | (uint32_t)h0[k].x);
      const int ldc = h0[k].z, a0 = h0[k].w, b0 = h1[k].x;
      const int na = h1[k].y & 0xffff, nab = na * ((uint32_t)h1[k].y >> 16);
      if (k < nk && wbase < nab) {  // uniform
        const int e = min(tid, nab - 1);
        const int j = (int)(((uint32_t)e * (uint32_t)h1[k].z) >> 16), i = e - j * na;
        const int ra = a0 + i, cb = b0 + j;
        x[k] = arena[uo + ra + (int64_t)cb * ldc];
        const BigChildRec* __restrict__ R = brec + kc + k;
        rb[k] = R->rows[i];
        cbt[k] = R->cols[j];
        ok |= (uint32_t)(tid < nab && ra >= cb) << k;
      }
    }
#pragma unroll
    for (int k = 0; k < ABR; ++k)
      if (k < nk) {  // uniform
        if ((ok >> k) & 1u) Ts[cbt[k] * 64 + rb[k]] += x[k];
        __syncthreads();
      }
  }
}

// k_assemble runs two tiles per CU (8 waves per SIMD, <= 64 VGPRs: 2 chunk sums per entry and
// round, 8 big-child records per batch; 32 KB of LDS each).  Launches of few tiles (a root's
// high-fan-in assembly: ex10's 3 root tiles, up to 8 chunks per entry) take the CU = 8 instance,
// one round of chunk loads per entry, one tile per CU.
template <int CU, typename IDX>
__global__ __launch_bounds__(ANT, CU == 2 ? 8 : 4) void k_assemble(FrontTab T, const SymbolicPlan::AsmTile* __restrict__ tiles,
                                                     const int32_t* __restrict__ gptr, const double* __restrict__ part,
                                                     const BigChildRec* __restrict__ brec, double* __restrict__ arena,
                                                     double* __restrict__ fscratch, const IDX* __restrict__ gsrc,
                                                     const double* __restrict__ Kx, int32_t* go, int go_epoch,
                                                     const int32_t* cwait, int ncw) {
  constexpr int WS = kAsmLdsSrc;
  __shared__ double Ts[64 * 64];
  extern __shared__ __attribute__((aligned(16))) double vals[];  // WS doubles (dynamic: past 64 KB of static LDS)
  if (ncw > 0) {  // the root tail's assembly on the side stream: the chunk pass's blocks (main stream) first
    if (threadIdx.x < 64) {
      const int lane = threadIdx.x;
      for (int q0 = 0; q0 < ncw; q0 += 64) {
        int spins = 0;
        for (;;) {
          const bool ok = q0 + lane >= ncw ||
                          __hip_atomic_load(cwait + q0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == go_epoch;
          if (__all(ok)) break;
          __builtin_amdgcn_s_sleep(1);
          if (++spins > (1 << 25)) {
            if (lane == 0) atomicOr(T.err, kErrHandoff);
            break;
          }
        }
      }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the chunk sums, the children's blocks, K
  }
  const SymbolicPlan::AsmTile tl = tiles[blockIdx.x];
  const int s = tl.front, ti = tl.tij & 0xffff, tj = (tl.tij >> 16) & 0x7fff;
  const bool acc = tl.tij < 0;  // SymbolicPlan::kAccumulate: F += tile (sharded top fronts, phase 2)
  const int r = T.nrows[s];
  const int I0 = ti * 64, J0 = tj * 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  asm_chunks_lds<CU, IDX, WS>(tl, gptr, part, gsrc, Kx, arena, Ts, vals, T.err, T.asm_src_cap);
  asm_children_lds<8>(tl.bt0, tl.bt1, brec, arena, Ts);
  double v[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) v[m] = Ts[(wv + 16 * m) * 64 + lane];
  const int64_t fso = T.fs_off[s];
  double* __restrict__ F = (fso >= 0 ? fscratch + fso : arena + T.l_off[s]);
  const int i = I0 + lane;
  const int img = (fso >= 0) ? T.fs_img[s] : 0;  // tree front: write its LDS image
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = J0 + wv + 16 * m;
    if (i < r && j < r && i >= j) {
      const int64_t q = !img ? i + (int64_t)j * r : (r > 128 ? (int64_t)((j * (2 * r - j - 1)) >> 1) + i : i + (int64_t)j * (r | 1));
      const double x = acc ? F[q] + v[m] : v[m];
      if (go)
        __hip_atomic_store(F + q, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (st_sc1): to the root tail
      else
        F[q] = x;
    }
  }
  if (go) {  // the root tail's release (LDLSolver::root_async_): the last tile out raises go[0]
    // (form R1: write-through stores drained, one relaxed counter / flag per workgroup)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      const int old = __hip_atomic_fetch_add(go + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == (int)gridDim.x - 1) {
        __hip_atomic_store(go + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(go, go_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// Single-panel big fronts (SymbolicPlan::fused, w <= 64): once k_big_diag / k_big_trsm have written
// the panel's L and D, ONE pass per 64x64 tile assembles the trailing entries (asm_chunks_lds and
// asm_children_lds, as k_assemble) and subtracts L_I D L_J^T (K = w, f64 MFMA 16x16x4) before the tile's only store.  The
// level path moved every trailing entry through HBM three times (k_assemble's store, k_big_upd128's
// load and store); neos' 1220 skinny big fronts (w <= 39, r up to 2.7k) are mostly trailing matrix.
// Each of the 16 waves owns one 16x16 block, and each thread assembles exactly the four entries its
// MFMA result holds (no result tile in LDS); the operands are staged [k][row] for the K = kmax rows
// the launch needs (dynamic LDS: 2 x kmax x 80 doubles, 51 KB at neos' w <= 39, beside the 32 KB
// assembled tile).  Column block 0's tiles (assembled for the panel by k_assemble) get their columns >= w here.
// Operands and MFMA order are k_big_upd128's (A = L_J, B = (L D)_I, K ascending, one accumulator):
// the same U bit for bit.
constexpr int AU_LDT = 80;  // [k][row] operand stride (conflict-free ds_read_b64 for the 16x4 pattern)
template <typename IDX>
__global__ __launch_bounds__(ANT) void k_asm_update(FrontTab T, const SymbolicPlan::AsmTile* __restrict__ tiles,
                                                    const int32_t* __restrict__ gptr, const double* __restrict__ part,
                                                    const BigChildRec* __restrict__ brec, double* __restrict__ arena,
                                                    const double* __restrict__ D, int kmax, const IDX* __restrict__ gsrc,
                                                    const double* __restrict__ Kx) {
  extern __shared__ __attribute__((aligned(16))) double AUs[];
  __shared__ double Ts[64 * 64];     // the assembled tile
  double* Wt = AUs;                  // (L D)[I rows], kmax x AU_LDT
  double* Lt = AUs + kmax * AU_LDT;  // L[J rows]
  double* vals = AUs + 2 * kmax * AU_LDT;  // the tile's sources (asm_chunks_lds), kAsmLdsSrc doubles
  const SymbolicPlan::AsmTile tl = tiles[blockIdx.x];
  const int s = tl.front, ti = tl.tij & 0xffff, tj = (tl.tij >> 16) & 0x7fff;
  const int r = T.nrows[s], f0 = T.first[s], w = T.first[s + 1] - f0;
  const int I0 = ti * 64, J0 = tj * 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bi = wv & 3, bj = wv >> 2;
  double* __restrict__ F = arena + T.l_off[s];
  // the panel rows of I and J, [k][row]: thread (row lane, k = wv + 16 q); clamped loads, masked stores
  {
    double a[4], b[4], d[4];
    const int ri = min(I0 + lane, r - 1), rj = min(J0 + lane, r - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kc = min(wv + 16 * q, w - 1);
      a[q] = F[ri + (int64_t)kc * r];
      b[q] = F[rj + (int64_t)kc * r];
      d[q] = D[f0 + kc];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = wv + 16 * q;
      if (k < kmax) {
        Wt[k * AU_LDT + lane] = (k < w && I0 + lane < r) ? a[q] * d[q] : 0.0;
        Lt[k * AU_LDT + lane] = (k < w && J0 + lane < r) ? b[q] : 0.0;
      }
    }
  }
  // this thread's entries = its MFMA result's: row 16 bi + (lane & 15), column 16 bj + (lane >> 4) + 4 g
  int ei[4], ej[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    ei[g] = 16 * bi + (lane & 15);
    ej[g] = 16 * bj + (lane >> 4) + 4 * g;
  }
  asm_chunks_lds<4, IDX, kAsmLdsSrc>(tl, gptr, part, gsrc, Kx, arena, Ts, vals, T.err, T.asm_src_cap);
  asm_children_lds<8>(tl.bt0, tl.bt1, brec, arena, Ts);
  double v[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) v[g] = Ts[ej[g] * 64 + ei[g]];
  __syncthreads();  // the operands in LDS
  dbl4 acc = {0.0, 0.0, 0.0, 0.0};
  const int nks = (w + 3) >> 2;
  for (int ks = 0; ks < nks; ++ks) {  // wave-uniform
    const int kk = 4 * ks + (lane >> 4);
    const double a = Lt[kk * AU_LDT + 16 * bj + (lane & 15)];
    const double b = Wt[kk * AU_LDT + 16 * bi + (lane & 15)];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int i = I0 + ei[g], j = J0 + ej[g];
    if (i < r && j < r && i >= j && j >= w) F[i + (int64_t)j * r] = v[g] - acc[g];
  }
}

// ------------------------------------------------------------------ big fronts (HBM)

// ---- blocked 64x64 panel kernels (16x16 sub-blocks; wave w owns sub-block row w)
// Layout conventions: A64 = LDS 64x64 tile, col-major, ld 65.  MFMA f64 16x16x4 fragments:
// A operand lane l = (m = l & 15, k = l >> 4); B operand lane l = (k = l >> 4, n = l & 15);
// result D lane l, element g = (m = (l >> 4) + 4 g, n = l & 15).
constexpr int LDA = 65;

// Blocked LDL^T of the LDS tile A64 (lower part valid) by 4 waves: after the call A64 holds the
// strictly-lower L (diagonal untouched), Dl the pivots and Ms[K] the four M_K blocks.
// (the pipelined schedule of blocked_factor_pipe on this tile was measured slower — supportcase10
// k_big_diag 18.1 -> 19.8 us, r3: four pivot blocks leave the other waves too little to overlap)
__device__ __forceinline__ void diag64(double* A64, double* Dl, double* Ms, int tid) {
  const int lane = tid & 63, w = tid >> 6;
  for (int K = 0; K < 4; ++K) {
    if (w == K) factor16r<false, true>(A64, 64, LDA, 16 * K, 16, Dl, Ms + K * 16 * LDM, lane);
    __syncthreads();
    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
    if (w > K) {  // L_wK = A_wK M_K
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int k = 4 * ks + (lane >> 4);
        const double av = A64[(16 * w + (lane & 15)) + (16 * K + k) * LDA];
        const double bv = Ms[K * 16 * LDM + k * LDM + (lane & 15)];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
    }
    __syncthreads();  // every wave has read A_wK before it is overwritten
    if (w > K) {
#pragma unroll
      for (int g = 0; g < 4; ++g) A64[(16 * w + (lane >> 4) + 4 * g) + (16 * K + (lane & 15)) * LDA] = acc[g];
    }
    __syncthreads();
    if (w > K) {  // A_wJ -= (L_wK D_K) L_JK^T, K < J <= w
      for (int J = K + 1; J <= w; ++J) {
        dbl4 u = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int k = 4 * ks + (lane >> 4);
          const double av = A64[(16 * w + (lane & 15)) + (16 * K + k) * LDA] * Dl[16 * K + k];
          const double bv = A64[(16 * J + (lane & 15)) + (16 * K + k) * LDA];
          u = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, u, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) A64[(16 * w + (lane >> 4) + 4 * g) + (16 * J + (lane & 15)) * LDA] -= u[g];
      }
    }
    // next K: wave K+1 factors the block it just updated itself; the others read M_{K+1} after
    // the barrier at the top of the next iteration
  }
  __syncthreads();
}

// the consumer's end of the hand-off (ldl_device.hpp) for ONE flag: poll relaxed, then load sc1
__device__ __forceinline__ bool poll_flag(int32_t* f, int epoch, int32_t* err) {
  int spins = 0;
  while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > (1 << 25)) {
      atomicOr(err, kErrHandoff);
      return false;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler ordering only (sc1 loads follow)
  return true;
}

// ------------------------------------------------------------------ small fronts in LDS (r <= 192)
// One workgroup per front, factorised by ldl_front_lds.hpp's blocked LDL^T.
// k_small_blocked: 8 waves (2 per SIMD): twice the loads in flight of the staging copy and write-out,
// and 7 waves beside the pivot chain of the pipelined factorisation (the 120-column ex10 root)
constexpr int SBT = 512;
template <bool PK>
__global__ __launch_bounds__(SBT) void k_small_blocked(FrontTab T, const int32_t* __restrict__ fronts,
                                                      const double* __restrict__ Kx, double* __restrict__ arena,
                                                      const double* __restrict__ fscratch, double* __restrict__ D,
                                                      LDLStatus* st, double tol, LDLStatus* stamp, int32_t* go,
                                                      int go_epoch) {
  extern __shared__ __attribute__((aligned(16))) double A[];  // lower part of F (square ld r|1, or packed)
  __shared__ double Dl[192];
  __shared__ double MK[16 * LDM];
  __shared__ __attribute__((aligned(16))) double cbuf[2 * 16 * LDM];
  const int s = fronts[blockIdx.x];
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int ld = r | 1;
  const int tid = threadIdx.x;
  // the root tail (LDLSolver::root_async_): launched on the side stream ahead of time, it waits for
  // the root assembly's go[0] (k_assemble's last tile, main stream), then acquires its stores.  The
  // pivot chain runs beside the solve's kernels on this CU: its waves issue first
  if (go) {
    __builtin_amdgcn_s_setprio(3);
    if (tid < 64) poll_flag(go, go_epoch, T.err);
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  const int64_t fso = T.fs_off[s];
  if (fso >= 0 && !T.fs_img[s]) {  // batched-leaf parent: the SYRK and k_assemble wrote ld r
    stage_front<PK, SBT>(fscratch + fso, A, r, ld);
  } else if (fso >= 0) {  // assembled by k_assemble as the LDS image (lower part valid): a straight copy
    const double* __restrict__ src = fscratch + fso;
    const int n = PK ? r * (r + 1) / 2 : r * ld;
    for (int base = 0; base < n; base += SBT * 16) {
      double v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int q = base + k * SBT + tid;
        v[k] = (q < n) ? src[q] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int q = base + k * SBT + tid;
        if (q < n) A[q] = v[k];
      }
    }
  } else {  // leaf: original entries only
    const int ntot = PK ? r * (r + 1) / 2 : r * ld;
    for (int q = tid; q < ntot; q += SBT) A[q] = 0.0;
    __syncthreads();
    for (int64_t q = T.asm_ptr[s] + tid; q < T.asm_ptr[s + 1]; q += SBT) {
      const int d = (int)T.asm_dst[q], dj = d / r;  // d < r^2: 32-bit division
      A[fidx<PK>(d - dj * r, dj, r, ld)] = Kx[T.asm_src[q]];
    }
  }
  __syncthreads();
  factor_lds<PK>(T, A, r, w, ld, Dl, MK, cbuf);
  blocked_writeout<PK, false>(A, r, w, ld, Dl, arena + T.l_off[s], arena + T.u_off[s], T.u_ld[s], D, f0, st, tol);
  if (go) {  // released to k_root_solve (go[2 + front]: the epoch); nothing of this kernel follows
    __threadfence();
    __syncthreads();
  }
  if (tid == 0) {
    // lazy inertia: the factorisation's end
    if (stamp) atomicMax(reinterpret_cast<unsigned long long*>(&stamp->t1), (unsigned long long)wall_clock64());
    if (go) __hip_atomic_store(go + 2 + blockIdx.x, go_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ------------------------------------------------------------------ leaf folding
// A tree front folds its micro-leaf children (w <= 2, r <= 32; SymbolicPlan::absorb) into its LDS
// front instead of k_micro_factor writing their update blocks to HBM and the gather pre-assembly
// summing them.  Per batch of leaves: (1) thread per leaf row gathers the row's entries of the leaf's
// two columns from the caller's K values; (2) thread per leaf row: the leaf's pivots d0, l10, d1 (from
// its first two rows) and the row's l (and l d) in LDS; (3) the product list: thread t walks its chunk of destination-sorted products
// F(i, j) -= l0(q1) l0(q2) d0 + l1(q1) l1(q2) d1, one partial sum per destination run, so every
// entry of F has one writer and a fixed order (leaf order) — no atomics, balanced by product count
// whatever the row density.
// Latency: every phase is one or two global round trips at most (8 leaf rows per thread in flight;
// product entries 16 per thread in flight, the next group's loads issued before the current group's
// arithmetic, the first group before phase 1).
// k_fact_tree's workgroup: 8 waves (2 per SIMD) — every memory phase of a tree front (the leaf fold,
// the staging copy, the children's pushes, the write-out) is latency-bound, and a second wave per SIMD
// doubles the loads in flight; the in-LDS factorisation deals its tiles over the 8 waves
constexpr int FTN = SymbolicPlan::kFoldThreads;
static_assert(FTN == 512, "k_fact_tree: 512 threads");

// one copy for both storage variants (a static __shared__ inside the template would be allocated twice)
struct FoldBatchTab {
  int64_t j[SymbolicPlan::kFoldMaxBatches + 1], po[SymbolicPlan::kFoldMaxBatches];
  int32_t k[SymbolicPlan::kFoldMaxBatches + 1], pl[SymbolicPlan::kFoldMaxBatches];
};
__device__ __forceinline__ FoldBatchTab& fold_batch_tab() {
  __shared__ FoldBatchTab t;
  return t;
}

#ifndef MADIPM_FOLD_GP
#define MADIPM_FOLD_GP 16  // fold product entries per thread and group (32 spills; variants: tools/build_variant.sh)
#endif
// cval / cdst: per thread, the parked sum and destination of a chunk's first run when it continues
// the left neighbour's run (k_fact_tree's MK / cbuf, idle during the fold)
template <bool PK>
__device__ __forceinline__ void fold_leaves(const FrontTab& T, int s, int r, int ld, double* A, const double* Kx, double* arena,
                                            double* D, LDLStatus* st, double tol, double* ext, double* cval,
                                            int32_t* cdst, int64_t* fdg, const FoldStart& F0, bool with_asm) {
  int64_t tph[4] = {0, 0, 0, 0}, tc = fdg ? wall_clock64() : 0;
  auto lap = [&](int k) {
    if (fdg) {
      const int64_t t2 = wall_clock64();
      tph[k] += t2 - tc;
      tc = t2;
    }
  };
  constexpr int RPT = 8;   // leaf rows per thread and pass
  constexpr int GP = MADIPM_FOLD_GP;  // product entries per thread and group
  const int RM = T.fold_rmax[s], LM = T.fold_lmax[s];
  double2* LQ = reinterpret_cast<double2*>(ext);  // per batch row: K values of columns 0/1, then (l0, l1)
  double2* PQ = LQ + RM;                          // (l0 d0, l1 d1)
  int32_t* pf0 = reinterpret_cast<int32_t*>(PQ + RM);     // per leaf: first pivot (in 3 LM doubles of carve)
  int64_t* ploff = reinterpret_cast<int64_t*>(reinterpret_cast<double*>(pf0) + 3 * LM);
  int32_t* prow0 = reinterpret_cast<int32_t*>(ploff + LM);  // batch-local first row of the leaf
  int32_t* pwrc = prow0 + LM;
  int32_t* kk = pwrc + LM;                                   // per batch row: batch-local leaf
  const int tid = threadIdx.x;
  const int b0 = F0.b0, nb = F0.b1 - F0.b0;  // the front's batches (a helper: its share)
  if (nb > SymbolicPlan::kFoldMaxBatches) {  // the batch table below has room for kFoldMaxBatches
    if (tid == 0) __hip_atomic_fetch_or(T.err, kErrLdsCarve, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  // the batch table (first leaf, first row, product offset and length), loaded once into LDS: read
  // from global per batch it cost two dependent round trips at each batch's gather and products
  FoldBatchTab& ft = fold_batch_tab();
  int32_t *tb_k = ft.k, *tb_pl = ft.pl;
  int64_t *tb_j = ft.j, *tb_po = ft.po;
  int32_t rk = 0, rpl = 0;
  int64_t rj = 0, rpo = 0;
  if (tid <= nb) {
    const int bq = b0 + tid, bc = min(bq, b0 + nb - 1);  // the sentinel entry (tid == nb) is the next batch's start
    rk = T.fold_bat[bq];
    rpl = T.fold_plen[bc];
    rj = T.fold_row0[bq];
    rpo = T.fold_poff[bc];
  }
  // product entries (SymbolicPlan::fold_prod): thread t walks chunk t, GP entries per group
  constexpr uint32_t PAD = SymbolicPlan::kFoldPad;
  uint32_t e[GP];
  auto load_group = [&](uint32_t (&g)[GP], const uint32_t* P, int k, int len) {
#pragma unroll
    for (int u = 0; u < GP; ++u) {
      const int kk = k + u;  // uniform: a scalar branch, not a per-lane wait
      g[u] = (kk < len) ? P[(int64_t)kk * FTN] : PAD;
    }
  };
  // the leaf rows' K entries of batch b + 1 are loaded into registers during batch b (indices before
  // its pivots, values before its products) and stored after its products: only batch 0's gather is
  // exposed (r3: every batch's gather, two dependent round trips, lay on the front's critical path).
  // A batch of more than RPT x FTN rows gathers its remaining passes in place.
  int32_t sa[RPT], sb[RPT];
  double va[RPT], vb[RPT];
  auto gather_idx = [&](int64_t j0, int nrow, int q0) {
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      const int q = q0 + u * FTN + tid;
      sa[u] = (q < nrow) ? T.ab_src0[j0 + q] : -1;
      sb[u] = (q < nrow) ? T.ab_src1[j0 + q] : -1;
    }
  };
  auto gather_val = [&]() {
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      va[u] = (sa[u] >= 0) ? Kx[sa[u]] : 0.0;
      vb[u] = (sb[u] >= 0) ? Kx[sb[u]] : 0.0;
    }
  };
  auto gather_store = [&](int nrow, int q0) {
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      const int q = q0 + u * FTN + tid;
      if (q < nrow) LQ[q] = double2{va[u], vb[u]};
    }
  };
  // the leaf tables (first row, w | rc, L offset, first pivot) of batch b + 1 are loaded during batch
  // b's L and product phases (after batch b's pivots consumed them): no exposed round trip in the
  // gather and pivot phases (r5: two per batch, ~3 us of the level-2 fronts' ~13 us per batch)
  int64_t laf[2], llo[2];
  int32_t lwr[2], lf0[2];
  auto leaf_tab = [&](int kb, int nl) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = tid + h * FTN;
      const bool ok = k < nl;
      laf[h] = ok ? T.ab_first[kb + k] : 0;
      lwr[h] = ok ? T.ab_wrc[kb + k] : 0;
      llo[h] = ok ? T.ab_loff[kb + k] : 0;
      lf0[h] = ok ? T.ab_f0[kb + k] : 0;
    }
  };
  // batch 0's leaf tables, first gather pass and first product group (its table entries as uniform
  // loads) and this front's original K entries, all in one round trip; their K values (the leaf rows'
  // and the front's own) in a second — the zero fill of the front beside them
  if (nb > 0) {
    leaf_tab(F0.kq0, F0.kq1 - F0.kq0);
    gather_idx(F0.row0, (int)(F0.row1 - F0.row0), 0);
    load_group(e, T.fold_prod + F0.poff + tid, 0, F0.plen);
  } else {
    gather_idx(0, 0, 0);  // no leaves: no loads
  }
  const int64_t qa = with_asm ? T.asm_ptr[s] + tid : 0, qe = with_asm ? T.asm_ptr[s + 1] : 0;
  const bool a0 = qa < qe;
  const int ad = a0 ? (int)T.asm_dst[qa] : 0;
  const int64_t as = a0 ? T.asm_src[qa] : 0;
  const int ntot = PK ? r * (r + 1) / 2 : r * ld;
  for (int q = tid; q < ntot; q += FTN) A[q] = 0.0;
  const double av = a0 ? Kx[as] : 0.0;
  gather_val();
  if (tid <= nb) {
    tb_k[tid] = rk;
    tb_j[tid] = rj;
    if (tid < nb) tb_po[tid] = rpo, tb_pl[tid] = rpl;
  }
  __syncthreads();  // the zero fill
  if (a0) {
    const int dj = ad / r;  // d < r^2: 32-bit division
    A[fidx<PK>(ad - dj * r, dj, r, ld)] = av;
  }
  for (int64_t q = qa + FTN; q < qe; q += FTN) {
    const int d = (int)T.asm_dst[q], dj = d / r;
    A[fidx<PK>(d - dj * r, dj, r, ld)] = Kx[T.asm_src[q]];
  }
  __syncthreads();  // the batch table and the original entries
  for (int b = 0; b < nb; ++b) {
    const int k0 = tb_k[b], k1 = tb_k[b + 1];
    const int64_t j0 = tb_j[b];
    const int nrow = (int)(tb_j[b + 1] - j0), nleaf = k1 - k0;
    if (nrow > RM || nleaf > LM || nleaf > 2 * FTN) {  // a batch beyond the carve the front was sized by
      if (tid == 0) __hip_atomic_fetch_or(T.err, kErrLdsCarve, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;  // (uniform: the batch table is in LDS)
    }
    // (1) the leaf rows' K entries (the first pass and the leaf tables in registers already)
    gather_store(nrow, 0);
    for (int q0 = RPT * FTN; q0 < nrow; q0 += RPT * FTN) {
      gather_idx(j0, nrow, q0);
      gather_val();
      gather_store(nrow, q0);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = tid + h * FTN;
      if (k < nleaf) {
        const int q0 = (int)(laf[h] - j0), wrc = lwr[h];
        prow0[k] = q0;
        pwrc[k] = wrc;
        ploff[k] = llo[h];
        pf0[k] = lf0[h];
        for (int i = 0; i < (wrc >> 8); ++i) kk[q0 + i] = k;
      }
    }
    __syncthreads();
    lap(0);
    const bool pre = b + 1 < nb;  // prefetch the next batch's first pass and leaf tables
    if (pre) {
      gather_idx(tb_j[b + 1], (int)(tb_j[b + 2] - tb_j[b + 1]), 0);
      leaf_tab(tb_k[b + 1], tb_k[b + 2] - tb_k[b + 1]);
    }
    lap(1);
    // (2) per leaf row: the leaf's pivots from its first two rows (rows i < w, never rewritten here;
    // every row's thread forms them itself: no per-leaf phase and barrier), then its L entries (HBM
    // panel for the solves: d on the diagonal, zero above; LDS: l and l d of the update rows); the
    // first row's thread stores D and checks the pivots
    for (int q = tid; q < nrow; q += FTN) {
      const int k = kk[q];
      const int wrc = pwrc[k], w = wrc & 255, rc = wrc >> 8, jf = prow0[k], i = q - jf;
      const double2 r0 = LQ[jf], r1 = (w == 2) ? LQ[jf + 1] : double2{0.0, 0.0};
      const double d0 = r0.x, f10 = r1.x;
      const double l10 = (w == 2) ? f10 / d0 : 0.0;
      const double d1 = (w == 2) ? r1.y - l10 * f10 : 0.0;
      double* __restrict__ L = arena + ploff[k];
      if (i >= w) {
        const double2 a = LQ[q];
        const double li0 = a.x / d0;
        const double li1 = (w == 2) ? (a.y - li0 * f10) / d1 : 0.0;
        LQ[q] = double2{li0, li1};
        PQ[q] = double2{li0 * d0, li1 * d1};
        L[i] = li0;
        if (w == 2) L[i + rc] = li1;
      } else if (i == 0) {
        L[0] = d0;
        if (w == 2) L[rc] = 0.0;
        const int f0 = pf0[k];
        D[f0] = d0;
        if (bad_pivot(d0, tol)) atomicMin(&st->fail_pivot, f0 + 1);
        if (w == 2) {
          D[f0 + 1] = d1;
          if (bad_pivot(d1, tol)) atomicMin(&st->fail_pivot, f0 + 2);
        }
      } else {  // i == 1, w == 2
        L[1] = l10;
        L[1 + rc] = d1;
      }
    }
    __syncthreads();
    lap(2);
    if (pre) gather_val();
    // (3) this thread's chunk of the destination-sorted products (entry k at FTN k + tid: each load
    // instruction is coalesced)
    const uint32_t* __restrict__ P = T.fold_prod + tb_po[b] + tid;
    const int len = tb_pl[b];
    const uint32_t head = T.fold_chead[(int64_t)(b0 + b) * FTN + tid];
    int d = (int)(head & 0xffffu);              // the running destination
    bool park = (head & SymbolicPlan::kFoldCont) != 0;  // the first run continues the left chunk's
    cdst[tid] = -1;
    double acc = 0.0;  // the negated sum of the open run
    for (int k = 0; k < len; k += GP) {
      uint32_t nx[GP];
      if (k + GP < len) {
        load_group(nx, P, k + GP, len);
      } else if (b + 1 < nb) {  // the next batch's first group
        load_group(nx, T.fold_prod + tb_po[b + 1] + tid, 0, tb_pl[b + 1]);
      }
      // every LDS operand of the group is read before its first update of A (a kFoldPad entry reads
      // row 0 and adds nothing)
      double v[GP];
#pragma unroll
      for (int u = 0; u < GP; ++u) {
        const uint32_t q1 = e[u] & 0xfffu, q2 = (e[u] >> 12) & 0xfffu;
        const bool pad = q1 == PAD;
        const double2 la = LQ[pad ? 0u : q1], pb = PQ[q2];
        v[u] = pad ? 0.0 : fma(la.x, pb.x, la.y * pb.y);
      }
      // a run's sum is subtracted at its last entry with a non-returning LDS atomic — one writer per
      // address (a run split by a chunk cut parks its continuation parts instead), so the result is
      // deterministic, and no wait for the old value.  Selects and one predicated atomic per entry;
      // padding never ends a run, and acc restarts every batch.
#pragma unroll
      for (int u = 0; u < GP; ++u) {
        d += (int)((e[u] >> 24) & 127u);
        const bool end = (int32_t)e[u] < 0;
        const double sum = acc - v[u];
        if (end && park) {
          cval[tid] = sum;
          cdst[tid] = d;
        } else if (end) {
          __hip_atomic_fetch_add(A + d, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        park = park && !end;
        acc = end ? 0.0 : sum;
      }
      if (k + GP < len || b + 1 < nb) {
#pragma unroll
        for (int u = 0; u < GP; ++u) e[u] = nx[u];
      }
    }
    if (len == 0 && b + 1 < nb) load_group(e, T.fold_prod + tb_po[b + 1] + tid, 0, tb_pl[b + 1]);
    __syncthreads();
    // the parked parts, left to right: the first chunk of each continued run adds the run's parts
    if (cdst[tid] >= 0 && (tid == 0 || cdst[tid - 1] != cdst[tid])) {
      const int dd = cdst[tid];
      double t = 0.0;
      for (int u = tid; u < FTN && cdst[u] == dd; ++u) t += cval[u];
      A[dd] += t;
    }
    __syncthreads();
    lap(3);
  }
  if (fdg && threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) fdg[k] = tph[k];
}

// ------------------------------------------------------------------ factorisation tree
// ONE launch factorises every tree front (SymbolicPlan::ftree: phase-1 fronts of <= 192 rows whose
// children are pre-leaves or tree fronts).  Workgroups take fronts in topological order from an
// atomic ticket (no deadlock at any grid size); a front stages its pre-assembled scratch (original
// entries + pre-leaf children, one gather pass before this launch) into LDS, then waits for its tree
// children's flags and adds their update blocks child by child (sc1 loads; the children stored them
// write-through), factorises in LDS and publishes (every wave drains, barrier, one flag store).  The
// last workgroup to finish resets the ticket counters for the next launch.
// Child update block -> parent front in LDS: child columns dealt to waves (NC per wave and round,
// NH 64-row chunks), all of a round's loads (sc1: handed over inside the launch) issued before the
// read-modify-writes; the parent column base is wave-uniform, so a row costs one rels lookup.
// Destinations are distinct within a child, so all LDS reads of a round precede its writes.
#ifndef PUSH_NC2
#define PUSH_NC2 8
#endif
#ifndef PUSH_NC3
#define PUSH_NC3 6
#endif
template <bool PK, int NH, int NC>
__device__ __forceinline__ void push_cols(double* A, int r, int ld, const double* U, int64_t uld, int uc,
                                          const int32_t* rels) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  for (int b0 = NC * wv; b0 < uc; b0 += nw * NC) {
    // every global load of the round first, from clamped addresses (no branches between them)
    double x[NC][NH];
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      const int bc = min(b0 + cb, uc - 1);
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const int ac = min(b0 + cb + lane + 64 * h, uc - 1);
        x[cb][h] = __hip_atomic_load(U + ac + ucol_off(bc, uc, uld), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // then the destinations (relative indices in LDS) and the read-modify-writes
    int dst[NC][NH];
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      const int b = b0 + cb, j = rels[min(b, uc - 1)];
      const int base = PK ? ((j * (2 * r - j - 1)) >> 1) : j * ld;  // fidx(i, j) = base + i
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const int a = b + lane + 64 * h;
        dst[cb][h] = (b < uc && a < uc) ? base + rels[min(a, uc - 1)] : -1;
      }
    }
#pragma unroll
    for (int cb = 0; cb < NC; ++cb)
#pragma unroll
      for (int h = 0; h < NH; ++h) x[cb][h] += A[max(dst[cb][h], 0)];
#pragma unroll
    for (int cb = 0; cb < NC; ++cb)
#pragma unroll
      for (int h = 0; h < NH; ++h)
        if (dst[cb][h] >= 0) A[dst[cb][h]] = x[cb][h];
  }
}

template <bool PK>
__device__ __forceinline__ void fact_tree_front(const FrontTab& T, int s, const int32_t* __restrict__ dep, int q0, int q1,
                                                int32_t* flags, int epoch, const double* Kx, double* arena,
                                                const double* fscratch,
                                                double* D, LDLStatus* st, double tol, int32_t* err, double* A,
                                                double* Dl, double* MK, double* cbuf, int32_t* rels, int64_t* dg) {
  const int tid = threadIdx.x;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int ld = PK ? 0 : (r | 1);
  const FoldStart F0 = T.fstart[s];  // (with the front's other words: no dependent round trip later)
  // the fold helper (if any) and its flag / image, loaded now — after the fold they were two dependent
  // round trips in front of the children's wait
  const int hh = T.absorb[s] ? T.fold_help[s] : -1;
  const int hflag = hh >= 0 ? T.fhelp[hh].flag : 0;
  const int64_t himg = hh >= 0 ? T.fhelp[hh].img : 0, hdofs = hh >= 0 ? T.fhelp[hh].dofs : 0;
  const int hnimg = hh >= 0 ? T.fhelp[hh].nimg : 0;
  {  // the front and its leaf batches must fit the launch's LDS: else a sticky error, never a write
     // past the carve (the symbolic analysis sizes both; this catches a plan that breaks it)
    const int ntot = PK ? r * (r + 1) / 2 : r * ld;
    const int64_t need = 8 * (int64_t)((ntot + 1) & ~1) +
                         (T.absorb[s] ? (int64_t)SymbolicPlan::kFoldRowBytes * T.fold_rmax[s] +
                                            (int64_t)SymbolicPlan::kFoldLeafBytes * T.fold_lmax[s]
                                      : 0);
    if (need > T.lds_cap) {
      if (tid == 0) {
        __hip_atomic_fetch_or(T.err, kErrLdsCarve, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&flags[s], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);  // release the parent
      }
      return;
    }
  }
  if (T.absorb[s]) {  // original entries, then the micro-leaf children folded in LDS
    const int ntot = PK ? r * (r + 1) / 2 : r * ld;
    fold_leaves<PK>(T, s, r, ld, A, Kx, arena, D, st, tol, A + ((ntot + 1) & ~1), cbuf, reinterpret_cast<int32_t*>(MK),
                    dg ? dg + 16 : nullptr, F0, true);  // 16-byte aligned
  } else {  // pre-assembled as the LDS image: a straight copy, 16 loads in flight per thread
    const double* __restrict__ src = fscratch + T.fs_off[s];
    const int n = PK ? r * (r + 1) / 2 : r * ld;
    for (int base = 0; base < n; base += FTN * 16) {
      double v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int q = base + k * FTN + tid;
        v[k] = (q < n) ? src[q] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int q = base + k * FTN + tid;
        if (q < n) A[q] = v[k];
      }
    }
  }
  if (dg) {
    __syncthreads();
    if (tid == 0) dg[1] = wall_clock64();
  }
  if (q1 > q0) {  // the first child's relative indices are symbolic: load them before the wait
    const int c = dep[q0];
    const int uc = T.nrows[c] - (T.first[c + 1] - T.first[c]);
    for (int a = tid; a < uc; a += FTN) rels[a] = T.rel[T.rel_ptr[c] + a];
  }
  if (tid < 64) poll_deps(dep, q0, q1, flags, epoch, err);
  if (hh >= 0 && tid == 0) poll_flag(flags + hflag, epoch, err);  // the helper that folded the first batches
  __syncthreads();
  if (dg && tid == 0) dg[2] = wall_clock64();
  if (hh >= 0) {  // its image — the entries its products reached, in LDS order — added entry by entry,
                  // 16 loads in flight per thread (the untouched entries, zero in the image, are skipped)
    const double* __restrict__ img = T.fimg + himg;
    const uint16_t* __restrict__ hd = T.fimg_dst + hdofs;
    for (int base = 0; base < hnimg; base += FTN * 16) {
      double v[16];
      int q[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int e = min(base + k * FTN + tid, hnimg - 1);
        v[k] = ld_sc1(img + e);
        q[k] = hd[e];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (base + k * FTN + tid < hnimg) A[q[k]] += v[k];
    }
    __syncthreads();
  }
  for (int q = q0; q < q1; ++q) {  // tree children, child order
    const int c = dep[q];
    const int uc = T.nrows[c] - (T.first[c + 1] - T.first[c]);
    const int64_t uld = T.u_ld[c];
    const double* U = arena + T.u_off[c];
    if (q > q0) {
      for (int a = tid; a < uc; a += FTN) rels[a] = T.rel[T.rel_ptr[c] + a];
      __syncthreads();
    }
    // one memory round trip per round: 8 waves x NC columns
    if (uc <= 64)
      push_cols<PK, 1, 8>(A, r, ld, U, uld, uc, rels);
    else if (uc <= 128)
      push_cols<PK, 2, PUSH_NC2>(A, r, ld, U, uld, uc, rels);
    else
      push_cols<PK, 3, PUSH_NC3>(A, r, ld, U, uld, uc, rels);
    __syncthreads();
  }
  if (dg && tid == 0) dg[3] = wall_clock64();
  factor_lds<PK>(T, A, r, w, ld, Dl, MK, cbuf, dg ? dg + 8 : nullptr);
  if (dg && tid == 0) dg[4] = wall_clock64();
  // the parent reads only U: publish it first, then write L and D (read by later launches)
  writeout_u<PK, true>(A, r, w, ld, arena + T.u_off[s], T.u_ld[s]);
  if (dg) {
    __syncthreads();
    if (tid == 0) dg[14] = wall_clock64();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_store(&flags[s], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (dg && tid == 0) dg[15] = wall_clock64();
  writeout_ld<PK>(A, r, w, ld, Dl, arena + T.l_off[s], D, f0, st, tol);
  if (dg && tid == 0) {
    dg[5] = wall_clock64();
    dg[6] = s;
    dg[7] = r;
  }
}

// ---- Medium tree fronts (kFactTreeMax < r <= kFactTreeMedMax): the front F (r x r, ld r, big-front
// storage: L = F[:, :w], U = F[w:, w:] in place) stays in HBM — pre-assembled there by the gather pass
// (original entries + pre-leaf children) — and ONE workgroup factorises it panel by panel, right-looking:
//   children: the tree children's update blocks are added into F (read-modify-write, child order);
//   panel k (columns c0 .. c0 + pw, pw <= 64): rows c0 .. r staged into LDS as an (r - c0) x pw front,
//     factorised by the in-LDS schedule without its Schur pass (blocked_factor_pipe, defer 2), written
//     back (L, d on the diagonal, D, pivot check);
//   trailing update in HBM: F[i, j] -= sum_t L(i, t) d_t L(j, t) over the panel's columns, i >= j >= c0 + pw,
//     16 x 16 tiles on f64 MFMA with both operands from the LDS panel (tile rows along the lanes:
//     16 consecutive rows of one column per store, coalesced); the last panel's tiles are the update
//     block U, stored write-through (sc1) for the parent, then the flag.
// (The level path ran each 64-column panel of these fronts as three launches, k_big_diag -> k_big_trsm
// -> k_big_update, per level: ~37 us per panel plus the launch gaps, supportcase10's fronts r ~ 230.)
constexpr int MED_PW = 64;
__device__ __forceinline__ void med_trailing(double* __restrict__ F, int r, int c0, int pw, const double* A, int ld,
                                             const double* Dl, bool last) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int rp = r - c0;                // panel rows (LDS row i' = front row c0 + i')
  const int nb = (rp - pw + 15) >> 4;   // 16-row blocks of the trailing matrix
  const int ntile = nb * (nb + 1) / 2;
  const int nks = (pw + 3) >> 2;
  const int kl = lane >> 4, il = lane & 15;
  // tile t -> (I, J), J <= I, row-major over the lower triangle; its C entries (lane: row i0 + il,
  // columns j0 + kl + 4 g), clamped in range — the next tile's C is loaded before this tile's MFMAs
  auto coords = [&](int t, int& i0, int& j0) {
    int I = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    while (I * (I + 1) / 2 > t) --I;
    const int J = t - I * (I + 1) / 2;
    i0 = pw + 16 * I;  // LDS rows of the tile's rows (i) and columns (j)
    j0 = pw + 16 * J;
  };
  auto load_c = [&](int t, double (&c)[4]) {
    int i0, j0;
    coords(min(t, ntile - 1), i0, j0);
    const int ic = min(i0 + il, rp - 1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int jc = min(j0 + kl + 4 * g, rp - 1);
      c[g] = F[(int64_t)(c0 + ic) + (int64_t)(c0 + jc) * r];
    }
  };
  // C of the next TWO tiles in flight while a tile's MFMAs run (one ahead left each wave's C loads
  // exposed: a tile's 16 k-steps take ~0.4 us against a ~1-2 us HBM round trip)
  double c[4], cn[4];
  if (wv < ntile) {
    load_c(wv, c);
    load_c(wv + nw, cn);
  }
  for (int t = wv; t < ntile; t += nw) {
    int i0, j0;
    coords(t, i0, j0);
    double cnn[4];
    load_c(t + 2 * nw, cnn);  // (clamped: the last tile's again when there is no such tile)
    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
    const int ja = min(j0 + il, rp - 1), ib = min(i0 + il, rp - 1);
    for (int ks = 0; ks < nks; ++ks) {
      const int k = 4 * ks + kl;
      const int kc = min(k, pw - 1);
      const double d = (k < pw) ? Dl[kc] : 0.0;
      const double av = A[ja + kc * ld] * d;   // A operand: (m = il -> column j0 + il, k)
      const double bv = A[ib + kc * ld];       // B operand: (k, n = il -> row i0 + il)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    // result lane l, element g: (m = kl + 4 g -> column j0 + m, n = il -> row i0 + il)
    const int i = i0 + il;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = j0 + kl + 4 * g;
      if (i < rp && j < rp && i >= j) {
        double* q = F + (int64_t)(c0 + i) + (int64_t)(c0 + j) * r;
        const double v = c[g] - acc[g];
        if (last)
          __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
          *q = v;
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      c[g] = cn[g];
      cn[g] = cnn[g];
    }
  }
}

__device__ __forceinline__ void fact_med_front(const FrontTab& T, int s, const int32_t* __restrict__ dep, int q0, int q1,
                                               int32_t* flags, int epoch, double* arena, double* D, LDLStatus* st,
                                               double tol, int32_t* err, double* A, double* Dl, double* MK, double* cbuf,
                                               int64_t* dg) {
  const int tid = threadIdx.x;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  double* __restrict__ F = arena + T.l_off[s];
  if (dg && tid == 0) dg[1] = wall_clock64();  // (no staging: the front lives in HBM)
  if (tid < 64) poll_deps(dep, q0, q1, flags, epoch, err);
  __syncthreads();
  if (dg && tid == 0) dg[2] = wall_clock64();
  // tree children's update blocks (agent-scope loads: written by other workgroups), child order
  for (int q = q0; q < q1; ++q) {
    const int c = dep[q];
    const int uc = T.nrows[c] - (T.first[c + 1] - T.first[c]);
    const int64_t uld = T.u_ld[c];
    const double* U = arena + T.u_off[c];
    const int32_t* __restrict__ rl = T.rel + T.rel_ptr[c];
    const int ne = uc * uc;
    for (int base = 0; base < ne; base += FTN * 8) {
      double x[8];
      int64_t dst[8];
      int32_t ra[8], rb[8];
      bool ok[8];
      // every load of the round first and unconditional (a, b are in range: e is clamped) — the
      // relative indices loaded under `ok` compiled into a branch with a wait per entry, 8 serial
      // round trips per round (r5: the critical level-3/4 medium fronts of supportcase10 spent 40-60
      // us here)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = min(base + k * FTN + tid, ne - 1);
        const int b = e / uc, a = e - b * uc;
        ok[k] = base + k * FTN + tid < ne && a >= b;
        x[k] = __hip_atomic_load(U + max(a, b) + ucol_off(b, uc, uld), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ra[k] = rl[a];
        rb[k] = rl[b];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(ra[k]), "+v"(rb[k]));
#pragma unroll
      for (int k = 0; k < 8; ++k) dst[k] = ok[k] ? (int64_t)ra[k] + (int64_t)rb[k] * r : -1;
      // the read-modify-writes: every F load of the round first, unconditional from clamped addresses
      // (a masked += compiled into a branch with a wait inside: 8 serial round trips per round)
      double f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = F[max(dst[k], (int64_t)0)];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (dst[k] >= 0) F[dst[k]] = f[k] + x[k];
    }
    __syncthreads();
  }
  if (dg && tid == 0) dg[3] = wall_clock64();
  for (int c0 = 0; c0 < w; c0 += MED_PW) {
    const int pw = min(MED_PW, w - c0), rp = r - c0, ld = rp | 1;
    const bool last = c0 + pw >= w;
    // stage rows c0 .. r of the panel's columns (lower part) into LDS, 16 loads in flight per thread
    const int ne = rp * pw;
    for (int base = 0; base < ne; base += FTN * 16) {
      double v[16];
      int dst[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int e = base + k * FTN + tid;
        const int ec = min(e, ne - 1);
        const int j = ec / rp, i = ec - j * rp;
        v[k] = F[(int64_t)(c0 + i) + (int64_t)(c0 + j) * r];
        dst[k] = (e < ne && i >= j) ? i + j * ld : -1;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (dst[k] >= 0) A[dst[k]] = v[k];
    }
    __syncthreads();
    blocked_factor_pipe<false>(A, rp, pw, ld, Dl, MK, cbuf, 2, nullptr, T.err, 0);
    __syncthreads();
    // write back: L (d on the diagonal), D + pivot check
    for (int base = 0; base < ne; base += FTN * 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = base + k * FTN + tid;
        if (e < ne) {
          const int j = e / rp, i = e - j * rp;
          if (i >= j) F[(int64_t)(c0 + i) + (int64_t)(c0 + j) * r] = (i == j) ? Dl[j] : A[i + j * ld];
        }
      }
    }
    if (tid < pw) {
      const double d = Dl[tid];
      D[f0 + c0 + tid] = d;
      if (bad_pivot(d, tol)) atomicMin(&st->fail_pivot, f0 + c0 + tid + 1);
    }
    if (rp > pw) med_trailing(F, r, c0, pw, A, ld, Dl, last);
    __syncthreads();  // the next panel's staging reads the updated trailing matrix; A is rewritten
  }
  if (dg && tid == 0) dg[4] = wall_clock64();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_store(&flags[s], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (dg && tid == 0) {
    dg[5] = wall_clock64();
    dg[6] = s;
    dg[7] = r;
  }
}

// A fold helper: the first batches of a front's micro leaves (FoldHelp [b0, b1)) folded into a zeroed
// LDS image of the front — their L and D written as the front's own — and the image stored
// write-through for the front, which adds it after its own batches and waits (fixed order: bitwise
// reproducible).  The helpers take the first tickets, so the heaviest fronts' folds are split over two
// CUs (ex10: 272 fronts of 35-50 us of folding on 256 CUs made the 16 late level-2 fronts the chain).
template <bool PK>
__device__ __forceinline__ void fold_help_task(const FrontTab& T, int h, int32_t* flags, int epoch, const double* Kx,
                                               double* arena, double* D, LDLStatus* st, double tol, double* A,
                                               double* MK, double* cbuf) {
  const int tid = threadIdx.x;
  const FoldHelp H = T.fhelp[h];
  const int s = H.front, r = T.nrows[s], ld = PK ? 0 : (r | 1);
  const int ntot = PK ? r * (r + 1) / 2 : r * ld;
  const int64_t need = 8 * (int64_t)((ntot + 1) & ~1) + (int64_t)SymbolicPlan::kFoldRowBytes * T.fold_rmax[s] +
                       (int64_t)SymbolicPlan::kFoldLeafBytes * T.fold_lmax[s];
  if (need > T.lds_cap) {  // as the front's own check: a sticky error, never a write past the carve
    if (tid == 0) {
      __hip_atomic_fetch_or(T.err, kErrLdsCarve, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&flags[H.flag], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  fold_leaves<PK>(T, s, r, ld, A, Kx, arena, D, st, tol, A + ((ntot + 1) & ~1), cbuf, reinterpret_cast<int32_t*>(MK),
                  nullptr, H.fs, false);
  __syncthreads();
  double* __restrict__ img = T.fimg + H.img;  // only the entries its products reached (fimg_dst)
  const uint16_t* __restrict__ hd = T.fimg_dst + H.dofs;
  for (int k = tid; k < H.nimg; k += FTN) st_sc1(img + k, A[hd[k]]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_store(&flags[H.flag], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FTN) void k_fact_tree(FrontTab T, const int32_t* __restrict__ order, int nt, int nhelp,
                                                  const int32_t* __restrict__ dep_ptr, const int32_t* __restrict__ dep,
                                                  int32_t* counter, int32_t* flags, int epoch,
                                                  const double* __restrict__ Kx, double* arena,
                                                  const double* __restrict__ fscratch, double* D, LDLStatus* st,
                                                  double tol, int32_t* err, int64_t* dbg) {
  extern __shared__ __attribute__((aligned(16))) double A[];
  __shared__ double Dl[192];
  __shared__ double MK[16 * LDM];
  __shared__ __attribute__((aligned(16))) double cbuf[2 * 16 * LDM];
  __shared__ int32_t rels[192];
  __shared__ int s_task;
  if (threadIdx.x == 0) s_task = atomicAdd(counter, 1);
  __syncthreads();
  const int t = s_task;
  if (t >= nt) return;
  if (t < nhelp) {  // fold helper tickets first (no dependencies)
    const int sh = T.fhelp[t].front;
    if (T.nrows[sh] <= 128 && !T.fold_pk[sh])
      fold_help_task<false>(T, t, flags, epoch, Kx, arena, D, st, tol, A, MK, cbuf);
    else
      fold_help_task<true>(T, t, flags, epoch, Kx, arena, D, st, tol, A, MK, cbuf);
  } else {
  const int s = order[t - nhelp];
  int64_t* dg = dbg ? dbg + 24 * t : nullptr;
  if (dg && threadIdx.x == 0) dg[0] = wall_clock64();
  if (T.nrows[s] > SymbolicPlan::kFactTreeMax)
    fact_med_front(T, s, dep, dep_ptr[t], dep_ptr[t + 1], flags, epoch, arena, D, st, tol, err, A, Dl, MK, cbuf, dg);
  else if (T.nrows[s] <= 128 && !T.fold_pk[s])
    fact_tree_front<false>(T, s, dep, dep_ptr[t], dep_ptr[t + 1], flags, epoch, Kx, arena, fscratch, D, st, tol, err, A, Dl,
                           MK, cbuf, rels, dg);
  else
    fact_tree_front<true>(T, s, dep, dep_ptr[t], dep_ptr[t + 1], flags, epoch, Kx, arena, fscratch, D, st, tol, err, A, Dl,
                          MK, cbuf, rels, dg);
  }
  if (threadIdx.x == 0 && atomicAdd(counter + 1, 1) == nt - 1) {  // last one out: reset the tickets
    counter[0] = 0;
    counter[1] = 0;
  }
}

// Diagonal block of 64-column panel `step` (one workgroup per front): load, blocked factorisation,
// write L11 (d on the diagonal), D and the M_K blocks for k_big_trsm.
// The diagonal block of panel `step` of front s, staged in A64 (lower part, identity-padded past kw):
// blocked factorisation, then L11 (d on the diagonal), D and the M_K blocks for k_big_trsm.
// Loads / stores of the big-front panel kernels: plain in their own launches (kernel boundaries order
// them), write-through (sc1) stores and sc1 loads inside k_big_dag, whose tasks hand tiles to each
// other within one launch (every handed-off byte stored sc1 and drained before the flag, every load
// of it sc1: the guide's Guideline 16, R1 without an acquire).
// (global address space explicitly: inside a non-inlined task body a generic pointer compiles to flat_
// loads / stores, which also count on lgkmcnt — every LDS wait then waits for them — and are not the
// global_ sc1 accesses the hand-off protocol requires)
typedef __attribute__((address_space(1))) double gdouble;
template <bool SC>
__device__ __forceinline__ double ldF(const double* p) {
  if constexpr (SC) return __hip_atomic_load((const gdouble*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *(const gdouble*)p;
}
template <bool SC>
__device__ __forceinline__ void stF(double* p, double v) {
  if constexpr (SC) __hip_atomic_store((gdouble*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *(gdouble*)p = v;
}
static_assert(BIG_MSZ == 4 * 16 * LDM, "one panel's M_K blocks");

// the diagonal block of panel `step`, staged in A64: factorised; L11 (d on the diagonal), D and the
// M_K blocks (to M: the front's slot in Mbuf, or the panel's slot in k_big_dag's Mch) written
template <bool SC = false>
__device__ __forceinline__ void big_diag_tail(const FrontTab& T, int s, int step, double* A64, double* Ms, double* Dl,
                                              double* __restrict__ arena, double* __restrict__ D,
                                              double* __restrict__ M, LDLStatus* st, double tol) {
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int k0 = step * 64, kw = min(64, w - k0);
  double* __restrict__ F = arena + T.l_off[s] + k0 + (int64_t)k0 * r;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  diag64(A64, Dl, Ms, tid);
  for (int j = wv; j < kw; j += 4)
    if (lane >= j && lane < kw) stF<SC>(F + lane + (int64_t)j * r, (lane == j) ? Dl[j] : A64[lane + j * LDA]);
  if (tid < kw) {
    const double d = Dl[tid];
    stF<SC>(D + f0 + k0 + tid, d);
    if (bad_pivot(d, tol)) atomicMin(&st->fail_pivot, f0 + k0 + tid + 1);
  }
  for (int e = tid; e < BIG_MSZ; e += NT) stF<SC>(M + e, Ms[e]);
}

// Lookahead: the update launch of panel `step` leaves panel step + 1's diagonal tile final in the
// workgroup of its task (0, 0), which factorises it right away (big_diag_tail) while the launch's
// other tiles are still updated — no k_big_diag launch, and its latency off the panel chain, for
// every panel but the first.  Entry (i, j) of the tile (< 64 each) arrives through put(i, j, v).
__device__ __forceinline__ bool big_next_diag(const FrontTab& T, int s, int step) {
  return 64 * (step + 1) < T.first[s + 1] - T.first[s];
}
__device__ __forceinline__ void big_diag_prepare(double* A64, int kw) {
  const int tid = threadIdx.x;
  for (int e = tid; e < 64 * 64; e += NT) {
    const int i = e & 63, j = e >> 6;
    A64[i + j * LDA] = (i < kw && j < kw) ? 0.0 : (i == j ? 1.0 : 0.0);
  }
}

// the diagonal block of panel `step`: staged (identity-padded past kw), factorised, written (big_diag_tail)
template <bool SC>
__device__ __forceinline__ void diag_body(const FrontTab& T, int s, int step, double* __restrict__ arena,
                                          double* __restrict__ D, double* __restrict__ M, LDLStatus* st, double tol,
                                          double* sm) {
  double* A64 = sm;
  double* Ms = sm + 64 * LDA;
  double* Dl = Ms + 4 * 16 * LDM;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int k0 = step * 64, kw = min(64, w - k0);
  const double* __restrict__ F = arena + T.l_off[s] + k0 + (int64_t)k0 * r;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  (void)f0;
  {
    // all 16 loads in flight from clamped addresses, masked after (a predicated load compiles into a
    // branch with a wait of its own)
    double v[16];
    const int lc = min(lane, kw - 1);
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = ldF<SC>(F + lc + (int64_t)min(wv + 4 * e, kw - 1) * r);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = wv + 4 * e;
      A64[lane + j * LDA] = (lane < kw && j < kw) ? (lane >= j ? v[e] : 0.0) : (lane == j ? 1.0 : 0.0);
    }
  }
  __syncthreads();
  big_diag_tail<SC>(T, s, step, A64, Ms, Dl, arena, D, M, st, tol);
}
constexpr int DIAG_LDS = 64 * LDA + 4 * 16 * LDM + 64;
__global__ __launch_bounds__(NT) void k_big_diag(FrontTab T, const int32_t* __restrict__ list, int step,
                                                 double* __restrict__ arena, double* __restrict__ D,
                                                 double* __restrict__ Mbuf, LDLStatus* st, double tol) {
  __shared__ __attribute__((aligned(16))) double sm[DIAG_LDS];
  int s, item;
  task_of(list, s, item);
  (void)item;
  diag_body<false>(T, s, step, arena, D, Mbuf + (int64_t)T.bigslot[s] * 4096, st, tol, sm);
}

// Rows below the diagonal block of panel `step` (64-row tiles; wave w owns 16 rows): blocked
// forward substitution X_K = A_K - sum_{J<K} (L_J D_J) L_KJ^T, L_K = X_K M_K, all on f64 MFMA.
// LDS of one k_big_trsm task: L11 (64 x LDA), the M_K blocks, the pivots, four 16 x 64 slabs
constexpr int TRSM_LDS = 64 * LDA + BIG_MSZ + 64 + 4 * 17 * 64;
template <bool SC>
__device__ __forceinline__ void trsm_body(const FrontTab& T, int s, int step, int rt, double* __restrict__ arena,
                                          const double* __restrict__ D, const double* __restrict__ M, double* sm) {
  double* L11 = sm;
  double* Ms = sm + 64 * LDA;
  double* Dl = Ms + BIG_MSZ;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int k0 = step * 64, kw = min(64, w - k0);
  const int I0 = k0 + kw + rt * 64;
  double* __restrict__ F = arena + T.l_off[s];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* S = Dl + 64 + wv * (17 * 64);  // this wave's slab: 16 rows x 64 cols, S[m + 17 * j]
  const int row = I0 + 16 * wv + (lane & 15);  // slab row of this lane; 4 columns per pass
  {
    // every operand load in flight at once from clamped addresses, masked at the LDS stores (a
    // predicated load compiles into a branch with a wait of its own)
    double lv[16], sv[16], mv[5], dv;
    const int lc = min(lane, kw - 1), rc = min(row, r - 1);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      lv[e] = ldF<SC>(F + (k0 + lc) + (int64_t)(k0 + min(wv + 4 * e, kw - 1)) * r);
      sv[e] = ldF<SC>(F + rc + (int64_t)(k0 + min((lane >> 4) + 4 * e, kw - 1)) * r);
    }
#pragma unroll
    for (int e = 0; e < 5; ++e) mv[e] = ldF<SC>(M + min(tid + e * NT, BIG_MSZ - 1));
    dv = ldF<SC>(D + f0 + k0 + min(tid, kw - 1));
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = wv + 4 * e, jj = (lane >> 4) + 4 * e;
      L11[lane + j * LDA] = (lane < kw && j < kw && lane > j) ? lv[e] : 0.0;
      S[(lane & 15) + jj * 17] = (row < r && jj < kw) ? sv[e] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < 5; ++e)
      if (tid + e * NT < BIG_MSZ) Ms[tid + e * NT] = mv[e];
    if (tid < 64) Dl[tid] = (tid < kw) ? dv : 1.0;
  }
  __syncthreads();
  for (int K = 0; K < 4; ++K) {
    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int J = 0; J < K; ++J) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int k = 16 * J + 4 * ks + (lane >> 4);
        const double av = S[(lane & 15) + k * 17] * Dl[k];
        const double bv = L11[(16 * K + (lane & 15)) + k * LDA];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) S[((lane >> 4) + 4 * g) + (16 * K + (lane & 15)) * 17] -= acc[g];
    wave_sync();
    dbl4 l = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k = 4 * ks + (lane >> 4);
      const double av = S[(lane & 15) + (16 * K + k) * 17];
      const double bv = Ms[K * 16 * LDM + k * LDM + (lane & 15)];
      l = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, l, 0, 0, 0);
    }
    wave_sync();
#pragma unroll
    for (int g = 0; g < 4; ++g) S[((lane >> 4) + 4 * g) + (16 * K + (lane & 15)) * 17] = l[g];
    wave_sync();
  }
  for (int j = lane >> 4; j < kw; j += 4)
    if (row < r) stF<SC>(F + row + (int64_t)(k0 + j) * r, S[(lane & 15) + j * 17]);
}

// Rows below the diagonal block of panel `step` (64-row tiles; wave w owns 16 rows): blocked
// forward substitution X_K = A_K - sum_{J<K} (L_J D_J) L_KJ^T, L_K = X_K M_K, all on f64 MFMA.
__global__ __launch_bounds__(NT) void k_big_trsm(FrontTab T, const int32_t* __restrict__ list, int step,
                                                 double* __restrict__ arena, const double* __restrict__ D,
                                                 const double* __restrict__ Mbuf) {
  __shared__ __attribute__((aligned(16))) double sm[TRSM_LDS];
  int s, rt;
  task_of(list, s, rt);
  trsm_body<false>(T, s, step, rt, arena, D, Mbuf + (int64_t)T.bigslot[s] * 4096, sm);
}

// Trailing update of one 64x64 lower tile: C -= (L_I D) L_J^T, f64 MFMA 16x16x4, over K = the
// columns of up to kpan panels (deferred multi-panel update).  Task tij = ti | tj << 16 | mode << 31:
//   mode 0 (local): K = panel `step` only, tiles relative to the panel's end, columns limited to the
//     end of the panel group (kpan panels from (step / kpan) kpan): the group's later panels only;
//   mode 1 (trailing): K = the panels of the group ending at `step`, tiles relative to the group's
//     end: the rest of the front, ONE load/store of C per group instead of one per panel.
// kpan = 1: every step is a group of one (the r2 right-looking update).  The K chunks of 64 are
// staged through LDS one after another; the next chunk's operands are loaded (from
// clamped addresses) while the current chunk's MFMAs run.
constexpr int UPD_LDT = 80;  // [k][row] layout: conflict-free ds_read_b64 for the 16x4 operand pattern
constexpr int UPD_LDS = 2 * 64 * UPD_LDT;
// Mnext: where the lookahead diagonal block's M_K blocks go (the front's Mbuf slot; k_big_dag: the
// next panel's slot)
template <bool SC>
__device__ __forceinline__ void update_body(const FrontTab& T, int s, int step, int kpan, int tij,
                                            double* __restrict__ arena, double* __restrict__ D,
                                            double* __restrict__ Mnext, LDLStatus* st, double tol, double* WLt) {
  constexpr int LDT = UPD_LDT;
  double* Wt = WLt;
  double* Lt = WLt + 64 * LDT;
  static_assert(64 * LDA <= 64 * LDT && 4 * 16 * LDM + 64 <= 64 * LDT, "lookahead diagonal block aliases Wt / Lt");
  const int ti = tij & 0xffff, tj = (tij >> 16) & 0x7fff;
  const bool trailing = tij < 0;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int g0 = (step / kpan) * kpan;                         // first panel of the group
  const int gend = min(64 * (g0 + kpan), w);                   // first column after the group
  const int kb = trailing ? 64 * g0 : 64 * step;               // K range [kb, ke)
  const int ke = trailing ? gend : min(64 * step + 64, w);
  const int c0 = ke;                                           // tiles relative to the K range's end
  const int jlim = trailing ? r : gend;
  const int I0 = c0 + ti * 64, J0 = c0 + tj * 64;
  const int nch = (ke - kb + 63) >> 6;                         // K chunks of 64 (<= kpan)
  double* __restrict__ F = arena + T.l_off[s];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int qr = (wv >> 1) * 32, qc = (wv & 1) * 32;
  const int ri = min(I0 + lane, r - 1), rj = min(J0 + lane, r - 1);
  // operands of chunk ch: columns kb + 64 ch + wv + 4 e (clamped into the K range); one register
  // set, reloaded with the next chunk right after its LDS stores, so those loads run under the
  // current chunk's MFMAs (which read LDS only)
  double wl[16], ll[16], dk[16];
  auto load = [&](int ch) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kk = min(kb + 64 * ch + wv + 4 * e, ke - 1);
      const int64_t col = (int64_t)kk * r;
      wl[e] = ldF<SC>(F + ri + col);
      ll[e] = ldF<SC>(F + rj + col);
      dk[e] = ldF<SC>(D + f0 + kk);
    }
  };
  load(0);
  // C tile prefetch (its latency overlaps the first chunk)
  double c[2][2][4];
#pragma unroll
  for (int bj = 0; bj < 2; ++bj)
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = min(I0 + qr + bi * 16 + (lane & 15), r - 1);
        const int j = min(J0 + qc + bj * 16 + (lane >> 4) + 4 * g, r - 1);
        c[bj][bi][g] = ldF<SC>(F + i + (int64_t)j * r);  // masked at the store
      }
  dbl4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = dbl4{0.0, 0.0, 0.0, 0.0};
  for (int ch = 0; ch < nch; ++ch) {
    const int kc = kb + 64 * ch, kw = min(64, ke - kc);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kk = wv + 4 * e;
      Wt[kk * LDT + lane] = (kk < kw && I0 + lane < r) ? wl[e] * dk[e] : 0.0;
      Lt[kk * LDT + lane] = (kk < kw && J0 + lane < r) ? ll[e] : 0.0;
    }
    __syncthreads();
    if (ch + 1 < nch) load(ch + 1);  // wave-uniform
    const int nks = (kw + 3) >> 2;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      if (ks < nks) {  // wave-uniform
        const int kk = ks * 4 + (lane >> 4);
        const double a0 = Lt[kk * LDT + qc + (lane & 15)];
        const double a1 = Lt[kk * LDT + qc + 16 + (lane & 15)];
        const double b0 = Wt[kk * LDT + qr + (lane & 15)];
        const double b1 = Wt[kk * LDT + qr + 16 + (lane & 15)];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    if (ch + 1 < nch) __syncthreads();  // the LDS tiles are rewritten by the next chunk
  }
  // D layout: col n = lane&15 (-> row i of F), row m = (lane>>4) + 4g (-> column j of F)
#pragma unroll
  for (int bj = 0; bj < 2; ++bj)
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = I0 + qr + bi * 16 + (lane & 15);
        const int j = J0 + qc + bj * 16 + (lane >> 4) + 4 * g;
        if (i < r && j < jlim && i >= j) stF<SC>(F + i + (int64_t)j * r, c[bj][bi][g] - acc[bj][bi][g]);
      }
  // lookahead: task (0, 0) of a local update holds the next panel's diagonal tile, final now (the
  // panel's last local update; the next panel lies inside the group, below jlim)
  // (trailing mode, k_big_dag's tiles next to the group: only when the group is full, c0 = its end)
  if (ti == 0 && tj == 0 && (!trailing || 64 * (step + 1) == c0) && big_next_diag(T, s, step)) {
    double* A64 = Wt;  // the operand tiles are free: aliased by the diagonal block, M_K and pivots
    double* Ms = Lt;
    double* Dl = Lt + 4 * 16 * LDM;
    const int kw = min(64, w - c0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the tile's C stores land before L11's (same addresses)
    __syncthreads();  // every wave's last MFMA operand read
    big_diag_prepare(A64, kw);
    __syncthreads();
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int i = qr + bi * 16 + (lane & 15), j = qc + bj * 16 + (lane >> 4) + 4 * g;
          if (i < kw && j < kw && i >= j) A64[i + j * LDA] = c[bj][bi][g] - acc[bj][bi][g];
        }
    __syncthreads();
    big_diag_tail<SC>(T, s, step + 1, A64, Ms, Dl, arena, D, Mnext, st, tol);
  }
}

__global__ __launch_bounds__(NT) void k_big_update(FrontTab T, const int32_t* __restrict__ list, int step, int kpan,
                                                   double* __restrict__ arena, double* __restrict__ D,
                                                   double* __restrict__ Mbuf, LDLStatus* st, double tol) {
  __shared__ __attribute__((aligned(16))) double WLt[UPD_LDS];
  int s, tij;
  task_of(list, s, tij);
  update_body<false>(T, s, step, kpan, tij, arena, D, Mbuf + (int64_t)T.bigslot[s] * 4096, st, tol, WLt);
}

// (pos, neg, zero) of D over the columns with colmask == want (colmask NULL: all)
__global__ __launch_bounds__(NT) void k_inertia(const double* __restrict__ D, int n, LDLStatus* st, int spd,
                                                const uint8_t* __restrict__ colmask, int want) {
  __shared__ int red[3][NT / 64];
  int pos = 0, neg = 0, zero = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (colmask && colmask[i] != want) continue;
    const double d = D[i];
    pos += d > 0.0;
    neg += d < 0.0;
    zero += !(d > 0.0) && !(d < 0.0);
    if (spd && !(d > 0.0)) atomicMin(&st->fail_pivot, i + 1);
  }
  for (int o = 32; o > 0; o >>= 1) {
    pos += __shfl_down(pos, o, 64);
    neg += __shfl_down(neg, o, 64);
    zero += __shfl_down(zero, o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wv] = pos;
    red[1][wv] = neg;
    red[2][wv] = zero;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int v = 0;
    for (int q = 0; q < NT / 64; ++q) v += red[threadIdx.x][q];
    atomicAdd(threadIdx.x == 0 ? &st->npos : (threadIdx.x == 1 ? &st->nneg : &st->nzero), v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && want != 1) st->t1 = wall_clock64();  // end of the factorisation
}

// LDLSolver::count_inertia (lazily, after a factorisation without k_inertia): clear the counts; then
// k_inertia with want = 1 and no column mask counts every pivot and leaves the t1 stamp alone
__global__ void k_zero_counts(LDLStatus* st) { st->npos = st->nneg = st->nzero = 0; }

// ------------------------------------------------------------------ batched leaf columns (SymbolicPlan::lb)
// A group: n single-column leaf fronts c_j under one parent P, W (m x n, ld m) = their K columns on the
// parent rows gpos, d_j = K(c_j, c_j).  Factor: L(:, c_j) = W(:, j) / d_j, and P absorbs
// F_P[gpos, gpos] -= W D^{-1} W^T (one SYRK instead of n rank-1 fronts).

// W / d from the caller's values: one workgroup per member column (contiguous CSC run)
__global__ __launch_bounds__(NT) void k_lb_build(const SymbolicPlan::LBGroup* __restrict__ G,
                                                 const int32_t* __restrict__ gid, const int32_t* __restrict__ mem,
                                                 const int64_t* __restrict__ cs, const int64_t* __restrict__ ce,
                                                 const int64_t* __restrict__ wbase, const int32_t* __restrict__ wrow,
                                                 const double* __restrict__ Kx, double* __restrict__ W,
                                                 double* __restrict__ dlb, double* __restrict__ dinv,
                                                 double* __restrict__ D, LDLStatus* st, double tol) {
  const int j = blockIdx.x;
  const SymbolicPlan::LBGroup g = G[gid[j]];
  double* __restrict__ Wc = W + g.w_off + (int64_t)(j - g.mem_off) * g.m;
  const int64_t c0 = cs[j], c1 = ce[j];
  const int32_t* __restrict__ wr = wrow + wbase[j] - c0;
  for (int64_t e = c0 + threadIdx.x; e < c1; e += NT) {
    const int k = wr[e];
    const double v = Kx[e];
    if (k >= 0) {
      Wc[k] = v;
    } else {
      dlb[j] = v;
      dinv[j] = 1.0 / v;
      D[mem[j]] = v;
      if (bad_pivot(v, tol)) atomicMin(&st->fail_pivot, mem[j] + 1);
    }
  }
}

// F[gpos[a], gpos[b]] -= sum_{j in [k0, k1)} W[a, j] W[b, j] / d_j for a >= b: 128 x 128 output
// tiles (lower), 4 waves of 64 x 64 (4 x 4 f64 MFMA 16x16x4 blocks each), K staged through LDS
// 16 columns at a time (double-buffered, operands [k][row] with a padded stride).  One launch per
// K-chunk keeps the chunk of W (m x 2048) resident in the Infinity Cache across all tiles.
constexpr int SYT = 128, SYK = 16, SYLD = SYT + 16;
#ifndef SYRK_WAVES
#define SYRK_WAVES 2  // waves per SIMD the register budget is cut for (2: accumulators in VGPRs, 2 WGs per CU)
#endif
__global__ __launch_bounds__(NT, SYRK_WAVES) void k_lb_syrk(const double* __restrict__ W, const double* __restrict__ dinv, int m,
                                                int k0, int k1, const int32_t* __restrict__ gpos,
                                                double* __restrict__ F, int ld) {
  __shared__ __attribute__((aligned(16))) double As[2][SYK * SYLD];  // (W D^{-1})[I rows]
  __shared__ __attribute__((aligned(16))) double Bs[2][SYK * SYLD];  // W[J rows]
  int I = 0, rem = blockIdx.x;
  while (rem > I) {
    rem -= I + 1;
    ++I;
  }
  const int J = rem;
  const int I0 = I * SYT, J0 = J * SYT;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;  // wave's 64 x 64 quadrant: I rows wm.., J rows wn..
  const int lr = tid & (SYT - 1), lk = tid >> 7;      // loader: row lr, columns lk + 2q
  dbl4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = dbl4{0.0, 0.0, 0.0, 0.0};
  // the next chunk's operands: loads from clamped addresses, issued together and consumed (masked,
  // scaled) only at the LDS store after the current chunk's MFMAs — a predicated load compiled into a
  // branch with a wait inside, exposing 8 memory latencies per chunk (SQ_WAIT_ANY 55 % of wave cycles)
  double ra[8], rb[8], rd[8];
  auto gload = [&](int kb) {
    const int ri = min(I0 + lr, m - 1), rj = min(J0 + lr, m - 1);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int kc = min(kb + lk + 2 * q, k1 - 1);
      const int64_t col = (int64_t)kc * m;
      ra[q] = W[ri + col];
      rb[q] = W[rj + col];
      rd[q] = dinv[kc];
    }
  };
  auto sstore = [&](int kb, int buf) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool ok = kb + lk + 2 * q < k1;
      As[buf][(lk + 2 * q) * SYLD + lr] = (ok && I0 + lr < m) ? ra[q] * rd[q] : 0.0;
      Bs[buf][(lk + 2 * q) * SYLD + lr] = (ok && J0 + lr < m) ? rb[q] : 0.0;
    }
  };
  gload(k0);
  sstore(k0, 0);
  __syncthreads();
  int buf = 0;
  for (int kb = k0; kb < k1; kb += SYK) {
    const bool more = kb + SYK < k1;
    if (more) gload(kb + SYK);
#pragma unroll
    for (int k4 = 0; k4 < SYK / 4; ++k4) {
      const int kk = 4 * k4 + (lane >> 4);
      double fa[4], fb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        fa[t] = Bs[buf][kk * SYLD + wn + 16 * t + (lane & 15)];  // A operand: W_J rows (m)
        fb[t] = As[buf][kk * SYLD + wm + 16 * t + (lane & 15)];  // B operand: (W D^-1)_I rows (n)
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    if (more) {
      sstore(kb + SYK, buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }
  // acc[a][b][g]: row i = I0 + wm + 16 b + (lane & 15), column j = J0 + wn + 16 a + (lane >> 4) + 4 g.
  // F read-modify-written 16 entries at a time: the reads from clamped addresses, all in flight
  // together, the writes masked (a masked read-modify-write per entry compiled into a branch with a
  // wait inside: 64 serial memory latencies per lane)
  int gi[4], gj[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b) gi[b] = gpos[min(I0 + wm + 16 * b + (lane & 15), m - 1)];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int g = 0; g < 4; ++g) gj[a][g] = gpos[min(J0 + wn + 16 * a + (lane >> 4) + 4 * g, m - 1)];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    double fv[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) fv[b][g] = F[gi[b] + (int64_t)gj[a][g] * ld];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = I0 + wm + 16 * b + (lane & 15), j = J0 + wn + 16 * a + (lane >> 4) + 4 * g;
        if (i < m && j <= i) F[gi[b] + (int64_t)gj[a][g] * ld] = fv[b][g] - acc[a][b][g];
      }
  }
}

// Trailing update of a big front's panel group on 128 x 128 lower tiles (the group's K = 64 kpan columns,
// tiles relative to the group's end c0): C -= (L_I D) L_J^T, four waves x 64 x 64 quadrants of f64 MFMA
// 16x16x4, K-chunks of 16 double-buffered through LDS (k_lb_syrk's engine on the front's own columns).
// A 128-tile reads 2 x 128 K doubles per 2 x 128^2 K flops — twice k_big_update's 64-tile arithmetic
// intensity, on the update that carries ~90 % of neos' factorisation flops.
// Split K (nsplit > 1, launches of few tiles: one workgroup per CU ran each tile's K chain with its
// loads exposed, ~67 us per tile whatever the launch size on neos): workgroup blockIdx.x takes part
// blockIdx.x % nsplit of tile blockIdx.x / nsplit's K range (16-column chunks), stores its partial
// product write-through (psum), and the last part to take the tile's ticket sums the partials in part
// order (fixed: bitwise reproducible), then runs the epilogue (and the lookahead of tile (0, 0)).
constexpr int U128_LDS = 4 * SYK * SYLD;   // As[2] then Bs[2]
// acc[a][b] += sum_{k in [k0, k1)} (L D)[I0 + rows, k] L[J0 + cols, k] on a 128 x 128 tile of front F (ld r):
// four waves x 64 x 64 quadrants of f64 MFMA 16x16x4, K-chunks of 16 double-buffered through LDS (AB)
template <bool SC>
__device__ __forceinline__ void upd128_gemm(const double* __restrict__ F, const double* __restrict__ D, int f0, int r,
                                            int I0, int J0, int k0, int k1, double* AB, dbl4 (&acc)[4][4]) {
  double (*As)[SYK * SYLD] = reinterpret_cast<double (*)[SYK * SYLD]>(AB);           // (L D)[I rows]
  double (*Bs)[SYK * SYLD] = reinterpret_cast<double (*)[SYK * SYLD]>(AB + 2 * SYK * SYLD);  // L[J rows]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
  const int lr = tid & (SYT - 1), lk = tid >> 7;
  double ra[8], rb[8], rd[8];
  const int ri = min(I0 + lr, r - 1), rj = min(J0 + lr, r - 1);
  auto gload = [&](int kb) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int kc = min(kb + lk + 2 * q, k1 - 1);
      const int64_t col = (int64_t)kc * r;
      ra[q] = ldF<SC>(F + ri + col);
      rb[q] = ldF<SC>(F + rj + col);
      rd[q] = ldF<SC>(D + f0 + kc);
    }
  };
  auto sstore = [&](int kb, int buf) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool ok = kb + lk + 2 * q < k1;
      As[buf][(lk + 2 * q) * SYLD + lr] = (ok && I0 + lr < r) ? ra[q] * rd[q] : 0.0;
      Bs[buf][(lk + 2 * q) * SYLD + lr] = (ok && J0 + lr < r) ? rb[q] : 0.0;
    }
  };
  if (k0 >= k1) return;  // (a split part past the group's K has nothing to multiply)
  gload(k0);
  sstore(k0, 0);
  __syncthreads();
  int buf = 0;
  for (int kb = k0; kb < k1; kb += SYK) {
    const bool more = kb + SYK < k1;
    if (more) gload(kb + SYK);
#pragma unroll
    for (int k4 = 0; k4 < SYK / 4; ++k4) {
      const int kk = 4 * k4 + (lane >> 4);
      double fa[4], fb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        fa[t] = Bs[buf][kk * SYLD + wn + 16 * t + (lane & 15)];
        fb[t] = As[buf][kk * SYLD + wm + 16 * t + (lane & 15)];
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    if (more) {
      sstore(kb + SYK, buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }
}

__global__ __launch_bounds__(NT, 2) void k_big_upd128(FrontTab T, const int32_t* __restrict__ list, int step, int kpan,
                                                     double* __restrict__ arena, double* __restrict__ D,
                                                     double* __restrict__ Mbuf, LDLStatus* st, double tol,
                                                     int nsplit, double* __restrict__ psum, int32_t* ptick) {
  // one buffer: As[2] then Bs[2]; after the MFMAs task (0, 0) reuses it for the lookahead diagonal block
  __shared__ __attribute__((aligned(16))) double AB[U128_LDS];
  __shared__ int s_last;
  static_assert(64 * LDA + 4 * 16 * LDM + 64 <= U128_LDS, "lookahead diagonal block aliases As / Bs");
  const int tile = blockIdx.x / nsplit, part = blockIdx.x - tile * nsplit;
  const int2 task = reinterpret_cast<const int2*>(list)[tile];
  const int s = task.x, tij = task.y;
  const int ti = tij & 0xffff, tj = (tij >> 16) & 0x7fff;
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int g0 = (step / kpan) * kpan;
  const int kg0 = 64 * g0, k1g = min(64 * (g0 + kpan), w);  // K range = the group's columns
  const int c0 = k1g;
  const int kps = ((k1g - kg0 + nsplit - 1) / nsplit + SYK - 1) / SYK * SYK;  // this part's K columns
  const int k0 = min(kg0 + part * kps, k1g), k1 = min(k0 + kps, k1g);
  const int I0 = c0 + ti * SYT, J0 = c0 + tj * SYT;
  double* __restrict__ F = arena + T.l_off[s];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
  dbl4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = dbl4{0.0, 0.0, 0.0, 0.0};
  upd128_gemm<false>(F, D, f0, r, I0, J0, k0, k1, AB, acc);
  if (nsplit > 1) {  // the tile's parts: partials write-through, the last part sums them in part order
    double* __restrict__ mine = psum + ((int64_t)tile * nsplit + part) * UPD_PART;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g) st_sc1(mine + ((a * 4 + b) * 4 + g) * NT + tid, acc[a][b][g]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
      s_last = __hip_atomic_fetch_add(ptick + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsplit - 1;
    __syncthreads();
    if (!s_last) return;
    if (tid == 0) ptick[tile] = 0;  // every part has taken its ticket: ready for the next launch
    // the sum in part order, every part (this one's too) read back: 8 values of every part per round,
    // all 32 loads in flight (unconditional, the part index clamped; a load per value in a runtime
    // loop compiled to one memory round trip per load)
    const double* __restrict__ all = psum + (int64_t)tile * nsplit * UPD_PART;
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      double pv[4][8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double* pq = all + (int64_t)min(q, nsplit - 1) * UPD_PART + tid;
#pragma unroll
        for (int u = 0; u < 8; ++u) pv[q][u] = ld_sc1(pq + (h * 8 + u) * NT);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = h * 8 + u, a = e >> 4, b = (e >> 2) & 3, g = e & 3;
        double v = pv[0][u];
#pragma unroll
        for (int q = 1; q < 4; ++q) v = (q < nsplit) ? v + pv[q][u] : v;
        acc[a][b][g] = v;
      }
    }
  }
  // acc[a][b][g]: row i = I0 + wm + 16 b + (lane & 15), column j = J0 + wn + 16 a + (lane >> 4) + 4 g;
  // the C reads of a column block from clamped addresses, all in flight, the writes masked
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    double fv[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = min(I0 + wm + 16 * b + (lane & 15), r - 1), j = min(J0 + wn + 16 * a + (lane >> 4) + 4 * g, r - 1);
        fv[b][g] = F[i + (int64_t)j * r];
      }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = I0 + wm + 16 * b + (lane & 15), j = J0 + wn + 16 * a + (lane >> 4) + 4 * g;
        if (i < r && j <= i) F[i + (int64_t)j * r] = fv[b][g] - acc[a][b][g];
        acc[a][b][g] = fv[b][g] - acc[a][b][g];  // kept for the lookahead diagonal block below
      }
  }
  // lookahead: task (0, 0) holds the next panel's diagonal tile (rows / columns [c0, c0 + 64): wave 0's
  // quadrant), final now — the group's trailing update is its last before that panel
  if (ti == 0 && tj == 0 && 64 * (step + 1) == c0 && big_next_diag(T, s, step)) {
    double* A64 = AB;
    double* Ms = AB + 64 * LDA;
    double* Dl = Ms + 4 * 16 * LDM;
    const int kw = min(64, w - c0);
    __syncthreads();  // every wave's last MFMA operand read
    big_diag_prepare(A64, kw);
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int i = 16 * b + (lane & 15), j = 16 * a + (lane >> 4) + 4 * g;
            if (i < kw && j < kw && i >= j) A64[i + j * LDA] = acc[a][b][g];
          }
    }
    __syncthreads();
    big_diag_tail(T, s, step + 1, A64, Ms, Dl, arena, D, Mbuf + (int64_t)T.bigslot[s] * 4096, st, tol);
  }
}

// All big fronts of a level in ONE launch (r6): their 64-column panels' diagonal blocks, trsm tiles,
// local updates and trailing updates as tasks of a dependency-driven persistent kernel, instead of a
// k_big_diag / k_big_trsm / k_big_update / k_big_upd128 launch per panel step and kind (neos: ~400
// launches per factorisation, each boundary a ~4.6 us gap, and the panel chain diag -> trsm -> update
// serialised by them).  Per panel group G (kpan panels, columns [64 g0, gend)):
//   chain(G):  trsm tiles (kind 0) and local updates inside the group (kind 1, as k_big_update mode 0;
//              task (0, 0) factorises the next panel's diagonal block);
//   feed(G):   the trailing update of the next group's columns [gend, gend + 64 kpan), 64 x 64 tiles with
//              K = the group (kind 1, k_big_update's trailing mode; tile (0, 0) factorises the next
//              group's first diagonal block);
//   bulk(G):   the rest of the trailing matrix, 128 x 128 tiles (kind 2, k_big_upd128's engine, K unsplit).
// Tickets run chain(0) feed(0) chain(1) bulk(0) feed(1) chain(2) bulk(1) ... : the next group's panel
// chain only needs the feed tiles, so it runs while the previous group's bulk update occupies the chip.
// A task's dependencies (host-built, LDLSolver::build_schedules) are the last earlier writers of every
// 64 x 64 block of the front it reads or read-modify-writes: all earlier tickets (a workgroup waits only
// for tickets taken by running workgroups: no deadlock whatever the residency).  Every handed-off value
// is stored write-through (sc1) and drained before the task's flag, every load of one is sc1; each
// panel's M_K blocks go to a slot of their own (Mch, per front and panel).  Same operands and MFMA order
// as the per-step kernels with K unsplit (MADIPM_UPD_SPLIT=0): the same factor bit for bit.
// the task bodies as calls (one register allocation per body, not the union of four inlined ones)
__device__ __attribute__((noinline)) void dag_trsm(const FrontTab& T, int s, int step, int rt, double* arena,
                                                   const double* D, const double* M, double* sm) {
  trsm_body<true>(T, s, step, rt, arena, D, M, sm);
}
__device__ __attribute__((noinline)) void dag_update(const FrontTab& T, int s, int step, int kpan, int tij, double* arena,
                                                     double* D, double* Mnext, LDLStatus* st, double tol, double* sm) {
  update_body<true>(T, s, step, kpan, tij, arena, D, Mnext, st, tol, sm);
}
__device__ __attribute__((noinline)) void dag_diag(const FrontTab& T, int s, double* arena, double* D, double* M,
                                                   LDLStatus* st, double tol, double* sm) {
  diag_body<true>(T, s, 0, arena, D, M, st, tol, sm);
}
__device__ __attribute__((noinline)) void dag_bulk(const FrontTab& T, int s, int step, int kpan, int item, double* arena,
                                                   const double* D, double* sm) {
  const int f0 = T.first[s], w = T.first[s + 1] - f0, r = T.nrows[s];
  const int g0 = (step / kpan) * kpan, gend = min(64 * (g0 + kpan), w), cb = gend + 64 * kpan;
  const int I0 = cb + 128 * (item & 0xffff), J0 = cb + 128 * ((item >> 16) & 0x7fff);
  double* __restrict__ F = arena + T.l_off[s];
  const int tid = threadIdx.x, lane = tid & 63;
  dbl4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = dbl4{0.0, 0.0, 0.0, 0.0};
  upd128_gemm<true>(F, D, f0, r, I0, J0, 64 * g0, gend, sm, acc);
  const int wv = tid >> 6, wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    double fv[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = min(I0 + wm + 16 * b + (lane & 15), r - 1), j = min(J0 + wn + 16 * a + (lane >> 4) + 4 * g, r - 1);
        fv[b][g] = ldF<true>(F + i + (int64_t)j * r);
      }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = I0 + wm + 16 * b + (lane & 15), j = J0 + wn + 16 * a + (lane >> 4) + 4 * g;
        if (i < r && j <= i) stF<true>(F + i + (int64_t)j * r, fv[b][g] - acc[a][b][g]);
      }
  }
}

struct DagTask {
  int32_t s, step, item, kind;  // 0 trsm (item: row tile), 1 64-tile update (ti | tj << 16, bit 31: trailing),
                                // 2 128-tile trailing update (I | J << 16), 3 first diagonal block
};
constexpr int DAG_LDS = UPD_LDS > TRSM_LDS ? (UPD_LDS > U128_LDS ? UPD_LDS : U128_LDS) : (TRSM_LDS > U128_LDS ? TRSM_LDS : U128_LDS);
static_assert(DAG_LDS * 8 <= 80 * 1024 && DIAG_LDS <= DAG_LDS, "two k_big_dag workgroups per CU");
__global__ __launch_bounds__(NT, 2) void k_big_dag(FrontTab T, const DagTask* __restrict__ tasks, const int32_t* __restrict__ dptr,
                                                   const int32_t* __restrict__ dlist, int ntask, int32_t* flags, int epoch,
                                                   int32_t* counter, int kpan, double* __restrict__ arena,
                                                   double* __restrict__ D, double* __restrict__ Mch,
                                                   const int64_t* __restrict__ mslot, LDLStatus* st, double tol,
                                                   int32_t* err, int64_t* dbg) {
  // 80 KB: two workgroups per CU (the ticket word borrows the first double: read before any task uses it)
  __shared__ __attribute__((aligned(16))) double sm[DAG_LDS];
  int* s_t = reinterpret_cast<int*>(sm);
  const int tid = threadIdx.x, lane = tid & 63;
  for (;;) {
    __syncthreads();  // the previous task's LDS reads
    if (tid == 0) *s_t = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int t = *s_t;
    __syncthreads();  // every wave has the ticket before a task overwrites the word
    if (t >= ntask) break;
    const DagTask tk = tasks[t];
    if (dbg && tid == 0) dbg[4 * t] = wall_clock64();
    if (tid < 64) {  // wave 0 polls the dependencies' flags, 64 at a time
      const int q0 = dptr[t], q1 = dptr[t + 1];
      for (int q = q0; q < q1; q += 64) {
        const int d = q + lane < q1 ? dlist[q + lane] : -1;
        int spins = 0;
        for (;;) {
          const bool ok = d < 0 || __hip_atomic_load(flags + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch;
          if (__all(ok)) break;
          __builtin_amdgcn_s_sleep(1);
          ++spins;
          // bounded: a lost hand-off raises the sticky error, and once raised no later wait spins
          // (the launch drains in milliseconds, the factor is reported invalid)
          if (spins > (1 << 25) ||
              ((spins & 1023) == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
            if (lane == 0) atomicOr(err, kErrHandoff);
            break;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler ordering only (sc1 loads follow)
    }
    __syncthreads();
    if (dbg && tid == 0) dbg[4 * t + 1] = wall_clock64();
    double* Mp = Mch + mslot[tk.s] * BIG_MSZ;  // the front's per-panel M_K slots
    // the panel chain's tasks (latency-bound, on the critical path) issue ahead of a co-resident 128-tile
    // update's waves (MFMA-bound, off it)
    if (tk.kind == 2)
      __builtin_amdgcn_s_setprio(0);
    else
      __builtin_amdgcn_s_setprio(2);
    if (tk.kind == 0)
      dag_trsm(T, tk.s, tk.step, tk.item, arena, D, Mp + (int64_t)tk.step * BIG_MSZ, sm);
    else if (tk.kind == 1)
      dag_update(T, tk.s, tk.step, kpan, tk.item, arena, D, Mp + (int64_t)(tk.step + 1) * BIG_MSZ, st, tol, sm);
    else if (tk.kind == 3)
      dag_diag(T, tk.s, arena, D, Mp, st, tol, sm);
    else  // 128 x 128 trailing tile, columns past the feed tiles: rows / columns cb + 128 (I, J)
      dag_bulk(T, tk.s, tk.step, kpan, tk.item, arena, D, sm);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's sc1 stores drained
    __syncthreads();
    if (tid == 0) __hip_atomic_store(flags + t, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (dbg && tid == 0) {
      dbg[4 * t + 2] = wall_clock64();
      dbg[4 * t + 3] = blockIdx.x;
    }
  }
  if (tid == 0 && atomicAdd(counter + 1, 1) == (int)gridDim.x - 1) {  // last one out: reset the tickets
    counter[0] = 0;
    counter[1] = 0;
  }
}

// status of this shard's subtrees -> its slot (other slots 0), all-reduced with the top fronts
__global__ void k_pack_status(const LDLStatus* st, double* slots, int shard, int nshards) {
  const int q = threadIdx.x;
  if (q >= nshards) return;
  const bool me = q == shard;
  slots[4 * q + 0] = me ? (double)st->fail_pivot : 0.0;
  slots[4 * q + 1] = me ? (double)st->npos : 0.0;
  slots[4 * q + 2] = me ? (double)st->nneg : 0.0;
  slots[4 * q + 3] = me ? (double)st->nzero : 0.0;
}

// Top-front exchange buffer (sharded factorisation): only the lower triangles of the top fronts
// (plus the status slots) travel through the all-reduce — half the bytes of the full r x r blocks.
// One workgroup per top-front column: col[3 c] = arena offset of F(c, c), col[3 c + 1] = packed
// offset, col[3 c + 2] = length r - c.
__global__ __launch_bounds__(NT) void k_tri_pack(const int64_t* __restrict__ col, const double* __restrict__ arena,
                                                 double* __restrict__ xp, int dir) {
  const int64_t a = col[3 * blockIdx.x], p = col[3 * blockIdx.x + 1], n = col[3 * blockIdx.x + 2];
  for (int64_t i = threadIdx.x; i < n; i += NT) {
    if (dir == 0)
      xp[p + i] = arena[a + i];
    else
      const_cast<double*>(arena)[a + i] = xp[p + i];
  }
}

__global__ void k_unpack_status(LDLStatus* st, const double* slots, int nshards) {
  double f = (double)INT_MAX, p = 0, ng = 0, z = 0;
  for (int q = 0; q < nshards; ++q) {
    f = fmin(f, slots[4 * q]);
    p += slots[4 * q + 1];
    ng += slots[4 * q + 2];
    z += slots[4 * q + 3];
  }
  st->fail_pivot = (int)f;
  st->npos = (int)p;
  st->nneg = (int)ng;
  st->nzero = (int)z;
}

// static + dynamic LDS of a kernel must fit one CU (160 KB on gfx950)
void check_lds_fit(const void* f, size_t dyn, const char* nm) {
  int dev = 0, cu_lds = 0;
  MADIPM_HIP(hipGetDevice(&dev));
  MADIPM_HIP(hipDeviceGetAttribute(&cu_lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev));
  hipFuncAttributes fa{};
  MADIPM_HIP(hipFuncGetAttributes(&fa, f));
  MADIPM_REQUIRE(fa.sharedSizeBytes + dyn <= (size_t)cu_lds,
                 std::string(nm) + ": LDS " + std::to_string(fa.sharedSizeBytes) + " + " + std::to_string(dyn) +
                     " bytes exceeds the CU's " + std::to_string(cu_lds));
}

}  // namespace

void ldl_factor_kernel_attributes(bool first, size_t ftree_lds) {
  constexpr int asm_lds = 8 * kAsmLdsSrc, asm_upd_lds = 2 * 64 * AU_LDT * 8 + 8 * kAsmLdsSrc;
  if (first) {
    set_max_dyn_lds((const void*)k_small_blocked<false>, kSmall128Lds);
    set_max_dyn_lds((const void*)k_small_blocked<true>, kSmall192Lds);
    set_max_dyn_lds((const void*)k_fact_tree, (int)SymbolicPlan::kFactTreeLdsMax);
    set_max_dyn_lds((const void*)k_asm_update<int32_t>, asm_upd_lds);
    set_max_dyn_lds((const void*)k_asm_update<int64_t>, asm_upd_lds);
    set_max_dyn_lds((const void*)k_assemble<8, int32_t>, asm_lds);
    set_max_dyn_lds((const void*)k_assemble<8, int64_t>, asm_lds);
    set_max_dyn_lds((const void*)k_assemble<2, int32_t>, asm_lds);
    set_max_dyn_lds((const void*)k_assemble<2, int64_t>, asm_lds);
    check_lds_fit((const void*)k_assemble<2, int32_t>, asm_lds, "k_assemble");
    check_lds_fit((const void*)k_assemble<8, int64_t>, asm_lds, "k_assemble");
    check_lds_fit((const void*)k_asm_update<int32_t>, asm_upd_lds, "k_asm_update");
    check_lds_fit((const void*)k_asm_update<int64_t>, asm_upd_lds, "k_asm_update");
  }
  if (ftree_lds) check_lds_fit((const void*)k_fact_tree, ftree_lds, "k_fact_tree");  // this plan's carve
}

// F_P[gpos, gpos] -= W D^{-1} W^T, one launch per K-chunk of LB_KCHUNK members
void LDLSolver::lb_syrk(int g, hipStream_t s) {
  const auto& G = S_.lb[g];
  const int P = G.parent;
  double* F = S_.is_big[P] ? arena_.p + S_.l_off[P] : fscratch_.p + S_.fs_off[P];
  const int nt = (int)cdiv(G.m, SYT);
  const unsigned ntile = (unsigned)(nt * (nt + 1) / 2);
  const double* dinv = lbd_.p + S_.lb_mem.size() + G.mem_off;
  for (int k0 = 0; k0 < G.n; k0 += LB_KCHUNK)
    k_lb_syrk<<<ntile, NT, 0, s>>>(lbW_.p + G.w_off, dinv, G.m, k0, std::min(G.n, k0 + LB_KCHUNK),
                                   lbgpos_.p + G.gpos_off, F, S_.nrows[P]);
}

void LDLSolver::run_fact(const std::vector<Launch>& LL, const double* Kx, hipStream_t s, size_t b, size_t e,
                         LDLStatus* stamp) {
  if (b == 0) ++cepoch_;  // k_big_dag's flags: this factorisation's epoch (never 0)
  // the assembly's source indices, int32 when every arena / K index fits (the constructor uploads one
  // width): f(gsrc) with the pointer of that width
  auto with_gsrc = [&](auto&& f) { g_src32_.p ? f(g_src32_.p) : f(g_src_.p); };
  for (size_t li = b; li < std::min(e, LL.size()); ++li) {
    const Launch& L = LL[li];
    // the root tail (root_async_): the roots' assembly raises go, their factorisation waits for it
    int32_t* go = (root_async_ && &LL == &fact1_ && (li + 1 == side0_ || li == side0_)) ? rflag_.p : nullptr;
    const int32_t* list = sched_.p + L.off;
    switch (L.kind) {
      case ASSEMBLE: {
        // root_async_ with asm_side_: the roots' assembly (the launch before side0_) runs its chunk pass on
        // the caller's stream, each block raising a flag, and its tiles on side_, waiting for those flags
        const bool split = go && asm_side_ && li + 1 == side0_;
        const bool chunks = L.nchunk && !(split && side_phase_);
        const bool tiles = !(split && !side_phase_);
        int32_t* cfl = split ? rflag_.p + 2 + 64 : nullptr;
        const int ncw = split ? (int)cdiv(L.nchunk, NT) : 0;
        with_gsrc([&](const auto* gsrc) {
          using IDX = std::decay_t<decltype(*gsrc)>;
          if (chunks)
            TIMED(KK_ASM_CHUNKS, L.bytes2, 0.0, L.flops2,
                  (k_asm_chunks<IDX><<<(unsigned)cdiv(L.nchunk, NT), NT, 0, s>>>(
                      chunk_ids_, g_chunk_, gsrc, L.chunk0, L.nchunk, Kx, arena_, gpart_, cfl, repoch_)));
          if (tiles)
            TIMED(KK_ASSEMBLE, L.bytes, 0.0, L.flops,
                  (L.items < 256 ? k_assemble<8, IDX><<<(unsigned)L.items, ANT, 8 * kAsmLdsSrc, s>>>(
                                       T_, atiles_.p + L.off, g_ptr_, gpart_, brec_, arena_, fscratch_, gsrc, Kx, go, repoch_,
                                       cfl, ncw)
                                 : k_assemble<2, IDX><<<(unsigned)L.items, ANT, 8 * kAsmLdsSrc, s>>>(
                                       T_, atiles_.p + L.off, g_ptr_, gpart_, brec_, arena_, fscratch_, gsrc, Kx, go, repoch_,
                                       cfl, ncw)));
        });
        break;
      }
      case MICRO:
        TIMED(KK_TINY, L.bytes, L.alg, L.flops,
              (k_micro_factor<<<(unsigned)cdiv(L.items, NT / MG), NT, 0, s>>>(T_, list, (int)L.items, Kx, arena_, D_,
                                                                             st_, pivot_tol)));
        break;
      case SMALL32:
        TIMED(KK_TINY, L.bytes, L.alg, L.flops,
              (k_tiny_factor<<<(unsigned)cdiv(L.items, 4), NT, 0, s>>>(T_, list, (int)L.items, Kx, arena_, fscratch_, D_,
                                                                      st_, pivot_tol)));
        break;
      case SMALL64:
      case SMALL128:
        TIMED(KK_SMALL, L.bytes, L.alg, L.flops,
              (k_small_blocked<false><<<(unsigned)L.items, SBT, L.lds_bytes, s>>>(T_, list, Kx, arena_, fscratch_, D_,
                                                                                st_, pivot_tol, stamp, go, repoch_)));
        break;
      case SMALL192:
        TIMED(KK_SMALL, L.bytes, L.alg, L.flops,
              (k_small_blocked<true><<<(unsigned)L.items, SBT, L.lds_bytes, s>>>(T_, list, Kx, arena_, fscratch_, D_,
                                                                               st_, pivot_tol, stamp, go, repoch_)));
        break;
      case BIG_DIAG:
        TIMED(KK_DIAG, L.bytes, L.alg, L.flops,
              (k_big_diag<<<(unsigned)L.items, NT, 0, s>>>(T_, list, L.step, arena_, D_, minv_, st_, pivot_tol)));
        break;
      case BIG_TRSM:
        TIMED(KK_TRSM, L.bytes, L.alg, L.flops, (k_big_trsm<<<(unsigned)L.items, NT, 0, s>>>(T_, list, L.step, arena_, D_, minv_)));
        break;
      case BIG_UPDATE:
        TIMED(KK_UPDATE, L.bytes, L.alg, L.flops,
              (k_big_update<<<(unsigned)L.items, NT, 0, s>>>(T_, list, L.step, knobs_.big_kpan, arena_, D_, minv_, st_,
                                                              pivot_tol)));
        break;
      case ASM_UPDATE:  // nf = the launch's K rows (the widest panel, rounded up to 4)
        with_gsrc([&](const auto* gsrc) {
          using IDX = std::decay_t<decltype(*gsrc)>;
          TIMED(KK_ASM_UPDATE, L.bytes, 0.0, L.flops,
                (k_asm_update<IDX><<<(unsigned)L.items, ANT, 2 * L.nf * AU_LDT * 8 + 8 * kAsmLdsSrc, s>>>(
                    T_, atiles_.p + L.off, g_ptr_, gpart_, brec_, arena_, D_, L.nf, gsrc, Kx)));
        });
        break;
      case BIG_DAG:  // off = the launch's first task (global index), items = its tasks
        TIMED(KK_BIG_DAG, L.bytes, L.alg, L.flops,
              (k_big_dag<<<(unsigned)std::min<int64_t>(L.items, dag_grid_), NT, 0, s>>>(
                  T_, reinterpret_cast<const DagTask*>(dag_tasks_.p) + L.off, dag_dptr_.p + L.off, dag_dlist_.p,
                  (int)L.items, dag_flags_.p + L.off, cepoch_, dag_cnt_.p, knobs_.big_kpan, arena_, D_, dag_m_, dag_mslot_,
                  st_, pivot_tol, &st_->err, dag_dbg_.p ? dag_dbg_.p + 4 * L.off : nullptr)));
        if (dag_dbg_.p) dag_debug_dump(s, L);
        break;
      case BIG_UPDATE128:
        TIMED(KK_UPDATE, L.bytes, L.alg, L.flops,
              (k_big_upd128<<<(unsigned)(L.items * std::max(1, L.nf)), NT, 0, s>>>(
                  T_, list, L.step, knobs_.big_kpan, arena_, D_, minv_, st_, pivot_tol, std::max(1, L.nf), upsum_, uptick_)));
        break;
      case LB_BUILD:
        TIMED(KK_LB_BUILD, L.bytes, L.alg, 0.0,
              (k_lb_build<<<(unsigned)L.items, NT, 0, s>>>(lbg_, lbgid_, lbmem_, lbcs_, lbce_, lbwbase_, lbwrow_, Kx, lbW_,
                                                          lbd_.p, lbd_.p + S_.lb_mem.size(), D_, st_, pivot_tol)));
        break;
      case LB_SYRK:
        TIMED(KK_LB_SYRK, L.bytes, 0.0, L.flops, lb_syrk((int)L.off, s));
        break;
      case FTREE:
        ++fepoch_;
        TIMED(KK_FACT_TREE, L.bytes, L.alg, L.flops,
              (k_fact_tree<<<(unsigned)(nftree_ + nfhelp_), FTN, L.lds_bytes, s>>>(
                  T_, ft_order_, nftree_ + nfhelp_, nfhelp_, ft_dptr_, ft_dep_, fcnt_, fflags_, fepoch_, Kx, arena_,
                  fscratch_, D_, st_, pivot_tol, &st_->err, fdbg_.p)));
        if (fdbg_.p)  // (the helper tickets stamp nothing: the fronts' records follow them)
          tree_debug_dump(s, "fact", fdbg_.p + 24 * nfhelp_, nftree_, "stage", "wait", "push", "factor", "store", 24);
        break;
    }
  }
}

// Phase 1: this shard's subtrees (unsharded: the whole factorisation) + the top fronts' external
// assembly and the shard's status slot.
void LDLSolver::fact_phase1(const double* Kx, hipStream_t s) {
  if (S_.N == 0) return;
  join(s);  // the previous factorisation's root tail writes the same arena
  if (!(ext_reset && ext_status_ && !sharded())) k_status_init<<<1, 1, 0, s>>>(st_);
  const bool lazy = !sharded() && lazy_inertia && !spd && ext_status_;
  if (root_async_) {
    // the tree launch and the roots' assembly on s, the roots' factorisation on side_, where it waits
    // on the device for the assembly's go flag (no cross-stream event: its ~17 us of latency, r6_w).
    // s goes on to the caller's next kernels (the solve's right-hand side, forward leaves and tree
    // fronts), which read nothing the tail writes; k_root_solve waits for the tail's done flags.
    // Lazy inertia: the root kernel stamps t1.
    ++repoch_;
    run_fact(fact1_, Kx, s, 0, side0_);
    // not event-timed: the launch waits on the device from its enqueue (during the previous solve)
    // until the go flag, and events would count that wait as the kernel's time
    untimed_ = side_phase_ = true;
    run_fact(fact1_, Kx, side_, asm_side_ ? side0_ - 1 : side0_, fact1_.size(), lazy ? st_ : nullptr);
    untimed_ = side_phase_ = false;
    MADIPM_HIP(hipEventRecord(ev_join_, side_));
    root_pending_ = true;
    if (!lazy) join(s);  // k_inertia and the status copy below need the whole factor
  } else {
    run_fact(fact1_, Kx, s);
  }
  const int nb = (int)std::min<int64_t>(64, cdiv(S_.N, NT));
  const int spdf = spd ? 1 : 0;
  if (!sharded()) {
    if (lazy) {  // the driver's next kernel (root_async_: the root kernel) stamps t1
      inertia_stale_ = true;
      return;
    }
    TIMED(KK_INERTIA, 8.0 * S_.N, 0.0, 0.0, (k_inertia<<<nb, NT, 0, s>>>(D_, S_.N, st_, spdf, nullptr, 0)));
    MADIPM_HIP(hipGetLastError());
    if (!ext_status_) MADIPM_HIP(hipMemcpyAsync(h_st_, st_, sizeof(LDLStatus), hipMemcpyDeviceToHost, s));
    return;
  }
  TIMED(KK_INERTIA, 8.0 * S_.N, 0.0, 0.0, (k_inertia<<<nb, NT, 0, s>>>(D_, S_.N, st_, spdf, colmask_, 1)));
  k_pack_status<<<1, 64, 0, s>>>(st_, arena_.p + S_.top_hi, S_.shard, S_.nshards);
  if (ntopcol_) k_tri_pack<<<(unsigned)ntopcol_, NT, 0, s>>>(topcol_, arena_, xpack_, 0);
  MADIPM_HIP(hipMemcpyAsync(xpack_.p + xpack_tri_, arena_.p + S_.top_hi, sizeof(double) * 4 * S_.nshards,
                            hipMemcpyDeviceToDevice, s));
  MADIPM_HIP(hipGetLastError());
}

// Phase 2 (sharded): after the all-reduce of fact_xbuf(), every shard factorises the top fronts.
void LDLSolver::fact_phase2(hipStream_t s) {
  if (S_.N == 0 || !sharded()) return;
  if (ntopcol_) k_tri_pack<<<(unsigned)ntopcol_, NT, 0, s>>>(topcol_, arena_, xpack_, 1);
  MADIPM_HIP(hipMemcpyAsync(arena_.p + S_.top_hi, xpack_.p + xpack_tri_, sizeof(double) * 4 * S_.nshards,
                            hipMemcpyDeviceToDevice, s));
  k_unpack_status<<<1, 1, 0, s>>>(st_, arena_.p + S_.top_hi, S_.nshards);
  run_fact(fact2_, nullptr, s);
  const int nb = (int)std::min<int64_t>(64, cdiv(S_.N, NT));
  TIMED(KK_INERTIA, 8.0 * S_.N, 0.0, 0.0, (k_inertia<<<nb, NT, 0, s>>>(D_, S_.N, st_, spd ? 1 : 0, colmask_, 2)));
  MADIPM_HIP(hipGetLastError());
  MADIPM_HIP(hipMemcpyAsync(h_st_, st_, sizeof(LDLStatus), hipMemcpyDeviceToHost, s));
}

void LDLSolver::factorize_async(const double* Kx, hipStream_t s) {
  fact_phase1(Kx, s);
  if (!sharded() || S_.N == 0) return;
  MADIPM_REQUIRE(comm_ != nullptr, "sharded LDL^T without a communicator");
  comm_->allreduce_sum(fact_xbuf(), fact_xlen(), s);
  fact_phase2(s);
}

bool LDLSolver::external_status(LDLStatus* dev, LDLStatus* host) {
  if (sharded() || !dev || !host) return false;
  st_ = dev;
  h_st_ = host;
  T_.err = &st_->err;
  ext_status_ = true;
  k_status_init<<<1, 1, 0, nullptr>>>(st_, 1);
  MADIPM_HIP(hipDeviceSynchronize());
  return true;
}

// lazy_inertia: count the current factor's inertia now (inertia() of a driver that skips k_inertia)
void LDLSolver::count_inertia(hipStream_t s) {
  if (!inertia_stale_ || S_.N == 0) return;
  inertia_stale_ = false;
  join(s);
  const int nb = (int)std::min<int64_t>(64, cdiv(S_.N, NT));
  k_zero_counts<<<1, 1, 0, s>>>(st_);
  k_inertia<<<nb, NT, 0, s>>>(D_, S_.N, st_, 0, nullptr, 1);
  MADIPM_HIP(hipGetLastError());
  status(s, true);
}

int LDLSolver::status(hipStream_t s, bool sync) {
  if (S_.N == 0) {
    factorized = true;
    return 0;
  }
  if (sync) join(s);
  if (sync && ext_status_) MADIPM_HIP(hipMemcpyAsync(h_st_, st_, sizeof(LDLStatus), hipMemcpyDeviceToHost, s));
  if (sync) MADIPM_HIP(hipStreamSynchronize(s));
  if (h_st_->err) {  // a lost hand-off or a carve overflow gives a wrong factor or solve: never success
    const int e = h_st_->err;
    h_st_->err = 0;
    k_status_init<<<1, 1, 0, s>>>(st_, 1);
    MADIPM_HIP(hipStreamSynchronize(s));
    if (e & kErrAsmSrc)
      throw Error("LDL^T: an assembly tile's source count exceeded the LDS source path's windows (factor is invalid)", -5);
    if (e & kErrLdsCarve)
      throw Error("LDL^T: a front or folded-leaf batch exceeded k_fact_tree's LDS carve (factor is invalid)", -5);
    throw Error("LDL^T: a dependency hand-off between fronts timed out (factor or solve is invalid)", -5);
  }
  npos = h_st_->npos;
  nneg = h_st_->nneg;
  nzero = h_st_->nzero;
  const int fp = h_st_->fail_pivot;
  factorized = (fp == INT_MAX);
  return factorized ? 0 : fp;
}

// MADIPM_DAG_DEBUG=1: per kind of k_big_dag task (trsm, 64-tile update, 128-tile update, diagonal
// block) the tasks, their mean wait for dependencies and mean run time, and the launch's span and the
// workgroup-time it kept busy / waiting (first few launches; 100 MHz clock)
void LDLSolver::dag_debug_dump(hipStream_t s, const Launch& L) {
  static int calls = 0;
  if (++calls > 12) return;
  MADIPM_HIP(hipStreamSynchronize(s));
  std::vector<int64_t> h((size_t)4 * L.items);
  MADIPM_HIP(hipMemcpy(h.data(), dag_dbg_.p + 4 * L.off, h.size() * 8, hipMemcpyDeviceToHost));
  double n[5] = {0, 0, 0, 0, 0}, wt[5] = {0, 0, 0, 0, 0}, rt[5] = {0, 0, 0, 0, 0};
  int64_t t0 = INT64_MAX, t1 = 0;
  for (int64_t t = 0; t < L.items; ++t) {
    const int k = dag_kind_[4 * (L.off + t) + 3];
    n[k] += 1;
    wt[k] += (double)(h[4 * t + 1] - h[4 * t]);
    rt[k] += (double)(h[4 * t + 2] - h[4 * t + 1]);
    t0 = std::min(t0, h[4 * t]);
    t1 = std::max(t1, h[4 * t + 2]);
  }
  const char* nm[5] = {"trsm", "upd64", "upd128", "diag", "step"};
  fprintf(stderr, "dag launch: %lld tasks, span %.1f us, wait %.1f / run %.1f WG-ms\n", (long long)L.items, (t1 - t0) / 100.0,
          (wt[0] + wt[1] + wt[2] + wt[3] + wt[4]) / 1e5, (rt[0] + rt[1] + rt[2] + rt[3] + rt[4]) / 1e5);
  for (int k = 0; k < 5; ++k)
    if (n[k] > 0)
      fprintf(stderr, "  %-7s %6.0f tasks  wait %7.2f us  run %7.2f us (mean)\n", nm[k], n[k], wt[k] / n[k] / 100.0, rt[k] / n[k] / 100.0);
}

}  // namespace madipm
