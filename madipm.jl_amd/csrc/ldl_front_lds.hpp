// Private to ldl.hip: the blocked LDL^T of a front held in LDS (k_small_blocked, k_fact_tree and,
// through factor16r, the big fronts' diagonal blocks), with the wave helpers of the factorisation
// kernels.  Device functions only, all inlined; no kernel lives here.
#pragma once
#include "ldl_device.hpp"

namespace madipm {
namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

// Pin loaded values (an empty asm that "modifies" them) so the compiler keeps clamped loads
// unconditional instead of sinking them into the branch of their conditional use.  The asm needs the
// value, so it waits for the load: pin a batch only after ALL its loads are issued (pinning each load
// right after it serialised the LDS loads of the MFMA loops on the LDS latency).
#define LDL_PIN(x) asm volatile("" : "+v"(x))
#define LDL_PIN4(a) asm volatile("" : "+v"((a)[0]), "+v"((a)[1]), "+v"((a)[2]), "+v"((a)[3]))

__device__ __forceinline__ bool bad_pivot(double d, double tol) { return !(fabs(d) > tol) || isinf(d); }

// wave-synchronous LDS hand-off: LDS ops of one wave complete in order; keep the compiler from
// moving them across this point
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

constexpr int LDM = 17;  // ld of a 16 x 16 M_K block

// ------------------------------------------------------------------ small fronts, blocked (r <= 128)
// The front lives in LDS (ld = r | 1).  Pivots are taken 16 at a time: one wave factors the 16 x 16
// diagonal block (wave-synchronous, no barriers; identity-padded when fewer than 16 pivots remain),
// the rows below get L = A M_K on f64 MFMA, and the trailing lower triangle is updated tile by tile
// (16 x 16 tiles, C -= (L_I D) L_J^T, f64 MFMA 16x16x4) — 3 barriers per 16 pivots instead of one per
// pivot.  Row/column blocks of a step start right after its last pivot (not 16-aligned), exactly
// like the big-front path.
// Factor the kw (<= 16) pivots at (k0, k0) of A (ld) with ONE wave: strictly-lower L_KK into A,
// pivots into Dl[k0 + t], M_K = L_KK^{-T} D^{-1} (16 x 16, ld LDM, identity-padded) into MK.
template <bool PK>
__device__ __forceinline__ int fidx(int i, int j, int r, int ld) {
  return PK ? ((j * (2 * r - j - 1)) >> 1) + i : i + j * ld;
}

// PK = false: square storage, ld = r | 1 (r <= 128); PK = true: packed lower-triangular columns
// (r <= 192 fits LDS), element (i, j >= ...) at j (2r - j - 1) / 2 + i

// Factor the 16 x 16 diagonal block K at (k0, k0) of the front in LDS with ONE wave (identity-padded
// past kw): writes the strictly-lower unit L_KK into A, d into Dl[k0 + i] and M_K = L_KK^{-T} D^{-1}
// (ld LDM, zero above the diagonal) into MK — register-resident, no LDS hand-off per step (the LDS
// hand-off variant took ~3.8 us per block against ~2.6 us for this one, r3).
// Lane (i = lane & 15, g = lane >> 4) holds A(i, j) and X(i, j) for the four columns j = 4m + g in
// a[m], x[m]: column t lives in register t >> 2 of row group t & 3.  Step t:
//   d_t = A(t, t): v_readlane (wave-uniform);
//   A(i, t) to every row group: v_permlane16_swap + v_permlane32_swap (gfx950) of row group t & 3;
//   A(t, j), X(t, j) of the lane's columns: DPP row_newbcast:t inside the lane's 16-lane row.
// Every row i > t is updated with the mirrored row t (A(t, j), j > t).
template <int G>
__device__ __forceinline__ int xrow_bcast32(int v) {  // row G (16 lanes) of the wave, to every row
  const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // [r0 r0 r2 r2] | [r1 r1 r3 r3]
  const int y = (G & 1) ? (int)p[1] : (int)p[0];
  const auto q = __builtin_amdgcn_permlane32_swap(y, y, false, false);  // [rA rA rA rA] | [rB rB rB rB]
  return (G & 2) ? (int)q[1] : (int)q[0];
}
template <int G>
__device__ __forceinline__ double xrow_bcast(double v) {
  return __hiloint2double(xrow_bcast32<G>(__double2hiint(v)), xrow_bcast32<G>(__double2loint(v)));
}
// acc += acc[lane T of the lane's 16-lane row] * mul: ONE v_fmac_f64 with a DPP row_newbcast source
// (64-bit DPP, gfx90a+).  The s_nop covers the VALU-write -> DPP-read hazard (2 wait states) that the
// compiler does not track through inline asm.
template <int T>
__device__ __forceinline__ void fmac_row_bcast(double& acc, double mul) {
  asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf"
               : "+v"(acc)
               : "v"(mul), "n"(T));
}
// RCP: l = A(i, t) * (1 / d_t) with the reciprocal from v_rcp_f64 + two Newton steps
// (within an ulp of the IEEE quotient; ~6 dependent instructions on the pivot chain instead of the
// ~10 of the IEEE division sequence)
__device__ __forceinline__ double recip_nr(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  return fma(fma(-d, r, 1.0), r, r);
}
template <int T, bool RCP>
__device__ __forceinline__ void f16r_step(double (&a)[4], double (&x)[4], double& dmine, int i, int g) {
  constexpr int gt = T & 3, mt = T >> 2;
  const double dt = readlane_f64(a[mt], T + 16 * gt);
  const double ci = xrow_bcast<gt>(a[mt]);
  const double li = (i > T) ? (RCP ? ci * recip_nr(dt) : ci / dt) : 0.0;  // IEEE quotient unless RCP
  // A(i, j) -= l_i A(t, j) for j > t; X(i, j) -= l_i X(t, j) for j <= t (a zero multiplier elsewhere:
  // exact, the products are finite); the column ranges are static except for one register.  The
  // register holding the next pivot column goes first and the X updates (off the pivot chain) last:
  // the waves issue in order, so the next step's readlane then finds its operand ready (the same
  // operations as before, in another order: bitwise the same factor)
  constexpr int mn = (T + 1 < 16) ? ((T + 1) >> 2) : -1;
  if constexpr (mn >= 0) fmac_row_bcast<T>(a[mn], (4 * mn + g > T) ? -li : 0.0);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = 4 * m + g;
    if (m != mn && 4 * m + 3 > T) fmac_row_bcast<T>(a[m], (j > T) ? -li : 0.0);
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = 4 * m + g;
    if (4 * m <= T) fmac_row_bcast<T>(x[m], (j <= T) ? -li : 0.0);
  }
  if (i == T) dmine = dt;
  if (g == gt && i > T) a[mt] = li;
}
template <int T, bool RCP>
__device__ __forceinline__ void f16r_steps(double (&a)[4], double (&x)[4], double& dmine, int i, int g) {
  if constexpr (T < 16) {
    f16r_step<T, RCP>(a, x, dmine, i, g);
    f16r_steps<T + 1, RCP>(a, x, dmine, i, g);
  }
}
template <bool PK, bool RCP>
__device__ __forceinline__ void factor16r(double* A, int r, int ld, int k0, int kw, double* Dl, double* MK, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int ic = min(i, kw - 1);
  double a[4], x[4], v[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = 4 * m + g, jc = min(j, kw - 1);
    v[m] = A[fidx<PK>(k0 + max(ic, jc), k0 + min(ic, jc), r, ld)];  // mirrored: the full symmetric block
  }
  LDL_PIN4(v);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = 4 * m + g;
    a[m] = (i < kw && j < kw) ? v[m] : (i == j ? 1.0 : 0.0);
    x[m] = (i == j) ? 1.0 : 0.0;
  }
  double dmine = 1.0;
  f16r_steps<0, RCP>(a, x, dmine, i, g);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = 4 * m + g;
    if (j < i && i < kw) A[fidx<PK>(k0 + i, k0 + j, r, ld)] = a[m];
    MK[j * LDM + i] = (j <= i) ? x[m] / dmine : 0.0;
  }
  if (g == 0 && i < kw) Dl[k0 + i] = dmine;
  wave_sync();
}

// Blocked right-looking LDL^T of the w pivots of a front held in LDS (lower part; square ld r|1 or
// packed), all 256 threads; pivots in Dl.
//
// Codegen notes (measured on gfx950 with tools/factor_bench.hip, tools/tile_bench.hip): one f64
// MFMA 16x16x4 issues every 64 cycles per SIMD, an LDS round trip is ~80 cycles, and a wave has
// nothing to hide them behind (one 256-thread workgroup per CU).  So every LDS operand of a step is
// loaded unconditionally (clamped indices, pinned so the compiler cannot sink a load into a branch
// with its own wait), a wave updates a STRIP of up to four 16 x 16 tiles sharing the (L_I D)
// operand (four independent accumulator chains back to back), and the next pivot block is
// factorised by one wave while the other three finish the trailing update (lookahead).

// L_R = A[R, k0:k0+kw] M_K for the 16-row blocks b = b0, b0 + bstep, ... below the pivots
template <bool PK>
__device__ __forceinline__ void panel_blocks(double* A, int r, int ld, int k0, int kw, int R0, int nbr, const double* MK,
                                             int b0, int bstep, int lane) {
  const int kl = lane >> 4, il = lane & 15;
  double bv[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) bv[ks] = MK[(4 * ks + kl) * LDM + il];
  for (int b = b0; b < nbr; b += 2 * bstep) {
    const bool two = b + bstep < nbr;  // wave-uniform
    double av[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int row = min(R0 + 16 * (b + u * bstep) + il, r - 1);
        av[u][ks] = A[fidx<PK>(row, k0 + min(4 * ks + kl, kw - 1), r, ld)];
      }
    LDL_PIN4(av[0]);
    LDL_PIN4(av[1]);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) av[u][ks] = (4 * ks + kl < kw) ? av[u][ks] : 0.0;
    dbl4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0][ks], bv[ks], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1][ks], bv[ks], acc1, 0, 0, 0);  // unpredicated
    }
    // acc[g] = D[m][n]: m = kl + 4 g (row in the block: the A operand carried the rows), n = il (pivot)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row0 = R0 + 16 * b + kl + 4 * g, row1 = row0 + 16 * bstep;
      if (row0 < r && il < kw) A[fidx<PK>(row0, k0 + il, r, ld)] = acc0[g];
      if (two && row1 < r && il < kw) A[fidx<PK>(row1, k0 + il, r, ld)] = acc1[g];
    }
  }
}

// One strip: tiles (I, J0 .. J0+NS-1).  NS is static so the MFMA sequence has no branches (a
// predicated MFMA makes the compiler drain the accumulators after every step).
template <bool PK, int NS>
__device__ __forceinline__ void trail_strip(double* A, int r, int ld, int k0, int kw, int R0, int I, int J0,
                                            const double (&dk)[4], int lane, int jend) {
  const int kl = lane >> 4, il = lane & 15;
  const int i0 = R0 + 16 * I;
  const int ri = min(i0 + il, r - 1);
  double bv[4], av[NS][4], cv[NS][4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int kc = k0 + min(4 * ks + kl, kw - 1);
    bv[ks] = A[fidx<PK>(ri, kc, r, ld)];
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      const int rj = min(R0 + 16 * (J0 + t) + il, r - 1);
      av[t][ks] = A[fidx<PK>(rj, kc, r, ld)];
    }
  }
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = min(R0 + 16 * (J0 + t) + kl + 4 * g, r - 1);
      cv[t][g] = A[fidx<PK>(max(ri, j), min(ri, j), r, ld)];
    }
  // pins in issue order, after every load (the MFMA operands first: their waits come first)
  LDL_PIN4(bv);
#pragma unroll
  for (int t = 0; t < NS; ++t) LDL_PIN4(av[t]);
#pragma unroll
  for (int t = 0; t < NS; ++t) LDL_PIN4(cv[t]);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) bv[ks] *= dk[ks];  // dk = 0 past kw
  dbl4 acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int t = 0; t < NS; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t][ks], bv[ks], acc[t], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = R0 + 16 * (J0 + t) + kl + 4 * g, i = i0 + il;
      if (i < r && j < jend && i >= j) A[fidx<PK>(i, j, r, ld)] = cv[t][g] - acc[t][g];
    }
}

// C_IJ -= L_J (L_I D)^T over the 16 x 16 tiles (I, J) of the trailing lower triangle with
// jlo <= J <= min(I, jhi), I < nbr; strips (I, J0 .. J0+3) dealt to waves w0, w0 + wstep, ...
template <bool PK>
__device__ __forceinline__ void trail_strips(double* A, int r, int ld, int k0, int kw, int R0, int nbr, int jlo, int jhi,
                                             const double (&dk)[4], int w0, int wstep, int lane, int jend, int i0 = 0) {
  if (jlo > jhi) return;
  int I = max(jlo, i0), J0 = jlo;  // rows I >= i0 only
  auto adv = [&]() {
    J0 += 4;
    if (J0 > min(I, jhi)) {
      ++I;
      J0 = jlo;
    }
  };
  for (int s = 0; s < w0; ++s) adv();
  while (I < nbr) {
    switch (min(4, min(I, jhi) - J0 + 1)) {  // tiles in this strip (wave-uniform)
      case 1: trail_strip<PK, 1>(A, r, ld, k0, kw, R0, I, J0, dk, lane, jend); break;
      case 2: trail_strip<PK, 2>(A, r, ld, k0, kw, R0, I, J0, dk, lane, jend); break;
      case 3: trail_strip<PK, 3>(A, r, ld, k0, kw, R0, I, J0, dk, lane, jend); break;
      default: trail_strip<PK, 4>(A, r, ld, k0, kw, R0, I, J0, dk, lane, jend); break;
    }
    for (int s = 0; s < wstep; ++s) adv();
  }
}

// Deferred Schur complement: U -= L_U D L_U^T over all w pivots in one pass (tiles of the lower
// triangle of A[w:, w:]).  K runs over the pivots in 16-column chunks with the accumulators held in
// registers, so each C tile is loaded and stored once (the per-block right-looking update touches it
// w/16 times); the next chunk's operands are loaded before the current chunk's MFMAs.
template <bool PK, int NS>
__device__ __forceinline__ void schur_strip(double* A, int r, int ld, int w, const double* Dl, int I, int J0, int lane) {
  const int kl = lane >> 4, il = lane & 15;
  const int i0 = w + 16 * I;
  const int ri = min(i0 + il, r - 1);
  int rj[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) rj[t] = min(w + 16 * (J0 + t) + il, r - 1);
  dbl4 acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = dbl4{0.0, 0.0, 0.0, 0.0};
  // raw operands of the next 16-pivot chunk: issued one chunk ahead, pinned (waited for) only at the
  // top of the iteration that consumes them, i.e. after the previous chunk's MFMAs
  double bn[4], an[NS][4];
  auto load = [&](int k0) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int kc = min(k0 + 4 * ks + kl, w - 1);
      bn[ks] = A[fidx<PK>(ri, kc, r, ld)];
#pragma unroll
      for (int t = 0; t < NS; ++t) an[t][ks] = A[fidx<PK>(rj[t], kc, r, ld)];
    }
  };
  load(0);
  for (int k0 = 0; k0 < w; k0 += 16) {
    LDL_PIN4(bn);
#pragma unroll
    for (int t = 0; t < NS; ++t) LDL_PIN4(an[t]);
    double b2[4], a2[NS][4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k = k0 + 4 * ks + kl;
      b2[ks] = (k < w) ? bn[ks] * Dl[min(k, w - 1)] : 0.0;  // pivots: LDS, read at the point of use
#pragma unroll
      for (int t = 0; t < NS; ++t) a2[t][ks] = an[t][ks];
    }
    if (k0 + 16 < w) load(k0 + 16);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int t = 0; t < NS; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[t][ks], b2[ks], acc[t], 0, 0, 0);
  }
  double cv[NS][4];
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = min(w + 16 * (J0 + t) + kl + 4 * g, r - 1);
      cv[t][g] = A[fidx<PK>(max(ri, j), min(ri, j), r, ld)];
    }
#pragma unroll
  for (int t = 0; t < NS; ++t) LDL_PIN4(cv[t]);
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = w + 16 * (J0 + t) + kl + 4 * g, i = i0 + il;
      if (i < r && j < r && i >= j) A[fidx<PK>(i, j, r, ld)] = cv[t][g] - acc[t][g];
    }
}

template <bool PK>
__device__ __forceinline__ void schur_strips(double* A, int r, int ld, int w, const double* Dl, int wv, int nw, int lane) {
  const int nbu = (r - w + 15) >> 4;
  int I = 0, J0 = 0;
  auto adv = [&]() {
    J0 += 4;
    if (J0 > I) {
      ++I;
      J0 = 0;
    }
  };
  for (int q = 0; q < wv; ++q) adv();
  while (I < nbu) {
    switch (min(4, I - J0 + 1)) {
      case 1: schur_strip<PK, 1>(A, r, ld, w, Dl, I, J0, lane); break;
      case 2: schur_strip<PK, 2>(A, r, ld, w, Dl, I, J0, lane); break;
      case 3: schur_strip<PK, 3>(A, r, ld, w, Dl, I, J0, lane); break;
      default: schur_strip<PK, 4>(A, r, ld, w, Dl, I, J0, lane); break;
    }
    for (int q = 0; q < nw; ++q) adv();
  }
}

// defer: the right-looking block steps update only the pivot columns (columns < w); the update
// block U gets its whole Schur complement afterwards in one pass (schur_strips)
// pt (diagnostics, MADIPM_TREE_DEBUG): thread 0 accumulates the phase times (first pivot block,
// panels, J = 0 strips, lookahead sections, Schur pass) into pt[0..4]
template <bool PK>
__device__ __forceinline__ void blocked_factor_lds(double* A, int r, int w, int ld, double* Dl, double* MK, double* cbuf,
                                                   int defer = 0, int64_t* pt = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  const int nblk = (w + 15) >> 4;
  defer = defer && w < r;
  const int jend = defer ? w : r;
  int64_t tp[5] = {0, 0, 0, 0, 0}, tl = (pt && tid == 0) ? wall_clock64() : 0;
  auto stamp = [&](int k) {
    if (pt && tid == 0) {
      const int64_t now = wall_clock64();
      tp[k] += now - tl;
      tl = now;
    }
  };
  const int64_t cyc0 = (pt && tid == 0) ? (int64_t)clock64() : 0;
  if (wv == 0) factor16r<PK, true>(A, r, ld, 0, min(16, w), Dl, MK, lane);
  __syncthreads();
  stamp(0);
  const int64_t cyc1 = (pt && tid == 0) ? (int64_t)clock64() : 0;
  for (int kb = 0; kb < nblk; ++kb) {
    const int k0 = 16 * kb, kw = min(16, w - k0);
    const int R0 = k0 + kw;                       // first row / column after the pivots
    const int nbr = (r - R0 + 15) >> 4;           // 16-row blocks below
    const int jhi = defer ? ((w - R0 + 15) >> 4) - 1 : nbr;  // last column block updated
    panel_blocks<PK>(A, r, ld, k0, kw, R0, nbr, MK, wv, nw, lane);
    __syncthreads();
    stamp(1);
    double dk[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k = 4 * ks + (lane >> 4);
      dk[ks] = (k < kw) ? Dl[k0 + min(k, kw - 1)] : 0.0;
    }
    if (kb + 1 < nblk) {
      // the next pivot block's columns (J = 0: its diagonal block and panel rows) first ...
      trail_strips<PK>(A, r, ld, k0, kw, R0, nbr, 0, 0, dk, wv, nw, lane, jend);
      __syncthreads();
      stamp(2);
      // ... then one wave factorises it while the others update the rest (J >= 1)
      const int fw = (kb + 1) % nw;
      if (wv == fw)
        factor16r<PK, true>(A, r, ld, R0, min(16, w - R0), Dl, MK, lane);
      else
        trail_strips<PK>(A, r, ld, k0, kw, R0, nbr, 1, jhi, dk, (wv - fw + nw - 1) % nw, nw - 1, lane, jend);
    } else if (!defer) {
      trail_strips<PK>(A, r, ld, k0, kw, R0, nbr, 0, nbr, dk, wv, nw, lane, jend);
    }
    __syncthreads();
    stamp(3);
  }
  if (defer) {
    schur_strips<PK>(A, r, ld, w, Dl, wv, nw, lane);
    __syncthreads();
    stamp(4);
  }
  if (pt && tid == 0) {
    for (int k = 0; k < 5; ++k) pt[k] = tp[k];
    pt[5] = cyc1 - cyc0;  // shader clocks of the first pivot block (vs pt[0] in 100 MHz ticks)
  }
}

// ---- Pipelined schedule of the same factorisation (MADIPM_FACT_PIPE=1, default; needs factor16r).
// In blocked_factor_lds every pivot block costs panel + column-0 strips + max(next diagonal factor,
// trailing update), three workgroup barriers apart, and the diagonal factor (~2.6 us of division and
// lane-swap latency) dominates.  Here wave 0 runs the pivot chain alone: once block k is factorised it
// forms the panel tile of row block 0 below it (the next pivot rows), updates the next diagonal tile
// with it and factorises that tile at once — while waves 1.. form the rest of block k's panel and its
// trailing update.  Hand-offs are LDS counters (workgroup-scope release / acquire), not barriers, so
// the chain never waits for the trailing update of its own step:
//   mk     = k + 1  wave 0: block k's M_K (buffer k & 1), pivots and L_kk are in LDS
//   pt     = k + 1  wave 0: panel tile 0 of step k is in LDS
//   j0    += 1      each other wave, after its priority tiles of step k: column block 0 (tiles (I, 0),
//                   I >= 1) and the diagonal tile (1, 1) — everything wave 0 reads at step k + 1
//   ob    += 1      barrier among the other waves (panel rows complete before the trailing update)
// Tile (0, 0) of a non-final step is wave 0's alone.  Every tile and panel block is formed by the
// same MFMA sequence from the same operands as in blocked_factor_lds: the two schedules agree
// bitwise (test_ldl_fact_pipe_bitwise).  A wait that spins for ~2^20 polls sets `abort` (a schedule
// bug must not hang the GPU: the factor is then garbage and the tests fail).
struct PipeCtr {
  int mk, pt, j0, ob, abort;
  int64_t ow;  // diagnostics: wave 1's wait ticks
};
__device__ __forceinline__ PipeCtr& pipe_ctr() {
  __shared__ PipeCtr c;
  return c;
}
__device__ __forceinline__ void pipe_wait(int* f, int v, int* abort) {
  int spins = 0;
  while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < v) {
    if (__hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
    __builtin_amdgcn_s_sleep(1);
    if (++spins > (1 << 20)) {
      __hip_atomic_store(abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return;
    }
  }
}
// one lane per wave, after the wave's LDS writes (the release orders them before the counter)
__device__ __forceinline__ void pipe_set(int* f, int v) {
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(f, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void pipe_add(int* f) {
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(f, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool PK>
__device__ __forceinline__ void blocked_factor_pipe(double* A, int r, int w, int ld, double* Dl, double* MK0,
                                                    double* MK1, int defer, int64_t* pt, int32_t* err, int fault) {
  constexpr bool RCP = true;
  double* const MKall = nullptr;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  const int no = nw - 1;  // waves 1 .. nw - 1: panel rest + trailing update
  const int nblk = (w + 15) >> 4;
  // defer 2: the caller forms the update block's Schur complement itself (the medium fronts' panels,
  // whose trailing matrix lives in HBM): rows below the pivots get their L only
  const bool schur = defer == 1;
  defer = defer && w < r;
  const int jend = defer ? w : r;
  PipeCtr& pc = pipe_ctr();
  int64_t t0 = (pt && tid == 0) ? wall_clock64() : 0;
  if (tid == 0) pc = PipeCtr{0, 0, 0, 0, 0, 0};
  // diagnostics (pt): wave 0's wait / diagonal-factor ticks, wave 1's wait ticks
  const bool dbg = pt && (tid == 0 || tid == 64);
  int64_t tw = 0, tf = 0, tc = 0;
  auto lap = [&](int64_t& acc) {
    if (dbg) {
      const int64_t now = wall_clock64();
      acc += now - tc;
      tc = now;
    }
  };
  if (wv == 0) factor16r<PK, RCP>(A, r, ld, 0, min(16, w), Dl, MKall ? MKall : MK0, lane);
  __syncthreads();  // block 0 factorised; the counters are zero
  const int64_t t1 = (pt && tid == 0) ? wall_clock64() : 0;
  int gen = 0;  // O-barrier generation (waves 1..)
  for (int kb = 0; kb < nblk; ++kb) {
    const int k0 = 16 * kb, kw = min(16, w - k0);
    const int R0 = k0 + kw;
    const int nbr = (r - R0 + 15) >> 4;
    const int jhi = defer ? ((w - R0 + 15) >> 4) - 1 : nbr;
    const bool last = kb + 1 == nblk;
    const double* MKc = MKall ? MKall + kb * 16 * LDM : ((kb & 1) ? MK1 : MK0);
    double dk[4];
    int64_t tx = 0;
    if (dbg) tc = wall_clock64();
    if (wv == 0) {
      // the pivot chain: step kb - 1's priority tiles (this step's raw panel tile 0 and diagonal tile)
      if (kb > 0) pipe_wait(&pc.j0, no * kb, &pc.abort);
      lap(tw);
      if (nbr > 0) panel_blocks<PK>(A, r, ld, k0, kw, R0, 1, MKc, 0, 1, lane);
      pipe_set(&pc.pt, kb + 1);
      if (!last) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int k = 4 * ks + (lane >> 4);
          dk[ks] = (k < kw) ? Dl[k0 + min(k, kw - 1)] : 0.0;
        }
        trail_strip<PK, 1>(A, r, ld, k0, kw, R0, 0, 0, dk, lane, jend);  // the next diagonal tile
        wave_sync();
        lap(tx);
        factor16r<PK, RCP>(A, r, ld, R0, min(16, w - R0), Dl,
                           MKall ? MKall + (kb + 1) * 16 * LDM : ((kb & 1) ? MK0 : MK1), lane);
        if (!fault) pipe_set(&pc.mk, kb + 2);  // fault: MADIPM_DEBUG_PIPE_FAULT (tests only): never published
        lap(tf);
      }
    } else {
      const int ow = wv - 1;
      if (kb > 0) {
        pipe_wait(&pc.mk, kb + 1, &pc.abort);      // block kb's M_K and pivots
        pipe_wait(&pc.j0, no * kb, &pc.abort);     // every other wave's column-0 tiles of step kb - 1 (raw panel rows)
      }
      lap(tw);
      panel_blocks<PK>(A, r, ld, k0, kw, R0, nbr, MKc, 1 + ow, no, lane);  // rows 1 .. nbr - 1
      ++gen;
      lap(tx);
      pipe_add(&pc.ob);
      pipe_wait(&pc.ob, no * gen, &pc.abort);
      pipe_wait(&pc.pt, kb + 1, &pc.abort);
      lap(tw);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int k = 4 * ks + (lane >> 4);
        dk[ks] = (k < kw) ? Dl[k0 + min(k, kw - 1)] : 0.0;
      }
      if (!last) {
        // priority: strip (1, 0..1) (tile (1, 1) only inside the update range), then (I, 0) for I >= 2
        const bool d11 = nbr > 1 && jhi >= 1;
        for (int it = ow; it < nbr - 1; it += no) {
          if (it == 0) {
            if (d11)
              trail_strip<PK, 2>(A, r, ld, k0, kw, R0, 1, 0, dk, lane, jend);
            else
              trail_strip<PK, 1>(A, r, ld, k0, kw, R0, 1, 0, dk, lane, jend);
          } else {
            trail_strip<PK, 1>(A, r, ld, k0, kw, R0, it + 1, 0, dk, lane, jend);
          }
        }
        pipe_add(&pc.j0);
        // the rest: rows I >= 2, column blocks 1 .. jhi
        trail_strips<PK>(A, r, ld, k0, kw, R0, nbr, 1, jhi, dk, ow, no, lane, jend, 2);
      } else if (!defer) {
        trail_strips<PK>(A, r, ld, k0, kw, R0, nbr, 0, nbr, dk, ow, no, lane, jend);
      }
    }
  }
  if (dbg && tid == 64) pc.ow = tw;
  __syncthreads();
  // a lost hand-off (a wait that timed out) leaves a wrong factor: raise the sticky status error that
  // status() turns into a failure (the flag polls between fronts do the same)
  if (tid == 0 && __hip_atomic_load(&pc.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) && err)
    __hip_atomic_fetch_or(err, kErrHandoff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int64_t t2 = (pt && tid == 0) ? wall_clock64() : 0;
  if (defer && schur) {
    schur_strips<PK>(A, r, ld, w, Dl, wv, nw, lane);
    __syncthreads();
  }
  if (pt && tid == 0) {
    pt[0] = t1 - t0;
    pt[1] = t2 - t1;  // the pipelined block steps
    pt[2] = tw;       // wave 0 waiting for the other waves' priority tiles
    pt[3] = tf;       // wave 0 in factor16r
    pt[4] = wall_clock64() - t2;
    pt[5] = pc.ow;    // wave 1 waiting (M_K, barrier, panel tile 0, column-0 tiles)
  }
}

template <bool PK>
__device__ __forceinline__ void factor_lds(const FrontTab& T, double* A, int r, int w, int ld, double* Dl, double* MK,
                                           double* cbuf, int64_t* pt = nullptr) {
  if (T.fpipe && (blockDim.x >> 6) >= 2)
    blocked_factor_pipe<PK>(A, r, w, ld, Dl, MK, cbuf, 1, pt, T.err, T.pipe_fault);
  else
    blocked_factor_lds<PK>(A, r, w, ld, Dl, MK, cbuf, 1, pt);
}

// write-out: L panel (ld r; d on the diagonal, zeros above), lower triangle of U (ld uld), D and the
// pivot check.  SC1: U stored write-through (handed to a parent inside the same launch).
template <bool PK, bool SC1>
__device__ __forceinline__ void writeout_u(const double* A, int r, int w, int ld, double* Uo, int uld);
// offset of column b of a u x u update block: square ld uld, or packed lower (uld == 0: column b
// holds rows b .. u - 1, entry (a, b) at b (2u - b - 1) / 2 + a)
__device__ __forceinline__ int64_t ucol_off(int b, int u, int64_t uld) {
  return uld ? (int64_t)b * uld : ((int64_t)b * (2 * u - b - 1)) >> 1;
}
template <bool PK>
__device__ __forceinline__ void writeout_ld(const double* A, int r, int w, int ld, const double* Dl, double* L, double* D,
                                           int f0, LDLStatus* st, double tol) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  // L panel (ld r; d on the diagonal, zeros above): columns dealt to waves as in writeout_u
  for (int j0 = 4 * wv; j0 < w; j0 += 4 * nw) {
    double x[4][3], dd[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int j = min(j0 + cb, w - 1);
      const int base = PK ? ((j * (2 * r - j - 1)) >> 1) : j * ld;
      dd[cb] = Dl[j];
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const int i = lane + 64 * h, ic = min(max(i, j), r - 1);
        x[cb][h] = A[base + ic];
      }
    }
    LDL_PIN4(dd);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      asm volatile("" : "+v"(x[cb][0]), "+v"(x[cb][1]), "+v"(x[cb][2]));
      const int j = min(j0 + cb, w - 1);
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const int i = lane + 64 * h;
        x[cb][h] = (i > j) ? x[cb][h] : (i == j ? dd[cb] : 0.0);
      }
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int j = j0 + cb;
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const int i = lane + 64 * h;
        if (j < w && i < r) L[i + (int64_t)j * r] = x[cb][h];
      }
    }
  }
  if (tid < w) {
    const double d = Dl[tid];
    D[f0 + tid] = d;
    if (bad_pivot(d, tol)) atomicMin(&st->fail_pivot, f0 + tid + 1);
  }
}
template <bool PK, bool SC1>
__device__ __forceinline__ void blocked_writeout(const double* A, int r, int w, int ld, const double* Dl, double* L,
                                                 double* Uo, int uld, double* D, int f0, LDLStatus* st, double tol) {
  writeout_ld<PK>(A, r, w, ld, Dl, L, D, f0, st, tol);
  writeout_u<PK, SC1>(A, r, w, ld, Uo, uld);
}
// lower triangle of the update block U (ld uld); SC1: stored write-through (handed to a parent
// inside the same launch)
// columns dealt to waves, NC per wave and round, NH 64-row chunks per column; a column's rows run
// over the lanes, so the LDS and global addresses are a wave-uniform column base + the row (no
// per-element index arithmetic: with one wave per SIMD that arithmetic bounded this loop)
template <bool PK, bool SC1, int NH, int NC>
__device__ __forceinline__ void writeout_u_cols(const double* A, int r, int w, int ld, double* Uo, int uld) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int u = r - w;
  for (int b0 = NC * wv; b0 < u; b0 += nw * NC) {
    double x[NC][NH];
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      const int b = min(b0 + cb, u - 1), j = w + b;
      const int base = PK ? ((j * (2 * r - j - 1)) >> 1) : j * ld;  // fidx(i, j) = base + i
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const int a = min(b + lane + 64 * h, u - 1);
        x[cb][h] = A[base + w + a];
      }
    }
#pragma unroll
    for (int cb = 0; cb < NC; ++cb)
#pragma unroll
      for (int h = 0; h < NH; ++h) LDL_PIN(x[cb][h]);
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      const int b = b0 + cb;
      double* col = Uo + ucol_off(b, u, uld);
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const int a = b + lane + 64 * h;
        if (b < u && a < u) {
          if (SC1)
            __hip_atomic_store(col + a, x[cb][h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else
            col[a] = x[cb][h];
        }
      }
    }
  }
}
template <bool PK, bool SC1>
__device__ __forceinline__ void writeout_u(const double* A, int r, int w, int ld, double* Uo, int uld) {
  const int u = r - w;
  if (u <= 64)
    writeout_u_cols<PK, SC1, 1, 8>(A, r, w, ld, Uo, uld);
  else if (u <= 128)
    writeout_u_cols<PK, SC1, 2, 6>(A, r, w, ld, Uo, uld);
  else
    writeout_u_cols<PK, SC1, 3, 4>(A, r, w, ld, Uo, uld);
}

// lower part of an r x r front assembled in HBM scratch (ld r) -> LDS, 16 loads in flight per thread
template <bool PK, int NTH = NT>
__device__ __forceinline__ void stage_front(const double* __restrict__ Fs, double* A, int r, int ld) {
  const int tid = threadIdx.x;
  const int nel = r * r;
  ColWalk wk(tid, r, NTH);
  for (int base = 0; base < nel; base += NTH * 16) {
    double v[16];
    int dst[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int q = base + k * NTH + tid;
      const bool ok = q < nel && wk.i >= wk.j;
      v[k] = ok ? Fs[q] : 0.0;
      dst[k] = ok ? fidx<PK>(wk.i, wk.j, r, ld) : -1;
      wk.next();
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (dst[k] >= 0) A[dst[k]] = v[k];
  }
}

}  // namespace
}  // namespace madipm
