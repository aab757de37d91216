// Private to the ldl*.hip units (ldl.hip: numeric factorisation; ldl_solve.hip: triangular solves;
// ldl_solver.hip: host side).  It holds ONLY what more than one of them uses, so a change here
// reaches both the factorisation and the solve kernels; a helper of one unit lives in that unit.
// Everything is inlined or has internal linkage: no external device symbol, no -fgpu-rdc.
#pragma once
#include "ldl.hpp"

namespace madipm {
using namespace ldlconst;  // NT and the other constants shared with the planner (ldl_plan.hpp)

// The units' one-time function attributes (dynamic-LDS maxima, LDS fit), called by LDLSolver's
// constructor.  first: no solver of this process has set them yet; ftree_lds: this plan's k_fact_tree
// carve (0: it has no tree launch), checked for every solver.
void ldl_factor_kernel_attributes(bool first, size_t ftree_lds);
void ldl_solve_kernel_attributes();

namespace {

__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// (i, j) of the column-major indices q = q0, q0 + NT, q0 + 2 NT, ... of an r-row matrix: one integer
// division per thread instead of one per element (a division is ~15 VALU instructions, and the
// staging / write-out loops of a front are otherwise dominated by them)
struct ColWalk {
  int i, j, di, dj, r;
  __device__ __forceinline__ ColWalk(int q0, int r_, int stride = NT) : r(r_) {
    j = q0 / r_;
    i = q0 - j * r_;
    dj = stride / r_;
    di = stride - dj * r_;
  }
  __device__ __forceinline__ void next() {
    i += di;
    j += dj;
    if (i >= r) {
      i -= r;
      ++j;
    }
  }
};

// micro fronts (w <= 2, r <= 32): lanes per front, in the factorisation and the solves alike
constexpr int MG = 16;

// Big-front kernels read their (front, item) pair from the launch's task list.
__device__ __forceinline__ void task_of(const int32_t* __restrict__ list, int& s, int& item) {
  const int2 t = reinterpret_cast<const int2*>(list)[blockIdx.x];
  s = t.x;
  item = t.y;
}

// In-launch hand-offs between workgroups (MI355X_MICROARCH.md "inter-workgroup visibility", form R1):
// payload stored sc1 and drained before ONE lane stores the flag; consumers poll relaxed and load sc1.
__device__ __forceinline__ double ld_sc1(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// wave 0: poll the flags of dep[q0 .. q1) together (one lane per dependency, 64 per pass)
__device__ __forceinline__ void poll_deps(const int32_t* __restrict__ dep, int q0, int q1, int32_t* flags, int epoch,
                                          int32_t* err) {
  const int lane = threadIdx.x & 63;
  for (int q = q0; q < q1; q += 64) {
    const int32_t* f = (q + lane < q1) ? flags + dep[q + lane] : nullptr;
    int spins = 0;
    for (;;) {
      const bool ok = !f || __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch;
      if (__all(ok)) break;
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 25)) {
        if (lane == 0) atomicOr(err, kErrHandoff);
        break;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

void set_max_dyn_lds(const void* f, int bytes) {
  MADIPM_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
}

}  // namespace

// bytes: the launch's staging-traffic model; alg: SURVEY 8(d)'s bytes of the same launch
#define TIMED(kind, bytes, alg, flops, launch)          \
  do {                                                  \
    const bool tm_ = t_begin(kind, s);                  \
    launch;                                             \
    if (tm_) t_end(kind, s, (bytes), (alg), (flops));   \
  } while (0)

}  // namespace madipm
