// Multifrontal supernodal LDL^T for gfx950, host side: LDLSolver's construction (symbolic analysis,
// launch plan, uploads, workspace), live kernel timing, the joins with the root tail, the tree
// kernels' debug dump, and ShardGroup.  The numeric factorisation, its status and its launchers are
// in ldl.hip, the triangular solves in ldl_solve.hip; ldl_device.hpp holds what those two share.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstdio>

#include "ldl_device.hpp"

namespace madipm {
namespace {

struct BufList {
  double* p[16];
};
__global__ __launch_bounds__(NT) void k_local_allreduce(BufList B, int nbuf, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
    double v = 0.0;
    for (int q = 0; q < nbuf; ++q) v += B.p[q][i];
    for (int q = 0; q < nbuf; ++q) B.p[q][i] = v;
  }
}

// Upload of a host table; returns the device pointer for the FrontTab field (or kernel argument) it
// feeds.  up: a one-element placeholder when the table is empty, so kernels never see a null table.
template <class T, class V>
T* put(DBuf<T>& d, const V& v) {
  d.upload(v);
  return d.p;
}
template <class T, class V>
T* up(DBuf<T>& d, const V& v, T fill = T{}) {
  if (v.empty())
    d.upload(&fill, 1);
  else
    d.upload(v);
  return d.p;
}

bool env_on(const char* k) {
  const char* v = std::getenv(k);
  return v && v[0] && v[0] != '0';
}

}  // namespace

// symbolic_analyze -> read_ldl_knobs -> build_launch_plan (ldl_plan.cpp: every launch decision, on the
// host) -> uploads -> workspace -> function attributes
LDLSolver::LDLSolver(int n, const int64_t* colptr, const int32_t* rowval, const SymbolicOptions& sopt,
                     double ptol, const int32_t* user_perm, Comm* comm)
    : pivot_tol(ptol), comm_(comm) {
  PhaseClock clk("LDLSolver");
  symbolic_analyze(n, colptr, rowval, sopt, user_perm, S_);
  clk("symbolic_analyze");
  const SymbolicPlan& S = S_;
  MADIPM_REQUIRE(S.nshards == 1 || comm == nullptr || (comm->size == S.nshards && comm->rank == S.shard),
                 "communicator does not match the shard layout");
  knobs_ = read_ldl_knobs();
  LaunchPlan P;  // host tables: they live until the uploads are done (the synchronisation at the end)
  build_launch_plan(S, knobs_, P);
  clk("launch plan (total)");
  const int ns = S.nsuper, NL = S.nlevels;

  // ---- front tables
  T_.first = put(first_, S.first);
  T_.nrows = put(nrows_, S.nrows);
  T_.row_ptr = put(row_ptr_, S.row_ptr);
  T_.rows = put(rows_, S.rows);
  T_.l_off = put(l_off_, S.l_off);
  T_.u_off = put(u_off_, S.u_off);
  T_.u_ld = put(u_ld_, P.u_ld);
  T_.uvec_off = put(uvec_off_, S.uvec_off);
  T_.asm_ptr = put(asm_ptr_, S.asm_ptr);
  T_.asm_src = put(asm_src_, S.asm_src);
  T_.asm_dst = put(asm_dst64_, S.asm_dst);
  T_.child_ptr = put(child_ptr_, S.child_ptr);
  T_.child_list = put(child_list_, S.child_list);
  T_.rel_ptr = put(rel_ptr_, S.rel_ptr);
  T_.rel = put(rel_, S.rel);
  T_.perm = put(perm_, S.perm);
  T_.fs_off = put(fs_off_, S.fs_off);
  T_.fs_img = put(fs_img_, P.fs_img);
  T_.sv_ptr = put(sv_ptr_, S.sv_ptr);
  T_.sv_src = put(sv_src_, P.sv_src);  // reordered: tree-task entries last, sv_nt of them per row
  T_.sv_nt = put(sv_nt_, P.sv_nt);
  T_.bigslot = put(bigslot_, P.bigslot);
  T_.upos = put(upos_, P.upos);
  T_.fpipe = knobs_.fact_pipe;
  T_.pipe_fault = knobs_.pipe_fault;
  T_.asm_src_cap = knobs_.asm_src_cap;
  T_.lds_cap = P.lds_cap;
  // ---- assembly: int32 sources when every arena / K index fits
  if (P.g32_fits)
    g_src32_.upload(P.g_src32);
  else
    g_src_.upload(S.g_src);
  P.g_src32 = {};
  g_chunk_.upload(S.g_chunk);
  gpart_.alloc(std::max<size_t>(S.g_chunk.size(), 1));
  brec_.upload(P.brec);
  g_ptr_.upload(P.g_ptr);
  chunk_ids_.upload(P.chunk_ids);
  atiles_.upload(P.atiles);
  fscratch_.alloc(std::max<int64_t>(S.fs_size, 1));
  minv_.alloc((int64_t)std::max(P.nbigslot, 1) * 4096);
  // ---- sharding
  gper_ = P.gper;
  up(gidx_, P.gidx, -1);
  gsol_.alloc(std::max<int64_t>(S.nshards * gper_, 1));
  T_.xoff = put(xoff_, P.xoff);
  T_.wout = put(wout_, P.wout);
  colmask_.upload(P.colmask);
  xch_.alloc(std::max<int64_t>(S.xlen, 1));
  T_.xch = xch_;
  up(sx_ptr_, S.sx_ptr);
  up(sx_src_, S.sx_src);
  // ---- batched leaf columns
  lb_at_level_ = std::move(P.lb_at_level);
  if (!S.lb.empty()) {
    lbg_.upload(S.lb);
    lbmem_.upload(S.lb_mem);
    lbgid_.upload(P.lb_gid);
    lbxrow_.upload(P.lb_xrow);
    lbpoff_.upload(P.lb_poff);
    lbcs_.upload(S.lb_cs);
    lbce_.upload(S.lb_ce);
    lbwbase_.upload(S.lb_wbase);
    lbwrow_.upload(S.lb_wrow);
    lbgpos_.upload(S.lb_gpos);
    lbW_.alloc(std::max<int64_t>(S.lb_wsize, 1));
    lbW_.zero();  // the pattern is fixed: entries outside it stay 0
    lbd_.alloc(2 * S.lb_mem.size());
    lbpart_.alloc(std::max<int64_t>(P.lb_npart, 1));
  }
  clk("tables + uploads");

  // ---- factorisation tree (k_fact_tree), fold helpers, leaf folding (SymbolicPlan::absorb / fold_* / ab_*)
  nftree_ = P.nftree;
  nfhelp_ = P.nfhelp;
  up(ft_order_, P.ft_order);
  up(ft_dptr_, P.ft_dptr);
  up(ft_dep_, P.ft_dep);
  T_.fstart = put(fstart_, P.fstart);
  T_.fold_help = put(fold_help_, P.fold_help);
  T_.fhelp = up(fhelp_, P.fhelp, FoldHelp{0, 0, 0, 0, 0, 0, FoldStart{0, 0, 0, 0, 0, 0, 0, 0, 0}});
  fimg_.alloc((size_t)std::max<int64_t>(P.fimg_size, 2));
  T_.fimg = fimg_;
  T_.fimg_dst = up(fimg_dst_, P.fimg_dst);
  fflags_.alloc(std::max(ns + nfhelp_, 1));
  fflags_.zero();
  T_.absorb = up(absorb_, S.absorb);
  T_.fold_pk = up(fold_pk_, S.fold_pk);
  T_.mc_ptr = up(mc_ptr_, S.mc_ptr);
  T_.ab_first = up(ab_first_, S.ab_first);
  T_.ab_src0 = up(ab_src0_, S.ab_src0);
  T_.ab_src1 = up(ab_src1_, S.ab_src1);
  T_.ab_k = up(ab_k_, S.ab_k);
  T_.ab_f0 = up(ab_f0_, S.ab_f0);
  T_.ab_wrc = up(ab_wrc_, S.ab_wrc);
  T_.ab_loff = put(ab_loff_, P.ab_loff);
  T_.fold_bptr = up(fold_bptr_, S.fold_bptr);
  T_.fold_bat = up(fold_bat_, S.fold_bat);
  T_.fold_row0 = up(fold_row0_, S.fold_row0);
  T_.fold_poff = up(fold_poff_, S.fold_poff);
  T_.fold_plen = up(fold_plen_, S.fold_plen);
  T_.fold_rmax = up(fold_rmax_, S.fold_rmax);
  T_.fold_lmax = up(fold_lmax_, S.fold_lmax);
  T_.fold_prod = up(fold_prod_, S.fold_prod, SymbolicPlan::kFoldPad);
  T_.fold_chead = up(fold_chead_, S.fold_chead);
  fcnt_.alloc(4);
  fcnt_.zero();
  if (knobs_.tree_debug && nftree_) {
    fdbg_.alloc((int64_t)24 * (nftree_ + nfhelp_));
    fdbg_.zero();
  }
  clk("  fold table uploads");

  // ---- factorisation launches (phase 1: this shard's subtrees; phase 2: the top fronts)
  fact1_ = std::move(P.fact1);
  fact2_ = std::move(P.fact2);
  if (!P.dag_tasks.empty()) {  // DAG tasks, dependencies, flags, counters, per-panel M_K slots
    dag_tasks_.upload(P.dag_tasks);
    dag_dptr_.upload(P.dag_dptr);
    up(dag_dlist_, P.dag_dlist);
    dag_flags_.alloc((int64_t)P.dag_tasks.size() / 4);
    dag_flags_.zero();
    dag_cnt_.alloc(2);
    dag_cnt_.zero();
    dag_m_.alloc(std::max<int64_t>(P.nmslot, 1) * BIG_MSZ);
    dag_mslot_.upload(P.mslot);
    int dev = 0, ncu = 0;
    MADIPM_HIP(hipGetDevice(&dev));
    MADIPM_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    dag_grid_ = std::max(1, 2 * ncu);  // two workgroups per CU (80 KB of LDS, <= 256 registers)
    if (knobs_.dag_debug) {  // per-task stamps (diagnostics)
      dag_dbg_.alloc((int64_t)P.dag_tasks.size());
      dag_dbg_.zero();
      dag_kind_ = P.dag_tasks;
    }
  }
  if (P.upd_np) {  // k_big_upd128's split-K scratch
    upsum_.alloc((size_t)P.upd_np * UPD_PART);
    uptick_.alloc((size_t)P.upd_nt);
    uptick_.zero();
  }

  // ---- solve levels, tree-solve tables, big-front solve tasks
  slev1_ = std::move(P.slev1);
  slev2_ = std::move(P.slev2);
  mlev_ = std::move(P.mlev);
  mstat_.native = S.nshards == 1 && S.lb.empty() && !mlev_.empty();
  for (const SolveLevel& L : mlev_) mstat_.n_big_fronts += mstat_.native ? L.nbig : 0;
  for (const SolveLevel& L : mlev_) mbig_.n_big_levels += mstat_.native && L.nbig > 0;
  mbig_.multi_big = knobs_.multi_big ? 1 : 0;
  xg_off_ = P.xg_off;
  nxg_ = P.nxg;
  ntree_ = P.ntree;
  ntask_ = P.ntask;
  nroot_task_ = P.nroot_task;
  rargs_ = P.rargs;
  tree_lds_ = P.tree_lds;
  root_lds_ = P.root_lds;
  tree_bytes_ = P.tree_bytes, tree_flops_ = P.tree_flops, tree_alg_ = P.tree_alg;
  nsleaf_ = P.nsleaf;
  leaf_bytes_ = P.leaf_bytes, leaf_flops_ = P.leaf_flops, leaf_alg_ = P.leaf_alg;
  tchunk_.upload(P.tchunk);
  trootbwd_.upload(P.trootbwd);
  up(tc_ptr_, P.tc_ptr);
  up(tc_list_, P.tc_list);
  up(tdep_ptr_, P.tdep_ptr);
  up(tdep_, P.tdep);
  up(tpar_, P.tpar);
  up(tleaf_, P.tleaf);
  tlrow_.upload(reinterpret_cast<const int2*>(P.tlrow.data()), P.tlrow.size());
  tflags_.alloc(std::max(ns, 1));
  tflags_.zero();
  gbuf_.alloc(std::max<int64_t>(S.sv_ptr[S.row_ptr[ns]], 1));
  T_.gbuf = gbuf_;
  if (knobs_.tree_debug && ntree_) tdbg_.alloc((int64_t)8 * ntree_);
  if (P.tasks.empty()) P.tasks = {0, 0};
  tasks_.upload(P.tasks);
  flag_off_.upload(P.flag_off);
  bp_off_.upload(P.bp_off);
  bpart_.alloc(std::max<int64_t>(P.nbpart, 1) * 64);
  flags_.alloc(std::max<int64_t>(P.nflags, 1));
  flags_.zero();
  // the big fronts' panel solutions as self-validating words (ll_put / ll_get): 64 values x 2 halves
  // per panel flag
  xll_.alloc(std::max<int64_t>(P.nflags, 1) * 128);
  xll_.zero();
  T_.xll = xll_;
  counters_.alloc(4 * std::max(NL, 1) + 4);  // + the tree-solve tickets (4 NL, 4 NL + 1)
  counters_.zero();

  // ---- the root tail (LaunchPlan::tail_ok: the launch lists allow it).  The tail's kernel waits on
  // the device for a kernel of the caller's stream: never where kernels are serialised (counter
  // collection — rocprofv3 --pmc dispatches one kernel at a time, and the waiting kernel would hold
  // the GPU until its wait times out — AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING)
  const bool serial = env_on("ROCPROF_COUNTER_COLLECTION") || env_on("ROCPROF_COUNTERS") ||
                      env_on("AMD_SERIALIZE_KERNEL") || env_on("HIP_LAUNCH_BLOCKING");
  root_async_ = P.tail_ok && !serial && knobs_.root_async != '0';
  if (knobs_.root_async == '2')  // diagnostics: why (not)
    fprintf(stderr, "root tail: async %d %s\n", (int)root_async_, P.tail_diag.c_str());
  if (root_async_) {
    side0_ = P.side0;
    nroot_side_ = P.nroot_side;
    asm_side_ = P.asm_side;
    side_tree_ = P.side_tree;
    int lo = 0, hi = 0;  // the tail is the critical path beside the forward solve: the higher priority
    MADIPM_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    MADIPM_HIP(hipStreamCreateWithPriority(&side_, hipStreamNonBlocking, hi));
    MADIPM_HIP(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
    const int64_t ncb = asm_side_ ? cdiv(fact1_[side0_ - 1].nchunk, NT) : 0;
    rflag_.alloc(2 + 64 + ncb);  // go, the assembly's tile counter, one done flag per root, chunk blocks
    rflag_.zero();
    tside_.upload(P.tside);
  }
  clk("  launch + solve table uploads");
  up(sched_, P.sched);
  arena_.alloc(std::max<int64_t>(S.arena_size, 2));
  if (S.nshards > 1) {  // top fronts: the strict upper triangles are never written, keep them 0
    MADIPM_HIP(hipMemset(arena_.p + S.top_lo, 0, sizeof(double) * (S.arena_size - S.top_lo)));
    // exchange buffer: the top fronts' lower triangles (column by column) + 4 status slots per shard
    ntopcol_ = (int)(P.topcol.size() / 3);
    xpack_tri_ = P.xpack_tri;
    if (P.topcol.empty()) P.topcol = {0, 0, 0};
    topcol_.upload(P.topcol);
    xpack_.alloc(xpack_tri_ + 4 * S.nshards);
    xpack_.zero();
  }
  clk("  sched upload + arena");
  D_.alloc(std::max(S.N, 1));
  xi_.alloc(std::max(S.N, 1));
  uvec_.alloc(std::max<int64_t>(S.uvec_size, 1));
  vwork_.alloc(std::max<int64_t>(S.row_ptr[ns], 1));
  status_.alloc(1);
  MADIPM_HIP(hipHostMalloc((void**)&h_status_, sizeof(LDLStatus), hipHostMallocDefault));
  st_ = status_.p;
  h_st_ = h_status_;
  T_.err = &st_->err;
  status_.zero();
  h_st_->err = 0;
  static bool attr_done = false;
  if (!attr_done) ldl_solve_kernel_attributes();
  ldl_factor_kernel_attributes(!attr_done, nftree_ ? (size_t)P.ftree_lds : 0);
  attr_done = true;
  clk("  buffers + attributes");
  MADIPM_HIP(hipDeviceSynchronize());
  clk("schedules + workspace");
}

LDLSolver::~LDLSolver() {
  if (side_) {  // a root tail never joined (a factorisation nothing solved with) ends before its buffers
    (void)hipStreamSynchronize(side_);
    (void)hipStreamDestroy(side_);
  }
  if (ev_join_) (void)hipEventDestroy(ev_join_);
  if (h_status_) (void)hipHostFree(h_status_);
  for (hipEvent_t e : evs_) (void)hipEventDestroy(e);
}

const char* kernel_kind_name(int k) {
  static const char* names[] = {"k_asm_chunks", "k_assemble",   "k_micro_factor", "k_small_blocked", "k_big_diag",
                                "k_big_trsm",   "k_big_update", "k_inertia",      "k_fwd_small",     "k_fwd_gather",
                                "k_fwd_big",    "k_bwd_below",  "k_bwd_big",      "k_bwd_small",     "k_fwd_tiny",
                                "k_bwd_tiny",   "k_lb_build",   "k_lb_syrk",      "k_lb_gemv",       "k_fwd_tree",
                                "k_bwd_tree",   "k_fact_tree",  "k_asm_update",   "k_big_dag"};
  static_assert(sizeof(names) / sizeof(*names) == KK_COUNT, "one name per KernelKind");
  return (k >= 0 && k < KK_COUNT) ? names[k] : "?";
}

void LDLSolver::set_timing(unsigned mask) {
  tmask_ = mask;
  ev_used_ = 0;
  pend_.clear();
  for (auto& k : kst_) k = KernelStat{};
}

bool LDLSolver::t_begin(int kind, hipStream_t s) {
  if (!(tmask_ >> kind & 1u) || untimed_) return false;
  while (evs_.size() < ev_used_ + 2) {
    hipEvent_t e;  // no system-scope fence: the timestamps bracket the kernel, not a cache flush
    MADIPM_HIP(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    evs_.push_back(e);
  }
  pend_.push_back({kind, ev_used_, 0.0, 0.0, 0.0});
  MADIPM_HIP(hipEventRecord(evs_[ev_used_], s));
  ev_used_ += 2;
  return true;
}

void LDLSolver::t_end(int kind, hipStream_t s, double bytes, double alg, double flops) {
  Pending& p = pend_.back();
  (void)kind;
  p.bytes = bytes;
  p.alg = alg;
  p.flops = flops;
  MADIPM_HIP(hipEventRecord(evs_[p.e0 + 1], s));
}

void LDLSolver::kernel_stats(KernelStat out[KK_COUNT]) {
  for (const Pending& p : pend_) {
    MADIPM_HIP(hipEventSynchronize(evs_[p.e0 + 1]));
    float ms = 0.f;
    MADIPM_HIP(hipEventElapsedTime(&ms, evs_[p.e0], evs_[p.e0 + 1]));
    KernelStat& k = kst_[p.kind];
    k.launches++;
    k.ms += ms;
    k.bytes += p.bytes;
    k.alg_bytes += p.alg;
    k.flops += p.flops;
  }
  pend_.clear();
  ev_used_ = 0;
  for (int k = 0; k < KK_COUNT; ++k) out[k] = kst_[k];
}

void LDLSolver::join(hipStream_t s) {
  if (!root_pending_) return;
  MADIPM_HIP(hipStreamWaitEvent(s, ev_join_, 0));
  root_pending_ = false;
}

double LDLSolver::fact_seconds(hipStream_t s) {
  if (S_.N == 0) return 0.0;
  join(s);
  LDLStatus h;
  MADIPM_HIP(hipMemcpyAsync(&h, st_, sizeof(LDLStatus), hipMemcpyDeviceToHost, s));
  MADIPM_HIP(hipStreamSynchronize(s));
  int dev = 0, khz = 0;
  MADIPM_HIP(hipGetDevice(&dev));
  MADIPM_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
  const uint64_t t = h.ticks + (h.t1 > h.t0 ? h.t1 - h.t0 : 0);
  return khz > 0 ? (double)t / (1e3 * khz) : 0.0;
}

// MADIPM_TREE_DEBUG=1: per-task wall-clock phases of the tree kernels (100 MHz counter), summarised
// per level on stderr for the first few launches (diagnostics only)
void LDLSolver::tree_debug_dump(hipStream_t s, const char* what, const int64_t* dbuf, int nt, const char* p1,
                                const char* p2, const char* p3, const char* p4, const char* p5, int stride) {
  static int ndump = 0;
  if (ndump++ >= 8) return;
  std::vector<int64_t> hs((size_t)stride * nt), h((size_t)8 * nt);
  MADIPM_HIP(hipMemcpyAsync(hs.data(), dbuf, hs.size() * 8, hipMemcpyDeviceToHost, s));
  MADIPM_HIP(hipStreamSynchronize(s));
  for (int t = 0; t < nt; ++t)
    for (int k = 0; k < 8; ++k) h[8 * t + k] = hs[(size_t)stride * t + k];
  if (stride == 24) {  // factor sub-phases, leaf-folding phases, per level
    std::vector<double> ab((size_t)S_.nlevels * 6, 0.0), fo((size_t)S_.nlevels * 4, 0.0);
    std::vector<int> na(S_.nlevels, 0);
    for (int t = 0; t < nt; ++t) {
      const int lv = S_.level[(int)h[8 * t + 6]];
      na[lv]++;
      for (int k = 0; k < 6; ++k) ab[lv * 6 + k] += hs[(size_t)24 * t + 8 + k] * 0.01;
      for (int k = 0; k < 4; ++k) fo[lv * 4 + k] += hs[(size_t)24 * t + 16 + k] * 0.01;
    }
    for (int lv = 0; lv < S_.nlevels; ++lv)
      if (na[lv])
        fprintf(stderr, "  fold level %d: gather %.2f  pivots %.2f  L %.2f  products %.2f us\n", lv, fo[lv * 4] / na[lv],
                fo[lv * 4 + 1] / na[lv], fo[lv * 4 + 2] / na[lv], fo[lv * 4 + 3] / na[lv]);
    std::vector<double> sq((size_t)S_.nlevels * 3, 0.0);
    for (int t = 0; t < nt; ++t) {
      const int lv = S_.level[(int)h[8 * t + 6]];
      const int64_t* d = &hs[(size_t)24 * t];
      sq[lv * 3] += (d[14] - d[4]) * 0.01;
      sq[lv * 3 + 1] += (d[15] - d[14]) * 0.01;
      sq[lv * 3 + 2] += (d[5] - d[15]) * 0.01;
    }
    for (int lv = 0; lv < S_.nlevels; ++lv)
      if (na[lv])
        fprintf(stderr, "  store level %d: U issue %.2f  drain+flag %.2f  L/D %.2f us\n", lv, sq[lv * 3] / na[lv],
                sq[lv * 3 + 1] / na[lv], sq[lv * 3 + 2] / na[lv]);
    for (int lv = 0; lv < S_.nlevels; ++lv)
      if (na[lv] && T_.fpipe)
        fprintf(stderr,
                "  factor level %d: %d fronts  first16 %.2f  block steps %.2f  (wave 0: waits %.2f  diag factors %.2f; "
                "wave 1 waits %.2f)  schur %.2f us\n",
                lv, na[lv], ab[lv * 6] / na[lv], ab[lv * 6 + 1] / na[lv], ab[lv * 6 + 2] / na[lv], ab[lv * 6 + 3] / na[lv],
                ab[lv * 6 + 5] / na[lv], ab[lv * 6 + 4] / na[lv]);
      else if (na[lv])
        fprintf(stderr,
                "  factor level %d: %d fronts  first16 [kcyc/100] %.2f  first16 %.2f  panels %.2f  J0 %.2f  look %.2f  schur %.2f us\n",
                lv, na[lv], ab[lv * 6 + 5] / na[lv], ab[lv * 6] / na[lv], ab[lv * 6 + 1] / na[lv], ab[lv * 6 + 2] / na[lv],
                ab[lv * 6 + 3] / na[lv], ab[lv * 6 + 4] / na[lv]);
  }
  // tasks that stamped nothing (the big roots: k_root_solve) are skipped; a stamp a path did not
  // take (a chunked front's) repeats the previous one
  for (int t = 0; t < nt; ++t) {
    int64_t* d = &h[8 * t];
    if (d[0] == 0) continue;
    for (int k = 1; k <= 5; ++k)
      if (d[k] == 0) d[k] = d[k - 1];
  }
  int64_t t0 = INT64_MAX, t1 = 0;
  for (int t = 0; t < nt; ++t)
    if (h[8 * t]) t0 = std::min(t0, h[8 * t]), t1 = std::max(t1, h[8 * t + 5]);
  std::vector<double> acc((size_t)S_.nlevels * 8, 0.0);
  std::vector<int> cnt(S_.nlevels, 0);
  for (int t = 0; t < nt; ++t) {
    const int64_t* d = &h[8 * t];
    if (d[0] == 0) continue;
    const int lv = S_.level[(int)d[6]];
    cnt[lv]++;
    acc[lv * 8 + 0] += (d[0] - t0) * 0.01;
    for (int k = 1; k <= 5; ++k) acc[lv * 8 + k] += (d[k] - d[k - 1]) * 0.01;
    acc[lv * 8 + 6] = std::max(acc[lv * 8 + 6], (d[5] - t0) * 0.01);
  }
  fprintf(stderr, "tree %s: %d tasks, span %.1f us\n", what, nt, (t1 - t0) * 0.01);
  if (stride == 24) {  // the critical path: from the last front to end, back through the latest child
    std::vector<int> task_of(S_.nsuper, -1);
    for (int t = 0; t < nt; ++t) task_of[(int)h[8 * t + 6]] = t;
    int t = 0;
    for (int q = 1; q < nt; ++q)
      if (h[8 * q + 5] > h[8 * t + 5]) t = q;
    for (int depth = 0; t >= 0 && depth < 12; ++depth) {
      const int64_t* d = &h[8 * t];
      const int sf = (int)d[6];
      auto us = [&](int k) { return (d[k] - t0) * 0.01; };
      fprintf(stderr, "  crit front %6d lev %d r %3d w %3d: start %6.1f %s %6.1f %s %6.1f %s %6.1f %s %6.1f %s %6.1f\n", sf,
              S_.level[sf], S_.nrows[sf], S_.first[sf + 1] - S_.first[sf], us(0), p1, us(1), p2, us(2), p3, us(3), p4,
              us(4), p5, us(5));
      int nxt = -1;
      for (int q = S_.child_ptr[sf]; q < S_.child_ptr[sf + 1]; ++q) {
        const int c = S_.child_list[q], tc = task_of[c];
        if (tc >= 0 && (nxt < 0 || h[8 * tc + 5] > h[8 * nxt + 5])) nxt = tc;
      }
      t = nxt;
    }
  }
  for (int lv = 0; lv < S_.nlevels; ++lv)
    if (cnt[lv])
      fprintf(stderr, "  level %d: %5d fronts  start %.1f  %s %.2f  %s %.2f  %s %.2f  %s %.2f  %s %.2f  last end %.1f us\n", lv,
              cnt[lv], acc[lv * 8] / cnt[lv], p1, acc[lv * 8 + 1] / cnt[lv], p2, acc[lv * 8 + 2] / cnt[lv], p3,
              acc[lv * 8 + 3] / cnt[lv], p4, acc[lv * 8 + 4] / cnt[lv], p5, acc[lv * 8 + 5] / cnt[lv], acc[lv * 8 + 6]);
}

// ------------------------------------------------------------------ ShardGroup (P shards, one device)
void local_allreduce(double* const* bufs, int nbuf, int64_t n, hipStream_t s) {
  MADIPM_REQUIRE(nbuf >= 1 && nbuf <= 16, "local_allreduce: 1..16 buffers");
  if (n <= 0) return;
  BufList B{};
  for (int q = 0; q < nbuf; ++q) B.p[q] = bufs[q];
  k_local_allreduce<<<(unsigned)std::min<int64_t>(2048, cdiv(n, NT)), NT, 0, s>>>(B, nbuf, n);
  MADIPM_HIP(hipGetLastError());
}

ShardGroup::ShardGroup(int nshards, int n, const int64_t* colptr, const int32_t* rowval, const SymbolicOptions& sopt,
                       double pivot_tol, const int32_t* user_perm) {
  MADIPM_REQUIRE(nshards >= 1 && nshards <= 16, "ShardGroup: 1..16 shards");
  for (int r = 0; r < nshards; ++r) {
    SymbolicOptions o = sopt;
    o.nshards = nshards;
    o.shard = r;
    sh_.push_back(std::make_unique<LDLSolver>(n, colptr, rowval, o, pivot_tol, user_perm));
  }
  rhs_.resize(nshards);
  for (int r = 1; r < nshards; ++r) rhs_[r].alloc(std::max(n, 1));
}

void ShardGroup::factorize_async(const double* Kx, hipStream_t s) {
  const int P = (int)sh_.size();
  for (auto& h : sh_) h->spd = spd;
  for (int r = 0; r < P; ++r) sh_[r]->fact_phase1(Kx, s);
  if (P > 1) {
    std::vector<double*> bufs;
    for (auto& h : sh_) bufs.push_back(h->fact_xbuf());
    local_allreduce(bufs.data(), P, sh_[0]->fact_xlen(), s);
  }
  for (int r = 0; r < P; ++r) sh_[r]->fact_phase2(s);
}

int ShardGroup::status(hipStream_t s, bool sync) {
  int st = sh_[0]->status(s, sync);
  for (size_t r = 1; r < sh_.size(); ++r)
    MADIPM_REQUIRE(sh_[r]->status(s, false) == st, "ShardGroup: shards disagree on the factorisation status");
  return st;
}

void ShardGroup::solve_async(double* b, hipStream_t s) {
  const int P = (int)sh_.size();
  const int n = sh_[0]->n();
  std::vector<double*> rhs(P);
  rhs[0] = b;
  for (int r = 1; r < P; ++r) {
    rhs[r] = rhs_[r].p;
    MADIPM_HIP(hipMemcpyAsync(rhs[r], b, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  }
  for (int r = 0; r < P; ++r) sh_[r]->solve_phase1(rhs[r], s);
  if (P == 1) return;
  std::vector<double*> xb;
  for (auto& h : sh_) xb.push_back(h->solve_xbuf());
  local_allreduce(xb.data(), P, sh_[0]->solve_xlen(), s);
  for (int r = 0; r < P; ++r) sh_[r]->solve_phase2(rhs[r], s);
  std::vector<double*> gb;
  for (auto& h : sh_) gb.push_back(h->solve_gbuf());
  local_allreduce(gb.data(), P, P * sh_[0]->solve_gper(), s);  // the gather (slices zero elsewhere)
  sh_[0]->solve_phase3(b, s);  // the other shards' copies are scratch
}

}  // namespace madipm
