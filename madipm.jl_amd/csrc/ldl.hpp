// Multifrontal supernodal LDL^T on the GPU (gfx950) — the linear-solver plugin of SURVEY §8 a11/a14.
//
// Replaces `MadNLP.factorize!(kkt.linear_solver)` / `MadNLP.solve!(kkt.linear_solver, x)` for the
// solvers the reference plugs in (LDLFactorizations' LDLSolver, MadNLPGPU's CUDSSSolver with
// cudss_algorithm = LDL, HSL Ma57Solver): called from src/linear_solver.jl:10 and :26 via MadNLP.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "common.hpp"
#include "ldl_plan.hpp"
#include "symbolic.hpp"

namespace madipm {

// Device view of the front table (SoA, all device pointers).
struct FrontTab {
  const int32_t* first;
  const int32_t* nrows;
  const int64_t* row_ptr;
  const int32_t* rows;
  const int64_t* l_off;
  const int64_t* u_off;
  const int32_t* u_ld;
  const int64_t* uvec_off;
  const int64_t* asm_ptr;
  const int64_t* asm_src;
  const int64_t* asm_dst;
  const int32_t* child_ptr;
  const int32_t* child_list;
  const int64_t* rel_ptr;
  const int32_t* rel;
  const int32_t* perm;
  const int64_t* fs_off;   // small fronts assembled by k_assemble: r x r scratch offset (else -1)
  const int64_t* sv_ptr;   // forward-solve gather lists (indexed by row_ptr[s] + i)
  const int64_t* sv_src;
  const uint16_t* sv_nt;   // per row: its trailing gather entries from tree tasks (tree solve tables)
  const int32_t* bigslot;  // big front -> slot in the panel-inverse scratch (64x64 per slot)
  // sharding: top fronts start their forward solve from the exchanged vector xch[xoff[s] + i]
  // (xoff = -1 elsewhere); wout[s] = 0 would suppress the write of x to the caller's vector (every
  // shard writes the top x it computes redundantly: all 1)
  const int64_t* xoff;
  const double* xch;
  const uint8_t* wout;
  // tree solves: update entry a of front c goes to gbuf[upos[rel_ptr[c] + a]] when c's parent is a
  // tree front (its contiguous gather range), else to uvec[uvec_off[c] + a] (upos = -1)
  const int64_t* upos;
  double* gbuf;
  // leaf folding (SymbolicPlan::absorb / fold_* / ab_*)
  const uint8_t* absorb;
  const uint8_t* fold_pk;
  const int32_t* mc_ptr;
  const int64_t* ab_first;
  const int32_t* ab_src0;
  const int32_t* ab_src1;
  const int32_t* ab_k;
  const int32_t* ab_f0;
  const int32_t* ab_wrc;
  const int64_t* ab_loff;
  const int32_t* fold_bptr;
  const int32_t* fold_bat;
  const int64_t* fold_row0;
  const int64_t* fold_poff;
  const int32_t* fold_plen;
  const int32_t* fold_rmax;
  const int32_t* fold_lmax;
  const uint32_t* fold_prod;
  const uint32_t* fold_chead;
  const uint8_t* fs_img;  // 1: fscratch holds the front's LDS image (tree fronts), else ld r
  int32_t* err;     // the status block's sticky error (LDLStatus::err): a timed-out hand-off inside a front
  int fpipe;        // pipelined in-LDS schedule (blocked_factor_pipe; MADIPM_FACT_PIPE=0: blocked_factor_lds)
  int pipe_fault;   // tests (MADIPM_DEBUG_PIPE_FAULT=1): blocked_factor_pipe drops one hand-off
  int lds_cap;      // k_fact_tree's dynamic LDS (bytes): a front (+ its leaf batches) beyond it is an error
  int asm_src_cap;  // assembly LDS source path: a tile of more sources is an error (kErrAsmSrc); tests shrink it
  // fold helpers (k_fact_tree tickets before the fronts): a helper folds the first batches of a front's
  // micro leaves into a zeroed LDS image and hands it over in HBM (fimg); the front folds the rest
  // from fstart[s] and adds the image after its waits (fold_help[s] = the helper, -1: none)
  const FoldStart* fstart;  // per front: the batches it folds itself
  const int32_t* fold_help;
  const FoldHelp* fhelp;
  double* fimg;
  const uint16_t* fimg_dst;  // per helper: the sorted LDS destinations of its products (FoldHelp::dofs)
  uint64_t* xll;  // big-front solves: panel solutions as self-validating words (ll_put / ll_get)
};

// LDLStatus::err bits (sticky; status() raises on any)
constexpr int32_t kErrHandoff = 1;   // a dependency hand-off (flag poll) timed out
constexpr int32_t kErrLdsCarve = 2;  // a k_fact_tree front or leaf batch did not fit its LDS carve
constexpr int32_t kErrAsmSrc = 4;    // an assembly tile on the LDS source path has more sources than its windows

struct SolveTask {
  int32_t front, blk;
};

struct LDLStatus {  // device-resident, read back by status()
  int32_t fail_pivot;  // min failing internal pivot + 1 (INT32_MAX when none)
  int32_t npos, nneg, nzero;
  int32_t err;  // sticky: a dependency hand-off (flag poll) timed out in a factorisation or solve
  int32_t pad_;
  // device wall clock (wall_clock64, hipDeviceAttributeWallClockRate): t0 at the start of the latest
  // factorisation, t1 at its end; ticks = the sum over the earlier ones (folded in by the next start)
  uint64_t t0, t1, ticks;
};

// Start of a factorisation (k_status_init's work; one thread): fold the previous factorisation's
// time in, stamp t0, clear the pivot check and the inertia counts.  A caller whose own kernel runs
// right before the factorisation does this itself (LinSolver::ext_reset) and saves that launch.
__device__ __forceinline__ void ldl_status_start(LDLStatus* st) {
  const uint64_t now = wall_clock64();
  if (st->t1 > st->t0) st->ticks += st->t1 - st->t0;
  st->t0 = st->t1 = now;
  st->fail_pivot = INT32_MAX;
  st->npos = st->nneg = st->nzero = 0;
}
// end of a factorisation whose inertia is counted lazily (LinSolver::lazy_inertia): stamp t1
__device__ __forceinline__ void ldl_status_end(LDLStatus* st) { st->t1 = wall_clock64(); }

// Kernel kinds for the live per-kernel timing (HIP events around each launch on the launch
// stream) and their algorithmic bytes / flops per launch (DESIGN.md "Kernels and their rooflines").
enum KernelKind {
  KK_ASM_CHUNKS = 0, KK_ASSEMBLE, KK_TINY, KK_SMALL, KK_DIAG, KK_TRSM, KK_UPDATE, KK_INERTIA,
  KK_FWD_SMALL, KK_FWD_GATHER, KK_FWD_BIG, KK_BWD_BELOW, KK_BWD_BIG, KK_BWD_SMALL, KK_FWD_TINY, KK_BWD_TINY,
  KK_LB_BUILD, KK_LB_SYRK, KK_LB_GEMV, KK_FWD_TREE, KK_BWD_TREE, KK_FACT_TREE, KK_ASM_UPDATE, KK_BIG_DAG,
  KK_COUNT
};
const char* kernel_kind_name(int k);

struct KernelStat {
  int64_t launches = 0;
  double ms = 0.0, bytes = 0.0, flops = 0.0;
  double alg_bytes = 0.0;  // SURVEY 8(d)'s bytes of the launches (8 nnzL + 12 nnzK of the columns factorised,
                           // 8 nnzL of the columns a solve launch substitutes); `bytes` = the staging model
};

// All-reduce (sum) of a device buffer across the shards of a sharded factorisation, ordered on
// `s`.  RcclComm (csrc/comm.cpp) is the multi-GPU implementation (RCCL over xGMI).
struct Comm {
  int rank = 0, size = 1;
  virtual ~Comm() = default;
  virtual void allreduce_sum(double* buf, int64_t n, hipStream_t s) = 0;
  // In-place all-gather of `size` slices of nper doubles: rank q's slice is buf[q nper, (q+1) nper)
  // and the other slices are zero on entry, so a sum all-reduce of the whole buffer is a valid (twice
  // as heavy) implementation — the default, for communicators without a gather (HostComm).
  virtual void allgather_inplace(double* buf, int64_t nper, hipStream_t s) { allreduce_sum(buf, nper * size, s); }
};
Comm* make_rccl_comm(int nranks, int rank, const void* unique_id /* 128 bytes */);
void rccl_unique_id(void* out /* 128 bytes */);
Comm* make_host_comm(int nranks, int rank, int (*fn)(double*, int64_t, void*), void* ctx);

// What a solver's multi-right-hand-side solves did so far (madipm_ldl_multi_info).
struct MultiStat {
  int32_t width = ldlconst::MULTI_W;  // columns of one chunk
  int32_t native = 0;                 // 1: the level-scheduled multi-column route, 0: the loop of single solves
  int64_t n_calls = 0, n_chunks = 0, n_columns = 0;
  int64_t n_big_fronts = 0;  // fronts of the native route's big class (task-queue kernels)
};
// How the native route solves its big fronts (madipm_ldl_multi_big_info).
struct MultiBigStat {
  int32_t multi_big = 1;     // 1: a chunk's columns in one pass per level and direction, 0: column after column
  int32_t n_big_levels = 0;  // levels of the native route that hold a big front
  int64_t n_big_passes = 0;  // (level, direction) big passes launched so far
  int64_t big_bytes = 0;     // device bytes of the multi hand-off, vwork and bpart buffers (0 before the first use)
};

// Linear-solver interface the MPC driver uses (MadNLP.AbstractLinearSolver methods).
class LinSolver {
 public:
  virtual ~LinSolver() = default;
  virtual void factorize_async(const double* Kx, hipStream_t s) = 0;
  // sync = false: the caller already waited for an event recorded after factorize_async
  virtual int status(hipStream_t s, bool sync = true) = 0;
  // Keep the factorisation status at caller-provided device / pinned-host addresses, so the caller's
  // own per-iteration read-back carries it (no separate copy); status(s, false) then reads the
  // caller's copy.  Returns false when unsupported (sharded solvers).
  virtual bool external_status(LDLStatus* dev, LDLStatus* host) {
    (void)dev;
    (void)host;
    return false;
  }
  virtual void solve_async(double* b, hipStream_t s) = 0;
  // k right-hand sides in place, column j at b + j n().  The default is the loop of single solves (column by
  // column the bits of solve_async); LDLSolver has a multi-column route
  virtual void solve_multi_async(double* b, int k, hipStream_t s) {
    if (k <= 0) return;
    ++mstat_.n_calls;
    mstat_.n_columns += k;
    mstat_.n_chunks += (k + mstat_.width - 1) / mstat_.width;
    for (int j = 0; j < k; ++j) solve_async(b + (int64_t)j * n(), s);
  }
  const MultiStat& multi_stat() const { return mstat_; }
  const MultiBigStat& multi_big_stat() const { return mbig_; }
  // the switch of the big fronts' multi-column pass; solvers without the native route only record it
  virtual void set_multi_big(bool on) { mbig_.multi_big = on ? 1 : 0; }
  virtual const SymbolicPlan& plan() const = 0;
  virtual void set_timing(unsigned mask) = 0;
  virtual void kernel_stats(KernelStat out[]) = 0;
  virtual int n() const = 0;
  // doubles all-reduced per factorisation / per solve, and all-gathered per solve (the whole
  // buffer, nshards slices) — 0 unsharded
  virtual int64_t xch_fact() const { return 0; }
  virtual int64_t xch_solve() const { return 0; }
  virtual int64_t xch_gather() const { return 0; }
  // seconds of device time spent in factorisations so far (synchronises s; cnt.linear_solver_time)
  virtual double fact_seconds(hipStream_t s) = 0;
  bool spd = false;  // Cholesky semantics: any non-positive pivot fails (normal equations)
  // launch savings for a driver that owns the kernels around the factorisation (MPCSolver):
  //   ext_reset: the driver's kernel right before every factorisation runs ldl_status_start on the
  //     status block (external_status) — no k_status_init launch;
  //   lazy_inertia: no k_inertia after the factorisation (the driver's next kernel runs
  //     ldl_status_end); the pivot check does not need it unless spd, and inertia() counts on demand
  bool ext_reset = false, lazy_inertia = false;
  virtual void count_inertia(hipStream_t s) { (void)s; }
  // The factorisation's tail (an elimination-tree root factorised after the tree launch, LDLSolver::
  // root_async_) may run on a side stream after factorize_async returns, beside the next solve's
  // forward leaves and tree fronts.  join(s) orders s after it; solve_async, status(s, true),
  // count_inertia and fact_seconds join by themselves.  With tail_async() the status carried by a
  // kernel enqueued right after factorize_async is not final: read it after the next solve.
  virtual bool tail_async() const { return false; }
  virtual void join(hipStream_t s) { (void)s; }

 protected:
  MultiStat mstat_;
  MultiBigStat mbig_;
};

class LDLSolver : public LinSolver {
 public:
  LDLSolver(int n, const int64_t* colptr, const int32_t* rowval, const SymbolicOptions& sopt,
            double pivot_tol, const int32_t* user_perm = nullptr, Comm* comm = nullptr);
  ~LDLSolver();
  LDLSolver(const LDLSolver&) = delete;
  LDLSolver& operator=(const LDLSolver&) = delete;

  // Enqueue the numeric factorisation of the values `Kx` (device, caller's CSC order) on `s`.
  // Sharded: phase 1, all-reduce of the top fronts (comm), phase 2.
  void factorize_async(const double* Kx, hipStream_t s) override;
  // Synchronise `s` and return 0 or failing pivot + 1; fills the inertia.
  int status(hipStream_t s, bool sync = true) override;
  bool external_status(LDLStatus* dev, LDLStatus* host) override;
  // In-place solve K x = b for a device vector of length n (caller's ordering).
  void solve_async(double* b, hipStream_t s) override;
  void solve_multi_async(double* b, int k, hipStream_t s) override;
  void set_multi_big(bool on) override;

  // Phases of a sharded factorisation / solve, for callers that run their own collective
  // (ShardGroup below, or a host binding with its own RCCL communicator):
  //   factorize: fact_phase1; all-reduce fact_xbuf(); fact_phase2
  //   solve:     solve_phase1; all-reduce solve_xbuf(); solve_phase2; all-gather solve_gbuf()
  //              (nshards slices of solve_gper(); this shard's slice filled, the others zero);
  //              solve_phase3
  void fact_phase1(const double* Kx, hipStream_t s);
  void count_inertia(hipStream_t s) override;  // lazy_inertia: the counts of the current factor
  void fact_phase2(hipStream_t s);
  void solve_phase1(double* b, hipStream_t s);
  void solve_phase2(double* b, hipStream_t s);
  void solve_phase3(double* b, hipStream_t s);
  double* fact_xbuf() const { return xpack_.p; }  // the top fronts' lower triangles + status slots
  int64_t fact_xlen() const { return S_.nshards > 1 ? xpack_tri_ + 4 * S_.nshards : 0; }
  double* solve_xbuf() const { return xch_.p; }
  int64_t solve_xlen() const { return S_.nshards > 1 ? S_.xlen : 0; }
  double* solve_gbuf() const { return gsol_.p; }
  int64_t solve_gper() const { return gper_; }  // doubles per shard slice of solve_gbuf()
  bool sharded() const { return S_.nshards > 1; }
  int64_t xch_fact() const override { return fact_xlen(); }
  int64_t xch_solve() const override { return sharded() ? solve_xlen() : 0; }
  int64_t xch_gather() const override { return sharded() ? S_.nshards * gper_ : 0; }
  double fact_seconds(hipStream_t s) override;
  bool tail_async() const override { return root_async_; }
  void join(hipStream_t s) override;

  const SymbolicPlan& plan() const override { return S_; }
  int n() const override { return S_.N; }
  int npos = 0, nneg = 0, nzero = 0;
  bool factorized = false;
  double pivot_tol = 0.0;

  // device buffers for diagnostics
  const double* d_diag() const { return D_.p; }

  // live kernel timing: bit k of `mask` => HIP events around every launch of KernelKind k.
  // set_timing() clears the accumulated statistics; kernel_stats() synchronises the events.
  void set_timing(unsigned mask) override;
  void kernel_stats(KernelStat out[KK_COUNT]) override;

 private:
  // ---- front tables: the symbolic plan, the kernels' view of it (T_) and the tables T_ points to;
  // the factor itself (L panels and update blocks in arena_, pivots in D_)
  SymbolicPlan S_;
  LdlKnobs knobs_;  // the MADIPM_* environment, read once by the constructor
  FrontTab T_{};
  DBuf<int32_t> first_, nrows_, rows_, u_ld_, child_ptr_, child_list_, rel_, perm_, sched_;
  DBuf<int32_t> bigslot_;
  DBuf<int64_t> fs_off_, sv_ptr_, sv_src_;
  DBuf<int64_t> row_ptr_, l_off_, u_off_, uvec_off_, asm_ptr_, asm_src_, asm_dst64_, rel_ptr_;
  DBuf<uint16_t> sv_nt_;
  DBuf<int64_t> upos_;
  DBuf<uint8_t> fs_img_;
  DBuf<double> arena_, D_;

  // ---- factorisation (ldl.hip)
  std::vector<Launch> fact1_, fact2_;  // phase 1 (this shard's subtrees; everything unsharded), phase 2 (top)
  // launches [b, e) of L on s; stamp: SMALL* launches stamp the factorisation's end into it
  void run_fact(const std::vector<Launch>& L, const double* Kx, hipStream_t s, size_t b = 0, size_t e = SIZE_MAX,
                LDLStatus* stamp = nullptr);
  // the root tail on a side stream (MADIPM_ROOT_ASYNC, default on): fact1_[side0_] (the last launch)
  // factorises elimination-tree roots that only k_root_solve reads.  It is enqueued on side_ and waits
  // on the device for rflag_[0] == repoch_ (raised by the roots' assembly, fact1_[side0_ - 1], on the
  // caller's stream), then raises rflag_[2 + k] for k_root_solve; ev_join_ (recorded after it) joins
  // the host-side users (status, fact_seconds, a factorisation no solve followed)
  bool root_async_ = false, root_pending_ = false, untimed_ = false;
  bool asm_side_ = false, side_phase_ = false;  // the roots' assembly tiles on side_ too; run_fact is enqueuing side_'s part
  size_t side0_ = 0;
  int nroot_side_ = 0, repoch_ = 0;
  bool side_tree_ = false;  // some side root is solved by its k_fwd_tree task (tside_), not k_root_solve
  DBuf<int32_t> rflag_;
  DBuf<uint8_t> tside_;
  hipStream_t side_ = nullptr;
  hipEvent_t ev_join_ = nullptr;
  // assembly
  DBuf<int32_t> g_ptr_;
  DBuf<BigChildRec> brec_;
  DBuf<int64_t> g_src_, g_chunk_, chunk_ids_;
  DBuf<int32_t> g_src32_;
  DBuf<SymbolicPlan::AsmTile> atiles_;
  DBuf<double> minv_, fscratch_, gpart_;
  // batched leaf columns (SymbolicPlan::lb): W, pivots, member tables, per-level launch lists
  DBuf<double> lbW_, lbd_, lbpart_;
  DBuf<int32_t> lbmem_, lbgid_, lbwrow_, lbgpos_, lbxrow_;
  DBuf<int64_t> lbcs_, lbce_, lbwbase_, lbpoff_;
  DBuf<SymbolicPlan::LBGroup> lbg_;
  std::vector<std::vector<int>> lb_at_level_;
  void lb_syrk(int g, hipStream_t s);
  // factorisation tree (k_fact_tree): fronts in topological order, their tree children, flags
  // (per-factorisation epoch), ticket counters (reset by the launch's last workgroup)
  int nftree_ = 0, fepoch_ = 0;
  DBuf<int32_t> ft_order_, ft_dptr_, ft_dep_, fflags_, fcnt_;
  DBuf<int64_t> fdbg_, ab_first_, ab_loff_, fold_poff_, fold_row0_;
  DBuf<int32_t> ab_src0_, ab_src1_, ab_k_, ab_f0_, ab_wrc_, fold_bptr_, fold_bat_, fold_plen_, fold_rmax_, fold_lmax_;
  DBuf<FoldStart> fstart_;
  DBuf<int32_t> fold_help_;
  DBuf<FoldHelp> fhelp_;
  DBuf<double> fimg_;
  DBuf<uint16_t> fimg_dst_;
  int nfhelp_ = 0;  // fold helper tickets (k_fact_tree: before the fronts')
  DBuf<uint8_t> absorb_, fold_pk_;
  DBuf<int32_t> mc_ptr_;
  DBuf<uint32_t> fold_prod_, fold_chead_;
  // big fronts as one task graph per launch (k_big_dag)
  DBuf<int32_t> dag_tasks_;  // DagTask (4 int32) per task of every DAG launch, in launch order
  DBuf<int32_t> dag_dptr_;   // per task: its first dependency in dag_dlist_ (launch-local tickets), + end
  DBuf<int32_t> dag_dlist_;
  DBuf<int32_t> dag_flags_;  // per task: the epoch of the factorisation that completed it
  DBuf<int32_t> dag_cnt_;    // ticket + done counters (reset by the last workgroup out)
  DBuf<double> dag_m_;       // M_K blocks per (big front, panel)
  DBuf<int64_t> dag_mslot_;  // per front: its first panel's slot in dag_m_
  int cepoch_ = 0;
  int dag_grid_ = 256;
  DBuf<int64_t> dag_dbg_;          // MADIPM_DAG_DEBUG: 4 stamps per task
  std::vector<int32_t> dag_kind_;  // (its host copy of the task words)
  void dag_debug_dump(hipStream_t s, const Launch& L);
  DBuf<double> upsum_;    // k_big_upd128 split K on launches of few tiles: its partial products
  DBuf<int32_t> uptick_;  // its per-tile tickets (reset by each tile's last part)
  // status
  DBuf<LDLStatus> status_;
  LDLStatus* h_status_ = nullptr;
  LDLStatus* st_ = nullptr;    // status in use: status_ or the caller's (external_status)
  LDLStatus* h_st_ = nullptr;  // its host copy
  bool ext_status_ = false;
  bool inertia_stale_ = false;  // lazy_inertia: npos / nneg / nzero not counted for the current factor

  // ---- solves (ldl_solve.hip)
  std::vector<SolveLevel> slev1_, slev2_;  // per level, leaves first
  void fwd_levels(const std::vector<SolveLevel>& V, int phase, double* b, hipStream_t s);
  void bwd_levels(const std::vector<SolveLevel>& V, int phase, double* b, hipStream_t s);
  void lb_fwd(const double* b, hipStream_t s);
  void lb_bwd(int g, double* b, hipStream_t s);
  DBuf<double> xi_, uvec_, vwork_;
  // multi-right-hand-side solve: every phase-1 front by level (LaunchPlan::mlev), and MULTI_W columns of the
  // internal and the update vector, allocated by the first solve_multi_async
  std::vector<SolveLevel> mlev_;
  DBuf<double> xim_, uvm_;
  // its big fronts' multi-column pass (§13k): MULTI_W columns of the hand-off words (epoch-tagged like xll_, its
  // own buffer), of vwork_ and of bpart_, allocated by the first such pass
  DBuf<uint64_t> xllm_;
  DBuf<double> vwm_, bpm_;
  // tree solves (k_fwd_tree / k_bwd_tree): the phase-1 fronts solved by ONE dependency-driven launch
  // per direction (topological ticket order, forward dependencies = tree children, backward = tree
  // parent), between the level-0 launches and the remaining levels
  int ntree_ = 0, tree_lds_ = 0;
  double tree_bytes_ = 0, tree_flops_ = 0, tree_alg_ = 0;
  DBuf<int32_t> tc_ptr_, tc_list_, tdep_ptr_, tdep_, tpar_, tflags_;
  DBuf<uint8_t> trootbwd_;  // per forward task: an elimination-tree root solved backward by k_fwd_tree
  int nroot_task_ = 0, root_lds_ = 0;  // tree-solve tasks of big etree roots (last, own forward launch)
  RootArgs rargs_{};                   // their fronts' shapes, passed by value to k_root_solve
  DBuf<uint8_t> tchunk_;    // per front: tree solves stream its panel in chunks (fwd_med_front / bwd_med_front)
  int ntask_ = 0;         // tree-solve tasks (one per tree front)
  int64_t nsleaf_ = 0;    // micro leaves solved from leaf records by the flat leaf launches
  double leaf_bytes_ = 0, leaf_flops_ = 0, leaf_alg_ = 0;  // the flat leaf launches (per direction)
  DBuf<SolveLeaf> tleaf_;
  DBuf<int2> tlrow_;
  DBuf<int64_t> tdbg_;
  DBuf<double> gbuf_;
  // big-front task queues (k_fwd_big / k_bwd_big)
  DBuf<uint64_t> xll_;
  DBuf<int32_t> tasks_, flags_, flag_off_, counters_, bp_off_;
  DBuf<double> bpart_;
  int epoch_ = 0;

  // ---- sharding and timing
  Comm* comm_ = nullptr;
  int64_t xg_off_ = 0;  // (top front, 256-row chunk) pairs of the external forward gather
  int nxg_ = 0;
  DBuf<int64_t> xoff_, sx_ptr_, sx_src_;
  DBuf<double> xch_;
  DBuf<double> xpack_;     // sharded: packed top-front lower triangles (+ status slots), all-reduced
  DBuf<int64_t> topcol_;   // per top-front column: arena offset, packed offset, length
  int ntopcol_ = 0;
  int64_t xpack_tri_ = 0;
  DBuf<uint8_t> wout_, colmask_;
  // sharded solve: caller positions of every shard's subtree columns, nshards slices of gper_
  // (padding -1), and the gathered solution slices
  DBuf<int32_t> gidx_;
  DBuf<double> gsol_;
  int64_t gper_ = 0;
  // MADIPM_TREE_DEBUG: the stamps of a tree launch (k_fact_tree, k_fwd_tree), summarised on stderr
  void tree_debug_dump(hipStream_t s, const char* what, const int64_t* dbuf, int nt, const char* p1, const char* p2,
                       const char* p3, const char* p4, const char* p5, int stride);
  // live timing
  unsigned tmask_ = 0;
  std::vector<hipEvent_t> evs_;
  size_t ev_used_ = 0;
  struct Pending {
    int kind;
    size_t e0;
    double bytes, flops, alg;
  };
  std::vector<Pending> pend_;
  KernelStat kst_[KK_COUNT];
  bool t_begin(int kind, hipStream_t s);
  void t_end(int kind, hipStream_t s, double bytes, double alg, double flops);
};

// The shards of one sharded factorisation on ONE device (single process): the phases run shard by
// shard and the all-reduces are a device kernel over the shards' buffers (local_allreduce).  It runs
// the whole sharded data path of SURVEY §8 e on one GPU; across GPUs each process owns one
// LDLSolver shard with an RcclComm instead.
class ShardGroup : public LinSolver {
 public:
  ShardGroup(int nshards, int n, const int64_t* colptr, const int32_t* rowval, const SymbolicOptions& sopt,
             double pivot_tol, const int32_t* user_perm = nullptr);
  void factorize_async(const double* Kx, hipStream_t s) override;
  int status(hipStream_t s, bool sync = true) override;
  void solve_async(double* b, hipStream_t s) override;
  const SymbolicPlan& plan() const override { return sh_[0]->plan(); }
  void set_timing(unsigned mask) override { sh_[0]->set_timing(mask); }
  void kernel_stats(KernelStat out[]) override { sh_[0]->kernel_stats(out); }
  int n() const override { return sh_[0]->n(); }
  int64_t xch_fact() const override { return sh_[0]->xch_fact(); }
  int64_t xch_solve() const override { return sh_[0]->xch_solve(); }
  int64_t xch_gather() const override { return sh_[0]->xch_gather(); }
  double fact_seconds(hipStream_t s) override { return sh_[0]->fact_seconds(s); }
  LDLSolver& shard(int r) { return *sh_[r]; }
  int nshards() const { return (int)sh_.size(); }

 private:
  std::vector<std::unique_ptr<LDLSolver>> sh_;
  std::vector<DBuf<double>> rhs_;
};

// bufs[q][i] <- sum_{q' in order} bufs[q'][i] for every q (q = 0..nbuf-1, nbuf <= 16)
void local_allreduce(double* const* bufs, int nbuf, int64_t n, hipStream_t s);

}  // namespace madipm
