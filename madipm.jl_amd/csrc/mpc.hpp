// Native Mehrotra predictor-corrector driver (restates MadIPM's `mpc!`, src/solver.jl:332-360)
// on top of the HIP LDL^T and the fused IPM vector kernels.  All vectors stay in HBM; scalar
// reductions land in a device-resident state block; the host reads ONE small block per iteration.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/madipm_hip.h"
#include "common.hpp"
#include "ldl.hpp"

namespace madipm {

struct Csr {
  int64_t* rp = nullptr;
  int32_t* ci = nullptr;
  double* v = nullptr;
};

// Device-resident scalars (one struct, copied to host once per iteration).
struct DevState {
  double mu, mu_curr, mu_aff;
  double alpha_p, alpha_d;            // final step
  double alpha_aff_p, alpha_aff_d;    // predictor (tau = 1)
  double a_xl, a_xu, a_zl, a_zu;      // last ratio test pieces
  double obj_val;
  double inf_pr_raw, inf_du_raw, inf_compl_raw, dobj;
  double res_ratio;                   // last solve_system! residual ratio
  double max_res_ratio;               // max over the iteration's solves
  double dx_inf;                      // ||primal(d)||_inf (print_iter)
  double delta_x, delta_s, delta_x2, delta_s2;  // init_starting_point! shifts
  double init_viol;                   // init assertion violations
  int32_t i_xl, i_xu, i_zl, i_zu;     // argmin indices (-1 = init element)
  int32_t nan_flag;
  int32_t pad;
  LDLStatus ldl_status;  // the linear solver's status (external_status): one read-back per iteration
};

struct QPHost;       // host copy of the problem (qp_model.hpp)
struct DV;           // the kernels' view of the device vectors (mpc_kernels.hpp)
struct UpdatePlan;   // index plans of the value refresh, built by prepare_update (mpc_kernels.hpp)
struct DevUpdate;    // staging, start vectors and sum-order lists of the device route (mpc.hip)
struct WarmStart;    // the warm point and its scratch, on the device (mpc.hip)
struct PostSolve;    // everything adjoint, tangent and polish keep between calls (mpc_post.hip)
struct SensView;     // the scratch one tangent / adjoint call runs on: the single calls' or the batch's (mpc_post.hip)
struct PostSolveDelete {
  void operator()(PostSolve* p) const;
};

class MPCSolver {
 public:
  // comm != nullptr (size > 1): this process holds shard comm->rank of the sharded factorisation
  MPCSolver(const madipm_qp& qp, const madipm_options& opt, Comm* comm = nullptr);
  ~MPCSolver();
  int solve(madipm_stats* stats);
  void initialize_public();  // initialize! alone (so that callers can time the MPC loop only)
  void set_max_iter(int k) { opt_.max_iter = k; }
  void get_solution(double* x, double* y, double* zl, double* zu, double* cons);
  const std::vector<madipm_iter_trace>& trace() const { return trace_; }
  LinSolver& ldl() { return *ldl_; }
  hipStream_t stream() const { return stream_; }
  int spmv_group() const { return spmv_g_; }  // lanes per row of the SpMV kernels (heuristic or MADIPM_SPMV_G)
  // New numbers for the same pattern (madipm_solver_prepare_update / _update / _counters): prepare_update
  // builds the refresh plan once (a solver that never calls it pays nothing); update installs the data
  // without touching the linear solver and leaves the stream idle.
  void prepare_update(const madipm_qp& qp);
  void update(const madipm_qp_update& u);
  // The device route (madipm_solver_update_device / _get_solution_device / _get_data): update_device reads
  // DEVICE arrays after the work enqueued on `caller`, recomputes numeric_host's results with kernels and
  // leaves the stream idle; its first call allocates everything it needs.  get_solution_device writes the
  // un-scaled solution to device arrays without blocking the host; work enqueued on `caller` afterwards
  // sees it.  get_data copies the raw numbers the solver holds to host arrays.
  void update_device(const madipm_qp_update& u, hipStream_t caller);
  void get_solution_device(double* x, double* y, double* zl, double* zu, double* cons, hipStream_t caller);
  void get_data(double* c, double* c0, double* Hvals, double* Avals, double* lcon, double* ucon, double* lvar,
                double* uvar, double* x0, double* y0);
  // Warm start (madipm_solver_set_warm_start / _device / _warm_start_last / _clear_warm_start / _warm_info):
  // a point (x, y, zl, zu) of the public space, any block absent (null), that initialize() blends with the
  // cold start.  The first call that sets one allocates its device copy; a solver that never sets one, or
  // cleared it, initializes exactly as before.  device: the pointers are device arrays produced on `caller`.
  void set_warm_start(const double* x, const double* y, const double* zl, const double* zu, double weight,
                      bool device, hipStream_t caller);
  void warm_start_last(double weight);
  void clear_warm_start();
  void warm_info(int32_t* active, double* weight, int64_t* n_warm_inits) const;
  // Adjoint gradients (madipm_solver_adjoint / _adjoint_device / _adjoint_info): given
  // gx = dl/dx* at the point of the last successful solve, the gradients of l with respect to the problem
  // data the caller asks for (non-null fields of `out`).  Factorises the K2 system at that point once per
  // solve; further calls on the same point reuse the factor.  device: gx and the outputs are device arrays
  // produced / consumed on `caller`.  Changes nothing a later initialize / solve / warm_start_last reads.
  void adjoint(const double* gx, const madipm_qp_gradients& out, bool device, hipStream_t caller);
  // The same for a loss of all five solution blocks (madipm_solver_adjoint_full / _full_device):
  // non-null fields of `g` are the cotangents of x, y, zl, zu and A x.  `name`: the entry point, for the
  // messages.  With g.x alone this is adjoint()'s path, bit for bit.
  void adjoint(const madipm_qp_cotangents& g, const madipm_qp_gradients& out, bool device, hipStream_t caller,
               const char* name);
  void adjoint_info(int64_t* n_adjoints, int64_t* n_adjoint_factorizations, double* last_residual);
  // Forward mode (madipm_solver_tangent / _tangent_device / _tangent_info): given a direction of
  // the data (non-null fields of `d`), the directional derivative of the solution blocks the caller asks for
  // (non-null fields of `out`) at the point of the last successful solve.  Shares the adjoint's factor (one
  // factorisation per solved point serves both), refinement and residual; device and `caller` as there.
  void tangent(const madipm_qp_directions& d, const madipm_qp_point_tangents& out, bool device, hipStream_t caller);
  void tangent_info(int64_t* n_tangents, double* last_residual);
  // The exact active-set solve after the interior-point method (madipm_solver_polish / _polish_device /
  // _polish_info).  av / ar: the supplied set (both null: the guess); device: every pointer but
  // `info` is a device pointer, ordered against `caller` as in adjoint().
  void polish(const madipm_polish_opts& o, const int8_t* av, const int8_t* ar, const madipm_polish_out& out,
              madipm_polish_info* info, bool device, hipStream_t caller);
  void polish_info(madipm_polish_info* info) const;
  // The active-set solve of the data the solver holds, without an interior-point end point
  // (madipm_solver_active_set_solve / _device / _active_set_info): rounds of the polish's
  // factor, solves and verdict from a start that reads nothing of the iterate, the set repaired between
  // them.  av / ar: the starting set (both null: the kept set); device and `caller` as in polish().
  void active_set_solve(const madipm_active_set_opts& o, const int8_t* av, const int8_t* ar,
                        const madipm_polish_out& out, madipm_active_set_info* info, bool device, hipStream_t caller);
  void active_set_info(madipm_active_set_info* info) const;
  // tangent() and adjoint() at the polished point (madipm_solver_tangent_polished / _adjoint_polished / _device /
  // _polished_sens_info): the exact derivatives of the face the last polish() of this solved point
  // ended POLISHED on.  They solve with the polish's factor (restored from the kept set when an adjoint or a
  // tangent took the LDL^T since) and read the polish's scratch point; arguments and `caller` as there.
  void tangent_polished(const madipm_qp_directions& d, const madipm_qp_point_tangents& out, bool device,
                        hipStream_t caller);
  void adjoint_polished(const madipm_qp_cotangents& g, const madipm_qp_gradients& out, bool device,
                        hipStream_t caller);
  void polished_sens_info(int64_t* n_tangents, int64_t* n_adjoints, int64_t* n_factorizations, double* last_residual);
  // k tangents / adjoints of one point per call (madipm_solver_tangent_batch / _adjoint_batch / _device /
  // _sens_batch_info): every non-null block holds k vectors back to back.  At the end point the
  // columns run in chunks of sens_batch_cols() through the single calls' kernels and host path, so each column
  // has the single call's bits; polished: one tangent_polished / adjoint_polished per column.
  static int sens_batch_cols();
  void tangent_batch(int32_t k, const madipm_qp_directions& d, const madipm_qp_point_tangents& out, bool polished,
                     bool device, hipStream_t caller);
  void adjoint_batch(int32_t k, const madipm_qp_cotangents& g, const madipm_qp_gradients& out, bool polished,
                     bool device, hipStream_t caller);
  void sens_batch_info(int64_t* n_batches, int64_t* n_columns, int64_t* n_chunks) const;
  // on: the batched end-point sensitivities solve every chunk with LinSolver::solve_multi_async:
  // a row's bits then do not depend on k, and differ from the single calls' within the formulas' tolerance
  void set_multi_solve(bool on) { multi_solve_ = on; }
  const MultiStat& multi_solve_stat() const { return ldl_->multi_stat(); }
  const MultiBigStat& multi_big_stat() const { return ldl_->multi_big_stat(); }
  int64_t n_analyses() const { return n_analyses_; }
  int64_t n_updates() const { return n_updates_; }
  double last_update_s() const { return last_update_s_; }

 private:
  void setup_host(const madipm_qp& qp);
  void build_device_route();
  WarmStart& warm_buffers();
  void warm_blend();
  void refresh_host_mirrors();
  const double* device_con_scale();
  DV view() const;
  // k_cons of a scaled point; k_cons (cons given) + k_unscale of the iterate: get_solution's values on the device
  void cons_rows(const double* xs, double* ax);
  void unscale_point(const double* cscale, double* ax, double* x, double* y, double* zl, double* zu, double* cons);
  // shared by the post-solve calls (mpc_post.hip): the refusals, the state, the regularised factorisation
  // trials (enqueue(dw, dc) writes the diagonal and enqueues one factorisation), the adjoint's and tangent's
  // factor of the point and their refined solve
  friend struct PostSolve;
  void sens_refuse(const std::string& who) const;
  PostSolve& post_state();
  template <class Enqueue>
  bool factor_trials(Enqueue&& enqueue);
  void sens_factor(const std::string& who);
  // (of the kc columns of a chunk on the scratch V names, §13i; resid[0]: the largest ratio of the call so far),
  // and the one implementation of tangent / tangent_batch and of adjoint / adjoint_batch: k columns in chunks
  void sens_solve(const SensView& V, int kc, double* resid, bool first_chunk);
  int64_t tangent_cols(const std::string& who, int64_t k, bool batch, bool polished, const madipm_qp_directions& d,
                       const madipm_qp_point_tangents& out, bool device, hipStream_t caller);
  int64_t adjoint_cols(const std::string& who, int64_t k, bool batch, bool polished, bool need_gx,
                       const madipm_qp_cotangents& g, const madipm_qp_gradients& out, bool device, hipStream_t caller);
  // the polished sensitivities': the refusals, the polish's factor, the masked solves
  void polished_refuse(const std::string& who) const;
  void polished_factor(const std::string& who);
  void polished_solve();
  // the polish's and the active-set solve's buffers and raw bounds (device_bounds: gathered from the device
  // route's staging, no host copy); the tag of the polish factor the LDL^T holds
  void polish_buffers(bool device_bounds);
  bool device_raw_bounds(const double* (&raw)[4]) const;  // false: the host's copies are the newer ones
  bool polish_factor_held() const;
  void polish_factor_tag(double sigma);
  bool active_set_point() const;
  std::unique_ptr<LinSolver> make_linsolver(int n, const int64_t* cp, const int32_t* ri, const SymbolicOptions& so);
  void initialize();
  void init_starting_point();
  // amode >= 0: k_alpha of that mode runs after the residual and is finalised with it (one k_final less)
  // mu_nb > 0: the corrector's k_rhs finalises the barrier update from k_mu's mu_nb partials
  void solve_system(int mode, double mu, int reset = 0, int amode = -1, double atau = 1.0, int mu_nb = 0);
  void gondzio();
  // predictor + corrector directions (speculated before the status read); fuse_step: the corrector's
  // solve also runs update_step_size!'s step test (only when nothing changes d in between: no Gondzio)
  void directions(bool redo, bool fuse_step);
  void step_size(bool fused);
  void launch_reduce_final(int kind, int nvals, int amode = -1, int nb_eval = 0, LDLStatus* rs = nullptr,
                           bool publish = false);
  int step_alpha_mode(double& tau) const;
  void read_state();  // enqueue the publication of the device state to the host mirror
  void wait_state();  // wait (host spin) until the last publication has landed
  void kkt_diag(double dw, double dc);
  // build_kkt!: diagonal (+ K2.5 scaling / normal-matrix assembly) -> values handed to the LDL^T
  void assemble_kkt(double dw, double dc, bool diag_done = false);
  const double* kvals() const;
  // MadNLP.solve!(kkt, d) after the right-hand side is in d_: reduced solve in the chosen formulation
  void kkt_solve();
  void factor_enqueue(double dw, double dc);
  void timed_factorize();
  LDLStatus* fact_reset() const;
  LDLStatus* take_fact_end();
  int blocks(int64_t n) const;
  int spmv_blocks(int64_t rows) const;

  madipm_options opt_{};
  hipStream_t stream_ = nullptr;
  std::unique_ptr<QPHost> H_;
  std::unique_ptr<LinSolver> ldl_;
  bool multi_solve_ = false;  // set_multi_solve
  Comm* comm_ = nullptr;
  // sizes
  int nx_ = 0, ns_ = 0, n_ = 0, m_ = 0, nlb_ = 0, nub_ = 0;
  int64_t nnzK_ = 0, L_ = 0;  // L_ = unreduced vector length
  // device vectors
  DBuf<double> x_, xl_, xu_, zl_, zu_, f_, jacl_, c_, y_, rhs_, pr_diag_, l_diag_, u_diag_, l_lower_, u_lower_;
  DBuf<double> d_, p_, corr_lb_, corr_ub_, dsave_;
  DBuf<double> Kx_, Hdiag_, cs_, gfix_, cfix_, lo_full_, hi_full_;
  DBuf<int64_t> diag_pos_;
  DBuf<int32_t> ind_lb_, ind_ub_, lbpos_, ubpos_;
  DBuf<uint8_t> fixed_;
  DBuf<int64_t> Hrp_, Jrp_, JTrp_;
  DBuf<int32_t> Hci_, Jci_, JTci_;
  DBuf<double> Hv_, Jv_, JTv_;
  DBuf<double> part_;
  // KKT formulation (0 K2, 1 K2.5, 2 normal equations)
  int kkt_ = 0;
  int spmv_g_ = 8;  // lanes per row in the SpMV kernels
  static constexpr int kFinDbg = 4096;
  DBuf<int64_t> fdbg_;  // MADIPM_FINAL_DEBUG: k_final stamps (ring of kFinDbg launches)
  int64_t fdbg_n_ = 0;
  int maxb_ = 2048;  // partial-reduction blocks per producer launch (<= MAXB; r3 / r5: 1024 or 512 measured slower)
  DBuf<double> sk_, K0_, Dinv_, bufm_, Cx_;
  DBuf<int32_t> Krow_, Kcol_, cprod_;
  DBuf<int64_t> cpp_;
  int64_t nnzC_ = 0;
  DBuf<DevState> st_;
  DevState* hst_ = nullptr;          // host mirror of st_ (coherent pinned memory, written by k_publish)
  uint32_t* hseq_ = nullptr;         // publication counter beside it
  uint32_t pub_seq_ = 0;
  bool publish_next_ = false;        // the next solve_system's k_rhs publishes the state
  bool fact_end_pending_ = false;    // the next solve_system's k_rhs stamps the factorisation's end
  // host scalars (MPCSolver fields of src/structure.jl:62-76)
  double del_w_ = 0, del_c_ = 0, norm_b_ = 0, norm_c_ = 0, best_compl_ = 0, obj_scale_ = 1, c0s_ = 0;
  bool eval_pending_ = false;  // k_eval's objective partials await the next FIN_TERM
  double adapt_dp_ = 0, adapt_dd_ = 0, adapt_dmin_ = 0;
  int status_ = 0, k_ = 0;
  int exception_ = 0;  // MADIPM_EXC_* of the last solve (what solve!'s catch-all caught)
  bool initialized_ = false;
  double inf_pr_ = 0, inf_du_ = 0, inf_compl_ = 0;
  double spec_near_ = 10.0;  // MADIPM_SPEC_NEAR: hold the speculative factorisation when residuals <= this x tol (0: never)
  double t_init_ = 0, t_total_ = 0, t_linsol_ = 0;
  std::vector<madipm_iter_trace> trace_;
  double fs0_ = 0;  // device factorisation seconds at initialize! (cnt.linear_solver_time origin)
  DevState last_{};                // the state of the last termination test
  std::unique_ptr<UpdatePlan> plan_;  // null until prepare_update
  std::unique_ptr<DevUpdate> dev_;     // null until the first update_device
  int host_stale_ = 0;                 // raw fields whose host mirror is older than the device staging (bit mask)
  bool dev_raw_stale_ = false;         // a host update ran since the device staging of c / bounds / x0 / y0 was written
  bool start_on_device_ = false;       // initialize() restarts from dev_'s start vectors (last update: device)
  bool cscale_host_stale_ = false;     // QPHost::con_scale is older than the plan's device con_scale
  bool cscale_dev_ok_ = false;         // the plan's device con_scale has been written by an update
  DBuf<double> sol_ax_, sol_cs_;       // get_solution_device: constraint values; con_scale when no update wrote it
  StreamHandoff sol_sync_;
  std::unique_ptr<WarmStart> warm_;     // null until a warm point is set
  int64_t n_warm_inits_ = 0;           // initialize() calls that blended
  bool solved_ = false;                // a solve has run (warm_start_last needs its point)
  std::unique_ptr<PostSolve, PostSolveDelete> post_;  // null until the first adjoint, tangent or polish
  bool point_ok_ = false;              // the iterate is the end point of a completed solve
  int64_t n_solves_ = 0;               // completed solves (the adjoint's factor belongs to one of them)
  int64_t solve_updates_ = 0;          // n_updates_ at the end of the last solve
  int64_t n_analyses_ = 0, n_updates_ = 0;
  int64_t n_inits_ = 0, n_factor_calls_ = 0;  // initialize() calls; factorisations enqueued (the post-solve factors' tags)
  double last_update_s_ = 0;
};

// update_step! on caller-given vectors (madipm_update_step); v = the 10 device pointers in header order
void update_step_standalone(int rule, double tau_param, double mu, int nlb, int nub, const double* const* v,
                            madipm_step_result* out, hipStream_t s);

}  // namespace madipm
