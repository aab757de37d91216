/*
 * madipm_hip.h — C-ABI of libmadipm_hip.so, the MI355X (gfx950) hot path of MadIPM's
 * Mehrotra predictor-corrector (reference: klamike/MadIPM.jl v0.1.2).
 *
 * Conventions: 0-based indices, Float64 values, int32 row indices, int64 column pointers /
 * nonzero counts.  Every function returns 0 on success, a negative code on error (text in
 * madipm_last_error(), thread-local); madipm_ldl_factorize additionally returns k+1 > 0 when
 * pivot k (internal order) is zero / non-finite, which maps to MadIPM.is_factorized == false.
 * Device pointers are plain hipMalloc'd (or torch / AMDGPU.jl ROCArray) addresses; `stream` is a
 * hipStream_t (NULL = default stream).  No exceptions cross this boundary.
 *
 * Which reference interface each entry point replaces is cited per function (file:line relative
 * to the reference root).  INTEGRATION.md shows the Julia `ccall` binding a maintainer would add.
 */
#ifndef MADIPM_HIP_H
#define MADIPM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* madipm_stream_t; /* hipStream_t */

/* ------------------------------------------------------------------ library */
int madipm_version(void);                 /* MAJOR*10000 + MINOR*100 + PATCH */
const char* madipm_last_error(void);
int madipm_device_count(void);            /* hipGetDeviceCount; 0 when no GPU is present */
int madipm_set_device(int32_t dev);       /* hipSetDevice for the calling thread (one process per GPU),
                                            and the runtime's one-off device set-up done
                                            (context, first stream) */

/* ------------------------------------------------------------------ symbolic analysis (host)
 * Replaces the symbolic phase run by the linear-solver constructor `linear_solver(aug_com; opt)`
 * (src/KKT/normalkkt.jl:113-115; SparseKKTSystem constructor in MadNLP [EXT]) — SURVEY §8 a12. */
typedef struct madipm_ldl_opts {
  int32_t ordering;        /* 0 natural, 1 AMD, 2 user permutation, 3 nested dissection,
                              4 auto = AMD and ND, fewer flops wins (default) */
  double dense_alpha;      /* AMD dense-node threshold factor (default 10) */
  int32_t relax;           /* relaxed supernode amalgamation (default 1) */
  int32_t small_front_max; /* fronts with <= this many rows are factorised in LDS (default 128; up to 192 with packed LDS storage) */
  double pivot_tol;        /* |d| <= pivot_tol  =>  pivot failure (default 0: only 0 / NaN / Inf) */
  int32_t nshards;         /* > 1: subtree-sharded factorisation with nshards shards on THIS device
                              (single process, local all-reduce; SURVEY §8 e); default 1.  Across
                              GPUs use madipm_solver_create_dist / madipm_ldl_analyze_shard. */
  int32_t cholesky;        /* 1: Cholesky semantics — the matrix must be SPD, any pivot that is not > 0
                              fails the factorisation (is_factorized == false): the cuDSS CHOLESKY
                              configuration the reference pairs with NormalKKTSystem
                              (test/test_gpu.jl:11); default 0 (quasi-definite LDL^T)  [ABI 0.2] */
} madipm_ldl_opts;

typedef struct madipm_ldl_info {
  int64_t n;
  int64_t nnzK;            /* entries of the lower CSC input */
  int64_t nnzL;            /* exact nnz(L) incl. diagonal */
  int64_t nnzL_stored;     /* lower-trapezoid entries stored by the supernodes (incl. relaxed zeros) */
  double flops;            /* factorisation flops, sum_j (c_j-1)(c_j+2) */
  int32_t nsuper;          /* fronts */
  int32_t nlevels;         /* levels of the front tree (launch schedule depth) */
  int32_t max_front;       /* largest front order */
  int32_t nbig;            /* fronts handled by the global-memory blocked path */
  int64_t arena_bytes;     /* device bytes for factor + update blocks */
  int32_t lb_groups;       /* batched leaf-column groups (each absorbed by one SYRK into its parent) */
  int32_t lb_members;      /* single-column leaf fronts in those groups */
  int32_t fold_fronts;     /* tree fronts that fold their micro leaves (LDS product lists) */
  int32_t fold_leaves;     /* micro leaves folded by them */
  int64_t xch_fact;        /* sharded: doubles all-reduced per factorisation (top-front lower triangles
                              + 4 status slots per shard); 0 unsharded */
  int64_t xch_solve;       /* sharded: doubles all-reduced per solve (the top fronts' forward right-hand
                              sides); 0 unsharded */
  int64_t xch_gather;      /* sharded: doubles of the per-solve in-place all-gather of the shards'
                              subtree solution slices (nshards slices); 0 unsharded */
  int32_t tree_fronts;     /* fronts factorised by the dependency-driven tree launch (k_fact_tree) [ABI 0.2] */
  int32_t tree_medium;     /* of which medium fronts (192 < r <= 256: factorised in HBM, one 64-column
                              panel in LDS at a time) [ABI 0.2] */
  int32_t root_tail_async; /* 1: the elimination-tree roots after the tree launch are assembled and
                              factorised on a side stream, beside the next solve's forward leaves and
                              tree fronts (MADIPM_ROOT_ASYNC, default on) [ABI 0.2.3] */
  int32_t pad_;
} madipm_ldl_info;

void madipm_ldl_default_opts(madipm_ldl_opts* opts);

typedef struct madipm_symbolic* madipm_symbolic_t;
/* colptr[n+1] (int64), rowval[nnz] (int32): lower triangle (row >= col), unique entries. */
int madipm_symbolic_analyze(int32_t n, const int64_t* colptr, const int32_t* rowval,
                            const madipm_ldl_opts* opts, const int32_t* user_perm,
                            madipm_symbolic_t* out);
int madipm_symbolic_info(madipm_symbolic_t sym, madipm_ldl_info* info);
int madipm_symbolic_perm(madipm_symbolic_t sym, int32_t* perm /* n */);
/* first[nsuper+1], parent[nsuper], nrows[nsuper] (any may be NULL) */
int madipm_symbolic_supernodes(madipm_symbolic_t sym, int32_t* first, int32_t* parent, int32_t* nrows);
void madipm_symbolic_destroy(madipm_symbolic_t sym);
/* symbolic analysis of one shard of a subtree-sharded factorisation (see "subtree sharding" below),
 * and the partition: owner[nsuper] (-1 top, else shard) and the cost-model totals */
int madipm_symbolic_analyze_shard(int32_t n, const int64_t* colptr, const int32_t* rowval,
                                  const madipm_ldl_opts* opts, int32_t nshards, int32_t shard,
                                  const int32_t* user_perm, madipm_symbolic_t* out);
int madipm_symbolic_shard_info(madipm_symbolic_t sym, int32_t* owner, double* top_cost, double* shard_cost_max,
                               double* shard_cost_sum);

/* ------------------------------------------------------------------ LDL^T linear solver (device)
 * The MadNLP.AbstractLinearSolver the reference plugs in through `linear_solver=`
 * (src/utils.jl:72, src/structure.jl:117-123): LDLSolver (LDLFactorizations), CUDSSSolver with
 * cudss_algorithm=MadNLP.LDL (scripts/benchmarks_gpu.jl:41-42), Ma57Solver
 * (scripts/benchmarks_cpu.jl:36).  SURVEY §8 a11/a12/a14, boundary §8(b). */
typedef struct madipm_ldl* madipm_ldl_t;
/* Constructor `LS(aug_com; opt)`: symbolic analysis + device upload (src/KKT/normalkkt.jl:113-115). */
int madipm_ldl_analyze(int32_t n, const int64_t* colptr, const int32_t* rowval,
                       const madipm_ldl_opts* opts, const int32_t* user_perm, madipm_ldl_t* out);
int madipm_ldl_get_info(madipm_ldl_t ls, madipm_ldl_info* info);
/* MadNLP.factorize!(ls) (called via factorize_wrapper!, src/linear_solver.jl:10, src/solver.jl:21).
 * d_nzval: device values in the CSC order given to madipm_ldl_analyze.  Synchronises `stream`;
 * returns 0, or k+1 for the first failing pivot k (=> madipm_ldl_is_factorized() == 0). */
int madipm_ldl_factorize(madipm_ldl_t ls, const double* d_nzval, madipm_stream_t stream);
/* Asynchronous variant; the outcome is read by madipm_ldl_is_factorized / madipm_ldl_inertia. */
int madipm_ldl_factorize_async(madipm_ldl_t ls, const double* d_nzval, madipm_stream_t stream);
/* MadIPM.is_factorized(ls) (src/utils.jl:54-62): 1 when the last factorisation succeeded. */
int madipm_ldl_is_factorized(madipm_ldl_t ls);
/* MadNLP.solve!(ls, x) (src/linear_solver.jl:26 via MadNLP.solve!(kkt, d)): in place, nrhs
 * columns of length n stored contiguously. */
int madipm_ldl_solve(madipm_ldl_t ls, double* d_x, int32_t nrhs, madipm_stream_t stream);
/* MadNLP.inertia(ls) -> (pos, zero, neg); MadNLP.is_inertia(ls) is true. */
int madipm_ldl_inertia(madipm_ldl_t ls, int32_t* pos, int32_t* zero, int32_t* neg);
/* Diagonal D of the last factorisation, internal (permuted) order, copied to host memory. */
int madipm_ldl_get_d(madipm_ldl_t ls, double* h_d);
int madipm_ldl_perm(madipm_ldl_t ls, int32_t* perm /* n */);
void madipm_ldl_destroy(madipm_ldl_t ls);

/* ------------------------------------------------------------------ subtree sharding (SURVEY §8 e)
 * The north star's multi-GPU mode: the front tree is cut into independent subtrees dealt to
 * `nshards` shards (one per GPU) plus their common ancestors ("top" fronts), which every shard
 * factorises redundantly after ONE all-reduce (sum) of the top fronts' external contributions.
 * A solve needs two more: an all-reduce of the top fronts' forward right-hand sides and an all-gather
 * of the shards' subtree solution slices (the top solution is computed redundantly on every shard).
 * No reference counterpart (the reference is single-device: cuDSS / LDLFactorizations); these entry
 * points let a host binding drive the phases with its own collective (e.g. Julia + RCCL.jl):
 *   factorize: phase 1 -> all-reduce(xbuf, xlen) -> phase 2
 *   solve:     phase 1 -> all-reduce(xbuf, xlen) -> phase 2 -> all-gather(xbuf, xlen) -> phase 3
 * The solve's phase 2 returns the gather buffer: nshards slices of xlen / nshards doubles, this
 * shard's slice (at shard * xlen / nshards) filled and the others zero, so an in-place all-gather
 * (madipm_comm_allgather, ncclAllGather) or a sum all-reduce of the whole buffer completes it.
 * Phase 3 scatters the other shards' slices into x (xbuf = NULL, xlen = 0).
 * Shards must be created with the same pattern and options; every shard computes the same cut. */
int madipm_ldl_analyze_shard(int32_t n, const int64_t* colptr, const int32_t* rowval, const madipm_ldl_opts* opts,
                             int32_t nshards, int32_t shard, const int32_t* user_perm, madipm_ldl_t* out);
int madipm_ldl_factorize_phase(madipm_ldl_t ls, int32_t phase /* 1 | 2 */, const double* d_nzval,
                               madipm_stream_t stream, double** xbuf, int64_t* xlen);
int madipm_ldl_solve_phase(madipm_ldl_t ls, int32_t phase /* 1 | 2 | 3 */, double* d_x, madipm_stream_t stream,
                           double** xbuf, int64_t* xlen);
/* owner[s] of every front (-1 top, else shard), and the partition's cost model totals */
int madipm_ldl_shard_info(madipm_ldl_t ls, int32_t* owner, double* top_cost, double* shard_cost_max,
                          double* shard_cost_sum);
/* sum of nbuf device buffers of length n, written back to all of them (single-process shards) */
int madipm_local_allreduce(double* const* d_bufs, int32_t nbuf, int64_t n, madipm_stream_t stream);

/* RCCL communicator (one process per GPU): rank 0 makes the 128-byte id, the host broadcasts it. */
typedef struct madipm_comm* madipm_comm_t;
int madipm_comm_unique_id(void* id128);
int madipm_comm_create(int32_t nranks, int32_t rank, const void* id128, madipm_comm_t* out);
/* Host-staged communicator: each all-reduce synchronises the stream, copies the buffer to pinned host
 * memory, calls fn(host_buf, n, ctx) (which must sum it across ranks in place and return 0) and
 * copies it back.  For testing the multi-process protocol where RCCL cannot run (ranks sharing a GPU). */
typedef int (*madipm_allreduce_fn)(double* host_buf, int64_t n, void* ctx);
int madipm_comm_create_host(int32_t nranks, int32_t rank, madipm_allreduce_fn fn, void* ctx, madipm_comm_t* out);
/* in-place fp64 sum over the communicator's ranks, ordered on `stream` */
int madipm_comm_allreduce(madipm_comm_t comm, double* d_buf, int64_t n, madipm_stream_t stream);
/* in-place all-gather of nranks slices of nper doubles (rank r's slice at d_buf + r * nper, the other
 * slices zero on entry; a host-staged communicator sums the whole buffer), ordered on `stream` */
int madipm_comm_allgather(madipm_comm_t comm, double* d_buf, int64_t nper, madipm_stream_t stream);
void madipm_comm_destroy(madipm_comm_t comm);

/* Live per-kernel timing (no reference counterpart; measurement for bench.py's roofline).
 * Bit k of `mask` records HIP events around every launch of kernel kind k on the launch stream
 * (kinds: 0 k_asm_chunks, 1 k_assemble, 2 k_tiny_factor, 3 k_small_factor, 4 k_big_diag,
 * 5 k_big_trsm, 6 k_big_update, 7 k_inertia, 8 k_fwd_small, 9 k_fwd_gather, 10 k_fwd_big,
 * 11 k_bwd_below, 12 k_bwd_big, 13 k_bwd_small, 14 k_fwd_tiny, 15 k_bwd_tiny, 16 k_lb_build,
 * 17 k_lb_syrk, 18 k_lb_gemv, 19 k_fwd_tree, 20 k_bwd_tree, 21 k_fact_tree, 22 k_asm_update,
 * 23 k_big_dag [ABI 0.2.2]).  Setting a mask clears the statistics. */
#define MADIPM_NKERNELS 24
typedef struct madipm_kstat {
  char name[32];
  int64_t launches;
  double time_ms;          /* summed event time of the launches */
  double bytes;            /* staging-traffic model of those launches (what the kernel moves) */
  double flops;            /* algorithmic flops of those launches */
  double alg_bytes;        /* SURVEY 8(d)'s algorithmic bytes of those launches: 8 nnzL + 12 nnzK of the
                              columns they factorise, 8 nnzL of the columns a solve launch substitutes */
} madipm_kstat;
int madipm_ldl_set_timing(madipm_ldl_t ls, uint32_t mask);
/* synchronises the recorded events; out[MADIPM_NKERNELS] */
int madipm_ldl_kernel_stats(madipm_ldl_t ls, madipm_kstat* out);

/* ------------------------------------------------------------------ array-type overrides
 * The ROCArray counterparts of the methods MadIPM's CUDA extension overrides so that MPCSolver
 * runs on device arrays (ext/MadIPMCUDAExt/cuda_wrapper.jl, MadIPMCUDAExt.jl).  Device pointers,
 * 0-based, int32 indices as the reference's CuSparseMatrix{Float64,Int32}; every sum has a fixed
 * order (bitwise reproducible), and transfer / assemble_normal_system follow the reference CPU
 * loops' order and rounding exactly.  Asynchronous on `stream` unless stated. */

/* MadNLP.transfer!(dest::CSC, src::COO, map) (cuda_wrapper.jl:4-24, used by build_kkt!/
 * compress_hessian! :26-30): dest .= 0; dest[map[k]] += src[k] for k = 0..nsrc-1, sources of one
 * entry summed in ascending k.  The plan is built once from the map (host or device pointer). */
typedef struct madipm_transfer* madipm_transfer_t;
int madipm_transfer_create(int64_t nsrc, const int64_t* map, int32_t map_on_device, int64_t ndest,
                           madipm_transfer_t* out);
int madipm_transfer(madipm_transfer_t t, double* d_dest, const double* d_src, madipm_stream_t stream);
void madipm_transfer_destroy(madipm_transfer_t t);

/* compress_jacobian!(::NormalKKTSystem) (normalkkt.jl:163-172, cuda_wrapper.jl:32-41):
 * AV[nnz-n_slack .. nnz-1] = -1 (in place), then ATnz[i] = AV[csr_map[i]] for i < nnz. */
int madipm_compress_jacobian(double* d_AV, int64_t nnz, int32_t n_slack, const int64_t* d_csr_map,
                             double* d_ATnz, madipm_stream_t stream);

/* MadIPMOperator(A::CuSparseMatrixCSR; transa, symmetric) (cuda_wrapper.jl:43-83) and its mul!
 * (:85-94).  A is m x n CSR (rowptr m+1, colval/nzval nnz; device).  symmetric != 0 (and nnz > 0):
 * the operator is mat = tril(A,-1) + A', copied at creation like the reference's `mat`;
 * otherwise the caller's arrays are read live at every apply ('T' through a transposed index plan
 * built at creation).  apply: y = alpha op(A) x + beta y (y is not read when beta == 0); y has
 * m rows for 'N' / symmetric, n for 'T'.  size reports size(A) and nnz(A) (Base.size, nnz). */
typedef struct madipm_spmv* madipm_spmv_t;
int madipm_spmv_create(int32_t m, int32_t n, int64_t nnz, const int32_t* d_rowptr, const int32_t* d_colval,
                       const double* d_nzval, char transa, int32_t symmetric, madipm_spmv_t* out);
int madipm_spmv_apply(madipm_spmv_t op, const double* d_x, double* d_y, double alpha, double beta,
                      madipm_stream_t stream);
int madipm_spmv_size(madipm_spmv_t op, int32_t* m, int32_t* n, int64_t* nnz);
void madipm_spmv_destroy(madipm_spmv_t op);

/* MadIPM.coo_to_csr(n_rows, n_cols, Ai, Aj, Ax) (src/utils.jl:158-201; GPU cuda_wrapper.jl:96-106),
 * device arrays, 0-based.  Entries are grouped by row in input order (utils.jl's counting sort);
 * sort_cols != 0 orders each row by column (ties in input order), the layout cuSPARSE produces.
 * Duplicates are kept, as in the reference.  rowptr: n_rows+1.  Synchronises `stream`.
 * An index outside [0, n_rows) x [0, n_cols) is an error (negative return; outputs invalid). */
int madipm_coo_to_csr(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t* d_Ai, const int32_t* d_Aj,
                      const double* d_Ax, int32_t* d_rowptr, int32_t* d_colval, double* d_nzval,
                      int32_t sort_cols, madipm_stream_t stream);

/* MadIPM.build_normal_system(n_rows, n_cols, Jtp, Jtj) (src/utils.jl:209-274; the GPU path runs it
 * on host copies too, normalkkt.jl:104): HOST arrays.  Pattern of tril(J J') for J in CSR:
 * column i of the lower CSC (Cp[n_rows+1], Cj) lists the rows j >= i sharing a column with row i,
 * ascending.  *nnz_out always receives the count; Cj (capacity cap) is filled when it is large
 * enough (-4 otherwise); pass Cj = NULL to size it. */
int madipm_build_normal_system(int32_t n_rows, int32_t n_cols, const int32_t* Jtp, const int32_t* Jtj,
                               int32_t* Cp, int32_t* Cj, int64_t cap, int64_t* nnz_out);

/* MadIPM.assemble_normal_system!(n_rows, n_cols, Jtp, Jtj, Jtx, Cp, Cj, Cx, Dx) (src/utils.jl:
 * 276-308; GPU cuda_wrapper.jl:108-156): Cx[c] = sum_k (Jx[i,k] Dx[k]) Jx[j,k] for entry c = (j,
 * column i), merge-joined over each row's ascending column indices (the GPU reference's
 * precondition, which coo_to_csr with sort_cols provides).  Device arrays. */
int madipm_assemble_normal_system(int32_t n_rows, int32_t n_cols, const int32_t* d_Jtp, const int32_t* d_Jtj,
                                  const double* d_Jtx, const int32_t* d_Cp, const int32_t* d_Cj, double* d_Cx,
                                  const double* d_Dx, madipm_stream_t stream);

/* fill_structure!(A::CSR, rows, cols) (MadIPMCUDAExt.jl:15-32; hess_structure!/jac_lin_structure!):
 * rows[c] = i, cols[c] = colval[c] for the entries c of row i. */
int madipm_csr_fill_structure(int32_t n_rows, const int32_t* d_Ap, const int32_t* d_Aj, int32_t* d_rows,
                              int32_t* d_cols, madipm_stream_t stream);

/* NLPModels.obj(qp, x) (MadIPMCUDAExt.jl:34-38): v = H x; obj = c0 + c'x + v'x/2 written to
 * d_work[512] (d_work: 513 doubles of scratch) and, when h_obj != NULL, to *h_obj (synchronises).
 * NLPModels.grad!(qp, x, g) (:40-45): g = H x + c.  H: a symmetric madipm_spmv_t of size n. */
int madipm_qp_obj(madipm_spmv_t H, const double* d_c, double c0, const double* d_x, double* d_v, int32_t n,
                  double* d_work, double* h_obj, madipm_stream_t stream);
int madipm_qp_grad(madipm_spmv_t H, const double* d_c, const double* d_x, double* d_g, int32_t n,
                   madipm_stream_t stream);

/* update_step! (src/kernels.jl:291-358) with get_alpha_max_primal / get_alpha_max_dual
 * (src/kernels.jl:226-272) on DEVICE vectors over the bounded coordinates (the reference's views
 * x_lr, xl_r, zl_r, dx_lr, dual_lb(d) and x_ur, xu_r, zu_r, dx_ur, dual_ub(d)); the same kernels the
 * native MPC loop runs.  rule: 0 ConservativeStep(tau), 1 AdaptiveStep(tau_min = tau; uses mu),
 * 2 MehrotraAdaptiveStep(gamma_f = tau).  The argmin follows the reference's left fold with
 * init (1.0, 0): the LAST index among equal ratios; index -1 = the init element (Julia's 0). */
typedef struct madipm_step_result {
  double alpha_p, alpha_d;                      /* solver.alpha_p / alpha_d after update_step! */
  double alpha_xl, alpha_xu, alpha_zl, alpha_zu; /* the four max-ratio values (tau of the rule) */
  int32_t i_xl, i_xu, i_zl, i_zu;               /* their argmin indices, 0-based */
} madipm_step_result;
int madipm_update_step(int32_t rule, double tau, double mu, int32_t nlb, int32_t nub,
                       const double* d_x_lr, const double* d_xl_r, const double* d_zl_r, const double* d_dx_lr,
                       const double* d_dzl, const double* d_x_ur, const double* d_xu_r, const double* d_zu_r,
                       const double* d_dx_ur, const double* d_dzu, madipm_step_result* out,
                       madipm_stream_t stream);

/* ------------------------------------------------------------------ native MPC solver
 * `MPCSolver(qp; kwargs...)` + `solve!(solver)` (src/structure.jl:79-178, src/solver.jl:362-418)
 * for a QuadraticModel with SparseKKTSystem (K2), run entirely on the GPU with the LDL^T above.
 * All problem arrays are HOST pointers (0-based COO; H = lower triangle). */
typedef struct madipm_qp {
  int32_t nvar, ncon;
  int64_t nnzh, nnzj;
  const double* c;
  double c0;
  const int32_t *Hrows, *Hcols;
  const double* Hvals;
  const int32_t *Arows, *Acols;
  const double* Avals;
  const double *lcon, *ucon, *lvar, *uvar;
  const double *x0, *y0; /* may be NULL (zeros) */
  int32_t minimize;
} madipm_qp;

/* IPMOptions (src/utils.jl:69-105) */
typedef struct madipm_options {
  double tol;                 /* 1e-8 */
  int32_t max_iter;           /* 3000 */
  double max_wall_time;       /* 1e6 */
  double divergence_tol;      /* 1e4 */
  int32_t scaling;            /* 1 */
  double bound_push, bound_fac, bound_relax_factor; /* 1e-2, 1e-2, 1e-12 */
  int32_t regularization;     /* 0 NoRegularization, 1 FixedRegularization, 2 AdaptiveRegularization */
  double delta_p, delta_d, delta_min; /* (1e-10, 1e-10, -) */
  int32_t step_rule;          /* 0 ConservativeStep(tau), 1 AdaptiveStep(tau_min), 2 MehrotraAdaptiveStep(gamma_f) */
  double step_tau;            /* 0.99 */
  int32_t max_ncorr;          /* 0 (Gondzio correctors) */
  double mu_init, mu_min;     /* 1e-1, 1e-12 */
  double tol_linear_solve;    /* 1e-8 */
  int32_t check_residual;     /* 0 */
  int32_t kkt_system;         /* 0 SparseKKTSystem (K2), 1 ScaledSparseKKTSystem (K2.5),
                                 2 NormalKKTSystem (src/KKT/normalkkt.jl; LPs only, Cholesky semantics) */
  int32_t print_level;        /* 0 silent, 1 iteration log to stdout */
  madipm_ldl_opts ldl;
} madipm_options;

/* MadNLP.Status values used by MadIPM */
enum {
  MADIPM_REGULAR = 0,
  MADIPM_SOLVE_SUCCEEDED = 1,
  MADIPM_INFEASIBLE_PROBLEM_DETECTED = 2,
  MADIPM_MAXIMUM_ITERATIONS_EXCEEDED = -1,
  MADIPM_MAXIMUM_WALLTIME_EXCEEDED = -2,
  MADIPM_DIVERGING_ITERATES = -3,
  MADIPM_ERROR_IN_STEP_COMPUTATION = -4,
  MADIPM_INTERNAL_ERROR = -5
};

typedef struct madipm_stats {
  int32_t status, iter;
  double objective;           /* un-scaled, sign-corrected (update_solution!, src/utils.jl:150-156) */
  double dual_objective;
  double inf_pr, inf_du, inf_compl, mu;
  double total_time;          /* MPC loop only, as cnt.total_time (src/solver.jl:181,407) */
  double linear_solver_time;  /* factorizations (GPU events) */
  double init_time;           /* symbolic analysis + initialize! */
  int32_t exception;          /* MADIPM_EXC_*: the exception solve!'s catch-all caught (status INTERNAL_ERROR);
                                 a binding with rethrow_error = true rethrows it (src/solver.jl:398-403) */
} madipm_stats;

/* Exceptions of the MPC loop.  Both end in solve!'s catch-all (src/solver.jl:398-403) as
 * INTERNAL_ERROR: linear_solver.jl:41 throws the TYPE MadNLP.SolveException, which is not
 * `isa MadNLP.LinearSolverException`, and the linear solver's own refusal to solve with an
 * unfactorized matrix (after factorize_regularized_system!'s three failed trials,
 * linear_solver.jl:6-17; LDLFactorizations' ldiv! [EXT]) is not one either. */
enum {
  MADIPM_EXC_NONE = 0,
  MADIPM_EXC_SOLVE = 1,         /* residual NaN, or > tol_linear_solve with check_residual */
  MADIPM_EXC_UNFACTORIZED = 2   /* solve with a failed factorization */
};

typedef struct madipm_iter_trace {
  int32_t k;
  double obj, inf_pr, inf_du, inf_compl, mu, alpha_p, alpha_d, del_w, dx_inf, residual;
} madipm_iter_trace;

typedef struct madipm_solver* madipm_solver_t;
void madipm_default_options(madipm_options* opt);
int madipm_solver_create(const madipm_qp* qp, const madipm_options* opt, madipm_solver_t* out);
/* Sharded across the processes of `comm` (shard = comm rank): every process runs the MPC loop on
 * replicated vectors; the LDL^T is subtree-sharded with RCCL all-reduces (SURVEY §8 e). */
int madipm_solver_create_dist(const madipm_qp* qp, const madipm_options* opt, madipm_comm_t comm,
                              madipm_solver_t* out);
/* initialize! alone (src/solver.jl:127-189); the next solve() then runs only the MPC loop.
 * Without it, solve() initializes first (as solve! does). */
int madipm_solver_initialize(madipm_solver_t s);
int madipm_solver_set_max_iter(madipm_solver_t s, int32_t max_iter);
int madipm_solver_solve(madipm_solver_t s, madipm_stats* stats);
/* any pointer may be NULL: x/zl/zu length nvar, y/cons length ncon (un-scaled, as MadNLP stats) */
int madipm_solver_get_solution(madipm_solver_t s, double* x, double* y, double* zl, double* zu, double* cons);
/* copies up to cap records, returns the number of recorded iterations */
int madipm_solver_trace(madipm_solver_t s, madipm_iter_trace* out, int32_t cap);
int madipm_solver_ldl_info(madipm_solver_t s, madipm_ldl_info* info);
/* fill-reducing pivot order of the K2 factorization (length nvar_std + ncon, K2 unknowns [x; y]) */
int madipm_solver_ldl_perm(madipm_solver_t s, int32_t* perm);
/* lanes per row of the MPC loop's SpMV kernels (4, 8, 16, 32 or 64): chosen at construction from the
 * mean row length of [H A^T; A], or forced by the environment variable MADIPM_SPMV_G (one of those five
 * values; anything else is ignored).  Returns the width, < 0 on error.  [ABI 0.2.3, additive] */
int madipm_solver_spmv_group(madipm_solver_t s);
/* the solver's LDL^T: timing as madipm_ldl_set_timing / madipm_ldl_kernel_stats */
int madipm_solver_set_timing(madipm_solver_t s, uint32_t mask);
int madipm_solver_kernel_stats(madipm_solver_t s, madipm_kstat* out);
void madipm_solver_destroy(madipm_solver_t s);

/* ------------------------------------------------------------------ re-solve with new data  [ABI 0.2.4, additive]
 * A sequence of problems with one sparsity pattern: the ordering, the symbolic factorisation, the device
 * plan and every allocation of an existing solver are kept and only the numbers are replaced.
 * (madipm_version() still returns 203: these three symbols are the whole addition, no struct changed.)
 *
 * New numbers for the problem an existing solver was created with.  Any pointer may be NULL (= keep the
 * current data); lengths are the creation-time nvar / ncon / nnzj / nnzh; HOST pointers, read during the
 * call only.  The pattern and the classification of every bound are fixed at creation. */
typedef struct madipm_qp_update {
  const double *c; const double *c0;            /* c0: pointer so that NULL means "keep" */
  const double *Hvals, *Avals;                  /* in the creation-time COO order */
  const double *lcon, *ucon, *lvar, *uvar;
  const double *x0, *y0;
} madipm_qp_update;

/* Builds, once, the host and device index plans of the refresh from the madipm_qp the solver was created
 * with.  Its dimensions must be the creation-time ones; its index arrays are copied, and so is Avals (the
 * solver keeps no host copy of A otherwise, and a later update with Avals == NULL has to keep them); the
 * other fields are not read.  A second call is a no-op.  A solver that never calls it gets no extra work
 * and no extra host or device memory.  Cost: 16 B of device plan + 8 B of device staging + 16 B of host
 * memory per entry of A, 12 B + 8 B per stored entry of H. */
int madipm_solver_prepare_update(madipm_solver_t s, const madipm_qp* qp);
/* Installs the new data; the next madipm_solver_initialize / madipm_solver_solve runs on the new problem
 * from its x0 / y0.  Starts no solve, allocates no device memory, runs no analysis, and returns with the
 * solver's stream idle.  The matrix values are refreshed by device kernels with the bits a fresh
 * madipm_solver_create of the updated problem would have uploaded.
 * Rejected (negative code, madipm_last_error() names the first offending index and what changed, solver
 * untouched): a change, with the merged data, of an equality row (lcon == ucon) into a ranged one or back,
 * of a fixed variable (lvar == uvar) into a free one or back, of an infinite bound into a finite one or
 * back; and a call before madipm_solver_prepare_update.
 * madipm_solver_create_dist: every rank calls it with the same data. */
int madipm_solver_update(madipm_solver_t s, const madipm_qp_update* u);
/* n_analyses: linear-solver analyses run for this solver (1 after creation, and it stays 1); n_updates:
 * successful updates; last_update_s: host wall time of the last one, its stream synchronisation included.
 * Any pointer may be NULL. */
int madipm_solver_counters(madipm_solver_t s, int64_t* n_analyses, int64_t* n_updates, double* last_update_s);

/* ------------------------------------------------------------------ the device route  [ABI 0.2.5, additive]
 * The re-solve loop without the host: the update reads DEVICE arrays, the solution is written to DEVICE
 * arrays, and everything the host update computes on the host (bound relaxation and push, the slack start
 * A x, set_scaling!'s row maxima and gradient, the fixed variables' terms, the norms) is recomputed by
 * kernels, every sum in the host loop's order and rounding: the refreshed solver holds exactly the bits a
 * madipm_solver_create of the updated problem would hold.  (madipm_version() still returns 203.)
 *
 * madipm_solver_update_device: as madipm_solver_update, but every array pointer of `u` is a DEVICE pointer
 * (c0 stays a host pointer); NULL = keep.  Needs madipm_solver_prepare_update first.
 * Stream contract: `stream` is the stream the caller's arrays were produced on (NULL = the default
 * stream).  The reads are ordered after the work already enqueued on it (an event wait: the caller's
 * stream is not synchronised with the host).  The call returns with all its reads done and the solver's
 * stream idle: the caller may then overwrite or free its arrays, which are never written.  Starts no
 * solve, runs no analysis; n_updates and last_update_s count it.
 * Rejections: those of madipm_solver_update, on the merged data (given fields over kept fields), with the
 * same negative code and the same madipm_last_error() text (first offending index in the host's check
 * order: row kinds, then variables, then ranged rows); the solver is untouched.
 * Memory: the first call on a solver allocates, on top of madipm_solver_prepare_update's plan: 8 B per
 * entry of A (row lists of the slack start and the row maxima) + 8 B per entry of A in a fixed column;
 * 8 B per endpoint of a stored entry of H (16 B off the diagonal) + 8 B per entry between a fixed and a
 * free variable + 12 B per entry between two fixed ones; 4 B per row and per variable for each list
 * start; 8 B x (4 nvar + 3 ncon) of raw staging; 8 B x (3 (nvar + ranged rows) + nvar + ncon) of start
 * vectors.  Later calls allocate nothing; a solver that never calls it, or calls only
 * madipm_solver_prepare_update / madipm_solver_update, pays nothing.
 * Mixing: madipm_solver_update, _update_device, _solve and _get_solution may follow each other in any
 * order.  A host update after a device update first reads the device-installed numbers back, so that its
 * "keep" fields and its classification check see them (madipm_solver_get_data does the same).
 * madipm_solver_create_dist: every rank calls it with its own device copy of the same data. */
int madipm_solver_update_device(madipm_solver_t s, const madipm_qp_update* u, madipm_stream_t stream);
/* update_solution! into DEVICE arrays (any may be NULL): un-scaled, lengths and bits as
 * madipm_solver_get_solution.  Does not block the host: the writes are ordered after the work already
 * enqueued on `stream`, and work enqueued on `stream` after the call returns sees the results. */
int madipm_solver_get_solution_device(madipm_solver_t s, double* d_x, double* d_y, double* d_zl, double* d_zu,
                                      double* d_cons, madipm_stream_t stream);
/* The raw problem numbers the solver currently holds (what was last installed by create / update /
 * update_device), copied to HOST arrays; any pointer may be NULL.  Avals needs
 * madipm_solver_prepare_update (the solver keeps no copy of A before it). */
int madipm_solver_get_data(madipm_solver_t s, double* c, double* c0, double* Hvals, double* Avals, double* lcon,
                           double* ucon, double* lvar, double* uvar, double* x0, double* y0);

/* ------------------------------------------------------------------ warm start  [ABI 0.2.6, additive]
 * A re-solve from a previous or caller-supplied point instead of the Mehrotra least-squares start alone.
 * (madipm_version() still returns 203: these five symbols are the whole addition, no struct changed.)
 *
 * A warm point is (x, y, zl, zu) in the public, un-scaled space — what madipm_solver_get_solution and
 * madipm_solver_get_solution_device return: lengths nvar, ncon, nvar, nvar.  Any of the four may be NULL
 * (that block keeps its cold values; the slack values need x, the slack multipliers need y), not all four.
 * While a point is set, madipm_solver_initialize / the initialisation inside madipm_solver_solve runs
 * unchanged up to the end of init_starting_point!, then blends: x is clamped into the (relaxed) bounds,
 * the slacks are the clamped scaled row values of it, y and z are scaled (z clamped at 0, the slack
 * multipliers max(-y, 0) / max(y, 0)), every block becomes weight * warm + (1 - weight) * cold, a coordinate
 * whose blended value is not strictly inside its bounds (or a multiplier that is not > 0) keeps its cold
 * value, and the model is evaluated at the blended point.  The MPC loop is unchanged; it is the same rule
 * for every KKT formulation, for a sharded solver and (every rank setting the same point) a distributed one.
 * Without a point — never set, or cleared — initialisation is bit for bit the cold one: no extra kernel, no
 * allocation.
 * The point is kept on the device un-scaled (obj_scale and con_scale may change with the next update) and
 * persists across solves and updates until it is replaced (a call replaces the whole point: the blocks it
 * leaves NULL become absent) or cleared.  Memory: 8 B x (3 nvar + ncon) + 12 B per inequality row (+ 8 B x
 * ncon for con_scale on a solver that never ran an update), allocated by the first call that sets a point
 * and never again.
 * weight must lie in the open interval (0, 1) (0.99 is the recommended value); a weight outside it or NaN,
 * or four NULL pointers, is refused: negative code, the reason in madipm_last_error(), solver untouched.
 * Non-finite entries of the point are NOT checked: they reach the iterate and the solve ends as any
 * NaN does (INTERNAL_ERROR).
 *
 * madipm_solver_set_warm_start: HOST pointers, read during the call only. */
int madipm_solver_set_warm_start(madipm_solver_t s, const double* x, const double* y, const double* zl,
                                 const double* zu, double weight);
/* DEVICE pointers, with the stream contract of madipm_solver_update_device: `stream` is the stream the
 * arrays were produced on; the reads are ordered after the work already enqueued on it by an event wait,
 * and the host is not synchronised.  The arrays are copied by the call: work enqueued on `stream` after it
 * returns is ordered after the copies, so the caller may overwrite the arrays from that stream at once. */
int madipm_solver_set_warm_start_device(madipm_solver_t s, const double* d_x, const double* d_y, const double* d_zl,
                                        const double* d_zu, double weight, madipm_stream_t stream);
/* The solver's own current iterate as the warm point: the bits madipm_solver_get_solution_device would
 * write at the time of the call, without a trip through the host and without blocking it.  An error before
 * the first solve.  The iterate is un-scaled with the solver's CURRENT obj_scale / con_scale: in a re-solve
 * loop call it after the solve and BEFORE the next update, so that the solution is un-scaled with the
 * scaling it was computed in (after an update the two differ when set_scaling! gives other factors). */
int madipm_solver_warm_start_last(madipm_solver_t s, double weight);
/* Back to cold starts; the device copy stays allocated for the next point. */
int madipm_solver_clear_warm_start(madipm_solver_t s);
/* active: a point is set; weight: its weight (0 when none); n_warm_inits: initialisations that blended.
 * Any pointer may be NULL. */
int madipm_solver_warm_info(madipm_solver_t s, int32_t* active, double* weight, int64_t* n_warm_inits);

/* ------------------------------------------------------------------ adjoint gradients  [ABI 0.2.7, additive]
 * The solver as a differentiable layer: for a loss l(x*) of the optimal x alone, given gx = dl/dx* (length
 * nvar), the gradients of l with respect to the problem data.  (madipm_version() still returns 203: these
 * three symbols and one struct are the whole addition, no existing struct changed.)
 *
 * Every non-NULL field of madipm_qp_gradients receives one gradient: c, lvar, uvar of length nvar, lcon, ucon of
 * length ncon, Hvals of length nnzh and Avals of length nnzj in the creation-time COO order (a duplicated
 * entry receives the full value in each copy).  Conventions: an infinite bound has gradient 0; for a fixed
 * variable (lvar == uvar) and an equality row (lcon == ucon) the whole derivative with respect to the common
 * value is in lvar / lcon and uvar / ucon is 0, so a caller that passes one array as both bounds adds the two
 * and gets the right sum; c0 has no influence.  The derivation is DESIGN §13c.
 * The call factorises the K2 matrix of the last solve's end point (kkt_diag + assemble + LDL^T, with the
 * regularisation the options prescribe: none, the fixed pair, or the adaptive pair as the solve left it,
 * and the loop's x100 retries, three trials) and runs one solve with it plus two steps of iterative refinement
 * towards the matrix WITHOUT the regularisation, so that the gradients do not carry it (MADIPM_ADJ_REFINE =
 * 0..8 sets the step count, for measurements); a later call on the same point (another gx) reuses the factor.  Nothing a later madipm_solver_initialize / _solve / _warm_start_last
 * reads is changed: solve, adjoint, solve gives the second solve the bits of solve, solve.
 * Refused (negative code, reason in madipm_last_error(), solver untouched): before the first solve; when the
 * last solve did not end with MADIPM_SOLVE_SUCCEEDED; after a madipm_solver_update / _update_device /
 * _initialize that no solve followed (the iterate no longer belongs to the data); kkt_system 1 or 2 (K2.5
 * and the normal equations are left to a later release); a solver made by madipm_solver_create_dist; gx
 * NULL; all seven outputs NULL.  A failure of all three factorisation trials is an error (-4).
 * Memory, each part allocated by the first call that needs it and never again: 8 B x (3 nvar + 2 ncon +
 * 2 inequality rows + 2) of right-hand side, solution and residual scratch; 4 B per row with lcon / ucon; 8 B per entry of
 * A with Avals and 8 B per entry of H with Hvals (device copies of the COO indices); with lvar on a problem
 * with fixed variables 8 B per entry of A in a fixed column and per entry of H between a fixed and a free
 * variable; on the host route 8 B per entry of each output asked for.  Avals, Hvals and that lvar need
 * madipm_solver_prepare_update first (the raw values and index arrays it keeps); c, the bounds of a problem
 * without fixed variables, lcon and ucon need nothing per entry of A.
 *
 * madipm_solver_adjoint: HOST pointers, read / written during the call. */
typedef struct madipm_qp_gradients { double *c, *Hvals, *Avals, *lcon, *ucon, *lvar, *uvar; } madipm_qp_gradients; /* NULL = not wanted */
int madipm_solver_adjoint(madipm_solver_t s, const double* gx, const madipm_qp_gradients* out);
/* DEVICE pointers.  d_gx has the stream contract of madipm_solver_set_warm_start_device: it is read after
 * the work already enqueued on `stream` (an event wait; the host is not blocked on it).  The outputs have
 * that of madipm_solver_get_solution_device: work enqueued on `stream` after the call returns sees them.
 * The first call on a point waits, on the host, for the status of its factorisation. */
int madipm_solver_adjoint_device(madipm_solver_t s, const double* d_gx, const madipm_qp_gradients* d_out,
                                 madipm_stream_t stream);
/* n_adjoints: successful adjoint calls; n_adjoint_factorizations: those that factorised (one per point);
 * last_residual: ||g - K a||_inf / max(1, ||g||_inf) of the last call's refined solution, K the K2 matrix of
 * the point without the regularisation (H, J, J^T and Sigma_l + Sigma_u); large on a degenerate point, whose
 * gradients are then only as good as that (synchronises the solver's stream).  Any pointer may be NULL. */
int madipm_solver_adjoint_info(madipm_solver_t s, int64_t* n_adjoints, int64_t* n_adjoint_factorizations,
                               double* last_residual);

/* ------------------------------------------------------------------ adjoint of all five blocks  [ABI 0.2.8, additive]
 * The same gradients for a loss l(x, y, zl, zu, cons) of everything madipm_solver_get_solution returns: the
 * row multipliers y (length ncon), the bound multipliers zl, zu (length nvar) and the constraint values
 * cons = A x (length ncon), besides x.  (Two symbols and one struct; nothing above changed.)
 * Every non-NULL field of madipm_qp_cotangents is the derivative of l with respect to that block, in the
 * public un-scaled space; a NULL field is read as 0.  Constants, whose cotangents are ignored: zl_i / zu_i of
 * a variable without that bound, and zl, zu of a fixed variable (all of them are returned as 0).  The slack
 * multipliers max(-/+y, 0) are not separate arguments of the loss: it sees y.
 * One more solve with the factor madipm_solver_adjoint uses (one factorisation per solved point serves both
 * calls; the counters and the residual of madipm_solver_adjoint_info cover both), with a right-hand side in
 * which the 1 / gap^2 terms of the active bounds are cancelled analytically: the bound
 * gradients do not lose digits where Sigma = z / gap is 1e8 and more.  last_residual is that of this shifted
 * system.  The outputs, their conventions, the stream contracts and the prerequisites (prepare_update for
 * Avals, Hvals and lvar with fixed variables) are those of madipm_solver_adjoint / _adjoint_device.
 * Refused as there, and when all five cotangents are NULL.  With x alone the call runs madipm_solver_adjoint's
 * own path and returns its bits.
 * Memory on top of madipm_solver_adjoint's, by the first call with a cotangent other than x: 8 B x (2 nvar +
 * ncon + inequality rows); on the host route 8 B per entry of each cotangent given. */
typedef struct madipm_qp_cotangents { const double *x, *y, *zl, *zu, *cons; } madipm_qp_cotangents; /* NULL = absent (0) */
int madipm_solver_adjoint_full(madipm_solver_t s, const madipm_qp_cotangents* g, const madipm_qp_gradients* out);
int madipm_solver_adjoint_full_device(madipm_solver_t s, const madipm_qp_cotangents* d_g,
                                      const madipm_qp_gradients* d_out, madipm_stream_t stream);

/* ------------------------------------------------------------------ forward-mode sensitivities  [ABI 0.2.9, additive]
 * The transpose of the adjoint: given a DIRECTION in the data (dc, dHvals, dAvals, dlcon, ducon, dlvar, duvar),
 * the directional derivative (dx, dy, dzl, dzu, dcons) of everything madipm_solver_get_solution returns, at
 * the end point of the last successful solve: x*(theta + t d) = x* + t dx + O(t^2), the first-order prediction
 * of a re-solve, or one column of the Jacobian per call.  (Three symbols and two structs; madipm_version()
 * still returns 203; nothing above changed.)
 * Every non-NULL field of madipm_qp_directions is one direction block, with the lengths and the COO order of
 * madipm_qp_gradients; a NULL field is read as 0; duplicated COO entries are separate parameters that add.
 * Conventions, the transposes of the adjoint's: an entry on an infinite bound is not read; for a fixed
 * variable the common value moves by lvar's entry and uvar's is not read; for an equality row it moves by
 * lcon's entry and ucon's is not read (so one array passed as both bounds stays right); c0 has no direction.
 * Every non-NULL field of madipm_qp_point_tangents receives that block's derivative (x, zl, zu of length nvar;
 * y, cons of length ncon); dzl_i / dzu_i is 0 for a variable without that bound and for a fixed variable.
 * One solve with the factor madipm_solver_adjoint uses (one factorisation per solved point serves the adjoint
 * and the tangent, in either order; n_adjoint_factorizations counts it), plus its two refinement steps
 * towards the matrix without the regularisation, with the right-hand side and the outputs in a shifted form
 * in which no product of Sigma = z / gap (1e8 and more at an active bound) with a direction remains (DESIGN
 * §13e).  Nothing a later madipm_solver_initialize / _solve / _warm_start_last reads is changed.
 * Refused as madipm_solver_adjoint refuses (before the first solve; a last status other than SOLVE_SUCCEEDED;
 * an update / update_device / initialize that no solve followed; kkt_system 1 or 2; a solver made by
 * madipm_solver_create_dist), and when all seven directions or all five outputs are NULL.  Directions in
 * Hvals, Avals, and in lvar on a problem with fixed variables, need madipm_solver_prepare_update first (the raw
 * values and index arrays it keeps).
 * Memory, each part allocated by the first call that needs it and never again: madipm_solver_adjoint's scratch
 * and that of its five-block call if no adjoint allocated them (8 B x (4 nvar + 3 ncon + 3 inequality rows + 2),
 * 4 B per row), 8 B x (2 nvar + ncon + 2 inequality rows + 1) of its own; with a direction that needs
 * prepare_update, 16 B per entry of A, 8 B per endpoint of a stored entry of H (16 B off the diagonal) and
 * 4 B x (2 nvar + ncon + 3) of list starts; on the host route 8 B per entry of each direction given and each
 * output asked for.  A solver that never calls it pays nothing.
 *
 * madipm_solver_tangent: HOST pointers, read / written during the call. */
typedef struct madipm_qp_directions { const double *c, *Hvals, *Avals, *lcon, *ucon, *lvar, *uvar; } madipm_qp_directions; /* NULL = 0 */
typedef struct madipm_qp_point_tangents { double *x, *y, *zl, *zu, *cons; } madipm_qp_point_tangents; /* NULL = not wanted */
int madipm_solver_tangent(madipm_solver_t s, const madipm_qp_directions* d, const madipm_qp_point_tangents* out);
/* DEVICE pointers.  The directions have the stream contract of madipm_solver_adjoint_device's cotangents (read
 * after the work already enqueued on `stream`), the outputs that of its outputs (work enqueued on `stream`
 * after the call returns sees them).  The first call on a point waits, on the host, for the status of its
 * factorisation. */
int madipm_solver_tangent_device(madipm_solver_t s, const madipm_qp_directions* d_d,
                                 const madipm_qp_point_tangents* d_out, madipm_stream_t stream);
/* n_tangents: successful tangent calls; last_residual: ||r - K w||_inf / max(1, ||r||_inf) of the last call's
 * refined solution of the shifted system, as madipm_solver_adjoint_info reports it for the adjoint (the two
 * do not overwrite each other; synchronises the solver's stream).  Any pointer may be NULL. */
int madipm_solver_tangent_info(madipm_solver_t s, int64_t* n_tangents, double* last_residual);

/* ------------------------------------------------------------------ polish: exact active-set solve  [ABI 0.2.10, additive]
 * madipm_solver_solve ends at a central-path point (mu about 1e-9): no bound is attained exactly and the
 * multipliers of inactive bounds are about 1e-8.  The polish identifies the active set at that point (or takes
 * the caller's), fixes the active coordinates of v = [x_free; s] (s = the inequality rows' values) at their
 * bounds and solves the equality-constrained QP of that face to rounding level: one factorisation of the K2
 * pattern (active coordinates penalised by sigma on the diagonal, no Sigma on the others) preconditions
 * 1 + refine_steps solves with the EXACT reduced operator.  (Four symbols and three structs;
 * madipm_version() still returns 203; nothing above changed.)
 * The guess: coordinate j is lower-active when it has a lower bound and zl_j > v_j - lo_j, upper-active when it
 * has an upper bound and zu_j > hi_j - v_j (both: the larger multiplier, lower on a tie), on the values
 * madipm_solver_get_solution returns (a row's multipliers are max(-y, 0) and max(y, 0)).  A supplied set is one
 * int8 per variable and one per row: -1 lower, +1 upper, 0 inactive; 0 on fixed variables and equality rows.
 * The verdict (the larger number wins):
 *   0 POLISHED: residual <= tol_resid (max-norm of the exact reduced residual at the final point, scaled space),
 *     every active multiplier >= -tol_sign max(1, max |multiplier|), every inactive bound kept
 *     (gap >= -tol_feas max(1, |bound|)).  The outputs are the polished point: an active variable equals its
 *     bound, an inactive multiplier is 0, cons of an active row is the row's bound.
 *   1 WRONG_SET: a sign or a bound is violated.   2 NO_CONVERGENCE: the residual is above tol_resid or not
 *   finite (a degenerate face with dependent active constraints).   3 FACTORIZATION_FAILED: all three
 *   regularisation trials failed.  In verdicts 1 - 3 the outputs are madipm_solver_get_solution's, bit for bit.
 * info: verdict; n_active; residual; min_multiplier (the smallest active multiplier, +inf without one);
 * min_gap (the smallest gap over the inactive bounds, +inf without one); the two counters.
 * Refused as madipm_solver_adjoint refuses, and: exactly one of active_var / active_row given; a code other
 * than -1, 0, +1, or one on a bound that does not exist, on a fixed variable or on an equality row; every
 * output NULL; sigma, a tolerance or refine_steps (0..8) out of range.
 * The call overwrites the KKT diagonal and the LDL^T factor: a later adjoint / tangent on the point
 * factorises again (and a polish after those as well); a second polish of the same point with the same set
 * and sigma does not.  Nothing a later madipm_solver_initialize / _solve reads is changed.
 * Memory, allocated by the first call: madipm_solver_adjoint's scratch if no adjoint allocated it, 8 B x (4 n +
 * 2 ncon) + 2 n bytes + 4 B per inequality row + 64 KiB of its own (n = nvar + inequality rows); on the host
 * route 8 B per entry of each block and 1 B per code asked for or supplied. */
enum { MADIPM_POLISHED = 0, MADIPM_POLISH_WRONG_SET = 1, MADIPM_POLISH_NO_CONVERGENCE = 2,
       MADIPM_POLISH_FACTORIZATION_FAILED = 3 };
typedef struct madipm_polish_opts { double sigma, tol_resid, tol_sign, tol_feas; int32_t refine_steps; } madipm_polish_opts;
typedef struct madipm_polish_out { double *x, *y, *zl, *zu, *cons; int8_t *active_var, *active_row; } madipm_polish_out; /* any NULL */
typedef struct madipm_polish_info {
  int32_t verdict, n_active;
  double residual, min_multiplier, min_gap;
  int64_t n_polishes, n_polish_factorizations;
} madipm_polish_info;
void madipm_polish_default_opts(madipm_polish_opts* o); /* sigma 1e10, tolerances 1e-10, 1e-9, 1e-9, refine_steps 2 */
/* HOST pointers.  opts NULL: the defaults; active_var and active_row both NULL: the guess; info may be NULL. */
int madipm_solver_polish(madipm_solver_t s, const madipm_polish_opts* opts, const int8_t* active_var,
                         const int8_t* active_row, const madipm_polish_out* out, madipm_polish_info* info);
/* DEVICE pointers for the sets and `out` (info is a host struct), with the stream contract of
 * madipm_solver_adjoint_device; the call waits, on the host, for the set's validation and the verdict. */
int madipm_solver_polish_device(madipm_solver_t s, const madipm_polish_opts* opts, const int8_t* d_active_var,
                                const int8_t* d_active_row, const madipm_polish_out* d_out, madipm_polish_info* info,
                                madipm_stream_t stream);
/* The last polish's info (zeros and verdict -1 before the first); no device access. */
int madipm_solver_polish_info(madipm_solver_t s, madipm_polish_info* info);

/* ------------------------------------------------------------------ sensitivities at the polished point  [ABI 0.2.11, additive]
 * madipm_solver_tangent / _adjoint differentiate the central-path point.  These differentiate the point the last
 * madipm_solver_polish left: the exact derivatives of the equality-constrained QP of the face its active set
 * defines.  Structs, conventions (what is not read, where a fixed variable's and an equality
 * row's derivative goes), routes and the stream contract are those of madipm_solver_tangent /
 * madipm_solver_adjoint_full.  What differs: the tangent of an active variable IS the direction of its bound
 * and dcons of an active row the direction of the row's bound (copies); dzl / dzu of an inactive, absent or
 * fixed bound are exactly 0; the gradient of an inactive or absent bound is exactly 0; cons of an inequality
 * row is the row's slack and of an equality row lcon itself.  (Five symbols, no struct; madipm_version()
 * still returns 203; nothing above changed.)
 * Both solve one system with the polish's operator and factor, 1 + refine_steps (the polish's) times; when an
 * adjoint or tangent took the LDL^T since the polish, the polish's factor is rebuilt from the kept set and
 * sigma (counted in n_factorizations), and a later adjoint / tangent factorises again.
 * Refused as madipm_solver_tangent / _adjoint_full refuse, and: no polish has run on the point of the last
 * solve; the last polish's verdict was not POLISHED (the message names it).
 * Memory, allocated by the first call: 8 B x (3 n + 2 ncon) of its own (n = nvar + inequality rows), the
 * tangent's data terms and entry lists or the adjoint's index lists as those calls allocate them; on the host
 * route 8 B per entry of each block given or asked for. */
int madipm_solver_tangent_polished(madipm_solver_t s, const madipm_qp_directions* d,
                                   const madipm_qp_point_tangents* out);
int madipm_solver_tangent_polished_device(madipm_solver_t s, const madipm_qp_directions* d_d,
                                          const madipm_qp_point_tangents* d_out, madipm_stream_t stream);
int madipm_solver_adjoint_polished(madipm_solver_t s, const madipm_qp_cotangents* g, const madipm_qp_gradients* out);
int madipm_solver_adjoint_polished_device(madipm_solver_t s, const madipm_qp_cotangents* d_g,
                                          const madipm_qp_gradients* d_out, madipm_stream_t stream);
/* Successful polished tangent / adjoint calls; factorisations they ran to restore the polish's factor;
 * last_residual: the max-norm of the last call's final masked residual, scaled space (0 before the first;
 * synchronises the solver's stream).  Any pointer may be NULL. */
int madipm_solver_polished_sens_info(madipm_solver_t s, int64_t* n_tangents, int64_t* n_adjoints,
                                     int64_t* n_factorizations, double* last_residual);

/* ------------------------------------------------------------------ active-set solve of the held data  [ABI 0.2.12, additive]
 * After madipm_solver_update / _update_device everything an active-set solve of the new problem needs is on the
 * device, and in a sequence of problems the optimal active set is often the previous one or a few bounds away
 * from it.  This call solves the problem the solver holds from a starting set, without an interior-point solve
 * and without reading the iterate.  Set encoding, outputs, routes and the stream contract are
 * madipm_solver_polish's.  (Four symbols and two structs; madipm_version() still returns 203; nothing above
 * changed.)
 * Round k = 1 .. max_rounds: the start (an active coordinate of v = [x_free; s] at its raw bound, an inactive
 * one at 0, y = 0, a fixed variable at its value), then the polish's factor, 1 + refine_steps delta-form solves,
 * residual, measures and verdict.  POLISHED, NO_CONVERGENCE and FACTORIZATION_FAILED end the call; so does
 * WRONG_SET in the last round; WRONG_SET before it gives the next set from exactly the violations found, with
 * M = max(1, max |active multiplier|): an active coordinate with multiplier < -tol_sign M becomes inactive, an
 * inactive one with gap < -tol_feas max(1, |bound|) to a bound it has becomes active there (the lower bound
 * when both are violated).  Every round starts the same way, so the result depends on the data, the final set
 * and the options only.  POLISHED is an optimality certificate of the convex QP.
 * The starting set: active_var / active_row, or with both NULL the kept set: the codes of the last
 * madipm_solver_polish or active-set solve on this solver that ended POLISHED.
 * Outputs: on POLISHED the five blocks exactly as madipm_solver_polish writes a polished point; on any other
 * verdict they are NOT written.  active_var / active_row always receive the last set tried.
 * info: verdict (the MADIPM_POLISH* values), rounds, n_active, n_changed (codes of the last set that differ from
 * the starting set), residual / min_multiplier / min_gap of the last round, the cumulative counters.
 * It needs K2, no communicator, valid codes, an output, max_rounds in 1..16 and the polish's option ranges; with
 * both sets NULL, a kept set.  It needs NO solve, status or initialize: it runs on a fresh solver, after an
 * update, or after a solve.  A round's factor is the polish factor already held when data (update count), codes
 * and sigma are its own: such a call does not factorise.
 * State: a POLISHED call makes its point the current polished point of madipm_solver_tangent_polished /
 * _adjoint_polished until the next update, initialize, solve, polish or active-set solve; any other verdict
 * leaves none.  madipm_solver_adjoint / _tangent / _polish / _warm_start_last, madipm_solver_get_solution and
 * madipm_solver_polish_info are unchanged, and nothing a later madipm_solver_initialize / _solve reads is
 * changed: update; active-set solve; solve gives the bits of update; solve.
 * Memory: the polish's scratch, allocated by the first call of either, + 2 n bytes for the kept and the starting
 * set. */
typedef struct madipm_active_set_opts { madipm_polish_opts polish; int32_t max_rounds; } madipm_active_set_opts;
typedef struct madipm_active_set_info {
  int32_t verdict, rounds, n_active, n_changed;
  double residual, min_multiplier, min_gap;
  int64_t n_calls, n_factorizations;
} madipm_active_set_info;
void madipm_active_set_default_opts(madipm_active_set_opts* o); /* the polish defaults, max_rounds 4 */
/* HOST pointers.  opts NULL: the defaults; active_var and active_row both NULL: the kept set; info may be NULL. */
int madipm_solver_active_set_solve(madipm_solver_t s, const madipm_active_set_opts* opts, const int8_t* active_var,
                                   const int8_t* active_row, const madipm_polish_out* out,
                                   madipm_active_set_info* info);
/* DEVICE pointers for the sets and `out`, with madipm_solver_polish_device's contract; the call waits, on the
 * host, for the set's validation and each round's verdict. */
int madipm_solver_active_set_solve_device(madipm_solver_t s, const madipm_active_set_opts* opts,
                                          const int8_t* d_active_var, const int8_t* d_active_row,
                                          const madipm_polish_out* d_out, madipm_active_set_info* info,
                                          madipm_stream_t stream);
/* The last active-set solve's info (zeros and verdict -1 before the first); no device access. */
int madipm_solver_active_set_info(madipm_solver_t s, madipm_active_set_info* info);

/* ------------------------------------------------------------------ batched sensitivities  [ABI 0.2.13, additive]
 * k tangents or k adjoints of ONE point per call: the columns of a Jacobian, a Gauss-Newton step, several
 * losses on one solve.  The structs are those of madipm_solver_tangent / _adjoint_full, and every
 * non-NULL block holds k vectors back to back: vector j of a block of length len starts at j * len.  A NULL
 * direction / cotangent block is 0 in every column, a NULL output is not wanted; k >= 1.  Column j of every
 * output is, bit for bit, what the single call returns for column j of the inputs (with gx alone:
 * madipm_solver_adjoint's bits; with any other cotangent block given: madipm_solver_adjoint_full's for every
 * column).  (Six symbols, no struct; madipm_version() still returns 203; nothing above changed.)
 * polished = 0, the central-path point: the columns are processed in chunks of at most W =
 * madipm_sens_batch_cols().  Per chunk the right-hand sides, the refinement residuals (the KKT operator's
 * entries and column indices are read once and applied to every column of the chunk) and the outputs are one
 * launch each instead of one per column; the solves are the single call's, one column after the other, with
 * the factor the single calls use (one factorisation per solved point, however many batches and single calls
 * follow).  madipm_solver_tangent_info / _adjoint_info count k more calls and report as last_residual the
 * largest of the columns' ratios (a NaN is kept).
 * polished != 0, the point of the last madipm_solver_polish (or POLISHED active-set solve): the columns run one
 * after another through madipm_solver_tangent_polished / _adjoint_polished with offset pointers: the same bits
 * by construction, no batched kernels and no saving per column; madipm_solver_polished_sens_info counts k more
 * calls and reports the last column's residual.
 * Refused, before anything is allocated or enqueued: k < 1; whatever madipm_solver_tangent / _adjoint_full
 * (polished: _tangent_polished / _adjoint_polished) refuse, including all blocks or all outputs NULL and the
 * madipm_solver_prepare_update requirement of Hvals, Avals and lvar.
 * Memory (polished = 0), allocated by the first batched call that needs it: W columns of what the single call
 * allocates, 8 B x W x (7 n + 6 ncon + nvar + 1) with all of it in use (n = nvar + inequality rows); on the host
 * route 8 B x W per entry of each block given or asked for (the chunks are staged one at a time).  A solver
 * that never batches pays nothing.  The single-column calls are unchanged and share no kernel with these. */
int madipm_sens_batch_cols(void); /* the chunk width W, a compile-time constant (8) */
/* HOST pointers, read / written during the call. */
int madipm_solver_tangent_batch(madipm_solver_t s, int32_t k, const madipm_qp_directions* d,
                                const madipm_qp_point_tangents* out, int32_t polished);
int madipm_solver_adjoint_batch(madipm_solver_t s, int32_t k, const madipm_qp_cotangents* g,
                                const madipm_qp_gradients* out, int32_t polished);
/* DEVICE pointers, with the stream contract of madipm_solver_tangent_device / _adjoint_device. */
int madipm_solver_tangent_batch_device(madipm_solver_t s, int32_t k, const madipm_qp_directions* d_d,
                                       const madipm_qp_point_tangents* d_out, int32_t polished,
                                       madipm_stream_t stream);
int madipm_solver_adjoint_batch_device(madipm_solver_t s, int32_t k, const madipm_qp_cotangents* d_g,
                                       const madipm_qp_gradients* d_out, int32_t polished, madipm_stream_t stream);
/* Successful batched calls, the columns they held, and the chunks of at most W columns the polished = 0 calls
 * ran (ceil(k / W) each; a polished batch adds none); no device access.  Any pointer may be NULL. */
int madipm_solver_sens_batch_info(madipm_solver_t s, int64_t* n_batches, int64_t* n_columns, int64_t* n_chunks);

/* ------------------------------------------------------------------ multi-right-hand-side solve  [ABI 0.2.14, additive]
 * nrhs right-hand sides through ONE pass over the factor per chunk of `width` columns: every L
 * panel is read once and every launch paid once per chunk instead of once per column.  In place, column j at
 * d_x + j * n; nrhs >= 1.  The native route runs on an unsharded factorisation without batched-leaf groups;
 * elsewhere the call is the loop of madipm_ldl_solve.  A column's bits depend neither on nrhs nor on the
 * column's position; they are NOT those of madipm_ldl_solve (another summation order), which keeps its loop
 * and its bits, also after calls of this entry. */
/* (a struct tag only, no typedef: the entry that fills it carries the same name, so write
 * `struct madipm_ldl_multi_info`) */
struct madipm_ldl_multi_info {
  int32_t width;        /* columns of one chunk (8) */
  int32_t native;       /* 1: the multi-column route, 0: the loop of single solves */
  int64_t n_calls;      /* multi-solve calls so far */
  int64_t n_chunks;     /* ceil(nrhs / width) of every call */
  int64_t n_columns;
  int64_t n_big_fronts; /* fronts of the native route's big class (past 192 rows, or a panel beyond the small
                           kernels' LDS): solved by the task-queue kernels, see madipm_ldl_multi_big_info */
};
int madipm_ldl_solve_multi(madipm_ldl_t ls, double* d_x, int32_t nrhs, madipm_stream_t stream);
int madipm_ldl_multi_info(madipm_ldl_t ls, struct madipm_ldl_multi_info* info);
/* on != 0: madipm_solver_tangent_batch / _adjoint_batch (and their _device forms) at the interior-point end
 * point solve every chunk of columns, a chunk of one column included, with the multi-right-hand-side solve: a
 * row's bits then do not depend on k, and are within the formulas' tolerance of (not bitwise equal to) the
 * single calls'.  Default 0: every bit as before.  The single calls and the polished calls never change. */
int madipm_solver_set_multi_solve(madipm_solver_t s, int32_t on);
/* The multi-solve counters of the solver's linear solver (those of madipm_ldl_multi_info). */
int madipm_solver_multi_solve_info(madipm_solver_t s, struct madipm_ldl_multi_info* info);

/* ------------------------------------------------------------------ multi-column big fronts  [ABI 0.2.15, additive]
 * The native route's big fronts carry a chunk's columns through ONE pass per level and direction:
 * their L entries are read once per chunk and the launches paid once, as for the other classes.  A column's
 * arithmetic is that of the single-column big-front kernels, so the rows of madipm_ldl_solve_multi are bit for bit
 * the same with the switch on or off; off (or MADIPM_MULTI_BIG=0 at creation) keeps the column-after-column
 * passes as the reference.  Sharded solvers and plans with batched-leaf groups keep the loop of single solves
 * (native = 0) and only record the switch.  (Three symbols and one struct; `struct madipm_ldl_multi_info` and
 * everything above are unchanged; madipm_version() still returns 203.) */
struct madipm_ldl_multi_big_info {
  int32_t multi_big;     /* 1: big fronts carry a chunk's columns in one pass; 0: column after column */
  int32_t n_big_levels;  /* levels of mlev that hold a big front */
  int64_t n_big_passes;  /* (level, direction) big passes launched so far: 2 * n_big_levels per chunk
                            with multi_big, times the chunk's columns without */
  int64_t big_bytes;     /* device bytes of the multi hand-off, vwork and bpart buffers (0 before the first use) */
};
int madipm_ldl_set_multi_big(madipm_ldl_t ls, int32_t on);
int madipm_ldl_multi_big_info(madipm_ldl_t ls, struct madipm_ldl_multi_big_info* info);
int madipm_solver_multi_big_info(madipm_solver_t s, struct madipm_ldl_multi_big_info* info);

#ifdef __cplusplus
}
#endif

#endif /* MADIPM_HIP_H */
