// Launch planning of the multifrontal LDL^T (host only: no HIP call, no device buffer, no stream).
//
// build_launch_plan turns a SymbolicPlan into everything LDLSolver uploads and launches from: the
// factorisation launch lists, the solve levels, the dependency tables of the tree and DAG kernels, the
// assembly records.  It is plain arithmetic over the plan, so it also runs (and is checked) on a
// machine without a GPU: tools/plan_check.cpp.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "symbolic.hpp"

namespace madipm {

// Constants the kernels (ldl.hip, ldl_solve.hip) and the planner share; defined here and nowhere else.
namespace ldlconst {
constexpr int NT = 256;  // threads of most kernels
// assembly, LDS source path: sources per window (five per thread of the 1024-thread assembly kernels),
// windows of a tile in the large launches, and the most a tile may carry
constexpr int kAsmLdsSrc = 5 * 1024, kAsmLdsWin = 4, kAsmLdsWinMax = 12;
constexpr int BIG_MSZ = 4 * 16 * 17;      // doubles of one panel's M_K blocks (four 16-row blocks, ld 17)
constexpr int UPD_PART = 4 * 4 * 4 * NT;  // partial product doubles of one part (acc of every thread)
constexpr int LBF_COLS = 256;
constexpr int LB_KCHUNK = 2048;  // members per SYRK launch (m x 2048 doubles of W stay cache-resident)
constexpr int GAT_ROWS = NT / 8;
constexpr int BWD_CHUNK = 256;
constexpr int SMALL_SOLVE_MAX = 192;
constexpr int MULTI_W = 8;  // right-hand sides one pass of the multi-column level kernels carries
constexpr int kWorkgroupLds = 160 * 1024;  // LDS one gfx950 workgroup may hold (static + dynamic)
constexpr int kSolveSmallMultiLds = kWorkgroupLds - 8 * MULTI_W * SMALL_SOLVE_MAX;  // k_fwd_small_m / k_bwd_small_m's panel
constexpr int MED_SOLVE_MAX = SymbolicPlan::kFactTreeMedMax;
constexpr int TREE_ROOT_LDS = 150 * 1024;  // the big etree roots' own forward launch (LaunchPlan::nroot_task)
constexpr int TREE_SOLVE_LDS = 76 * 1024;
// dynamic LDS of the in-LDS factorisation classes: r <= 128 square with ld r | 1, r <= 192 packed lower
constexpr int small_sq_lds(int r) { return 8 * r * (r | 1); }
constexpr int small_pk_lds(int r) { return 8 * r * (r + 1) / 2; }
constexpr int kSmall128Lds = small_sq_lds(128), kSmall192Lds = small_pk_lds(192);
constexpr int kSolveSmallLds = kSmall128Lds;  // what k_fwd_small / k_bwd_small may ask for
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
}  // namespace ldlconst

// the batch range a k_fact_tree task folds and its first batch's table entries, in one record loaded
// with the task's other per-front words (r5: the first batch's entries were a dependent round trip)
struct FoldStart {
  int32_t b0, b1;      // batches [b0, b1)
  int32_t kq0, kq1;    // the first batch's leaves [kq0, kq1) (fold_bat)
  int64_t row0, row1;  // its flat leaf rows (fold_row0)
  int64_t poff;        // its product entries (fold_poff, fold_plen)
  int32_t plen, pad;
};
struct FoldHelp {
  int32_t front, flag;  // the front, the flag the helper publishes
  int64_t img;          // its image in FrontTab::fimg: nimg doubles, entry k = LDS entry fimg_dst[dofs + k]
  int64_t dofs;         // its destinations in FrontTab::fimg_dst (the LDS entries its batches' products reach)
  int32_t nimg, pad;
  FoldStart fs;         // its batches
};

// assembly: a big child's block on one 64x64 tile of its parent (SymbolicPlan::bt entry, split by
// column ranges so that na * nb <= kBigRecEntries).  The child's update rows on the tile are the
// consecutive rows a0 .. a0 + na - 1 (its rows are a sorted subset of the parent's), its columns
// b0 .. b0 + nb - 1; rows[i] / cols[j] = their tile row / column.  Entry e < na nb of the record is
// (i, j) = (e mod na, e div na), e div na = (e * na_inv) >> 16 (exact for e < 1024, na <= 64).
constexpr int kBigRecEntries = 1024;
struct BigChildRec {
  int64_t u_off;
  int32_t u_ld, a0, b0;
  uint16_t na, nb;
  uint32_t na_inv, pad;
  uint8_t rows[64], cols[64];
};

// a micro leaf (w <= 2, r <= 32, no children) folded into a tree-solve chain task: its L panel, first
// pivot, r | w << 8, the caller's indices of its two pivots, and the offset of its below rows' entries
// in the row table (LeafRow: gbuf position of the forward update entry, xi index of the row)
struct SolveLeaf {
  int64_t loff;
  int32_t f0, rw, p0, p1, roff, pad;
};
struct LeafRow {  // the device reads it as an int2
  int32_t g, row;
};

// k_root_solve's fronts (up to kRootArgs) by value: their shapes come with the launch instead of two
// dependent table loads (front id, then first / nrows / row_ptr / l_off) before the gather
constexpr int kRootArgs = 4;
struct RootArgs {
  int32_t n;
  int32_t s[kRootArgs], f0[kRootArgs], w[kRootArgs], r[kRootArgs];
  int64_t e0[kRootArgs], loff[kRootArgs];
};

enum LaunchKind { ASSEMBLE = 0, SMALL32 = 1, SMALL64 = 2, SMALL128 = 3, BIG_DIAG = 4, BIG_TRSM = 5, BIG_UPDATE = 6,
                  LB_BUILD = 7, LB_SYRK = 8, MICRO = 9, SMALL192 = 10, FTREE = 11, BIG_UPDATE128 = 12,
                  ASM_UPDATE = 13, BIG_DAG = 14 };
struct Launch {
  int kind;
  int step;       // panel step for BIG_DIAG / BIG_TRSM / BIG_UPDATE
  int64_t off;    // ASSEMBLE: first tile; SMALL*: front list in sched; BIG_*: (front, item) pairs in sched
  int nf;         // number of fronts (SMALL*)
  int64_t items;  // workgroups
  int64_t chunk0 = 0, nchunk = 0;  // ASSEMBLE: chunk range of the level
  double bytes = 0, flops = 0;       // staging traffic model / algorithmic work of the launch
  double alg = 0;                    // SURVEY 8(d) bytes of the columns the launch factorises
  double bytes2 = 0, flops2 = 0;     // ASSEMBLE: of the chunk pass
  bool lds = true;                   // SMALL*: some front is a leaf (assembled in LDS)
  int lds_bytes = 0;                 // SMALL*: dynamic LDS of the blocked kernel (largest front)
};
struct SolveLevel {
  int64_t tiny_off;  // fronts with r <= 32 (half a wave each)
  int ntiny;
  int64_t micro_off;  // fronts with r <= 32, w <= 2 (16 lanes each)
  int nmicro;
  double micro_bytes = 0, micro_flops = 0, micro_alg = 0;
  int64_t small_off;
  int nsmall;
  int64_t big_off;
  int nbig;
  int64_t gat_off;  // (front, 256-row chunk) pairs for k_fwd_gather
  int ngat;
  int64_t below_off;  // (front, panel | chunk << 16) pairs for k_bwd_below
  int nbelow;
  int64_t ftask_off;
  int nftask;
  int64_t btask_off;
  int nbtask;
  int small_lds = 0;  // dynamic LDS of the small-front solve kernels (largest panel, ld r | 1)
  double tiny_bytes = 0, tiny_flops = 0;
  double small_bytes = 0, small_flops = 0, big_bytes = 0, big_flops = 0, below_bytes = 0, gat_bytes = 0;
  // SURVEY 8(d) bytes per direction: 8 nnzL of the fronts' columns (big: diagonal block / below it)
  double tiny_alg = 0, small_alg = 0, big_alg = 0, below_alg = 0;
};

// The MADIPM_* environment variables of the LDL^T solver, read once (read_ldl_knobs).
struct LdlKnobs {
  int big_kpan = 4;         // BIG_KPAN: panels per deferred big-front update group (1..8)
  bool upd_split = true;    // UPD_SPLIT=0: one workgroup per k_big_upd128 tile (A/B)
  bool big_dag = true;      // BIG_DAG=0: one launch per panel step and kind (A/B)
  int big_solve_wg = 512;   // BIG_SOLVE_WG: persistent workgroups of the big-front solve kernels (>= 64)
  bool multi_big = true;    // MULTI_BIG=0: the multi-RHS solve takes its big fronts column after column (A/B)
  int fact_pipe = 1;        // FACT_PIPE=0: the barrier schedule, bitwise the same factor
  int pipe_fault = 0;       // DEBUG_PIPE_FAULT=1, tests: drop one hand-off (sticky error)
  int asm_src_cap = ldlconst::kAsmLdsSrc * ldlconst::kAsmLdsWinMax;  // DEBUG_ASM_SRC_CAP=<n>, tests: a smaller bound
  int lds_shrink = 0;       // DEBUG_LDS_SHRINK=<bytes>, tests: k_fact_tree's carve check sees that much less
  bool asm_lds_src = true;  // ASM_LDS_SRC=0: every tile through the chunk pass (A/B)
  int asm_lds_win = 0;      // ASM_LDS_WIN=<n>, tests: every tile of <= n windows on the LDS source path
  bool asm_stats = false;   // ASM_STATS (set): the source-path tile counts on stderr
  bool tree_solve = true;   // TREE_SOLVE=0: no k_fwd_tree / k_bwd_tree set (A/B)
  bool tree_debug = false, tree_debug_set = false;  // TREE_DEBUG=1: per-task stamps and shapes; set: the helper count
  bool dag_debug = false;   // DAG_DEBUG=1: per-task stamps of k_big_dag
  bool fold_help = true;    // FOLD_HELP=0: no fold helpers
  int fold_help_min = 3;    // FOLD_HELP_MIN: fronts of at least this many batches get a helper (>= 2)
  int fold_help_share = 2;  // FOLD_HELP_SHARE: the helper's share of the batches, in quarters (1..3)
  char root_async = 0;      // ROOT_ASYNC's first character: '0' off, '2' diagnostics
  bool root_asm_side = true;  // ROOT_ASM_SIDE=0: the roots' assembly tiles on the caller's stream
};
LdlKnobs read_ldl_knobs();

struct LaunchPlan {
  // front tables
  std::vector<int32_t> u_ld;     // SymbolicPlan::u_ld, 0 where a tree front's update block is packed lower
  std::vector<uint8_t> fs_img;   // 1: fscratch holds the front's LDS image
  hvec<int32_t> g_src32;         // g_src narrowed (valid when g32_fits)
  bool g32_fits = false;
  std::vector<BigChildRec> brec;
  std::vector<SymbolicPlan::AsmTile> atiles;  // bt0 / bt1 renumbered to brec, LDS-source tiles rewritten
  std::vector<int32_t> g_ptr;
  std::vector<int64_t> chunk_ids, asm_cid_off;  // chunk-path chunks; per assembly group: its range in chunk_ids
  std::vector<int32_t> bigslot;
  int nbigslot = 0;
  // sharding (unsharded: xoff = -1, every x written, every column counted)
  std::vector<int64_t> xoff, topcol;
  std::vector<uint8_t> wout, colmask;
  std::vector<int32_t> gidx;
  int64_t gper = 0, xpack_tri = 0;
  // batched leaf columns
  std::vector<int32_t> lb_gid, lb_xrow;
  std::vector<int64_t> lb_poff;
  int64_t lb_npart = 0;
  std::vector<std::vector<int>> lb_at_level;
  // factorisation tree (k_fact_tree): tickets = nfhelp helpers, then nftree fronts
  std::vector<int32_t> ft_order, ft_dptr, ft_dep, fold_help;
  std::vector<FoldStart> fstart;
  std::vector<FoldHelp> fhelp;
  std::vector<uint16_t> fimg_dst;
  std::vector<int64_t> ab_loff;
  int64_t fimg_size = 0;
  int nftree = 0, nfhelp = 0, ftree_lds = 0, lds_cap = 0;
  double ftree_bytes = 0, ftree_flops = 0, ftree_alg = 0;
  // factorisation launches: phase 1 (this shard's subtrees; everything unsharded), phase 2 (top)
  std::vector<Launch> fact1, fact2;
  std::vector<int32_t> sched;
  std::vector<int32_t> dag_tasks, dag_dptr{0}, dag_dlist;  // DagTask words, CSR of dependencies (launch-local tickets)
  std::vector<int64_t> mslot;
  int64_t nmslot = 0;
  int64_t upd_np = 0, upd_nt = 0;  // k_big_upd128's split-K scratch: parts, tiles of the largest split launch
  // solves: per level, leaves first
  std::vector<SolveLevel> slev1, slev2;
  // multi-right-hand-side solve (unsharded plans): the levels of phase 1 with EVERY front in them, the
  // tree tasks' and the flat leaves' too; its lists follow the single solve's in sched / tasks
  std::vector<SolveLevel> mlev;
  std::vector<int32_t> tasks, flag_off, bp_off;
  int64_t nflags = 0, nbpart = 0;
  int64_t xg_off = 0;  // (top front, 256-row chunk) pairs of the external forward gather
  int nxg = 0;
  // tree solves
  std::vector<char> in_tree, sleaf;
  std::vector<int64_t> sv_src, upos;
  std::vector<uint16_t> sv_nt;
  std::vector<uint8_t> tchunk, trootbwd, rootf;  // rootf: roots solved by k_root_solve (1) / a k_fwd_tree task (2)
  std::vector<int32_t> tc_ptr, tc_list, tdep_ptr, tdep, tpar, tfront;
  std::vector<SolveLeaf> tleaf;
  std::vector<LeafRow> tlrow;
  RootArgs rargs{};
  int ntree = 0, ntask = 0, nroot_task = 0, root_lds = 0, tree_lds = 0;
  int64_t nsleaf = 0;
  double tree_bytes = 0, tree_flops = 0, tree_alg = 0, leaf_bytes = 0, leaf_flops = 0, leaf_alg = 0;
  // root tail, as far as the plan decides it (the constructor adds the process's and the device's say)
  bool tail_ok = false, asm_side = false, side_tree = false;
  size_t side0 = 0;
  int nroot_side = 0;
  std::vector<uint8_t> tside;
  std::string tail_diag;  // ROOT_ASYNC=2
};

void build_launch_plan(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P);

// SURVEY 8(d) bytes of front s: factorisation 8 nnzL + 12 nnzK of its columns; solve 8 nnzL
double fact_alg(const SymbolicPlan& S, int s);
double fact_alg_cols(const SymbolicPlan& S, int c0, int c1);
double solve_alg(const SymbolicPlan& S, int s);
double lb_alg(const SymbolicPlan& S, size_t g);  // solve bytes of a batched-leaf group: 8 nnzL of its members

// front classes of the planner
bool lb_member(const SymbolicPlan& S, int s);
bool in_phase(const SymbolicPlan& S, int s, int phase);
bool solve_small(const SymbolicPlan& S, int s);
bool solve_small_multi(const SymbolicPlan& S, int s);  // small in LaunchPlan::mlev

}  // namespace madipm
