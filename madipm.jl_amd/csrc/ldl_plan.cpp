// Launch planning of the multifrontal LDL^T: see ldl_plan.hpp.  Host arithmetic over SymbolicPlan only.
#include "ldl_plan.hpp"

#include <algorithm>
#include <array>
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <thread>

#include "common.hpp"

namespace madipm {
using namespace ldlconst;

LdlKnobs read_ldl_knobs() {
  LdlKnobs K;
  auto env = [](const char* k) { return std::getenv(k); };
  auto off = [&](const char* k) {  // A/B switches: off when the value starts with '0'
    const char* v = env(k);
    return v && v[0] == '0';
  };
  auto one = [&](const char* k) {
    const char* v = env(k);
    return v && v[0] == '1';
  };
  if (const char* e = env("MADIPM_BIG_KPAN")) K.big_kpan = std::max(1, std::min(8, std::atoi(e)));
  K.upd_split = !off("MADIPM_UPD_SPLIT");
  K.big_dag = !off("MADIPM_BIG_DAG");
  if (const char* e = env("MADIPM_BIG_SOLVE_WG")) K.big_solve_wg = std::max(64, std::atoi(e));
  K.multi_big = !off("MADIPM_MULTI_BIG");
  K.fact_pipe = off("MADIPM_FACT_PIPE") ? 0 : 1;
  K.pipe_fault = one("MADIPM_DEBUG_PIPE_FAULT") ? 1 : 0;
  if (const char* e = env("MADIPM_DEBUG_ASM_SRC_CAP")) K.asm_src_cap = std::atoi(e);
  if (const char* e = env("MADIPM_DEBUG_LDS_SHRINK")) K.lds_shrink = std::atoi(e);
  K.asm_lds_src = !off("MADIPM_ASM_LDS_SRC");
  if (const char* e = env("MADIPM_ASM_LDS_WIN")) K.asm_lds_win = std::max(0, std::min(kAsmLdsWinMax, std::atoi(e)));
  K.asm_stats = env("MADIPM_ASM_STATS") != nullptr;
  K.tree_solve = !off("MADIPM_TREE_SOLVE");
  K.tree_debug = one("MADIPM_TREE_DEBUG");
  K.tree_debug_set = env("MADIPM_TREE_DEBUG") != nullptr;
  K.dag_debug = one("MADIPM_DAG_DEBUG");
  K.fold_help = !off("MADIPM_FOLD_HELP");
  if (const char* e = env("MADIPM_FOLD_HELP_MIN")) K.fold_help_min = std::max(2, std::atoi(e));
  if (const char* e = env("MADIPM_FOLD_HELP_SHARE")) K.fold_help_share = std::max(1, std::min(3, std::atoi(e)));
  if (const char* e = env("MADIPM_ROOT_ASYNC")) K.root_async = e[0];
  K.root_asm_side = !off("MADIPM_ROOT_ASM_SIDE");
  return K;
}

double fact_alg_cols(const SymbolicPlan& S, int c0, int c1) {
  double b = 0.0;
  for (int c = c0; c < c1; ++c) b += 8.0 * S.colcnt[c] + 12.0 * S.kcol[c];
  return b;
}
double lb_alg(const SymbolicPlan& S, size_t g) {
  const auto& G = S.lb[g];
  double b = 0.0;
  for (int64_t k = G.mem_off; k < G.mem_off + G.n; ++k) b += 8.0 * S.colcnt[S.lb_mem[k]];
  return b;
}
double fact_alg(const SymbolicPlan& S, int s) { return fact_alg_cols(S, S.first[s], S.first[s + 1]); }
double solve_alg(const SymbolicPlan& S, int s) {
  double b = 0.0;
  for (int c = S.first[s]; c < S.first[s + 1]; ++c) b += 8.0 * S.colcnt[c];
  return b;
}

bool lb_member(const SymbolicPlan& S, int s) { return !S.lb_of.empty() && S.lb_of[s] >= 0; }
// solve classes: fronts up to SMALL_SOLVE_MAX rows whose L panel fits in LDS take the one-launch
// workgroup-per-front kernels; larger ones the dependency-driven big-front kernels
bool solve_small(const SymbolicPlan& S, int s) {
  const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
  return r <= SMALL_SOLVE_MAX && 8 * (r | 1) * w <= 150 * 1024;
}
// multi-right-hand-side small class (LaunchPlan::mlev): the panel and MULTI_W staged columns of
// SMALL_SOLVE_MAX doubles share the workgroup's LDS
bool solve_small_multi(const SymbolicPlan& S, int s) {
  const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
  return solve_small(S, s) && 8 * (r | 1) * w + 8 * MULTI_W * SMALL_SOLVE_MAX <= kWorkgroupLds;
}
bool in_phase(const SymbolicPlan& S, int s, int phase) {
  if (lb_member(S, s)) return false;  // batched leaves: W build + the parent's SYRK + GEMV solves
  return phase == 1 ? (!S.top(s) && S.mine(s)) : S.top(s);
}

namespace {

int64_t tree_panel_doubles(const SymbolicPlan& S, int s) {  // max(forward row-major, backward col-major) staged panel
  const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
  const int ldt = ((w + 15) & ~15) + 2, ldc = ((r + 31) & ~31) + 2;
  return std::max<int64_t>((int64_t)r * ldt, (int64_t)w * ldc);
}

void align2(std::vector<int32_t>& sched) {
  if (sched.size() & 1) sched.push_back(0);
}

// ------------------------------------------------------------------ front tables
void plan_front_tables(const SymbolicPlan& S, LaunchPlan& P) {
  // a small tree front whose parent is a tree front stores its update block packed lower
  // (u (u + 1) / 2, column-major; u_ld 0 on the device): written by k_fact_tree's write-out and read
  // only by its tree parent's push (or a medium parent's add) — about half the square block's lines
  P.u_ld = S.u_ld;
  for (int f = 0; f < S.nsuper; ++f) {
    const int p = S.parent[f];
    if (!S.ftree.empty() && S.ftree[f] && S.nrows[f] <= SymbolicPlan::kFactTreeMax && p >= 0 && S.ftree[p] &&
        S.nrows[f] > S.first[f + 1] - S.first[f])
      P.u_ld[f] = 0;
  }
  {
    // int32 sources when every arena / K index fits (leaf update blocks stay materialised: forming
    // them from the leaves' L panels in the gather was measured slower, r1 — 6 scattered loads per
    // source instead of 1)
    // (the check and the narrowing on the analysis threads: ~170 M sources on neos)
    const int64_t ns = (int64_t)S.g_src.size();
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(analysis_threads(), ns / 4000000));
    hvec<int32_t>& g32 = P.g_src32;
    g32.resize(ns);
    std::atomic<bool> fits{ns > 0};
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        const int64_t q0 = ns * t / T, q1 = ns * (t + 1) / T;
        bool ok = true;
        for (int64_t q = q0; q < q1; ++q) {
          const int64_t v = S.g_src[q];
          ok = ok && v >= INT32_MIN && v < (1LL << 30);
          g32[q] = (int32_t)v;
        }
        if (!ok) fits = false;
      });
    for (auto& x : th) x.join();
    P.g32_fits = fits;
  }
  {
    // fronts staged into LDS by k_fact_tree (all sizes) and k_small_blocked (r > 32, not big, not a
    // batched-leaf parent, whose SYRK writes ld r) are pre-assembled as their LDS image
    P.fs_img.assign(std::max<size_t>(S.nrows.size(), 1), 0);
    std::vector<uint8_t> lbpar(S.nrows.size(), 0);
    for (const auto& G : S.lb) lbpar[G.parent] = 1;
    for (size_t f = 0; f < S.nrows.size(); ++f)
      P.fs_img[f] = (S.fs_off[f] >= 0 &&
                     (S.ftree[f] ? !S.absorb[f] : (!S.is_big[f] && !lbpar[f] && S.nrows[f] > 32))) ? 1 : 0;
  }
  P.bigslot.assign(std::max(S.nsuper, 1), -1);
  for (int s = 0; s < S.nsuper; ++s)
    if (S.is_big[s]) P.bigslot[s] = P.nbigslot++;
}

// ------------------------------------------------------------------ assembly records, LDS-source rewrite
void plan_assembly(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P) {
  // big-child records of the assembly tiles (BigChildRec): a bt entry's block, split into column
  // ranges of <= kBigRecEntries entries; the tiles' bt0 / bt1 renumbered to the records
  const int64_t nb = (int64_t)S.bt.size() / 5;
  std::vector<int64_t> rptr(nb + 1, 0);
  for (int64_t k = 0; k < nb; ++k) {
    const int32_t* e = &S.bt[5 * k];
    const int na = e[4] - e[3], nbt = e[2] - e[1], cpr = kBigRecEntries / na;
    MADIPM_REQUIRE(na >= 1 && na <= 64 && nbt >= 1 && nbt <= 64, "assembly: big-child block outside its tile");
    rptr[k + 1] = rptr[k] + (nbt + cpr - 1) / cpr;
  }
  MADIPM_REQUIRE(rptr[nb] < INT32_MAX, "assembly: too many big-child records");
  std::vector<BigChildRec>& br = P.brec;
  br.resize(std::max<int64_t>(rptr[nb], 1));
  const int T = (int)std::min<int64_t>(analysis_threads(), std::max<int64_t>(1, nb / 4096));
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      for (int64_t k = t; k < nb; k += T) {
        const int32_t* e = &S.bt[5 * k];
        const int c = e[0], b0 = e[1], b1 = e[2], a0 = e[3], a1 = e[4];
        const int32_t* rel = S.rel.data() + S.rel_ptr[c];
        const int I0 = rel[a0] & ~63, J0 = rel[b0] & ~63;
        const int na = a1 - a0, cpr = kBigRecEntries / na;
        for (int64_t q = rptr[k]; q < rptr[k + 1]; ++q) {
          BigChildRec& R = br[q];
          R = BigChildRec{};
          R.u_off = S.u_off[c];
          R.u_ld = S.u_ld[c];
          R.a0 = a0;
          R.b0 = b0 + (int)(q - rptr[k]) * cpr;
          R.na = (uint16_t)na;
          R.nb = (uint16_t)std::min(cpr, b1 - R.b0);
          R.na_inv = (65536u + na - 1) / na;
          for (int i = 0; i < na; ++i) R.rows[i] = (uint8_t)(rel[a0 + i] - I0);
          for (int j = 0; j < R.nb; ++j) R.cols[j] = (uint8_t)(rel[R.b0 + j] - J0);
        }
      }
    });
  for (auto& x : th) x.join();
  std::vector<SymbolicPlan::AsmTile>& at = P.atiles;
  at = S.atiles;
  for (auto& a : at) {
    a.bt0 = (int32_t)rptr[a.bt0];
    a.bt1 = (int32_t)rptr[a.bt1];
    // the tile's nonempty-entry count rides in gptr's top 16 bits (asm_chunks_lds: no load of it)
    MADIPM_REQUIRE(a.gptr < ((int64_t)1 << 47), "assembly: entry list offset past 2^47");
    if (a.gptr >= 0) a.gptr |= (int64_t)S.g_ptr[a.gptr] << 48;
  }
  // Tiles of <= kAsmLdsWin windows of sources sum them from LDS (asm_chunks_lds): their entry lists point at
  // sources (pos | first source << 12, then the count << 12), gptr bit 47 set, gchk = the first
  // source | the count << 48; the chunk pass keeps only the other tiles' chunks (chunk_ids, per
  // assembly group).  MADIPM_ASM_LDS_SRC=0: every tile through the chunk pass (A/B).
  const bool lds_src = K.asm_lds_src;
  const int force_win = K.asm_lds_win;  // tests: every tile of <= n windows on the LDS source path (no launch-size rule)
  std::vector<int32_t>& gp2 = P.g_ptr;
  gp2 = S.g_ptr;
  std::vector<int64_t>& cids = P.chunk_ids;
  int64_t st_lds = 0, st_multi = 0, st_straddle = 0, st_chunk = 0, st_nsmax = 0;  // MADIPM_ASM_STATS
  P.asm_cid_off.assign(S.atile_lev.size(), 0);
  for (size_t g = 0; g + 1 < S.atile_lev.size(); ++g) {
    P.asm_cid_off[g] = (int64_t)cids.size();
    for (int32_t t = S.atile_lev[g]; t < S.atile_lev[g + 1]; ++t) {
      const SymbolicPlan::AsmTile& a0 = S.atiles[t];
      if (a0.gptr < 0) continue;
      const int32_t ne = S.g_ptr[a0.gptr];
      const int64_t nchk = S.g_ptr[a0.gptr + ne + 1] >> 12, cb = a0.gchk;
      const int64_t sb = S.g_chunk[cb], ns = S.g_chunk[cb + nchk] - sb;
      // one window in k_assemble's launches of < 256 tiles (LDLSolver::run_fact's one-tile-per-CU
      // instance), kAsmLdsWin elsewhere (k_asm_update: the tiles past the group's fused-front mark)
      const int32_t aend = (int)g < S.nlevels ? S.atile_fz1[g] : S.atile_lev[g + 1];
      const int64_t nwin = force_win ? force_win : (t < aend && aend - S.atile_lev[g] < 256) ? 1 : kAsmLdsWin;
      if (lds_src && ns <= kAsmLdsSrc * nwin && sb < ((int64_t)1 << 48)) {
        for (int32_t k = 0; k < ne; ++k) {
          const int32_t e = S.g_ptr[a0.gptr + 1 + k];
          gp2[a0.gptr + 1 + k] = (e & 4095) | (int32_t)((S.g_chunk[cb + (e >> 12)] - sb) << 12);
        }
        gp2[a0.gptr + ne + 1] = (int32_t)(ns << 12);
        at[t].gptr |= (int64_t)1 << 47;
        at[t].gchk = sb | (ns << 48);
        ++st_lds;
        st_multi += ns > kAsmLdsSrc;
        st_nsmax = std::max(st_nsmax, ns);
        for (int32_t k = 0; k < ne; ++k) {  // entries whose sources cross a window boundary
          const int64_t a = gp2[a0.gptr + 1 + k] >> 12, b = gp2[a0.gptr + 2 + k] >> 12;
          st_straddle += b > a && a / kAsmLdsSrc != (b - 1) / kAsmLdsSrc;
        }
      } else {
        for (int64_t c = cb; c < cb + nchk; ++c) cids.push_back(c);
        ++st_chunk;
      }
    }
  }
  P.asm_cid_off.back() = (int64_t)cids.size();
  if (K.asm_stats)
    fprintf(stderr, "asm lds-src: tiles %lld (multi-window %lld, straddling entries %lld, max sources %lld)  chunk-path tiles %lld\n",
            (long long)st_lds, (long long)st_multi, (long long)st_straddle, (long long)st_nsmax, (long long)st_chunk);
}

// ------------------------------------------------------------------ sharding, tree-solve set, batched leaves
void plan_sharding(const SymbolicPlan& S, LaunchPlan& P) {
  const int ns = S.nsuper;
  P.xoff.assign(std::max(ns, 1), -1);
  P.wout.assign(std::max(ns, 1), 1);
  P.colmask.assign(std::max(S.N, 1), 1);
  if (S.nshards <= 1) return;
  // solution exchange: every shard writes the top x it computes redundantly; the subtree x are
  // all-gathered by shard slices (the partition is shard-independent, so every shard knows them all)
  std::vector<std::vector<int32_t>> own(S.nshards);
  for (int s = 0; s < ns; ++s) {
    P.xoff[s] = S.xoff[s];
    for (int j = S.first[s]; j < S.first[s + 1]; ++j) {
      P.colmask[j] = S.top(s) ? 2 : (S.mine(s) ? 1 : 0);
      if (!S.top(s)) own[S.owner[s]].push_back(S.perm[j]);
    }
  }
  for (const auto& o : own) P.gper = std::max<int64_t>(P.gper, (int64_t)o.size());
  P.gper = std::max<int64_t>(P.gper, 1);
  P.gidx.assign((size_t)(S.nshards * P.gper), -1);
  for (int q = 0; q < S.nshards; ++q) std::copy(own[q].begin(), own[q].end(), P.gidx.begin() + q * P.gper);
  // exchange buffer: the top fronts' lower triangles (column by column) + 4 status slots per shard
  int64_t po = 0;
  for (int s = 0; s < ns; ++s)
    if (S.top(s)) {
      const int64_t r = S.nrows[s];
      for (int64_t c = 0; c < r; ++c) {
        P.topcol.insert(P.topcol.end(), {S.l_off[s] + c * r + c, po, r - c});
        po += r - c;
      }
    }
  P.xpack_tri = po;
}

void plan_tree_sets(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P) {
  const int ns = S.nsuper;
  // tree solve set (k_fwd_tree / k_bwd_tree); MADIPM_TREE_SOLVE=0 disables it (A/B measurements)
  std::vector<char>& in_tree = P.in_tree;
  in_tree.assign(std::max(ns, 1), 0);
  {
    const bool on = K.tree_solve;
    std::vector<char> lbpar(std::max(ns, 1), 0);
    for (const auto& G : S.lb) lbpar[G.parent] = 1;
    auto preleaf = [&](int c) { return S.child_ptr[c] == S.child_ptr[c + 1] && S.nrows[c] <= 32; };
    // fronts whose whole panel (+ 8 KB of gather staging) does not fit TREE_SOLVE_LDS, medium fronts
    // (SMALL_SOLVE_MAX < r <= MED_SOLVE_MAX) included, join with their panel streamed in chunks
    for (int s = 0; on && s < ns; ++s) {  // postorder: children first
      if (!in_phase(S, s, 1) || preleaf(s) || lbpar[s] || S.nrows[s] > MED_SOLVE_MAX) continue;
      bool ok = true;
      for (int q = S.child_ptr[s]; q < S.child_ptr[s + 1] && ok; ++q) {
        const int c = S.child_list[q];
        ok = in_tree[c] || (preleaf(c) && in_phase(S, c, 1));
      }
      in_tree[s] = ok;
    }
  }
  // micro leaves (w <= 2, r <= 32, no children) under tree fronts, solved from precomputed leaf records
  // (SolveLeaf) by the flat k_fwd_leaves / k_bwd_leaves launches (r3: solving them inside the tree tasks,
  // or their backward only, measured slower: 1478 vs 1534 iters/s)
  P.sleaf.assign(std::max(ns, 1), 0);
  for (int c = 0; c < ns; ++c) {
    const int p = S.parent[c];
    P.sleaf[c] = p >= 0 && in_tree[p] && in_phase(S, c, 1) && S.child_ptr[c] == S.child_ptr[c + 1] && S.nrows[c] <= 32 &&
                 S.first[c + 1] - S.first[c] <= 2;
  }
}

void plan_leaf_batches(const SymbolicPlan& S, LaunchPlan& P) {
  P.lb_at_level.assign(std::max(S.nlevels, 1), {});
  if (S.lb.empty()) return;
  P.lb_gid.resize(S.lb_mem.size());
  for (size_t g = 0; g < S.lb.size(); ++g) {
    const auto& G = S.lb[g];
    for (int j = 0; j < G.n; ++j) P.lb_gid[G.mem_off + j] = (int32_t)g;
    for (int k = 0; k < G.m; ++k) P.lb_xrow.push_back(S.rows[S.row_ptr[G.parent] + S.lb_gpos[G.gpos_off + k]]);
    P.lb_poff.push_back(P.lb_npart);
    P.lb_npart += (int64_t)cdiv(G.n, LBF_COLS) * G.m;
    P.lb_at_level[S.level[G.parent]].push_back((int)g);
  }
}

// ------------------------------------------------------------------ factorisation tree (k_fact_tree)
void plan_fact_tree(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P) {
  P.ft_order = S.ft_order;  // ticket order (SymbolicPlan::ft_order)
  const std::vector<int32_t>& ord = P.ft_order;
  std::vector<int32_t>&dptr = P.ft_dptr, &dl = P.ft_dep;
  dptr = {0};
  P.nftree = (int)ord.size();
  for (int s : ord) {
    for (int q = S.child_ptr[s]; q < S.child_ptr[s + 1]; ++q)
      if (S.ftree[S.child_list[q]]) dl.push_back(S.child_list[q]);
    dptr.push_back((int32_t)dl.size());
    const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
    const bool sq = r <= 128 && !S.fold_pk[s];
    if (r > SymbolicPlan::kFactTreeMax)  // medium front: one panel (r | 1) x min(64, w) in LDS
      P.ftree_lds = std::max<int>(P.ftree_lds, 8 * (((r | 1) * std::min(64, w) + 1) & ~1));
    else
      P.ftree_lds = std::max<int>(P.ftree_lds, (sq ? 8 * ((r * (r | 1) + 1) & ~1) : 8 * ((r * (r + 1) / 2 + 1) & ~1)) +
                                                   (S.absorb[s] ? SymbolicPlan::kFoldRowBytes * S.fold_rmax[s] +
                                                                      SymbolicPlan::kFoldLeafBytes * S.fold_lmax[s]
                                                                : 0));
    // folded leaves: their K entries read, their L entries written
    for (int k = S.absorb[s] ? S.mc_ptr[s] : 0; k < (S.absorb[s] ? S.mc_ptr[s + 1] : 0); ++k) {
      const int c = S.mc_list[k];
      const double rc = S.nrows[c], wc = S.first[c + 1] - S.first[c];
      P.ftree_bytes += 12.0 * (S.asm_ptr[c + 1] - S.asm_ptr[c]) + 8.0 * (rc * wc - wc * (wc - 1) / 2.0);
      P.ftree_alg += fact_alg(S, c);
      for (int t = 0; t < (int)wc; ++t) P.ftree_flops += (rc - t - 1) * (rc - t);
    }
    // staging model: the stored lower trapezoid of the panel written and the front's scatter list
    // read (ftree_bytes); SURVEY 8(d)'s algorithmic bytes (B_fact = 8 nnzL + 12 nnzK of the
    // front's columns, exact column counts) in ftree_alg
    P.ftree_bytes += 8.0 * (r * (double)w - w * (w - 1) / 2.0) + 12.0 * (double)(S.asm_ptr[s + 1] - S.asm_ptr[s]);
    P.ftree_alg += fact_alg(S, s);
    for (int t = 0; t < w; ++t) P.ftree_flops += (double)(r - t - 1) * (r - t);
  }
  if (K.tree_debug) {  // per-level front shapes
    std::map<int, std::array<double, 7>> lv;  // count, sum r, max r, sum w, sum lds, max lds, sum leaves
    for (int s : ord) {
      const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
      const bool sq = r <= 128 && !S.fold_pk[s];
      const double lds = (sq ? 8.0 * r * (r | 1) : 4.0 * r * (r + 1)) +
                         (S.absorb[s] ? SymbolicPlan::kFoldRowBytes * S.fold_rmax[s] + SymbolicPlan::kFoldLeafBytes * S.fold_lmax[s] : 0);
      auto& a = lv[S.level[s]];
      a[0] += 1, a[1] += r, a[2] = std::max<double>(a[2], r), a[3] += w, a[4] += lds, a[5] = std::max(a[5], lds);
      a[6] += S.absorb[s] ? S.mc_ptr[s + 1] - S.mc_ptr[s] : 0;
    }
    for (auto& [l, a] : lv)
      fprintf(stderr, "tree level %d: %4.0f fronts  r avg %.0f max %.0f  w avg %.1f  LDS avg %.0f max %.0f KB  leaves avg %.0f\n", l,
              a[0], a[1] / a[0], a[2], a[3] / a[0], a[4] / a[0] / 1024, a[5] / 1024, a[6] / a[0]);
  }
  // the device-side carve check compares against this (MADIPM_DEBUG_LDS_SHRINK=<bytes>, tests only:
  // pretend the launch has that much less, so the check fires)
  P.lds_cap = P.ftree_lds - K.lds_shrink;
  P.ab_loff.assign(S.mc_list.size() + 1, 0);
  for (size_t k = 0; k < S.mc_list.size(); ++k) P.ab_loff[k] = S.l_off[S.mc_list[k]];
}

FoldStart fold_start(const SymbolicPlan& S, int b0, int b1) {  // batches [b0, b1) and the first one's table entries
  FoldStart F{b0, b1, 0, 0, 0, 0, 0, 0, 0};
  if (b1 > b0) {
    F.kq0 = S.fold_bat[b0];
    F.kq1 = S.fold_bat[b0 + 1];
    F.row0 = S.fold_row0[b0];
    F.row1 = S.fold_row0[b0 + 1];
    F.poff = S.fold_poff[b0];
    F.plen = S.fold_plen[b0];
  }
  return F;
}

// the run-end entries of a batch's product chunks name every destination it writes (a parked
// continuation ends at its run's destination too): the image holds exactly those, ascending.
void fold_dests(const SymbolicPlan& S, int b0, int b1, std::vector<uint8_t>& mark, std::vector<uint16_t>& out) {
  for (int b = b0; b < b1; ++b) {
    const int64_t po = S.fold_poff[b];
    const int len = S.fold_plen[b];
    for (int t = 0; t < SymbolicPlan::kFoldThreads; ++t) {
      int d = (int)(S.fold_chead[(int64_t)b * SymbolicPlan::kFoldThreads + t] & 0xffffu);
      for (int k = 0; k < len; ++k) {
        const uint32_t e = S.fold_prod[po + (int64_t)SymbolicPlan::kFoldThreads * k + t];
        d += (int)((e >> 24) & 127u);
        if ((int32_t)e < 0) {
          MADIPM_REQUIRE(d >= 0 && d < 65536, "fold helper: LDS destination beyond 16 bits");
          if (!mark[d]) {
            mark[d] = 1;
            out.push_back((uint16_t)d);
          }
        }
      }
    }
  }
  std::sort(out.begin(), out.end());
  for (uint16_t x : out) mark[x] = 0;
}

// fold helpers: a front with two or more leaf batches hands the first half of them to a helper
// ticket (before every front's; the helpers with the most batches first), folds the rest itself
// and adds the helper's image after its waits (MADIPM_FOLD_HELP=0: no helpers)
void plan_fold_helpers(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P) {
  const int ns = S.nsuper;
  const bool on = K.fold_help;
  const int min_nb = K.fold_help_min;   // fronts of at least this many batches get a helper
  const int share4 = K.fold_help_share;  // the helper's share of the batches, in quarters
  std::vector<int32_t>& help = P.fold_help;
  help.assign(std::max(ns, 1), -1);
  std::vector<FoldStart>& fst = P.fstart;
  fst.assign(std::max(ns, 1), FoldStart{0, 0, 0, 0, 0, 0, 0, 0, 0});
  std::vector<FoldHelp>& hv = P.fhelp;
  std::vector<uint16_t>& hdst = P.fimg_dst;  // per helper: the sorted LDS destinations its batches' products reach
  int64_t img = 0;
  if (!S.fold_bptr.empty())
    for (int f = 0; f < ns; ++f) fst[f] = fold_start(S, S.fold_bptr[f], S.fold_bptr[f + 1]);
  std::vector<std::array<int, 3>> cand;  // (front, first batch, end of the helper's batches), ticket order
  for (int f : P.ft_order) {
    if (!on || !S.absorb[f]) continue;
    const int b0 = S.fold_bptr[f], nb = S.fold_bptr[f + 1] - b0;
    if (nb < min_nb) continue;
    cand.push_back({f, b0, b0 + std::max(1, std::min(nb - 1, nb * share4 / 4))});
  }
  // Helpers are independent: their lists are built on threads (marks over the 16-bit LDS space,
  // then the distinct ones sorted), then appended in ticket order.
  std::vector<std::vector<uint16_t>> cd(cand.size());
  {
    std::atomic<size_t> next{0};
    auto work = [&] {
      std::vector<uint8_t> mark(65536, 0);
      for (size_t k; (k = next.fetch_add(1)) < cand.size();) fold_dests(S, cand[k][1], cand[k][2], mark, cd[k]);
    };
    const int nt = std::max(1, std::min<int>(analysis_threads(), (int)(cand.size() / 8)));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
  }
  for (size_t k = 0; k < cand.size(); ++k) {
    const int64_t dofs = (int64_t)hdst.size();
    const int32_t nimg = (int32_t)cd[k].size();
    hdst.insert(hdst.end(), cd[k].begin(), cd[k].end());
    hv.push_back(FoldHelp{cand[k][0], 0, img, dofs, nimg, 0, fold_start(S, cand[k][1], cand[k][2])});
    img += (nimg + 1) & ~1LL;
  }
  std::stable_sort(hv.begin(), hv.end(),
                   [](const FoldHelp& a, const FoldHelp& b) { return a.fs.b1 - a.fs.b0 > b.fs.b1 - b.fs.b0; });
  P.nfhelp = (int)hv.size();
  for (int h = 0; h < P.nfhelp; ++h) {
    hv[h].flag = ns + h;
    help[hv[h].front] = h;
    fst[hv[h].front] = fold_start(S, hv[h].fs.b1, S.fold_bptr[hv[h].front + 1]);  // the front keeps the rest
  }
  P.fimg_size = img;
  if (K.tree_debug_set)
    fprintf(stderr, "fold helpers: %d, image entries %lld (%.1f MB per factorisation, stored + read)\n", P.nfhelp,
            (long long)hdst.size(), 16e-6 * (double)hdst.size());
  P.ft_dptr.insert(P.ft_dptr.begin(), (size_t)P.nfhelp, 0);  // dep_ptr by ticket: the helpers' ranges are empty
}

// ------------------------------------------------------------------ factorisation launch lists
// phase-1 level groups: the fused fronts' tiles past their column block 0 wait for k_asm_update
int32_t asm_end(const SymbolicPlan& S, int g) { return g < S.nlevels ? S.atile_fz1[g] : S.atile_lev[g + 1]; }

// Staging bytes of one assembly tile, added to `bytes`: the written entries (rmw = 2: read-modify-
// written) and the chunk sums' offsets (+ extra), then the big children's blocks.  Returns nr * nc.
double add_tile_bytes(const SymbolicPlan& S, const SymbolicPlan::AsmTile& at, double rmw, double per_rowcol, double& bytes) {
  const int r = S.nrows[at.front], ti = at.tij & 0xffff, tj = (at.tij >> 16) & 0x7fff;
  const double nr = std::min(64, r - 64 * ti), nc = std::min(64, r - 64 * tj);
  bytes += 8.0 * (ti == tj ? nr * (nr + 1) / 2 : nr * nc) * rmw + (at.gptr >= 0 ? 4.0 * (S.g_ptr[at.gptr] + 2) : 0.0) +
           8.0 * (nr + nc) * per_rowcol;
  for (int k = at.bt0; k < at.bt1; ++k) {
    const int32_t* e = &S.bt[5 * k];
    for (int b = e[1]; b < e[2]; ++b) bytes += 8.0 * std::max(0, e[4] - std::max(b, e[3]));
  }
  return nr * nc;
}

void asm_launch(const SymbolicPlan& S, const LaunchPlan& P, int g, std::vector<Launch>& out) {
  if (asm_end(S, g) <= S.atile_lev[g]) return;
  Launch L{ASSEMBLE, 0, S.atile_lev[g], 0, asm_end(S, g) - S.atile_lev[g], P.asm_cid_off[g],
           P.asm_cid_off[g + 1] - P.asm_cid_off[g]};  // the chunks of the group's chunk-path tiles
  // algorithmic traffic: chunk pass reads (index, value) per source, writes one partial per chunk;
  // the tile pass reads the entry offsets + partials (+ big-children blocks), writes the lower tile
  const int64_t nsrc = S.g_chunk[S.chunk_lev[g + 1]] - S.g_chunk[S.chunk_lev[g]];
  L.bytes2 = 16.0 * nsrc + 16.0 * L.nchunk;
  L.flops2 = (double)nsrc;
  for (int32_t t = S.atile_lev[g]; t < asm_end(S, g); ++t)
    add_tile_bytes(S, S.atiles[t], S.atiles[t].tij < 0 ? 2.0 : 1.0, 0.0, L.bytes);
  L.bytes += 8.0 * L.nchunk;
  out.push_back(L);
}

// the fused fronts' trailing tiles of a phase-1 level: assembled + updated after their panel (one
// launch): the written entries + the chunk sums' offsets + the panel rows of I and J (+ big children)
void asm_update_launch(const SymbolicPlan& S, int lev, std::vector<Launch>& out) {
  const int32_t t0 = S.atile_fz0[lev], t1 = S.atile_lev[lev + 1];
  if (t0 >= t1) return;
  Launch A{ASM_UPDATE, 0, t0, 4, t1 - t0};
  for (int32_t t = t0; t < t1; ++t) {
    const SymbolicPlan::AsmTile& at = S.atiles[t];
    const int f = at.front, w = S.first[f + 1] - S.first[f];
    A.nf = std::max(A.nf, (w + 3) & ~3);
    A.flops += 2.0 * add_tile_bytes(S, at, 1.0, w, A.bytes) * w;
  }
  out.push_back(A);
}

void lb_syrk_launch(const SymbolicPlan& S, int g, std::vector<Launch>& out) {
  const auto& G = S.lb[g];
  Launch L{LB_SYRK, 0, g, 0, 0};
  L.flops = (double)G.m * (G.m + 1) * (double)G.n;
  // W once + the parent's lower triangle read-modify-written once per K-chunk
  L.bytes = 8.0 * (double)G.m * G.n + 16.0 * (double)G.m * (G.m + 1) / 2.0 * cdiv(G.n, LB_KCHUNK);
  out.push_back(L);
}

// The big fronts of a level in one k_big_dag launch: tasks in ticket order DIAG(0) | chain(0) feed(0) |
// chain(1) bulk(0) feed(1) | chain(2) bulk(1) feed(2) | ... | bulk(last) (k_big_dag's comment), every
// front of the level interleaved; each task's dependencies are the last earlier writers of the 64 x 64
// blocks of its front that it reads or read-modify-writes (every writer also reads what it writes, so
// the last writer stands for all earlier ones).  Then the fused fronts' k_asm_update.  The same tiles,
// operands and order of sums as the per-step launches with K unsplit.
void dag_level(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P, const std::vector<int32_t>& big, int lev, int phase,
               std::vector<Launch>& out) {
  std::vector<int32_t>&dtask = P.dag_tasks, &ddptr = P.dag_dptr, &ddlist = P.dag_dlist;
  const int kp = K.big_kpan;
  Launch L{BIG_DAG, 0, (int64_t)(dtask.size() / 4), 0, 0};
  // per front, the live written rectangles bucketed by the 64 x 64 blocks they touch: a task depends on
  // every live rectangle its reads or read-modify-writes intersect; a write drops the rectangles (per
  // block) it covers — it depends on them, so it stands for them — and adds its own
  struct Ent {
    int r0, r1, c0, c1, w;
  };
  std::map<int, std::vector<std::vector<Ent>>> live;
  std::vector<int32_t> deps;
  std::vector<Ent> wr;
  std::vector<int> wrs;
  auto region = [&](int s, int r0, int r1, int c0, int c1, bool write) {
    const int nb = (int)cdiv(S.nrows[s], 64);
    auto& g = live[s];
    if (g.empty()) g.resize((size_t)nb * nb);
    r1 = std::min(r1, S.nrows[s]);
    c1 = std::min(c1, S.nrows[s]);
    if (r0 >= r1 || c0 >= c1) return;
    for (int R = r0 >> 6; R <= (r1 - 1) >> 6; ++R)
      for (int C = c0 >> 6; C <= std::min((c1 - 1) >> 6, R); ++C)
        for (const Ent& e : g[(size_t)R * nb + C])
          if (e.r0 < r1 && r0 < e.r1 && e.c0 < c1 && c0 < e.c1) deps.push_back(e.w);
    if (write) {
      wr.push_back(Ent{r0, r1, c0, c1, -1});
      wrs.push_back(s);
    }
  };
  auto emit = [&](int s, int step, int item, int kind) {
    const int t = (int)L.items++;
    std::sort(deps.begin(), deps.end());
    deps.erase(std::unique(deps.begin(), deps.end()), deps.end());
    for (int d : deps) ddlist.push_back(d);
    ddptr.push_back((int32_t)ddlist.size());
    for (size_t k = 0; k < wr.size(); ++k) {
      const Ent q{wr[k].r0, wr[k].r1, wr[k].c0, wr[k].c1, t};
      const int f = wrs[k], nb = (int)cdiv(S.nrows[f], 64);
      auto& g = live[f];
      for (int R = q.r0 >> 6; R <= (q.r1 - 1) >> 6; ++R)
        for (int C = q.c0 >> 6; C <= std::min((q.c1 - 1) >> 6, R); ++C) {
          auto& cell = g[(size_t)R * nb + C];
          const int br0 = R * 64, br1 = br0 + 64, bc0 = C * 64, bc1 = bc0 + 64;
          cell.erase(std::remove_if(cell.begin(), cell.end(), [&](const Ent& e) {
                       const int a0 = std::max(e.r0, br0), a1 = std::min(e.r1, br1);
                       const int b0 = std::max(e.c0, bc0), b1 = std::min(e.c1, bc1);
                       return a0 >= q.r0 && a1 <= q.r1 && b0 >= q.c0 && b1 <= q.c1;  // covered here
                     }),
                     cell.end());
          cell.push_back(q);
        }
    }
    deps.clear();
    wr.clear();
    wrs.clear();
    dtask.insert(dtask.end(), {s, step, item, kind});
  };
  int maxsteps = 0;
  for (int s : big) maxsteps = std::max<int>(maxsteps, (int)cdiv(S.first[s + 1] - S.first[s], 64));
  // first diagonal blocks
  for (int s : big) {
    const int w = S.first[s + 1] - S.first[s], kw = std::min(64, w);
    region(s, 0, kw, 0, kw, true);
    emit(s, 0, 0, 3);
    L.bytes += 8.0 * (kw * (kw + 1.0) + 4 * 16 * 17);
    L.flops += (double)kw * kw * kw / 3.0;
  }
  for (int s : big) L.alg += fact_alg(S, s);  // every column of the level's big fronts
  auto bulk = [&](int g0) {  // 128 x 128 trailing tiles of group [g0, g0 + kp), columns past the feed tiles
    for (int s : big) {
      const int w = S.first[s + 1] - S.first[s], r = S.nrows[s];
      if ((int)cdiv(w, 64) <= g0 || S.fused[s]) continue;
      const int gend = std::min(64 * (g0 + kp), w), cb = gend + 64 * kp;
      if (cb >= r) continue;
      const int nt = (int)cdiv(r - cb, 128);
      const double K = gend - 64 * g0, nbt = r - cb;
      L.bytes += 8.0 * (nbt * (nbt + 1) + 2.0 * nbt * K);
      L.flops += K * nbt * (nbt + 1);
      // column by column: the first columns feed the next group's feed tiles (and its bulk's first
      // columns), so their tickets come first and are done by the time those wait for them
      for (int J = 0; J < nt; ++J)
        for (int I = J; I < nt; ++I) {
          const int i0 = cb + 128 * I, j0 = cb + 128 * J;
          region(s, i0, i0 + 128, 64 * g0, gend, false);  // (L D)_I and L_J: the group's panels
          region(s, j0, j0 + 128, 64 * g0, gend, false);
          region(s, i0, i0 + 128, j0, j0 + 128, true);
          emit(s, g0 + kp - 1, I | (J << 16), 2);
        }
    }
  };
  for (int g0 = 0; g0 < maxsteps; g0 += kp) {
    // chain, per step: the critical tasks of every front first — trsm tiles 0 and 1 and the updates of
    // tiles (0, 0) (with the next diagonal block), (1, 0) and (1, 1), which the next step's first
    // tasks wait for — then the other trsm tiles and local updates
    for (int p = g0; p < std::min(g0 + kp, maxsteps); ++p)
      for (int phase2 = 0; phase2 < 2; ++phase2)
        for (int kind = 0; kind < 2; ++kind)
          for (int s : big) {
            const int w = S.first[s + 1] - S.first[s], r = S.nrows[s];
            const int npan = (int)cdiv(w, 64);
            if (npan <= p) continue;
            const int k0 = p * 64, kw = std::min(64, w - k0);
            const int nt = (int)cdiv(r - k0 - kw, 64);
            const double dk = kw, nb = r - k0 - kw;
            const int gl = std::min(g0 + kp, npan) - 1, gend = std::min(64 * (gl + 1), w);
            const bool local = !S.fused[s] && p < gl;  // local updates (then kw = 64, c0 = k0 + 64)
            const int c0 = k0 + 64;
            const int ncol = local ? (int)cdiv(gend - c0, 64) : 0;
            auto trsm = [&](int rt) {
              const int R0 = k0 + kw + 64 * rt;
              region(s, k0, k0 + kw, k0, k0 + kw, false);  // L11, D, M_K
              region(s, R0, R0 + 64, k0, k0 + kw, true);
            };
            auto upd = [&](int i, int j) {
              region(s, c0 + 64 * i, c0 + 64 * i + 64, k0, k0 + 64, false);
              region(s, c0 + 64 * j, c0 + 64 * j + 64, k0, k0 + 64, false);
              region(s, c0 + 64 * i, c0 + 64 * i + 64, c0 + 64 * j, std::min(c0 + 64 * j + 64, gend), true);
            };
            const bool crit = phase2 == 0;
            if (kind == 0) {
              if (crit) {
                L.bytes += 8.0 * (2.0 * nb * dk + nt * (dk * (dk + 1) / 2 + 4 * 16 * 17));
                L.flops += nb * dk * dk;
                if (local) {
                  const double nc = gend - c0;
                  L.bytes += 8.0 * (2.0 * nb * nc + nb * dk + nc * dk);
                  L.flops += 2.0 * dk * nc * (nb - 0.5 * nc);
                }
              }
              for (int rt = crit ? 0 : 2; rt < (crit ? std::min(nt, 2) : nt); ++rt) {
                trsm(rt);
                emit(s, p, rt, 0);
              }
            } else if (local) {
              for (int j = 0; j < ncol; ++j)
                for (int i = j; i < nt; ++i) {
                  const bool c = (i == 1 && j <= 1) || (i == 0 && j == 0);
                  if (c != crit) continue;
                  upd(i, j);
                  emit(s, p, i | (j << 16), 1);
                }
            }
          }
    if (g0 > 0) bulk(g0 - kp);
    // feed: the trailing update of the next group's columns, 64 x 64 tiles (k_big_update trailing mode)
    for (int s : big) {
      const int w = S.first[s + 1] - S.first[s], r = S.nrows[s];
      if ((int)cdiv(w, 64) <= g0 || S.fused[s]) continue;
      const int gend = std::min(64 * (g0 + kp), w);
      if (gend >= r) continue;
      const int nt = (int)cdiv(r - gend, 64), ncb = std::min(kp, nt);
      const double K = gend - 64 * g0, nbt = r - gend, nc = std::min(64.0 * kp, nbt);
      L.bytes += 8.0 * (2.0 * nbt * nc + (nbt + nc) * K);
      L.flops += 2.0 * K * nc * (nbt - 0.5 * nc);
      for (int j = 0; j < ncb; ++j)
        for (int i = j; i < nt; ++i) {
          const int i0 = gend + 64 * i, j0 = gend + 64 * j;
          region(s, i0, i0 + 64, 64 * g0, gend, false);
          region(s, j0, j0 + 64, 64 * g0, gend, false);
          region(s, i0, i0 + 64, j0, j0 + 64, true);
          emit(s, g0 + kp - 1, (int)((uint32_t)i | ((uint32_t)j << 16) | 0x80000000u), 1);
        }
    }
  }
  bulk(((maxsteps - 1) / kp) * kp);
  out.push_back(L);
  if (phase == 1) asm_update_launch(S, lev, out);
}

// The big fronts of a level, one launch per panel step and kind (MADIPM_BIG_DAG=0).
void step_level(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P, const std::vector<int32_t>& big, int lev, int phase,
                std::vector<Launch>& out) {
  std::vector<int32_t>& sched = P.sched;
  int maxsteps = 0;
  for (int s : big) maxsteps = std::max<int>(maxsteps, (int)cdiv(S.first[s + 1] - S.first[s], 64));
  int64_t last_upd = -1;  // the latest update launch (it factorised the next step's diagonal blocks)
  for (int p = 0; p < maxsteps; ++p) {
    std::vector<int32_t> td, tt, tu, tu128;  // (front, item) pairs
    double kb[4] = {0, 0, 0, 0}, kf[4] = {0, 0, 0, 0}, ka = 0;
    for (int s : big) {
      const int w = S.first[s + 1] - S.first[s], r = S.nrows[s];
      const int npan = (int)cdiv(w, 64);
      if (npan <= p) continue;
      const int k0 = p * 64, kw = std::min(64, w - k0);
      const int nt = (int)cdiv(r - k0 - kw, 64);
      const double dk = kw, nb = r - k0 - kw;
      kb[0] += 8.0 * (dk * (dk + 1) + 4 * 16 * 17);  // diag: read + write lower, write the M blocks
      ka += fact_alg_cols(S, S.first[s] + k0, S.first[s] + k0 + kw);  // 8(d): the panel's columns
      kf[0] += dk * dk * dk / 3.0;
      kb[1] += 8.0 * (2.0 * nb * dk + nt * (dk * (dk + 1) / 2 + 4 * 16 * 17));  // trsm: rows in/out + L11, M per tile
      kf[1] += nb * dk * dk;
      if (p == 0) td.insert(td.end(), {s, 0});  // later panels: the previous update's task (0, 0)
      for (int i = 0; i < nt; ++i) tt.insert(tt.end(), {s, i});
      if (S.fused[s]) continue;  // its trailing update: k_asm_update (below)
      // deferred multi-panel update (k_big_update): panel groups of big_kpan panels; inside a
      // group each panel updates the group's later panels only (local tiles), the group's last
      // panel updates the rest of the front with K = the whole group (trailing tiles)
      const int g0 = (p / K.big_kpan) * K.big_kpan, gl = std::min(g0 + K.big_kpan, npan) - 1;
      const int gend = std::min(64 * (gl + 1), w);
      if (p < gl) {
        const double nc = gend - (k0 + kw);  // the group's later columns
        for (int j = 0; j < (int)cdiv((int)nc, 64); ++j)
          for (int i = j; i < nt; ++i) tu.insert(tu.end(), {s, i | (j << 16)});
        kb[2] += 8.0 * (2.0 * nb * nc + nb * dk + nc * dk);  // C in/out + the panel rows once
        kf[2] += 2.0 * dk * nc * (nb - 0.5 * nc);
      } else {  // 128 x 128 tiles (k_big_upd128)
        const int c0 = gend, ntt = (int)cdiv(r - c0, 128);
        const double KK = gend - 64 * g0, nbt = r - c0;
        for (int i = 0; i < ntt; ++i)
          for (int j = 0; j <= i; ++j) tu128.insert(tu128.end(), {s, i | (j << 16)});
        kb[3] += 8.0 * (nbt * (nbt + 1) + 2.0 * nbt * KK);  // C in/out once per group + the group's panels
        kf[3] += KK * nbt * (nbt + 1);
      }
    }
    const std::pair<int, std::vector<int32_t>*> kinds[4] = {
        {BIG_DIAG, &td}, {BIG_TRSM, &tt}, {BIG_UPDATE, &tu}, {BIG_UPDATE128, &tu128}};
    bool alg_done = false;  // the panels' 8(d) bytes ride on the step's first launch (k_big_diag at
                            // step 0, k_big_trsm after: the diagonal blocks are factorised by the
                            // previous step's update launch)
    for (int q = 0; q < 4; ++q) {
      const auto& kv = kinds[q];
      if (kv.second->empty()) continue;
      align2(sched);
      Launch L{kv.first, p, (int64_t)sched.size(), 0, (int64_t)kv.second->size() / 2};
      L.bytes = kb[q];
      L.alg = alg_done ? 0.0 : ka;
      alg_done = true;
      if (kv.first == BIG_UPDATE || kv.first == BIG_UPDATE128) last_upd = (int64_t)out.size();
      if (kv.first == BIG_UPDATE128)  // K split over 2-4 workgroups per tile when the tiles alone
                                      // would leave most CUs idle (k_big_upd128; nf = the split)
        L.nf = !K.upd_split ? 1 : L.items <= 128 ? 4 : L.items <= 170 ? 3 : L.items <= 256 ? 2 : 1;
      L.flops = kf[q];
      out.push_back(L);
      sched.insert(sched.end(), kv.second->begin(), kv.second->end());
    }
    // a last panel without rows below (r == w) launches nothing: its diagonal block was factorised
    // by the previous step's update launch, which carries its bytes
    if (!alg_done && ka > 0.0 && last_upd >= 0) out[last_upd].alg += ka;
    if (p == 0 && phase == 1) asm_update_launch(S, lev, out);
  }
}

void build_fact(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P, int phase, std::vector<Launch>& out) {
  const int NL = S.nlevels;
  std::vector<int32_t>& sched = P.sched;
  if (phase == 1 && !S.lb.empty()) {
    Launch L{LB_BUILD, 0, 0, 0, (int64_t)S.lb_mem.size()};
    for (const auto& G : S.lb) L.bytes += 8.0 * (double)G.m * G.n * 2.0 + 12.0 * G.n * G.m;
    for (int32_t c : S.lb_mem) L.alg += fact_alg_cols(S, c, c + 1);
    out.push_back(L);
  }
  auto ftree_launch = [&]() {  // factorisation tree: after every level-0 launch (the pre-leaves)
    asm_launch(S, P, 2 * NL + 1, out);
    Launch L{FTREE, 0, 0, P.nftree, (int64_t)P.nftree};
    L.bytes = P.ftree_bytes;
    L.alg = P.ftree_alg;
    L.flops = P.ftree_flops;
    L.lds_bytes = P.ftree_lds;
    out.push_back(L);
  };
  for (int lev = 0; lev < NL; ++lev) {
    if (phase == 1 && lev == 1 && P.nftree) ftree_launch();
    asm_launch(S, P, phase == 1 ? lev : NL + 1 + lev, out);
    if (phase == 1)
      for (int g : P.lb_at_level[lev])
        if (!S.top(S.lb[g].parent)) lb_syrk_launch(S, g, out);  // top parents: after their external part
    std::vector<int32_t> cls[4], big, micro;
    for (int q = S.level_ptr[lev]; q < S.level_ptr[lev + 1]; ++q) {
      const int s = S.level_list[q];
      if (!in_phase(S, s, phase) || S.ftree[s]) continue;
      if (S.parent[s] >= 0 && S.absorb[S.parent[s]]) continue;  // factorised by its absorbing parent
      const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
      if (r <= 32 && w <= 2 && S.fs_off[s] < 0 && !S.is_big[s])
        micro.push_back(s);
      else if (!S.is_big[s])
        cls[r <= 32 ? 0 : (r <= 64 ? 1 : (r <= 128 ? 2 : 3))].push_back(s);
      else
        big.push_back(s);
    }
    if (!micro.empty()) {
      Launch L{MICRO, 0, (int64_t)sched.size(), (int)micro.size(), (int64_t)micro.size()};
      for (int f : micro) {
        const double r = S.nrows[f], w = S.first[f + 1] - S.first[f];
        L.bytes += 8.0 * (r * w + (r - w) * (r - w + 1) / 2 + w) + 16.0 * (S.asm_ptr[f + 1] - S.asm_ptr[f]);
        L.alg += fact_alg(S, f);
        for (int t = 0; t < (int)w; ++t) L.flops += (r - t - 1) * (r - t);
      }
      out.push_back(L);
      sched.insert(sched.end(), micro.begin(), micro.end());
    }
    for (int c = 0; c < 4; ++c)
      if (!cls[c].empty()) {
        Launch L{c == 3 ? SMALL192 : SMALL32 + c, 0, (int64_t)sched.size(), (int)cls[c].size(), (int64_t)cls[c].size()};
        L.lds = false;
        for (int f : cls[c]) {
          L.lds = L.lds || S.fs_off[f] < 0;
          const int r = S.nrows[f];
          L.lds_bytes = std::max<int>(L.lds_bytes, c == 3 ? small_pk_lds(r) : small_sq_lds(r));
        }
        for (int f : cls[c]) {  // reads: K entries or the assembled front; writes: L panel, U block, D
          const double r = S.nrows[f], w = S.first[f + 1] - S.first[f];
          L.bytes += 8.0 * (r * w + (r - w) * (r - w) + w) +
                     (S.fs_off[f] >= 0 ? 8.0 * r * (r + 1) / 2 : 16.0 * (S.asm_ptr[f + 1] - S.asm_ptr[f]));
          L.alg += fact_alg(S, f);
          for (int t = 0; t < (int)w; ++t) L.flops += (r - t - 1) * (r - t);
        }
        out.push_back(L);
        sched.insert(sched.end(), cls[c].begin(), cls[c].end());
      }
    if (big.empty()) continue;
    (K.big_dag ? dag_level : step_level)(S, K, P, big, lev, phase, out);
  }
  if (phase == 1 && NL == 1 && P.nftree) ftree_launch();
}

void plan_fact(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P) {
  P.mslot.assign(std::max(S.nsuper, 1), 0);
  for (int f = 0; f < S.nsuper; ++f)
    if (S.is_big[f]) {
      P.mslot[f] = P.nmslot;
      P.nmslot += cdiv(S.first[f + 1] - S.first[f], 64) + 1;
    }
  build_fact(S, K, P, 1, P.fact1);
  if (S.nshards > 1) {
    asm_launch(S, P, S.nlevels, P.fact1);  // top fronts, external part (all-reduced next)
    for (size_t g = 0; g < S.lb.size(); ++g)  // this shard's batched leaves under top fronts: into it
      if (S.top(S.lb[g].parent)) lb_syrk_launch(S, (int)g, P.fact1);
    build_fact(S, K, P, 2, P.fact2);
  }
  // k_big_upd128's split-K scratch: partial products and per-tile tickets of the largest split launch
  for (const auto* V : {&P.fact1, &P.fact2})
    for (const Launch& L : *V)
      if (L.kind == BIG_UPDATE128 && L.nf > 1) {
        P.upd_np = std::max<int64_t>(P.upd_np, L.items * L.nf);
        P.upd_nt = std::max<int64_t>(P.upd_nt, L.items);
      }
}

// ------------------------------------------------------------------ solve levels
// per level, small fronts (wave per front) and big fronts (task queues).  multi (LaunchPlan::mlev): every
// front of the phase, the tree tasks' and the flat leaves' included; a front that is big in both lists keeps
// the bp_off the first list gave it
void build_solve(const SymbolicPlan& S, LaunchPlan& P, int phase, std::vector<SolveLevel>& out, bool multi = false) {
  std::vector<int32_t>&sched = P.sched, &tasks = P.tasks;
  std::vector<char> has_bp;
  if (multi) {
    has_bp.assign(std::max(S.nsuper, 1), 0);
    for (const SolveLevel& L : P.slev1)
      for (int k = 0; k < L.nbig; ++k) has_bp[sched[L.big_off + k]] = 1;
  }
  for (int lev = 0; lev < S.nlevels; ++lev) {
    std::vector<int32_t> tiny, small, big, micro;
    for (int q = S.level_ptr[lev]; q < S.level_ptr[lev + 1]; ++q) {
      const int s = S.level_list[q];
      if (!in_phase(S, s, phase) || (phase == 1 && !multi && (P.in_tree[s] || P.sleaf[s]))) continue;
      const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
      if (r <= 32 && w <= 2)
        micro.push_back(s);
      else if (solve_small(S, s) && (!multi || r <= 32 || solve_small_multi(S, s)))
        (r > 32 ? small : tiny).push_back(s);
      else
        big.push_back(s);
    }
    SolveLevel L{};
    L.micro_off = (int64_t)sched.size();
    L.nmicro = (int)micro.size();
    sched.insert(sched.end(), micro.begin(), micro.end());
    for (int f : micro) {
      const double r = S.nrows[f], w = S.first[f + 1] - S.first[f];
      L.micro_bytes += 8.0 * (r * w + 3.0 * r);
      L.micro_flops += 2.0 * (r * w - w * (w + 1) / 2);
      L.micro_alg += solve_alg(S, f);
    }
    L.tiny_off = (int64_t)sched.size();
    L.ntiny = (int)tiny.size();
    sched.insert(sched.end(), tiny.begin(), tiny.end());
    L.small_off = (int64_t)sched.size();
    L.nsmall = (int)small.size();
    sched.insert(sched.end(), small.begin(), small.end());
    L.big_off = (int64_t)sched.size();
    L.nbig = (int)big.size();
    sched.insert(sched.end(), big.begin(), big.end());
    align2(sched);
    L.gat_off = (int64_t)sched.size();
    for (int s : big)
      for (int c = 0; c < cdiv(S.nrows[s], GAT_ROWS); ++c) sched.insert(sched.end(), {s, c});
    L.ngat = (int)(((int64_t)sched.size() - L.gat_off) / 2);
    L.below_off = (int64_t)sched.size();
    for (int s : big) {
      const int w = S.first[s + 1] - S.first[s], r = S.nrows[s];
      if (r == w) continue;
      const int np = (int)cdiv(w, 64), nch = (int)cdiv(r - w, BWD_CHUNK);
      if (!multi || !has_bp[s]) {
        P.bp_off[s] = (int32_t)P.nbpart;
        P.nbpart += (int64_t)np * nch;
      }
      for (int p = 0; p < np; ++p)
        for (int c = 0; c < nch; ++c) sched.insert(sched.end(), {s, p | (c << 16)});
    }
    L.nbelow = (int)(((int64_t)sched.size() - L.below_off) / 2);
    int maxblk = 0, maxpan = 0;
    for (int s : big) {
      maxblk = std::max<int>(maxblk, (int)cdiv(S.nrows[s], 64));
      maxpan = std::max<int>(maxpan, (int)cdiv(S.first[s + 1] - S.first[s], 64));
    }
    L.ftask_off = (int64_t)tasks.size() / 2;
    for (int i = 0; i < maxblk; ++i)
      for (int s : big)
        if (i < cdiv(S.nrows[s], 64)) {
          tasks.push_back(s);
          tasks.push_back(i);
        }
    L.nftask = (int)((int64_t)tasks.size() / 2 - L.ftask_off);
    L.btask_off = (int64_t)tasks.size() / 2;
    for (int k = 0; k < maxpan; ++k)
      for (int s : big) {
        const int np = (int)cdiv(S.first[s + 1] - S.first[s], 64);
        if (k < np) {
          tasks.push_back(s);
          tasks.push_back(np - 1 - k);
        }
      }
    L.nbtask = (int)((int64_t)tasks.size() / 2 - L.btask_off);
    // algorithmic traffic of one sweep: the L panel once (+ the vectors), 2 flops per panel entry
    for (int f : small) {
      const double r = S.nrows[f], w = S.first[f + 1] - S.first[f];
      L.small_bytes += 8.0 * (r * w + 3.0 * r);
      L.small_flops += 2.0 * (r * w - w * (w + 1) / 2);
      L.small_alg += solve_alg(S, f);
      L.small_lds = std::max<int>(L.small_lds, 8 * (S.nrows[f] | 1) * (S.first[f + 1] - S.first[f]));
    }
    for (int f : tiny) {
      const double r = S.nrows[f], w = S.first[f + 1] - S.first[f];
      L.tiny_bytes += 8.0 * (r * w + 3.0 * r);
      L.tiny_flops += 2.0 * (r * w - w * (w + 1) / 2);
      L.tiny_alg += solve_alg(S, f);
    }
    for (int f : big) {
      const double r = S.nrows[f], w = S.first[f + 1] - S.first[f];
      L.big_bytes += 8.0 * (r * w + 3.0 * r);
      L.big_flops += 2.0 * (r * w - w * (w + 1) / 2);
      L.below_bytes += 8.0 * (r - w) * w;
      const double sa = solve_alg(S, f), da = std::min(sa, 4.0 * w * (w + 1));  // diagonal block / below it
      L.big_alg += da;
      L.below_alg += sa - da;
      L.gat_bytes += 8.0 * (2.0 * r + 2.0 * (S.sv_ptr[S.row_ptr[f + 1]] - S.sv_ptr[S.row_ptr[f]]));
    }
    out.push_back(L);
  }
}

// ------------------------------------------------------------------ tree-solve tables
// elimination-tree roots (r == w, no parent) whose panel needs more LDS than the tree launches'
// TREE_SOLVE_LDS (two workgroups per CU) go last, into their own forward launch with the LDS they
// need (ex10's 120-column coupling root: 125 KB), solved forward and backward there in one pass
// (r3: the root sized every tree task's LDS; r4's first cut streamed it in chunks: slower)
bool big_root(const SymbolicPlan& S, int s) {
  const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
  const int64_t need = 8 * tree_panel_doubles(S, s) + 8 * 1024;
  return S.parent[s] < 0 && r == w && r <= SMALL_SOLVE_MAX && need > TREE_SOLVE_LDS && need <= TREE_ROOT_LDS;
}

void plan_tree_solve(const SymbolicPlan& S, LaunchPlan& P) {
  const int ns = S.nsuper, NL = S.nlevels;
  const std::vector<char>& in_tree = P.in_tree;
  P.rootf.assign(std::max(ns, 1), 0);
  std::vector<int32_t> ord, roots;
  for (int lev = 0; lev < NL; ++lev)
    for (int q = S.level_ptr[lev]; q < S.level_ptr[lev + 1]; ++q)
      if (in_tree[S.level_list[q]]) (big_root(S, S.level_list[q]) ? roots : ord).push_back(S.level_list[q]);
  P.nroot_task = (int)roots.size();
  for (int s : roots) P.rootf[s] = 1;
  P.rargs.n = std::min(P.nroot_task, kRootArgs);
  for (int q = 0; q < P.rargs.n; ++q) {
    const int s = roots[q];
    P.rargs.s[q] = s;
    P.rargs.f0[q] = S.first[s];
    P.rargs.w[q] = S.first[s + 1] - S.first[s];
    P.rargs.r[q] = S.nrows[s];
    P.rargs.e0[q] = S.row_ptr[s];
    P.rargs.loff[q] = S.l_off[s];
  }
  ord.insert(ord.end(), roots.begin(), roots.end());
  P.ntree = (int)ord.size();
  // children of tree fronts scatter their forward update entries straight into the parent's
  // gather range (sv order, gbuf); everyone else keeps its own update vector (uvec)
  // each tree-front row's gather entries: those of fronts solved by earlier launches (the flat
  // leaves, batched-leaf groups, level-path children) first, those of tree tasks (this launch)
  // last, sv_nt[row] of them — k_fwd_tree sums the first part before it waits for its children
  std::vector<int64_t>& svs = P.sv_src;
  svs = S.sv_src;
  {
    std::vector<uint8_t> from_task((size_t)std::max<int64_t>(S.uvec_size, 1), 0);
    for (int s : ord)
      if (S.uvec_off[s] >= 0)
        for (int a = 0; a < S.nrows[s] - (S.first[s + 1] - S.first[s]); ++a) from_task[S.uvec_off[s] + a] = 1;
    std::vector<uint16_t>& nt = P.sv_nt;
    nt.assign((size_t)std::max<int64_t>(S.row_ptr[ns], 1), 0);
    std::vector<int64_t> tail;
    for (int s : ord)
      for (int i = 0; i < S.nrows[s]; ++i) {
        const int64_t t = S.row_ptr[s] + i, p0 = S.sv_ptr[t], p1 = S.sv_ptr[t + 1];
        tail.clear();
        int64_t o = p0;
        for (int64_t p = p0; p < p1; ++p)
          if (from_task[S.sv_src[p]])
            tail.push_back(S.sv_src[p]);
          else
            svs[o++] = S.sv_src[p];
        for (int64_t v : tail) svs[o++] = v;
        MADIPM_REQUIRE(tail.size() <= 65535, "tree solve: tree-task entries of one row beyond 16 bits");
        nt[t] = (uint16_t)tail.size();
      }
  }
  std::vector<int64_t> inv((size_t)std::max<int64_t>(S.uvec_size, 1), -1);
  std::vector<int64_t>& upm = P.upos;
  upm.assign((size_t)std::max<int64_t>(S.rel_ptr[ns], 1), -1);
  for (int s : ord)
    for (int64_t p = S.sv_ptr[S.row_ptr[s]]; p < S.sv_ptr[S.row_ptr[s] + S.nrows[s]]; ++p) inv[svs[p]] = p;
  for (int c = 0; c < ns; ++c)
    if (S.parent[c] >= 0 && in_tree[S.parent[c]])
      for (int64_t a = 0; a < S.rel_ptr[c + 1] - S.rel_ptr[c]; ++a) {
        upm[S.rel_ptr[c] + a] = inv[S.uvec_off[c] + a];
        MADIPM_REQUIRE(upm[S.rel_ptr[c] + a] >= 0, "tree gather map");
      }
  std::vector<uint8_t>& chunk = P.tchunk;
  chunk.assign(std::max(ns, 1), 0);
  for (int s : ord) {
    const double r = S.nrows[s], w = S.first[s + 1] - S.first[s];
    P.tree_bytes += 8.0 * (r * w + 3.0 * r);
    P.tree_flops += 2.0 * (r * w - w * (w + 1) / 2);
    P.tree_alg += solve_alg(S, s);
    chunk[s] = !big_root(S, s) && (S.nrows[s] > SMALL_SOLVE_MAX || 8 * tree_panel_doubles(S, s) + 8 * 1024 > TREE_SOLVE_LDS);
    if (big_root(S, s)) P.root_lds = std::max<int>(P.root_lds, 8 * tree_panel_doubles(S, s));  // k_root_solve: the panel
  }
  P.tree_lds = TREE_SOLVE_LDS;  // the rest of the budget stages gather sources
  // one task per tree front, in `ord` order (levels ascending): a task's forward dependencies (its
  // tree children) have earlier tickets, and in reverse order the backward one (its tree parent)
  // does.  (r3: chains of only-children solved back to back by one workgroup measured slower.)
  std::vector<int32_t>&cptr = P.tc_ptr, &clist = P.tc_list, &dptr = P.tdep_ptr, &dl = P.tdep, &tops = P.tfront;
  cptr = {0};
  dptr = {0};
  for (int s : ord) {
    clist.push_back(s);
    for (int q = S.child_ptr[s]; q < S.child_ptr[s + 1]; ++q)
      if (in_tree[S.child_list[q]]) dl.push_back(S.child_list[q]);
    cptr.push_back((int32_t)clist.size());
    dptr.push_back((int32_t)dl.size());
    tops.push_back(s);
  }
  // the flat leaf launches: every folded leaf, in postorder (L panels in order)
  std::vector<SolveLeaf>& lv = P.tleaf;
  std::vector<LeafRow>& lrow = P.tlrow;
  for (int c = 0; c < ns; ++c) {
    if (!P.sleaf[c]) continue;
    const int r = S.nrows[c], w = S.first[c + 1] - S.first[c], f0 = S.first[c];
    lv.push_back(SolveLeaf{S.l_off[c], f0, r | (w << 8), S.perm[f0], w == 2 ? S.perm[f0 + 1] : -1,
                           (int32_t)lrow.size(), 0});
    for (int a = 0; a < r - w; ++a) {
      const int64_t g = upm[S.rel_ptr[c] + a];
      MADIPM_REQUIRE(g >= 0 && g < INT32_MAX, "tree solve: folded leaf gather position");
      lrow.push_back(LeafRow{(int32_t)g, S.rows[S.row_ptr[c] + w + a]});
    }
  }
  P.ntask = (int)tops.size();
  {  // elimination-tree roots (r == w, no parent) solved backward by k_fwd_tree right after their forward
     // substitution, on the panel already in LDS (bitwise k_bwd_tree's x; r3: k_bwd_tree 52 -> 43 us)
    P.trootbwd.assign(std::max(P.ntask, 1), 0);
    for (int t = 0; t < P.ntask; ++t) {
      const int f = tops[t];
      P.trootbwd[t] = S.parent[f] < 0 && S.nrows[f] == S.first[f + 1] - S.first[f] && !chunk[f];
      if (P.trootbwd[t] && !P.rootf[f]) P.rootf[f] = 2;  // solved forward and backward by its k_fwd_tree task
    }
  }
  // backward ticket t -> task ntask - 1 - t: the tree parent of its top
  for (int t = P.ntask - 1; t >= 0; --t) {
    const int p = S.parent[tops[t]];
    P.tpar.push_back(p >= 0 && in_tree[p] ? p : -1);
  }
  P.nsleaf = (int64_t)lv.size();
  for (const SolveLeaf& L : lv) {
    const double r = L.rw & 255, w = L.rw >> 8;
    P.leaf_alg += 8.0 * (S.colcnt[L.f0] + (w == 2 ? S.colcnt[L.f0 + 1] : 0));
    P.leaf_bytes += 8.0 * (r * w + 3.0 * r) + 32.0 + 8.0 * (r - w);
    P.leaf_flops += 2.0 * (r * w - w * (w + 1) / 2);
  }
  lrow.push_back(LeafRow{0, 0});  // padding: the leaf kernels' clamped loads of a leaf without update rows
}

void plan_solve(const SymbolicPlan& S, LaunchPlan& P) {
  const int ns = S.nsuper;
  P.flag_off.assign(ns, 0);
  for (int s = 0; s < ns; ++s)
    if (!solve_small(S, s)) {
      P.flag_off[s] = (int32_t)P.nflags;
      P.nflags += cdiv(S.first[s + 1] - S.first[s], 64);
    }
  P.bp_off.assign(ns, 0);
  build_solve(S, P, 1, P.slev1);
  plan_tree_solve(S, P);
  if (S.nshards > 1) {
    build_solve(S, P, 2, P.slev2);
    align2(P.sched);
    P.xg_off = (int64_t)P.sched.size();
    for (int s = 0; s < ns; ++s)
      if (S.top(s))
        for (int c = 0; c < cdiv(S.nrows[s], NT); ++c) P.sched.insert(P.sched.end(), {s, c});
    P.nxg = (int)(((int64_t)P.sched.size() - P.xg_off) / 2);
  } else {
    // the multi-right-hand-side levels, after everything the single solve reads (no offset of it moves).  A
    // front that passes solve_small but not the multi small class's LDS test is big there and has no flags yet
    for (int s = 0; s < ns; ++s)
      if (S.nrows[s] > 32 && solve_small(S, s) && !solve_small_multi(S, s)) {
        P.flag_off[s] = (int32_t)P.nflags;
        P.nflags += cdiv(S.first[s + 1] - S.first[s], 64);
      }
    align2(P.sched);
    build_solve(S, P, 1, P.mlev, true);
  }
}

// ------------------------------------------------------------------ root tail
// the launches after the last tree launch factorise only k_root_solve's fronts
void plan_root_tail(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P) {
  const std::vector<Launch>& fact1 = P.fact1;
  size_t ft = SIZE_MAX;
  for (size_t i = 0; i < fact1.size(); ++i)
    if (fact1[i].kind == FTREE) ft = i;
  // after it: assembly launches, the last of which assembles the roots, then ONE factorisation
  // launch (SMALL*) of <= 64 roots, all of them solved by k_root_solve
  const size_t nl = fact1.size();
  bool ok = S.nshards == 1 && P.ntree > 0 && ft != SIZE_MAX && ft + 2 < nl && fact1[nl - 2].kind == ASSEMBLE;
  for (size_t i = ft + 1; ok && i + 1 < nl; ++i) ok = fact1[i].kind == ASSEMBLE;
  if (ok) {
    const Launch& L = fact1[nl - 1];
    ok = (L.kind == SMALL64 || L.kind == SMALL128 || L.kind == SMALL192) && L.items <= 64;
    for (int64_t k = 0; ok && k < L.items; ++k) ok = P.rootf[P.sched[L.off + k]] != 0;
  }
  P.tail_ok = ok;
  if (K.root_async == '2') {  // diagnostics: why (not)
    std::string k;
    for (const Launch& L : fact1) k += std::to_string(L.kind) + "/" + std::to_string(L.items) + " ";
    std::string rk;
    if (nl > 0)
      for (int64_t q = 0; q < std::min<int64_t>(fact1[nl - 1].items, 8); ++q) {
        const int f = P.sched[fact1[nl - 1].off + q];
        rk += std::to_string(f) + ":" + std::to_string(P.rootf[f]) + ":r" + std::to_string(S.nrows[f]) + " ";
      }
    P.tail_diag = "(roots " + std::to_string(P.nroot_task) + ", tree launch " +
                  std::to_string(ft == SIZE_MAX ? -1LL : (long long)ft) + ", launches kind/items: " + k +
                  "; last launch fronts " + rk + ")";
  }
  if (!ok) return;
  P.side0 = nl - 1;
  P.nroot_side = (int)fact1[nl - 1].items;
  // the roots' assembly tiles on the side stream too, behind the chunk pass's block flags
  // (MADIPM_ROOT_ASM_SIDE=0: on the caller's stream)
  P.asm_side = fact1[nl - 2].nchunk > 0 && K.root_asm_side;
  // the k_fwd_tree tasks of the side roots wait for the tail themselves (supportcase10's root)
  P.tside.assign(std::max(P.ntask, 1), 0);
  const Launch& L = fact1[nl - 1];
  for (int64_t k = 0; k < L.items; ++k) {
    const int f = P.sched[L.off + k];
    if (P.rootf[f] == 2)
      for (int t = 0; t < P.ntask; ++t)
        if (P.tfront[t] == f) P.tside[t] = 1, P.side_tree = true;
  }
}

}  // namespace

void build_launch_plan(const SymbolicPlan& S, const LdlKnobs& K, LaunchPlan& P) {
  PhaseClock clk("LDLSolver");
  P = LaunchPlan{};
  plan_front_tables(S, P);
  plan_assembly(S, K, P);
  plan_sharding(S, P);
  plan_tree_sets(S, K, P);
  plan_leaf_batches(S, P);
  clk("  front + assembly tables");
  plan_fact_tree(S, K, P);
  clk("  tree tables");
  plan_fold_helpers(S, K, P);
  clk("  fold helpers");
  plan_fact(S, K, P);
  clk("  build_fact + dag tables");
  plan_solve(S, P);
  plan_root_tail(S, K, P);
  clk("  tree solve tables + root tail");
}

}  // namespace madipm
