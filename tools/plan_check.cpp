// Runs the LDL^T launch planner on a CPU and checks its tables (csrc/ldl_plan.hpp; no GPU, no HIP call).
//
//   plan_check <pattern file>
// The file holds whitespace-separated integers: n nnz, colptr (n + 1), rowval (nnz) of the lower-
// triangular CSC pattern, then ordering relax small_front_max nshards shard.  The MADIPM_* environment
// applies as in the solver.  Exit status 1 with a message on the first violated invariant; otherwise
// one line per LaunchPlan array: "<class> <name> <count> <FNV-1a 64>" (classes: front, tree, solve,
// launch; the model sums as raw bits), then "info" lines: the fronts of the multi-right-hand-side levels (mlev) by
// level and class, and their class totals.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

#include "../madipm.jl_amd/csrc/ldl_plan.hpp"

using namespace madipm;
using namespace madipm::ldlconst;

namespace {

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  }
  template <class T>
  Fnv& operator<<(const T& v) {  // scalars only (no padding)
    bytes(&v, sizeof(T));
    return *this;
  }
};
template <class V>
void dump(const char* cls, const char* name, const V& v) {  // arrays of padding-free elements
  Fnv f;
  f.bytes(v.data(), v.size() * sizeof(v[0]));
  printf("%s %s %zu %016llx\n", cls, name, v.size(), (unsigned long long)f.h);
}
void dump(const char* cls, const char* name, const Fnv& f, size_t n = 1) {
  printf("%s %s %zu %016llx\n", cls, name, n, (unsigned long long)f.h);
}
Fnv hash_launches(const std::vector<Launch>& V) {
  Fnv f;
  for (const Launch& L : V)
    f << L.kind << L.step << L.off << L.nf << L.items << L.chunk0 << L.nchunk << L.bytes << L.flops << L.alg << L.bytes2
      << L.flops2 << (int)L.lds << L.lds_bytes;
  return f;
}
Fnv hash_levels(const std::vector<SolveLevel>& V) {
  Fnv f;
  for (const SolveLevel& L : V)
    f << L.tiny_off << L.ntiny << L.micro_off << L.nmicro << L.micro_bytes << L.micro_flops << L.micro_alg << L.small_off
      << L.nsmall << L.big_off << L.nbig << L.gat_off << L.ngat << L.below_off << L.nbelow << L.ftask_off << L.nftask
      << L.btask_off << L.nbtask << L.small_lds << L.tiny_bytes << L.tiny_flops << L.small_bytes << L.small_flops
      << L.big_bytes << L.big_flops << L.below_bytes << L.gat_bytes << L.tiny_alg << L.small_alg << L.big_alg << L.below_alg;
  return f;
}

[[noreturn]] void fail(const std::string& m) {
  fprintf(stderr, "plan_check: %s\n", m.c_str());
  exit(1);
}
#define CHECK(c, m) \
  if (!(c)) fail(std::string(m) + " [" #c "]")
std::string at(const std::string& what, long long i) { return what + " " + std::to_string(i); }

void check_plan(const SymbolicPlan& S, const LaunchPlan& P) {
  const int ns = S.nsuper;
  const int64_t nsched = (int64_t)P.sched.size(), ndag = (int64_t)P.dag_tasks.size() / 4;
  std::vector<int> nfact(std::max(ns, 1), 0), nsolve(std::max(ns, 1), 0);
  // ---- factorisation launches: DAG tasks, sched ranges, the fronts each launch factorises
  int64_t dag0 = 0;
  CHECK((int64_t)P.dag_dptr.size() == ndag + 1, "dag_dptr size");
  for (const auto* V : {&P.fact1, &P.fact2})
    for (size_t li = 0; li < V->size(); ++li) {
      const Launch& L = (*V)[li];
      const bool list = L.kind == MICRO || L.kind == SMALL32 || L.kind == SMALL64 || L.kind == SMALL128 || L.kind == SMALL192;
      const bool pairs = L.kind == BIG_DIAG || L.kind == BIG_TRSM || L.kind == BIG_UPDATE || L.kind == BIG_UPDATE128;
      if (list) {
        CHECK(L.off >= 0 && L.off + L.nf <= nsched && L.nf == L.items, at("front list outside sched, launch", li));
        for (int k = 0; k < L.nf; ++k) ++nfact[P.sched[L.off + k]];
      }
      if (pairs) {
        CHECK(L.off >= 0 && L.off % 2 == 0 && L.off + 2 * L.items <= nsched, at("pair list odd or outside sched, launch", li));
        if (L.kind == BIG_DIAG && L.step == 0)
          for (int64_t k = 0; k < L.items; ++k) ++nfact[P.sched[L.off + 2 * k]];
      }
      if (L.kind != BIG_DAG) continue;
      CHECK(L.off == dag0 && L.off + L.items <= ndag, at("DAG launches do not tile the task array, launch", li));
      dag0 += L.items;
      for (int64_t t = 0; t < L.items; ++t) {
        const int32_t* w = &P.dag_tasks[4 * (L.off + t)];
        CHECK(w[3] >= 0 && w[3] <= 3 && w[0] >= 0 && w[0] < ns && S.is_big[w[0]], at("DAG task kind / front, task", L.off + t));
        if (w[3] == 3) ++nfact[w[0]];
        for (int32_t q = P.dag_dptr[L.off + t]; q < P.dag_dptr[L.off + t + 1]; ++q) {
          const int32_t d = P.dag_dlist[q];
          CHECK(d >= 0 && d < t, at("DAG dependency not an earlier ticket, task", L.off + t));
          CHECK(q == P.dag_dptr[L.off + t] || P.dag_dlist[q - 1] < d, at("DAG dependencies unsorted or repeated, task", L.off + t));
        }
      }
    }
  CHECK(dag0 == ndag, "DAG tasks beyond the launches");
  // ---- factorisation tree: helper tickets first, dependencies earlier
  CHECK((int)P.ft_dptr.size() == P.nfhelp + P.nftree + 1 && (int)P.ft_order.size() == P.nftree, "ft_dptr entries");
  std::vector<int> tick(std::max(ns, 1), -1);
  for (int t = 0; t < P.nftree; ++t) tick[P.ft_order[t]] = P.nfhelp + t;
  for (int t = 0; t < P.nfhelp + P.nftree; ++t) {
    CHECK(t >= P.nfhelp || P.ft_dptr[t] == P.ft_dptr[t + 1], at("helper ticket with dependencies", t));
    for (int q = P.ft_dptr[t]; q < P.ft_dptr[t + 1]; ++q)
      CHECK(tick[P.ft_dep[q]] >= 0 && tick[P.ft_dep[q]] < t, at("factorisation tree dependency not earlier, ticket", t));
  }
  for (int f : P.ft_order) {
    ++nfact[f];
    for (int k = S.absorb[f] ? S.mc_ptr[f] : 0; k < (S.absorb[f] ? S.mc_ptr[f + 1] : 0); ++k) ++nfact[S.mc_list[k]];
  }
  // ---- solves: sched ranges, coverage
  for (const auto* V : {&P.slev1, &P.slev2})
    for (const SolveLevel& L : *V) {
      const int64_t off[4] = {L.micro_off, L.tiny_off, L.small_off, L.big_off};
      const int cnt[4] = {L.nmicro, L.ntiny, L.nsmall, L.nbig};
      for (int c = 0; c < 4; ++c) {
        CHECK(off[c] >= 0 && off[c] + cnt[c] <= nsched, "solve level list outside sched");
        for (int k = 0; k < cnt[c]; ++k) ++nsolve[P.sched[off[c] + k]];
      }
      CHECK(L.gat_off % 2 == 0 && L.gat_off + 2 * L.ngat <= nsched, "gather pairs odd or outside sched");
      CHECK(L.below_off % 2 == 0 && L.below_off + 2 * L.nbelow <= nsched, "below pairs odd or outside sched");
      CHECK(2 * (L.ftask_off + L.nftask) <= (int64_t)P.tasks.size() && 2 * (L.btask_off + L.nbtask) <= (int64_t)P.tasks.size(),
            "big-solve tasks outside the task array");
    }
  CHECK(P.xg_off % 2 == 0 && P.xg_off + 2 * P.nxg <= std::max<int64_t>(nsched, 0), "external gather pairs");
  std::vector<int> task(std::max(ns, 1), -1);
  CHECK((int)P.tc_list.size() == P.ntask && (int)P.tpar.size() == P.ntask && (int)P.tdep_ptr.size() == P.ntask + 1, "tree-solve sizes");
  for (int t = 0; t < P.ntask; ++t) task[P.tc_list[t]] = t, ++nsolve[P.tc_list[t]];
  for (int c = 0; c < ns; ++c) nsolve[c] += P.sleaf[c] ? 1 : 0;
  for (int t = 0; t < P.ntask; ++t) {
    for (int q = P.tdep_ptr[t]; q < P.tdep_ptr[t + 1]; ++q)
      CHECK(task[P.tdep[q]] >= 0 && task[P.tdep[q]] < t, at("tree-solve child not an earlier task, task", t));
    const int p = P.tpar[P.ntask - 1 - t];  // backward ticket ntask - 1 - t is task t
    CHECK(p < 0 || (task[p] > t), at("tree-solve parent without an earlier backward ticket, task", t));
  }
  for (int s = 0; s < ns; ++s) {
    const int want = !lb_member(S, s) && (in_phase(S, s, 1) || in_phase(S, s, 2));
    CHECK(nfact[s] == want, at("front factorised " + std::to_string(nfact[s]) + " times, front", s));
    CHECK(nsolve[s] == want, at("front solved " + std::to_string(nsolve[s]) + " times, front", s));
  }
  // ---- upos inside the parent's gather range and distinct; sv_nt within the row's gather count
  std::vector<uint8_t> seen((size_t)std::max<int64_t>(S.sv_ptr[S.row_ptr[ns]], 1), 0);
  for (int c = 0; c < ns; ++c) {
    const int p = S.parent[c];
    if (p < 0 || !P.in_tree[p]) continue;
    const int64_t g0 = S.sv_ptr[S.row_ptr[p]], g1 = S.sv_ptr[S.row_ptr[p] + S.nrows[p]];
    for (int64_t a = S.rel_ptr[c]; a < S.rel_ptr[c + 1]; ++a) {
      CHECK(P.upos[a] >= g0 && P.upos[a] < g1, at("upos outside the parent's gather range, child", c));
      CHECK(!seen[P.upos[a]], at("upos entry used twice, child", c));
      seen[P.upos[a]] = 1;
    }
  }
  for (int64_t t = 0; t < S.row_ptr[ns]; ++t)
    CHECK(P.sv_nt[t] <= S.sv_ptr[t + 1] - S.sv_ptr[t], at("sv_nt beyond the row's gather count, row", t));
  // ---- assembly: LDS-source tiles, chunk ids per group
  for (size_t t = 0; t < P.atiles.size(); ++t)
    if (P.atiles[t].gptr >= 0 && (P.atiles[t].gptr >> 47 & 1))
      CHECK((int64_t)((uint64_t)P.atiles[t].gchk >> 48) <= kAsmLdsSrc * kAsmLdsWinMax, at("LDS-source tile with too many sources, tile", t));
  for (size_t g = 0; g + 1 < P.asm_cid_off.size(); ++g)
    for (int64_t k = P.asm_cid_off[g]; k < P.asm_cid_off[g + 1]; ++k)
      CHECK(P.chunk_ids[k] >= S.chunk_lev[g] && P.chunk_ids[k] < S.chunk_lev[g + 1], at("chunk id outside its group, group", g));
}

// ---- multi-right-hand-side levels: every front of the plan exactly once over all levels and classes, its
// children at strictly lower levels, and a level's gather / below / task lists cover exactly its big fronts
void check_mlev(const SymbolicPlan& S, const LaunchPlan& P) {
  const int ns = S.nsuper;
  const int64_t nsched = (int64_t)P.sched.size(), ntask = (int64_t)P.tasks.size() / 2;
  if (S.nshards > 1) {
    CHECK(P.mlev.empty(), "mlev on a sharded plan");
    return;
  }
  CHECK((int)P.mlev.size() == S.nlevels, "mlev levels");
  std::vector<int> at_level(std::max(ns, 1), -1);
  for (int lev = 0; lev < (int)P.mlev.size(); ++lev) {
    const SolveLevel& L = P.mlev[lev];
    const int64_t off[4] = {L.micro_off, L.tiny_off, L.small_off, L.big_off};
    const int cnt[4] = {L.nmicro, L.ntiny, L.nsmall, L.nbig};
    std::vector<int32_t> big;
    for (int c = 0; c < 4; ++c) {
      CHECK(off[c] >= 0 && off[c] + cnt[c] <= nsched, at("mlev list outside sched, level", lev));
      for (int k = 0; k < cnt[c]; ++k) {
        const int s = P.sched[off[c] + k];
        CHECK(s >= 0 && s < ns, at("mlev front id, level", lev));
        CHECK(at_level[s] < 0, at("front twice in mlev, front", s));
        at_level[s] = lev;
        const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
        const int cls = (r <= 32 && w <= 2) ? 0 : !solve_small(S, s) ? 3 : r <= 32 ? 1 : solve_small_multi(S, s) ? 2 : 3;
        CHECK(cls == c, at("mlev class of front", s));
        if (c == 2) CHECK(8 * (r | 1) * w <= L.small_lds && L.small_lds + 8 * MULTI_W * SMALL_SOLVE_MAX <= kWorkgroupLds,
                          at("mlev small front beyond the level's LDS, front", s));
        if (c == 3) big.push_back(s);
      }
    }
    // gather pairs: (front, chunk) for every chunk of GAT_ROWS rows of every big front, and of no other
    CHECK(L.gat_off % 2 == 0 && L.gat_off + 2 * (int64_t)L.ngat <= nsched, at("mlev gather pairs, level", lev));
    CHECK(L.below_off % 2 == 0 && L.below_off + 2 * (int64_t)L.nbelow <= nsched, at("mlev below pairs, level", lev));
    CHECK(L.ftask_off + L.nftask <= ntask && L.btask_off + L.nbtask <= ntask, at("mlev tasks, level", lev));
    auto pairs = [](std::vector<std::pair<int, int>>& v) { std::sort(v.begin(), v.end()); };
    std::vector<std::pair<int, int>> wg, gg, wb, gb, wf, gf, wt, gt;
    for (int s : big) {
      const int r = S.nrows[s], w = S.first[s + 1] - S.first[s];
      for (int c = 0; c < cdiv(r, GAT_ROWS); ++c) wg.push_back({s, c});
      const int np = (int)cdiv(w, 64), nch = (int)cdiv(r - w, BWD_CHUNK);
      for (int p = 0; p < np; ++p)
        for (int c = 0; c < nch; ++c) wb.push_back({s, p | (c << 16)});
      for (int i = 0; i < cdiv(r, 64); ++i) wf.push_back({s, i});
      for (int p = 0; p < np; ++p) wt.push_back({s, p});
      CHECK(P.flag_off[s] >= 0 && P.flag_off[s] + np <= P.nflags, at("mlev big front's flags, front", s));
      CHECK(r == w || (P.bp_off[s] >= 0 && P.bp_off[s] + (int64_t)np * nch <= P.nbpart), at("mlev big front's bp_off, front", s));
    }
    for (int k = 0; k < L.ngat; ++k) gg.push_back({P.sched[L.gat_off + 2 * k], P.sched[L.gat_off + 2 * k + 1]});
    for (int k = 0; k < L.nbelow; ++k) gb.push_back({P.sched[L.below_off + 2 * k], P.sched[L.below_off + 2 * k + 1]});
    for (int k = 0; k < L.nftask; ++k) gf.push_back({P.tasks[2 * (L.ftask_off + k)], P.tasks[2 * (L.ftask_off + k) + 1]});
    for (int k = 0; k < L.nbtask; ++k) gt.push_back({P.tasks[2 * (L.btask_off + k)], P.tasks[2 * (L.btask_off + k) + 1]});
    // queue order: a front's forward blocks ascend and its backward panels descend (a task only waits for
    // tasks dequeued before it)
    for (size_t a = 0; a < gf.size(); ++a)
      for (size_t b = a + 1; b < gf.size(); ++b)
        if (gf[a].first == gf[b].first) {
          CHECK(gf[a].second < gf[b].second, at("mlev forward tasks of a front out of order, level", lev));
          break;
        }
    for (size_t a = 0; a < gt.size(); ++a)
      for (size_t b = a + 1; b < gt.size(); ++b)
        if (gt[a].first == gt[b].first) {
          CHECK(gt[a].second > gt[b].second, at("mlev backward tasks of a front out of order, level", lev));
          break;
        }
    pairs(wg), pairs(gg), pairs(wb), pairs(gb), pairs(wf), pairs(gf), pairs(wt), pairs(gt);
    CHECK(wg == gg, at("mlev gather list does not cover exactly the big fronts, level", lev));
    CHECK(wb == gb, at("mlev below list does not cover exactly the big fronts, level", lev));
    CHECK(wf == gf, at("mlev forward tasks do not cover exactly the big fronts, level", lev));
    CHECK(wt == gt, at("mlev backward tasks do not cover exactly the big fronts, level", lev));
  }
  for (int s = 0; s < ns; ++s) {
    const bool want = in_phase(S, s, 1);
    CHECK((at_level[s] >= 0) == want, at("front missing from (or wrongly in) mlev, front", s));
    if (!want) continue;
    for (int q = S.child_ptr[s]; q < S.child_ptr[s + 1]; ++q) {
      const int c = S.child_list[q];
      CHECK(!in_phase(S, c, 1) || at_level[c] < at_level[s], at("mlev child not at a lower level, front", s));
    }
  }
}

// the fronts of mlev, level by level and class by class ("info" lines: not digests)
void print_mlev(const SymbolicPlan& S, const LaunchPlan& P) {
  static const char* const cname[4] = {"micro", "tiny", "small", "big"};
  int64_t tot[4] = {0, 0, 0, 0};
  for (int lev = 0; lev < (int)P.mlev.size(); ++lev) {
    const SolveLevel& L = P.mlev[lev];
    const int64_t off[4] = {L.micro_off, L.tiny_off, L.small_off, L.big_off};
    const int cnt[4] = {L.nmicro, L.ntiny, L.nsmall, L.nbig};
    for (int c = 0; c < 4; ++c) {
      if (!cnt[c]) continue;
      tot[c] += cnt[c];
      printf("info mlev_fronts %d %s", lev, cname[c]);
      for (int k = 0; k < cnt[c]; ++k) printf(" %d", P.sched[off[c] + k]);
      printf("\n");
    }
  }
  printf("info mlev_classes levels %zu fronts %d micro %lld tiny %lld small %lld big %lld\n", P.mlev.size(), S.nsuper,
         (long long)tot[0], (long long)tot[1], (long long)tot[2], (long long)tot[3]);
}

void print_digests(const LaunchPlan& P) {
  dump("front", "u_ld", P.u_ld), dump("front", "fs_img", P.fs_img), dump("front", "g_src32", P.g_src32);
  dump("front", "brec", P.brec), dump("front", "atiles", P.atiles), dump("front", "g_ptr", P.g_ptr);
  dump("front", "chunk_ids", P.chunk_ids), dump("front", "asm_cid_off", P.asm_cid_off), dump("front", "bigslot", P.bigslot);
  dump("front", "xoff", P.xoff), dump("front", "topcol", P.topcol), dump("front", "wout", P.wout);
  dump("front", "colmask", P.colmask), dump("front", "gidx", P.gidx), dump("front", "lb_gid", P.lb_gid);
  dump("front", "lb_xrow", P.lb_xrow), dump("front", "lb_poff", P.lb_poff);
  dump("front", "scalars", Fnv() << (int)P.g32_fits << P.nbigslot << P.gper << P.xpack_tri << P.lb_npart);
  dump("tree", "ft_order", P.ft_order), dump("tree", "ft_dptr", P.ft_dptr), dump("tree", "ft_dep", P.ft_dep);
  dump("tree", "fold_help", P.fold_help), dump("tree", "fstart", P.fstart), dump("tree", "fhelp", P.fhelp);
  dump("tree", "fimg_dst", P.fimg_dst), dump("tree", "ab_loff", P.ab_loff);
  dump("tree", "in_tree", P.in_tree), dump("tree", "sleaf", P.sleaf), dump("tree", "sv_src", P.sv_src);
  dump("tree", "upos", P.upos), dump("tree", "sv_nt", P.sv_nt), dump("tree", "tchunk", P.tchunk);
  dump("tree", "trootbwd", P.trootbwd), dump("tree", "rootf", P.rootf), dump("tree", "tc_ptr", P.tc_ptr);
  dump("tree", "tc_list", P.tc_list), dump("tree", "tdep_ptr", P.tdep_ptr), dump("tree", "tdep", P.tdep);
  dump("tree", "tpar", P.tpar), dump("tree", "tfront", P.tfront), dump("tree", "tleaf", P.tleaf), dump("tree", "tlrow", P.tlrow);
  Fnv r;
  r << P.rargs.n;
  for (int q = 0; q < kRootArgs; ++q)
    r << P.rargs.s[q] << P.rargs.f0[q] << P.rargs.w[q] << P.rargs.r[q] << P.rargs.e0[q] << P.rargs.loff[q];
  dump("tree", "rargs", r);
  dump("tree", "scalars", Fnv() << P.fimg_size << P.nftree << P.nfhelp << P.ftree_lds << P.lds_cap << P.ftree_bytes
                                << P.ftree_flops << P.ftree_alg << P.ntree << P.ntask << P.nroot_task << P.root_lds << P.tree_lds
                                << P.nsleaf << P.tree_bytes << P.tree_flops << P.tree_alg << P.leaf_bytes << P.leaf_flops
                                << P.leaf_alg);
  dump("solve", "tasks", P.tasks), dump("solve", "flag_off", P.flag_off), dump("solve", "bp_off", P.bp_off);
  dump("solve", "scalars", Fnv() << P.nflags << P.nbpart);
  dump("launch", "fact1", hash_launches(P.fact1), P.fact1.size()), dump("launch", "fact2", hash_launches(P.fact2), P.fact2.size());
  dump("launch", "slev1", hash_levels(P.slev1), P.slev1.size()), dump("launch", "slev2", hash_levels(P.slev2), P.slev2.size());
  dump("launch", "mlev", hash_levels(P.mlev), P.mlev.size());
  dump("launch", "sched", P.sched), dump("launch", "dag_tasks", P.dag_tasks), dump("launch", "dag_dptr", P.dag_dptr);
  dump("launch", "dag_dlist", P.dag_dlist), dump("launch", "mslot", P.mslot), dump("launch", "tside", P.tside);
  dump("launch", "scalars", Fnv() << P.nmslot << P.upd_np << P.upd_nt << P.xg_off << P.nxg << (int)P.tail_ok << (int)P.asm_side
                                  << (int)P.side_tree << (uint64_t)P.side0 << P.nroot_side);
  int small_lds = 0;
  for (const auto* V : {&P.slev1, &P.slev2})
    for (const SolveLevel& L : *V) small_lds = std::max(small_lds, L.small_lds);
  printf("info max_small_solve_lds %d of %d\n", small_lds, kSolveSmallLds);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) fail("usage: plan_check <pattern file>");
  std::ifstream in(argv[1]);
  long long n = -1, nnz = -1;
  in >> n >> nnz;
  if (!in || n < 0 || nnz < 0 || n > INT32_MAX) fail("cannot read n, nnz");
  std::vector<int64_t> colptr(n + 1);
  std::vector<int32_t> rowval(nnz);
  for (auto& v : colptr) in >> v;
  for (auto& v : rowval) in >> v;
  SymbolicOptions opt;
  in >> opt.ordering >> opt.relax >> opt.small_front_max >> opt.nshards >> opt.shard;
  if (!in) fail("pattern file too short");
  try {
    SymbolicPlan S;
    symbolic_analyze((int)n, colptr.data(), rowval.data(), opt, nullptr, S);
    LaunchPlan P;
    build_launch_plan(S, read_ldl_knobs(), P);
    check_plan(S, P);
    check_mlev(S, P);
    print_digests(P);
    print_mlev(S, P);
  } catch (const std::exception& e) {
    fail(e.what());
  }
  return 0;
}
