// Builds the MPC's problem model on a CPU and checks it (csrc/qp_model.hpp; no GPU, no HIP call).
//
//   model_check <problem file> [--scaling S] [--kkt_system K] [--bound_relax_factor X] [--bound_push X]
//               [--bound_fac X] [--dump DIR] [--update FILE]
// The problem file is one text line "madipm_qp nvar ncon nnzj nnzh minimize" followed by raw little-endian
// arrays: c0 (1 double), c, lvar, uvar, x0 (nvar doubles each), lcon, ucon, y0 (ncon doubles each), Arows,
// Acols (nnzj int32 each), Avals (nnzj doubles), Hrows, Hcols (nnzh int32 each), Hvals (nnzh doubles).
// --update FILE: raw lvar, uvar (nvar doubles each), lcon, ucon (ncon doubles each) of an update, run through
// update()'s class-change checks after everything else.
// Builds the model, the refresh plan, the device route's lists, the adjoint's and the tangent's lists, checks their
// invariants (exit status 1 with a message on the first violation; 2 with "error: <text>" when the model
// itself refuses the problem or the update) and prints one line per array: "<name> <count> <FNV-1a 64>";
// --dump DIR also writes each array raw to DIR/<name>.bin.  MADIPM_ANALYSIS_THREADS applies as in the solver.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../madipm.jl_amd/csrc/qp_model.hpp"

using namespace madipm;

namespace {

std::string dump_dir;

[[noreturn]] void fail(const std::string& m) {
  fprintf(stderr, "model_check: %s\n", m.c_str());
  exit(1);
}
#define CHECK(c, m) \
  if (!(c)) fail(std::string(m) + " [" #c "]")
std::string at(const std::string& what, long long i) { return what + " " + std::to_string(i); }

template <class V>
void dump(const char* name, const V& v) {  // arrays of padding-free elements
  uint64_t h = 1469598103934665603ull;
  const unsigned char* p = (const unsigned char*)v.data();
  const size_t nb = v.size() * sizeof(v[0]);
  for (size_t i = 0; i < nb; ++i) h = (h ^ p[i]) * 1099511628211ull;
  printf("%s %zu %016llx\n", name, v.size(), (unsigned long long)h);
  if (dump_dir.empty()) return;
  FILE* f = fopen((dump_dir + "/" + name + ".bin").c_str(), "wb");
  CHECK(f, std::string("cannot write ") + name);
  if (nb) CHECK(fwrite(p, 1, nb, f) == nb, std::string("short write of ") + name);
  fclose(f);
}
void dump(const char* name, double v) { dump(name, std::vector<double>{v}); }

template <class T>
std::vector<T> read_raw(FILE* f, int64_t n, const char* what) {
  std::vector<T> v(n);
  if (n) CHECK(fread(v.data(), sizeof(T), n, f) == (size_t)n, std::string("short read of ") + what);
  return v;
}

// ascending row pointers, strictly ascending in-range columns inside each row
template <class CI>
void check_csr(const std::string& name, int64_t nrow, int64_t ncol, const std::vector<int64_t>& rp, const CI& ci) {
  CHECK((int64_t)rp.size() == nrow + 1 && rp[0] == 0 && rp[nrow] == (int64_t)ci.size(), name + " row pointers");
  for (int64_t i = 0; i < nrow; ++i) {
    CHECK(rp[i] <= rp[i + 1], at(name + " row", i));
    for (int64_t q = rp[i]; q < rp[i + 1]; ++q) {
      CHECK(ci[q] >= 0 && ci[q] < ncol, at(name + " index out of range at", q));
      CHECK(q == rp[i] || ci[q - 1] < ci[q], at(name + " columns not strictly ascending at", q));
    }
  }
}
template <class CI>
std::vector<int32_t> rows_of(const std::vector<int64_t>& rp, const CI& ci) {
  std::vector<int32_t> r(ci.size());
  for (size_t i = 0; i + 1 < rp.size(); ++i)
    for (int64_t q = rp[i]; q < rp[i + 1]; ++q) r[q] = (int32_t)i;
  return r;
}
// per-destination lists of (input index, other): sp ascending, input indices strictly ascending inside a
// destination, every pair accepted by ok(destination, pair); cover[input index] counts the appearances
void check_lists(const std::string& name, int64_t nd, const std::vector<int32_t>& sp, const std::vector<I2>& e,
                 const std::function<bool(int, I2)>& ok, std::vector<int>& cover) {
  CHECK((int64_t)sp.size() == nd + 1 && sp[0] == 0 && sp[nd] == (int32_t)e.size(), name + " list starts");
  for (int64_t d = 0; d < nd; ++d) {
    CHECK(sp[d] <= sp[d + 1], at(name + " starts at", d));
    for (int32_t q = sp[d]; q < sp[d + 1]; ++q) {
      CHECK(e[q].x >= 0 && e[q].x < (int32_t)cover.size(), at(name + " input index at", q));
      CHECK(q == sp[d] || e[q - 1].x < e[q].x, at(name + " not ascending in input index at", q));
      CHECK(ok((int)d, e[q]), at(name + " entry does not belong to its destination at", q));
      cover[e[q].x]++;
    }
  }
}
void check_cover(const std::string& name, const std::vector<int>& cover, const std::function<int(int64_t)>& want) {
  for (size_t k = 0; k < cover.size(); ++k) CHECK(cover[k] == want((int64_t)k), at(name + " covers input entry", k));
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

}  // namespace

int main(int argc, char** argv) try {
  if (argc < 2) fail("usage: model_check <problem file> [--scaling S] [--kkt_system K] [--bound_relax_factor X] "
                     "[--bound_push X] [--bound_fac X] [--dump DIR] [--update FILE]");
  madipm_options opt{};
  opt.scaling = 1;
  opt.bound_push = 1e-2;
  opt.bound_fac = 1e-2;
  opt.bound_relax_factor = 1e-12;
  std::string update_file;
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    CHECK(i + 1 < argc, "missing value of " + a);
    const char* v = argv[++i];
    if (a == "--scaling") opt.scaling = atoi(v);
    else if (a == "--kkt_system") opt.kkt_system = atoi(v);
    else if (a == "--bound_relax_factor") opt.bound_relax_factor = atof(v);
    else if (a == "--bound_push") opt.bound_push = atof(v);
    else if (a == "--bound_fac") opt.bound_fac = atof(v);
    else if (a == "--dump") dump_dir = v;
    else if (a == "--update") update_file = v;
    else fail("unknown option " + a);
  }
  // ---- the problem
  FILE* f = fopen(argv[1], "rb");
  CHECK(f, "cannot open the problem file");
  char head[256];
  CHECK(fgets(head, sizeof head, f), "no header line");
  long long nvar, ncon, nnzj, nnzh;
  int minimize;
  CHECK(sscanf(head, "madipm_qp %lld %lld %lld %lld %d", &nvar, &ncon, &nnzj, &nnzh, &minimize) == 5, "bad header line");
  const auto c0 = read_raw<double>(f, 1, "c0");
  const auto c = read_raw<double>(f, nvar, "c"), lvar = read_raw<double>(f, nvar, "lvar"),
             uvar = read_raw<double>(f, nvar, "uvar"), x0 = read_raw<double>(f, nvar, "x0"),
             lcon = read_raw<double>(f, ncon, "lcon"), ucon = read_raw<double>(f, ncon, "ucon"),
             y0 = read_raw<double>(f, ncon, "y0");
  const auto Ar = read_raw<int32_t>(f, nnzj, "Arows"), Ac = read_raw<int32_t>(f, nnzj, "Acols");
  const auto Av = read_raw<double>(f, nnzj, "Avals");
  const auto Hr = read_raw<int32_t>(f, nnzh, "Hrows"), Hc = read_raw<int32_t>(f, nnzh, "Hcols");
  const auto Hv = read_raw<double>(f, nnzh, "Hvals");
  fclose(f);
  madipm_qp q{};
  q.nvar = (int32_t)nvar;
  q.ncon = (int32_t)ncon;
  q.nnzh = nnzh;
  q.nnzj = nnzj;
  q.c = c.data();
  q.c0 = c0[0];
  q.Hrows = Hr.data();
  q.Hcols = Hc.data();
  q.Hvals = Hv.data();
  q.Arows = Ar.data();
  q.Acols = Ac.data();
  q.Avals = Av.data();
  q.lcon = lcon.data();
  q.ucon = ucon.data();
  q.lvar = lvar.data();
  q.uvar = uvar.data();
  q.x0 = x0.data();
  q.y0 = y0.data();
  q.minimize = minimize;

  // ---- build: as setup_host, prepare_update, build_device_route and adjoint do
  QPHost P;
  qp_intake(P, q);
  HostNumeric num;
  JCoo jcoo;
  numeric_host(P, opt, num, &jcoo);
  const QPStructure S = build_structure(P, opt, jcoo);
  RefreshPlan R = build_refresh_plan(P, q);
  P.Ar = R.Ar.data();
  P.Ac = R.Ac.data();
  P.Av = R.Av.data();
  const RouteLists L = build_route_lists(P);
  const std::vector<int32_t> rowslack = adjoint_rowslack(P);
  const AdjointLists G = build_adjoint_lists(P);
  const TangentLists TL = build_tangent_lists(P);
  const int nx = P.nx, m = P.m, n = P.n;
  const int64_t nJ = R.nJ, nH = R.nH;

  // ---- invariants
  check_csr("H", n, n, S.Hrp, S.Hci);
  check_csr("J", m, n, S.Jrp, S.Jci);
  check_csr("J^T", n, m, S.JTrp, S.JTci);
  check_csr("K2", n + m, n + m, S.Kcp, S.Kri);
  CHECK((int64_t)S.Jci.size() == nJ && (int64_t)S.JTci.size() == nJ && (int64_t)S.Hci.size() == nH, "entry counts");
  CHECK(S.Hcv.size() == S.Hci.size() && S.Jcv.size() == S.Jci.size() && S.JTcv.size() == S.JTci.size() &&
            S.Kv.size() == S.Kri.size(),
        "value array lengths");
  const std::vector<int32_t> Jrow = rows_of(S.Jrp, S.Jci), JTrow = rows_of(S.JTrp, S.JTci), Hrow = rows_of(S.Hrp, S.Hci);
  {  // J and J^T hold the same entries; j2jt is the permutation between them
    CHECK((int64_t)R.j2jt.size() == nJ, "j2jt length");
    std::vector<char> seen(nJ, 0);
    for (int64_t t = 0; t < nJ; ++t) {
      const int32_t u = R.j2jt[t];
      CHECK(u >= 0 && u < nJ && !seen[u], at("j2jt is not a permutation at", t));
      seen[u] = 1;
      CHECK(JTrow[u] == S.Jci[t] && S.JTci[u] == Jrow[t], at("j2jt names another entry at", t));
      CHECK(same_bits(S.Jcv[t], S.JTcv[u]), at("J and J^T values differ at", t));
    }
  }
  {  // K2's columns and the slots the refresh writes
    CHECK((int64_t)S.diag_pos.size() == n + m, "diag_pos length");
    CHECK((int64_t)R.hk.size() == nH && (int64_t)R.jtk.size() == nJ && (int64_t)R.hdpos.size() == n, "plan lengths");
    std::vector<int> hit(S.Kri.size(), 0);
    for (int j = 0; j < n + m; ++j) {
      int64_t o = S.Kcp[j];
      CHECK(S.diag_pos[j] == o && S.Kri[o] == j && same_bits(S.Kv[o], 0.0), at("K2 column does not start with its diagonal:", j));
      hit[o++] = 1;  // the diagonal belongs to k_diag
      if (j >= n) {
        CHECK(S.Kcp[j + 1] == o, at("K2 constraint column is not its diagonal alone:", j));
        continue;
      }
      for (int64_t qh = S.Hrp[j]; qh < S.Hrp[j + 1]; ++qh) {
        if (S.Hci[qh] <= j) {
          CHECK(R.hk[qh] == -1, at("hk of an upper-triangle entry", qh));
          continue;
        }
        CHECK(o < S.Kcp[j + 1] && S.Kri[o] == S.Hci[qh] && same_bits(S.Kv[o], S.Hcv[qh]), at("K2 H part of column", j));
        CHECK(R.hk[qh] == o, at("hk of H entry", qh));
        hit[o++]++;
      }
      for (int64_t qt = S.JTrp[j]; qt < S.JTrp[j + 1]; ++qt) {
        CHECK(o < S.Kcp[j + 1] && S.Kri[o] == n + S.JTci[qt] && same_bits(S.Kv[o], S.JTcv[qt]), at("K2 J part of column", j));
        CHECK(R.jtk[qt] == o, at("jtk of J^T entry", qt));
        hit[o++]++;
      }
      CHECK(o == S.Kcp[j + 1], at("K2 column length", j));
    }
    for (size_t o = 0; o < hit.size(); ++o) CHECK(hit[o] == 1, at("K2 slot not written exactly once:", o));
    for (int i = 0; i < n; ++i) {
      const int32_t t = R.hdpos[i];
      bool has = false;
      for (int64_t qh = S.Hrp[i]; qh < S.Hrp[i + 1]; ++qh) has |= S.Hci[qh] == i;
      CHECK(t == -1 ? !has : (t >= 0 && t < nH && Hrow[t] == i && S.Hci[t] == i), at("hdpos", i));
    }
  }
  const int64_t na = P.nnzA, nh = (int64_t)P.Hv.size();
  auto hfree = [&](int64_t k) { return !P.fixed[P.Hr[k]] && !P.fixed[P.Hc[k]]; };
  auto hcross = [&](int64_t k) { return P.fixed[P.Hr[k]] != P.fixed[P.Hc[k]]; };
  auto hdiag = [&](int64_t k) { return P.Hr[k] == P.Hc[k]; };
  auto pairs = [](const std::vector<int32_t>& src) {  // a plain source list as (source, 0) pairs
    std::vector<I2> e(src.size());
    for (size_t i = 0; i < src.size(); ++i) e[i] = {src[i], 0};
    return e;
  };
  {
    std::vector<int> cov(na, 0);
    check_lists("tsp/tsrc", nJ, R.tsp, pairs(R.tsrc),
                [&](int t, I2 e) { return P.Ac[e.x] == JTrow[t] && P.Ar[e.x] == S.JTci[t]; }, cov);
    check_cover("tsp/tsrc", cov, [&](int64_t k) { return P.fixed[P.Ac[k]] ? 0 : 1; });
    for (int64_t t = 0; t < nJ; ++t)
      CHECK((JTrow[t] >= nx) == (R.tsp[t] == R.tsp[t + 1]), at("a slack entry has a source, or an entry of A none:", t));
  }
  {
    std::vector<int> cov(nh, 0);
    check_lists("hsp/hsrc", nH, R.hsp, pairs(R.hsrc), [&](int t, I2 e) {
      return (P.Hr[e.x] == Hrow[t] && P.Hc[e.x] == S.Hci[t]) || (P.Hc[e.x] == Hrow[t] && P.Hr[e.x] == S.Hci[t]);
    }, cov);
    check_cover("hsp/hsrc", cov, [&](int64_t k) { return !hfree(k) ? 0 : hdiag(k) ? 1 : 2; });
  }
  {
    std::vector<int> cov(na, 0);
    check_lists("asp/ae", m, L.asp, L.ae, [&](int d, I2 e) { return P.Ar[e.x] == d && P.Ac[e.x] == e.y; }, cov);
    check_cover("asp/ae", cov, [](int64_t) { return 1; });
    cov.assign(na, 0);
    check_lists("fsp/fe", m, L.fsp, L.fe,
                [&](int d, I2 e) { return P.Ar[e.x] == d && P.Ac[e.x] == e.y && P.fixed[e.y]; }, cov);
    check_cover("fsp/fe", cov, [&](int64_t k) { return P.fixed[P.Ac[k]] ? 1 : 0; });
    cov.assign(na, 0);
    const int nf = (int)G.fix.size();
    check_lists("fasp/fa", nf, G.fasp, G.fa, [&](int d, I2 e) { return P.Ac[e.x] == G.fix[d] && P.Ar[e.x] == e.y; }, cov);
    check_cover("fasp/fa", cov, [&](int64_t k) { return P.fixed[P.Ac[k]] ? 1 : 0; });
    int want = 0;
    for (int i = 0; i < nx; ++i)
      if (P.fixed[i]) CHECK(want < nf && G.fix[want++] == i, at("fix misses variable", i));
    CHECK(want == nf, "fix length");
  }
  {
    auto ends = [&](int d, I2 e) {
      return (P.Hr[e.x] == d && P.Hc[e.x] == e.y) || (P.Hc[e.x] == d && P.Hr[e.x] == e.y);
    };
    std::vector<int> cov(nh, 0);
    check_lists("gsp/ge", nx, L.gsp, L.ge, ends, cov);
    check_cover("gsp/ge", cov, [&](int64_t k) { return hdiag(k) ? 1 : 2; });
    cov.assign(nh, 0);
    check_lists("xsp/xe", nx, L.xsp, L.xe, [&](int d, I2 e) { return ends(d, e) && !P.fixed[d] && P.fixed[e.y]; }, cov);
    check_cover("xsp/xe", cov, [&](int64_t k) { return hcross(k) ? 1 : 0; });
    cov.assign(nh, 0);
    check_lists("fhsp/fh", (int64_t)G.fix.size(), G.fhsp, G.fh,
                [&](int d, I2 e) { return ends(G.fix[d], e) && !P.fixed[e.y]; }, cov);
    check_cover("fhsp/fh", cov, [&](int64_t k) { return hcross(k) ? 1 : 0; });
    size_t b = 0;
    CHECK(L.bfk.size() == L.bfrc.size(), "bfk / bfrc lengths");
    for (int64_t k = 0; k < nh; ++k)
      if (P.fixed[P.Hr[k]] && P.fixed[P.Hc[k]]) {
        CHECK(b < L.bfk.size() && L.bfk[b] == k && L.bfrc[b].x == P.Hr[k] && L.bfrc[b].y == P.Hc[k], at("bfk misses H entry", k));
        ++b;
      }
    CHECK(b == L.bfk.size(), "bfk length");
  }
  {  // the tangent's lists: every entry of A once per row and once per column, every entry of H per endpoint
    std::vector<int> cov(na, 0);
    check_lists("tangent asp/ae", m, TL.asp, TL.ae, [&](int d, I2 e) { return P.Ar[e.x] == d && P.Ac[e.x] == e.y; }, cov);
    check_cover("tangent asp/ae", cov, [](int64_t) { return 1; });
    cov.assign(na, 0);
    check_lists("tangent csp/ce", nx, TL.csp, TL.ce, [&](int d, I2 e) { return P.Ac[e.x] == d && P.Ar[e.x] == e.y; }, cov);
    check_cover("tangent csp/ce", cov, [](int64_t) { return 1; });
    cov.assign(nh, 0);
    check_lists("tangent gsp/ge", nx, TL.gsp, TL.ge, [&](int d, I2 e) {
      return (P.Hr[e.x] == d && P.Hc[e.x] == e.y) || (P.Hc[e.x] == d && P.Hr[e.x] == e.y);
    }, cov);
    check_cover("tangent gsp/ge", cov, [&](int64_t k) { return hdiag(k) ? 1 : 2; });
  }
  CHECK((int)L.vcls.size() == nx && (int)L.ccls.size() == m, "class lengths");
  for (int i = 0; i < nx; ++i) CHECK(L.vcls[i] == bound_class(P.lvar[i], P.uvar[i]), at("vcls", i));
  for (int i = 0; i < m; ++i) CHECK(L.ccls[i] == bound_class(P.lcon[i], P.ucon[i]), at("ccls", i));
  for (int i = 0; i < m; ++i) {
    const int32_t s = rowslack[i];
    CHECK(s == -1 ? P.lcon[i] == P.ucon[i] : (s >= nx && s < n && P.ind_ineq[s - nx] == i), at("rowslack", i));
  }
  if (opt.kkt_system == KKT_NORMAL) {
    check_csr("C", m, m, S.Ccp, S.Cri);
    const int64_t nC = (int64_t)S.Cri.size();
    CHECK((int64_t)S.cpp.size() == nC + 1 && S.cpp[0] == 0 && 2 * S.cpp[nC] == (int64_t)S.cprod.size(), "cpp / cprod lengths");
    for (int i = 0; i < m; ++i)
      for (int64_t e = S.Ccp[i]; e < S.Ccp[i + 1]; ++e) {
        CHECK(S.Cri[e] >= i && S.cpp[e] <= S.cpp[e + 1], at("C entry", e));
        for (int64_t p = S.cpp[e]; p < S.cpp[e + 1]; ++p) {
          const int32_t a = S.cprod[2 * p], b = S.cprod[2 * p + 1];
          CHECK(a >= 0 && a < nJ && b >= 0 && b < nJ && Jrow[a] == i && Jrow[b] == S.Cri[e] && S.Jci[a] == S.Jci[b],
                at("product of C entry", e));
        }
      }
  }

  // ---- digests
  dump("ind_ineq", P.ind_ineq);
  dump("ind_fixed", P.ind_fixed);
  dump("ind_lb", P.ind_lb);
  dump("ind_ub", P.ind_ub);
  dump("fixed", P.fixed);
  dump("lbpos", S.lbpos);
  dump("ubpos", S.ubpos);
  dump("x", P.x);
  dump("xl", P.xl);
  dump("xu", P.xu);
  dump("y", P.y);
  dump("rhs", P.rhs);
  dump("con_scale", P.con_scale);
  dump("obj_scale", num.obj_scale);
  dump("c0s", num.c0s);
  dump("norm_b", num.norm_b);
  dump("gfix", num.gfix);
  dump("cfix", num.cfix);
  dump("cs", num.cs);
  dump("Hdiag", S.Hdiag);
  dump("Hrp", S.Hrp);
  dump("Hci", S.Hci);
  dump("Hv", S.Hcv);
  dump("Jrp", S.Jrp);
  dump("Jci", S.Jci);
  dump("Jv", S.Jcv);
  dump("JTrp", S.JTrp);
  dump("JTci", S.JTci);
  dump("JTv", S.JTcv);
  dump("Kcp", S.Kcp);
  dump("Kri", S.Kri);
  dump("Kv", S.Kv);
  dump("diag_pos", S.diag_pos);
  if (opt.kkt_system == KKT_K25) dump("kcol", k2_slot_columns(S.Kcp));
  dump("Ccp", S.Ccp);
  dump("Cri", S.Cri);
  dump("cpp", S.cpp);
  dump("cprod", S.cprod);
  dump("tsp", R.tsp);
  dump("tsrc", R.tsrc);
  dump("jtk", R.jtk);
  dump("j2jt", R.j2jt);
  dump("hsp", R.hsp);
  dump("hsrc", R.hsrc);
  dump("hk", R.hk);
  dump("hdpos", R.hdpos);
  dump("asp", L.asp);
  dump("ae", L.ae);
  dump("fsp", L.fsp);
  dump("fe", L.fe);
  dump("gsp", L.gsp);
  dump("ge", L.ge);
  dump("xsp", L.xsp);
  dump("xe", L.xe);
  dump("bfk", L.bfk);
  dump("bfrc", L.bfrc);
  dump("vcls", L.vcls);
  dump("ccls", L.ccls);
  dump("rowslack", rowslack);
  dump("fix", G.fix);
  dump("fhsp", G.fhsp);
  dump("fh", G.fh);
  dump("fasp", G.fasp);
  dump("fa", G.fa);

  if (!update_file.empty()) {
    FILE* u = fopen(update_file.c_str(), "rb");
    CHECK(u, "cannot open the update file");
    const auto lv = read_raw<double>(u, nvar, "update lvar"), uv = read_raw<double>(u, nvar, "update uvar"),
               lc = read_raw<double>(u, ncon, "update lcon"), uc = read_raw<double>(u, ncon, "update ucon");
    fclose(u);
    require_same_classes(P, lv.data(), uv.data(), lc.data(), uc.data());
  }
  return 0;
} catch (const std::runtime_error& e) {  // madipm::Error: the model's own refusals
  fprintf(stderr, "error: %s\n", e.what());
  return 2;
}
