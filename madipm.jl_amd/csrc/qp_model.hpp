// The problem model of MPCSolver (host only: no HIP call, no device buffer, no stream).
//
// Everything the solver derives on the host from the caller's QP before a byte is uploaded: the copy of
// the problem and its index sets, the value-dependent vectors (numeric_host), the H / J / J^T CSR arrays,
// the K2 and normal-equations patterns, the refresh plan of prepare_update, the sum-order lists of the
// device route, the fixed-variable lists of the adjoint and the entry lists of the tangent.  mpc.hip and
// mpc_post.hip build these, upload them and synchronise; tools/model_check.cpp builds and checks them on a
// machine without a GPU.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/madipm_hip.h"
#include "hvec.hpp"

namespace madipm {

struct PhaseClock;  // common.hpp (MADIPM_SYMBOLIC_TIMING); the builders take one or null

struct I2 {  // the device code's int2 (mpc_kernels.hpp asserts the layout)
  int32_t x, y;
};

enum { KKT_K2 = 0, KKT_K25 = 1, KKT_NORMAL = 2 };  // madipm_options.kkt_system

struct QPHost {
  int nx = 0, m = 0, n = 0, ns = 0;
  std::vector<double> c, lvar, uvar, lcon, ucon, x0, y0, Hv;
  std::vector<int32_t> Hr, Hc;
  // A's COO: the caller's arrays, read during construction only (no host copy: 8 GB for the dense QP)
  const int32_t* Ar = nullptr;
  const int32_t* Ac = nullptr;
  const double* Av = nullptr;
  int64_t nnzA = 0;
  double c0 = 0, sgn = 1;
  bool minimize = true;
  std::vector<int32_t> ind_ineq, ind_fixed, ind_lb, ind_ub;
  std::vector<uint8_t> fixed;
  bool has_ineq = false;
  std::vector<double> con_scale;
  double obj_scale = 1;
  std::vector<double> x, xl, xu, rhs, y;
  bool anyfix = false;  // a fixed structural variable: J is built from a filtered COO, cfix is non-zero
  int64_t nJ = 0, nH = 0, nnzK = 0;  // entries of J (= J^T), H and K2 as build_structure laid them out
};

// What numeric_host hands to the device besides QPHost's own vectors, and the solver's three scalars
struct HostNumeric {
  std::vector<double> gfix, cfix, cs;
  double obj_scale = 1, c0s = 0, norm_b = 0;
};

// The filtered COO of J that numeric_host's cfix pass collects at creation (a fixed variable only)
struct JCoo {
  std::vector<int32_t> r, c;
  std::vector<double> v;
};

// Copy and validation of the problem, its index sets (MadNLP.get_index_constraints: EnforceEquality,
// MakeParameter) and the raw bounds of [x; s]
void qp_intake(QPHost& P, const madipm_qp& q, PhaseClock* clk = nullptr);

// The numeric part of the construction: everything of size O(n + m) that depends on the problem's numbers
// (and the O(nnz) host sums behind it), from QPHost's data, its index sets and A's COO.  The constructor
// and update() both run it, so a refreshed solver holds the bits a fresh one would; update_device's
// kernels reproduce every sum here in this order.
void numeric_host(QPHost& P, const madipm_options& opt, HostNumeric& o, JCoo* jcoo = nullptr);

// The arrays the constructor uploads; setup_host hands the struct to free_async afterwards
struct QPStructure {
  std::vector<double> Hdiag;
  std::vector<int64_t> Hrp, Jrp, JTrp, Kcp, diag_pos;
  hvec<int32_t> Hci, Jci, JTci, Kri;
  hvec<double> Hcv, Jcv, JTcv, Kv;
  std::vector<int32_t> lbpos, ubpos;
  // normal equations: lower CSC of C = J J^T and, per entry, its products as pairs of positions in Jcv
  std::vector<int64_t> Ccp, cpp;
  std::vector<int32_t> Cri, cprod;
};
// jcoo: numeric_host's (consumed) when P.anyfix, unused otherwise (J is read from the caller's A)
QPStructure build_structure(QPHost& P, const madipm_options& opt, JCoo& jcoo, PhaseClock* clk = nullptr);

// K2's lower-CSC column pointers: column j < n = [j; H's rows i > j (row j of the symmetric CSR);
// n + row j of J^T], column j >= n = [j].  The one definition of the layout: build_structure fills the
// pattern by it and build_refresh_plan addresses the slots by it.
std::vector<int64_t> k2_colptr(int n, int m, const int64_t* Hrp, const int32_t* Hci, const int64_t* JTrp);
// the column of every slot of the CSC (K2.5's scaling kernels)
hvec<int32_t> k2_slot_columns(const std::vector<int64_t>& Kcp);

// csr_from_coo's structure for the COO (r, c) without its values: destination entries sorted by
// (row, column), each with the ids of its COO entries in input order (id < 0: a constant entry, no source)
struct CooPlan {
  std::vector<int32_t> sp, src, drow, dcol;
  std::vector<int64_t> rp;  // row pointers of the destination entries
};
CooPlan coo_plan(int nrow, const std::vector<int32_t>& r, const std::vector<int32_t>& c,
                 const std::vector<int32_t>& id);

// The refresh plan (prepare_update).  Every destination entry of a value array owns a list of COO
// sources, [sp[q], sp[q + 1]) into src, in ascending input index: csr_from_coo's merge order.  J's lists
// are kept once, in J^T's entry order (whose column-index array already names each entry's constraint
// row, i.e. its con_scale); J's own values are gathered from J^T's through j2jt.  32-bit throughout.
struct RefreshPlan {
  std::vector<int32_t> Ar, Ac;  // host copy of A's COO for the host passes (slack start, row maxima, cfix)
  std::vector<double> Av;
  std::vector<int32_t> tsp, tsrc, jtk, j2jt;  // J^T entry -> sources, -> its K2 slot; J entry -> J^T entry
  std::vector<int32_t> hsp, hsrc, hk, hdpos;  // H entry -> sources, -> its K2 slot (-1: upper triangle);
                                              // hdpos[i] = H's entry (i, i) or -1
  int64_t nJ = 0, nH = 0;                     // destination entries of J (= J^T) and H
};
// q: the problem the solver was created with (its A arrays are copied); refuses anything else
RefreshPlan build_refresh_plan(const QPHost& P, const madipm_qp& q);

// The device route's lists, which give every host sum of numeric_host its input order: per destination
// [sp[i], sp[i + 1]) of (input index, other index) pairs.  asp / ae: A's entries per row; fsp / fe: those
// in a fixed column; gsp / ge: H's entries per endpoint; xsp / xe: fixed / free entries of H per free
// endpoint; bfk / bfrc: entries of H between two fixed variables; vcls / ccls: creation-time bound classes.
// Reads A through P.Ar / P.Ac (the plan's copy after prepare_update).
struct RouteLists {
  std::vector<int32_t> asp, fsp, gsp, xsp, bfk;
  std::vector<I2> ae, fe, ge, xe, bfrc;
  std::vector<uint8_t> vcls, ccls;
};
RouteLists build_route_lists(const QPHost& P);

// The adjoint's lists: row -> its slack (index into [nx, n)) or -1; the fixed variables with, per fixed
// variable, (entry of Hvals, free endpoint) and (entry of Avals, row)
std::vector<int32_t> adjoint_rowslack(const QPHost& P);
struct AdjointLists {
  std::vector<int32_t> fix, fhsp, fasp;
  std::vector<I2> fh, fa;
};
AdjointLists build_adjoint_lists(const QPHost& P);

// The tangent's lists (forward-mode sensitivities): the entries of the COO input per destination as
// (input index, other index) pairs in ascending input index, so every data product has a fixed order.
// asp / ae: A's entries per row (entry, column); csp / ce: A's entries per column (entry, row); gsp / ge:
// H's entries per endpoint (entry, other endpoint; a diagonal entry once).  Fixed columns and endpoints are
// kept: their terms are the fixed variables' part of the right-hand side.  Reads A through P.Ar / P.Ac.
struct TangentLists {
  std::vector<int32_t> asp, csp, gsp;
  std::vector<I2> ae, ce, ge;
};
TangentLists build_tangent_lists(const QPHost& P);

// what qp_intake derives from one coordinate's bounds: fixed (1), or finite lower (2) | finite upper (4)
int bound_class(double l, double u);
// The classification derived at creation must hold for an update's bounds; a change throws Error -3 that
// names the coordinate and the change.  a, b: bound_class before and after.
[[noreturn]] void throw_kind_change(int idx, bool was_equality);
void require_same_class(const char* what, int idx, int a, int b);
void require_same_class(const char* what, int idx, double l0, double u0, double l1, double u1);
// update()'s checks in its order: every row's kind, every variable, every ranged row
void require_same_classes(const QPHost& P, const double* lvar, const double* uvar, const double* lcon,
                          const double* ucon);

}  // namespace madipm
