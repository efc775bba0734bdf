// The argument and CSR checks of fu_create, fu_dist_create(_local) and the scaffold engines
// (csrc/fu_graph.cpp: check_fu_create, check_create, pairing_rev, check_csr), fed every malformed
// array of tests/test_create_abi.py. Built with AddressSanitizer and UndefinedBehaviorSanitizer;
// every array is a heap block of exactly its length, so a check that walks an array before the
// checks ahead of it have proved the index good is reported as a heap-buffer-overflow.
// Prints one line per failed expectation and "<N> cases, <F> failed"; exit 0 only if F == 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fu_common.h"

namespace {

constexpr int ARG = FU_ERR_ARG, GRAPH = FU_ERR_GRAPH;

// A heap block of exactly v.size() elements (nullptr for "pass NULL").
template <typename T>
struct Exact {
  std::unique_ptr<T[]> p;
  bool null = false;
  Exact(std::initializer_list<T> v) : p(new T[v.size()]) { std::copy(v.begin(), v.end(), p.get()); }
  Exact(std::nullptr_t) : null(true) {}
  const T *get() const { return null ? nullptr : p.get(); }
};
using I64 = Exact<int64_t>;
using I32 = Exact<int32_t>;

int g_cases = 0, g_failed = 0;

void expect(const char *what, int rc, int code, const std::string &text) {
  ++g_cases;
  const std::string got = rc ? fu_last_error() : "";
  if (rc == code && got == text) return;
  ++g_failed;
  std::printf("FAILED %s: got (%d, \"%s\"), expected (%d, \"%s\")\n", what, rc, got.c_str(), code, text.c_str());
}

const double kValue[4] = {1.0, 2.0, 3.0, 4.0};
int g_out_slot;
void *const kOut = &g_out_slot;

// fu_create(n, e, rowptr, col, rev, value, ., out) up to its device probe
void create(const char *what, int32_t n, int64_t e, const I64 &rp, const I32 &col, const I32 &rev, int code,
            const std::string &tail, const double *value = kValue, const void *out = kOut) {
  const int rc = fu::check_fu_create(n, e, rp.get(), col.get(), rev.get(), value, out);
  expect(what, rc, code, code == 0 ? "" : tail.rfind("graph is", 0) == 0 ? tail : "fu_create: " + tail);
}

// fu_dist_create(_local)'s local CSR, after its halo plan checks
void dist(const char *what, int32_t n, int64_t e, const I64 &rp, const I32 &col, int32_t ghosts, int code,
          const std::string &text) {
  expect(what, fu::check_create("fu_dist_create", n, e, rp.get(), col.get(), kValue, ghosts, kOut), code, text);
}

// fu_lossy_create, fu_churn_create, fu_pair_create, fu_churn_live
void pairing(const char *what, int32_t n, int64_t e, const I64 &rp, const I32 &col, const I32 &rev, int code,
             const std::string &tail) {
  const int32_t *r = rev.get();
  std::vector<int32_t> built;
  const int rc = fu::pairing_rev("fu_lossy_create", n, e, rp.get(), col.get(), &r, &built);
  expect(what, rc, code, code == 0 ? "" : tail.rfind("graph is", 0) == 0 ? tail : "fu_lossy_create: " + tail);
}

const std::string kBad = "bad arguments";
const std::string kEnds = "rowptr[0] must be 0 and rowptr[n] == e";
const std::string kMono = "rowptr not monotone";
const std::string kCol = "col index out of range at edge ";
const std::string kRev = "rev is not the reverse-edge pairing (the graph must be symmetric) at edge ";
const std::string kAsym = "graph is not symmetric (edge 0 has no reverse edge)";
const std::string kMany = "more than 2^31-1 edges";

#define PATH_RP {0, 1, 3, 4}
#define PATH_COL {1, 0, 2, 1}
#define PATH_REV {1, 0, 3, 2}

// one bad CSR, through fu_create without and with a rev, and through the pairing engines
void csr_row(const char *what, int32_t n, int64_t e, std::initializer_list<int64_t> rp, std::initializer_list<int32_t> col,
             int code, const std::string &tail) {
  create(what, n, e, I64(rp), I32(col), nullptr, code, tail);
  create(what, n, e, I64(rp), I32(col), PATH_REV, code, tail);
  pairing(what, n, e, I64(rp), I32(col), nullptr, code, tail);
  pairing(what, n, e, I64(rp), I32(col), PATH_REV, code, tail);
  expect(what, fu::check_csr("fu_batch_create", n, e, I64(rp).get(), I32(col).get()), code, "fu_batch_create: " + tail);
}

}  // namespace

int main() {
  // the scalars and the null pointers
  create("null out", 3, 4, PATH_RP, PATH_COL, nullptr, ARG, kBad, kValue, nullptr);
  create("null rowptr", 3, 4, nullptr, PATH_COL, nullptr, ARG, kBad);
  create("null value", 3, 4, PATH_RP, PATH_COL, nullptr, ARG, kBad, nullptr);
  create("n == 0", 0, 4, PATH_RP, PATH_COL, nullptr, ARG, kBad);
  create("n < 0", -3, 4, PATH_RP, PATH_COL, nullptr, ARG, kBad);
  create("e < 0", 3, -1, PATH_RP, PATH_COL, nullptr, ARG, kBad);
  create("e > 0, null col", 3, 4, PATH_RP, nullptr, nullptr, ARG, kBad);
  // only the scalar e is large
  create("e = 2^31", 3, (int64_t)1 << 31, PATH_RP, PATH_COL, nullptr, ARG, kMany);
  create("e = INT32_MAX - 64", 3, (int64_t)INT32_MAX - 64, PATH_RP, PATH_COL, PATH_REV, ARG, kMany);
  create("e = INT32_MAX - 65", 3, (int64_t)INT32_MAX - 65, PATH_RP, PATH_COL, nullptr, ARG, kEnds);
  // the CSR
  csr_row("rowptr[0] != 0", 3, 4, {1, 1, 3, 4}, PATH_COL, ARG, kEnds);
  csr_row("rowptr[n] != e", 3, 3, PATH_RP, PATH_COL, ARG, kEnds);
  csr_row("rowptr not monotone", 3, 4, {0, 3, 1, 4}, PATH_COL, ARG, kMono);
  csr_row("rowptr [0, 100, 4]", 2, 4, {0, 100, 4}, {1, 1, 0, 0}, ARG, kMono);
  csr_row("rowptr [0, 100, 2, 4]", 3, 4, {0, 100, 2, 4}, PATH_COL, ARG, kMono);
  csr_row("rowptr [0, 2^40, 4]", 2, 4, {0, (int64_t)1 << 40, 4}, {1, 1, 0, 0}, ARG, kMono);
  csr_row("rowptr [0, -5, 4]", 2, 4, {0, -5, 4}, {1, 1, 0, 0}, ARG, kMono);
  csr_row("rowptr [0, 1, -100, 4]", 3, 4, {0, 1, -100, 4}, PATH_COL, ARG, kMono);
  csr_row("col too large", 3, 4, PATH_RP, {1, 3000, 2, 1}, ARG, kCol + "1");
  csr_row("col == n", 3, 4, PATH_RP, {1, 0, 3, 1}, ARG, kCol + "2");
  csr_row("col negative", 3, 4, PATH_RP, {1, 0, 2, -1}, ARG, kCol + "3");
  csr_row("col INT32_MIN", 3, 4, PATH_RP, {INT32_MIN, 0, 2, 1}, ARG, kCol + "0");
  csr_row("self-loop", 3, 4, PATH_RP, {1, 1, 2, 1}, GRAPH, "self-loop at node 1");
  create("self-loop, rev[k] == k", 2, 4, {0, 2, 4}, {0, 1, 0, 1}, {0, 2, 1, 3}, GRAPH, "self-loop at node 0");
  create("self-loop on the last row", 2, 4, {0, 1, 4}, {1, 0, 1, 1}, nullptr, GRAPH, "self-loop at node 1");
  // the rev
  create("rev too large", 3, 4, PATH_RP, PATH_COL, {1, 0, 4, 2}, GRAPH, kRev + "2");
  create("rev far too large", 3, 4, PATH_RP, PATH_COL, {1, 0, 3, INT32_MAX}, GRAPH, kRev + "3");
  create("rev negative", 3, 4, PATH_RP, PATH_COL, {-1, 0, 3, 2}, GRAPH, kRev + "0");
  create("rev into the wrong row", 3, 4, PATH_RP, PATH_COL, {3, 2, 1, 0}, GRAPH, kRev + "0");
  // a triangle: slot 0 (0 -> 1) names slot 3 of row 1, which holds 2, not 0
  create("rev at another node's slot", 3, 6, {0, 2, 4, 6}, {1, 2, 0, 2, 0, 1}, {3, 4, 0, 5, 1, 2}, GRAPH, kRev + "0");
  pairing("rev too large", 3, 4, PATH_RP, PATH_COL, {1, 0, 4, 2}, GRAPH, kRev + "2");
  pairing("rev negative", 3, 4, PATH_RP, PATH_COL, {-1, 0, 3, 2}, GRAPH, kRev + "0");
  pairing("rev into the wrong row", 3, 4, PATH_RP, PATH_COL, {3, 2, 1, 0}, GRAPH, kRev + "0");
  create("asymmetric, no rev", 2, 1, {0, 1, 1}, {1}, nullptr, GRAPH, kAsym);
  pairing("asymmetric, no rev", 2, 1, {0, 1, 1}, {1}, nullptr, GRAPH, kAsym);
  // a partition: 2 local rows, 1 ghost slot (id 2)
  dist("col == n_local + n_ghost_a", 2, 3, {0, 1, 3}, {1, 0, 3}, 1, ARG, "fu_create: " + kCol + "2");
  dist("col == n_local + n_ghost_a - 1", 2, 3, {0, 1, 3}, {1, 0, 2}, 1, 0, "");
  dist("ghost column without a ghost", 2, 3, {0, 1, 3}, {1, 0, 2}, 0, ARG, "fu_create: " + kCol + "2");
  dist("rowptr not monotone", 2, 3, {0, 100, 3}, {1, 0, 2}, 1, ARG, "fu_create: " + kMono);
  dist("negative rowptr", 2, 3, {0, -1, 3}, {1, 0, 2}, 1, ARG, "fu_create: " + kMono);
  dist("local self-loop", 2, 3, {0, 1, 3}, {1, 1, 2}, 1, GRAPH, "fu_dist_create: self-loop at node 1");
  dist("ghost column equal to no local row", 2, 2, {0, 1, 2}, {2, 2}, 1, 0, "");
  // good inputs pass
  create("path of 3", 3, 4, PATH_RP, PATH_COL, nullptr, 0, "");
  create("path of 3 with its rev", 3, 4, PATH_RP, PATH_COL, PATH_REV, 0, "");
  create("no edge, no col", 3, 0, {0, 0, 0, 0}, nullptr, nullptr, 0, "");
  create("no edge, a col array", 3, 0, {0, 0, 0, 0}, {0}, nullptr, 0, "");
  pairing("path of 3", 3, 4, PATH_RP, PATH_COL, nullptr, 0, "");
  pairing("path of 3 with its rev", 3, 4, PATH_RP, PATH_COL, PATH_REV, 0, "");
  std::printf("%d cases, %d failed\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
