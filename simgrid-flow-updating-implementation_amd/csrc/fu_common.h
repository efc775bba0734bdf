// Internal helpers shared by the libfu translation units.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "fu.h"

namespace fu {

// Thread-local last error (fu_last_error).
void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// The hash helpers also run in kernels (fu_lossy.hip): one definition for host and device.
#if defined(__HIPCC__)
#define FU_HD __host__ __device__
#else
#define FU_HD
#endif

FU_HD inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// Element i of the SplitMix64 stream seeded with `seed` (counter form, thread-count free).
FU_HD inline uint64_t splitmix_at(uint64_t seed, uint64_t i) { return mix64(seed + (i + 1) * kGolden); }
// Sequential SplitMix64 step (same as the Python oracle's splitmix64()).
inline uint64_t splitmix_next(uint64_t &state) {
  state += kGolden;
  return mix64(state);
}
FU_HD inline double u01(uint64_t x) { return (double)(x >> 11) * 0x1.0p-53; }

}  // namespace fu

// Host graph: CSR with int64 row pointer on the host (device copies use int32).
struct fu_graph {
  int32_t n = 0;
  std::vector<int64_t> rowptr;  // n + 1
  std::vector<int32_t> col;     // E
  std::vector<int32_t> rev;     // E, empty if not symmetric
  int32_t max_deg = 0;
};

namespace fu {
// Builds rev for g (fails if some i->j lacks j->i). Parallel, deterministic.
int build_rev(fu_graph &g);

// What fu_batch_create, fu_lossy_create and fu_pair_create ask of a caller's CSR, on the host
// and before any HIP call; `who` is the entry point's name, for the message.
// rowptr[0] == 0, rowptr[n] == e, rowptr monotone, every col in [0, n), all FU_ERR_ARG; then no
// row holds its own id (FU_ERR_GRAPH, "<who>: self-loop at node i": fu_graph_from_csr's rule).
// No array is read past what the checks before it have proved to be there.
int check_csr(const char *who, int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col);
// The same for one rank's rows of a partition: columns run to ncols = n_local + n_ghost_a (a
// ghost column is never a self-loop), and the self-loop text carries loop_who.
int check_csr_cols(const char *who, const char *loop_who, int32_t n, int64_t ncols, int64_t e, const int64_t *rowptr,
                   const int32_t *col);
// Everything fu_create, fu_create_from_graph and fu_dist_create(_local) ask of their arguments
// ahead of the device probe, in this order: the null, n and e checks, e < INT32_MAX - 64, then
// check_csr_cols with the texts under "fu_create" and ncols = n + a_extra.
int check_create(const char *loop_who, int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                 const double *value, int32_t a_extra, const void *out);
// All of fu_create's checks: check_create, then symmetry: a caller's rev as check_rev(kSymmetric),
// none as rev_of_csr's verdict.
int check_fu_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                    const double *value, const void *out);
// rev against a CSR that passed check_csr. kSymmetric: rev[k] lies in the row of k's neighbour
// at a slot that points back, which proves the graph symmetric (the batched engine never reads
// rev on the device). kPairing: rev is an involution as well (the lossy and pairwise engines
// gather through it: anything less would be an out-of-bounds or wrong access there).
enum class RevCheck { kSymmetric, kPairing };
int check_rev(const char *who, RevCheck level, int32_t n, const int64_t *rowptr, const int32_t *col, const int32_t *rev);
// build_rev for a caller's CSR: the reverse-edge index in *rev, or with rev == nullptr only
// the verdict (FU_ERR_GRAPH if some i -> j lacks its j -> i).
int rev_of_csr(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, std::vector<int32_t> *rev);
// The engines that gather through rev (lossy, churn, pairwise), before their first HIP call:
// the CSR checked, *rev built into *built where the caller gave none, and checked as a pairing.
int pairing_rev(const std::string &who, int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                const int32_t **rev, std::vector<int32_t> *built);
}  // namespace fu

// A HIP call that fails ends the calling entry point with FU_ERR_HIP and the call's text (the
// device translation units; <hip/hip_runtime.h> is theirs to include).
#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return fu::fail(FU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
  } while (0)

#define FU_TRY_BEGIN try {
#define FU_TRY_END                                                   \
  }                                                                  \
  catch (const std::bad_alloc &) {                                   \
    return fu::fail(FU_ERR_ALLOC, "host allocation failed");         \
  }                                                                  \
  catch (const std::exception &ex) {                                 \
    return fu::fail(FU_ERR_ARG, std::string("exception: ") + ex.what()); \
  }
