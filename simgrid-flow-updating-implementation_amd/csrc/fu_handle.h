// The handle scaffold of the batched, lossy, pairwise and churn engines: included by
// fu_batch.hip, fu_pair.hip and fu_rev_round.h (the round of fu_lossy.hip and fu_churn.hip)
// and, for its stream_base part alone (a handle without targets), by fu_replay.hip. DESIGN.md
// §4.15-4.18.
//
// An engine's handle derives from fu::handle_base, names itself in `kTag` ("fu_batch", ...:
// the prefix of its entry points and of every message), and supplies
//   int launch_round(H *h);             queue round h->round and advance the counter
//   int launch_err(H *h, u64 *slot);    queue max |a - target| of the last round run into
//                                       h->width slots
// as functions at file scope. Everything below is written once over H: open and close, the
// error slots, the uploads and downloads, the run loop with its error trace, the timed loop
// and the small entry points. Where the engines differ on purpose, the difference is an
// argument (max_err's needs_a_round), not a second copy.
//
// Everything but the two base structs has internal linkage: each engine file gets its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fu_common.h"

namespace fu {

using u64 = unsigned long long;

// What every device handle has (the tick replay's, fu_replay.hip, has nothing more of the below).
struct stream_base {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

struct handle_base : stream_base {
  int32_t n = 0;
  int32_t width = 1;  // error slots per check: 1, or the batch's K
  int64_t E = 0;
  int64_t round = 0;
  bool has_target = false;
  double *target = nullptr;  // n * width
  u64 *err = nullptr;        // errcap slots, width per check
  int64_t errcap = 0;
};

namespace {

// ---- kernels ------------------------------------------------------------------------------
// max_i |a_i - target_i| as a uint64 bit pattern, the rule of the scalar engine's k_max_err:
// non-negative doubles order like their bits, and a NaN with its sign cleared is above +inf,
// so one NaN makes the result NaN.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_max_err(int n, const double *__restrict__ a, const double *__restrict__ target,
                                                   u64 *__restrict__ err) {
  u64 m = 0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    const u64 x = (u64)__double_as_longlong(fabs(a[i] - target[i]));
    m = x > m ? x : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const u64 y = __shfl_xor(m, off, 64);
    m = m > y ? m : y;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(err, m);
}

// k_max_err over the alive nodes only (the churn engine's and the pair engine's under a
// topology): a dead node's frozen estimate never enters the maximum, and with no node alive the
// slot keeps its +0.0.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_max_err_alive(int n, const double *__restrict__ a, const double *__restrict__ target,
                                                         const unsigned char *__restrict__ alive, u64 *__restrict__ err) {
  u64 m = 0;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
    if (!alive[i]) continue;
    const u64 x = (u64)__double_as_longlong(fabs(a[i] - target[i]));
    m = x > m ? x : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const u64 y = __shfl_xor(m, off, 64);
    m = m > y ? m : y;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(err, m);
}

// The block's sum of cnt, added to *dst with one atomic if it is not zero. Every thread of the
// block calls it; cnt is left holding its wave's sum.
template <int BLOCK>
__device__ inline void block_count_to(int &cnt, u64 *dst) {
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  __shared__ int s_w[BLOCK / 64];
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int q = 0; q < BLOCK / 64; ++q) t += s_w[q];
    if (t) atomicAdd(dst, (u64)t);
  }
}

// ---- helpers ------------------------------------------------------------------------------
template <typename H>
int bad_arguments(const char *entry) {
  return fail(FU_ERR_ARG, std::string(H::kTag) + "_" + entry + ": bad arguments");
}

inline int set_device(const stream_base *h) {
  HIP_TRY(hipSetDevice(h->device));
  return FU_OK;
}

template <typename H, typename T>
int dmalloc(H *, T **p, int64_t count) {
  if (hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * (size_t)std::max<int64_t>(count, 1)) != hipSuccess) {
    *p = nullptr;
    return fail(FU_ERR_ALLOC, std::string(H::kTag) + ": hipMalloc failed");
  }
  return FU_OK;
}

template <typename H>
int err_slots(H *h, int64_t count) {
  if (count <= h->errcap) return FU_OK;
  if (h->err) hipFree(h->err);
  h->err = nullptr;
  h->errcap = 0;
  if (int rc = dmalloc(h, &h->err, count)) return rc;
  h->errcap = count;
  return FU_OK;
}

// *_create, after every check on the arguments: the device, the stream and the events. On an
// error the caller destroys the handle.
template <typename H>
int stream_open(H *h, int32_t device) {
  const std::string who = std::string(H::kTag) + "_create";
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FU_ERR_HIP, who + ": no HIP device visible");
  if (device < 0 || device >= ndev) return fail(FU_ERR_ARG, who + ": device out of range");
  h->device = device;
  if (int rc = set_device(h)) return rc;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    return fail(FU_ERR_HIP, who + ": hipStreamCreate failed");
  if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess)
    return fail(FU_ERR_HIP, who + ": hipEventCreate failed");
  return FU_OK;
}
// The same, and the buffers every round engine has.
template <typename H>
int handle_open(H *h, int32_t device, int32_t n, int64_t e, int32_t width) {
  h->n = n;
  h->E = e;
  h->width = width;
  if (int rc = stream_open(h, device)) return rc;
  if (int rc = dmalloc(h, &h->target, (int64_t)n * width)) return rc;
  return err_slots(h, width);
}

// *_destroy: waits for the stream, frees the handle's buffers, the events and the stream.
inline void stream_close(stream_base *h, const std::vector<void *> &own) {
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void *p : own)
    if (p) (void)hipFree(p);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}
inline void handle_close(handle_base *h, std::vector<void *> own) {
  own.insert(own.end(), {h->target, h->err});
  stream_close(h, own);
}

// *_create: count elements of T to or at dst, synchronously; nothing for count == 0.
template <typename H, typename T>
int put(H *, T *dst, const void *src, int64_t count) {
  if (count > 0 && hipMemcpy(dst, src, sizeof(T) * (size_t)count, hipMemcpyHostToDevice) != hipSuccess)
    return fail(FU_ERR_HIP, std::string(H::kTag) + "_create: upload failed");
  return FU_OK;
}
template <typename H, typename T>
int zero(H *, T *dst, int64_t count) {
  if (count > 0 && hipMemset(dst, 0, sizeof(T) * (size_t)count) != hipSuccess)
    return fail(FU_ERR_HIP, std::string(H::kTag) + "_create: memset failed");
  return FU_OK;
}

// A live handle: over its stream, complete on return.
inline int upload(stream_base *h, void *dst, const void *src, size_t bytes) {
  FU_TRY_BEGIN
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return FU_OK;
  FU_TRY_END
}
inline int download(stream_base *h, void *dst, const void *src, size_t bytes) {
  FU_TRY_BEGIN
  if (bytes == 0) return FU_OK;
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return FU_OK;
  FU_TRY_END
}

// launch_err of an engine with one estimate per node: a is the last round's.
template <int BLOCK>
int launch_max_err(const handle_base *h, const double *a, u64 *slot) {
  const unsigned grid = (unsigned)std::min<int64_t>(1024, ((int64_t)h->n + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(k_max_err<BLOCK>, dim3(grid), dim3(BLOCK), 0, h->stream, h->n, a, h->target, slot);
  HIP_TRY(hipGetLastError());
  return FU_OK;
}

// The same over the alive nodes only.
template <int BLOCK>
int launch_max_err_alive(const handle_base *h, const double *a, const unsigned char *alive, u64 *slot) {
  const unsigned grid = (unsigned)std::min<int64_t>(1024, ((int64_t)h->n + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(k_max_err_alive<BLOCK>, dim3(grid), dim3(BLOCK), 0, h->stream, h->n, a, h->target, alive, slot);
  HIP_TRY(hipGetLastError());
  return FU_OK;
}

// A link is up or down as a whole: FU_ERR_ARG where link_up (may be null: all ones) differs
// between a slot and its reverse. rev has passed check_rev.
inline int check_link_up(const char *who, int64_t e, const int32_t *rev, const uint8_t *link_up) {
  for (int64_t k = 0; link_up && k < e; ++k)
    if ((link_up[k] != 0) != (link_up[rev[k]] != 0))
      return fail(FU_ERR_ARG, std::string(who) + ": link_up differs between slot " + std::to_string(k) + " and its reverse");
  return FU_OK;
}

// *_create_from_graph: the CSR of a symmetric host graph handed to the engine's *_create,
// create(n, e, rowptr, col, rev).
template <typename H, typename Create>
int create_from_graph(const fu_graph *g, const void *value, const void *out, Create create) {
  FU_TRY_BEGIN
  if (!g || !value || !out) return bad_arguments<H>("create_from_graph");
  const int64_t E = g->rowptr[g->n];
  if ((int64_t)g->rev.size() != E) return fail(FU_ERR_GRAPH, std::string(H::kTag) + "_create_from_graph: graph is not symmetric");
  return create(g->n, E, g->rowptr.data(), g->col.data(), E ? g->rev.data() : nullptr);
  FU_TRY_END
}

// ---- the shared entry points ----------------------------------------------------------------
template <typename H>
int set_targets(H *h, const double *target) {
  if (!h || !target) return bad_arguments<H>("set_targets");
  if (int rc = upload(h, h->target, target, sizeof(double) * (size_t)h->n * h->width)) return rc;
  h->has_target = true;
  return FU_OK;
}

// err_every > 0: a check after every err_every-th round of this call, each into its own
// h->width slots; the trace comes back once, after the last round. A failed launch returns at
// once: the rounds queued before it stay queued.
template <typename H>
int run(H *h, int32_t rounds, int32_t err_every, double *err_trace) {
  FU_TRY_BEGIN
  if (!h || rounds < 0) return bad_arguments<H>("run");
  const std::string tag(H::kTag);
  if (err_every > 0 && !h->has_target) return fail(FU_ERR_STATE, tag + "_run: err_every > 0 needs " + tag + "_set_targets");
  if (int rc = set_device(h)) return rc;
  const int64_t slots = err_every > 0 ? (int64_t)(rounds / err_every) * h->width : 0;
  if (slots > 0) {
    if (int rc = err_slots(h, slots)) return rc;
    HIP_TRY(hipMemsetAsync(h->err, 0, sizeof(u64) * (size_t)slots, h->stream));
  }
  for (int32_t r = 0; r < rounds; ++r) {
    if (int rc = launch_round(h)) return rc;
    if (slots > 0 && (r + 1) % err_every == 0)
      if (int rc = launch_err(h, h->err + (int64_t)((r + 1) / err_every - 1) * h->width)) return rc;
  }
  if (slots > 0) {
    std::vector<u64> bits((size_t)slots);
    HIP_TRY(hipMemcpyAsync(bits.data(), h->err, sizeof(u64) * bits.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (err_trace) std::memcpy(err_trace, bits.data(), sizeof(double) * bits.size());
  }
  return FU_OK;
  FU_TRY_END
}

template <typename H>
int run_timed(H *h, int32_t rounds, float *ms) {
  FU_TRY_BEGIN
  if (!h || !ms || rounds < 0) return bad_arguments<H>("run_timed");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  for (int32_t r = 0; r < rounds; ++r)
    if (int rc = launch_round(h)) return rc;
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev1));
  HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return FU_OK;
  FU_TRY_END
}

// out: h->width doubles. needs_a_round: before round 0 the engine has no estimates to compare
// (the pairwise engine has: every node's last average starts at 0.0).
template <typename H>
int max_err(H *h, double *out, bool needs_a_round) {
  FU_TRY_BEGIN
  if (!h || !out) return bad_arguments<H>("max_err");
  const std::string tag(H::kTag);
  if (!h->has_target) return fail(FU_ERR_STATE, tag + "_max_err: call " + tag + "_set_targets first");
  if (needs_a_round && h->round == 0) return fail(FU_ERR_STATE, tag + "_max_err: no round has run");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemsetAsync(h->err, 0, sizeof(u64) * h->width, h->stream));
  if (int rc = launch_err(h, h->err)) return rc;
  std::vector<u64> bits((size_t)h->width);
  HIP_TRY(hipMemcpyAsync(bits.data(), h->err, sizeof(u64) * bits.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::memcpy(out, bits.data(), sizeof(double) * bits.size());
  return FU_OK;
  FU_TRY_END
}

template <typename H>
int get_round(H *h, int64_t *rounds_done) {
  if (!h || !rounds_done) return bad_arguments<H>("get_round");
  *rounds_done = h->round;
  return FU_OK;
}

template <typename H>
int synchronize(H *h) {
  if (!h) return bad_arguments<H>("synchronize");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return FU_OK;
}

}  // namespace
}  // namespace fu
