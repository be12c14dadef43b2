// A HOST-ONLY stand-in for <hip/hip_runtime.h>, for ONE purpose: building the boundary's host logic (mina_bridge_amd/csrc/api_verify.hip: slots, group commit,
// culprit search, shape vote, device sharding) with g++ -fsanitize=thread and hammering it from many caller threads WITHOUT a GPU (tests/fuzz/tsan_boundary.cpp).
// Streams execute their commands at once on the calling thread (a valid in-order schedule of every stream), events are already complete when recorded, device
// memory is host memory.  Test infrastructure: never part of the product build (mina_bridge_amd/build.py uses hipcc and the real runtime).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#define MB_HIP_STUB 1
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
#ifndef __restrict__
#define __restrict__ __restrict
#endif
typedef int hipError_t;
enum : int { hipSuccess = 0, hipErrorInvalidValue = 1 };
struct mb_stub_stream { int id; };
struct mb_stub_event { int done; int id; };
typedef mb_stub_stream *hipStream_t;
typedef mb_stub_event *hipEvent_t;
// -DMB_STUB_TRACE (tsan_boundary.cpp `trace`, tests/test_boundary_trace.py): every call that orders or moves something writes one line to stdout -- what the
// boundary asks of the runtime, in the order it asks.  Streams, events and allocations are named by creation order (s1, e1, m1 ..; s0 / e0 = null), never by
// address; a pointer is its allocation + offset, `host` outside every allocation.  For ONE calling thread: the names are plain counters.
#if defined(MB_STUB_TRACE)
#include <cstdio>
#include <map>
#include <string>
struct mb_stub_names { int streams = 0, events = 0, allocs = 0; std::map<const char *, std::pair<int, size_t>> mem; };
inline mb_stub_names &mb_stub_trace() { static mb_stub_names t; return t; }
inline std::string mb_stub_mem(const void *p) {
    auto &m = mb_stub_trace().mem; auto it = m.upper_bound((const char *)p);
    if (it == m.begin() || (size_t)((const char *)p - (--it)->first) >= it->second.second) return "host";
    return "m" + std::to_string(it->second.first) + "+" + std::to_string((const char *)p - it->first);
}
#define MB_TRACE(...) printf(__VA_ARGS__)
#define MB_TRACE_ID(counter) (++mb_stub_trace().counter)
#if defined(MB_STUB_TRACE_QUIET_ALLOC)      // allocations keep their names but write no line (trace_state_job.cpp: a log of streams and events)
#define MB_TRACE_ALLOC(what, p, n) do { const int id_ = MB_TRACE_ID(allocs); mb_stub_trace().mem[(const char *)(p)] = {id_, (n) ? (n) : 1}; } while (0)
#define MB_TRACE_FREE(what, p) do { if (p) mb_stub_trace().mem.erase((const char *)(p)); } while (0)
#else
#define MB_TRACE_ALLOC(what, p, n) do { const int id_ = MB_TRACE_ID(allocs); mb_stub_trace().mem[(const char *)(p)] = {id_, (n) ? (n) : 1}; printf("%s %zu -> m%d\n", what, (size_t)(n), id_); } while (0)
#define MB_TRACE_FREE(what, p) do { if (p) { printf("%s %s\n", what, mb_stub_mem(p).c_str()); mb_stub_trace().mem.erase((const char *)(p)); } } while (0)
#endif
#else
#define MB_TRACE(...) ((void)0)
#define MB_TRACE_ID(counter) 0
#define MB_TRACE_ALLOC(what, p, n) ((void)0)
#define MB_TRACE_FREE(what, p) ((void)0)
#endif
static inline int mb_stub_id(hipStream_t s) { return s ? s->id : 0; }
static inline int mb_stub_id(hipEvent_t e) { return e ? e->id : 0; }
static const char *const mb_stub_kind[5] = {"H2H", "H2D", "D2H", "D2D", "default"};
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipHostMallocDefault = 0, hipDeviceAttributeMultiprocessorCount = 63 };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }
static const dim3 blockIdx, blockDim, threadIdx, gridDim;
static inline const char *hipGetErrorString(hipError_t) { return "stub"; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipSetDevice(int) { return hipSuccess; }
static inline hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
static inline hipError_t hipDeviceGetAttribute(int *v, int, int) { *v = 256; return hipSuccess; }
static inline hipError_t hipDeviceSynchronize() { MB_TRACE("hipDeviceSynchronize\n"); return hipSuccess; }
// Live allocations: hipMalloc + hipHostMalloc less the frees of non-null pointers, over every translation unit (atomic: the ThreadSanitizer build counts too).  A
// program that has destroyed everything checks mb_stub_live_allocs() == 0: a buffer nobody freed shows without a list of buffers.
inline std::atomic<long> &mb_stub_live() { static std::atomic<long> n{0}; return n; }
static inline long mb_stub_live_allocs() { return mb_stub_live().load(); }
static inline hipError_t mb_stub_alloc(const char *what, void **p, size_t n) { *p = calloc(1, n ? n : 1); if (!*p) return hipErrorInvalidValue; mb_stub_live().fetch_add(1); MB_TRACE_ALLOC(what, *p, n); return hipSuccess; }
static inline void mb_stub_free(const char *what, void *p) { if (p) mb_stub_live().fetch_sub(1); MB_TRACE_FREE(what, p); free(p); }
static inline hipError_t hipMalloc(void **p, size_t n) { return mb_stub_alloc("hipMalloc", p, n); }
template <class T> static inline hipError_t hipMalloc(T **p, size_t n) { return hipMalloc((void **)p, n); }
static inline hipError_t hipFree(void *p) { mb_stub_free("hipFree", p); return hipSuccess; }
static inline hipError_t hipHostMalloc(void **p, size_t n, unsigned = 0) { return mb_stub_alloc("hipHostMalloc", p, n); }
static inline hipError_t hipHostFree(void *p) { mb_stub_free("hipHostFree", p); return hipSuccess; }
static inline hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { MB_TRACE("hipMemcpy %s %zu %s <- %s\n", mb_stub_kind[k], n, mb_stub_mem(d).c_str(), mb_stub_mem(s).c_str()); memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st = nullptr) {
    MB_TRACE("hipMemcpyAsync %s %zu %s <- %s on s%d\n", mb_stub_kind[k], n, mb_stub_mem(d).c_str(), mb_stub_mem(s).c_str(), mb_stub_id(st)); memcpy(d, s, n); return hipSuccess;
}
static inline hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t = nullptr) { memset(d, v, n); return hipSuccess; }
static inline hipError_t hipMemset(void *d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
static inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = new mb_stub_stream{MB_TRACE_ID(streams)}; MB_TRACE("hipStreamCreateWithFlags -> s%d\n", (*s)->id); return hipSuccess; }
static inline hipError_t hipExtStreamCreateWithCUMask(hipStream_t *s, uint32_t n, const uint32_t *mask) {
    *s = new mb_stub_stream{MB_TRACE_ID(streams)}; MB_TRACE("hipExtStreamCreateWithCUMask -> s%d, mask", (*s)->id); for (uint32_t i = 0; i < n; ++i) MB_TRACE(" %08x", mask[i]); MB_TRACE("\n"); return hipSuccess;
}
static inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int priority) { *s = new mb_stub_stream{MB_TRACE_ID(streams)}; MB_TRACE("hipStreamCreateWithPriority %d -> s%d\n", priority, (*s)->id); return hipSuccess; }
static inline hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { *least = 0; *greatest = -1; return hipSuccess; }      // (numerically lower = higher priority)
static inline hipError_t hipStreamDestroy(hipStream_t s) { MB_TRACE("hipStreamDestroy s%d\n", mb_stub_id(s)); delete s; return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t s) { MB_TRACE("hipStreamSynchronize s%d\n", mb_stub_id(s)); return hipSuccess; }
static inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { MB_TRACE("hipStreamWaitEvent s%d waits for e%d\n", mb_stub_id(s), mb_stub_id(e)); return hipSuccess; }
static inline hipError_t hipEventCreate(hipEvent_t *e) { *e = new mb_stub_event{1, MB_TRACE_ID(events)}; MB_TRACE("hipEventCreate -> e%d\n", (*e)->id); return hipSuccess; }
static inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
static inline hipError_t hipEventDestroy(hipEvent_t e) { MB_TRACE("hipEventDestroy e%d\n", mb_stub_id(e)); delete e; return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s = nullptr) { MB_TRACE("hipEventRecord e%d on s%d\n", mb_stub_id(e), mb_stub_id(s)); return hipSuccess; }
static inline hipError_t hipEventSynchronize(hipEvent_t e) { MB_TRACE("hipEventSynchronize e%d\n", mb_stub_id(e)); return hipSuccess; }
static inline hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
