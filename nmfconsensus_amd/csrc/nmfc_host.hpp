// nmfc_host.hpp -- the host runtime every translation unit of the library shares (engine.hip, brunet.hip, solo.hip,
// generic.hip, compat.hip): error reporting into the thread's error slot, device and pinned buffers, launch timing
// and the shared part of the nmf_mu drop-in's per-process caches.  Host only: no kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "nmfc_internal.hpp"

namespace nmfc_host {

// ---- error reporting: one formatted message into the thread's error slot (nmfc_last_error) ----

__attribute__((format(printf, 1, 2))) inline void errorf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  nmfc_set_error(buf);
}

// "<who>: <what>: <HIP's message>", -1: the failure of one named step of an entry point
inline int hip_fail(const char* who, const char* what, hipError_t e) {
  errorf("%s: %s: %s", who, what, hipGetErrorString(e));
  return -1;
}

inline int check_failed(const char* expr, hipError_t e, const char* file, int line, const char* who = nullptr) {
  if (who) return hip_fail(who, expr, e);
  errorf("%s failed: %s (%s:%d)", expr, hipGetErrorString(e), file, line);
  return -1;
}

// returns -1 from the calling function when a hipError_t expression fails; HIPCHK(expr, "entry") reports it
// under that entry point's name, HIPCHK(expr) with the source position
#define HIPCHK(expr, ...)                                                                               \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return nmfc_host::check_failed(#expr, e_, __FILE__, __LINE__, ##__VA_ARGS__); \
  } while (0)

inline long round_up(long v, long a) { return (v + a - 1) / a * a; }

// ---- buffers: grow-only, freed on destruction (every early return frees what it allocated), movable ----
// DevBuf is device memory (hipMalloc), PinBuf pinned host memory (hipHostMalloc): staging that small per-iteration
// copies read and write without HIP's shared pageable path.  ensure(need) keeps a buffer that is large enough (so
// ensure(0) does nothing) and otherwise replaces it; the contents are not kept.
template <bool PINNED>
struct HipBuf {
  void* p = nullptr;
  size_t bytes = 0;
  HipBuf() = default;
  HipBuf(const HipBuf&) = delete;
  HipBuf& operator=(const HipBuf&) = delete;
  HipBuf(HipBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  HipBuf& operator=(HipBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      bytes = std::exchange(o.bytes, 0);
    }
    return *this;
  }
  ~HipBuf() { release(); }
  int ensure(size_t need) {
    if (need <= bytes) return 0;
    release();
    const hipError_t e = PINNED ? hipHostMalloc(&p, need, hipHostMallocDefault) : hipMalloc(&p, need);
    if (e != hipSuccess) {
      errorf("%s(%zu) failed: %s", PINNED ? "hipHostMalloc" : "hipMalloc", need, hipGetErrorString(e));
      p = nullptr;
      return -1;
    }
    bytes = need;
    return 0;
  }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};
using DevBuf = HipBuf<false>;
using PinBuf = HipBuf<true>;

// ---- launch timing: HIP events around single launches, read back in one go ----
// A pool of events and the list of recorded (kernel id, start, stop) pairs.  drain() waits for each pair, hands
// (kid, ms) to its owner and returns the events to the pool; the owner keeps its own counters.
struct LaunchTimer {
  struct Pending {
    int kid;
    hipEvent_t a, b;
  };
  std::vector<hipEvent_t> pool;
  std::vector<Pending> pending;
  hipEvent_t take() {
    hipEvent_t ev = nullptr;
    if (!pool.empty()) {
      ev = pool.back();
      pool.pop_back();
    } else if (hipEventCreate(&ev) != hipSuccess) {
      ev = nullptr;
    }
    return ev;
  }
  template <class Owner>
  void drain(Owner&& owner) {   // owner(kid, ms) for every pair whose time could be read
    for (const Pending& pnd : pending) {
      float ms = 0.f;
      if (hipEventSynchronize(pnd.b) == hipSuccess && hipEventElapsedTime(&ms, pnd.a, pnd.b) == hipSuccess)
        owner(pnd.kid, ms);
      pool.push_back(pnd.a);
      pool.push_back(pnd.b);
    }
    pending.clear();
  }
  void destroy_events() {   // after a drain: nothing is pending
    for (hipEvent_t ev : pool) (void)hipEventDestroy(ev);
    pool.clear();
  }
};

// Records an event pair on `st` around the launches of its scope when `on`; a pair that cannot be completed (no
// stop event) is dropped and its start event goes back to the pool.
struct TimedScope {
  LaunchTimer& t;
  hipStream_t st;
  int kid;
  hipEvent_t a = nullptr;
  TimedScope(LaunchTimer& t_, hipStream_t st_, int kid_, bool on) : t(t_), st(st_), kid(kid_) {
    if (on && (a = t.take())) (void)hipEventRecord(a, st);
  }
  TimedScope(const TimedScope&) = delete;
  TimedScope& operator=(const TimedScope&) = delete;
  ~TimedScope() {
    if (!a) return;
    if (hipEvent_t b = t.take()) {
      (void)hipEventRecord(b, st);
      t.pending.push_back({kid, a, b});
    } else {
      t.pool.push_back(a);
    }
  }
};

// ---- the nmf_mu drop-in's per-process caches (compat.hip: an engine; solo.hip, generic.hip: a device copy of A,
// work buffers and a stream) ----
// nmf.r calls nmf_mu once per restart on one data matrix and R passes a fresh copy each time, so the cached
// resources are matched by A's shape and content: a host copy compared byte for byte (one pass over A, and no
// collision can reuse a stale A).
//
// Process exit: a cache object is allocated with `new` and never destroyed (static Cache& g = *new Cache), so no
// HIP call ever runs from a static destructor, where the runtime may already be gone.  What a cache holds is
// released by nmfc_nmf_mu_release() or stays until the process ends.  Never make a DevBuf, a PinBuf or anything
// that owns one a global with a live destructor.
struct MatrixKey {
  std::vector<double> a;
  int m = 0, n = 0;
  bool empty() const { return a.empty(); }
  bool same(const double* A, int m_, int n_) const {
    return !a.empty() && m == m_ && n == n_ && memcmp(a.data(), A, a.size() * sizeof(double)) == 0;
  }
  void set(const double* A, int m_, int n_) {
    a.assign(A, A + (size_t)m_ * n_);
    m = m_;
    n = n_;
  }
  void drop() {
    std::vector<double>().swap(a);
    m = n = 0;
  }
};

// What the three caches share; each derives from it, adds its payload and a drop() that frees the payload and
// calls drop_key().
struct MuCacheBase {
  std::mutex lock;
  MatrixKey key;
  int dev = -1;   // the HIP device every cached resource lives on
  void drop_key() {
    key.drop();
    dev = -1;
  }
};

inline bool mu_cache_enabled() {
  const char* env = getenv("NMFC_NMF_MU_CACHE");
  return !(env && atoi(env) == 0);
}

// Runs call() under the cache's lock.  The cache is dropped before the call when it lives on another device than
// the current one, and after it when the call failed (nothing cached may hold a half-done upload or a broken engine)
// or NMFC_NMF_MU_CACHE=0 (nothing is kept).
template <class Cache, class Call>
int cached_call(Cache& c, const char* who, Call&& call) {
  std::lock_guard<std::mutex> guard(c.lock);
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return hip_fail(who, "hipGetDevice", hipErrorInvalidDevice);
  if (c.dev >= 0 && c.dev != dev) c.drop();
  const int rc = call();
  if (rc != 0 || !mu_cache_enabled())
    c.drop();
  else
    c.dev = dev;
  return rc;
}

}  // namespace nmfc_host
