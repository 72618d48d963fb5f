// generic.hip -- nmf_mu for ranks above the batched engine's limit (k > 16; the reference's nmf_mu takes any k,
// nmf_mu.c:84-85).  One restart per call, on the GPU: the six products of nmf_mu.c:174-202 as plain fp64
// contractions (one thread per output element, a sequential fma chain over K: deterministic), the two
// multiplicative rules (nmf_mu.c:184-191, 209-216) and the stability check (nmf_mu.c:253-282) as small kernels.
// Layouts are the reference's: A m x n, W m x k, H k x n, all column-major.  A rare path (consensus clustering
// sweeps k = 2..10 or so); the fast paths are the team kernel and the batched engine (engine.hip).
// Cost: W^T A runs k n threads, each a serial chain over all m genes, and an iteration is 9 dependent launches, so on a
// large matrix (e.g. 60000 x 2000 at k = 20: 40000 threads x 60000 dependent fmas) one iteration takes on the order of
// milliseconds -- correct and deterministic, not fast.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/nmfc.h"
#include "nmfc_host.hpp"
#include "nmfc_internal.hpp"
#include "nmfc_common.hpp"

namespace {

constexpr int GB = 256;

// C(r, c) = sum_{t < K} P(t, r) Q(t, c); element (t, r) of P at P[t * pt + r * pr], (t, c) of Q at Q[t * qt + c * qc],
// C(r, c) at C[r * cr + c * cc].  One thread per output, t in order.
__global__ __launch_bounds__(GB) void k_gen_prod(int M, int N, int K, const double* __restrict__ P, long pt, long pr,
                                                 const double* __restrict__ Q, long qt, long qc, double* __restrict__ C,
                                                 long cr, long cc) {
  const long x = (long)blockIdx.x * GB + threadIdx.x;
  if (x >= (long)M * N) return;
  const long r = x % M, c = x / M;
  const double* p = P + r * pr;
  const double* q = Q + c * qc;
  double s = 0.0;
  for (int t = 0; t < K; ++t) s = fma(p[t * pt], q[t * qt], s);
  C[r * cr + c * cc] = s;
}

// x = mu_rule(x, num, den) elementwise (nmf_mu.c:184-191 / 209-216), unless the restart has stopped
__global__ __launch_bounds__(GB) void k_gen_rule(long len, double* __restrict__ x, const double* __restrict__ num,
                                                 const double* __restrict__ den, const int* __restrict__ state) {
  if (state[0]) return;
  const long i = (long)blockIdx.x * GB + threadIdx.x;
  if (i < len) x[i] = nmfc::mu_rule(x[i], num[i], den[i]);
}

// state: [0] stopped, [1] stop iteration, [2] reason (1 stable, 2 maxiter), [3] unchanged checks; cls[n] classes.
// REF_COMPAT: window i < min(k, n) of the flat k x n buffer, class = last jj in [1, k) with h[i n + jj] > h[i n + jj - 1]
// (windows i >= k would read past the buffer, nmf_mu.c:259: the zero padding keeps them at class 0).
__global__ __launch_bounds__(GB) void k_gen_check(int iter, int maxiter, int stop_rule, int k, int n,
                                                  const double* __restrict__ H, int* __restrict__ cls,
                                                  int* __restrict__ state) {
  __shared__ int changed;
  if (state[0]) return;
  if (threadIdx.x == 0) changed = 0;
  __syncthreads();
  const bool check = stop_rule != nmfc::STOP_FIXED && iter > 1 && (iter % 2 == 0);
  if (check) {
    if (stop_rule == nmfc::STOP_REF_COMPAT) {
      for (int i = threadIdx.x; i < k && i < n; i += GB) {
        int c = 0;
        for (int jj = 1; jj < k; ++jj)
          if (H[(long)i * n + jj] > H[(long)i * n + jj - 1]) c = jj;
        if (cls[i] != c) {
          cls[i] = c;
          changed = 1;
        }
      }
    } else if (stop_rule == nmfc::STOP_ARGMAX_STABLE) {
      for (int j = threadIdx.x; j < n; j += GB) {
        int best = 0;
        double bv = H[(long)j * k];
        for (int a = 1; a < k; ++a)
          if (H[(long)j * k + a] > bv) {
            bv = H[(long)j * k + a];
            best = a;
          }
        if (cls[j] != best) {
          cls[j] = best;
          changed = 1;
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int reason = 0;
    if (check) {
      if (!changed) {
        if (++state[3] >= 200) reason = 1;   // nmf_mu.c:269-271
      } else {
        state[3] = 0;
      }
    }
    if (!reason && iter >= maxiter) reason = 2;
    if (reason) {
      state[0] = 1;
      state[1] = iter;
      state[2] = reason;
    }
  }
}

struct GenCache : nmfc_host::MuCacheBase {   // device copy of the last A and work buffers
  nmfc_host::DevBuf dA, work, state;
  nmfc_host::DevBuf cls;   // the stability check's classes (n of them)
  hipStream_t st = nullptr;
  void drop() {   // lock held
    if (st) (void)hipStreamSynchronize(st);
    for (nmfc_host::DevBuf* b : {&dA, &work, &state, &cls}) b->release();
    if (st) (void)hipStreamDestroy(st);
    st = nullptr;
    drop_key();
  }
};
GenCache& g = *new GenCache;   // never destroyed (nmfc_host.hpp, process exit)

constexpr char WHO[] = "nmfc_mu_generic";   // the entry point HIPCHK reports under

int mu_generic_call(const double* A, int m, int n, int k, int maxiter, int stop_rule, double* W, double* H, int* iters,
                    int* early) {
  const size_t la = (size_t)m * n;
  if (!g.st) HIPCHK(hipStreamCreateWithFlags(&g.st, hipStreamNonBlocking), WHO);
  if (!(g.dA.p && g.key.same(A, m, n))) {
    g.key.set(A, m, n);
    if (g.dA.ensure(la * sizeof(double))) return -1;
    HIPCHK(hipMemcpyAsync(g.dA.p, A, la * sizeof(double), hipMemcpyHostToDevice, g.st), WHO);
  }
  // work: W, H, numerh / hden (k x n), wtw / hht (k x k), numerw / wden (m x k)
  const size_t lw = (size_t)m * k, lh = (size_t)k * n, lk = (size_t)k * k;
  if (g.work.ensure(sizeof(double) * (3 * lw + 3 * lh + 2 * lk)) || g.state.ensure(sizeof(int) * 8) ||
      g.cls.ensure(sizeof(int) * (size_t)n))
    return -1;
  double* dW = g.work.as<double>();
  double* dH = dW + lw;
  double* numw = dH + lh;
  double* denw = numw + lw;
  double* numh = denw + lw;
  double* denh = numh + lh;
  double* wtw = denh + lh;
  double* hht = wtw + lk;
  int* cls = g.cls.as<int>();
  int* state = g.state.as<int>();
  HIPCHK(hipMemsetAsync(cls, 0, sizeof(int) * (size_t)n, g.st), WHO);   // nmf_mu.c:132
  HIPCHK(hipMemsetAsync(state, 0, sizeof(int) * 8, g.st), WHO);
  HIPCHK(hipMemcpyAsync(dW, W, lw * sizeof(double), hipMemcpyHostToDevice, g.st), WHO);
  HIPCHK(hipMemcpyAsync(dH, H, lh * sizeof(double), hipMemcpyHostToDevice, g.st), WHO);
  auto grid = [](long cnt) { return dim3((unsigned)((cnt + GB - 1) / GB)); };
  const double* dA = g.dA.as<double>();
  int hstate[4] = {0, 0, 0, 0};
  int it = 0;
  for (; it < maxiter;) {
    const int chunk = std::min(32, maxiter - it);
    for (int q = 0; q < chunk; ++q) {
      const int iter = ++it;
      // H side (nmf_mu.c:174-191): numerh = W^T A, wtw = W^T W, hden = wtw H, H rule
      hipLaunchKernelGGL(k_gen_prod, grid((long)k * n), dim3(GB), 0, g.st, k, n, m, dW, 1L, (long)m, dA, 1L, (long)m, numh,
                         1L, (long)k);
      hipLaunchKernelGGL(k_gen_prod, grid((long)k * k), dim3(GB), 0, g.st, k, k, m, dW, 1L, (long)m, dW, 1L, (long)m, wtw,
                         1L, (long)k);
      hipLaunchKernelGGL(k_gen_prod, grid((long)k * n), dim3(GB), 0, g.st, k, n, k, wtw, (long)k, 1L, dH, 1L, (long)k, denh,
                         1L, (long)k);
      hipLaunchKernelGGL(k_gen_rule, grid((long)lh), dim3(GB), 0, g.st, (long)lh, dH, numh, denh, state);
      // W side (nmf_mu.c:198-216) with the new h: numerw = A h^T, hht = h h^T, wden = W0 hht, W rule
      hipLaunchKernelGGL(k_gen_prod, grid((long)m * k), dim3(GB), 0, g.st, m, k, n, dA, (long)m, 1L, dH, (long)k, 1L, numw,
                         1L, (long)m);
      hipLaunchKernelGGL(k_gen_prod, grid((long)k * k), dim3(GB), 0, g.st, k, k, n, dH, (long)k, 1L, dH, (long)k, 1L, hht,
                         1L, (long)k);
      hipLaunchKernelGGL(k_gen_prod, grid((long)m * k), dim3(GB), 0, g.st, m, k, k, dW, (long)m, 1L, hht, 1L, (long)k, denw,
                         1L, (long)m);
      hipLaunchKernelGGL(k_gen_rule, grid((long)lw), dim3(GB), 0, g.st, (long)lw, dW, numw, denw, state);
      hipLaunchKernelGGL(k_gen_check, dim3(1), dim3(GB), 0, g.st, iter, maxiter, stop_rule, k, n, dH, cls, state);
    }
    HIPCHK(hipGetLastError(), WHO);
    HIPCHK(hipMemcpyAsync(hstate, state, sizeof(int) * 4, hipMemcpyDeviceToHost, g.st), WHO);
    HIPCHK(hipStreamSynchronize(g.st), WHO);
    if (hstate[0]) break;
  }
  HIPCHK(hipMemcpyAsync(W, dW, lw * sizeof(double), hipMemcpyDeviceToHost, g.st), WHO);
  HIPCHK(hipMemcpyAsync(H, dH, lh * sizeof(double), hipMemcpyDeviceToHost, g.st), WHO);
  HIPCHK(hipMemcpyAsync(hstate, state, sizeof(int) * 4, hipMemcpyDeviceToHost, g.st), WHO);
  HIPCHK(hipStreamSynchronize(g.st), WHO);
  if (iters) *iters = maxiter == 0 ? 0 : hstate[1];
  if (early) *early = hstate[2] == 1;
  return 0;
}

}  // namespace

// nmfc_nmf_mu_release (compat.hip): the device copy of A, the work buffers, the stream and the host copy of A
extern "C" void nmfc_generic_release() {
  std::lock_guard<std::mutex> lock(g.lock);
  g.drop();
}

// The device copy of A, the work buffers and the stream are kept across calls under the rules of
// nmfc_host::cached_call.
extern "C" int nmfc_mu_generic(const double* A, int m, int n, int k, int maxiter, int stop_rule, double* W, double* H,
                               int* iters, int* early) {
  if (!A || !W || !H || m < 1 || n < 1 || k < 1 || k > m || k > n || maxiter < 0 ||
      !nmfc_mu_stop_rule_ok(stop_rule)) {
    nmfc_set_error("nmfc_mu_generic: bad arguments");
    return -1;
  }
  return nmfc_host::cached_call(g, WHO,
                                [&] { return mu_generic_call(A, m, n, k, maxiter, stop_rule, W, H, iters, early); });
}
