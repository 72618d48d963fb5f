// nmfc_norm.hpp -- calculateNorm and calculateMaxchange partials (the nmf_mu drop-in's reductions, compat.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmfc_common.hpp"

namespace nmfc {

// ---------------------------------------------------------------------------------------------
// calculateNorm (calculatenorm.c:44-78) and calculateMaxchange (calculatemaxchange.c:42-71)
// ---------------------------------------------------------------------------------------------
// grid (x: gene blocks of NT, y: column groups); block (x, y) covers genes x*NT.. of columns y, y + gridDim.y, ...
static __global__ __launch_bounds__(NT) void k_norm_partial(const double* __restrict__ a, const double* __restrict__ w,
                                                            const double* __restrict__ h, double* __restrict__ d, int m,
                                                            int n, int k, double* __restrict__ partial) {
  __shared__ double red[NT];
  const int i = blockIdx.x * NT + threadIdx.x;
  double ss = 0.0;
  if (i < m) {
    for (int j = blockIdx.y; j < n; j += gridDim.y) {
      const long idx = (long)j * m + i;
      double s = 0.0;
      for (int q = 0; q < k; ++q) s = fma(w[i + (long)q * m], h[q + (long)j * k], s);
      const double v = a[idx] - s;
      d[idx] = v;
      ss = fma(v, v, ss);
    }
  }
  red[threadIdx.x] = ss;
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// The same pass for rank K <= 16 known at compile time: the thread's row of W is loaded once into
// registers, the column of H is wave-uniform (scalar loads), and 4 columns are in flight per step, so the
// pass streams A in and d out at HBM rate instead of re-reading W per element.  Per element the sum over
// q runs in q order with fma, as k_norm_partial (identical d); the per-block partial of v^2 likewise.
template <int K>
static __global__ __launch_bounds__(NT) void k_norm_partial_k(const double* __restrict__ a, const double* __restrict__ w,
                                                              const double* __restrict__ h, double* __restrict__ d, int m,
                                                              int n, double* __restrict__ partial) {
  __shared__ double red[NT];
  const int i = blockIdx.x * NT + threadIdx.x;
  double ss = 0.0;
  if (i < m) {
    double wr[K];
#pragma unroll
    for (int q = 0; q < K; ++q) wr[q] = w[i + (long)q * m];
    constexpr int U = 4;
    int j = blockIdx.y;
    for (; j + (U - 1) * (int)gridDim.y < n; j += U * gridDim.y) {
      double av[U], sv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) av[u] = a[(long)(j + u * gridDim.y) * m + i];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double* hc = h + (long)(j + u * gridDim.y) * K;
        double sacc = 0.0;
#pragma unroll
        for (int q = 0; q < K; ++q) sacc = fma(wr[q], hc[q], sacc);
        sv[u] = sacc;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double v = av[u] - sv[u];
        d[(long)(j + u * gridDim.y) * m + i] = v;
        ss = fma(v, v, ss);
      }
    }
    for (; j < n; j += gridDim.y) {
      const double* hc = h + (long)j * K;
      double sacc = 0.0;
#pragma unroll
      for (int q = 0; q < K; ++q) sacc = fma(wr[q], hc[q], sacc);
      const double v = a[(long)j * m + i] - sacc;
      d[(long)j * m + i] = v;
      ss = fma(v, v, ss);
    }
  }
  red[threadIdx.x] = ss;
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

static __global__ __launch_bounds__(NT) void k_maxchange_partial(const double* __restrict__ mat,
                                                                 double* __restrict__ mat0, long len,
                                                                 double* __restrict__ partial) {
  __shared__ double r0[NT], r1[NT];
  double mx0 = 0.0, mxd = 0.0;
  for (long idx = (long)blockIdx.x * NT + threadIdx.x; idx < len; idx += (long)gridDim.x * NT) {
    const double v0 = mat0[idx];
    mx0 = fmax(mx0, fabs(v0));
    const double dv = v0 - mat[idx];
    mat0[idx] = dv;
    mxd = fmax(mxd, fabs(dv));
  }
  r0[threadIdx.x] = mx0;
  r1[threadIdx.x] = mxd;
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      r0[threadIdx.x] = fmax(r0[threadIdx.x], r0[threadIdx.x + off]);
      r1[threadIdx.x] = fmax(r1[threadIdx.x], r1[threadIdx.x + off]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = r0[0];
    partial[2 * blockIdx.x + 1] = r1[0];
  }
}

}  // namespace nmfc
