// nmfc_resid.hpp -- the batched residual pass over the final-factor archive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmfc_common.hpp"

namespace nmfc {

// ---------------------------------------------------------------------------------------------
// Batched residual pass over the final-factor archive (nmfc_engine_set_residuals): the sum of d^2, d = A - W_j H_j,
// of every job, without writing d.  A workgroup owns a tile of RES_GT genes x RES_ST samples of A: each of its four
// waves keeps RES_GT x RES_WJ of it in registers (lane = gene, read once from the K-blocked Ablk) and walks the
// workgroup's RES_JG restarts over it.  Per restart a thread loads its row of W (k registers), the rows of H are
// wave-uniform (scalar loads), and per element s = sum_q w[q] h[q] runs by fma in q order, v = a - s, ss = fma(v, v,
// ss) in sample order: k_norm_partial_k's arithmetic.  Lanes are summed by a fixed butterfly, the four waves in wave
// order, and the (job, tile) partial is stored; k_resid_sum adds a job's partials in tile order.  Tiling and every
// order are functions of (m, n) alone, so a job's sum does not depend on the restarts it shares a launch with, on its
// archive row or on the shard.  Rows >= m and samples >= n contribute exactly 0 whatever the padding holds: such a
// row's sum is dropped, such a sample's a and h are replaced by 0 (its products are then w * 0 = 0 for finite w).
// ---------------------------------------------------------------------------------------------
constexpr int RES_GT = 64;    // genes per tile: one per lane
constexpr int RES_WJ = 16;    // samples per wave (A registers per thread; 32 cost a wave per SIMD: 13.4 against 10.5 ms on C3)
constexpr int RES_ST = 64;    // samples per workgroup tile: four waves
constexpr int RES_JG = 32;    // restarts a workgroup walks over its tile (A is read once per such group)

// RES_WB samples of one restart: B-th block of the wave's RES_WJ; MASK: only the first nvalid of them exist.  Per rank
// index q one run of RES_WB wave-uniform h (one s_load_dwordx16), each feeding one fma of the wave
constexpr int RES_WB = 8;
template <int K, int B, bool MASK>
__device__ __forceinline__ void resid_blkw(const double (&wr)[K], const double* __restrict__ h, long n_pad,
                                           const double (&av)[RES_WJ], int nvalid, double& ss) {
  double s[RES_WB];
#pragma unroll
  for (int u = 0; u < RES_WB; ++u) s[u] = 0.0;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const double* hq = h + q * n_pad + RES_WB * B;
#pragma unroll
    for (int u = 0; u < RES_WB; ++u) {
      double hv = hq[u];
      if (MASK) hv = u < nvalid ? hv : 0.0;
      s[u] = fma(wr[q], hv, s[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < RES_WB; ++u) {
    const double v = av[RES_WB * B + u] - s[u];
    ss = fma(v, v, ss);
  }
}

template <int K, int B>
__device__ __forceinline__ void resid_blk(const double (&wr)[K], const double* __restrict__ h, long n_pad,
                                          const double (&av)[RES_WJ], int ncols, double& ss) {
  const int nvalid = ncols - RES_WB * B;
  if (nvalid >= RES_WB)
    resid_blkw<K, B, false>(wr, h, n_pad, av, RES_WB, ss);
  else if (nvalid > 0)
    resid_blkw<K, B, true>(wr, h, n_pad, av, nvalid, ss);
}

// one thread's sum over the wave's ncols samples for a rank-K restart: w = its gene's first archive entry (rows m_pad
// apart), h = the restart's first archive row at the wave's first sample
template <int K>
__device__ __forceinline__ double resid_job(const double* __restrict__ w, long m_pad, const double* __restrict__ h,
                                            long n_pad, const double (&av)[RES_WJ], int ncols) {
  double wr[K];
#pragma unroll
  for (int q = 0; q < K; ++q) wr[q] = w[q * m_pad];
  // a branch per block of RES_WB samples: the blocks stay apart in the schedule (run together they cost registers
  // worth a wave per SIMD and more)
  double ss = 0.0;
  resid_blk<K, 0>(wr, h, n_pad, av, ncols, ss);
  resid_blk<K, 1>(wr, h, n_pad, av, ncols, ss);
  static_assert(RES_WJ == 2 * RES_WB, "two blocks per wave");
  return ss;
}

// grid (x: tiles, gene tile major, nst sample tiles each; y: groups of RES_JG entries of fi).  fi[r]: col0 = the
// restart's first archive row, k its rank, rid its row in partial (rid x gridDim.x).
static __global__ __launch_bounds__(NT) void k_resid(const RestartInfo* __restrict__ fi, int nj,
                                                     const double* __restrict__ Ablk, long ld,
                                                     const double* __restrict__ Wfin, long m_pad,
                                                     const double* __restrict__ Hfin, long n_pad, int m, int n, int nst,
                                                     double* __restrict__ partial) {
  __shared__ double red[RES_JG][4];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int tile = blockIdx.x, gt = tile / nst, stl = tile - gt * nst;
  const int i = gt * RES_GT + lane;                    // < m_pad (a multiple of GT = 2 RES_GT)
  const int j0 = stl * RES_ST + wave * RES_WJ;         // the wave's first sample
  const int ncols = min(RES_WJ, n - j0);               // <= 0: no sample of A left for this wave
  const int r0 = blockIdx.y * RES_JG, r1 = min(nj, r0 + RES_JG);
  if (ncols > 0) {   // then j0 + RES_WJ <= n_pad (j0 and n_pad multiples of RES_WJ, j0 < n): every H read stays inside its row
    double av[RES_WJ];
    const double* ap = Ablk + (long)(i >> 4) * ld * 16 + (long)j0 * 16 + (i & 15);
#pragma unroll
    for (int u = 0; u < RES_WJ; ++u) {
      const double a = ap[u * 16];
      av[u] = u < ncols ? a : 0.0;
    }
#pragma unroll 1
    for (int r = r0; r < r1; ++r) {
      const RestartInfo me = fi[r];
      const double* w = Wfin + (long)me.col0 * m_pad + i;
      const double* h = Hfin + (long)me.col0 * n_pad + j0;
      double ss = 0.0;
      switch (me.k) {
#define NMFC_RES_K(KK) \
  case KK: ss = resid_job<KK>(w, m_pad, h, n_pad, av, ncols); break;
        NMFC_RES_K(2) NMFC_RES_K(3) NMFC_RES_K(4) NMFC_RES_K(5) NMFC_RES_K(6) NMFC_RES_K(7) NMFC_RES_K(8)
        NMFC_RES_K(9) NMFC_RES_K(10) NMFC_RES_K(11) NMFC_RES_K(12) NMFC_RES_K(13) NMFC_RES_K(14) NMFC_RES_K(15)
        NMFC_RES_K(16)
#undef NMFC_RES_K
        default: break;   // the engine takes ranks 2..KMAX only
      }
      ss = i < m ? ss : 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
      if (lane == 0) red[r - r0][wave] = ss;
    }
  } else if (lane == 0) {
    for (int r = r0; r < r1; ++r) red[r - r0][wave] = 0.0;
  }
  __syncthreads();
  if ((int)threadIdx.x < r1 - r0) {
    const double* p = red[threadIdx.x];
    partial[(long)fi[r0 + threadIdx.x].rid * gridDim.x + tile] = ((p[0] + p[1]) + p[2]) + p[3];
  }
}

// ssq[slot[rid]] = the job's ntiles partials added in tile order: lane l takes tiles l, l + 64, ..., then the butterfly
static __global__ __launch_bounds__(64) void k_resid_sum(const double* __restrict__ partial, int ntiles,
                                                         const int* __restrict__ slot, double* __restrict__ ssq) {
  const int rid = blockIdx.x;
  const double* p = partial + (long)rid * ntiles;
  double s = 0.0;
  for (int t = threadIdx.x; t < ntiles; t += 64) s += p[t];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) ssq[slot[rid]] = s;
}

}  // namespace nmfc
