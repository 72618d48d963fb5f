// brunet.hip -- batched Brunet KL-divergence MU restarts (C ABI nmfc_brunet_* in include/nmfc.h).
//
// The per-restart algorithm is the BROAD nmfconsensus / GenePattern NMF.div (Brunet et al. 2004),
// which the reference names at test_nmf.r:29 but does not ship (restated in
// oracle/brunet_oracle.c, parity against the reference unpinned):
//   VP = W H;  H <- (H * (W^T (A / VP)) + eps) / colSums(W)          (k_br_hnum + k_br_hupd)
//   VP = W H;  W <- (W * ((A / VP) H^T) + eps) / rowSums(H)          (k_br_wupd)
//   every stopfreq iterations: per-sample argmax class, stop after stopconv unchanged checks.
// Init per restart: set.seed(seed + i); W <- runif(m k); H <- runif(k n) (R's Mersenne-Twister, k_br_init).
//
// The quotient A / VP is restart-specific, so the per-iteration work is 2 m n divides plus 8 m n k
// flop of rank-k products per restart with nothing to share but A: these are VALU kernels (fp64 FMA
// + IEEE divide, the divide dominating for small k), not MFMA GEMMs.  A is shared by streaming one A
// element per lane and applying it to RG restarts at once; the per-restart W row (H-side) or H column
// (W-side) is wave-uniform: it comes through scalar loads into SGPR operands, or for some ranks through
// LDS tiles read back by broadcast (the per-k SL table below), and no cross-lane reductions are needed.
// Layouts (per k batch of B restarts):
//   Arm [m][n_pad] (sample-contiguous rows), Acm [n][m_pad] (gene-contiguous columns)
//   W   [B][m][K]  (gene-major, k contiguous)    H [B][n][K]  (= libnmf column-major k x n)
//   Gp  [chunk][B][K][n_pad]  split-K partials of W^T (A / VP) over fixed gene chunks
// Every sum's order depends only on (m, n, k): fixed gene chunks, fixed tree reductions, never on
// the batch, the group a restart lands in or the GPU count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lane_pool.hpp"
#include "nmfc_host.hpp"
#include "nmfc_tuning.hpp"
#include "rmt.hpp"
#include "../../include/nmfc.h"
#include "nmfc_internal.hpp"

using nmfc_host::DevBuf;
using nmfc_host::errorf;
using nmfc_host::PinBuf;
using nmfc_host::round_up;

namespace {

constexpr int BT = 256;
constexpr int BR_KMAX = 16;
constexpr double EPS = 2.220446049250313e-16;   // .Machine$double.eps

// q = a / p from a refined reciprocal r of p: q = a r and one residual correction (Markstein's final step), i.e. the
// compiler's IEEE sequence without its operand-scaling steps (div_scale / div_fmas / div_fixup), which only matter
// near the exponent limits, and without its second Newton step.  r comes from v_rcp_f64 (good to 2^-24.4 on gfx950)
// and one Newton step (|1 - p r| <= 2^-48.6 measured on the device over the whole admitted domain, batched or not), so
// the corrected quotient's error is ~2^-97 relative before its rounding.  The contract (measured
// by tests/test_gpu_brunet_quot.py through nmfc_brunet_quot_probe, which calls this function):
//  * a = 0 gives +0.0, and for a >= 2^-969 the result is FAITHFUL: the double just below or just above a / p.  It is
//    not correctly rounded: of 131 072 constructed quotients 2^-106 from a rounding midpoint, 5.9 % (one quotient per
//    v_rcp_f64) to 8.1 % (five) come out as the other neighbour.  Random operands get that close with probability
//    below 2^-43: 0 of 3.2e9 random probe pairs (tools/quot_probe.hip) and 0 of 7e6 at the ends of the domain differ
//    from IEEE a / p, and iterations and labels equal the IEEE-divide oracle's on the tested sweeps
//    (tests/test_gpu_brunet.py).
//  * for 0 < a < 2^-969 the last bit of the exact residual, 2^(e_a - 105), is below 2^-1074: fma(-p, q, a) is rounded
//    on the subnormal grid (for subnormal a usually to zero) and the result tends to the uncorrected a r, so only
//    |q - a / p| <= max(2^-43 |a / p|, 2^-1074) is promised (measured: at most 17.3 ulp, and a whole ulp off only for
//    a < 2^-1021).  Such entries do not occur in expression data; no scaling step is spent on them here.
// NMFC_BRUNET_IEEEDIV (a build of tools/build_variant.sh) is the exact IEEE option.
__device__ __forceinline__ double quot_r(double a, double p, double r) {
#if NMFC_BRUNET_IEEEDIV
  (void)r;
  return a / p;
#else
  const double q = a * r;
  return fma(fma(-p, q, a), r, q);
#endif
}

// Refined reciprocals of N positive values from ONE v_rcp_f64 (Montgomery's batch inversion): prefix products
// c_i = p_0 ... p_i, u = 1 / c_{N-1} by v_rcp_f64 and one Newton step, then r_i = u c_{i-1} and u <- u p_i from the top
// down (N = 1: v_rcp_f64 + one Newton step, the round-5 sequence).  v_rcp_f64 issues at about a third of the fp64 FMA
// rate on gfx950 (6.9 vs 2.1 ns per wave instruction per SIMD, tools/quot_probe.hip rate mode,
// profiles/r06/brunet_rcp/), so a batch of N trades N - 1 of them for 3 (N - 1) multiplies.  Each r_i carries the
// Newton error plus at most 2 N roundings of 2^-53, so the corrected quotient keeps its ~2^-96 error and stays faithful
// (0 differences from IEEE a / p in 3.2e9 batched probe quotients; on the device the order of a batch and prefix
// products down to 2^-1020 change nothing, tests/test_gpu_brunet_quot.py).  The prefix products must stay normal: with A
// finite, non-negative and at most 2^64 (checked by nmfc_brunet_create) and caller factors in [2^-60, 2^60] (checked by
// nmfc_brunet_run), every VP of the KL updates lies in [eps^2 / T, T] for T = sum(A) <= 2^100 -- the H update makes the
// column sums of W H equal those of A (the W update the row sums), and the eps terms floor W and H at eps over the
// row / column sums whose products are bounded by T -- so a batch of at most BR_RCP_MAX = 5
// values spans at most 2^(5 (104 + 100)) = 2^1020.
constexpr int BR_RCP_MAX = 5;
template <int N>
__device__ __forceinline__ void recip_batch(const double* p, double* r) {
  static_assert(N >= 1 && N <= BR_RCP_MAX, "batch of 1 .. BR_RCP_MAX reciprocals");
  double c[N];
  c[0] = p[0];
#pragma unroll
  for (int i = 1; i < N; ++i) c[i] = c[i - 1] * p[i];
  double u = __builtin_amdgcn_rcp(c[N - 1]);
  u = fma(u, fma(-c[N - 1], u, 1.0), u);
#pragma unroll
  for (int i = N - 1; i > 0; --i) {
    r[i] = u * c[i - 1];
    u = u * p[i];
  }
  r[0] = u;
}

// reciprocals of NQ values in consecutive batches of at most B
template <int NQ, int B>
__device__ __forceinline__ void recips(const double* p, double* r) {
  constexpr int N = NQ < B ? NQ : B;
  recip_batch<N>(p, r);
  if constexpr (NQ > N) recips<NQ - N, B>(p + N, r + N);
}

// Per-rank configuration of the two VALU kernels (tables in nmfc_tuning.hpp, per kernel since round 6):
//  SPL  elements per lane: the LDS return path moves 8K bytes per lane for every element-restart's operand row; where
//       that (rather than the VALU work) bounds the kernel, each row serves 2 elements (k = 8, 9; elsewhere the doubled
//       register state costs more occupancy than the traffic saves: profiles/r01f_brunet_spl.txt).
//  RG   restarts per workgroup: each lane keeps SPL * RG * 4K values of state; RG shares every A element loaded over RG
//       restarts.  The best RG is not monotone in k: register-count occupancy steps and grid size (groups = R / RG)
//       move together (profiles/r01g/brunet_rg/, profiles/r06/brunet_sload/).  RG never changes a restart's arithmetic.
//  SL   the wave-uniform operand rows by scalar loads into SGPR operands instead of the double-buffered LDS tiles: no
//       LDS return-path bytes and no barriers, and the rows leave the VGPRs (occupancy up a step for k >= 4); the same
//       arithmetic in the same order, so the same bits.
//  RCP  the RG * SPL quotients of a lane's gene (sample) step take their reciprocals in batches of at most RCP from one
//       v_rcp_f64 each (recip_batch); 1: one v_rcp_f64 per quotient.
constexpr int br_nib(unsigned long long t, int K) { return K < 16 ? (int)((t >> (4 * K)) & 15) : 0; }
constexpr int rgh_of(int K) { return br_nib(NMFC_BR_RGH, K) ? br_nib(NMFC_BR_RGH, K) : 1; }
constexpr int rgw_of(int K) { return br_nib(NMFC_BR_RGW, K) ? br_nib(NMFC_BR_RGW, K) : 1; }
constexpr int splh_of(int K) { return ((NMFC_BR_SPLH >> K) & 1ULL) ? 2 : 1; }
constexpr int splw_of(int K) { return ((NMFC_BR_SPLW >> K) & 1ULL) ? 2 : 1; }
constexpr bool slh_of(int K) { return (NMFC_BR_SLH >> K) & 1ULL; }
constexpr bool slw_of(int K) { return (NMFC_BR_SLW >> K) & 1ULL; }
constexpr int rcp_clamp(int b) { return b < 1 ? 1 : (b > BR_RCP_MAX ? BR_RCP_MAX : b); }
constexpr int rcph_of(int K) { return rcp_clamp(br_nib(NMFC_BR_RCPH, K)); }
constexpr int rcpw_of(int K) { return rcp_clamp(br_nib(NMFC_BR_RCPW, K)); }
// small batches (B <= NMFC_BR_SMALL_B restarts of one k, e.g. one rank's shard of a strong-scaling
// run): fewer restarts per workgroup so the batch still spreads over the CUs
constexpr int rg_small(int rg) {
  return NMFC_BR_RG_SMALL_DIV == 0 ? 1 : (rg / NMFC_BR_RG_SMALL_DIV > 1 ? rg / NMFC_BR_RG_SMALL_DIV : 1);
}

// ------------------------------------------------------------------------------------------------
// Kernels
// ------------------------------------------------------------------------------------------------

// set.seed(seeds[b]); W <- matrix(runif(m*K), m, K); H <- matrix(runif(K*n), K, n)  (one workgroup per
// restart; R's Mersenne-Twister from rmt.hpp).
__global__ __launch_bounds__(BT) void k_br_init(const uint32_t* __restrict__ seeds, int m, int n, int K,
                                                double* __restrict__ W, long wstride, double* __restrict__ H,
                                                long hstride) {
  __shared__ uint32_t mt[624];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) rmt::seed_table(mt, seeds[b]);
  __syncthreads();
  const long nw = (long)m * K, total = nw + (long)K * n;
  double* Wb = W + (long)b * wstride;
  double* Hb = H + (long)b * hstride;
  for (long base = 0; base < total; base += 624) {
    rmt::regenerate<BT>(mt);
    for (int t = tid; t < 624; t += BT) {
      const long d = base + t;
      if (d >= total) break;
      const double u = rmt::unif(mt[t]);
      if (d < nw)
        Wb[(d % m) * K + d / m] = u;
      else
        Hb[d - nw] = u;
    }
    __syncthreads();
  }
}

// Tile of the wave-uniform operand (W rows of the H side, H columns of the W side) for the RG
// restarts of a workgroup: TL consecutive gene (sample) rows of K doubles per restart, contiguous in
// HBM, fetched with coalesced vector loads one tile ahead into registers and stored into the other
// half of a double-buffered LDS array; the inner loop reads it back with broadcast LDS reads.
constexpr int TL = NMFC_BR_TL;
// inner-loop unroll per k and kernel (tools/brunet_kbench.py on the C5 shape; unroll 2 where the unrolled live ranges
// push the register count past an occupancy step).  Round 6, re-measured with the per-kernel SL / RG / SPL tables
// against 1 / 2 / 4 / 8 for every k (profiles/r06/brunet_sload/n_*): H side 2 at k = 4 (-5 %), 4 at k = 6 (-8 %), 8 at
// k = 10 (-6.5 %); W side 4 at k = 4 (-4 %), 2 at k = 6; the rest as round 5 (profiles/r05/brunet/kbench_unroll_rg.txt).
constexpr int br_unroll_h(int K) {   // NMFC_BR_UNROLL != 0: one unroll for every k and kernel (experiment builds)
  return NMFC_BR_UNROLL != 0 ? NMFC_BR_UNROLL
                             : K == 10 ? 8 : (K == 4 || K == 5 || K == 7 || K == 8) ? 2 : 4;
}
constexpr int br_unroll_w(int K) {
  return NMFC_BR_UNROLL != 0 ? NMFC_BR_UNROLL : (K == 5 || K == 6 || K == 7 || K == 8 || K == 10) ? 2 : 4;
}

template <int K, int RG>
struct OperandTiles {
  static constexpr int TW = RG * TL * K;              // doubles per tile (all restarts)
  static constexpr int PER = (TW + BT - 1) / BT;      // per thread
  double pre[PER];
  // rows [t0, t0 + TL) of X[slot_r][row][c] (row stride K), rows >= rows_end read as 0
  __device__ __forceinline__ void fetch(const double* __restrict__ X, long stride, const int* sl, int t0,
                                        int rows_end) {
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int idx = threadIdx.x + e * BT;
      double v = 0.0;
      if (idx < TW) {
        const int r = idx / (TL * K), rem = idx - r * (TL * K);
        if (rem < (rows_end - t0) * K) v = X[(long)sl[r] * stride + (long)t0 * K + rem];
      }
      pre[e] = v;
    }
  }
  __device__ __forceinline__ void store(double* lds) {
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int idx = threadIdx.x + e * BT;
      if (idx < TW) lds[idx] = pre[e];
    }
  }
};

// H side, split over fixed gene chunks: Gp[chunk][b][c][j] = sum_{i in chunk} W[b][i][c] * A[i][j] / VP[i][j],
// VP[i][j] = sum_c W[b][i][c] H[b][j][c].  Lane = SPL samples j (H columns and accumulators in
// registers); W rows through the double-buffered LDS tiles.  A broadcast ds_read_b128 still moves
// 1 KiB per wave through the LDS return path, so for larger k each W row read serves SPL = 2 samples.
template <int K, int RG, int SPL, bool SL>
__global__ __launch_bounds__(BT) void k_br_hnum(const double* __restrict__ Arm, long n_pad, int m, int n, int gc,
                                                const int* __restrict__ act, int nact, const double* __restrict__ W,
                                                long wstride, const double* __restrict__ H, long hstride,
                                                double* __restrict__ Gp, long gp_cs) {
  using OT = OperandTiles<K, RG>;
  __shared__ double wl[2][OT::TW];
  __shared__ int sl[RG];
  int jj[SPL], jl[SPL];
#pragma unroll
  for (int s = 0; s < SPL; ++s) {
    jj[s] = blockIdx.x * (BT * SPL) + s * BT + threadIdx.x;
    jl[s] = jj[s] < n ? jj[s] : n - 1;
  }
  const int chunk = blockIdx.y;
  const int g0 = blockIdx.z * RG;
  const int nlive = min(RG, nact - g0);
  const int i0 = chunk * gc, i1 = min(m, i0 + gc);
  if (threadIdx.x < RG) sl[threadIdx.x] = act[min(g0 + (int)threadIdx.x, nact - 1)];
  __syncthreads();
  long wro[RG];   // SL: each restart's W row base, wave-uniform
#pragma unroll
  for (int r = 0; r < RG; ++r) wro[r] = (long)__builtin_amdgcn_readfirstlane(sl[r]) * wstride;
  double h[SPL][RG][K], g[SPL][RG][K];
#pragma unroll
  for (int s = 0; s < SPL; ++s)
#pragma unroll
    for (int r = 0; r < RG; ++r)
#pragma unroll
      for (int c = 0; c < K; ++c) {
        h[s][r][c] = H[(long)sl[r] * hstride + (long)jl[s] * K + c];
        g[s][r][c] = 0.0;
      }
  OT ot;
  if constexpr (!SL) {
    ot.fetch(W, wstride, sl, i0, i1);
    ot.store(wl[0]);
    __syncthreads();
  }
  int buf = 0;
  for (int t0 = i0; t0 < i1; t0 += TL, buf ^= 1) {
    const bool more = !SL && t0 + TL < i1;
    if (more) ot.fetch(W, wstride, sl, t0 + TL, i1);
    const double* ap = Arm + (long)t0 * n_pad;
    const double* wt = wl[buf];
    const double* wg = W + (long)t0 * K;
    // one gene: every quotient's VP first, their reciprocals in batches of rcph_of(K) (recips), then the accumulations
    // (each accumulator still adds its genes in gene order).  Slots past the live restarts repeat the last live one
    // (computed, never stored): no branches here
    auto gene = [&](int ii) {
      constexpr int NQ = RG * SPL;
      double a[SPL], w[RG][K], p[NQ], rr[NQ];
#pragma unroll
      for (int s = 0; s < SPL; ++s) a[s] = ap[(long)ii * n_pad + jl[s]];
#pragma unroll
      for (int r = 0; r < RG; ++r) {
        const double* wr = SL ? wg + wro[r] + ii * K : wt + r * (TL * K) + ii * K;
#pragma unroll
        for (int c = 0; c < K; ++c) w[r][c] = wr[c];
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
          double v = 0.0;
#pragma unroll
          for (int c = 0; c < K; ++c) v = fma(w[r][c], h[s][r][c], v);
          p[r * SPL + s] = v;
        }
      }
      recips<NQ, rcph_of(K)>(p, rr);
#pragma unroll
      for (int r = 0; r < RG; ++r)
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
          const double q = quot_r(a[s], p[r * SPL + s], rr[r * SPL + s]);
#pragma unroll
          for (int c = 0; c < K; ++c) g[s][r][c] = fma(w[r][c], q, g[s][r][c]);
        }
    };
    if (i1 - t0 >= TL) {
#pragma unroll br_unroll_h(K)
      for (int ii = 0; ii < TL; ++ii) gene(ii);
    } else {
      for (int ii = 0; ii < i1 - t0; ++ii) gene(ii);
    }
    if constexpr (!SL) {
      if (more) ot.store(wl[buf ^ 1]);
      __syncthreads();
    }
  }
#pragma unroll
  for (int s = 0; s < SPL; ++s)
    if (jj[s] < n) {
#pragma unroll
      for (int r = 0; r < RG; ++r)
        if (r < nlive) {
#pragma unroll
          for (int c = 0; c < K; ++c) Gp[(long)chunk * gp_cs + ((long)sl[r] * K + c) * n_pad + jj[s]] = g[s][r][c];
        }
    }
}

// The workgroup sum of v[c] in the fixed tree order red[t] += red[t + s], s = BT/2, ..., 1: the strides of 64 and
// more through LDS, the last six inside wave 0 by lane shuffles (lane t adds lane t + s's value of the previous
// step, exactly the LDS tree's operands), so 3 barriers instead of 9 and the same bits.
template <int K>
__device__ __forceinline__ void tree_sum(double (*red)[BT], double* v) {
  static_assert(BT == 256, "tree_sum: two LDS steps then one wave");
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < K; ++c) red[c][tid] = v[c];
  __syncthreads();
  if (tid < 128) {
#pragma unroll
    for (int c = 0; c < K; ++c) red[c][tid] += red[c][tid + 128];
  }
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int c = 0; c < K; ++c) {
      double x = red[c][tid] + red[c][tid + 64];
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) x = x + __shfl_down(x, s);
      if (tid == 0) red[c][0] = x;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < K; ++c) v[c] = red[c][0];
  __syncthreads();
}

// One workgroup per live restart: colSums(W) (apply(W, 2, sum)), sum of the chunk partials,
// H <- (H * G + eps) / colSums(W), rowSums(new H) for the W side, and on check iterations the
// membership test (order(H[,j], decreasing = TRUE)[1] vs the previous check).
template <int K>
__global__ __launch_bounds__(BT) void k_br_hupd(int t, int check, int stopconv, int nchunks, int m, int n, long n_pad,
                                                const int* __restrict__ act, const double* __restrict__ W, long wstride,
                                                double* __restrict__ H, long hstride, const double* __restrict__ Gp,
                                                long gp_cs, double* __restrict__ RS, int* __restrict__ memb,
                                                int* __restrict__ nochange, int* __restrict__ stop_iter) {
  __shared__ double red[K][BT];
  const int b = act[blockIdx.x], tid = threadIdx.x;
  double cs[K];
#pragma unroll
  for (int c = 0; c < K; ++c) cs[c] = 0.0;
  const double* Wb = W + (long)b * wstride;
  // this thread's rows i = tid, tid + BT, ... in order, U rows' loads issued ahead of their adds
  constexpr int U = K <= 8 ? 4 : 2;
  int i = tid;
  for (; i + (U - 1) * BT < m; i += U * BT) {
    double v[U][K];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < K; ++c) v[u][c] = Wb[(long)(i + u * BT) * K + c];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < K; ++c) cs[c] += v[u][c];
  }
  for (; i < m; i += BT) {
#pragma unroll
    for (int c = 0; c < K; ++c) cs[c] += Wb[(long)i * K + c];
  }
  tree_sum<K>(red, cs);
  double rs[K];
#pragma unroll
  for (int c = 0; c < K; ++c) rs[c] = 0.0;
  int changed = 0;
  double* Hb = H + (long)b * hstride;
  for (int j = tid; j < n; j += BT) {
    double hv[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const double* gp = Gp + ((long)b * K + c) * n_pad + j;
      double g = 0.0;   // the chunk partials in chunk order, eight chunks' loads in flight
      for (int ch0 = 0; ch0 < nchunks; ch0 += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ch0 + u < nchunks ? gp[(long)(ch0 + u) * gp_cs] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (ch0 + u < nchunks) g += v[u];
      }
      hv[c] = __dadd_rn(__dmul_rn(Hb[(long)j * K + c], g), EPS) / cs[c];
      Hb[(long)j * K + c] = hv[c];
      rs[c] += hv[c];
    }
    if (check) {
      int best = 0;
#pragma unroll
      for (int c = 1; c < K; ++c)
        if (hv[c] > hv[best]) best = c;
      const int mm = best + 1;
      if (mm != memb[(long)b * n + j]) changed = 1;
      memb[(long)b * n + j] = mm;
    }
  }
  tree_sum<K>(red, rs);
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < K; ++c) RS[(long)b * K + c] = rs[c];
  }
  if (check) {
    const int any = __syncthreads_or(changed);
    if (tid == 0) {
      const int nc = any ? 0 : nochange[b] + 1;
      nochange[b] = nc;
      if (nc == stopconv) stop_iter[b] = t;
    }
  }
}

// W side: lane = SPL genes i over every sample j: F[i][c] = sum_j A[i][j] / VP[i][j] * H[j][c] with the
// new H (LDS tiles of TL samples) and the old W rows in registers; W <- (W * F + eps) / rowSums(H).
template <int K, int RG, int SPL, bool SL>
__global__ __launch_bounds__(BT) void k_br_wupd(const double* __restrict__ Acm, long m_pad, int m, int n,
                                                const int* __restrict__ act, int nact, double* __restrict__ W,
                                                long wstride, const double* __restrict__ H, long hstride,
                                                const double* __restrict__ RS) {
  using OT = OperandTiles<K, RG>;
  __shared__ double hl[2][OT::TW];
  __shared__ int sl[RG];
  int ig[SPL], il[SPL];
#pragma unroll
  for (int s = 0; s < SPL; ++s) {
    ig[s] = blockIdx.x * (BT * SPL) + s * BT + threadIdx.x;
    il[s] = ig[s] < m ? ig[s] : m - 1;
  }
  const int g0 = blockIdx.y * RG;
  const int nlive = min(RG, nact - g0);
  if (threadIdx.x < RG) sl[threadIdx.x] = act[min(g0 + (int)threadIdx.x, nact - 1)];
  __syncthreads();
  long hro[RG];   // SL: each restart's H row base, wave-uniform
#pragma unroll
  for (int r = 0; r < RG; ++r) hro[r] = (long)__builtin_amdgcn_readfirstlane(sl[r]) * hstride;
  double w[SPL][RG][K], f[SPL][RG][K];
#pragma unroll
  for (int s = 0; s < SPL; ++s)
#pragma unroll
    for (int r = 0; r < RG; ++r)
#pragma unroll
      for (int c = 0; c < K; ++c) {
        w[s][r][c] = W[(long)sl[r] * wstride + (long)il[s] * K + c];
        f[s][r][c] = 0.0;
      }
  OT ot;
  if constexpr (!SL) {
    ot.fetch(H, hstride, sl, 0, n);
    ot.store(hl[0]);
    __syncthreads();
  }
  int buf = 0;
  for (int s0 = 0; s0 < n; s0 += TL, buf ^= 1) {
    const bool more = !SL && s0 + TL < n;
    if (more) ot.fetch(H, hstride, sl, s0 + TL, n);
    const double* ap = Acm + (long)s0 * m_pad;
    const double* ht = hl[buf];
    const double* hg = H + (long)s0 * K;
    // one sample, as the H side's gene(): VPs, batched reciprocals, accumulations
    auto sample = [&](int jj) {
      constexpr int NQ = RG * SPL;
      double a[SPL], hh[RG][K], p[NQ], rr[NQ];
#pragma unroll
      for (int s = 0; s < SPL; ++s) a[s] = ap[(long)jj * m_pad + il[s]];
#pragma unroll
      for (int r = 0; r < RG; ++r) {
        const double* hj = SL ? hg + hro[r] + jj * K : ht + r * (TL * K) + jj * K;
#pragma unroll
        for (int c = 0; c < K; ++c) hh[r][c] = hj[c];
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
          double v = 0.0;
#pragma unroll
          for (int c = 0; c < K; ++c) v = fma(w[s][r][c], hh[r][c], v);
          p[r * SPL + s] = v;
        }
      }
      recips<NQ, rcpw_of(K)>(p, rr);
#pragma unroll
      for (int r = 0; r < RG; ++r)
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
          const double q = quot_r(a[s], p[r * SPL + s], rr[r * SPL + s]);
#pragma unroll
          for (int c = 0; c < K; ++c) f[s][r][c] = fma(q, hh[r][c], f[s][r][c]);
        }
    };
    if (n - s0 >= TL) {
#pragma unroll br_unroll_w(K)
      for (int jj = 0; jj < TL; ++jj) sample(jj);
    } else {
      for (int jj = 0; jj < n - s0; ++jj) sample(jj);
    }
    if constexpr (!SL) {
      if (more) ot.store(hl[buf ^ 1]);
      __syncthreads();
    }
  }
#pragma unroll
  for (int s = 0; s < SPL; ++s)
    if (ig[s] < m) {
#pragma unroll
      for (int r = 0; r < RG; ++r)
        if (r < nlive) {
#pragma unroll
          for (int c = 0; c < K; ++c)
            W[(long)sl[r] * wstride + (long)ig[s] * K + c] =
                __dadd_rn(__dmul_rn(w[s][r][c], f[s][r][c]), EPS) / RS[(long)sl[r] * K + c];
        }
    }
}

// labels[b][j] = order(H[,j], decreasing = TRUE)[1] (first row of the column maximum, 1-based)
__global__ __launch_bounds__(BT) void k_br_labels(const double* __restrict__ H, long hstride, int K, int n,
                                                  int32_t* __restrict__ labels) {
  const int b = blockIdx.y, j = blockIdx.x * BT + threadIdx.x;
  if (j >= n) return;
  const double* h = H + (long)b * hstride + (long)j * K;
  int best = 0;
  for (int c = 1; c < K; ++c)
    if (h[c] > h[best]) best = c;
  labels[(long)b * n + j] = best + 1;
}

// connect.matrix[i][j] = sum_b [labels_b(i) == labels_b(j)]   (exact integers)
__global__ __launch_bounds__(BT) void k_br_counts(const int32_t* __restrict__ labels, int B, int n,
                                                  int32_t* __restrict__ counts) {
  const int i = blockIdx.x * 16 + (threadIdx.x & 15);
  const int j = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= n || j >= n) return;
  int32_t cnt = 0;
  for (int b = 0; b < B; ++b) cnt += labels[(long)b * n + i] == labels[(long)b * n + j];
  counts[(long)j * n + i] = cnt;
}

__global__ void k_br_divide(const int32_t* __restrict__ counts, double denom, long len, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < len) out[i] = (double)counts[i] / denom;
}

// ... and the domain check of recip_batch: *bad = 1 (a plain store; every writer stores the same value) when an entry
// is not a finite number in [0, 2^64]
__global__ void k_br_layout(const double* __restrict__ A, int m, int n, long m_pad, long n_pad,
                            double* __restrict__ Acm, double* __restrict__ Arm, int* __restrict__ bad) {
  const int i = blockIdx.x * BT + threadIdx.x, j = blockIdx.y;
  if (i >= m) return;
  const double v = A[(long)j * m + i];
  Acm[(long)j * m_pad + i] = v;
  Arm[(long)i * n_pad + j] = v;
  if (!(v >= 0.0 && v <= 0x1p64)) *bad = 1;   // NaN fails both tests
}

// ---- KL divergence of a batch's final factors (nmfc_brunet_set_divergence) -------------------------------
// D_b = sum_{i,j} (a log((a + eps) / (p + eps)) - a + p) / (m n), p = sum_q W_b[i][q] H_b[j][q]: NMF.div's error.v figure
// (oracle/brunet_oracle.c) on the factors the run returns.  A tile is DIV_GT genes (one per lane) by DIV_ST samples
// (DIV_WJ per wave): a thread keeps its DIV_WJ values of A in registers and walks all B restarts of the batch over them,
// so A is read once per batch.  Per restart it holds its row of W (K contiguous doubles) in registers; the restart's H
// columns are wave-uniform.  The tiling and every summation order are functions of (m, n) alone.
constexpr int DIV_GT = 64;
constexpr int DIV_WJ = 8;
constexpr int DIV_ST = (BT / 64) * DIV_WJ;
static_assert(BT / 64 == 4, "k_br_div adds four wave sums");
constexpr int DIV_JG = 16;   // restarts between two workgroup barriers (the LDS rows of the wave sums)
// VALU instructions of the device log() as hipcc compiles it for gfx950 (counted in the ISA listing: 83 from
// v_frexp_mant_f64 to the last special-case select, its literal moves left out; one sample's stretch of k_br_div<2>
// holds 102 = 83 + 2 FMAs + 17 for the two eps adds, the IEEE division, a log r - a + p, the select and the running
// sum).  Kernel id 3 of nmfc_brunet_kernel_time is priced at 2k + 6 + BR_LOG_OPS lane-operations per element.
constexpr int BR_LOG_OPS = 83;

// one element's term from the oracle's expression, one rounding per operation, the quotient an IEEE division; a = 0
// gives exactly p
__device__ __forceinline__ double div_term(double a, double p) {
  const double lg = log(__ddiv_rn(__dadd_rn(a, EPS), __dadd_rn(p, EPS)));
  return __dadd_rn(__dsub_rn(__dmul_rn(a, lg), a), p);
}

// grid x: tiles, gene tile major with nst sample tiles each.  part[b][tile] = the tile's sum for restart b: a thread adds
// its samples in order, the wave by the xor butterfly (every lane ends with the same bits), the four waves in wave order.
// Needs n >= DIV_WJ (narrower matrices: k_br_div_narrow).  A wave whose DIV_WJ samples would pass n starts at
// n - DIV_WJ instead and drops the samples below its own first one by a select, so its reads sit at constant offsets
// inside Acm and the restart's own H.  Rows >= m read row m - 1 of W and are dropped by the same select.
template <int K>
__global__ __launch_bounds__(BT) void k_br_div(const double* __restrict__ Acm, long m_pad, int m, int n, int nst, int B,
                                               const double* __restrict__ W, long wstride,
                                               const double* __restrict__ H, long hstride, double* __restrict__ part,
                                               int ntiles) {
  __shared__ double red[DIV_JG][BT / 64];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int tile = blockIdx.x, gt = tile / nst, stl = tile - gt * nst;
  const int i = gt * DIV_GT + lane;            // < m_pad (a multiple of BT): every Acm read stays inside its column
  const int il = i < m ? i : m - 1;
  const int j0 = stl * DIV_ST + wave * DIV_WJ; // the wave's first sample
  const int jb = min(j0, n - DIV_WJ);          // the first sample read: 0 <= jb, jb + DIV_WJ <= n
  const int skip = i < m ? j0 - jb : DIV_WJ;   // samples u < skip are not this thread's: all of them when j0 >= n
  double av[DIV_WJ];
#pragma unroll
  for (int u = 0; u < DIV_WJ; ++u) av[u] = Acm[(long)(jb + u) * m_pad + i];
  const double* wr = W + (long)il * K;   // this thread's row of W and the wave's first column of H, restart 0
  const double* hj = H + (long)jb * K;
  double* po = part + (long)threadIdx.x * ntiles + tile;   // thread t stores restart t's sum of each round of DIV_JG
#pragma unroll 1
  for (int b = 0; b < B; ++b, wr += wstride, hj += hstride) {
    double w[K];
#pragma unroll
    for (int q = 0; q < K; ++q) w[q] = wr[q];
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < DIV_WJ; ++u) {
      double p = 0.0;
#pragma unroll
      for (int q = 0; q < K; ++q) {
        p = fma(w[q], hj[u * K + q], p);
        // a long H column is consumed four entries at a time in the schedule (two or one where the column is no
        // multiple of 32 bytes): the counts at which no scalar register is spilled, as the barrier per sample below
        constexpr int QM = K == 15 ? 0 : (K & 3) ? 1 : 3;
        if (K >= 12 && (q & QM) == QM) __builtin_amdgcn_sched_barrier(0);
      }
      const double t = div_term(av[u], p);
      s = __dadd_rn(s, u >= skip ? t : 0.0);
      // one sample at a time in the schedule: with several H columns hoisted the scalar registers spill
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const int r = b & (DIV_JG - 1);
    if (lane == 0) red[r][wave] = s;
    if (r == DIV_JG - 1 || b == B - 1) {   // the wave sums of the last r + 1 restarts, in wave order
      __syncthreads();
      if ((int)threadIdx.x <= r) {
        const double* p = red[threadIdx.x];
        *po = ((p[0] + p[1]) + p[2]) + p[3];
      }
      __syncthreads();
      po += (long)DIV_JG * ntiles;
    }
  }
}

// n < DIV_WJ (one sample tile, all of it wave 0's): the same sums in the same order by rolled loops, any K.  One wave
// per gene tile and restart; part[b][tile] as k_br_div writes it (the other three wave sums are 0).
__global__ __launch_bounds__(64) void k_br_div_narrow(const double* __restrict__ Acm, long m_pad, int m, int n, int K,
                                                      const double* __restrict__ W, long wstride,
                                                      const double* __restrict__ H, long hstride,
                                                      double* __restrict__ part, int ntiles) {
  const int tile = blockIdx.x, b = blockIdx.y;
  const int i = tile * DIV_GT + threadIdx.x, il = i < m ? i : m - 1;
  const double* wr = W + (long)b * wstride + (long)il * K;
  const double* hb = H + (long)b * hstride;
  double s = 0.0;
  for (int u = 0; u < n; ++u) {
    double p = 0.0;
    for (int q = 0; q < K; ++q) p = fma(wr[q], hb[u * K + q], p);
    const double t = div_term(Acm[(long)u * m_pad + i], p);
    s = __dadd_rn(s, i < m ? t : 0.0);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) part[(long)b * ntiles + tile] = ((s + 0.0) + 0.0) + 0.0;
}

// div[b] = (restart b's ntiles partials: lane l adds tiles l, l + 64, ... in order, then the butterfly) / (m n)
__global__ __launch_bounds__(64) void k_br_div_sum(const double* __restrict__ part, int ntiles, double mn,
                                                   double* __restrict__ div) {
  const double* p = part + (long)blockIdx.x * ntiles;
  double s = 0.0;
  for (int t = threadIdx.x; t < ntiles; t += 64) s += p[t];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) div[blockIdx.x] = s / mn;
}

// y[i] = log(x[i]) by the device log that k_br_div calls (nmfc_brunet_log_probe: the tests measure it against logl)
__global__ void k_br_log(const double* __restrict__ x, int len, double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < len) y[i] = log(x[i]);
}

// One batch of N quotients per thread by the hot loops' own recip_batch<N> and quot_r (nmfc_brunet_quot_probe: the
// tests measure them at the ends of the reciprocals' domain).  Thread j handles pairs j N .. j N + N - 1.
template <int N>
__global__ void k_br_quot(const double* __restrict__ a, const double* __restrict__ p, int nb, double* __restrict__ q,
                          double* __restrict__ r) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nb) return;
  double pp[N], rr[N];
#pragma unroll
  for (int i = 0; i < N; ++i) pp[i] = p[j * N + i];
  recip_batch<N>(pp, rr);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    q[j * N + i] = quot_r(a[j * N + i], pp[i], rr[i]);
    r[j * N + i] = rr[i];
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Host side.  Each k is one batch of B restarts run by a "lane" (own HIP stream and buffers); up to
// BR_LANES lanes run concurrently from a small host thread pool, largest k first, so that the small
// grids of a batch's last stragglers overlap with the other ranks' batches instead of idling the chip.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int BR_LANES = 4;   // = the HW queues HIP gives a process by default (GPU_MAX_HW_QUEUES)
enum { BK_HNUM = 0, BK_HUPD = 1, BK_WUPD = 2, BK_DIV = 3, BK_N = 4 };

struct BrLane {
  hipStream_t st = nullptr;
  DevBuf W, H, Gp, RS, memb, nochange, stop_iter, act, seeds, labels;
  DevBuf part, div;                 // divergence pass: per (restart, tile) partials, per restart D (only when enabled)
  // pinned host mirrors of stop_iter, act, seeds: the small per-iteration copies of four lanes never go through HIP's
  // shared pageable staging path
  PinBuf h_si, h_act, h_seeds;
  PinBuf h_div;                  // ... and of div
  bool timing = false;
  nmfc_host::LaunchTimer timer;
  double kms[BK_N] = {0, 0, 0, 0};
  long long kcount[BK_N] = {0, 0, 0, 0};
  double kfl_sum[BK_N] = {0, 0, 0, 0};
};

void br_drain(BrLane* L) {
  L->timer.drain([L](int kid, float ms) { L->kms[kid] += ms; });
}

// counts the launch and its flops; HIP events on the lane's stream around it only when timing is enabled
struct BTimed {
  nmfc_host::TimedScope scope;
  BTimed(BrLane* L, int kid, double flops) : scope(L->timer, L->st, kid, L->timing) {
    L->kcount[kid] += 1;
    L->kfl_sum[kid] += flops;
  }
};

}  // namespace

struct nmfc_brunet {
  int dev = 0;
  hipStream_t st = nullptr;
  int m = 0, n = 0;
  long m_pad = 0, n_pad = 0;
  int gc = 0, nchunks = 0;
  int nlanes = BR_LANES;
  DevBuf Acm, Arm, counts_tmp, cons_tmp;
  BrLane lanes[BR_LANES];
  bool timing = false;
  double kms[BK_N] = {0, 0, 0, 0};
  long long kcount[BK_N] = {0, 0, 0, 0};
  double kfl_sum[BK_N] = {0, 0, 0, 0};
  // nmfc_brunet_set_divergence: the last run's D per job and, per k index, the best restart and its factors (device,
  // in the lane layouts W [gene][K], H [sample][K]); a lane writes only the entries of its own k
  bool divergence = false, div_valid = false;
  int div_B = 0, div_rb = 0;
  std::vector<int> div_ks, best_slot;
  std::vector<double> div_vals;
  std::vector<DevBuf> bestW, bestH;
};

namespace {

// one k: B restarts (slots 0..B-1) already initialised in L->W / L->H; iterates to the stop rule.
template <int K, int RGH = rgh_of(K), int RGW = rgw_of(K)>
int br_iterate(const nmfc_brunet* e, BrLane* L, int B, const nmfc_brunet_opts& o, std::vector<int>& iters,
               std::vector<int>& stopped) {
  constexpr int SPLH = splh_of(K), SPLW = splw_of(K);
  const int m = e->m, n = e->n;
  hipStream_t st = L->st;
  const long wstride = (long)m * K, hstride = (long)n * K;
  const long gp_cs = (long)B * K * e->n_pad;
  int* act = L->h_act.as<int>();   // pinned (br_run_k sized them): host list of live restart slots
  int* si = L->h_si.as<int>();     // pinned read-back of stop_iter
  for (int b = 0; b < B; ++b) act[b] = b, si[b] = 0;
  int nact = B;
  HIPCHK(hipMemcpyAsync(L->act.p, act, sizeof(int) * B, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(L->memb.p, 0, sizeof(int) * (size_t)B * n, st));   // old.membership starts at 0
  HIPCHK(hipMemsetAsync(L->nochange.p, 0, sizeof(int) * B, st));
  HIPCHK(hipMemsetAsync(L->stop_iter.p, 0, sizeof(int) * B, st));
  const double fl = 4.0 * m * n * K;   // algorithmic flop per restart and kernel: VP (2mnk) + product (2mnk)
  for (int t = 1; t <= o.maxiter && nact > 0; ++t) {
    const int check = (t % o.stopfreq) == 0;
    const int groups_h = (nact + RGH - 1) / RGH, groups_w = (nact + RGW - 1) / RGW;
    {
      BTimed tl(L, BK_HNUM, fl * nact);
      hipLaunchKernelGGL((k_br_hnum<K, RGH, SPLH, slh_of(K)>), dim3((n + BT * SPLH - 1) / (BT * SPLH), e->nchunks, groups_h),
                         dim3(BT), 0, st,
                         e->Arm.as<double>(), e->n_pad, m, n, e->gc, L->act.as<int>(), nact, L->W.as<double>(), wstride,
                         L->H.as<double>(), hstride, L->Gp.as<double>(), gp_cs);
    }
    {
      BTimed tl(L, BK_HUPD, 0.0);
      hipLaunchKernelGGL((k_br_hupd<K>), dim3(nact), dim3(BT), 0, st, t, check, o.stopconv, e->nchunks, m, n, e->n_pad,
                         L->act.as<int>(), L->W.as<double>(), wstride, L->H.as<double>(), hstride, L->Gp.as<double>(),
                         gp_cs, L->RS.as<double>(), L->memb.as<int>(), L->nochange.as<int>(), L->stop_iter.as<int>());
    }
    {
      BTimed tl(L, BK_WUPD, fl * nact);
      hipLaunchKernelGGL((k_br_wupd<K, RGW, SPLW, slw_of(K)>), dim3((m + BT * SPLW - 1) / (BT * SPLW), groups_w), dim3(BT), 0, st,
                         e->Acm.as<double>(),
                         e->m_pad, m, n, L->act.as<int>(), nact, L->W.as<double>(), wstride, L->H.as<double>(), hstride,
                         L->RS.as<double>());
    }
    HIPCHK(hipGetLastError());
    if (check) {
      // stops happen only on check iterations, after that iteration's W update (NMF.div breaks at the
      // end of the iteration): drop stopped restarts from the launch list
      HIPCHK(hipMemcpyAsync(si, L->stop_iter.p, sizeof(int) * B, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (L->timing) br_drain(L);
      int q = 0;
      for (int x = 0; x < nact; ++x)
        if (si[act[x]] == 0) act[q++] = act[x];
      if (q != nact) {
        nact = q;
        if (nact > 0) HIPCHK(hipMemcpyAsync(L->act.p, act, sizeof(int) * nact, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
      }
    }
  }
  HIPCHK(hipMemcpyAsync(si, L->stop_iter.p, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (L->timing) br_drain(L);
  iters.resize(B);
  stopped.resize(B);
  for (int b = 0; b < B; ++b) {
    iters[b] = si[b] ? si[b] : o.maxiter;   // NMF.div returns t: the break iteration, else maxniter
    stopped[b] = si[b] != 0;
  }
  return 0;
}

int br_dispatch(const nmfc_brunet* e, BrLane* L, int K, int B, const nmfc_brunet_opts& o, std::vector<int>& iters,
                std::vector<int>& stopped) {
  switch (K) {
#define BR_CASE(KK) \
  case KK:          \
    return B <= NMFC_BR_SMALL_B ? br_iterate<KK, rg_small(rgh_of(KK)), rg_small(rgw_of(KK))>(e, L, B, o, iters, stopped) \
                                : br_iterate<KK>(e, L, B, o, iters, stopped);
    BR_CASE(2) BR_CASE(3) BR_CASE(4) BR_CASE(5) BR_CASE(6) BR_CASE(7) BR_CASE(8) BR_CASE(9) BR_CASE(10) BR_CASE(11)
    BR_CASE(12) BR_CASE(13) BR_CASE(14) BR_CASE(15) BR_CASE(16)
#undef BR_CASE
    default:
      errorf("nmfc_brunet_run: k=%d unsupported", K);
      return -1;
  }
}

// Everything for one k on one lane: init, iterations, labels, counts slice, host outputs.
struct KJob {
  int ki, K;
  long woff, hoff;   // offsets of this k's jobs in the W / H outputs
};

// D of the B restarts whose final factors lie in L->W / L->H (one pass: k_br_div + k_br_div_sum), the first argmin on
// the host, and that restart's factors copied to the k's own device buffer before the lane reuses W and H.
int br_divergence(nmfc_brunet* e, BrLane* L, const KJob& kj, int B) {
  const int m = e->m, n = e->n, K = kj.K;
  hipStream_t st = L->st;
  const int nst = (n + DIV_ST - 1) / DIV_ST, ntiles = (m + DIV_GT - 1) / DIV_GT * nst;
  const size_t wbytes = sizeof(double) * (size_t)m * K, hbytes = sizeof(double) * (size_t)n * K;
  if (L->part.ensure(sizeof(double) * (size_t)B * ntiles) || L->div.ensure(sizeof(double) * B) ||
      L->h_div.ensure(sizeof(double) * B) || e->bestW[kj.ki].ensure(wbytes) || e->bestH[kj.ki].ensure(hbytes))
    return -1;
  {
    BTimed tl(L, BK_DIV, (2.0 * K + 6 + BR_LOG_OPS) * m * n * B);
    if (n < DIV_WJ)
      hipLaunchKernelGGL(k_br_div_narrow, dim3(ntiles, B), dim3(64), 0, st, e->Acm.as<double>(), e->m_pad, m, n, K,
                         L->W.as<double>(), (long)m * K, L->H.as<double>(), (long)n * K, L->part.as<double>(), ntiles);
    else switch (K) {
#define BR_DIV_CASE(KK)                                                                                             \
  case KK:                                                                                                           \
    hipLaunchKernelGGL((k_br_div<KK>), dim3(ntiles), dim3(BT), 0, st, e->Acm.as<double>(), e->m_pad, m, n, nst, B,   \
                       L->W.as<double>(), (long)m * KK, L->H.as<double>(), (long)n * KK, L->part.as<double>(), ntiles); \
    break;
      BR_DIV_CASE(2) BR_DIV_CASE(3) BR_DIV_CASE(4) BR_DIV_CASE(5) BR_DIV_CASE(6) BR_DIV_CASE(7) BR_DIV_CASE(8)
      BR_DIV_CASE(9) BR_DIV_CASE(10) BR_DIV_CASE(11) BR_DIV_CASE(12) BR_DIV_CASE(13) BR_DIV_CASE(14) BR_DIV_CASE(15)
      BR_DIV_CASE(16)
#undef BR_DIV_CASE
      default:
        errorf("nmfc_brunet_run: k=%d unsupported", K);
        return -1;
    }
    hipLaunchKernelGGL(k_br_div_sum, dim3(B), dim3(64), 0, st, L->part.as<double>(), ntiles, (double)m * n,
                       L->div.as<double>());
  }
  HIPCHK(hipGetLastError());
  double* d = L->h_div.as<double>();
  HIPCHK(hipMemcpyAsync(d, L->div.p, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (L->timing) br_drain(L);
  int best = 0;
  for (int b = 0; b < B; ++b) {
    e->div_vals[(size_t)kj.ki * B + b] = d[b];
    if (d[b] < d[best]) best = b;   // the lowest restart on ties
  }
  e->best_slot[kj.ki] = best;
  HIPCHK(hipMemcpyAsync(e->bestW[kj.ki].p, L->W.as<double>() + (size_t)best * m * K, wbytes, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(e->bestH[kj.ki].p, L->H.as<double>() + (size_t)best * n * K, hbytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

int br_run_k(nmfc_brunet* e, BrLane* L, const KJob& kj, int B, int R, const nmfc_brunet_opts& o, const double* W_init,
             const double* H_init, int32_t* dcounts, nmfc_result* out, long long* tot_iters, int* max_it) {
  const int m = e->m, n = e->n, K = kj.K, ki = kj.ki;
  HIPCHK(hipSetDevice(e->dev));
  if (!L->st) HIPCHK(hipStreamCreateWithFlags(&L->st, hipStreamNonBlocking));
  hipStream_t st = L->st;
  if (L->W.ensure(sizeof(double) * (size_t)B * m * K) || L->H.ensure(sizeof(double) * (size_t)B * n * K) ||
      L->Gp.ensure(sizeof(double) * (size_t)e->nchunks * B * K * e->n_pad) ||
      L->RS.ensure(sizeof(double) * (size_t)B * K) || L->memb.ensure(sizeof(int) * (size_t)B * n) ||
      L->nochange.ensure(sizeof(int) * B) || L->stop_iter.ensure(sizeof(int) * B) || L->act.ensure(sizeof(int) * B) ||
      L->seeds.ensure(sizeof(uint32_t) * B) || L->labels.ensure(sizeof(int32_t) * (size_t)B * n) ||
      L->h_si.ensure(sizeof(int) * B) || L->h_act.ensure(sizeof(int) * B) || L->h_seeds.ensure(sizeof(uint32_t) * B))
    return -1;
  const long wstride = (long)m * K, hstride = (long)n * K;
  std::vector<double> hw, hh;
  uint32_t* seeds = L->h_seeds.as<uint32_t>();
  const int rb = std::max(0, o.restart_begin);
  for (int b = 0; b < B; ++b) seeds[b] = o.seed + (uint32_t)(rb + b + 1);   // set.seed(rseed + i), i 1-based
  HIPCHK(hipMemcpyAsync(L->seeds.p, seeds, sizeof(uint32_t) * B, hipMemcpyHostToDevice, st));
  if (W_init && H_init) {
    // caller factors for this k's B jobs: W_b m x K column-major, H_b K x n column-major; positive and within
    // [2^-60, 2^60] (the batched reciprocals' domain, recip_batch)
    const size_t nwk = (size_t)B * m * K, nhk = (size_t)B * n * K;
    for (size_t x = 0; x < nwk + nhk; ++x) {
      const double v = x < nwk ? W_init[kj.woff + x] : H_init[kj.hoff + (x - nwk)];
      if (!(v >= 0x1p-60 && v <= 0x1p60)) {
        errorf("nmfc_brunet_run: caller factors must lie in [2^-60, 2^60] (k=%d: %g)", K, v);
        return -1;
      }
    }
    hw.assign((size_t)B * m * K, 0.0);
    for (int b = 0; b < B; ++b)
      for (int c = 0; c < K; ++c)
        for (int i = 0; i < m; ++i)
          hw[(size_t)b * wstride + (size_t)i * K + c] = W_init[kj.woff + (long)b * wstride + (long)c * m + i];
    HIPCHK(hipMemcpyAsync(L->W.p, hw.data(), sizeof(double) * hw.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L->H.p, H_init + kj.hoff, sizeof(double) * (size_t)B * hstride, hipMemcpyHostToDevice, st));
  } else {
    hipLaunchKernelGGL(k_br_init, dim3(B), dim3(BT), 0, st, L->seeds.as<uint32_t>(), m, n, K, L->W.as<double>(), wstride,
                       L->H.as<double>(), hstride);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));   // seeds / hw host buffers
  std::vector<int> iters, stopped;
  if (br_dispatch(e, L, K, B, o, iters, stopped)) return -1;
  if (e->divergence && br_divergence(e, L, kj, B)) return -1;
  hipLaunchKernelGGL(k_br_labels, dim3((n + BT - 1) / BT, B), dim3(BT), 0, st, L->H.as<double>(), hstride, K, n,
                     L->labels.as<int32_t>());
  HIPCHK(hipGetLastError());
  if (dcounts) {
    hipLaunchKernelGGL(k_br_counts, dim3((n + 15) / 16, (n + 15) / 16), dim3(BT), 0, st, L->labels.as<int32_t>(), B, n,
                       dcounts + (size_t)n * n * ki);
    HIPCHK(hipGetLastError());
  }
  if (out && out->labels)
    HIPCHK(hipMemcpyAsync(out->labels + (size_t)ki * B * n, L->labels.p, sizeof(int32_t) * (size_t)B * n,
                          hipMemcpyDeviceToHost, st));
  if (out && (out->W || out->H)) {
    hw.resize((size_t)B * wstride);
    hh.resize((size_t)B * hstride);
    HIPCHK(hipMemcpyAsync(hw.data(), L->W.p, sizeof(double) * hw.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hh.data(), L->H.p, sizeof(double) * hh.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out->W)
      for (int b = 0; b < B; ++b)
        for (int c = 0; c < K; ++c)
          for (int i = 0; i < m; ++i)
            out->W[kj.woff + (long)b * wstride + (long)c * m + i] = hw[(size_t)b * wstride + (size_t)i * K + c];
    if (out->H) memcpy(out->H + kj.hoff, hh.data(), sizeof(double) * hh.size());
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    *tot_iters += iters[b];
    *max_it = std::max(*max_it, iters[b]);
    if (out && out->iters) out->iters[(size_t)ki * B + b] = iters[b];
    if (out && out->stopped_early) out->stopped_early[(size_t)ki * B + b] = stopped[b];
  }
  return 0;
}

}  // namespace

extern "C" {

const char* nmfc_build_tuning_brunet(void) { return NMFC_TUNING_BRUNET; }

void nmfc_brunet_default_opts(nmfc_brunet_opts* o) {
  memset(o, 0, sizeof *o);
  o->maxiter = 2000;        // NMF.div maxniter
  o->stopconv = 40;         // nmfconsensus stopconv
  o->stopfreq = 10;         // nmfconsensus stopfreq
  o->seed = 123456789u;     // nmfconsensus rseed
  o->restart_begin = 0;
  o->restart_end = -1;
  o->verbose = 0;
}

nmfc_brunet* nmfc_brunet_create(int device, const double* A, int m, int n, int a_on_device) {
  if (!A || m <= 0 || n <= 0) {
    errorf("nmfc_brunet_create: bad arguments (A=%p m=%d n=%d)", (const void*)A, m, n);
    return nullptr;
  }
  nmfc_brunet* e = new nmfc_brunet();
  auto fail = [&](const char* what, hipError_t err) -> nmfc_brunet* {
    nmfc_host::hip_fail("nmfc_brunet_create", what, err);
    nmfc_brunet_destroy(e);
    return nullptr;
  };
  hipError_t err;
  if (device >= 0 && (err = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", err);
  if ((err = hipGetDevice(&e->dev)) != hipSuccess) return fail("hipGetDevice", err);
  if ((err = hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", err);
  if (const char* s = getenv("NMFC_BRUNET_LANES")) e->nlanes = std::max(1, std::min(BR_LANES, atoi(s)));
  e->m = m;
  e->n = n;
  e->m_pad = round_up(m, BT);
  e->n_pad = round_up(n, BT);
  // fixed gene chunks (a function of m only): about 16 chunks of whole LDS tiles, at most 2048 genes
  e->gc = (int)std::min<long>(2048, std::max<long>(TL, round_up((m + 15) / 16, TL)));
  e->nchunks = (m + e->gc - 1) / e->gc;
  if (e->Acm.ensure(sizeof(double) * e->m_pad * n) || e->Arm.ensure(sizeof(double) * (size_t)m * e->n_pad)) {
    nmfc_brunet_destroy(e);
    return nullptr;
  }
  if ((err = hipMemsetAsync(e->Acm.p, 0, e->Acm.bytes, e->st)) != hipSuccess) return fail("memset", err);
  if ((err = hipMemsetAsync(e->Arm.p, 0, e->Arm.bytes, e->st)) != hipSuccess) return fail("memset", err);
  const double* dA = A;
  DevBuf tmp;
  if (!a_on_device) {
    if (tmp.ensure(sizeof(double) * (size_t)m * n)) {
      nmfc_brunet_destroy(e);
      return nullptr;
    }
    if ((err = hipMemcpyAsync(tmp.p, A, sizeof(double) * (size_t)m * n, hipMemcpyHostToDevice, e->st)) != hipSuccess)
      return fail("upload A", err);
    dA = tmp.as<double>();
  }
  DevBuf dbad;
  if (dbad.ensure(sizeof(int))) {
    nmfc_brunet_destroy(e);
    return nullptr;
  }
  if ((err = hipMemsetAsync(dbad.p, 0, sizeof(int), e->st)) != hipSuccess) return fail("memset", err);
  hipLaunchKernelGGL(k_br_layout, dim3((m + BT - 1) / BT, n), dim3(BT), 0, e->st, dA, m, n, e->m_pad, e->n_pad,
                     e->Acm.as<double>(), e->Arm.as<double>(), dbad.as<int>());
  if ((err = hipGetLastError()) != hipSuccess) return fail("k_br_layout", err);
  int bad = 0;
  if ((err = hipMemcpyAsync(&bad, dbad.p, sizeof(int), hipMemcpyDeviceToHost, e->st)) != hipSuccess)
    return fail("read-back", err);
  if ((err = hipStreamSynchronize(e->st)) != hipSuccess) return fail("sync", err);
  if (bad) {
    // the KL updates need A >= 0; the bound keeps the batched reciprocals' products normal (recip_batch)
    errorf("nmfc_brunet_create: A must hold finite, non-negative entries of at most 2^64");
    nmfc_brunet_destroy(e);
    return nullptr;
  }
  return e;
}

int nmfc_brunet_device(const nmfc_brunet* e) { return e ? e->dev : -1; }

void nmfc_brunet_destroy(nmfc_brunet* e) {
  if (!e) return;
  // every stream is synchronised before anything is freed and destroyed after everything is
  hipStream_t sts[BR_LANES + 1] = {e->st};
  for (int l = 0; l < BR_LANES; ++l) sts[l + 1] = e->lanes[l].st;
  for (hipStream_t st : sts)
    if (st) (void)hipStreamSynchronize(st);
  for (BrLane& L : e->lanes) {
    br_drain(&L);
    L.timer.destroy_events();
  }
  delete e;   // every DevBuf / PinBuf member frees itself
  for (hipStream_t st : sts)
    if (st) (void)hipStreamDestroy(st);
}

void nmfc_brunet_set_timing(nmfc_brunet* e, int enable) {
  if (e) e->timing = enable != 0;
}

long long nmfc_brunet_kernel_time(nmfc_brunet* e, int kid, double* ms_out, double* flops_per_launch) {
  if (!e || kid < 0 || kid >= BK_N) return -1;
  if (ms_out) *ms_out = e->kms[kid];
  if (flops_per_launch) *flops_per_launch = e->kcount[kid] ? e->kfl_sum[kid] / e->kcount[kid] : 0.0;
  return e->kcount[kid];
}

void nmfc_brunet_set_divergence(nmfc_brunet* e, int enable) {
  if (e) e->divergence = enable != 0;
}

namespace {
int div_ready(const nmfc_brunet* e, const char* who) {
  if (!e) {
    errorf("%s: NULL engine", who);
    return -1;
  }
  if (!e->div_valid) {
    errorf("%s: the last run on this engine had the divergence disabled (nmfc_brunet_set_divergence) or failed", who);
    return -1;
  }
  return 0;
}
}  // namespace

int nmfc_brunet_divergence(nmfc_brunet* e, double* div_out) {
  if (div_ready(e, "nmfc_brunet_divergence")) return -1;
  if (!div_out) {
    errorf("nmfc_brunet_divergence: NULL output");
    return -1;
  }
  memcpy(div_out, e->div_vals.data(), sizeof(double) * e->div_vals.size());
  return (int)e->div_vals.size();
}

int nmfc_brunet_log_probe(nmfc_brunet* e, const double* x, int count, double* y) {
  if (!e || !x || !y || count <= 0) {
    errorf("nmfc_brunet_log_probe: bad arguments");
    return -1;
  }
  HIPCHK(hipSetDevice(e->dev));
  DevBuf dx, dy;
  if (dx.ensure(sizeof(double) * count) || dy.ensure(sizeof(double) * count)) return -1;
  hipError_t err = hipMemcpyAsync(dx.p, x, sizeof(double) * count, hipMemcpyHostToDevice, e->st);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_br_log, dim3((count + BT - 1) / BT), dim3(BT), 0, e->st, dx.as<double>(), count, dy.as<double>());
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipMemcpyAsync(y, dy.p, sizeof(double) * count, hipMemcpyDeviceToHost, e->st);
  if (err == hipSuccess) err = hipStreamSynchronize(e->st);
  if (err != hipSuccess) {
    errorf("nmfc_brunet_log_probe: %s", hipGetErrorString(err));
    return -1;
  }
  return 0;
}

int nmfc_brunet_quot_probe(nmfc_brunet* e, const double* a, const double* p, int count, int batch, double* q_out,
                           double* r_out) {
  if (!e || !a || !p || !q_out || count <= 0 || batch < 1 || batch > BR_RCP_MAX || count % batch != 0) {
    errorf("nmfc_brunet_quot_probe: bad arguments (count=%d must be a positive multiple of batch=%d in 1..%d)", count,
           batch, BR_RCP_MAX);
    return -1;
  }
  HIPCHK(hipSetDevice(e->dev));
  const size_t bytes = sizeof(double) * (size_t)count;
  const int nb = count / batch;
  DevBuf da, dp, dq, dr;
  if (da.ensure(bytes) || dp.ensure(bytes) || dq.ensure(bytes) || dr.ensure(bytes)) return -1;
  hipError_t err = hipMemcpyAsync(da.p, a, bytes, hipMemcpyHostToDevice, e->st);
  if (err == hipSuccess) err = hipMemcpyAsync(dp.p, p, bytes, hipMemcpyHostToDevice, e->st);
  if (err == hipSuccess) {
    const dim3 grid((nb + BT - 1) / BT), block(BT);
    const double *xa = da.as<double>(), *xp = dp.as<double>();
    double *xq = dq.as<double>(), *xr = dr.as<double>();
    static_assert(BR_RCP_MAX == 5, "nmfc_brunet_quot_probe: one case per batch size");
    switch (batch) {
      case 1: hipLaunchKernelGGL(k_br_quot<1>, grid, block, 0, e->st, xa, xp, nb, xq, xr); break;
      case 2: hipLaunchKernelGGL(k_br_quot<2>, grid, block, 0, e->st, xa, xp, nb, xq, xr); break;
      case 3: hipLaunchKernelGGL(k_br_quot<3>, grid, block, 0, e->st, xa, xp, nb, xq, xr); break;
      case 4: hipLaunchKernelGGL(k_br_quot<4>, grid, block, 0, e->st, xa, xp, nb, xq, xr); break;
      default: hipLaunchKernelGGL(k_br_quot<5>, grid, block, 0, e->st, xa, xp, nb, xq, xr); break;
    }
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipMemcpyAsync(q_out, dq.p, bytes, hipMemcpyDeviceToHost, e->st);
  if (err == hipSuccess && r_out) err = hipMemcpyAsync(r_out, dr.p, bytes, hipMemcpyDeviceToHost, e->st);
  if (err == hipSuccess) err = hipStreamSynchronize(e->st);
  if (err != hipSuccess) {
    errorf("nmfc_brunet_quot_probe: %s", hipGetErrorString(err));
    return -1;
  }
  return 0;
}

int nmfc_brunet_best(nmfc_brunet* e, int32_t* best_restart_out, double* best_div_out, double* W_out, double* H_out) {
  if (div_ready(e, "nmfc_brunet_best")) return -1;
  const int m = e->m, n = e->n, nk = (int)e->div_ks.size();
  HIPCHK(hipSetDevice(e->dev));
  std::vector<double> tmp;
  long woff = 0, hoff = 0;
  for (int ki = 0; ki < nk; ++ki) {
    const int K = e->div_ks[ki], b = e->best_slot[ki];
    if (best_restart_out) best_restart_out[ki] = e->div_rb + b;
    if (best_div_out) best_div_out[ki] = e->div_vals[(size_t)ki * e->div_B + b];
    if (W_out) {   // the lane layout [gene][K] to m x K column-major
      tmp.resize((size_t)m * K);
      HIPCHK(hipMemcpyAsync(tmp.data(), e->bestW[ki].p, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, e->st));
      HIPCHK(hipStreamSynchronize(e->st));
      for (int c = 0; c < K; ++c)
        for (int i = 0; i < m; ++i) W_out[woff + (long)c * m + i] = tmp[(size_t)i * K + c];
    }
    if (H_out) {
      HIPCHK(hipMemcpyAsync(H_out + hoff, e->bestH[ki].p, sizeof(double) * (size_t)n * K, hipMemcpyDeviceToHost, e->st));
      HIPCHK(hipStreamSynchronize(e->st));
    }
    woff += (long)m * K;
    hoff += (long)n * K;
  }
  return nk;
}

int nmfc_brunet_run(nmfc_brunet* e, const int* ks, int nk, int R, const nmfc_brunet_opts* opts_in,
                    const double* W_init, const double* H_init, nmfc_result* out) {
  if (e) e->div_valid = false;   // until this run has filled them
  if (!e || !ks || nk <= 0 || R <= 0) {
    errorf("nmfc_brunet_run: bad arguments");
    return -1;
  }
  nmfc_brunet_opts o;
  if (opts_in)
    o = *opts_in;
  else
    nmfc_brunet_default_opts(&o);
  const int m = e->m, n = e->n;
  if (o.maxiter < 1 || o.stopfreq < 1 || o.stopconv < 1) {
    errorf("nmfc_brunet_run: maxiter, stopfreq and stopconv must be >= 1");
    return -1;
  }
  for (int q = 0; q < nk; ++q)
    if (ks[q] < 2 || ks[q] > BR_KMAX) {
      errorf("nmfc_brunet_run: k=%d unsupported (need 2 <= k <= %d)", ks[q], BR_KMAX);
      return -1;
    }
  const int rb = std::max(0, o.restart_begin);
  const int re = o.restart_end < 0 ? R : std::min(o.restart_end, R);
  if (rb >= re) {
    errorf("nmfc_brunet_run: empty restart range [%d, %d)", rb, re);
    return -1;
  }
  o.restart_begin = rb;
  const int B = re - rb;
  HIPCHK(hipSetDevice(e->dev));
  auto t0 = std::chrono::steady_clock::now();
  int32_t* dcounts = nullptr;
  const size_t nn = (size_t)n * n;
  if (out && (out->counts || out->consensus)) {
    if (out->counts && out->counts_on_device) {
      dcounts = out->counts;
    } else {
      if (e->counts_tmp.ensure(sizeof(int32_t) * nn * nk)) return -1;
      dcounts = e->counts_tmp.as<int32_t>();
    }
  }
  // jobs: output offsets in nmfconsensus order; executed largest k first
  std::vector<KJob> jobs(nk);
  long woff = 0, hoff = 0;
  for (int ki = 0; ki < nk; ++ki) {
    jobs[ki] = {ki, ks[ki], woff, hoff};
    woff += (long)B * m * ks[ki];
    hoff += (long)B * n * ks[ki];
  }
  std::vector<KJob> order(jobs);
  std::stable_sort(order.begin(), order.end(), [](const KJob& a, const KJob& b) { return a.K > b.K; });
  const int nl = std::min(o.lanes > 0 ? std::min(o.lanes, BR_LANES) : e->nlanes, nk);
  if (e->divergence) {
    e->div_ks.assign(ks, ks + nk);
    e->div_B = B;
    e->div_rb = rb;
    e->div_vals.assign((size_t)nk * B, 0.0);
    e->best_slot.assign(nk, 0);
    if ((int)e->bestW.size() < nk) e->bestW.resize(nk), e->bestH.resize(nk);
  }
  std::vector<long long> lane_iters(nl, 0);
  std::vector<int> lane_max(nl, 0);
  for (int l = 0; l < nl; ++l) {
    BrLane& L = e->lanes[l];
    L.timing = e->timing;
    for (int q = 0; q < BK_N; ++q) L.kms[q] = 0, L.kcount[q] = 0, L.kfl_sum[q] = 0;
  }
  // the k batches, largest first, on nl lanes (csrc/lane_pool.hpp; the scheduler alone runs under TSan in the CPU
  // suite): a lane touches only its own BrLane, its lane_iters / lane_max slot and the outputs of its k
  std::string first_err;
  const int rc = nmfc_host::run_lanes(
      nl, nk,
      [&](int l, int idx) {
        return br_run_k(e, &e->lanes[l], order[idx], B, R, o, W_init, H_init, dcounts, out, &lane_iters[l], &lane_max[l]);
      },
      [] { return std::string(nmfc_last_error()); }, &first_err);
  if (rc) {
    nmfc_set_error(first_err.c_str());
    return -1;
  }
  long long tot_iters = 0;
  int max_it = 0;
  for (int q = 0; q < BK_N; ++q) e->kms[q] = 0, e->kcount[q] = 0, e->kfl_sum[q] = 0;
  for (int l = 0; l < nl; ++l) {
    tot_iters += lane_iters[l];
    max_it = std::max(max_it, lane_max[l]);
    for (int q = 0; q < BK_N; ++q) {
      e->kms[q] += e->lanes[l].kms[q];
      e->kcount[q] += e->lanes[l].kcount[q];
      e->kfl_sum[q] += e->lanes[l].kfl_sum[q];
    }
  }
  hipStream_t st = e->st;
  if (out && dcounts) {
    if (out->consensus) {
      if (e->cons_tmp.ensure(sizeof(double) * nn * nk)) return -1;
      hipLaunchKernelGGL(k_br_divide, dim3((unsigned)((nn * nk + BT - 1) / BT)), dim3(BT), 0, st, dcounts, (double)R,
                         (long)(nn * nk), e->cons_tmp.as<double>());
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(out->consensus, e->cons_tmp.p, sizeof(double) * nn * nk, hipMemcpyDeviceToHost, st));
    }
    if (out->counts && !out->counts_on_device)
      HIPCHK(hipMemcpyAsync(out->counts, dcounts, sizeof(int32_t) * nn * nk, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  e->div_valid = e->divergence;
  auto t1 = std::chrono::steady_clock::now();
  if (out) {
    out->seconds_total = std::chrono::duration<double>(t1 - t0).count();
    out->seconds_iterate = out->seconds_total;
    out->restart_iterations = tot_iters;
    out->max_iter_run = max_it;
  }
  if (o.verbose)
    fprintf(stderr, "[nmfc brunet] %d restarts x %d k on %d lanes, mean iters %.1f, max %d, %.3f s\n", B, nk, nl,
            (double)tot_iters / ((double)B * nk), max_it, std::chrono::duration<double>(t1 - t0).count());
  return 0;
}

}  // extern "C"
