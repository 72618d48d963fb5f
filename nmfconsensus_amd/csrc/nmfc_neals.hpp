// nmfc_neals.hpp -- nmf_neals: the normal-equation ALS kernels (k_hupdate_neals, k_wsolve_neals, k_neals_stop).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmfc_hupdate.hpp"

namespace nmfc {

// ---------------------------------------------------------------------------------------------
// nmf_neals (nmf_neals.c:86-495; DESIGN.md "NEALS"): the normal-equation ALS rule.  Per iteration
//   H <- max(0, (W0^T W0)^-1 W0^T A)   (:200-204, :294-295)      W <- max(0, (H H^T)^-1 H A^T)^T   (:302-306, :397-403)
// both by LU with partial pivoting (dgesv).  k_hupdate_neals is k_hupdate's sibling: it factors the Gram matrix once per
// workgroup in LDS, solves one sample per thread, accumulates S = H H^T in k_hupdate's fixed order, factors S too and
// publishes its LU in the restart's SHP rows (row c0 + i, KMAX doubles: row i of L \ U, unit diagonal of L implied) with
// the row permutation in lupiv[c0 + i] (row i of P S is row lupiv[c0 + i] of S).  The A h^T kernels' RULE_NEALS forms
// store the raw product; k_wsolve_neals solves S y = c with that LU, one gene row per thread, clamps, writes W and
// folds calculateMaxchange(W, W0)'s two maxima; k_neals_stop tests delta = max(dh, dw) on every iteration > 1.
// An exactly zero pivot stops the restart (the reference's QR fallback is not built): stop_reason 4 for the H solve
// (H not written, no W step), 5 for the W solve (H written, no W step).
// ---------------------------------------------------------------------------------------------
constexpr int NEALS_ZERO_G = 4, NEALS_ZERO_S = 5;   // stop_reason: status 1 / 2 of nmfc_engine_neals_status

// LU with partial pivoting of the k x k matrix a (row stride KMAX) in LDS.  Every thread of the workgroup calls (the
// barriers); the first KMAX * KMAX = 256 threads hold one entry each and thread KMAX keeps perm, the others (k_hupdate_neals
// runs NTH = 512) only find the pivot and wait.  dgetf2's pivot choice and layout: the pivot of column c is the first
// entry of largest magnitude in rows c.., the rows are interchanged (whole rows), L gets a unit diagonal.  Its
// arithmetic is not copied: the multipliers are quotients a / pivot (dgetf2 scales by the reciprocal) and the update is
// one FMA per entry.  perm[i]: the row of the input that ended as row i.  *zero: 0, or c + 1 when column c's pivot is
// exactly 0.0 (dgesv's info); the factorization stops there.
__device__ __forceinline__ void lu_factor_lds(double* a, int* perm, int* zero, int k, int tid) {
  const int i = tid >> 4, j = tid & 15;
  if (tid < KMAX) perm[tid] = tid;
  if (tid == 0) *zero = 0;
  __syncthreads();
  for (int c = 0; c < k; ++c) {
    int p = c;   // every thread finds the same pivot (LDS broadcast reads)
    double best = fabs(a[c * KMAX + c]);
    for (int r = c + 1; r < k; ++r) {
      const double v = fabs(a[r * KMAX + c]);
      if (v > best) {
        best = v;
        p = r;
      }
    }
    const double pv = a[p * KMAX + c];
    __syncthreads();   // the column is read
    if (pv == 0.0) {   // workgroup-uniform
      if (tid == 0) *zero = c + 1;
      break;
    }
    if (p != c) {
      if (tid < k) {
        const double t = a[c * KMAX + tid];
        a[c * KMAX + tid] = a[p * KMAX + tid];
        a[p * KMAX + tid] = t;
      }
      if (tid == KMAX) {
        const int t = perm[c];
        perm[c] = perm[p];
        perm[p] = t;
      }
    }
    __syncthreads();
    const bool in = tid < KMAX * KMAX && i > c && i < k && j >= c && j < k;
    double l = 0.0, u = 0.0;
    if (in) {
      l = a[i * KMAX + c] / pv;
      u = a[c * KMAX + j];
    }
    __syncthreads();   // column c is read before the multipliers replace it
    if (in) {
      if (j == c)
        a[i * KMAX + c] = l;
      else
        a[i * KMAX + j] = fma(-l, u, a[i * KMAX + j]);
    }
    __syncthreads();
  }
  __syncthreads();   // *zero
}

// x <- (L U)^-1 x for the unit-lower / upper factors in lu (row stride KMAX; LDS, every lane reads the same address);
// the caller has applied the row permutation to x.
template <int K>
__device__ __forceinline__ void lu_solve(const double* lu, double* x) {
#pragma unroll
  for (int i = 1; i < K; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) x[i] = fma(-lu[i * KMAX + j], x[j], x[i]);
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
#pragma unroll
    for (int j = i + 1; j < K; ++j) x[i] = fma(-lu[i * KMAX + j], x[j], x[i]);
    x[i] = x[i] / lu[i * KMAX + i];
  }
}

struct NealsSmem {
  double g[KMAX * KMAX];    // W0^T W0, then its LU; later H H^T and its LU
  double Hn[KMAX * HCH2];
  double shp[NTH];
  int perm[KMAX];
  int zero;
  unsigned long long dmax, omax;
};

template <int K, int GSV = 32>
__device__ __forceinline__ void hupdate_neals_body(const RestartInfo me, int iter, int maxiter, bool tol, int n, long n_pad,
                                                   const double* __restrict__ Gpart, long g_ld, long g_split, int gsplit,
                                                   int nsplit, const double* __restrict__ SWpart, long sw_total,
                                                   double* __restrict__ H, double* __restrict__ SH,
                                                   int* __restrict__ stop_iter, int* __restrict__ stop_reason,
                                                   int* __restrict__ n_stopped, double* __restrict__ SHP,
                                                   int* __restrict__ lupiv, int* __restrict__ colact,
                                                   double* __restrict__ Hstat, NealsSmem& sm) {
  constexpr int GS = (GSV / K) < 1 ? 1 : (GSV / K) > 16 ? 16 : (GSV / K);
  constexpr int k = K;
  const int rid = me.rid, tid = threadIdx.x, c0 = me.col0;
  const bool check = tol && iter > 1;   // iteration 1's delta is not tested (nmf_neals.c:447)
  double* Hn = sm.Hn;
  if (tid == 0) {
    sm.dmax = 0ull;
    sm.omax = 0ull;
  }
  // W0^T W0: the chunk partials in chunk order, as hupdate_body sums them
  for (int idx = tid; idx < k * k; idx += NTH) {
    const double* src = SWpart + me.sq_off + idx;
    double sacc = 0.0;
    for (int g0 = 0; g0 < nsplit; g0 += 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = (g0 + u < nsplit) ? src[(long)(g0 + u) * sw_total] : 0.0;
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (g0 + u < nsplit) sacc = (g0 + u == 0) ? v[u] : sacc + v[u];
    }
    sm.g[(idx / k) * KMAX + (idx % k)] = sacc;
  }
  lu_factor_lds(sm.g, sm.perm, &sm.zero, k, tid);
  if (sm.zero) {   // status 1: the restart keeps the factors of its last complete iteration
    if (tid == 0) {
      stop_iter[rid] = iter;
      stop_reason[rid] = NEALS_ZERO_G;
      atomicAdd(n_stopped, 1);
    }
    return;
  }
  int pr[K];   // the right-hand side's rows are read in pivot order: the interchanges cost nothing
#pragma unroll
  for (int a = 0; a < K; ++a) pr[a] = sm.perm[a];
  // h h^T: hupdate_body's pair scheme and its T, chosen against 256 threads, so that a restart's sums run in the order
  // they have there (a function of k only); with NTH = 512 the upper half of the workgroup idles in this part
  const int npairs = k * (k + 1) / 2;
  const int T = (npairs * 8 <= 256) ? 8 : (npairs * 4 <= 256) ? 4 : (npairs * 2 <= 256) ? 2 : 1;
  const int pid = tid / T, pq = tid % T;
  int pa = 0, pb = 0;
  if (pid < npairs) {
    int t = pid;
    while (t >= k - pa) {
      t -= k - pa;
      ++pa;
    }
    pb = pa + t;
  }
  double shacc = 0.0, tdm = 0.0, tom = 0.0;
  for (int j0 = 0; j0 < n; j0 += HCH2) {
    const int j = j0 + tid;
    const bool valid = j < n;
    double hc[K], gs[K];
#pragma unroll
    for (int a = 0; a < K; ++a) {
      hc[a] = 0.0;
      gs[a] = 0.0;
    }
    if (valid) {
      if (check) {
#pragma unroll
        for (int a = 0; a < K; ++a) hc[a] = H[(long)(c0 + a) * n_pad + j];
      }
      const double* gsrc = Gpart + (long)c0 * g_ld + j;
      for (int g0 = 0; g0 < gsplit; g0 += GS) {
        double v[GS][K];
#pragma unroll
        for (int u = 0; u < GS; ++u) {   // chunks past the end re-read the last one (not added)
          const double* q = gsrc + (long)min(g0 + u, gsplit - 1) * g_split;
#pragma unroll
          for (int a = 0; a < K; ++a) v[u][a] = q[(long)pr[a] * g_ld];
        }
#pragma unroll
        for (int u = 0; u < GS; ++u)
          if (g0 + u < gsplit) {
#pragma unroll
            for (int a = 0; a < K; ++a) gs[a] = (g0 + u == 0) ? v[u][a] : gs[a] + v[u][a];
          }
      }
      lu_solve<K>(sm.g, gs);
    }
    if (j0 > 0) __syncthreads();   // Hn free
#pragma unroll
    for (int a = 0; a < K; ++a) {
      double hn = 0.0;
      if (valid) {
        hn = gs[a] > 0.0 ? gs[a] : 0.0;   // ZERO_THRESHOLD = 0: NaN, -0.0 and negatives become +0.0
        H[(long)(c0 + a) * n_pad + j] = hn;
        if (check) {
          tdm = fmax(tdm, fabs(hc[a] - hn));
          tom = fmax(tom, fabs(hc[a]));
        }
      }
      Hn[a * HCH2 + tid] = hn;
    }
    __syncthreads();
    if (pid < npairs) {
      const int cnt = min(HCH2, n - j0);
      const double* ha = Hn + pa * HCH2;
      const double* hb = Hn + pb * HCH2;
      int q = pq;
      for (; q + 7 * T < cnt; q += 8 * T) {
        double xa[8], xb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          xa[u] = ha[q + u * T];
          xb[u] = hb[q + u * T];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) shacc = fma(xa[u], xb[u], shacc);
      }
      for (; q < cnt; q += T) shacc = fma(ha[q], hb[q], shacc);
    }
  }
  sm.shp[tid] = shacc;
  if (check) {
    atomicMax(&sm.dmax, (unsigned long long)__double_as_longlong(tdm));
    atomicMax(&sm.omax, (unsigned long long)__double_as_longlong(tom));
  }
  __syncthreads();   // shp, dmax / omax; every sample's solve has read the LU of W0^T W0
  if (check && tid == 0)
    Hstat[rid] = __longlong_as_double((long long)sm.dmax) / (SQRTEPS + __longlong_as_double((long long)sm.omax));
  if (pid < npairs && pq == 0) {
    double s = sm.shp[tid];
    for (int q = 1; q < T; ++q) s += sm.shp[tid + q];
    SH[me.sq_off + pa * k + pb] = s;
    SH[me.sq_off + pb * k + pa] = s;
    sm.g[pa * KMAX + pb] = s;
    sm.g[pb * KMAX + pa] = s;
  }
  lu_factor_lds(sm.g, sm.perm, &sm.zero, k, tid);
  if (sm.zero) {   // status 2: H of this iteration is written, W keeps the previous iteration's
    if (tid == 0) {
      stop_iter[rid] = iter;
      stop_reason[rid] = NEALS_ZERO_S;
      atomicAdd(n_stopped, 1);
    }
    return;
  }
  if (tid < KMAX * KMAX && (tid >> 4) < k) SHP[(long)(c0 + (tid >> 4)) * KMAX + (tid & 15)] = (tid & 15) < k ? sm.g[tid] : 0.0;
  if (tid < k) {
    lupiv[c0 + tid] = sm.perm[tid];
    colact[c0 + tid] = iter;   // this restart's columns take part in the W update
  }
  if (tid == 0 && iter >= maxiter) {
    stop_iter[rid] = iter;
    stop_reason[rid] = 2;
    atomicAdd(n_stopped, 1);
  }
}

static __global__ __launch_bounds__(NTH, 4) void k_hupdate_neals(int iter, int maxiter, int tol,
                                                                const RestartInfo* __restrict__ ri, int n, long n_pad,
                                                                const double* __restrict__ Gpart, long g_ld, long g_split,
                                                                int gsplit, int nsplit, const double* __restrict__ SWpart,
                                                                long sw_total, double* __restrict__ H,
                                                                double* __restrict__ SH, int* __restrict__ stop_iter,
                                                                int* __restrict__ stop_reason, int* __restrict__ n_stopped,
                                                                double* __restrict__ SHP, int* __restrict__ lupiv,
                                                                int* __restrict__ colact, double* __restrict__ Hstat) {
  __shared__ NealsSmem sm;
  const RestartInfo me = ri[blockIdx.x];
  if (stop_iter[me.rid] != 0) return;
#define NMFC_HUPD_CASE(KK)                                                                                            \
  case KK:                                                                                                            \
    hupdate_neals_body<KK>(me, iter, maxiter, tol != 0, n, n_pad, Gpart, g_ld, g_split, gsplit, nsplit, SWpart,       \
                           sw_total, H, SH, stop_iter, stop_reason, n_stopped, SHP, lupiv, colact, Hstat, sm);        \
    break;
  switch (me.k) {
    NMFC_HUPD_CASE(2) NMFC_HUPD_CASE(3) NMFC_HUPD_CASE(4) NMFC_HUPD_CASE(5) NMFC_HUPD_CASE(6)
    NMFC_HUPD_CASE(7) NMFC_HUPD_CASE(8) NMFC_HUPD_CASE(9) NMFC_HUPD_CASE(10) NMFC_HUPD_CASE(11)
    NMFC_HUPD_CASE(12) NMFC_HUPD_CASE(13) NMFC_HUPD_CASE(14) NMFC_HUPD_CASE(15) NMFC_HUPD_CASE(16)
    default: break;
  }
#undef NMFC_HUPD_CASE
}

// The W solve: workgroup (restart, block of NT gene rows), one gene row per thread.  Craw holds H A^T of the restart's
// columns (k_ahtw4<RULE_NEALS>); c is read in pivot order, solved with the LU of H H^T and clamped with nmf_neals.c:397-403's
// `if (w < 0) w = 0` (NaN and -0.0 pass); W still holds W0, so the two maxima of calculateMaxchange(W, W0) are folded
// here (wd / wo: per restart, non-negative doubles as bits; k_neals_stop reads and zeroes them).  Padded gene rows are
// written +0.0: they feed W^T W.
template <int K>
__device__ __forceinline__ void wsolve_neals_body(const RestartInfo me, int check, int m, long m_pad,
                                                  const double* __restrict__ Craw, double* __restrict__ W,
                                                  const double* lu, const int* perm, unsigned long long* __restrict__ wd,
                                                  unsigned long long* __restrict__ wo, unsigned long long* red) {
  const long i = (long)blockIdx.y * NT + threadIdx.x;
  const int c0 = me.col0;
  double tdm = 0.0, tom = 0.0;
  if (i < m) {
    double x[K];
#pragma unroll
    for (int a = 0; a < K; ++a) x[a] = Craw[(long)(c0 + perm[a]) * m_pad + i];
    lu_solve<K>(lu, x);
#pragma unroll
    for (int a = 0; a < K; ++a) {
      const double v = x[a] < 0.0 ? 0.0 : x[a];
      double* dst = W + (long)(c0 + a) * m_pad + i;
      if (check) {
        const double o = *dst;
        tdm = fmax(tdm, fabs(o - v));
        tom = fmax(tom, fabs(o));
      }
      *dst = v;
    }
  } else if (i < m_pad) {
#pragma unroll
    for (int a = 0; a < K; ++a) W[(long)(c0 + a) * m_pad + i] = 0.0;
  }
  if (check) {
    atomicMax(&red[0], (unsigned long long)__double_as_longlong(tdm));
    atomicMax(&red[1], (unsigned long long)__double_as_longlong(tom));
    __syncthreads();
    if (threadIdx.x == 0) {
      atomicMax(&wd[me.rid], red[0]);
      atomicMax(&wo[me.rid], red[1]);
    }
  }
}

static __global__ __launch_bounds__(NT) void k_wsolve_neals(int iter, int check, const RestartInfo* __restrict__ ri, int m,
                                                            long m_pad, const double* __restrict__ Craw,
                                                            double* __restrict__ W, const double* __restrict__ SHP,
                                                            const int* __restrict__ lupiv, const int* __restrict__ colact,
                                                            unsigned long long* __restrict__ wd,
                                                            unsigned long long* __restrict__ wo) {
  __shared__ double lu[KMAX * KMAX];
  __shared__ int perm[KMAX];
  __shared__ unsigned long long red[2];
  const RestartInfo me = ri[blockIdx.x];
  if (colact[me.col0] != iter) return;   // stopped earlier, or a zero pivot at this iteration: no W step
  const int tid = threadIdx.x;
  lu[tid] = (tid >> 4) < me.k ? SHP[(long)(me.col0 + (tid >> 4)) * KMAX + (tid & 15)] : 0.0;
  if (tid < KMAX) perm[tid] = tid < me.k ? lupiv[me.col0 + tid] : 0;
  if (tid < 2) red[tid] = 0ull;
  __syncthreads();
#define NMFC_WSOLVE_CASE(KK)                                                                    \
  case KK:                                                                                      \
    wsolve_neals_body<KK>(me, check, m, m_pad, Craw, W, lu, perm, wd, wo, red);                 \
    break;
  switch (me.k) {
    NMFC_WSOLVE_CASE(2) NMFC_WSOLVE_CASE(3) NMFC_WSOLVE_CASE(4) NMFC_WSOLVE_CASE(5) NMFC_WSOLVE_CASE(6)
    NMFC_WSOLVE_CASE(7) NMFC_WSOLVE_CASE(8) NMFC_WSOLVE_CASE(9) NMFC_WSOLVE_CASE(10) NMFC_WSOLVE_CASE(11)
    NMFC_WSOLVE_CASE(12) NMFC_WSOLVE_CASE(13) NMFC_WSOLVE_CASE(14) NMFC_WSOLVE_CASE(15) NMFC_WSOLVE_CASE(16)
    default: break;
  }
#undef NMFC_WSOLVE_CASE
}

// The stop test of nmf_neals.c:447-457 on every iteration > 1, one thread per live restart: delta = max(dh, dw) < TolX,
// or TolFun >= 1 (dnorm0 = dnorm is assigned before dnorm <= TolFun * dnorm0 is tested, so that arm fires exactly then).
static __global__ __launch_bounds__(NT) void k_neals_stop(int iter, int nact, const RestartInfo* __restrict__ ri,
                                                          const int* __restrict__ colact, const double* __restrict__ Hstat,
                                                          unsigned long long* __restrict__ wd,
                                                          unsigned long long* __restrict__ wo, double TolX, double TolFun,
                                                          int* __restrict__ stop_iter, int* __restrict__ stop_reason,
                                                          int* __restrict__ n_stopped) {
  const int x = blockIdx.x * NT + threadIdx.x;
  if (x >= nact) return;
  const RestartInfo me = ri[x];
  if (colact[me.col0] != iter) return;
  const double dw = __longlong_as_double((long long)wd[me.rid]) / (SQRTEPS + __longlong_as_double((long long)wo[me.rid]));
  wd[me.rid] = 0ull;
  wo[me.rid] = 0ull;
  if (stop_iter[me.rid] != 0) return;   // iter == maxiter
  const double dh = Hstat[me.rid];
  const double delta = dh > dw ? dh : dw;
  if (delta < TolX || TolFun >= 1.0) {
    stop_iter[me.rid] = iter;
    stop_reason[me.rid] = 3;
    atomicAdd(n_stopped, 1);
  }
}

}  // namespace nmfc
