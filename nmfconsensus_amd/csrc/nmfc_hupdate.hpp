// nmfc_hupdate.hpp -- k_hupdate: the H update, h h^T and the stop rules, one workgroup per restart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmfc_common.hpp"

namespace nmfc {

// ---------------------------------------------------------------------------------------------
// K2 "hupdate": one workgroup per active restart.
//   work1 = W0^T W0 = sum of the per-chunk Gram partials (nmf_mu.c:176); work2 = work1 H0 (:178);
//   H <- mu_rule(H, G, work2) (:184-191); SH = H H^T (:200); stability check (:253-282).
// ---------------------------------------------------------------------------------------------
constexpr int NTH = 512;           // threads of the H-update kernel (one sample per thread and round)
constexpr int HCH2 = NTH;          // samples per round

struct HupdSmem {
  double sw[KMAX * KMAX];
  double Hn[KMAX * HCH2];
  double win[KMAX * KMAX];
  double shp[NTH];
  int changed;
  unsigned long long dmax, omax;   // STOP_TOLX: max |h0 - h| and max |h0| (non-negative doubles as bits)
};

// The body for rank K (compile time).  Latency is what matters here (one workgroup per restart, often
// only a few restarts live): every load the workgroup needs is issued before its first use -- the stop
// state, the Gram partials and the first round's H and W^T A partials together -- and the split-K
// partials of one sample are loaded GS chunks at a time (GS*K <= 64 values in flight per thread).  The
// arithmetic order is fixed: chunk partials and Gram partials summed in chunk order, d = sum_b in b order,
// h h^T by T = f(k) threads per pair over j = pq (mod T) in j order, then the T partials in pq order.
// RULE_EUCLID: euclid_rule_h instead of mu_rule, and the membership check (STOP_MEMBER) instead of the four nmf_mu
// rules: on iterations that are multiples of stopfreq, the 1-based first-maximum row of every sample against the stored
// one (the zeroed classes row is R's old.membership <- 0, so the first check always counts as a change).
template <int K, int GSV = 32, int RULE = RULE_MU>
__device__ __forceinline__ void hupdate_body(const RestartInfo me, int iter, int maxiter, int stop_rule, int stopconv,
                                             int stopfreq, int n,
                                             long n_pad, const double* __restrict__ Gpart, long g_ld, long g_split,
                                             int gsplit, int nsplit, const double* __restrict__ SWpart, long sw_total,
                                             double* __restrict__ H, double* __restrict__ SH,
                                             int* __restrict__ stop_iter, int* __restrict__ stop_reason,
                                             int* __restrict__ unchanged, int* __restrict__ classes, long cls_ld,
                                             int* __restrict__ n_stopped, double* __restrict__ SHP,
                                             int* __restrict__ colact, double* __restrict__ Hstat, HupdSmem& sm) {
  // GSV: chunk-partial values in flight per thread (32: 128 VGPRs, two workgroups per CU).  Round 4 measured a
  // "latency form" <100, 2> (every chunk of a C3 restart in one group of loads, one workgroup per CU) for launches
  // of at most one restart per CU: the 8-GPU replay went 380.8 -> 373.3 per GPU, so it is not used.
  constexpr int GS = (GSV / K) < 1 ? 1 : (GSV / K) > 16 ? 16 : (GSV / K);
  double* sw = sm.sw;
  double* Hn = sm.Hn;
  double* win = sm.win;
  double* shp = sm.shp;
  int& changed = sm.changed;
  const int rid = me.rid;
  const int tid = threadIdx.x;
  constexpr int k = K;
  const int c0 = me.col0;
  constexpr bool EUC = RULE == RULE_EUCLID;
  const bool check = EUC ? (stop_rule == STOP_MEMBER && iter % stopfreq == 0)
                         : ((stop_rule != STOP_FIXED) && iter > 1 && (iter % 2 == 0));
  const bool tolx = !EUC && check && stop_rule == STOP_TOLX;
  constexpr int CLS0 = EUC ? 1 : 0;   // stored class of row 0: 1-based for the membership rule (0 = none yet)
  double tdm = 0.0, tom = 0.0;   // this thread's max |h0 - h| and max |h0| (STOP_TOLX)
  // stop state, loaded now and used at the end
  const int u_prev = (tid == 0 && check) ? unchanged[rid] : 0;
  const int nwin = k < n ? k : n;
  const bool refc = !EUC && check && stop_rule == STOP_REF_COMPAT;
  const int cl_prev = (refc && tid < nwin) ? classes[(long)rid * cls_ld + tid] : 0;
  // the sample rounds' loads: H and the split-K partials of W^T A (first group issued here)
  auto load_h = [&](int j, double* hc) {
#pragma unroll
    for (int a = 0; a < K; ++a) hc[a] = H[(long)(c0 + a) * n_pad + j];
  };
  auto sum_g = [&](int j, double* gs) {   // chunk partials of this sample, added in chunk order
    const double* gsrc = Gpart + (long)c0 * g_ld + j;
    for (int g0 = 0; g0 < gsplit; g0 += GS) {
      double v[GS][K];
#pragma unroll
      for (int u = 0; u < GS; ++u) {   // chunks past the end re-read the last one (not added)
        const double* q = gsrc + (long)min(g0 + u, gsplit - 1) * g_split;
#pragma unroll
        for (int a = 0; a < K; ++a) v[u][a] = q[(long)a * g_ld];
      }
#pragma unroll
      for (int u = 0; u < GS; ++u)
        if (g0 + u < gsplit) {
#pragma unroll
          for (int a = 0; a < K; ++a) gs[a] = (g0 + u == 0) ? v[u][a] : gs[a] + v[u][a];
        }
    }
  };
  if (tid == 0) {
    changed = 0;
    sm.dmax = 0ull;
    sm.omax = 0ull;
  }
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
    sw[(idx / k) * KMAX + (idx % k)] = sacc;
  }
  for (int idx = tid; idx < KMAX * KMAX; idx += NTH) win[idx] = 0.0;
  // h h^T: T threads per (pa, pb) pair (T a function of k only); thread pq of a pair sums the samples
  // j = pq (mod T) in order, and the T partials are added in pq order at the end.
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
  double shacc = 0.0;

  for (int j0 = 0; j0 < n; j0 += HCH2) {
    const int j = j0 + tid;
    const bool valid = j < n;
    double hc[K], gs[K];
#pragma unroll
    for (int a = 0; a < K; ++a) {
      hc[a] = 0.0;
      gs[a] = 0.0;
    }
    int cl_j = 0;
    if (valid) {
      load_h(j, hc);
      if ((EUC ? check : (check && stop_rule == STOP_ARGMAX_STABLE))) cl_j = classes[(long)rid * cls_ld + j];
      sum_g(j, gs);
    }
    __syncthreads();   // sw, win (first round) / Hn free (later rounds)
    int best = 0;
    double bestv = 0.0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      double hn = 0.0;
      if (valid) {
        double d = 0.0;
#pragma unroll
        for (int bb = 0; bb < K; ++bb) d = fma(sw[a * KMAX + bb], hc[bb], d);
        if constexpr (EUC)
          hn = euclid_rule_h(hc[a], gs[a], d);
        else
          hn = mu_rule(hc[a], gs[a], d);
        H[(long)(c0 + a) * n_pad + j] = hn;
        if (tolx) {   // calculateMaxchange(h, h0) (calculatemaxchange.c:55-60): dlange('M') of h0 and h0 - h
          tdm = fmax(tdm, fabs(hc[a] - hn));
          tom = fmax(tom, fabs(hc[a]));
        }
        if (refc) {
          // flat column-major index of (a, j) in the k x n buffer; window i reads [i*n, i*n + k)
          const int tf = j * k + a;
          const int wi = tf / n;
          const int wj = tf - wi * n;
          if (wi < k && wj < k) win[wi * KMAX + wj] = hn;
        }
      }
      Hn[a * HCH2 + tid] = hn;
      if (a == 0 || hn > bestv) {   // first maximum
        best = a;
        bestv = hn;
      }
    }
    if ((EUC ? check : (check && stop_rule == STOP_ARGMAX_STABLE)) && valid && cl_j != best + CLS0) {
      classes[(long)rid * cls_ld + j] = best + CLS0;
      changed = 1;
    }
    __syncthreads();
    if (pid < npairs) {
      const int cnt = min(HCH2, n - j0);
      const double* ha = Hn + pa * HCH2;
      const double* hb = Hn + pb * HCH2;
      // 8 samples' operands loaded ahead of their (in-order) FMAs: the LDS latency is paid once per 8 terms
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
  shp[tid] = shacc;
  if (tolx) {
    atomicMax(&sm.dmax, (unsigned long long)__double_as_longlong(tdm));
    atomicMax(&sm.omax, (unsigned long long)__double_as_longlong(tom));
  }
  __syncthreads();
  if (tolx && tid == 0)
    Hstat[rid] = __longlong_as_double((long long)sm.dmax) / (SQRTEPS + __longlong_as_double((long long)sm.omax));
  if (pid < npairs && pq == 0) {
    double s = shp[tid];
    for (int q = 1; q < T; ++q) s += shp[tid + q];
    SH[me.sq_off + pa * k + pb] = s;
    SH[me.sq_off + pb * k + pa] = s;
    if (SHP) {   // the panel-row copy for the W update: row = global column c0 + a, KMAX doubles
      SHP[(long)(c0 + pa) * KMAX + pb] = s;
      SHP[(long)(c0 + pb) * KMAX + pa] = s;
    }
  }
  if (colact && tid < k) colact[c0 + tid] = iter;   // this restart's columns take part in the W update
  if (refc && tid < nwin) {
    int c = 0;
    for (int jj = 1; jj < k; ++jj)
      if (win[tid * KMAX + jj] > win[tid * KMAX + jj - 1]) c = jj;
    if (cl_prev != c) {
      classes[(long)rid * cls_ld + tid] = c;
      changed = 1;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int reason = 0;
    if (check && stop_rule != STOP_TOLX) {   // the TolX test runs after the W update (k_wstat)
      if (!changed) {
        const int u = u_prev + 1;
        unchanged[rid] = u;
        if (u >= stopconv) reason = 1;   // nmf_mu.c:269-271 (200) / the script's stopconv
      } else {
        unchanged[rid] = 0;
      }
    }
    if (!reason && iter >= maxiter) reason = 2;
    if (reason) {
      stop_iter[rid] = iter;
      stop_reason[rid] = reason;
      atomicAdd(n_stopped, 1);
    }
  }
}

// <32, 4>: 4 waves per SIMD, two 512-thread workgroups per CU (full-load launch 150 -> 118 us).
template <int GSV = 32, int MINW = 4, int RULE = RULE_MU>
static __global__ __launch_bounds__(NTH, MINW) void k_hupdate(int iter, int maxiter, typename RuleArgs<RULE>::Stop stop,
                                                        const RestartInfo* __restrict__ ri, int n, long n_pad,
                                                        const double* __restrict__ Gpart, long g_ld, long g_split,
                                                        int gsplit, int nsplit, const double* __restrict__ SWpart,
                                                        long sw_total,
                                                        double* __restrict__ H, double* __restrict__ SH,
                                                        int* __restrict__ stop_iter, int* __restrict__ stop_reason,
                                                        int* __restrict__ unchanged, int* __restrict__ classes,
                                                        long cls_ld, int* __restrict__ n_stopped,
                                                        double* __restrict__ SHP, int* __restrict__ colact,
                                                        double* __restrict__ Hstat) {
  __shared__ HupdSmem sm;
  const RestartInfo me = ri[blockIdx.x];
  if (stop_iter[me.rid] != 0) return;
#define NMFC_HUPD_CASE(KK)                                                                                      \
  case KK:                                                                                                     \
    hupdate_body<KK, GSV, RULE>(me, iter, maxiter, stop_rule_of(stop), stopconv_of(stop), stopfreq_of(stop), n, n_pad, Gpart, g_ld, g_split, gsplit, nsplit, SWpart, sw_total, H, SH, \
                     stop_iter, stop_reason, unchanged, classes, cls_ld, n_stopped, SHP, colact, Hstat, sm);   \
    break;
  switch (me.k) {
    NMFC_HUPD_CASE(2) NMFC_HUPD_CASE(3) NMFC_HUPD_CASE(4) NMFC_HUPD_CASE(5) NMFC_HUPD_CASE(6)
    NMFC_HUPD_CASE(7) NMFC_HUPD_CASE(8) NMFC_HUPD_CASE(9) NMFC_HUPD_CASE(10) NMFC_HUPD_CASE(11)
    NMFC_HUPD_CASE(12) NMFC_HUPD_CASE(13) NMFC_HUPD_CASE(14) NMFC_HUPD_CASE(15) NMFC_HUPD_CASE(16)
    default: break;
  }
#undef NMFC_HUPD_CASE
}

}  // namespace nmfc
