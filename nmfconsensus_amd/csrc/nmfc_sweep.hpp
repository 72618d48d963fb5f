// nmfc_sweep.hpp -- the sweep's plumbing: repacking, the init streams, the TolX statistic, labels, counts and the
// layouts of A.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmfc_common.hpp"
#include "rmt.hpp"

namespace nmfc {

// ---------------------------------------------------------------------------------------------
// Repacking (compaction of live restarts) and the final-factor archive: k rows per job.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(NT) void k_move_rows(const MoveJob* __restrict__ jobs, const double* __restrict__ src,
                                                         long src_ld, double* __restrict__ dst, long dst_ld, long len) {
  const MoveJob jb = jobs[blockIdx.x];
  for (int a = 0; a < jb.k; ++a) {
    const double* s = src + (long)(jb.src_row + a) * src_ld;
    double* d = dst + (long)(jb.dst_row + a) * dst_ld;
    for (long x = (long)blockIdx.y * NT + threadIdx.x; x < len; x += (long)gridDim.y * NT) d[x] = s[x];
  }
}

// ---------------------------------------------------------------------------------------------
// Init: generateMatrix(ran) (generatematrix.c:131-137) with randnumber (randnumber.c:34) over the
// glibc TYPE_3 stream seeded per job.  Thread = (restart, chunk of 31 * rnb draws); the chunk's start
// state is J[c] * s_344 (mod 2^32), J[c] = M^(c * 31 * rnb) the 31x31 jump matrix of the lagged
// recurrence r[i] = r[i-31] + r[i-3].  The host picks rnb per run: long chunks (few jump products) when the
// sweep has draws enough to fill the GPU, short ones when it has not (C1's 73 000 draws were 74 threads).
// ---------------------------------------------------------------------------------------------
constexpr int RCHUNK = 31 * 32;   // longest chunk: draws per thread (a multiple of 31: a statically indexed ring)

static __global__ __launch_bounds__(NT) void k_init(const InitJob* __restrict__ jobs, const int* __restrict__ chunk_job,
                                                    const int* __restrict__ chunk_idx, int total_chunks,
                                                    const uint32_t* __restrict__ jump, int rnb, int m, int n, long m_pad,
                                                    long n_pad, int min_init, int max_init, double* __restrict__ W,
                                                    double* __restrict__ H) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total_chunks) return;
  const InitJob jb = jobs[chunk_job[gid]];
  const int c = chunk_idx[gid];
  // srand(seed): r[0..30] by the Park-Miller LCG (Schrage), r[31..33] = r[0..2]
  uint32_t ring[31];
  int32_t word = (int32_t)(jb.seed ? jb.seed : 1u);
  ring[0] = (uint32_t)word;
#pragma unroll
  for (int i = 1; i < 31; ++i) {
    long hi = word / 127773;
    long lo = word % 127773;
    long wv = 16807 * lo - 2836 * hi;
    if (wv < 0) wv += 2147483647;
    word = (int32_t)wv;
    ring[i] = (uint32_t)word;
  }
  // ring[q] holds r[q]; r[31..33] = r[0..2] occupy the same slots.  Steps i = 34..343 (10 x 31).
#pragma unroll 1
  for (int blk = 0; blk < 10; ++blk) {
#pragma unroll
    for (int q = 0; q < 31; ++q) {
      const int pos = (3 + q) % 31;
      ring[pos] = ring[pos] + ring[(pos + 28) % 31];
    }
  }
  // ordered window s[q] = r[313 + q] sits at ring[(3 + q) % 31]
  uint32_t s[31];
#pragma unroll
  for (int q = 0; q < 31; ++q) s[q] = ring[(3 + q) % 31];
  if (c > 0) {
    const uint32_t* J = jump + (long)c * 31 * 31;
#pragma unroll
    for (int q = 0; q < 31; ++q) {
      uint32_t v = 0;
#pragma unroll
      for (int pq = 0; pq < 31; ++pq) v += J[q * 31 + pq] * s[pq];
      ring[q] = v;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 31; ++q) ring[q] = s[q];
  }
  // ring[q] = r[i0 - 31 + q]; step jj overwrites slot jj % 31 with r[i0+jj] = slot + slot[(jj+28)%31].
  // Draw t goes to W (column-major m x k: row i, column a) while t < m k, then to H (k x n: row a, column jcol);
  // both positions advance incrementally (one division per thread, not two 64-bit divisions per draw).
  const int mk = m * jb.k;
  const int total = mk + jb.k * n;
  int t = c * 31 * rnb;
  int p0, p1;   // (i, a) in W, then (a, jcol) in H
  if (t < mk) {
    p1 = t / m;
    p0 = t - p1 * m;
  } else {
    p1 = (t - mk) / jb.k;
    p0 = (t - mk) - p1 * jb.k;
  }
#pragma unroll 1
  for (int blk = 0; blk < rnb; ++blk) {
#pragma unroll
    for (int q = 0; q < 31; ++q) {
      const uint32_t v = ring[q] + ring[(q + 28) % 31];
      ring[q] = v;
      if (t < total) {
        const int32_t o = (int32_t)(v >> 1);
        const int32_t prod = (int32_t)((uint32_t)(max_init - min_init) * (uint32_t)o);
        const double val = (double)min_init + (double)prod / 2147483647.0;
        if (t < mk) {
          W[(long)(jb.col0 + p1) * m_pad + p0] = val;
          if (++p0 == m) {
            p0 = 0;
            if (++p1 == jb.k) p1 = 0;   // t + 1 == mk: H starts at (a, jcol) = (0, 0)
          }
        } else {
          H[(long)(jb.col0 + p0) * n_pad + p1] = val;
          if (++p0 == jb.k) {
            p0 = 0;
            ++p1;
          }
        }
      }
      ++t;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Init, R path (nmf.r:37-38): the BatchJobs job seed s = seed + job_id - 1, then set.seed(s);
// W <- runif(m*k) (column-major m x k); H <- runif(k*n) (column-major k x n).  One workgroup per
// restart walks R's Mersenne-Twister stream (rmt.hpp) 624 draws at a time.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(NT) void k_init_runif(const InitJob* __restrict__ jobs, int m, int n, long m_pad,
                                                          long n_pad, double* __restrict__ W, double* __restrict__ H) {
  __shared__ uint32_t mt[624];
  const InitJob jb = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  if (tid == 0) rmt::seed_table(mt, jb.seed);
  __syncthreads();
  const long mk = (long)m * jb.k, total = mk + (long)jb.k * n;
  for (long base = 0; base < total; base += 624) {
    rmt::regenerate<NT>(mt);
    for (int t = tid; t < 624; t += NT) {
      const long d = base + t;
      if (d >= total) break;
      const double u = rmt::unif(mt[t]);
      if (d < mk) {
        const long a = d / m, i = d - a * m;
        W[(long)(jb.col0 + a) * m_pad + i] = u;
      } else {
        const long tt = d - mk, jcol = tt / jb.k, a = tt - jcol * jb.k;
        H[(long)(jb.col0 + a) * n_pad + jcol] = u;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// STOP_TOLX, after the W update of an even iteration > 1 (nmf_als.c:304-349 applied to MU): one
// workgroup per live restart: dw = calculateMaxchange(W, W0) from the pre-update snapshot W0,
// delta = max(dh, dw) with dh from k_hupdate; stop if delta < TolX, or if TolFun >= 1 (the test
// dnorm <= TolFun * dnorm0 runs after dnorm0 = dnorm, nmf_als.c:330/:345, so it only fires then --
// or on an exactly-zero residual, which is not evaluated here).
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(NT) void k_wstat(int iter, const RestartInfo* __restrict__ ri,
                                                     const double* __restrict__ W, const double* __restrict__ W0,
                                                     long m_pad, int m, const int* __restrict__ colact,
                                                     const double* __restrict__ Hstat, double TolX, double TolFun,
                                                     int* __restrict__ stop_iter, int* __restrict__ stop_reason,
                                                     int* __restrict__ n_stopped) {
  __shared__ unsigned long long dmax, omax;
  const RestartInfo me = ri[blockIdx.x];
  if (stop_iter[me.rid] != 0 || colact[me.col0] != iter) return;   // stopped, or no W update this iteration
  if (threadIdx.x == 0) {
    dmax = 0ull;
    omax = 0ull;
  }
  __syncthreads();
  double tdm = 0.0, tom = 0.0;
  for (int a = 0; a < me.k; ++a) {
    const double* w = W + (long)(me.col0 + a) * m_pad;
    const double* w0 = W0 + (long)(me.col0 + a) * m_pad;
    for (int i = threadIdx.x; i < m; i += NT) {
      const double o = w0[i];
      tdm = fmax(tdm, fabs(o - w[i]));
      tom = fmax(tom, fabs(o));
    }
  }
  atomicMax(&dmax, (unsigned long long)__double_as_longlong(tdm));
  atomicMax(&omax, (unsigned long long)__double_as_longlong(tom));
  __syncthreads();
  if (threadIdx.x == 0) {
    const double dw = __longlong_as_double((long long)dmax) / (SQRTEPS + __longlong_as_double((long long)omax));
    const double dh = Hstat[me.rid];
    const double delta = dh > dw ? dh : dw;
    if (delta < TolX || TolFun >= 1.0) {
      stop_iter[me.rid] = iter;
      stop_reason[me.rid] = 3;
      atomicAdd(n_stopped, 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Labels (nmf.r:128 / documented intent) and connectivity counts (nmf.r:140-141).
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(NT) void k_labels(const RestartInfo* __restrict__ ri, const int* __restrict__ slot,
                                                      const double* __restrict__ H, long n_pad, int n, int rule,
                                                      int32_t* __restrict__ labels) {
  const int r = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int c0 = ri[r].col0, k = ri[r].k;
  int best = 0;
  double bv = H[(long)c0 * n_pad + j];
  for (int a = 1; a < k; ++a) {
    const double v = H[(long)(c0 + a) * n_pad + j];
    if (rule == 0 ? (v > bv) : (v < bv)) {
      bv = v;
      best = a;
    }
  }
  labels[(long)slot[r] * n + j] = best + 1;
}

// counts[g][i + j*n] = sum over the group's restarts of [L[i] == L[j]] (nmf.r:140-141).  A workgroup owns a
// 64 x 64 block of (i, j); the two 64-label strips of CR restarts at a time are staged in LDS (each label
// read once per block) and every thread accumulates a 4 x 4 register block of exact integer counts.
constexpr int CNT_T = 64, CNT_R = 32;
static __global__ __launch_bounds__(NT) void k_counts(const int32_t* __restrict__ labels,
                                                      const int* __restrict__ grp_begin,
                                                      const int* __restrict__ grp_list, int n,
                                                      int32_t* __restrict__ counts) {
  __shared__ int32_t li[CNT_R][CNT_T], lj[CNT_R][CNT_T];
  const int gidx = blockIdx.z;
  const int i0 = blockIdx.x * CNT_T, j0 = blockIdx.y * CNT_T;
  const int tid = threadIdx.x, ti = (tid & 15) * 4, tj = (tid >> 4) * 4;
  const int b = grp_begin[gidx], e = grp_begin[gidx + 1];
  int32_t cnt[4][4] = {};
  for (int q0 = b; q0 < e; q0 += CNT_R) {
    const int nr = min(CNT_R, e - q0);
    for (int x = tid; x < nr * CNT_T; x += NT) {
      const int r = x / CNT_T, c = x % CNT_T;
      const int32_t* L = labels + (long)grp_list[q0 + r] * n;
      li[r][c] = (i0 + c < n) ? L[i0 + c] : -1;
      lj[r][c] = (j0 + c < n) ? L[j0 + c] : -2;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      int32_t a[4], bb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = li[r][ti + u];
        bb[u] = lj[r][tj + u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) cnt[u][v] += (a[u] == bb[v]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int j = j0 + tj + v;
    if (j >= n) continue;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + ti + u;
      if (i < n) counts[(long)gidx * n * n + (long)j * n + i] = cnt[u][v];
    }
  }
}

static __global__ void k_divide(const int32_t* __restrict__ counts, double denom, long len, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < len) out[i] = (double)counts[i] / denom;
}

// A (m x n, ld lda) -> Acm (column j at j*m_pad, zero padded) and Arm (row i at i*n_pad)
static __global__ void k_layout_a(const double* __restrict__ A, long lda, int m, int n, long m_pad, long n_pad,
                                  double* __restrict__ Acm, double* __restrict__ Arm) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y;
  if (i >= m) return;
  const double v = A[(long)j * lda + i];
  if (Acm) Acm[(long)j * m_pad + i] = v;
  Arm[i * n_pad + j] = v;
}

// A -> Ablk, the K-blocked operand of W^T A: Ablk[(i / 16) * ld * 16 + j * 16 + i % 16] (ld = n_cols_pad rows),
// so the 16-gene block of a tile's sample rows is one contiguous run.  Block (x, y): NT genes x the 16
// sample columns 16 y ..; lanes run along the genes of one column (16 doubles = 128 B contiguous).
static __global__ __launch_bounds__(NT) void k_layout_ablk(const double* __restrict__ A, long lda, int m, int n, long ld,
                                                           double* __restrict__ Ablk) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;   // gene
  if (i >= m) return;
  const long kb = i >> 4, r = i & 15;
#pragma unroll 4
  for (int jj = 0; jj < 16; ++jj) {
    const int j = 16 * blockIdx.y + jj;
    if (j < n) Ablk[kb * ld * 16 + (long)j * 16 + r] = A[(long)j * lda + i];
  }
}

}  // namespace nmfc
