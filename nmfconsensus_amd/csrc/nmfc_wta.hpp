// nmfc_wta.hpp -- W^T A on the GTile core: k_wta2, the stream-K k_wta2_sk and the narrow (tail) forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "nmfc_gtile.hpp"

namespace nmfc {

// ---------------------------------------------------------------------------------------------
// K1 v2 "wta2": G = W^T A on the GTile core.  A tile = NPT panels (64*NPT restart columns) x RQ
// samples; waves WR x WC.  Gram blocks (per panel: 4 diagonal + 3 straddling 16x16 blocks) are spread
// over the ntj sample-tile workgroups of the panel group and their waves.
// ---------------------------------------------------------------------------------------------
// GRAM = false: no Gram blocks (a probe: a wave carrying a Gram chain sets every barrier step of its workgroup,
// 20-35 % of a 1-panel tile's time and 4-7 % of the 2- and 4-panel tiles', tools/tailbench.hip).
// GITEM (1-panel tiles): the Gram blocks run in 3 extra workgroups per (chunk, panel), their first three waves
// each one candidate block as a 1-wave GTile<16, 16> (P, Q = the block's W rows; the rest of the wave set exits),
// beside the W^T A workgroups instead of on their waves (bit-identical: see k_wta_narrow).
// Gram candidate blocks of an NPT-panel tile, diagonal blocks first: cand < 4 NPT is the diagonal block
// cand & 3 of panel cand >> 2; the rest are the 3 blocks per panel straddling two 16-column blocks (needed only
// when a restart crosses a block boundary, which the engine's 16-column block packing never produces).
// cand = t + ntj (w + NW x) then gives waves 0..3 of each sample-tile workgroup one diagonal block each when
// ntj = 4, one Gram chain per SIMD (a wave w shares its SIMD with w + 4): 4 MFMAs on the SIMD's 128 per stage,
// where the per-panel order (7 candidates per panel) put two chains on each of two SIMDs (+2.6 % W^T A, C3).
template <int NPT>
__device__ __forceinline__ void gram_cand(int cand, int& q, int& br, int& bc) {
  if (cand < 4 * NPT) {
    q = cand >> 2;
    br = bc = cand & 3;
  } else {
    const int s = cand - 4 * NPT;
    q = s / 3;
    br = s % 3;
    bc = br + 1;
  }
}

// GREG (4-panel tiles, ntj >= 4): each diagonal Gram block is accumulated by a wave of the wave row that holds the
// block's W rows, from the tile's own W fragments (GTile GREG) -- no LDS reads of its own; wave column (wr >> 1) & 1
// of wave row wr, so at ntj = 4 the four chains of a workgroup sit on four SIMDs.  The straddling candidates (never
// produced by the engine's 16-column block packing) keep the LDS form.  Same operands, same K order: bit-identical.
template <int NPT, int RQ, int WR, int WC, int GPW, int NBUF = GT_NBUF, int MINW = 1, bool ABLK = false, bool GRAM = true,
          bool GITEM = false, bool GREG = false, bool SPLIT = true>
static __global__ __launch_bounds__(WR * WC * 64, MINW) void k_wta2(const double* __restrict__ W, const double* __restrict__ Acm,
                                                              long m_pad, int ngroups, int ntj, int nsplit, int kchunk,
                                                              const int* __restrict__ prb, const int* __restrict__ pre,
                                                              const RestartInfo* __restrict__ ri,
                                                              const ColInfo* __restrict__ ci,
                                                              const int* __restrict__ stop_iter, double* __restrict__ Gpart,
                                                              long g_ld, long g_split, double* __restrict__ SWpart,
                                                              long sw_total) {
  using T = GTile<64 * NPT, RQ, WR, WC, NBUF, ABLK, GREG, SPLIT>;
  static_assert(!GREG || (WR == NPT && GPW == 1 && GRAM && !GITEM), "register Gram: one panel per wave row");
  constexpr int NCAND = 7 * NPT;
  __shared__ __attribute__((aligned(1024))) char smem[T::LDS_BYTES + 64];
  int* need = reinterpret_cast<int*>(smem + T::LDS_BYTES);
  constexpr int NGW = GITEM ? 3 : 0;   // Gram workgroups per (chunk, panel)
  const int ntt = ntj + NGW;
  const int nitems = nsplit * ngroups * ntt;
  const int item = xcd_item(blockIdx.x, nitems);
  const int t = item % ntt;
  const int pg = (item / ntt) % ngroups;
  const int s = item / (ntt * ngroups);
  if constexpr (GITEM) {
    static_assert(NPT == 1 && T::NW >= 3, "Gram items: 1-panel tiles of at least 3 waves");
    using TG = GTile<16, 16, 1, 1, NBUF, false>;
    static_assert(3 * TG::LDS_BYTES <= T::LDS_BYTES, "three Gram rings fit the tile's");
    if (t >= ntj) {
      const int w = wave_id(), l = threadIdx.x & 63, fr = l & 15, g = l >> 4;
      const int x = 3 * (t - ntj) + w;   // candidate: 4 diagonal, 3 straddling blocks
      if (w >= 3 || x >= 7) return;
      if (!panel_live(prb, pre, pg, ri, stop_iter, 0)) return;
      const int br = x < 4 ? x : x - 4, bc = x < 4 ? x : x - 3;
      const ColInfo* cp = ci + (long)pg * PANEL;
      if (br != bc) {   // a straddling block only when the restart at column 16 bc started before it
        const ColInfo c = cp[16 * bc];
        if (!(c.k > 0 && c.lc0 < 16 * bc)) return;
      }
      const int kbeg = s * kchunk;
      const int kend = (int)min((long)kbeg + kchunk, m_pad);
      TG tg;
      tg.wo = w;
      tg.zero();
      const double* Pr = W + ((long)pg * PANEL + 16 * br) * m_pad + kbeg;
      const double* Qr = W + ((long)pg * PANEL + 16 * bc) * m_pad + kbeg;
      tg.run(Pr, m_pad, Qr, m_pad, 0, kend - kbeg, smem + w * TG::LDS_BYTES, [](const char*) {});
      double* so = SWpart + (long)s * sw_total;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int lr = 16 * br + g + 4 * reg, lcn = 16 * bc + fr;
        const ColInfo cr = cp[lr];
        if (cr.k == 0 || cr.lc0 != cp[lcn].lc0 || cp[lcn].k == 0) continue;   // not the same restart
        const int a = lr - cr.lc0, b = lcn - cr.lc0;
        so[cr.sq_off + a * cr.k + b] = tg.acc[0][0][reg];
        so[cr.sq_off + b * cr.k + a] = tg.acc[0][0][reg];
      }
      return;
    }
  }
  bool live[NPT];
  bool any = false;
#pragma unroll
  for (int q = 0; q < NPT; ++q) {
    live[q] = panel_live(prb, pre, NPT * pg + q, ri, stop_iter, 0);
    any = any || live[q];
  }
  if (!any) return;
  if (threadIdx.x < NCAND) {
    int q, br, bc;
    gram_cand<NPT>(threadIdx.x, q, br, bc);
    int nd = live[q];
    if (nd && br != bc) {
      const ColInfo c = ci[(long)(NPT * pg + q) * PANEL + 16 * bc];
      nd = (c.k > 0 && c.lc0 < 16 * bc);
    }
    need[threadIdx.x] = nd;
  }
  // ABLK: Acm is K-blocked over all ntj * RQ sample rows.  Both operands are rebased to the chunk start, so the
  // buffer offsets stay within one chunk (32-bit for any n_cols_pad up to 2^17).
  const int kbeg = s * kchunk;
  const int kend = (int)min((long)kbeg + kchunk, m_pad);
  const long ldq = ABLK ? (long)ntj * RQ : m_pad;
  const double* Q = ABLK ? Acm + (long)kbeg * ldq + (long)t * RQ * 16 : Acm + (long)t * RQ * m_pad + kbeg;
  T tl;
  tl.zero();
  d4 gacc[GPW];
#pragma unroll
  for (int x = 0; x < GPW; ++x) gacc[x] = (d4){0.0, 0.0, 0.0, 0.0};
  const int w = wave_id(), l = threadIdx.x & 63;
  const int fr = l & 15, g = l >> 4;
  __syncthreads();   // need[] visible (no DMA in flight yet)
  int my_need[GPW], my_ra[GPW], my_rb[GPW];
  bool gram = false;
#pragma unroll
  for (int x = 0; x < GPW; ++x) {
    const int cand = t + ntj * (w + T::NW * x);
    my_need[x] = 0;
    my_ra[x] = 0;
    my_rb[x] = 0;
    if (cand < NCAND) {
      int q, br, bc;
      gram_cand<NPT>(cand, q, br, bc);
      my_need[x] = (GREG && (cand < 4 * NPT || WC == 4)) ? 0 : need[cand];
      my_ra[x] = 64 * q + 16 * br;
      my_rb[x] = 64 * q + 16 * bc;
      gram = GRAM && !GITEM && (gram || my_need[x]);
    }
  }
  if constexpr (GREG) {
    const int wr = w / WC, wc = w % WC;
    int gi = -1, gj = -1;
    if constexpr (WC == 4) {
      // 16 waves: every Gram candidate of panel wr that falls to this workgroup (cand % ntj == t: at most two per
      // panel for ntj >= 4) on its own wave of row wr, the k-th on wave column (t + wr + 2 k) & 3 -- the diagonal
      // chains of a workgroup on four SIMDs (wave w runs on SIMD w & 3), a straddling one two SIMDs away
      int kth = 0;
#pragma unroll
      for (int c = 0; c < 7; ++c) {   // panel wr's candidates: 4 diagonal blocks, then 3 straddling blocks
        const int cand = c < 4 ? 4 * wr + c : 4 * NPT + 3 * wr + (c - 4);
        if (cand % ntj != t) continue;
        if (wc == ((t + wr + 2 * kth) & 3) && need[cand]) {
          gi = c < 4 ? c : c - 4;
          gj = c < 4 ? c : c - 3;
        }
        ++kth;
      }
    } else if (wc == ((wr >> 1) & 1) % WC) {   // WC = 2: the diagonal blocks, wave column (wr >> 1) & 1 of row wr
#pragma unroll
      for (int br = 0; br < 4; ++br)
        if ((4 * wr + br) % ntj == t && need[4 * wr + br]) gi = gj = br;
    }
    tl.gi = __builtin_amdgcn_readfirstlane(gi);
    tl.gj = __builtin_amdgcn_readfirstlane(gj);
  }
  const double* P = W + (long)pg * 64 * NPT * m_pad + kbeg;
  auto lds_gram = [&](const char* stg) {
#pragma unroll
    for (int x = 0; x < GPW; ++x) {
      if (!my_need[x]) continue;
      const char* pa = stg + (my_ra[x] + fr) * 128;
      const char* pb = stg + (my_rb[x] + fr) * 128;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int so = ((4 * kk + g) ^ (fr >> 1)) << 4;
        const d2 a = *reinterpret_cast<const d2*>(pa + so);
        const d2 b = *reinterpret_cast<const d2*>(pb + so);
        gacc[x] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, gacc[x], 0, 0, 0);
        gacc[x] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, gacc[x], 0, 0, 0);
      }
    }
  };
  // two instantiations of the K loop: the LDS Gram chains' accumulators are live only in the loop that runs them
  // (a wave without an LDS chain -- every wave of a GREG tile under block packing -- keeps none of their registers)
  constexpr bool LDSG = GRAM && !GITEM && !(GREG && WC == 4);   // the 16-wave GREG tile keeps every chain in registers
  if constexpr (GREG && WC == 4) {
    // one K-loop instantiation per register Gram block (4 diagonal, 3 straddling, none): the block is a compile-time
    // constant in the MFMA stream, with no fragment select and no branch in the loop
    auto go = [&](auto gc) {
      tl.template run<0, 2, decltype(gc)::value>(P, m_pad, Q, ldq, 0, kend - kbeg, smem, [] { return true; },
                                                 [](const char*) {}, [] {});
    };
    switch (tl.gi < 0 ? -1 : 4 * tl.gi + tl.gj) {
      case 0: go(std::integral_constant<int, 0>{}); break;
      case 5: go(std::integral_constant<int, 5>{}); break;
      case 10: go(std::integral_constant<int, 10>{}); break;
      case 15: go(std::integral_constant<int, 15>{}); break;
      case 1: go(std::integral_constant<int, 1>{}); break;
      case 6: go(std::integral_constant<int, 6>{}); break;
      case 11: go(std::integral_constant<int, 11>{}); break;
      default: go(std::integral_constant<int, -1>{}); break;
    }
  } else if (LDSG && gram) {
    tl.run(P, m_pad, Q, ldq, 0, kend - kbeg, smem, lds_gram);
  } else {
    tl.run(P, m_pad, Q, ldq, 0, kend - kbeg, smem, [](const char*) {});
  }
  double* out = Gpart + (long)s * g_split + (long)pg * 64 * NPT * g_ld + (long)t * RQ;
#pragma unroll
  for (int mb = 0; mb < T::MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < T::NB; ++nb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) out[(long)T::row_of(mb, reg) * g_ld + T::col_of(nb)] = tl.acc[mb][nb][reg];
  // the restart-diagonal entries of Gram block (rows ra .. ra + 15, columns rb .. rb + 15 of the tile)
  auto put_gram = [&](int ra, int rb, const d4& v) {
    double* so = SWpart + (long)s * sw_total;
    const int pnl = ra >> 6;
    const ColInfo* cp = ci + (long)(NPT * pg + pnl) * PANEL;
    const int ln = lane_id();   // not the pre-loop lane values: nothing lane-derived held across the K loop
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int lr = (ra & 63) + (ln >> 4) + 4 * reg;
      const int lcn = (rb & 63) + (ln & 15);
      const ColInfo cr = cp[lr];
      if (cr.k == 0 || cr.lc0 != cp[lcn].lc0 || cp[lcn].k == 0) continue;
      const int a = lr - cr.lc0, b = lcn - cr.lc0;
      so[cr.sq_off + a * cr.k + b] = v[reg];
      so[cr.sq_off + b * cr.k + a] = v[reg];
    }
  };
  if (gram) {
#pragma unroll
    for (int x = 0; x < GPW; ++x)
      if (my_need[x]) put_gram(my_ra[x], my_rb[x], gacc[x]);
  }
  if constexpr (GREG) {
    if (tl.gi >= 0) put_gram(64 * (w / WC) + 16 * tl.gi, 64 * (w / WC) + 16 * tl.gj, tl.gacc);
  }
}

// ---------------------------------------------------------------------------------------------
// K1 stream-K form of the 16-wave 4-panel x 128-sample W^T A tile (round 6).  The big tile's grid is nsplit x ng x
// ntj items of up to kchunk / 16 stages each; as one workgroup per item (one per CU: 144 KiB of LDS) the launch takes
// ceil(items / CUs) rounds for items / CUs rounds of work (C3 at full load: 1 720 items = 6.72 rounds, the short last
// chunk makes it 6.56 rounds of work for 7 rounds of time).  Here G <= #CU persistent workgroups each take an equal
// contiguous range of the S stages of all items (in the item order of k_wta2, ranges XCD-contiguous); a range starts
// and ends anywhere inside an item, so an item is cut at a stage boundary into at most two pieces (G <= S / longest
// item).  The canonical K order is kept exactly: the first piece accumulates stages [0, x) from zero, stores its
// accumulators (G tile and register Gram chain, fp64 stores are exact) and publishes them; the second piece loads them
// and continues the same MFMA chains over [x, end) -- the same chain, instruction for instruction, as one workgroup
// running the whole item, so G and the Gram partials are bit-identical to k_wta2's (tools/kvar.hip checks it).
// Deadlock freedom without any assumption on dispatch order: every range runs its first-piece (start) item FIRST
// and its continuation LAST, and a continuation waits a bounded time; if the start piece has not been published by
// then (its workgroup not yet dispatched), it recomputes the item from stage 0 -- the same bits again, only slower.
// Hand-off (MI355X_MICROARCH.md, inter-workgroup visibility; cdna_hip_programming.md split-K recipe): plain stores ->
// every wave vmcnt(0) -> barrier -> lane 0 agent release fence -> vmcnt(0) -> relaxed agent flag store (= epoch of
// this launch); reader lane 0 relaxed agent poll -> agent acquire fence -> vmcnt(0) -> barrier -> plain loads.
// fix: G slots of SK_FIX doubles (9 d4 per lane: the 8 accumulator blocks and the Gram chain); flags: G words.
// ---------------------------------------------------------------------------------------------
constexpr int SK_THREADS = 1024;              // the 4-panel tile's 16 waves (the 2-panel tile: 8, SK_THREADS / 2)
constexpr long SK_FIX = 9L * 4 * SK_THREADS;   // doubles per range slot (either tile: 8 blocks + the Gram chain per lane)
constexpr int SK_POLLS = 256;                  // x s_sleep 127 (~3.4 us each): ~0.9 ms before recomputing

// A wave-uniform copy of a value held in VGPRs (device-function arguments arrive in VGPRs): SGPR operands for the
// buffer resources and soffsets of the K loop (a VGPR resource would wrap every buffer access in a waterfall loop).
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long uni(long v) {
  const unsigned long long u = (unsigned long long)v;
  return (long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) |
                (unsigned)__builtin_amdgcn_readfirstlane((int)(u & 0xffffffffu)));
}
template <class P>
__device__ __forceinline__ P* uni(P* p) {
  return reinterpret_cast<P*>(uni(reinterpret_cast<long>(p)));
}
// An SGPR value the compiler may not treat as loop-invariant (an empty asm that "redefines" it): what is computed from
// it stays inside the loop instead of being hoisted and held in registers across the whole loop.
template <class V>
__device__ __forceinline__ V opaque(V v) {
  asm volatile("" : "+s"(v));
  return v;
}

struct SkArgs {   // the launch's operands: k_wta2_sk's only kernel argument (offset 0 of the kernarg segment)
  const double* W;
  const double* Acm;
  long m_pad;
  int ngroups, ntj, kchunk;
  const int* prb;
  const int* pre;
  const RestartInfo* ri;
  const ColInfo* ci;
  const int* stop_iter;
  double* Gpart;
  long g_ld, g_split;
  double* SWpart;
  long sw_total;
  double* fix;
  unsigned* flags;
  unsigned epoch;
  int nsplit;
  unsigned* tcnt;   // LSUM: per-tile chunk-arrival counters (monotonic: nsplit arrivals per tile and launch)
  int dp_xcd;       // whole rounds: 0 round-robin (item k G + r), 1 XCD-contiguous blocks (a speed / DVFS probe)
};
typedef const SkArgs __attribute__((address_space(4)))* SkArgsK;   // the kernarg copy, read by scalar loads

// The kernarg segment as an opaque pointer: every operand is re-read (s_load) where it is used, instead of being held
// in SGPRs across the whole piece loop -- the K loop then keeps k_wta2's SGPR and VGPR budget (a first form spilled).
__device__ __forceinline__ SkArgsK sk_args() {
  unsigned long long u = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(u));
  return (SkArgsK)u;
}

// One piece of the stream-K range: item `item`, stages [s0, s1); mode 0 whole item, 1 start piece (publish its
// chains in slot r), 2 continuation (of slot r - 1).  Every operand is re-read through opaque() per piece, so the
// compiler cannot hoist per-piece scalars (buffer resources, row offsets of the eight K-loop instantiations) out of the
// piece loop and hold them all at once: the K loop keeps k_wta2's register budget (a first form spilled).
// LSUM (probe arm, NMFC_WTA_LASTSUM=1): the workgroup that writes a tile's last chunk partial sums
// the tile's nsplit partials in chunk order -- k_hupdate's order, the same bits -- into chunk slot 0, so k_hupdate
// reads one partial instead of nsplit.  Publication: every wave vmcnt(0) -> barrier -> lane 0 agent release -> ticket;
// the ticket that completes the tile -> agent acquire -> barrier -> plain loads.
// NPT: 4 (the 16-wave big tile) or 2 (the 8-wave 2-panel tile of k_wta2<2, 128, 2, 4, ...>: wave rows = panels, the same
// register Gram scheme, one workgroup per CU; round 6, for grids between one and two rounds of it -- the 8-GPU shard).
template <int NBUF, bool NOWAIT, bool LSUM = false, int NPT = 4>
__device__ __forceinline__ void wta_sk_piece(int r, int item_in, int s0_in, int s1_in, int mode_in,
                                             char* __restrict__ smem) {
  constexpr int RQ = 128, WC = 4;
  using T = GTile<64 * NPT, RQ, NPT, WC, NBUF, true, true, true, true>;
  static_assert(T::MB * T::NB == 8 && T::NTH <= SK_THREADS, "a slot holds 8 accumulator blocks + the Gram chain per lane");
  SkArgsK A = sk_args();
  const double* W = A->W;
  const double* Acm = A->Acm;
  const long m_pad = A->m_pad;
  const int ngroups = A->ngroups, ntj = A->ntj, kchunk = A->kchunk;
  const int* prb = A->prb;
  const int* pre = A->pre;
  const RestartInfo* ri = A->ri;
  const ColInfo* ci = A->ci;
  const int* stop_iter = A->stop_iter;
  r = uni(r);
  const int item = uni(item_in), s0 = uni(s0_in), s1 = uni(s1_in), mode = uni(mode_in);
  const unsigned epoch = A->epoch;
  // lane-derived values are computed from an opaque copy of the lane index where they are used: hoisted out of the
  // piece loop they would all be held across the K loop (one VGPR too many there)
  auto lane = [] {
    int v = lane_id();
    asm volatile("" : "+v"(v));
    return v;
  };
  int* need = reinterpret_cast<int*>(smem + T::LDS_BYTES);   // 28 Gram candidates
  int* okw = need + 7 * NPT;                                  // the continuation's "published" word
  const int w = wave_id();
  const int t = uni(item % ntj);
  const int pg = uni((item / ntj) % ngroups);
  const int s = uni(item / (ngroups * ntj));
  bool live[NPT];
  bool any = false;
#pragma unroll
  for (int q = 0; q < NPT; ++q) {
    live[q] = panel_live(prb, pre, NPT * pg + q, ri, stop_iter, 0);
    any = any || live[q];
  }
  if (!any) return;   // both pieces of a dead item see the same stop_iter: neither runs, nobody waits
  const int tid = 64 * w + lane();
  if (tid < 7 * NPT) {
    int q, br, bc;
    gram_cand<NPT>(tid, q, br, bc);
    int nd = live[q];
    if (nd && br != bc) {
      const ColInfo c = ci[(long)(NPT * pg + q) * PANEL + 16 * bc];
      nd = (c.k > 0 && c.lc0 < 16 * bc);
    }
    need[tid] = nd;
  }
  unsigned* flags = A->flags;
  double* fix = A->fix;
  if (mode == 2 && tid == 0) {
    int ok = 0;
    for (int i = 0; i < (NOWAIT ? 0 : SK_POLLS); ++i) {
      if (__hip_atomic_load(flags + (r - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch) {
        ok = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(127);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *okw = ok;
  }
  const int kbeg = s * kchunk;
  const long ldq = (long)ntj * RQ;
  const double* Q = Acm + (long)kbeg * ldq + (long)t * RQ * 16;
  T tl;
  tl.zero();
  __syncthreads();   // need[] and okw visible
  // continuation: the chains come back from slot r - 1 in run()'s pre() hook, after the prologue's first DMA issue (held
  // in registers only from there on, where the K loop holds them anyway); not published: the whole item from stage 0
  const bool cont = mode == 2 && uni(*okw) != 0;
  const int resume = uni(cont ? s0 : (mode == 2 ? 0 : s0));
  auto load_chains = [&] {
    if (cont) {
      const double* src = fix + (long)(r - 1) * SK_FIX + 4L * (64 * w);
      const int ln = lane();
#pragma unroll
      for (int mb = 0; mb < T::MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < T::NB; ++nb)
          tl.acc[mb][nb] = *reinterpret_cast<const d4*>(src + ((long)(mb * T::NB + nb) * SK_THREADS + ln) * 4);
      tl.gacc = *reinterpret_cast<const d4*>(src + ((long)T::MB * T::NB * SK_THREADS + ln) * 4);
    }
    return true;
  };
  {
    const int wr = w / WC, wc = w % WC;
    int gi = -1, gj = -1, kth = 0;
#pragma unroll
    for (int c = 0; c < 7; ++c) {   // as k_wta2 (GREG, WC = 4)
      const int cand = c < 4 ? 4 * wr + c : 4 * NPT + 3 * wr + (c - 4);
      if (cand % ntj != t) continue;
      if (wc == ((t + wr + 2 * kth) & 3) && need[cand]) {
        gi = c < 4 ? c : c - 4;
        gj = c < 4 ? c : c - 3;
      }
      ++kth;
    }
    tl.gi = __builtin_amdgcn_readfirstlane(gi);
    tl.gj = __builtin_amdgcn_readfirstlane(gj);
  }
  const double* P = W + (long)pg * 64 * NPT * m_pad + kbeg;
  auto go = [&](auto gc) {
    tl.template run<0, 2, decltype(gc)::value>(P, m_pad, Q, ldq, BK2 * resume, BK2 * s1, smem, load_chains,
                                               [](const char*) {}, [] {});
  };
  switch (tl.gi < 0 ? -1 : 4 * tl.gi + tl.gj) {
    case 0: go(std::integral_constant<int, 0>{}); break;
    case 5: go(std::integral_constant<int, 5>{}); break;
    case 10: go(std::integral_constant<int, 10>{}); break;
    case 15: go(std::integral_constant<int, 15>{}); break;
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 6: go(std::integral_constant<int, 6>{}); break;
    case 11: go(std::integral_constant<int, 11>{}); break;
    default: go(std::integral_constant<int, -1>{}); break;
  }
  if (mode == 1) {   // publish the start piece's chains for range r + 1
    // lane index by mbcnt and the wave index in an SGPR: nothing derived from threadIdx.x is held across the K loop
    A = sk_args();
    fix = A->fix;
    flags = A->flags;
    double* dst = fix + (long)r * SK_FIX + 4L * (64 * w);
    const int ln = lane();
#pragma unroll
    for (int mb = 0; mb < T::MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < T::NB; ++nb)
        *reinterpret_cast<d4*>(dst + ((long)(mb * T::NB + nb) * SK_THREADS + ln) * 4) = tl.acc[mb][nb];
    *reinterpret_cast<d4*>(dst + ((long)T::MB * T::NB * SK_THREADS + ln) * 4) = tl.gacc;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (w == 0 && ln == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(flags + r, A->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  A = sk_args();   // re-read after the K loop
  const long g_ld = A->g_ld, g_split = A->g_split;
  double* out = A->Gpart + (long)s * g_split + (long)pg * 64 * NPT * g_ld + (long)t * RQ;
  {   // T::row_of / T::col_of from the opaque lane
    const int ln = lane();
    const int r0 = (w / WC) * 64 + (ln >> 4), c0 = (w % WC) * (RQ / WC) + (ln & 15);
#pragma unroll
    for (int mb = 0; mb < T::MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < T::NB; ++nb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(long)(r0 + mb * 16 + 4 * reg) * g_ld + c0 + nb * 16] = tl.acc[mb][nb][reg];
  }
  if (tl.gi >= 0) {   // the restart-diagonal entries of the wave's Gram block (as k_wta2's put_gram)
    const int ra = 64 * (w / WC) + 16 * tl.gi, rb = 64 * (w / WC) + 16 * tl.gj;
    double* so = A->SWpart + (long)s * A->sw_total;
    const ColInfo* cp = ci + (long)(NPT * pg + (ra >> 6)) * PANEL;
    const int ln = lane();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int lr = (ra & 63) + (ln >> 4) + 4 * reg;
      const int lcn = (rb & 63) + (ln & 15);
      const ColInfo cr = cp[lr];
      if (cr.k == 0 || cr.lc0 != cp[lcn].lc0 || cp[lcn].k == 0) continue;
      const int a = lr - cr.lc0, bq = lcn - cr.lc0;
      so[cr.sq_off + a * cr.k + bq] = tl.gacc[reg];
      so[cr.sq_off + bq * cr.k + a] = tl.gacc[reg];
    }
  }
  if constexpr (LSUM) {
    A = sk_args();   // everything from the kernarg copy and `item` again: nothing extra held across the K loop
    const int nsplit = A->nsplit;
    if (nsplit > 1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const int ntj2 = A->ntj, ng2 = A->ngroups;
      const int tile = item % (ng2 * ntj2), pg2 = (item / ntj2) % ng2, t2 = item % ntj2;
      if (w == 0 && lane() == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned old = __hip_atomic_fetch_add(A->tcnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (old + 1) % (unsigned)nsplit == 0;
        if (last) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *okw = last;
      }
      __syncthreads();
      if (uni(*okw)) {   // the tile's partials, chunk 0 first, summed as k_hupdate sums them, into chunk slot 0
        const long g_ld2 = A->g_ld, g_split2 = A->g_split;
        double* base = A->Gpart + (long)pg2 * 64 * NPT * g_ld2 + (long)t2 * RQ;
        const int ln = lane();
        const int r0 = (w / WC) * 64 + (ln >> 4), c0 = (w % WC) * (RQ / WC) + (ln & 15);
#pragma unroll
        for (int mb = 0; mb < T::MB; ++mb)
#pragma unroll
          for (int nb = 0; nb < T::NB; ++nb) {
            double v[4];
            double* e0 = base + (long)(r0 + mb * 16) * g_ld2 + c0 + nb * 16;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) v[reg] = e0[(long)4 * reg * g_ld2];
            for (int c = 1; c < nsplit; ++c) {
              double u[4];
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) u[reg] = e0[(long)c * g_split2 + (long)4 * reg * g_ld2];
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) v[reg] = v[reg] + u[reg];
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) e0[(long)4 * reg * g_ld2] = v[reg];
          }
      }
    }
  }
}

// NOWAIT (tools/kvar.hip, and the engine under NMFC_WTA_SK_NOWAIT=1): every continuation takes the recompute path (tests its bits)
template <int NBUF = GT_NBUF, bool NOWAIT = false, bool LSUM = false, int NPT = 4>
static __global__ __launch_bounds__(64 * NPT * 4, 1) void k_wta2_sk(SkArgs args) {
  using T = GTile<64 * NPT, 128, NPT, 4, NBUF, true, true, true, true>;
  static_assert(NPT == 4 || NPT == 2, "the 16-wave 4-panel tile or the 8-wave 2-panel tile");
  __shared__ __attribute__((aligned(1024))) char smem[T::LDS_BYTES + 128];
  (void)args;   // read through sk_args() (the kernarg segment), see there
  SkArgsK A = sk_args();
  const int nsplit = A->nsplit;
  const int G = gridDim.x;
  const int r = __builtin_amdgcn_readfirstlane(xcd_item(blockIdx.x, G));
  // this workgroup's XCD (blocks b, b + 8, ... share one): its xcd_item range [xb, xb + xc) of the G ranges
  const int xq = G >> 3, xrem = G & 7, xcd = blockIdx.x & 7;
  const int xc = xq + (xcd < xrem ? 1 : 0), xb = xcd < xrem ? xcd * (xq + 1) : xrem * (xq + 1) + (xcd - xrem) * xq;
  const int ipc = A->ngroups * A->ntj;
  const int nitems = nsplit * ipc;
  const int nst_full = A->kchunk / BK2;
  const int nst_last = (int)((A->m_pad - (long)(nsplit - 1) * A->kchunk) / BK2);
  const int nst_max = nsplit > 1 ? nst_full : nst_last;
  const int c_last = ipc * (nsplit - 1);   // first item of the last chunk
  auto nst_of = [&](int item) { return item >= c_last ? nst_last : nst_full; };
  auto off = [&](int item) -> long {        // stage offset of an item in k_wta2's item order
    return item <= c_last ? (long)item * nst_full : (long)c_last * nst_full + (long)(item - c_last) * nst_last;
  };
  auto locate = [&](long x, int& item, int& st) {
    const long lc = (long)c_last * nst_full;
    const int it = x < lc ? (int)(x / nst_full) : c_last + (int)((x - lc) / nst_last);
    item = __builtin_amdgcn_readfirstlane(it);
    st = __builtin_amdgcn_readfirstlane((int)(x - off(it)));
  };
  // whole rounds first, item k G + r in round k (the dispatch order of k_wta2: the items a round runs at once are
  // neighbours that share their A chunk and W rows in L2); the items left after them -- between one and two rounds'
  // worth, at least G x the longest item in stages -- are split evenly over the G workgroups (stream-K)
  int D = (nitems / G - 1) * G;
  if (D < 0) D = 0;
  while (D > 0 && off(nitems) - off(D) < (long)G * nst_max) D -= G;
  D = __builtin_amdgcn_readfirstlane(D);
  const long base = off(D), S = off(nitems) - base;
  const long b = base + S * r / G, e = base + S * (r + 1) / G;
  int ib, sb, ie, se;
  locate(b, ib, sb);
  locate(e - 1, ie, se);
  ++se;   // the range's piece of item ie is [0, se)
  const bool head = sb > 0;                 // [sb, nst) of item ib: a continuation of range r - 1's start piece
  const bool tail = se < nst_of(ie);        // [0, se) of item ie: the start piece, published for range r + 1
  const int f0 = head ? ib + 1 : ib, f1 = tail ? ie - 1 : ie;   // whole items f0 .. f1 of the split part
  const int nfull = f1 >= f0 ? f1 - f0 + 1 : 0;
  const int ndp = D / G;
  const int t0 = tail ? 1 : 0;
  const int npieces = t0 + ndp + nfull + (head ? 1 : 0);
  for (int pc = 0; pc < npieces; ++pc) {
    // piece order: the whole rounds first -- every workgroup starts them together, so the workgroups that share an A
    // or W stage read it at the same time and L2 serves all but the first (starting with the split part's start pieces,
    // of every length, desynchronised them and tripled the L2-miss bytes) -- then the split part: the start piece (a
    // later range waits for it), its whole items, the continuation last.  With shares of at least one item the start
    // piece of range r - 1 ends before range r reaches its continuation, so nobody waits.
    int item, s0, s1, mode;
    if (pc < ndp) {
      item = A->dp_xcd ? ndp * xb + pc * xc + (r - xb) : pc * G + r;
      s0 = 0, s1 = nst_of(item), mode = 0;
    } else if (pc < ndp + t0) {
      item = ie, s0 = 0, s1 = se, mode = 1;
    } else if (head && pc == npieces - 1) {
      item = ib, s0 = sb, s1 = nst_of(ib), mode = 2;
    } else {
      item = f0 + pc - t0 - ndp, s0 = 0, s1 = nst_of(item), mode = 0;
    }
    __syncthreads();   // the previous piece's LDS ring, need[] and okw are free
    wta_sk_piece<NBUF, NOWAIT, LSUM, NPT>(r, item, s0, s1, mode, smem);
  }
}

// ---------------------------------------------------------------------------------------------
// K1 narrow form (the tail: the live restarts block-packed into the first nblk 16-column blocks, none
// straddling a block): G rows 16 b .. 16 b + 15 = W^T A over the same fixed gene chunks, one wave per
// (chunk, block, RQ-sample tile), RP = 16 rows -- only the live blocks' MFMA work, and many more, lighter
// workgroups than the 64-row tiles.  The accumulation is the canonical GTile K order, so the rows are
// bit-identical to every other shape.  Tile t == 0 of each (chunk, block) also forms the block's 16 x 16
// Gram block (nmf_mu.c:176); no restart crosses a block, so that is every Gram entry of its restarts.
// ---------------------------------------------------------------------------------------------
// Tile t == ntq of each (chunk, block) is the block's Gram item: its own wave runs the 16 x 16 W^T W block
// (P = Q = the block's W rows) beside the W^T A waves, instead of a W^T A wave carrying the Gram chain next
// to its own (that wave took 50 us where the others take 30).  A GTile MFMA with the same rows on both sides
// is the in-tile Gram MFMA operand for operand, in the same canonical K order: bit-identical partials.
template <int RQ, int NBUF, bool ABLK = false>
static __global__ __launch_bounds__(64) void k_wta_narrow(const double* __restrict__ W, const double* __restrict__ Acm,
                                                          long m_pad, int ntq, int nsplit, int kchunk, int nblk,
                                                          const ColInfo* __restrict__ ci, double* __restrict__ Gpart,
                                                          long g_ld, long g_split, double* __restrict__ SWpart,
                                                          long sw_total) {
  using T = GTile<16, RQ, 1, 1, NBUF, ABLK>;
  using TG = GTile<16, 16, 1, 1, NBUF, false>;
  static_assert(TG::LDS_BYTES <= T::LDS_BYTES, "the Gram item's ring fits the tile's");
  __shared__ __attribute__((aligned(1024))) char smem[T::LDS_BYTES];
  const int nt = ntq + 1;   // ntq W^T A tiles + the Gram item
  const int item = xcd_item(blockIdx.x, nsplit * nblk * nt);
  const int t = item % nt, bk = (item / nt) % nblk, s = item / (nt * nblk);
  const int kbeg = s * kchunk;
  const int kend = (int)min((long)kbeg + kchunk, m_pad);
  const int l = threadIdx.x, fr = l & 15, g = l >> 4;
  const double* Wb = W + (long)bk * 16 * m_pad + kbeg;
  if (t == ntq) {   // the Gram item
    TG tg;
    tg.zero();
    tg.run(Wb, m_pad, Wb, m_pad, 0, kend - kbeg, smem, [](const char*) {});
    double* so = SWpart + (long)s * sw_total;
    const ColInfo* cb = ci + (long)bk * 16;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int lr = g + 4 * reg, lcn = fr;
      const ColInfo cr = cb[lr];
      if (cr.k == 0 || cr.lc0 != cb[lcn].lc0 || cb[lcn].k == 0) continue;   // not the same restart
      const int a = lr - (cr.lc0 & 15), b = lcn - (cr.lc0 & 15);
      so[cr.sq_off + a * cr.k + b] = tg.acc[0][0][reg];
      so[cr.sq_off + b * cr.k + a] = tg.acc[0][0][reg];
    }
    return;
  }
  T tl;
  tl.zero();
  const long ldq = ABLK ? (long)ntq * RQ : m_pad;   // operands rebased to the chunk start (see k_wta2)
  const double* Q = ABLK ? Acm + (long)kbeg * ldq + (long)t * RQ * 16 : Acm + (long)t * RQ * m_pad + kbeg;
  tl.run(Wb, m_pad, Q, ldq, 0, kend - kbeg, smem, [](const char*) {});
  double* out = Gpart + (long)s * g_split + (long)bk * 16 * g_ld + (long)t * RQ;
#pragma unroll
  for (int nb = 0; nb < T::NB; ++nb)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) out[(long)T::row_of(0, reg) * g_ld + T::col_of(nb)] = tl.acc[0][nb][reg];
}

// Loader / consumer form of k_wta_narrow (round 4): the same items and the same canonical K order (GTile's
// load_frag / mfma_frag on the same stages), but two waves per item: wave 1 only issues the LDS-DMA stages and waits
// for them to land, wave 0 only reads fragments and issues the MFMA chain; they meet at one barrier per stage.  In the
// one-wave form the wave's in-order issue serialises each stage's four 1-KiB DMA pieces (~60 cycles of issue each)
// with its four dependent MFMAs (~64 cycles each): here the two run on two SIMDs at once.  Bit-identical results.
template <int RQ, int NBUF, bool ABLK = false>
static __global__ __launch_bounds__(128) void k_wta_narrow_lc(const double* __restrict__ W, const double* __restrict__ Acm,
                                                             long m_pad, int ntq, int nsplit, int kchunk, int nblk,
                                                             const ColInfo* __restrict__ ci, double* __restrict__ Gpart,
                                                             long g_ld, long g_split, double* __restrict__ SWpart,
                                                             long sw_total) {
  static_assert(RQ == 16, "the Gram item shares the tile type: RQ = 16");
  using T = GTile<16, RQ, 1, 1, NBUF, ABLK>;
  __shared__ __attribute__((aligned(1024))) char smem[T::LDS_BYTES];
  const int nt = ntq + 1;   // ntq W^T A tiles + the Gram item
  const int item = xcd_item(blockIdx.x, nsplit * nblk * nt);
  const int t = item % nt, bk = (item / nt) % nblk, s = item / (nt * nblk);
  const int kbeg = s * kchunk;
  const int kend = (int)min((long)kbeg + kchunk, m_pad);
  const int wave = wave_id(), l = threadIdx.x & 63, fr = l & 15, g = l >> 4;
  const bool gram = t == ntq;
  const double* Wb = W + (long)bk * 16 * m_pad + kbeg;
  const long ldq = gram ? m_pad : (ABLK ? (long)ntq * RQ : m_pad);   // operands rebased to the chunk start
  const double* Q = gram ? Wb : (ABLK ? Acm + (long)kbeg * ldq + (long)t * RQ * 16 : Acm + (long)t * RQ * m_pad + kbeg);
  const int nst = (kend - kbeg) / BK2;
  constexpr int D = NBUF - 1;
  const uint32_t base = (uint32_t)(uintptr_t)smem;
  T tl;
  tl.wo = wave;   // each wave is wave 0 of its own 1-wave tile view
  if (wave == 1) {
    // loader: the K-blocked A operand only for the W^T A items (the Gram item stages W rows on both sides)
    if (gram) {
      GTile<16, RQ, 1, 1, NBUF, false> tg;
      tg.wo = 1;
      tg.bind(Wb, m_pad, Q, ldq, kend - kbeg);
      const int npro = nst < D ? nst : D;
      for (int q = 0; q < npro; ++q) tg.issue(base + q * T::STAGE_BYTES, q * BK2);
      T::template wait_stages<D - 1, 0>(npro - 1, false);
      step_barrier();
      for (int st = 0; st + 1 < nst; ++st) {
        if (st + D < nst) tg.issue(base + ((st + D) % NBUF) * T::STAGE_BYTES, (st + D) * BK2);
        const int left = nst - st - 2;
        T::template wait_stages<D - 1, 0>(left < D - 1 ? left : D - 1, false);
        step_barrier();
      }
    } else {
      tl.bind(Wb, m_pad, Q, ldq, kend - kbeg);
      const int npro = nst < D ? nst : D;
      for (int q = 0; q < npro; ++q) tl.issue(base + q * T::STAGE_BYTES, q * BK2);
      T::template wait_stages<D - 1, 0>(npro - 1, false);
      step_barrier();
      for (int st = 0; st + 1 < nst; ++st) {
        if (st + D < nst) tl.issue(base + ((st + D) % NBUF) * T::STAGE_BYTES, (st + D) * BK2);
        const int left = nst - st - 2;
        T::template wait_stages<D - 1, 0>(left < D - 1 ? left : D - 1, false);
        step_barrier();
      }
    }
    return;
  }
  // consumer: GTile::run's split steps (kk = 1 MFMAs of stage st behind the barrier publishing stage st + 1)
  tl.zero();
  step_barrier();
  typename T::Frag f0, f1;
  int b = 0;
  tl.load_frag(smem, 0, f0);
  for (int st = 0; st + 1 < nst; ++st) {
    const char* cur = smem + b * T::STAGE_BYTES;
    tl.load_frag(cur, 1, f1);
    tl.mfma_frag(f0);
    const int bn = (b + 1 == NBUF) ? 0 : b + 1;
    __builtin_amdgcn_sched_barrier(0);
    step_barrier();
    tl.load_frag(smem + bn * T::STAGE_BYTES, 0, f0);
    __builtin_amdgcn_sched_barrier(0);
    tl.mfma_frag(f1);
    b = bn;
  }
  {
    const char* cur = smem + b * T::STAGE_BYTES;
    tl.load_frag(cur, 1, f1);
    tl.mfma_frag(f0);
    tl.mfma_frag(f1);
  }
  if (gram) {
    double* so = SWpart + (long)s * sw_total;
    const ColInfo* cb = ci + (long)bk * 16;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int lr = g + 4 * reg, lcn = fr;
      const ColInfo cr = cb[lr];
      if (cr.k == 0 || cr.lc0 != cb[lcn].lc0 || cb[lcn].k == 0) continue;   // not the same restart
      const int a = lr - (cr.lc0 & 15), bb = lcn - (cr.lc0 & 15);
      so[cr.sq_off + a * cr.k + bb] = tl.acc[0][0][reg];
      so[cr.sq_off + bb * cr.k + a] = tl.acc[0][0][reg];
    }
    return;
  }
  double* out = Gpart + (long)s * g_split + (long)bk * 16 * g_ld + (long)t * RQ;
#pragma unroll
  for (int nb = 0; nb < T::NB; ++nb)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) out[(long)T::row_of(0, reg) * g_ld + T::col_of(nb)] = tl.acc[0][nb][reg];
}

}  // namespace nmfc
