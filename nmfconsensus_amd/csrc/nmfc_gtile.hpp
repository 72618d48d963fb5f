// nmfc_gtile.hpp -- the GTile core: the LDS-DMA-staged fp64 MFMA tile of W^T A and A h^T.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmfc_common.hpp"
#include "nmfc_tuning.hpp"

namespace nmfc {

// ---------------------------------------------------------------------------------------------
// GTile: the LDS-DMA-staged MFMA tile (v2 core).  RP x RQ outputs over NW waves (WR x WC), K in
// stages of BK2 = 16 doubles (one 128 B row per tile row per stage) in a ring of 3 LDS buffers filled
// by buffer_load ... lds (16 B per lane, no VGPR round trip).  A stage is issued two steps ahead; each
// step ends with ONE counted vmcnt wait + a raw s_barrier, so the next stage's DMA stays in flight
// across it.  LDS image: row r at r*128 B, logical 16-byte slot s stored at physical slot
// s ^ ((r >> 1) & 7) -- the swizzle is applied on the per-lane SOURCE address (the DMA destination is
// lane-linear) and on the fragment reads; it makes the ds_read_b128 fragment reads conflict-free.
// Canonical K order (a function of the 16-aligned K block only): MFMA j = 2*kk + sub (kk, sub in
// {0,1}) consumes k = 8*kk + sub + 2*g for lane group g = 0..3.  Every GTile shape uses this order, so
// results are bit-identical across tile shapes (the tail variants) and batch compositions.
// ---------------------------------------------------------------------------------------------
constexpr int BK2 = 16;
constexpr int GT_NBUF = 3;
constexpr bool GT_PRIO = NMFC_GT_PRIO != 0;   // raise the wave priority around each MFMA block (experiment)

__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t r, uint32_t lds_addr, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)(uintptr_t)lds_addr, 16, voff,
                                           soff, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void step_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// QBLK: the Q operand is K-blocked ([K/16][rows][16] doubles: one 16-gene block of every row
// contiguous, `ldq` = the total row count), so a stage of a tile is ONE contiguous RQ x 128 B run instead
// of RQ rows 8 * ldq bytes apart.  The same canonical K order either way.
// GREG: the wave may also accumulate one 16 x 16 Gram block of its own P rows -- row block `gi` against row block
// `gj` of its MB row blocks (gj = gi: a restart-diagonal block; gj = gi + 1: a block straddled by a restart) -- into
// `gacc`: W^T W from the W fragments already in registers for the tile MFMAs (the A operand lane map (row fr, k g)
// and the B operand map (k g, col fr) hold the same value for P = Q), in the canonical K order; gi < 0: none.
// SPLIT (NBUF >= 3): the split-step form (below); false: each step computes its whole stage between the barriers
// (one fragment set live instead of two: 24 VGPRs fewer at MB = 4, NB = 2, for the 16-wave tile).  Same order of
// accumulation either way (kk = 0 then kk = 1 of every stage), so the same bits.
// OPQ: the lane index comes from an opaque copy taken in bind() (per run), not from threadIdx.x: inside an outer loop
// (k_wta2_sk's pieces) the lane-derived offsets then stay inside each run instead of being hoisted out of the outer
// loop and held across every K loop.  The same values, the same code in the loop.
template <int RP, int RQ, int WR, int WC, int NBUF = GT_NBUF, bool QBLK = false, bool GREG = false, bool SPLIT = true,
          bool OPQ = false>
struct GTile {
  static_assert(NBUF >= 2 && NBUF <= 16, "ring of 2..16 stages");
  static constexpr int NW = WR * WC;
  static constexpr int NTH = NW * 64;
  static constexpr int STAGE_BYTES = (RP + RQ) * BK2 * 8;
  static constexpr int LDS_BYTES = NBUF * STAGE_BYTES;
  static constexpr int PIECES = (RP + RQ) / 8;   // 1 KiB DMA pieces (8 rows) per stage
  static constexpr int PPW = PIECES / NW;        // pieces per wave per stage
  static constexpr int PPW_P = RP / 8 / NW;      // of which rows of P
  static_assert(PIECES % NW == 0 && (RP / 8) % NW == 0, "pieces must split evenly over waves");
  static constexpr int MB = RP / WR / 16;
  static constexpr int NB = RQ / WC / 16;
  static_assert(!GREG || NBUF >= 3, "register Gram on the split-step ring only");

  d4 acc[MB][NB];
  d4 gacc;
  int gi = -1, gj = -1;   // GREG: wave-uniform
  __amdgpu_buffer_rsrc_t rp, rq;
  int voff[PPW];
  int qkm;
  int tix = 0;  // OPQ: the opaque lane index (bind)
  int wo = 0;   // wave offset: this tile's waves are wo .. wo + NW - 1 of the workgroup (several 1-wave tiles per workgroup)   // QBLK: bytes between consecutive K positions' blocks / 8 (= 8 * total rows); else 8

  // P rows are K-contiguous at P + row*ldp, Q rows at Q + row*ldq (doubles); QBLK: Q + (k/16)*16*ldq + row*16
  __device__ __forceinline__ int lane_ix() const { return OPQ ? tix : (int)(threadIdx.x & 63); }
  __device__ __forceinline__ void bind(const double* P, long ldp, const double* Q, long ldq, int kend) {
    if constexpr (OPQ) {
      tix = lane_id();
      asm volatile("" : "+v"(tix));
    }
    const int w = wave_id() - wo, l = lane_ix();
    rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(P), 0, (int)(RP * ldp * 8), 0x00020000);
    rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(Q), 0, QBLK ? (int)((long)kend * ldq * 8) : (int)(RQ * ldq * 8),
                                           0x00020000);
    qkm = QBLK ? (int)ldq * 8 : 8;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int piece = w + NW * i;
      const bool isq = i >= PPW_P;
      const int row = (isq ? piece - RP / 8 : piece) * 8 + (l >> 3);
      const int slot = (l & 7) ^ ((row >> 1) & 7);
      voff[i] = (int)((long)row * (isq ? (QBLK ? 16 : ldq) : ldp) * 8 + slot * 16);
    }
  }

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
    gacc = (d4){0.0, 0.0, 0.0, 0.0};
  }

  // DMA of the stage starting at K position k0 into the LDS buffer at byte address `buf`
  __device__ __forceinline__ void issue(uint32_t buf, int k0) const {
#pragma unroll
    for (int i = 0; i < PPW; ++i) issue_piece(buf, k0, i);
  }
  // piece i of this wave (the wave index is wave-uniform: read into an SGPR so M0 is scalar arithmetic)
  __device__ __forceinline__ void issue_piece(uint32_t buf, int k0, int i) const {
    const int w = wave_id() - wo;
    const uint32_t dst = buf + (uint32_t)(w + NW * i) * 1024u;
    if (i >= PPW_P)
      lds_dma16(rq, dst, voff[i], k0 * qkm);
    else
      lds_dma16(rp, dst, voff[i], k0 * 8);
  }

  // byte offset of (row, logical slot) in a stage
  __device__ __forceinline__ static uint32_t off(int row, int slot) {
    return (uint32_t)(row * 128 + ((slot ^ ((row >> 1) & 7)) << 4));
  }

  // the split form of compute(): fragments of one kk half of a stage, then its MFMAs
  struct Frag {
    d2 a[MB], b[NB];
  };
  __device__ __forceinline__ void load_frag(const char* __restrict__ st, int kk, Frag& f) const {
    const int w = wave_id() - wo, l = lane_ix();
    const int wr = w / WC, wc = w % WC;
    const int fr = l & 15, g = l >> 4;
    const char* sp = st + (wr * (RP / WR) + fr) * 128;
    const char* sq = st + RP * 128 + (wc * (RQ / WC) + fr) * 128;
    const int so = ((4 * kk + g) ^ (fr >> 1)) << 4;
#pragma unroll
    for (int i = 0; i < MB; ++i) f.a[i] = *reinterpret_cast<const d2*>(sp + i * 16 * 128 + so);
#pragma unroll
    for (int j = 0; j < NB; ++j) f.b[j] = *reinterpret_cast<const d2*>(sq + j * 16 * 128 + so);
  }
  // GC: the wave's register Gram block.  GC_DYN: chosen at run time by gi (diagonal blocks only, a VGPR select of the
  // fragment); -1: none; gi * 4 + gj: fixed at compile time (a K-loop instantiation per block: no selects, no branches)
  static constexpr int GC_DYN = -2;
  template <int GC = GC_DYN>
  __device__ __forceinline__ void mfma_frag(const Frag& f) {
    if constexpr (GT_PRIO) __builtin_amdgcn_s_setprio(1);
    mfma_frag_body<GC>(f);
    if constexpr (GT_PRIO) __builtin_amdgcn_s_setprio(0);
  }
  template <int GC = GC_DYN>
  __device__ __forceinline__ void mfma_frag_body(const Frag& f) {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.a[i].x, f.b[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.a[i].y, f.b[j].y, acc[i][j], 0, 0, 0);
    if constexpr (GREG && GC >= 0) {
      constexpr int i = GC >> 2, j = GC & 3;
      static_assert(i < MB && j < MB, "Gram block inside the wave's rows");
      gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.a[i].x, f.a[j].x, gacc, 0, 0, 0);
      gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.a[i].y, f.a[j].y, gacc, 0, 0, 0);
    } else if constexpr (GREG && GC == GC_DYN) {
      if (gi >= 0) {
        d2 v = f.a[0];
#pragma unroll
        for (int i = 1; i < MB; ++i)
          if (gi == i) v = f.a[i];
        gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(v.x, v.x, gacc, 0, 0, 0);
        gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(v.y, v.y, gacc, 0, 0, 0);
      }
    }
  }
  template <int NKK = 2>
  __device__ __forceinline__ void compute(const char* __restrict__ st) {
    const int w = wave_id() - wo, l = threadIdx.x & 63;
    const int wr = w / WC, wc = w % WC;
    const int fr = l & 15, g = l >> 4;
    const char* sp = st + (wr * (RP / WR) + fr) * 128;
    const char* sq = st + RP * 128 + (wc * (RQ / WC) + fr) * 128;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      const int so = ((4 * kk + g) ^ (fr >> 1)) << 4;
      d2 a[MB], b[NB];
#pragma unroll
      for (int i = 0; i < MB; ++i) a[i] = *reinterpret_cast<const d2*>(sp + i * 16 * 128 + so);
#pragma unroll
      for (int j = 0; j < NB; ++j) b[j] = *reinterpret_cast<const d2*>(sq + j * 16 * 128 + so);
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
    }
  }

  // the pipelined K loop over [kbeg, kend) (multiple of BK2); `extra(stage_ptr)` runs after each
  // stage's MFMAs on the same staged data.  smem: GT_NBUF * STAGE_BYTES bytes.
  template <class Extra>
  __device__ __forceinline__ void run(const double* __restrict__ P, long ldp, const double* __restrict__ Q, long ldq,
                                      int kbeg, int kend, char* __restrict__ smem, Extra extra) {
    run(P, ldp, Q, ldq, kbeg, kend, smem, extra, [] {});
  }

  // as above with `at_last()`: a place to issue the epilogue's own XL global loads early (see below)
  // NBUF == 2: `at_last()` runs right after the last DMA issue and may issue XL vector-memory
  // operations of its own; the one wait that follows leaves those XL in flight.
  template <int XL = 0, class Extra, class AtLast>
  __device__ __forceinline__ void run(const double* __restrict__ P, long ldp, const double* __restrict__ Q, long ldq,
                                      int kbeg, int kend, char* __restrict__ smem, Extra extra, AtLast at_last) {
    (void)run<XL>(P, ldp, Q, ldq, kbeg, kend, smem, [] { return true; }, extra, at_last);
  }

  // with `pre()`: runs right after the prologue's first DMA issue, so the workgroup's own setup loads
  // overlap the first stages' latency; returning false abandons the tile (the DMA is drained first)
  // and run returns false.  All waves must return the same answer.
  // LASTKK (NBUF == 2) = 1: the last stage's second half (K positions 8..15) holds zeros in both operands (the K
  // padding) and is skipped -- adding exact zeros to sums of non-negative products would change no bit.
  template <int XL = 0, int LASTKK = 2, int GC = GC_DYN, class Pre, class Extra, class AtLast>
  __device__ __forceinline__ bool run(const double* __restrict__ P, long ldp, const double* __restrict__ Q, long ldq,
                                      int kbeg, int kend, char* __restrict__ smem, Pre pre, Extra extra, AtLast at_last) {
    static_assert(LASTKK == 2 || NBUF == 2, "half last stage on the two-stage ring only");
    const int nst = (kend - kbeg) / BK2;
    bind(P, ldp, Q, ldq, kend);
    const uint32_t base = (uint32_t)(uintptr_t)smem;
    if constexpr (NBUF == 2) {   // one stage in flight, issued after the barrier that freed its buffer
      issue(base, kbeg);
      if (!pre()) {
        wait_vmcnt<0>();
        return false;
      }
      wait_vmcnt<0>();
      step_barrier();
      if (nst == 1) at_last();
      for (int s = 0; s + 1 < nst; ++s) {
        const int b = s & 1;
        issue(base + (b ^ 1) * STAGE_BYTES, kbeg + (s + 1) * BK2);
        if (s + 2 == nst) at_last();
        const char* cur = smem + b * STAGE_BYTES;
        compute(cur);
        extra(cur);
        if (s + 2 == nst)
          wait_vmcnt<XL>();
        else
          wait_vmcnt<0>();
        step_barrier();
      }
      {   // last step
        const char* cur = smem + ((nst - 1) & 1) * STAGE_BYTES;
        compute<LASTKK>(cur);
        extra(cur);
      }
      return true;
    }
    // NBUF >= 3: a ring of NBUF stages with D = NBUF - 1 stages in flight; stage s + D is issued at step
    // s into the buffer that stage s - 1 freed (every wave passed the barrier after computing it).
    // `at_last()` runs right after the LAST DMA issue and may issue XL vector-memory operations; every
    // later wait leaves those XL in flight.  After step s the wait leaves min(D - 1, nst - s - 2) stages
    // in flight (each PPW pieces per wave), so stage s + 1 has landed for this wave; the barrier makes
    // it landed for all waves.
    constexpr int D = NBUF - 1;
    static_assert(PPW * (D - 1) + XL <= 63, "vmcnt holds at most 63 outstanding operations");
    const int npro = nst < D ? nst : D;
    bool xl = false;
    for (int q = 0; q < npro; ++q) issue(base + q * STAGE_BYTES, kbeg + q * BK2);
    if (!pre()) {
      wait_vmcnt<0>();
      return false;
    }
    if (nst <= D) {
      at_last();
      xl = true;
    }
    wait_stages<D - 1, XL>(npro - 1, xl);
    step_barrier();
    int b = 0;
    // split steps: the kk = 1 MFMAs of stage s are issued AFTER the barrier that publishes stage s + 1,
    // right behind the LDS reads of stage s + 1's kk = 0 fragments, so those reads (and the barrier) are
    // covered by matrix work instead of leaving the pipe idle at every step.  Each accumulator still sees
    // kk = 0 (x, y) then kk = 1 (x, y) of every stage in order: the same sums bit for bit.
    // (the last step is peeled: no branch around the barrier, so the compiler's lgkmcnt for the kk = 1
    // fragments leaves the next stage's reads in flight)
    if constexpr (!SPLIT) {
      for (int s = 0; s < nst; ++s) {
        const char* cur = smem + b * STAGE_BYTES;
        if (s + D < nst) {
          const int bd = (b + D >= NBUF) ? b + D - NBUF : b + D;
          issue(base + bd * STAGE_BYTES, kbeg + (s + D) * BK2);
          if (s + D + 1 == nst) {
            at_last();
            xl = true;
          }
        }
        Frag f;
        load_frag(cur, 0, f);
        mfma_frag<GC>(f);
        load_frag(cur, 1, f);
        mfma_frag<GC>(f);
        extra(cur);
        if (s + 1 < nst) {
          const int left = nst - s - 2;
          wait_stages<D - 1, XL>(left < D - 1 ? left : D - 1, xl);
          step_barrier();
        }
        b = (b + 1 == NBUF) ? 0 : b + 1;
      }
      return true;
    }
    Frag f0, f1;
    load_frag(smem, 0, f0);
    for (int s = 0; s + 1 < nst; ++s) {
      const char* cur = smem + b * STAGE_BYTES;
      // the stage's DMA pieces go out as one block at the step head (spreading them one by one between the
      // MFMAs was measured 2 % slower on both contractions: the data then lands later)
      if (s + D < nst) {
        const int bd = (b + D >= NBUF) ? b + D - NBUF : b + D;
        issue(base + bd * STAGE_BYTES, kbeg + (s + D) * BK2);
        if (s + D + 1 == nst) {
          at_last();
          xl = true;
        }
      }
      load_frag(cur, 1, f1);
      mfma_frag<GC>(f0);
      extra(cur);
      const int bn = (b + 1 == NBUF) ? 0 : b + 1;
      const int left = nst - s - 2;
      __builtin_amdgcn_sched_barrier(0);   // the kk = 1 MFMAs stay behind the barrier and the next reads
      wait_stages<D - 1, XL>(left < D - 1 ? left : D - 1, xl);
      step_barrier();   // also: every wave has read stage s (its kk = 1 fragments are in registers)
      load_frag(smem + bn * STAGE_BYTES, 0, f0);
      __builtin_amdgcn_sched_barrier(0);
      mfma_frag<GC>(f1);
      b = bn;
    }
    {   // last step (its DMA was issued D steps ago)
      const char* cur = smem + b * STAGE_BYTES;
      load_frag(cur, 1, f1);
      mfma_frag<GC>(f0);
      extra(cur);
      mfma_frag<GC>(f1);
    }
    return true;
  }

  // s_waitcnt vmcnt(PPW * j + (xl ? XL : 0)) for a wave-uniform j in [0, J] (the count is an immediate)
  template <int J, int XL>
  __device__ __forceinline__ static void wait_stages(int j, bool xl) {
    if (j >= J) {
      if (xl)
        wait_vmcnt<PPW * J + XL>();
      else
        wait_vmcnt<PPW * J>();
    } else if constexpr (J > 0) {
      wait_stages<J - 1, XL>(j, xl);
    }
  }

  // C/D map of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  __device__ __forceinline__ static int row_of(int mb, int reg) {
    const int w = wave_id(), l = lane_id();
    return (w / WC) * (RP / WR) + mb * 16 + (l >> 4) + 4 * reg;
  }
  __device__ __forceinline__ static int col_of(int nb) {
    const int w = wave_id(), l = lane_id();
    return (w % WC) * (RQ / WC) + nb * 16 + (l & 15);
  }
};

// A panel takes part when one of its restarts is still running, or (for the W update) stopped at
// exactly this iteration.  [prb[p], pre[p]) is the panel's range in the active restart list.
__device__ __forceinline__ bool panel_live(const int* __restrict__ prb, const int* __restrict__ pre, int p,
                                           const RestartInfo* __restrict__ ri, const int* __restrict__ stop_iter,
                                           int iter) {
  const int b = prb[p], e = pre[p];
  for (int q = b; q < e; ++q) {
    const int s = stop_iter[ri[q].rid];
    if (s == 0 || s == iter) return true;
  }
  return false;
}

}  // namespace nmfc
