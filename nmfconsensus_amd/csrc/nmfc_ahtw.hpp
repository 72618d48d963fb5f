// nmfc_ahtw.hpp -- k_ahtw4: A h^T fused with W0 (h h^T) and the W rule, on the GTile core.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmfc_gtile.hpp"

namespace nmfc {

constexpr bool AHTW_KSKIP = NMFC_AHTW_KSKIP != 0;   // A h^T: skip the K-padding half of the last stage (KHALF)

// ---------------------------------------------------------------------------------------------
// Item map of the A h^T kernels: (panel, gene tile) from the XCD-contiguous item index.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void ahtw_map(int item, int npanels, int ngt, int& p, int& gt) {
  // bands of SP panels, gene super-tiles of SG: neighbours share operands in L2
  const int SP = NMFC_AHTW_SP, SG = NMFC_AHTW_SG;
  const int band = item / (SP * ngt);
  const int rem = item % (SP * ngt);
  const int bp = min(SP, npanels - band * SP);
  const int sg = rem / (bp * SG);
  const int gsz = min(SG, ngt - sg * SG);
  const int w2 = rem - sg * bp * SG;
  p = band * SP + w2 / gsz;
  gt = ngt - 1 - (sg * SG + w2 % gsz);   // high gene tiles first: W^T A streamed them last
}

// ---------------------------------------------------------------------------------------------
// K3 v4 "ahtw4": F = A h^T on the GTile ring (NPT panels x GTG genes, 4 waves per panel: WR = NPT,
// WC = 4, each wave 64 panel rows x GTG/4 genes) + the panels' h h^T rows in LDS.  Engine default (LATE,
// NBUF = 2, GTG = 128): a 2 x 24 KiB ring and 160 VGPRs, so THREE workgroups share a CU and their K loops
// cover each other's prologues and epilogues (MFMA busy 75.5 -> 80.2 % at full load, +4.5 % kernel rate
// over the 3-stage, 80 KiB, two-per-CU form); the h h^T rows wait in registers until the loop is done,
// and W0 streams in by 16-row blocks during the epilogue.  Column state lives in registers: each wave reads its
// panel's 64 ColInfo entries (lane = column), the active set is a 64-bit ballot of colact[c] == iter
// (k_hupdate stamps its restart's columns with the iteration it ran) and the E-operand rows' (lc0, k)
// come by lane shuffles.  These setup loads are issued after the first DMA stages, so they overlap
// them.  The h h^T rows are read from SHP (panel-row layout written by k_hupdate), one coalesced
// block.  W0 is loaded in the D layout right after the last DMA issue and is the B operand of
// E = W0 (h h^T) directly.
// ---------------------------------------------------------------------------------------------
// GTG: genes per tile (128 at full load; 64 for small grids: half the MFMA chain per wave, twice the
// workgroups).  ngt = m_pad / GTG; npanels is a multiple of NPT.  Every shape accumulates in the
// canonical GTile K order.
// PR = 16 is the narrow (tail) form: only the first 16 columns of panel 0 are live, so the tile covers
// those 16 rows (WC waves along the genes): a quarter of the H / W bytes and MFMA work per gene tile.
// LATE: the h h^T rows stay in registers through the K loop and are staged afterwards into a ring buffer
// the last step no longer reads, and W0 is loaded after the loop: no LDS beyond the ring and no W0
// registers live in the loop, so more workgroups fit a CU (their K loops cover each other's epilogues).
template <int GTG = GT, int NBUF = GT_NBUF, int NPT = 1, int PR = PANEL, int WC = 4, bool LATE = false>
static constexpr int ahtw4_lds() {
  return GTile<PR * NPT, GTG, NPT, WC, NBUF>::LDS_BYTES + (LATE ? 0 : NPT * PR * KMAX * 8);
}
// KHALF: the last K stage's second half is padding (n_pad - n >= 8, decided on the host): skipped.
// RULE_EUCLID: euclid_rule_w instead of mu_rule_sel.  That rule has no zero guard, so a padded gene row (gene >= m,
// all of old, num and den zero) would become 0 * 0 / 0 + eps = NaN and poison W^T W: the epilogue masks by the gene
// index (the kernel receives m beside ngt) and writes +0.0 there; a real row follows the rule whatever it holds.
// A real row can therefore turn NaN (a zero column of a caller's W0), and E = W0 (h h^T) would hand that NaN to the
// other restarts of its 16-column block as 0 x NaN: a block whose W0 holds a non-finite value takes a path of its own
// in the epilogue, restart by restart, that gives every restart the bits it has alone.
// RULE_NEALS (nmf_neals, DESIGN.md "NEALS"): the K loop alone.  The epilogue reads neither W0 nor the h h^T rows and
// stores the raw product H A^T of the active columns (+0.0 in padded gene rows) into the buffer passed as W, which the
// engine points at a scratch matrix: k_wsolve_neals solves S y = c from it and writes the real W.
template <int GTG = GT, int NBUF = GT_NBUF, int NPT = 1, int PR = PANEL, int WC = 4, bool LATE = false, bool KHALF = false,
          int RULE = RULE_MU>
static __global__ __launch_bounds__(64 * NPT * WC,
                                    (163840 / ahtw4_lds<GTG, NBUF, NPT, PR, WC, LATE>()) * NPT * WC / 4 > 8
                                        ? 8
                                        : (163840 / ahtw4_lds<GTG, NBUF, NPT, PR, WC, LATE>()) * NPT * WC / 4)
void k_ahtw4(int iter, const double* __restrict__ H, long n_pad, const double* __restrict__ Arm, long m_pad,
             double* __restrict__ W, const double* __restrict__ SHP, const ColInfo* __restrict__ ci,
             const int* __restrict__ colact, int npanels, typename RuleArgs<RULE>::Tiles tiles) {
  const int ngt = ngt_of(tiles);
  using TileW4 = GTile<PR * NPT, GTG, NPT, WC, NBUF>;
  constexpr int AHTW4_SH = TileW4::LDS_BYTES;
  constexpr int AHTW4_LDS = ahtw4_lds<GTG, NBUF, NPT, PR, WC, LATE>();
  static_assert(AHTW4_LDS <= 163840, "LDS of one CU");
  static_assert(PR == PANEL || (PR == 16 && NPT == 1), "narrow tiles: one 16-column block");
  static_assert(!LATE || TileW4::STAGE_BYTES >= NPT * PR * KMAX * 8, "h h^T rows fit one ring stage");
  constexpr int NTH = 64 * NPT * WC;
  __shared__ __attribute__((aligned(1024))) char smem[AHTW4_LDS];
  double* SHl = reinterpret_cast<double*>(smem + AHTW4_SH);   // !LATE; LATE: set after the K loop
  int pp, gt;
  ahtw_map(xcd_item(blockIdx.x, (npanels / NPT) * ngt), npanels / NPT, ngt, pp, gt);
  const int p0 = pp * NPT;   // first panel of the tile
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), wr = w / WC, wc = w % WC;
  const int p = p0 + wr;     // this wave's panel
  ColInfo cc;
  uint64_t actmask = 0;
  TileW4 tl;
  tl.zero();
  // PR = 16: the "panel" index p is a 16-column block (column 16 p of the stacked W / H).
  // W0 loads and W stores through a buffer resource over this wave's W rows: one 32-bit lane offset, the
  // (row block, nb) part wave-uniform in soffset -- no 64-bit row addresses held in VGPRs across the K loop
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      W + (long)p * PR * m_pad + (long)gt * GTG + (GTG / WC) * wc, 0, (int)(PR * m_pad * 8), 0x00020000);
  const int wvoff = (int)(((lane >> 4) * m_pad + (lane & 15)) * 8);
  auto woff = [&](int mb, int reg, int nb) { return (int)(((16 * mb + 4 * reg) * m_pad + 16 * nb) * 8); };
  double w0[TileW4::MB][TileW4::NB][4];
  auto load_w0_block = [&](int mb) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
#pragma unroll
      for (int nb = 0; nb < TileW4::NB; ++nb)
        w0[mb][nb][reg] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rw, wvoff, woff(mb, reg, nb), 0));
  };
  auto load_w0 = [&] {
#pragma unroll
    for (int mb = 0; mb < TileW4::MB; ++mb) load_w0_block(mb);
  };
  constexpr int NSH = NPT * PR * KMAX / 2 / NTH;
  static_assert(NSH * 2 * NTH == NPT * PR * KMAX, "h h^T rows split evenly over the threads");
  d2 shv[NSH];
  // W0 blocks 0 and 1 go out with the last K stage's DMA (EARLY, the 2-stage LATE form): their latency is covered by
  // the last step's MFMAs instead of opening the epilogue (round 5: +2 % at full load, tools/kvar.hip form EW)
  constexpr bool EARLY = LATE && NBUF == 2 && TileW4::MB >= 2;
  constexpr bool NE = RULE == RULE_NEALS;
  constexpr int XL = NE ? 0 : LATE ? (EARLY ? 2 * TileW4::NB * 4 : 0) : TileW4::MB * TileW4::NB * 4;
  const bool live = tl.template run<XL, KHALF ? 1 : 2>(
      H + (long)p0 * PR * n_pad, n_pad, Arm + (long)gt * GTG * n_pad, n_pad, 0, (int)n_pad, smem,
      [&] {   // setup loads, independent of each other, overlapping the first stages' DMA
        cc = lane < PR ? ci[(long)p * PR + lane] : ColInfo{0, 0, 0, 0};
        int ca[NPT];
#pragma unroll
        for (int q = 0; q < NPT; ++q) ca[q] = lane < PR ? colact[(long)(p0 + q) * PR + lane] : -1;
        if constexpr (!NE) {
          const d2* src = reinterpret_cast<const d2*>(SHP + (long)p0 * PR * KMAX);
#pragma unroll
          for (int j = 0; j < NSH; ++j) shv[j] = src[tid + NTH * j];
        }
        bool any = false;
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
          const uint64_t mk = __ballot(ca[q] == iter);   // the column's restart ran k_hupdate at this iteration
          if (q == wr) actmask = mk;
          any = any || mk != 0;
        }
        if (!any) return false;   // every panel of the tile idle (the same answer in every wave)
        if constexpr (!LATE && !NE) {
#pragma unroll
          for (int j = 0; j < NSH; ++j) reinterpret_cast<d2*>(SHl)[tid + NTH * j] = shv[j];
        }
        return true;   // SHl is published by the ring prologue's barrier
      },
      [](const char*) {},
      [&] {
        if constexpr (!LATE && !NE) load_w0();
        if constexpr (EARLY && !NE) {
          load_w0_block(0);
          load_w0_block(1);
        }
      });
  if (!live) return;
  if constexpr (NE) {
    if (actmask == 0) return;   // this wave's panel is idle
#pragma unroll
    for (int mb = 0; mb < TileW4::MB; ++mb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int c = 16 * mb + (lane >> 4) + 4 * reg;
        if (!((actmask >> c) & 1)) continue;
#pragma unroll
        for (int nb = 0; nb < TileW4::NB; ++nb) {
          const int gene = gt * GTG + (GTG / WC) * wc + 16 * nb + (lane & 15);
          const double v = gene < tiles.m ? tl.acc[mb][nb][reg] : 0.0;
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rw, wvoff, woff(mb, reg, nb), 0);
        }
      }
    return;
  }
  if constexpr (LATE) {
    // the ring buffer of stage nst - 2: every wave passed the barrier after reading it (nst >= 2)
    const int nst = (int)n_pad / BK2;
    SHl = reinterpret_cast<double*>(smem + ((nst - 2) % NBUF) * TileW4::STAGE_BYTES);
#pragma unroll
    for (int j = 0; j < NSH; ++j) reinterpret_cast<d2*>(SHl)[tid + NTH * j] = shv[j];
    // W0 by 16-row blocks, one block ahead of the epilogue's block loop (block mb's E reads blocks
    // mb - 1 .. mb + 1 only), so at most three blocks are live at once
    if constexpr (!EARLY) {
#pragma unroll
      for (int mb = 0; mb < (TileW4::MB < 2 ? TileW4::MB : 2); ++mb) load_w0_block(mb);
    }
  }
  // Block-aligned restarts (the engine's 16-column block packing: no active restart crosses a 16-column block) take
  // E over the four K steps of their own block, no shuffles for its K range; the K steps the restarts do not cover
  // add exact zeros (0 x finite W0), so the bits are those of the general form, which stays for any other packing.
  const bool cross = ((actmask >> lane) & 1) && ((cc.lc0 & (PR - 1)) >> 4) != (((cc.lc0 & (PR - 1)) + cc.k - 1) >> 4);
  const bool aligned = __ballot(cross) == 0;   // wave-uniform
  if constexpr (LATE) __syncthreads();
  if (actmask == 0) return;   // this wave's panel is idle (its partner panel is not)
  const double* SHw = SHl + (long)wr * PR * KMAX;
#pragma unroll
  for (int mb = 0; mb < TileW4::MB; ++mb) {
    if constexpr (LATE) {
      if (mb + 2 < TileW4::MB) load_w0_block(mb + 2);
    }
    const int ra = 16 * mb + (lane & 15);
    const int alc = __shfl(cc.lc0, ra) & (PR - 1);   // tile-local (a restart never straddles a tile)
    const int ak = ((actmask >> ra) & 1) ? __shfl(cc.k, ra) : 0;
    if constexpr (RULE == RULE_EUCLID) {
      // E below multiplies every W0 column of its K steps into every row and relies on 0 x finite = 0 outside a row's
      // own restart.  This rule has no guard, so a restart can hold NaN or Inf (a caller's zero column of W0 gives
      // 0 / 0), live or stopped, and 0 x NaN would hand it to every restart of the block.  When a K step holds a
      // non-finite W0, the block is done restart by restart instead, the other restarts' columns of W0 masked to 0.0: the
      // same K steps in the same order with zeros for zeros, so a finite restart keeps its bits and a non-finite one
      // gets R's IEEE result.
      bool nonfin = false;
#pragma unroll
      for (int b2 = 0; b2 < TileW4::MB; ++b2) {
        if (b2 < mb - 1 || b2 > mb + 1 || (aligned && b2 != mb)) continue;   // the blocks E reads
#pragma unroll
        for (int nb = 0; nb < TileW4::NB; ++nb)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            nonfin |= __builtin_amdgcn_class(w0[b2][nb][reg], 0x207);   // NaN or +-Inf
      }
      if (__ballot(nonfin) != 0) {   // wave-uniform
#pragma unroll 1
        for (int x = 0; x < 16; ++x) {   // the restarts with a column in block mb, by their first column in it
          const int col = 16 * mb + x;
          const int st = __builtin_amdgcn_readfirstlane(__shfl(cc.lc0, col)) & (PR - 1);
          const int kk = __builtin_amdgcn_readfirstlane(__shfl(cc.k, col));
          if (kk == 0 || (st != col && x != 0) || !((actmask >> col) & 1)) continue;
          // opaque copies: nothing of this loop is computed ahead of it and held in registers across the tile's hot path
          // (without them LICM hoists old * num and the row tests of all four registers, and the 64-gene form, which
          // sits on its 96-VGPR cap, spills into the K loop).  They only steer register allocation;
          // tests/test_euclid_resources.py compiles this file and fails on a spill, on scratch or on fewer waves per
          // SIMD than the nmf_mu form has (hipcc of ROCm 7.2, clang 22: 158 / 96 / 48 VGPRs for the 128-, 64-gene and narrow forms).
          int l4 = lane >> 4;
          asm volatile("" : "+v"(l4));
#pragma unroll
          for (int nb = 0; nb < TileW4::NB; ++nb) {
            d4 t = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = (4 * mb - 4 > 0 ? 4 * mb - 4 : 0); q < (4 * mb + 8 < 4 * TileW4::MB ? 4 * mb + 8 : 4 * TileW4::MB); ++q) {
              if (4 * q + 3 < st || 4 * q >= st + kk) continue;   // wave-uniform
              const int ck = 4 * q + l4;                          // the K step's column of this lane
              const bool own = ck >= st && ck < st + kk;
              const double sv = (own && alc == st) ? SHw[ra * KMAX + ck - st] : 0.0;
              const double bv = own ? w0[q >> 2][nb][q & 3] : 0.0;
              t = __builtin_amdgcn_mfma_f64_16x16x4f64(sv, bv, t, 0, 0, 0);
            }
            const int gene = gt * GTG + (GTG / WC) * wc + 16 * nb + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int c = 16 * mb + l4 + 4 * reg;
              if (c < st || c >= st + kk) continue;
              double old = w0[mb][nb][reg];
              asm volatile("" : "+v"(old));
              const double v = gene < tiles.m ? euclid_rule_w(old, tl.acc[mb][nb][reg], t[reg]) : 0.0;
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rw, wvoff, woff(mb, reg, nb), 0);
            }
          }
        }
        continue;
      }
    }
    d4 e[TileW4::NB];
#pragma unroll
    for (int nb = 0; nb < TileW4::NB; ++nb) e[nb] = d4{0.0, 0.0, 0.0, 0.0};
    if (aligned) {
      double av[4];   // the block's four K steps' operands loaded ahead of the MFMA chain
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int bb = 16 * mb + 4 * q + (lane >> 4) - alc;
        av[q] = (bb >= 0 && bb < ak) ? SHw[ra * KMAX + bb] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int nb = 0; nb < TileW4::NB; ++nb)
          e[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], w0[mb][nb][q], e[nb], 0, 0, 0);
    } else {
      int lo = ak ? alc : PANEL, hi = ak ? alc + ak : 0;
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
      }
      lo = __builtin_amdgcn_readfirstlane(lo);
      hi = __builtin_amdgcn_readfirstlane(hi);
      // K = the rows of the restarts touching block mb: within [16 mb - 15, 16 mb + 31) (k <= 16, restarts never
      // leave the tile), i.e. K steps q in [4 mb - 4, 4 mb + 8)
#pragma unroll
      for (int q = (4 * mb - 4 > 0 ? 4 * mb - 4 : 0); q < (4 * mb + 8 < 4 * TileW4::MB ? 4 * mb + 8 : 4 * TileW4::MB); ++q) {
        if (4 * q + 3 < lo || 4 * q >= hi) continue;   // wave-uniform
        const int bb = 4 * q + (lane >> 4) - alc;
        const double av = (bb >= 0 && bb < ak) ? SHw[ra * KMAX + bb] : 0.0;
#pragma unroll
        for (int nb = 0; nb < TileW4::NB; ++nb)
          e[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, w0[q >> 2][nb][q & 3], e[nb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int c = 16 * mb + (lane >> 4) + 4 * reg;
      if (!((actmask >> c) & 1)) continue;
#pragma unroll
      for (int nb = 0; nb < TileW4::NB; ++nb) {
        double v;
        if constexpr (RULE == RULE_EUCLID) {
          const int gene = gt * GTG + (GTG / WC) * wc + 16 * nb + (lane & 15);
          v = gene < tiles.m ? euclid_rule_w(w0[mb][nb][reg], tl.acc[mb][nb][reg], e[nb][reg]) : 0.0;
        } else {
          v = mu_rule_sel(w0[mb][nb][reg], tl.acc[mb][nb][reg], e[nb][reg]);
        }
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rw, wvoff, woff(mb, reg, nb), 0);
      }
    }
  }
}

}  // namespace nmfc
