// nmfc_common.hpp -- what every kernel family of the MU engine and the single-restart paths share: vector types,
// tile and stop-rule constants, the elementwise update rules, lane helpers and the plain structs the host fills.
// No __global__ function: a translation unit that includes only this header emits no kernel of the engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmfc {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));

constexpr int PANEL = 64;          // restart columns per panel
constexpr int BK = 32;             // padding multiple of the sample dimension (K of A h^T)
constexpr int NT = 256;            // threads per workgroup
constexpr int KMAX = 16;           // largest rank k
constexpr int GT = 128;            // genes per A h^T tile (and per Gram partial)
constexpr int STOP_FIXED = 0, STOP_REF_COMPAT = 1, STOP_ARGMAX_STABLE = 2, STOP_TOLX = 3;
constexpr double SQRTEPS = 1.0536712127723509e-08;   // sqrt(dlamch('E')), nmf_als.c sqrteps
constexpr double DIV_BY_ZERO_AVOIDANCE = 1E-09;   // nmf_mu.c:56

// nmf_mu.c:184-191 / :209-216: h = (h0 == 0 || num == 0) ? 0 : h0 * (num / (den + 1e-9)); clamp < 0
// (ZERO_THRESHOLD = 0.0, common.h:15).  Order add -> divide -> multiply is kept (no contraction).
__device__ __forceinline__ double mu_rule(double old, double num, double den) {
  if (old == 0.0 || num == 0.0) return 0.0;
  const double q = num / (den + DIV_BY_ZERO_AVOIDANCE);
  const double t = old * q;
  return t < 0.0 ? 0.0 : t;
}

// The BROAD nmfconsensus script's Euclidean NMF() (DESIGN.md "Euclidean NMF()"): the second elementwise rule the H and
// W update kernels can be instantiated with, and its stop rule (every stopfreq-th iteration the per-sample first-maximum
// class against the stored one; stopconv unchanged checks in a row stop the restart).
constexpr int RULE_MU = 0, RULE_EUCLID = 1, RULE_NEALS = 2;
constexpr int STOP_MEMBER = 4;                          // internal to the engine: set by nmfc_engine_set_euclid runs
constexpr double R_EPS = 2.220446049250313080847e-16;   // R's .Machine$double.eps = 2^-52

// H <- H * (crossprod(W, V) / crossprod(W, VP)) + eps: divide, multiply, add, each rounded on its own (no FMA
// contraction); no zero guard and no clamp, so the IEEE results are R's.
__device__ __forceinline__ double euclid_rule_h(double old, double num, double den) {
#pragma clang fp contract(off)
  const double q = num / den;
  const double t = old * q;
  return t + R_EPS;
}

// W <- W * (V %*% t(H)) / (VP %*% t(H)) + eps: multiply, divide, add.
__device__ __forceinline__ double euclid_rule_w(double old, double num, double den) {
#pragma clang fp contract(off)
  const double t = old * num;
  const double q = t / den;
  return q + R_EPS;
}

// Kernel arguments only the Euclidean instantiations take: they stand in the place of an int of the default rule's
// signature, which therefore stays as it is.
struct StopMember {
  int rule, stopconv, stopfreq;   // STOP_FIXED or STOP_MEMBER, and the script's stopconv / stopfreq
};
struct GeneTiles {
  int ngt, m;   // gene tiles of the launch, and the rows of A: W rows >= m are padding and stay +0.0
};
template <int RULE>
struct RuleArgs {
  using Stop = int;
  using Tiles = int;
};
template <>
struct RuleArgs<RULE_EUCLID> {
  using Stop = StopMember;
  using Tiles = GeneTiles;
};
template <>
struct RuleArgs<RULE_NEALS> {   // nmf_neals: its H side is a kernel of its own (k_hupdate_neals)
  using Stop = int;
  using Tiles = GeneTiles;
};
__device__ __forceinline__ int stop_rule_of(int s) { return s; }
__device__ __forceinline__ int stop_rule_of(const StopMember& s) { return s.rule; }
__device__ __forceinline__ int stopconv_of(int) { return 200; }   // nmf_mu.c:269
__device__ __forceinline__ int stopconv_of(const StopMember& s) { return s.stopconv; }
__device__ __forceinline__ int stopfreq_of(int) { return 2; }     // nmf_mu.c:253
__device__ __forceinline__ int stopfreq_of(const StopMember& s) { return s.stopfreq; }
__device__ __forceinline__ int ngt_of(int t) { return t; }
__device__ __forceinline__ int ngt_of(const GeneTiles& t) { return t.ngt; }

// The wave's index in its workgroup as a wave-uniform (SGPR) value.  threadIdx.x >> 6 is uniform within a wave, but the
// compiler does not know it: a buffer resource or a base pointer derived from it would be kept in VGPRs and every
// buffer load / store through it wrapped in a readfirstlane "waterfall" loop (round 5: 64 such loops around k_ahtw4's
// W0 loads and W stores).
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
// The lane index by v_mbcnt: recomputed where it is used (two VALU instructions) instead of a value derived from
// threadIdx.x before a K loop and held in a VGPR across it (the 16-wave W^T A tile has no register to spare).
__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// mu_rule without branches: the quotient and product are formed for every element and the zero cases selected after,
// so a wave's rule is one straight instruction stream (no exec-mask branch per element).  The same bits as mu_rule for
// every input: where mu_rule returns early, the select returns the same +0.0.
__device__ __forceinline__ double mu_rule_sel(double old, double num, double den) {
  const double q = num / (den + DIV_BY_ZERO_AVOIDANCE);
  const double t = old * q;
  return (old == 0.0 || num == 0.0 || t < 0.0) ? 0.0 : t;
}

// Workgroup id -> work item such that each XCD (blocks b, b+8, ... share one) receives a contiguous
// range of items (bijective for any count; a speed choice only, never correctness).
__device__ __forceinline__ int xcd_item(int b, int nblocks) {
  const int xcd = b & 7, idx = b >> 3;
  const int q = nblocks >> 3, r = nblocks & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Per-restart metadata.  rid is the persistent restart index (stop state, Gram/SH offsets, output
// slot); col0 is its current first column in W/H (changes when the engine repacks live restarts).
struct RestartInfo {
  int col0;
  int k;
  int rid;
  int sq_off;   // offset of its k x k blocks in the compact Gram / SH arrays
};

// Per panel column: the owning restart's compact-block offset, its first panel-local column, k
// (k = 0: padding column) and its restart id.
struct ColInfo {
  int sq_off;
  int lc0;
  int k;
  int rid;
};

constexpr int SMALL_MAXR = 8;   // restarts per 16-column block (k >= 2)

// One 16-column block of restarts of the small-shape kernels (k_small_mu, k_team_mu)
struct SmallBlock {
  int col0;                  // first stacked column of the block (W/H rows col0 .. col0 + 15)
  int nr;                    // restarts in the block
  int rid[SMALL_MAXR];       // persistent restart ids
  int k[SMALL_MAXR];
  int lc0[SMALL_MAXR];       // block-local first column
};

// One restart of a batched k_solo_mu launch (csrc/solo.hip; rank <= 4 on gct-sized shapes): its stacked W/H
// rows col0 .. col0 + k - 1 and its persistent restart id (stop iteration / reason slots).
struct SoloJob {
  int col0, k, rid, pad;
};

// k rows to move: repacking and the final-factor archive (k_move_rows)
struct MoveJob {
  int src_row;
  int dst_row;
  int k;
};

// One restart to initialise: its job seed, its columns and its chunks of the draw stream (k_init, k_init_runif)
struct InitJob {
  uint32_t seed;
  int col0;
  int k;
  int nchunks;
};

}  // namespace nmfc
