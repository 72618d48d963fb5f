// nmfc_kernels.hpp -- HIP kernels of the batched MU restart engine (gfx950 / CDNA4).
//
// Device layouts (DESIGN.md "Data layout in HBM"):
//   Ablk [m_pad/16][n_cols_pad][16]  16-gene blocks of every column j of A (operand of W^T A)
//   Acm [n_cols_pad][m_pad]  column j of A, gene-contiguous              (small-shape kernel only)
//   Arm [m_pad][n_pad]       row i of A, sample-contiguous              (operand of A h^T)
//   W   [cols][m_pad]        column c of the stacked W_all (restart owns columns col0..col0+k-1)
//   H   [cols][n_pad]        row c of the stacked H_all (sample-contiguous)
//   Restarts are packed into panels of 64 columns; a restart never straddles a panel.
// Both contractions are "TN" tiles C[r][c] = sum_k P[r][k] Q[c][k] over K-contiguous rows, computed
// with v_mfma_f64_16x16x4_f64 on the GTile core (LDS-DMA ring, nmfc_gtile.hpp).
//
// This file is the umbrella: it holds no kernel.  The include order below is the order of the engine's code object --
// hipcc emits a translation unit's non-template kernels in the order they are defined, then its template instantiations
// in the order engine.hip first names them -- so a new family header goes after every existing one.
#pragma once
#include "nmfc_common.hpp"
#include "nmfc_gtile.hpp"
#include "nmfc_wta.hpp"
#include "nmfc_hupdate.hpp"
#include "nmfc_neals.hpp"
#include "nmfc_ahtw.hpp"
#include "nmfc_small.hpp"
#include "nmfc_sweep.hpp"
#include "nmfc_norm.hpp"
#include "nmfc_resid.hpp"
