// nmfc_internal.hpp -- what the library's translation units share beside the public C ABI (include/nmfc.h):
// the functions one file defines for another, declared once, and the stop-rule check of the nmf_mu-shaped entries.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/nmfc.h"

namespace nmfc {
struct SoloJob;   // nmfc_common.hpp (brunet.hip and the host-runtime driver include this file without it)
}

// Exported but in no public header: compat.hip is also built on its own and linked against the library (the host
// sanitizer build of the drop-in's C), so what it calls in other translation units (nmfc_set_error and the two
// release functions below) must resolve from outside.
// engine.hip: the thread's error slot behind nmfc_last_error
extern "C" void nmfc_set_error(const char* msg);

// solo.hip: the batched one-workgroup-per-restart kernels on gct-sized shapes -- the kernel rank (2, 3, 4 or 8) that
// takes rank k, and one launch of njobs jobs of kernel rank kp (0: every rank) on at most max_wgs workgroups
__attribute__((visibility("hidden"))) int nmfc_solo_batch_rank(int n, int k);
__attribute__((visibility("hidden"))) int nmfc_solo_batch_launch(const double* Acm, long a_ld, int m, int n, double* W,
                                                                 long w_ld, double* H, long h_ld,
                                                                 const nmfc::SoloJob* djobs, int njobs, int kp,
                                                                 int maxiter, int stop_rule, int* stop_iter,
                                                                 int* stop_reason, int max_wgs, hipStream_t st);

// solo.hip: drops its per-process copy of A, work buffer and pinned staging (nmfc_nmf_mu_release, compat.hip)
extern "C" void nmfc_solo_release();
// generic.hip: drops its per-process copy of A, work buffers and stream (nmfc_nmf_mu_release, compat.hip)
extern "C" void nmfc_generic_release();

// the stop rules of the single-restart entries (nmfc_engine_mu1, nmfc_mu_solo, nmfc_mu_generic): not STOP_TOLX
inline bool nmfc_mu_stop_rule_ok(int stop_rule) {
  return stop_rule == NMFC_STOP_FIXED || stop_rule == NMFC_STOP_REF_COMPAT || stop_rule == NMFC_STOP_ARGMAX_STABLE;
}
