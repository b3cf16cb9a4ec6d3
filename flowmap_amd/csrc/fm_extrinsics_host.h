// The regressed-extrinsics entry points (include/flowmap_hip.h, ABI version 8) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  Both entries are serial loops over the per-pair steps of
// fm_pose.h, the very functions the device kernels (fm_extrinsics.hip) call.  fm_pose.h includes fm_math.h, so those steps are defined
// AFTER this point of the translation unit: they are declared here, and a host build of the ABI includes fm_pose.h as well.
#pragma once

#include <cstddef>

#include "../../include/flowmap_hip.h"

namespace fm {
inline void quat_pose_fwd_one(const float* q, const float* t, float* tf, float* tf_inv);
inline void quat_pose_bwd_one(const float* q, const float* t, const float* tf_inv, const float* g_tf, const float* g_tf_inv, float* g_q, float* g_t,
                              const float* g_tf_more);
inline void pose_chain_fwd_one(const float* rel, int steps, float* e);
}  // namespace fm

extern "C" {

int fm_quat_pose_fwd(const float* quat, const float* trans, int pairs, float* t_bwd, float* t_fwd, float* ext, void*) {
  if (!quat || !trans || !t_bwd || !t_fwd || pairs < 1) return 1;
  for (int p = 0; p < pairs; ++p) fm::quat_pose_fwd_one(quat + (size_t)p * 4, trans + (size_t)p * 3, t_bwd + (size_t)p * 16, t_fwd + (size_t)p * 16);
  if (ext) fm::pose_chain_fwd_one(t_bwd, pairs, ext);
  return 0;
}

int fm_quat_pose_bwd(const float* quat, const float* trans, const float* t_fwd, const float* g_t_bwd, const float* g_t_fwd,
                     const float* g_rel_chain, int pairs, float* g_quat, float* g_trans, void*) {
  if (!quat || !trans || !t_fwd || !g_quat || !g_trans || pairs < 1) return 1;
  for (int p = 0; p < pairs; ++p) {
    const size_t at = (size_t)p * 16;
    fm::quat_pose_bwd_one(quat + (size_t)p * 4, trans + (size_t)p * 3, t_fwd + at, g_t_bwd ? g_t_bwd + at : nullptr, g_t_fwd ? g_t_fwd + at : nullptr,
                          g_quat + (size_t)p * 4, g_trans + (size_t)p * 3, g_rel_chain ? g_rel_chain + at : nullptr);
  }
  return 0;
}

}  // extern "C"
