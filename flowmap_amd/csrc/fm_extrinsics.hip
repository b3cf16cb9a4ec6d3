// Regressed extrinsics (flowmap/model/extrinsics/extrinsics_regressed.py): per-pair quaternion + translation parameters ->
// 4x4 poses, their inverses and (optionally) the camera-to-world chain, in ONE launch; the analytic backward in one more.
//
// Both launches are latency-bound (at most a few thousand pairs, 32 floats out per pair): one thread per pair does the
// per-pair step of fm_pose.h in fp64 (quat_pose_fwd_one / quat_pose_bwd_one, shared with the host build), workgroups of
// 256, nothing staged in LDS.  The chain is the one-wave scan of the Procrustes fit (fm_device.h: pose_chain_one_wave), run
// by the first wave of the last workgroup to finish.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_pose.h"

namespace fm {

constexpr int kQuatThreads = 256;

// Finished workgroups of a forward launch that chains (more than one workgroup only).  Zero between launches: the last
// workgroup resets it.  One per device: such launches are ordered by their streams (include/flowmap_hip.h).
__device__ int quat_pose_blocks_done;

__global__ void __launch_bounds__(kQuatThreads) quat_pose_fwd_kernel(const float* __restrict__ quat, const float* __restrict__ trans, int pairs,
                                                                     float* t_bwd, float* t_fwd, float* ext) {
  const int pair = blockIdx.x * kQuatThreads + threadIdx.x;
  if (pair < pairs) {
    float q[4], t[3], tf[16], inv[16];
    for (int a = 0; a < 4; ++a) q[a] = quat[(size_t)pair * 4 + a];
    for (int a = 0; a < 3; ++a) t[a] = trans[(size_t)pair * 3 + a];
    quat_pose_fwd_one(q, t, tf, inv);
    for (int a = 0; a < 16; ++a) {
      t_bwd[(size_t)pair * 16 + a] = tf[a];
      t_fwd[(size_t)pair * 16 + a] = inv[a];
    }
  }
  if (ext == nullptr) return;  // (uniform: a kernel argument)
  __shared__ int last_block;
  if (gridDim.x > 1) {
    __threadfence();  // this thread's pose is visible device-wide before the counter says so
    __syncthreads();
    if (threadIdx.x == 0) {
      last_block = atomicAdd(&quat_pose_blocks_done, 1) == (int)gridDim.x - 1;
      if (last_block) quat_pose_blocks_done = 0;
    }
    __syncthreads();
    if (!last_block) return;
    __threadfence();  // see every workgroup's poses
  } else {
    __syncthreads();  // one workgroup: its own stores, ordered by the barrier
  }
  if (threadIdx.x < kWave) pose_chain_one_wave(t_bwd, pairs, ext);
}

__global__ void __launch_bounds__(kQuatThreads) quat_pose_bwd_kernel(const float* __restrict__ quat, const float* __restrict__ trans,
                                                                     const float* __restrict__ t_fwd, const float* __restrict__ g_t_bwd,
                                                                     const float* __restrict__ g_t_fwd, const float* __restrict__ g_rel_chain,
                                                                     int pairs, float* __restrict__ g_quat, float* __restrict__ g_trans) {
  const int pair = blockIdx.x * kQuatThreads + threadIdx.x;
  if (pair >= pairs) return;
  float q[4], t[3], inv[16], gq[4], gt[3];
  for (int a = 0; a < 4; ++a) q[a] = quat[(size_t)pair * 4 + a];
  for (int a = 0; a < 3; ++a) t[a] = trans[(size_t)pair * 3 + a];
  for (int a = 0; a < 16; ++a) inv[a] = t_fwd[(size_t)pair * 16 + a];
  const size_t at = (size_t)pair * 16;
  quat_pose_bwd_one(q, t, inv, g_t_bwd ? g_t_bwd + at : nullptr, g_t_fwd ? g_t_fwd + at : nullptr, gq, gt, g_rel_chain ? g_rel_chain + at : nullptr);
  for (int a = 0; a < 4; ++a) g_quat[(size_t)pair * 4 + a] = gq[a];
  for (int a = 0; a < 3; ++a) g_trans[(size_t)pair * 3 + a] = gt[a];
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_quat_pose_fwd(const float* quat, const float* trans, int pairs, float* t_bwd, float* t_fwd, float* ext, void* stream) {
  FM_CHECK_ARG(quat && trans && t_bwd && t_fwd && pairs >= 1 && pairs <= (1 << 24));
  const int blocks = (pairs + kQuatThreads - 1) / kQuatThreads;
  hipLaunchKernelGGL(quat_pose_fwd_kernel, dim3(blocks), dim3(kQuatThreads), 0, (hipStream_t)stream, quat, trans, pairs, t_bwd, t_fwd, ext);
  FM_LAUNCH_STATUS();
}

int fm_quat_pose_bwd(const float* quat, const float* trans, const float* t_fwd, const float* g_t_bwd, const float* g_t_fwd,
                     const float* g_rel_chain, int pairs, float* g_quat, float* g_trans, void* stream) {
  FM_CHECK_ARG(quat && trans && t_fwd && g_quat && g_trans && pairs >= 1 && pairs <= (1 << 24));
  const int blocks = (pairs + kQuatThreads - 1) / kQuatThreads;
  hipLaunchKernelGGL(quat_pose_bwd_kernel, dim3(blocks), dim3(kQuatThreads), 0, (hipStream_t)stream, quat, trans, t_fwd, g_t_bwd, g_t_fwd,
                     g_rel_chain, pairs, g_quat, g_trans);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
