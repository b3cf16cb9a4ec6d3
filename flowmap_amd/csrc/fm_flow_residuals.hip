// Flow residual maps (LossFlow.residuals; include/flowmap_hip.h: fm_flow_residuals): per pixel and pair the unmasked flow term of
// LossFlow.compute_unweighted_loss (flowmap/loss/loss_flow.py:46-68), optionally the pose-induced flow it maps, and the per-pair
// masked sums — for a WINDOW of pairs, straight from depth, in one HBM-bound launch plus one tiny one.
//
// A workgroup of 256 threads owns kResTile = 2048 consecutive pixels of ONE (batch entry, pair, direction); a thread handles
// kResQuads quads of four adjacent pixels, 256 quads apart (a wave's loads are contiguous).  Per pixel and pair it moves 4 + 4 bytes
// of depth, 16 of flows, 8 of masks in and 8 (24 with the predicted flows) out; the arithmetic is flow_residual_at (fm_math.h:
// flow_term_fast, the fused pass's own term) — a few dozen VALU instructions per pixel, far below the memory time.  Nothing is
// staged in LDS; the only LDS is the 64 bytes of the block reduction.
//
// The sums use no atomics: a thread adds (double)(residual·mask) and (double)mask of its pixels in fp64, and the ordered two-stage sum of
// fm_ordered_sums.h takes them from there — the workgroup's slot is [b][pair][direction][workgroup], a row a (batch entry, pair,
// direction).  Which pixels a workgroup owns depends on (height, width) only, so a pair's sums are the same bits however it is reached.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_ordered_sums.h"
#include "fm_residual_args.h"

namespace fm {

constexpr int kResThreads = 256;
constexpr int kResQuads = 2;                            // quads per thread
constexpr int kResTile = kResThreads * kResQuads * 4;   // pixels per workgroup
static_assert(kResTile == kFlowResTile, "fm_residual_args.h sizes the workspace");

struct ResidualParams {
  const float* depth;
  const float* k;
  const float* kinv;
  const float* t_fwd;
  const float* t_bwd;
  const float* flow_fwd;
  const float* flow_bwd;
  const float* mask_fwd;  // (null together with mask_bwd and work: no sums)
  const float* mask_bwd;
  float* res_fwd;
  float* res_bwd;
  float* pred_fwd;  // (null together with pred_bwd: no predicted flows)
  float* pred_bwd;
  double* work;
  long fs[5], bs[5];  // element strides of depth, flow_fwd, flow_bwd, mask_fwd, mask_bwd (fm_layout)
  int frames, height, width, first_pair, count, blocks;
  float delta, ax, ay;
};

template <int VEC, int KIND>
__global__ void __launch_bounds__(kResThreads) flow_residuals_kernel(ResidualParams p) {
  const int dir = blockIdx.z;  // 0: pair's earlier frame towards the later one, 1: the later towards the earlier
  const int bp = blockIdx.y;   // batch entry x pairs of the window
  const int b = bp / p.count;
  const int pair = p.first_pair + (bp - b * p.count);
  const int src = pair + dir, dst = pair + 1 - dir;
  const int n = p.height * p.width;

  const float* pose44 = (dir ? p.t_bwd : p.t_fwd) + ((size_t)b * (p.frames - 1) + pair) * 16;
  const float* kinv9 = p.kinv + ((size_t)b * p.frames + src) * 9;
  const float* kdst9 = p.k + ((size_t)b * p.frames + dst) * 9;
  DirConst d;
  {
    Mat3 kinv, kd;
    Pose t;
    load_mat3(kinv9, kinv);
    load_mat3(kdst9, kd);
    load_pose44(pose44, t);
    make_dir(t, kinv, kd, p.ax, p.ay, d);
  }
  const float inv_delta = KIND == kHuber ? 1.0f / p.delta : 0.f;
  const float inv_ax = 1.0f / p.ax, inv_ay = 1.0f / p.ay;

  const float* depth = p.depth + (size_t)b * p.bs[0] + (size_t)src * p.fs[0];
  const float* flow = dir ? p.flow_bwd + (size_t)b * p.bs[2] + (size_t)pair * p.fs[2] : p.flow_fwd + (size_t)b * p.bs[1] + (size_t)pair * p.fs[1];
  const bool sums = p.work != nullptr;  // (uniform: kernel arguments)
  const float* mask = nullptr;
  if (sums) mask = dir ? p.mask_bwd + (size_t)b * p.bs[4] + (size_t)pair * p.fs[4] : p.mask_fwd + (size_t)b * p.bs[3] + (size_t)pair * p.fs[3];
  float* res = (dir ? p.res_bwd : p.res_fwd) + (size_t)bp * n;
  float* pred = dir ? p.pred_bwd : p.pred_fwd;
  if (pred) pred += (size_t)bp * n * 2;

  double sum_r = 0.0, sum_m = 0.0;
  const int quads = (n + 3) / 4;  // (the last one partial on the scalar path only)
#pragma unroll
  for (int it = 0; it < kResQuads; ++it) {
    const int quad = blockIdx.x * (kResThreads * kResQuads) + it * kResThreads + threadIdx.x;
    if (quad >= quads) continue;
    const int px0 = quad * 4;
    float z[4], fx[4], fy[4], m[4], rho[4], ox[4], oy[4];
    int row[4], col[4];
    if (VEC == 4) {  // width % 4 == 0: the quad lies in one image row, every base is 16-byte aligned
      const float4 z4 = *reinterpret_cast<const float4*>(depth + px0);
      const float4 f0 = *reinterpret_cast<const float4*>(flow + (size_t)px0 * 2);
      const float4 f1 = *reinterpret_cast<const float4*>(flow + (size_t)px0 * 2 + 4);
      float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (sums) m4 = *reinterpret_cast<const float4*>(mask + px0);
      z[0] = z4.x, z[1] = z4.y, z[2] = z4.z, z[3] = z4.w;
      fx[0] = f0.x, fy[0] = f0.y, fx[1] = f0.z, fy[1] = f0.w, fx[2] = f1.x, fy[2] = f1.y, fx[3] = f1.z, fy[3] = f1.w;
      m[0] = m4.x, m[1] = m4.y, m[2] = m4.z, m[3] = m4.w;
      const int r = px0 / p.width, c0 = px0 - r * p.width;
#pragma unroll
      for (int e = 0; e < 4; ++e) row[e] = r, col[e] = c0 + e;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int px = px0 + e;
        const bool in = px < n;
        z[e] = in ? depth[px] : 1.f;
        fx[e] = in ? flow[(size_t)px * 2] : 0.f;
        fy[e] = in ? flow[(size_t)px * 2 + 1] : 0.f;
        m[e] = (in && sums) ? mask[px] : 0.f;
        row[e] = (in ? px : 0) / p.width;
        col[e] = (in ? px : 0) - row[e] * p.width;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float u = pixel_center(col[e], p.width), v = pixel_center(row[e], p.height);
      // a1·v + a2 (and b, c alike): constant along an image row, as the fused pass forms them
      const float arow = fmaf(d.a1, v, d.a2), brow = fmaf(d.b1, v, d.b2), crow = fmaf(d.c1, v, d.c2);
      const FlowResidual o = flow_residual_at<KIND>(d, arow, brow, crow, z[e], u, v, u * p.ax, v * p.ay, fx[e], fy[e], p.delta, inv_delta, p.ax,
                                                    p.ay, inv_ax, inv_ay, pose44, kinv9, kdst9);
      rho[e] = o.rho, ox[e] = o.fx, oy[e] = o.fy;
      if (sums && (VEC == 4 || px0 + e < n)) {
        sum_r += (double)(o.rho * m[e]);
        sum_m += (double)m[e];
      }
    }
    if (VEC == 4) {
      *reinterpret_cast<float4*>(res + px0) = make_float4(rho[0], rho[1], rho[2], rho[3]);
      if (pred) {
        *reinterpret_cast<float4*>(pred + (size_t)px0 * 2) = make_float4(ox[0], oy[0], ox[1], oy[1]);
        *reinterpret_cast<float4*>(pred + (size_t)px0 * 2 + 4) = make_float4(ox[2], oy[2], ox[3], oy[3]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int px = px0 + e;
        if (px >= n) continue;
        res[px] = rho[e];
        if (pred) {
          pred[(size_t)px * 2] = ox[e];
          pred[(size_t)px * 2 + 1] = oy[e];
        }
      }
    }
  }

  if (!sums) return;  // (uniform)
  block_sum_to_slot<kResThreads>(sum_r, sum_m, p.work + 2 * (((size_t)bp * 2 + dir) * p.blocks + blockIdx.x));
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_flow_residual_blocks(int height, int width, int* blocks) {
  FM_CHECK_ARG(flow_residual_blocks_args_ok(height, width, blocks));
  blocks[0] = (int)flow_residual_blocks((long)height * width);
  return FM_OK;
}

int fm_flow_residuals(const float* depth, const float* k, const float* kinv, const float* t_fwd, const float* t_bwd, const float* flow_fwd,
                      const float* flow_bwd, const float* mask_fwd, const float* mask_bwd, int batch, int frames, int height, int width,
                      int mapping_kind, float delta, float aspect_x, float aspect_y, int first_pair, int count, float* residual_fwd,
                      float* residual_bwd, float* pred_fwd, float* pred_bwd, double* pair_sum, double* pair_valid, double* workspace,
                      const fm_layout* layouts, void* stream) {
  FM_CHECK_ARG(flow_residuals_args_ok(depth, k, kinv, t_fwd, t_bwd, flow_fwd, flow_bwd, mask_fwd, mask_bwd, batch, frames, height, width, mapping_kind,
                                      aspect_x, aspect_y, first_pair, count, residual_fwd, residual_bwd, pred_fwd, pred_bwd, pair_sum, pair_valid, workspace));
  const bool sums = pair_sum != nullptr;
  ResidualParams p{depth, k, kinv, t_fwd, t_bwd, flow_fwd, flow_bwd, sums ? mask_fwd : nullptr, sums ? mask_bwd : nullptr, residual_fwd, residual_bwd,
                   pred_fwd, pred_bwd, workspace};
  const long n = (long)height * width;
  FM_CHECK_ARG(flow_strides(layouts, batch, frames, n, p.fs, p.bs));
  p.frames = frames, p.height = height, p.width = width, p.first_pair = first_pair, p.count = count;
  p.blocks = (int)flow_residual_blocks(n);
  p.delta = delta, p.ax = aspect_x, p.ay = aspect_y;
  bool vec4 = width % 4 == 0 && aligned(depth) && aligned(flow_fwd) && aligned(flow_bwd) && aligned(residual_fwd) && aligned(residual_bwd);
  vec4 = vec4 && (!sums || (aligned(mask_fwd) && aligned(mask_bwd))) && (!pred_fwd || (aligned(pred_fwd) && aligned(pred_bwd)));
  for (int i = 0; i < (sums ? 5 : 3); ++i) vec4 = vec4 && p.fs[i] % 4 == 0 && p.bs[i] % 4 == 0;
  FM_CHECK_ARG(!sums || aligned(workspace));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)(batch * count), 2);
#define FM_RES_LAUNCH(V)                                                                                              \
  do {                                                                                                                \
    if (mapping_kind == kHuber) hipLaunchKernelGGL((flow_residuals_kernel<V, kHuber>), grid, dim3(kResThreads), 0, st, p); \
    else if (mapping_kind == kL1) hipLaunchKernelGGL((flow_residuals_kernel<V, kL1>), grid, dim3(kResThreads), 0, st, p);  \
    else hipLaunchKernelGGL((flow_residuals_kernel<V, kL2>), grid, dim3(kResThreads), 0, st, p);                      \
  } while (0)
  if (vec4) FM_RES_LAUNCH(4);
  else FM_RES_LAUNCH(1);
#undef FM_RES_LAUNCH
  if (sums)
    hipLaunchKernelGGL(ordered_slot_sums_kernel, dim3((unsigned)(batch * count * 2)), dim3(kWave), 0, st, workspace, p.blocks, pair_sum, pair_valid);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
