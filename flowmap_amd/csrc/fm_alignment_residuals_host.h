// The alignment residual maps (include/flowmap_hip.h, ABI version 11) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  Per element it calls corr_load_with and alignment_offset
// (fm_math.h), the very functions the device kernel (fm_alignment_residuals.hip) calls; the sums are fp64 from the element upward, in
// element order (one serial "workgroup" per pair: reproducible and window-independent by construction), and the workspace is not used.
#pragma once

#include <cstddef>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"

extern "C" {

int fm_alignment_residual_workspace(long points, long* doubles) {
  if (!fm::alignment_residual_workspace_args_ok(points, doubles)) return 1;
  doubles[0] = 2 * fm::alignment_residual_tiles(points);
  return 0;
}

int fm_alignment_residuals(const float* depth, const float* kinv, const float* surfaces, const float* bwd_flow, const float* weights,
                           float weight_sensitivity, const float* rel, const int64_t* indices, long points, int batch, int frames,
                           int height, int width, int first_pair, int count, float* residual, float* offset, float* weight_out,
                           double* pair_sum, double* pair_weight, double* workspace, void*) {
  using namespace fm;
  if (!alignment_residuals_args_ok(depth, kinv, surfaces, bwd_flow, rel, indices, points, batch, frames, height, width, first_pair, count, residual, pair_sum,
                                   pair_weight, workspace))
    return 1;
  const bool sums = pair_sum != nullptr;
  const int n = height * width;
  for (int b = 0; b < batch; ++b)
    for (int lp = 0; lp < count; ++lp) {
      const int pair = first_pair + lp;
      const size_t bp = (size_t)b * count + lp, fe = (size_t)b * frames + pair, pr = (size_t)b * (frames - 1) + pair;
      CorrSrc s;
      s.depth_e = depth ? depth + fe * n : nullptr;
      s.depth_l = depth ? depth + (fe + 1) * n : nullptr;
      s.surf_e = surfaces ? surfaces + fe * n * 3 : nullptr;
      s.surf_l = surfaces ? surfaces + (fe + 1) * n * 3 : nullptr;
      s.bwd_flow = bwd_flow + pr * n * 2;
      s.weights = weights ? weights + pr * n : s.bwd_flow;  // (read and replaced by 1, as the device kernel does)
      s.weight_sens = weights ? weight_sensitivity : 0.f;
      s.height = height;
      s.width = width;
      Mat3 kinv_e{}, kinv_l{};
      if (depth) {
        load_mat3(kinv + fe * 9, kinv_e);
        load_mat3(kinv + (fe + 1) * 9, kinv_l);
      }
      Pose t;
      load_pose44(rel + pr * 16, t);
      double sum_r = 0.0, sum_w = 0.0;
      for (long j = 0; j < points; ++j) {
        const int idx = alignment_pixel(indices ? (long)indices[j] : j, n);
        const Corr c = corr_load_with<false>(s, kinv_e, kinv_l, pixel_ref(idx, height, width), [&](int tr, int tc, float& ut, float& vt) {
          ut = pixel_center(tc, width);
          vt = pixel_center(tr, height);
          return s.depth_e[tr * width + tc];
        });
        const float w = weights ? c.w : 1.f;
        float d[3];
        const float r = alignment_offset(t, c.p, c.q, d);
        const size_t o = bp * (size_t)points + (size_t)j;
        residual[o] = r;
        if (offset) {
          offset[o * 3] = d[0];
          offset[o * 3 + 1] = d[1];
          offset[o * 3 + 2] = d[2];
        }
        if (weight_out) weight_out[o] = w;
        sum_r += (double)(w * r);
        sum_w += (double)w;
      }
      if (sums) {
        pair_sum[bp] = sum_r;
        pair_weight[bp] = sum_w;
      }
    }
  return 0;
}

}  // extern "C"
