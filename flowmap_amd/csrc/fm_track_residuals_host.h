// The tracking residual maps (include/flowmap_hip.h, ABI version 10) for a HOST build of the C ABI.
//
// fm_pose.h includes this file at its end when it is compiled by a plain host compiler — the serial build of the ABI that the CPU
// test-suite links the package against instead of libflowmap_hip.so — and never under hipcc.  Per element it calls track_source_point,
// track_target / track_scale_target and track_residual_at (fm_pose.h), the very functions the device kernels (fm_track_residuals.hip)
// call; the sums are fp64 from the element upward with the same select (`visible ? ρ : 0`), in element order — points ascending per
// pair, then (fs, ft) ascending per point: reproducible and window-independent by construction — and neither `tgt` nor the workspace
// is used.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"

namespace fm {
namespace track_residuals_host {

template <int KIND>
inline void run(const float* depth, const float* kinv, const float* ext, const float* ext_inv, const float* k, const float* xy, const uint8_t* vis,
                const int32_t* seg, int first, int count, int height, int width, float delta, float ax, float ay, float* residual, uint8_t* visible,
                float* xy_target, double* pair_sum, double* pair_count, double* track_sum, double* track_count) {
  const float inv_delta = KIND == kHuber ? 1.0f / delta : 0.f;
  size_t elems = 0, pairs = 0, points = 0;
  for (int sg = first; sg < first + count; ++sg) {
    const int start = seg[sg * 4], f = seg[sg * 4 + 1], pc = seg[sg * 4 + 2];
    const size_t off = (size_t)seg[sg * 4 + 3];
    if (pair_sum) {
      for (size_t i = 0; i < (size_t)f * f; ++i) pair_sum[pairs + i] = pair_count[pairs + i] = 0.0;
      for (int p = 0; p < pc; ++p) track_sum[points + p] = track_count[points + p] = 0.0;
    }
    for (int fs = 0; fs < f; ++fs)
      for (int p = 0; p < pc; ++p) {
        const size_t src = off + (size_t)fs * pc + p;
        const float qx = xy[src * 2], qy = xy[src * 2 + 1];
        float xw[3];
        track_source_point(depth + (size_t)(start + fs) * height * width, kinv + (size_t)(start + fs) * 9, ext + (size_t)(start + fs) * 16, qx, qy,
                           height, width, xw);
        const bool source = vis[src] != 0 && qx >= 0.f && qy >= 0.f && qx < 1.f && qy < 1.f;
        for (int ft = 0; ft < f; ++ft) {
          float tg[kTrackTgt], ts[kTrackTgt];
          track_target(ext_inv + (size_t)(start + ft) * 16, k + (size_t)(start + ft) * 9, tg);
          track_scale_target(tg, ax, ay, ts);
          const size_t dst = off + (size_t)ft * pc + p;
          const TrackResidual r = track_residual_at<KIND>(ts, xw, xy[dst * 2] * ax, xy[dst * 2 + 1] * ay, delta, inv_delta, ax, ay,
                                                          ext_inv + (size_t)(start + ft) * 16, k + (size_t)(start + ft) * 9);
          const bool seen = source && vis[dst] != 0 && r.inside;
          const size_t o = elems + ((size_t)fs * f + ft) * pc + p;
          residual[o] = r.rho;
          visible[o] = seen ? 1 : 0;
          if (xy_target) {
            xy_target[o * 2] = r.u;
            xy_target[o * 2 + 1] = r.v;
          }
          if (pair_sum) {
            const double term = seen ? (double)r.rho : 0.0, one = seen ? 1.0 : 0.0;
            pair_sum[pairs + (size_t)fs * f + ft] += term;
            pair_count[pairs + (size_t)fs * f + ft] += one;
            track_sum[points + p] += term;
            track_count[points + p] += one;
          }
        }
      }
    elems += (size_t)f * f * pc;
    pairs += (size_t)f * f;
    points += (size_t)pc;
  }
}

}  // namespace track_residuals_host
}  // namespace fm

extern "C" {

int fm_track_residual_workspace(int frames, int points, long* doubles) {
  if (!fm::track_residual_workspace_args_ok(frames, points, doubles)) return 1;
  doubles[0] = fm::track_res_work(frames, points);
  return 0;
}

int fm_track_residuals(const float* depth, const float* kinv, const float* ext, const float* ext_inv, const float* k, int frames, const float* xy,
                       const uint8_t* vis, const int32_t* seg, int first_segment, int count, int pmax, int fmax, int height, int width,
                       int mapping_kind, float delta, float aspect_x, float aspect_y, float* tgt, float* residual, uint8_t* visible,
                       float* xy_target, double* pair_sum, double* pair_count, double* track_sum, double* track_count, double* workspace, void*) {
  if (!fm::track_residuals_args_ok(depth, kinv, ext, ext_inv, k, frames, xy, vis, seg, first_segment, count, pmax, fmax, height, width, mapping_kind, aspect_x,
                                   aspect_y, tgt, residual, visible, pair_sum, pair_count, track_sum, track_count, workspace))
    return 1;
  for (int sg = first_segment; sg < first_segment + count; ++sg)
    if (seg[sg * 4] < 0 || seg[sg * 4 + 1] < 1 || seg[sg * 4 + 2] < 1 || seg[sg * 4] + seg[sg * 4 + 1] > frames) return 1;
#define FM_TRES_HOST(K)                                                                                                                        \
  fm::track_residuals_host::run<fm::K>(depth, kinv, ext, ext_inv, k, xy, vis, seg, first_segment, count, height, width, delta, aspect_x, aspect_y, \
                                       residual, visible, xy_target, pair_sum, pair_count, track_sum, track_count)
  if (mapping_kind == fm::kHuber) FM_TRES_HOST(kHuber);
  else if (mapping_kind == fm::kL1) FM_TRES_HOST(kL1);
  else FM_TRES_HOST(kL2);
#undef FM_TRES_HOST
  return 0;
}

}  // extern "C"
