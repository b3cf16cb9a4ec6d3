// The softmin focal sweep per pair (include/flowmap_hip.h, ABI version 12) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  Per correspondence it calls corr_load_with, moments_add and
// softmin_term (fm_math.h) and per (batch entry, pair, candidate) moments_finish and pose_solve_one (fm_pose.h), the very functions the
// device kernel (fm_focal_sweep.hip) calls; the moments (each correspondence's fp32 terms) and the error are summed in fp64 in element
// order: one serial "workgroup" per output element, reproducible and window-independent by construction.  fm_pose.h includes fm_math.h,
// so pose_solve_one is defined AFTER this point of the translation unit: it is declared here, and a host build of the ABI includes
// fm_pose.h as well.
#pragma once

#include <cmath>
#include <cstddef>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"

namespace fm {
inline void pose_solve_one(const double* st, float* tb, float* tf, double* ax);
}  // namespace fm

extern "C" {

int fm_focal_sweep(const float* depth, const float* weights, float weight_sensitivity, const float* bwd_flow, const int64_t* indices, long points,
                   const float* focal_lengths, const float* candidate_k, const float* candidate_kinv, int batch, int frames, int height, int width,
                   int first_pair, int count, int candidates, double* error, float* soft, float* focal, float* intrinsics, float* poses,
                   float* point_error, void*) {
  using namespace fm;
  if (!focal_sweep_args_ok(depth, weights, bwd_flow, indices, points, focal_lengths, candidate_k, candidate_kinv, batch, frames, height, width, first_pair,
                           count, candidates, error, soft, focal, intrinsics))
    return 1;
  const int n = height * width;
  for (int b = 0; b < batch; ++b)
    for (int lp = 0; lp < count; ++lp) {
      const int pair = first_pair + lp;
      const size_t bp = (size_t)b * count + lp, fe = (size_t)b * frames + pair, pr = (size_t)b * (frames - 1) + pair;
      CorrSrc s;
      s.depth_e = depth + fe * n;
      s.depth_l = depth + (fe + 1) * n;
      s.surf_e = s.surf_l = nullptr;
      s.bwd_flow = bwd_flow + pr * n * 2;
      s.weights = weights + pr * n;
      s.weight_sens = weight_sensitivity;
      s.height = height;
      s.width = width;
      for (int cand = 0; cand < candidates; ++cand) {
        Mat3 k, kinv;
        load_mat3(candidate_k + (size_t)cand * 9, k);
        load_mat3(candidate_kinv + (size_t)cand * 9, kinv);
        float shift[3];
        later_point(s, kinv, alignment_pixel((long)indices[points / 2], n), shift);
        double st[16];
        for (int i = 0; i < 16; ++i) st[i] = 0.0;
        for (long j = 0; j < points; ++j) {
          const int idx = alignment_pixel((long)indices[j], n);
          const Corr c = corr_load_with<false>(s, kinv, kinv, pixel_ref(idx, height, width), [&](int tr, int tc, float& ut, float& vt) {
            ut = pixel_center(tc, width);
            vt = pixel_center(tr, height);
            return s.depth_e[tr * width + tc];
          });
          float one[kMomentCount];
          for (int i = 0; i < kMomentCount; ++i) one[i] = 0.f;
          moments_add(c, shift, one);
          for (int i = 0; i < kMomentCount; ++i) st[i] += (double)one[i];
        }
        moments_finish(st, shift);
        float pose44[16];
        double aux[40];
        pose_solve_one(st, pose44, nullptr, aux);
        const size_t out = bp * (size_t)candidates + (size_t)cand;
        if (poses)
          for (int i = 0; i < 16; ++i) poses[out * 16 + i] = pose44[i];
        Pose t;
        load_pose44(pose44, t);
        double sum = 0.0;
        for (long j = 0; j < points; ++j) {
          const int idx = alignment_pixel((long)indices[j], n);
          const PixelRef px = pixel_ref(idx, height, width);
          float w = s.weights[idx];
          if (weight_sensitivity != 0.f) w = fm_sigmoid<false>(weight_sensitivity * w);
          SoftminTerm o;
          const float e = softmin_term(k, kinv, t, px.u, px.v, s.depth_l[idx], s.bwd_flow[2 * (size_t)idx], s.bwd_flow[2 * (size_t)idx + 1], w, o);
          if (point_error) point_error[out * (size_t)points + (size_t)j] = e;
          sum += (double)e;
        }
        error[out] = sum;
      }
      // the curve of this (batch entry, pair): the arithmetic of the host build's fm_softmin_blend_fwd
      const double* e = error + bp * (size_t)candidates;
      float lo = (float)e[0];
      for (int c = 1; c < candidates; ++c) lo = std::fmin(lo, (float)e[c]);
      double total = 0.0;
      for (int c = 0; c < candidates; ++c) total += std::exp(-(((float)e[c] - lo) * 10.f));
      float m[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, fl = 0.f;
      for (int c = 0; c < candidates; ++c) {
        const float sn = (float)(std::exp(-(((float)e[c] - lo) * 10.f)) / total);
        soft[bp * (size_t)candidates + c] = sn;
        for (int i = 0; i < 9; ++i) m[i] += candidate_k[(size_t)c * 9 + i] * sn;
        fl += focal_lengths[c] * sn;
      }
      for (int i = 0; i < 9; ++i) intrinsics[bp * 9 + i] = m[i];
      focal[bp] = fl;
    }
  return 0;
}

}  // extern "C"
