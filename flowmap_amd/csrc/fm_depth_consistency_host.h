// The depth consistency across frame offsets (include/flowmap_hip.h, ABI version 13) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  Per pixel and offset it calls depth_consistency_at, per row
// depth_consistency_pose (fm_math.h), the very functions the device kernels (fm_depth_consistency.hip) call; the sums are fp64 from the
// pixel upward, in pixel order (one serial "workgroup" per row: reproducible and window-independent by construction), and the workspace
// is not used.
#pragma once

#include <cstddef>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"

extern "C" {

int fm_depth_consistency_blocks(int height, int width, int* blocks) {
  if (!fm::depth_consistency_blocks_args_ok(height, width, blocks)) return 1;
  blocks[0] = (int)fm::depth_consistency_blocks((long)height * width);
  return 0;
}

int fm_depth_consistency(const float* depth, const float* k, const float* kinv, const float* ext, const int32_t* offsets, int n_offsets, int batch,
                         int frames, int height, int width, int first_frame, int count, float tolerance, float* error, uint8_t* code,
                         float* positions, float* reprojected, float* sampled, uint8_t* support, double* frame_sum, double* frame_valid, float* rel,
                         double* workspace, void*) {
  if (!fm::depth_consistency_args_ok(depth, k, kinv, ext, offsets, n_offsets, batch, frames, height, width, first_frame, count, tolerance, error, code,
                                     positions, reprojected, sampled, support, frame_sum, frame_valid, rel, workspace))
    return 1;
  const size_t n = (size_t)height * width;
  for (int b = 0; b < batch; ++b)
    for (int lf = 0; lf < count; ++lf) {
      const int src = first_frame + lf;
      const size_t bf = (size_t)b * count + lf;
      const float* z = depth + ((size_t)b * frames + src) * n;
      fm::Mat3 ki;
      fm::load_mat3(kinv + ((size_t)b * frames + src) * 9, ki);
      if (support)
        for (size_t px = 0; px < n; ++px) support[bf * n + px] = 0;
      for (int o = 0; o < n_offsets; ++o) {
        const int dst = src + offsets[o];
        const size_t row = bf * n_offsets + o;
        float* rel16 = rel + row * 16;
        const bool present = dst >= 0 && dst < frames;
        if (present) fm::depth_consistency_pose(ext + ((size_t)b * frames + src) * 16, ext + ((size_t)b * frames + dst) * 16, rel16);
        else
          for (int e = 0; e < 16; ++e) rel16[e] = 0.f;
        fm::Pose t;
        fm::Mat3 kj;
        const float* depth_j = nullptr;
        if (present) {
          fm::load_pose44(rel16, t);
          fm::load_mat3(k + ((size_t)b * frames + dst) * 9, kj);
          depth_j = depth + ((size_t)b * frames + dst) * n;
        }
        double sum_e = 0.0, sum_n = 0.0;
        for (int r = 0; r < height; ++r)
          for (int c = 0; c < width; ++c) {
            const size_t px = (size_t)r * width + c, at = row * n + px;
            fm::DepthConsistencyTerm term{0.f, 0.f, 0.f, 0.f, 0.f, 1};
            if (present) {
              float ray[3];
              fm::ray_dir(ki, fm::pixel_center(c, width), fm::pixel_center(r, height), ray);
              term = fm::depth_consistency_at(ray, z[px], t, kj, depth_j, height, width);
            }
            error[at] = term.error;
            code[at] = (uint8_t)term.code;
            if (positions) {
              positions[at * 2] = term.u;
              positions[at * 2 + 1] = term.v;
              reprojected[at] = term.qz;
              sampled[at] = term.sampled;
            }
            if (term.code == 0) {
              sum_e += (double)fabsf(term.error);
              sum_n += 1.0;
              if (support && fabsf(term.error) <= tolerance) ++support[bf * n + px];
            }
          }
        if (frame_sum) {
          frame_sum[row] = sum_e;
          frame_valid[row] = sum_n;
        }
      }
    }
  return 0;
}

}  // extern "C"
