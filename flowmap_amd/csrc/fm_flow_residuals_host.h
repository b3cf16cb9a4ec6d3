// The flow residual maps (include/flowmap_hip.h, ABI version 9) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  Per pixel it calls flow_residual_at (fm_math.h), the very
// function the device kernel (fm_flow_residuals.hip) calls; the sums are fp64 from the pixel upward, in pixel order (one serial "workgroup"
// per pair: reproducible and window-independent by construction), and the workspace is not used.
#pragma once

#include <cstddef>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"

namespace fm {
namespace residuals_host {

template <int KIND>
inline void run(const float* depth, const float* k, const float* kinv, const float* t_fwd, const float* t_bwd, const float* const flow[2],
                const float* const mask[2], int batch, int frames, int height, int width, float delta, float ax, float ay, int first_pair, int count,
                float* const res[2], float* const pred[2], double* pair_sum, double* pair_valid, const long* fs, const long* bs) {
  const size_t n = (size_t)height * width;
  const float inv_delta = KIND == kHuber ? 1.0f / delta : 0.f;
  const float inv_ax = 1.0f / ax, inv_ay = 1.0f / ay;
  for (int b = 0; b < batch; ++b)
    for (int lp = 0; lp < count; ++lp)
      for (int dir = 0; dir < 2; ++dir) {
        const int pair = first_pair + lp, src = pair + dir, dst = pair + 1 - dir;
        const size_t bp = (size_t)b * count + lp;
        const float* pose44 = (dir ? t_bwd : t_fwd) + ((size_t)b * (frames - 1) + pair) * 16;
        const float* kinv9 = kinv + ((size_t)b * frames + src) * 9;
        const float* kdst9 = k + ((size_t)b * frames + dst) * 9;
        Mat3 ki, kd;
        Pose t;
        DirConst d;
        load_mat3(kinv9, ki);
        load_mat3(kdst9, kd);
        load_pose44(pose44, t);
        make_dir(t, ki, kd, ax, ay, d);
        const float* z = depth + (size_t)b * bs[0] + (size_t)src * fs[0];
        const float* fl = flow[dir] + (size_t)b * bs[1 + dir] + (size_t)pair * fs[1 + dir];
        const float* m = mask[dir] ? mask[dir] + (size_t)b * bs[3 + dir] + (size_t)pair * fs[3 + dir] : nullptr;
        double sum_r = 0.0, sum_m = 0.0;
        for (int row = 0; row < height; ++row) {
          const float v = pixel_center(row, height);
          const float arow = fmaf(d.a1, v, d.a2), brow = fmaf(d.b1, v, d.b2), crow = fmaf(d.c1, v, d.c2);
          for (int col = 0; col < width; ++col) {
            const size_t px = (size_t)row * width + col;
            const float u = pixel_center(col, width);
            const FlowResidual o = flow_residual_at<KIND>(d, arow, brow, crow, z[px], u, v, u * ax, v * ay, fl[px * 2], fl[px * 2 + 1], delta, inv_delta,
                                                          ax, ay, inv_ax, inv_ay, pose44, kinv9, kdst9);
            res[dir][bp * n + px] = o.rho;
            if (pred[dir]) {
              pred[dir][(bp * n + px) * 2] = o.fx;
              pred[dir][(bp * n + px) * 2 + 1] = o.fy;
            }
            if (m) {
              sum_r += (double)(o.rho * m[px]);
              sum_m += (double)m[px];
            }
          }
        }
        if (pair_sum) {
          pair_sum[bp * 2 + dir] = sum_r;
          pair_valid[bp * 2 + dir] = sum_m;
        }
      }
}

}  // namespace residuals_host
}  // namespace fm

extern "C" {

int fm_flow_residual_blocks(int height, int width, int* blocks) {
  if (!fm::flow_residual_blocks_args_ok(height, width, blocks)) return 1;
  blocks[0] = (int)fm::flow_residual_blocks((long)height * width);
  return 0;
}

int fm_flow_residuals(const float* depth, const float* k, const float* kinv, const float* t_fwd, const float* t_bwd, const float* flow_fwd,
                      const float* flow_bwd, const float* mask_fwd, const float* mask_bwd, int batch, int frames, int height, int width,
                      int mapping_kind, float delta, float aspect_x, float aspect_y, int first_pair, int count, float* residual_fwd,
                      float* residual_bwd, float* pred_fwd, float* pred_bwd, double* pair_sum, double* pair_valid, double* workspace,
                      const fm_layout* layouts, void*) {
  if (!fm::flow_residuals_args_ok(depth, k, kinv, t_fwd, t_bwd, flow_fwd, flow_bwd, mask_fwd, mask_bwd, batch, frames, height, width, mapping_kind, aspect_x,
                                  aspect_y, first_pair, count, residual_fwd, residual_bwd, pred_fwd, pred_bwd, pair_sum, pair_valid, workspace))
    return 1;
  const bool sums = pair_sum != nullptr;
  long fs[5], bs[5];
  if (!fm::flow_strides(layouts, batch, frames, (long)height * width, fs, bs)) return 1;
  const float* const flow[2] = {flow_fwd, flow_bwd};
  const float* const mask[2] = {sums ? mask_fwd : nullptr, sums ? mask_bwd : nullptr};
  float* const res[2] = {residual_fwd, residual_bwd};
  float* const pred[2] = {pred_fwd, pred_bwd};
#define FM_RES_HOST(K) \
  fm::residuals_host::run<fm::K>(depth, k, kinv, t_fwd, t_bwd, flow, mask, batch, frames, height, width, delta, aspect_x, aspect_y, first_pair, count, res, pred, pair_sum, pair_valid, fs, bs)
  if (mapping_kind == fm::kHuber) FM_RES_HOST(kHuber);
  else if (mapping_kind == fm::kL1) FM_RES_HOST(kL1);
  else FM_RES_HOST(kL2);
#undef FM_RES_HOST
  return 0;
}

}  // extern "C"
