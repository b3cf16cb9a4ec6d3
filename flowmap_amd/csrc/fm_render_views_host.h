// The rendered views (include/flowmap_hip.h, ABI version 14) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  Per source pixel it calls render_splat_at, render_key and
// render_footprint, per pair depth_consistency_pose (fm_math.h), the very functions the device kernels (fm_render_views.hip) call; the
// z-buffer is the same 64-bit keys in the same workspace, lowered serially in pair and pixel order — the minimum does not depend on the
// order, which is the point of the key.
#pragma once

#include <cstddef>
#include <cstring>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"

extern "C" {

int fm_render_views_workspace(int batch, int views, int out_height, int out_width, int n_pairs, long* bytes) {
  if (!fm::render_views_workspace_args_ok(batch, views, out_height, out_width, n_pairs, bytes)) return 1;
  bytes[0] = fm::render_views_workspace_bytes(batch, views, (long)out_height * out_width, n_pairs);
  return 0;
}

int fm_render_views(const float* depth, const float* kinv, const float* ext, const float* colors, const float* view_k, const float* view_ext,
                    const int32_t* pairs, int n_pairs, int batch, int frames, int height, int width, int views, int out_height, int out_width, int radius,
                    float near, float background, float* color, float* out_depth, int32_t* source, void* workspace, void*) {
  if (!fm::render_views_args_ok(depth, kinv, ext, colors, view_k, view_ext, pairs, n_pairs, batch, frames, height, width, views, out_height, out_width,
                                radius, near, background, color, out_depth, source, workspace))
    return 1;
  const size_t n = (size_t)height * width, out_pixels = (size_t)out_height * out_width, total = (size_t)batch * views * out_pixels;
  unsigned long long* zbuf = static_cast<unsigned long long*>(workspace);
  float* rel = reinterpret_cast<float*>(static_cast<char*>(workspace) + fm::render_views_key_bytes(batch, views, (long)out_pixels));
  memset(zbuf, 0xFF, total * 8);
  for (int b = 0; b < batch; ++b)
    for (int pair = 0; pair < n_pairs; ++pair) {
      const int view = pairs[2 * pair], src = pairs[2 * pair + 1];
      float* rel16 = rel + ((size_t)b * n_pairs + pair) * 16;
      if (view < 0 || view >= views || src < 0 || src >= frames) {
        for (int e = 0; e < 16; ++e) rel16[e] = 0.f;
        continue;
      }
      fm::depth_consistency_pose(ext + ((size_t)b * frames + src) * 16, view_ext + ((size_t)b * views + view) * 16, rel16);
      fm::Mat3 ki, kv;
      fm::Pose t;
      fm::load_mat3(kinv + ((size_t)b * frames + src) * 9, ki);
      fm::load_mat3(view_k + ((size_t)b * views + view) * 9, kv);
      fm::load_pose44(rel16, t);
      const float* z = depth + ((size_t)b * frames + src) * n;
      unsigned long long* zb = zbuf + ((size_t)b * views + view) * out_pixels;
      for (int r = 0; r < height; ++r)
        for (int c = 0; c < width; ++c) {
          const size_t px = (size_t)r * width + c;
          float ray[3];
          fm::ray_dir(ki, fm::pixel_center(c, width), fm::pixel_center(r, height), ray);
          const fm::RenderSplat s = fm::render_splat_at(ray, z[px], t, kv, near, out_height, out_width);
          if (!s.live) continue;
          const unsigned long long key = fm::render_key(s.qz, (unsigned int)((size_t)src * n + px));
          fm::render_footprint(s, radius, out_height, out_width, [&](size_t at) { zb[at] = key < zb[at] ? key : zb[at]; });
        }
    }
  for (size_t t = 0; t < total; ++t) {
    const unsigned long long key = zbuf[t];
    const bool hole = key == fm::kRenderHole;
    const unsigned int index = (unsigned int)(key & 0xffffffffULL);
    source[t] = hole ? -1 : (int32_t)index;
    out_depth[t] = hole ? 0.f : __builtin_bit_cast(float, (unsigned int)(key >> 32));
    if (color) {
      const size_t bv = t / out_pixels, at = t - bv * out_pixels, b = bv / views;
      const size_t frame = hole ? 0 : index / n, px = hole ? 0 : index - frame * n;
      for (int c = 0; c < 3; ++c)
        color[(bv * 3 + c) * out_pixels + at] = hole ? background : colors[((b * frames + frame) * 3 + c) * n + px];
    }
  }
  return 0;
}

}  // extern "C"
