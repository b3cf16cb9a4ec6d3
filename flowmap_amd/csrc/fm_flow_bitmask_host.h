// The bit-mask packed format of the fused flow loss (include/flowmap_hip.h, ABI version 7) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  The three bit-mask entry points are written here once,
// portably, ON TOP of the fp32-format entry points such a build already has: the masks are classified and packed serially, and the loss
// expands the bytes back into the fp32 packed layout and calls its namesake, so every residual sees the 0.0f / 1.0f the device kernel
// rebuilds from the bits and the rest is that build's own arithmetic.  No device code, no HIP.
#pragma once

#include <cstring>
#include <vector>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"

namespace fm {
namespace bitmask_host {

// a (batch, frames, per_frame) stack read through an fm_layout ({0, 0} / NULL = dense) into a dense vector: how the host builds of the
// `_views` entry points (here and in tests/host_sim) read a frame window
inline std::vector<float> densify(const float* p, const fm_layout* lay, int batch, int frames, size_t per_frame) {
  std::vector<float> out;
  if (!p) return out;
  long fs, bs;
  layout_strides(lay, 0, (long)per_frame, frames, fs, bs);
  out.resize((size_t)batch * frames * per_frame);
  for (int b = 0; b < batch; ++b)
    for (int f = 0; f < frames; ++f) std::memcpy(out.data() + ((size_t)b * frames + f) * per_frame, p + (size_t)b * bs + (size_t)f * fs, per_frame * sizeof(float));
  return out;
}

}  // namespace bitmask_host
}  // namespace fm

extern "C" {

int fm_flow_masks_binary(const float* mask_fwd, const float* mask_bwd, int batch, int pairs, long pixels, int* not_binary, const fm_layout* layouts,
                         void*) {
  if (!mask_fwd || !mask_bwd || !not_binary || batch < 1 || pairs < 1 || pixels < 1) return 1;
  const auto mf = fm::bitmask_host::densify(mask_fwd, layouts ? layouts + 0 : nullptr, batch, pairs, (size_t)pixels);
  const auto mb = fm::bitmask_host::densify(mask_bwd, layouts ? layouts + 1 : nullptr, batch, pairs, (size_t)pixels);
  const float one = 1.0f, zero = 0.0f;
  int other = 0;
  for (const auto* v : {&mf, &mb})
    for (const float& x : *v)
      if (std::memcmp(&x, &zero, sizeof(float)) != 0 && std::memcmp(&x, &one, sizeof(float)) != 0) other = 1;
  not_binary[0] = other;
  return 0;
}

int fm_flow_pack_inputs_bitmask(const float* flow_fwd, const float* flow_bwd, const float* mask_fwd, const float* mask_bwd, int batch, int frames,
                                int height, int width, uint8_t* packed, void*) {
  if (!flow_fwd || !flow_bwd || !mask_fwd || !mask_bwd || !packed || batch < 1 || frames < 2 || height < 1 || width < 1 || width % 4 != 0) return 1;
  const size_t n = (size_t)height * width, quads = n / 4, chunks = (quads + 63) / 64, stride = FM_FLOW_BITMASK_CHUNK_BYTES;
  std::memset(packed, 0, (size_t)batch * frames * chunks * stride);
  for (int b = 0; b < batch; ++b)
    for (int f = 0; f < frames; ++f)
      for (size_t q = 0; q < quads; ++q) {
        uint8_t* chunk = packed + (((size_t)b * frames + f) * chunks + q / 64) * stride;
        float* dst = reinterpret_cast<float*>(chunk) + (q % 64) * 4;
        const size_t pair = (size_t)b * (frames - 1) + f;
        unsigned bits = 0;
        for (int e = 0; e < 4; ++e) {
          if (f < frames - 1) {
            dst[0 * 256 + e] = flow_fwd[(pair * n + q * 4) * 2 + e];
            dst[1 * 256 + e] = flow_fwd[(pair * n + q * 4) * 2 + 4 + e];
            if (mask_fwd[pair * n + q * 4 + e] != 0.f) bits |= 1u << e;
          }
          if (f > 0) {
            dst[2 * 256 + e] = flow_bwd[((pair - 1) * n + q * 4) * 2 + e];
            dst[3 * 256 + e] = flow_bwd[((pair - 1) * n + q * 4) * 2 + 4 + e];
            if (mask_bwd[(pair - 1) * n + q * 4 + e] != 0.f) bits |= 16u << e;
          }
        }
        chunk[4096 + q % 64] = (uint8_t)bits;
      }
  return 0;
}

int fm_flow_pack_inputs_bitmask_views(const float* flow_fwd, const float* flow_bwd, const float* mask_fwd, const float* mask_bwd, int batch,
                                      int frames, int height, int width, uint8_t* packed, const fm_layout* layouts, void* stream) {
  if (!flow_fwd || !flow_bwd || !mask_fwd || !mask_bwd || !packed || batch < 1 || frames < 2 || height < 1 || width < 1) return 1;
  const size_t n = (size_t)height * width;
  const auto ff = fm::bitmask_host::densify(flow_fwd, layouts ? layouts + 0 : nullptr, batch, frames - 1, 2 * n);
  const auto fb = fm::bitmask_host::densify(flow_bwd, layouts ? layouts + 1 : nullptr, batch, frames - 1, 2 * n);
  const auto mf = fm::bitmask_host::densify(mask_fwd, layouts ? layouts + 2 : nullptr, batch, frames - 1, n);
  const auto mb = fm::bitmask_host::densify(mask_bwd, layouts ? layouts + 3 : nullptr, batch, frames - 1, n);
  return fm_flow_pack_inputs_bitmask(ff.data(), fb.data(), mf.data(), mb.data(), batch, frames, height, width, packed, stream);
}

int fm_flow_loss_fused_bitmask(float* depth, const float* k, const float* kinv, const float* t_fwd, const float* t_bwd, const uint8_t* packed,
                               const float* scale, int batch, int frames, int height, int width, int mapping_kind, float delta, float ax, float ay,
                               float* grad_depth, double* acc, int items, const fm_layout* depth_layout, const fm_flow_taps* taps, float* exp_avg,
                               float* exp_avg_sq, const uint8_t* touched, long step, double lr, double beta1, double beta2, double eps, void* stream) {
  if (!packed || !depth || !k || !kinv || !acc || batch < 1 || frames < 2 || height < 1 || width < 1 || width % 4 != 0) return 1;
  const bool view = fm::layout_is_view(depth_layout);
  if (view && (taps || exp_avg)) return 1;
  const size_t n = (size_t)height * width, quads = n / 4, chunks = (quads + 63) / 64, stride = FM_FLOW_BITMASK_CHUNK_BYTES;
  std::vector<float> wide((size_t)batch * frames * chunks * 6 * 64 * 4, 0.f);  // the fp32 packed layout of the same inputs
  for (size_t bf = 0; bf < (size_t)batch * frames; ++bf)
    for (size_t q = 0; q < quads; ++q) {
      const uint8_t* chunk = packed + (bf * chunks + q / 64) * stride;
      const float* src = reinterpret_cast<const float*>(chunk) + (q % 64) * 4;
      float* dst = wide.data() + ((bf * chunks + q / 64) * 6 * 64 + q % 64) * 4;
      const unsigned bits = chunk[4096 + q % 64];
      for (int e = 0; e < 4; ++e) {
        dst[0 * 256 + e] = src[0 * 256 + e];
        dst[1 * 256 + e] = src[1 * 256 + e];
        dst[2 * 256 + e] = (bits >> e) & 1u ? 1.f : 0.f;
        dst[3 * 256 + e] = src[2 * 256 + e];
        dst[4 * 256 + e] = src[3 * 256 + e];
        dst[5 * 256 + e] = (bits >> (4 + e)) & 1u ? 1.f : 0.f;
      }
    }
  if (taps)
    return fm_flow_loss_fused_taps(depth, k, kinv, t_fwd, t_bwd, nullptr, nullptr, nullptr, nullptr, wide.data(), scale, batch, frames, height, width,
                                   mapping_kind, delta, ax, ay, grad_depth, acc, items, taps, exp_avg, exp_avg_sq, touched, step, lr, beta1, beta2, eps, stream);
  if (exp_avg)
    return fm_flow_loss_fused_adam(depth, k, kinv, t_fwd, t_bwd, nullptr, nullptr, nullptr, nullptr, wide.data(), scale, batch, frames, height, width,
                                   mapping_kind, delta, ax, ay, grad_depth, acc, items, exp_avg, exp_avg_sq, touched, step, lr, beta1, beta2, eps, stream);
  if (exp_avg_sq || touched) return 1;
  fm_layout lay[5] = {};
  if (view) lay[0] = *depth_layout;
  return fm_flow_loss_fused_views(depth, k, kinv, t_fwd, t_bwd, nullptr, nullptr, nullptr, nullptr, wide.data(), scale, batch, frames, height, width,
                                  mapping_kind, delta, ax, ay, grad_depth, acc, items, view ? lay : nullptr, stream);
}

}  // extern "C"
