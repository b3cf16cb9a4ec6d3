// Depth consistency across frame offsets (projection.depth_consistency; include/flowmap_hip.h: fm_depth_consistency): per source pixel
// and offset d the relative error of frame i+d's depth, sampled where the pixel reprojects under the chained poses, against the depth
// the reprojection predicts — for a WINDOW of source frames, straight from depth, in one HBM-bound launch plus two tiny ones.
//
// depth_consistency_poses_kernel: one thread per (batch entry, source frame, offset) row forms E_j⁻¹·E_i in fp64 (fm_math.h:
// depth_consistency_pose) — the rows of the window only, no F×F table — and flags a row whose target frame does not exist.
//
// depth_consistency_kernel: a workgroup of 256 threads owns kConsTile = 1024 consecutive pixels of ONE (batch entry, source frame); a
// thread holds four adjacent pixels and loops over the offsets, so the source depth and the ray K_i⁻¹[u, v, 1] are loaded and formed
// once per pixel, not once per offset.  Per pixel it moves 4 bytes of depth in; per pixel and offset four target taps (bilinear_taps,
// through L2: adjacent source pixels land on adjacent target pixels, so a target frame is fetched from HBM about once — 4 bytes) and
// 4 + 1 bytes out (21 with the details).  The arithmetic is depth_consistency_at (fm_math.h), a few dozen VALU instructions, far below
// the memory time.  Nothing is staged in LDS; the only LDS is the 512 bytes of the block reduction (a wave's partial per offset: one
// barrier per workgroup, none inside the offset loop).  No atomics: a thread adds (double)|error| and the count of its code-0 pixels,
// and the ordered two-stage sum of fm_ordered_sums.h takes them from there — the
// workgroup's slot is [b][frame][offset][workgroup], a row a (batch entry, source frame, offset).  Which pixels a workgroup owns
// depends on (height, width) only, so a row's sums are the same bits however it is reached.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_ordered_sums.h"
#include "fm_residual_args.h"

namespace fm {

constexpr int kConsThreads = 256;
constexpr int kConsTile = kConsThreads * 4;  // pixels per workgroup: one quad per thread
static_assert(kConsTile == kDepthConsTile, "fm_residual_args.h sizes the workspace");

struct ConsistencyParams {
  const float* depth;
  const float* k;
  const float* kinv;
  const float* rel;  // (B, count, n_off, 16)
  float* error;
  uint8_t* code;
  float* positions;  // (null together with reprojected and sampled: no details)
  float* reprojected;
  float* sampled;
  uint8_t* support;  // (null: no tolerance)
  double* work;      // (null: no sums)
  int offsets[kDepthConsMaxOffsets];
  int n_off, frames, height, width, first_frame, count, blocks;
  float tolerance;
};

struct ConsistencyPoseParams {
  const float* ext;
  float* rel;
  int offsets[kDepthConsMaxOffsets];
  int n_off, frames, first_frame, count, rows;
};

__global__ void __launch_bounds__(kWave) depth_consistency_poses_kernel(ConsistencyPoseParams p) {
  const int row = blockIdx.x * kWave + threadIdx.x;  // [b][frame of the window][offset]
  if (row >= p.rows) return;
  const int o = row % p.n_off, bf = row / p.n_off;
  const int b = bf / p.count, i = p.first_frame + (bf - b * p.count);
  int d = 0;
#pragma unroll
  for (int s = 0; s < kDepthConsMaxOffsets; ++s) d = s == o ? p.offsets[s] : d;  // (no run-time index into the kernel argument)
  const int j = i + d;
  float* out = p.rel + (size_t)row * 16;
  if (j < 0 || j >= p.frames) {
    for (int e = 0; e < 16; ++e) out[e] = 0.f;
    return;
  }
  const float* ext = p.ext + (size_t)b * p.frames * 16;
  float m[16];
  depth_consistency_pose(ext + (size_t)i * 16, ext + (size_t)j * 16, m);
  for (int e = 0; e < 16; ++e) out[e] = m[e];
}

template <int VEC>
__global__ void __launch_bounds__(kConsThreads) depth_consistency_kernel(ConsistencyParams p) {
  const int bf = blockIdx.y;  // batch entry x source frames of the window
  const int b = bf / p.count;
  const int src = p.first_frame + (bf - b * p.count);
  const int n = p.height * p.width;
  const bool sums = p.work != nullptr;           // (uniform: kernel arguments)
  const bool details = p.positions != nullptr;  // (uniform)

  const int quad = blockIdx.x * kConsThreads + threadIdx.x;
  const int px0 = quad * 4;
  const bool any = px0 < n;  // (a thread past the frame still takes part in the block reduction)
  const float* depth = p.depth + ((size_t)b * p.frames + src) * n;

  float z[4], ray[4][3];
  bool live[4];
  {
    Mat3 kinv;
    load_mat3(p.kinv + ((size_t)b * p.frames + src) * 9, kinv);
    if (VEC == 4) {  // width % 4 == 0: the quad lies in one image row and inside the frame, every base is 16-byte aligned
      float4 z4 = make_float4(1.f, 1.f, 1.f, 1.f);
      if (any) z4 = *reinterpret_cast<const float4*>(depth + px0);
      z[0] = z4.x, z[1] = z4.y, z[2] = z4.z, z[3] = z4.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int px = px0 + e;
      live[e] = VEC == 4 ? any : px < n;
      if (VEC != 4) z[e] = live[e] ? depth[px] : 1.f;
      const int row = (live[e] ? px : 0) / p.width, col = (live[e] ? px : 0) - row * p.width;
      ray_dir(kinv, pixel_center(col, p.width), pixel_center(row, p.height), ray[e]);
    }
  }

  __shared__ RowPartials<kConsThreads, kDepthConsMaxOffsets> partials;
  int support[4] = {0, 0, 0, 0};
  for (int o = 0; o < p.n_off; ++o) {
    int d = 0;
#pragma unroll
    for (int s = 0; s < kDepthConsMaxOffsets; ++s) d = s == o ? p.offsets[s] : d;
    const int dst = src + d;
    const size_t row = (size_t)bf * p.n_off + o;
    const float* rel16 = p.rel + row * 16;
    const bool present = dst >= 0 && dst < p.frames && rel16[15] != 0.f;  // (uniform)
    float err[4], u[4], v[4], qz[4], zs[4];
    int code[4];
    double sum_e = 0.0, sum_n = 0.0;
    if (present) {
      Pose rel;
      Mat3 kj;
      load_pose44(rel16, rel);
      load_mat3(p.k + ((size_t)b * p.frames + dst) * 9, kj);
      const float* depth_j = p.depth + ((size_t)b * p.frames + dst) * n;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const DepthConsistencyTerm t = depth_consistency_at(ray[e], z[e], rel, kj, depth_j, p.height, p.width);
        err[e] = t.error, u[e] = t.u, v[e] = t.v, qz[e] = t.qz, zs[e] = t.sampled, code[e] = t.code;
        if (live[e] && t.code == 0) {
          sum_e += (double)fabsf(t.error);
          sum_n += 1.0;
          if (fabsf(t.error) <= p.tolerance) ++support[e];
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) err[e] = u[e] = v[e] = qz[e] = zs[e] = 0.f, code[e] = 1;
    }

    const size_t base = row * n;
    if (VEC == 4) {
      if (any) {
        *reinterpret_cast<float4*>(p.error + base + px0) = make_float4(err[0], err[1], err[2], err[3]);
        *reinterpret_cast<uint32_t*>(p.code + base + px0) = (uint32_t)code[0] | (uint32_t)code[1] << 8 | (uint32_t)code[2] << 16 | (uint32_t)code[3] << 24;
        if (details) {
          *reinterpret_cast<float4*>(p.positions + (base + px0) * 2) = make_float4(u[0], v[0], u[1], v[1]);
          *reinterpret_cast<float4*>(p.positions + (base + px0) * 2 + 4) = make_float4(u[2], v[2], u[3], v[3]);
          *reinterpret_cast<float4*>(p.reprojected + base + px0) = make_float4(qz[0], qz[1], qz[2], qz[3]);
          *reinterpret_cast<float4*>(p.sampled + base + px0) = make_float4(zs[0], zs[1], zs[2], zs[3]);
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!live[e]) continue;
        const size_t at = base + px0 + e;
        p.error[at] = err[e];
        p.code[at] = (uint8_t)code[e];
        if (details) {
          p.positions[at * 2] = u[e];
          p.positions[at * 2 + 1] = v[e];
          p.reprojected[at] = qz[e];
          p.sampled[at] = zs[e];
        }
      }
    }
    if (sums) wave_partial_to_lds(partials, o, sum_e, sum_n);  // (uniform; no barrier inside the loop)
  }
  if (sums)  // slot [b][frame][offset][workgroup]: an offset's slot lies `blocks` slots after the one before
    block_rows_to_slots(partials, p.n_off, p.work + 2 * ((size_t)bf * p.n_off * p.blocks + blockIdx.x), 2 * (size_t)p.blocks);

  if (p.support) {
    uint8_t* out = p.support + (size_t)bf * n;
    if (VEC == 4) {
      if (any) *reinterpret_cast<uint32_t*>(out + px0) = (uint32_t)support[0] | (uint32_t)support[1] << 8 | (uint32_t)support[2] << 16 | (uint32_t)support[3] << 24;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (live[e]) out[px0 + e] = (uint8_t)support[e];
    }
  }
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_depth_consistency_blocks(int height, int width, int* blocks) {
  FM_CHECK_ARG(depth_consistency_blocks_args_ok(height, width, blocks));
  blocks[0] = (int)depth_consistency_blocks((long)height * width);
  return FM_OK;
}

int fm_depth_consistency(const float* depth, const float* k, const float* kinv, const float* ext, const int32_t* offsets, int n_offsets, int batch,
                         int frames, int height, int width, int first_frame, int count, float tolerance, float* error, uint8_t* code,
                         float* positions, float* reprojected, float* sampled, uint8_t* support, double* frame_sum, double* frame_valid, float* rel,
                         double* workspace, void* stream) {
  FM_CHECK_ARG(depth_consistency_args_ok(depth, k, kinv, ext, offsets, n_offsets, batch, frames, height, width, first_frame, count, tolerance, error, code,
                                         positions, reprojected, sampled, support, frame_sum, frame_valid, rel, workspace));
  const bool sums = frame_sum != nullptr;
  FM_CHECK_ARG(!sums || aligned(workspace, 16));
  const long n = (long)height * width;
  ConsistencyParams p{depth, k, kinv, rel, error, code, positions, reprojected, sampled, support, workspace};
  ConsistencyPoseParams q{ext, rel};
  for (int i = 0; i < kDepthConsMaxOffsets; ++i) p.offsets[i] = q.offsets[i] = i < n_offsets ? offsets[i] : 0;
  p.n_off = q.n_off = n_offsets, p.frames = q.frames = frames, p.first_frame = q.first_frame = first_frame, p.count = q.count = count;
  p.height = height, p.width = width, p.blocks = (int)depth_consistency_blocks(n);
  p.tolerance = support ? tolerance : 0.f;
  q.rows = batch * count * n_offsets;
  bool vec4 = width % 4 == 0 && aligned(depth, 16) && aligned(error, 16) && aligned(code, 4) && (!support || aligned(support, 4));
  vec4 = vec4 && (!positions || (aligned(positions, 16) && aligned(reprojected, 16) && aligned(sampled, 16)));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_consistency_poses_kernel, dim3((unsigned)((q.rows + kWave - 1) / kWave)), dim3(kWave), 0, st, q);
  const dim3 grid((unsigned)p.blocks, (unsigned)(batch * count));
  if (vec4) hipLaunchKernelGGL(depth_consistency_kernel<4>, grid, dim3(kConsThreads), 0, st, p);
  else hipLaunchKernelGGL(depth_consistency_kernel<1>, grid, dim3(kConsThreads), 0, st, p);
  if (sums) hipLaunchKernelGGL(ordered_slot_sums_kernel, dim3((unsigned)q.rows), dim3(kWave), 0, st, workspace, p.blocks, frame_sum, frame_valid);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
