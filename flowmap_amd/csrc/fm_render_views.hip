// Rendered views (projection.render_views; include/flowmap_hip.h: fm_render_views): the depth maps of a list of source frames splatted
// into any camera with a z-buffer — a FORWARD warp: many source pixels compete for one target pixel and the nearest wins.
//
// The z-buffer is one 64-bit key per target pixel, float_bits(q.z) << 32 | absolute source index (fm_math.h: render_key), filled with
// all-ones and lowered with atomic minima: the smallest q.z wins, among equal q.z the lower index.  The result is a function of the SET of
// candidates, never of their arrival order: bit-reproducible by construction.
//
// render_poses_kernel: one thread per (batch entry, pair) row forms E_v⁻¹·E_i in fp64 (fm_math.h: depth_consistency_pose) and flags a
// row whose pair does not name a view and a frame of this call (row[15] = 0: the splat pass skips it, nothing is indexed with it).
//
// render_splat_kernel: the geometry of depth_consistency_kernel.  A workgroup of 256 threads owns kRenderSplatTile = 1024 consecutive
// pixels of ONE (batch entry, pair); a thread loads four adjacent pixels (one 16-byte depth load when width % 4 == 0 and the base is
// aligned, else a scalar, bounds-checked path).  Per source pixel it moves 4 bytes of depth in and, when live, reads the key of every
// covered target pixel and lowers it with one no-return 8-byte atomic minimum unless it is already smaller; nothing else is written.
// The pose row and K_v are uniform loads.  The atomics are the bound, and they are issued lane-contiguously — a
// wave's 64 minima of one round go to neighbouring keys —, which is why the 16-byte path hands its depth round through 4 KB of LDS (one
// barrier); the scalar path loads in that order to begin with.
//
// render_resolve_kernel: one thread per target pixel decodes the key, gathers the three colour planes of the winner and writes color,
// depth and source — every output element, holes included.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_residual_args.h"

namespace fm {

constexpr int kRenderThreads = 256;
constexpr int kRenderSplatTile = kRenderThreads * 4;  // source pixels per workgroup: one quad per thread
static_assert(kRenderSplatTile == kRenderTile, "fm_residual_args.h states the tile");

struct RenderParams {
  const float* depth;
  const float* kinv;
  const float* view_k;
  const int32_t* pairs;  // (n_pairs, 2): view, source frame
  const float* rel;      // (B, n_pairs, 16)
  unsigned long long* zbuf;  // (B, V, OH, OW)
  int n_pairs, frames, height, width, views, out_height, out_width, radius;
  float near;
};

struct RenderPoseParams {
  const float* ext;
  const float* view_ext;
  const int32_t* pairs;
  float* rel;
  int n_pairs, frames, views, rows;
};

struct RenderResolveParams {
  const unsigned long long* zbuf;
  const float* colors;  // (B, F, 3, H, W) or null
  float* color;         // (B, V, 3, OH, OW) or null
  float* out_depth;
  int32_t* source;
  size_t total;  // B·V·OH·OW
  int frames, views;
  unsigned int pixels, out_pixels;
  float background;
};

__global__ void __launch_bounds__(kWave) render_poses_kernel(RenderPoseParams p) {
  const int row = blockIdx.x * kWave + threadIdx.x;  // [b][pair]
  if (row >= p.rows) return;
  const int b = row / p.n_pairs, pair = row - b * p.n_pairs;
  const int view = p.pairs[2 * pair], src = p.pairs[2 * pair + 1];
  float* out = p.rel + (size_t)row * 16;
  if (view < 0 || view >= p.views || src < 0 || src >= p.frames) {
    for (int e = 0; e < 16; ++e) out[e] = 0.f;
    return;
  }
  float m[16];
  depth_consistency_pose(p.ext + ((size_t)b * p.frames + src) * 16, p.view_ext + ((size_t)b * p.views + view) * 16, m);
  for (int e = 0; e < 16; ++e) out[e] = m[e];
}

template <int VEC>
__global__ void __launch_bounds__(kRenderThreads) render_splat_kernel(RenderParams p) {
  const int row = blockIdx.y;  // batch entry x pair
  const int b = row / p.n_pairs, pair = row - b * p.n_pairs;
  const int view = p.pairs[2 * pair], src = p.pairs[2 * pair + 1];  // (uniform)
  const float* rel16 = p.rel + (size_t)row * 16;
  if (view < 0 || view >= p.views || src < 0 || src >= p.frames || rel16[15] == 0.f) return;  // (uniform: no such pair)
  const int n = p.height * p.width;
  const int tile0 = blockIdx.x * kRenderSplatTile;  // (< n: the grid is render_blocks(n))
  const float* depth = p.depth + ((size_t)b * p.frames + src) * n;

  // The workgroup's depth comes in with one 16-byte load per thread (VEC == 4) and is handed round through LDS, because the atomics
  // want the OTHER order: in round e lane l of a wave takes pixel e·256 + wave·64 + l, so a wave's 64 minima go to (nearly) adjacent
  // keys — 512 bytes, eight 64-byte atomic requests — where four adjacent pixels per lane spread them over 2 KB, thirty-two requests.
  __shared__ float staged[VEC == 4 ? kRenderSplatTile : 1];
  if (VEC == 4) {  // width % 4 == 0: the quad lies inside the frame or past it, the base is 16-byte aligned
    const int px0 = tile0 + (int)threadIdx.x * 4;
    if (px0 < n) *reinterpret_cast<float4*>(&staged[threadIdx.x * 4]) = *reinterpret_cast<const float4*>(depth + px0);
    __syncthreads();  // (every thread of the workgroup arrives: the returns above are uniform)
  }

  Mat3 kinv, kv;
  Pose rel;
  load_mat3(p.kinv + ((size_t)b * p.frames + src) * 9, kinv);
  load_mat3(p.view_k + ((size_t)b * p.views + view) * 9, kv);
  load_pose44(rel16, rel);

  unsigned long long* zbuf = p.zbuf + ((size_t)b * p.views + view) * ((size_t)p.out_height * p.out_width);
  const unsigned int index0 = (unsigned int)src * (unsigned int)n;  // (frames·height·width < 2^31)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int local = e * kRenderThreads + (int)threadIdx.x, px = tile0 + local;
    if (px >= n) break;
    const float z = VEC == 4 ? staged[local] : depth[px];
    const int r = px / p.width, c = px - r * p.width;
    float ray[3];
    ray_dir(kinv, pixel_center(c, p.width), pixel_center(r, p.height), ray);
    const RenderSplat s = render_splat_at(ray, z, rel, kv, p.near, p.out_height, p.out_width);
    if (!s.live) continue;
    const unsigned long long key = render_key(s.qz, index0 + (unsigned int)px);
    render_footprint(s, p.radius, p.out_height, p.out_width, [&](size_t at) {
      // keys only fall: a key that is already smaller — even a stale copy of it — means this candidate has lost, without an atomic
      if (zbuf[at] <= key) return;
      __hip_atomic_fetch_min(&zbuf[at], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (result unused: a no-return atomic)
    });
  }
}

__global__ void __launch_bounds__(kRenderThreads) render_resolve_kernel(RenderResolveParams p) {
  const size_t t = (size_t)blockIdx.x * kRenderThreads + threadIdx.x;  // [b][view][y][x]
  if (t >= p.total) return;
  const unsigned long long key = p.zbuf[t];
  const unsigned int index = (unsigned int)(key & 0xffffffffULL);
  const bool hole = key == kRenderHole || index >= (unsigned int)p.frames * p.pixels;
  p.source[t] = hole ? -1 : (int32_t)index;
  p.out_depth[t] = hole ? 0.f : __builtin_bit_cast(float, (unsigned int)(key >> 32));
  if (p.color) {
    const size_t bv = t / p.out_pixels, at = t - bv * p.out_pixels, b = bv / p.views;
    const unsigned int frame = hole ? 0u : index / p.pixels, px = hole ? 0u : index - frame * p.pixels;
    const float* from = p.colors + ((b * p.frames + frame) * 3) * (size_t)p.pixels + px;
    float* to = p.color + bv * 3 * (size_t)p.out_pixels + at;
#pragma unroll
    for (int c = 0; c < 3; ++c) to[(size_t)c * p.out_pixels] = hole ? p.background : from[(size_t)c * p.pixels];
  }
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_render_views_workspace(int batch, int views, int out_height, int out_width, int n_pairs, long* bytes) {
  FM_CHECK_ARG(render_views_workspace_args_ok(batch, views, out_height, out_width, n_pairs, bytes));
  bytes[0] = render_views_workspace_bytes(batch, views, (long)out_height * out_width, n_pairs);
  return FM_OK;
}

int fm_render_views(const float* depth, const float* kinv, const float* ext, const float* colors, const float* view_k, const float* view_ext,
                    const int32_t* pairs, int n_pairs, int batch, int frames, int height, int width, int views, int out_height, int out_width, int radius,
                    float near, float background, float* color, float* out_depth, int32_t* source, void* workspace, void* stream) {
  FM_CHECK_ARG(render_views_args_ok(depth, kinv, ext, colors, view_k, view_ext, pairs, n_pairs, batch, frames, height, width, views, out_height, out_width,
                                    radius, near, background, color, out_depth, source, workspace));
  FM_CHECK_ARG(aligned(workspace, 8));
  const long n = (long)height * width, out_pixels = (long)out_height * out_width;
  const long key_bytes = render_views_key_bytes(batch, views, out_pixels);
  unsigned long long* zbuf = static_cast<unsigned long long*>(workspace);
  float* rel = reinterpret_cast<float*>(static_cast<char*>(workspace) + key_bytes);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(zbuf, 0xFF, (size_t)key_bytes, st) != hipSuccess) return FM_ERR_LAUNCH;
  if (n_pairs > 0) {
    RenderPoseParams q{ext, view_ext, pairs, rel, n_pairs, frames, views, batch * n_pairs};
    hipLaunchKernelGGL(render_poses_kernel, dim3((unsigned)((q.rows + kWave - 1) / kWave)), dim3(kWave), 0, st, q);
    RenderParams p{depth, kinv, view_k, pairs, rel, zbuf, n_pairs, frames, height, width, views, out_height, out_width, radius, near};
    const dim3 grid((unsigned)render_blocks(n), (unsigned)(batch * n_pairs));
    if (width % 4 == 0 && aligned(depth, 16)) hipLaunchKernelGGL(render_splat_kernel<4>, grid, dim3(kRenderThreads), 0, st, p);
    else hipLaunchKernelGGL(render_splat_kernel<1>, grid, dim3(kRenderThreads), 0, st, p);
  }
  RenderResolveParams r{zbuf, colors, color, out_depth, source, (size_t)batch * views * out_pixels, frames, views, (unsigned int)n, (unsigned int)out_pixels,
                        background};
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((r.total + kRenderThreads - 1) / kRenderThreads)), dim3(kRenderThreads), 0, st, r);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
