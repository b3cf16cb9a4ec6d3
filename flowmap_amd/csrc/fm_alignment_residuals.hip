// Alignment residual maps (ExtrinsicsProcrustes.residuals; include/flowmap_hip.h: fm_alignment_residuals): per element and pair the
// term of the objective the Procrustes fit minimises, ‖T·p − q‖² (flowmap/model/procrustes.py:7-51) over the correspondences of
// align_surfaces (flowmap/model/projection.py:213-252), optionally the offset T·p − q and the weight, and the per-pair weighted sums —
// for a WINDOW of pairs, in one gather-bound launch plus one tiny one.
//
// The element is corr_load_with (fm_math.h): the fit's own per-correspondence function, depth-sourced (depth_*, K⁻¹: lazy surfaces) or
// surface-sourced (surf_*: an explicit tensor) — ONE kernel, two sources, as the fit has them.  A workgroup of 256 threads owns
// kAlignTile = 1024 consecutive elements of ONE (batch entry, pair); a thread owns kAlignPer = 4 consecutive ones.  Per element it
// reads 4 bytes of the later depth, 8 of flow, 4 of weight and four taps of the earlier depth (neighbouring pixels share taps: mostly
// L2) and writes 4 (residual) to 20 (offset, weight) bytes.  Lanes past the end store nothing; every output element is written.
// Nothing is staged in LDS; the only LDS is the 64 bytes of the block reduction.  A thread evaluates its four elements before it
// stores any of them, and depth-sourced it reads their sixteen tap depths together, ahead of corr_load_with (see the kernel).
//
// The sums use no atomics: a thread adds (double)(w·residual) — the fp32 product — and (double)w of its elements in fp64, and the ordered
// two-stage sum of fm_ordered_sums.h takes them from there — the workgroup's slot is [b][pair][tile], a row a (batch entry, pair).  Which
// elements a tile owns depends on the number of elements only, so a pair's sums are the same bits however it is reached.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_ordered_sums.h"
#include "fm_residual_args.h"

namespace fm {

constexpr int kAlignThreads = 256;
constexpr int kAlignPer = 4;                             // consecutive elements per thread
constexpr int kAlignTile = kAlignThreads * kAlignPer;    // elements per workgroup
static_assert(kAlignTile == kAlignResTile, "fm_residual_args.h sizes the workspace");

struct AlignParams {
  const float* depth;      // (B,F,H,W)     [depth-sourced]
  const float* kinv;       // (B,F,3,3)     [depth-sourced]
  const float* surfaces;   // (B,F,H,W,3)   [surface-sourced]
  const float* bwd_flow;   // (B,F-1,H,W,2)
  const float* weights;    // (B,F-1,H,W), or null: weight 1
  const float* rel;        // (B,F-1,4,4) camera i+1 -> camera i
  const int64_t* indices;  // (points), or null: element j is pixel j
  float* residual;         // (B,count,points)
  float* offset;           // (B,count,points,3) or null
  float* weight_out;       // (B,count,points) or null
  double* work;            // (B,count,tiles,2) or null: no sums
  long points;
  int frames, height, width, first_pair, count, tiles;
  float weight_sens;
};

enum { ALIGN_DEPTH = 0, ALIGN_SURF = 1 };

template <int SRC>
__global__ void __launch_bounds__(kAlignThreads) alignment_residuals_kernel(AlignParams p) {
  const int bp = blockIdx.y;  // batch entry x pairs of the window
  const int b = bp / p.count;
  const int pair = p.first_pair + (bp - b * p.count);
  const int n = p.height * p.width;
  const size_t fe = (size_t)b * p.frames + pair;          // the earlier frame; the later one follows it
  const size_t pr = (size_t)b * (p.frames - 1) + pair;

  CorrSrc s;
  s.depth_e = SRC == ALIGN_DEPTH ? p.depth + fe * n : nullptr;
  s.depth_l = SRC == ALIGN_DEPTH ? p.depth + (fe + 1) * n : nullptr;
  s.surf_e = SRC == ALIGN_SURF ? p.surfaces + fe * n * 3 : nullptr;
  s.surf_l = SRC == ALIGN_SURF ? p.surfaces + (fe + 1) * n * 3 : nullptr;
  s.bwd_flow = p.bwd_flow + pr * n * 2;
  const bool weighted = p.weights != nullptr;  // (uniform: a kernel argument)
  // without weights corr_load_with still reads weights[idx]: it is pointed at the flow image (2n floats, so idx is inside) and the
  // value is replaced by 1 below
  s.weights = weighted ? p.weights + pr * n : s.bwd_flow;
  s.weight_sens = weighted ? p.weight_sens : 0.f;
  s.height = p.height;
  s.width = p.width;

  Mat3 kinv_e, kinv_l;
#pragma unroll
  for (int i = 0; i < 9; ++i) kinv_e.m[i] = kinv_l.m[i] = 0.f;
  if (SRC == ALIGN_DEPTH) {
    load_mat3(p.kinv + fe * 9, kinv_e);
    load_mat3(p.kinv + (fe + 1) * 9, kinv_l);
  }
  Pose t;
  load_pose44(p.rel + pr * 16, t);

  const bool sums = p.work != nullptr;  // (uniform)
  const size_t out0 = (size_t)bp * p.points;
  const long first = (long)blockIdx.x * kAlignTile + (long)threadIdx.x * kAlignPer;
  // All of a thread's elements are loaded and evaluated before the first store, in two stages, so that a thread waits for memory twice
  // and not once per load.  corr_load_with skips a tap outside the frame with a branch, and a load behind a branch is a round trip of
  // its own (flow -> tap -> tap -> tap -> tap, per element).  So stage 1 reads the index and the flow of every element of the thread,
  // and the four tap depths of every element together from addresses clamped into the frame (bilinear_taps already keeps the
  // north-west tap inside; the clamp folds a tap past the last row or column, which corr_load_with never asks for, onto it); stage 2
  // calls corr_load_with with a `tap` that hands out those registers — its contract allows a staged window — and finds the
  // flow, weight and later depth it reads itself in flight since stage 1 began (no store stands between the stages: the outputs may
  // alias the inputs as far as the compiler knows).  Surface-sourced, the taps are read inside corr_load_with as the fit reads them.
  int idx[kAlignPer], x0[kAlignPer], y0[kAlignPer];  // (x0, y0: the north-west tap as bilinear_taps gives it)
  float z[kAlignPer][4];
#pragma unroll
  for (int e = 0; e < kAlignPer; ++e) {
    const long j = first + e < p.points ? first + e : p.points - 1;  // (lanes past the end evaluate the last element and store nothing)
    idx[e] = alignment_pixel(p.indices ? (long)p.indices[j] : j, n);
  }
  if (SRC == ALIGN_DEPTH) {
#pragma unroll
    for (int e = 0; e < kAlignPer; ++e) {
      const PixelRef px = pixel_ref(idx[e], p.height, p.width);
      const Taps tp = bilinear_taps(px.u + s.bwd_flow[2 * (size_t)idx[e]], px.v + s.bwd_flow[2 * (size_t)idx[e] + 1], p.height, p.width);  // as corr_load_with
      x0[e] = tp.x0;
      y0[e] = tp.y0;
      const int xa = min(max(tp.x0, 0), p.width - 1), ya = min(max(tp.y0, 0), p.height - 1);
      const int xb = min(xa + 1, p.width - 1), yb = min(ya + 1, p.height - 1);
      z[e][0] = s.depth_e[ya * p.width + xa];
      z[e][1] = s.depth_e[ya * p.width + xb];
      z[e][2] = s.depth_e[yb * p.width + xa];
      z[e][3] = s.depth_e[yb * p.width + xb];
    }
  }
  float r[kAlignPer], wt[kAlignPer], d[kAlignPer][3];
#pragma unroll
  for (int e = 0; e < kAlignPer; ++e) {
    const Corr c = corr_load_with<false>(s, kinv_e, kinv_l, pixel_ref(idx[e], p.height, p.width), [&](int tr, int tc, float& ut, float& vt) {
      ut = pixel_center(tc, s.width);
      vt = pixel_center(tr, s.height);
      const int k = (tr - y0[e]) * 2 + (tc - x0[e]);  // (an inside tap is the north-west one or its neighbour: k in 0..3)
      return k == 0 ? z[e][0] : (k == 1 ? z[e][1] : (k == 2 ? z[e][2] : z[e][3]));
    });
    wt[e] = weighted ? c.w : 1.f;
    r[e] = alignment_offset(t, c.p, c.q, d[e]);
  }
  double sum_r = 0.0, sum_w = 0.0;
#pragma unroll
  for (int e = 0; e < kAlignPer; ++e) {
    const long j = first + e;
    if (j >= p.points) continue;
    p.residual[out0 + j] = r[e];
    if (p.offset) {
      float* o = p.offset + (out0 + j) * 3;
      o[0] = d[e][0];
      o[1] = d[e][1];
      o[2] = d[e][2];
    }
    if (p.weight_out) p.weight_out[out0 + j] = wt[e];
    sum_r += (double)(wt[e] * r[e]);
    sum_w += (double)wt[e];
  }

  if (!sums) return;  // (uniform)
  block_sum_to_slot<kAlignThreads>(sum_r, sum_w, p.work + 2 * ((size_t)bp * p.tiles + blockIdx.x));
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_alignment_residual_workspace(long points, long* doubles) {
  FM_CHECK_ARG(alignment_residual_workspace_args_ok(points, doubles));
  doubles[0] = 2 * alignment_residual_tiles(points);
  return FM_OK;
}

int fm_alignment_residuals(const float* depth, const float* kinv, const float* surfaces, const float* bwd_flow, const float* weights,
                           float weight_sensitivity, const float* rel, const int64_t* indices, long points, int batch, int frames,
                           int height, int width, int first_pair, int count, float* residual, float* offset, float* weight_out,
                           double* pair_sum, double* pair_weight, double* workspace, void* stream) {
  FM_CHECK_ARG(alignment_residuals_args_ok(depth, kinv, surfaces, bwd_flow, rel, indices, points, batch, frames, height, width, first_pair, count, residual,
                                           pair_sum, pair_weight, workspace));
  const bool sums = pair_sum != nullptr;
  FM_CHECK_ARG(!sums || (reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  AlignParams p{depth, kinv, surfaces, bwd_flow, weights, rel, indices, residual, offset, weight_out, sums ? workspace : nullptr};
  p.points = points;
  p.frames = frames, p.height = height, p.width = width, p.first_pair = first_pair, p.count = count;
  p.tiles = (int)alignment_residual_tiles(points);
  p.weight_sens = weight_sensitivity;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.tiles, (unsigned)(batch * count));
  if (depth) hipLaunchKernelGGL((alignment_residuals_kernel<ALIGN_DEPTH>), grid, dim3(kAlignThreads), 0, st, p);
  else hipLaunchKernelGGL((alignment_residuals_kernel<ALIGN_SURF>), grid, dim3(kAlignThreads), 0, st, p);
  if (sums)
    hipLaunchKernelGGL(ordered_slot_sums_kernel, dim3((unsigned)(batch * count)), dim3(kWave), 0, st, workspace, p.tiles, pair_sum, pair_weight);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
