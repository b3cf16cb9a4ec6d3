// Tracking residual maps (LossTracking.residuals; include/flowmap_hip.h: fm_track_residuals): per (source frame fs, target frame ft,
// point p) of a WINDOW of track segments the unmasked term of LossTracking.compute_unweighted_loss (flowmap/loss/loss_tracking.py:48-56),
// the visibility compute_track_flow returns (flowmap/model/projection.py:291-296), optionally the reprojected positions, and the
// per-pair and per-track masked sums — straight from depth, in one store-bound launch plus two tiny ones.  A diagnostic pass: the hot
// path (fm_track.hip) reduces all of this to one scalar and never forms the (f, f, P) tensors written here.
//
// A workgroup of 256 threads owns up to 256 consecutive points of ONE (segment, source frame); its four waves never synchronise.  A
// thread samples its source point once (track_source_point: four taps of the depth image, X_w = E_fs·[xyz; 1]) and walks the
// segment's target frames: the twelve scaled target constants come from a table a small launch fills first (wave-uniform loads),
// xy[ft, p] and vis[ft, p] are coalesced loads, residual / visible / xy_target[fs, ft, p] coalesced stores — 5 (13 with the positions)
// bytes out and 9 in per element; the arithmetic is track_residual_at (fm_pose.h), the forward half of the hot path's pair term.
// Lanes beyond the segment's points work on a clamped point and store nothing; waves and workgroups with no point return at once.
//
// The sums use no atomics.  A term is `visible ? (double)ρ : 0.0` — a select, never a product.  Per (fs, ft) a wave adds its 64 terms
// in a butterfly (the count is a popcount of the ballot) and lane 0 leaves them in the wave's own workspace slot
// [fs][ft][chunk of 64 points]; per (fs, p) a thread adds its terms over ft in ascending order into its own slot [fs][p].  A second
// launch adds a pair's chunks in ascending order and a point's source frames in ascending order.  Which points a chunk holds depends
// on the segment alone — not on the window, not on the other segments — so a segment's sums are the same bits however it is reached.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_pose.h"
#include "fm_residual_args.h"

namespace fm {

constexpr int kTrResThreads = kTrackResThreads;
static_assert(kTrackResChunk == kWave, "a workspace slot per wave (fm_residual_args.h: track_res_chunks, track_res_work)");

struct TrackResParams {
  const float* depth;
  const float* kinv;
  const float* ext;
  const float* ext_inv;
  const float* k;
  const float* xy;
  const uint8_t* vis;
  const int32_t* seg;  // (S, 4): start_frame, f, p, offset (in points)
  const float* tgt;    // (frames, kTrackTgt): track_target + track_scale_target
  float* residual;
  uint8_t* visible;
  float* xy_target;  // (null: no positions)
  double* work;      // (null: no sums)
  double* pair_sum;
  double* pair_count;
  double* track_sum;
  double* track_count;
  int frames, first, count, fmax, height, width;
  float delta, ax, ay;
};

// Where segment sg's share of every output starts: the segments of the window lie one after the other.
struct SegPlace {
  size_t elems, pairs, points, work;
};
__device__ __forceinline__ SegPlace place_of(const int32_t* seg, int first, int sg) {
  SegPlace o{0, 0, 0, 0};
  for (int s = first; s < sg; ++s) {
    const size_t f = (size_t)seg[s * 4 + 1], p = (size_t)seg[s * 4 + 2];
    o.elems += f * f * p;
    o.pairs += f * f;
    o.points += p;
    o.work += (size_t)track_res_work((long)f, (long)p);
  }
  return o;
}

__global__ void __launch_bounds__(64) track_residual_targets_kernel(const float* ext_inv, const float* k, int frames, float ax, float ay, float* tgt) {
  const int fr = blockIdx.x * blockDim.x + threadIdx.x;
  if (fr >= frames) return;
  float tg[kTrackTgt], ts[kTrackTgt];
  track_target(ext_inv + (size_t)fr * 16, k + (size_t)fr * 9, tg);
  track_scale_target(tg, ax, ay, ts);
  for (int i = 0; i < kTrackTgt; ++i) tgt[(size_t)fr * kTrackTgt + i] = ts[i];
}

template <int KIND>
__global__ void __launch_bounds__(kTrResThreads) track_residuals_kernel(TrackResParams a) {
  const int sl = blockIdx.x / a.fmax, fs = blockIdx.x - sl * a.fmax, sg = a.first + sl;
  const int start = a.seg[sg * 4], f = a.seg[sg * 4 + 1], pc = a.seg[sg * 4 + 2], off = a.seg[sg * 4 + 3];
  if (fs >= f || start < 0 || start + f > a.frames) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int chunk = blockIdx.y * (kTrResThreads / kWave) + (threadIdx.x >> 6);
  if ((long)chunk * kWave >= pc) return;  // (wave-uniform; the waves of a workgroup share nothing)
  const int p = chunk * kWave + lane;
  const bool live = p < pc;
  const int pp = live ? p : pc - 1;
  const SegPlace at = place_of(a.seg, a.first, sg);
  const int chunks = (int)track_res_chunks(pc);

  const size_t src = (size_t)off + (size_t)fs * pc + pp;
  const float2 q = reinterpret_cast<const float2*>(a.xy)[src];
  float xw[3];
  track_source_point(a.depth + (size_t)(start + fs) * a.height * a.width, a.kinv + (size_t)(start + fs) * 9, a.ext + (size_t)(start + fs) * 16, q.x,
                     q.y, a.height, a.width, xw);
  const bool source = live && a.vis[src] != 0 && q.x >= 0.f && q.y >= 0.f && q.x < 1.f && q.y < 1.f;
  const float inv_delta = KIND == kHuber ? 1.0f / a.delta : 0.f;
  const bool sums = a.work != nullptr;  // (uniform: a kernel argument)
  double2* pair_slots = reinterpret_cast<double2*>(a.work + at.work);
  double tsum = 0.0, tcnt = 0.0;

  for (int ft = 0; ft < f; ++ft) {
    float ts[kTrackTgt];
#pragma unroll
    for (int i = 0; i < kTrackTgt; ++i) ts[i] = a.tgt[(size_t)(start + ft) * kTrackTgt + i];
    const size_t dst = (size_t)off + (size_t)ft * pc + pp;
    const float2 g = reinterpret_cast<const float2*>(a.xy)[dst];
    const bool target = a.vis[dst] != 0;
    const TrackResidual r = track_residual_at<KIND>(ts, xw, g.x * a.ax, g.y * a.ay, a.delta, inv_delta, a.ax, a.ay,
                                                    a.ext_inv + (size_t)(start + ft) * 16, a.k + (size_t)(start + ft) * 9);
    const bool visible = source && target && r.inside;
    if (live) {
      const size_t o = at.elems + ((size_t)fs * f + ft) * pc + p;
      a.residual[o] = r.rho;
      a.visible[o] = visible ? 1 : 0;
      if (a.xy_target) reinterpret_cast<float2*>(a.xy_target)[o] = make_float2(r.u, r.v);
    }
    if (sums) {
      const double term = visible ? (double)r.rho : 0.0;
      tsum += term;
      tcnt += visible ? 1.0 : 0.0;
      const double wave_total = wave_sum(term);
      const double wave_count = (double)__popcll(__ballot(visible));
      if (lane == 0) pair_slots[((size_t)fs * f + ft) * chunks + chunk] = make_double2(wave_total, wave_count);
    }
  }
  if (sums && live) pair_slots[(size_t)f * f * chunks + (size_t)fs * pc + p] = make_double2(tsum, tcnt);
}

// blockIdx.z = 0: one thread per (fs, ft) of a segment adds the pair's chunk partials in ascending chunk order; 1: one thread per point
// adds its per-source-frame partials in ascending fs order.  (The order IS the contract.)
__global__ void __launch_bounds__(kTrResThreads) track_residual_sums_kernel(TrackResParams a) {
  const int sg = a.first + blockIdx.x;
  const int start = a.seg[sg * 4], f = a.seg[sg * 4 + 1], pc = a.seg[sg * 4 + 2];
  if (start < 0 || start + f > a.frames) return;
  const SegPlace at = place_of(a.seg, a.first, sg);
  const int chunks = (int)track_res_chunks(pc);
  const double2* slots = reinterpret_cast<const double2*>(a.work + at.work);
  const size_t i = (size_t)blockIdx.y * kTrResThreads + threadIdx.x;
  double s = 0.0, c = 0.0;
  if (blockIdx.z == 0) {
    if (i >= (size_t)f * f) return;
    for (int ch = 0; ch < chunks; ++ch) {
      const double2 v = slots[i * chunks + ch];
      s += v.x;
      c += v.y;
    }
    a.pair_sum[at.pairs + i] = s;
    a.pair_count[at.pairs + i] = c;
  } else {
    if (i >= (size_t)pc) return;
    const double2* mine = slots + (size_t)f * f * chunks;
    for (int fs = 0; fs < f; ++fs) {
      const double2 v = mine[(size_t)fs * pc + i];
      s += v.x;
      c += v.y;
    }
    a.track_sum[at.points + i] = s;
    a.track_count[at.points + i] = c;
  }
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_track_residual_workspace(int frames, int points, long* doubles) {
  FM_CHECK_ARG(track_residual_workspace_args_ok(frames, points, doubles));
  doubles[0] = track_res_work(frames, points);
  return FM_OK;
}

int fm_track_residuals(const float* depth, const float* kinv, const float* ext, const float* ext_inv, const float* k, int frames, const float* xy,
                       const uint8_t* vis, const int32_t* seg, int first_segment, int count, int pmax, int fmax, int height, int width,
                       int mapping_kind, float delta, float aspect_x, float aspect_y, float* tgt, float* residual, uint8_t* visible,
                       float* xy_target, double* pair_sum, double* pair_count, double* track_sum, double* track_count, double* workspace,
                       void* stream) {
  FM_CHECK_ARG(track_residuals_args_ok(depth, kinv, ext, ext_inv, k, frames, xy, vis, seg, first_segment, count, pmax, fmax, height, width, mapping_kind,
                                       aspect_x, aspect_y, tgt, residual, visible, pair_sum, pair_count, track_sum, track_count, workspace));
  const bool sums = pair_sum != nullptr;
  const long point_blocks = track_res_point_blocks(pmax), sum_blocks = track_res_sum_blocks(pmax, fmax);
  FM_CHECK_ARG(!sums || (reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  FM_CHECK_ARG((reinterpret_cast<uintptr_t>(xy) & 7) == 0 && (!xy_target || (reinterpret_cast<uintptr_t>(xy_target) & 7) == 0));
  TrackResParams a{depth, kinv, ext, ext_inv, k, xy, vis, seg, tgt, residual, visible, xy_target, workspace, pair_sum, pair_count, track_sum, track_count,
                   frames, first_segment, count, fmax, height, width, delta, aspect_x, aspect_y};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(track_residual_targets_kernel, dim3((frames + 63) / 64), dim3(64), 0, st, ext_inv, k, frames, aspect_x, aspect_y, tgt);
  const dim3 grid((unsigned)((long)count * fmax), (unsigned)point_blocks);
  if (mapping_kind == kHuber) hipLaunchKernelGGL((track_residuals_kernel<kHuber>), grid, dim3(kTrResThreads), 0, st, a);
  else if (mapping_kind == kL1) hipLaunchKernelGGL((track_residuals_kernel<kL1>), grid, dim3(kTrResThreads), 0, st, a);
  else hipLaunchKernelGGL((track_residuals_kernel<kL2>), grid, dim3(kTrResThreads), 0, st, a);
  if (sums) hipLaunchKernelGGL(track_residual_sums_kernel, dim3((unsigned)count, (unsigned)sum_blocks, 2), dim3(kTrResThreads), 0, st, a);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
