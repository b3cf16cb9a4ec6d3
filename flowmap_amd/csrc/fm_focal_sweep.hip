// The softmin focal sweep of ONE frame pair after another (IntrinsicsSoftmin.residuals; include/flowmap_hip.h: fm_focal_sweep): for every
// (batch entry, pair of the window, focal-length candidate) the Procrustes fit of the pair under the candidate's K (align_surfaces,
// flowmap/model/projection.py:213-252 -> align_rigid, flowmap/model/procrustes.py:7-51) and the weighted L1 error of the pose-induced
// backward flow at the sampled pixels (flowmap/model/intrinsics/intrinsics_softmin.py:105-125), then per (batch entry, pair) the softmin
// over the candidates, the blended K and the blended focal length (intrinsics_softmin.py:123-141) — two launches, depth-sourced only.
//
// focal_sweep_kernel: one workgroup of 256 threads per (batch entry, pair, candidate).  Pass 1 strides over the P correspondences with
// corr_load_with (fm_math.h), the fit's own per-correspondence function — the later pixel's depth, weight and flow and the four tap depths
// of the earlier frame; both frames take the candidate's K⁻¹ — and moments_add about the fit's shift (the later point of the middle
// sample): per-thread fp32 moments as in the fit, a wave butterfly, then the waves' totals in fp64 through LDS in wave order.  Thread 0
// finishes the moments and solves the pose (moments_finish, pose_solve_one: fp64), which goes to LDS and, when asked for, to `poses`.
// Pass 2 strides over the same correspondences with softmin_term under that pose (the operands are L2-hot), stores the per-point term
// when asked for, and sums it in fp64 from the element upward: thread, wave butterfly, waves in order.  One thread writes the sum.
// A workgroup owns its output elements: no atomics, no workspace; which elements a thread owns depends on P only, so a result is the same
// bits run to run and however its pair is reached (full range or window).
//
// focal_sweep_curve_kernel: one wave per (batch entry, pair), the arithmetic of softmin_blend_fwd_kernel (fm_points.hip) with lane-strided
// loops over the candidates.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_pose.h"
#include "fm_residual_args.h"

namespace fm {

constexpr int kSweepThreads = 256;
constexpr int kSweepWaves = kSweepThreads / kWave;

struct SweepParams {
  const float* depth;       // (B,F,H,W)
  const float* weights;     // (B,F-1,H,W) weights, or logits when weight_sens != 0
  const float* bwd_flow;    // (B,F-1,H,W,2)
  const int64_t* indices;   // (P)
  const float* cand_k;      // (N,3,3)
  const float* cand_kinv;   // (N,3,3)
  double* error;            // (B,count,N)
  float* poses;             // (B,count,N,4,4) or null
  float* point_error;       // (B,count,N,P) or null
  long points;
  int frames, height, width, first_pair, count, candidates;
  float weight_sens;
};

__global__ void __launch_bounds__(kSweepThreads) focal_sweep_kernel(SweepParams p) {
  __shared__ double red[kSweepWaves][kMomentCount];
  __shared__ double aux[kAuxStride];  // (pose_solve_one's by-products: written, never read)
  __shared__ float pose44[16];
  const int cand = blockIdx.x;
  const int bp = blockIdx.y;  // batch entry x pairs of the window
  const int b = bp / p.count;
  const int pair = p.first_pair + (bp - b * p.count);
  const int n = p.height * p.width;
  const size_t fe = (size_t)b * p.frames + pair;  // the earlier frame; the later one follows it
  const size_t pr = (size_t)b * (p.frames - 1) + pair;

  CorrSrc s;
  s.depth_e = p.depth + fe * n;
  s.depth_l = p.depth + (fe + 1) * n;
  s.surf_e = s.surf_l = nullptr;
  s.bwd_flow = p.bwd_flow + pr * n * 2;
  s.weights = p.weights + pr * n;
  s.weight_sens = p.weight_sens;
  s.height = p.height;
  s.width = p.width;

  Mat3 k, kinv;
  load_mat3(p.cand_k + (size_t)cand * 9, k);
  load_mat3(p.cand_kinv + (size_t)cand * 9, kinv);

  // ---- pass 1: the fit's moments ----
  float shift[3];
  later_point(s, kinv, alignment_pixel((long)p.indices[p.points / 2], n), shift);
  float acc[kMomentCount];
#pragma unroll
  for (int i = 0; i < kMomentCount; ++i) acc[i] = 0.f;
  for (long j = threadIdx.x; j < p.points; j += kSweepThreads) {
    const int idx = alignment_pixel((long)p.indices[j], n);
    const Corr c = corr_load_with<false>(s, kinv, kinv, pixel_ref(idx, p.height, p.width), [&](int tr, int tc, float& ut, float& vt) {
      ut = pixel_center(tc, s.width);
      vt = pixel_center(tr, s.height);
      return s.depth_e[tr * s.width + tc];
    });
    moments_add(c, shift, acc);
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kMomentCount; ++i) {
    const float tot = wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = (double)tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double st[kStatStride];
#pragma unroll
    for (int i = 0; i < kMomentCount; ++i) {
      double tot = 0.0;
      for (int v = 0; v < kSweepWaves; ++v) tot += red[v][i];
      st[i] = tot;
    }
    moments_finish(st, shift);
    pose_solve_one(st, pose44, nullptr, aux);
  }
  __syncthreads();
  const size_t out = (size_t)bp * p.candidates + cand;
  if (p.poses != nullptr && threadIdx.x < 16) p.poses[out * 16 + threadIdx.x] = pose44[threadIdx.x];
  Pose t;
  load_pose44(pose44, t);

  // ---- pass 2: the flow error under that pose ----
  double sum = 0.0;
  float* pe = p.point_error ? p.point_error + out * (size_t)p.points : nullptr;
  for (long j = threadIdx.x; j < p.points; j += kSweepThreads) {
    const int idx = alignment_pixel((long)p.indices[j], n);
    const PixelRef px = pixel_ref(idx, p.height, p.width);
    float w = s.weights[idx];
    if (p.weight_sens != 0.f) w = fm_sigmoid<false>(p.weight_sens * w);
    SoftminTerm o;
    const float e = softmin_term(k, kinv, t, px.u, px.v, s.depth_l[idx], s.bwd_flow[2 * (size_t)idx], s.bwd_flow[2 * (size_t)idx + 1], w, o);
    if (pe) pe[j] = e;
    sum += (double)e;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wave][0] = sum;  // (thread 0 read the moments out of `red` before the barrier that published the pose)
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int v = 0; v < kSweepWaves; ++v) tot += red[v][0];
    p.error[out] = tot;  // this workgroup's own element: a plain store
  }
}

// One wave per (batch entry, pair): soft = softmin((error − min error)·10) in fp32 like the reference's F.softmin, K = Σ soft·K_candidate,
// focal = Σ soft·candidate (intrinsics_softmin.py:123-141 and the value it appends to its window).
__global__ void __launch_bounds__(kWave) focal_sweep_curve_kernel(const double* __restrict__ error, const float* __restrict__ cand_k,
                                                                  const float* __restrict__ focal_lengths, int candidates, float* __restrict__ soft,
                                                                  float* __restrict__ focal, float* __restrict__ intrinsics) {
  const int bp = blockIdx.x, lane = threadIdx.x;
  const double* e = error + (size_t)bp * candidates;
  float lo = 3.0e38f;
  for (int n = lane; n < candidates; n += kWave) lo = fminf(lo, (float)e[n]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) lo = fminf(lo, __shfl_xor(lo, off, kWave));
  float total = 0.f;
  for (int n = lane; n < candidates; n += kWave) total += expf(-(((float)e[n] - lo) * 10.f));
  total = wave_sum(total);
  float m[9], fl = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = 0.f;
  for (int n = lane; n < candidates; n += kWave) {
    const float sn = expf(-(((float)e[n] - lo) * 10.f)) / total;
    soft[(size_t)bp * candidates + n] = sn;
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] += cand_k[(size_t)n * 9 + i] * sn;
    fl += focal_lengths[n] * sn;
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = wave_sum(m[i]);
  fl = wave_sum(fl);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) intrinsics[(size_t)bp * 9 + i] = m[i];
    focal[bp] = fl;
  }
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_focal_sweep(const float* depth, const float* weights, float weight_sensitivity, const float* bwd_flow, const int64_t* indices, long points,
                   const float* focal_lengths, const float* candidate_k, const float* candidate_kinv, int batch, int frames, int height, int width,
                   int first_pair, int count, int candidates, double* error, float* soft, float* focal, float* intrinsics, float* poses,
                   float* point_error, void* stream) {
  FM_CHECK_ARG(focal_sweep_args_ok(depth, weights, bwd_flow, indices, points, focal_lengths, candidate_k, candidate_kinv, batch, frames, height, width,
                                   first_pair, count, candidates, error, soft, focal, intrinsics));
  SweepParams p{depth, weights, bwd_flow, indices, candidate_k, candidate_kinv, error, poses, point_error};
  p.points = points;
  p.frames = frames, p.height = height, p.width = width, p.first_pair = first_pair, p.count = count, p.candidates = candidates;
  p.weight_sens = weight_sensitivity;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(focal_sweep_kernel, dim3((unsigned)candidates, (unsigned)(batch * count)), dim3(kSweepThreads), 0, st, p);
  hipLaunchKernelGGL(focal_sweep_curve_kernel, dim3((unsigned)(batch * count)), dim3(kWave), 0, st, error, candidate_k, focal_lengths, candidates, soft,
                     focal, intrinsics);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
