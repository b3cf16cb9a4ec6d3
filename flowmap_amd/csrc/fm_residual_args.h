// Argument checks and size formulas of the residual entry points (include/flowmap_hip.h: fm_flow_residuals, fm_track_residuals,
// fm_alignment_residuals, fm_focal_sweep, fm_depth_consistency, fm_render_views, fm_voxel_cloud, fm_tsdf_volume, fm_tsdf_surface_count / _emit, fm_tsdf_mesh_count / _emit and their size functions) and the fm_layout rules of the `_views` entry points, stated ONCE: the device build (fm_*.hip) and the serial host build of
// the same ABI (fm_*_host.h) both call these, so the two refuse the same calls and size the same workspaces.  Plain C++, no HIP.
// Device-only, and therefore not here: the 16-byte path's eligibility and the pointer alignment the kernels need (the host build reads
// element by element and never touches the workspace).
#pragma once

#include <stdint.h>

#include "../../include/flowmap_hip.h"

namespace fm {

constexpr int kFlowResTile = 2048;    // pixels per workgroup of flow_residuals_kernel
constexpr int kAlignResTile = 1024;   // elements per workgroup of alignment_residuals_kernel
constexpr int kTrackResChunk = 64;    // points per wave of track_residuals_kernel: one workspace slot per (fs, ft, chunk)
constexpr int kTrackResThreads = 256;
constexpr long kResMaxPixels = 1L << 30;  // pixels of a frame are indexed with 32 bits
constexpr long kResMaxRows = 65535;       // (batch entry, pair) rows of one call: a grid dimension

static inline bool res_frame_ok(int height, int width) { return height >= 1 && width >= 1 && (long)height * width < kResMaxPixels; }
static inline bool res_window_ok(int batch, int frames, int first_pair, int count) {
  return batch >= 1 && frames >= 2 && first_pair >= 0 && count >= 1 && (long)first_pair + count <= frames - 1 && (long)batch * count <= kResMaxRows;
}

// ---- fm_layout: the element strides of a frame window read in place ----
// Every `_views` launcher of the device build (fm_flow.hip, fm_procrustes.hip, fm_flow_residuals.hip) and the host build's reader (densify,
// fm_flow_bitmask_host.h) resolve a layout here.  What a launcher asks of the strides beyond this — divisible by 4 for a 16-byte path, frames
// apart only, or nothing — is its own and stays with it.
// layout_is_view: does any of the `n` entries at `layouts` describe a view?  NULL and {0, 0} both mean dense.
static inline bool layout_is_view(const fm_layout* layouts, int n = 1) {
  for (int i = 0; layouts && i < n; ++i)
    if (layouts[i].frame_stride != 0 || layouts[i].batch_stride != 0) return true;
  return false;
}

// Element strides of stack i: `per_frame` elements per frame, `frames_of` frames per batch entry when dense.
static inline void layout_strides(const fm_layout* layouts, int i, long per_frame, long frames_of, long& fs, long& bs) {
  const bool view = layouts && layout_is_view(layouts + i);
  fs = view ? layouts[i].frame_stride : per_frame;
  bs = view ? layouts[i].batch_stride : per_frame * frames_of;
}

// Frames do not overlap, and neither do batch entries (a batch-expanded stack, stride 0 over the batch, is the caller's to copy).
static inline bool layout_apart(long fs, long bs, long per_frame, long frames_of, int batch) {
  return fs >= per_frame && (batch == 1 || bs >= fs * (frames_of - 1) + per_frame);
}

// The five stacks of the flow loss — depth, flow_fwd, flow_bwd, mask_fwd, mask_bwd — for the fused pass and the residual maps alike;
// false: a stack's frames or batch entries would overlap.
static inline bool flow_strides(const fm_layout* layouts, int batch, int frames, long pixels, long fs[5], long bs[5]) {
  const long per_frame[5] = {pixels, 2 * pixels, 2 * pixels, pixels, pixels};
  const long frames_of[5] = {frames, frames - 1, frames - 1, frames - 1, frames - 1};
  for (int i = 0; i < 5; ++i) {
    layout_strides(layouts, i, per_frame[i], frames_of[i], fs[i], bs[i]);
    if (!layout_apart(fs[i], bs[i], per_frame[i], frames_of[i], batch)) return false;
  }
  return true;
}

// ---- flow ----
static inline long flow_residual_blocks(long pixels) { return (pixels + kFlowResTile - 1) / kFlowResTile; }
static inline bool flow_residual_blocks_args_ok(int height, int width, const int* blocks) { return blocks && res_frame_ok(height, width); }

static inline bool flow_residuals_args_ok(const float* depth, const float* k, const float* kinv, const float* t_fwd, const float* t_bwd,
                                          const float* flow_fwd, const float* flow_bwd, const float* mask_fwd, const float* mask_bwd, int batch, int frames,
                                          int height, int width, int mapping_kind, float aspect_x, float aspect_y, int first_pair, int count,
                                          const float* residual_fwd, const float* residual_bwd, const float* pred_fwd, const float* pred_bwd,
                                          const double* pair_sum, const double* pair_valid, const double* workspace) {
  if (!(depth && k && kinv && t_fwd && t_bwd && flow_fwd && flow_bwd && residual_fwd && residual_bwd)) return false;
  if ((pred_fwd == nullptr) != (pred_bwd == nullptr)) return false;
  const bool sums = pair_sum != nullptr;
  if ((pair_valid != nullptr) != sums || (workspace != nullptr) != sums || (sums && !(mask_fwd && mask_bwd))) return false;
  if (!res_frame_ok(height, width) || !res_window_ok(batch, frames, first_pair, count)) return false;
  return mapping_kind >= 0 && mapping_kind <= 2 && aspect_x > 0.f && aspect_y > 0.f;
}

// ---- tracking ----
// (constexpr: the kernels call these two as well)
constexpr long track_res_chunks(long p) { return (p + kTrackResChunk - 1) / kTrackResChunk; }
// doubles of workspace of one segment: [f][f][chunks][2] pair partials, then [f][p][2] per-source-frame track partials
constexpr long track_res_work(long f, long p) { return 2 * (f * f * track_res_chunks(p) + f * p); }
static inline bool track_residual_workspace_args_ok(int frames, int points, const long* doubles) { return doubles && frames >= 1 && points >= 1; }
static inline long track_res_point_blocks(int pmax) { return ((long)pmax + kTrackResThreads - 1) / kTrackResThreads; }
static inline long track_res_sum_blocks(int pmax, int fmax) {
  const long pair_blocks = ((long)fmax * fmax + kTrackResThreads - 1) / kTrackResThreads, point_blocks = track_res_point_blocks(pmax);
  return pair_blocks > point_blocks ? pair_blocks : point_blocks;
}

static inline bool track_residuals_args_ok(const float* depth, const float* kinv, const float* ext, const float* ext_inv, const float* k, int frames,
                                           const float* xy, const uint8_t* vis, const int32_t* seg, int first_segment, int count, int pmax, int fmax,
                                           int height, int width, int mapping_kind, float aspect_x, float aspect_y, const float* tgt, const float* residual,
                                           const uint8_t* visible, const double* pair_sum, const double* pair_count, const double* track_sum,
                                           const double* track_count, const double* workspace) {
  if (!(depth && kinv && ext && ext_inv && k && xy && vis && seg && tgt && residual && visible)) return false;
  const bool sums = pair_sum != nullptr;
  if ((pair_count != nullptr) != sums || (track_sum != nullptr) != sums || (track_count != nullptr) != sums || (workspace != nullptr) != sums) return false;
  if (!(frames >= 1 && first_segment >= 0 && count >= 1 && pmax >= 1 && fmax >= 1 && res_frame_ok(height, width))) return false;
  if (!(mapping_kind >= 0 && mapping_kind <= 2 && aspect_x > 0.f && aspect_y > 0.f)) return false;
  return (long)count * fmax < (1L << 31) - 1 && track_res_point_blocks(pmax) <= kResMaxRows && track_res_sum_blocks(pmax, fmax) <= kResMaxRows;
}

// ---- alignment ----
static inline long alignment_residual_tiles(long points) { return (points + kAlignResTile - 1) / kAlignResTile; }
static inline bool res_points_ok(long points) { return points >= 1 && points < kResMaxPixels; }
static inline bool alignment_residual_workspace_args_ok(long points, const long* doubles) { return doubles && res_points_ok(points); }

static inline bool alignment_residuals_args_ok(const float* depth, const float* kinv, const float* surfaces, const float* bwd_flow, const float* rel,
                                               const int64_t* indices, long points, int batch, int frames, int height, int width, int first_pair, int count,
                                               const float* residual, const double* pair_sum, const double* pair_weight, const double* workspace) {
  if (!(bwd_flow && rel && residual)) return false;
  if ((depth != nullptr) == (surfaces != nullptr) || (depth != nullptr && kinv == nullptr)) return false;
  const bool sums = pair_sum != nullptr;
  if ((pair_weight != nullptr) != sums || (workspace != nullptr) != sums) return false;
  if (!res_frame_ok(height, width) || !res_window_ok(batch, frames, first_pair, count)) return false;
  return res_points_ok(points) && (indices != nullptr || points == (long)height * width);
}

// ---- focal sweep ----
static inline bool focal_sweep_args_ok(const float* depth, const float* weights, const float* bwd_flow, const int64_t* indices, long points,
                                       const float* focal_lengths, const float* candidate_k, const float* candidate_kinv, int batch, int frames, int height,
                                       int width, int first_pair, int count, int candidates, const double* error, const float* soft, const float* focal,
                                       const float* intrinsics) {
  if (!(depth && weights && bwd_flow && indices && focal_lengths && candidate_k && candidate_kinv)) return false;
  if (!(error && soft && focal && intrinsics)) return false;
  if (!res_frame_ok(height, width) || !res_window_ok(batch, frames, first_pair, count)) return false;
  return res_points_ok(points) && candidates >= 1;
}

// ---- depth consistency ----
constexpr int kDepthConsTile = 1024;       // pixels per workgroup of depth_consistency_kernel
constexpr int kDepthConsMaxOffsets = 8;    // frame offsets of one call
static inline long depth_consistency_blocks(long pixels) { return (pixels + kDepthConsTile - 1) / kDepthConsTile; }
static inline bool depth_consistency_blocks_args_ok(int height, int width, const int* blocks) { return blocks && res_frame_ok(height, width); }

static inline bool depth_consistency_args_ok(const float* depth, const float* k, const float* kinv, const float* ext, const int32_t* offsets, int n_offsets,
                                             int batch, int frames, int height, int width, int first_frame, int count, float tolerance, const float* error,
                                             const uint8_t* code, const float* positions, const float* reprojected, const float* sampled,
                                             const uint8_t* support, const double* frame_sum, const double* frame_valid, const float* rel,
                                             const double* workspace) {
  if (!(depth && k && kinv && ext && offsets && error && code && rel)) return false;
  if ((positions != nullptr) != (reprojected != nullptr) || (positions != nullptr) != (sampled != nullptr)) return false;
  const bool sums = frame_sum != nullptr;
  if ((frame_valid != nullptr) != sums || (workspace != nullptr) != sums) return false;
  if (support && !(tolerance >= 0.f)) return false;
  if (!res_frame_ok(height, width)) return false;
  if (!(batch >= 1 && frames >= 2 && first_frame >= 0 && count >= 1 && (long)first_frame + count <= frames && (long)batch * count <= kResMaxRows)) return false;
  if (n_offsets < 1 || n_offsets > kDepthConsMaxOffsets) return false;
  for (int i = 0; i < n_offsets; ++i) {
    if (offsets[i] == 0 || offsets[i] <= -frames || offsets[i] >= frames) return false;
    for (int j = 0; j < i; ++j)
      if (offsets[j] == offsets[i]) return false;
  }
  return true;
}

// ---- rendered views ----
constexpr int kRenderTile = 1024;        // source pixels per workgroup of render_splat_kernel
constexpr int kRenderMaxRadius = 2;      // a splat covers (2r+1)² target pixels
constexpr long kRenderMaxSources = 1L << 31;  // `source` is int32: frames x height x width stays below this
static inline long render_blocks(long pixels) { return (pixels + kRenderTile - 1) / kRenderTile; }
// a (frames, height, width) stack of depth maps whose pixels an int32 can name (render_views' `source`) ...
static inline bool depth_sources_ok(int frames, int height, int width) {
  return frames >= 1 && res_frame_ok(height, width) && (long)frames * height * width < kRenderMaxSources;
}
// ... and whose frames are a grid dimension as well (voxel cloud, TSDF)
static inline bool depth_stack_ok(int frames, int height, int width) { return frames <= kResMaxRows && depth_sources_ok(frames, height, width); }
// colours in <=> colours out
static inline bool color_pair_ok(const void* colors_in, const void* colors_out) { return (colors_in != nullptr) == (colors_out != nullptr); }
// bytes of workspace: the (B,V,OH,OW) 64-bit z-buffer, then one 16-float pose row per (batch entry, pair)
static inline long render_views_key_bytes(long batch, long views, long out_pixels) { return 8 * batch * views * out_pixels; }
static inline long render_views_workspace_bytes(long batch, long views, long out_pixels, long n_pairs) {
  return render_views_key_bytes(batch, views, out_pixels) + 64 * batch * n_pairs;
}
static inline bool render_views_shape_ok(int batch, int views, int out_height, int out_width, int n_pairs) {
  if (!(batch >= 1 && views >= 1 && n_pairs >= 0 && res_frame_ok(out_height, out_width))) return false;
  if ((long)batch * n_pairs > kResMaxRows) return false;
  return (long)batch * views <= (1L << 37) / ((long)out_height * out_width);  // (one resolve thread per target pixel: a grid dimension)
}
static inline bool render_views_workspace_args_ok(int batch, int views, int out_height, int out_width, int n_pairs, const long* bytes) {
  return bytes && render_views_shape_ok(batch, views, out_height, out_width, n_pairs);
}

static inline bool render_views_args_ok(const float* depth, const float* kinv, const float* ext, const float* colors, const float* view_k,
                                        const float* view_ext, const int32_t* pairs, int n_pairs, int batch, int frames, int height, int width, int views,
                                        int out_height, int out_width, int radius, float near, float background, const float* color, const float* out_depth,
                                        const int32_t* source, const void* workspace) {
  if (!(depth && kinv && ext && view_k && view_ext && out_depth && source && workspace)) return false;
  if (!color_pair_ok(colors, color)) return false;
  if (!render_views_shape_ok(batch, views, out_height, out_width, n_pairs) || (n_pairs > 0 && !pairs)) return false;
  if (!depth_sources_ok(frames, height, width)) return false;
  if (radius < 0 || radius > kRenderMaxRadius) return false;
  return near >= 0.f && near < __builtin_inff() && background == background;
}

// ---- voxel point cloud ----
constexpr int kVoxelTile = 1024;              // pixels per workgroup of voxel_insert_kernel (the geometry of render_splat_kernel)
constexpr long kVoxelMaxCapacity = 1L << 28;  // rows of one call: the table has at most 2^30 slots, a slot index is an int32
constexpr int kVoxelCounters = 8;             // 8-byte words of `counters`: rows drawn, overflow, masked, invalid, out of range, 3 spare
// the table: the smallest power of two >= 2·capacity slots (load factor <= 1/2), a 64-byte record and an 8-byte key per slot
static inline long voxel_cloud_slots(long capacity) {
  long slots = 2;
  while (slots < 2 * capacity) slots *= 2;
  return slots;
}
static inline long voxel_cloud_workspace_bytes(long capacity) { return 72 * voxel_cloud_slots(capacity); }
static inline bool voxel_cloud_workspace_args_ok(long capacity, const long* slots, const long* bytes) {
  return slots && bytes && capacity >= 1 && capacity <= kVoxelMaxCapacity;
}
static inline bool voxel_cloud_args_ok(const float* depth, const float* kinv, const float* ext, const float* colors, const uint8_t* keep, int frames,
                                       int height, int width, double voxel_size, int min_count, long capacity, const float* xyz, const float* rgb,
                                       const int32_t* count, const int64_t* first, const int32_t* slot, const int32_t* pixel_slot,
                                       const unsigned long long* counters, const void* workspace) {
  (void)keep, (void)pixel_slot;  // (optional)
  if (!(depth && kinv && ext && xyz && count && first && slot && counters && workspace)) return false;
  if (!color_pair_ok(colors, rgb) || !depth_stack_ok(frames, height, width)) return false;
  const float inv = (float)(1.0 / voxel_size);  // (finite and normal, or the call is refused)
  if (!(voxel_size > 0.0 && voxel_size < (double)__builtin_inff() && inv >= 1.17549435e-38f && inv < __builtin_inff())) return false;
  if (min_count < 1 || capacity < 1 || capacity > kVoxelMaxCapacity) return false;
  // the records are 64-byte requests, the counters 8-byte words: both builds refuse a misaligned pointer
  return (reinterpret_cast<uintptr_t>(workspace) & 63) == 0 && (reinterpret_cast<uintptr_t>(counters) & 7) == 0;
}

// ---- TSDF volume ----
constexpr int kTsdfTile = 256;              // voxels per workgroup of tsdf_integrate_kernel, of the two surface kernels and of the three mesh kernels (x fastest)
constexpr long kTsdfMaxVoxels = 1L << 31;   // nx·ny·nz stays below this: a voxel index is an int32, an edge id (voxel·3 + axis) an int64
static inline bool tsdf_dims_ok(int nx, int ny, int nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && (long)nx * ny < kTsdfMaxVoxels && (long)nx * ny * nz < kTsdfMaxVoxels;
}
static inline long tsdf_blocks(long voxels) { return (voxels + kTsdfTile - 1) / kTsdfTile; }
static inline bool tsdf_surface_blocks_args_ok(int nx, int ny, int nz, const long* blocks) { return blocks && tsdf_dims_ok(nx, ny, nz); }
static inline bool tsdf_finite(float x) { return x > -__builtin_inff() && x < __builtin_inff(); }
static inline bool tsdf_grid_ok(float ox, float oy, float oz, float voxel_size) {
  return tsdf_finite(ox) && tsdf_finite(oy) && tsdf_finite(oz) && voxel_size > 0.f && voxel_size < __builtin_inff();
}

static inline bool tsdf_volume_args_ok(const float* depth, const float* k, const float* ext, const float* colors, const uint8_t* keep, int frames, int height,
                                       int width, int first_frame, int count, float ox, float oy, float oz, int nx, int ny, int nz, float voxel_size,
                                       float truncation, float near, const float* world_to_camera, const float* tsdf, const int32_t* weight,
                                       const float* color, const int32_t* color_weight) {
  (void)keep;  // (optional)
  if (!(depth && k && ext && world_to_camera && tsdf && weight)) return false;
  if (!color_pair_ok(colors, color) || !color_pair_ok(colors, color_weight) || !depth_stack_ok(frames, height, width)) return false;
  if (!(first_frame >= 0 && count >= 1 && (long)first_frame + count <= frames)) return false;
  if (!tsdf_dims_ok(nx, ny, nz) || !tsdf_grid_ok(ox, oy, oz, voxel_size)) return false;
  return truncation > 0.f && truncation < __builtin_inff() && near >= 0.f && near < __builtin_inff();
}

static inline bool tsdf_surface_count_args_ok(const float* tsdf, const int32_t* weight, int nx, int ny, int nz, int min_weight, const int64_t* block_counts) {
  return tsdf && weight && block_counts && tsdf_dims_ok(nx, ny, nz) && min_weight >= 1;
}

static inline bool tsdf_surface_emit_args_ok(const float* tsdf, const int32_t* weight, const float* color, const int32_t* color_weight, int nx, int ny, int nz,
                                             float ox, float oy, float oz, float voxel_size, int min_weight, const int64_t* block_offsets, long rows,
                                             const float* xyz, const float* normals, const float* rgb, const int64_t* edge) {
  if (!(tsdf && weight && block_offsets && xyz && normals && edge)) return false;
  if ((color != nullptr) != (color_weight != nullptr) || (color != nullptr) != (rgb != nullptr)) return false;
  return tsdf_dims_ok(nx, ny, nz) && tsdf_grid_ok(ox, oy, oz, voxel_size) && min_weight >= 1 && rows >= 1;
}

static inline bool tsdf_mesh_count_args_ok(const float* tsdf, const int32_t* weight, int nx, int ny, int nz, int min_weight, const int64_t* cell_counts,
                                           const int64_t* quad_counts) {
  return tsdf && weight && cell_counts && quad_counts && tsdf_dims_ok(nx, ny, nz) && min_weight >= 1;
}

// (a mesh has vertices; it may have no quad — one active cell at the rim — and then takes no quad_offsets, faces or edge)
static inline bool tsdf_mesh_emit_args_ok(const float* tsdf, const int32_t* weight, const float* color, const int32_t* color_weight, int nx, int ny, int nz,
                                          float ox, float oy, float oz, float voxel_size, int min_weight, const int64_t* cell_offsets,
                                          const int64_t* quad_offsets, long vertex_rows, long quad_rows, const float* xyz, const float* normals,
                                          const float* rgb, const int64_t* cell, const int32_t* cell_vertex, const int32_t* faces, const int64_t* edge) {
  if (!(tsdf && weight && cell_offsets && xyz && normals && cell && cell_vertex)) return false;
  if ((color != nullptr) != (color_weight != nullptr) || (color != nullptr) != (rgb != nullptr)) return false;
  if (vertex_rows < 1 || quad_rows < 0 || (quad_rows > 0 && !(quad_offsets && faces && edge))) return false;
  return tsdf_dims_ok(nx, ny, nz) && tsdf_grid_ok(ox, oy, oz, voxel_size) && min_weight >= 1;
}

}  // namespace fm
