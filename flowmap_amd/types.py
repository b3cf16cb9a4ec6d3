"""Plain containers mirroring the reference's hot-path input/output types.

  Flows        flowmap/flow/flow_predictor.py:16-21
  Tracks       flowmap/tracking/track_predictor.py:13-20
  Batch        flowmap/dataset/types.py:12-19      (only .videos shape/device is read)
  ModelOutput  flowmap/model/model.py:24-30
  BackboneOutput  flowmap/model/backbone/backbone.py:14-17
  FlowResiduals  what LossFlow.residuals returns (no counterpart in the reference: its loss keeps these maps to itself)
  TrackResiduals  what LossTracking.residuals returns, one per segment (likewise)
  AlignmentResiduals  what ExtrinsicsProcrustes.residuals returns (likewise: the fit keeps its objective's terms to itself)
  FocalSweep  what IntrinsicsSoftmin.residuals returns (likewise: the sweep keeps its error curve and per-candidate poses to itself)
  DepthConsistency  what projection.depth_consistency / Model.consistency return (likewise: the reference never compares its depth maps)
  RenderedViews  what projection.render_views / Model.render return (likewise: the reference never renders its reconstruction)
  VoxelCloud  what export.voxel_point_cloud / Model.point_cloud return (likewise: the reference exports every pixel as a point)
  TsdfVolume  what export.tsdf_volume / Model.tsdf return (likewise: the reference has no surface, only per-pixel points)
  TsdfMesh  what TsdfVolume.mesh returns (likewise)

The reference's own dataclasses are accepted everywhere these are (duck typing): the
drop-in never checks the class, only the attribute names.
"""

from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Any, Optional

import torch
from torch import Tensor


class _Movable:
    def to(self, device):
        kw = {}
        for f in fields(self):
            v = getattr(self, f.name)
            kw[f.name] = v.to(device) if hasattr(v, "to") else v
        return type(self)(**kw)


@dataclass
class Flows(_Movable):
    forward: Tensor  # (batch, pair, H, W, 2)
    backward: Tensor  # (batch, pair, H, W, 2)
    forward_mask: Tensor  # (batch, pair, H, W)
    backward_mask: Tensor  # (batch, pair, H, W)


@dataclass
class Tracks(_Movable):
    xy: Tensor  # (batch, frame, point, 2)
    visibility: Tensor  # (batch, frame, point) bool
    start_frame: int


@dataclass
class Batch(_Movable):
    videos: Tensor  # (batch, frame, 3, H, W)
    indices: Optional[Tensor] = None
    scenes: Optional[list] = None
    datasets: Optional[list] = None
    extrinsics: Optional[Tensor] = None
    intrinsics: Optional[Tensor] = None


@dataclass
class BackboneOutput:
    depths: Tensor  # (batch, frame, H, W)
    weights: Tensor  # (batch, frame-1, H, W)


@dataclass
class ModelOutput:
    depths: Tensor  # (batch, frame, H, W)
    surfaces: Any  # (batch, frame, H, W, 3) Tensor, or LazySurfaces
    intrinsics: Tensor  # (batch, frame, 3, 3)
    extrinsics: Tensor  # (batch, frame, 4, 4)
    backward_correspondence_weights: Tensor  # (batch, frame-1, H, W)


@dataclass
class FlowResiduals:
    """The per-pixel terms of LossFlow.compute_unweighted_loss (flowmap/loss/loss_flow.py:46-68) for the pairs
    [first_pair, first_pair + count) — LossFlow.residuals."""

    forward: Tensor  # (batch, count, H, W): mapping.forward(xy_flowed_forward − xy, flows.forward, (H, W)), before the mask
    backward: Tensor  # (batch, count, H, W)
    forward_flow: Optional[Tensor]  # (batch, count, H, W, 2): xy_flowed_forward − xy, the pose-induced flow; None unless asked for
    backward_flow: Optional[Tensor]
    pair_sum: Optional[Tensor]  # (batch, count, 2) float64: Σ residual·mask per pair, [..., 0] forward, [..., 1] backward; None unless asked for
    pair_valid: Optional[Tensor]  # (batch, count, 2) float64: Σ mask
    first_pair: int

    def pair_loss(self) -> Tensor:
        """pair_sum / (pair_valid or 1): each pair's and direction's own masked mean."""
        if self.pair_sum is None:
            raise RuntimeError("flowmap_amd: FlowResiduals.pair_loss needs the sums (LossFlow.residuals(..., sums=True))")
        from .loss.loss import or_one

        return self.pair_sum / or_one(self.pair_valid)


@dataclass
class TrackResiduals:
    """The per-(source frame, target frame, point) terms of LossTracking.compute_unweighted_loss (flowmap/loss/loss_tracking.py:44-61)
    for ONE track segment of f frames and P points — LossTracking.residuals."""

    residual: Tensor  # (1, f, f, P): mapping.forward(xy_target, segment.xy[:, None], (H, W)), BEFORE visibility; [0, fs, ft, p]
    visible: Tensor  # (1, f, f, P) bool: the visibility compute_track_flow returns (projection.py:291-296)
    xy_target: Optional[Tensor]  # (1, f, f, P, 2): the reprojected positions; None unless asked for
    pair_sum: Optional[Tensor]  # (f, f) float64: Σ_p residual where visible; None unless asked for (as the three below)
    pair_count: Optional[Tensor]  # (f, f) float64: Σ_p visible
    track_sum: Optional[Tensor]  # (P,) float64: Σ_{fs,ft} residual where visible
    track_count: Optional[Tensor]  # (P,) float64: Σ_{fs,ft} visible
    segment: int  # index into the track list
    start_frame: int

    def _ratio(self, total, count, what: str) -> Tensor:
        if total is None:
            raise RuntimeError(f"flowmap_amd: TrackResiduals.{what} needs the sums (LossTracking.residuals(..., sums=True))")
        from .loss.loss import or_one

        return total / or_one(count)

    def pair_loss(self) -> Tensor:
        """pair_sum / (pair_count or 1): each (source frame, target frame)'s own masked mean."""
        return self._ratio(self.pair_sum, self.pair_count, "pair_loss")

    def track_loss(self) -> Tensor:
        """track_sum / (track_count or 1): each track's own masked mean over all frame pairs."""
        return self._ratio(self.track_sum, self.track_count, "track_loss")


@dataclass
class AlignmentResiduals:
    """The terms of the objective the Procrustes fit minimises, Σ w‖T·p − q‖² (flowmap/model/procrustes.py:7-51) over the correspondences
    of align_surfaces (flowmap/model/projection.py:213-252), for the pairs [first_pair, first_pair + count) —
    ExtrinsicsProcrustes.residuals.  ``maps`` is (batch, count, H, W) over every pixel, or (batch, count, P) over P indices."""

    residual: Tensor  # maps: ‖T·[p; 1] − q‖², before the weight
    offset: Optional[Tensor]  # maps + (3,): T·[p; 1] − q in the earlier camera's space; None unless asked for
    weight: Optional[Tensor]  # maps: the weight the kernel used (the sigmoid it applied to lazy logits; 1 without weights); None unless asked for
    pair_sum: Optional[Tensor]  # (batch, count) float64: Σ weight·residual per pair; None unless asked for
    pair_weight: Optional[Tensor]  # (batch, count) float64: Σ weight
    first_pair: int

    def pair_loss(self) -> Tensor:
        """pair_sum / (pair_weight or 1): each pair's own weighted mean."""
        if self.pair_sum is None:
            raise RuntimeError("flowmap_amd: AlignmentResiduals.pair_loss needs the sums (ExtrinsicsProcrustes.residuals(..., sums=True))")
        from .loss.loss import or_one

        return self.pair_sum / or_one(self.pair_weight)


@dataclass
class FocalSweep:
    """The softmin focal sweep (flowmap/model/intrinsics/intrinsics_softmin.py:85-141) of the pairs [first_pair, first_pair + count), pair i
    being frames (i, i+1), over n focal-length candidates on P sampled pixels — IntrinsicsSoftmin.residuals.  The reference evaluates
    pair 0 only and keeps nothing but the blended K."""

    first_pair: int
    count: int
    focal_lengths: Tensor  # (n) float32: the candidates
    indices: Tensor  # (P) int64: the pixel indices used
    error: Tensor  # (batch, count, n) float64: Σ over the points of |w·Δflow_x| + |w·Δflow_y| (intrinsics_softmin.py:124-125), per pair
    soft: Tensor  # (batch, count, n) float32: softmin((error − min)·10)
    focal: Tensor  # (batch, count) float32: Σ candidates·soft — what the reference appends to its window
    intrinsics: Tensor  # (batch, count, 3, 3) float32: Σ soft·K_candidate — what forward returns per frame
    poses: Optional[Tensor]  # (batch, count, n, 4, 4) float32: the fitted relative pose per candidate, later -> earlier; None unless asked for
    point_error: Optional[Tensor]  # (batch, count, n, P) float32: the per-point term before the sum; None unless asked for


@dataclass
class DepthConsistency:
    """Do the depth maps agree with each other under the chained camera poses?  For the source frames [first_frame, first_frame + count),
    every offset d of ``offsets`` (target j = i + d) and every pixel: p = unproject(xy, depth_i, K_i), q = (E_j⁻¹·E_i)·[p; 1],
    uv = project_camera_space(q, K_j), ẑ = the bilinear, border-clamped sample of depth_j at uv (flowmap/model/projection.py:76-90, :154,
    :49-58, :235-241) — projection.depth_consistency.  ``maps`` is (batch, count, n_off, H, W)."""

    error: Tensor  # maps float32: (ẑ − q.z) / q.z where code == 0, else exactly 0; negative: frame j's surface is nearer than the point
    code: Tensor  # maps uint8: 1 no frame j, 2 not q.z > 0, 3 not 0 <= uv < 1 (projection.py:294-295), 0 otherwise — the first that applies
    positions: Optional[Tensor]  # maps + (2,): uv; None unless asked for (details), as the two below
    reprojected: Optional[Tensor]  # maps: q.z
    sampled: Optional[Tensor]  # maps: ẑ
    support: Optional[Tensor]  # (batch, count, H, W) uint8: the offsets with code == 0 and |error| <= tolerance; None without a tolerance
    frame_sum: Optional[Tensor]  # (batch, count, n_off) float64: Σ |error| over code == 0; None unless asked for (sums)
    frame_valid: Optional[Tensor]  # (batch, count, n_off) float64: the number of pixels with code == 0
    first_frame: int
    offsets: tuple

    def frame_error(self) -> Tensor:
        """frame_sum / (frame_valid or 1): the mean |error| of each (frame, offset) over the pixels that land in the other frame."""
        if self.frame_sum is None:
            raise RuntimeError("flowmap_amd: DepthConsistency.frame_error needs the sums (depth_consistency(..., sums=True))")
        from .loss.loss import or_one

        return self.frame_sum / or_one(self.frame_valid)


@dataclass
class RenderedViews:
    """The depth maps (and colours) of some source frames splatted into a list of cameras with a z-buffer — projection.render_views /
    Model.render.  Per target pixel of a view the nearest source pixel that lands in it: p = unproject(xy, depth_i, K_i),
    q = (E_v⁻¹·E_i)·[p; 1], uv = project_camera_space(q, K_v); the smallest q.z wins, among equal q.z the lower source index."""

    color: Optional[Tensor]  # (batch, V, 3, OH, OW) float32: colors[i, :, y, x] of the winner bit for bit, ``background`` in a hole; None without colors
    depth: Tensor  # (batch, V, OH, OW) float32: the winner's q.z, 0 in a hole
    source: Tensor  # (batch, V, OH, OW) int32: the winner's absolute index i·H·W + y·W + x, −1 in a hole
    source_shape: tuple  # (H, W) of the source frames
    first_frame: Optional[int] = None  # held-out mode: view v is frame first_frame + v
    offsets: Optional[tuple] = None  # held-out mode: view v was rendered from the frames first_frame + v + d that exist

    def source_frame(self) -> Tensor:
        """The source frame of every target pixel (source // (H·W)), −1 in a hole."""
        h, w = self.source_shape
        return torch.where(self.source < 0, self.source, torch.div(self.source, h * w, rounding_mode="floor"))

    def coverage(self) -> Tensor:
        """(batch, V) float64: the share of target pixels that are not holes."""
        return (self.source >= 0).to(torch.float64).mean(dim=(2, 3))

    def _error_sums(self, images: Tensor, power: int):
        if self.color is None:
            raise RuntimeError("flowmap_amd: RenderedViews: there is no colour to compare (render_views(..., colors=...))")
        if not torch.is_tensor(images) or tuple(images.shape) != tuple(self.color.shape):
            raise RuntimeError(f"flowmap_amd: RenderedViews: images of shape {tuple(getattr(images, 'shape', ()))}; expected {tuple(self.color.shape)}")
        covered = (self.source >= 0)[:, :, None]
        diff = (self.color.to(torch.float64) - images.to(torch.float64)).abs() ** power
        total = torch.where(covered, diff, torch.zeros_like(diff)).sum(dim=(2, 3, 4))
        return total, 3.0 * covered.to(torch.float64).sum(dim=(2, 3, 4))

    def abs_error(self, images: Tensor) -> Tensor:
        """(batch, V) float64: the mean |color − images| over the covered pixels only (NaN for a view without any)."""
        total, count = self._error_sums(images, 1)
        return total / count

    def psnr(self, images: Tensor) -> Tensor:
        """(batch, V) float64: −10·log10 of the mean squared error against ``images`` (batch, V, 3, OH, OW, values in [0, 1]) over the
        covered pixels only, summed in float64 (NaN for a view without any).  In held-out mode ``psnr(batch.videos[:, window])`` is the
        held-out score."""
        total, count = self._error_sums(images, 2)
        return -10.0 * torch.log10(total / count)


@dataclass
class VoxelCloud:
    """The world points of the depth maps merged per cell of a world-space grid — export.voxel_point_cloud / Model.point_cloud.  One
    row per occupied voxel, in ascending ``first``; every field is a function of the set of points that fell into the voxel."""

    xyz: Tensor  # (M, 3) float32: the centroid
    rgb: Optional[Tensor]  # (M, 3) float32: the mean colour (clamped to [0, 1]); None without colors
    count: Tensor  # (M,) int32: the points merged into the voxel
    first: Tensor  # (M,) int64: the lowest linear index frame·H·W + pixel among them
    dropped: dict  # Python ints: masked, invalid (depth not finite or <= 0, or a non-finite world coordinate), out_of_range
    voxel_of: Optional[Tensor] = None  # (F, H, W) int32, with details=True: the row each pixel went to; −1 if dropped or filtered by min_count
    voxel_size: Optional[float] = None

    def __len__(self) -> int:
        return int(self.xyz.shape[0])

    def write_ply(self, path) -> None:
        """export.write_ply of the centroids and mean colours (black without colours)."""
        from .export import write_ply

        xyz = self.xyz.detach().cpu().numpy()
        write_ply(path, xyz, (torch.zeros_like(self.xyz) if self.rgb is None else self.rgb).detach().cpu().numpy())


def _check_min_weight(what: str, min_weight) -> None:
    if isinstance(min_weight, bool) or not isinstance(min_weight, int) or not 1 <= min_weight < 1 << 31:
        raise ValueError(f"flowmap_amd: {what}: min_weight must be an integer >= 1 (got {min_weight!r})")


@dataclass
class TsdfMesh:
    """The surface of a TsdfVolume as a triangle mesh — TsdfVolume.mesh.  One vertex per active cell in ascending ``cell``, two triangles
    per quad in ascending ``edge``; rows 2q and 2q+1 of ``faces`` belong to quad q."""

    vertices: Tensor  # (V, 3) float32
    normals: Tensor  # (V, 3) float32: unit, out of the surface; zero where the summed normals have no length
    rgb: Optional[Tensor]  # (V, 3) float32; None without colours
    cell: Tensor  # (V,) int64: the linear index of the cell's low-corner voxel
    faces: Tensor  # (2Q, 3) int32: rows of ``vertices``
    edge: Tensor  # (Q,) int64: voxel_linear_index·3 + axis of the crossing edge each quad surrounds

    def write_ply(self, path) -> None:
        """export.write_ply of the vertices with their normals (black without colours) and the faces."""
        from .export import write_ply

        rgb = torch.zeros_like(self.vertices) if self.rgb is None else self.rgb
        write_ply(path, self.vertices.cpu().numpy(), rgb.cpu().numpy(), self.normals.cpu().numpy(), self.faces.cpu().numpy())


@dataclass
class TsdfVolume:
    """The depth maps fused into a truncated-signed-distance grid — export.tsdf_volume / Model.tsdf.  Voxel (i, j, k) is element
    [k, j, i] of every field; its centre is ``origin + (index + 0.5)·voxel_size`` per axis.  ``tsdf`` is the mean over the frames that see
    the voxel of min(sdf/truncation, 1) — positive in front of the surface, toward the cameras —, exactly 1 where ``weight`` is 0."""

    tsdf: Tensor  # (nz, ny, nx) float32
    weight: Tensor  # (nz, ny, nx) int32: the frames that contributed
    color: Optional[Tensor]  # (nz, ny, nx, 3) float32: the mean colour over the frames with sdf <= truncation; None without colors
    color_weight: Optional[Tensor]  # (nz, ny, nx) int32; None without colors
    world_to_camera: Tensor  # (F, 4, 4) float32: E_f⁻¹ as the pass used it, for every frame of the video
    origin: tuple  # 3 floats (as rounded to float32): the low corner of voxel (0, 0, 0)
    voxel_size: float
    truncation: float
    near: float
    frames: tuple  # (first, count): the window of frames that was fused

    @property
    def dims(self) -> tuple:
        """(nx, ny, nz)"""
        nz, ny, nx = self.tsdf.shape
        return int(nx), int(ny), int(nz)

    def surface_points(self, min_weight: int = 1):
        """The zero crossings of the volume as an oriented point set -> (xyz (M,3), normals (M,3), rgb (M,3) or None, edge (M,) int64), rows
        in ascending ``edge`` = voxel_linear_index·3 + axis: the edge from a voxel to its +x, +y or +z neighbour crosses when both ends have
        ``weight >= min_weight`` and exactly one tsdf is negative.  The point lies at s = t0/(t0 − t1) along the edge; the normal is the
        normalised lerp of the ends' gradients (out of the surface, toward the cameras; zero where the gradient vanishes); rgb the lerp of
        the ends' colours.  Two HIP passes, count and emit, around one cumulative sum: no atomics, no sort, no capacity; bit-reproducible."""
        from . import _ops

        _check_min_weight("surface_points", min_weight)
        with torch.no_grad():
            return _ops.tsdf_surface(self.tsdf, self.weight, self.color, self.color_weight, self.origin, self.voxel_size, min_weight)

    def mesh(self, min_weight: int = 1) -> "TsdfMesh":
        """The surface of the volume as a triangle mesh, by surface nets -> TsdfMesh.  A CELL has a voxel as its low corner and the seven
        voxels at +1 along the axes as its other corners; it is active when one of its 12 edges is a crossing of ``surface_points``
        (``min_weight`` as there).  Every active cell carries one vertex, in ascending cell id: the mean of its crossing edges' points, the
        normalised sum of their normals, the mean of their colours.  Every crossing edge whose four cells exist carries one quad, in
        ascending edge id, split into the triangles (q0, q1, q2) and (q0, q2, q3), which face out of the surface, toward the cameras, as
        the normals do.  A crossing on the rim of the grid has a surface point and no quad: the mesh is open there and at the rim of what
        was observed.

        Known property: where two sheets of the surface pass through one cell (a feature thinner than about two voxels) they share that
        cell's vertex, and the mesh is not manifold there (a torus with a tube radius of 2.4 voxels shows it, one of 2.6 does not).

        Three HIP passes — count, vertices, faces — around two cumulative sums: no atomics, no sort, no case table; every output element
        is written once, so the result is bit-reproducible.  One int32 per voxel of workspace; waits for the device once."""
        from . import _ops

        _check_min_weight("mesh", min_weight)
        with torch.no_grad():
            return TsdfMesh(*_ops.tsdf_mesh(self.tsdf, self.weight, self.color, self.color_weight, self.origin, self.voxel_size, min_weight))

    def write_ply(self, path, min_weight: int = 1) -> None:
        """export.write_ply of ``surface_points(min_weight)`` with their normals (black without colours)."""
        from .export import write_ply

        xyz, normals, rgb, _ = self.surface_points(min_weight)
        rgb = torch.zeros_like(xyz) if rgb is None else rgb
        write_ply(path, xyz.cpu().numpy(), rgb.cpu().numpy(), normals.cpu().numpy())
