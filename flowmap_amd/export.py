"""What follows the optimisation — SURVEY.md §8f rank 4.

* ``world_point_cloud``: the point cloud ``export_to_colmap`` builds frame by frame
  (flowmap/export/colmap.py:86-101: unproject, homogenise, camera-to-world, colours to
  point-major), as ONE launch (fm_world_points) instead of F × (unproject + einsum + 2 copies).
* ``voxel_point_cloud``: the same points merged per cell of a world-space grid — one averaged point and colour per occupied voxel, a
  count and the lowest contributing pixel —, in ONE pass over depth (fm_voxel_cloud) with no point cloud formed; bit-reproducible.
* ``tsdf_volume``: the depth maps fused into a truncated-signed-distance grid (fm_tsdf_volume: one thread per voxel walks the frames, no
  atomics) -> ``TsdfVolume``, whose ``surface_points`` are the zero crossings with normals and whose ``mesh`` is the surface-nets
  triangle mesh (``TsdfMesh``); ``grid_around`` sizes the grid from a cloud.
* ``write_ply``: the vertex layout of colmap.py:31-53 (x y z nx ny nz red green blue, binary
  little-endian — what 3D Gaussian Splatting reads), written with numpy alone; with ``faces`` a triangle face element follows.
* ``compute_ate``: flowmap/misc/ate.py:7-25 (scipy Procrustes alignment, RMS over all
  coordinates) — tiny, stays on the host.
The COLMAP camera/image records (colmap.py:114-, third_party/colmap) are file IO and stay with
the reference.
"""

from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _ops
from ._base import parse_window
from ._lib import call, check_device, ptr, stream_for
from .types import TsdfVolume, VoxelCloud

VOXEL_MAX_CAPACITY = 1 << 28  # (fm_residual_args.h: kVoxelMaxCapacity)


def _check_cloud_arguments(depths, intrinsics, extrinsics, colors, keep) -> Tuple[int, int, int]:
    """The checks world_point_cloud and voxel_point_cloud share -> (frames, height, width)."""
    check_device(depths, intrinsics, extrinsics, *(() if colors is None else (colors,)))
    if depths.dim() != 3:
        raise RuntimeError("flowmap_amd: depths must be (frame, height, width)")
    f, h, w = depths.shape
    if tuple(intrinsics.shape) != (f, 3, 3) or tuple(extrinsics.shape) != (f, 4, 4):
        raise RuntimeError("flowmap_amd: intrinsics / extrinsics do not match the depths")
    if colors is not None and tuple(colors.shape) != (f, 3, h, w):
        raise RuntimeError("flowmap_amd: colors must be (frame, 3, height, width)")
    if keep is not None:
        if not torch.is_tensor(keep) or keep.dtype != torch.bool:
            raise RuntimeError(f"flowmap_amd: keep must be a bool tensor (got {getattr(keep, 'dtype', type(keep).__name__)})")
        if tuple(keep.shape) != (f, h, w):
            raise RuntimeError(f"flowmap_amd: keep of shape {tuple(keep.shape)} does not match the depths {(f, h, w)}")
        if keep.device != depths.device:
            raise RuntimeError(f"flowmap_amd: keep is on {keep.device}, the depths on {depths.device}")
    return f, h, w


def _check_stack_fits(what: str, f: int, h: int, w: int) -> None:
    """The stack limits of voxel_point_cloud and tsdf_volume (fm_residual_args.h: depth_stack_ok)."""
    if f > 65535 or h * w >= 1 << 30 or f * h * w >= 1 << 31:
        raise ValueError(f"flowmap_amd: {what}: frames x height x width = {f} x {h} x {w} does not fit (at most 65535 frames, int32 pixel indices)")


def world_point_cloud(depths: Tensor, intrinsics: Tensor, extrinsics: Tensor, colors: Optional[Tensor] = None,
                      keep: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """depths (F,H,W), intrinsics (F,3,3), extrinsics (F,4,4) camera-to-world, colors
    (F,3,H,W) -> world points (F·H·W,3) and colours (F·H·W,3), frames concatenated in order
    (colmap.py:86-101 with ``exports.*[0]``).  ``keep``: a bool (F,H,W) mask on the depths' device — the points and colours
    returned are the kept ones, in the same order (e.g. ``depth_consistency(...).support[0] >= 2``: the points that at least two
    other frames confirm); None: every point."""
    f, h, w = _check_cloud_arguments(depths, intrinsics, extrinsics, colors, keep)
    with torch.no_grad():
        depths, extrinsics = _ops._f32c(depths, "depths"), _ops._f32c(extrinsics, "extrinsics")
        kinv = _ops.intrinsics_inverse(_ops._f32c(intrinsics, "intrinsics"))
        colors = None if colors is None else _ops._f32c(colors, "colors")
        xyz = torch.empty((f * h * w, 3), dtype=torch.float32, device=depths.device)
        rgb = None if colors is None else torch.empty_like(xyz)
        with _ops._guard(depths.device):
            call("fm_world_points", ptr(depths), ptr(kinv), ptr(extrinsics), ptr(colors), f, h, w, ptr(xyz), ptr(rgb), stream_for(depths))
        if keep is not None:
            kept = keep.reshape(-1)
            xyz, rgb = xyz[kept], None if rgb is None else rgb[kept]
    return xyz, rgb


VOXEL_DEFAULT_DIVISOR = 16  # default capacity: one voxel per 16 candidate pixels (at least VOXEL_DEFAULT_FLOOR, at most the candidates)
VOXEL_DEFAULT_FLOOR = 4096


def voxel_default_capacity(candidates: int) -> int:
    """The ``capacity`` voxel_point_cloud takes when none is given: the candidate pixels, capped at max(candidates // 16, 4096).  The
    table has fewer than 4·capacity slots of 72 bytes, so beyond 65 536 candidates the workspace stays below 18 bytes per candidate
    pixel: 4.5 times the depth tensor."""
    return max(1, min(candidates, max(candidates // VOXEL_DEFAULT_DIVISOR, VOXEL_DEFAULT_FLOOR)))


def voxel_point_cloud(depths: Tensor, intrinsics: Tensor, extrinsics: Tensor, colors: Optional[Tensor], voxel_size: float, *,
                      keep: Optional[Tensor] = None, min_count: int = 1, capacity: Optional[int] = None, details: bool = False) -> VoxelCloud:
    """The points of ``world_point_cloud`` (same arguments, same checks) merged per cell of a world-space grid of edge ``voxel_size``:
    one centroid, mean colour, point count and lowest linear index ``frame·H·W + pixel`` per occupied voxel, rows in ascending lowest
    index -> VoxelCloud.  One pass over depth (fm_voxel_cloud: a hash table of integer accumulators; no point cloud is formed), so the
    result is a function of the SET of points: bit-reproducible.

    ``keep``: a bool (F,H,W) mask — only these pixels take part (``depth_consistency(...).support[0] >= 2``).  ``min_count``: a voxel
    with fewer points is left out (it is not an error and not counted in ``dropped``).  ``capacity``: the most voxels the call can
    hold — the table and the outputs are sized by it; None: ``voxel_default_capacity`` of the candidate pixels (F·H·W, or ``keep``'s
    count).  A cloud that does not fit raises and names ``capacity``.  ``details``: also ``voxel_of`` (F,H,W), the row of each pixel.
    A point is dropped as ``masked`` (keep), ``invalid`` (depth not finite or <= 0, or a non-finite world coordinate) or
    ``out_of_range`` (a cell outside [−2²⁰, 2²⁰) — a larger ``voxel_size`` brings it in)."""
    f, h, w = _check_cloud_arguments(depths, intrinsics, extrinsics, colors, keep)
    if isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float)) or not (0.0 < float(voxel_size) < float("inf")):
        raise ValueError(f"flowmap_amd: voxel_point_cloud: voxel_size must be a finite number > 0 (got {voxel_size!r})")
    with np.errstate(over="ignore"):
        inverse = np.float32(1.0 / float(voxel_size))
    if not (2.0**-126 <= float(inverse) < float("inf")):
        raise ValueError(f"flowmap_amd: voxel_point_cloud: voxel_size = {voxel_size!r} has no finite, normal float32 reciprocal")
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
        raise ValueError(f"flowmap_amd: voxel_point_cloud: min_count must be an integer >= 1 (got {min_count!r})")
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= VOXEL_MAX_CAPACITY):
        raise ValueError(f"flowmap_amd: voxel_point_cloud: capacity must be an integer in [1, 2^28] (got {capacity!r})")
    if not isinstance(details, bool):
        raise ValueError(f"flowmap_amd: voxel_point_cloud: details must be a bool (got {details!r})")
    _check_stack_fits("voxel_point_cloud", f, h, w)
    with torch.no_grad():
        if capacity is None:  # (counting a mask's candidates waits for the device once more: pass capacity to avoid it)
            capacity = min(voxel_default_capacity(f * h * w if keep is None else int(keep.sum())), VOXEL_MAX_CAPACITY)
        kinv = _ops.intrinsics_inverse_peek(_ops._f32c(intrinsics.detach(), "intrinsics"))
        xyz, rgb, count, first, slot, pixel_slot, counters = _ops.voxel_cloud(depths, kinv, extrinsics, colors, keep, float(voxel_size), min_count, capacity, details)
        rows, overflow, masked, invalid, out_of_range = (int(v) for v in counters[:5].tolist())  # (the one synchronisation: this is an export step)
        if overflow > 0 or rows > capacity:
            raise RuntimeError(f"flowmap_amd: voxel_point_cloud: the cloud does not fit capacity = {capacity}: {rows} voxels, {overflow} points found no "
                               f"slot in the table; pass a larger capacity (at most the {f * h * w} pixels) or a larger voxel_size")
        first, order = torch.sort(first[:rows])
        xyz, count, slot = xyz[:rows][order], count[:rows][order], slot[:rows][order]
        rgb = None if colors is None else rgb[:rows][order]
        voxel_of = None
        if details:
            slots, table_bytes = ctypes.c_long(0), ctypes.c_long(0)
            call("fm_voxel_cloud_workspace", capacity, ctypes.byref(slots), ctypes.byref(table_bytes))  # (the table's size, stated by the library)
            row_of_slot = torch.full((slots.value + 1,), -1, dtype=torch.int32, device=depths.device)  # (the last entry serves pixel_slot == −1)
            row_of_slot[slot.long()] = torch.arange(rows, dtype=torch.int32, device=depths.device)
            voxel_of = row_of_slot[pixel_slot.long()]
    return VoxelCloud(xyz, rgb, count, first, {"masked": masked, "invalid": invalid, "out_of_range": out_of_range}, voxel_of, float(voxel_size))


TSDF_MAX_VOXELS = 1 << 31  # (fm_residual_args.h: kTsdfMaxVoxels)


def _f32_number(value, what: str, name: str, *, positive: bool = False, minimum: Optional[float] = None) -> float:
    """A Python number as the float32 the kernels take -> that float32's value as a float; a bool, a non-number, a non-finite value (after
    rounding to float32 too) or one out of range raises ValueError naming the argument."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"flowmap_amd: {what}: {name} must be a number (got {value!r})")
    with np.errstate(over="ignore"):
        rounded = float(np.float32(value))
    if not np.isfinite(rounded) or (positive and not rounded > 0.0) or (minimum is not None and not rounded >= minimum):
        bound = "> 0" if positive else (f">= {minimum:g}" if minimum is not None else "finite")
        raise ValueError(f"flowmap_amd: {what}: {name} must be a finite float32 {bound} (got {value!r})")
    return rounded


def grid_around(points, voxel_size: float, margin: float = 0.0) -> Tuple[Tuple[float, float, float], Tuple[int, int, int]]:
    """The grid of edge ``voxel_size`` that encloses a VoxelCloud's centroids or an (N, 3) tensor of points with ``margin`` world units to
    spare on every side -> (origin, dims) for ``tsdf_volume``.  Non-finite points are ignored; the minimum and maximum are taken with
    torch (plumbing over a small cloud) and read back once."""
    what = "grid_around"
    voxel_size = _f32_number(voxel_size, what, "voxel_size", positive=True)
    margin = _f32_number(margin, what, "margin", minimum=0.0)
    xyz = points.xyz if isinstance(points, VoxelCloud) else points
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3 or not xyz.is_floating_point():
        raise ValueError(f"flowmap_amd: {what}: points must be a VoxelCloud or a floating (N, 3) tensor (got {getattr(xyz, 'shape', type(xyz).__name__)})")
    with torch.no_grad():
        xyz = xyz.detach().double()
        xyz = xyz[torch.isfinite(xyz).all(dim=1)]
        if xyz.shape[0] == 0:
            raise ValueError(f"flowmap_amd: {what}: points holds no finite point")
        low, high = xyz.min(dim=0).values.cpu() - margin, xyz.max(dim=0).values.cpu() + margin
    origin = tuple(float(np.float32(v)) for v in low.tolist())
    dims = tuple(max(1, int(np.ceil((hi - lo) / voxel_size)) + 1) for lo, hi in zip(origin, high.tolist()))  # (+1: the rounding of the origin and of the last cell)
    if dims[0] * dims[1] * dims[2] >= TSDF_MAX_VOXELS:
        raise ValueError(f"flowmap_amd: {what}: {dims[0]} x {dims[1]} x {dims[2]} voxels at voxel_size = {voxel_size!r} do not fit 2^31: pass a larger voxel_size")
    return origin, dims


def tsdf_volume(depths: Tensor, intrinsics: Tensor, extrinsics: Tensor, colors: Optional[Tensor], voxel_size: float, *, origin, dims,
                truncation: Optional[float] = None, near: float = 0.0, keep: Optional[Tensor] = None, frames=None) -> TsdfVolume:
    """The depth maps (arguments and checks of ``world_point_cloud``) fused into a truncated-signed-distance grid -> TsdfVolume.

    ``origin``: the world position of the low corner of voxel (0, 0, 0), 3 numbers; ``dims`` = (nx, ny, nz), each >= 1, fewer than 2^31
    voxels in all (``grid_around`` gives both for a cloud).  Voxel (i, j, k) has its centre at ``origin + (index + 0.5)·voxel_size``.  For
    each frame of the window ``frames`` (None: all; a slice with step 1; (first, count)), in ascending order, the centre is moved into the
    camera (p = E_f⁻¹·c), skipped unless ``p.z > near``, projected, skipped unless it lands inside the frame, and compared with the depth d
    of the pixel it lands in (skipped where d is not finite, d <= 0 or ``keep`` is False): sdf = d − p.z; a voxel more than ``truncation``
    (default 4·voxel_size) behind the surface is hidden and skipped; otherwise min(sdf/truncation, 1) enters the voxel's mean and, where
    sdf <= truncation, the pixel's colour its mean colour.  One HIP pass, one thread per voxel, sums in registers in frame order: no
    atomics, and the result is bit-reproducible.  Never differentiable; reads its arguments and nothing else."""
    what = "tsdf_volume"
    f, h, w = _check_cloud_arguments(depths, intrinsics, extrinsics, colors, keep)
    voxel_size = _f32_number(voxel_size, what, "voxel_size", positive=True)
    truncation = _f32_number(4.0 * voxel_size if truncation is None else truncation, what, "truncation", positive=True)
    near = _f32_number(near, what, "near", minimum=0.0)
    if isinstance(origin, (str, bytes)) or not hasattr(origin, "__len__") or len(origin) != 3:
        raise ValueError(f"flowmap_amd: {what}: origin must be 3 numbers (got {origin!r})")
    origin = tuple(_f32_number(v.item() if torch.is_tensor(v) else v, what, "origin") for v in origin)
    if isinstance(dims, (str, bytes)) or not hasattr(dims, "__len__") or len(dims) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in dims):
        raise ValueError(f"flowmap_amd: {what}: dims must be 3 integers (nx, ny, nz) (got {dims!r})")
    dims = tuple(int(v) for v in dims)
    if min(dims) < 1 or dims[0] * dims[1] * dims[2] >= TSDF_MAX_VOXELS:
        raise ValueError(f"flowmap_amd: {what}: dims must each be >= 1 with nx * ny * nz < 2^31 (got {dims!r})")
    _check_stack_fits(what, f, h, w)
    first, count = parse_window(frames, f, what, "frames")
    with torch.no_grad():
        w2c, tsdf, weight, color, color_weight = _ops.tsdf_volume(depths, _ops._f32c(intrinsics.detach(), "intrinsics"), extrinsics, colors, keep, first, count,
                                                                  origin, dims, voxel_size, truncation, near)
    return TsdfVolume(tsdf, weight, color, color_weight, w2c, origin, voxel_size, truncation, near, (first, count))


_PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                       ("red", "u1"), ("green", "u1"), ("blue", "u1")])


_PLY_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", 3)])  # `property list uchar int vertex_indices`: a count of 3 and three indices


def write_ply(path: Path, xyz: np.ndarray, rgb: np.ndarray, normals: Optional[np.ndarray] = None, faces: Optional[np.ndarray] = None) -> None:
    """colmap.py:31-53: zero normals, colours scaled by 255 and truncated to uint8.  ``normals`` (N, 3): written as nx ny nz instead of the
    zeros (TsdfVolume.write_ply); ``faces`` (M, 3) integer rows of ``xyz``: a face element of triangles after the vertices
    (TsdfMesh.write_ply); without either the file is what it always was."""
    xyz = np.asarray(xyz, dtype=np.float32)
    vertices = np.zeros(xyz.shape[0], dtype=_PLY_DTYPE)
    vertices["x"], vertices["y"], vertices["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float32)
        if normals.shape != xyz.shape:
            raise ValueError(f"flowmap_amd: write_ply: normals of shape {normals.shape} do not match the points {xyz.shape}")
        vertices["nx"], vertices["ny"], vertices["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    scaled = (np.asarray(rgb) * 255).astype(np.float32)
    vertices["red"], vertices["green"], vertices["blue"] = scaled[:, 0], scaled[:, 1], scaled[:, 2]
    kinds = {"<f4": "float", "|u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {xyz.shape[0]}"]
    header += [f"property {kinds[_PLY_DTYPE[name].str]} {name}" for name in _PLY_DTYPE.names]
    records = None
    if faces is not None:
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or not np.issubdtype(faces.dtype, np.integer):
            raise ValueError(f"flowmap_amd: write_ply: faces must be (M, 3) integers (got {faces.dtype} of shape {faces.shape})")
        if faces.size and not (0 <= int(faces.min()) and int(faces.max()) < xyz.shape[0]):
            raise ValueError(f"flowmap_amd: write_ply: faces index rows {int(faces.min())} to {int(faces.max())} of {xyz.shape[0]} points")
        records = np.zeros(faces.shape[0], dtype=_PLY_FACE_DTYPE)
        records["n"], records["v"] = 3, faces
        header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices"]
    header.append("end_header")
    with open(path, "wb") as handle:
        handle.write(("\n".join(header) + "\n").encode("ascii"))
        handle.write(vertices.tobytes())
        if records is not None:
            handle.write(records.tobytes())


def read_ply(path: Path) -> Tuple[np.ndarray, np.ndarray]:
    """Inverse of write_ply for the layout above (colmap.py:18-28)."""
    with open(path, "rb") as handle:
        count = None
        while True:
            line = handle.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                count = int(line.split()[-1])
            if line == "end_header":
                break
        vertices = np.frombuffer(handle.read(), dtype=_PLY_DTYPE, count=count)
    xyz = np.stack([vertices["x"], vertices["y"], vertices["z"]], axis=1)
    rgb = np.stack([vertices["red"], vertices["green"], vertices["blue"]], axis=1) / 255.0
    return xyz, rgb


def compute_ate(gt: Tensor, predicted: Tensor):
    """flowmap/misc/ate.py:7-25 -> (ate, aligned_gt, aligned_predicted)."""
    from scipy import spatial

    a, b, _ = spatial.procrustes(gt.detach().cpu().numpy(), predicted.detach().cpu().numpy())
    a = torch.tensor(a, dtype=torch.float32, device=gt.device)
    b = torch.tensor(b, dtype=torch.float32, device=predicted.device)
    return ((a - b) ** 2).mean() ** 0.5, a, b
