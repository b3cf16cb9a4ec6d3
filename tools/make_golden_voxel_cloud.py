"""Generate tests/golden/fn_voxel_cloud.npz: the world points of export_to_colmap as the REFERENCE's own functions compose them —
sample_image_grid, unproject, homogenize_points and the einsum with the camera-to-world matrix (flowmap/export/colmap.py:86-101,
flowmap/model/projection.py:93-113, :76-90, :11-15) — on the seeded inputs of tests/voxel_cloud_cases.py (GOLDEN_CASES), in fp32 (its
native precision) and in fp64 (same code, inputs up-cast, its hard-coded fp32 constants patched as oracle/make_golden.py does).  The
reference has no voxel grid: the voxelisation on top of its points is the cases module's (``restate`` on the fp32 points, ``voxelise64`` on
the fp64 ones).  Data only.  Needs the reference importable (FLOWMAP_REFERENCE, as oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_voxel_cloud.py

Keys ``<case>_<array>``: depth, k, ext, colors (the inputs), points (F·h·w, 3) float32 and f64_points float64, and the voxelisation of
each: voxel_of (F·h·w,), xyz (M, 3), count, first with their ``f64_`` twins.  Every case is checked here on the CPU: the two
voxelisations may group at most 0.5 % of the points differently (the tests' condition, voxel_cloud_cases.GOLDEN_CAP).
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402
from einops import einsum, rearrange  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (puts the reference and its stubs on sys.path; generates nothing on import)

from flowmap.model import projection as rp  # noqa: E402

from voxel_cloud_cases import GOLDEN_CAP, GOLDEN_CASES, case_inputs, restate, same_membership, spec_of, voxelise64  # noqa: E402


def reference_points(x, dtype):
    depth, k, ext = (x[key].to(dtype) for key in ("depth", "k", "ext"))
    xy = rp.sample_image_grid(tuple(depth.shape[1:]), depth.device)[0].to(dtype)
    points = []
    for extrinsics, intrinsics, depths in zip(ext, k, depth):
        xyz = rp.homogenize_points(rp.unproject(xy, depths, intrinsics))
        xyz = einsum(extrinsics, xyz, "i j, ... j -> ... i")[..., :3]
        points.append(rearrange(xyz, "h w xyz -> (h w) xyz"))
    return torch.cat(points)


def main():
    arrays = {}
    for name in GOLDEN_CASES:
        x = case_inputs(name)
        voxel_size = spec_of(name)["voxel_size"]
        p32 = reference_points(x, torch.float32)
        with mg.fp64_reference():
            p64 = reference_points(x, torch.float64)
        assert p32.dtype == torch.float32 and p64.dtype == torch.float64
        colors = x["colors"].permute(0, 2, 3, 1).reshape(-1, 3)
        v32, v64 = restate(p32.numpy(), colors.numpy(), x["depth"].numpy(), None, voxel_size), voxelise64(p64.numpy(), voxel_size)
        differ = 1.0 - same_membership(v32["voxel_of"], v64["voxel_of"]).mean()
        assert differ <= GOLDEN_CAP, f"{name}: the reference's fp32 and fp64 voxelisations group {differ:.2e} of the points differently"
        print(f"  {name}: {len(p32)} points, {len(v64['count'])} voxels at {voxel_size}; fp32 and fp64 group {differ:.2e} of the points differently; "
              f"points differ by at most {float((p32.double() - p64).abs().max()):.2e}")
        arrays.update({f"{name}_{k}": v for k, v in x.items()})
        arrays[f"{name}_points"], arrays[f"{name}_f64_points"] = p32, p64
        for prefix, vox in (("", v32), ("f64_", v64)):
            for key in ("voxel_of", "xyz", "count", "first"):
                arrays[f"{name}_{prefix}{key}"] = vox[key]
    mg.save("fn_voxel_cloud", **arrays)


if __name__ == "__main__":
    main()
