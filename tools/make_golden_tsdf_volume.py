"""Generate tests/golden/fn_tsdf_volume.npz: where the voxel centres of export.tsdf_volume land in every frame, as the REFERENCE's own
functions compose it — homogenize_points, transform_world2cam (its own ``extrinsics.inverse()``) and project_camera_space
(flowmap/model/projection.py:11-15, :41-46, :49-58) — on the seeded inputs of tests/tsdf_volume_cases.py (GOLDEN_CASES), in fp32 (its native
precision) and in fp64 (same code, inputs up-cast, its hard-coded fp32 constants patched as oracle/make_golden.py does).  The reference has
no voxel grid: the centres are the cases module's (``centres``), and so is everything after the projection (``outcomes``, ``fuse``).  Data
only.  Needs the reference importable (FLOWMAP_REFERENCE, as oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_tsdf_volume.py

Keys ``<case>_<array>``: depth, k, ext, colors (the inputs), origin (3,), dims (3,), voxel_size, truncation (the grid), uv (V, F, 2) and pz
(V, F) float32 with their ``f64_`` twins, V = nx·ny·nz voxels with x fastest.  Every case is checked here on the CPU: the fp64 evaluation
leaves at most 1 % of the voxels undecided (the tests' condition) and the oracle's fp64 evaluation agrees with the reference's.
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (puts the reference and its stubs on sys.path; generates nothing on import)

from flowmap.model import projection as rp  # noqa: E402

from tsdf_volume_cases import GOLDEN_CASES, INPUT_KEYS, case_of, evaluate, outcomes  # noqa: E402

REFERENCE = (rp.homogenize_points, rp.transform_world2cam, rp.project_camera_space)


def main():
    arrays = {}
    for name in GOLDEN_CASES:
        x, call = case_of(name)
        ev32 = evaluate(x, call, torch.float32, fns=REFERENCE)
        with mg.fp64_reference():
            ev64 = evaluate(x, call, torch.float64, fns=REFERENCE)
        assert ev32["uv"].dtype == torch.float32 and ev64["pz"].dtype == torch.float64
        mine = evaluate(x, call, torch.float64)
        assert float((mine["pz"] - ev64["pz"]).abs().max()) < 1e-12 and float((mine["uv"] - ev64["uv"]).abs().max()) < 1e-9
        share = float(((~outcomes(ev64, x, call)["firm"]).sum(dim=1) > 0).double().mean())
        assert share <= 0.01, f"{name}: {share:.3%} of the voxels are undecided"
        print(f"  {name}: {ev64['pz'].shape[0]} voxels x {ev64['pz'].shape[1]} frames; {share:.3%} undecided; fp32 and fp64 differ by at most "
              f"{float((ev32['pz'].double() - ev64['pz']).abs().max()):.2e} in p.z")
        arrays.update({f"{name}_{key}": x[key] for key in INPUT_KEYS})
        arrays[f"{name}_origin"], arrays[f"{name}_dims"] = np.asarray(call["origin"], dtype=np.float32), np.asarray(call["dims"], dtype=np.int64)
        arrays[f"{name}_voxel_size"], arrays[f"{name}_truncation"] = np.float32(call["voxel_size"]), np.float32(call["truncation"])
        for prefix, ev in (("", ev32), ("f64_", ev64)):
            arrays[f"{name}_{prefix}uv"], arrays[f"{name}_{prefix}pz"] = ev["uv"], ev["pz"]
    mg.save("fn_tsdf_volume", **arrays)


if __name__ == "__main__":
    main()
