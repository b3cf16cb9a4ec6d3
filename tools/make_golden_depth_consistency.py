"""Generate tests/golden/fn_depth_consistency.npz: the depth consistency across frame offsets (flowmap_amd.model.projection.depth_consistency)
as the REFERENCE's own functions compose it — sample_image_grid, unproject, homogenize_points, transform_rigid with
extrinsics_target.inverse() @ extrinsics_source (flowmap/model/projection.py:288), project_camera_space and F.grid_sample(bilinear, border,
align_corners=False) (projection.py:235-241) — on the seeded inputs of tests/depth_consistency_cases.py, in fp32 (its native precision) and
in fp64 (same code, inputs up-cast, its hard-coded fp32 constants patched as oracle/make_golden.py does).  Data only.  Needs the reference
importable (FLOWMAP_REFERENCE, as oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_depth_consistency.py

Keys ``<case>_<array>``: depth, k, ext (the inputs), offsets, and per field (error, code, positions, reprojected, sampled — ``odd`` keeps
error, code and sampled only, to stay below the size of the largest fixture) the fp32 evaluation and its ``f64_`` twin, shaped
(b, F, n_off, h, w[, 2]) over EVERY source frame.  Every case is checked here on the CPU: the two evaluations must agree on the code of
every element (the tests' condition on ``code`` then has room), and the fp32 fields must pass the tests' gate against the fp64 ones.
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (puts the reference and its stubs on sys.path; generates nothing on import)

from flowmap.model import projection as rp  # noqa: E402

from conftest import assert_close_or_reference_gap  # noqa: E402

from depth_consistency_cases import FIELDS, GOLDEN_CASES, GOLDEN_FIELDS, SPECS, case_inputs  # noqa: E402


def reference_terms(x, offsets, dtype):
    depth, k, ext = (x[n].to(dtype) for n in ("depth", "k", "ext"))
    b, f, h, w = depth.shape
    xy, _ = rp.sample_image_grid((h, w), depth.device)
    xy = xy.to(dtype)
    maps = (b, f, len(offsets), h, w)
    out = {"error": torch.zeros(maps, dtype=dtype), "code": torch.ones(maps, dtype=torch.uint8), "positions": torch.zeros((*maps, 2), dtype=dtype),
           "reprojected": torch.zeros(maps, dtype=dtype), "sampled": torch.zeros(maps, dtype=dtype)}
    for o, d in enumerate(offsets):
        src = [i for i in range(f) if 0 <= i + d < f]
        if not src:
            continue
        dst = [i + d for i in src]
        n = len(src)
        p = rp.unproject(xy, depth[:, src], k[:, src][:, :, None, None])
        rel = ext[:, dst].inverse() @ ext[:, src]
        q = rp.transform_rigid(rp.homogenize_points(p), rel[:, :, None, None])[..., :3]
        uv = rp.project_camera_space(q, k[:, dst][:, :, None, None])
        zs = F.grid_sample(depth[:, dst].reshape(b * n, 1, h, w), (uv * 2 - 1).reshape(b * n, h, w, 2), mode="bilinear", padding_mode="border",
                           align_corners=False).reshape(b, n, h, w)
        qz = q[..., 2]
        inside = (uv >= 0).all(-1) & (uv < 1).all(-1)  # projection.py:294-295
        code = torch.where(~(qz > 0), 2, torch.where(inside, 0, 3)).to(torch.uint8)
        out["code"][:, src, o] = code
        out["error"][:, src, o] = torch.where(code == 0, (zs - qz) / qz, torch.zeros_like(qz))
        out["positions"][:, src, o], out["reprojected"][:, src, o], out["sampled"][:, src, o] = uv, qz, zs
    return out


def main():
    arrays = {}
    for name in GOLDEN_CASES:
        x, offsets = case_inputs(name), SPECS[name][2]
        r32 = reference_terms(x, offsets, torch.float32)
        with mg.fp64_reference():
            r64 = reference_terms(x, offsets, torch.float64)
        assert torch.equal(r32["code"], r64["code"]), f"{name}: the reference's fp32 and fp64 evaluations disagree on {int((r32['code'] != r64['code']).sum())} codes"
        sel = r64["code"] == 0
        assert int(sel.sum()) > 0
        for key in FIELDS:
            _, gap = assert_close_or_reference_gap(r32[key][sel], r64[key][sel], r32[key][sel], what=f"{name}.{key}")
            print(f"  {name}.{key}: fp32-to-fp64 gap {gap:.2e} over {int(sel.sum())} elements")
        if name == "edge":
            assert set(r64["code"].unique().tolist()) == {0, 1, 2, 3}, "the edge case must show every code"
        keep = GOLDEN_FIELDS.get(name, FIELDS) + ("code",)
        arrays.update({f"{name}_{k}": v for k, v in x.items()})
        arrays[f"{name}_offsets"] = torch.tensor(offsets)
        arrays.update({f"{name}_{k}": r32[k] for k in keep})
        arrays.update({f"{name}_f64_{k}": r64[k] for k in keep})
    mg.save("fn_depth_consistency", **arrays)


if __name__ == "__main__":
    main()
