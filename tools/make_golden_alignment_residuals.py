"""Generate tests/golden/fn_alignment_residuals.npz: the terms of the objective the REFERENCE's Procrustes fit minimises, per correspondence
— T·p − q, its squared norm and the weighted mean per pair — in fp32 (its native precision) and in fp64 (same code, inputs up-cast, its
hard-coded fp32 constants patched as oracle/make_golden.py does).  Data only.  Needs the reference importable (FLOWMAP_REFERENCE, as
oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_alignment_residuals.py

The correspondences are the reference's own: its ``align_surfaces`` (flowmap/model/projection.py:213-252) runs with ``align_rigid``
temporarily replaced by a recorder that keeps (xyz_later, xyz_earlier, weights) and forwards to the original; T·p − q is formed with its
``transform_rigid`` and ``homogenize_points``.  Per case (tests/alignment_residual_cases.py: FIXTURE_SPECS) and route — ``dense``: every
pixel, T_i = E_i⁻¹·E_{i+1} of the given extrinsics (projection.py:176); ``given``: the case's indices, the same T; ``fit``: the case's
indices, the T align_rigid returned on them (its chain is stored as ``<case>_fit_extrinsics``) — the keys are
``<case>_<route>_offset`` (b, f-1, P, 3), ``_residual`` (b, f-1, P), ``_loss`` (b, f-1) with their ``<case>_f64_`` twins, beside the inputs
``<case>_depth`` / ``_k`` / ``_extrinsics`` / ``_bwd`` / ``_weights`` / ``_indices``.  Every fp32 map is checked against its fp64 twin with
the tests' gate as it is written.
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (puts the reference and its stubs on sys.path; generates nothing on import)

from flowmap.model import projection as rp  # noqa: E402

from conftest import assert_close_or_reference_gap  # noqa: E402

from alignment_residual_cases import FIXTURE_SPECS, fixture_indices, fixture_inputs  # noqa: E402


def reference_terms(x, indices, dtype, fit):
    """The reference's correspondences on ``indices`` (None: every pixel) and the terms of its objective at the given or the fitted T."""
    depth, k, ext, bwd, wts = (x[n].to(dtype) for n in ("depth", "k", "extrinsics", "bwd", "weights"))
    b, f, h, w = depth.shape
    xy, _ = rp.sample_image_grid((h, w), depth.device)
    surfaces = rp.unproject(xy.to(dtype), depth, k[:, :, None, None])  # model.py: the surfaces the fit is handed
    seen = {}
    original = rp.align_rigid

    def recorder(xyz_later, xyz_earlier, weights):
        seen["p"], seen["q"], seen["w"] = xyz_later, xyz_earlier, weights
        seen["rel"] = original(xyz_later, xyz_earlier, weights)
        return seen["rel"]

    rp.align_rigid = recorder
    try:
        fitted = rp.align_surfaces(surfaces, bwd, wts, torch.arange(h * w) if indices is None else indices)
    finally:
        rp.align_rigid = original
    rel = seen["rel"] if fit else rp.earlier(ext).inverse() @ rp.later(ext)  # projection.py:176
    offset = rp.transform_rigid(rp.homogenize_points(seen["p"]), rel[:, :, None])[..., :3] - seen["q"]
    residual = (offset * offset).sum(dim=-1)
    return {"offset": offset, "residual": residual, "loss": (seen["w"] * residual).sum(dim=-1) / seen["w"].sum(dim=-1)}, fitted


def main():
    arrays = {}
    for name in FIXTURE_SPECS:
        x, indices = fixture_inputs(name), fixture_indices(name)
        arrays.update({f"{name}_{key}": v for key, v in x.items()})
        arrays[f"{name}_indices"] = indices
        for route, idx, fit in (("dense", None, False), ("given", indices, False), ("fit", indices, True)):
            r32, fitted32 = reference_terms(x, idx, torch.float32, fit)
            with mg.fp64_reference():
                r64, _ = reference_terms(x, idx, torch.float64, fit)
            if fit:
                arrays[f"{name}_fit_extrinsics"] = fitted32
            for key in ("offset", "residual", "loss"):
                _, gap = assert_close_or_reference_gap(r32[key], r64[key], r32[key], what=f"{name}.{route}.{key}")
                print(f"  {name}.{route}.{key}: fp32-to-fp64 gap {gap:.2e}")
                arrays[f"{name}_{route}_{key}"] = r32[key]
                arrays[f"{name}_f64_{route}_{key}"] = r64[key]
    mg.save("fn_alignment_residuals", **arrays)


if __name__ == "__main__":
    main()
