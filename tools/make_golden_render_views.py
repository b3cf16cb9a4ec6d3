"""Generate tests/golden/fn_render_views.npz: the rendered views (flowmap_amd.model.projection.render_views) as the REFERENCE's own
functions compose them — sample_image_grid, unproject, homogenize_points, transform_rigid with the relative pose E_v⁻¹·E_i and
project_camera_space (flowmap/model/projection.py:93-113, :76-90, :11-15, :25-30, :49-58) — on the seeded inputs of
tests/render_views_cases.py, in fp32 (its native precision) and in fp64 (same code, inputs up-cast, its hard-coded fp32 constants patched
as oracle/make_golden.py does).  The reference has no splat: the z-buffer decision on top of its positions is the cases module's
``winners``.  Data only.  Needs the reference importable (FLOWMAP_REFERENCE, as oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_render_views.py

Keys ``<case>_<array>``: depth, k, ext, colors (the inputs), pairs (n_pairs, 2), per (view, source pixel) uv (b, V, F, h·w, 2) and qz
(b, V, F, h·w) — NaN where (view, frame) is no pair of the call — with their ``f64_`` twins, and per target pixel win_source (b, V, oh·ow;
−1: hole) and win_depth, again with ``f64_`` twins.  Every case is checked here on the CPU: the winners of the two evaluations may differ on
at most 0.5 % of the target pixels (the tests' condition).
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

from render_views_cases import GOLDEN_CASES, call_of, case_inputs, evaluate, winners  # noqa: E402


def reference_functions(dtype):
    return (lambda shape: rp.sample_image_grid(shape, torch.device("cpu"))[0].to(dtype), rp.unproject, rp.homogenize_points, rp.transform_rigid,
            rp.project_camera_space)


def main():
    arrays = {}
    for name in GOLDEN_CASES:
        x = case_inputs(name)
        _, view_k, view_ext, pairs, shape, radius, near = call_of(name)
        r32 = evaluate(x, view_k, view_ext, pairs, torch.float32, reference_functions(torch.float32))
        with mg.fp64_reference():
            r64 = evaluate(x, view_k, view_ext, pairs, torch.float64, reference_functions(torch.float64))
        w32, w64 = winners(r32, shape, radius, near), winners(r64, shape, radius, near)
        differ = int((w32[0] != w64[0]).sum())
        assert differ <= 5e-3 * w64[0].numel(), f"{name}: the reference's fp32 and fp64 evaluations disagree on {differ} winners"
        print(f"  {name}: {len(pairs)} pairs, {int((w64[0] >= 0).sum())} of {w64[0].numel()} target pixels covered, {differ} winners differ between fp32 and fp64")
        arrays.update({f"{name}_{k}": v for k, v in x.items()})
        arrays[f"{name}_pairs"] = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2)
        for prefix, ev, win in (("", r32, w32), ("f64_", r64, w64)):
            arrays[f"{name}_{prefix}uv"], arrays[f"{name}_{prefix}qz"] = ev["uv"], ev["qz"]
            arrays[f"{name}_{prefix}win_source"], arrays[f"{name}_{prefix}win_depth"] = win[0].to(torch.int32), win[1]
    mg.save("fn_render_views", **arrays)


if __name__ == "__main__":
    main()
