"""Generate tests/golden/fn_focal_sweep.npz: the softmin focal sweep of the REFERENCE on every frame pair of a case — per candidate the
flow error and the fitted pose, per pair the softmin weights, the blended focal length and the blended K — in fp32 (its native precision)
and in fp64 (same code, inputs up-cast, its hard-coded fp32 constants patched as oracle/make_golden.py does).  Data only.  Needs the
reference importable (FLOWMAP_REFERENCE, as oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_focal_sweep.py

The reference sweeps frames (0, 1) only, so pair k is its run on the two-frame slice (frames k and k+1, ``flows.backward[:, k:k+1]``,
``weights[:, k:k+1]``), one batch entry at a time (its window entry sums over the batch).  ``error`` and ``soft`` are composed from its own
``unproject``, ``align_surfaces``, ``compute_backward_flow`` and lines 105-129 of flowmap/model/intrinsics/intrinsics_softmin.py;
``poses`` are what its ``align_rigid`` returned inside ``align_surfaces`` (recorded); ``intrinsics`` is its ``IntrinsicsSoftmin.forward``
with ``torch.randperm`` replaced for the call so that it yields the case's indices, and ``focal`` its ``window[-1]`` in training mode.
Per case of tests/focal_sweep_cases.py: GOLDEN_CASES the keys are ``<case>_<field>`` with their ``<case>_f64_`` twins, beside the inputs
``<case>_depth`` / ``_weights`` / ``_bwd`` / ``_indices`` / ``_candidates``.  The cases that let the call draw its indices store what
``_ops.random_subset(h·w, h·w, seed=0)`` gives (the serial host build of the package's own function).  Every fp32 field is checked
against its fp64 twin with the tests' gate as it is written, and the gaps are printed.
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402
from einops import rearrange, reduce, repeat  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (puts the reference and its stubs on sys.path; generates nothing on import)

from flowmap.dataset.types import Batch  # noqa: E402
from flowmap.flow.flow_predictor import Flows  # noqa: E402
from flowmap.model import projection as rp  # noqa: E402
from flowmap.model.backbone.backbone import BackboneOutput  # noqa: E402
from flowmap.model.intrinsics import intrinsics_softmin as ism  # noqa: E402
from flowmap.model.intrinsics.common import focal_lengths_to_intrinsics  # noqa: E402

from conftest import assert_close_or_reference_gap  # noqa: E402

from focal_sweep_cases import FIELDS, GOLDEN_CASES, SPECS, candidates_of, case_indices, case_inputs, gate_soft  # noqa: E402


def composed(depth2, bwd1, wts1, candidates, indices, dtype):
    """error (b, n), soft (b, n), poses (b, n, 4, 4) of one two-frame slice, composed from the reference's functions (intrinsics_softmin.py:85-129)."""
    b, _, h, w = depth2.shape
    n = candidates.numel()
    candidate_intrinsics = focal_lengths_to_intrinsics(candidates, (h, w))
    xy, _ = rp.sample_image_grid((h, w), depth2.device)
    xy = xy.to(dtype)
    surfaces = rp.unproject(xy, repeat(depth2, "b f h w -> (b n) f h w", n=n), repeat(candidate_intrinsics, "n i j -> (b n) f () () i j", b=b, f=2))
    seen = {}
    original = rp.align_rigid

    def recorder(xyz_later, xyz_earlier, weights):
        seen["rel"] = original(xyz_later, xyz_earlier, weights)
        return seen["rel"]

    rp.align_rigid = recorder
    try:
        extrinsics = rp.align_surfaces(surfaces, repeat(bwd1, "b f h w xy -> (b n) f h w xy", n=n), repeat(wts1, "b f h w -> (b n) f h w", n=n), indices)
    finally:
        rp.align_rigid = original
    flowed = rp.compute_backward_flow(rearrange(surfaces, "bn f h w xyz -> bn f (h w) xyz")[:, :, indices], extrinsics,
                                      repeat(candidate_intrinsics, "n i j -> (b n) f i j", b=b, f=2))
    flowed = rearrange(flowed, "(b n) () p xy -> b n p xy", b=b, n=n)
    flow = flowed - rearrange(xy, "h w xy -> (h w) xy")[indices]
    flow_gt = rearrange(bwd1, "b () h w xy -> b () (h w) xy")[:, :, indices]
    weights = rearrange(wts1, "b () h w -> b () (h w) ()")[:, :, indices]
    error = reduce(((flow - flow_gt) * weights).abs(), "b n p xy -> b n", "sum")
    soft = torch.nn.functional.softmin((error - error.min(dim=1, keepdim=True).values) * 10, dim=1)
    return error, soft, rearrange(seen["rel"], "(b n) () i j -> b n i j", b=b, n=n)


def module_run(depth2, bwd1, wts1, n, indices, dtype):
    """(K (3, 3), focal ()) of ONE batch entry's two-frame slice by the reference's IntrinsicsSoftmin.forward in training mode."""
    _, _, h, w = depth2.shape
    cfg = ism.IntrinsicsSoftminCfg("softmin", indices.numel(), 0.5, 2.0, n, ism.RegressionCfg(1000, 1000))
    module = ism.IntrinsicsSoftmin(cfg).to(dtype).train()
    batch = Batch(torch.zeros((1, 2, 3, h, w)), torch.arange(2)[None], ["s"], ["d"])
    real_randperm, grid32 = torch.randperm, ism.sample_image_grid
    torch.randperm = lambda *a, **k: indices.clone()
    if dtype == torch.float64:
        ism.sample_image_grid = lambda *a, **k: (lambda xy_ij: (xy_ij[0].double(), xy_ij[1]))(grid32(*a, **k))
    try:
        k = module.forward(batch, Flows(bwd1, bwd1, None, None), BackboneOutput(depth2, wts1), 0)
    finally:
        torch.randperm, ism.sample_image_grid = real_randperm, grid32
    assert k.dtype == dtype and len(module.window) == 1
    return k[0, 0].detach(), module.window[-1]


def reference_sweep(x, candidates, indices, dtype):
    depth, wts, bwd = (x[key].to(dtype) for key in ("depth", "weights", "bwd"))
    b, f, _, _ = depth.shape
    cand = candidates.to(dtype)
    out = {key: [] for key in FIELDS}
    for i in range(f - 1):
        error, soft, poses = composed(depth[:, i:i + 2], bwd[:, i:i + 1], wts[:, i:i + 1], cand, indices, dtype)
        runs = [module_run(depth[e:e + 1, i:i + 2], bwd[e:e + 1, i:i + 1], wts[e:e + 1, i:i + 1], cand.numel(), indices, dtype) for e in range(b)]
        for key, value in (("error", error), ("soft", soft), ("poses", poses), ("intrinsics", torch.stack([r[0] for r in runs])),
                           ("focal", torch.stack([r[1] for r in runs]))):
            out[key].append(value)
    return {key: torch.stack(v, dim=1) for key, v in out.items()}


def drawn_indices(name):
    indices = case_indices(name)
    if indices is not None:
        return indices
    from flowmap_amd import _lib, _ops
    from helpers import build_host_sim

    h, w = SPECS[name][0][2:]
    _lib.set_library_for_testing(build_host_sim())
    try:
        return _ops.random_subset(h * w, h * w, "cpu", seed=0)
    finally:
        _lib.set_library_for_testing(None)


def main():
    arrays = {}
    for name in GOLDEN_CASES:
        x, indices, candidates = case_inputs(name), drawn_indices(name), candidates_of(name)
        arrays.update({f"{name}_{key}": v for key, v in x.items()})
        arrays[f"{name}_indices"], arrays[f"{name}_candidates"] = indices, candidates
        r32 = reference_sweep(x, candidates, indices, torch.float32)
        with mg.fp64_reference():
            r64 = reference_sweep(x, candidates, indices, torch.float64)
        for key in FIELDS:
            assert r64[key].dtype == torch.float64 and r32[key].dtype == torch.float32
            if key == "soft":
                _, gap = gate_soft(r32[key], r64[key], r32[key], f"{name}.{key}")
            else:
                _, gap = assert_close_or_reference_gap(r32[key], r64[key], r32[key], what=f"{name}.{key}")
            print(f"  {name}.{key}: fp32-to-fp64 gap {gap:.2e}")
            arrays[f"{name}_{key}"] = r32[key]
            arrays[f"{name}_f64_{key}"] = r64[key]
    mg.save("fn_focal_sweep", **arrays)


if __name__ == "__main__":
    main()
