"""Generate tests/golden/fn_flow_residuals.npz: the per-pixel quantities of the REFERENCE's LossFlow.compute_unweighted_loss
(flowmap/loss/loss_flow.py:46-68) — forward_loss / backward_loss BEFORE the mask and the pose-induced flows xy_flowed − xy — on seeded
inputs, in fp32 (its native precision) and in fp64 (same code, inputs up-cast, its hard-coded fp32 constants patched as
oracle/make_golden.py does).  Data only.  Needs the reference importable (FLOWMAP_REFERENCE, as oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_flow_residuals.py

Cases (keys ``<case>_<array>``; every case has depth, k, extrinsics, fwd, bwd, fwd_mask, bwd_mask and, per mapping kind,
``<kind>_forward`` / ``<kind>_backward`` with their ``f64_`` twins, plus ``pred_forward`` / ``pred_backward``):
  a     1 x 2 x 5 x 7     one pair, fewer pixels than a wavefront, one K shared by the frames
  b     1 x 5 x 17 x 23   odd sizes, a K per frame with the principal point off the centre
  c     2 x 4 x 9 x 12    two batch entries (what the frame-window / batch-slice tests read in place)
  edge  1 x 3 x 9 x 12    pair 0: a band of frame 0 has depth 0 and the pose moves it to Z' = −1e-5 exactly, so project_camera_space
                          divides by zero and clamps (±1e8, NaN -> 0); pair 1: the pose moves half of frame 1 behind the camera
The general cases are well conditioned (depth >= 0.5, rotations of a few degrees): no pixel comes near the camera plane.  Every case is
checked here on the CPU: the reference's fp32 output must pass the tests' gate (conftest.assert_close_or_reference_gap) against its own
fp64 run, and the edge case must really clamp.
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

import flowmap.loss.loss_flow as ref_loss_flow  # noqa: E402
from flowmap.loss.mapping import get_mapping  # noqa: E402
from flowmap.model import projection as rp  # noqa: E402

from conftest import assert_close_or_reference_gap  # noqa: E402

from flow_residual_cases import CLAMPED, KINDS, inputs  # noqa: E402  (the seeded input recipe the tests' larger shapes use too)


def edge_inputs(seed):
    b, f, h, w = 1, 3, 9, 12
    x = inputs(seed, b, f, h, w, per_frame_k=False)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))  # the fp32 value project_camera_space adds to Z'
    x["depth"][0, 0, 3:6] = 0.0  # with the pose below: Z' = −eps exactly, X' = 0.3, Y' = 0 -> (+inf, NaN, −inf) -> (1e8, 0, −1e8)
    x["depth"][0, 1, :5] = 0.5 + 0.3 * x["depth"][0, 1, :5] / 2.0  # 0.575 .. 0.8: behind the camera after the second pose
    x["depth"][0, 1, 5:] = 1.5 + 0.25 * x["depth"][0, 1, 5:]  # 1.6 .. 2.0: in front of it
    ext = torch.eye(4).repeat(b, f, 1, 1)
    ext[0, 1, :3, 3] = torch.tensor([-0.3, 0.0, eps])  # later⁻¹·earlier = [I | (0.3, 0, −eps)]
    ext[0, 2, :3, 3] = ext[0, 1, :3, 3] + torch.tensor([0.02, -0.01, 1.1])  # pair 1: forward along the axis by 1.1
    x["extrinsics"] = ext
    return x


def reference_terms(x, dtype):
    """loss_flow.py:39-68 up to (not including) the masked sums, for the three mappings."""
    depth, k, ext = (x[n].to(dtype) for n in ("depth", "k", "extrinsics"))
    fwd, bwd = x["fwd"].to(dtype), x["bwd"].to(dtype)
    _, _, h, w = depth.shape
    xy, _ = ref_loss_flow.sample_image_grid((h, w), depth.device)
    surfaces = rp.unproject(xy, depth, k[:, :, None, None])  # model.py: the surfaces the loss is handed
    pred_f = rp.compute_forward_flow(surfaces, ext, k) - xy
    pred_b = rp.compute_backward_flow(surfaces, ext, k) - xy
    out = {"pred_forward": pred_f, "pred_backward": pred_b}
    for kind in KINDS:
        mapping = get_mapping(mg.mapping_cfg(kind))
        out[f"{kind}_forward"] = mapping.forward(pred_f, fwd, (h, w))
        out[f"{kind}_backward"] = mapping.forward(pred_b, bwd, (h, w))
    return out


def main():
    arrays = {}
    cases = {"a": inputs(101, 1, 2, 5, 7, False), "b": inputs(102, 1, 5, 17, 23, True), "c": inputs(103, 2, 4, 9, 12, True), "edge": edge_inputs(104)}
    for name, x in cases.items():
        r32 = reference_terms(x, torch.float32)
        with mg.fp64_reference():
            r64 = reference_terms(x, torch.float64)
        for key in r32:
            e, gap = assert_close_or_reference_gap(r32[key], r64[key], r32[key], what=f"{name}.{key}")
            print(f"  {name}.{key}: fp32-to-fp64 gap {gap:.2e}")
        clamped = (r32["pred_forward"].abs() > CLAMPED).any(-1) | (r32["pred_backward"].abs() > CLAMPED).any(-1)
        if name == "edge":
            assert int(clamped.sum()) == 3 * 12 and bool(clamped[0, 0, 3:6].all()), "the edge case must clamp exactly the zero-depth band of pair 0"
            behind = x["depth"][0, 1, :5] - 1.1 < 0
            assert bool(behind.all()), "the edge case must put the upper rows of frame 1 behind the camera"
        else:
            assert not bool(clamped.any()), f"{name}: a general case clamps — badly conditioned, replace it"
            assert max(float(r32[f"pred_{d}"].abs().max()) for d in ("forward", "backward")) < 1.0, f"{name}: a pixel comes near the camera plane"
        arrays.update({f"{name}_{k}": v for k, v in x.items()})
        arrays.update({f"{name}_{k}": v for k, v in r32.items()})
        arrays.update({f"{name}_f64_{k}": v for k, v in r64.items()})
    mg.save("fn_flow_residuals", **arrays)


if __name__ == "__main__":
    main()
