"""Generate tests/golden/fn_extrinsics_regressed.npz and tests/golden/step_regressed_extrinsics.npz by running the REFERENCE's
ExtrinsicsRegressed (flowmap/model/extrinsics/extrinsics_regressed.py) on seeded inputs, in fp32 (its native precision) and in fp64
(same code, inputs up-cast, its hard-coded fp32 identities patched as oracle/make_golden.py does).  Needs the reference importable
(FLOWMAP_REFERENCE, as oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_extrinsics_regressed.py
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (puts the reference and its stubs on sys.path; generates nothing on import)
from oracle import flowmap_oracle as orc  # noqa: E402  (input generators only)

from flowmap.dataset.types import Batch  # noqa: E402
from flowmap.flow.flow_predictor import Flows  # noqa: E402
from flowmap.loss import get_losses  # noqa: E402
from flowmap.loss.loss_flow import LossFlowCfg  # noqa: E402
from flowmap.loss.loss_tracking import LossTrackingCfg  # noqa: E402
from flowmap.model.backbone.backbone_explicit_depth import BackboneExplicitDepthCfg  # noqa: E402
from flowmap.model.extrinsics.extrinsics_regressed import ExtrinsicsRegressed, ExtrinsicsRegressedCfg, quaternion_to_matrix  # noqa: E402
from flowmap.model.intrinsics.intrinsics_regressed import IntrinsicsRegressedCfg  # noqa: E402
from flowmap.model.model import Model, ModelCfg  # noqa: E402
from flowmap.model.projection import get_extrinsics  # noqa: E402
from flowmap.tracking.track_predictor import Tracks  # noqa: E402

F, H, W = 6, 24, 32
FOCAL = 0.85


def pose_parameters(pairs: int, seed: int):
    """Quaternions (0, 0, 0, 1) + N(0, 0.15), deliberately not normalised, one row of norm 0.5 and one of norm 2; translations N(0, 0.05)."""
    g = torch.Generator().manual_seed(seed)
    rotations = torch.zeros((pairs, 4))
    rotations[:, 3] = 1
    rotations = rotations + 0.15 * torch.randn((pairs, 4), generator=g)
    rotations[1] *= 0.5 / rotations[1].norm()
    rotations[3] *= 2.0 / rotations[3].norm()
    translations = 0.05 * torch.randn((pairs, 3), generator=g)
    return rotations, translations


def function_level(rotations, translations, cots, dtype):
    """tf as ExtrinsicsRegressed.forward builds it (extrinsics_regressed.py:78-81), its inverse, the chain, and the gradients of
    Σ tf·c0 + Σ tf⁻¹·c1 + Σ chain·c2."""
    q = rotations.to(dtype).clone().requires_grad_(True)
    t = translations.to(dtype).clone().requires_grad_(True)
    tf = torch.eye(4, dtype=dtype).broadcast_to((q.shape[0], 4, 4)).contiguous()
    tf[:, :3, :3] = quaternion_to_matrix(q)
    tf[:, :3, 3] = t
    inv = torch.linalg.inv(tf)
    ext = get_extrinsics(tf)
    c0, c1, c2 = (c.to(dtype) for c in cots)
    ((tf * c0).sum() + (inv * c1).sum() + (ext * c2).sum()).backward()
    return {"tf": tf, "tf_inv": inv, "extrinsics": ext, "g_rotations": q.grad, "g_translations": t.grad}


def run_step(depth, focal, rotations, translations, flows, hw, tracks=None, dtype=torch.float32):
    """The reference's Model with `extrinsics: regressed` + its losses, driven like ModelWrapperOverfit.training_step."""
    f = depth.shape[0]
    cfg = ModelCfg(BackboneExplicitDepthCfg("explicit_depth", 1.0, 100.0), IntrinsicsRegressedCfg("regressed", float(focal)),
                   ExtrinsicsRegressedCfg("regressed"), True)
    model = Model(cfg, num_frames=f, image_shape=hw)
    assert isinstance(model.extrinsics, ExtrinsicsRegressed)
    model.backbone.depth.data = depth.clone()
    model.extrinsics.rotations.data = rotations.clone()
    model.extrinsics.translations.data = translations.clone()
    if dtype == torch.float64:
        model = model.double()
    batch = Batch(torch.zeros((1, f, 3, *hw), dtype=dtype), torch.arange(f)[None], ["s"], ["d"])
    rflows = Flows(*(x.to(dtype) for x in (flows.forward, flows.backward, flows.forward_mask, flows.backward_mask)))
    rtracks = None
    loss_cfgs = [LossFlowCfg(0, 1000.0, "flow", mg.mapping_cfg("huber"))]
    if tracks is not None:
        rtracks = [Tracks(t.xy.to(dtype), t.visibility, t.start_frame) for t in tracks]
        loss_cfgs.append(LossTrackingCfg(0, 100.0, "tracking", mg.mapping_cfg("huber")))
    out = model(batch, rflows, 0)
    out.intrinsics.retain_grad()
    parts = [fn(batch, rflows, rtracks, out, 0) for fn in get_losses(loss_cfgs)]
    total = sum(parts)
    total.backward()
    gk = out.intrinsics.grad[0]  # the magnitude of the cancelling terms of dL/dfocal (tests/helpers.py: focal_close)
    return {
        "total": total, "loss_flow": parts[0], "loss_tracking": parts[1] if tracks is not None else torch.zeros(()),
        "extrinsics": out.extrinsics, "g_depth": model.backbone.depth.grad, "g_focal": model.intrinsics.focal_length.grad,
        "g_rotations": model.extrinsics.rotations.grad, "g_translations": model.extrinsics.translations.grad,
        "g_focal_terms": float((gk[:, 0, 0].abs() / hw[1] + gk[:, 1, 1].abs() / hw[0]).sum() * (hw[0] * hw[1]) ** 0.5),
    }


def main():
    rotations, translations = pose_parameters(F - 1, seed=41)
    g = torch.Generator().manual_seed(42)
    cots = (torch.randn((F - 1, 4, 4), generator=g), torch.randn((F - 1, 4, 4), generator=g), torch.randn((F, 4, 4), generator=g))
    r32 = function_level(rotations, translations, cots, torch.float32)
    with mg.fp64_reference():
        r64 = function_level(rotations, translations, cots, torch.float64)
    mg.save("fn_extrinsics_regressed", rotations=rotations, translations=translations, cot_tf=cots[0], cot_tf_inv=cots[1], cot_extrinsics=cots[2],
            **r32, **{f"f64_{k}": v for k, v in r64.items()})

    sc = orc.synth_scene(F, H, W, seed=7, focal=FOCAL)
    tracks = orc.synth_tracks(F, H, W, scene=sc, seed=7, interval=3, radius=2, grid=6)
    fl = sc["flows"]
    arrays = {}
    for tag, trk in (("", None), ("trk_", tracks)):
        s32 = run_step(sc["depth_init"], FOCAL, rotations, translations, fl, (H, W), trk)
        with mg.fp64_reference():
            s64 = run_step(sc["depth_init"].double(), FOCAL, rotations.double(), translations.double(), fl, (H, W), trk, dtype=torch.float64)
        arrays.update({f"{tag}{k}": v for k, v in s32.items()})
        arrays.update({f"{tag}f64_{k}": v for k, v in s64.items()})
    mg.save("step_regressed_extrinsics", depth=sc["depth_init"], focal=np.float32(FOCAL), rotations=rotations, translations=translations,
            fwd=fl.forward, bwd=fl.backward, fwd_mask=fl.forward_mask, bwd_mask=fl.backward_mask, **mg.tracks_arrays(tracks), **arrays)


if __name__ == "__main__":
    main()
