"""Device-agnostic cases of the regressed extrinsics (flowmap_amd/model/extrinsics_regressed.py, _ops.QuaternionPoses): run on the host
double by tests/test_extrinsics_regressed.py and on the GPU by tests/test_gpu_extrinsics_regressed.py."""

from __future__ import annotations

import torch

import flowmap_amd
from conftest import assert_close, assert_close_or_reference_gap, load_golden, relerr, t
from flowmap_amd import Batch, _ops
from flowmap_amd.loss import LossFlow, LossFlowCfg, LossTracking, LossTrackingCfg
from flowmap_amd.model.extrinsics_regressed import ExtrinsicsRegressed, ExtrinsicsRegressedCfg
from flowmap_amd.model.model import BackboneExplicitDepthCfg, IntrinsicsRegressedCfg, Model, ModelCfg
from flowmap_amd.model.projection import LazyExtrinsics
from helpers import focal_close, mapping_cfg, to_flows, to_tracks
from oracle import flowmap_oracle as orc

STEP_GRADS = ("g_rotations", "g_translations", "g_depth")


def golden_flows(g):
    return orc.OFlows(t(g["fwd"]), t(g["bwd"]), t(g["fwd_mask"]), t(g["bwd_mask"]))


def golden_tracks(g):
    return [orc.OTracks(t(g[f"trk{i}_xy"]), t(g[f"trk{i}_vis"]), int(g[f"trk{i}_start"])) for i in range(int(g["n_segments"]))]


def quat_poses_torch(q, tr):
    """extrinsics_regressed.py:17-39,78-81 restated: (P,4) quaternions as (i, j, k, r) and (P,3) translations -> (P,4,4), any dtype."""
    i, j, k, r = q.unbind(-1)
    two_s = 2 / ((q * q).sum(-1) + 1e-8)
    rot = torch.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                       two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                       two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], -1).reshape(-1, 3, 3)
    top = torch.cat([rot, tr[:, :, None]], dim=2)
    bottom = torch.tensor([0, 0, 0, 1], dtype=q.dtype, device=q.device).expand(q.shape[0], 1, 4)
    return torch.cat([top, bottom], dim=1)


def pose_parameters(pairs: int, seed: int, sigma: float = 0.15):
    """The golden generator's recipe (tools/make_golden_extrinsics_regressed.py): un-normalised quaternions near the identity, one row of
    norm 0.5 and one of norm 2 where there are that many pairs.  ``sigma``: the spread of the quaternion about (0, 0, 0, 1); a pair's
    rotation angle is about 2·sigma·sqrt(3) (0.15: 30 degrees, tails beyond 60)."""
    g = torch.Generator().manual_seed(seed)
    rotations = torch.zeros((pairs, 4))
    rotations[:, 3] = 1
    rotations = rotations + sigma * torch.randn((pairs, 4), generator=g)
    if pairs > 1:
        rotations[1] *= 0.5 / rotations[1].norm()
    if pairs > 3:
        rotations[3] *= 2.0 / rotations[3].norm()
    return rotations, 0.05 * torch.randn((pairs, 3), generator=g)


def function_level(rotations, translations, cots, device):
    """_ops.QuaternionPoses with the chain from the forward launch, and the gradients of Σ tf·c0 + Σ tf⁻¹·c1 + Σ chain·c2."""
    q = rotations.clone().to(device).requires_grad_(True)
    tr = translations.clone().to(device).requires_grad_(True)
    rel, rel_inv, ext = _ops.QuaternionPoses.apply(q, tr, True)
    c0, c1, c2 = (c.to(device) for c in cots)
    ((rel[0] * c0).sum() + (rel_inv[0] * c1).sum() + (ext[0] * c2).sum()).backward()
    return {"tf": rel[0].detach().cpu(), "tf_inv": rel_inv[0].detach().cpu(), "extrinsics": ext[0].detach().cpu(),
            "g_rotations": q.grad.cpu(), "g_translations": tr.grad.cpu()}


def function_truth(rotations, translations, cots, dtype=torch.float64):
    q = rotations.to(dtype).clone().requires_grad_(True)
    tr = translations.to(dtype).clone().requires_grad_(True)
    tf = quat_poses_torch(q, tr)
    inv = torch.linalg.inv(tf)
    ext = orc.chain_poses(tf)
    c0, c1, c2 = (c.to(dtype) for c in cots)
    ((tf * c0).sum() + (inv * c1).sum() + (ext * c2).sum()).backward()
    return {"tf": tf.detach(), "tf_inv": inv.detach(), "extrinsics": ext.detach(), "g_rotations": q.grad, "g_translations": tr.grad}


def case_function_golden(device):
    g = load_golden("fn_extrinsics_regressed")
    cots = tuple(t(g[k]) for k in ("cot_tf", "cot_tf_inv", "cot_extrinsics"))
    ours = function_level(t(g["rotations"]), t(g["translations"]), cots, device)
    for key in ("tf", "tf_inv", "extrinsics", "g_rotations", "g_translations"):
        assert_close(ours[key], t(g[key]), 1e-4, what=f"{key} vs the reference's fp32")
        assert_close_or_reference_gap(ours[key], t(g["f64_" + key]), t(g[key]), 1e-4, what=key)
    eye = torch.eye(4, dtype=torch.float64).expand(ours["tf"].shape[0], 4, 4)
    product = ours["tf_inv"].double() @ ours["tf"].double()
    # an entry of the product is a sum of four products of entries of magnitude <~ 1.1, each factor rounded to fp32 once (2^-24):
    # 4 x 2 x 2^-24 x 1.2 < 2^-20
    assert (product - eye).abs().max().item() <= 2.0**-20, (product - eye).abs().max().item()
    # the rows of norm 0.5 and 2: a rotation all the same (s = 2/|q|² normalises), each to the fp64 truth on its own
    for row in (1, 3):
        assert abs(float(t(g["rotations"])[row].norm()) - (0.5 if row == 1 else 2.0)) < 1e-6
        for key in ("tf", "tf_inv", "g_rotations"):
            assert_close_or_reference_gap(ours[key][row], t(g["f64_" + key])[row], t(g[key])[row], 1e-4, what=f"{key}[{row}]")
    return ours


def case_finite_differences(device, pairs=5, seed=3):
    """g_q / g_t against central finite differences, in fp64, of the torch restatement above (gradcheck's recipe: eps 1e-6)."""
    rotations, translations = pose_parameters(pairs, seed)
    g = torch.Generator().manual_seed(seed + 100)
    cots = (torch.randn((pairs, 4, 4), generator=g), torch.randn((pairs, 4, 4), generator=g), torch.randn((pairs + 1, 4, 4), generator=g))
    for c in cots[:2]:
        c[:, 3] = 0  # (the bottom rows of the pose gradients carry no meaning: csrc/fm_pose.h)
    ours = function_level(rotations, translations, cots, device)

    def value(q, tr):
        tf = quat_poses_torch(q, tr)
        return float((tf * cots[0].double()).sum() + (torch.linalg.inv(tf) * cots[1].double()).sum() + (orc.chain_poses(tf) * cots[2].double()).sum())

    q64, t64 = rotations.double(), translations.double()
    eps = 1e-6
    for name, base, other, first in (("g_rotations", q64, t64, True), ("g_translations", t64, q64, False)):
        numeric = torch.zeros_like(base)
        for idx in range(base.numel()):
            step = torch.zeros(base.numel(), dtype=torch.float64)
            step[idx] = eps
            step = step.reshape(base.shape)
            hi = value(base + step, other) if first else value(other, base + step)
            lo = value(base - step, other) if first else value(other, base - step)
            numeric.view(-1)[idx] = (hi - lo) / (2 * eps)
        assert_close(ours[name], numeric, 1e-4, what=f"{name} vs finite differences")


def case_identity(device, pairs=4):
    """The module's initial values: every pose, its inverse and the chain are exactly the identity."""
    module = ExtrinsicsRegressed(ExtrinsicsRegressedCfg("regressed"), pairs + 1).to(device)
    rel, rel_inv, ext = _ops.QuaternionPoses.apply(module.rotations, module.translations, True)
    eye = torch.eye(4)
    for name, value in (("tf", rel), ("tf_inv", rel_inv), ("extrinsics", ext)):
        # s = 2/(1 + 1e-8) rounds the rotation's diagonal to 1 − 2·0 exactly: every B entry on the diagonal is 0 for q = (0, 0, 0, 1)
        assert torch.equal(value[0].cpu(), eye.expand(value.shape[1], 4, 4)), name


def build_model(depth, focal, rotations, translations, device):
    f, h, w = depth.shape
    cfg = ModelCfg(BackboneExplicitDepthCfg("explicit_depth", 1.0, 100.0), IntrinsicsRegressedCfg("regressed", float(focal)), ExtrinsicsRegressedCfg("regressed"))
    model = Model(cfg, num_frames=f, image_shape=(h, w))
    assert isinstance(model.extrinsics, ExtrinsicsRegressed)
    model.backbone.depth.data = depth.clone()
    model.extrinsics.rotations.data = rotations.clone()
    model.extrinsics.translations.data = translations.clone()
    return model.to(device)


def make_losses(with_tracks, kind="huber"):
    losses = [LossFlow(LossFlowCfg(0, 1000.0, "flow", mapping_cfg(kind)))]
    if with_tracks:
        losses.append(LossTracking(LossTrackingCfg(0, 100.0, "tracking", mapping_cfg(kind))))
    return losses


def run_ours(depth, focal, rotations, translations, oflows, otracks=None, device="cpu", steps=1):
    """One step (the last of ``steps``) of Model(extrinsics: regressed) + LossFlow (+ LossTracking) on lazy surfaces."""
    f, h, w = depth.shape
    flowmap_amd.set_lazy_surfaces(True)
    try:
        model = build_model(depth, focal, rotations, translations, device)
        batch = Batch(torch.zeros((1, f, 3, h, w), device=device))
        flows, tracks = to_flows(oflows, device), to_tracks(otracks, device)
        losses = make_losses(tracks is not None)
        for _ in range(steps):
            model.zero_grad(set_to_none=True)
            out = model(batch, flows, 0)
            parts = [fn(batch, flows, tracks, out, 0) for fn in losses]
            total = sum(parts)
            total.backward()
        return {
            "total": total.detach().cpu(), "loss_flow": parts[0].detach().cpu(),
            "loss_tracking": parts[1].detach().cpu() if tracks is not None else torch.zeros(()),
            "extrinsics": torch.as_tensor(out.extrinsics.materialize() if isinstance(out.extrinsics, LazyExtrinsics) else out.extrinsics).detach().cpu(),
            "g_depth": model.backbone.depth.grad.cpu(), "g_focal": model.intrinsics.focal_length.grad.cpu(),
            "g_rotations": model.extrinsics.rotations.grad.cpu(), "g_translations": model.extrinsics.translations.grad.cpu(),
            "output": out, "model": model,
        }
    finally:
        flowmap_amd.set_lazy_surfaces(False)


def run_oracle(depth, focal, rotations, translations, oflows, otracks=None, dtype=torch.float64):
    """The same step rebuilt from the oracle's pieces: chain_poses over the restated matrices, flow_loss / tracking_loss."""
    f, h, w = depth.shape
    d = depth.to(dtype).clone().requires_grad_(True)
    fo = torch.tensor(float(focal), dtype=dtype, requires_grad=True)
    q = rotations.to(dtype).clone().requires_grad_(True)
    tr = translations.to(dtype).clone().requires_grad_(True)
    fl = orc.OFlows(*(x.to(dtype) for x in (oflows.forward, oflows.backward, oflows.forward_mask, oflows.backward_mask)))
    tracks = None if otracks is None else [orc.OTracks(s.xy.to(dtype), s.visibility, s.start_frame) for s in otracks]
    k = orc.focal_to_k(fo, (h, w)).expand(1, f, 3, 3)
    k.retain_grad()
    xy, _ = orc.pixel_grid((h, w), d.device, dtype)
    surfaces = orc.lift(xy, d[None], k[:, :, None, None])
    ext = orc.chain_poses(quat_poses_torch(q, tr))[None]
    flow = 1000.0 * orc.flow_loss(surfaces, ext, k, fl, (h, w))
    tracking = 100.0 * orc.tracking_loss(surfaces, ext, k, tracks, (h, w)) if tracks is not None else torch.zeros((), dtype=dtype)
    total = flow + tracking
    total.backward()
    gk = k.grad[0]
    return {"total": total.detach(), "loss_flow": flow.detach(), "loss_tracking": tracking.detach(), "extrinsics": ext.detach(), "g_depth": d.grad,
            "g_focal": fo.grad, "g_rotations": q.grad, "g_translations": tr.grad,
            "g_focal_terms": float((gk[:, 0, 0].abs() / w + gk[:, 1, 1].abs() / h).sum() * (h * w) ** 0.5)}


def compare_step(ours, truth, ref32, ratios=None, what=""):
    """Loss and the four gradients at the project's standing gate: max(1e-4, 2 x the reference's own fp32 gap) of the fp64 truth;
    dL/dfocal through helpers.focal_close.  ``ratios``: collects err / bound per quantity (the worst are quoted in DESIGN.md)."""
    for key in ("total", "loss_flow", "loss_tracking", "extrinsics") + STEP_GRADS:
        if key == "loss_tracking" and float(truth[key]) == 0.0:
            assert float(ours[key]) == 0.0
            continue
        e, gap = assert_close_or_reference_gap(ours[key], truth[key], ref32[key], 1e-4, what=f"{what}{key}")
        if ratios is not None:
            ratios[key] = max(ratios.get(key, 0.0), e / max(1e-4, 2.0 * gap))
    err, bound = focal_close(ours["g_focal"], {"g_focal": truth["g_focal"], "g_focal_terms": truth.get("g_focal_terms")}, ref32, what=f"{what}g_focal")
    if ratios is not None:
        ratios["g_focal"] = max(ratios.get("g_focal", 0.0), err / bound)


def case_step_golden(device, with_tracks, ratios=None):
    g = load_golden("step_regressed_extrinsics")
    tag = "trk_" if with_tracks else ""
    ours = run_ours(t(g["depth"]), float(g["focal"]), t(g["rotations"]), t(g["translations"]), golden_flows(g), golden_tracks(g) if with_tracks else None, device)
    keys = ("total", "loss_flow", "loss_tracking", "extrinsics", "g_focal") + STEP_GRADS
    truth = {k: t(g[f"{tag}f64_{k}"]) for k in keys}
    truth["g_focal_terms"] = float(g[f"{tag}f64_g_focal_terms"])
    ref32 = {k: t(g[f"{tag}{k}"]) for k in keys}
    compare_step(ours, truth, ref32, ratios, what=f"golden[{tag or 'flow'}] ")
    # the oracle's restatement of the same step agrees with the reference's fp64 run: the truth of the fixture-free cases below
    again = run_oracle(t(g["depth"]), float(g["focal"]), t(g["rotations"]), t(g["translations"]), golden_flows(g), golden_tracks(g) if with_tracks else None)
    for k in keys:
        assert relerr(again[k], truth[k]) <= 1e-8, (k, relerr(again[k], truth[k]))
    return ours


def scene_problem(f, h, w, seed):
    sc = orc.synth_scene(f, h, w, seed=seed)
    tracks = orc.synth_tracks(f, h, w, scene=sc, seed=seed, interval=3, radius=2, grid=6)
    rotations, translations = pose_parameters(f - 1, seed + 1)
    return sc["depth_init"], float(sc["focal"]), rotations, translations, sc["flows"], tracks


def case_step_oracle(device, f, h, w, seed, with_tracks=True, ratios=None, problem=None):
    depth, focal, rotations, translations, flows, tracks = problem or scene_problem(f, h, w, seed)
    tracks = tracks if with_tracks else None
    ours = run_ours(depth, focal, rotations, translations, flows, tracks, device)
    truth = run_oracle(depth, focal, rotations, translations, flows, tracks, torch.float64)
    ref32 = run_oracle(depth, focal, rotations, translations, flows, tracks, torch.float32)
    compare_step(ours, truth, ref32, ratios, what=f"{f}x{h}x{w} ")
    return ours
