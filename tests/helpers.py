"""Shared helpers for the parity tests: build/inject the host test double, convert
oracle inputs to flowmap_amd inputs, run one optimisation step through either side."""

from __future__ import annotations

import os
import subprocess
from pathlib import Path

import torch

from conftest import assert_close, assert_close_or_reference_gap, assert_grad_close

import flowmap_amd
from flowmap_amd import Batch, Flows, Tracks
from flowmap_amd.loss import LossFlow, LossFlowCfg, LossTracking, LossTrackingCfg
from flowmap_amd.loss.mapping import MappingHuberCfg, MappingL1Cfg, MappingL2Cfg
from flowmap_amd.model.extrinsics_procrustes import ExtrinsicsProcrustesCfg
from flowmap_amd.model.model import BackboneExplicitDepthCfg, IntrinsicsRegressedCfg, Model, ModelCfg
from oracle import flowmap_oracle as orc

ROOT = Path(__file__).resolve().parent.parent
SIM_SRC = ROOT / "tests" / "host_sim" / "fm_host_sim.cpp"
SIM_LIB = ROOT / "tests" / "host_sim" / "libfm_host_sim.so"


def build_host_sim() -> Path:
    deps = [SIM_SRC, *(ROOT / "flowmap_amd" / "csrc").glob("*.h"), ROOT / "include" / "flowmap_hip.h"]
    if not SIM_LIB.exists() or SIM_LIB.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(
            ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", str(SIM_SRC), "-o", str(SIM_LIB)], check=True
        )
    return SIM_LIB


def mapping_cfg(kind: str, delta: float = 0.01):
    return {"huber": MappingHuberCfg("huber", delta), "l1": MappingL1Cfg("l1"), "l2": MappingL2Cfg("l2")}[kind]


def to_flows(of: orc.OFlows, device) -> Flows:
    return Flows(of.forward.to(device), of.backward.to(device), of.forward_mask.to(device), of.backward_mask.to(device))


def to_tracks(ot, device):
    if ot is None:
        return None
    return [Tracks(t.xy.to(device), t.visibility.to(device), t.start_frame) for t in ot]


def run_ours(depth, wlogit, focal, oflows, hw, num_points, otracks=None, kind="huber", device="cpu", lazy=True,
             flow_weight=1000.0, track_weight=100.0, loss_scale=1.0, steps=1):
    """One step through flowmap_amd exactly as ModelWrapperOverfit.training_step would
    drive it.  Returns dict of loss values and parameter gradients (on CPU).  ``steps`` > 1: the same step repeated on the
    same parameters (no optimiser), the LAST one reported — from its second step on a flow + tracking loop runs the tap
    exchange, from its third the tracking loss samples the compact tap image (flowmap_amd/_ops.py: TapPlan)."""
    from flowmap_amd import config

    f = depth.shape[0]
    flowmap_amd.set_lazy_surfaces(lazy)
    # (a repeated step is asked for to exercise the tap exchange, whatever the size)
    with config.override(**({"tap_exchange_min_bytes": 0} if steps > 1 else {})):
        try:
            cfg = ModelCfg(
                BackboneExplicitDepthCfg("explicit_depth", 1.0, 100.0),
                IntrinsicsRegressedCfg("regressed", float(focal)),
                ExtrinsicsProcrustesCfg("procrustes", num_points, False),
            )
            model = Model(cfg, num_frames=f, image_shape=tuple(hw))
            model.backbone.depth.data = depth.clone()
            model.backbone.weights.data = wlogit.clone()
            model = model.to(device)
            batch = Batch(torch.zeros((1, f, 3, *hw), device=device))
            flows = to_flows(oflows, device)
            tracks = to_tracks(otracks, device)
            losses = [LossFlow(LossFlowCfg(0, flow_weight, "flow", mapping_cfg(kind)))]
            if tracks is not None:
                losses.append(LossTracking(LossTrackingCfg(0, track_weight, "tracking", mapping_cfg(kind))))
            for _ in range(steps):
                model.zero_grad(set_to_none=True)
                out = model(batch, flows, 0)
                parts = [fn(batch, flows, tracks, out, 0) for fn in losses]
                total = sum(parts) * loss_scale if loss_scale != 1.0 else sum(parts)
                total.backward()
            return {
                "total": total.detach().cpu(),
                "loss_flow": parts[0].detach().cpu(),
                "loss_tracking": parts[1].detach().cpu() if tracks is not None else torch.zeros(()),
                "extrinsics": out.extrinsics.detach().cpu(),
                "g_depth": model.backbone.depth.grad.cpu(),
                "g_wlogit": model.backbone.weights.grad.cpu(),
                "g_focal": model.intrinsics.focal_length.grad.cpu(),
            }
        finally:
            flowmap_amd.set_lazy_surfaces(False)


def run_oracle(depth, wlogit, focal, oflows, hw, num_points, otracks=None, kind="huber", dtype=torch.float32,
               flow_weight=1000.0, track_weight=100.0):
    d = depth.to(dtype).clone().requires_grad_(True)
    w = wlogit.to(dtype).clone().requires_grad_(True)
    fo = torch.tensor(float(focal), dtype=dtype, requires_grad=True)
    fl = orc.OFlows(*(x.to(dtype) for x in (oflows.forward, oflows.backward, oflows.forward_mask, oflows.backward_mask)))
    tr = None if otracks is None else [orc.OTracks(t.xy.to(dtype), t.visibility, t.start_frame) for t in otracks]
    total, parts, out = orc.explicit_depth_step(d, w, fo, fl, tuple(hw), num_points=num_points, tracks=tr, kind=kind,
                                                flow_weight=flow_weight, track_weight=track_weight)
    out.intrinsics.retain_grad()
    total.backward()
    # dL/dfocal = sqrt(hw) * sum_f (dL/dK_f[0,0] / w + dL/dK_f[1,1] / h) (intrinsics/common.py:6-20): the magnitude of the
    # terms that sum runs over — on i.i.d. inputs they cancel to 1e-4 .. 1e-5 of themselves
    gk = out.intrinsics.grad[0]
    focal_terms = float((gk[:, 0, 0].abs() / hw[1] + gk[:, 1, 1].abs() / hw[0]).sum() * (hw[0] * hw[1]) ** 0.5)
    return {
        "g_focal_terms": focal_terms,
        "total": total.detach(),
        "loss_flow": parts["flow"].detach(),
        "loss_tracking": parts.get("tracking", torch.zeros(())).detach(),
        "extrinsics": out.extrinsics.detach(),
        "g_depth": d.grad,
        "g_wlogit": w.grad,
        "g_focal": fo.grad,
    }


FOCAL_ULPS = 8  # fp32 roundings (2^-24 each) of the cancelling dL/dK terms tolerated in dL/dfocal: worst measured 3.4 (host double, tests/golden/step_iid_flow) and 1.7 (GPU suite, profiles/r05_focal_gate_ratios_gpu.txt); 32 until round 5


def focal_close(got, truth, ref32=None, tol=1e-4, what="g_focal"):
    """dL/dfocal: ``tol`` of the fp64 truth; where the REFERENCE's own fp32 evaluation of the same step (``ref32``) is further than that from the
    truth, twice its measured gap; and — because dL/dfocal = sqrt(hw)·Σ_f (dL/dK_f[0,0]/w + dL/dK_f[1,1]/h) is a sum whose per-frame terms cancel
    to 1e-4 .. 1e-5 of themselves on i.i.d. inputs, so that ONE fp32 rounding of a term is already a 1e-3 relative error of the sum and the
    reference's own gap is a single draw of that noise — FOCAL_ULPS fp32 roundings (2^-24 each) of the terms' magnitude Σ|term| (from the fp64
    oracle).  FOCAL_ULPS is measured, not chosen: the worst ratio seen over the CPU and GPU suites is recorded by FLOWMAP_FOCAL_LOG."""
    g, t = float(got), float(truth["g_focal"])
    err = abs(g - t)
    bound = tol * abs(t)
    if ref32 is not None:
        bound = max(bound, 2.0 * abs(float(ref32["g_focal"]) - t))
    terms = truth.get("g_focal_terms")
    if terms:
        bound = max(bound, FOCAL_ULPS * 2.0**-24 * terms)
        log = os.environ.get("FLOWMAP_FOCAL_LOG")
        if log:
            with open(log, "a") as fh:
                fh.write(f"{err / (2.0**-24 * terms):.3f} {err / max(abs(t), 1e-300):.3e} {what}\n")
    assert err <= bound, (f"{what}: |{g:.6e} - {t:.6e}| = {err:.2e} > {bound:.2e}"
                          + ("" if ref32 is None else f" (fp32-reference gap {abs(float(ref32['g_focal']) - t):.2e})"))
    return err, bound


STEP_KEYS = ("total", "loss_flow", "loss_tracking", "extrinsics", "g_depth", "g_wlogit", "g_focal")


def compare_step(ours, truth, ref32=None, tol=1e-4, masks=None):
    """One optimisation step of ours against the truth (the fp64 oracle): every value and gradient at
    ``tol`` (1e-4, north_star's bar), dL/ddepth also element-wise and on its sparse parts (``masks``).
    ``ref32``: the REFERENCE's own fp32 results for the same inputs (golden vectors / the fp32 oracle).
    When given, dL/ddepth and dL/dweights may be as far from the truth as four times the reference's own
    measured gap (one draw of the same fp32 rounding noise) —
    on i.i.d. inputs the fp32 reference misses its fp64 self by up to 2e-4 on dL/ddepth and 1e-2 on
    the heavily cancelling dL/dfocal; consistent-scene fixtures pass ``ref32=None``
    and are held to ``tol`` outright."""
    for key in ("total", "loss_flow", "loss_tracking", "extrinsics"):
        assert_close(ours[key], truth[key], tol, what=key)
    # dL/dfocal: like every other gradient — 1e-4, or twice the reference's own measured fp32 gap where that is larger (focal_close)
    err, _ = focal_close(ours["g_focal"], truth, ref32, tol)
    if ref32 is None:
        assert_grad_close(ours["g_depth"], truth["g_depth"], tol, masks=masks or {}, what="g_depth")
        assert_close(ours["g_wlogit"], truth["g_wlogit"], tol, what="g_wlogit")
        assert err <= tol * abs(float(truth["g_focal"])), f"g_focal: rel err {err / abs(float(truth['g_focal'])):.2e} on a consistent scene"
        return
    assert_close_or_reference_gap(ours["g_depth"], truth["g_depth"], ref32["g_depth"], tol, what="g_depth")
    for name, mask in (masks or {}).items():
        assert_close_or_reference_gap(ours["g_depth"][mask], truth["g_depth"][mask], ref32["g_depth"][mask], tol, what=f"g_depth[{name}]")
    assert_close_or_reference_gap(ours["g_wlogit"], truth["g_wlogit"], ref32["g_wlogit"], tol, what="g_wlogit")


def step_masks(hw, num_points, oflows, otracks=None, frames=None):
    """The sparse parts of dL/ddepth: pixels the Procrustes fit / the tracking loss write to."""
    frames = oflows.backward.shape[1] + 1 if frames is None else frames
    masks = {}
    if num_points is not None:
        masks["procrustes"] = orc.procrustes_touched(hw, orc.procrustes_indices(hw, num_points), oflows.backward)
    if otracks:
        masks["tracks"] = orc.tracks_touched(hw, frames, otracks)
    return masks
