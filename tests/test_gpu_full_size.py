"""Parity at the sizes the headline numbers are quoted on: BASELINE.json configs[1] (150 frames @
720x1280, flow loss, Procrustes P = 1000) and configs[2] (+ tracking: 30 segments x 1225 tracks, the
layout of flowmap/tracking/__init__.py:49-70), HIP path vs the oracle run ONCE on the GPU box's host
cores (about a minute: one forward, one backward per loss).  The scene is the consistent one of SURVEY.md §8d (generated
on the GPU by the oracle's own functions, seconds instead of minutes), so every gradient —
dL/dfocal included — is well conditioned and held to 1e-4; dL/ddepth is also compared element-wise
and on the pixels the Procrustes fit / the tracks write to.

Round 3: BASELINE.json configs[3] at its own size (65 frames @ 1080x1920, consistent scene, flow loss)
and ONE GPU's shard of configs[4] (150 frames @ 1080x1920, i.i.d. depth / flow / masks, flow loss) against the oracle.  On
i.i.d. inputs the fp32 reference itself is further than 1e-4 from the fp64 truth in the Procrustes-conditioned gradients, so
that test runs the oracle twice (fp64 = truth, fp32 = the reference's own arithmetic), records both gaps and holds ours to
max(1e-4, 2 x the reference's gap).

FLOWMAP_SKIP_FULL_SIZE=1 skips the module (iteration runs); the oracle runs in fp64 when the host has
the memory for it (>= 256 GB free), else in fp32 — the reference's own precision — and says which: every comparison emits
its record (oracle dtype, achieved errors) as a UserWarning, so that it shows in pytest's warnings summary — the driver's
log — and appends it to $FLOWMAP_PARITY_RECORD when that is set."""

import json
import os
import warnings

import pytest
import torch

from conftest import assert_close, assert_grad_close, maxerr, relerr
from helpers import mapping_cfg, run_ours, step_masks
from oracle import flowmap_oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("FLOWMAP_SKIP_FULL_SIZE") == "1", reason="FLOWMAP_SKIP_FULL_SIZE=1")]
DEV = "cuda:0"
F, H, W, P = 150, 720, 1280, 1000
FOCAL = 0.8  # not the scene's 0.85: dL/dfocal is then a first-order quantity


def _host_memory_gb():
    try:
        import psutil

        return psutil.virtual_memory().available / 2**30
    except Exception:
        return 0.0


def build_reference(f, h, w, p, dev, dtype, **track_layout):
    """(scene, weight logits, tracks, oracle results): one oracle forward, one backward per loss."""
    sc = orc.synth_scene(f, h, w, seed=1, device=dev)
    tracks = orc.synth_tracks(f, h, w, scene=sc, seed=1, **track_layout)  # default: every 5th frame, +-20 frames, 35 x 35 queries
    wl = 0.01 * torch.randn((f - 1, h, w), generator=torch.Generator().manual_seed(7))
    d = sc["depth_init"].to(dtype).requires_grad_(True)
    wp = wl.to(dtype).requires_grad_(True)
    fo = torch.tensor(FOCAL, dtype=dtype, requires_grad=True)
    fl = orc.OFlows(*(x.to(dtype) for x in (sc["flows"].forward, sc["flows"].backward, sc["flows"].forward_mask, sc["flows"].backward_mask)))
    tr = [orc.OTracks(t.xy.to(dtype), t.visibility, t.start_frame) for t in tracks]
    total, parts, out = orc.explicit_depth_step(d, wp, fo, fl, (h, w), num_points=p, tracks=tr)
    ref = {"dtype": dtype, "extrinsics": out.extrinsics.detach(), "loss_flow": parts["flow"].detach(), "loss_tracking": parts["tracking"].detach()}
    for name, last in (("flow", False), ("tracking", True)):
        g = torch.autograd.grad(parts[name], (d, wp, fo), retain_graph=not last)
        ref[name] = {"g_depth": g[0], "g_wlogit": g[1], "g_focal": g[2]}
    return sc, wl, tracks, ref


@pytest.fixture(scope="module")
def full_size():
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    dtype = torch.float64 if _host_memory_gb() >= 256 else torch.float32
    sc, wl, tracks, ref = build_reference(F, H, W, P, DEV, dtype)
    assert len(tracks) == 30 and tracks[0].xy.shape[2] == 1225
    return sc, wl, tracks, ref


def emit(record):
    print(record)
    warnings.warn("full-size parity record: " + json.dumps(record))  # (pytest's warnings summary: the driver's log keeps it)
    out = os.environ.get("FLOWMAP_PARITY_RECORD")  # tools/gpu_call.sh points this under gpurun_out/
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(record) + "\n")


def check(ours, ref, grads, masks, what):
    tol = 1e-4
    record = {"case": what, "oracle_dtype": str(ref["dtype"]), "extrinsics": relerr(ours["extrinsics"], ref["extrinsics"])}
    for key in ("g_depth", "g_wlogit", "g_focal"):
        record[key] = relerr(ours[key], grads[key])
        record[key + "_max_abs_over_max_ref"] = maxerr(ours[key], grads[key])
    for name, mask in masks.items():
        record[f"g_depth[{name}]"] = relerr(ours["g_depth"][mask], grads["g_depth"][mask])
    emit(record)
    assert_close(ours["extrinsics"], ref["extrinsics"], tol, what="extrinsics")
    assert_grad_close(ours["g_depth"], grads["g_depth"], tol, masks=masks, what="g_depth")
    assert_grad_close(ours["g_wlogit"], grads["g_wlogit"], tol, what="g_wlogit")
    assert_close(ours["g_focal"], grads["g_focal"], tol, what="g_focal")


def compare_flow_only(built, hw, p, dev):
    sc, wl, _, ref = built
    ours = run_ours(sc["depth_init"], wl, FOCAL, sc["flows"], hw, p, device=dev)
    assert_close(ours["loss_flow"], ref["loss_flow"], 1e-4, what="loss_flow")
    check(ours, ref, ref["flow"], step_masks(hw, p, sc["flows"]), "C1")


def compare_flow_and_tracking(built, hw, p, dev, steps=1, label="C2"):
    sc, wl, tracks, ref = built
    ours = run_ours(sc["depth_init"], wl, FOCAL, sc["flows"], hw, p, tracks, device=dev, steps=steps)
    assert_close(ours["loss_flow"], ref["loss_flow"], 1e-4, what="loss_flow")
    assert_close(ours["loss_tracking"], ref["loss_tracking"], 1e-4, what="loss_tracking")
    both = {k: ref["flow"][k] + ref["tracking"][k] for k in ("g_depth", "g_wlogit", "g_focal")}
    check(ours, ref, both, step_masks(hw, p, sc["flows"], tracks, frames=sc["depth_init"].shape[0]), label)


def test_c1_flow_loss_150x720x1280_vs_oracle(full_size):
    compare_flow_only(full_size, (H, W), P, DEV)


def test_c2_flow_and_tracking_150x720x1280_vs_oracle(full_size):
    compare_flow_and_tracking(full_size, (H, W), P, DEV)


def test_c2_tap_exchange_150x720x1280_vs_oracle(full_size):
    """The third step of a flow + tracking loop: the tracking loss evaluated ahead of the flow pass from the compact tap image, its depth
    gradient absorbed by that pass (fm_flow_loss_fused_taps / fm_track_loss_fused_fwd_taps) — against the same fp64 oracle step."""
    from flowmap_amd import _ops

    before = dict(_ops.counters)
    compare_flow_and_tracking(full_size, (H, W), P, DEV, steps=3, label="C2-tap-exchange")
    assert _ops.counters["flow_tap_absorbs"] - before["flow_tap_absorbs"] == 2 and _ops.counters["track_tap_samples"] - before["track_tap_samples"] == 1


def test_c1_installed_standin_150x720x1280_vs_oracle(full_size, standin):
    """configs[1] at its own size THROUGH install(): the stand-in package's Model — every part from the registries install()
    rebound, the lazy-weight backbone included — and its get_losses, on cuda:0, against the same oracle step as test_c1_..."""
    import flowmap.loss as pkg_loss
    from flowmap.dataset.types import Batch
    from flowmap.flow.flow_predictor import Flows
    from flowmap.loss.loss_flow import LossFlowCfg
    from flowmap.loss.mapping import MappingHuberCfg
    from flowmap.model.backbone import BackboneExplicitDepthCfg
    from flowmap.model.extrinsics.extrinsics_procrustes import ExtrinsicsProcrustesCfg
    from flowmap.model.intrinsics import IntrinsicsRegressedCfg
    from flowmap.model.model import Model, ModelCfg

    import flowmap_amd
    from flowmap_amd.model.projection import LazySurfaces, LazyWeights

    sc, wl, _, ref = full_size
    flowmap_amd.install()
    try:
        model = Model(ModelCfg(BackboneExplicitDepthCfg("explicit_depth", 1.0, 100.0), IntrinsicsRegressedCfg("regressed", FOCAL),
                               ExtrinsicsProcrustesCfg("procrustes", P, False), True), num_frames=F, image_shape=(H, W))
        assert type(model.backbone).__module__ == "flowmap_amd.model.backbone"
        model.backbone.depth.data = sc["depth_init"].clone()
        model.backbone.weights.data = wl.clone()
        model = model.to(DEV)
        batch = Batch(torch.zeros((1, F, 3, 1, 1), device=DEV).expand(1, F, 3, H, W))
        fl = sc["flows"]
        flows = Flows(fl.forward.to(DEV), fl.backward.to(DEV), fl.forward_mask.to(DEV), fl.backward_mask.to(DEV))
        losses = pkg_loss.get_losses([LossFlowCfg(0, 1000.0, "flow", MappingHuberCfg("huber", 0.01))])
        for _ in range(2):  # (the second step runs the packed kernel: what bench.py times)
            model.zero_grad(set_to_none=True)
            out = model(batch, flows, 0)
            loss = losses[0](batch, flows, None, out, 0)
            loss.backward()
        assert isinstance(out.surfaces, LazySurfaces) and isinstance(out.backward_correspondence_weights, LazyWeights)
        ours = {"loss_flow": loss.detach().cpu(), "extrinsics": out.extrinsics.detach().cpu(), "g_depth": model.backbone.depth.grad.cpu(),
                "g_wlogit": model.backbone.weights.grad.cpu(), "g_focal": model.intrinsics.focal_length.grad.cpu()}
    finally:
        flowmap_amd.uninstall()
    assert_close(ours["loss_flow"], ref["loss_flow"], 1e-4, what="loss_flow")
    check(ours, ref, ref["flow"], step_masks((H, W), P, sc["flows"]), "C1-installed-standin")


# ---- BASELINE.json configs[3], configs[4] at their own frame size (row J1) ----


def _oracle_dtype():
    return torch.float64 if _host_memory_gb() >= 256 else torch.float32


def c3_case(f, h, w, points, dev, dtype, label):
    sc = orc.synth_scene(f, h, w, seed=3, device=dev)
    wl = 0.01 * torch.randn((f - 1, h, w), generator=torch.Generator().manual_seed(8))
    d = sc["depth_init"].to(dtype).requires_grad_(True)
    wp = wl.to(dtype).requires_grad_(True)
    fo = torch.tensor(FOCAL, dtype=dtype, requires_grad=True)
    fl = orc.OFlows(*(x.to(dtype) for x in (sc["flows"].forward, sc["flows"].backward, sc["flows"].forward_mask, sc["flows"].backward_mask)))
    total, parts, out = orc.explicit_depth_step(d, wp, fo, fl, (h, w), num_points=points)
    g = torch.autograd.grad(parts["flow"], (d, wp, fo))
    ref = {"dtype": dtype, "extrinsics": out.extrinsics.detach(), "loss_flow": parts["flow"].detach()}
    grads = {"g_depth": g[0], "g_wlogit": g[1], "g_focal": g[2]}
    del total, parts, out, d, wp, fl
    ours = run_ours(sc["depth_init"], wl, FOCAL, sc["flows"], (h, w), points, device=dev)
    assert_close(ours["loss_flow"], ref["loss_flow"], 1e-4, what="loss_flow")
    check(ours, ref, grads, step_masks((h, w), points, sc["flows"]), label)


def test_c3_flow_loss_65x1080x1920_vs_oracle():
    """configs[3]: 65 frames @ 1080x1920 (the video BASELINE.json shards over 4 GPUs), consistent scene, flow loss, P = 1000."""
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    c3_case(65, 1080, 1920, P, DEV, _oracle_dtype(), "C3 (65 x 1080x1920, scene, flow)")


def c4_shard_case(f, h, w, points, dev, dtype, label):
    from helpers import focal_close, run_oracle

    depth, wlogit, flows = orc.synth_iid(f, h, w, seed=4)
    ours = run_ours(depth, wlogit, 0.85, flows, (h, w), points, device=dev)
    truth = run_oracle(depth, wlogit, 0.85, flows, (h, w), points, dtype=dtype)
    ref32 = run_oracle(depth, wlogit, 0.85, flows, (h, w), points, dtype=torch.float32) if dtype == torch.float64 else None
    masks = step_masks((h, w), points, flows)
    record = {"case": label, "oracle_dtype": str(dtype)}
    for key in ("loss_flow", "extrinsics", "g_depth", "g_wlogit"):
        record[key] = relerr(ours[key], truth[key])
        if ref32 is not None:
            record[key + "_fp32_reference_gap"] = relerr(ref32[key], truth[key])
    for name, mask in masks.items():
        record[f"g_depth[{name}]"] = relerr(ours["g_depth"][mask], truth["g_depth"][mask])
        if ref32 is not None:
            record[f"g_depth[{name}]_fp32_reference_gap"] = relerr(ref32["g_depth"][mask], truth["g_depth"][mask])
    err_focal = abs(float(ours["g_focal"]) - float(truth["g_focal"]))
    record.update({"g_focal_abs_err": err_focal, "g_focal": float(truth["g_focal"]), "g_focal_sum_of_abs_terms": truth["g_focal_terms"],
                   "g_focal_fp32_reference_abs_gap": None if ref32 is None else abs(float(ref32["g_focal"]) - float(truth["g_focal"]))})
    emit(record)
    slack = 2.0
    for key in ("loss_flow", "extrinsics"):
        assert record[key] <= 1e-4, (key, record)
    for key in ["g_depth", "g_wlogit"] + [f"g_depth[{name}]" for name in masks]:
        gap = record.get(key + "_fp32_reference_gap", 0.0)
        assert record[key] <= max(1e-4, slack * gap), (key, record[key], gap)
    focal_close(ours["g_focal"], truth, ref32)  # (1e-4, twice the fp32 reference's own gap, or FOCAL_ULPS roundings of the cancelling terms)
    return record


def test_c4_shard_flow_loss_150x1080x1920_iid_vs_oracle():
    """One GPU's shard of configs[4]: 150 frames @ 1080x1920 of i.i.d. inputs (depth U(1.10,1.15), flows
    N(0,0.01²), masks U(0,1), weight logits N(0,0.01²)), flow loss, P = 1000.  Truth = the fp64 oracle; the fp32 oracle =
    what the reference's own arithmetic delivers on these inputs.  Both gaps are recorded."""
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    c4_shard_case(150, 1080, 1920, P, DEV, _oracle_dtype(), "C4 shard (150 x 1080x1920, i.i.d., flow)")


# ---- BASELINE.json configs[4] WHOLE on one GPU: 1200 frames @ 1080x1920, 2.5e9 pixels ----


def _device_relerr(a, b, chunk=1 << 28):
    """conftest.relerr for tensors of 10 GB: ||a - b|| / ||b|| accumulated in fp64 ON the device, a chunk at a time."""
    a, b = a.reshape(-1), b.reshape(-1)
    num = den = 0.0
    for i in range(0, a.numel(), chunk):
        x, y = a[i : i + chunk].double(), b[i : i + chunk].double()
        num += float(((x - y) ** 2).sum())
        den += float((y**2).sum())
    return (num / den) ** 0.5 if den > 1e-60 else num**0.5


def _gpu_step(depth, wlogit, flows, hw, points, focal=0.85):
    """One step of the product path (Model + LossFlow, as helpers.run_ours drives it) on tensors that ALREADY live on the GPU and
    are used in place (frame windows of the whole video included): loss (python float), V = Σmask (python float, fp64 sum) and the
    gradients, left on the GPU."""
    import flowmap_amd
    from flowmap_amd import Batch
    from flowmap_amd.loss import LossFlow, LossFlowCfg
    from flowmap_amd.model.extrinsics_procrustes import ExtrinsicsProcrustesCfg
    from flowmap_amd.model.model import BackboneExplicitDepthCfg, IntrinsicsRegressedCfg, Model, ModelCfg

    f = depth.shape[0]
    flowmap_amd.set_lazy_surfaces(True)
    try:
        cfg = ModelCfg(BackboneExplicitDepthCfg("explicit_depth", 1.0, 100.0), IntrinsicsRegressedCfg("regressed", float(focal)),
                       ExtrinsicsProcrustesCfg("procrustes", points, False))
        with torch.device("meta"):
            model = Model(cfg, num_frames=2, image_shape=(2, 2))  # (no 10 GB host allocation for parameters that are replaced below)
        model = model.to_empty(device=depth.device)
        model.intrinsics.focal_length.data = torch.tensor(float(focal), device=depth.device)
        model.backbone.depth = torch.nn.Parameter(depth)
        model.backbone.weights = torch.nn.Parameter(wlogit)
        model.extrinsics = type(model.extrinsics)(cfg.extrinsics, f)
        batch = Batch(torch.zeros((1, f, 3, 1, 1), device=depth.device).expand(1, f, 3, *hw))
        loss_fn = LossFlow(LossFlowCfg(0, 1000.0, "flow", mapping_cfg("huber")))
        out = model(batch, flows, 0)
        loss = loss_fn(batch, flows, None, out, 0)
        loss.backward()
        valid = float(flows.forward_mask.sum(dtype=torch.float64) + flows.backward_mask.sum(dtype=torch.float64))
        return {"loss": float(loss.detach().double()), "valid": valid, "extrinsics": out.extrinsics.detach(),
                "g_depth": model.backbone.depth.grad, "g_wlogit": model.backbone.weights.grad,
                "g_focal": float(model.intrinsics.focal_length.grad.double())}
    finally:
        flowmap_amd.set_lazy_surfaces(False)


def test_c4_whole_1200x1080x1920_on_one_gpu():
    """BASELINE.json configs[4] WHOLE on one MI355X: 1200 frames @ 1080x1920 of i.i.d. inputs = 2.49e9 pixels, 79.6 GB of inputs + a
    59.7 GB packed copy + 10 GB gradients of the 288 GB.  Element offsets pass 2^31 at frame 1036 (2^32 bytes at frame 518, 2^32 elements
    of the packed buffer at frame 350), grid.y = 1200, the pose chain has 1199 links.  Too big for the oracle whole, so:
      * run-to-run agreement of the whole video (packed kernel);
      * additivity over the eight 150-frame shards configs[4] assigns to eight GPUs (each the size test_c4_shard_... holds against the
        fp64 oracle): Σ loss_s·V_s = loss·V, interior frames' dL/ddepth equal, halo frames' sum, Σ dL/dfocal_s·V_s = dL/dfocal·V;
      * a four-frame window BEYOND element 2^31 (frames 1100..1103) against the fp64 oracle: dL/ddepth and dL/dweights of its interior
        frames / pair depend on nothing outside the window (the relative pose of a pair is a function of its two frames)."""
    from flowmap_amd import Flows, config
    from flowmap_amd.sharding import shard_frames, shard_pairs
    from helpers import run_oracle

    if torch.cuda.get_device_properties(0).total_memory < 250 * 2**30:
        pytest.skip("needs a 288 GB GPU")
    f, h, w, p = 1200, 1080, 1920, 1000
    g = torch.Generator(device=DEV).manual_seed(4)
    depth = 1.10 + 0.05 * torch.rand((f, h, w), device=DEV, generator=g)
    wlogit = 0.01 * torch.randn((f - 1, h, w), device=DEV, generator=g)
    flows = Flows(0.01 * torch.randn((1, f - 1, h, w, 2), device=DEV, generator=g), 0.01 * torch.randn((1, f - 1, h, w, 2), device=DEV, generator=g),
                  torch.rand((1, f - 1, h, w), device=DEV, generator=g), torch.rand((1, f - 1, h, w), device=DEV, generator=g))
    assert depth.numel() > 2**31 and flows.forward.numel() > 2**32

    with config.override(pack_on_first_sight=True):
        whole = _gpu_step(depth, wlogit, flows, (h, w), p)
        assert flows.forward.__dict__.get("_fm_packed") is not None, "the whole-video step did not run the packed kernel"
        assert flows.forward.__dict__["_fm_packed"][1][1].numel() > 2**32
        again = _gpu_step(depth, wlogit, flows, (h, w), p)
        assert whole["loss"] == whole["loss"] and bool(torch.isfinite(whole["g_depth"]).all())
        record = {"case": "C4 whole (1200 x 1080x1920, i.i.d., flow, one GPU)", "loss": whole["loss"], "valid": whole["valid"],
                  "run_to_run_loss": abs(again["loss"] - whole["loss"]) / abs(whole["loss"]),
                  "run_to_run_g_depth": _device_relerr(again["g_depth"], whole["g_depth"]), "run_to_run_g_wlogit": _device_relerr(again["g_wlogit"], whole["g_wlogit"])}
        assert record["run_to_run_loss"] <= 1e-6 and record["run_to_run_g_depth"] <= 1e-5 and record["run_to_run_g_wlogit"] <= 1e-5, record
        del again
        torch.cuda.empty_cache()

        # -- the eight shards of configs[4] --
        num, focal_sum, worst = 0.0, 0.0, {"interior": 0.0, "halo": 0.0, "wlogit": 0.0}
        halo_carry = None
        for a, b in shard_pairs(f - 1, 8):
            lo, hi = shard_frames((a, b))
            part = Flows(*(x[:, a:b] for x in (flows.forward, flows.backward, flows.forward_mask, flows.backward_mask)))
            sh = _gpu_step(depth[lo : hi + 1], wlogit[a:b], part, (h, w), p)
            scale = sh["valid"] / whole["valid"]  # the shard normalises by its own Σmask
            num += sh["loss"] * scale
            focal_sum += sh["g_focal"] * scale
            gd = sh["g_depth"] * scale
            worst["interior"] = max(worst["interior"], _device_relerr(gd[1:-1], whole["g_depth"][lo + 1 : hi]))
            worst["wlogit"] = max(worst["wlogit"], _device_relerr(sh["g_wlogit"] * scale, whole["g_wlogit"][a:b]))
            first = gd[0] if halo_carry is None else gd[0] + halo_carry
            worst["halo"] = max(worst["halo"], _device_relerr(first, whole["g_depth"][lo]))
            halo_carry = gd[-1].clone()
            del sh, gd, part
            torch.cuda.empty_cache()
        worst["halo"] = max(worst["halo"], _device_relerr(halo_carry, whole["g_depth"][f - 1]))
        record.update({"shard_additivity_loss": abs(num - whole["loss"]) / abs(whole["loss"]),
                       "shard_additivity_g_focal_abs": abs(focal_sum - whole["g_focal"]), "g_focal": whole["g_focal"],
                       "shard_g_depth_interior": worst["interior"], "shard_g_depth_halo": worst["halo"], "shard_g_wlogit": worst["wlogit"]})

        # -- a window beyond element 2^31 against the oracle --
        lo, hi = 1100, 1103
        assert lo * h * w > 2**31
        win = orc.OFlows(*(x[:, lo:hi].cpu() for x in (flows.forward, flows.backward, flows.forward_mask, flows.backward_mask)))
        d_win, w_win = depth[lo : hi + 1].cpu(), wlogit[lo:hi].cpu()
        truth = run_oracle(d_win, w_win, 0.85, win, (h, w), p, dtype=torch.float64)
        ref32 = run_oracle(d_win, w_win, 0.85, win, (h, w), p, dtype=torch.float32)
        v_win = float(win.forward_mask.sum(dtype=torch.float64) + win.backward_mask.sum(dtype=torch.float64))
        scale = whole["valid"] / v_win  # the whole video normalises by ITS Σmask
        ours_d = (whole["g_depth"][lo + 1 : hi] * scale).cpu()
        ours_w = (whole["g_wlogit"][lo + 1 : hi - 1] * scale).cpu()  # the pair between the two interior frames
        touched = step_masks((h, w), p, win)["procrustes"][1:-1]
        for key, ours, tr, r32 in (("g_depth", ours_d, truth["g_depth"][1:-1], ref32["g_depth"][1:-1]),
                                    ("g_depth[procrustes]", ours_d[touched], truth["g_depth"][1:-1][touched], ref32["g_depth"][1:-1][touched]),
                                    ("g_wlogit", ours_w, truth["g_wlogit"][1:-1], ref32["g_wlogit"][1:-1])):
            record["window_" + key] = relerr(ours, tr)
            record["window_" + key + "_fp32_reference_gap"] = relerr(r32, tr)
        emit(record)
        assert record["shard_additivity_loss"] <= 1e-5, record
        assert record["shard_g_depth_interior"] <= 1e-4 and record["shard_g_depth_halo"] <= 1e-4 and record["shard_g_wlogit"] <= 1e-4, record
        for key in ("g_depth", "g_depth[procrustes]", "g_wlogit"):
            assert record["window_" + key] <= max(1e-4, 2.0 * record["window_" + key + "_fp32_reference_gap"]), (key, record)
