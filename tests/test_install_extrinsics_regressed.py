"""flowmap_amd.install() and the reference's `extrinsics: regressed` (flowmap/model/extrinsics/extrinsics_regressed.py), against the REAL
reference package (importable only where it is mounted; skipped elsewhere): the registry hands out this package's module, the reference's
own Model runs the configuration on lazy surfaces and reproduces the un-installed reference's step, host tensors reach the reference's own
forward, uninstall() restores, and the keyword leaves the reference's class alone."""

import os
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("FLOWMAP_REFERENCE", "/root/reference"))


def _reference_readable() -> bool:
    try:
        return (REF / "flowmap" / "model" / "extrinsics" / "extrinsics_regressed.py").is_file()
    except OSError:
        return False


pytestmark = pytest.mark.skipif(not _reference_readable(), reason="reference not mounted or not readable")


@pytest.fixture()
def reference_on_path():
    sys.dont_write_bytecode = True
    added = [str(ROOT / "oracle" / "refstubs"), str(REF)]
    sys.path[:0] = added
    import flowmap_amd
    from flowmap_amd import _lib

    flowmap_amd.uninstall()
    yield
    flowmap_amd.uninstall()
    _lib.set_library_for_testing(None)
    for p in added:
        sys.path.remove(p)


def _reference_step(g, with_tracks):
    """The reference's own Model (`extrinsics: regressed`) + get_losses on the fixture's inputs -> (model, output, results)."""
    from conftest import t

    import flowmap.loss as ref_loss
    from flowmap.dataset.types import Batch
    from flowmap.flow.flow_predictor import Flows
    from flowmap.loss.loss_flow import LossFlowCfg
    from flowmap.loss.loss_tracking import LossTrackingCfg
    from flowmap.loss.mapping.mapping_huber import MappingHuberCfg
    from flowmap.model.backbone.backbone_explicit_depth import BackboneExplicitDepthCfg
    from flowmap.model.extrinsics.extrinsics_regressed import ExtrinsicsRegressedCfg
    from flowmap.model.intrinsics.intrinsics_regressed import IntrinsicsRegressedCfg
    from flowmap.model.model import Model, ModelCfg
    from flowmap.tracking.track_predictor import Tracks

    depth = t(g["depth"])
    f, h, w = depth.shape
    cfg = ModelCfg(BackboneExplicitDepthCfg("explicit_depth", 1.0, 100.0), IntrinsicsRegressedCfg("regressed", float(g["focal"])),
                   ExtrinsicsRegressedCfg("regressed"), True)
    model = Model(cfg, num_frames=f, image_shape=(h, w))  # the reference's Model, unmodified
    model.backbone.depth.data = depth.clone()
    model.extrinsics.rotations.data = t(g["rotations"]).clone()
    model.extrinsics.translations.data = t(g["translations"]).clone()
    batch = Batch(torch.zeros((1, f, 3, h, w)), torch.arange(f)[None], ["s"], ["d"])
    flows = Flows(t(g["fwd"]), t(g["bwd"]), t(g["fwd_mask"]), t(g["bwd_mask"]))
    cfgs = [LossFlowCfg(0, 1000.0, "flow", MappingHuberCfg("huber", 0.01))]
    tracks = None
    if with_tracks:
        cfgs.append(LossTrackingCfg(0, 100.0, "tracking", MappingHuberCfg("huber", 0.01)))
        tracks = [Tracks(t(g[f"trk{i}_xy"]), t(g[f"trk{i}_vis"]), int(g[f"trk{i}_start"])) for i in range(int(g["n_segments"]))]
    out = model(batch, flows, 0)
    parts = [fn(batch, flows, tracks, out, 0) for fn in ref_loss.get_losses(cfgs)]
    total = sum(parts)
    total.backward()
    extrinsics = out.extrinsics.materialize() if hasattr(out.extrinsics, "materialize") else out.extrinsics
    results = {"total": total.detach(), "loss_flow": parts[0].detach(), "loss_tracking": parts[1].detach() if with_tracks else torch.zeros(()),
               "extrinsics": extrinsics.detach(), "g_depth": model.backbone.depth.grad, "g_focal": model.intrinsics.focal_length.grad,
               "g_rotations": model.extrinsics.rotations.grad, "g_translations": model.extrinsics.translations.grad}
    return model, out, results


def _golden(with_tracks):
    from conftest import load_golden, t

    import regressed_cases as rc

    g = load_golden("step_regressed_extrinsics")
    tag = "trk_" if with_tracks else ""
    keys = ("total", "loss_flow", "loss_tracking", "extrinsics", "g_focal") + rc.STEP_GRADS
    truth = {k: t(g[f"{tag}f64_{k}"]) for k in keys}
    truth["g_focal_terms"] = float(g[f"{tag}f64_g_focal_terms"])
    return g, truth, {k: t(g[f"{tag}{k}"]) for k in keys}


@pytest.mark.parametrize("with_tracks", [False, True])
def test_the_references_model_runs_the_configuration_on_lazy_surfaces(reference_on_path, with_tracks):
    import flowmap.model.extrinsics as ref_extr
    from flowmap.model.extrinsics.extrinsics import Extrinsics
    from flowmap.model.extrinsics.extrinsics_regressed import ExtrinsicsRegressedCfg

    import flowmap_amd
    import regressed_cases as rc
    from flowmap_amd import _lib, _ops
    from flowmap_amd.model.extrinsics_regressed import ExtrinsicsRegressed
    from flowmap_amd.model.projection import LazySurfaces
    from helpers import build_host_sim

    _lib.set_library_for_testing(build_host_sim())
    flowmap_amd.install()  # lazy_surfaces=True: the module reads only the shape of the surfaces
    assert ref_extr.EXTRINSICS["regressed"] is ExtrinsicsRegressed
    built = ref_extr.get_extrinsics(ExtrinsicsRegressedCfg("regressed"), 5)
    assert type(built) is ExtrinsicsRegressed and isinstance(built, Extrinsics)
    assert [n for n, _ in built.named_parameters()] == ["translations", "rotations"]
    g, truth, ref32 = _golden(with_tracks)
    before = dict(_ops.counters)
    model, out, ours = _reference_step(g, with_tracks)
    assert type(model.extrinsics) is ExtrinsicsRegressed
    assert isinstance(out.surfaces, LazySurfaces) and out.surfaces._dense is None
    assert _ops.counters["quat_pose_fwd"] - before["quat_pose_fwd"] == 1 and _ops.counters["quat_pose_bwd"] - before["quat_pose_bwd"] == 1
    rc.compare_step(ours, truth, ref32, what="installed ")


def test_host_tensors_reach_the_references_forward(reference_on_path):
    """The real library selected and tensors on the host: the reference's own forward runs on this module's parameters, so the step
    IS the reference's arithmetic and reproduces its fp32 numbers to rounding."""
    from conftest import assert_close

    import flowmap_amd
    from flowmap_amd import _lib, _reference
    from flowmap_amd.model.extrinsics_regressed import ExtrinsicsRegressed

    _lib.set_library_for_testing(None)
    flowmap_amd.install()
    assert _reference.twins["ExtrinsicsRegressed"].__module__ == "flowmap.model.extrinsics.extrinsics_regressed"
    g, _, ref32 = _golden(True)
    before = _reference.counters["host_calls"]
    model, out, ours = _reference_step(g, True)
    assert type(model.extrinsics) is ExtrinsicsRegressed and torch.is_tensor(out.extrinsics)
    assert _reference.counters["host_calls"] > before
    for key in ("total", "extrinsics"):
        assert_close(ours[key], ref32[key], 2e-6, what=key)
    for key in ("g_rotations", "g_translations", "g_depth"):
        assert_close(ours[key], ref32[key], 2e-5, what=key)


def test_uninstall_restores_and_the_keyword_leaves_the_references_class(reference_on_path):
    import flowmap.model.extrinsics as ref_extr

    import flowmap_amd
    from flowmap_amd import _reference
    from flowmap_amd.model.extrinsics_regressed import ExtrinsicsRegressed

    theirs = ref_extr.EXTRINSICS["regressed"]
    assert theirs.__module__ == "flowmap.model.extrinsics.extrinsics_regressed"
    flowmap_amd.install()
    assert ref_extr.EXTRINSICS["regressed"] is ExtrinsicsRegressed
    flowmap_amd.uninstall()
    assert ref_extr.EXTRINSICS["regressed"] is theirs and "ExtrinsicsRegressed" not in _reference.twins
    flowmap_amd.install(fused_extrinsics_regressed=False)
    assert ref_extr.EXTRINSICS["regressed"] is theirs and "ExtrinsicsRegressed" not in _reference.twins
    assert ref_extr.EXTRINSICS["procrustes"].__module__.startswith("flowmap_amd")


def test_state_dicts_go_both_ways_between_the_references_module_and_ours(reference_on_path):
    """A state_dict of the reference's own ExtrinsicsRegressed loads into this package's module with strict=True, and the reverse."""
    import flowmap.model.extrinsics as ref_extr
    from flowmap.model.extrinsics.extrinsics_regressed import ExtrinsicsRegressedCfg

    from flowmap_amd.model.extrinsics_regressed import ExtrinsicsRegressed

    theirs = ref_extr.EXTRINSICS["regressed"](ExtrinsicsRegressedCfg("regressed"), 6)
    assert type(theirs).__module__ == "flowmap.model.extrinsics.extrinsics_regressed"
    ours = ExtrinsicsRegressed(ExtrinsicsRegressedCfg("regressed"), 6)
    fresh_theirs, fresh_ours = theirs.state_dict(), ours.state_dict()
    assert list(fresh_theirs) == list(fresh_ours)
    for key in fresh_theirs:  # the same initial values
        assert torch.equal(fresh_theirs[key], fresh_ours[key]), key
    with torch.no_grad():
        theirs.rotations.add_(0.1 * torch.randn((5, 4), generator=torch.Generator().manual_seed(1)))
        theirs.translations.add_(0.1 * torch.randn((5, 3), generator=torch.Generator().manual_seed(2)))
    result = ours.load_state_dict(theirs.state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(ours.rotations, theirs.rotations) and torch.equal(ours.translations, theirs.translations)
    with torch.no_grad():
        ours.rotations.mul_(1.5)
    result = theirs.load_state_dict(ours.state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(ours.rotations, theirs.rotations)
