"""The regressed extrinsics (flowmap_amd/model/extrinsics_regressed.py, _ops.QuaternionPoses, csrc/fm_pose.h: quat_pose_fwd_one /
quat_pose_bwd_one) on the host double of the C ABI: function level against the reference's golden vectors and finite differences, the
whole step against the reference's fp64 run and the oracle, and the structure of the step (launch counts, what stays unevaluated).

Worst err / bound ratios measured on the host double are quoted in DESIGN.md (the subsection on regressed extrinsics)."""

import pytest
import torch

import flowmap_amd
import regressed_cases as rc
from conftest import assert_close, load_golden, t
from flowmap_amd import Batch, FusedAdam, _lib, _ops
from flowmap_amd.model.extrinsics_regressed import ExtrinsicsRegressed, ExtrinsicsRegressedCfg
from flowmap_amd.model.projection import LazyExtrinsics, LazySurfaces
from helpers import build_host_sim, to_flows, to_tracks


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


def test_function_level_vs_reference_golden():
    rc.case_function_golden("cpu")


def test_gradients_vs_finite_differences():
    rc.case_finite_differences("cpu")


def test_identity_initialisation():
    rc.case_identity("cpu")


def test_arguments_are_checked():
    q, tr = torch.zeros((3, 4)), torch.zeros((2, 3))
    with pytest.raises(RuntimeError, match="rotations"):
        _ops.QuaternionPoses.apply(q, tr, True)
    with pytest.raises(RuntimeError, match="float32"):
        _ops.QuaternionPoses.apply(q.double(), torch.zeros((3, 3)), True)


@pytest.mark.parametrize("with_tracks", [False, True])
def test_step_vs_reference_golden(with_tracks, record_property):
    ratios = {}
    rc.case_step_golden("cpu", with_tracks, ratios)
    print("err / bound:", {k: round(v, 4) for k, v in ratios.items()})
    record_property("ratios", ratios)


@pytest.mark.parametrize("f,h,w,seed", [(6, 24, 32, 2), (5, 17, 23, 2)])
def test_step_vs_oracle_fp64(f, h, w, seed, record_property):
    ratios = {}
    rc.case_step_oracle("cpu", f, h, w, seed, True, ratios)
    print("err / bound:", {k: round(v, 4) for k, v in ratios.items()})
    record_property("ratios", ratios)


def _problem(device="cpu"):
    g = load_golden("step_regressed_extrinsics")
    depth = t(g["depth"])
    f, h, w = depth.shape
    model = rc.build_model(depth, float(g["focal"]), t(g["rotations"]), t(g["translations"]), device)
    batch = Batch(torch.zeros((1, f, 3, h, w), device=device))
    return g, model, batch, to_flows(rc.golden_flows(g), device), to_tracks(rc.golden_tracks(g), device)


def test_a_flow_only_step_is_one_launch_each_way(monkeypatch):
    """quat_pose_fwd and quat_pose_bwd move by exactly one; the chain and the relative poses are never derived: the fused flow loss reads
    the poses the module attached, and the surfaces stay a LazySurfaces nobody evaluated."""
    g, model, batch, flows, _ = _problem()
    called = []
    monkeypatch.setattr(_ops.RelativePoses, "apply", staticmethod(lambda *a: called.append("RelativePoses")))
    monkeypatch.setattr(_ops.PoseChain, "apply", staticmethod(lambda *a: called.append("PoseChain")))
    flowmap_amd.set_lazy_surfaces(True)
    try:
        before = dict(_ops.counters)
        out = model(batch, flows, 0)
        assert isinstance(out.extrinsics, LazyExtrinsics) and out.extrinsics._dense is None
        assert isinstance(out.surfaces, LazySurfaces)
        loss = rc.make_losses(False)[0](batch, flows, None, out, 0)
        assert _ops.counters["quat_pose_fwd"] - before["quat_pose_fwd"] == 1 and _ops.counters["quat_pose_bwd"] == before["quat_pose_bwd"]
        loss.backward()
        assert _ops.counters["quat_pose_fwd"] - before["quat_pose_fwd"] == 1 and _ops.counters["quat_pose_bwd"] - before["quat_pose_bwd"] == 1
        assert called == []
        assert out.extrinsics._dense is None and out.surfaces._dense is None
        rel_inv, rel = out.extrinsics._fm_relative_poses
        assert tuple(rel.shape) == tuple(rel_inv.shape) == (1, depth_frames(model) - 1, 4, 4)
        assert model.extrinsics.rotations.grad is not None and model.extrinsics.translations.grad is not None
    finally:
        flowmap_amd.set_lazy_surfaces(False)


def depth_frames(model):
    return model.backbone.depth.shape[0]


def test_reading_the_extrinsics_evaluates_the_chain_and_the_next_step_chains_in_the_forward_launch():
    g, model, batch, flows, _ = _problem()
    flowmap_amd.set_lazy_surfaces(True)
    try:
        out = model(batch, flows, 0)
        assert isinstance(out.extrinsics, LazyExtrinsics)
        positions = out.extrinsics[0, :, :3, 3]  # (what a trajectory logger reads)
        assert out.extrinsics._dense is not None and flows.backward.__dict__["_fm_extrinsics_wanted"] is True
        assert_close(positions, t(g["extrinsics"])[0, :, :3, 3], 1e-4, what="camera positions")
        before = dict(_ops.counters)
        again = model(batch, flows, 0)
        assert torch.is_tensor(again.extrinsics) and not isinstance(again.extrinsics, LazyExtrinsics)
        assert _ops.counters["quat_pose_fwd"] - before["quat_pose_fwd"] == 1
        assert_close(again.extrinsics, t(g["extrinsics"]), 1e-4, what="extrinsics from the forward launch")
        rel_inv, rel = again.extrinsics._fm_relative_poses
        assert_close(rel[0], t(load_golden("fn_extrinsics_regressed")["tf"]), 1e-4, what="attached poses")
        assert again.surfaces._dense is None
    finally:
        flowmap_amd.set_lazy_surfaces(False)


def test_no_grad_returns_the_tensor():
    _, model, batch, flows, _ = _problem()
    flowmap_amd.set_lazy_surfaces(True)
    try:
        with torch.no_grad():
            out = model(batch, flows, 0)
        assert torch.is_tensor(out.extrinsics) and tuple(out.extrinsics.shape) == (1, depth_frames(model), 4, 4)
    finally:
        flowmap_amd.set_lazy_surfaces(False)


def test_batch_of_two_is_refused():
    module = ExtrinsicsRegressed(ExtrinsicsRegressedCfg("regressed"), 3)
    with pytest.raises(AssertionError):
        module(None, None, None, torch.zeros((2, 3, 4, 5, 3)))


def test_parameters_equal_the_references():
    """Names, shapes, dtypes and initial values of flowmap/model/extrinsics/extrinsics_regressed.py:57-63; fewer than two frames refused."""
    module = ExtrinsicsRegressed(ExtrinsicsRegressedCfg("regressed"), 7)
    named = dict(module.named_parameters())
    assert list(named) == ["translations", "rotations"]
    assert tuple(named["translations"].shape) == (6, 3) and tuple(named["rotations"].shape) == (6, 4)
    assert all(p.dtype == torch.float32 for p in named.values())
    assert torch.equal(named["translations"].detach(), torch.zeros((6, 3)))
    assert torch.equal(named["rotations"].detach(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(6, 4))
    with pytest.raises(AssertionError):
        ExtrinsicsRegressed(ExtrinsicsRegressedCfg("regressed"), 1)


def test_a_reference_state_dict_loads_strictly():
    """The keys and shapes the reference's module saves (its two nn.Parameters, extrinsics_regressed.py:58-63), restated here; a state_dict
    of the reference's own module is loaded, both ways, in tests/test_install_extrinsics_regressed.py, where the reference is importable."""
    g = load_golden("fn_extrinsics_regressed")
    state = {"translations": t(g["translations"]), "rotations": t(g["rotations"])}
    module = ExtrinsicsRegressed(ExtrinsicsRegressedCfg("regressed"), state["rotations"].shape[0] + 1)
    assert set(module.state_dict()) == set(state)
    result = module.load_state_dict(state, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(module.rotations.detach(), state["rotations"])


def test_fused_adam_steps_the_new_parameters_like_torch_adam():
    """Five steps of FusedAdam over ALL parameters of the model against torch.optim.Adam fed the same gradients, at the tolerance of
    tests/cases.py: case_fused_adam (2e-6 relative, 1e-7 absolute)."""
    _, model, batch, flows, tracks = _problem()
    twins = {name: p.detach().clone().requires_grad_(True) for name, p in model.named_parameters()}
    ours, theirs = FusedAdam(model.parameters(), lr=3e-3), torch.optim.Adam(twins.values(), lr=3e-3)
    losses = rc.make_losses(True)
    flowmap_amd.set_lazy_surfaces(True)
    try:
        history = []
        for _ in range(5):
            ours.zero_grad(set_to_none=True)
            out = model(batch, flows, 0)
            total = sum(fn(batch, flows, tracks, out, 0) for fn in losses)
            total.backward()
            history.append(float(total))
            for name, p in model.named_parameters():
                twins[name].grad = None if p.grad is None else p.grad.detach().clone()
            ours.step()
            theirs.step()
    finally:
        flowmap_amd.set_lazy_surfaces(False)
    assert history[-1] < history[0]
    moved = {name for name, p in model.named_parameters() if p.grad is not None}
    assert {"extrinsics.rotations", "extrinsics.translations", "backbone.depth", "intrinsics.focal_length"} <= moved
    for name, p in model.named_parameters():
        assert_close(p.detach(), twins[name].detach(), 2e-6, abs_=1e-7, what=name)


def test_model_cfg_selects_the_module_and_the_default_is_unchanged():
    from flowmap_amd.model.extrinsics_procrustes import ExtrinsicsProcrustes, ExtrinsicsProcrustesCfg
    from flowmap_amd.model.model import BackboneExplicitDepthCfg, IntrinsicsRegressedCfg, Model, ModelCfg

    backbone, intrinsics = BackboneExplicitDepthCfg("explicit_depth", 1.0, 100.0), IntrinsicsRegressedCfg("regressed", 0.85)
    assert isinstance(Model(ModelCfg(backbone, intrinsics, ExtrinsicsProcrustesCfg("procrustes", 100, False)), 4, (8, 12)).extrinsics, ExtrinsicsProcrustes)
    assert isinstance(Model(ModelCfg(backbone, intrinsics, ExtrinsicsRegressedCfg("regressed")), 4, (8, 12)).extrinsics, ExtrinsicsRegressed)


def test_a_sharded_step_refuses_the_module_by_name():
    from flowmap_amd.sharding import FrameShard

    _, model, _, _, _ = _problem()
    with pytest.raises(ValueError, match="ExtrinsicsRegressed"):
        FrameShard(rank=0, world=2).prepare_model(model)


def test_the_captured_step_accepts_the_module():
    from flowmap_amd import training

    assert ExtrinsicsRegressed in training._our_classes()[1]


def test_the_package_exports_the_module():
    assert flowmap_amd.model.extrinsics_regressed.ExtrinsicsRegressed is ExtrinsicsRegressed
    assert flowmap_amd.ExtrinsicsRegressed is ExtrinsicsRegressed and flowmap_amd.ExtrinsicsRegressedCfg is ExtrinsicsRegressedCfg
