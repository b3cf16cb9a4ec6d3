"""flowmap_amd.install() and LossFlow.residuals, on the stand-in package (bench_support/standin: the reference's module layout), where the
reference itself cannot be: the method is on the loss objects the reference's own ``get_losses`` builds, on device tensors it is the fused
launch, and HOST tensors (the real C ABI selected, no test double) reach the functions install() replaced — the stand-in's own
compute_forward_flow / compute_backward_flow / mapping — and come back as the same fields."""

import pytest
import torch


def _problem(dev):
    import flow_residual_cases as fr

    import flowmap.loss as ref_loss
    from flowmap.dataset.types import Batch
    from flowmap.flow.flow_predictor import Flows
    from flowmap.loss.loss_flow import LossFlowCfg
    from flowmap.loss.mapping import MappingHuberCfg
    from flowmap.model.model import ModelOutput
    from flowmap.model.projection import sample_image_grid, unproject

    x = {key: v.to(dev) for key, v in fr.golden_inputs("b").items()}
    b, f, h, w = x["depth"].shape
    xy, _ = sample_image_grid((h, w), x["depth"].device)
    surfaces = unproject(xy, x["depth"], x["k"][:, :, None, None])  # model.py: what the reference's Model hands its losses
    out = ModelOutput(x["depth"], surfaces, x["k"], x["extrinsics"], None)
    flows = Flows(x["fwd"], x["bwd"], x["fwd_mask"], x["bwd_mask"])
    (loss,) = ref_loss.get_losses([LossFlowCfg(0, 1000.0, "flow", MappingHuberCfg("huber", 0.01))])
    return loss, Batch(torch.zeros((b, f, 3, h, w), device=dev), torch.arange(f)[None], ["s"], ["d"]), flows, out


def _check_against_fixture(r, first=0, count=None):
    import flow_residual_cases as fr
    from conftest import assert_close_or_reference_gap

    g = fr.golden()
    win = slice(first, None if count is None else first + count)
    for ours, name in ((r.forward, "huber_forward"), (r.backward, "huber_backward"), (r.forward_flow, "pred_forward"), (r.backward_flow, "pred_backward")):
        assert_close_or_reference_gap(ours.cpu(), g[f"b_f64_{name}"][:, win], g[f"b_{name}"][:, win], rel=1e-4, slack=2.0, what=name)


def test_host_tensors_after_install_reach_the_replaced_functions(standin):
    import flowmap.model.projection as ref_projection

    import flowmap_amd
    from flowmap_amd import FlowResiduals, _lib, _reference

    _lib.set_library_for_testing(None)
    original_forward = ref_projection.compute_forward_flow
    flowmap_amd.install()
    try:
        loss, batch, flows, out = _problem("cpu")
        assert type(loss) is flowmap_amd.loss.LossFlow and torch.is_tensor(out.surfaces)
        before = _reference.counters["host_calls"]
        r = loss.residuals(batch, flows, out, pairs=(1, 2), predicted_flow=True)
        assert _reference.counters["host_calls"] > before
        assert isinstance(r, FlowResiduals) and r.first_pair == 1
        assert r.forward.shape == (1, 2, 17, 23) and r.forward_flow.shape == (1, 2, 17, 23, 2) and r.pair_sum.shape == (1, 2, 2)
        assert r.pair_sum.dtype == torch.float64 and r.forward.device.type == "cpu" and not r.forward.requires_grad
        _check_against_fixture(r, 1, 2)
        # the same numbers as the replaced functions called directly (what install() recorded as their twins)
        xy, _ = _reference.twins["sample_image_grid"]((17, 23), torch.device("cpu"))
        want = _reference.twins["compute_forward_flow"](out.surfaces[:, 1:4], out.extrinsics[:, 1:4], out.intrinsics[:, 1:4]) - xy
        assert _reference.twins["compute_forward_flow"] is original_forward and torch.equal(r.forward_flow, want)
        assert torch.equal(r.pair_sum[..., 0], (r.forward * flows.forward_mask[:, 1:3]).double().sum(dim=(2, 3)))
        assert torch.equal(r.pair_loss(), r.pair_sum / r.pair_valid)
        bare = loss.residuals(batch, flows, out, sums=False)
        assert bare.pair_sum is None and bare.forward_flow is None and bare.forward.shape == (1, 4, 17, 23)
    finally:
        flowmap_amd.uninstall()


def _installed_device_call(dev):
    import flowmap_amd
    from flowmap_amd import _ops
    from flowmap_amd.model.projection import LazySurfaces

    flowmap_amd.install()
    try:
        loss, batch, flows, out = _problem(dev)
        assert type(loss) is flowmap_amd.loss.LossFlow and isinstance(out.surfaces, LazySurfaces)  # the stand-in's unproject went lazy
        before = _ops.counters["flow_residuals"]
        r = loss.residuals(batch, flows, out, predicted_flow=True)
        assert _ops.counters["flow_residuals"] == before + 1  # the fused launch
        _check_against_fixture(r)
    finally:
        flowmap_amd.uninstall()
        flowmap_amd.set_lazy_surfaces(False)


def test_install_on_the_standin_with_the_host_double(standin):
    from flowmap_amd import _lib
    from helpers import build_host_sim

    _lib.set_library_for_testing(build_host_sim())
    try:
        _installed_device_call("cpu")
    finally:
        _lib.set_library_for_testing(None)


@pytest.mark.gpu
def test_install_on_the_standin_runs_the_hip_kernel(standin):
    from flowmap_amd import _lib

    _lib.set_library_for_testing(None)
    _installed_device_call("cuda:0")
