"""flowmap_amd.install() and ExtrinsicsProcrustes.residuals, on the stand-in package (bench_support/standin: the reference's module layout),
where the reference itself cannot be: the method is on the module the reference's own ``get_extrinsics`` builds (install() registers this
package's class as EXTRINSICS["procrustes"]), on device tensors it is the fused launch, and HOST tensors are refused — the reference has
no function that returns this quantity, so there is nothing to hand them to."""

import pytest
import torch


def _problem(dev):
    import alignment_residual_cases as ar

    from flowmap.dataset.types import Batch
    from flowmap.flow.flow_predictor import Flows
    from flowmap.model.extrinsics import get_extrinsics
    from flowmap.model.extrinsics.extrinsics_procrustes import ExtrinsicsProcrustesCfg
    from flowmap.model.model import ModelOutput
    from flowmap.model.projection import sample_image_grid, unproject

    x = {key: v.to(dev) for key, v in ar.golden_inputs("b").items()}
    b, f, h, w = x["depth"].shape
    xy, _ = sample_image_grid((h, w), x["depth"].device)
    surfaces = unproject(xy, x["depth"], x["k"][:, :, None, None])  # model.py: what the reference's Model hands its extrinsics module
    out = ModelOutput(x["depth"], surfaces, x["k"], x["extrinsics"], x["weights"])
    flows = Flows(x["bwd"], x["bwd"], x["weights"], x["weights"])
    module = get_extrinsics(ExtrinsicsProcrustesCfg("procrustes", 40, False), f)
    return module, Batch(torch.zeros((b, f, 3, h, w), device=dev), torch.arange(f)[None], ["s"], ["d"]), flows, out


def _installed_device_call(dev):
    import alignment_residual_cases as ar

    import flowmap_amd
    from flowmap_amd import AlignmentResiduals, _ops
    from flowmap_amd.model.projection import LazySurfaces

    flowmap_amd.install()
    try:
        module, batch, flows, out = _problem(dev)
        assert type(module) is flowmap_amd.model.extrinsics_procrustes.ExtrinsicsProcrustes  # what install() registered
        assert isinstance(out.surfaces, LazySurfaces)  # the stand-in's unproject went lazy
        before = _ops.counters["alignment_residuals"]
        r = module.residuals(batch, flows, out, offsets=True)
        assert _ops.counters["alignment_residuals"] == before + 1  # the fused launch, once
        assert isinstance(r, AlignmentResiduals) and r.residual.shape == (1, 4, 17, 23) and r.residual.device.type == torch.device(dev).type
        ar.check_terms(r, *ar.golden_terms("b", "dense"), "installed, dense")
        indices = ar.t(ar.golden()["b_indices"]).to(dev)
        win = module.residuals(batch, flows, out, pairs=(1, 2), indices=indices, offsets=True)
        assert win.first_pair == 1 and win.residual.shape == (1, 2, 40)
        ar.check_terms(win, *ar.golden_terms("b", "given"), "installed, window on indices", win=slice(1, 3))
        assert _ops.counters["alignment_residuals"] == before + 2
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


def test_host_tensors_after_install_are_refused(standin):
    import flowmap_amd
    from flowmap_amd import _lib, _ops

    _lib.set_library_for_testing(None)
    flowmap_amd.install()
    try:
        module, batch, flows, out = _problem("cpu")
        assert type(module) is flowmap_amd.model.extrinsics_procrustes.ExtrinsicsProcrustes and torch.is_tensor(out.surfaces)
        before = _ops.counters["alignment_residuals"]
        with pytest.raises(RuntimeError, match="flowmap_amd: alignment_residuals: tensors are on cpu.*no CPU fallback"):
            module.residuals(batch, flows, out)
        assert _ops.counters["alignment_residuals"] == before
    finally:
        flowmap_amd.uninstall()


@pytest.mark.gpu
def test_install_on_the_standin_runs_the_hip_kernel(standin):
    from flowmap_amd import _lib

    _lib.set_library_for_testing(None)
    _installed_device_call("cuda:0")
