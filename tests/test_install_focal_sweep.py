"""flowmap_amd.install() and IntrinsicsSoftmin.residuals: the method is on the module the host application's own ``get_intrinsics`` builds
(install() registers this package's class as INTRINSICS["softmin"]), on device tensors it is the fused call and returns the numbers of the
oracle parity, HOST tensors are refused, and after uninstall() the host application's class is back and has no such method.  The host
application is the stand-in package (bench_support/standin: the reference's module layout) and, where it is importable, the reference."""

import os
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("FLOWMAP_REFERENCE", "/root/reference"))
CASE = "odd"


def _reference_readable() -> bool:
    try:
        return (REF / "flowmap" / "model" / "projection.py").is_file()
    except OSError:
        return False


def _problem(dev):
    import focal_sweep_cases as fs

    from flowmap.dataset.types import Batch
    from flowmap.flow.flow_predictor import Flows
    from flowmap.model.intrinsics import IntrinsicsSoftminCfg, get_intrinsics

    try:  # (the reference keeps RegressionCfg beside its class, the stand-in beside its registry)
        from flowmap.model.intrinsics.intrinsics_softmin import RegressionCfg
    except ImportError:
        from flowmap.model.intrinsics import RegressionCfg

    x = {key: v.clone().to(dev) for key, v in fs.case_inputs(CASE).items()}
    (b, f, h, w), _, points, n = fs.SPECS[CASE]
    module = get_intrinsics(IntrinsicsSoftminCfg("softmin", points, 0.5, 2.0, n, RegressionCfg(1000, 100))).to(dev)  # the host application's factory
    flows = Flows(x["bwd"], x["bwd"], x["weights"], x["weights"])
    batch = Batch(torch.zeros((b, f, 3, h, w), device=dev), torch.arange(f)[None], ["s"], ["d"])
    return module, batch, flows, x


def _installed_device_call(dev):
    import focal_sweep_cases as fs

    import flowmap_amd
    from flowmap_amd import BackboneOutput, FocalSweep, _ops

    flowmap_amd.install()
    try:
        module, batch, flows, x = _problem(dev)
        assert type(module) is flowmap_amd.model.intrinsics_softmin.IntrinsicsSoftmin  # what install() registered
        idx = fs.case_indices(CASE).to(dev)
        before = _ops.counters["focal_sweep"]
        r = module.residuals(batch, flows, BackboneOutput(x["depth"], x["weights"]), indices=idx, points=True)
        assert _ops.counters["focal_sweep"] == before + 1 and isinstance(r, FocalSweep)  # the fused call, once
        fs.check_layout(r, CASE, dev)
        terms = fs.oracle_case(CASE, idx)
        fs.check_fields(r, terms[torch.float64], terms[torch.float32], "installed")
        win = module.residuals(batch, flows, BackboneOutput(x["depth"], x["weights"]), indices=idx, pairs=(1, 2))
        fs.check_fields(win, terms[torch.float64], terms[torch.float32], "installed, window (1, 2)", rows=slice(1, 3))
    finally:
        flowmap_amd.uninstall()
        flowmap_amd.set_lazy_surfaces(False)
    module, _, _, _ = _problem("cpu")  # after uninstall(): the host application's own class, which has no such method
    assert not type(module).__module__.startswith("flowmap_amd") and not hasattr(module, "residuals")


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
    from flowmap_amd import BackboneOutput, _lib, _ops

    _lib.set_library_for_testing(None)
    flowmap_amd.install()
    try:
        module, batch, flows, x = _problem("cpu")
        assert type(module) is flowmap_amd.model.intrinsics_softmin.IntrinsicsSoftmin
        before = _ops.counters["focal_sweep"]
        with pytest.raises(RuntimeError, match="flowmap_amd: focal_sweep: tensors are on cpu.*no CPU fallback"):
            module.residuals(batch, flows, BackboneOutput(x["depth"], x["weights"]))
        assert _ops.counters["focal_sweep"] == before
    finally:
        flowmap_amd.uninstall()


@pytest.mark.gpu
def test_install_on_the_standin_runs_the_hip_kernel(standin):
    from flowmap_amd import _lib

    _lib.set_library_for_testing(None)
    _installed_device_call("cuda:0")


@pytest.mark.skipif(not _reference_readable(), reason="reference not mounted or not readable")
def test_install_on_the_reference_with_the_host_double():
    import flowmap_amd
    from conftest import forget_flowmap_modules
    from flowmap_amd import _lib
    from helpers import build_host_sim

    sys.dont_write_bytecode = True
    flowmap_amd.uninstall()
    forget_flowmap_modules()
    added = [str(ROOT / "oracle" / "refstubs"), str(REF)]
    sys.path[:0] = added
    _lib.set_library_for_testing(build_host_sim())
    try:
        import flowmap

        assert not str(getattr(flowmap, "__file__", None) or list(flowmap.__path__)[0]).startswith(str(ROOT))  # the reference, not the stand-in
        _installed_device_call("cpu")
    finally:
        flowmap_amd.uninstall()
        _lib.set_library_for_testing(None)
        forget_flowmap_modules()
        for p in added:
            sys.path.remove(p)
