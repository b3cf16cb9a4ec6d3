"""flowmap_amd.install() and LossTracking.residuals.  On the stand-in package (bench_support/standin: the reference's module layout), where
the reference itself cannot be: the method is on the loss objects the reference's own ``get_losses`` builds, on device tensors it is the
fused launch, and HOST tensors (the real C ABI selected, no test double) reach the functions install() replaced — compute_track_flow and
the mapping — and agree with the fixture.  Where the real reference is mounted (skipped elsewhere) the same on its own classes."""

import os
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("FLOWMAP_REFERENCE", "/root/reference"))


def _reference_readable() -> bool:
    try:
        return (REF / "flowmap" / "loss" / "loss_tracking.py").is_file()
    except OSError:
        return False


def _problem(dev):
    """The fixture's case "a" in the `flowmap` package that is importable right now (the stand-in or the reference)."""
    import track_residual_cases as tr

    import flowmap.loss as ref_loss
    from flowmap.dataset.types import Batch
    from flowmap.loss.loss_tracking import LossTrackingCfg
    from flowmap.loss.mapping import MappingHuberCfg
    from flowmap.model.model import ModelOutput
    from flowmap.model.projection import sample_image_grid, unproject
    from flowmap.tracking.track_predictor import Tracks

    spec, (depth, k, e), tracks = tr.golden_problem("a")
    depth, k, e = depth.to(dev), k.to(dev), e.to(dev)
    h, w = spec.hw
    xy, _ = sample_image_grid((h, w), depth.device)
    surfaces = unproject(xy, depth, k[:, :, None, None])  # model.py: what the reference's Model hands its losses
    out = ModelOutput(depth, surfaces, k, e, None)
    (loss,) = ref_loss.get_losses([LossTrackingCfg(0, 100.0, "tracking", MappingHuberCfg("huber", tr.DELTA))])
    trk = [Tracks(x.xy.to(dev), x.visibility.to(dev), x.start_frame) for x in tracks]
    return loss, Batch(torch.zeros((1, spec.frames, 3, h, w), device=dev), torch.arange(spec.frames)[None], ["s"], ["d"]), trk, out


def _check_against_fixture(rs, first=0):
    import track_residual_cases as tr

    truth, ref32 = tr.golden_terms("a", "huber")
    for i, r in enumerate(rs):
        assert r.segment == first + i
        tr.check_segment(r, truth[first + i], ref32[first + i], f"install, segment {first + i}")


def _host_tensors_reach_the_replaced_functions(projection_module):
    import flowmap_amd
    from flowmap_amd import TrackResiduals, _lib, _reference

    _lib.set_library_for_testing(None)
    original = projection_module.compute_track_flow
    flowmap_amd.install()
    try:
        loss, batch, trk, out = _problem("cpu")
        assert type(loss) is flowmap_amd.loss.LossTracking and torch.is_tensor(out.surfaces)
        before = _reference.counters["host_calls"]
        rs = loss.residuals(batch, trk, out, segments=(1, 1), predicted=True)
        assert _reference.counters["host_calls"] > before
        (r,) = rs
        assert isinstance(r, TrackResiduals) and (r.segment, r.start_frame) == (1, 1)
        assert r.residual.shape == (1, 3, 3, 7) and r.xy_target.shape == (1, 3, 3, 7, 2) and r.pair_sum.shape == (3, 3) and r.track_sum.shape == (7,)
        assert r.pair_sum.dtype == torch.float64 and r.residual.device.type == "cpu" and not r.residual.requires_grad
        _check_against_fixture(rs, 1)
        # the same numbers as the replaced function called directly (what install() recorded as its twin)
        assert _reference.twins["compute_track_flow"] is original
        want, vis = original(out.surfaces[:, 1:4], out.extrinsics[:, 1:4], out.intrinsics[:, 1:4], trk[1])
        assert torch.equal(r.xy_target, want) and torch.equal(r.visible, vis)
        assert torch.equal(r.pair_count, vis[0].double().sum(dim=2))
        bare = loss.residuals(batch, trk, out, sums=False)
        assert len(bare) == 2 and bare[0].pair_sum is None and bare[0].xy_target is None and bare[0].residual.shape == (1, 5, 5, 40)
        _check_against_fixture(bare)
    finally:
        flowmap_amd.uninstall()


def test_host_tensors_after_install_reach_the_replaced_functions(standin):
    import flowmap.model.projection as ref_projection

    _host_tensors_reach_the_replaced_functions(ref_projection)


def _installed_device_call(dev):
    import flowmap_amd
    from flowmap_amd import _ops
    from flowmap_amd.model.projection import LazySurfaces

    flowmap_amd.install()
    try:
        loss, batch, trk, out = _problem(dev)
        assert type(loss) is flowmap_amd.loss.LossTracking and isinstance(out.surfaces, LazySurfaces)  # the package's unproject went lazy
        before = _ops.counters["track_residuals"]
        rs = loss.residuals(batch, trk, out, predicted=True)
        assert _ops.counters["track_residuals"] == before + 1  # the fused launch
        _check_against_fixture(rs)
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


@pytest.fixture()
def reference_on_path():
    from conftest import forget_flowmap_modules

    sys.dont_write_bytecode = True
    added = [str(ROOT / "oracle" / "refstubs"), str(REF)]
    import flowmap_amd
    from flowmap_amd import _lib

    flowmap_amd.uninstall()
    forget_flowmap_modules()
    sys.path[:0] = added
    yield
    flowmap_amd.uninstall()
    _lib.set_library_for_testing(None)
    forget_flowmap_modules()
    for p in added:
        sys.path.remove(p)


@pytest.mark.skipif(not _reference_readable(), reason="reference not mounted or not readable")
def test_host_tensors_after_install_on_the_real_reference(reference_on_path):
    import flowmap.model.projection as ref_projection

    assert str(Path(ref_projection.__file__).resolve()).startswith(str(REF.resolve()))
    _host_tensors_reach_the_replaced_functions(ref_projection)


@pytest.mark.skipif(not _reference_readable(), reason="reference not mounted or not readable")
def test_install_on_the_real_reference_with_the_host_double(reference_on_path):
    from flowmap_amd import _lib
    from helpers import build_host_sim

    _lib.set_library_for_testing(build_host_sim())
    try:
        _installed_device_call("cpu")
    finally:
        _lib.set_library_for_testing(None)
