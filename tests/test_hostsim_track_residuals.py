"""LossTracking.residuals (tests/track_residual_cases.py) — CPU, through the serial host double: the per-element function is the device
kernel's own (fm_pose.h: track_residual_at), so reference parity, the launch-geometry list's inputs and truths, the sums, the windows, the
camera-plane element, the agreement with the fused loss and the general route, and the untouched training run are all decided here before
a GPU is involved."""

import pytest

import track_residual_cases as tr
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("case", tr.FIXTURE_CASES)
def test_reference_parity(case, kind):
    tr.case_reference_parity("cpu", case, kind)


@pytest.mark.parametrize("spec", tr.GEOMETRY)
def test_launch_geometry(spec):
    tr.case_geometry("cpu", spec)


@pytest.mark.parametrize("spec", ["mixed", "P257", "items260", "nothing-visible", "tap-edges"])
def test_sums_repeats_and_windows(spec):
    tr.case_sums("cpu", spec)


@pytest.mark.parametrize("spec", ["mixed", "mixed-l1", "mixed-l2", "mixed-10x13", "P257", "source-outside"])
def test_agrees_with_the_fused_loss_and_the_general_route(spec):
    tr.case_hot_path("cpu", spec)


@pytest.mark.parametrize("kind", tr.KINDS)
def test_camera_plane(kind):
    tr.case_camera_plane("cpu", kind)


@pytest.mark.parametrize("fuse", [True, False])
def test_training_is_left_alone(fuse):
    tr.case_training_untouched("cpu", fuse)


def test_arguments():
    tr.case_arguments("cpu")


def test_host_tensor_without_install_is_refused():
    try:
        tr.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


def test_visibility_equality_is_not_vacuous():
    """No spec of the list happens to hold a target within fp32 rounding of the frame edge, so one is built: without the
    margin rule the exact comparison of ``visible`` fails there, with it the comparison passes."""
    found, differ, with_rule, altered = tr.case_negative_control("cpu", tr.GEOMETRY)
    assert differ > 0, "no fp32 neighbour of the built principal point separates the fp32 from the fp64 visibility"
    assert with_rule == 0 and altered > 0


def test_exported():
    import flowmap_amd

    assert flowmap_amd.TrackResiduals is flowmap_amd.types.TrackResiduals and "TrackResiduals" in flowmap_amd.__all__
