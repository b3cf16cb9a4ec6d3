"""LossTracking.residuals (tests/track_residual_cases.py) — on the MI355X: the cases of the CPU module through fm_track_residuals.hip (one
point to several workgroups of points, one to thirteen frames per segment, 65 segments in one launch, idle point chunks, an odd width),
plus the kernel against the host build of the same functions element for element."""

import pytest

import track_residual_cases as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("case", tr.FIXTURE_CASES)
def test_reference_parity_gpu(case, kind):
    tr.case_reference_parity(DEV, case, kind)


@pytest.mark.parametrize("spec", tr.GEOMETRY)
def test_launch_geometry_gpu(spec):
    tr.case_geometry(DEV, spec)


@pytest.mark.parametrize("spec", ["mixed", "P257", "items260", "nothing-visible", "tap-edges"])
def test_sums_repeats_and_windows_gpu(spec):
    tr.case_sums(DEV, spec)


@pytest.mark.parametrize("spec", ["mixed", "mixed-l1", "mixed-l2", "mixed-10x13", "P257", "source-outside"])
def test_agrees_with_the_fused_loss_and_the_general_route_gpu(spec):
    tr.case_hot_path(DEV, spec)


@pytest.mark.parametrize("kind", tr.KINDS)
def test_camera_plane_gpu(kind):
    tr.case_camera_plane(DEV, kind)


@pytest.mark.parametrize("fuse", [True, False])
def test_training_is_left_alone_gpu(fuse):
    tr.case_training_untouched(DEV, fuse)


def test_arguments_gpu():
    tr.case_arguments(DEV)


def test_host_tensor_without_install_is_refused_gpu():
    tr.case_host_tensor_refused()


@pytest.mark.parametrize("which", ["a", "b", "mixed", "camera-plane"])
def test_gpu_against_host_double(which):
    tr.case_gpu_against_host_double(DEV, which)
