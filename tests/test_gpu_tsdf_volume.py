"""export.tsdf_volume / TsdfVolume.surface_points (tests/tsdf_volume_cases.py) — on the MI355X: the cases of the CPU module through
fm_tsdf_volume.hip (fewer voxels than a wavefront, a partial second workgroup, a wavefront exactly on a row and one past it, exactly one
workgroup and one voxel more, rows that wrap inside wavefronts, a thousand workgroups, a window of frames, a mask, spoilt depths, everything
behind a camera, no colours), the plane bit for bit against the closed form AND the host double, two calls against each other, the surface
points against the restatement (crossings in the last workgroup only, none at all, on every edge) and the peak memory."""

import ctypes

import pytest

import tsdf_volume_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", sorted(tc.SPECS))
def test_oracle_parity_gpu(name):
    tc.case_oracle_parity(DEV, name)


@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_reference_parity_gpu(name):
    tc.case_reference_parity(DEV, name)


@pytest.mark.parametrize("name", ["part", "row65", "wrap", "wide"])
def test_two_calls_are_bit_identical_gpu(name):
    tc.case_repeatable(DEV, name)


def test_plane_is_the_closed_form_and_the_host_double_bit_for_bit_gpu():
    tc.case_plane(DEV, against_host=True)


@pytest.mark.parametrize("name", ["wrap", "vec"])
def test_gpu_against_host_double(name):
    tc.case_gpu_against_host_double(DEV, name)


@pytest.mark.parametrize("name", sorted(tc.SPECS))
def test_surface_points_gpu(name):
    tc.case_surface(DEV, name)


def test_surface_points_min_weight_gpu():
    tc.case_surface(DEV, "wrap", min_weight=3)


@pytest.mark.parametrize("kind", ["none", "last", "every", "weights"])
def test_surface_points_of_hand_made_volumes_gpu(kind):
    tc.case_surface_synthetic(DEV, kind)


def test_arguments_gpu():
    tc.case_arguments(DEV)


def test_c_entry_refuses_gpu():
    from flowmap_amd import _lib

    tc.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_is_refused_gpu():
    tc.case_host_tensor_refused()


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone_gpu(tracking, fuse):
    tc.case_training_untouched(DEV, tracking, fuse)


def test_peak_memory_gpu():
    tc.case_memory(DEV, "wide")


def test_model_tsdf_grid_around_and_write_ply_gpu(tmp_path):
    tc.case_model_tsdf_grid_and_ply(DEV, tmp_path)
