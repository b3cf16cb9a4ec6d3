"""export.voxel_point_cloud (tests/voxel_cloud_cases.py) — on the MI355X: the cases of the CPU module through fm_voxel_cloud.hip (fewer
pixels than a wavefront, the scalar path with a partial last quad, exactly one tile and one pixel past it, several tiles, a depth base off
the 16-byte boundary, every lane on one record, every point its own voxel, a full table, a probe chain that wraps, the grid's limits, every
way of being dropped), plus the kernel against the host build of the same functions, two calls against each other and the peak memory."""

import ctypes

import pytest

import voxel_cloud_cases as vc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", sorted(vc.SPECS))
def test_exact_properties_gpu(name):
    vc.case_exact_properties(DEV, name)


def test_cases_do_what_they_are_for_gpu():
    vc.case_shapes(DEV)


def test_capacity_one_too_small_raises_gpu():
    vc.case_capacity_short(DEV)


@pytest.mark.parametrize("name", vc.EXACT_PRODUCT_CASES)
def test_gpu_against_host_double(name):
    vc.case_gpu_against_host_double(DEV, name)


@pytest.mark.parametrize("name", ["scene", "support"])
def test_two_calls_are_bit_identical_gpu(name):
    vc.case_repeatable(DEV, name)


@pytest.mark.parametrize("name", vc.GOLDEN_CASES)
def test_reference_parity_gpu(name):
    vc.case_reference_parity(DEV, name)


def test_arguments_gpu():
    vc.case_arguments(DEV)


def test_c_entry_refuses_gpu():
    from flowmap_amd import _lib

    vc.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_is_refused_gpu():
    vc.case_host_tensor_refused()


def test_world_point_cloud_is_unchanged_gpu():
    vc.case_world_points_unchanged(DEV)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone_gpu(tracking, fuse):
    vc.case_training_untouched(DEV, tracking, fuse)


@pytest.mark.parametrize("name", ["wide", "one"])
def test_peak_memory_gpu(name):
    vc.case_memory(DEV, name)


def test_model_point_cloud_and_write_ply_gpu(tmp_path):
    vc.case_model_point_cloud(DEV, tmp_path)
