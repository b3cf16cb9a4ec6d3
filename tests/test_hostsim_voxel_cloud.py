"""export.voxel_point_cloud (tests/voxel_cloud_cases.py) — CPU, through the serial host double: the per-point functions are the device
kernels' own (fm_math.h: world_point_at, voxel_point, voxel_hash, voxel_color, voxel_finalize), so the restatement, the derived bounds,
reference parity, the arguments, the untouched operators and the exported names are all decided here before a GPU is involved.  What the
double does not cover — the compare-and-swap under contention, the atomics, the launch geometry — the `-m gpu` tests do."""

import ctypes

import pytest

import voxel_cloud_cases as vc
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("name", sorted(vc.SPECS))
def test_exact_properties(name):
    vc.case_exact_properties("cpu", name)


def test_cases_do_what_they_are_for():
    vc.case_shapes("cpu")


def test_capacity_one_too_small_raises():
    vc.case_capacity_short("cpu")


@pytest.mark.parametrize("name", vc.GOLDEN_CASES)
def test_reference_parity(name):
    vc.case_reference_parity("cpu", name)


def test_arguments():
    vc.case_arguments("cpu")


def test_c_entries_refuse_on_both_builds():
    if not _lib.LIB_PATH.exists():
        from flowmap_amd.build import build_library

        build_library()
    vc.case_c_entries_refuse(ctypes.CDLL(str(build_host_sim())), "host double")
    vc.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_without_the_double_is_refused():
    try:
        vc.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


def test_world_point_cloud_is_unchanged():
    vc.case_world_points_unchanged("cpu")


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone(tracking, fuse):
    vc.case_training_untouched("cpu", tracking, fuse)


def test_model_point_cloud_and_write_ply(tmp_path):
    vc.case_model_point_cloud("cpu", tmp_path)


def test_exported():
    import flowmap_amd
    from flowmap_amd.model.model import Model

    assert flowmap_amd.VoxelCloud is flowmap_amd.types.VoxelCloud and "VoxelCloud" in flowmap_amd.__all__
    assert "voxel_point_cloud" in flowmap_amd.__all__ and callable(Model.point_cloud)
    assert flowmap_amd.voxel_point_cloud is flowmap_amd.export.voxel_point_cloud
