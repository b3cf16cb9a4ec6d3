"""export.tsdf_volume / TsdfVolume.surface_points (tests/tsdf_volume_cases.py) — CPU, through the serial host double: the per-voxel and
per-edge functions are the device kernels' own (fm_math.h: tsdf_centre, tsdf_pixel_of, tsdf_term, tsdf_edge_crosses, tsdf_edge_point), so
the gate on the decisions, the closed form of the plane, the surface restatement and its bounds, reference parity, the arguments and the
exported names are all decided here before a GPU is involved.  What the double does not cover — the launch geometry, the scan through LDS,
the scalar loads of the per-frame constants — the `-m gpu` tests do."""

import ctypes

import pytest

import tsdf_volume_cases as tc
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("name", sorted(tc.SPECS))
def test_inputs_are_well_conditioned(name):
    tc.case_well_conditioned(name)


@pytest.mark.parametrize("name", sorted(tc.SPECS))
def test_oracle_parity(name):
    tc.case_oracle_parity("cpu", name)


@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_reference_parity(name):
    tc.case_reference_parity("cpu", name)


@pytest.mark.parametrize("name", ["part", "wrap"])
def test_two_calls_are_bit_identical(name):
    tc.case_repeatable("cpu", name)


def test_plane_is_the_closed_form_bit_for_bit():
    tc.case_plane("cpu")


@pytest.mark.parametrize("name", sorted(tc.SPECS))
def test_surface_points(name):
    tc.case_surface("cpu", name)


def test_surface_points_min_weight():
    tc.case_surface("cpu", "wrap", min_weight=3)


@pytest.mark.parametrize("kind", ["none", "last", "every", "weights"])
def test_surface_points_of_hand_made_volumes(kind):
    tc.case_surface_synthetic("cpu", kind)


def test_arguments():
    tc.case_arguments("cpu")


def test_c_entries_refuse_on_both_builds():
    if not _lib.LIB_PATH.exists():
        from flowmap_amd.build import build_library

        build_library()
    tc.case_c_entries_refuse(ctypes.CDLL(str(build_host_sim())), "host double")
    tc.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_without_the_double_is_refused():
    try:
        tc.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone(tracking, fuse):
    tc.case_training_untouched("cpu", tracking, fuse)


def test_model_tsdf_grid_around_and_write_ply(tmp_path):
    tc.case_model_tsdf_grid_and_ply("cpu", tmp_path)


def test_exported():
    import flowmap_amd
    from flowmap_amd.model.model import Model

    assert flowmap_amd.TsdfVolume is flowmap_amd.types.TsdfVolume and "TsdfVolume" in flowmap_amd.__all__
    assert "tsdf_volume" in flowmap_amd.__all__ and callable(Model.tsdf) and callable(flowmap_amd.export.grid_around)
    assert flowmap_amd.tsdf_volume is flowmap_amd.export.tsdf_volume
