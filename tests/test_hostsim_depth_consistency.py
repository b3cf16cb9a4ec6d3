"""projection.depth_consistency (tests/depth_consistency_cases.py) — CPU, through the serial host double: the per-element and per-row
functions are the device kernels' own (fm_math.h: depth_consistency_at, depth_consistency_pose), so reference and oracle parity on every
shape and window, the flow residuals' route to the same positions, reproducibility, the derived outputs, the arguments, the untouched
training run and the filtered point cloud are all decided here before a GPU is involved."""

import ctypes

import pytest

import depth_consistency_cases as dc
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("name", dc.GOLDEN_CASES)
def test_reference_parity(name):
    dc.case_reference_parity("cpu", name)


@pytest.mark.parametrize("name", sorted(dc.SPECS))
def test_oracle_parity_every_window(name):
    dc.case_oracle_parity("cpu", name)


@pytest.mark.parametrize("name", sorted(dc.SPECS))
def test_inputs_are_well_conditioned(name):
    dc.case_generator_precondition(name)


@pytest.mark.parametrize("name", ["tiny", "odd", "vec", "two"])
def test_agrees_with_the_flow_residuals(name):
    dc.case_flow_cross_check("cpu", name)


@pytest.mark.parametrize("name", sorted(dc.SPECS))
def test_reproducible_window_independent_and_derived_outputs(name):
    dc.case_reproducible("cpu", name)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone(tracking, fuse):
    dc.case_training_untouched("cpu", tracking, fuse)


def test_arguments():
    dc.case_arguments("cpu")


def test_c_entries_refuse_on_both_builds():
    if not _lib.LIB_PATH.exists():
        from flowmap_amd.build import build_library

        build_library()
    dc.case_c_entries_refuse(ctypes.CDLL(str(build_host_sim())), "host double")
    dc.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_without_the_double_is_refused():
    try:
        dc.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


def test_point_cloud_keep():
    dc.case_point_cloud_keep("cpu")


def test_exported():
    import flowmap_amd
    from flowmap_amd.model.model import Model

    assert flowmap_amd.DepthConsistency is flowmap_amd.types.DepthConsistency and "DepthConsistency" in flowmap_amd.__all__
    assert "depth_consistency" in flowmap_amd.__all__ and callable(Model.consistency)
