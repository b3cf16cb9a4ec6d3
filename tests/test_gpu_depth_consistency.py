"""projection.depth_consistency (tests/depth_consistency_cases.py) — on the MI355X: the cases of the CPU module through
fm_depth_consistency.hip (fewer pixels than a wavefront, the scalar path with a partial last quad, eight offsets, the 16-byte path below
one tile, several whole tiles, exactly one tile and one pixel past it, two batch entries, every code), plus the kernel against the host
build of the same functions element for element, and the peak memory of a call."""

import ctypes

import pytest

import depth_consistency_cases as dc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", dc.GOLDEN_CASES)
def test_reference_parity_gpu(name):
    dc.case_reference_parity(DEV, name)


@pytest.mark.parametrize("name", sorted(dc.SPECS))
def test_oracle_parity_every_window_gpu(name):
    dc.case_oracle_parity(DEV, name)


@pytest.mark.parametrize("name", ["tiny", "odd", "vec", "two"])
def test_agrees_with_the_flow_residuals_gpu(name):
    dc.case_flow_cross_check(DEV, name)


@pytest.mark.parametrize("name", sorted(dc.SPECS))
def test_reproducible_window_independent_and_derived_outputs_gpu(name):
    dc.case_reproducible(DEV, name)


@pytest.mark.parametrize("name", sorted(dc.SPECS))
def test_gpu_against_host_double(name):
    dc.case_gpu_against_host_double(DEV, name)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone_gpu(tracking, fuse):
    dc.case_training_untouched(DEV, tracking, fuse)


def test_arguments_gpu():
    dc.case_arguments(DEV)


def test_c_entry_refuses_gpu():
    from flowmap_amd import _lib

    dc.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_is_refused_gpu():
    dc.case_host_tensor_refused()


@pytest.mark.parametrize("name", ["wide", "odd"])
def test_peak_memory_gpu(name):
    dc.case_memory(DEV, name)


def test_point_cloud_keep_gpu():
    dc.case_point_cloud_keep(DEV)
