"""The lazy values of flowmap_amd/model/projection.py (tests/lazy_value_cases.py) — CPU, through the serial host double: the tensor
protocol the three classes share, peek(), the kernel input of the weights, and LossTracking.residuals as a reader that only reads."""

import pytest

import lazy_value_cases as lv
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("kind", lv.KINDS)
def test_metadata_does_not_evaluate(kind):
    lv.case_metadata("cpu", kind)


def test_frame_slices():
    lv.case_frame_slices("cpu")


@pytest.mark.parametrize("first,second", lv.PAIRS)
def test_torch_function_converts_every_lazy_argument(first, second):
    lv.case_mixed_torch_function("cpu", first, second)


def test_like_functions_of_weights_evaluate_nothing():
    lv.case_like_functions_of_weights("cpu")


@pytest.mark.parametrize("kind", lv.KINDS)
def test_reference_dispatch_does_not_evaluate(kind):
    lv.case_reference_dispatch("cpu", kind)


@pytest.mark.parametrize("kind", lv.KINDS)
def test_source_is_named(kind):
    lv.case_source_is_named("cpu", kind)


@pytest.mark.parametrize("poses", lv.POSE_COUNTS)
def test_peek_extrinsics(poses):
    lv.case_peek_extrinsics("cpu", poses)


def test_peek_surfaces_and_weights():
    lv.case_peek_surfaces_and_weights("cpu")


def test_kernel_input_of_weights():
    lv.case_kernel_input("cpu")


def test_tracking_residuals_only_read():
    lv.case_tracking_residuals_only_read("cpu")
