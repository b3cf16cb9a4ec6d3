"""The lazy values of flowmap_amd/model/projection.py (tests/lazy_value_cases.py) — on the MI355X: the cases of the CPU module with the
values evaluated by the device kernels (fm_unproject_fwd, fm_pose_chain_fwd at 1, 3 and 257 poses, fm_track_residuals)."""

import pytest

import lazy_value_cases as lv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("kind", lv.KINDS)
def test_metadata_does_not_evaluate_gpu(kind):
    lv.case_metadata(DEV, kind)


def test_frame_slices_gpu():
    lv.case_frame_slices(DEV)


@pytest.mark.parametrize("first,second", lv.PAIRS)
def test_torch_function_converts_every_lazy_argument_gpu(first, second):
    lv.case_mixed_torch_function(DEV, first, second)


def test_like_functions_of_weights_evaluate_nothing_gpu():
    lv.case_like_functions_of_weights(DEV)


@pytest.mark.parametrize("kind", lv.KINDS)
def test_reference_dispatch_does_not_evaluate_gpu(kind):
    lv.case_reference_dispatch(DEV, kind)


@pytest.mark.parametrize("kind", lv.KINDS)
def test_source_is_named_gpu(kind):
    lv.case_source_is_named(DEV, kind)


@pytest.mark.parametrize("poses", lv.POSE_COUNTS)
def test_peek_extrinsics_gpu(poses):
    lv.case_peek_extrinsics(DEV, poses)


def test_peek_surfaces_and_weights_gpu():
    lv.case_peek_surfaces_and_weights(DEV)


def test_kernel_input_of_weights_gpu():
    lv.case_kernel_input(DEV)


def test_tracking_residuals_only_read_gpu():
    lv.case_tracking_residuals_only_read(DEV)
