"""LossFlow.residuals (tests/flow_residual_cases.py) — CPU, through the serial host double: the per-pixel function is the device kernel's
own (fm_math.h: flow_residual_at), so reference parity, the clamping edge, the sums, the windows, the views, the agreement with the fused
loss and with the general route, and the untouched training run are all decided here before a GPU is involved."""

import pytest

import flow_residual_cases as fr
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


# (batch, frames, h, w, a K per frame)
SHAPES = [(1, 2, 5, 7, False), (1, 5, 17, 23, True), (1, 6, 24, 32, False), (1, 4, 64, 128, True), (1, 2, 27, 76, False), (1, 2, 7, 292, True), (2, 4, 9, 12, True)]


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_reference_parity(case, kind):
    fr.case_reference_parity("cpu", case, kind)


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("shape", SHAPES[2:6])
def test_oracle_parity(shape, kind):
    fr.case_oracle_parity("cpu", shape, kind)


@pytest.mark.parametrize("kind", fr.KINDS)
def test_clamping_edge(kind):
    fr.case_edge("cpu", kind)


@pytest.mark.parametrize("shape", SHAPES)
def test_sums_repeats_and_windows(shape):
    fr.case_sums("cpu", shape)


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[6]])
def test_agrees_with_the_fused_loss_and_the_general_route(shape, kind):
    fr.case_hot_path("cpu", shape, kind)


@pytest.mark.parametrize("hw", [(9, 12), (5, 7)])
def test_frame_windows_and_batch_slices_in_place(hw):
    fr.case_views("cpu", hw)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone(tracking, fuse):
    fr.case_training_untouched("cpu", tracking, fuse)


def test_arguments():
    fr.case_arguments("cpu")


def test_host_tensor_without_install_is_refused():
    try:
        fr.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


def test_exported():
    import flowmap_amd

    assert flowmap_amd.FlowResiduals is flowmap_amd.types.FlowResiduals and "FlowResiduals" in flowmap_amd.__all__
