"""LossFlow.residuals (tests/flow_residual_cases.py) — on the MI355X: the cases of the CPU module through fm_flow_residuals.hip (scalar and
16-byte paths, one and several workgroups per pair, workgroup tails, fm_layout views), plus the kernel against the host build of the same
functions element for element."""

import pytest

import flow_residual_cases as fr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (batch, frames, h, w, a K per frame); the last two reach the second stage of the sums past one batch of 64 slots: 65 workgroups per
# pair, the last half full (a second trip of one slot), and 64 exactly — only test_sums_repeats_and_windows_gpu takes them
SHAPES = [(1, 2, 5, 7, False), (1, 5, 17, 23, True), (1, 6, 24, 32, False), (1, 4, 64, 128, True), (1, 2, 27, 76, False), (1, 2, 7, 292, True), (2, 4, 9, 12, True),
          (1, 4, 258, 512, False), (1, 2, 256, 512, False)]


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_reference_parity_gpu(case, kind):
    fr.case_reference_parity(DEV, case, kind)


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("shape", SHAPES[2:6])
def test_oracle_parity_gpu(shape, kind):
    fr.case_oracle_parity(DEV, shape, kind)


@pytest.mark.parametrize("kind", fr.KINDS)
def test_clamping_edge_gpu(kind):
    fr.case_edge(DEV, kind)


@pytest.mark.parametrize("shape", SHAPES)
def test_sums_repeats_and_windows_gpu(shape):
    fr.case_sums(DEV, shape)


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[6]])
def test_agrees_with_the_fused_loss_and_the_general_route_gpu(shape, kind):
    fr.case_hot_path(DEV, shape, kind)


@pytest.mark.parametrize("hw", [(9, 12), (5, 7)])
def test_frame_windows_and_batch_slices_in_place_gpu(hw):
    fr.case_views(DEV, hw)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone_gpu(tracking, fuse):
    fr.case_training_untouched(DEV, tracking, fuse)


def test_arguments_gpu():
    fr.case_arguments(DEV)


def test_host_tensor_without_install_is_refused_gpu():
    fr.case_host_tensor_refused()


@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("case", ["a", "b", "c", "edge"])
def test_gpu_against_host_double(case, kind):
    fr.case_gpu_against_host_double(DEV, case, kind)
