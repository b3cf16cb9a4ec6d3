"""ExtrinsicsProcrustes.residuals (tests/alignment_residual_cases.py) — on the MI355X: the cases of the CPU module through
fm_alignment_residuals.hip (both sources; fewer elements than a wavefront, one and several tiles per pair, tile tails, two batch entries,
the index sets), plus the kernel against the host build of the same functions element for element."""

import pytest

import alignment_residual_cases as ar

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (batch, frames, h, w, a K per frame); the last two reach the second stage of the sums past one batch of 64 slots: 65 tiles per pair
# (a second trip of one slot) and 64 exactly — only test_sums_repeats_and_windows_gpu takes them
SHAPES = [(1, 2, 5, 7, False), (1, 5, 17, 23, True), (1, 6, 24, 32, False), (1, 4, 64, 128, True), (1, 2, 25, 41, False), (1, 2, 31, 33, True), (2, 4, 9, 12, True),
          (1, 4, 129, 512, False), (1, 2, 128, 512, False)]
# (shape, how the indices are drawn)
INDEXED = [(SHAPES[1], "three"), (SHAPES[0], "fifty"), (SHAPES[2], "tile+1"), (SHAPES[3], "linspace")]


@pytest.mark.parametrize("case", ["a", "b", "c", "border"])
def test_reference_parity_gpu(case):
    ar.case_reference_parity(DEV, case)


def test_border_clamp_gpu():
    ar.case_border(DEV)


@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("shape", SHAPES[2:6])
def test_oracle_parity_gpu(shape, fit):
    ar.case_oracle_parity(DEV, shape, None, fit)


@pytest.mark.parametrize("shape,how", INDEXED)
def test_oracle_parity_on_indices_gpu(shape, how):
    ar.case_oracle_parity(DEV, shape, how, how != "three")


@pytest.mark.parametrize("shape,how", [(SHAPES[1], None), (SHAPES[6], None), (SHAPES[4], None)] + INDEXED[1:])
def test_convention_by_the_fit_gpu(shape, how):
    ar.case_convention(DEV, shape, how)


@pytest.mark.parametrize("shape", SHAPES)
def test_sums_repeats_and_windows_gpu(shape):
    ar.case_sums(DEV, shape)


@pytest.mark.parametrize("shape,how", INDEXED)
def test_sums_repeats_and_windows_on_indices_gpu(shape, how):
    ar.case_sums(DEV, shape, how)


@pytest.mark.parametrize("shape,how", [(SHAPES[1], None), (SHAPES[4], None), INDEXED[1]])
def test_lazy_weights_gpu(shape, how):
    ar.case_lazy_weights(DEV, shape, how)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone_gpu(tracking, fuse):
    ar.case_training_untouched(DEV, tracking, fuse)


def test_arguments_gpu():
    ar.case_arguments(DEV)


def test_host_tensor_is_refused_gpu():
    ar.case_host_tensor_refused()


@pytest.mark.parametrize("case", ["a", "b", "c", "border"])
def test_gpu_against_host_double(case):
    ar.case_gpu_against_host_double(DEV, case)
