"""ExtrinsicsProcrustes.residuals (tests/alignment_residual_cases.py) — CPU, through the serial host double: the per-element functions are
the device kernel's own (fm_math.h: corr_load_with, alignment_offset), so reference parity on both sources, the border clamp, the
convention, the sums, the windows, lazy weights, the arguments and the untouched training run are all decided here before a GPU is
involved."""

import pytest

import alignment_residual_cases as ar
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


# (batch, frames, h, w, a K per frame)
SHAPES = [(1, 2, 5, 7, False), (1, 5, 17, 23, True), (1, 6, 24, 32, False), (1, 4, 64, 128, True), (1, 2, 25, 41, False), (1, 2, 31, 33, True), (2, 4, 9, 12, True)]
# (shape, how the indices are drawn)
INDEXED = [(SHAPES[1], "three"), (SHAPES[0], "fifty"), (SHAPES[2], "tile+1"), (SHAPES[3], "linspace")]


@pytest.mark.parametrize("case", ["a", "b", "c", "border"])
def test_reference_parity(case):
    ar.case_reference_parity("cpu", case)


def test_border_clamp():
    ar.case_border("cpu")


@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("shape", SHAPES[2:6])
def test_oracle_parity(shape, fit):
    ar.case_oracle_parity("cpu", shape, None, fit)


@pytest.mark.parametrize("shape,how", INDEXED)
def test_oracle_parity_on_indices(shape, how):
    ar.case_oracle_parity("cpu", shape, how, how != "three")


@pytest.mark.parametrize("shape,how", [(SHAPES[1], None), (SHAPES[6], None), (SHAPES[4], None)] + INDEXED[1:])
def test_convention_by_the_fit(shape, how):
    ar.case_convention("cpu", shape, how)


@pytest.mark.parametrize("shape", SHAPES)
def test_sums_repeats_and_windows(shape):
    ar.case_sums("cpu", shape)


@pytest.mark.parametrize("shape,how", INDEXED)
def test_sums_repeats_and_windows_on_indices(shape, how):
    ar.case_sums("cpu", shape, how)


@pytest.mark.parametrize("shape,how", [(SHAPES[1], None), (SHAPES[4], None), INDEXED[1]])
def test_lazy_weights(shape, how):
    ar.case_lazy_weights("cpu", shape, how)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone(tracking, fuse):
    ar.case_training_untouched("cpu", tracking, fuse)


def test_arguments():
    ar.case_arguments("cpu")


def test_host_tensor_without_the_double_is_refused():
    try:
        ar.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


def test_exported():
    import flowmap_amd

    assert flowmap_amd.AlignmentResiduals is flowmap_amd.types.AlignmentResiduals and "AlignmentResiduals" in flowmap_amd.__all__
