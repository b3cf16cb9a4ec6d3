"""IntrinsicsSoftmin.residuals (tests/focal_sweep_cases.py) — CPU, through the serial host double: the per-correspondence and per-pair
functions are the device kernel's own (fm_math.h: corr_load_with, moments_add, softmin_term; fm_pose.h: pose_solve_one), so reference and
oracle parity on every shape and window, the agreement with the training path, reproducibility, lazy weights, the arguments and the
untouched training run are all decided here before a GPU is involved."""

import pytest

import focal_sweep_cases as fs
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("name", fs.GOLDEN_CASES)
def test_reference_parity(name):
    fs.case_reference_parity("cpu", name)


@pytest.mark.parametrize("name", sorted(fs.SPECS))
def test_oracle_parity_every_window(name):
    fs.case_oracle_parity("cpu", name)


@pytest.mark.parametrize("name", ["tiny1", "tiny3", "odd", "ref200", "two"])
def test_agrees_with_the_training_path(name):
    fs.case_training_path("cpu", name)


@pytest.mark.parametrize("name", sorted(fs.SPECS))
def test_reproducible_and_window_independent(name):
    fs.case_reproducible("cpu", name)


@pytest.mark.parametrize("sensitivity", [100.0, 0.0])
@pytest.mark.parametrize("name", ["odd", "two"])
def test_lazy_weights(name, sensitivity):
    fs.case_lazy_weights("cpu", name, sensitivity)


@pytest.mark.parametrize("regressed", [False, True])
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone(tracking, fuse, regressed):
    fs.case_training_untouched("cpu", tracking, fuse, regressed)


def test_arguments():
    fs.case_arguments("cpu")


def test_no_global_step_and_no_state():
    fs.case_state_untouched("cpu")


def test_host_tensor_without_the_double_is_refused():
    try:
        fs.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


def test_exported():
    import flowmap_amd

    assert flowmap_amd.FocalSweep is flowmap_amd.types.FocalSweep and "FocalSweep" in flowmap_amd.__all__
