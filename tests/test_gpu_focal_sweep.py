"""IntrinsicsSoftmin.residuals (tests/focal_sweep_cases.py) — on the MI355X: the cases of the CPU module through fm_focal_sweep.hip (fewer
points than a wavefront, one short of a wave, one past a round of the workgroup, several rounds plus one, more candidates than a wave in
the curve kernel, two batch entries, skipped taps), plus the kernel against the host build of the same functions element for element."""

import pytest

import focal_sweep_cases as fs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", fs.GOLDEN_CASES)
def test_reference_parity_gpu(name):
    fs.case_reference_parity(DEV, name)


@pytest.mark.parametrize("name", sorted(fs.SPECS))
def test_oracle_parity_every_window_gpu(name):
    fs.case_oracle_parity(DEV, name)


@pytest.mark.parametrize("name", ["tiny1", "tiny3", "odd", "ref200", "two"])
def test_agrees_with_the_training_path_gpu(name):
    fs.case_training_path(DEV, name)


@pytest.mark.parametrize("name", sorted(fs.SPECS))
def test_reproducible_and_window_independent_gpu(name):
    fs.case_reproducible(DEV, name)


@pytest.mark.parametrize("name", fs.GOLDEN_CASES)
def test_gpu_against_host_double(name):
    fs.case_gpu_against_host_double(DEV, name)


@pytest.mark.parametrize("sensitivity", [100.0, 0.0])
@pytest.mark.parametrize("name", ["odd", "two"])
def test_lazy_weights_gpu(name, sensitivity):
    fs.case_lazy_weights(DEV, name, sensitivity)


@pytest.mark.parametrize("regressed", [False, True])
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone_gpu(tracking, fuse, regressed):
    fs.case_training_untouched(DEV, tracking, fuse, regressed)


def test_arguments_gpu():
    fs.case_arguments(DEV)


def test_no_global_step_and_no_state_gpu():
    fs.case_state_untouched(DEV)


def test_host_tensor_is_refused_gpu():
    fs.case_host_tensor_refused()
