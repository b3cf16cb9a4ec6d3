"""The fused tracking loss alone against a plain fp64 evaluation (tests/track_geometry_cases.py) — CPU, host double.  The host double
loops where the kernels launch, so geometry edges cannot break it: what this module proves is that the cases and their reference are
right, that the input conditions hold (the share of points the margin rule altered is printed per case and is at most 1 %), and that the
per-residual, per-source and per-frame arithmetic shared with the kernels (fm_pose.h) and the Python layer are right.
tests/test_gpu_track_geometry.py runs the same lists where the launch geometry exists."""

import pytest

import track_geometry_cases as tg
from flowmap_amd import _lib
from helpers import build_host_sim

DEV = "cpu"


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


def test_constants():
    tg.case_constants()


@pytest.mark.parametrize("spec", tg.GEOMETRY_CASES, ids=tg.spec_id)
def test_input_conditions(spec):
    tg.check_conditions(tg.make_case(spec))


@pytest.mark.parametrize("spec", tg.GEOMETRY_CASES, ids=tg.spec_id)
def test_geometry(spec):
    tg.case_geometry(DEV, spec)


@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_forward_only(spec):
    tg.case_forward_only(DEV, spec)


@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_backward_paths(spec):
    tg.case_backward_paths(DEV, spec)


@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_atomic_scatter(spec):
    tg.case_atomic_scatter(DEV, spec)


@pytest.mark.parametrize("spec", tg.TAP_CASES, ids=tg.spec_id)
def test_tap_image(spec):
    tg.case_tap_image(DEV, spec)


@pytest.mark.parametrize("spec", tg.TAP_CASES, ids=tg.spec_id)
def test_tap_gradient(spec):
    tg.case_tap_gradient(DEV, spec)


@pytest.mark.parametrize("parts", (2, 3))
@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_sharded(spec, parts):
    tg.case_sharded(DEV, spec, parts)


@pytest.mark.parametrize("parts", (2, 3))
@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_sharded_flags(spec, parts):
    tg.case_sharded_flags(DEV, spec, parts)


@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_unfused_entry_points(spec):
    tg.case_unfused_entry_points(DEV, spec)


@pytest.mark.parametrize("spec", (tg.MIXED, tg.TAP_EDGES), ids=tg.spec_id)
def test_step_tap_exchange(spec):
    tg.case_step_tap_exchange(DEV, spec)


@pytest.mark.parametrize("spec", (tg.MIXED, tg.TAP_EDGES), ids=tg.spec_id)
def test_step_in_pass_adam(spec):
    tg.case_step_in_pass_adam(DEV, spec)


def test_refusals():
    """Arguments that would launch out of range are the host layer's to refuse: asserted here, on the CPU, only."""
    tg.case_refusals(DEV)
