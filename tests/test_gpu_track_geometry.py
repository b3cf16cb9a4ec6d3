"""The fused tracking loss alone against a plain fp64 evaluation (tests/track_geometry_cases.py) — on the GPU: the same lists as the CPU
module, where they reach the second point of a lane, idle point groups, the odd tail of a register tile, the two-deep target prefetch,
the XCD dealing and the padded grid of track_pairs, the 256-thread stride of track_reduce and the second block of the 64-thread frame
kernels.  Nothing here hands a kernel an index it could fault on: refusals are asserted on the CPU."""

import pytest

import track_geometry_cases as tg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("spec", tg.GEOMETRY_CASES, ids=tg.spec_id)
def test_geometry_gpu(spec):
    tg.case_geometry(DEV, spec)


@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_forward_only_gpu(spec):
    tg.case_forward_only(DEV, spec)


@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_backward_paths_gpu(spec):
    tg.case_backward_paths(DEV, spec)


@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_atomic_scatter_gpu(spec):
    tg.case_atomic_scatter(DEV, spec)


@pytest.mark.parametrize("spec", tg.TAP_CASES, ids=tg.spec_id)
def test_tap_image_gpu(spec):
    tg.case_tap_image(DEV, spec)


@pytest.mark.parametrize("spec", tg.TAP_CASES, ids=tg.spec_id)
def test_tap_gradient_gpu(spec):
    tg.case_tap_gradient(DEV, spec)


@pytest.mark.parametrize("parts", (2, 3))
@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_sharded_gpu(spec, parts):
    tg.case_sharded(DEV, spec, parts)


@pytest.mark.parametrize("parts", (2, 3))
@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_sharded_flags_gpu(spec, parts):
    tg.case_sharded_flags(DEV, spec, parts)


@pytest.mark.parametrize("spec", tg.PATH_CASES, ids=tg.spec_id)
def test_unfused_entry_points_gpu(spec):
    tg.case_unfused_entry_points(DEV, spec)


@pytest.mark.parametrize("spec", (tg.MIXED, tg.TAP_EDGES), ids=tg.spec_id)
def test_step_tap_exchange_gpu(spec):
    tg.case_step_tap_exchange(DEV, spec)


@pytest.mark.parametrize("spec", (tg.MIXED, tg.TAP_EDGES), ids=tg.spec_id)
def test_step_in_pass_adam_gpu(spec):
    tg.case_step_in_pass_adam(DEV, spec)
