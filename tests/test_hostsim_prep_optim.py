"""Data preparation (mask, fused post-processing, resize + crop) and the Adam / fill entry points against plain fp64 evaluations
(tests/prep_optim_cases.py) — CPU, host double: the per-element arithmetic of fm_math.h and the Python layer.  The host double
runs plain loops, so nothing here says anything about launch geometry; tests/test_gpu_prep_optim.py does."""

import pytest

import prep_optim_cases as po
from flowmap_amd import _lib
from helpers import build_host_sim

DEV = "cpu"


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("kernel", ("host", "capturable"))
@pytest.mark.parametrize("count", po.COUNTS)
def test_adam_count(count, kernel):
    po.case_adam_count(DEV, count, kernel)


@pytest.mark.parametrize("kernel", ("host", "capturable"))
@pytest.mark.parametrize("count", po.ALIGN_COUNTS)
def test_adam_alignment(count, kernel):
    po.case_adam_alignment(DEV, count, kernel)


@pytest.mark.parametrize("kernel", ("host", "capturable"))
@pytest.mark.parametrize("count", po.ZERO_COUNTS)
def test_adam_zero_patterns(count, kernel):
    po.case_adam_zero_patterns(DEV, count, kernel)


@pytest.mark.parametrize("name,changes", po.MAGNITUDE_HYPERS, ids=[n for n, _ in po.MAGNITUDE_HYPERS])
@pytest.mark.parametrize("step", po.STEPS)
def test_adam_magnitudes(step, name, changes):
    po.case_adam_magnitudes(DEV, step, name, changes)


@pytest.mark.parametrize("count", po.TRAJECTORY_COUNTS)
def test_adam_trajectory(count):
    po.case_adam_trajectory(DEV, count)


def test_adam_capturable_step_tensor():
    po.case_adam_capturable_step_tensor(DEV)


@pytest.mark.parametrize("length", po.ELEMENT_LENGTHS)
def test_adam_elements(length):
    po.case_adam_elements(DEV, length)


@pytest.mark.parametrize("blocks", po.FILL_BLOCKS)
@pytest.mark.parametrize("count", po.COUNTS)
def test_fill_zero(count, blocks):
    po.case_fill_zero(DEV, count, blocks)


def test_fill_zero_misaligned():
    po.case_fill_zero_misaligned(DEV)


def test_adam_eps():
    po.case_adam_eps(DEV)


def test_adam_eps_zero_is_one_answer():
    po.case_adam_eps_zero_is_one_answer(DEV)


@pytest.mark.parametrize("cfg", po.RESIZE_CASES, ids=po.resize_id)
def test_resize(cfg):
    po.case_resize(DEV, cfg)


def test_resize_many_planes():
    po.case_resize_many_planes(DEV)


@pytest.mark.parametrize("cfg", po.MASK_CASES, ids=po.mask_id)
def test_mask(cfg):
    po.case_mask(DEV, cfg)


@pytest.mark.parametrize("cfg", po.POST_CASES, ids=po.post_id)
def test_postprocess(cfg):
    po.case_postprocess(DEV, cfg)


@pytest.mark.parametrize("cfg", po.NONFINITE_CASES, ids=lambda c: f"b{c[0]}-f{c[1]}-{c[2][0]}x{c[2][1]}-to-{c[3][0]}x{c[3][1]}")
def test_mask_nonfinite(cfg):
    po.case_mask_nonfinite(DEV, cfg)


@pytest.mark.parametrize("cfg", po.NONFINITE_CASES, ids=lambda c: f"b{c[0]}-f{c[1]}-{c[2][0]}x{c[2][1]}-to-{c[3][0]}x{c[3][1]}")
def test_postprocess_nonfinite(cfg):
    po.case_postprocess_nonfinite(DEV, cfg)


def test_pair_limit():
    po.case_pair_limit(DEV)
