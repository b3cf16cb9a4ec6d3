"""Data preparation (mask, fused post-processing, resize + crop) and the Adam / fill kernels against plain fp64 evaluations
(tests/prep_optim_cases.py) — on the GPU: the same lists as the CPU module, where they enter the grid-stride loops, the second
block column, the vector bodies and their tails, plus the production sizes (FLOWMAP_SKIP_FULL_SIZE=1 skips those)."""

import pytest

import prep_optim_cases as po

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("kernel", ("host", "capturable"))
@pytest.mark.parametrize("count", po.COUNTS)
def test_adam_count_gpu(count, kernel):
    po.case_adam_count(DEV, count, kernel)


@pytest.mark.parametrize("count", po.full_size(*po.COUNTS_FULL_SIZE))
def test_adam_full_size_gpu(count):
    po.case_adam_full_size(DEV, count)


@pytest.mark.parametrize("kernel", ("host", "capturable"))
@pytest.mark.parametrize("count", po.ALIGN_COUNTS)
def test_adam_alignment_gpu(count, kernel):
    po.case_adam_alignment(DEV, count, kernel)


@pytest.mark.parametrize("kernel", ("host", "capturable"))
@pytest.mark.parametrize("count", po.ZERO_COUNTS)
def test_adam_zero_patterns_gpu(count, kernel):
    po.case_adam_zero_patterns(DEV, count, kernel)


@pytest.mark.parametrize("name,changes", po.MAGNITUDE_HYPERS, ids=[n for n, _ in po.MAGNITUDE_HYPERS])
@pytest.mark.parametrize("step", po.STEPS)
def test_adam_magnitudes_gpu(step, name, changes):
    po.case_adam_magnitudes(DEV, step, name, changes)


@pytest.mark.parametrize("count", po.TRAJECTORY_COUNTS)
def test_adam_trajectory_gpu(count):
    po.case_adam_trajectory(DEV, count)


def test_adam_capturable_step_tensor_gpu():
    po.case_adam_capturable_step_tensor(DEV)


@pytest.mark.parametrize("length", po.ELEMENT_LENGTHS)
def test_adam_elements_gpu(length):
    po.case_adam_elements(DEV, length)


@pytest.mark.parametrize("blocks", po.FILL_BLOCKS)
@pytest.mark.parametrize("count", po.COUNTS)
def test_fill_zero_gpu(count, blocks):
    po.case_fill_zero(DEV, count, blocks)


@pytest.mark.parametrize("count", po.full_size(*po.COUNTS_FULL_SIZE))
def test_fill_zero_full_size_gpu(count):
    po.case_fill_zero(DEV, count, 64)


def test_fill_zero_misaligned_gpu():
    po.case_fill_zero_misaligned(DEV)


def test_adam_eps_gpu():
    po.case_adam_eps(DEV)


def test_adam_eps_zero_is_one_answer_gpu():
    po.case_adam_eps_zero_is_one_answer(DEV)


@pytest.mark.parametrize("cfg", po.RESIZE_CASES, ids=po.resize_id)
def test_resize_gpu(cfg):
    po.case_resize(DEV, cfg)


def test_resize_many_planes_gpu():
    po.case_resize_many_planes(DEV)


@pytest.mark.parametrize("cfg", po.full_size(*po.RESIZE_FULL_SIZE), ids=lambda c: f"{c[0]}-{c[2][0]}x{c[2][1]}-x{c[3]}")
def test_resize_full_size_gpu(cfg):
    po.case_resize_full_size(DEV, cfg)


@pytest.mark.parametrize("cfg", po.MASK_CASES, ids=po.mask_id)
def test_mask_gpu(cfg):
    po.case_mask(DEV, cfg)


@pytest.mark.parametrize("cfg", po.full_size(*po.MASK_FULL_SIZE), ids=po.mask_id)
def test_mask_full_size_gpu(cfg):
    po.case_mask(DEV, cfg, warn=True)


@pytest.mark.parametrize("cfg", po.POST_CASES, ids=po.post_id)
def test_postprocess_gpu(cfg):
    po.case_postprocess(DEV, cfg)


@pytest.mark.parametrize("cfg", po.full_size(*po.POST_FULL_SIZE), ids=po.post_id)
def test_postprocess_full_size_gpu(cfg):
    po.case_postprocess(DEV, cfg, warn=True)


@pytest.mark.parametrize("cfg", po.NONFINITE_CASES, ids=lambda c: f"b{c[0]}-f{c[1]}-{c[2][0]}x{c[2][1]}-to-{c[3][0]}x{c[3][1]}")
def test_mask_nonfinite_gpu(cfg):
    po.case_mask_nonfinite(DEV, cfg)


@pytest.mark.parametrize("cfg", po.NONFINITE_CASES, ids=lambda c: f"b{c[0]}-f{c[1]}-{c[2][0]}x{c[2][1]}-to-{c[3][0]}x{c[3][1]}")
def test_postprocess_nonfinite_gpu(cfg):
    po.case_postprocess_nonfinite(DEV, cfg)


def test_pair_limit_gpu():
    po.case_pair_limit(DEV)
