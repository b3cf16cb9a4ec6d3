"""projection.render_views (tests/render_views_cases.py) — on the MI355X: the cases of the CPU module through fm_render_views.hip (fewer
pixels than a wavefront, the scalar path with a partial last quad, the 16-byte path below one tile, several whole tiles, exactly one tile
and one pixel past it, two batch entries, coarser and finer target grids with every radius, free cameras, every way of not being live,
every lane on one of four addresses, equal keys but for the index), plus the kernel against the host build of the same functions and the
peak memory of a call."""

import ctypes

import pytest

import render_views_cases as rv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", rv.GOLDEN_CASES)
def test_reference_parity_gpu(name):
    rv.case_reference_parity(DEV, name)


@pytest.mark.parametrize("name", sorted(rv.SPECS))
def test_oracle_parity_gpu(name):
    rv.case_oracle_parity(DEV, name)


@pytest.mark.parametrize("name", sorted(rv.SPECS))
def test_exact_properties_gpu(name):
    rv.case_exact_properties(DEV, name)


@pytest.mark.parametrize("name", sorted(rv.SPECS))
def test_gpu_against_host_double(name):
    rv.case_gpu_against_host_double(DEV, name)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone_gpu(tracking, fuse):
    rv.case_training_untouched(DEV, tracking, fuse)


def test_arguments_gpu():
    rv.case_arguments(DEV)


def test_c_entry_refuses_gpu():
    from flowmap_amd import _lib

    rv.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_is_refused_gpu():
    rv.case_host_tensor_refused()


@pytest.mark.parametrize("name", ["wide", "odd", "up2"])
def test_peak_memory_gpu(name):
    rv.case_memory(DEV, name)


def test_scores_gpu():
    rv.case_scores(DEV)


def test_model_render_gpu():
    rv.case_model_render(DEV)
