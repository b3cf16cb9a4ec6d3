"""projection.render_views (tests/render_views_cases.py) — CPU, through the serial host double: the per-element functions are the device
kernels' own (fm_math.h: render_splat_at, render_key, render_footprint, depth_consistency_pose), so oracle and reference parity on every
case, the exact properties, the arguments, the scores, the untouched training run and the exported names are all decided here before a
GPU is involved.  What the double does not cover — the atomic minima under contention, the launch geometry — the `-m gpu` tests do."""

import ctypes

import pytest

import render_views_cases as rv
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("name", rv.GOLDEN_CASES)
def test_reference_parity(name):
    rv.case_reference_parity("cpu", name)


@pytest.mark.parametrize("name", sorted(rv.SPECS))
def test_oracle_parity(name):
    rv.case_oracle_parity("cpu", name)


@pytest.mark.parametrize("name", sorted(rv.SPECS))
def test_inputs_are_well_conditioned(name):
    rv.case_well_conditioned(name)


@pytest.mark.parametrize("name", sorted(rv.SPECS))
def test_exact_properties(name):
    rv.case_exact_properties("cpu", name)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tracking", [True, False])
def test_training_is_left_alone(tracking, fuse):
    rv.case_training_untouched("cpu", tracking, fuse)


def test_arguments():
    rv.case_arguments("cpu")


def test_c_entries_refuse_on_both_builds():
    if not _lib.LIB_PATH.exists():
        from flowmap_amd.build import build_library

        build_library()
    rv.case_c_entries_refuse(ctypes.CDLL(str(build_host_sim())), "host double")
    rv.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_without_the_double_is_refused():
    try:
        rv.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


def test_scores():
    rv.case_scores("cpu")


def test_model_render():
    rv.case_model_render("cpu")


def test_exported():
    import flowmap_amd
    from flowmap_amd.model.model import Model

    assert flowmap_amd.RenderedViews is flowmap_amd.types.RenderedViews and "RenderedViews" in flowmap_amd.__all__
    assert "render_views" in flowmap_amd.__all__ and callable(Model.render)
    assert flowmap_amd.render_views is flowmap_amd.model.projection.render_views
