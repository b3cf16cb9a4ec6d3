"""The Procrustes fit alone against a plain fp64 evaluation (tests/procrustes_geometry_cases.py) — CPU, host double.  The host double
loops where the kernels launch, so geometry edges cannot break it: what this module proves is that the cases and their reference are
right, that the input conditions hold (the fp32 reference itself is within the gates of the fp64 truth on every case, nothing masked;
no dense sample next to a coordinate that decides its tiles), that the constants the lists straddle are the sources', that every call
sequence reaches the backward form it claims (the operator library's counters), and that the arithmetic shared with the kernels
(fm_math.h, fm_pose.h) and the Python layer are right.  tests/test_gpu_procrustes_geometry.py runs the same lists where the launch
geometry exists."""

import pytest

import procrustes_geometry_cases as pg
from flowmap_amd import _lib
from helpers import build_host_sim

DEV = "cpu"


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


def test_constants():
    pg.case_constants()


@pytest.mark.parametrize("spec", pg.ALL_CASES, ids=pg.spec_id)
def test_input_conditions(spec):
    pg.check_conditions(spec)


@pytest.mark.parametrize("spec", pg.SPARSE_CASES, ids=pg.spec_id)
def test_sparse(spec):
    pg.case_sparse(DEV, spec)


@pytest.mark.parametrize("spec", pg.ATOMIC_ONLY_CASES, ids=pg.spec_id)
def test_atomic_only(spec):
    pg.case_atomic_only(DEV, spec)


@pytest.mark.parametrize("spec", pg.ALL_DENSE, ids=pg.spec_id)
def test_dense(spec):
    pg.case_dense(DEV, spec)


@pytest.mark.parametrize("spec", pg.SURFACE_CASES, ids=pg.spec_id)
def test_surfaces(spec):
    pg.case_surfaces(DEV, spec)


@pytest.mark.parametrize("spec", pg.REPEAT_CASES, ids=pg.spec_id)
def test_repeat(spec):
    pg.case_repeat(DEV, spec)


@pytest.mark.parametrize("spec", pg.REUSE_CASES, ids=pg.spec_id)
def test_reuse(spec):
    pg.case_reuse(DEV, spec)


@pytest.mark.parametrize("spec", pg.STATS_CASES, ids=pg.spec_id)
def test_stats(spec):
    pg.case_stats(DEV, spec)
