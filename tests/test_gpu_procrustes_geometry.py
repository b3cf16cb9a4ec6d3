"""The Procrustes fit alone against a plain fp64 evaluation (tests/procrustes_geometry_cases.py) — on the GPU: the same lists as the CPU
module, where they reach the wave, the 256- and 1024-thread strides, SLOTS 1..4 and the second gather trip of the one-launch backward,
the election of the last block per pair and of the last pair with the self-cleaning workspace, iters = 8, both in-fit pose chains next
to their 64 chunks, the second block of the 64-thread per-pair kernels, the groups of the repeated-batch scatter, and — for the tiled
dense kernels — odd widths, partial tiles, the XCD dealing with its padded grid, chunk-wise sorted and empty tile lists and several tap
batches.  Nothing here hands a kernel an index it could fault on.  The worst figure per family is printed when the module ends."""

import pytest

import procrustes_geometry_cases as pg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True, scope="module")
def worst_figures():
    yield
    pg.print_figures()


@pytest.mark.parametrize("spec", pg.SPARSE_CASES, ids=pg.spec_id)
def test_sparse_gpu(spec):
    pg.case_sparse(DEV, spec)


@pytest.mark.parametrize("spec", pg.ATOMIC_ONLY_CASES, ids=pg.spec_id)
def test_atomic_only_gpu(spec):
    pg.case_atomic_only(DEV, spec)


@pytest.mark.parametrize("spec", pg.ALL_DENSE, ids=pg.spec_id)
def test_dense_gpu(spec):
    pg.case_dense(DEV, spec)


@pytest.mark.parametrize("spec", pg.SURFACE_CASES, ids=pg.spec_id)
def test_surfaces_gpu(spec):
    pg.case_surfaces(DEV, spec)


@pytest.mark.parametrize("spec", pg.REPEAT_CASES, ids=pg.spec_id)
def test_repeat_gpu(spec):
    pg.case_repeat(DEV, spec)


@pytest.mark.parametrize("spec", pg.REUSE_CASES, ids=pg.spec_id)
def test_reuse_gpu(spec):
    pg.case_reuse(DEV, spec)


@pytest.mark.parametrize("spec", pg.STATS_CASES, ids=pg.spec_id)
def test_stats_gpu(spec):
    pg.case_stats(DEV, spec)
