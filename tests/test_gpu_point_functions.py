"""The explicit-point function kernels of fm_points.hip against plain fp64 evaluations (tests/point_function_cases.py) — on the
GPU: the same lists as the CPU module, where they enter the grid-stride loops, the second block, the inter-block fp64 atomics, the
group offsets and the finalize launches over many groups, plus the sizes at which the block caps bind (``capped``) and one
1080 x 1920 frame (FLOWMAP_SKIP_FULL_SIZE=1 skips that).  No case hands a kernel a misaligned pointer: the raw refusals are tested
on the CPU, against the same library."""

import pytest

import point_function_cases as pf
from prep_optim_cases import full_size

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_unproject_gpu(cfg):
    pf.case_unproject(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes((), pf.POINTS_CAPPED), ids=pf.shape_id)
def test_unproject_capped_gpu(cfg):
    pf.case_unproject(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_unproject_abi_gpu(cfg):
    pf.case_unproject_abi(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes((), pf.POINTS_CAPPED), ids=pf.shape_id)
def test_unproject_abi_capped_gpu(cfg):
    pf.case_unproject_abi(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_reproject_gpu(cfg):
    pf.case_reproject(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes((), pf.POINTS_CAPPED), ids=pf.shape_id)
def test_reproject_capped_gpu(cfg):
    pf.case_reproject(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_project_gpu(cfg):
    pf.case_project(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_flow_positions_gpu(cfg):
    pf.case_flow_positions(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_reproject_abi_gpu(cfg):
    pf.case_reproject_abi(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes((), pf.POINTS_CAPPED), ids=pf.shape_id)
def test_reproject_abi_capped_gpu(cfg):
    pf.case_reproject_abi(DEV, cfg)


def test_projection_edges_gpu():
    pf.case_projection_edges(DEV)


@pytest.mark.parametrize("c", pf.CHANNELS)
@pytest.mark.parametrize("cfg", pf.shapes(pf.SAMPLE_POINTS), ids=pf.shape_id)
def test_bilinear_gpu(cfg, c):
    pf.case_bilinear(DEV, (*cfg, c))


@pytest.mark.parametrize("c", pf.CHANNELS)
@pytest.mark.parametrize("cfg", pf.shapes((), pf.SAMPLE_POINTS_CAPPED), ids=pf.shape_id)
def test_bilinear_capped_gpu(cfg, c):
    pf.case_bilinear(DEV, (*cfg, c))


def test_bilinear_census_gpu():
    pf.case_bilinear_census(DEV)


@pytest.mark.parametrize("points", (257, 1025))
def test_sampler_edges_gpu(points):
    pf.case_sampler_edges(DEV, points)


@pytest.mark.parametrize("kind", pf.KINDS)
@pytest.mark.parametrize("n", pf.POINTS)
def test_mapping_gpu(n, kind):
    pf.case_mapping(DEV, n, kind)


@pytest.mark.parametrize("kind", pf.KINDS)
@pytest.mark.parametrize("n", pf.POINTS_CAPPED)
def test_mapping_capped_gpu(n, kind):
    pf.case_mapping(DEV, n, kind)


@pytest.mark.parametrize("cfg", pf.shapes(pf.RIGID_POINTS), ids=pf.shape_id)
def test_align_rigid_gpu(cfg):
    pf.case_align_rigid(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes((), pf.RIGID_POINTS_CAPPED), ids=pf.shape_id)
def test_align_rigid_capped_gpu(cfg):
    pf.case_align_rigid(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.RIGID_POINTS), ids=pf.shape_id)
def test_rigid_stats_abi_gpu(cfg):
    pf.case_rigid_stats_abi(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes((), pf.RIGID_POINTS_CAPPED), ids=pf.shape_id)
def test_rigid_stats_abi_capped_gpu(cfg):
    pf.case_rigid_stats_abi(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_sum_census_gpu(cfg):
    pf.case_sum_census(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes((), pf.POINTS_CAPPED), ids=pf.shape_id)
def test_sum_census_capped_gpu(cfg):
    pf.case_sum_census(DEV, cfg)


@pytest.mark.parametrize("frames", pf.WORLD_FRAMES)
@pytest.mark.parametrize("hw", pf.WORLD_SHAPES, ids=pf.shape_id)
def test_world_points_gpu(hw, frames):
    pf.case_world_points(DEV, (frames, *hw))


@pytest.mark.parametrize("cfg", full_size(pf.WORLD_FULL_SIZE), ids=pf.shape_id)
def test_world_points_full_size_gpu(cfg):
    pf.case_world_points(DEV, cfg, warn=True)


@pytest.mark.parametrize("n", pf.OVER_POINTS)
@pytest.mark.parametrize("g", pf.OVER_GROUPS)
def test_over_groups_gpu(g, n):
    pf.case_over_groups(DEV, g, n)


def test_over_groups_other_operators_gpu():
    pf.case_over_groups_other_operators(DEV)


@pytest.mark.parametrize("offset", (1, 3))
def test_misaligned_views_gpu(offset):
    pf.case_misaligned_views(DEV, offset)


def test_empty_gpu():
    pf.case_empty(DEV)
