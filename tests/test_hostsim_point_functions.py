"""The explicit-point function entry points (unproject, reproject / project, the bilinear sampler, Mapping.forward, align_rigid,
world_point_cloud) against plain fp64 evaluations (tests/point_function_cases.py) — CPU, host double: the per-element arithmetic of
fm_math.h / fm_pose.h and the Python layer (group slices, empty point sets, misaligned views).  The host double runs plain loops,
so nothing here says anything about launch geometry; tests/test_gpu_point_functions.py does.  The refusal tests at the end run
against the device build of the library, which loads without a GPU and refuses before its first HIP call."""

import pytest

import point_function_cases as pf
from flowmap_amd import _lib
from helpers import build_host_sim

DEV = "cpu"


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_unproject(cfg):
    pf.case_unproject(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_unproject_abi(cfg):
    pf.case_unproject_abi(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_reproject(cfg):
    pf.case_reproject(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_project(cfg):
    pf.case_project(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_flow_positions(cfg):
    pf.case_flow_positions(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_reproject_abi(cfg):
    pf.case_reproject_abi(DEV, cfg)


def test_projection_edges():
    pf.case_projection_edges(DEV)


@pytest.mark.parametrize("c", pf.CHANNELS)
@pytest.mark.parametrize("cfg", pf.shapes(pf.SAMPLE_POINTS), ids=pf.shape_id)
def test_bilinear(cfg, c):
    pf.case_bilinear(DEV, (*cfg, c))


def test_bilinear_census():
    pf.case_bilinear_census(DEV)


@pytest.mark.parametrize("points", (257, 1025))
def test_sampler_edges(points):
    pf.case_sampler_edges(DEV, points)


@pytest.mark.parametrize("kind", pf.KINDS)
@pytest.mark.parametrize("n", pf.POINTS)
def test_mapping(n, kind):
    pf.case_mapping(DEV, n, kind)


@pytest.mark.parametrize("cfg", pf.shapes(pf.RIGID_POINTS), ids=pf.shape_id)
def test_align_rigid(cfg):
    pf.case_align_rigid(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.RIGID_POINTS), ids=pf.shape_id)
def test_rigid_stats_abi(cfg):
    pf.case_rigid_stats_abi(DEV, cfg)


@pytest.mark.parametrize("cfg", pf.shapes(pf.POINTS), ids=pf.shape_id)
def test_sum_census(cfg):
    pf.case_sum_census(DEV, cfg)


@pytest.mark.parametrize("frames", pf.WORLD_FRAMES)
@pytest.mark.parametrize("hw", pf.WORLD_SHAPES, ids=pf.shape_id)
def test_world_points(hw, frames):
    pf.case_world_points(DEV, (frames, *hw))


@pytest.mark.parametrize("n", pf.OVER_POINTS)
@pytest.mark.parametrize("g", pf.OVER_GROUPS)
def test_over_groups(g, n):
    pf.case_over_groups(DEV, g, n)


def test_over_groups_other_operators():
    pf.case_over_groups_other_operators(DEV)


@pytest.mark.parametrize("offset", (1, 3))
def test_misaligned_views(offset):
    pf.case_misaligned_views(DEV, offset)


def test_empty():
    pf.case_empty(DEV)


def test_misaligned_refused_by_the_host_double():
    pf.case_misaligned_refused(double=True)


def test_misaligned_refused_by_the_library():
    pf.case_misaligned_refused(double=False)


def test_group_limit_refused_by_the_library():
    pf.case_group_limit_refused()
