"""TsdfVolume.mesh (tests/tsdf_mesh_cases.py) — CPU, through the serial host double: the per-cell and per-quad functions are the device
kernels' own (fm_tsdf_mesh.h: tsdf_cell_crossings, tsdf_cell_vertex, tsdf_edge_has_quad, tsdf_quad_cells, over fm_math.h's
tsdf_edge_crosses and tsdf_edge_point), so the restatement parity and its bounds, the closed form of the plane, the closed surfaces'
topology, the count-then-emit edges, the arguments, the PLY file and the exported names are all decided here before a GPU is involved.
What the double does not cover — the launch geometry, the packed scan through LDS, cell_vertex across workgroups on a device — the
`-m gpu` tests do."""

import ctypes

import pytest

import tsdf_mesh_cases as mc
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("name", sorted(mc.SPECS))
def test_mesh_is_the_restatement(name):
    mc.case_restatement("cpu", name)


def test_mesh_min_weight():
    mc.case_restatement("cpu", "wrap", min_weight=3)


def test_plane_is_the_closed_form_bit_for_bit():
    mc.case_plane("cpu")


@pytest.mark.parametrize("kind", sorted(mc.CLOSED))
def test_closed_surface_is_watertight_and_oriented(kind):
    mc.case_closed("cpu", kind)


@pytest.mark.parametrize("kind", ["none", "last", "every", "weights"])
def test_mesh_of_hand_made_volumes(kind):
    mc.case_synthetic("cpu", kind)


@pytest.mark.parametrize("name", ["part", "wrap", "wide"])
def test_two_calls_are_bit_identical(name):
    mc.case_repeatable("cpu", name)


def test_arguments():
    mc.case_arguments("cpu")


def test_c_entries_refuse_on_both_builds():
    if not _lib.LIB_PATH.exists():
        from flowmap_amd.build import build_library

        build_library()
    mc.case_c_entries_refuse(ctypes.CDLL(str(build_host_sim())), "host double")
    mc.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_without_the_double_is_refused():
    try:
        mc.case_host_tensor_refused()
    finally:
        _lib.set_library_for_testing(build_host_sim())


def test_write_ply_with_faces(tmp_path):
    mc.case_ply("cpu", tmp_path)


def test_exported():
    import flowmap_amd

    assert flowmap_amd.TsdfMesh is flowmap_amd.types.TsdfMesh and "TsdfMesh" in flowmap_amd.__all__
    assert callable(flowmap_amd.TsdfVolume.mesh) and callable(flowmap_amd.TsdfMesh.write_ply)
    assert {"fm_tsdf_mesh_count", "fm_tsdf_mesh_emit"} <= set(_lib.SIGNATURES)
