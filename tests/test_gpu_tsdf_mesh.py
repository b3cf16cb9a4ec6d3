"""TsdfVolume.mesh (tests/tsdf_mesh_cases.py) — on the MI355X: the cases of the CPU module through the three mesh kernels of
fm_tsdf_volume.hip (fewer voxels than a wavefront, exactly one workgroup and one voxel more with no cell at all, rows that drift and wrap
through the wavefronts, a partial last workgroup, a thousand workgroups), the plane against the closed form AND the host double, the sphere
and the torus watertight, oriented and bit-equal to the host double, vertices and quads in the last workgroup only, none at all, in every
cell, two calls against each other, the PLY file and the peak memory."""

import ctypes

import pytest

import tsdf_mesh_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", sorted(mc.SPECS))
def test_mesh_is_the_restatement_gpu(name):
    mc.case_restatement(DEV, name)


def test_mesh_min_weight_gpu():
    mc.case_restatement(DEV, "wrap", min_weight=3)


def test_plane_is_the_closed_form_and_the_host_double_bit_for_bit_gpu():
    mc.case_plane(DEV, against_host=True)


@pytest.mark.parametrize("kind", sorted(mc.CLOSED))
def test_closed_surface_is_watertight_and_oriented_gpu(kind):
    mc.case_closed(DEV, kind, against_host=True)


@pytest.mark.parametrize("kind", ["none", "last", "every", "weights"])
def test_mesh_of_hand_made_volumes_gpu(kind):
    mc.case_synthetic(DEV, kind)


@pytest.mark.parametrize("name", ["part", "wrap", "wide"])
def test_two_calls_are_bit_identical_gpu(name):
    mc.case_repeatable(DEV, name)


@pytest.mark.parametrize("name", ["wrap", "vec", "sphere"])
def test_gpu_against_host_double(name):
    mc.case_gpu_against_host_double(DEV, name)


def test_arguments_gpu():
    mc.case_arguments(DEV)


def test_c_entry_refuses_gpu():
    from flowmap_amd import _lib

    mc.case_c_entries_refuse(ctypes.CDLL(str(_lib.LIB_PATH)), "device build")


def test_host_tensor_is_refused_gpu():
    mc.case_host_tensor_refused()


def test_write_ply_with_faces_gpu(tmp_path):
    mc.case_ply(DEV, tmp_path)


def test_peak_memory_gpu():
    mc.case_memory(DEV, "wide")
