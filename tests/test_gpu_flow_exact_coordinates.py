"""The fused flow pass with its pixel coordinates free of divisions — (row, item in the row) walked with integer adds, the pixel centres
from a host reciprocal with one correction step (item_walk, pixel_center_recip: fm_math.h) — against the outputs recorded from the commit
before, which divided per quad (tests/golden/flow_exact_coordinates_parent_bits.npz and ..._multi.npz,
tools/make_golden_flow_exact_coordinates.py; shapes: tests/flow_exact_coordinates_cases.py).  Three frames per case; the three mappings,
the formats each shape admits, with and without gradients.

* Frames of one workgroup, at the row lengths where the walk changes its behaviour (1, 2, 255, 256, 257 quads per row; one pixel per item):
  loss, dL/ddepth, dL/dT, dL/dK and the 13 sums are the recorded BITS.
* A frame of two workgroups, and one wider than the reciprocal form's proven range (the instances that divide): dL/ddepth is the recorded
  bits; the sums meet through fp64 atomics, so they and what finalize derives from them are held to the 1e-6 relative
  include/flowmap_hip.h states for them."""

import json
from pathlib import Path

import numpy as np
import pytest
import torch

import flow_exact_coordinates_cases as ec
import flow_frame_constants_cases as fc
from conftest import assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN_DIR = Path(__file__).resolve().parent / "golden"
GOLDEN = {"one": GOLDEN_DIR / "flow_exact_coordinates_parent_bits.npz", "multi": GOLDEN_DIR / "flow_exact_coordinates_parent_bits_multi.npz"}


@pytest.fixture(scope="module")
def golden():
    files = {}
    for which, path in GOLDEN.items():
        data = np.load(path)
        assert int(data["seed"]) == fc.SEED
        files[which] = (data, json.loads(str(data["aliases"])))

    def get(shape, name):
        data, aliases = files["one" if shape in ec.ONE_WORKGROUP_SHAPES else "multi"]
        return torch.from_numpy(data[aliases.get(name, name)])

    return get


@pytest.fixture(scope="module")
def problems(golden):
    made = {}

    def get(shape):
        if shape not in made:
            name = fc.shape_name(shape)
            prob = fc.Problem(shape, DEV, small={n: golden(shape, f"{name}.input.{n}") for n in fc.SMALL})
            assert fc.checksum(prob.host) == int(golden(shape, f"{name}.input.checksum")), "this host generates other inputs than the recording one"
            made[shape] = prob
        return made[shape]

    return get


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "loss_only"])
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("shape,fmt", [(shape, fmt) for shape in ec.ONE_WORKGROUP_SHAPES for fmt in fc.formats_of(shape)],
                         ids=lambda v: v if isinstance(v, str) else fc.shape_name(v))
def test_one_workgroup_frames_keep_the_parents_bits(golden, problems, shape, kind, fmt, grad):
    out, _ = problems(shape).run(kind, fmt, grad)
    assert set(out) == set(fc.OUTPUTS) - (set() if grad else {"grad_depth"})
    for name, value in out.items():
        want = golden(shape, fc.key(shape, kind, fmt, grad, name))
        assert torch.equal(value, want), (name, float((value.double() - want.double()).abs().max()))


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "loss_only"])
@pytest.mark.parametrize("fmt", fc.FORMATS)
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("shape", ec.ATOMIC_SHAPES, ids=fc.shape_name)
def test_frames_of_several_workgroups(golden, problems, shape, kind, fmt, grad):
    """8 x 1020: the second workgroup starts inside a row.  1 x 16388: beyond the reciprocal form's range, the instances that divide."""
    out, _ = problems(shape).run(kind, fmt, grad)
    assert set(out) == set(fc.OUTPUTS) - (set() if grad else {"grad_depth"})
    for name, value in out.items():
        want = golden(shape, fc.key(shape, kind, fmt, grad, name))
        if name == "grad_depth":
            assert torch.equal(value, want), float((value - want).abs().max())
        else:
            assert_close(value, want, 1e-6, what=name)
