"""The fused flow pass with its per-(frame, direction) constants computed once per step (flow_dir_table_kernel, fm_flow.hip) against the
outputs recorded from the commit before that change, where every wave computed them in the kernel's prologue
(tests/golden/flow_fused_parent_bits.npz, tools/make_golden_flow_bits.py; cases and shapes: tests/flow_frame_constants_cases.py).

* Frames of one workgroup: loss, dL/ddepth, dL/dT, dL/dK and the 13 sums are the recorded BITS, for the three mappings, the three input
  formats, with and without gradients.
* A frame of two workgroups: dL/ddepth is the recorded bits; the sums meet through fp64 atomics, so they and what finalize derives from them
  are held to the 1e-6 relative include/flowmap_hip.h states for them.
* The workspace contract: the constants travel in the padding of `acc`; after finalize the whole workspace is zero again, and steps on a
  workspace kept across them equal steps on fresh zeros."""

import json
from pathlib import Path

import numpy as np
import pytest
import torch

import flow_frame_constants_cases as fc
from conftest import assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden" / "flow_fused_parent_bits.npz"


@pytest.fixture(scope="module")
def golden():
    data = np.load(GOLDEN)
    aliases = json.loads(str(data["aliases"]))
    assert int(data["seed"]) == fc.SEED

    def get(name):
        return torch.from_numpy(data[aliases.get(name, name)])

    return get


@pytest.fixture(scope="module")
def problems(golden):
    made = {}

    def get(shape):
        if shape not in made:
            name = fc.shape_name(shape)
            prob = fc.Problem(shape, DEV, small={n: golden(f"{name}.input.{n}") for n in fc.SMALL})
            assert fc.checksum(prob.host) == int(golden(f"{name}.input.checksum")), "this host generates other inputs than the recording one"
            made[shape] = prob
        return made[shape]

    return get


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "loss_only"])
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("shape,fmt", [(shape, fmt) for shape in fc.ONE_WORKGROUP_SHAPES for fmt in fc.formats_of(shape)],
                         ids=lambda v: v if isinstance(v, str) else fc.shape_name(v))
def test_one_workgroup_frames_keep_the_parents_bits(golden, problems, shape, kind, fmt, grad):
    out, _ = problems(shape).run(kind, fmt, grad)
    assert set(out) == set(fc.OUTPUTS) - (set() if grad else {"grad_depth"})
    for name, value in out.items():
        want = golden(fc.key(shape, kind, fmt, grad, name))
        assert torch.equal(value, want), (name, float((value.double() - want.double()).abs().max()))


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "loss_only"])
@pytest.mark.parametrize("fmt", fc.FORMATS)
@pytest.mark.parametrize("kind", fc.KINDS)
def test_two_workgroup_frames(golden, problems, kind, fmt, grad):
    shape = fc.MULTI_WORKGROUP_SHAPE
    out, _ = problems(shape).run(kind, fmt, grad)
    for name, value in out.items():
        want = golden(fc.key(shape, kind, fmt, grad, name))
        if name == "grad_depth":
            assert torch.equal(value, want), float((value - want).abs().max())
        else:
            assert_close(value, want, 1e-6, what=name)


@pytest.mark.parametrize("fmt", fc.FORMATS)
@pytest.mark.parametrize("shape", [fc.ONE_WORKGROUP_SHAPES[1], fc.MULTI_WORKGROUP_SHAPE], ids=fc.shape_name)
def test_finalize_leaves_the_whole_workspace_zero(problems, shape, fmt):
    prob = problems(shape)
    acc = prob.new_acc()
    prob.fused("huber", fmt, True, acc)
    assert float(acc.abs().max()) > 0
    prob.finalize(acc)
    assert torch.equal(acc, torch.zeros_like(acc))  # the sums AND the padding the constants travelled in


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_a_kept_workspace_equals_fresh_zeros(problems, fmt):
    """Three steps (another mapping each: other sums, the same constants) on one workspace against the same steps on fresh zeros."""
    prob = problems(fc.ONE_WORKGROUP_SHAPES[1])
    kept = prob.new_acc()
    for kind in fc.KINDS:
        on_kept, kept = prob.run(kind, fmt, True, acc=kept)
        on_fresh, _ = prob.run(kind, fmt, True)
        for name in fc.OUTPUTS:
            assert torch.equal(on_kept[name], on_fresh[name]), (kind, name)
        assert torch.equal(kept, torch.zeros_like(kept))
