"""Record tests/golden/flow_exact_coordinates_parent_bits.npz (and ..._multi.npz): the outputs of the fused flow pass of the commit that is
checked out and built, at the shapes of tests/flow_exact_coordinates_cases.py.  Run on a GPU, on the PARENT of a change that must keep the
pass's bits:

    python tools/make_golden_flow_exact_coordinates.py --commit $(git rev-parse HEAD)

Method, seeded inputs and keys are those of tools/make_golden_flow_bits.py (``<BxFxHxW>.<kind>.<format>.<grad|loss>.<output>``; an array
equal, bit for bit, to one already recorded is stored once and listed in ``aliases``; per shape the small inputs and a checksum of the
image-sized ones; each case is run twice and must reproduce itself where the test demands equality).  The frames of one workgroup go into
the first file, the two shapes whose frames take several workgroups into the second one: together their dL/ddepth images would pass the
size a committed file may have.
"""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import flow_exact_coordinates_cases as ec  # noqa: E402
import flow_frame_constants_cases as fc  # noqa: E402

OUT = ROOT / "tests" / "golden" / "flow_exact_coordinates_parent_bits.npz"


def record(shapes, exact_outputs, path, commit, dev="cuda:0"):
    arrays, aliases, first_of = {}, {}, {}

    def put(name, value):
        a = np.ascontiguousarray(value.numpy())
        digest = (a.dtype.str, a.shape, a.tobytes())
        if digest in first_of:
            aliases[name] = first_of[digest]
        else:
            first_of[digest] = name
            arrays[name] = a

    problems = {}
    for shape in shapes:
        prob = problems[shape] = fc.Problem(shape, dev)
        for name in fc.SMALL:
            arrays[f"{fc.shape_name(shape)}.input.{name}"] = prob.host[name].numpy()
        arrays[f"{fc.shape_name(shape)}.input.checksum"] = np.array(fc.checksum(prob.host), dtype=np.int64)
    for shape, kind, fmt, grad in ec.combos(shapes):
        out, _ = problems[shape].run(kind, fmt, grad)
        again, _ = problems[shape].run(kind, fmt, grad)
        for name, value in out.items():
            assert bool(torch.isfinite(value).all()), (shape, kind, fmt, grad, name)
            if name in exact_outputs:
                assert torch.equal(value, again[name]), f"{fc.key(shape, kind, fmt, grad, name)} does not reproduce itself"
            put(fc.key(shape, kind, fmt, grad, name), value)
        assert float(out["sums"].abs().max()) > 0 and (not grad or float(out["grad_depth"].abs().max()) > 0)
    np.savez_compressed(path, commit=np.array(commit), seed=np.array(fc.SEED, dtype=np.int64), aliases=np.array(json.dumps(aliases)), **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {len(aliases)} aliases, {Path(path).stat().st_size} bytes, commit {commit}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="hash of the commit that is built (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=str(OUT), help="the one-workgroup file; the other one gets `_multi` in front of its suffix")
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    out = Path(args.out)
    record(ec.ONE_WORKGROUP_SHAPES, fc.OUTPUTS, out, commit)
    record(ec.ATOMIC_SHAPES, ("grad_depth",), out.with_name(out.stem + "_multi" + out.suffix), commit)


if __name__ == "__main__":
    main()
