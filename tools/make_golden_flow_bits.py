"""Record tests/golden/flow_fused_parent_bits.npz: the outputs of the fused flow pass of the commit that is checked out and built, on the
seeded inputs of tests/flow_frame_constants_cases.py.  Run on a GPU, on the PARENT of a change that must keep the pass's bits:

    python tools/make_golden_flow_bits.py --commit $(git rev-parse HEAD)

Per case (shape, mapping, packed format, with / without gradients; keys ``<BxFxHxW>.<kind>.<format>.<grad|loss>.<output>``): loss, dL/ddepth,
dL/dT_fwd, dL/dT_bwd, dL/dK and the 13 sums per (frame, direction).  An array equal, bit for bit, to one already recorded is stored once:
``aliases`` (JSON) maps its key to the first one's.  Beside them: ``commit``, ``seed``, per shape the small inputs (K, K⁻¹, poses — their
recipe goes through a matrix exponential and an inverse, which two hosts need not round alike) and a checksum of the image-sized inputs,
which every host regenerates from torch.rand.  Each case is run twice here and must reproduce itself where the test demands equality.
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

import flow_frame_constants_cases as fc  # noqa: E402

OUT = ROOT / "tests" / "golden" / "flow_fused_parent_bits.npz"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="hash of the commit that is built (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=str(OUT))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dev = "cuda:0"
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
    for shape in fc.SHAPES:
        prob = problems[shape] = fc.Problem(shape, dev)
        for name in fc.SMALL:
            arrays[f"{fc.shape_name(shape)}.input.{name}"] = prob.host[name].numpy()
        arrays[f"{fc.shape_name(shape)}.input.checksum"] = np.array(fc.checksum(prob.host), dtype=np.int64)
    for shape, kind, fmt, grad in fc.combos():
        out, _ = problems[shape].run(kind, fmt, grad)
        again, _ = problems[shape].run(kind, fmt, grad)
        exact = fc.OUTPUTS if shape in fc.ONE_WORKGROUP_SHAPES else ("grad_depth",)
        for name, value in out.items():
            assert bool(torch.isfinite(value).all()), (shape, kind, fmt, grad, name)
            if name in exact:
                assert torch.equal(value, again[name]), f"{fc.key(shape, kind, fmt, grad, name)} does not reproduce itself"
            put(fc.key(shape, kind, fmt, grad, name), value)
        assert float(out["sums"].abs().max()) > 0 and (not grad or float(out["grad_depth"].abs().max()) > 0)
    np.savez(args.out, commit=np.array(commit), seed=np.array(fc.SEED, dtype=np.int64), aliases=np.array(json.dumps(aliases)), **arrays)
    size = Path(args.out).stat().st_size
    print(f"wrote {args.out}: {len(arrays)} arrays, {len(aliases)} aliases, {size} bytes, commit {commit}")


if __name__ == "__main__":
    main()
