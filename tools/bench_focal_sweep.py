"""Time IntrinsicsSoftmin.residuals on the GPU and, beside it, the composition of the existing operators that gives the same curves
(DESIGN.md §3.6a).

    python tools/bench_focal_sweep.py [--frames 150 --height 720 --width 1280] [--points 8192] [--candidates 60] [--rounds 5] [--iters 10] [--out FILE]

The fused route: one fm_focal_sweep call (a workgroup per (pair, candidate), then a wave per pair) — all pairs with and without the
per-point terms, and one pair — timed with device events around ``iters`` calls after a warm-up.  The composed route, on the same
indices: per pair the two-frame slices (``LeadingFrames``), ``ProcrustesFit`` with ``batch_repeat`` = candidates and
``_ops.softmin_intrinsics`` — what ``IntrinsicsSoftmin.forward`` launches for frames (0, 1), once per pair.  For one pair the sum of the
sweep's forward kernels on record (profiles/r06_c1_softmin_rocprofv3_summary.csv: moments, finish + solve, score, blend) is printed
beside both.  ``gathered_GBps``: the bytes a workgroup asks for per correspondence — index 8, later depth 4, weight 4, flow 8 and four
tap depths 16 in the first pass, index 8, depth 4, weight 4, flow 8 in the second — over the time: requests served by the caches, not
HBM traffic (the 8192 pixels of a pair are shared by its 60 workgroups).  The two routes alternate, ``rounds`` times, each measurement in
a fresh child process under its own time limit; the first child that fails or runs out of time ends the run.  Prints one JSON line
(medians and the spread over the rounds); needs a GPU.  No test gates on its numbers.
"""

from __future__ import annotations

import argparse
import csv
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import _bench_common as bc  # noqa: E402
from _bench_common import timed  # noqa: E402

GATHER_BYTES = (8 + 4 + 4 + 8 + 16) + (8 + 4 + 4 + 8)  # per (pair, candidate, correspondence), both passes
NAMES = ("all_pairs", "all_pairs_points", "one_pair")
PROFILE = ROOT / "profiles" / "r06_c1_softmin_rocprofv3_summary.csv"
SWEEP_FORWARD_KERNELS = ("fm::procrustes_moments_kernel<0>", "fm::procrustes_finish_solve_kernel<0>", "softmin_score_fwd_kernel", "softmin_blend_fwd_kernel")


def profiled_forward_us():
    """Σ of the average times of the sweep's forward kernels in the recorded profile of the training step (None when the file is not there)."""
    if not PROFILE.is_file():
        return None
    total = 0.0
    with PROFILE.open() as fh:
        for row in csv.reader(line for line in fh if not line.startswith("#")):
            if len(row) >= 4 and any(row[0].startswith(name) for name in SWEEP_FORWARD_KERNELS):
                total += float(row[3])
    return round(total, 2)


def child(args):
    import torch

    assert torch.cuda.is_available(), "bench_focal_sweep needs a GPU"
    from flowmap_amd import BackboneOutput, Batch, Flows, _ops
    from flowmap_amd.model.intrinsics_softmin import IntrinsicsSoftmin, IntrinsicsSoftminCfg

    dev = "cuda:0"
    f, h, w, n = args.frames, args.height, args.width, args.candidates
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 0.5 + 1.5 * torch.rand((1, f, h, w), device=dev, generator=g)
    bwd = 0.02 * torch.randn((1, f - 1, h, w, 2), device=dev, generator=g)
    weights = 0.1 + 0.9 * torch.rand((1, f - 1, h, w), device=dev, generator=g)
    module = IntrinsicsSoftmin(IntrinsicsSoftminCfg("softmin", args.points, 0.5, 2.0, n, None)).to(dev)
    idx = _ops.random_subset(h * w, min(args.points, h * w), dev, seed=0)
    middle = (f - 1) // 2
    result = {"pairs": f - 1, "points": idx.numel(), "candidates": n}
    if args.child == "fused":
        batch = Batch(torch.zeros((1, f, 3, 1, 1), device=dev).expand(1, f, 3, h, w))
        flows, out = Flows(None, bwd, None, None), BackboneOutput(depth, weights)
        runs = {"all_pairs": dict(), "all_pairs_points": dict(points=True), "one_pair": dict(pairs=(middle, 1))}
        for name in NAMES:
            kw = runs[name]
            ms = timed(lambda: module.residuals(batch, flows, out, indices=idx, **kw), args.iters)
            pairs = kw["pairs"][1] if "pairs" in kw else f - 1
            result[name] = {"ms": ms, "gathered_GBps": pairs * n * idx.numel() * GATHER_BYTES / (ms * 1e-3) / 1e9}
    else:
        candidate_k, k_pair = module._candidate_intrinsics(1, (h, w))

        def pair(i):
            depths = _ops.LeadingFrames.apply(depth[:, i:], 2)
            wts, flow = _ops.LeadingFrames.apply(weights[:, i:], 1), bwd[:, i:i + 1]
            rel, _ = _ops.ProcrustesFit.apply(depths, k_pair, None, wts, flow, idx, 0.0, n)
            return _ops.softmin_intrinsics(depths, wts, flow, idx, candidate_k, rel.reshape(n, 4, 4), 0.0, 2)

        with torch.no_grad():
            result["all_pairs"] = {"ms": timed(lambda: [pair(i) for i in range(f - 1)], max(1, args.iters // 4))}
            result["one_pair"] = {"ms": timed(lambda: pair(middle), args.iters)}
    result["device"] = torch.cuda.get_device_name(0)
    bc.print_child_result(result)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--candidates", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-timeout", type=float, default=90.0, help="seconds a single measurement (one child process) may take")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", choices=("fused", "composed"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    common = []
    for key in ("frames", "height", "width", "points", "candidates", "iters"):
        common += [f"--{key}", str(getattr(args, key))]
    runs = bc.child_rounds("bench_focal_sweep", __file__, common, ("fused", "composed"), args.rounds, args.step_timeout)
    first = runs["fused"][0]
    result = {"frames": args.frames, "height": args.height, "width": args.width, "points": first["points"], "candidates": first["candidates"],
              "device": first["device"], "rounds": args.rounds,
              "fused": {name: bc.summary(runs["fused"], name, scale_to_median=("gathered_GBps",)) for name in NAMES},
              "composed": {name: bc.summary(runs["composed"], name) for name in ("all_pairs", "one_pair")},
              "profiled_sweep_forward_kernels_us": profiled_forward_us()}
    for name in ("all_pairs", "one_pair"):
        result[f"composed_over_fused_{name}"] = round(result["composed"][name]["ms"] / result["fused"][name]["ms"], 2)
    bc.emit(result, args.out)


if __name__ == "__main__":
    main()
