"""Time LossTracking.residuals on the GPU and, beside it, the general route producing the same maps.

    python tools/bench_track_residuals.py [--frames 150 --height 720 --width 1280] [--rounds 5] [--iters 20] [--out FILE]

The track layout is BASELINE.json configs[2]'s: a segment around every 5th frame, ±20 frames, 35 × 35 points (30 segments of up to 41
frames and 1225 points at 150 frames).  The fused route: one fm_track_residuals launch (+ the table of target constants before it and
the ordered second stage of the sums after it) for ONE segment (the middle one) and for ALL segments, with and without the reprojected
positions and the sums, timed with device events around ``iters`` calls after a warm-up; the bytes it writes (5 per element, 13 with the
positions) and reads (9 per element) over the time give the share of the 8 TB/s HBM peak.  The general route: explicit surfaces ->
compute_track_flow -> mapping.forward segment by segment, the operators a caller had before this method existed, timed the same way with
the peak memory torch allocated for it.  The two routes alternate, ``rounds`` times, each measurement in a fresh child process under its
own time limit; the first child that fails or runs out of time ends the run.  Prints one JSON line (medians and the spread over the
rounds); needs a GPU.  No test gates on its numbers.
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import _bench_common as bc  # noqa: E402
from _bench_common import HBM_PEAK, timed  # noqa: E402,F401


def make_tracks(f, dev, seed=0, interval=5, radius=20, grid=35):
    """generate_video_tracks' layout (flowmap/tracking/__init__.py:49-70) with positions drifting as a random walk, ~90 % visible."""
    import torch

    from flowmap_amd import Tracks

    g = torch.Generator(device=dev).manual_seed(seed)
    lin = (torch.arange(grid, device=dev, dtype=torch.float32) + 0.5) / grid
    query = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), dim=-1).reshape(-1, 2)
    out = []
    for mid in range(0, f, interval):
        start, end = max(0, mid - radius), min(f, mid + radius + 1)
        drift = (0.003 * torch.randn((end - start, query.shape[0], 2), device=dev, generator=g)).cumsum(0)
        xy = query[None] + drift - drift[mid - start]
        vis = (xy >= 0).all(-1) & (xy < 1).all(-1) & (torch.rand(xy.shape[:2], device=dev, generator=g) < 0.9)
        out.append(Tracks(xy[None].contiguous(), vis[None].contiguous(), start))
    return out


def child(args):
    import torch

    assert torch.cuda.is_available(), "bench_track_residuals needs a GPU"
    from flowmap_amd import Batch, ModelOutput
    from flowmap_amd.loss import LossTracking, LossTrackingCfg
    from flowmap_amd.loss.mapping import MappingHuberCfg
    from flowmap_amd.model.projection import LazySurfaces

    dev = "cuda:0"
    f, h, w = args.frames, args.height, args.width
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 0.5 + 1.5 * torch.rand((1, f, h, w), device=dev, generator=g)
    k = torch.eye(3, device=dev).repeat(1, f, 1, 1)
    k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2] = 0.85, 1.1, 0.5, 0.5
    ext = torch.eye(4, device=dev).repeat(1, f, 1, 1)
    ext[0, :, 0, 3] = 0.002 * torch.arange(f, device=dev)
    tracks = make_tracks(f, dev)
    batch = Batch(torch.zeros((1, f, 3, 1, 1), device=dev).expand(1, f, 3, h, w))
    loss = LossTracking(LossTrackingCfg(0, 100.0, "tracking", MappingHuberCfg("huber", 0.01)))
    middle = len(tracks) // 2
    elements = [t.xy.shape[1] ** 2 * t.xy.shape[2] for t in tracks]
    result = {"segments": len(tracks), "elements_all": sum(elements), "elements_one": elements[middle]}
    if args.child == "fused":
        out = ModelOutput(depth, LazySurfaces(depth, k), k, ext, None)
        for name, segments, predicted, sums in (("one", middle, False, True), ("one_predicted", middle, True, True), ("all", None, False, True),
                                                ("all_predicted", None, True, True), ("all_no_sums", None, False, False)):
            ms = timed(lambda: loss.residuals(batch, tracks, out, segments=segments, predicted=predicted, sums=sums), args.iters)
            n = elements[middle] if segments is not None else sum(elements)
            written, moved = n * (13 if predicted else 5), n * ((13 if predicted else 5) + 9)
            result[name] = {"ms": ms, "written_MB": written / 1e6, "share_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK}
    else:
        surfaces = LazySurfaces(depth, k).materialize()
        out = ModelOutput(depth, surfaces, k, ext, None)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        result["one"] = {"ms": timed(lambda: loss.residuals(batch, tracks, out, segments=middle), args.general_iters, warmup=1)}
        result["all"] = {"ms": timed(lambda: loss.residuals(batch, tracks, out), args.general_iters, warmup=1),
                         "peak_extra_GB": (torch.cuda.max_memory_allocated() - base) / 1e9, "surfaces_GB": surfaces.numel() * 4 / 1e9}
    result["device"] = torch.cuda.get_device_name(0)
    bc.print_child_result(result)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--general-iters", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=90.0, help="seconds a single measurement (one child process) may take")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", choices=("fused", "general"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    common = ["--frames", str(args.frames), "--height", str(args.height), "--width", str(args.width), "--iters", str(args.iters),
              "--general-iters", str(args.general_iters)]
    runs = bc.child_rounds("bench_track_residuals", __file__, common, ("fused", "general"), args.rounds, args.step_timeout)
    first = runs["fused"][0]
    result = {"frames": args.frames, "height": args.height, "width": args.width, "device": first["device"], "rounds": args.rounds,
              "segments": first["segments"], "elements_all": first["elements_all"], "elements_one": first["elements_one"],
              "fused": {name: bc.summary(runs["fused"], name) for name in ("one", "one_predicted", "all", "all_predicted", "all_no_sums")},
              "general": {name: bc.summary(runs["general"], name) for name in ("one", "all")}}
    result["general_over_fused"] = {name: round(result["general"][name]["ms"] / result["fused"][name]["ms"], 1) for name in ("one", "all")}
    bc.emit(result, args.out)


if __name__ == "__main__":
    main()
