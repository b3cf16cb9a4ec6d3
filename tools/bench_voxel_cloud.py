"""Time export.voxel_point_cloud on the GPU and, beside it, the same cloud composed from what a caller could write before
(DESIGN.md §3.1d).

    python tools/bench_voxel_cloud.py [--frames 150 --height 720 --width 1280] [--sizes 0.01,0.003,0.002] [--iters 5] [--rounds 3] [--out FILE]
    python tools/bench_voxel_cloud.py --fused-only --iters 3      (the run rocprofv3 --kernel-trace --stats wraps)

The scene: a static wall 2 m in front of a camera that slides along it 2 cm a frame (depth 2 with 0.1 % noise, no rotation), so
neighbouring pixels and neighbouring frames land in the same voxels, as the frames of a video of a static scene do.  Per ``voxel_size``, without and with a ``keep`` mask (a fixed
random half of the pixels):

* the fused route: fm_voxel_cloud — three memsets, ONE pass over depth into a hash table of integer accumulators, one pass over the
  table — and the sort of the M rows by their lowest index, at the default capacity, timed with device events around ``iters`` calls;
* the composition: ``world_point_cloud`` (all F·H·W points and colours materialised, then masked), ``floor``, the three cells packed into
  ONE int64 key — kinder to the composition than ``torch.unique(dim=0)`` on (N, 3) rows —, ``torch.unique(return_inverse, return_counts)``,
  ``index_add_`` of the float points and colours, ``scatter_reduce_(amin)`` for the lowest index, the sort by it.  Its float sums run in
  arrival order: it is not reproducible from run to run, and its centroids are compared with the fused ones at a tolerance only.

Both in the same process, alternating over ``--rounds`` rounds, with the peak memory torch allocated for each.  No ratio is promised.
Beside the times: M, the points merged, the atomic requests per live point the kernel issues (8 adds/max into one 64-byte record, and one
compare-and-swap per voxel rather than per point) and the rate they imply over the WHOLE call.  Prints one JSON line; needs a GPU.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import _bench_common as bc  # noqa: E402

LAUNCHES = 5  # three memsets, the insert pass, the compact pass (then torch's sort and gathers)
ATOMICS_PER_POINT = 8  # into one 64-byte record: 3 position sums, 3 colour sums, the count, the lowest index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--sizes", type=str, default="0.01,0.003,0.002")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxel_cloud needs a GPU"

    from flowmap_amd import voxel_point_cloud
    from flowmap_amd.export import voxel_default_capacity, world_point_cloud

    dev = "cuda:0"
    f, h, w = args.frames, args.height, args.width
    n = f * h * w
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 2.0 * (1.0 + 1e-3 * (torch.rand((f, h, w), device=dev, generator=g) - 0.5))
    colors = torch.rand((f, 3, h, w), device=dev, generator=g)
    k = torch.eye(3, device=dev).repeat(f, 1, 1)
    k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2] = 0.85, 1.1, 0.5, 0.5
    ext = torch.eye(4, device=dev).repeat(f, 1, 1)
    ext[:, 0, 3] = 0.02 * torch.arange(f, device=dev)
    ext[:, 1, 3] = 0.002 * torch.arange(f, device=dev)
    half = torch.rand((f, h, w), device=dev, generator=g) < 0.5
    index = torch.arange(n, device=dev)

    def fused(voxel, keep):
        capacity = voxel_default_capacity(n)  # (given: no count of the mask inside the timed call)
        return voxel_point_cloud(depth, k, ext, colors, voxel, keep=keep, capacity=capacity)

    def composed(voxel, keep):
        with torch.no_grad():
            xyz, rgb = world_point_cloud(depth, k, ext, colors, keep=keep)
            where = index if keep is None else index[keep.reshape(-1)]
            cells = torch.floor(xyz / voxel).to(torch.int64) + (1 << 20)
            key = (cells[:, 0] << 42) | (cells[:, 1] << 21) | cells[:, 2]
            del cells
            _, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
            del key
            m = counts.numel()
            centre = torch.zeros((m, 3), device=dev).index_add_(0, inverse, xyz) / counts[:, None]
            colour = torch.zeros((m, 3), device=dev).index_add_(0, inverse, rgb) / counts[:, None]
            first = torch.full((m,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, where, "amin")
            first, order = torch.sort(first)
            return centre[order], colour[order], counts[order], first

    sizes = [float(s) for s in args.sizes.split(",")]
    result = {"frames": f, "height": h, "width": w, "points": n, "device": torch.cuda.get_device_name(0), "launches": LAUNCHES, "iters": args.iters,
              "rounds": args.rounds, "atomic_requests_per_live_point": ATOMICS_PER_POINT, "cases": []}
    for voxel in sizes:
        for keep, label in ((None, "all"), (half, "keep half")):
            fused(voxel, keep)
            torch.cuda.synchronize()
            if args.fused_only:
                bc.timed(lambda: fused(voxel, keep), args.iters, warmup=0)
                continue
            composed(voxel, keep)
            times = {"fused": [], "composition": []}
            for _ in range(args.rounds):  # alternating, in one process
                times["fused"].append(bc.timed(lambda: fused(voxel, keep), args.iters, warmup=1))
                times["composition"].append(bc.timed(lambda: composed(voxel, keep), max(1, args.iters // 2), warmup=0))
            peaks = {}
            for name, fn in (("fused", fused), ("composition", composed)):  # peak memory of each route, from the same base
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                out = fn(voxel, keep)
                torch.cuda.synchronize()
                peaks[name] = torch.cuda.max_memory_allocated() - base
                del out
            cloud = fused(voxel, keep)
            centre, colour, counts, first = composed(voxel, keep)
            live = int(cloud.count.sum())
            same_rows = len(cloud) == first.numel() and bool(torch.equal(cloud.first, first))
            ms, ms_c = statistics.median(times["fused"]), statistics.median(times["composition"])
            case = {"voxel_size": voxel, "keep": label, "voxels": len(cloud), "live_points": live, "dropped": cloud.dropped, "points_per_voxel": round(live / max(len(cloud), 1), 2),
                    "same_voxels_as_the_composition": same_rows,
                    "fused": {"ms": round(ms, 3), "ms_min": round(min(times["fused"]), 3), "ms_max": round(max(times["fused"]), 3), "peak_extra_GB": round(peaks["fused"] / 1e9, 3),
                              "atomic_G_requests_per_s_over_the_whole_call": round(live * ATOMICS_PER_POINT / (ms * 1e-3) / 1e9, 2)},
                    "composition": {"ms": round(ms_c, 3), "ms_min": round(min(times["composition"]), 3), "ms_max": round(max(times["composition"]), 3),
                                    "peak_extra_GB": round(peaks["composition"] / 1e9, 3), "ratio_to_fused": round(ms_c / ms, 2)}}
            if same_rows:  # (a cell the two floors — x·fl(1/s) and x/s — disagree on would show as another row count or another first)
                case["max_centroid_difference"] = float((cloud.xyz - centre).abs().max())
                case["counts_equal"] = bool(torch.equal(cloud.count.long(), counts))
            result["cases"].append(case)
            del cloud, centre, colour, counts, first
    bc.emit(result, args.out)


if __name__ == "__main__":
    main()
