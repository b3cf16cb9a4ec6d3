"""Time TsdfVolume.mesh on the GPU and, beside it, TsdfVolume.surface_points of the same volume.

    python tools/bench_tsdf_mesh.py [--frames 150 --height 720 --width 1280] [--grids 256x256x128,512x512x256] [--iters 5] [--rounds 3] [--out FILE]

The scene and the grids are those of bench_tsdf_volume.py (§3.1e): the static wall 2 m in front of a camera that slides along it 2 cm a
frame, fused with colours into a grid that encloses what the frames see of it, truncation 4 voxels.  Per grid, on the finished volume:

* ``volume.mesh()`` — the count pass, two cumulative sums, one read of the totals, the vertex and the face pass;
* ``volume.surface_points()`` — the nearest thing there was before: the count pass, one cumulative sum, the emit pass;
* the two count passes alone (fm_tsdf_mesh_count, fm_tsdf_surface_count through the C ABI, into preallocated counts): the mesh pass reads
  the 8 corners of a cell where the other reads a voxel and its 3 neighbours.

All with device events after a warm-up, in the same process, alternating over ``--rounds`` rounds, with the peak memory torch allocated
for each call.  Nothing is gated on the times.  Checked on the way: Q < crossings (the rim), every face indexes a vertex, and the mesh
is the same on a second call.  Prints one JSON line; needs a GPU.
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


def wall_scene(f, h, w, dev):
    """bench_tsdf_volume.py's scene -> (depth, k, ext, colors, low, high): the frames and the xy extent of what they see of the wall."""
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 2.0 * (1.0 + 1e-3 * (torch.rand((f, h, w), device=dev, generator=g) - 0.5))
    colors = torch.rand((f, 3, h, w), device=dev, generator=g)
    k = torch.eye(3, device=dev).repeat(f, 1, 1)
    k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2] = 0.85, 1.1, 0.5, 0.5
    ext = torch.eye(4, device=dev).repeat(f, 1, 1)
    ext[:, 0, 3] = 0.02 * torch.arange(f, device=dev)
    ext[:, 1, 3] = 0.002 * torch.arange(f, device=dev)
    low = torch.tensor([-0.5 / 0.85 * 2.0, -0.5 / 1.1 * 2.0])
    high = torch.tensor([0.5 / 0.85 * 2.0 + 0.02 * (f - 1), 0.5 / 1.1 * 2.0 + 0.002 * (f - 1)])
    return depth, k, ext, colors, low, high


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--grids", type=str, default="256x256x128,512x512x256")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf_mesh needs a GPU"

    from flowmap_amd import tsdf_volume
    from flowmap_amd._lib import call, ptr, stream_for

    dev = "cuda:0"
    f, h, w = args.frames, args.height, args.width
    depth, k, ext, colors, low, high = wall_scene(f, h, w, dev)
    result = {"frames": f, "height": h, "width": w, "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "cases": []}
    for dims in [tuple(int(v) for v in item.split("x")) for item in args.grids.split(",")]:
        nx, ny, nz = dims
        voxels = nx * ny * nz
        voxel = float(torch.tensor(max(float(high[0] - low[0]) / nx, float(high[1] - low[1]) / ny), dtype=torch.float32))
        volume = tsdf_volume(depth, k, ext, colors, voxel, origin=(float(low[0]), float(low[1]), 2.0 - 0.5 * nz * voxel), dims=dims)
        blocks = (voxels + 255) // 256
        counts = torch.empty((3, blocks), dtype=torch.int64, device=dev)
        stream = stream_for(volume.tsdf)
        routes = {
            "mesh": lambda: volume.mesh(),
            "surface_points": lambda: volume.surface_points(),
            "mesh_count": lambda: call("fm_tsdf_mesh_count", ptr(volume.tsdf), ptr(volume.weight), nx, ny, nz, 1, ptr(counts[0]), ptr(counts[1]), stream),
            "surface_count": lambda: call("fm_tsdf_surface_count", ptr(volume.tsdf), ptr(volume.weight), nx, ny, nz, 1, ptr(counts[2]), stream),
        }
        mesh, again, surface = volume.mesh(), volume.mesh(), volume.surface_points()
        vertices, quads, crossings = int(mesh.vertices.shape[0]), int(mesh.edge.shape[0]), int(surface[3].shape[0])
        assert 0 < quads < crossings and 0 < vertices, f"{dims}: {vertices} vertices, {quads} quads, {crossings} crossings"
        assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < vertices, f"{dims}: a face indexes no vertex"
        assert all(torch.equal(getattr(mesh, name), getattr(again, name)) for name in ("vertices", "normals", "rgb", "cell", "faces", "edge")), f"{dims}: two calls differ"
        routes["mesh_count"]()
        routes["surface_count"]()
        assert int(counts[0].sum()) == vertices and int(counts[1].sum()) == quads and int(counts[2].sum()) == crossings
        del again
        times = {name: [] for name in routes}
        for _ in range(args.rounds):  # alternating, in one process
            for name, fn in routes.items():
                times[name].append(bc.timed(fn, args.iters, warmup=1))
        peaks = {}
        for name in ("mesh", "surface_points"):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = routes[name]()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
            del out
        case = {"dims": list(dims), "voxels": voxels, "voxel_size": voxel, "vertices": vertices, "quads": quads, "triangles": 2 * quads, "crossings": crossings}
        for name in routes:
            ms = statistics.median(times[name])
            case[name] = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4), "G_voxels_per_s": round(voxels / (ms * 1e-3) / 1e9, 2)}
            if name in peaks:
                case[name]["peak_extra_MB"] = round(peaks[name] / 1e6, 3)
        # what the count passes must read at least once: 8 B per voxel (tsdf and weight); every further read of a voxel is a cache hit or not
        for name in ("mesh_count", "surface_count"):
            case[name]["share_of_hbm_peak_at_8B_per_voxel"] = round(8 * voxels / (case[name]["ms"] * 1e-3) / bc.HBM_PEAK, 4)
        result["cases"].append(case)
        print(f"{dims}: mesh {case['mesh']['ms']:.3f} ms, surface_points {case['surface_points']['ms']:.3f} ms, mesh count pass {case['mesh_count']['ms']:.3f} ms, "
              f"surface count pass {case['surface_count']['ms']:.3f} ms", file=sys.stderr, flush=True)
        del volume, mesh, surface, counts
        torch.cuda.empty_cache()
    bc.emit(result, args.out)


if __name__ == "__main__":
    main()
