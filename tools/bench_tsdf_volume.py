"""Time export.tsdf_volume on the GPU and, beside it, the same volume composed from what a caller could write before.

    python tools/bench_tsdf_volume.py [--frames 150 --height 720 --width 1280] [--grids 256x256x128,512x512x256] [--iters 5] [--rounds 3] [--out FILE]
    python tools/bench_tsdf_volume.py --fused-only --iters 3      (the run rocprofv3 --kernel-trace --stats wraps)

The scene: the static wall of bench_voxel_cloud.py — 2 m in front of a camera that slides along it 2 cm a frame (depth 2 with 0.1 % noise, no
rotation).  A grid of the stated dims encloses what the frames see of the wall, centred on it in z; truncation is 4 voxels.  Per grid, with
and without colours:

* the fused route: fm_tsdf_volume — one thread per frame for the poses, ONE pass with one thread per voxel that walks the frames with its
  sums in registers and writes the volume once —, timed with device events around ``iters`` calls;
* the composition: per frame, in torch, voxel centres @ pose, the divide, the floor, a ``gather`` of depth (and colour), ``where``, and an
  add into volume-sized sums — F full passes over the volume with volume-sized temporaries each.  ``--composition-iters`` calls per timing.

Both in the same process, alternating over ``--rounds`` rounds, with the peak memory torch allocated for each.  No ratio is promised.  The
two are compared: ``weight`` must be equal on every voxel of a random sample whose observations are all FIRM in an fp64 evaluation (the
tests' gate, tests/tsdf_volume_cases.py, with RHO = 1e-5 and DELTA = 1e-3 pixel: at 1280 pixels fp32 resolves a pixel coordinate to 1.2e-4,
so two fp32 routes may floor it differently inside the tests' 1e-4), and ``tsdf`` may differ there by 8 ulp of the depth over the
truncation (both routes round d − p.z and the pose product a few times).  Beside the times: the voxel-frames per second and a lower bound
on the bytes moved.  Prints one JSON line; needs a GPU.
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

LAUNCHES = 2  # the poses, the volume
DELTA, RHO = 1e-3, 1e-5
SAMPLE = 200_000  # voxels of the fp64 check


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--grids", type=str, default="256x256x128,512x512x256")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--composition-iters", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf_volume needs a GPU"

    from flowmap_amd import tsdf_volume

    dev = "cuda:0"
    f, h, w = args.frames, args.height, args.width
    n = h * w
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 2.0 * (1.0 + 1e-3 * (torch.rand((f, h, w), device=dev, generator=g) - 0.5))
    colors = torch.rand((f, 3, h, w), device=dev, generator=g)
    k = torch.eye(3, device=dev).repeat(f, 1, 1)
    k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2] = 0.85, 1.1, 0.5, 0.5
    ext = torch.eye(4, device=dev).repeat(f, 1, 1)
    ext[:, 0, 3] = 0.02 * torch.arange(f, device=dev)
    ext[:, 1, 3] = 0.002 * torch.arange(f, device=dev)
    # what the frames see of the wall: x = (u − 0.5)/0.85·2 + the camera's x, y likewise
    low = torch.tensor([-0.5 / 0.85 * 2.0, -0.5 / 1.1 * 2.0])
    high = torch.tensor([0.5 / 0.85 * 2.0 + 0.02 * (f - 1), 0.5 / 1.1 * 2.0 + 0.002 * (f - 1)])

    def grid_of(dims):
        nx, ny, nz = dims
        voxel = float(torch.tensor(max(float(high[0] - low[0]) / nx, float(high[1] - low[1]) / ny), dtype=torch.float32))
        origin = (float(low[0]), float(low[1]), 2.0 - 0.5 * nz * voxel)
        return voxel, origin

    def fused(dims, coloured):
        voxel, origin = grid_of(dims)
        return tsdf_volume(depth, k, ext, colors if coloured else None, voxel, origin=origin, dims=dims)

    def centres_of(dims, dtype=torch.float32, at=None):
        voxel, origin = grid_of(dims)
        nx, ny, nz = dims
        index = torch.arange(nx * ny * nz, device=dev) if at is None else at
        ijk = torch.stack((index % nx, (index // nx) % ny, index // (nx * ny)), dim=1).to(dtype)
        return torch.tensor(origin, device=dev, dtype=dtype) + (ijk + 0.5) * torch.tensor(voxel, device=dev, dtype=torch.float32).to(dtype)

    def composed(dims, coloured, world_to_camera):
        with torch.no_grad():
            voxel, _ = grid_of(dims)
            trunc = float(torch.tensor(4.0 * voxel, dtype=torch.float32))
            c = centres_of(dims)
            total = torch.zeros(c.shape[0], device=dev)
            weight = torch.zeros(c.shape[0], device=dev, dtype=torch.int32)
            if coloured:
                sums = torch.zeros((3, c.shape[0]), device=dev)
                color_weight = torch.zeros_like(weight)
            for i in range(f):
                p = c @ world_to_camera[i, :3, :3].T + world_to_camera[i, :3, 3]
                z = p[:, 2]
                q = torch.nan_to_num(p / (z + 1e-5)[:, None], nan=0.0, posinf=1e8, neginf=-1e8)
                uv = q @ k[i, :2].T
                ok = (z > 0) & (uv >= 0).all(dim=1) & (uv < 1).all(dim=1)
                col = torch.floor(uv[:, 0] * w).clamp(0, w - 1).long()
                row = torch.floor(uv[:, 1] * h).clamp(0, h - 1).long()
                pixel = torch.where(ok, row * w + col, torch.zeros_like(col))
                d = depth[i].reshape(-1).gather(0, pixel)
                sdf = d - z
                take = ok & torch.isfinite(d) & (d > 0) & (sdf >= -trunc)
                total += torch.where(take, (sdf / trunc).clamp_max(1.0), torch.zeros_like(sdf))
                weight += take
                if coloured:
                    tinted = take & (sdf <= trunc)
                    sums += torch.where(tinted[None], colors[i].reshape(3, -1).gather(1, pixel[None].expand(3, -1)), torch.zeros_like(sums[:, :1]))
                    color_weight += tinted
            tsdf = torch.where(weight > 0, total / weight.clamp_min(1), torch.ones_like(total))
            if not coloured:
                return tsdf, weight, None, None
            return tsdf, weight, torch.where(color_weight > 0, sums / color_weight.clamp_min(1), torch.zeros_like(sums)).T, color_weight

    def firm_sample(dims, world_to_camera):
        """A random sample of voxels -> (their linear indices, all of their observations firm in fp64)."""
        voxel, _ = grid_of(dims)
        trunc = float(torch.tensor(4.0 * voxel, dtype=torch.float32))
        nx, ny, nz = dims
        at = torch.randint(0, nx * ny * nz, (SAMPLE,), device=dev, generator=g)
        c = centres_of(dims, torch.float64, at)
        firm = torch.ones(SAMPLE, dtype=torch.bool, device=dev)
        inverse = torch.linalg.inv(ext.double())
        for i in range(f):
            p = c @ inverse[i, :3, :3].T + inverse[i, :3, 3]
            z = p[:, 2]
            uv = torch.nan_to_num(p / (z + 1e-5)[:, None], nan=0.0, posinf=1e8, neginf=-1e8) @ k[i, :2].double().T
            px, py = uv[:, 0] * w, uv[:, 1] * h
            front = z > 0
            inside = (uv >= 0).all(dim=1) & (uv < 1).all(dim=1)
            pixel = torch.where(inside, torch.floor(py).clamp(0, h - 1).long() * w + torch.floor(px).clamp(0, w - 1).long(), torch.zeros_like(at))
            d = depth[i].reshape(-1).gather(0, pixel).double()
            sdf = d - z
            out_firm = (px < -DELTA) | (px > w + DELTA) | (py < -DELTA) | (py > h + DELTA)
            in_firm = inside & ((px - torch.round(px)).abs() > DELTA) & ((py - torch.round(py)).abs() > DELTA)
            hidden_firm = (sdf + trunc).abs() > RHO * (z.abs() + trunc)
            near_firm = z.abs() > RHO * z.abs()
            firm &= (near_firm & ~front) | (near_firm & front & (out_firm | (in_firm & hidden_firm)))
        return at, firm

    grids = [tuple(int(v) for v in item.split("x")) for item in args.grids.split(",")]
    result = {"frames": f, "height": h, "width": w, "device": torch.cuda.get_device_name(0), "launches": LAUNCHES, "iters": args.iters,
              "composition_iters": args.composition_iters, "rounds": args.rounds, "cases": []}
    for dims in grids:
        voxels = dims[0] * dims[1] * dims[2]
        for coloured in (False, True):
            volume = fused(dims, coloured)
            torch.cuda.synchronize()
            if args.fused_only:
                bc.timed(lambda: fused(dims, coloured), args.iters, warmup=0)
                continue
            w2c = volume.world_to_camera
            composed(dims, coloured, w2c)
            times = {"fused": [], "composition": []}
            for _ in range(args.rounds):  # alternating, in one process
                times["fused"].append(bc.timed(lambda: fused(dims, coloured), args.iters, warmup=1))
                times["composition"].append(bc.timed(lambda: composed(dims, coloured, w2c), args.composition_iters, warmup=0))
            peaks = {}
            for name, fn in (("fused", lambda: fused(dims, coloured)), ("composition", lambda: composed(dims, coloured, w2c))):
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                out = fn()
                torch.cuda.synchronize()
                peaks[name] = torch.cuda.max_memory_allocated() - base
                del out
            tsdf, weight, color, color_weight = composed(dims, coloured, w2c)
            at, firm = firm_sample(dims, w2c)
            mine_w, mine_t = volume.weight.reshape(-1)[at], volume.tsdf.reshape(-1)[at]
            weights_equal = bool(torch.equal(mine_w[firm], weight[at][firm]))
            tsdf_gap = float((mine_t[firm] - tsdf[at][firm]).abs().max())
            assert weights_equal, f"{dims}: the fused pass and the composition disagree on the weight of a firm voxel"
            tolerance = 8.0 * 2.0**-22 / float(volume.truncation)  # (8 ulp of a depth in [2, 4) over the truncation)
            assert tsdf_gap <= tolerance, f"{dims}: tsdf differs by {tsdf_gap:.3e} > {tolerance:.3e} between the routes on a firm voxel"
            ms, ms_c = statistics.median(times["fused"]), statistics.median(times["composition"])
            observed = int(volume.weight.sum())
            # a lower bound: 4 bytes of depth per TAKEN observation (a hidden one reads its depth too), 12 of colour per coloured one, and per
            # voxel the 8 bytes written (16 more with colours); the per-frame constants are scalar loads shared by a wavefront
            bytes_moved = 4 * observed + 12 * (int(volume.color_weight.sum()) if coloured else 0) + voxels * (8 + (16 if coloured else 0))
            case = {"dims": list(dims), "voxels": voxels, "colours": coloured, "voxel_size": grid_of(dims)[0], "voxel_frames": voxels * f, "observations": observed,
                    "crossings": int(volume.surface_points()[3].shape[0]), "sample": SAMPLE, "firm_in_sample": int(firm.sum()), "weights_equal_where_firm": weights_equal,
                    "max_tsdf_difference_where_firm": tsdf_gap, "tsdf_tolerance": tolerance, "weights_differ_in_all": int((volume.weight.reshape(-1) != weight).sum()),
                    "fused": {"ms": round(ms, 3), "ms_min": round(min(times["fused"]), 3), "ms_max": round(max(times["fused"]), 3), "peak_extra_GB": round(peaks["fused"] / 1e9, 3),
                              "G_voxel_frames_per_s": round(voxels * f / (ms * 1e-3) / 1e9, 2), "algorithmic_GB": round(bytes_moved / 1e9, 3),
                              "share_of_hbm_peak": round(bytes_moved / (ms * 1e-3) / bc.HBM_PEAK, 4)},
                    "composition": {"ms": round(ms_c, 3), "ms_min": round(min(times["composition"]), 3), "ms_max": round(max(times["composition"]), 3),
                                    "peak_extra_GB": round(peaks["composition"] / 1e9, 3), "ratio_to_fused": round(ms_c / ms, 2)}}
            result["cases"].append(case)
            print(f"{dims} colours={coloured}: fused {ms:.3f} ms, composition {ms_c:.3f} ms", file=sys.stderr, flush=True)
            del volume, tsdf, weight, color, color_weight
            torch.cuda.empty_cache()
    bc.emit(result, args.out)


if __name__ == "__main__":
    main()
