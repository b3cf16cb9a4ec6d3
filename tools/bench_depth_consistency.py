"""Time projection.depth_consistency on the GPU and, beside it, the same maps composed from the package's existing operators
(DESIGN.md §3.1b).

    python tools/bench_depth_consistency.py [--frames 150 --height 720 --width 1280 --window 8] [--iters 20] [--rounds 3] [--out FILE]

The fused route: fm_depth_consistency — one small launch for the window's relative poses, ONE pass over depth, the ordered second stage
of the sums: 3 launches (one more for K⁻¹ when it is not already on K) — on a window of ``--window`` frames in the middle of the video at offsets (−2, −1, 1, 2), with and without the
details, timed with device events around ``iters`` calls after a warm-up of every shape timed.  Its algorithmic bytes per pixel and
offset (the formula below: the source depth once per pixel, one target depth map per offset — the four taps of adjacent pixels share
their lines —, error and code out, with the details uv, q.z and the sample as well) over the time give the share of the 8 TB/s HBM peak.
The composition: what a caller can do without this call — ``unproject`` once (materialised surfaces of the window), then per offset
``transform_rigid`` / ``project_camera_space`` through ``reproject_points`` for the positions, the third row of the same transform in
torch for q.z, ``BilinearSample`` of the target depth, and the code and the error in torch — timed the same way in the same process,
alternating with the fused route over ``--rounds`` rounds, with the peak memory torch allocated for it.  The call is also timed without
its sums.  Prints one JSON line and fails unless the fused call is faster and allocates less; needs a GPU.
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
from _bench_common import HBM_PEAK  # noqa: E402

OFFSETS = (-2, -1, 1, 2)
LAUNCHES = 3  # the pose rows, the pass over depth, the ordered sums


def algorithmic_bytes(pixels, frames, n_off, details, tolerance):
    """Bytes the call has to move for ``frames`` source frames of ``pixels`` pixels: the source depth once per pixel, a target depth map
    per (frame, offset), error (4) and code (1) out per pixel and offset — uv (8), q.z (4) and the sample (4) with the details —, and the
    support byte per pixel with a tolerance."""
    per_offset = 4 + 4 + 1 + (16 if details else 0)
    return frames * pixels * (4 + n_off * per_offset + (1 if tolerance else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_consistency needs a GPU"

    from flowmap_amd import _ops, depth_consistency
    from flowmap_amd.model.projection import reproject_points, sample_image_grid, unproject_dense

    dev = "cuda:0"
    f, h, w, count = args.frames, args.height, args.width, args.window
    first = (f - count) // 2
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 1.5 + 0.5 * torch.rand((1, f, h, w), device=dev, generator=g)
    k = torch.eye(3, device=dev).repeat(1, f, 1, 1)
    k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2] = 0.85, 1.1, 0.5, 0.5
    ext = torch.eye(4, device=dev).repeat(1, f, 1, 1)
    ext[0, :, 0, 3] = 0.02 * torch.arange(f, device=dev)
    ext[0, :, 2, 3] = 0.005 * torch.arange(f, device=dev)
    xy, _ = sample_image_grid((h, w), dev)
    frames = (first, count)
    n_off = len(OFFSETS)

    def fused(details, sums=True):
        return depth_consistency(depth, k, ext, offsets=OFFSETS, frames=frames, tolerance=0.05, details=details, sums=sums)

    def composed():
        """error and code of the same window from the existing operators, one offset at a time (every source frame has its target here)."""
        with torch.no_grad():
            src = slice(first, first + count)
            points = unproject_dense(xy, depth[:, src], k[:, src][:, :, None, None])  # (1, count, h, w, 3)
            errors, codes = [], []
            for d in OFFSETS:
                dst = slice(first + d, first + count + d)
                rel = torch.linalg.inv(ext[:, dst]) @ ext[:, src]
                uv = reproject_points(points, rel[:, :, None, None], k[:, dst][:, :, None, None])
                # q.z: the third row of the rigid transform (transform_rigid's einsum restricted to the row that is read)
                qz = (points * rel[:, :, None, None, 2, :3]).sum(-1) + rel[:, :, None, None, 2, 3]
                zs = _ops.BilinearSample.apply(depth[0, dst].reshape(count, h, w, 1), uv.reshape(count, h * w, 2)).reshape(1, count, h, w)
                inside = (uv >= 0).all(-1) & (uv < 1).all(-1)
                code = torch.where(~(qz > 0), 2, torch.where(inside, 0, 3)).to(torch.uint8)
                errors.append(torch.where(code == 0, (zs - qz) / qz, torch.zeros_like(qz)))
                codes.append(code)
            return torch.stack(errors, dim=2), torch.stack(codes, dim=2)

    assert first + min(OFFSETS) >= 0 and first + count + max(OFFSETS) <= f, "the window's targets must lie inside the video"
    result = {"frames": f, "height": h, "width": w, "window": list(frames), "offsets": list(OFFSETS), "device": torch.cuda.get_device_name(0),
              "launches": LAUNCHES, "iters": args.iters, "rounds": args.rounds}
    for fn in (lambda: fused(False), lambda: fused(True), lambda: fused(False, sums=False), composed):  # a warm-up of every shape timed
        fn()
    torch.cuda.synchronize()
    times = {"fused": [], "fused_details": [], "fused_no_sums": [], "composition": []}
    for _ in range(args.rounds):  # alternating, in one process
        times["fused"].append(bc.timed(lambda: fused(False), args.iters, warmup=1))
        times["composition"].append(bc.timed(composed, max(1, args.iters // 4), warmup=1))
        times["fused_details"].append(bc.timed(lambda: fused(True), args.iters, warmup=1))
        times["fused_no_sums"].append(bc.timed(lambda: fused(False, sums=False), args.iters, warmup=1))
    pixels = h * w
    for name, details in (("fused", False), ("fused_details", True), ("fused_no_sums", False)):
        ms = statistics.median(times[name])
        nbytes = algorithmic_bytes(pixels, count, n_off, details, True)
        result[name] = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
                        "bytes_per_pixel_and_offset": round(nbytes / (count * pixels * n_off), 2), "algorithmic_GB": round(nbytes / 1e9, 4),
                        "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
    # peak memory of each route, from the same base
    peaks = {}
    for name, fn in (("fused", lambda: fused(False)), ("composition", composed)):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        del out
    ms = statistics.median(times["composition"])
    result["fused"]["peak_extra_GB"] = round(peaks["fused"] / 1e9, 4)
    result["composition"] = {"ms": round(ms, 4), "ms_min": round(min(times["composition"]), 4), "ms_max": round(max(times["composition"]), 4),
                             "peak_extra_GB": round(peaks["composition"] / 1e9, 4), "ratio_to_fused": round(ms / result["fused"]["ms"], 2)}
    r, (err, code) = fused(False), composed()
    same = (r.code == code) & (code == 0)
    result["codes_differing"] = int((r.code != code).sum())
    result["max_rel_diff_to_composition"] = float((r.error[same] - err[same]).norm() / err[same].norm().clamp_min(1e-30))
    result["fused_is_faster"] = result["fused"]["ms"] < result["composition"]["ms"]
    result["fused_allocates_less"] = peaks["fused"] < peaks["composition"]
    bc.emit(result, args.out)
    assert result["fused_is_faster"] and result["fused_allocates_less"], "the fused call must be faster than the composition and allocate less"


if __name__ == "__main__":
    main()
