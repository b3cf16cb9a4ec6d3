"""Time projection.render_views on the GPU and, beside it, the same render composed from what a caller could write before
(DESIGN.md §3.1c).

    python tools/bench_render_views.py [--frames 150 --height 720 --width 1280 --window 8] [--iters 20] [--rounds 3] [--out FILE]

The fused route: fm_render_views — the z-buffer set to all-ones, one small launch for the pairs' relative poses, ONE pass over the
sources' depth with at most one 64-bit atomic minimum per live pixel, one resolve pass — in held-out mode on a window of ``--window`` frames in the
middle of the video at offsets (−2, −1, 1, 2), radius 0, output at the source shape, coloured, timed with device events around ``iters``
calls after a warm-up.  The composition: per (view, source) ``unproject`` (materialised points), ``reproject_points`` for the positions,
the third row of the same transform in torch for q.z, an int64 key per source pixel in torch, ``scatter_reduce_(amin)`` into an int64
z-buffer, then the decode and the colour gather in torch — timed the same way in the same process, alternating with the fused route over
``--rounds`` rounds, with the peak memory torch allocated for each.  No ratio is promised.  Beside the times it records the algorithmic
bytes of the call and the number of live source pixels (counted by the composition) — each a candidate key, lowered into the z-buffer
with an atomic minimum unless the key already there is smaller — with the rate of keys they imply over the WHOLE call; the kernel's own
time is in the rocprofv3 summary.  No figure for 64-bit integer minima existed before this file;
the float-atomic figure of the micro-architecture guide (about 1.3 TB/s of added bytes) stands beside it for context only.  Prints one
JSON line; needs a GPU.
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
LAUNCHES = 4  # the fill, the pose rows, the splat pass, the resolve pass
FLOAT_ATOMIC_ADD_BYTES_PER_S = 1.3e12  # (the guide's chip-wide figure for float atomic adds: context, not a bound on 64-bit minima)


def algorithmic_bytes(pixels, n_pairs, targets, live):
    """Bytes the call has to move: 4 of depth per source pixel of every pair, 8 of key per live source pixel, and per target pixel 8 of fill, 8 of
    key read, 12 of colour gathered and 12 + 4 + 4 of colour, depth and source written."""
    return n_pairs * pixels * 4 + live * 8 + targets * (8 + 8 + 12 + 20)


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
    assert torch.cuda.is_available(), "bench_render_views needs a GPU"

    from flowmap_amd import render_views
    from flowmap_amd.model.projection import reproject_points, sample_image_grid, unproject_dense

    dev = "cuda:0"
    f, h, w, count = args.frames, args.height, args.width, args.window
    first = (f - count) // 2
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 1.5 + 0.5 * torch.rand((1, f, h, w), device=dev, generator=g)
    colors = torch.rand((1, f, 3, h, w), device=dev, generator=g)
    k = torch.eye(3, device=dev).repeat(1, f, 1, 1)
    k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2] = 0.85, 1.1, 0.5, 0.5
    ext = torch.eye(4, device=dev).repeat(1, f, 1, 1)
    ext[0, :, 0, 3] = 0.02 * torch.arange(f, device=dev)
    ext[0, :, 2, 3] = 0.005 * torch.arange(f, device=dev)
    xy, _ = sample_image_grid((h, w), dev)
    n = h * w
    pairs = [(v, first + v + d) for v in range(count) for d in OFFSETS if 0 <= first + v + d < f]
    hole = torch.iinfo(torch.int64).max
    index = torch.arange(n, device=dev)

    def fused():
        return render_views(depth, k, ext, colors, held_out=(first, count), offsets=OFFSETS)

    def composed(count_live=False):
        """source, depth and color of the same views from the existing operators, one (view, source) at a time."""
        with torch.no_grad():
            zbuf = torch.full((count, n), hole, dtype=torch.int64, device=dev)
            live_total = 0
            for view, src in pairs:
                j = first + view
                points = unproject_dense(xy, depth[:, src], k[:, src][:, None, None])  # (1, h, w, 3)
                rel = (torch.linalg.inv(ext[:, j].double()) @ ext[:, src].double()).float()
                uv = reproject_points(points, rel[:, None, None], k[:, j][:, None, None])
                qz = (points * rel[:, None, None, 2, :3]).sum(-1) + rel[:, None, None, 2, 3]
                live = ((qz > 0) & (uv >= 0).all(-1) & (uv < 1).all(-1)).reshape(n)
                tx = torch.floor(uv[..., 0] * w).clamp(0, w - 1).long().reshape(n)
                ty = torch.floor(uv[..., 1] * h).clamp(0, h - 1).long().reshape(n)
                key = (qz.contiguous().view(torch.int32).long().reshape(n) << 32) | (src * n + index)
                zbuf[view].scatter_reduce_(0, torch.where(live, ty * w + tx, torch.zeros_like(tx)), torch.where(live, key, torch.full_like(key, hole)), "amin")
                if count_live:
                    live_total += int(live.sum())
            holes = zbuf == hole
            winner = torch.where(holes, torch.zeros_like(zbuf), zbuf & 0xFFFFFFFF)
            source = torch.where(holes, torch.full_like(zbuf, -1), winner).to(torch.int32).reshape(1, count, h, w)
            out_depth = torch.where(holes, torch.zeros_like(zbuf), zbuf >> 32).to(torch.int32).view(torch.float32).reshape(1, count, h, w)
            planes = colors[0].permute(1, 0, 2, 3).reshape(3, 1, f * n).expand(3, count, f * n)
            color = torch.gather(planes, 2, winner[None].expand(3, count, n))
            color = torch.where(holes[None], torch.zeros_like(color), color).permute(1, 0, 2).reshape(1, count, 3, h, w)
            return (source, out_depth, color, live_total) if count_live else (source, out_depth, color)

    result = {"frames": f, "height": h, "width": w, "held_out": [first, count], "offsets": list(OFFSETS), "radius": 0, "pairs": len(pairs),
              "device": torch.cuda.get_device_name(0), "launches": LAUNCHES, "iters": args.iters, "rounds": args.rounds}
    for fn in (fused, composed):  # a warm-up of every shape timed
        fn()
    torch.cuda.synchronize()
    times = {"fused": [], "composition": []}
    for _ in range(args.rounds):  # alternating, in one process
        times["fused"].append(bc.timed(fused, args.iters, warmup=1))
        times["composition"].append(bc.timed(composed, max(1, args.iters // 4), warmup=1))
    peaks = {}
    for name, fn in (("fused", fused), ("composition", composed)):  # peak memory of each route, from the same base
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        del out
    r = fused()
    source, out_depth, color, live = composed(count_live=True)
    same = r.source == source
    result["sources_differing"] = int((~same).sum())  # (the composition's positions are another fp32 evaluation: ties near a bin's edge)
    result["depth_bits_differing_on_equal_sources"] = int((r.depth[same] != out_depth[same]).sum())
    result["colors_equal_on_equal_sources"] = bool(torch.equal(r.color.permute(0, 1, 3, 4, 2)[same], color.permute(0, 1, 3, 4, 2)[same]))
    result["coverage"] = [round(float(v), 4) for v in r.coverage()[0]]
    ms = statistics.median(times["fused"])
    nbytes = algorithmic_bytes(n, len(pairs), count * n, live)
    result["fused"] = {"ms": round(ms, 4), "ms_min": round(min(times["fused"]), 4), "ms_max": round(max(times["fused"]), 4),
                       "peak_extra_GB": round(peaks["fused"] / 1e9, 4), "algorithmic_GB": round(nbytes / 1e9, 4),
                       "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3), "live_source_pixels": live,
                       "key_GB_per_s_over_the_whole_call": round(live * 8 / (ms * 1e-3) / 1e9, 1),
                       "guide_float_atomic_add_GB_per_s_for_context": FLOAT_ATOMIC_ADD_BYTES_PER_S / 1e9}
    ms_c = statistics.median(times["composition"])
    result["composition"] = {"ms": round(ms_c, 4), "ms_min": round(min(times["composition"]), 4), "ms_max": round(max(times["composition"]), 4),
                             "peak_extra_GB": round(peaks["composition"] / 1e9, 4), "ratio_to_fused": round(ms_c / ms, 2)}
    bc.emit(result, args.out)


if __name__ == "__main__":
    main()
