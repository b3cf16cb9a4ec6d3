"""Time ExtrinsicsProcrustes.residuals on the GPU and, beside it, a torch composition producing the same maps.

    python tools/bench_alignment_residuals.py [--frames 150 --height 720 --width 1280] [--rounds 5] [--iters 20] [--out FILE]

The fused route: one fm_alignment_residuals launch (+ the ordered second stage of the sums) on lazy surfaces — every pixel of every pair
with and without the offsets, without the sums, a window of 8 pairs, and the default configuration's 1000 indices
(procrustes_indices) — timed with device events around ``iters`` calls after a warm-up.  The bytes the kernel has to move per element —
4 of the later depth, 8 of flow, 4 of weight, 4 of the earlier depth (four taps, shared between neighbouring pixels: once per pixel)
in, 4 (residual) + 12 (offset) out — over the time give the share of the 8 TB/s HBM peak; on indices the figure is a latency, not a rate.
The torch composition, for context: surfaces materialised with torch (K⁻¹·[x, y, 1]·depth), F.grid_sample (bilinear, border), matmul with
T, for every pixel, in windows of at most ``--torch-window`` frames (16: the reference's op sequence is on record as failing on stock
PyTorch-ROCm from 32 frames on, README), with the peak memory torch allocated for a window.  The two routes alternate, ``rounds`` times,
each measurement in a fresh child process under its own time limit; the first child that fails or runs out of time ends the run.  Prints
one JSON line (medians and the spread over the rounds); needs a GPU.  No test gates on its numbers.
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import _bench_common as bc  # noqa: E402
from _bench_common import HBM_PEAK, timed  # noqa: E402

READ_BYTES = 4 + 8 + 4 + 4  # later depth, flow, weight, earlier depth (once per pixel)
FUSED = ("dense", "dense_offsets", "dense_no_sums", "window8_offsets", "indices1000_offsets")


def torch_composition(depth, k, rel, bwd, weights, window):
    """offset, residual and the weighted sums of every pixel with torch operators, ``window`` frames at a time."""
    import torch
    import torch.nn.functional as F

    from flowmap_amd.model.projection import sample_image_grid

    b, f, h, w = depth.shape
    xy, _ = sample_image_grid((h, w), depth.device)
    xy1 = torch.cat((xy, torch.ones_like(xy[..., :1])), dim=-1)
    kinv = torch.linalg.inv(k)
    out = []
    for lo in range(0, f - 1, window - 1):
        hi = min(f - 1, lo + window - 1)  # pairs [lo, hi): frames [lo, hi]
        rays = torch.einsum("bfij,hwj->bfhwi", kinv[:, lo : hi + 1], xy1)
        surfaces = rays * depth[:, lo : hi + 1, :, :, None]
        n = hi - lo
        q = F.grid_sample(surfaces[:, :-1].reshape(b * n, h, w, 3).permute(0, 3, 1, 2), ((xy + bwd[:, lo:hi]) * 2 - 1).reshape(b * n, h, w, 2), mode="bilinear",
                          padding_mode="border", align_corners=False).permute(0, 2, 3, 1).reshape(b, n, h, w, 3)
        t = rel[:, lo:hi]
        offset = torch.einsum("bfij,bfhwj->bfhwi", t[..., :3, :3], surfaces[:, 1:]) + t[:, :, None, None, :3, 3] - q
        residual = (offset * offset).sum(-1)
        wt = weights[:, lo:hi]
        out.append((offset, residual, (wt * residual).double().sum(dim=(2, 3)), wt.double().sum(dim=(2, 3))))
    return out


def child(args):
    import torch

    assert torch.cuda.is_available(), "bench_alignment_residuals needs a GPU"
    from flowmap_amd import Batch, Flows, ModelOutput, _ops
    from flowmap_amd.model.extrinsics_procrustes import ExtrinsicsProcrustes, ExtrinsicsProcrustesCfg, procrustes_indices
    from flowmap_amd.model.projection import LazySurfaces

    dev = "cuda:0"
    f, h, w = args.frames, args.height, args.width
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 0.5 + 1.5 * torch.rand((1, f, h, w), device=dev, generator=g)
    k = torch.eye(3, device=dev).repeat(1, f, 1, 1)
    k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2] = 0.85, 1.1, 0.5, 0.5
    ext = torch.eye(4, device=dev).repeat(1, f, 1, 1)
    ext[0, :, 0, 3] = 0.002 * torch.arange(f, device=dev)
    bwd = 0.02 * torch.randn((1, f - 1, h, w, 2), device=dev, generator=g)
    weights = torch.rand((1, f - 1, h, w), device=dev, generator=g)
    n = h * w
    result = {"pixels_per_pair": n, "pairs": f - 1}
    if args.child == "fused":
        module = ExtrinsicsProcrustes(ExtrinsicsProcrustesCfg("procrustes", 1000, False), f)
        batch = Batch(torch.zeros((1, f, 3, 1, 1), device=dev).expand(1, f, 3, h, w))
        flows = Flows(None, bwd, None, None)
        out = ModelOutput(depth, LazySurfaces(depth, k), k, ext, weights)
        own = procrustes_indices(h, w, 1000, False, torch.device(dev))
        first = max(0, (f - 1) // 2 - 4)
        runs = {"dense": dict(), "dense_offsets": dict(offsets=True), "dense_no_sums": dict(sums=False),
                "window8_offsets": dict(pairs=(first, min(8, f - 1)), offsets=True), "indices1000_offsets": dict(indices=own, offsets=True)}
        for name in FUSED:
            kw = runs[name]
            ms = timed(lambda: module.residuals(batch, flows, out, **kw), args.iters)
            pairs = kw["pairs"][1] if "pairs" in kw else f - 1
            elements = pairs * (own.numel() if "indices" in kw else n)
            written = elements * (16 if kw.get("offsets") else 4)
            result[name] = {"ms": ms, "elements": elements, "written_MB": written / 1e6, "share_of_hbm_peak": (elements * READ_BYTES + written) / (ms * 1e-3) / HBM_PEAK}
    else:
        rel = _ops.RelativePoses.apply(ext)[1]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = timed(lambda: torch_composition(depth, k, rel, bwd, weights, args.torch_window), args.general_iters, warmup=1)
        result["dense_offsets"] = {"ms": ms, "window_frames": args.torch_window, "peak_extra_GB": (torch.cuda.max_memory_allocated() - base) / 1e9}
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
    ap.add_argument("--torch-window", type=int, default=16, help="frames the torch composition handles at a time")
    ap.add_argument("--step-timeout", type=float, default=90.0, help="seconds a single measurement (one child process) may take")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", choices=("fused", "torch"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    common = ["--frames", str(args.frames), "--height", str(args.height), "--width", str(args.width), "--iters", str(args.iters),
              "--general-iters", str(args.general_iters), "--torch-window", str(args.torch_window)]
    runs = bc.child_rounds("bench_alignment_residuals", __file__, common, ("fused", "torch"), args.rounds, args.step_timeout)
    first = runs["fused"][0]
    result = {"frames": args.frames, "height": args.height, "width": args.width, "device": first["device"], "rounds": args.rounds,
              "fused": {name: bc.summary(runs["fused"], name, scale_to_median=("share_of_hbm_peak",)) for name in FUSED},
              "torch": {"dense_offsets": bc.summary(runs["torch"], "dense_offsets")}}
    result["torch_over_fused"] = round(result["torch"]["dense_offsets"]["ms"] / result["fused"]["dense_offsets"]["ms"], 1)
    bc.emit(result, args.out)


if __name__ == "__main__":
    main()
