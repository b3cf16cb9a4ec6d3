"""Time LossFlow.residuals on the GPU and, beside it, the general path producing the same maps.

    python tools/bench_flow_residuals.py [--frames 150 --height 720 --width 1280] [--iters 20] [--out FILE]

The fused route: one fm_flow_residuals launch (+ the ordered second stage of the sums) over depth, with and without the predicted
flows, timed with device events around ``iters`` calls after a warm-up; its algorithmic bytes per pixel and pair — 4 + 4 depth, 16 flows,
8 masks read, 8 (24 with the predicted flows) written — over the time give the share of the 8 TB/s HBM peak.  The general route:
compute_forward_flow / compute_backward_flow over explicit surfaces -> mapping.forward, the operators a caller had before this method
existed (they are unchanged by it), timed the same way, with the peak memory torch allocated for it.  Prints one JSON line; needs a GPU.
"""

from __future__ import annotations

import argparse
import functools
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import _bench_common as bc  # noqa: E402
from _bench_common import HBM_PEAK  # noqa: E402

timed = functools.partial(bc.timed, warmup=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--general-iters", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_flow_residuals needs a GPU"

    from flowmap_amd import Batch, Flows, ModelOutput
    from flowmap_amd.loss import LossFlow, LossFlowCfg
    from flowmap_amd.loss.mapping import MappingHuberCfg
    from flowmap_amd.model.projection import LazySurfaces, compute_backward_flow, compute_forward_flow, sample_image_grid

    dev = "cuda:0"
    f, h, w = args.frames, args.height, args.width
    g = torch.Generator(device=dev).manual_seed(0)
    depth = 0.5 + 1.5 * torch.rand((1, f, h, w), device=dev, generator=g)
    k = torch.eye(3, device=dev).repeat(1, f, 1, 1)
    k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2] = 0.85, 1.1, 0.5, 0.5
    ext = torch.eye(4, device=dev).repeat(1, f, 1, 1)
    ext[0, :, 0, 3] = 0.02 * torch.arange(f, device=dev)
    flows = Flows(*(0.02 * torch.randn((1, f - 1, h, w, 2), device=dev, generator=g) for _ in range(2)),
                  *(torch.rand((1, f - 1, h, w), device=dev, generator=g) for _ in range(2)))
    batch = Batch(torch.zeros((1, f, 3, 1, 1), device=dev).expand(1, f, 3, h, w))
    loss = LossFlow(LossFlowCfg(0, 1.0, "flow", MappingHuberCfg("huber", 0.01)))
    out = ModelOutput(depth, LazySurfaces(depth, k), k, ext, None)
    px_pairs = (f - 1) * h * w
    result = {"frames": f, "height": h, "width": w, "device": torch.cuda.get_device_name(0)}

    for name, pred, written in (("residuals", False, 8), ("residuals_predicted_flow", True, 24)):
        ms = timed(lambda: loss.residuals(batch, flows, out, predicted_flow=pred), args.iters)
        nbytes = px_pairs * (4 + 4 + 16 + 8 + written)
        result[name] = {"ms": round(ms, 4), "algorithmic_GB": round(nbytes / 1e9, 3), "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
    ms = timed(lambda: loss.residuals(batch, flows, out, sums=False), args.iters)
    nbytes = px_pairs * (4 + 4 + 16 + 8)
    result["residuals_no_sums"] = {"ms": round(ms, 4), "algorithmic_GB": round(nbytes / 1e9, 3), "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
    ms = timed(lambda: loss.residuals(batch, flows, out, pairs=(f // 2, 8), predicted_flow=True), args.iters)
    result["window_of_8_pairs_predicted_flow"] = {"ms": round(ms, 4)}
    fused = loss.residuals(batch, flows, out)

    # the general path: the operators a caller had before (surfaces materialised, positions, mapping), with no_grad like the method
    xy, _ = sample_image_grid((h, w), dev)

    def general():
        with torch.no_grad():
            surfaces = LazySurfaces(depth, k).materialize()
            fwd = loss.mapping.forward(compute_forward_flow(surfaces, ext, k) - xy, flows.forward, (h, w))
            bwd = loss.mapping.forward(compute_backward_flow(surfaces, ext, k) - xy, flows.backward, (h, w))
            return fwd, bwd

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(general, args.general_iters, warmup=1)
    result["general_path"] = {"ms": round(ms, 3), "peak_extra_GB": round((torch.cuda.max_memory_allocated() - base) / 1e9, 3),
                              "ratio_to_residuals": round(ms / result["residuals"]["ms"], 1)}
    fwd, bwd = general()
    result["max_rel_diff_to_general"] = max(float((a - b).norm() / b.norm()) for a, b in ((fused.forward, fwd), (fused.backward, bwd)))
    bc.emit(result, args.out)


if __name__ == "__main__":
    main()
