"""Step time and kernel launches of a model with `extrinsics: regressed`, flow loss, on the MI355X: the fused module against the
path such a model took before it existed.

    python tools/bench_extrinsics_regressed.py --frames 150 --height 180 --width 240            # ms per step, both legs, alternating
    python tools/bench_extrinsics_regressed.py --frames 150 --height 180 --width 240 --launches  # kernel launches per step (rocprofv3)

Legs:
  new     flowmap_amd's ExtrinsicsRegressed (one launch forward, one backward; the fused flow loss reads its relative poses)
  parent  a plain-torch module with the reference's op sequence (extrinsics_regressed.py:17-39,72-83: eye, broadcast_to, contiguous,
          unbind / stack, two indexed writes, get_extrinsics — the latter this package's one-launch chain, as after install()) in the
          same Model, feeding the same fused flow loss, which then derives both relative poses from the chain (RelativePoses).
Both run lazy surfaces.  Timing: HIP events around ``--steps`` steps after ``--warmup`` (bench.py's loop), ``--rounds`` alternating rounds,
the median round per leg.  ``--launches`` starts, per leg, two rocprofv3 --kernel-trace --stats children (each under a time limit; the
first failure ends the run) that differ by 20 steps: launches per step = the difference of their kernel counts / 20.
No GPU, no number: the tool fails without one.
"""

from __future__ import annotations

import argparse
import csv
import json
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def reference_ops_module(num_frames):
    import torch
    from torch import nn

    from flowmap_amd.model.projection import get_extrinsics

    class ReferenceOpsExtrinsics(nn.Module):
        """The reference's ExtrinsicsRegressed restated op for op (the same ATen launches and autograd nodes)."""

        def __init__(self):
            super().__init__()
            self.translations = nn.Parameter(torch.zeros((num_frames - 1, 3), dtype=torch.float32))
            rotations = torch.zeros((num_frames - 1, 4), dtype=torch.float32)
            rotations[:, -1] = 1
            self.rotations = nn.Parameter(rotations)

        def forward(self, batch, flows, backbone_output, surfaces):
            device = surfaces.device
            b, f = surfaces.shape[:2]
            assert b == 1
            q = self.rotations
            i, j, k, r = torch.unbind(q, dim=-1)
            two_s = 2 / ((q * q).sum(dim=-1) + 1e-8)
            o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                             two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                             two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
            tf = torch.eye(4, dtype=torch.float32, device=device)
            tf = tf.broadcast_to((f - 1, 4, 4)).contiguous()
            tf[:, :3, :3] = o.reshape(-1, 3, 3)
            tf[:, :3, 3] = self.translations
            return get_extrinsics(tf)[None]

    return ReferenceOpsExtrinsics()


def make_step(leg, frames, height, width, device):
    import torch

    import flowmap_amd
    from flowmap_amd import Batch, Flows
    from flowmap_amd.loss import LossFlow, LossFlowCfg
    from flowmap_amd.loss.mapping import MappingHuberCfg
    from flowmap_amd.model.extrinsics_regressed import ExtrinsicsRegressedCfg
    from flowmap_amd.model.model import BackboneExplicitDepthCfg, IntrinsicsRegressedCfg, Model, ModelCfg

    g = torch.Generator(device=device).manual_seed(7)
    cfg = ModelCfg(BackboneExplicitDepthCfg("explicit_depth", 1.0, 100.0), IntrinsicsRegressedCfg("regressed", 0.85), ExtrinsicsRegressedCfg("regressed"))
    with torch.device("meta"):
        model = Model(cfg, num_frames=2, image_shape=(2, 2))
    model = model.to_empty(device=device)
    model.intrinsics.focal_length.data = torch.tensor(0.85, device=device)
    model.backbone.depth = torch.nn.Parameter(1.10 + 0.05 * torch.rand((frames, height, width), device=device, generator=g))
    model.backbone.weights = torch.nn.Parameter(torch.zeros((frames - 1, height, width), device=device))
    rotations = torch.zeros((frames - 1, 4), device=device)
    rotations[:, 3] = 1
    rotations += 0.02 * torch.randn((frames - 1, 4), device=device, generator=g)
    translations = 0.01 * torch.randn((frames - 1, 3), device=device, generator=g)
    model.extrinsics = (type(model.extrinsics)(cfg.extrinsics, frames) if leg == "new" else reference_ops_module(frames)).to(device)
    model.extrinsics.rotations.data, model.extrinsics.translations.data = rotations, translations
    pairs = (1, frames - 1, height, width)
    flows = Flows(0.01 * torch.randn((*pairs, 2), device=device, generator=g), 0.01 * torch.randn((*pairs, 2), device=device, generator=g),
                  (torch.rand(pairs, device=device, generator=g) > 0.3).float(), (torch.rand(pairs, device=device, generator=g) > 0.3).float())
    batch = Batch(torch.zeros((1, frames, 3, 1, 1), device=device).expand(1, frames, 3, height, width))
    loss_fn = LossFlow(LossFlowCfg(0, 1000.0, "flow", MappingHuberCfg("huber", 0.01)))
    flowmap_amd.set_lazy_surfaces(True)

    def step():
        model.zero_grad(set_to_none=True)
        out = model(batch, flows, 0)
        loss = loss_fn(batch, flows, None, out, 0)
        loss.backward()
        return loss

    return step, model


def timed(step, warmup, steps, device):
    import torch

    for _ in range(warmup):
        step()
    torch.cuda.synchronize(device)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        step()
    end.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(end) / steps


def run_timing(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_extrinsics_regressed: no GPU; nothing is measured without one")
    device = torch.device("cuda:0")
    legs = {}
    for leg in ("new", "parent"):
        legs[leg] = make_step(leg, args.frames, args.height, args.width, device)
    # same parameters, same inputs: the two legs compute the same step
    losses = {leg: float(step().detach()) for leg, (step, _) in legs.items()}
    grads = {leg: model.extrinsics.rotations.grad.detach().clone() for leg, (_, model) in legs.items()}
    agreement = float((grads["new"] - grads["parent"]).norm() / grads["parent"].norm())
    rounds = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg, (step, _) in legs.items():
            rounds[leg].append(timed(step, args.warmup, args.steps, device))
    result = {"tool": "bench_extrinsics_regressed", "frames": args.frames, "height": args.height, "width": args.width, "steps": args.steps,
              "warmup": args.warmup, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
              "loss": losses, "g_rotations_rel_diff_new_vs_parent": agreement}
    for leg in legs:
        result[f"ms_per_step_{leg}"] = statistics.median(rounds[leg])
        result[f"ms_per_step_{leg}_rounds"] = [round(x, 4) for x in rounds[leg]]
    print(json.dumps(result))


def run_leg(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_extrinsics_regressed: no GPU; nothing is measured without one")
    device = torch.device("cuda:0")
    step, _ = make_step(args.leg, args.frames, args.height, args.width, device)
    for _ in range(args.warmup + args.steps):
        step()
    torch.cuda.synchronize(device)


def kernel_calls(directory):
    """{kernel name: calls} summed over every *kernel_stats.csv rocprofv3 wrote under ``directory``."""
    calls = {}
    for path in Path(directory).rglob("*kernel_stats.csv"):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
    if not calls:
        raise SystemExit(f"bench_extrinsics_regressed: rocprofv3 left no kernel statistics under {directory}")
    return calls


def run_launches(args):
    extra = 20
    result = {"tool": "bench_extrinsics_regressed --launches", "frames": args.frames, "height": args.height, "width": args.width}
    for leg in ("new", "parent"):
        counts = []
        for steps in (args.steps, args.steps + extra):
            with tempfile.TemporaryDirectory(dir=args.scratch) as out:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "trace", "--", sys.executable, str(Path(__file__).resolve()),
                       "--leg", leg, "--frames", str(args.frames), "--height", str(args.height), "--width", str(args.width),
                       "--warmup", str(args.warmup), "--steps", str(steps)]
                done = subprocess.run(cmd, timeout=args.child_timeout, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if done.returncode != 0:  # (nothing more is started after a failure)
                    sys.stderr.write(done.stdout[-4000:])
                    raise SystemExit(f"bench_extrinsics_regressed: the {leg} leg under rocprofv3 ended with status {done.returncode}")
                counts.append(kernel_calls(out))
        short, long = counts
        per_step = (sum(long.values()) - sum(short.values())) / extra
        result[f"launches_per_step_{leg}"] = per_step
        result[f"kernels_per_step_{leg}"] = {name[:100]: (long[name] - short.get(name, 0)) / extra for name in sorted(long) if long[name] != short.get(name, 0)}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--width", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg", choices=("new", "parent"), default=None, help="run warmup + steps of one leg and print nothing (what --launches profiles)")
    ap.add_argument("--launches", action="store_true", help="kernel launches per step of both legs from rocprofv3 --kernel-trace --stats children")
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--scratch", default=None, help="where the rocprofv3 children write (a temporary directory below it; default: the system's)")
    args = ap.parse_args()
    if args.launches:
        run_launches(args)
    elif args.leg:
        run_leg(args)
    else:
        run_timing(args)


if __name__ == "__main__":
    main()
