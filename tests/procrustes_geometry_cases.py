"""The Procrustes fit ALONE (csrc/fm_procrustes.hip: the generic moments / scatter kernels, the one-block-per-pair fit, the multi-block
elected fit with its self-cleaning workspace, both in-fit pose chains, the one-launch planned backward and its three-launch twin, the
repeated-batch scatter, the tiled dense kernels with their static tap lists, the 64-thread per-pair kernels, fm_procrustes_stats) at
every edge of its launch geometry.  Shared by the CPU (host double) and GPU modules: the host double loops where the kernels launch, so
only the GPU module says anything about blocks, waves, tiles, the XCD dealing and the elections; the CPU module proves the cases, their
reference and the input conditions.

Truth is a plain fp64 evaluation with oracle.flowmap_oracle — lift -> gather / bilinear_border -> rigid_fit on sigmoid(100·logit) weights,
chain_poses where the call returns the extrinsics — under seeded cotangents on t_bwd and t_fwd (zero last row) and on the extrinsics, with
autograd's gradients w.r.t. depth, logits and a per-frame K (surfaces and weights for surface-sourced fits); ``ref32`` is the same function
in torch fp32.  Gates, all the project's own: poses and extrinsics assert_close(1e-5); gradients assert_close_or_reference_gap(1e-4);
dense dL/ddepth and dL/dlogits additionally max-abs <= 10·TOL; planned vs atomic 2e-5 / 1e-7; a repeated planned step 1e-6 / 1e-9.
Every figure is printed before it is asserted.

Input conditions: nothing is masked or left out of a comparison (the share of excluded elements is 0).  ``check_conditions`` asserts per
case that ref32 is itself within 1e-4 of the truth (a seed for which the reference misses is a bad case, not a kernel finding), and, for
the dense tap lists, that no sample lies within PLAN_MARGIN pixels of a coordinate that decides which tiles list it.

Two cases are not what a list of sizes alone would give: the flow that fills ONE tile's list contracts the image about
that tile's centre (a collapse onto one point leaves the fit rank 0 and the reference undefined), and the sizes whose last block holds
one live point come a second time with that point made heavy (among 65 537 equal weights it moves nothing by more than a gate).

Every run asserts the backward form it claims to test from the operator library's own counters (_ops.FIT_BACKWARD_FORMS), and after
every chained call that the fit's persistent workspace is all zero."""

from __future__ import annotations

import contextlib
import dataclasses
import re
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from conftest import assert_close, assert_close_or_reference_gap, maxerr, relerr
from oracle import flowmap_oracle as orc

ROOT = Path(__file__).resolve().parent.parent

# ---- the constants of csrc/fm_procrustes.hip the lists below straddle (case_constants checks them against the sources) -----------------
ONE_BLOCK_POINTS = 4096  # fit_chain_launch: up to here one 1024-thread block per pair (and the limit of the static tap records)
ITERS_POINTS = 65536  # choose_iters: beyond it a thread of the generic moments / scatter kernels takes 8 points
ITERS_LARGE = 8
FIT_BWD_MAX_POINTS = 2048  # FM_FIT_BWD_MAX_POINTS: the one-launch planned backward
FIT_BWD_THREADS, FIT_BWD_GATHER = 512, 10  # kFitBwdThreads x kFitBwdGather plan pixels per trip of a frame block's gather loop
TILE_H, TILE_W = 32, 64  # FM_DENSE_TILE_H x FM_DENSE_TILE_W
XCDS = 8  # kXcds: the dense grid is padded to a multiple
SORT_CHUNK = 4096  # kSortChunk: a tile list is sorted in chunks of this many entries
TAP_BATCH = 6  # FM_DENSE_TAP_BATCH x 256 list entries per batch of the tap kernel
REPEAT_GROUP = 6  # kRepeatGroup: candidates per block of the repeated-batch scatter
CHAIN_THREADS = 256  # kChainThreads: the stand-alone pose chain
CHAIN_CHUNKS = 64  # the in-fit chains: one wave, 64 chunks
PAIR_BLOCK = 64  # the per-pair kernels: 64 pairs (or frames) per block
POINT_BLOCK, PAIR_FIT_BLOCK = 256, 1024  # generic moments / scatter block; the one-block-per-pair fit

SENS = 100.0
TOL = 1e-4
POSE_TOL = 1e-5
PLAN_REL, PLAN_ABS = 2e-5, 1e-7  # planned vs atomic (cases.case_procrustes_planned_backward)
REPEAT_REL, REPEAT_ABS = 1e-6, 1e-9  # a repeated planned step
STATS_FLOOR = 1e-5  # point_function_cases.FLOOR_RIGID, norm-wise and element-wise (case_rigid_stats_abi)
PLAN_MARGIN = 1e-6  # of the image size, in pixels: dense_taps forms a coordinate below `size` in about six fp32 roundings, good to ~4e-7·size

FORMS = ("one_launch", "three_launch", "atomic", "dense_fused", "dense_planned", "repeat")
FAMILIES = ("sparse", "large-P", "dense", "surfaces", "repeat", "chain")


# ---- the lists ------------------------------------------------------------------------------------------------------------------------------


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    family: str
    hw: tuple
    points: Optional[int]  # None: every pixel a correspondence (indices=None)
    f: int = 3
    b: int = 1
    dup: bool = False  # indices drawn with replacement (never planned)
    source: str = "depth"  # or "surfaces" (lazy=False)
    flow: str = "iid"  # iid | shift | contract
    sigma: float = 0.01
    repeat: int = 1
    window: bool = False  # depth, flows and weights are [:, 1:4] / [:, 1:3] windows of six- / five-frame stacks
    spike: bool = False  # the LAST correspondence alone sits on the last pixel and carries weight ~1 among weights ~0.007
    seed: int = 0

    @property
    def pairs(self):
        return self.b * self.repeat * (self.f - 1)

    @property
    def plans(self):  # a static backward plan is possible
        return self.source == "depth" and self.points is not None and not self.dup and self.repeat == 1

    @property
    def chains(self):  # apply_chained(chain=True) takes fm_procrustes_fit_chain
        return self.points is not None and self.repeat == 1


def spec_id(spec):
    return spec.name


# 1. distinct sorted indices on 64 x 80 = 5120 pixels:
#   3, 4                 the least the fit takes; one lane and a few
#   63, 64, 65           the wave
#   255, 256, 257        the 256-thread block of the generic moments / scatter / plan kernels
#   511 .. 1537          SLOTS 1 -> 2 -> 3 -> 4 of the one-launch backward (512 threads); 1023, 1024, 1025 also the second stride of the
#                        1024-thread pair block
#   2047, 2048, 2049     the last one-launch planned backward and the first three-launch one
#   4095, 4096, 4097     the last one-block fit (tap-record limit) and the first elected fit, 17 blocks per pair
POINTS = (3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 4095, 4096, 4097)
POINT_CASES = tuple(Spec(f"P{p}", "sparse", (64, 80), p, seed=p) for p in POINTS)

# 2. past choose_iters' threshold, indices with duplicates on 24 x 32: iters 1 -> 8, a last block with one live point (65 537 = 32·2048 + 1),
#    33 full blocks and one point (67 585)
LARGE_POINTS = (65535, 65536, 65537, 67585)
LARGE_CASES = tuple(Spec(f"dupP{p}", "large-P", (24, 32), p, dup=True, seed=p) for p in LARGE_POINTS)
#    ... and, beyond the issue's list, the two sizes whose last block holds ONE live point with that point made heavy: one point in 65 537 of
#    equal weight moves the poses by 1e-5 and the gradients' norms by less, which no gate sees (a host double that dropped the point passed)
SPIKE_CASES = tuple(Spec(f"dupP{p}-spike", "large-P", (24, 32), p, dup=True, spike=True, seed=p + 1) for p in (65537, 67585))

# 3. a frame's plan slice longer than kFitBwdThreads·kFitBwdGather = 5120 pixels: a second trip of the gather loop
LONG_SLICE = Spec("slice-96x128-P2048", "sparse", (96, 128), 2048, seed=31)

# 4. frames and batch
TWO_FRAME_CASES = tuple(Spec(f"f2-P{p}", "sparse", (64, 80), p, f=2, seed=40 + p) for p in (65, 513))
BATCHED = Spec("b2-f4-P257", "sparse", (64, 80), 257, f=4, b=2, seed=41)
BATCHED_DENSE = Spec("dense-b2-f4-33x65", "dense", (33, 65), None, f=4, b=2, seed=42)
#    pairs next to a 64-thread block (f = 64, 65, 66: 63, 64, 65 pairs; 64, 65, 66 frames for pose_solve_bwd_kinv) and the in-fit
#    one-wave chain's 64 chunks (1, 63, 64, 65, 129 steps)
CHAIN_PAIRS = (1, 63, 64, 65, 129)
CHAIN_CASES = tuple(Spec(f"pairs{n}-P40", "chain", (8, 12), 40, f=n + 1, seed=400 + n) for n in CHAIN_PAIRS)
PAIR_DENSE_CASES = tuple(Spec(f"dense-pairs{n}", "dense", (8, 12), None, f=n + 1, seed=500 + n) for n in (63, 64, 65))  # 65 blocks -> grid 72
ELECTED_CHAIN_CASES = tuple(Spec(f"pairs{n}-dupP4097", "chain", (8, 12), 4097, f=n + 1, dup=True, seed=600 + n) for n in (65, 129))

# 6. dense, depth-sourced, indices=None
#    one tile less a row and a column, exactly one, one more of each; odd widths (scalar staging) and width % 4 == 2; less than a tile; 2 x 2 tiles
DENSE_SHAPES = ((31, 63), (32, 64), (33, 65), (32, 66), (32, 68), (16, 20), (64, 128))
DENSE_CASES = tuple(Spec(f"dense-{h}x{w}-s{s}", "dense", (h, w), None, sigma=s, seed=h * w + int(100 * s) + 5) for h, w in DENSE_SHAPES for s in (0.01, 0.5))
#    tiles x pairs next to kXcds: 1, 7, 8, 9 blocks (seeds here and above: the first that meet PLAN_MARGIN)
XCD_SHAPES = ((32, 64, 2), (32, 448, 2), (64, 128, 3), (32, 192, 4))
XCD_CASES = tuple(Spec(f"dense-{h}x{w}-f{f}", "dense", (h, w), None, f=f, seed=700) for h, w, f in XCD_SHAPES)
#    a window wholly off the image; every sample in ONE tile (a list of 8192 entries: two sort chunks, more than five tap batches) and
#    three empty lists
SHIFT_CASES = tuple(Spec(f"dense-{h}x{w}-shift", "dense", (h, w), None, flow="shift", seed=800 + w) for h, w in ((33, 65), (32, 66)))
CONTRACT = Spec("dense-64x128-contract", "dense", (64, 128), None, flow="contract", seed=810)
ALL_DENSE = DENSE_CASES + XCD_CASES + SHIFT_CASES + (CONTRACT, BATCHED_DENSE) + PAIR_DENSE_CASES

# 7. surface-sourced (lazy=False): gradients w.r.t. surfaces and weights; indices=None on 258 x 256 = 66 048 points goes through the
#    generic kernels with iters = 8 (32 full blocks and one whose threads take one or two live strides)
SURFACE_CASES = tuple(Spec(f"surf-P{p}", "surfaces", (64, 80), p, source="surfaces", seed=900 + p) for p in (65, 257, 4097)) + (
    Spec("surf-258x256-all", "surfaces", (258, 256), None, source="surfaces", seed=950),)

# 8. batch repeat (kRepeatGroup = 6: one group less one, exactly, one more; two groups and one more) x the 256-thread block
REPEATS = (2, 5, 6, 7, 12, 13)
REPEAT_CASES = tuple(Spec(f"R{r}-P{p}", "repeat", (24, 32), p, repeat=r, seed=1000 + 10 * r + p % 10) for r in REPEATS for p in (255, 256, 257)) + (
    Spec("b2-R7-P256", "repeat", (24, 32), 256, b=2, repeat=7, seed=1100),)

# 9. frame windows read in place (two batch entries: with one, a frame window is contiguous)
WINDOW_CASES = tuple(Spec(f"window-P{p}", "sparse", (64, 80), p, b=2, window=True, seed=1200 + p) for p in (65, 4097))

# 10. statistics only
STATS_CASES = tuple(Spec(f"stats-P{p}", "sparse", (8, 12), p, f=66, seed=1300 + p) for p in (64, 65))

# 11. the chained fit's workspace over three calls on changing depth
REUSE_CASES = tuple(Spec(f"reuse-P{p}", "sparse", (64, 80), p, seed=1400 + p) for p in (4097, 1000))

SPARSE_CASES = POINT_CASES + (LONG_SLICE,) + TWO_FRAME_CASES + (BATCHED,) + CHAIN_CASES + WINDOW_CASES
ATOMIC_ONLY_CASES = LARGE_CASES + SPIKE_CASES + ELECTED_CHAIN_CASES
ALL_CASES = SPARSE_CASES + ATOMIC_ONLY_CASES + ALL_DENSE + SURFACE_CASES + REPEAT_CASES + REUSE_CASES
SPECS = {s.name: s for s in ALL_CASES + STATS_CASES}
assert len(SPECS) == len(ALL_CASES) + len(STATS_CASES)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------

_INPUTS: dict = {}
_REFS: dict = {}


def make_inputs(spec) -> dict:
    """cases.case_dense_procrustes' inputs: depth 1 + 0.3·U, K = focal_to_k(0.85) + 0.01·N per frame (per candidate: its own focal length as
    well), logits 0.01·N, flows sigma·N in normalised units — fp32, CPU, computed once and never written to."""
    if spec.name in _INPUTS:
        return _INPUTS[spec.name]
    g = torch.Generator().manual_seed(10_000 + spec.seed)
    b, f, (h, w), rep = spec.b, spec.f, spec.hw, spec.repeat
    n = h * w
    stack = 6 if spec.window else f
    x = {"depth": 1.0 + 0.3 * torch.rand((b, stack, h, w), generator=g)}
    focal = torch.full((b * rep,), 0.85) if rep == 1 else (0.7 + 0.3 * torch.arange(b * rep) / (b * rep)).float()
    x["k"] = orc.focal_to_k(focal, (h, w))[:, None].repeat(1, f, 1, 1) + 0.01 * torch.randn((b * rep, f, 3, 3), generator=g)
    if spec.flow == "iid":
        flow = spec.sigma * torch.randn((b, stack - 1, h, w, 2), generator=g)
    elif spec.flow == "shift":
        flow = torch.tensor([0.9, -0.9]).expand(b, stack - 1, h, w, 2).contiguous()
    else:  # every sample inside tile (0, 0): the image shrunk to 0.4 of its size about the tile's centre
        xy, _ = orc.pixel_grid((h, w))
        centre = torch.tensor([TILE_W / 2 / w, TILE_H / 2 / h])
        flow = (centre + 0.4 * (xy - 0.5) - xy).expand(b, stack - 1, h, w, 2) + 0.002 * torch.randn((b, stack - 1, h, w, 2), generator=g)
    x["flow"] = flow.contiguous()
    x["logits"] = 0.01 * torch.randn((b, stack - 1, h, w), generator=g)
    if spec.source == "surfaces":
        xy, _ = orc.pixel_grid((h, w))
        x["surfaces"] = orc.lift(xy, x["depth"], x["k"][:, :, None, None]).contiguous()
        x["weights"] = 0.2 + 0.8 * torch.rand((b, f - 1, h, w), generator=g)
    if spec.points is None:
        x["idx"] = None
    elif spec.dup:
        x["idx"] = torch.randint(0, n - 1 if spec.spike else n, (spec.points,), generator=g)
        if spec.spike:
            x["idx"][-1] = n - 1
            x["logits"] -= 0.05  # sigmoid(-5) = 0.0067
            x["logits"].reshape(b, stack - 1, n)[..., n - 1] = 0.05  # sigmoid(5) = 0.9933
    else:
        assert spec.points <= n
        x["idx"] = torch.randperm(n, generator=g)[: spec.points].sort().values
    for name, frames in (("cot_b", f - 1), ("cot_f", f - 1), ("cot_e", f)):
        x[name] = torch.randn((b * rep, frames, 4, 4), generator=g)
        x[name][..., 3, :] = 0
    _INPUTS[spec.name] = x
    return x


def _window(spec, t, frames):
    return t[:, 1 : 1 + frames] if spec.window else t


def _evaluate(spec, x, dtype, with_ext):
    """The reference: (poses, gradients) of Σ t_bwd·cot_b + Σ t_fwd·cot_f [+ Σ extrinsics·cot_e] in ``dtype`` on the CPU."""
    b, f, (h, w), rep = spec.b, spec.f, spec.hw, spec.repeat
    n = h * w
    xy, _ = orc.pixel_grid((h, w), dtype=dtype)
    flow = _window(spec, x["flow"], f - 1).to(dtype).repeat_interleave(rep, dim=0)
    if spec.source == "depth":
        depth, k, logits = (x[name].to(dtype).clone().requires_grad_(True) for name in ("depth", "k", "logits"))
        leaves = {"g_depth": depth, "g_k": k, "g_logits": logits}
        surfaces = orc.lift(xy, _window(spec, depth, f).repeat_interleave(rep, dim=0), k[:, :, None, None])
        weights = (SENS * _window(spec, logits, f - 1)).sigmoid().repeat_interleave(rep, dim=0)
    else:
        surfaces, weights = (x[name].to(dtype).clone().requires_grad_(True) for name in ("surfaces", "weights"))
        leaves = {"g_surfaces": surfaces, "g_weights": weights}
    later = surfaces[:, 1:].reshape(b * rep, f - 1, n, 3)
    where = (xy + flow).reshape(b * rep, f - 1, n, 2)
    wts = weights.reshape(b * rep, f - 1, n)
    if x["idx"] is not None:
        later, where, wts = later[:, :, x["idx"]], where[:, :, x["idx"]], wts[..., x["idx"]]
    rel = orc.rigid_fit(later, orc.bilinear_border(surfaces[:, :-1], where), wts)
    inv = torch.linalg.inv(rel)
    out = {"t_bwd": rel.detach(), "t_fwd": inv.detach()}
    loss = (rel * x["cot_b"].to(dtype)).sum() + (inv * x["cot_f"].to(dtype)).sum()
    if with_ext:
        ext = orc.chain_poses(rel)
        out["ext"] = ext.detach()
        loss = loss + (ext * x["cot_e"].to(dtype)).sum()
    loss.backward()
    out.update({name: leaf.grad for name, leaf in leaves.items()})
    return out


def reference(spec, with_ext=False, x=None):
    """(truth, ref32): computed once per (case, with / without the chain) and shared; with ``x`` (changed inputs) computed afresh."""
    key = (spec.name, with_ext)
    if x is not None:
        return tuple(_evaluate(spec, x, dtype, with_ext) for dtype in (torch.float64, torch.float32))
    if key not in _REFS:
        _REFS[key] = tuple(_evaluate(spec, make_inputs(spec), dtype, with_ext) for dtype in (torch.float64, torch.float32))
    return _REFS[key]


def check_conditions(spec):
    """The input condition: the fp32 reference is itself within the gates of the fp64 truth, on every quantity, with nothing left out."""
    for with_ext in ((False, True) if spec.chains else (False,)):
        truth, ref32 = reference(spec, with_ext)
        for key, value in truth.items():
            assert bool(torch.isfinite(value).all()), f"{spec.name}: fp64 {key} is not finite"
            gap = relerr(ref32[key], value)
            print(f"[{spec.name} ext={with_ext}] fp32 reference vs fp64: {key} {gap:.2e}", flush=True)
            assert gap <= (POSE_TOL if key in ("t_bwd", "t_fwd", "ext") else TOL), f"{spec.name}: the fp32 reference misses {key}: {gap:.3e} (a bad case)"
        if spec.family == "dense":
            for key in ("g_depth", "g_logits"):
                assert maxerr(ref32[key], truth[key]) <= 10 * TOL, f"{spec.name}: the fp32 reference misses {key} in max-abs (a bad case)"
            expected_tile_lists(spec, make_inputs(spec)["flow"])  # (asserts PLAN_MARGIN)


# ---- running ours ------------------------------------------------------------------------------------------------------------------------------

FIGURES: dict = {}  # family -> quantity -> (worst of ours, the reference's own fp32 gap of that comparison)


def forms_now():
    from flowmap_amd import _ops

    return tuple(_ops.counters[name] for name in _ops.FIT_BACKWARD_FORMS)


class Runner:
    """One case on one device: the flow and index tensors stay the same objects from call to call (the static plans are keyed by them);
    depth, K and logits are fresh leaves every call."""

    def __init__(self, dev, spec, arange=False):
        self.dev, self.spec, self.x = dev, spec, make_inputs(spec)
        self.flow = _window(spec, self.x["flow"].clone().to(dev), spec.f - 1)
        idx = torch.arange(spec.hw[0] * spec.hw[1]) if arange else self.x["idx"]
        self.idx = None if idx is None else idx.clone().to(dev)
        assert not spec.window or not self.flow.is_contiguous()

    def workspace(self):
        slot = self.flow.__dict__.get("_fm_fit_work")
        return None if slot is None else slot[1]

    def plan(self):
        (entry,) = self.flow.__dict__["_fm_sparse_plans"].values()
        return entry[1]

    def __call__(self, mode="apply", expect=None, dense_plan=None, depth=None):
        """mode: apply (fm_procrustes_fit) | chained (fm_procrustes_fit_chain with the extrinsics) | chained_noext.  -> results on the CPU."""
        from flowmap_amd import _ops, config

        spec, x, dev = self.spec, self.x, self.dev
        out, leaves = {}, {}
        if spec.source == "depth":
            for name, src in (("g_depth", x["depth"] if depth is None else depth), ("g_k", x["k"]), ("g_logits", x["logits"])):
                leaves[name] = src.clone().to(dev).requires_grad_(True)
            args = (_window(spec, leaves["g_depth"], spec.f), leaves["g_k"], None, _window(spec, leaves["g_logits"], spec.f - 1))
            assert not spec.window or not args[0].is_contiguous()
            sens = SENS
        else:
            leaves = {"g_surfaces": x["surfaces"].clone().to(dev).requires_grad_(True), "g_weights": x["weights"].clone().to(dev).requires_grad_(True)}
            args, sens = (None, None, leaves["g_surfaces"], leaves["g_weights"]), 0.0
        before = forms_now()
        with config.override(dense_plan=dense_plan) if dense_plan is not None else contextlib.nullcontext():
            t_bwd, t_fwd, ext = _ops.ProcrustesFit.apply_chained(*args, self.flow, self.idx, sens, spec.repeat, chain=mode != "apply",
                                                                 want_extrinsics=mode == "chained")
        assert (ext is not None) == (mode == "chained" and spec.chains), (spec.name, mode)
        work = self.workspace()
        if mode != "apply" and spec.chains:
            assert work is not None and not bool(work.any()), f"{spec.name} {mode}: the fit left its workspace dirty"
        loss = (t_bwd * x["cot_b"].to(dev)).sum() + (t_fwd * x["cot_f"].to(dev)).sum()
        if ext is not None:
            loss = loss + (ext * x["cot_e"].to(dev)).sum()
            out["ext"] = ext.detach().cpu()
        loss.backward()
        taken = [name for name, a, c in zip(FORMS, before, forms_now()) if c != a]
        delta = sum(c - a for a, c in zip(before, forms_now()))
        assert delta == 1 and len(taken) == 1, f"{spec.name} {mode}: one backward, counted {delta} time(s) as {taken}"
        out["form"] = taken[0]
        if expect is not None:
            assert taken[0] == expect, f"{spec.name} {mode}: the backward took the {taken[0]} form, the case is about {expect}"
        out.update({"t_bwd": t_bwd.detach().cpu(), "t_fwd": t_fwd.detach().cpu()})
        out.update({name: leaf.grad.cpu() for name, leaf in leaves.items()})
        return out


def gate(spec, ours, refs, what):
    """Every quantity of one run against the fp64 truth: printed, recorded for the table of DESIGN.md §4, then asserted."""
    truth, ref32 = refs
    keys = [k for k in truth if k in ours]
    assert set(k for k in ours if k != "form") == set(keys), (sorted(ours), sorted(truth))
    figures = {k: (relerr(ours[k], truth[k]), relerr(ref32[k], truth[k])) for k in keys}
    print(f"[{spec.family}] {spec.name} {what} ({ours['form']}): " + " ".join(f"{k}={e:.1e}/{g:.1e}" for k, (e, g) in figures.items()), flush=True)
    worst = FIGURES.setdefault(spec.family, {})
    for k, (e, g) in figures.items():
        if e >= worst.get(k, (-1.0, 0.0))[0]:
            worst[k] = (e, g)
    for k in keys:
        assert bool(torch.isfinite(ours[k]).all()), f"{spec.name} {what}: {k} is not finite"
        if k in ("t_bwd", "t_fwd", "ext"):
            assert_close(ours[k], truth[k], POSE_TOL, what=f"{spec.name} {what}: {k}")
        else:
            assert_close_or_reference_gap(ours[k], truth[k], ref32[k], TOL, what=f"{spec.name} {what}: {k}")
    if spec.family == "dense":
        for k in ("g_depth", "g_logits"):
            e = maxerr(ours[k], truth[k])
            print(f"[{spec.family}] {spec.name} {what}: {k} max-abs {e:.1e}", flush=True)
            assert e <= 10 * TOL, f"{spec.name} {what}: {k}: max-abs {e:.3e}"
    if spec.window:
        for k in ("g_depth", "g_logits"):
            frames = spec.f if k == "g_depth" else spec.f - 1
            assert float(ours[k][:, :1].abs().max()) == 0 and float(ours[k][:, 1 + frames :].abs().max()) == 0, f"{spec.name} {what}: {k} written outside the window"


def gate_pair(spec, a, b, rel, abs_, what):
    """Two runs of ours on the same inputs, on every quantity both returned."""
    for k in a:
        if k != "form" and k in b:
            assert_close(a[k], b[k], rel, abs_=abs_, what=f"{spec.name} {what}: {k}")


def print_figures():
    for family in FAMILIES:
        for k, (e, g) in sorted(FIGURES.get(family, {}).items()):
            print(f"[worst] {family:9s} {k:10s} ours {e:.1e}  fp32 reference {g:.1e}", flush=True)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------


def case_constants(dev=None):
    """The lists above straddle these values: they must be the sources'."""
    from flowmap_amd import _ops

    src = (ROOT / "flowmap_amd" / "csrc" / "fm_procrustes.hip").read_text()
    math_h = (ROOT / "flowmap_amd" / "csrc" / "fm_math.h").read_text()
    header = (ROOT / "include" / "flowmap_hip.h").read_text()

    def one(pattern, text=src):
        found = re.findall(pattern, text)
        assert len(found) >= 1 and len(set(found)) == 1, (pattern, found)
        return int(found[0])

    assert one(r"if \(points <= (\d+)\) \{  // one block per pair") == ONE_BLOCK_POINTS
    assert one(r"numel\(\) == pairs \* points \* 8 && points <= (\d+);", (ROOT / "flowmap_amd" / "csrc" / "fm_torch.cpp").read_text()) == ONE_BLOCK_POINTS
    found = re.search(r"return points <= (\d+) \? (\d+) : (\d+);", src)
    assert (int(found.group(1)), int(found.group(2)), int(found.group(3))) == (ITERS_POINTS, 1, ITERS_LARGE)
    assert one(r"#define FM_FIT_BWD_MAX_POINTS (\d+)", header) == FIT_BWD_MAX_POINTS
    assert one(r"constexpr int kFitBwdThreads = (\d+);") == FIT_BWD_THREADS and one(r"constexpr int kFitBwdGather = (\d+);") == FIT_BWD_GATHER
    assert FIT_BWD_MAX_POINTS == 4 * FIT_BWD_THREADS  # SLOTS 1..4
    assert one(r"#define FM_DENSE_TILE_H (\d+)", math_h) == TILE_H and one(r"#define FM_DENSE_TILE_W (\d+)", math_h) == TILE_W
    assert one(r"constexpr int kXcds = (\d+);") == XCDS
    assert one(r"constexpr int kSortChunk = (\d+);") == SORT_CHUNK
    assert one(r"#define FM_DENSE_TAP_BATCH (\d+)") == TAP_BATCH
    assert one(r"constexpr int kRepeatGroup = (\d+);") == REPEAT_GROUP
    assert one(r"constexpr int kChainThreads = (\d+);") == CHAIN_THREADS
    assert one(r"const int chunk = \(steps \+ (\d+)\) / \d+;") == CHAIN_CHUNKS - 1  # pose_chain_by_wave0
    assert one(r"const int chunk = \(steps \+ (\d+)\) / \d+;", (ROOT / "flowmap_amd" / "csrc" / "fm_device.h").read_text()) == CHAIN_CHUNKS - 1
    # the 64-thread per-pair kernels and their grids
    assert one(r"const dim3 fgrid\(\(unsigned\)\(\(pairs \+ 63\) / (\d+)\)\);") == PAIR_BLOCK
    per_pair = re.findall(r"procrustes_(?:finish_solve|finish_solve_dense|moments_finish)_kernel(?:<\w+>\))?, fgrid, dim3\((\d+)\)", src)
    assert len(per_pair) == 5 and set(per_pair) == {str(PAIR_BLOCK)}, per_pair
    for kernel in ("pose_solve_kernel", "pose_solve_bwd_kernel", "pose_solve_bwd_kinv_kernel", "procrustes_dense_consts_kernel"):
        found = re.search(kernel + r", dim3\(\((\w+) \+ 63\) / (\d+)\), dim3\((\d+)\)", src)
        assert found and int(found.group(2)) == PAIR_BLOCK and int(found.group(3)) == PAIR_BLOCK, kernel
    for kernel in ("procrustes_moments_kernel", "procrustes_scatter_kernel", "procrustes_scatter_repeat_kernel", "procrustes_scatter_plan_kernel"):
        assert one(r"__launch_bounds__\((\d+)\) " + kernel + r"\(") == POINT_BLOCK, kernel
    assert one(r"__launch_bounds__\((\d+)\) procrustes_fit_pair_kernel\(") == PAIR_FIT_BLOCK
    assert _ops.FIT_BACKWARD_FORMS == tuple("fit_bwd_" + name for name in FORMS)


def case_sparse(dev, spec):
    """Every form a depth-sourced fit on a constant, duplicate-free index set qualifies for.  fm_procrustes_fit: the atomic scatter, then
    the plan in three launches (no records without the chained fit), twice.  fm_procrustes_fit_chain on a fresh flow tensor: the staged
    gather and the atomic scatter; then static tap records with the planned backward — one launch up to FM_FIT_BWD_MAX_POINTS points,
    three beyond — twice; the same without the extrinsics; and, where the one-launch form ran, the three-launch form on the same plan."""
    from flowmap_amd._lib import torch_ops

    assert spec.plans and spec.chains
    planned = "one_launch" if spec.points <= FIT_BWD_MAX_POINTS else "three_launch"
    plain, chained = reference(spec, False), reference(spec, True)
    run = Runner(dev, spec)
    atomic = run("apply", expect="atomic")
    gate(spec, atomic, plain, "fit, first call")
    second = run("apply", expect="three_launch")
    third = run("apply", expect="three_launch")
    gate(spec, third, plain, "fit, third call")
    gate_pair(spec, second, atomic, PLAN_REL, PLAN_ABS, "fit: planned vs atomic")
    gate_pair(spec, third, second, REPEAT_REL, REPEAT_ABS, "fit: repeat")
    assert run.workspace() is None

    run = Runner(dev, spec)
    first = run("chained", expect="atomic")
    gate(spec, first, chained, "chained, first call")
    second = run("chained", expect=planned)
    third = run("chained", expect=planned)
    gate(spec, third, chained, "chained, third call")
    gate_pair(spec, second, first, PLAN_REL, PLAN_ABS, "chained: planned vs atomic")
    gate_pair(spec, third, second, REPEAT_REL, REPEAT_ABS, "chained: repeat")
    noext = run("chained_noext", expect=planned)
    gate(spec, noext, plain, "chained without extrinsics")
    gate_pair(spec, noext, atomic, PLAN_REL, PLAN_ABS, "chained without extrinsics vs the plain fit's atomic scatter")
    if planned == "one_launch":
        torch_ops().set_one_launch_backward(False)
        try:
            three = run("chained_noext", expect="three_launch")
        finally:
            torch_ops().set_one_launch_backward(True)
        gate(spec, three, plain, "chained, three launches")
        gate_pair(spec, three, atomic, PLAN_REL, PLAN_ABS, "three launches vs atomic")
    if spec is LONG_SLICE:
        frame_first = run.plan()[4].cpu()
        middle = int(frame_first[2] - frame_first[1])
        print(f"[{spec.name}] plan pixels per frame {(frame_first[1:] - frame_first[:-1]).tolist()}", flush=True)
        assert middle > FIT_BWD_THREADS * FIT_BWD_GATHER, "the middle frame's plan slice fits one trip of the gather loop"


def case_atomic_only(dev, spec):
    """Index sets with duplicates never plan: fm_procrustes_fit three times and fm_procrustes_fit_chain with and without the extrinsics,
    all with the atomic scatter.  Past 4096 points the chained fit is the multi-block elected form; past 65 536 a thread takes 8 points."""
    assert spec.dup and spec.chains and spec.points > ONE_BLOCK_POINTS
    plain, chained = reference(spec, False), reference(spec, True)
    run = Runner(dev, spec)
    first = run("apply", expect="atomic")
    gate(spec, first, plain, "fit, first call")
    run("apply", expect="atomic")
    third = run("apply", expect="atomic")
    gate(spec, third, plain, "fit, third call")
    gate(spec, run("chained", expect="atomic"), chained, "elected fit")
    gate(spec, run("chained_noext", expect="atomic"), plain, "elected fit without extrinsics")


def expected_tile_lists(spec, flow):
    """{(pair, tile): sorted packed later pixels} from the flows, in fp64 on the CPU (fm_math.h: dense_taps; procrustes_dense_plan_kernel),
    with the input condition that no sample is within PLAN_MARGIN pixels of a coordinate that decides its tiles."""
    h, w = spec.hw
    xy, _ = orc.pixel_grid((h, w))
    tiles_x, tiles_y = -(-w // TILE_W), -(-h // TILE_H)
    rows, cols = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    packed = ((rows << 16) | cols).reshape(-1).numpy().astype(np.uint32)
    out = {}
    for pair, fl in enumerate(flow.reshape(-1, h, w, 2)):
        pos = xy.double() + fl.double()
        lists = {}
        tiles = []
        for axis, (size, tile) in enumerate(((w, TILE_W), (h, TILE_H))):
            raw = (pos[..., axis] * size - 0.5).reshape(-1)
            # floor(x) passing m changes the tiles of columns floor(x) and floor(x) + 1 only where m or m + 1 starts a tile
            deciding = [m for m in range(1, size) if m % tile in (0, tile - 1)]
            near = min((float((raw - m).abs().min()) for m in deciding), default=1.0)
            assert near >= PLAN_MARGIN * size, f"{spec.name}: a sample within {near:.1e} pixels of a coordinate that decides its tiles (a bad case)"
            lo = raw.clamp(0, size - 1).floor().long()
            hi = torch.where(lo + 1 < size, lo + 1, lo)
            tiles.append((lo // tile, hi // tile))
        (xa, xb), (ya, yb) = tiles
        seen = torch.stack([ya * tiles_x + xa, ya * tiles_x + xb, yb * tiles_x + xa, yb * tiles_x + xb], dim=1).numpy()
        for t in range(tiles_x * tiles_y):
            lists[t] = np.sort(packed[(seen == t).any(axis=1)])
        out.update({(pair, t): v for t, v in lists.items()})
    return out, tiles_x * tiles_y


def case_dense(dev, spec):
    """indices=None: the fused pass, the planned pair of kernels and the generic kernels (explicit arange) against the fp64 truth and
    against each other, as cases.case_dense_procrustes compares them; the static tap lists against lists built on the CPU."""
    assert spec.points is None and spec.source == "depth"
    refs = reference(spec)
    res = {}
    for name, arange, dense_plan, expect in (("fused", False, False, "dense_fused"), ("planned", False, True, "dense_planned"), ("generic", True, None, "atomic")):
        run = Runner(dev, spec, arange=arange)
        res[name] = run("apply", expect=expect, dense_plan=dense_plan)
        assert ("_fm_dense_plan" in run.flow.__dict__) == (name == "planned")
        gate(spec, res[name], refs, name)
        if name == "planned":
            first, entries = (t.cpu() for t in run.flow._fm_dense_plan[1])
    for mode in ("fused", "planned"):
        for k in ("t_bwd", "t_fwd", "g_depth", "g_logits", "g_k"):
            assert_close(res[mode][k], res["generic"][k], TOL, abs_=1e-7, what=f"{spec.name} {mode}: {k} vs generic kernels")
    for k in ("g_depth", "g_logits"):
        assert_close(res["fused"][k], res["planned"][k], 1e-6, what=f"{spec.name}: {k}: fused pass vs planned kernels")
    # the static tap lists
    h, w = spec.hw
    want, tiles = expected_tile_lists(spec, make_inputs(spec)["flow"])
    entries = entries.numpy().view(np.uint32)
    first = first.tolist()
    assert len(first) == spec.pairs * tiles + 1 and first[0] == 0
    lengths = [hi - lo for lo, hi in zip(first[:-1], first[1:])]
    print(f"[{spec.name}] {tiles} tiles x {spec.pairs} pairs = {tiles * spec.pairs} blocks; tile lists {min(lengths)} .. {max(lengths)} entries", flush=True)
    for slot, (lo, hi) in enumerate(zip(first[:-1], first[1:])):
        seg = entries[lo:hi]
        for c in range(0, len(seg), SORT_CHUNK):
            chunk = seg[c : c + SORT_CHUNK].astype(np.int64)
            assert (chunk[1:] > chunk[:-1]).all(), f"{spec.name}: tile list {slot}: a chunk is not in ascending pixel order"
        if len(seg) <= SORT_CHUNK:
            assert (seg[1:] > seg[:-1]).all()
        assert np.array_equal(np.sort(seg), want[(slot // tiles, slot % tiles)]), f"{spec.name}: tile list {slot} is not the CPU's"
    if spec is CONTRACT:
        assert sorted(lengths) == sorted([0, 0, 0, h * w] * spec.pairs), lengths
        assert h * w > SORT_CHUNK and h * w > 5 * TAP_BATCH * 256
    if spec in XCD_CASES:
        assert tiles * spec.pairs == {XCD_CASES[0]: 1, XCD_CASES[1]: 7, XCD_CASES[2]: 8, XCD_CASES[3]: 9}[spec]


def case_surfaces(dev, spec):
    """Surface-sourced fits (lazy=False): fm_procrustes_fit and, with an index set, fm_procrustes_fit_chain; the backward is the atomic
    scatter into dL/dsurfaces whatever the call count."""
    assert spec.source == "surfaces"
    run = Runner(dev, spec)
    gate(spec, run("apply", expect="atomic"), reference(spec, False), "fit")
    if spec.chains:
        gate(spec, run("chained", expect="atomic"), reference(spec, True), "chained")
        gate(spec, run("chained_noext", expect="atomic"), reference(spec, False), "chained without extrinsics")
        gate(spec, run("apply", expect="atomic"), reference(spec, False), "fit, fourth call")


def case_repeat(dev, spec):
    """batch_repeat > 1 (the softmin sweep's candidates on shared images): poses per candidate; dL/ddepth and dL/dlogits summed over the
    candidates, dL/dK per candidate — procrustes_scatter_repeat_kernel."""
    assert spec.repeat > 1
    run = Runner(dev, spec)
    refs = reference(spec)
    first = run("apply", expect="repeat")
    gate(spec, first, refs, "fit")
    for r in range(spec.b * spec.repeat):  # per candidate: one whose gradient is wrong cannot hide under the norm of the stack
        assert_close_or_reference_gap(first["g_k"][r], refs[0]["g_k"][r], refs[1]["g_k"][r], TOL, what=f"{spec.name}: g_k[candidate {r}]")
        assert_close(first["t_bwd"][r], refs[0]["t_bwd"][r], POSE_TOL, what=f"{spec.name}: t_bwd[candidate {r}]")
    gate(spec, run("apply", expect="repeat"), refs, "fit, second call")


def case_reuse(dev, spec):
    """Three back-to-back chained calls on changing depth: each against its own truth, the workspace zero after each (Runner)."""
    run = Runner(dev, spec)
    x = make_inputs(spec)
    g = torch.Generator().manual_seed(77 + spec.seed)
    for step in range(3):
        depth = 1.0 + 0.3 * torch.rand(x["depth"].shape, generator=g)
        gate(spec, run("chained", depth=depth), reference(spec, True, dict(x, depth=depth)), f"chained call {step}")


def case_stats(dev, spec):
    """fm_procrustes_stats (moments + procrustes_moments_finish_kernel, no solve) on a garbage-filled buffer: Σw, Σw·p, Σw·q and M of
    every pair against the fp64 sums, at the tolerance of point_function_cases.case_rigid_stats_abi."""
    from flowmap_amd import _ops
    from point_function_cases import STAT_STRIDE, abi, acc_buffer, acc_values, hold, stats_truth, stream

    x = make_inputs(spec)
    f, (h, w) = spec.f, spec.hw
    n, pairs = h * w, spec.pairs
    xy, _ = orc.pixel_grid((h, w), dtype=torch.float64)
    surfaces = orc.lift(xy, x["depth"].double(), x["k"].double()[:, :, None, None])
    p = surfaces[:, 1:].reshape(pairs, n, 3)[:, x["idx"]]
    q = orc.bilinear_border(surfaces[:, :-1], (xy + x["flow"].double()).reshape(1, f - 1, n, 2)[:, :, x["idx"]])[0]
    wts = (SENS * x["logits"].double()).sigmoid().reshape(pairs, n)[:, x["idx"]]
    want = stats_truth(p, q, wts)
    depth, k, flow, logits, idx = (x[name].to(dev) for name in ("depth", "k", "flow", "logits", "idx"))
    kinv = _ops.intrinsics_inverse(k)
    stats = acc_buffer(pairs * STAT_STRIDE, dev)
    abi("fm_procrustes_stats", depth.data_ptr(), kinv.data_ptr(), None, flow.data_ptr(), logits.data_ptr(), SENS, idx.data_ptr(), spec.points, 1, 1, f, h, w,
        stats.ptr, stream(dev))
    stats.check_guards(spec.name)
    got = acc_values(stats, (pairs, STAT_STRIDE))
    for pair in range(pairs):
        hold(f"{spec.name} pair {pair} sums", got[pair, :7], want[pair, :7], STATS_FLOOR)
        hold(f"{spec.name} pair {pair} M", got[pair, 7:], want[pair, 7:], STATS_FLOOR)
