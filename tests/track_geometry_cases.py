"""The fused tracking loss ALONE (csrc/fm_track.hip: track_targets, track_pairs, track_reduce, both finalizers, the atomic scatter, the
scatter plan, the planned gather, tap_grad and the compact tap image) at every edge of its launch geometry.  Shared by the CPU (host
double) and GPU modules: the host double loops where the kernels launch, so only the GPU module says anything about point groups, register
tiles, the prefetch, the XCD dealing and the 64- and 256-thread blocks; the CPU module proves the cases, their reference and the input
conditions.

Truth is a plain fp64 evaluation of ``weight * orc.tracking_loss`` on surfaces lifted from the leaves depth (1,F,H,W), K (1,F,3,3) and
E (1,F,4,4) — independent random leaves, not a Procrustes output — with autograd's gradients; ``ref32`` is the same function in torch fp32
(the reference's own arithmetic).  The gate is conftest.assert_close_or_reference_gap: 1e-4 of the truth, or twice the fp32 evaluation's
own measured gap where that is larger.  Every figure is printed before it is asserted.

Input conditions (``Case.altered``): a visibility test (uv in [0,1)^2) or a Huber kink (|d| = delta) within fp32 rounding of its threshold
flips between fp32 and fp64, which is no kernel error.  The generator evaluates the fp64 reference and clears the source-frame visibility
bit of every (source, point) that has an otherwise visible target projected closer than EDGE_MARGIN to 0 or 1, or a residual norm within
KINK_MARGIN·delta of delta.  The track is altered, nothing is left out of a comparison, and at most ALTERED_CAP of a case's points may be
altered that way (asserted)."""

from __future__ import annotations

import contextlib
import dataclasses
import json
import math
import os
import re
from pathlib import Path

import pytest
import torch

from conftest import assert_close, assert_close_or_reference_gap, maxerr, relerr
from oracle import flowmap_oracle as orc

ROOT = Path(__file__).resolve().parent.parent

# ---- the constants of csrc/fm_track.hip the lists below straddle (case_constants checks them against the sources) -----------------------
TILE = 6  # FM_TRACK_TILE: source frames a lane of track_pairs holds in registers, processed in packed pairs (.x / .y)
PG = 2  # FM_TRACK_PG: points per lane
WAVE = 64  # one wave per block of track_pairs: a work item covers WAVE * PG = 128 points
AHEAD = 2  # FM_TRACK_AHEAD: target frames whose (visibility, position) loads are in flight
XCDS = 8  # kXcds: launch indices are dealt to eight shares of the (tile, point group) list; the grid is padded to a multiple
REDUCE_BLOCK = 256  # track_reduce: one block per frame strides over ntiles x pgroups entries
FRAME_BLOCK = 64  # track_targets, track_finalize_bwd, inv4 (and the single wave of track_finalize_fwd): 64 frames per block

EDGE_MARGIN = 1e-4
KINK_MARGIN = 1e-3
ALTERED_CAP = 0.01
DELTA = 0.01
TOL = 1e-4  # the project's gate (conftest.assert_close_or_reference_gap)
PATH_REL = 2e-6  # agreement between two paths on the same inputs, of the largest magnitude (cases.case_tap_exchange)
SCATTER_REL, SCATTER_ABS = 2e-6, 1e-6  # two runs of the atomic scatter (cases.case_track_scatter_plan)


# ---- the lists ------------------------------------------------------------------------------------------------------------------------------


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    frames: int
    hw: tuple
    segments: tuple  # ((start_frame, f, P), ...)
    kind: str = "huber"
    weight: float = 100.0
    upstream: float = 1.0
    seed: int = 0
    spread: float = 0.01
    edit: str = ""  # a function of EDITS applied to the generated inputs before the margin rule
    visible: bool = True  # False: the case is about zero visibility (the count may be 0)

    @property
    def diagonal_only(self):
        """Every visible pair has source = target: inv(E)·E = I and K·K^-1 = I, so the loss depends on neither E nor K in exact arithmetic
        (the residual is the depth-weighted shift of the bilinear sample alone) — dL/dE and dL/dK are rounding residue in ANY precision and are
        printed, not compared; loss, count and dL/ddepth are."""
        return self.edit == "one_pair" or all(f == 1 for _, f, _ in self.segments)

    @property
    def geometry(self):  # what the tracks and the leaves depend on (kind, weight and upstream share them)
        return (self.frames, self.hw, self.segments, self.seed, self.spread, self.edit)


# Points per segment, one segment of f = 7 (a full tile and one frame of the next) in a video of 8 frames (frame 0 is covered by nothing):
#   1, 2            one lane, one point; the second point of lane 0 does not exist
#   63, 64, 65      the wave: the second point of a lane (p = lane + 64) goes wholly inactive at 64 and starts to exist at 65
#   127, 128, 129   WAVE * PG: one point group exactly, and the first point of a second one (127 idle lanes clamped to p_count - 1)
#   255, 256, 257   two groups, and a third
POINTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)
P_CASES = tuple(Spec(f"P{p}", 8, (8, 12), ((1, 7, p),), seed=p) for p in POINTS)

# Frames per segment at P = 65 (both points of lane 0, one of every other lane):
#   1, 2, 3     AHEAD = 2: the prologue's prefetch covers the whole segment (1, 2) or all but one target (3)
#   5           an odd tile tail: the .y half of the third packed pair is absent
#   6, 7        TILE: exactly one tile, and one frame into the next (.x alone)
#   11, 12, 13  two tiles less one, two tiles, one frame into the third
# The segment starts at frame 1 of 14: f = 13 ends on the video's last frame.
FRAMES_PER_SEGMENT = (1, 2, 3, 5, 6, 7, 11, 12, 13)
F_CASES = tuple(Spec(f"f{f}", 14, (12, 16), ((1, f, 65),), seed=100 + f) for f in FRAMES_PER_SEGMENT)

# Segments of different P {129, 3, 64, 65} (pmax = 129: two point groups, the second wholly idle for P = 3, 64, 65 and 127 lanes idle for
# P = 129) and different f {13, 1, 6, 7} in one launch; overlapping windows, start_frame > 0, a segment ending on the last frame (14 + 6 = 20);
# frame 0 is covered by nothing.  8 tiles x 2 groups = 16 work items.
MIXED_SEGMENTS = ((2, 13, 129), (1, 1, 3), (9, 6, 64), (14, 6, 129), (5, 7, 65))
MIXED = Spec("mixed", 20, (12, 16), MIXED_SEGMENTS, seed=7)
MIXED_WIDE = Spec("mixed-16x20", 20, (16, 20), MIXED_SEGMENTS, seed=8)
ODD_WIDTH = Spec("mixed-10x13", 20, (10, 13), MIXED_SEGMENTS, seed=9)  # width % 4 != 0: the tap plan must quietly not apply


def _short_segments(count, frames, p=5):
    return tuple((i % (frames - 4), 2 + i % 3, p) for i in range(count))


# Work items (ntiles x pgroups): 1, 7, 8, 9, 17 around XCDS (the padded grid and the dealing: 7 -> one item per share and an idle block, 9 ->
# two per share with 7 idle blocks), and 260 = 65 segments x 2 tiles (f = 12) x 2 groups (P = 129) for the 256-thread stride of track_reduce.
WORK_ITEMS = (1, 7, 8, 9, 17)
ITEM_CASES = tuple(Spec(f"items{n}", 10, (8, 12), _short_segments(n, 10), seed=200 + n) for n in WORK_ITEMS) + (
    Spec("items260", 14, (8, 12), tuple((i % 3, 12, 129) for i in range(65)), seed=260),)

# Frames of the video around FRAME_BLOCK (track_targets, finalize_bwd, inv4: a second block from 65 on; finalize_fwd: a second trip of its one
# wave) and 130 = two blocks and two frames; segments of 3 frames every fourth frame (one frame in four is covered by nothing), one ending
# on the last frame.
VIDEO_FRAMES = (63, 64, 65, 130)
VIDEO_CASES = tuple(Spec(f"F{n}", n, (8, 12), tuple((s, 3, 5) for s in range(0, n - 6, 4)) + ((n - 3, 3, 5),), seed=300 + n) for n in VIDEO_FRAMES)

KIND_CASES = tuple(dataclasses.replace(s, name=f"{s.name}-{kind}", kind=kind) for kind in ("l1", "l2") for s in (MIXED, P_CASES[7], F_CASES[5]))
UPSTREAM_CASES = (dataclasses.replace(MIXED, name="mixed-upstream2.5", upstream=2.5), dataclasses.replace(MIXED, name="mixed-weight3.7", weight=3.7),
                  dataclasses.replace(MIXED, name="mixed-weight1", weight=1.0))

TAP_EDGES = Spec("tap-edges", 6, (8, 12), ((0, 6, 40), (2, 4, 40), (1, 3, 10)), seed=11, edit="tap_edges")
TAP_EDGES_L2 = dataclasses.replace(TAP_EDGES, name="tap-edges-l2", kind="l2")
OUTSIDE = Spec("source-outside", 8, (8, 12), ((1, 7, 65),), seed=12, edit="outside")
NOTHING = Spec("nothing-visible", 8, (8, 12), ((1, 7, 65), (0, 3, 3)), seed=13, edit="nothing", visible=False)
ONE_PAIR = Spec("one-pair", 8, (8, 12), ((1, 7, 65), (0, 3, 3)), seed=14, edit="one_pair")

GEOMETRY_CASES = P_CASES + F_CASES + (MIXED, MIXED_WIDE, ODD_WIDTH) + ITEM_CASES + VIDEO_CASES + KIND_CASES + UPSTREAM_CASES + (
    TAP_EDGES, TAP_EDGES_L2, OUTSIDE, NOTHING, ONE_PAIR)
# every path is run on the mixed list and on the P and f boundary cases
PATH_CASES = (MIXED, P_CASES[4], P_CASES[6], P_CASES[7], F_CASES[3], F_CASES[4], F_CASES[5], F_CASES[8], TAP_EDGES)
TAP_CASES = tuple(s for s in PATH_CASES if s.hw[1] % 4 == 0)
SPECS = {s.name: s for s in GEOMETRY_CASES}
assert len(SPECS) == len(GEOMETRY_CASES)


def spec_id(spec):
    return spec.name


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------


def _random_rigid(n, gen):
    """cases._random_rigid, enlarged (angle 0.03 -> 0.04 rad, shift 0.05 -> 0.08): the projected targets move by several times the Huber
    delta, so residuals are well away from zero and most of them beyond the kink."""
    from cases import _random_rigid as small

    return small(n, gen, angle=0.04, shift=0.08)


def make_leaves(spec):
    """depth (1,F,H,W), K (1,F,3,3) with its own fx, fy, skew and principal point per frame (third row 0,0,1), E (1,F,4,4) rigid: fp32."""
    f, (h, w) = spec.frames, spec.hw
    gen = torch.Generator().manual_seed(1000 + spec.seed)
    depth = 1.0 + 0.5 * torch.rand((1, f, h, w), generator=gen, dtype=torch.float64)
    k = orc.focal_to_k(torch.tensor(0.85, dtype=torch.float64), (h, w)).repeat(1, f, 1, 1).clone()
    k[0, :, 0, 0] *= 1.0 + 0.05 * torch.randn((f,), generator=gen, dtype=torch.float64)
    k[0, :, 1, 1] *= 1.0 + 0.05 * torch.randn((f,), generator=gen, dtype=torch.float64)
    k[0, :, 0, 1] = 0.02 * torch.randn((f,), generator=gen, dtype=torch.float64)
    k[0, :, :2, 2] += 0.03 * torch.randn((f, 2), generator=gen, dtype=torch.float64)
    e = _random_rigid(f, gen)[None]
    return depth.float(), k.float(), e.float()


def make_tracks(spec):
    """One OTracks per (start_frame, f, P): i.i.d. drift around a grid as orc.synth_tracks(scene=None) lays it out, but with its own P per
    segment (synth_tracks gives every segment the same grid^2)."""
    gen = torch.Generator().manual_seed(2000 + spec.seed)
    out = []
    for start, f, p in spec.segments:
        assert start >= 0 and f >= 1 and p >= 1 and start + f <= spec.frames, (spec.name, start, f, p)
        side = math.ceil(math.sqrt(p))
        lin = 0.06 + 0.88 * (torch.arange(side, dtype=torch.float32) + 0.5) / side
        q = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), dim=-1).reshape(-1, 2)[:p]
        drift = spec.spread * torch.randn((f, p, 2), generator=gen).cumsum(0)
        xy = q[None] + drift - drift[f // 2]
        inside = (xy >= 0).all(-1) & (xy < 1).all(-1)
        vis = inside & (torch.rand(inside.shape, generator=gen) < 0.85)
        out.append(orc.OTracks(xy[None].contiguous(), vis[None].contiguous(), start))
    return out


def _pixel(col, row, hw):
    return torch.tensor([(col + 0.5) / hw[1], (row + 0.5) / hw[0]])


def _edit_tap_edges(spec, leaves, tracks):
    """Points on pixel centres (weights 1,0,0,0), in the four corners and on each border (clipped taps, slot -1: one or both taps of an image
    row missing), on the last pixel of the last frame (the padded tail of the tap image, read with an 8-byte load), several points of
    different segments at identical positions (shared taps), all points of a segment at one position."""
    h, w = spec.hw
    a, b, c = tracks
    for fr in range(a.xy.shape[1]):
        a.xy[0, fr, 0], a.xy[0, fr, 1] = _pixel(3 + fr % 2, 2, spec.hw), _pixel(0, 0, spec.hw)  # pixel centres; the first pixel of a frame
        a.xy[0, fr, 2] = torch.tensor([0.2 / w, 0.2 / h])  # the four corners: beyond the outer pixel centres, one tap left
        a.xy[0, fr, 3] = torch.tensor([1 - 0.2 / w, 0.2 / h])
        a.xy[0, fr, 4] = torch.tensor([0.2 / w, 1 - 0.2 / h])
        a.xy[0, fr, 5] = torch.tensor([1 - 0.2 / w, 1 - 0.2 / h])
        a.xy[0, fr, 6] = torch.tensor([0.52, 0.1 / h])  # the four borders: one image row / one image column of taps
        a.xy[0, fr, 7] = torch.tensor([0.52, 1 - 0.1 / h])
        a.xy[0, fr, 8] = torch.tensor([0.1 / w, 0.47])
        a.xy[0, fr, 9] = torch.tensor([1 - 0.1 / w, 0.47])
        a.visibility[0, fr, :10] = True
    a.xy[0, -1, 10] = _pixel(w - 1, h - 1, spec.hw)  # segment a ends on the last frame: its last pixel is the last tap of the image
    a.visibility[0, -1, 10] = True
    for fr in range(b.xy.shape[1]):  # segment b starts at frame 2: its frame fr is a's frame fr + 2
        b.xy[0, fr, :4] = a.xy[0, fr + 2, 11:15]  # shared taps between segments (and with themselves: 0/1 and 2/3 coincide)
        b.xy[0, fr, 1], b.xy[0, fr, 3] = b.xy[0, fr, 0], b.xy[0, fr, 2]
        b.xy[0, fr, 4] = a.xy[0, fr + 2, 0]  # ... and on a pixel centre another point sits on
        b.visibility[0, fr, :5] = True
        a.visibility[0, fr + 2, 11:15] = True
    for fr in range(c.xy.shape[1]):
        c.xy[0, fr, :] = c.xy[0, fr, 0]  # all P points of a segment at one position
        c.visibility[0, fr, :] = True


def _edit_outside(spec, leaves, tracks):
    """Sources outside [0,1)^2 with their visibility bit set (x < 0, x = 1 exactly, y >= 1, y < 0): they are no sources and no targets'
    positions are read for them as sources, but they still serve as target positions of visible sources."""
    t = tracks[0]
    for fr in range(t.xy.shape[1]):
        t.xy[0, fr, 0 + fr % 3, 0] = -0.02
        t.xy[0, fr, 5 + fr % 3, 0] = 1.0
        t.xy[0, fr, 10 + fr % 3, 1] = 1.3
        t.xy[0, fr, 64, 1] = -1e-6
        t.visibility[0, fr, :16] = True
        t.visibility[0, fr, 64] = True


def _edit_nothing(spec, leaves, tracks):
    """Nothing visible: one segment by its visibility bits, the other by sources outside the frame."""
    tracks[0].visibility[:] = False
    tracks[1].xy[..., 0] += 1.0
    tracks[1].visibility[:] = True


def _edit_one_pair(spec, leaves, tracks):
    """Exactly one visible pair: one point visible in one frame (its own source and target).  The residual of such a pair is the shift
    between the depth-weighted and the plain bilinear mean of its tap positions and nothing else; with the i.i.d. depths it would be a
    tenth of delta, the difference of two coordinates that agree to three digits.  The point sits between four pixel centres whose depths
    are 1, 2, 1, 2: a sixth of a pixel, beyond the kink."""
    for t in tracks:
        t.visibility[:] = False
    seg = tracks[0]
    seg.visibility[0, 3, 64] = True
    seg.xy[0, 3, 64] = torch.tensor([5.0 / spec.hw[1], 4.0 / spec.hw[0]])  # taps: columns 4, 5 of rows 3, 4
    leaves[0][0, seg.start_frame + 3, 3:5, 4] = 1.0
    leaves[0][0, seg.start_frame + 3, 3:5, 5] = 2.0


EDITS = {"tap_edges": _edit_tap_edges, "outside": _edit_outside, "nothing": _edit_nothing, "one_pair": _edit_one_pair}


def _surfaces(depth, k, hw):
    xy, _ = orc.pixel_grid(hw, dtype=depth.dtype)
    return orc.lift(xy, depth, k[:, :, None, None])


def apply_margins(spec, leaves, tracks):
    """The rule of the module docstring, on the fp64 reference -> (altered points, points)."""
    depth, k, e = (x.double() for x in leaves)
    surfaces = _surfaces(depth, k, spec.hw)
    altered = total = 0
    for seg in tracks:
        s, f = seg.start_frame, seg.xy.shape[1]
        seg64 = orc.OTracks(seg.xy.double(), seg.visibility, s)
        tgt, vis = orc.track_positions(surfaces[:, s : s + f], e[:, s : s + f], k[:, s : s + f], seg64)  # (1, fs, ft, P, 2), (1, fs, ft, P)
        src = seg64.xy[:, :, None]
        candidate = seg.visibility[:, :, None] & seg.visibility[:, None, :] & (src >= 0).all(-1) & (src < 1).all(-1)
        within = ((tgt > -EDGE_MARGIN) & (tgt < 1 + EDGE_MARGIN)).all(-1)
        near = ((tgt.abs() < EDGE_MARGIN) | ((tgt - 1).abs() < EDGE_MARGIN)).any(-1) & within
        norm = (orc.aspect_scale(tgt, spec.hw) - orc.aspect_scale(seg64.xy[:, None], spec.hw)).norm(dim=-1)
        kink = vis & ((norm - DELTA).abs() < KINK_MARGIN * DELTA)
        alter = ((candidate & near) | kink).any(dim=2)  # (1, fs, P): the source-frame visibility bit
        seg.visibility &= ~alter
        altered += int(alter.sum())
        total += alter.numel()
    return altered, total


@dataclasses.dataclass
class Case:
    spec: Spec
    leaves: tuple  # depth, K, E (fp32, CPU)
    tracks: list  # OTracks (fp32 positions, CPU)
    altered: int
    points: int
    count: int = 0  # the fp64 visible count
    truth: dict = None  # loss, g_depth, g_k, g_e in fp64 (the gradients of upstream * loss)
    ref32: dict = None  # the same function in torch fp32
    touched: torch.Tensor = None  # orc.tracks_touched

    @property
    def share(self):
        return self.altered / max(self.points, 1)


_INPUTS: dict = {}
_CASES: dict = {}


def _evaluate(spec, leaves, tracks, dtype):
    depth, k, e = (x.to(dtype).clone().requires_grad_(True) for x in leaves)
    tr = [orc.OTracks(t.xy.to(dtype), t.visibility, t.start_frame) for t in tracks]
    loss = spec.weight * orc.tracking_loss(_surfaces(depth, k, spec.hw), e, k, tr, spec.hw, spec.kind, DELTA)
    (spec.upstream * loss).backward()
    return {"loss": loss.detach(), "g_depth": depth.grad, "g_k": k.grad, "g_e": e.grad}


def make_case(spec) -> Case:
    """Inputs (shared by the specs of one geometry), the fp64 truth and its fp32 twin: computed once, shared, never written to."""
    if spec.name in _CASES:
        return _CASES[spec.name]
    if spec.geometry not in _INPUTS:
        leaves, tracks = make_leaves(spec), make_tracks(spec)
        if spec.edit:
            EDITS[spec.edit](spec, leaves, tracks)
        altered, points = apply_margins(spec, leaves, tracks)
        _INPUTS[spec.geometry] = (leaves, tracks, altered, points)
    leaves, tracks, altered, points = _INPUTS[spec.geometry]
    case = Case(spec, leaves, tracks, altered, points)
    depth, k, e = (x.double() for x in leaves)
    with torch.no_grad():
        surfaces = _surfaces(depth, k, spec.hw)
        for seg in tracks:
            s, f = seg.start_frame, seg.xy.shape[1]
            case.count += int(orc.track_positions(surfaces[:, s : s + f], e[:, s : s + f], k[:, s : s + f], orc.OTracks(seg.xy.double(), seg.visibility, s))[1].sum())
    case.truth, case.ref32 = _evaluate(spec, leaves, tracks, torch.float64), _evaluate(spec, leaves, tracks, torch.float32)
    case.touched = orc.tracks_touched(spec.hw, spec.frames, tracks)
    _CASES[spec.name] = case
    return case


def check_conditions(case):
    """The input conditions and the vacuity conditions of one case (CPU module; repeated by every comparison)."""
    spec = case.spec
    print(f"[{spec.name}] altered {case.altered} of {case.points} points ({100 * case.share:.3f} %), fp64 count {case.count}", flush=True)
    assert case.share <= ALTERED_CAP, f"{spec.name}: {case.altered} of {case.points} points altered by the margin rule (> {ALTERED_CAP:.0%})"
    for x in case.leaves + tuple(t.xy for t in case.tracks):
        assert bool(torch.isfinite(x).all())
    k = case.leaves[1]
    assert torch.equal(k[0, :, 2], torch.tensor([0.0, 0.0, 1.0]).expand(spec.frames, 3))
    if not spec.visible:
        assert case.count == 0
        return
    assert case.count > 0, f"{spec.name}: nothing visible"
    for name in ("g_depth",) if spec.diagonal_only else ("g_depth", "g_k", "g_e"):
        assert float(case.truth[name].norm()) > 0, f"{spec.name}: the reference's {name} is zero"
    if not spec.diagonal_only:  # the pose and intrinsics gradients are no rounding residue: of the size of their terms
        for name in ("g_k", "g_e"):
            assert float(case.truth[name].norm()) > 1e-6 * float(case.truth["g_depth"].norm()), f"{spec.name}: the reference's {name} cancels to nothing"
    assert float(case.truth["loss"]) > 0


# ---- ours -----------------------------------------------------------------------------------------------------------------------------------


class _Recorder:
    """torch.ops.flowmap_amd with the outputs of every track_loss call kept (scale and totals are not returned by the Python facade)."""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def track_loss(self, *args):
        out = self._ops.track_loss(*args)
        self.calls.append(out)
        return out


@contextlib.contextmanager
def recorded():
    from flowmap_amd import _ops

    real = _ops.torch_ops
    rec = _Recorder(real())
    _ops.torch_ops = lambda: rec
    try:
        yield rec
    finally:
        _ops.torch_ops = real


def device_tracks(case, dev):
    from helpers import to_tracks

    return to_tracks(case.tracks, dev)


def covered_frames(spec):
    covered = torch.zeros((spec.frames,), dtype=torch.bool)
    for start, f, _ in spec.segments:
        covered[start : start + f] = True
    return covered


def run_ours(dev, case, grad=True, defer=True, own=None, reducer=None, taps=None):
    """_ops.TrackLossFused.apply on fresh leaves (the path LossTracking._fused takes) and, with ``grad``, backward of upstream * loss ->
    dict on the CPU.  ``own = (a, b)``: the tracks packed for the source frames [a, b), depth the window of those frames, frame0 = a.
    ``taps``: None, "image" (the compact tap image holds every tap depth, sampled branch-free) or "around" (every third tap is flagged
    "read the depth image" and its image value is poisoned: the general branch of track_sample_many)."""
    from flowmap_amd import _ops
    from flowmap_amd.config import override

    spec = case.spec
    depth, k, e = (x.clone().to(dev) for x in case.leaves)
    frame0 = 0
    if own is not None:
        frame0 = own[0]
        depth = depth[:, own[0] : own[1]].contiguous()
    leaves = [x.requires_grad_(True) for x in (depth, k, e)]
    packed = _ops.PackedTracks(device_tracks(case, dev), torch.device(dev), own)
    options = {}
    if taps is not None:
        plan = packed.tap_plan(spec.frames, *spec.hw)
        assert plan is not None, f"{spec.name}: no tap plan"
        image = depth.detach().reshape(-1)[plan.pixels].clone()
        if taps == "around":
            kept = plan.pixels[::3].clone()
            image[::3] = 1.0e3  # what an in-pass update leaves there is the PRE-update value: it must not be read
            plan.image_slots = plan.slots_reading_around(kept)
            assert int(((plan.image_slots >= 0) & ((plan.image_slots & 0x20000000) != 0)).sum()) > 0
        plan.image.copy_(image)
        plan.tag(depth)
        options = dict(tap_exchange=True, tap_image=True, tap_exchange_min_bytes=0)
    sampled = _ops.counters["track_tap_samples"]
    with override(**options), recorded() as rec, (contextlib.nullcontext() if grad else torch.no_grad()):
        loss = _ops.TrackLossFused.apply(depth, k, e, packed, spec.weight, _ops.MAPPING_KINDS[spec.kind], DELTA, defer, frame0, reducer)
    if taps is not None:
        assert _ops.counters["track_tap_samples"] == sampled + 1, f"{spec.name}: the compact tap image was not sampled"
    (_, scale, totals), = rec.calls
    out = {"loss": loss.detach().cpu().clone(), "scale": scale.detach().cpu().clone(), "totals": totals.detach().cpu().clone()}
    if grad:
        (spec.upstream * loss).backward()
        for name, leaf in zip(("g_depth", "g_k", "g_e"), leaves):
            out[name] = torch.zeros_like(leaf).cpu() if leaf.grad is None else leaf.grad.detach().cpu().clone()
    return out


RECORD = {}  # quantity -> (worst ours / truth, the fp32 reference / truth of that case, case)


def _note(quantity, err, gap, name):
    if quantity not in RECORD or err > RECORD[quantity][0]:
        RECORD[quantity] = (err, gap, name)
    out = os.environ.get("FLOWMAP_PARITY_RECORD")
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps({"what": f"track geometry {name}", "quantity": quantity, "rel": err, "rel_fp32": gap}) + "\n")


def gate(case, ours, what=""):
    """Loss, count, dL/ddepth, dL/dK rows 0 and 1, the twelve entries of dL/dE's top three rows against the fp64 truth."""
    spec, truth, ref32 = case.spec, case.truth, case.ref32
    name = f"{spec.name}{' ' + what if what else ''}"
    assert int(ours["scale"][1]) == case.count, f"{name}: visible count {int(ours['scale'][1])}, the fp64 reference counts {case.count}"
    off = ~case.touched[None]
    assert float(ours["g_depth"][off].abs().max()) == 0.0 if bool(off.any()) else True, f"{name}: dL/ddepth is not zero off the track taps"
    idle = ~covered_frames(spec)
    if bool(idle.any()):
        assert float(ours["g_e"][0, idle].abs().max()) == 0.0 and float(ours["g_k"][0, idle].abs().max()) == 0.0, f"{name}: a frame no segment covers has a gradient"
    if not spec.visible:
        for key in ("loss", "g_depth", "g_k", "g_e"):
            assert float(ours[key].abs().max()) == 0.0, f"{name}: {key} must be exactly 0 when nothing is visible"
        return
    assert case.count > 0
    parts = (("loss", ours["loss"], truth["loss"], ref32["loss"]), ("dL/ddepth", ours["g_depth"], truth["g_depth"], ref32["g_depth"]),
             ("dL/dK", ours["g_k"][0, :, :2], truth["g_k"][0, :, :2], ref32["g_k"][0, :, :2]),
             ("dL/dE", ours["g_e"][0, :, :3], truth["g_e"][0, :, :3], ref32["g_e"][0, :, :3]))
    for quantity, a, t, r in parts:
        assert bool(torch.isfinite(a).all()), f"{name}: {quantity} is not finite"
    if spec.diagonal_only:
        for quantity, a, t, r in parts[2:]:
            print(f"[{name}] {quantity} (zero in exact arithmetic, not compared): |ours| {float(a.double().norm()):.3e}  |fp32 reference| {float(r.double().norm()):.3e}  "
                  f"|fp64| {float(t.norm()):.3e}", flush=True)
        parts = parts[:2]
    for quantity, a, t, r in parts:
        assert float(t.norm()) > 0 and float(a.double().norm()) > 0, f"{name}: {quantity} is zero"
        err, gap = relerr(a, t), relerr(r, t)
        print(f"[{name}] {quantity}: ours/fp64 {err:.3e}   fp32 reference/fp64 {gap:.3e}   (max-abs of max|ref| {maxerr(a, t):.3e} / {maxerr(r, t):.3e})", flush=True)
        _note(quantity, err, gap, name)
    for quantity, a, t, r in parts:
        assert_close_or_reference_gap(a, t, r, TOL, what=f"{name}: {quantity}")
    # element-wise: the same gate on the largest single deviation, so that a few wrong pixels cannot hide under the norm
    a, t, r = parts[1][1:]
    assert maxerr(a, t) <= max(TOL, 2.0 * maxerr(r, t)), f"{name}: dL/ddepth max-abs err {maxerr(a, t):.3e} of max|ref| > max({TOL:.0e}, 2 x fp32 gap {maxerr(r, t):.3e})"


def same_bits(a, b, keys=("loss", "g_depth", "g_k", "g_e"), what=""):
    for key in keys:
        assert torch.equal(a[key], b[key]), f"{what}: {key} differs between two runs ({int((a[key] != b[key]).sum())} elements)"


def paths_agree(a, b, keys=("loss", "g_depth", "g_k", "g_e"), what=""):
    for key in keys:
        err, ref = float((a[key].double() - b[key].double()).abs().max()), float(b[key].abs().max())
        print(f"[{what}] {key}: max |a - b| {err:.3e} of {ref:.3e}", flush=True)
        assert err <= PATH_REL * max(ref, 1e-30), f"{what}: {key} differs by {err:.3e} (> {PATH_REL:.0e} of {ref:.3e})"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------


def case_constants(dev=None):
    """The lists above straddle these values: they must be the sources'."""
    from flowmap_amd import _base

    track = (ROOT / "flowmap_amd" / "csrc" / "fm_track.hip").read_text()
    assert _base.TRACK_TILE == TILE
    assert re.search(r"#define FM_TRACK_PG (\d+)", track).group(1) == str(PG)
    assert re.search(r"#define FM_TRACK_AHEAD (\d+)", track).group(1) == str(AHEAD)
    assert re.search(r"constexpr unsigned kXcds = (\d+);", track).group(1) == str(XCDS)
    assert re.search(r"__launch_bounds__\((\d+)\) track_reduce_kernel", track).group(1) == str(REDUCE_BLOCK)
    for kernel in ("track_targets_kernel", "track_finalize_bwd_kernel", "inv4_kernel"):
        assert re.search(r"__launch_bounds__\((\d+)\)\s+" + kernel, track).group(1) == str(FRAME_BLOCK), kernel
    assert re.search(r"constexpr int kWave = (\d+);", (ROOT / "flowmap_amd" / "csrc" / "fm_device.h").read_text()).group(1) == str(WAVE)


def case_geometry(dev, spec):
    """One case through the path production takes by default (gradients on, the planned gather): every quantity against the fp64 truth, and
    a second run bit for bit (the planned gather and the fixed-order reduction claim to be reproducible)."""
    from flowmap_amd import _ops

    case = make_case(spec)
    check_conditions(case)
    ours = run_ours(dev, case)
    gate(case, ours)
    same_bits(run_ours(dev, case), ours, what=f"{spec.name}: planned gather")
    packed = _ops.PackedTracks(device_tracks(case, dev), torch.device(dev))
    pgroups = (packed.pmax + WAVE * PG - 1) // (WAVE * PG)
    print(f"[{spec.name}] ntiles {packed.ntiles} x pgroups {pgroups} = {packed.ntiles * pgroups} work items, pmax {packed.pmax}, fmax {packed.fmax}", flush=True)
    if spec.name.startswith("items"):
        assert packed.ntiles * pgroups == int(spec.name[5:])
    if spec.hw[1] % 4 != 0:
        assert packed.tap_plan(spec.frames, *spec.hw) is None, "a width that is no multiple of 4 has no tap plan"


def case_forward_only(dev, spec):
    """Under torch.no_grad() (the GRAD = false instantiation of track_pairs, two sums per target instead of fourteen): loss and count equal
    the grad-enabled run's bit for bit."""
    case = make_case(spec)
    with_grad, without = run_ours(dev, case), run_ours(dev, case, grad=False)
    same_bits(without, with_grad, keys=("loss", "scale"), what=f"{spec.name}: no_grad vs grad")
    assert int(without["scale"][1]) == case.count
    assert_close_or_reference_gap(without["loss"], case.truth["loss"], case.ref32["loss"], TOL, what=f"{spec.name}: loss under no_grad")


def case_backward_paths(dev, spec):
    """defer = False (no DepthSink) and defer = True with no fit downstream (the sink never parks: the same planned gather into fresh
    zeros): both against the truth, bit-identical to each other and between runs."""
    case = make_case(spec)
    plain, deferred = run_ours(dev, case, defer=False), run_ours(dev, case, defer=True)
    gate(case, plain, "defer=False")
    same_bits(plain, deferred, what=f"{spec.name}: defer=False vs defer=True")


def case_tap_image(dev, spec):
    """The compact tap image sampled (track_sample_many: branch-free, one 8-byte load per image row) and an image with holes as an in-pass
    Adam update leaves it (slots with the "read the depth image" bit, poisoned image values: the general branch) against the truth and
    against the run that samples the depth images."""
    case = make_case(spec)
    plain = run_ours(dev, case)
    for taps in ("image", "around"):
        got = run_ours(dev, case, taps=taps)
        gate(case, got, f"taps={taps}")
        paths_agree(got, plain, what=f"{spec.name}: taps={taps} vs depth images")
        same_bits(run_ours(dev, case, taps=taps), got, what=f"{spec.name}: taps={taps}")


def _cuts_a_tile(spec, frame):
    return any(start < frame < start + f and (frame - start) % TILE != 0 for start, f, _ in spec.segments)


def shard_ranges(spec, parts):
    """Two or three source ranges over the frames the segments cover, every inner boundary in the middle of a segment and of one of its
    register tiles."""
    lo, hi = min(s for s, _, _ in spec.segments), max(s + f for s, f, _ in spec.segments)
    inner = [lo + (hi - lo) // 2] if parts == 2 else [lo + (hi - lo) // 3, lo + (2 * (hi - lo)) // 3 + 1]
    for i in range(len(inner)):
        while not _cuts_a_tile(spec, inner[i]):
            inner[i] += 1
    cuts = [0, *inner, spec.frames]
    assert all(a < b for a, b in zip(cuts[:-1], cuts[1:])), (spec.name, cuts)
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]


def case_sharded(dev, spec, parts):
    """Frame sharding on one device: the tracks packed with own = (a, b) per range, depth the window, frame0 = a, a reducer that sums the
    fp64 totals of the ranges evaluated one after the other.  The summed gradients and the global loss equal the unsharded run."""
    case = make_case(spec)
    ranges = shard_ranges(spec, parts)
    assert all(_cuts_a_tile(spec, a) for a, _ in ranges[1:]), (spec.name, ranges)  # a segment, and a register tile of it, cut in the middle
    whole = run_ours(dev, case)
    local = [run_ours(dev, case, own=r, reducer=lambda totals: totals) for r in ranges]  # each range's own totals
    total = sum(r["totals"].double() for r in local)
    assert int(total[1]) == case.count, f"{spec.name}: the ranges count {int(total[1])} pairs, the reference {case.count}"
    summed = {"g_depth": torch.zeros_like(whole["g_depth"]), "g_k": torch.zeros_like(whole["g_k"]), "g_e": torch.zeros_like(whole["g_e"])}
    for (a, b), _ in zip(ranges, local):
        got = run_ours(dev, case, own=(a, b), reducer=lambda totals, total=total: total.to(totals.device))
        summed["g_depth"][:, a:b] += got["g_depth"]
        summed["g_k"] += got["g_k"]
        summed["g_e"] += got["g_e"]
        summed["loss"] = got["loss"]
        err = abs(float(got["loss"]) - float(whole["loss"]))
        assert err <= PATH_REL * abs(float(whole["loss"])), f"{spec.name}: range {(a, b)} reports loss {float(got['loss'])}, unsharded {float(whole['loss'])}"
        assert int(got["scale"][1]) == case.count
    paths_agree(summed, whole, what=f"{spec.name}: {parts} ranges vs unsharded")
    summed["scale"] = whole["scale"]
    gate(case, summed, f"{parts} ranges")


# ---- the C ABI: buffers of our own, so that flags, per-point gradients and the compact gradient can be looked at ----------------------------


def _abi_buffers(dev, case, packed, own=None):
    from flowmap_amd import _ops
    from flowmap_amd._lib import call, ptr, stream_for

    spec = case.spec
    f, (h, w) = spec.frames, spec.hw
    depth, k, e = (x.clone().to(dev).contiguous() for x in case.leaves)
    b = {"depth": depth, "k": k, "ext": e, "kinv": _ops.intrinsics_inverse(k), "ext_inv": torch.empty_like(e)}
    with _ops._guard(depth.device):
        call("fm_extrinsics_inverse", ptr(e), f, ptr(b["ext_inv"]), stream_for(e))
    total, pgroups64 = packed.total, (packed.pmax + 63) // 64
    b["ws"] = torch.zeros((total, 9), device=dev)
    b["flag"] = torch.full((total,), 7 if own is None else 0, dtype=torch.uint8, device=dev)  # (a partial pack starts from zeroed flags, as the operator does)
    b["tgt"] = torch.zeros((f, 12), device=dev)
    b["partial"] = torch.zeros((max(packed.ntiles, 1) * pgroups64 * (packed.fmax * 14 + TILE * 21),), device=dev)
    b["acc"], b["acc2"] = torch.zeros((f * 20,), dtype=torch.float64, device=dev), torch.zeros((f * 24,), dtype=torch.float64, device=dev)
    b["loss"], b["scale"], b["totals"] = torch.zeros((1,), device=dev), torch.zeros((2,), device=dev), torch.zeros((2,), dtype=torch.float64, device=dev)
    b["gws"] = torch.zeros((total, 3), device=dev)
    sc = torch.tensor(float(h * w)).sqrt()  # (in fp32, as csrc/fm_torch.cpp forms the aspect factors)
    b["aspect"] = (float(torch.tensor(float(w)) / sc), float(torch.tensor(float(h)) / sc))
    return b


def _abi_fused(dev, case, packed, own=None, frame0=0, window=None):
    """fm_track_loss_fused_fwd on buffers of our own (as csrc/fm_torch.cpp sizes them) -> the buffers."""
    from flowmap_amd import _ops
    from flowmap_amd._lib import call, ptr, stream_for

    spec = case.spec
    f, (h, w) = spec.frames, spec.hw
    b = _abi_buffers(dev, case, packed, own)
    depth = b["depth"] if window is None else b["depth"][:, window[0] : window[1]].contiguous()
    own_first, own_end = (0, f) if own is None else own
    with _ops._guard(depth.device):
        call("fm_track_loss_fused_fwd", ptr(depth), frame0, max(own_first, frame0), own_end, ptr(b["kinv"]), ptr(b["ext"]), ptr(b["ext_inv"]), ptr(b["k"]), f,
             ptr(packed.xy), ptr(packed.vis), ptr(packed.seg), ptr(packed.tiles), packed.ntiles, packed.pmax, packed.fmax, h, w,
             _ops.MAPPING_KINDS[spec.kind], DELTA, *b["aspect"], spec.weight, ptr(b["ws"]), ptr(b["flag"]), ptr(b["tgt"]), ptr(b["partial"]),
             ptr(b["acc"]), ptr(b["loss"]), ptr(b["scale"]), ptr(b["totals"]), ptr(b["gws"]), ptr(b["acc2"]), stream_for(depth))
    b["window"] = depth
    return b


def _abi_backward(dev, case, packed, b, upstream, frame0=0, frames_local=None):
    """fm_track_loss_bwd + the ATOMIC scatter fm_track_scatter (twice) + the planned gather fm_depth_gather (twice) on the buffers of a
    forward -> g_e, g_k, [atomic, atomic], [gather, gather]."""
    from flowmap_amd import _ops
    from flowmap_amd._lib import call, ptr, stream_for

    spec = case.spec
    f, (h, w) = spec.frames, spec.hw
    frames_local = f if frames_local is None else frames_local
    up = torch.tensor([upstream], device=dev)
    g_e, g_k = torch.zeros((1, f, 4, 4), device=dev), torch.zeros((1, f, 3, 3), device=dev)
    atomic, gather = [], []
    with _ops._guard(up.device):
        call("fm_track_loss_bwd", ptr(b["acc"]), ptr(b["acc2"]), ptr(b["scale"]), ptr(up), ptr(b["ext_inv"]), ptr(b["k"]), ptr(b["kinv"]), f, ptr(g_e), ptr(g_k),
             stream_for(up))
        plan = packed.scatter_plan(h, w)
        for _ in range(2):
            out = torch.zeros((1, frames_local, h, w), device=dev)
            if packed.nblocks > 0:
                call("fm_track_scatter", ptr(b["gws"]), ptr(b["flag"]), ptr(packed.xy), ptr(packed.vis), ptr(packed.seg), ptr(packed.blocks), packed.nblocks,
                     packed.pmax, ptr(b["kinv"]), ptr(b["scale"]), ptr(up), h, w, frame0, ptr(out), stream_for(out))
            atomic.append(out.cpu())
            out = torch.zeros((1, frames_local, h, w), device=dev)
            if plan is not None:
                pixels, first, entries, weights = plan
                call("fm_depth_gather", ptr(b["gws"]), ptr(pixels), ptr(first), ptr(entries), ptr(weights), pixels.numel(), ptr(b["kinv"]), ptr(b["scale"]),
                     ptr(up), h, w, frame0, ptr(out), stream_for(out))
            gather.append(out.cpu())
    return g_e.cpu(), g_k.cpu(), atomic, gather


def case_atomic_scatter(dev, spec):
    """The entry points of the fused forward and of both backward forms through the C ABI: the atomic scatter (fm_track_scatter: two runs
    agree at the bound of cases.case_track_scatter_plan), the planned gather (two runs bit for bit), each against the truth and against
    the operator."""
    from flowmap_amd import _ops

    case = make_case(spec)
    packed = _ops.PackedTracks(device_tracks(case, dev), torch.device(dev))
    b = _abi_fused(dev, case, packed)
    g_e, g_k, atomic, gather = _abi_backward(dev, case, packed, b, spec.upstream)
    assert torch.equal(gather[0], gather[1]), f"{spec.name}: two runs of the planned gather differ"
    assert_close(atomic[0], atomic[1], SCATTER_REL, abs_=SCATTER_ABS, what=f"{spec.name}: two runs of the atomic scatter")
    assert_close(gather[0], atomic[0], SCATTER_REL, abs_=SCATTER_ABS, what=f"{spec.name}: gather vs atomic scatter")
    operator = run_ours(dev, case)
    for g_depth, what in ((atomic[0], "atomic scatter"), (gather[0], "planned gather")):
        ours = {"loss": b["loss"].cpu().reshape(()), "scale": b["scale"].cpu(), "g_depth": g_depth, "g_k": g_k, "g_e": g_e}
        gate(case, ours, f"C ABI, {what}")
        paths_agree(ours, operator, what=f"{spec.name}: C ABI ({what}) vs operator")
    # the flags: 1 exactly for the visible sources inside the frame
    want = ((packed.vis != 0) & (packed.xy >= 0).all(-1) & (packed.xy < 1).all(-1)).to(torch.uint8)
    assert torch.equal(b["flag"], want), f"{spec.name}: flags"


def case_sharded_flags(dev, spec, parts):
    """own = (a, b) through the C ABI: the flags of sources this range does not own are 0, those it owns are the unsharded flags; the ranges'
    per-point gradients and fp64 totals add up to the unsharded run's."""
    from flowmap_amd import _ops

    case = make_case(spec)
    tracks = device_tracks(case, dev)
    whole_pack = _ops.PackedTracks(tracks, torch.device(dev))
    whole = _abi_fused(dev, case, whole_pack)
    frame_of = torch.zeros((whole_pack.total,), dtype=torch.int64)
    for start, f, p, off in whole_pack.seg.cpu().tolist():
        frame_of[off : off + f * p] = start + torch.arange(f).repeat_interleave(p)
    totals, gws = torch.zeros((2,), dtype=torch.float64), torch.zeros_like(whole["gws"].cpu())
    for a, b_ in shard_ranges(spec, parts):
        packed = _ops.PackedTracks(tracks, torch.device(dev), (a, b_))
        assert packed.ntiles > 0, (spec.name, a, b_)
        got = _abi_fused(dev, case, packed, own=(a, b_), frame0=a, window=(a, b_))
        owned = (frame_of >= a) & (frame_of < b_)
        flag = got["flag"].cpu()
        assert int(flag[~owned].sum()) == 0, f"{spec.name}: range {(a, b_)} flags {int(flag[~owned].sum())} sources it does not own"
        assert torch.equal(flag[owned], whole["flag"].cpu()[owned]), f"{spec.name}: range {(a, b_)}: flags of its own sources"
        totals += got["totals"].cpu()
        live = owned & (flag != 0)
        gws[live] += got["gws"].cpu()[live]
    assert float(totals[1]) == float(whole["totals"][1]) == case.count
    assert abs(float(totals[0]) - float(whole["totals"][0])) <= PATH_REL * float(whole["totals"][0])
    live = whole["flag"].cpu() != 0
    err, ref = float((gws[live] - whole["gws"].cpu()[live]).abs().max()), float(whole["gws"].cpu()[live].abs().max())
    assert err <= PATH_REL * ref, f"{spec.name}: per-point gradients of the ranges differ from the unsharded run's by {err:.3e} of {ref:.3e}"


def case_unfused_entry_points(dev, spec):
    """fm_track_points + fm_track_loss_fwd (sampling in a launch of its own, ws / flag read back by the pair kernel) are reached by nothing
    in the package any more, but they are part of the C ABI: compared with the fused forward on the same inputs."""
    from flowmap_amd import _ops
    from flowmap_amd._lib import call, ptr, stream_for

    case = make_case(spec)
    f, (h, w) = spec.frames, spec.hw
    packed = _ops.PackedTracks(device_tracks(case, dev), torch.device(dev))
    fused = _abi_fused(dev, case, packed)
    b = _abi_buffers(dev, case, packed)
    with _ops._guard(b["depth"].device):
        call("fm_track_points", ptr(b["depth"]), 0, ptr(b["kinv"]), ptr(b["ext"]), ptr(b["ext_inv"]), ptr(b["k"]), f, ptr(packed.xy), ptr(packed.vis),
             ptr(packed.seg), ptr(packed.blocks), packed.nblocks, packed.pmax, h, w, ptr(b["ws"]), ptr(b["flag"]), ptr(b["tgt"]), stream_for(b["depth"]))
        call("fm_track_loss_fwd", ptr(b["ws"]), ptr(b["flag"]), ptr(packed.xy), ptr(packed.vis), ptr(packed.seg), ptr(packed.tiles), packed.ntiles, packed.pmax,
             packed.fmax, ptr(b["ext"]), ptr(b["tgt"]), f, h, w, _ops.MAPPING_KINDS[spec.kind], DELTA, *b["aspect"], spec.weight, ptr(b["partial"]),
             ptr(b["acc"]), ptr(b["loss"]), ptr(b["scale"]), ptr(b["totals"]), ptr(b["gws"]), ptr(b["acc2"]), stream_for(b["depth"]))
    assert torch.equal(b["flag"], fused["flag"]) and torch.equal(b["tgt"], fused["tgt"])
    assert float(b["scale"][1]) == float(fused["scale"][1]) == case.count
    err, ref = abs(float(b["loss"]) - float(fused["loss"])), abs(float(fused["loss"]))
    print(f"[{spec.name}: unfused vs fused] loss: {err:.3e} of {ref:.3e}", flush=True)
    assert err <= PATH_REL * ref, f"{spec.name}: the loss of the unfused entry points differs by {err:.3e} of {ref:.3e}"
    # The per-point and per-frame gradient sums are two fp32 evaluations of one quantity: track_points and the sampling prologue of track_pairs
    # round X_w differently in the last bit (one skips a tap outside the image, the other weighs it with an exact zero: other contractions),
    # and beyond the Huber kink a residual's gradient is its DIRECTION r / |r|, which moves by ulp(u) / |r| — 1e-5 of itself at |r| = delta.
    # That is the rounding the gate allows either of them against the fp64 truth (below), so they are held to each other at the gate's
    # floor, norm-wise; the bound between paths that share their per-point arithmetic (PATH_REL) does not apply to them.
    live = (b["flag"] != 0).cpu()
    pairs = {"gws": (b["gws"].cpu()[live], fused["gws"].cpu()[live]), "acc": (b["acc"], fused["acc"]), "acc2": (b["acc2"], fused["acc2"])}
    for key, (x, y) in pairs.items():
        err = relerr(x, y)
        print(f"[{spec.name}: unfused vs fused] {key}: rel {err:.3e} (max-abs of max {maxerr(x, y):.3e})", flush=True)
        assert err <= TOL, f"{spec.name}: {key} of the unfused entry points differs from the fused forward's by {err:.3e} (> {TOL:.0e})"
    g_e, g_k, atomic, _ = _abi_backward(dev, case, packed, b, spec.upstream)
    gate(case, {"loss": b["loss"].cpu().reshape(()), "scale": b["scale"].cpu(), "g_depth": atomic[0], "g_k": g_k, "g_e": g_e}, "unfused entry points")


def case_tap_gradient(dev, spec):
    """fm_track_loss_fused_fwd_taps through the C ABI: the compact dL/ddepth at the static taps (tap_grad) — stored by the epilogue of
    track_pairs for the taps one point owns and summed by tap_grad_kernel for the shared ones (shared_ranks), or all of it by
    tap_grad_kernel — with the depths sampled from the depth images (slots only: the first step after registration) and from the compact
    image.  scale * upstream * tap_grad at the plan's pixels is the tracking loss's dL/ddepth."""
    from flowmap_amd import _ops
    from flowmap_amd._lib import call, ptr, stream_for

    case = make_case(spec)
    f, (h, w) = spec.frames, spec.hw
    packed = _ops.PackedTracks(device_tracks(case, dev), torch.device(dev))
    plan = packed.tap_plan(f, h, w)
    assert plan is not None
    pixels, first, entries, weights = plan.plan
    if spec.edit == "tap_edges":
        assert plan.shared_ranks.numel() > 0, "the tap-edge case has shared taps"
        assert int(pixels[-1]) == f * h * w - 1, "the tap-edge case has a tap on the last pixel of the last frame"
        assert int((plan.slots.reshape(-1, 4)[:, 0::2] >= 0).sum()) > int((plan.slots.reshape(-1, 4)[:, 1::2] >= 0).sum()), "clipped taps"
    reference = _abi_fused(dev, case, packed)
    _, _, _, gather = _abi_backward(dev, case, packed, reference, spec.upstream)
    results = {}
    for sampled in (False, True):
        for shared in (True, False):
            b = _abi_buffers(dev, case, packed)
            image = b["depth"].reshape(-1)[pixels].clone() if sampled else None
            if image is not None:
                image = torch.cat([image, image.new_zeros(1)])[: pixels.numel()]  # (padded by one value, as TapPlan.image is)
            tap_grad = torch.full((pixels.numel(),), float("nan"), device=dev)  # every tap must be written
            ranks = plan.shared_ranks if shared else None
            with _ops._guard(b["depth"].device):
                call("fm_track_loss_fused_fwd_taps", ptr(b["depth"]), ptr(b["kinv"]), ptr(b["ext"]), ptr(b["ext_inv"]), ptr(b["k"]), f, ptr(packed.xy),
                     ptr(packed.vis), ptr(packed.seg), ptr(packed.tiles), packed.ntiles, packed.pmax, packed.fmax, h, w, _ops.MAPPING_KINDS[spec.kind], DELTA,
                     *b["aspect"], spec.weight, ptr(b["ws"]), ptr(b["flag"]), ptr(b["tgt"]), ptr(b["partial"]), ptr(b["acc"]), ptr(b["loss"]), ptr(b["scale"]),
                     ptr(b["totals"]), ptr(b["gws"]), ptr(b["acc2"]), ptr(plan.slots), ptr(image), ptr(pixels), ptr(first), ptr(entries), ptr(weights),
                     pixels.numel(), ptr(ranks), 0 if ranks is None else ranks.numel(), ptr(tap_grad), stream_for(b["depth"]))
            what = f"taps entry point (image {'sampled' if sampled else 'not sampled'}, {'direct stores + shared taps' if shared else 'tap_grad_kernel alone'})"
            assert bool(torch.isfinite(tap_grad).all()), f"{spec.name}: {what}: {int((~torch.isfinite(tap_grad)).sum())} taps were never written"
            dense = torch.zeros((f * h * w,), device=dev)
            dense[pixels] = tap_grad * (b["scale"][0] * spec.upstream)
            g_e, g_k, _, _ = _abi_backward(dev, case, packed, b, spec.upstream)
            ours = {"loss": b["loss"].cpu().reshape(()), "scale": b["scale"].cpu(), "g_depth": dense.reshape(1, f, h, w).cpu(), "g_k": g_k, "g_e": g_e}
            gate(case, ours, what)
            paths_agree({"g_depth": ours["g_depth"], "loss": ours["loss"]}, {"g_depth": gather[0], "loss": reference["loss"].cpu().reshape(())},
                        keys=("loss", "g_depth"), what=f"{spec.name}: {what} vs planned gather")
            results[(sampled, shared)] = ours
    for sampled in (False, True):
        paths_agree(results[(sampled, True)], results[(sampled, False)], what=f"{spec.name}: direct stores vs tap_grad_kernel alone")


# ---- a whole step: the tap exchange with a flow loss beside the tracking loss --------------------------------------------------------------


def case_step_tap_exchange(dev, spec, steps=4):
    """The paths only a step with a flow loss reaches: from the second step on the tracking loss runs AHEAD of the flow pass and offers its
    compact gradient (direct tap_grad stores), which that pass absorbs; from the third it samples the compact image the pass left.  Each
    step's tracking loss and every gradient equal the same step run with the exchange off (where the tracking loss takes the path the
    cases above hold against the fp64 truth), and the tracking loss's own depth contribution — the step's dL/ddepth less the flow-only
    step's — is compared the same way, so that it cannot hide under the flow loss's."""
    import flowmap_amd
    from cases import _small_problem
    from flowmap_amd import _ops
    from flowmap_amd.config import override
    from flowmap_amd.loss import LossFlow, LossFlowCfg, LossTracking, LossTrackingCfg
    from helpers import mapping_cfg

    case = make_case(spec)
    f, (h, w) = spec.frames, spec.hw

    def run(exchange, tracking=True):
        with override(tap_exchange=exchange, tap_exchange_min_bytes=0):
            model, batch, flows, _ = _small_problem(dev, f=f, h=h, w=w, tracking=False, seed=33, points=40)
            tracks = device_tracks(case, dev)
            flow_fn = LossFlow(LossFlowCfg(0, 1000.0, "flow", mapping_cfg("huber")))
            track_fn = LossTracking(LossTrackingCfg(0, spec.weight, "tracking", mapping_cfg(spec.kind, DELTA)))
            results = []
            for step in range(steps):
                model.zero_grad(set_to_none=True)
                out = model(batch, flows, step)
                lf = flow_fn(batch, flows, tracks, out, step)
                lt = track_fn(batch, flows, tracks, out, step) if tracking else torch.zeros((), device=dev)
                (lf + lt).backward()
                results.append({"loss_tracking": lt.detach().cpu().clone(), "g_depth": model.backbone.depth.grad.cpu().clone(),
                                "g_wlogit": model.backbone.weights.grad.cpu().clone(), "g_focal": model.intrinsics.focal_length.grad.cpu().clone()})
            return results

    try:
        before = dict(_ops.counters)
        flow_only = run(False, tracking=False)
        plain = run(False)
        assert _ops.counters["flow_tap_passes"] == before["flow_tap_passes"] and _ops.counters["track_tap_samples"] == before["track_tap_samples"]
        got = run(True)
        assert _ops.counters["flow_tap_absorbs"] - before["flow_tap_absorbs"] == steps - 1, _ops.counters
        assert _ops.counters["track_tap_samples"] - before["track_tap_samples"] == steps - 2, _ops.counters  # from the third step on
    finally:
        flowmap_amd.set_lazy_surfaces(False)
    for step, (a, b, c) in enumerate(zip(got, plain, flow_only)):
        assert float(b["loss_tracking"]) > 0
        paths_agree(a, b, keys=("loss_tracking", "g_depth", "g_wlogit", "g_focal"), what=f"{spec.name}: step {step}, exchange on vs off")
        own_a, own_b = a["g_depth"] - c["g_depth"], b["g_depth"] - c["g_depth"]
        ref = float(own_b.abs().max())
        assert ref > 0, "the tracking loss contributes to dL/ddepth"
        # (two fp32 differences of sums whose flow part is up to |g_depth| / |own| times larger: the bound is of the step's gradient)
        err = float((own_a - own_b).abs().max())
        print(f"[{spec.name}: step {step}] the tracking loss's own dL/ddepth: {err:.3e} of {ref:.3e} (step gradient {float(b['g_depth'].abs().max()):.3e})", flush=True)
        assert err <= PATH_REL * float(b["g_depth"].abs().max())


def case_step_in_pass_adam(dev, spec, steps=6, lr=1e-3):
    """The image an in-pass Adam update leaves (FusedAdam.fuse_depth_update): the flow pass updates depth where it writes its gradient, the
    taps included, and the image holds the UPDATED depth except at the pixels the element-list update finishes later — their slots carry
    the "read the depth image" bit, the general branch of track_sample_many.  Every step's tracking loss (sampled from that image once it
    exists) equals the loss evaluated from the depth images on the same parameters, just before the step's flow pass moves them.
    (Two optimiser trajectories are not compared: Adam turns a difference in the last bit of a small gradient into a difference of lr.)"""
    import flowmap_amd
    from cases import _small_problem
    from flowmap_amd import FusedAdam, _ops
    from flowmap_amd.config import override
    from flowmap_amd.loss import LossFlow, LossFlowCfg, LossTracking, LossTrackingCfg
    from flowmap_amd.model.projection import _dense_extrinsics
    from helpers import mapping_cfg

    case = make_case(spec)
    f, (h, w) = spec.frames, spec.hw
    around, history = [], []
    try:
        with override(tap_exchange=True, tap_exchange_min_bytes=0):
            before = dict(_ops.counters)
            model, batch, flows, _ = _small_problem(dev, f=f, h=h, w=w, tracking=False, seed=33, points=40)
            tracks = device_tracks(case, dev)
            packed = _ops.PackedTracks(tracks, torch.device(dev))
            flow_fn = LossFlow(LossFlowCfg(0, 1000.0, "flow", mapping_cfg("huber")))
            track_fn = LossTracking(LossTrackingCfg(0, spec.weight, "tracking", mapping_cfg(spec.kind, DELTA)))
            optimizer = FusedAdam(model.parameters(), lr=lr)
            optimizer.fuse_depth_update(model.backbone.depth, max_touched_fraction=1.0)
            start = model.backbone.depth.detach().cpu().clone()
            for step in range(steps):
                optimizer.zero_grad(set_to_none=True)
                out = model(batch, flows, step)
                with torch.no_grad():  # from the depth images, on the parameters as this step finds them
                    want = _ops.TrackLossFused.apply(out.depths, out.intrinsics, _dense_extrinsics(out.extrinsics), packed, spec.weight,
                                                     _ops.MAPPING_KINDS[spec.kind], DELTA, False).detach().cpu().clone()
                sampled = _ops.counters["track_tap_samples"]
                total = flow_fn(batch, flows, tracks, out, step)
                lt = track_fn(batch, flows, tracks, out, step)
                (total + lt).backward()
                optimizer.step()
                plan = _ops._root(out.depths).__dict__.get("_fm_tap_plan")
                holes = 0 if plan is None or plan.image_slots is plan.slots else int(((plan.image_slots >= 0) & ((plan.image_slots & 0x20000000) != 0)).sum())
                around.append(holes)
                history.append((lt.detach().cpu().clone(), want, _ops.counters["track_tap_samples"] > sampled))
            assert optimizer.counters["in_pass_updates"] >= steps - 3, optimizer.counters
            assert _ops.counters["track_tap_samples"] - before["track_tap_samples"] >= steps - 3, _ops.counters
            assert max(around) > 0, "no slot ever carried the read-the-depth-image bit"
            assert float((model.backbone.depth.detach().cpu() - start).abs().max()) > 1e-3  # (the parameter moves: every image is another one)
    finally:
        flowmap_amd.set_lazy_surfaces(False)
    for step, (got, want, from_image) in enumerate(history):
        err = abs(float(got) - float(want))
        print(f"[{spec.name}: in-pass Adam, step {step}] tracking loss {float(got):.7e} ({'tap image' if from_image else 'depth images'}), from the depth images "
              f"{float(want):.7e}: {err:.3e}; slots reading the depth image: {around[step]}", flush=True)
        assert float(want) > 0 and err <= PATH_REL * float(want), f"{spec.name}: step {step}: tracking loss {float(got)} vs {float(want)} from the depth images"


# ---- arguments that would launch out of range: refused by the host layer (CPU module only) -------------------------------------------------


def case_refusals(dev):
    """A segment past the last frame, a depth window past the video, own_end < own_first: refused before anything is launched."""
    from flowmap_amd import _ops
    from flowmap_amd._lib import call, ptr

    case = make_case(P_CASES[4])
    spec = case.spec
    depth, k, e = (x.clone().to(dev) for x in case.leaves)
    packed = _ops.PackedTracks(device_tracks(case, dev), torch.device(dev))
    kind = _ops.MAPPING_KINDS[spec.kind]
    with pytest.raises(RuntimeError, match="past the last frame"):
        _ops.TrackLossFused.apply(depth[:, :5].contiguous(), k[:, :5].contiguous(), e[:, :5].contiguous(), packed, 1.0, kind, DELTA, True)
    with pytest.raises(RuntimeError, match="cover the whole video"):
        _ops.TrackLossFused.apply(depth, k, e, packed, 1.0, kind, DELTA, True, 1)  # frame0 + frames of depth > frames of the video
    with pytest.raises(RuntimeError, match="cover the whole video"):
        _ops.TrackLossFused.apply(depth, k[:, :7].contiguous(), e, packed, 1.0, kind, DELTA, True)
    late = [orc.OTracks(t.xy, t.visibility, t.start_frame + 2) for t in case.tracks]
    from helpers import to_tracks

    with pytest.raises(RuntimeError, match="past the last frame"):
        _ops.TrackLossFused.apply(depth, k, e, _ops.PackedTracks(to_tracks(late, dev), torch.device(dev)), 1.0, kind, DELTA, True)
    # the entry point itself: own_end < own_first, own_first < depth_frame0, no tiles, a mapping kind that does not exist
    b = _abi_buffers(dev, case, packed)
    f, (h, w) = spec.frames, spec.hw

    def fused(frame0, own_first, own_end, ntiles=packed.ntiles, mapping=kind):
        call("fm_track_loss_fused_fwd", ptr(b["depth"]), frame0, own_first, own_end, ptr(b["kinv"]), ptr(b["ext"]), ptr(b["ext_inv"]), ptr(b["k"]), f, ptr(packed.xy),
             ptr(packed.vis), ptr(packed.seg), ptr(packed.tiles), ntiles, packed.pmax, packed.fmax, h, w, mapping, DELTA, *b["aspect"], 1.0, ptr(b["ws"]),
             ptr(b["flag"]), ptr(b["tgt"]), ptr(b["partial"]), ptr(b["acc"]), ptr(b["loss"]), ptr(b["scale"]), ptr(b["totals"]), ptr(b["gws"]), ptr(b["acc2"]), None)

    b["loss"].fill_(-3.0)
    for args in ((0, 5, 3), (2, 1, 6), (-1, 0, 8), (0, 0, 8, 0), (0, 0, 8, packed.ntiles, 3)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            fused(*args)
    assert float(b["loss"]) == -3.0 and int(b["flag"].max()) == 7 and float(b["gws"].abs().max()) == 0.0, "a refused call wrote to its buffers"
    fused(0, 0, 8)
    assert float(b["loss"]) > 0
