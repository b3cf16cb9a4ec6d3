"""LossTracking.residuals (fm_track_residuals): per (source frame, target frame, point) the unmasked tracking term, the visibility and the
reprojected position, and the per-pair / per-track sums, straight from depth.  The cases here take a device;
tests/test_hostsim_track_residuals.py runs them on the serial host double of the C ABI, tests/test_gpu_track_residuals.py on the MI355X.

Inputs, the margin rule and the oracle are tests/track_geometry_cases.py's: independent random leaves (depth, a K per frame, rigid E),
tracks with their own P and f per segment, and ``make_case`` clears the source bit of every pair whose target lies within EDGE_MARGIN of
the frame edge — so ``visible`` and the counts are compared EXACTLY with the fp64 oracle (``check_conditions`` caps the altered share at
1 %; ``case_negative_control`` shows the equality is not vacuous).  Truth: ``orc.track_positions`` + ``orc.robust`` in fp64 on the case's
leaves; ``ref32``: the same in torch fp32.  tests/golden/fn_track_residuals.npz holds what the REFERENCE computes on two small track lists
(tools/make_golden_track_residuals.py).  The gate is the project's:
  norm-wise      conftest.assert_close_or_reference_gap(ours, truth64, ref32, rel=1e-4, slack=2.0)
  element-wise   conftest.maxerr <= max(10 x 1e-4, 2 x the fp32 reference's own maxerr)      (assert_grad_close's convention)
  visible, pair_count, track_count: equal to the fp64 oracle's.
Every figure is printed before it is asserted."""

from __future__ import annotations

import functools

import torch

import track_geometry_cases as tg
from conftest import assert_close, assert_close_or_reference_gap, load_golden, maxerr, relerr, t
from helpers import mapping_cfg
from operator_checks import assert_training_untouched, host_tensor_refused, same_tensors, train, ulp_distance
from oracle import flowmap_oracle as orc
from track_geometry_cases import DELTA, SPECS, TOL, Spec, check_conditions, device_tracks, make_case  # noqa: F401

KINDS = ("huber", "l1", "l2")
THREADS = 256  # fm_track_residuals.hip: kTrResThreads — points per workgroup; a wave of 64 of them shares one workspace slot per pair
# The launch-geometry list: the names of track_geometry_cases.SPECS, straddling the wave (P63/64/65) and the workgroup (P255/256/257)
GEOMETRY = ("P1", "P63", "P64", "P65", "P255", "P256", "P257", "f1", "f2", "f7", "f13", "mixed", "mixed-10x13", "F65", "items260", "mixed-l1",
            "mixed-l2", "tap-edges", "source-outside", "nothing-visible")
FIXTURE_CASES = ("a", "b")


# ---- the fixture's inputs (tools/make_golden_track_residuals.py draws them from here) ------------------------------------------------


def _edit_fixture(spec, leaves, tracks):
    """A few source positions outside the frame with their bit set, and a few invisible bits among visible neighbours."""
    first = tracks[0]
    for fr in range(first.xy.shape[1]):
        first.xy[0, fr, fr % 3, 0] = -0.03
        first.xy[0, fr, 3 + fr % 2, 1] = 1.0
        first.visibility[0, fr, :6] = True
        first.visibility[0, fr, 6 + fr % 4] = False
    last = tracks[-1]
    last.xy[0, 0, 0, 0] = 1.2
    last.visibility[0, 0, 0] = True
    last.visibility[0, -1, 1] = False


FIXTURE_SPECS = {
    "a": Spec("fixture-a", 5, (9, 12), ((0, 5, 40), (1, 3, 7)), seed=41),
    "b": Spec("fixture-b", 5, (10, 13), ((0, 2, 65), (2, 3, 5), (0, 5, 3)), seed=42),
}


@functools.lru_cache(maxsize=None)
def fixture_inputs(name):
    """(leaves, tracks, altered, points) of a fixture case: track_geometry_cases' generators, the edit above, the margin rule."""
    spec = FIXTURE_SPECS[name]
    leaves, tracks = tg.make_leaves(spec), tg.make_tracks(spec)
    _edit_fixture(spec, leaves, tracks)
    altered, points = tg.apply_margins(spec, leaves, tracks)
    return leaves, tracks, altered, points


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("fn_track_residuals")


def golden_problem(name):
    """(spec, leaves, tracks) as the fixture file holds them."""
    g = golden()
    spec = FIXTURE_SPECS[name]
    leaves = tuple(t(g[f"{name}_{key}"]) for key in ("depth", "k", "extrinsics"))
    tracks = [orc.OTracks(t(g[f"{name}_seg{i}_xy"]), t(g[f"{name}_seg{i}_visibility"]), int(g[f"{name}_seg{i}_start"])) for i in range(int(g[f"{name}_n_segments"]))]
    assert tuple(leaves[0].shape[1:]) == (spec.frames, *spec.hw) and len(tracks) == len(spec.segments)
    return spec, leaves, tracks


def golden_terms(name, kind):
    """-> (truth64, ref32): per segment {residual, visible, xy_target} as the reference computed them."""
    g = golden()
    out = []
    for prefix in (f"{name}_f64_", f"{name}_"):
        out.append([{"residual": t(g[f"{prefix}seg{i}_{kind}"]), "visible": t(g[f"{prefix}seg{i}_visible"]), "xy_target": t(g[f"{prefix}seg{i}_xy_target"])}
                    for i in range(int(g[f"{name}_n_segments"]))])
    return out


# ---- truth -----------------------------------------------------------------------------------------------------------------------------

_TERMS: dict = {}


def oracle_terms(key, leaves, tracks, hw, kind):
    """-> (truth64, ref32) per segment from orc.track_positions + orc.robust on the leaves; computed once per (key, kind), never written to."""
    if (key, kind) not in _TERMS:
        out = []
        for dtype in (torch.float64, torch.float32):
            depth, k, e = (x.to(dtype) for x in leaves)
            surfaces = tg._surfaces(depth, k, hw)
            per_segment = []
            with torch.no_grad():
                for seg in tracks:
                    s, f = seg.start_frame, seg.xy.shape[1]
                    seg_t = orc.OTracks(seg.xy.to(dtype), seg.visibility, s)
                    xy_target, visible = orc.track_positions(surfaces[:, s : s + f], e[:, s : s + f], k[:, s : s + f], seg_t)
                    per_segment.append({"residual": orc.robust(xy_target, seg_t.xy[:, None], hw, kind, DELTA), "visible": visible, "xy_target": xy_target})
            out.append(per_segment)
        _TERMS[(key, kind)] = tuple(out)
    return _TERMS[(key, kind)]


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------


def problem(leaves, tracks, hw, dev, kind="huber", lazy=True):
    """(loss, batch, tracks, model_output): lazy surfaces of the output's own depths (the fused route) or the explicit tensor (general)."""
    from flowmap_amd import Batch, ModelOutput
    from flowmap_amd.loss import LossTracking, LossTrackingCfg
    from flowmap_amd.model.projection import LazySurfaces
    from helpers import to_tracks

    depth, k, e = (x.clone().to(dev) for x in leaves)
    surfaces = LazySurfaces(depth, k)
    if not lazy:
        surfaces = surfaces.materialize()
    out = ModelOutput(depth, surfaces, k, e, None)
    loss = LossTracking(LossTrackingCfg(0, 100.0, "tracking", mapping_cfg(kind, DELTA)))
    return loss, Batch(torch.zeros((1, depth.shape[1], 3, *hw), device=dev)), to_tracks(tracks, dev), out


def case_problem(case, dev, lazy=True):
    return problem(case.leaves, case.tracks, case.spec.hw, dev, case.spec.kind, lazy)


def masked64(residual, visible):
    return torch.where(visible, residual.double(), torch.zeros((), dtype=torch.float64, device=residual.device))


def check_segment(r, truth, ref32, what, skip=None):
    """The gate of the module docstring on one TrackResiduals.  ``skip``: a boolean (1,f,f,P) mask of elements left out of the value
    comparisons (the camera-plane element, whose fp64 value is not the clamped one)."""
    f, p = truth["residual"].shape[1], truth["residual"].shape[3]
    assert r.residual.shape == (1, f, f, p) and r.residual.dtype == torch.float32 and not r.residual.requires_grad, what
    assert r.visible.shape == (1, f, f, p) and r.visible.dtype == torch.bool, what
    keep = torch.ones_like(truth["visible"]) if skip is None else ~skip
    fields = [("residual", r.residual.cpu(), truth["residual"], ref32["residual"])]
    if r.xy_target is not None:
        assert r.xy_target.shape == (1, f, f, p, 2) and r.xy_target.dtype == torch.float32, what
        fields.append(("xy_target", r.xy_target.cpu(), truth["xy_target"], ref32["xy_target"]))
    for name, a, tr, rf in fields:
        assert bool(torch.isfinite(a).all()), f"{what}: {name} is not finite"
        a, tr, rf = a[keep], tr[keep], rf[keep]
        err, gap, worst, worst_ref = relerr(a, tr), relerr(rf, tr), maxerr(a, tr), maxerr(rf, tr)
        print(f"[{what}] {name}: ours/fp64 {err:.3e}  fp32 reference/fp64 {gap:.3e}  max-abs of max|ref| {worst:.3e} / {worst_ref:.3e}", flush=True)
        assert_close_or_reference_gap(a, tr, rf, rel=TOL, slack=2.0, what=f"{what}: {name}")
        assert worst <= max(10 * TOL, 2.0 * worst_ref), f"{what}: {name} max-abs err {worst:.3e} of max|ref| > max({10 * TOL:.0e}, 2 x fp32 gap {worst_ref:.3e})"
    differ = int((r.visible.cpu() != truth["visible"]).sum())
    print(f"[{what}] visible: {int(truth['visible'].sum())} of {truth['visible'].numel()} in fp64, {differ} differ", flush=True)
    assert differ == 0, f"{what}: visible differs from the fp64 oracle at {differ} elements"
    if r.pair_sum is None:
        return
    vis = truth["visible"]
    assert r.pair_sum.shape == (f, f) and r.track_sum.shape == (p,) and r.pair_sum.dtype == torch.float64 and r.track_count.dtype == torch.float64
    assert torch.equal(r.pair_count.cpu(), vis[0].double().sum(dim=2)), f"{what}: pair_count differs from the fp64 oracle's"
    assert torch.equal(r.track_count.cpu(), vis[0].double().sum(dim=(0, 1))), f"{what}: track_count differs from the fp64 oracle's"
    shown64, shown32 = masked64(truth["residual"], vis)[0], masked64(ref32["residual"], vis)[0]
    for name, ours, dims in (("pair_sum", r.pair_sum.cpu(), 2), ("track_sum", r.track_sum.cpu(), (0, 1))):
        want, ref = shown64.sum(dim=dims), shown32.sum(dim=dims)
        if float(want.abs().max()) == 0.0:
            assert float(ours.abs().max()) == 0.0, f"{what}: {name} must be exactly 0 where nothing is visible"
            continue
        err, gap = assert_close_or_reference_gap(ours, want, ref, rel=TOL, slack=2.0, what=f"{what}: {name}")
        print(f"[{what}] {name}: ours/fp64 {err:.3e}  fp32 reference/fp64 {gap:.3e}", flush=True)


def same_fields(a, b, what="", **kw):
    same_tensors(a, b, ("residual", "visible", "xy_target", "pair_sum", "pair_count", "track_sum", "track_count"), what, scalars=("segment", "start_frame"), **kw)


# ---- 1: reference parity ------------------------------------------------------------------------------------------------------------------


def case_reference_parity(dev, name, kind):
    """The fixture — what the reference's own compute_track_flow and mapping give in fp32 and fp64 — maps, visibility, positions, sums."""
    spec, leaves, tracks = golden_problem(name)
    again = fixture_inputs(name)  # the generator still draws what the file holds (the margin rule was applied before it was written)
    assert all(torch.equal(a, b) for a, b in zip(leaves, again[0])) and all(torch.equal(x.xy, y.xy) and torch.equal(x.visibility, y.visibility) for x, y in zip(tracks, again[1]))
    print(f"[fixture {name}] altered {again[2]} of {again[3]} points", flush=True)
    assert again[2] <= tg.ALTERED_CAP * again[3]
    truth, ref32 = golden_terms(name, kind)
    loss, batch, trk, out = problem(leaves, tracks, spec.hw, dev, kind)
    rs = loss.residuals(batch, trk, out, predicted=True)
    assert len(rs) == len(tracks)
    for i, r in enumerate(rs):
        assert torch.equal(truth[i]["visible"], ref32[i]["visible"]), "the fixture's fp32 and fp64 visibility differ: regenerate it"
        assert r.segment == i and r.start_frame == tracks[i].start_frame
        check_segment(r, truth[i], ref32[i], f"fixture {name}/{kind} segment {i}")
    assert sum(int(x["visible"].sum()) for x in truth) > 0
    # the reference and the oracle are the same arithmetic: their fp64 maps agree to fp64 rounding
    for mine, theirs in zip(oracle_terms(("fixture", name), leaves, tracks, spec.hw, kind)[0], truth):
        assert_close(mine["residual"], theirs["residual"], 1e-9, what="oracle vs reference, fp64")
        assert torch.equal(mine["visible"], theirs["visible"])


# ---- 2: launch geometry ---------------------------------------------------------------------------------------------------------------------


def case_geometry(dev, spec_name):
    case = make_case(SPECS[spec_name])
    check_conditions(case)
    spec = case.spec
    truth, ref32 = oracle_terms(spec.geometry, case.leaves, case.tracks, spec.hw, spec.kind)
    loss, batch, trk, out = case_problem(case, dev)
    rs = loss.residuals(batch, trk, out, predicted=True)
    assert len(rs) == len(spec.segments)
    for i, (r, (start, f, p)) in enumerate(zip(rs, spec.segments)):
        assert (r.segment, r.start_frame) == (i, start)
        check_segment(r, truth[i], ref32[i], f"{spec.name} segment {i} (start {start}, f {f}, P {p})")
    count = sum(int(r.pair_count.sum()) for r in rs)
    assert count == case.count, f"{spec.name}: {count} visible, the fp64 reference counts {case.count}"
    if not spec.visible:
        for r in rs:
            assert float(r.pair_loss().abs().max()) == 0.0 and float(r.track_loss().abs().max()) == 0.0, "nothing visible: the losses are 0, not NaN"


# ---- 3: the sums ------------------------------------------------------------------------------------------------------------------------------


def case_sums(dev, spec_name):
    """Per segment: pair_sum and track_sum against the fp64 sums of the RETURNED fp32 map where visible — the same terms, (double)ρ or 0, in
    another order: |Δ| <= N · 2^-52 · Σ terms with N = f·f·P non-negative terms; their totals agree within the same bound and the counts'
    totals exactly.  Two calls bit-equal; a window bit-equal, maps and sums, to the same segments of the full call; what was not asked for
    is not produced."""
    import pytest

    from flowmap_amd import _ops

    case = make_case(SPECS[spec_name])
    check_conditions(case)
    loss, batch, trk, out = case_problem(case, dev)
    rs = loss.residuals(batch, trk, out, predicted=True)
    for r in rs:
        shown = masked64(r.residual, r.visible)[0]
        bound = r.residual.numel() * 2.0**-52 * float(shown.sum())
        for name, ours, want in (("pair_sum", r.pair_sum, shown.sum(dim=2)), ("track_sum", r.track_sum, shown.sum(dim=(0, 1)))):
            err = float((ours - want).abs().max())
            print(f"[{spec_name} segment {r.segment}] {name}: max |Δ| to the sum of the returned map {err:.3e} (bound {bound:.3e})", flush=True)
            assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
        assert torch.equal(r.pair_count, r.visible[0].double().sum(dim=2)) and torch.equal(r.track_count, r.visible[0].double().sum(dim=(0, 1)))
        assert abs(float(r.pair_sum.sum()) - float(r.track_sum.sum())) <= bound, "Σ pair_sum != Σ track_sum"
        assert float(r.pair_count.sum()) == float(r.track_count.sum()), "Σ pair_count != Σ track_count"
        assert_close(r.pair_loss(), r.pair_sum / torch.where(r.pair_count == 0, torch.ones_like(r.pair_count), r.pair_count), 1e-15, what="pair_loss")
        assert_close(r.track_loss(), r.track_sum / torch.where(r.track_count == 0, torch.ones_like(r.track_count), r.track_count), 1e-15, what="track_loss")
    for a, b in zip(loss.residuals(batch, trk, out, predicted=True), rs):
        same_fields(a, b, "repeat: ")
    n = len(rs)
    for i in sorted({0, n // 2, n - 1}):
        (one,) = loss.residuals(batch, trk, out, segments=(i, 1), predicted=True)
        same_fields(one, rs[i], f"segments=({i}, 1): ")
        (one,) = loss.residuals(batch, trk, out, segments=i, predicted=True)
        same_fields(one, rs[i], f"segments={i}: ")
        if i + 2 <= n:
            for a, b in zip(loss.residuals(batch, trk, out, segments=slice(i, i + 2), predicted=True), rs[i : i + 2]):
                same_fields(a, b, f"segments=slice({i}, {i + 2}): ")
    (bare,) = loss.residuals(batch, trk, out, segments=(n - 1, 1), sums=False)
    assert bare.xy_target is None and bare.pair_sum is None and bare.pair_count is None and bare.track_sum is None and bare.track_count is None
    assert torch.equal(bare.residual, rs[-1].residual) and torch.equal(bare.visible, rs[-1].visible)
    # no second stage without the sums: the operator hands back empty sum tensors (it allocated no workspace and launched nothing for them)
    packed = _ops.pack_tracks(trk, out.depths.device)
    f, p = packed.shapes[n - 1]
    flat = _ops.torch_ops().track_residuals(out.depths, out.intrinsics, _ops.intrinsics_inverse(out.intrinsics), out.extrinsics, packed.xy, packed.vis, packed.seg,
                                            packed.counts, [f], [p], n - 1, _ops.MAPPING_KINDS[case.spec.kind], DELTA, False, False)
    assert flat[0].numel() == f * f * p and all(x.numel() == 0 for x in flat[2:])
    for method in (bare.pair_loss, bare.track_loss):
        with pytest.raises(RuntimeError, match="needs the sums"):
            method()


# ---- 4: the hot path and the general route --------------------------------------------------------------------------------------------------


def case_hot_path(dev, spec_name):
    from flowmap_amd import _ops
    from flowmap_amd.loss.loss import or_one

    case = make_case(SPECS[spec_name])
    check_conditions(case)
    loss, batch, trk, out = case_problem(case, dev)
    before = _ops.counters["track_residuals"]
    rs = loss.residuals(batch, trk, out, predicted=True)
    assert _ops.counters["track_residuals"] == before + 1
    with tg.recorded() as rec, torch.no_grad():
        fused = loss.compute_unweighted_loss(batch, None, trk, out, 0)
    (_, scale, _), = rec.calls
    total, count = sum(r.pair_sum.sum() for r in rs), sum(r.pair_count.sum() for r in rs)
    print(f"[{spec_name}] Σ pair_sum / Σ pair_count {float(total / or_one(count)):.9e}, the fused loss {float(fused):.9e}; counts {int(count)} / {int(scale[1])}", flush=True)
    assert_close(total / or_one(count), fused.detach().double().reshape(()), 1e-4, what="Σ pair_sum / Σ pair_count vs the fused loss")
    assert int(count) == int(scale[1]), "Σ pair_count differs from the fused pass's count"
    loss_g, batch_g, trk_g, out_g = case_problem(case, dev, lazy=False)
    general = loss_g.residuals(batch_g, trk_g, out_g, predicted=True)
    assert _ops.counters["track_residuals"] == before + 1  # (the general route launches no residual kernel)
    for a, b in zip(rs, general):
        assert (a.segment, a.start_frame) == (b.segment, b.start_frame)
        for name in ("residual", "visible", "xy_target", "pair_sum", "pair_count", "track_sum", "track_count"):
            x, y = getattr(a, name), getattr(b, name)
            assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device, f"lazy vs general: {name}"
            if name == "visible":
                assert torch.equal(x, y), f"segment {a.segment}: visible differs between the fused and the general route ({int((x != y).sum())} elements)"
            elif float(y.double().abs().max()) > 0:
                assert_close(x, y, 1e-4, what=f"lazy vs general, segment {a.segment}: {name}")
    (win,) = loss_g.residuals(batch_g, trk_g, out_g, segments=(len(rs) - 1, 1), sums=False)
    assert win.pair_sum is None and win.xy_target is None and win.segment == len(rs) - 1
    assert_close(win.residual, rs[-1].residual, 1e-4, what="general route, window")


# ---- 5: the camera plane --------------------------------------------------------------------------------------------------------------------

PLANE = Spec("camera-plane", 2, (8, 12), ((0, 2, 6),), seed=51)


@functools.lru_cache(maxsize=None)
def plane_inputs():
    """Two frames, E_0 = I, E_1 = [I | (−0.3, 0, 2·eps)] with eps the fp32 value project_camera_space adds.  Point 0 of frame 0 sits on
    the centre of a pixel whose depth is eps (weights 1, 0, 0, 0: xyz_z = eps exactly); inv(E_1)·E_0 moves it to Z' = eps − 2·eps = −eps
    exactly, so Z' + eps = 0 in fp32 and the element (fs 0, ft 1, p 0) divides by zero (flow_residual_cases.case_edge's construction, with
    a depth that keeps the point's own frame away from the division).  Every access stays in bounds: an input edge."""
    spec = PLANE
    depth, k, e = tg.make_leaves(spec)
    tracks = tg.make_tracks(spec)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    k[0, 1] = k[0, 0]
    e[0] = torch.eye(4)
    e[0, 1, :3, 3] = torch.tensor([-0.3, 0.0, 2 * eps])
    depth[0, 0, 4, 5] = eps
    tracks[0].xy[0, 0, 0] = tg._pixel(5, 4, spec.hw)
    tracks[0].xy[0, 1, 0] = torch.tensor([0.4, 0.5])
    tracks[0].visibility[0, :, 0] = True
    altered, points = tg.apply_margins(spec, (depth, k, e), tracks)
    assert bool(tracks[0].visibility[0, :, 0].all()), "the margin rule cleared the constructed point"
    return (depth, k, e), tracks, altered, points


def case_camera_plane(dev, kind):
    spec = PLANE
    leaves, tracks, altered, points = plane_inputs()
    print(f"[camera-plane] altered {altered} of {points} points", flush=True)
    truth, ref32 = oracle_terms(("plane",), leaves, tracks, spec.hw, kind)
    at = (0, 0, 1, 0)
    assert abs(float(ref32[0]["xy_target"][at].abs().max())) > 1e6, "the fp32 reference does not clamp at the constructed element"
    assert not bool(truth[0]["visible"][at]) and not bool(ref32[0]["visible"][at])
    loss, batch, trk, out = problem(leaves, tracks, spec.hw, dev, kind)
    (r,) = loss.residuals(batch, trk, out, predicted=True)
    assert not bool(r.visible[at])
    for x in (r.residual, r.xy_target, r.pair_sum, r.pair_count, r.track_sum, r.track_count):
        assert bool(torch.isfinite(x).all())
    skip = torch.zeros_like(truth[0]["visible"])
    skip[at] = True
    check_segment(r, truth[0], ref32[0], f"camera-plane/{kind}", skip=skip)
    # at the element: the reference's clamped value — the same handful of fp32 operations on ±1e8 and 0
    print(f"[camera-plane/{kind}] at the element: residual {float(r.residual[at]):.6e} (fp32 reference {float(ref32[0]['residual'][at]):.6e}), "
          f"xy_target {r.xy_target[at].tolist()} (fp32 reference {ref32[0]['xy_target'][at].tolist()})", flush=True)
    assert_close(r.residual[at], ref32[0]["residual"][at], 1e-5, what="the clamped residual vs the fp32 reference")
    assert_close(r.xy_target[at], ref32[0]["xy_target"][at], 1e-5, what="the clamped position vs the fp32 reference")
    # the sums do not see it: they are the sums of the returned map where visible
    shown = masked64(r.residual, r.visible)[0]
    bound = r.residual.numel() * 2.0**-52 * float(shown.sum())
    assert float((r.pair_sum - shown.sum(dim=2)).abs().max()) <= bound and float((r.track_sum - shown.sum(dim=(0, 1))).abs().max()) <= bound
    assert int(r.pair_count.sum()) > 0
    return r


# ---- 6: training is left alone ----------------------------------------------------------------------------------------------------------------


def case_training_untouched(dev, fuse):
    """operator_checks.train, flow + tracking, 5 steps from step 0 after the warm-up, with and without LossTracking.residuals between forward
    and backward (one segment, with the predicted positions) and between the steps: operator_checks.assert_training_untouched with
    ``track_residuals`` the one counter that differs, and the tap exchange ran in both."""
    steps = 5
    mid = lambda ns: ns.track_fn.residuals(ns.batch, ns.tracks, ns.out, segments=(1, 1), predicted=True)  # noqa: E731
    after = lambda ns: ns.track_fn.residuals(ns.batch, ns.tracks, ns.out)  # noqa: E731
    plain = train(dev, tracking=True, fuse=fuse, steps=steps, first_step=0, warm_up=True)
    with_calls = train(dev, tracking=True, fuse=fuse, steps=steps, first_step=0, warm_up=True, calls=(mid, after))
    moved, base = assert_training_untouched(plain, with_calls, "track_residuals", 2 * steps)
    assert plain.state["in_pass"] >= (steps - 3 if fuse else 0)
    assert base["procrustes_plans_built"] == 1 and base["procrustes_planned"] == steps  # (every compared backward went through the plan)
    assert base["flow_tap_passes"] > 0 and moved["flow_tap_passes"] > 0  # the tap exchange really ran, in both runs
    segments = with_calls.state["segments"]
    for i, rs in enumerate(with_calls.seen):
        assert len(rs) == (1 if i % 2 == 0 else segments)
        for r in rs:
            assert bool(torch.isfinite(r.residual).all()) and bool(torch.isfinite(r.pair_sum).all())
    assert with_calls.seen[0][0].segment == 1 and with_calls.seen[0][0].xy_target is not None


# ---- 7: the GPU against the host double -------------------------------------------------------------------------------------------------------


def _inputs_of(which):
    if which in FIXTURE_CASES:
        spec, leaves, tracks = golden_problem(which)
        truth, ref32 = golden_terms(which, spec.kind)
        return spec, leaves, tracks, truth, ref32
    if which == "camera-plane":
        leaves, tracks, _, _ = plane_inputs()
        return (PLANE, leaves, tracks) + oracle_terms(("plane",), leaves, tracks, PLANE.hw, PLANE.kind)
    case = make_case(SPECS[which])
    check_conditions(case)
    return (case.spec, case.leaves, case.tracks) + oracle_terms(case.spec.geometry, case.leaves, case.tracks, case.spec.hw, case.spec.kind)


def case_gpu_against_host_double(dev, which):
    """The same inputs through the HIP kernel and through the serial host build of the same functions, element for element: both pass the
    gate against the fp64 truth, ``visible`` is equal, and the largest ulp distance is printed — bit equality is not required (the device
    contracts multiply-adds the host build, compiled with contraction off, does not; hardware reciprocal and reciprocal square root
    against IEEE division)."""
    from flowmap_amd import _lib
    from helpers import build_host_sim

    spec, leaves, tracks, truth, ref32 = _inputs_of(which)
    loss, batch, trk, out = problem(leaves, tracks, spec.hw, dev, spec.kind)
    gpu = loss.residuals(batch, trk, out, predicted=True)
    _lib.set_library_for_testing(build_host_sim())
    try:
        loss_h, batch_h, trk_h, out_h = problem(leaves, tracks, spec.hw, "cpu", spec.kind)
        host = loss_h.residuals(batch_h, trk_h, out_h, predicted=True)
    finally:
        _lib.set_library_for_testing(None)
    skip = None
    if which == "camera-plane":
        skip = torch.zeros_like(truth[0]["visible"])
        skip[0, 0, 1, 0] = True
    worst = {"residual": 0, "xy_target": 0}
    for i, (a, b) in enumerate(zip(gpu, host)):
        check_segment(a, truth[i], ref32[i], f"gpu {which} segment {i}", skip=skip)
        check_segment(b, truth[i], ref32[i], f"host {which} segment {i}", skip=skip)
        assert torch.equal(a.visible.cpu(), b.visible)
        assert torch.equal(a.pair_count.cpu(), b.pair_count) and torch.equal(a.track_count.cpu(), b.track_count)
        for name in worst:
            worst[name] = max(worst[name], ulp_distance(getattr(a, name).cpu(), getattr(b, name)))
        if skip is not None:  # at the camera-plane element both took the clamped route: the same few operations on ±1e8 and 0
            at = (0, 0, 1, 0)
            assert_close(a.residual.cpu()[at], b.residual[at], 1e-5, what="the clamped residual, GPU vs host double")
            assert_close(a.xy_target.cpu()[at], b.xy_target[at], 1e-5, what="the clamped position, GPU vs host double")
        for name in ("pair_sum", "track_sum"):
            if float(getattr(b, name).abs().max()) > 0:
                assert_close(getattr(a, name).cpu(), getattr(b, name), 1e-4, what=name)
    print(f"[GPU vs host double, {which}] max ulp distance {worst}", flush=True)
    return worst


# ---- 8: arguments ---------------------------------------------------------------------------------------------------------------------------


def case_arguments(dev):
    import pytest

    from flowmap_amd import _ops

    case = make_case(SPECS["mixed"])
    loss, batch, trk, out = case_problem(case, dev)
    n = len(trk)
    for bad in (slice(0, 4, 2), (0, 0), (n - 1, 2), (-1, 2), (0, n + 1), "all", n, -n - 1, (1.0, 2), (0, 1, 2), slice(3, 1), True, 1.5):
        with pytest.raises(ValueError, match="flowmap_amd: LossTracking.residuals"):
            loss.residuals(batch, trk, out, segments=bad)
    assert len(loss.residuals(batch, trk, out, segments=slice(None), sums=False)) == n
    assert [r.segment for r in loss.residuals(batch, trk, out, segments=slice(-2, None), sums=False)] == [n - 2, n - 1]
    assert [r.segment for r in loss.residuals(batch, trk, out, segments=[3, 1], sums=False)] == [3]
    assert [r.segment for r in loss.residuals(batch, trk, out, segments=-1, sums=False)] == [n - 1]
    for none in (None, []):
        with pytest.raises(ValueError, match="flowmap_amd: LossTracking.residuals: there are no tracks"):
            loss.residuals(batch, none, out)

    def changed(**leaf):
        depth, k, e = (leaf.get(name, x) for name, x in zip(("depth", "k", "e"), case.leaves))
        return problem((depth, k, e), case.tracks, case.spec.hw, dev)

    depth, k, e = case.leaves
    with pytest.raises(RuntimeError, match="flowmap_amd: depth must be float32"):
        loss_, batch_, trk_, out_ = changed(depth=depth.double())
        loss_.residuals(batch_, trk_, out_)
    with pytest.raises(RuntimeError, match="flowmap_amd: intrinsics shape does not match"):
        loss_, batch_, trk_, out_ = changed(k=k[:, :-1])
        loss_.residuals(batch_, trk_, out_)
    with pytest.raises(RuntimeError, match="flowmap_amd: .*frame shard"):  # depth holds fewer frames than the poses: a shard
        loss_, batch_, trk_, out_ = changed(depth=depth[:, 2:9].contiguous())
        loss_.residuals(batch_, trk_, out_)
    with pytest.raises(RuntimeError, match="flowmap_amd: a track segment extends past the last frame"):
        loss_, batch_, trk_, out_ = changed(depth=depth[:, :15].contiguous(), k=k[:, :15].contiguous(), e=e[:, :15].contiguous())
        loss_.residuals(batch_, trk_, out_)
    sharded = _ops.PackedTracks(trk, torch.device(dev), own=(2, 9))
    with pytest.raises(RuntimeError, match="flowmap_amd: .*frame shard"):
        _ops.track_residuals(out.depths, out.intrinsics, out.extrinsics, sharded, 0, 1, 0, DELTA, False, True)
    (r,) = loss.residuals(batch, trk, out, segments=0, sums=False)
    with pytest.raises(RuntimeError, match="needs the sums"):
        r.pair_loss()


def case_host_tensor_refused():
    """Host tensors are refused on the fused route and on the general one."""
    spec, leaves, tracks = golden_problem("a")
    for lazy in (True, False):
        def call(lazy=lazy):
            loss, batch, trk, out = problem(leaves, tracks, spec.hw, "cpu", lazy=lazy)
            loss.residuals(batch, trk, out)

        host_tensor_refused(call, "no CPU fallback|needs a GPU")


# ---- 9: the negative control ----------------------------------------------------------------------------------------------------------------


def _visibility_gap(dev, spec, leaves, tracks):
    """Elements whose ``visible`` on ``dev`` differs from the fp64 oracle's on the same (fp32-valued) inputs."""
    depth, k, e = (x.double() for x in leaves)
    surfaces = tg._surfaces(depth, k, spec.hw)
    loss, batch, trk, out = problem(leaves, tracks, spec.hw, dev, spec.kind)
    differ = 0
    for r, seg in zip(loss.residuals(batch, trk, out, sums=False), tracks):
        s, f = seg.start_frame, seg.xy.shape[1]
        _, vis = orc.track_positions(surfaces[:, s : s + f], e[:, s : s + f], k[:, s : s + f], orc.OTracks(seg.xy.double(), seg.visibility, s))
        differ += int((r.visible.cpu() != vis).sum())
    return differ


def case_negative_control(dev, spec_names, built_on="P65"):
    """The exact comparison of ``visible`` is not vacuous.  (a) WITHOUT the margin rule, count the elements of every listed spec whose
    visibility differs from the fp64 oracle's (printed; the random lists happen to hold no target within fp32 rounding of the frame edge).
    (b) Build such a target: in ``built_on`` without the margin rule, take the candidate pair whose target lies nearest the right edge and
    move the principal point of its target frame so that the fp64 target lands on u = 1, then walk c_x a few fp32 neighbours either way —
    the fp64 evaluation steps across the edge at one of them, the fp32 one at another.  There the comparison of case 2 FAILS, and with the
    margin rule applied to the very same inputs it passes again.  -> (found in the lists, differing elements at the built one)."""
    found = {}
    for name in spec_names:
        spec = SPECS[name]
        leaves, tracks = tg.make_leaves(spec), tg.make_tracks(spec)
        if spec.edit:
            tg.EDITS[spec.edit](spec, leaves, tracks)
        found[name] = _visibility_gap(dev, spec, leaves, tracks)
    print(f"[negative control] elements whose visibility differs from the fp64 oracle without the margin rule: {found}", flush=True)

    spec = SPECS[built_on]
    (depth, k, e), tracks = tg.make_leaves(spec), tg.make_tracks(spec)
    seg = tracks[0]
    s, f = seg.start_frame, seg.xy.shape[1]
    surfaces = tg._surfaces(depth.double(), k.double(), spec.hw)
    tgt, _ = orc.track_positions(surfaces[:, s : s + f], e.double()[:, s : s + f], k.double()[:, s : s + f], orc.OTracks(seg.xy.double(), seg.visibility, s))
    src = seg.xy[:, :, None]
    candidate = seg.visibility[:, :, None] & seg.visibility[:, None, :] & (src >= 0).all(-1) & (src < 1).all(-1) & (tgt[..., 1] > 0.1) & (tgt[..., 1] < 0.9)
    candidate &= ~torch.eye(f, dtype=torch.bool)[None, :, :, None]  # (a source's own frame projects it onto itself: no edge to cross)
    gap = torch.where(candidate, (1.0 - tgt[..., 0]).abs(), torch.full_like(tgt[..., 0], 9.0))
    _, fs, ft, p = (int(i) for i in torch.unravel_index(gap.argmin(), gap.shape))
    moved = (k[0, s + ft, 0, 2].double() + (1.0 - tgt[0, fs, ft, p, 0])).float()
    for ulps in range(-8, 9):
        cx = moved.clone()
        for _ in range(abs(ulps)):
            cx = torch.nextafter(cx, torch.tensor(float("inf") if ulps > 0 else float("-inf")))
        k_built = k.clone()
        k_built[0, s + ft, 0, 2] = cx
        differ = _visibility_gap(dev, spec, (depth, k_built, e), tracks)
        if differ:
            break
    print(f"[negative control] {built_on}: target of (fs {fs}, ft {ft}, p {p}) moved onto u = 1 (c_x {ulps:+d} ulp): {differ} elements differ without the margin rule", flush=True)
    kept = [orc.OTracks(x.xy.clone(), x.visibility.clone(), x.start_frame) for x in tracks]
    altered, points = tg.apply_margins(spec, (depth, k_built, e), kept)
    with_rule = _visibility_gap(dev, spec, (depth, k_built, e), kept)
    print(f"[negative control] {built_on}: with the margin rule ({altered} of {points} points altered) {with_rule} elements differ", flush=True)
    return found, differ, with_rule, altered
