"""Step-level and fit-level parity on many seeds and on inputs that are legal for the reference but unlike the two benign
generators (oracle.synth_iid / synth_scene) every other step test draws from.  Shared by the CPU (host double) and GPU modules.

Truth is always the fp64 oracle, ``ref32`` the same oracle in fp32 (what the reference's arithmetic delivers on these inputs);
the gates are helpers.compare_step's, unchanged.  Every case first asserts that the truth is finite, and prints the figures it
is about to assert (``ours vs fp64 / fp32 oracle vs fp64``, norm-wise relative error)."""

from __future__ import annotations

import pytest
import torch

from conftest import assert_close, assert_close_or_reference_gap, relerr
from helpers import compare_step, run_oracle, run_ours, step_masks
from oracle import flowmap_oracle as orc

FOCAL = 0.85
KEYS = ("total", "loss_flow", "loss_tracking", "extrinsics", "g_depth", "g_wlogit", "g_focal")
KINDS = ("huber", "l1", "l2")

# ---- 1. seed sweep, i.i.d. inputs ------------------------------------------------------------------------------------------

SWEEP_SHAPES = ((5, 40, 44, 300), (5, 40, 44, 1000), (3, 64, 96, 600), (8, 32, 48, 300), (5, 40, 44, 64), (5, 40, 44, None))
SWEEP_SEEDS = (0, 1, 2, 3)
SWEEP_FULL_SIZE = ((4, 720, 1280, 1000),)  # GPU only (seeds 0-1): the fp64 oracle takes seconds there


def sweep_configs(shapes=SWEEP_SHAPES, seeds=SWEEP_SEEDS, first=0):
    """(f, h, w, P, kind, seed, lazy): the mapping cycles over huber / l1 / l2 with the seed, offset per shape, so that every
    shape sees each mapping; lazy surfaces alternate with the seed."""
    return [(f, h, w, p, KINDS[(first + si + seed) % 3], seed, seed % 2 == 0) for si, (f, h, w, p) in enumerate(shapes) for seed in seeds]


def sweep_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-P{c[3]}-{c[4]}-s{c[5]}-l{int(c[6])}"


def assert_truth_finite(ref):
    """A regime in which the truth is NaN tests nothing."""
    for key in KEYS:
        assert bool(torch.isfinite(torch.as_tensor(ref[key])).all()), f"fp64 oracle: {key} is not finite"


def report(tag, ours, ref, ref32=None):
    def one(key):
        s = f"{key}={relerr(ours[key], ref[key]):.1e}"
        return s + (f"/{relerr(ref32[key], ref[key]):.1e}" if ref32 is not None else "")

    pairs = range(ref["g_wlogit"].shape[0])
    per_pair = " ".join(f"{relerr(ours['g_wlogit'][i], ref['g_wlogit'][i]):.1e}" + (f"/{relerr(ref32['g_wlogit'][i], ref['g_wlogit'][i]):.1e}" if ref32 is not None else "")
                        for i in pairs)
    print(f"\n[{tag}] total={float(ref['total']):.6g} " + " ".join(one(k) for k in KEYS) + f" g_wlogit per pair: {per_pair}", flush=True)


def run_step(device, tag, depth, wlogit, flows, hw, p, tracks=None, kind="huber", lazy=True, with_ref32=True):
    """One step of ours and of the oracle (fp64, and fp32 when ``with_ref32``), reported; -> (ours, truth, ref32, masks)."""
    args = (depth, wlogit, FOCAL, flows, tuple(hw), p, tracks, kind)
    ref = run_oracle(*args, dtype=torch.float64)
    assert_truth_finite(ref)
    ref32 = run_oracle(*args, dtype=torch.float32) if with_ref32 else None
    ours = run_ours(*args, device=device, lazy=lazy)
    report(tag, ours, ref, ref32)
    return ours, ref, ref32, step_masks(tuple(hw), p, flows, tracks)


def case_seed_sweep(device, cfg):
    f, h, w, p, kind, seed, lazy = cfg
    depth, wlogit, flows = orc.synth_iid(f, h, w, seed=seed)
    ours, ref, ref32, masks = run_step(device, sweep_id(cfg), depth, wlogit, flows, (h, w), p, None, kind, lazy)
    compare_step(ours, ref, ref32, masks=masks)


# ---- 2. the sampled fit on its own, per pair -------------------------------------------------------------------------------

FIT_SHAPES = ((5, 40, 44, 300), (3, 64, 96, 600))


def fit_configs():
    return [(f, h, w, p, seed) for (f, h, w, p) in FIT_SHAPES for seed in SWEEP_SEEDS]


def oracle_relative_fit(depth, wlogit, k, bwd_flow, indices, dtype, weight_sens=100.0):
    """orc.fit_poses up to (not including) the pose chain, from depth and K: leaves (depth, logits, K) and the relative poses
    later -> earlier with their inverses — what _ops.ProcrustesFit.apply returns."""
    d = depth.detach()[None].to(dtype).requires_grad_(True)
    lg = wlogit.detach()[None].to(dtype).requires_grad_(True)
    kk = k.detach().clone().to(dtype).requires_grad_(True)
    _, f, h, w = d.shape
    xy, _ = orc.pixel_grid((h, w), dtype=dtype)
    surfaces = orc.lift(xy, d, kk[:, :, None, None])
    later = surfaces[:, 1:].reshape(1, f - 1, h * w, 3)[:, :, indices]
    where = (xy + bwd_flow.to(dtype)).reshape(1, f - 1, h * w, 2)[:, :, indices]
    earlier = orc.bilinear_border(surfaces[:, :-1], where)
    weights = (weight_sens * lg).sigmoid().reshape(1, f - 1, h * w)[..., indices]
    t_bwd = orc.rigid_fit(later, earlier, weights)
    return d, lg, kk, t_bwd, torch.linalg.inv(t_bwd)


def case_fit_per_pair(device, cfg):
    """_ops.ProcrustesFit as cases.case_procrustes_planned_backward calls it — first call (atomics), third call (planned
    one-launch backward) and the planned backward in three launches — under a seeded random cotangent, against the fp64 oracle
    fit: dL/dlogits PER PAIR (a pair whose gradient is noisy cannot hide under the norm of the stack), dL/ddepth on the pixels
    the fit writes to, dL/dK."""
    from flowmap_amd import _ops
    from flowmap_amd._lib import torch_ops

    f, h, w, points, seed = cfg
    depth, wlogit, of = orc.synth_iid(f, h, w, seed=seed)
    k = orc.focal_to_k(torch.tensor(FOCAL), (h, w)).expand(1, f, 3, 3).contiguous()
    cot = torch.randn((1, f - 1, 4, 4), generator=torch.Generator().manual_seed(seed + 7))
    indices = orc.procrustes_indices((h, w), points)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        d, lg, kk, t_bwd, t_fwd = oracle_relative_fit(depth, wlogit, k, of.backward, indices, dtype)
        ((t_bwd + 0.5 * t_fwd) * cot.to(dtype)).sum().backward()
        refs[dtype] = {"t_bwd": t_bwd.detach(), "g_depth": d.grad[0], "g_logits": lg.grad[0], "g_k": kk.grad[0]}
    truth, ref32 = refs[torch.float64], refs[torch.float32]
    for key, value in truth.items():
        assert bool(torch.isfinite(value).all()), f"fp64 oracle: {key} is not finite"
    touched = orc.procrustes_touched((h, w), indices, of.backward)
    assert int(touched.sum()) > 0

    bwd, idx, cot_d = of.backward.to(device), indices.to(device), cot.to(device)

    def run():
        d = depth[None].to(device).requires_grad_(True)
        lg = wlogit[None].to(device).requires_grad_(True)
        kk = k.clone().to(device).requires_grad_(True)
        # the chained fit (without the extrinsics): only it leaves the records the one-launch backward reads
        t_bwd, t_fwd, _ = _ops.ProcrustesFit.apply_chained(d, kk, None, lg, bwd, idx, 100.0, 1, chain=True, want_extrinsics=False)
        ((t_bwd + 0.5 * t_fwd) * cot_d).sum().backward()
        return {"t_bwd": t_bwd.detach().cpu(), "g_depth": d.grad[0].cpu(), "g_logits": lg.grad[0].cpu(), "g_k": kk.grad[0].cpu()}

    def forms():
        return tuple(_ops.counters[name] for name in ("fit_bwd_one_launch", "fit_bwd_three_launch", "fit_bwd_atomic"))

    before = _ops.counters["procrustes_planned"]
    one, three_, atomic = forms()
    runs = {"atomics": run()}
    assert _ops.counters["procrustes_planned"] == before and forms() == (one, three_, atomic + 1)
    run()  # builds the plan
    runs["planned"] = run()
    assert _ops.counters["procrustes_planned"] == before + 2 and forms() == (one + 2, three_, atomic + 1)
    torch_ops().set_one_launch_backward(False)
    try:
        runs["three-launch"] = run()
    finally:
        torch_ops().set_one_launch_backward(True)
    assert _ops.counters["procrustes_planned"] == before + 3 and forms() == (one + 2, three_ + 1, atomic + 1)  # two different paths

    tag = f"fit {f}x{h}x{w}-P{points}-s{seed}"
    for name, got in runs.items():
        pairs = " ".join(f"{relerr(got['g_logits'][i], truth['g_logits'][i]):.1e}/{relerr(ref32['g_logits'][i], truth['g_logits'][i]):.1e}"
                         for i in range(f - 1))
        print(f"\n[{tag} {name}] t_bwd={relerr(got['t_bwd'], truth['t_bwd']):.1e}/{relerr(ref32['t_bwd'], truth['t_bwd']):.1e}"
              f" g_depth[touched]={relerr(got['g_depth'][touched], truth['g_depth'][touched]):.1e}/{relerr(ref32['g_depth'][touched], truth['g_depth'][touched]):.1e}"
              f" g_k={relerr(got['g_k'], truth['g_k']):.1e}/{relerr(ref32['g_k'], truth['g_k']):.1e} g_logits per pair: {pairs}", flush=True)
    for name, got in runs.items():
        assert_close(got["t_bwd"], truth["t_bwd"], 1e-5, what=f"{name}: t_bwd")
        for i in range(f - 1):
            assert_close_or_reference_gap(got["g_logits"][i], truth["g_logits"][i], ref32["g_logits"][i], 1e-4, what=f"{name}: g_logits[pair {i}]")
        assert_close_or_reference_gap(got["g_logits"], truth["g_logits"], ref32["g_logits"], 1e-4, what=f"{name}: g_logits")
        assert bool((got["g_depth"][~touched] == 0).all()), f"{name}: dL/ddepth written outside the pixels the fit touches"
        assert_close_or_reference_gap(got["g_depth"][touched], truth["g_depth"][touched], ref32["g_depth"][touched], 1e-4, what=f"{name}: g_depth[touched]")
        assert_close_or_reference_gap(got["g_k"], truth["g_k"], ref32["g_k"], 1e-4, what=f"{name}: g_k")


# ---- 3. degenerate but legal inputs ----------------------------------------------------------------------------------------

REGIMES = ("pair_masked", "all_masked", "binary_masks", "saturated_weights", "big_flows", "iid_tracks", "tracks_on_pixel_centres")
REGIME_SHAPES = ((4, 24, 36, 64, "huber"), (3, 17, 13, None, "l1"), (5, 40, 44, 300, "l2"))
TINY_FRAMES = ((2, 1, 4, None), (3, 1, 8, None), (3, 4, 1, None), (3, 2, 2, None), (2, 3, 3, 3))
DEPTH_SCALES = (0.05, 1.0, 40.0)


def regime(name, f, h, w, seed):
    """-> (depth, weight logits, flows, tracks or None): synth_iid with one property pushed to its edge."""
    depth, wlogit, flows = orc.synth_iid(f, h, w, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    tracks = None
    if name == "pair_masked":  # one pair contributes nothing to the loss (its pose is still fitted and chained)
        flows.forward_mask[:, 0] = 0
        flows.backward_mask[:, 0] = 0
    elif name == "all_masked":  # valid_sum == 0 -> `or 1`
        flows.forward_mask.zero_()
        flows.backward_mask.zero_()
    elif name == "binary_masks":
        flows.forward_mask = (flows.forward_mask > 0.5).float()
        flows.backward_mask = (flows.backward_mask > 0.7).float()
    elif name == "saturated_weights":  # x100 sensitivity: sigmoid saturates to 0 / 1 in fp32
        wlogit = 0.2 * torch.randn(wlogit.shape, generator=g)
    elif name == "big_flows":  # most Procrustes samples clamp to the border
        flows.forward = 0.3 * torch.randn(flows.forward.shape, generator=g)
        flows.backward = 0.3 * torch.randn(flows.backward.shape, generator=g)
    elif name in ("iid_tracks", "tracks_on_pixel_centres"):
        tracks = orc.synth_tracks(f, h, w, scene=None, seed=seed, interval=2, radius=3, grid=6)
        if name == "tracks_on_pixel_centres":  # bilinear weights exactly (1, 0, 0, 0)
            for t in tracks:
                t.xy[..., 0] = ((t.xy[..., 0] * w).floor() + 0.5) / w
                t.xy[..., 1] = ((t.xy[..., 1] * h).floor() + 0.5) / h
    elif name != "plain":
        raise KeyError(name)
    return depth, wlogit, flows, tracks


def regime_configs():
    return [(name, *shape) for name in REGIMES for shape in REGIME_SHAPES]


def case_regime(device, cfg, seed=0):
    name, f, h, w, p, kind = cfg
    depth, wlogit, flows, tracks = regime(name, f, h, w, seed)
    ours, ref, ref32, masks = run_step(device, f"{name} {f}x{h}x{w}-P{p}-{kind}", depth, wlogit, flows, (h, w), p, tracks, kind)
    compare_step(ours, ref, ref32, masks=masks)
    if name == "all_masked":  # nothing is valid: the loss and every gradient are exactly zero, the poses are still the fit's
        for key in ("total", "loss_flow", "g_depth", "g_wlogit", "g_focal"):
            assert torch.equal(ours[key].float(), torch.zeros_like(ours[key].float())), f"{key} is not exactly zero"


def case_tiny_frame(device, cfg, seed=0):
    f, h, w, p = cfg
    depth, wlogit, flows, tracks = regime("plain", f, h, w, seed)
    ours, ref, ref32, masks = run_step(device, f"tiny {f}x{h}x{w}-P{p}", depth, wlogit, flows, (h, w), p, tracks, "huber")
    compare_step(ours, ref, ref32, masks=masks)


def case_scaled_scene(device, scale):
    """A consistent scene with its depth scaled: held to the fp64 oracle ON THE SAME scaled input at the plain 1e-4 (the
    reference's own maths is not invariant under the scale, so invariance of the loss is not what is asserted)."""
    f, h, w, p = 6, 32, 48, 200
    sc = orc.synth_scene(f, h, w, seed=3, depth_noise=0.03)
    tracks = orc.synth_tracks(f, h, w, scene=sc, seed=3, interval=2, radius=2, grid=6)
    ours, ref, _, masks = run_step(device, f"scene depth x{scale}", sc["depth_init"] * scale, torch.zeros((f - 1, h, w)), sc["flows"], (h, w), p, tracks,
                                   "huber", with_ref32=False)
    assert float(ref["loss_tracking"]) > 0
    compare_step(ours, ref, None, masks=masks)


def case_two_frames_with_tracks(device):
    f, h, w, p = 2, 24, 32, 100
    sc = orc.synth_scene(f, h, w, seed=5, depth_noise=0.03)
    tracks = orc.synth_tracks(f, h, w, scene=sc, seed=5, interval=1, radius=1, grid=5)
    ours, ref, _, masks = run_step(device, "two frames with tracks", sc["depth_init"], torch.zeros((1, h, w)), sc["flows"], (h, w), p, tracks, "huber",
                                   with_ref32=False)
    assert float(ref["loss_tracking"]) > 0
    compare_step(ours, ref, None, masks=masks)


def case_nothing_visible(device):
    """Tracks without one visible point: the tracking loss is exactly zero and the step is the step without tracks."""
    f, h, w, p = 5, 24, 32, 100
    sc = orc.synth_scene(f, h, w, seed=5, depth_noise=0.03)
    tracks = orc.synth_tracks(f, h, w, scene=sc, seed=5, interval=2, radius=2, grid=5)
    for t in tracks:
        t.visibility[:] = False
    wlogit = torch.zeros((f - 1, h, w))
    ours, ref, _, _ = run_step(device, "nothing visible", sc["depth_init"], wlogit, sc["flows"], (h, w), p, tracks, "huber", with_ref32=False)
    assert float(ref["loss_tracking"]) == 0.0
    compare_step(ours, ref, None, masks=step_masks((h, w), p, sc["flows"]))
    assert float(ours["loss_tracking"]) == 0.0
    plain = run_ours(sc["depth_init"], wlogit, FOCAL, sc["flows"], (h, w), p, None, "huber", device=device)
    for key in ("total", "g_depth", "g_wlogit", "g_focal", "extrinsics"):
        print(f"[nothing visible] {key} vs the step without tracks: {relerr(ours[key], plain[key]):.1e}", flush=True)
        assert_close(ours[key], plain[key], 1e-6, what=f"{key} vs the step without tracks")


# ---- 4. a tracking loss that is zero in exact arithmetic -------------------------------------------------------------------


def compare_step_near_zero_tracking(ours, truth, ref32, masks=None):
    """compare_step for a step whose tracking loss is zero in exact arithmetic and rounding noise in any other (segments of one
    frame: every point is compared with itself): ``loss_tracking`` and ``total`` are held to the truth at 1e-4 or twice the fp32 reference's own gap
    (conftest.assert_close_or_reference_gap) — a relative gate on a value that is zero but for rounding means nothing — and
    everything else goes through compare_step as it stands, on a copy whose two loss values are the ones just checked."""
    for key in ("loss_tracking", "total"):
        assert_close_or_reference_gap(ours[key], truth[key], ref32[key], 1e-4, what=key)
    checked = dict(ours)
    checked["loss_tracking"], checked["total"] = truth["loss_tracking"], truth["total"]
    compare_step(checked, truth, None, masks=masks)


def case_one_frame_segments(device):
    """Measured, relative to a loss_tracking of 5.5e-5 (absolute errors of 2e-9 .. 1e-8): ours 3.2e-5 on the host double and
    1.4e-4 on the GPU, the fp32 oracle 1.3e-4 .. 1.9e-4 depending on the host's reduction order."""
    f, h, w, p = 5, 24, 32, 100
    sc = orc.synth_scene(f, h, w, seed=5, depth_noise=0.03)
    tracks = orc.synth_tracks(f, h, w, scene=sc, seed=5, interval=2, radius=0, grid=5)
    assert all(t.xy.shape[1] == 1 for t in tracks)
    ours, ref, ref32, masks = run_step(device, "one-frame segments", sc["depth_init"], torch.zeros((f - 1, h, w)), sc["flows"], (h, w), p, tracks, "huber")
    print(f"[one-frame segments] loss_tracking ours {float(ours['loss_tracking']):.3e} fp64 {float(ref['loss_tracking']):.3e} fp32 {float(ref32['loss_tracking']):.3e}")
    # every point is reprojected into its own frame: off its track only by the fp32 rounding of the stored coordinates
    assert abs(float(ref["loss_tracking"])) < 1e-4 * abs(float(ref["loss_flow"]))
    compare_step_near_zero_tracking(ours, ref, ref32, masks=masks)


# ---- 5. few points ---------------------------------------------------------------------------------------------------------

FEW_POINTS_SHAPE = (4, 16, 16)


def case_few_points(device, p):
    """P = 3, 4: the smallest index sets that determine a rigid transformation."""
    f, h, w = FEW_POINTS_SHAPE
    depth, wlogit, flows, _ = regime("plain", f, h, w, 0)
    ours, ref, ref32, masks = run_step(device, f"few points P{p}", depth, wlogit, flows, (h, w), p, None, "huber")
    compare_step(ours, ref, ref32, masks=masks)


def case_too_few_points(device, p):
    """P = 1, 2: the centred cloud has rank <= 1, so the rotation is not determined by the data (free about the line through
    the two points; entirely free for one point) — the reference returns whatever its SVD picks in the null space and dL/dM
    carries a factor 1/(sigma_2 + sigma_3) = 1/0 (numerics).  flowmap_amd refuses such a fit by name, from Python,
    before anything is launched, on every device alike."""
    f, h, w = FEW_POINTS_SHAPE
    depth, wlogit, flows, _ = regime("plain", f, h, w, 0)
    with pytest.raises(ValueError, match="num_points") as err:
        run_ours(depth, wlogit, FOCAL, flows, (h, w), p, None, "huber", device=device)
    assert "HIP launch/runtime failure" not in str(err.value)
    # ... and the fit called directly with such an index set
    from flowmap_amd import _ops

    k = orc.focal_to_k(torch.tensor(FOCAL), (h, w)).expand(1, f, 3, 3).contiguous().to(device)
    with pytest.raises(ValueError, match="num_points"):
        _ops.ProcrustesFit.apply(depth[None].to(device), k, None, wlogit[None].to(device), flows.backward.to(device),
                                 orc.procrustes_indices((h, w), p).to(device), 100.0, 1)
