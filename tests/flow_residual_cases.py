"""LossFlow.residuals (fm_flow_residuals): the per-pixel flow terms, the pose-induced flows and the per-pair sums straight from depth.
The cases here take a device; tests/test_hostsim_flow_residuals.py runs them on the serial host double of the C ABI,
tests/test_gpu_flow_residuals.py on the MI355X.

Truths.  tests/golden/fn_flow_residuals.npz holds what the REFERENCE computes (tools/make_golden_flow_residuals.py) in fp32 and in fp64
for the small shapes and the clamping edge case; for the shapes too large to commit per-pixel fp64 maps of (several workgroups per pair,
workgroup tails) the same two evaluations come from the oracle (oracle/flowmap_oracle.py: the reference's arithmetic restated), computed
once per shape.  Either way the gate is the project's: conftest.assert_close_or_reference_gap, rel 1e-4, slack 2x the fp32 evaluation's
own gap to fp64.

Shapes (frames x h x w): 2x5x7 (one pair, less than a wavefront, scalar path), 5x17x23 (odd everything), 6x24x32 (the golden step size,
16-byte path), 4x64x128 (four workgroups per pair: the ordered second stage adds real partials), 2x27x76 and 2x7x292 (2052 and 2044
pixels: one quad more / fewer than a whole 2048-pixel workgroup tile, 16-byte path), and two batch entries read through fm_layout strides.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

from conftest import assert_close, assert_close_or_reference_gap, load_golden, t
from helpers import mapping_cfg
from operator_checks import FRAMES, HEIGHT, WIDTH, assert_training_untouched, host_tensor_refused, same_tensors, train, ulp_distance
from oracle import flowmap_oracle as orc

KINDS = ("huber", "l1", "l2")
INPUT_KEYS = ("depth", "k", "extrinsics", "fwd", "bwd", "fwd_mask", "bwd_mask")
CLAMPED = 1e6  # |xy_flowed − xy| above this: the ±1e8 of project_camera_space
TILE = 2048  # pixels per workgroup (fm_flow_residuals.hip: kResTile)


# ---- inputs (tools/make_golden_flow_residuals.py draws the fixture's from the same functions) ----------------------------------------


def small_poses(g, b, f, degrees=3.0, shift=0.05):
    """(b, f, 4, 4) camera-to-world chains of per-pair rotations of a few degrees and translations N(0, shift)."""
    ext = torch.eye(4, dtype=torch.float64).repeat(b, f, 1, 1)
    for i in range(b):
        for j in range(1, f):
            a = torch.randn(3, generator=g, dtype=torch.float64)
            a = a / a.norm() * np.deg2rad(degrees) * (0.5 + torch.rand((), generator=g, dtype=torch.float64))
            kx = torch.zeros((3, 3), dtype=torch.float64)
            kx[0, 1], kx[0, 2], kx[1, 0], kx[1, 2], kx[2, 0], kx[2, 1] = -a[2], a[1], a[2], -a[0], -a[1], a[0]
            rel = torch.eye(4, dtype=torch.float64)
            rel[:3, :3] = torch.linalg.matrix_exp(kx)
            rel[:3, 3] = shift * torch.randn(3, generator=g, dtype=torch.float64)
            ext[i, j] = ext[i, j - 1] @ rel
    return ext.float()


def intrinsics(g, b, f, per_frame):
    k = torch.eye(3).repeat(b, f, 1, 1)
    if per_frame:
        k[..., 0, 0] = 0.8 + 0.3 * torch.rand((b, f), generator=g)
        k[..., 1, 1] = 0.9 + 0.3 * torch.rand((b, f), generator=g)
        k[..., 0, 2] = 0.5 + 0.05 * torch.randn((b, f), generator=g)
        k[..., 1, 2] = 0.5 + 0.05 * torch.randn((b, f), generator=g)
    else:  # what IntrinsicsRegressed hands out: one K for every frame, the principal point in the centre
        k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2] = 0.85, 1.1, 0.5, 0.5
    return k


def inputs(seed, b, f, h, w, per_frame_k):
    """Well conditioned: depth in [0.5, 2], rotations of a few degrees; flows N(0, 0.02) (residuals on both sides of Huber's knee 0.01);
    continuous mask weights in [0, 1), a quarter of them zero."""
    g = torch.Generator().manual_seed(seed)
    mask = lambda: torch.rand((b, f - 1, h, w), generator=g) * (torch.rand((b, f - 1, h, w), generator=g) > 0.25)  # noqa: E731
    return {
        "depth": 0.5 + 1.5 * torch.rand((b, f, h, w), generator=g),
        "k": intrinsics(g, b, f, per_frame_k),
        "extrinsics": small_poses(g, b, f),
        "fwd": 0.02 * torch.randn((b, f - 1, h, w, 2), generator=g),
        "bwd": 0.02 * torch.randn((b, f - 1, h, w, 2), generator=g),
        "fwd_mask": mask(),
        "bwd_mask": mask(),
    }


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("fn_flow_residuals")


def golden_inputs(case):
    return {key: t(golden()[f"{case}_{key}"]) for key in INPUT_KEYS}


@functools.lru_cache(maxsize=None)
def oracle_case(b, f, h, w, per_frame_k):
    """(inputs, {dtype: terms}) of a shape the fixture does not hold: the oracle's fp32 and fp64 evaluation of loss_flow.py:46-68, once."""
    x = inputs(1000 + f * h * w, b, f, h, w, per_frame_k)
    terms = {}
    for dtype in (torch.float32, torch.float64):
        depth, k, ext = (x[n].to(dtype) for n in ("depth", "k", "extrinsics"))
        xy, _ = orc.pixel_grid((h, w), dtype=dtype)
        surfaces = orc.lift(xy, depth, k[:, :, None, None])
        out = {"pred_forward": orc.forward_flow_positions(surfaces, ext, k) - xy, "pred_backward": orc.backward_flow_positions(surfaces, ext, k) - xy}
        for kind in KINDS:
            out[f"{kind}_forward"] = orc.robust(out["pred_forward"], x["fwd"].to(dtype), (h, w), kind, 0.01)
            out[f"{kind}_backward"] = orc.robust(out["pred_backward"], x["bwd"].to(dtype), (h, w), kind, 0.01)
        terms[dtype] = out
    return x, terms


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------


def problem(x, dev, kind="huber", lazy=True):
    """(loss, batch, flows, model_output) over the inputs ``x``: lazy surfaces of the output's own depths (the fused route) or the
    explicit (b, f, h, w, 3) tensor (the general route)."""
    from flowmap_amd import Batch, Flows, ModelOutput
    from flowmap_amd.loss import LossFlow, LossFlowCfg
    from flowmap_amd.model.projection import LazySurfaces

    x = {key: v.to(dev) for key, v in x.items()}
    b, f, h, w = x["depth"].shape
    surfaces = LazySurfaces(x["depth"], x["k"])
    if not lazy:
        surfaces = surfaces.materialize()
    out = ModelOutput(x["depth"], surfaces, x["k"], x["extrinsics"], None)
    flows = Flows(x["fwd"], x["bwd"], x["fwd_mask"], x["bwd_mask"])
    return LossFlow(LossFlowCfg(0, 1.0, "flow", mapping_cfg(kind))), Batch(torch.zeros((b, f, 3, h, w), device=dev)), flows, out


def check_maps(r, truth, ref32, kind, what, where=None):
    """Check 1 on the four maps of a FlowResiduals: ``truth`` / ``ref32`` map names -> arrays (fp64 / fp32 evaluation of the reference);
    ``where``: (forward, backward) boolean pixel masks to restrict the comparison to."""
    worst = 0.0
    for ours, name in ((r.forward, f"{kind}_forward"), (r.backward, f"{kind}_backward"), (r.forward_flow, "pred_forward"), (r.backward_flow, "pred_backward")):
        a, tr, rf = ours.cpu(), torch.as_tensor(truth[name]), torch.as_tensor(ref32[name])
        if where is not None:
            sel = where[0] if name.endswith("forward") else where[1]
            a, tr, rf = a[sel], tr[sel], rf[sel]
        e, gap = assert_close_or_reference_gap(a, tr, rf, rel=1e-4, slack=2.0, what=f"{what}.{name}")
        print(f"  {what}.{name}: rel err {e:.2e} (fp32 reference's own gap {gap:.2e})")
        worst = max(worst, e)
    return worst


FIELDS = ("forward", "backward", "forward_flow", "backward_flow", "pair_sum", "pair_valid")
def same_fields(a, b, what="", **kw):
    same_tensors(a, b, FIELDS, what, **kw)


# ---- check 1: reference parity, per pixel ------------------------------------------------------------------------------------------------


def case_reference_parity(dev, case, kind):
    """The fixture's general cases — a: shared K, 2x5x7; b: a K per frame with cx, cy != 0.5, 5x17x23; c: two batch entries, 4x9x12 —
    against the reference's fp64 run."""
    g = golden()
    loss, batch, flows, out = problem(golden_inputs(case), dev, kind)
    r = loss.residuals(batch, flows, out, predicted_flow=True)
    b, f, h, w = out.depths.shape
    assert r.forward.shape == (b, f - 1, h, w) and r.forward_flow.shape == (b, f - 1, h, w, 2) and r.pair_sum.shape == (b, f - 1, 2) and r.first_pair == 0
    assert r.forward.dtype == torch.float32 and r.pair_sum.dtype == torch.float64 and not r.forward.requires_grad
    check_maps(r, {k[len(case) + 5:]: v for k, v in g.items() if k.startswith(f"{case}_f64_")},
               {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(f"{case}_")}, kind, case)


def case_oracle_parity(dev, shape, kind):
    """The shapes with several workgroups per pair and with workgroup tails, against the oracle's fp64 evaluation."""
    x, terms = oracle_case(*shape)
    loss, batch, flows, out = problem(x, dev, kind)
    r = loss.residuals(batch, flows, out, predicted_flow=True)
    check_maps(r, terms[torch.float64], terms[torch.float32], kind, "x".join(map(str, shape[1:4])))


def case_edge(dev, kind):
    """The fixture's edge case: a band of pair 0 lands on Z' = −1e-5 exactly and project_camera_space clamps (±1e8, NaN -> 0); the upper rows
    of pair 1 land behind the camera.  The SET of clamped pixels equals the reference's; the values there and elsewhere pass the gate.
    (The fp64 run of the reference does not clamp — its Z' + 1e-5 is 2.5e-13, not 0 — so at the clamped pixels the gate's reference-gap
    term is of order one; there the maps must also agree with the reference's fp32 values to 1e-5: both apply the same handful of fp32
    operations to ±1e8 and 0.)"""
    g = golden()
    loss, batch, flows, out = problem(golden_inputs("edge"), dev, kind)
    r = loss.residuals(batch, flows, out, predicted_flow=True)
    truth = {k[len("edge_f64_"):]: v for k, v in g.items() if k.startswith("edge_f64_")}
    ref32 = {k[len("edge_"):]: v for k, v in g.items() if k.startswith("edge_")}
    ours_clamped = [(p.cpu().abs() > CLAMPED).any(-1) for p in (r.forward_flow, r.backward_flow)]
    ref_clamped = [(torch.as_tensor(ref32[f"pred_{d}"]).abs() > CLAMPED).any(-1) for d in ("forward", "backward")]
    assert int(ref_clamped[0].sum()) == 36 and int(ref_clamped[1].sum()) == 0
    for ours, ref, d in zip(ours_clamped, ref_clamped, ("forward", "backward")):
        assert torch.equal(ours, ref), f"{d}: clamped pixels differ from the reference's ({int(ours.sum())} vs {int(ref.sum())})"
    for m in (r.forward, r.backward, r.forward_flow, r.backward_flow):
        assert bool(torch.isfinite(m).all())
    check_maps(r, truth, ref32, kind, "edge[clamped]", where=(ref_clamped[0], ref_clamped[0]))  # (the backward maps on the same pixels: nothing clamps there)
    check_maps(r, truth, ref32, kind, "edge[elsewhere]", where=(~ref_clamped[0], ~ref_clamped[1]))
    sel = ref_clamped[0]
    assert_close(r.forward.cpu()[sel], torch.as_tensor(ref32[f"{kind}_forward"])[sel], 1e-5, what="clamped residuals vs the fp32 reference")
    assert_close(r.forward_flow.cpu()[sel], torch.as_tensor(ref32["pred_forward"])[sel], 1e-5, what="clamped flows vs the fp32 reference")


# ---- check 2: the sums --------------------------------------------------------------------------------------------------------------------


def case_sums(dev, shape, kind="huber"):
    """pair_sum / pair_valid against the fp64 sums of the RETURNED fp32 maps times the masks — the terms are the fp32 products the kernel
    converts, (double)(residual·mask), so the only difference is the order of the fp64 additions: |Δ| <= n · 2^-52 · Σ|terms|, n the pixels
    per pair.  Three calls bit-equal; a window bit-equal, maps and sums, to the same pairs of the full call."""
    x, _ = oracle_case(*shape)
    loss, batch, flows, out = problem(x, dev, kind)
    r = loss.residuals(batch, flows, out, predicted_flow=True)
    b, f, h, w = out.depths.shape
    n = h * w
    for d, (res, mask) in enumerate(((r.forward, flows.forward_mask), (r.backward, flows.backward_mask))):
        terms = (res * mask).double()  # fp32 products, then exact
        want, mag = terms.sum(dim=(2, 3)), terms.abs().sum(dim=(2, 3))
        err = (r.pair_sum[..., d] - want).abs()
        assert bool((err <= n * 2.0**-52 * mag).all()), f"pair_sum[{d}]: worst {float((err / mag.clamp_min(1e-300)).max()):.3e} relative, bound {n * 2.0**-52:.3e}"
        want_valid = mask.double().sum(dim=(2, 3))
        err = (r.pair_valid[..., d] - want_valid).abs()
        assert bool((err <= n * 2.0**-52 * want_valid).all()), f"pair_valid[{d}]"
        assert float(want.min()) > 0 and float(want_valid.min()) > 0
    assert_close(r.pair_loss(), r.pair_sum / r.pair_valid, 1e-15, what="pair_loss")
    for _ in range(2):
        same_fields(loss.residuals(batch, flows, out, predicted_flow=True), r, "repeat: ")
    if f - 1 >= 3:
        win = loss.residuals(batch, flows, out, pairs=(1, 2), predicted_flow=True)
        assert win.first_pair == 1 and win.forward.shape == (b, 2, h, w) and win.pair_sum.shape == (b, 2, 2)
        part = type(r)(*(None if v is None else v[:, 1:3] for v in (r.forward, r.backward, r.forward_flow, r.backward_flow, r.pair_sum, r.pair_valid)), 1)
        same_fields(win, part, "window (1, 2): ")
        same_fields(loss.residuals(batch, flows, out, pairs=slice(1, 3), predicted_flow=True), win, "slice(1, 3): ")
    bare = loss.residuals(batch, flows, out, sums=False)  # what was not asked for is not produced
    assert bare.pair_sum is None and bare.pair_valid is None and bare.forward_flow is None and bare.backward_flow is None
    assert torch.equal(bare.forward, r.forward) and torch.equal(bare.backward, r.backward)


# ---- check 3: agreement with the hot path --------------------------------------------------------------------------------------------------


def case_hot_path(dev, shape, kind):
    """Σ pair_sum / Σ pair_valid is the fused loss (the same device function per pixel), and the lazy route gives what the general route
    (explicit surfaces: reproject -> mapping, each a kernel of its own) gives: rel 1e-4."""
    from flowmap_amd import _ops
    from flowmap_amd.loss.loss import or_one

    x, _ = oracle_case(*shape)
    loss, batch, flows, out = problem(x, dev, kind)
    before = _ops.counters["flow_residuals"]
    r = loss.residuals(batch, flows, out, predicted_flow=True)
    assert _ops.counters["flow_residuals"] == before + 1
    fused = loss.compute_unweighted_loss(batch, flows, None, out, 0)
    assert_close(r.pair_sum.sum() / or_one(r.pair_valid.sum()), fused.detach().double(), 1e-4, what="Σ pair_sum / Σ pair_valid vs the fused loss")
    loss_g, batch_g, flows_g, out_g = problem(x, dev, kind, lazy=False)
    general = loss_g.residuals(batch_g, flows_g, out_g, predicted_flow=True)
    assert _ops.counters["flow_residuals"] == before + 1  # (the general route launches no residual kernel)
    for name in ("forward", "backward", "forward_flow", "backward_flow", "pair_sum", "pair_valid"):
        assert getattr(general, name).shape == getattr(r, name).shape and getattr(general, name).dtype == getattr(r, name).dtype, name
        assert_close(getattr(r, name), getattr(general, name), 1e-4, what=f"lazy vs general: {name}")
    win = loss_g.residuals(batch_g, flows_g, out_g, pairs=(0, 1), sums=False)
    assert win.pair_sum is None and win.forward_flow is None
    assert_close(win.forward, r.forward[:, :1], 1e-4, what="general route, window")


# ---- frame windows and batch slices read in place ------------------------------------------------------------------------------------------


def case_views(dev, hw):
    """Two batch entries.  Depth (and once every image stack) handed over as a frame window x[:, 1:5] of a larger tensor and as a batch
    slice x[::2] (fm_layout strides), against the same data made contiguous: bit-equal, and nothing was copied."""
    from flowmap_amd._lib import torch_ops

    h, w = hw
    b, f = 2, 4
    x = {key: v.to(dev) for key, v in (golden_inputs("c") if hw == (9, 12) else inputs(77, b, f, h, w, True)).items()}
    loss, batch, flows, out = problem(x, dev)
    want = loss.residuals(batch, flows, out, predicted_flow=True)

    def embed(v, how):
        if how == "frames":  # x[:, 1:1+frames] of a tensor with three more frames
            big = torch.full((b, v.shape[1] + 3, *v.shape[2:]), 7.0, device=dev)
            big[:, 1:1 + v.shape[1]] = v
            return big[:, 1:1 + v.shape[1]]
        big = torch.full((2 * b, *v.shape[1:]), 7.0, device=dev)  # x[::2] of a tensor with twice the batch entries
        big[::2] = v
        return big[::2]

    copies = torch_ops().view_copies()
    for how in ("frames", "batch"):
        for which in (("depth",), ("depth", "fwd", "bwd", "fwd_mask", "bwd_mask")):
            y = {key: embed(v, how) if key in which else v for key, v in x.items()}
            assert not y["depth"].is_contiguous()
            loss_v, batch_v, flows_v, out_v = problem(y, dev)
            assert out_v.depths is y["depth"]
            same_fields(loss_v.residuals(batch_v, flows_v, out_v, predicted_flow=True), want, f"{how} view of {which}: ")
            if how == "frames":
                win = loss_v.residuals(batch_v, flows_v, out_v, pairs=(1, 2))
                assert torch.equal(win.forward, want.forward[:, 1:3]) and torch.equal(win.pair_sum, want.pair_sum[:, 1:3])
    assert torch_ops().view_copies() == copies, "a frame window was copied instead of read in place"


# ---- check 4: it leaves training alone ------------------------------------------------------------------------------------------------------


def _train(dev, tracking, calls, fuse, steps=5):
    """operator_checks.train, 5 steps from step 0 without a warm-up; ``calls``: LossFlow.residuals between forward and backward (a window,
    with the predicted flows) and again between the steps.  -> (the record, the PoseChain evaluations of the run and whether the fit
    was asked for chained poses: ``_fm_extrinsics_wanted`` on the backward flows).

    No step is discarded here, so step 0 holds the FIRST backward, which is compared bit for bit like every other.  The sparse fit's scatter
    plan is built when the same (indices, flows) are seen a second time, and without it fm_procrustes_scatter adds into dL/ddepth with float
    atomics whose order differs between two runs ("Determinism": this case failed on the GPU at step 0, dL/ddepth off by
    1.5e-8 .. 1.2e-7, in 15 to 17 of 80 pairs of runs).  Where dL/ddepth is compared (not ``fuse``) ``prepare`` therefore shows the plan
    the fit's (indices, flows) once before step 0, in both runs: nothing is launched, and the first fit is their second sighting.  With
    ``fuse`` the plan must not exist before every consumer of depth has run once (_ops.note_touched), dL/ddepth is compared through the
    parameter it moved, and the first step stays as it was."""
    from flowmap_amd import _ops
    from flowmap_amd.model.extrinsics_procrustes import procrustes_indices

    chain_calls = [0]
    chain = _ops.PoseChain.apply

    def counted_chain(rel):
        chain_calls[0] += 1
        return chain(rel)

    mid = lambda ns: ns.flow_fn.residuals(ns.batch, ns.flows, ns.out, pairs=(1, 2), predicted_flow=True)  # noqa: E731
    after = lambda ns: ns.flow_fn.residuals(ns.batch, ns.flows, ns.out)  # noqa: E731
    flows = []

    def prepare(ns):
        flows.append(ns.flows)
        if fuse:
            return
        own = procrustes_indices(HEIGHT, WIDTH, ns.model.extrinsics.cfg.num_points, False, torch.device(dev))
        assert _ops._procrustes_scatter_plan(own, ns.flows.backward, 1, FRAMES, HEIGHT, WIDTH) is None  # (first sighting: noted, not built)

    _ops.PoseChain.apply = staticmethod(counted_chain)
    try:
        run = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=0, warm_up=False, calls=(mid, after) if calls else None, prepare=prepare)
    finally:
        _ops.PoseChain.apply = staticmethod(chain)
    return run, {"wanted": bool(flows[0].backward.__dict__.get("_fm_extrinsics_wanted", False)), "chain_calls": chain_calls[0]}


def case_training_untouched(dev, tracking, fuse):
    """A flow (+ tracking, tap exchange on) run with FusedAdam (``fuse``: FusedAdam.fuse_depth_update), with and without residuals() between
    forward and backward and between the steps: operator_checks.assert_training_untouched with exactly one residual launch per call, and no
    pose chain was evaluated for the calls and nothing was noted on the flow tensor."""
    steps = 5
    plain, chained = _train(dev, tracking, calls=False, fuse=fuse, steps=steps)
    with_calls, chained_with_calls = _train(dev, tracking, calls=True, fuse=fuse, steps=steps)
    _, base = assert_training_untouched(plain, with_calls, "flow_residuals", 2 * steps)
    assert chained_with_calls == chained, (chained_with_calls, chained)
    assert plain.state["in_pass"] >= (steps - 3 if fuse else 0)  # the update inside the pass really ran (and as often with the calls: state is equal)
    assert base["procrustes_plans_built"] == 1 and base["procrustes_planned"] == (steps - 1 if fuse else steps)  # (not fuse: every compared backward went through the plan)
    if tracking:
        assert base["flow_tap_passes"] > 0  # the tap exchange really ran
    else:
        assert chained["chain_calls"] == 0 and not chained["wanted"]  # a flow-only run never chains the poses, with the calls neither
    # what the calls returned is the view of the step they were made in: finite, and the windowed one equals that step's full one
    for r in with_calls.seen:
        assert bool(torch.isfinite(r.forward).all()) and bool(torch.isfinite(r.pair_sum).all())
    assert with_calls.seen[0].first_pair == 1 and with_calls.seen[0].forward.shape[1] == 2 and with_calls.seen[1].forward.shape[1] == 4


# ---- check 5: arguments ---------------------------------------------------------------------------------------------------------------------


def case_arguments(dev):
    import pytest

    x = {key: v.to(dev) for key, v in golden_inputs("b").items()}
    loss, batch, flows, out = problem(x, dev)
    for bad in (slice(0, 4, 2), (0, 0), (3, 2), (-1, 2), (0, 5), "all", 1, (1.0, 2), (0, 1, 2), slice(3, 1)):
        with pytest.raises(ValueError, match="flowmap_amd: LossFlow.residuals"):
            loss.residuals(batch, flows, out, pairs=bad)
    assert loss.residuals(batch, flows, out, pairs=slice(None)).forward.shape[1] == 4
    assert loss.residuals(batch, flows, out, pairs=slice(-2, None)).first_pair == 2
    assert loss.residuals(batch, flows, out, pairs=[3, 1]).forward.shape[1] == 1

    def call(**changed):
        return problem({**x, **changed}, dev)

    with pytest.raises(RuntimeError, match="flowmap_amd: flow shape does not match depth"):
        loss_, batch_, flows_, out_ = call(fwd=x["fwd"][:, :, :-1])
        loss_.residuals(batch_, flows_, out_)
    with pytest.raises(RuntimeError, match="flowmap_amd: mask shape does not match depth"):
        loss_, batch_, flows_, out_ = call(bwd_mask=x["bwd_mask"][:, :-1])
        loss_.residuals(batch_, flows_, out_)
    with pytest.raises(RuntimeError, match="flowmap_amd: intrinsics / pose shapes do not match depth"):
        loss_, batch_, flows_, out_ = call(k=x["k"][:, :-1])
        loss_.residuals(batch_, flows_, out_)
    with pytest.raises(RuntimeError, match="flowmap_amd: depth must be float32"):
        loss_, batch_, flows_, out_ = call(depth=x["depth"].double())
        loss_.residuals(batch_, flows_, out_)
    with pytest.raises(RuntimeError, match="flowmap_amd: flows and masks must be float32"):
        loss_, batch_, flows_, out_ = call(fwd_mask=x["fwd_mask"].half())
        loss_.residuals(batch_, flows_, out_)
    r = loss.residuals(batch, flows, out, sums=False)
    with pytest.raises(RuntimeError, match="needs the sums"):
        r.pair_loss()


def case_host_tensor_refused():
    """Host tensors are refused on the fused route and on the general one."""
    for lazy in (True, False):
        def call(lazy=lazy):
            loss, batch, flows, out = problem(golden_inputs("a"), "cpu", lazy=lazy)
            loss.residuals(batch, flows, out)

        host_tensor_refused(call, "no CPU fallback|needs a GPU")


# ---- check 6: the GPU against the host double ----------------------------------------------------------------------------------------------


def case_gpu_against_host_double(dev, case, kind):
    """The same fixture through the HIP kernel and through the serial host build of the same functions: element for element.  Bit-equality
    is not required (the device contracts multiply-adds the host build, compiled with contraction off, does not; hardware reciprocal
    and reciprocal square root against IEEE division): the gate is check 1's, the largest ulp distance is printed."""
    from flowmap_amd import _lib
    from helpers import build_host_sim

    g = golden()
    x = golden_inputs(case)
    loss, batch, flows, out = problem(x, dev, kind)
    gpu = loss.residuals(batch, flows, out, predicted_flow=True)
    _lib.set_library_for_testing(build_host_sim())
    try:
        loss_h, batch_h, flows_h, out_h = problem(x, "cpu", kind)
        host = loss_h.residuals(batch_h, flows_h, out_h, predicted_flow=True)
    finally:
        _lib.set_library_for_testing(None)
    truth = {k[len(case) + 5:]: v for k, v in g.items() if k.startswith(f"{case}_f64_")}
    ref32 = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(f"{case}_")}
    worst = {}
    for name in ("forward", "backward", "forward_flow", "backward_flow"):
        a, b = getattr(gpu, name).cpu(), getattr(host, name)
        worst[name] = ulp_distance(a, b)
        key = (f"{kind}_" if "flow" not in name else "pred_") + name.split("_")[0]
        if case != "edge":  # (the edge case is gated piecewise by case_edge)
            assert_close_or_reference_gap(a, truth[key], ref32[key], rel=1e-4, slack=2.0, what=f"gpu {case}.{key}")
            assert_close_or_reference_gap(b, truth[key], ref32[key], rel=1e-4, slack=2.0, what=f"host {case}.{key}")
    assert_close(gpu.pair_sum.cpu(), host.pair_sum, 1e-4, what="pair_sum")
    assert_close(gpu.pair_valid.cpu(), host.pair_valid, 1e-12, what="pair_valid")
    print(f"  GPU vs host double, {case}/{kind}: max ulp distance {worst}")
    return worst
