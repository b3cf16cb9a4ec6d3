"""IntrinsicsSoftmin.residuals / projection.focal_sweep (fm_focal_sweep): the softmin focal sweep per frame pair — per candidate the flow
error and the fitted pose, per pair the softmin weights, the blended focal length and the blended K — straight from depth.  The cases
here take a device; tests/test_hostsim_focal_sweep.py runs them on the serial host double of the C ABI, tests/test_gpu_focal_sweep.py on
the MI355X.

Truths.  tests/golden/fn_focal_sweep.npz holds what the REFERENCE computes on two-frame slices (tools/make_golden_focal_sweep.py: its own
unproject, align_surfaces, compute_backward_flow and IntrinsicsSoftmin.forward) in fp32 and in fp64, for the shapes small enough to
commit; at every shape the same two evaluations come from the oracle (oracle/flowmap_oracle.py: lift, fit_poses, backward_flow_positions —
the per-pair form of its softmin_intrinsics, restated in oracle_sweep below), computed once per case.  Either way the gate is the
project's: conftest.assert_close_or_reference_gap, rel 1e-4, slack 2x the fp32 evaluation's own gap to fp64, norm-wise on error, focal,
intrinsics and poses and in max-abs on soft (gate_soft).

Inputs: oracle.synth_scene (noisy initial depth, its backward flows) with seeded uniform weights in [0.1, 1]; candidates
linspace(0.5, 2, n) as the reference's configuration spaces them.

Cases (batch, frames, h, w), P, n; a workgroup of 256 threads owns one (batch entry, pair, candidate): 1x2x5x7 with indices=None (all 35
pixels: fewer points than a wave, one pair) at n = 1 (a softmin of one) and 3; 1x5x17x23, P 63 (one short of a wave), n 7; 1x6x24x32,
P 200 and 257 (one past a round of the workgroup), n 60 (the reference's count); 1x4x64x128, P 1025 (several rounds plus one), n 65 (the
curve kernel's second lane-strided round); 2x4x9x12, P 64, n 5 (two batch entries); 1x3x9x12 with flows that leave the frame (taps skipped).
"""

from __future__ import annotations

import functools

import torch

from conftest import assert_close_or_reference_gap, load_golden, relerr, t
from operator_checks import HEIGHT, WIDTH, assert_training_untouched, gate_pair, host_tensor_refused, same_tensors, train, ulp_distance, window_rows
from oracle import flowmap_oracle as orc

THREADS = 256  # threads per workgroup (fm_focal_sweep.hip: kSweepThreads)
INPUT_KEYS = ("depth", "weights", "bwd")
FIELDS = ("error", "soft", "focal", "intrinsics", "poses")

# name -> ((batch, frames, h, w), seed, P (None: indices=None with num_points 8192), candidates)
SPECS = {
    "tiny1": ((1, 2, 5, 7), 41, None, 1),
    "tiny3": ((1, 2, 5, 7), 41, None, 3),
    "odd": ((1, 5, 17, 23), 42, 63, 7),
    "ref200": ((1, 6, 24, 32), 43, 200, 60),
    "ref257": ((1, 6, 24, 32), 43, 257, 60),
    "wide": ((1, 4, 64, 128), 44, 1025, 65),
    "two": ((2, 4, 9, 12), 45, 64, 5),
    "border": ((1, 3, 9, 12), 46, 60, 5),
}
GOLDEN_CASES = ("tiny1", "tiny3", "odd", "ref200", "two", "border")  # (the others' inputs are too large to commit)
NUM_POINTS_DEFAULT = 8192


def candidates_of(name):
    return torch.linspace(0.5, 2.0, SPECS[name][3])


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """depth (b, f, h, w), weights (b, f-1, h, w), bwd (b, f-1, h, w, 2) of a case (tools/make_golden_focal_sweep.py draws them from here)."""
    (b, f, h, w), seed, _, _ = SPECS[name]
    scenes = [orc.synth_scene(f, h, w, seed=seed + 100 * i) for i in range(b)]
    out = {"depth": torch.stack([s["depth_init"] for s in scenes]), "bwd": torch.cat([s["flows"].backward for s in scenes]).clone(),
           "weights": 0.1 + 0.9 * torch.rand((b, f - 1, h, w), generator=torch.Generator().manual_seed(seed))}
    if name == "border":  # (as alignment_residual_cases' border fixture: a band along every side leaves the frame by 0.3 of it, the corners on two sides)
        out["bwd"][:, :, :, :2, 0] -= 0.3
        out["bwd"][:, :, :, -2:, 0] += 0.3
        out["bwd"][:, :, :2, :, 1] -= 0.3
        out["bwd"][:, :, -2:, :, 1] += 0.3
    return out


def case_indices(name):
    """The indices of a case with an explicit P; None for the cases that let the call draw them."""
    (_, _, h, w), seed, points, _ = SPECS[name]
    if points is None:
        return None
    if name == "border":  # every pixel of the outermost rows first: the band that leaves the frame is in the selection
        return torch.linspace(0, h * w - 1, points, dtype=torch.int64)
    return torch.randperm(h * w, generator=torch.Generator().manual_seed(seed))[:points]


def windows_of(frames):
    """All pairs, the first, the last, and a middle slice — on every multi-pair shape."""
    pairs = frames - 1
    if pairs == 1:
        return [None]
    return [None, (0, 1), (pairs - 1, 1), slice(1, max(2, pairs - 1))]


# ---- the oracle's per-pair sweep ----------------------------------------------------------------------------------------------------------


def oracle_sweep(x, candidates, indices, dtype):
    """error (b, pairs, n), soft, focal (b, pairs), intrinsics (b, pairs, 3, 3), poses (b, pairs, n, 4, 4) of every pair by the oracle in
    ``dtype``: oracle.softmin_intrinsics (intrinsics_softmin.py:85-131) on the two-frame slice of each pair, with what it drops kept."""
    depth, wts, bwd = (x[key].to(dtype) for key in INPUT_KEYS)
    b, f, h, w = depth.shape
    n = candidates.numel()
    cand = candidates.to(dtype)
    k = orc.focal_to_k(cand, (h, w))  # (n, 3, 3)
    xy, _ = orc.pixel_grid((h, w), dtype=dtype)
    rep = lambda v: v[:, None].expand(b, n, *v.shape[1:]).reshape(b * n, *v.shape[1:])  # noqa: E731
    kk = k[None, :, None].expand(b, n, 2, 3, 3).reshape(b * n, 2, 3, 3)
    out = {key: [] for key in FIELDS + ("point_error",)}
    for i in range(f - 1):
        surfaces = orc.lift(xy, rep(depth[:, i:i + 2]), kk[:, :, None, None])
        e = orc.fit_poses(surfaces, rep(bwd[:, i:i + 1]), rep(wts[:, i:i + 1]), indices)  # (b·n, 2, 4, 4): E_0 = I, E_1 = the fitted pose
        pts = surfaces.reshape(b * n, 2, h * w, 3)[:, :, indices]
        back = orc.backward_flow_positions(pts, e, kk).reshape(b, n, -1, 2)
        flow = back - xy.reshape(h * w, 2)[indices]
        flow_gt = bwd[:, i:i + 1].reshape(b, 1, h * w, 2)[:, :, indices]
        wt = wts[:, i:i + 1].reshape(b, 1, h * w, 1)[:, :, indices]
        per_point = ((flow - flow_gt) * wt).abs().sum(dim=3)
        err = per_point.sum(dim=2)
        soft = torch.nn.functional.softmin((err - err.min(dim=1, keepdim=True).values) * 10, dim=1)
        out["error"].append(err)
        out["point_error"].append(per_point)
        out["soft"].append(soft)
        out["focal"].append((cand * soft).sum(dim=1))
        out["intrinsics"].append((k[None] * soft[:, :, None, None]).sum(dim=1))
        out["poses"].append(e[:, 1].reshape(b, n, 4, 4))
    return {key: torch.stack(v, dim=1) for key, v in out.items()}


@functools.lru_cache(maxsize=None)
def _oracle_case(name, index_key):
    indices = torch.tensor(index_key, dtype=torch.int64)
    return {dtype: oracle_sweep(case_inputs(name), candidates_of(name), indices, dtype) for dtype in (torch.float32, torch.float64)}


def oracle_case(name, indices):
    """{dtype: fields} of a case on ``indices``, once per (case, index set)."""
    return _oracle_case(name, tuple(int(i) for i in indices.cpu().tolist()))


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------


def gate_soft(ours, truth, ref32, what):
    """``soft`` in max-abs against the fp64 twin: max(1e-4, 2 x the fp32 evaluation's own max-abs gap)."""
    ours, truth, ref32 = (torch.as_tensor(v).double().cpu() for v in (ours, truth, ref32))
    e, gap = float((ours - truth).abs().max()), float((ref32 - truth).abs().max())
    assert e <= max(1e-4, 2.0 * gap), f"{what}: max abs err {e:.3e} > max(1e-4, 2 x fp32-reference gap {gap:.3e})"
    return e, gap


def check_fields(r, truth, ref32, what, rows=slice(None)):
    """The gate on every field of a FocalSweep against (truth, ref32) restricted to the pairs ``rows``."""
    worst = {}
    for name in FIELDS + ("point_error",):
        ours = getattr(r, name)
        if ours is None or name not in truth:
            continue
        tr, rf = torch.as_tensor(truth[name])[:, rows], torch.as_tensor(ref32[name])[:, rows]
        assert tuple(ours.shape) == tuple(tr.shape), f"{what}.{name}: shape {tuple(ours.shape)} vs {tuple(tr.shape)}"
        if name == "soft":
            e, gap = gate_soft(ours, tr, rf, f"{what}.soft")
        else:
            e, gap = assert_close_or_reference_gap(ours.cpu(), tr, rf, rel=1e-4, slack=2.0, what=f"{what}.{name}")
        print(f"  {what}.{name}: err {e:.2e} (fp32 reference's own gap {gap:.2e})")
        worst[name] = e
    return worst


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------


def problem(name, dev, weights="tensor", x=None, model_output=False, num_points=None, regression=None):
    """(module, batch, flows, backbone_output) over the inputs of a case; ``weights``: "tensor" or ("logits", sensitivity) for a LazyWeights
    of x["weights"]; ``model_output``: a ModelOutput (``backward_correspondence_weights``) instead of a BackboneOutput (``weights``)."""
    from flowmap_amd import BackboneOutput, Batch, Flows, ModelOutput
    from flowmap_amd.model.intrinsics_softmin import IntrinsicsSoftmin, IntrinsicsSoftminCfg
    from flowmap_amd.model.projection import LazyWeights

    x = {key: v.clone().to(dev) for key, v in (x or case_inputs(name)).items()}  # (clones: the cached inputs stay as they were drawn)
    b, f, h, w = x["depth"].shape
    wts = x["weights"] if weights == "tensor" else LazyWeights(x["weights"], weights[1])
    points = SPECS[name][2]
    cfg = IntrinsicsSoftminCfg("softmin", num_points or points or NUM_POINTS_DEFAULT, 0.5, 2.0, SPECS[name][3], regression)
    module = IntrinsicsSoftmin(cfg).to(dev)
    out = ModelOutput(x["depth"], None, None, None, wts) if model_output else BackboneOutput(x["depth"], wts)
    return module, Batch(torch.zeros((b, f, 3, h, w), device=dev)), Flows(None, x["bwd"], None, None), out


def run(name, dev, **kw):
    module, batch, flows, out = problem(name, dev)
    idx = case_indices(name)
    return module.residuals(batch, flows, out, indices=None if idx is None else idx.to(dev), **kw)


def same_fields(a, b, what="", **kw):
    same_tensors(a, b, FIELDS + ("point_error",), what, **kw)


def check_layout(r, name, dev, count=None, first=0):
    (b, f, h, w), _, points, n = SPECS[name]
    count = f - 1 if count is None else count
    p = r.indices.numel()
    assert p == (min(NUM_POINTS_DEFAULT, h * w) if points is None else points)
    assert (r.first_pair, r.count) == (first, count)
    assert r.focal_lengths.shape == (n,) and r.focal_lengths.dtype == torch.float32 and r.indices.dtype == torch.int64
    assert r.error.shape == (b, count, n) and r.error.dtype == torch.float64
    assert r.soft.shape == (b, count, n) and r.focal.shape == (b, count) and r.intrinsics.shape == (b, count, 3, 3)
    assert all(v.dtype == torch.float32 for v in (r.soft, r.focal, r.intrinsics))
    assert r.poses is None or (r.poses.shape == (b, count, n, 4, 4) and r.poses.dtype == torch.float32)
    assert r.point_error is None or (r.point_error.shape == (b, count, n, p) and r.point_error.dtype == torch.float32)
    for v in (r.error, r.soft, r.focal, r.intrinsics, r.poses, r.point_error, r.indices, r.focal_lengths):
        assert v is None or (not v.requires_grad and v.device.type == torch.device(dev).type)


# ---- case 1: reference parity --------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("fn_focal_sweep")


def golden_fields(name):
    g = golden()
    return {key: g[f"{name}_f64_{key}"] for key in FIELDS}, {key: g[f"{name}_{key}"] for key in FIELDS}


def case_reference_parity(dev, name):
    """A fixture case against what the imported reference computes on the two-frame slices, fp64 the truth, fp32 the reference evaluation."""
    g = golden()
    module, batch, flows, out = problem(name, dev, x={key: t(g[f"{name}_{key}"]) for key in INPUT_KEYS})  # the inputs the fixture was made from
    idx = None if SPECS[name][2] is None else t(g[f"{name}_indices"]).to(dev)
    r = module.residuals(batch, flows, out, indices=idx, points=True)
    check_layout(r, name, dev)
    assert torch.equal(r.indices.cpu(), t(g[f"{name}_indices"])), "the indices the fixture was computed on"
    assert torch.equal(r.focal_lengths.cpu(), t(g[f"{name}_candidates"]))
    check_fields(r, *golden_fields(name), f"{name} vs the reference")
    total = r.point_error.double().sum(-1)  # the per-point terms are the fp32 values the kernel converts and adds in fp64: only the order differs
    assert bool(((total - r.error).abs() <= r.indices.numel() * 2.0**-52 * total).all()), "error is not the sum of point_error"
    assert bool((r.soft.sum(-1) - 1).abs().max() <= 1e-5) and bool(torch.isfinite(r.poses).all())
    return r


# ---- case 2: oracle parity, every shape and window -----------------------------------------------------------------------------------------


def case_oracle_parity(dev, name):
    module, batch, flows, out = problem(name, dev)
    idx = case_indices(name)
    f = SPECS[name][0][1]
    full = None
    for window in windows_of(f):
        r = module.residuals(batch, flows, out, pairs=window, indices=None if idx is None else idx.to(dev))
        rows = window_rows(window, f - 1)
        check_layout(r, name, dev, count=rows.stop - rows.start, first=rows.start)
        terms = oracle_case(name, r.indices)
        check_fields(r, terms[torch.float64], terms[torch.float32], f"{name}[{window}]", rows=rows)
        full = r if window is None else full
    if name.startswith("tiny"):  # indices=None drew every pixel once
        assert sorted(full.indices.cpu().tolist()) == list(range(35))
    if name == "border":
        xy, _ = orc.pixel_grid(SPECS[name][0][2:])
        where = (xy + case_inputs(name)["bwd"]).reshape(1, f - 1, -1, 2)[:, :, idx]
        outside = ((where < 0) | (where > 1)).any(-1)
        assert bool(outside.any(-1).all()) and int(outside.sum()) < outside.numel(), "the border case does not leave the frame"
    return full


# ---- case 3: agreement with the training path -------------------------------------------------------------------------------------------------


def case_training_path(dev, name):
    """residuals against what ``forward`` and the fit's own launch give on the same indices: K of pair (0, 1), the candidates' poses against
    ProcrustesFit with batch_repeat = n, and pair k against ``forward`` on the video cut down to frames (k, k+1)."""
    from flowmap_amd import BackboneOutput, Batch, Flows, _ops

    module, batch, flows, out = problem(name, dev)
    idx = case_indices(name)
    r0 = module.residuals(batch, flows, out, indices=None if idx is None else idx.to(dev))
    idx = r0.indices
    module._draw_indices = lambda count, device: idx
    terms = oracle_case(name, idx)
    gap = {key: relerr(terms[torch.float32][key], terms[torch.float64][key]) for key in FIELDS}
    (b, f, h, w), _, _, n = SPECS[name]
    first = module.residuals(batch, flows, out, pairs=(0, 1), indices=idx)
    k = module.forward(batch, flows, out, 0)
    assert k.shape == (b, f, 3, 3)
    e = gate_pair(first.intrinsics[:, 0].cpu(), k[:, 0].cpu(), gap["intrinsics"], f"{name}: intrinsics of pair 0 vs forward")
    print(f"  {name}: K of pair 0 vs forward: rel err {e:.2e}")
    _, k_pair = module._candidate_intrinsics(b, (h, w))
    rel, _ = _ops.ProcrustesFit.apply(out.depths[:, :2].contiguous(), k_pair, None, out.weights[:, :1].contiguous(), flows.backward[:, :1].contiguous(), idx, 0.0, n)
    e = gate_pair(first.poses[:, 0].cpu(), rel.reshape(b, n, 4, 4).cpu(), gap["poses"], f"{name}: poses of pair 0 vs ProcrustesFit(batch_repeat=n)")
    print(f"  {name}: poses of pair 0 vs the fit: rel err {e:.2e}")
    for pair in range(f - 1):
        cut = BackboneOutput(out.depths[:, pair:pair + 2].contiguous(), out.weights[:, pair:pair + 1].contiguous())
        k = module.forward(Batch(batch.videos[:, pair:pair + 2]), Flows(None, flows.backward[:, pair:pair + 1].contiguous(), None, None), cut, 0)
        gate_pair(r0.intrinsics[:, pair].cpu(), k[:, 0].cpu(), gap["intrinsics"], f"{name}: intrinsics of pair {pair} vs forward on frames ({pair}, {pair + 1})")


# ---- case 4: reproducible and window-independent ----------------------------------------------------------------------------------------------


def case_reproducible(dev, name):
    module, batch, flows, out = problem(name, dev)
    idx = case_indices(name)
    kw = dict(indices=None if idx is None else idx.to(dev), points=True)
    full = module.residuals(batch, flows, out, **kw)
    same_fields(module.residuals(batch, flows, out, **kw), full, "repeat: ")
    assert torch.equal(module.residuals(batch, flows, out, **kw).indices, full.indices)
    for pair in range(SPECS[name][0][1] - 1):
        same_fields(module.residuals(batch, flows, out, pairs=(pair, 1), **kw), full, f"window ({pair}, 1): ", rows=slice(pair, pair + 1))
    bare = module.residuals(batch, flows, out, indices=kw["indices"], poses=False)  # what was not asked for is not produced
    assert bare.poses is None and bare.point_error is None and torch.equal(bare.error, full.error) and torch.equal(bare.soft, full.soft)


# ---- case 5: the GPU against the host double --------------------------------------------------------------------------------------------------


def case_gpu_against_host_double(dev, name):
    """The same case through the HIP kernel and through the serial host build of the same functions, element for element on point_error,
    poses and error: the gate of the oracle parity (the host double's values taken as the other fp32 evaluation), the largest ulp distance
    printed.  Bit-equality is not required: the device contracts multiply-adds and sums the moments in another order."""
    from flowmap_amd import _lib
    from helpers import build_host_sim

    gpu = run(name, dev, points=True)
    _lib.set_library_for_testing(build_host_sim())
    try:
        module, batch, flows, out = problem(name, "cpu")
        host = module.residuals(batch, flows, out, indices=gpu.indices.cpu(), points=True)
    finally:
        _lib.set_library_for_testing(None)
    terms = oracle_case(name, gpu.indices)
    gap = {key: relerr(terms[torch.float32][key], terms[torch.float64][key]) for key in ("point_error", "poses", "error")}
    worst = {}
    for key in ("point_error", "poses", "error"):
        e = gate_pair(getattr(gpu, key).cpu(), getattr(host, key), gap[key], f"{name}: gpu vs host double, {key}")
        worst[key] = (e, ulp_distance(getattr(gpu, key).cpu().float(), getattr(host, key).float()))
    print(f"  GPU vs host double, {name}: (rel err, max ulp distance in fp32) {worst}")
    check_fields(gpu, terms[torch.float64], terms[torch.float32], f"gpu {name}")
    check_fields(host, terms[torch.float64], terms[torch.float32], f"host {name}")
    return worst


# ---- case 6: lazy weights ----------------------------------------------------------------------------------------------------------------------


def case_lazy_weights(dev, name, sensitivity):
    """A LazyWeights of logits — sensitivity != 0: the kernel applies the sigmoid; 0: its value (0.5 everywhere) is formed for the call —
    against the same call on the materialised weights, inside the gate; nothing is evaluated ON the LazyWeights."""
    x = dict(case_inputs(name))
    x["weights"] = 0.03 * torch.randn(x["weights"].shape, generator=torch.Generator().manual_seed(3))
    idx = case_indices(name).to(dev)
    module, batch, flows, out = problem(name, dev, weights=("logits", sensitivity), x=x)
    lazy = module.residuals(batch, flows, out, indices=idx, points=True)
    assert out.weights._dense is None, "the LazyWeights was evaluated"
    dense = (sensitivity * x["weights"]).sigmoid()
    module_p, batch_p, flows_p, out_p = problem(name, dev, x={**x, "weights": dense})
    plain = module_p.residuals(batch_p, flows_p, out_p, indices=idx, points=True)
    if sensitivity != 0.0:
        assert float(dense.min()) < 0.2 and float(dense.max()) > 0.8  # (the logits really spread the weights)
    truth = oracle_sweep({**x, "weights": dense.double()}, candidates_of(name), idx.cpu(), torch.float64)
    ref32 = oracle_sweep({**x, "weights": dense}, candidates_of(name), idx.cpu(), torch.float32)
    check_fields(lazy, truth, ref32, f"{name}[lazy, sensitivity {sensitivity}]")
    check_fields(plain, truth, ref32, f"{name}[materialised]")
    gap = {key: relerr(ref32[key], truth[key]) for key in FIELDS}
    for key in ("error", "focal", "intrinsics", "poses"):
        gate_pair(getattr(lazy, key).cpu(), getattr(plain, key).cpu(), gap[key], f"{name}: lazy vs materialised weights, {key}")
    if sensitivity == 0.0:  # the same numbers reach the kernel on both routes
        same_fields(lazy, plain, "sensitivity 0: ")


# ---- case 7: training is left alone ------------------------------------------------------------------------------------------------------------


def _rng_state(dev):
    from flowmap_amd import _ops

    state = [torch.get_rng_state().clone()]
    if torch.device(dev).type == "cuda":
        state.append(torch.cuda.get_rng_state(torch.device(dev)).clone())
    return state, {key: v.clone() for key, v in _ops._rng_states.items()}


def _train(dev, tracking, fuse, regressed, calls, steps=3):
    """operator_checks.train, 3 steps from step 1 after the warm-up, on a model with softmin intrinsics — ``regressed``: past the hand-over,
    else inside the sweep's window; ``calls``: IntrinsicsSoftmin.residuals between forward and backward (a window, given indices) and
    between the steps (every pair, indices=None).  -> (the record, per call whether torch's generators and the seed state stayed put).

    The sweep draws 64 points for 6 candidates: the backward kernels of the sweep (fm_softmin_score_bwd, the fit's batch_repeat scatter) add
    into dL/ddepth with float atomics, one thread per point for a group of six candidates — at this size ONE wavefront issues all of them,
    so two runs add in the same order and the baseline itself is bit-reproducible on the GPU; with more points or candidates it is not, calls
    or no calls (cases.py, the fused-Adam trajectory: "float atomics whose order differs from run to run"), and nothing could be decided."""
    from flowmap_amd.model.intrinsics_softmin import IntrinsicsSoftminCfg, RegressionCfg

    given = torch.randperm(HEIGHT * WIDTH, generator=torch.Generator().manual_seed(9))[:100].to(dev)
    rng_kept = []

    def probed(call):
        def probe(ns):
            state = _rng_state(dev)
            r = call(ns)
            rng_kept.append(_states_equal(state, _rng_state(dev)))
            return r

        return probe

    mid = probed(lambda ns: ns.model.intrinsics.residuals(ns.batch, ns.flows, ns.out, pairs=(1, 2), indices=given, points=True))
    after = probed(lambda ns: ns.model.intrinsics.residuals(ns.batch, ns.flows, ns.out, seed=ns.step))
    regression = RegressionCfg(1, 1) if regressed else RegressionCfg(100, 100)
    run = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True, calls=(mid, after) if calls else None,
                intrinsics=IntrinsicsSoftminCfg("softmin", 64, 0.5, 2.0, 6, regression),
                prepare=lambda ns: torch.manual_seed(7))  # the sweep's own indices come from torch's CPU generator
    return run, rng_kept


def _states_equal(a, b):
    return (len(a[0]) == len(b[0]) and all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1].keys() == b[1].keys()
            and all(torch.equal(a[1][key], b[1][key]) for key in a[1]))


def case_training_untouched(dev, tracking, fuse, regressed):
    """Two identical runs of three steps, with and without residuals() calls (one of them with indices=None):
    operator_checks.assert_training_untouched with ``focal_sweep`` the one counter that differs, the module's window has the same length
    and entries, and torch's CPU and device generators and the graph-capturable seed state are unchanged across every call."""
    steps = 3
    plain, _ = _train(dev, tracking, fuse, regressed, calls=False, steps=steps)
    with_calls, rng_kept = _train(dev, tracking, fuse, regressed, calls=True, steps=steps)
    assert_training_untouched(plain, with_calls, "focal_sweep", 2 * steps)
    window, base_window = with_calls.model.intrinsics.window, plain.model.intrinsics.window
    assert len(window) == len(base_window) and all(torch.equal(x, y) for x, y in zip(window, base_window)), "the window differs"
    assert len(base_window) == (1 if regressed else steps + 1)  # (the discarded step is a training step of the sweep too)
    assert len(rng_kept) == 2 * steps and all(rng_kept), "a generator or the seed state moved across a call"
    for r in with_calls.seen:
        assert bool(torch.isfinite(r.error).all()) and bool(torch.isfinite(r.intrinsics).all())
    first, second = with_calls.seen[0], with_calls.seen[1]
    assert (first.first_pair, first.count) == (1, 2) and first.point_error.shape == (1, 2, 6, 100) and second.error.shape == (1, 4, 6) and second.indices.numel() == 64


# ---- case 8: arguments -------------------------------------------------------------------------------------------------------------------------


def case_arguments(dev):
    import pytest

    from flowmap_amd import FocalSweep, _ops
    from flowmap_amd.model import projection as fm

    name = "odd"
    module, batch, flows, out = problem(name, dev)
    x = {key: v.clone().to(dev) for key, v in case_inputs(name).items()}
    idx = case_indices(name).to(dev)
    for bad in (slice(0, 4, 2), (0, 0), (3, 2), (-1, 2), (0, 5), "all", 1, (1.0, 2), (0, 1, 2), slice(3, 1)):
        with pytest.raises(ValueError, match="flowmap_amd: .*pairs"):
            module.residuals(batch, flows, out, pairs=bad, indices=idx)
    assert module.residuals(batch, flows, out, pairs=slice(None), indices=idx).count == 4
    assert module.residuals(batch, flows, out, pairs=slice(-2, None), indices=idx).first_pair == 2
    assert module.residuals(batch, flows, out, pairs=[3, 1], indices=idx).count == 1
    # a ModelOutput qualifies as well as a BackboneOutput; the function is the same call
    before = _ops.counters["focal_sweep"]
    module_m, batch_m, flows_m, out_m = problem(name, dev, model_output=True)
    via_model_output = module_m.residuals(batch_m, flows_m, out_m, indices=idx, pairs=(1, 2))
    direct = fm.focal_sweep(x["depth"], x["weights"], x["bwd"], module.focal_length_candidates, indices=idx, pairs=(1, 2))
    assert _ops.counters["focal_sweep"] == before + 2 and isinstance(direct, FocalSweep)
    same_fields(direct, via_model_output, "function vs method: ")
    # indices outside the image are clamped: bit for bit the call on pre-clamped indices
    h, w = x["depth"].shape[2:]
    wild = idx.clone()
    wild[::5] += h * w
    wild[1::5] -= 10 * h * w
    clamped = module.residuals(batch, flows, out, indices=wild, points=True)
    same_fields(clamped, module.residuals(batch, flows, out, indices=wild.clamp(0, h * w - 1), points=True), "clamped indices: ")
    assert torch.equal(clamped.indices, wild)
    # indices=None: num_points of them, from the explicit seed
    module_s, batch_s, flows_s, out_s = problem(name, dev, num_points=50)
    a, b, c = (module_s.residuals(batch_s, flows_s, out_s, seed=s) for s in (0, 0, 1))
    assert a.indices.numel() == 50 and a.indices.unique().numel() == 50 and torch.equal(a.indices, b.indices) and not torch.equal(a.indices, c.indices)
    same_fields(a, b, "same seed: ")
    assert fm.focal_sweep(x["depth"], x["weights"], x["bwd"], module.focal_length_candidates).indices.numel() == h * w  # num_points None: every pixel
    for tensor in (x["depth"], x["weights"], x["bwd"], out.depths, out.weights, flows.backward, idx, module.focal_length_candidates):
        assert not [key for key in tensor.__dict__ if key.startswith("_fm_")], "a note was left on an argument"

    def refused(match, kw=None, **changed):
        y = {**x, **changed}
        with pytest.raises(RuntimeError, match=match):
            fm.focal_sweep(y["depth"], y["weights"], y["bwd"], module.focal_length_candidates, **{"indices": idx, **(kw or {})})

    refused("flowmap_amd: focal_sweep: indices must be an int64 tensor", kw={"indices": idx.float()})
    refused("flowmap_amd: focal_sweep: indices must be an int64 tensor", kw={"indices": idx.int()})
    refused("flowmap_amd: focal_sweep: indices must be an int64 tensor", kw={"indices": [0, 1, 2]})
    refused("flowmap_amd: focal_sweep: indices must be a non-empty 1-D tensor", kw={"indices": idx[:0]})
    refused("flowmap_amd: focal_sweep: indices must be a non-empty 1-D tensor", kw={"indices": idx[None]})
    if torch.device(dev).type != "cpu":
        refused("flowmap_amd: focal_sweep: indices are on cpu", kw={"indices": idx.cpu()})
    refused("flowmap_amd: focal_sweep: backward_flow of shape .* does not match the depths", bwd=x["bwd"][:, :, :-1])
    refused("flowmap_amd: focal_sweep: backward_flow of shape .* does not match the depths", bwd=x["bwd"][:, :-1])
    refused("flowmap_amd: focal_sweep: weights of shape .* do not match the depths", weights=x["weights"][:, :-1])
    refused("flowmap_amd: focal_sweep: depths of shape .* expected", depth=x["depth"][0])
    refused("flowmap_amd: focal_sweep: depths must be float32", depth=x["depth"].double())
    refused("flowmap_amd: focal_sweep: backward_flow must be float32", bwd=x["bwd"].double())
    refused("flowmap_amd: focal_sweep: weights must be float32", weights=x["weights"].double())
    with pytest.raises(RuntimeError, match="flowmap_amd: focal_sweep: focal_length_candidates must be a non-empty 1-D tensor"):
        fm.focal_sweep(x["depth"], x["weights"], x["bwd"], module.focal_length_candidates[:0], indices=idx)
    # batch x pairs beyond one call's rows: refused before anything of that size is formed (expanded views: no memory behind them)
    big = 65536
    with pytest.raises(ValueError, match="flowmap_amd: focal_sweep: batch x pairs = 65536 exceeds"):
        fm.focal_sweep(x["depth"][:, :2].expand(big, 2, h, w), x["weights"][:, :1].expand(big, 1, h, w), x["bwd"][:, :1].expand(big, 1, h, w, 2),
                       module.focal_length_candidates, indices=idx)
    # a module whose frame shard is active
    class Shard:
        active = True

    module.shard = Shard()
    with pytest.raises(RuntimeError, match="flowmap_amd: IntrinsicsSoftmin.residuals: this module's frame shard is active"):
        module.residuals(batch, flows, out, indices=idx)
    module.shard = None
    # gradients recorded around the call change nothing: the outputs never require one
    depth = case_inputs(name)["depth"].clone().requires_grad_(True)
    module_, batch_, flows_, out_ = problem(name, dev, x={**case_inputs(name), "depth": depth})
    rg = module_.residuals(batch_, flows_, out_, indices=idx, points=True)
    assert not any(v.requires_grad for v in (rg.error, rg.soft, rg.focal, rg.intrinsics, rg.poses, rg.point_error))


def case_state_untouched(dev):
    """No global_step: the call works before and after the hand-over and leaves ``window`` and the regressed focal length alone."""
    from flowmap_amd.model.intrinsics_softmin import RegressionCfg

    name = "odd"
    module, batch, flows, out = problem(name, dev, regression=RegressionCfg(2, 2))
    idx = case_indices(name).to(dev)
    module._draw_indices = lambda count, device: idx
    module.train()
    before = module.residuals(batch, flows, out, indices=idx)
    assert module.window == []
    with torch.no_grad():
        for step in range(4):  # steps 0, 1: the sweep (both inside the window); 2: the hand-over; 3: regressed
            module.forward(batch, flows, out, step)
    window = [v.clone() for v in module.window]
    focal = module.intrinsics_regressed.focal_length.detach().clone()
    assert len(window) == 2
    after = module.residuals(batch, flows, out, indices=idx)
    same_fields(after, before, "after the hand-over: ")
    assert len(module.window) == 2 and all(torch.equal(x, y) for x, y in zip(module.window, window))
    assert torch.equal(module.intrinsics_regressed.focal_length.detach(), focal)
    terms = oracle_case(name, idx.cpu())
    gate_pair(window[0].cpu(), before.focal[0, 0].cpu(), relerr(terms[torch.float32]["focal"], terms[torch.float64]["focal"]), "the window's entry vs focal of pair 0")


def case_host_tensor_refused():
    """Host tensors are refused by name — through the method and through the function."""
    from flowmap_amd.model import projection as fm

    module, batch, flows, out = problem("tiny3", "cpu")
    host_tensor_refused(lambda: module.residuals(batch, flows, out), "flowmap_amd: focal_sweep: tensors are on cpu.*no CPU fallback")
    host_tensor_refused(lambda: fm.focal_sweep(out.depths, out.weights, flows.backward, module.focal_length_candidates),
                        "flowmap_amd: focal_sweep: tensors are on cpu")
