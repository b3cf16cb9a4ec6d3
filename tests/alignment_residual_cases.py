"""ExtrinsicsProcrustes.residuals / projection.alignment_residuals (fm_alignment_residuals): the terms of the objective the Procrustes fit
minimises — offset = T·p − q, residual = ‖offset‖², Σ w·residual and Σ w per pair — straight from depth or from an explicit surfaces tensor.
The cases here take a device; tests/test_hostsim_alignment_residuals.py runs them on the serial host double of the C ABI,
tests/test_gpu_alignment_residuals.py on the MI355X.

Truths.  tests/golden/fn_alignment_residuals.npz holds what the REFERENCE computes (tools/make_golden_alignment_residuals.py: its own
align_surfaces with align_rigid recorded, transform_rigid, homogenize_points) in fp32 and in fp64 for the small shapes and the border case;
for the shapes too large to commit, the same two evaluations come from the oracle (oracle/flowmap_oracle.py: lift, bilinear_border,
rigid_fit), computed once per shape.  Either way the gate is the project's: conftest.assert_close_or_reference_gap, rel 1e-4, slack 2x the
fp32 evaluation's own gap to fp64.

Inputs: flow_residual_cases.inputs (depth in [0.5, 2], flows N(0, 0.02), continuous weights in [0, 1) with a quarter zero — its backward
mask serves as the correspondence weights — and small_poses).

Shapes (batch, frames, h, w); a workgroup owns TILE = 1024 elements of one (batch entry, pair): 1x2x5x7 (one pair, fewer elements than a
wavefront), 1x5x17x23 (odd everything, a K per frame), 1x6x24x32 (the golden step size), 1x4x64x128 (eight tiles per pair: the second
stage adds real partials), 1x2x25x41 and 1x2x31x33 (1025 and 1023 pixels: one element more / fewer than a whole tile), 2x4x9x12 (two
batch entries); index sets: P = 3, P = 50 on 5x7 (repeats, P > h·w), P = TILE + 1, and procrustes_indices' linspace selection.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

from conftest import assert_close, assert_close_or_reference_gap, load_golden, t
from flow_residual_cases import inputs
from operator_checks import HEIGHT, WIDTH, assert_training_untouched, same_tensors, train, ulp_distance
from oracle import flowmap_oracle as orc

TILE = 1024  # elements per workgroup (fm_alignment_residuals.hip: kAlignTile)
INPUT_KEYS = ("depth", "k", "extrinsics", "bwd", "weights")

# name -> (seed, batch, frames, h, w, a K per frame, number of indices of the fit, how they are drawn)
FIXTURE_SPECS = {
    "a": (11, 1, 2, 5, 7, False, 50, "randint"),  # repeats, P > h·w
    "b": (12, 1, 5, 17, 23, True, 40, "linspace"),  # procrustes_indices' deterministic selection
    "c": (13, 2, 4, 9, 12, True, 30, "randint"),
    "border": (14, 1, 3, 9, 12, False, 60, "linspace"),  # flows that push samples off all four sides and a corner
}


def fixture_indices(name):
    seed, _, _, h, w, _, points, how = FIXTURE_SPECS[name]
    if how == "linspace":  # extrinsics_procrustes.py:34-51 without randomisation
        return torch.linspace(0, h * w - 1, points, dtype=torch.int64)
    return torch.randint(0, h * w, (points,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def fixture_inputs(name):
    """The inputs of a fixture case (tools/make_golden_alignment_residuals.py draws them from here and stores them)."""
    seed, b, f, h, w, per_frame_k, _, _ = FIXTURE_SPECS[name]
    x = inputs(seed, b, f, h, w, per_frame_k)
    out = {"depth": x["depth"], "k": x["k"], "extrinsics": x["extrinsics"], "bwd": x["bwd"].clone(), "weights": x["bwd_mask"]}
    if name == "border":  # a band along every side leaves the frame by 0.3 of it; the corner pixels leave it on two sides at once
        out["bwd"][:, :, :, :2, 0] -= 0.3
        out["bwd"][:, :, :, -2:, 0] += 0.3
        out["bwd"][:, :, :2, :, 1] -= 0.3
        out["bwd"][:, :, -2:, :, 1] += 0.3
    return out


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("fn_alignment_residuals")


def golden_inputs(case):
    return {key: t(golden()[f"{case}_{key}"]) for key in INPUT_KEYS}


def golden_terms(case, route):
    """({name: fp64 array}, {name: fp32 array}) of a fixture case; ``route``: "dense" (every pixel, the given poses), "given" (the case's
    indices, the given poses) or "fit" (the case's indices, the reference's own fit on them)."""
    g = golden()
    names = ("offset", "residual", "loss")
    return {n: g[f"{case}_f64_{route}_{n}"] for n in names}, {n: g[f"{case}_{route}_{n}"] for n in names}


def relative_pose(ext):
    """T_i = E_i⁻¹·E_{i+1} (projection.py:176)."""
    return torch.linalg.inv(ext[:, :-1]) @ ext[:, 1:]


def oracle_terms(x, indices, dtype, fit):
    """offset, residual, pair loss and T of the inputs ``x`` by the oracle's composition in ``dtype``: lift + bilinear_border + the given
    T_i = E_i⁻¹E_{i+1} or, with ``fit``, rigid_fit on the same correspondences."""
    depth, k, ext, bwd, wts = (x[n].to(dtype) for n in INPUT_KEYS)
    b, f, h, w = depth.shape
    xy, _ = orc.pixel_grid((h, w), dtype=dtype)
    surfaces = orc.lift(xy, depth, k[:, :, None, None])
    idx = torch.arange(h * w) if indices is None else indices
    p = surfaces[:, 1:].reshape(b, f - 1, h * w, 3)[:, :, idx]
    where = (xy + bwd).reshape(b, f - 1, h * w, 2)[:, :, idx]
    q = orc.bilinear_border(surfaces[:, :-1], where)
    wt = wts.reshape(b, f - 1, h * w)[..., idx]
    rel = orc.rigid_fit(p, q, wt) if fit else relative_pose(ext)
    offset = orc.matvec(rel[:, :, None], orc.append_one(p))[..., :3] - q
    residual = (offset * offset).sum(-1)
    return {"offset": offset, "residual": residual, "loss": (wt * residual).sum(-1) / wt.sum(-1), "rel": rel}


def special_indices(shape, how):
    b, f, h, w, _ = shape
    if how is None:
        return None
    if how == "linspace":
        return torch.linspace(0, h * w - 1, min(1000, h * w // 2), dtype=torch.int64)
    points = {"three": 3, "fifty": 50, "tile+1": TILE + 1}[how]
    return torch.randint(0, h * w, (points,), generator=torch.Generator().manual_seed(5 + points), dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def oracle_case(shape, how, fit):
    """(inputs, indices, {dtype: terms}) of a shape the fixture does not hold, once.  With ``fit`` the inputs' extrinsics are the chain of
    the oracle's fp32 fit."""
    b, f, h, w, per_frame_k = shape
    x = inputs(2000 + f * h * w, b, f, h, w, per_frame_k)
    x = {"depth": x["depth"], "k": x["k"], "extrinsics": x["extrinsics"], "bwd": x["bwd"], "weights": x["bwd_mask"]}
    indices = special_indices(shape, how)
    terms = {dtype: oracle_terms(x, indices, dtype, fit) for dtype in (torch.float32, torch.float64)}
    if fit:
        x["extrinsics"] = orc.chain_poses(terms[torch.float32]["rel"])
    return x, indices, terms


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------


def problem(x, dev, lazy=True, weights="tensor"):
    """(module, batch, flows, model_output) over the inputs ``x``: lazy surfaces of the output's own depths (depth-sourced) or the explicit
    (b, f, h, w, 3) tensor (surface-sourced); ``weights``: "tensor", None, or ("logits", sensitivity) for a LazyWeights of x["weights"]."""
    from flowmap_amd import Batch, Flows, ModelOutput
    from flowmap_amd.model.extrinsics_procrustes import ExtrinsicsProcrustes, ExtrinsicsProcrustesCfg
    from flowmap_amd.model.projection import LazySurfaces, LazyWeights

    x = {key: v.to(dev) for key, v in x.items()}
    b, f, h, w = x["depth"].shape
    surfaces = LazySurfaces(x["depth"], x["k"])
    if not lazy:
        surfaces = surfaces.materialize()
    wts = x["weights"]
    if weights is None:
        wts = None
    elif weights != "tensor":
        wts = LazyWeights(x["weights"], weights[1])
    out = ModelOutput(x["depth"], surfaces, x["k"], x["extrinsics"], wts)
    flows = Flows(None, x["bwd"], None, None)
    module = ExtrinsicsProcrustes(ExtrinsicsProcrustesCfg("procrustes", 1000, False), f)
    return module, Batch(torch.zeros((b, f, 3, h, w), device=dev)), flows, out


def check_terms(r, truth, ref32, what, win=slice(None)):
    """The gate on offset, residual and pair_sum / pair_weight of an AlignmentResiduals; maps are compared flat over their elements."""
    worst = 0.0
    b, count = r.residual.shape[:2]
    for ours, name in ((r.offset.reshape(b, count, -1, 3), "offset"), (r.residual.reshape(b, count, -1), "residual"), (r.pair_loss(), "loss")):
        e, gap = assert_close_or_reference_gap(ours.cpu(), torch.as_tensor(truth[name])[:, win], torch.as_tensor(ref32[name])[:, win], rel=1e-4, slack=2.0,
                                               what=f"{what}.{name}")
        print(f"  {what}.{name}: rel err {e:.2e} (fp32 reference's own gap {gap:.2e})")
        worst = max(worst, e)
    return worst


def same_fields(a, b, what="", **kw):
    same_tensors(a, b, ("residual", "offset", "weight", "pair_sum", "pair_weight"), what, **kw)


# ---- case 1: reference parity --------------------------------------------------------------------------------------------------------------


def case_reference_parity(dev, case):
    """A fixture case through both sources, on every pixel with the given poses, on the case's indices with the given poses and with the
    reference's own fit (its fp32 extrinsics handed in): each inside the gate against the reference's fp64 run, and the two sources
    inside the gate of each other's truth."""
    g = golden()
    x = golden_inputs(case)
    indices = t(g[f"{case}_indices"])
    b, f, h, w = x["depth"].shape
    results = {}
    for lazy in (True, False):
        src = "depth" if lazy else "surfaces"
        module, batch, flows, out = problem(x, dev, lazy)
        r = module.residuals(batch, flows, out, offsets=True, weights=True)
        assert r.residual.shape == (b, f - 1, h, w) and r.offset.shape == (b, f - 1, h, w, 3) and r.weight.shape == (b, f - 1, h, w)
        assert r.pair_sum.shape == (b, f - 1) and r.pair_weight.shape == (b, f - 1) and r.first_pair == 0
        assert r.residual.dtype == torch.float32 and r.pair_sum.dtype == torch.float64 and not r.residual.requires_grad and not r.offset.requires_grad
        assert r.residual.device.type == torch.device(dev).type
        assert torch.equal(r.weight.cpu(), x["weights"])
        check_terms(r, *golden_terms(case, "dense"), f"{case}[{src}, dense]")
        ri = module.residuals(batch, flows, out, indices=indices.to(dev), offsets=True)
        assert ri.residual.shape == (b, f - 1, indices.numel()) and ri.offset.shape == (b, f - 1, indices.numel(), 3) and ri.weight is None
        check_terms(ri, *golden_terms(case, "given"), f"{case}[{src}, indices]")
        # the same elements as the dense maps at those pixels, bit for bit: one function per element
        assert torch.equal(ri.residual, r.residual.reshape(b, f - 1, h * w)[:, :, indices.to(dev)])
        module, batch, flows, out = problem({**x, "extrinsics": t(g[f"{case}_fit_extrinsics"])}, dev, lazy)
        rf = module.residuals(batch, flows, out, indices=indices.to(dev), offsets=True)
        check_terms(rf, *golden_terms(case, "fit"), f"{case}[{src}, the reference's fit]")
        results[lazy] = (r, ri, rf)
    for a, b_, route in zip(results[True], results[False], ("dense", "given", "fit")):
        truth, ref32 = golden_terms(case, route)
        for name in ("offset", "residual"):
            n = getattr(a, name).shape
            assert_close_or_reference_gap(getattr(a, name).cpu(), getattr(b_, name).cpu().double(), torch.as_tensor(ref32[name]).reshape(n), rel=1e-4, slack=2.0,
                                          what=f"{case}.{route}.{name}: depth-sourced vs surface-sourced")
    return results


def case_border(dev):
    """The fixture's border case: in a band along every side the flow pushes the sample out of the frame, at the corners on two sides at
    once — the border clamp decides q there.  The band alone passes the gate."""
    g = golden()
    x = golden_inputs("border")
    b, f, h, w = x["depth"].shape
    xy, _ = orc.pixel_grid((h, w))
    where = xy + x["bwd"]
    outside = ((where < 0) | (where > 1)).any(-1)  # (b, f-1, h, w)
    both = ((where < 0) | (where > 1)).all(-1)
    assert bool(outside[:, :, 0].all()) and bool(outside[:, :, -1].all()) and bool(outside[:, :, :, 0].all()) and bool(outside[:, :, :, -1].all())
    assert bool(both[:, :, 0, 0].all()) and bool(both[:, :, -1, -1].all()) and int(outside.sum()) < outside.numel()
    truth, ref32 = golden_terms("border", "dense")
    for lazy in (True, False):
        module, batch, flows, out = problem(x, dev, lazy)
        r = module.residuals(batch, flows, out, offsets=True)
        for name in ("offset", "residual"):
            ours = getattr(r, name).cpu()
            sel = outside if name == "residual" else outside[..., None].expand_as(ours)
            e, gap = assert_close_or_reference_gap(ours[sel], torch.as_tensor(truth[name]).reshape(ours.shape)[sel],
                                                   torch.as_tensor(ref32[name]).reshape(ours.shape)[sel], rel=1e-4, slack=2.0, what=f"border band.{name}")
            print(f"  border band ({'depth' if lazy else 'surfaces'}).{name}: rel err {e:.2e} (fp32 reference's own gap {gap:.2e})")
        assert bool(torch.isfinite(r.residual).all())


def case_oracle_parity(dev, shape, how, fit):
    """The shapes with several tiles per pair and with tile tails, and the index sets, against the oracle's fp64 evaluation."""
    x, indices, terms = oracle_case(shape, how, fit)
    for lazy in (True, False):
        module, batch, flows, out = problem(x, dev, lazy)
        r = module.residuals(batch, flows, out, indices=None if indices is None else indices.to(dev), offsets=True)
        check_terms(r, terms[torch.float64], terms[torch.float32], f"{'x'.join(map(str, shape[:4]))}[{how}, {'fit' if fit else 'given'}, {'depth' if lazy else 'surfaces'}]")


# ---- case 2: the convention, by a property of the fit ---------------------------------------------------------------------------------------


def _rotated(ext_rel, degrees=1.0, shift=0.01):
    """The relative poses with a rotation of ``degrees`` about each axis in turn applied and the translation shifted."""
    a = np.deg2rad(degrees)
    c, s = float(np.cos(a)), float(np.sin(a))
    rx = torch.tensor([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=torch.float64)
    ry = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
    rz = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float64)
    out = ext_rel.double().clone()
    out[..., :3, :3] = (rz @ ry @ rx) @ out[..., :3, :3]
    out[..., :3, 3] += shift
    return out.float()


def case_convention(dev, shape, how):
    """Poses from THIS package's align_surfaces on the same correspondences: Σ w·offset vanishes —
    ‖Σ w·offset‖ / (Σ w · √mean(residual)) <= 1e-4 per pair (measured on these shapes: 1e-8 … 1.2e-7 for the fit's pose and 0.09 … 0.49
    for small_poses, a pose that is not the fit's: the bound sits about three orders from either, so a swapped direction, an inverted T or the
    wrong frame's K fails it) — and pair_sum is strictly below pair_sum at that pose rotated by 1 degree about each axis and shifted by 0.01."""
    from flowmap_amd.model import projection as fm

    x, indices, _ = oracle_case(shape, how, False)
    for lazy in (True, False):
        module, batch, flows, out = problem(x, dev, lazy)
        h, w = out.depths.shape[2:]
        idx = (torch.arange(h * w) if indices is None else indices).to(dev)
        fitted = fm.align_surfaces(out.surfaces, flows.backward, out.backward_correspondence_weights, idx)
        assert getattr(fitted, "_fm_relative_poses", None) is not None
        out.extrinsics = fitted
        r = module.residuals(batch, flows, out, indices=None if indices is None else idx, offsets=True, weights=True)
        b, count = r.pair_sum.shape
        wt, off, res = r.weight.reshape(b, count, -1).double(), r.offset.reshape(b, count, -1, 3).double(), r.residual.reshape(b, count, -1).double()
        ratio = (wt[..., None] * off).sum(2).norm(dim=-1) / (wt.sum(2) * res.mean(2).sqrt())
        print(f"  weighted mean offset / rms, fit's pose ({'depth' if lazy else 'surfaces'}): {ratio.flatten().tolist()}")
        assert bool((ratio <= 1e-4).all()), f"Σ w·offset does not vanish at the fit's pose: {ratio.flatten().tolist()}"
        # a pose that is not the fit's: the inputs' small_poses
        module2, batch2, flows2, out2 = problem(x, dev, lazy)
        r2 = module2.residuals(batch2, flows2, out2, indices=None if indices is None else idx, offsets=True, weights=True)
        off2, res2 = r2.offset.reshape(b, count, -1, 3).double(), r2.residual.reshape(b, count, -1).double()
        ratio2 = (wt[..., None] * off2).sum(2).norm(dim=-1) / (wt.sum(2) * res2.mean(2).sqrt())
        print(f"  weighted mean offset / rms, small_poses: {ratio2.flatten().tolist()}")
        assert bool((ratio2 > 1e-2).all()), "the negative control passes the bound as well: the property decides nothing"
        # the fit's pose minimises the objective: a perturbed pose has the larger sum
        rel = fitted._fm_relative_poses[1].cpu()
        out.extrinsics = orc.chain_poses(_rotated(rel)).to(dev)
        worse = module.residuals(batch, flows, out, indices=None if indices is None else idx)
        assert bool((r.pair_sum < worse.pair_sum).all()), (r.pair_sum.tolist(), worse.pair_sum.tolist())


# ---- case 3: the sums ---------------------------------------------------------------------------------------------------------------------


def case_sums(dev, shape, how=None):
    """pair_sum / pair_weight against the fp64 sums of the RETURNED fp32 maps — the terms are the fp32 products the kernel converts,
    (double)(weight·residual), so the only difference is the order of the fp64 additions: |Δ| <= n · 2^-52 · Σ|terms|, n the elements per
    pair.  Three calls bit-equal; a window and a slice bit-equal, maps and sums, to the same pairs of the full call; without weights
    pair_weight is the element count exactly."""
    x, indices, _ = oracle_case(shape, how, False)
    module, batch, flows, out = problem(x, dev)
    idx = None if indices is None else indices.to(dev)
    kw = dict(indices=idx, offsets=True, weights=True)
    r = module.residuals(batch, flows, out, **kw)
    b, count = r.pair_sum.shape
    n = r.residual[0, 0].numel()
    terms = (r.weight * r.residual).double().reshape(b, count, -1)  # fp32 products, then exact
    want, mag = terms.sum(-1), terms.abs().sum(-1)
    err = (r.pair_sum - want).abs()
    assert bool((err <= n * 2.0**-52 * mag).all()), f"pair_sum: worst {float((err / mag.clamp_min(1e-300)).max()):.3e} relative, bound {n * 2.0**-52:.3e}"
    want_w = r.weight.double().reshape(b, count, -1).sum(-1)
    assert bool(((r.pair_weight - want_w).abs() <= n * 2.0**-52 * want_w).all()), "pair_weight"
    assert float(want.min()) > 0 and float(want_w.min()) > 0
    assert_close(r.pair_loss(), r.pair_sum / r.pair_weight, 1e-15, what="pair_loss")
    for _ in range(2):
        same_fields(module.residuals(batch, flows, out, **kw), r, "repeat: ")
    if count >= 3:
        win = module.residuals(batch, flows, out, pairs=(1, 2), **kw)
        assert win.first_pair == 1 and win.residual.shape[:2] == (b, 2) and win.pair_sum.shape == (b, 2)
        part = type(r)(*(v[:, 1:3] for v in (r.residual, r.offset, r.weight, r.pair_sum, r.pair_weight)), 1)
        same_fields(win, part, "window (1, 2): ")
        same_fields(module.residuals(batch, flows, out, pairs=slice(1, 3), **kw), win, "slice(1, 3): ")
    bare = module.residuals(batch, flows, out, indices=idx, sums=False)  # what was not asked for is not produced
    assert bare.pair_sum is None and bare.pair_weight is None and bare.offset is None and bare.weight is None
    assert torch.equal(bare.residual, r.residual)
    module_n, batch_n, flows_n, out_n = problem(x, dev, weights=None)
    plain = module_n.residuals(batch_n, flows_n, out_n, indices=idx, weights=True)
    assert torch.equal(plain.pair_weight, torch.full((b, count), float(n), dtype=torch.float64, device=plain.pair_weight.device))
    assert torch.equal(plain.weight, torch.ones_like(plain.weight)) and torch.equal(plain.residual, r.residual)
    terms = plain.residual.double().reshape(b, count, -1)
    assert bool(((plain.pair_sum - terms.sum(-1)).abs() <= n * 2.0**-52 * terms.sum(-1)).all()), "pair_sum without weights"


# ---- case 4: lazy weights -----------------------------------------------------------------------------------------------------------------


def case_lazy_weights(dev, shape, how=None, sensitivity=100.0):
    """A LazyWeights of logits: the ``weight`` map is torch.sigmoid(sens·logits) inside the gate (the fp64 sigmoid is the truth, torch's
    fp32 one the reference evaluation), residual and offset are bit-equal to the plain-tensor call, and nothing was evaluated on the
    LazyWeights."""
    x, indices, _ = oracle_case(shape, how, False)
    g = torch.Generator().manual_seed(3)
    logits = 0.03 * torch.randn(x["weights"].shape, generator=g)
    idx = None if indices is None else indices.to(dev)
    module, batch, flows, out = problem({**x, "weights": logits}, dev, weights=("logits", sensitivity))
    r = module.residuals(batch, flows, out, indices=idx, offsets=True, weights=True)
    assert out.backward_correspondence_weights._dense is None, "the LazyWeights was evaluated"
    b, f, h, w = x["depth"].shape
    sel = (lambda m: m) if indices is None else (lambda m: m.reshape(b, f - 1, h * w)[:, :, indices])
    e, gap = assert_close_or_reference_gap(r.weight.cpu(), sel(torch.sigmoid(sensitivity * logits.double())), sel(torch.sigmoid(sensitivity * logits)), rel=1e-4,
                                           slack=2.0, what="weight map of lazy logits")
    print(f"  lazy weights: rel err {e:.2e} (torch's fp32 sigmoid: {gap:.2e})")
    assert float(r.weight.min()) < 0.2 and float(r.weight.max()) > 0.8  # (the logits really spread the weights)
    module_p, batch_p, flows_p, out_p = problem(x, dev)
    plain = module_p.residuals(batch_p, flows_p, out_p, indices=idx, offsets=True)
    assert torch.equal(plain.residual, r.residual) and torch.equal(plain.offset, r.offset)
    terms = (r.weight * r.residual).double().reshape(b, f - 1, -1)
    n = terms.shape[-1]
    assert bool(((r.pair_sum - terms.sum(-1)).abs() <= n * 2.0**-52 * terms.sum(-1)).all()), "pair_sum uses the weights it returns"


# ---- case 5: it leaves training alone --------------------------------------------------------------------------------------------------------


def _train(dev, tracking, calls, fuse, steps=5):
    """operator_checks.train, 5 steps from step 0 after the warm-up; ``calls``: ExtrinsicsProcrustes.residuals between forward and backward
    (a window on the fit's own indices, with offsets and weights) and again between the steps.  -> (the record, the PoseChain evaluations
    of the run and whether the fit was asked for chained poses: ``_fm_extrinsics_wanted`` on the backward flows)."""
    from flowmap_amd import _ops
    from flowmap_amd.model.extrinsics_procrustes import procrustes_indices

    chain_calls = [0]
    chain = _ops.PoseChain.apply

    def counted_chain(rel):
        chain_calls[0] += 1
        return chain(rel)

    def mid(ns):
        own = procrustes_indices(HEIGHT, WIDTH, ns.model.extrinsics.cfg.num_points, False, torch.device(dev))
        return ns.model.extrinsics.residuals(ns.batch, ns.flows, ns.out, pairs=(1, 2), indices=own, offsets=True, weights=True)

    after = lambda ns: ns.model.extrinsics.residuals(ns.batch, ns.flows, ns.out)  # noqa: E731
    flows = []
    _ops.PoseChain.apply = staticmethod(counted_chain)
    try:
        run = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=0, warm_up=True, calls=(mid, after) if calls else None,
                    prepare=lambda ns: flows.append(ns.flows))
    finally:
        _ops.PoseChain.apply = staticmethod(chain)
    return run, {"wanted": bool(flows[0].backward.__dict__.get("_fm_extrinsics_wanted", False)), "chain_calls": chain_calls[0]}


def case_training_untouched(dev, tracking, fuse):
    """A flow (+ tracking, tap exchange on) run with FusedAdam (``fuse``: FusedAdam.fuse_depth_update), with and without two residuals()
    calls per step: operator_checks.assert_training_untouched with ``alignment_residuals`` the one counter that differs, no pose chain was
    evaluated for the calls, and a flow-only step does hand out a LazyExtrinsics for the shared check to find unevaluated after a call."""
    steps = 5
    plain, chained = _train(dev, tracking, calls=False, fuse=fuse, steps=steps)
    with_calls, chained_with_calls = _train(dev, tracking, calls=True, fuse=fuse, steps=steps)
    _, base = assert_training_untouched(plain, with_calls, "alignment_residuals", 2 * steps)
    assert chained_with_calls == chained, (chained_with_calls, chained)
    if not tracking:
        assert chained["chain_calls"] == 0 and not chained["wanted"]  # a flow-only run never chains the poses, with the calls neither
        assert any(was for was, _ in with_calls.lazy_kept) and all(after for was, after in with_calls.lazy_kept if was), "a LazyExtrinsics was evaluated by residuals()"
    else:
        assert base["flow_tap_passes"] > 0  # the tap exchange really ran
    for r in with_calls.seen:
        assert bool(torch.isfinite(r.residual).all()) and bool(torch.isfinite(r.pair_sum).all())
    first, second = with_calls.seen[0], with_calls.seen[1]
    assert first.first_pair == 1 and first.residual.shape == (1, 2, 60) and first.offset.shape == (1, 2, 60, 3) and second.residual.shape == (1, 4, 24, 32)


# ---- case 6: arguments ---------------------------------------------------------------------------------------------------------------------


def case_arguments(dev):
    import pytest

    from flowmap_amd import _ops
    from flowmap_amd.model import projection as fm

    x = {key: v.to(dev) for key, v in golden_inputs("b").items()}
    module, batch, flows, out = problem(x, dev)
    for bad in (slice(0, 4, 2), (0, 0), (3, 2), (-1, 2), (0, 5), "all", 1, (1.0, 2), (0, 1, 2), slice(3, 1)):
        with pytest.raises(ValueError, match="flowmap_amd: alignment_residuals"):
            module.residuals(batch, flows, out, pairs=bad)
    assert module.residuals(batch, flows, out, pairs=slice(None)).residual.shape[1] == 4
    assert module.residuals(batch, flows, out, pairs=slice(-2, None)).first_pair == 2
    assert module.residuals(batch, flows, out, pairs=[3, 1]).residual.shape[1] == 1
    idx = torch.tensor([0, 5, 390], device=dev)
    few = module.residuals(batch, flows, out, indices=idx[:2], weights=True)  # fewer than 3 points: nothing is solved
    assert few.residual.shape == (1, 4, 2) and few.weight.shape == (1, 4, 2) and few.offset is None
    before = _ops.counters["alignment_residuals"]
    direct = fm.alignment_residuals(out.surfaces, flows.backward, out.backward_correspondence_weights, out.extrinsics, indices=idx, pairs=(1, 2))
    assert _ops.counters["alignment_residuals"] == before + 1
    assert torch.equal(direct.residual, module.residuals(batch, flows, out, indices=idx, pairs=(1, 2)).residual)
    for tensor in (x["depth"], x["k"], x["bwd"], x["weights"], x["extrinsics"], idx):
        assert not [key for key in tensor.__dict__ if key.startswith("_fm_")], "a note was left on an argument"

    def refused(match, **changed):
        kw = changed.pop("kw", {})
        module_, batch_, flows_, out_ = problem({**x, **changed}, dev)
        with pytest.raises(RuntimeError, match=match):
            module_.residuals(batch_, flows_, out_, **kw)

    refused("flowmap_amd: alignment_residuals: indices must be an int64 tensor", kw={"indices": idx.int()})
    refused("flowmap_amd: alignment_residuals: indices must be an int64 tensor", kw={"indices": [0, 1, 2]})
    refused("flowmap_amd: alignment_residuals: indices must be a non-empty 1-D tensor", kw={"indices": idx[:0]})
    refused("flowmap_amd: alignment_residuals: indices must be a non-empty 1-D tensor", kw={"indices": idx[None]})
    if torch.device(dev).type != "cpu":
        refused("flowmap_amd: alignment_residuals: indices are on cpu", kw={"indices": idx.cpu()})
    refused("flowmap_amd: alignment_residuals: backward_flows of shape .* do not match the depths", bwd=x["bwd"][:, :, :-1])
    refused("flowmap_amd: alignment_residuals: backward_flows of shape .* do not match the depths", bwd=x["bwd"][:, :-1])
    refused("flowmap_amd: alignment_residuals: backward_weights of shape .* do not match the depths", weights=x["weights"][:, :-1])
    refused("flowmap_amd: alignment_residuals: extrinsics of shape .* do not match the depths", extrinsics=torch.cat((x["extrinsics"], x["extrinsics"][:, :1]), 1))
    refused("flowmap_amd: depth must be float32", depth=x["depth"].double())
    refused("flowmap_amd: backward flow must be float32", bwd=x["bwd"].double())
    r = module.residuals(batch, flows, out, sums=False)
    assert r.pair_sum is None and r.pair_weight is None and r.offset is None and r.weight is None
    assert r.residual.dtype == torch.float32 and r.residual.device == x["depth"].device and not r.residual.requires_grad
    with pytest.raises(RuntimeError, match="needs the sums"):
        r.pair_loss()
    # gradients recorded around the call change nothing: the outputs never require one
    depth = x["depth"].clone().requires_grad_(True)
    module_, batch_, flows_, out_ = problem({**x, "depth": depth}, dev)
    rg = module_.residuals(batch_, flows_, out_, offsets=True, weights=True)
    assert not any(v.requires_grad for v in (rg.residual, rg.offset, rg.weight, rg.pair_sum, rg.pair_weight))


def case_host_tensor_refused():
    """Without the test double, host tensors are refused by name — on both sources, through the method and through the function."""
    import pytest

    from flowmap_amd import _lib
    from flowmap_amd.model import projection as fm

    from helpers import build_host_sim

    for lazy in (True, False):
        _lib.set_library_for_testing(build_host_sim())  # (the explicit surfaces tensor of the host problem is made by the double)
        module, batch, flows, out = problem(golden_inputs("a"), "cpu", lazy=lazy)
        _lib.set_library_for_testing(None)
        with pytest.raises(RuntimeError, match="flowmap_amd: alignment_residuals: tensors are on cpu.*no CPU fallback"):
            module.residuals(batch, flows, out)
        with pytest.raises(RuntimeError, match="flowmap_amd: alignment_residuals: tensors are on cpu"):
            fm.alignment_residuals(out.surfaces, flows.backward, out.backward_correspondence_weights, out.extrinsics)


# ---- case 7: the GPU against the host double ----------------------------------------------------------------------------------------------


def case_gpu_against_host_double(dev, case):
    """The same fixture through the HIP kernel and through the serial host build of the same functions: element for element.  Bit-equality
    is not required (the device contracts multiply-adds the host build, compiled with contraction off, does not): both sit inside the gate,
    the largest ulp distance is printed."""
    from flowmap_amd import _lib
    from helpers import build_host_sim

    x = golden_inputs(case)
    worst = {}
    for lazy in (True, False):
        module, batch, flows, out = problem(x, dev, lazy)
        gpu = module.residuals(batch, flows, out, offsets=True, weights=True)
        _lib.set_library_for_testing(build_host_sim())
        try:
            module_h, batch_h, flows_h, out_h = problem(x, "cpu", lazy)
            host = module_h.residuals(batch_h, flows_h, out_h, offsets=True, weights=True)
        finally:
            _lib.set_library_for_testing(None)
        truth, ref32 = golden_terms(case, "dense")
        src = "depth" if lazy else "surfaces"
        check_terms(gpu, truth, ref32, f"gpu {case}[{src}]")
        check_terms(host, truth, ref32, f"host {case}[{src}]")
        assert torch.equal(gpu.weight.cpu(), host.weight)
        assert_close(gpu.pair_weight.cpu(), host.pair_weight, 1e-12, what="pair_weight")
        worst[src] = {name: ulp_distance(getattr(gpu, name).cpu(), getattr(host, name)) for name in ("residual", "offset")}
    print(f"  GPU vs host double, {case}: max ulp distance {worst}")
    return worst
