"""projection.depth_consistency / Model.consistency (fm_depth_consistency): per source pixel and frame offset d the relative error of frame
i+d's depth, sampled where the pixel reprojects under the chained poses, against the depth the reprojection predicts — with its code,
optionally uv / q.z / the sample, the per-pixel support under a tolerance and per-(frame, offset) fp64 sums.  The cases here take a
device; tests/test_hostsim_depth_consistency.py runs them on the serial host double of the C ABI, tests/test_gpu_depth_consistency.py on
the MI355X.

Truths.  tests/golden/fn_depth_consistency.npz holds what the REFERENCE computes (tools/make_golden_depth_consistency.py: its own
unproject, homogenize_points, transform_rigid, project_camera_space, sample_image_grid and F.grid_sample) in fp32 and in fp64, for the
shapes small enough to commit (``odd`` keeps error and sampled only: every field of it would be 560 KB); at every shape the same two
evaluations come from the oracle (oracle/flowmap_oracle.py: lift, matvec, pinhole, bilinear_border — restated in oracle_consistency
below), computed once per case.  The gate is the project's: conftest.assert_close_or_reference_gap, rel 1e-4, slack 2x the fp32
evaluation's own gap to fp64, norm-wise over the elements with code == 0, on error, positions, reprojected and sampled.

``code`` is a decision: ours may differ from the fp64 truth's only where an fp64 uv coordinate lies within 1e-5 of 0 or 1 or |q.z| < 1e-5;
such elements may number at most 0.1 % of a case's and are left out of the value comparison.

Inputs: oracle.synth_scene — the noisy ``depth_init`` (on the ground-truth depth the numerator of ``error`` cancels to 1e-4 of its terms),
its ground-truth poses and K; ``edge`` is hand-built (a rotation by pi, two translations) so that every code occurs.

Cases (batch, frames, h, w); a workgroup owns T = 1024 consecutive pixels of one (batch entry, source frame): see SPECS.
"""

from __future__ import annotations

import functools
import math

import torch

from conftest import assert_close_or_reference_gap, load_golden, relerr, t
from operator_checks import assert_training_untouched, c_entry_refuses, gate_pair, host_tensor_refused, same_tensors, train, ulp_distance, window_rows
from oracle import flowmap_oracle as orc

T = 1024  # pixels per workgroup (fm_residual_args.h: kDepthConsTile)
PM3 = (-3, -2, -1, 1, 2, 3)
# name -> ((batch, frames, h, w), seeds per batch entry, offsets)
SPECS = {
    "tiny": ((1, 2, 5, 7), (41,), (-1, 1)),  # fewer pixels than a wavefront; every frame misses one neighbour (code 1)
    "odd": ((1, 6, 17, 23), (42,), PM3),  # odd width: the scalar path with a partial last quad
    "eight": ((1, 6, 17, 23), (42,), (-4, -3, -2, -1, 1, 2, 3, 4)),  # the most offsets one call takes
    "vec": ((1, 7, 24, 32), (43,), PM3),  # the 16-byte path with less than one tile
    "wide": ((1, 5, 64, 128), (44,), PM3),  # several whole tiles
    "tile": ((1, 3, 1, T), (48,), (-1, 1)),  # exactly one tile (16-byte path)
    "tile1": ((1, 3, 1, T + 1), (49,), (-1, 1)),  # one pixel past a tile: a second workgroup with one live thread (scalar path)
    "two": ((2, 4, 9, 12), (45, 145), (-2, -1, 1, 2)),  # two batch entries with different poses
    "edge": ((1, 4, 9, 12), (47,), PM3),  # hand-built: codes 1, 2 and 3 at nearly every offset
}
GOLDEN_CASES = ("tiny", "odd", "two", "edge")  # (the others are generated from the seed: their fixtures would not fit the size limit)
FIELDS = ("error", "positions", "reprojected", "sampled")
GOLDEN_FIELDS = {"odd": ("error", "sampled")}
INPUT_KEYS = ("depth", "k", "ext")


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """depth (b, F, h, w), k (b, F, 3, 3), ext (b, F, 4, 4) of a case (tools/make_golden_depth_consistency.py draws them from here)."""
    (b, f, h, w), seeds, _ = SPECS[name]
    if name == "edge":
        depth = 1.5 + torch.rand((1, f, h, w), generator=torch.Generator().manual_seed(seeds[0]))
        k = orc.focal_to_k(torch.tensor(0.85), (h, w)).expand(1, f, 3, 3).contiguous()
        ext = torch.eye(4).repeat(1, f, 1, 1)
        ext[0, 1, 0, 0] = ext[0, 1, 2, 2] = -1.0  # a rotation by pi about y at the origin
        ext[0, 2, :3, 3] = torch.tensor([1.0, 0.0, 0.0])
        ext[0, 3, :3, 3] = torch.tensor([0.0, -0.7, 0.3])
        return {"depth": depth, "k": k, "ext": ext}
    scenes = [orc.synth_scene(f, h, w, seed=seed) for seed in seeds]
    return {"depth": torch.stack([s["depth_init"] for s in scenes]), "k": torch.stack([s["intrinsics_gt"].expand(f, 3, 3) for s in scenes]).contiguous(),
            "ext": torch.stack([s["extrinsics_gt"] for s in scenes])}


def windows_of(frames):
    """Every frame, the first alone, the last alone, and a middle slice whose targets lie outside the window."""
    if frames <= 2:
        return [None, (0, 1), (frames - 1, 1)]
    return [None, (0, 1), (frames - 1, 1), slice(1, max(2, frames - 1))]


# ---- the oracle's composition ----------------------------------------------------------------------------------------------------------------


def oracle_consistency(x, offsets, dtype):
    """error, code, positions, reprojected, sampled of EVERY frame, (b, F, n_off, h, w[, 2]), by the oracle in ``dtype``."""
    depth, k, ext = (x[key].to(dtype) for key in INPUT_KEYS)
    b, f, h, w = depth.shape
    xy, _ = orc.pixel_grid((h, w), dtype=dtype)
    maps = (b, f, len(offsets), h, w)
    out = {"error": torch.zeros(maps, dtype=dtype), "code": torch.ones(maps, dtype=torch.uint8), "positions": torch.zeros((*maps, 2), dtype=dtype),
           "reprojected": torch.zeros(maps, dtype=dtype), "sampled": torch.zeros(maps, dtype=dtype)}
    for o, d in enumerate(offsets):
        src = [i for i in range(f) if 0 <= i + d < f]
        if not src:
            continue
        dst = [i + d for i in src]
        n = len(src)
        p = orc.lift(xy, depth[:, src], k[:, src][:, :, None, None])
        rel = torch.linalg.inv(ext[:, dst]) @ ext[:, src]
        q = orc.matvec(rel[:, :, None, None], orc.append_one(p))[..., :3]
        uv = orc.pinhole(q, k[:, dst][:, :, None, None])
        zs = orc.bilinear_border(depth[:, dst][..., None], uv.reshape(b, n, h * w, 2)).reshape(b, n, h, w)
        qz = q[..., 2]
        inside = (uv >= 0).all(-1) & (uv < 1).all(-1)
        code = torch.where(~(qz > 0), 2, torch.where(inside, 0, 3)).to(torch.uint8)
        out["code"][:, src, o] = code
        out["error"][:, src, o] = torch.where(code == 0, (zs - qz) / qz, torch.zeros_like(qz))
        out["positions"][:, src, o], out["reprojected"][:, src, o], out["sampled"][:, src, o] = uv, qz, zs
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    return {dtype: oracle_consistency(case_inputs(name), SPECS[name][2], dtype) for dtype in (torch.float32, torch.float64)}


def admitted(truth):
    """Where ``code`` may differ from the fp64 truth's: an fp64 uv coordinate within 1e-5 of 0 or 1, or |q.z| < 1e-5 (never a missing frame)."""
    uv, qz = truth["positions"], truth["reprojected"]
    near = ((uv.abs() < 1e-5) | ((uv - 1).abs() < 1e-5)).any(-1) | (qz.abs() < 1e-5)
    return near & (truth["code"] != 1)


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------


def check_code(r, truth, what, rows=slice(None)):
    """The condition on ``code`` -> the bool map of elements the values are compared on (truth's code 0, not admitted)."""
    want, may = truth["code"][:, rows], admitted(truth)[:, rows]
    ours = r.code.cpu()
    assert ours.dtype == torch.uint8 and tuple(ours.shape) == tuple(want.shape), f"{what}.code: {ours.dtype} {tuple(ours.shape)} vs {tuple(want.shape)}"
    wrong = (ours != want) & ~may
    assert not bool(wrong.any()), f"{what}.code: {int(wrong.sum())} elements differ from the fp64 truth away from every boundary"
    assert int(may.sum()) <= 1e-3 * may.numel(), f"{what}: {int(may.sum())} of {may.numel()} elements lie on a boundary: a badly conditioned case"
    assert bool((r.error.cpu()[ours != 0] == 0).all()), f"{what}.error is not exactly 0 where code != 0"
    return (want == 0) & ~may & (ours == 0)


def check_fields(r, truth, ref32, what, rows=slice(None), fields=FIELDS, code_truth=None):
    """The gate on the fields of a DepthConsistency against (truth, ref32) restricted to the source frames ``rows``."""
    sel = check_code(r, code_truth or truth, what, rows)
    assert int(sel.sum()) > 0 or what.startswith("tile"), f"{what}: no element with code 0"
    worst = {}
    for name in fields:
        ours = getattr(r, name)
        if ours is None:
            continue
        tr, rf = torch.as_tensor(truth[name])[:, rows], torch.as_tensor(ref32[name])[:, rows]
        assert tuple(ours.shape) == tuple(tr.shape) and ours.dtype == torch.float32, f"{what}.{name}: shape {tuple(ours.shape)} vs {tuple(tr.shape)}"
        e, gap = assert_close_or_reference_gap(ours.cpu()[sel], tr[sel], rf[sel], rel=1e-4, slack=2.0, what=f"{what}.{name}")
        print(f"  {what}.{name}: err {e:.2e} (fp32 reference's own gap {gap:.2e}) over {int(sel.sum())} elements")
        worst[name] = e
    return worst


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------


def run(name, dev, x=None, **kw):
    import flowmap_amd

    x = {key: v.clone().to(dev) for key, v in (x or case_inputs(name)).items()}
    kw.setdefault("offsets", SPECS[name][2])
    return flowmap_amd.depth_consistency(x["depth"], x["k"], x["ext"], **kw)


MAPS = ("error", "code", "positions", "reprojected", "sampled", "support", "frame_sum", "frame_valid")


def same_fields(a, b, what="", **kw):
    same_tensors(a, b, MAPS, what, **kw)


def check_layout(r, name, dev, count=None, first=0, details=True, tolerance=True, sums=True):
    (b, f, h, w), _, offsets = SPECS[name]
    count = f if count is None else count
    maps = (b, count, len(offsets), h, w)
    assert (r.first_frame, r.offsets) == (first, tuple(offsets))
    assert r.error.shape == maps and r.error.dtype == torch.float32 and r.code.shape == maps and r.code.dtype == torch.uint8
    if details:
        assert r.positions.shape == (*maps, 2) and r.reprojected.shape == maps and r.sampled.shape == maps
    else:
        assert r.positions is None and r.reprojected is None and r.sampled is None
    assert (r.support.shape == (b, count, h, w) and r.support.dtype == torch.uint8) if tolerance else r.support is None
    if sums:
        assert r.frame_sum.shape == (b, count, len(offsets)) and r.frame_sum.dtype == torch.float64 and r.frame_valid.shape == r.frame_sum.shape
    else:
        assert r.frame_sum is None and r.frame_valid is None
    for name_ in MAPS:
        v = getattr(r, name_)
        assert v is None or (not v.requires_grad and v.device.type == torch.device(dev).type)


# ---- check 1: reference and oracle parity, every window ---------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("fn_depth_consistency")


def golden_inputs(name):
    return {key: t(golden()[f"{name}_{key}"]) for key in INPUT_KEYS}


def case_reference_parity(dev, name):
    """A fixture case against what the imported reference computes, fp64 the truth, fp32 the reference evaluation, on every window."""
    g = golden()
    x = golden_inputs(name)  # the inputs the fixture was made from (a scene drawn on another machine differs in the last bits of sin / cos)
    for key in INPUT_KEYS:
        assert relerr(case_inputs(name)[key], x[key]) < 1e-6, f"{name}: the fixture's {key} is not the case's"
    assert tuple(int(d) for d in g[f"{name}_offsets"]) == tuple(SPECS[name][2])
    fields = GOLDEN_FIELDS.get(name, FIELDS)
    truth = {key: t(g[f"{name}_f64_{key}"]) for key in fields + ("code",)}
    ref32 = {key: t(g[f"{name}_{key}"]) for key in fields + ("code",)}
    assert truth["code"].dtype == torch.uint8 and torch.equal(truth["code"], ref32["code"])  # (the generator asserted it)
    oracle64 = oracle_consistency(x, SPECS[name][2], torch.float64)  # (uv and q.z in fp64 of every element: where ``code`` may differ)
    assert torch.equal(truth["code"], oracle64["code"]), "the reference and the oracle decide alike in fp64"
    f = SPECS[name][0][1]
    for window in windows_of(f):
        r = run(name, dev, x=x, frames=window, details=True, tolerance=0.05)
        rows = window_rows(window, f)
        check_layout(r, name, dev, count=rows.stop - rows.start, first=rows.start)
        check_fields(r, truth, ref32, f"{name}[{window}] vs the reference", rows=rows, fields=fields, code_truth=oracle64)


def case_oracle_parity(dev, name):
    terms = oracle_case(name)
    f = SPECS[name][0][1]
    full = None
    for window in windows_of(f):
        r = run(name, dev, frames=window, details=True)
        rows = window_rows(window, f)
        check_layout(r, name, dev, count=rows.stop - rows.start, first=rows.start, tolerance=False)
        check_fields(r, terms[torch.float64], terms[torch.float32], f"{name}[{window}]", rows=rows)
        full = r if window is None else full
    codes = set(full.code.unique().tolist())
    if name == "tiny":
        assert bool((full.code[:, 0, 0] == 1).all()) and bool((full.code[:, 1, 1] == 1).all()) and 0 in codes
    if name == "edge":
        assert codes == {0, 1, 2, 3}, f"edge: codes {codes}"
        for o, d in enumerate(SPECS[name][2]):
            if abs(d) <= 2:
                assert set(full.code[:, :, o].unique().tolist()) == {0, 1, 2, 3}, f"edge: offset {d}"
    # the quantity separates a consistent reconstruction from the noisy one: the mean |error| per (frame, offset)
    print(f"  {name}: mean |error| per offset {[round(float(v), 5) for v in (full.frame_sum.sum((0, 1)) / full.frame_valid.sum((0, 1)).clamp_min(1))]}")
    return full


def case_generator_precondition(name):
    """What the issue states of the inputs: the oracle's own fp32 and fp64 evaluations disagree on no element's code."""
    terms = oracle_case(name)
    assert torch.equal(terms[torch.float32]["code"], terms[torch.float64]["code"])


# ---- check 2: the flow residuals' route to the same positions --------------------------------------------------------------------------------


def case_flow_cross_check(dev, name):
    """positions − xy at d = +1 / −1 against forward_flow / backward_flow of LossFlow.residuals(predicted_flow=True) on the same model output."""
    from flowmap_amd import Batch, Flows, ModelOutput
    from flowmap_amd.loss import LossFlow, LossFlowCfg
    from flowmap_amd.model.projection import LazySurfaces, sample_image_grid
    from helpers import mapping_cfg

    (b, f, h, w), _, offsets = SPECS[name]
    x = {key: v.clone().to(dev) for key, v in case_inputs(name).items()}
    out = ModelOutput(x["depth"], LazySurfaces(x["depth"], x["k"]), x["k"], x["ext"], None)
    zeros = torch.zeros((b, f - 1, h, w, 2), device=dev)
    flows = Flows(zeros, zeros, torch.ones((b, f - 1, h, w), device=dev), torch.ones((b, f - 1, h, w), device=dev))
    res = LossFlow(LossFlowCfg(0, 1.0, "flow", mapping_cfg("huber"))).residuals(Batch(torch.zeros((b, f, 3, h, w), device=dev)), flows, out, predicted_flow=True)
    from flowmap_amd.model.model import Model

    r = Model.consistency(None, out, offsets=offsets, details=True)
    xy = sample_image_grid((h, w), dev)[0]
    terms = oracle_case(name)
    xy64 = orc.pixel_grid((h, w), dtype=torch.float64)[0]
    for d, flow, src in ((1, res.forward_flow, slice(0, f - 1)), (-1, res.backward_flow, slice(1, f))):
        o = offsets.index(d)
        sel = (r.code[:, src, o] == 0).cpu()
        ours = (r.positions[:, src, o] - xy).cpu()[sel]
        gap = relerr((terms[torch.float32]["positions"][:, src, o] - xy.cpu())[sel], (terms[torch.float64]["positions"][:, src, o] - xy64)[sel])
        e = gate_pair(ours, flow.cpu()[sel], gap, f"{name}: positions - xy at d = {d} vs LossFlow.residuals")
        print(f"  {name}: d = {d}: rel err {e:.2e} against the flow residuals' route (fp32 gap {gap:.2e})")


# ---- check 3 and 4: windows, reproducibility, derived outputs ---------------------------------------------------------------------------------


def case_reproducible(dev, name):
    (b, f, h, w), _, offsets = SPECS[name]
    kw = dict(details=True, tolerance=0.02)
    full = run(name, dev, **kw)
    same_fields(run(name, dev, **kw), full, "repeat: ")
    for i in range(f):
        same_fields(run(name, dev, frames=(i, 1), **kw), full, f"window ({i}, 1): ", rows=slice(i, i + 1))
    if f > 2:
        same_fields(run(name, dev, frames=slice(1, f - 1), **kw), full, "middle window: ", rows=slice(1, f - 1))
    if b > 1:  # batch entry 0 alone against the batch
        alone = run(name, dev, x={key: v[:1] for key, v in case_inputs(name).items()}, **kw)
        for key in MAPS:
            assert torch.equal(getattr(alone, key), getattr(full, key)[:1]), f"batch entry 0 alone: {key}"
    bare = run(name, dev, sums=False)  # what was not asked for is not produced
    check_layout(bare, name, dev, details=False, tolerance=False, sums=False)
    assert torch.equal(bare.error, full.error) and torch.equal(bare.code, full.code)
    # derived outputs
    ok = full.code == 0
    assert torch.equal(full.support, (ok & (full.error.abs() <= 0.02)).sum(dim=2).to(torch.uint8)), "support"
    assert 0 < int(full.support.sum()) and int((full.support < ok.sum(dim=2)).sum()) > 0 or name.startswith("tile"), "the tolerance decides nothing here"
    assert torch.equal(full.frame_valid, ok.sum(dim=(3, 4)).double()), "frame_valid"
    want = torch.where(ok, full.error.abs(), torch.zeros_like(full.error)).double().sum(dim=(3, 4))
    err = (full.frame_sum - want).abs()
    assert bool((err <= h * w * 2.0**-52 * want).all()), f"frame_sum: worst {float((err / want.clamp_min(1e-300)).max()):.3e} relative, bound {h * w * 2.0**-52:.3e}"
    assert torch.equal(full.frame_error(), full.frame_sum / torch.where(full.frame_valid != 0, full.frame_valid, torch.ones_like(full.frame_valid)))
    zero = run(name, dev, tolerance=0.0)
    assert torch.equal(zero.support, (ok & (full.error == 0)).sum(dim=2).to(torch.uint8))


# ---- check 5: the GPU against the host double --------------------------------------------------------------------------------------------------


def case_gpu_against_host_double(dev, name):
    from flowmap_amd import _lib
    from helpers import build_host_sim

    gpu = run(name, dev, details=True)
    _lib.set_library_for_testing(build_host_sim())
    try:
        host = run(name, "cpu", details=True)
    finally:
        _lib.set_library_for_testing(None)
    terms = oracle_case(name)
    check_fields(gpu, terms[torch.float64], terms[torch.float32], f"gpu {name}")
    check_fields(host, terms[torch.float64], terms[torch.float32], f"host {name}")
    differ = (gpu.code.cpu() != host.code) & ~admitted(terms[torch.float64])
    assert not bool(differ.any()), f"{name}: code differs between the GPU and the host double away from every boundary"
    sel = (gpu.code.cpu() == 0) & (host.code == 0)
    worst = {key: ulp_distance(getattr(gpu, key).cpu()[sel], getattr(host, key)[sel]) for key in ("error", "reprojected", "sampled")}
    print(f"  GPU vs host double, {name}: max ulp distance in fp32 {worst}")
    return worst


# ---- check 6: refused arguments ----------------------------------------------------------------------------------------------------------------


def case_arguments(dev):
    import pytest

    import flowmap_amd
    from flowmap_amd import DepthConsistency, _ops
    from flowmap_amd.model import projection as fm

    name = "odd"
    x = {key: v.clone().to(dev) for key, v in case_inputs(name).items()}
    call = lambda **kw: fm.depth_consistency(x["depth"], x["k"], x["ext"], **kw)  # noqa: E731
    for bad in ((0,), (1, 0), (1, 1), (), tuple(range(1, 6)) + tuple(range(-4, 0)), (6,), (-6,), (1, -7), 1, (1.0,), None, "1"):
        with pytest.raises(ValueError, match="flowmap_amd: depth_consistency: .*offsets"):
            call(offsets=bad)
    for bad in (slice(0, 4, 2), (0, 0), (5, 2), (-1, 2), (0, 7), "all", 1, (1.0, 2), (0, 1, 2), slice(3, 1)):
        with pytest.raises(ValueError, match="flowmap_amd: depth_consistency.*frames"):
            call(frames=bad)
    for bad in (-1e-3, float("nan"), -1):
        with pytest.raises(ValueError, match="flowmap_amd: depth_consistency: tolerance"):
            call(tolerance=bad)
    assert call(frames=slice(None)).error.shape[1] == 6 and call(frames=slice(-2, None)).first_frame == 4 and call(frames=[3, 1]).error.shape[1] == 1
    assert call(offsets=[5, -5]).offsets == (5, -5) and isinstance(call(), DepthConsistency) and call().offsets == (-1, 1)
    assert flowmap_amd.depth_consistency is fm.depth_consistency

    def refused(match, **changed):
        y = {**x, **changed}
        with pytest.raises(RuntimeError, match=match):
            fm.depth_consistency(y["depth"], y["k"], y["ext"])

    refused("flowmap_amd: depth_consistency: depths must be float32", depth=x["depth"].double())
    refused("flowmap_amd: depth_consistency: intrinsics must be float32", k=x["k"].double())
    refused("flowmap_amd: depth_consistency: extrinsics must be float32", ext=x["ext"].double())
    refused("flowmap_amd: depth_consistency: depths of shape .* expected", depth=x["depth"][0])
    refused("flowmap_amd: depth_consistency: intrinsics of shape .* do not match the depths", k=x["k"][:, :-1])
    refused("flowmap_amd: depth_consistency: extrinsics of shape .* do not match the depths", ext=x["ext"][:, 1:])
    refused("flowmap_amd: depth_consistency: extrinsics of shape .* do not match the depths", ext=x["ext"][..., :3, :])
    refused("flowmap_amd: depth_consistency: depths and intrinsics must be tensors", k=None)
    with pytest.raises(ValueError, match="flowmap_amd: depth_consistency: batch x frames = 65536 exceeds"):
        fm.depth_consistency(x["depth"][:, :2].expand(32768, 2, 17, 23), x["k"][:, :2].expand(32768, 2, 3, 3), x["ext"][:, :2].expand(32768, 2, 4, 4))
    for tensor in x.values():
        assert not [key for key in tensor.__dict__ if key.startswith("_fm_")], "a note was left on an argument"
    # gradients recorded around the call change nothing: the outputs never require one
    depth = x["depth"].clone().requires_grad_(True)
    rg = fm.depth_consistency(depth, x["k"], x["ext"], details=True, tolerance=0.1)
    assert not any(getattr(rg, key).requires_grad for key in MAPS)
    before = _ops.counters["depth_consistency"]
    call()
    assert _ops.counters["depth_consistency"] == before + 1


# the C entries through ctypes, on REJECTED calls only (nothing reaches a launch); the last parameter of the size function is its output
C_PARAMS = ("depth k kinv ext offsets n_offsets batch frames height width first_frame count tolerance error code positions reprojected sampled support "
            "frame_sum frame_valid rel workspace stream").split()
C_VALID = dict(n_offsets=2, batch=1, frames=5, height=8, width=16, first_frame=1, count=2, tolerance=0.1)
C_REFUSED = ["nulls", dict(first_frame=4), dict(first_frame=-1), dict(count=0), dict(frames=1, first_frame=0, count=1), dict(batch=65536, first_frame=0, count=1),
             dict(height=32768, width=32768), dict(n_offsets=0), dict(n_offsets=9), dict(offsets=(0, 1)), dict(offsets=(1, 1)), dict(offsets=(5, 1)),
             dict(offsets=(-5, 1)), dict(tolerance=-1.0), dict(positions=None), dict(sampled=None), dict(frame_valid=None), dict(workspace=None),
             dict(rel=None), dict(code=None), dict(offsets=None), dict(kinv=None)]


def case_c_entries_refuse(lib, what):
    import ctypes

    from flowmap_amd import _lib

    def pointer(param, change, address):  # (the entry reads ``offsets`` on the host to check them: a real array of eight)
        if param != "offsets":
            return address
        return ctypes.cast((ctypes.c_int32 * 8)(*(list(change.get("offsets") or (-1, 2)) + [0] * 6)[:8]), ctypes.c_void_p)

    c_entry_refuses(lib, what, "fm_depth_consistency", C_PARAMS, C_VALID, C_REFUSED, pointer)
    size = lib.fm_depth_consistency_blocks
    size.argtypes, size.restype = _lib.SIGNATURES["fm_depth_consistency_blocks"], ctypes.c_int
    out = ctypes.c_int(-1)
    for hw, want in (((1, 1), 1), ((5, 7), 1), ((1, T), 1), ((1, T + 1), 2), ((64, 128), 8), ((720, 1280), 900)):
        assert size(*hw, ctypes.cast(ctypes.byref(out), ctypes.c_void_p)) == 0 and out.value == want, f"{what}: blocks{hw} = {out.value}"
    for hw in ((0, 4), (4, 0), (32768, 32768)):
        assert size(*hw, ctypes.cast(ctypes.byref(out), ctypes.c_void_p)) == 1 and size(*hw, None) == 1, f"{what}: blocks{hw} not refused"
    assert size(4, 4, None) == 1


def case_host_tensor_refused():
    host_tensor_refused(lambda: run("tiny", "cpu"), "flowmap_amd: depth_consistency: tensors are on cpu.*no CPU fallback")


# ---- check 7: training is left alone -----------------------------------------------------------------------------------------------------------


def case_training_untouched(dev, tracking, fuse):
    """operator_checks.train, 3 steps from step 1 after the warm-up, with and without Model.consistency between forward and backward (a
    window, details, a tolerance) and between the steps: operator_checks.assert_training_untouched with ``depth_consistency`` the one
    counter that differs — a LazyExtrinsics handed in is still unevaluated afterwards, and a flow-only step does hand one in."""
    steps = 3
    mid = lambda ns: ns.model.consistency(ns.out, offsets=(-2, -1, 1, 2), frames=(1, 3), details=True, tolerance=0.05)  # noqa: E731
    after = lambda ns: ns.model.consistency(ns.out)  # noqa: E731
    plain = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True)
    with_calls = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True, calls=(mid, after))
    assert_training_untouched(plain, with_calls, "depth_consistency", 2 * steps)
    if not tracking:
        assert all(was for was, _ in with_calls.lazy_kept), "a flow-only training step hands out a LazyExtrinsics: the case must exercise it"
    for r in with_calls.seen:
        assert bool(torch.isfinite(r.error).all()) and bool((r.code <= 3).all())
    first, second = with_calls.seen[0], with_calls.seen[1]
    assert first.error.shape == (1, 3, 4, 24, 32) and first.first_frame == 1 and second.error.shape == (1, 5, 2, 24, 32) and second.positions is None


# ---- check 8: memory (GPU) ---------------------------------------------------------------------------------------------------------------------


def case_memory(dev, name="wide"):
    """Peak allocated bytes during a call stay below the outputs + the workspace + one (h, w) float map: no (…, h, w, 3) surfaces, no F x F
    poses.  The workspace: the pose rows, K⁻¹, and the sums' slots."""
    (b, f, h, w), _, offsets = SPECS[name]
    x = {key: v.clone().to(dev) for key, v in case_inputs(name).items()}
    import flowmap_amd

    kw = dict(offsets=offsets, details=True, tolerance=0.05)
    flowmap_amd.depth_consistency(x["depth"], x["k"], x["ext"], **kw)  # (warm: libraries loaded, allocator primed)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = flowmap_amd.depth_consistency(x["depth"], x["k"], x["ext"], **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = sum(getattr(r, key).numel() * getattr(r, key).element_size() for key in MAPS)
    rows = b * f * len(offsets)
    round_up = lambda n: (n + 511) // 512 * 512  # noqa: E731  (the caching allocator's granularity)
    workspace = round_up(rows * 16 * 4) + round_up(b * f * 9 * 4) + round_up(rows * math.ceil(h * w / T) * 16)
    slack = 8 * 512  # (each output's share of the allocator's rounding)
    print(f"  {name}: peak {peak} B; outputs {outputs} B, workspace {workspace} B, one map {h * w * 4} B")
    assert peak <= outputs + workspace + h * w * 4 + slack, f"peak {peak} B > outputs {outputs} + workspace {workspace} + one map {h * w * 4}"


# ---- check 10: world_point_cloud(keep=...) -----------------------------------------------------------------------------------------------------


def case_point_cloud_keep(dev):
    import pytest

    from flowmap_amd import export

    g = load_golden("fn_export")
    depths, k, ext, colors = (t(g[key]).to(dev) for key in ("depths", "intrinsics", "extrinsics", "colors"))
    xyz, rgb = export.world_point_cloud(depths, k, ext, colors)
    same = export.world_point_cloud(depths, k, ext, colors, keep=None)
    assert torch.equal(same[0], xyz) and torch.equal(same[1], rgb)
    f, h, w = depths.shape
    r = run_support(depths, k, ext)
    keep = r.support[0] >= 2
    assert 0 < int(keep.sum()) < keep.numel(), "the mask must drop some points and keep some"
    kept_xyz, kept_rgb = export.world_point_cloud(depths, k, ext, colors, keep=keep)
    assert torch.equal(kept_xyz, xyz[keep.reshape(-1)]) and torch.equal(kept_rgb, rgb[keep.reshape(-1)])
    only_xyz, none = export.world_point_cloud(depths, k, ext, keep=keep)
    assert none is None and torch.equal(only_xyz, kept_xyz)
    for bad, match in ((keep[:-1], "keep of shape"), (keep.reshape(-1), "keep of shape"), (keep.float(), "keep must be a bool tensor"),
                       (keep.to(torch.uint8), "keep must be a bool tensor"), ([True], "keep must be a bool tensor")):
        with pytest.raises(RuntimeError, match=f"flowmap_amd: {match}"):
            export.world_point_cloud(depths, k, ext, colors, keep=bad)
    if torch.device(dev).type != "cpu":
        with pytest.raises(RuntimeError, match="flowmap_amd: keep is on cpu"):
            export.world_point_cloud(depths, k, ext, colors, keep=keep.cpu())


def run_support(depths, k, ext):
    import flowmap_amd

    f = depths.shape[0]
    offsets = tuple(d for d in (-2, -1, 1, 2) if abs(d) <= f - 1)
    return flowmap_amd.depth_consistency(depths[None], k[None], ext[None], offsets=offsets, tolerance=0.05)
