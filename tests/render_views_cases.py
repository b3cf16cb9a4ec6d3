"""projection.render_views / Model.render (fm_render_views): the depth maps of some source frames splatted into a list of cameras with a
64-bit z-buffer of atomic minima — per target pixel the nearest source pixel that lands in it, its depth and its colour.  The cases here
take a device; tests/test_hostsim_render_views.py runs them on the serial host double of the C ABI, tests/test_gpu_render_views.py on the
MI355X.

Truths.  tests/golden/fn_render_views.npz holds what the REFERENCE computes (tools/make_golden_render_views.py: its own sample_image_grid,
unproject, homogenize_points, transform_rigid and project_camera_space) in fp32 and in fp64 — per (view, source pixel) uv and q.z, per
target pixel the winner and its depth — for the cases small enough to commit; at every shape the same two evaluations come from the oracle
(oracle/flowmap_oracle.py: pixel_grid, lift, matvec, pinhole — restated in ``evaluate`` below), computed once per case.

The gate on a decision is exact and leaves nothing out (``check_render``).  With the fp64 evaluation, DELTA = 1e-4 of a target pixel and
RHO = 1e-5: a candidate FIRMLY covers pixel t when it covers t for every shift of its position by up to DELTA and q.z > near·(1+RHO); it
POSSIBLY covers t when some such shift does, with q.z > near·(1−RHO).  For every target pixel: a hole only where no candidate firmly
covers it (then depth == 0 and color == background exactly); otherwise the source must possibly cover it, its fp64 q.z must be
<= (1+RHO) x the smallest fp64 q.z among the firm candidates, the colour must be the source's bit for bit, and the depth is compared with
the fp64 q.z of ITS OWN source under conftest.assert_close_or_reference_gap (rel 1e-4, slack 2x the fp32 evaluation's own gap, norm-wise
over the covered pixels).  Pixels whose source differs from the fp64 winner may number at most 0.5 % of a case's target pixels; the fp32
oracle alone is held to the same cap against the fp64 oracle (``case_well_conditioned``).

Inputs: oracle.synth_scene (``depth_init``, ground-truth poses and K), seeded random colours; ``edge`` and ``tie`` are hand-built.
Cases (batch, frames, h, w); a workgroup owns T = 1024 consecutive source pixels of one (batch entry, view, source): see SPECS.
"""

from __future__ import annotations

import functools
import math

import torch

from conftest import assert_close_or_reference_gap, load_golden, relerr, t
from operator_checks import FRAMES, HEIGHT, WIDTH, assert_training_untouched, batch_colours, c_entry_refuses, host_tensor_refused, same_tensors, train, ulp_distance
from oracle import flowmap_oracle as orc

T = 1024  # source pixels per workgroup (fm_residual_args.h: kRenderTile)
DELTA, RHO = 1e-4, 1e-5
PM2, PM3 = (-2, -1, 1, 2), (-3, -2, -1, 1, 2, 3)
ALL = slice(None)
# name -> (scene: (batch, frames, h, w), seeds), what the call adds to (depths, intrinsics, extrinsics, colors)
SPECS = {
    "tiny": (((1, 2, 5, 7), (41,)), dict(held_out=ALL, offsets=(-1, 1))),  # fewer pixels than a wavefront; one neighbour each
    "odd": (((1, 6, 17, 23), (42,)), dict(held_out=ALL, offsets=PM3)),  # scalar path, partial last quad; the ends have fewer sources
    "vec": (((1, 7, 24, 32), (43,)), dict(held_out=ALL, offsets=PM2)),  # the 16-byte path below one tile
    "wide": (((1, 5, 64, 128), (44,)), dict(held_out=ALL, offsets=PM2)),  # several whole tiles
    "tile": (((1, 2, 1, T), (48,)), dict(held_out=ALL, offsets=(-1, 1))),  # exactly one tile
    "tile1": (((1, 2, 1, T + 1), (49,)), dict(held_out=ALL, offsets=(-1, 1))),  # one pixel past it
    "two": (((2, 4, 9, 12), (45, 145)), dict(held_out=ALL, offsets=PM2)),  # two batch entries with different poses and views
    "down": (((1, 6, 17, 23), (42,)), dict(held_out=ALL, offsets=PM3, shape=(9, 12))),  # many-to-one
    "up": (((1, 6, 17, 23), (42,)), dict(held_out=ALL, offsets=PM3, shape=(34, 46))),  # a finer target grid: holes exist
    "up1": (((1, 6, 17, 23), (42,)), dict(held_out=ALL, offsets=PM3, shape=(34, 46), radius=1)),  # footprints clipped at the border
    "up2": (((1, 6, 17, 23), (42,)), dict(held_out=ALL, offsets=PM3, shape=(34, 46), radius=2)),
    "free": (((1, 4, 9, 12), (46,)), dict(views="free", sources=(1, 2))),  # cameras that are none of the frames', a window of sources
    "edge": (((1, 4, 9, 12), (47,)), dict(held_out=ALL, offsets=(-1, 1), near=1.9)),  # hand-built: all behind, partly outside, cut by near
    "pile": (((1, 3, 16, 16), (50,)), dict(views="frame1", shape=(2, 2))),  # every lane of every wave hits one of four addresses
    "tie": (((1, 3, 8, 8), (51,)), dict(held_out=(0, 1), offsets=(1, 2))),  # frames 1 and 2 identical: equal keys but for the index
    "identity": (((1, 6, 17, 23), (42,)), dict(views="frame0", sources=(0, 1))),  # a single source into its own camera
}
GOLDEN_CASES = ("tiny", "two", "free", "edge")  # (the others are generated from the seed: their fixtures would not fit the size limit)
INPUT_KEYS = ("depth", "k", "ext", "colors")


@functools.lru_cache(maxsize=None)
def scene_inputs(shape, seeds, kind):
    b, f, h, w = shape
    colors = torch.rand((b, f, 3, h, w), generator=torch.Generator().manual_seed(1000 + seeds[0]))
    if kind == "edge":  # (depth_consistency_cases' edge scene: a rotation by pi about y, two translations)
        depth = 1.5 + torch.rand((1, f, h, w), generator=torch.Generator().manual_seed(seeds[0]))
        k = orc.focal_to_k(torch.tensor(0.85), (h, w)).expand(1, f, 3, 3).contiguous()
        ext = torch.eye(4).repeat(1, f, 1, 1)
        ext[0, 1, 0, 0] = ext[0, 1, 2, 2] = -1.0
        ext[0, 2, :3, 3] = torch.tensor([1.0, 0.0, 0.0])
        ext[0, 3, :3, 3] = torch.tensor([0.0, -0.7, 0.3])
        return {"depth": depth, "k": k, "ext": ext, "colors": colors}
    scenes = [orc.synth_scene(f, h, w, seed=seed) for seed in seeds]
    x = {"depth": torch.stack([s["depth_init"] for s in scenes]), "k": torch.stack([s["intrinsics_gt"].expand(f, 3, 3) for s in scenes]).contiguous(),
         "ext": torch.stack([s["extrinsics_gt"] for s in scenes]), "colors": colors}
    if kind == "tie":  # frames 1 and 2 identical in depth, K and pose (colours differ: the winner shows)
        for key in ("depth", "k", "ext"):
            x[key][:, 2] = x[key][:, 1]
    return x


def case_inputs(name):
    """depth (b, F, h, w), k (b, F, 3, 3), ext (b, F, 4, 4), colors (b, F, 3, h, w) of a case (tools/make_golden_render_views.py draws them from here)."""
    (shape, seeds), _ = SPECS[name]
    return scene_inputs(shape, seeds, name if name in ("edge", "tie") else "scene")


def free_cameras(x):
    """Three cameras that are none of the frames': another focal length, a pose between / beside the frames'."""
    b, f, h, w = x["depth"].shape
    k = torch.stack([orc.focal_to_k(torch.tensor(focal), (h, w)) for focal in (0.7, 0.85, 1.1)])[None].expand(b, 3, 3, 3).contiguous()
    ext = x["ext"][:, [0, 1, 3]].clone()
    ext[:, 0, :3, 3] += torch.tensor([0.03, -0.02, 0.01])
    ext[:, 1, :3, 3] = 0.5 * (x["ext"][:, 1, :3, 3] + x["ext"][:, 2, :3, 3])
    angle = 0.05
    rot = torch.tensor([[math.cos(angle), 0.0, math.sin(angle)], [0.0, 1.0, 0.0], [-math.sin(angle), 0.0, math.cos(angle)]])
    ext[:, 2, :3, :3] = ext[:, 2, :3, :3] @ rot
    return k, ext


def call_of(name, x=None, **changed):
    """The keyword arguments of a case's call, and what they mean: (kw, view_k, view_ext, pairs, (oh, ow), radius, near)."""
    x = x or case_inputs(name)
    kw = {**SPECS[name][1], **changed}
    b, f, h, w = x["depth"].shape
    if "views" in kw:
        if isinstance(kw["views"], str):
            kw["views"] = free_cameras(x) if kw["views"] == "free" else tuple(x[key][:, int(kw["views"][5:])][:, None].contiguous() for key in ("k", "ext"))
        view_k, view_ext = kw["views"]
        sources = kw.get("sources")
        first, count = (0, f) if sources is None else sources
        pairs = [(v, i) for v in range(view_k.shape[1]) for i in range(first, first + count)]
    else:
        window = kw["held_out"]
        first, stop = window.indices(f)[:2] if isinstance(window, slice) else (window[0], window[0] + window[1])
        view_k, view_ext = x["k"][:, first:stop], x["ext"][:, first:stop]
        pairs = [(v, first + v + d) for v in range(stop - first) for d in kw.get("offsets", PM2) if 0 <= first + v + d < f]
    return kw, view_k, view_ext, pairs, tuple(kw.get("shape", (h, w))), kw.get("radius", 0), kw.get("near", 0.0)


# ---- the oracle's composition ----------------------------------------------------------------------------------------------------------------


def evaluate(x, view_k, view_ext, pairs, dtype, fns=None):
    """uv (b, V, F, h·w, 2) and q.z (b, V, F, h·w) of every pair in ``dtype`` and ``present`` (V, F), by the oracle's functions (``fns``: the
    reference's own, in tools/make_golden_render_views.py).  The relative pose is formed in fp64 and, for fp32, rounded once."""
    grid, lift, homogeneous, transform, project = fns or (lambda s: orc.pixel_grid(s, dtype=dtype)[0], orc.lift, orc.append_one,
                                                          lambda p, m: orc.matvec(m, p), orc.pinhole)
    depth, k = x["depth"].to(dtype), x["k"].to(dtype)
    b, f, h, w = depth.shape
    n_views = view_k.shape[1]
    uv = torch.full((b, n_views, f, h * w, 2), float("nan"), dtype=dtype)
    qz = torch.full((b, n_views, f, h * w), float("nan"), dtype=dtype)
    present = torch.zeros((n_views, f), dtype=torch.bool)
    if pairs:
        vs, srcs = [p[0] for p in pairs], [p[1] for p in pairs]
        xy = grid((h, w)).to(dtype)
        p = lift(xy, depth[:, srcs], k[:, srcs][:, :, None, None])
        rel = (torch.linalg.inv(view_ext[:, vs].double()) @ x["ext"][:, srcs].double()).to(dtype)
        q = transform(homogeneous(p), rel[:, :, None, None])[..., :3]
        uv[:, vs, srcs] = project(q, view_k.to(dtype)[:, vs][:, :, None, None]).reshape(b, len(pairs), h * w, 2)
        qz[:, vs, srcs] = q[..., 2].reshape(b, len(pairs), h * w)
        present[vs, srcs] = True
    return {"uv": uv, "qz": qz, "present": present}


def _scatter_min(values, at, ok, n_target, fill):
    """min over the candidates (b, V, C) that are ``ok`` of ``values`` per target pixel ``at`` -> (b, V, n_target), ``fill`` where none."""
    out = torch.full((*values.shape[:2], n_target), fill, dtype=values.dtype)
    out.scatter_reduce_(2, torch.where(ok, at, torch.zeros_like(at)), torch.where(ok, values, torch.full_like(values, fill)), "amin")
    return out


def winners(ev, shape, radius, near):
    """The evaluation's OWN decisions: per target pixel (b, V, oh·ow) the winner's absolute source index (−1: hole) and its q.z."""
    oh, ow = shape
    uv, qz = ev["uv"], ev["qz"]
    b, n_views, f, n = qz.shape
    live = (qz > near) & (uv >= 0).all(-1) & (uv < 1).all(-1)
    tx = torch.floor(uv[..., 0] * ow).clamp(0, ow - 1).nan_to_num(0).long()
    ty = torch.floor(uv[..., 1] * oh).clamp(0, oh - 1).nan_to_num(0).long()
    index = (torch.arange(f)[:, None] * n + torch.arange(n)).expand(b, n_views, f, n).reshape(b, n_views, f * n)
    depth_of = qz.double().reshape(b, n_views, f * n)
    best_z = torch.full((b, n_views, oh * ow), math.inf, dtype=torch.float64)
    spots = []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x, y = tx + dx, ty + dy
            ok = (live & (x >= 0) & (x < ow) & (y >= 0) & (y < oh)).reshape(b, n_views, f * n)
            at = (y * ow + x).reshape(b, n_views, f * n)
            spots.append((at, ok))
            best_z = torch.minimum(best_z, _scatter_min(depth_of, at, ok, oh * ow, math.inf))
    best = torch.full((b, n_views, oh * ow), 2**62, dtype=torch.int64)
    for at, ok in spots:
        at = torch.where(ok, at, torch.zeros_like(at))
        best = torch.minimum(best, _scatter_min(index, at, ok & (depth_of == best_z.gather(2, at)), oh * ow, 2**62))
    hole = best == 2**62
    return torch.where(hole, torch.full_like(best, -1), best), torch.where(hole, torch.zeros_like(best_z), best_z)


def firm_minimum(ev64, shape, radius, near):
    """Per target pixel (b, V, oh·ow) the smallest fp64 q.z among the candidates that FIRMLY cover it (inf: none does)."""
    oh, ow = shape
    uv, qz = ev64["uv"], ev64["qz"]
    b, n_views, f, n = qz.shape
    px, py = uv[..., 0] * ow, uv[..., 1] * oh
    tx, ty = torch.floor(px).nan_to_num(0).long(), torch.floor(py).nan_to_num(0).long()
    depth_of = qz.reshape(b, n_views, f * n)
    out = torch.full((b, n_views, oh * ow), math.inf, dtype=torch.float64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x, y = tx + dx, ty + dy
            inside = (x >= 0) & (x < ow) & (y >= 0) & (y < oh)
            firm = inside & (qz > near * (1 + RHO)) & _covers(px, py, x, y, radius, oh, ow, -DELTA)
            out = torch.minimum(out, _scatter_min(depth_of, (y * ow + x).reshape(b, n_views, f * n), firm.reshape(b, n_views, f * n), oh * ow, math.inf))
    return out


def _covers(px, py, x, y, radius, oh, ow, margin):
    """Does a candidate at (px, py) target pixels cover pixel (x, y)?  margin = −DELTA: under every shift by up to DELTA; +DELTA: under some."""
    lo_x, hi_x = (x - radius).clamp_min(0).to(px.dtype), (x + radius + 1).clamp_max(ow).to(px.dtype)
    lo_y, hi_y = (y - radius).clamp_min(0).to(py.dtype), (y + radius + 1).clamp_max(oh).to(py.dtype)
    return (px + margin >= lo_x) & (px - margin < hi_x) & (py + margin >= lo_y) & (py - margin < hi_y)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """(fp32 evaluation, fp64 evaluation, fp64 winners, firm minimum) of a case, computed once."""
    x = case_inputs(name)
    _, view_k, view_ext, pairs, shape, radius, near = call_of(name)
    ev = {dtype: evaluate(x, view_k, view_ext, pairs, dtype) for dtype in (torch.float32, torch.float64)}
    return ev[torch.float32], ev[torch.float64], winners(ev[torch.float64], shape, radius, near), firm_minimum(ev[torch.float64], shape, radius, near)


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------


def check_render(r, x, ev32, ev64, win64, firm, shape, radius, near, what, background=0.0, views=ALL, allow_empty=False):
    """The gate of the module docstring on a RenderedViews (``views``: the rows of the evaluation it holds) -> the number of target pixels
    whose source differs from the fp64 winner."""
    oh, ow = shape
    b, f, h, w = x["depth"].shape
    n = h * w
    uv, qz, present = ev64["uv"][:, views], ev64["qz"][:, views], ev64["present"][views]
    n_views = qz.shape[1]
    win, firm = win64[0][:, views], firm[:, views]
    source = r.source.cpu()
    assert source.dtype == torch.int32 and tuple(source.shape) == (b, n_views, oh, ow), f"{what}.source: {source.dtype} {tuple(source.shape)}"
    assert r.depth.dtype == torch.float32 and tuple(r.depth.shape) == (b, n_views, oh, ow) and r.source_shape == (h, w)
    src = source.long().reshape(b, n_views, oh * ow)
    depth = r.depth.cpu().reshape(b, n_views, oh * ow)
    hole = src < 0
    assert bool((src[hole] == -1).all()) and bool((src < f * n).all())
    wrong = hole & torch.isfinite(firm)
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} holes where a candidate firmly covers the pixel"
    assert bool((depth[hole] == 0).all()), f"{what}: depth is not exactly 0 in a hole"
    # the source of a covered pixel: a pair of the call that possibly covers it, no further than the firm minimum allows
    s = src.clamp_min(0)
    frame, pixel = s // n, s % n
    vi = torch.arange(n_views)[None, :, None].expand_as(s)
    bi = torch.arange(b)[:, None, None].expand_as(s)
    in_call = present[vi, frame]
    assert bool(in_call[~hole].all()), f"{what}: a source frame that is none of its view's"
    px, py, z = uv[bi, vi, frame, pixel, 0] * ow, uv[bi, vi, frame, pixel, 1] * oh, qz[bi, vi, frame, pixel]
    at = torch.arange(oh * ow)[None, None].expand_as(s)
    possible = _covers(px, py, at % ow, at // ow, radius, oh, ow, DELTA) & (z > near * (1 - RHO))
    assert bool(possible[~hole].all()), f"{what}: {int((~possible & ~hole).sum())} sources do not cover their pixel"
    late = ~hole & (z > (1 + RHO) * firm)
    assert not bool(late.any()), f"{what}: {int(late.sum())} pixels kept a source behind a firm candidate (worst ratio {float((z / firm)[late].max()):.8f})"
    if x.get("colors") is not None and r.color is not None:
        assert tuple(r.color.shape) == (b, n_views, 3, oh, ow) and r.color.dtype == torch.float32
        planes = x["colors"].permute(0, 2, 1, 3, 4).reshape(b, 3, 1, f * n).expand(b, 3, n_views, f * n)
        want = torch.gather(planes, 3, s[:, None].expand(b, 3, n_views, oh * ow))
        want = torch.where(hole[:, None], torch.full_like(want, background), want).permute(0, 2, 1, 3).reshape(b, n_views, 3, oh, ow)
        assert torch.equal(r.color.cpu(), want), f"{what}.color is not the winner's colour bit for bit (or the background in a hole)"
    covered = ~hole
    if int(covered.sum()) == 0:
        assert allow_empty, f"{what}: nothing is covered"
    else:
        z32 = ev32["qz"][:, views][bi, vi, frame, pixel]
        e, gap = assert_close_or_reference_gap(depth[covered], z[covered], z32[covered], rel=1e-4, slack=2.0, what=f"{what}.depth")
        print(f"  {what}.depth: err {e:.2e} (fp32 oracle's own gap {gap:.2e}) over {int(covered.sum())} pixels, {int(hole.sum())} holes")
    differ = int((src != win).sum())
    assert differ <= 5e-3 * src.numel(), f"{what}: {differ} of {src.numel()} target pixels keep another source than the fp64 winner"
    return differ


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------


def run(name, dev, x=None, colors=True, **changed):
    import flowmap_amd

    x = x or case_inputs(name)
    kw = call_of(name, x, **changed)[0]
    if "views" in kw:
        kw["views"] = tuple(v.clone().to(dev) for v in kw["views"])
    y = {key: v.clone().to(dev) for key, v in x.items()}
    return flowmap_amd.render_views(y["depth"], y["k"], y["ext"], y["colors"] if colors else None, **kw)


def same_render(a, b, what="", **kw):
    same_tensors(a, b, ("color", "depth", "source"), what, **kw)


def keys_of(r):
    """The z-buffer a render stands for: float_bits(depth) << 32 | source, the largest int64 in a hole."""
    key = (r.depth.contiguous().view(torch.int32).long() << 32) | r.source.long()
    return torch.where(r.source < 0, torch.full_like(key, torch.iinfo(torch.int64).max), key)


# ---- check 1: oracle and reference parity -------------------------------------------------------------------------------------------------------


def case_oracle_parity(dev, name):
    x = case_inputs(name)
    ev32, ev64, win64, firm = oracle_case(name)
    _, _, _, pairs, shape, radius, near = call_of(name)
    r = run(name, dev)
    check_render(r, x, ev32, ev64, win64, firm, shape, radius, near, name, allow_empty=False)
    b, f, h, w = x["depth"].shape
    source, frames = r.source.cpu(), r.source_frame().cpu()
    assert frames.dtype == torch.int32 and torch.equal(frames, torch.where(source < 0, source, source // (h * w)))
    if "held_out" in SPECS[name][1]:
        assert r.first_frame == 0 and r.offsets == tuple(SPECS[name][1]["offsets"])
        own = torch.arange(frames.shape[1], dtype=torch.int32)[None, :, None, None]
        assert not bool((frames == own).any()), "a held-out view drew from its own frame"
    else:
        assert r.first_frame is None and r.offsets is None
    if name == "up":
        assert int((source < 0).sum()) > 0, "a one-pixel splat into a finer grid must leave holes"
        fewer = [int((run(n, dev).source < 0).sum()) for n in ("up", "up1", "up2")]
        assert fewer[0] > fewer[1] >= fewer[2], f"radius must trade holes away: {fewer}"
    if name == "edge":
        assert bool((source[:, 1] == -1).all()) and bool((source[:, 0] == -1).all()), "every point lies behind the views 0 and 1"
        assert 0 < int((source[:, 2] >= 0).sum()) < h * w and 0 < int((source[:, 3] >= 0).sum())
        assert int((run(name, dev, near=0.0).source >= 0).sum()) > int((source >= 0).sum()), "near must cut some points"
    if name == "tie":
        assert set(frames.unique().tolist()) <= {-1, 1} and int((frames == 1).sum()) > 0, f"tie: frames {frames.unique().tolist()}"
    if name == "pile":
        assert int((source >= 0).sum()) == 4, "pile: every one of the four target pixels is covered"
        assert torch.equal(source.reshape(1, 1, 4).long(), win64[0]), "pile: the exact minimum must win"
    if name == "identity":
        assert torch.equal(source.reshape(-1).long(), torch.arange(h * w)), "identity: source[t] == t"
        assert float(((r.depth.cpu()[0, 0] - x["depth"][0, 0]).abs() / x["depth"][0, 0]).max()) <= 1e-5
    return r


def case_well_conditioned(name):
    """The fp32 oracle alone against the fp64 oracle: its winners differ on at most 0.5 % of the target pixels."""
    ev32, ev64, win64, _ = oracle_case(name)
    _, _, _, _, shape, radius, near = call_of(name)
    win32 = winners(ev32, shape, radius, near)
    differ = int((win32[0] != win64[0]).sum())
    assert differ <= 5e-3 * win64[0].numel(), f"{name}: the fp32 and fp64 oracles disagree on {differ} of {win64[0].numel()} target pixels: take another seed"


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("fn_render_views")


def golden_inputs(name):
    return {key: t(golden()[f"{name}_{key}"]) for key in INPUT_KEYS}


def case_reference_parity(dev, name):
    """A fixture case against what the imported reference computed: its fp64 evaluation the truth, its fp32 evaluation the gap."""
    g = golden()
    x = golden_inputs(name)  # the inputs the fixture was made from (a scene drawn on another machine differs in the last bits of sin / cos)
    for key in INPUT_KEYS:
        assert relerr(case_inputs(name)[key], x[key]) < 1e-6, f"{name}: the fixture's {key} is not the case's"
    kw, view_k, view_ext, pairs, shape, radius, near = call_of(name, x)
    assert [list(p) for p in pairs] == g[f"{name}_pairs"].tolist()
    present = torch.zeros((view_k.shape[1], x["depth"].shape[1]), dtype=torch.bool)
    present[[p[0] for p in pairs], [p[1] for p in pairs]] = True
    ev32 = {"uv": t(g[f"{name}_uv"]), "qz": t(g[f"{name}_qz"]), "present": present}
    ev64 = {"uv": t(g[f"{name}_f64_uv"]), "qz": t(g[f"{name}_f64_qz"]), "present": present}
    win64 = (t(g[f"{name}_f64_win_source"]).long(), t(g[f"{name}_f64_win_depth"]))
    again = winners(ev64, shape, radius, near)
    assert torch.equal(again[0], win64[0]) and torch.equal(again[1], win64[1]), "the fixture's winners are its evaluation's"
    oracle64 = evaluate(x, view_k, view_ext, pairs, torch.float64)
    ok = present[None, :, :, None].expand_as(oracle64["qz"])
    assert relerr(oracle64["qz"][ok], ev64["qz"][ok]) < 1e-12 and relerr(oracle64["uv"][ok], ev64["uv"][ok]) < 1e-12, "the reference and the oracle agree in fp64"
    r = run(name, dev, x=x)
    check_render(r, x, ev32, ev64, win64, firm_minimum(ev64, shape, radius, near), shape, radius, near, f"{name} vs the reference")


# ---- check 2: exact properties ------------------------------------------------------------------------------------------------------------------


def case_exact_properties(dev, name):
    """Three calls give the same bits; so does any order of the offsets and of the pairs; a render from A ∪ B is the per-pixel minimum-key
    merge of the renders from A and from B; batch entry 0 alone is entry 0 of the batch; a window of views is the same rows of the full call."""
    from flowmap_amd import _ops
    from flowmap_amd.types import RenderedViews

    x = case_inputs(name)
    b, f, h, w = x["depth"].shape
    spec = SPECS[name][1]
    full = run(name, dev)
    for _ in range(2):
        same_render(run(name, dev), full, "repeat: ")
    bare = run(name, dev, colors=False)
    assert bare.color is None and torch.equal(bare.source, full.source) and torch.equal(bare.depth, full.depth)
    kw, view_k, view_ext, pairs, shape, radius, near = call_of(name)
    if "held_out" in spec:
        offsets = tuple(spec["offsets"])
        same_render(run(name, dev, offsets=offsets[::-1]), full, "offsets reversed: ")
        same_render(run(name, dev, offsets=offsets[1:] + offsets[:1]), full, "offsets rotated: ")
        for window in ((0, 1), (f - 1, 1), (1, max(1, f - 2))) if spec["held_out"] == ALL else ():
            part = run(name, dev, held_out=window)
            assert part.first_frame == window[0]
            same_render(part, full, f"views {window}: ", rows=slice(window[0], window[0] + window[1]))
    # the pairs in another order, and split into two sets: at the operator
    y = {key: v.clone().to(dev) for key, v in x.items()}
    args = (y["depth"], _ops.intrinsics_inverse_peek(y["k"]), y["ext"], y["colors"], view_k.clone().to(dev).contiguous(), view_ext.clone().to(dev).contiguous())
    render = lambda some: RenderedViews(*_ops.render_views(*args, torch.tensor(some, dtype=torch.int32).reshape(-1, 2).to(dev), shape, radius, near, 0.0), (h, w))  # noqa: E731
    order = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(7)).tolist()
    same_render(render([pairs[i] for i in order]), full, "pairs permuted: ")
    same_render(render(pairs + pairs[::-1]), full, "pairs twice: ")
    if len(pairs) >= 2:
        part_a, part_b = render(pairs[0::2]), render(pairs[1::2])
        take_a = keys_of(part_a) <= keys_of(part_b)
        assert torch.equal(torch.where(take_a, part_a.source, part_b.source), full.source), "A ∪ B: source"
        assert torch.equal(torch.where(take_a, part_a.depth, part_b.depth), full.depth), "A ∪ B: depth"
        assert torch.equal(torch.where(take_a[:, :, None], part_a.color, part_b.color), full.color), "A ∪ B: color"
    none = render([])
    assert bool((none.source == -1).all()) and bool((none.depth == 0).all()) and bool((none.color == 0).all()), "no pair: all holes"
    if b > 1:
        alone = run(name, dev, x={key: v[:1] for key, v in x.items()})
        same_render(alone, full, "batch entry 0 alone: ", batch=slice(0, 1))
    ground = run(name, dev, background=0.25)
    assert torch.equal(ground.source, full.source) and bool((ground.color.permute(0, 1, 3, 4, 2)[ground.source < 0] == 0.25).all())


# ---- check 3: the GPU against the host double -------------------------------------------------------------------------------------------------


def case_gpu_against_host_double(dev, name):
    from flowmap_amd import _lib
    from helpers import build_host_sim

    gpu = run(name, dev)
    _lib.set_library_for_testing(build_host_sim())
    try:
        host = run(name, "cpu")
    finally:
        _lib.set_library_for_testing(None)
    x = case_inputs(name)
    ev32, ev64, win64, firm = oracle_case(name)
    _, _, _, _, shape, radius, near = call_of(name)
    for r, what in ((gpu, f"gpu {name}"), (host, f"host {name}")):  # a source may differ only where the gate admits both
        check_render(r, x, ev32, ev64, win64, firm, shape, radius, near, what)
    same = (gpu.source.cpu() == host.source) & (host.source >= 0)
    worst = ulp_distance(gpu.depth.cpu()[same], host.depth[same]) if int(same.sum()) else 0
    print(f"  GPU vs host double, {name}: {int((gpu.source.cpu() != host.source).sum())} sources differ, depth within {worst} ulp")
    assert worst <= 4, f"{name}: depth differs by {worst} ulp between the GPU and the host double on equal sources"


# ---- check 4: arguments and refusals -------------------------------------------------------------------------------------------------------------


def case_arguments(dev):
    import pytest

    import flowmap_amd
    from flowmap_amd import RenderedViews, _ops
    from flowmap_amd.model import projection as fm

    x = {key: v.clone().to(dev) for key, v in case_inputs("odd").items()}
    cams = (x["k"][:, :2].contiguous(), x["ext"][:, :2].contiguous())
    call = lambda *a, **kw: fm.render_views(x["depth"], x["k"], x["ext"], *a, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="flowmap_amd: render_views: give exactly one of views"):
        call()
    with pytest.raises(ValueError, match="flowmap_amd: render_views: give exactly one of views"):
        call(views=cams, held_out=(0, 2))
    with pytest.raises(ValueError, match="flowmap_amd: render_views: sources goes with views"):
        call(held_out=(0, 2), sources=(0, 2))
    for bad in ((0,), (1, 0), (1, 1), (), tuple(range(1, 6)) + tuple(range(-4, 0)), (6,), (1, -7), 1, (1.0,), None, "1"):
        with pytest.raises(ValueError, match="flowmap_amd: render_views: .*offsets"):
            call(held_out=(0, 2), offsets=bad)
    for bad in (slice(0, 4, 2), (0, 0), (5, 2), (-1, 2), (0, 7), "all", 1, (1.0, 2), (0, 1, 2)):
        with pytest.raises(ValueError, match="flowmap_amd: render_views.*frames"):
            call(held_out=bad)
        with pytest.raises(ValueError, match="flowmap_amd: render_views.*frames"):
            call(views=cams, sources=bad)
    for bad in (-1, 3, 1.0, None, True):
        with pytest.raises(ValueError, match="flowmap_amd: render_views: radius"):
            call(held_out=(0, 2), radius=bad)
    for bad in (-1e-3, float("nan"), float("inf"), None, "0"):
        with pytest.raises(ValueError, match="flowmap_amd: render_views: near"):
            call(held_out=(0, 2), near=bad)
    for bad in (float("nan"), None):
        with pytest.raises(ValueError, match="flowmap_amd: render_views: background"):
            call(held_out=(0, 2), background=bad)
    for bad in ((0, 4), (4,), (4.0, 4), 4, "hw", (4, -1)):
        with pytest.raises(ValueError, match="flowmap_amd: render_views: shape"):
            call(held_out=(0, 2), shape=bad)
    for bad in (x["k"], (x["k"],), (x["k"], None), "free"):
        with pytest.raises(ValueError, match="flowmap_amd: render_views: views must be a pair"):
            call(views=bad)
    for bad in ((cams[0], cams[1][:, :1]), (cams[0][0], cams[1]), (cams[0], cams[1][..., :3, :]), (cams[1], cams[0])):
        with pytest.raises(RuntimeError, match="flowmap_amd: render_views: views of shapes"):
            call(views=bad)

    def refused(match, colors=None, **changed):
        y = {**x, **changed}
        with pytest.raises(RuntimeError, match=match):
            fm.render_views(y["depth"], y["k"], y["ext"], colors, held_out=(0, 2))

    refused("flowmap_amd: render_views: depths must be float32", depth=x["depth"].double())
    refused("flowmap_amd: render_views: intrinsics must be float32", k=x["k"].double())
    refused("flowmap_amd: render_views: extrinsics must be float32", ext=x["ext"].double())
    refused("flowmap_amd: render_views: colors must be float32", colors=x["colors"].double())
    refused("flowmap_amd: render_views: depths of shape .* expected", depth=x["depth"][0])
    refused("flowmap_amd: render_views: intrinsics of shape .* do not match the depths", k=x["k"][:, :-1])
    refused("flowmap_amd: render_views: extrinsics of shape .* do not match the depths", ext=x["ext"][:, 1:])
    refused("flowmap_amd: render_views: colors of shape .* do not match the depths", colors=x["colors"][:, :, :2])
    refused("flowmap_amd: render_views: colors of shape .* do not match the depths", colors=x["depth"])
    refused("flowmap_amd: render_views: depths and intrinsics must be tensors", k=None)
    with pytest.raises(RuntimeError, match="flowmap_amd: render_views: views\\[0\\] must be float32"):
        call(views=(cams[0].double(), cams[1]))
    # frames x height x width >= 2^31: refused by name before anything is allocated (expanded views: no memory behind them)
    big = x["depth"][:, :1, :1, :1].expand(1, 2, 32768, 32768)
    with pytest.raises(ValueError, match="flowmap_amd: render_views: frames x height x width = 2147483648 does not fit the int32 source index"):
        fm.render_views(big, x["k"][:, :2], x["ext"][:, :2], held_out=(0, 1), offsets=(1,), shape=(4, 4))
    with pytest.raises(ValueError, match="flowmap_amd: render_views: batch x .* pairs = 65536 exceeds"):
        fm.render_views(x["depth"][:, :2].expand(16384, 2, 17, 23), x["k"][:, :2].expand(16384, 2, 3, 3), x["ext"][:, :2].expand(16384, 2, 4, 4),
                        views=(x["k"][:, :2].expand(16384, 2, 3, 3), x["ext"][:, :2].expand(16384, 2, 4, 4)))
    if torch.device(dev).type != "cpu":
        with pytest.raises(RuntimeError, match="flowmap_amd: .*different devices|flowmap_amd: .*on cpu"):
            fm.render_views(x["depth"], x["k"].cpu(), x["ext"], held_out=(0, 2))
        with pytest.raises(RuntimeError, match="flowmap_amd: .*different devices|flowmap_amd: .*on cpu"):
            call(x["colors"].cpu(), held_out=(0, 2))
    r = call(x["colors"], held_out=slice(-2, None), offsets=[5, -5, 1])
    assert isinstance(r, RenderedViews) and r.first_frame == 4 and r.offsets == (5, -5, 1) and r.color.shape == (1, 2, 3, 17, 23)
    assert call(views=cams, sources=slice(1, 3), shape=[4, 6]).source.shape == (1, 2, 4, 6) and call(held_out=(0, 1)).offsets == PM2
    assert flowmap_amd.render_views is fm.render_views
    for tensor in x.values():
        assert not [key for key in tensor.__dict__ if key.startswith("_fm_")], "a note was left on an argument"
    depth = x["depth"].clone().requires_grad_(True)
    rg = fm.render_views(depth, x["k"], x["ext"], x["colors"].clone().requires_grad_(True), held_out=(0, 2))
    assert not (rg.color.requires_grad or rg.depth.requires_grad or rg.source.requires_grad)
    before = _ops.counters["render_views"]
    call(held_out=(0, 2))
    assert _ops.counters["render_views"] == before + 1


# the C entries through ctypes, on REJECTED calls only (nothing reaches a launch); the last parameter of the size function is its output
C_PARAMS = ("depth kinv ext colors view_k view_ext pairs n_pairs batch frames height width views out_height out_width radius near background color out_depth "
            "source workspace stream").split()
C_VALID = dict(n_pairs=3, batch=1, frames=5, height=8, width=16, views=2, out_height=8, out_width=16, radius=1, near=0.0, background=0.0)
C_REFUSED = ["nulls", dict(n_pairs=-1), dict(batch=0), dict(batch=65536, n_pairs=1), dict(batch=2, n_pairs=32768), dict(frames=0), dict(views=0),
             dict(height=0), dict(width=0), dict(height=32768, width=32768), dict(frames=3, height=32768, width=32767), dict(out_height=0), dict(out_width=-1),
             dict(out_height=32768, out_width=32768), dict(views=65536, out_height=4096, out_width=4096), dict(radius=-1), dict(radius=3), dict(near=-1.0),
             dict(near=float("nan")), dict(near=float("inf")), dict(background=float("nan")), dict(depth=None), dict(kinv=None), dict(ext=None),
             dict(view_k=None), dict(view_ext=None), dict(pairs=None), dict(colors=None), dict(color=None), dict(out_depth=None), dict(source=None),
             dict(workspace=None)]


def case_c_entries_refuse(lib, what):
    import ctypes

    from flowmap_amd import _lib

    c_entry_refuses(lib, what, "fm_render_views", C_PARAMS, C_VALID, C_REFUSED)
    size = lib.fm_render_views_workspace
    size.argtypes, size.restype = _lib.SIGNATURES["fm_render_views_workspace"], ctypes.c_int
    out = ctypes.c_long(-1)
    cast = lambda: ctypes.cast(ctypes.byref(out), ctypes.c_void_p)  # noqa: E731
    for args in ((1, 1, 1, 1, 0), (1, 2, 5, 7, 2), (2, 4, 9, 12, 12), (1, 8, 720, 1280, 32)):
        b, v, oh, ow, n_pairs = args
        assert size(*args, cast()) == 0 and out.value == 8 * b * v * oh * ow + 64 * b * n_pairs, f"{what}: workspace{args} = {out.value}"
    for args in ((0, 1, 4, 4, 1), (1, 0, 4, 4, 1), (1, 1, 0, 4, 1), (1, 1, 4, 0, 1), (1, 1, 4, 4, -1), (1, 1, 32768, 32768, 1), (2, 1, 4, 4, 32768)):
        assert size(*args, cast()) == 1 and size(*args, None) == 1, f"{what}: workspace{args} not refused"
    assert size(1, 1, 4, 4, 1, None) == 1


def case_host_tensor_refused():
    host_tensor_refused(lambda: run("tiny", "cpu"), "flowmap_amd: render_views: tensors are on cpu.*no CPU fallback")


# ---- check 5: training is left alone -----------------------------------------------------------------------------------------------------------


def case_training_untouched(dev, tracking, fuse):
    """operator_checks.train, 3 steps from step 1 after the warm-up, with and without Model.render between forward and backward (held-out,
    coloured from the batch) and between the steps (free cameras): operator_checks.assert_training_untouched with ``render_views`` the
    one counter that differs — a LazyExtrinsics handed in is still unevaluated afterwards, and a flow-only step does hand one in."""
    steps = 3
    sc = orc.synth_scene(FRAMES, HEIGHT, WIDTH, seed=21)  # (the training problem's scene: two of its true cameras)
    cams = (sc["intrinsics_gt"].expand(1, 2, 3, 3).contiguous().to(dev), sc["extrinsics_gt"][None, 1:3].contiguous().to(dev))
    mid = lambda ns: ns.model.render(ns.out, ns.batch, held_out=(1, 3), radius=1)  # noqa: E731
    after = lambda ns: ns.model.render(ns.out, views=cams, shape=(12, 16))  # noqa: E731
    plain = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True, prepare=batch_colours)
    with_calls = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True, prepare=batch_colours, calls=(mid, after))
    assert_training_untouched(plain, with_calls, "render_views", 2 * steps)
    if not tracking:
        assert all(was for was, _ in with_calls.lazy_kept), "a flow-only training step hands out a LazyExtrinsics: the case must exercise it"
    first, second = with_calls.seen[0], with_calls.seen[1]
    assert first.color.shape == (1, 3, 3, 24, 32) and first.first_frame == 1 and first.offsets == PM2 and float(first.coverage().min()) > 0.5
    assert second.color is None and second.source.shape == (1, 2, 12, 16) and second.first_frame is None


# ---- check 6: memory (GPU) ---------------------------------------------------------------------------------------------------------------------


def case_memory(dev, name="wide"):
    """Peak allocated bytes during a call stay below the outputs + the workspace + one (h, w) float map: no point cloud, no key tensor per
    (view, source).  The workspace: the 64-bit z-buffer, the pose rows — and the call's small tensors: K⁻¹, the pair list."""
    x = {key: v.clone().to(dev) for key, v in case_inputs(name).items()}
    kw, _, _, pairs, (oh, ow), _, _ = call_of(name)
    b, f, h, w = x["depth"].shape
    import flowmap_amd

    flowmap_amd.render_views(x["depth"], x["k"], x["ext"], x["colors"], **kw)  # (warm: libraries loaded, allocator primed)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = flowmap_amd.render_views(x["depth"], x["k"], x["ext"], x["colors"], **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = sum(v.numel() * v.element_size() for v in (r.color, r.depth, r.source))
    n_views = r.source.shape[1]
    round_up = lambda n: (n + 511) // 512 * 512  # noqa: E731  (the caching allocator's granularity)
    workspace = round_up(8 * b * n_views * oh * ow + 64 * b * len(pairs)) + round_up(b * f * 9 * 4) + round_up(len(pairs) * 8)
    slack = 8 * 512  # (each output's and each view tensor's share of the allocator's rounding)
    print(f"  {name}: peak {peak} B; outputs {outputs} B, workspace {workspace} B, one map {h * w * 4} B")
    assert peak <= outputs + workspace + h * w * 4 + slack, f"peak {peak} B > outputs {outputs} + workspace {workspace} + one map {h * w * 4}"


# ---- check 7: psnr, abs_error, coverage ---------------------------------------------------------------------------------------------------------


def case_scores(dev):
    """coverage / psnr / abs_error against a direct numpy evaluation; a held-out render of synth_scene on the ground-truth depth scores a
    higher PSNR than on ``depth_init`` (the colours are a smooth function of the world point, so the frames agree where the depth is right)."""
    import numpy as np
    import pytest

    import flowmap_amd

    f, h, w = 7, 48, 64  # (wide baselines at a fine grid: the 5 % depth noise moves a point by more than the half pixel a splat is off by)
    sc = orc.synth_scene(f, h, w, seed=52)
    k, ext = sc["intrinsics_gt"].expand(1, f, 3, 3).contiguous(), sc["extrinsics_gt"][None]
    xy = orc.pixel_grid((h, w))[0]
    world = orc.matvec(ext[:, :, None, None], orc.append_one(orc.lift(xy, sc["depth_gt"][None], k[:, :, None, None])))[..., :3]
    videos = (0.5 + 0.5 * torch.sin(6.0 * world + torch.tensor([0.0, 1.0, 2.0]))).permute(0, 1, 4, 2, 3).contiguous()
    scores = {}
    for which in ("depth_gt", "depth_init"):
        r = flowmap_amd.render_views(sc[which][None].to(dev), k.to(dev), ext.to(dev), videos.to(dev), held_out=slice(2, 5), offsets=(-3, 3))
        images = videos[:, 2:5]
        color, source = r.color.cpu().double().numpy(), r.source.cpu().numpy()
        covered = source >= 0
        want_cov = covered.reshape(1, 3, -1).mean(axis=2)
        diff = np.where(covered[:, :, None], color - images.double().numpy(), 0.0)
        count = 3.0 * covered.reshape(1, 3, -1).sum(axis=2)
        want_psnr = -10.0 * np.log10((diff**2).reshape(1, 3, -1).sum(axis=2) / count)
        want_abs = np.abs(diff).reshape(1, 3, -1).sum(axis=2) / count
        got = r.coverage(), r.psnr(images.to(dev)), r.abs_error(images.to(dev))
        assert all(g.dtype == torch.float64 and tuple(g.shape) == (1, 3) for g in got)
        for g, want, what in zip(got, (want_cov, want_psnr, want_abs), ("coverage", "psnr", "abs_error")):
            assert np.allclose(g.cpu().numpy(), want, rtol=1e-12, atol=0.0), f"{which}: {what} {g.cpu().numpy()} vs {want}"
        assert float(r.coverage().min()) > 0.5
        scores[which] = r.psnr(images.to(dev)).cpu()
        print(f"  held-out PSNR on {which}: {[round(float(v), 2) for v in scores[which][0]]} dB at coverage {[round(float(v), 3) for v in r.coverage()[0]]}")
    assert bool((scores["depth_gt"] > scores["depth_init"]).all()), "the ground-truth depth must score higher than the noisy one"
    with pytest.raises(RuntimeError, match="flowmap_amd: RenderedViews: images of shape"):
        r.psnr(videos.to(dev))
    bare = flowmap_amd.render_views(sc["depth_gt"][None].to(dev), k.to(dev), ext.to(dev), held_out=(0, 1))
    with pytest.raises(RuntimeError, match="flowmap_amd: RenderedViews: there is no colour"):
        bare.psnr(videos[:, :1].to(dev))
    empty = flowmap_amd.render_views(sc["depth_gt"][None].to(dev), k.to(dev), ext.to(dev), videos.to(dev), held_out=(0, 1), offsets=(1,), near=1e6)
    assert float(empty.coverage()) == 0.0 and bool(torch.isnan(empty.psnr(videos[:, :1].to(dev))).all())


def case_model_render(dev):
    """Model.render: the colours come from batch.videos when a batch is given."""
    import flowmap_amd
    from flowmap_amd import Batch, ModelOutput
    from flowmap_amd.model.model import Model
    from flowmap_amd.model.projection import LazySurfaces

    x = {key: v.clone().to(dev) for key, v in case_inputs("vec").items()}
    out = ModelOutput(x["depth"], LazySurfaces(x["depth"], x["k"]), x["k"], x["ext"], None)
    direct = flowmap_amd.render_views(x["depth"], x["k"], x["ext"], x["colors"], held_out=(2, 3))
    same_render(Model.render(None, out, Batch(x["colors"]), held_out=(2, 3)), direct, "Model.render: ")
    bare = Model.render(None, out, held_out=(2, 3))
    assert bare.color is None and torch.equal(bare.source, direct.source)
    flowmap_amd.set_lazy_surfaces(False)
