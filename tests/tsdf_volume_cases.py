"""export.tsdf_volume / Model.tsdf / TsdfVolume.surface_points (fm_tsdf_volume, fm_tsdf_surface_count, fm_tsdf_surface_emit): the depth maps
fused into a truncated-signed-distance grid, one thread per voxel, and the grid's zero crossings as oriented points.  The cases here take a
device; tests/test_hostsim_tsdf_volume.py runs them on the serial host double of the C ABI, tests/test_gpu_tsdf_volume.py on the MI355X.

Truths.  tests/golden/fn_tsdf_volume.npz holds what the REFERENCE computes (tools/make_golden_tsdf_volume.py: its own homogenize_points,
transform_world2cam and project_camera_space) in fp32 and fp64 — per (voxel, frame) uv and p.z — for the cases small enough to commit; at
every shape the same two evaluations come from the oracle (oracle/flowmap_oracle.py: append_one, matvec, pinhole — restated in ``evaluate``
below), computed once per case.  The world-to-camera pose is formed in fp64 and, for fp32, rounded once.

The gate on a decision is exact and leaves nothing out (``check_volume``, after render_views_cases.check_render).  With the fp64 evaluation,
DELTA = 1e-4 of a pixel and RHO = 1e-5, an observation (voxel, frame) is FIRM when its outcome — skipped as behind `near`, skipped as outside
the frame, skipped for its depth or mask, skipped as hidden, or taken from a given pixel — is the same for every shift of (u·W, v·H) by up to
DELTA, and with p.z, near and the ``sdf >= −truncation`` test each moved by a factor (1 ± RHO): |p.z − near| > RHO·(|p.z| + near); the pixel
position either further than DELTA outside the frame on some axis, or inside with both coordinates further than DELTA from an integer;
|sdf + truncation| > RHO·(|p.z| + truncation).  Otherwise it is OPEN.  A voxel with only firm observations is DECIDED: its ``weight`` must
equal the fp64 count exactly and its ``tsdf`` is compared with the fp64 value under conftest.assert_close_or_reference_gap (rel 1e-4, slack
2x the fp32 oracle's own gap, norm-wise over the decided voxels).  A voxel with open observations must satisfy firm count <= weight <=
firm + open count, tsdf in [−1, 1], color in [0, 1].  The colour hangs on one more comparison, ``sdf <= truncation``, which no fp32 build
can reproduce where |sdf − truncation| <= RHO·(|p.z| + truncation): a decided voxel all of whose taken observations pass that margin too is
COLOUR-DECIDED — ``color_weight`` exact, ``color`` compared like tsdf —, any other voxel has its color_weight between the firm and the
firm + open colour counts.  Each case asserts, from the fp64 oracle alone, that at most 1 % of its voxels are undecided.

``surface_points`` is fed the same build's own volume, so its decisions are comparisons of identical floats: the set of ``edge`` ids and
their order must be exactly those of the numpy restatement (``restate_surface``); xyz, normals and rgb are compared with the fp64
evaluation of the same volume within bounds derived here, with u = 2⁻²⁴:
  xyz      6 ulp(M) per axis, M = max(|origin|, |origin + n·voxel_size|) the largest magnitude on that axis: the centre costs two
           roundings (the product (i + 0.5)·voxel_size and the sum), s = t0/(t0 − t1) two relative ones which voxel_size <= 2M turns into at
           most 4 ulp(M), the product s·voxel_size and the final sum half an ulp each;
  rgb      6u absolute: colours lie in [0, 1], c0 + s·(c1 − c0) is a subtraction, s (2u relative), a product and a sum;
  normals  per component 24u·‖G‖/L + 4u, G the component-wise maximum of the two ends' |gradients| and L the fp64 length of the lerped
           gradient n: a gradient component is one subtraction (the halving is exact), so it is off by u·G; the lerp g0 + s·(g1 − g0) adds
           a subtraction, s, a product and a sum — 12u·G_a per component in all; normalising turns ‖δn‖ into at most 2‖δn‖/L, and the
           squares, their sum, the root and the division are four more roundings of a component that is at most 1.  Where the bound
           reaches 2 it says nothing (the lerp cancelled): any unit vector, or zero, passes.
The worst measured fraction of each bound is printed per case (DESIGN.md §3.1e records them).

Inputs: oracle.synth_scene (``depth_init``, ground-truth poses and K), seeded random colours; ``edge`` and ``plane`` are hand-built.  The
grid of a scene case has the stated dims and encloses the scene's world points; truncation is 4 voxels and near 0 unless the case says so.
A workgroup owns T = 256 consecutive voxels, x fastest; the frames are not chunked (the per-frame constants are scalar loads), so there is
no F = chunk case.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

from conftest import assert_close_or_reference_gap, load_golden, relerr, t
from operator_checks import FRAMES, HEIGHT, WIDTH, assert_training_untouched, batch_colours, c_entry_refuses, host_tensor_refused, same_tensors, train
from oracle import flowmap_oracle as orc

T = 256  # voxels per workgroup (fm_residual_args.h: kTsdfTile)
DELTA, RHO = 1e-4, 1e-5
U = 2.0**-24
FIELDS = ("tsdf", "weight", "color", "color_weight", "world_to_camera")
SCALARS = ("origin", "voxel_size", "truncation", "near", "frames")

# name -> (scene (frames, h, w), seed), dims (nx, ny, nz), what the case changes
SPECS = {
    "tiny": (((2, 5, 7), 41), (5, 3, 2), {}),  # 30 voxels: fewer than a wavefront; h·w = 35 is no multiple of 4
    "part": (((2, 5, 7), 41), (9, 7, 5), {}),  # 315 voxels: a partial second workgroup
    "row64": (((4, 9, 12), 45), (64, 8, 4), {}),  # a wavefront exactly on a row
    "row65": (((4, 9, 12), 45), (65, 8, 4), {}),  # one voxel past it: rows drift through the wavefronts
    "one": (((4, 9, 12), 45), (16, 4, 4), {}),  # exactly one workgroup
    "one1": (((4, 9, 12), 45), (257, 1, 1), {}),  # one voxel more
    "wrap": (((6, 17, 23), 42), (33, 21, 13), {}),  # rows wrap inside wavefronts; h·w = 391 is odd
    "vec": (((7, 24, 32), 43), (64, 24, 16), {}),
    "wide": (((5, 64, 128), 44), (128, 64, 32), {}),  # 1024 workgroups
    "window": (((6, 17, 23), 42), (33, 21, 13), dict(frames=(2, 3))),  # a window in the middle of the video
    "keep": (((6, 17, 23), 42), (33, 21, 13), dict(keep=0.7)),  # a mask that keeps about 70 % of the pixels
    "spoil": (((6, 17, 23), 42), (33, 21, 13), dict(spoil=True)),  # depths that are NaN, +inf, 0 and negative
    "nocolor": (((2, 5, 7), 41), (9, 7, 5), dict(colors=False)),
    "edge": (((4, 9, 12), 47), (12, 10, 8), dict(near=1.9)),  # render_views_cases' edge scene: a rotation by pi, everything behind one camera
    "behind": (((4, 9, 12), 45), (16, 8, 4), dict(behind=True)),  # a grid behind every camera: weight 0, tsdf exactly 1, no surface
}
GOLDEN_CASES = ("part", "edge")
INPUT_KEYS = ("depth", "k", "ext", "colors")


@functools.lru_cache(maxsize=None)
def scene_inputs(shape, seed, kind):
    f, h, w = shape
    colors = torch.rand((f, 3, h, w), generator=torch.Generator().manual_seed(1000 + seed))
    if kind == "edge":  # (the edge scene of render_views_cases / depth_consistency_cases: a rotation by pi about y, two translations)
        depth = 1.5 + torch.rand((f, h, w), generator=torch.Generator().manual_seed(seed))
        k = orc.focal_to_k(torch.tensor(0.85), (h, w)).expand(f, 3, 3).contiguous()
        ext = torch.eye(4).repeat(f, 1, 1)
        ext[1, 0, 0] = ext[1, 2, 2] = -1.0
        ext[2, :3, 3] = torch.tensor([1.0, 0.0, 0.0])
        ext[3, :3, 3] = torch.tensor([0.0, -0.7, 0.3])
        return {"depth": depth, "k": k, "ext": ext, "colors": colors}
    sc = orc.synth_scene(f, h, w, seed=seed)
    return {"depth": sc["depth_init"].clone(), "k": sc["intrinsics_gt"].expand(f, 3, 3).contiguous(), "ext": sc["extrinsics_gt"].clone(), "colors": colors}


def world_points(x):
    xy = orc.pixel_grid(tuple(x["depth"].shape[1:]), dtype=torch.float64)[0]
    p = orc.lift(xy, x["depth"].double(), x["k"].double()[:, None, None])
    return orc.matvec(x["ext"].double()[:, None, None], orc.append_one(p))[..., :3].reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def case_of(name):
    """-> (inputs, call): inputs depth (F,h,w), k, ext, colors (F,3,h,w) or None, keep or None; call = the keyword arguments of tsdf_volume
    plus voxel_size (tools/make_golden_tsdf_volume.py draws them from here)."""
    (shape, seed), dims, change = SPECS[name]
    x = dict(scene_inputs(shape, seed, "edge" if name == "edge" else "scene"))
    seen = {key: v[[0, 2, 3]] for key, v in x.items()} if name == "edge" else x  # (edge: the frames that look along +z; frame 1 looks away)
    points = world_points(seen)  # (of the clean depths: the grid does not move with what a case spoils)
    low, high = points.min(dim=0).values, points.max(dim=0).values
    voxel_size = float(np.float32(1.001 * float(((high - low) / torch.tensor(dims, dtype=torch.float64)).max())))
    centre = 0.5 * (low + high)
    if change.get("behind"):  # (behind the mean camera, along its mean viewing direction, by more than the grid's diagonal)
        forward = x["ext"][:, :3, 2].double().mean(dim=0)
        reach = float(torch.tensor(dims, dtype=torch.float64).norm()) * voxel_size + 2.0
        centre = x["ext"][:, :3, 3].double().mean(dim=0) - forward / forward.norm() * reach
    origin = tuple(float(np.float32(float(c) - 0.5 * n * voxel_size)) for c, n in zip(centre, dims))
    x["keep"] = None
    if "keep" in change:
        x["keep"] = torch.rand(x["depth"].shape, generator=torch.Generator().manual_seed(seed + 7)) < change["keep"]
    if change.get("spoil"):
        x["depth"] = x["depth"].clone()
        flat = x["depth"].reshape(-1)
        at = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed + 9))[:80]
        flat[at[:20]], flat[at[20:40]], flat[at[40:60]], flat[at[60:]] = float("nan"), float("inf"), 0.0, -1.5
    if change.get("colors") is False:
        x["colors"] = None
    call = dict(voxel_size=voxel_size, origin=origin, dims=dims, truncation=float(np.float32(4.0 * voxel_size)), near=float(np.float32(change.get("near", 0.0))),
                frames=change.get("frames"))
    return x, call


def window_of(call, f):
    return (0, f) if call["frames"] is None else tuple(call["frames"])


# ---- the oracle's composition -----------------------------------------------------------------------------------------------------------------


def centres(call, dtype):
    """(V, 3) voxel centres, x fastest, from the float32 origin and voxel_size, evaluated in ``dtype``."""
    nx, ny, nz = call["dims"]
    axes = [torch.tensor(o, dtype=dtype) + (torch.arange(n, dtype=dtype) + 0.5) * torch.tensor(call["voxel_size"], dtype=dtype) for o, n in zip(call["origin"], (nx, ny, nz))]
    gz, gy, gx = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return torch.stack((gx, gy, gz), dim=-1).reshape(-1, 3)


def evaluate(x, call, dtype, fns=None):
    """uv (V, F, 2) and p.z (V, F) of every voxel against every frame of the video in ``dtype`` by the oracle's functions (``fns``: the
    reference's own, in tools/make_golden_tsdf_volume.py)."""
    homogeneous, to_camera, project = fns or (orc.append_one, lambda p, e: orc.matvec(torch.linalg.inv(e.double()).to(e.dtype), p), orc.pinhole)
    c = centres(call, dtype)
    p = to_camera(homogeneous(c)[:, None], x["ext"].to(dtype)[None])[..., :3]
    return {"uv": project(p, x["k"].to(dtype)[None]), "pz": p[..., 2]}


def outcomes(ev, x, call):
    """The evaluation's own decisions per (voxel, frame) of the window and, for the fp64 one, their firmness.
    -> dict of (V, Fw) tensors: taken, coloured, t (the term, 0 where not taken), colour (V, Fw, 3), firm (decision robust), colour_firm."""
    f, h, w = x["depth"].shape
    first, count = window_of(call, f)
    uv, pz = ev["uv"][:, first:first + count].double(), ev["pz"][:, first:first + count].double()
    near, trunc = call["near"], call["truncation"]
    px, py = uv[..., 0] * w, uv[..., 1] * h
    front = pz > near
    inside = (uv[..., 0] >= 0) & (uv[..., 0] < 1) & (uv[..., 1] >= 0) & (uv[..., 1] < 1)
    col = torch.floor(px).clamp(0, w - 1).nan_to_num(0).long()
    row = torch.floor(py).clamp(0, h - 1).nan_to_num(0).long()
    frame = torch.arange(first, first + count)[None].expand_as(col)
    d = x["depth"].double()[frame, row, col]
    kept = torch.ones_like(front) if x["keep"] is None else x["keep"][frame, row, col]
    valid = torch.isfinite(d) & (d > 0) & kept
    sdf = d - pz
    seen = valid & (sdf >= -trunc)
    taken = front & inside & seen
    coloured = taken & (sdf <= trunc)
    term = torch.where(taken, (sdf / trunc).clamp_max(1.0), torch.zeros_like(sdf))
    colour = None if x["colors"] is None else torch.where(coloured[..., None], x["colors"].double().permute(0, 2, 3, 1)[frame, row, col], torch.zeros(1, dtype=torch.float64))
    # firmness (meaningful for the fp64 evaluation)
    near_firm = (pz - near).abs() > RHO * (pz.abs() + near)
    away = lambda p, n: (p < -DELTA) | (p > n + DELTA)  # noqa: E731
    clear = lambda p: (p - torch.round(p)).abs() > DELTA  # noqa: E731
    out_firm = away(px, w) | away(py, h)
    in_firm = inside & clear(px) & clear(py)
    margin = RHO * (pz.abs() + trunc)
    hidden_firm = (sdf + trunc).abs() > margin
    firm = (near_firm & ~front) | (near_firm & front & (out_firm | (in_firm & (~valid | hidden_firm))))
    colour_firm = firm & (~taken | ((sdf - trunc).abs() > margin))
    return {"taken": taken, "coloured": coloured, "t": term, "colour": colour, "firm": firm, "colour_firm": colour_firm}


def fuse(o, dtype):
    """weight, tsdf, color_weight, color of the decisions ``o`` with sums in ``dtype``, in frame order."""
    weight = o["taken"].sum(dim=1)
    total = torch.zeros(o["t"].shape[0], dtype=dtype)
    for j in range(o["t"].shape[1]):
        total = total + o["t"][:, j].to(dtype)
    tsdf = torch.where(weight > 0, total / weight.clamp_min(1).to(dtype), torch.ones_like(total))
    if o["colour"] is None:
        return weight, tsdf, None, None
    cw = o["coloured"].sum(dim=1)
    sums = torch.zeros((o["t"].shape[0], 3), dtype=dtype)
    for j in range(o["t"].shape[1]):
        sums = sums + o["colour"][:, j].to(dtype)
    return weight, tsdf, cw, torch.where(cw[:, None] > 0, sums / cw.clamp_min(1).to(dtype)[:, None], torch.zeros_like(sums))


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    x, call = case_of(name)
    return evaluate(x, call, torch.float32), evaluate(x, call, torch.float64)


def check_volume(v, x, call, ev32, ev64, what, cap=0.01):
    """The gate of the module docstring on a TsdfVolume -> (undecided voxels, decided voxels)."""
    nx, ny, nz = call["dims"]
    f = x["depth"].shape[0]
    o64, o32 = outcomes(ev64, x, call), outcomes(ev32, x, call)
    w64, t64, cw64, c64 = fuse(o64, torch.float64)
    _, t32, _, c32 = fuse(o32, torch.float32)
    open_obs = ~o64["firm"]
    n_open = open_obs.sum(dim=1)
    decided = n_open == 0
    undecided = int((~decided).sum())
    assert undecided <= cap * decided.numel(), f"{what}: {undecided} of {decided.numel()} voxels are undecided in fp64: the case is ill-conditioned"
    assert v.tsdf.dtype == torch.float32 and tuple(v.tsdf.shape) == (nz, ny, nx) and v.weight.dtype == torch.int32 and tuple(v.weight.shape) == (nz, ny, nx)
    assert v.dims == (nx, ny, nz) and v.frames == window_of(call, f) and tuple(v.world_to_camera.shape) == (f, 4, 4)
    assert v.origin == tuple(call["origin"]) and v.voxel_size == call["voxel_size"] and v.truncation == call["truncation"] and v.near == call["near"]
    assert relerr(v.world_to_camera.cpu(), torch.linalg.inv(x["ext"].double())) < 1e-6, f"{what}: world_to_camera is not the inverse of the extrinsics"
    tsdf, weight = v.tsdf.cpu().reshape(-1), v.weight.cpu().reshape(-1).long()
    assert bool(torch.equal(weight[decided], w64[decided])), f"{what}: {int((weight[decided] != w64[decided]).sum())} decided voxels have another weight than the fp64 count"
    firm_taken = (o64["taken"] & o64["firm"]).sum(dim=1)
    assert bool(((weight >= firm_taken) & (weight <= firm_taken + n_open)).all()), f"{what}: a weight outside [firm, firm + open]"
    assert bool(((tsdf >= -1) & (tsdf <= 1)).all()), f"{what}: tsdf outside [-1, 1]"
    assert bool((tsdf[weight == 0] == 1).all()), f"{what}: tsdf is not exactly 1 where weight is 0"
    e, gap = assert_close_or_reference_gap(tsdf[decided], t64[decided], t32[decided], rel=1e-4, slack=2.0, what=f"{what}.tsdf")
    print(f"  {what}.tsdf: err {e:.2e} (fp32 oracle's own gap {gap:.2e}) over {int(decided.sum())} decided voxels, {undecided} undecided, "
          f"{int((weight > 0).sum())} observed")
    if x["colors"] is None:
        assert v.color is None and v.color_weight is None
        return undecided, int(decided.sum())
    assert v.color.dtype == torch.float32 and tuple(v.color.shape) == (nz, ny, nx, 3) and v.color_weight.dtype == torch.int32
    color, cw = v.color.cpu().reshape(-1, 3), v.color_weight.cpu().reshape(-1).long()
    c_open = (~o64["colour_firm"]).sum(dim=1)
    c_decided = c_open == 0
    assert bool(torch.equal(cw[c_decided], cw64[c_decided])), f"{what}: a colour-decided voxel has another color_weight than the fp64 count"
    c_firm = (o64["coloured"] & o64["colour_firm"]).sum(dim=1)
    assert bool(((cw >= c_firm) & (cw <= c_firm + c_open)).all()), f"{what}: a color_weight outside [firm, firm + open]"
    assert bool(((color >= 0) & (color <= 1)).all()) and bool((color[cw == 0] == 0).all()) and bool((cw <= weight).all())
    if int(c_decided.sum()):
        e, gap = assert_close_or_reference_gap(color[c_decided], c64[c_decided], c32[c_decided], rel=1e-4, slack=2.0, what=f"{what}.color")
        print(f"  {what}.color: err {e:.2e} (fp32 oracle's own gap {gap:.2e}) over {int(c_decided.sum())} colour-decided voxels")
    return undecided, int(decided.sum())


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------


def run(name, dev, x=None, call=None, **changed):
    import flowmap_amd

    cx, ccall = case_of(name)
    x, call = x or cx, {**(call or ccall), **changed}
    y = {key: (None if v is None else v.clone().to(dev)) for key, v in x.items()}
    kw = {key: v for key, v in call.items() if key != "voxel_size"}
    return flowmap_amd.tsdf_volume(y["depth"], y["k"], y["ext"], y["colors"], call["voxel_size"], keep=y["keep"], **kw)


def same_volume(a, b, what=""):
    same_tensors(a, b, FIELDS, what, scalars=SCALARS)


def same_surface(a, b, what=""):
    for name, p, q in zip(("xyz", "normals", "rgb", "edge"), a, b):
        assert (p is None) == (q is None), f"{what}{name}"
        if p is not None:
            assert p.dtype == q.dtype and p.shape == q.shape and torch.equal(p.cpu(), q.cpu()), f"{what}{name}: not bit-equal"


# ---- check 1: oracle and reference parity -------------------------------------------------------------------------------------------------------


def case_oracle_parity(dev, name):
    x, call = case_of(name)
    ev32, ev64 = oracle_case(name)
    v = run(name, dev)
    undecided, decided = check_volume(v, x, call, ev32, ev64, name)
    weight = v.weight.cpu()
    if name == "behind":
        assert int(weight.sum()) == 0 and bool((v.tsdf == 1).all()), "a grid behind every camera is seen by none"
        assert all(r.shape[0] == 0 for r in v.surface_points() if r is not None)
    elif name == "edge":
        alone = run(name, dev, frames=(1, 1))
        assert int(alone.weight.sum()) == 0, "edge: frame 1 looks the other way: everything is behind it"
        assert int(run(name, dev, near=0.0).weight.sum()) > int(weight.sum()) > 0, "edge: near must cut some observations"
    else:
        assert int((weight > 0).sum()) > 0 and bool((v.tsdf.cpu()[weight > 0] < 0).any()), f"{name}: the grid must straddle the surface"
    if name == "window":
        full = run(name, dev, frames=None)
        assert v.frames == (2, 3) and int(v.weight.max()) <= 3 < int(full.weight.max())
        assert torch.equal(v.world_to_camera, full.world_to_camera)
        assert same_volume(run(name, dev, frames=slice(2, 5)), v, "slice: ") is None
    if name == "keep":
        assert int(run(name, dev, x={**x, "keep": None}).weight.sum()) > int(weight.sum())
    if name == "spoil":
        assert int(run("wrap", dev).weight.sum()) > int(weight.sum()), "spoilt depths must cost observations"
    return v


def case_well_conditioned(name):
    """From the fp64 oracle alone: at most 1 % of the voxels are undecided."""
    x, call = case_of(name)
    o = outcomes(oracle_case(name)[1], x, call)
    share = float(((~o["firm"]).sum(dim=1) > 0).double().mean())
    print(f"  {name}: {share:.4%} of the voxels are undecided")
    assert share <= 0.01, f"{name}: {share:.3%} of the voxels are undecided: take another seed"


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("fn_tsdf_volume")


def case_reference_parity(dev, name):
    """A fixture case against what the imported reference computed: its fp64 evaluation the truth, its fp32 evaluation the gap."""
    g = golden()
    x, call = case_of(name)
    gx = {key: t(g[f"{name}_{key}"]) for key in INPUT_KEYS}  # (a scene drawn on another machine may differ in the last bits of sin / cos)
    for key in INPUT_KEYS:
        assert relerr(x[key], gx[key]) < 1e-6, f"{name}: the fixture's {key} is not the case's"
    gx["keep"] = x["keep"]
    gcall = {**call, "voxel_size": float(g[f"{name}_voxel_size"]), "origin": tuple(float(o) for o in g[f"{name}_origin"]), "truncation": float(g[f"{name}_truncation"])}
    assert tuple(g[f"{name}_dims"].tolist()) == tuple(call["dims"]) and abs(gcall["voxel_size"] - call["voxel_size"]) <= 1e-6 * call["voxel_size"]
    ev32 = {"uv": t(g[f"{name}_uv"]), "pz": t(g[f"{name}_pz"])}
    ev64 = {"uv": t(g[f"{name}_f64_uv"]), "pz": t(g[f"{name}_f64_pz"])}
    mine = evaluate(gx, gcall, torch.float64)
    assert relerr(mine["pz"], ev64["pz"]) < 1e-12 and relerr(mine["uv"], ev64["uv"]) < 1e-9, "the reference and the oracle agree in fp64"
    v = run(name, dev, x=gx, call=gcall)
    check_volume(v, gx, gcall, ev32, ev64, f"{name} vs the reference")


# ---- check 2: the builds against themselves and each other ----------------------------------------------------------------------------------------


def case_repeatable(dev, name):
    """Two calls are bit-equal in every field, and so are their surfaces."""
    a, b = run(name, dev), run(name, dev)
    same_volume(a, b, f"{name} twice: ")
    same_surface(a.surface_points(), b.surface_points(), f"{name} surface twice: ")


def case_gpu_against_host_double(dev, name):
    """Both builds evaluate the same written-out form (fm_math.h: tsdf_pixel_of), so each passes the gate; on ``plane`` they are bit-equal
    (case_plane).  Here: the two agree on weight wherever the fp64 oracle is decided."""
    from flowmap_amd import _lib
    from helpers import build_host_sim

    gpu = run(name, dev)
    _lib.set_library_for_testing(build_host_sim())
    try:
        host = run(name, "cpu")
    finally:
        _lib.set_library_for_testing(None)
    x, call = case_of(name)
    ev32, ev64 = oracle_case(name)
    for v, what in ((gpu, f"gpu {name}"), (host, f"host {name}")):
        check_volume(v, x, call, ev32, ev64, what)
    differ = int((gpu.weight.cpu() != host.weight).sum())
    print(f"  GPU vs host double, {name}: {differ} weights differ, tsdf max |diff| {float((gpu.tsdf.cpu() - host.tsdf).abs().max()):.3e}")


# ---- check 3: the plane, exact arithmetic ------------------------------------------------------------------------------------------------------------

PLANE = dict(frames=3, h=4, w=6, voxel_size=0.125, truncation=0.4375, origin=(-0.25, -0.25, 1.375), dims=(4, 4, 10), colour=(0.25, 0.5, 0.75))


def plane_inputs():
    """Identity poses, K with focal 1 and centre 0.5, depth exactly 2, constant colours: p.z is the centre's z, d − p.z an exact multiple of
    2⁻⁴ whichever pixel a voxel lands in.  Centres at z = 1.4375, 1.5625, … 2.5625: sdf runs from +truncation + one step (t = 1, no colour)
    through +truncation (t = 1, coloured), +0.0625 / −0.0625 (the crossing at z = 2, s = 0.5) and −truncation (taken, t = −1) to
    −truncation − one step (hidden: weight 0)."""
    p = PLANE
    f, h, w = p["frames"], p["h"], p["w"]
    k = torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]).expand(f, 3, 3).contiguous()
    colors = torch.tensor(p["colour"]).reshape(1, 3, 1, 1).expand(f, 3, h, w).contiguous()
    return {"depth": torch.full((f, h, w), 2.0), "k": k, "ext": torch.eye(4).repeat(f, 1, 1), "colors": colors, "keep": None}


def plane_closed_form():
    p = PLANE
    nx, ny, nz = p["dims"]
    f = p["frames"]
    z = np.float32(p["origin"][2]) + (np.arange(nz, dtype=np.float32) + np.float32(0.5)) * np.float32(p["voxel_size"])
    sdf = np.float32(2.0) - z
    trunc = np.float32(p["truncation"])
    taken, coloured = sdf >= -trunc, (sdf >= -trunc) & (sdf <= trunc)
    term = np.minimum(sdf / trunc, np.float32(1.0)).astype(np.float32)
    total = np.zeros(nz, dtype=np.float32)
    for _ in range(f):
        total = (total + term).astype(np.float32)
    tsdf = np.where(taken, total / np.float32(f), np.float32(1.0)).astype(np.float32)
    shape = (nz, ny, nx)
    colour = np.where(coloured[:, None], np.array(p["colour"], dtype=np.float32)[None], np.float32(0.0))
    volume = dict(tsdf=np.broadcast_to(tsdf[:, None, None], shape), weight=np.broadcast_to(np.where(taken, f, 0).astype(np.int32)[:, None, None], shape),
                  color=np.broadcast_to(colour[:, None, None, :], shape + (3,)), color_weight=np.broadcast_to(np.where(coloured, f, 0).astype(np.int32)[:, None, None], shape))
    k0 = int(np.nonzero(z == np.float32(1.9375))[0][0])
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    voxel = ((k0 * ny + jj) * nx + ii).reshape(-1)
    cx = np.float32(p["origin"][0]) + (ii.reshape(-1).astype(np.float32) + np.float32(0.5)) * np.float32(p["voxel_size"])
    cy = np.float32(p["origin"][1]) + (jj.reshape(-1).astype(np.float32) + np.float32(0.5)) * np.float32(p["voxel_size"])
    surface = dict(edge=voxel.astype(np.int64) * 3 + 2, xyz=np.stack((cx, cy, np.full_like(cx, 2.0)), axis=1).astype(np.float32),
                   normals=np.tile(np.array([[0.0, 0.0, -1.0]], dtype=np.float32), (len(voxel), 1)),
                   rgb=np.tile(np.array([p["colour"]], dtype=np.float32), (len(voxel), 1)))
    return volume, surface


def run_plane(dev):
    import flowmap_amd

    p = PLANE
    y = {key: (None if v is None else v.to(dev)) for key, v in plane_inputs().items()}
    return flowmap_amd.tsdf_volume(y["depth"], y["k"], y["ext"], y["colors"], p["voxel_size"], origin=p["origin"], dims=p["dims"], truncation=p["truncation"])


def case_plane(dev, against_host=False):
    """Volume, crossings (z = 2 exactly, s = 0.5) and normals (0, 0, −1) against the closed form bit for bit; with ``against_host`` (GPU)
    the host double too."""
    volume, surface = plane_closed_form()
    v = run_plane(dev)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    assert set(np.unique(volume["weight"])) == {0, 3} and {-1.0, 1.0} <= set(np.unique(volume["tsdf"]).tolist()), "the case must hold t = −1, t = 1 and a hidden layer"
    assert int((volume["color_weight"] != volume["weight"]).sum()) > 0, "the case must hold an uncoloured layer beyond +truncation"
    for name in ("tsdf", "color"):
        assert np.array_equal(bits(getattr(v, name).cpu().numpy()), bits(volume[name])), f"plane: {name} is not the closed form bit for bit"
    for name in ("weight", "color_weight"):
        assert np.array_equal(getattr(v, name).cpu().numpy(), volume[name]), f"plane: {name}"
    xyz, normals, rgb, edge = v.surface_points()
    assert np.array_equal(edge.cpu().numpy(), surface["edge"]) and edge.dtype == torch.int64
    for got, name in ((xyz, "xyz"), (normals, "normals"), (rgb, "rgb")):
        assert np.array_equal(bits(got.cpu().numpy()), bits(surface[name])), f"plane: surface {name} is not the closed form bit for bit"
    assert v.surface_points(min_weight=3)[3].shape[0] == len(surface["edge"]) and v.surface_points(min_weight=4)[3].shape[0] == 0
    if against_host:
        from flowmap_amd import _lib
        from helpers import build_host_sim

        _lib.set_library_for_testing(build_host_sim())
        try:
            host = run_plane("cpu")
            host_surface = host.surface_points()
        finally:
            _lib.set_library_for_testing(None)
        same_tensors(v, host, FIELDS, "plane, GPU vs host double: ", scalars=SCALARS, equal=lambda a, b: torch.equal(a.cpu(), b.cpu()))
        same_surface(v.surface_points(), host_surface, "plane surface, GPU vs host double: ")


# ---- check 4: surface_points against the restatement ----------------------------------------------------------------------------------------------


def restate_surface(tsdf, weight, color, color_weight, origin, voxel_size, min_weight):
    """The zero crossings of a volume (numpy arrays of the build's own output) in fp64: edge (M,) ascending, xyz, normals, rgb (M, 3) and
    per row the normal's bound ingredients (‖G‖, L)."""
    nz, ny, nx = tsdf.shape
    t64 = tsdf.astype(np.float64)
    ok = weight >= min_weight
    size = {0: nx, 1: ny, 2: nz}
    ax = {0: 2, 1: 1, 2: 0}  # axis of the (nz, ny, nx) arrays that world axis a runs along

    def shift(a, axis, by):  # a[index + by] along world axis `axis`, edge-padded
        return np.take(a, np.clip(np.arange(size[axis]) + by, 0, size[axis] - 1), axis=ax[axis])

    grad = np.zeros(tsdf.shape + (3,))
    for a in range(3):
        index = np.arange(size[a]).reshape([-1 if d == ax[a] else 1 for d in range(3)])
        lo, hi = shift(ok, a, -1) & (index > 0), shift(ok, a, 1) & (index < size[a] - 1)
        below, above = np.where(lo, shift(t64, a, -1), t64), np.where(hi, shift(t64, a, 1), t64)
        grad[..., a] = np.where(lo & hi, 0.5, 1.0) * (above - below)
    rows = []
    linear = np.arange(nz * ny * nx).reshape(nz, ny, nx)
    for a in range(3):
        index = np.arange(size[a]).reshape([-1 if d == ax[a] else 1 for d in range(3)])
        cross = (index < size[a] - 1) & ok & shift(ok, a, 1) & ((tsdf < 0) != (shift(tsdf, a, 1) < 0))
        rows.append(np.stack((linear[cross] * 3 + a, linear[cross], np.full(int(cross.sum()), a)), axis=1))
    rows = np.concatenate(rows)
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    edge, voxel, axis = rows[:, 0], rows[:, 1], rows[:, 2]
    stride = np.array([1, nx, nx * ny])[axis]
    other = voxel + stride
    flat_t, flat_g = t64.reshape(-1), grad.reshape(-1, 3)
    t0, t1 = flat_t[voxel], flat_t[other]
    s = t0 / (t0 - t1)
    ijk = np.stack((voxel % nx, (voxel // nx) % ny, voxel // (nx * ny)), axis=1)
    xyz = np.asarray(origin, dtype=np.float64)[None] + (ijk + 0.5) * voxel_size
    xyz[np.arange(len(axis)), axis] += s * voxel_size
    g0, g1 = flat_g[voxel], flat_g[other]
    n = g0 + s[:, None] * (g1 - g0)
    length = np.sqrt((n * n).sum(axis=1))
    normals = np.where(length[:, None] > 0, n / np.where(length > 0, length, 1.0)[:, None], 0.0)
    scale = np.sqrt((np.maximum(np.abs(g0), np.abs(g1)) ** 2).sum(axis=1))
    rgb = None
    if color is not None:
        c, cw = color.astype(np.float64).reshape(-1, 3), color_weight.reshape(-1)
        has0, has1 = (cw[voxel] > 0)[:, None], (cw[other] > 0)[:, None]
        rgb = np.where(has0 & has1, c[voxel] + s[:, None] * (c[other] - c[voxel]), np.where(has0, c[voxel], np.where(has1, c[other], 0.0)))
    return {"edge": edge.astype(np.int64), "xyz": xyz, "normals": normals, "rgb": rgb, "scale": scale, "length": length}


def check_surface(v, min_weight, what):
    """TsdfVolume.surface_points against restate_surface of the same volume -> the worst fractions of the three bounds."""
    xyz, normals, rgb, edge = v.surface_points(min_weight)
    color = None if v.color is None else v.color.cpu().numpy()
    cw = None if v.color is None else v.color_weight.cpu().numpy()
    want = restate_surface(v.tsdf.cpu().numpy(), v.weight.cpu().numpy(), color, cw, v.origin, v.voxel_size, min_weight)
    assert edge.dtype == torch.int64 and np.array_equal(edge.cpu().numpy(), want["edge"]), f"{what}: the edge ids or their order differ from the restatement"
    m = len(want["edge"])
    assert tuple(xyz.shape) == (m, 3) and tuple(normals.shape) == (m, 3) and xyz.dtype == normals.dtype == torch.float32 and (rgb is None) == (v.color is None)
    if m == 0:
        return 0.0, 0.0, 0.0
    nx, ny, nz = v.dims
    extent = np.maximum(np.abs(np.asarray(v.origin)), np.abs(np.asarray(v.origin) + np.array([nx, ny, nz]) * v.voxel_size))
    ulp = 2.0 ** (np.floor(np.log2(extent)) - 23)
    worst_xyz = float((np.abs(xyz.cpu().numpy().astype(np.float64) - want["xyz"]) / (6.0 * ulp[None])).max())
    bound = 24.0 * U * want["scale"] / np.maximum(want["length"], 1e-300) + 4.0 * U
    said = bound < 2.0
    got_n = normals.cpu().numpy().astype(np.float64)
    worst_n = float((np.abs(got_n - want["normals"]).max(axis=1) / bound)[said].max()) if said.any() else 0.0
    lengths = np.sqrt((got_n**2).sum(axis=1))
    assert bool(((np.abs(lengths - 1.0) <= 8 * U) | (lengths == 0)).all()), f"{what}: a normal is neither a unit vector nor zero"
    worst_rgb = 0.0 if rgb is None else float((np.abs(rgb.cpu().numpy().astype(np.float64) - want["rgb"]) / (6.0 * U)).max())
    print(f"  {what}: {m} crossings at min_weight {min_weight}; worst fraction of the bound: xyz {worst_xyz:.3f}, normals {worst_n:.3f} "
          f"({int((~said).sum())} rows where it says nothing), rgb {worst_rgb:.3f}")
    assert worst_xyz <= 1.0 and worst_n <= 1.0 and worst_rgb <= 1.0, f"{what}: xyz {worst_xyz:.3f}, normals {worst_n:.3f}, rgb {worst_rgb:.3f} of the bounds"
    return worst_xyz, worst_n, worst_rgb


def case_surface(dev, name, min_weight=1):
    v = run(name, dev)
    check_surface(v, min_weight, f"{name} surface")
    xyz, normals, rgb, edge = v.surface_points(min_weight)
    if name not in ("behind", "edge", "one1") and min_weight == 1:  # (one1 is a single row along x: it need not cut the surface)
        assert edge.shape[0] > 0, f"{name}: a grid that straddles the surface has crossings"
        toward = (v.world_to_camera[0, :3, :3].T.cpu().double() @ torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64))  # camera 0's −z axis in the world
        assert float((normals.cpu().double() @ toward > 0).double().mean()) > 0.6, f"{name}: the normals must point toward the cameras"
    if min_weight > 1:
        assert 0 < edge.shape[0] < v.surface_points(1)[3].shape[0], f"{name}: min_weight = {min_weight} must drop some crossings and keep some"


SYNTHETIC_DIMS = (8, 8, 13)  # 832 voxels: three workgroups and a quarter; the last layer, z = 12, IS the last workgroup (voxels 768 .. 831)


def synthetic_volume(dev, kind):
    """Hand-made volumes for the count-then-emit edges: ``none`` — no crossing at all; ``last`` — signs change inside the last layer only
    and the layer below it is unobserved, so every crossing starts in the last workgroup; ``every`` — a checkerboard, every edge crosses;
    ``weights`` — the same with weights 0 to 3 drawn per voxel."""
    from flowmap_amd import TsdfVolume

    nx, ny, nz = SYNTHETIC_DIMS
    g = torch.Generator().manual_seed(3)
    k, j, i = torch.meshgrid(torch.arange(nz), torch.arange(ny), torch.arange(nx), indexing="ij")
    board = torch.where((i + j + k) % 2 == 0, 0.1 + 0.8 * torch.rand((nz, ny, nx), generator=g), -0.1 - 0.8 * torch.rand((nz, ny, nx), generator=g))
    tsdf = torch.full((nz, ny, nx), 0.5)
    weight = torch.full((nz, ny, nx), 2, dtype=torch.int32)
    if kind == "last":
        tsdf[nz - 1] = board[nz - 1]
        weight[nz - 2] = 0
    elif kind in ("every", "weights"):
        tsdf = board
        if kind == "weights":
            weight = torch.randint(0, 4, (nz, ny, nx), generator=g, dtype=torch.int32)
    color_weight = torch.randint(0, 3, (nz, ny, nx), generator=g, dtype=torch.int32)
    color = torch.where(color_weight[..., None] > 0, torch.rand((nz, ny, nx, 3), generator=g), torch.zeros(()))
    return TsdfVolume(tsdf.to(dev), weight.to(dev), color.to(dev), color_weight.to(dev), torch.eye(4)[None].to(dev), (-0.4, 0.3, 1.7), 0.1, 0.4, 0.0, (0, 1))


def case_surface_synthetic(dev, kind):
    v = synthetic_volume(dev, kind)
    check_surface(v, 1, f"synthetic {kind}")
    edge = v.surface_points()[3].cpu()
    if kind == "none":
        assert edge.shape[0] == 0 and all(r.shape[0] == 0 for r in v.surface_points())
    if kind == "last":
        assert edge.shape[0] > 0 and int(edge.min()) // 3 >= 3 * T, "every crossing starts in the last workgroup"
    if kind == "every":
        nx, ny, nz = v.dims
        assert edge.shape[0] == (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1), "a checkerboard crosses on every edge"
    if kind == "weights":
        for min_weight in (2, 3):
            check_surface(v, min_weight, f"synthetic weights, min_weight {min_weight}")
        assert v.surface_points(3)[3].shape[0] < v.surface_points(2)[3].shape[0] < edge.shape[0]
        assert v.surface_points(4)[3].shape[0] == 0


# ---- check 5: arguments and refusals -------------------------------------------------------------------------------------------------------------


def case_arguments(dev):
    import pytest

    import flowmap_amd
    from flowmap_amd import TsdfVolume, _ops, export

    x, call = case_of("part")
    y = {key: (None if v is None else v.clone().to(dev)) for key, v in x.items()}
    args = (y["depth"], y["k"], y["ext"], y["colors"])
    grid = dict(origin=call["origin"], dims=call["dims"])
    vs = call["voxel_size"]
    for bad in (0.0, -1.0, float("nan"), float("inf"), None, "0.1", True, 1e-50, 1e39):
        with pytest.raises(ValueError, match="flowmap_amd: tsdf_volume: voxel_size"):
            flowmap_amd.tsdf_volume(*args, bad, **grid)
    for bad in (0.0, -0.5, float("nan"), float("inf"), "1", True, 1e39):
        with pytest.raises(ValueError, match="flowmap_amd: tsdf_volume: truncation"):
            flowmap_amd.tsdf_volume(*args, vs, truncation=bad, **grid)
    for bad in (-1e-3, float("nan"), float("inf"), None, "0", True):
        with pytest.raises(ValueError, match="flowmap_amd: tsdf_volume: near"):
            flowmap_amd.tsdf_volume(*args, vs, near=bad, **grid)
    for bad in ((0.0, 0.0), (0.0, 0.0, float("nan")), (0.0, float("inf"), 0.0), None, "abc", (0.0, 0.0, True), 1.0, (0.0, 0.0, "0")):
        with pytest.raises(ValueError, match="flowmap_amd: tsdf_volume: origin"):
            flowmap_amd.tsdf_volume(*args, vs, origin=bad, dims=call["dims"])
    for bad in ((4, 4), (4, 4, 0), (4, -1, 4), (4.0, 4, 4), None, "444", (True, 4, 4), (2048, 2048, 512), 8):
        with pytest.raises(ValueError, match="flowmap_amd: tsdf_volume: dims"):
            flowmap_amd.tsdf_volume(*args, vs, origin=call["origin"], dims=bad)
    for bad in (slice(0, 2, 2), (0, 0), (1, 2), (-1, 1), (0, 3), "all", 1, (1.0, 1), (0, 1, 1)):
        with pytest.raises(ValueError, match="flowmap_amd: tsdf_volume.*frames"):
            flowmap_amd.tsdf_volume(*args, vs, frames=bad, **grid)
    with pytest.raises(TypeError):
        flowmap_amd.tsdf_volume(*args, vs)  # origin and dims are required
    # what world_point_cloud refuses, refused alike
    for fn in (lambda *a, **kw: export.world_point_cloud(*a, **kw), lambda *a, **kw: flowmap_amd.tsdf_volume(*a, vs, **grid, **kw)):
        with pytest.raises(RuntimeError, match="flowmap_amd: depths must be \\(frame, height, width\\)"):
            fn(y["depth"][None], y["k"], y["ext"], y["colors"])
        with pytest.raises(RuntimeError, match="flowmap_amd: intrinsics / extrinsics do not match the depths"):
            fn(y["depth"], y["k"][:-1], y["ext"], y["colors"])
        with pytest.raises(RuntimeError, match="flowmap_amd: intrinsics / extrinsics do not match the depths"):
            fn(y["depth"], y["k"], y["ext"][:, :3], y["colors"])
        with pytest.raises(RuntimeError, match="flowmap_amd: colors must be \\(frame, 3, height, width\\)"):
            fn(y["depth"], y["k"], y["ext"], y["colors"][:, :2])
        with pytest.raises(RuntimeError, match="flowmap_amd: keep must be a bool tensor"):
            fn(*args, keep=torch.ones(y["depth"].shape, device=dev))
        with pytest.raises(RuntimeError, match="flowmap_amd: keep of shape .* does not match the depths"):
            fn(*args, keep=torch.ones(y["depth"].shape[1:], dtype=torch.bool, device=dev))
        with pytest.raises(RuntimeError, match="flowmap_amd: .*must be float32"):
            fn(y["depth"].double(), y["k"], y["ext"], y["colors"])
    if torch.device(dev).type != "cpu":
        with pytest.raises(RuntimeError, match="flowmap_amd: .*different devices|flowmap_amd: .*on cpu"):
            flowmap_amd.tsdf_volume(y["depth"], y["k"].cpu(), y["ext"], y["colors"], vs, **grid)
        with pytest.raises(RuntimeError, match="flowmap_amd: keep is on cpu"):
            flowmap_amd.tsdf_volume(*args, vs, keep=torch.ones(y["depth"].shape, dtype=torch.bool), **grid)
    big = y["depth"][:1, :1, :1].expand(2, 32768, 32768)  # (an expanded view: no memory behind it)
    with pytest.raises(ValueError, match="flowmap_amd: tsdf_volume: frames x height x width = 2 x 32768 x 32768 does not fit"):
        flowmap_amd.tsdf_volume(big, y["k"], y["ext"], None, vs, **grid)
    before = _ops.counters["tsdf_volume"]
    depth = y["depth"].clone().requires_grad_(True)
    r = flowmap_amd.tsdf_volume(depth, y["k"], y["ext"], y["colors"].clone().requires_grad_(True), vs, origin=list(call["origin"]), dims=list(call["dims"]))
    assert isinstance(r, TsdfVolume) and not (r.tsdf.requires_grad or r.color.requires_grad or r.world_to_camera.requires_grad)
    assert r.truncation == float(np.float32(4.0 * vs)) and r.near == 0.0 and r.frames == (0, 2) and r.origin == tuple(call["origin"])
    assert _ops.counters["tsdf_volume"] == before + 1
    assert flowmap_amd.tsdf_volume is export.tsdf_volume and "tsdf_volume" in flowmap_amd.__all__ and "TsdfVolume" in flowmap_amd.__all__
    for tensor in args:
        assert not [key for key in tensor.__dict__ if key.startswith("_fm_")], "a note was left on an argument"
    for bad in (0, -1, 1.0, None, True, "1"):
        with pytest.raises(ValueError, match="flowmap_amd: surface_points: min_weight"):
            r.surface_points(min_weight=bad)
    assert not any(v.requires_grad for v in r.surface_points() if v is not None)


C_PARAMS = ("depth k ext colors keep frames height width first_frame count ox oy oz nx ny nz voxel_size truncation near world_to_camera tsdf weight color "
            "color_weight stream").split()
C_VALID = dict(frames=5, height=8, width=16, first_frame=1, count=3, ox=0.0, oy=0.0, oz=0.0, nx=8, ny=4, nz=2, voxel_size=0.1, truncation=0.4, near=0.0)
INF, NAN = float("inf"), float("nan")
C_REFUSED = ["nulls", dict(frames=0), dict(frames=65536), dict(height=0), dict(width=-1), dict(height=32768, width=32768), dict(frames=3, height=32768, width=32767),
             dict(first_frame=-1), dict(count=0), dict(first_frame=3, count=3), dict(first_frame=5, count=1), dict(nx=0), dict(ny=-1), dict(nz=0),
             dict(nx=2048, ny=2048, nz=512), dict(nx=65536, ny=65536, nz=1), dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=NAN), dict(voxel_size=INF),
             dict(truncation=0.0), dict(truncation=-1.0), dict(truncation=NAN), dict(truncation=INF), dict(near=-1.0), dict(near=NAN), dict(near=INF),
             dict(ox=NAN), dict(oy=INF), dict(oz=-INF), dict(depth=None), dict(k=None), dict(ext=None), dict(colors=None), dict(color=None),
             dict(color_weight=None), dict(world_to_camera=None), dict(tsdf=None), dict(weight=None)]
COUNT_PARAMS = "tsdf weight nx ny nz min_weight block_counts stream".split()
COUNT_VALID = dict(nx=8, ny=4, nz=2, min_weight=1)
COUNT_REFUSED = ["nulls", dict(nx=0), dict(ny=0), dict(nz=-1), dict(nx=2048, ny=2048, nz=512), dict(min_weight=0), dict(min_weight=-1), dict(tsdf=None),
                 dict(weight=None), dict(block_counts=None)]
EMIT_PARAMS = "tsdf weight color color_weight nx ny nz ox oy oz voxel_size min_weight block_offsets rows xyz normals rgb edge stream".split()
EMIT_VALID = dict(nx=8, ny=4, nz=2, ox=0.0, oy=0.0, oz=0.0, voxel_size=0.1, min_weight=1, rows=4)
EMIT_REFUSED = ["nulls", dict(nx=0), dict(nz=0), dict(nx=2048, ny=2048, nz=512), dict(voxel_size=0.0), dict(voxel_size=NAN), dict(ox=NAN), dict(oz=INF),
                dict(min_weight=0), dict(rows=0), dict(rows=-1), dict(tsdf=None), dict(weight=None), dict(color=None), dict(color_weight=None), dict(rgb=None),
                dict(block_offsets=None), dict(xyz=None), dict(normals=None), dict(edge=None)]


def case_c_entries_refuse(lib, what):
    """The C entries through ctypes, on REJECTED calls only (nothing reaches a launch); the size function also where it answers."""
    import ctypes

    from flowmap_amd import _lib

    c_entry_refuses(lib, what, "fm_tsdf_volume", C_PARAMS, C_VALID, C_REFUSED)
    c_entry_refuses(lib, what, "fm_tsdf_surface_count", COUNT_PARAMS, COUNT_VALID, COUNT_REFUSED)
    c_entry_refuses(lib, what, "fm_tsdf_surface_emit", EMIT_PARAMS, EMIT_VALID, EMIT_REFUSED)
    size = lib.fm_tsdf_surface_blocks
    size.argtypes, size.restype = _lib.SIGNATURES["fm_tsdf_surface_blocks"], ctypes.c_int
    out = ctypes.c_long(-1)
    cast = lambda: ctypes.cast(ctypes.byref(out), ctypes.c_void_p)  # noqa: E731
    for dims in ((1, 1, 1), (16, 4, 4), (257, 1, 1), (9, 7, 5), (128, 64, 32), (2047, 1024, 1024)):
        assert size(*dims, cast()) == 0 and out.value == (dims[0] * dims[1] * dims[2] + T - 1) // T, f"{what}: blocks{dims} = {out.value}"
    for dims in ((0, 1, 1), (1, 0, 1), (1, 1, -1), (2048, 1024, 1024), (65536, 65536, 1)):
        assert size(*dims, cast()) == 1, f"{what}: blocks{dims} not refused"
    assert size(4, 4, 4, None) == 1


def case_host_tensor_refused():
    """Host tensors are refused by name: there is no reference function to hand over to."""
    host_tensor_refused(lambda: run("tiny", "cpu"), "flowmap_amd: tensors are on cpu.*no CPU fallback")


# ---- check 6: training is left alone; Model.tsdf, grid_around, write_ply -------------------------------------------------------------------------


def case_training_untouched(dev, tracking, fuse):
    """operator_checks.train, 3 steps from step 1 after the warm-up, with and without Model.tsdf between forward and backward (coloured
    from the batch, then its surface points) and between the steps: operator_checks.assert_training_untouched with ``tsdf_volume`` the one
    counter that differs — a LazyExtrinsics handed in is still unevaluated afterwards, and a flow-only step does hand one in."""
    steps = 3
    grid = dict(origin=(-1.0, -1.0, 0.5), dims=(24, 20, 16))

    def mid(ns):
        v = ns.model.tsdf(ns.out, ns.batch, voxel_size=0.1, **grid)
        return v, v.surface_points()

    after = lambda ns: ns.model.tsdf(ns.out, voxel_size=0.1, frames=(1, 3), near=0.1, **grid)  # noqa: E731
    plain = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True, prepare=batch_colours)
    with_calls = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True, prepare=batch_colours, calls=(mid, after))
    assert_training_untouched(plain, with_calls, "tsdf_volume", 2 * steps)
    if not tracking:
        assert all(was for was, _ in with_calls.lazy_kept), "a flow-only training step hands out a LazyExtrinsics: the case must exercise it"
    (first, surface), second = with_calls.seen[0], with_calls.seen[1]
    assert first.color is not None and first.dims == (24, 20, 16) and tuple(first.world_to_camera.shape) == (FRAMES, 4, 4) and int(first.weight.sum()) > 0
    assert surface[3].dtype == torch.int64 and surface[2] is not None
    assert second.color is None and second.frames == (1, 3) and int(second.weight.max()) <= 3
    assert HEIGHT * WIDTH > 0


def case_model_tsdf_grid_and_ply(dev, tmp_path):
    """Model.tsdf is export.tsdf_volume of the output's tensors; grid_around encloses a cloud; write_ply without normals is byte for byte
    what it was, with normals it round-trips."""
    import pytest

    import flowmap_amd
    from flowmap_amd import Batch, ModelOutput, export
    from flowmap_amd.model.model import Model
    from flowmap_amd.model.projection import LazySurfaces

    x, call = case_of("wrap")
    y = {key: (None if v is None else v.clone().to(dev)) for key, v in x.items()}
    depth, k, ext = y["depth"][None], y["k"][None], y["ext"][None]
    out = ModelOutput(depth, LazySurfaces(depth, k), k, ext, None)
    kw = {key: v for key, v in call.items() if key != "voxel_size"}
    direct = run("wrap", dev)
    same_volume(Model.tsdf(None, out, Batch(y["colors"][None]), voxel_size=call["voxel_size"], **kw), direct, "Model.tsdf: ")
    bare = Model.tsdf(None, out, voxel_size=call["voxel_size"], **kw)
    assert bare.color is None and bare.color_weight is None and torch.equal(bare.tsdf, direct.tsdf) and torch.equal(bare.weight, direct.weight)
    with pytest.raises(ValueError, match="flowmap_amd: Model.tsdf: voxel_size is required"):
        Model.tsdf(None, out, **kw)
    flowmap_amd.set_lazy_surfaces(False)
    # grid_around: of a tensor and of a VoxelCloud
    points = world_points(x).float().to(dev)
    origin, dims = export.grid_around(points, 0.05, margin=0.1)
    low, high = points.min(dim=0).values.cpu().double(), points.max(dim=0).values.cpu().double()
    top = torch.tensor(origin, dtype=torch.float64) + torch.tensor(dims, dtype=torch.float64) * float(np.float32(0.05))
    assert all(isinstance(o, float) for o in origin) and all(isinstance(n, int) and n >= 1 for n in dims)
    assert bool((torch.tensor(origin, dtype=torch.float64) <= low - 0.1 + 1e-6).all()) and bool((top >= high + 0.1).all()), "the grid must enclose the points and the margin"
    assert bool((top <= high + 0.1 + 2.5 * 0.05).all()), "and no more than two voxels beyond it"
    cloud = flowmap_amd.voxel_point_cloud(y["depth"], y["k"], y["ext"], y["colors"], 0.05)
    assert export.grid_around(cloud, 0.05, margin=0.1) == export.grid_around(cloud.xyz, 0.05, margin=0.1)
    volume = flowmap_amd.tsdf_volume(y["depth"], y["k"], y["ext"], y["colors"], 0.05, **dict(zip(("origin", "dims"), export.grid_around(cloud, 0.05, margin=0.2))))
    assert volume.surface_points()[3].shape[0] > 0
    withnan = torch.cat((points, torch.full((1, 3), float("nan"), device=dev)))
    assert export.grid_around(withnan, 0.05, margin=0.1) == (origin, dims)
    for bad in (0.0, -1.0, float("nan"), None, True):
        with pytest.raises(ValueError, match="flowmap_amd: grid_around: voxel_size"):
            export.grid_around(points, bad)
    for bad in (-0.1, float("inf"), "1"):
        with pytest.raises(ValueError, match="flowmap_amd: grid_around: margin"):
            export.grid_around(points, 0.05, margin=bad)
    for bad in (points[:, :2], points[0], "cloud", points.long(), points[:0]):
        with pytest.raises(ValueError, match="flowmap_amd: grid_around: points"):
            export.grid_around(bad, 0.05)
    with pytest.raises(ValueError, match="flowmap_amd: grid_around: .* do not fit"):
        export.grid_around(points, 1e-6)
    # write_ply
    xyz, normals, rgb, _ = direct.surface_points()
    n_xyz, n_rgb, n_normals = xyz.cpu().numpy(), rgb.cpu().numpy(), normals.cpu().numpy()
    plain, again, full = tmp_path / "plain.ply", tmp_path / "again.ply", tmp_path / "normals.ply"
    export.write_ply(plain, n_xyz, n_rgb)
    vertices = np.zeros(len(n_xyz), dtype=[("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])  # today's bytes, stated independently
    vertices["xyz"], vertices["rgb"] = n_xyz, (n_rgb * 255).astype(np.float32)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
              "property float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(n_xyz)).encode("ascii")
    assert plain.read_bytes() == header + vertices.tobytes(), "write_ply without normals must be byte for byte what it was"
    export.write_ply(again, n_xyz, n_rgb, None)
    assert again.read_bytes() == plain.read_bytes()
    direct.write_ply(full)
    raw = full.read_bytes()
    assert raw.startswith(header) and len(raw) == len(header) + 27 * len(n_xyz)
    back = np.frombuffer(raw[len(header):], dtype=vertices.dtype)
    assert np.array_equal(back["xyz"].view(np.uint32), n_xyz.view(np.uint32)) and np.array_equal(back["n"].view(np.uint32), n_normals.view(np.uint32))
    assert np.array_equal(back["rgb"], vertices["rgb"])
    got_xyz, got_rgb = export.read_ply(full)
    assert np.array_equal(got_xyz, n_xyz) and np.array_equal(got_rgb, vertices["rgb"] / 255.0)
    with pytest.raises(ValueError, match="flowmap_amd: write_ply: normals of shape"):
        export.write_ply(again, n_xyz, n_rgb, n_normals[:-1])
    bare.write_ply(again, min_weight=2)
    assert np.array_equal(export.read_ply(again)[1], np.zeros((bare.surface_points(2)[3].shape[0], 3)))
    assert math.isfinite(float(xyz.sum()))


# ---- check 7: memory (GPU) ---------------------------------------------------------------------------------------------------------------------


def case_memory(dev, name="wide"):
    """Peak allocated bytes during a call stay below the outputs plus the call's small tensors: the volume is written once, no
    volume-sized temporary is formed."""
    import flowmap_amd

    x, call = case_of(name)
    y = {key: (None if v is None else v.clone().to(dev)) for key, v in x.items()}
    kw = {key: v for key, v in call.items() if key != "voxel_size"}
    flowmap_amd.tsdf_volume(y["depth"], y["k"], y["ext"], y["colors"], call["voxel_size"], **kw)  # (warm: libraries loaded, allocator primed)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    v = flowmap_amd.tsdf_volume(y["depth"], y["k"], y["ext"], y["colors"], call["voxel_size"], **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = sum(getattr(v, key).numel() * getattr(v, key).element_size() for key in FIELDS)
    slack = 8 * 512  # (the caching allocator's granularity on each output)
    print(f"  {name}: peak {peak} B; outputs {outputs} B")
    assert peak <= outputs + slack, f"peak {peak} B > outputs {outputs} B"
