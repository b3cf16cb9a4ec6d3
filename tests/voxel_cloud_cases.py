"""export.voxel_point_cloud (fm_voxel_cloud): the cases, a numpy restatement of the operator, and the checks the CPU (host double) and
GPU test modules share.

THE RESTATEMENT (``restate``) takes the fp32 world points that ``world_point_cloud`` returns ON THE SAME DEVICE and repeats the rest in
numpy: the fp32 cell (one multiply by ``float32(1/voxel_size)``, floor, the exact difference), the 63-bit key, the integer sums of
min(uint32(frac·2²⁰), 2²⁰−1) and uint32(clamp(c)·2¹⁶), the minimum index, the fp64 finalize rounded once, the order by ``first``.  Every
field of the operator must equal it bit for bit (check 1).

BOUND 2 — a centroid against the fp64 mean of the voxel's fp32 points x, per coordinate.  With t = fl(x·inv), inv = fl(1/s):
  * inv·s = 1 + δ, |δ| <= 2⁻²⁴, so t·s misses x by |x|·2⁻²⁴ < ulp₃₂(x);                          (the rounded reciprocal)
  * |t − x·inv| <= ulp₃₂(t)/2, and ulp₃₂(t)·s <= 2·ulp₃₂(x) (the binades of t·s and x may be one apart): <= ulp₃₂(x); (the multiply)
  * cell + frac = t exactly; q/2²⁰ truncates frac by less than 2⁻²⁰ and the + 0.5 centres that: <= s·2⁻²¹ (s·2⁻²⁰ where the min bites);
  * sums, mean and finalize are integers and fp64: exact to 2⁻⁵³; the result is rounded once to fp32: ulp₃₂(x)/2.
  Together s·2⁻²⁰ + 2.5·ulp₃₂(max|x|); the gate is the issue's s·2⁻²⁰ + 4·ulp₃₂(max|x|), which contains it (max over the voxel's points and
  its centroid).  Colour: each quantised channel is short of c by less than 2⁻¹⁶, so is their mean; the one fp32 rounding of a value <= 1
  adds 2⁻²⁵: 2⁻¹⁶ + 2⁻²⁵ (the issue's 2⁻¹⁶ leaves that rounding out: a single-point voxel whose c·2¹⁶ has a fraction above 0.998 needs it).

GPU AGAINST HOST DOUBLE (check 3).  The device build evaluates the world point with the fused multiply-adds fm_world_points has always
been compiled to, the host build product by product (fm_math.h: world_point_at) — as the two builds of fm_world_points always have.  A
point within an ulp of a cell face can therefore sit in another voxel on the other build.  The cases are built so that it cannot: a
LATTICE scene has power-of-two focal lengths, a principal point of 1/2, signed-permutation rotations and power-of-two depths, so every
PRODUCT of the world point is exact and fusing changes nothing (translations, pixel centres and colours are arbitrary fp32); the check
asserts first that the two builds' world points are bit-equal, then that every field is.  The cases on a free scene ("scene", "support")
are checked against the restatement on each build (check 1), not across builds.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

from conftest import load_golden, t
from operator_checks import assert_training_untouched, batch_colours, c_entry_refuses, host_tensor_refused, same_tensors, train
from oracle import flowmap_oracle as orc

T = 1024  # pixels per workgroup (fm_residual_args.h: kVoxelTile)
LIMIT = 1 << 20
# name -> dict(scene=(kind, (f, h, w), seed), voxel_size, and what the call adds)
SPECS = {
    "tiny": dict(scene=("lattice", (2, 3, 5), 61), voxel_size=0.25),  # fewer pixels than a wavefront
    "odd": dict(scene=("lattice", (3, 17, 23), 62), voxel_size=0.125),  # scalar path, a partial last quad
    "tile": dict(scene=("lattice", (2, 32, 32), 63), voxel_size=0.125),  # exactly one tile
    "tile1": dict(scene=("lattice", (2, 25, 41), 64), voxel_size=0.125),  # one pixel past it
    "wide": dict(scene=("lattice", (5, 40, 52), 65), voxel_size=0.1),  # several tiles, the 16-byte path
    "slice": dict(scene=("lattice", (2, 8, 16), 66), voxel_size=0.125, misaligned=True),  # width % 4 == 0 but a base 4 bytes off 16
    "one": dict(scene=("lattice_far", (3, 20, 24), 67), voxel_size=64.0),  # every point in ONE voxel: every lane on one record
    "own": dict(scene=("lattice", (2, 9, 12), 68), voxel_size=2.0**-14),  # every point its own voxel: M = N
    "fit": dict(scene=("lattice", (3, 17, 23), 62), voxel_size=0.125, capacity="exact"),  # M == capacity
    "collide": dict(scene=("collide", 24, 69), voxel_size=1.0, capacity=8),  # one home slot, a chain that wraps past the table's end
    "straddle": dict(scene=("points", "straddle", 70), voxel_size=1.0),  # coordinates either side of 0: floor, not truncation
    "multiples": dict(scene=("points", "multiples", 71), voxel_size=0.5),  # exact multiples of a power-of-two voxel: frac == 0
    "limits": dict(scene=("points", "limits", 72), voxel_size=1.0),  # cells −2²⁰ and 2²⁰−1 kept, one beyond on each side out of range
    "invalid": dict(scene=("lattice_invalid", (2, 12, 20), 73), voxel_size=0.125),  # depth 0, negative, NaN, ±inf
    "none": dict(scene=("lattice", (2, 12, 20), 74), voxel_size=0.125, keep="none"),  # keep all false: M = 0
    "half": dict(scene=("lattice", (3, 17, 23), 75), voxel_size=0.125, keep="random"),
    "min2": dict(scene=("lattice", (5, 40, 52), 65), voxel_size=0.1, min_count=2),
    "min3": dict(scene=("lattice", (5, 40, 52), 65), voxel_size=0.1, min_count=3),
    "bare": dict(scene=("lattice", (3, 17, 23), 62), voxel_size=0.125, colors=False),  # colors=None
    "scene": dict(scene=("scene", (4, 24, 32), 76), voxel_size=0.05),  # a free scene: skewless K, smooth poses, noisy depth
    "support": dict(scene=("scene", (5, 24, 32), 77), voxel_size=0.05, keep="support"),  # keep from a real depth_consistency call
}
EXACT_PRODUCT_CASES = tuple(sorted(name for name, spec in SPECS.items() if spec["scene"][0] not in ("scene",)))
GOLDEN_CASES = ("g_small", "g_odd", "g_wide")
GOLDEN_SPECS = {
    "g_small": dict(scene=("scene", (2, 12, 16), 81), voxel_size=0.1),
    "g_odd": dict(scene=("scene", (3, 15, 21), 82), voxel_size=0.1),
    "g_wide": dict(scene=("scene", (3, 16, 40), 83), voxel_size=0.15),
}
GOLDEN_CAP = 5e-3  # the share of points whose voxel may have other members than in the fp64 reference


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------


def restated_hash(key):
    """fm_math.h: voxel_hash on a uint64 array."""
    key = np.asarray(key, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        key ^= key >> np.uint64(33)
        key *= np.uint64(0xFF51AFD7ED558CCD)
        key ^= key >> np.uint64(33)
        key *= np.uint64(0xC4CEB9FE1A85EC53)
        key ^= key >> np.uint64(33)
    return key


def restated_key(cells):
    biased = (np.asarray(cells, dtype=np.int64) + LIMIT).astype(np.uint64)
    return (biased[..., 0] << np.uint64(42)) | (biased[..., 1] << np.uint64(21)) | biased[..., 2]


def slots_of(capacity):
    slots = 2
    while slots < 2 * capacity:
        slots *= 2
    return slots


def restate(xyz, rgb, depth, keep, voxel_size, min_count=1):
    """xyz (N,3) float32 — the world points —, rgb (N,3) float32 or None, depth (N,) float32, keep (N,) bool or None -> dict(xyz, rgb,
    count, first, dropped, voxel_of (N,), filtered (points in voxels below min_count), cells (N,3) int64 with LIMIT where dropped)."""
    xyz, depth = np.asarray(xyz, dtype=np.float32), np.asarray(depth, dtype=np.float32).reshape(-1)
    n = xyz.shape[0]
    masked = np.zeros(n, bool) if keep is None else ~np.asarray(keep, dtype=bool).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        invalid = ~masked & (~((depth > 0) & np.isfinite(depth)) | ~np.isfinite(xyz).all(axis=1))
        inv = np.float32(1.0 / float(voxel_size))
        scaled = xyz * inv  # (one fp32 multiply)
        cell = np.floor(scaled)
        inside = ((cell >= -float(LIMIT)) & (cell < float(LIMIT))).all(axis=1)
        out_of_range = ~masked & ~invalid & ~inside
        live = ~masked & ~invalid & inside
        frac = (scaled - cell)[live]  # (exact)
    q = np.minimum((frac * np.float32(LIMIT)).astype(np.uint32), np.uint32(LIMIT - 1)).astype(np.int64)
    cells = np.full((n, 3), LIMIT, dtype=np.int64)
    cells[live] = cell[live].astype(np.int64)
    index = np.nonzero(live)[0]
    keys, member = np.unique(restated_key(cells[live]), return_inverse=True)
    m = len(keys)
    count = np.bincount(member, minlength=m).astype(np.int64)
    first = np.full(m, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, member, index)
    sums = np.zeros((m, 3), dtype=np.int64)
    np.add.at(sums, member, q)
    voxel_cell = np.zeros((m, 3), dtype=np.int64)
    voxel_cell[member] = cells[live]
    safe = np.maximum(count, 1).astype(np.float64)[:, None]
    centroid = ((voxel_cell.astype(np.float64) + (sums.astype(np.float64) / safe + 0.5) / float(LIMIT)) * float(voxel_size)).astype(np.float32)
    mean_rgb = None
    if rgb is not None:
        c = np.asarray(rgb, dtype=np.float32)[live]
        clamped = np.where(c > 0, np.where(c < 1, c, np.float32(1)), np.float32(0)).astype(np.float32)
        colour_sums = np.zeros((m, 3), dtype=np.int64)
        np.add.at(colour_sums, member, (clamped * np.float32(65536)).astype(np.uint32).astype(np.int64))
        mean_rgb = (colour_sums.astype(np.float64) / safe / 65536.0).astype(np.float32)
    kept = count >= min_count
    order = np.argsort(first[kept], kind="stable")
    rows = np.nonzero(kept)[0][order]
    row_of = np.full(m, -1, dtype=np.int32)
    row_of[rows] = np.arange(len(rows), dtype=np.int32)
    voxel_of = np.full(n, -1, dtype=np.int32)
    voxel_of[index] = row_of[member]
    return dict(xyz=centroid[rows], rgb=None if mean_rgb is None else mean_rgb[rows], count=count[rows].astype(np.int32), first=first[rows],
                dropped=dict(masked=int(masked.sum()), invalid=int(invalid.sum()), out_of_range=int(out_of_range.sum())), voxel_of=voxel_of,
                filtered=int(count[~kept].sum()), cells=cells)


def voxelise64(xyz, voxel_size):
    """The same grid on fp64 points (the fp64 evaluation of the reference): cell = floor(x / voxel_size) and the plain mean, all in fp64
    -> dict(voxel_of (N,), xyz (M,3) float64, count, first), rows in ascending ``first``."""
    xyz = np.asarray(xyz, dtype=np.float64)
    cells = np.floor(xyz / float(voxel_size)).astype(np.int64)
    assert np.abs(cells).max() < LIMIT
    keys, member = np.unique(restated_key(cells), return_inverse=True)
    m = len(keys)
    count = np.bincount(member, minlength=m)
    first = np.full(m, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, member, np.arange(len(xyz)))
    sums = np.zeros((m, 3))
    np.add.at(sums, member, xyz)
    order = np.argsort(first, kind="stable")
    row_of = np.empty(m, dtype=np.int32)
    row_of[order] = np.arange(m, dtype=np.int32)
    return dict(voxel_of=row_of[member], xyz=(sums / count[:, None])[order], count=count[order].astype(np.int32), first=first[order])


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------

_ROTATIONS = [np.array(m, dtype=np.float32) for m in (
    [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
    [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]])]  # proper rotations with entries 0, ±1
_UNIT_K = [[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]]


def _point_lists(which):
    if which == "straddle":
        values = (-1.25, -0.75, -0.25, -2.0**-30, 0.0, 2.0**-30, 0.25, 0.75, 1.25)
        return [(a, b, 0.5) for a in values for b in (-0.5, 0.5)] + [(0.5, 0.5, a) for a in values]
    if which == "multiples":  # voxel 0.5: every coordinate a multiple of it
        return [(0.5 * i, -0.5 * j, 0.5 * (i + j)) for i in range(-3, 4) for j in range(-2, 3)] + [(1.0, -1.0, 1.5)] * 3
    edge = float(LIMIT)
    inside, outside = (-edge + 0.5, edge - 0.5, -edge, edge - 2.0**-4), (-edge - 0.5, edge + 0.5, edge, -edge - 2.0**-3)
    points = []
    for axis in range(3):
        for value in inside + outside:
            p = [3.5, -7.5, 11.5]
            p[axis] = value
            points.append(tuple(p))
    return points + [(-edge + 0.5, edge - 0.5, -edge + 0.5), (edge + 0.5, 0.5, 0.5), (3.5, -7.5, 11.5)]


def _points_scene(points, seed):
    """One 1 x 1 frame per point: K with ray (0, 0, 1) at the pixel centre, depth 1, an identity rotation, translation p − (0, 0, 1)."""
    p = torch.tensor(points, dtype=torch.float64)
    f = p.shape[0]
    ext = torch.eye(4).repeat(f, 1, 1)
    ext[:, :3, 3] = (p - torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).float()
    return {"depth": torch.ones((f, 1, 1)), "k": torch.tensor(_UNIT_K).repeat(f, 1, 1), "ext": ext,
            "colors": torch.rand((f, 3, 1, 1), generator=torch.Generator().manual_seed(seed))}


def colliding_cells(count, slots, home):
    """``count`` distinct cells (i, j, 0) whose restated hash has the home slot ``home`` in a table of ``slots``."""
    grid = np.stack(np.meshgrid(np.arange(-40, 40), np.arange(-40, 40), indexing="ij"), axis=-1).reshape(-1, 2)
    cells = np.concatenate([grid, np.zeros((len(grid), 1), dtype=grid.dtype)], axis=1)
    hit = cells[(restated_hash(restated_key(cells)) & np.uint64(slots - 1)) == np.uint64(home)]
    assert len(hit) >= count, "widen the search"
    return hit[:count]


@functools.lru_cache(maxsize=None)
def scene_inputs(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "points":
        return _points_scene(_point_lists(shape), seed)
    if kind == "collide":  # `shape` frames: 6 voxels on the LAST home slot of the 16-slot table (the chain wraps to slots 0..4), 2 elsewhere
        slots = slots_of(8)
        chain, other = colliding_cells(6, slots, slots - 1), colliding_cells(2, slots, 5)
        cells = np.concatenate([chain, other])
        picks = torch.randint(0, len(cells), (shape,), generator=g).numpy()
        picks[: len(cells)] = np.arange(len(cells))
        offsets = torch.rand((shape, 3), generator=g).double().numpy()
        return _points_scene((cells[picks] + 0.05 + 0.9 * offsets).tolist(), seed)
    f, h, w = shape
    colors = torch.rand((f, 3, h, w), generator=g)
    if kind == "scene":
        sc = orc.synth_scene(f, h, w, seed=seed)
        return {"depth": sc["depth_init"].contiguous(), "k": sc["intrinsics_gt"].expand(f, 3, 3).contiguous(), "ext": sc["extrinsics_gt"].contiguous(),
                "colors": colors}
    # lattice: every product of the world point is exact (see the module docstring)
    k = torch.tensor(_UNIT_K).repeat(f, 1, 1)
    k[:, 0, 0] = torch.tensor([1.0, 0.5, 2.0])[torch.randint(0, 3, (f,), generator=g)]
    k[:, 1, 1] = torch.tensor([1.0, 0.5, 2.0])[torch.randint(0, 3, (f,), generator=g)]
    ext = torch.eye(4).repeat(f, 1, 1)
    for i in range(f):
        ext[i, :3, :3] = torch.from_numpy(_ROTATIONS[int(torch.randint(0, len(_ROTATIONS), (1,), generator=g))])
    ext[:, :3, 3] = torch.randn((f, 3), generator=g) * 0.3
    depth = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (f, h, w), generator=g)]
    if kind == "lattice_far":  # every coordinate in (8, 12) + 2·(−1, 1) ⊂ (0, 64)
        ext[:, :3, 3] = 10.0 + 2.0 * torch.rand((f, 3), generator=g)
        k[:, 0, 0] = k[:, 1, 1] = 1.0
    if kind == "lattice_invalid":
        flat = depth.view(-1)
        bad = torch.randperm(flat.numel(), generator=g)[:40]
        flat[bad] = torch.tensor([0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf"), -2.0, 0.0]).repeat(5)
    return {"depth": depth, "k": k, "ext": ext, "colors": colors}


def spec_of(name):
    return SPECS[name] if name in SPECS else GOLDEN_SPECS[name]


def case_inputs(name):
    """depth (F,h,w), k (F,3,3), ext (F,4,4), colors (F,3,h,w) of a case on the CPU (tools/make_golden_voxel_cloud.py draws them from here)."""
    return scene_inputs(*spec_of(name)["scene"])


def on_device(name, dev):
    """The case's tensors on ``dev`` and the keyword arguments of its call (``capacity="exact"`` still to be resolved)."""
    spec = spec_of(name)
    x = {key: value.clone().to(dev) for key, value in case_inputs(name).items()}
    if spec.get("misaligned"):  # the same values in a buffer whose base is 4 bytes past a 16-byte boundary
        raw = torch.empty(x["depth"].numel() + 1, dtype=torch.float32, device=dev)
        raw[1:] = x["depth"].reshape(-1)
        x["depth"] = raw[1:].view(x["depth"].shape)
        assert x["depth"].is_contiguous() and x["depth"].data_ptr() % 16 == 4
    if not spec.get("colors", True):
        x["colors"] = None
    kw = {key: spec[key] for key in ("min_count", "capacity") if key in spec}
    keep = spec.get("keep")
    if keep == "none":
        kw["keep"] = torch.zeros(x["depth"].shape, dtype=torch.bool, device=dev)
    elif keep == "random":
        kw["keep"] = (torch.rand(x["depth"].shape, generator=torch.Generator().manual_seed(7)) < 0.5).to(dev)
    elif keep == "support":
        import flowmap_amd

        seen = flowmap_amd.depth_consistency(x["depth"][None], x["k"][None], x["ext"][None], tolerance=0.05)
        kw["keep"] = seen.support[0] >= 1
        assert 0 < int(kw["keep"].sum()) < kw["keep"].numel(), "the support mask must keep some points and drop some"
    return x, spec["voxel_size"], kw


def world_points(x):
    from flowmap_amd import export

    xyz, rgb = export.world_point_cloud(x["depth"], x["k"], x["ext"], x["colors"])
    return xyz.cpu().numpy(), None if rgb is None else rgb.cpu().numpy()


def run(name, dev, details=True, **changed):
    """-> (VoxelCloud, the restatement fed the same device's world points, the inputs, the world points)."""
    import flowmap_amd

    x, voxel_size, kw = on_device(name, dev)
    xyz, rgb = world_points(x)
    keep = kw.get("keep")
    want = restate(xyz, rgb, x["depth"].cpu().numpy(), None if keep is None else keep.cpu().numpy(), voxel_size, kw.get("min_count", 1))
    if kw.get("capacity") == "exact":
        kw["capacity"] = len(want["count"])
    kw.update(changed)
    got = flowmap_amd.voxel_point_cloud(x["depth"], x["k"], x["ext"], x["colors"], voxel_size, details=details, **kw)
    return got, want, x, xyz


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_cloud(a, b, what):
    """Two VoxelClouds equal bit for bit in every field."""
    same_tensors(a, b, ("xyz", "rgb", "count", "first", "voxel_of"), f"{what}: ", scalars=("dropped",), equal=lambda u, v: np.array_equal(bits(u), bits(v)))


# ---- checks 1 and 2 -----------------------------------------------------------------------------------------------------------------------


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def case_exact_properties(dev, name):
    """Check 1: every field equals the restatement bit for bit and every point is accounted for.  Check 2: the centroids and mean colours
    against the fp64 mean of the voxels' fp32 points, at the derived bound."""
    got, want, x, xyz = run(name, dev)
    f, h, w = x["depth"].shape
    n = f * h * w
    m = len(want["count"])
    assert got.dropped == want["dropped"], f"{name}: dropped {got.dropped} vs {want['dropped']}"
    assert len(got) == m and tuple(got.xyz.shape) == (m, 3) and got.xyz.dtype == torch.float32, f"{name}: {len(got)} voxels, the restatement has {m}"
    assert got.count.dtype == torch.int32 and got.first.dtype == torch.int64 and got.voxel_of.dtype == torch.int32 and tuple(got.voxel_of.shape) == (f, h, w)
    assert np.array_equal(got.count.cpu().numpy(), want["count"]), f"{name}: count"
    assert np.array_equal(got.first.cpu().numpy(), want["first"]), f"{name}: first"
    assert np.array_equal(got.voxel_of.cpu().numpy().reshape(-1), want["voxel_of"]), f"{name}: voxel_of"
    assert np.array_equal(bits(got.xyz), bits(want["xyz"])), f"{name}: xyz is not the restated fixed-point finalize"
    assert (got.rgb is None) == (want["rgb"] is None)
    if got.rgb is not None:
        assert np.array_equal(bits(got.rgb), bits(want["rgb"])), f"{name}: rgb is not the restated fixed-point finalize"
    assert int(got.count.sum()) + sum(got.dropped.values()) + want["filtered"] == n, f"{name}: points are not accounted for"
    assert bool((got.first[1:] > got.first[:-1]).all()), f"{name}: rows are not in ascending first"
    voxel_size = spec_of(name)["voxel_size"]
    voxel_of = want["voxel_of"]
    live = voxel_of >= 0
    if m:
        sums, top = np.zeros((m, 3)), np.zeros((m, 3))
        np.add.at(sums, voxel_of[live], xyz[live].astype(np.float64))
        np.maximum.at(top, voxel_of[live], np.abs(xyz[live]).astype(np.float64))
        mean = sums / want["count"][:, None]
        ours = got.xyz.cpu().numpy().astype(np.float64)
        bound = voxel_size * 2.0**-20 + 4.0 * ulp32(np.maximum(top, np.abs(ours)))
        worst = float((np.abs(ours - mean) / bound).max())
        print(f"  {name}: {m} voxels of {n} points; centroid error at most {worst:.3f} of the bound")
        assert worst <= 1.0, f"{name}: a centroid is {worst:.3f} bounds from the fp64 mean of its points"
        if got.rgb is not None:
            colour_sums = np.zeros((m, 3))
            np.add.at(colour_sums, voxel_of[live], np.clip(x["colors"].permute(0, 2, 3, 1).reshape(-1, 3).cpu().numpy()[live].astype(np.float64), 0, 1))
            err = float(np.abs(got.rgb.cpu().numpy().astype(np.float64) - colour_sums / want["count"][:, None]).max())
            assert err <= 2.0**-16 + 2.0**-25, f"{name}: a mean colour is {err:.3e} from the fp64 mean"
    return got, want


def case_shapes(dev):
    """What the named cases are there for, asserted so that a change of a scene cannot quietly retire them."""
    got, want = case_exact_properties(dev, "one")
    assert len(got) == 1 and int(got.count[0]) == 3 * 20 * 24 and int(got.first[0]) == 0
    got, _ = case_exact_properties(dev, "own")
    assert len(got) == 2 * 9 * 12 and bool((got.count == 1).all()) and torch.equal(got.first.cpu(), torch.arange(216))
    got, _ = case_exact_properties(dev, "none")
    assert len(got) == 0 and got.dropped["masked"] == 2 * 12 * 20 and tuple(got.rgb.shape) == (0, 3) and bool((got.voxel_of == -1).all())
    got, want = case_exact_properties(dev, "limits")
    assert got.dropped["out_of_range"] == 13 and len(got) == 3 * 2 + 2, (got.dropped, len(got))  # (two of the four kept values per axis share a cell)
    cells = want["cells"][want["voxel_of"] >= 0]
    assert cells.min() == -LIMIT and cells.max() == LIMIT - 1
    got, want = case_exact_properties(dev, "invalid")
    assert got.dropped["invalid"] == 40
    got, want = case_exact_properties(dev, "straddle")
    cells = want["cells"][:, 0]
    assert {-2, -1, 0, 1} <= set(cells.tolist()), "the straddle case must visit the cells either side of 0"
    got, want = case_exact_properties(dev, "multiples")
    assert np.array_equal(got.xyz[0].cpu().numpy(), ((np.array(_point_lists("multiples")[0]) / 0.5 + 0.5 / LIMIT) * 0.5).astype(np.float32)), "frac must be 0"
    got, want = case_exact_properties(dev, "collide")
    keys = restated_key(want["cells"][want["voxel_of"] >= 0])
    homes = restated_hash(np.unique(keys)) & np.uint64(15)
    assert len(got) == 8 and int((homes == 15).sum()) == 6, "six voxels share the last home slot of the 16-slot table: the chain wraps"
    got, want = case_exact_properties(dev, "fit")
    assert len(got) == len(want["count"]) > 100
    for name in ("min2", "min3"):
        got, want = case_exact_properties(dev, name)
        assert want["filtered"] > 0 and int(got.count.min()) >= spec_of(name)["min_count"]
    got, _ = case_exact_properties(dev, "bare")
    assert got.rgb is None
    got, _ = case_exact_properties(dev, "support")
    assert 0 < got.dropped["masked"] < 5 * 24 * 32


def case_capacity_short(dev):
    """One row too few: the call raises, names capacity and returns nothing; the table full (a chain that finds no slot) likewise."""
    import pytest

    _, want, _, _ = run("odd", dev)
    m = len(want["count"])
    with pytest.raises(RuntimeError, match=f"flowmap_amd: voxel_point_cloud: the cloud does not fit capacity = {m - 1}: {m} voxels"):
        run("odd", dev, capacity=m - 1)
    with pytest.raises(RuntimeError, match="flowmap_amd: voxel_point_cloud: the cloud does not fit capacity = 1: .* points found no slot"):
        run("odd", dev, capacity=1)  # two slots for hundreds of voxels: the walk ends after `slots` probes, nothing waits
    same_cloud(run("odd", dev, capacity=m)[0], run("odd", dev)[0], "capacity == M against the default")


def case_repeatable(dev, name):
    a, b = run(name, dev)[0], run(name, dev)[0]
    same_cloud(a, b, f"{name}: two identical calls")


# ---- check 3: the GPU against the host double ------------------------------------------------------------------------------------------


def case_gpu_against_host_double(dev, name):
    from flowmap_amd import _lib
    from helpers import build_host_sim

    gpu, _, _, xyz_gpu = run(name, dev)
    again = run(name, dev)[0]
    _lib.set_library_for_testing(build_host_sim())
    try:
        host, _, _, xyz_host = run(name, "cpu")
    finally:
        _lib.set_library_for_testing(None)
    same_cloud(gpu, again, f"{name}: two identical GPU calls")
    assert np.array_equal(xyz_gpu.view(np.uint32), xyz_host.view(np.uint32)), f"{name}: the case is built so that the two builds' world points agree to the bit"
    same_cloud(gpu, host, f"{name}: GPU against the host double")


# ---- check 4: reference parity -----------------------------------------------------------------------------------------------------------


def same_membership(a, b):
    """Per point: does its voxel have exactly the same members under the labellings ``a`` and ``b`` (−1: dropped)?"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    pair = (a + 1) * (b.max() + 2) + (b + 1)
    _, inverse, together = np.unique(pair, return_inverse=True, return_counts=True)
    size_a, size_b = np.bincount(a + 1), np.bincount(b + 1)
    same = (together[inverse] == size_a[a + 1]) & (together[inverse] == size_b[b + 1])
    return np.where((a < 0) | (b < 0), (a < 0) & (b < 0), same)


@functools.lru_cache(maxsize=1)
def golden():
    return load_golden("fn_voxel_cloud")


def case_reference_parity(dev, name):
    """Our voxels against the voxelisation of the REFERENCE's world points (export_to_colmap's composition, recorded in fp32 and fp64 by
    tools/make_golden_voxel_cloud.py): the partition agrees with the fp64 reference's on all but GOLDEN_CAP of the points, and the
    centroids of voxels with identical members agree within bound 2 plus the reference's own fp32–fp64 gap on those voxels."""
    import flowmap_amd

    z = golden()
    x = {key: t(z[f"{name}_{key}"]).to(dev) for key in ("depth", "k", "ext", "colors")}
    # (the fixture's own inputs: a scene regenerated from its seed may differ in a last bit with the host's elementary functions)
    voxel_size = spec_of(name)["voxel_size"]
    got = flowmap_amd.voxel_point_cloud(x["depth"], x["k"], x["ext"], x["colors"], voxel_size, details=True)
    ours = got.voxel_of.cpu().numpy().reshape(-1)
    ref64, ref32 = z[f"{name}_f64_voxel_of"], z[f"{name}_voxel_of"]
    agree = same_membership(ours, ref64)
    share, own = 1.0 - agree.mean(), 1.0 - same_membership(ref32, ref64).mean()
    print(f"  {name}: {len(got)} voxels; {share:.2e} of the points sit in a voxel with other members than in the fp64 reference (its own fp32: {own:.2e})")
    assert own <= GOLDEN_CAP, f"{name}: the reference's own fp32 and fp64 voxelisations disagree on {own:.2e} of the points: the case is ill-conditioned"
    assert share <= GOLDEN_CAP, f"{name}: {share:.2e} of the points are grouped differently from the fp64 reference"
    rows = np.unique(ours[agree & (ours >= 0)])
    first_of_row = got.first.cpu().numpy()[rows]
    want64, want32 = z[f"{name}_f64_xyz"][ref64[first_of_row]], z[f"{name}_xyz"]
    both = same_membership(ref32, ref64)[first_of_row]  # (the reference's gap is measured where its two evaluations group alike)
    gap = np.abs(want32[ref32[first_of_row][both]].astype(np.float64) - want64[both]).max() if both.any() else 0.0
    mine = got.xyz.cpu().numpy().astype(np.float64)[rows]
    bound = voxel_size * 2.0**-20 + 4.0 * ulp32(np.abs(mine)) + gap
    worst = float((np.abs(mine - want64) / bound).max())
    print(f"  {name}: {len(rows)} voxels with identical members; centroids within {worst:.3f} of the bound (reference fp32-fp64 gap {gap:.2e})")
    assert worst <= 1.0, f"{name}: a centroid is {worst:.3f} bounds from the fp64 reference's"


# ---- check 5: arguments --------------------------------------------------------------------------------------------------------------------


def case_arguments(dev):
    import pytest

    import flowmap_amd
    from flowmap_amd import VoxelCloud, _ops, export

    x, voxel_size, _ = on_device("odd", dev)
    args = (x["depth"], x["k"], x["ext"], x["colors"])
    for bad in (0.0, -1.0, float("nan"), float("inf"), None, "0.1", True, 1e-46, 1e39):
        with pytest.raises(ValueError, match="flowmap_amd: voxel_point_cloud: voxel_size"):
            flowmap_amd.voxel_point_cloud(*args, bad)
    for bad in (0, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="flowmap_amd: voxel_point_cloud: min_count must be an integer >= 1"):
            flowmap_amd.voxel_point_cloud(*args, voxel_size, min_count=bad)
    for bad in (0, -5, 2.0, "8", True, (1 << 28) + 1):
        with pytest.raises(ValueError, match="flowmap_amd: voxel_point_cloud: capacity must be an integer in"):
            flowmap_amd.voxel_point_cloud(*args, voxel_size, capacity=bad)
    with pytest.raises(ValueError, match="flowmap_amd: voxel_point_cloud: details must be a bool"):
        flowmap_amd.voxel_point_cloud(*args, voxel_size, details=1)
    # what world_point_cloud refuses, refused alike
    for call in (lambda *a, **kw: export.world_point_cloud(*a, **kw), lambda *a, **kw: flowmap_amd.voxel_point_cloud(*a, voxel_size, **kw)):
        with pytest.raises(RuntimeError, match="flowmap_amd: depths must be \\(frame, height, width\\)"):
            call(x["depth"][None], x["k"], x["ext"], x["colors"])
        with pytest.raises(RuntimeError, match="flowmap_amd: intrinsics / extrinsics do not match the depths"):
            call(x["depth"], x["k"][:-1], x["ext"], x["colors"])
        with pytest.raises(RuntimeError, match="flowmap_amd: intrinsics / extrinsics do not match the depths"):
            call(x["depth"], x["k"], x["ext"][:, :3], x["colors"])
        with pytest.raises(RuntimeError, match="flowmap_amd: colors must be \\(frame, 3, height, width\\)"):
            call(x["depth"], x["k"], x["ext"], x["colors"][:, :2])
        with pytest.raises(RuntimeError, match="flowmap_amd: keep must be a bool tensor"):
            call(*args, keep=torch.ones(x["depth"].shape, device=dev))
        with pytest.raises(RuntimeError, match="flowmap_amd: keep of shape .* does not match the depths"):
            call(*args, keep=torch.ones(x["depth"].shape[1:], dtype=torch.bool, device=dev))
        with pytest.raises(RuntimeError, match="flowmap_amd: .*must be float32"):
            call(x["depth"].double(), x["k"], x["ext"], x["colors"])
    if torch.device(dev).type != "cpu":
        with pytest.raises(RuntimeError, match="flowmap_amd: .*different devices|flowmap_amd: .*on cpu"):
            flowmap_amd.voxel_point_cloud(x["depth"], x["k"].cpu(), x["ext"], x["colors"], voxel_size)
        with pytest.raises(RuntimeError, match="flowmap_amd: keep is on cpu"):
            flowmap_amd.voxel_point_cloud(*args, voxel_size, keep=torch.ones(x["depth"].shape, dtype=torch.bool))
    big = x["depth"][:1, :1, :1].expand(2, 32768, 32768)  # (an expanded view: no memory behind it)
    with pytest.raises(ValueError, match="flowmap_amd: voxel_point_cloud: frames x height x width = 2 x 32768 x 32768 does not fit"):
        flowmap_amd.voxel_point_cloud(big, x["k"][:2], x["ext"][:2], None, voxel_size)
    before = _ops.counters["voxel_cloud"]
    depth = x["depth"].clone().requires_grad_(True)
    r = flowmap_amd.voxel_point_cloud(depth, x["k"], x["ext"], x["colors"].clone().requires_grad_(True), voxel_size)
    assert isinstance(r, VoxelCloud) and r.voxel_of is None and r.voxel_size == voxel_size and not (r.xyz.requires_grad or r.rgb.requires_grad)
    assert _ops.counters["voxel_cloud"] == before + 1
    assert flowmap_amd.voxel_point_cloud is export.voxel_point_cloud and "voxel_point_cloud" in flowmap_amd.__all__ and "VoxelCloud" in flowmap_amd.__all__
    for tensor in args:
        assert not [key for key in tensor.__dict__ if key.startswith("_fm_")], "a note was left on an argument"
    assert export.voxel_default_capacity(100) == 100 and export.voxel_default_capacity(65536) == 4096 and export.voxel_default_capacity(1600000) == 100000


C_PARAMS = "depth kinv ext colors keep frames height width voxel_size min_count capacity xyz rgb count first slot pixel_slot counters workspace stream".split()
C_VALID = dict(frames=5, height=8, width=16, voxel_size=0.1, min_count=1, capacity=64)
C_REFUSED = ["nulls", dict(frames=0), dict(frames=65536), dict(height=0), dict(width=-1), dict(height=32768, width=32768), dict(frames=3, height=32768, width=32767),
             dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")), dict(voxel_size=1e-46),
             dict(voxel_size=1e39), dict(min_count=0), dict(min_count=-3), dict(capacity=0), dict(capacity=-1), dict(capacity=(1 << 28) + 1),
             dict(depth=None), dict(kinv=None), dict(ext=None), dict(colors=None), dict(rgb=None), dict(xyz=None), dict(count=None), dict(first=None),
             dict(slot=None), dict(counters=None), dict(workspace=None), dict(workspace="misaligned"), dict(counters="misaligned")]


def case_c_entries_refuse(lib, what):
    """The C entries through ctypes, on REJECTED calls only (nothing reaches a launch); the size function also where it answers."""
    import ctypes

    from flowmap_amd import _lib

    c_entry_refuses(lib, what, "fm_voxel_cloud", C_PARAMS, C_VALID, C_REFUSED,
                    pointer=lambda param, change, address: address + (4 if change.get(param) == "misaligned" else 0))
    size = lib.fm_voxel_cloud_workspace
    size.argtypes, size.restype = _lib.SIGNATURES["fm_voxel_cloud_workspace"], ctypes.c_int
    slots, nbytes = ctypes.c_long(-1), ctypes.c_long(-1)
    cast = lambda v: ctypes.cast(ctypes.byref(v), ctypes.c_void_p)  # noqa: E731
    for capacity in (1, 2, 3, 8, 9, 4096, 100000, 1 << 28):
        assert size(capacity, cast(slots), cast(nbytes)) == 0 and slots.value == slots_of(capacity) and nbytes.value == 72 * slots_of(capacity), \
            f"{what}: workspace({capacity}) = {slots.value} slots, {nbytes.value} bytes"
    for capacity in (0, -1, (1 << 28) + 1):
        assert size(capacity, cast(slots), cast(nbytes)) == 1, f"{what}: workspace({capacity}) not refused"
    assert size(8, None, cast(nbytes)) == 1 and size(8, cast(slots), None) == 1


def case_host_tensor_refused():
    """Host tensors are refused by name: there is no reference function to hand over to."""
    import flowmap_amd

    x = case_inputs("tiny")
    host_tensor_refused(lambda: flowmap_amd.voxel_point_cloud(x["depth"], x["k"], x["ext"], x["colors"], 0.25), "flowmap_amd: tensors are on cpu.*no CPU fallback")


# ---- check 6: the other operators are left alone -------------------------------------------------------------------------------------------


def case_world_points_unchanged(dev):
    """export.world_point_cloud against the reference's recorded points (tests/golden/fn_export.npz) exactly as before, and bit-equal
    before and after voxel_point_cloud calls on the same tensors."""
    import flowmap_amd
    from flowmap_amd import export

    z = load_golden("fn_export")
    args = [t(z[key]).to(dev) for key in ("depths", "intrinsics", "extrinsics", "colors")]
    before = export.world_point_cloud(*args)
    flowmap_amd.voxel_point_cloud(*args, 0.05, details=True)
    after = export.world_point_cloud(*args)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert float((before[0].cpu() - t(z["points"])).abs().max()) < 1e-5 and torch.equal(before[1].cpu(), t(z["point_colors"]))


def case_training_untouched(dev, tracking, fuse):
    """operator_checks.train, 3 steps from step 1 after the warm-up, with and without Model.point_cloud between forward and backward
    (coloured from the batch, with details) and between the steps: operator_checks.assert_training_untouched with ``voxel_cloud`` the one
    counter that differs — a LazyExtrinsics handed in is still unevaluated afterwards, and a flow-only step does hand one in."""
    steps = 3
    mid = lambda ns: ns.model.point_cloud(ns.out, ns.batch, voxel_size=0.05, details=True)  # noqa: E731
    after = lambda ns: ns.model.point_cloud(ns.out, voxel_size=0.1, min_count=2)  # noqa: E731
    plain = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True, prepare=batch_colours)
    with_calls = train(dev, tracking=tracking, fuse=fuse, steps=steps, first_step=1, warm_up=True, prepare=batch_colours, calls=(mid, after))
    assert_training_untouched(plain, with_calls, "voxel_cloud", 2 * steps)
    if not tracking:
        assert all(was for was, _ in with_calls.lazy_kept), "a flow-only training step hands out a LazyExtrinsics: the case must exercise it"
    first, second = with_calls.seen[0], with_calls.seen[1]
    assert first.rgb is not None and tuple(first.voxel_of.shape) == (5, 24, 32) and len(first) > 100
    assert second.rgb is None and second.voxel_of is None and int(second.count.min()) >= 2


# ---- check 7: memory (GPU) ---------------------------------------------------------------------------------------------------------------


def case_memory(dev, name):
    """Peak allocated bytes during a call stay below what world_point_cloud alone allocates for the same input (its xyz and rgb: 24 bytes a
    point) plus the stated workspace (fm_voxel_cloud_workspace) — no point cloud and no key tensor are formed."""
    import flowmap_amd

    capacity = len(run(name, dev)[1]["count"])  # (sized to the cloud, as a caller who knows it would)
    x, voxel_size, kw = on_device(name, dev)
    kw["capacity"] = capacity
    f, h, w = x["depth"].shape
    flowmap_amd.voxel_point_cloud(x["depth"], x["k"], x["ext"], x["colors"], voxel_size, **kw)  # (warm: libraries loaded, allocator primed)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = flowmap_amd.voxel_point_cloud(x["depth"], x["k"], x["ext"], x["colors"], voxel_size, **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    workspace = 72 * slots_of(capacity)
    cloud = 24 * f * h * w
    slack = 16 * 512  # (the caching allocator's granularity on the call's small tensors: K⁻¹, the counters, the five outputs, the sorted copies)
    print(f"  {name}: peak {peak} B; world_point_cloud's outputs {cloud} B, workspace {workspace} B; {len(got)} voxels at capacity {capacity}")
    assert len(got) > 0 and peak <= cloud + workspace + slack, f"peak {peak} B > the point cloud's {cloud} + workspace {workspace}"


# ---- check 8: Model.point_cloud and write_ply ----------------------------------------------------------------------------------------


def case_model_point_cloud(dev, tmp_path):
    import flowmap_amd
    from flowmap_amd import Batch, ModelOutput
    from flowmap_amd.export import read_ply
    from flowmap_amd.model.model import Model
    from flowmap_amd.model.projection import LazySurfaces

    x, voxel_size, _ = on_device("wide", dev)
    depth, k, ext = x["depth"][None], x["k"][None], x["ext"][None]
    out = ModelOutput(depth, LazySurfaces(depth, k), k, ext, None)
    direct = flowmap_amd.voxel_point_cloud(x["depth"], x["k"], x["ext"], x["colors"], voxel_size, min_count=2)
    same_cloud(Model.point_cloud(None, out, Batch(x["colors"][None]), voxel_size=voxel_size, min_count=2), direct, "Model.point_cloud")
    bare = Model.point_cloud(None, out, voxel_size=voxel_size, min_count=2)
    assert bare.rgb is None and torch.equal(bare.xyz, direct.xyz) and torch.equal(bare.first, direct.first)
    path = tmp_path / "cloud.ply"
    direct.write_ply(path)
    xyz, rgb = read_ply(path)
    assert np.array_equal(xyz.view(np.uint32), bits(direct.xyz)) and len(direct) > 0
    assert np.array_equal(rgb, (direct.rgb.cpu().numpy() * 255).astype(np.float32).astype(np.uint8) / 255.0)
    bare.write_ply(path)
    assert np.array_equal(read_ply(path)[1], np.zeros((len(bare), 3)))
