"""The explicit-point function kernels of fm_points.hip — unproject, reproject / project, the bilinear sampler, Mapping.forward,
align_rigid and the exporter's world_point_cloud — at every edge of their launch geometry.  Shared by the CPU (host double) and GPU
modules; the host double runs the same per-element functions in plain loops and checks no launch limit, so only the GPU module says
anything about grids, strides, group offsets, caps and atomics.

Sizes, from ``blocks_for(n, per_thread, cap) = clamp(ceil(n / (256·per_thread)), 1, cap)`` and the launches in fm_points.hip (a block
is 256 threads, the grid is (blocks_for(points), groups), every kernel walks ``i = block·256 + thread; i < n; i += blocks·256``):

* unproject, reproject, mapping, world_points — ``blocks_for(n, 4, 4096)``: ONE block, making ceil(n / 256) <= 4 trips, until
  n = 1024; a second block at 1025 (each thread then makes ceil(n / (256·blocks)) trips: 2049 -> 3 blocks x 3 trips); the cap binds
  above P4 = 4096·1024 = 4 194 304, where a fifth trip begins.  POINTS brackets the wave (63, 64, 65), the block (255, 256, 257), the
  one-block limit (1023, 1024, 1025), the two-block limit (2047, 2049) and holds one many-block size; POINTS_CAPPED brackets P4.
* bilinear_* — ``blocks_for(p, 1, 4096)``: one thread per point and no second trip until p > 4096·256 = 2²⁰.
* rigid_* — ``blocks_for(n, 4, 1024)``: the cap binds above 1024·1024 = 2²⁰.
* reproject_finalize_kernel, pose_solve*, kinv_grad_to_k_kernel launch (g + 63) / 64 blocks of 64 over the groups: MANY_GROUPS
  brackets one block (63, 64, 65) and holds a many-block count, at 5 and 257 points.
* block_accumulate<NV> reduces 16 values at a time: <9> (unproject's K⁻¹ sums, rigid pass 2) is one chunk, <18> (reproject) a full
  chunk and one with 2 live values, <7> rigid pass 1; wave -> LDS -> one fp64 atomicAdd per block and value, so every size with more
  than one block exercises the inter-block atomics.  The spikes (a cotangent, or a weight, that singles out ONE index: 0, the last
  thread of a block, the first of the next, the one-block limit, n−1, and the grid's thread count ``pass`` with its neighbours)
  make a dropped or doubled point visible that a tolerance of 1e-4 over a million points cannot see; the exact census (inputs whose
  every partial sum is an integer below 2²⁴ in units of a power of two) is compared BIT FOR BIT, in any summation order.

Truth is always a plain fp64 evaluation by the oracle on ``.double()`` inputs with fp64 autograd, ``ref32`` the same call in fp32 on
the CPU; ``gate`` (prep_optim_cases) holds ours, norm-wise and element-wise, to max(floor, 2 x ref32's own measured error) with the
floors tests/cases.py holds these operators to (FLOOR_*).  The sampler has no floor of its own there (it is only tested through
compute_track_flow at reproject's 1e-5 / 1e-4): a sample is a convex combination of four taps whose weights carry a handful of fp32
roundings of a coordinate below 8 (the images are at most 8 wide; the one 40-wide image, case_bilinear above 2¹⁶ points, rounds its
coordinates to 2e-6 of a pixel in ATen's formula and ours alike, which is the gate's ref32 term), i.e. what unproject's value carries,
and its image gradient is an fp32 sum like unproject's as long as a pixel collects thousands of terms, not hundreds of thousands
(case_bilinear) — so it is held to unproject's floors, 1e-6 and 1e-5.  Every figure is printed before it is asserted.

Entry points reached through the C ABI write into ``Carved`` buffers: guard bands checked bit for bit, outputs pre-filled with a
sentinel, inputs compared bit for bit afterwards, and the fp64 accumulators (kinv_acc, reproject's acc, stats) pre-filled with
garbage — the Python layer hands the kernels ``torch.empty``, so the entry point's own memset is under test.

``bilinear_taps`` (fm_math.h) and wild coordinates: ix = ((x·2 − 1 + 1)·w − 1) / 2 is clamped with ``fminf(w − 1, fmaxf(ix, 0))``
BEFORE floorf and the int conversion, so 0, 1, half a pixel outside, ±1e30 and ±inf (fmaxf(−inf, 0) = 0, fminf(w − 1, +inf) = w − 1)
all end with 0 <= x0 <= w − 1; the only tap that can leave the image is x0 + 1 = w (at the clamped right / bottom edge), which the
``in`` flags drop (its weight is exactly 0 there).  fmaxf(NaN, 0) = 0 too: a NaN coordinate samples pixel 0 — ATen's CPU and GPU
builds disagree about that input, so only "nothing outside the buffers, every other point untouched" is pinned for it."""

from __future__ import annotations

import contextlib

import pytest
import torch

from conftest import load_golden, t as as_tensor
from oracle import flowmap_oracle as orc
from prep_optim_cases import FULL_SIZE, SENTINEL, Carved, abi, emit, errors, gate, refused, same_bits, stream  # noqa: F401

FLOOR_UNPROJECT, FLOOR_UNPROJECT_GRAD = 1e-6, 1e-5  # cases.case_grid_and_unproject
FLOOR_REPROJECT, FLOOR_REPROJECT_GRAD = 1e-5, 1e-4  # cases.case_flow_positions / case_projection_edges
FLOOR_MAPPING = 1e-6  # cases.case_mappings
FLOOR_RIGID, FLOOR_RIGID_GRAD = 1e-5, 1e-4  # cases.case_align_rigid
FLOOR_WORLD = 2e-6  # cases.case_export
FLOOR_SAMPLE, FLOOR_SAMPLE_GRAD = FLOOR_UNPROJECT, FLOOR_UNPROJECT_GRAD  # (module docstring)

P4 = 4096 * 1024
POINTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 5000)
POINTS_CAPPED = (P4 - 1, P4, P4 + 1, P4 + 1025)
SAMPLE_POINTS = (1, 63, 64, 65, 255, 256, 257, 1025)
SAMPLE_POINTS_CAPPED = ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 259)
CHANNELS = (1, 3, 4)
RIGID_POINTS = (4, 64, 65, 256, 257, 1024, 1025, 5000)
RIGID_POINTS_CAPPED = (1 << 20, (1 << 20) + 1, (1 << 20) + 1027)
GROUPS = (1, 2, 3)
MANY_GROUPS = (63, 64, 65, 300)
MANY_GROUPS_POINTS = (5, 257)
OVER_GROUPS = (65535, 65536, 70001)  # one launch's grid.y, one more, and a second slice of some length
OVER_POINTS = (1, 3)
KINDS = ("huber", "l1", "l2")
STAT_STRIDE, GARBAGE = 16, 12345.678


def shapes(points, capped=()):
    """[(groups, points)]: every size with 1, 2 and 3 groups, MANY_GROUPS at 5 and 257 points, the capped sizes with 1 and 2."""
    return ([(g, n) for n in points for g in GROUPS] + [(g, n) for g in MANY_GROUPS for n in MANY_GROUPS_POINTS]
            + [(g, n) for n in capped for g in (1, 2)])


def shape_id(c):
    return "x".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


def blocks_for(n, per_thread=4, cap=4096):
    return max(1, min(cap, (n + 256 * per_thread - 1) // (256 * per_thread)))


def spike_indices(n, per_thread=4, cap=4096):
    sweep = blocks_for(n, per_thread, cap) * 256  # threads of the grid: index i and i + sweep belong to the same thread
    return sorted({i for i in (0, 255, 256, 1023, 1024, n - 1, sweep - 1, sweep, sweep + 1) if 0 <= i < n})


# ---- inputs ----------------------------------------------------------------------------------------------------------------


def gen_of(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (1 << 31))


def rand_k(gen, g):
    """General K per group (skew, off-centre principal point), as oracle/make_golden.py's rand_k."""
    k = torch.eye(3).repeat(g, 1, 1)
    k[:, 0, 0] = 0.8 + 0.3 * torch.rand((g,), generator=gen)
    k[:, 1, 1] = 0.9 + 0.3 * torch.rand((g,), generator=gen)
    k[:, 0, 1] = 0.02 * torch.randn((g,), generator=gen)
    k[:, 0, 2] = 0.5 + 0.05 * torch.randn((g,), generator=gen)
    k[:, 1, 2] = 0.5 + 0.05 * torch.randn((g,), generator=gen)
    return k


def rand_pose(gen, g, scale=0.2):
    """Rodrigues rotation + translation per group, as oracle/make_golden.py's rand_pose."""
    a = scale * torch.randn((g, 3), generator=gen)
    th = a.norm(dim=-1, keepdim=True).clamp_min(1e-9)
    ax = a / th
    kx = torch.zeros((g, 3, 3))
    kx[:, 0, 1], kx[:, 0, 2], kx[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    kx[:, 1, 2], kx[:, 2, 0], kx[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    r = torch.eye(3) + torch.sin(th)[..., None] * kx + (1 - torch.cos(th))[..., None] * (kx @ kx)
    e = torch.eye(4).repeat(g, 1, 1)
    e[:, :3, :3] = r
    e[:, :3, 3] = scale * torch.randn((g, 3), generator=gen)
    return e


def rand_points(gen, g, n):
    """Points in front of every rand_pose camera, at depth 1.5 .. 3.5: x / (z + eps) magnifies the rounding of z by 1 / z, so among
    thousands of N(2.5, 1) depths the few that land within 1e-3 of the camera plane would decide the norm of the whole comparison.
    The camera plane has its own case (case_projection_edges)."""
    p = torch.randn((g, n, 3), generator=gen) * 0.7
    p[..., 2] = 1.5 + 2.0 * torch.rand((g, n), generator=gen)
    return p


def leaf(x, dev, grad=True, dtype=torch.float32):
    return x.detach().to(dtype).to(dev).requires_grad_(grad)


def hold(what, ours, truth, floor):
    """ours against the fp64 truth where the operands are ONE point's contribution (a spike): a handful of fp32 roundings, no sum —
    so the floor itself is the bar, norm-wise and element-wise."""
    assert ours.shape == truth.shape, f"{what}: shapes {tuple(ours.shape)} / {tuple(truth.shape)}"
    assert bool(torch.isfinite(ours).all()), f"{what}: not finite"
    rel, mx, mabs = errors(ours.cpu(), truth)
    emit({"what": what, "n": int(truth.numel()), "rel": rel, "max": mx, "max_abs": mabs})
    assert rel <= floor and mx <= floor, f"{what}: rel {rel:.3e} / max {mx:.3e} > {floor:.1e}"


def grad_variants(names):
    """Every needs_input_grad pattern with at least one input: all of them, each alone, each left out."""
    n = len(names)
    out = [tuple(True for _ in names)]
    for i in range(n):
        out.append(tuple(j == i for j in range(n)))
        if n > 2:
            out.append(tuple(j != i for j in range(n)))
    return list(dict.fromkeys(out))


def run_variants(what, dev, fn, inputs, cot, floors, names):
    """``fn(*tensors)`` in fp64 (truth) and fp32 on the CPU (ref32) with all gradients, then ours on ``dev`` once per pattern of
    inputs that require a gradient (each pattern turns other output pointers of the backward null): values and the gradients asked
    for, through the gate."""
    ours_fn, oracle_fn = fn
    refs = {}
    for dtype in (torch.float64, torch.float32):
        xs = [leaf(x, "cpu", True, dtype) for x in inputs]
        out = oracle_fn(*xs)
        out.backward(cot.to(dtype))
        refs[dtype] = (out.detach(), [x.grad for x in xs])
    for pattern in grad_variants(names):
        xs = [leaf(x, dev, need) for x, need in zip(inputs, pattern)]
        out = ours_fn(*xs)
        out.backward(cot.to(dev))
        tag = "+".join(nm for nm, need in zip(names, pattern) if need)
        gate(f"{what} value [{tag}]", out.detach().cpu(), refs[torch.float64][0], refs[torch.float32][0], floors[0])
        for i, (nm, need) in enumerate(zip(names, pattern)):
            if need:
                gate(f"{what} g_{nm} [{tag}]", xs[i].grad.cpu(), refs[torch.float64][1][i], refs[torch.float32][1][i], floors[1])
            else:
                assert xs[i].grad is None
        for x, x0 in zip(xs, inputs):
            assert same_bits(x.detach().cpu(), x0), f"{what}: an input was written to"


def acc_buffer(doubles, dev):
    """``doubles`` fp64 values carved out of a float allocation (8-byte aligned: GUARD is even), pre-filled with garbage."""
    return Carved(2 * doubles, dev, fill=GARBAGE)


def acc_values(c, shape):
    return c.view.view(torch.float64).detach().cpu().clone().reshape(shape)


# ---- unproject -------------------------------------------------------------------------------------------------------------


def unproject_inputs(g, n, seed=0):
    gen = gen_of(g, n, seed)
    xy = torch.rand((g, n, 2), generator=gen) * 1.2 - 0.1
    z = 1 + torch.rand((g, n), generator=gen)
    return xy, z, rand_k(gen, g)


def case_unproject(dev, cfg):
    """fm.unproject_dense with one K per group, shared (n, 2) coordinates and per-group (g, n, 2) ones."""
    from flowmap_amd.model import projection as fm

    g, n = cfg
    xy, z, k = unproject_inputs(g, n)
    cot = torch.randn((g, n, 3), generator=gen_of(g, n, 1))
    for name, coords in (("shared xy", xy[0]), ("per-group xy", xy)):
        co = coords.to(dev)
        run_variants(f"unproject {g}x{n} {name}", dev,
                     (lambda zz, kk: fm.unproject_dense(co, zz, kk[:, None]), lambda zz, kk: orc.lift(coords.to(zz.dtype), zz, kk[:, None])),
                     (z, k), cot, (FLOOR_UNPROJECT, FLOOR_UNPROJECT_GRAD), ("z", "k"))
        assert same_bits(co.cpu(), coords)


def kinv_of(k):
    return torch.linalg.inv(k.double()).float()


def case_unproject_abi(dev, cfg):
    """fm_unproject_fwd / _bwd on carved buffers: sentinels, guards, inputs, and the K⁻¹ sums — pre-filled with garbage — under
    cotangents that are zero except at ONE index, which must leave that point's contribution alone."""
    g, n = cfg
    xy, z, k = unproject_inputs(g, n, seed=2)
    kinv = kinv_of(k)
    what = f"unproject abi {g}x{n}"
    cxy, cz, cki = Carved(xy.numel(), dev).set(xy), Carved(z.numel(), dev).set(z), Carved(kinv.numel(), dev).set(kinv)
    out = Carved(g * n * 3, dev)
    abi("fm_unproject_fwd", cxy.ptr, n * 2, cz.ptr, cki.ptr, g, n, out.ptr, stream(dev))
    out.check_guards(what)
    got = out.cpu((g, n, 3))
    assert not bool((got == SENTINEL).any()), f"{what}: {int((got == SENTINEL).sum())} outputs were never written"
    truth = (torch.einsum("gij,gnj->gni", kinv.double(), orc.append_one(xy.double()))) * z.double()[..., None]
    ref32 = (torch.einsum("gij,gnj->gni", kinv, orc.append_one(xy))) * z[..., None]
    gate(what, got, truth, ref32, FLOOR_UNPROJECT)
    zh = orc.append_one(xy.double()) * z.double()[..., None]  # (g, n, 3): z·[x, y, 1]
    spikes = spike_indices(n)
    values = torch.randn((g, len(spikes), 3), generator=gen_of(g, n, 3))
    cgo, g_z = Carved(g * n * 3, dev, fill=0.0), Carved(g * n, dev)  # (kept across the spikes and rewritten in place, on the device)
    go, gz = cgo.view.view(g, n, 3), g_z.view.view(g, n)
    for s, i in enumerate(spikes):
        go[:, i] = values[:, s].to(dev)
        g_z.view.fill_(SENTINEL)
        acc = acc_buffer(g * 9, dev)
        abi("fm_unproject_bwd", cxy.ptr, n * 2, cz.ptr, cki.ptr, cgo.ptr, g, n, g_z.ptr, acc.ptr, stream(dev))
        for c in (g_z, acc, cgo):
            c.check_guards(f"{what} spike {i}")
        want = torch.einsum("ga,gd->gad", values[:, s].double(), zh[:, i]).reshape(g, 9)
        hold(f"{what} kinv_acc spike {i}", acc_values(acc, (g, 9)), want, FLOOR_UNPROJECT_GRAD)
        ray = torch.einsum("gij,gj->gi", kinv.double(), orc.append_one(xy[:, i].double()))
        hold(f"{what} g_z spike {i}", gz[:, i].cpu(), (values[:, s].double() * ray).sum(-1), FLOOR_UNPROJECT_GRAD)
        gz[:, i] = 0
        assert not bool(gz.any()), f"{what} spike {i}: g_z is not zero away from the spike"
        # the null combinations at the entry point itself
        g_z.view.fill_(SENTINEL)
        abi("fm_unproject_bwd", cxy.ptr, n * 2, cz.ptr, cki.ptr, cgo.ptr, g, n, None, acc.ptr, stream(dev))
        hold(f"{what} kinv_acc spike {i}, no g_z", acc_values(acc, (g, 9)), want, FLOOR_UNPROJECT_GRAD)
        abi("fm_unproject_bwd", cxy.ptr, n * 2, cz.ptr, cki.ptr, cgo.ptr, g, n, g_z.ptr, None, stream(dev))
        assert not bool((g_z.view == SENTINEL).any()), f"{what} spike {i}: g_z was not written when kinv_acc is null"
        go[:, i] = 0
    for c, x in ((cxy, xy), (cz, z), (cki, kinv)):
        c.check_guards(what)
        assert same_bits(c.view.cpu(), x.reshape(-1)), f"{what}: an input was written to"


# ---- reproject / project / flow positions ----------------------------------------------------------------------------------


def case_reproject(dev, cfg):
    from flowmap_amd.model import projection as fm

    g, n = cfg
    gen = gen_of(g, n, 4)
    xyz, tr, k = rand_points(gen, g, n), rand_pose(gen, g), rand_k(gen, g)
    cot = torch.randn((g, n, 2), generator=gen)
    run_variants(f"reproject {g}x{n}", dev,
                 (lambda p, tt, kk: fm.reproject_points(p, tt[:, None], kk[:, None]), lambda p, tt, kk: orc.warp_points(p, tt[:, None], kk[:, None])),
                 (xyz, tr, k), cot, (FLOOR_REPROJECT, FLOOR_REPROJECT_GRAD), ("xyz", "t", "k"))


def case_project(dev, cfg):
    """fm.project (world -> image through the inverse extrinsics, plus the in-front test) and project_camera_space."""
    from flowmap_amd.model import projection as fm

    g, n = cfg
    gen = gen_of(g, n, 5)
    xyz, ext, k = rand_points(gen, g, n), rand_pose(gen, g), rand_k(gen, g)
    cot = torch.randn((g, n, 2), generator=gen)
    run_variants(f"project {g}x{n}", dev,
                 (lambda p, e, kk: fm.project(p, e[:, None], kk[:, None])[0], lambda p, e, kk: orc.world_to_image(p, e[:, None], kk[:, None])[0]),
                 (xyz, ext, k), cot, (FLOOR_REPROJECT, FLOOR_REPROJECT_GRAD), ("xyz", "e", "k"))
    front = fm.project(xyz.to(dev), ext[:, None].to(dev), k[:, None].to(dev))[1].cpu()
    truth_front = orc.world_to_image(xyz.double(), ext[:, None].double(), k[:, None].double())
    cam_z = orc.matvec(torch.linalg.inv(ext[:, None].double()), orc.append_one(xyz.double()))[..., 2]
    sure = cam_z.abs() > 1e-5  # (a point within rounding of the camera plane may fall on either side)
    assert torch.equal(front[sure], truth_front[1][sure]), f"project {g}x{n}: the in-front test"
    run_variants(f"project_camera_space {g}x{n}", dev,
                 (lambda p, kk: fm.project_camera_space(p, kk[:, None]), lambda p, kk: orc.pinhole(p, kk[:, None])),
                 (xyz, k), cot, (FLOOR_REPROJECT, FLOOR_REPROJECT_GRAD), ("xyz", "k"))


def case_flow_positions(dev, cfg):
    """compute_forward_flow / compute_backward_flow on a 1-D grid (as IntrinsicsSoftmin calls them): g pairs of n points.  The
    cameras are a video's: poses of scale 0.05, so that the relative pose of two neighbours (up to twice a pose apart) leaves every
    point well in front of both (rand_points)."""
    from flowmap_amd.model import projection as fm

    g, n = cfg
    gen = gen_of(g, n, 6)
    surfaces, ext, k = rand_points(gen, g + 1, n)[None], rand_pose(gen, g + 1, scale=0.05)[None], rand_k(gen, g + 1)[None]
    cot = torch.randn((1, g, n, 2), generator=gen)
    for name, ours, theirs in (("forward", fm.compute_forward_flow, orc.forward_flow_positions), ("backward", fm.compute_backward_flow, orc.backward_flow_positions)):
        run_variants(f"flow positions {name} {g}x{n}", dev, (ours, theirs), (surfaces, ext, k), cot, (FLOOR_REPROJECT, FLOOR_REPROJECT_GRAD), ("surfaces", "e", "k"))


def case_reproject_abi(dev, cfg):
    """fm_reproject_fwd / _bwd on carved buffers, the 18 sums per group pre-filled with garbage, under cotangents that are zero
    except at one index: g_t, g_k and g_xyz must then be that one point's."""
    g, n = cfg
    gen = gen_of(g, n, 7)
    xyz, tr, k = rand_points(gen, g, n), rand_pose(gen, g), rand_k(gen, g)
    what = f"reproject abi {g}x{n}"
    cx, ct, ck = Carved(xyz.numel(), dev).set(xyz), Carved(tr.numel(), dev).set(tr), Carved(k.numel(), dev).set(k)
    out = Carved(g * n * 2, dev)
    abi("fm_reproject_fwd", cx.ptr, ct.ptr, ck.ptr, g, n, out.ptr, stream(dev))
    out.check_guards(what)
    got = out.cpu((g, n, 2))
    assert not bool((got == SENTINEL).any()), f"{what}: {int((got == SENTINEL).sum())} outputs were never written"
    gate(what, got, orc.warp_points(xyz.double(), tr[:, None].double(), k[:, None].double()), orc.warp_points(xyz, tr[:, None], k[:, None]), FLOOR_REPROJECT)
    spikes = spike_indices(n)
    values = torch.randn((g, len(spikes), 2), generator=gen)
    cgo, g_xyz = Carved(g * n * 2, dev, fill=0.0), Carved(g * n * 3, dev)  # (kept across the spikes and rewritten in place, on the device)
    go, gx = cgo.view.view(g, n, 2), g_xyz.view.view(g, n, 3)
    for s, i in enumerate(spikes):
        go[:, i] = values[:, s].to(dev)
        p64, t64, k64 = (leaf(x, "cpu", True, torch.float64) for x in (xyz[:, i : i + 1], tr, k))
        (orc.warp_points(p64, t64[:, None], k64[:, None]) * values[:, s : s + 1].double()).sum().backward()
        for with_xyz in (True, False):
            g_xyz.view.fill_(SENTINEL)
            g_t, g_k, acc = Carved(g * 16, dev), Carved(g * 9, dev), acc_buffer(g * 18, dev)
            abi("fm_reproject_bwd", cx.ptr, ct.ptr, ck.ptr, cgo.ptr, g, n, g_xyz.ptr if with_xyz else None, g_t.ptr, g_k.ptr, acc.ptr, stream(dev))
            for c in (g_xyz, g_t, g_k, acc, cgo):
                c.check_guards(f"{what} spike {i}")
            tag = f"{what} spike {i}" + ("" if with_xyz else ", no g_xyz")
            hold(f"{tag} g_t", g_t.cpu((g, 4, 4)), t64.grad, FLOOR_REPROJECT_GRAD)
            hold(f"{tag} g_k", g_k.cpu((g, 3, 3)), k64.grad, FLOOR_REPROJECT_GRAD)
            if with_xyz:
                hold(f"{tag} g_xyz", gx[:, i].cpu(), p64.grad[:, 0], FLOOR_REPROJECT_GRAD)
                gx[:, i] = 0
                assert not bool(gx.any()), f"{tag}: g_xyz is not zero away from the spike"
            else:
                assert bool((g_xyz.view == SENTINEL).all()), f"{tag}: a null g_xyz was written through another pointer"
        if s == 0:  # null g_t / g_k (what Reproject.backward passes for inputs that need no gradient)
            g_xyz.view.fill_(SENTINEL)
            acc = acc_buffer(g * 18, dev)
            abi("fm_reproject_bwd", cx.ptr, ct.ptr, ck.ptr, cgo.ptr, g, n, g_xyz.ptr, None, None, acc.ptr, stream(dev))
            for c in (g_xyz, acc):
                c.check_guards(what)
            hold(f"{what} spike {i}, no g_t / g_k: g_xyz", gx[:, i].cpu(), p64.grad[:, 0], FLOOR_REPROJECT_GRAD)
        go[:, i] = 0
    for c, x in ((cx, xyz), (ct, tr), (ck, k)):
        c.check_guards(what)
        assert same_bits(c.view.cpu(), x.reshape(-1)), f"{what}: an input was written to"


EDGE_GROUP = 2049


def case_projection_edges(dev):
    """The six fn_project_edge points (z = −eps twice, behind the camera, z = 1e-30, z = 0, and an ordinary one) at indices 0, 1024
    and n − 1 of a 2049-point group, every point at every place.  Forward against the golden values; backward finite, and against the
    fp64 truth — evaluated with z = −eps meaning −eps exactly, as it does in fp32 where float(−1e-5) + float(1e-5) = 0: the divide
    by zero and its clamp are the point of that input."""
    from flowmap_amd.model import projection as fm

    gold = load_golden("fn_project_edge")
    edge, k, edge_xy = as_tensor(gold["points"]), as_tensor(gold["k"]), as_tensor(gold["xy"])
    n, places = EDGE_GROUP, (0, 1024, EDGE_GROUP - 1)
    gen = gen_of(8)
    for turn in range(len(edge)):
        xyz = rand_points(gen, 1, n)[0]
        who = [(turn + j) % len(edge) for j in range(len(places))]
        for place, e in zip(places, who):
            xyz[place] = edge[e]
        cot = torch.randn((n, 2), generator=gen)
        refs = {}
        for dtype in (torch.float64, torch.float32):
            p = xyz.detach().to(dtype).clone()
            if dtype == torch.float64:
                p[(xyz[:, 2] + orc.EPS_PROJECT) == 0, 2] = -orc.EPS_PROJECT
            p, kk = p.requires_grad_(True), leaf(k, "cpu", True, dtype)
            out = orc.pinhole(p, kk)
            out.backward(cot.to(dtype))
            refs[dtype] = (out.detach(), p.grad, kk.grad)
        p, kk = leaf(xyz, dev), leaf(k, dev)
        out = fm.project_camera_space(p, kk)
        out.backward(cot.to(dev))
        what = f"projection edges, turn {turn}"
        for place, e in zip(places, who):
            rel, mx, mabs = errors(out[place].detach().cpu(), edge_xy[e])
            emit({"what": f"{what}: edge point {e} at {place}", "rel": rel, "max": mx, "max_abs": mabs})
            assert rel <= 1e-6, f"{what}: edge point {e} at index {place}: rel {rel:.3e} from the golden value"
        assert bool(torch.isfinite(out).all() and torch.isfinite(p.grad).all() and torch.isfinite(kk.grad).all()), f"{what}: not finite"
        # (autograd's own gradient at z = −eps is 0 / 0 = NaN, in fp64 and fp32 alike: ours is compared where the truth is finite)
        for name, ours, i, floor in (("value", out.detach(), 0, FLOOR_REPROJECT), ("g_xyz", p.grad, 1, FLOOR_REPROJECT_GRAD), ("g_k", kk.grad, 2, FLOOR_REPROJECT_GRAD)):
            ok = torch.isfinite(refs[torch.float64][i]) & torch.isfinite(refs[torch.float32][i])
            assert int(ok.sum()) >= ok.numel() - 6, f"{what} {name}: the truth is finite at {int(ok.sum())} of {ok.numel()} elements only"
            gate(f"{what} {name}", ours.cpu()[ok], refs[torch.float64][i][ok], refs[torch.float32][i][ok], floor)


# ---- the bilinear sampler --------------------------------------------------------------------------------------------------


def sample_reference(img, xy):
    return orc.bilinear_border(img[None], xy[None])[0]


def case_bilinear(dev, cfg):
    """_ops.BilinearSample on a 3 x 5 image (inexact pixel centres), coordinates from −0.1 to 1.1: values and the image gradient,
    whose atomicAdds collide by construction (15 pixels).  Above 2¹⁶ points the image is 24 x 40: the backward adds in fp32, as
    ATen's does, and a sum of N terms of either sign carries about 2⁻²⁴·√N of its own size in rounding — 4·2²⁰ / 15 = 280 000 adds
    per pixel put that at 1e-5 for the kernel and the fp32 reference alike (measured on the MI355X at 3 x 5 and 2²⁰ + 259 points:
    ours 4e-6 .. 1.8e-5, ATen's 5e-6 .. 1.9e-5 of max|g_img|), and the gate would compare two draws of that noise.  At 960 pixels
    a sum has 4 400 terms (about 2e-6), still a thousand collisions per pixel; the heavy collisions are the census's, bit for bit."""
    from flowmap_amd import _ops

    g, p, c = cfg
    hw = (3, 5) if p <= 1 << 16 else (24, 40)
    gen = gen_of(g, p, c)
    img = torch.randn((g, *hw, c), generator=gen)
    xy = (torch.rand((g, p, 2), generator=gen) * 1.2 - 0.1).to(dev)
    cot = torch.randn((g, p, c), generator=gen)
    run_variants(f"bilinear {g}x{p}x{c}", dev, (lambda im: _ops.BilinearSample.apply(im, xy), lambda im: sample_reference(im, xy.cpu().to(im.dtype))),
                 (img,), cot, (FLOOR_SAMPLE, FLOOR_SAMPLE_GRAD), ("img",))


CENSUS_HW = (4, 8)


def census_points(count, seed):
    """``count`` points on pixel centres of a 4 x 8 image — dyadic, so ((x·2 − 1 + 1)·w − 1) / 2 lands exactly on the column."""
    h, w = CENSUS_HW
    gen = gen_of(count, seed)
    col, row = torch.randint(0, w, (count,), generator=gen), torch.randint(0, h, (count,), generator=gen)
    xy = torch.stack(((col.float() + 0.5) / w, (row.float() + 0.5) / h), dim=-1)
    return xy, row * w + col


def case_bilinear_census(dev, points=(1 << 20) + 3, c=3):
    """Exact census of the sampler: every point taps ONE pixel with weight exactly 1, cotangents in {1, 2, 3} — every partial sum
    is an integer below 2²⁴ (the largest per-pixel sum is about 66 000), so the image gradient equals the fp64 count bit for bit
    in any order of the atomicAdds; one lost, doubled or misplaced add fails it.  Forward returns the tapped pixel bit for bit."""
    h, w = CENSUS_HW
    xy, pixel = census_points(points, 1)
    gen = gen_of(points, 2)
    img = torch.randn((1, h, w, c), generator=gen)
    cot = torch.randint(1, 4, (1, points, c), generator=gen).float()
    truth = torch.zeros((h * w, c), dtype=torch.float64).index_add_(0, pixel, cot[0].double())
    assert float(truth.max()) < 1 << 24
    # the inputs are exact: ATen's own fp32 grid_sample backward reproduces the fp64 count, and its forward the tapped pixel
    im32 = img.clone().requires_grad_(True)
    out32 = sample_reference(im32, xy[None])
    out32.backward(cot)
    assert same_bits(im32.grad.reshape(h * w, c), truth.float()) and same_bits(out32[0].detach(), img.reshape(h * w, c)[pixel]), "the census inputs are not exact"
    what = f"bilinear census {points}"
    cimg, cxy, ccot = Carved(img.numel(), dev).set(img), Carved(xy.numel(), dev).set(xy), Carved(cot.numel(), dev).set(cot)
    out, g_img = Carved(points * c, dev), Carved(h * w * c, dev, fill=0.0)
    abi("fm_bilinear_sample_fwd", cimg.ptr, cxy.ptr, 1, h, w, c, points, out.ptr, stream(dev))
    abi("fm_bilinear_sample_bwd", ccot.ptr, cxy.ptr, 1, h, w, c, points, g_img.ptr, stream(dev))
    for cc in (out, g_img, cimg, cxy, ccot):
        cc.check_guards(what)
    assert same_bits(out.cpu((points, c)), img.reshape(h * w, c)[pixel]), f"{what}: forward is not the tapped pixel"
    got = g_img.cpu((h * w, c))
    emit({"what": what, "n": int(got.numel()), "wrong": int((got.double() != truth).sum()), "max_abs": float((got.double() - truth).abs().max())})
    assert same_bits(got, truth.float()), f"{what}: {int((got.double() != truth).sum())} pixel sums differ from the count (max {float((got.double() - truth).abs().max())})"
    assert same_bits(cxy.view.cpu(), xy.reshape(-1)) and same_bits(ccot.view.cpu(), cot.reshape(-1)) and same_bits(cimg.view.cpu(), img.reshape(-1))


SAMPLER_EDGES = (0.0, 1.0, "centre", "half out low", "half out high", 1e30, -1e30, float("inf"), float("-inf"))


def case_sampler_edges(dev, points, hw=(3, 5), c=3):
    """Coordinates exactly 0 and 1, on pixel centres, half a pixel outside, ±1e30 and ±inf, one in a hundred among ordinary points:
    values and the image gradient against orc.bilinear_border.  (Why each ends in an in-range tap: module docstring.)"""
    h, w = hw
    gen = gen_of(points, 9)
    xy = torch.rand((1, points, 2), generator=gen)
    special = []
    for j, i in enumerate(range(0, points, 100)):
        e = SAMPLER_EDGES[j % len(SAMPLER_EDGES)]
        axis = (j // len(SAMPLER_EDGES)) % 3  # x alone, y alone, both
        for a, size in ((0, w), (1, h)):
            if axis == 2 or axis == a:
                pix = (j * 7) % size
                xy[0, i, a] = {"centre": (pix + 0.5) / size, "half out low": -0.5 / size, "half out high": 1 + 0.5 / size}.get(e, e)
        special.append(i)
    img = torch.randn((1, h, w, c), generator=gen)
    cot = torch.randn((1, points, c), generator=gen)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        im = img.to(dtype).requires_grad_(True)
        out = sample_reference(im, xy.to(dtype))
        out.backward(cot.to(dtype))
        refs[dtype] = (out.detach(), im.grad)
    assert bool(torch.isfinite(refs[torch.float64][0]).all())
    what = f"sampler edges {points}"
    cimg, cxy, ccot = Carved(img.numel(), dev).set(img), Carved(xy.numel(), dev).set(xy), Carved(cot.numel(), dev).set(cot)
    out, g_img = Carved(points * c, dev), Carved(h * w * c, dev, fill=0.0)
    abi("fm_bilinear_sample_fwd", cimg.ptr, cxy.ptr, 1, h, w, c, points, out.ptr, stream(dev))
    abi("fm_bilinear_sample_bwd", ccot.ptr, cxy.ptr, 1, h, w, c, points, g_img.ptr, stream(dev))
    for cc in (out, g_img, cimg, cxy, ccot):
        cc.check_guards(what)
    got = out.cpu((1, points, c))
    gate(f"{what} value", got, refs[torch.float64][0], refs[torch.float32][0], FLOOR_SAMPLE)
    gate(f"{what} value at the edges", got[:, special], refs[torch.float64][0][:, special], refs[torch.float32][0][:, special], FLOOR_SAMPLE)
    gate(f"{what} g_img", g_img.cpu((1, h, w, c)), refs[torch.float64][1], refs[torch.float32][1], FLOOR_SAMPLE_GRAD)
    # a NaN coordinate: nothing outside the buffers, every other point untouched
    poisoned = xy.clone()
    poisoned[0, special[1::2], 0] = float("nan")
    poisoned[0, special[::3], 1] = float("nan")
    bad = torch.isnan(poisoned).any(-1)[0]
    cxy.set(poisoned)
    out_nan, g_nan = Carved(points * c, dev), Carved(h * w * c, dev, fill=0.0)
    abi("fm_bilinear_sample_fwd", cimg.ptr, cxy.ptr, 1, h, w, c, points, out_nan.ptr, stream(dev))
    abi("fm_bilinear_sample_bwd", ccot.ptr, cxy.ptr, 1, h, w, c, points, g_nan.ptr, stream(dev))
    for cc in (out_nan, g_nan, cimg, cxy, ccot):
        cc.check_guards(what + ", NaN coordinates")
    assert same_bits(out_nan.cpu((1, points, c))[0, ~bad], got[0, ~bad]), f"{what}: a NaN coordinate disturbed another point"


# ---- mapping ---------------------------------------------------------------------------------------------------------------

MAPPING_SHAPE = (24, 36)


def case_mapping(dev, n, kind):
    """get_mapping(kind).forward on (n, 2) pairs whose residuals straddle the Huber knee (delta 0.01), one in seven exactly 0."""
    from flowmap_amd.loss.mapping import get_mapping
    from helpers import mapping_cfg

    gen = gen_of(n, KINDS.index(kind))
    a = torch.rand((n, 2), generator=gen)
    b = a + torch.randn((n, 2), generator=gen) * 0.01
    b[::7] = a[::7]
    cot = torch.randn((n,), generator=gen)
    mapping = get_mapping(mapping_cfg(kind))
    run_variants(f"mapping {kind} {n}", dev, (lambda x, y: mapping.forward(x, y, MAPPING_SHAPE), lambda x, y: orc.robust(x, y, MAPPING_SHAPE, kind, 0.01)),
                 (a, b), cot, (FLOOR_MAPPING, FLOOR_MAPPING), ("a", "b"))
    # the entry point on carved buffers
    from flowmap_amd.loss.mapping.mapping import aspect_correction

    ax, ay = aspect_correction(MAPPING_SHAPE)
    ca, cb, out = Carved(2 * n, dev).set(a), Carved(2 * n, dev).set(b), Carved(n, dev)
    abi("fm_mapping_fwd", ca.ptr, cb.ptr, n, KINDS.index(kind), 0.01, ax, ay, out.ptr, stream(dev))
    for c in (ca, cb, out):
        c.check_guards(f"mapping {kind} {n}")
    got = out.cpu()
    assert not bool((got == SENTINEL).any()), f"mapping {kind} {n}: {int((got == SENTINEL).sum())} outputs were never written"
    gate(f"mapping abi {kind} {n}", got, orc.robust(a.double(), b.double(), MAPPING_SHAPE, kind, 0.01), orc.robust(a, b, MAPPING_SHAPE, kind, 0.01), FLOOR_MAPPING)
    assert same_bits(ca.view.cpu(), a.reshape(-1)) and same_bits(cb.view.cpu(), b.reshape(-1))


# ---- align_rigid -----------------------------------------------------------------------------------------------------------


def rigid_inputs(g, n, seed=0):
    gen = gen_of(g, n, 10 + seed)
    p = torch.randn((g, n, 3), generator=gen)
    tr = rand_pose(gen, g, scale=0.5)
    q = torch.einsum("gij,gnj->gni", tr[:, :3, :3], p) + tr[:, None, :3, 3] + 0.01 * torch.randn((g, n, 3), generator=gen)
    w = 0.1 + 0.9 * torch.rand((g, n), generator=gen)
    return p, q, w


def case_align_rigid(dev, cfg):
    from flowmap_amd.model import procrustes as fp

    g, n = cfg
    p, q, w = rigid_inputs(g, n)
    cot = torch.randn((g, 4, 4), generator=gen_of(g, n, 11))
    run_variants(f"align_rigid {g}x{n}", dev, (fp.align_rigid, orc.rigid_fit), (p, q, w), cot, (FLOOR_RIGID, FLOOR_RIGID_GRAD), ("p", "q", "w"))


def stats_truth(p, q, w):
    p, q, w = p.double(), q.double(), w.double()
    ws = w.sum(-1)
    sp, sq = (w[..., None] * p).sum(-2), (w[..., None] * q).sum(-2)
    inv = 1.0 / (ws + 1e-8)
    pbar, qbar = sp * inv[:, None], sq * inv[:, None]
    cov = torch.einsum("gn,gna,gnd->gad", w, q - qbar[:, None], p - pbar[:, None])
    return torch.cat([ws[:, None], sp, sq, cov.reshape(-1, 9)], dim=-1)


def case_rigid_stats_abi(dev, cfg):
    """fm_align_rigid_stats on a garbage-filled stats buffer: both passes against the fp64 sums, with weights 1e-6 everywhere but
    at ONE index, which holds 1 — a pass that drops or doubles that point misses Σw by a factor, whatever the size."""
    g, n = cfg
    p, q, _ = rigid_inputs(g, n, seed=1)
    what = f"rigid stats {g}x{n}"
    cp, cq = Carved(p.numel(), dev).set(p), Carved(q.numel(), dev).set(q)
    for i in spike_indices(n, 4, 1024):
        w = torch.full((g, n), 1e-6)
        w[:, i] = 1.0
        cw, stats = Carved(w.numel(), dev).set(w), acc_buffer(g * STAT_STRIDE, dev)
        abi("fm_align_rigid_stats", cp.ptr, cq.ptr, cw.ptr, g, n, stats.ptr, stream(dev))
        stats.check_guards(f"{what} spike {i}")
        got, want = acc_values(stats, (g, STAT_STRIDE)), stats_truth(p, q, w)
        for gi in range(g):  # per group: a sum that landed in another group's slot cannot hide under the norm of the stack
            hold(f"{what} spike {i} group {gi} pass 1", got[gi, :7], want[gi, :7], FLOOR_RIGID)
            hold(f"{what} spike {i} group {gi} pass 2", got[gi, 7:], want[gi, 7:], FLOOR_RIGID)
        assert same_bits(cw.view.cpu(), w.reshape(-1))
    for c, x in ((cp, p), (cq, q)):
        c.check_guards(what)
        assert same_bits(c.view.cpu(), x.reshape(-1)), f"{what}: an input was written to"


def small_integers(shape, gen, signed=True):
    v = torch.randint(1, 4, shape, generator=gen).float()
    return v * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1) if signed else v


def case_sum_census(dev, cfg):
    """Exact census of the two fp64 accumulators fed by block_accumulate: unproject_bwd's kinv_acc with integer g_out and z in
    ±{1, 2, 3} and xy on the dyadic pixel centres of a 4 x 8 grid (every product a multiple of 1/16 below 2⁴), and pass 1 of
    rigid_stats (Σw, Σw·p, Σw·q) with w in {1, 2, 3} and p, q in ±{1, 2, 3}.  A thread's sum, a wave's and a block's stay integers
    (in sixteenths) far below 2²⁴, so every order of adding gives the fp64 sum exactly: compared bit for bit."""
    g, n = cfg
    gen = gen_of(g, n, 12)
    xy = torch.stack([census_points(n, 20 + i)[0] for i in range(g)])
    z, go = small_integers((g, n), gen), small_integers((g, n, 3), gen)
    kinv = kinv_of(rand_k(gen, g))
    want = torch.einsum("gna,gnd->gad", go.double(), orc.append_one(xy.double()) * z.double()[..., None]).reshape(g, 9)
    ref32 = torch.einsum("gna,gnd->gad", go, orc.append_one(xy) * z[..., None]).reshape(g, 9)
    assert float(want.abs().max()) * 16 < 1 << 24 and (n > 1 << 16 or torch.equal(ref32.double(), want)), "the census inputs are not exact"
    cxy, cz, cki, cgo = (Carved(x.numel(), dev).set(x) for x in (xy, z, kinv, go))
    g_z, acc = Carved(g * n, dev), acc_buffer(g * 9, dev)
    abi("fm_unproject_bwd", cxy.ptr, n * 2, cz.ptr, cki.ptr, cgo.ptr, g, n, g_z.ptr, acc.ptr, stream(dev))
    acc.check_guards(f"sum census {g}x{n}")
    got = acc_values(acc, (g, 9))
    emit({"what": f"kinv_acc census {g}x{n}", "n": 9 * g, "wrong": int((got != want).sum()), "max_abs": float((got - want).abs().max())})
    assert torch.equal(got, want), f"kinv_acc census {g}x{n}: {int((got != want).sum())} sums differ (max {float((got - want).abs().max())})"
    if n < 4:
        return
    p, q, w = small_integers((g, n, 3), gen), small_integers((g, n, 3), gen), small_integers((g, n), gen, signed=False)
    want = stats_truth(p, q, w)[:, :7]
    ref32 = torch.cat([w.sum(-1)[:, None], (w[..., None] * p).sum(-2), (w[..., None] * q).sum(-2)], dim=-1)
    assert float(want.abs().max()) < 1 << 24 and torch.equal(ref32.double(), want), "the census inputs are not exact"
    cp, cq, cw = (Carved(x.numel(), dev).set(x) for x in (p, q, w))
    stats = acc_buffer(g * STAT_STRIDE, dev)
    abi("fm_align_rigid_stats", cp.ptr, cq.ptr, cw.ptr, g, n, stats.ptr, stream(dev))
    stats.check_guards(f"sum census {g}x{n}")
    got = acc_values(stats, (g, STAT_STRIDE))[:, :7]
    emit({"what": f"rigid pass-1 census {g}x{n}", "n": 7 * g, "wrong": int((got != want).sum()), "max_abs": float((got - want).abs().max())})
    assert torch.equal(got, want), f"rigid pass-1 census {g}x{n}: {int((got != want).sum())} sums differ (max {float((got - want).abs().max())})"


# ---- world point cloud -----------------------------------------------------------------------------------------------------

WORLD_SHAPES = ((1, 1), (1, 257), (257, 1), (5, 7), (33, 31), (32, 32), (45, 91))
WORLD_FRAMES = (1, 2, 65)
WORLD_FULL_SIZE = (1, 1080, 1920)


def case_world_points(dev, cfg, warn=False):
    from flowmap_amd import export

    f, h, w = cfg
    gen = gen_of(f, h, w)
    depths, k, ext, colors = 1 + torch.rand((f, h, w), generator=gen), rand_k(gen, f), rand_pose(gen, f), torch.rand((f, 3, h, w), generator=gen)
    truth, truth_colors = orc.world_point_cloud(depths.double(), k.double(), ext.double(), colors.double())
    ref32, _ = orc.world_point_cloud(depths, k, ext, colors)
    on = [x.to(dev) for x in (depths, k, ext, colors)]
    pts, cols = export.world_point_cloud(*on)
    gate(f"world points {f}x{h}x{w}", pts.cpu(), truth, ref32, FLOOR_WORLD, warn=warn)
    for frame in sorted({0, f // 2, f - 1}):  # a frame read with another frame's K or pose cannot hide under the norm of the stack
        s = slice(frame * h * w, (frame + 1) * h * w)
        gate(f"world points {f}x{h}x{w} frame {frame}", pts[s].cpu(), truth[s], ref32[s], FLOOR_WORLD)
    assert same_bits(cols.cpu(), truth_colors.float()), f"world points {f}x{h}x{w}: colours"
    only, none = export.world_point_cloud(*on[:3])
    assert none is None and same_bits(only.cpu(), pts.cpu())
    for x, x0 in zip(on, (depths, k, ext, colors)):
        assert same_bits(x.cpu(), x0)


# ---- the three fixes -------------------------------------------------------------------------------------------------------


def case_over_groups(dev, g, n):
    """More groups than one launch's grid.y takes: a matrix per point through reproject_points and unproject_dense."""
    from flowmap_amd.model import projection as fm

    gen = gen_of(g, n, 13)
    xyz, tr, k = rand_points(gen, g, n), rand_pose(gen, g), rand_k(gen, g)
    run_variants(f"reproject {g}x{n}", dev,
                 (lambda p, tt, kk: fm.reproject_points(p, tt[:, None], kk[:, None]), lambda p, tt, kk: orc.warp_points(p, tt[:, None], kk[:, None])),
                 (xyz, tr, k), torch.randn((g, n, 2), generator=gen), (FLOOR_REPROJECT, FLOOR_REPROJECT_GRAD), ("xyz", "t", "k"))
    xy, z, _ = unproject_inputs(1, n, seed=3)
    z = z.expand(g, n) * (1 + torch.rand((g, 1), generator=gen))
    co = xy[0].to(dev)
    run_variants(f"unproject {g}x{n}", dev, (lambda zz, kk: fm.unproject_dense(co, zz, kk[:, None]), lambda zz, kk: orc.lift(xy[0].to(zz.dtype), zz, kk[:, None])),
                 (z.contiguous(), k), torch.randn((g, n, 3), generator=gen), (FLOOR_UNPROJECT, FLOOR_UNPROJECT_GRAD), ("z", "k"))


def case_over_groups_other_operators(dev, g=65536 + 3, n=2):
    """The sampler and align_rigid past one launch's groups (one size: their slicing loop is the same three lines)."""
    from flowmap_amd import _ops
    from flowmap_amd.model import procrustes as fp

    gen = gen_of(g, n, 14)
    img = torch.randn((g, 2, 2, 1), generator=gen)
    xy = torch.rand((g, n, 2), generator=gen).to(dev)
    run_variants(f"bilinear {g}x{n}", dev, (lambda im: _ops.BilinearSample.apply(im, xy), lambda im: sample_reference(im, xy.cpu().to(im.dtype))),
                 (img,), torch.randn((g, n, 1), generator=gen), (FLOOR_SAMPLE, FLOOR_SAMPLE_GRAD), ("img",))
    p, q, w = rigid_inputs(g, 4, seed=2)
    run_variants(f"align_rigid {g}x4", dev, (fp.align_rigid, orc.rigid_fit), (p, q, w), torch.randn((g, 4, 4), generator=gen),
                 (FLOOR_RIGID, FLOOR_RIGID_GRAD), ("p", "q", "w"))


@contextlib.contextmanager
def real_library():
    """The device build of the library (it loads without a GPU, as tests/test_abi.py relies on) for calls that are refused before
    the first HIP call; the host double is put back afterwards when it was in place."""
    from flowmap_amd import _lib
    from helpers import build_host_sim

    double = _lib.using_test_double()
    _lib.set_library_for_testing(None)
    try:
        yield
    finally:
        if double:
            _lib.set_library_for_testing(build_host_sim())


def point_entry_calls(dev, g, n, shift=0):
    """One call of each entry point that takes groups on grid.y, on carved host or device buffers: [(name, args, outputs)].
    ``shift``: bytes added to every pointer the kernels read or write as float2."""
    c = lambda count: Carved(count, dev)  # noqa: E731
    xy, z, ki, out3, go3, g_z, acc9 = c(g * n * 2), c(g * n), c(g * 9), c(g * n * 3), c(g * n * 3), c(g * n), c(2 * g * 9)
    xyz, tr, k, out2, g_xyz, g_t, g_k, acc18 = c(g * n * 3), c(g * 16), c(g * 9), c(g * n * 2), c(g * n * 3), c(g * 16), c(g * 9), c(2 * g * 18)
    img, samp, g_img = c(g * 4), c(g * n), c(g * 4)
    w, stats, aux, pg = c(g * n), c(2 * g * 16), c(2 * g * 40), c(2 * g * 20)
    st = stream(dev)
    calls = [
        ("fm_unproject_fwd", (xy.ptr + shift, n * 2, z.ptr, ki.ptr, g, n, out3.ptr, st), (out3,)),
        ("fm_unproject_bwd", (xy.ptr + shift, n * 2, z.ptr, ki.ptr, go3.ptr, g, n, g_z.ptr, acc9.ptr, st), (g_z, acc9)),
        ("fm_reproject_fwd", (xyz.ptr, tr.ptr, k.ptr, g, n, out2.ptr + shift, st), (out2,)),
        ("fm_reproject_bwd", (xyz.ptr, tr.ptr, k.ptr, out2.ptr + shift, g, n, g_xyz.ptr, g_t.ptr, g_k.ptr, acc18.ptr, st), (g_xyz, g_t, g_k, acc18)),
        ("fm_bilinear_sample_fwd", (img.ptr, xy.ptr + shift, g, 2, 2, 1, n, samp.ptr, st), (samp,)),
        ("fm_bilinear_sample_bwd", (samp.ptr, xy.ptr + shift, g, 2, 2, 1, n, g_img.ptr, st), (g_img,)),
    ]
    if not shift:
        calls += [("fm_align_rigid_stats", (xyz.ptr, go3.ptr, w.ptr, g, n, stats.ptr, st), (stats,)),
                  ("fm_align_rigid_bwd", (xyz.ptr, go3.ptr, w.ptr, g, n, aux.ptr, pg.ptr, g_xyz.ptr, out3.ptr, g_z.ptr, st), (g_xyz, out3, g_z))]
    else:
        a, b, m, g_a, g_b = c(g * n * 2), c(g * n * 2), c(g * n), c(g * n * 2), c(g * n * 2)
        calls += [("fm_unproject_fwd", (xy.ptr, n * 2 + 1, z.ptr, ki.ptr, g, n, out3.ptr, st), (out3,)),
                  ("fm_mapping_fwd", (a.ptr + shift, b.ptr, g * n, 0, 0.01, 1.0, 1.0, m.ptr, st), (m,)),
                  ("fm_mapping_fwd", (a.ptr, b.ptr + shift, g * n, 0, 0.01, 1.0, 1.0, m.ptr, st), (m,)),
                  ("fm_mapping_bwd", (a.ptr + shift, b.ptr, m.ptr, g * n, 0, 0.01, 1.0, 1.0, g_a.ptr, g_b.ptr, st), (g_a, g_b)),
                  ("fm_mapping_bwd", (a.ptr, b.ptr, m.ptr, g * n, 0, 0.01, 1.0, 1.0, g_a.ptr + shift, g_b.ptr, st), (g_a, g_b)),
                  ("fm_mapping_bwd", (a.ptr, b.ptr, m.ptr, g * n, 0, 0.01, 1.0, 1.0, None, g_b.ptr + shift, st), (g_a, g_b))]
    return calls


def assert_all_refused(calls, what):
    for name, args, outputs in calls:
        refused(name, *args)
        for c in outputs:
            assert bool((c.view == SENTINEL).all()), f"{what}: the refused {name} wrote to an output"
            c.check_guards(what)


def case_group_limit_refused():
    """The raw entry points keep refusing 65536 groups (the Python layer slices): the device build, on host memory — the check
    precedes the first HIP call, so nothing is launched and nothing dereferenced."""
    with real_library():
        assert_all_refused(point_entry_calls("cpu", 65536, 1), "65536 groups")


def case_misaligned_refused(double):
    """A pointer to coordinate pairs that is not 8-byte aligned (data_ptr() + 4), or an odd xy_group_stride, is refused before
    anything is launched, by the device build (on host memory) and by the host double alike; the outputs keep their sentinel."""
    with contextlib.nullcontext() if double else real_library():
        assert_all_refused(point_entry_calls("cpu", 2, 5, shift=4), "misaligned pairs")


def case_misaligned_views(dev, offset):
    """A contiguous view that starts ``offset`` floats into its allocation gives the bits of an aligned clone, for all four
    operators that move pairs as float2: the Python layer copies it, and no kernel ever sees the odd pointer."""
    from flowmap_amd import _ops
    from flowmap_amd.loss.mapping import get_mapping
    from flowmap_amd.model import projection as fm
    from helpers import mapping_cfg

    g, n = 2, 259
    gen = gen_of(offset, 15)

    def view_of(x):
        buf = torch.zeros((x.numel() + 8,))
        buf[offset : offset + x.numel()] = x.reshape(-1)
        v = buf.to(dev)[offset : offset + x.numel()].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 8 == (4 * offset) % 8
        return v

    xy, z, k = unproject_inputs(g, n, seed=4)
    xyz, tr = rand_points(gen, g, n), rand_pose(gen, g)
    img, cot2 = torch.randn((g, 3, 5, 3), generator=gen), torch.randn((g, n, 2), generator=gen)
    a, b = torch.rand((g * n, 2), generator=gen), torch.rand((g * n, 2), generator=gen)
    mapping = get_mapping(mapping_cfg("huber"))

    def run(wrap):
        out = {}
        zz, kk = leaf(z, dev), leaf(k, dev)
        out["unproject shared"] = fm.unproject_dense(wrap(xy[0]), zz, kk[:, None])
        out["unproject per group"] = fm.unproject_dense(wrap(xy), zz, kk[:, None])
        (out["unproject shared"].sum() + 2 * out["unproject per group"].sum()).backward()
        out["unproject g_z"], out["unproject g_k"] = zz.grad, kk.grad
        p, tt = leaf(xyz, dev), leaf(tr, dev)
        out["reproject"] = fm.reproject_points(p, tt[:, None], kk.detach()[:, None])
        out["reproject"].backward(wrap(cot2))  # (the cotangent is what the backward reads as pairs)
        out["reproject g_xyz"], out["reproject g_t"] = p.grad, tt.grad
        im = leaf(img, dev)
        out["sample"] = _ops.BilinearSample.apply(im, wrap(xy))
        out["sample"].sum().backward()
        out["sample g_img"] = im.grad
        aa, bb = wrap(a).requires_grad_(True), wrap(b).requires_grad_(True)
        out["mapping"] = mapping.forward(aa, bb, MAPPING_SHAPE)
        out["mapping"].sum().backward()
        out["mapping g_a"], out["mapping g_b"] = aa.grad, bb.grad
        return {name: v.detach().cpu() for name, v in out.items()}

    aligned, shifted = run(lambda x: x.clone().to(dev)), run(view_of)
    for name in aligned:
        if name == "sample g_img":  # (float atomics: the order of the adds is not fixed on the GPU)
            rel, mx, _ = errors(shifted[name], aligned[name])
            assert rel <= FLOOR_SAMPLE_GRAD and mx <= FLOOR_SAMPLE_GRAD, f"misaligned view +{offset}: {name}"
        else:
            assert same_bits(shifted[name], aligned[name]), f"misaligned view +{offset}: {name} differs from the aligned run"


def case_empty(dev):
    """Zero points, or zero groups: empty outputs of the right shape without a launch, zero gradients of the right shape for K, T,
    z and the image; align_rigid keeps raising, and says why."""
    from flowmap_amd import _ops
    from flowmap_amd.loss.mapping import get_mapping
    from flowmap_amd.model import procrustes as fp
    from flowmap_amd.model import projection as fm
    from helpers import mapping_cfg

    gen = gen_of(16)
    for g, n in ((3, 0), (0, 5), (0, 0)):
        k, tr = leaf(rand_k(gen, g), dev), leaf(rand_pose(gen, g), dev)
        z, xyz = leaf(torch.rand((g, n)), dev), leaf(torch.rand((g, n, 3)), dev)
        out = fm.unproject_dense(torch.rand((n, 2)).to(dev), z, k[:, None])
        assert tuple(out.shape) == (g, n, 3)
        out.sum().backward()
        assert tuple(z.grad.shape) == (g, n) and tuple(k.grad.shape) == (g, 3, 3) and not bool(k.grad.any())
        k.grad = None
        out = fm.reproject_points(xyz, tr[:, None], k[:, None])
        assert tuple(out.shape) == (g, n, 2)
        out.sum().backward()
        assert tuple(xyz.grad.shape) == (g, n, 3) and tuple(tr.grad.shape) == (g, 4, 4) and tuple(k.grad.shape) == (g, 3, 3)
        assert not bool(tr.grad.any()) and not bool(k.grad.any())
        img = leaf(torch.rand((g, 3, 5, 2)), dev)
        out = _ops.BilinearSample.apply(img, torch.rand((g, n, 2)).to(dev))
        assert tuple(out.shape) == (g, n, 2)
        out.sum().backward()
        assert tuple(img.grad.shape) == (g, 3, 5, 2) and not bool(img.grad.any())
        with pytest.raises(RuntimeError, match="empty point set"):
            fp.align_rigid(torch.rand((g, n, 3)).to(dev), torch.rand((g, n, 3)).to(dev), torch.rand((g, n)).to(dev))
    a = leaf(torch.rand((0, 2)), dev)
    out = get_mapping(mapping_cfg("huber")).forward(a, torch.rand((0, 2)).to(dev), MAPPING_SHAPE)
    assert tuple(out.shape) == (0,)
    out.sum().backward()
    assert tuple(a.grad.shape) == (0, 2)
