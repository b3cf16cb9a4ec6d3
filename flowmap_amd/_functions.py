"""Function-level operators on explicit point sets — ``torch.autograd.Function``s over the C ABI through ctypes: Unproject, Reproject,
BilinearSample, RobustMapping (flowmap/model/projection.py, flowmap/loss/mapping) and AlignRigid (flowmap/model/procrustes.py:7-51).
The per-step fused operators are in _ops.py / csrc/fm_torch.cpp."""

from __future__ import annotations

import ctypes
import warnings
import weakref
from typing import Optional

import torch
from torch import Tensor

from ._lib import call, check_device, ptr, stream_for, torch_ops  # noqa: F401
from ._base import AUX_STRIDE, PAIR_GRAD_STRIDE, STAT_STRIDE, TRACK_TILE, _f32c, _guard  # noqa: F401


def intrinsics_inverse(k):
    from ._ops import intrinsics_inverse as impl  # (K^-1 is kept on K: _ops.intrinsics_inverse; imported late — _ops imports this module)

    return impl(k)


# --------------------------------------------------------------------------------------
# Function-level building blocks on explicit point sets
# --------------------------------------------------------------------------------------

MAX_GROUPS = 65535  # groups one call of these entry points takes (they ride on grid.y); more are walked in slices


def _group_slices(g: int):
    """[(first, end)] covering g groups, at most MAX_GROUPS each."""
    return [(s, min(s + MAX_GROUPS, g)) for s in range(0, g, MAX_GROUPS)]


def _rows(t: Optional[Tensor], s: int, e: int) -> Optional[Tensor]:
    """Groups [s, e) of a contiguous (G, ...) tensor (a view: a whole number of rows, so a pair-aligned tensor stays pair-aligned)."""
    return t if t is None or (s == 0 and e == t.shape[0]) else t[s:e]


def _pairs(t: Tensor, what: str) -> Tensor:
    """_f32c for a tensor of coordinate pairs, which the kernels move as one float2: a contiguous view that starts an odd number of
    floats into its allocation is copied to a fresh one (the entry points refuse a pointer that is not 8-byte aligned)."""
    t = _f32c(t, what)
    if t.numel() and t.data_ptr() % 8:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


class Unproject(torch.autograd.Function):
    """unproject (flowmap/model/projection.py:76-90) for G groups of N points:
    xy (N,2) shared or (G,N,2); z (G,N); k (G,3,3) -> (G,N,3)."""

    @staticmethod
    def forward(ctx, xy, z, k):
        dev = check_device(xy, z, k)
        if xy.requires_grad:
            raise RuntimeError("flowmap_amd: gradients w.r.t. image coordinates are not supported")
        xy, z, k = _pairs(xy, "coordinates"), _f32c(z, "z"), _f32c(k, "intrinsics")
        g, n = z.shape
        shared = xy.dim() == 2
        out = torch.empty((g, n, 3), dtype=torch.float32, device=dev)
        ctx.shared = shared
        if g == 0 or n == 0:  # an empty point set: nothing to launch
            ctx.save_for_backward(xy, z, torch.empty_like(k))
            return out
        kinv = intrinsics_inverse(k)
        with _guard(dev):
            for s, e in _group_slices(g):
                call("fm_unproject_fwd", ptr(xy if shared else _rows(xy, s, e)), 0 if shared else n * 2, ptr(_rows(z, s, e)), ptr(_rows(kinv, s, e)),
                     e - s, n, ptr(_rows(out, s, e)), stream_for(z))
        ctx.save_for_backward(xy, z, kinv)
        return out

    @staticmethod
    def backward(ctx, g_out):
        xy, z, kinv = ctx.saved_tensors
        g, n = z.shape
        g_out = _f32c(g_out, "grad")
        need_k = ctx.needs_input_grad[2]
        if g == 0 or n == 0:
            return None, torch.zeros_like(z) if ctx.needs_input_grad[1] else None, torch.zeros_like(kinv) if need_k else None
        g_z = torch.empty_like(z) if ctx.needs_input_grad[1] else None
        acc = torch.empty((g, 9), dtype=torch.float64, device=z.device) if need_k else None
        g_k = None
        with _guard(z.device):
            st = stream_for(z)
            for s, e in _group_slices(g):
                call("fm_unproject_bwd", ptr(xy if ctx.shared else _rows(xy, s, e)), 0 if ctx.shared else n * 2, ptr(_rows(z, s, e)),
                     ptr(_rows(kinv, s, e)), ptr(_rows(g_out, s, e)), e - s, n, ptr(_rows(g_z, s, e)), ptr(_rows(acc, s, e)), st)
            if need_k:
                g_k = torch.empty_like(kinv)
                call("fm_intrinsics_inverse_bwd", ptr(acc), ptr(kinv), g, ptr(g_k), 0, st)
        return None, g_z, g_k


class Reproject(torch.autograd.Function):
    """reproject_points (flowmap/model/projection.py:116-134): xyz (G,N,3), T (G,4,4),
    K (G,3,3) -> xy (G,N,2)."""

    @staticmethod
    def forward(ctx, xyz, t, k):
        dev = check_device(xyz, t, k)
        xyz, t, k = _f32c(xyz, "points"), _f32c(t, "transformations"), _f32c(k, "intrinsics")
        g, n, _ = xyz.shape
        out = torch.empty((g, n, 2), dtype=torch.float32, device=dev)
        with _guard(dev):
            for s, e in _group_slices(g if n else 0):  # (an empty point set: nothing to launch)
                call("fm_reproject_fwd", ptr(_rows(xyz, s, e)), ptr(_rows(t, s, e)), ptr(_rows(k, s, e)), e - s, n, ptr(_rows(out, s, e)),
                     stream_for(xyz))
        ctx.save_for_backward(xyz, t, k)
        return out

    @staticmethod
    def backward(ctx, g_xy):
        xyz, t, k = ctx.saved_tensors
        g, n, _ = xyz.shape
        g_xy = _pairs(g_xy, "grad")
        need_xyz, need_t, need_k = ctx.needs_input_grad[:3]
        if g == 0 or n == 0:
            return (torch.zeros_like(xyz) if need_xyz else None, torch.zeros_like(t) if need_t else None, torch.zeros_like(k) if need_k else None)
        g_xyz = torch.empty_like(xyz) if need_xyz else None
        g_t = torch.empty_like(t) if need_t else None
        g_k = torch.empty_like(k) if need_k else None
        acc = torch.empty((min(g, MAX_GROUPS), 18), dtype=torch.float64, device=xyz.device)
        with _guard(xyz.device):
            for s, e in _group_slices(g):
                call("fm_reproject_bwd", ptr(_rows(xyz, s, e)), ptr(_rows(t, s, e)), ptr(_rows(k, s, e)), ptr(_rows(g_xy, s, e)), e - s, n,
                     ptr(_rows(g_xyz, s, e)), ptr(_rows(g_t, s, e)), ptr(_rows(g_k, s, e)), ptr(acc), stream_for(xyz))
        return g_xyz, g_t, g_k


class BilinearSample(torch.autograd.Function):
    """F.grid_sample(bilinear, border, align_corners=False) of a channels-last image
    (G,H,W,C) at normalised coordinates (G,P,2) in (0,1) -> (G,P,C)
    (flowmap/model/projection.py:235-241,266-272)."""

    @staticmethod
    def forward(ctx, img, xy):
        dev = check_device(img, xy)
        if xy.requires_grad:
            raise RuntimeError("flowmap_amd: gradients w.r.t. sampling coordinates are not supported")
        img, xy = _f32c(img, "image"), _pairs(xy, "coordinates")
        g, h, w, c = img.shape
        p = xy.shape[1]
        out = torch.empty((g, p, c), dtype=torch.float32, device=dev)
        with _guard(dev):
            for s, e in _group_slices(g if p and c else 0):  # (an empty point set: nothing to launch)
                call("fm_bilinear_sample_fwd", ptr(_rows(img, s, e)), ptr(_rows(xy, s, e)), e - s, h, w, c, p, ptr(_rows(out, s, e)), stream_for(img))
        ctx.save_for_backward(xy)
        ctx.dims = (g, h, w, c, p)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (xy,) = ctx.saved_tensors
        g, h, w, c, p = ctx.dims
        g_out = _f32c(g_out, "grad")
        g_img = torch.zeros((g, h, w, c), dtype=torch.float32, device=xy.device)
        with _guard(xy.device):
            for s, e in _group_slices(g if p and g_img.numel() else 0):
                call("fm_bilinear_sample_bwd", ptr(_rows(g_out, s, e)), ptr(_rows(xy, s, e)), e - s, h, w, c, p, ptr(_rows(g_img, s, e)), stream_for(xy))
        return g_img, None


class RobustMapping(torch.autograd.Function):
    """Mapping.forward (flowmap/loss/mapping/mapping.py:35-43) on (n,2) pairs."""

    @staticmethod
    def forward(ctx, a, b, kind, delta, ax, ay):
        dev = check_device(a, b)
        a, b = _pairs(a, "a"), _pairs(b, "b")
        n = a.shape[0]
        out = torch.empty((n,), dtype=torch.float32, device=dev)
        if n:  # (an empty tensor has no pointer to hand over)
            with _guard(dev):
                call("fm_mapping_fwd", ptr(a), ptr(b), n, kind, float(delta), float(ax), float(ay), ptr(out), stream_for(a))
        ctx.save_for_backward(a, b)
        ctx.cfg = (kind, float(delta), float(ax), float(ay))
        return out

    @staticmethod
    def backward(ctx, g_out):
        a, b = ctx.saved_tensors
        kind, delta, ax, ay = ctx.cfg
        g_out = _f32c(g_out, "grad")
        g_a = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        g_b = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if a.shape[0]:
            with _guard(a.device):
                call("fm_mapping_bwd", ptr(a), ptr(b), ptr(g_out), a.shape[0], kind, delta, ax, ay, ptr(g_a), ptr(g_b), stream_for(a))
        return g_a, g_b, None, None, None, None


class AlignRigid(torch.autograd.Function):
    """align_rigid (flowmap/model/procrustes.py:7-51): p, q (G,P,3), w (G,P) -> (G,4,4)."""

    @staticmethod
    def forward(ctx, p, q, w):
        dev = check_device(p, q, w)
        p, q, w = _f32c(p, "p"), _f32c(q, "q"), _f32c(w, "weights")
        g, n, _ = p.shape
        if g == 0 or n == 0:
            raise RuntimeError(f"flowmap_amd: align_rigid needs at least one group of at least one point (got {g} groups of {n} points): "
                               "an empty point set has no rigid fit")
        stats = torch.empty((g, STAT_STRIDE), dtype=torch.float64, device=dev)
        t = torch.empty((g, 4, 4), dtype=torch.float32, device=dev)
        aux = torch.empty((g, AUX_STRIDE), dtype=torch.float64, device=dev)
        with _guard(dev):
            st = stream_for(p)
            for s, e in _group_slices(g):
                call("fm_align_rigid_stats", ptr(_rows(p, s, e)), ptr(_rows(q, s, e)), ptr(_rows(w, s, e)), e - s, n, ptr(_rows(stats, s, e)), st)
            call("fm_pose_solve", ptr(stats), g, ptr(t), None, ptr(aux), st)
        ctx.save_for_backward(p, q, w, t, aux)
        return t

    @staticmethod
    def backward(ctx, g_t):
        p, q, w, t, aux = ctx.saved_tensors
        g, n, _ = p.shape
        g_t = _f32c(g_t, "grad")
        pair_grad = torch.empty((g, PAIR_GRAD_STRIDE), dtype=torch.float64, device=p.device)
        g_p = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        g_q = torch.empty_like(q) if ctx.needs_input_grad[1] else None
        g_w = torch.empty_like(w) if ctx.needs_input_grad[2] else None
        with _guard(p.device):
            st = stream_for(p)
            call("fm_pose_solve_bwd", ptr(g_t), None, ptr(t), ptr(aux), g, ptr(pair_grad), None, 0, st)
            for s, e in _group_slices(g):
                call("fm_align_rigid_bwd", ptr(_rows(p, s, e)), ptr(_rows(q, s, e)), ptr(_rows(w, s, e)), e - s, n, ptr(_rows(aux, s, e)),
                     ptr(_rows(pair_grad, s, e)), ptr(_rows(g_p, s, e)), ptr(_rows(g_q, s, e)), ptr(_rows(g_w, s, e)), st)
        return g_p, g_q, g_w
