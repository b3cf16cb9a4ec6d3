"""Drop-in for ``flowmap.model.projection`` (flowmap/model/projection.py) backed by the
HIP kernels in libflowmap_hip.so.

Same public names, positional order, shapes and gradient behaviour as the reference;
every function cites the reference lines it stands in for.  Differences, all opt-in or
invisible to results:

* ``unproject`` may return a :class:`LazySurfaces` (see ``set_lazy_surfaces``): a view
  of (depth, intrinsics) that the fused consumers in this package read directly, so the
  1.66 GB (B,F,H,W,3) tensor of config C1 never touches HBM.  Anything else that
  touches it (torch functions, attribute access, indexing beyond frame slices)
  materialises the real tensor on the spot.
* tensors must be fp32 and live on the GPU; there is no CPU path (RuntimeError).
* flows / track coordinates are constants: gradients w.r.t. them are not implemented.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _ops
from .._base import parse_window
from .._lib import check_device, using_test_double
from ..types import AlignmentResiduals, DepthConsistency, FocalSweep, RenderedViews

# --------------------------------------------------------------------------------------
# small tensor helpers (no kernels needed: pure indexing / concatenation)
# --------------------------------------------------------------------------------------


def homogenize_points(points: Tensor) -> Tensor:
    """flowmap/model/projection.py:11-15"""
    return torch.cat([points, torch.ones_like(points[..., :1])], dim=-1)


def homogenize_vectors(vectors: Tensor) -> Tensor:
    """flowmap/model/projection.py:18-22"""
    return torch.cat([vectors, torch.zeros_like(vectors[..., :1])], dim=-1)


earlier = lambda x: x[:, :-1]  # noqa: E731   flowmap/model/projection.py:139
later = lambda x: x[:, 1:]  # noqa: E731     flowmap/model/projection.py:140

_grid_cache: dict = {}


def sample_image_grid(shape: Tuple[int, ...], device: torch.device = torch.device("cpu")):
    """flowmap/model/projection.py:93-113.  Returns (xy float grid, ij int64 indices).

    The grid is a constant of (shape, device); it is built once with the reference's
    arithmetic ((int64 + 0.5) / length in fp32) and cached — the reference rebuilds it
    three times per step.  The fused kernels never read it (they derive coordinates from
    the thread index); it exists for API parity and as the identity token that lets
    ``unproject`` recognise the canonical grid.
    """
    device = torch.device(device)
    key = (tuple(int(s) for s in shape), str(device))
    hit = _grid_cache.get(key)
    if hit is not None:
        return hit
    # Built on the host and copied once: torch's GPU division differs from the CPU's by an
    # ulp on some pixel centres, and the kernels (which derive coordinates from the thread
    # index with an IEEE divide) follow the CPU values the oracle and golden vectors use.
    indices = [torch.arange(length) for length in shape]
    stacked = torch.stack(torch.meshgrid(*indices, indexing="ij"), dim=-1).to(device)
    coords = [(idx + 0.5) / length for idx, length in zip(indices, shape)]
    coords = list(reversed(coords))
    xy = torch.stack(torch.meshgrid(*coords, indexing="xy"), dim=-1).to(device)
    if len(_grid_cache) > 16:
        _grid_cache.clear()
    _grid_cache[key] = (xy, stacked)
    return xy, stacked


# --------------------------------------------------------------------------------------
# lazy surfaces
# --------------------------------------------------------------------------------------

_LAZY = False


def set_lazy_surfaces(enabled: bool) -> None:
    """When enabled, ``unproject(canonical grid, depths (b,f,h,w), K (b,f,1,1,3,3))``
    returns a LazySurfaces instead of writing (b,f,h,w,3) floats to HBM."""
    global _LAZY
    _LAZY = bool(enabled)


def lazy_surfaces_enabled() -> bool:
    return _LAZY


class _LazyValue:
    """What the values that are not stored (LazySurfaces, LazyWeights, LazyExtrinsics) share — the tensor protocol, stated once.

    A subclass names its source tensor in ``_fm_lazy`` (``device`` and ``dtype`` are that tensor's, and flowmap_amd/_reference.py asks a
    lazy value for its device through this attribute, without evaluating it), gives its ``shape`` and says in ``_evaluate`` how the value
    is computed.  Metadata never evaluates.  Any other use — an attribute, an index, a torch function — behaves like the real tensor:
    ``materialize()`` evaluates once (autograd intact) and keeps the result in ``_dense``.  ``peek()`` is the read-only door."""

    _fm_lazy = ""
    _dense: Optional[Tensor] = None

    # -- cheap metadata ---------------------------------------------------------------
    @property
    def device(self):
        return self.__dict__[self._fm_lazy].device

    @property
    def dtype(self):
        return self.__dict__[self._fm_lazy].dtype

    @property
    def ndim(self):
        return len(self.shape)

    def dim(self):
        return len(self.shape)

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    # -- the value --------------------------------------------------------------------
    def _evaluate(self, detached: bool) -> Tensor:
        """The value from the sources; ``detached``: from the detached sources, and without any side effect."""
        raise NotImplementedError

    def materialize(self) -> Tensor:
        if self._dense is None:
            self._dense = self._evaluate(False)
        return self._dense

    def peek(self) -> Tensor:
        """The value for this call only, detached: the evaluated one if there is one, otherwise computed from the detached sources —
        nothing is kept on this object and no note is left on any tensor.  What the diagnostics that "only read" use."""
        return (self._dense if self._dense is not None else self._evaluate(True)).detach()

    @staticmethod
    def _frame_slice(item) -> bool:
        """``[:, s:e]``: the index that LazySurfaces and LazyWeights answer without evaluating."""
        return isinstance(item, tuple) and len(item) == 2 and isinstance(item[0], slice) and item[0] == slice(None) and isinstance(item[1], slice)

    def __getitem__(self, item):
        return self.materialize()[item]

    def __getattr__(self, name):
        # anything we did not anticipate: behave like the real tensor
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        conv = lambda a: a.materialize() if isinstance(a, _LazyValue) else a  # noqa: E731  (top-level arguments only)
        return func(*(conv(a) for a in args), **{k: conv(v) for k, v in (kwargs or {}).items()})


class LazySurfaces(_LazyValue):
    """Camera-space surfaces defined by (depths, intrinsics) but not stored.

    Quacks like the (b, f, h, w, 3) tensor for what the hot path's callers read
    (``shape``, ``device``, ``dtype``, ``ndim``, frame slicing ``[:, s:e]``); any other
    use transparently materialises the real tensor (with autograd intact).
    """

    _fm_lazy = "depths"

    def __init__(self, depths: Tensor, intrinsics: Tensor):
        self.depths = depths  # (b, f, h, w)
        self.intrinsics = intrinsics  # (b, f, 3, 3)

    @property
    def shape(self):
        return torch.Size((*self.depths.shape, 3))

    def _evaluate(self, detached: bool) -> Tensor:
        depths, intrinsics = (self.depths.detach(), self.intrinsics.detach()) if detached else (self.depths, self.intrinsics)
        b, f, h, w = depths.shape
        xy, _ = sample_image_grid((h, w), depths.device)
        return _unproject_dense(xy, depths, intrinsics.reshape(b, f, 1, 1, 3, 3))

    def __getitem__(self, item):
        # frame slices keep laziness: surfaces[:, s:e]  (loss_tracking.py:48-49)
        if self._frame_slice(item):
            return LazySurfaces(self.depths[item], self.intrinsics[item])
        return self.materialize()[item]

    def __repr__(self):
        return f"LazySurfaces(shape={tuple(self.shape)}, device={self.device})"


def _dense(surfaces) -> Tensor:
    return surfaces.materialize() if isinstance(surfaces, LazySurfaces) else surfaces


class LazyWeights(_LazyValue):
    """Correspondence weights sigmoid(sensitivity · logits) (BackboneExplicitDepth,
    flowmap/model/backbone/backbone_explicit_depth.py:38-41) that are not stored: only
    the P sampled pixels per pair are ever read (0.1 % at 720p with P = 1000), so
    ``align_surfaces`` applies the sigmoid inside its gather and writes the logit gradient
    directly.  Any other use materialises the real (b, f-1, h, w) tensor."""

    _fm_lazy = "logits"

    def __init__(self, logits: Tensor, sensitivity: float, lazy_slices: bool = True):
        self.logits = logits  # (b, f-1, h, w)
        self.sensitivity = float(sensitivity)
        # frame slices stay lazy only for consumers that understand a LazyWeights (this package's IntrinsicsSoftmin / align_surfaces); the
        # reference's own IntrinsicsSoftmin hands `weights[:, :1]` to einops (intrinsics_softmin.py:120), which needs a real tensor
        self.lazy_slices = bool(lazy_slices)

    @property
    def shape(self):
        return self.logits.shape

    def _evaluate(self, detached: bool) -> Tensor:
        return (self.sensitivity * (self.logits.detach() if detached else self.logits)).sigmoid()

    def kernel_input(self, keep: bool = False):
        """(the tensor the kernels read, sensitivity): the logits, which the kernels put through the sigmoid themselves, when the
        sensitivity is not 0; at sensitivity 0, which the kernels read as "these are the weights", the value — ``peek()`` for the callers
        that only read, ``materialize()`` (differentiable, kept) with ``keep``, for a training step."""
        if self.sensitivity != 0.0:
            return self.logits, self.sensitivity
        return (self.materialize() if keep else self.peek()), 0.0

    def __getitem__(self, item):
        # frame slices keep laziness: weights[:, :1]  (intrinsics_softmin.py:100,120 read the first pair only)
        if self._frame_slice(item):
            if self.lazy_slices:
                return LazyWeights(self.logits[item], self.sensitivity)
            if self._dense is None:  # the sigmoid of the frames asked for, not of the whole (b, f-1, h, w) tensor
                return (self.sensitivity * self.logits[item]).sigmoid()
        return self.materialize()[item]

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if func in (torch.ones_like, torch.zeros_like, torch.empty_like) and args and isinstance(args[0], LazyWeights):
            # model/model.py:67-68 (`use_correspondence_weights: false`) asks for the shape only: no sigmoid over (f-1, h, w) for that
            return func(args[0].logits.detach(), *args[1:], **(kwargs or {}))
        return super().__torch_function__(func, types, args, kwargs)

    def __repr__(self):
        return f"LazyWeights(shape={tuple(self.shape)}, sensitivity={self.sensitivity})"


class LazyExtrinsics(_LazyValue):
    """The camera-to-world chain of ``get_extrinsics`` (flowmap/model/projection.py:187-210) over the fit's relative poses, NOT evaluated yet.

    ``align_surfaces`` returns one while gradients are being recorded (a training step) and nothing has asked for the chain in an earlier
    step: the fused flow loss reads the relative poses (``_fm_relative_poses``), so a flow-only step never chains them — in the fit's launch
    that is the LAST block's one wave working for ~7 us at 149 poses while the rest of the GPU waits (``profiles/r06_fit_microbench.jsonl``).
    Anything else — an attribute, an index, a torch function, this package's tracking loss — evaluates the chain (one launch,
    ``fm_pose_chain_fwd``, differentiable through the fit's poses) and notes on the constant flow tensor that the chain is wanted: from the
    next step on the fit's own launch produces it again, as in rounds 1-5.  The diagnostics that only read take ``peek()``, which does
    neither.  Under ``torch.no_grad()`` (validation, ``Model.export``: the reference's ``ModelExports`` checks its fields) the module
    returns the tensor as before; so does the function-level ``align_surfaces``."""

    _fm_lazy = "_rel"

    def __init__(self, rel: Tensor, rel_inv: Tensor, flow_tensor: Optional[Tensor] = None):
        self._rel = rel  # (b, f-1, 4, 4): later camera -> earlier camera, the factors of the chain
        self._fm_relative_poses = (rel_inv, rel)
        self._flow_tensor = flow_tensor

    @property
    def shape(self):
        b, pairs = self._rel.shape[:2]
        return torch.Size((b, pairs + 1, 4, 4))

    def _evaluate(self, detached: bool) -> Tensor:
        if detached:
            return _ops.PoseChain.apply(self._rel.detach())
        dense = _ops.PoseChain.apply(self._rel)
        dense._fm_relative_poses = self._fm_relative_poses
        if self._flow_tensor is not None:  # something reads the chain in this optimisation: the fit's launch chains it from the next step on
            self._flow_tensor.__dict__["_fm_extrinsics_wanted"] = True
        return dense

    def __len__(self):
        return int(self._rel.shape[0])

    def __iter__(self):
        return iter(self.materialize())

    # torch.as_tensor / numpy.asarray of the value (the array protocols: a detached view of the evaluated chain)
    def __dlpack__(self, *args, **kwargs):
        return self.materialize().detach().__dlpack__(*args, **kwargs)

    def __dlpack_device__(self):
        return self._rel.__dlpack_device__()

    def __array__(self, dtype=None, copy=None):
        out = self.materialize().detach().cpu().numpy()
        return out if dtype is None else out.astype(dtype)

    # torch.save / pickle / copy.deepcopy: the VALUE travels — the evaluated chain as a plain, detached tensor
    def __reduce_ex__(self, protocol):
        return self.materialize().detach().__reduce_ex__(protocol)

    def __deepcopy__(self, memo):
        return self.materialize().detach().clone()

    def __repr__(self):
        return f"LazyExtrinsics(shape={tuple(self.shape)}, device={self.device}, evaluated={self._dense is not None})"


def _dense_extrinsics(extrinsics):
    return extrinsics.materialize() if isinstance(extrinsics, LazyExtrinsics) else extrinsics


def _peek_extrinsics(extrinsics) -> Tensor:
    """The extrinsics for this call only, detached: a tensor as it is, a LazyExtrinsics through ``peek()`` — it stays unevaluated."""
    return extrinsics.peek() if isinstance(extrinsics, _LazyValue) else extrinsics.detach()


# --------------------------------------------------------------------------------------
# unproject
# --------------------------------------------------------------------------------------


def _pad_shape(shape, nd):
    return (1,) * (nd - len(shape)) + tuple(shape)


def _split_lead(out_shape, *mat_batch_shapes):
    """Leading dims over which the small matrices vary ("groups") vs trailing dims over
    which they are constant ("points")."""
    nd = len(out_shape)
    n_lead = 0
    for i in range(nd):
        if any(_pad_shape(ms, nd)[i] != 1 for ms in mat_batch_shapes):
            n_lead = i + 1
    lead, pts = tuple(out_shape[:n_lead]), tuple(out_shape[n_lead:])
    g = 1
    for s_ in lead:
        g *= s_
    n = 1
    for s_ in pts:
        n *= s_
    return n_lead, lead, pts, g, n


def _flatten_mats(m: Tensor, nd: int, n_lead: int, lead, g: int) -> Tensor:
    r, c = m.shape[-2:]
    ms = _pad_shape(m.shape[:-2], nd)
    return m.reshape(ms[:n_lead] + (r, c)).expand(*lead, r, c).reshape(g, r, c)


def _unproject_dense(coordinates: Tensor, z: Tensor, intrinsics: Tensor) -> Tensor:
    """Materialising unproject through fm_unproject_fwd.  Handles the reference's
    broadcast patterns: coordinates (*#batch, 2), z (*#batch), intrinsics (*#batch, 3, 3)
    where the intrinsics are constant over the trailing ("grid") dims."""
    check_device(coordinates, z, intrinsics)
    out_shape = torch.broadcast_shapes(coordinates.shape[:-1], z.shape, intrinsics.shape[:-2])
    nd = len(out_shape)
    n_lead, lead, pts, g, n = _split_lead(out_shape, intrinsics.shape[:-2])
    k = _flatten_mats(intrinsics, nd, n_lead, lead, g)
    zz = z.expand(out_shape).reshape(g, n)
    cshape = _pad_shape(coordinates.shape[:-1], nd)
    if all(s_ == 1 for s_ in cshape[:n_lead]):
        xy = coordinates.reshape(cshape[n_lead:] + (2,)).expand(*pts, 2).reshape(n, 2)
    else:
        xy = coordinates.expand(*out_shape, 2).reshape(g, n, 2)
    return _ops.Unproject.apply(xy, zz, k).reshape(*out_shape, 3)


def _squeeze_intrinsics(intrinsics: Tensor) -> Tensor:
    """(b,f,1,1,3,3) -> (b,f,3,3) without leaving work for autograd: the caller's own tensor when
    the argument is ``K[:, :, None, None]`` of a contiguous (b,f,3,3) K (model/model.py:69-74 —
    gradients then reach K directly and every consumer of the step sees ONE tensor object),
    otherwise a reshape (a view; indexing ``[:, :, 0, 0]`` would cost two select_backward
    zero-fill + copy launches per step)."""
    b, f = intrinsics.shape[:2]
    base = intrinsics._base
    if (
        base is not None
        and tuple(base.shape) == (b, f, 3, 3)
        and base.is_contiguous()
        and base.data_ptr() == intrinsics.data_ptr()
        and base.requires_grad == intrinsics.requires_grad
    ):
        return base
    return intrinsics.reshape(b, f, 3, 3)


def unproject(coordinates: Tensor, z: Tensor, intrinsics: Tensor):
    """flowmap/model/projection.py:76-90: (K⁻¹·[x,y,1])·z."""
    if (
        _LAZY
        and z.dim() == 4
        and intrinsics.dim() == 6
        and tuple(intrinsics.shape[2:4]) == (1, 1)
        and tuple(intrinsics.shape[:2]) == tuple(z.shape[:2])
        and coordinates is sample_image_grid(tuple(z.shape[2:]), z.device)[0]
    ):
        check_device(z, intrinsics)
        return LazySurfaces(z, _squeeze_intrinsics(intrinsics))
    return _unproject_dense(coordinates, z, intrinsics)


def unproject_dense(coordinates: Tensor, z: Tensor, intrinsics: Tensor) -> Tensor:
    """``unproject`` that always returns a real tensor (never a LazySurfaces)."""
    return _unproject_dense(coordinates, z, intrinsics)


# --------------------------------------------------------------------------------------
# rigid transforms / projection on explicit points
# --------------------------------------------------------------------------------------


def _group_points(points: Tensor, *mats: Tensor):
    """Broadcast points (*batch, d) against matrices (*batch, r, c) and flatten to groups:
    returns (points (G,N,d), [mats (G,r,c)], out_batch_shape)."""
    bshape = torch.broadcast_shapes(points.shape[:-1], *[m.shape[:-2] for m in mats])
    nd = len(bshape)
    n_lead, lead, pts, g, n = _split_lead(bshape, *[m.shape[:-2] for m in mats])
    p = points.expand(*bshape, points.shape[-1]).reshape(g, n, points.shape[-1])
    return p, [_flatten_mats(m, nd, n_lead, lead, g) for m in mats], bshape


def transform_rigid(homogeneous_coordinates: Tensor, transformation: Tensor) -> Tensor:
    """flowmap/model/projection.py:25-30 (tiny generic matvec; kept in torch)."""
    return (transformation @ homogeneous_coordinates.unsqueeze(-1)).squeeze(-1)


def transform_cam2world(homogeneous_coordinates: Tensor, extrinsics: Tensor) -> Tensor:
    """flowmap/model/projection.py:33-38"""
    return transform_rigid(homogeneous_coordinates, _dense_extrinsics(extrinsics))


def transform_world2cam(homogeneous_coordinates: Tensor, extrinsics: Tensor) -> Tensor:
    """flowmap/model/projection.py:41-46"""
    return transform_rigid(homogeneous_coordinates, torch.linalg.inv_ex(_dense_extrinsics(extrinsics), check_errors=False)[0])


_EYE_CACHE: dict = {}


def _eye44(device) -> Tensor:
    key = str(device)
    if key not in _EYE_CACHE:
        _EYE_CACHE[key] = torch.eye(4, dtype=torch.float32, device=device)
    return _EYE_CACHE[key]


def reproject_points(xyz: Tensor, relative_transformations: Tensor, intrinsics: Tensor) -> Tensor:
    """flowmap/model/projection.py:116-134."""
    check_device(xyz, relative_transformations, intrinsics)
    p, (t, k), bshape = _group_points(xyz, relative_transformations, intrinsics)
    return _ops.Reproject.apply(p, t, k).reshape(*bshape, 2)


def project_camera_space(points: Tensor, intrinsics: Tensor, epsilon: float = 1e-5, infinity: float = 1e8) -> Tensor:
    """flowmap/model/projection.py:49-58 (3-D points; the kernel fixes eps=1e-5, inf=1e8
    like every caller in the reference)."""
    if epsilon != 1e-5 or infinity != 1e8 or points.shape[-1] != 3:
        raise NotImplementedError("flowmap_amd.project_camera_space supports 3-D points with epsilon=1e-5, infinity=1e8")
    ident = _eye44(points.device)
    return reproject_points(points, ident, intrinsics)


def project(points: Tensor, extrinsics: Tensor, intrinsics: Tensor, epsilon: float = 1e-5):
    """flowmap/model/projection.py:61-73: world -> image, plus the in-front test."""
    if epsilon != 1e-5:
        raise NotImplementedError("flowmap_amd.project supports epsilon=1e-5")
    inv = torch.linalg.inv_ex(_dense_extrinsics(extrinsics), check_errors=False)[0]
    cam_z = (inv[..., 2, :3] * points).sum(-1) + inv[..., 2, 3]
    return reproject_points(points, inv, intrinsics), cam_z >= 0


# --------------------------------------------------------------------------------------
# flow-induced positions
# --------------------------------------------------------------------------------------


def _flow_positions(surfaces, extrinsics: Tensor, intrinsics: Tensor, forward: bool) -> Tensor:
    surfaces, extrinsics = _dense(surfaces), _dense_extrinsics(extrinsics)
    check_device(surfaces, extrinsics, intrinsics)
    rel_f, rel_b = _ops.RelativePoses.apply(extrinsics)
    b, f = surfaces.shape[:2]
    grid = surfaces.shape[2:-1]
    n = 1
    for s in grid:
        n *= s
    if forward:
        src, rel, k = surfaces[:, :-1], rel_f, intrinsics[:, 1:]
    else:
        src, rel, k = surfaces[:, 1:], rel_b, intrinsics[:, :-1]
    out = _ops.Reproject.apply(src.reshape(b * (f - 1), n, 3), rel.reshape(b * (f - 1), 4, 4), k.reshape(b * (f - 1), 3, 3))
    return out.reshape(b, f - 1, *grid, 2)


def compute_forward_flow(surfaces, extrinsics: Tensor, intrinsics: Tensor) -> Tensor:
    """flowmap/model/projection.py:143-162: positions of all surface points after the
    forward flow induced by the poses.  surfaces (b,f,*grid,3) -> (b,f-1,*grid,2)."""
    return _flow_positions(surfaces, extrinsics, intrinsics, True)


def compute_backward_flow(surfaces, extrinsics: Tensor, intrinsics: Tensor) -> Tensor:
    """flowmap/model/projection.py:165-184."""
    return _flow_positions(surfaces, extrinsics, intrinsics, False)


# --------------------------------------------------------------------------------------
# poses
# --------------------------------------------------------------------------------------


def get_extrinsics(inverse_relative_transformations: Tensor) -> Tensor:
    """flowmap/model/projection.py:187-210: P_0 = I, P_k = P_{k-1}·T_{k-1} — one launch
    instead of a Python loop of F-1 matmuls."""
    check_device(inverse_relative_transformations)
    return _ops.PoseChain.apply(inverse_relative_transformations)


def align_surfaces(surfaces, backward_flows: Tensor, backward_weights: Tensor, indices: Tensor) -> Tensor:
    """flowmap/model/projection.py:213-252: per-pair weighted Procrustes on flow-induced
    correspondences, chained into camera-to-world extrinsics (b,f,4,4)."""
    return _align_surfaces(surfaces, backward_flows, backward_weights, indices, lazy_ok=False)


# The front door of the diagnostics below (alignment_residuals, depth_consistency, focal_sweep): what they refuse and unwrap alike.


def _refuse_host(what: str, dev) -> None:
    if dev.type != "cuda" and not using_test_double():
        raise RuntimeError(f"flowmap_amd: {what}: tensors are on {dev}; it runs on the GPU only (device 'cuda' on ROCm) — the reference has no "
                           "function that returns this quantity, so host tensors have nowhere to go. There is no CPU fallback.")


def _check_indices(what: str, indices, dev) -> None:
    if indices is None:
        return
    if not torch.is_tensor(indices) or indices.dtype != torch.int64:
        raise RuntimeError(f"flowmap_amd: {what}: indices must be an int64 tensor (got {getattr(indices, 'dtype', type(indices).__name__)})")
    if indices.device != dev:
        raise RuntimeError(f"flowmap_amd: {what}: indices are on {indices.device}, the depths on {dev}")
    if indices.dim() != 1 or indices.numel() == 0:
        raise RuntimeError(f"flowmap_amd: {what}: indices must be a non-empty 1-D tensor (got shape {tuple(indices.shape)})")


def _check_posed_depths(what: str, depths, intrinsics, extrinsics, colors=None) -> Tensor:
    """The shapes depth_consistency and render_views ask of ``depths`` (b, f, h, w), ``intrinsics`` (b, f, 3, 3), ``extrinsics`` (b, f, 4, 4)
    — a tensor or a LazyExtrinsics — and ``colors`` (b, f, 3, h, w) or None.  -> the tensor that stands for the extrinsics where a dtype
    or a device is asked (a LazyExtrinsics' relative poses: it is not evaluated)."""
    pose_tensor = extrinsics._rel if isinstance(extrinsics, LazyExtrinsics) else extrinsics
    if not torch.is_tensor(depths) or not torch.is_tensor(intrinsics) or not torch.is_tensor(pose_tensor):
        raise RuntimeError(f"flowmap_amd: {what}: depths and intrinsics must be tensors, extrinsics a tensor or a LazyExtrinsics")
    if depths.dim() != 4:
        raise RuntimeError(f"flowmap_amd: {what}: depths of shape {tuple(depths.shape)}; expected (batch, frame, height, width)")
    b, f, h, w = depths.shape
    if tuple(intrinsics.shape) != (b, f, 3, 3):
        raise RuntimeError(f"flowmap_amd: {what}: intrinsics of shape {tuple(intrinsics.shape)} do not match the depths {(b, f, h, w)}: expected {(b, f, 3, 3)}")
    if tuple(extrinsics.shape) != (b, f, 4, 4):
        raise RuntimeError(f"flowmap_amd: {what}: extrinsics of shape {tuple(extrinsics.shape)} do not match the depths {(b, f, h, w)}: expected {(b, f, 4, 4)}")
    if colors is not None and (not torch.is_tensor(colors) or tuple(colors.shape) != (b, f, 3, h, w)):
        raise RuntimeError(f"flowmap_amd: {what}: colors of shape {tuple(getattr(colors, 'shape', ()))} do not match the depths {(b, f, h, w)}: "
                           f"expected {(b, f, 3, h, w)}")
    return pose_tensor


def _check_float32(what: str, named) -> None:
    for name, value in named:
        if value.dtype != torch.float32:
            raise RuntimeError(f"flowmap_amd: {what}: {name} must be float32 (got {value.dtype})")


def _peek_weights(weights):
    """(what the kernel reads, sensitivity) of a weights argument WITHOUT evaluating a LazyWeights (``LazyWeights.kernel_input``); a
    tensor (or None) as it is, with sensitivity 0."""
    return weights.kernel_input() if isinstance(weights, LazyWeights) else (weights, 0.0)


def alignment_residuals(surfaces, backward_flows: Tensor, backward_weights, extrinsics, indices: Optional[Tensor] = None, pairs=None,
                        offsets: bool = False, weights: bool = False, sums: bool = True) -> AlignmentResiduals:
    """The terms of the objective ``align_surfaces`` minimises per pair (flowmap/model/projection.py:213-252 -> align_rigid,
    flowmap/model/procrustes.py:7-51): for pair i and element j, with p_j = surfaces[:, i+1] at pixel idx_j, q_j the bilinear,
    border-clamped sample of surfaces[:, i] at xy[idx_j] + backward_flows[:, i, idx_j], w_j = backward_weights[:, i, idx_j] and
    T_i = E_i⁻¹·E_{i+1} of ``extrinsics`` (the matrix align_rigid returned when the extrinsics come from the fit):
    ``offset`` = T_i·[p_j; 1] − q_j, ``residual`` = ‖offset‖² before the weight, ``pair_sum`` = Σ_j w_j·residual_j and
    ``pair_weight`` = Σ_j w_j in float64.  ``indices`` None: every pixel, maps (b, count, h, w); an int64 tensor of length P (repeats
    and P > h·w allowed): maps (b, count, P) — the fit's own correspondences when it is the fit's selection
    (extrinsics_procrustes.procrustes_indices).  ``pairs``: None, a slice with step 1, or (first, count).

    ONE launch (fm_alignment_residuals, plus the small ordered second stage of the sums) that walks the fit's own per-correspondence
    function over the elements: depth-sourced on a LazySurfaces, surface-sourced on an explicit (b, f, h, w, 3) tensor; nothing of the
    surfaces' size is formed.  ``backward_weights``: a tensor as it is, a LazyWeights through its logits (the kernel applies the
    sigmoid), None = weight 1.  Never differentiable, and it only reads: no note on any tensor, no LazyExtrinsics / LazyWeights
    evaluated, no optimiser or tap state.  Host tensors are refused — the reference has no function that returns this quantity, so
    there is nothing to hand them to, with or without install()."""
    with torch.no_grad():
        lazy = isinstance(surfaces, LazySurfaces)
        src = surfaces.depths if lazy else surfaces
        if not torch.is_tensor(src) or not torch.is_tensor(backward_flows):
            raise RuntimeError("flowmap_amd: alignment_residuals: surfaces must be a LazySurfaces or a tensor, backward_flows a tensor")
        dev = src.device
        _refuse_host("alignment_residuals", dev)
        if (lazy and src.dim() != 4) or (not lazy and (src.dim() != 5 or src.shape[-1] != 3)):
            raise RuntimeError(f"flowmap_amd: alignment_residuals: surfaces of shape {tuple(surfaces.shape)}; expected (batch, frame, height, width, 3)")
        b, f, h, w = src.shape[:4]
        if tuple(backward_flows.shape) != (b, f - 1, h, w, 2):
            raise RuntimeError(f"flowmap_amd: alignment_residuals: backward_flows of shape {tuple(backward_flows.shape)} do not match the depths "
                               f"{(b, f, h, w)}: expected {(b, f - 1, h, w, 2)}")
        if backward_weights is not None and tuple(backward_weights.shape) != (b, f - 1, h, w):
            raise RuntimeError(f"flowmap_amd: alignment_residuals: backward_weights of shape {tuple(backward_weights.shape)} do not match the depths "
                               f"{(b, f, h, w)}: expected {(b, f - 1, h, w)}")
        if tuple(extrinsics.shape) != (b, f, 4, 4):
            raise RuntimeError(f"flowmap_amd: alignment_residuals: extrinsics of shape {tuple(extrinsics.shape)} do not match the depths {(b, f, h, w)} "
                               f"(a depth tensor that holds fewer frames than the poses — a frame shard — is not supported): expected {(b, f, 4, 4)}")
        _check_indices("alignment_residuals", indices, dev)
        first, count = parse_window(pairs, f - 1, "alignment_residuals", "pairs")

        # T_i = E_i⁻¹·E_{i+1}: the second of the pair the fit leaves on its extrinsics (rel_inv, rel) and of fm_relative_pose_fwd's outputs
        direct = getattr(extrinsics, "_fm_relative_poses", None)
        if direct is not None and tuple(direct[1].shape) == (b, f - 1, 4, 4):
            rel = direct[1].detach()
        else:
            rel = _ops.RelativePoses.apply(_peek_extrinsics(extrinsics))[1]  # (a LazyExtrinsics: the chain for this call only)

        backward_weights, sens = _peek_weights(backward_weights)
        if backward_weights is not None:
            backward_weights = backward_weights.detach()
        if lazy:
            out = _ops.alignment_residuals(src.detach(), _ops.intrinsics_inverse_peek(surfaces.intrinsics), None, backward_flows, backward_weights, sens, rel,
                                           indices, first, count, offsets, weights, sums)
        else:
            out = _ops.alignment_residuals(None, None, src.detach(), backward_flows, backward_weights, sens, rel, indices, first, count, offsets, weights, sums)
        return AlignmentResiduals(*out, first)


def _check_offsets(offsets, frames: int, what: str = "depth_consistency") -> tuple:
    is_int = lambda x: isinstance(x, int) and not isinstance(x, bool)  # noqa: E731
    if not isinstance(offsets, (tuple, list)) or not all(is_int(d) for d in offsets):
        raise ValueError(f"flowmap_amd: {what}: offsets must be a tuple or list of ints, got {offsets!r}")
    offsets = tuple(int(d) for d in offsets)
    if not 1 <= len(offsets) <= 8:
        raise ValueError(f"flowmap_amd: {what}: between 1 and 8 offsets per call (got {len(offsets)})")
    if 0 in offsets or len(set(offsets)) != len(offsets):
        raise ValueError(f"flowmap_amd: {what}: offsets must be distinct and non-zero, got {offsets}")
    if any(abs(d) > frames - 1 for d in offsets):
        raise ValueError(f"flowmap_amd: {what}: offsets {offsets} reach past the {frames} frames of the video (|d| <= {frames - 1})")
    return offsets


def _consistency_on_host(ref, depths, intrinsics, extrinsics, offsets, first, count, tolerance, details, sums) -> DepthConsistency:
    """Host tensors after install(): the same composition from the reference's own functions (``ref``: name -> original)."""
    b, f, h, w = depths.shape
    xy, _ = ref("sample_image_grid")((h, w), depths.device)
    maps = (b, count, len(offsets), h, w)
    error, code = torch.zeros(maps, dtype=torch.float32), torch.ones(maps, dtype=torch.uint8)
    uv_out, qz_out, zs_out = (torch.zeros((*maps, 2)), torch.zeros(maps), torch.zeros(maps)) if details else (None, None, None)
    for o, d in enumerate(offsets):
        rows = [lf for lf in range(count) if 0 <= first + lf + d < f]
        if not rows:
            continue
        src = [first + lf for lf in rows]
        dst = [i + d for i in src]
        points = ref("unproject")(xy, depths[:, src], intrinsics[:, src][:, :, None, None])
        rel = extrinsics[:, dst].inverse() @ extrinsics[:, src]
        q = ref("transform_rigid")(ref("homogenize_points")(points), rel[:, :, None, None])[..., :3]
        uv = ref("project_camera_space")(q, intrinsics[:, dst][:, :, None, None])
        n = len(rows)
        zs = torch.nn.functional.grid_sample(depths[:, dst].reshape(b * n, 1, h, w), (uv * 2 - 1).reshape(b * n, h, w, 2), mode="bilinear",
                                             padding_mode="border", align_corners=False).reshape(b, n, h, w)
        qz = q[..., 2]
        inside = (uv >= 0).all(dim=-1) & (uv < 1).all(dim=-1)
        c = torch.where(~(qz > 0), 2, torch.where(inside, 0, 3)).to(torch.uint8)
        code[:, rows, o] = c
        error[:, rows, o] = torch.where(c == 0, (zs - qz) / qz, torch.zeros_like(qz))
        if details:
            uv_out[:, rows, o], qz_out[:, rows, o], zs_out[:, rows, o] = uv, qz, zs
    ok = code == 0
    support = None if tolerance is None else (ok & (error.abs() <= tolerance)).sum(dim=2).to(torch.uint8)
    frame_sum = torch.where(ok, error.abs(), torch.zeros_like(error)).to(torch.float64).sum(dim=(3, 4)) if sums else None
    frame_valid = ok.to(torch.float64).sum(dim=(3, 4)) if sums else None
    return DepthConsistency(error, code, uv_out, qz_out, zs_out, support, frame_sum, frame_valid, first, offsets)


def depth_consistency(depths: Tensor, intrinsics: Tensor, extrinsics, offsets=(-1, 1), frames=None, tolerance: Optional[float] = None,
                      details: bool = False, sums: bool = True) -> DepthConsistency:
    """Do the depth maps agree with each other under the chained camera poses, a few frames apart?  For a source frame i of ``frames``, an
    offset d of ``offsets``, the target frame j = i + d and the pixel with centre xy (``sample_image_grid``):

      p = unproject(xy, depth_i, K_i) (flowmap/model/projection.py:76-90);  q = (E_j⁻¹·E_i)·[p; 1], xyz — the relative transformation
      ``compute_forward_flow`` / ``compute_track_flow`` form (projection.py:154, :288), at distance d instead of 1;
      uv = project_camera_space(q, K_j) (projection.py:49-58, its ε = 1e-5 and ±1e8 / NaN clamp);
      ẑ = grid_sample(depth_j, uv·2−1, bilinear, padding_mode="border", align_corners=False) (projection.py:235-241, :266-272);
      ``code`` = the first that applies of 1: j outside [0, F); 2: not q.z > 0; 3: not 0 <= uv < 1 in both coordinates
      (projection.py:294-295); 0 otherwise;  ``error`` = (ẑ − q.z) / q.z where code == 0, else exactly 0 — negative: frame j's surface
      is nearer than the point (occluded there, or inconsistent); positive: the point floats in front of j's surface.

    ``depths`` (b, F, h, w); ``intrinsics`` (b, F, 3, 3); ``extrinsics`` (b, F, 4, 4) camera-to-world, or a LazyExtrinsics (its chain is
    formed for this call only).  ``offsets``: 1 to 8 distinct non-zero ints with |d| <= F − 1, in the order of the outputs.  ``frames``:
    None, a slice with step 1 or (first, count) over the F frames; targets outside the window but inside the video are read.
    ``tolerance`` (None or >= 0): with it ``support`` (b, count, h, w) uint8, the number of offsets with code == 0 and
    |error| <= tolerance.  ``details``: ``positions`` (uv), ``reprojected`` (q.z) and ``sampled`` (ẑ).  ``sums``: ``frame_sum`` = Σ|error|
    over code == 0 and ``frame_valid`` = their count per (frame, offset), float64.  -> DepthConsistency; maps are (b, count, n_off, h, w).

    ONE pass over depth (fm_depth_consistency), a small launch before it for the window's relative poses and the ordered second stage of
    the sums after it: no (…, h, w, 3) surfaces and no F×F poses exist.  Never differentiable, and it only reads: nothing is cached or
    noted on any tensor, no LazyExtrinsics is left evaluated, no look-ahead, tap image or optimiser state moves.  Host tensors after
    install() go to the same composition of the reference's own functions; without install() they are refused."""
    with torch.no_grad():
        pose_tensor = _check_posed_depths("depth_consistency", depths, intrinsics, extrinsics)
        b, f, h, w = depths.shape
        _check_float32("depth_consistency", (("depths", depths), ("intrinsics", intrinsics), ("extrinsics", pose_tensor)))
        if f < 2:
            raise ValueError("flowmap_amd: depth_consistency: a video of one frame has no other frame to compare with")
        offsets = _check_offsets(offsets, f)
        first, count = parse_window(frames, f, "depth_consistency", "frames")
        if tolerance is not None and not float(tolerance) >= 0.0:
            raise ValueError(f"flowmap_amd: depth_consistency: tolerance must be None or >= 0 (got {tolerance!r})")
        if b * count > 65535:
            raise ValueError(f"flowmap_amd: depth_consistency: batch x frames = {b * count} exceeds the 65 535 (batch entry, frame) rows of one call: "
                             "ask for a window of frames")
        dev = depths.device
        from .. import _reference

        if _reference.twins and _reference.on_host(depths):  # host tensors after install(): the reference's own functions
            _reference.counters["host_calls"] += 1
            ext = _dense_extrinsics(extrinsics).detach()  # (a LazyExtrinsics of host tensors is the reference's own)
            return _consistency_on_host(_reference.twins.__getitem__, depths.detach(), intrinsics.detach(), ext, offsets, first, count,
                                        None if tolerance is None else float(tolerance), details, sums)
        _refuse_host("depth_consistency", dev)
        check_device(depths, intrinsics, pose_tensor)
        ext = _peek_extrinsics(extrinsics)  # (a LazyExtrinsics: the chain for this call only, nothing kept on it or noted on the flow tensor)
        k = intrinsics.detach()
        out = _ops.depth_consistency(depths.detach(), k, _ops.intrinsics_inverse_peek(k), ext, offsets, first, count, tolerance, details, sums)
        return DepthConsistency(*out, first, offsets)


def _render_on_host(ref, depths, intrinsics, extrinsics, colors, view_k, view_ext, pairs, shape, radius, near, background):
    """Host tensors after install(): the same composition from the reference's own functions (``ref``: name -> original), an int64 key
    per candidate and scatter_reduce_(amin) -> (color, depth, source)."""
    b, f, h, w = depths.shape
    oh, ow = shape
    v = view_k.shape[1]
    xy, _ = ref("sample_image_grid")((h, w), depths.device)
    hole = torch.iinfo(torch.int64).max
    zbuf = torch.full((b, v, oh * ow), hole, dtype=torch.int64)
    index = torch.arange(h * w, dtype=torch.int64)
    for view, src in pairs:
        points = ref("unproject")(xy, depths[:, src], intrinsics[:, src][:, None, None])
        rel = (view_ext[:, view].double().inverse() @ extrinsics[:, src].double()).float()
        q = ref("transform_rigid")(ref("homogenize_points")(points), rel[:, None, None])[..., :3]
        uv = ref("project_camera_space")(q, view_k[:, view][:, None, None])
        qz = q[..., 2].contiguous()
        live = ((qz > near) & (uv >= 0).all(dim=-1) & (uv < 1).all(dim=-1)).reshape(b, h * w)
        tx = torch.floor(uv[..., 0] * ow).clamp(0, ow - 1).long().reshape(b, h * w)
        ty = torch.floor(uv[..., 1] * oh).clamp(0, oh - 1).long().reshape(b, h * w)
        key = (qz.view(torch.int32).long().reshape(b, h * w) << 32) | (src * h * w + index)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                x, y = tx + dx, ty + dy
                ok = live & (x >= 0) & (x < ow) & (y >= 0) & (y < oh)
                at = torch.where(ok, y * ow + x, torch.zeros_like(x))
                zbuf[:, view].scatter_reduce_(1, at, torch.where(ok, key, torch.full_like(key, hole)), "amin")
    holes = zbuf == hole
    winner = torch.where(holes, torch.zeros_like(zbuf), zbuf & 0xFFFFFFFF)
    source = torch.where(holes, torch.full_like(zbuf, -1), winner).to(torch.int32).reshape(b, v, oh, ow)
    depth = torch.where(holes, torch.zeros_like(zbuf), zbuf >> 32).to(torch.int32).view(torch.float32).reshape(b, v, oh, ow)
    color = None
    if colors is not None:
        planes = colors.permute(0, 2, 1, 3, 4).reshape(b, 3, 1, f * h * w).expand(b, 3, v, f * h * w)
        color = torch.gather(planes, 3, winner[:, None].expand(b, 3, v, oh * ow))
        color = torch.where(holes[:, None], torch.full_like(color, background), color).permute(0, 2, 1, 3).reshape(b, v, 3, oh, ow).contiguous()
    return color, depth, source


def render_views(depths: Tensor, intrinsics: Tensor, extrinsics, colors: Optional[Tensor] = None, *, views=None, sources=None, held_out=None,
                 offsets=(-2, -1, 1, 2), shape=None, radius: int = 0, near: float = 0.0, background: float = 0.0) -> RenderedViews:
    """What does the reconstruction look like from a camera?  The depth maps of some source frames are splatted into each view with a
    z-buffer — a forward warp.  For a view v (camera K_v, E_v, output shape (oh, ow)), a source frame i of its list and the pixel of
    frame i with centre xy (``sample_image_grid``):

      p = unproject(xy, depth_i, K_i);  q = (E_v⁻¹·E_i)·[p; 1], the relative pose formed in fp64 and rounded once;
      uv = project_camera_space(q, K_v) (the reference's ε = 1e-5 and clamp);  the point is live when q.z > ``near`` and 0 <= uv < 1 in
      both coordinates;  its bin is (floor(u·ow), floor(v·oh));  with ``radius`` r in {0, 1, 2} it covers the (2r+1)² pixels around the
      bin that lie inside the image.  A target pixel keeps the candidate with the smallest q.z, among equal q.z the lower absolute source
      index i·h·w + y·w + x: the result depends on the set of candidates only and is bit-reproducible.

    ``depths`` (b, F, h, w); ``intrinsics`` (b, F, 3, 3); ``extrinsics`` (b, F, 4, 4) camera-to-world, or a LazyExtrinsics (its chain is
    formed for this call only); ``colors`` (b, F, 3, h, w) or None.  Exactly one of:

      ``views`` = (K_v (b, V, 3, 3), E_v (b, V, 4, 4)): free cameras, every one rendered from the frames ``sources`` — None (all), a
      slice with step 1 or (first, count) over the F frames;
      ``held_out`` = a slice with step 1 (``slice(None)``: every frame) or (first, count) over the F frames: view v is frame j's own K_j,
      E_j, rendered from the frames j + d, d in ``offsets`` (1 to 8 distinct non-zero ints), that exist — never from frame j itself.
      ``psnr(videos[:, window])`` of the result is the held-out score.

    ``shape`` defaults to (h, w).  A view with no source is all holes.  -> RenderedViews: ``source`` int32 (−1: hole), ``depth`` (the
    winner's q.z, 0 in a hole), ``color`` (the winner's colour bit for bit, ``background`` in a hole; None without ``colors``).

    Known limits.  A one-pixel splat leaves holes when the target grid is finer than the source's (or a surface is seen at a grazing
    angle); ``radius`` trades holes for fattened silhouettes.  Background can show through the gaps of a foreground surface: a point
    splat knows nothing of the surface between its neighbours.  F·h·w must stay below 2³¹ (``source`` is int32).

    One pass over the sources' depth with 64-bit atomic minima, then one resolve pass (fm_render_views): no point cloud, no key tensor
    per (view, source) exists.  Never differentiable, and it only reads: nothing is cached or noted on any tensor, no LazyExtrinsics
    is left evaluated.  Host tensors after install() go to the same composition of the reference's own functions; without install()
    they are refused."""
    what = "render_views"
    with torch.no_grad():
        pose_tensor = _check_posed_depths(what, depths, intrinsics, extrinsics, colors)
        b, f, h, w = depths.shape
        if (views is None) == (held_out is None):
            raise ValueError(f"flowmap_amd: {what}: give exactly one of views=(K_v, E_v) and held_out=<a window of frames>")
        tensors = [("depths", depths), ("intrinsics", intrinsics), ("extrinsics", pose_tensor)] + ([("colors", colors)] if colors is not None else [])
        first_frame = kept_offsets = None
        if views is not None:
            if not isinstance(views, (tuple, list)) or len(views) != 2 or not all(torch.is_tensor(x) for x in views):
                raise ValueError(f"flowmap_amd: {what}: views must be a pair of tensors (K_v (b, V, 3, 3), E_v (b, V, 4, 4))")
            view_k, view_ext = views
            n_views = view_k.shape[1] if view_k.dim() == 4 else 0
            if n_views < 1 or tuple(view_k.shape) != (b, n_views, 3, 3) or tuple(view_ext.shape) != (b, n_views, 4, 4):
                raise RuntimeError(f"flowmap_amd: {what}: views of shapes {tuple(view_k.shape)} and {tuple(view_ext.shape)}; expected (b, V, 3, 3) and "
                                   f"(b, V, 4, 4) with b = {b}")
            tensors += [("views[0]", view_k), ("views[1]", view_ext)]
            first_source, n_sources = parse_window(sources, f, what, "frames")
            pairs = [(v, i) for v in range(n_views) for i in range(first_source, first_source + n_sources)]
        else:
            if sources is not None:
                raise ValueError(f"flowmap_amd: {what}: sources goes with views=; a held-out view is rendered from the frames at its offsets")
            kept_offsets = _check_offsets(offsets, f, what)
            first_frame, n_views = parse_window(held_out, f, what, "frames")
            pairs = [(v, first_frame + v + d) for v in range(n_views) for d in kept_offsets if 0 <= first_frame + v + d < f]
            view_k = view_ext = None
        _check_float32(what, tensors)
        is_int = lambda x: isinstance(x, int) and not isinstance(x, bool)  # noqa: E731
        if shape is None:
            shape = (h, w)
        if not isinstance(shape, (tuple, list)) or len(shape) != 2 or not all(is_int(x) and x >= 1 for x in shape):
            raise ValueError(f"flowmap_amd: {what}: shape must be (height, width) of the output, positive ints, got {shape!r}")
        shape = (int(shape[0]), int(shape[1]))
        if not is_int(radius) or not 0 <= radius <= 2:
            raise ValueError(f"flowmap_amd: {what}: radius must be 0, 1 or 2 (got {radius!r})")
        if not (isinstance(near, (int, float)) and 0.0 <= float(near) < float("inf")):
            raise ValueError(f"flowmap_amd: {what}: near must be a finite number >= 0 (got {near!r})")
        if not (isinstance(background, (int, float)) and float(background) == float(background)):
            raise ValueError(f"flowmap_amd: {what}: background must be a number (got {background!r})")
        if f * h * w >= 2**31:
            raise ValueError(f"flowmap_amd: {what}: frames x height x width = {f * h * w} does not fit the int32 source index (below 2^31): render a "
                             "window of the video")
        if b * len(pairs) > 65535:
            raise ValueError(f"flowmap_amd: {what}: batch x (view, source) pairs = {b * len(pairs)} exceeds the 65 535 rows of one call: ask for fewer views "
                             "or sources")
        dev = depths.device
        from .. import _reference

        held = slice(first_frame, first_frame + n_views) if views is None else None
        if _reference.twins and _reference.on_host(depths):  # host tensors after install(): the reference's own functions
            _reference.counters["host_calls"] += 1
            ext = _dense_extrinsics(extrinsics).detach()
            if views is None:
                view_k, view_ext = intrinsics[:, held], ext[:, held]
            out = _render_on_host(_reference.twins.__getitem__, depths.detach(), intrinsics.detach(), ext, None if colors is None else colors.detach(),
                                  view_k.detach(), view_ext.detach(), pairs, shape, radius, float(near), float(background))
            return RenderedViews(*out, (h, w), first_frame, kept_offsets)
        _refuse_host(what, dev)
        check_device(*(value for _, value in tensors))
        # (a LazyExtrinsics: the chain for this call only, nothing kept on it or noted on the flow tensor)
        ext, k = _peek_extrinsics(extrinsics), intrinsics.detach()
        if views is None:
            view_k, view_ext = k[:, held], ext[:, held]
        pair_tensor = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(dev)
        out = _ops.render_views(depths.detach(), _ops.intrinsics_inverse_peek(k), ext, None if colors is None else colors.detach(), view_k.detach(),
                                view_ext.detach(), pair_tensor, shape, radius, near, background)
        return RenderedViews(*out, (h, w), first_frame, kept_offsets)


def focal_sweep(depths: Tensor, weights, backward_flow: Tensor, focal_length_candidates: Tensor, pairs=None, indices: Optional[Tensor] = None,
                seed: int = 0, points: bool = False, poses: bool = True, num_points: Optional[int] = None) -> FocalSweep:
    """The softmin focal sweep (flowmap/model/intrinsics/intrinsics_softmin.py:85-141) of every pair of ``pairs`` — None (all), a slice with
    step 1 or (first, count), the forms of LossFlow.residuals; pair i is frames (i, i+1) — instead of pair 0 only, with what the reference
    drops kept: per candidate the error (float64) and the fitted pose of frame i+1 in frame i's space, per pair the softmin weights, the
    blended focal length and the blended K; with ``points`` the per-point term.  ``depths`` (b, f, h, w); ``weights`` (b, f-1, h, w), a tensor
    or a LazyWeights (its logits go to the kernel when its sensitivity is not 0, its value otherwise); ``backward_flow`` (b, f-1, h, w, 2);
    ``focal_length_candidates`` (n).  ``indices``: an int64 tensor of P pixel indices (one outside the image is clamped), or None:
    min(num_points, h·w) of them from ``_ops.random_subset(..., seed=seed)`` — an explicit seed, so the call advances no random state.

    ONE call of fm_focal_sweep: a launch with a workgroup per (batch entry, pair, candidate) that fits and scores from depth, and a launch
    with a wave per (batch entry, pair) for the curve.  Never differentiable, and it only reads: no LeadingFrames, no note on any tensor,
    no LazyWeights evaluated, no generator advanced.  Host tensors are refused — the reference has no function that returns this."""
    with torch.no_grad():
        if not torch.is_tensor(depths) or not torch.is_tensor(backward_flow) or not torch.is_tensor(focal_length_candidates):
            raise RuntimeError("flowmap_amd: focal_sweep: depths, backward_flow and focal_length_candidates must be tensors")
        dev = depths.device
        _refuse_host("focal_sweep", dev)
        if depths.dim() != 4:
            raise RuntimeError(f"flowmap_amd: focal_sweep: depths of shape {tuple(depths.shape)}; expected (batch, frame, height, width)")
        b, f, h, w = depths.shape
        if tuple(backward_flow.shape) != (b, f - 1, h, w, 2):
            raise RuntimeError(f"flowmap_amd: focal_sweep: backward_flow of shape {tuple(backward_flow.shape)} does not match the depths {(b, f, h, w)}: "
                               f"expected {(b, f - 1, h, w, 2)}")
        if weights is None or tuple(weights.shape) != (b, f - 1, h, w):
            raise RuntimeError(f"flowmap_amd: focal_sweep: weights of shape {None if weights is None else tuple(weights.shape)} do not match the depths "
                               f"{(b, f, h, w)}: expected {(b, f - 1, h, w)}")
        if focal_length_candidates.dim() != 1 or focal_length_candidates.numel() < 1:
            raise RuntimeError(f"flowmap_amd: focal_sweep: focal_length_candidates must be a non-empty 1-D tensor (got shape {tuple(focal_length_candidates.shape)})")
        weights, sens = _peek_weights(weights)
        _check_float32("focal_sweep", (("depths", depths), ("backward_flow", backward_flow), ("focal_length_candidates", focal_length_candidates),
                                       ("weights", weights)))
        _check_indices("focal_sweep", indices, dev)
        first, count = parse_window(pairs, f - 1, "focal_sweep", "pairs")
        if b * count > 65535:
            raise ValueError(f"flowmap_amd: focal_sweep: batch x pairs = {b * count} exceeds the 65 535 (batch entry, pair) rows of one call: "
                             "ask for a window of pairs")
        if indices is None:
            indices = _ops.random_subset(h * w, min(h * w if num_points is None else int(num_points), h * w), dev, seed=int(seed))
        from .model import focal_lengths_to_intrinsics

        candidates = focal_length_candidates.detach()
        candidate_k = focal_lengths_to_intrinsics(candidates, (h, w))
        out = _ops.focal_sweep(depths.detach(), weights.detach(), sens, backward_flow.detach(), indices, candidates, candidate_k,
                               _ops.intrinsics_inverse_peek(candidate_k), first, count, poses, points)
        return FocalSweep(first, count, candidates, indices, *out)


def _align_surfaces(surfaces, backward_flows: Tensor, backward_weights: Tensor, indices: Tensor, lazy_ok: bool):
    """``lazy_ok`` (ExtrinsicsProcrustes.forward, i.e. Model.forward -> ModelOutput.extrinsics): the chain may come back as a LazyExtrinsics;
    the function-level API above always returns the tensor."""
    idx = indices
    if isinstance(surfaces, LazySurfaces):
        h, w = surfaces.depths.shape[2:]
    else:
        h, w = surfaces.shape[2:4]
    if idx is not None and idx.numel() == h * w and getattr(idx, "_fm_is_arange", False):
        idx = None  # dense: the kernel derives the index from the thread id
    sens = 0.0
    if isinstance(backward_weights, LazyWeights):  # (at sensitivity 0 the value, evaluated and kept: the step differentiates through it)
        backward_weights, sens = backward_weights.kernel_input(keep=True)
    if isinstance(surfaces, LazySurfaces):
        # the chain only when something reads it (LazyExtrinsics): a training step (gradients recorded) on lazy surfaces, in an optimisation
        # where nothing has asked for the extrinsics so far.  (Inside a hipGraph capture too: a reader inside the captured region becomes part of
        # the graph, and the captured steps of this package — GraphedStep, GraphedShardedStep, training.py — hand no ModelOutput out of it.)
        lazy = (lazy_ok and _ops.options.lazy_extrinsics and torch.is_grad_enabled() and idx is not None and torch.is_tensor(backward_flows)
                and not backward_flows.__dict__.get("_fm_extrinsics_wanted", False))
        rel, rel_inv, extrinsics = _ops.ProcrustesFit.apply_chained(surfaces.depths, surfaces.intrinsics, None, backward_weights, backward_flows, idx, sens,
                                                                    want_extrinsics=not lazy)
        if lazy and extrinsics is None:
            return LazyExtrinsics(rel, rel_inv, backward_flows)
    else:
        rel, rel_inv, extrinsics = _ops.ProcrustesFit.apply_chained(None, None, surfaces, backward_weights, backward_flows, idx, sens)
    if extrinsics is None:  # (dense fits chain the poses in a launch of their own)
        extrinsics = _ops.PoseChain.apply(rel)
    # The per-pair poses the chain was built from: later(E)⁻¹·earlier(E) and its inverse up to
    # rounding (the chain cancels).  The fused flow loss reads them from here
    # instead of re-deriving them from the chain (two launches + three in the backward).
    extrinsics._fm_relative_poses = (rel_inv, rel)
    return extrinsics


# --------------------------------------------------------------------------------------
# tracks
# --------------------------------------------------------------------------------------


def compute_track_flow(surfaces, extrinsics: Tensor, intrinsics: Tensor, tracks):
    """flowmap/model/projection.py:255-298: reproject every track point from every source
    frame into every target frame.  Returns (xy_target (b,fs,ft,p,2), visibility
    (b,fs,ft,p) bool)."""
    surfaces, extrinsics = _dense(surfaces), _dense_extrinsics(extrinsics)
    check_device(surfaces, extrinsics, intrinsics, tracks.xy)
    b, f, h, w, _ = surfaces.shape
    p = tracks.xy.shape[2]
    xyz = _ops.BilinearSample.apply(surfaces.reshape(b * f, h, w, 3), tracks.xy.reshape(b * f, p, 2)).reshape(b, f, p, 3)
    rel = _ops.AllPairsPoses.apply(extrinsics)  # (b, fs, ft, 4, 4) = inv(E_ft) @ E_fs
    pts = xyz[:, :, None].expand(b, f, f, p, 3).reshape(b * f * f, p, 3)
    k = intrinsics[:, None].expand(b, f, f, 3, 3).reshape(b * f * f, 3, 3)
    xy_target = _ops.Reproject.apply(pts, rel.reshape(b * f * f, 4, 4), k).reshape(b, f, f, p, 2)
    xy_source = tracks.xy[:, :, None]
    visibility = tracks.visibility[:, :, None] & tracks.visibility[:, None]
    source_in = (xy_source >= 0).all(dim=-1) & (xy_source < 1).all(dim=-1)
    target_in = (xy_target >= 0).all(dim=-1) & (xy_target < 1).all(dim=-1)
    return xy_target, visibility & source_in & target_in
