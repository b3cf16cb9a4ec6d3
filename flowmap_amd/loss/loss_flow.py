"""Drop-in for flowmap/loss/loss_flow.py."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Literal, Optional

import torch
from torch import Tensor

from .. import _ops, _reference
from .._base import parse_window
from ..types import FlowResiduals
from ..model.projection import LazyExtrinsics, LazySurfaces, _dense_extrinsics, _peek_extrinsics, compute_backward_flow, compute_forward_flow, sample_image_grid
from .loss import Loss, LossCfgCommon, or_one
from .mapping import MappingCfg, get_mapping


@dataclass
class LossFlowCfg(LossCfgCommon):
    name: Literal["flow"]
    mapping: MappingCfg


class LossFlow(Loss[LossFlowCfg]):
    """flowmap/loss/loss_flow.py:26-70.

    Fast path (surfaces are a LazySurfaces of the model's own depths/intrinsics): ONE
    HIP kernel evaluates both flow directions straight from depth and writes every
    gradient in the same pass (fm_flow_loss_fused); nothing of size (b,f,h,w,3) or
    (b,f-1,h,w,2) is ever materialised.  General path (explicit surfaces tensor): the
    reference's composition of compute_*_flow -> mapping -> masked mean, each step a HIP
    kernel with its own backward.
    """

    reference_name = "LossFlow"

    # tuning knob of the fused kernel (items per thread); None -> library default
    items_per_thread: Optional[int] = None
    # park the dense depth gradient on the Procrustes node instead of returning it twice
    carry_depth_grad: bool = True
    # frame sharding: maps the local Σmask (fp64 device tensor) to the global one
    valid_sum_reducer = None
    # take the relative poses align_surfaces attached to the extrinsics instead of inverting the chain
    use_fitted_poses: bool = True

    def __init__(self, cfg: LossFlowCfg) -> None:
        super().__init__(cfg)
        self.mapping = get_mapping(cfg.mapping)

    # -- fused ----------------------------------------------------------------------------
    @staticmethod
    def _fusable(model_output) -> bool:
        s = model_output.surfaces
        return isinstance(s, LazySurfaces) and s.depths is model_output.depths

    # The tap exchange: when, in the previous step, a fused tracking loss followed this loss on the same depth parameter,
    # evaluate it AHEAD of the flow pass — same arguments, same value, returned when that loss is called — so that the pass can absorb its
    # depth gradient at the static taps instead of the tracking loss read-modify-writing cold lines of dL/ddepth afterwards.
    look_ahead: bool = True

    def _look_ahead(self, tracks, model_output, global_step: int) -> None:
        depths = model_output.surfaces.depths
        note = _ops._root(depths).__dict__.get("_fm_tracking_follows_flow")
        if note is None or not (torch.is_grad_enabled() and depths.requires_grad) or not _ops.options.tap_exchange:
            return
        follower, weight = note[0](), note[1]
        if follower is None or global_step < follower.cfg.enable_after or not follower._fusable(model_output, tracks):
            return
        if _ops.tap_plan_of(depths) is None or (id(follower), weight) in depths.__dict__.get("_fm_tracking_ahead", {}):
            return
        follower._fused(tracks, model_output, weight, look_ahead=True)

    def _fused(self, flows, model_output, weight: float, tracks=None, global_step: int = 0) -> Tensor:
        s: LazySurfaces = model_output.surfaces
        if tracks is not None and self.look_ahead and self.carry_depth_grad:
            self._look_ahead(tracks, model_output, global_step)
        s.depths.__dict__["_fm_flow_ran"] = True
        direct = getattr(model_output.extrinsics, "_fm_relative_poses", None) if self.use_fitted_poses else None
        if direct is not None and direct[0].shape[:2] == (s.depths.shape[0], s.depths.shape[1] - 1):
            rel_fwd, rel_bwd = direct  # straight from the Procrustes fit (align_surfaces)
        else:
            rel_fwd, rel_bwd = _ops.RelativePoses.apply(_dense_extrinsics(model_output.extrinsics))
        norm = _ops.flow_valid_norm(flows.forward_mask, flows.backward_mask, weight, self.valid_sum_reducer)
        packed = _ops.packed_flow_inputs(flows.forward, flows.backward, flows.forward_mask, flows.backward_mask)  # cached
        return _ops.FlowLossFused.apply(
            s.depths, model_output.intrinsics, rel_fwd, rel_bwd, flows.forward, flows.backward, flows.forward_mask,
            flows.backward_mask, norm, _ops.MAPPING_KINDS[self.mapping.kind], self.mapping.delta, self.carry_depth_grad,
            self.items_per_thread or 0, packed,
        )

    def compute_weighted_loss(self, batch, flows, tracks, model_output, global_step: int, weight: float) -> Tensor:
        if self._fusable(model_output):
            return self._fused(flows, model_output, weight, tracks, global_step)
        return weight * self.compute_unweighted_loss(batch, flows, tracks, model_output, global_step)

    # -- general --------------------------------------------------------------------------
    def compute_unweighted_loss(self, batch, flows, tracks: Optional[list], model_output, global_step: int) -> Tensor:
        if self._fusable(model_output):
            return self._fused(flows, model_output, 1.0, tracks, global_step)

        _, _, _, h, w = batch.videos.shape
        device = batch.videos.device
        xy, _ = sample_image_grid((h, w), device)

        # forward flow term (loss_flow.py:46-56)
        xy_flowed_forward = compute_forward_flow(model_output.surfaces, model_output.extrinsics, model_output.intrinsics)
        forward_loss = self.mapping.forward(xy_flowed_forward - xy, flows.forward, (h, w))
        loss_sum = (forward_loss * flows.forward_mask).sum()
        valid_sum = flows.forward_mask.sum()

        # backward flow term (loss_flow.py:58-68)
        xy_flowed_backward = compute_backward_flow(model_output.surfaces, model_output.extrinsics, model_output.intrinsics)
        backward_loss = self.mapping.forward(xy_flowed_backward - xy, flows.backward, (h, w))
        loss_sum = loss_sum + (backward_loss * flows.backward_mask).sum()
        valid_sum = valid_sum + flows.backward_mask.sum()

        return loss_sum / or_one(valid_sum)

    # -- per-pixel view ---------------------------------------------------------------------
    def residuals(self, batch, flows, model_output, pairs=None, predicted_flow: bool = False, sums: bool = True) -> FlowResiduals:
        """The per-pixel and per-pair quantities of ``compute_unweighted_loss`` (loss_flow.py:46-68) for the pairs ``pairs`` — None (all), a
        slice with step 1, or (first, count): ``forward`` / ``backward`` = mapping.forward(xy_flowed − xy, flow, (h, w)) BEFORE the mask;
        with ``predicted_flow`` the pose-induced flows xy_flowed − xy; with ``sums`` Σ residual·mask and Σ mask per pair and direction
        in float64.  The forward term of pair i reads frame i's depth, the backward term frame i+1's.

        On the model's own lazy surfaces (the fused loss's condition) this is ONE launch over depth (fm_flow_residuals, plus the small
        ordered second stage of the sums) and nothing of size (b,f,h,w,3) exists; with an explicit surfaces tensor it composes the
        general-path operators; host tensors after install() go to the reference's own functions.  Never differentiable, and it leaves
        the training step alone: no look-ahead or fused-Adam state, no tap image, no note on the flow tensors."""
        total = model_output.depths.shape[1] - 1
        first, count = parse_window(pairs, total, "LossFlow.residuals", "pairs")
        with torch.no_grad():
            if self._fusable(model_output) and not _reference.on_host(batch):
                return self._residuals_fused(flows, model_output, first, count, predicted_flow, sums)
            return self._residuals_general(batch, flows, model_output, first, count, predicted_flow, sums)

    def _residuals_fused(self, flows, model_output, first: int, count: int, predicted_flow: bool, sums: bool) -> FlowResiduals:
        s: LazySurfaces = model_output.surfaces
        ext = model_output.extrinsics
        direct = getattr(ext, "_fm_relative_poses", None) if (self.use_fitted_poses or isinstance(ext, LazyExtrinsics)) else None
        if direct is not None and direct[0].shape[:2] == (s.depths.shape[0], s.depths.shape[1] - 1):
            rel_fwd, rel_bwd = direct
        else:
            rel_fwd, rel_bwd = _ops.RelativePoses.apply(_dense_extrinsics(ext).detach())
        out = _ops.flow_residuals(s.depths.detach(), model_output.intrinsics.detach(), rel_fwd.detach(), rel_bwd.detach(), flows.forward, flows.backward,
                                  flows.forward_mask, flows.backward_mask, _ops.MAPPING_KINDS[self.mapping.kind], self.mapping.delta, first, count,
                                  predicted_flow, sums)
        return FlowResiduals(*out, first)

    def _residuals_general(self, batch, flows, model_output, first: int, count: int, predicted_flow: bool, sums: bool) -> FlowResiduals:
        _, _, _, h, w = batch.videos.shape
        # host tensors after install(): the reference's own functions (flowmap_amd/_reference.py); without install() ours refuse them
        grid = _reference.host_twin("sample_image_grid", batch) or sample_image_grid
        forward_flow = _reference.host_twin("compute_forward_flow", batch) or compute_forward_flow
        backward_flow = _reference.host_twin("compute_backward_flow", batch) or compute_backward_flow
        xy, _ = grid((h, w), batch.videos.device)
        ext = _peek_extrinsics(model_output.extrinsics)  # (a LazyExtrinsics: the chain for this call only, nothing is noted on the flow tensor)
        win, frames = slice(first, first + count), slice(first, first + count + 1)
        surfaces, ext, k = model_output.surfaces[:, frames], ext[:, frames], model_output.intrinsics[:, frames]
        fields = []
        for positions, flow, mask in ((forward_flow, flows.forward, flows.forward_mask), (backward_flow, flows.backward, flows.backward_mask)):
            pred = positions(surfaces, ext, k) - xy
            res = self.mapping.forward(pred, flow[:, win], (h, w))
            fields.append((res, pred, (res * mask[:, win]).to(torch.float64).sum(dim=(2, 3)), mask[:, win].to(torch.float64).sum(dim=(2, 3))))
        (rf, pf, sf, vf), (rb, pb, sb, vb) = fields
        return FlowResiduals(rf, rb, pf if predicted_flow else None, pb if predicted_flow else None, torch.stack((sf, sb), dim=-1) if sums else None,
                             torch.stack((vf, vb), dim=-1) if sums else None, first)
