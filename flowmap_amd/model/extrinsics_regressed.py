"""Drop-in for flowmap/model/extrinsics/extrinsics_regressed.py — explicit per-pair pose parameters (the paper's
``ablation_explicit_pose`` experiment): a quaternion and a translation for every pair of adjacent frames, turned into 4x4 matrices
and chained with get_extrinsics.  One HIP launch forward, one backward (``_ops.QuaternionPoses``)."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Literal

import torch
from torch import Tensor, nn

from .. import _ops, _reference
from .projection import LazyExtrinsics


@dataclass
class ExtrinsicsRegressedCfg:
    """flowmap/model/extrinsics/extrinsics_regressed.py:42-44"""

    name: Literal["regressed"]


class ExtrinsicsRegressed(nn.Module):
    """flowmap/model/extrinsics/extrinsics_regressed.py:47-83 (same parameter names, shapes and initial values: state_dict-compatible)"""

    def __init__(self, cfg: ExtrinsicsRegressedCfg, num_frames: int) -> None:
        super().__init__()
        self.cfg = cfg
        self.num_frames = num_frames
        assert num_frames >= 2
        # Initialize identity translations and rotations.
        self.translations = nn.Parameter(torch.zeros((num_frames - 1, 3), dtype=torch.float32))
        rotations = torch.zeros((num_frames - 1, 4), dtype=torch.float32)
        rotations[:, -1] = 1
        self.rotations = nn.Parameter(rotations)

    def forward(self, batch, flows, backbone_output, surfaces) -> Tensor:
        ref_cls = _reference.host_twin("ExtrinsicsRegressed", surfaces, batch)
        if ref_cls is not None:  # host tensors after install(): the reference's forward on THIS module's parameters (same names)
            return ref_cls.forward(self, batch, flows, backbone_output, surfaces)
        # (only the shape of the surfaces is read: a LazySurfaces stays unevaluated)
        b, f = surfaces.shape[:2]
        # Regressing the extrinsics only makes sense during overfitting.
        assert b == 1
        backward_flows = getattr(flows, "backward", None)
        # the chain only when something reads it (LazyExtrinsics), as ExtrinsicsProcrustes decides it: a training step in an optimisation where
        # nothing has asked for the extrinsics so far — the fused flow loss reads the relative poses
        lazy = (_ops.options.lazy_extrinsics and torch.is_grad_enabled() and torch.is_tensor(backward_flows)
                and not backward_flows.__dict__.get("_fm_extrinsics_wanted", False))
        rel, rel_inv, extrinsics = _ops.QuaternionPoses.apply(self.rotations, self.translations, not lazy)
        if lazy:
            return LazyExtrinsics(rel, rel_inv, backward_flows)
        # the per-pair poses the chain was built from: later(E)⁻¹·earlier(E) and its inverse (what _align_surfaces attaches)
        extrinsics._fm_relative_poses = (rel_inv, rel)
        return extrinsics
