"""Generate tests/golden/fn_track_residuals.npz: the per-(source frame, target frame, point) quantities of the REFERENCE's
LossTracking.compute_unweighted_loss (flowmap/loss/loss_tracking.py:44-56) — ``compute_track_flow``'s reprojected positions and visibility
and the three mappings of them BEFORE visibility — on two small track lists, in fp32 (its native precision) and in fp64 (same code,
inputs up-cast, its hard-coded fp32 constants patched as oracle/make_golden.py does).  Data only.  Needs the reference importable
(FLOWMAP_REFERENCE, as oracle/make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_track_residuals.py

Cases (tests/track_residual_cases.py: FIXTURE_SPECS; keys ``<case>_depth`` / ``_k`` / ``_extrinsics``, ``<case>_n_segments``,
``<case>_seg<i>_xy`` / ``_visibility`` / ``_start`` and, per segment, ``<case>_seg<i>_<kind>`` / ``_xy_target`` / ``_visible`` with their
``<case>_f64_`` twins):
  a   5 frames at 9 x 12, a K per frame; segments (start 0, f 5, P 40) and (start 1, f 3, P 7)
  b   5 frames at 10 x 13 (odd width); segments (0, 2, 65), (2, 3, 5), (0, 5, 3)
Both have source positions outside the frame with their bit set and invisible bits among visible neighbours.  The inputs come from the
tests' own generators, margin rule included, so the reference's fp32 and fp64 visibility agree — asserted here, together with the tests'
gate of the fp32 maps against the fp64 ones.
"""

from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

from oracle import make_golden as mg  # noqa: E402  (puts the reference and its stubs on sys.path; generates nothing on import)

from flowmap.loss.mapping import get_mapping  # noqa: E402
from flowmap.model import projection as rp  # noqa: E402
from flowmap.tracking.track_predictor import Tracks  # noqa: E402

from conftest import assert_close_or_reference_gap  # noqa: E402

from track_residual_cases import DELTA, FIXTURE_SPECS, KINDS, fixture_inputs  # noqa: E402


def reference_terms(spec, leaves, tracks, dtype):
    """loss_tracking.py:44-56 up to (not including) the masked sums, per segment, for the three mappings."""
    depth, k, ext = (x.to(dtype) for x in leaves)
    h, w = spec.hw
    xy, _ = rp.sample_image_grid((h, w), depth.device)
    surfaces = rp.unproject(xy.to(dtype), depth, k[:, :, None, None])  # model.py: the surfaces the loss is handed
    out = []
    for seg in tracks:
        s, f = seg.start_frame, seg.xy.shape[1]
        segment = Tracks(seg.xy.to(dtype), seg.visibility, s)
        xy_target, visible = rp.compute_track_flow(surfaces[:, s : s + f], ext[:, s : s + f], k[:, s : s + f], segment)
        terms = {"xy_target": xy_target, "visible": visible}
        for kind in KINDS:
            terms[kind] = get_mapping(mg.mapping_cfg(kind, DELTA)).forward(xy_target, segment.xy[:, None], (h, w))
        out.append(terms)
    return out


def main():
    arrays = {}
    for name, spec in FIXTURE_SPECS.items():
        leaves, tracks, altered, points = fixture_inputs(name)
        print(f"  {name}: {altered} of {points} points altered by the margin rule")
        r32 = reference_terms(spec, leaves, tracks, torch.float32)
        with mg.fp64_reference():
            r64 = reference_terms(spec, leaves, tracks, torch.float64)
        arrays.update({f"{name}_depth": leaves[0], f"{name}_k": leaves[1], f"{name}_extrinsics": leaves[2], f"{name}_n_segments": torch.tensor(len(tracks))})
        for i, (seg, a, b) in enumerate(zip(tracks, r32, r64)):
            assert torch.equal(a["visible"], b["visible"]), f"{name} segment {i}: the fp32 and fp64 visibility differ"
            assert 0 < int(a["visible"].sum()) < a["visible"].numel()
            for key in ("xy_target",) + KINDS:
                _, gap = assert_close_or_reference_gap(a[key], b[key], a[key], what=f"{name}.seg{i}.{key}")
                print(f"  {name}.seg{i}.{key}: fp32-to-fp64 gap {gap:.2e}")
            inside = ((seg.xy >= 0) & (seg.xy < 1)).all(-1)
            assert bool((seg.visibility & ~inside).any()) or i > 0, f"{name}: no source outside the frame with its bit set"
            arrays.update({f"{name}_seg{i}_xy": seg.xy, f"{name}_seg{i}_visibility": seg.visibility, f"{name}_seg{i}_start": torch.tensor(seg.start_frame)})
            arrays.update({f"{name}_seg{i}_{key}": v for key, v in a.items()})
            arrays.update({f"{name}_f64_seg{i}_{key}": v for key, v in b.items()})
    mg.save("fn_track_residuals", **arrays)


if __name__ == "__main__":
    main()
