"""The bit-mask packed format of the fused flow loss (fm_flow_masks_binary, fm_flow_pack_inputs_bitmask, fm_flow_loss_fused_bitmask) against
the fp32 packed format it replaces for binary masks.  Device-agnostic cases: tests/test_hostsim_flow_bitmask.py runs them on the serial host
double, tests/test_gpu_flow_bitmask.py on the GPU.

What is compared, and how hard:
* dL/ddepth of the flow pass (poses held fixed: the kernel's own output) is BIT-identical between the two formats on both devices — the kernel
  rebuilds 0.0f / 1.0f from the bits and runs the same arithmetic in the same order — and so are the values an in-pass Adam update and a tap
  exchange leave behind.
* the 13 per-(frame, direction) sums meet through fp64 atomics on the GPU: they, and everything derived from them (loss, pose and intrinsics
  gradients and — through the Procrustes fit's backward — the whole step's dL/ddepth and dL/dweights), pass the gate of the existing
  packed-vs-streamed test (cases.case_packed_inputs): 1e-5 relative, 1e-9 absolute.  On the serial host double they are equal.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import torch

import cases
from conftest import assert_close
from flowmap_amd import _ops, config
from flowmap_amd._base import FLOW_BITMASK_CHUNK_BYTES
from flowmap_amd._lib import call, ptr, stream_for
from oracle import flowmap_oracle as orc

GATE = dict(rel=1e-5, abs_=1e-9)
CHUNK = FLOW_BITMASK_CHUNK_BYTES


class FmFlowTaps(ctypes.Structure):
    """include/flowmap_hip.h: fm_flow_taps."""

    _fields_ = [("chunk_base", ctypes.c_void_p), ("pixel", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("scale", ctypes.c_void_p),
                ("depth", ctypes.c_void_p), ("stale", ctypes.c_void_p)]


def forced(bitmask: bool, first_sight: bool = True):
    """The Options switch that forces the fp32 format (False) or leaves the choice to the classification (True)."""
    return config.override(packed_bitmask=bitmask, pack_on_first_sight=first_sight)


def binary_flows(batch, f, h, w, seed=0, full=None):
    """(flow_fwd, flow_bwd, mask_fwd, mask_bwd) with masks of exactly 0.0f / 1.0f (``full``: every element that value)."""
    gen = torch.Generator().manual_seed(seed)
    ff = 0.01 * torch.randn((batch, f - 1, h, w, 2), generator=gen)
    fb = 0.01 * torch.randn((batch, f - 1, h, w, 2), generator=gen)
    mf = (torch.rand((batch, f - 1, h, w), generator=gen) < 0.7).float()
    mb = (torch.rand((batch, f - 1, h, w), generator=gen) < 0.6).float()
    if full is not None:
        mf, mb = torch.full_like(mf, full), torch.full_like(mb, full)
    return ff, fb, mf, mb


def numpy_bitmask_layout(ff, fb, mf, mb):
    """The layout include/flowmap_hip.h describes, re-derived with numpy from the four tensors (b, F-1, H, W[, 2])."""
    ff, fb, mf, mb = (x.detach().cpu().numpy() for x in (ff, fb, mf, mb))
    b, pairs, h, w = mf.shape
    f, quads = pairs + 1, h * w // 4
    chunks = (quads + 63) // 64
    out = np.zeros((b * f, chunks, CHUNK), np.uint8)
    for be in range(b):
        for fr in range(f):
            flows = np.zeros((chunks * 64, 4, 4), np.float32)  # [quad][vector][component]
            bits = np.zeros((chunks * 64,), np.uint8)
            weights = np.array([1, 2, 4, 8], np.uint8)
            if fr < f - 1:
                flows[:quads, 0:2] = ff[be, fr].reshape(quads, 2, 4)
                bits[:quads] |= ((mf[be, fr].reshape(quads, 4) != 0) * weights).sum(1).astype(np.uint8)
            if fr > 0:
                flows[:quads, 2:4] = fb[be, fr - 1].reshape(quads, 2, 4)
                bits[:quads] |= (((mb[be, fr - 1].reshape(quads, 4) != 0) * weights).sum(1) << 4).astype(np.uint8)
            flows = flows.reshape(chunks, 64, 4, 4).transpose(0, 2, 1, 3).reshape(chunks, 4096 // 4)  # [chunk][vector][lane][component]
            out[be * f + fr, :, :4096] = flows.view(np.uint8).reshape(chunks, 4096)
            out[be * f + fr, :, 4096:4160] = bits.reshape(chunks, 64)
    return out


def case_header_constant():
    header = (Path(__file__).resolve().parent.parent / "include" / "flowmap_hip.h").read_text()
    assert int(re.search(r"#define FM_FLOW_BITMASK_CHUNK_BYTES (\d+)", header).group(1)) == CHUNK
    assert CHUNK % 16 == 0 and CHUNK >= 4096 + 64


def case_pack_layout(dev, batch, f, hw, views=False):
    """fm_flow_pack_inputs_bitmask(_views) against the numpy re-layout: tail chunks (quads not a multiple of 64), F = 2, batch > 1 and
    frame windows of larger tensors."""
    h, w = hw
    if views:  # a window of f frames out of f + 3: read in place through fm_layout
        big = binary_flows(batch, f + 3, h, w, seed=3)
        ff, fb, mf, mb = (x.to(dev)[:, 2 : 2 + f - 1] for x in big)
        assert not mf.is_contiguous() or batch == 1 and f == 2
    else:
        ff, fb, mf, mb = (x.to(dev) for x in binary_flows(batch, f, h, w, seed=3))
    before = dict(_ops.counters)
    with forced(True):
        packed = _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (batch * f, (h * w // 4 + 63) // 64, CHUNK)
    assert _ops.counters["flow_packs_bitmask"] - before["flow_packs_bitmask"] == 1 and _ops.counters["flow_packs"] - before["flow_packs"] == 1
    assert np.array_equal(packed.cpu().numpy(), numpy_bitmask_layout(ff, fb, mf, mb))
    with forced(True):
        assert _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True) is packed  # cached, decision included
    with forced(False):  # the switch: the fp32 format of the same tensors
        wide = _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True)
    assert wide.dtype == torch.float32 and tuple(wide.shape) == (batch * f, (h * w // 4 + 63) // 64, 6, 64, 4)
    assert _ops.counters["flow_packs_bitmask"] - before["flow_packs_bitmask"] == 1


ODD_VALUES = {"half": 0.5, "minus_zero": -0.0, "nan": float("nan"), "one_plus_ulp": float(np.nextafter(np.float32(1.0), np.float32(2.0)))}


def case_classification(dev, which, odd):
    """One odd element in either mask selects the fp32 format; all-zero and all-one masks select bits (counters)."""
    b, f, h, w = 2, 3, 10, 12
    full = {"zeros": 0.0, "ones": 1.0}.get(odd)
    ff, fb, mf, mb = (x.to(dev) for x in binary_flows(b, f, h, w, seed=5, full=full))
    if full is None and odd != "binary":
        target = mf if which == "fwd" else mb
        target[1, 1, 7, 5 if which == "fwd" else 11] = ODD_VALUES[odd]  # (an in-place edit before the first pack)
    before = dict(_ops.counters)
    with forced(True):
        packed = _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True)
    want_bits = full is not None or odd == "binary"
    assert _ops.counters["flow_packs"] - before["flow_packs"] == 1
    assert _ops.counters["flow_packs_bitmask"] - before["flow_packs_bitmask"] == int(want_bits)
    assert packed.dtype == (torch.uint8 if want_bits else torch.float32)
    if not want_bits:  # the existing format, bit for bit
        with forced(False):
            again = _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True)
        assert tuple(packed.shape) == (b * f, (h * w // 4 + 63) // 64, 6, 64, 4)
        assert np.array_equal(packed.cpu().numpy().view(np.uint32), again.cpu().numpy().view(np.uint32))


def case_repack(dev):
    """An in-place mask edit bumps the version: repacked AND reclassified, both ways."""
    b, f, h, w = 1, 3, 8, 16
    ff, fb, mf, mb = (x.to(dev) for x in binary_flows(b, f, h, w, seed=9))
    with forced(True):
        first = _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True)
        assert first.dtype == torch.uint8
        mb[0, 0, 3, 3] = 0.25
        second = _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True)
        assert second is not first and second.dtype == torch.float32
        mb[0, 0, 3, 3] = 1.0
        third = _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True)
        assert third.dtype == torch.uint8 and np.array_equal(third.cpu().numpy(), numpy_bitmask_layout(ff, fb, mf, mb))


# ---- the kernel, entry point against entry point -----------------------------------------------------------------------------------------


def _tap_tables(batch, f, h, w, gen, per_frame):
    """A static tap set in (frame, pixel) order: (chunk_base (B·F·chunks + 1) int32, pixel (M) int32)."""
    chunks = (h * w // 4 + 63) // 64
    pixels, base = [], [0]
    for _ in range(batch * f):
        px = torch.randperm(h * w, generator=gen)[:per_frame].sort().values
        for c in range(chunks):
            base.append(base[-1] + int(((px >= 256 * c) & (px < 256 * (c + 1))).sum()))
        pixels.append(px)
    return torch.tensor(base, dtype=torch.int32), torch.cat(pixels).to(torch.int32)


def case_kernel_parity(dev, kind, variant, hw, batch=1, f=4):
    """fm_flow_loss_fused_bitmask against fm_flow_loss_fused / _adam / _taps reading the fp32 packed copy of the same binary-mask inputs:
    dL/ddepth, the updated depth / exp_avg / exp_avg_sq and the tap image bit-identical, the fp64 sums equal (host) or within the gate (GPU)."""
    h, w = hw
    gen = torch.Generator().manual_seed(17)
    adam, taps = variant in ("adam", "adam_taps"), variant in ("taps", "adam_taps")
    depth0 = (1.0 + 0.3 * torch.rand((batch, f, h, w), generator=gen)).to(dev)
    k = orc.focal_to_k(torch.tensor(0.85), (h, w)).float().repeat(batch, f, 1, 1).contiguous().to(dev)
    kinv = torch.linalg.inv(k.cpu().double()).float().contiguous().to(dev)
    t_fwd = cases._random_rigid(batch * (f - 1), gen).float().reshape(batch, f - 1, 4, 4).contiguous().to(dev)
    t_bwd = cases._random_rigid(batch * (f - 1), gen).float().reshape(batch, f - 1, 4, 4).contiguous().to(dev)
    ff, fb, mf, mb = (x.to(dev) for x in binary_flows(batch, f, h, w, seed=23))
    scale = torch.tensor([0.37], device=dev)
    chunks = (h * w // 4 + 63) // 64
    stream = stream_for(depth0)
    wide = torch.empty((batch * f, chunks, 6, 64, 4), dtype=torch.float32, device=dev)
    bits = torch.empty((batch * f, chunks, CHUNK), dtype=torch.uint8, device=dev)
    call("fm_flow_pack_inputs", ptr(ff), ptr(fb), ptr(mf), ptr(mb), batch, f, h, w, ptr(wide), stream)
    call("fm_flow_pack_inputs_bitmask", ptr(ff), ptr(fb), ptr(mf), ptr(mb), batch, f, h, w, ptr(bits), stream)
    touched = (torch.rand((batch * f * h * w // 4,), generator=gen) < 0.3).to(torch.uint8) * 5  # bits 0 and 2 of some quads
    touched = touched.to(dev)
    chunk_base, pixel = _tap_tables(batch, f, h, w, gen, per_frame=37)
    tap_grad = torch.randn((pixel.numel(),), generator=gen)
    chunk_base, pixel, tap_grad, tap_scale = chunk_base.to(dev), pixel.to(dev), tap_grad.to(dev), torch.tensor([0.5], device=dev)
    ax, ay = w / (h * w) ** 0.5, h / (h * w) ** 0.5
    kind_id, delta = _ops.MAPPING_KINDS[kind], 0.01
    hyper = (3, 1e-3, 0.9, 0.999, 1e-8)

    def run(fmt):
        depth = depth0.clone()
        exp_avg, exp_avg_sq = 0.01 * torch.ones_like(depth), 1e-4 * torch.ones_like(depth)
        grad = torch.zeros_like(depth)
        acc = torch.zeros((batch * f * 2 * _ops.FLOW_ACC_STRIDE,), dtype=torch.float64, device=dev)
        tap_depth = torch.zeros((pixel.numel(),), device=dev)
        tp = FmFlowTaps(ptr(chunk_base), ptr(pixel), ptr(tap_grad), ptr(tap_scale), ptr(tap_depth), None)
        geometry = (batch, f, h, w, kind_id, delta, ax, ay, ptr(grad), ptr(acc), 0)
        adam_args = (ptr(exp_avg), ptr(exp_avg_sq), ptr(touched), *hyper) if adam else (None, None, None, 0, 0.0, 0.0, 0.0, 0.0)
        head = (ptr(depth), ptr(k), ptr(kinv), ptr(t_fwd), ptr(t_bwd))
        if fmt == "bits":
            call("fm_flow_loss_fused_bitmask", *head, ptr(bits), ptr(scale), *geometry, None, ctypes.addressof(tp) if taps else None, *adam_args, stream)
        elif taps:
            call("fm_flow_loss_fused_taps", *head, None, None, None, None, ptr(wide), ptr(scale), *geometry, ctypes.addressof(tp), *adam_args, stream)
        elif adam:
            call("fm_flow_loss_fused_adam", *head, None, None, None, None, ptr(wide), ptr(scale), *geometry, *adam_args, stream)
        else:
            call("fm_flow_loss_fused", *head, None, None, None, None, ptr(wide), ptr(scale), *geometry, stream)
        return {"depth": depth.cpu(), "exp_avg": exp_avg.cpu(), "exp_avg_sq": exp_avg_sq.cpu(), "grad_depth": grad.cpu(), "acc": acc.cpu(),
                "tap_depth": tap_depth.cpu()}

    wide_out, bits_out = run("wide"), run("bits")
    assert float(wide_out["grad_depth"].abs().max()) > 0 and float(wide_out["acc"].abs().max()) > 0  # (the comparison is not vacuous)
    if adam:
        assert not torch.equal(wide_out["depth"], depth0.cpu())
    if taps:
        assert float(wide_out["tap_depth"].abs().max()) > 0
    for key in ("grad_depth", "depth", "exp_avg", "exp_avg_sq", "tap_depth"):
        assert torch.equal(wide_out[key], bits_out[key]), (key, float((wide_out[key] - bits_out[key]).abs().max()))
    one_workgroup_per_frame = h * w // 4 <= 256 * 3  # (one atomic per value: the sums are deterministic on the GPU too)
    if str(dev) == "cpu" or one_workgroup_per_frame:
        assert torch.equal(wide_out["acc"], bits_out["acc"])
    else:
        assert_close(bits_out["acc"], wide_out["acc"], what="the 13 sums", **GATE)


def case_loss_parity(dev, kind, hw=(18, 28), view=False):
    """FlowLossFused with the poses held as leaves, forced fp32 format against bits: dL/ddepth torch.equal; loss and pose / intrinsics
    gradients equal (host) or within the gate (GPU).  ``view``: depth is a frame window of a larger tensor (fm_layout)."""
    h, w = hw
    f = 4
    gen = torch.Generator().manual_seed(31)
    depth_full = 1.0 + 0.3 * torch.rand((1, f + 2, h, w), generator=gen)
    k0 = orc.focal_to_k(torch.tensor(0.85), (h, w)).float().repeat(1, f, 1, 1)
    tf0 = cases._random_rigid(f - 1, gen)[None].float()
    tb0 = cases._random_rigid(f - 1, gen)[None].float()
    ff, fb, mf, mb = (x.to(dev) for x in binary_flows(1, f, h, w, seed=37))
    norm = _ops.flow_valid_norm(mf, mb, 1000.0)
    out = {}
    for bitmask in (False, True):
        base = depth_full.clone().to(dev).requires_grad_(True)
        d = base[:, 1 : 1 + f] if view else base[:, :f].contiguous()
        kk, tf, tb = (x.clone().to(dev).requires_grad_(True) for x in (k0, tf0, tb0))
        with forced(bitmask):
            pk = _ops.packed_flow_inputs(ff, fb, mf, mb, eager=True)
        assert pk.dtype == (torch.uint8 if bitmask else torch.float32)
        loss = _ops.FlowLossFused.apply(d, kk, tf, tb, ff, fb, mf, mb, norm, _ops.MAPPING_KINDS[kind], 0.01, False, 0, pk)
        loss.backward()
        out[bitmask] = {"loss": loss.detach().cpu(), "g_depth": base.grad.cpu(), "g_k": kk.grad.cpu(), "g_t_fwd": tf.grad.cpu(), "g_t_bwd": tb.grad.cpu()}
    assert float(out[False]["g_depth"].abs().max()) > 0
    assert torch.equal(out[True]["g_depth"], out[False]["g_depth"])
    for key in ("loss", "g_k", "g_t_fwd", "g_t_bwd"):
        if str(dev) == "cpu":
            assert torch.equal(out[True][key], out[False][key]), key
        else:
            assert_close(out[True][key], out[False][key], what=key, **GATE)


def case_step_parity(dev, kind, tracking=False, hw=(24, 32)):
    """The whole step (explicit depth, regressed focal length, Procrustes poses; ``tracking``: flow + tracking losses, three steps, so that
    the tap exchange runs) through the forced fp32 format and through bits.  On the host double every output is equal.  On the GPU the
    pose gradients come from fp64 atomics and reach dL/ddepth and dL/dweights through the Procrustes fit's backward: all outputs pass the
    gate; the pass's own dL/ddepth is held to equality by case_loss_parity / case_kernel_parity."""
    from helpers import run_ours

    h, w = hw
    f = 5
    sc = orc.synth_scene(f, h, w, seed=21)
    oflows = sc["flows"]
    assert all(bool(((m == 0) | (m == 1)).all()) for m in (oflows.forward_mask, oflows.backward_mask))
    wlogit = 0.01 * torch.randn((f - 1, h, w), generator=torch.Generator().manual_seed(3))
    tracks = orc.synth_tracks(f, h, w, scene=sc, seed=21, interval=2, radius=2, grid=5) if tracking else None
    res = {}
    for bitmask in (False, True):
        before = dict(_ops.counters)
        with forced(bitmask):
            # (fresh tensor objects per run: what the package caches on them — packed copies, scatter plans — starts from nothing both times)
            fresh = orc.OFlows(*(x.clone() for x in (oflows.forward, oflows.backward, oflows.forward_mask, oflows.backward_mask)))
            res[bitmask] = run_ours(sc["depth_init"], wlogit, 0.9, fresh, (h, w), 60, otracks=tracks, kind=kind, device=dev, steps=3 if tracking else 1)
        assert _ops.counters["flow_packs"] - before["flow_packs"] == 1
        assert _ops.counters["flow_packs_bitmask"] - before["flow_packs_bitmask"] == int(bitmask)
        if tracking:
            assert _ops.counters["flow_tap_passes"] > before["flow_tap_passes"]
    for key in ("total", "loss_flow", "loss_tracking", "extrinsics", "g_depth", "g_wlogit", "g_focal"):
        if str(dev) == "cpu":
            assert torch.equal(res[True][key], res[False][key]), key
        else:
            assert_close(res[True][key], res[False][key], what=key, **GATE)


def _optimise(dev, bitmask, steps, in_pass=True, release_at=None, graph=False):
    """``steps`` of flow-loss overfitting on a consistent scene with FusedAdam (``in_pass``: the depth update inside the flow pass)."""
    import flowmap_amd
    from flowmap_amd import FusedAdam

    try:
        with forced(bitmask, first_sight=False):
            model, batch, flows, loss_of = cases._small_problem(dev, tracking=False)
            optimizer = FusedAdam(model.parameters(), lr=1e-3, capturable=graph)
            if in_pass:
                optimizer.fuse_depth_update(model.backbone.depth, max_touched_fraction=1.0)
            before = dict(_ops.counters)
            losses = []

            def step():
                optimizer.zero_grad(set_to_none=True)
                loss = loss_of(model(batch, flows, 0))
                loss.backward()
                optimizer.step()
                return loss

            if graph:
                graphed = flowmap_amd.GraphedStep(step, warmup=3)
                try:
                    for _ in range(steps - 3):
                        losses.append(float(graphed()))
                finally:
                    graphed.close()
            else:
                for i in range(steps):
                    losses.append(float(step().detach()))
                    if release_at is not None and i == release_at:
                        flowmap_amd.release_flow_originals(flows)
            moved = {key: _ops.counters[key] - before[key] for key in ("flow_packs", "flow_packs_bitmask")}
            focal = next(p for name, p in model.named_parameters() if name.endswith("focal_length"))
            return {"losses": torch.tensor(losses), "depth": model.backbone.depth.detach().cpu().clone(), "weights": model.backbone.weights.detach().cpu().clone(),
                    "focal": focal.detach().cpu().clone(), "in_pass_updates": optimizer.counters.get("in_pass_updates", 0), "moved": moved}
    finally:
        flowmap_amd.set_lazy_surfaces(False)


def _compare_runs(dev, got, want, keys=("losses", "depth", "weights", "focal")):
    for key in keys:
        if str(dev) == "cpu":
            assert torch.equal(got[key], want[key]), key
        else:
            assert_close(got[key], want[key], what=key, **GATE)


def case_in_pass_adam_parity(dev, steps=6):
    """The in-pass Adam update reading bits against the same update reading the fp32 format: the same trajectory (equal on the host double)."""
    wide, bits = _optimise(dev, False, steps), _optimise(dev, True, steps)
    assert wide["moved"] == {"flow_packs": 1, "flow_packs_bitmask": 0} and bits["moved"] == {"flow_packs": 1, "flow_packs_bitmask": 1}
    assert bits["in_pass_updates"] == wide["in_pass_updates"] >= steps - 3
    _compare_runs(dev, bits, wide)


def case_release_originals(dev, steps=5):
    """release_flow_originals after the bit-mask pack: the following steps read the packed bytes alone and walk the same trajectory."""
    kept, released = _optimise(dev, True, steps, in_pass=False), _optimise(dev, True, steps, in_pass=False, release_at=2)
    assert released["moved"] == {"flow_packs": 1, "flow_packs_bitmask": 1}
    _compare_runs(dev, released, kept)


def case_graphed_step(dev, steps=8):
    """GraphedStep on binary masks: the warm-up packs (bits), the replays equal the eager steps."""
    eager, graphed = _optimise(dev, True, steps, in_pass=False), _optimise(dev, True, steps, in_pass=False, graph=True)
    assert graphed["moved"] == {"flow_packs": 1, "flow_packs_bitmask": 1}
    assert_close(graphed["losses"], eager["losses"][3:], what="loss history", **GATE)
    _compare_runs(dev, graphed, eager, keys=("depth", "weights", "focal"))
