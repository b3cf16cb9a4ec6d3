"""What the case modules of the read-only operators (tests/*_cases.py: LossFlow.residuals, LossTracking.residuals,
ExtrinsicsProcrustes.residuals, IntrinsicsSoftmin.residuals, depth_consistency, render_views, voxel_point_cloud) share: the training loop
behind "the operator leaves training alone" and its common assertions, the loop over refused C calls, the bit-equality walker, and a few
small gates.  Nothing here knows an operator: a module hands in its calls, its counter's name and its tables, and keeps its own assertions."""

from __future__ import annotations

import ctypes
import types
from typing import NamedTuple

import torch

from conftest import relerr
from oracle import flowmap_oracle as orc


# ---- small gates ---------------------------------------------------------------------------------------------------------------------------


def ulp_distance(a, b):
    """Largest distance, in units in the last place of fp32, between two finite fp32 tensors."""
    def key(v):
        i = v.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)

    return int((key(a) - key(b)).abs().max())


def gate_pair(a, b, gap, what):
    """Two fp32 evaluations of one quantity against each other: max(1e-4, 2 x the fp32-to-fp64 gap of that quantity)."""
    e = relerr(a, b)
    assert e <= max(1e-4, 2.0 * gap), f"{what}: rel err {e:.3e} > max(1e-4, 2 x fp32-reference gap {gap:.3e})"
    return e


def window_rows(window, count):
    """The rows of a full call (``count`` of them: frames or pairs) that a window — None, (first, count) or a slice — selects."""
    if window is None:
        return slice(0, count)
    if isinstance(window, slice):
        return slice(*window.indices(count)[:2])
    return slice(window[0], window[0] + window[1])


def same_tensors(a, b, fields, what="", rows=None, batch=None, scalars=(), equal=torch.equal):
    """Two results equal bit for bit: the attributes ``scalars`` compare equal, and every attribute of ``fields`` is None in both or has
    the same shape, dtype and — by ``equal`` — content.  ``rows`` / ``batch``: ``a`` is compared with ``b[:, rows]`` / ``b[batch]``."""
    for name in scalars:
        assert getattr(a, name) == getattr(b, name), f"{what}{name}: {getattr(a, name)} vs {getattr(b, name)}"
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), f"{what}{name}"
        if x is None:
            continue
        y = y if rows is None else y[:, rows]
        y = y if batch is None else y[batch]
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}{name}: {x.dtype} {tuple(x.shape)} vs {y.dtype} {tuple(y.shape)}"
        assert equal(x, y), f"{what}{name}: not bit-equal (max |diff| {float((x.double() - y.double()).abs().max()):.3e})"


def host_tensor_refused(call, match):
    """Without install() and without the test double, ``call`` on host tensors is refused with the package's message
    (test_abi.py::test_no_cpu_fallback)."""
    import pytest

    from flowmap_amd import _lib

    _lib.set_library_for_testing(None)
    with pytest.raises(RuntimeError, match=match):
        call()


# ---- a C entry through ctypes, on REFUSED calls only ---------------------------------------------------------------------------------------


def c_entry_refuses(lib, what, entry, params, valid, refused, pointer=None):
    """Call ``entry`` of ``lib`` once per element of ``refused`` — "nulls" (every pointer null) or a dict of parameters changed against
    ``valid`` — and assert that it returns 1.  ``params`` names the entry's parameters in order.  A pointer is null for ``stream``, for a
    parameter changed to None and for "nulls"; every other one is the address of 4 KiB of HOST memory, 64-byte aligned, that is never
    dereferenced because the entry refuses before it launches anything — or what ``pointer(param, change, address)`` returns.  A
    parameter missing from ``valid`` and from the change is a KeyError, not a default."""
    from flowmap_amd import _lib

    fn = getattr(lib, entry)
    fn.argtypes, fn.restype = _lib.SIGNATURES[entry], ctypes.c_int
    raw = ctypes.create_string_buffer(4096 + 64)
    address = (ctypes.addressof(raw) + 63) & ~63
    for change in refused:
        nulls = change == "nulls"
        change = {} if nulls else change
        args = []
        for param, kind in zip(params, _lib.SIGNATURES[entry], strict=True):
            if kind is not ctypes.c_void_p:
                args.append({**valid, **change}[param])
            elif nulls or param == "stream" or (param in change and change[param] is None):
                args.append(None)
            else:
                args.append(address if pointer is None else pointer(param, change, address))
        assert fn(*args) == 1, f"{what}: {entry} did not refuse ({'all pointers null' if nulls else change})"


# ---- an operator leaves training alone -----------------------------------------------------------------------------------------------------

FRAMES, HEIGHT, WIDTH = 5, 24, 32  # the training problem: cases._small_problem's consistent scene, synthetic tracks at seed 21


class Trained(NamedTuple):
    history: list  # per step: {"loss", "g_depth" (None with ``fuse`` or without a gradient), "g_<name>" of every other parameter with a gradient}
    params: dict  # name -> every parameter after the last step
    moved: dict  # the operator counters' deltas over the counted steps (taken after the warm-up)
    notes: list  # the names of the ``_fm_*`` notes on the backward flows, the depth and the weight tensors
    state: dict  # in_pass (FusedAdam's updates inside the flow pass), depth_version, and with tracking the number of track segments
    seen: list  # what the calls returned: mid, after, mid, after, ...
    lazy_kept: list  # per ``mid`` call: (the output's extrinsics were an unevaluated LazyExtrinsics before, and after)
    model: object


def _unevaluated(extrinsics):
    from flowmap_amd.model.projection import LazyExtrinsics

    return isinstance(extrinsics, LazyExtrinsics) and extrinsics._dense is None


def batch_colours(ns):
    """A ``prepare`` for operators that colour from the batch: the problem's own videos are zeros."""
    ns.batch.videos = torch.rand((1, FRAMES, 3, HEIGHT, WIDTH), generator=torch.Generator().manual_seed(5)).to(ns.batch.videos.device)


def train(dev, *, tracking, fuse, steps, first_step, warm_up, calls=None, intrinsics=None, prepare=None) -> Trained:
    """``steps`` optimisation steps, global steps ``first_step``.., of the flow loss (weight 1000; with ``tracking`` plus the tracking loss,
    weight 100, and the tap exchange at any size) with FusedAdam(lr=1e-3) — ``fuse``: FusedAdam.fuse_depth_update, the depth update inside
    the flow pass — on cases._small_problem (``intrinsics``: its intrinsics configuration).

    ``calls``: None, or (mid, after): ``mid(ns)`` runs between forward and backward, ``after(ns)`` after optimizer.step(), ``ns`` a namespace
    of model, batch, flows, tracks, out, flow_fn, track_fn and step; what they return is collected in ``seen``.  ``prepare(ns)`` runs once
    when the problem is built (out and step are None then).  A test runs this twice, without and with calls, and hands both records to
    ``assert_training_untouched``.

    ``warm_up``: one forward + backward at step 0 whose gradients are thrown away, in both runs, before anything is counted or compared.
    The sparse fit's scatter plan is built when the same (indices, flows) come back a second time, and until it exists
    fm_procrustes_scatter adds into dL/ddepth with float atomics — two runs of that FIRST backward differ in the last bit of dL/ddepth
    where two taps share a pixel ("Determinism"), calls or no calls, and Adam would carry the bit into every later step.  No
    parameter moves in the warm-up; it is a training step of every module that keeps state per forward all the same (the softmin sweep's
    window grows by one).  From the second backward on every sum into dL/ddepth has a fixed order, so the two runs are comparable bit for
    bit on the GPU as on the host double — given ``max_touched_fraction=1.0`` (the depth update inside the pass never falls back to the
    separate one by how many pixels the other operators touched) and, where ``intrinsics`` is a softmin sweep, a sweep small enough that ONE
    wavefront issues all of its backward's float atomics (focal_sweep_cases.case_training_untouched: 64 points, 6 candidates)."""
    import cases
    import flowmap_amd
    from flowmap_amd import FusedAdam, _ops, config
    from flowmap_amd.loss import LossFlow, LossFlowCfg, LossTracking, LossTrackingCfg
    from helpers import mapping_cfg, to_tracks

    f, h, w = FRAMES, HEIGHT, WIDTH
    with config.override(tap_exchange_min_bytes=0):
        try:
            model, batch, flows, _ = cases._small_problem(dev, f=f, h=h, w=w, tracking=False, intrinsics=intrinsics)
            sc = orc.synth_scene(f, h, w, seed=21)
            tracks = to_tracks(orc.synth_tracks(f, h, w, scene=sc, seed=21, interval=2, radius=2, grid=5), dev) if tracking else None
            ns = types.SimpleNamespace(model=model, batch=batch, flows=flows, tracks=tracks, out=None, step=None,
                                       flow_fn=LossFlow(LossFlowCfg(0, 1000.0, "flow", mapping_cfg("huber"))),
                                       track_fn=LossTracking(LossTrackingCfg(0, 100.0, "tracking", mapping_cfg("huber"))))
            if prepare is not None:
                prepare(ns)
            optimizer = FusedAdam(model.parameters(), lr=1e-3)
            depth = model.backbone.depth
            if fuse:
                optimizer.fuse_depth_update(depth, max_touched_fraction=1.0)
            model.train()

            def forward_loss(step):
                out = model(batch, flows, step)
                total = ns.flow_fn(batch, flows, tracks, out, step)
                return out, (total + ns.track_fn(batch, flows, tracks, out, step) if tracking else total)

            if warm_up:
                out, total = forward_loss(0)
                total.backward()
                optimizer.zero_grad(set_to_none=True)
                del out, total
            before = dict(_ops.counters)
            history, seen, lazy_kept = [], [], []
            for step in range(first_step, first_step + steps):
                ns.step = step
                optimizer.zero_grad(set_to_none=True)
                ns.out, total = forward_loss(ns.step)
                if calls is not None:
                    was = _unevaluated(ns.out.extrinsics)
                    seen.append(calls[0](ns))
                    lazy_kept.append((was, _unevaluated(ns.out.extrinsics)))
                total.backward()
                record = {"loss": total.detach().clone(), "g_depth": None if (fuse or depth.grad is None) else depth.grad.detach().clone()}
                record.update({f"g_{name}": p.grad.detach().clone() for name, p in model.named_parameters() if p is not depth and p.grad is not None})
                history.append(record)
                optimizer.step()
                if calls is not None:
                    seen.append(calls[1](ns))
            moved = {key: value - before.get(key, 0) for key, value in _ops.counters.items()}
            params = {name: p.detach().clone() for name, p in model.named_parameters()}
            # (a note's name may end in the id() of the object it belongs to: dropped, the two runs build their own objects)
            notes = sorted(key.rstrip("0123456789") for tensor in (flows.backward, depth, model.backbone.weights) for key in tensor.__dict__
                           if key.startswith("_fm_"))
            state = {"in_pass": optimizer.counters.get("in_pass_updates", 0), "depth_version": depth._version}
            if tracking:
                state["segments"] = len(tracks)
            return Trained(history, params, moved, notes, state, seen, lazy_kept, model)
        finally:
            flowmap_amd.set_lazy_surfaces(False)


def assert_training_untouched(plain: Trained, with_calls: Trained, counter, calls_expected):
    """What every operator promises of a run with its calls against the same run without: the loss and every recorded gradient of every
    step and every parameter after the last are bit-equal; the operator counters differ by ``counter`` alone, which counts
    ``calls_expected`` launches with the calls and none without; the same ``_fm_*`` notes sit on the flow, depth and weight tensors; FusedAdam did
    the same work; and extrinsics handed out unevaluated are still unevaluated after every call between forward and backward.  (With the
    depth update inside the flow pass ``depth.grad`` is defined at the sparse pixels of the other operators only —
    FusedAdam.fuse_depth_update — and the rest of the buffer is whatever the allocator left: there dL/ddepth is compared through the depth
    parameter it moved, and element for element in the run with the separate update.)  -> (moved, base): the counters of the two runs
    without ``counter``, for the module's own assertions."""
    assert len(with_calls.history) == len(plain.history)
    for step, (a, b) in enumerate(zip(with_calls.history, plain.history)):
        assert a.keys() == b.keys(), f"step {step}: {sorted(a)} vs {sorted(b)}"
        for what in a:
            x, y = a[what], b[what]
            assert (x is None) == (y is None), f"step {step}: {what}"
            if x is not None:
                assert torch.equal(x, y), f"step {step}: {what} differs (max |diff| {float((x.double() - y.double()).abs().max()):.3e})"
    assert with_calls.params.keys() == plain.params.keys()
    for name, x in with_calls.params.items():
        assert torch.equal(x, plain.params[name]), f"{name} after {len(plain.history)} steps differs"
    moved, base = dict(with_calls.moved), dict(plain.moved)
    assert moved.pop(counter) == calls_expected and base.pop(counter) == 0
    assert moved == base, (moved, base)
    assert not plain.lazy_kept and len(with_calls.lazy_kept) == len(with_calls.history)
    assert all(after == was for was, after in with_calls.lazy_kept), "a LazyExtrinsics was left evaluated"
    assert with_calls.notes == plain.notes, (with_calls.notes, plain.notes)
    assert with_calls.state == plain.state, (with_calls.state, plain.state)
    return moved, base
