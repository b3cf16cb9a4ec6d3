"""The values that are not stored (flowmap_amd/model/projection.py: LazySurfaces, LazyWeights, LazyExtrinsics over _LazyValue): the tensor
protocol they share, ``peek()`` — the value for one call, with nothing kept and no note left — the kernel input of the weights, and
LossTracking.residuals as a reader that only reads.  The cases here take a device; tests/test_hostsim_lazy_values.py runs them on the
serial host double of the C ABI, tests/test_gpu_lazy_values.py on the MI355X.

Shapes: b = 1, f = 3, h = 4, w = 5 — the protocol is Python, so the smallest tensors the kernels accept; the pose chain at 1, 3 and 257
poses (pose_chain_fwd_kernel gives a thread a run of consecutive poses: at 257 one thread walks two and others none); the tracking case on
cases._small_problem (f = 5, 24 x 32, 60 points).  Every comparison is bit for bit: the two sides run the same launch on the same inputs.
"""

from __future__ import annotations

import itertools

import torch

from oracle import flowmap_oracle as orc

B, F, H, W = 1, 3, 4, 5
KINDS = ("surfaces", "weights", "extrinsics")
POSE_COUNTS = (1, 3, 257)
WANTED = "_fm_extrinsics_wanted"


def relative_poses(count, seed=0):
    """(1, count, 4, 4) rigid transformations near the identity, and their inverses."""
    g = torch.Generator().manual_seed(seed)
    twist = torch.zeros((count, 4, 4), dtype=torch.float64)
    omega = 0.02 * torch.randn((count, 3), generator=g, dtype=torch.float64)
    twist[:, 0, 1], twist[:, 0, 2], twist[:, 1, 2] = -omega[:, 2], omega[:, 1], -omega[:, 0]
    twist[:, 1, 0], twist[:, 2, 0], twist[:, 2, 1] = omega[:, 2], -omega[:, 1], omega[:, 0]
    twist[:, :3, 3] = 0.05 * torch.randn((count, 3), generator=g, dtype=torch.float64)
    rel = torch.linalg.matrix_exp(twist)
    return rel.float()[None].contiguous(), torch.linalg.inv(rel).float()[None].contiguous()


def make(kind, dev, poses=F - 1, sensitivity=100.0, lazy_slices=True, seed=0):
    """A lazy value of ``kind`` over leaves that require a gradient (a training step's); ``extrinsics`` with a flow tensor attached."""
    from flowmap_amd.model import projection as fm

    g = torch.Generator().manual_seed(seed)
    if kind == "surfaces":
        depths = (1.0 + torch.rand((B, F, H, W), generator=g)).to(dev).requires_grad_(True)
        k = orc.focal_to_k(torch.tensor(0.9), (H, W)).expand(B, F, 3, 3).contiguous().to(dev).requires_grad_(True)
        return fm.LazySurfaces(depths, k)
    if kind == "weights":
        logits = (0.01 * torch.randn((B, F - 1, H, W), generator=g)).to(dev).requires_grad_(True)
        return fm.LazyWeights(logits, sensitivity, lazy_slices)
    rel, rel_inv = relative_poses(poses, seed)
    flow = torch.zeros((B, poses, H, W, 2), device=dev)
    return fm.LazyExtrinsics(rel.to(dev).requires_grad_(True), rel_inv.to(dev), flow)


SOURCES = {"LazySurfaces": "depths", "LazyWeights": "logits", "LazyExtrinsics": "_rel"}  # the tensor a value's device and dtype are read from


def source(value):
    return value.__dict__[SOURCES[type(value).__name__]]


def untouched(value):
    """Nothing was evaluated and, for extrinsics, no note was left on the flow tensor."""
    flow = value.__dict__.get("_flow_tensor")
    return value._dense is None and (flow is None or WANTED not in flow.__dict__)


# ---- case 1: the protocol -----------------------------------------------------------------------------------------------------------------


def case_metadata(dev, kind):
    value = make(kind, dev)
    seen = (value.shape, value.device, value.dtype, value.ndim, value.dim(), value.size(), [value.size(i) for i in range(-value.ndim, value.ndim)])
    assert untouched(value), f"{kind}: reading the metadata evaluated it"
    dense = value.materialize()
    want = (dense.shape, dense.device, dense.dtype, dense.ndim, dense.dim(), dense.size(), [dense.size(i) for i in range(-dense.ndim, dense.ndim)])
    assert seen == want, f"{kind}: {seen} vs {want}"
    assert isinstance(seen[0], torch.Size) and value._dense is dense and value.materialize() is dense


def case_frame_slices(dev):
    from flowmap_amd.model import projection as fm

    surfaces = make("surfaces", dev)
    part = surfaces[:, 0:2]
    assert isinstance(part, fm.LazySurfaces) and part.shape == (B, 2, H, W, 3) and untouched(surfaces) and untouched(part)
    assert torch.equal(part.materialize(), surfaces.materialize()[:, 0:2])
    weights = make("weights", dev, lazy_slices=True)
    part = weights[:, 0:2]
    assert isinstance(part, fm.LazyWeights) and part.shape == (B, 2, H, W) and part.sensitivity == 100.0 and untouched(weights) and untouched(part)
    eager = make("weights", dev, lazy_slices=False)
    part = eager[:, 0:2]
    assert torch.is_tensor(part) and eager._dense is None, "the sigmoid of the frames asked for, not of the whole tensor"
    assert torch.equal(part, eager.materialize()[:, 0:2]) and torch.equal(eager[:, 0:2], part)
    assert torch.is_tensor(surfaces[0, 1]) and torch.is_tensor(weights[0]) and weights._dense is not None


def case_mixed_torch_function(dev, first, second):
    a, b = make(first, dev, seed=1), make(second, dev, seed=2)
    assert torch.result_type(a, b) == torch.float32
    assert a._dense is not None and b._dense is not None, f"result_type({first}, {second}) left one unevaluated"
    c = make(first, dev, seed=3)
    assert torch.result_type(tensor=c, other=1.0) == torch.float32 and c._dense is not None  # (keyword arguments are converted too)


def case_like_functions_of_weights(dev):
    weights = make("weights", dev)
    for like, want in ((torch.zeros_like, 0.0), (torch.ones_like, 1.0)):
        out = like(weights)
        assert out.shape == (B, F - 1, H, W) and out.dtype == torch.float32 and not out.requires_grad and bool((out == want).all())
    assert torch.empty_like(weights).shape == (B, F - 1, H, W) and torch.zeros_like(weights, dtype=torch.float64).dtype == torch.float64
    assert untouched(weights), "zeros_like / ones_like / empty_like ask for the shape only"


def case_reference_dispatch(dev, kind):
    from flowmap_amd import _reference

    value = make(kind, dev)
    assert _reference._first_tensor(value) is source(value) and _reference._first_tensor([value]) is source(value)
    assert _reference.on_host(value) is False  # (with the host double its input is the double's; on the GPU the value is on the GPU)
    assert untouched(value), f"{kind}: asking for its device evaluated it"


def case_source_is_named(dev, kind):
    """Every class names its source tensor in ``_fm_lazy`` and shares the one base.  (LazySurfaces did not name it before there was a base.)"""
    from flowmap_amd.model import projection as fm

    value = make(kind, dev)
    assert isinstance(value, fm._LazyValue) and type(value)._fm_lazy == SOURCES[type(value).__name__]
    assert value.device == source(value).device and value.dtype == source(value).dtype and untouched(value)


# ---- case 2: peek() -----------------------------------------------------------------------------------------------------------------------


def check_peek(value, what):
    first = value.peek()
    assert untouched(value), f"{what}: peek() kept the value or left a note"
    assert torch.is_tensor(first) and not first.requires_grad and first.grad_fn is None
    dense = value.materialize()
    assert dense.requires_grad, f"{what}: the evaluated value carries the gradient of its leaves"
    assert torch.equal(first, dense.detach()), f"{what}: peek() differs from materialize()"
    assert tuple(first.shape) == tuple(value.shape) and torch.equal(value.peek(), first)
    again = value.peek()
    assert again.data_ptr() == dense.data_ptr() and not again.requires_grad, f"{what}: after materialize() peek() is the cached tensor, detached"
    return first


def case_peek_extrinsics(dev, poses):
    from flowmap_amd.model import projection as fm

    value = make("extrinsics", dev, poses=poses)
    chain = check_peek(value, f"extrinsics of {poses} poses")
    assert chain.shape == (B, poses + 1, 4, 4) and value._flow_tensor.__dict__[WANTED] is True  # (materialize() does leave the note)
    want = torch.eye(4, dtype=torch.float64)
    for i, factor in enumerate(value._rel.detach().cpu().double()[0]):  # P_0 = I, P_k = P_{k-1}·T_{k-1} (flowmap/model/projection.py:187-210)
        assert (chain[0, i].cpu().double() - want).abs().max() < 1e-4 * max(1.0, float(want.abs().max())), f"pose {i} of {poses}"
        want = want @ factor
    plain = torch.eye(4, device=dev).repeat(B, 2, 1, 1).requires_grad_(True)
    peeked = fm._peek_extrinsics(plain)
    assert torch.is_tensor(peeked) and not peeked.requires_grad and peeked.data_ptr() == plain.data_ptr()
    fresh = make("extrinsics", dev, poses=poses)
    assert torch.equal(fm._peek_extrinsics(fresh), chain) and untouched(fresh)


def case_peek_surfaces_and_weights(dev):
    check_peek(make("surfaces", dev), "surfaces")
    for sensitivity in (100.0, 0.0):
        value = check_peek(make("weights", dev, sensitivity=sensitivity), f"weights at sensitivity {sensitivity}")
        assert sensitivity != 0.0 or bool((value == 0.5).all())


# ---- case 3: the kernel input of the weights ----------------------------------------------------------------------------------------------


def case_kernel_input(dev):
    weights = make("weights", dev, sensitivity=100.0)
    tensor, sensitivity = weights.kernel_input()
    assert tensor.data_ptr() == weights.logits.data_ptr() and tensor.shape == weights.logits.shape and sensitivity == 100.0 and untouched(weights)
    kept, _ = weights.kernel_input(keep=True)
    assert kept is weights.logits and untouched(weights), "at a sensitivity other than 0 the kernels read the logits: nothing to keep"
    flat = make("weights", dev, sensitivity=0.0)
    tensor, sensitivity = flat.kernel_input()
    assert sensitivity == 0.0 and flat._dense is None and not tensor.requires_grad
    assert torch.equal(tensor, (0.0 * flat.logits.detach()).sigmoid()) and torch.equal(tensor, flat.materialize().detach())
    training = make("weights", dev, sensitivity=0.0)
    tensor, sensitivity = training.kernel_input(keep=True)  # what a training step takes: differentiable, evaluated once
    assert sensitivity == 0.0 and tensor is training._dense and tensor.requires_grad


# ---- case 4: LossTracking.residuals only reads ----------------------------------------------------------------------------------------------

RESIDUAL_FIELDS = ("residual", "visible", "xy_target", "pair_sum", "pair_count", "track_sum", "track_count")


def case_tracking_residuals_only_read(dev):
    """After LossTracking.residuals the LazyExtrinsics of a flow-only step is still unevaluated, the backward flows carry no note that the
    chain is wanted, and the optimisation's next steps still hand out the chain unevaluated; every returned field is bit-equal to the same
    call on an output whose chain was evaluated first."""
    import cases
    import flowmap_amd
    from flowmap_amd import ModelOutput
    from flowmap_amd.loss import LossTracking, LossTrackingCfg
    from flowmap_amd.model.projection import LazyExtrinsics
    from helpers import mapping_cfg, to_tracks
    from operator_checks import same_tensors

    f, h, w = 5, 24, 32
    try:
        model, batch, flows, loss_of = cases._small_problem(dev, tracking=False)
        flows.backward.__dict__.pop(WANTED, None)
        tracks = to_tracks(orc.synth_tracks(f, h, w, seed=0, interval=2, radius=2, grid=4), dev)
        loss = LossTracking(LossTrackingCfg(0, 100.0, "tracking", mapping_cfg("huber")))
        model.train()
        out = model(batch, flows, 0)
        assert isinstance(out.extrinsics, LazyExtrinsics) and out.extrinsics._dense is None, "a flow-only step hands out the chain unevaluated"
        got = loss.residuals(batch, tracks, out, predicted=True)
        assert out.extrinsics._dense is None, "LossTracking.residuals evaluated the LazyExtrinsics"
        assert WANTED not in flows.backward.__dict__, "LossTracking.residuals asked the optimisation's later steps for the chain"
        loss_of(out).backward()
        for step in (1, 2):  # the next two training steps
            model.zero_grad(set_to_none=True)
            later = model(batch, flows, step)
            assert isinstance(later.extrinsics, LazyExtrinsics) and later.extrinsics._dense is None, f"step {step}: the fit chained the poses itself"
            loss_of(later).backward()
        # a second output of the SAME fit whose chain is evaluated first.  (Not a second forward: on the GPU the fit takes its planned
        # path once the same indices and flows have come back, and its poses may then differ from the first forward's in the last bit.)
        chain = LazyExtrinsics(out.extrinsics._rel, out.extrinsics._fm_relative_poses[0]).materialize()
        second = ModelOutput(out.depths, out.surfaces, out.intrinsics, chain, out.backward_correspondence_weights)
        want = loss.residuals(batch, tracks, second, predicted=True)
        assert out.extrinsics._dense is None and WANTED not in flows.backward.__dict__
        assert len(got) == len(want) == len(tracks) > 1
        for a, b in zip(got, want):
            assert not a.residual.requires_grad and int(a.visible.sum()) > 0
            same_tensors(a, b, RESIDUAL_FIELDS, f"segment {a.segment}: ", scalars=("segment", "start_frame"))
    finally:
        flowmap_amd.set_lazy_surfaces(False)


PAIRS = tuple(itertools.product(KINDS, KINDS))
