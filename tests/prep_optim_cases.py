"""The seven kernels around the step — fm_preprocess.hip (consistency mask, fused flow post-processing, resize + crop) and
fm_optim.hip (Adam, capturable Adam, Adam on an element list, zero fill) — at every edge of their launch geometry.  Shared by the
CPU (host double) and GPU modules; the host double runs the same per-element functions in plain loops, so only the GPU module says
anything about grids, strides, vector bodies and tails.

Truth is always a plain fp64 evaluation (F.interpolate + slice, the oracle's consistency_mask / bidirectional_flows on .double()
inputs, the textbook Adam formulas), ``ref32`` the same formula in torch fp32 on the CPU — the reference's own arithmetic.  The
gate (``gate``) holds ours, norm-wise (relerr) AND element-wise (maxerr), to max(floor, 2 x ref32's own measured error), with the
floors the project already holds these operators to (FLOOR_*).  Every figure is printed before it is asserted.

Outputs and in-place buffers are carved out of the middle of a larger allocation (``Carved``): guard bands of GUARD floats on
each side hold a finite pattern that is checked bit for bit after the call, outputs are pre-filled with a sentinel no correct
result equals, inputs are compared bit for bit with what went in.  Unaligned pointers are reached through the C ABI with
``data_ptr() + 4·k`` inside a live tensor."""

from __future__ import annotations

import json
import math
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import flowmap_oracle as orc

G = 1 << 20  # elements of one grid pass of the Adam kernels (1024 blocks x 256 threads x 4) and pixels of one pass of the flow kernels (4096 x 256)
GUARD = 64  # floats of guard band on each side (a multiple of 4: the carved view keeps the allocation's 16-byte alignment)
SENTINEL = -777.25

FLOOR_CROP = 2e-6  # cases.case_cropping
FLOOR_FLOW = 2e-5  # cases.case_flow_preprocess
FLOOR_ADAM = 2e-6  # cases.case_fused_adam: parameters (with ABS_ADAM_PARAM) and both moments
ABS_ADAM_PARAM = 1e-7
CAPTURABLE_REL, CAPTURABLE_ABS = 1e-6, 1e-8  # cases.case_capturable_pieces: capturable against the host-step kernel
SLACK = 2.0  # conftest.assert_close_or_reference_gap

FULL_SIZE = os.environ.get("FLOWMAP_SKIP_FULL_SIZE") != "1"


def full_size(*cfgs):
    """Production-size cases (GPU module only): skipped under FLOWMAP_SKIP_FULL_SIZE=1 like tests/test_gpu_full_size.py."""
    return [pytest.param(c, marks=pytest.mark.skipif(not FULL_SIZE, reason="FLOWMAP_SKIP_FULL_SIZE=1")) for c in cfgs]


# ---- buffers, errors, the gate ---------------------------------------------------------------------------------------------


def bits(x):
    return x.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b.to(a.device)))


class Carved:
    """``numel`` floats in the middle of a larger allocation on ``dev``, ``shift`` floats (0..3) past a 16-byte boundary."""

    def __init__(self, numel, dev, shift=0, fill=SENTINEL):
        assert 0 <= shift < 4
        self.numel, self.start = int(numel), GUARD + shift
        total = self.numel + 2 * GUARD + 4
        self.pattern = 1000.0 + (torch.arange(total) % 251).float()
        self.buf = self.pattern.clone().to(dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.start : self.start + self.numel]
        if fill is not None:
            self.view.fill_(fill)

    def set(self, values):
        self.view.copy_(values.reshape(-1))
        return self

    @property
    def ptr(self):  # (an empty view has no data_ptr of its own)
        return self.buf.data_ptr() + 4 * self.start

    def cpu(self, shape=None):
        out = self.view.detach().cpu().clone()
        return out if shape is None else out.reshape(shape)

    def check_guards(self, what):
        end = self.start + self.numel
        assert same_bits(self.buf[: self.start].cpu(), self.pattern[: self.start]), f"{what}: written below the buffer"
        assert same_bits(self.buf[end:].cpu(), self.pattern[end:]), f"{what}: written past the buffer"


def stream(dev):
    return torch.cuda.current_stream(torch.device(dev)).cuda_stream if str(dev).startswith("cuda") else None


def errors(a, b):
    """(conftest.relerr, conftest.maxerr, max|a-b|) in one pass, on the device the operands live on."""
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    if b.numel() == 0:
        return 0.0, 0.0, 0.0
    diff = a - b
    num, den = diff.norm().item(), b.norm().item()
    mx, mden = diff.abs().max().item(), b.abs().max().item()
    return (num / den if den > 1e-30 else num), (mx / mden if mden > 1e-30 else mx), mx


RECORDS = []


def emit(record, warn=False):
    """The record of one comparison, as tests/test_gpu_full_size.py emits its own: printed, appended to $FLOWMAP_PARITY_RECORD
    when that is set, and (production-size cases) raised as a UserWarning so that pytest's summary keeps it."""
    print(record, flush=True)
    RECORDS.append(record)
    if warn:
        warnings.warn("prep/optim parity record: " + json.dumps(record))
    out = os.environ.get("FLOWMAP_PARITY_RECORD")
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(record) + "\n")


def gate(what, ours, truth, ref32, floor, abs_=0.0, warn=False):
    """ours against the fp64 truth, norm-wise and element-wise: at most max(floor, SLACK x the fp32 evaluation's own error), both
    measured here.  ``abs_``: the absolute tolerance the project's gate for this operator carries beside the relative one
    (conftest.assert_close's ``abs_``).  Where the truth is not finite ours must be non-finite at the same elements, and
    NaN where the truth is NaN; the errors are taken over the rest."""
    assert ours.shape == truth.shape == ref32.shape, f"{what}: shapes {tuple(ours.shape)} / {tuple(truth.shape)} / {tuple(ref32.shape)}"
    truth, ref32 = truth.to(ours.device), ref32.to(ours.device)
    finite = torch.isfinite(truth)
    if not bool(finite.all()):
        assert torch.equal(torch.isfinite(ours), finite), f"{what}: non-finite at {int((~torch.isfinite(ours)).sum())} elements, the reference at {int((~finite).sum())}"
        # (an element that is ±inf in the reference may be NaN in ours: at the clamped last row / column both resize taps are the
        # same pixel and ours weighs the second with an exact 0)
        assert bool(torch.isnan(ours[torch.isnan(truth)]).all()), f"{what}: the reference is NaN where ours is ±inf"
        finite = finite & torch.isfinite(ref32)
        ours, truth, ref32 = ours[finite], truth[finite], ref32[finite]
    assert bool(torch.isfinite(ours).all()), f"{what}: {int((~torch.isfinite(ours)).sum())} non-finite elements where the reference is finite"
    rel, mx, mabs = errors(ours, truth)
    rel32, mx32, _ = errors(ref32, truth)
    emit({"what": what, "n": int(truth.numel()), "rel": rel, "rel_fp32": rel32, "max": mx, "max_fp32": mx32, "max_abs": mabs}, warn)
    if abs_ > 0 and mabs <= abs_:
        return
    assert rel <= max(floor, SLACK * rel32), f"{what}: rel err {rel:.3e} > max({floor:.1e}, {SLACK} x fp32 gap {rel32:.3e})"
    assert mx <= max(floor, SLACK * mx32), f"{what}: max-abs err {mx:.3e} of max|ref| > max({floor:.1e}, {SLACK} x fp32 gap {mx32:.3e})"


def abi(name, *args):
    from flowmap_amd._lib import call

    call(name, *args)


def refused(name, *args):
    """The entry point returns the argument error (and, checked by the caller, writes nothing)."""
    with pytest.raises(RuntimeError, match="invalid argument"):
        abi(name, *args)


# ---- Adam ------------------------------------------------------------------------------------------------------------------

COUNTS = (0, 1, 3, 4, 5, 1023, 1024, 1025, G - 1, G, G + 1, G + 5, 3 * G + 7)
COUNTS_FULL_SIZE = (150 * 720 * 1280, 149 * 720 * 1280 + 3)
HYPER = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0)
STEPS = (1, 2, 1000, 100000)


def hyper(**changes):
    return {**HYPER, **changes}


def adam_state(count, seed, dev="cpu"):
    """(p, g, m, v): parameters 1e-3 .. 1e3 and gradients 1e-12 .. 1e4 (log-uniform, either sign) in one tensor, moments of the
    gradient's order of magnitude."""
    gen = torch.Generator(device=dev).manual_seed(seed)

    def rand():
        return torch.rand((count,), generator=gen, device=dev)

    def sign():
        return torch.where(rand() < 0.5, -1.0, 1.0)

    p = sign() * 10.0 ** (rand() * 6 - 3)
    g = sign() * 10.0 ** (rand() * 16 - 12)
    m = g * (rand() * 2 - 1)
    v = (g * rand()) ** 2
    return p, g, m, v


def adam_reference(state, step, h, dtype):
    """One textbook Adam step (torch.optim.Adam: L2 weight decay, no amsgrad) from the fp32 state, evaluated in ``dtype``."""
    p, g, m, v = (x.to(dtype) for x in state)
    bc1, bc2 = 1.0 - h["b1"] ** step, 1.0 - h["b2"] ** step
    if h["wd"] != 0:
        g = g + h["wd"] * p
    m = h["b1"] * m + (1.0 - h["b1"]) * g
    v = h["b2"] * v + (1.0 - h["b2"]) * g * g
    p = p - (h["lr"] / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + h["eps"]))
    return p, m, v


def run_adam(dev, state, step, h, kernel="host", shifts=(0, 0, 0, 0), elements=None, what="adam"):
    """One launch of fm_adam_step / _capturable / _elements on carved copies of ``state`` -> (p, m, v) on the state's device.
    Guard bands of all four buffers and every bit of the gradient are checked."""
    count = state[0].numel()
    p, g, m, v = (Carved(count, dev, s).set(x) for x, s in zip(state, shifts))
    tail = (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], stream(dev))
    if kernel == "host":
        abi("fm_adam_step", p.ptr, g.ptr, m.ptr, v.ptr, count, step, *tail)
    elif kernel == "capturable":
        step_t = torch.full((1,), float(step), device=dev)
        abi("fm_adam_step_capturable", p.ptr, g.ptr, m.ptr, v.ptr, count, step_t.data_ptr(), *tail)
    else:
        el = elements.to(dev)
        abi("fm_adam_step_elements", p.ptr, g.ptr, m.ptr, v.ptr, el.data_ptr() if el.numel() else None, el.numel(), step, *tail)
        assert torch.equal(el.cpu(), elements.cpu()), f"{what}: the element list was written to"
    for name, c in (("param", p), ("grad", g), ("exp_avg", m), ("exp_avg_sq", v)):
        c.check_guards(f"{what}: {name}")
    assert same_bits(g.view, state[1]), f"{what}: the gradient was written to"
    back = state[0].device
    return tuple(c.view.detach().clone().to(back) for c in (p, m, v))


def gate_adam(what, ours, state, step, h, warn=False):
    truth = adam_reference(state, step, h, torch.float64)
    ref32 = adam_reference(tuple(x.cpu() for x in state), step, h, torch.float32)
    assert all(bool(torch.isfinite(x).all()) for x in truth), f"{what}: the fp64 truth is not finite"
    gate(f"{what} param", ours[0], truth[0], ref32[0], FLOOR_ADAM, ABS_ADAM_PARAM, warn)
    gate(f"{what} exp_avg", ours[1], truth[1], ref32[1], FLOOR_ADAM, warn=warn)
    gate(f"{what} exp_avg_sq", ours[2], truth[2], ref32[2], FLOOR_ADAM, warn=warn)


def case_adam_count(dev, count, kernel="host"):
    """Every count around the quad, the block and the grid pass: body, tail and grid-stride loop, every element compared."""
    state = adam_state(count, seed=count % 1000)
    ours = run_adam(dev, state, 3, HYPER, kernel, what=f"adam[{kernel}] n={count}")
    if count:
        gate_adam(f"adam[{kernel}] n={count}", ours, state, 3, HYPER)


def case_adam_full_size(dev, count):
    """Production sizes (depth: 150 x 720 x 1280): state and fp64 truth on the GPU, the fp32 evaluation on the host."""
    state = adam_state(count, seed=11, dev=dev)
    ours = run_adam(dev, state, 7, HYPER, "host", what=f"adam n={count}")
    gate_adam(f"adam n={count}", ours, state, 7, HYPER, warn=True)
    del ours
    shifted = run_adam(dev, state, 7, HYPER, "capturable", what=f"adam[capturable] n={count}")
    gate_adam(f"adam[capturable] n={count}", shifted, state, 7, HYPER, warn=True)


ALIGNMENTS = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1), (3, 2, 1, 0))
ALIGN_COUNTS = (5, 1025, G + 5)


def case_adam_alignment(dev, count, kernel):
    """A pointer that is not 16-byte aligned selects the scalar path (vec_ok = 0; under frame sharding p[frame] with H·W % 4 != 0):
    the same adam_update runs per element, so the result equals the aligned run bit for bit."""
    state = adam_state(count, seed=5)
    for wd in (0.0, 0.01):
        aligned = run_adam(dev, state, 2, hyper(wd=wd), kernel, what=f"adam[{kernel}] n={count} aligned")
        gate_adam(f"adam[{kernel}] n={count} wd={wd} aligned", aligned, state, 2, hyper(wd=wd))
        for shifts in ALIGNMENTS:
            got = run_adam(dev, state, 2, hyper(wd=wd), kernel, shifts, what=f"adam[{kernel}] n={count} shifts={shifts}")
            for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, aligned):
                assert same_bits(a, b), f"adam[{kernel}] n={count} wd={wd} shifts={shifts}: {name} differs from the aligned run at {int((bits(a) != bits(b)).sum())} elements"


def zero_pattern_state(count, seed=3):
    """Quads with 0, 1, 3 and 4 elements having g = m = v = 0 (cycling), a fifth kind of quad with g = 0 but m, v != 0."""
    p, g, m, v = adam_state(count, seed)
    i = torch.arange(count)
    quad, lane = (i // 4) % 5, i % 4
    idle = ((quad == 1) & (lane == 2)) | ((quad == 2) & (lane != 1)) | (quad == 3)
    g[idle], m[idle], v[idle] = 0.0, 0.0, 0.0
    g[quad == 4] = 0.0
    return (p, g, m, v), idle, quad == 4


ZERO_COUNTS = (43, 4 * 5 * 300 + 3, G + 5)


def case_adam_zero_patterns(dev, count, kernel):
    state, idle, decaying = zero_pattern_state(count)
    what = f"adam[{kernel}] zero patterns n={count}"
    for shifts in ((0, 0, 0, 0), (0, 0, 1, 0)):  # the skipping vector body, and the scalar path that never skips
        ours = run_adam(dev, state, 4, HYPER, kernel, shifts, what=what)
        gate_adam(f"{what} shifts={shifts}", ours, state, 4, HYPER)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), ours, (state[0], state[2], state[3])):
            assert same_bits(a[idle], b[idle]), f"{what}: {name} of an idle element (g = m = v = 0) changed"
        live = decaying & (state[2] != 0) & (state[3] != 0)  # g = 0 but m, v != 0: both moments decay (the gate above says by how much)
        assert int(live.sum()) > 0 and bool((ours[1][live] != state[2][live]).all() and (ours[2][live] != state[3][live]).all()), f"{what}: g = 0, m, v != 0 must decay"
        # with weight decay nothing is idle: a zero-gradient element moves like any other
        wd = hyper(wd=0.01)
        ours = run_adam(dev, state, 4, wd, kernel, shifts, what=what + " wd")
        gate_adam(f"{what} wd shifts={shifts}", ours, state, 4, wd)
        assert bool((ours[0][idle] != state[0][idle]).all()), f"{what}: weight decay must move a zero-gradient element"
        assert bool((ours[1][idle] != 0).all() and (ours[2][idle] != 0).all())


MAGNITUDE_HYPERS = (("plain", {}), ("lr0", dict(lr=0.0)), ("beta1_0", dict(b1=0.0)), ("beta2_0", dict(b2=0.0)), ("betas_0", dict(b1=0.0, b2=0.0)),
                    ("wd", dict(wd=0.1)), ("big_eps", dict(eps=1e-3)))


def case_adam_magnitudes(dev, step, name, changes, kernel="host", count=4099):
    """Gradients 1e-12 .. 1e4 and parameters 1e-3 .. 1e3 in one tensor (adam_state), at steps whose bias corrections run from
    1e-3 to 1, with lr = 0 and betas at 0."""
    h = hyper(**changes)
    state = adam_state(count, seed=step % 97)
    ours = run_adam(dev, state, step, h, kernel, what=f"adam[{kernel}] {name} step={step}")
    gate_adam(f"adam[{kernel}] {name} step={step}", ours, state, step, h)
    if h["lr"] == 0:
        assert same_bits(ours[0], state[0]), "lr = 0 moved a parameter"


TRAJECTORY_COUNTS = (G + 5, 3 * G + 7)


def case_adam_trajectory(dev, count, steps=6):
    """The host-step kernel and the capturable kernel (step number read from device memory) over the same gradients, against
    torch.optim.Adam in fp64 (and in fp32: the gap); one third of the elements never see a gradient."""
    gen = torch.Generator().manual_seed(count % 1000)
    init = torch.randn((count,), generator=gen)
    grads = [torch.randn((count,), generator=gen) * 10.0 ** (k % 3 - 1) for k in range(steps)]
    never = torch.arange(count) % 3 == 1
    for gr in grads:
        gr[never] = 0.0
    refs = {}
    for dtype in (torch.float64, torch.float32):
        q = init.to(dtype).clone().requires_grad_(True)
        opt = torch.optim.Adam([q], lr=HYPER["lr"], betas=(HYPER["b1"], HYPER["b2"]), eps=HYPER["eps"])
        for gr in grads:
            q.grad = gr.to(dtype)
            opt.step()
        refs[dtype] = (q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"])
    runs = {}
    tail = (HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], 0.0, stream(dev))
    for kernel in ("host", "capturable"):
        p, m, v = Carved(count, dev).set(init), Carved(count, dev).set(torch.zeros(count)), Carved(count, dev).set(torch.zeros(count))
        step_t = torch.zeros((1,), device=dev)
        for k, gr in enumerate(grads):
            g = Carved(count, dev).set(gr)
            if kernel == "host":
                abi("fm_adam_step", p.ptr, g.ptr, m.ptr, v.ptr, count, k + 1, *tail)
            else:
                step_t += 1
                abi("fm_adam_step_capturable", p.ptr, g.ptr, m.ptr, v.ptr, count, step_t.data_ptr(), *tail)
            assert same_bits(g.view, gr)
        for c in (p, m, v):
            c.check_guards(f"adam[{kernel}] trajectory n={count}")
        runs[kernel] = (p.cpu(), m.cpu(), v.cpu())
        what = f"adam[{kernel}] trajectory n={count}"
        gate(f"{what} param", runs[kernel][0], refs[torch.float64][0], refs[torch.float32][0], FLOOR_ADAM, ABS_ADAM_PARAM)
        gate(f"{what} exp_avg", runs[kernel][1], refs[torch.float64][1], refs[torch.float32][1], FLOOR_ADAM)
        gate(f"{what} exp_avg_sq", runs[kernel][2], refs[torch.float64][2], refs[torch.float32][2], FLOOR_ADAM)
        assert same_bits(runs[kernel][0][never], init[never]), f"{what}: an element that never saw a gradient moved"
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), runs["capturable"], runs["host"]):
        rel, mx, mabs = errors(a, b)
        print(f"[capturable vs host-step n={count}] {name}: rel {rel:.2e} max {mx:.2e} max-abs {mabs:.2e}", flush=True)
        assert rel <= CAPTURABLE_REL or mabs <= CAPTURABLE_ABS, f"capturable vs host-step n={count}: {name} rel {rel:.3e} (max-abs {mabs:.3e})"


def case_adam_capturable_step_tensor(dev, count=G + 5):
    """A step tensor changed between two launches is honoured: (1, then 1000) equals the host-step kernel at (1, then 1000)."""
    state = adam_state(count, seed=9)
    tail = (HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], 0.0, stream(dev))
    out = {}
    for kernel in ("host", "capturable"):
        p, g, m, v = (Carved(count, dev).set(x) for x in state)
        step_t = torch.ones((1,), device=dev)
        for step in (1, 1000):
            if kernel == "host":
                abi("fm_adam_step", p.ptr, g.ptr, m.ptr, v.ptr, count, step, *tail)
            else:
                step_t.fill_(float(step))
                abi("fm_adam_step_capturable", p.ptr, g.ptr, m.ptr, v.ptr, count, step_t.data_ptr(), *tail)
        out[kernel] = (p.cpu(), m.cpu(), v.cpu())
    once = run_adam(dev, state, 1, HYPER, "host")
    twice_at_1 = run_adam(dev, (once[0], state[1], once[1], once[2]), 1, HYPER, "host")
    assert not torch.equal(out["host"][0], twice_at_1[0])  # (the step number matters on this state)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), out["capturable"], out["host"]):
        rel, _, mabs = errors(a, b)
        print(f"[capturable step tensor 1 -> 1000] {name}: rel {rel:.2e} max-abs {mabs:.2e}", flush=True)
        assert rel <= CAPTURABLE_REL or mabs <= CAPTURABLE_ABS, f"capturable step tensor: {name} rel {rel:.3e}"


ELEMENT_LENGTHS = (0, 1, 255, 256, 257, 10**6)


def case_adam_elements(dev, length):
    """fm_adam_step_elements on an unsorted list of unique elements that contains element 0 and the last one: listed elements
    against the truth, every unlisted element of p, m and v bit-identical."""
    count = 1 if length == 1 else 2 * length + 3
    gen = torch.Generator().manual_seed(length)
    if length < 2:
        elements = torch.zeros((length,), dtype=torch.int64)  # (length 1: one parameter, element 0 is the last one)
    else:
        middle = 1 + torch.randperm(count - 2, generator=gen)[: length - 2]
        elements = torch.cat([middle, torch.tensor([0, count - 1])])
        elements = elements[torch.randperm(length, generator=gen)]
        assert bool((elements == 0).any()) and bool((elements == count - 1).any()) and not torch.equal(elements, elements.sort().values)
    assert elements.numel() == length and elements.unique().numel() == length
    state = adam_state(count, seed=length % 89)
    ours = run_adam(dev, state, 5, HYPER, "elements", elements=elements, what=f"adam elements len={length}")
    listed = torch.zeros((count,), dtype=torch.bool)
    listed[elements] = True
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), ours, (state[0], state[2], state[3])):
        assert same_bits(a[~listed], b[~listed]), f"adam elements len={length}: an unlisted element of {name} changed"
    if length:
        sub = tuple(x[listed] for x in state)
        gate_adam(f"adam elements len={length}", tuple(x[listed] for x in ours), sub, 5, HYPER)


FILL_BLOCKS = (1, 7, 4096)


def case_fill_zero(dev, count, blocks):
    x = Carved(count, dev)
    abi("fm_fill_zero", x.ptr, count, blocks, stream(dev))
    x.check_guards(f"fill n={count} blocks={blocks}")
    got = x.cpu()
    assert same_bits(got, torch.zeros(count)), f"fill n={count} blocks={blocks}: {int((bits(got) != 0).sum())} elements are not +0.0"


def case_fill_zero_misaligned(dev):
    for shift in (1, 2, 3):
        x = Carved(1030, dev, shift)
        before = x.buf.cpu().clone()
        refused("fm_fill_zero", x.ptr, 1030, 4, stream(dev))
        assert same_bits(x.buf.cpu(), before), "a refused fill wrote to its buffer"


def case_adam_eps(dev):
    """eps must be positive: the zero-gradient shortcuts (the idle quads of the vector body, FusedAdam's element-list update and
    the in-pass depth update) rest on 0 / (0 + eps) = 0, which torch's eps = 0 turns into 0 / 0."""
    from flowmap_amd import FusedAdam

    q = torch.zeros((8,), device=dev, requires_grad=True)
    with pytest.raises(ValueError, match="eps > 0"):
        FusedAdam([q], eps=0.0)
    with pytest.raises(ValueError, match="eps > 0"):
        FusedAdam([q], eps=1e-60)  # zero once the kernels hold it in fp32
    with pytest.raises(ValueError):
        FusedAdam([q], eps=-1e-8)
    opt = FusedAdam([q], lr=1e-2)
    q.grad = torch.ones_like(q)
    opt.step()
    after = q.detach().clone()
    opt.param_groups[0]["eps"] = 0.0
    with pytest.raises(ValueError, match="eps > 0"):
        opt.step()
    assert torch.equal(q.detach(), after) and float(opt.state[q]["step"]) == 1.0  # refused before anything moved
    # the three entry points
    count = 1029
    state = adam_state(count, seed=1)
    elements = torch.arange(count - 1, -1, -3)
    for eps in (0.0, -1e-8):
        p, g, m, v = (Carved(count, dev).set(x) for x in state)
        step_t = torch.ones((1,), device=dev)
        tail = (HYPER["lr"], HYPER["b1"], HYPER["b2"], eps, 0.0, stream(dev))
        refused("fm_adam_step", p.ptr, g.ptr, m.ptr, v.ptr, count, 1, *tail)
        refused("fm_adam_step_capturable", p.ptr, g.ptr, m.ptr, v.ptr, count, step_t.data_ptr(), *tail)
        el = elements.to(dev)
        refused("fm_adam_step_elements", p.ptr, g.ptr, m.ptr, v.ptr, el.data_ptr(), el.numel(), 1, *tail)
        for c, x in zip((p, g, m, v), state):
            assert same_bits(c.view, x), "a refused Adam step wrote to its buffers"


def case_adam_eps_zero_is_one_answer(dev):
    """What the refusal prevents: with eps = 0 and g = m = v = 0 torch gives 0 / 0 = NaN; the vector body skips such quads (the
    parameter is kept) and the scalar tail does not, so one tensor would hold both answers.  Asserted through the only door
    left, the entry point: it refuses, and the tensor holds neither."""
    count = 9  # two quads and a tail element
    state = tuple(torch.zeros(count) if k else torch.ones(count) for k in range(4))
    p, g, m, v = (Carved(count, dev).set(x) for x in state)
    refused("fm_adam_step", p.ptr, g.ptr, m.ptr, v.ptr, count, 1, 1e-3, 0.9, 0.999, 0.0, 0.0, stream(dev))
    assert same_bits(p.view, state[0])


# ---- resize + crop ---------------------------------------------------------------------------------------------------------


def iid_video(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def planes_of(kind, planes, h, w, seed):
    """(planes, h, w) in [0, 1]: i.i.d. (a one-pixel misplacement shows in maxerr) or the oracle's smooth video."""
    if kind == "iid":
        return iid_video((planes, h, w), seed)
    frames = (planes + 2) // 3
    return orc.synth_video(frames, h, w, seed=seed).reshape(frames * 3, h, w)[:planes].contiguous()


def resize_reference(x, resized, origin, crop, dtype):
    full = F.interpolate(x.to(dtype)[None], tuple(resized), mode="bilinear", align_corners=False)[0]
    return full[:, origin[0] : origin[0] + crop[0], origin[1] : origin[1] + crop[1]]


# (planes, (h, w), resized (rh, rw), origin (row0, col0), crop (oh, ow), out shifts)
RESIZE_CASES = (
    (3, (5, 1), (9, 4), (1, 1), (7, 1), (0,)),  # w = 1 (1 -> n across), ow = 1
    (3, (4, 2), (17, 9), (0, 3), (17, 2), (0,)),  # w = 2, ow = 2, oh = 17
    (2, (6, 3), (24, 12), (3, 1), (8, 3), (0,)),  # x4, w = 3, ow = 3, oh = 8
    (2, (7, 4), (28, 16), (1, 5), (9, 4), (0, 1, 2)),  # x4, w = 4: the window base min(i0, w - 4) = 0; ow = 4 aligned and not
    (2, (7, 4), (7, 4), (0, 0), (7, 4), (0, 3)),  # identity at w = 4
    (2, (9, 4), (9, 16), (1, 0), (1, 16), (0,)),  # oh = 1; every window of w = 4
    (2, (3, 5), (36, 60), (5, 7), (17, 5), (0,)),  # x12, w = 5, ow = 5
    (2, (9, 5), (9, 5), (1, 0), (7, 5), (0,)),  # identity, w = 5
    (2, (1, 1), (9, 13), (1, 3), (7, 5), (0,)),  # 1 -> n both ways
    (1, (11, 260), (44, 1040), (3, 9), (9, 1023), (0,)),  # x4, one block short of a column
    (1, (11, 260), (44, 1040), (1, 7), (8, 1024), (0, 1)),  # exactly one block; 16-byte stores, and the same at an address 4 mod 16
    (1, (11, 260), (44, 1040), (1, 7), (8, 1025), (0,)),  # blockIdx.x = 1 holds one column
    (1, (11, 260), (44, 1040), (1, 11), (8, 1028), (0, 1)),  # blockIdx.x = 1 holds one quad
    (2, (5, 110), (60, 1320), (7, 15), (17, 1290), (0,)),  # x12
    (1, (9, 2100), (9, 2100), (1, 23), (7, 2052), (0, 1)),  # identity, three blocks across
    (2, (40, 53), (31, 40), (1, 1), (17, 37), (0,)),  # 53 -> 40: the window condition differs between threads of one block
    (2, (40, 53), (31, 40), (3, 0), (9, 40), (0, 2)),
    (2, (30, 2100), (9, 300), (1, 3), (7, 290), (0,)),  # 2100 -> 300: gathers seven pixels apart
    (1, (12, 2100), (9, 1050), (1, 1), (8, 1028), (0,)),  # shrinking (no window) with blockIdx.x > 0
    (1, (20, 300), (15, 1300), (3, 5), (9, 1290), (0,)),  # x4.33 across, shrinking down
)


def resize_id(c):
    return f"{c[0]}x{c[1][0]}x{c[1][1]}-to-{c[2][0]}x{c[2][1]}-at-{c[3][0]},{c[3][1]}-crop-{c[4][0]}x{c[4][1]}"


def case_resize(dev, cfg):
    planes, (h, w), resized, origin, crop, shifts = cfg
    for kind in ("iid", "smooth"):
        x = planes_of(kind, planes, h, w, seed=h * w)
        truth, ref32 = resize_reference(x, resized, origin, crop, torch.float64), resize_reference(x, resized, origin, crop, torch.float32)
        src = Carved(x.numel(), dev).set(x)
        for shift in shifts:
            out = Carved(truth.numel(), dev, shift)
            abi("fm_resize_crop", src.ptr, planes, h, w, *resized, *origin, *crop, out.ptr, stream(dev))
            what = f"resize {resize_id(cfg)} {kind} out+{shift}"
            out.check_guards(what)
            assert same_bits(src.view, x.reshape(-1)), f"{what}: the input was written to"
            got = out.cpu(truth.shape)
            assert not bool((got == SENTINEL).any()), f"{what}: {int((got == SENTINEL).sum())} output pixels were never written"
            gate(what, got, truth, ref32, FLOOR_CROP)


def case_resize_many_planes(dev, planes=70_000):
    """More planes than one launch's grid.z takes (the chunking loop of _preprocess.resize_crop), planes on either side of the
    seam singled out."""
    from flowmap_amd import _ops

    x = iid_video((planes, 2, 3), seed=7)
    resized, crop = (5, 7), (3, 4)
    origin = ((resized[0] - crop[0]) // 2, (resized[1] - crop[1]) // 2)
    assert origin == (1, 1)
    truth, ref32 = resize_reference(x, resized, origin, crop, torch.float64), resize_reference(x, resized, origin, crop, torch.float32)
    x_dev = x.to(dev)
    got = _ops.resize_crop(x_dev, resized, crop).cpu()
    assert same_bits(x_dev, x)
    gate(f"resize {planes} planes", got, truth, ref32, FLOOR_CROP)
    for plane in (0, 65534, 65535, 65536, planes - 1):
        gate(f"resize {planes} planes: plane {plane}", got[plane], truth[plane], ref32[plane], FLOOR_CROP)


def case_resize_full_size(dev, cfg):
    """The flow network's input at 720p: six planes of 720 x 1280 -> 2880 x 5120, cropped to whole 32-pixel patches, through
    cropping.crop_and_resize_batch_for_flow."""
    from flowmap_amd import Batch
    from flowmap_amd.misc import cropping

    kind, (h, w), image_shape, mult, patch = cfg
    x = planes_of(kind, 6, h, w, seed=2)
    resized, crop = orc.cropped_shapes((h, w), image_shape, patch, mult)
    origin = ((resized[0] - crop[0]) // 2, (resized[1] - crop[1]) // 2)
    videos = x.reshape(1, 2, 3, h, w).to(dev)
    got = cropping.crop_and_resize_batch_for_flow(Batch(videos), cropping.CroppingCfg(image_shape, mult, patch)).videos
    assert tuple(got.shape) == (1, 2, 3, *crop) and same_bits(videos.reshape(6, h, w), x)
    truth, ref32 = resize_reference(x, resized, origin, crop, torch.float64), resize_reference(x, resized, origin, crop, torch.float32)
    gate(f"resize {kind} {h}x{w} -> {resized[0]}x{resized[1]} crop {crop[0]}x{crop[1]}", got.reshape(6, *crop).cpu(), truth, ref32, FLOOR_CROP, warn=True)


RESIZE_FULL_SIZE = (("iid", (720, 1280), (720, 1280), 4, 8),)

# ---- consistency mask and fused post-processing ----------------------------------------------------------------------------

FLOW_KINDS = ("iid", "shift", "edge", "far")


def video_of(kind, b, f, h, w, seed):
    if kind == "iid":
        return iid_video((b, f, 3, h, w), seed)
    return torch.cat([orc.synth_video(f, h, w, seed=seed + i) for i in range(b)])


def flow_of(kind, b, pairs, h, w, seed, amp=0.3):
    """Raw flow (b, pairs, h, w, 2) in normalised units.  iid: uniform within ±amp; shift: exact integer pixel shifts; edge:
    samples landing exactly on -0.5 px and on size - 0.5 px (the outer edge of the zero padding's last half pixel); far: half
    the pixels ±1e30."""
    gen = torch.Generator().manual_seed(seed)
    shape = (b, pairs, h, w, 2)
    size = torch.tensor([w, h], dtype=torch.float32)
    if kind == "iid":
        return (torch.rand(shape, generator=gen) * 2 - 1) * amp
    if kind == "shift":
        return torch.randint(-3, 4, shape, generator=gen).float() / size
    if kind == "edge":
        xy, _ = orc.pixel_grid((h, w))
        low = torch.rand(shape, generator=gen) < 0.5
        return torch.where(low, -xy.expand(shape), 1.0 - xy.expand(shape)).contiguous()
    if kind == "far":
        flow = (torch.rand(shape, generator=gen) * 2 - 1) * amp
        far = torch.rand(shape, generator=gen) < 0.5
        sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1e30, 1e30)
        return torch.where(far, sign, flow)
    raise KeyError(kind)


# (batch, frames, h, w, flow kind, video kind)
MASK_CASES = (
    (1, 2, 1, 1, "iid", "iid"),
    (2, 5, 1, 1, "far", "iid"),
    (3, 2, 1, 1, "shift", "iid"),
    (2, 3, 1, 7, "shift", "iid"),
    (3, 4, 1, 7, "edge", "iid"),
    (2, 3, 9, 1, "iid", "iid"),
    (3, 2, 9, 1, "edge", "iid"),
    (2, 5, 5, 3, "iid", "smooth"),
    (3, 4, 5, 3, "far", "iid"),
    (3, 5, 17, 13, "edge", "smooth"),
    (2, 4, 24, 36, "shift", "smooth"),
    (2, 3, 61, 1037, "iid", "iid"),
    (3, 2, 61, 1037, "edge", "iid"),
    (1, 4, 61, 1037, "far", "smooth"),
    (1, 2, 1031, 1021, "iid", "iid"),  # 1,052,651 pixels: just over one grid pass
    (2, 2, 1031, 1021, "shift", "smooth"),
    (3, 2, 1031, 1021, "edge", "iid"),
)
MASK_FULL_SIZE = ((1, 3, 2880, 5120, "iid", "iid"),)  # 2 pairs at the flow network's resolution for 720p


def mask_id(c):
    return f"b{c[0]}-f{c[1]}-{c[2]}x{c[3]}-{c[4]}-{c[5]}"


def case_mask(dev, cfg, warn=False):
    b, f, h, w, flow_kind, video_kind = cfg
    videos, flow = video_of(video_kind, b, f, h, w, seed=h + w), flow_of(flow_kind, b, f - 1, h, w, seed=b * 10 + f)
    truth, ref32 = orc.consistency_mask(videos.double(), flow.double()), orc.consistency_mask(videos, flow)
    assert bool(torch.isfinite(truth).all())
    v, fl, out = Carved(videos.numel(), dev).set(videos), Carved(flow.numel(), dev).set(flow), Carved(truth.numel(), dev)
    abi("fm_consistency_mask", v.ptr, fl.ptr, b, f, h, w, out.ptr, stream(dev))
    what = f"mask {mask_id(cfg)}"
    out.check_guards(what)
    assert same_bits(v.view, videos.reshape(-1)) and same_bits(fl.view, flow.reshape(-1)), f"{what}: an input was written to"
    got = out.cpu(truth.shape)
    assert not bool((got == SENTINEL).any()), f"{what}: {int((got == SENTINEL).sum())} pixels were never written"
    gate(what, got, truth, ref32, FLOOR_FLOW, warn=warn)
    for pair in range(b * (f - 1)):  # a pair read from the wrong frames cannot hide under the norm of the stack
        i, j = divmod(pair, f - 1)
        gate(f"{what} pair {i},{j}", got[i, j], truth[i, j], ref32[i, j], FLOOR_FLOW)


# (batch, frames, (h, w), (oh, ow), flow kind, video kind)
POST_CASES = (
    (1, 2, (1, 1), (1, 1), "iid", "iid"),
    (2, 3, (1, 1), (3, 5), "shift", "iid"),
    (3, 2, (1, 9), (1, 9), "iid", "iid"),
    (2, 4, (7, 1), (3, 1), "edge", "iid"),
    (3, 5, (5, 3), (5, 3), "iid", "iid"),
    (2, 5, (5, 3), (11, 8), "far", "smooth"),
    (3, 3, (5, 3), (2, 2), "shift", "iid"),
    (2, 4, (24, 36), (17, 53), "iid", "smooth"),
    (3, 3, (37, 53), (9, 13), "edge", "iid"),
    (2, 3, (61, 1037), (61, 1037), "iid", "iid"),
    (1, 5, (61, 1037), (16, 259), "shift", "smooth"),
    (2, 2, (61, 1037), (40, 701), "far", "iid"),
    (1, 3, (61, 1037), (122, 2074), "edge", "iid"),
    (1, 2, (1031, 1021), (1031, 1021), "iid", "iid"),  # input and output just over one grid pass
    (2, 2, (258, 255), (1031, 1021), "iid", "smooth"),  # x4: the output alone exceeds one pass
    (3, 2, (1031, 1021), (516, 511), "shift", "iid"),  # the input alone exceeds one pass
    (3, 3, (258, 255), (1031, 1021), "edge", "iid"),
)
POST_FULL_SIZE = ((2, 2, (2880, 5120), (1080, 1920), "iid", "iid"),)  # 2 pairs at the flow network's resolution; the output exceeds one pass


def post_id(c):
    return f"b{c[0]}-f{c[1]}-{c[2][0]}x{c[2][1]}-to-{c[3][0]}x{c[3][1]}-{c[4]}-{c[5]}"


def run_postprocess(dev, videos, raws, shape, what):
    """fm_flow_postprocess in both directions on carved outputs -> {forward, backward, forward_mask, backward_mask} on the CPU."""
    b, f, _, h, w = videos.shape
    v = Carved(videos.numel(), dev).set(videos)
    got = {}
    for name, reverse, raw in (("forward", 0, raws[0]), ("backward", 1, raws[1])):
        fl = Carved(raw.numel(), dev).set(raw)
        out_flow, out_mask = Carved(b * (f - 1) * shape[0] * shape[1] * 2, dev), Carved(b * (f - 1) * shape[0] * shape[1], dev)
        abi("fm_flow_postprocess", v.ptr, fl.ptr, b, f, h, w, *shape, reverse, out_flow.ptr, out_mask.ptr, stream(dev))
        out_flow.check_guards(f"{what} {name} flow")
        out_mask.check_guards(f"{what} {name} mask")
        assert same_bits(fl.view, raw.reshape(-1)), f"{what} {name}: the raw flow was written to"
        got[name], got[name + "_mask"] = out_flow.cpu((b, f - 1, *shape, 2)), out_mask.cpu((b, f - 1, *shape))
    assert same_bits(v.view, videos.reshape(-1)), f"{what}: the video was written to"
    return got


def two_way_predictor(videos, raws):
    """A predictor for orc.bidirectional_flows that returns a DIFFERENT raw flow for the time-flipped video, so that the reverse
    direction's raw index (frames - 2 - pair, per batch entry) is part of what is compared."""

    def predictor(v):
        assert v.shape == videos.shape
        return (raws[0] if torch.equal(v, videos.to(v.dtype)) else raws[1]).to(v.dtype)

    return predictor


def case_postprocess(dev, cfg, warn=False):
    b, f, (h, w), shape, flow_kind, video_kind = cfg
    videos = video_of(video_kind, b, f, h, w, seed=h + w + 1)
    raws = (flow_of(flow_kind, b, f - 1, h, w, seed=b * 10 + f), flow_of(flow_kind, b, f - 1, h, w, seed=b * 10 + f + 100))
    assert not torch.equal(videos, videos.flip(dims=(1,)))
    truth = orc.bidirectional_flows(videos.double(), two_way_predictor(videos, raws), shape)
    ref32 = orc.bidirectional_flows(videos, two_way_predictor(videos, raws), shape)
    what = f"postprocess {post_id(cfg)}"
    got = run_postprocess(dev, videos, raws, shape, what)
    for name in ("forward", "backward", "forward_mask", "backward_mask"):
        t64, t32 = getattr(truth, name), getattr(ref32, name)
        assert bool(torch.isfinite(t64).all())
        assert not bool((got[name] == SENTINEL).any()), f"{what} {name}: {int((got[name] == SENTINEL).sum())} elements were never written"
        gate(f"{what} {name}", got[name], t64, t32, FLOOR_FLOW, warn=warn)
        for pair in range(b * (f - 1)):
            i, j = divmod(pair, f - 1)
            gate(f"{what} {name} pair {i},{j}", got[name][i, j], t64[i, j], t32[i, j], FLOOR_FLOW)
    if h * w <= 2 * G:  # the Python layer (FlowPredictor.compute_bidirectional_flow) runs the same two launches
        from flowmap_amd import Batch
        from flowmap_amd.flow import FlowPredictor

        videos_dev, raws_dev = videos.to(dev), tuple(r.to(dev) for r in raws)

        class TwoWay(FlowPredictor):
            def forward(self, v):
                return raws_dev[0] if torch.equal(v, videos_dev) else raws_dev[1]

        flows = TwoWay(None).compute_bidirectional_flow(Batch(videos_dev), shape)
        for name in ("forward", "backward", "forward_mask", "backward_mask"):
            assert same_bits(getattr(flows, name).cpu(), got[name]), f"{what}: FlowPredictor's {name} differs from the entry point's"


NONFINITE = (float("nan"), float("inf"), float("-inf"))
NONFINITE_CASES = ((2, 3, (9, 11), (9, 11)), (1, 2, (9, 11), (18, 22)), (2, 2, (12, 10), (6, 5)), (1, 4, (9, 11), (13, 7)))


def poison(flow, seed):
    """Six pixels of every pair get a NaN, +inf or -inf in one component -> the (b, pairs, h, w) mask of those pixels."""
    b, pairs, h, w, _ = flow.shape
    gen = torch.Generator().manual_seed(seed)
    bad = torch.zeros((b, pairs, h, w), dtype=torch.bool)
    for i in range(b):
        for j in range(pairs):
            where = torch.randperm(h * w, generator=gen)[:6]
            for k, pixel in enumerate(where.tolist()):
                flow[i, j, pixel // w, pixel % w, k % 2] = NONFINITE[(k // 2) % 3]
                bad[i, j, pixel // w, pixel % w] = True
    return bad


def case_mask_nonfinite(dev, cfg):
    """A NaN, +inf or -inf flow gives a NaN mask at that pixel, as grid_sample + torch.max do; every other pixel is untouched."""
    b, f, (h, w), _ = cfg
    videos, flow = video_of("iid", b, f, h, w, seed=3), flow_of("iid", b, f - 1, h, w, seed=4)
    clean = flow.clone()
    bad = poison(flow, seed=5)
    truth, ref32 = orc.consistency_mask(videos.double(), flow.double()), orc.consistency_mask(videos, flow)
    assert torch.equal(torch.isnan(truth), bad), "the reference's mask is NaN exactly where the flow is not finite"
    v, fl, out = Carved(videos.numel(), dev).set(videos), Carved(flow.numel(), dev).set(flow), Carved(truth.numel(), dev)
    abi("fm_consistency_mask", v.ptr, fl.ptr, b, f, h, w, out.ptr, stream(dev))
    out.check_guards("mask, non-finite flow")
    got = out.cpu(truth.shape)
    print(f"\n[mask, non-finite flow {b}x{f}x{h}x{w}] at the {int(bad.sum())} poisoned pixels ours: {sorted(set(got[bad].tolist()), key=str)[:4]}", flush=True)
    gate(f"mask, non-finite flow {b}x{f}x{h}x{w}", got, truth, ref32, FLOOR_FLOW)
    # ... and the finite pixels are, bit for bit, those of the clean flow
    fl.set(clean)
    clean_out = Carved(truth.numel(), dev)
    abi("fm_consistency_mask", v.ptr, fl.ptr, b, f, h, w, clean_out.ptr, stream(dev))
    assert same_bits(got[~bad], clean_out.cpu(truth.shape)[~bad])


def case_postprocess_nonfinite(dev, cfg):
    """After the fused post-processing the output pixels whose taps include a poisoned pixel are non-finite in flow and NaN in
    mask exactly where the reference's are; all others are finite and, bit for bit, those of the clean flow."""
    b, f, (h, w), shape = cfg
    videos = video_of("iid", b, f, h, w, seed=6)
    raws = [flow_of("iid", b, f - 1, h, w, seed=7), flow_of("iid", b, f - 1, h, w, seed=8)]
    clean = [r.clone() for r in raws]
    bad = [poison(raws[0], seed=9), poison(raws[1], seed=10)]
    truth = orc.bidirectional_flows(videos.double(), two_way_predictor(videos, raws), shape)
    ref32 = orc.bidirectional_flows(videos, two_way_predictor(videos, raws), shape)
    what = f"postprocess, non-finite flow {b}x{f}x{h}x{w} -> {shape[0]}x{shape[1]}"
    got = run_postprocess(dev, videos, raws, shape, what)
    got_clean = run_postprocess(dev, videos, clean, shape, what + " (clean)")
    for name in ("forward", "backward"):
        mask_nan = torch.isnan(getattr(truth, name + "_mask"))
        flow_bad = ~torch.isfinite(getattr(truth, name)).all(dim=-1)
        assert 0 < int(mask_nan.sum()) < mask_nan.numel() and torch.equal(mask_nan, flow_bad)
        print(f"\n[{what} {name}] {int(mask_nan.sum())} of {mask_nan.numel()} output pixels are NaN in the reference", flush=True)
        gate(f"{what} {name}", got[name], getattr(truth, name), getattr(ref32, name), FLOOR_FLOW)
        gate(f"{what} {name}_mask", got[name + "_mask"], getattr(truth, name + "_mask"), getattr(ref32, name + "_mask"), FLOOR_FLOW)
        assert same_bits(got[name + "_mask"][~mask_nan], got_clean[name + "_mask"][~mask_nan])
        assert same_bits(got[name][~flow_bad], got_clean[name][~flow_bad])


def case_pair_limit(dev):
    """65535 pairs is the most one launch takes (grid.y); one more is refused with the argument error before anything is
    launched.  1 x 1 frames."""
    for f, ok in ((65536, True), (65537, False)):
        videos, flow = iid_video((1, f, 3, 1, 1), seed=1), flow_of("iid", 1, f - 1, 1, 1, seed=2, amp=2.0)
        v, fl = Carved(videos.numel(), dev).set(videos), Carved(flow.numel(), dev).set(flow)
        mask, out_flow, out_mask = Carved(f - 1, dev), Carved(2 * (f - 1), dev), Carved(f - 1, dev)
        args_mask = ("fm_consistency_mask", v.ptr, fl.ptr, 1, f, 1, 1, mask.ptr, stream(dev))
        args_post = ("fm_flow_postprocess", v.ptr, fl.ptr, 1, f, 1, 1, 1, 1, 1, out_flow.ptr, out_mask.ptr, stream(dev))
        if ok:
            abi(*args_mask)
            abi(*args_post)
            truth, ref32 = orc.consistency_mask(videos.double(), flow.double()), orc.consistency_mask(videos, flow)
            gate("mask, 65535 pairs of 1x1", mask.cpu(truth.shape), truth, ref32, FLOOR_FLOW)
            flipped = flow.flip(dims=(1,))  # reverse: pair p reads raw flow frames-2-p, source frame p+1, target frame p
            back = orc.consistency_mask(videos.flip(dims=(1,)).double(), flow.double()).flip(dims=(1,))
            back32 = orc.consistency_mask(videos.flip(dims=(1,)), flow).flip(dims=(1,))
            gate("postprocess, 65535 pairs of 1x1: mask", out_mask.cpu(truth.shape), back, back32, FLOOR_FLOW)
            assert same_bits(out_flow.cpu(flipped.shape), flipped)
        else:
            refused(*args_mask)
            refused(*args_post)
            for c in (mask, out_flow, out_mask):
                assert bool((c.view == SENTINEL).all()), "a refused launch wrote to its output"
        for c in (mask, out_flow, out_mask):
            c.check_guards("pair limit")
