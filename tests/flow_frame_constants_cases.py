"""The fused flow pass, C entry point by C entry point, on seeded inputs: what tools/make_golden_flow_bits.py records from one commit and
tests/test_gpu_flow_frame_constants.py compares a later one against, bit for bit.

The pass derives twelve constants per (frame, direction) from K, K⁻¹ and the relative poses (make_dir, fm_math.h).  Where they are computed
— once per wave in the kernel's prologue, or once per step by a small launch that leaves them in the padding of `acc` — must not show in
any output: dL/ddepth, the 13 sums per (frame, direction), the loss and dL/dT, dL/dK that fm_flow_loss_finalize derives from the sums.

Shapes (B, F, H, W).  The first three make a frame ONE workgroup of the pass: each sum then receives a single fp64 atomic onto zero and is
reproducible, so every output is compared with torch.equal.  The last one fills a whole workgroup and part of a second one per frame.
"""

import torch

import cases
from flowmap_amd import _ops
from flowmap_amd._base import FLOW_BITMASK_CHUNK_BYTES
from flowmap_amd._lib import call, ptr, stream_for

SEED = 20240607
ONE_WORKGROUP_SHAPES = [(1, 2, 8, 16),   # two frames: each lacks a direction
                        (2, 3, 6, 20),   # batch entries: frame and pair indices across them
                        (1, 4, 5, 7)]    # W % 4 != 0: the one-pixel-per-item path (no packed format exists for it)
MULTI_WORKGROUP_SHAPE = (1, 3, 40, 128)  # 1 280 quads per frame: a full workgroup and a partial one
SHAPES = ONE_WORKGROUP_SHAPES + [MULTI_WORKGROUP_SHAPE]
KINDS = ("huber", "l1", "l2")
FORMATS = ("none", "fp32", "bits")
OUTPUTS = ("loss", "grad_depth", "g_t_fwd", "g_t_bwd", "g_k", "sums")
ACC_USED = 13  # doubles of an `acc` entry that hold sums (the rest of FLOW_ACC_STRIDE is padding)


def shape_name(shape):
    return "x".join(str(s) for s in shape)


def formats_of(shape):
    return FORMATS if shape[3] % 4 == 0 else ("none",)


SMALL = ("k", "kinv", "t_fwd", "t_bwd")  # inputs whose recipe goes through matrix functions: recorded with the outputs, not regenerated


def inputs(shape, seed=SEED, small=None):
    """Host tensors: depth, a K per frame (focal length and principal point differ from frame to frame, so a wrong frame index shows), its
    inverse, random rigid relative poses, flows, BINARY masks (every format reads the same inputs) and the gradient scale.  The image-sized
    ones come from torch.rand and exactly rounded fp32 arithmetic alone — the same bits on every host; ``small``: the recorded SMALL ones
    (a matrix exponential and an inverse need not round alike on two hosts)."""
    b, f, h, w = shape
    gen = torch.Generator().manual_seed(seed + 1000 * b + 100 * f + h * w)
    depth = 1.0 + 0.3 * torch.rand((b, f, h, w), generator=gen)
    ff = 0.04 * (torch.rand((b, f - 1, h, w, 2), generator=gen) - 0.5)
    fb = 0.04 * (torch.rand((b, f - 1, h, w, 2), generator=gen) - 0.5)
    mf = (torch.rand((b, f - 1, h, w), generator=gen) < 0.7).float()
    mb = (torch.rand((b, f - 1, h, w), generator=gen) < 0.6).float()
    x = {"depth": depth.contiguous(), "ff": ff, "fb": fb, "mf": mf, "mb": mb, "scale": torch.tensor([0.37]), "norm": torch.tensor([2.5e-3, 1.0])}
    if small is not None:
        x.update({name: torch.as_tensor(small[name]).float().contiguous() for name in SMALL})
        return x
    k = torch.eye(3).repeat(b, f, 1, 1)
    k[..., 0, 0] = 0.8 + 0.2 * torch.rand((b, f), generator=gen)
    k[..., 1, 1] = 0.9 + 0.2 * torch.rand((b, f), generator=gen)
    k[..., 0, 2] = 0.45 + 0.1 * torch.rand((b, f), generator=gen)
    k[..., 1, 2] = 0.45 + 0.1 * torch.rand((b, f), generator=gen)
    x["k"] = k.contiguous()
    x["kinv"] = torch.linalg.inv(k.double()).float().contiguous()
    x["t_fwd"] = cases._random_rigid(b * (f - 1), gen).float().reshape(b, f - 1, 4, 4).contiguous()
    x["t_bwd"] = cases._random_rigid(b * (f - 1), gen).float().reshape(b, f - 1, 4, 4).contiguous()
    return x


def checksum(x):
    """Sum of the image-sized inputs' bit patterns: says whether two hosts generated the same ones."""
    return int(sum(int(x[name].contiguous().view(torch.int32).to(torch.int64).sum()) for name in ("depth", "ff", "fb", "mf", "mb")))


class Problem:
    """One shape's inputs on the device, packed once in both formats."""

    def __init__(self, shape, dev, small=None):
        self.shape, self.dev = shape, dev
        self.host = inputs(shape, small=small)
        self.x = {name: v.to(dev) for name, v in self.host.items()}
        b, f, h, w = shape
        self.stream = stream_for(self.x["depth"])
        self.wide = self.bits = None
        if w % 4 == 0:
            chunks = (h * w // 4 + 63) // 64
            x = self.x
            self.wide = torch.empty((b * f, chunks, 6, 64, 4), dtype=torch.float32, device=dev)
            self.bits = torch.empty((b * f, chunks, FLOW_BITMASK_CHUNK_BYTES), dtype=torch.uint8, device=dev)
            call("fm_flow_pack_inputs", ptr(x["ff"]), ptr(x["fb"]), ptr(x["mf"]), ptr(x["mb"]), b, f, h, w, ptr(self.wide), self.stream)
            call("fm_flow_pack_inputs_bitmask", ptr(x["ff"]), ptr(x["fb"]), ptr(x["mf"]), ptr(x["mb"]), b, f, h, w, ptr(self.bits), self.stream)

    def new_acc(self):
        b, f = self.shape[:2]
        return torch.zeros((b * f * 2 * _ops.FLOW_ACC_STRIDE,), dtype=torch.float64, device=self.dev)

    def fused(self, kind, fmt, grad, acc):
        """The fused pass alone: dL/ddepth (None without gradients); the sums are added into ``acc``."""
        b, f, h, w = self.shape
        x = self.x
        ax, ay = w / (h * w) ** 0.5, h / (h * w) ** 0.5
        g_depth = torch.full_like(x["depth"], float("nan")) if grad else None
        scale = ptr(x["scale"]) if grad else None
        head = (ptr(x["depth"]), ptr(x["k"]), ptr(x["kinv"]), ptr(x["t_fwd"]), ptr(x["t_bwd"]))
        geometry = (b, f, h, w, _ops.MAPPING_KINDS[kind], 0.01, ax, ay, ptr(g_depth) if grad else None, ptr(acc), 0)
        if fmt == "bits":
            call("fm_flow_loss_fused_bitmask", *head, ptr(self.bits), scale, *geometry, None, None, None, None, None, 0, 0.0, 0.0, 0.0, 0.0, self.stream)
        elif fmt == "fp32":
            call("fm_flow_loss_fused", *head, None, None, None, None, ptr(self.wide), scale, *geometry, self.stream)
        else:
            call("fm_flow_loss_fused", *head, ptr(x["ff"]), ptr(x["fb"]), ptr(x["mf"]), ptr(x["mb"]), None, scale, *geometry, self.stream)
        return g_depth

    def finalize(self, acc):
        b, f, h, w = self.shape
        x = self.x
        ax, ay = w / (h * w) ** 0.5, h / (h * w) ** 0.5
        loss = torch.empty((1,), device=self.dev)
        g_tf, g_tb, g_k = torch.empty_like(x["t_fwd"]), torch.empty_like(x["t_bwd"]), torch.empty_like(x["k"])
        call("fm_flow_loss_finalize", ptr(acc), ptr(x["k"]), ptr(x["kinv"]), ptr(x["t_fwd"]), ptr(x["t_bwd"]), ptr(x["norm"]), b, f, ax, ay, ptr(loss),
             ptr(g_tf), ptr(g_tb), ptr(g_k), self.stream)
        return loss, g_tf, g_tb, g_k

    def run(self, kind, fmt, grad, acc=None):
        """Fused pass + finalize -> the outputs (OUTPUTS) on the host, and the workspace as finalize left it."""
        acc = self.new_acc() if acc is None else acc
        g_depth = self.fused(kind, fmt, grad, acc)
        sums = acc.reshape(-1, _ops.FLOW_ACC_STRIDE)[:, :ACC_USED].clone()
        loss, g_tf, g_tb, g_k = self.finalize(acc)
        out = {"loss": loss, "g_t_fwd": g_tf, "g_t_bwd": g_tb, "g_k": g_k, "sums": sums}
        if grad:
            out["grad_depth"] = g_depth
        return {name: v.cpu() for name, v in out.items()}, acc


def combos():
    """(shape, kind, format, gradients?) of every recorded case."""
    for shape in SHAPES:
        for kind in KINDS:
            for fmt in formats_of(shape):
                for grad in (True, False):
                    yield shape, kind, fmt, grad


def key(shape, kind, fmt, grad, name):
    return f"{shape_name(shape)}.{kind}.{fmt}.{'grad' if grad else 'loss'}.{name}"
