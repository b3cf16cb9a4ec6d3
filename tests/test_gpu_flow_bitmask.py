"""The bit-mask packed format of the fused flow loss (tests/flow_bitmask_cases.py) — on the GPU: the same cases as the CPU module at sizes
that fill several workgroups and leave tail chunks, plus captured steps.  dL/ddepth of the pass is bit-identical between the formats; what
passes through the fp64 atomics is held to 1e-5 relative / 1e-9 absolute (the gate of the packed-vs-streamed test)."""

import pytest

import flow_bitmask_cases as fb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("batch,f,hw,views", [(1, 4, (18, 28), False), (1, 2, (16, 64), False), (3, 3, (10, 12), False), (2, 4, (18, 28), True),
                                              (2, 2, (7, 36), True), (1, 3, (96, 128), False)])
def test_pack_layout_gpu(batch, f, hw, views):
    fb.case_pack_layout(DEV, batch, f, hw, views)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("odd", sorted(fb.ODD_VALUES))
def test_odd_value_selects_fp32_gpu(which, odd):
    fb.case_classification(DEV, which, odd)


@pytest.mark.parametrize("odd", ["binary", "zeros", "ones"])
def test_binary_masks_select_bits_gpu(odd):
    fb.case_classification(DEV, "fwd", odd)


def test_in_place_edit_repacks_and_reclassifies_gpu():
    fb.case_repack(DEV)


@pytest.mark.parametrize("hw", [(20, 52), (96, 128), (120, 160)])
@pytest.mark.parametrize("variant", ["plain", "adam", "taps", "adam_taps"])
@pytest.mark.parametrize("kind", ["huber", "l1", "l2"])
def test_kernel_parity_gpu(kind, variant, hw):
    fb.case_kernel_parity(DEV, kind, variant, hw, batch=2)


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("kind", ["huber", "l1", "l2"])
def test_loss_parity_gpu(kind, view):
    fb.case_loss_parity(DEV, kind, hw=(40, 52), view=view)


@pytest.mark.parametrize("kind", ["huber", "l1", "l2"])
def test_step_parity_gpu(kind):
    fb.case_step_parity(DEV, kind)


@pytest.mark.parametrize("kind", ["huber", "l1", "l2"])
def test_step_parity_with_taps_gpu(kind):
    fb.case_step_parity(DEV, kind, tracking=True)


def test_in_pass_adam_parity_gpu():
    fb.case_in_pass_adam_parity(DEV)


def test_release_originals_gpu():
    fb.case_release_originals(DEV)


def test_graphed_step_gpu():
    fb.case_graphed_step(DEV)
