"""The bit-mask packed format of the fused flow loss (tests/flow_bitmask_cases.py) — CPU, through the serial host double: layout,
classification, repacking, and parity with the fp32 packed format (everything equal: no atomics on the host)."""

import pytest

import flow_bitmask_cases as fb
from flowmap_amd import _lib
from helpers import build_host_sim


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


def test_chunk_constant_matches_header():
    fb.case_header_constant()


@pytest.mark.parametrize("batch,f,hw,views", [(1, 4, (18, 28), False), (1, 2, (16, 64), False), (3, 3, (10, 12), False), (2, 4, (18, 28), True),
                                              (2, 2, (7, 36), True)])
def test_pack_layout(batch, f, hw, views):
    fb.case_pack_layout("cpu", batch, f, hw, views)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("odd", sorted(fb.ODD_VALUES))
def test_odd_value_selects_fp32(which, odd):
    fb.case_classification("cpu", which, odd)


@pytest.mark.parametrize("odd", ["binary", "zeros", "ones"])
def test_binary_masks_select_bits(odd):
    fb.case_classification("cpu", "fwd", odd)


def test_in_place_edit_repacks_and_reclassifies():
    fb.case_repack("cpu")


@pytest.mark.parametrize("variant", ["plain", "adam", "taps", "adam_taps"])
@pytest.mark.parametrize("kind", ["huber", "l1", "l2"])
def test_kernel_parity(kind, variant):
    fb.case_kernel_parity("cpu", kind, variant, (20, 52), batch=2)


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("kind", ["huber", "l1", "l2"])
def test_loss_parity(kind, view):
    fb.case_loss_parity("cpu", kind, view=view)


@pytest.mark.parametrize("kind", ["huber", "l1", "l2"])
def test_step_parity(kind):
    fb.case_step_parity("cpu", kind)


@pytest.mark.parametrize("kind", ["huber", "l1", "l2"])
def test_step_parity_with_taps(kind):
    fb.case_step_parity("cpu", kind, tracking=True)


def test_in_pass_adam_parity():
    fb.case_in_pass_adam_parity("cpu")


def test_release_originals():
    fb.case_release_originals("cpu")
