"""flowmap_amd.install() and projection.depth_consistency: on device tensors (the host double's, the GPU's) it is the fused call and returns
the numbers of the oracle parity whatever the host application is; HOST tensors after install() go to the same composition of the host
application's own functions — on the real reference the result equals the fixture exactly as the reference computes it; after uninstall()
host tensors are refused again.  The host application is the stand-in package (bench_support/standin: the reference's module layout)
and, where it is importable, the reference."""

import os
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("FLOWMAP_REFERENCE", "/root/reference"))
CASE = "odd"


def _reference_readable() -> bool:
    try:
        return (REF / "flowmap" / "model" / "projection.py").is_file()
    except OSError:
        return False


def _installed_device_call(dev):
    import depth_consistency_cases as dc

    import flowmap_amd
    from flowmap_amd import DepthConsistency, _ops, _reference

    flowmap_amd.install()
    try:
        before, host_before = _ops.counters["depth_consistency"], _reference.counters["host_calls"]
        r = dc.run(CASE, dev, details=True, tolerance=0.05)
        assert _ops.counters["depth_consistency"] == before + 1 and isinstance(r, DepthConsistency)  # the fused call, once
        assert _reference.counters["host_calls"] == host_before
        dc.check_layout(r, CASE, dev)
        terms = dc.oracle_case(CASE)
        dc.check_fields(r, terms[torch.float64], terms[torch.float32], "installed")
        win = dc.run(CASE, dev, details=True, frames=(2, 3))
        dc.check_fields(win, terms[torch.float64], terms[torch.float32], "installed, window (2, 3)", rows=slice(2, 5))
    finally:
        flowmap_amd.uninstall()
        flowmap_amd.set_lazy_surfaces(False)


def _host_tensors_after_install(exact_golden):
    """No test double: host tensors after install() run the host application's own functions; after uninstall() they are refused."""
    import depth_consistency_cases as dc

    import flowmap_amd
    from flowmap_amd import _lib, _ops, _reference

    _lib.set_library_for_testing(None)
    flowmap_amd.install()
    try:
        before, host_before = _ops.counters["depth_consistency"], _reference.counters["host_calls"]
        r = dc.run(CASE, "cpu", details=True, tolerance=0.05)
        # no kernel ran; the hand-over was counted (the reference's functions call each other through the rebound names: more than once)
        assert _ops.counters["depth_consistency"] == before and _reference.counters["host_calls"] > host_before
        dc.check_layout(r, CASE, "cpu")
        terms = dc.oracle_case(CASE)
        dc.check_fields(r, terms[torch.float64], terms[torch.float32], "host tensors after install()")
        win = dc.run(CASE, "cpu", details=True, tolerance=0.05, frames=(2, 3))
        dc.check_layout(win, CASE, "cpu", count=3, first=2)
        dc.check_fields(win, terms[torch.float64], terms[torch.float32], "host tensors, window (2, 3)", rows=slice(2, 5))
        ok = r.code == 0
        assert torch.equal(r.support, (ok & (r.error.abs() <= 0.05)).sum(dim=2).to(torch.uint8)) and torch.equal(r.frame_valid, ok.sum(dim=(3, 4)).double())
        if exact_golden:  # the reference's own arithmetic: bit for bit what the fixture's generator got from it
            g = dc.golden()
            r = dc.run(CASE, "cpu", x=dc.golden_inputs(CASE), details=True)  # (on the inputs the fixture was made from)
            for key in dc.GOLDEN_FIELDS.get(CASE, dc.FIELDS) + ("code",):
                assert torch.equal(getattr(r, key), dc.t(g[f"{CASE}_{key}"])), f"{key} is not the fixture's"
    finally:
        flowmap_amd.uninstall()
    assert not _reference.twins
    with pytest.raises(RuntimeError, match="flowmap_amd: depth_consistency: tensors are on cpu.*no CPU fallback"):
        dc.run(CASE, "cpu")


def test_install_on_the_standin_with_the_host_double(standin):
    from flowmap_amd import _lib
    from helpers import build_host_sim

    _lib.set_library_for_testing(build_host_sim())
    try:
        _installed_device_call("cpu")
    finally:
        _lib.set_library_for_testing(None)


def test_host_tensors_after_install_on_the_standin(standin):
    _host_tensors_after_install(exact_golden=False)


@pytest.mark.gpu
def test_install_on_the_standin_runs_the_hip_kernel(standin):
    from flowmap_amd import _lib

    _lib.set_library_for_testing(None)
    _installed_device_call("cuda:0")


@pytest.mark.skipif(not _reference_readable(), reason="reference not mounted or not readable")
def test_host_tensors_after_install_on_the_reference_equal_the_fixture():
    import flowmap_amd
    from conftest import forget_flowmap_modules
    from flowmap_amd import _lib

    sys.dont_write_bytecode = True
    flowmap_amd.uninstall()
    forget_flowmap_modules()
    added = [str(ROOT / "oracle" / "refstubs"), str(REF)]
    sys.path[:0] = added
    try:
        import flowmap

        assert not str(getattr(flowmap, "__file__", None) or list(flowmap.__path__)[0]).startswith(str(ROOT))  # the reference, not the stand-in
        _host_tensors_after_install(exact_golden=True)
    finally:
        flowmap_amd.uninstall()
        _lib.set_library_for_testing(None)
        forget_flowmap_modules()
        for p in added:
            sys.path.remove(p)
