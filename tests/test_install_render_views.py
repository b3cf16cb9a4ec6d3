"""flowmap_amd.install() and projection.render_views: on device tensors (the host double's, the GPU's) it is the fused call and passes the
oracle gate whatever the host application is; HOST tensors after install() go to the same composition of the host application's own
functions (an int64 key per candidate, scatter_reduce_(amin)) — on the real reference the result passes the fixture's gate; after
uninstall() host tensors are refused again.  The host application is the stand-in package (bench_support/standin: the reference's module
layout) and, where it is importable, the reference."""

import os
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("FLOWMAP_REFERENCE", "/root/reference"))
CASES = ("two", "up1", "free", "edge")


def _reference_readable() -> bool:
    try:
        return (REF / "flowmap" / "model" / "projection.py").is_file()
    except OSError:
        return False


def _gate(rv, r, name):
    ev32, ev64, win64, firm = rv.oracle_case(name)
    _, _, _, _, shape, radius, near = rv.call_of(name)
    rv.check_render(r, rv.case_inputs(name), ev32, ev64, win64, firm, shape, radius, near, f"installed, {name}")


def _installed_device_call(dev):
    import render_views_cases as rv

    import flowmap_amd
    from flowmap_amd import RenderedViews, _ops, _reference

    flowmap_amd.install()
    try:
        for name in CASES:
            before, host_before = _ops.counters["render_views"], _reference.counters["host_calls"]
            r = rv.run(name, dev)
            assert _ops.counters["render_views"] == before + 1 and isinstance(r, RenderedViews)  # the fused call, once
            assert _reference.counters["host_calls"] == host_before
            _gate(rv, r, name)
    finally:
        flowmap_amd.uninstall()
        flowmap_amd.set_lazy_surfaces(False)


def _host_tensors_after_install(golden):
    """No test double: host tensors after install() run the host application's own functions; after uninstall() they are refused."""
    import render_views_cases as rv

    import flowmap_amd
    from flowmap_amd import _lib, _ops, _reference

    _lib.set_library_for_testing(None)
    flowmap_amd.install()
    try:
        for name in CASES:
            before, host_before = _ops.counters["render_views"], _reference.counters["host_calls"]
            r = rv.run(name, "cpu")
            # no kernel ran; the hand-over was counted (the reference's functions call each other through the rebound names: more than once)
            assert _ops.counters["render_views"] == before and _reference.counters["host_calls"] > host_before
            assert r.source.device.type == "cpu" and not r.depth.requires_grad
            _gate(rv, r, name)
            bare = rv.run(name, "cpu", colors=False, background=0.5)
            assert bare.color is None and torch.equal(bare.source, r.source) and torch.equal(bare.depth, r.depth)
            ground = rv.run(name, "cpu", background=0.5)
            assert bool((ground.color.permute(0, 1, 3, 4, 2)[ground.source < 0] == 0.5).all())
        if golden:  # the reference's own arithmetic decides as the fixture's generator got it from the same functions
            for name in rv.GOLDEN_CASES:
                rv.case_reference_parity("cpu", name)
    finally:
        flowmap_amd.uninstall()
    assert not _reference.twins
    with pytest.raises(RuntimeError, match="flowmap_amd: render_views: tensors are on cpu.*no CPU fallback"):
        rv.run("tiny", "cpu")


def test_install_on_the_standin_with_the_host_double(standin):
    from flowmap_amd import _lib
    from helpers import build_host_sim

    _lib.set_library_for_testing(build_host_sim())
    try:
        _installed_device_call("cpu")
    finally:
        _lib.set_library_for_testing(None)


def test_host_tensors_after_install_on_the_standin(standin):
    _host_tensors_after_install(golden=False)


@pytest.mark.gpu
def test_install_on_the_standin_runs_the_hip_kernel(standin):
    from flowmap_amd import _lib

    _lib.set_library_for_testing(None)
    _installed_device_call("cuda:0")


@pytest.mark.skipif(not _reference_readable(), reason="reference not mounted or not readable")
def test_host_tensors_after_install_on_the_reference_pass_the_fixture():
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
        _host_tensors_after_install(golden=True)
    finally:
        flowmap_amd.uninstall()
        _lib.set_library_for_testing(None)
        forget_flowmap_modules()
        for p in added:
            sys.path.remove(p)
