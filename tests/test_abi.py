"""The C-ABI library loads and exports every entry point include/flowmap_hip.h declares;
the ctypes table matches the header; the product path refuses to run without a GPU."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

from flowmap_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "flowmap_hip.h").read_text()
DECLS = re.findall(r"^int\s+(fm_\w+)\s*\(([^;]*?)\)\s*;", HEADER, flags=re.M | re.S)


def test_header_declares_entry_points():
    assert len(DECLS) >= 30
    assert {n for n, _ in DECLS} == set(_lib.SIGNATURES), "ctypes table and header disagree on the symbol set"


@pytest.mark.parametrize("name,args", DECLS)
def test_signature_arity_matches_header(name, args):
    n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
    assert n_args == len(_lib.SIGNATURES[name]), f"{name}: header has {n_args} parameters"


def test_library_exports_every_symbol():
    if not _lib.LIB_PATH.exists():
        from flowmap_amd.build import build_library

        build_library()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    missing = [n for n, _ in DECLS if not hasattr(lib, n)]
    assert not missing, missing


def test_host_double_exports_every_symbol():
    from helpers import build_host_sim

    lib = ctypes.CDLL(str(build_host_sim()))
    missing = [n for n, _ in DECLS if not hasattr(lib, n)]
    assert not missing, missing


def test_no_cpu_fallback():
    """CPU tensors must be refused loudly by the product path (no eager fallback)."""
    from flowmap_amd.model import projection as fm

    _lib.set_library_for_testing(None)
    with pytest.raises(RuntimeError, match="no CPU fallback|needs a GPU"):
        fm.get_extrinsics(torch.eye(4).repeat(1, 3, 1, 1))


@pytest.mark.parametrize("name", sorted(_lib.SIGNATURES))
def test_null_arguments_are_rejected_without_touching_the_gpu(name):
    """Every entry point validates its arguments before the first HIP call and reports
    FM_ERR_ARG (1) as a status — nothing is thrown across the boundary, nothing is launched."""
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    fn = getattr(lib, name)
    fn.argtypes = _lib.SIGNATURES[name]
    fn.restype = ctypes.c_int
    zeros = [None if t is ctypes.c_void_p else t(0) for t in _lib.SIGNATURES[name]]
    if name == "fm_abi_version":  # no arguments: reports the interface version the header states
        assert fn() == int(re.search(r"#define FM_ABI_VERSION (\d+)", HEADER).group(1))
        return
    assert fn(*zeros) == 1


# ---- the residual entry points: the device build and the host double refuse the same calls and size the same workspaces ----------------
# (flowmap_amd/csrc/fm_residual_args.h states the checks once for both.)  Only REJECTED calls and the size functions are exercised: every
# check precedes the first HIP call, so nothing here reaches a launch — on a machine with a GPU either.

RESIDUAL_PARAMS = {
    "fm_flow_residuals": "depth k kinv t_fwd t_bwd flow_fwd flow_bwd mask_fwd mask_bwd batch frames height width mapping_kind delta aspect_x aspect_y "
                         "first_pair count residual_fwd residual_bwd pred_fwd pred_bwd pair_sum pair_valid workspace layouts stream",
    "fm_track_residuals": "depth kinv ext ext_inv k frames xy vis seg first_segment count pmax fmax height width mapping_kind delta aspect_x aspect_y tgt "
                          "residual visible xy_target pair_sum pair_count track_sum track_count workspace stream",
    "fm_alignment_residuals": "depth kinv surfaces bwd_flow weights weight_sensitivity rel indices points batch frames height width first_pair count "
                              "residual offset weight_out pair_sum pair_weight workspace stream",
    "fm_focal_sweep": "depth weights weight_sensitivity bwd_flow indices points focal_lengths candidate_k candidate_kinv batch frames height width "
                      "first_pair count candidates error soft focal intrinsics poses point_error stream",
}
# a call each build would ACCEPT (never made): every pointer but these set, 5 frames of 8 x 16, the window of pairs [1, 3)
RESIDUAL_NULL = {"layouts", "stream", "surfaces"}
RESIDUAL_VALID = dict(batch=1, frames=5, height=8, width=16, mapping_kind=0, delta=0.01, aspect_x=1.0, aspect_y=1.0, first_pair=1, count=2,
                      first_segment=0, pmax=7, fmax=3, points=128, weight_sensitivity=0.0, candidates=4)
NULLS = "all pointers null"
RESIDUAL_REFUSED = [
    ("fm_flow_residuals", NULLS), ("fm_flow_residuals", dict(first_pair=3)), ("fm_flow_residuals", dict(count=0)), ("fm_flow_residuals", dict(first_pair=-1)),
    ("fm_flow_residuals", dict(batch=65536, first_pair=0, count=1)), ("fm_flow_residuals", dict(height=32768, width=32768)),
    ("fm_flow_residuals", dict(mapping_kind=3)), ("fm_flow_residuals", dict(aspect_x=0.0)), ("fm_flow_residuals", dict(aspect_y=-1.0)),
    ("fm_flow_residuals", dict(pred_bwd=None)), ("fm_flow_residuals", dict(pair_valid=None)), ("fm_flow_residuals", dict(workspace=None)),
    ("fm_flow_residuals", dict(mask_bwd=None)), ("fm_flow_residuals", dict(frames=1, first_pair=0, count=1)),
    ("fm_track_residuals", NULLS), ("fm_track_residuals", dict(count=0)), ("fm_track_residuals", dict(height=32768, width=32768)),
    ("fm_track_residuals", dict(mapping_kind=3)), ("fm_track_residuals", dict(aspect_x=0.0)), ("fm_track_residuals", dict(pair_count=None)),
    ("fm_track_residuals", dict(workspace=None)), ("fm_track_residuals", dict(pmax=0)), ("fm_track_residuals", dict(fmax=0)),
    ("fm_track_residuals", dict(fmax=65536)), ("fm_track_residuals", dict(first_segment=-1)),
    ("fm_alignment_residuals", NULLS), ("fm_alignment_residuals", dict(first_pair=3)), ("fm_alignment_residuals", dict(count=0)),
    ("fm_alignment_residuals", dict(batch=65536, first_pair=0, count=1)), ("fm_alignment_residuals", dict(height=32768, width=32768, points=1 << 29)),
    ("fm_alignment_residuals", dict(surfaces="set")), ("fm_alignment_residuals", dict(depth=None)), ("fm_alignment_residuals", dict(kinv=None)),
    ("fm_alignment_residuals", dict(pair_weight=None)), ("fm_alignment_residuals", dict(workspace=None)), ("fm_alignment_residuals", dict(points=0)),
    ("fm_alignment_residuals", dict(points=1 << 30)), ("fm_alignment_residuals", dict(points=127, indices=None)),
    ("fm_focal_sweep", NULLS), ("fm_focal_sweep", dict(first_pair=3)), ("fm_focal_sweep", dict(count=0)),
    ("fm_focal_sweep", dict(batch=65536, first_pair=0, count=1)), ("fm_focal_sweep", dict(height=32768, width=32768)), ("fm_focal_sweep", dict(points=0)),
    ("fm_focal_sweep", dict(candidates=0)), ("fm_focal_sweep", dict(indices=None)), ("fm_focal_sweep", dict(soft=None)),
]
RESIDUAL_SIZES = {
    "fm_flow_residual_blocks": [(1, 1), (5, 7), (64, 128), (256, 512), (258, 512), (720, 1280), (1, 2048), (1, 2049), (32767, 32768)],
    "fm_alignment_residual_workspace": [(1,), (1024,), (1025,), (128 * 512,), (129 * 512,), (720 * 1280,), ((1 << 30) - 1,)],
    "fm_track_residual_workspace": [(1, 1), (5, 64), (5, 65), (13, 257), (41, 1225)],
}
RESIDUAL_SIZES_REFUSED = {
    "fm_flow_residual_blocks": [(0, 4), (4, 0), (32768, 32768)],
    "fm_alignment_residual_workspace": [(0,), (1 << 30,)],
    "fm_track_residual_workspace": [(0, 1), (1, 0)],
}


@pytest.fixture(scope="module")
def both_builds():
    from helpers import build_host_sim

    if not _lib.LIB_PATH.exists():
        from flowmap_amd.build import build_library

        build_library()
    return {"device build": ctypes.CDLL(str(_lib.LIB_PATH)), "host double": ctypes.CDLL(str(build_host_sim()))}


def _entry(lib, name):
    fn = getattr(lib, name)
    fn.argtypes = _lib.SIGNATURES[name]
    fn.restype = ctypes.c_int
    return fn


@pytest.mark.parametrize("name,change", RESIDUAL_REFUSED, ids=[f"{n}-{c if isinstance(c, str) else ','.join(f'{k}={v}' for k, v in c.items())}" for n, c in RESIDUAL_REFUSED])
def test_residual_calls_are_refused_by_both_builds(both_builds, name, change):
    raw = ctypes.create_string_buffer(4096 + 64)  # what the non-null pointers point at: host memory, 64-byte aligned, never dereferenced
    address = (ctypes.addressof(raw) + 63) & ~63
    args = []
    for param, kind in zip(RESIDUAL_PARAMS[name].split(), _lib.SIGNATURES[name], strict=True):
        if kind is ctypes.c_void_p:
            null = change == NULLS or (param in RESIDUAL_NULL and change.get(param) != "set") or (param in change and change[param] is None)
            args.append(None if null else address)
        else:
            args.append((RESIDUAL_VALID if change == NULLS else {**RESIDUAL_VALID, **change})[param])
    for build, lib in both_builds.items():
        assert _entry(lib, name)(*args) == 1, f"{build}: {name} did not refuse ({change})"


@pytest.mark.parametrize("name", sorted(RESIDUAL_SIZES))
def test_residual_size_functions_agree_between_the_builds(both_builds, name):
    out_type = ctypes.c_int if name == "fm_flow_residual_blocks" else ctypes.c_long
    for args in RESIDUAL_SIZES[name]:
        got = {}
        for build, lib in both_builds.items():
            out = out_type(-1)
            assert _entry(lib, name)(*args, ctypes.cast(ctypes.byref(out), ctypes.c_void_p)) == 0, f"{build}: {name}{args}"
            got[build] = out.value
        assert got["device build"] == got["host double"] > 0, f"{name}{args}: {got}"
    for args in RESIDUAL_SIZES_REFUSED[name]:
        out = out_type(-1)
        for build, lib in both_builds.items():
            assert _entry(lib, name)(*args, ctypes.cast(ctypes.byref(out), ctypes.c_void_p)) == 1, f"{build}: {name}{args} not refused"
            assert _entry(lib, name)(*args, None) == 1, f"{build}: {name}{args} with a null output not refused"


def test_residual_size_functions_at_the_tile_edges(both_builds):
    """The 64- and 65-tile sizes of the GPU sums tests, by value: 2048 pixels and 1024 elements per workgroup, 64 points per chunk."""
    lib = both_builds["host double"]
    blocks, doubles = ctypes.c_int(0), ctypes.c_long(0)
    for hw, want in (((256, 512), 64), ((258, 512), 65)):
        assert _entry(lib, "fm_flow_residual_blocks")(*hw, ctypes.cast(ctypes.byref(blocks), ctypes.c_void_p)) == 0 and blocks.value == want
    for points, want in ((128 * 512, 2 * 64), (129 * 512, 2 * 65)):
        assert _entry(lib, "fm_alignment_residual_workspace")(points, ctypes.cast(ctypes.byref(doubles), ctypes.c_void_p)) == 0 and doubles.value == want
    assert _entry(lib, "fm_track_residual_workspace")(5, 65, ctypes.cast(ctypes.byref(doubles), ctypes.c_void_p)) == 0
    assert doubles.value == 2 * (5 * 5 * 2 + 5 * 65)


def test_track_tile_constant_matches_header():
    from flowmap_amd import _ops

    assert int(re.search(r"#define FM_TRACK_TILE (\d+)", HEADER).group(1)) == _ops.TRACK_TILE


def test_integration_doc_names_every_entry_point():
    """Every entry point the header declares is named in INTEGRATION.md's table (x_fwd/bwd and x(_suffix)
    shorthands included)."""
    import re

    header = (ROOT / "include" / "flowmap_hip.h").read_text()
    names = set(re.findall(r"\bint (fm_\w+)\(", header))
    integration = (ROOT / "INTEGRATION.md").read_text()
    mentioned = integration
    for base in re.findall(r"`(fm_\w+)_fwd/bwd`", integration):
        mentioned += f" {base}_fwd {base}_bwd"
    for base in re.findall(r"`(fm_\w+)/bwd`", integration):
        mentioned += f" {base} {base.rsplit('_', 1)[0]}_bwd"
    for base, suffix in re.findall(r"`(fm_\w+)\((_\w+)\)`", integration):
        mentioned += f" {base} {base}{suffix}"
    missing = sorted(n for n in names if n not in mentioned)
    assert not missing, missing
