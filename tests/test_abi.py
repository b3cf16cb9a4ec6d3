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


# ---- fm_layout and the in-pass Adam arguments: calls the launchers refuse ---------------------------------------------------------------
# Each call starts from one the device build would accept (never made: B = 2, F = 3, 8 x 16, every pointer the same 64-byte-aligned host
# address) and breaks one thing.  Every check precedes the first HIP call, so the answer is FM_ERR_ARG (1) with or without a GPU; a call
# that slipped past the checks would come back as 2 (launch failure) on a machine without one.

N = 8 * 16
VIEW_VALID = dict(batch=2, frames=3, height=8, width=16, mapping_kind=0, delta=0.01, aspect_x=1.0, aspect_y=1.0, items_per_thread=0, pairs=2, pixels=N,
                  points=64, weight_sensitivity=0.0, weight=1.0, first_pair=0, count=2, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
FLOW5 = [(N, 3), (2 * N, 2), (2 * N, 2), (N, 2), (N, 2)]  # (elements per frame, frames per batch entry) of depth, flow_fwd, flow_bwd, mask_fwd, mask_bwd
PACK4 = [(2 * N, 2), (2 * N, 2), (N, 2), (N, 2)]  # flow_fwd, flow_bwd, mask_fwd, mask_bwd
PROC4 = [(N, 3), (3 * N, 3), (2 * N, 2), (N, 2)]  # depth, surfaces, bwd_flow, weights
NO_ADAM = {"taps", "exp_avg", "exp_avg_sq", "touched"}
# label: (entry, its fm_layout parameter, the stacks that describes, parameters left NULL, batch entries must not overlap?, stacks whose
#         strides must be divisible by 4, what makes a call with a dense layout invalid, builds)
VIEW_ENTRIES = {
    "flow": ("fm_flow_loss_fused_views", "layouts", FLOW5, {"packed"}, True, [], dict(batch=0), ("device build",)),
    "flow-packed": ("fm_flow_loss_fused_views", "layouts", FLOW5, {"flow_fwd", "flow_bwd", "mask_fwd", "mask_bwd"}, True, [0], dict(batch=0), ("device build",)),
    "flow-bitmask": ("fm_flow_loss_fused_bitmask", "depth_layout", FLOW5[:1], NO_ADAM, True, [0], dict(batch=0), ("device build",)),
    "pack": ("fm_flow_pack_inputs_views", "layouts", PACK4, set(), False, [0, 1, 2, 3], dict(batch=0), ("device build",)),
    "pack-bitmask": ("fm_flow_pack_inputs_bitmask_views", "layouts", PACK4, set(), False, [0, 1, 2, 3], dict(batch=0), ("device build",)),
    "masks-binary": ("fm_flow_masks_binary", "layouts", [(N, 2), (N, 2)], set(), False, [], dict(batch=0), ("device build",)),
    "fit": ("fm_procrustes_fit_views", "layouts", PROC4, {"surfaces"}, False, [], dict(points=0), ("device build",)),
    "fit-chain": ("fm_procrustes_fit_chain_views", "layouts", PROC4, {"surfaces", "corr_out", "tap_records"}, False, [], dict(points=0), ("device build",)),
    "scatter": ("fm_procrustes_scatter_views", "layouts", PROC4, {"surfaces"}, False, [], dict(points=0), ("device build",)),
    "scatter-plan": ("fm_procrustes_scatter_plan_views", "flow_layout", [(2 * N, 2)], set(), False, [], dict(points=0), ("device build",)),
    "residuals": ("fm_flow_residuals", "layouts", FLOW5, set(), True, [], dict(batch=0), ("device build", "host double")),
}


def _view_cases():
    for label, (_, _, stacks, _, overlap, mod4, invalid, _) in VIEW_ENTRIES.items():
        for i, (per_frame, frames_of) in enumerate(stacks):
            yield f"{label}-stack{i}-frames-overlap", label, {i: (per_frame - 1, per_frame * frames_of)}, {}
            if overlap:
                yield f"{label}-stack{i}-batch-entries-overlap", label, {i: (per_frame, per_frame * frames_of - 1)}, {}
            if i in mod4:
                yield f"{label}-stack{i}-frames-overlap-by-4", label, {i: (per_frame - 4, per_frame * frames_of)}, {}
                yield f"{label}-stack{i}-frame_stride%4", label, {i: (per_frame + 2, 4 * (per_frame + 2) * frames_of)}, {}
                yield f"{label}-stack{i}-batch_stride%4", label, {i: (per_frame, per_frame * frames_of + 2)}, {}
        yield f"{label}-dense-as-zeros", label, {}, invalid
        yield f"{label}-dense-as-null", label, None, invalid


VIEW_REFUSED = list(_view_cases())
ADAM_ENTRIES = {
    "fm_flow_loss_fused_adam": {"packed"},
    "fm_flow_loss_fused_taps": {"packed"},
    "fm_flow_loss_fused_bitmask": {"depth_layout", "taps"},
}
ADAM_REFUSED = [(name, change) for name in ADAM_ENTRIES for change in (dict(beta1=1.0), dict(step=0), dict(exp_avg="misaligned"), dict(touched=None))]


def _host_arguments(name, values, null, raw, layouts=None, layout_param=None):
    """The arguments of entry ``name``: numbers from ``values``, every pointer the 64-byte-aligned address inside ``raw`` (host memory,
    never dereferenced) unless it is in ``null`` / None in ``values``.  -> (args, what they point at: keep it alive over the call)."""
    address = (ctypes.addressof(raw) + 63) & ~63
    taps = (ctypes.c_void_p * 6)(*[address] * 6)  # include/flowmap_hip.h: fm_flow_taps, six pointers (the launcher reads the struct itself)
    names = [re.search(r"(\w+)\s*$", a).group(1) for a in dict(DECLS)[name].split(",")]
    args = []
    for param, kind in zip(names, _lib.SIGNATURES[name], strict=True):
        if kind is not ctypes.c_void_p:
            args.append(values[param])
        elif param == layout_param:
            args.append(None if layouts is None else ctypes.addressof(layouts))
        elif param in null or (param in values and values[param] is None):
            args.append(None)
        elif param == "taps":
            args.append(ctypes.addressof(taps))
        else:
            args.append(address + 4 if values.get(param) == "misaligned" else address)
    return args, taps


@pytest.mark.parametrize("label,strides,change", [c[1:] for c in VIEW_REFUSED], ids=[c[0] for c in VIEW_REFUSED])
def test_bad_layouts_are_refused(both_builds, label, strides, change):
    """frame_stride below a frame, batch entries that overlap, strides the 16-byte routes cannot take, and the two spellings of "dense"
    ({0, 0} and NULL) beside an invalid argument: status 1, each at the entries whose launcher checks it."""
    from flowmap_amd._base import FmLayout

    name, layout_param, stacks, null, _, _, _, builds = VIEW_ENTRIES[label]
    layouts = None
    if strides is not None:
        layouts = (FmLayout * len(stacks))()
        for i, (frame_stride, batch_stride) in strides.items():
            layouts[i].frame_stride, layouts[i].batch_stride = frame_stride, batch_stride
    raw = ctypes.create_string_buffer(4096 + 64)
    args, _alive = _host_arguments(name, {**VIEW_VALID, **change}, null | {"stream"}, raw, layouts, layout_param)
    for build in builds:
        assert _entry(both_builds[build], name)(*args) == 1, f"{build}: {name} did not refuse ({label}: {strides}, {change})"


@pytest.mark.parametrize("name,change", ADAM_REFUSED, ids=[f"{n}-{k}={v}" for n, c in ADAM_REFUSED for k, v in c.items()])
def test_bad_adam_arguments_of_the_flow_pass_are_refused(both_builds, name, change):
    """The in-pass Adam update: beta1 outside [0, 1), step 0, a moment off the 16-byte grid, `touched` missing -> status 1."""
    raw = ctypes.create_string_buffer(4096 + 64)
    args, _alive = _host_arguments(name, {**VIEW_VALID, **change}, ADAM_ENTRIES[name] | {"stream"}, raw)
    assert _entry(both_builds["device build"], name)(*args) == 1, f"{name} did not refuse ({change})"


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
