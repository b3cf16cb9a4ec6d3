"""TsdfVolume.mesh (fm_tsdf_mesh_count, fm_tsdf_mesh_emit): the surface-nets triangle mesh of a signed-distance grid.  The cases here take a
device; tests/test_hostsim_tsdf_mesh.py runs them on the serial host double of the C ABI, tests/test_gpu_tsdf_mesh.py on the MI355X.  The
volumes, the workgroup size T and u = 2⁻²⁴ are those of tests/tsdf_volume_cases.py, imported and left as they are.

The definition (include/flowmap_hip.h, ABI 17).  Cell c has voxel c as its low corner; it exists when i+1 < nx, j+1 < ny, k+1 < nz and is
active when one of its 12 edges is a crossing of ``surface_points``.  One vertex per active cell in ascending cell id: the fp32 sum of
the crossing edges' points, in the fixed edge order, over their number n; the sum of their normals over its length; the sum of their rgb
over n.  One quad per crossing edge whose four cells exist, in ascending edge id, cells (−1,−1), (0,−1), (0,0), (−1,0) along (b, c) from the
edge's voxel when the tsdf at the edge's low end is negative, reversed otherwise; triangles (q0, q1, q2), (q0, q2, q3).

``restate_mesh`` restates that in numpy fp64 from the build's OWN tsdf / weight / color arrays, over ``restate_surface``'s edge points, so
no decision depends on a rounding: ``cell``, ``edge`` and ``faces`` must be EXACTLY the restatement's, order included.  The values are
compared within bounds derived here from tsdf_volume_cases' bounds on one edge point (xyz 6 ulp(M), rgb 6u, a normal's component
e = 24u·‖G‖/L + 4u) plus the sum of n <= 12 terms and the division:
  xyz      (6.5 + (n+1)/2) ulp(M) per axis, M the largest magnitude on that axis: the mean of n inputs off by 6 ulp(M) each is off by at
           most 6 ulp(M); the partial sum of j terms is at most j·M, so its rounding is at most u·j·M <= j·ulp(M), Σ_{j=2..n} j = n(n+1)/2 − 1,
           divided by n: under (n+1)/2 − 1/n (the 1/n dropped covers the second-order terms); the division rounds once: half an ulp.
  rgb      (7 + (n+1)/2)·u absolute: the same with values in [0, 1] (a lerped colour may exceed 1 by a rounding: the half u more).
  normals  per component 2·√3·E/Λ + 4u with E = Σ e_i + u·(n(n+1)/2 − 1) and Λ the fp64 length of the summed normals S: every component
           of S is off by at most the sum of the edges' bounds plus the roundings of the partial sums (each at most j in magnitude), so
           ‖δS‖ <= √3·E; normalising turns it into at most 2‖δS‖/Λ; the squares, their sum, the root and the division are four more
           roundings of a component that is at most 1.  Where the bound reaches 2 it says nothing (the summed normals nearly cancel, or an
           edge's own bound says nothing): any unit vector, or zero, passes.  The number of such rows is printed; on the plane, the sphere
           and the torus it must be 0.
The worst measured fraction of each bound is printed per case (DESIGN.md §3.1f records them).

The closed surfaces are hand-made: tsdf = clip(distance / 3 voxels, −1, 1) in float32, negative inside, weight 2 everywhere, origin 0,
voxel size 1, the distance taken at the voxel centres (index + 0.5).  Their counts (sphere: V = 522, Q = 520; torus: V = Q = 1062) were
found with a numpy prototype of the definition and are re-derived by ``restate_mesh`` in every run.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

from operator_checks import c_entry_refuses, host_tensor_refused
from tsdf_volume_cases import PLANE, SPECS, T, U, restate_surface, run, run_plane, synthetic_volume

MESH_FIELDS = ("vertices", "normals", "rgb", "cell", "faces", "edge")
STRADDLING = tuple(sorted(set(SPECS) - {"behind", "edge", "one1"}))  # (as tsdf_volume_cases.case_surface: the grids that must cut the surface)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------


def restate_mesh(tsdf, weight, color, color_weight, origin, voxel_size, min_weight):
    """The mesh of a volume (numpy arrays of the build's own output) in fp64 -> dict: cell (V,), vertices, normals, rgb (V, 3), n (V,) the
    crossing edges per cell, normal_bound (V,) the per-component bound of the module docstring, faces (2Q, 3) int32, edge (Q,)."""
    nz, ny, nx = tsdf.shape
    s = restate_surface(tsdf, weight, color, color_weight, origin, voxel_size, min_weight)
    size, stride = np.array([nx, ny, nz]), np.array([1, nx, nx * ny])
    edge = s["edge"]
    rows = np.arange(len(edge))
    voxel, axis = edge // 3, edge % 3
    ijk = np.stack((voxel % nx, (voxel // nx) % ny, voxel // (nx * ny)), axis=1)
    b, c = (axis + 1) % 3, (axis + 2) % 3
    ib, ic = ijk[rows, b], ijk[rows, c]
    # every crossing edge enters the (up to four) cells that hold it, as edge a·4 + db + 2·dc of the cell at −(db, dc) along (b, c)
    members = []
    for dc in (0, 1):
        for db in (0, 1):
            lb, lc = ib - db, ic - dc
            ok = (lb >= 0) & (lc >= 0) & (lb + 1 < size[b]) & (lc + 1 < size[c])  # (index_a + 1 < size_a: the edge crosses)
            members.append(np.stack((voxel[ok] - db * stride[b][ok] - dc * stride[c][ok], axis[ok] * 4 + db + 2 * dc, rows[ok]), axis=1))
    m = np.concatenate(members)
    m = m[np.lexsort((m[:, 1], m[:, 0]))]  # by cell, then in the fixed edge order
    cell, first, n = np.unique(m[:, 0], return_index=True, return_counts=True)
    empty = np.zeros((0, 3))
    if len(cell) == 0:
        return {"cell": cell.astype(np.int64), "vertices": empty, "normals": empty, "rgb": None if color is None else empty, "n": n, "normal_bound": np.zeros(0),
                "faces": np.zeros((0, 3), dtype=np.int32), "edge": np.zeros(0, dtype=np.int64)}
    total = lambda a: np.add.reduceat(a[m[:, 2]], first, axis=0)  # noqa: E731
    vertices = total(s["xyz"]) / n[:, None]
    summed = total(s["normals"])
    length = np.sqrt((summed * summed).sum(axis=1))
    normals = np.where(length[:, None] > 0, summed / np.where(length > 0, length, 1.0)[:, None], 0.0)
    rgb = None if color is None else total(s["rgb"]) / n[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        per_edge = np.where(s["length"] > 0, 24.0 * U * s["scale"] / s["length"], np.inf) + 4.0 * U
        off = total(per_edge) + U * (n * (n + 1) / 2.0 - 1.0)
        normal_bound = np.where(length > 0, 2.0 * np.sqrt(3.0) * off / length, np.inf) + 4.0 * U
    # quads
    has = (ib >= 1) & (ib <= size[b] - 2) & (ic >= 1) & (ic <= size[c] - 2)
    qv, sb, sc = voxel[has], stride[b][has], stride[c][has]
    around = np.stack((qv - sb - sc, qv - sc, qv, qv - sb), axis=1)
    low_negative = tsdf.reshape(-1)[qv] < 0
    around = np.where(low_negative[:, None], around, around[:, ::-1])
    q = np.searchsorted(cell, around)
    assert np.array_equal(cell[q], around), "a quad's cell holds a crossing edge, so it is active"
    faces = np.stack((q[:, [0, 1, 2]], q[:, [0, 2, 3]]), axis=1).reshape(-1, 3).astype(np.int32)
    return {"cell": cell.astype(np.int64), "vertices": vertices, "normals": normals, "rgb": rgb, "n": n, "normal_bound": normal_bound, "faces": faces,
            "edge": edge[has].astype(np.int64)}


def restate_of(v, min_weight=1):
    color = None if v.color is None else v.color.cpu().numpy()
    cw = None if v.color is None else v.color_weight.cpu().numpy()
    return restate_mesh(v.tsdf.cpu().numpy(), v.weight.cpu().numpy(), color, cw, v.origin, v.voxel_size, min_weight)


def check_mesh(v, min_weight, what, silent_normals_allowed=True):
    """TsdfVolume.mesh against restate_mesh of the same volume -> (the mesh, the restatement)."""
    mesh = v.mesh(min_weight)
    want = restate_of(v, min_weight)
    count, quads = len(want["cell"]), len(want["edge"])
    assert mesh.cell.dtype == torch.int64 and mesh.edge.dtype == torch.int64 and mesh.faces.dtype == torch.int32
    assert mesh.vertices.dtype == mesh.normals.dtype == torch.float32 and (mesh.rgb is None) == (v.color is None)
    assert tuple(mesh.vertices.shape) == (count, 3) and tuple(mesh.normals.shape) == (count, 3) and tuple(mesh.cell.shape) == (count,)
    assert tuple(mesh.faces.shape) == (2 * quads, 3) and tuple(mesh.edge.shape) == (quads,), f"{what}: {tuple(mesh.faces.shape)} faces, {quads} quads restated"
    assert mesh.rgb is None or (mesh.rgb.dtype == torch.float32 and tuple(mesh.rgb.shape) == (count, 3))
    assert np.array_equal(mesh.cell.cpu().numpy(), want["cell"]), f"{what}: the cells or their order differ from the restatement"
    assert np.array_equal(mesh.edge.cpu().numpy(), want["edge"]), f"{what}: the quads' edges or their order differ from the restatement"
    assert np.array_equal(mesh.faces.cpu().numpy(), want["faces"]), f"{what}: the faces differ from the restatement"
    if count == 0:
        print(f"  {what}: no vertex at min_weight {min_weight}")
        return mesh, want
    nx, ny, nz = v.dims
    extent = np.maximum(np.abs(np.asarray(v.origin)), np.abs(np.asarray(v.origin) + np.array([nx, ny, nz]) * v.voxel_size))
    ulp = 2.0 ** (np.floor(np.log2(extent)) - 23)
    n = want["n"].astype(np.float64)
    got = mesh.vertices.cpu().numpy().astype(np.float64)
    worst_xyz = float((np.abs(got - want["vertices"]) / ((6.5 + (n[:, None] + 1.0) / 2.0) * ulp[None])).max())
    got_n = mesh.normals.cpu().numpy().astype(np.float64)
    said = want["normal_bound"] < 2.0
    worst_n = float((np.abs(got_n - want["normals"]).max(axis=1) / want["normal_bound"])[said].max()) if said.any() else 0.0
    lengths = np.sqrt((got_n**2).sum(axis=1))
    assert bool(((np.abs(lengths - 1.0) <= 8 * U) | (lengths == 0)).all()), f"{what}: a normal is neither a unit vector nor zero"
    worst_rgb = 0.0
    if mesh.rgb is not None:
        worst_rgb = float((np.abs(mesh.rgb.cpu().numpy().astype(np.float64) - want["rgb"]) / ((7.0 + (n[:, None] + 1.0) / 2.0) * U)).max())
    silent = int((~said).sum())
    print(f"  {what}: {count} vertices, {quads} quads at min_weight {min_weight}; worst fraction of the bound: xyz {worst_xyz:.3f}, normals {worst_n:.3f} "
          f"({silent} rows where it says nothing), rgb {worst_rgb:.3f}")
    assert worst_xyz <= 1.0 and worst_n <= 1.0 and worst_rgb <= 1.0, f"{what}: xyz {worst_xyz:.3f}, normals {worst_n:.3f}, rgb {worst_rgb:.3f} of the bounds"
    assert silent_normals_allowed or silent == 0, f"{what}: the normals' bound says nothing on {silent} rows"
    return mesh, want


def same_mesh(a, b, what=""):
    for name in MESH_FIELDS:
        p, q = getattr(a, name), getattr(b, name)
        assert (p is None) == (q is None), f"{what}{name}"
        if p is not None:
            assert p.dtype == q.dtype and p.shape == q.shape and torch.equal(p.cpu(), q.cpu()), f"{what}{name}: not bit-equal"


def on_host_double(fn):
    """fn() with the serial host double of the C ABI loaded (GPU tests: the other build)."""
    from flowmap_amd import _lib
    from helpers import build_host_sim

    _lib.set_library_for_testing(build_host_sim())
    try:
        return fn()
    finally:
        _lib.set_library_for_testing(None)


def moved(v, dev):
    """The volume with its tensors on ``dev``: the same arrays for the other build."""
    from flowmap_amd import TsdfVolume

    to = lambda x: None if x is None else x.to(dev)  # noqa: E731
    return TsdfVolume(to(v.tsdf), to(v.weight), to(v.color), to(v.color_weight), to(v.world_to_camera), v.origin, v.voxel_size, v.truncation, v.near, v.frames)


# ---- checks 1 and 5: restatement parity at every launch geometry ---------------------------------------------------------------------------------


def case_restatement(dev, name, min_weight=1):
    v = run(name, dev)
    mesh, want = check_mesh(v, min_weight, f"{name} mesh")
    crossings = int(v.surface_points(min_weight)[3].shape[0])
    quads = int(mesh.edge.shape[0])
    if name in STRADDLING and min_weight == 1:
        assert 0 < quads < crossings, f"{name}: {quads} quads of {crossings} crossings: the rim edges carry no quad, the others do"
    if name == "one1":
        assert mesh.vertices.shape[0] == 0 and quads == 0, "257 x 1 x 1 has no cell"
    if min_weight > 1:
        first = v.mesh(1)
        assert 0 < mesh.vertices.shape[0] < first.vertices.shape[0] and 0 < quads < first.edge.shape[0], f"{name}: min_weight = {min_weight} must drop some and keep some"
    if quads:
        faces = mesh.faces.cpu().numpy().reshape(-1, 2, 3)
        corners = np.sort(np.concatenate((faces[:, 0], faces[:, 1, 2:]), axis=1), axis=1)
        assert bool((corners[:, 1:] != corners[:, :-1]).all()), f"{name}: a quad repeats a vertex"


def case_repeatable(dev, name):
    v = run(name, dev)
    same_mesh(v.mesh(), v.mesh(), f"{name} mesh twice: ")


def case_gpu_against_host_double(dev, name):
    """The mesh of the SAME arrays by both builds is bit-equal in every field: the decisions compare identical floats, and the sums, the
    divisions and the root are the same IEEE operations in the same order."""
    v = closed_volume(dev, name) if name in CLOSED else run(name, dev)
    mine = v.mesh()
    host = on_host_double(lambda: moved(v, "cpu").mesh())
    assert mine.vertices.shape[0] > 0 and mine.edge.shape[0] > 0
    same_mesh(mine, host, f"{name} mesh, GPU vs host double: ")


# ---- check 2: the plane, closed form ---------------------------------------------------------------------------------------------------------------


def case_plane(dev, against_host=False):
    v = run_plane(dev)
    mesh, _ = check_mesh(v, 1, "plane mesh", silent_normals_allowed=False)
    nx, ny, nz = PLANE["dims"]
    size = np.float32(PLANE["voxel_size"])
    weight, tsdf = v.weight.cpu().numpy(), v.tsdf.cpu().numpy()
    z = np.float32(PLANE["origin"][2]) + (np.arange(nz, dtype=np.float32) + np.float32(0.5)) * size
    k0 = int(np.nonzero(z == np.float32(1.9375))[0][0])  # the layer below the crossing at z = 2
    assert bool((tsdf[k0] > 0).all() and (tsdf[k0 + 1] < 0).all()), "the plane crosses between these two layers, positive toward the cameras"
    column = (weight[k0] >= 1) & (weight[k0 + 1] >= 1)  # (ny, nx): the z edge of this column crosses
    active = column[:-1, :-1] | column[1:, :-1] | column[:-1, 1:] | column[1:, 1:]  # a cell is active when one of its four z edges crosses
    want_v, want_q = int(active.sum()), int(column[1:-1, 1:-1].sum())
    assert bool(column.all()) and (want_v, want_q) == (9, 4), "every column of the 4 x 4 grid is observed: 9 cells, 4 interior edges"
    assert mesh.vertices.shape[0] == want_v and mesh.edge.shape[0] == want_q and mesh.faces.shape[0] == 2 * want_q
    jj, ii = np.nonzero(active)
    cx = np.float32(PLANE["origin"][0]) + (ii.astype(np.float32) + np.float32(1.0)) * size  # the cell centre: one voxel from the low corner
    cy = np.float32(PLANE["origin"][1]) + (jj.astype(np.float32) + np.float32(1.0)) * size
    xyz = mesh.vertices.cpu().numpy()
    assert np.array_equal(mesh.cell.cpu().numpy(), (k0 * ny + jj) * nx + ii)
    assert np.array_equal(xyz.view(np.uint32), np.stack((cx, cy, np.full_like(cx, 2.0)), axis=1).view(np.uint32)), "plane: z == 2 and xy the cell centre, bit for bit"
    assert np.array_equal(mesh.normals.cpu().numpy(), np.tile(np.array([[0.0, 0.0, -1.0]], dtype=np.float32), (want_v, 1))), "plane: the normals are (0, 0, −1)"
    assert np.array_equal(mesh.rgb.cpu().numpy().view(np.uint32), np.tile(np.array([PLANE["colour"]], dtype=np.float32), (want_v, 1)).view(np.uint32))
    tri = xyz.astype(np.float64)[mesh.faces.cpu().numpy()]
    geometric = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert bool((geometric[:, 2] < 0).all()) and bool((geometric[:, :2] == 0).all()), "plane: every triangle faces −z, toward the cameras"
    assert np.array_equal(mesh.edge.cpu().numpy() % 3, np.full(want_q, 2))
    same_mesh(v.mesh(3), mesh, "plane, min_weight 3: ")
    assert v.mesh(4).vertices.shape[0] == 0 and v.mesh(4).faces.shape == (0, 3)
    if against_host:
        same_mesh(mesh, on_host_double(lambda: run_plane("cpu").mesh()), "plane mesh, GPU vs host double: ")


# ---- check 3: closed surfaces ------------------------------------------------------------------------------------------------------------------------

CLOSED = {
    # name: dims (nx, ny, nz), centre, radii, V, Q, Euler characteristic
    "sphere": ((16, 16, 16), (7.9, 8.2, 8.1), (5.3,), 522, 520, 2),
    "torus": ((24, 24, 10), (12.1, 11.8, 5.2), (7.3, 2.6), 1062, 1062, 0),  # axis along z; 5 760 voxels: a partial 23rd workgroup
}


@functools.lru_cache(maxsize=None)
def closed_fields(kind):
    (nx, ny, nz), centre, radii = CLOSED[kind][:3]
    k, j, i = np.meshgrid(np.arange(nz) + 0.5, np.arange(ny) + 0.5, np.arange(nx) + 0.5, indexing="ij")
    x, y, z = i - centre[0], j - centre[1], k - centre[2]
    if kind == "sphere":
        distance = np.sqrt(x * x + y * y + z * z) - radii[0]
    else:
        distance = np.sqrt((np.sqrt(x * x + y * y) - radii[0]) ** 2 + z * z) - radii[1]
    tsdf = torch.from_numpy(np.clip(distance / 3.0, -1.0, 1.0).astype(np.float32))
    g = torch.Generator().manual_seed(11)
    return tsdf, torch.full((nz, ny, nx), 2, dtype=torch.int32), torch.rand((nz, ny, nx, 3), generator=g), torch.ones((nz, ny, nx), dtype=torch.int32)


def closed_volume(dev, kind):
    from flowmap_amd import TsdfVolume

    tsdf, weight, color, color_weight = closed_fields(kind)
    return TsdfVolume(tsdf.to(dev), weight.to(dev), color.to(dev), color_weight.to(dev), torch.eye(4)[None].to(dev), (0.0, 0.0, 0.0), 1.0, 3.0, 0.0, (0, 1))


def signed_volume(vertices, faces):
    tri = np.asarray(vertices, dtype=np.float64)[faces]
    return float(np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6.0)


def case_closed(dev, kind, against_host=False):
    dims, centre, radii, want_v, want_q, euler = CLOSED[kind]
    v = closed_volume(dev, kind)
    mesh, want = check_mesh(v, 1, f"{kind} mesh", silent_normals_allowed=False)
    faces, xyz = mesh.faces.cpu().numpy().astype(np.int64), mesh.vertices.cpu().numpy()
    count = xyz.shape[0]
    assert (count, mesh.edge.shape[0], faces.shape[0]) == (want_v, want_q, 2 * want_q), f"{kind}: V = {count}, Q = {mesh.edge.shape[0]}"
    surface = v.surface_points()
    assert torch.equal(mesh.edge, surface[3]), f"{kind}: a closed surface inside the grid has a quad on every crossing"
    tri = xyz.astype(np.float64)[faces]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert bool((area > 0).all()) and bool((np.sort(faces, axis=1)[:, 1:] != np.sort(faces, axis=1)[:, :-1]).all()), f"{kind}: a degenerate triangle"
    half = np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))
    code = half[:, 0] * count + half[:, 1]
    assert len(np.unique(code)) == len(code), f"{kind}: a directed half-edge occurs twice: the orientation is not consistent"
    assert np.array_equal(np.sort(code), np.sort(half[:, 1] * count + half[:, 0])), f"{kind}: a half-edge without its reverse: the mesh is not watertight"
    edges = len(code) // 2
    assert count - edges + faces.shape[0] == euler, f"{kind}: V − E + F = {count - edges + faces.shape[0]}"
    assert set(np.unique(faces).tolist()) == set(range(count)), f"{kind}: a vertex no face uses"
    volume, restated = signed_volume(xyz, faces), signed_volume(want["vertices"], want["faces"])
    exact = 4.0 / 3.0 * np.pi * radii[0] ** 3 if kind == "sphere" else 2.0 * np.pi**2 * radii[0] * radii[1] ** 2
    print(f"  {kind}: signed volume {volume:.3f} = {volume / exact:.4f} of the solid's {exact:.3f} (surface nets shrink convex shapes)")
    # 3 V vertex coordinates off by at most 12.5 ulp(M) each move the volume by at most the mesh's area / 3 times that: far below 1e-4
    assert volume > 0 and abs(volume - restated) <= 1e-4 * restated, f"{kind}: signed volume {volume} vs the restatement's {restated}"
    outward = np.einsum("ij,ij->i", np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), mesh.normals.cpu().numpy().astype(np.float64)[faces[:, 0]])
    assert bool((outward > 0).all()), f"{kind}: a triangle faces against its vertex normal"
    if against_host:
        same_mesh(mesh, on_host_double(lambda: closed_volume("cpu", kind).mesh()), f"{kind} mesh, GPU vs host double: ")


# ---- check 4: count-then-emit edges ------------------------------------------------------------------------------------------------------------------


def case_synthetic(dev, kind):
    v = synthetic_volume(dev, kind)
    mesh, _ = check_mesh(v, 1, f"synthetic {kind} mesh")
    nx, ny, nz = v.dims
    if kind == "none":
        assert [tuple(getattr(mesh, name).shape) for name in MESH_FIELDS] == [(0, 3), (0, 3), (0, 3), (0,), (0, 3), (0,)]
        assert [getattr(mesh, name).dtype for name in MESH_FIELDS] == [torch.float32] * 3 + [torch.int64, torch.int32, torch.int64]
    if kind == "last":
        # Every crossing lies inside the last layer, k = nz − 1, which is the last workgroup.  A cell is named by its LOW corner and needs
        # k + 1 < nz, so the cells that hold those edges are the (nx − 1)(ny − 1) of layer nz − 2: the tail of the workgroup before the
        # last, after two workgroups and three quarters of a third that count nothing.  And an edge of the top layer is on the rim of the
        # grid: no quad.  (No quad can start in the last workgroup of this grid at all: an x or y edge there has k = nz − 1, and no z edge
        # starts there.)
        cells = mesh.cell.cpu().numpy()
        assert len(cells) == (nx - 1) * (ny - 1) == 49 and bool((cells // (nx * ny) == nz - 2).all()) and int(cells.min()) >= 2 * T + 192
        assert mesh.edge.shape[0] == 0 and mesh.faces.shape == (0, 3) and int(v.surface_points()[3].min()) // 3 >= 3 * T
    if kind == "every":
        crossings = int(v.surface_points()[3].shape[0])
        assert mesh.vertices.shape[0] == (nx - 1) * (ny - 1) * (nz - 1) == 588
        assert mesh.edge.shape[0] == (nx - 1) * (ny - 2) * (nz - 2) + (ny - 1) * (nx - 2) * (nz - 2) + (nz - 1) * (nx - 2) * (ny - 2) == 1356 and crossings == 2224
    if kind == "weights":
        sizes = [(mesh.vertices.shape[0], mesh.edge.shape[0])]
        for min_weight in (2, 3):
            m, _ = check_mesh(v, min_weight, f"synthetic weights mesh, min_weight {min_weight}")
            sizes.append((m.vertices.shape[0], m.edge.shape[0]))
        assert sizes[0][0] > sizes[1][0] > sizes[2][0] > 0 and sizes[0][1] > sizes[1][1] > sizes[2][1] > 0, f"counts must strictly decrease: {sizes}"
        empty = v.mesh(4)
        assert empty.vertices.shape[0] == 0 and empty.faces.shape == (0, 3) and empty.edge.shape[0] == 0


# ---- check 6: arguments and the boundary -------------------------------------------------------------------------------------------------------------

INF, NAN = float("inf"), float("nan")
MESH_COUNT_PARAMS = "tsdf weight nx ny nz min_weight cell_counts quad_counts stream".split()
MESH_COUNT_VALID = dict(nx=8, ny=4, nz=2, min_weight=1)
MESH_COUNT_REFUSED = ["nulls", dict(nx=0), dict(ny=0), dict(nz=-1), dict(nx=2048, ny=2048, nz=512), dict(min_weight=0), dict(min_weight=-1), dict(tsdf=None),
                      dict(weight=None), dict(cell_counts=None), dict(quad_counts=None)]
MESH_EMIT_PARAMS = ("tsdf weight color color_weight nx ny nz ox oy oz voxel_size min_weight cell_offsets quad_offsets vertex_rows quad_rows xyz normals rgb cell "
                    "cell_vertex faces edge stream").split()
MESH_EMIT_VALID = dict(nx=8, ny=4, nz=2, ox=0.0, oy=0.0, oz=0.0, voxel_size=0.1, min_weight=1, vertex_rows=4, quad_rows=2)
MESH_EMIT_REFUSED = ["nulls", dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=2048, ny=2048, nz=512), dict(min_weight=0), dict(min_weight=-3), dict(voxel_size=0.0),
                     dict(voxel_size=-0.1), dict(voxel_size=NAN), dict(voxel_size=INF), dict(ox=NAN), dict(oy=INF), dict(oz=-INF), dict(vertex_rows=-1),
                     dict(vertex_rows=0), dict(quad_rows=-1), dict(color=None), dict(color_weight=None), dict(rgb=None), dict(cell_vertex=None), dict(tsdf=None),
                     dict(weight=None), dict(cell_offsets=None), dict(quad_offsets=None), dict(xyz=None), dict(normals=None), dict(cell=None), dict(faces=None),
                     dict(edge=None)]


def case_c_entries_refuse(lib, what):
    """The C entries through ctypes, on REJECTED calls only (nothing reaches a launch)."""
    c_entry_refuses(lib, what, "fm_tsdf_mesh_count", MESH_COUNT_PARAMS, MESH_COUNT_VALID, MESH_COUNT_REFUSED)
    c_entry_refuses(lib, what, "fm_tsdf_mesh_emit", MESH_EMIT_PARAMS, MESH_EMIT_VALID, MESH_EMIT_REFUSED)


def case_arguments(dev):
    import pytest

    from flowmap_amd import TsdfMesh

    v = run("part", dev)
    for bad in (0, -1, True, 1.5, 1.0, None, "1"):
        with pytest.raises(ValueError, match="flowmap_amd: mesh: min_weight"):
            v.mesh(min_weight=bad)
    mesh = v.mesh()
    assert isinstance(mesh, TsdfMesh) and not any(getattr(mesh, name).requires_grad for name in MESH_FIELDS)
    same_mesh(v.mesh(min_weight=1), mesh)


def case_host_tensor_refused():
    v = synthetic_volume("cpu", "every")
    host_tensor_refused(lambda: v.mesh(), "flowmap_amd: tensors are on cpu.*no CPU fallback")


# ---- check 7: PLY ----------------------------------------------------------------------------------------------------------------------------------------


def read_ply_faces(path):
    """A small reader of what write_ply writes -> (the vertex count, the faces (M, 3) int32, the header's lines)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    count = int(next(line for line in lines if line.startswith("element vertex")).split()[-1])
    faces = int(next(line for line in lines if line.startswith("element face")).split()[-1])
    body = raw[end + 27 * count:]
    assert len(body) == 13 * faces, "the face block is one uchar and three int32 per face, and nothing follows it"
    records = np.frombuffer(body, dtype=np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    assert bool((records["n"] == 3).all())
    return count, records["v"], lines


def case_ply(dev, tmp_path):
    import pytest

    from flowmap_amd import export

    v = closed_volume(dev, "sphere")
    mesh = v.mesh()
    path = tmp_path / "mesh.ply"
    mesh.write_ply(path)
    xyz, rgb = export.read_ply(path)
    assert np.array_equal(xyz, mesh.vertices.cpu().numpy()), "read_ply returns the vertices of a file with faces"
    assert np.array_equal(rgb, (mesh.rgb.cpu().numpy() * 255).astype(np.float32).astype(np.uint8) / 255.0)
    count, faces, lines = read_ply_faces(path)
    assert count == mesh.vertices.shape[0] and faces.dtype == np.int32 and np.array_equal(faces, mesh.faces.cpu().numpy())
    assert lines[-3:] == [f"element face {mesh.faces.shape[0]}", "property list uchar int vertex_indices", "end_header"] and lines[-4] == "property uchar blue"
    n_xyz, n_rgb, n_normals = mesh.vertices.cpu().numpy(), mesh.rgb.cpu().numpy(), mesh.normals.cpu().numpy()
    four, none, plain = tmp_path / "four.ply", tmp_path / "none.ply", tmp_path / "plain.ply"
    export.write_ply(four, n_xyz, n_rgb, n_normals)
    export.write_ply(none, n_xyz, n_rgb, n_normals, faces=None)
    export.write_ply(plain, n_xyz, n_rgb, n_normals, None)
    assert four.read_bytes() == none.read_bytes() == plain.read_bytes(), "faces=None and the four-argument call write identical bytes"
    head, full = four.read_bytes(), path.read_bytes()
    assert b"element face" not in head and head[-27 * count:] == full[-13 * faces.shape[0] - 27 * count:-13 * faces.shape[0]], "the vertex block is the same"
    bare = synthetic_volume(dev, "every")
    no_colour = type(bare)(bare.tsdf, bare.weight, None, None, bare.world_to_camera, bare.origin, bare.voxel_size, bare.truncation, bare.near, bare.frames).mesh()
    assert no_colour.rgb is None
    no_colour.write_ply(path)
    assert np.array_equal(export.read_ply(path)[1], np.zeros((no_colour.vertices.shape[0], 3))) and np.array_equal(read_ply_faces(path)[1], no_colour.faces.cpu().numpy())
    for bad in (faces[:, :2], faces.astype(np.float32), faces + count):
        with pytest.raises(ValueError, match="flowmap_amd: write_ply: faces"):
            export.write_ply(none, n_xyz, n_rgb, n_normals, bad)


# ---- check 8: memory (GPU) ---------------------------------------------------------------------------------------------------------------------------------


def case_memory(dev, name="wide"):
    """Peak allocated bytes during mesh() stay below the outputs plus 4 B per voxel (cell_vertex) plus the per-workgroup counts, their
    cumulative sums and offsets (three (2, blocks) int64 tensors) and the two totals."""
    v = run(name, dev)
    v.mesh()  # (warm: libraries loaded, allocator primed)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mesh = v.mesh()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = sum(getattr(mesh, key).numel() * getattr(mesh, key).element_size() for key in MESH_FIELDS if getattr(mesh, key) is not None)
    nx, ny, nz = v.dims
    blocks = (nx * ny * nz + T - 1) // T
    allowed = outputs + 4 * nx * ny * nz + 3 * 2 * blocks * 8 + 16
    slack = 12 * 512  # (the caching allocator's granularity on each of the six outputs, the workspace, the four small tensors and the totals)
    print(f"  {name} mesh: peak {peak} B; outputs {outputs} B, cell_vertex {4 * nx * ny * nz} B, counts and offsets {3 * 2 * blocks * 8} B")
    assert peak <= allowed + slack, f"peak {peak} B > {allowed} B"
