"""The definition of the TSDF triangle mesh (include/tgs.h: tgs_tsdf_mesh_count, tgs_tsdf_mesh_emit) in NumPy:
marching tetrahedra on the Kuhn (Freudenthal) split of every grid cell.  With ``dtype=np.float64`` it is the reference; with
``np.float32`` it is the kernel-independent emulation (every operation rounded on its own).  Also the generator of the 16-entry
case table (printed from here into csrc/tsdf.hip), a topology checker, a PLY face reader and the analytic states.

Cell a = (i, j, k), i < nx-1, j < ny-1, k < nz-1, has the corners a + d, d in {0,1}^3; it is ACTIVE iff all eight are valid
(Wt >= w_min).  A corner is INSIDE iff f = S / Wt < 0.  Six tetrahedra per cell, one per permutation pi of (x, y, z) in the order
PERMS, with the corners 000 -> e_pi1 -> e_pi1 + e_pi2 -> 111.  Voxel a owns the seven edges a -> a + OFFSETS[e], key 7 a + e.  A
vertex exists on an edge iff both ends are valid, exactly one is inside and an active cell contains the edge.  Vertices in
key order, faces in (cell, tetrahedron, table) order.

Units: those of tests/tsdf_ref.py, with the edge's own two ends (a diagonal edge uses the same formulas).  The fixtures bring
the un-cancelled mass U of their integration; an analytic state is exact by construction and carries U = eps |S|,
UC = eps |C| (the rounding of the stored value itself).
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import tsdf_ref as T

EPS = T.EPS
OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))      # edge class -> offset
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))                    # xyz xzy yxz yzx zxy zyx
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))                                  # tetrahedron edge -> its corners
CORNERS = tuple(itertools.product((0, 1), repeat=3))
# The fp32 emulation's largest errors against fp64 ON THE SAME fp32 STATE over tsdf_ref.ALL and the analytic states, all
# seven edge classes, in the units above, as measured (rounded up in the third digit; tests/test_cpu_tsdf_mesh.py measures
# them on every run, prints them and holds the emulation to them): t and point 0.5454 (two_balls), normal 0.0799 (ball),
# colour 0.5336 (eight).  t and point are NOT within tsdf_ref.FLOORS (0.511: on an analytic state U = eps |S| is the smallest
# unit there can be), so the mesh carries its own floors, and the GPU bars are 4 x these, the project's margin.
FLOORS = dict(t=0.546, point=0.546, normal=0.0800, color=0.534)
BARS = {k: 4.0 * v for k, v in FLOORS.items()}


def parity(perm):
    """0 = even, 1 = odd."""
    return sum(perm[a] > perm[b] for a in range(3) for b in range(a + 1, 3)) & 1


def tet_corners(perm):
    """The four corners of the permutation's tetrahedron as offsets in {0,1}^3."""
    c = [[0, 0, 0]]
    for ax in perm:
        nxt = list(c[-1])
        nxt[ax] = 1
        c.append(nxt)
    return [tuple(x) for x in c]


@functools.lru_cache(maxsize=None)
def case_table():
    """table[parity][case] = a tuple of triangles, each three tetrahedron-edge indices (TET_EDGES); case = the 4-bit inside
    mask, bit q = corner q.  Built from geometry on the even tetrahedron (000, 100, 110, 111; positive orientation) with
    the vertices at the edge midpoints: counter-clockwise seen from the outside.  1 or 3 inside: the three cut edges in
    rising order, the last two swapped where needed.  2 inside: the quad's cycle starts at its lowest edge index and is split
    along the diagonal from there.  An odd tetrahedron is the mirror image: every triangle's last two indices swap."""
    Vt = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)], dtype=np.float64)
    assert np.linalg.det(Vt[1:] - Vt[0]) > 0
    mid = np.array([(Vt[p] + Vt[q]) / 2 for p, q in TET_EDGES])
    eidx = {pq: n for n, pq in enumerate(TET_EDGES)}
    edge = lambda p, q: eidx[(min(p, q), max(p, q))]
    even = []
    for case in range(16):
        ins = [q for q in range(4) if case >> q & 1]
        out = [q for q in range(4) if not case >> q & 1]
        if not ins or not out:
            even.append(())
            continue
        outward = Vt[out].mean(0) - Vt[ins].mean(0)
        if len(ins) == 2:
            (a, b), (c, d) = ins, out
            cyc = [edge(a, c), edge(a, d), edge(b, d), edge(b, c)]
            s = cyc.index(min(cyc))
            cyc = cyc[s:] + cyc[:s]
        else:
            cyc = sorted(edge(p, q) for p in ins for q in out)
        if np.cross(mid[cyc[1]] - mid[cyc[0]], mid[cyc[2]] - mid[cyc[0]]) @ outward < 0:
            cyc = [cyc[0]] + cyc[:0:-1]
        even.append(tuple((cyc[0], cyc[n], cyc[n + 1]) for n in range(1, len(cyc) - 1)))
    odd = [tuple((a, c, b) for a, b, c in tris) for tris in even]
    return (tuple(even), tuple(odd))


def case_table_text():
    """The table as it stands in csrc/tsdf.hip between the two marker comments: [parity][case] = {n, then n triangles x 3
    tetrahedron-edge indices, padded with 0}."""
    lines = []
    for par, name in enumerate(("even", "odd")):
        rows = []
        for tris in case_table()[par]:
            flat = [len(tris)] + [e for tri in tris for e in tri]
            rows.append("{" + ", ".join(str(x) for x in flat + [0] * (7 - len(flat))) + "}")
        for q in range(0, 16, 4):
            lines.append(("  {" if q == 0 else "   ") + ", ".join(rows[q:q + 4]) + ("},  // " + name if q == 12 else ","))
    return "\n".join(lines)


def _lin_offset(d, dims):
    return d[0] + d[1] * dims[0] + d[2] * dims[0] * dims[1]


def extract_mesh(grid, S, Wt, C, w_min, dtype=np.float64, U=None, UC=None):
    """-> dict(vmask [V] u8, ntri [V] u8, edge_key, a, b, cls, t, points, normals, g, colors | None, faces [F,3] int32,
    face_cell [F] [+ the units if U is given])."""
    f = dtype
    dims = tuple(grid["dims"])
    nx, ny, nz = dims
    V = nx * ny * nz
    vox = f(grid["vox"])
    S, Wt = np.asarray(S, dtype=f), np.asarray(Wt, dtype=f)
    valid = Wt >= f(w_min)
    with np.errstate(all="ignore"):
        fval = np.where(valid, S / Wt, f(0))
    inside = valid & (fval < 0)
    idx = T.voxel_indices(dims)
    step = (1, nx, nx * ny)
    lin = np.arange(V)

    def shifted(d, sign=1):
        """(the voxel a + sign d exists [V], its index or 0)"""
        has = np.ones(V, bool)
        for m in range(3):
            c = idx[m] + sign * d[m]
            has &= (c >= 0) & (c < dims[m])
        return has, np.where(has, lin + sign * _lin_offset(d, dims), 0)

    # cells
    exists = (idx[0] < nx - 1) & (idx[1] < ny - 1) & (idx[2] < nz - 1)
    active = exists.copy()
    for d in CORNERS:
        active &= valid[np.where(exists, lin + _lin_offset(d, dims), 0)]
    # vertices, by the definition
    vmask = np.zeros(V, np.uint8)
    for e, d in enumerate(OFFSETS):
        hb, b = shifted(d)
        cross = valid & hb & valid[b] & (inside != inside[b])
        held = np.zeros(V, bool)
        for s in CORNERS:
            if any(s[m] and d[m] for m in range(3)):
                continue
            hc, c = shifted(s, -1)
            held |= hc & active[c]
        vmask |= ((cross & held).astype(np.uint8) << e).astype(np.uint8)
    bits = (vmask[:, None] >> np.arange(7)) & 1
    a, cls = np.nonzero(bits)                                  # row-major: key order
    keys = 7 * a + cls
    # faces
    table = case_table()
    cells = lin[active]
    parts = []
    for tet, perm in enumerate(PERMS):
        tc = tet_corners(perm)
        corner = [cells + _lin_offset(c, dims) for c in tc]
        case = sum(inside[corner[q]].astype(np.int64) << q for q in range(4))
        for cs in range(1, 15):
            sel = case == cs
            if not sel.any():
                continue
            for n, tri in enumerate(table[parity(perm)][cs]):
                fk = []
                for te in tri:
                    p, q = TET_EDGES[te]
                    d = tuple(tc[q][m] - tc[p][m] for m in range(3))
                    fk.append(7 * corner[p][sel] + OFFSETS.index(d))
                parts.append((cells[sel], np.full(sel.sum(), tet), np.full(sel.sum(), n), np.stack(fk, -1)))
    if parts:
        fc, ft, fn, fk = (np.concatenate([p[q] for p in parts]) for q in range(4))
        order = np.lexsort((fn, ft, fc))
        fc, fk = fc[order], fk[order]
        pos = np.searchsorted(keys, fk)
        assert (pos < len(keys)).all() and (keys[np.minimum(pos, len(keys) - 1)] == fk).all(), "a face names an edge without a vertex"
        assert len(np.unique(pos)) == len(keys), "a vertex that no face references"
        faces = pos.astype(np.int32)
    else:
        fc, faces = np.zeros(0, np.int64), np.zeros((0, 3), np.int32)
        assert len(keys) == 0
    ntri = np.bincount(fc, minlength=V).astype(np.uint8)
    # attributes
    def neighbour(axis, sign):
        c = idx[axis] + sign
        has = (c >= 0) & (c < dims[axis])
        other = np.where(has, lin + sign * step[axis], 0)
        return has & valid[other], fval[other]

    grad = np.zeros((V, 3), f)
    for m in range(3):
        hm, fm = neighbour(m, -1)
        hp, fp = neighbour(m, +1)
        both, po, mo = hm & hp, hp & ~hm, hm & ~hp
        with np.errstate(all="ignore"):
            grad[:, m] = np.where(both, (fp - fm) / (f(2.0) * vox), np.where(po, (fp - fval) / vox, np.where(mo, (fval - fm) / vox, f(0))))
    grad[~valid] = 0
    off = np.asarray(OFFSETS)[cls].reshape(-1, 3)
    b = a + off @ np.asarray(step)
    fa, fb = fval[a], fval[b]
    with np.errstate(all="ignore"):
        t = fa / (fa - fb)
    pts = np.stack([(idx[m][a].astype(f) + f(0.5)) * vox for m in range(3)], -1).reshape(-1, 3)
    pts = np.where(off == 1, pts + (t * vox)[:, None], pts)
    g = (f(1.0) - t)[:, None] * grad[a] + t[:, None] * grad[b]
    with np.errstate(all="ignore"):
        length = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
        okn = (length > 0) & np.isfinite(length)
        normals = np.where(okn[:, None], g / length[:, None], f(0))
    out = dict(vmask=vmask, ntri=ntri, edge_key=keys, a=a, b=b, cls=cls, offsets=off, t=t, points=pts, normals=normals, g=g,
               colors=None, faces=faces, face_cell=fc, active=active, exists=exists, vox=float(vox),
               centre_max=float(vox) * (max(dims) + 1))
    ca = cb = None
    if C is not None:
        C = np.asarray(C, dtype=f)
        ca, cb = C[a] / Wt[a][:, None], C[b] / Wt[b][:, None]
        out["colors"] = (f(1.0) - t)[:, None] * ca + t[:, None] * cb
    if U is not None:
        with np.errstate(all="ignore"):
            E = np.where(valid, U / Wt.astype(np.float64), 0.0)
        N = E.copy()
        for m in range(3):
            for sign in (-1, 1):
                has, _ = neighbour(m, sign)
                N += np.where(has, E[np.clip(lin + sign * step[m], 0, V - 1)], 0.0)
        ut = (E[a] + E[b]) / np.abs(fa - fb).astype(np.float64)
        glen = np.maximum(length.astype(np.float64), 1e-300)
        out["unit_t"] = ut
        out["unit_point"] = ut * float(vox) + EPS * out["centre_max"]
        ga, gb = (np.linalg.norm(grad[q].astype(np.float64), axis=1) for q in (a, b))
        out["unit_normal"] = ((N[a] + N[b]) / float(vox) + ut * np.linalg.norm((grad[b] - grad[a]).astype(np.float64), axis=1)
                              + 4 * EPS * (ga + gb)) / glen + 4 * EPS
        if C is not None and UC is not None:
            with np.errstate(all="ignore"):
                ec = np.where(valid[:, None], UC / Wt.astype(np.float64)[:, None], 0.0)
            out["unit_color"] = 2.0 * (ec[a] + ec[b]) + ut[:, None] * np.abs(cb - ca).astype(np.float64)
    return out


def vertex_errors(ref, got):
    """`ref`: extract_mesh(..., U=...) in fp64; `got`: dict(points, normals, colors | None) with the SAME vertices in the same
    order.  -> the largest errors in units.  t is recovered from the point: the coordinates along the edge's offset."""
    fig = dict(t=0.0, point=0.0, normal=0.0, color=0.0, normal_zero_mismatch=0, normal_abs_deg=0.0, n=len(ref["edge_key"]))
    if not fig["n"]:
        return fig
    p = np.asarray(got["points"], dtype=np.float64).reshape(-1, 3)
    dp = np.abs(p - ref["points"])
    fig["point"] = float((dp.max(1) / ref["unit_point"]).max())
    dt = np.where(ref["offsets"] == 1, dp, 0.0).max(1) / ref["vox"]
    fig["t"] = float((dt / (ref["unit_t"] + EPS * (ref["centre_max"] / ref["vox"]))).max())
    n = np.asarray(got["normals"], dtype=np.float64).reshape(-1, 3)
    rn = ref["normals"]
    ang = np.arctan2(np.linalg.norm(np.cross(n, rn), axis=1), (n * rn).sum(1))
    zero = ~rn.any(1)
    fig["normal_zero_mismatch"] = int((zero != ~n.any(1)).sum())
    with np.errstate(all="ignore"):
        fig["normal"] = float(np.where(zero, 0.0, ang / ref["unit_normal"]).max())
    fig["normal_abs_deg"] = float(np.degrees(np.where(zero, 0.0, ang)).max())
    if got.get("colors") is not None and ref["colors"] is not None:
        dc = np.abs(np.asarray(got["colors"], dtype=np.float64).reshape(-1, 3) - ref["colors"])
        with np.errstate(all="ignore"):
            fig["color"] = float(np.where(ref["unit_color"] > 0, dc / ref["unit_color"], np.where(dc == 0, 0, np.inf)).max())
    return fig


# ------------------------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------------------------
def topology(faces, n_vertices):
    """By vertex INDEX (coincident vertices of degenerate faces stay distinct): dict(boundary = undirected edges with one
    face, nonmanifold = with more than two, or two that run the same way, boundary_edges [nb,2], edge_faces = the most faces
    on an edge, chi = V - E + F over the referenced vertices, components)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(faces) == 0:
        return dict(boundary=0, nonmanifold=0, boundary_edges=np.zeros((0, 2), np.int64), boundary_faces=np.zeros(0, np.int64),
                    edge_faces=0, chi=0, components=0, edges=0)
    u = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]])
    v = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]])
    fid = np.tile(np.arange(len(faces)), 3)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    code = lo * np.int64(n_vertices) + hi
    order = np.argsort(code, kind="stable")
    uniq, first, count = np.unique(code[order], return_index=True, return_counts=True)
    forward = np.add.reduceat((u < v)[order].astype(np.int64), first)
    nonmanifold = (count > 2) | ((count == 2) & (forward != 1))
    bnd = count == 1
    used = np.unique(faces)
    parent = np.arange(n_vertices)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for p, q in zip(uniq // n_vertices, uniq % n_vertices):
        rp, rq = find(p), find(q)
        if rp != rq:
            parent[rp] = rq
    comps = len({find(x) for x in used.tolist()})
    return dict(boundary=int(bnd.sum()), nonmanifold=int(nonmanifold.sum()),
                boundary_edges=np.stack([uniq[bnd] // n_vertices, uniq[bnd] % n_vertices], -1),
                boundary_faces=fid[order][first[bnd]], edge_faces=int(count.max()), chi=int(len(used) - len(uniq) + len(faces)),
                components=comps, edges=int(len(uniq)))


def signed_volume(points, faces):
    p = np.asarray(points, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float((np.cross(p[:, 0], p[:, 1]) * p[:, 2]).sum() / 6.0)


def face_normals(points, faces):
    """Un-normalised (twice the area) geometric normals [F,3], fp64."""
    p = np.asarray(points, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def read_ply_mesh(path):
    """A binary little-endian PLY with a vertex element (float / uchar properties) and an optional face element
    (property list uchar int vertex_indices) -> (names, vertex records, faces [F,3] int32 | None)."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = [int(l.split()[2]) for l in lines if l.startswith("element vertex")][0]
    nf = [int(l.split()[2]) for l in lines if l.startswith("element face")]
    kinds = {"float": "<f4", "uchar": "u1"}
    fields = [(l.split()[2], kinds[l.split()[1]]) for l in lines if l.startswith("property") and not l.startswith("property list")]
    vt = np.dtype(fields)
    rec = np.frombuffer(body[:nv * vt.itemsize], dtype=vt)
    faces = None
    if nf:
        assert "property list uchar int vertex_indices" in lines
        ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
        fr = np.frombuffer(body[nv * vt.itemsize:], dtype=ft)
        assert len(fr) == nf[0] and (fr["n"] == 3).all()
        faces = fr["v"].copy()
    else:
        assert len(body) == nv * vt.itemsize
    return [f[0] for f in fields], rec, faces


# ------------------------------------------------------------------------------------------------------------------
# analytic states
# ------------------------------------------------------------------------------------------------------------------
AVOX = 2.0 ** -6                    # a power of two: voxel centres and their distances are exact where the test needs f == 0
ANALYTIC = ("ball", "two_balls", "ball_half_valid", "ball_on_centres", "single_cell")
BALLS = {                           # centres and radii in voxels (grid-local)
    "ball": dict(dims=(19, 17, 15), balls=[((9.3, 8.6, 7.4), 4.7)]),
    "two_balls": dict(dims=(29, 17, 15), balls=[((7.8, 8.6, 7.4), 3.6), ((20.1, 8.3, 7.7), 4.2)]),
    "ball_half_valid": dict(dims=(19, 17, 15), balls=[((9.3, 8.6, 7.4), 4.7)], invalid_from_i=11),
    "ball_on_centres": dict(dims=(19, 17, 15), balls=[((9.5, 8.5, 7.5), 5.0)]),       # a voxel centre, radius 5 voxels
}


@functools.lru_cache(maxsize=None)
def analytic(name):
    """-> (grid, dict(S, Wt, C, U, UC)) in fp64: Wt = 1, S = clip((|c - centre| - r) / trunc, -1, 1) (the smallest over the
    balls), C = Wt x a smooth colour of the position.  Shared: do not modify."""
    if name == "single_cell":
        dims, vox = (2, 2, 2), AVOX
        S = np.full(8, 0.5)
        S[0] = -0.5
        Wt = np.ones(8)
        balls = None
    else:
        spec = BALLS[name]
        dims, vox = spec["dims"], AVOX
        balls = spec["balls"]
    grid = dict(dims=dims, vox=vox, origin=(-0.13, 0.07, 0.21), trunc=3 * vox)
    i, j, k = T.voxel_indices(dims)
    c = np.stack([(q + 0.5) * vox for q in (i, j, k)], -1)
    if balls is not None:
        S = np.min([np.clip((np.linalg.norm(c - np.asarray(ctr) * vox, axis=1) - r * vox) / grid["trunc"], -1.0, 1.0)
                    for ctr, r in balls], axis=0)
        Wt = np.ones(len(S))
        if "invalid_from_i" in spec:
            Wt[i >= spec["invalid_from_i"]] = 0.0
    col = np.stack([0.5 + 0.4 * np.sin(40.0 * c[:, 0]), 0.5 + 0.4 * np.cos(55.0 * c[:, 1]), 0.2 + 3.0 * c[:, 2]], -1)
    C = Wt[:, None] * col
    return grid, dict(S=S, Wt=Wt, C=C, U=EPS * np.abs(S), UC=EPS * np.abs(C))


def state32(name):
    """(grid, S, Wt, C as fp32 arrays, U, UC) of a tsdf_ref fixture (its fp64 reference state) or of an analytic state: what
    the pin copies into a TsdfVolume."""
    if name in ANALYTIC:
        grid, st = analytic(name)
    else:
        grid, st = T.fixture(name)[0], T.reference(name)[0]
    return grid, st["S"].astype(np.float32), st["Wt"].astype(np.float32), st["C"].astype(np.float32), st["U"], st["UC"]


@functools.lru_cache(maxsize=None)
def reference32(name):
    """The fp64 definition evaluated on the fp32-rounded state.  Shared: do not modify."""
    grid, S, Wt, C, U, UC = state32(name)
    return extract_mesh(grid, S, Wt, C, T.W_MIN, U=U, UC=UC)


@functools.lru_cache(maxsize=None)
def emulation32(name):
    grid, S, Wt, C, _, _ = state32(name)
    return extract_mesh(grid, S, Wt, C, T.W_MIN, dtype=np.float32)
