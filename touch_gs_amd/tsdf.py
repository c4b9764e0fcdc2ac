"""Export of the learned surface: TSDF fusion of rendered depth into a voxel grid and the grid's zero crossings as an oriented,
coloured point cloud (include/tgs.h: tgs_tsdf_integrate / tgs_tsdf_extract_count / tgs_tsdf_extract_points; csrc/tsdf.hip;
DESIGN 5.1k) or as a triangle mesh (tgs_tsdf_mesh_count / tgs_tsdf_mesh_emit), surface metrics against
ground-truth points, mesh statistics, and a binary PLY writer.

    vol = fuse_model(model, cams, (lo, hi), resolution=256)
    cloud = vol.extract_points()
    write_ply("surface.ply", cloud["points"], cloud["normals"], cloud["colors"])
    mesh = vol.extract_mesh()
    write_ply("mesh.ply", mesh["vertices"], mesh["normals"], mesh["colors"], mesh["faces"])

Nothing here is on the training path: a run that never exports issues none of these launches.  The fusion and the extraction
run in HIP on the volume's device (there is no CPU path); the metrics and the file formats are host code.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

MAX_VIEWS_PER_LAUNCH = 8


class TsdfVolume:
    """A grid of ``dims = (nx, ny, nz)`` voxels of side ``voxel_size`` whose corner (not the first centre) is ``origin``
    (world, kept in fp64), x fastest.  The state is the sums ``S = sum w d``, ``Wt = sum w`` and, with ``color``,
    ``C = sum w rgb`` (fp32 device tensors); the TSDF value is S / Wt."""

    def __init__(self, origin, voxel_size: float, dims: Sequence[int], trunc: float, device="cuda", color: bool = True):
        import torch
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3).copy()
        self.voxel_size, self.trunc = float(voxel_size), float(trunc)
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1 or not self.voxel_size > 0 or not self.trunc > 0:
            raise ValueError("dims must be three positive ints, voxel_size and trunc positive")
        V = self.num_voxels
        self.S = torch.zeros(V, dtype=torch.float32, device=torch.device(device))
        self.device = self.S.device          # resolved: "cuda" becomes the current device's "cuda:<index>"
        self.Wt = torch.zeros(V, dtype=torch.float32, device=self.device)
        self.C = torch.zeros(V, 3, dtype=torch.float32, device=self.device) if color else None
        self.views_integrated = 0

    @property
    def num_voxels(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def view_struct(self, cam, depth, weight=None, rgb=None):
        """The TgsTsdfView of one camera: R and t' = R origin + t formed in fp64 and rounded once (the grid's world origin
        never reaches the device)."""
        from . import _lib
        H, W = cam.H, cam.W
        for name, img, shape in (("depth", depth, (H, W)), ("weight", weight, (H, W)), ("rgb", rgb, (H, W, 3))):
            if img is None:
                continue
            if tuple(img.shape) != shape or str(img.dtype) != "torch.float32" or img.device != self.device or not img.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float32 {list(shape)} tensor on {self.device}")
        vm = np.asarray(cam.viewmat, dtype=np.float64)
        R, t = vm[:3, :3], vm[:3, 3]
        tp = R @ self.origin + t
        v = _lib.TgsTsdfView()
        v.R[:] = [float(x) for x in R.reshape(9)]
        v.t[:] = [float(x) for x in tp]
        v.fx, v.fy, v.cx, v.cy, v.W, v.H = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), int(W), int(H)
        v.near_plane, v.pix_center = float(cam.near), float(cam.pix_center)
        v.depth, v.weight, v.rgb = _lib.ptr(depth), _lib.ptr(weight), _lib.ptr(rgb)
        return v

    def integrate(self, cams, depths, weights=None, rgbs=None) -> None:
        """Fuse the views in order, eight to a launch.  ``depths[i]``: camera-space z [H,W] (what the rasterizer renders; 0,
        negative or non-finite = no measurement), ``weights[i]`` [H,W] or None (= 1), ``rgbs[i]`` [H,W,3] or None.  How the
        views are batched cannot be seen in the result's bits.  No host synchronisation."""
        import torch
        from . import _lib
        lib = _lib.load()
        n = len(cams)
        weights = [None] * n if weights is None else list(weights)
        rgbs = [None] * n if rgbs is None else list(rgbs)
        if not (len(depths) == len(weights) == len(rgbs) == n):
            raise ValueError("cams, depths, weights and rgbs must have one entry per view")
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            for i0 in range(0, n, MAX_VIEWS_PER_LAUNCH):
                i1 = min(i0 + MAX_VIEWS_PER_LAUNCH, n)
                arr = (_lib.TgsTsdfView * (i1 - i0))(*[self.view_struct(cams[i], depths[i], weights[i], rgbs[i])
                                                      for i in range(i0, i1)])
                _lib.check(lib.tgs_tsdf_integrate(nx, ny, nz, C.c_float(self.voxel_size), C.c_float(self.trunc), _lib.ptr(self.S),
                                                  _lib.ptr(self.Wt), _lib.ptr(self.C), i1 - i0, arr, self._stream()),
                           "tgs_tsdf_integrate")
        self.views_integrated += n

    def tsdf(self, w_min: float = 1e-6):
        """f = S / Wt as a [nz, ny, nx] tensor, NaN where Wt < w_min."""
        import torch
        f = torch.where(self.Wt >= w_min, self.S / self.Wt, torch.full_like(self.S, float("nan")))
        return f.view(self.dims[2], self.dims[1], self.dims[0])

    def extract_local(self, w_min: float = 1e-6, want_colors: Optional[bool] = None):
        """The crossings as device tensors in GRID-LOCAL coordinates: dict(points [n,3], normals [n,3], colors [n,3] | None,
        edge_id [n] int64, counts [V] int32).  Rows in edge_id order.  One host read (the number of rows)."""
        import torch
        from . import _lib
        lib = _lib.load()
        if not w_min > 0:
            raise ValueError("w_min must be positive")
        want_colors = self.C is not None if want_colors is None else want_colors
        if want_colors and self.C is None:
            raise ValueError("the volume holds no colour")
        nx, ny, nz = self.dims
        dev = self.device
        counts = torch.empty(self.num_voxels, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.tgs_tsdf_extract_count(nx, ny, nz, C.c_float(self.voxel_size), _lib.ptr(self.S), _lib.ptr(self.Wt),
                                                  C.c_float(w_min), _lib.ptr(counts), self._stream()), "tgs_tsdf_extract_count")
            inclusive = torch.cumsum(counts, 0, dtype=torch.int64)
            offsets = (inclusive - counts).contiguous()
            total = int(inclusive[-1].item())
            points = torch.empty(total, 3, dtype=torch.float32, device=dev)
            normals = torch.empty(total, 3, dtype=torch.float32, device=dev)
            colors = torch.empty(total, 3, dtype=torch.float32, device=dev) if want_colors else None
            edge_id = torch.empty(total, dtype=torch.int64, device=dev)
            if total:
                _lib.check(lib.tgs_tsdf_extract_points(nx, ny, nz, C.c_float(self.voxel_size), _lib.ptr(self.S), _lib.ptr(self.Wt),
                                                       _lib.ptr(self.C) if want_colors else None, C.c_float(w_min),
                                                       _lib.ptr(offsets), _lib.ptr(points), _lib.ptr(normals), _lib.ptr(colors),
                                                       _lib.ptr(edge_id), self._stream()), "tgs_tsdf_extract_points")
        return dict(points=points, normals=normals, colors=colors, edge_id=edge_id, counts=counts)

    def extract_points(self, w_min: float = 1e-6) -> dict:
        """The surface as host arrays: points [n,3] float64 in the WORLD (the origin added in fp64), normals [n,3] float32
        (outward; the grid's axes are the world's), colors [n,3] float32 or None, edge_id [n] int64 = 3 voxel + axis."""
        loc = self.extract_local(w_min)
        return dict(points=loc["points"].cpu().numpy().astype(np.float64) + self.origin,
                    normals=loc["normals"].cpu().numpy(),
                    colors=None if loc["colors"] is None else loc["colors"].cpu().numpy(),
                    edge_id=loc["edge_id"].cpu().numpy())

    def extract_mesh_local(self, w_min: float = 1e-6, want_colors: Optional[bool] = None):
        """The zero level set as a triangle mesh (marching tetrahedra on the Kuhn split of every cell), device
        tensors in GRID-LOCAL coordinates: dict(points [n,3], normals [n,3], colors [n,3] | None, edge_key [n] int64 = 7 voxel
        + edge class, faces [F,3] int32, vmask [V] uint8, ntri [V] uint8).  Vertices in edge_key order, faces in (cell,
        tetrahedron, table) order.  One host read (the two totals); no emit launch for an empty mesh."""
        import torch
        from . import _lib
        lib = _lib.load()
        if not w_min > 0:
            raise ValueError("w_min must be positive")
        want_colors = self.C is not None if want_colors is None else want_colors
        if want_colors and self.C is None:
            raise ValueError("the volume holds no colour")
        nx, ny, nz = self.dims
        dev, V = self.device, self.num_voxels
        vmask, ntri, flags = (torch.empty(V, dtype=torch.uint8, device=dev) for _ in range(3))
        with torch.cuda.device(dev):
            _lib.check(lib.tgs_tsdf_mesh_count(nx, ny, nz, C.c_float(self.voxel_size), _lib.ptr(self.S), _lib.ptr(self.Wt),
                                               C.c_float(w_min), _lib.ptr(vmask), _lib.ptr(ntri), _lib.ptr(flags), self._stream()),
                       "tgs_tsdf_mesh_count")
            popcount = torch.tensor([bin(m).count("1") for m in range(256)], dtype=torch.int64, device=dev)
            nvert = popcount[vmask.long()]
            v_incl, t_incl = torch.cumsum(nvert, 0, dtype=torch.int64), torch.cumsum(ntri, 0, dtype=torch.int64)
            vert_offsets, tri_offsets = (v_incl - nvert).contiguous(), (t_incl - ntri).contiguous()
            n_v, n_f = (int(x) for x in torch.stack([v_incl[-1], t_incl[-1]]).tolist())
            if n_v >= 2 ** 31:
                raise ValueError(f"the mesh has {n_v} vertices: more than an int32 face index holds")
            points = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
            normals = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
            colors = torch.empty(n_v, 3, dtype=torch.float32, device=dev) if want_colors else None
            edge_key = torch.empty(n_v, dtype=torch.int64, device=dev)
            faces = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
            if n_v:
                _lib.check(lib.tgs_tsdf_mesh_emit(nx, ny, nz, C.c_float(self.voxel_size), _lib.ptr(self.S), _lib.ptr(self.Wt),
                                                  _lib.ptr(self.C) if want_colors else None, C.c_float(w_min), _lib.ptr(flags),
                                                  _lib.ptr(vmask), _lib.ptr(vert_offsets), _lib.ptr(tri_offsets), _lib.ptr(points),
                                                  _lib.ptr(normals), _lib.ptr(colors), _lib.ptr(edge_key), _lib.ptr(faces),
                                                  self._stream()), "tgs_tsdf_mesh_emit")
        return dict(points=points, normals=normals, colors=colors, edge_key=edge_key, faces=faces, vmask=vmask, ntri=ntri)

    def extract_mesh(self, w_min: float = 1e-6) -> dict:
        """The mesh as host arrays: vertices [n,3] float64 in the WORLD (the origin added in fp64), normals [n,3] float32,
        colors [n,3] float32 or None, faces [F,3] int32 (counter-clockwise seen from the outside), edge_key [n] int64."""
        loc = self.extract_mesh_local(w_min)
        return dict(vertices=loc["points"].cpu().numpy().astype(np.float64) + self.origin,
                    normals=loc["normals"].cpu().numpy(),
                    colors=None if loc["colors"] is None else loc["colors"].cpu().numpy(),
                    faces=loc["faces"].cpu().numpy(), edge_key=loc["edge_key"].cpu().numpy())

    def save(self, path: str) -> None:
        np.savez_compressed(path, S=self.S.cpu().numpy(), Wt=self.Wt.cpu().numpy(),
                            C=np.zeros((0, 3), np.float32) if self.C is None else self.C.cpu().numpy(), origin=self.origin,
                            voxel_size=np.float64(self.voxel_size), trunc=np.float64(self.trunc),
                            dims=np.asarray(self.dims, dtype=np.int64), views_integrated=np.int64(self.views_integrated))

    @staticmethod
    def load(path: str, device="cuda") -> "TsdfVolume":
        import torch
        with np.load(path) as z:
            vol = TsdfVolume(z["origin"], float(z["voxel_size"]), [int(d) for d in z["dims"]], float(z["trunc"]), device,
                             color=len(z["C"]) > 0)
            vol.S.copy_(torch.from_numpy(z["S"]))
            vol.Wt.copy_(torch.from_numpy(z["Wt"]))
            if vol.C is not None:
                vol.C.copy_(torch.from_numpy(z["C"]))
            vol.views_integrated = int(z["views_integrated"])
        return vol


def grid_for_bounds(bounds, resolution: Optional[int] = 256, voxel_size: Optional[float] = None):
    """(origin, voxel_size, dims) of the grid that covers the box ``bounds = (lo, hi)``: ``resolution`` voxels along its longest
    side, or voxels of ``voxel_size``."""
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
    ext = hi - lo
    if not (ext > 0).all():
        raise ValueError("bounds must have a positive extent on every axis")
    if voxel_size is None:
        voxel_size = float(ext.max()) / int(resolution)
    dims = tuple(int(max(1, np.ceil(e / voxel_size - 1e-9))) for e in ext)
    return lo, float(voxel_size), dims


def fusion_images(out: dict, depth: str = "median", weight: str = "inverse_variance", alpha_min: float = 0.5,
                  max_jump: float = 0.1, var_floor: float = 1.0):
    """The (depth, weight | None) images that one ``model.get_outputs(cam, depth_stats=True)`` contributes, in torch:
    ``depth``: "median" (the expected depth where ``median_gid < 0``) or "expected"; 0 where the accumulation is below
    ``alpha_min`` and where the depth fails the jump gate of ops.depth_normals,
    max(|x_r - x_l|, |x_d - x_u|) > max_jump x  (neighbours clamped at the image border; ``max_jump <= 0``: no gate) --
    the expected depth blends object and table at silhouettes and, unfiltered, fuses into sheets.
    ``weight``: "inverse_variance" = var_floor / (depth_var + var_floor), in (0, 1]; "uniform" = None (1 everywhere)."""
    import torch
    if depth not in ("median", "expected") or weight not in ("inverse_variance", "uniform"):
        raise ValueError('depth must be "median" or "expected", weight "inverse_variance" or "uniform"')
    alpha = out["alpha"].detach()
    x = out["depth"].detach()[..., 0]
    if depth == "median":
        x = torch.where(out["median_gid"] >= 0, out["median_depth"].detach()[..., 0], x)
    keep = alpha >= alpha_min
    if max_jump > 0:
        xr, xl = torch.cat([x[:, 1:], x[:, -1:]], 1), torch.cat([x[:, :1], x[:, :-1]], 1)
        xd, xu = torch.cat([x[1:], x[-1:]], 0), torch.cat([x[:1], x[:-1]], 0)
        keep &= ~(torch.maximum((xr - xl).abs(), (xd - xu).abs()) > max_jump * x)
    d = torch.where(keep, x, torch.zeros_like(x)).float().contiguous()
    w = None
    if weight == "inverse_variance":
        w = (var_floor / (out["depth_var"].detach()[..., 0] + var_floor)).float().contiguous()
    return d, w


def fuse_model(model, cams, bounds, resolution: Optional[int] = 256, voxel_size: Optional[float] = None,
               trunc_voxels: float = 4, depth: str = "median", weight: str = "inverse_variance", alpha_min: float = 0.5,
               max_jump: float = 0.1, var_floor: Optional[float] = None, color: bool = True) -> TsdfVolume:
    """Render every camera with ``model.get_outputs(cam, depth_stats=True)`` and fuse the depth images (fusion_images) into a
    new :class:`TsdfVolume` over ``bounds = (lo, hi)`` (the model's frame).  ``var_floor`` defaults to voxel_size^2."""
    import torch
    origin, vox, dims = grid_for_bounds(bounds, resolution, voxel_size)
    dev = model.params.means.device
    vol = TsdfVolume(origin, vox, dims, trunc_voxels * vox, dev, color=color)
    var_floor = vox * vox if var_floor is None else float(var_floor)
    batch = ([], [], [], [])
    with torch.no_grad():
        for n, cam in enumerate(cams):
            out = model.get_outputs(cam, depth_stats=True)
            d, w = fusion_images(out, depth, weight, alpha_min, max_jump, var_floor)
            for lst, item in zip(batch, (cam, d, w, out["rgb"].detach().float().contiguous() if color else None)):
                lst.append(item)
            if len(batch[0]) == MAX_VIEWS_PER_LAUNCH or n == len(cams) - 1:
                vol.integrate(*batch)
                batch = ([], [], [], [])
    return vol


def nearest_distances_device(p, g, device):
    """(d_pg [len(p)], d_gp [len(g)]) float64: the nearest-neighbour distances between two fp64 clouds from the exact HIP
    k-NN (ops.knn, k = 1).  Both clouds lose their common fp64 centroid before the cast to fp32, so a capture
    far from the origin keeps its digits; d2 is formed in fp32, the root and everything after it in fp64."""
    import torch
    from . import ops
    c = np.concatenate([p, g]).mean(0)
    tp = torch.from_numpy((p - c).astype(np.float32)).to(device)
    tg = torch.from_numpy((g - c).astype(np.float32)).to(device)
    d_pg = ops.knn(tg, 1, queries=tp)[0][:, 0].double().sqrt().cpu().numpy()
    d_gp = ops.knn(tp, 1, queries=tg)[0][:, 0].double().sqrt().cpu().numpy()
    return d_pg, d_gp


def surface_metrics(points, gt_points, tau: float, device=None) -> dict:
    """chamfer = the mean of the two directed mean nearest-neighbour distances; precision = the share of ``points`` within
    ``tau`` of ``gt_points``, recall = the share of ``gt_points`` within ``tau`` of ``points``, fscore = their harmonic mean.
    ``device`` None (the default): two scipy cKDTree queries in fp64 on the host; a GPU device: ``nearest_distances_device``
    (fp32 squared distances of the centred clouds; the means and shares are formed in fp64 either way)."""
    p, g = np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(gt_points, dtype=np.float64).reshape(-1, 3)
    if len(p) == 0 or len(g) == 0:
        return dict(chamfer=float("nan"), precision=0.0, recall=0.0, fscore=0.0, n_points=len(p), n_gt=len(g), tau=float(tau))
    if device is not None:
        d_pg, d_gp = nearest_distances_device(p, g, device)
    else:
        from scipy.spatial import cKDTree
        d_pg = cKDTree(g).query(p)[0]
        d_gp = cKDTree(p).query(g)[0]
    precision, recall = float((d_pg <= tau).mean()), float((d_gp <= tau).mean())
    fscore = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return dict(chamfer=float(0.5 * (d_pg.mean() + d_gp.mean())), precision=precision, recall=recall, fscore=fscore,
                n_points=len(p), n_gt=len(g), tau=float(tau))


def write_ply_table(path: str, names: Sequence[str], columns: Sequence[np.ndarray], comment: Optional[str] = None,
                    faces=None) -> None:
    """A binary little-endian PLY with one ``vertex`` element: column i is property ``names[i]``, float32 -- or uchar where
    the array is uint8 -- and, with ``faces`` [F,3], a ``face`` element of int32 triangles."""
    n = len(columns[0])
    fields = [(name, "u1" if col.dtype == np.uint8 else "<f4") for name, col in zip(names, columns)]
    rec = np.empty(n, dtype=fields)
    for (name, _), col in zip(fields, columns):
        rec[name] = col
    head = ["ply", "format binary_little_endian 1.0"] + ([f"comment {comment}"] if comment else []) + [f"element vertex {n}"]
    head += [f"property {'uchar' if t == 'u1' else 'float'} {name}" for name, t in fields]
    tail = b""
    if faces is not None:
        tri = np.asarray(faces).reshape(-1, 3)
        frec = np.empty(len(tri), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        frec["n"], frec["v"] = 3, tri
        head += [f"element face {len(tri)}", "property list uchar int vertex_indices"]
        tail = frec.tobytes()
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        f.write(tail)


def write_ply(path: str, points, normals=None, colors=None, faces=None) -> None:
    """A point cloud -- with ``faces`` [F,3] a triangle mesh -- as binary little-endian PLY: x y z [nx ny nz] [red green blue],
    floats and uchar colours (``colors`` in [0, 1]); faces as ``property list uchar int vertex_indices``."""
    p = np.asarray(points, dtype=np.float64)
    names, cols = ["x", "y", "z"], [p[:, 0], p[:, 1], p[:, 2]]
    if normals is not None:
        nr = np.asarray(normals)
        names += ["nx", "ny", "nz"]
        cols += [nr[:, 0], nr[:, 1], nr[:, 2]]
    if colors is not None:
        c = np.clip(np.rint(np.asarray(colors, dtype=np.float64) * 255.0), 0, 255).astype(np.uint8)
        names += ["red", "green", "blue"]
        cols += [c[:, 0], c[:, 1], c[:, 2]]
    write_ply_table(path, names, cols, faces=faces)


def mesh_stats(vertices, faces) -> dict:
    """What a viewer cannot tell at a glance: n_vertices, n_faces, boundary_edges (undirected edges with one face),
    nonmanifold_edges (more than two faces, or two that run along it in the same direction), components (of the vertices
    that faces reference), area, volume (signed, outward faces positive; meaningful when the mesh is closed) and
    degenerate_faces (zero area)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    out = dict(n_vertices=int(len(v)), n_faces=int(len(f)), boundary_edges=0, nonmanifold_edges=0, components=0, area=0.0,
               volume=0.0, degenerate_faces=0)
    if len(f) == 0:
        return out
    a, b = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]), np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    code, inv = np.unique(np.minimum(a, b) * len(v) + np.maximum(a, b), return_inverse=True)
    count = np.bincount(inv, minlength=len(code))
    forward = np.bincount(inv, weights=(a < b), minlength=len(code))
    out["boundary_edges"] = int((count == 1).sum())
    out["nonmanifold_edges"] = int(((count > 2) | ((count == 2) & (forward != 1))).sum())
    used = np.unique(f)
    graph = coo_matrix((np.ones(len(code)), (code // len(v), code % len(v))), shape=(len(v), len(v)))
    labels = connected_components(graph, directed=False)[1]
    out["components"] = int(len(np.unique(labels[used])))
    p = v[f] - v[used].mean(0)                                  # (centred: the volume's terms stay small far from the origin)
    cr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    dbl = np.linalg.norm(cr, axis=1)
    out["area"] = float(dbl.sum() / 2.0)
    out["volume"] = float((np.cross(p[:, 0], p[:, 1]) * p[:, 2]).sum() / 6.0)
    out["degenerate_faces"] = int((dbl == 0).sum())
    return out
