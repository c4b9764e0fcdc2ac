"""The definition of the TSDF fusion and of the crossing extraction (include/tgs.h: tgs_tsdf_integrate, tgs_tsdf_extract_count,
tgs_tsdf_extract_points) in NumPy.  With ``dtype=np.float64`` it is the reference; with ``np.float32`` it is the
kernel-independent emulation (every product and sum rounded on its own, in the header's order) whose error against the
reference gives the floors the GPU bars are derived from.  Also the fixtures, the classification of clear / unclear voxels
and sign-clear crossings, and the error units.

Units (the project's un-cancelled-mass convention), eps = 2^-24:
  S      : U  = eps sum w (|d| + Z / trunc),  Z = sum_j |R_2j c_j| + |t'_z|  the un-cancelled magnitude of p.z
  Wt     : eps Wt
  C      : UC = eps sum w |rgb|   (per channel)
  t      : Ut = (U_a / Wt_a + U_b / Wt_b) / |f_a - f_b|        (the ends differ in sign: the denominator does not cancel)
  point  : Ut vox + eps |centre|_max                          (the centre's own rounding)
           (as a test recovers t from the point's coordinate along the edge, t is held to Ut + eps |centre|_max / vox)
  colour : 2 (UC_a / Wt_a + UC_b / Wt_b) + Ut |c_b - c_a|      (C / Wt: the sum's and the weight's rounding, then the blend)
  normal : the angle, radians:  ((N_a + N_b) / vox + Ut |g_b - g_a| + 4 eps (|g_a| + |g_b|)) / |g| + 4 eps,   N_v = the sum of
           U / Wt over v and its valid 6-neighbours (the stencil of g(v)),  g = (1 - t) g_a + t g_b  before normalisation;
           4 eps (|g_a| + |g_b|): the four roundings of a gradient on its way into g (difference, quotient, product, sum),
           which matter where g_a and g_b cancel;  4 eps: the unit vector's own rounding (square root, three quotients)
"""
from __future__ import annotations

import functools

import numpy as np

EPS = 2.0 ** -24
CAP_UNCLEAR = 0.03        # share of unclear voxels, and of reference crossings with an end that is not sign-clear
PIX_MARGIN, NEAR_MARGIN, TRUNC_MARGIN = 1e-3, 1e-4, 1e-5
SIGN_CLEAR = 8.0          # an end is sign-clear if |S_ref| > SIGN_CLEAR * U
# The fp32 emulation's largest errors over the fixtures and the eight-view scene, in the units above, as measured (rounded up
# in the third digit; tests/test_cpu_tsdf.py measures them on every run, prints them and holds the emulation to them); the GPU
# bars are 4 x these floors, the margin of the projection and SSIM pins.
FLOORS = dict(S=1.41, Wt=2.71, C=3.11, t=0.511, point=0.511, normal=0.182, color=0.732)
BARS = {k: 4.0 * v for k, v in FLOORS.items()}


# ------------------------------------------------------------------------------------------------------------------
# cameras and analytic depth
# ------------------------------------------------------------------------------------------------------------------
def look_at(pos, target=(0.0, 0.0, 0.0), up=(0.13, 0.21, 1.0)):
    """-> (R [3,3] world -> camera in OpenCV axes (x right, y down, z forward), t [3]), fp64."""
    pos, target, up = (np.asarray(a, dtype=np.float64) for a in (pos, target, up))
    z = target - pos
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ pos


def _rays(R, W, H, fx, fy, cx, cy, pix_center):
    us, vs = np.meshgrid(np.arange(W) + pix_center, np.arange(H) + pix_center)
    d = np.stack([(us - cx) / fx, (vs - cy) / fy, np.ones_like(us)], -1)      # camera frame, z = 1: the ray parameter IS z
    return d, d @ R                                                           # world directions R^T d


def sphere_depth(R, t, W, H, fx, fy, cx, cy, centre, radius, pix_center=0.5):
    """Camera-space z of the first hit of each pixel's ray with the sphere; 0 where it misses.  fp64 [H,W]."""
    d, _ = _rays(R, W, H, fx, fy, cx, cy, pix_center)
    cc = R @ np.asarray(centre, dtype=np.float64) + t
    b, dd = d @ cc, (d * d).sum(-1)
    disc = b * b - dd * (cc @ cc - radius * radius)
    s = (b - np.sqrt(np.maximum(disc, 0.0))) / dd
    return np.where((disc > 0) & (s > 0), s, 0.0)


def plane_depth(R, t, W, H, fx, fy, cx, cy, normal, h, pix_center=0.5):
    """The same for the plane  normal . x = h."""
    _, dw = _rays(R, W, H, fx, fy, cx, cy, pix_center)
    n = np.asarray(normal, dtype=np.float64)
    pos = -R.T @ t
    den = dw @ n
    s = (h - n @ pos) / np.where(den == 0, 1.0, den)
    return np.where((den != 0) & (s > 0), s, 0.0)


# ------------------------------------------------------------------------------------------------------------------
# the two passes
# ------------------------------------------------------------------------------------------------------------------
def voxel_indices(dims):
    nx, ny, nz = dims
    lin = np.arange(nx * ny * nz)
    return lin % nx, (lin // nx) % ny, lin // (nx * ny)


def recentre(view, origin):
    """(R, t' = R origin + t) in fp64: what the host hands to the device after ONE rounding."""
    R = np.asarray(view["R"], dtype=np.float64)
    return R, R @ np.asarray(origin, dtype=np.float64) + np.asarray(view["t"], dtype=np.float64)


def integrate(grid, views, state=None, dtype=np.float64, color=True):
    """-> dict(S, Wt, C | None, U, UC, unclear, updates): the state after `views` (array order) on top of `state` (a dict of
    an earlier call, or None = zeros).  U, UC, unclear (bool per voxel) and updates (count per voxel) continue too."""
    f = dtype
    nx, ny, nz = grid["dims"]
    V = nx * ny * nz
    i, j, k = voxel_indices(grid["dims"])
    vox, trunc = f(grid["vox"]), f(grid["trunc"])
    X, Y, Z = ((a.astype(f) + f(0.5)) * vox for a in (i, j, k))
    if state is None:
        state = dict(S=np.zeros(V, f), Wt=np.zeros(V, f), C=np.zeros((V, 3), f) if color else None, U=np.zeros(V),
                     UC=np.zeros((V, 3)), unclear=np.zeros(V, bool), updates=np.zeros(V, np.int64))
    st = {key: (None if val is None else val.copy()) for key, val in state.items()}
    S, Wt, C = st["S"], st["Wt"], st["C"]
    for vw in views:
        R64, t64 = recentre(vw, grid["origin"])
        R, t = R64.astype(f), t64.astype(f)
        W, H = vw["W"], vw["H"]
        near = f(vw["near"])
        off = f(0.5) - f(vw["pix_center"])
        with np.errstate(all="ignore"):
            pz = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + t[2]
            px = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + t[0]
            py = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + t[1]
            u = f(vw["fx"]) * px / pz + f(vw["cx"]) + off
            v = f(vw["fy"]) * py / pz + f(vw["cy"]) + off
            fu, fv = np.floor(u), np.floor(v)
            front = pz > near
            ok = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            pu, pv = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
            D = np.asarray(vw["depth"], dtype=np.float32)[pv, pu].astype(f)
            ok &= np.isfinite(D) & (D > 0)
            w = np.ones(V, f) if vw.get("weight") is None else np.asarray(vw["weight"], dtype=np.float32)[pv, pu].astype(f)
            ok &= np.isfinite(w) & (w > 0)
            sdf = D - pz
            inside = ok.copy()
            ok &= ~(sdf < -trunc)
            d = np.minimum(sdf / trunc, f(1.0))
        S[ok] = S[ok] + (w * d)[ok]
        Wt[ok] = Wt[ok] + w[ok]
        rgb = None
        if C is not None and vw.get("rgb") is not None:
            rgb = np.asarray(vw["rgb"], dtype=np.float32)[pv, pu].astype(f)
            C[ok] = C[ok] + (w[:, None] * rgb)[ok]
        # units and the classification (fp64 whatever dtype is)
        Zmass = np.abs(R64[2, 0] * X) + np.abs(R64[2, 1] * Y) + np.abs(R64[2, 2] * Z) + abs(t64[2])
        w64, d64 = w.astype(np.float64), d.astype(np.float64)
        st["U"][ok] += EPS * (w64 * (np.abs(d64) + Zmass / float(trunc)))[ok]
        if rgb is not None:
            st["UC"][ok] += EPS * (w64[:, None] * np.abs(rgb.astype(np.float64)))[ok]
        st["updates"][ok] += 1
        with np.errstate(all="ignore"):
            fr_u, fr_v = u - fu, v - fv
            edge = front & ((np.minimum(fr_u, 1 - fr_u) < PIX_MARGIN) | (np.minimum(fr_v, 1 - fr_v) < PIX_MARGIN))
            st["unclear"] |= edge | (np.abs(pz - near) < NEAR_MARGIN) | (inside & (np.abs(sdf + trunc) < TRUNC_MARGIN))
    return st


def extract(grid, S, Wt, C, w_min, dtype=np.float64, U=None, UC=None):
    """-> dict(counts [V], edge_id, t, points, normals, colors | None [+ units if U is given]); rows in edge_id order, which
    is the order the header prescribes."""
    f = dtype
    nx, ny, nz = grid["dims"]
    V = nx * ny * nz
    vox = f(grid["vox"])
    S, Wt = np.asarray(S, dtype=f), np.asarray(Wt, dtype=f)
    valid = Wt >= f(w_min)
    with np.errstate(all="ignore"):
        fval = np.where(valid, S / Wt, f(0))
    idx = voxel_indices(grid["dims"])
    dims, step = (nx, ny, nz), (1, nx, nx * ny)
    lin = np.arange(V)

    def neighbour(axis, sign):
        """(exists and valid [V], f there)"""
        c = idx[axis] + sign
        has = (c >= 0) & (c < dims[axis])
        other = np.where(has, lin + sign * step[axis], 0)
        return has & valid[other], fval[other]

    grad = np.zeros((V, 3), f)
    for m in range(3):
        hm, fm = neighbour(m, -1)
        hp, fp = neighbour(m, +1)
        both, po, mo = hm & hp, hp & ~hm, hm & ~hp
        grad[:, m] = np.where(both, (fp - fm) / (f(2.0) * vox), np.where(po, (fp - fval) / vox, np.where(mo, (fval - fm) / vox, f(0))))
    grad[~valid] = 0
    counts = np.zeros(V, np.int32)
    rows = []
    for ax in range(3):
        hb, fb = neighbour(ax, +1)
        cross = valid & hb & ((fval < 0) != (fb < 0))
        counts += cross
        a = lin[cross]
        rows.append((3 * a + ax, a, a + step[ax], np.full(len(a), ax)))
    eid = np.concatenate([r[0] for r in rows])
    order = np.argsort(eid, kind="stable")
    eid = eid[order]
    a, b, ax = (np.concatenate([r[q] for r in rows])[order] for q in (1, 2, 3))
    fa, fb = fval[a], fval[b]
    t = fa / (fa - fb)
    pts = np.stack([(idx[m][a].astype(f) + f(0.5)) * vox for m in range(3)], -1)
    pts[np.arange(len(a)), ax] = pts[np.arange(len(a)), ax] + t * vox
    g = (f(1.0) - t)[:, None] * grad[a] + t[:, None] * grad[b]
    with np.errstate(all="ignore"):
        length = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
        okn = (length > 0) & np.isfinite(length)
        normals = np.where(okn[:, None], g / length[:, None], f(0))
    out = dict(counts=counts, edge_id=eid, a=a, b=b, axis=ax, t=t, points=pts, normals=normals, g=g, colors=None, steps=step)
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
        out["unit_t"], out["vox"], out["centre_max"] = ut, float(vox), float(vox) * (max(dims) + 1)
        out["unit_point"] = ut * float(vox) + EPS * out["centre_max"]
        ga, gb = (np.linalg.norm(grad[q].astype(np.float64), axis=1) for q in (a, b))
        out["unit_normal"] = ((N[a] + N[b]) / float(vox) + ut * np.linalg.norm((grad[b] - grad[a]).astype(np.float64), axis=1)
                              + 4 * EPS * (ga + gb)) / glen + 4 * EPS
        out["end_clear"] = np.abs(S) > SIGN_CLEAR * U                     # per voxel
        out["sign_clear"] = out["end_clear"][a] & out["end_clear"][b]
        if C is not None and UC is not None:
            with np.errstate(all="ignore"):
                ec = np.where(valid[:, None], UC / Wt.astype(np.float64)[:, None], 0.0)
            out["unit_color"] = 2.0 * (ec[a] + ec[b]) + ut[:, None] * np.abs(cb - ca).astype(np.float64)
    return out


# ------------------------------------------------------------------------------------------------------------------
# fixtures
# ------------------------------------------------------------------------------------------------------------------
VOX = 0.0137
SPHERE_C, SPHERE_R = (0.01, -0.02, 0.0), 0.11
CAM_POS = [(0.55, 0.12, 0.2), (-0.3, 0.5, 0.1), (0.05, -0.35, 0.45)]
IMG = dict(W=53, H=41, fx=60.0, fy=60.0, cx=26.3, cy=20.9, near=0.01, pix_center=0.5)
PLANE_N = np.array([0.2, 0.1, 1.0]) / np.linalg.norm([0.2, 0.1, 1.0])
PLANE_H = -0.125
W_MIN = 0.5

GRIDS = {
    "sphere": dict(dims=(37, 29, 23), vox=VOX, origin=(-0.2531, -0.1987, -0.1579), trunc=3 * VOX),
    "aligned": dict(dims=(64, 8, 4), vox=0.006, origin=(-0.19, -0.047, 0.091), trunc=0.018),
    "thin_z": dict(dims=(1, 1, 5), vox=VOX, origin=(0.0033, -0.0271, 0.0789), trunc=3 * VOX),
    "thin_x": dict(dims=(130, 1, 1), vox=0.003, origin=(-0.1893, -0.0213, -0.0017), trunc=0.009),
}
FIXTURES = ("sphere", "plane_behind", "weights_rgb", "aligned", "thin_z", "thin_x", "behind")
ALL = FIXTURES + ("eight",)      # "eight": eight weighted, coloured views of the sphere-and-plane scene (batching, continuation)


def _pattern_rgb(W, H):
    us, vs = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([0.2 + 0.6 * us / W, 0.9 - 0.7 * vs / H, 0.5 + 0.4 * np.sin(0.3 * us + 0.2 * vs)], -1).astype(np.float32)


def sphere_views(plane=False, positions=CAM_POS, img=IMG):
    views = []
    for pos in positions:
        R, t = look_at(pos)
        geo = {k: img[k] for k in ("W", "H", "fx", "fy", "cx", "cy")}
        d = sphere_depth(R, t, **geo, centre=SPHERE_C, radius=SPHERE_R, pix_center=img["pix_center"])
        if plane:
            p = plane_depth(R, t, **geo, normal=PLANE_N, h=PLANE_H, pix_center=img["pix_center"])
            d = np.where((d > 0) & ((p <= 0) | (d < p)), d, p)
        views.append(dict(R=R, t=t, **img, depth=d.astype(np.float32), weight=None, rgb=_pattern_rgb(img["W"], img["H"])))
    return views


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> (grid, views).  The arrays are shared: do not modify them."""
    if name == "sphere":
        return GRIDS["sphere"], sphere_views()
    if name == "plane_behind":
        return GRIDS["sphere"], sphere_views(plane=True)
    if name == "weights_rgb":
        rng = np.random.default_rng(5)
        views = sphere_views(plane=True)
        for n, vw in enumerate(views):
            w = rng.uniform(0.0, 2.0, size=(vw["H"], vw["W"])).astype(np.float32)
            w[rng.random(w.shape) < 0.1] = 0.0
            if n == 1:
                w[vw["H"] // 2, vw["W"] // 2] = np.nan
            vw["weight"] = w
            vw["rgb"] = rng.random((vw["H"], vw["W"], 3)).astype(np.float32)
        return GRIDS["sphere"], views
    if name in ("aligned", "thin_z", "thin_x"):
        return GRIDS[name], sphere_views()
    if name == "behind":
        # one camera with the whole grid behind it, one that looks past it
        img = IMG
        away = look_at((0.55, 0.12, 0.2), target=(1.1, 0.24, 0.4))
        past = look_at((0.55, 0.12, 0.2), target=(0.55, 3.0, 0.2))
        views = []
        for R, t in (away, past):
            views.append(dict(R=R, t=t, **img, depth=np.full((img["H"], img["W"]), 0.5, np.float32), weight=None,
                              rgb=_pattern_rgb(img["W"], img["H"])))
        return GRIDS["sphere"], views
    if name == "eight":
        return eight_views()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64 state after the fixture's views, and its extraction with W_MIN.  Shared: do not modify."""
    grid, views = fixture(name)
    st = integrate(grid, views)
    ex = extract(grid, st["S"], st["Wt"], st["C"], W_MIN, U=st["U"], UC=st["UC"])
    return st, ex


@functools.lru_cache(maxsize=None)
def emulation(name):
    """The same in fp32 arithmetic."""
    grid, views = fixture(name)
    st = integrate(grid, views, dtype=np.float32)
    ex = extract(grid, st["S"], st["Wt"], st["C"], W_MIN, dtype=np.float32)
    return st, ex


def eight_views():
    """Eight views of the sphere-and-plane scene with weights and colours (batching, continuation): five poses, three of
    them used twice with other weights -- every pose adds its own 0.4 % of voxels within the pixel-edge margin, and eight
    distinct poses exceed the cap on the unclear share (3.3 %)."""
    rng = np.random.default_rng(11)
    pos = CAM_POS + [(0.4, -0.3, 0.3), (-0.45, -0.2, 0.25)] + CAM_POS
    views = sphere_views(plane=True, positions=pos)
    for vw in views:
        vw["weight"] = rng.uniform(0.1, 2.0, size=(vw["H"], vw["W"])).astype(np.float32)
    return GRIDS["sphere"], views


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
def state_errors(ref, S, Wt, C):
    """Largest error of a state against the reference on the CLEAR voxels, in units; and what the unclear ones do."""
    clear = ~ref["unclear"]
    S, Wt = np.asarray(S, dtype=np.float64), np.asarray(Wt, dtype=np.float64)

    def units(err, unit):
        with np.errstate(all="ignore"):
            r = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
        return r

    eS, eW = units(np.abs(S - ref["S"]), ref["U"]), units(np.abs(Wt - ref["Wt"]), EPS * ref["Wt"])
    fig = dict(S=float(eS[clear].max(initial=0.0)), Wt=float(eW[clear].max(initial=0.0)), clear=int(clear.sum()),
               unclear=int((~clear).sum()), unclear_share=float((~clear).mean()),
               unclear_differ=int(((eS > 64) | (eW > 64))[~clear].sum()), nonfinite=int((~np.isfinite(S)).sum() + (~np.isfinite(Wt)).sum()))
    if C is not None and ref["C"] is not None:
        eC = units(np.abs(np.asarray(C, dtype=np.float64) - ref["C"]), ref["UC"])
        fig["C"] = float(eC[clear].max(initial=0.0))
    return fig


def crossing_errors(ref_ex, got):
    """`got`: dict(edge_id, points, normals, colors | None), points grid-local.  Set comparison by edge_id and the errors on the
    common crossings, in units.  t is recovered from the point (the coordinate along the edge's axis)."""
    rid, gid = ref_ex["edge_id"], np.asarray(got["edge_id"])
    common, ri, gi = np.intersect1d(rid, gid, return_indices=True)
    missing = np.setdiff1d(rid, gid)
    extra = np.setdiff1d(gid, rid)
    sc = dict(zip(rid.tolist(), ref_ex["sign_clear"].tolist()))
    xa = extra // 3
    xb = xa + np.asarray(ref_ex["steps"])[extra % 3]
    fig = dict(ref=len(rid), got=len(gid), common=len(common),
               extra_clear=int((ref_ex["end_clear"][xa] & ref_ex["end_clear"][xb]).sum()) if len(extra) else 0,
               missing_clear=int(sum(sc[e] for e in missing.tolist())), missing_unclear=int(sum(not sc[e] for e in missing.tolist())),
               extra=extra, not_sign_clear_share=float((~ref_ex["sign_clear"]).mean()) if len(rid) else 0.0)
    if len(common):
        p = np.asarray(got["points"], dtype=np.float64)[gi]
        dp = np.abs(p - ref_ex["points"][ri]).max(1)
        fig["point"] = float((dp / ref_ex["unit_point"][ri]).max())
        fig["point_abs"] = float(dp.max())
        ax, rows = ref_ex["axis"][ri], np.arange(len(ri))
        dt = np.abs(p[rows, ax] - ref_ex["points"][ri][rows, ax]) / ref_ex["vox"]
        fig["t"] = float((dt / (ref_ex["unit_t"][ri] + EPS * (ref_ex["centre_max"] / ref_ex["vox"]))).max())
        n = np.asarray(got["normals"], dtype=np.float64)[gi]
        rn = ref_ex["normals"][ri]
        ang = np.arctan2(np.linalg.norm(np.cross(n, rn), axis=1), (n * rn).sum(1))     # (arccos loses half the digits near 0)
        zero = ~rn.any(1)
        fig["normal_zero_mismatch"] = int((zero != ~n.any(1)).sum())
        with np.errstate(all="ignore"):
            fig["normal"] = float(np.where(zero, 0.0, ang / ref_ex["unit_normal"][ri]).max())
        fig["normal_abs_deg"] = float(np.degrees(np.where(zero, 0.0, ang)).max())
        if got.get("colors") is not None and ref_ex["colors"] is not None:
            dc = np.abs(np.asarray(got["colors"], dtype=np.float64)[gi] - ref_ex["colors"][ri])
            with np.errstate(all="ignore"):
                fig["color"] = float(np.where(ref_ex["unit_color"][ri] > 0, dc / ref_ex["unit_color"][ri], np.where(dc == 0, 0, np.inf)).max())
    return fig


def read_ply(path):
    """A small reader of binary little-endian PLY files with one vertex element -> (names, structured array)."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = [int(l.split()[2]) for l in lines if l.startswith("element vertex")][0]
    kinds = {"float": "<f4", "uchar": "u1"}
    fields = [(l.split()[2], kinds[l.split()[1]]) for l in lines if l.startswith("property")]
    rec = np.frombuffer(body, dtype=fields)
    assert len(rec) == n
    return [f[0] for f in fields], rec
