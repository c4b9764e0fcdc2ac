"""Reference side of the GPIS render tests (include/tgs.h, tgs_gpis_render).

The reference is the code that exists: ``GPIS.render_depth`` and ``GPIS.predict`` on the CPU in fp64, plus
``GPIS.normal_at``.  This module holds

* the fixture: the cap-of-a-sphere fit of tests/test_cpu_plumbing.py::test_gpis_sphere (length scale 0.04, offset 0.01) with
  ``max_points`` 150 (n about 600), at the world origin and with the whole world moved by (3, -2, 5) m;
* the cases (image, intrinsics, stride, max_var) the CPU and the GPU tests share;
* ``render_depth_parent``: the body of ``render_depth`` as it was before the ``backend`` / ``return_normals`` arguments,
  verbatim, for the byte-identity test of the default path;
* ``march``: an INSTRUMENTED restatement of that body (same calls on the same arrays, so the same bits) that also keeps, per
  ray of the region, what the status decisions hang on: the smallest |m| among the march samples the ray visits, N . ray of
  the facing test, the distances of the two nearest touched points, the variance before the cut -- and the normal;
* ``images``: depth / var / normal images and the CLEAR / UNCLEAR classification from a march;
* ``emulate``: an all-fp32 NumPy emulation of the kernel's arithmetic (centred coordinates, squared differences, fp32
  exponentials; fp32 kernel values widened into an fp64 k^T Kinv k);
* ``compare``: the figures the bars are set on.

Every march is computed once per process and shared (``functools.lru_cache``); callers do not modify what they get.

A ray is UNCLEAR iff any march sample it visits has |m| < 1e-4 (50 x the fp32 mean error), or |N . ray + 0.05| < 1e-3, or its
two nearest touched points are within 1e-5 m of a tie, or |var - max_var| < 1e-4.  Bars (the feature's specification):
status agrees on every clear ray and differs on at most 0.5 % of the region's rays; depth <= 5e-5 m on clear common hits
(1 / 20 of the stored millimetre) and <= 1e-3 m on the other common hits; variance <= 2.5e-4 on common hits (a quarter of the
stored 1e-3); normal within 0.05 degrees of normal_at at the reference's crossing on common hits and exactly 0 elsewhere.
"""
import functools
import math

import numpy as np

M_CLEAR = 1e-4
FACING = -0.05
FACING_CLEAR = 1e-3
TIE_CLEAR = 1e-5
VAR_CLEAR = 1e-4
BAR_DEPTH_CLEAR = 5e-5
BAR_DEPTH = 1e-3
BAR_VAR = 2.5e-4
BAR_NORMAL_DEG = 0.05
BAR_STATUS_SHARE = 0.005
BAR_UNCLEAR_SHARE = 0.10
WORLD_SHIFT = np.array([3.0, -2.0, 5.0])


def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def world_pose(world: str) -> np.ndarray:
    """c2w (OpenGL axes) of the test camera: the identity at the origin, or moved with the world by WORLD_SHIFT and
    rotated about its own y (3 degrees) and z (25 degrees) axes -- the cap stays in view."""
    c2w = np.eye(4)
    if world == "moved":
        c2w[:3, :3] = _rot(1, 3.0) @ _rot(2, 25.0)
        c2w[:3, 3] = WORLD_SHIFT
    return c2w


@functools.lru_cache(maxsize=None)
def sphere_points(n_pts: int = 600):
    rng = np.random.default_rng(0)
    c, r = np.array([0.0, 0.0, -0.5]), 0.1            # sphere in front of an OpenGL camera at the origin
    th = np.arccos(1 - 0.35 * rng.random(n_pts))       # cap facing the camera (+z side of the sphere)
    ph = 2 * np.pi * rng.random(n_pts)
    n = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    return c + r * n, n


@functools.lru_cache(maxsize=None)
def sphere_fit(world: str = "origin", max_points: int = 150, n_pts: int = 600, drop: int = 0):
    """The fit of test_gpis_sphere with fewer points; ``world="moved"``: the same points translated by WORLD_SHIFT.
    ``drop``: the GP is refitted without its last ``drop`` observations (the fit's n is 4 n_p: this gives an odd n)."""
    from scipy.linalg import cho_factor, cho_solve
    from touch_gs_amd.gpis import GPIS, estimate_outward_normals
    pts, _ = sphere_points(n_pts)
    shift = WORLD_SHIFT if world == "moved" else np.zeros(3)
    pts = pts + shift
    normals = estimate_outward_normals(pts, np.broadcast_to(shift, pts.shape))
    gp = GPIS(length_scale=0.04, offset=0.01).fit(pts, normals, max_points=max_points, rng=np.random.default_rng(0))
    if drop:
        n_p = len(gp.P)
        assert len(gp.X) == 4 * n_p
        y = np.concatenate([np.zeros(n_p), np.full(n_p, gp.offset), np.full(n_p, -gp.offset), np.full(n_p, -2 * gp.offset)])
        gp.X, y = gp.X[:-drop], y[:-drop]
        K = gp._k(gp.X, gp.X)
        K[np.diag_indices_from(K)] += gp.sn2
        gp.chol = cho_factor(K, lower=True)
        gp.alpha = cho_solve(gp.chol, y)
    return gp


_CENTRE = dict(W=64, H=64, fx=120.0, fy=120.0, cx=32.0, cy=32.0, n_steps=64, near=0.05, far=1.0, world="origin", fit=(150, 0))
_UNALIGNED = dict(_CENTRE, W=37, H=29, fx=70.0, fy=70.0, cx=17.3, cy=15.9)
# n = 4 * 41 - 1 = 163 GP points (odd: the remainders of the kernel's unrolled loops and of its strips), n_p = 41
_SMALL_ODD = dict(_CENTRE, W=24, H=20, fx=45.0, fy=45.0, cx=12.2, cy=9.7, n_steps=48, fit=(41, 1))
_ONE_PIXEL = dict(_CENTRE, W=1, H=1, cx=0.5, cy=0.5)
# name -> (camera of the march, stride, max_var, var_floor)
CASES = {
    "centre": (_CENTRE, 1, None, 0.0),
    "centre_max_var": (_CENTRE, 1, 0.01, 1e-3),
    "unaligned": (_UNALIGNED, 1, None, 0.0),
    "unaligned_max_var": (_UNALIGNED, 1, 0.01, 1e-3),
    "centre_stride2": (_CENTRE, 2, 0.01, 1e-3),
    "moved": (dict(_CENTRE, world="moved"), 1, 0.01, 1e-3),
    "small_odd": (_SMALL_ODD, 1, None, 0.0),
    "one_pixel": (_ONE_PIXEL, 1, None, 0.0),
}


def render_kwargs(name: str) -> dict:
    """Arguments of ``GPIS.render_depth`` for a case (without backend / return_normals)."""
    cam, stride, max_var, var_floor = CASES[name]
    return dict(c2w_opengl=world_pose(cam["world"]), fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], W=cam["W"], H=cam["H"],
                near=cam["near"], far=cam["far"], n_steps=cam["n_steps"], stride=stride, max_var=max_var, var_floor=var_floor)


def _fit_of(cam: dict):
    return sphere_fit(cam["world"], cam["fit"][0], drop=cam["fit"][1])


def case_fit(name: str):
    return _fit_of(CASES[name][0])


def render_depth_parent(self, c2w_opengl, fx, fy, cx, cy, W, H, near=0.02, far=2.0, n_steps=None, stride=1, roi_margin_px=24,
                        chunk=20000, max_var=None, var_floor=0.0):
    """``GPIS.render_depth`` of the parent commit, verbatim."""
    c2w = np.asarray(c2w_opengl, dtype=np.float64)
    R = c2w[:3, :3] @ np.diag([1.0, -1.0, -1.0])  # OpenCV camera axes in the world
    t = c2w[:3, 3]
    depth = np.full((H, W), np.nan)
    var = np.full((H, W), np.nan)
    # region of interest: pixels near the projection of the observed surface points
    Pc = (self.P - t) @ R
    front = Pc[:, 2] > near
    if not front.any():
        return depth, var
    u = fx * Pc[front, 0] / Pc[front, 2] + cx
    v = fy * Pc[front, 1] / Pc[front, 2] + cy
    u0, u1 = int(max(0, np.floor(u.min()) - roi_margin_px)), int(min(W - 1, np.ceil(u.max()) + roi_margin_px))
    v0, v1 = int(max(0, np.floor(v.min()) - roi_margin_px)), int(min(H - 1, np.ceil(v.max()) + roi_margin_px))
    if u1 < u0 or v1 < v0:
        return depth, var
    zs_lo = max(near, Pc[front, 2].min() - 3 * self.l - self.offset)
    zs_hi = min(far, Pc[front, 2].max() + 3 * self.l + self.offset)
    us, vs = np.meshgrid(np.arange(u0, u1 + 1, stride), np.arange(v0, v1 + 1, stride))
    us, vs = us.ravel(), vs.ravel()
    dirs_c = np.stack([(us + 0.5 - cx) / fx, (vs + 0.5 - cy) / fy, np.ones_like(us, dtype=np.float64)], 1)
    if n_steps is None:
        n_steps = int(np.clip(np.ceil((zs_hi - zs_lo) / (0.6 * self.offset)), 16, 512))
    zgrid = np.linspace(zs_lo, zs_hi, n_steps)
    for s in range(0, len(us), chunk):
        dc = dirs_c[s:s + chunk]
        n = len(dc)
        dw = dc @ R.T
        prev = np.full(n, np.inf)
        z_lo = np.full(n, np.nan)
        z_hi = np.full(n, np.nan)
        done = np.zeros(n, dtype=bool)
        for z in zgrid:
            m, _ = self.predict(t + z * dw, want_var=False)
            hit = (~done) & (prev > 0) & (m <= 0) & np.isfinite(prev)
            z_lo[hit] = z - (zgrid[1] - zgrid[0])
            z_hi[hit] = z
            done |= hit
            prev = m
        idx = np.nonzero(done)[0]
        if len(idx) == 0:
            continue
        lo, hi = z_lo[idx], z_hi[idx]
        for _ in range(12):  # bisection on the posterior mean
            mid = 0.5 * (lo + hi)
            m, _ = self.predict(t + mid[:, None] * dw[idx], want_var=False)
            inside = m <= 0
            hi = np.where(inside, mid, hi)
            lo = np.where(inside, lo, mid)
        zhit = 0.5 * (lo + hi)
        _, vv = self.predict(t + zhit[:, None] * dw[idx], want_var=True)
        # facing test: outward normal of the touched point nearest to the crossing against the ray
        ph = t + zhit[:, None] * dw[idx]
        _, nn = self._tree().query(ph)
        sure = np.einsum("ij,ij->i", self.N[nn], dw[idx] / np.linalg.norm(dw[idx], axis=1, keepdims=True)) < -0.05
        if max_var is not None:
            sure &= vv <= max_var
        idx, zhit, vv = idx[sure], zhit[sure], vv[sure]
        depth[vs[s:s + chunk][idx], us[s:s + chunk][idx]] = zhit
        var[vs[s:s + chunk][idx], us[s:s + chunk][idx]] = np.maximum(vv, var_floor)
    return depth, var


def view_setup(gp, c2w_opengl, fx, fy, cx, cy, W, H, near, far, n_steps, roi_margin_px=24):
    """The per-view host part of render_depth: R, t, region of interest, march grid.  None if nothing is in front."""
    c2w = np.asarray(c2w_opengl, dtype=np.float64)
    R = c2w[:3, :3] @ np.diag([1.0, -1.0, -1.0])
    t = c2w[:3, 3]
    Pc = (gp.P - t) @ R
    front = Pc[:, 2] > near
    if not front.any():
        return None
    u = fx * Pc[front, 0] / Pc[front, 2] + cx
    v = fy * Pc[front, 1] / Pc[front, 2] + cy
    u0, u1 = int(max(0, np.floor(u.min()) - roi_margin_px)), int(min(W - 1, np.ceil(u.max()) + roi_margin_px))
    v0, v1 = int(max(0, np.floor(v.min()) - roi_margin_px)), int(min(H - 1, np.ceil(v.max()) + roi_margin_px))
    if u1 < u0 or v1 < v0:
        return None
    zs_lo = max(near, Pc[front, 2].min() - 3 * gp.l - gp.offset)
    zs_hi = min(far, Pc[front, 2].max() + 3 * gp.l + gp.offset)
    return dict(R=R, t=t, roi=(u0, v0, u1, v1), zgrid=np.linspace(zs_lo, zs_hi, n_steps), W=W, H=H, fx=fx, fy=fy, cx=cx, cy=cy)


def _rays(vs, stride=1):
    u0, v0, u1, v1 = vs["roi"]
    us, vv = np.meshgrid(np.arange(u0, u1 + 1, stride), np.arange(v0, v1 + 1, stride))
    return us.ravel(), vv.ravel()


# case -> the case whose camera (and so whose march) it shares
CAMERA_OF = {"centre": "centre", "centre_max_var": "centre", "centre_stride2": "centre", "unaligned": "unaligned",
             "unaligned_max_var": "unaligned", "moved": "moved", "small_odd": "small_odd", "one_pixel": "one_pixel"}


def march(name: str):
    """The instrumented fp64 march of every ray (stride 1) of the region of a case's camera; cases with the same camera
    share it.  -> dict of per-ray arrays (zhit, var, facing, near2, normal_c: crossing rays only, in the order of idx)."""
    return _march(CAMERA_OF[name])


@functools.lru_cache(maxsize=None)
def _march(camera_key: str):
    cam = CASES[camera_key][0]
    gp = _fit_of(cam)
    vs = view_setup(gp, world_pose(cam["world"]), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["W"], cam["H"], cam["near"],
                    cam["far"], cam["n_steps"])
    R, t, zgrid = vs["R"], vs["t"], vs["zgrid"]
    us, vv_ = _rays(vs)
    dirs_c = np.stack([(us + 0.5 - vs["cx"]) / vs["fx"], (vv_ + 0.5 - vs["cy"]) / vs["fy"], np.ones_like(us, dtype=np.float64)], 1)
    dw = dirs_c @ R.T
    n = len(dw)
    prev = np.full(n, np.inf)
    z_lo, z_hi = np.full(n, np.nan), np.full(n, np.nan)
    done = np.zeros(n, dtype=bool)
    min_abs = np.full(n, np.inf)
    for z in zgrid:
        m, _ = gp.predict(t + z * dw, want_var=False)
        min_abs = np.where(done, min_abs, np.minimum(min_abs, np.abs(m)))     # (the crossing sample itself is visited)
        hit = (~done) & (prev > 0) & (m <= 0) & np.isfinite(prev)
        z_lo[hit] = z - (zgrid[1] - zgrid[0])
        z_hi[hit] = z
        done |= hit
        prev = m
    idx = np.nonzero(done)[0]
    lo, hi = z_lo[idx], z_hi[idx]
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        m, _ = gp.predict(t + mid[:, None] * dw[idx], want_var=False)
        inside = m <= 0
        hi = np.where(inside, mid, hi)
        lo = np.where(inside, lo, mid)
    zhit = 0.5 * (lo + hi)
    ph = t + zhit[:, None] * dw[idx]
    _, vv = gp.predict(ph, want_var=True)
    d2, nn2 = gp._tree().query(ph, k=2)
    unit = dw[idx] / np.linalg.norm(dw[idx], axis=1, keepdims=True)
    facing = np.einsum("ij,ij->i", gp.N[nn2[:, 0]], unit)
    normal_c = gp.normal_at(ph) @ R
    return dict(view=vs, us=us, vs=vv_, crossing=done, min_abs=min_abs, idx=idx, zhit=zhit, var=vv, facing=facing,
                near2=d2, normal_c=normal_c)


def images(name: str, mar=None):
    """Reference images of a case from its march: depth, var [H,W] fp64 (NaN = no surface), normal [H,W,3] (0 = none), and
    the masks region (the rays the case renders), unclear."""
    cam, stride, max_var, var_floor = CASES[name]
    mar = march(name) if mar is None else mar
    vs = mar["view"]
    H, W = vs["H"], vs["W"]
    u0, v0, _, _ = vs["roi"]
    us, vv_ = mar["us"], mar["vs"]
    on_grid = ((us - u0) % stride == 0) & ((vv_ - v0) % stride == 0)
    region = np.zeros((H, W), dtype=bool)
    region[vv_[on_grid], us[on_grid]] = True
    unclear_ray = mar["min_abs"] < M_CLEAR
    idx = mar["idx"]
    unc_x = (np.abs(mar["facing"] - FACING) < FACING_CLEAR) | (np.abs(mar["near2"][:, 1] - mar["near2"][:, 0]) < TIE_CLEAR)
    sure = mar["facing"] < FACING
    if max_var is not None:
        unc_x |= np.abs(mar["var"] - max_var) < VAR_CLEAR
        sure = sure & (mar["var"] <= max_var)
    unclear_ray = unclear_ray.copy()
    unclear_ray[idx] |= unc_x
    unclear = np.zeros((H, W), dtype=bool)
    unclear[vv_[on_grid], us[on_grid]] = unclear_ray[on_grid]
    depth, var, normal = np.full((H, W), np.nan), np.full((H, W), np.nan), np.zeros((H, W, 3))
    keep = sure & on_grid[idx]
    y, x = vv_[idx][keep], us[idx][keep]
    depth[y, x] = mar["zhit"][keep]
    var[y, x] = np.maximum(mar["var"][keep], var_floor)
    normal[y, x] = mar["normal_c"][keep]
    return dict(depth=depth, var=var, normal=normal, region=region, unclear=unclear)


# ------------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic in NumPy fp32
# ------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float32)


class Fp32Gp:
    """The inputs tgs_gpis_render gets (centred in fp64, then rounded) and its per-point arithmetic."""

    def __init__(self, gp):
        from scipy.linalg import cho_solve
        self.centre = gp.P.mean(axis=0)
        self.X, self.alpha = _f32(gp.X - self.centre), _f32(gp.alpha)
        self.P, self.N = _f32(gp.P - self.centre), _f32(gp.N)
        self.Kinv = cho_solve(gp.chol, np.eye(len(gp.X)))
        self.c_exp = np.float32(-1.4426950408889634 / (2.0 * gp.l * gp.l))
        self.inv_l2 = np.float32(1.0 / (gp.l * gp.l))
        self.sf2, self.prior = np.float32(gp.sf2), np.float32(gp.prior)

    def e(self, q):
        D = q[:, None, :] - self.X[None, :, :]
        return np.exp2(self.c_exp * ((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2])), D

    @staticmethod
    def blocked_sum(T):
        """Sum over axis 1 the way the kernel sums: fp32 inside blocks of 8 consecutive points, fp64 across the blocks."""
        pad = (-T.shape[1]) % 8
        T = np.concatenate([T, np.zeros((T.shape[0], pad) + T.shape[2:], dtype=np.float32)], axis=1)
        part = T.reshape((T.shape[0], -1, 8) + T.shape[2:]).sum(axis=2, dtype=np.float32)
        return part.astype(np.float64).sum(axis=1).astype(np.float32)

    def mean(self, q):
        E, _ = self.e(q)
        return self.sf2 * self.blocked_sum(E * self.alpha[None, :]) + self.prior * (np.float32(1) - E.max(axis=1))


def emulate(name: str):
    """depth, var, normal images of a case from the fp32 emulation (var: fp32 kernel values widened, fp64 quadratic form)."""
    cam, stride, max_var, var_floor = CASES[name]
    gp = _fit_of(cam)
    vs = view_setup(gp, world_pose(cam["world"]), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["W"], cam["H"], cam["near"],
                    cam["far"], cam["n_steps"])
    f = Fp32Gp(gp)
    R, t = _f32(vs["R"]), _f32(vs["t"] - f.centre)
    H, W = vs["H"], vs["W"]
    us, vv_ = _rays(vs, stride)
    dx = (_f32(us) + np.float32(0.5) - np.float32(vs["cx"])) / np.float32(vs["fx"])
    dy = (_f32(vv_) + np.float32(0.5) - np.float32(vs["cy"])) / np.float32(vs["fy"])
    d = np.stack([R[i, 0] * dx + (R[i, 1] * dy + R[i, 2]) for i in range(3)], 1)
    z0, dz = np.float32(vs["zgrid"][0]), np.float32((vs["zgrid"][-1] - vs["zgrid"][0]) / (len(vs["zgrid"]) - 1))
    n = len(d)
    prev = np.zeros(n, dtype=np.float32)
    z_hi = np.zeros(n, dtype=np.float32)
    done = np.zeros(n, dtype=bool)
    for k in range(len(vs["zgrid"])):
        z = np.float32(k) * dz + z0
        m = f.mean(t + z * d)
        hit = (~done) & (prev > 0) & (m <= 0) & (k > 0)
        z_hi[hit] = z
        done |= hit
        prev = m
    idx = np.nonzero(done)[0]
    lo, hi = z_hi[idx] - dz, z_hi[idx]
    for _ in range(12):
        mid = np.float32(0.5) * (lo + hi)
        inside = f.mean(t + mid[:, None] * d[idx]) <= 0
        hi = np.where(inside, mid, hi)
        lo = np.where(inside, lo, mid)
    zhit = np.float32(0.5) * (lo + hi)
    q = t + zhit[:, None] * d[idx]
    Dp = q[:, None, :] - f.P[None, :, :]
    nn = ((Dp[..., 0] * Dp[..., 0] + Dp[..., 1] * Dp[..., 1]) + Dp[..., 2] * Dp[..., 2]).argmin(axis=1)
    facing = (f.N[nn] * d[idx]).sum(1) / np.sqrt((d[idx] * d[idx]).sum(1))
    E, D = f.e(q)
    k64 = (f.sf2 * E).astype(np.float64)
    vv = np.maximum(float(f.sf2) - np.einsum("ij,jk,ik->i", k64, f.Kinv, k64), 0.0)
    J = E.argmax(axis=1)
    r = np.arange(len(J))
    g = (f.sf2 * f.inv_l2) * f.blocked_sum((E * f.alpha[None, :])[..., None] * -D) - (f.prior * f.inv_l2 * E[r, J])[:, None] * -D[r, J]
    nc = g @ R
    nc = nc / np.linalg.norm(nc, axis=1, keepdims=True)
    sure = facing < np.float32(FACING)
    if max_var is not None:
        sure &= vv <= np.float32(max_var)
    depth, var, normal = np.full((H, W), np.nan), np.full((H, W), np.nan), np.zeros((H, W, 3))
    y, x = vv_[idx][sure], us[idx][sure]
    depth[y, x] = zhit[sure]
    var[y, x] = np.maximum(vv[sure], np.float32(var_floor)).astype(np.float32)
    normal[y, x] = nc[sure]
    return dict(depth=depth, var=var, normal=normal)


def compare(ref: dict, depth, var, normal) -> dict:
    """Figures of a rendered (depth, var, normal) against ``images(...)``.  ``normal`` may be None."""
    depth, var = np.asarray(depth, dtype=np.float64), np.asarray(var, dtype=np.float64)
    region, unclear = ref["region"], ref["unclear"]
    hit_r, hit_g = np.isfinite(ref["depth"]), np.isfinite(depth)
    both = hit_r & hit_g
    differ = hit_r != hit_g
    err_d = np.abs(depth - ref["depth"])
    out = dict(rays=int(region.sum()), hits=int(hit_r.sum()), common_hits=int(both.sum()),
               unclear_share=float((unclear & region).sum() / max(region.sum(), 1)),
               outside_region_hits=int((hit_g & ~region).sum()),
               var_nan_mismatch=int((np.isfinite(var) != hit_g).sum()),
               status_diff_clear=int((differ & ~unclear).sum()), status_diff=int(differ.sum()),
               status_diff_share=float(differ.sum() / max(region.sum(), 1)),
               depth_clear=float(err_d[both & ~unclear].max()) if (both & ~unclear).any() else 0.0,
               depth_other=float(err_d[both & unclear].max()) if (both & unclear).any() else 0.0,
               var=float(np.abs(var - ref["var"])[both].max()) if both.any() else 0.0)
    if normal is not None:
        normal = np.asarray(normal, dtype=np.float64)
        cosang = np.clip((normal[both] * ref["normal"][both]).sum(-1), -1.0, 1.0)
        # the angle from the chord: acos loses half the digits near 0
        chord = np.linalg.norm(normal[both] - ref["normal"][both], axis=-1)
        out["normal_deg"] = float(np.degrees(2.0 * np.arcsin(np.clip(chord / 2.0, 0.0, 1.0))).max()) if both.any() else 0.0
        out["normal_unit_err"] = float(np.abs(np.linalg.norm(normal[both], axis=-1) - 1.0).max()) if both.any() else 0.0
        out["normal_nonzero_off_hits"] = int((normal[~hit_g] != 0).any(axis=-1).sum())
        del cosang
    return out


def check(fig: dict, with_normals: bool = True):
    """The bars, asserted."""
    assert fig["outside_region_hits"] == 0 and fig["var_nan_mismatch"] == 0, fig
    assert fig["status_diff_clear"] == 0, fig
    assert fig["status_diff_share"] <= BAR_STATUS_SHARE, fig
    assert fig["depth_clear"] <= BAR_DEPTH_CLEAR, fig
    assert fig["depth_other"] <= BAR_DEPTH, fig
    assert fig["var"] <= BAR_VAR, fig
    if with_normals:
        assert fig["normal_deg"] <= BAR_NORMAL_DEG, fig
        assert fig["normal_unit_err"] <= 1e-5, fig
        assert fig["normal_nonzero_off_hits"] == 0, fig


def report(name: str, fig: dict) -> str:
    s = (f"{name}: rays {fig['rays']} hits {fig['hits']} unclear {fig['unclear_share']:.3%} | status diff {fig['status_diff']} "
         f"({fig['status_diff_clear']} clear; bar {BAR_STATUS_SHARE:.1%}) | depth clear {fig['depth_clear']:.2e} (bar {BAR_DEPTH_CLEAR:.0e}) "
         f"other {fig['depth_other']:.2e} (bar {BAR_DEPTH:.0e}) | var {fig['var']:.2e} (bar {BAR_VAR:.1e})")
    if "normal_deg" in fig:
        s += f" | normal {fig['normal_deg']:.4f} deg (bar {BAR_NORMAL_DEG})"
    return s
