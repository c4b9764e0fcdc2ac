"""Constructed cases for the projection kernels K1 / K8 / K8a (project.hip) -- CPU only, deterministic, seeded.

Every parameter and every camera entry a case holds is EXACTLY representable in fp32: it is rounded first, and the very
same values go to the kernel and to the fp64 oracle.  Whatever difference remains is then the kernel's arithmetic, not
the rounding of its inputs (tests/test_gpu_parity.py::test_project_fwd feeds unrounded fp64 to the oracle).

A *case* is one launch: parameters, camera, SH degree / storage width, glob_scale.  Its Gaussians are grouped into
named *tags* (index arrays) that say which branch each of them was built for; tests/test_cpu_project_cases.py checks
from fp64 quantities that every tag holds what its name says and that RefC("f32") and RefC("f64") take the same integer
decisions on every constructed Gaussian -- the condition under which the GPU test may demand exact integers.

Units (all from fp64 quantities, see `geometry`):
  m_ij    = sum_kl |Tm_ik| |Sigma3_kl| |Tm_jl| + blur      the un-cancelled magnitude of the 2x2 covariance
  kappa   = max(1, (m00 m11 + m01^2) / det)                 how much of the determinant's terms cancels
  u_conic = 2^-24 kappa max|conic|
  u_rgb   = 2^-24 (sum_k |Y_k c_k| + 0.5),  u_depth = 2^-24 (sum_j |R_2j m_j| + |t_2|)     un-cancelled sums again
  gradient unit = 2^-24 kappa mass,  mass = tests.util.param_mass (the oracle's |J| column by column); for v_quats plus
                  mass(v_log_scales) / |q| (grad_mass says why)
"""
import dataclasses
import functools
import math

import numpy as np
import torch

from oracle import torch_oracle as O
from oracle.ref_c import RefC
from tests.util import PARAM_KEYS, param_mass

EPS32 = 2.0 ** -24
BLUR = 0.3
NEAR = float(np.float32(0.01))
SH_C0 = 0.28209479177387814


def f32(a):
    """Round to fp32, keep as fp64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------------------------
def camera(W, H, view=1, nviews=8, skew=False, identity=False):
    """Orbit camera whose every entry is an fp32 number: the rotation is built from fp32-rounded cos / sin, the
    translation is rounded after it is formed from that rotation.  skew: the off-centre intrinsics of
    tests/test_gpu_fullsize_oracle.py's skewed case."""
    fx = fy = (W / 2) / math.tan(math.radians(30.0))
    cx, cy = W / 2, H / 2
    if skew:
        fx, cx, cy = 1.15 * fx, cx + 37.0, cy - 21.5
    M = np.eye(4)
    if not identity:
        th = 2 * math.pi * view / nviews
        c, s = float(np.float32(math.cos(th))), float(np.float32(math.sin(th)))
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        ctr = np.array([0.0, 0.0, 4.0])
        M[:3, :3] = R
        M[:3, 3] = f32(ctr - R @ ctr)
    return O.Camera(viewmat=torch.from_numpy(M), fx=float(np.float32(fx)), fy=float(np.float32(fy)),
                    cx=float(np.float32(cx)), cy=float(np.float32(cy)), W=W, H=H, near=NEAR, bg=(0.0, 0.0, 0.0))


def cam_parts(cam):
    V = cam.viewmat.numpy().astype(np.float64)
    return V[:3, :3], V[:3, 3]


def place(cam, tcam):
    """World means (fp32 numbers) whose camera-space position is `tcam` up to the rounding of the mean."""
    Rw, tw = cam_parts(cam)
    return f32(np.linalg.solve(Rw, (np.asarray(tcam, np.float64) - tw).T).T)


def quat_mul(a, b):
    w1, x1, y1, z1 = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    w2, x2, y2, z2 = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def quat_from_rot(R):
    """One rotation matrix -> (w, x, y, z); trace > -1 is enough for the rotations used here."""
    w = 0.5 * math.sqrt(max(1e-300, 1 + R[0, 0] + R[1, 1] + R[2, 2]))
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def quat_between(a, b):
    """Quaternion turning unit vector a into unit vector b (a != -b)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    q = np.concatenate([[1 + a @ b], np.cross(a, b)])
    return q / np.linalg.norm(q)


# ---------------------------------------------------------------------------------------------
# the case
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    P: dict                 # means [N,3], log_scales [N,3], quats [N,4], opac_logit [N], sh [N,Ks,3] or None -- fp64 holding fp32 numbers
    cam: O.Camera
    deg: int                # active SH degree, -1 = no SH
    tags: dict              # tag -> index array
    glob_scale: float = 1.0
    constructed: bool = True   # False: random fill, 0.5 % of the integer decisions may differ between fp32 and fp64
    k1_only: bool = False

    @property
    def N(self):
        return self.P["means"].shape[0]

    @property
    def Ks(self):
        return 0 if self.P["sh"] is None else self.P["sh"].shape[1]

    def take(self, idx, name=None):
        idx = np.asarray(idx)
        inv = -np.ones(self.N, np.int64)
        inv[idx] = np.arange(len(idx))
        tags = {k: inv[v][inv[v] >= 0] for k, v in self.tags.items()}
        P = {k: (None if v is None else np.ascontiguousarray(v[idx])) for k, v in self.P.items()}
        return dataclasses.replace(self, name=name or self.name, P=P, tags=tags)

    def torch_params(self):
        return {k: (None if v is None else torch.from_numpy(v.copy())) for k, v in self.P.items()}

    def amd_cam(self, **kw):
        from touch_gs_amd import Camera
        c = self.cam
        return Camera(c.viewmat.numpy(), c.fx, c.fy, c.cx, c.cy, c.W, c.H, c.near, c.pix_center, c.bg,
                      glob_scale=self.glob_scale, **kw)


def generic(n, cam, seed, deg=3, Ks=16):
    """n Gaussians of the project's synthetic scene (S(N,W,H,deg,seed)), rounded to fp32, SH rows widened to Ks bases.
    The scene lives in the frame of view 0, so under an orbit view some of it is off screen or behind the camera."""
    P, _ = O.synthetic_scene(n, cam.W, cam.H, max(deg, 0), seed)
    P = {k: f32(v.numpy()) for k, v in P.items()}
    if deg < 0:
        P["sh"] = None
    else:
        sh = np.zeros((n, Ks, 3))
        K = (deg + 1) ** 2
        sh[:, :K] = P["sh"]
        if Ks > K:    # rows above the active degree hold values that must not be read
            sh[:, K:] = f32(np.random.default_rng(seed).normal(size=(n, Ks - K, 3)))
        P["sh"] = sh
    return P


def on_screen(n, cam, rng, z=(2.0, 5.0), frac=0.85):
    """Camera-space positions inside the image (|u| < frac * half size)."""
    tz = rng.uniform(*z, n)
    tx = rng.uniform(-frac, frac, n) * (cam.W / 2) / cam.fx * tz
    ty = rng.uniform(-frac, frac, n) * (cam.H / 2) / cam.fy * tz
    return np.stack([tx, ty, tz], 1)


def concat(name, cases, **kw):
    P, tags, off = {}, {}, 0
    for k in cases[0].P:
        P[k] = None if cases[0].P[k] is None else np.concatenate([c.P[k] for c in cases])
    for c in cases:
        tags[c.name] = np.arange(off, off + c.N)
        for t, idx in c.tags.items():
            tags[f"{c.name}/{t}"] = idx + off
        off += c.N
    return dataclasses.replace(cases[0], name=name, P=P, tags=tags, **kw)


# ---------------------------------------------------------------------------------------------
# fp64 geometry: everything the strata and the units are defined by
# ---------------------------------------------------------------------------------------------
def geometry(case):
    P, cam = case.P, case.cam
    Rw, tw = cam_parts(cam)
    m = P["means"]
    t = m @ Rw.T + tw
    tx, ty, tz = t.T
    front = tz > cam.near
    tzs = np.where(front, tz, 1.0)
    q = P["quats"] / np.linalg.norm(P["quats"], axis=1, keepdims=True)
    w, x, y, z = q.T
    Rq = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                   2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    s = np.exp(P["log_scales"]) * case.glob_scale
    M = Rq * s[:, None, :]
    Sig = M @ M.transpose(0, 2, 1)
    limx, limy = 1.3 * (cam.W / 2) / cam.fx, 1.3 * (cam.H / 2) / cam.fy
    ux, uy = tx / tzs, ty / tzs
    ucx, ucy = np.clip(ux, -limx, limx), np.clip(uy, -limy, limy)
    zero = np.zeros_like(tz)
    J = np.stack([cam.fx / tzs, zero, -cam.fx * ucx / tzs, zero, cam.fy / tzs, -cam.fy * ucy / tzs], 1).reshape(-1, 2, 3)
    Tm = J @ Rw
    cov = Tm @ Sig @ Tm.transpose(0, 2, 1)
    c00, c01, c11 = cov[:, 0, 0] + BLUR, cov[:, 0, 1], cov[:, 1, 1] + BLUR
    det = c00 * c11 - c01 * c01
    mag = np.abs(Tm) @ np.abs(Sig) @ np.abs(Tm).transpose(0, 2, 1)
    m00, m01, m11 = mag[:, 0, 0] + BLUR, mag[:, 0, 1], mag[:, 1, 1] + BLUR
    kappa = np.maximum(1.0, (m00 * m11 + m01 * m01) / np.where(det > 0, det, 1.0))
    mid = 0.5 * (c00 + c11)
    disc = mid * mid - det
    lam1 = mid + np.sqrt(np.maximum(disc, 0.1))
    conic = np.stack([c11, -c01, c00], 1) / np.where(det > 0, det, 1.0)[:, None]
    xy = np.stack([cam.fx * tx / tzs + cam.cx, cam.fy * ty / tzs + cam.cy], 1)
    u_depth = EPS32 * (np.abs(m * Rw[2]).sum(1) + abs(tw[2]))
    out = dict(t=t, front=front, ux=ux, uy=uy, limx=limx, limy=limy, Tm=Tm, Sig=Sig, c00=c00, c01=c01, c11=c11, det=det,
               kappa=kappa, disc=disc, r3=3 * np.sqrt(lam1), conic=conic, xy=xy, u_depth=u_depth,
               u_conic=EPS32 * kappa * np.abs(conic).max(1), opac=1 / (1 + np.exp(-P["opac_logit"])))
    if P["sh"] is not None:
        Rinv_t = -(Rw.T @ tw)
        d = m - Rinv_t
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        K = (case.deg + 1) ** 2
        Y = O.sh_basis(case.deg, torch.from_numpy(d)).numpy()
        terms = Y[:, :, None] * P["sh"][:, :K]
        out.update(dir=d, Y=Y, pre=terms.sum(1) + 0.5, u_rgb=EPS32 * (np.abs(terms).sum(1) + 0.5))
    return out


def sigmoid_deriv(x):
    """d sigmoid / d logit in fp64 without the cancellation of o (1 - o)."""
    t = np.exp(-np.abs(np.asarray(x, np.float64)))
    return t / (1 + t) ** 2


def settle(case, rounds=40, how="scales"):
    """Nudge the builder: a constructed Gaussian whose radius (ceil of 3 sqrt(lam1)) or tile-rect edges sit within fp32
    noise of an integer gets all three log-scales raised by 2^-6 (so that isotropy and aspect ratios stay exact) until
    no integer decision is near its threshold; how="depth" moves it 2^-6 further along its view ray instead (where
    the log-scales themselves are the point of the stratum).  The margins are generous multiples of the fp32 error."""
    P = case.P
    for _ in range(rounds):
        g = geometry(case)
        r3 = g["r3"]
        near_int = np.abs(r3 - np.round(r3)) < np.minimum(256 * EPS32 * g["kappa"] * r3, 0.05) + 1e-4
        rad = np.ceil(r3)
        for c, T in enumerate(case.cam.tiles):
            for sgn in (-1.0, 1.0):
                e = (g["xy"][:, c] + sgn * rad) / 16.0
                live = (e > -1.5) & (e < T + 1.5)          # beyond that the clamp to [0, T] decides, not the truncation
                near_int |= live & (np.abs(e - np.round(e)) < 64 * EPS32 * (np.abs(g["xy"][:, c]) + rad) / 16.0 + 1e-4)
        near_int &= g["front"] & (g["det"] > 0)
        if not near_int.any():
            return case
        if how == "depth":
            P["means"][near_int] = place(case.cam, g["t"][near_int] * (1 + 2.0 ** -6))
        else:
            P["log_scales"][near_int] = f32(P["log_scales"][near_int] + 2.0 ** -6)
    raise AssertionError(f"{case.name}: could not move {int(near_int.sum())} Gaussians off their integer thresholds")


# ---------------------------------------------------------------------------------------------
# strata
# ---------------------------------------------------------------------------------------------
W0, H0 = 160, 96


def _fill():
    cam = camera(W0, H0)
    return Case("fill", generic(1024, cam, 101), cam, 3, dict(all=np.arange(1024)), constructed=False)


def _near():
    """tz = near (1 +- 2^-k), k = 4..20, and tz <= 0.  The rotation is the identity so that tz IS the mean's z: an fp32
    mean under an orbit camera cannot sit closer to the plane than its own ulp (2^-15 near)."""
    cam = camera(W0, H0, identity=True)
    rng = np.random.default_rng(11)
    tz, tag = [], []
    for k in range(4, 21):
        for rep in range(2):
            tz += [NEAR * (1 + 2.0 ** -k), NEAR * (1 - 2.0 ** -k)]
            tag += ["front", "behind"]
    tz += [NEAR, 0.0, -NEAR, -1.0, -3.0, -NEAR * (1 + 2.0 ** -20)]
    tag += ["on", "zero", "neg", "neg", "neg", "neg"]
    tz = f32(tz)
    n = len(tz)
    u = rng.uniform(-0.4, 0.4, (n, 2))
    means = f32(np.stack([u[:, 0] * np.abs(tz) + 1e-4, u[:, 1] * np.abs(tz) - 1e-4, tz], 1))
    means[:, 2] = tz
    P = generic(n, cam, 12)
    P["means"] = means
    P["log_scales"] = f32(math.log(1e-3) + 0.3 * rng.normal(size=(n, 3)))   # ~8 px at tz = near
    tag = np.array(tag)
    return settle(Case("near", P, cam, 3, {t: np.nonzero(tag == t)[0] for t in np.unique(tag)}))


CLAMP_FACTORS = (0.9, 0.999, 1.001, 1.1, 2.0)


def _clamp():
    cam = camera(W0, H0)
    rng = np.random.default_rng(21)
    limx, limy = 1.3 * (cam.W / 2) / cam.fx, 1.3 * (cam.H / 2) / cam.fy
    rows, tag = [], []
    for f in CLAMP_FACTORS:
        for sx in (-1, 1):
            for rep in range(2):
                rows.append((sx * f * limx, rng.uniform(-0.5, 0.5) * limy)); tag.append(f"x{'+' if sx > 0 else '-'}{f}")
                rows.append((rng.uniform(-0.5, 0.5) * limx, sx * f * limy)); tag.append(f"y{'+' if sx > 0 else '-'}{f}")
            for sy in (-1, 1):
                rows.append((sx * f * limx, sy * f * limy)); tag.append(f"xy{'+' if sx > 0 else '-'}{'+' if sy > 0 else '-'}{f}")
    u = np.array(rows)
    n = len(u)
    tz = rng.uniform(2.0, 5.0, n)
    P = generic(n, cam, 22)
    P["means"] = place(cam, np.stack([u[:, 0] * tz, u[:, 1] * tz, tz], 1))
    P["log_scales"] = f32(np.log(45.0 * tz / cam.fx)[:, None] + 0.3 * rng.normal(size=(n, 3)))   # ~45 px: reaches the image
    P["opac_logit"] = f32(rng.uniform(0.0, 3.0, n))
    tag = np.array(tag)
    return settle(Case("clamp", P, cam, 3, {t: np.nonzero(tag == t)[0] for t in np.unique(tag)}))


OPACITY_LOGITS = (-30.0, -12.0, -5.6, -5.5, 0.0, 5.0, 12.0, 17.0, 30.0)


def _opacity():
    cam = camera(W0, H0)
    rng = np.random.default_rng(31)
    per = 7
    n = per * len(OPACITY_LOGITS)
    P = generic(n, cam, 32)
    P["means"] = place(cam, on_screen(n, cam, rng))
    P["opac_logit"] = f32(np.repeat(OPACITY_LOGITS, per))
    return settle(Case("opacity", P, cam, 3, {f"{l:g}": np.arange(i * per, (i + 1) * per) for i, l in enumerate(OPACITY_LOGITS)}))


GATE_LEVELS = (-0.2, -1e-3, 1e-3, 0.2)


def _gate():
    """Pre-clamp colour of each channel, independently, at one of GATE_LEVELS: degree 3, non-zero higher rows, the DC
    coefficient solved for in fp64 and then rounded (its rounding moves the colour by 3e-8, the levels are >= 1e-3)."""
    cam = camera(W0, H0)
    rng = np.random.default_rng(41)
    lv = np.array([(a, b, c) for a in GATE_LEVELS for b in GATE_LEVELS for c in GATE_LEVELS])
    n = len(lv)
    P = generic(n, cam, 42)
    P["means"] = place(cam, on_screen(n, cam, rng))
    P["sh"][:, 1:] = f32(0.05 * rng.normal(size=(n, 15, 3)))
    c = Case("gate", P, cam, 3, {})
    g = geometry(c)
    rest = (g["Y"][:, 1:, None] * P["sh"][:, 1:16]).sum(1)
    P["sh"][:, 0] = f32((lv - 0.5 - rest) / SH_C0)
    c.tags = {f"ch{ch}_{l:g}": np.nonzero(lv[:, ch] == l)[0] for ch in range(3) for l in GATE_LEVELS}
    c.tags["levels"] = np.arange(n)
    return settle(c)


QUAT_NORMS = (1e-3, 0.1, 1.0, 10.0, 1e3)


def _quat():
    cam = camera(W0, H0)
    rng = np.random.default_rng(51)
    per = 13
    n = per * len(QUAT_NORMS)
    P = generic(n, cam, 52)
    P["means"] = place(cam, on_screen(n, cam, rng))
    d = rng.normal(size=(n, 4))
    d[0::per, 0] = 0.0            # w exactly 0
    d[1::per, 0] = 1e-8           # w ~ 0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P["quats"] = f32(d * np.repeat(QUAT_NORMS, per)[:, None])
    P["log_scales"] = f32(np.log(8.0 * 3.5 / cam.fx) + rng.normal(size=(n, 3)) * np.array([0.9, 0.3, 0.3]))   # anisotropic: the rotation matters
    tags = {f"{q:g}": np.arange(i * per, (i + 1) * per) for i, q in enumerate(QUAT_NORMS)}
    tags["w0"] = np.arange(0, n, per)
    return settle(Case("quat", P, cam, 3, tags))


def _shape():
    cam = camera(W0, H0)
    Rw, _ = cam_parts(cam)
    q_cam = quat_from_rot(Rw.T)            # camera axes -> world
    rng = np.random.default_rng(61)
    per = 8
    blocks, tags, off = [], {}, 0

    def add(tag, tcam, ls, q):
        nonlocal off
        n = len(tcam)
        blocks.append((place(cam, tcam), f32(ls), f32(q)))
        tags[tag] = np.arange(off, off + n)
        off += n

    for ang in (0.0, 45.0, 89.0):          # in-plane needles 100:1: long axis in the image plane, turned about the view axis
        tc = on_screen(per, cam, rng, frac=0.5)
        a = math.radians(ang) / 2
        q = quat_mul(q_cam, np.array([math.cos(a), 0.0, 0.0, math.sin(a)]))
        s_short = 0.6 * tc[:, 2] / cam.fx
        add(f"needle{ang:g}", tc, np.log(np.stack([100 * s_short, s_short, s_short], 1)), np.tile(q, (per, 1)))
    tc = on_screen(per, cam, rng)          # exactly isotropic, sigma 0.01 px: blur dominates, the 0.1 floor is active
    s = f32(np.log(0.01 * tc[:, 2] / cam.fx))
    add("iso", tc, np.stack([s, s, s], 1), rng.normal(size=(per, 4)))
    tc = on_screen(per, cam, rng)          # sigma 1000 px
    add("huge", tc, np.log(1000.0 * tc[:, 2] / cam.fx)[:, None] + 0.2 * rng.normal(size=(per, 3)), rng.normal(size=(per, 4)))
    # ray: 100:1 elongation ALONG the view ray, near the four image corners
    corners = np.array([(sx * 0.9, sy * 0.9) for sx in (-1, 1) for sy in (-1, 1)] * 2)
    tz = rng.uniform(2.5, 4.5, per)
    tc = np.stack([corners[:, 0] * (cam.W / 2) / cam.fx * tz, corners[:, 1] * (cam.H / 2) / cam.fy * tz, tz], 1)
    qs = np.stack([quat_mul(q_cam, quat_between([0, 0, 1.0], r / np.linalg.norm(r))) for r in tc])
    s_short = 1.5 * tz / cam.fx
    add("ray", tc, np.log(np.stack([s_short, s_short, 100 * s_short], 1)), qs)
    n = off
    P = generic(n, cam, 62)
    P["means"] = np.concatenate([b[0] for b in blocks])
    P["log_scales"] = np.concatenate([b[1] for b in blocks])
    P["quats"] = np.concatenate([b[2] for b in blocks])
    P["opac_logit"] = f32(rng.uniform(-1.0, 3.0, n))
    return settle(Case("shape", P, cam, 3, tags))


def _scale(glob_scale):
    cam = camera(W0, H0)
    rng = np.random.default_rng(71)
    per = 16
    n = 4 * per
    P = generic(n, cam, 72)
    P["means"] = place(cam, on_screen(n, cam, rng))
    P["log_scales"][0 * per:1 * per] = -12.0
    P["log_scales"][1 * per:2 * per] = 4.0
    P["log_scales"][2 * per:3 * per] = np.array([-12.0, 4.0, 0.0])
    tags = dict(tiny=np.arange(0, per), big=np.arange(per, 2 * per), mixed=np.arange(2 * per, 3 * per), generic=np.arange(3 * per, n))
    return settle(Case(f"scale@{glob_scale:g}", P, cam, 3, tags, glob_scale=glob_scale), how="depth")


def _sh(deg, Ks):
    """View directions on +-x, +-y, +-z (two distances each) and generic ones; deg = -1: no SH tensor."""
    cam = camera(W0, H0)
    Rw, tw = cam_parts(cam)
    campos = -(Rw.T @ tw)
    n = 64
    P = generic(n, cam, 80 + 4 * max(deg, 0) + (Ks == 16), deg=deg, Ks=max(Ks, 1))
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)
    P["means"][:12] = f32(np.concatenate([campos + 1.5 * axes, campos + 4.0 * axes]))
    tags = dict(axis=np.arange(12), generic=np.arange(12, n))
    return settle(Case("nosh" if deg < 0 else f"sh{deg}_k{Ks}", P, cam, deg, tags))


def _wide():
    """2048 Gaussians under a 3840 x 2160 camera with off-centre intrinsics, positions out to the last tile column and
    row: where an absolute pixel coordinate costs the most fp32 bits.  K1 only."""
    cam = camera(3840, 2160, skew=True)
    n = 2048
    P = generic(n, cam, 91)
    rng = np.random.default_rng(92)
    tc = on_screen(n, cam, rng, frac=1.0)
    # the intrinsics are off centre: spread u over the whole image, not over +- half of it about cx
    u = rng.uniform(0.0, cam.W, n)
    v = rng.uniform(0.0, cam.H, n)
    u[:32], v[32:64] = cam.W - rng.uniform(0.5, 15.0, 32), cam.H - rng.uniform(0.5, 7.0, 32)
    tc[:, 0], tc[:, 1] = (u - cam.cx) / cam.fx * tc[:, 2], (v - cam.cy) / cam.fy * tc[:, 2]
    P["means"] = place(cam, tc)
    return settle(Case("wide", P, cam, 3, dict(all=np.arange(n), last_col=np.arange(32), last_row=np.arange(32, 64)),
                       k1_only=True))


SH_VARIANTS = ((-1, 0), (0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 16), (3, 16))


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> Case.  Cached: the cases (and the references derived from them) are built once and never modified."""
    cs = [_fill(), _near(), _clamp(), _opacity(), _gate(), _quat(), _shape(), _scale(0.5), _scale(2.0)]
    cs += [_sh(d, k) for d, k in SH_VARIANTS]
    cs.append(_wide())
    out = {c.name: c for c in cs}
    # every stratum that shares the 160 x 96 orbit camera, degree 3, 16 bases and glob_scale 1, in one launch
    tog = [out[k] for k in ("fill", "clamp", "opacity", "gate", "quat", "shape", "sh3_k16")]
    out["together"] = concat("together", tog, constructed=False)
    return out


def constructed_mask(case):
    """Gaussians whose integer decisions must be exact (everything but the random fill)."""
    m = np.ones(case.N, bool)
    if case.name == "fill":
        m[:] = False
    elif case.name == "together":
        m[case.tags["fill"]] = False
    return m


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refc(prec):
    return RefC(prec)


def cam_block(R, cam):
    return R.cam_block(cam.viewmat.numpy(), cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.pix_center, cam.bg)


def ref_fwd(case, prec="f64"):
    R = _refc(prec)
    P, cam = case.P, case.cam
    return R.project_fwd(P["means"], P["log_scales"], P["quats"], P["opac_logit"], P["sh"], case.deg,
                         cam_block(R, cam), cam.W, cam.H, case.glob_scale)


def split_upstream(v):
    """[N,10] {v_x, v_y, v_depth, v_opac, v_a, v_b, v_c, v_r, v_g, v_b} -> the oracle's keyword arguments."""
    v = np.asarray(v, np.float64)
    return dict(v_xy=v[:, 0:2], v_depth=v[:, 2], v_opac=v[:, 3], v_conic=v[:, 4:7], v_rgb=v[:, 7:10])


def ref_bwd(case, v, radius, prec="f64"):
    """B.8 of the C oracle.  `radius` decides which Gaussians get a geometry gradient (the kernel asks its own record)."""
    R = _refc(prec)
    P, cam = case.P, case.cam
    u = split_upstream(v)
    o = R.project_bwd(P["means"], P["log_scales"], P["quats"], P["opac_logit"], P["sh"], case.deg, cam_block(R, cam),
                      cam.W, cam.H, radius, u["v_xy"], u["v_conic"], u["v_opac"], u["v_rgb"], u["v_depth"], case.glob_scale)
    if P["sh"] is None:
        o["v_sh"] = np.zeros((case.N, 0, 3))
    return o


def upstream(case, seed=5):
    """Seeded upstream gradients [N,10] (fp32 numbers): normals with a lognormal scale per Gaussian."""
    rng = np.random.default_rng(seed + case.N)
    return f32(rng.normal(size=(case.N, 10)) * np.exp(rng.normal(size=(case.N, 1))))


def grad_mass(case, radius, vmag):
    """tests.util.param_mass for upstream magnitudes `vmag` [N,10]; glob_scale is folded into the log-scales (the unit
    is an fp64 quantity, and d/d log_scale is the same either way)."""
    R = _refc("f64")
    P = dict(case.P)
    P["log_scales"] = P["log_scales"] + math.log(case.glob_scale)
    m7 = split_upstream(np.abs(vmag))
    if P["sh"] is None:
        P["sh"] = np.zeros((case.N, 1, 3))
    mass = param_mass(R, P, max(case.deg, 0), cam_block(R, case.cam), case.cam.W, case.cam.H, radius, m7)
    if case.P["sh"] is None:
        mass["v_sh"] = np.zeros((case.N, 0))
    # v_quats is formed from DIFFERENCES of the entries of v_R = v_M diag(s), the same numbers whose sums give
    # v_log_scales.  For an isotropic Gaussian they cancel exactly (its covariance does not depend on the rotation): the
    # Jacobian column, and with it the mass, is zero, while the terms that were subtracted are of the size of
    # v_log_scales / |q|.  That size is the un-cancelled magnitude of the quaternion gradient.
    qn = np.linalg.norm(case.P["quats"], axis=1, keepdims=True)
    mass["v_quats"] = mass["v_quats"] + mass["v_log_scales"].max(1, keepdims=True) / qn
    return mass


def grad_err(case, got, ref, mass, kappa, slack=None):
    """Per Gaussian and gradient: max_c |got - ref| / (2^-24 kappa max_c mass).  0 / 0 = 0: a gradient whose mass is
    zero is asserted exactly elsewhere.  slack: an absolute allowance per gradient component, taken off the difference
    first (the share of an upstream that the kernel holds rounded: |J| |dv|, see grad_mass)."""
    out = {}
    for k in PARAM_KEYS:
        g, r, m = (np.asarray(a[k], np.float64).reshape(case.N, -1) for a in (got, ref, mass))
        if g.shape[1] == 0:
            out[k] = np.zeros(case.N)
            continue
        d = np.abs(g - r)
        if slack is not None:
            d = np.maximum(d - 1.001 * np.asarray(slack[k], np.float64).reshape(case.N, -1), 0.0)
        e = d.max(1)
        u = EPS32 * kappa * m.max(1)
        out[k] = np.where(e == 0, 0.0, e / np.maximum(u, 1e-300))
    return out


FWD_KEYS = ("conic", "rgb", "opac", "depth")


def fwd_err(case, got, ref, g, vis):
    """Forward errors in their units: conic in u_conic (visible Gaussians only), rgb and depth in the rounding of their
    un-cancelled sums, opacity relative (in 2^-24)."""
    e = dict(conic=np.where(vis, np.abs(np.asarray(got["conic"]) - ref["conic"]).max(1) / g["u_conic"], 0.0),
             opac=np.abs(np.asarray(got["opac"]) - ref["opac"]) / (EPS32 * ref["opac"]),
             depth=np.abs(np.asarray(got["depth"]) - ref["depth"]) / np.maximum(g["u_depth"], 1e-300))
    if case.P["sh"] is not None:
        e["rgb"] = (np.abs(np.asarray(got["rgb"]) - ref["rgb"]) / g["u_rgb"]).max(1)
    else:
        e["rgb"] = np.zeros(case.N)
    return e


@functools.lru_cache(maxsize=None)
def floors(name):
    """The fp32 floor of a case: error of RefC("f32") against RefC("f64") in the units above, maximum over the case.
    -> dict over FWD_KEYS + PARAM_KEYS.  (The two take the same integer decisions on constructed Gaussians; on the
    random fill only Gaussians with equal radius enter.)"""
    case = all_cases()[name]
    g = geometry(case)
    r64, r32 = ref_fwd(case, "f64"), ref_fwd(case, "f32")
    same = r64["radius"] == r32["radius"]
    vis = (r64["radius"] > 0) & same
    fe = fwd_err(case, r32, r64, g, vis)
    out = {k: float(fe[k][same].max()) for k in FWD_KEYS}
    if not case.k1_only:
        v = upstream(case)
        rad = np.where(same, r64["radius"], 0).astype(np.int32)
        b64, b32 = ref_bwd(case, v, rad, "f64"), ref_bwd(case, v, rad, "f32")
        ge = grad_err(case, b32, b64, grad_mass(case, rad, v), g["kappa"])
        # v_opac_logit has no floor from RefC("f32"): it evaluates o (1 - o), which is 0 in fp32 from logit 17 on.  The
        # kernel's claim is the cancellation-free form; the GPU test holds it to OPAC_LOGIT_BAR against the closed form
        out.update({k: float(ge[k].max()) for k in PARAM_KEYS if k != "v_opac_logit"})
    return out


# sigmoid'(x) = t / (1 + t)^2, t = exp(-|x|): expf (2 ulp) + the sum, the reciprocal (entering twice), two products and
# the product with the upstream, half an ulp each -> 2 + 0.5 + 2 * 0.5 + 1 + 0.5 = 5 ulp; 8 leaves room for an expf of 4
OPAC_LOGIT_BAR = 8.0


def bars(name):
    """4 x the fp32 floor of the case (another summation order, FMA contraction, the GPU's exp / divide), and never
    below 4 units: a single correctly rounded operation is already half a unit off."""
    return {k: 4.0 * max(v, 1.0) for k, v in floors(name).items()}
