"""NumPy statement of the camera-pose gradient (the spec of k_pose_grad) -- CPU only.

V = [R | p] are rows 0-2 of the world->camera matrix.  The loss reaches V through
  1. the camera-space mean t = R m + p:         G_p += vt,  G_R[i][j] += vt[i] m[j]         (visible Gaussians)
  2. the covariance factor Tm = J R (2x3):       G_R += J^T vTm                              (visible Gaussians)
  3. the SH view direction, campos = -R^T p:     G_p[i] += sum_j R[i][j] vmd[j],  G_R[i][j] += p[i] vmd[j]
     (every Gaussian; vmd = the gradient w.r.t. the mean through the direction alone; zero below degree 1)
Beside each of the 12 entries goes its MASS: the sum of the absolute values of the products written above.

Generic in dtype: np.float64 is the reference (tests/test_cpu_pose_ref.py holds it to torch autograd of the oracle), and
np.float32 is the floor emulation -- every operation rounds to fp32 and the sums run in the kernel's declared order, within
a 256-Gaussian group first, then the groups in index order.  Also here, in fp64: the tangent (g_phi, g_upsilon) of the
left-multiplied parametrisation, the retraction, and the host Adam of touch_gs_amd/pose.py restated.
"""
import functools

import numpy as np

from tests.project_cases import BLUR, EPS32, cam_parts

GROUP = 256
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)


def sh_basis_and_grad(deg, d):
    """Y [n,K] and dY/dd [n,K,3] of the real SH basis at unit directions d [n,3] (dtype of d)."""
    T = d.dtype
    x, y, z = d.T
    n = len(x)
    K = (deg + 1) ** 2
    Y, dY = np.zeros((n, K), T), np.zeros((n, K, 3), T)
    c = lambda a: T.type(a)
    Y[:, 0] = c(0.28209479177387814)
    if deg >= 1:
        Y[:, 1], Y[:, 2], Y[:, 3] = -c(SH_C1) * y, c(SH_C1) * z, -c(SH_C1) * x
        dY[:, 1, 1], dY[:, 2, 2], dY[:, 3, 0] = -c(SH_C1), c(SH_C1), -c(SH_C1)
    if deg >= 2:
        xx, yy, zz = x * x, y * y, z * z
        C = [c(a) for a in SH_C2]
        Y[:, 4], Y[:, 5], Y[:, 6] = C[0] * x * y, C[1] * y * z, C[2] * (2 * zz - xx - yy)
        Y[:, 7], Y[:, 8] = C[3] * x * z, C[4] * (xx - yy)
        dY[:, 4, 0], dY[:, 4, 1] = C[0] * y, C[0] * x
        dY[:, 5, 1], dY[:, 5, 2] = C[1] * z, C[1] * y
        dY[:, 6, 0], dY[:, 6, 1], dY[:, 6, 2] = -2 * C[2] * x, -2 * C[2] * y, 4 * C[2] * z
        dY[:, 7, 0], dY[:, 7, 2] = C[3] * z, C[3] * x
        dY[:, 8, 0], dY[:, 8, 1] = 2 * C[4] * x, -2 * C[4] * y
    if deg >= 3:
        C = [c(a) for a in SH_C3]
        Y[:, 9], Y[:, 10] = C[0] * y * (3 * xx - yy), C[1] * x * y * z
        Y[:, 11], Y[:, 12] = C[2] * y * (4 * zz - xx - yy), C[3] * z * (2 * zz - 3 * xx - 3 * yy)
        Y[:, 13], Y[:, 14], Y[:, 15] = C[4] * x * (4 * zz - xx - yy), C[5] * z * (xx - yy), C[6] * x * (xx - 3 * yy)
        dY[:, 9, 0], dY[:, 9, 1] = 6 * C[0] * x * y, 3 * C[0] * (xx - yy)
        dY[:, 10, 0], dY[:, 10, 1], dY[:, 10, 2] = C[1] * y * z, C[1] * x * z, C[1] * x * y
        dY[:, 11, 0], dY[:, 11, 1], dY[:, 11, 2] = -2 * C[2] * x * y, C[2] * (4 * zz - xx - 3 * yy), 8 * C[2] * y * z
        dY[:, 12, 0], dY[:, 12, 1], dY[:, 12, 2] = -6 * C[3] * x * z, -6 * C[3] * y * z, C[3] * (6 * zz - 3 * xx - 3 * yy)
        dY[:, 13, 0], dY[:, 13, 1], dY[:, 13, 2] = C[4] * (4 * zz - 3 * xx - yy), -2 * C[4] * x * y, 8 * C[4] * x * z
        dY[:, 14, 0], dY[:, 14, 1], dY[:, 14, 2] = 2 * C[5] * x * z, -2 * C[5] * y * z, C[5] * (xx - yy)
        dY[:, 15, 0], dY[:, 15, 1] = 3 * C[6] * (xx - yy), -6 * C[6] * x * y
    return Y, dY


def _geom_terms(case, v, idx, T):
    """vt [n,3], vTm [n,2,3], J00, J02, J11, J12 of the Gaussians idx (all visible: tz > near, det > 0)."""
    P, cam = case.P, case.cam
    R, p = (a.astype(T) for a in cam_parts(cam))
    fx, fy = T(cam.fx), T(cam.fy)
    m, ls, q = (P[k][idx].astype(T) for k in ("means", "log_scales", "quats"))
    v = v[idx].astype(T)
    t = m @ R.T + p
    tx, ty, tz = t.T
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    w, x, y, z = q.T
    Rq = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                   2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    s = np.exp(ls) * T(case.glob_scale)
    M = Rq * s[:, None, :]
    Sig = M @ M.transpose(0, 2, 1)
    limx, limy = T(1.3) * T(0.5 * cam.W) / fx, T(1.3) * T(0.5 * cam.H) / fy
    rz = 1 / tz
    ux, uy = tx * rz, ty * rz
    inx, iny = np.abs(ux) <= limx, np.abs(uy) <= limy
    ucx, ucy = np.clip(ux, -limx, limx), np.clip(uy, -limy, limy)
    J00, J02, J11, J12 = fx * rz, -fx * ucx * rz, fy * rz, -fy * ucy * rz
    zero = np.zeros_like(rz)
    J = np.stack([J00, zero, J02, zero, J11, J12], 1).reshape(-1, 2, 3)
    Tm = J @ R
    cov = Tm @ Sig @ Tm.transpose(0, 2, 1)
    c00, c01, c11 = cov[:, 0, 0] + T(BLUR), cov[:, 0, 1], cov[:, 1, 1] + T(BLUR)
    det = c00 * c11 - c01 * c01
    a, b, c = c11 / det, -c01 / det, c00 / det
    va, vb, vc = v[:, 4], v[:, 5], v[:, 6]
    G00 = -(a * a * va + a * b * vb + b * b * vc)
    G11 = -(b * b * va + b * c * vb + c * c * vc)
    G01 = -T(0.5) * (2 * a * b * va + (a * c + b * b) * vb + 2 * b * c * vc)
    Gm = np.stack([G00, G01, G01, G11], 1).reshape(-1, 2, 2)
    vTm = 2 * (Gm @ Tm @ Sig)
    vJ = vTm @ R.T
    vJ00, vJ02, vJ11, vJ12 = vJ[:, 0, 0], vJ[:, 0, 2], vJ[:, 1, 1], vJ[:, 1, 2]
    rz2 = rz * rz
    vt = np.zeros_like(t)
    vt[:, 2] = -(vJ00 * fx + vJ11 * fy) * rz2
    vt[:, 0] += np.where(inx, -vJ02 * fx * rz2, 0)
    vt[:, 2] += np.where(inx, 2 * vJ02 * fx * tx * rz2 * rz, vJ02 * fx * ucx * rz2)
    vt[:, 1] += np.where(iny, -vJ12 * fy * rz2, 0)
    vt[:, 2] += np.where(iny, 2 * vJ12 * fy * ty * rz2 * rz, vJ12 * fy * ucy * rz2)
    vt[:, 0] += v[:, 0] * fx * rz
    vt[:, 1] += v[:, 1] * fy * rz
    vt[:, 2] += -v[:, 0] * fx * tx * rz2 - v[:, 1] * fy * ty * rz2 + v[:, 2]
    return vt, vTm, (J00, J02, J11, J12), m


def _dir_grad(case, v, T):
    """vmd [N,3]: the gradient w.r.t. the mean through the SH view direction alone (every Gaussian)."""
    P, cam = case.P, case.cam
    R, p = (a.astype(T) for a in cam_parts(cam))
    K = (case.deg + 1) ** 2
    m, ck, v = P["means"].astype(T), P["sh"][:, :K].astype(T), v.astype(T)
    d = m - (-(R.T @ p))
    inv = 1 / np.sqrt((d * d).sum(1, keepdims=True))
    d = d * inv
    Y, dY = sh_basis_and_grad(case.deg, d)
    col = (Y[:, :, None] * ck).sum(1) + T(0.5)
    vr = np.where(col > 0, v[:, 7:10], 0)
    s = (ck * vr[:, None, :]).sum(2)                      # [N,K]
    vd = (dY * s[:, :, None]).sum(1)
    return (vd - d * (d * vd).sum(1, keepdims=True)) * inv


def per_gaussian(case, v, visible, dtype=np.float64):
    """-> (C [N,12], M [N,12]): each Gaussian's contribution to G (entry 4 i + j: G_R[i][j] for j < 3, G_p[i] for j = 3)
    and to the masses.  `visible` [N] bool is the kernel's own set (conic written)."""
    T = np.dtype(dtype).type
    N = case.N
    C, M = np.zeros((N, 3, 4), T), np.zeros((N, 3, 4), T)
    R, p = (a.astype(T) for a in cam_parts(case.cam))

    def add(sl, term):
        C[sl] += term
        M[sl] += np.abs(term)

    if case.P["sh"] is not None and case.deg >= 1:
        vmd = _dir_grad(case, v, T)
        for j in range(3):
            add((slice(None), slice(None), 3), R[None, :, j] * vmd[:, j:j + 1])
        add((slice(None), slice(None), slice(0, 3)), p[None, :, None] * vmd[:, None, :])
    idx = np.nonzero(visible)[0]
    if len(idx):
        vt, vTm, (J00, J02, J11, J12), m = _geom_terms(case, v, idx, T)
        add((idx, slice(None), 3), vt)
        add((idx, slice(None), slice(0, 3)), vt[:, :, None] * m[:, None, :])
        add((idx, 0, slice(0, 3)), J00[:, None] * vTm[:, 0])
        add((idx, 1, slice(0, 3)), J11[:, None] * vTm[:, 1])
        add((idx, 2, slice(0, 3)), J02[:, None] * vTm[:, 0])
        add((idx, 2, slice(0, 3)), J12[:, None] * vTm[:, 1])
    return C.reshape(N, 12), M.reshape(N, 12)


def ordered_sum(X, dtype):
    """Rows of X [N,k] summed group by group (256 rows), then the groups in index order, every add in `dtype`."""
    T = np.dtype(dtype).type
    acc = np.zeros(X.shape[1], T)
    for g0 in range(0, len(X), GROUP):
        acc = (acc + X[g0:g0 + GROUP].astype(T).sum(0, dtype=T)).astype(T)
    return acc


def pose_grad(case, v, visible, dtype=np.float64):
    """-> dict(G [3,4], mass [3,4], g_phi [3], g_ups [3], n_visible) of one case and upstream v [N,10]."""
    C, M = per_gaussian(case, v, visible, dtype)
    G, mass = ordered_sum(C, dtype).reshape(3, 4), ordered_sum(M, dtype).reshape(3, 4)
    R, p = cam_parts(case.cam)
    g_phi, g_ups = tangent(G.astype(np.float64), R, p)
    return dict(G=G, mass=mass, g_phi=g_phi, g_ups=g_ups, n_visible=int(np.count_nonzero(visible)))


# ---------------------------------------------------------------------------------------------
# parametrisation, retraction, optimizer (fp64)
# ---------------------------------------------------------------------------------------------
def tangent(G, R, p):
    """Gradient w.r.t. (phi, upsilon) at 0 of  R <- exp([phi]x) R,  p <- exp([phi]x) p + upsilon  from G = [G_R | G_p]:
    g_ups = G_p,  g_phi = sum_j R[:,j] x G_R[:,j] + p x G_p."""
    G = np.asarray(G, np.float64).reshape(3, 4)
    g_phi = np.cross(p, G[:, 3])
    for j in range(3):
        g_phi = g_phi + np.cross(R[:, j], G[:, j])
    return g_phi, G[:, 3].copy()


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rodrigues(w):
    th = float(np.linalg.norm(w))
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K)


def retract(R, p, dphi, dups):
    E = rodrigues(np.asarray(dphi, np.float64))
    return E @ R, E @ p + np.asarray(dups, np.float64)


def rot_log(R):
    """Rotation vector of a rotation matrix (angle < pi)."""
    c = np.clip((np.trace(R) - 1) / 2, -1.0, 1.0)
    th = np.arccos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return 0.5 * w if th < 1e-8 else w * (th / (2 * np.sin(th)))


class Adam6:
    """Adam on the 6-vector (phi, upsilon) with separate learning rates, as touch_gs_amd.pose.PoseRefiner keeps it."""

    def __init__(self, lr_rot, lr_trans, betas=(0.9, 0.999), eps=1e-15):
        self.lr = np.array([lr_rot] * 3 + [lr_trans] * 3, np.float64)
        self.b1, self.b2, self.eps = betas[0], betas[1], eps
        self.m, self.v, self.t = np.zeros(6), np.zeros(6), 0

    def step(self, g):
        g = np.asarray(g, np.float64)
        self.t += 1
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        mh, vh = self.m / (1 - self.b1 ** self.t), self.v / (1 - self.b2 ** self.t)
        return -self.lr * mh / (np.sqrt(vh) + self.eps)


def pose_error(R, p, R0, p0):
    """(rotation angle in degrees, distance of the camera centres) between two poses."""
    ang = np.degrees(np.linalg.norm(rot_log(R @ R0.T)))
    return float(ang), float(np.linalg.norm(-R.T @ p + R0.T @ p0))


# ---------------------------------------------------------------------------------------------
# the pinned cases and their fp32 floors
# ---------------------------------------------------------------------------------------------
# strata of tests/project_cases.py: the random fill, both sides of the 1.3 clamp (inx / iny false occurs), the near plane,
# the 3840 x 2160 camera, and SH storage (-1, 0), (0, 16), (1, 4), (3, 16), (1, 16), (2, 9), (2, 16).  fill and wide are cut to 513 and 300
# Gaussians: more than one group with a partial last one, in seconds.
PIN_NAMES = ("fill", "clamp", "near", "wide", "nosh", "sh0_k16", "sh1_k4", "sh3_k16",
             "sh1_k16", "sh2_k9", "sh2_k16")     # ... and degrees 1 and 2 on rows of 16 and of 9 bases
PIN_TAKE = {"fill": 513, "wide": 300}


@functools.lru_cache(maxsize=None)
def pin_case(name):
    from tests import project_cases as PC
    case = PC.all_cases()[name]
    if name in PIN_TAKE:
        case = case.take(np.arange(PIN_TAKE[name]), name=name)
    return case


def cpu_visible(case):
    """The kernel's visible set as the fp64 C oracle decides it (the GPU test asks the built records instead)."""
    from tests import project_cases as PC
    return PC.ref_fwd(case)["radius"] > 0


def err_units(got, ref, mass):
    """max over the 12 entries of |got - ref| / (2^-24 mass); an entry without mass must be exact."""
    got, ref, mass = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, mass))
    d = np.abs(got - ref)
    assert (d[mass == 0] == 0).all(), "an entry whose mass is zero must be exactly zero"
    return float(np.where(mass > 0, d / np.maximum(EPS32 * mass, 1e-300), 0.0).max())


@functools.lru_cache(maxsize=None)
def floor(name):
    """fp32 floor of G of a pinned case: the fp32 emulation against fp64, in units of 2^-24 mass, maximum over entries."""
    from tests import project_cases as PC
    case = pin_case(name)
    v, vis = PC.upstream(case), cpu_visible(case)
    r64, r32 = pose_grad(case, v, vis, np.float64), pose_grad(case, v, vis, np.float32)
    return err_units(r32["G"], r64["G"], r64["mass"])


def bar(name):
    """4 x the floor, never below 4 units (the rule of project_cases.bars)."""
    return 4.0 * max(floor(name), 1.0)


# ---------------------------------------------------------------------------------------------
# whole-loss gradient from the oracle, and the pose-recovery loop it drives
# ---------------------------------------------------------------------------------------------
LOSS_KW = dict(ssim_lambda=0.2, depth_loss_mult=0.2, uncertainty_weight=1.0)


def tiny_scene(N, W, H, deg, seed, view=1, nviews=8):
    """Synthetic scene with fp32-exact parameters and camera -> (P fp64 tensors, intrinsics dict, V [4,4] fp64)."""
    import torch
    from oracle import torch_oracle as O
    P, c = O.synthetic_scene(N, W, H, deg, seed)
    P = {k: v.float().double() for k, v in P.items()}
    c = {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in c.items()}
    V = O.orbit_viewmat(view, nviews).float().double().numpy()
    return P, c, V


def oracle_render(P, c, V, deg, dtype=None, bg=(0.1, 0.2, 0.3)):
    """Oracle render at pose V -> (out dict, viewmat tensor with requires_grad)."""
    import torch
    from oracle import torch_oracle as O
    dtype = dtype or torch.float64
    Vt = torch.from_numpy(np.asarray(V, np.float64)).to(dtype).requires_grad_(True)
    cam = O.Camera(viewmat=Vt, **c, bg=bg)
    Pd = {k: v.to(dtype) for k, v in P.items()}
    out, _, _, _ = O.render(Pd["means"], Pd["log_scales"], Pd["quats"], Pd["opac_logit"], Pd["sh"], cam, deg)
    return out, Vt


def oracle_pose_grad(P, c, V, deg, gt, dgt, unc, dtype=None):
    """(loss, dL/dV rows 0-2 [3,4]) of the train loss (L1 + SSIM + uncertainty-weighted depth) by autograd."""
    import torch
    from oracle import torch_oracle as O
    dtype = dtype or torch.float64
    out, Vt = oracle_render(P, c, V, deg, dtype)
    L = O.train_loss(out, gt.to(dtype), dgt.to(dtype), unc.to(dtype), **LOSS_KW)
    L.backward()
    return float(L.detach()), Vt.grad.double().numpy()[:3].copy()


def supervision_from(P, c, V, deg):
    """Ground truth of the recovery test: the model's own render at the true pose (fp32 numbers): rgb, depth where the
    pixel is mostly covered (0 = unsupervised elsewhere), unit uncertainty."""
    import torch
    with torch.no_grad():
        out, _ = oracle_render(P, c, V, deg)
    rgb = out["rgb"].detach().float().double().clamp(0, 1)
    a = out["alpha"].detach()
    d = torch.where(a > 0.5, out["depth_acc"].detach() / a.clamp(min=1e-10), torch.zeros_like(a)).float().double()
    return rgb, d, torch.ones_like(d)


# the recovery test: one view turned by RECOVER_ROT degrees about RECOVER_AXIS and moved by RECOVER_TRANS, then
# RECOVER_STEPS pose-only Adam steps at these rates (chosen so that the fp64-oracle-driven loop ends below one fifth of
# both initial errors; tests/test_cpu_pose_ref.py::test_recovery_reference checks and prints it)
RECOVER = dict(N=150, W=48, H=32, deg=3, seed=3, rot_deg=0.6, axis=(0.3, 1.0, 0.2), trans=(0.02, -0.015, 0.01),
               lr_rot=4e-4, lr_trans=8e-4, steps=60)


# largest distance between the GPU trajectory and the reference trajectory over the 60 steps, as a fraction of the initial
# error (rotation and camera centre alike): 4 x the gap observed on an MI355X, 1.75e-4
RECOVER_GAP_BAR = 4 * 1.75e-4


def perturbed(V, rot_deg, axis, trans):
    a = np.asarray(axis, np.float64)
    R, p = retract(V[:3, :3], V[:3, 3], np.radians(rot_deg) * a / np.linalg.norm(a), np.asarray(trans, np.float64))
    V2 = np.eye(4)
    V2[:3, :3], V2[:3, 3] = R, p
    return V2.astype(np.float32).astype(np.float64)


def recovery_loop(grad_fn, V_start, lr_rot, lr_trans, steps):
    """Pose-only Adam steps from V_start; grad_fn(V) -> G [3,4].  -> list of poses V_0 .. V_steps."""
    V, adam, traj = V_start.copy(), Adam6(lr_rot, lr_trans), [V_start.copy()]
    for _ in range(steps):
        g_phi, g_ups = tangent(grad_fn(V), V[:3, :3], V[:3, 3])
        d = adam.step(np.concatenate([g_phi, g_ups]))
        R, p = retract(V[:3, :3], V[:3, 3], d[:3], d[3:])
        V = np.eye(4)
        V[:3, :3], V[:3, 3] = R, p
        traj.append(V.copy())
    return traj
