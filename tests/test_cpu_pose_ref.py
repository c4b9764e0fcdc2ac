"""The camera-pose gradient's reference (tests/pose_ref.py) against torch autograd of the oracle, the tangent formula and
the retraction, the ABI of tgs_pose_grad, and the fp32 floors that set the bars of tests/test_gpu_pose_grad.py.  CPU only.

Floors (fp32 emulation against fp64, units of 2^-24 mass, max over the 12 entries; printed by test_floors):
see DESIGN.md section 5.1m for the table and the MI355X figures beside it.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests import pose_ref as PR
from tests import project_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd_G(case, v, visible):
    """d/d viewmat of <cotangents, oracle.project>: v on xy, depth, conic of the visible Gaussians, on rgb of all."""
    P = case.torch_params()
    V = case.cam.viewmat.clone().double().requires_grad_(True)
    c = case.cam
    cam = O.Camera(viewmat=V, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy, W=c.W, H=c.H, near=c.near, pix_center=c.pix_center, bg=c.bg)
    out = O.project(P["means"], P["log_scales"], P["quats"], P["opac_logit"], P["sh"], cam, case.deg, case.glob_scale)
    u = {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in PC.split_upstream(v).items()}
    vis = torch.from_numpy(visible.astype(np.float64))
    L = (out["xy"] * u["v_xy"] * vis[:, None]).sum() + (out["depth"] * u["v_depth"] * vis).sum() \
        + (out["conic"] * u["v_conic"] * vis[:, None]).sum()
    if P["sh"] is not None:
        L = L + (out["rgb"] * u["v_rgb"]).sum()
    L.backward()
    return V.grad.numpy()


@pytest.mark.parametrize("name", PR.PIN_NAMES)
def test_reference_equals_autograd(name):
    case = PR.pin_case(name)
    v, vis = PC.upstream(case), PR.cpu_visible(case)
    assert vis.any()
    if name in ("fill", "near"):      # culled Gaussians occur: paths 1 and 2 skip them, path 3 does not
        assert not vis.all()
    ref = PR.pose_grad(case, v, vis)
    G = _autograd_G(case, v, vis)
    assert (G[3] == 0).all()
    e = np.abs(ref["G"] - G[:3]) / ref["mass"]
    print(f"FIG {name:10s} reference vs autograd: max |dG| / mass = {e.max():.2e}")
    assert (e <= 1e-10).all(), (name, e)
    if name == "clamp":      # both sides of the 1.3 limit occur among the visible Gaussians
        g = PC.geometry(case)
        out_x, out_y = np.abs(g["ux"]) > g["limx"], np.abs(g["uy"]) > g["limy"]
        assert (out_x & vis).any() and (out_y & vis).any() and (~out_x & ~out_y & vis).any()
    if case.deg < 1:         # no view dependence: the colour path adds nothing, the cotangent on rgb is inert
        v2 = v.copy()
        v2[:, 7:10] = 0
        assert np.array_equal(PR.pose_grad(case, v2, vis)["G"], ref["G"])


def test_whole_loss_gradient_against_finite_differences():
    """d train_loss / d viewmat by autograd through torch_oracle.render + train_loss, taken to the tangent (phi, ups), against
    a central difference along the retraction: 48 x 32, 200 Gaussians, SH 3, L1 + SSIM + depth.

    The rendered loss is only piecewise smooth (tile rects, radii and the 1/255 alpha cut-off are decisions), and a probe
    that crosses a decision measures the jump, not the derivative -- at h = 1e-6 one of the six directions already does.
    So the step is h = 1e-7, where all twelve probes stay in the piece of the centre.  Truncation, h^2 / 6 times the third
    derivative, is then far below the rounding of the difference quotient: each loss value (a mean over 1536 pixels of
    sums over a few dozen Gaussians, |L| ~ 1) carries at most ~64 roundings of 2^-53 |L|, so
    |fd - exact| <= 64 * 2^-53 * |L| / h."""
    N, W, H, deg, h = 200, 48, 32, 3, 1e-7
    P, c, V = PR.tiny_scene(N, W, H, deg, 11)
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(H, W, 3, generator=g, dtype=torch.float64)
    dgt = torch.rand(H, W, generator=g, dtype=torch.float64) * 5
    unc = torch.rand(H, W, generator=g, dtype=torch.float64) + 0.1
    L0, G = PR.oracle_pose_grad(P, c, V, deg, gt, dgt, unc)
    an = np.concatenate(PR.tangent(G, V[:3, :3], V[:3, 3]))

    def loss(x):
        X = np.eye(4)
        X[:3, :3], X[:3, 3] = PR.retract(V[:3, :3], V[:3, 3], x[:3], x[3:])
        return PR.oracle_pose_grad(P, c, X, deg, gt, dgt, unc)[0]

    fd = np.array([(loss(h * e) - loss(-h * e)) / (2 * h) for e in np.eye(6)])
    bound = 64 * 2.0 ** -53 * abs(L0) / h
    print(f"FIG whole loss: |fd - autograd| max {np.abs(fd - an).max():.2e}, bound {bound:.2e}, |g| max {np.abs(an).max():.2e}")
    assert np.abs(an).max() > 1e3 * bound
    assert (np.abs(fd - an) <= bound).all(), (fd, an)


def test_recovery_reference():
    """The loop the GPU recovery test is compared with (fp64 oracle gradients, PR.RECOVER) ends with at most one fifth of
    the initial rotation and translation error."""
    k = PR.RECOVER
    P, c, V = PR.tiny_scene(k["N"], k["W"], k["H"], k["deg"], k["seed"])
    gt, dgt, unc = PR.supervision_from(P, c, V, k["deg"])
    V1 = PR.perturbed(V, k["rot_deg"], k["axis"], k["trans"])
    traj = PR.recovery_loop(lambda X: PR.oracle_pose_grad(P, c, X.astype(np.float32).astype(np.float64), k["deg"], gt, dgt, unc)[1],
                            V1, k["lr_rot"], k["lr_trans"], k["steps"])
    err = lambda X: PR.pose_error(X[:3, :3], X[:3, 3], V[:3, :3], V[:3, 3])
    (r0, t0), (r1, t1) = err(traj[0]), err(traj[-1])
    print(f"FIG recovery reference: {r0:.4f} deg, {t0:.5f} -> {r1:.4f} deg, {t1:.5f} after {k['steps']} steps")
    assert r1 <= r0 / 5 and t1 <= t0 / 5


def test_tangent_equals_autograd_through_the_exponential():
    """g_phi, g_ups from G equal autograd of  L(exp([phi]x) R, exp([phi]x) p + ups) = <G, V>  at phi = ups = 0."""
    rng = np.random.default_rng(3)
    for _ in range(5):
        R, p, G = PR.rodrigues(rng.normal(size=3)), rng.normal(size=3) * 3, rng.normal(size=(3, 4))
        phi = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        ups = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        z = torch.zeros((), dtype=torch.float64)
        K = torch.stack([torch.stack([z, -phi[2], phi[1]]), torch.stack([phi[2], z, -phi[0]]), torch.stack([-phi[1], phi[0], z])])
        E = torch.linalg.matrix_exp(K)
        Rn, pn = E @ torch.from_numpy(R), E @ torch.from_numpy(p) + ups
        L = (Rn * torch.from_numpy(G[:, :3])).sum() + (pn * torch.from_numpy(G[:, 3])).sum()
        L.backward()
        g_phi, g_ups = PR.tangent(G, R, p)
        assert np.allclose(g_phi, phi.grad.numpy(), rtol=0, atol=1e-13 * np.abs(G).max() * 10)
        assert np.allclose(g_ups, ups.grad.numpy(), rtol=0, atol=0)


def test_retraction_stays_orthonormal():
    """R^T R = I to 1e-14 over 10^4 updates (re-orthonormalised every 100, as PoseRefiner does), and the package's
    retraction is the reference's."""
    from touch_gs_amd import pose
    rng = np.random.default_rng(4)
    R, p = PR.rodrigues(rng.normal(size=3)), rng.normal(size=3)
    R2, p2 = R.copy(), p.copy()
    worst = 0.0
    for k in range(10000):
        dphi, dups = rng.normal(size=3) * 1e-3, rng.normal(size=3) * 1e-3
        R, p = pose.retract(R, p, dphi, dups)
        if k < 50:
            R2, p2 = PR.retract(R2, p2, dphi, dups)
            assert np.allclose(R, R2, atol=1e-15) and np.allclose(p, p2, atol=1e-15)
        if (k + 1) % 100 == 0:
            R = pose.orthonormalise(R)
        worst = max(worst, float(np.abs(R.T @ R - np.eye(3)).max()))
    print(f"FIG retraction: max |R^T R - I| over 10^4 updates = {worst:.2e}")
    assert worst <= 1e-14
    assert abs(np.linalg.det(R) - 1) < 1e-13


def test_host_adam_is_the_reference():
    from touch_gs_amd import pose
    rng = np.random.default_rng(5)
    a, b = PR.Adam6(1e-3, 2e-3), pose.Adam6(1e-3, 2e-3)
    for _ in range(20):
        g = rng.normal(size=6)
        assert np.array_equal(a.step(g), b.step(g))


def test_abi():
    from touch_gs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert re.search(r"\bint\s+tgs_pose_grad\s*\(", hdr)
    assert "tgs_pose_grad" in _lib.SIGNATURES and len(_lib.SIGNATURES["tgs_pose_grad"][1]) == 16
    lib = _lib.load()
    assert hasattr(lib, "tgs_pose_grad")
    assert lib.tgs_version() == 320
    assert re.search(r"#define\s+TGS_POSE_ROW\s+%d\b" % _lib.POSE_ROW, hdr) and re.search(r"#define\s+TGS_POSE_OUT\s+%d\b" % _lib.POSE_OUT, hdr)


@pytest.mark.parametrize("name", PR.PIN_NAMES)
def test_floors(name):
    """Printed, and finite: they set the bars of the GPU test (4 x, never below 4 units)."""
    f = PR.floor(name)
    print(f"FIG {name:10s} fp32 floor of G = {f:8.2f} units of 2^-24 mass  -> bar {PR.bar(name):8.2f}")
    assert np.isfinite(f) and f > 0
