"""The constructed projection cases (tests/project_cases.py) hold what their names say, the two fp64 references agree on
them, fp32 and fp64 take the same integer decisions on every constructed Gaussian, and the fp32 floor of every stratum
-- the figure the GPU bars of tests/test_gpu_project_oracle.py are 4 x of -- is reported (run with -s to see it)."""
import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests import project_cases as PC
from tests.util import PARAM_KEYS

CASES = PC.all_cases()
NAMES = [n for n in CASES if n != "together"]


def test_every_entry_is_an_fp32_number():
    for c in CASES.values():
        for k, v in c.P.items():
            if v is not None:
                assert np.array_equal(v, PC.f32(v)) and v.dtype == np.float64, (c.name, k)
        cam = c.cam
        for x in list(cam.viewmat.numpy().ravel()) + [cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.pix_center, c.glob_scale]:
            assert float(np.float32(x)) == float(x), (c.name, x)


def _torch_oracle(case, v):
    """O.project + autograd with the upstream `v`: geometry terms flow for visible Gaussians, colour / opacity for all."""
    P = {k: (None if t is None else t.requires_grad_(True)) for k, t in case.torch_params().items()}
    pr = O.project(P["means"], P["log_scales"], P["quats"], P["opac_logit"], P["sh"], case.cam, max(case.deg, 0),
                   glob_scale=case.glob_scale)
    vt = torch.from_numpy(v)
    vz = torch.where(pr["valid"][:, None], vt, torch.zeros_like(vt))
    L = (pr["xy"] * vz[:, 0:2]).sum() + (pr["depth"] * vz[:, 2]).sum() + (pr["opac"] * vt[:, 3]).sum() \
        + (pr["conic"] * vz[:, 4:7]).sum()
    if P["sh"] is not None:
        L = L + (pr["rgb"] * vt[:, 7:10]).sum()
    L.backward()
    return pr, P


@pytest.mark.parametrize("name", NAMES)
def test_references_agree(name):
    """O.project + autograd and the C oracle RefC("f64") -- two independent restatements -- agree to 1e-12 on every
    stratum, forward and all five gradients: values relative to their own size plus the unit's un-cancelled magnitude
    (kappa for what goes through the determinant).  v_opac_logit: both use o (1 - o), whose fp64 cancellation is
    2^-53 / (1 - o); each is held against the cancellation-free closed form within that."""
    case = CASES[name]
    g = PC.geometry(case)
    v = PC.upstream(case)
    r = PC.ref_fwd(case)
    pr, P = _torch_oracle(case, v)
    valid = pr["valid"].numpy()
    assert np.array_equal(valid, r["radius"] > 0)
    assert np.array_equal(pr["radius"].numpy(), r["radius"])
    assert np.array_equal(pr["rect"].numpy()[valid], r["rect"][valid])
    assert np.array_equal(pr["tiles_hit"].numpy(), r["tiles_hit"])
    tol = 1e-12
    front = g["front"]
    k = g["kappa"]
    assert (np.abs(pr["xy"].detach().numpy() - r["xy"])[front] <= tol * (1 + np.abs(r["xy"][front]))).all()
    assert (np.abs(pr["depth"].detach().numpy() - r["depth"]) <= tol * g["u_depth"] / PC.EPS32).all()
    assert (np.abs(pr["opac"].detach().numpy() - r["opac"]) <= tol * r["opac"]).all()
    dc = np.abs(pr["conic"].detach().numpy() - r["conic"])[valid].max(1)
    assert (dc <= tol * (k * np.abs(r["conic"]).max(1))[valid]).all()
    # ... and so does the builder's own numpy geometry, which defines the strata and the units
    assert (np.abs(g["conic"] - r["conic"])[valid].max(1) <= tol * (k * np.abs(r["conic"]).max(1))[valid]).all()
    if case.P["sh"] is not None:
        assert (np.abs(pr["rgb"].detach().numpy() - r["rgb"]) <= tol * g["u_rgb"] / PC.EPS32).all()
    if case.k1_only:
        return
    b = PC.ref_bwd(case, v, r["radius"])
    mass = PC.grad_mass(case, r["radius"], v)
    tg = dict(v_means=P["means"].grad, v_log_scales=P["log_scales"].grad, v_quats=P["quats"].grad,
              v_opac_logit=P["opac_logit"].grad, v_sh=None if P["sh"] is None else P["sh"].grad)
    for key in PARAM_KEYS:
        if tg[key] is None:
            continue
        a, c, m = (np.asarray(x, np.float64).reshape(case.N, -1) for x in (tg[key].numpy(), b[key], mass[key]))
        if key == "v_opac_logit":
            exact = v[:, 3:4] * PC.sigmoid_deriv(case.P["opac_logit"])[:, None]
            canc = 2.0 ** -50 / (1 - g["opac"])[:, None] + tol       # o (1 - o): 1 - o keeps 53 + log2(1 - o) bits
            for x in (a, c):
                assert (np.abs(x - exact) <= canc * np.abs(exact)).all(), (name, key)
            continue
        bad = np.abs(a - c).max(1) > tol * (k * m.max(1)) + 1e-300
        assert not bad.any(), (name, key, np.nonzero(bad)[0][:8])


def test_integer_decisions_fp32_vs_fp64():
    """RefC("f32") and RefC("f64") agree on radius, rect and visibility for EVERY constructed Gaussian (the builder is
    nudged until they do); on the random fill at most 0.5 % may differ, the project's existing figure."""
    for name in NAMES:
        case = CASES[name]
        a, b = PC.ref_fwd(case, "f64"), PC.ref_fwd(case, "f32")
        diff = (a["radius"] != b["radius"]) | (a["tiles_hit"] != b["tiles_hit"]) | \
            ((a["rect"] != b["rect"]).any(1) & (a["radius"] > 0))
        if case.constructed:
            assert not diff.any(), (name, np.nonzero(diff)[0])
        else:
            assert diff.mean() <= 0.005, (name, diff.mean())


def test_strata_hold_what_their_names_say():
    G = {n: PC.geometry(CASES[n]) for n in NAMES}
    R = {n: PC.ref_fwd(CASES[n]) for n in NAMES}

    # near: every k on both sides of the plane; behind and tz <= 0 are culled, in front is visible
    c, g, r = CASES["near"], G["near"], R["near"]
    tz = g["t"][:, 2]
    for k in range(4, 21):
        assert (tz[c.tags["front"]] == np.float32(PC.NEAR * (1 + 2.0 ** -k))).sum() == 2
        assert (tz[c.tags["behind"]] == np.float32(PC.NEAR * (1 - 2.0 ** -k))).sum() == 2
    assert (tz[c.tags["front"]] > c.cam.near).all() and (r["radius"][c.tags["front"]] > 0).all()
    for t in ("behind", "on", "zero", "neg"):
        assert (tz[c.tags[t]] <= c.cam.near).all() and (r["radius"][c.tags[t]] == 0).all()
    assert (tz[c.tags["neg"]] < 0).all() and tz[c.tags["zero"]][0] == 0 and tz[c.tags["on"]][0] == c.cam.near

    # clamp: inx / iny false on each side and both; every clamp decision >= 1e-4 relative off the limit; all visible
    c, g, r = CASES["clamp"], G["clamp"], R["clamp"]
    assert (r["radius"] > 0).all(), "a clamped Gaussian does not reach the image"
    ox_p, ox_m = g["ux"] > g["limx"], g["ux"] < -g["limx"]
    oy_p, oy_m = g["uy"] > g["limy"], g["uy"] < -g["limy"]
    for m in (ox_p, ox_m, oy_p, oy_m, ox_p & oy_p, ox_p & oy_m, ox_m & oy_p, ox_m & oy_m):
        assert m.sum() >= 3
    assert (~(ox_p | ox_m) & ~(oy_p | oy_m)).sum() >= 8
    assert (np.abs(np.abs(g["ux"]) / g["limx"] - 1) > 1e-4).all() and (np.abs(np.abs(g["uy"]) / g["limy"] - 1) > 1e-4).all()
    for f in PC.CLAMP_FACTORS:
        for t in (f"x+{f}", f"x-{f}", f"y+{f}", f"y-{f}"):
            i = c.tags[t]
            u, lim = (g["ux"], g["limx"]) if t[0] == "x" else (g["uy"], g["limy"])
            assert np.allclose(np.abs(u[i]) / lim, f, rtol=2e-5), t
            assert ((np.abs(u[i]) > lim) == (f > 1)).all(), t

    # opacity: the 255 o = 1 threshold lies between -5.6 and -5.5
    c, g, r = CASES["opacity"], G["opacity"], R["opacity"]
    for l in PC.OPACITY_LOGITS:
        i = c.tags[f"{l:g}"]
        assert (c.P["opac_logit"][i] == np.float32(l)).all() and (r["radius"][i] > 0).all()
        assert ((255 * g["opac"][i] > 1) == (l >= -5.5)).all()

    # gate: every channel at every level, independently
    c, g = CASES["gate"], G["gate"]
    assert c.deg == 3 and (np.abs(c.P["sh"][:, 1:16]).max(2) > 0).all()
    for ch in range(3):
        for l in PC.GATE_LEVELS:
            i = c.tags[f"ch{ch}_{l:g}"]
            assert len(i) == 16 and np.allclose(g["pre"][i, ch], l, rtol=0, atol=1e-6)
    assert len({tuple(x) for x in (g["pre"] > 0)}) == 8

    # quat: |q| far from 1, w = 0 included
    c = CASES["quat"]
    qn = np.linalg.norm(c.P["quats"], axis=1)
    for q in PC.QUAT_NORMS:
        assert np.allclose(qn[c.tags[f"{q:g}"]], q, rtol=1e-6)
    assert (c.P["quats"][c.tags["w0"], 0] == 0).all() and (R["quat"]["radius"] > 0).all()

    # shape
    c, g, r = CASES["shape"], G["shape"], R["shape"]
    assert (r["radius"] > 0).all()
    lam = lambda i: np.linalg.eigvalsh(np.stack([np.stack([g["c00"][i] - PC.BLUR, g["c01"][i]], -1),
                                                 np.stack([g["c01"][i], g["c11"][i] - PC.BLUR], -1)], -2))
    for ang in (0.0, 45.0, 89.0):
        i = c.tags[f"needle{ang:g}"]
        e = lam(i)
        assert (np.sqrt(e[:, 1] / e[:, 0]) > 60).all(), ang          # ~100:1 on screen
        axis = 0.5 * np.degrees(np.arctan2(2 * g["c01"][i], g["c00"][i] - g["c11"][i]))
        assert (np.abs(np.abs(axis) - ang) < 12).all(), (ang, axis)  # perspective turns it by a few degrees
    i = c.tags["iso"]
    assert (c.P["log_scales"][i].std(1) == 0).all() and (g["disc"][i] < 0.1).all() and (g["c00"][i] < 0.3002).all()
    assert (np.sqrt(g["c00"][c.tags["huge"]]) > 500).all()
    i = c.tags["ray"]
    assert (g["kappa"][i] >= 1).all() and (np.abs(c.cam.fx * g["ux"][i]) > 0.85 * c.cam.W / 2).all()
    S = g["Sig"][i]
    d = g["t"][i] / np.linalg.norm(g["t"][i], axis=1, keepdims=True)
    Rw, _ = PC.cam_parts(c.cam)
    dw = d @ Rw                                                       # the ray in world axes
    along = np.einsum("ni,nij,nj->n", dw, S, dw)
    assert np.allclose(np.sqrt(along / np.linalg.eigvalsh(S)[:, 0]), 100, rtol=1e-3)

    # scale: the extreme log-scales under both glob_scales
    for gs in (0.5, 2.0):
        c = CASES[f"scale@{gs:g}"]
        assert c.glob_scale == gs and (c.P["log_scales"][c.tags["tiny"]] == -12).all() and (c.P["log_scales"][c.tags["big"]] == 4).all()
        assert (R[c.name]["radius"] > 0).all()

    # sh: the axis directions, all degrees, both storage widths, and no SH at all
    seen = set()
    for deg, Ks in PC.SH_VARIANTS:
        c = CASES["nosh" if deg < 0 else f"sh{deg}_k{Ks}"]
        seen.add((c.deg, c.Ks))
        if deg >= 0:
            d = G[c.name]["dir"][c.tags["axis"]]
            assert np.allclose(np.abs(d).max(1), 1, atol=1e-6) and len({tuple(np.round(x)) for x in d}) == 6
    assert seen == {(-1, 0), (0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 16), (3, 16)}

    # wide: the last tile column and row are reached
    c, r = CASES["wide"], R["wide"]
    TW, TH = c.cam.tiles
    assert (c.cam.W, c.cam.H) == (3840, 2160) and c.cam.cx != c.cam.W / 2
    assert (r["rect"][c.tags["last_col"], 2] == TW).all() and (r["rect"][c.tags["last_row"], 3] == TH).all()
    assert (r["radius"] > 0).mean() > 0.95


def test_hits_zero_with_radius():
    """opacity below 1/255: the oracle still gives a radius (B.4 knows no opacity), the kernel's rect will be empty."""
    c, r, g = CASES["opacity"], PC.ref_fwd(CASES["opacity"]), PC.geometry(CASES["opacity"])
    low = 255 * g["opac"] <= 1
    assert low.sum() == 21 and (r["radius"][low] > 0).all()


def test_fp32_floor_report():
    """The fp32 floor per stratum, in the units of tests/project_cases.py (maximum over the stratum)."""
    keys = PC.FWD_KEYS + PARAM_KEYS
    print("\n%-12s" % "stratum" + "".join("%13s" % k for k in keys))
    for name in NAMES:
        f = PC.floors(name)
        print("%-12s" % name + "".join(("%13.2f" % f[k]) if k in f else "%13s" % "-" for k in keys))
        for k, x in f.items():
            assert np.isfinite(x), (name, k)
            # fp32 arithmetic of a few dozen operations: a floor of thousands of units would mean a unit that
            # does not describe the quantity
            assert x < 200, (name, k, x)
