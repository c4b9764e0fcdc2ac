"""K1 (k_project_fwd), K8 (k_project_bwd and the LDS-staged k_project_bwd_lds) and K8a (group_sum_partials) against the
fp64 C oracle on the constructed cases of tests/project_cases.py: every Gaussian of every stratum is asserted, none is
excused by a quantile.  Inputs are fp32 numbers on both sides, so what is measured is the kernels' arithmetic.

Units (tests/project_cases.py): conic in 2^-24 kappa max|conic|; rgb and depth in the rounding of their un-cancelled
sums; opacity relative; gradients in 2^-24 kappa mass.  The bar of a stratum is 4 x its fp32 floor -- the error of the
scalar C restatement compiled for float, RefC("f32"), against RefC("f64"), in the same units -- and never below 4
units.  The factor 4 covers another summation order, FMA contraction and the GPU's exp / divide, as in the SSIM pin.

fp32 floor | measured on the MI355X (max over the stratum, same units; gradients: the larger of the v_splats form, the
partials forms and the colour form; v_opac_logit in 2^-24 of v sigmoid'(x), bar 8; xy as a fraction of its bar):

stratum            conic           rgb          opac         depth       v_means  v_log_scales       v_quats          v_sh  v_opac_logit     xy
fill         12.8 | 10.8     2.9 | 2.9     1.9 | 1.9     1.8 | 1.5     5.3 | 5.5   16.6 | 11.6    9.9 | 13.8     5.3 | 6.1          4.53   0.25
near          6.1 | 10.5     2.5 | 2.5     1.8 | 1.8     0.0 | 0.0     8.6 | 6.9     9.1 | 8.3    10.0 | 8.9     4.7 | 5.8          3.88   0.25
clamp          7.0 | 9.8     2.4 | 2.4     1.5 | 1.5     1.5 | 1.5     2.1 | 2.9     8.2 | 9.2     5.2 | 8.5     4.1 | 3.9          3.40   0.25
opacity        6.6 | 7.7     2.1 | 2.1     1.1 | 1.1     1.4 | 1.3     1.6 | 2.0     8.5 | 8.5     6.6 | 8.0     4.0 | 4.2          3.01   0.25
gate           9.0 | 8.4     1.9 | 1.9     1.8 | 1.4     1.6 | 1.3     2.1 | 2.8     6.7 | 7.3     6.3 | 5.7     5.2 | 5.2          3.83   0.25
quat           6.9 | 8.4     2.6 | 2.6     1.6 | 1.6     1.3 | 1.3     2.0 | 1.8     7.4 | 9.1     7.6 | 8.5     4.1 | 3.4          4.23   0.25
shape         8.8 | 17.5     2.2 | 2.1     1.4 | 1.4     1.5 | 1.3     1.9 | 3.4   12.1 | 15.3   79.8 | 66.2     4.4 | 4.8          3.39   0.25
scale@0.5    12.5 | 11.7     1.9 | 1.9     1.2 | 1.1     1.4 | 1.3     2.9 | 2.5   19.6 | 17.6   16.5 | 16.8     5.4 | 6.1          3.15   0.24
scale@2      11.6 | 11.3     1.9 | 1.9     1.2 | 1.1     1.4 | 1.3     3.0 | 3.2   18.5 | 16.5   11.8 | 21.7     5.1 | 6.1          3.15   0.24
nosh           4.2 | 7.1     0.0 | 0.0     1.6 | 1.6     1.7 | 1.3     2.0 | 2.0     6.1 | 6.1     4.6 | 5.0     0.0 | 0.0          3.81   0.25
sh0_k1         4.2 | 7.1     1.1 | 1.1     1.6 | 1.6     1.7 | 1.3     2.0 | 2.0     6.1 | 6.1     4.6 | 5.0     1.7 | 1.7          3.81   0.25
sh0_k16        6.5 | 6.5     1.3 | 1.3     1.3 | 1.8     1.2 | 1.2     1.9 | 1.7     6.3 | 9.1     5.1 | 5.2     1.5 | 1.5          3.81   0.25
sh1_k4         8.0 | 9.4     1.7 | 1.7     1.6 | 1.6     1.5 | 1.4     7.3 | 7.3     8.9 | 9.1     5.6 | 6.8     1.6 | 1.6          3.90   0.25
sh1_k16        5.9 | 9.5     1.2 | 1.2     1.7 | 1.4     1.7 | 1.4     2.9 | 2.3    6.8 | 10.3    4.7 | 11.1     1.9 | 2.3          3.24   0.25
sh2_k9         8.4 | 7.8     1.4 | 1.4     1.2 | 1.6     1.4 | 1.5     2.4 | 2.4     7.0 | 7.0     6.6 | 6.0     2.3 | 2.3          3.82   0.23
sh2_k16        6.2 | 4.5     1.9 | 1.6     1.4 | 1.4     1.8 | 1.1     4.4 | 3.0     5.5 | 6.7     4.2 | 4.3     4.6 | 2.8          3.83   0.25
sh3_k16        6.0 | 7.8     1.9 | 1.9     1.4 | 1.7     1.7 | 1.4     2.8 | 2.5     6.5 | 8.2     8.0 | 8.7     3.5 | 4.3          3.91   0.25
wide         13.0 | 11.5     4.5 | 4.5     1.8 | 1.9     1.9 | 1.5             -             -             -             -             -   0.25
together     12.8 | 17.5     2.9 | 2.9     1.9 | 1.9     1.8 | 1.5     6.1 | 3.5   16.3 | 11.2  161.6 | 43.2     5.5 | 6.3          4.32   0.25

v_opac_logit has no floor from RefC("f32") (it evaluates o (1 - o), which is 0 in fp32 from logit 17 on): it is held to
8 x 2^-24 of v sigmoid'(x) in its cancellation-free fp64 form at every logit, -30 .. 30.
The screen position is held to 2 ulp32(max(|xy_rel|, 1)) -- the rounding of the stored number plus one for the final
add -- on every stratum, the 3840 x 2160 one included, where a plain fp32 evaluation is a hundred times over it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import project_cases as PC
from tests.util import PARAM_KEYS, splat_fields

pytestmark = pytest.mark.gpu

CASES = PC.all_cases()
NAMES = [n for n in CASES if n != "together"]
K8_NAMES = [n for n in NAMES if not CASES[n].k1_only]
SENTINEL = -77


def _note(name, key, value, bar):
    """Every figure is printed before it is asserted (pytest -s shows them; they are the table above)."""
    print(f"FIG {name:12s} {key:13s} measured {value:9.2f}  bar {bar:9.2f}")


def _dev(case, dev):
    return {k: (None if v is None else torch.from_numpy(v).float().to(dev).contiguous()) for k, v in case.P.items()}


def _k1(case, dev, D=None):
    """tgs_project_fwd into NaN-filled buffers with one sentinel row behind each -> (splats [N,12], radii [N])."""
    from touch_gs_amd import _lib, ops
    lib = _lib.load()
    D = D or _dev(case, dev)
    N = case.N
    sp = torch.full((N + 1, 12), float("nan"), dtype=torch.float32, device=dev)
    rad = torch.full((N + 1,), SENTINEL, dtype=torch.int32, device=dev)
    cs = case.amd_cam().c_struct()
    _lib.check(lib.tgs_project_fwd(C.byref(cs), N, _lib.ptr(D["means"]), _lib.ptr(D["log_scales"]), _lib.ptr(D["quats"]),
                                   _lib.ptr(D["opac_logit"]), _lib.ptr(D["sh"]), case.Ks, case.deg, None, _lib.ptr(sp),
                                   _lib.ptr(rad), ops._stream()), "tgs_project_fwd")
    assert torch.isnan(sp[N]).all() and int(rad[N]) == SENTINEL, "K1 wrote behind its last row"
    assert not torch.isnan(sp[:N]).any() and not (rad[:N] == SENTINEL).any()
    return sp[:N], rad[:N]


def _ulp32(x):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 1.0))) - 23)


def _check_k1(case, sp, rad):
    name = case.name
    f = {k: v.numpy() for k, v in splat_fields(sp, rad).items()}
    g = PC.geometry(case)
    ref = PC.ref_fwd(case)
    R = PC._refc("f64")
    cm = PC.constructed_mask(case)
    same = f["radius"] == ref["radius"]
    # integers: exact on every constructed Gaussian; the random fill keeps the project's 0.5 %
    assert same[cm].all(), (name, np.nonzero(~same & cm)[0])
    assert (~same).mean() <= 0.005, (name, (~same).mean())
    assert np.array_equal(f["visible"], f["radius"] > 0)
    culled = f["radius"] == 0
    assert (f["conic"][culled] == 0).all() and (f["hits"][culled] == 0).all()
    # opacity below 1/255 (tau2 <= 0): radius and conic are written, the rect is empty
    low = 255 * g["opac"] < 0.99
    assert (f["hits"][low] == 0).all() and (f["conic"][low & ~culled, 0] > 0).all()
    behind = ~g["front"]
    assert (f["xy_rel"][behind] == 0).all() and culled[behind].all()
    # packed rect: a subset of the normative rect ...
    rr, orr = f["rect"], ref["rect"]
    has = f["hits"] > 0
    sub = (rr[:, 0] >= orr[:, 0]) & (rr[:, 1] >= orr[:, 1]) & (rr[:, 2] <= orr[:, 2]) & (rr[:, 3] <= orr[:, 3])
    assert sub[has & same].all(), (name, np.nonzero(has & same & ~sub)[0])
    # ... and every dropped (tile, Gaussian) pair stays below 1/255 at all of its pixel centres
    tight = np.where(has[:, None], rr, 0).astype(np.int32)
    hit_ref = np.where(same, ref["tiles_hit"], 0).astype(np.int32)
    amax, ndrop = R.dropped_pairs_max_alpha(ref["xy"], ref["conic"], ref["opac"], ref["rect"], hit_ref, tight,
                                            PC.cam_block(R, case.cam), case.cam.W, case.cam.H)
    ray = np.zeros(case.N, bool)
    for t, idx in case.tags.items():
        if t.split("/")[-1] == "ray":
            ray[idx] = True
    assert (amax[~ray] < 1 / 255).all(), (name, np.nonzero((amax >= 1 / 255) & ~ray)[0], amax.max())
    assert (amax[ray] < 1.5 / 255).all(), (name, amax[ray].max())     # the known fp32-extent case
    # position: the stored relative number plus the (exact) rect origin against the fp64 position
    front = g["front"]
    err = np.abs(f["xy_rel"] + 16.0 * rr[:, 0:2] - g["xy"])[front]
    bar = 2 * _ulp32(f["xy_rel"][front])
    worst = (err / bar).max() if front.any() else 0.0
    _note(name, "xy/(2ulp)", worst, 1.0)
    assert (err <= bar).all(), (name, worst)
    # values
    bars = PC.bars(name)
    fe = PC.fwd_err(case, f, ref, g, same & ~culled)
    for k in PC.FWD_KEYS:
        m = float(fe[k][same].max()) if k != "rgb" else float(fe[k].max())     # colour is defined for every Gaussian
        _note(name, k, m, bars[k])
        assert m <= bars[k], (name, k, m, bars[k], int(np.argmax(fe[k])))
    return f, ref, g


@pytest.mark.parametrize("name", NAMES)
def test_k1_strata(dev, name):
    """Every stratum (SH degrees -1 .. 3 and both storage widths come with the sh strata) through tgs_project_fwd."""
    case = CASES[name]
    sp, rad = _k1(case, dev)
    _check_k1(case, sp.cpu(), rad.cpu())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 0])
def test_k1_sizes_and_fused(dev, n):
    """N of 1, 255, 256, 257 and all strata together (n = 0); together also through the fused tgs_project_bin_sort, whose
    records must be the stand-alone kernel's bit for bit (slot 11, the pair offset, is its own)."""
    from touch_gs_amd import ops
    tog = CASES["together"]
    case = tog if n == 0 else tog.take(np.arange(tog.N - n, tog.N), name="together")   # the tail holds constructed strata
    D = _dev(case, dev)
    sp, rad = _k1(case, dev, D)
    _check_k1(case, sp.cpu(), rad.cpu())
    if n == 0:
        sp2, rad2, *_ = ops.project_bin_sort(case.amd_cam(), D["means"], D["log_scales"], D["quats"], D["opac_logit"],
                                             D["sh"], case.deg, want_radii=True)
        assert torch.equal(sp2[:, :11].view(torch.int32), sp[:, :11].view(torch.int32)) and torch.equal(rad2, rad)


def test_k1_refuses_an_image_side_above_4080(dev):
    from touch_gs_amd import ops
    case = CASES["opacity"]
    D = _dev(case, dev)
    for W, H in ((4096, 96), (160, 4081)):
        cam = case.amd_cam()
        cam.W, cam.H = W, H
        with pytest.raises(RuntimeError, match="4080"):
            ops.project_fwd(cam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], case.deg)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# K8
# ---------------------------------------------------------------------------------------------
def _front(case, dev, D, **camkw):
    """K1 fused with binning -> records, radii, group bases, capacity, and per Gaussian its run (base, hits), checked
    on the host to lie inside the buffer and not to overlap: the kernels index the partials with nothing else."""
    from touch_gs_amd import ops
    cam = case.amd_cam(**camkw)
    sp, rad, gb, ts, sg, st = ops.project_bin_sort(cam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"],
                                                   case.deg, want_radii=True)
    n, ovf = st.tolist()
    assert ovf == 0
    cap = sg.shape[0]
    return cam, sp, rad, gb, cap


def _runs(sp, gb, cap):
    s = sp.cpu()
    hits = splat_fields(s)["hits"].numpy().astype(np.int64)
    off = s[:, 11].contiguous().view(torch.int32).numpy().astype(np.int64)
    base = gb.cpu().numpy().astype(np.int64)[np.arange(len(hits)) // 256] + off
    base = np.where(hits > 0, base, 0)
    live = hits > 0
    assert (base[live] >= 0).all() and (base[live] + hits[live] <= cap).all()
    o = np.argsort(base[live], kind="stable")
    b, h = base[live][o], hits[live][o]
    assert (b[1:] >= (b + h)[:-1]).all(), "runs overlap"
    return base, hits


def _partials(base, hits, cap, seed, dev):
    """NaN-filled [cap,12]; lognormal-scaled normal records in slots 0..9 of every run, NaN left in slots 10, 11.
    -> (device buffer, fp64 sum per Gaussian [N,10], sum of magnitudes [N,10])."""
    rng = np.random.default_rng(seed)
    N, tot = len(hits), int(hits.sum())
    owner = np.repeat(np.arange(N), hits)
    k = np.arange(tot) - np.repeat(np.cumsum(hits) - hits, hits)
    rows = base[owner] + k
    vals = PC.f32(rng.normal(size=(tot, 10)) * np.exp(rng.normal(size=(tot, 1))))
    buf = np.full((cap, 12), np.nan, np.float32)
    buf[rows, :10] = vals
    S, A = np.zeros((N, 10)), np.zeros((N, 10))
    np.add.at(S, owner, vals)
    np.add.at(A, owner, np.abs(vals))
    return torch.from_numpy(buf).to(dev), S, A


def _nan_outs(case, dev, with_sh=True):
    N = case.N
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    sh = e(N + 1, case.Ks, 3) if (with_sh and case.P["sh"] is not None) else None
    return [e(N + 1, 3), e(N + 1, 3), e(N + 1, 4), e(N + 1), sh]


def _check_outs(full, N):
    """No write behind the last row, every row written."""
    out = []
    for t in full:
        if t is None:
            out.append(None)
            continue
        assert torch.isnan(t[N:]).all(), "K8 wrote behind its last row"
        assert not torch.isnan(t[:N]).any()
        out.append(t[:N].cpu().double().numpy())
    return out


def _check_k8(case, form, got, vxy, v, vabs, v32, radius):
    """got: the five gradients (numpy).  v / vabs: the fp64 upstream and its un-cancelled magnitude [N,10]; v32: the fp32
    upstream as the kernel held it (its v_xy echo; for the partials forms K8a's sum, which test_k8a_segmented_sum and
    the partials tests bound on its own); radius: the kernel's own (it decides visibility by its record).
    The projection backward is linear in its upstream, so of the difference to the oracle exactly |J| |v32 - v| is the
    rounding of the upstream the kernel was handed or summed: that share is taken off, the rest meets the bar."""
    name, N = case.name, case.N
    g = PC.geometry(case)
    ref = PC.ref_bwd(case, v, radius)
    mass = PC.grad_mass(case, radius, vabs)
    dv = np.abs(v32 - v)
    slack = PC.grad_mass(case, radius, dv) if dv.any() else None
    gd = dict(zip(PARAM_KEYS, got))
    if gd["v_sh"] is None:
        gd["v_sh"] = np.zeros((N, 0, 3))
    bars = PC.bars(name)
    ge = PC.grad_err(case, gd, ref, mass, g["kappa"], slack)
    for k in PARAM_KEYS:
        if k == "v_opac_logit":
            continue
        m = float(ge[k].max())
        _note(name, k, m, bars[k])
        assert (ge[k] <= bars[k]).all(), (name, form, k, m, bars[k], int(np.argmax(ge[k])))
    # exact expectations
    culled = radius == 0
    assert (gd["v_log_scales"][culled] == 0).all() and (gd["v_quats"][culled] == 0).all()
    if case.P["sh"] is None:
        assert (gd["v_means"][culled] == 0).all()
    else:
        K = (case.deg + 1) ** 2
        vsh = gd["v_sh"].reshape(N, case.Ks, 3)
        assert (vsh[:, K:] == 0).all(), "SH rows above the active degree"
        clear = np.abs(g["pre"]) > 1e-5
        gated = (g["pre"] <= 0) & clear
        assert (vsh[:, :K][np.broadcast_to(gated[:, None, :], (N, K, 3))] == 0).all(), "gated channel"
        flows = (g["pre"] > 0) & clear & (v32[:, 7:10] != 0)
        assert (vsh[:, 0][flows] != 0).all()                       # colour gradients flow, culled or not
        assert (vsh[:, 0][flows & culled[:, None]] != 0).all()
    assert np.array_equal(vxy, v32[:, 0:2]), "v_xy echoes the upstream"
    # v_opac_logit = (fp32 upstream) * sigmoid'(x): a few ulp of the closed form at EVERY logit
    sd = PC.sigmoid_deriv(case.P["opac_logit"])
    err = np.abs(gd["v_opac_logit"] - v[:, 3] * sd) - 1.001 * dv[:, 3] * sd
    eo = np.where(err <= 0, 0.0, err / np.maximum(PC.EPS32 * np.abs(v32[:, 3]) * sd, 1e-300))
    _note(name, "v_opac_logit", float(eo.max()), PC.OPAC_LOGIT_BAR)
    assert (eo <= PC.OPAC_LOGIT_BAR).all(), (name, form, float(eo.max()), int(np.argmax(eo)))
    assert (gd["v_opac_logit"][(v32[:, 3] != 0)] != 0).all()        # opacity gradients flow, culled or not, at every logit


@pytest.mark.parametrize("name", K8_NAMES)
def test_k8_v_splats_form(dev, name):
    """(a) the upstream handed over as v_splats: always k_project_bwd."""
    from touch_gs_amd import ops
    case = CASES[name]
    D = _dev(case, dev)
    sp, rad = _k1(case, dev, D)
    v = PC.upstream(case)
    vs = torch.full((case.N, 12), float("nan"), dtype=torch.float32)     # slots 10, 11 are not the kernel's to read
    vs[:, :10] = torch.from_numpy(v).float()
    full = _nan_outs(case, dev)
    out = tuple(None if t is None else t[:case.N] for t in full)
    *_, vxy = ops.project_bwd(case.amd_cam(), D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], case.deg,
                              sp, v_splats=vs.to(dev), out=out, want_v_xy=True)
    got = _check_outs(full, case.N)
    _check_k8(case, "v_splats", got, vxy.cpu().double().numpy(), v, np.abs(v), v, rad.cpu().numpy())


def _k8_partials(case, dev, seed=9):
    from touch_gs_amd import ops
    D = _dev(case, dev)
    cam, sp, rad, gb, cap = _front(case, dev, D)
    base, hits = _runs(sp, gb, cap)
    buf, S, A = _partials(base, hits, cap, seed, dev)
    v32 = ops.reduce_partials(cam, sp, gb, buf).cpu().double().numpy()
    return D, cam, sp, rad, gb, buf, S, A, hits, v32


@pytest.mark.parametrize("name", K8_NAMES + ["together:1", "together:255", "together:257", "together"])
def test_k8_partials_form(dev, name):
    """(b) the upstream as hand-built partial records: storage of 4 or 16 bases runs k_project_bwd_lds (the form training
    uses), storage of 1 or 9 bases and sh=None run k_project_bwd with partials.  together:255 / :257 have a tail
    workgroup of the LDS form (nrows < 256), together:1 a single row."""
    from touch_gs_amd import ops
    nm, _, n = name.partition(":")
    case = CASES[nm]
    if n:
        case = case.take(np.arange(case.N - int(n), case.N), name=nm)
    D, cam, sp, rad, gb, buf, S, A, hits, v32 = _k8_partials(case, dev)
    assert (v32[:, 10:] == 0).all() and not np.isnan(v32).any()
    assert (np.abs(v32[:, :10] - S) <= hits[:, None] * PC.EPS32 * A).all()       # K8a's own bound, any summation order
    full = _nan_outs(case, dev)
    out = tuple(None if t is None else t[:case.N] for t in full)
    *_, vxy = ops.project_bwd(cam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], case.deg, sp,
                              group_base=gb, partials=buf, out=out, want_v_xy=True)
    got = _check_outs(full, case.N)
    _check_k8(case, "partials", got, vxy.cpu().double().numpy(), S, A, v32[:, :10], rad.cpu().numpy())


def test_k8_forms_agree(dev):
    """The two K8 kernels share one B.5 body (sh_color_bwd) and one geom_bwd and are compiled with fusion decided per
    source expression, so they give the same bits: on the last 257 rows of all strata together (two workgroups, the
    second with a single row) the partials form (k_project_bwd_lds: storage is 16 bases) equals the v_splats form
    (k_project_bwd) fed K8a's sum of the same records, in every output."""
    from touch_gs_amd import ops
    tog = CASES["together"]
    case = tog.take(np.arange(tog.N - 257, tog.N), name="together")
    assert case.Ks == 16 and case.P["sh"] is not None
    D, cam, sp, rad, gb, buf, S, A, hits, v32 = _k8_partials(case, dev)
    args = (cam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], case.deg, sp)
    lds = ops.project_bwd(*args, group_base=gb, partials=buf, want_v_xy=True)
    gen = ops.project_bwd(*args, v_splats=ops.reduce_partials(cam, sp, gb, buf), want_v_xy=True)
    for k, a, b in zip(PARAM_KEYS + ("v_xy",), lds, gen):
        assert not torch.isnan(a).any(), k
        assert torch.equal(a, b), (k, int((a != b).sum()))


@pytest.mark.parametrize("rows", [None, 256])
def test_k8_colour_form(dev, rows):
    """tgs_project_bwd_color on all strata together, whole and for rows (256, N): the geometry gradients meet the same
    bars, v_color is the clamp-gated upstream colour gradient exactly, the trailer holds the camera position and a zero
    flag, and a row-range call leaves the other rows alone."""
    from touch_gs_amd import ops
    case = CASES["together"]
    N = case.N
    D, cam, sp, rad, gb, buf, S, A, hits, v32 = _k8_partials(case, dev)
    b, e = (0, N) if rows is None else (rows, N)
    full = _nan_outs(case, dev, with_sh=False)
    out = tuple(t[:N] for t in full[:4])
    vc = torch.full((3 * (e - b) + 4 + 1,), float("nan"), dtype=torch.float32, device=dev)
    vxy = torch.full((N, 2), float("nan"), dtype=torch.float32, device=dev)
    ops.project_bwd_color(cam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], case.deg, sp, gb, buf, out,
                          vc[:-1], rows=None if rows is None else (b, e), v_xy=vxy, want_v_xy=True)
    for t in full[:4]:
        assert torch.isnan(t[N:]).all() and torch.isnan(t[:b]).all() and not torch.isnan(t[b:N]).any()
    assert torch.isnan(vc[-1]) and torch.isnan(vxy[:b]).all()
    vc = vc[:-1].cpu().double().numpy()
    g = PC.geometry(case)
    sub = case.take(np.arange(b, N), name="together")
    want = np.where(g["pre"] > 0, v32[:, 7:10], 0.0)[b:]
    clear = (np.abs(g["pre"]) > 1e-5)[b:]          # (all of the constructed strata; a random fill colour may sit on 0)
    assert clear.mean() > 0.999
    assert np.array_equal(vc[:3 * (e - b)].reshape(-1, 3)[clear], want[clear]), "v_color is the gated upstream colour gradient"
    Rw, tw = PC.cam_parts(case.cam)
    assert np.allclose(vc[3 * (e - b):3 * (e - b) + 3], -(Rw.T @ tw), rtol=1e-6, atol=1e-6) and vc[3 * (e - b) + 3] == 0
    # geometry gradients of the rows: same oracle, same bars; the SH gradient is not formed in this form
    ref_sh = PC.ref_bwd(sub, S[b:], rad.cpu().numpy()[b:])["v_sh"]
    got = [t[b:N].cpu().double().numpy() for t in full[:4]] + [ref_sh]
    _check_k8(sub, "colour", got, vxy[b:].cpu().double().numpy(), S[b:], A[b:], v32[b:, :10], rad.cpu().numpy()[b:])


# ---------------------------------------------------------------------------------------------
# K8a
# ---------------------------------------------------------------------------------------------
def _factor(h):
    """hits -> (w, h) with both sides <= 255 (the packed rect's fields), or None."""
    for a in range(1, 256):
        if h % a == 0 and h // a <= 255:
            return h // a, a
    return None


K8A_MUST = (0, 1, 63, 64, 65, 127, 128, 129, 1025, 2050)


def _k8a_hits(L, rng):
    """Per-Gaussian run lengths in four groups: (0) no long run -- the early exit; (1) a single long run among 255 short
    ones; (2) more than 16 long runs, among them every boundary value; (3) a last, partial group with a long run.
    L + 1 = 257 is prime and cannot be a packed rect (sides <= 255): 258 = 129 x 2 stands in for it."""
    ok = np.array([h for h in range(0, 700) if _factor(h) or h == 0])
    short = ok[ok <= L]
    lp1 = L + 1 if _factor(L + 1) else L + 2
    g0 = rng.choice(short, 256)
    g0[[3, 100, 255]] = [0, 1, L]
    g1 = rng.choice(short, 256)
    g1[rng.integers(0, 256)] = 1025
    g2 = rng.choice(short, 256)
    must = [h for h in K8A_MUST + (L, lp1)]
    long_more = rng.choice(ok[(ok > L) & (ok < 300)], 24)
    vals = np.concatenate([must, long_more])
    g2[rng.choice(256, len(vals), replace=False)] = vals
    g3 = rng.choice(short, 100)
    g3[37] = 130
    g3[99] = lp1
    return np.concatenate([g0, g1, g2, g3]).astype(np.int64), lp1


@pytest.mark.parametrize("L", [4, 32, 256])
def test_k8a_segmented_sum(dev, L):
    """ops.reduce_partials, and K8 with partials in both forms, against the plain fp64 sum of the records, with the
    long-run threshold L given per call (Camera.long_run).  Run lengths sit on the threshold (L, L + 1), on the
    64-record segment boundaries (63 .. 65, 127 .. 129) and beyond one 16-segment round (1025: 17 segments, the second
    round and the other buffer; 2050: 33, a third).  127 and 129 tiles cannot be a rectangle of a 40 x 30 tile image,
    so the records' rect and offset fields are written by hand onto the records K1 made for a 640 x 480 camera: K8a
    reads nothing else of a record, K8 besides them only the conic.
    Bar per component: |sum - ref| <= hits 2^-24 sum|x| -- the bound of ANY summation order, needing no measurement."""
    from touch_gs_amd import ops
    rng = np.random.default_rng(100 + L)
    hits, lp1 = _k8a_hits(L, rng)
    N = len(hits)
    cam0 = PC.camera(640, 480)
    assert cam0.tiles[0] * cam0.tiles[1] == 1200
    P = PC.generic(N, cam0, 7)
    P["means"] = PC.place(cam0, PC.on_screen(N, cam0, rng))
    case = PC.Case("k8a", P, cam0, 3, {})
    D = _dev(case, dev)
    cam = case.amd_cam(long_run=L)
    sp, rad = _k1(case, dev, D)
    # rect and offset fields by hand: runs in order with gaps of 0 .. 3 records (left NaN) between them
    gaps = rng.integers(0, 4, N)
    base = np.cumsum(hits + gaps) - hits
    cap = int(base[-1] + hits[-1] + 8)
    gb = base[::256].copy()
    gb[:] = [base[i] - int(rng.integers(0, 3)) for i in range(0, N, 256)]
    gb = np.maximum(gb, 0)
    off = base - gb[np.arange(N) // 256]
    wh = np.array([_factor(h) or (0, 0) for h in hits])
    rect = (rng.integers(0, 200, N) | (rng.integers(0, 200, N) << 8) | (wh[:, 0] << 16) | (wh[:, 1] << 24)).astype(np.uint32)
    rect[hits == 0] = 0
    rec = sp.cpu().clone()
    rec[:, 10] = torch.from_numpy(rect.view(np.float32).copy())
    rec[:, 11] = torch.from_numpy(off.astype(np.int32).view(np.float32).copy())
    rec = rec.to(dev)
    gbt = torch.from_numpy(gb.astype(np.int32)).to(dev)
    b2, h2 = _runs(rec, gbt, cap)            # read back FROM THE RECORDS: inside the buffer, disjoint
    assert np.array_equal(h2, hits) and np.array_equal(b2[hits > 0], base[hits > 0])
    seen = set(h2.tolist())
    assert set(K8A_MUST) | {L, lp1} <= seen and max(seen) >= 1025
    per_group = [h2[i:i + 256] for i in range(0, N, 256)]
    assert (per_group[0] <= L).all() and (per_group[1] > L).sum() == 1 and (per_group[2] > L).sum() > 16
    assert len(per_group[3]) < 256 and (per_group[3] > L).any()
    buf, S, A = _partials(b2, h2, cap, 200 + L, dev)
    v = ops.reduce_partials(cam, rec, gbt, buf).cpu().double().numpy()
    assert not np.isnan(v).any(), "NaN in the output: a read outside a run"
    assert (v[:, 10:] == 0).all()
    bound = h2[:, None] * PC.EPS32 * A
    worst = (np.abs(v[:, :10] - S) / np.maximum(bound, 1e-300) * (bound > 0)).max()
    print(f"FIG k8a L={L}: worst |sum - ref| / (hits 2^-24 sum|x|) = {worst:.3f}")
    assert (np.abs(v[:, :10] - S) <= bound).all(), (L, worst)
    # K8 forms its upstream with the same function: its v_xy echo is K8a's sum bit for bit, LDS form and plain form
    for sh in (D["sh"], None):
        *_, vxy = ops.project_bwd(cam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], sh, 3 if sh is not None else -1,
                                  rec, group_base=gbt, partials=buf, want_v_xy=True)
        assert np.array_equal(vxy.cpu().double().numpy(), v[:, 0:2]), "K8's sum differs from K8a's"
