"""The build's counterpart of ``ns-export``: a trained run as geometry other tools read.

    python -m touch_gs_amd.export tsdf --run <run_dir> --output-dir <dir> [--resolution 256 | --voxel-size m]
        [--bounds touch | gaussians | x0 y0 z0 x1 y1 z1] [--depth median|expected] [--weight inverse_variance|uniform]
        [--views train|all] [--mesh]
    python -m touch_gs_amd.export gaussians --run <run_dir> --output-dir <dir>

``tsdf`` renders the run's views, fuses their depth into a TSDF in HIP (touch_gs_amd.tsdf) and writes
``surface.ply`` (points, outward normals, colours: the grid's zero crossings), ``tsdf.npz`` (TsdfVolume.save) and, with
``--mesh``, ``mesh.ply`` (the same level set as a triangle mesh: marching tetrahedra in HIP), and
``export.json`` (grid, options, counts, seconds per stage and, for a capture with ``gt_depth/`` -- the analytic one --, the
surface metrics against the points back-projected from it).  ``gaussians`` writes the INRIA-layout ``point_cloud.ply`` that
splat viewers read.  Points, normals and Gaussians are in the CAPTURE's metric frame: the centring and the scale that the
data layer applies (dataset.Scene) are undone.  ``--voxel-size`` and explicit ``--bounds`` are in that frame too.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np

from .tsdf import fuse_model, mesh_stats, surface_metrics, write_ply, write_ply_table


def load_run(run_dir: str, device="cuda"):
    """(model, config dict, Scene) of a training run's newest checkpoint, rebuilt as run_eval.eval_run does."""
    from .dataset import Scene
    from .run_eval import load_model
    model, cfg, ckpt = load_model(run_dir, device)
    if cfg.get("synthetic") or not cfg.get("data"):
        raise ValueError("export needs a run trained on a capture (--data)")
    scene = Scene(cfg["data"], cfg["train_split_fraction"], device)
    return model, dict(cfg, checkpoint=ckpt), scene


def to_capture_frame(points, scene) -> np.ndarray:
    """Scaled-frame positions -> the capture's metric frame (fp64): the inverse of Scene's centring and scaling."""
    return np.asarray(points, dtype=np.float64) / scene.scale + scene._centre


def to_model_frame(points, scene) -> np.ndarray:
    return (np.asarray(points, dtype=np.float64) - scene._centre) * scene.scale


def choose_bounds(spec, model, scene):
    """(lo, hi, how): the box in the MODEL's (scaled) frame and which rule gave it ("touch", "gaussians", "explicit").  ``spec``: ["touch"] = the box around points_touch.npy padded by 20 % of its
    extent on every side; ["gaussians"] = the 1 - 99 percentile box of the means with opacity > 0.5; six numbers = the box
    itself, capture frame; None = touch when the capture has points_touch.npy, else gaussians."""
    touch = os.path.join(scene.root, "points_touch.npy")
    if spec is None:
        spec = ["touch"] if os.path.exists(touch) else ["gaussians"]
    if len(spec) == 6:
        box = np.asarray([float(x) for x in spec], dtype=np.float64)
        return to_model_frame(box[:3], scene), to_model_frame(box[3:], scene), "explicit"
    if spec == ["touch"]:
        pts = to_model_frame(np.load(touch), scene)
        lo, hi = pts.min(0), pts.max(0)
        pad = 0.2 * (hi - lo)
        return lo - pad, hi + pad, "touch"
    if spec == ["gaussians"]:
        import torch
        p = model.params
        m = p.means[torch.sigmoid(p.opac_logit) > 0.5].detach().double().cpu().numpy()
        if len(m) == 0:
            raise ValueError("no Gaussian with opacity > 0.5")
        return np.percentile(m, 1, axis=0), np.percentile(m, 99, axis=0), "gaussians"
    raise ValueError("--bounds takes touch, gaussians or six numbers")


def gt_surface_points(root: str, max_points: int = 400000) -> np.ndarray:
    """The analytic capture's object surface: gt_depth/<stem>.npy (camera-space z, metres) back-projected inside
    gt_object_mask/<stem>.npy for ALL views, capture frame; evenly thinned to at most ``max_points``."""
    with open(os.path.join(root, "transforms.json")) as f:
        meta = json.load(f)
    out = []
    for fr in meta["frames"]:
        stem = os.path.splitext(os.path.basename(fr["file_path"]))[0]
        dp, mp = os.path.join(root, "gt_depth", stem + ".npy"), os.path.join(root, "gt_object_mask", stem + ".npy")
        if not (os.path.exists(dp) and os.path.exists(mp)):
            continue
        z, m = np.load(dp).astype(np.float64), np.load(mp).astype(bool)
        m &= z > 0
        g = lambda k, d=None: fr.get(k, meta.get(k, d))
        H, W = z.shape
        vs, us = np.nonzero(m)
        x = (us + 0.5 - g("cx", W / 2)) / g("fl_x") * z[m]
        y = (vs + 0.5 - g("cy", H / 2)) / g("fl_y") * z[m]
        c2w = np.asarray(fr["transform_matrix"], dtype=np.float64)
        pc = np.stack([x, -y, -z[m]], -1)                    # OpenCV camera axes -> the file's OpenGL axes
        out.append(pc @ c2w[:3, :3].T + c2w[:3, 3])
    if not out:
        return np.zeros((0, 3))
    pts = np.concatenate(out)
    if len(pts) > max_points:
        pts = pts[np.linspace(0, len(pts) - 1, max_points).astype(np.int64)]
    return pts


def export_tsdf(run_dir: str, output_dir: str, resolution: int = 256, voxel_size=None, bounds=None, depth: str = "median",
                weight: str = "inverse_variance", views: str = "train", device="cuda", w_min: float = 0.5,
                loaded=None, mesh: bool = False, metrics_device=None) -> dict:
    """-> what export.json holds.  ``loaded`` = a (model, cfg, scene) of :func:`load_run`, to spare the reload.  ``mesh``:
    also write mesh.ply and add the ``mesh`` block (tsdf.mesh_stats in the capture's frame, and the seconds).
    ``metrics_device``: where the Chamfer / F-score's nearest neighbours are found -- None = scipy on the host, a GPU device =
    the HIP k-NN (tsdf.surface_metrics); recorded in the options."""
    import torch
    clock = time.perf_counter
    t0 = clock()
    model, cfg, scene = loaded or load_run(run_dir, device)
    idx = list(scene.i_train) if views == "train" else list(range(len(scene.views)))
    cams = [scene.views[i].cam for i in idx]
    lo, hi, how = choose_bounds(bounds, model, scene)
    t1 = clock()
    vol = fuse_model(model, cams, (lo, hi), resolution=resolution,
                     voxel_size=None if voxel_size is None else float(voxel_size) * scene.scale, depth=depth, weight=weight)
    torch.cuda.synchronize(vol.device)
    t2 = clock()
    cloud = vol.extract_points(w_min)
    t3 = clock()
    os.makedirs(output_dir, exist_ok=True)
    pts = to_capture_frame(cloud["points"], scene)
    write_ply(os.path.join(output_dir, "surface.ply"), pts, cloud["normals"], cloud["colors"])
    vol.save(os.path.join(output_dir, "tsdf.npz"))
    t4 = clock()
    vox_m = vol.voxel_size / scene.scale
    info = dict(run=run_dir, checkpoint=cfg["checkpoint"], frame="capture (metres)",
                grid=dict(dims=list(vol.dims), voxel_size_m=vox_m, trunc_m=vol.trunc / scene.scale,
                          origin_m=to_capture_frame(vol.origin, scene).tolist(), bounds=how, voxel_size_model=vol.voxel_size,
                          origin_model=vol.origin.tolist(), dataparser_scale=scene.scale, centre_m=scene._centre.tolist()),
                options=dict(depth=depth, weight=weight, views=views, resolution=resolution, voxel_size=voxel_size, w_min=w_min),
                counts=dict(views=len(cams), voxels=vol.num_voxels, observed_voxels=int((vol.Wt >= w_min).sum().item()),
                            points=int(len(pts))),
                seconds=dict(load=round(t1 - t0, 3), render_and_fuse=round(t2 - t1, 3), extract=round(t3 - t2, 3),
                             write=round(t4 - t3, 3)))
    if mesh:
        t5 = clock()
        m = vol.extract_mesh(w_min)
        t6 = clock()
        verts = to_capture_frame(m["vertices"], scene)
        write_ply(os.path.join(output_dir, "mesh.ply"), verts, m["normals"], m["colors"], m["faces"])
        t7 = clock()
        info["mesh"] = dict(mesh_stats(verts, m["faces"]), seconds=dict(extract=round(t6 - t5, 3), write=round(t7 - t6, 3)))
        t4 = clock()                                         # (the metrics' seconds below start after the mesh)
    if os.path.isdir(os.path.join(scene.root, "gt_depth")):
        gt = gt_surface_points(scene.root)
        if len(gt):
            info["surface_metrics"] = surface_metrics(pts, gt, tau=2 * vox_m, device=metrics_device)
            if metrics_device is not None:
                info["options"]["metrics_device"] = str(metrics_device)
            info["seconds"]["metrics"] = round(clock() - t4, 3)
    with open(os.path.join(output_dir, "export.json"), "w") as f:
        json.dump(info, f, indent=2)
    return info


def gaussian_ply_columns(means, sh, opac_logit, log_scales, quats):
    """(names, columns) of the INRIA Gaussian-splatting PLY: x y z nx ny nz f_dc_0..2 f_rest_* opacity scale_0..2 rot_0..3,
    all float.  ``sh`` [N,K,3]: f_dc = the degree-0 row, f_rest CHANNEL-MAJOR (all of red's K - 1 coefficients, then green's,
    then blue's); opacity and scales in their stored (logit / log) form; quaternions (w, x, y, z) as stored."""
    means, sh, opac_logit, log_scales, quats = (np.asarray(a, dtype=np.float32) for a in (means, sh, opac_logit, log_scales, quats))
    N, K = sh.shape[0], sh.shape[1]
    rest = np.transpose(sh[:, 1:, :], (0, 2, 1)).reshape(N, 3 * (K - 1))
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * (K - 1))] \
        + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    cols = [means[:, 0], means[:, 1], means[:, 2]] + [np.zeros(N, np.float32)] * 3 + [sh[:, 0, i] for i in range(3)] \
        + [rest[:, i] for i in range(rest.shape[1])] + [opac_logit.reshape(N)] + [log_scales[:, i] for i in range(3)] \
        + [quats[:, i] for i in range(4)]
    return names, cols


def write_gaussian_ply(path: str, means, sh, opac_logit, log_scales, quats) -> None:
    names, cols = gaussian_ply_columns(means, sh, opac_logit, log_scales, quats)
    write_ply_table(path, names, cols)


def export_gaussians(run_dir: str, output_dir: str, device="cuda", loaded=None) -> dict:
    """point_cloud.ply of the run's Gaussians in the capture frame: positions un-centred and un-scaled, log scales shifted
    by -log(dataparser scale); rotations, opacities and SH coefficients are frame-independent."""
    model, cfg, scene = loaded or load_run(run_dir, device)
    p = model.params
    host = lambda t: t.detach().cpu().numpy()
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, "point_cloud.ply")
    write_gaussian_ply(path, to_capture_frame(host(p.means), scene), host(p.sh), host(p.opac_logit),
                       host(p.log_scales).astype(np.float64) - np.log(scene.scale), host(p.quats))
    return dict(path=path, gaussians=int(p.N), sh_coefficients=int(p.K))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Export a trained run as geometry.")
    sub = ap.add_subparsers(dest="what", required=True)
    t = sub.add_parser("tsdf", help="surface.ply + tsdf.npz + export.json from a TSDF fusion of the rendered depth")
    g = sub.add_parser("gaussians", help="point_cloud.ply in the INRIA layout")
    for s in (t, g):
        s.add_argument("--run", required=True, help="a run directory (config.json + step-*.ckpt)")
        s.add_argument("--output-dir", "--output_dir", dest="output_dir", required=True)
        s.add_argument("--device", default="cuda")
    t.add_argument("--resolution", type=int, default=256, help="voxels along the longest side of the bounds")
    t.add_argument("--voxel-size", type=float, default=None, help="metres; overrides --resolution")
    t.add_argument("--bounds", nargs="+", default=None, help="touch | gaussians | x0 y0 z0 x1 y1 z1 (metres, capture frame)")
    t.add_argument("--depth", choices=("median", "expected"), default="median")
    t.add_argument("--weight", choices=("inverse_variance", "uniform"), default="inverse_variance")
    t.add_argument("--views", choices=("train", "all"), default="train")
    t.add_argument("--mesh", action="store_true", help="also write mesh.ply: the level set as a triangle mesh")
    t.add_argument("--metrics-device", "--metrics_device", dest="metrics_device", default=None,
                   help="find the surface metrics' nearest neighbours with the HIP k-NN on this device (e.g. cuda); "
                        "default: scipy cKDTree on the host")
    a = ap.parse_args(argv)
    if a.what == "tsdf":
        info = export_tsdf(a.run, a.output_dir, a.resolution, a.voxel_size, a.bounds, a.depth, a.weight, a.views, a.device,
                           mesh=a.mesh, metrics_device=a.metrics_device)
    else:
        info = export_gaussians(a.run, a.output_dir, a.device)
    print(json.dumps(info))
    return info


if __name__ == "__main__":
    main()
