"""The build's counterpart of the reference's ``experiment_utils/run_eval.py`` (which shells out to
``ns-eval`` and ``ns-render dataset``, :37-57): walks the run directories of one scene newest first,
evaluates the last checkpoint of each and writes

    <output_dir>/<exp_name>/<exp_name>_<k>.json     k = 1 .. past_n_trials   (run_eval.py:40-43)
    <exp_name>_renders/                             eval-view renders        (run_eval.py:48)

with the ``results`` keys the reference's aggregator reads (experiment_utils/get_results.py:35-52:
psnr, ssim, lpips (NaN: needs pretrained weights), depth_mse, supervised_depth_mse and -- when
IS_REAL_WORLD is exported as scripts/train_bunny_real.sh:54 does -- gt_depth_mse, gt_object_depth_mse).

    IS_REAL_WORLD=True python -m touch_gs_amd.run_eval --input_dir outputs/<scene>/depth-gaussian-splatting \\
        --output_dir experiments --exp_name bunny_real_exp --past_n_trials 1
"""
from __future__ import annotations

import argparse
import glob
import json
import os

import torch


def load_model(run_dir: str, device="cuda"):
    """(model, config dict, checkpoint path): the model of one training run rebuilt from its config.json + newest checkpoint."""
    from .model import DepthGaussianSplattingModel, ModelConfig
    from .optim import GaussianParams
    with open(os.path.join(run_dir, "config.json")) as f:
        cfg = json.load(f)
    ckpts = sorted(glob.glob(os.path.join(run_dir, "step-*.ckpt")))
    if not ckpts:
        raise FileNotFoundError(f"no checkpoint in {run_dir}")
    sd = torch.load(ckpts[-1], map_location=device)
    mc = {k: v for k, v in cfg["model"].items() if k in ModelConfig.__dataclass_fields__}
    mc["background_color"] = tuple(mc.get("background_color", (0.0, 0.0, 0.0)))
    model = DepthGaussianSplattingModel(ModelConfig(**mc), GaussianParams.allocate(sd["N"], sd["K"], device))
    model.load_state_dict(sd)
    return model, cfg, ckpts[-1]


def eval_run(run_dir: str, out_json: str, render_dir=None, device="cuda", depth_stats: bool = False,
             normals: bool = False, normal_dir=None, normal_frame=None, surface: bool = False, metrics_device=None,
             color_correct: bool = False) -> dict:
    """Rebuild the model of one training run from its config.json + newest checkpoint and evaluate
    it on the run's eval split.  ``depth_stats``: the results gain median_depth_mse / gt_depth_mse_median /
    gt_object_depth_mse_median and the render dump median_depth/ and uncertainty/ (train.render_views).  ``normals``: the
    results gain normal_angle_deg (against the run's own normal priors, or those of ``normal_dir`` / ``normal_frame`` if
    given) and the render dump normal/.  ``surface``: the run's surface is exported beside the results
    (touch_gs_amd.export.export_tsdf with its defaults -> ``<out_json stem>_surface/``) and, when the capture has ground truth
    (``gt_depth/``), the results gain surface_chamfer / surface_precision / surface_recall / surface_fscore;
    ``metrics_device``: passed to export_tsdf (None = scipy on the host, a GPU device = the HIP k-NN).  ``color_correct``:
    the results gain cc_psnr / cc_ssim (train.evaluate: each render fitted to its ground truth by a least-squares 3x4 affine
    colour transform before the metric); no other key changes."""
    from .dataset import Scene
    from .train import evaluate, render_views
    model, cfg, ckpt = load_model(run_dir, device)
    if cfg.get("synthetic"):
        from .scene import make_view
        N, W, H = cfg["synthetic"]
        views = [make_view(N, W, H, cfg["sh_degree"], 1235, device, view=7, n_views=8)]
        names, scale = None, 1.0
    else:
        scene = Scene(cfg["data"], cfg["train_split_fraction"], device,
                      normal_dir=(normal_dir or cfg.get("normal_dir")) if normals else None,
                      normal_frame=normal_frame or cfg.get("normal_frame") or "opencv")
        from .pose import apply_refined_poses
        apply_refined_poses(run_dir, scene.views, scene.names)   # training views as the run left them (held-out ones are not listed)
        idx = list(scene.i_eval) or list(scene.i_train)[:1]
        views, names, scale = [scene.views[i] for i in idx], [scene.names[i] for i in idx], scene.scale
    results = evaluate(model, views, depth_stats=depth_stats, normals=normals, color_correct=color_correct)
    results.setdefault("lpips", float("nan"))   # get_results.py:38 indexes it unconditionally
    if surface:
        if cfg.get("synthetic"):
            raise ValueError("--surface needs a run trained on a capture")
        from .export import export_tsdf
        info = export_tsdf(run_dir, os.path.splitext(os.path.abspath(out_json))[0] + "_surface", device=device,
                           loaded=(model, dict(cfg, checkpoint=ckpt), scene), metrics_device=metrics_device)
        for k in ("chamfer", "precision", "recall", "fscore"):
            if "surface_metrics" in info:
                results["surface_" + k] = info["surface_metrics"][k]
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump({"experiment_name": os.path.basename(os.path.dirname(os.path.dirname(run_dir))),
                   "method_name": "depth-gaussian-splatting", "checkpoint": ckpt, "results": results}, f, indent=2)
    if render_dir:
        render_views(model, views, render_dir, names, depth_stats=depth_stats, dataparser_scale=scale, normals=normals)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser(description="Run evaluation on the output directories.")
    ap.add_argument("--input_dir", required=True, help="outputs/<scene>/depth-gaussian-splatting")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--exp_name", required=True)
    ap.add_argument("--past_n_trials", type=int, required=True)
    ap.add_argument("--no_render", action="store_true")
    ap.add_argument("--depth-stats", "--depth_stats", dest="depth_stats", action="store_true",
                    help="also evaluate the median depth and dump median_depth/ + uncertainty/ (rendered depth variance, "
                         "uint16 like the input uncertainty maps)")
    ap.add_argument("--normals", action="store_true",
                    help="also render the normals of the depth: normal/ PNGs ((n + 1) / 2, OpenCV camera axes) and, for runs "
                         "trained with --normal-dir, normal_angle_deg")
    ap.add_argument("--surface", action="store_true",
                    help="also export the run's surface (python -m touch_gs_amd.export tsdf, defaults) next to the results "
                         "and, for a capture with gt_depth/, add surface_chamfer / _precision / _recall / _fscore")
    ap.add_argument("--metrics-device", "--metrics_device", dest="metrics_device", default=None,
                    help="--surface: find the metrics' nearest neighbours with the HIP k-NN on this device (e.g. cuda); "
                         "default: scipy cKDTree on the host")
    ap.add_argument("--color-correct", "--color_correct", dest="color_correct", action="store_true",
                    help="also report cc_psnr / cc_ssim: each render is fitted to its ground truth by a least-squares 3x4 affine "
                         "colour transform before the metric (the evaluation of runs with per-view colour models: --exposure-lr, "
                         "--bilagrid-lr); the other keys do not change")
    a = ap.parse_args(argv)
    full_exp_dir = os.path.join(a.output_dir, a.exp_name)
    os.makedirs(full_exp_dir, exist_ok=True)
    done = []
    for run in sorted(os.listdir(a.input_dir))[::-1]:            # newest first (timestamped names)
        run_dir = os.path.join(a.input_dir, run)
        if not os.path.exists(os.path.join(run_dir, "config.json")):
            continue
        out_json = os.path.join(full_exp_dir, f"{a.exp_name}_{len(done) + 1}.json")
        res = eval_run(run_dir, out_json, None if a.no_render else f"{a.exp_name}_renders", depth_stats=a.depth_stats,
                       normals=a.normals, surface=a.surface, metrics_device=a.metrics_device,
                       color_correct=a.color_correct)
        print(out_json, json.dumps(res))
        done.append(out_json)
        if len(done) == a.past_n_trials:
            break
    return done


if __name__ == "__main__":
    main()
