"""Per-view camera pose refinement (Splatfacto's ``camera_optimizer`` counterpart).

The device side is ``ops.pose_grad``: the raw gradient G = [G_R | G_p] of the step's loss w.r.t. rows 0-2 of the
world->camera matrix V = [R | p].  Everything here is host arithmetic in fp64 on 12 numbers per step.

Parametrisation: left-multiplied, in the camera frame, by retraction (no Jacobian of the exponential map):

    g_ups = G_p,    g_phi = sum_j R[:,j] x G_R[:,j] + p x G_p          (gradient at phi = ups = 0)
    (dphi, dups) = Adam(g_phi, g_ups)
    R <- exp([dphi]x) R,    p <- exp([dphi]x) p + dups                  (Rodrigues; R re-orthonormalised every 100 updates)

The optional L2 terms pull the accumulated change back to the original pose V0: with w = log(R R0^T) and
d = p - (R R0^T) p0 they add 2 l2_rot w to g_phi and 2 l2_trans d to g_ups.

No host synchronisation on the training path: a step's [32] result is copied asynchronously into the view's pinned slot
behind an event, and the update is applied immediately before the view is next used (as the step's view or as its
announced next view) -- a pose matters only when its view is rendered, so this is the immediate update.  With at least
one other step between a view's step and its next use or announcement -- any loop over three or more views that announces
the next view, two or more without -- the event has fired by then; in a two-view loop with announced next views (and with a
single view) ``event.synchronize()`` waits for the step just enqueued.
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

REORTHO_EVERY = 100


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rodrigues(w) -> np.ndarray:
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K)


def rot_log(R) -> np.ndarray:
    """Rotation vector of a rotation matrix (angle < pi)."""
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1.0, 1.0))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return 0.5 * w if th < 1e-8 else w * (th / (2 * np.sin(th)))


def retract(R, p, dphi, dups):
    E = rodrigues(dphi)
    return E @ R, E @ p + np.asarray(dups, np.float64)


def orthonormalise(R) -> np.ndarray:
    """The nearest rotation (polar factor through the SVD)."""
    U, _, Vt = np.linalg.svd(R)
    if np.linalg.det(U @ Vt) < 0:
        U[:, 2] = -U[:, 2]
    return U @ Vt


def tangent(G, R, p):
    """(g_phi, g_ups) from the raw 3x4 gradient G = [G_R | G_p] at the pose (R, p)."""
    G = np.asarray(G, np.float64).reshape(3, 4)
    g_phi = np.cross(p, G[:, 3])
    for j in range(3):
        g_phi = g_phi + np.cross(R[:, j], G[:, j])
    return g_phi, G[:, 3].copy()


class Adam6:
    """Adam on the 6-vector (phi, ups) with one learning rate for each half."""

    def __init__(self, lr_rot, lr_trans, betas=(0.9, 0.999), eps=1e-15):
        self.lr = np.array([lr_rot] * 3 + [lr_trans] * 3, np.float64)
        self.b1, self.b2, self.eps = float(betas[0]), float(betas[1]), float(eps)
        self.m, self.v, self.t = np.zeros(6), np.zeros(6), 0

    def step(self, g) -> np.ndarray:
        g = np.asarray(g, np.float64)
        self.t += 1
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        mh, vh = self.m / (1 - self.b1 ** self.t), self.v / (1 - self.b2 ** self.t)
        return -self.lr * mh / (np.sqrt(vh) + self.eps)


@dataclasses.dataclass
class _Slot:
    view: object
    V0: np.ndarray
    adam: Adam6
    pinned: Optional[torch.Tensor] = None
    event: Optional[torch.cuda.Event] = None
    pending: bool = False
    dropped: int = 0


class PoseRefiner:
    """Original pose, current pose (``view.cam.viewmat``), Adam moments and step count of every training view, on the host
    in fp64.  ``views`` are the FULL-resolution training views; held-out views are simply not given."""

    def __init__(self, views: Sequence, lr_rot: float, lr_trans: float, betas=(0.9, 0.999), eps: float = 1e-15,
                 l2_rot: float = 0.0, l2_trans: float = 0.0, model=None):
        # model: whose memo of tuned cameras (model._tuned_cams, keyed by camera identity) must forget a replaced camera
        self.model = model
        self.lr_rot, self.lr_trans, self.betas, self.eps = float(lr_rot), float(lr_trans), tuple(betas), float(eps)
        self.l2_rot, self.l2_trans = float(l2_rot), float(l2_trans)
        self.views = list(views)
        self._slots: Dict[int, _Slot] = {}
        for v in self.views:
            self._slots[id(v)] = _Slot(v, np.array(v.cam.viewmat, np.float64), Adam6(lr_rot, lr_trans, betas, eps))

    def owns(self, view) -> bool:
        s = self._slots.get(id(view))
        return s is not None and s.view is view

    # -- the training path ---------------------------------------------------------------------
    def submit(self, view, result: torch.Tensor) -> None:
        """Queue the [32] device result of the step just enqueued on ``view``: async copy + event, no sync."""
        s = self._slots[id(view)]
        if s.pending:          # the caller did not announce the view's re-use: settle the older result first
            self.apply_pending(view)
        if s.pinned is None:
            s.pinned = torch.empty(32, dtype=torch.float32).pin_memory()
            s.event = torch.cuda.Event()
        s.pinned.copy_(result, non_blocking=True)
        s.event.record()
        s.pending = True

    def apply_pending(self, view, model=None) -> bool:
        """Apply the queued update of ``view`` (if any) and give it a new Camera object; -> whether the pose changed.
        ``model``: its memo of tuned cameras drops the old camera's entry."""
        s = self._slots.get(id(view))
        if s is None or not s.pending:
            return False
        s.event.synchronize()
        s.pending = False
        return self.apply(view, s.pinned.numpy().astype(np.float64), model)

    def apply(self, view, out32, model=None) -> bool:
        """One optimizer update of ``view`` from a [32] result on the host."""
        s = self._slots[id(view)]
        out32 = np.asarray(out32, np.float64)
        if out32[24] == 0 or not np.isfinite(out32[:12]).all():    # voided frame (overflow): nothing to learn from
            s.dropped += 1
            return False
        V = np.array(view.cam.viewmat, np.float64)
        R, p = V[:3, :3], V[:3, 3]
        g_phi, g_ups = tangent(out32[:12], R, p)
        if self.l2_rot > 0 or self.l2_trans > 0:
            D = R @ s.V0[:3, :3].T
            g_phi = g_phi + 2 * self.l2_rot * rot_log(D)
            g_ups = g_ups + 2 * self.l2_trans * (p - D @ s.V0[:3, 3])
        d = s.adam.step(np.concatenate([g_phi, g_ups]))
        R, p = retract(R, p, d[:3], d[3:])
        if s.adam.t % REORTHO_EVERY == 0:
            R = orthonormalise(R)
        V = np.eye(4)
        V[:3, :3], V[:3, 3] = R, p
        self.set_pose(view, V, model)
        return True

    def set_pose(self, view, V, model=None) -> None:
        old = view.cam
        model = model if model is not None else self.model
        if model is not None:     # the replaced camera and its downscaled forms will never be asked for again
            for c in [old] + [v.cam for v in view.__dict__.get("_downscaled", {}).values()]:
                model._tuned_cams.pop(id(c), None)
        view.set_camera(dataclasses.replace(old, viewmat=np.array(V, np.float64)))

    def flush(self, model=None) -> None:
        for s in self._slots.values():
            self.apply_pending(s.view, model)

    # -- reporting and state ---------------------------------------------------------------------
    def deltas(self):
        """Per view (rotation angle in degrees, distance of the camera centres) against the original pose."""
        out = []
        for s in self._slots.values():
            V, V0 = np.asarray(s.view.cam.viewmat, np.float64), s.V0
            ang = np.degrees(np.linalg.norm(rot_log(V[:3, :3] @ V0[:3, :3].T)))
            out.append((float(ang), float(np.linalg.norm(-V[:3, :3].T @ V[:3, 3] + V0[:3, :3].T @ V0[:3, 3]))))
        return out

    def poses(self):
        """[(V0, V)] in the order of ``views``."""
        return [(s.V0.copy(), np.array(s.view.cam.viewmat, np.float64)) for s in self._slots.values()]

    def state_dict(self, model=None) -> dict:
        """fp64 / int64 host tensors (plain tensors, so that a checkpoint loads under ``weights_only``)."""
        self.flush(model)
        sl = list(self._slots.values())
        T = lambda rows, dt=np.float64: torch.from_numpy(np.stack([np.asarray(r, dt) for r in rows]))
        return dict(V0=T([s.V0 for s in sl]), V=T([s.view.cam.viewmat for s in sl]), m=T([s.adam.m for s in sl]),
                    v=T([s.adam.v for s in sl]), t=T([s.adam.t for s in sl], np.int64))

    def load_state_dict(self, sd: dict, model=None) -> None:
        sl = list(self._slots.values())
        sd = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in sd.items()}
        if len(sd["V"]) != len(sl):
            raise ValueError(f"checkpoint holds the poses of {len(sd['V'])} views, the refiner {len(sl)}")
        for i, s in enumerate(sl):
            s.pending = False
            s.V0 = np.array(sd["V0"][i], np.float64)
            s.adam.m, s.adam.v, s.adam.t = np.array(sd["m"][i], np.float64), np.array(sd["v"][i], np.float64), int(sd["t"][i])
            self.set_pose(s.view, sd["V"][i], model)


POSES_FILE = "refined_poses.json"


def save_refined_poses(run_dir: str, refiner: PoseRefiner, names: Sequence[str]) -> str:
    """<run_dir>/refined_poses.json: per training image its original and its refined world->camera matrix."""
    refiner.flush()
    path = os.path.join(run_dir, POSES_FILE)
    with open(path, "w") as f:
        json.dump({n: dict(V0=V0.tolist(), V=V.tolist()) for n, (V0, V) in zip(names, refiner.poses())}, f, indent=1)
    return path


def apply_refined_poses(run_dir: str, views: Sequence, names: Sequence[str]) -> int:
    """Give the views whose names the run's refined_poses.json lists (its training views) their refined cameras;
    -> how many.  A run without the file changes nothing."""
    path = os.path.join(run_dir, POSES_FILE)
    if not os.path.exists(path):
        return 0
    with open(path) as f:
        poses = json.load(f)
    n = 0
    for v, name in zip(views, names):
        if name in poses:
            v.set_camera(dataclasses.replace(v.cam, viewmat=np.array(poses[name]["V"], np.float64)))
            n += 1
    return n

