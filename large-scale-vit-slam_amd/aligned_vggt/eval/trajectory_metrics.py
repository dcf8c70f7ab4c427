"""ATE / RPE / scale consistency (eval/trajectory_metrics.py of the reference),
restated without the ``torchmetrics`` dependency, which is absent from this
image.

Same public surface: ``update(preds, target)`` with (N, 4, 4) camera-to-world
poses, ``compute()`` -> dict with the reference's keys, ``detailed`` flag and
RPE ``delta``, ``plot(preds, target, title, outpath)`` -> (dict, path); plus
``reset()`` and ``sync(group)``, the latter standing in for torchmetrics'
``dist_reduce_fx`` ("cat": all ranks' error lists concatenated in rank order;
"sum" for ScaleConsistency).  Pinned by tests/golden/trajectory_metrics.npz
and ref_metrics.npz, produced by the reference's own bodies.

State lives on the host by default and ``update`` is then the reference's chain
of torch ops.  ``to(device | tensor)`` moves it; with the state and fp32 inputs
on one HIP device, ``update`` / ``update_batch`` are one ``vggt_trajectory_errors``
launch (csrc/pose.hip: fp64 from the fp32 poses, rounded once, the general 4x4
inverse) plus the concatenations, and nothing synchronises with the host.
``plot`` takes the kernel whenever its inputs are fp32 on a HIP device.  One
difference: a singular pose gives non-finite errors on the kernel route where
``torch.linalg.inv`` raises.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ..utils.geometry import closed_form_inverse_se3
from ..utils.pose_enc import pose_encoding_to_extri_intri


def _cat_across_ranks(t: torch.Tensor, group=None) -> torch.Tensor:
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return t
    W = dist.get_world_size(group)
    n = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
    ns = [torch.zeros_like(n) for _ in range(W)]
    dist.all_gather(ns, n, group=group)
    m = int(max(x.item() for x in ns))
    pad = torch.zeros((m,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[: t.shape[0]] = t
    outs = [torch.zeros_like(pad) for _ in range(W)]
    dist.all_gather(outs, pad, group=group)
    return torch.cat([o[: int(k.item())] for o, k in zip(outs, ns)], 0)


def _new_figure(size, title: Optional[str]):
    """A figure drawn by the Agg canvas alone: pyplot is not imported, so the backend a
    caller selected for the process (a notebook's, an interactive one) stays as it is and
    no figure is registered anywhere that would need closing."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    fig = Figure(figsize=size)
    FigureCanvasAgg(fig)
    if title:
        fig.suptitle(title, fontsize=10, fontweight="bold")
    return fig, fig.subplots()


def _curve_figure(title: Optional[str], heading: str, steps, curves):
    """One curve per entry of ``curves`` = (values, colour, axis label, legend label) over
    ``steps``, each on a y axis of its own colour (the second and later ones twinned)."""
    fig, first = _new_figure((7, 4), title)
    first.set_xlabel("Frame index")
    for k, (values, colour, axis_label, label) in enumerate(curves):
        ax = first if k == 0 else first.twinx()
        ax.plot(steps, values, colour + "-", label=label)
        ax.set_ylabel(axis_label, color=colour)
        ax.tick_params(axis="y", labelcolor=colour)
    first.set_title(heading, fontsize=10)
    fig.tight_layout()
    return fig


def _write_plot(fig, outpath: Optional[str], stem: str, data: dict) -> str:
    """Write ``{outpath}{stem}.png`` (300 dpi) and the plotted data as ``{outpath}{stem}.npy``
    when there is an ``outpath``; the path of the image is returned either way, formatted
    from ``outpath`` as it is (the reference does the same with its missing one)."""
    path = f"{outpath}{stem}.png"
    if outpath:
        fig.savefig(path, dpi=300)
        np.save(f"{outpath}{stem}.npy", data)
    return path


def _kernel_inputs(*ts) -> bool:
    """fp32 tensors on one HIP device."""
    return all(t.is_cuda and t.dtype == torch.float32 and t.device == ts[0].device for t in ts)


def _check_poses(preds: torch.Tensor, target: torch.Tensor) -> None:
    assert preds.shape == target.shape, "Preds and targets must have the same shape"
    assert preds.shape[-2:] == (4, 4), "Poses must be 4x4 matrices"


def _errors(preds: torch.Tensor, target: torch.Tensor, delta: int = 1, **want) -> dict:
    """vggt_trajectory_errors on (B, S, 4, 4) poses (detached, made contiguous)."""
    from .. import _native
    return _native.trajectory_errors(preds.detach().contiguous(), target.detach().contiguous(), delta, **want)


class _TrajectoryMetric:
    """State handling shared by the three metrics: ``_state`` names the state tensors."""
    _state: Tuple[str, ...] = ()

    def to(self, target):
        """Move the state to a device, or to the device of a tensor (as the reference's
        ``metric.to(gt_poses)``); returns self."""
        device = target.device if isinstance(target, torch.Tensor) else torch.device(target)
        for name in self._state:
            setattr(self, name, getattr(self, name).to(device))
        return self

    def _device_route(self, preds: torch.Tensor, target: torch.Tensor) -> bool:
        state = getattr(self, self._state[0])
        return state.is_cuda and _kernel_inputs(preds, target) and preds.device == state.device

    def update_batch(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        """``update`` for every sequence of (B, S, 4, 4) poses: one launch on the device
        route, a loop over the batch otherwise."""
        assert preds.dim() == 4, "update_batch: (B, S, 4, 4) poses"
        _check_poses(preds, target)
        if self._device_route(preds, target):
            return self._update_device(preds, target)
        for p, g in zip(preds, target):
            self.update(p, g)

    def __call__(self, preds, target):
        return self.update(preds, target)


class AbsoluteTrajectoryError(_TrajectoryMetric):
    """RMSE of camera-centre differences (trajectory_metrics.py:11-134)."""
    _state = ("errors", "per_dim_errors")

    def __init__(self, detailed: bool = False, **kwargs):
        self.detailed = detailed
        self.reset()

    def reset(self) -> None:
        device = self.errors.device if hasattr(self, "errors") else None
        self.errors = torch.tensor([], dtype=torch.float32, device=device)
        self.per_dim_errors = torch.tensor([], dtype=torch.float32, device=device)

    def _update_device(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        out = _errors(preds, target, ate=True, rpe=False, scale=False)
        self.errors = torch.cat([self.errors, out["ate_norm"].reshape(-1)])
        self.per_dim_errors = torch.cat([self.per_dim_errors, out["ate_vec"].reshape(-1, 3)])

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        assert preds.shape == target.shape, "Preds and targets must have the same shape"
        assert preds.shape[-2:] == (4, 4), "Poses must be 4x4 matrices"
        if self._device_route(preds, target):
            return self._update_device(preds[None], target[None])
        err = preds[:, :3, 3] - target[:, :3, 3]
        trans = torch.linalg.norm(err, dim=1)
        self.errors = torch.cat([self.errors, trans.detach().to(self.errors.device)])
        self.per_dim_errors = torch.cat([self.per_dim_errors, err.detach().to(self.per_dim_errors.device)])

    def sync(self, group=None) -> None:
        self.errors = _cat_across_ranks(self.errors, group)
        self.per_dim_errors = _cat_across_ranks(self.per_dim_errors.reshape(-1, 3), group)

    def compute(self) -> dict:
        e, pd = self.errors, self.per_dim_errors
        rmse = torch.sqrt(torch.mean(e ** 2)).item()
        if not self.detailed:
            return {"ate_rmse": rmse}
        return {"ate_rmse": rmse, "ate_mean": torch.mean(e).item(), "ate_median": torch.median(e).item(),
                "ate_std": torch.std(e).item(), "ate_min": torch.min(e).item(), "ate_max": torch.max(e).item(),
                "ate_rmse_per_dim": torch.sqrt(torch.mean(pd ** 2, dim=0)).tolist()}

    def plot(self, preds: torch.Tensor, target: torch.Tensor, title: Optional[str] = None,
             outpath: Optional[str] = None) -> Tuple[dict, str]:
        """trajectory_metrics.py:79-134: the metric of one (N, 4, 4) trajectory and its
        top view (x against z): both tracks and a thin segment from every GT position to
        its prediction.  ``{outpath}traj_ate.png`` / ``.npy`` are written only with
        ``outpath``.  Returns ``({"ate_rmse": float}, path)``."""
        from matplotlib.collections import LineCollection
        _check_poses(preds, target)
        if _kernel_inputs(preds, target):
            out = _errors(preds[None], target[None], ate=True, rpe=False, scale=False)
            err, trans = out["ate_vec"][0], out["ate_norm"][0]
        else:
            err = preds[:, :3, 3] - target[:, :3, 3]
            trans = torch.linalg.norm(err, dim=1)
        rmse = torch.sqrt(torch.mean(trans ** 2)).item()
        per_dim = torch.sqrt(torch.mean(err ** 2, dim=0)).tolist()
        tracks = {"Ground Truth": ("k-", target[:, :3, 3].detach().cpu().numpy()),
                  "Prediction": ("b-", preds[:, :3, 3].detach().cpu().numpy())}
        fig, ax = _new_figure((6, 6), title)
        for label, (style, xyz) in tracks.items():
            ax.plot(xyz[:, 0], xyz[:, 2], style, label=label)
        ends = np.stack([xyz[:, [0, 2]] for _, xyz in tracks.values()], axis=1)  # (N, 2 ends, x | z)
        ax.add_collection(LineCollection(ends, colors="r", alpha=0.5, linewidths=0.5))
        ax.set_xlabel("x [m]")
        ax.set_ylabel("z [m]")
        ax.legend()
        ax.set_title("ATE RMSE: %.3f m, per-dim RMSE: x:%.3f m, y:%.3f m, z:%.3f m" % (rmse, *per_dim), fontsize=10)
        data = {"pred_xyz": tracks["Prediction"][1], "gt_xyz": tracks["Ground Truth"][1], "rmse": np.array(rmse),
                "rmse_per_dim": np.array(per_dim)}
        return {"ate_rmse": rmse}, _write_plot(fig, outpath, "traj_ate", data)


def _rpe_terms(preds: torch.Tensor, target: torch.Tensor, d: int):
    """trajectory_metrics.py:169-179 on (N, 4, 4) poses with N > d: (trans, rot)."""
    pred_rel = torch.linalg.inv(preds[:-d]) @ preds[d:]
    gt_rel = torch.linalg.inv(target[:-d]) @ target[d:]
    err = torch.linalg.inv(gt_rel) @ pred_rel
    trans = torch.linalg.norm(err[:, :3, 3], dim=1)
    tr = torch.sum(torch.diagonal(err[:, :3, :3], dim1=-2, dim2=-1), dim=1)
    return trans, torch.acos(torch.clamp((tr - 1) / 2, -1.0, 1.0))


class RelativePoseError(_TrajectoryMetric):
    """Translational / rotational RPE over frame pairs (i, i+delta)
    (trajectory_metrics.py:136-290); rotation error acos((tr R - 1)/2) in
    degrees in ``compute``."""
    _state = ("trans_errors", "rot_errors")

    def __init__(self, delta: int = 1, detailed: bool = False, **kwargs):
        self.delta = delta
        self.detailed = detailed
        self.reset()

    def reset(self) -> None:
        device = self.trans_errors.device if hasattr(self, "trans_errors") else None
        self.trans_errors = torch.tensor([], dtype=torch.float32, device=device)
        self.rot_errors = torch.tensor([], dtype=torch.float32, device=device)

    def _update_device(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        if preds.shape[1] <= self.delta:
            return
        out = _errors(preds, target, self.delta, ate=False, rpe=True, scale=False)
        self.trans_errors = torch.cat([self.trans_errors, out["rpe_trans"].reshape(-1)])
        self.rot_errors = torch.cat([self.rot_errors, out["rpe_rot"].reshape(-1)])

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        assert preds.shape == target.shape, "Preds and targets must have the same shape"
        assert preds.shape[-2:] == (4, 4), "Poses must be 4x4 matrices"
        if preds.shape[0] <= self.delta:
            return
        if self._device_route(preds, target):
            return self._update_device(preds[None], target[None])
        d = self.delta
        pred_rel = torch.linalg.inv(preds[:-d]) @ preds[d:]
        gt_rel = torch.linalg.inv(target[:-d]) @ target[d:]
        err = torch.linalg.inv(gt_rel) @ pred_rel
        trans = torch.linalg.norm(err[:, :3, 3], dim=1)
        tr = torch.sum(torch.diagonal(err[:, :3, :3], dim1=-2, dim2=-1), dim=1)
        rot = torch.acos(torch.clamp((tr - 1) / 2, -1.0, 1.0))
        self.trans_errors = torch.cat([self.trans_errors, trans.detach().to(self.trans_errors.device)])
        self.rot_errors = torch.cat([self.rot_errors, rot.detach().to(self.rot_errors.device)])

    def sync(self, group=None) -> None:
        self.trans_errors = _cat_across_ranks(self.trans_errors, group)
        self.rot_errors = _cat_across_ranks(self.rot_errors, group)

    def compute(self) -> dict:
        t, r = self.trans_errors, self.rot_errors
        have = len(t) > 0

        def f(fn, x, deg=False):
            if not have:
                return 0.0
            v = fn(x)
            return (torch.rad2deg(v) if deg else v).item()
        out = {"rpe_trans_rmse": f(lambda x: torch.sqrt(torch.mean(x ** 2)), t),
               "rpe_rot_rmse": f(lambda x: torch.sqrt(torch.mean(x ** 2)), r, True)}
        if not self.detailed:
            return out
        for name, fn in (("mean", torch.mean), ("median", torch.median), ("std", torch.std), ("min", torch.min),
                         ("max", torch.max)):
            out[f"rpe_trans_{name}"] = f(fn, t)
            out[f"rpe_rot_{name}"] = f(fn, r, True)
        return {k: out[k] for k in ("rpe_trans_rmse", "rpe_trans_mean", "rpe_trans_median", "rpe_trans_std",
                                    "rpe_trans_min", "rpe_trans_max", "rpe_rot_rmse", "rpe_rot_mean",
                                    "rpe_rot_median", "rpe_rot_std", "rpe_rot_min", "rpe_rot_max")}

    def plot(self, preds: torch.Tensor, target: torch.Tensor, title: Optional[str] = None,
             outpath: Optional[str] = None) -> Tuple[dict, str]:
        """trajectory_metrics.py:225-290: the metric of one (N, 4, 4) trajectory and the
        two error curves; ``{outpath}traj_rpe.png`` / ``.npy`` only with ``outpath``.
        Returns ``({"rpe_trans_rmse": float, "rpe_rot_rmse": float (degrees)}, path)``.
        With N <= delta the reference returns None, which its caller cannot unpack; this
        returns ``compute()``'s values for an empty state and draws nothing."""
        _check_poses(preds, target)
        if preds.shape[0] <= self.delta:
            return {"rpe_trans_rmse": 0.0, "rpe_rot_rmse": 0.0}, f"{outpath}traj_rpe.png"
        if _kernel_inputs(preds, target):
            out = _errors(preds[None], target[None], self.delta, ate=False, rpe=True, scale=False)
            trans, rot = out["rpe_trans"][0], out["rpe_rot"][0]
        else:
            trans, rot = _rpe_terms(preds, target, self.delta)
        result = {"rpe_trans_rmse": torch.sqrt(torch.mean(trans ** 2)).item(),
                  "rpe_rot_rmse": torch.rad2deg(torch.sqrt(torch.mean(rot ** 2))).item()}
        steps = range(len(trans))
        trans_np, rot_np = trans.detach().cpu().numpy(), torch.rad2deg(rot).detach().cpu().numpy()
        fig = _curve_figure(title, "Trans RMSE: %.3f m, Rot RMSE: %.3f deg" % tuple(result.values()), steps,
                            [(trans_np, "b", "Translation [m]", "Translational Error [m]"),
                             (rot_np, "r", "Rotation [deg]", "Rotational Error [deg]")])
        data = {"steps": steps, "trans_error": trans_np, "rot_error": rot_np,
                "trans_rmse": np.array(result["rpe_trans_rmse"]), "rot_rmse": np.array(result["rpe_rot_rmse"])}
        return result, _write_plot(fig, outpath, "traj_rpe", data)


def _scale_factors(preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """trajectory_metrics.py:318-325: per-frame LSE scale g.p / max(p.p, 1e-8) of the
    translations, the first frame (always the origin) left out."""
    pred_t, gt_t = preds[1:, :3, 3], target[1:, :3, 3]
    return (gt_t * pred_t).sum(dim=-1) / pred_t.pow(2).sum(dim=-1).clamp_min(1e-8)


class ScaleConsistency(_TrajectoryMetric):
    """Variance of the per-frame scale factors between a predicted and a GT trajectory,
    averaged over the trajectories seen (trajectory_metrics.py:293-394).  ``compute``
    returns ``{"scale_var": 0-dim tensor}`` (the float 0.0 on empty state), as the
    reference does."""
    _state = ("var_sum", "count")

    def __init__(self, **kwargs):
        self.reset()

    def reset(self) -> None:
        device = self.var_sum.device if hasattr(self, "var_sum") else None
        self.var_sum = torch.tensor(0.0, device=device)
        self.count = torch.tensor(0, device=device)

    def _update_device(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        out = _errors(preds, target, ate=False, rpe=False, scale=True)
        self.var_sum = self.var_sum + out["scale_factor"].var(dim=-1, unbiased=False).sum()
        self.count = self.count + preds.shape[0]

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        _check_poses(preds, target)
        if self._device_route(preds, target):
            return self._update_device(preds[None], target[None])
        scale_var = _scale_factors(preds, target).var(dim=-1, unbiased=False)
        self.var_sum = self.var_sum + scale_var.detach().to(self.var_sum.device)
        self.count = self.count + 1

    def sync(self, group=None) -> None:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.var_sum, group=group)
            dist.all_reduce(self.count, group=group)

    def compute(self) -> dict:
        return {"scale_var": self.var_sum / self.count if self.count > 0 else 0.0}

    def plot(self, preds: torch.Tensor, target: torch.Tensor, title: Optional[str] = None,
             outpath: Optional[str] = None) -> Tuple[dict, str]:
        """trajectory_metrics.py:340-394: the variance of one (N, 4, 4) trajectory's scale
        factors and their curve; ``{outpath}traj_scale_cons.png`` / ``.npy`` only with
        ``outpath``.  Returns ``({"scale_var": 0-dim tensor}, path)``."""
        _check_poses(preds, target)
        if _kernel_inputs(preds, target):
            factors = _errors(preds[None], target[None], ate=False, rpe=False, scale=True)["scale_factor"][0]
        else:
            factors = _scale_factors(preds, target)
        scale_var = factors.var(dim=-1, unbiased=False)
        steps = range(1, len(factors) + 1)  # frame 0 has no factor
        factors_np = factors.detach().cpu().numpy()
        fig = _curve_figure(title, "Scale Variance: %.3f" % float(scale_var), steps,
                            [(factors_np, "b", "Scale Factor", "Per-frame Scale Factors")])
        data = {"steps": steps, "scale_factors": factors_np, "scale_var": scale_var.detach().cpu().numpy()}
        return {"scale_var": scale_var}, _write_plot(fig, outpath, "traj_scale_cons", data)


def poses_c2w_from_predictions(pose_enc: torch.Tensor, extrinsics: torch.Tensor, image_hw,
                               device: Optional[torch.device] = None):
    """The pose half of training_metrics.py:233-260 (prepare_data_for_metrics):
    pose encodings (B,S,9) and GT w2c extrinsics (B,S,3,4) -> 4x4 c2w (B,S,4,4)."""
    B, S = extrinsics.shape[:2]
    pred_extr, _ = pose_encoding_to_extri_intri(pose_enc.float(), image_size_hw=image_hw)
    pred = closed_form_inverse_se3(pred_extr.reshape(B * S, 3, 4)).reshape(B, S, 4, 4)
    gt = closed_form_inverse_se3(extrinsics.float().reshape(B * S, 3, 4)).reshape(B, S, 4, 4)
    if device is not None:
        pred, gt = pred.to(device), gt.to(device)
    return pred, gt
