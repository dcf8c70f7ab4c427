"""Chamfer / accuracy / completion (eval/reconstruction_metrics.py:11-84 of the
reference) and the rigid ICP that precedes them (training_metrics.py:343-364),
restated without ``torchmetrics`` and ``pytorch3d``, neither of which is in
this image.

Both of the reference's PyTorch3D calls -- ``knn_points(K=1)`` and
``iterative_closest_point`` -- are nearest-neighbour searches; here they run
through the exact brute-force HIP kernel ``vggt_nn1`` (csrc/nn.hip).  There is
no CPU path: clouds on the CPU raise ``RuntimeError`` like every other binding.
The PyTorch3D semantics restated here (squared L2 for ``norm=2``, the ICP
iteration, its stopping rule) are listed in SPEC_ASSUMPTIONS.md.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from .. import _native
from .trajectory_metrics import _cat_across_ranks


def _host_has_zero(lengths) -> bool:
    if lengths is None:
        return False
    if isinstance(lengths, torch.Tensor):
        return lengths.device.type == "cpu" and lengths.numel() > 0 and bool((lengths == 0).any())
    return any(int(v) == 0 for v in lengths)


def nearest_neighbors(q: torch.Tensor, r: torch.Tensor, norm: int = 2, q_lengths=None, r_lengths=None,
                      return_idx: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Exact 1-nearest-neighbour of every row of ``q`` among the rows of ``r``
    (``knn_points(q, r, K=1, norm=norm)``): ``(dists, idx)``.

    ``q``: (Nq, 3) and ``r``: (Nr, 3), or (B, Nq, 3) and (B, Nr, 3) padded, with
    ``q_lengths`` / ``r_lengths`` (B,) giving the valid rows.  ``dists`` is the
    SQUARED Euclidean distance for ``norm=2`` and the L1 distance for
    ``norm=1``; ``idx`` int64 (None with ``return_idx=False``).  Ties take the
    smallest index; padded query rows get ``(0, -1)``; a query with no
    selectable reference gets ``(+inf, -1)``.  Runs on the current stream.
    """
    for t in (q, r):
        if not t.is_cuda:
            raise RuntimeError(f"nearest_neighbors: tensor on {t.device}; the MI355X hot path runs on HIP devices "
                               f"only")
    if norm not in (1, 2):
        raise ValueError(f"nearest_neighbors: norm must be 1 or 2, got {norm}")
    single = q.dim() == 2
    if single:
        if r.dim() != 2:
            raise ValueError("nearest_neighbors: q is (N, 3), so r must be (M, 3)")
        q, r = q[None], r[None]
    if q.dim() != 3 or r.dim() != 3 or q.shape[-1] != 3 or r.shape[-1] != 3 or q.shape[0] != r.shape[0]:
        raise ValueError(f"nearest_neighbors: expected (B, N, 3) clouds, got {tuple(q.shape)} and {tuple(r.shape)}")
    if r.shape[1] == 0 or _host_has_zero(r_lengths):
        raise ValueError("nearest_neighbors: empty reference cloud")
    dists, idx = _native.nn1(q.detach().float(), r.detach().float(), norm, q_lengths, r_lengths, return_idx)
    if single:
        return dists[0], (idx[0] if idx is not None else None)
    return dists, idx


class ChamferDistanceMetrics:
    """Chamfer distance, accuracy (pred -> GT) and completion (GT -> pred),
    reconstruction_metrics.py:11-84.  ``norm=2`` accumulates SQUARED distances,
    as knn_points returns them, and ``rmse=True`` squares them once more before
    the mean and the root: the reference does, so this does.  ``compute()``
    returns the reference's keys and types: 0-dim tensors under ``rmse=True``
    (floats ``0.0`` on empty state), Python floats otherwise."""

    def __init__(self, norm: int = 2, max_dist: Optional[float] = None, rmse: bool = True, **kwargs):
        self.norm = norm
        self.max_dist = max_dist
        self.rmse = rmse
        self.reset()

    def reset(self) -> None:
        self.pred_to_gt = torch.tensor([], dtype=torch.float32)
        self.gt_to_pred = torch.tensor([], dtype=torch.float32)

    def distances(self, preds: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The two clamped distance vectors (pred -> GT (N_pred,), GT -> pred
        (N_gt,)) that ``update`` accumulates and the reference's ``plot``
        histograms."""
        assert preds.ndim == 2 and target.ndim == 2
        p2g, _ = nearest_neighbors(preds, target, norm=self.norm, return_idx=False)
        g2p, _ = nearest_neighbors(target, preds, norm=self.norm, return_idx=False)
        if self.max_dist is not None:
            p2g = torch.clamp(p2g, max=self.max_dist)
            g2p = torch.clamp(g2p, max=self.max_dist)
        return p2g, g2p

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        p2g, g2p = self.distances(preds, target)
        self.pred_to_gt = torch.cat([self.pred_to_gt, p2g.flatten().detach().to(self.pred_to_gt.device)])
        self.gt_to_pred = torch.cat([self.gt_to_pred, g2p.flatten().detach().to(self.gt_to_pred.device)])

    def sync(self, group=None) -> None:
        self.pred_to_gt = _cat_across_ranks(self.pred_to_gt, group)
        self.gt_to_pred = _cat_across_ranks(self.gt_to_pred, group)

    def compute(self) -> dict:
        if self.rmse:
            acc_rmse = torch.sqrt((self.pred_to_gt ** 2).mean()) if len(self.pred_to_gt) > 0 else 0.0
            # the reference tests pred_to_gt's length here too (reconstruction_metrics.py:65)
            comp_rmse = torch.sqrt((self.gt_to_pred ** 2).mean()) if len(self.pred_to_gt) > 0 else 0.0
            return {"chamfer_distance_rmse": 0.5 * acc_rmse + 0.5 * comp_rmse, "accuracy_rmse": acc_rmse,
                    "completion_rmse": comp_rmse}
        acc = self.pred_to_gt.mean().item() if len(self.pred_to_gt) > 0 else 0.0
        comp = self.gt_to_pred.mean().item() if len(self.gt_to_pred) > 0 else 0.0
        return {"chamfer_distance": 0.5 * acc + 0.5 * comp, "accuracy": acc, "completion": comp}

    def to(self, target):
        """Move the accumulated distances to a device, or to the device of a tensor (as
        the reference's ``metric.to(gt_points[0])``); returns self.  With the state on
        the clouds' device ``update`` copies nothing to the host."""
        device = target.device if isinstance(target, torch.Tensor) else torch.device(target)
        self.pred_to_gt, self.gt_to_pred = self.pred_to_gt.to(device), self.gt_to_pred.to(device)
        return self

    def plot(self, preds: torch.Tensor, target: torch.Tensor, title: Optional[str] = None,
             outpath: Optional[str] = None) -> Tuple[dict, str]:
        """reconstruction_metrics.py:86-153: the metric of one pair of clouds ((N_pred, 3),
        (N_gt, 3)) and the histogram of both distance vectors;
        ``{outpath}rec_chamfer_distribution.png`` / ``.npy`` are written only with
        ``outpath``.  Returns ``(dict, path)`` with ``compute()``'s keys and types: 0-dim
        tensors under ``rmse=True``, Python floats otherwise."""
        import numpy as np
        from .trajectory_metrics import _new_figure, _write_plot

        def reduce(d):  # one direction's figure of merit
            if len(d) == 0:
                return 0.0
            return torch.sqrt((d ** 2).mean()) if self.rmse else d.mean().item()
        dists = dict(zip(("pred_to_gt", "gt_to_pred"), self.distances(preds, target)))
        acc, comp = reduce(dists["pred_to_gt"]), reduce(dists["gt_to_pred"])
        names = ("chamfer_distance", "accuracy", "completion")
        values = (0.5 * acc + 0.5 * comp, acc, comp)
        result = {n + ("_rmse" if self.rmse else ""): v for n, v in zip(names, values)}
        host = {k: d.cpu().numpy() for k, d in dists.items()}
        fig, ax = _new_figure((6, 6), title)
        for key, label in (("pred_to_gt", "Pred\u2192GT"), ("gt_to_pred", "GT\u2192Pred")):
            ax.hist(host[key], bins=100, alpha=0.5, label=label)
        ax.set_xlabel("Distance")
        ax.set_ylabel("Count")
        ax.legend()
        unit = " RMSE" if self.rmse else ""
        ax.set_title(", ".join("%s%s: %.3f m" % (what, unit, float(v))
                               for what, v in zip(("Chamfer", "Accuracy", "Completion"), values)), fontsize=10)
        data = {"dists_" + k: v for k, v in host.items()}
        data.update((k, np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v))
                    for k, v in zip(("chamfer", "acc", "comp"), values))
        return result, _write_plot(fig, outpath, "rec_chamfer_distribution", data)

    __call__ = update


@dataclass
class ICPSolution:
    """Result of ``iterative_closest_point``: ``Xt = s * X @ R + T`` (row
    vectors).  ``Xt`` is a list of (N_i, 3) tensors when lists were given, else
    the padded (B, N, 3) tensor."""
    converged: bool
    rmse: torch.Tensor
    Xt: Union[torch.Tensor, List[torch.Tensor]]
    R: torch.Tensor
    T: torch.Tensor
    s: torch.Tensor
    iterations: int


def _pad(clouds: Sequence[torch.Tensor]):
    B = len(clouds)
    if B == 0:
        raise ValueError("iterative_closest_point: empty list of clouds")
    dev = clouds[0].device
    lens = [int(c.shape[0]) for c in clouds]
    out = torch.zeros(B, max(max(lens), 1), 3, device=dev, dtype=torch.float32)
    for i, c in enumerate(clouds):
        if c.dim() != 2 or c.shape[1] != 3:
            raise ValueError("iterative_closest_point: clouds are (N_i, 3)")
        out[i, : lens[i]] = c.detach().to(device=dev, dtype=torch.float32)
    return out, torch.tensor(lens, dtype=torch.int64, device=dev)


def solve_similarity(stats: torch.Tensor, sumsq_x: Optional[torch.Tensor], estimate_scale: bool,
                     allow_reflection: bool):
    """(R, T, s) of PyTorch3D's corresponding_points_alignment from the sums of
    ``vggt_nn1_pair_stats`` (B, 17) -- count, sum x, sum y, sum x^T y -- and,
    for the scale, sum |x|^2 (B,): centred cross-covariance, 3x3 SVD,
    R = U diag(1, 1, det(U V^T)) V^T, s = tr(S E) / var(x), T = y_mean -
    s x_mean R.  fp64 on whatever device ``stats`` is on; a batch item with no
    pairs gets the identity."""
    st = stats.double()
    B = st.shape[0]
    n = st[:, 0].clamp_min(1.0)
    xm, ym = st[:, 1:4] / n[:, None], st[:, 4:7] / n[:, None]
    cov = st[:, 7:16].reshape(B, 3, 3) / n[:, None, None] - xm[:, :, None] * ym[:, None, :]
    U, S, Vh = torch.linalg.svd(cov)
    E = torch.eye(3, dtype=torch.float64, device=st.device).repeat(B, 1, 1)
    if not allow_reflection:
        E[:, 2, 2] = torch.sign(torch.linalg.det(U @ Vh))
    R = U @ E @ Vh
    if estimate_scale:
        var = (sumsq_x.double() / n - (xm * xm).sum(1)).clamp_min(1e-9)
        s = (torch.diagonal(E, dim1=1, dim2=2) * S).sum(1) / var
    else:
        s = torch.ones(B, dtype=torch.float64, device=st.device)
    T = ym - s[:, None] * torch.einsum("bi,bij->bj", xm, R)
    empty = st[:, 0] < 1
    if bool(empty.any()):
        R[empty] = torch.eye(3, dtype=torch.float64, device=st.device)
        T[empty] = 0.0
        s[empty] = 1.0
    return R, T, s


def _apply(X: torch.Tensor, R: torch.Tensor, T: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """s * X @ R + T through vggt_sim3_points (which computes M (s p) + t for
    column vectors: M = R^T)."""
    B = X.shape[0]
    M = torch.zeros(B, 4, 4, dtype=torch.float32)
    M[:, :3, :3] = R.transpose(1, 2).float()
    M[:, :3, 3] = T.float()
    M[:, 3, 3] = 1.0
    return _native.sim3_points(X, M.to(X.device), s.float().to(X.device))


def iterative_closest_point(X, Y, max_iterations: int = 100, relative_rmse_thr: float = 1e-6,
                            estimate_scale: bool = False, allow_reflection: bool = False,
                            X_lengths=None, Y_lengths=None) -> ICPSolution:
    """PyTorch3D's ``iterative_closest_point`` restated (SPEC_ASSUMPTIONS.md):
    align ``X`` to ``Y``.  ``X`` / ``Y``: lists of (N_i, 3) / (M_i, 3) clouds (as
    training_metrics.py:344-358 builds them) or padded (B, N, 3) / (B, M, 3)
    tensors with ``X_lengths`` / ``Y_lengths``.

    Each iteration, from ``Xt = X``: nearest neighbours ``Y_nn`` of ``Xt`` in
    ``Y`` (vggt_nn1), the fp64 sums of (X, Y_nn) (vggt_nn1_pair_stats), the
    3x3 solve on the host in fp64 (72 bytes a batch item; the stopping rule
    needs the host every iteration anyway), ``Xt = s X R + T``
    (vggt_sim3_points), ``rmse = sqrt(mean |Xt - Y_nn|^2)`` (pair_stats
    again); stop when ``(prev - rmse) / prev <= relative_rmse_thr`` for every
    batch item (never on the first iteration)."""
    as_list = isinstance(X, (list, tuple))
    if as_list:
        X, X_lengths = _pad(X)
    if isinstance(Y, (list, tuple)):
        Y, Y_lengths = _pad(Y)
    for t in (X, Y):
        if not t.is_cuda:
            raise RuntimeError(f"iterative_closest_point: tensor on {t.device}; the MI355X hot path runs on HIP "
                               f"devices only")
    if X.dim() != 3 or Y.dim() != 3 or X.shape[0] != Y.shape[0] or X.shape[-1] != 3 or Y.shape[-1] != 3:
        raise ValueError("iterative_closest_point: X (B, N, 3) and Y (B, M, 3) with one batch size")
    if Y.shape[1] == 0 or _host_has_zero(Y_lengths):
        raise ValueError("iterative_closest_point: empty target cloud")
    X = X.detach().float().contiguous()
    Y = Y.detach().float().contiguous()
    B, N = X.shape[:2]
    dev = X.device
    xl = _native._len_arg(X_lengths, B, dev, "X_lengths")
    yl = _native._len_arg(Y_lengths, B, dev, "Y_lengths")

    sumsq = None
    if estimate_scale:
        own = torch.arange(N, device=dev, dtype=torch.int64).expand(B, N).contiguous()
        sxx = _native.nn1_pair_stats(X, X, own, xl, xl).cpu()
        sumsq = sxx[:, 7] + sxx[:, 11] + sxx[:, 15]

    Xt = X
    R = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    T = torch.zeros(B, 3, dtype=torch.float64)
    s = torch.ones(B, dtype=torch.float64)
    rmse = torch.zeros(B, dtype=torch.float64)
    prev = None
    converged = False
    iterations = 0
    for it in range(max_iterations):
        _, idx = _native.nn1(Xt, Y, 2, xl, yl, True)
        R, T, s = solve_similarity(_native.nn1_pair_stats(X, Y, idx, xl, yl).cpu(), sumsq, estimate_scale,
                                   allow_reflection)
        Xt = _apply(X, R, T, s)
        res = _native.nn1_pair_stats(Xt, Y, idx, xl, yl).cpu()
        rmse = torch.sqrt((res[:, 16] / res[:, 0].clamp_min(1.0)).clamp_min(0.0))
        iterations = it + 1
        rel = torch.ones(B, dtype=torch.float64) if prev is None else (prev - rmse) / prev
        if bool((rel <= relative_rmse_thr).all()):
            converged = True
            break
        prev = rmse
    if as_list:
        lens = [int(v) for v in xl.cpu()]
        Xt_out = [Xt[i, : lens[i]] for i in range(B)]
    else:
        Xt_out = Xt
    return ICPSolution(converged, rmse.float().to(dev), Xt_out, R.float().to(dev), T.float().to(dev),
                       s.float().to(dev), iterations)
