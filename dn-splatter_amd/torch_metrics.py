"""The reference's evaluation scores in plain PyTorch, any device and dtype: ``DepthMetrics.forward`` (dn_splatter/metrics.py:130-149),
``NormalMetrics.forward`` (:171-183), ``mean_angular_error`` (:59-74) and the mse -> psnr formula of torchmetrics'
``PeakSignalNoiseRatio(data_range=1.0)``, restated operation by operation — the yardstick of ``metrics.hip`` (tests/test_gpu_metrics.py
runs it in float64) and what ``tools/eval_metrics_time.py`` times as "the reference's path".  tests/test_metrics_reference.py holds the
first three to vectors the reference's own code produced; the psnr formula is torchmetrics' as published and is NOT pinned (torchmetrics
was not at hand).  LPIPS (a network with downloaded weights) is left to the reference.

``eval_sums`` returns the numerators and integer counts ``dnsplat_eval_metrics`` exposes, before any division.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

# include/dnsplat.h DNSPLAT_METRIC_*: the order of the kernel's `metrics` output
METRIC_INDEX = {"rgb_mse": 0, "rgb_psnr": 1, "depth_abs_rel": 2, "depth_sq_rel": 3, "depth_rmse": 4, "depth_rmse_log": 5, "depth_a1": 6,
                "depth_a2": 7, "depth_a3": 8, "normal_mae": 9, "normal_rsme": 10, "normal_mean_err": 11, "normal_med_err": 12}
METRIC_COUNT, METRIC_COUNTS, METRIC_SUMS = 16, 8, 8
RGB_KEYS = ("rgb_mse", "rgb_psnr")
DEPTH_KEYS = ("depth_abs_rel", "depth_sq_rel", "depth_rmse", "depth_rmse_log", "depth_a1", "depth_a2", "depth_a3")
NORMAL_KEYS = ("normal_mae", "normal_rsme", "normal_mean_err", "normal_med_err")     # "rsme": the reference's spelling (dn_model.py:913)


def _tolerance(tolerance: float, like: Tensor) -> Tensor:
    """``gt > self.tolerance`` on a float32 image compares in float32 (0.1f > 0.1 is false); the tolerance is rounded there first, so
    that a float64 evaluation of float32 images masks the same pixels."""
    return torch.tensor(tolerance, dtype=torch.float32).to(dtype=like.dtype, device=like.device)


def depth_metrics(pred: Tensor, gt: Tensor, tolerance: float = 0.1) -> Tuple[Tensor, ...]:
    """DepthMetrics.forward: (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3)."""
    mask = gt > _tolerance(tolerance, gt)

    thresh = torch.max((gt[mask] / pred[mask]), (pred[mask] / gt[mask]))
    a1 = (thresh < 1.25).to(gt.dtype).mean()
    a2 = (thresh < 1.25**2).to(gt.dtype).mean()
    a3 = (thresh < 1.25**3).to(gt.dtype).mean()
    rmse = (gt[mask] - pred[mask]) ** 2
    rmse = torch.sqrt(rmse.mean())

    rmse_log = (torch.log(gt[mask]) - torch.log(pred[mask])) ** 2
    rmse_log = torch.sqrt(rmse_log).nanmean()                  # sqrt of the square: a mean ABSOLUTE log difference, as the reference has it

    abs_rel = torch.abs(gt - pred)[mask] / gt[mask]
    abs_rel = abs_rel.mean()
    sq_rel = (gt - pred)[mask] ** 2 / gt[mask]
    sq_rel = sq_rel.mean()
    return (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3)


def mean_angular_error(pred: Tensor, gt: Tensor) -> Tensor:
    """[B,C,H,W] x 2 -> [B,H,W]: the angle between the vectors as they are (no normalisation, no 2 x - 1)."""
    dot_products = torch.sum(gt * pred, dim=1)
    dot_products = torch.clamp(dot_products, -1.0, 1.0)
    return torch.acos(dot_products)


def normal_metrics(pred: Tensor, gt: Tensor) -> Tuple[Tensor, ...]:
    """NormalMetrics.forward on [B,C,H,W]: (mae, rmse, mean_err, med_err).  ``torch.median`` is the LOWER median and nan if any is."""
    b, c, _, _ = gt.shape
    mae = mean_angular_error(pred, gt).mean()
    rmse = torch.sqrt(torch.mean(torch.square(gt - pred), dim=[1, 2, 3])).mean()
    mean_err = torch.mean(torch.abs(gt - pred), dim=[1, 2, 3]).mean()
    med_err = torch.median(torch.abs(gt.reshape(b, c, -1) - pred.reshape(b, c, -1))).mean()
    return mae, rmse, mean_err, med_err


def mse(gt: Tensor, pred: Tensor) -> Tensor:
    return torch.mean((gt - pred) ** 2)


def psnr(gt: Tensor, pred: Tensor, data_range: float = 1.0) -> Tensor:
    """torchmetrics' PeakSignalNoiseRatio(data_range): 10 log10(data_range^2 / mse) over all elements (unpinned, see the module text)."""
    return 10.0 * torch.log10(data_range ** 2 / mse(gt, pred))


def eval_sums(rgb: Optional[Tensor] = None, gt_rgb: Optional[Tensor] = None, depth: Optional[Tensor] = None,
              gt_depth: Optional[Tensor] = None, normal: Optional[Tensor] = None, gt_normal: Optional[Tensor] = None,
              tolerance: float = 0.1) -> Tuple[Tensor, Tensor]:
    """(sums [8] in the images' dtype, counts int64 [8]) in the order of DNSPLAT_METRIC_SUM_* / DNSPLAT_METRIC_N_*: what the metrics
    above divide.  rgb [H,W,3]; depth any shape; normal [H,W,3] (the channels last)."""
    like = next(t for t in (rgb, depth, normal) if t is not None)
    sums = torch.zeros(METRIC_SUMS, dtype=like.dtype, device=like.device)
    counts = torch.zeros(METRIC_COUNTS, dtype=torch.int64, device=like.device)
    if rgb is not None:
        sums[0] = ((gt_rgb - rgb) ** 2).sum()
    if depth is not None:
        mask = gt_depth > _tolerance(tolerance, gt_depth)
        g, p = gt_depth[mask], depth[mask]
        thresh = torch.max(g / p, p / g)
        log_term = torch.sqrt((torch.log(g) - torch.log(p)) ** 2)
        kept = ~torch.isnan(log_term)
        sums[1] = ((g - p) ** 2).sum()
        sums[2] = (torch.abs(g - p) / g).sum()
        sums[3] = ((g - p) ** 2 / g).sum()
        sums[4] = log_term[kept].sum()
        counts[0] = mask.sum()
        counts[1], counts[2], counts[3] = (thresh < 1.25).sum(), (thresh < 1.25**2).sum(), (thresh < 1.25**3).sum()
        counts[4] = kept.sum()
    if normal is not None:
        diff = torch.abs(gt_normal - normal)
        sums[5] = mean_angular_error(normal.movedim(-1, 0)[None], gt_normal.movedim(-1, 0)[None]).sum()
        sums[6] = (diff ** 2).sum()
        sums[7] = diff.sum()
        counts[5] = torch.isnan(diff).sum()
    return sums, counts


def _frame(t: Tensor) -> Tensor:
    return t[0, ...] if t.dim() == 4 else t


def image_metrics(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], depth_tolerance: float = 0.1, ssim=None) -> Dict[str, float]:
    """The scalar half of ``DNSplatterModel.get_image_metrics_and_images`` (dn_model.py:824-918) as the reference executes it: the
    modules above on the [1,C,H,W] views, every result read back with its own ``.item()``.  ``ssim``: a callable for ``rgb_ssim`` (the
    model's ``self.ssim``), or None to leave that key out; ``rgb_lpips`` is not computed.  The resize branches are not restated."""
    gt_rgb = batch["image"].to(outputs["rgb"].device)
    predicted_rgb = _frame(outputs["rgb"])
    predicted_normal = _frame(outputs["normal"]) if "normal" in outputs else None
    mask = None
    if "mask" in batch:
        # :849-852 multiplies the [1,C,H,W] views by the mask as it comes, which broadcasts only for an [H,W] mask; here the mask is
        # taken per pixel, [H,W] or [H,W,1]
        mask = batch["mask"].to(gt_rgb.device).reshape(gt_rgb.shape[0], gt_rgb.shape[1], 1)
        gt_rgb = gt_rgb * mask
        predicted_rgb = predicted_rgb * mask
    gt_rgb = torch.moveaxis(gt_rgb, -1, 0)[None, ...]
    predicted_rgb = torch.moveaxis(predicted_rgb, -1, 0)[None, ...]
    out = {"rgb_mse": float(mse(gt_rgb, predicted_rgb).item()), "rgb_psnr": float(psnr(gt_rgb, predicted_rgb).item())}
    if ssim is not None:
        out["rgb_ssim"] = float(ssim(gt_rgb, predicted_rgb))
    predicted_depth = outputs["depth"]
    if "sensor_depth" in batch:
        gt_depth = batch["sensor_depth"].to(predicted_depth.device)
        if predicted_depth.shape[:2] != gt_depth.shape[:2]:
            raise ValueError(f"depth {tuple(predicted_depth.shape)} and sensor_depth {tuple(gt_depth.shape)} differ in size")
        gt_depth = gt_depth.to(predicted_depth.dtype)             # :874 `.to(torch.float32)`: the rendered depth's dtype
        if mask is not None:
            gt_depth = gt_depth * mask
            predicted_depth = predicted_depth * mask
        res = depth_metrics(predicted_depth.permute(2, 0, 1), gt_depth.permute(2, 0, 1), depth_tolerance)
        out.update({k: float(v.item()) for k, v in zip(DEPTH_KEYS, res)})
    if "normal" in batch:
        gt_normal = batch["normal"].to(predicted_normal.device)
        if gt_normal.shape != predicted_normal.shape:
            raise ValueError(f"normal {tuple(predicted_normal.shape)} and batch normal {tuple(gt_normal.shape)} differ in size")
        res = normal_metrics(predicted_normal.permute(2, 0, 1).unsqueeze(0), gt_normal.permute(2, 0, 1).unsqueeze(0))
        out.update({k: float(v.item()) for k, v in zip(NORMAL_KEYS, res)})
    return out

