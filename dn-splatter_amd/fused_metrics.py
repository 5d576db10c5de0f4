"""The evaluation scores of dn-splatter on HIP: what ``DNSplatterModel.get_image_metrics_and_images`` (dn_model.py:809-926) computes
with ``DepthMetrics``, ``NormalMetrics`` and ``PeakSignalNoiseRatio`` (dn_splatter/metrics.py) — about twenty boolean-mask gathers, a
sort-based ``torch.median`` and fourteen ``.item()`` reads per image — as ONE ``dnsplat_eval_metrics`` call (``metrics.hip``) whose
sixteen floats are read back with one copy.  ``torch_metrics`` is the PyTorch restatement the kernel is tested against.

``image_metrics`` / ``image_metrics_dict`` take the model's ``outputs`` and ``batch``; ``DepthMetrics``, ``NormalMetrics`` and ``PSNR`` are
drop-ins for the three modules the model holds (``install.install_metrics`` swaps them).  SSIM is ``fused_loss.ssim_hip``; LPIPS stays
with the reference.  There is no CPU path: tensors that are not on the GPU raise.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._ops import _eval_metrics_args, _need_gpu, _stream
from .fused_loss import AGS_LAYOUT, ssim_hip
from .torch_metrics import DEPTH_KEYS, METRIC_COUNT, METRIC_COUNTS, METRIC_INDEX, METRIC_SUMS, NORMAL_KEYS, RGB_KEYS

SUM_RGB_SQ = 0          # include/dnsplat.h DNSPLAT_METRIC_SUM_RGB_SQ


def eval_metrics(width: int, height: int, *, rgb: Optional[Tensor] = None, gt_rgb: Optional[Tensor] = None, depth: Optional[Tensor] = None,
                 gt_depth: Optional[Tensor] = None, depth_tolerance: float = 0.1, normal: Optional[Tensor] = None,
                 gt_normal: Optional[Tensor] = None, normal_layout: str = "hwc", with_sums: bool = False):
    """``dnsplat_eval_metrics`` on contiguous float32 device tensors holding ``width x height`` pixels: (metrics float32 [16], counts
    int64 [8]) and, ``with_sums``, the numerators float64 [8] — device tensors, nothing is read on the host.  The layouts are the
    caller's word: rgb 3 floats per pixel, depth one, normal three in ``normal_layout``."""
    pairs = [("rgb", rgb, gt_rgb, 3), ("depth", depth, gt_depth, 1), ("normal", normal, gt_normal, 3)]
    dev = None
    for name, a, b, per in pairs:
        if (a is None) != (b is None):
            raise ValueError(f"{name}: prediction and ground truth are given together or not at all")
        if a is None:
            continue
        for t in (a, b):
            _need_gpu(t, name)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != per * width * height:
                raise ValueError(f"{name}: contiguous float32 of {per} x {width} x {height} values, got {t.dtype} {tuple(t.shape)}")
        dev = a.device
    if dev is None:
        raise ValueError("eval_metrics: none of the three image pairs is given")
    L = _lib.lib()
    scratch = torch.empty(L.dnsplat_eval_metrics_scratch_bytes(width, height) // 8, dtype=torch.float64, device=dev)
    metrics = torch.empty(METRIC_COUNT, dtype=torch.float32, device=dev)
    counts = torch.empty(METRIC_COUNTS, dtype=torch.int64, device=dev)
    sums = torch.empty(METRIC_SUMS, dtype=torch.float64, device=dev) if with_sums else None
    a = _eval_metrics_args(width, height, rgb, gt_rgb, depth, gt_depth, float(depth_tolerance), normal, gt_normal,
                           AGS_LAYOUT[normal_layout], scratch, metrics, counts, sums)
    _lib.run("dnsplat_eval_metrics", L.dnsplat_eval_metrics, ctypes.byref(a), _stream())
    return (metrics, counts, sums) if with_sums else (metrics, counts)


def _frame(t: Tensor) -> Tensor:
    return t[0, ...] if t.dim() == 4 else t


def _f32(t: Tensor, name: str) -> Tensor:
    """Contiguous float32 on the GPU; any other dtype is cast, as the reference casts the sensor depth (dn_model.py:874)."""
    _need_gpu(t, name)
    return t.to(torch.float32).contiguous()


def _metrics_of(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], depth_tolerance: float, ssim: bool):
    """(metrics [16] on the device, the keys present, rgb_ssim or None)."""
    pred_rgb = _frame(outputs["rgb"])
    dev = pred_rgb.device
    gt_rgb = batch["image"].to(dev)
    if gt_rgb.shape != pred_rgb.shape or pred_rgb.dim() != 3 or pred_rgb.shape[2] != 3:
        raise ValueError(f"rgb {tuple(pred_rgb.shape)} and image {tuple(gt_rgb.shape)}: two [H,W,3] images of one size")
    H, W = pred_rgb.shape[0], pred_rgb.shape[1]
    mask = batch["mask"].to(dev).reshape(H, W, 1) if "mask" in batch else None
    kw, keys = {}, list(RGB_KEYS)                                       # every shape is looked at before anything is computed
    if "sensor_depth" in batch:
        pred_depth = outputs["depth"]
        gt_depth = batch["sensor_depth"].to(dev)
        if tuple(pred_depth.shape[:2]) != (H, W) or tuple(gt_depth.shape[:2]) != (H, W) or pred_depth.numel() != H * W \
                or gt_depth.numel() != H * W:
            raise ValueError(f"depth {tuple(pred_depth.shape)} and sensor_depth {tuple(gt_depth.shape)} must have the size of the rgb "
                             f"image {(H, W)}: the reference's resize branch (dn_model.py:869-872) is not supported")
        keys += DEPTH_KEYS
    if "normal" in batch:
        pred_normal = _frame(outputs["normal"])
        gt_normal = batch["normal"].to(dev)
        if gt_normal.shape != pred_normal.shape or tuple(pred_normal.shape) != (H, W, 3):
            raise ValueError(f"normal {tuple(pred_normal.shape)} and batch normal {tuple(gt_normal.shape)} must be [H,W,3] images of the "
                             f"rgb image's size {(H, W)}: the reference's resize branch (dn_model.py:900-905) is not supported")
        kw.update(normal=_f32(pred_normal, "normal"), gt_normal=_f32(gt_normal, "batch normal"), normal_layout="hwc")
        keys += NORMAL_KEYS
    if "sensor_depth" in batch:
        gt_depth = gt_depth.to(torch.float32)                           # :874
        if mask is not None:                                            # :876-878
            gt_depth, pred_depth = gt_depth.reshape(H, W, 1) * mask, pred_depth.reshape(H, W, 1) * mask
        kw.update(depth=_f32(pred_depth, "depth"), gt_depth=_f32(gt_depth, "sensor_depth"), depth_tolerance=depth_tolerance)
    if mask is not None:                                                # dn_model.py:849-852
        gt_rgb, pred_rgb = gt_rgb * mask, pred_rgb * mask
    kw.update(rgb=_f32(pred_rgb, "rgb"), gt_rgb=_f32(gt_rgb, "image"))
    metrics, _ = eval_metrics(W, H, **kw)
    return metrics, keys, (ssim_hip(kw["rgb"], kw["gt_rgb"]).detach() if ssim else None)


@torch.no_grad()
def image_metrics(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], *, depth_tolerance: float = 0.1, ssim: bool = True) -> Dict[str, Tensor]:
    """The scalars of ``get_image_metrics_and_images`` as 0-dim device tensors under the reference's keys: ``rgb_mse``, ``rgb_psnr``,
    ``rgb_ssim`` (``ssim``; from ``ssim_hip``); with ``batch["sensor_depth"]`` ``depth_abs_rel``, ``depth_sq_rel``, ``depth_rmse``,
    ``depth_rmse_log``, ``depth_a1`` .. ``depth_a3``; with ``batch["normal"]`` ``normal_mae``, ``normal_rsme``, ``normal_mean_err``,
    ``normal_med_err``.  A ``batch["mask"]`` ([H,W] or [H,W,1]) multiplies prediction and ground truth of rgb and depth first.  Images of
    any dtype are cast to float32 (the kernel's format) after the mask.  Images of different sizes raise ``ValueError`` (the reference
    resizes).  Nothing is read on the host.  ``rgb_lpips`` is not computed."""
    metrics, keys, s = _metrics_of(outputs, batch, depth_tolerance, ssim)
    out = {k: metrics[METRIC_INDEX[k]] for k in keys}
    if s is not None:
        out["rgb_ssim"] = s
    return out


@torch.no_grad()
def image_metrics_dict(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], *, depth_tolerance: float = 0.1, ssim: bool = True) -> Dict[str, float]:
    """``image_metrics`` as floats after ONE device-to-host copy."""
    metrics, keys, s = _metrics_of(outputs, batch, depth_tolerance, ssim)
    if s is not None:
        metrics = torch.cat([metrics, s.reshape(1).to(metrics.dtype)])
    host = metrics.tolist()
    out = {k: host[METRIC_INDEX[k]] for k in keys}
    if s is not None:
        out["rgb_ssim"] = host[-1]
    return out


def _same_memory_order(a: Tensor, b: Tensor) -> bool:
    """Both tensors are permutations of a dense block with the same strides: an elementwise mean may read them as they lie."""
    if a.stride() != b.stride():
        return False
    order = sorted(range(a.dim()), key=lambda i: (-a.stride(i), i))
    return a.permute(order).is_contiguous()


def _flat_pair(a: Tensor, b: Tensor, what: str) -> Tuple[Tensor, Tensor]:
    if a.shape != b.shape:
        raise ValueError(f"{what}: two tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    _need_gpu(a, what); _need_gpu(b, what)
    a, b = a.detach().to(torch.float32), b.detach().to(torch.float32)
    if not _same_memory_order(a, b):
        a, b = a.contiguous(), b.contiguous()
    return a, b


def _as_dense(t: Tensor) -> Tensor:
    """The dense block under a permuted view, as a contiguous tensor without a copy."""
    order = sorted(range(t.dim()), key=lambda i: (-t.stride(i), i))
    return t.permute(order)


class DepthMetrics(torch.nn.Module):
    """Drop-in for ``dn_splatter.metrics.DepthMetrics``: ``forward(pred, gt) -> (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3)``, 0-dim
    device tensors.  Any two tensors of one shape: the masked means are elementwise."""

    def __init__(self, tolerance: float = 0.1, **kwargs):
        super().__init__()
        self.tolerance = tolerance

    @torch.no_grad()
    def forward(self, pred: Tensor, gt: Tensor):
        pred, gt = _flat_pair(pred, gt, "DepthMetrics")
        n = pred.numel()
        if n < 1 or n > 2 ** 31 - 1:
            raise ValueError(f"DepthMetrics: 1 .. 2^31 - 1 values, got {n}")
        m, _ = eval_metrics(n, 1, depth=_as_dense(pred), gt_depth=_as_dense(gt), depth_tolerance=self.tolerance)
        return tuple(m[METRIC_INDEX[k]] for k in DEPTH_KEYS)


class NormalMetrics(torch.nn.Module):
    """Drop-in for ``dn_splatter.metrics.NormalMetrics``: ``forward(pred, gt) -> (mae, rmse, mean_err, med_err)`` on [1,3,H,W].  The
    permuted view of an [H,W,3] image (how the model calls it, dn_model.py:907-910) is recognised by its strides and read in place; any
    other layout is copied to [3,H,W].  ``B > 1`` or ``C != 3`` raise ``NotImplementedError``."""

    def __init__(self, **kwargs):
        super().__init__()

    @torch.no_grad()
    def forward(self, pred: Tensor, gt: Tensor):
        if pred.dim() != 4 or pred.shape != gt.shape:
            raise ValueError(f"NormalMetrics: two [B,C,H,W] tensors of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
        if pred.shape[0] != 1 or pred.shape[1] != 3:
            raise NotImplementedError(f"dnsplat NormalMetrics covers one image of three channels, got {tuple(pred.shape)}")
        _need_gpu(pred, "NormalMetrics"); _need_gpu(gt, "NormalMetrics")
        H, W = pred.shape[2], pred.shape[3]
        p, g = pred[0].detach().to(torch.float32), gt[0].detach().to(torch.float32)
        hwc = all(t.permute(1, 2, 0).is_contiguous() for t in (p, g))
        if hwc:
            p, g = p.permute(1, 2, 0), g.permute(1, 2, 0)
        else:
            p, g = p.contiguous(), g.contiguous()
        m, _ = eval_metrics(W, H, normal=p, gt_normal=g, normal_layout="hwc" if hwc else "chw")
        return tuple(m[METRIC_INDEX[k]] for k in NORMAL_KEYS)


class PSNR(torch.nn.Module):
    """Drop-in for the model's ``self.psnr`` (torchmetrics' ``PeakSignalNoiseRatio(data_range=1.0)``), called as ``psnr(gt, pred)``:
    10 log10(1 / mse) over all elements of two tensors of any one shape, a 0-dim device tensor.  The kernel reads three values per
    pixel; an element count that is no multiple of 3 gets one or two zero differences appended (a copy), which add nothing to the sum of
    squares, and the mean is taken over the true count."""

    def __init__(self, data_range: float = 1.0, **kwargs):
        super().__init__()
        if data_range != 1.0:
            raise NotImplementedError("dnsplat PSNR: data_range=1.0 (the module dn-splatter constructs)")

    @torch.no_grad()
    def forward(self, gt: Tensor, pred: Tensor) -> Tensor:
        gt, pred = _flat_pair(gt, pred, "PSNR")
        n = gt.numel()
        if n < 1 or (n + 2) // 3 > 2 ** 31 - 1:
            raise ValueError(f"PSNR: 1 .. 3 (2^31 - 1) values, got {n}")
        g, p = _as_dense(gt).reshape(-1), _as_dense(pred).reshape(-1)
        if n % 3 == 0:
            m, _ = eval_metrics(n // 3, 1, rgb=p, gt_rgb=g)
            return m[METRIC_INDEX["rgb_psnr"]]
        pad = 3 - n % 3
        g, p = torch.nn.functional.pad(g, (0, pad)), torch.nn.functional.pad(p, (0, pad))
        _, _, sums = eval_metrics((n + pad) // 3, 1, rgb=p, gt_rgb=g, with_sums=True)
        return (10.0 * torch.log10(1.0 / (sums[SUM_RGB_SQ] / n))).to(torch.float32)      # the kernel's last step, in double as there
