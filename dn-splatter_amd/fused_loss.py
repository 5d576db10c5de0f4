"""dn-splatter's per-pixel training loss as two HIP launches.

``dn_loss_fused`` computes what ``torch_losses.dn_loss`` (the PyTorch restatement of
``DNSplatterModel.get_loss_dict``, dn_splatter/dn_model.py:614-729) computes — same value, same gradients w.r.t. the
rendered rgb / depth / normal images — but with the cotangents produced directly by ``dnsplat_dn_loss`` instead of by
autograd over ~120 torch kernels; the per-Gaussian min-scale term is one more launch (``dnsplat_scale_reg``).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import DnLossArgs
from ._ops import _f32c, _ptr, _stream


def depth_counts(gt_depth: Tensor, depth_tolerance: float = 0.1) -> Tensor:
    """Normalisers of the two EdgeAwareLogL1 means (losses.py:216-222): valid pixels in columns < W-1 and rows < H-1.
    Depends on the batch only — compute once per image, no host sync."""
    valid = gt_depth.reshape(gt_depth.shape[0], gt_depth.shape[1]) > depth_tolerance
    return torch.stack([valid[:, :-1].sum(), valid[:-1, :].sum()]).to(torch.float32)


class _DnLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, depth, normal, image, gt_depth, gt_normal, counts, ssim_lambda, depth_lambda, depth_tolerance):
        rgb = _f32c(rgb, "rgb"); depth = _f32c(depth, "depth"); normal = _f32c(normal, "normal")
        image = _f32c(image, "image")
        H, W = rgb.shape[0], rgb.shape[1]
        dev = rgb.device
        f32 = dict(dtype=torch.float32, device=dev)
        maps = torch.empty(9 * H * W + 512, **f32)      # dnsplat_dn_loss_args.maps: scratch
        v_rgb = torch.empty(H, W, 3, **f32)
        v_depth = torch.empty(depth.shape, **f32)
        v_normal = torch.empty(H, W, 3, **f32)
        sums = torch.empty(8, **f32)
        a = DnLossArgs()
        a.width, a.height = W, H
        a.rgb, a.depth, a.normal, a.gt_rgb = _ptr(rgb), _ptr(depth), _ptr(normal), _ptr(image)
        if gt_depth is not None:
            gt_depth = _f32c(gt_depth, "mono_depth")
            counts = _f32c(counts, "depth_counts")
        if gt_normal is not None:
            gt_normal = _f32c(gt_normal, "normal gt")
        a.gt_depth, a.gt_normal, a.depth_counts = _ptr(gt_depth), _ptr(gt_normal), _ptr(counts)
        a.ssim_lambda, a.depth_weight, a.depth_tolerance = ssim_lambda, 1.0 + depth_lambda, depth_tolerance
        a.maps, a.v_rgb, a.v_depth, a.v_normal, a.sums = _ptr(maps), _ptr(v_rgb), _ptr(v_depth), _ptr(v_normal), _ptr(sums)
        _lib.run("dnsplat_dn_loss", _lib.lib().dnsplat_dn_loss, ctypes.byref(a), _stream())
        P = float(W * H)
        M = 3.0 * (W - 10) * (H - 10)
        loss = (1 - ssim_lambda) * sums[1] / (3 * P) + ssim_lambda * (1 - sums[0] / M)
        if gt_depth is not None:
            loss = loss + (1.0 + depth_lambda) * (sums[2] / counts[0] + sums[3] / counts[1])
        if gt_normal is not None:
            loss = loss + sums[4] / (3 * P) + sums[5] / (3.0 * H * (W - 1)) + sums[6] / (3.0 * (H - 1) * W)
        ctx.save_for_backward(v_rgb, v_depth, v_normal)
        return loss

    @staticmethod
    def backward(ctx, g):
        v_rgb, v_depth, v_normal = ctx.saved_tensors
        return (v_rgb * g, v_depth * g, v_normal * g) + (None,) * 7


class _SsimFn(torch.autograd.Function):
    """Mean SSIM of two [H,W,3] images and its gradient w.r.t. the first in two launches (``dnsplat_ssim``)."""

    @staticmethod
    def forward(ctx, x, y):
        x = _f32c(x, "ssim x"); y = _f32c(y, "ssim y")
        if x.dim() != 3 or x.shape[2] != 3 or x.shape != y.shape:
            raise ValueError(f"dnsplat_ssim takes two [H,W,3] images, got {tuple(x.shape)} and {tuple(y.shape)}")
        H, W = x.shape[0], x.shape[1]
        f32 = dict(dtype=torch.float32, device=x.device)
        maps = torch.empty(9 * H * W + 512, **f32)
        need_grad = ctx.needs_input_grad[0]
        v_x = torch.empty(H, W, 3, **f32) if need_grad else None
        sums = torch.empty(8, **f32)
        _lib.run("dnsplat_ssim", _lib.lib().dnsplat_ssim, W, H, _ptr(x), _ptr(y), _ptr(maps), _ptr(v_x), _ptr(sums), _stream())
        if need_grad:
            ctx.save_for_backward(v_x)
        return sums[0] / (3.0 * (W - 10) * (H - 10))

    @staticmethod
    def backward(ctx, g):
        (v_x,) = ctx.saved_tensors
        return v_x * g, None


def ssim_hip(pred: Tensor, gt: Tensor) -> Tensor:
    """Mean SSIM of two [H,W,3] images in [0,1] (pytorch_msssim's definition: 11-tap Gaussian, sigma 1.5, valid padding), with the
    gradient w.r.t. ``pred`` — ``torch_losses.ssim`` as ONE autograd node on two HIP launches instead of ~45 torch kernels."""
    return _SsimFn.apply(pred, gt)


class SSIM(torch.nn.Module):
    """Stand-in for the module ``DNSplatterModel`` holds as ``self.ssim`` — ``torchmetrics.StructuralSimilarityIndexMeasure(
    data_range=1.0, kernel_size=11)`` (dn_model.py:180; nerfstudio's own splatfacto holds ``pytorch_msssim.SSIM(data_range=1.0,
    size_average=True, channel=3)``: the same 11-tap sigma-1.5 Gaussian statistics averaged over the (W-10)(H-10) windows that do
    not touch the border — torchmetrics reflect-pads and crops the padded rim away again) — as the inherited RGB term calls it:
    ``1 - self.ssim(gt.permute(2,0,1)[None], pred.permute(2,0,1)[None])`` (two [1,3,H,W] views of [H,W,3] images: read in place;
    any other layout is copied), and as the evaluation calls it (dn_model.py:855).  SSIM is symmetric in its arguments; the gradient
    goes to whichever of the two requires it (the rendered image).  Not restated: recent torchmetrics clamp the two variances at 0
    before the ratio (a decision on fp32 rounding noise of a quantity that is >= 0 in exact arithmetic).  ``install_ssim(model)``
    puts it in place."""

    def __init__(self, data_range: float = 1.0, size_average: bool = True, channel: int = 3, kernel_size: int = 11, sigma: float = 1.5):
        super().__init__()
        if data_range != 1.0 or not size_average or channel != 3 or kernel_size != 11 or sigma != 1.5:
            raise NotImplementedError("dnsplat SSIM: data_range=1.0, kernel_size=11, sigma=1.5, mean over 3 channels (the module "
                                      "dn-splatter / splatfacto construct)")

    def forward(self, X: Tensor, Y: Tensor) -> Tensor:
        if X.dim() != 4 or X.shape[0] != 1 or X.shape[1] != 3 or X.shape != Y.shape:
            raise NotImplementedError(f"dnsplat SSIM takes two [1,3,H,W] images, got {tuple(X.shape)} and {tuple(Y.shape)}")
        x, y = X[0].permute(1, 2, 0), Y[0].permute(1, 2, 0)
        if y.requires_grad and not x.requires_grad:
            x, y = y, x
        elif y.requires_grad:
            raise NotImplementedError("dnsplat SSIM differentiates one argument (the rendered image)")
        return _SsimFn.apply(x, y)


class _EdgeAwareLogL1Fn(torch.autograd.Function):
    """EdgeAwareLogL1 ("scalar", losses.py:187-224): value and gradient w.r.t. the prediction in one pass (``dnsplat_edge_aware_logl1``)."""

    @staticmethod
    def forward(ctx, pred, gt, rgb, mask):
        shape = pred.shape
        H, W = shape[0], shape[1]
        p2 = _f32c(pred.reshape(H, W), "pred"); g2 = _f32c(gt.reshape(H, W).float(), "gt"); rgb = _f32c(rgb, "rgb")
        if rgb.shape != (H, W, 3):
            raise ValueError(f"EdgeAwareLogL1: rgb must be [H,W,3] for a [{H},{W}] depth, got {tuple(rgb.shape)}")
        m = None
        if mask is not None:
            if mask.dtype != torch.bool or mask.numel() != H * W:
                raise ValueError("EdgeAwareLogL1: mask must be a bool tensor of the depth's shape")
            m = mask.reshape(H, W).contiguous()
        f32 = dict(dtype=torch.float32, device=p2.device)
        need = ctx.needs_input_grad[0]
        v_x = torch.empty(H, W, **f32) if need else None
        v_y = torch.empty(H, W, **f32) if need else None
        scratch = torch.empty(512, **f32)
        sums = torch.empty(8, **f32)
        _lib.run("dnsplat_edge_aware_logl1", _lib.lib().dnsplat_edge_aware_logl1, W, H, _ptr(p2), _ptr(g2), _ptr(rgb), _ptr(m),
                 _ptr(v_x), _ptr(v_y), _ptr(scratch), _ptr(sums), _stream())
        if need:
            ctx.save_for_backward(v_x, v_y, sums)
            ctx.shape = shape
        return sums[0] / sums[2] + sums[1] / sums[3]        # mean over the counted pixels of each term (an empty mask: nan, as the reference)

    @staticmethod
    def backward(ctx, g):
        v_x, v_y, sums = ctx.saved_tensors
        return (v_x * (g / sums[2]) + v_y * (g / sums[3])).reshape(ctx.shape), None, None, None


class EdgeAwareLogL1(torch.nn.Module):
    """Drop-in for ``dn_splatter.losses.EdgeAwareLogL1(implementation="scalar")`` (losses.py:187-224) as
    ``DNRegularization.get_depth_loss`` calls it (regularization_strategy.py:162-170): ``loss(pred_depth, gt_depth, gt_img, valid_mask)``
    with [H,W,1] depths, an [H,W,3] image and an [H,W,1] bool mask (or None).  One launch instead of ~20 torch kernels and — what costs
    more in an eager step — instead of the two boolean-mask gathers ``loss_x[mask]``, whose data-dependent size is a host
    synchronisation each.  Gradient w.r.t. ``pred`` only (the reference differentiates nothing else here)."""

    def __init__(self, implementation: str = "scalar", **kwargs):
        super().__init__()
        if implementation != "scalar":
            raise NotImplementedError('dnsplat EdgeAwareLogL1: implementation="scalar" (what DNRegularization constructs)')
        self.implementation = implementation

    def forward(self, pred: Tensor, gt: Tensor, rgb: Tensor, mask: Optional[Tensor]) -> Tensor:
        if pred.dim() not in (2, 3) or (pred.dim() == 3 and pred.shape[2] != 1):
            raise NotImplementedError(f"dnsplat EdgeAwareLogL1 takes one [H,W,1] depth image, got {tuple(pred.shape)}")
        if gt.requires_grad or rgb.requires_grad:
            raise NotImplementedError("dnsplat EdgeAwareLogL1 differentiates the prediction only")
        return _EdgeAwareLogL1Fn.apply(pred, gt, rgb, mask)


class _PearsonFn(torch.autograd.Function):
    """``w_whole`` x the whole-frame Pearson loss + ``w_box`` x the MEAN of the box losses, value and gradient w.r.t. the prediction in
    one entry-point call (``dnsplat_pearson_depth``).  ``rows`` / ``cols``: int64 device tensors of box origins, passed on unread."""

    @staticmethod
    def forward(ctx, pred, gt, mask, rows, cols, box, whole, w_whole, w_box):
        shape = pred.shape
        n_boxes = 0 if rows is None else int(rows.numel())
        if n_boxes:
            H, W = shape[0], shape[1]
            if pred.numel() != H * W:
                raise NotImplementedError(f"dnsplat Pearson boxes take one [H,W] or [H,W,1] depth image, got {tuple(shape)}")
            if rows.dtype != torch.int64 or cols.dtype != torch.int64 or cols.numel() != n_boxes or rows.device != pred.device \
                    or cols.device != pred.device:
                raise ValueError("dnsplat Pearson boxes: rows and cols are int64 tensors of one length on the prediction's device")
            rows, cols = rows.contiguous(), cols.contiguous()
        else:
            H, W = 1, pred.numel()                       # the whole-frame region is a set of pixels: any shape
            rows = cols = None
        if gt.numel() != pred.numel():
            raise ValueError(f"dnsplat Pearson: prediction {tuple(shape)} and ground truth {tuple(gt.shape)} differ in size")
        p2 = _f32c(pred.reshape(H, W), "pred"); g2 = _f32c(gt.reshape(H, W).float(), "gt")
        m = None
        if mask is not None:
            if mask.dtype != torch.bool or mask.numel() != H * W:
                raise ValueError("dnsplat Pearson: mask must be a bool tensor of the depth's shape")
            m = mask.reshape(H, W).contiguous()
        dev = p2.device
        need = ctx.needs_input_grad[0]
        v = torch.empty(H, W, dtype=torch.float32, device=dev) if need else None
        L = _lib.lib()
        scratch = torch.empty(L.dnsplat_pearson_scratch_bytes(n_boxes) // 8, dtype=torch.float64, device=dev)
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        w_each = w_box / n_boxes if n_boxes else 0.0                      # the division by n_corr stays on this side
        _lib.run("dnsplat_pearson_depth", L.dnsplat_pearson_depth, W, H, _ptr(p2), _ptr(g2), _ptr(m), 1 if whole else 0, n_boxes,
                 int(box), _ptr(rows), _ptr(cols), w_whole if whole else 0.0, w_each, _ptr(v), _ptr(scratch), _ptr(sums), _stream())
        if need:
            ctx.save_for_backward(v)
            ctx.shape = shape
        if whole and n_boxes:
            return w_whole * sums[0] + w_each * sums[1]
        return w_whole * sums[0] if whole else w_each * sums[1]

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return ((v * g).reshape(ctx.shape),) + (None,) * 8


def _no_gt_grad(gt: Tensor, what: str) -> None:
    if gt.requires_grad:
        raise NotImplementedError(f"dnsplat {what} differentiates the prediction only")


def pearson_depth(pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """``PearsonDepthLoss()(pred, gt)`` (losses.py:428-450) over all pixels of ``pred`` (any shape), or — with a bool ``mask`` of the
    same shape — ``PearsonDepthLoss()(pred[mask], gt[mask])`` without the gather; gradient w.r.t. ``pred``.  Fewer than two pixels: nan."""
    _no_gt_grad(gt, "pearson_depth")
    return _PearsonFn.apply(pred, gt, mask, None, None, 0, True, 1.0, 0.0)


def local_pearson_depth(pred: Tensor, gt: Tensor, rows: Tensor, cols: Tensor, box: int = 128) -> Tensor:
    """The loop of ``LocalPearsonDepthLoss.forward`` (losses.py:480-485) for given origins: the mean over the boxes
    ``[rows[i] : rows[i] + box, cols[i] : cols[i] + box]`` of the Pearson loss; ``pred`` [H,W] or [H,W,1], ``rows`` / ``cols`` int64 tensors
    on its device, never read on the host.  No boxes: nan (the reference's 0 / 0) without a launch."""
    _no_gt_grad(gt, "local_pearson_depth")
    if rows.numel() == 0:
        return pred.new_full((), float("nan"), dtype=torch.float32)
    return _PearsonFn.apply(pred, gt, None, rows, cols, box, False, 0.0, 1.0)


def pearson_depth_combined(pred: Tensor, gt: Tensor, rows: Tensor, cols: Tensor, box: int = 128, w_whole: float = 1.0,
                           w_box: float = 1.0, mask: Optional[Tensor] = None) -> Tensor:
    """``w_whole * pearson_depth(pred, gt, mask) + w_box * local_pearson_depth(pred, gt, rows, cols, box)`` in one entry-point call
    (the ``PearsonDepth`` branch of ``DNRegularization.get_depth_loss``: w_box = depth_lambda)."""
    _no_gt_grad(gt, "pearson_depth_combined")
    if rows.numel() == 0:
        return w_whole * pearson_depth(pred, gt, mask) + float("nan")
    return _PearsonFn.apply(pred, gt, mask, rows, cols, box, True, float(w_whole), float(w_box))


def draw_pearson_boxes(depth_pred: Tensor, box_p: int = 128, p_corr: float = 0.5):
    """The box origins as ``LocalPearsonDepthLoss.forward`` draws them (losses.py:469-476): the same two ``torch.randint`` calls in
    the same order with the same bounds, on the prediction's device — a seeded run consumes the generator as the reference does."""
    H, W = depth_pred.shape[0], depth_pred.shape[1]
    count = int(p_corr * (H // box_p) * (W // box_p))
    dev = depth_pred.device
    rows = torch.randint(0, H - box_p, size=(count,), device=dev)        # first draw: top rows, upper bound exclusive
    cols = torch.randint(0, W - box_p, size=(count,), device=dev)        # second draw: left columns
    return rows, cols


class PearsonDepthLoss(torch.nn.Module):
    """Drop-in for ``dn_splatter.losses.PearsonDepthLoss`` (losses.py:428-450): ``forward(depth_pred, depth_gt)`` on tensors of any one
    shape.  Gradient w.r.t. the prediction only.  The reference's ``assert not torch.any(torch.isnan(co))`` is a host synchronisation
    and is not reproduced: a nan comes back as a nan."""

    def forward(self, depth_pred: Tensor, depth_gt: Tensor) -> Tensor:
        return pearson_depth(depth_pred, depth_gt)


class LocalPearsonDepthLoss(torch.nn.Module):
    """Drop-in for ``dn_splatter.losses.LocalPearsonDepthLoss`` (losses.py:454-485): ``forward(depth_pred, depth_gt, box_p=128,
    p_corr=0.5)`` on an [H,W] or [H,W,1] depth image.  The origins are drawn as the reference draws them (``draw_pearson_boxes``) and
    handed to the kernels as device data: no slice by a device scalar, so no host synchronisation.  ``n_corr == 0`` returns nan (the reference's 0 / 0) without a launch; a frame that is no larger than a box raises
    what ``torch.randint`` raises.  The per-box ``assert not torch.any(torch.isnan(co))`` of the reference is a host synchronisation
    and is not reproduced.  Gradient w.r.t. the prediction only."""

    def __init__(self):
        super().__init__()
        self.pearson_depth_loss = PearsonDepthLoss()

    def forward(self, depth_pred: Tensor, depth_gt: Tensor, box_p: int = 128, p_corr: float = 0.5) -> Tensor:
        rows, cols = draw_pearson_boxes(depth_pred, box_p, p_corr)
        return local_pearson_depth(depth_pred, depth_gt, rows, cols, box_p)


class _TVLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred):
        pred = _f32c(pred, "pred")
        H, W, C = pred.shape
        f32 = dict(dtype=torch.float32, device=pred.device)
        v = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        scratch = torch.empty(512, **f32)
        sums = torch.empty(8, **f32)
        _lib.run("dnsplat_tv_loss", _lib.lib().dnsplat_tv_loss, W, H, C, _ptr(pred), _ptr(v), _ptr(scratch), _ptr(sums), _stream())
        if v is not None:
            ctx.save_for_backward(v)
        return sums[0] / float(C * H * (W - 1)) + sums[1] / float(C * (H - 1) * W)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return v * g


class TVLoss(torch.nn.Module):
    """Drop-in for ``dn_splatter.losses.TVLoss`` (losses.py:279-295) on one [H,W,C] image, as ``NormalLoss(Smooth)`` applies it to
    the rendered normals (regularization_strategy.py:188-193): one launch for value and gradient instead of ~14 torch kernels."""

    def forward(self, pred: Tensor) -> Tensor:
        if pred.dim() != 3:
            raise NotImplementedError(f"dnsplat TVLoss takes one [H,W,C] image, got {tuple(pred.shape)}")
        return _TVLossFn.apply(pred)


class _ScaleRegFn(torch.autograd.Function):
    """mean_g min_k exp(scales[g, k]) (regularization_strategy.py:195-199) and its gradient in one launch (dnsplat_scale_reg)."""

    @staticmethod
    def forward(ctx, scales):
        scales = _f32c(scales, "scales")
        N = scales.shape[0]
        v = torch.empty_like(scales)
        total = torch.zeros((), dtype=torch.float32, device=scales.device)
        _lib.run("dnsplat_scale_reg", _lib.lib().dnsplat_scale_reg, N, _ptr(scales), 1.0 / max(N, 1), _ptr(v), _ptr(total), _stream())
        if N == 0:
            total.fill_(float("nan"))                       # the mean of no Gaussians: nan, as the reference's .mean()
        ctx.save_for_backward(v)
        return total

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return v * g


def scale_reg(scales: Tensor) -> Tensor:
    """``torch.min(torch.exp(scales), dim=1, keepdim=True)[0].mean()`` (``DNRegularization.get_scale_loss``,
    regularization_strategy.py:195-199) and its gradient in one launch (``dnsplat_scale_reg``) instead of ten kernels over [N,3]."""
    return _ScaleRegFn.apply(scales)


AGS_LAYOUT = {"chw": 0, "hwc": 1}      # dnsplat.h DNSPLAT_AGS_LAYOUT_*: [3,H,W] in [-1, 1] | [H,W,3] in [0, 1]


class _AgsNormalFn(torch.autograd.Function):
    """``weight`` x (mean over the selected elements of |surf - gt| + mean over all elements of |pred - gt|) on the normals in [-1, 1]
    — ``AGSMeshRegularization.get_normal_loss`` (regularization_strategy.py:292-321) — and the selection, in one entry-point call
    (``dnsplat_ags_normal_loss``: two launches).  ``mode`` 0 selects the elements off the dilated edge map of ``gt``, 1 the pixels whose
    surface normal is within 0.1 rad of it.  The number selected stays on the device: the value and the gradient divide by it there."""

    @staticmethod
    def forward(ctx, surf, gt, pred, mode, weight, layout):
        surf = _f32c(surf, "surf_normal"); gt = _f32c(gt, "gt_normal"); pred = _f32c(pred, "pred_normal")
        if surf.dim() != 3 or surf.shape[0 if layout == "chw" else 2] != 3 or gt.shape != surf.shape or pred.shape != surf.shape:
            raise ValueError(f"dnsplat AGS normal loss takes three {'[3,H,W]' if layout == 'chw' else '[H,W,3]'} images, got "
                             f"{tuple(surf.shape)}, {tuple(gt.shape)}, {tuple(pred.shape)}")
        H, W = (surf.shape[1], surf.shape[2]) if layout == "chw" else (surf.shape[0], surf.shape[1])
        dev = surf.device
        need_s, _, need_p = ctx.needs_input_grad[:3]
        v_surf = torch.empty_like(surf) if need_s else None
        v_pred = torch.empty_like(pred) if need_p else None
        selection = torch.empty((3, H, W) if mode == 0 else (H, W), dtype=torch.bool, device=dev)
        L = _lib.lib()
        scratch = torch.empty(L.dnsplat_ags_normal_scratch_bytes(W, H) // 8, dtype=torch.float64, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.run("dnsplat_ags_normal_loss", L.dnsplat_ags_normal_loss, W, H, _ptr(surf), _ptr(gt), _ptr(pred), AGS_LAYOUT[layout], int(mode),
                 float(weight), _ptr(v_surf), _ptr(v_pred), _ptr(selection), _ptr(scratch), _ptr(sums), _ptr(count), _stream())
        ctx.save_for_backward(v_surf, v_pred, count)
        ctx.mark_non_differentiable(selection)
        # 0 / 0 = nan for an empty selection, as the reference's mean of nothing; times a weight of 0 it stays nan
        loss = (sums[0] / count[0]) * weight + (sums[1] / (3.0 * H * W)) * weight
        return loss.float(), selection

    @staticmethod
    def backward(ctx, g, _g_selection):
        v_surf, v_pred, count = ctx.saved_tensors
        g_surf = g_pred = None
        if v_surf is not None:
            # nothing selected: v_surf is all zeros and autograd's gather backward leaves zeros too (not 0 x inf)
            n = count[0]
            g_surf = v_surf * torch.where(n > 0, g / n.clamp(min=1), torch.zeros_like(g))
        if v_pred is not None:
            g_pred = v_pred * g
        return g_surf, None, g_pred, None, None, None


def ags_normal_loss(surf_normal: Tensor, gt_normal: Tensor, pred_normal: Tensor, step: int, normal_lambda: float = 0.1,
                    normal_mask_steps: int = 15000, layout: str = "chw", return_selection: bool = False):
    """``AGSMeshRegularization.get_normal_loss(step, surf_normal, gt_normal, pred_normal)`` (regularization_strategy.py:292-321;
    ``torch_losses.ags_normal_loss``) without the six conv2d calls of ``find_edges`` and without the two boolean-mask gathers, whose
    data-dependent size is a host synchronisation each: two launches, nothing read on the host, so the call can be captured.
    ``layout`` "chw": [3,H,W] tensors in [-1, 1], what the method receives; "hwc": the [H,W,3] images in [0, 1] that ``outputs`` /
    ``batch`` hold (``2 x - 1`` is applied by the kernel, the gradients are w.r.t. the images).  ``step <= 7000`` takes the same path
    with weight 0: the value is 0 with zero gradients — or nan where nothing is selected, as in the reference.  Gradients w.r.t.
    ``surf_normal`` and ``pred_normal``.  ``return_selection``: also the filter map, bool — before ``normal_mask_steps`` [3,H,W], the
    elements OFF the dilated edge map; from then on [H,W], the confident pixels."""
    if gt_normal.requires_grad:
        raise NotImplementedError("dnsplat ags_normal_loss differentiates the surface and the predicted normal only")
    if layout not in AGS_LAYOUT:
        raise ValueError(f'layout must be "chw" or "hwc", got {layout!r}')
    weight = float(normal_lambda) if step > 7000 else 0.0                               # regularization_strategy.py:296
    loss, selection = _AgsNormalFn.apply(surf_normal, gt_normal, pred_normal, 0 if step < normal_mask_steps else 1, weight, layout)
    return (loss, selection) if return_selection else loss


def ags_mesh_loss_fused(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], scales: Tensor, step: int,
                        confidence: Optional[Tensor] = None, ssim_lambda: float = 0.2, depth_lambda: float = 0.2,
                        depth_tolerance: float = 0.1, normal_lambda: float = 0.1, normal_mask_steps: int = 15000) -> Tensor:
    """main_loss of ``DNSplatterModel.get_loss_dict`` for regularization_strategy == "ags-mesh" (dn_model.py:614-729 with
    ``AGSMeshRegularization.get_loss``, regularization_strategy.py:233-255; ``torch_losses.ags_mesh_loss``), the counterpart of
    ``dn_loss_fused``: the rgb term (``dnsplat_dn_loss`` without depth and normal ground truth), ``depth_lambda`` x EdgeAwareLogL1 under
    the mask ``torch_losses.ags_depth_mask`` (``dnsplat_edge_aware_logl1``), the filtered normal term on the [H,W,3] images as they are
    (``dnsplat_ags_normal_loss``) and the scale term.  ``confidence``: the confidence MAP, by default ``1 - batch["confidence"] /
    255`` (:646).  A ``batch["mask"]`` multiplies the rendered depth, the predicted normal and the two ground truths (:648-660; not the
    surface normal).  Nothing is read on the host: forward and backward can be captured into a HIP graph."""
    from .torch_losses import ags_depth_mask

    rgb = outputs["rgb"]
    if not rgb.is_cuda:
        raise _lib.DnsplatError("ags_mesh_loss_fused runs on the GPU: the tensors are on " + str(rgb.device))
    depth, normal, surf_normal = outputs["depth"], outputs["normal"], outputs["surface_normal"]
    gt_depth, gt_normal = batch["mono_depth"], batch["normal"]
    if confidence is None:
        confidence = 1 - batch["confidence"] / 255.0
    if "mask" in batch:
        mask = batch["mask"]
        depth, normal, gt_depth, gt_normal = depth * mask, normal * mask, gt_depth * mask, gt_normal * mask
    gt_img = batch["image"].clamp(min=10 / 255.0)                                        # dn_model.py:633
    loss = _DnLossFn.apply(rgb, depth.detach(), normal.detach(), batch["image"], None, None, None, ssim_lambda, depth_lambda, depth_tolerance)
    depth_mask = ags_depth_mask(gt_depth, confidence, step, depth_tolerance).reshape(depth.shape[0], depth.shape[1])
    loss = loss + _EdgeAwareLogL1Fn.apply(depth, gt_depth, gt_img, depth_mask) * depth_lambda
    loss = loss + ags_normal_loss(surf_normal, gt_normal, normal, step, normal_lambda, normal_mask_steps, layout="hwc")
    return loss + _ScaleRegFn.apply(scales)


def dn_loss_fused(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], scales: Tensor, ssim_lambda: float = 0.2,
                  depth_lambda: float = 0.2, depth_tolerance: float = 0.1, counts: Optional[Tensor] = None) -> Tensor:
    """Drop-in for ``torch_losses.dn_loss`` (mono depth + mono normal supervision).  A ``batch["mask"]`` multiplies the rendered
    depth, both normals and the two ground truths before the launch, as dn_model.py:646-659 does (the rgb term does not see it);
    ``counts`` (``depth_counts``) are then those of the MASKED ground-truth depth."""
    depth, normal = outputs["depth"], outputs["normal"]
    gt_depth, gt_normal = batch.get("mono_depth"), batch.get("normal")
    if "mask" in batch:                                                             # dn_model.py:646-659
        mask = batch["mask"]
        depth, normal = depth * mask, normal * mask
        gt_depth = gt_depth * mask if gt_depth is not None else None
        gt_normal = gt_normal * mask if gt_normal is not None else None
    if gt_depth is not None and counts is None:
        counts = depth_counts(gt_depth, depth_tolerance)
    per_pixel = _DnLossFn.apply(outputs["rgb"], depth, normal, batch["image"], gt_depth, gt_normal, counts, ssim_lambda,
                                depth_lambda, depth_tolerance)
    return per_pixel + _ScaleRegFn.apply(scales)                                      # regularization_strategy.py:195-199
