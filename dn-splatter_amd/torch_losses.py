"""The per-pixel losses of dn-splatter, kept in PyTorch-ROCm (BASELINE.json north star: "the per-pixel
depth/normal losses ... in dn_splatter/losses.py stay in PyTorch-ROCm").

This is the host-side restatement that BASELINE config C5 ("depth + mono-normal loss enabled") times together
with the renderer; nothing here is a kernel of ours.  It follows

* ``DNSplatterModel.get_loss_dict``                      dn_splatter/dn_model.py:614-729
* ``DNRegularization.get_loss`` / depth / normal / scale dn_splatter/regularization_strategy.py:146-199
* ``EdgeAwareLogL1``, ``LogL1``, ``L1``, ``TVLoss``      dn_splatter/losses.py:154-224, 279-295
* ``PearsonDepthLoss``, ``LocalPearsonDepthLoss``        dn_splatter/losses.py:428-485 (depth_loss_type = PearsonDepth)
* ``AGSMeshRegularization`` depth / normal, ``find_edges``, ``mean_angular_error``   dn_splatter/regularization_strategy.py:11-96, 202-327
* the inherited RGB term of nerfstudio's ``SplatfactoModel.get_loss_dict``: ``(1 - l) * L1 + l * (1 - SSIM)`` with
  ``l = ssim_lambda = 0.2``; ``self.ssim`` is, in dn-splatter, torchmetrics' ``StructuralSimilarityIndexMeasure(data_range=1.0,
  kernel_size=11)`` (dn_model.py:180; nerfstudio itself holds pytorch_msssim's SSIM): an 11 x 11 Gaussian window, sigma 1.5, averaged
  over the windows that do not touch the border (pytorch_msssim: valid convolution; torchmetrics: reflect-pad, then crop the rim) —
  neither package is vendored in the reference, so that term is restated from their published definitions.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import Tensor


def _gaussian_window(size: int = 11, sigma: float = 1.5, device=None) -> Tensor:
    x = torch.arange(size, dtype=torch.float32, device=device) - size // 2
    g = torch.exp(-(x ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def ssim(pred: Tensor, gt: Tensor, data_range: float = 1.0) -> Tensor:
    """Mean SSIM of two [H,W,3] images (separable 11-tap Gaussian, valid padding)."""
    x = pred.permute(2, 0, 1)[None]
    y = gt.permute(2, 0, 1)[None]
    C = x.shape[1]
    w = _gaussian_window(device=x.device).to(x.dtype)
    wh = w.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    ww = w.view(1, 1, 1, -1).repeat(C, 1, 1, 1)

    def blur(t):
        return F.conv2d(F.conv2d(t, wh, groups=C), ww, groups=C)

    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu_x, mu_y = blur(x), blur(y)
    sxx = blur(x * x) - mu_x * mu_x
    syy = blur(y * y) - mu_y * mu_y
    sxy = blur(x * y) - mu_x * mu_y
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    s = ((2 * mu_x * mu_y + c1) / (mu_x * mu_x + mu_y * mu_y + c1)) * cs
    return s.mean()


_TOEPLITZ: Dict = {}
SSIM_GEMM_BLOCK = int(os.environ.get("DNSPLAT_SSIM_GEMM_BLOCK", "64"))
SSIM_FAST_IMPL = os.environ.get("DNSPLAT_SSIM_IMPL", "conv")      # what dn_loss(capturable=True) uses: "conv" (ten grouped conv2d calls, the fastest measured) | "gemm" | "stacked"


def _toeplitz(block: int, device, size: int = 11, sigma: float = 1.5) -> Tensor:
    """[block + size - 1, block] banded matrix: column j holds the Gaussian window at rows j .. j + size - 1, so that a block of
    ``block + size - 1`` consecutive samples times it is the VALID 11-tap blur of that block (``block`` outputs)."""
    key = (block, str(device), size, sigma)
    T = _TOEPLITZ.get(key)
    if T is None:
        w = _gaussian_window(size, sigma)
        T = torch.zeros(block + size - 1, block)
        for j in range(block):
            T[j:j + size, j] = w
        T = T.to(device)
        _TOEPLITZ[key] = T
    return T


def _blur_valid_gemm(t: Tensor, block: int = 64, size: int = 11) -> Tensor:
    """Separable 11-tap Gaussian blur (valid padding) of the last two dims of ``t`` [..., H, W] as two block-Toeplitz GEMMs: the
    windows of ``block + 10`` samples at a stride of ``block`` are a view (``unfold``), the taps a [block + 10, block] banded matrix.
    Same sums as conv2d with the separable window, in hipBLASLt's order.  Why not conv2d: MIOpen runs the depthwise 11 x 1 / 1 x 11
    convolutions of a 1600 x 1200 image through general-purpose convolution kernels at ~250-500 us each, thirty of them per step
    (profiles/r06_c5_torch_loss_kernel_stats.txt): 5.5 ms, more than the whole render step."""
    T = _toeplitz(block, t.device, size)

    def along_last(x):
        n = x.shape[-1]
        out = n - size + 1
        nb = -(-out // block)
        need = nb * block + size - 1
        if need > n:
            x = F.pad(x, (0, need - n))
        y = x.unfold(-1, block + size - 1, block) @ T                  # [..., nb, block]
        return y.reshape(*x.shape[:-1], nb * block)[..., :out]

    t = along_last(t)                                                   # along W
    return along_last(t.transpose(-1, -2)).transpose(-1, -2)            # along H


def ssim_stacked(pred: Tensor, gt: Tensor, data_range: float = 1.0) -> Tensor:
    """``ssim`` with the five maps (x, y, x^2, y^2, xy) stacked into ONE [1, 15, H, W] tensor: two grouped conv2d calls (and two in the
    backward) instead of ten (and six)."""
    x = pred.permute(2, 0, 1)
    y = gt.permute(2, 0, 1)
    C = x.shape[0]
    t = torch.cat([x, y, x * x, y * y, x * y], 0)[None]
    w = _gaussian_window(device=x.device)
    wh = w.view(1, 1, -1, 1).repeat(5 * C, 1, 1, 1)
    ww = w.view(1, 1, 1, -1).repeat(5 * C, 1, 1, 1)
    b = F.conv2d(F.conv2d(t, wh, groups=5 * C), ww, groups=5 * C)[0]
    mu_x, mu_y, bxx, byy, bxy = b[:C], b[C:2 * C], b[2 * C:3 * C], b[3 * C:4 * C], b[4 * C:]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    cs = (2 * (bxy - mu_x * mu_y) + c2) / ((bxx - mu_x * mu_x) + (byy - mu_y * mu_y) + c2)
    s = ((2 * mu_x * mu_y + c1) / (mu_x * mu_x + mu_y * mu_y + c1)) * cs
    return s.mean()


def ssim_gemm(pred: Tensor, gt: Tensor, data_range: float = 1.0) -> Tensor:
    """``ssim`` with the five blurs (x, y, x^2, y^2, xy) stacked into one [15, H, W] tensor and run as two GEMMs (see
    ``_blur_valid_gemm``) instead of ten grouped conv2d calls: same value and gradient up to fp32 summation order, 5x fewer kernels."""
    x = pred.permute(2, 0, 1)
    y = gt.permute(2, 0, 1)
    C = x.shape[0]
    b = _blur_valid_gemm(torch.cat([x, y, x * x, y * y, x * y], 0), block=SSIM_GEMM_BLOCK)
    mu_x, mu_y, bxx, byy, bxy = b[:C], b[C:2 * C], b[2 * C:3 * C], b[3 * C:4 * C], b[4 * C:]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    sxx = bxx - mu_x * mu_x
    syy = byy - mu_y * mu_y
    sxy = bxy - mu_x * mu_y
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    s = ((2 * mu_x * mu_y + c1) / (mu_x * mu_x + mu_y * mu_y + c1)) * cs
    return s.mean()


def _dcol(t: Tensor) -> Tensor:
    """t[i, j] - t[i, j+1] for an [H,W,C] image."""
    return t[:, :-1] - t[:, 1:]


def _drow(t: Tensor) -> Tensor:
    """t[i, j] - t[i+1, j]."""
    return t[:-1] - t[1:]


def edge_aware_log_l1(pred: Tensor, gt: Tensor, rgb: Tensor, mask: Optional[Tensor], capturable: bool = False) -> Tensor:
    """Scalar EdgeAwareLogL1 (losses.py:187-224): log(1 + |pred - gt|), down-weighted across image edges by
    exp(-mean_c |colour difference to the right / lower neighbour|), averaged over the masked pixels separately for the
    horizontal and the vertical term.
    ``capturable``: the masked means as sum(term x mask) / sum(mask) instead of the reference's boolean-mask gather
    ``term[mask].mean()`` — the gather's output size is data dependent (a host synchronisation: the step cannot be captured into
    a HIP graph); same value and gradients up to the order of the fp32 sums."""
    err = torch.log(1 + (pred - gt).abs())
    edge_x = torch.exp(-_dcol(rgb).abs().mean(dim=-1, keepdim=True))
    edge_y = torch.exp(-_drow(rgb).abs().mean(dim=-1, keepdim=True))
    term_x = edge_x * err[:, :-1]
    term_y = edge_y * err[:-1]
    if mask is not None and capturable:
        mx, my = mask[:, :-1].to(term_x.dtype), mask[:-1].to(term_y.dtype)
        return (term_x * mx).sum() / mx.sum() + (term_y * my).sum() / my.sum()
    if mask is not None:
        term_x = term_x[mask[:, :-1]]
        term_y = term_y[mask[:-1]]
    return term_x.mean() + term_y.mean()


def tv_loss(pred: Tensor) -> Tensor:
    """TVLoss (losses.py:279-295): mean absolute difference to the right neighbour plus to the lower neighbour."""
    return _dcol(pred).abs().mean() + _drow(pred).abs().mean()


def _standardised(x: Tensor) -> Tensor:
    """x less its mean, over its unbiased standard deviation + 1e-6."""
    d = x - x.mean()
    return d / (d.std() + 1e-6)


def pearson_depth(pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """PearsonDepthLoss (losses.py:428-450): 1 - the mean product of the two arguments, each centred on its mean and divided by its
    unbiased standard deviation + 1e-6.  ``mask``: the loss of ``pred[mask], gt[mask]``, as the other depth branches call it (a
    boolean-mask gather: a host synchronisation).  The reference's assert on a nan correlation is left out."""
    if mask is not None:
        pred, gt = pred[mask], gt[mask]
    return 1 - (_standardised(pred) * _standardised(gt)).mean()


def local_pearson_depth(pred: Tensor, gt: Tensor, rows: Tensor, cols: Tensor, box: int = 128) -> Tensor:
    """The loop of LocalPearsonDepthLoss (losses.py:480-485) for GIVEN box origins (the reference draws them with two
    ``torch.randint`` calls, :475-476): the mean over the boxes of ``pearson_depth`` of the box's pixels.  The origins come to the
    host once (the reference slices with device scalars: four synchronisations per box).  No boxes: 0 / 0 = nan, as the reference."""
    n = int(rows.numel())
    loss = torch.zeros((), dtype=pred.dtype, device=pred.device)
    for r, c in zip(rows.tolist(), cols.tolist()):
        loss = loss + pearson_depth(pred[r:r + box, c:c + box].reshape(-1), gt[r:r + box, c:c + box].reshape(-1))
    return loss / n


def pearson_depth_term(pred_depth: Tensor, gt_depth: Tensor, rows: Tensor, cols: Tensor, box: int = 128, depth_lambda: float = 0.2,
                       depth_tolerance: float = 0.1) -> Tensor:
    """``DNRegularization.get_depth_loss`` for ``depth_loss_type = PearsonDepth`` (regularization_strategy.py:161-186) with the
    origins of the local term given: both terms times the number of valid ground-truth pixels and divided by it again (nan when
    there is none), the local one weighted by depth_lambda, and the sum once more ``+= depth_lambda x`` itself."""
    valid = gt_depth > depth_tolerance
    whole = (pearson_depth(pred_depth, gt_depth.float()) * valid.sum()) / valid.sum()
    local = (local_pearson_depth(pred_depth, gt_depth.float(), rows, cols, box) * valid.sum()) / valid.sum()
    depth_loss = whole + depth_lambda * local
    depth_loss = depth_loss + depth_lambda * depth_loss
    return depth_loss


AGS_LAMBDA_FROM = 7000      # regularization_strategy.py:296 / :261, :274: a literal in the reference


def _shifted(t: Tensor, dy: int, dx: int) -> Tensor:
    """t[..., y + dy, x + dx] with zeros outside the frame (dy, dx in -1, 0, 1) — one tap of a conv2d with padding=1."""
    p = F.pad(t, (1, 1, 1, 1))
    H, W = t.shape[-2], t.shape[-1]
    return p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def ags_find_edges(gt_normal: Tensor, threshold: float = 0.01) -> Tensor:
    """``find_edges`` (regularization_strategy.py:40-96) on a [3,H,W] normal map in [-1, 1], bool [3,H,W]: per channel the
    Laplacian of 1 / (n + 1e-6) with zeros outside the frame — up + down + left + right - 4 r, in this order — above ``threshold``,
    then one 3 x 3 dilation (zeros outside).  The reference phrases both stencils as one-channel conv2d calls; the taps are written
    out here, so a component of exactly -1e-6 (r = inf) reaches its four neighbours only and inf - inf = nan compares false."""
    r = 1.0 / (gt_normal + 1e-6)
    lap = _shifted(r, -1, 0) + _shifted(r, 1, 0) + _shifted(r, 0, -1) + _shifted(r, 0, 1) - 4 * r
    e = (lap > threshold).to(torch.uint8)
    out = torch.zeros_like(e)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out = out | _shifted(e, dy, dx)
    return out > 0


def ags_normal_confidence(surf_normal: Tensor, gt_normal: Tensor, max_angle: float = 0.1) -> Tensor:
    """The filter of regularization_strategy.py:299-300, :311 on [3,H,W] normals, bool [H,W]: not (``mean_angular_error`` >
    0.1 rad), the angle being arccos(clip(sum_c gt_c surf_c, -1, 1)) (:11-26).  A nan dot product is confident."""
    dot = torch.clip((gt_normal * surf_normal).sum(dim=0), -1.0, 1.0)
    return ~(torch.arccos(dot) > max_angle)


def ags_normal_loss(surf_normal: Tensor, gt_normal: Tensor, pred_normal: Tensor, step: int, normal_lambda: float = 0.1,
                    normal_mask_steps: int = 15000, selection: Optional[Tensor] = None) -> Tensor:
    """``AGSMeshRegularization.get_normal_loss`` (regularization_strategy.py:292-321) on [3,H,W] normals in [-1, 1]:
    lambda = normal_lambda after step 7000, else 0; before ``normal_mask_steps`` the L1 mean of surf - gt over the ELEMENTS off the
    dilated edge map, from then on over the three channels of the confident pixels; plus the L1 mean of pred - gt over everything;
    both times lambda.  Two boolean-mask gathers (a host synchronisation each); nothing selected: nan.
    ``selection``: the mask to use instead of the one computed here — bool [3,H,W] (elements kept) before ``normal_mask_steps``,
    bool [H,W] (pixels kept) from then on."""
    lam = normal_lambda if step > AGS_LAMBDA_FROM else 0.0
    if step < normal_mask_steps:
        keep = ~ags_find_edges(gt_normal) if selection is None else selection
        normal_l1 = torch.abs(surf_normal[keep] - gt_normal[keep]).mean() * lam
    else:
        keep = ags_normal_confidence(surf_normal, gt_normal) if selection is None else selection
        normal_l1 = torch.abs(surf_normal[:, keep] - gt_normal[:, keep]).mean() * lam
    return normal_l1 + torch.abs(pred_normal - gt_normal).mean() * lam


def ags_depth_mask(gt_depth: Tensor, confidence: Tensor, step: int, tolerance: float = 0.1) -> Tensor:
    """The mask ``AGSMeshRegularization.get_depth_loss`` (regularization_strategy.py:257-290) hands to EdgeAwareLogL1: the valid
    ground-truth depths, from step 7000 on only where the confidence map is positive (there the reference zeroes the other depths
    first; a ground truth under a false mask is never counted, so the mask alone says it)."""
    mask = gt_depth > tolerance
    if step >= AGS_LAMBDA_FROM:
        mask = mask & (confidence > 0)
    return mask


def ags_regularization_term(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], scales: Tensor, step: int, depth_lambda: float = 0.2,
                            depth_tolerance: float = 0.1, normal_lambda: float = 0.1, normal_mask_steps: int = 15000) -> Tensor:
    """What dn-splatter adds in get_loss_dict (dn_model.py:629-727) for regularization_strategy == "ags-mesh" with mono depth and
    mono normal supervision: ``AGSMeshRegularization.get_loss`` (regularization_strategy.py:233-255) on what the method picks — the
    image clamped at 10/255 (:633), confidence = 1 - batch["confidence"] / 255 (:646), depth, the predicted normal and the two
    ground truths times ``batch["mask"]`` (:648-660; the surface normal is not), the three normal images as 2 x - 1 in [3,H,W]
    (:721-723).  Pinned to the reference's own text: tests/golden/reference_ags.npz."""
    gt_img = batch["image"].clamp(min=10 / 255.0)
    depth_out, pred_normal, surf_normal = outputs["depth"], outputs["normal"], outputs["surface_normal"]
    gt_depth, gt_normal = batch["mono_depth"], batch["normal"]
    confidence = 1 - batch["confidence"] / 255.0
    if "mask" in batch:
        mask = batch["mask"]
        depth_out, gt_depth, gt_normal, pred_normal = depth_out * mask, gt_depth * mask, gt_normal * mask, pred_normal * mask
    depth_mask = ags_depth_mask(gt_depth, confidence, step, depth_tolerance)
    loss = edge_aware_log_l1(depth_out, gt_depth.to(depth_out.dtype), gt_img, depth_mask) * depth_lambda

    def chw(im):
        return (2 * im - 1).permute(2, 0, 1)

    loss = loss + ags_normal_loss(chw(surf_normal), chw(gt_normal), chw(pred_normal), step, normal_lambda, normal_mask_steps)
    return loss + torch.min(torch.exp(scales), dim=1, keepdim=True)[0].mean()


def ags_mesh_loss(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], scales: Tensor, step: int, ssim_lambda: float = 0.2,
                  depth_lambda: float = 0.2, depth_tolerance: float = 0.1, normal_lambda: float = 0.1,
                  normal_mask_steps: int = 15000) -> Tensor:
    """main_loss of ``DNSplatterModel.get_loss_dict`` for regularization_strategy == "ags-mesh" (dn_model.py:614-729):
    rgb_loss + regularization_strategy_loss (:727)."""
    return rgb_term(outputs, batch, ssim_lambda) + ags_regularization_term(outputs, batch, scales, step, depth_lambda, depth_tolerance,
                                                                           normal_lambda, normal_mask_steps)


def _ssim_hip(pred: Tensor, gt: Tensor) -> Tensor:
    from .fused_loss import ssim_hip
    return ssim_hip(pred, gt)


def rgb_term(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], ssim_lambda: float = 0.2, fast: bool = False,
             ssim_impl: Optional[str] = None) -> Tensor:
    """nerfstudio splatfacto's main_loss, which DNSplatterModel.get_loss_dict takes over unchanged (dn_model.py:624-627, :663):
    (1 - l) * L1 + l * (1 - SSIM).  Restated from nerfstudio / pytorch_msssim's published definitions (not vendored: unpinned).
    ``ssim_impl``: "conv" (pytorch_msssim's ten grouped conv2d calls), "gemm", "stacked" (the same sums phrased for other library
    kernels; both measured slower) or "hip" — the SSIM module alone as one autograd node on ``dnsplat_ssim`` (what
    ``fused_loss.SSIM`` installs as splatfacto's ``self.ssim``), everything else of the stack in PyTorch."""
    pred_img = outputs["rgb"]
    ll1 = torch.abs(batch["image"] - pred_img).mean()
    if ssim_impl is None:
        ssim_impl = SSIM_FAST_IMPL if fast else "conv"
    impl = {"gemm": ssim_gemm, "stacked": ssim_stacked, "hip": _ssim_hip}.get(ssim_impl, ssim)
    simloss = 1 - impl(pred_img, batch["image"])
    return (1 - ssim_lambda) * ll1 + ssim_lambda * simloss


def regularization_term(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], scales: Tensor, depth_lambda: float = 0.2,
                        depth_tolerance: float = 0.1, use_depth_loss: bool = True, use_normal_loss: bool = True,
                        capturable: bool = False, hip_modules: bool = False) -> Tensor:
    """What dn-splatter itself adds in get_loss_dict (dn_model.py:629-727) for regularization_strategy == "dn-splatter" with mono
    depth / mono normal supervision: ``DNRegularization.get_loss`` (regularization_strategy.py:146-199) on the ground truths the
    method picks — the image clamped at 10/255 for the edge weights (:633), depth, both normals and their ground truths multiplied
    by ``batch["mask"]`` if there is one (:646-659).  Pinned to the reference's own text: tests/golden/reference_regularization.npz.
    ``hip_modules``: the two stencil modules as ``install_losses(model)`` swaps them (``fused_loss.EdgeAwareLogL1`` / ``TVLoss``)."""
    gt_img = batch["image"].clamp(min=10 / 255.0)                                   # dn_model.py:633
    depth_out, pred_normal = outputs["depth"], outputs["normal"]
    gt_depth, gt_normal = batch.get("mono_depth"), batch.get("normal")
    if "mask" in batch:                                                             # dn_model.py:646-659
        mask = batch["mask"]
        depth_out = depth_out * mask
        gt_depth = gt_depth * mask if gt_depth is not None else None
        gt_normal = gt_normal * mask if gt_normal is not None else None
        pred_normal = pred_normal * mask
    if hip_modules:
        from .fused_loss import scale_reg
        loss = scale_reg(scales)
    else:
        loss = torch.min(torch.exp(scales), dim=1, keepdim=True)[0].mean()          # regularization_strategy.py:195-199
    if use_depth_loss and gt_depth is not None:
        valid = gt_depth > depth_tolerance                                          # :162
        if hip_modules:
            from .fused_loss import EdgeAwareLogL1
            d = EdgeAwareLogL1()(depth_out, gt_depth.float(), gt_img, valid)
        else:
            d = edge_aware_log_l1(depth_out, gt_depth.float(), gt_img, valid, capturable)
        loss = loss + (d + depth_lambda * d)                                        # :184
    if use_normal_loss and gt_normal is not None:
        if hip_modules:
            from .fused_loss import TVLoss
            tv = TVLoss()(pred_normal)
        else:
            tv = tv_loss(pred_normal)
        loss = loss + torch.abs(pred_normal - gt_normal).mean() + tv                     # :188-193
    return loss


def dn_loss(outputs: Dict[str, Tensor], batch: Dict[str, Tensor], scales: Tensor, ssim_lambda: float = 0.2,
            depth_lambda: float = 0.2, depth_tolerance: float = 0.1, use_depth_loss: bool = True,
            use_normal_loss: bool = True, capturable: bool = False, ssim_impl: Optional[str] = None, hip_modules: bool = False) -> Tensor:
    """main_loss of ``DNSplatterModel.get_loss_dict`` for regularization_strategy == "dn-splatter" with mono depth
    and mono normal supervision (dn_model.py:614-729): rgb_loss + regularization_strategy_loss (:727).
    ``capturable``: the same terms in PyTorch ops that need no host synchronisation and no convolution library — masked means as
    sum / count (``edge_aware_log_l1``), SSIM blurs as GEMMs (``ssim_gemm``): the whole step can be captured into a HIP graph."""
    return rgb_term(outputs, batch, ssim_lambda, fast=capturable, ssim_impl=ssim_impl) + regularization_term(outputs, batch, scales, depth_lambda, depth_tolerance,
                                                                       use_depth_loss, use_normal_loss, capturable, hip_modules)


def synthetic_batch(width: int, height: int, device, seed: int = 0) -> Dict[str, Tensor]:
    """Random ground truth with the shapes the datamanager hands over (dn_datamanager.py:90-150)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(height, width, 3, generator=g)
    depth = torch.rand(height, width, 1, generator=g) * 9.0 + 0.5
    nrm = F.normalize(torch.randn(height, width, 3, generator=g), dim=-1)
    return {"image": img.to(device), "mono_depth": depth.to(device), "normal": ((nrm + 1) / 2).to(device)}
