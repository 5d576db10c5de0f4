"""Golden vectors of the AGS-Mesh regularisation strategy, produced by THE REFERENCE's own code: find_edges and mean_angular_error
(dn_splatter/regularization_strategy.py:11-96), AGSMeshRegularization.get_normal_loss and get_depth_loss (:257-321), loaded by path as
make_reference_golden.py loads them, and the "ags-mesh" branch of DNSplatterModel.get_loss_dict (dn_model.py:614-729) executed from
its text as ``regularization_case`` does for the other strategy.

get_depth_loss calls ``.cuda()`` on the result of ``torch.where`` (:275), the only obstacle on a machine without a GPU: the loaded
module gets a proxy for the name ``torch`` whose ``where`` returns a tensor subclass with a no-op ``.cuda()``; every other attribute
is torch's own.  Nothing of the reference is copied: only inputs (tests/_ags_inputs.py) and the reference's OUTPUTS are stored
(tests/golden/reference_ags.npz).

    python tests/golden/make_reference_ags_golden.py     # needs the reference checkout; rewrites reference_ags.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_reference_golden import REF, _load, extract_method, load_reference  # noqa: E402

import _ags_inputs as inputs  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from dn_splatter_amd import torch_losses as tl  # noqa: E402

FRAMES = ((45, 70, 0), (33, 130, 1))           # H, W (neither a multiple of 16), seed of the noise: no borderline decision (asserted)
STEPS = (100, 7000, 7001, 14999, 15000)        # both sides of `step > 7000` and of `step < normal_mask_steps`


class _HereTensor(torch.Tensor):
    def cuda(self, *a, **k):
        return self


class _TorchOnCpu:
    """``torch`` whose ``where`` returns a tensor that is already "on the GPU" (regularization_strategy.py:275)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    def where(self, *a, **kw):
        return torch.where(*a, **kw).as_subclass(_HereTensor)


def strategy_cases(reg_mod, save):
    strat = reg_mod.AGSMeshRegularization()
    save["defaults"] = np.array([strat.depth_tolerance, strat.depth_lambda, strat.normal_lambda, strat.normal_mask_steps], dtype=np.float64)
    for H, W, seed in FRAMES:
        pre = f"f{H}x{W}_"
        gt_u8, surf, gt, pred = inputs.normal_inputs(H, W, seed=seed)
        edges = reg_mod.find_edges(gt)
        angle = reg_mod.mean_angular_error(surf, gt)
        conf = ~(angle > 0.1)
        # the recipe's conditions: the reference's fp32 decisions are those of exact arithmetic (find_edges itself pins its kernel
        # to float32, so the float64 edge map is the restatement's), and none of them is borderline
        edges64 = tl.ags_find_edges(gt.double())
        conf64 = ~(reg_mod.mean_angular_error(surf.double(), gt.double()) > 0.1)
        assert torch.equal(edges, edges64) and torch.equal(conf, conf64), "the reference's fp32 masks differ from its fp64 masks"
        n_fe = int(inputs.flagged_edge_decisions(gt).sum())
        n_fc = int(inputs.flagged_confidence_decisions(surf, gt).sum())
        assert n_fe == 0 and n_fc == 0, (n_fe, n_fc)
        save.update({pre + "gt_u8": gt_u8.numpy(), pre + "surf_q": torch.round(surf * inputs.GRID).to(torch.int16).numpy(),
                     pre + "pred_q": torch.round(pred * inputs.GRID).to(torch.int16).numpy(),
                     pre + "edges": np.packbits(edges.numpy()), pre + "confident": np.packbits(conf.numpy()),
                     pre + "angle": angle.numpy().astype(np.float32)})
        print(f"{H}x{W}: dilated edge share {float(edges.float().mean()):.3f}, confident {float(conf.float().mean()):.3f}")
        for step in STEPS:
            s = surf.clone().requires_grad_(True)
            p = pred.clone().requires_grad_(True)
            v = strat.get_normal_loss(step, s, gt, p)
            gs, gp = torch.autograd.grad(v, [s, p])
            # sgn x weight / count: three distinct values per tensor — stored as the sign pattern and the magnitude
            for name, gr in (("v_surf", gs), ("v_pred", gp)):
                mag = float(gr.abs().max())
                assert mag == 0.0 or bool(((gr == 0) | (gr.abs() == mag)).all())
                save[pre + f"s{step}_{name}_sign"] = torch.sign(gr).to(torch.int8).numpy()
                save[pre + f"s{step}_{name}_mag"] = np.float32(mag)
            save[pre + f"s{step}_value"] = np.float32(v.detach())
            print(f"  step {step:5d}: {float(v.detach()):.8f}")


def model_case(los, reg_mod, save, W=56, H=40, N=200, seed=31, step=8000):
    """get_loss_dict's "ags-mesh" branch with a confidence image and a mask in the batch; the parent's (nerfstudio's) rgb term is a
    recorded stand-in.  Also the strategy's depth loss on its own at steps 6999 / 7000."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.rand(*shape, generator=g)       # noqa: E731
    gt_u8, surf, _, pred = inputs.normal_inputs(H, W, seed=1)
    back = lambda chw: ((chw.permute(1, 2, 0) + 1) / 2).contiguous()      # noqa: E731   the [H,W,3] image in [0,1] the model holds
    image = rnd(H, W, 3)
    image[:6, :9] *= 0.02                                       # below the 10/255 clamp
    gt_depth = rnd(H, W, 1) * 6 + 0.2
    gt_depth[10:16, 20:31] = 0.05                               # below depth_tolerance
    confidence = torch.randint(0, 256, (H, W, 1), generator=g).float()
    confidence[5:25, 30:50] = 255.0                             # 1 - 255 / 255 = 0: not confident
    mask = torch.ones(H, W, 1)                                  # a block and three single pixels masked out: the masked ground
    mask[28:, :20] = 0.0                                        # truth is the image 0, the normal (-1, -1, -1), its rim an edge
    mask[3, 50] = mask[20, 5] = mask[33, 40] = 0.0
    gt_normal = gt_u8.float() / 255.0
    pred_depth = (rnd(H, W, 1) * 6 + 0.2).requires_grad_(True)
    pred_normal = back(pred).requires_grad_(True)
    surface_normal = back(surf).requires_grad_(True)
    pred_rgb = rnd(H, W, 3).requires_grad_(True)
    scales = (torch.randn(N, 3, generator=g) * 0.7 - 3.0).requires_grad_(True)
    strat = reg_mod.AGSMeshRegularization()
    masked_gt = inputs.to_chw(gt_normal * mask).contiguous()
    assert int(inputs.flagged_edge_decisions(masked_gt).sum()) == 0
    assert int(inputs.flagged_confidence_decisions(inputs.to_chw(surface_normal.detach()), masked_gt).sum()) == 0
    print(f"model case: dilated edge share {float(reg_mod.find_edges(masked_gt).float().mean()):.3f}")

    text = extract_method(os.path.join(REF, "dn_splatter/dn_model.py"), "DNSplatterModel", "get_loss_dict")
    rgb_term = (pred_rgb - image).abs().mean() * 0.8 + 0.05
    src = ("class _Base:\n"
           "    def get_loss_dict(self, outputs, batch, metrics_dict=None):\n"
           "        return {'main_loss': _RGB_TERM, 'scale_reg': _SCALE_REG}\n"
           "class _M(_Base):\n" + "\n".join("    " + ln for ln in text.splitlines()) + "\n")
    from typing import Dict, List, Union
    ns = dict(torch=torch, Dict=Dict, List=List, Union=Union, _RGB_TERM=rgb_term, _SCALE_REG=torch.tensor(0.0),
              normal_from_depth_image=None, CONSOLE=types.SimpleNamespace(log=lambda *a, **k: None))
    exec(compile(src, "dn_model.py::DNSplatterModel.get_loss_dict", "exec"), ns)
    me = ns["_M"]()
    me.config = types.SimpleNamespace(normal_supervision="mono", use_depth_loss=True, regularization_strategy="ags-mesh")
    me.regularization_strategy = strat
    me.get_gt_img = lambda im: im
    me.scales = scales
    me.step = step
    me.device = torch.device("cpu")
    outputs = {"rgb": pred_rgb, "depth": pred_depth, "normal": pred_normal, "surface_normal": surface_normal}
    batch = {"image": image, "mono_depth": gt_depth, "normal": gt_normal.clone(), "confidence": confidence, "mask": mask}
    main = me.get_loss_dict(outputs, batch)["main_loss"]
    gd, gn, gsn, gs = torch.autograd.grad(main, [pred_depth, pred_normal, surface_normal, scales])
    save.update(m_W=W, m_H=H, m_N=N, m_step=step, m_image=image.numpy(), m_gt_depth=gt_depth.numpy(), m_gt_normal_u8=gt_u8.numpy(),
                m_confidence=confidence.numpy().astype(np.uint8), m_mask=mask.numpy().astype(np.uint8),
                m_pred_depth=pred_depth.detach().numpy(), m_pred_normal=pred_normal.detach().numpy(),
                m_surface_normal=surface_normal.detach().numpy(), m_pred_rgb=pred_rgb.detach().numpy(),
                m_scales=scales.detach().numpy(), m_main=np.float64(main.item()), m_rgb_term=np.float64(rgb_term.item()),
                m_v_depth=gd.numpy(), m_v_normal=gn.numpy(), m_v_surface_normal=gsn.numpy(), m_v_scales=gs.numpy())
    print(f"get_loss_dict, ags-mesh, step {step}: {main.item():.8f} (rgb stand-in {rgb_term.item():.8f})")
    # the depth half on its own, either side of step 7000 (the confidence filter sets in AT 7000, the normal weight AFTER it)
    gt_img = image.clamp(min=10 / 255.0)
    conf = 1 - confidence / 255.0
    for st in (6999, 7000):
        d = pred_depth.detach().clone().requires_grad_(True)
        v = strat.get_depth_loss(step=st, pred_depth=d, gt_depth=gt_depth, confidence_map=conf, gt_img=gt_img)
        (gr,) = torch.autograd.grad(v, d)
        save[f"m_depth_loss_{st}"] = np.float64(v.item())
        save[f"m_depth_loss_{st}_grad"] = gr.numpy()
        print(f"  get_depth_loss at step {st}: {v.item():.8f}")


def main(path=os.path.join(HERE, "reference_ags.npz")):
    _, _, los = load_reference()
    reg_mod = _load("dn_splatter.regularization_strategy", "dn_splatter/regularization_strategy.py")
    reg_mod.torch = _TorchOnCpu()
    save = {}
    strategy_cases(reg_mod, save)
    model_case(los, reg_mod, save)
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
