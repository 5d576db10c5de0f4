"""Golden vectors of the Pearson depth losses, produced by THE REFERENCE's own classes: dn_splatter/losses.py:428-485
(PearsonDepthLoss, LocalPearsonDepthLoss) and DNRegularization.get_depth_loss in its PearsonDepth branch
(regularization_strategy.py:161-186), loaded by path as make_reference_golden.py loads them and executed on seeded inputs.

LocalPearsonDepthLoss.forward names ``device="cuda"`` literally (losses.py:473-479), the only obstacle on a machine without a GPU:
the loaded ``losses`` module gets a proxy for the name ``torch`` whose ``tensor`` and ``randint`` rewrite that one keyword to the CPU;
every other attribute is torch's own.  The origins a call drew are recovered by re-seeding and repeating its two draws.  Nothing of
the reference is copied: only inputs, drawn origins and the reference's OUTPUTS are stored (tests/golden/reference_pearson.npz).

    python tests/golden/make_reference_pearson_golden.py     # needs the reference checkout; rewrites reference_pearson.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_reference_golden import _load, load_reference  # noqa: E402


class _TorchOnCpu:
    """``torch`` with ``device="cuda"`` turned into the CPU in the two factory calls losses.py:473-479 make."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _cpu(kw):
        if kw.get("device") == "cuda":
            kw["device"] = "cpu"
        return kw

    def tensor(self, *a, **kw):
        return torch.tensor(*a, **self._cpu(kw))

    def randint(self, *a, **kw):
        return torch.randint(*a, **self._cpu(kw))


def draws(seed, H, W, box_p, p_corr=0.5):
    """The two draws of losses.py:475-476 after ``torch.manual_seed(seed)``."""
    torch.manual_seed(seed)
    n_corr = int(p_corr * (H // box_p) * (W // box_p))
    rows = torch.randint(0, H - box_p, size=(n_corr,))
    cols = torch.randint(0, W - box_p, size=(n_corr,))
    return rows, cols


def value_and_grad(fn, pred):
    x = pred.clone().requires_grad_(True)
    v = fn(x)
    (g,) = torch.autograd.grad(v, x)
    return np.float32(v.detach()), g.numpy()


def main(path=os.path.join(HERE, "reference_pearson.npz")):
    _, _, los = load_reference()
    los.torch = _TorchOnCpu()
    reg_mod = _load("dn_splatter.regularization_strategy", "dn_splatter/regularization_strategy.py")
    save = {}

    # (1) 72 x 48, boxes of 16: the whole-frame loss and the local loss (global seed 11: six boxes)
    W, H, box, seed = 72, 48, 16, 11
    g = torch.Generator().manual_seed(7)
    pred = torch.rand(H, W, 1, generator=g) * 4 + 1
    gt = 0.6 * pred + 0.8 * torch.rand(H, W, 1, generator=g) + 0.3
    rows, cols = draws(seed, H, W, box)
    whole, whole_grad = value_and_grad(lambda x: los.PearsonDepthLoss()(x, gt), pred)

    def local_small(x):
        torch.manual_seed(seed)
        return los.LocalPearsonDepthLoss()(x, gt, box_p=box)

    local, local_grad = value_and_grad(local_small, pred)
    save.update(small_W=W, small_H=H, small_box=box, small_seed=seed, small_pred=pred.numpy(), small_gt=gt.numpy(),
                small_rows=rows.numpy(), small_cols=cols.numpy(), small_whole=whole, small_whole_grad=whole_grad,
                small_local=local, small_local_grad=local_grad)
    print(f"72x48 box 16: whole {whole:.8f} local {local:.8f} rows {rows.tolist()} cols {cols.tolist()}")

    # (2) 400 x 272 at the default box of 128 (three boxes); inputs are exact in fp16 (a coarse grid of depths) and stored so
    W, H, seed = 400, 272, 5
    g = torch.Generator().manual_seed(23)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pred = 2.0 + xx / 256 + torch.sin(yy / 19.0) * 0.5 + torch.rand(H, W, generator=g) * 0.25
    gt = 0.5 * pred + 0.5 + torch.rand(H, W, generator=g) * 0.25
    gt[40:90, 100:180] = 0.0625                              # at or below depth_tolerance: invalid for the strategy
    pred = (pred * 64).round().div(64).half().float()[..., None]
    gt = (gt * 64).round().div(64).half().float()[..., None]
    rows, cols = draws(seed, H, W, 128)

    def local_big(x):
        torch.manual_seed(seed)
        return los.LocalPearsonDepthLoss()(x, gt)

    local, local_grad = value_and_grad(local_big, pred)
    save.update(big_W=W, big_H=H, big_seed=seed, big_pred=pred.numpy().astype(np.float16), big_gt=gt.numpy().astype(np.float16),
                big_rows=rows.numpy(), big_cols=cols.numpy(), big_local=local, big_local_grad=local_grad)
    print(f"400x272 box 128: local {local:.8f} rows {rows.tolist()} cols {cols.tolist()}")

    # (3) the strategy: DNRegularization(depth_loss_type = PearsonDepth).get_depth_loss on the inputs of (2) — the validity mask is
    # partly false — and on a ground truth without a valid pixel (nan).  The gradient is stored on every fourth row.
    strat = reg_mod.DNRegularization(depth_loss_type=los.DepthLossType.PearsonDepth)

    def strategy(x, target):
        torch.manual_seed(seed)
        return strat.get_depth_loss(x, target)

    value, grad = value_and_grad(lambda x: strategy(x, gt), pred)
    empty = strategy(pred, gt * 0.01)
    assert bool((gt > strat.depth_tolerance).any()) and not bool((gt > strat.depth_tolerance).all())
    assert torch.isnan(empty)
    save.update(strategy_defaults=np.array([strat.depth_tolerance, strat.depth_lambda], dtype=np.float64), strategy_value=value,
                strategy_grad_rows4=grad[::4], strategy_empty_scale=np.float32(0.01), strategy_empty_value=np.float32(empty))
    print(f"strategy: {value:.8f}, no valid pixel: {float(empty)}")

    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
