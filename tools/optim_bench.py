#!/usr/bin/env python3
"""Cost of the optimizer recipe (csrc/optim.hip) on UNetDC(3, 1) at batch 8 x 512^2 in bf16: the plain
fused step, then with global-norm clipping, with clipping and weight decay, and with clipping, decay and the EMA.
    python3 tools/optim_bench.py [--calls N] [--windows W]
One process.  HIP events around N back-to-back optimizer steps on the gradients of one backward (the optimizer alone), and
around N whole training steps (zero_grad, forward, loss, backward, step); median (min .. max) of W windows."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from models.model_2 import UNetDC
from oracle import recipe
from unet_dc_segmentation_amd.optim import FusedAdam
from utils.metrics_DC import focal_dice_loss

CASES = [("plain step", {}),
         ("+ clip", dict(clip_norm=1.0)),
         ("+ clip + decay", dict(clip_norm=1.0, weight_decay=1e-2)),
         ("+ clip + decay + EMA", dict(clip_norm=1.0, weight_decay=1e-2, ema_decay=0.999))]


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, calls, windows):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return np.median(out), f"{np.median(out):9.1f} us ({min(out):.1f} .. {max(out):.1f})"


def main():
    calls, windows = arg("--calls", 20), arg("--windows", 5)
    torch.manual_seed(0)
    model = UNetDC(3, 1).cuda().train()
    model.set_compute_dtype("bf16")
    x = recipe.seeded_input(1, (8, 3, 512, 512)).cuda()
    t = recipe.seeded_target(2, (8, 1, 512, 512), frac=0.1).cuda()
    n = sum(p.numel() for p in model.parameters())
    print(f"one MI355X; UNetDC(3, 1), {n} parameters ({4 * n / 1e6:.1f} MB fp32), batch 8 x 512^2, bf16; HIP events around {calls} "
          f"back-to-back calls, median (min .. max) of {windows} windows, us per call")

    def train(opt):
        opt.zero_grad()
        focal_dice_loss(model(x), t, alpha=1.0, gamma=2.0, ratio=0.3).backward()
        opt.step()

    base = {}
    for name, kw in CASES:
        opt = FusedAdam(model, lr=1e-4, **kw)
        train(opt)                                          # gradients in the flat buffer, state and table built
        alone, s_alone = timed(opt.step, calls, windows)
        whole, s_whole = timed(lambda: train(opt), calls, windows)
        base.setdefault("alone", alone), base.setdefault("whole", whole)
        print(f"{name:22s} optimizer alone: {s_alone}  {alone - base['alone']:+8.1f} | training step: {s_whole}  "
              f"{whole - base['whole']:+8.1f}")
        if kw:
            print(f"{'':22s} {opt.recipe_stats()}")
        del opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
