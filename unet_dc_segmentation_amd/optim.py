"""Fused Adam for the HIP path: ONE kernel per step updates every fp32 master parameter and rewrites the packed
compute-type weight images the conv kernels read (csrc/optim.hip, C ABI ``unetdc_adam_step``).

Reference: ``optimizer = optim.Adam(model.parameters(), lr=0.001)`` ... ``optimizer.step()``
(/root/reference/train_DC_focal.py:224,255; train.py:125,157).  Same update rule and defaults as
``torch.optim.Adam`` (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad); ``state_dict()`` carries the same
per-parameter entries (``step``, ``exp_avg``, ``exp_avg_sq``), so a checkpointed optimizer state moves between the two.

What is saved against torch.optim.Adam(fused=True) + the engine's re-pack launch: the 124 MB of parameters are read and
written once per step instead of three times, and the gradients are read straight out of the flat buffer the backward
kernels wrote (``grad_scale`` folds the 1/G of a SUM all-reduce into that read).  On CPU tensors (or any parameter set
that does not belong to one HIP module) the class falls back to the plain per-tensor formulas in PyTorch -- that is the
reference's own code path on a host without a GPU, not a fallback of the HIP path.

The fine-tuning recipe, all opt-in -- with the four arguments at their defaults step() launches
``unetdc_adam_step`` exactly as before and allocates nothing more:
  weight_decay, decay   decoupled weight decay (torch.optim.AdamW's rule, p <- p (1 - lr wd) before the update) on the
                        parameters with dim() >= 2 (decay="weights": conv, transposed-conv and head weights; biases and the
                        BatchNorm affine are left alone) or on every parameter (decay="all": torch's one-group AdamW);
  clip_norm             global-norm clipping by torch.nn.utils.clip_grad_norm_'s rule.  ``unetdc_grad_norm`` leaves the
                        coefficient in a device-resident record that the step kernel reads: the norm never reaches the host;
  skip_nonfinite        the guard that comes with clip_norm, for use without clipping: a step whose gradient holds an inf or
                        a NaN is dropped on the device (parameters, moments, images and EMA stay bit for bit);
  ema_decay             an exponential moving average of the parameters, updated in the step kernel; ema_weights() swaps it
                        into the module for validation and checkpoints.
The step counter: the host cannot know that the device dropped a step without waiting for it, so the counter (and with it the
bias corrections and the EMA warm-up) advances on a skipped step too -- the bias corrections run one step ahead per skipped
step.  The CPU formulas do the same.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import _lib

_DESC = np.dtype([("p", "<u8"), ("m", "<u8"), ("v", "<u8"), ("wf", "<u8"), ("wd", "<u8"), ("g_off", "<i8"),
                  ("begin", "<i8"), ("numel", "<i8"), ("a", "<i4"), ("b", "<i4"), ("kind", "<i4"), ("flags", "<i4")])
assert _DESC.itemsize == 80
# unetdc_step_ctl (include/unetdc_hip.h): written by unetdc_grad_norm, read by unetdc_adam_step_ex, zeroed once here
_CTL = np.dtype([("sumsq", "<f8"), ("norm", "<f8"), ("gscale_eff", "<f4"), ("skip", "<i4"), ("steps", "<i8"),
                 ("clipped", "<i8"), ("skipped", "<i8"), ("norm_sum", "<f8")])
assert _CTL.itemsize == 56
EMA_KEY = "ema"          # top-level key of state_dict(): the flat EMA buffer (parameters() order)


def ema_decay_at(decay, step):
    """The effective EMA decay of optimizer step `step` (counted from 1): min(D, (1 + t) / (10 + t)), the usual warm-up -- a
    0.999 average of a freshly initialised network is useless for the first thousand steps."""
    return min(float(decay), (1.0 + step) / (10.0 + step))


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, weight_decay=0.0, decay="weights",
                 clip_norm=None, ema_decay=None, skip_nonfinite=False):
        if not isinstance(model, torch.nn.Module):
            raise TypeError("FusedAdam takes the U-Net module (it needs the module's packed weight images), "
                            "not a parameter list")
        if decay not in ("weights", "all"):
            raise ValueError(f"decay must be 'weights' or 'all', not {decay!r}")
        if not weight_decay >= 0.0:
            raise ValueError(f"weight_decay must be >= 0, not {weight_decay}")
        if clip_norm is not None and not clip_norm > 0.0:
            raise ValueError(f"clip_norm must be > 0 (None: no clipping), not {clip_norm}")
        if ema_decay is not None and not 0.0 <= ema_decay <= 1.0:
            raise ValueError(f"ema_decay must be in [0, 1] (None: no EMA), not {ema_decay}")
        self.model = model
        # the full set of torch.optim.Adam defaults: a state_dict() of this class loads into torch.optim.Adam (whose
        # step() reads every one of these keys from the group) and the other way round; with weight decay the group is
        # torch.optim.AdamW's (decoupled_weight_decay=True)
        super().__init__(list(model.parameters()),
                         dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                              foreach=None, capturable=False, differentiable=False, fused=None,
                              decoupled_weight_decay=bool(weight_decay)))
        self.grad_scale = float(grad_scale)
        self.decay = decay
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.guard = clip_norm is not None or bool(skip_nonfinite)
        self._step = 0
        self._table = None
        self._table_key = None

    # ------------------------------------------------------------------ state
    def _init_state(self):
        params = self.param_groups[0]["params"]
        dev = params[0].device
        n = sum(p.numel() for p in params)
        self._m = torch.zeros(n, device=dev, dtype=torch.float32)
        self._v = torch.zeros(n, device=dev, dtype=torch.float32)
        self._offs, o = [], 0
        # ONE step counter object shared by every parameter's state entry (torch.optim.Adam keeps one per parameter, all
        # equal): 82 separate `step += 1` on 0-dim CPU tensors cost ~0.8 ms of host time per training step
        self._step_t = torch.tensor(float(self._step))
        for p in params:
            self._offs.append(o)
            st = self.state[p]
            st["step"] = self._step_t
            st["exp_avg"] = self._m[o:o + p.numel()].view_as(p)
            st["exp_avg_sq"] = self._v[o:o + p.numel()].view_as(p)
            o += p.numel()
        self._n = n
        if self.ema_decay is not None:
            # the moments' flat layout: the step kernel finds a tensor's average at ema + (m - m_base)
            with torch.no_grad():
                self._ema = torch.cat([p.detach().reshape(-1).float() for p in params])
            self._ema_views = [self._ema[off:off + p.numel()].view_as(p) for p, off in zip(params, self._offs)]
        if self.guard:
            if dev.type == "cuda":
                self._ctl = torch.zeros(_CTL.itemsize, dtype=torch.uint8, device=dev)
                self._norm_ws = torch.empty(max(8, int(_lib.load().unetdc_grad_norm_workspace(n))), dtype=torch.uint8, device=dev)
            else:
                self._cpu_stats = dict(steps=0, clipped=0, skipped=0, norm_sum=0.0)

    def state_dict(self):
        """torch.optim.Adam's layout: every parameter's entry carries its OWN ``step`` tensor (the shared counter object is
        an internal economy; handing it out would make a non-fused torch Adam advance it once per parameter).  With an EMA
        the flat buffer rides along under the extra top-level key ``ema`` (torch's optimizers ignore it)."""
        sd = super().state_dict()
        # torch.optim.Optimizer.state_dict() hands out the LIVE per-parameter dicts: build copies, never assign into them
        sd["state"] = {k: (dict(st, step=torch.tensor(float(self._step))) if "step" in st else st)
                       for k, st in sd["state"].items()}
        if self.ema_decay is not None and hasattr(self, "_ema"):
            sd[EMA_KEY] = self._ema
        return sd

    def load_state_dict(self, state_dict):
        for g in state_dict.get("param_groups", ()):
            if g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("FusedAdam implements Adam / AdamW only (amsgrad=False, maximize=False)")
            if g.get("weight_decay", 0) and not g.get("decoupled_weight_decay", False):
                raise ValueError("FusedAdam implements decoupled weight decay only (torch.optim.AdamW's rule), not the L2 term "
                                 "of torch.optim.Adam(weight_decay=...)")
        ema = state_dict.get(EMA_KEY)
        super().load_state_dict({k: v for k, v in state_dict.items() if k != EMA_KEY})
        params = self.param_groups[0]["params"]
        if params and "exp_avg" in self.state.get(params[0], {}):
            loaded = [(self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in params]
            self._step = int(float(self.state[params[0]]["step"]))
            self._init_state()                     # flat buffers; copy the loaded moments into them
            for p, (ea, es) in zip(params, loaded):
                self.state[p]["exp_avg"].copy_(ea)
                self.state[p]["exp_avg_sq"].copy_(es)
            if ema is not None and self.ema_decay is not None:
                self._ema.copy_(ema.reshape(-1))
            self._table = None

    # ------------------------------------------------------------------ EMA
    def ema_tensors(self):
        """The moving averages, one view per parameter in parameters() order (created as a copy of the parameters)."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdam was built without ema_decay")
        if not hasattr(self, "_m"):
            self._init_state()
        return self._ema_views

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside: the module's parameters hold the moving averages (torch._foreach_copy_: the version counters bump, so the
        engine re-packs by its existing rule); on exit the parameters are restored bit for bit.  BatchNorm running statistics
        are left as they are."""
        ema = self.ema_tensors()
        params = self.param_groups[0]["params"]
        with torch.no_grad():
            saved = [p.detach().clone() for p in params]
            torch._foreach_copy_(params, ema)
        try:
            yield self
        finally:
            with torch.no_grad():
                torch._foreach_copy_(params, saved)

    def recipe_stats(self):
        """{steps, clipped, skipped, grad_norm_mean} since the state was created, from ONE read of the device record (the
        mean is over the finite norms, before clipping).  Without clip_norm / skip_nonfinite no norm is taken: the counts are
        the host's and grad_norm_mean is None."""
        if hasattr(self, "_ctl"):
            r = self._ctl.cpu().numpy().view(_CTL)[0]
            s = dict(steps=int(r["steps"]), clipped=int(r["clipped"]), skipped=int(r["skipped"]), norm_sum=float(r["norm_sum"]))
        elif hasattr(self, "_cpu_stats"):
            s = dict(self._cpu_stats)
        else:
            return dict(steps=self._step, clipped=0, skipped=0, grad_norm_mean=None)
        done = s["steps"] - s["skipped"]
        return dict(steps=s["steps"], clipped=s["clipped"], skipped=s["skipped"],
                    grad_norm_mean=s["norm_sum"] / done if done else 0.0)

    # ------------------------------------------------------------------ descriptor table
    def _decays(self, p):
        return self.decay == "all" or p.dim() >= 2

    def _build_table(self, weights):
        params = self.param_groups[0]["params"]
        packed = {}
        if weights is not None:
            for w, wf, wd, a, b, kind in weights.entries():
                packed[id(w)] = (wf, wd, a, b, kind)
        tab = np.zeros(len(params), dtype=_DESC)
        begin = 0
        for i, (p, off) in enumerate(zip(params, self._offs)):
            m_ptr = self._m.data_ptr() + 4 * off
            v_ptr = self._v.data_ptr() + 4 * off
            flags = int(self._decays(p))           # (read by unetdc_adam_step_ex only)
            if id(p) in packed:
                wf, wd, a, b, kind = packed[id(p)]
                tab[i] = (p.data_ptr(), m_ptr, v_ptr, wf.data_ptr(), wd.data_ptr(), off, begin, p.numel(), a, b, kind, flags)
                begin += (a // 32) * (b // 32)
            else:
                tab[i] = (p.data_ptr(), m_ptr, v_ptr, 0, 0, off, begin, p.numel(), 0, 0, 2, flags)
                begin += (p.numel() + 4095) // 4096
        self._table = torch.from_numpy(tab.view(np.uint8).copy()).to(params[0].device)
        self._blocks = begin

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        params = group["params"]
        if any(p.grad is None for p in params):
            raise RuntimeError("FusedAdam.step(): every parameter needs a gradient (one backward through the module)")
        if not hasattr(self, "_m"):
            self._init_state()
        self._step += 1
        lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        recipe = bool(wd) or self.guard or self.ema_decay is not None
        if not params[0].is_cuda:
            self._step_torch(params, lr, b1, b2, eps, wd)
            return loss
        # gradients: normally the views autograd got from the HIP backward, i.e. ONE flat buffer in parameters() order
        base = params[0].grad.data_ptr()
        flat_ok = all(p.grad.is_contiguous() and p.grad.dtype == torch.float32 and
                      p.grad.data_ptr() == base + 4 * off for p, off in zip(params, self._offs))
        if flat_ok:
            flat_ptr, keep = base, None
        else:
            keep = torch.cat([p.grad.reshape(-1).float() for p in params])
            flat_ptr = keep.data_ptr()
        # the module's packed weight images (engine.PackedWeights: one set per module, shared by the engines of every input
        # shape); keyed by its never-reused serial, not id(): a rebuilt object may be handed a freed one's address
        weights = getattr(self.model, "_weights", None)
        key = (getattr(weights, "serial", None), tuple(p.data_ptr() for p in params))
        if self._table is None or self._table_key != key:
            self._build_table(weights)
            self._table_key = key
        dt = weights.dt if weights is not None else _lib.F32
        stream = torch.cuda.current_stream().cuda_stream
        if not recipe:
            _lib.call("unetdc_adam_step", self._table.data_ptr(), len(params), self._blocks, flat_ptr, float(lr), float(b1),
                      float(b2), float(eps), self._step, self.grad_scale, dt, stream)
        else:
            ctl = None
            if self.guard:
                # the norm of grad_scale * g, the clipping coefficient and the guard: all of it stays on the device
                ctl = self._ctl.data_ptr()
                _lib.call("unetdc_grad_norm", flat_ptr, self._n, self.grad_scale, self.clip_norm or 0.0, ctl,
                          self._norm_ws.data_ptr(), self._norm_ws.numel(), stream)
            ema, d = (None, 0.0) if self.ema_decay is None else (self._ema.data_ptr(), ema_decay_at(self.ema_decay, self._step))
            _lib.call("unetdc_adam_step_ex", self._table.data_ptr(), len(params), self._blocks, flat_ptr, float(lr), float(b1),
                      float(b2), float(eps), self._step, self.grad_scale, dt, ctl, float(wd), ema, self._m.data_ptr(), d, stream)
        if weights is not None:
            # both packed images were just rewritten from the parameters as they are NOW: the next forward skips its own
            # re-pack only while these version counters still stand (load_state_dict / copy_ / clamp_ after this step bump them)
            # (a step the device dropped left parameters AND images as they were: still a matching pair)
            weights.fresh(tuple(w._version for w, *_ in weights.entries()))
        self._step_t += 1
        return loss

    def _step_torch(self, params, lr, b1, b2, eps, wd=0.0):
        """CPU tensors, PyTorch ops: the same rules (clip_grad_norm_'s formula for the coefficient; the gradients are left as
        they are, like on the device)."""
        self._step_t += 1
        grads = [p.grad * self.grad_scale if self.grad_scale != 1.0 else p.grad for p in params]
        if self.guard:
            total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2.0) for g in grads]), 2.0)
            s = self._cpu_stats
            s["steps"] += 1
            if not bool(torch.isfinite(total)):
                s["skipped"] += 1
                return
            s["norm_sum"] += float(total)
            if self.clip_norm is not None:
                coef = torch.clamp(self.clip_norm / (total + 1e-6), max=1.0)
                s["clipped"] += int(float(coef) < 1.0)
                grads = [g * coef for g in grads]
        bc1, bc2 = 1.0 - b1 ** self._step, 1.0 - b2 ** self._step
        d = None if self.ema_decay is None else ema_decay_at(self.ema_decay, self._step)
        for k, (p, g) in enumerate(zip(params, grads)):
            st = self.state[p]
            if wd and self._decays(p):
                p.mul_(1.0 - lr * wd)
            st["exp_avg"].lerp_(g, 1.0 - b1)
            st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
            denom = (st["exp_avg_sq"].sqrt() / (bc2 ** 0.5)).add_(eps)
            p.addcdiv_(st["exp_avg"], denom, value=-lr / bc1)
            if d is not None:
                e = self._ema_views[k]
                e.add_(p - e, alpha=1.0 - d)
