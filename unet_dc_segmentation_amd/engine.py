"""Forward/backward schedule of the U-Net / U-Net-DC on the HIP kernels.

PyTorch is plumbing here: device memory (caching allocator), the current stream, autograd's
entry/exit points.  Every arithmetic op of ``UNetDC.forward`` (the reference's models/model_2.py:56-80)
and of its autograd is one of the C-ABI calls in ``include/unetdc_hip.h``.

Data layout in HBM
------------------
* activations: NHWC 2-D tensors ``[N*H*W, C]`` in the compute type (fp32 or bf16);
* decoder concat (``torch.cat([up, skip], 1)``, model_2.py:68-77): ONE ``[pixels, 2C]`` buffer per
  level -- the up-convolution writes columns ``[0, C)``, the encoder's normalise+ReLU pass writes
  its skip into columns ``[C, 2C)``; the concat itself moves no bytes, and in backward the two halves
  of the concat gradient are consumed in place (ConvT backward / encoder backward);
* per conv stage the raw (pre-BatchNorm) output ``y`` is kept for backward; the activation
  ``a = relu(scale*y + shift)`` is stored once (it is the next conv's input and the wgrad operand) --
  except where the consumer normalises ``y`` on load in training (see the plan below);
* parameters stay fp32 ``nn.Parameter``s in PyTorch layout; K-contiguous packed copies in the
  compute type are derived caches (ONE set per module, shared by the engines of every input shape)
  re-packed when a parameter's version counter changes or rewritten by the optimizer kernel;
* gradients are written by the kernels straight into one flat fp32 buffer in ``parameters()``
  order (so data-parallel buckets are contiguous slices, see dp.py).

The plan
--------
The topology is ``unet.conv_stages``.  Everything that depends only on the model, the input shape and the
compute type is decided when the engine is built: each ``_Stage`` records its kernel forms and the tensors
they read and write, the library's capability queries are asked there once, and the workspace is sized
from the calls the plan issues.  forward() and backward() walk the stages in order; what they decide per
call is train or eval, frozen statistics and whether dL/dx is asked for.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import call
from .unet import BLOCK_ORDER, ENCODER, conv_stages

_byref = ctypes.byref
# references to a tensor's storage (tensor + views + Python wrappers); absent on a torch build without it: allocate per step
_storage_use_count = getattr(torch._C, "_storage_Use_Count", None)

# The training forms the plan chooses from (each bit-identical to the stand-alone passes it replaces):
#  * "bnin": the second stage of an encoder or decoder block reads the first stage's RAW conv output, and its convolution and
#    weight gradient apply the first stage's BatchNorm + ReLU per staged tile in LDS (unetdc_conv3x3_fwd_bnin /
#    unetdc_conv3x3_wgrad_bnin): the first stage's normalisation pass and activation tensor disappear.  "bnin_store": the
#    forward also stores that activation, and the plain weight gradient reads it.  Where unetdc_conv3x3_bnin_supported says so;
#  * the head reads dec1.3's RAW conv output and applies its BatchNorm + ReLU on load (unetdc_head_fwd_bn): dec1.3 stores no
#    activation.  With one output channel and batch statistics the gradient of the head's input is dz * w[c] per pixel, and
#    dec1.3's BatchNorm backward recomputes it (unetdc_bn_relu_bwd_head) instead of reading a tensor the head backward wrote;
#  * the dgrad that writes a stage's incoming gradient also produces that stage's BatchNorm-backward sums (*_dgrad_bnstats,
#    unetdc_head_bwd_bnstats); every stage but an encoder's second, whose gradient arrives through the max-pool;
#  * the decoder's first dgrad also sums the up-convolution half of the concat gradient per channel: the ConvTranspose2d
#    bias gradient (unetdc_conv3x3_dgrad_colsum);
#  * "first_bn": the first layer's weight gradient applies its stage's BatchNorm + ReLU backward on load
#    (unetdc_conv3x3_first_wgrad_bn) -- per call only when nothing else reads that stage's dy (no dL/dx) and the statistics
#    are the batch's.  Where unetdc_conv3x3_first_wgrad_bn_supported says so.
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class PackedWeights:
    """The K-contiguous compute-type weight images of ONE module (per device and compute type): ``w_fwd[9][Cout][Cin]`` /
    ``w_dgrad[9][Cin][Cout]`` per 3x3 conv (taps flipped), ``w_fwd[4*Cout][Cin]`` / ``w_dgrad[4][Cin][Cout]`` per
    ConvTranspose2d.  They depend on the parameters only, not on the input shape, so every engine of the module (one per
    input shape, unet.py) reads the same set and the optimizer kernel (optim.FusedAdam) writes one set."""
    _serials = __import__("itertools").count(1)

    def __init__(self, model, device, tdtype, dt):
        self.serial = next(PackedWeights._serials)     # identity that is never reused (id() of a freed object can be)
        self.model, self.device, self.tdtype, self.dt = model, device, tdtype, dt
        self.conv, self.up = {}, {}
        for i, (block, idx, level, cin, cout, _) in enumerate(conv_stages(model.in_channels, model.DILATIONS)):
            if i:                                       # the C_in = 1/3 first layer reads the fp32 master directly
                self._add_conv(block, idx, cin, cout)
            if block.startswith("dec") and idx == 3:    # upconv<level+1> writes half of this block's input
                self.up[level + 1] = dict(mod=getattr(model, f"upconv{level + 1}"), cin=2 * cout, cout=cout,
                                          w_fwd=torch.empty(4 * cout * 2 * cout, device=device, dtype=tdtype),
                                          w_dgrad=torch.empty(4 * cout * 2 * cout, device=device, dtype=tdtype))
        self._versions = None          # parameter version counters the images were last built from
        self._fresh_versions = None    # set by an optimizer that has just written the images itself
        self._ptrs = None
        self._trained = False          # a train-mode forward has run: optimizer steps may follow at any time

    def _add_conv(self, block, idx, cin, cout):
        conv = getattr(self.model, block)[idx]
        self.conv[(block, idx)] = dict(mod=conv, cin=cin, cout=cout,
                                       w_fwd=torch.empty(9 * cout * cin, device=self.device, dtype=self.tdtype),
                                       w_dgrad=torch.empty(9 * cout * cin, device=self.device, dtype=self.tdtype))

    def entries(self):
        """(parameter, fwd image, dgrad image, a, b, kind) for every packed tensor, in a fixed order."""
        ent = [(c["mod"].weight, c["w_fwd"], c["w_dgrad"], c["cout"], c["cin"], 0) for c in self.conv.values()]
        ent += [(u["mod"].weight, u["w_fwd"], u["w_dgrad"], u["cin"], u["cout"], 1) for u in self.up.values()]
        return ent

    def invalidate(self):
        """Force the next forward to rebuild the images (call after writing parameters through a path that bumps no
        version counter)."""
        self._versions = None

    def fresh(self, versions):
        """Called by an optimizer that writes the images itself (FusedAdam, optim.py) with the version counters of the
        packed parameters at that moment: the next forward needs no re-pack IF those counters still stand (any write in
        between -- load_state_dict, copy_, clamp_, an EMA swap -- bumps one of them and the images are rebuilt)."""
        self._fresh_versions = tuple(versions)

    def ensure(self, need_dgrad):
        """Re-pack the images when they may be stale: ONE launch over a device-resident descriptor table.  Fused
        optimizers such as torch.optim.Adam(fused=True) update parameters WITHOUT bumping their version counters, so
        once a train-mode forward has run on this module (an optimizer may be stepping the parameters) the images are
        rebuilt on every forward, eval-mode ones included (train fwd, eval fwd, opt.step(), eval fwd must not see stale
        weights; the launch costs ~0.1 ms); in a pure-inference process the version counters (load_state_dict, copy_)
        decide.  An optimizer that writes the images itself (optim.FusedAdam) announces it through fresh() and the pack
        is skipped while the counters it saw still stand."""
        import numpy as np
        ent = self.entries()
        versions = tuple(w._version for w, *_ in ent)
        ptrs = tuple(w.data_ptr() for w, *_ in ent)
        if self._ptrs != ptrs:
            dt = np.dtype([("w", "<u8"), ("wf", "<u8"), ("wd", "<u8"), ("begin", "<i8"), ("a", "<i4"), ("b", "<i4"),
                           ("kind", "<i4"), ("pad", "<i4")])
            tab = np.zeros(len(ent), dtype=dt)
            off = 0
            for i, (w, wf, wd, a, b, kind) in enumerate(ent):
                tab[i] = (w.data_ptr(), wf.data_ptr(), wd.data_ptr(), off, a, b, kind, 0)
                off += (a // 32) * (b // 32)                 # 32 x 32 channel tiles of this tensor
            self._table = torch.from_numpy(tab.view(np.uint8).copy()).to(self.device)
            self._total, self._ptrs, self._versions = off, ptrs, None
        self._trained = self._trained or need_dgrad
        fresh, self._fresh_versions = self._fresh_versions, None
        if fresh is not None and fresh == versions and self._versions is not None:
            self._versions = versions          # the optimizer step wrote both images and nothing touched the parameters since
            return
        if self._trained or self._versions != versions:
            call("unetdc_pack_many", self._table.data_ptr(), len(ent), self._total, self.dt, _stream())
            self._versions = versions


class _Stage:
    """One conv3x3 -> BatchNorm -> ReLU stage: parameters, saved tensors, and its part of the plan (UNetEngine._build)."""

    def __init__(self, eng, block, idx, level, cin, cout, dil, first):
        m = getattr(eng.model, block)
        self.name = f"{block}.{idx}"
        self.conv, self.bn = m[idx], m[idx + 1]
        self.level, self.cin, self.cout, self.dil, self.first = level, cin, cout, dil, first
        self.hw, self.npix = eng.res[level], eng.npix[level]
        dev, dt = eng.device, eng.tdtype
        f32 = dict(device=dev, dtype=torch.float32)
        lib = _lib.load()
        self.y = torch.empty(self.npix, cout, device=dev, dtype=dt)          # raw conv output (pre-BN)
        if first:
            self.stat_rows = lib.unetdc_conv3x3_first_stats_rows(self.npix, cin, cout)
        else:
            self.stat_rows = lib.unetdc_conv3x3_stats_rows(self.npix, cout)
            img = eng.weights.conv[(block, idx)]
            self.w_fwd, self.w_dgrad = img["w_fwd"], img["w_dgrad"]
        self.stats = torch.empty(_lib.partial_floats(self.stat_rows, 2 * cout), **f32)
        self.scale, self.shift = torch.empty(cout, **f32), torch.empty(cout, **f32)
        self.mean, self.rstd = torch.empty(cout, **f32), torch.empty(cout, **f32)
        # BatchNorm-backward partial sums of the dgrad kernel that writes this stage's incoming gradient: rows = 256-pixel blocks
        self.bwd_rows = lib.unetdc_conv3x3_stats_rows(self.npix, cout)
        self.bwd_parts, self.bwd_nparts, self.bwd_coeffs = None, 0, None
        # the plan: kernel forms and the tensors they read and write
        self.fwd = "first" if first else "plain"     # training forward: "first", "plain", "bnin" or "bnin_store"
        self.wgrad = "first" if first else "plain"   # weight gradient: "first", "first_bn", "bnin" or "plain"
        self.src = None        # activated input [npix, cin] (None for the first layer: it reads the NCHW image)
        self.bnin = None       # stage whose RAW output the "bnin" forms read and normalise on load
        self.out = None        # activation [npix, cout]: written by every eval forward, by a training forward if `store`
        self.store = True
        self.pooled = None     # its 2x2 max-pooled copy (encoder blocks)
        self.up = None         # decoder stage 0: the ConvTranspose2d (packed images) that writes `up_out`, the first half
        self.up_src = None     # of `src`, from the activation of the stage `up_src`
        self.up_out = None
        self.dx_bn = None      # stage whose BatchNorm-backward sums the input-gradient dgrad also produces
        self.dx_colsum = None  # parameter that receives the column sums of dx[:, :cout] (the up-convolution bias gradient)
        # gradient views, bound when the gradient buffers are allocated (first backward)
        self.dy = None         # gradient of the conv output
        self.g_out = None      # incoming gradient of `out`
        self.g_pool = None     # incoming gradient of `pooled`
        self.dx = None         # input gradient [npix, cin] (None for the first layer)
        self.up_dout = None    # gradient of `up_out`


class UNetEngine:
    def __init__(self, model, x, weights=None):
        _lib.load()
        if not x.is_cuda:
            raise _lib.UnetdcError("UNetEngine needs a HIP device tensor")
        self.model = model
        self.device = x.device
        self.N, self.cin, self.H, self.W = x.shape
        if self.H % 16 or self.W % 16:
            raise ValueError(f"H and W must be multiples of 16 (4 poolings), got {self.H}x{self.W}")
        if self.cin != model.in_channels:
            raise ValueError(f"expected {model.in_channels} input channels, got {self.cin}")
        self.dtype_name = model.compute_dtype
        self.dt = _lib.BF16 if self.dtype_name == "bf16" else _lib.F32
        self.tdtype = torch.bfloat16 if self.dtype_name == "bf16" else torch.float32
        self.oc = model.out_channels
        # packed weight images: shared by every engine of the module (they do not depend on the input shape)
        if weights is None or weights.device != self.device or weights.dt != self.dt or weights.model is not model:
            weights = PackedWeights(model, self.device, self.tdtype, self.dt)
        self.weights = weights
        self.frozen = False            # per forward: BatchNorm statistics from the running buffers (eval mode under autograd)
        self.need_dx = False           # per backward: input_grad() follows, so the first stage writes its dy
        self._build()

    # ------------------------------------------------------------------ construction
    def matches(self, x):
        return (x.device == self.device and tuple(x.shape) == (self.N, self.cin, self.H, self.W)
                and self.dtype_name == self.model.compute_dtype)

    def _build(self):
        """The plan: buffers, and every kernel form that depends only on the model, the input shape and the compute type."""
        dev, dt = self.device, self.tdtype
        N, H, W = self.N, self.H, self.W
        lib = _lib.load()
        self.res = [(H >> l, W >> l) for l in range(len(ENCODER) + 1)]
        self.npix = [N * h * w for h, w in self.res]
        self.stages = {}
        for i, (block, idx, level, cin, cout, dil) in enumerate(conv_stages(self.cin, self.model.DILATIONS)):
            self.stages[(block, idx)] = _Stage(self, block, idx, level, cin, cout, dil, first=(i == 0))
        # activations: stage 0's output of every block (a0), stage 3's of the bottleneck and the decoder (a3); an encoder
        # block's stage 3 writes the skip half of its level's concat buffer (cat) and the pooled tensor (pool)
        self.a0, self.a3, self.cat, self.pool = {}, {}, {}, {}
        prev = None                                         # stage 3 of the block in front
        for block in BLOCK_ORDER:
            s0, s3 = self.stages[(block, 0)], self.stages[(block, 3)]
            l, c = s0.level, s0.cout
            s0.out = s3.src = self.a0[block] = torch.empty(self.npix[l], c, device=dev, dtype=dt)
            if block in ENCODER:
                self.cat[l] = torch.empty(self.npix[l], 2 * c, device=dev, dtype=dt)
                self.pool[l] = torch.empty(self.npix[l + 1], c, device=dev, dtype=dt)
                s3.out, s3.pooled = self.cat[l][:, c:], self.pool[l]
            else:
                s3.out = self.a3[block] = torch.empty(self.npix[l], c, device=dev, dtype=dt)
            if block.startswith("dec"):
                s0.src, s0.up, s0.up_src, s0.up_out = self.cat[l], self.weights.up[l + 1], prev, self.cat[l][:, :c]
                s0.dx_colsum = s0.up["mod"].bias
            elif prev is not None:                         # enc2..4, bottleneck: the pooled output of the block in front
                s0.src = prev.pooled
            s3.dx_bn = s0
            # stage 3 fed from stage 0's RAW output (encoder and decoder blocks, where the library has the kernels)
            mode = lib.unetdc_conv3x3_bnin_supported(N, *s3.hw, c, c, s3.dil, self.dt) if block != "bottleneck" else 0
            if mode:
                s3.fwd, s3.wgrad = ("bnin", "bnin") if mode == 1 else ("bnin_store", "plain")
                s3.bnin, s0.store = s0, False
            prev = s3
        first = self.stages[(BLOCK_ORDER[0], 0)]
        if lib.unetdc_conv3x3_first_wgrad_bn_supported(N, H, W, first.cin, first.cout, first.dil, self.dt):
            first.wgrad = "first_bn"
        self.last = prev                                    # dec1.3: the head normalises its raw output on load
        self.last.store = False
        self.head_fused = self.oc == 1                      # ... and with one output channel recomputes its input gradient
        # parameter order == model.parameters() order; flat gradient offsets
        self.params = list(self.model.parameters())
        self.pindex = {id(p): i for i, p in enumerate(self.params)}
        offs, o = [], 0
        for p in self.params:
            offs.append(o)
            o += p.numel()
        self.poffs, self.nparams = offs, o
        # workspace: the largest request of the backward calls the plan issues
        need = [1 << 20, lib.unetdc_head_bwd_workspace(N, H, W, self.last.cout, self.oc, self.dt)]
        for st in self.stages.values():
            h, w = st.hw
            need.append(lib.unetdc_conv3x3_first_wgrad_workspace(N, h, w, st.cin, st.cout) if st.first
                        else lib.unetdc_conv3x3_wgrad_workspace(N, h, w, st.cin, st.cout, self.dt))
            need.append(lib.unetdc_bn_relu_bwd_workspace(N, h, w, st.cout, int(st.pooled is not None), self.dt))
            if st.dx_colsum is not None:
                need.append(lib.unetdc_conv3x3_dgrad_colsum_workspace(N, h, w, st.cin))
            if st.up is not None:
                need.append(lib.unetdc_convT2x2_wgrad_workspace(N, *st.up_src.hw, st.up["cin"], st.up["cout"], self.dt))
        self.ws_bytes = int(max(need))
        self.workspace = None          # allocated with the gradient buffers on the first backward
        # Saved-for-backward activations live in this engine's buffers (one set, sized for 288 GB of HBM, nothing is
        # recomputed); `generation` counts forwards so that a backward can tell whether ITS forward's activations
        # are still the ones in the buffers (see _UNetFunction.backward).
        self.generation = 0
        # busy: the activations in the buffers belong to a live autograd graph (set by _UNetFunction.forward, cleared when its
        # backward has run or its graph has been freed); the module gives another forward of this shape its own engine meanwhile
        self.busy = False
        self._busy_gen = -1
        self._rows, self._np = ctypes.c_int(0), ctypes.c_int(0)      # out-parameters of the C ABI (statistics rows that carry data)
        self._flat = None              # flat fp32 gradient buffer, kept across steps (see _flat_grads)

    def saved_bytes(self):
        """Bytes of the activations a forward keeps for its backward."""
        saved = [st.y for st in self.stages.values()] + [*self.a0.values(), *self.a3.values(), *self.cat.values(),
                                                          *self.pool.values()]
        return sum(t.numel() * t.element_size() for t in saved)

    # ------------------------------------------------------------------ forward
    def run(self, x):
        """Called by the nn.Module: returns probabilities [N, OC, H, W] fp32 (autograd aware)."""
        model = self.model
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.params))
        if model.training and not needs_grad:
            # train-mode BatchNorm under no_grad: same arithmetic, nothing saved
            return self.forward(x, train=True)
        if needs_grad:
            # eval mode with gradients enabled (fine-tuning with frozen BatchNorm statistics): the training-path kernels with
            # mean / variance taken from the running buffers, which stay untouched
            return _UNetFunction.apply(x, self, not model.training, *self.params)
        return self.forward(x, train=False)

    def _stage_fwd(self, st, x, train):
        """conv -> BN -> ReLU of one stage in the forms of the plan.  x: the NCHW image (read by the first stage only)."""
        s = _stream()
        N = self.N
        h, w = st.hw
        conv, bn = st.conv, st.bn
        if train:
            y = st.y
            if st.fwd == "first":
                call("unetdc_conv3x3_first_fwd", x.data_ptr(), conv.weight.data_ptr(), conv.bias.data_ptr(),
                     None, None, y.data_ptr(), y.stride(0), st.stats.data_ptr(), N, h, w, st.cin, st.cout,
                     st.dil, self.dt, s)
            elif st.fwd == "plain":
                call("unetdc_conv3x3_fwd", st.src.data_ptr(), st.src.stride(0), st.w_fwd.data_ptr(), conv.bias.data_ptr(),
                     None, None, y.data_ptr(), y.stride(0), st.stats.data_ptr(), _byref(self._rows), N, h, w, st.cin,
                     st.cout, st.dil, self.dt, s)
                st.stat_rows = self._rows.value                         # rows that carry data (<= the sizing bound)
            else:                                  # the RAW output of the stage in front, normalised per staged patch
                p, act = st.bnin, (st.src if st.fwd == "bnin_store" else None)
                call("unetdc_conv3x3_fwd_bnin", p.y.data_ptr(), p.y.stride(0), p.scale.data_ptr(), p.shift.data_ptr(),
                     st.w_fwd.data_ptr(), conv.bias.data_ptr(), y.data_ptr(), y.stride(0), st.stats.data_ptr(), _byref(self._rows),
                     _ptr(act), act.stride(0) if act is not None else 0, N, h, w, st.cin, st.cout, st.dil, self.dt, s)
                st.stat_rows = self._rows.value
            track = bn.track_running_stats and bn.running_mean is not None
            mom = BN_MOMENTUM if bn.momentum is None else bn.momentum
            if self.frozen and track:
                call("unetdc_bn_frozen_affine", bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                     bn.running_var.data_ptr(), bn.eps, st.scale.data_ptr(), st.shift.data_ptr(), st.mean.data_ptr(),
                     st.rstd.data_ptr(), st.cout, s)
            else:                                              # (eval mode without running buffers = batch statistics, as nn.BatchNorm2d)
                call("unetdc_bn_finalize", st.stats.data_ptr(), st.stat_rows, st.npix, bn.weight.data_ptr(),
                     bn.bias.data_ptr(), bn.eps, mom, _ptr(bn.running_mean) if track and not self.frozen else None,
                     _ptr(bn.running_var) if track and not self.frozen else None, st.scale.data_ptr(), st.shift.data_ptr(),
                     st.mean.data_ptr(), st.rstd.data_ptr(), st.cout, s)
            if track and not self.frozen:
                self._nbt.append(bn.num_batches_tracked)       # incremented together at the end of forward()
            if st.store:
                dst, pooled = st.out, st.pooled
                call("unetdc_bn_relu_apply", y.data_ptr(), y.stride(0), st.scale.data_ptr(), st.shift.data_ptr(),
                     dst.data_ptr(), dst.stride(0), _ptr(pooled), pooled.stride(0) if pooled is not None else 0,
                     N, h, w, st.cout, self.dt, s)
        else:
            dst = st.out
            call("unetdc_bn_eval_affine", bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                 bn.running_var.data_ptr(), conv.bias.data_ptr(), bn.eps, st.scale.data_ptr(), st.shift.data_ptr(),
                 st.cout, s)
            if st.first:
                call("unetdc_conv3x3_first_fwd", x.data_ptr(), conv.weight.data_ptr(), None, st.scale.data_ptr(),
                     st.shift.data_ptr(), dst.data_ptr(), dst.stride(0), None, N, h, w, st.cin, st.cout, st.dil,
                     self.dt, s)
            else:
                call("unetdc_conv3x3_fwd", st.src.data_ptr(), st.src.stride(0), st.w_fwd.data_ptr(), None,
                     st.scale.data_ptr(), st.shift.data_ptr(), dst.data_ptr(), dst.stride(0), None, None, N, h, w,
                     st.cin, st.cout, st.dil, self.dt, s)
            if st.pooled is not None:
                call("unetdc_bn_relu_apply", dst.data_ptr(), dst.stride(0), None, None, None, 0,
                     st.pooled.data_ptr(), st.pooled.stride(0), N, h, w, st.cout, self.dt, s)

    def forward(self, x, train, frozen=False):
        """train: the training-path kernels (batch statistics, everything saved for backward); frozen (with train): BatchNorm
        statistics from the running buffers instead of the batch (eval mode under autograd)."""
        self.generation += 1               # every forward overwrites the activation buffers
        self.frozen = bool(frozen)
        self.weights.ensure(need_dgrad=train)
        self._nbt = []
        s = _stream()
        N = self.N
        for st in self.stages.values():
            if st.up is not None:
                u, src, up = st.up, st.up_src.out, st.up_out
                call("unetdc_convT2x2_fwd", src.data_ptr(), src.stride(0), u["w_fwd"].data_ptr(), u["mod"].bias.data_ptr(),
                     up.data_ptr(), up.stride(0), N, *st.up_src.hw, u["cin"], u["cout"], self.dt, s)
            self._stage_fwd(st, x, train)
        probs = torch.empty(N, self.oc, self.H, self.W, device=self.device, dtype=torch.float32)
        oc, last = self.model.out_conv, self.last
        if train:
            call("unetdc_head_fwd_bn", last.y.data_ptr(), last.y.stride(0), last.scale.data_ptr(), last.shift.data_ptr(),
                 oc.weight.data_ptr(), oc.bias.data_ptr(), probs.data_ptr(), N, self.H, self.W, last.cout, self.oc, self.dt, s)
        else:
            call("unetdc_head_fwd", last.out.data_ptr(), last.out.stride(0), oc.weight.data_ptr(), oc.bias.data_ptr(),
                 probs.data_ptr(), N, self.H, self.W, last.cout, self.oc, self.dt, s)
        if self._nbt:
            torch._foreach_add_(self._nbt, 1)                  # nn.BatchNorm2d's num_batches_tracked += 1, one launch
        return probs

    # ------------------------------------------------------------------ backward
    def _ensure_grad_bufs(self):
        """Allocate the gradient buffers on the first backward and bind them to the stages.  They mirror the activations:
        da[l] holds the gradient of a level-l block's output, then that of its stage-0 activation; dcat / dpool those of the
        concat and pooled buffers."""
        if self.workspace is not None:
            return
        dev, dt = self.device, self.tdtype
        da, dcat, dpool = {}, {}, {}
        for block in ENCODER + ("bottleneck",):
            l, c = self.stages[(block, 0)].level, self.stages[(block, 0)].cout
            da[l] = torch.empty(self.npix[l], c, device=dev, dtype=dt)
            if block in ENCODER:
                dcat[l] = torch.empty(self.npix[l], 2 * c, device=dev, dtype=dt)
                dpool[l] = torch.empty(self.npix[l + 1], c, device=dev, dtype=dt)
        for st in self.stages.values():
            st.dy = torch.empty(st.npix, st.cout, device=dev, dtype=dt)
        self.workspace = torch.empty(self.ws_bytes, device=dev, dtype=torch.uint8)
        for block in BLOCK_ORDER:
            s0, s3 = self.stages[(block, 0)], self.stages[(block, 3)]
            l, c = s0.level, s0.cout
            s0.g_out = s3.dx = da[l]
            if block in ENCODER:
                s3.g_out, s3.g_pool = dcat[l][:, c:], dpool[l]
                s0.dx = dpool[l - 1] if l else None
            else:
                s3.g_out = da[l]
                s0.dx = dcat[l] if s0.up is not None else dpool[l - 1]
            if s0.up is not None:
                s0.up_dout = dcat[l][:, :c]

    def _flat_grads(self):
        """The flat fp32 gradient buffer of this backward (124 MB for the U-Net-DC).  ONE buffer is kept per engine and handed
        out again when nothing but the engine still refers to its storage -- the usual training loop, where zero_grad() has
        dropped the previous step's ``.grad`` views (train_DC_focal.py:251) -- so that a step never goes back to the caching
        allocator for its largest block.  While anything still views it (gradient accumulation without zero_grad, gradients
        kept by the caller, torch.autograd.grad results) a fresh buffer is allocated instead and becomes the kept one:
        gradients handed out are never overwritten by a later backward."""
        f = self._flat
        if f is not None and _storage_use_count is not None and _storage_use_count(f.untyped_storage()._cdata) <= 2:
            return f                   # 2 = this tensor + the Python storage wrapper of the query
        self._flat = torch.empty(self.nparams, device=self.device, dtype=torch.float32)
        return self._flat

    def _gview(self, flat, p):
        i = self.pindex[id(p)]
        return flat[self.poffs[i]: self.poffs[i] + p.numel()]

    def _bnstats_args(self, st):
        """Arguments describing the stage whose BatchNorm-backward reduction a dgrad epilogue fuses."""
        if st.bwd_parts is None:
            st.bwd_parts = torch.empty(_lib.partial_floats(st.bwd_rows, 3 * st.cout), device=self.device, dtype=torch.float32)
        return (st.y.data_ptr(), st.y.stride(0), st.scale.data_ptr(), st.shift.data_ptr(), st.mean.data_ptr(),
                st.rstd.data_ptr(), st.bwd_parts.data_ptr(), st.bwd_parts.numel(), _byref(self._np))

    def _stage_bwd(self, st, flat, x, head=None):
        """Backward of one stage in the forms of the plan: BatchNorm + ReLU backward into dy, weight gradient, input
        gradient.  x: the forward's NCHW image (the first layer's weight gradient reads it); head: (dprobs, probs, head
        weight) when this stage recomputes the gradient of the head's input instead of reading it."""
        s = _stream()
        N = self.N
        h, w = st.hw
        dy, g = st.dy, st.g_out
        ws, wsb = self.workspace.data_ptr(), self.ws_bytes
        dgamma, dbeta, dbias = (self._gview(flat, p).data_ptr() for p in (st.bn.weight, st.bn.bias, st.conv.bias))
        dw = self._gview(flat, st.conv.weight).data_ptr()
        saved = (st.y.data_ptr(), st.y.stride(0), st.scale.data_ptr(), st.shift.data_ptr(), st.mean.data_ptr(),
                 st.rstd.data_ptr())
        pre = (st.bwd_parts.data_ptr(), st.bwd_nparts) if st.bwd_nparts else (None, 0)
        if st.wgrad == "first_bn" and pre[1] and not self.frozen and not self.need_dx:
            # BatchNorm backward on load of the weight gradient: dy is never written
            if st.bwd_coeffs is None:
                st.bwd_coeffs = torch.empty(3 * st.cout, device=self.device, dtype=torch.float32)
            call("unetdc_bn_relu_bwd_coeffs", *pre, st.bn.weight.data_ptr(), st.rstd.data_ptr(), dgamma, dbeta, dbias,
                 st.bwd_coeffs.data_ptr(), N, h, w, st.cout, s)
            call("unetdc_conv3x3_first_wgrad_bn", x.data_ptr(), g.data_ptr(), g.stride(0), *saved,
                 st.bwd_coeffs.data_ptr(), dw, ws, wsb, N, h, w, st.cin, st.cout, st.dil, self.dt, s)
            return
        if head is not None:
            call("unetdc_bn_relu_bwd_head", *(t.data_ptr() for t in head), *saved, st.bn.weight.data_ptr(), dy.data_ptr(),
                 dy.stride(0), dgamma, dbeta, dbias, ws, wsb, *pre, N, h, w, st.cout, self.dt, s)
        else:
            gp = st.g_pool
            call("unetdc_bn_relu_bwd_frozen" if self.frozen and st.bn.running_mean is not None else "unetdc_bn_relu_bwd",
                 g.data_ptr(), g.stride(0), _ptr(gp), gp.stride(0) if gp is not None else 0, *saved,
                 st.bn.weight.data_ptr(), dy.data_ptr(), dy.stride(0), dgamma, dbeta, dbias, ws, wsb, *pre,
                 N, h, w, st.cout, self.dt, s)
        if st.wgrad == "bnin":
            p = st.bnin
            call("unetdc_conv3x3_wgrad_bnin", p.y.data_ptr(), p.y.stride(0), p.scale.data_ptr(), p.shift.data_ptr(),
                 dy.data_ptr(), dy.stride(0), dw, ws, wsb, N, h, w, st.cin, st.cout, st.dil, self.dt, s)
        elif st.first:
            call("unetdc_conv3x3_first_wgrad", x.data_ptr(), dy.data_ptr(), dy.stride(0), dw, ws, wsb,
                 N, h, w, st.cin, st.cout, st.dil, self.dt, s)
        else:
            call("unetdc_conv3x3_wgrad", st.src.data_ptr(), st.src.stride(0), dy.data_ptr(), dy.stride(0), dw,
                 ws, wsb, N, h, w, st.cin, st.cout, st.dil, self.dt, s)
        dx = st.dx
        if st.dx_bn is not None:
            call("unetdc_conv3x3_dgrad_bnstats", dy.data_ptr(), dy.stride(0), st.w_dgrad.data_ptr(),
                 dx.data_ptr(), dx.stride(0), *self._bnstats_args(st.dx_bn), N, h, w, st.cin, st.cout,
                 st.dil, self.dt, s)
            st.dx_bn.bwd_nparts = self._np.value
        elif st.dx_colsum is not None:
            call("unetdc_conv3x3_dgrad_colsum", dy.data_ptr(), dy.stride(0), st.w_dgrad.data_ptr(), dx.data_ptr(),
                 dx.stride(0), self._gview(flat, st.dx_colsum).data_ptr(), 0, st.cout, ws, wsb, N, h, w, st.cin, st.cout,
                 st.dil, self.dt, s)
        elif dx is not None:
            call("unetdc_conv3x3_dgrad", dy.data_ptr(), dy.stride(0), st.w_dgrad.data_ptr(), dx.data_ptr(),
                 dx.stride(0), N, h, w, st.cin, st.cout, st.dil, self.dt, s)

    def _notify(self, flat, mods):
        """Tell the data-parallel wrapper that the gradients of `mods` (adjacent in parameters() order) are enqueued."""
        hook = self.model.grad_ready_hook
        if hook is not None:
            ps = [q for m in mods for q in m.parameters()]
            lo = self.poffs[self.pindex[id(ps[0])]]
            hi = self.poffs[self.pindex[id(ps[-1])]] + ps[-1].numel()
            assert hi - lo == sum(q.numel() for q in ps), "gradient ranges must be contiguous in the flat buffer"
            hook(flat, lo, hi)

    def input_grad(self):
        """dL/dx [N, C_in, H, W] fp32 of the backward that has just been enqueued: the first convolution's dgrad from the
        gradient of its output (kept in the stage's dy buffer).  Only computed when the input requires a gradient."""
        st = self.stages[(BLOCK_ORDER[0], 0)]
        dx = torch.empty(self.N, self.cin, self.H, self.W, device=self.device, dtype=torch.float32)
        call("unetdc_conv3x3_first_dgrad", st.dy.data_ptr(), st.dy.stride(0), st.conv.weight.data_ptr(), dx.data_ptr(), self.N,
             self.H, self.W, self.cin, st.cout, st.dil, self.dt, _stream())
        return dx

    def backward(self, dprobs, x, probs, need_dx=False):
        """dprobs, probs: [N, OC, H, W] fp32; x: the forward's input.  Returns the flat fp32 gradient buffer (parameters()
        order).  need_dx: input_grad() will be called afterwards (the first stage then keeps its dy)."""
        self._ensure_grad_bufs()
        self.need_dx = bool(need_dx)
        s = _stream()
        N = self.N
        ws, wsb = self.workspace.data_ptr(), self.ws_bytes
        flat = self._flat_grads()
        dprobs = dprobs.contiguous()
        oc, last = self.model.out_conv, self.last
        # batch statistics: the fused head applies, the head's input gradient is never stored (dec1.3 recomputes it)
        head = (dprobs, probs, oc.weight) if self.head_fused and not self.frozen else None
        # the BatchNorm-backward sums of dec1.3 come out of the same pass
        call("unetdc_head_bwd_bnstats", dprobs.data_ptr(), probs.data_ptr(), None, last.cout, oc.weight.data_ptr(),
             None if head is not None else last.g_out.data_ptr(), last.g_out.stride(0),
             self._gview(flat, oc.weight).data_ptr(), self._gview(flat, oc.bias).data_ptr(), ws, wsb,
             *self._bnstats_args(last), N, self.H, self.W, last.cout, self.oc, self.dt, s)
        last.bwd_nparts = self._np.value
        self._notify(flat, [oc])
        for st in reversed(self.stages.values()):
            self._stage_bwd(st, flat, x, head if st is last else None)
            self._notify(flat, [st.conv, st.bn])     # per STAGE: bottleneck.3's 37.7 MB travel while bottleneck.0 computes
            if st.up is not None:                    # the up-convolution in front of a decoder block
                u, p, dup = st.up, st.up_src, st.up_dout
                h, w = p.hw
                call("unetdc_convT2x2_wgrad", p.out.data_ptr(), p.out.stride(0), dup.data_ptr(), dup.stride(0),
                     self._gview(flat, u["mod"].weight).data_ptr(), ws, wsb, N, h, w, u["cin"], u["cout"], self.dt, s)
                call("unetdc_convT2x2_dgrad_bnstats", dup.data_ptr(), dup.stride(0), u["w_dgrad"].data_ptr(),
                     p.g_out.data_ptr(), p.g_out.stride(0), *self._bnstats_args(p), N, h, w, u["cin"], u["cout"], self.dt, s)
                p.bwd_nparts = self._np.value
                self._notify(flat, [u["mod"]])
        return flat


def _release_engine(ref, generation):
    eng = ref()
    if eng is not None and eng.busy and eng._busy_gen == generation:
        eng.busy = False


class _UNetFunction(torch.autograd.Function):
    """Autograd boundary: one node for the whole network (forward kernels / backward kernels)."""

    @staticmethod
    def forward(ctx, x, engine, frozen, *params):
        probs = engine.forward(x, train=True, frozen=frozen)
        ctx.engine = engine
        ctx.generation = engine.generation
        engine.busy, engine._busy_gen = True, engine.generation
        # a forward that is never back-propagated releases its engine when its graph is freed
        import weakref
        weakref.finalize(ctx, _release_engine, weakref.ref(engine), engine.generation)
        # x (read by the first layer's weight gradient) and probs (read by the head backward) go through autograd's
        # saved-tensor machinery so that an in-place edit of either between forward and backward is detected
        ctx.save_for_backward(x, probs)
        return probs

    @staticmethod
    def backward(ctx, dprobs):
        eng = ctx.engine
        if eng.generation != ctx.generation:
            raise _lib.UnetdcError(
                "backward through a U-Net forward whose saved activations were overwritten by a later forward of "
                "the same module (forward #%d, buffers now hold #%d): the HIP path keeps ONE set of activation "
                "buffers per module, so run backward before the next forward (train or eval) of that module"
                % (ctx.generation, eng.generation))
        x, probs = ctx.saved_tensors
        flat = eng.backward(dprobs, x, probs, need_dx=ctx.needs_input_grad[0])
        finish = eng.model.grad_sync_finish
        if finish is not None:           # data parallel: wait (stream-side) for the bucket all-reduces
            finish()
        grads = []
        for p, o in zip(eng.params, eng.poffs):
            grads.append(flat[o:o + p.numel()].view_as(p) if p.requires_grad else None)
        dx = eng.input_grad() if ctx.needs_input_grad[0] else None
        # the gradients are enqueued: the next forward may take the buffers (a SECOND backward through a retained graph stays
        # possible as long as no forward has used them in between -- the generation check above says so otherwise)
        _release_engine(lambda: eng, ctx.generation)
        return (dx, None, None, *grads)
