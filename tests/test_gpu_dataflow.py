"""Teacher-forced, stage-by-stage test of the HIP step's dataflow (tests/dataflow_ref.py states the graph and the bounds).

A tracer wraps the ``call`` binding of engine.py and loss.py for one test.  After every call it synchronises, labels each
output region with the MODEL-LEVEL value it holds (by matching it against the engine's named buffers: a stage's ``y``,
``scale``, activation, concat halves, pooled copy, ``dy``, the flat-gradient view of a parameter, ...), snapshots it, and
compares it with the fp64 reference computed from the snapshots of the values the MODEL says feed it -- never from the
pointers the call was given.  The bound stays a few ulps deep in the network, so a wrong, stale or swapped input shows.
Values the plan never materialises (an activation normalised on load, the fused head's input gradient, the first stage's
dy under its BatchNorm-on-load weight gradient) are derived from their own sources.  Every write must land in a labelled
region or a declared scratch region, every value of the step must be produced exactly once (or be one of those derived
ones), and every call must be checked or exempt with a reason."""
import collections
import time

import pytest
import torch

from tests import dataflow_ref as R
from tests import exact_ref as X

pytestmark = pytest.mark.gpu

# what each symbol writes (the header's parameter names); everything else it is given is read
OUTPUTS = {
    "unetdc_conv3x3_fwd": ("y", "stats_part"), "unetdc_conv3x3_fwd_bnin": ("y", "stats_part", "act_out"),
    "unetdc_conv3x3_first_fwd": ("y", "stats_part"),
    "unetdc_bn_finalize": ("running_mean", "running_var", "scale", "shift", "mean", "rstd"),
    "unetdc_bn_eval_affine": ("scale", "shift"), "unetdc_bn_frozen_affine": ("scale", "shift", "mean", "rstd"),
    "unetdc_bn_relu_apply": ("a", "pooled"), "unetdc_convT2x2_fwd": ("up",),
    "unetdc_head_fwd": ("probs",), "unetdc_head_fwd_bn": ("probs",),
    "unetdc_focal_dice_loss_fwd": ("loss_out", "coef", "workspace"), "unetdc_focal_dice_loss_bwd": ("dprobs",),
    "unetdc_head_bwd_bnstats": ("da", "dw", "db", "workspace", "parts"),
    "unetdc_bn_relu_bwd": ("dy", "dgamma", "dbeta", "dbias", "workspace"),
    "unetdc_bn_relu_bwd_frozen": ("dy", "dgamma", "dbeta", "dbias", "workspace"),
    "unetdc_bn_relu_bwd_head": ("dy", "dgamma", "dbeta", "dbias", "workspace"),
    "unetdc_bn_relu_bwd_coeffs": ("dgamma", "dbeta", "dbias", "coeffs"),
    "unetdc_conv3x3_first_wgrad_bn": ("dw", "workspace"), "unetdc_conv3x3_first_wgrad": ("dw", "workspace"),
    "unetdc_conv3x3_wgrad": ("dw", "workspace"), "unetdc_conv3x3_wgrad_bnin": ("dw", "workspace"),
    "unetdc_conv3x3_dgrad": ("dx",), "unetdc_conv3x3_dgrad_bnstats": ("dx", "parts"),
    "unetdc_conv3x3_dgrad_colsum": ("dx", "colsum", "workspace"), "unetdc_conv3x3_first_dgrad": ("dx_nchw",),
    "unetdc_convT2x2_wgrad": ("dw", "workspace"), "unetdc_convT2x2_dgrad_bnstats": ("dx", "parts"),
}
LD_OF = {"y": "ldy", "act_out": "ldact", "a": "lda", "pooled": "ldp", "up": "ldup", "da": "ldda", "dy": "lddy", "dx": "lddx"}
# symbols a traced step issues that are not checked here, with the reason and the test that covers them
EXEMPT = {
    "unetdc_pack_many": "re-packs the weight images the references read as the storage rounding of the parameters: "
                        "tests/test_gpu_ops.py::test_pack_many_matches_per_layer_packers",
    "unetdc_adam_step": "the optimizer step: fp64-bounded p, m, v and bit-exact packed images in tests/test_gpu_exact_optim.py; "
                        "its result reaches every reference of the next step through the parameter snapshots",
}
# symbols whose output is a tensor the caller allocates per call (not an engine buffer): role, and the value it holds
FRESH = {"unetdc_head_fwd": "probs", "unetdc_head_fwd_bn": "probs", "unetdc_focal_dice_loss_fwd": "loss_out",
         "unetdc_focal_dice_loss_bwd": "dprobs", "unetdc_conv3x3_first_dgrad": "dx_nchw"}
FRESH_NAME = {"unetdc_head_fwd": "probs", "unetdc_head_fwd_bn": "probs", "unetdc_focal_dice_loss_fwd": "loss",
              "unetdc_focal_dice_loss_bwd": "dprobs", "unetdc_conv3x3_first_dgrad": "dx"}
WORST = {}                                 # config -> {value kind: worst err / bound}


def kind(name):
    """Value kind for the margin report: the name without its stage."""
    if name.startswith("G:"):
        return "G:" + name.rsplit(".", 1)[1] + ("(bn)" if name.split(".")[1] in ("1", "4") else "")
    head, _, tail = name.rpartition(".")
    return (("g:" if name.startswith("g:") else "") + tail) if head else name


class Tracer:
    def __init__(self, model, dt, dims):
        from unet_dc_segmentation_amd import _lib
        self.lib = _lib.load()
        self.model, self.dt, self.dims = model, dt, dims
        self.g = R.Graph(model)
        self.pnames = [k for k, _ in model.named_parameters()]
        self.store = {}                    # id(engine) -> {value name: snapshot}
        self.derived = {}                  # id(engine) -> {value name: (value, uncertainty)}
        self.produced = {}                 # id(engine) -> Counter of the values of the current step
        self.mode, self.need_dx = {}, {}
        self.cur = None
        self.target = None
        self.issued = collections.Counter()
        self.kernels = set()
        self.forms = set()
        self.failures = []
        self.worst = {}
        self.checked = 0
        self.keep = {}                     # value name -> None: snapshots kept from the previous step (staleness probes)
        self.prev = {}                     # id(engine) -> {value name: (value, uncertainty)} of the previous step
        self.stale = {}                    # value name -> (stale source, fraction of elements out of bound)
        self.pending = {}
        self.probs_ptr = {}                # id(engine) -> data_ptr of the probabilities of its last forward
        self.engines = {}

    # ------------------------------------------------------------------ engine boundaries
    def on_forward(self, eng, x, train, frozen):
        e = id(eng)
        if e in self.store and self.keep:
            self.prev[e] = {k: self.lookup(e, k) for k in set(self.keep.values())}
        self.store[e], self.derived[e], self.produced[e] = {}, {}, collections.Counter()
        self.mode[e] = "eval" if not train else ("frozen" if frozen else "train")
        s = self.store[e]
        s["x"] = x.detach().clone()
        for k, v in self.model.state_dict().items():
            s[f"P:{k}"] = v.detach().clone()
        self.cur = eng

    def on_backward(self, eng, need_dx):
        self.cur = eng
        self.need_dx[id(eng)] = bool(need_dx)

    # ------------------------------------------------------------------ values
    def lookup(self, e, name, stale=None):
        if stale is not None and name == stale[0]:
            return stale[1]
        if stale is None:
            if name in self.store[e]:
                return self.store[e][name], None
            if name in self.derived[e]:
                return self.derived[e][name]
        elif name in self.store[e]:
            return self.store[e][name], None
        v = R.derive(self.g, name, lambda k: self.lookup(e, k, stale), self.dt, self.mode[e], self.dims)
        if stale is None:
            self.derived[e][name] = v
        return v

    # ------------------------------------------------------------------ labels
    def regions(self, eng):
        """(data_ptr, ld or None, value name or 'scratch:...', tensor) of every named buffer of the engine."""
        out = []

        def add(t, name):
            if t is not None:
                out.append((t.data_ptr(), t.stride(0) if t.dim() == 2 else None, name, t))
        for st in eng.stages.values():
            S = st.name
            add(st.y, f"{S}.y")
            for k in ("scale", "shift", "mean", "rstd"):
                add(getattr(st, k), f"{S}.{k}")
            add(st.bn.running_mean, f"{S}.running_mean")
            add(st.bn.running_var, f"{S}.running_var")
            add(st.stats, "scratch:stats")
            add(st.bwd_parts, f"scratch:parts:{S}")
            add(st.bwd_coeffs, "scratch:coeffs")
            add(st.dy, f"{S}.dy")
        for st in self.g.stages:
            es = eng.stages[(st.block, st.idx)]
            if st.idx == 0 and st.src[0] == "cat":
                c = self.g.ups[st.src[1]]["cout"]
                add(es.src[:, :c], st.src[1])
                add(es.src[:, c:], f"{st.src[2]}.a")
                if es.dx is not None:                       # the concat gradient, written whole: both halves at once
                    add(es.dx, f"g:{st.src[1]}|g:{st.src[2][:-2]}.skip")
            if st.idx == 0 and st.src[0] == "pool" and es.dx is not None:
                add(es.dx, f"g:{st.src[1]}.pool")
            if st.idx == 3:
                add(es.src, f"{st.block}.0.a")
                if es.pooled is not None:
                    add(es.pooled, f"{st.block}.pool")
                else:
                    add(es.out, f"{st.name}.a")
                if es.dx is not None:
                    add(es.dx, f"g:{st.block}.0.a")             # da[l]: also g:<B>.3.a below, told apart by the parts
                if es.pooled is None and es.g_out is not None:
                    add(es.g_out, f"g:{st.name}.a")
        if eng.workspace is not None:
            add(eng.workspace, "scratch:workspace")
        return out

    def grad_name(self, eng, ptr):
        flat = eng._flat
        if flat is None:
            return None
        off = (ptr - flat.data_ptr())
        if off < 0 or off >= flat.numel() * 4 or off % 4:
            return None
        off //= 4
        for name, p, o in zip(self.pnames, eng.params, eng.poffs):
            if o == off:
                return f"G:{name}", flat[o:o + p.numel()]
        return None

    def label(self, sym, kw):
        """[(value name, tensor)] of the call's outputs; raises on a write to an unnamed region."""
        eng = self.cur
        regs = self.regions(eng)
        parts = kw.get("ptr:parts")
        owner = next((n.split(":")[2] for p, _, n, _ in regs if p == parts and n.startswith("scratch:parts:")), None)
        out = []
        for role in OUTPUTS[sym]:
            ptr = kw.get("ptr:" + role)
            if not ptr:
                continue
            g = self.grad_name(eng, ptr)
            if g is not None:
                out.append(g)
                continue
            ld = kw.get(LD_OF.get(role, ""), None)
            hits = [(n, t) for p, l, n, t in regs if p == ptr and (ld is None or l is None or l == ld)]
            if len(hits) > 1:                               # da[l]: the gradient of stage 0's or stage 3's activation
                hits = [(n, t) for n, t in hits if n == f"g:{owner}.a"]
            if len(hits) != 1:
                raise AssertionError(f"{sym}: output {role} at {ptr:#x} (ld {ld}) lands in no named region: {hits}")
            name, t = hits[0]
            if "|" in name:
                c = t.shape[1] // 2
                out += [(name.split("|")[0], t[:, :c]), (name.split("|")[1], t[:, c:])]
            else:
                out.append(hits[0])
        return out

    # ------------------------------------------------------------------ the wrapped binding
    def call(self, orig, sym, *args):
        from unet_dc_segmentation_amd import _lib
        self.issued[sym] += 1
        kw = {}
        if sym in X.ARGS:
            kinds = X.arg_kinds(_lib.SIGNATURES[sym][1])
            for key, i in X.positions(sym, kinds).items():
                kw[key] = args[i]
        orig(sym, *args)
        if sym in EXEMPT:
            return
        torch.cuda.synchronize()
        if "conv" in sym:                  # (the elementwise / reduction kernels name no matrix-core kernel)
            self.kernels.add(f"{sym}|{self.lib.unetdc_last_kernel().decode()}")
        self.forms.add(sym)
        if sym == "unetdc_conv3x3_fwd_bnin":
            self.forms.add("bnin_store" if kw.get("ptr:act_out") else "bnin")
        if sym in FRESH:                   # outputs in tensors the caller allocates: checked where they are returned
            self.pending[sym] = kw["ptr:" + FRESH[sym]]
            return
        e = id(self.cur)
        outs = [(n, t) for n, t in self.label(sym, kw) if not n.startswith("scratch:")]
        self.produce(e, outs)

    def produce(self, e, outs):
        for n, t in outs:
            self.store[e][n] = t.detach().clone()
            self.produced[e][n] += 1
        names = [n for n, _ in outs]
        refs = R.reference(self.g, names, lambda k: self.lookup(e, k), self.dt, self.mode[e], self.dims)
        for n in names:
            self.compare(n, refs[n], self.store[e][n])
            if n in self.keep and e in self.prev:
                self.stale_probe(e, n)

    def fresh(self, sym, t, e=None):
        """The output of a FRESH symbol, as returned to its caller: the same storage the call wrote."""
        ptr = self.pending.pop(sym)
        assert ptr == t.data_ptr(), (sym, ptr, t.data_ptr())
        self.produce(id(self.cur) if e is None else e, [(FRESH_NAME[sym], t)])

    def compare(self, name, rb, got):
        ref, bnd = rb
        dt = got.dtype
        bad = X.within_bound(got, ref, bnd, dt)
        g64 = got.to(torch.float64).reshape(ref.shape)
        ratio = float(((g64 - ref).abs() / (bnd + R.unit(dt) * ref.abs() + 2.0 ** -126)).max()) if ref.numel() else 0.0
        k = kind(name)
        self.worst[k] = max(self.worst.get(k, 0.0), ratio)
        self.checked += 1
        nb = int(bad.sum())
        if nb:
            idx = tuple(int(i) for i in bad.nonzero()[0])
            self.failures.append(f"{name}: {nb} of {bad.numel()} out of bound; first at {idx}: got "
                                 f"{float(g64[idx]):.6g}, ref {float(ref[idx]):.6g}, bound {float(bnd.expand(ref.shape)[idx]):.3g}")

    def stale_probe(self, e, name):
        src = self.keep[name]
        old = self.prev[e][src]
        ref, bnd = R.reference(self.g, [name], lambda k: self.lookup(e, k, (src, old)), self.dt, self.mode[e], self.dims)[name]
        bad = X.within_bound(self.store[e][name], ref, bnd, self.store[e][name].dtype)
        self.stale[name] = (src, float(bad.double().mean()))

    def owner_of_probs(self, ptr):
        return next(e for e, p in self.probs_ptr.items() if p == ptr)

    # ------------------------------------------------------------------ step bookkeeping
    def end_step(self, eng, trained):
        e = id(eng)
        mode = self.mode[e]
        want = self.g.forward_values(mode)
        if trained:
            want = want + ["loss", "dprobs"] + self.g.backward_values(self.need_dx.get(e, False))
        got = self.produced[e]
        twice = sorted(k for k, v in got.items() if v > 1)
        assert not twice, f"values produced more than once in one step: {twice}"
        missing = [k for k in want if k not in got]
        derivable = {f"{b}.0.a" for b in self.g.encoders} | {f"dec{i}.0.a" for i in range(1, 5)}
        if mode != "eval":
            derivable |= {f"{self.g.last}.a", f"g:{self.g.last}.a", f"{self.g.stages[0].name}.dy"}
        bad = [k for k in missing if k not in derivable]
        assert not bad, f"values of the step never produced: {bad}"
        extra = sorted(k for k in got if k not in want)
        assert not extra, f"values outside the graph: {extra}"
        return missing


@pytest.fixture
def tracer(monkeypatch):
    """Install the tracer around engine.py's and loss.py's call binding, the engine's forward / backward / input_grad and the
    fused loss's autograd function (where the tensors the loss kernels write are returned)."""
    from unet_dc_segmentation_amd import engine, loss

    def make(model, dt, dims):
        tr = Tracer(model, dt, dims)
        orig_call = engine.call

        def traced(sym, *args):
            return tr.call(orig_call, sym, *args)
        monkeypatch.setattr(engine, "call", traced)
        monkeypatch.setattr(loss, "call", traced)
        fwd, bwd, igrad = engine.UNetEngine.forward, engine.UNetEngine.backward, engine.UNetEngine.input_grad

        def forward(self, x, train, frozen=False):
            tr.on_forward(self, x, train, frozen)
            probs = fwd(self, x, train, frozen)
            tr.cur = self
            tr.probs_ptr[id(self)], tr.engines[id(self)] = probs.data_ptr(), self
            tr.fresh("unetdc_head_fwd_bn" if "unetdc_head_fwd_bn" in tr.pending else "unetdc_head_fwd", probs)
            return probs

        def backward(self, dprobs, x, probs, need_dx=False):
            tr.on_backward(self, need_dx)
            return bwd(self, dprobs, x, probs, need_dx)

        def input_grad(self):
            tr.cur = self
            dx = igrad(self)
            tr.fresh("unetdc_conv3x3_first_dgrad", dx)
            return dx
        monkeypatch.setattr(engine.UNetEngine, "forward", forward)
        monkeypatch.setattr(engine.UNetEngine, "backward", backward)
        monkeypatch.setattr(engine.UNetEngine, "input_grad", input_grad)
        lf, lb = loss._FocalDice.forward, loss._FocalDice.backward

        def loss_fwd(ctx, pred, target, *rest):
            e = tr.owner_of_probs(pred.data_ptr())
            tr.cur = tr.engines[e]
            tr.store[e]["target"] = target.detach().clone()
            out = lf(ctx, pred, target, *rest)
            tr.fresh("unetdc_focal_dice_loss_fwd", out, e)
            ctx.tracer_engine = e
            return out

        def loss_bwd(ctx, gout):
            e = ctx.tracer_engine
            tr.cur = tr.engines[e]
            assert float(gout) == 1.0, "the references assume d loss = 1"
            res = lb(ctx, gout)
            tr.fresh("unetdc_focal_dice_loss_bwd", res[0], e)
            return res
        monkeypatch.setattr(loss._FocalDice, "forward", staticmethod(loss_fwd))
        monkeypatch.setattr(loss._FocalDice, "backward", staticmethod(loss_bwd))
        return tr
    yield make


# ---------------------------------------------------------------------------------------------------- configurations
def make_model(arch, cin, dtype, perturb=False):
    from models.model import UNet
    from models.model_2 import UNetDC
    from oracle import recipe
    torch.manual_seed(5)
    model = (UNetDC if arch == "unetdc" else UNet)(cin, 1)
    if perturb:                                    # non-trivial running statistics for the eval / frozen forms
        sd = model.state_dict()
        recipe.perturb_bn(sd, 11)
        model.load_state_dict(sd)
    model = model.cuda()
    if dtype == "bf16":
        model.set_compute_dtype("bf16")
    return model


def batch(seed, n, cin, size):
    from oracle import recipe
    x = recipe.seeded_input(seed, (n, cin, size, size)).cuda()
    t = recipe.seeded_target(seed + 1, (n, 1, size, size), frac=0.1).cuda()
    return x, t


def report(config, tr, t0):
    WORST[config] = dict(tr.worst)
    print(f"\n[{config}] {tr.checked} values checked in {time.time() - t0:.1f} s; calls: {dict(sorted(tr.issued.items()))}")
    print(f"[{config}] forms: {sorted(f for f in tr.forms if not f.startswith('unetdc_'))}")
    print(f"[{config}] kernels: {sorted(tr.kernels)}")
    print(f"[{config}] worst err / bound per value kind: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(tr.worst.items())))
    for name, (src, frac) in sorted(tr.stale.items()):
        print(f"[{config}] stale {src} -> {name}: {frac:.3f} of the elements out of bound")
    unchecked = sorted(s for s in tr.issued if s not in OUTPUTS and s not in EXEMPT)
    assert not unchecked, f"calls neither checked nor exempt: {unchecked}"
    assert not tr.failures, f"{len(tr.failures)} values out of bound:\n" + "\n".join(tr.failures[:40])


def train_step(model, tr, x, t, opt=None):
    from utils.metrics_DC import focal_dice_loss
    tr.target = t
    p = model(x)
    focal_dice_loss(p, t, alpha=1.0, gamma=2.0, ratio=0.3).backward()
    if opt is not None:
        opt.step()
    eng = tr.engines[tr.owner_of_probs(p.data_ptr())]
    return tr.end_step(eng, trained=True)


# the stale-source probes of the two-step config: value checked at step 2 -> the source taken from step 1 instead
STALE = {"enc1.3.y": "enc1.0.scale",            # normalise-on-load forward reads stage 0's constants
         "G:enc1.3.weight": "enc1.0.shift",     # ... and so does its weight gradient
         "dec1.3.y": "dec1.0.y",
         "G:dec1.3.weight": "dec1.0.y",         # the decoder's raw output, not another stage's of the same shape
         "G:enc2.3.weight": "enc2.0.a",         # the plain weight gradient after a forward that writes the activation back
         "G:enc1.0.weight": "g:enc1.0.a",       # BatchNorm backward on load in the first layer's weight gradient
         "probs": "dec1.3.scale"}               # the head normalises dec1.3's raw output on load
# A stale source must put a clear share of its consumer's elements out of bound (one is enough to fail the test).  Measured:
# >= 0.9 for every probe but the first layer's weight gradient under BatchNorm-on-load (about 0.08): its dy is never stored,
# so its reference carries the bf16 rounding of every dy term as a worst-case uncertainty.
STALE_MIN = 0.05


def test_dataflow_bf16_two_steps(tracer):
    """UNetDC(1, 1), bf16, 8 x 512^2, two FusedAdam steps; step 2 checked in full, with stale-source probes.  lr = 1e-2:
    one Adam step then moves every weight by about 1e-2, far more than a bf16 ulp of the smallest layers' weights, so the
    step-1 values are far from the step-2 ones everywhere (at the default 1e-3 the first layer's nine weights move by
    about a quarter of a bf16 ulp of its output and a stale copy would pass)."""
    from unet_dc_segmentation_amd.optim import FusedAdam
    t0 = time.time()
    model = make_model("unetdc", 1, "bf16").train()
    tr = tracer(model, torch.bfloat16, (8, 512, 512))
    opt = FusedAdam(model, lr=1e-2)
    x1, t1 = batch(20, 8, 1, 512)
    train_step(model, tr, x1, t1, opt)
    kept = [p.grad for p in model.parameters()]
    copies = [g.clone() for g in kept]
    model.zero_grad(set_to_none=True)
    tr.keep = dict(STALE)
    x2, t2 = batch(22, 8, 1, 512)
    derived = train_step(model, tr, x2, t2, opt)
    torch.cuda.synchronize()
    # the reused flat gradient buffer never overwrites gradients a caller still holds
    for p, g, c in zip(model.parameters(), kept, copies):
        assert torch.equal(g, c), "a kept step-1 gradient changed during step 2"
    print(f"\nnever materialised (derived): {sorted(derived)}")
    report("bf16_two_steps", tr, t0)
    assert {"bnin", "bnin_store", "unetdc_conv3x3_wgrad_bnin", "unetdc_conv3x3_first_wgrad_bn", "unetdc_bn_relu_bwd_coeffs",
            "unetdc_bn_relu_bwd_head", "unetdc_head_fwd_bn", "unetdc_conv3x3_dgrad_bnstats", "unetdc_conv3x3_dgrad_colsum",
            "unetdc_convT2x2_dgrad_bnstats", "unetdc_conv3x3_fwd", "unetdc_conv3x3_wgrad"} <= tr.forms, sorted(tr.forms)
    assert set(STALE) <= set(tr.stale), sorted(tr.stale)
    weak = {k: v for k, v in tr.stale.items() if v[1] < STALE_MIN}
    assert not weak, f"stale sources the check cannot tell from current ones: {weak}"


def test_dataflow_bf16_dx_three_channels(tracer):
    """UNetDC(3, 1) with x.requires_grad: the plain first-layer weight gradient, first_dgrad and dL/dx."""
    t0 = time.time()
    model = make_model("unetdc", 3, "bf16").train()
    tr = tracer(model, torch.bfloat16, (8, 512, 512))
    x, t = batch(30, 8, 3, 512)
    x.requires_grad_()
    train_step(model, tr, x, t)
    report("bf16_dc3_dx", tr, t0)
    assert {"unetdc_conv3x3_first_wgrad", "unetdc_conv3x3_first_dgrad"} <= tr.forms


def test_dataflow_bf16_unet(tracer):
    """UNet(3, 1) (bench.py --arch unet): every dilation 1."""
    t0 = time.time()
    model = make_model("unet", 3, "bf16").train()
    tr = tracer(model, torch.bfloat16, (8, 512, 512))
    x, t = batch(40, 8, 3, 512)
    train_step(model, tr, x, t)
    report("bf16_unet3", tr, t0)


def test_dataflow_bf16_frozen(tracer):
    """UNetDC(1, 1) in eval mode under autograd: frozen statistics, the unfused head backward."""
    t0 = time.time()
    model = make_model("unetdc", 1, "bf16", perturb=True).eval()
    tr = tracer(model, torch.bfloat16, (8, 512, 512))
    x, t = batch(50, 8, 1, 512)
    train_step(model, tr, x, t)
    report("bf16_frozen", tr, t0)
    assert {"unetdc_bn_frozen_affine", "unetdc_bn_relu_bwd_frozen"} <= tr.forms


def test_dataflow_bf16_eval_quantify(tracer):
    """UNetDC(3, 1) eval forward under no_grad (bench.py --mode quantify): folded statistics, pool-only normalisation pass."""
    t0 = time.time()
    model = make_model("unetdc", 3, "bf16", perturb=True).eval()
    tr = tracer(model, torch.bfloat16, (8, 512, 512))
    x, _ = batch(60, 8, 3, 512)
    with torch.no_grad():
        p = model(x)
    tr.end_step(tr.engines[tr.owner_of_probs(p.data_ptr())], trained=False)
    report("bf16_eval", tr, t0)
    assert {"unetdc_bn_eval_affine", "unetdc_head_fwd", "unetdc_bn_relu_apply"} <= tr.forms


def test_dataflow_bf16_two_live_forwards(tracer):
    """Two live training forwards of different inputs, an eval forward between them, then both backwards in reverse order:
    each backward is checked against its own forward's values."""
    from utils.metrics_DC import focal_dice_loss
    t0 = time.time()
    model = make_model("unetdc", 1, "bf16").train()
    tr = tracer(model, torch.bfloat16, (8, 512, 512))
    (x1, t1), (xe, _), (x2, t2) = batch(70, 8, 1, 512), batch(72, 8, 1, 512), batch(74, 8, 1, 512)
    p1 = model(x1)
    e1 = tr.engines[tr.owner_of_probs(p1.data_ptr())]
    tr.target = t1
    l1 = focal_dice_loss(p1, t1, alpha=1.0, gamma=2.0, ratio=0.3)
    model.eval()
    with torch.no_grad():
        pe = model(xe)
    tr.end_step(tr.engines[tr.owner_of_probs(pe.data_ptr())], trained=False)
    model.train()
    p2 = model(x2)
    e2 = tr.engines[tr.owner_of_probs(p2.data_ptr())]
    assert e1 is not e2
    tr.target = t2
    l2 = focal_dice_loss(p2, t2, alpha=1.0, gamma=2.0, ratio=0.3)
    l2.backward()
    tr.end_step(e2, trained=True)
    l1.backward()
    tr.end_step(e1, trained=True)
    report("bf16_two_live", tr, t0)


def test_dataflow_fp32_self_test(tracer):
    """The harness on the fp32 path, which the suite already verifies tightly: UNetDC(1, 1), 2 x 512^2."""
    t0 = time.time()
    model = make_model("unetdc", 1, "f32").train()
    tr = tracer(model, torch.float32, (2, 512, 512))
    x, t = batch(80, 2, 1, 512)
    train_step(model, tr, x, t)
    report("f32_self_test", tr, t0)
