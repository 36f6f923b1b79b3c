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
        self.calls_at = {}                 # (symbol, h, w of the call) -> kernel names it reached ('' where it names none)
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
        if "h" in kw and "w" in kw:
            self.calls_at.setdefault((sym, kw["h"], kw["w"]), set()).add(
                self.lib.unetdc_last_kernel().decode() if "conv" in sym else "")
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
def make_model(arch, cin, dtype, perturb=False, oc=1):
    from models.model import UNet
    from models.model_2 import UNetDC
    from oracle import recipe
    torch.manual_seed(5)
    model = (UNetDC if arch == "unetdc" else UNet)(cin, oc)
    if perturb:                                    # non-trivial running statistics for the eval / frozen forms
        sd = model.state_dict()
        recipe.perturb_bn(sd, 11)
        model.load_state_dict(sd)
    model = model.cuda()
    if dtype == "bf16":
        model.set_compute_dtype("bf16")
    return model


def batch(seed, n, cin, size, oc=1):
    """size: the side of a square image, or (H, W)."""
    from oracle import recipe
    h, w = (size, size) if isinstance(size, int) else size
    x = recipe.seeded_input(seed, (n, cin, h, w)).cuda()
    t = recipe.seeded_target(seed + 1, (n, oc, h, w), frac=0.1).cuda()
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


def eval_quantify(tracer, config, n=8, size=512, seed=60):
    """One traced bf16 eval forward of UNetDC(3, 1) under no_grad on n images of size x size."""
    t0 = time.time()
    model = make_model("unetdc", 3, "bf16", perturb=True).eval()
    tr = tracer(model, torch.bfloat16, (n, size, size))
    x, _ = batch(seed, n, 3, size)
    with torch.no_grad():
        p = model(x)
    tr.end_step(tr.engines[tr.owner_of_probs(p.data_ptr())], trained=False)
    report(config, tr, t0)
    assert {"unetdc_bn_eval_affine", "unetdc_head_fwd", "unetdc_bn_relu_apply"} <= tr.forms
    return tr


def test_dataflow_bf16_eval_quantify(tracer):
    """UNetDC(3, 1) eval forward under no_grad (bench.py --mode quantify): folded statistics, pool-only normalisation pass."""
    eval_quantify(tracer, "bf16_eval")


def test_dataflow_bf16_eval_tile_2x48(tracer):
    """The same eval forward at 2 x 48^2 (quantify_droplets_batch.py --tile 48 --dtype bf16, the ragged last chunk of a 4 + 2
    tile plan): the folded-BatchNorm, affine-ReLU epilogue on the small routes -- a 3 x 3 bottleneck under dilation 16 (the
    centre tap only), 6 x 6 maps under dilation 8, M = 18 at the bottleneck (no 16-row tile route).  Measured on MI355X, worst
    err / bound: 0.993 (activations and up-convolutions), probabilities 0.11."""
    tr = eval_quantify(tracer, "bf16_eval_2x48", n=2, size=48, seed=62)
    eng = next(iter(tr.engines.values()))
    assert eng.npix[-1] == 18 and eng.res[-1] == (3, 3), (eng.npix, eng.res)
    at18 = {k[0]: sorted(v) for k, v in tr.calls_at.items() if (k[1], k[2]) == (3, 3) and "conv" in k[0]}
    print(f"[bf16_eval_2x48] kernels on the 3 x 3 maps: {at18}")
    assert {"unetdc_conv3x3_fwd", "unetdc_convT2x2_fwd"} <= set(at18), at18
    for sym, names in at18.items():                # M % 16 != 0: plan_igemm leaves dma16; lattice and halo need whole tiles
        for name in names:
            assert not any(t in name for t in ("dma16", "16x16x32", "lattice", "halo")), (sym, name)


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


# ---------------------------------------------------------------------------------------------------- off the production shape
PRODUCTION = {}                            # (arch, cin) -> (per-stage plan, forms, kernels) of one 8 x 512^2 bf16 training step


def stage_plan(eng):
    """The decisions UNetEngine._build took: per stage (forward form, weight-gradient form, activation stored), the head."""
    plan = {f"{b}.{i}": (st.fwd, st.wgrad, bool(st.store)) for (b, i), st in eng.stages.items()}
    plan["head_fused"] = bool(eng.head_fused)
    return plan


def production_plan(arch, cin):
    """Plan, forms and kernels of the 8 x 512^2 bf16 training step of the one-output-channel model (no tracer: the recorded
    calls of one step, as tests/test_gpu_exact.py::record_step takes them)."""
    if (arch, cin) not in PRODUCTION:
        from unet_dc_segmentation_amd import _lib, engine
        from utils.metrics_DC import focal_dice_loss
        model = make_model(arch, cin, "bf16").train()
        x, t = batch(20, 8, cin, 512)
        plan = stage_plan(engine.UNetEngine(model, x))
        _lib.start_timing(_lib.SIGNATURES)
        try:
            focal_dice_loss(model(x), t, alpha=1.0, gamma=2.0, ratio=0.3).backward()
        finally:
            recs = _lib.stop_timing()
        forms, kernels = set(), set()
        for name_kernel, args, _ in recs:
            sym = name_kernel.split("|", 1)[0]
            if sym in EXEMPT:
                continue
            forms.add(sym)
            if "conv" in sym:
                kernels.add(name_kernel)
            if sym == "unetdc_conv3x3_fwd_bnin":
                pos = X.positions(sym, X.arg_kinds(_lib.SIGNATURES[sym][1]))
                forms.add("bnin_store" if args[pos["ptr:act_out"]] else "bnin")
        PRODUCTION[(arch, cin)] = (plan, forms, kernels)
        del model, x, t
        torch.cuda.empty_cache()
    return PRODUCTION[(arch, cin)]


def off_production(tracer, config, arch, cin, dims, seed, oc=1, dx=False, adam=False, different=True):
    """One traced bf16 training step at `dims`, reported like the configurations above, and compared with the production
    plan: `different` asserts that a form, a stored-vs-derived decision or a kernel (route) name differs from the
    8 x 512^2 step's."""
    t0 = time.time()
    torch.cuda.empty_cache()
    prod_plan, prod_forms, prod_kernels = production_plan(arch, cin)
    model = make_model(arch, cin, "bf16", oc=oc).train()
    tr = tracer(model, torch.bfloat16, dims)
    opt = None
    if adam:
        from unet_dc_segmentation_amd.optim import FusedAdam
        opt = FusedAdam(model, lr=1e-2)
    x, t = batch(seed, dims[0], cin, dims[1:], oc)
    if dx:
        x.requires_grad_()
    derived = train_step(model, tr, x, t, opt)
    eng = next(iter(tr.engines.values()))
    plan = stage_plan(eng)
    forms = {f for f in tr.forms}
    dplan = {k: (prod_plan[k], v) for k, v in plan.items() if prod_plan[k] != v}
    print(f"\n[{config}] pixel counts per level: {eng.npix}; never materialised (derived): {sorted(derived)}")
    print(f"[{config}] plan entries that differ from 8 x 512^2 (production, here): {dplan}")
    print(f"[{config}] forms only here: {sorted(forms - prod_forms)}; only at 8 x 512^2: {sorted(prod_forms - forms)}")
    print(f"[{config}] kernels only here: {sorted(tr.kernels - prod_kernels)}")
    print(f"[{config}] kernels only at 8 x 512^2: {sorted(prod_kernels - tr.kernels)}")
    report(config, tr, t0)
    if different:
        assert dplan or forms != prod_forms or tr.kernels != prod_kernels, f"{config} reaches exactly the production plan"
    del model, opt
    torch.cuda.empty_cache()
    return tr, plan, dplan


def test_dataflow_bf16_ragged_last_batch(tracer):
    """UNetDC(3, 1), 3 x 512^2, one FusedAdam step: the step every epoch of train_DC_focal.py ends with (no drop_last).  Every
    pixel count is 3 * 2^k: the statistics and the k-coefficients divide by a count that is not a power of two, the
    256-pixel statistics rows come in numbers that are not powers of two.  The maps are the production ones, so the plan
    may be the production plan (printed; not asserted to differ): it is kept for its pixel counts."""
    tr, _, _ = off_production(tracer, "bf16_dc3_3x512", "unetdc", 3, (3, 512, 512), 90, adam=True, different=False)
    assert {"unetdc_conv3x3_first_wgrad", "unetdc_bn_relu_bwd_head", "unetdc_head_fwd_bn"} <= tr.forms, sorted(tr.forms)


def test_dataflow_bf16_single_image(tracer):
    """UNetDC(1, 1), 1 x 512^2: batch 1 -- the normalise-on-load decisions (unetdc_conv3x3_bnin_supported) and the kernel
    routes at an eighth of the production pixel counts."""
    tr, plan, dplan = off_production(tracer, "bf16_1x512", "unetdc", 1, (1, 512, 512), 92)
    # the decisions of unetdc_conv3x3_bnin_supported and unetdc_conv3x3_first_wgrad_bn_supported depend on the maps, not on the
    # batch: at N = 1 every stage keeps the production form and no stage flips `store` ...
    assert not dplan, dplan
    assert plan["enc1.0"] == ("first", "first_bn", False) and plan["enc1.3"] == ("bnin", "bnin", True), plan
    assert plan["dec1.3"] == ("bnin", "bnin", False) and plan["enc2.3"] == ("bnin_store", "plain", True), plan
    assert {"bnin", "bnin_store", "unetdc_conv3x3_first_wgrad_bn", "unetdc_bn_relu_bwd_coeffs", "unetdc_bn_relu_bwd_head"} <= tr.forms
    # ... what changes with an eighth of the pixels is the weight-gradient route: the split-K DMA kernel where 8 x 512^2 takes
    # the fused split kernel, and the ring3 dma16 forward at the small levels
    _, _, prod_kernels = production_plan("unetdc", 1)
    here = tr.kernels - prod_kernels
    assert {"unetdc_conv3x3_wgrad|wgrad_dma_kernel<__bf16, 2>", "unetdc_conv3x3_wgrad|wgrad_dma_kernel<__bf16, 4>",
            "unetdc_conv3x3_fwd|igemm_dma16_kernel<4, 2, 4> ring3"} <= here, sorted(here)
    assert not any("wgrad_fused_split_kernel" in k for k in tr.kernels), sorted(tr.kernels)
    assert any("wgrad_fused_split_kernel" in k for k in prod_kernels), sorted(prod_kernels)


def test_dataflow_bf16_odd_maps(tracer):
    """UNetDC(1, 1), 3 x 48 x 80: a 45-pixel bottleneck (3 x 3 x 5: M % 16 != 0, so no 16x16x32 tile route takes it; odd map
    height and width under dilation 16), pooled maps with an odd number of rows (3, from 6), every count 15 * 2^k or 45, and the
    first layer's BatchNorm-on-load weight gradient at W % 8 == 0."""
    tr, plan, _ = off_production(tracer, "bf16_3x48x80", "unetdc", 1, (3, 48, 80), 94)
    eng = next(iter(tr.engines.values()))
    assert eng.npix[-1] == 45 and eng.npix[-1] % 16, eng.npix
    # first_bn at W = 80 (W % 8 == 0): chosen, and issued with its coefficients
    assert plan["enc1.0"] == ("first", "first_bn", True), plan["enc1.0"]
    assert {"unetdc_conv3x3_first_wgrad_bn", "unetdc_bn_relu_bwd_coeffs"} <= tr.forms, sorted(tr.forms)
    assert ("unetdc_conv3x3_first_wgrad_bn", 48, 80) in tr.calls_at, sorted(tr.calls_at)
    # no map of this step takes a normalise-on-load form: every other stage is plain and stores its activation
    assert all(v[:2] == ("plain", "plain") for k, v in plan.items() if k not in ("enc1.0", "head_fused")), plan
    assert not {"bnin", "bnin_store", "unetdc_conv3x3_fwd_bnin", "unetdc_conv3x3_wgrad_bnin"} & tr.forms, sorted(tr.forms)
    # the 45-pixel maps (M % 16 != 0): every matrix-core call on them -- both bottleneck stages forward, input gradient and
    # weight gradient, and the up-convolution that reads them -- leaves the 16x16x32 routes (dma16, the split weight-gradient
    # kernels) and the lattice / halo routes for the first-generation DMA kernels, which the production step never reaches
    _, _, prod_kernels = production_plan("unetdc", 1)
    at45 = {k: v for k, v in tr.calls_at.items() if (k[1], k[2]) == (3, 5) and "conv" in k[0]}
    print(f"[bf16_3x48x80] kernels on the 3 x 5 maps: { {k[0]: sorted(v) for k, v in sorted(at45.items())} }")
    assert {"unetdc_conv3x3_fwd", "unetdc_conv3x3_wgrad", "unetdc_conv3x3_dgrad", "unetdc_conv3x3_dgrad_bnstats", "unetdc_convT2x2_fwd",
            "unetdc_convT2x2_wgrad", "unetdc_convT2x2_dgrad_bnstats"} <= {k[0] for k in at45}, sorted(at45)
    for (sym, _, _), names in at45.items():
        for name in names:
            assert not any(t in name for t in ("dma16", "16x16x32", "lattice", "halo")), (sym, name)
            if "wgrad" not in sym:
                assert name.startswith("igemm_dma_kernel<__bf16"), (sym, name)
                assert f"{sym}|{name}" not in prod_kernels, (sym, name)
    # odd pooled rows: enc4's 6 x 10 map pools to 3 x 5, forward and backward
    assert eng.res[3] == (6, 10) and eng.res[4] == (3, 5), eng.res
    assert ("unetdc_bn_relu_apply", 6, 10) in tr.calls_at and ("unetdc_bn_relu_bwd", 6, 10) in tr.calls_at, sorted(tr.calls_at)


def small_crop_step(tracer, config, n, seed):
    """UNetDC(3, 1), n x 32^2, one FusedAdam step (train_DC_focal.py --device_data --crop 32 --dtype bf16), traced and compared
    with the production plan.  What the two planning queries say at these maps is what the engine must have planned: no stage
    takes a normalise-on-load form (unetdc_conv3x3_bnin_supported is 0 at 32 ... 4 pixels a side: the 32 x 32 level takes the
    lattice forward, but no input-normalising weight gradient exists below 32K pixels; the others are no lattice maps) and
    the first layer keeps the plain weight gradient (unetdc_conv3x3_first_wgrad_bn_supported: C_in = 3).  Measured on MI355X,
    worst err / bound over all value kinds: 0.996 at 4 x 32^2 and at 1 x 32^2 (stored bf16 activations, one rounding from the
    reference; the BatchNorm constants stay below 3e-5 and the gradients of the parameters below 0.37)."""
    from unet_dc_segmentation_amd import _lib
    lib = _lib.load()
    tr, plan, dplan = off_production(tracer, config, "unetdc", 3, (n, 32, 32), seed, adam=True)
    eng = next(iter(tr.engines.values()))
    print(f"[{config}] plan: {plan}")
    assert eng.npix == [n * 1024, n * 256, n * 64, n * 16, n * 4] and eng.res[-1] == (2, 2), (eng.npix, eng.res)
    for (block, idx), st in eng.stages.items():
        if idx == 3 and block != "bottleneck":
            assert lib.unetdc_conv3x3_bnin_supported(n, *st.hw, st.cout, st.cout, st.dil, 1) == 0, (block, st.hw)
    assert lib.unetdc_conv3x3_first_wgrad_bn_supported(n, 32, 32, 3, 64, 1, 1) == 0
    assert plan["enc1.0"] == ("first", "first", True), plan["enc1.0"]
    assert all(v[:2] == ("plain", "plain") for k, v in plan.items() if k not in ("enc1.0", "head_fused")), plan
    assert all(v[2] for k, v in plan.items() if k not in ("dec1.3", "head_fused")), plan       # every activation is stored
    assert plan["head_fused"] is True
    assert not {"bnin", "bnin_store", "unetdc_conv3x3_fwd_bnin", "unetdc_conv3x3_wgrad_bnin", "unetdc_conv3x3_first_wgrad_bn",
                "unetdc_bn_relu_bwd_coeffs"} & tr.forms, sorted(tr.forms)
    assert {"unetdc_conv3x3_first_wgrad", "unetdc_bn_relu_bwd_head", "unetdc_head_fwd_bn"} <= tr.forms, sorted(tr.forms)
    # the 2 x 2 bottleneck: both stages forward, input gradient and weight gradient, and the up-convolution that reads it
    at2 = {k[0]: sorted(v) for k, v in tr.calls_at.items() if (k[1], k[2]) == (2, 2) and "conv" in k[0]}
    print(f"[{config}] kernels on the 2 x 2 maps: {at2}")
    assert {"unetdc_conv3x3_fwd", "unetdc_conv3x3_wgrad", "unetdc_conv3x3_dgrad", "unetdc_conv3x3_dgrad_bnstats", "unetdc_convT2x2_fwd",
            "unetdc_convT2x2_wgrad", "unetdc_convT2x2_dgrad_bnstats"} <= set(at2), sorted(at2)
    for sym, names in at2.items():
        for name in names:
            assert "wgrad_rect_kernel" not in name, (sym, name)        # d = 16 >= 2: rect_plan finds an empty rectangle
            if (n * 4) % 16:                                           # M = 4 N below one 16-row tile
                assert not any(t in name for t in ("dma16", "16x16x32", "lattice", "halo")), (sym, name)
    return tr, eng


def test_dataflow_bf16_crop_4x32(tracer):
    """UNetDC(3, 1), 4 x 32^2 with FusedAdam: the smallest --crop step at a full batch.  A 2 x 2 bottleneck (M = 16, exactly
    one MFMA tile; BatchNorm statistics over 16 values), dilation >= the map side at the bottleneck, enc4 and enc3, the
    persistent lattice kernel with 16 items at the 32 x 32 level."""
    small_crop_step(tracer, "bf16_dc3_4x32", 4, 104)


def test_dataflow_bf16_crop_1x32(tracer):
    """The same at 1 x 32^2, the ragged last batch: M = 4 at the bottleneck (BatchNorm statistics over 4 values per
    channel), 4 lattice items on a grid of 4 at the 32 x 32 level."""
    _, eng = small_crop_step(tracer, "bf16_dc3_1x32", 1, 106)
    assert eng.npix[-1] == 4, eng.npix


def test_dataflow_bf16_odd_maps_three_channels_dx(tracer):
    """UNetDC(3, 1) with x.requires_grad, 2 x 96 x 160: the plain first-layer weight gradient, first_dgrad and dL/dx on a
    non-square map; 120-pixel bottleneck (2 x 6 x 10), below one 256-pixel statistics block."""
    tr, plan, _ = off_production(tracer, "bf16_dc3_2x96x160_dx", "unetdc", 3, (2, 96, 160), 96, dx=True)
    assert {"unetdc_conv3x3_first_wgrad", "unetdc_conv3x3_first_dgrad"} <= tr.forms, sorted(tr.forms)
    assert plan["enc1.0"] == ("first", "first", True), plan["enc1.0"]
    assert tr.calls_at[("unetdc_conv3x3_first_dgrad", 96, 160)] == {"first_dgrad_kernel<__bf16>"}, tr.calls_at
    assert all(v[:2] == ("plain", "plain") for k, v in plan.items() if k not in ("enc1.0", "head_fused")), plan
    # the 120-pixel bottleneck (M % 16 != 0 as well: 120 = 7.5 * 16) takes the first-generation DMA kernel
    at120 = set().union(*(v for k, v in tr.calls_at.items() if (k[1], k[2]) == (6, 10) and "conv" in k[0]))
    print(f"[bf16_dc3_2x96x160_dx] kernels on the 6 x 10 maps: {sorted(at120)}")
    assert "igemm_dma_kernel<__bf16, 4, 2, 2>" in at120 and not any("dma16" in k or "16x16x32" in k for k in at120), sorted(at120)


def test_dataflow_bf16_1024_tiles(tracer):
    """UNetDC(1, 1), 4 x 1024^2 (BASELINE.json configs[4]): the pixel counts of 8 x 512^2 on rows twice as wide -- the tile
    geometry of the lattice / halo routes, the pool and up-convolution decodes."""
    tr, plan, dplan = off_production(tracer, "bf16_4x1024", "unetdc", 1, (4, 1024, 1024), 98)
    # the same plan as 8 x 512^2 (the forms depend on maps the lattice kernels take at both sizes) ...
    assert not dplan, dplan
    # ... and the same lattice / halo kernels, on rows twice as wide; what moves is the dma16 tile choice of the levels
    # whose maps doubled: the 2x4x8 tiling with 16x16 blocks appears, the ring3 one of the 512^2 step is gone
    _, _, prod_kernels = production_plan("unetdc", 1)
    lattice = lambda ks: {k for k in ks if "lattice" in k or "halo" in k}           # noqa: E731
    assert lattice(tr.kernels) == lattice(prod_kernels), (sorted(lattice(tr.kernels)), sorted(lattice(prod_kernels)))
    here = tr.kernels - prod_kernels
    assert {"unetdc_conv3x3_fwd|igemm_dma16_kernel<2, 4, 8> blocks16x16",
            "unetdc_conv3x3_dgrad_bnstats|igemm_dma16_kernel<2, 4, 8> blocks16x16"} <= here, sorted(here)
    assert "unetdc_conv3x3_fwd|igemm_dma16_kernel<4, 2, 4> ring3 blocks16x16" in prod_kernels - tr.kernels
    # every pool and up-convolution of the step ran at the doubled row width
    assert {("unetdc_bn_relu_apply", 1024, 1024), ("unetdc_convT2x2_fwd", 512, 512), ("unetdc_convT2x2_fwd", 64, 64)} <= set(tr.calls_at)


def test_dataflow_bf16_two_output_channels(tracer):
    """UNetDC(1, 2), 2 x 128^2, a (N, 2, H, W) target through the fused loss (it takes any [N, OC, H, W] pair of equal shapes):
    head_fused is False, so the head backward stores dA and dec1.3 takes the plain unetdc_bn_relu_bwd."""
    tr, plan, dplan = off_production(tracer, "bf16_oc2_2x128", "unetdc", 1, (2, 128, 128), 100, oc=2)
    assert plan["head_fused"] is False and "head_fused" in dplan
    assert "unetdc_bn_relu_bwd_head" not in tr.forms and "unetdc_bn_relu_bwd" in tr.forms, sorted(tr.forms)
    eng = next(iter(tr.engines.values()))
    assert "g:dec1.3.a" in tr.produced[id(eng)], "the head's input gradient should be stored, not derived"


def test_dataflow_bf16_unet_384_batch_5(tracer):
    """UNet(3, 1), 5 x 384^2 (train.py --img_size 384 --batch 5 on the bf16 path): every count 45 * 2^k, maps of 384 ... 24
    pixels a side."""
    tr, plan, dplan = off_production(tracer, "bf16_unet3_5x384", "unet", 3, (5, 384, 384), 102)
    # the 48 x 48 level leaves the normalise-on-load forms (bnin_store at 64 x 64): enc4 and dec4 run plain and store
    assert set(dplan) == {"enc4.0", "enc4.3", "dec4.0", "dec4.3"}, dplan
    assert dplan["enc4.3"] == (("bnin_store", "plain", True), ("plain", "plain", True)), dplan
    assert dplan["dec4.3"] == (("bnin_store", "plain", True), ("plain", "plain", True)) and plan["enc4.0"][2] and plan["dec4.0"][2], dplan
    # the 24 x 24 bottleneck's up-convolution takes the first-generation DMA kernel and the DMA weight gradient
    _, _, prod_kernels = production_plan("unet", 3)
    here = tr.kernels - prod_kernels
    assert {"unetdc_convT2x2_fwd|igemm_dma_kernel<__bf16, 4, 2, 2>", "unetdc_convT2x2_wgrad|wgrad_dma_kernel<__bf16, 4>"} <= here, \
        sorted(here)
    assert tr.calls_at[("unetdc_convT2x2_fwd", 24, 24)] == {"igemm_dma_kernel<__bf16, 4, 2, 2>"}, tr.calls_at
