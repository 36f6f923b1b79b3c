"""The data-parallel step against a one-process replay: the shared workers of tests/test_gpu_dp_step.py (two ranks on one
card over gloo, HIP backward + hooks + FusedAdam) and tests/test_dp_step_cpu.py (the same scenarios on the ATen-CPU path,
sync_gradients() + FusedAdam._step_torch).

The reference is a replay, not a tolerance.  For two ranks the exchange is (g0 + g1).div_(2): one commutative fp32 addition
per element and one division, so every rank can recompute the exchanged gradient from both ranks' LOCAL gradients (taken on a
second module instance that has no hooks) and the data-parallel step must give the same bits.  The optimizer step is replayed
on that second instance from the same state, with ``p.grad`` set to the replayed average as separate tensors (FusedAdam's
torch.cat path, pinned equal to the flat path by test_fused_adam_cat_fallback_equals_the_flat_path).

Rules of the worker: every rank issues the same collectives in the same order whatever a check finds (checks are collected
and raised at the end of a scenario), the ranks agree on the outcome after every scenario, and after the first failure
nothing more runs: later scenarios are reported "not run: <name> failed first".

Plain Python at module level: torch and the package are imported inside the workers."""
import os
import socket
import time
import traceback
from datetime import timedelta

PG_TIMEOUT = timedelta(seconds=120)
SHAPE = (2, 1, 32, 32)                 # the smallest map the network takes (four poolings -> 2 x 2 at the bottleneck)
INF = float("inf")

# scenario -> needs the HIP path as a whole (flat-buffer reuse has no counterpart on CPU tensors)
SCENARIOS = {"replicas_after_broadcast": False, "plain_step": False, "recipe_step": False, "one_rank_nonfinite": False,
             "three_steps_reuse": True, "ragged_last_batch": False, "trace_does_not_disturb": False}
BUCKETS_MB = [21.5, 18.9, 23.1, 23.1, 18.9, 17.7, 1.0]      # the schedule tests/test_dp_gloo.py and DESIGN.md section 5 state


def scenario_ids(device):
    """The names the pair runs, in order: every scenario in fp32, on the HIP path in bf16 compute too (the ATen-CPU path has
    no compute type)."""
    dtypes = ("f32", "bf16") if device == "cuda" else ("f32",)
    return [f"{s}[{d}]" for s, hip_only in SCENARIOS.items() if device == "cuda" or not hip_only for d in dtypes]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


# ---------------------------------------------------------------------------------------------------------------- parent side
def run_children(target, per_rank_args, wait):
    """Start one fresh (spawn) process per entry of per_rank_args, read one result from each within `wait` seconds in all, and
    leave none behind: whatever happened, a child that is still alive is killed and joined.  No retries.
    -> (results in arrival order -- a string instead of a result for every child that did not answer --, wall seconds)."""
    import queue

    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(*a, q)) for a in per_rank_args]
    t0 = time.perf_counter()
    results = []
    try:
        for p in procs:
            p.start()
        for _ in procs:
            try:
                results.append(q.get(timeout=max(1.0, t0 + wait - time.perf_counter())))
            except queue.Empty:
                break
        wall = time.perf_counter() - t0
        if len(results) == len(procs):
            for p in procs:
                p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
            if p.pid is not None:
                p.join()
    missing = len(procs) - len(results)
    results += [f"no result within {wait:.0f} s (exit codes {[p.exitcode for p in procs]})"] * missing
    return results, wall


def run_pair(device, names, wait, world=2):
    """The scenarios `names` on `world` ranks.  -> ({rank: {scenario: "ok" | text}}, wall seconds, {rank: timings})."""
    port = free_port()
    results, wall = run_children(pair_worker, [(r, world, port, device, list(names)) for r in range(world)], wait)
    out = {res[0]: res[1] for res in results if not isinstance(res, str)}
    timings = {res[0]: res[2] for res in results if not isinstance(res, str)}
    silent = next((res for res in results if isinstance(res, str)), None)
    for r in range(world):
        out.setdefault(r, {n: silent for n in names})       # a rank that did not answer fails every scenario
    return out, wall, timings


# ---------------------------------------------------------------------------------------------------------------- worker side
class Checks:
    """Collects what a scenario finds; raised in one piece at its end, after every collective of the scenario has run."""

    def __init__(self):
        self.bad = []

    def __call__(self, ok, msg):
        if not ok:
            self.bad.append(msg)

    def done(self):
        if self.bad:
            more = f" (+{len(self.bad) - 8} more)" if len(self.bad) > 8 else ""
            raise AssertionError("; ".join(self.bad[:8]) + more)


class Ctx:
    def __init__(self, rank, world, device):
        self.rank, self.world, self.device, self.hip = rank, world, device, device == "cuda"


def bits_equal(a, b):
    """Same shape, type and bits (NaN equals the same NaN, +0.0 does not equal -0.0)."""
    import torch
    a, b = a.detach(), b.detach()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a, b.to(a.device)))


def gather(ctx, t):
    """Every rank's copy of `t`, the tensors themselves, over host memory."""
    import torch
    import torch.distributed as dist
    t = t.detach().cpu().contiguous()
    out = [torch.empty_like(t) for _ in range(ctx.world)]
    dist.all_gather(out, t)
    return out


def same_on_all_ranks(ctx, t):
    g = gather(ctx, t)
    return all(bits_equal(g[0], x) for x in g[1:])


def gather_objects(ctx, obj):
    import torch.distributed as dist
    out = [None] * ctx.world
    dist.all_gather_object(out, obj)
    return out


def flat_params(model):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def flat_buffers(model):
    import torch
    return torch.cat([b.detach().reshape(-1).double() for b in model.buffers()])     # (running statistics and the int64 counters)


def batch(ctx, r, k=0, n=2):
    """Rank r's input and target of round k, n items."""
    from oracle import recipe
    x = recipe.seeded_input(50 + r + 10 * k, SHAPE)[:n].contiguous()
    t = recipe.seeded_target(60 + r + 10 * k, SHAPE)[:n].contiguous()
    return x.to(ctx.device), t.to(ctx.device)


def eval_forward(model, x):
    import torch
    model.eval()
    with torch.no_grad():
        y = model(x).clone()
    model.train()
    return y


def train_forward(model, x):
    import torch
    with torch.no_grad():
        return model(x).clone()


def make_pair(ctx, dtype, wrap=True):
    """(module with a per-rank initialisation, its DataParallel wrapper, replay module in the wrapped module's state)."""
    import torch
    from models.model_2 import UNetDC
    from unet_dc_segmentation_amd.dp import DataParallel
    torch.manual_seed(100 + ctx.rank)                       # the broadcast must make the replicas equal
    model = UNetDC(1, 1).to(ctx.device).train()
    model.set_compute_dtype(dtype)
    if not wrap:
        return model, None, None
    dp = DataParallel(model)
    return model, dp, make_replay(ctx, model, dtype)


def make_replay(ctx, model, dtype):
    from models.model_2 import UNetDC
    replay = UNetDC(1, 1).to(ctx.device).train()
    replay.set_compute_dtype(dtype)
    replay.load_state_dict(model.state_dict())
    return replay


def local_grads(ctx, replay, k=0, n=2, scales=None):
    """Every rank's LOCAL gradient of round k at the replay module's parameters: no hooks, no exchange."""
    from utils.metrics_DC import focal_dice_loss
    out = []
    for r in range(ctx.world):
        x, t = batch(ctx, r, k, n)
        replay.zero_grad(set_to_none=True)
        loss = focal_dice_loss(replay(x), t)
        if scales is not None:
            loss = loss * scales[r]
        loss.backward()
        out.append([p.grad.clone() for p in replay.parameters()])
    replay.zero_grad(set_to_none=True)
    return out


def average(per_rank):
    """The exchange, replayed: one fp32 sum in rank order (commutative for two ranks), one division."""
    avg = []
    for gs in zip(*per_rank):
        s = gs[0].clone()
        for g in gs[1:]:
            s.add_(g)
        avg.append(s.div_(len(per_rank)))
    return avg


def dp_backward(ctx, model, dp, k=0, n=2, scale=None):
    """This rank's data-parallel forward + backward of round k (the HIP backward exchanges through the hooks; CPU tensors
    through sync_gradients(), as train_DC_focal.py does)."""
    from utils.metrics_DC import focal_dice_loss
    x, t = batch(ctx, ctx.rank, k, n)
    model.zero_grad(set_to_none=True)
    loss = focal_dice_loss(model(x), t)
    if scale is not None:
        loss = loss * scale
    loss.backward()
    if not ctx.hip:
        dp.sync_gradients()


def check_grads(ck, tag, model, avg):
    bad = [i for i, (p, g) in enumerate(zip(model.parameters(), avg)) if not bits_equal(p.grad, g)]
    ck(not bad, f"{tag}: gradients of {len(bad)} parameters differ from the replayed average (first: #{bad[0] if bad else -1})")


def check_flat_views(ck, tag, model):
    """Every p.grad is a view of ONE flat fp32 buffer in parameters() order."""
    params = list(model.parameters())
    base, off, bad = params[0].grad.data_ptr(), 0, []
    for i, p in enumerate(params):
        if p.grad.data_ptr() != base + 4 * off or not p.grad.is_contiguous():
            bad.append(i)
        off += p.numel()
    ck(not bad, f"{tag}: gradients {bad[:4]} are not views of one flat buffer")


def replay_step(replay, opt_r, avg):
    for p, g in zip(replay.parameters(), avg):
        p.grad = g
    opt_r.step()
    replay.zero_grad(set_to_none=True)


def check_state(ctx, ck, tag, model, opt, replay, opt_r, ema=False):
    """Parameters and optimizer state: bit-equal to the replay and across ranks."""
    pairs = [("parameters", flat_params(model), flat_params(replay)), ("exp_avg", opt._m, opt_r._m),
             ("exp_avg_sq", opt._v, opt_r._v)]
    if ema:
        pairs.append(("EMA", opt._ema, opt_r._ema))
    for name, a, b in pairs:
        ck(bits_equal(a, b), f"{tag}: {name} differ from the replay")
        ck(same_on_all_ranks(ctx, a), f"{tag}: {name} differ between the ranks")


def check_recipe_record(ctx, ck, tag, opt, opt_r):
    sa, sb = opt.recipe_stats(), opt_r.recipe_stats()
    ck(sa == sb, f"{tag}: recipe_stats {sa} != replay {sb}")
    everyone = gather_objects(ctx, sa)
    ck(all(s == everyone[0] for s in everyone), f"{tag}: recipe_stats differ between the ranks: {everyone}")
    if ctx.hip:                                              # the 56 bytes of the device record
        a, b = opt._ctl.cpu(), opt_r._ctl.cpu()
        ck(a.numel() == 56 and bits_equal(a, b), f"{tag}: device record {a.tolist()} != replay {b.tolist()}")
        ck(same_on_all_ranks(ctx, a), f"{tag}: device record differs between the ranks")
    return sa


def nparams(model):
    return sum(p.numel() for p in model.parameters())


# ---------------------------------------------------------------------------------------------------------------- scenarios
def replicas_after_broadcast(ctx, dtype, ck):
    import torch

    from oracle import recipe
    from unet_dc_segmentation_amd.dp import DataParallel
    model, _, _ = make_pair(ctx, dtype, wrap=False)
    xc = recipe.seeded_input(7, SHAPE).to(ctx.device)       # one common input
    train_forward(model, batch(ctx, ctx.rank)[0])           # running statistics that differ per rank
    y_own = eval_forward(model, xc)                         # (HIP: the packed images now hold THIS rank's weights)
    own = flat_params(model).clone()
    DataParallel(model)
    if ctx.hip:
        w = model._weights
        ck(w is not None and w._versions is None, "broadcast_state() did not invalidate the packed weight images")
    p, b = flat_params(model), flat_buffers(model)
    ck(same_on_all_ranks(ctx, p), "parameters differ between the ranks after the broadcast")
    ck(same_on_all_ranks(ctx, b), "buffers differ between the ranks after the broadcast")
    ck(ctx.rank == 0 or not bits_equal(p, own), "the broadcast left this rank's own initialisation in place")
    y = eval_forward(model, xc)
    ck(same_on_all_ranks(ctx, y), "eval forward of one common input differs between the ranks")
    ck(ctx.rank == 0 or not bits_equal(y, y_own), "eval forward still gives this rank's pre-broadcast output")
    fresh = make_replay(ctx, model, dtype)                  # images packed from the broadcast weights, nothing older
    ck(bits_equal(y, eval_forward(fresh, xc)), "eval forward differs from a fresh module in the same state")
    ck(bool(torch.isfinite(y).all()), "eval forward is not finite")


def plain_step(ctx, dtype, ck):
    from unet_dc_segmentation_amd.optim import FusedAdam
    model, dp, replay = make_pair(ctx, dtype)
    opt, opt_r = FusedAdam(model), FusedAdam(replay)
    avg = average(local_grads(ctx, replay))
    e0, s0 = dp.stats["elems"], dp.stats["steps"]
    dp_backward(ctx, model, dp)
    check_grads(ck, "backward", model, avg)
    if ctx.hip:
        check_flat_views(ck, "backward", model)
    ck(dp.stats["steps"] - s0 == 1 and dp.stats["elems"] - e0 == nparams(model),
       f"exchanged {dp.stats['elems'] - e0} elements in {dp.stats['steps'] - s0} step(s), the parameters have {nparams(model)}")
    opt.step()
    replay_step(replay, opt_r, avg)
    check_state(ctx, ck, "step", model, opt, replay, opt_r)
    x = batch(ctx, 0, 1)[0]                                  # one input for every rank: the outputs must agree
    y = train_forward(model, x)
    ck(bits_equal(y, train_forward(replay, x)), "next train forward differs from the replay")
    ck(same_on_all_ranks(ctx, y), "next train forward differs between the ranks")


def recipe_step(ctx, dtype, ck):
    import torch

    from unet_dc_segmentation_amd.optim import FusedAdam
    model, dp, replay = make_pair(ctx, dtype)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    avg = average(local_grads(ctx, replay))
    norm = float(torch.linalg.vector_norm(torch.cat([g.reshape(-1) for g in avg]).double()))
    ck(norm > 0.0 and norm < INF, f"replayed gradient norm {norm}")
    for tag, c, clipped in (("clipping step", 0.5 * norm, 1), ("unclipped step", 2.0 * norm, 0)):
        model.load_state_dict(sd0)
        replay.load_state_dict(sd0)
        kw = dict(weight_decay=0.01, clip_norm=c, ema_decay=0.99)
        opt, opt_r = FusedAdam(model, **kw), FusedAdam(replay, **kw)
        dp_backward(ctx, model, dp)
        check_grads(ck, tag, model, avg)
        opt.step()
        replay_step(replay, opt_r, avg)
        check_state(ctx, ck, tag, model, opt, replay, opt_r, ema=True)
        s = check_recipe_record(ctx, ck, tag, opt, opt_r)
        ck((s["steps"], s["clipped"], s["skipped"]) == (1, clipped, 0), f"{tag}: {s}")
        ck(abs(s["grad_norm_mean"] - norm) <= 1e-5 * norm, f"{tag}: norm {s['grad_norm_mean']} of the averaged gradient, replay {norm}")
        del opt, opt_r


def one_rank_nonfinite(ctx, dtype, ck):
    import torch

    from oracle import recipe
    from unet_dc_segmentation_amd.optim import FusedAdam
    model, dp, replay = make_pair(ctx, dtype)
    kw = dict(skip_nonfinite=True, ema_decay=0.99)
    opt, opt_r = FusedAdam(model, **kw), FusedAdam(replay, **kw)
    opt.ema_tensors(), opt_r.ema_tensors()                  # the state exists before the first step
    xc = recipe.seeded_input(7, SHAPE).to(ctx.device)
    scales = [1.0] * ctx.world
    scales[1] = INF                                          # rank 1 alone
    avg = average(local_grads(ctx, replay, scales=scales))
    ck(not all(bool(torch.isfinite(g).all()) for g in avg), "the replayed average is finite: nothing to skip")
    dp_backward(ctx, model, dp, scale=scales[ctx.rank])
    before = [t.clone() for t in (flat_params(model), opt._m, opt._v, opt._ema)]
    y0 = eval_forward(model, xc)
    opt.step()
    for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq", "EMA"), (flat_params(model), opt._m, opt._v, opt._ema), before):
        ck(bits_equal(a, b), f"skipped step: {name} changed on rank {ctx.rank}")
    ck(bits_equal(eval_forward(model, xc), y0), f"skipped step: eval forward changed on rank {ctx.rank}")
    s = opt.recipe_stats()
    everyone = gather_objects(ctx, (s["steps"], s["skipped"]))
    ck(all(e == (1, 1) for e in everyone), f"(steps, skipped) per rank {everyone}, expected (1, 1) on every rank")
    ck(same_on_all_ranks(ctx, flat_params(model)), "skipped step: parameters differ between the ranks")
    replay_step(replay, opt_r, avg)                         # the replay drops the same step: the counters run on
    avg = average(local_grads(ctx, replay, k=1))
    dp_backward(ctx, model, dp, k=1)
    check_grads(ck, "step after the skip", model, avg)
    opt.step()
    replay_step(replay, opt_r, avg)
    check_state(ctx, ck, "step after the skip", model, opt, replay, opt_r, ema=True)
    s = check_recipe_record(ctx, ck, "step after the skip", opt, opt_r)
    ck((s["steps"], s["skipped"]) == (2, 1), f"after the second step: {s}")
    ck(not bits_equal(flat_params(model), before[0]), "the step after the skip changed nothing")


def three_steps_reuse(ctx, dtype, ck):
    from unet_dc_segmentation_amd.optim import FusedAdam
    model, dp, replay = make_pair(ctx, dtype)
    opt, opt_r = FusedAdam(model), FusedAdam(replay)
    params = list(model.parameters())
    ptrs = []
    for k in range(3):
        avg = average(local_grads(ctx, replay, k=k))
        dp_backward(ctx, model, dp, k=k)                    # (zero_grad(set_to_none=True) first: the views of round k - 1 go)
        ptrs.append(params[0].grad.data_ptr())
        ck(not dp._works and dp._pending is None, f"round {k}: the wrapper keeps views of the flat buffer after finish()")
        check_grads(ck, f"round {k}", model, avg)
        opt.step()
        replay_step(replay, opt_r, avg)
        check_state(ctx, ck, f"round {k}", model, opt, replay, opt_r)
    ck(ptrs[1] == ptrs[0] and ptrs[2] == ptrs[0], f"the flat buffer was not handed out again: {[hex(p) for p in ptrs]}")
    # round 2's gradients kept alive by the caller: round 3 must take a fresh buffer and leave them alone
    kept = [p.grad for p in params]
    snap = [g.clone() for g in kept]
    avg = average(local_grads(ctx, replay, k=3))
    dp_backward(ctx, model, dp, k=3)
    ck(params[0].grad.data_ptr() != ptrs[2], "a backward wrote into a flat buffer whose gradients the caller still holds")
    bad = [i for i, (a, b) in enumerate(zip(kept, snap)) if not bits_equal(a, b)]
    ck(not bad, f"gradients kept from round 2 were overwritten by round 3 (first: #{bad[0] if bad else -1})")
    check_grads(ck, "round 3", model, avg)
    check_flat_views(ck, "round 3", model)


def ragged_last_batch(ctx, dtype, ck):
    from unet_dc_segmentation_amd.optim import FusedAdam
    model, dp, replay = make_pair(ctx, dtype)
    opt, opt_r = FusedAdam(model), FusedAdam(replay)
    for k, n in enumerate((2, 1, 2)):
        avg = average(local_grads(ctx, replay, k=k, n=n))
        e0 = dp.stats["elems"]
        dp_backward(ctx, model, dp, k=k, n=n)
        check_grads(ck, f"batch {k} of {n}", model, avg)
        ck(dp.stats["elems"] - e0 == nparams(model), f"batch {k} of {n}: exchanged {dp.stats['elems'] - e0} elements")
        opt.step()
        replay_step(replay, opt_r, avg)
        check_state(ctx, ck, f"batch {k} of {n}", model, opt, replay, opt_r)
    if ctx.hip:
        ck(len(model._engines) == 2, f"engines alive: {sorted(s for _, s in model._engines)}")


def trace_does_not_disturb(ctx, dtype, ck):
    model, dp, _ = make_pair(ctx, dtype)
    dp_backward(ctx, model, dp)
    plain = [p.grad.clone() for p in model.parameters()]
    dp.start_trace()
    dp_backward(ctx, model, dp)
    res = dp.stop_trace()
    check_grads(ck, "traced step", model, plain)
    ck(res is not None and res["traced_steps"] == 1, f"stop_trace() -> {res}")
    ck(res is not None and "perf_counter" in res["clock"], "gloo must be timed on the host clock")
    ck(dp._trace is None, "tracing is still on after stop_trace()")


def run_scenario(ctx, name):
    """-> "ok" or the traceback."""
    import gc

    import torch
    fn, dtype = name[:-1].split("[")
    ck = Checks()
    try:
        globals()[fn](ctx, dtype, ck)
        ck.done()
        if ctx.hip:
            torch.cuda.synchronize()
        return "ok"
    except BaseException as e:  # noqa: BLE001
        return f"{type(e).__name__} on rank {ctx.rank}: {e}\n{traceback.format_exc()}"
    finally:
        gc.collect()
        if ctx.hip:
            torch.cuda.empty_cache()


def pair_worker(rank, world, port, device, names, q):
    t_start = time.perf_counter()
    results, timings, failed = {}, {}, None
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch
        import torch.distributed as dist
        if device == "cpu":
            torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=PG_TIMEOUT)
        if device == "cuda":
            torch.cuda.set_device(0)
        ctx = Ctx(rank, world, device)
        timings["startup_s"] = time.perf_counter() - t_start
        for name in names:
            if failed is not None:
                results[name] = f"not run: {failed} failed first"
                continue
            t0 = time.perf_counter()
            results[name] = run_scenario(ctx, name)
            timings[name] = time.perf_counter() - t0
            # the ranks agree on the outcome (host tensors: nothing of this touches the device)
            flag = torch.tensor([0 if results[name] == "ok" else 1])
            try:
                dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            except Exception as e:  # noqa: BLE001
                flag[0] = 1
                results[name] += f"\n(the ranks could not agree on the outcome: {e!r})"
            if int(flag):
                failed = name
        if failed is None:
            dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        text = f"{type(e).__name__} on rank {rank}: {e}\n{traceback.format_exc()}"
        first = failed or next((n for n in names if n not in results), names[-1])
        for n in names:
            results.setdefault(n, text if n == first else f"not run: {first} failed first")
    q.put((rank, results, timings))


# ---------------------------------------------------------------------------------------------------------------- one-rank RCCL
def rccl_worker(port, q):
    """UNETDC_DP_FORCE=1: init_from_env() brings up a one-rank 'nccl' (= RCCL) group on cuda:0; two traced bf16 steps."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                          UNETDC_DP_FORCE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch
        import torch.distributed as dist

        from unet_dc_segmentation_amd import dp as dpmod
        from unet_dc_segmentation_amd.optim import FusedAdam
        rank, local, world = dpmod.init_from_env(timeout=PG_TIMEOUT)
        group = dict(rank=rank, local=local, world=world, initialised=dist.is_initialized(),
                     backend=dist.get_backend() if dist.is_initialized() else None, device=torch.cuda.current_device())
        ctx = Ctx(0, 1, "cuda")
        model, _, _ = make_pair(ctx, "bf16", wrap=False)
        dp = dpmod.DataParallel(model, single_rank_collectives=True)
        sd0 = {k: v.clone() for k, v in model.state_dict().items()}

        def two_steps(traced):
            model.load_state_dict(sd0)
            opt = FusedAdam(model)
            grads = []
            if traced:
                dp.start_trace()
                dp.mark_step_start()
            for k in range(2):
                dp_backward(ctx, model, dp, k=k)
                grads.append([p.grad.clone() for p in model.parameters()])
                opt.step()
            return grads, (dp.stop_trace() if traced else None)

        plain, _ = two_steps(False)
        traced, res = two_steps(True)
        torch.cuda.synchronize()
        same = all(bits_equal(a, b) for ga, gb in zip(plain, traced) for a, b in zip(ga, gb))
        moved = not all(bits_equal(a, b) for a, b in zip(plain[0], plain[1]))
        out = dict(group=group, trace=res, trace_off=dp._trace is None, grads_equal=same, steps_differ=moved,
                   elems_per_step=dp.stats["elems"] / max(dp.stats["steps"], 1), nparams=nparams(model))
        dist.barrier()
        dist.destroy_process_group()
        q.put(("ok", out))
    except BaseException as e:  # noqa: BLE001
        q.put((f"{type(e).__name__}: {e}\n{traceback.format_exc()}", None))


# ---------------------------------------------------------------------------------------------------------------- entry point
def train_worker(rank, world, port, argv, q):
    """train_DC_focal.main under `world` gloo ranks that share cuda:0; the process group is up before main() looks for one.
    -> (rank, "ok", epoch records, number of torch.save calls of this rank)."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=PG_TIMEOUT)
        import train_DC_focal as t
        saves, save = [], torch.save

        def counting_save(obj, f, *a, **k):
            saves.append(str(f))
            return save(obj, f, *a, **k)
        torch.save = counting_save
        try:
            hist = t.main(argv)
        finally:
            torch.save = save
        q.put((rank, "ok", [dict(r) for r in hist], saves))
    except BaseException as e:  # noqa: BLE001
        q.put((rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}", None, None))


def write_pairs(d, n, h=100, w=140, discs=12):
    """n image / mask PNG pairs by the recipe of the data_dir fixture of tests/test_gpu_device_data.py (bench's synthetic
    micrograph, its mask by threshold, one grayscale file), at a size that keeps the native-resolution run to a few windows.
    -> (image dir, mask dir)."""
    import numpy as np
    from PIL import Image

    import bench
    ind, md = d / "images", d / "masks"
    ind.mkdir()
    md.mkdir()
    for i in range(n):
        img = bench.synthetic_micrograph(100 + i, h=h, w=w, discs=discs)
        mask = (img[..., 0] > 110).astype(np.uint8) * 255
        Image.fromarray(img[..., 0] if i == 2 else img).save(ind / f"img_{i:03d}.png")
        Image.fromarray(mask).save(md / f"img_{i:03d}.png")
    return str(ind), str(md)
