"""GPU: the data-parallel step on the device against a one-process replay (tests/dp_step_cases.py).

Two ranks share cuda:0 and exchange over gloo (RCCL refuses two ranks on one device), as in tests/test_gpu_dp.py: the HIP
backward announces its ranges, dp.py all-reduces the flat buffer in place, FusedAdam reads that buffer.  For two ranks the
exchange is (g0 + g1).div_(2), which a rank can recompute from both ranks' local gradients, so everything here is compared
BITWISE: averaged gradients, parameters, moments, EMA, the optimizer's device record, the next forward, and all of it across
the ranks.  A one-rank RCCL worker covers the 'nccl' branch with the device-event trace, and two runs of train_DC_focal.main
cover the entry point under two ranks on the device.

Every spawned group is measured where it runs (the print of its fixture); each wait below is three times the wall time
measured on an MI355X, and no more than the 900 s of tests/test_gpu_dp.py."""
import pytest
import torch

from tests import dp_step_cases as cases

pytestmark = pytest.mark.gpu

NAMES = cases.scenario_ids("cuda")
DTYPES = ("f32", "bf16")
# seconds a parent waits for its children: 3 x the measured wall time of the group (see the summary of the change that
# added this file; the larger of two runs: the pair of 14 scenarios 24.2 s, the one-rank RCCL worker 8.1 s, the entry-point
# pairs 4.7 s and 5.2 s)
WAIT_PAIR, WAIT_RCCL, WAIT_ENTRY = 75, 25, 16


# ---------------------------------------------------------------------------------------------------------------- the pair
@pytest.fixture(scope="module")
def pair():
    results, wall, timings = cases.run_pair("cuda", NAMES, WAIT_PAIR)
    print(f"\ndata-parallel step, two ranks on one card: pair wall {wall:.1f} s; rank 0: "
          f"{ {k: round(v, 1) for k, v in timings.get(0, {}).items()} }")
    for rank in sorted(results):
        for name, text in results[rank].items():
            if text != "ok":
                print(f"rank {rank} {name}: {str(text)[:1500]}")
    return results


def _entry(pair, scenario, dtype):
    """A scenario that did not run is a failure like any other."""
    name = f"{scenario}[{dtype}]"
    assert name in NAMES
    for rank in sorted(pair):
        assert pair[rank][name] == "ok", f"rank {rank}: {pair[rank][name]}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_replicas_after_broadcast(pair, dtype):
    """Parameters, buffers and an eval forward of one common input (so the packed images too) are bit-equal across ranks."""
    _entry(pair, "replicas_after_broadcast", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_plain_step(pair, dtype):
    """Averaged gradients == replay, views of one flat buffer, every element exchanged once; p, m, v and the next forward
    after FusedAdam.step() == replay == the other rank."""
    _entry(pair, "plain_step", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_recipe_step(pair, dtype):
    """AdamW + clipping (one step that clips, one that does not) + EMA: p, m, v, EMA, recipe_stats() and the 56-byte device
    record == replay == the other rank: the norm is the averaged gradient's."""
    _entry(pair, "recipe_step", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_rank_nonfinite(pair, dtype):
    """Rank 1 alone has an infinite loss: BOTH ranks drop the step (a norm taken before the exchange lets rank 0 step alone),
    and the step after it is a normal one."""
    _entry(pair, "one_rank_nonfinite", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_steps_reuse(pair, dtype):
    """Three rounds on one flat buffer (the wrapper keeps no view of it after finish()); gradients the caller keeps are never
    overwritten by the next round."""
    _entry(pair, "three_steps_reuse", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_last_batch(pair, dtype):
    """Batches of 2, 1, 2 with both engines alive: each step == its replay == the other rank."""
    _entry(pair, "ragged_last_batch", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_trace_does_not_disturb(pair, dtype):
    """start_trace() ... stop_trace() around a step (gloo, host clock): the same gradient bits, one closed step."""
    _entry(pair, "trace_does_not_disturb", dtype)


# ---------------------------------------------------------------------------------------------------------------- one-rank RCCL
def test_rccl_one_rank_forced_group_and_device_event_trace():
    """UNETDC_DP_FORCE=1: init_from_env() brings up a one-rank 'nccl' group on cuda:0; with single_rank_collectives the trace
    of two bf16 steps is taken with HIP events.  Orderings only: no timing value is asserted."""
    results, wall = cases.run_children(cases.rccl_worker, [(cases.free_port(),)], WAIT_RCCL)
    status, out = results[0] if not isinstance(results[0], str) else (results[0], None)
    print(f"\none-rank RCCL worker: wall {wall:.1f} s")
    assert status == "ok", status
    g = out["group"]
    assert g["initialised"] and g["backend"] == "nccl" and (g["rank"], g["local"], g["world"], g["device"]) == (0, 0, 1, 0), g
    res = out["trace"]
    assert res is not None and "HIP events" in res["clock"], res
    assert res["traced_steps"] == 2 and out["trace_off"], res
    assert res["exposed_ms_per_step"] >= 0.0, res
    assert [round(b["MB"], 1) for b in res["buckets"]] == cases.BUCKETS_MB, res["buckets"]
    assert all(0.0 <= b["ready_at_ms"] <= b["done_at_ms"] for b in res["buckets"]), res["buckets"]
    ready = [b["ready_at_ms"] for b in res["buckets"]]
    assert ready == sorted(ready), ready
    assert out["elems_per_step"] == out["nparams"], out
    assert out["steps_differ"], "the two steps gave the same gradients: the comparison below would say nothing about step 2"
    assert out["grads_equal"], "gradients of the traced steps differ from the untraced ones"


# ---------------------------------------------------------------------------------------------------------------- entry point
N_FILES = 13        # -> 2 test + 2 validation + 9 training images: an odd split, 4 per rank
RUNS = {
    "recipe": ["--img_size", "64", "--dtype", "bf16", "--epochs", "3", "--patience", "5", "--weight_decay", "0.01",
               "--clip_grad", "1.0", "--ema", "0.9", "--lr_schedule", "cosine", "--warmup_steps", "2"],
    "crop": ["--crop", "32", "--crops_per_image", "2", "--border_weight", "--dtype", "f32", "--epochs", "2"],
}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return cases.write_pairs(tmp_path_factory.mktemp("dp_step_data"), N_FILES)


def _argv(files, run, ckpt):
    return ["--image_dir", files[0], "--mask_dir", files[1], "--device_data", "--batch", "2", "--workers", "0",
            "--device", "cuda", "--ckpt_path", str(ckpt)] + RUNS[run]


@pytest.mark.parametrize("run", list(RUNS))
def test_train_entry_two_ranks_on_the_device(run, files, tmp_path):
    """train_DC_focal.main under two gloo ranks on cuda:0 with --device_data: both ranks run the same epochs with bit-equal
    parameters (param_checksum) and rank 0's validation Dice, the recipe's counters and the rate agree, rank 0 alone writes
    the checkpoint, and with --ema that checkpoint is not the live weights."""
    from models.model_2 import UNetDC
    ckpt = tmp_path / "best.pth"
    argv = _argv(files, run, ckpt)
    port = cases.free_port()
    results, wall = cases.run_children(cases.train_worker, [(r, 2, port, argv) for r in range(2)], WAIT_ENTRY)
    print(f"\nentry point, run '{run}': pair wall {wall:.1f} s")
    assert all(not isinstance(r, str) and r[1] == "ok" for r in results), results
    (_, _, h0, saves0), (_, _, h1, saves1) = sorted(results, key=lambda r: r[0])
    assert len(h0) == len(h1) == int(argv[argv.index("--epochs") + 1]), (len(h0), len(h1))
    for a, b in zip(h0, h1):
        assert a["param_checksum"] == b["param_checksum"], (a, b)          # replicas bit-identical after every epoch
        assert a["val_dice"] == b["val_dice"], (a, b)
        for key in ("clipped_steps", "skipped_steps", "lr"):
            assert (key in a) == (key in b) and a.get(key) == b.get(key), (key, a, b)
        for rec in (a, b):
            assert all(torch.isfinite(torch.tensor([rec["train_loss"], rec["val_loss"]]))), rec
    if run == "recipe":
        assert all(k in h0[0] for k in ("clipped_steps", "skipped_steps", "lr")), h0[0]
        assert sum(r["skipped_steps"] for r in h0) == 0, h0
    # the checkpoint: written by rank 0 alone, loads into a fresh module
    assert saves0 and set(saves0) == {str(ckpt)} and saves1 == [], (saves0, saves1)
    model = UNetDC(3, 1)
    model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True))
    with torch.no_grad():
        saved = float(sum(p.double().sum() for p in model.parameters()))
    best, rec_saved = 0.0, None
    for rec in h0:                                           # the epoch that wrote the file last (train_DC_focal.py's rule)
        if rec["val_dice"] > best:
            best, rec_saved = rec["val_dice"], rec
    live = rec_saved["param_checksum"]
    # fp64 sums of the same 31 M fp32 values in two orders (device, host) agree to ~1e-13 relative; an average that lags the
    # weights by even one Adam step of 1e-3 per element does not
    gap = abs(saved - live) / max(abs(live), 1.0)
    if run == "recipe":
        assert gap > 1e-9, (saved, live)                     # --ema: the averaged weights, not the live ones
    else:
        assert gap <= 1e-9, (saved, live)


@pytest.mark.parametrize("run", list(RUNS))
def test_device_loader_shards(run, files, tmp_path):
    """make_device_loaders(args, r, 2, device) without any collective: equal, disjoint shards, the ids range(r, 2 * per_rank,
    2) of the training split, cached exactly as the unsharded loader caches those rows."""
    import train_DC_focal as T
    args = T.build_parser().parse_args(_argv(files, run, tmp_path / "unused.pth"))
    dev = torch.device("cuda:0")
    full = T.make_device_loaders(args, 0, 1, dev)[0]
    n = len(full.dataset)
    assert n == 9 and full.ids == list(range(n))
    per_rank = n // 2
    shards = [T.make_device_loaders(args, r, 2, dev)[0] for r in range(2)]
    for r, sh in enumerate(shards):
        assert sh.ids == list(range(r, per_rank * 2, 2)) and len(sh.dataset) == per_rank
        assert sh.dataset.names == [full.dataset.names[i] for i in sh.ids]
        for j, i in enumerate(sh.ids):
            if run == "crop":
                assert torch.equal(sh.dataset.image(j), full.dataset.image(i)) and torch.equal(sh.dataset.mask(j), full.dataset.mask(i))
            else:
                assert torch.equal(sh.dataset.images[j], full.dataset.images[i])
                assert torch.equal(sh.dataset.masks[j], full.dataset.masks[i])
    assert len(shards[0]) == len(shards[1]) and not set(shards[0].ids) & set(shards[1].ids)
