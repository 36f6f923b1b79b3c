"""The data-parallel step against its one-process replay (tests/dp_step_cases.py) on the ATen-CPU path: two gloo ranks,
sync_gradients() for the exchange, FusedAdam._step_torch for the step.  The same scenarios as tests/test_gpu_dp_step.py, so
the harness runs on a host without a GPU; what belongs to the HIP path alone -- the flat buffer and its reuse, the packed
weight images, the device record -- is not in this list (dp_step_cases.scenario_ids("cpu")) or sits behind the HIP branch of
a scenario: nothing is skipped at run time."""
import pytest

from tests import dp_step_cases as cases

NAMES = cases.scenario_ids("cpu")
WAIT = 600          # seconds for the pair as a whole: interpreter start, torch import and ~25 small CPU steps


@pytest.fixture(scope="module")
def pair():
    results, wall, timings = cases.run_pair("cpu", NAMES, WAIT)
    print(f"\ndata-parallel step on CPU tensors: pair wall {wall:.1f} s; rank 0: "
          f"{ {k: round(v, 1) for k, v in timings.get(0, {}).items()} }")
    return results


def test_the_cpu_list_leaves_out_what_needs_the_hip_path():
    assert "three_steps_reuse[f32]" not in NAMES and "three_steps_reuse[f32]" in cases.scenario_ids("cuda")
    assert all(n.endswith("[f32]") for n in NAMES) and len(NAMES) == 6


def _entry(pair, name):
    """A scenario that did not run is a failure like any other."""
    assert name in NAMES
    for rank in sorted(pair):
        assert pair[rank][name] == "ok", f"rank {rank}: {pair[rank][name]}"


def test_replicas_after_broadcast(pair):
    _entry(pair, "replicas_after_broadcast[f32]")


def test_plain_step(pair):
    _entry(pair, "plain_step[f32]")


def test_recipe_step(pair):
    _entry(pair, "recipe_step[f32]")


def test_one_rank_nonfinite(pair):
    _entry(pair, "one_rank_nonfinite[f32]")


def test_ragged_last_batch(pair):
    _entry(pair, "ragged_last_batch[f32]")


def test_trace_does_not_disturb(pair):
    _entry(pair, "trace_does_not_disturb[f32]")
