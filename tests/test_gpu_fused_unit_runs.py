"""The whole-layer decode launch with waves 8-10 of the workers that run no attention requesting
their share of the run's gate/up register units in the attention window (csrc/fused_kernels.h: with
the LDS copies, crossing cross-o on its barriers alone), against the per-op launches at the true
2b-2b widths (2 + 2 layers). Row counts: 1 (8 attention workers of 255), 3, 8 (the benchmark's
map: 64 attention workers, 96 + 88 others with 5 / 4 units), 12 (176 workers with 5 units: 96
attention workers and 80 of the 148 others), 13 (an odd count) and 16 (the one-tile limit: 128
attention and 112 other workers), in the three stage-S placements. Tokens and every recorded
logit row are compared on their bits;
repeated fused runs in one engine must agree with each other as well (a barrier crossed with
the wrong thing in flight shows as a run-to-run difference)."""
import functools

import pytest

from tests.engine_cases import assert_same_run, both_loops, mid_engine, need_gpu, utterances

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _engine():
    return mid_engine(16)


def _case(B):
    cfg, eng = _engine()
    return eng, utterances(cfg, B, 150 + B), list(range(900, 900 + B))


@functools.lru_cache(maxsize=None)
def _per_op(B):
    """(host, fast) of the per-op launches for the B-row case, run once."""
    eng, utts, seeds = _case(B)
    eng.set_fused(False)
    return both_loops(eng, utts, seeds)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B", [1, 3, 8, 12, 13, 16])
def test_unit_runs_bitwise_equal_to_per_op_launches(B, mode):
    need_gpu()
    ref_host, ref_fast = _per_op(B)
    eng, utts, seeds = _case(B)
    eng.set_attn_in_block(mode)   # stage S: 0 the separate flash launch, 1 in front, 2 at the end
    eng.set_fused(True)
    host, fast = both_loops(eng, utts, seeds)
    assert_same_run(host, ref_host, B, ("host", B, mode))
    assert_same_run(fast, ref_fast, B, ("graph", B, mode))
    assert sum(len(g) for g in host["gen"]) > B


@pytest.mark.parametrize("B", [8, 16])
def test_unit_runs_run_to_run(B):
    need_gpu()
    eng, utts, seeds = _case(B)
    eng.set_attn_in_block(2)
    eng.set_fused(True)
    runs = [both_loops(eng, utts, seeds) for _ in range(3)]
    for k in (1, 2):
        assert_same_run(runs[k][0], runs[0][0], B, ("host", B, k))
        assert_same_run(runs[k][1], runs[0][1], B, ("graph", B, k))
    assert sum(len(g) for g in runs[0][0]["gen"]) > B
