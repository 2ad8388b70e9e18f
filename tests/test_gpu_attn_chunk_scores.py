"""The fast path's chunk scores at the 2b-2b head geometry (8 q / 4 kv heads x 256), where a key's
two heads are reduced together (csrc/common.h xsum2_v32, in attn.hip's flash launch and in
fused_attn.h's stage S: the adds of the lane-split butterfly per head), through
t5g_attention_decode_flash against exact fp64 attention and the aten-order form
(t5g_attention_decode) on the same inputs: at the chunk edges, with chunks that start at an
arbitrary key (a sliding window), with NaN in the cache slots past each row's length, with a
peaked softmax; and inside the engine, rows crossing the 64-key boundary (one-chunk aten-order
path -> flash chunks) mid-call, the three placements of the attention bitwise equal. Bounds
(tests/test_gpu_attention.py's flash bounds): max |err| <= 2^-7 max(1, max |exact|), mean
error <= 1.5 x the aten-order form's; rows of <= 64 keys equal the aten-order form bit for
bit. Reference: [tf] modeling_t5gemma.py:264-304."""
import numpy as np
import pytest
import torch

from tests.engine_cases import assert_same_run, both_loops, mid_config, need_gpu
from tests.kernel_cases import decode_attention_call as _run
from tests.kernel_cases import decode_exact_attention as _exact

pytestmark = pytest.mark.gpu
SCALE = 256 ** -0.5


def _check(tag, L, lens, seed, window=0, cap=None, prepare=None):
    """Flash and aten-order form on the same inputs against fp64 attention: the flash bounds,
    and the rows of one chunk (<= 64 keys in the window) bit for bit."""
    B = len(lens)
    got, q, K, V = _run(L, B, lens, seed=seed, flash=True, window=window, cap=cap, prepare=prepare)
    base, _, _, _ = _run(L, B, lens, seed=seed, flash=False, window=window, cap=cap, prepare=prepare)
    exact = _exact(q, K, V, lens, SCALE, window=window)
    err = (got - exact).abs()
    err_base = (base - exact).abs()
    print(f"{tag}: max |err| {err.max().item():.3g} (aten-order {err_base.max().item():.3g}), "
          f"mean {err.mean().item():.3g} ({err_base.mean().item():.3g}), max |exact| {exact.abs().max().item():.3g}")
    assert bool(torch.isfinite(got).all()), tag
    assert err.max().item() <= 2.0 ** -7 * max(1.0, exact.abs().max().item()), tag
    assert err.mean().item() <= 1.5 * err_base.mean().item() + 1e-6, tag
    small = [b for b in range(B) if (min(lens[b], window) if window > 0 else lens[b]) <= 64]
    assert torch.equal(got[small], base[small]), tag


@pytest.mark.parametrize("L", [65, 128, 191])
def test_chunk_edges(L):
    """Rows of 1, 64 (one chunk, aten-order path), 65 (a second chunk of one key) and L keys
    (L = 128: two full chunks, 191: a last chunk of 63) in one launch."""
    need_gpu()
    _check(f"edges L={L}", L, [L, 65, 64, 1], seed=L)


def test_unaligned_chunk_start():
    """A 100-key sliding window: the chunks start at t - 99, so a row's chunks begin at an
    arbitrary key (and its second chunk holds 36 keys)."""
    need_gpu()
    _check("window 100", 300, [300, 251, 101, 64], seed=300, window=100)


def test_masked_keys_never_leak():
    """70 cache slots past the longest row, every slot past a row's length NaN in K and V:
    no key past the row's last one reaches a score or an output."""
    need_gpu()
    L, lens = 191, [191, 130, 65, 64]

    def prepare(q, K, V):
        for b, n in enumerate(lens):
            K[b, :, n:] = float("nan")
            V[b, :, n:] = float("nan")

    _check("NaN past len", L, lens, seed=7, cap=L + 70, prepare=prepare)


def test_peaked_softmax():
    """q and K scaled by 8 (scores 64 times as large: one key takes nearly all the weight)."""
    need_gpu()

    def prepare(q, K, V):
        q.mul_(8.0)
        K.mul_(8.0)

    _check("peaked", 191, [191, 128, 65, 64], seed=11, prepare=prepare)


def test_single_to_multi_transition_in_engine():
    """golden_mid (2 + 2 layers at the 2b-2b widths), 8 rows with prompts of 58-66 codes, 12
    generated tokens: the rows cross 64 keys mid-call. The separate flash launch (mode 0) and
    stage S in front (1) and at the end (2) give the same tokens and bitwise the same logits,
    and a second run of mode 2 repeats the first."""
    need_gpu()
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine, Utterance
    cfg, sd = mid_config()
    # not engine_cases.mid_engine: max_gen 14
    eng = T5GemmaTTSEngine(cfg, sd, device="cuda:0", max_batch=8, max_text=64, max_audio=128, max_gen=14)
    rng = np.random.default_rng(5866)
    B = 8
    utts = []
    for i in range(B):
        tp = 58 + i + (i == 7)   # 58 .. 64, 66 codes
        x = rng.integers(3, 4000, size=int(rng.integers(4, 40))).tolist()
        utts.append(Utterance(x=x, y=rng.integers(0, 65536, size=tp).tolist() + [cfg.y_sep_token],
                              tgt_y_len=tp + 1 + 12))
    seeds = list(range(700, 700 + B))

    def run(mode):
        eng.set_attn_in_block(mode)   # 0 the separate flash launch, 1 stage S in front, 2 at the end
        before = eng.attn_in_block_launches()
        out, fast = both_loops(eng, utts, seeds)
        return out, fast, eng.attn_in_block_launches() - before

    def same(a, b, tag):
        assert_same_run(a, b, B, tag)

    o2, f2, n2 = run(2)
    o0, f0, n0 = run(0)
    o1, f1, n1 = run(1)
    o2b, f2b, n2b = run(2)
    assert n0 == 0 and n1 > 0 and n2 > 0 and n2b > 0   # stage S ran, and only when enabled
    print("generated", [len(g) for g in o2["gen"]])
    # (rows 0-4 start at <= 63 keys: one of them generated its way past 64)
    assert max(len(o2["gen"][r]) for r in range(5)) >= 7
    same(o2, o0, "2/0")
    same(o1, o0, "1/0")
    same(o2, o2b, "2/2")
    same(f2, f0, "graph 2/0")
    same(f1, f0, "graph 1/0")
    same(f2, f2b, "graph 2/2")
