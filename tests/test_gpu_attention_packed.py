"""The fast path's many-query attention (csrc/attn.hip attn_kernel<D, G, EAGER>: encoder self
attention with a bidirectional window, decoder prefill self attention with a causal window,
prefill cross attention) through t5g_attention_packed, against exact fp64 softmax attention
over the same bf16 inputs at the project's bound for the aten-order form,
max |err| <= 2^-6 max(1, max |exact|) (tests/test_gpu_attention.py).

The kernel states its three key ranges itself -- causal `lo = max(0, t - W + 1)`, bidirectional
`lo = max(0, t - W)` and `hi = min(len, t + W + 1)` -- and counts its 512-key blocks from lo.
The window tests plant one marker key per query on either side of an edge (the method of
tests/test_gpu_attention_window.py); their teeth are asserted from the reference alone.

Printed, not asserted: the bit-equal rate against oracle/sdpa_emu.attention (aten's CPU SDPA
order, which this kernel follows) for the un-windowed causal and cross cases.
"""
import ctypes as C
import functools

import pytest
import torch

from tests import kernel_cases as kc
from tests.engine_cases import need_gpu
from tests.kernel_cases import BF16
from tests.kernel_cases import attn_bound as _bound
from tests.kernel_cases import attn_inputs as _inputs
from tests.kernel_cases import exact_attention as _exact

pytestmark = pytest.mark.gpu


def _run(q, K, V, lens, rows, pos, causal, window=0, softcap=0.0):
    """One t5g_attention_packed call; the raw bf16 output [Mq][Hq][D] (host). The output buffer
    starts as NaN: a query the launch skips or half writes shows."""
    from t5gemma_tts_amd import _lib
    Mq, Hq, D = q.shape
    B, Hkv, cap, _ = K.shape
    dev = "cuda"
    qd, Kd, Vd = q.to(dev), K.to(dev), V.to(dev)
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    rd = torch.tensor(rows, dtype=torch.int32, device=dev)
    pd = torch.tensor(pos, dtype=torch.int32, device=dev)
    out = torch.full((Mq, Hq * D), float("nan"), dtype=BF16, device=dev)
    a = _lib.AttnPackedArgs(Mq=Mq, n_heads=Hq, n_kv_heads=Hkv, head_dim=D, q=qd.data_ptr(), q_row=rd.data_ptr(),
                            q_pos=pd.data_ptr(), k_cache=Kd.data_ptr(), v_cache=Vd.data_ptr(), kv_len=ld.data_ptr(),
                            cap=cap, causal=causal, window=window, scale=D ** -0.5, softcap=softcap,
                            out=out.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().t5g_attention_packed(C.byref(a), st), "attention_packed")
    torch.cuda.synchronize()
    return out.cpu().view(Mq, Hq, D)


def _emu_rate(got, q, K, V, lens, rows, pos, causal):
    """Share of outputs bit-equal to oracle/sdpa_emu.attention, row by row. A causal row is one
    aten call of lens[b] queries (its q-block split depends on that count): the given queries at
    their positions, zeros at the others."""
    from oracle import sdpa_emu
    same = n = 0
    for b in sorted(set(rows)):
        idx = [i for i in range(len(rows)) if rows[i] == b]
        L = lens[b]
        if causal:
            qf = torch.zeros(q.shape[1], L, q.shape[2], dtype=BF16)
            for i in idx:
                qf[:, pos[i]] = q[i]
            ref = sdpa_emu.attention(qf, K[b, :, :L], V[b, :, :L], q.shape[2] ** -0.5, is_causal=True)
            ref = torch.stack([ref[:, pos[i]] for i in idx])
        else:
            ref = sdpa_emu.attention(q[idx].transpose(0, 1), K[b, :, :L], V[b, :, :L], q.shape[2] ** -0.5)
            ref = ref.transpose(0, 1)
        same += int((got[idx] == ref).sum())
        n += ref.numel()
    return same / n


# ---------------------------------------------------------------------------
# prefill: every position a query
PREFILL_LENS = [1, 70, 200]


@functools.lru_cache(maxsize=None)
def _prefill_case():
    rows = [b for b, L in enumerate(PREFILL_LENS) for _ in range(L)]
    pos = [t for L in PREFILL_LENS for t in range(L)]
    q, K, V = _inputs(11, len(rows), 8, 4, 256, 3, 256)
    for b, L in enumerate(PREFILL_LENS):   # as test_cap_larger_than_rows: a stride or bound slip shows
        K[b, :, L:] = 1e4
        V[b, :, L:] = float("nan")
    return q, K, V, rows, pos


def test_prefill_every_position():
    """8 q / 4 kv heads x 256, rows of 1, 70 and 200 keys in a cache of 256 slots, causal: all
    271 positions in one launch. The unused slots hold K = 1e4 and V = NaN."""
    need_gpu()
    q, K, V, rows, pos = _prefill_case()
    got = _run(q, K, V, PREFILL_LENS, rows, pos, causal=1)
    exact = _exact(q, K, V, PREFILL_LENS, rows, pos, 256 ** -0.5, True)
    err = (got.double() - exact).abs().max().item()
    rate = _emu_rate(got, q, K, V, PREFILL_LENS, rows, pos, True)
    print(f"prefill rows {PREFILL_LENS}: max |err| vs fp64 {err:.3g}, bound {_bound(exact):.3g}, "
          f"bit-equal to sdpa_emu {rate:.5f} (not asserted)")
    assert not torch.isnan(got).any()
    assert err <= _bound(exact)


def test_batch_invariance():
    """A query launched alone is bitwise the same query inside the packed batch (one workgroup
    per (query, kv head), nothing shared between queries)."""
    need_gpu()
    q, K, V, rows, pos = _prefill_case()
    got = _run(q, K, V, PREFILL_LENS, rows, pos, causal=1)
    for i in (0, 1 + 69, 1 + 70 + 131):
        alone = _run(q[i:i + 1], K, V, PREFILL_LENS, rows[i:i + 1], pos[i:i + 1], causal=1)
        assert torch.equal(alone[0].view(torch.int16), got[i].view(torch.int16)), (rows[i], pos[i])


# ---------------------------------------------------------------------------
# window edges (the cases and their reference-only teeth: tests/kernel_cases.py window_case)
@pytest.mark.parametrize("W", [24, 64])
@pytest.mark.parametrize("causal", [1, 0], ids=["causal", "bidirectional"])
def test_window_edges(causal, W):
    """Causal (decoder prefill): a key at t - W must not count, a key at t - W + 1 must, for
    queries in mid row, at t = W - 1 and at t = W. Bidirectional (the encoder's |t - k| <= W):
    keys at t - W - 1 / t - W and t + W + 1 / t + W, for queries in mid row, with t < W, with
    t + W >= len, and in rows shorter than the window. Ragged rows in a larger cache."""
    need_gpu()
    q, K, V, lens, rows, pos, exact, bound, move = kc.window_case(causal, W)
    got = _run(q, K, V, lens, rows, pos, causal, W)
    err = (got.double() - exact).abs().amax(dim=(1, 2))
    print(f"causal={causal} W={W}: max |err| vs fp64 {err.max().item():.3g}, bound {bound:.3g}, "
          f"smallest reference shift of a marker at W +- 1: {move:.3g}")
    assert not torch.isnan(got).any()
    assert err.max().item() <= bound, err.tolist()


# ---------------------------------------------------------------------------
def test_cross_attention_ignores_query_positions():
    """Prefill cross attention: non-causal, no window, text rows of 60, 1 and 33 keys; the query
    positions are audio positions (up to 200, past every kv_len) and must not matter."""
    need_gpu()
    lens = [60, 1, 33]
    rows = [0] * 7 + [1] * 4 + [2] * 6
    pos = [0, 59, 60, 61, 150, 200, 7, 0, 1, 90, 200, 0, 32, 33, 34, 120, 200]
    q, K, V = _inputs(60, len(rows), 8, 4, 256, 3, 64)
    for b, L in enumerate(lens):
        K[b, :, L:] = 1e4
        V[b, :, L:] = float("nan")
    got = _run(q, K, V, lens, rows, pos, causal=0)
    exact = _exact(q, K, V, lens, rows, pos, 256 ** -0.5, False)
    err = (got.double() - exact).abs().max().item()
    rate = _emu_rate(got, q, K, V, lens, rows, pos, False)
    print(f"cross rows {lens}: max |err| vs fp64 {err:.3g}, bound {_bound(exact):.3g}, "
          f"bit-equal to sdpa_emu {rate:.5f} (not asserted)")
    assert not torch.isnan(got).any()
    assert err <= _bound(exact)
    zero = _run(q, K, V, lens, rows, [0] * len(rows), causal=0)
    assert torch.equal(zero.view(torch.int16), got.view(torch.int16))


# ---------------------------------------------------------------------------
def test_several_aten_blocks():
    """One row of 1 100 keys, keys with scores about +8 and +9 planted in the second and third
    512-key block (kernel_cases.blocks_case): causal queries on both sides of the block edges
    and of the planted keys."""
    need_gpu()
    q, K, V = kc.blocks_case()
    T = kc.BLOCK_T
    lens, rows, scale = [kc.BLOCK_LEN], [0] * len(T), 256 ** -0.5
    s700, s1060 = kc.planted_scores()
    assert 6.5 <= s700 <= 9.5 and s700 + 0.5 <= s1060 <= 11, (s700, s1060)
    got = _run(q, K, V, lens, rows, T, causal=1)
    exact = _exact(q, K, V, lens, rows, T, scale, True)
    err = (got.double() - exact).abs().max().item()
    rate = _emu_rate(got, q, K, V, lens, rows, T, True)
    print(f"1100 keys, t in {T}: planted scores {s700:.2f} / {s1060:.2f}, max |err| vs fp64 {err:.3g}, "
          f"bound {_bound(exact):.3g}, bit-equal to sdpa_emu {rate:.5f} (not asserted)")
    assert err <= _bound(exact)


@pytest.mark.parametrize("window", kc.BLOCK_WINDOWS)
def test_blocks_counted_from_lo(window):
    """The same row's last query (t = 1099) under a window, so that lo is no multiple of 512 and
    the kernel's blocks are counted from lo. Window 600: lo = 500, blocks [500, 1012) and
    [1012, 1100). Window 560: lo = 540, the block edge at key 1052, where (j0 - lo) / 512 = 1
    but j0 / 512 = 2 -- an index that forgets lo reads another slot. The planted keys fall in
    the first and second block either way, so the rescale matters: losing it moves the
    reference by ten times the bound (asserted in kernel_cases.blocks_window_case)."""
    need_gpu()
    q, K, V = kc.blocks_case()
    qi, exact, bound, shift = kc.blocks_window_case(window)
    got = _run(qi, K, V, [kc.BLOCK_LEN], [0], [kc.BLOCK_LEN - 1], causal=1, window=window)
    err = (got.double() - exact).abs().max().item()
    print(f"window {window} at t = 1099 (lo = {kc.BLOCK_LEN - window}): max |err| vs fp64 {err:.3g}, bound {bound:.3g}, "
          f"a lost block rescale moves the reference by {shift:.3g}")
    assert err <= bound


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,G", [(256, 2), (64, 2), (128, 2), (256, 1)])
def test_all_instantiated_geometries(D, G):
    """Every (head_dim, group) attention() instantiates, with 2 and 4 kv heads, causal and
    bidirectional, window 0 and 50; ragged rows up to 200 keys, 14 queries."""
    need_gpu()
    lens = [200, 1, 65, 137]
    rows = [0, 0, 0, 0, 0, 1, 2, 2, 2, 2, 3, 3, 3, 3]
    pos = [0, 49, 50, 120, 199, 0, 0, 13, 51, 64, 0, 68, 100, 136]
    for Hkv in (2, 4):
        q, K, V = _inputs(D + G + Hkv, len(rows), G * Hkv, Hkv, D, 4, 200)
        for causal in (1, 0):
            for window in (0, 50):
                got = _run(q, K, V, lens, rows, pos, causal, window)
                exact = _exact(q, K, V, lens, rows, pos, D ** -0.5, causal, window)
                err = (got.double() - exact).abs().max().item()
                print(f"D={D} G={G} Hkv={Hkv} causal={causal} window={window}: max |err| vs fp64 {err:.3g}, "
                      f"bound {_bound(exact):.3g}")
                assert err <= _bound(exact), (Hkv, causal, window)


def test_rows_past_8192_keys():
    """8 200 score slots at G = 2 are 65 600 bytes of LDS: the launch that opts in to 96 KiB.
    One row, one kv head; t = 8 199 reads every slot. The same query under a window of 5 000."""
    need_gpu()
    cap = 8200
    q, K, V = _inputs(8200, 3, 2, 1, 256, 1, cap)
    lens, rows, pos, scale = [cap], [0, 0, 0], [0, 4100, cap - 1], 256 ** -0.5
    got = _run(q, K, V, lens, rows, pos, causal=1)
    exact = _exact(q, K, V, lens, rows, pos, scale, True)
    err = (got.double() - exact).abs().max().item()
    gw = _run(q[2:], K, V, lens, [0], [cap - 1], causal=1, window=5000)
    ew = _exact(q[2:], K, V, lens, [0], [cap - 1], scale, True, 5000)
    errw = (gw.double() - ew).abs().max().item()
    print(f"cap 8200: max |err| vs fp64 {err:.3g} (bound {_bound(exact):.3g}), window 5000: {errw:.3g} "
          f"(bound {_bound(ew):.3g})")
    assert err <= _bound(exact) and errw <= _bound(ew)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 256])
def test_eager_softcap(D):
    """softcap 50 selects the eager variant (bf16 scores, tanh softcap, bf16 normalised
    probabilities), so the fp64 bound above does not apply. Yardstick: a CPU restatement of
    eager_attention_forward in torch bf16 ops (oracle/t5g_oracle.attention, impl="eager") has
    its own error against fp64 on the same inputs; the kernel's different sum order draws
    independent roundings of the same size, so its error may be up to twice that."""
    need_gpu()
    from oracle import t5g_oracle
    L, Hq, Hkv = 100, 4, 2
    q, K, V = _inputs(50 + D, L, Hq, Hkv, D, 1, L)
    rows, pos, scale = [0] * L, list(range(L)), D ** -0.5
    kw = dict(scale=scale, softcap=50.0, n_rep=Hq // Hkv, mask=None, is_causal=True, impl="eager")
    restated = t5g_oracle.attention(q.transpose(0, 1)[None], K, V, **kw)[0].view(L, Hq, D)
    exact = _exact(q, K, V, [L], rows, pos, scale, True, softcap=50.0)
    got = _run(q, K, V, [L], rows, pos, causal=1, softcap=50.0)
    err_r = (restated.double() - exact).abs().max().item()
    err_k = (got.double() - exact).abs().max().item()
    print(f"eager D={D}: kernel max |err| vs fp64 {err_k:.3g}, bf16 restatement's own {err_r:.3g} (bound 2x)")
    assert not torch.isnan(got).any()
    assert err_k <= 2 * err_r
