"""Decode attention through the C ABI (t5g_attention_decode: the kernels the engine runs
every step) against the reference's attention numerics -- torch's CPU SDPA on bf16
([tf] T5GemmaSelfAttention :264-304 / PMCrossAttention :167-253), restated in
oracle/sdpa_emu.py and pinned bitwise to torch there -- and against exact fp64 softmax
attention, at the C3 lengths: self attention over L in {1, 63, 64, 65, 152, 527, 903}
keys (1 to 15 64-key chunks per (row, kv head), one or two aten 512-key blocks, ragged
rows in one launch) and cross attention over T_x = 60 encoder keys."""
import pytest
import torch

from tests.engine_cases import need_gpu
from tests.kernel_cases import decode_attention_call as _run
from tests.kernel_cases import decode_exact_attention as _exact

pytestmark = pytest.mark.gpu


def _reference(q, K, V, lens, scale, causal):
    """aten CPU SDPA numerics (oracle/sdpa_emu.py, pinned bitwise to torch here) per row
    over its first lens[b] keys; the query is the row's last key."""
    from oracle import sdpa_emu
    B, Hq, D = q.shape
    out = torch.zeros(B, Hq, D, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        out[b] = sdpa_emu.attention(q[b][:, None], K[b, :, :L], V[b, :, :L], scale)[:, 0].double()
    return out


@pytest.mark.parametrize("L", [1, 63, 64, 65, 152, 527, 903, 1500, 2100, 6000])
def test_self_attention_decode_vs_cpu_sdpa(L):
    """8 rows x 8 q heads / 4 kv heads x 256 (2b-2b), ragged lengths up to L: rows of > 64
    keys go through the two-launch path (scores, then P.V / combine: one pass for rows of
    <= 1024 keys, the block loop beyond), the others one launch. Bit-equal to aten's CPU
    SDPA numerics except fp32 GEMM-order flips (<= 1 ulp)."""
    need_gpu()
    B = 8
    lens = [L, max(1, L - 1), max(1, L // 2), max(1, L - 64), 1, max(1, L - 3), max(1, (3 * L) // 4), L]
    got, q, K, V = _run(L, B, lens, seed=L)
    ref = _reference(q, K, V, lens, 256 ** -0.5, True)
    exact = _exact(q, K, V, lens, 256 ** -0.5)
    same = (got == ref).float().mean().item()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -60))) - 7)
    within1 = ((got - ref).abs() <= ulp * 1.01).float().mean().item()
    print(f"L={L}: bit-equal to CPU SDPA {same:.5f}, within 1 ulp {within1:.5f}, max |err| vs exact "
          f"{(got - exact).abs().max().item():.3g}")
    # past two aten blocks (L > 1024; the C3 rows stay below 911 keys) the P.V order that
    # is not pinned to aten (fp32 sums within a block) compounds over the block rescales:
    # a few more outputs land 2 ulps off, none far from the exact value
    assert same >= 0.998 and within1 >= (0.9999 if L <= 1024 else 0.9995), (same, within1)
    assert (got - exact).abs().max().item() <= 2.0 ** -6 * max(1.0, exact.abs().max().item())


def test_self_attention_decode_batch32():
    """32 rows (the C5 batch): the P.V / combine launch takes 64-dimension slices (one
    round of workgroups); the same CPU-SDPA bit-equality as at 8 rows."""
    need_gpu()
    B, L = 32, 527
    lens = [max(1, L - 17 * i) for i in range(B)]
    got, q, K, V = _run(L, B, lens, seed=32)
    ref = _reference(q, K, V, lens, 256 ** -0.5, True)
    same = (got == ref).float().mean().item()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -60))) - 7)
    within1 = ((got - ref).abs() <= ulp * 1.01).float().mean().item()
    print(f"B=32 L<={L}: bit-equal to CPU SDPA {same:.5f}, within 1 ulp {within1:.5f}")
    assert same >= 0.998 and within1 >= 0.9999, (same, within1)


def test_cross_attention_decode_tx60():
    """PMCrossAttention shape: T_x = 60 encoder keys (non-causal), 8 rows, ragged text."""
    need_gpu()
    B, T = 8, 60
    lens = [60, 59, 33, 1, 60, 17, 48, 60]
    got, q, K, V = _run(T, B, lens, causal=0, seed=60)
    ref = _reference(q, K, V, lens, 256 ** -0.5, False)
    same = (got == ref).float().mean().item()
    print(f"cross T_x=60: bit-equal to CPU SDPA {same:.5f}")
    assert same >= 0.998, same


@pytest.mark.parametrize("L,B", [(65, 8), (152, 8), (527, 8), (903, 8), (2100, 8), (527, 32),
                                 # past 64 chunks of 64 keys: the combine's lanes own several
                                 # chunks (a 100 s prompt + a 120 s target is ~11 250 keys)
                                 (6000, 8), (12288, 4)])
def test_self_attention_decode_flash(L, B):
    """The fast path's one-launch form (t5g_attention_decode_flash: per-chunk online-softmax
    partials, combined by the last chunk to arrive) against exact fp64 attention over the
    same bf16 inputs. Rows of <= 64 keys take the aten-order kernel (bit-equal to CPU SDPA).
    Tolerance: 2^-7 relative to max |exact| per output (fast-mode numerics: bf16 p, fp32
    sums in a different order, bf16 output), and a mean error no larger than 1.5x that of
    the aten-order form on the same inputs."""
    need_gpu()
    lens = [max(1, L - (L // B) * i) for i in range(B)]
    lens[1] = 1
    lens[2] = min(L, 64)
    got, q, K, V = _run(L, B, lens, seed=L + B, flash=True)
    base, _, _, _ = _run(L, B, lens, seed=L + B, flash=False)
    exact = _exact(q, K, V, lens, 256 ** -0.5)
    err = (got - exact).abs()
    err_base = (base - exact).abs()
    print(f"flash L<={L} B={B}: max |err| {err.max().item():.3g} (aten-order {err_base.max().item():.3g}), "
          f"mean {err.mean().item():.3g} ({err_base.mean().item():.3g})")
    assert err.max().item() <= 2.0 ** -7 * max(1.0, exact.abs().max().item())
    assert err.mean().item() <= 1.5 * err_base.mean().item() + 1e-6
    # rows of <= 64 keys: the same kernel path as the aten-order form, bit-equal
    small = [b for b in range(B) if lens[b] <= 64]
    assert torch.equal(got[small], base[small])
