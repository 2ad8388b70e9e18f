"""Decode attention through the C ABI (t5g_attention_decode: the kernels the engine runs
every step) against the reference's attention numerics -- torch's CPU SDPA on bf16
([tf] T5GemmaSelfAttention :264-304 / PMCrossAttention :167-253), restated in
oracle/sdpa_emu.py and pinned bitwise to torch there -- and against exact fp64 softmax
attention, at the C3 lengths: self attention over L in {1, 63, 64, 65, 152, 527, 903}
keys (1 to 15 64-key chunks per (row, kv head), one or two aten 512-key blocks, ragged
rows in one launch) and cross attention over T_x = 60 encoder keys."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


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


def _exact(q, K, V, lens, scale, window=0):
    """fp64 softmax attention of each row's query (at position lens[b] - 1) over its keys
    [lo, lens[b]), lo = max(0, lens[b] - window) for a sliding window, else 0."""
    B, Hq, D = q.shape
    G = Hq // K.shape[1]
    out = torch.zeros(B, Hq, D, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        lo = max(0, L - window) if window > 0 else 0
        for h in range(Hq):
            s = (K[b, h // G, lo:L].double() @ q[b, h].double()) * scale
            out[b, h] = torch.softmax(s, 0) @ V[b, h // G, lo:L].double()
    return out


def _run(L, B, lens, Hq=8, Hkv=4, D=256, causal=1, seed=0, flash=False, window=0, cap=None, prepare=None,
         want_rc=0):
    """One t5g_attention_decode(_flash) call on random bf16 q / K / V; returns the output
    (fp64, [B][Hq][D]) and the host inputs. cap: cache slots per (row, kv head), default L;
    prepare(q, K, V) edits the inputs in place before the upload; want_rc != 0: the call must
    return that status and write nothing (returns None)."""
    from t5gemma_tts_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(seed)
    cap = L if cap is None else cap
    q = torch.randn(B, Hq, D, generator=g).to(BF16)
    K = torch.randn(B, Hkv, cap, D, generator=g).to(BF16)
    V = torch.randn(B, Hkv, cap, D, generator=g).to(BF16)
    if prepare is not None:
        prepare(q, K, V)
    dev = "cuda"
    qd, Kd, Vd = q.to(dev), K.to(dev), V.to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.zeros(B, Hq * D, dtype=BF16, device=dev)
    nb = lib.t5g_attention_decode_work_bytes(B, Hq, Hkv, D, cap)
    assert nb > 0
    work = torch.zeros(nb // 4, dtype=torch.float32, device=dev)   # flash: tickets start at zero
    a = _lib.AttnDecodeArgs(B=B, n_heads=Hq, n_kv_heads=Hkv, head_dim=D, q=qd.data_ptr(), k_cache=Kd.data_ptr(),
                            v_cache=Vd.data_ptr(), cap=cap, kv_len=lens_d.data_ptr(), causal=causal, window=window,
                            scale=D ** -0.5, out=out.data_ptr(), work=work.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = lib.t5g_attention_decode_flash if flash else lib.t5g_attention_decode
    if want_rc != 0:
        assert fn(C.byref(a), st) == want_rc
        torch.cuda.synchronize()
        assert int((out != 0).sum().item()) == 0 and int((work != 0).sum().item()) == 0   # nothing launched
        return None
    _lib.check(fn(C.byref(a), st), "attention_decode")
    torch.cuda.synchronize()
    got = out.cpu().view(B, Hq, D).double()
    if flash:   # the tickets are left at zero for the next call
        nt = B * Hkv
        assert int(work[-nt:].view(torch.int32).abs().sum().item()) == 0
    return got, q, K, V


@pytest.mark.parametrize("L", [1, 63, 64, 65, 152, 527, 903, 1500, 2100, 6000])
def test_self_attention_decode_vs_cpu_sdpa(L):
    """8 rows x 8 q heads / 4 kv heads x 256 (2b-2b), ragged lengths up to L: rows of > 64
    keys go through the two-launch path (scores, then P.V / combine: one pass for rows of
    <= 1024 keys, the block loop beyond), the others one launch. Bit-equal to aten's CPU
    SDPA numerics except fp32 GEMM-order flips (<= 1 ulp)."""
    _need_gpu()
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
    _need_gpu()
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
    _need_gpu()
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
    _need_gpu()
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
