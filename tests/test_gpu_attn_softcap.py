"""The fast path's decode attention on an eager checkpoint's score (softcap 50): csrc/common.h
fast_score -- bf16(q.k), bf16(x scale), bf16(/ softcap), bf16(tanh), bf16(x softcap) -- at its two
call sites in csrc/attn.hip (the two-heads-per-key reduction of the flash launch at 8 q / 4 kv
heads x 256, and the general one), through t5g_attention_decode and t5g_attention_decode_flash with
the softcap field of t5g_attn_decode_args, against fp64 softmax and P.V over the scores of
fast_score restated in torch (tests/kernel_cases.py fast_score_ref; the fp64 formula
softcap * tanh(s * scale / softcap) is 0.04 - 0.06 away on the marked heads, more than the
flash bound). Reference: [tf] eager_attention_forward, modeling_t5gemma.py:216-221.

Inputs: randn plus two planted keys per (row, kv head) along the group's first query, scaled
scores 50 and 53 (V = +4 / -4): about 38 and 39.25 after the softcap, so the marked heads'
outputs (-2.22) hang on the softcap's value there. tests/test_kernel_cases_cpu.py asserts on the
CPU, from the references alone, that a dropped softcap or one applied after the scale moves every
marked head by ten times the bound, that a lost last rounding moves them by 1.5 bounds, and that
every marker's score is far enough from a bf16 tie at all five rounding points for the kernel's
fp32 sum order not to matter. The two spread cases give every (row, kv head) its own marker
scores, so that each of the five roundings, left out, moves some marked head by 4 bounds
(head_dim 128; at 256 the scale is a power of two and the first two roundings are one).

Bounds, the project's own for these kernels (tests/test_gpu_attention.py), against the restated
reference: aten-order form max |err| <= 2^-6 max(1, max |ref|), flash form 2^-7; rows of <= 64
keys in range: flash == aten-order bit for bit.

Measured on the MI355X, max |err| against the restated reference (aten-order and flash form
alike to the digits shown, but nan_past: flash 0.00238) beside the aten-order bound; the flash
bound is half of it. On the marked heads of the 50 / 53 cases the error is 0.00035 everywhere: the
bf16 rounding of -2.2184.

    edges65    0.00391 / 0.0347     geom64x2   0.00351 / 0.0510     rows32     0.00503 / 0.0581 (flash only)
    edges128   0.00532 / 0.0347     geom128x2  0.00425 / 0.0540     spread256  0.00374 / 0.0347
    edges191   0.00342 / 0.0347     geom256x1  0.00035 / 0.0496     spread128  0.00756 / 0.0373
    window100  0.00313 / 0.0347     geom256x2  0.00346 / 0.0510     softcap 0  0.00701 / 0.0567
    cross      0.00437 / 0.0347     nan_past   0.00249 / 0.0347

The largest share of a bound taken: 0.41 (spread128, flash form).
"""
import pytest
import torch

from tests import kernel_cases as kc
from tests.engine_cases import need_gpu

pytestmark = pytest.mark.gpu


def _call(name, flash, softcap=kc.SOFTCAP):
    r = kc.softcap_case(name)
    c = r["c"]
    got, q, K, V = kc.decode_attention_call(c["L"], len(c["lens"]), c["lens"], Hq=c["Hq"], Hkv=c["Hkv"], D=c["D"],
                                            causal=c["causal"], seed=c["seed"], flash=flash, window=c["window"],
                                            cap=c["cap"], prepare=kc.softcap_prepare(c), softcap=softcap)
    # the launch ran on the inputs the CPU teeth were asserted on
    for a, b in ((q, r["q"]), (K, r["K"]), (V, r["V"])):
        assert torch.equal(kc.i16(a), kc.i16(b)), name
    return got


def _check(name):
    """Every form of the case against the restated reference at its bound, the errors printed
    beside the bounds; rows of one chunk bit for bit between the forms."""
    r = kc.softcap_case(name)
    c, ref = r["c"], r["ref"]["restated"]
    got = {flash: _call(name, flash) for flash in c["forms"]}
    err = {flash: (g - ref).abs() for flash, g in got.items()}
    mk = torch.tensor([[b, h] for b, h in r["marked"]])
    print(f"softcap {name}: " + ", ".join(
        f"{'flash' if f else 'aten-order'} max |err| {e.max().item():.3g} (marked heads {e[mk[:, 0], mk[:, 1]].max().item():.3g}) "
        f"bound {r['bound'][f]:.3g}" for f, e in err.items()) + f", max |ref| {ref.abs().max().item():.3g}")
    for flash, g in got.items():
        assert bool(torch.isfinite(g).all()), (name, flash)
    for flash, e in err.items():
        assert e.max().item() <= r["bound"][flash], (name, flash, e.max().item(), r["bound"][flash])
    if len(got) == 2:
        small = [b for b, L in enumerate(c["lens"]) if (min(L, c["window"]) if c["window"] > 0 else L) <= 64]
        assert small and torch.equal(got[True][small], got[False][small]), name
    return got


@pytest.mark.parametrize("L", [65, 128, 191])
def test_chunk_edges(L):
    """Rows of 2 and 64 keys (one chunk), 65 (a second chunk of one key: the last marker alone
    in it) and L keys (128: two full chunks, 191: a last chunk of 63)."""
    need_gpu()
    _check(f"edges{L}")


def test_unaligned_chunk_start():
    """A 100-key window: chunks that start at key t - 99, the first marker on that key."""
    need_gpu()
    _check("window100")


def test_cross_attention_shape():
    """causal = 0 over 60 / 64 / 9 / 2 text keys in 64 slots: the per-op launch (one workgroup
    per q head) that stage A of the persistent layer launch has to equal."""
    need_gpu()
    _check("cross")


def test_masked_keys_never_leak():
    """NaN in K and V in every slot past each row's length, 70 slots past the longest row: no
    NaN reaches an output (tanh and the roundings would pass one on)."""
    need_gpu()
    for g in _check("nan_past").values():
        assert not torch.isnan(g).any()


@pytest.mark.parametrize("D,G", [(64, 2), (128, 2), (256, 1), (256, 2)])
def test_all_instantiated_geometries(D, G):
    """Every (head_dim, group) attention_decode builds, 2 kv heads, rows of 70 / 64 / 9 / 1 keys:
    both fast_score call sites of attn.hip (the flash launch at (256, 2) reduces a key's two
    heads together; every other launch takes the general one)."""
    need_gpu()
    _check(f"geom{D}x{G}")


def test_rows32_flash():
    """32 rows of 1 .. 130 keys, flash form."""
    need_gpu()
    _check("rows32")


@pytest.mark.parametrize("name", ["spread256", "spread128"])
def test_every_rounding_point(name):
    """Marker scores of 26 .. 69 (22 .. 45 after the softcap), one pair per (row, kv head): a
    fast_score without any one of its roundings fails this bound (tests/test_kernel_cases_cpu.py)."""
    need_gpu()
    _check(name)


@pytest.mark.parametrize("flash", [False, True], ids=["aten_order", "flash"])
def test_softcap_zero_is_the_unset_field(flash):
    """softcap = 0 through the new field == a call that never touches the field, bit for bit, and
    both differ from the softcap-50 call on these inputs."""
    need_gpu()
    zero = _call("edges191", flash, softcap=0.0)
    unset = _call("edges191", flash, softcap=None)
    on = _call("edges191", flash)
    assert torch.equal(zero, unset)
    assert not torch.equal(zero, on)
    # softcap 0 on the marked inputs is the "nocap" reference, at the sdpa bound
    r = kc.softcap_case("edges191")
    ref = r["ref"]["nocap"]
    bound = (2.0 ** -7 if flash else 2.0 ** -6) * max(1.0, ref.abs().max().item())
    err = (zero - ref).abs().max().item()
    print(f"softcap 0 {'flash' if flash else 'aten-order'}: max |err| vs the uncapped reference {err:.3g}, bound {bound:.3g}")
    assert err <= bound
