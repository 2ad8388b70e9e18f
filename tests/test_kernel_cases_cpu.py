"""What the kernel-level GPU tests of the fast path's encoder / prefill kernels take for granted
before they launch anything, checked with no GPU (tests/kernel_cases.py): the teeth of the
window and block cases come from the fp64 reference alone, the slab values tell a slab order,
the RoPE safe-set rule leaves the share of unsafe pairs it predicts, and the softcap cases of the
decode attention (tests/test_gpu_attn_softcap.py) have safe markers and references that move
when the softcap is dropped, misplaced or loses a rounding point."""
import pytest
import torch

from oracle.t5g_oracle import inv_freq_table
from tests import kernel_cases as kc


@pytest.mark.parametrize("causal,W", kc.WINDOW_CASES)
def test_window_markers_move_the_reference(causal, W):
    """Every marker sits on the side of its edge that its case says, and the reference with the
    window one key longer / shorter moves every marked query by at least ten times the bound
    (window_case asserts both for the seeds the GPU test uses)."""
    *_, exact, bound, move = kc.window_case(causal, W)
    assert bound == 2.0 ** -6 * max(1.0, exact.abs().max().item())
    assert move >= 10 * bound


def test_planted_keys_raise_the_running_max():
    s700, s1060 = kc.planted_scores()
    assert 6.5 <= s700 <= 9.5 and s700 + 0.5 <= s1060 <= 11, (s700, s1060)


@pytest.mark.parametrize("window", kc.BLOCK_WINDOWS)
def test_lost_block_rescale_moves_the_reference(window):
    """lo is no multiple of 512, the row spans two blocks counted from lo with a planted key in
    each, and a lost rescale moves the reference by ten times the bound. Window 560 also puts
    the block edge where an index counted from key 0 names another block."""
    _, _, bound, shift = kc.blocks_window_case(window)
    assert shift >= 10 * bound
    lo = kc.BLOCK_LEN - window
    if window == 560:
        assert (lo + 512) // 512 != 1
    else:
        assert (lo + 512) // 512 == 1


@pytest.mark.parametrize("name", sorted(kc.SOFTCAP_CASES))
def test_softcap_cases_have_teeth(name):
    """tests/test_gpu_attn_softcap.py's cases, from the references alone (softcap_case asserts
    them for the seed the GPU test uses): every marker's score lies more than 2^-10 of a bf16
    step from a tie at each of fast_score's five rounding points; the 50 / 53 cases move every
    marked head by ten times the aten-order bound when the softcap is dropped or applied after
    the scale, and by 1.5 bounds when the last rounding is; the spread cases move some marked
    head by 4 bounds for each rounding point their head_dim can tell."""
    r = kc.softcap_case(name)
    c, ref = r["c"], r["ref"]["restated"]
    print(f"{name}: seed {c['seed']}, {len(r['marked'])} marked heads, smallest marker margin {r['margin']:.3g} "
          f"of a step, bound {r['bound'][False]:.3g}, moves {r['move']}")
    assert r["bound"][False] == 2.0 ** -6 * max(1.0, ref.abs().max().item()) == 2 * r["bound"][True]
    assert r["margin"] > 2.0 ** -10
    rows = {b for b, _ in r["marked"]}
    assert rows == {b for b in range(len(c["lens"])) if min(c["lens"][b], c["window"] or c["lens"][b]) >= 2}
    if c["marks"] is None:
        assert r["move"]["nocap"] >= 10 * r["bound"][False] and r["move"]["late_scale"] >= 10 * r["bound"][False]
        assert r["move"]["drop4"] >= 1.5 * r["bound"][False]
        # the restatement, not the fp64 formula, is the reference: every marked head differs by
        # more than the flash bound
        assert r["move"]["exact"] > r["bound"][True]
    else:
        assert all(r["move"]["drop%d" % i] >= 1 for i in kc.SPREAD_DROPS[name])


def test_fast_score_ref_rounding_points():
    """The restatement on hand-computed values: 800 x 1/16 -> 50 -> 1 -> tanh 0.76159 -> 0.76171875
    -> 38.0859 -> 38; 848 -> 53 -> 1.06 -> 1.0625 -> 0.78661 -> 0.78515625 -> 39.2578 -> 39.25;
    softcap 0 is the plain fp32 product; at a power-of-two scale roundings 0 and 1 are one."""
    s = torch.tensor([800.0, 848.0, 801.3, 16.7])
    got = kc.fast_score_ref(s, 1 / 16, 50.0)
    assert got[:3].tolist() == [38.0, 39.25, 38.0]
    assert kc.fast_score_ref(s, 1 / 16, 0.0).tolist() == (s * (1 / 16)).tolist()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4096, generator=g) * 400
    full = kc.fast_score_ref(x, 1 / 16, 50.0)
    assert torch.equal(full, kc.fast_score_ref(x, 1 / 16, 50.0, drop=0))
    assert torch.equal(full, kc.fast_score_ref(x, 1 / 16, 50.0, drop=1))
    for i in (2, 3, 4):
        assert not torch.equal(full, kc.fast_score_ref(x, 1 / 16, 50.0, drop=i)), i
    # every result is a bf16 value, odd, and below the cap
    assert torch.equal(full, full.to(kc.BF16).float()) and torch.equal(full, -kc.fast_score_ref(-x, 1 / 16, 50.0))
    assert full.abs().max().item() <= 50.0
    # a value on a bf16 value is 0.5 from a tie, one on a tie 0
    assert kc.bf16_tie_margin(torch.tensor([1.0, 1.00390625, 800.0, 802.0], dtype=torch.float64)).tolist() == [0.5, 0.0, 0.5, 0.0]


@pytest.mark.parametrize("nsplit", [3, 5, 8])
def test_slab_values_tell_the_order(nsplit):
    p = kc.order_slabs(torch.Generator().manual_seed(nsplit), nsplit, 5, 2328, amp=3.0)
    assert kc.order_sensitivity(p) >= 0.25


@pytest.mark.parametrize("D", [256, 64])
def test_unsafe_pair_share_is_as_expected(D):
    """Positions up to 12 000 as the GPU tests draw them: the unsafe share is near
    2 * 8 / 65 536 per (cos, sin) pair, nowhere near the 1 % the GPU tests allow."""
    g = torch.Generator().manual_seed(D)
    pos = (torch.rand(4000, generator=g) * 12000.0).float()
    share = 1.0 - kc.trig_safe(inv_freq_table(D, 10000.0), pos).float().mean().item()
    print(f"D={D}: unsafe share over 4000 positions {share:.2e} (expected about {16 / 65536:.2e})")
    assert 0.25 * 16 / 65536 <= share <= 4 * 16 / 65536
