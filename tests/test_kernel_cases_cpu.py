"""What the kernel-level GPU tests of the fast path's encoder / prefill kernels take for granted
before they launch anything, checked with no GPU (tests/kernel_cases.py): the teeth of the
window and block cases come from the fp64 reference alone, the slab values tell a slab order,
and the RoPE safe-set rule leaves the share of unsafe pairs it predicts."""
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
