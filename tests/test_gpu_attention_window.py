"""The fast path's decode attention (csrc/attn.hip: attn_decode_kernel, attn_pvc_kernel, the
flash tail) through the C ABI where tests/test_gpu_attention.py does not go: a sliding window
(`lo = max(0, t - window + 1)`, stated three times in attn.hip), a cache capacity larger than
the rows, and every instantiated (head_dim, group) geometry -- against exact fp64 softmax
attention over the same bf16 inputs, at the bounds test_gpu_attention.py uses
(2^-6 max(1, max|exact|) for the aten-order form, 2^-7 for the flash form).

The query of a row of `len` keys sits at len - 1, so its window holds keys
[max(0, len - window), len).
"""
import pytest
import torch

from tests.engine_cases import need_gpu
from tests.kernel_cases import BF16
from tests.kernel_cases import decode_attention_call as _run
from tests.kernel_cases import decode_exact_attention as _exact

pytestmark = pytest.mark.gpu


def _bound(exact, flash):
    return (2.0 ** -7 if flash else 2.0 ** -6) * max(1.0, exact.abs().max().item())


def _plant_markers(lens, window, flip, G):
    """prepare() for _run: per row longer than the window, one marker key -- 8 q / |q| for head 0
    of every GQA group (score 8 |q| scale = 8 at |q| ~ sqrt(D): about e^8 times an ordinary
    key's weight), its V row +4 everywhere. Rows of parity `flip` carry it just outside the
    window (key len - window - 1: it must not count), the others on the first key inside
    (key len - window: it must count). Returns the rows that carry a marker."""
    marked = {}

    def prepare(q, K, V):
        for b, L in enumerate(lens):
            if L <= window:
                continue
            key = L - window - 1 if b % 2 == flip else L - window
            marked[b] = key
            for h in range(K.shape[1]):
                qh = q[b, h * G].float()
                K[b, h, key] = (8.0 * qh / qh.norm()).to(BF16)
                V[b, h, key] = 4.0
    return prepare, marked


@pytest.mark.parametrize("flash", [False, True], ids=["aten_order", "flash"])
def test_window_boundary_is_exact(flash):
    """8 rows x 8 q heads / 4 kv heads x 256; window 100 with row lengths around 100 and
    100 + 64 (the chunk edge of the windowed span), window 64 with lengths 64 / 65 / 128 / 129.
    An off-by-one in `lo` takes a marker key in or out, which moves the output by ~4."""
    need_gpu()
    scale = 256 ** -0.5
    for window, lens in ((100, [1, 64, 99, 100, 101, 164, 165, 400]), (64, [64, 65, 128, 129, 129, 128, 65, 64])):
        for flip in (0, 1):
            prepare, marked = _plant_markers(lens, window, flip, 2)
            got, q, K, V = _run(max(lens), len(lens), lens, seed=1000 + window + flip, flash=flash, window=window,
                                prepare=prepare)
            exact = _exact(q, K, V, lens, scale, window)
            bound = _bound(exact, flash)
            err = (got - exact).abs().amax(dim=(1, 2))
            # teeth, from the reference alone: the window one key longer / shorter moves every
            # marked row's output by at least ten times the bound
            wider = (_exact(q, K, V, lens, scale, window + 1) - exact).abs().amax(dim=(1, 2))
            narrower = (_exact(q, K, V, lens, scale, window - 1) - exact).abs().amax(dim=(1, 2))
            print(f"flash={flash} window={window} flip={flip}: bound {bound:.3g}, per-row max |err| "
                  f"{[round(e, 4) for e in err.tolist()]}, marker moves the reference by "
                  f"{[round(max(wider[b].item(), narrower[b].item()), 2) for b in sorted(marked)]}")
            assert sorted(marked) == [b for b, L in enumerate(lens) if L > window] and len(marked) >= 4
            for b, key in marked.items():
                moved = wider[b] if key == lens[b] - window - 1 else narrower[b]
                assert moved.item() >= 10 * bound, (window, flip, b, moved.item())
            assert err.max().item() <= bound, (window, flip, err.tolist())


@pytest.mark.parametrize("flash", [False, True], ids=["aten_order", "flash"])
def test_cap_larger_than_rows(flash):
    """The cache holds more slots than any row uses (cap 1024 over rows of <= 200 keys; cap 129,
    no multiple of the 64-key chunk, over rows of <= 129): the unused slots hold K = 1e4 and
    V = NaN, so a stride or bound slip shows as a huge or NaN output. window 0 and 100."""
    need_gpu()
    scale = 256 ** -0.5
    for cap, lens in ((1024, [200, 1, 64, 65, 129, 199, 100, 137]), (129, [129, 128, 65, 64, 1, 100, 129, 77])):
        def prepare(q, K, V, lens=lens):
            for b, L in enumerate(lens):
                K[b, :, L:] = 1e4
                V[b, :, L:] = float("nan")
        for window in (0, 100):
            got, q, K, V = _run(max(lens), len(lens), lens, seed=cap + window, flash=flash, window=window, cap=cap,
                                prepare=prepare)
            exact = _exact(q, K, V, lens, scale, window)
            err = (got - exact).abs()
            print(f"flash={flash} cap={cap} window={window}: max |err| {err.max().item():.3g}")
            assert not torch.isnan(got).any(), (cap, window)
            assert err.max().item() <= _bound(exact, flash), (cap, window)


@pytest.mark.parametrize("D,G", [(256, 2), (64, 2), (128, 2), (256, 1)])
def test_all_instantiated_geometries(D, G):
    """Every (head_dim, group) attention_decode instantiates, with 2 and 4 kv heads, 4 ragged
    rows up to 200 keys, both forms, window 0 and 50."""
    need_gpu()
    lens = [200, 1, 65, 137]
    for Hkv in (2, 4):
        for flash in (False, True):
            for window in (0, 50):
                got, q, K, V = _run(200, 4, lens, Hq=G * Hkv, Hkv=Hkv, D=D, seed=D + G + Hkv, flash=flash,
                                    window=window)
                exact = _exact(q, K, V, lens, D ** -0.5, window)
                err = (got - exact).abs().max().item()
                print(f"D={D} G={G} Hkv={Hkv} flash={flash} window={window}: max |err| {err:.3g}")
                assert err <= _bound(exact, flash), (Hkv, flash, window)


@pytest.mark.parametrize("flash", [False, True], ids=["aten_order", "flash"])
def test_uninstantiated_geometry_is_unsupported(flash):
    """(head_dim, group) = (64, 4) is not built: T5G_EUNSUPPORTED, and nothing is launched."""
    need_gpu()
    from t5gemma_tts_amd import _lib
    assert _run(200, 4, [200, 1, 65, 137], Hq=8, Hkv=2, D=64, flash=flash, want_rc=_lib.T5G_EUNSUPPORTED) is None
