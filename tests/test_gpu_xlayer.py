"""Parity mode's decode layer after the self attention as one persistent launch
(csrc/xlayer.hip: self o-proj, norm, cross-q, PM cross attention, cross-o, norm, gate/up
GeGLU, down in the reference's two K parts, norm, the next layer's q|k|v) against the same
step as parity mode's per-op launches (xmm.hip / norm.hip / xattn.hip): tokens and every
logit row bitwise equal, at the true 2b-2b widths (d 2304, FFN 9216, 8 x 256 q heads over 4
kv heads; 2 + 2 layers), for 1-8 rows, across repeated calls (the launch's counter sets
reset themselves), and after a hand-off timeout (the call reruns on the per-op launches).
Reference: hf_export/modeling_t5gemma_voice.py:256-323 (PMDecoderLayer), [tf]
modeling_t5gemma.py:81-97; the parity goldens (tests/test_gpu_parity_full.py) run the
persistent layer against the reference's own outputs."""
import pytest

from tests.engine_cases import assert_same_run, default_params, mid_engine, need_gpu, utterances

pytestmark = pytest.mark.gpu


def _run(eng, utts, p, seeds, fused):
    eng.set_fused(fused)
    before = eng.xlayer_launches()
    out = eng.generate(utts, p, seeds=seeds, parity=True, record_logits=True)
    return out, eng.xlayer_launches() - before


@pytest.mark.parametrize("B", [1, 3, 8])
def test_xlayer_bitwise_equal_to_per_op_exact_launches(B):
    need_gpu()
    cfg, eng = mid_engine(16)
    utts = utterances(cfg, B, 90 + B, max_text=64)
    p = default_params()
    seeds = list(range(700, 700 + B))
    on0, n_on0 = _run(eng, utts, p, seeds, True)
    off, n_off = _run(eng, utts, p, seeds, False)
    on1, n_on1 = _run(eng, utts, p, seeds, True)
    assert n_off == 0
    assert n_on0 >= cfg.backbone.num_decoder_layers and n_on1 >= cfg.backbone.num_decoder_layers   # the persistent layer ran
    assert_same_run(on0, off, B, "on/off")
    assert_same_run(on0, on1, B, "on/on")
    assert sum(len(g) for g in on0["gen"]) > B


def test_xlayer_not_used_past_its_shape():
    """More than 8 rows: parity mode keeps the per-op launches (no persistent layer)."""
    need_gpu()
    cfg, eng = mid_engine(16)
    utts = utterances(cfg, 9, 33)
    p = default_params()
    out, n = _run(eng, utts, p, list(range(9)), True)
    assert n == 0
    assert sum(len(g) for g in out["gen"]) > 9


def test_xlayer_handoff_timeout_reruns_on_per_op_launches():
    """The sticky timeout word set through the test hook: every in-launch wait of the
    persistent layer gives up at once (no hang), the call reports T5G_EHANDOFF and reruns on
    the per-op launches -- the tokens of a per-op run; the next call uses the launch again."""
    need_gpu()
    from t5gemma_tts_amd import _lib
    cfg, eng = mid_engine(8)
    utts = utterances(cfg, 4, 55)
    p = default_params()
    seeds = list(range(40, 44))
    ref, _ = _run(eng, utts, p, seeds, False)
    eng.set_fused(True)
    _lib.check(_lib.lib().t5g_engine_poison_handoff(eng.h, 77), "poison_handoff")
    with pytest.warns(UserWarning):
        out = eng.generate(utts, p, seeds=seeds, parity=True, record_logits=True)
    assert_same_run(out, ref, 4, "rerun")
    again, n = _run(eng, utts, p, seeds, True)
    assert n > 0
    assert_same_run(again, ref, 4, "again")
