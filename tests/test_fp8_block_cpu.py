"""The FP8 whole-layer launch's interface, without a GPU: the C symbol is declared, bound and
exported and checks its arguments; the launch's bytes model counts P8 weights; the CLI refuses
--fp8_block without --weight_format fp8 before anything is loaded."""
import os
import re

import pytest

from conftest import REPO


def test_fp8_block_interface_declared_and_exported():
    from t5gemma_tts_amd import _lib
    src = open(os.path.join(REPO, "include", "t5gtts.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    name = "t5g_engine_set_fp8_block"
    assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert name in _lib.SIGNATURES, name
    assert hasattr(L, name), name
    # the argument check needs no device: a null engine
    assert L.t5g_engine_set_fp8_block(None, 1) < 0
    assert L.t5g_engine_set_fp8_block(None, 0) < 0


def test_fused_block_bytes_counts_p8_weights():
    """weight_format="fp8": every weight term of the model -- self o, cross q, cross o, gate/up,
    down, and on all layers but the last the next layer's q|k|v (the launch's seventh weight is
    the next layer's self o in place of its own: the model counts one self o per launch) -- is
    1 byte per element plus 4 bytes per output row instead of 2 bytes per element."""
    from t5gemma_tts_amd._lib import fused_block_bytes
    M, T_x, d, f, q_dim, kv_dim, n_layers = 8, 60, 2304, 9216, 2048, 1024, 26
    qkv_dim = q_dim + 2 * kv_dim
    bf16 = fused_block_bytes(M, T_x)
    assert bf16 == fused_block_bytes(M, T_x, weight_format="bf16")
    shapes = [(d, q_dim), (q_dim, d), (d, q_dim), (2 * f, d), (d, f)]   # (output rows, K)
    elems = sum(n * k for n, k in shapes)
    rows = sum(n for n, _ in shapes)
    share = (n_layers - 1) / n_layers   # the last layer projects no next q|k|v
    want = bf16 - (elems + share * qkv_dim * d) + 4 * (rows + share * qkv_dim)
    got = fused_block_bytes(M, T_x, weight_format="fp8")
    assert got == pytest.approx(want, rel=1e-12)
    assert got < 0.52 * bf16   # the launch's bytes are nearly all weights
    # with stage S the same weight terms change
    k = 4000.0
    assert fused_block_bytes(M, T_x, self_keys=k) - fused_block_bytes(M, T_x, self_keys=k, weight_format="fp8") \
        == pytest.approx(bf16 - got, rel=1e-12)
    with pytest.raises(ValueError):
        fused_block_bytes(M, T_x, weight_format="fp4")


def test_cli_rejects_fp8_block_without_fp8_weights(monkeypatch, capsys):
    from t5gemma_tts_amd import cli

    def no_load(*a, **k):
        raise AssertionError("nothing may be loaded or run for a refused flag combination")
    monkeypatch.setattr(cli, "load_model", no_load)
    monkeypatch.setattr(cli, "load_codec", no_load)
    # run_inference itself, as the library entry point
    with pytest.raises(ValueError, match="fp8_block"):
        cli.run_inference(target_text="hi", synthetic="tiny", fp8_block=True)
    # the command line: an argparse error (exit status 2) that names the flag
    seen = {}
    monkeypatch.setattr(cli, "run_inference", lambda **kw: seen.update(kw))
    for argv in (["--fp8_block", "True"], ["--fp8_block", "True", "--weight_format", "bf16"]):
        with pytest.raises(SystemExit) as ex:
            cli.main(["--target_text", "hi", "--synthetic", "tiny"] + argv)
        assert ex.value.code == 2
        assert "--fp8_block" in capsys.readouterr().err
    assert not seen
    # accepted with the format, and off by default
    cli.main(["--target_text", "hi", "--synthetic", "tiny", "--weight_format", "fp8", "--fp8_block", "True"])
    assert seen["fp8_block"] is True and seen["weight_format"] == "fp8"
    seen.clear()
    cli.main(["--target_text", "hi", "--synthetic", "tiny", "--weight_format", "fp8"])
    assert seen["fp8_block"] is False
