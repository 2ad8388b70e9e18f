"""The FP8 MLP-half launch's interface, without a GPU: the C symbols are declared, bound and
exported and check their arguments; the launch's bytes model counts P8 weights; the CLI refuses
--fp8_mlp without --weight_format fp8 before anything is loaded."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO


def test_fp8_mlp_interface_declared_and_exported():
    from t5gemma_tts_amd import _lib
    src = open(os.path.join(REPO, "include", "t5gtts.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for name in ("t5g_engine_set_fp8_mlp", "t5g_engine_mlp_half_launches"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    # the argument checks need no device: a null engine
    assert L.t5g_engine_set_fp8_mlp(None, 1) < 0
    assert L.t5g_engine_set_fp8_mlp(None, 0) < 0
    n = C.c_int64()
    assert L.t5g_engine_mlp_half_launches(None, C.byref(n)) < 0


def test_fused_mlp_bytes_counts_p8_weights():
    """weight_format="fp8": gate/up and down are 1 byte per element plus 4 bytes per output row
    (2 f + d rows) instead of 2 bytes per element; nothing else of the model changes."""
    from t5gemma_tts_amd._lib import fused_mlp_bytes
    d, f = 2304, 9216
    for M in (1, 8, 17, 32):
        bf16 = fused_mlp_bytes(M)
        assert bf16 == fused_mlp_bytes(M, d, f) == fused_mlp_bytes(M, d, f, weight_format="bf16")
        # the bf16 value bench.py quotes, term by term
        assert bf16 == 2 * f * d * 2 + d * f * 2 + 4 * M * d * 4 + M * d * 2 + 2 * d * 2 + M * d * 2 + 8 * M * d * 4
        got = fused_mlp_bytes(M, d, f, weight_format="fp8")
        assert got == bf16 - (2 * f * d + d * f) + 4 * (2 * f + d)
    assert fused_mlp_bytes(32, weight_format="fp8") < 0.52 * fused_mlp_bytes(32)
    with pytest.raises(ValueError):
        fused_mlp_bytes(32, weight_format="fp4")


def test_cli_rejects_fp8_mlp_without_fp8_weights(monkeypatch, capsys):
    from t5gemma_tts_amd import cli

    def no_load(*a, **k):
        raise AssertionError("nothing may be loaded or run for a refused flag combination")
    monkeypatch.setattr(cli, "load_model", no_load)
    monkeypatch.setattr(cli, "load_codec", no_load)
    # run_inference itself, as the library entry point
    with pytest.raises(ValueError, match="fp8_mlp"):
        cli.run_inference(target_text="hi", synthetic="tiny", fp8_mlp=True)
    # the command line: an argparse error (exit status 2) that names the flag
    seen = {}
    monkeypatch.setattr(cli, "run_inference", lambda **kw: seen.update(kw))
    for argv in (["--fp8_mlp", "True"], ["--fp8_mlp", "True", "--weight_format", "bf16"]):
        with pytest.raises(SystemExit) as ex:
            cli.main(["--target_text", "hi", "--synthetic", "tiny"] + argv)
        assert ex.value.code == 2
        assert "--fp8_mlp" in capsys.readouterr().err
    assert not seen
    # accepted with the format, and off by default
    cli.main(["--target_text", "hi", "--synthetic", "tiny", "--weight_format", "fp8", "--fp8_mlp", "True"])
    assert seen["fp8_mlp"] is True and seen["weight_format"] == "fp8" and seen["fp8_block"] is False
    seen.clear()
    cli.main(["--target_text", "hi", "--synthetic", "tiny", "--weight_format", "fp8"])
    assert seen["fp8_mlp"] is False
