"""CPU-side checks of libt5gtts.so: it loads, exports every symbol include/t5gtts.h
declares, and its host-only parity sampler (std::sort tie order) reproduces the
reference's sampler golden cases. No GPU compute is invoked."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN
from tests.engine_cases import header_symbols


def test_library_exports_header_symbols():
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    syms = header_symbols("t5gtts.h", "t5g")
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(_lib.SIGNATURES), set(syms) ^ set(_lib.SIGNATURES)


def test_struct_layouts_match_header():
    from t5gemma_tts_amd import _lib
    assert C.sizeof(_lib.SamplerRow) == 48
    assert C.sizeof(_lib.SamplerState) == 48
    assert C.sizeof(_lib.LayerWeights) == 13 * 8
    assert C.sizeof(_lib.AttnDecodeArgs) == 4 * 4 + 3 * 8 + 8 + 8 + 4 * 4 + 2 * 8 + 8
    # softcap is appended: every earlier field keeps its offset
    assert _lib.AttnDecodeArgs.softcap.offset == 88 and _lib.AttnDecodeArgs.work.offset == 80
    assert _lib.AttnDecodeArgs().softcap == 0.0
    assert C.sizeof(_lib.GemvArgs) == 152
    # the three kernel-test hooks (csrc/engine_hooks.hip static_asserts the same sizes)
    assert C.sizeof(_lib.AttnPackedArgs) == 4 * 4 + 6 * 8 + 6 * 4 + 8
    assert C.sizeof(_lib.RopeStoreArgs) == 2 * 8 + 10 * 4 + 6 * 8 + 2 * 4 + 2 * 8 + 2 * 8 + 8
    assert C.sizeof(_lib.NormSrcArgs) == 2 * 4 + 3 * 8 + 2 * 4 + 8 + 2 * 4 + 3 * 8 + 2 * 4 + 6 * 8
    assert _lib.AttnPackedArgs.out.offset == 88 and _lib.AttnPackedArgs.cap.offset == 64
    assert _lib.RopeStoreArgs.pos.offset == 56 and _lib.RopeStoreArgs.c_bstride.offset == 128
    assert _lib.NormSrcArgs.part.offset == 40 and _lib.NormSrcArgs.resid_out.offset == 88


def _csrc_include_closure(src):
    """`src` and every csrc file its #include "..." lines reach, transitively."""
    import re
    from t5gemma_tts_amd import build
    seen, todo = set(), [src]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        with open(os.path.join(build.CSRC, name)) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                if os.path.exists(os.path.join(build.CSRC, inc)):
                    todo.append(inc)
    return seen


def test_fused_sources_are_tracked_by_build_and_digest():
    """The persistent decode launches are built from stage headers: every csrc file the three
    fused units include must be a rebuild dependency (build.py HEADERS / SOURCES), and every
    file behind the one-tile kernels must be hashed by the PMC source digests."""
    from t5gemma_tts_amd import _lib, build
    units = ["fused.hip", "fused_rows32.hip", "fused_p8.hip"]
    reach = {u: _csrc_include_closure(u) for u in units}
    assert all(len(reach[u]) > 5 for u in units), reach   # the closure walk found the headers
    tracked = set(build.HEADERS) | set(build.SOURCES)
    for u in units:
        assert reach[u] <= tracked, (u, sorted(reach[u] - tracked))
        assert not [f for f in reach[u] - {u} if f.endswith(".hip")], (u, "includes another source")
    one_tile = reach["fused.hip"] | reach["fused_p8.hip"]
    for op in ("fused_block", "fused_block_s"):
        assert one_tile <= set(_lib.PMC_SOURCES[op]), (op, sorted(one_tile - set(_lib.PMC_SOURCES[op])))
    attention = {"fused_attn.h", "attn_chunk.h"}
    assert attention <= one_tile
    assert one_tile - attention <= set(_lib.PMC_SOURCES["fused_mlp"]), \
        sorted(one_tile - attention - set(_lib.PMC_SOURCES["fused_mlp"]))
    for op in ("fused_block", "fused_block_s", "fused_mlp", "fast_path"):
        assert len(_lib.kernel_source_digest(op)) == 16   # every listed file exists


def test_packed_bytes():
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    assert L.t5g_packed_bytes(4096, 2304) == 4096 * 2304 * 2
    assert L.t5g_packed_bytes(65541, 2304) == 4100 * 16 * 2304 * 2  # row groups padded to x4
    assert L.t5g_packed_bytes(16, 33) < 0


def test_host_sampler_matches_reference_golden():
    """t5g_host_sample (exact std::sort tie order) on every reference sampler case."""
    from tests.golden.make_golden import make_sampler_logits
    from t5gemma_tts_amd import _lib
    from t5gemma_tts_amd.engine import reference_noise
    L = _lib.lib()
    meta = json.load(open(os.path.join(GOLDEN, "golden_sampler.json")))
    for c in meta["cases"]:
        V = c["V"]
        logits = make_sampler_logits(c["logit_seed"], V, c["scale"], c["quant"]).contiguous()
        noise = reference_noise(c["noise_seed"], 1, V)[0].contiguous()
        row = _lib.SamplerRow(top_k=c["top_k"], top_p=c["top_p"], min_p=c["min_p"],
                              temperature=c["temperature"])
        st = _lib.SamplerState(cur_num_gen=100, current_length=200, prompt_offset=1, target_total=-1,
                               est_total=1000, prev_token=-1, first_input_len=5)
        out = _lib.SamplerState()
        tok = C.c_int32()
        tk = (C.c_int32 * 1)()
        rc = L.t5g_host_sample(C.c_void_p(logits.data_ptr()), V, C.byref(row), tk, tk, C.byref(st),
                               C.c_void_p(noise.data_ptr()), 65539, 10, 250.0, 0, 2000.0, 4096, 4096,
                               C.byref(out), C.byref(tok))
        assert rc == 0
        assert tok.value == c["token"], c
        assert out.cur_num_gen == 101 and out.prev_token == c["token"]


@pytest.mark.parametrize("layout,M,K,splits,epi,nw", [
    (1, 33, 2304, 1, 3, 12),    # register-X: at most 32 rows
    (1, 8, 2304, 2, 3, 12),     # split K only into fp32 slabs
    (1, 8, 2048, 1, 4, 8),      # unsplit slices must be 72 k-steps
    (1, 8, 9216, 8, 4, 8),      # 36-k-step slices: nw must divide 36
    (1, 8, 9216, 3, 4, 12),     # 96-k-step slices: not instantiated
    (1, 8, 2304, 5, 4, 4),      # 72 k-steps do not split in 5
    (0, 17, 2304, 1, 3, 8),     # LDS-staged X: at most 16 rows
    (2, 8, 2304, 1, 3, 8),      # no third layout
    (1, 8, 2304, 1, 3, 16),     # register-X wave counts: 4 / 6 / 8 / 9 / 12 only
    (1, 8, 2304, 1, 3, 5),
])
def test_gemv_rejects_unsupported_shapes(layout, M, K, splits, epi, nw):
    """t5g_gemv validates on the host and returns an error code before any launch for the
    shapes its kernels are not built for (csrc/gemv.hip gemv_rx / gemv_dec)."""
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    a = _lib.GemvArgs()
    a.M, a.K, a.N, a.epi, a.pro, a.nw, a.un = M, K, 2304, epi, 0, nw, 8
    a.X, a.ldx, a.Y, a.ldy, a.splits, a.layout, a.max_grid = 16, K, 16, 2304, splits, layout, 0
    a.W = 16   # never dereferenced: every case is rejected before a launch
    assert L.t5g_gemv(C.byref(a), None) < 0


@pytest.mark.parametrize("D,G", [(64, 4), (128, 1), (96, 2), (256, 4)])
def test_attention_decode_reports_unbuilt_geometry(D, G):
    """t5g_attention_decode / _flash answer T5G_EUNSUPPORTED on the host, before any launch, for
    a (head_dim, group) csrc/attn.hip builds no kernel for -- in the flash form too, whose
    thread-budget check would otherwise call it a bad argument."""
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    # pointers are never dereferenced: the call is rejected before a launch
    a = _lib.AttnDecodeArgs(B=4, n_heads=2 * G, n_kv_heads=2, head_dim=D, q=16, k_cache=16, v_cache=16, cap=200,
                            kv_len=16, causal=1, window=0, scale=D ** -0.5, out=16, work=16)
    assert L.t5g_attention_decode(C.byref(a), None) == _lib.T5G_EUNSUPPORTED
    assert L.t5g_attention_decode_flash(C.byref(a), None) == _lib.T5G_EUNSUPPORTED
    # a softcap that is negative or not finite is a bad argument whatever the geometry; 50 is not
    for bad in (-1.0, -50.0, float("nan"), float("inf"), float("-inf")):
        a.softcap = bad
        assert L.t5g_attention_decode(C.byref(a), None) == _lib.T5G_EINVAL, bad
        assert L.t5g_attention_decode_flash(C.byref(a), None) == _lib.T5G_EINVAL, bad
    a.softcap = 50.0
    assert L.t5g_attention_decode(C.byref(a), None) == _lib.T5G_EUNSUPPORTED
    assert L.t5g_attention_decode_flash(C.byref(a), None) == _lib.T5G_EUNSUPPORTED


@pytest.mark.parametrize("flash", [False, True], ids=["aten_order", "flash"])
def test_attention_decode_rejects_bad_softcap(flash):
    """A built geometry (8 q / 4 kv heads x 256) with a negative or non-finite softcap:
    T5G_EINVAL on the host, before any launch (the pointers are never dereferenced)."""
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    fn = L.t5g_attention_decode_flash if flash else L.t5g_attention_decode
    for bad in (-1.0, -1e-30, float("nan"), float("inf")):
        a = _lib.AttnDecodeArgs(B=4, n_heads=8, n_kv_heads=4, head_dim=256, q=16, k_cache=16, v_cache=16, cap=200,
                                kv_len=16, causal=1, window=0, scale=1 / 16, out=16, work=16, softcap=bad)
        assert fn(C.byref(a), None) == _lib.T5G_EINVAL, bad


def _packed_args(**kw):
    """A t5g_attention_packed call that would be valid (pointers are never dereferenced: every
    case below is rejected before a launch), with fields overridden."""
    from t5gemma_tts_amd import _lib
    f = dict(Mq=4, n_heads=8, n_kv_heads=4, head_dim=256, q=16, q_row=16, q_pos=16, k_cache=16, v_cache=16,
             kv_len=16, cap=256, causal=1, window=0, scale=1 / 16, softcap=0.0, out=16)
    f.update(kw)
    return _lib.AttnPackedArgs(**f)


def _rope_args(**kw):
    from t5gemma_tts_amd import _lib
    f = dict(X=16, Xpart=None, nsplit=0, ldx=4096, M=5, D=256, nq=8, nk=4, nv=4, col0=0, rope_q=1, rope_k=1,
             pos=16, inv_freq=16, tok_row=16, tok_t=16, kv_len=16, Qout=32, ldq=2048, Kc=16, Vc=16,
             c_bstride=4 * 64 * 256, c_hstride=64 * 256, rope_tab=None)
    f.update(kw)
    return _lib.RopeStoreArgs(**f)


def _norm_args(**kw):
    from t5gemma_tts_amd import _lib
    f = dict(M=3, d=2304, delta=16, resid=16, post_w=16, pre_w=16, eps=1e-6, resid_out=16, normed_out=16)
    f.update(kw)
    return _lib.NormSrcArgs(**f)


@pytest.mark.parametrize("kw", [dict(q=None), dict(k_cache=None), dict(v_cache=None), dict(kv_len=None),
                                dict(out=None), dict(reserved=1), dict(Mq=0), dict(cap=0), dict(cap=-3),
                                dict(n_kv_heads=0), dict(n_heads=7), dict(head_dim=0), dict(window=-1),
                                # scores of one query: G * cap * 4 bytes <= 96 KiB
                                dict(cap=12289), dict(n_heads=4, cap=12289)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_attention_packed_rejects_bad_arguments(kw):
    from t5gemma_tts_amd import _lib
    assert _lib.lib().t5g_attention_packed(C.byref(_packed_args(**kw)), None) == _lib.T5G_EINVAL


def test_attention_packed_null_struct_and_unbuilt_geometry():
    """(head_dim, group) = (64, 4) has no attn_kernel: T5G_EUNSUPPORTED, also where its scores
    would not fit; 12 288 keys at G = 2 (exactly 96 KiB) pass the size check and are refused
    only for their geometry here."""
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    assert L.t5g_attention_packed(None, None) == _lib.T5G_EINVAL
    for D, G in ((64, 4), (128, 1), (96, 2), (256, 4)):
        for cap in (200, 12289):
            a = _packed_args(n_heads=2 * G, n_kv_heads=2, head_dim=D, cap=cap)
            assert L.t5g_attention_packed(C.byref(a), None) == _lib.T5G_EUNSUPPORTED, (D, G, cap)


@pytest.mark.parametrize("kw", [dict(X=None), dict(Xpart=16, nsplit=2), dict(reserved=1), dict(M=0), dict(D=0), dict(D=255),
                                dict(nq=0, nk=0, nv=0), dict(nq=-1), dict(col0=-8), dict(ldx=4095),
                                dict(col0=8), dict(Qout=None), dict(ldq=2040), dict(Kc=None), dict(Vc=None),
                                dict(tok_t=None, kv_len=None), dict(c_hstride=255), dict(pos=None),
                                dict(inv_freq=None),
                                # split-K slabs: 1 to 8
                                dict(X=None, Xpart=16, nsplit=9), dict(X=None, Xpart=16, nsplit=0),
                                # q in place needs one row stride
                                dict(Qout=16, ldq=2048)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_rope_store_rejects_bad_arguments(kw):
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    assert L.t5g_rope_store(C.byref(_rope_args(**kw)), None) == _lib.T5G_EINVAL
    assert L.t5g_rope_store(None, None) == _lib.T5G_EINVAL


@pytest.mark.parametrize("kw", [dict(M=0), dict(d=0), dict(d=2300), dict(d=8200), dict(d=8196), dict(delta=None),
                                dict(ids=16), dict(delta=None, ids=16), dict(delta=None, ids=16, table=16),
                                dict(delta=None, part=16, nsplit=9, ldp=2304),
                                dict(delta=None, part=16, nsplit=0, ldp=2304),
                                dict(delta=None, part=16, nsplit=2, ldp=2296),
                                dict(delta=None, part=16, nsplit=2, ldp=2306),
                                dict(resid_out=None, normed_out=None), dict(normed_out=None),
                                dict(rope_tab=16), dict(rope_tab=16, rope_pos=16, rope_inv_freq=16, rope_D=255),
                                dict(delta=None, ids=16, table=16, n_table=300, out_rows=16, resid=None)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_resid_norm_src_rejects_bad_arguments(kw):
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    assert L.t5g_resid_norm_src(C.byref(_norm_args(**kw)), None) == _lib.T5G_EINVAL
    assert L.t5g_resid_norm_src(None, None) == _lib.T5G_EINVAL


def test_resid_norm_src_out_rows_with_slabs_is_unsupported():
    """The slabs' row stride is the launch's row count, so a row subset of them has no meaning."""
    from t5gemma_tts_amd import _lib
    a = _norm_args(delta=None, part=16, nsplit=2, ldp=2304, out_rows=16)
    assert _lib.lib().t5g_resid_norm_src(C.byref(a), None) == _lib.T5G_EUNSUPPORTED


def _op(name, table):
    from t5gemma_tts_amd import _lib
    fn = getattr(_lib.lib(), name)
    fn.restype, fn.argtypes = table[name]
    return fn


def _refused(fn, good, kw):
    """The call with `kw` over the valid arguments `good` (pointers are never dereferenced: the
    valid call itself is never made) returns -1."""
    a = dict(good)
    a.update(kw)
    return fn(*a.values()) == -1


_IDS = dict(ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))


@pytest.mark.parametrize("kw", [dict(qkv=None), dict(qe=None), dict(out=None), dict(T=0), dict(T=-5), dict(heads=0),
                                dict(heads=-2), dict(L=-1), dict(R=-1)], **_IDS)
def test_xc2e_attention_relkey_rejects_bad_arguments(kw):
    from t5gemma_tts_amd.codec_enc import XC2E_SIGNATURES
    good = dict(qkv=16, T=42, heads=2, qe=16, L=64, R=8, out=16, stream=None)
    assert _refused(_op("xc2e_attention_relkey", XC2E_SIGNATURES), good, kw)


@pytest.mark.parametrize("kw", [dict(x=None), dict(alpha=None), dict(beta=None), dict(up=None), dict(down=None),
                                dict(y=None), dict(T=0), dict(C=0), dict(C=-1), dict(form=2), dict(form=-1),
                                dict(T=1 << 20, C=1 << 12)], **_IDS)
def test_xc2e_snake_rejects_bad_arguments(kw):
    from t5gemma_tts_amd.codec_enc import XC2E_SIGNATURES
    good = dict(x=16, T=12, C=5, alpha=16, beta=16, up=16, down=16, y=16, form=0, stream=None)
    assert _refused(_op("xc2e_snake", XC2E_SIGNATURES), good, kw)


@pytest.mark.parametrize("kw", [dict(p1=None), dict(dw=None), dict(ln_w=None), dict(ln_b=None), dict(out=None),
                                dict(T=0), dict(H=0), dict(H=126), dict(H=1028), dict(H=2048), dict(KW=0),
                                dict(KW=-31)], **_IDS)
def test_xc2e_conv_module_mid_rejects_bad_arguments(kw):
    from t5gemma_tts_amd.codec_enc import XC2E_SIGNATURES
    good = dict(p1=16, T=42, H=128, KW=31, dw=16, ln_w=16, ln_b=16, eps=1e-5, out=16, stream=None)
    assert _refused(_op("xc2e_conv_module_mid", XC2E_SIGNATURES), good, kw)


@pytest.mark.parametrize("kw", [dict(m=None), dict(Q=None), dict(K=None), dict(V=None), dict(O=None), dict(Tq=0),
                                dict(Tk=0), dict(q_off=-1), dict(causal=2), dict(ldkv=0), dict(ldkv=130),
                                # a key / value width that is not 64 x heads or more
                                dict(ldkv=64), dict(ldkv=124),
                                # causal: the last query's range ends inside the keys
                                dict(q_off=7), dict(Tq=11, q_off=0),
                                # one query: all keys count, and the split workspace holds 1500
                                dict(Tq=1, Tk=10, q_off=3), dict(Tq=1, Tk=1501, causal=0, q_off=0)], **_IDS)
def test_whs_attention_op_rejects_bad_arguments(kw):
    """The checks read only the model's leading whs_config (head count, the two context lengths),
    so a host buffer that starts with one stands in for a model: creating a real one needs the
    GPU, and every case here is refused before a launch."""
    from t5gemma_tts_amd import whisper_asr as w
    cfg = w.WHSConfig(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=2, n_vocab=51866,
                      n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=2, max_samples=16000)
    standin = C.create_string_buffer(bytes(cfg), C.sizeof(cfg) + C.sizeof(w.WHSWeights) + 1024)
    good = dict(m=C.addressof(standin), Q=16, K=16, V=16, ldkv=128, Tq=4, Tk=10, causal=1, q_off=6, O=16, stream=None)
    assert _refused(_op("whs_attention_op", w.WHS_SIGNATURES), good, kw)


@pytest.mark.parametrize("kw", [dict(X=None), dict(W=None), dict(Y=None), dict(M=0), dict(N=0), dict(K=0), dict(K=-4),
                                dict(epi=1), dict(epi=5), dict(epi=-1),
                                # the tiled GEMM's K step is 32: M > 4 or K % 4 != 0 lands there
                                dict(M=5, K=2052), dict(K=130), dict(M=5, K=130)], **_IDS)
def test_whs_linear_op_rejects_bad_arguments(kw):
    from t5gemma_tts_amd import whisper_asr as w
    good = dict(X=16, M=2, W=16, N=128, K=128, bias=None, resid=None, epi=0, Y=16, stream=None)
    assert _refused(_op("whs_linear_op", w.WHS_SIGNATURES), good, kw)


def test_status_codes_map_to_python_errors():
    """The C ABI's statuses raise what the reference's code paths would (ValueError for bad
    arguments / capacity) and a FusedHandoffError for a fused decode launch whose hand-off
    gave up (engine.generate reruns such a call on the per-op launches)."""
    import pytest as _pt
    from t5gemma_tts_amd import _lib
    _lib.check(0, "ok")
    with _pt.raises(ValueError):
        _lib.check(-1, "x")
    with _pt.raises(ValueError):
        _lib.check(-5, "x")
    with _pt.raises(_lib.FusedHandoffError):
        _lib.check(-6, "x")
    with _pt.raises(_lib.T5GError):
        _lib.check(-2, "x")
    assert issubclass(_lib.FusedHandoffError, _lib.T5GError)
