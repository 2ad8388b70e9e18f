"""Weight tables for the engine: seeded synthetic weights and HF safetensors loading.

Key names are the reference's HF export layout (SURVEY 3.4;
``scripts/export_t5gemma_voice_hf.py:152-171``, ``hf_export/modeling_t5gemma_voice.py:497-506``):
``backbone.model.{encoder,decoder}.*``, ``audio_embedding.0.weight``,
``predict_layer.0.{0,2}.{weight,bias}`` with ``prune_text_modules=2`` (no decoder
``embed_tokens``, no ``lm_head``).

The seeded generator is deterministic on CPU (torch's CPU Philox/MT stream), so the
GPU box regenerates exactly the weights the golden fixtures were produced with.
"""
from __future__ import annotations

import hashlib
from typing import Dict, List, Tuple

import torch

from .config import VoiceConfig

ENC = "backbone.model.encoder"
DEC = "backbone.model.decoder"


def weight_shapes(cfg: VoiceConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """Ordered (name, shape) list of every tensor the generate() path reads."""
    bb = cfg.backbone
    d, f, q, kv = bb.hidden_size, bb.intermediate_size, bb.q_dim, bb.kv_dim
    V = cfg.n_audio_tokens
    out: List[Tuple[str, Tuple[int, ...]]] = [(f"{ENC}.embed_tokens.weight", (bb.text_vocab_size, d))]
    for side, n in ((ENC, bb.num_encoder_layers), (DEC, bb.num_decoder_layers)):
        for i in range(n):
            p = f"{side}.layers.{i}"
            out += [
                (f"{p}.self_attn.q_proj.weight", (q, d)),
                (f"{p}.self_attn.k_proj.weight", (kv, d)),
                (f"{p}.self_attn.v_proj.weight", (kv, d)),
                (f"{p}.self_attn.o_proj.weight", (d, q)),
            ]
            if side == DEC:
                out += [
                    (f"{p}.cross_attn.q_proj.weight", (q, d)),
                    (f"{p}.cross_attn.k_proj.weight", (kv, d)),
                    (f"{p}.cross_attn.v_proj.weight", (kv, d)),
                    (f"{p}.cross_attn.o_proj.weight", (d, q)),
                ]
            out += [
                (f"{p}.mlp.gate_proj.weight", (f, d)),
                (f"{p}.mlp.up_proj.weight", (f, d)),
                (f"{p}.mlp.down_proj.weight", (d, f)),
                (f"{p}.pre_self_attn_layernorm.weight", (d,)),
                (f"{p}.post_self_attn_layernorm.weight", (d,)),
            ]
            if side == DEC:
                out += [
                    (f"{p}.pre_cross_attn_layernorm.weight", (d,)),
                    (f"{p}.post_cross_attn_layernorm.weight", (d,)),
                ]
            out += [
                (f"{p}.pre_feedforward_layernorm.weight", (d,)),
                (f"{p}.post_feedforward_layernorm.weight", (d,)),
            ]
        out.append((f"{side}.norm.weight", (d,)))
    out += [
        ("audio_embedding.0.weight", (V, d)),
        ("predict_layer.0.0.weight", (d, d)),
        ("predict_layer.0.0.bias", (d,)),
        ("predict_layer.0.2.weight", (V, d)),
        ("predict_layer.0.2.bias", (V,)),
    ]
    return out


def _std_for(name: str) -> float:
    if name.endswith("layernorm.weight") or name.endswith("norm.weight"):
        return 0.05   # RMSNorm scales are (1 + w)
    return 0.02


def synthetic_weights(cfg: VoiceConfig, seed: int, device: str = "cpu",
                      dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """Seeded N(0, std) weights at the exact tensor shapes of ``cfg``.

    On CPU the stream is reproducible bit-for-bit across machines (same torch);
    on a GPU device the values are random but not comparable to the CPU stream
    (used for throughput runs only).
    """
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    sd: Dict[str, torch.Tensor] = {}
    for name, shape in weight_shapes(cfg):
        t = torch.empty(shape, dtype=torch.float32, device=device)
        t.normal_(0.0, _std_for(name), generator=g)
        sd[name] = t.to(dtype)
    return sd


def state_dict_digest(sd: Dict[str, torch.Tensor]) -> str:
    """sha256 over names + raw bytes (order-independent of dict insertion)."""
    h = hashlib.sha256()
    for k in sorted(sd):
        t = sd[k].detach().contiguous().cpu()
        h.update(k.encode())
        h.update(t.view(torch.uint8).numpy().tobytes() if t.dtype != torch.bfloat16
                 else t.view(torch.int16).numpy().tobytes())
    return h.hexdigest()


def load_hf_checkpoint(model_dir: str) -> Dict[str, torch.Tensor]:
    """Read every ``*.safetensors`` shard of an HF export (no pickle)."""
    import glob
    import os

    from safetensors.torch import load_file

    files = sorted(glob.glob(os.path.join(model_dir, "*.safetensors")))
    if not files:
        raise FileNotFoundError(f"no safetensors in {model_dir}")
    sd: Dict[str, torch.Tensor] = {}
    for fn in files:
        sd.update(load_file(fn))
    return sd


def check_state_dict(cfg: VoiceConfig, sd: Dict[str, torch.Tensor]) -> None:
    """Raise ValueError if a required tensor is missing or mis-shaped."""
    for name, shape in weight_shapes(cfg):
        if name not in sd:
            raise ValueError(f"missing weight {name}")
        if tuple(sd[name].shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(sd[name].shape)} != {shape}")


# ---- FP8 e4m3 weights for the fast decode step (opt-in; csrc/fp8.hip) ----
WEIGHT_FORMATS = ("bf16", "fp8")
FP8_MAX = 448.0      # largest finite e4m3fn magnitude
FP8_EMIN = -100      # smallest row exponent: 2^-100 * 2^-9 (the smallest code) is a normal bf16


def fp8_supported(cfg: VoiceConfig) -> bool:
    """Whether an engine of this config takes ``weight_format="fp8"``: the widths the decode
    step's register-X GEMV sites are built for (hidden 2304, intermediate 9216, q_dim 2048)."""
    bb = cfg.backbone
    return bb.hidden_size == 2304 and bb.intermediate_size == 9216 and bb.q_dim == 2048


def fp8_quantized_names(cfg: VoiceConfig) -> List[str]:
    """State-dict keys of the tensors FP8 mode quantises -- what a decode step streams: every
    DECODER layer's self q / k / v / o, cross q / o, gate / up / down projections, and the
    65 541-row head ``predict_layer.0.2``. Not the encoder, the cross k / v projections (once
    per call), ``predict_layer.0.0``, embeddings, norms or biases."""
    names = []
    for i in range(cfg.backbone.num_decoder_layers):
        p = f"{DEC}.layers.{i}"
        names += [f"{p}.self_attn.{n}_proj.weight" for n in "qkvo"]
        names += [f"{p}.cross_attn.q_proj.weight", f"{p}.cross_attn.o_proj.weight"]
        names += [f"{p}.mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
    return names + ["predict_layer.0.2.weight"]


def quantize_fp8_rows(W: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The quantiser rule of csrc/fp8.hip restated in torch, per output row of ``W`` [N][K]
    (taken as bf16): ``e`` = the smallest integer >= -100 with ``amax * 2^-e <= 448`` (0 for an
    all-zero row), ``q = RNE_e4m3fn(W * 2^-e)`` (the scaling is exact; the NaN codes 0x7F / 0xFF
    are never produced). Returns ``(codes uint8 [N][K], scale fp32 [N] = 2^e, Wq bf16 [N][K])``
    with ``Wq = 2^e * q`` exactly. A non-finite weight raises ValueError."""
    if W.dim() != 2:
        raise ValueError(f"quantize_fp8_rows takes an [N][K] matrix, got {tuple(W.shape)}")
    w = W.detach().to(torch.bfloat16).float().cpu()
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_fp8_rows: non-finite weight")
    amax = w.abs().amax(dim=1)
    fr, ex = torch.frexp(amax)                       # amax = fr * 2^ex, fr in [0.5, 1); 448 = 0.875 * 2^9
    e = torch.where(fr <= 0.875, ex - 9, ex - 8).clamp(min=FP8_EMIN)
    e = torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int32)
    q8 = torch.ldexp(w, (-e)[:, None]).to(torch.float8_e4m3fn)
    scale = torch.ldexp(torch.ones_like(amax), e)
    wq = torch.ldexp(q8.float(), e[:, None])
    assert bool((wq.bfloat16().float() == wq).all()), "2^e * q must be exactly bf16"
    return q8.view(torch.uint8), scale, wq.bfloat16()


def fp8_rounded_state_dict(cfg: VoiceConfig, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``sd`` with exactly the tensors FP8 mode quantises (``fp8_quantized_names``) replaced by
    their dequantised images W_q: an ordinary bf16 engine built from it computes, bit for bit,
    what a ``weight_format="fp8"`` engine built from ``sd`` computes on the fast path."""
    out = dict(sd)
    for name in fp8_quantized_names(cfg):
        t = sd[name]
        out[name] = quantize_fp8_rows(t)[2].to(device=t.device, dtype=t.dtype)
    return out
