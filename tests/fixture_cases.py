"""Fixtures a CPU test and its GPU counterpart both build: the FP8 quantiser's planted matrix
(tests/test_fp8_cpu.py, test_gpu_fp8_gemv.py) and the export-shaped checkpoint directory
(tests/test_checkpoint_cpu.py, test_gpu_checkpoint.py)."""
import json
import os

import torch

from conftest import GOLDEN

BF16 = torch.bfloat16


def planted_matrix(N, K, seed):
    """Random normal x 0.02 with the rows the rule's edges sit on: an all-zero row, amax =
    448 * 2^-3 (e = -3 exactly), amax = 464 * 2^-3 (just past it: e = -2), and 3.0 next to
    1e-4-scale values (most of the row lands in e4m3's subnormals)."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
    W[3] = 0
    W[5] = (W[5].float().clamp(-1, 1)).to(BF16)
    W[5, 7] = 448 * 2.0 ** -3
    W[6, K - 1] = -464 * 2.0 ** -3
    W[9] = (torch.randn(K, generator=g) * 1e-4).to(BF16)
    W[9, 0] = 3.0
    return W


def export_fixture():
    with open(os.path.join(GOLDEN, "golden_export.json")) as f:
        return json.load(f)


def write_export(path, fx=None, config_overrides=None, unpruned=False, shards=2):
    """An export directory of the golden_tiny_eager model: config.json + safetensors shards
    (+ model.safetensors.index.json), tensors under the reference export's names."""
    from safetensors.torch import save_file
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.weights import synthetic_weights
    fx = fx or export_fixture()
    cfg = named_config(fx["config"], **fx["config_kw"])
    sd = synthetic_weights(cfg, fx["weight_seed"])
    tensors = {k: sd[k] for k in fx["state_dict"]}
    if unpruned:
        for k, shape in fx["state_dict_unpruned_extra"].items():
            tensors[k] = torch.zeros(shape, dtype=torch.bfloat16)
    conf = dict(fx["config_json"])
    conf.update(config_overrides or {})
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(conf, f, indent=2)
    names = sorted(tensors)
    weight_map = {}
    for i in range(shards):
        part = names[i::shards]
        fn = f"model-{i + 1:05d}-of-{shards:05d}.safetensors"
        save_file({k: tensors[k].contiguous() for k in part}, os.path.join(path, fn), metadata={"format": "pt"})
        weight_map.update({k: fn for k in part})
    with open(os.path.join(path, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {}, "weight_map": weight_map}, f)
    return cfg, sd
