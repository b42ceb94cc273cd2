"""CLI-compatible replacement of reference aq_preprocess/change_customized_embed_layer.py:18-90.

Loads ``model_dir/checkpoint``, makes the residual quantizer's codebooks (``model_dir/aq_index``) the decoder's output
embeddings (``list_output_embeds.i = codebook i``, reference T5SeqAQEncoder.assign_output_embeds,
t5_generative_retriever.py:832-846), gives the decoder fresh input embeddings ``list_decoder_embeds.i`` ~ N(0, 1) (as
nn.Embedding initialises them; seeded here), sets ``decoder_vocab_sizes = [K] * M`` and ``max_decoder_length = M`` and
saves ``model_dir/no_share_checkpoint`` with the tokenizer files."""
from __future__ import annotations

import argparse
import os
import shutil

import numpy as np
import torch

TOKENIZER_FILES = ("spiece.model", "tokenizer.json", "tokenizer_config.json", "special_tokens_map.json", "added_tokens.json")


def get_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_dir", default=None, type=str)
    ap.add_argument("--K", default=256, type=int)
    ap.add_argument("--seed", default=0, type=int, help="seed of the fresh decoder input embeddings")
    return ap.parse_args(argv)


def change_embed_layer(model_dir: str, K: int, seed: int = 0) -> str:
    from ripor_amd.modeling.t5_generative_retriever import T5ForDocIDGeneration, T5forDocIDConfig, _load_checkpoint
    from ripor_amd.tasks.rq_indexer import load_index

    pretrained_path = os.path.join(model_dir, "checkpoint")
    out_dir = os.path.join(model_dir, "no_share_checkpoint")
    books, info = load_index(os.path.join(model_dir, "aq_index"))
    M = info["M"]
    if info["K"] != K:
        raise ValueError(f"--K {K}, but the index in {model_dir}/aq_index has K = {info['K']}")
    config = T5forDocIDConfig.from_pretrained(pretrained_path)
    print("M, K, d_model are: ", M, K, config.d_model)
    if books.shape[2] != config.d_model:
        raise ValueError(f"codebooks of width {books.shape[2]} for a model of d_model {config.d_model}")
    sd = _load_checkpoint(pretrained_path)
    old = [k for k in sd if k.startswith("list_decoder_embeds.") or k.startswith("list_output_embeds.")]
    print("before modifying embed_layers")
    for k in old:
        print(k, tuple(sd[k].shape))
    for k in old:
        del sd[k]
    g = torch.Generator().manual_seed(seed)
    for i in range(M):
        sd[f"list_decoder_embeds.{i}.weight"] = torch.randn((K, config.d_model), generator=g, dtype=torch.float32)
        sd[f"list_output_embeds.{i}.weight"] = torch.from_numpy(np.ascontiguousarray(books[i], dtype=np.float32))
    config.shared_output_input_embeds = False
    config.decoder_vocab_sizes = [K] * M
    config.max_decoder_length = M
    model = T5ForDocIDGeneration(config, sd)
    print("after modifying embed_layers")
    for i in range(M):
        for name in (f"list_decoder_embeds.{i}.weight", f"list_output_embeds.{i}.weight"):
            print(name, tuple(sd[name].shape))
    os.makedirs(out_dir, exist_ok=True)
    model.save_pretrained(out_dir)
    for f in TOKENIZER_FILES:
        src = os.path.join(pretrained_path, f)
        if os.path.exists(src):
            shutil.copyfile(src, os.path.join(out_dir, f))
    return out_dir


def main(argv=None):
    args = get_args(argv)
    print("model_dir: ", args.model_dir, "K: ", args.K)
    return change_embed_layer(args.model_dir, args.K, args.seed)


if __name__ == "__main__":
    main()
