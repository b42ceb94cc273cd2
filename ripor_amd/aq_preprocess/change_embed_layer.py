"""CLI-compatible replacement of reference aq_preprocess/change_embed_layer.py: the K = 256 case of
change_customized_embed_layer (same outputs)."""
from __future__ import annotations

from .change_customized_embed_layer import change_embed_layer, get_args  # noqa: F401


def main(argv=None):
    args = get_args(argv)
    print("model_dir: ", args.model_dir, "K: ", args.K)
    return change_embed_layer(args.model_dir, args.K, args.seed)


if __name__ == "__main__":
    main()
