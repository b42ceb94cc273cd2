from ripor_amd.modeling.cross_encoder import CrossEncoder  # noqa: F401
