"""clip_lora_match_amd -- MI355X-native CLIP+LoRA encode -> L2-normalise -> cosine top-k.

Drop-in for the reference's `models/clip_model.py`, `models/lora_adapter.py` and
`src/embedding/*` API; compute runs in hand-written gfx950 HIP kernels behind the
C-ABI library `libclm.so` (include/clm.h).
"""
from .config import ModelConfig, TowerConfig, PRESETS, get_preset  # noqa: F401

# the retrieval evaluator (evaluate.py), loaded on first use: importing the package stays light
_EVALUATE = ("retrieval_ranks", "recall_at_k", "mrr", "mean_average_precision", "evaluate_retrieval",
             "matching_accuracy", "contrastive_loss", "CLIPEvaluator", "contrastive_loss_grad",
             "contrastive_loss_tensor", "ContrastiveLoss")

__all__ = ["ModelConfig", "TowerConfig", "PRESETS", "get_preset", *_EVALUATE]


def __getattr__(name):
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
