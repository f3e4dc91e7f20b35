"""Generate tests/golden/contrastive_loss.npz: inputs and outputs of the reference's own
compute_clip_contrastive_loss (scripts/train_lora.py:83-108), run where the read-only reference
exists (as make_eval_golden.py):

  python tests/golden/make_loss_golden.py

train_lora.py imports peft, the dataset and the adapter loader at module level; whatever is missing
here is stubbed in sys.modules for the import -- none of it is reached by the loss function.

Stored: the inputs a, b (float32 [257, 64], make_eval_golden.py's), T = 0.07, the reference's loss
on the fp32 tensors (`loss32`), the same function on float64 tensors (`loss64`), their gap (`gap`:
what the reference's own fp32 arithmetic is worth), and the validation number of train_lora.py:
213-241 at B = 32 -- the mean over consecutive batches, the last short one included, of the same
function's per-batch loss -- on fp32 (`batch32`) and fp64 (`batch64`) tensors with their gap
(`batch_gap`).
"""
from __future__ import annotations

import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
T = 0.07
B = 32


def _load_reference_loss():
    stubs = {}
    for name in ("peft", "yaml", "tqdm", "transformers", "datasets", "datasets.dataset", "models",
                 "models.clip_model", "models.lora_adapter", "src", "src.utils", "src.utils.config"):
        try:
            importlib.import_module(name)
        except Exception:
            stubs[name] = types.ModuleType(name)
    for name, mod in stubs.items():
        mod.__path__ = []
        mod.__getattr__ = lambda attr: None   # `from stub import anything` gives None
        sys.modules[name] = mod
    if "tqdm" in stubs:
        stubs["tqdm"].tqdm = lambda it, **kw: it
    try:
        spec = importlib.util.spec_from_file_location("ref_train_lora", os.path.join(REF, "scripts/train_lora.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name in stubs:
            sys.modules.pop(name, None)
    return mod.compute_clip_contrastive_loss


def _batched(fn, a: torch.Tensor, b: torch.Tensor) -> float:
    total, n = 0.0, 0
    for s in range(0, a.shape[0], B):
        total += fn(a[s:s + B], b[s:s + B], T).item()   # train_lora.py:232-234
        n += 1
    return total / n


def main():
    loss = _load_reference_loss()
    rng = np.random.default_rng(0)
    a = rng.standard_normal((257, 64)).astype(np.float32)
    b = (a + 3.0 * rng.standard_normal((257, 64))).astype(np.float32)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    with torch.no_grad():
        l32 = loss(ta, tb, T).item()
        l64 = loss(ta.double(), tb.double(), T).item()
        b32 = _batched(loss, ta, tb)
        b64 = _batched(loss, ta.double(), tb.double())
    out = {"a": a, "b": b, "T": np.float64(T), "loss32": np.float64(l32), "loss64": np.float64(l64),
           "gap": np.float64(abs(l32 - l64)), "B": np.int64(B), "batch32": np.float64(b32),
           "batch64": np.float64(b64), "batch_gap": np.float64(abs(b32 - b64))}
    np.savez_compressed(os.path.join(HERE, "contrastive_loss.npz"), **out)
    print(f"contrastive_loss.npz: loss32 {l32:.10f} loss64 {l64:.10f} gap {abs(l32 - l64):.2e}; "
          f"B={B}: {b32:.10f} / {b64:.10f} gap {abs(b32 - b64):.2e}")


if __name__ == "__main__":
    main()
