"""Generate tests/golden/contrastive_loss_grad.npz: the gradients of the reference's own
compute_clip_contrastive_loss (scripts/train_lora.py:83-108) by its own autograd, run where the
read-only reference exists (as make_loss_golden.py, whose loader and inputs this reuses):

  python tests/golden/make_loss_grad_golden.py

Stored: the inputs a, b (float32 [257, 64], make_loss_golden.py's) and T = 0.07; loss.backward()'s
gradients with respect to a and b on float64 leaf tensors (`grad_a64`, `grad_b64`: the yardstick)
and on float32 ones (`grad_a32`, `grad_b32`); `gap` = the largest absolute difference between the
two (what the reference's own fp32 arithmetic is worth). The function normalises its inputs inside,
so these are gradients with respect to the raw, unnormalised rows.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_loss_golden import T, _load_reference_loss  # noqa: E402


def _grads(loss, a: np.ndarray, b: np.ndarray, dtype):
    ta = torch.from_numpy(a).to(dtype).requires_grad_(True)
    tb = torch.from_numpy(b).to(dtype).requires_grad_(True)
    loss(ta, tb, T).backward()
    return ta.grad.numpy(), tb.grad.numpy()


def main():
    loss = _load_reference_loss()
    rng = np.random.default_rng(0)
    a = rng.standard_normal((257, 64)).astype(np.float32)
    b = (a + 3.0 * rng.standard_normal((257, 64))).astype(np.float32)
    ga64, gb64 = _grads(loss, a, b, torch.float64)
    ga32, gb32 = _grads(loss, a, b, torch.float32)
    gap = max(np.abs(ga32 - ga64).max(), np.abs(gb32 - gb64).max())
    np.savez_compressed(os.path.join(HERE, "contrastive_loss_grad.npz"), a=a, b=b, T=np.float64(T), grad_a64=ga64,
                        grad_b64=gb64, grad_a32=ga32, grad_b32=gb32, gap=np.float64(gap))
    print(f"|grad| max {np.abs(ga64).max():.3e}, fp32 - fp64 gap {gap:.3e}")


if __name__ == "__main__":
    main()
