"""numpy float64 restatement of the streaming contrastive-loss gradient: the yardstick of
tests/test_loss_grad_host.py and tests/test_gpu_loss_grad.py. Nothing here shares code with the
package.

  unit(x)                         rows / their norms
  lse_rows(qu, ru, scale)         log sum_j exp(scale * qu_i . ru_j), per row i
  softmax_grad_ref(...)           dq, dr and the weight masses A of CosineIndex.softmax_grad, chunked
                                  over the index rows like the GPU route (the chunk must not matter)
  contrastive_grad_ref(a, b, T)   the loss's gradients with respect to the raw rows, assembled from
                                  log-sum-exps, the weighted sums, the diagonal and the normalise
                                  backward
"""
import numpy as np


def unit(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def lse_rows(qu, ru, scale):
    x = scale * (qu @ ru.T)
    m = x.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def softmax_grad_ref(qu, ru, scale, q_lse, row_lse=None, wq=1.0, wr=1.0, chunk=None):
    """(dq [nq, d], dr [N, d], Aq [nq], Ar [N]) in float64 from unit rows qu, ru: W_ij = wq exp(scale
    s_ij - q_lse[i]) + wr exp(scale s_ij - row_lse[j]) (the second term absent without row_lse), dq =
    W ru, dr = W^T qu, Aq / Ar = W's row / column sums."""
    qu, ru = np.asarray(qu, dtype=np.float64), np.asarray(ru, dtype=np.float64)
    nq, n = qu.shape[0], ru.shape[0]
    chunk = n if not chunk else int(chunk)
    dq, dr = np.zeros_like(qu), np.zeros_like(ru)
    aq, ar = np.zeros(nq), np.zeros(n)
    q_lse = np.asarray(q_lse, dtype=np.float64)
    for r0 in range(0, n, chunk):
        rc = ru[r0:r0 + chunk]
        x = scale * (qu @ rc.T)
        w = wq * np.exp(x - q_lse[:, None])
        if row_lse is not None:
            w = w + wr * np.exp(x - np.asarray(row_lse, dtype=np.float64)[None, r0:r0 + chunk])
        dq += w @ rc
        dr[r0:r0 + chunk] = w.T @ qu
        aq += w.sum(axis=1)
        ar[r0:r0 + chunk] = w.sum(axis=0)
    return dq, dr, aq, ar


def normalize_backward_ref(g, x):
    x = np.asarray(x, dtype=np.float64)
    nrm = np.linalg.norm(x, axis=1, keepdims=True)
    xu = x / nrm
    return (g - (g * xu).sum(axis=1, keepdims=True) * xu) / nrm


def contrastive_grad_ref(a, b, T, chunk=None):
    """(grad_a, grad_b, Aq, Ar): d loss / d a and d loss / d b of the symmetric InfoNCE loss of the
    pairs (a_i, b_i) at temperature T with respect to the raw rows, and the weight masses of the rows"""
    au, bu = unit(a), unit(b)
    n = au.shape[0]
    lse_i = lse_rows(au, bu, 1.0 / T)
    lse_t = lse_rows(bu, au, 1.0 / T)
    dq, dr, aq, ar = softmax_grad_ref(au, bu, 1.0 / T, lse_i, lse_t, 1.0, 1.0, chunk)
    ga = dq / (2 * n * T) - bu / (n * T)
    gb = dr / (2 * n * T) - au / (n * T)
    return normalize_backward_ref(ga, a), normalize_backward_ref(gb, b), aq, ar
