"""Attention inputs with exactly known answers (tests/test_attn_families.py, tests/test_gpu_attention.py,
tests/attn_mode_worker.py, tests/test_gpu_fused_attention.py): qkv [B*T, 3*H*64] whose every value is exact in bf16 and in fp16, built so
that each query's softmax sits on one key or on two equally scored keys, and an fp64 reference of
softmax(q k^T [+ causal mask]) v per (batch, head).

Layout, shared by the families: B = 2, H = 3; keys are +-1 codes of 64 dims drawn per (T, head,
batch), redrawn until no two distinct keys agree in more than 50 dims (dot <= 36); V rows are integers
in [-16, 16] computed from the key index with four moduli (33, 32, 31, 29) and odd multipliers, so any
two keys of a sequence differ and neighbouring keys differ in every dim; the output has ldo = H*64 + 64
and B*T + 8 rows, pre-filled with SENTINEL. make_batch cycles the two batch items into a batch of any
size for the fused kernel, whose tiles hold many sequences.

  single        q_i = k_pi(i): score 64 on the intended key, N(0, 64) elsewhere; answer v_pi(i).
                pi is a seeded permutation (every key is somebody's answer: key 0, key T-1, both sides
                of every multiple of 16); causal: pi(i) = i on those edge keys, a seeded key <= i elsewhere.
  pair          q_i = 2 (k_a + k_b), entries in {-4, 0, 4}: both keys score 2 (64 + k_a.k_b), the answer
                is (v_a + v_b) / 2 exactly. a and b lie in different 64-key tiles when T > 64 (causal:
                when i >= 64) and as far apart as possible otherwise, with k_a.k_b >= 0 and every other
                key at least 24 below the pair. Causal: a = i, the mask's edge, wherever a partner exists.
  causal_pairs  causal only: k_2m = k_2m+1, q_i = k_i. Row 2m sees one of the twins (answer v_2m), row
                2m+1 both ((v_2m + v_2m+1) / 2): a mask off by one either way moves a row by >= 0.5.
"""
import functools
from collections import namedtuple

import numpy as np

B, H, HD = 2, 3, 64
D = H * HD
LDO = D + 64
PAD_ROWS = 8
SENTINEL = -99.0
LOG2E = 1.4426950408889634
HALF_ULP = {"bfloat16": 2.0 ** -9, "float16": 2.0 ** -12}
ABS_TERM = 1e-4          # max|v| (16) x the leak cap (1e-6), 6x margin: covers answers of 0
LEAK_CAP = 1e-6
FAMILIES = ("single", "pair", "causal_pairs")

# the sequence lengths of the GPU tests: attn_small_kernel's wave (16) and key-tile (64) edges; the
# long kernels' tails of 1 / 0 / 1 / 0 / 1 / 0 / 1 keys of a 64-key tile, one query in the last
# 128-query block (129, 257), 2 keys (130), 5 full tiles (320) and the L/14 length
SMALL_T = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 77, 127, 128)
DMA_T = (129, 192, 193, 256, 257, 320, 577)
CAUSAL_LONG_T = (129, 192, 257)
MODE_T = (129, 130, 192, 193, 256, 257, 577)


def cases_used():
    """every (family, T, causal, log2e) the GPU tests run"""
    out = []
    for T in SMALL_T:
        out += [("single", T, False, False), ("pair", T, False, False), ("causal_pairs", T, True, False)]
    for T in sorted(set(DMA_T) | set(MODE_T)):
        out += [(f, T, False, False) for f in ("single", "pair")]
    out += [(f, T, False, True) for T in DMA_T for f in ("single", "pair")]
    out += [(f, T, True, False) for T in CAUSAL_LONG_T for f in FAMILIES]
    return out


# the fused q/k/v + attention kernel (k_gemm_attn.hip, tests/test_gpu_fused_attention.py): a tile holds
# G = 256 // T sequences, which changes at 42/43, 51/52, 64/65, 85/86 and 128; the second key tile is
# empty at 64 and holds one key at 65; the causal nkt goes from one key tile to two at query 48 -> 49
FUSED_T = (1, 2, 15, 16, 17, 31, 32, 33, 42, 43, 48, 49, 50, 51, 52, 63, 64, 65, 77, 85, 86, 127, 128)
FUSED_FAMILIES = (("single", False), ("pair", False), ("causal_pairs", True), ("single", True))


def fused_batches(T):
    """the batch sizes of the fused kernel's fixed-length tests: one sequence in the last tile
    (G + 1) and one short of two full tiles (2 G - 1)"""
    G = 256 // T
    return sorted({G + 1, 2 * G - 1})


_MODS = (33, 32, 31, 29)
_MULS = (1, 5, 7, 13, 17, 19, 23, 25, 35, 37, 41, 43, 47, 49, 53, 59)   # coprime to every modulus

Case = namedtuple("Case", "family T causal qkv intended expect")
# qkv      float32 [B*T, 3*D]; intended  int [B, H, T, 2] (the one or two keys a row must return);
# expect   float64 [B*T, D], the exact answer


def _values(T, h, b):
    j = np.arange(T)[:, None]
    c = np.arange(HD)[None, :]
    mod = np.array(_MODS)[c % 4]
    mul = np.array(_MULS)[c // 4]
    return ((j * mul + c + 3 * h + 7 * b) % mod - 16).astype(np.float64)


def _keys(rng, n):
    while True:
        k = rng.integers(0, 2, (n, HD)) * 2.0 - 1.0
        g = k @ k.T
        np.fill_diagonal(g, 0)
        if n == 1 or np.abs(g).max() <= 36:
            return k


def _edges(T):
    e = {0, T - 1}
    for m in range(16, T + 1, 16):
        e.update((m - 1, m))
    return sorted(x for x in e if x < T)


def _single(rng, T, causal, k):
    if not causal:
        pi = rng.permutation(T)
    else:
        pi = np.array([rng.integers(0, i + 1) for i in range(T)])
        pi[_edges(T)] = _edges(T)
    return k[pi], np.stack([pi, pi], 1)


def _pair(rng, T, causal, k):
    g = k @ k.T
    order = rng.permutation(T)
    ab = np.zeros((T, 2), dtype=np.int64)
    for i in range(T):
        hi = i if causal else T - 1            # last visible key
        found = None
        for step in range(T):
            # causal: the row's own key first (the mask's edge), then earlier ones
            a = i - step if causal else int(order[(i + step) % T])
            if a < 0:
                break
            if hi >= 64:
                cand = [x for x in rng.permutation(hi + 1) if x // 64 != a // 64]
            else:
                cand = sorted((x for x in range(hi + 1) if x != a), key=lambda x: -abs(x - a))[:8]
            for bb in cand:
                others = g[a] + g[bb]
                top = others[a]
                vis = np.ones(T, bool)
                vis[[a, bb]] = False
                vis[hi + 1:] = False
                if g[a, bb] >= 0 and (not vis.any() or others[vis].max() <= top - 12):
                    found = (a, int(bb))
                    break
            if found:
                break
        if found is None:      # a row with too few visible keys for a pair: its own key, alone
            assert hi < 64, (T, i)
            found = (hi, hi)
        ab[i] = found
    return 2.0 * (k[ab[:, 0]] + k[ab[:, 1]]), ab


@functools.lru_cache(maxsize=None)
def make(family, T, causal):
    """The case of one (family, T, mask). Cached; the arrays are read-only."""
    assert family in FAMILIES and (causal or family != "causal_pairs")
    qkv = np.zeros((B, T, 3, H, HD))
    intended = np.zeros((B, H, T, 2), dtype=np.int64)
    expect = np.zeros((B, T, H, HD))
    for b in range(B):
        for h in range(H):
            rng = np.random.default_rng([FAMILIES.index(family), int(causal), T, h, b])
            v = _values(T, h, b)
            if family == "causal_pairs":
                k = np.repeat(_keys(rng, (T + 1) // 2), 2, axis=0)[:T]
                q = k
                i = np.arange(T)
                tw = np.stack([i - (i & 1), i], 1)   # even rows: themselves; odd rows: both twins
            else:
                k = _keys(rng, T)
                q, tw = (_single if family == "single" else _pair)(rng, T, causal, k)
            qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = q, k, v
            intended[b, h] = tw
            expect[b, :, h] = 0.5 * (v[tw[:, 0]] + v[tw[:, 1]])
    out = Case(family, T, causal, qkv.reshape(B * T, 3 * D).astype(np.float32), intended, expect.reshape(B * T, D))
    for a in out[3:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def make_batch(family, T, causal, nb):
    """make()'s case as a batch of nb sequences, sequence b being item b % 2: neighbours in a batch
    (and in a tile of the fused kernel, tests/test_gpu_fused_attention.py) carry different keys and
    values, so a sequence offset that is one off returns another item's V row. qkv [nb*T, 3*D],
    intended [nb, H, T, 2], expect [nb*T, D]; read-only. Goes with reference(..., nb=nb)."""
    c = make(family, T, causal)
    idx = np.arange(nb) % B
    out = Case(family, T, causal, c.qkv.reshape(B, T, 3 * D)[idx].reshape(nb * T, 3 * D), c.intended[idx],
               c.expect.reshape(B, T, D)[idx].reshape(nb * T, D))
    for a in out[3:]:
        a.setflags(write=False)
    return out


def fold_log2e(qkv):
    """(kernel input, reference input) of the CLM_ATTN_Q_LOG2E form: q times log2 e in fp32, rounded
    once to bf16; the reference sees that rounded q with log2 e divided back out in fp32."""
    import torch
    t = torch.from_numpy(np.array(qkv))
    t[:, :D] *= LOG2E
    folded = t.to(torch.bfloat16)
    ref_in = folded.float()
    ref_in[:, :D] /= LOG2E
    return folded, ref_in.numpy()


def reference(qkv, T, causal, fault=None, nb=B):
    """fp64 softmax(q k^T [+ causal mask]) v -> (out [nb*T, D], probabilities [nb, H, T, T]), nb = B
    sequences unless given (make_batch).
    `fault` plants one deliberate error in this reference (never in a kernel), for the tests that show
    the bar would catch it: "drop_last" hides key T-1, "mask_minus" / "mask_plus" shift the causal
    mask by one key (row 0 keeps key 0), "swap_v" pairs keys 2m and 2m+1 with each other's V rows,
    "next_seq" reads every sequence's V rows one sequence further on (the last one's from the first)."""
    x = np.asarray(qkv, dtype=np.float64).reshape(nb, T, 3, H, HD)
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))   # [B, H, T, 64]
    if fault == "swap_v":
        idx = np.arange(T)
        idx[: T - (T & 1)] ^= 1
        v = v[:, :, idx]
    if fault == "next_seq":
        v = np.roll(v, -1, axis=0)
    s = q @ k.transpose(0, 1, 3, 2)
    ki, qi = np.arange(T)[None, :], np.arange(T)[:, None]
    vis = np.ones((T, T), bool)
    if causal:
        vis = ki <= qi + {"mask_minus": -1, "mask_plus": 1}.get(fault, 0)
        vis[0, 0] = True
    else:
        assert fault not in ("mask_minus", "mask_plus")
    if fault == "drop_last":
        assert T > 1
        vis = vis & (ki < T - 1)
    s = np.where(vis, s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(nb * T, D), p


def leak(case, p):
    """largest softmax mass, over all rows, that lies outside the row's intended key(s)"""
    a, b = case.intended[..., :1], case.intended[..., 1:]
    on = np.take_along_axis(p, a, -1) + np.where(a == b, 0.0, np.take_along_axis(p, b, -1))
    return float((1.0 - on).max())


def violations(got, ref, dtype):
    """elements of `got` outside |got - ref| <= h |ref| + 1e-4, h half an ulp of dtype"""
    return np.abs(got - ref) > HALF_ULP[dtype] * np.abs(ref) + ABS_TERM


def run_on_gpu(family, T, causal, dtype, log2e=False):
    """Run one case through clm_attention_ex on the current device and hold it to the bar; columns
    past d and rows past B*T must keep the sentinel. Returns the largest |out - ref64|."""
    import torch
    from clip_lora_match_amd import _capi as C
    td, ct = {"bfloat16": (torch.bfloat16, C.CLM_BF16), "float16": (torch.float16, C.CLM_F16)}[dtype]
    case = make(family, T, causal)
    if log2e:
        assert dtype == "bfloat16" and not causal
        dev_in, ref_in = fold_log2e(case.qkv)
        dev_in = dev_in.cuda()
    else:
        dev_in, ref_in = torch.from_numpy(np.array(case.qkv)).to(td).cuda(), case.qkv
        assert torch.equal(dev_in.float().cpu(), torch.from_numpy(np.array(case.qkv)))
    ref, p = reference(ref_in, T, causal)
    assert leak(case, p) <= LEAK_CAP
    out = torch.full((B * T + PAD_ROWS, LDO), SENTINEL, device="cuda").to(td)
    flags = (C.CLM_ATTN_CAUSAL if causal else 0) | (C.CLM_ATTN_Q_LOG2E if log2e else 0)
    C.check(C.lib().clm_attention_ex(0, ct, flags, C.ptr(dev_in), C.ptr(out), out.stride(0), B, T, H,
                                     C.stream_of(dev_in.device)), "clm_attention_ex")
    got = out.double().cpu().numpy()
    what = (family, T, "causal" if causal else "full", dtype, "log2e" if log2e else "")
    assert (got[:, D:] == SENTINEL).all(), ("columns past d written", what)
    assert (got[B * T:] == SENTINEL).all(), ("rows past B*T written", what)
    got = got[: B * T, :D]
    err = np.abs(got - ref)
    bad = violations(got, ref, dtype)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} elements off the bar, max |err| {err.max():.3e}; first at "
                             f"row {r} (batch {r // T}, query {r % T}) col {c} (head {c // HD}): got {got[r, c]}, "
                             f"want {ref[r, c]}, intended keys {case.intended[r // T, c // HD, r % T].tolist()}")
    return float(err.max())
