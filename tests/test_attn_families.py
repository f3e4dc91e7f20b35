"""The exact-answer attention inputs (tests/attn_families.py) checked on the host alone: what the GPU
tests take for granted about them, and that the bar they hold the kernels to has teeth."""
import numpy as np
import pytest
import torch

import attn_families as F

CASES = F.cases_used()


def _id(c):
    return f"{c[0]}-{c[1]}-{'causal' if c[2] else 'full'}{'-log2e' if c[3] else ''}"


def _exact_in_16_bits(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64))
    return all(torch.equal(t.to(td).double(), t) for td in (torch.bfloat16, torch.float16))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_family_precondition_and_representability(case):
    """For every (family, T, mask, q form) a GPU test runs, on the fp64 reference alone: each row's
    softmax mass outside its intended key(s) is <= 1e-6, the reference is within 32 x that (the span of V) of the exact
    answer, and every input and every exact answer survives a round trip through bf16 and fp16."""
    family, T, causal, log2e = case
    c = F.make(family, T, causal)
    assert c.qkv.shape == (F.B * T, 3 * F.D) and np.abs(c.qkv[:, 2 * F.D:]).max() <= 16
    assert _exact_in_16_bits(c.qkv) and _exact_in_16_bits(c.expect)
    ref_in = F.fold_log2e(c.qkv)[1] if log2e else c.qkv
    ref, p = F.reference(ref_in, T, causal)
    lk = F.leak(c, p)
    assert lk <= F.LEAK_CAP, lk
    assert np.abs(ref - c.expect).max() <= 32 * lk + 1e-12
    if log2e:   # the folded q keeps both intended scores equal
        s = np.einsum("bthd,bshd->bhts", *(np.asarray(ref_in, np.float64).reshape(F.B, T, 3, F.H, 64)[:, :, i]
                                            for i in range(2)))
        a, b = (np.take_along_axis(s, c.intended[..., i:i + 1], -1) for i in range(2))
        assert (a == b).all()


@pytest.mark.parametrize("family,causal", [("single", False), ("pair", False), ("single", True), ("pair", True),
                                           ("causal_pairs", True)])
def test_family_structure(family, causal):
    """what the issue asks of the index maps: every edge key (0, T-1, both sides of each multiple of 16)
    is some row's answer; causal rows look at no later key and the edge rows at themselves; the pair's
    keys lie in different 64-key tiles wherever two tiles are visible, with k_a . k_b >= 0; V rows of
    a sequence are pairwise distinct and neighbours differ in every dim."""
    for T in sorted(set(F.SMALL_T + F.DMA_T + F.MODE_T)) if not causal else F.SMALL_T + F.CAUSAL_LONG_T:
        c = F.make(family, T, causal)
        x = c.qkv.reshape(F.B, T, 3, F.H, 64)
        for b in range(F.B):
            for h in range(F.H):
                k, v, ab = x[b, :, 1, h], x[b, :, 2, h], c.intended[b, h]
                assert len({r.tobytes() for r in v}) == T
                assert T == 1 or (v[1:] != v[:-1]).all()
                assert family == "pair" or set(F._edges(T)) <= set(ab.ravel().tolist()), (T, b, h)
                if causal:
                    assert (ab <= np.arange(T)[:, None]).all()
                    assert family == "pair" or (ab[F._edges(T), 1] == F._edges(T)).all()
                if family == "single" and not causal:
                    assert sorted(ab[:, 0].tolist()) == list(range(T))
                if family == "pair":
                    two = (np.arange(T) >= 64) if causal else np.full(T, T > 64)
                    assert (ab[two, 0] // 64 != ab[two, 1] // 64).all()
                    assert (np.einsum("td,td->t", k[ab[:, 0]], k[ab[:, 1]]) >= 0).all()
                if family == "causal_pairs":
                    assert (k[0: T - (T & 1): 2] == k[1::2]).all()


@pytest.mark.parametrize("T", F.FUSED_T)
def test_batch_helper_precondition_and_planted_sequence_shift(T):
    """make_batch / reference(nb=...) as the fused-kernel tests use them, for every family and mask they
    run at this T and a batch with a partial last tile: sequence b is item b % 2 bit for bit, inputs and
    answers are exact in both 16-bit types, the leak is <= LEAK_CAP, and V rows read one sequence too
    far -- an error planted in the reference, never in a kernel -- break the bar in every sequence
    whose successor is the other item."""
    nb = F.fused_batches(T)[0]
    for family, causal in F.FUSED_FAMILIES:
        c2, c = F.make(family, T, causal), F.make_batch(family, T, causal, nb)
        assert c.qkv.shape == (nb * T, 3 * F.D) and c.intended.shape == (nb, F.H, T, 2)
        for b in range(nb):
            assert (c.qkv[b * T:(b + 1) * T] == c2.qkv[(b % 2) * T:(b % 2 + 1) * T]).all()
            assert (c.expect[b * T:(b + 1) * T] == c2.expect[(b % 2) * T:(b % 2 + 1) * T]).all()
        assert _exact_in_16_bits(c.qkv) and _exact_in_16_bits(c.expect)
        ref, p = F.reference(c.qkv, T, causal, nb=nb)
        lk = F.leak(c, p)
        assert lk <= F.LEAK_CAP, (family, lk)
        assert np.abs(ref - c.expect).max() <= 32 * lk + 1e-12
        assert (ref[: 2 * T] == F.reference(c2.qkv, T, causal)[0]).all()   # nb changes no existing answer
        bad, _ = F.reference(c.qkv, T, causal, fault="next_seq", nb=nb)
        hit = F.violations(bad, ref, "bfloat16").reshape(nb, -1).any(1)
        differs = np.arange(nb) % 2 != (np.arange(nb) + 1) % nb % 2
        assert hit[differs].all() and differs.sum() >= nb - 1, (family, T)


FAULTS = [("drop_last", "single", False), ("drop_last", "pair", False), ("drop_last", "single", True),
          ("drop_last", "pair", True), ("drop_last", "causal_pairs", True),
          ("swap_v", "single", False), ("swap_v", "pair", False), ("swap_v", "single", True),
          ("swap_v", "pair", True), ("swap_v", "causal_pairs", True),
          ("mask_minus", "single", True), ("mask_minus", "pair", True), ("mask_minus", "causal_pairs", True),
          ("mask_plus", "causal_pairs", True)]


@pytest.mark.parametrize("fault,family,causal", FAULTS)
def test_bar_catches_planted_errors(fault, family, causal):
    """Three deliberate errors planted in the fp64 reference (never in a kernel) -- key T-1 dropped,
    the causal mask shifted by one key, the V rows of neighbouring keys swapped -- each break the
    bar the GPU tests use (the wider, bf16 one) against the unmodified reference, at every T the
    family runs at. A mask that lets one later key in (mask_plus) changes no answer of single or pair,
    whose rows name their keys; the twin keys of causal_pairs are there to catch it."""
    used = sorted({c[1] for c in CASES if c[0] == family and c[2] == causal})
    assert used
    for T in used:
        if T == 1:
            continue   # one key: nothing to drop, swap or mask
        c = F.make(family, T, causal)
        ref, _ = F.reference(c.qkv, T, causal)
        bad, _ = F.reference(c.qkv, T, causal, fault=fault)
        n = int(F.violations(bad, ref, "bfloat16").sum())
        assert n > 0, (fault, family, T)
        assert not F.violations(ref, ref, "bfloat16").any()
