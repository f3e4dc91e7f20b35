"""The keyed selecting epilogue alone (gemm_common.hpp: EPI_FILTER_KEYS, through clm_gemm_select_keyed) on
the heuristic's tile (config -1) and on every tile the selecting epilogues accept (1, 8-11).

The oracle is the masked epilogue: per row, the count and the (score bits, id) set must be exactly what
clm_gemm_select(CLM_EPI_FILTER_MASK) gives that row under the mask of its own open columns, {n : klo[m]
<= keys[n] <= khi[m]}. The rows of a case share a few distinct ranges, so the masked run of one range
covers all its rows at once (the same tile, the same M); a handful of rows are also run alone (M = 1).
N = 255 takes the ragged (scalar) epilogue, 256 one tile's vector path, 3000 many tiles and a partial
one; with cbound the skip test runs, without it nothing is skipped -- the selected sets are the same.
"""
import numpy as np
import pytest
import torch

from clip_lora_match_amd import _capi as C

pytestmark = pytest.mark.gpu

MASK = C.CLM_EPI_FILTER_MASK
CFGS = [-1, 1, 8, 9, 10, 11]
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
# (klo, khi): everything, empty (klo > khi), a band, one key, a band no key lies in, the sentinel alone
RANGES = [(I32_MIN, I32_MAX), (5, 4), (3, 7), (5, 5), (20, 30), (-1, -1), (0, 15)]
BASE = (1 << 32) + 77


def _p(t):
    return C.ptr(t) if t is not None else None


def _st():
    return C.stream_of(torch.device("cuda:0"))


def _mask_words(allowed):
    a = allowed.cpu().numpy().astype(np.uint8)
    b = np.packbits(a, bitorder="little")
    b = np.concatenate([b, np.zeros(-len(b) % 4, dtype=np.uint8)])
    return torch.from_numpy(b.view(np.int32).copy()).cuda()


def _bounds(cs):
    keys = torch.zeros(2, dtype=torch.int32, device="cuda")
    C.check(C.lib().clm_value_bounds(0, C.ptr(cs), cs.numel(), C.ptr(keys), _st()), "clm_value_bounds")
    return keys


def _case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) / K ** 0.5).half().cuda()
    W = torch.randn(N, K, generator=g).half().cuda()
    rs = (0.5 + torch.rand(M, generator=g)).cuda()
    cs = (0.5 + torch.rand(N, generator=g)).cuda()
    # thresholds from "everything passes" to "a few per cent pass" (scores are about N(0, 1))
    theta = torch.tensor([(-100.0, 0.0, 1.0, 2.0)[i % 4] for i in range(M)]).cuda()
    keys = torch.randint(-1, 16, (N,), generator=g).to(torch.int32).cuda()
    which = torch.arange(M) % len(RANGES) if M > 1 else torch.tensor([2])
    klo = torch.tensor([RANGES[i][0] for i in which.tolist()], dtype=torch.int32).cuda()
    khi = torch.tensor([RANGES[i][1] for i in which.tolist()], dtype=torch.int32).cuda()
    return A, W, rs, cs, theta, keys, klo, khi, which


def _alloc(M, cap):
    return (torch.zeros(M, dtype=torch.int32, device="cuda"), torch.full((M, cap), -99.0, device="cuda"),
            torch.full((M, cap), -12345, dtype=torch.int64, device="cuda"))


def _keyed(cfg, A, W, rs, cs, theta, keys, klo, khi, cap, cbound, expect=C.CLM_OK):
    M, K = A.shape
    cnt, cand_s, cand_i = _alloc(M, cap)
    rc = C.lib().clm_gemm_select_keyed(0, cfg, C.ptr(A), A.stride(0), C.ptr(W), W.stride(0), M, W.shape[0], K, _p(rs),
                                       C.ptr(cs), C.ptr(theta), 1, C.ptr(cnt), C.ptr(cand_s), C.ptr(cand_i), cap, BASE,
                                       _p(cbound), _p(keys), _p(klo), _p(khi), 1, _st())
    assert rc == expect, (rc, C.lib().clm_last_error())
    return cnt, cand_s, cand_i


def _masked(cfg, A, W, rs, cs, theta, words, cap, cbound):
    M, K = A.shape
    cnt, cand_s, cand_i = _alloc(M, cap)
    above = torch.zeros(M, dtype=torch.int32, device="cuda")
    C.check(C.lib().clm_gemm_select(0, MASK, cfg, C.ptr(A), A.stride(0), C.ptr(W), W.stride(0), M, W.shape[0], K,
                                    _p(rs), C.ptr(cs), C.ptr(theta), 1, 0.0, C.ptr(cnt), C.ptr(cand_s), C.ptr(cand_i),
                                    cap, BASE, _p(cbound), C.ptr(above), None, 0, 0.0, C.ptr(words), 1, _st()),
            "clm_gemm_select")
    return cnt, cand_s, cand_i


def _canon(res, N, cap):
    """(rows sorted [M, cap] of (score bits << 12 | column) with the unused slots at the end, used [M, cap]),
    after checking the slot discipline: the first min(cnt, cap) slots hold ids BASE + n, 0 <= n < N, the
    others keep the caller's fill"""
    cnt, cand_s, cand_i = res
    used = torch.arange(cap, device="cuda")[None, :] < cnt.clamp(max=cap)[:, None]
    n = cand_i - BASE
    assert bool(((n >= 0) & (n < N))[used].all()), "a stored id is not BASE + n"
    assert bool((cand_i[~used] == -12345).all()) and bool((cand_s[~used] == -99.0).all()), "a slot past the count written"
    comp = ((cand_s.contiguous().view(torch.int32).long() & 0xFFFFFFFF) << 12) | n.clamp(0, 4095)
    return torch.where(used, comp, torch.full_like(comp, 1 << 62)).sort(1).values, used


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("N", [255, 256, 3000])
def test_keyed_epilogue_equals_the_masked_one_row_by_row(cfg, N):
    assert N < 4096   # _canon's column field
    for K in (64, 512):
        for M in (1, 17, 300):
            A, W, rs, cs, theta, keys, klo, khi, which = _case(M, N, K, 7 * N + K + M)
            for cbound in (None, _bounds(cs)):
                got = _keyed(cfg, A, W, rs, cs, theta, keys, klo, khi, N, cbound)
                small = _keyed(cfg, A, W, rs, cs, theta, keys, klo, khi, 7, cbound)      # cap below the counts
                assert torch.equal(small[0], got[0]), "the count does not depend on cap"
                assert int(got[0].max()) > 7 and int(got[0].max()) <= N
                cg, _ = _canon(got, N, N)
                csm, used_sm = _canon(small, N, 7)
                # what a cap of 7 stored is a subset of the row's full list
                pos = torch.searchsorted(cg, csm).clamp(max=N - 1)
                assert bool((torch.gather(cg, 1, pos) == csm)[used_sm].all())
                listed = 0
                for r in sorted(set(which.tolist())):
                    lo_r, hi_r = RANGES[r]
                    open_r = (keys >= lo_r) & (keys <= hi_r)
                    ref = _masked(cfg, A, W, rs, cs, theta, _mask_words(open_r), N, cbound)
                    rows = torch.nonzero(which == r).reshape(-1).cuda()
                    assert torch.equal(got[0][rows], ref[0][rows]), (K, M, r)
                    cr, used_r = _canon(ref, N, N)
                    assert torch.equal(cg[rows], cr[rows]), (K, M, r)          # the same (score bits, id) sets
                    stored = (got[2][rows] - BASE).clamp(0, N - 1)
                    assert bool(open_r[stored][used_r[rows]].all())              # ... of open columns only
                    listed += int(got[0][rows].sum())
                    if r in (1, 4):   # the empty range and the band without keys list nothing
                        assert int(got[0][rows].sum()) == 0
                    elif r == 0 and M > 1:   # everything open, theta = -100 on row 0: every column
                        assert int(got[0][0]) == N
                assert listed > 0
                # a few rows alone (M = 1), each under its own mask
                for m in sorted(set([0, M // 2, M - 1])):
                    words = _mask_words((keys >= int(klo[m])) & (keys <= int(khi[m])))
                    one = _masked(cfg, A[m: m + 1], W, rs[m: m + 1], cs, theta[m: m + 1], words, N, cbound)
                    assert int(one[0][0]) == int(got[0][m])
                    assert torch.equal(_canon(one, N, N)[0][0], cg[m]), (K, M, m)


def test_keyed_hook_refuses_what_it_cannot_run():
    A, W, rs, cs, theta, keys, klo, khi, _ = _case(17, 256, 64, 3)
    for cfg in (0, 2, 3, 4, 5, 6, 7, 12, 13, 14):     # tiles without the epilogue: the launcher's answer
        cnt, cand_s, cand_i = _keyed(cfg, A, W, rs, cs, theta, keys, klo, khi, 256, None, expect=C.CLM_E_HIP)
        assert int(cnt.sum()) == 0 and bool((cand_i == -12345).all())
    for drop in range(3):                             # keys, klo, khi are all required
        args = [keys, klo, khi]
        args[drop] = None
        _keyed(-1, A, W, rs, cs, theta, *args, 256, None, expect=C.CLM_E_ARG)
    # clm_gemm_select has no room for the keys: it refuses the epilogue
    cnt, cand_s, cand_i = _alloc(17, 256)
    rc = C.lib().clm_gemm_select(0, C.CLM_EPI_FILTER_KEYS, -1, C.ptr(A), 64, C.ptr(W), 64, 17, 256, 64, _p(rs), C.ptr(cs),
                                 C.ptr(theta), 1, 0.0, C.ptr(cnt), C.ptr(cand_s), C.ptr(cand_i), 256, 0, None, None, None,
                                 0, 0.0, None, 1, _st())
    assert rc == C.CLM_E_ARG
