"""The varlen text plan (text_plan, k_ops.hip: lengths, prefix sums, tiles and row map of the live
caption rows) through clm_text_plan against a plain numpy reference (tests/text_plan_ref.py). Integers:
every comparison is exact equality. B runs past 256 (more than one caption per thread of the one-
workgroup scan) up to the launcher's 4096, L from 1 to 256, and the length patterns put 256 captions
in a tile, fill tiles to exactly 256 rows, and overflow them by one."""
import numpy as np
import pytest
import torch

import text_plan_ref as P

from clip_lora_match_amd import _capi as C

BS = (1, 2, 15, 16, 17, 255, 256, 257, 511, 512, 1000, 4095, 4096)
LS = (1, 2, 16, 77, 128, 256)


def _run_plan(ids, eos, B=None, L=None):
    """clm_text_plan on ids [B, L] into sentinel-filled arrays with PAD entries to spare ->
    (return code, lens, offs, rowmap, tiles, counts) as numpy"""
    b, l = ids.shape
    B, L = b if B is None else B, l if L is None else L
    dev = torch.from_numpy(ids).cuda()
    out = [torch.full((n + P.PAD,), P.SENTINEL, dtype=torch.int32, device="cuda")
           for n in (b, b + 1, b * l, b, 2)]
    rc = C.lib().clm_text_plan(0, C.ptr(dev), B, L, eos, *(C.ptr(t) for t in out), C.stream_of(dev.device))
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in out)


@pytest.mark.gpu
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("B", BS)
def test_text_plan_matches_reference(B, L):
    """every length pattern of text_plan_ref.captions at one (B, L): lens, offs, the written part of
    rowmap and tiles, and counts equal the reference; everything past them keeps the sentinel"""
    for pattern in P.PATTERNS:
        ids, eos = P.captions(pattern, B, L)
        lens, offs, rowmap, tiles, counts = P.reference(ids, eos)
        rc, g_lens, g_offs, g_rowmap, g_tiles, g_counts = _run_plan(ids, eos)
        what = (pattern, B, L)
        assert rc == C.CLM_OK, what
        assert (g_counts[:2] == counts).all(), (what, g_counts[:2], counts)
        assert (g_lens[:B] == lens).all(), what
        assert (g_offs[:B + 1] == offs).all(), what
        total, nt = counts
        assert (g_rowmap[:total] == rowmap).all(), what
        assert (g_tiles[:nt] == tiles).all(), (what, g_tiles[:nt][:8], tiles[:8])
        assert (g_rowmap[total:] == P.SENTINEL).all() and (g_tiles[nt:] == P.SENTINEL).all(), what
        for got, n in ((g_lens, B), (g_offs, B + 1), (g_counts, 2)):
            assert (got[n:] == P.SENTINEL).all(), what


@pytest.mark.gpu
def test_text_plan_refusals_write_nothing():
    """B = 4097, L = 0 and L = 257 are errors, B = 0 succeeds; none of them writes anything, and the
    next call works"""
    ids, eos = P.captions("random", 4097, 4)
    for B, L, ok in ((4097, 4, False), (8, 0, False), (8, 257, False), (-1, 4, False), (0, 4, True)):
        rc, *out = _run_plan(ids, eos, B=B, L=L)
        assert (rc == C.CLM_OK) == ok, (B, L, rc)
        assert all((a == P.SENTINEL).all() for a in out), (B, L)
    rc, g_lens, *_ = _run_plan(ids[:8], eos)
    assert rc == C.CLM_OK and (g_lens[:8] == P.reference(ids[:8], eos)[0]).all()


def test_reference_tile_count_within_the_varlen_grid():
    """Host only. gemm_attn_varlen sizes its grid for min(B, ceil(B L / (257 - L)) + 1) tiles
    (varlen_args in k_gemm_attn.hip, restated as text_plan_ref.tile_bound); a plan with more tiles than
    that would leave live rows unwritten. The reference's tile count stays within it on every pattern,
    and its tiles are what they claim: whole captions in order, <= 256 rows, none that could take the
    next caption as well."""
    for B in BS:
        for L in LS:
            for pattern in P.PATTERNS:
                ids, eos = P.captions(pattern, B, L)
                lens, offs, rowmap, tiles, counts = P.reference(ids, eos)
                assert counts[1] == len(tiles) <= P.tile_bound(B, L), (pattern, B, L, counts[1], P.tile_bound(B, L))
                first, n = tiles & 0xFFFF, tiles >> 16
                assert first[0] == 0 and (first[1:] == (first + n)[:-1]).all() and first[-1] + n[-1] == B
                rows = offs[first + n] - offs[first]
                assert (rows <= 256).all() and (rows[:-1] + lens[first[1:]] > 256).all()
                assert len(rowmap) == counts[0] == lens.sum()
    # the patterns reach what they are for: 256 captions in a tile, tiles of exactly 256 and of 255 rows
    _, offs, _, tiles, _ = P.reference(*P.captions("no_eos", 1000, 77))
    assert (tiles >> 16).max() == 256
    lens, offs, _, tiles, _ = P.reference(*P.captions("runs_256", 1000, 77))
    rows = offs[(tiles & 0xFFFF) + (tiles >> 16)] - offs[tiles & 0xFFFF]
    assert 256 in rows and 255 in rows and lens.max() == 77
