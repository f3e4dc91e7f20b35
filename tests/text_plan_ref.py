"""A plain numpy reference of the varlen text plan (text_plan, k_ops.hip) and the caption batches its
tests are run on (tests/test_gpu_text_plan.py, tests/test_gpu_fused_attention.py)."""
import numpy as np

EOS = 49407          # CLIP's <|endoftext|>; the other tokens of a caption are drawn below it
SENTINEL = -7
PAD = 8              # sentinel entries past the end of every output array
PATTERNS = ("no_eos", "eos_last", "eos_first", "several_eos", "random", "runs_256", "argmax_twice", "argmax_equal")


def reference(ids, eos):
    """(lens [B], offs [B + 1], rowmap [total], tiles [number of tiles], counts [2]) of ids [B, L]:
    lens = pooled row + 1, the pooled row being the first position equal to eos (0 if there is none),
    or for eos == 2 the first largest id; offs the exclusive prefix sums; rowmap[offs[b] + p] = b L + p;
    tiles greedy whole captions in order, <= 256 rows each, first | count << 16."""
    ids = np.asarray(ids)
    B, L = ids.shape
    if eos == 2:
        prow = ids.argmax(1)
    else:
        hit = ids == eos
        prow = np.where(hit.any(1), hit.argmax(1), 0)
    lens = prow.astype(np.int64) + 1
    offs = np.concatenate([[0], np.cumsum(lens)])
    total = int(offs[B])
    rowmap = np.arange(total) - np.repeat(offs[:-1], lens) + np.repeat(np.arange(B) * L, lens)
    tiles, first, rows = [], 0, 0
    for b in range(B):
        if rows + lens[b] > 256:
            tiles.append(first | (b - first) << 16)
            first, rows = b, 0
        rows += int(lens[b])
    if B:
        tiles.append(first | (B - first) << 16)
    return lens, offs, rowmap, np.array(tiles, dtype=np.int64), np.array([total, len(tiles)])


def tile_bound(B, L):
    """the tiles gemm_attn_varlen's grid covers (varlen_args, k_gemm_attn.hip): text_plan closes a tile
    only when the next caption does not fit, so every tile but the last holds more than 256 - L rows"""
    return min(B, (B * L + (256 - L)) // (257 - L) + 1)


def _fill(total, L):
    """lengths in [1, L] that sum to `total`: as many L as fit, then the rest"""
    return [L] * (total // L) + ([total % L] if total % L else [])


def runs_256(B, L):
    """lens [B]: runs of captions that sum to exactly 256 (the tile closes full: <= against <), to 255
    followed by a caption of 2 rows (which must open the next tile), and to 257 (the last caption of the
    run must), repeated"""
    unit = _fill(256, L) + _fill(255, L) + [min(2, L)] + _fill(257, L)
    return np.array((unit * (B // len(unit) + 1))[:B], dtype=np.int64)


def ids_from_lens(lens, L, rng, eos=EOS):
    """ids [B, L] int32 whose first eos sits at lens[b] - 1, random other tokens"""
    lens = np.asarray(lens)
    ids = rng.integers(3, eos, (len(lens), L)).astype(np.int32)
    ids[np.arange(len(lens)), lens - 1] = eos
    return ids


def captions(pattern, B, L, seed=0):
    """(ids [B, L] int32, eos) of one length pattern"""
    rng = np.random.default_rng([PATTERNS.index(pattern), B, L, seed])
    if pattern == "no_eos":                     # every caption one live row: 256 captions per tile
        return rng.integers(3, EOS, (B, L)).astype(np.int32), EOS
    if pattern == "eos_last":
        return ids_from_lens(np.full(B, L), L, rng), EOS
    if pattern == "eos_first":
        return ids_from_lens(np.full(B, 1), L, rng), EOS
    if pattern == "several_eos":                # the first of them wins
        first = rng.integers(0, L, B)
        ids = ids_from_lens(first + 1, L, rng)
        later = rng.integers(0, L, (B, 3))
        for j in range(3):
            p = np.maximum(later[:, j], first)
            ids[np.arange(B), p] = EOS
        if L > 1:
            ids[0, :] = EOS                     # and a caption of nothing else
        return ids, EOS
    if pattern == "random":
        return ids_from_lens(rng.integers(1, L + 1, B), L, rng), EOS
    if pattern == "runs_256":
        return ids_from_lens(runs_256(B, L), L, rng), EOS
    if pattern == "argmax_twice":               # eos == 2: the first largest id, which occurs twice
        ids = rng.integers(0, 1000, (B, L)).astype(np.int32)
        a, b = rng.integers(0, L, B), rng.integers(0, L, B)
        ids[np.arange(B), a] = 5000
        ids[np.arange(B), b] = 5000
        return ids, 2
    assert pattern == "argmax_equal"            # eos == 2, all ids equal: row 0
    return np.full((B, L), 2, dtype=np.int32), 2
