"""Plain-numpy references of the selection kernels under every exact search (k_search.hip): the order
key, topk_rows' (score desc, column asc) top-k, the k-th largest with multiplicity, the >= counters,
rescore_select's margin cut, and the np.longdouble cosine with the correctly-rounded criterion the exact
scores are held to. No GPU, no project code: tests/test_select_ref_host.py checks this file
against np.sort and torch.topk. tests/test_gpu_pass_error.py uses the rounding criterion; the selection
and re-score references wait for direct hooks to those kernels.
"""
import numpy as np


def float_key(v):
    """the documented order key on the fp32 bit pattern: bits ^ 0xFFFFFFFF for a set sign bit, bits |
    0x80000000 otherwise (uint32; ascending key = ascending value, -NaN < -inf, +inf < +NaN, -0 < +0)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where((u >> np.uint32(31)) == 1, u ^ np.uint32(0xFFFFFFFF), u | np.uint32(0x80000000)).astype(np.uint32)


def key_float(key):
    """the inverse of float_key"""
    k = np.ascontiguousarray(key, dtype=np.uint32)
    u = np.where((k >> np.uint32(31)) == 1, k & np.uint32(0x7FFFFFFF), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return u.view(np.float32)


def topk_rows_ref(scores, k, base=0):
    """scores [nq, C] f32 -> (out_s [nq, k] f32, out_i [nq, k] i64): per row the composites key << 32 |
    (0xFFFFFFFF - column) sorted descending; the first min(k, C) as (score bits, base + column), the rest
    (-inf, -1)"""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    nq, C = scores.shape
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    cols = np.arange(C, dtype=np.uint64)
    for q in range(nq):
        comp = (float_key(scores[q]).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - cols)
        order = np.sort(comp)[::-1][: min(k, C)]
        c = (np.uint64(0xFFFFFFFF) - (order & np.uint64(0xFFFFFFFF))).astype(np.int64)
        out_s[q, : c.size] = key_float((order >> np.uint64(32)).astype(np.uint32))
        out_i[q, : c.size] = base + c
    return out_s, out_i


def same_bits(a, b):
    """fp32 arrays equal bit for bit (a NaN equals only the same NaN, +0 differs from -0)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def kth_threshold_ref(values, k, margin):
    """values [nq, C] (fp32, or fp16 widened exactly) -> th [nq] f32: the k-th largest by the key order,
    duplicates counted, minus fp32(margin) in fp32"""
    v = np.ascontiguousarray(values, dtype=np.float32)
    key = np.sort(float_key(v), axis=1)[:, ::-1][:, k - 1]
    with np.errstate(invalid="ignore"):
        return (key_float(key) - np.float32(margin)).astype(np.float32)


def same_threshold(got, want):
    """thresholds equal bit for bit; where the reference is a NaN (a NaN k-th value, inf - inf) any NaN"""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan)) and same_bits(got[~nan], want[~nan])


def count_ge_ref(values, th):
    """cnt[q] = #{ j : values[q, j] >= th[q] } as IEEE comparisons of the values widened to fp32 (a NaN
    on either side is not counted, -0 >= +0)"""
    v = np.ascontiguousarray(values, dtype=np.float32)
    t = np.ascontiguousarray(th, dtype=np.float32)[:, None]
    with np.errstate(invalid="ignore"):
        return (v >= t).sum(axis=1).astype(np.int32)


def cos_longdouble(q, r):
    """cosines of paired rows q [m, dim], r [m, dim] (any float dtype, widened exactly) in np.longdouble;
    a zero-norm pair gives NaN"""
    q = np.asarray(q).astype(np.longdouble)
    r = np.asarray(r).astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (q * r).sum(axis=1) / (np.sqrt((q * q).sum(axis=1)) * np.sqrt((r * r).sum(axis=1)))


def ulp32(x):
    """the spacing of fp32 in the binade of |x| (float64 array; 2^-149 at and below the subnormals)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(a)
    return np.ldexp(1.0, np.where(a == 0, -149, np.maximum(e - 24, -149)))


def rounding_excess(got, ref):
    """|got - ref| - (ulp32(ref) / 2 + 2^-44) per element, ref in np.longdouble: <= 0 where the fp32 score
    is the correctly rounded cosine up to fp64 noise. A NaN must be a NaN: +inf where only one side is."""
    got = np.asarray(got, dtype=np.float32)
    ref = np.asarray(ref, dtype=np.longdouble)
    gn, rn = np.isnan(got), np.isnan(ref.astype(np.float64))
    with np.errstate(invalid="ignore"):
        ex = (np.abs(got.astype(np.longdouble) - ref)).astype(np.float64) - (ulp32(ref.astype(np.float64)) / 2 + 2.0 ** -44)
    ex = np.where(gn & rn, -np.inf, ex)
    return np.where(gn != rn, np.inf, ex)


def margin_cut_ref(cand_s, local, k, margin):
    """rescore_select's survivors of one query's list (cand_s [cnt] f32, local rows [cnt], distinct modulo
    2^32): the positions of the list sorted by (key of cand_s desc, local row asc), cut ahead of the first
    entry whose cand_s is < thr = fp32(sorted cand_s[k - 1]) - fp32(margin) when cnt >= k (a NaN thr cuts
    nothing), whole when cnt < k. Returns positions into the list, in sorted order."""
    cand_s = np.ascontiguousarray(cand_s, dtype=np.float32)
    local = np.asarray(local, dtype=np.int64)
    order = np.lexsort((local & 0xFFFFFFFF, -float_key(cand_s).astype(np.int64)))
    if cand_s.size < k:
        return order
    s = cand_s[order]
    with np.errstate(invalid="ignore"):
        thr = np.float32(s[k - 1]) - np.float32(margin)
        below = np.flatnonzero(s < thr)
    return order[: below[0]] if below.size else order
