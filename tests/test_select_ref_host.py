"""tests/select_ref.py against independent implementations, without a GPU: a reference that kernels are
held to must itself be right."""
import numpy as np
import pytest
import torch

import select_ref as SR


def _distinct(rng, nq, C):
    rows = []
    for _ in range(nq):
        v = np.unique(rng.standard_normal(C + C // 8 + 64).astype(np.float32))
        v = v[v != 0]   # keep one zero at the most: -0 and +0 compare equal but order by key
        assert v.size >= C
        rows.append(rng.permutation(v)[:C])
    return np.stack(rows)


def test_float_key_orders_as_the_values_do():
    rng = np.random.default_rng(1)
    v = np.concatenate([(rng.standard_normal(4000) * 10.0 ** rng.integers(-40, 38, 4000)).astype(np.float32),
                        np.array([0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, -3.4e38], np.float32)])
    v = np.unique(v)   # ascending, distinct (subnormals included)
    key = SR.float_key(v)
    assert np.all(key[1:] > key[:-1])
    assert SR.same_bits(SR.key_float(key), v)


def test_float_key_documented_corners():
    bits = np.array([0xFFFFFFFF, 0xFFC00000, 0xFF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x7F800000,
                     0x7F800001, 0x7FFFFFFF], np.uint32)
    key = SR.float_key(bits.view(np.float32))
    assert key[0] == 0 and key[-1] == 0xFFFFFFFF
    assert np.all(key[1:] > key[:-1])   # -NaN < -inf < -denormal < -0 < +0 < +denormal < +inf < +NaN
    assert SR.same_bits(SR.key_float(key), bits.view(np.float32))


@pytest.mark.parametrize("C,k", [(1, 1), (7, 3), (100, 100), (1000, 64), (5000, 1024), (50, 64)])
def test_topk_rows_ref_against_sort_and_torch(C, k):
    rng = np.random.default_rng(100 * C + k)
    sc = _distinct(rng, 3, C)
    base = (1 << 33) + 5
    got_s, got_i = SR.topk_rows_ref(sc, k, base)
    kk = min(k, C)
    want_s = np.sort(sc, axis=1)[:, ::-1][:, :kk]
    assert SR.same_bits(got_s[:, :kk], want_s)
    ts, ti = torch.topk(torch.from_numpy(sc), kk, dim=1, largest=True, sorted=True)
    assert SR.same_bits(got_s[:, :kk], ts.numpy())
    assert np.array_equal(got_i[:, :kk], ti.numpy() + base)
    assert np.all(np.isneginf(got_s[:, kk:])) and np.all(got_i[:, kk:] == -1)


def test_topk_rows_ref_ties_take_the_smallest_columns():
    sc = np.array([[1.0, 2.0, 2.0, 0.0, 2.0, -0.0, 1.0]], np.float32)
    s, i = SR.topk_rows_ref(sc, 6, 10)
    assert i.tolist() == [[11, 12, 14, 10, 16, 13]]
    assert SR.same_bits(s, np.array([[2, 2, 2, 1, 1, 0.0]], np.float32))


@pytest.mark.parametrize("k", [1, 3, 8])
def test_kth_threshold_ref_counts_duplicates(k):
    rng = np.random.default_rng(k)
    v = rng.integers(-4, 5, (5, 300)).astype(np.float32)   # heavy duplicates
    want = np.sort(v, axis=1)[:, ::-1][:, k - 1] - np.float32(0.25)
    assert SR.same_bits(SR.kth_threshold_ref(v, k, 0.25), want)
    assert SR.same_threshold(SR.kth_threshold_ref(v, k, 0.25), want)


def test_count_ge_ref_plain_loop():
    rng = np.random.default_rng(9)
    v = rng.integers(-3, 4, (4, 200)).astype(np.float32)
    v[1, 5] = np.nan
    th = np.array([0.0, 1.0, np.nan, -np.inf], np.float32)
    want = [sum(1 for x in row if x >= t) for row, t in zip(v.tolist(), th.tolist())]
    assert SR.count_ge_ref(v, th).tolist() == want
    assert want[2] == 0 and want[3] == 200


def test_margin_cut_ref():
    s = np.array([0.5, 0.9, 0.7, 0.7, 0.1, 0.6], np.float32)
    local = np.array([9, 8, 7, 3, 5, 4])
    # sorted: 0.9(8) 0.7(3) 0.7(7) 0.6(4) 0.5(9) 0.1(5); k = 2 -> thr = 0.7 - 0.15
    assert SR.margin_cut_ref(s, local, 2, 0.15).tolist() == [1, 3, 2, 5]
    assert SR.margin_cut_ref(s, local, 7, 0.15).tolist() == [1, 3, 2, 5, 0, 4]   # cnt < k: all
    thr = np.float32(0.7) - np.float32(0.15)
    s[0] = thr   # exactly at thr: kept
    assert SR.margin_cut_ref(s, local, 2, 0.15).tolist() == [1, 3, 2, 5, 0]
    s[0] = np.nextafter(thr, np.float32(-1))
    assert SR.margin_cut_ref(s, local, 2, 0.15).tolist() == [1, 3, 2, 5]


def test_rounding_excess_accepts_the_nearest_fp32_only():
    assert SR.ulp32(np.array([1.0, 0.75, -0.75, 1.5, 0.0, 1e-46])).tolist() == [2.0 ** -23, 2.0 ** -24, 2.0 ** -24,
                                                                            2.0 ** -23, 2.0 ** -149, 2.0 ** -149]
    rng = np.random.default_rng(4)
    q = rng.standard_normal((200, 33)).astype(np.float32)
    r = rng.standard_normal((200, 33)).astype(np.float32)
    ref = SR.cos_longdouble(q, r)
    want = (q.astype(np.float64) * r).sum(1) / np.sqrt((q.astype(np.float64) ** 2).sum(1) * (r.astype(np.float64) ** 2).sum(1))
    assert np.abs(ref.astype(np.float64) - want).max() < 1e-15
    near = ref.astype(np.float32)
    assert np.all(SR.rounding_excess(near, ref) <= 0)
    assert np.all(SR.rounding_excess(np.nextafter(near, np.float32(2)), ref) > 0)
    assert np.all(SR.rounding_excess(np.nextafter(near, np.float32(-2)), ref) > 0)
    nan, one = np.array([np.nan], np.float32), np.array([1.0], np.float32)
    ld = lambda a: a.astype(np.longdouble)
    assert SR.rounding_excess(nan, ld(nan))[0] <= 0
    assert SR.rounding_excess(nan, ld(one))[0] > 0 and SR.rounding_excess(one, ld(nan))[0] > 0
    assert np.isnan(SR.cos_longdouble(np.zeros((1, 4), np.float32), np.ones((1, 4), np.float32))[0])
