"""The copy of the selecting epilogues' tile cost model that tests/test_gpu_gemm_select.py keeps
(G2_MODEL / _g2_pick, used for the slab layout of config -1 and for the picks its docstring states)
against the table the library compiles, read from k_gemm.hip. No device needed."""
import os
import re

from test_gpu_gemm_select import G2_MODEL, _g2_pick

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clip-lora-match_amd", "csrc")


def test_g2_model_is_the_librarys():
    src = open(os.path.join(CSRC, "k_gemm.hip")).read()
    body = re.search(r"constexpr CfgModel MODELS_G2\[\] = \{(.*?)\};", src, re.S).group(1)
    rows = re.findall(r"\{(\d+), (\d+), (\d+), (\d+), ([0-9.]+)\}", body)
    assert len(rows) == 4 and all(r[3] == "1" for r in rows)   # _g2_pick assumes one workgroup per CU
    assert {int(r[0]): (int(r[1]), int(r[2]), float(r[4])) for r in rows} == G2_MODEL
    # pick_from: 256 slots per round, a later model wins only by more than 0.1 %
    assert "256LL * c.wg_per_cu" in src and "cost < best_cost * 0.999" in src


def test_heuristic_picks():
    """the picks the GPU file's docstring states"""
    for nq in (1, 5, 64, 300):
        for N in (1, 31, 255, 700, 3000, 4097, 9000):
            assert _g2_pick(nq, N) == 9
    assert _g2_pick(1300, 1000) == 9
    assert _g2_pick(512, 10_000_000) == 8
    assert _g2_pick(300, 70_001) == 11 and _g2_pick(300, 40_999) == 11
    assert _g2_pick(70, 70_000) == 11 and _g2_pick(128, 300_000) == 11
