"""Rank1Merge::plan() (csrc/host_eig_merge.hpp) without Qf -- what the device merge runs -- against plan() with Qf, the
first half of the host merge's build(): the column map and the rotation list must reproduce Qf bit for bit."""
import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

from device_merge_cases import KS, cases


def _replay(p, K, k1):
    """Qf from Q1 | Q2 by the column map, then the rotations in list order, in the host's arithmetic"""
    k2 = K - k1
    Qf = np.zeros((K, K))
    for c, cs in enumerate(p["colsrc"]):
        if cs >= 0:
            Qf[:k1, c] = p["Q1"][:, cs]
        else:
            Qf[k1:, c] = p["Q2"][:, -(cs + 1)]
    assert k2 == p["Q2"].shape[0]
    for pj, j, c, s in p["rots"]:
        x, y = Qf[:, pj].copy(), Qf[:, j].copy()
        Qf[:, pj] = c * x + s * y
        Qf[:, j] = c * y - s * x
    return Qf


@pytest.mark.parametrize("K", KS)
def test_plan_without_qf_replays_to_the_host_merges_qf_bit_for_bit(K):
    rotated = 0
    for name, D, f, al, be, k1 in cases(K):
        full = B.host_merge_plan(D, f, al, be, k1, with_qf=True)
        lean = B.host_merge_plan(D, f, al, be, k1, with_qf=False)
        assert lean["Qf"] is None
        for key in ("d", "z", "nd", "colsrc", "Q1", "Q2"):
            assert np.array_equal(full[key], lean[key]), (name, key)
        assert full["rots"] == lean["rots"] and full["deflated"] == lean["deflated"], name
        assert len(lean["nd"]) + lean["deflated"] == K, name
        assert np.array_equal(_replay(lean, K, k1), full["Qf"]), name
        rotated += len(lean["rots"])
        if name == "decoupled":
            assert len(lean["nd"]) == 0
        # the host merge built on the planner still returns what it did: same split between the two kinds of pole
        _, _, info = B.host_symeig_split(D, f, al, be, k1)
        assert info["nondeflated"] == len(lean["nd"]) and info["deflated"] == lean["deflated"], name
    if K >= 25:
        assert rotated > 0, "the cases must exercise a deflation rotation (the repeated Ritz value)"


def test_k2_equal_to_one():
    """K = 5 split at k1 = 4: the tail is a single entry"""
    name, D, f, al, be, _ = cases(5)[0]
    full = B.host_merge_plan(D, f, al, be, 4, with_qf=True)
    lean = B.host_merge_plan(D, f, al, be, 4, with_qf=False)
    assert lean["Q2"].shape == (1, 1)
    assert np.array_equal(_replay(lean, 5, 4), full["Qf"])
