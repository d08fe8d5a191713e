"""The registers, scratch, LDS and occupancy of every stretch kernel instance, against the figures of the commit before pass A / pass B of the fixed,
linked and reset families were folded into one template <LOG2N, SCHED, LINK, RESET> (hipcc -O3 --offload-arch=gfx950,
-Rpass-analysis=kernel-resource-usage, tests/resource_usage.py).

TABLE holds two columns per instance.  The first is that parent commit's build, in the order of resource_usage.FIELDS (its pv_stretch_pass_*<L, S> are
(L, S, 0, 0) here, pv_link_pass_*<L, S> are (L, S, 1, 0), pv_reset_pass_*<L, LINK> are (L, 1, LINK, 1)): no instance may use scratch, spill a VGPR, use
AGPRs or exceed 256 VGPRs, and LDS size and occupancy must equal the parent's.  The second column is (TotalSGPRs, VGPRs, SGPRs Spill) of the present
source, pinned exactly; where it differs from the parent's the row says `moved`.  The scans and the onset kernel were not touched by the fold: their
second column must equal the first."""
import os

import pytest

import resource_usage as RU

# ("a" | "b", log2n, SCHED, LINK, RESET) | ("scan", which) | ("onset", log2n): (parent: FIELDS, now: (TotalSGPRs, VGPRs, SGPRs Spill))
TABLE = {
    ('a', 8, 0, 0, 0): ((66, 80, 0, 0, 6, 0, 0, 0), (66, 80, 0)),
    ('a', 8, 0, 1, 0): ((86, 80, 0, 0, 6, 0, 0, 0), (86, 80, 0)),
    ('a', 8, 1, 0, 0): ((70, 76, 0, 0, 6, 0, 0, 0), (70, 76, 0)),
    ('a', 8, 1, 0, 1): ((72, 78, 0, 0, 6, 0, 0, 0), (72, 78, 0)),
    ('a', 8, 1, 1, 0): ((90, 76, 0, 0, 6, 0, 0, 0), (90, 76, 0)),
    ('a', 8, 1, 1, 1): ((88, 78, 0, 0, 6, 0, 0, 0), (88, 78, 0)),
    ('a', 9, 0, 0, 0): ((74, 80, 0, 0, 6, 0, 0, 0), (74, 80, 0)),
    ('a', 9, 0, 1, 0): ((96, 80, 0, 0, 6, 0, 0, 0), (96, 80, 0)),
    ('a', 9, 1, 0, 0): ((78, 76, 0, 0, 6, 0, 0, 0), (78, 76, 0)),
    ('a', 9, 1, 0, 1): ((82, 78, 0, 0, 6, 0, 0, 0), (82, 78, 0)),
    ('a', 9, 1, 1, 0): ((98, 76, 0, 0, 6, 0, 0, 0), (98, 76, 0)),
    ('a', 9, 1, 1, 1): ((96, 78, 0, 0, 6, 0, 0, 0), (96, 78, 0)),
    ('a', 10, 0, 0, 0): ((84, 82, 0, 0, 5, 0, 0, 0), (84, 82, 0)),
    ('a', 10, 0, 1, 0): ((98, 78, 0, 0, 6, 0, 0, 0), (98, 78, 0)),
    ('a', 10, 1, 0, 0): ((76, 84, 0, 0, 5, 0, 0, 0), (76, 84, 0)),
    ('a', 10, 1, 0, 1): ((80, 84, 0, 0, 5, 0, 0, 0), (80, 84, 0)),
    ('a', 10, 1, 1, 0): ((96, 78, 0, 0, 6, 0, 0, 0), (96, 78, 0)),
    ('a', 10, 1, 1, 1): ((100, 80, 0, 0, 6, 0, 0, 0), (100, 80, 0)),
    ('a', 11, 0, 0, 0): ((74, 86, 0, 0, 5, 0, 0, 0), (74, 86, 0)),
    ('a', 11, 0, 1, 0): ((86, 86, 0, 0, 5, 0, 0, 0), (86, 86, 0)),
    ('a', 11, 1, 0, 0): ((70, 86, 0, 0, 5, 0, 0, 0), (70, 86, 0)),
    ('a', 11, 1, 0, 1): ((74, 86, 0, 0, 5, 0, 0, 0), (74, 86, 0)),
    ('a', 11, 1, 1, 0): ((88, 84, 0, 0, 5, 0, 0, 0), (88, 84, 0)),
    ('a', 11, 1, 1, 1): ((86, 86, 0, 0, 5, 0, 0, 0), (86, 86, 0)),
    ('a', 12, 0, 0, 0): ((70, 86, 0, 0, 5, 0, 0, 0), (70, 86, 0)),
    ('a', 12, 0, 1, 0): ((82, 86, 0, 0, 5, 0, 0, 0), (82, 86, 0)),
    ('a', 12, 1, 0, 0): ((66, 86, 0, 0, 5, 0, 0, 0), (66, 86, 0)),
    ('a', 12, 1, 0, 1): ((70, 86, 0, 0, 5, 0, 0, 0), (70, 86, 0)),
    ('a', 12, 1, 1, 0): ((84, 84, 0, 0, 5, 0, 0, 0), (84, 84, 0)),
    ('a', 12, 1, 1, 1): ((84, 84, 0, 0, 5, 0, 0, 0), (84, 84, 0)),
    ('a', 13, 0, 0, 0): ((70, 86, 0, 0, 5, 0, 0, 0), (70, 86, 0)),
    ('a', 13, 0, 1, 0): ((82, 86, 0, 0, 5, 0, 0, 0), (82, 86, 0)),
    ('a', 13, 1, 0, 0): ((66, 86, 0, 0, 5, 0, 0, 0), (66, 86, 0)),
    ('a', 13, 1, 0, 1): ((70, 86, 0, 0, 5, 0, 0, 0), (70, 86, 0)),
    ('a', 13, 1, 1, 0): ((84, 84, 0, 0, 5, 0, 0, 0), (84, 84, 0)),
    ('a', 13, 1, 1, 1): ((84, 84, 0, 0, 5, 0, 0, 0), (84, 84, 0)),
    ('b', 8, 0, 0, 0): ((101, 100, 0, 0, 4, 0, 0, 0), (101, 100, 0)),
    ('b', 8, 0, 1, 0): ((106, 105, 0, 0, 4, 11, 0, 0), (106, 105, 11)),
    ('b', 8, 1, 0, 0): ((106, 96, 0, 0, 5, 0, 0, 0), (106, 96, 0)),
    ('b', 8, 1, 0, 1): ((106, 98, 0, 0, 4, 0, 0, 0), (106, 98, 0)),
    ('b', 8, 1, 1, 0): ((106, 99, 0, 0, 4, 19, 0, 0), (106, 99, 19)),
    ('b', 8, 1, 1, 1): ((106, 99, 0, 0, 4, 18, 0, 0), (106, 99, 18)),
    ('b', 9, 0, 0, 0): ((102, 102, 0, 0, 4, 0, 0, 0), (102, 102, 0)),
    ('b', 9, 0, 1, 0): ((106, 107, 0, 0, 4, 6, 0, 0), (106, 107, 6)),
    ('b', 9, 1, 0, 0): ((106, 99, 0, 0, 4, 2, 0, 0), (106, 99, 2)),
    ('b', 9, 1, 0, 1): ((106, 101, 0, 0, 4, 2, 0, 0), (106, 101, 2)),
    ('b', 9, 1, 1, 0): ((106, 100, 0, 0, 4, 8, 0, 0), (106, 100, 8)),
    ('b', 9, 1, 1, 1): ((106, 101, 0, 0, 4, 9, 0, 0), (106, 101, 9)),
    ('b', 10, 0, 0, 0): ((106, 107, 0, 0, 4, 2, 0, 0), (106, 107, 2)),
    ('b', 10, 0, 1, 0): ((106, 113, 0, 0, 4, 18, 0, 0), (106, 113, 18)),
    ('b', 10, 1, 0, 0): ((106, 107, 0, 0, 4, 2, 0, 0), (106, 107, 2)),
    ('b', 10, 1, 0, 1): ((106, 106, 0, 0, 4, 0, 0, 0), (106, 106, 0)),
    ('b', 10, 1, 1, 0): ((106, 109, 0, 0, 4, 18, 0, 0), (106, 109, 18)),
    ('b', 10, 1, 1, 1): ((106, 109, 0, 0, 4, 20, 0, 0), (106, 109, 20)),
    ('b', 11, 0, 0, 0): ((106, 121, 0, 0, 4, 2, 0, 0), (106, 121, 2)),
    ('b', 11, 0, 1, 0): ((106, 121, 0, 0, 4, 25, 0, 0), (106, 121, 25)),
    ('b', 11, 1, 0, 0): ((106, 115, 0, 0, 4, 2, 0, 0), (106, 115, 2)),
    ('b', 11, 1, 0, 1): ((106, 115, 0, 0, 4, 2, 0, 0), (106, 115, 2)),
    ('b', 11, 1, 1, 0): ((106, 119, 0, 0, 4, 23, 0, 0), (106, 119, 23)),
    ('b', 11, 1, 1, 1): ((106, 121, 0, 0, 4, 25, 0, 0), (106, 119, 25)),        # moved
    ('b', 12, 0, 0, 0): ((106, 145, 0, 0, 3, 13, 0, 0), (106, 145, 13)),
    ('b', 12, 0, 1, 0): ((106, 145, 0, 0, 3, 28, 0, 0), (106, 145, 28)),
    ('b', 12, 1, 0, 0): ((106, 140, 0, 0, 3, 2, 0, 0), (106, 140, 2)),
    ('b', 12, 1, 0, 1): ((106, 140, 0, 0, 3, 11, 0, 0), (106, 140, 2)),        # moved
    ('b', 12, 1, 1, 0): ((106, 140, 0, 0, 3, 26, 0, 0), (106, 140, 26)),
    ('b', 12, 1, 1, 1): ((106, 141, 0, 0, 3, 28, 0, 0), (106, 140, 28)),        # moved
    ('b', 13, 0, 0, 0): ((106, 247, 0, 0, 2, 20, 0, 0), (106, 247, 20)),
    ('b', 13, 0, 1, 0): ((106, 243, 0, 0, 2, 34, 0, 0), (106, 243, 34)),
    ('b', 13, 1, 0, 0): ((106, 243, 0, 0, 2, 16, 0, 0), (106, 243, 16)),
    ('b', 13, 1, 0, 1): ((106, 243, 0, 0, 2, 15, 0, 0), (106, 243, 18)),        # moved
    ('b', 13, 1, 1, 0): ((106, 239, 0, 0, 2, 33, 0, 0), (106, 239, 33)),
    ('b', 13, 1, 1, 1): ((106, 245, 0, 0, 2, 37, 0, 0), (106, 239, 35)),        # moved
    ('onset', 8): ((96, 48, 0, 0, 8, 0, 0, 1056), (96, 48, 0)),
    ('onset', 9): ((94, 48, 0, 0, 8, 0, 0, 1056), (94, 48, 0)),
    ('onset', 10): ((87, 56, 0, 0, 8, 0, 0, 1056), (87, 56, 0)),
    ('onset', 11): ((76, 60, 0, 0, 8, 0, 0, 1056), (76, 60, 0)),
    ('onset', 12): ((72, 60, 0, 0, 8, 0, 0, 1056), (72, 60, 0)),
    ('onset', 13): ((88, 62, 0, 0, 8, 0, 0, 1056), (88, 62, 0)),
    ('scan', 'reset'): ((37, 24, 0, 0, 8, 0, 0, 0), (37, 24, 0)),
    ('scan', 'stretch'): ((33, 17, 0, 0, 8, 0, 0, 0), (33, 17, 0)),
}
PINNED = [RU.FIELDS.index(f) for f in ("TotalSGPRs", "VGPRs", "SGPRs Spill")]
FLAGS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)]          # the (SCHED, LINK, RESET) the launcher uses


def test_the_table_holds_the_80_instances():
    passes = {(ab, L) + f for ab in "ab" for L in range(8, 14) for f in FLAGS}
    assert set(TABLE) == passes | {("scan", "stretch"), ("scan", "reset")} | {("onset", L) for L in range(8, 14)} and len(TABLE) == 80
    for k, (parent, now) in TABLE.items():
        if len(k) != 5:
            assert tuple(parent[i] for i in PINNED) == now, k


def _check(source, keys):
    got = {}
    for name, v in RU.resources(source).items():
        k = RU.stretch_key(name)
        assert k is not None and k not in got, name
        got[k] = v
    assert set(got) == set(keys), sorted(set(got) ^ set(keys), key=str)
    for k, v in got.items():
        parent, now = TABLE[k]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 256, (k, v)
        assert v["LDS Size"] == parent[RU.FIELDS.index("LDS Size")] and v["Occupancy"] == parent[RU.FIELDS.index("Occupancy")], (k, v, parent)
        assert (v["TotalSGPRs"], v["VGPRs"], v["SGPRs Spill"]) == now, (k, v, now)


@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_pass_and_scan_instances_keep_their_resources():
    """6 sizes x (pass A, pass B) x the six flag combinations, and the two scans: exactly these 74 kernels."""
    _check("stretch/pv_stretch_kernels.hip", [k for k in TABLE if k[0] != "onset"])


@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_onset_instances_keep_their_resources():
    _check("stretch/pv_onset_kernels.hip", [k for k in TABLE if k[0] == "onset"])
