"""CPU-only: the nine exported workspace-size queries answer what tests/golden/workspace_bytes.json records.

Each layout is stated once in the library, walked with a null base by the size query and with the real base by the
run; the recorded sizes pin that statement at the edges of every layout: pieces that are absent or present (padded
copies, the bound path's scratch, the inlier masks, the fold buffers), the 256-byte rounding around row counts of 255
/ 256 / 257, widths that are padded, wide or refused, and the largest shapes.  `python -m tests.test_workspace_layout`
rewrites the fixture from the library as built; that is done before a change to a layout, never after it."""
import itertools
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")
PLAN_KNOBS = ("SPECTAVI_L1K2_", "SPECTAVI_CASCADE_", "SPECTAVI_ANN_")   # the plans read these

YROWS = (0, 1, 255, 256, 257)
# 16: the narrowest row; 40: padded to 48 / 64 where any width goes, refused by the 16-byte rule elsewhere; 128: the
# bound path's width; 144, 272: the next kernel up, the wide kernel; 2048: the widest; 2064: refused
DIMS = (16, 40, 48, 128, 144, 272, 2048, 2064)


def product(*axes):
    return [list(c) for c in itertools.product(*axes)]


CASES = {
    # xrows 31 / 32 at dim 128: the bound path's scratch absent / present
    "spv_l1k2_workspace_bytes": product((0, 1, 31, 32, 100, 70000, 1000000), YROWS + (5000, 1000000), DIMS),
    "spv_bruteforce_workspace_bytes": product((0, 1, 300, 100000), YROWS + (5000,), (1, 17) + DIMS, (1, 5, 64, 65)),
    # xrows <= ncand: every row is a candidate, 0 bytes
    "spv_ann_l2_workspace_bytes": product((0, 16, 17, 64, 65, 700, 131072), YROWS + (5000,), DIMS, (2, 4, 64), (0, 64)),
    "spv_cascade_workspace_bytes": [c + mng for c in product((0, 1, 2000, 100000), YROWS + (700,), DIMS)
                                    for mng in ([4, 1, 2], [4, 3, 0], [22, 1, 2], [22, 3, 16], [31, 1, 2], [31, 3, 2],
                                                [8, 2, 2], [24, 1, 2])],
    "spv_sift_workspace_bytes": [[1, 1], [2, 2], [97, 64], [64, 97], [640, 480], [8192, 8192], [8193, 8192], [0, 5]],
    "spv_normalize_workspace_bytes": [[d] for d in (0, 1, 20, 128, 129, 2048)],
    "spv_normalize_workspace_bytes_rows": product((0, 1, 65535, 65536, 1000000), (1, 20, 128, 129, 2048)) + [[-1, 20], [5, 0]],
    "spv_ratio_test_workspace_bytes": [[y] for y in (-1, 0, 1, 255, 256, 257, 5000, 16128, 16129, 1500000)],
    "spv_dlt_score_workspace_bytes": product((-1, 0, 1, 4, 120, 65535), (0, 1, 200, 100000, 1 << 33)),
    "spv_ransac_workspace_bytes": product((-1, 0, 1, 30, 16383), (0, 1, 200, 100000), (0, 1)),
}


def answers(name):
    from spectavi_amd._lib import clib
    fn = getattr(clib, name)
    return [args + [int(fn(*args))] for args in CASES[name]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_size_query_answers_the_recorded_sizes(name):
    knobs = sorted(k for k in os.environ if k.startswith(PLAN_KNOBS))
    if knobs:
        pytest.skip("the plans read %s" % ", ".join(knobs))
    with open(FIXTURE) as f:
        recorded = json.load(f)[name]
    assert [r[:-1] for r in recorded] == CASES[name], "the fixture records other cases than this module lists"
    got = answers(name)
    wrong = [(r[:-1], r[-1], g[-1]) for r, g in zip(recorded, got) if r != g]
    assert not wrong, "%d of %d sizes differ (args, recorded, now): %s" % (len(wrong), len(got), wrong[:8])
    assert any(r[-1] > 0 for r in recorded)


if __name__ == "__main__":
    assert not [k for k in os.environ if k.startswith(PLAN_KNOBS)]
    with open(FIXTURE, "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join('"%s": [\n%s\n]' % (n, ",\n".join(json.dumps(r) for r in answers(n)))
                                           for n in sorted(CASES)))
    print("wrote %s: %d sizes" % (FIXTURE, sum(len(c) for c in CASES.values())))
