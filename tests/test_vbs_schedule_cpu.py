"""The schedule of a variable-block-size batch (flake_amd/csrc/vbs_schedule.h): which bins share an order-search / K3
launch, the order the launches are issued in, and the lane (0 = the handle's stream, 1.. = its internal ones) each
goes to.  fhip_last_launches shows kernels, not streams, so nothing else observes the lanes.  Runs without a GPU: a
host program includes the header (hipcc --cuda-host-only) and prints the schedule of each case.

The merge keys and the expected schedules were recorded from the code BEFORE the schedule was a function of its own
(fhip_encode_blocks_vbs_dev instrumented to print key, unit, weight, issue turn and lane, run on an MI355X) for
bench.py's two VBS presets: level 10 (vector searches; bins 3, 5, 7 group at 1024 blocks) and level 12 (matrix
searches; no bin's geometry groups), at 1024 and at 8192 blocks (above FHIP_VBS_MERGE_MAX: no groups), fanned out
over three lanes and serial (profiling).  Level 11 gives one key alone, which forms no group; 1- and 8-channel
level-10 batches gave level 10's keys."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flake_amd import build as fb  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")

NONE = [-1] * 8
L10_1024 = [-1, -1, -1, 256, -1, 256, -1, 256]
L11_1024 = [-1, -1, -1, 256, -1, -1, -1, -1]

# units in issue order: (member bins, weight, lane)
GROUPED = [([1], 39, 0), ([2], 38, 1), ([0], 35, 2), ([3, 5, 7], 15, 2), ([6], 14, 1), ([4], 11, 0)]
VEC = [([1], 39, 0), ([2], 38, 1), ([0], 35, 2), ([6], 14, 2), ([3], 11, 1), ([4], 11, 0), ([5], 8, 1), ([7], 8, 2)]
MAT = [([0], 55, 0), ([1], 53, 1), ([2], 49, 2), ([3], 34, 2), ([4], 27, 1), ([5], 27, 0), ([6], 23, 1), ([7], 23, 0)]


def serial(units):
    return [(m, w, 0) for m, w, _ in units]


# name: (merge keys, matrix-search weights, fan out, lanes, expected units)
CASES = {
    "level 10, 1024 blocks, fan": (L10_1024, False, True, 3, GROUPED),
    "level 10, 1024 blocks, serial": (L10_1024, False, False, 3, serial(GROUPED)),
    "level 10, 8192 blocks, fan": (NONE, False, True, 3, VEC),
    "level 10, 8192 blocks, serial": (NONE, False, False, 3, serial(VEC)),
    "level 12, 1024 blocks, fan": (NONE, True, True, 3, MAT),
    "level 12, 1024 blocks, serial": (NONE, True, False, 3, serial(MAT)),
    "level 12, 8192 blocks, fan": (NONE, True, True, 3, MAT),
    "level 12, 8192 blocks, serial": (NONE, True, False, 3, serial(MAT)),
    "no bin groups (all -1), fan": (NONE, False, True, 3, VEC),
    "level 11, 1024 blocks: one key alone, fan": (L11_1024, False, True, 3, VEC),
}
# the path per bin (no LPC: prediction_type 1) takes the bins from the longest, by the same lane rule: level 10's
# parameters with the fixed predictors, three lanes
PER_BIN_LANES = {7: 0, 6: 1, 5: 2, 4: 0, 3: 2, 2: 1, 1: 0, 0: 2}


@pytest.fixture(scope="module")
def schedules(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vbs_schedule")
    body = []
    for name, (key, mat, fan, lanes, _) in CASES.items():
        body.append(
            "    {\n"
            f"        const int key[8] = {{{', '.join(map(str, key))}}};\n"
            f"        const VbsSchedule s = vbs_schedule(key, {str(mat).lower()}, {str(fan).lower()}, {lanes});\n"
            f'        std::printf("case %s\\n", "{name}");\n'
            "        for (int t = 0; t < s.nunits; t++) {\n"
            '            std::printf("unit %d %d", s.unit[t].weight, s.unit[t].lane);\n'
            '            for (int j = 0; j < s.unit[t].nbins; j++) std::printf(" %d", s.unit[t].bins[j]);\n'
            '            std::printf("\\n");\n'
            "        }\n"
            '        std::printf("lane_of");\n'
            '        for (int k = 0; k < 8; k++) std::printf(" %d", s.lane_of[k]);\n'
            '        std::printf("\\n");\n'
            "    }\n")
    src = tmp / "sched.hip"
    src.write_text(
        '#include <cstdio>\n#include "vbs_schedule.h"\nusing namespace fhip;\n'
        "int main() {\n" + "".join(body) +
        "    long long queued[VBS_MAX_LANES] = {0};\n"
        '    std::printf("per_bin");\n'
        '    for (int k = 7; k >= 0; k--) std::printf(" %d", vbs_take_lane(queued, 3, vbs_bin_weights(false)[k]));\n'
        '    std::printf("\\n");\n'
        "    return 0;\n}\n")
    exe = tmp / "sched"
    subprocess.run([fb.HIPCC, "-std=c++17", "-O1", "--cuda-host-only", "-I", os.path.join(fb.PKG, "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got, cur = {}, None
    for line in out.splitlines():
        head, _, rest = line.partition(" ")
        if head == "case":
            cur = got.setdefault(rest, {"units": []})
        elif head == "unit":
            w, lane, *bins = map(int, rest.split())
            cur["units"].append((bins, w, lane))
        elif head == "lane_of":
            cur["lane_of"] = list(map(int, rest.split()))
        elif head == "per_bin":
            got["per_bin"] = list(map(int, rest.split()))
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_schedule_is_the_recorded_one(schedules, name):
    units = CASES[name][4]
    got = schedules[name]
    assert got["units"] == units, name
    lane_of = [None] * 8
    for bins, _, lane in units:
        for k in bins:
            lane_of[k] = lane
    assert got["lane_of"] == lane_of, name


def test_every_bin_is_scheduled_once(schedules):
    for name in CASES:
        bins = sorted(k for m, _, _ in schedules[name]["units"] for k in m)
        assert bins == list(range(8)), name


def test_per_bin_path_takes_the_recorded_lanes(schedules):
    assert schedules["per_bin"] == [PER_BIN_LANES[k] for k in range(7, -1, -1)]


def test_header_needs_nothing_from_hip():
    text = open(os.path.join(fb.PKG, "csrc", "vbs_schedule.h")).read()
    assert "#include" not in text
