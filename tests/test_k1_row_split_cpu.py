"""K1's producer row split (kernels.h: wt_split; k1_autocorr.hip: wt_split_of) without a GPU.

The headline's instance, k_autocorr_wt<3, false, 8> in both forms, stages its 32 rows in a split of its own.
Its register budget must not grow past what it was with 8/8/8/8 (170 VGPRs in the long form, 166 in the 128 form),
with no scratch and no vector spills: hipcc cross-compiles k1_autocorr.hip with
-Rpass-analysis=kernel-resource-usage, as tests/test_k1_residency_cpu.py does.  The row constants are checked by
a small host program compiled here against kernels.h: they sum to 32, are even, and their prefix sums cover every
row exactly once; the same checks reject splits that are odd, short or overlapping."""
import os
import re
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flake_amd import build as fb  # noqa: E402

# instance -> VGPRs of the parent (8/8/8/8)
VGPR_BUDGET = {"k_autocorr_wtl<3, false, 8>": 170, "k_autocorr_wt<3, false, 8>": 166}

pytestmark = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def resources():
    cmd = [fb.HIPCC, *[x for x in fb.HIP_FLAGS if x != "-shared"], "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(fb.PKG, "csrc"), "--cuda-device-only", "-c",
           os.path.join(fb.PKG, "csrc", "k1_autocorr.hip"), "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=1800).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: +([A-Za-z][^:]*?): +(-?\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    out = {}
    for mangled, res in kernels.items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout
        for inst in VGPR_BUDGET:
            if inst + "(" in name:
                out[inst] = res
    missing = set(VGPR_BUDGET) - set(out)
    assert not missing, f"{sorted(missing)} not found among {len(kernels)} kernels:\n{err[-2000:]}"
    return out


@pytest.mark.parametrize("inst", sorted(VGPR_BUDGET))
def test_headline_instance_keeps_its_registers(resources, inst):
    r = resources[inst]
    print(inst, r)
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["VGPRs Spill"] == 0, r
    assert r["VGPRs"] <= VGPR_BUDGET[inst], r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 256 and r["Occupancy [waves/SIMD]"] >= 2, r


HOST_CHECK = r"""
#include "kernels.h"
#include <cstdio>
using namespace fhip;
constexpr int sum_of(const wt_split &s) { return s.rows[0] + s.rows[1] + s.rows[2] + s.rows[3]; }
constexpr bool all_even(const wt_split &s)
{
    for (int p = 0; p < 4; p++) if (s.rows[p] & 1) return false;
    return true;
}
// every row 0 .. WT_SUB - 1 staged by exactly one producer, rows of producer p from its prefix sum on
constexpr bool covers_once(const wt_split &s)
{
    int seen[WT_SUB] = {};
    for (int p = 0; p < 4; p++)
        for (int r = 0; r < s.rows[p]; r++) {
            const int q = wt_split_first(s, p) + r;
            if (q < 0 || q >= WT_SUB) return false;
            seen[q]++;
        }
    for (int q = 0; q < WT_SUB; q++) if (seen[q] != 1) return false;
    return true;
}
static_assert(WT_SUB == 32, "rows per workgroup");
static_assert(sum_of(WT_SPLIT_O8) == 32 && all_even(WT_SPLIT_O8) && covers_once(WT_SPLIT_O8), "the headline's split");
static_assert(sum_of(WT_SPLIT_EVEN) == 32 && all_even(WT_SPLIT_EVEN) && covers_once(WT_SPLIT_EVEN), "8/8/8/8");
static_assert(wt_split_valid(WT_SPLIT_O8) && wt_split_valid(WT_SPLIT_EVEN), "the kernel's own check");
static_assert(wt_split_first(WT_SPLIT_O8, 0) == 0 && wt_split_first(WT_SPLIT_O8, 4) == 32, "prefix sums");
// the kernel's check refuses what would not stage every row once, or would split a channel pair
static_assert(!wt_split_valid(wt_split{{7, 11, 7, 7}}), "odd counts");
static_assert(!wt_split_valid(wt_split{{8, 8, 8, 6}}), "short");
static_assert(!wt_split_valid(wt_split{{8, 8, 8, 10}}), "long");
static_assert(!wt_split_valid(wt_split{{0, 16, 8, 8}}), "an idle producer");
static_assert(!covers_once(wt_split{{8, 8, 8, 10}}) && !covers_once(wt_split{{8, 8, 8, 6}}), "coverage");
static_assert(wt_split_valid(wt_split{{6, 12, 6, 8}}) && covers_once(wt_split{{6, 12, 6, 8}}), "an uneven split");
static_assert(wt_split_first_with(wt_split{{6, 12, 6, 8}}, 0) && !wt_split_first_with(wt_split{{6, 12, 6, 8}}, 2), "");
int main()
{
    std::printf("O8 %d %d %d %d\n", WT_SPLIT_O8.rows[0], WT_SPLIT_O8.rows[1], WT_SPLIT_O8.rows[2], WT_SPLIT_O8.rows[3]);
    std::printf("FIRST %d %d %d %d\n", wt_split_first(WT_SPLIT_O8, 0), wt_split_first(WT_SPLIT_O8, 1),
                wt_split_first(WT_SPLIT_O8, 2), wt_split_first(WT_SPLIT_O8, 3));
    return 0;
}
"""


def test_row_constants_cover_every_row_once(tmp_path):
    src = tmp_path / "row_split_check.hip"
    src.write_text(textwrap.dedent(HOST_CHECK))
    exe = tmp_path / "row_split_check"
    c = subprocess.run([fb.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(fb.PKG, "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [int(x) for x in re.search(r"O8 (\d+) (\d+) (\d+) (\d+)", r.stdout).groups()]
    first = [int(x) for x in re.search(r"FIRST (\d+) (\d+) (\d+) (\d+)", r.stdout).groups()]
    assert sum(rows) == 32 and all(x > 0 and x % 2 == 0 for x in rows), rows
    assert first == [sum(rows[:p]) for p in range(4)], (rows, first)
    staged = [q for p in range(4) for q in range(first[p], first[p] + rows[p])]
    assert staged == list(range(32)), staged
