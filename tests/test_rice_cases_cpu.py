"""The Rice boundary table (tests/ricecases.py) held on the CPU: its restatement of rice.c:30-139 against the oracle and
the reference (live where it is built, and the answers recorded in tests/golden/ref_rice_cases.npz), every case's prop
against its own PCM, three wrong restatements caught, every (site, family) pair and every parameter 0 .. 30 present."""
import operator
import os

import numpy as np
import pytest

import oraclelib
import ricecases as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_rice_cases.npz")
MODE_CODE = {0: 1, 1: 8, 2: 9, 3: 10}            # encode.c:636-641 as the records carry it


@pytest.fixture(scope="module")
def recs(oracle):
    return R.records(oracle)


@pytest.fixture(scope="module")
def restated(recs):
    """{case name: calc_rice's answer on the oracle's residual}"""
    out = {}
    for c, p, info, res in recs:
        lpc, pmin, pmax, order, bps, prec = R.rice_call(p, info)
        out[c.name] = R.calc_rice(res, order, pmin, pmax, lpc, bps, prec)
    return out


def answer(r):
    return (r["bits"], r["method"], r["porder"], r["params"])


def test_construction_holds(recs):
    """every frame ends as the predicted subframe: all-zero coefficient rows, shift 0, no wasted bits, the residual
    behind the warm-up equal to the sample, the order the configuration names"""
    for c, p, info, res in recs:
        assert int(info["type"]) == (8 if c.cfg.fixed else 32), (c.name, info["type"])
        assert info["wasted"] == 0 and info["shift"] == 0 and not info["coefs"].any(), c.name
        order = int(info["order"])
        assert (res[order:] == c.samples()[order:]).all(), c.name
        if c.cfg.search is None:
            assert order == c.cfg.order, (c.name, order)
        else:
            assert order <= c.cfg.maxorder and not c.samples()[:c.cfg.maxorder].any(), c.name


def test_restatement_equals_oracle(oracle, recs, restated):
    for c, p, info, res in recs:
        lpc, pmin, pmax, order, bps, prec = R.rice_call(p, info)
        bits, sf = oracle.subframe_bits(res, pmin, pmax, order, bps, prec, lpc)
        got = (int(bits) & R.M32, int(sf["rice_method"]), int(sf["porder"]), [int(v) for v in sf["rparams"][:1 << int(sf["porder"])]])
        assert answer(restated[c.name]) == got, c.name
        # ... and the record the whole encode left
        assert got == (int(info["est_bits"]), int(info["rice_method"]), int(info["porder"]),
                       [int(v) for v in info["rparams"][:1 << int(info["porder"])]]), c.name


def test_restatement_equals_reference(recs, restated):
    """tests/golden/ref_rice_cases.npz: what the compiled rice.c answered to every case (results only); where the
    reference is built here, its live answers are the recorded ones"""
    gold = R.unpack_answers(np.load(GOLDEN))
    assert sorted(gold) == sorted(restated)
    for name, r in restated.items():
        assert answer(r) == gold[name], name
    if oraclelib.Ref.available():
        ref = oraclelib.Ref()
        for c, p, info, res in recs:
            lpc, pmin, pmax, order, bps, prec = R.rice_call(p, info)
            bits, meth, por, par = ref.calc_rice_params(lpc, pmin, pmax, res, order, bps, prec)
            assert (int(bits), meth, por, [int(v) for v in par[:1 << por]]) == gold[c.name], c.name


def test_props(recs, restated):
    """the named sum sits where the case says; the named wave crosses its limit and no other does"""
    for c, p, info, res in recs:
        r, order = restated[c.name], int(info["order"])
        for nd in c.prop.get("nodes", ()):
            lv, j = nd["level"], nd["node"]
            u = R.fold_array(res)
            u[:order] = 0
            ln = len(res) >> lv
            assert int(u[j * ln:(j + 1) * ln].sum()) == nd["sum"], (c.name, nd)
            if lv in r["sums"]:
                assert r["sums"][lv][j] == nd["sum"], (c.name, nd)
            assert j > 0 or c.cfg.search is None, (c.name, nd)          # a search chooses the order: no target in partition 0
            assert (len(res) >> lv) - (order if j == 0 else 0) == nd["cnt"], (c.name, nd)
        if "below" in c.prop:
            b = c.prop["below"]
            sums = R.level_sums(res, order, b["level"], b["level"])
            assert max(sums[b["level"]]) < b["limit"] // 8, c.name
        if "threads" in c.prop:
            t = c.prop["threads"]
            run, big = R.thread_runs(res, order, c.cfg.C, c.cfg.T)
            per_wave = (big if t["kind"] == "umax" else run).max(axis=1)
            assert int(per_wave[t["wave"]]) == t["value"], (c.name, t)
            crossed = [w for w in range(len(per_wave)) if int(per_wave[w]) >= t["limit"]]
            assert crossed == ([t["wave"]] if t["crosses"] else []), (c.name, crossed)
            if t["kind"] == "umax":
                assert int(run.max()) < 1 << 32, c.name          # only the one switch is in play
        if "first" in c.prop:
            assert (len(res) >> r["pmax"]) - order == c.prop["first"], c.name
        if "tie" in c.prop:
            lo, hi = c.prop["tie"]["levels"]
            assert r["level_bits"][lo] == r["level_bits"][hi] == min(r["level_bits"].values()) and r["porder"] == hi > lo, c.name


def test_f3_rice2_in_and_beside_the_chosen_level(restated):
    """RICE2 because of one partition of the chosen level; a parameter above 14 in a level that is not chosen"""
    inside = beside = 0
    for c in R.cases():
        if c.family != "F3":
            continue
        r = restated[c.name]
        if r["method"] == 1 and sum(k > 14 for k in r["params"]) == 1:
            inside += 1
        if r["method"] == 0 and any(r["level_method"].values()):
            beside += 1
    assert inside > 0 and beside > 0, (inside, beside)


def test_closed_form_equals_scan_at_every_node(recs, restated):
    pairs = set()
    for c, p, info, res in recs:
        r, order = restated[c.name], int(info["order"])
        for lv, sums in r["sums"].items():
            pairs.update((s, (len(res) >> lv) - (order if j == 0 else 0)) for j, s in enumerate(sums))
    assert len(pairs) > 5000
    for s, cnt in pairs:
        assert R.closed_k(s, cnt) == R.scan_k(s, cnt), (s, cnt)


@pytest.mark.parametrize("family,kw", [
    ("F2", dict(find_k=lambda s, n: R.scan_k(s, n, operator.le))),          # <= for < in the scan
    ("F2", dict(find_k=lambda s, n: R.closed_k(s, n, correction=False))),   # the k++ correction left out
    ("F7", dict(le=operator.lt)),                                           # < for <= between levels
], ids=["scan-le", "no-correction", "levels-lt"])
def test_wrong_restatements_are_caught(recs, restated, family, kw):
    caught = total = 0
    for c, p, info, res in recs:
        if c.family != family:
            continue
        lpc, pmin, pmax, order, bps, prec = R.rice_call(p, info)
        total += 1
        caught += answer(R.calc_rice(res, order, pmin, pmax, lpc, bps, prec, **kw)) != answer(restated[c.name])
        if family == "F2" and caught >= 20:
            break
    assert caught > 0 and (family != "F7" or caught == total), (family, caught, total)


def test_coverage(restated):
    have = {(c.site, c.family) for c in R.cases()}
    fams = ("F1", "F2", "F3", "F4", "F5a", "F5b", "F6", "F7")
    for site in ("S1", "S2", "S3", "S4", "S7"):
        for f in fams:
            assert ((site, f) in have) != ((site, f) in R.EXCLUDED), (site, f)
    assert all(isinstance(v, str) and v for v in R.EXCLUDED.values())
    assert {c.cfg.launch for c in R.cases()} >= {cfg.launch for cfg in R.site_configs()}      # every instance has cases
    ks, methods = set(), set()
    for r in restated.values():
        ks.update(r["params"])
        methods.add(r["method"])
    assert ks == set(range(31)) and methods == {0, 1}, (sorted(ks), methods)
    # per site: the parameters its spacing lets through
    for site, top in (("S1", 27), ("S2", 26), ("S3", 30), ("S4", 26)):
        seen = set()
        for c in R.cases():
            if c.site == site:
                seen.update(restated[c.name]["params"])
        assert seen >= set(range(top + 1)), (site, sorted(set(range(top + 1)) - seen))


def test_stereo_estimate(oracle):
    """F8: the restated encode.c:598-643 against the oracle; the left sum where the case says; a parameter one too
    high, or the missing correction, changes some case's decision"""
    cases = R.stereo_cases()
    assert {(c.n, c.bps) for c in cases} == {(256, 16), (256, 32), (4096, 16), (4096, 32)}
    off_by_one = no_corr = 0
    tags = set()
    for c in cases:
        left, right = c.left.astype(np.int32), c.right.astype(np.int32)
        assert np.abs(c.left).max() < 1 << (c.bps - 1) and np.abs(c.right).max() < 1 << (c.bps - 1), c.name
        sums = R.stereo_sums(left, right)
        assert sums[0] == c.prop["left_sum"], c.name
        mode = R.stereo_mode(left, right)
        assert oracle.stereo_mode(left, right) == MODE_CODE[mode], c.name
        off_by_one += R.stereo_mode(left, right, find_k=lambda s, n: min(R.scan_k(s, n) + 1, 30)) != mode
        no_corr += R.stereo_mode(left, right, find_k=lambda s, n: R.closed_k(s, n, correction=False)) != mode
        tags.add(c.prop["tag"])
    assert off_by_one > 0 and no_corr > 0
    assert {"zero", "half-", "half", "half+", "k0at", "k1c+", "k8lo", "k20hi", "two32+0", "two32-2", "two32+2"} <= tags
