"""Compare bench.py --full JSON files: every other_configs row and the small batches of a branch run
against a parent run and a recorded file.  python3 tools/cmp_full.py <recorded.json> <parent.json> <branch.json>"""
import json, sys
def load(p):
    return json.loads(open(p).read().strip().splitlines()[-1])
ref, par, br = (load(p) for p in sys.argv[1:4])
print(f"headline ms/step: r05 {ref['ms_per_step']}  parent {par['ms_per_step']}  branch {br['ms_per_step']}")
def rows(d):
    out = {r["workload"]: r["ms_per_step"] for r in d["other_configs"]}
    sb = d.get("small_batch_ms") or {}
    if isinstance(sb, dict):
        for k, v in sb.items():
            out[f"small_batch {k}"] = v if not isinstance(v, dict) else v.get("ms_per_step", v)
    elif isinstance(sb, list):
        for r in sb:
            out[f"small_batch {r.get('frames', r)}"] = r.get("ms_per_step")
    return out
R, P, B = rows(ref), rows(par), rows(br)
for k in R:
    b = B.get(k); p = P.get(k); r = R[k]
    try:
        print(f"{k[:70]:70s} r05 {r:8.4f} parent {p:8.4f} branch {b:8.4f}  vs r05 {100 * (b / r - 1):+6.2f} %  vs parent {100 * (b / p - 1):+6.2f} %")
    except Exception:
        print(k, r, p, b)
