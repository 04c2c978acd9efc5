"""What the float64 anchor of the inference path (tests/infer_ref.py) measures, as profiles/infer_anchor/accuracy.txt.

  python tools/infer_anchor_report.py --measure measured.json     GPU box: every (stage, form, mode, case) of
                                                                  tests/test_gpu_infer_anchor.py once; e32, e_gpu and the bar per row
  python tools/infer_anchor_report.py measured.json [out.txt]     anywhere (CPU): the table, the worst ratio per quantity and mode, the
                                                                  constants the rule derives from them next to the committed ones,
                                                                  and per stage the finest weight image the committed bar rejects
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")          # as tests/conftest.py: the oracle's bits do not depend on the CPU vendor
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from puflow_amd._host import limit_host_threads  # noqa: E402

limit_host_threads()
import infer_ref as R  # noqa: E402

TEETH_CASES = ("s4_3x24", "s0_2x256")


def measure(path):
    import infer_anchor_gpu as G
    rows = []
    for case in R.GPU_CASES:
        for mode in G.MODES:
            for stage in G.GPU_STAGES:
                rows += G.measure(case, mode, stage)[0]
            rows += G.measure_e2e(case, mode)
            print(case, mode, len(rows), flush=True)
    for case, Rr in R.EXTRA_R.items():
        for stage in ("interp", "cg"):
            rows += G.measure(case, "f16n", stage, Rr)[0]
        rows += G.measure_e2e(case, "f16n", Rr)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    for r in rows:
        r.pop("bar")                                     # a function of the committed constants, not a measurement
    with open(path, "w") as f:
        json.dump(rows, f, indent=0)
    print("wrote", path, len(rows), "rows")


def group(r):
    """The constant a row is held by: (table, key)"""
    if r["stage"] == "e2e":
        return "RATIO_E2E", "cs" if r["q"].startswith("cs") else r["q"]
    pre = "ckpt:" if r["case"].startswith("ckpt") else ""
    if r["stage"].startswith("unit"):
        return "RATIO", pre + r["stage"]
    return "RATIO", pre + ("cs" if r["q"].startswith("cs") else r["q"])


def committed(table, key):
    if table == "RATIO_E2E":
        return R.RATIO_E2E[key]
    tab = R.RATIO_CKPT if key.startswith("ckpt:") else R.RATIO
    key = key.split(":")[-1]
    return tab["unit"][int(key[4:])] if key.startswith("unit") else tab[key]


def render(rows):
    out = ["Inference kernels against the float64 anchor (tests/infer_ref.py; tools/infer_anchor_report.py)", "",
           "e32   = max |fp32 oracle - float64| of the stage on the fp32-rounded anchor input (CPU)",
           "e_gpu = max |HIP kernel - float64| on the same input (MI355X); ldj and logp as relative errors",
           "e2e   = forward_stages against the whole float64 forward; e32 there is the fp32 oracle's end-to-end distance", "",
           "ratio = e_gpu / e32;  needed = max(e_gpu - floor, 0) / e32, the smallest constant the bar ratio * e32 + floor would pass with",
           "(floor = 2^-24 of the quantity's scale; the two differ only where e32 is below the floor: single numbers such as logp)", "",
           f"{'case':10s} {'mode':5s} {'R':>2s} {'stage':6s} {'q':4s} {'form':38s} {'e32':>10s} {'e_gpu':>10s} {'ratio':>7s} {'needed':>7s}"]
    worst = {}
    for r in rows:
        ratio = r["e_gpu"] / r["e32"]
        need = max(r["e_gpu"] - r["floor"], 0.0) / r["e32"]
        out.append(f"{r['case']:10s} {r['mode']:5s} {r['R']:2d} {r['stage']:6s} {r['q']:4s} {r['form']:38s} {r['e32']:10.3e} {r['e_gpu']:10.3e} {ratio:7.2f} {need:7.2f}")
        k = group(r)
        w = worst.setdefault(k, {})
        if need > w.get(r["mode"], (-1.0, ""))[0]:
            w[r["mode"]] = (need, f"{r['case']} {r['stage']} {r['q']}")
    out += ["", "Worst needed ratio per constant and EdgeConv arithmetic; derived = twice the worst over both, rounded up to a power of two.",
            "A committed RATIO_E2E below the derived value is capped by the parity tests' bar (tests/test_infer_ref.py,",
            "test_no_new_bar_admits_more_than_the_old_one); RATIO for the trained checkpoint's weights is scoped on its own (ckpt:).",
            f"{'table':10s} {'key':10s} {'f16n':>7s} {'f32':>7s} {'f16n/f32':>8s} {'derived':>8s} {'committed':>9s}   worst row"]
    for (table, key), w in worst.items():
        a, b = w.get("f16n", (0.0, ""))[0], w.get("f32", (0.0, ""))[0]
        top = max(w.values())
        d = R.constant_from(top[0])
        c = committed(table, key)
        flag = "" if c == d else ("   (capped)" if c < d and table == "RATIO_E2E" else "   <-- committed != derived")
        out.append(f"{table:10s} {key:10s} {a:7.2f} {b:7.2f} {a / b if b else float('nan'):8.2f} {d:8g} {c:9g}   {top[1]}{flag}")
    out += ["", "Finest weight image the committed stage bars reject: the fp32 oracle with the stage's matrix weights kept to n",
            "significant bits misses the bar for every n up to the figure (24 = fp32 itself; a dropped low fp16 half keeps 11)",
            f"{'stage':6s} " + " ".join(f"{c:>10s}" for c in TEETH_CASES)]
    for s in R.STAGES:
        if s in ("f", "g"):
            continue
        cells = []
        for c in TEETH_CASES:
            C = R.case(c)
            cells.append(R.finest_rejected_bits(s, C["sd"], C["S"][s], C["A"]["idx16"], C["R"]))
        out.append(f"{s:6s} " + " ".join(f"{v:10d}" for v in cells))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--measure":
        measure(sys.argv[2])
    else:
        src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "infer_anchor", "measured.json")
        dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, R.ACCURACY_FILE)
        with open(src) as f:
            text = render(json.load(f))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "w") as f:
            f.write(text)
        print(text)
