#!/usr/bin/env python3
"""Check A: compare kernels of two source trees (resources + instruction streams) for the default, bwdf32, gradf32 and f16 builds.
python tools/cmp_isa.py PARENT_ROOT BRANCH_ROOT [--dump DIR] [--removed REGEX] [--renamed REGEX REPL]
(two checkouts; build container, no GPU)
  --removed REGEX        kernel names that may exist at the parent only (a deleted kernel or template copy)
  --renamed REGEX REPL   re.sub(REGEX, REPL, name) on the parent's kernel names before the two sides are matched

A source is compiled when its own text differs between the trees or ANY header under csrc/ or include/ does (a header edit
changes every kernel that includes it).  Verdict per kernel copy:
  identical   same resource record, same instruction stream
  reordered   same resource record, same instruction count, same multiset of (mnemonic, operand count): the streams differ by
              register names and the order of independent instructions only
  ISA DIFFERS anything else
Exit status 0 only when every kernel is identical or reordered, none appeared or disappeared (--removed apart) and none uses
scratch that did not at the parent."""
import argparse, collections, concurrent.futures, filecmp, hashlib, importlib.util, os, re, subprocess, sys, tempfile

# variant -> (defines, the sources build.py recompiles for it: None = all, a str = that attribute of build.py)
VARIANTS = {"default": ([], None),
            "bwdf32": (["PF_EC_BWDG_F32", "PF_EC_DW_F32"], ("train_fused.hip",)),
            "gradf32": (["PF_EC_BWDG_F32", "PF_EC_DW_F32", "PF_EC_FWD_F32"], ("train_fused.hip", "train_ec_fwd.hip")),
            "f16": (["PF_MMN_TERMS=1"], "F16_SOURCES")}


def load_build(root):
    spec = importlib.util.spec_from_file_location("b_" + hashlib.md5(root.encode()).hexdigest(), os.path.join(root, "puflow_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def compile_s(B, path, defines, out):
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + B.FLAGS + B.EXTRA_FLAGS.get(os.path.basename(path), []) + [f"-D{d}" for d in defines] +
                          ["-S", "--cuda-device-only", "-o", out, path], stderr=subprocess.DEVNULL)
    return out


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


RES_KEYS = ("NumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def parse(asm_path):
    text = open(asm_path).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    dm = demangle(kernels)
    res = {}
    for k in kernels:
        m = re.search(r"^" + re.escape(k) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=^\s*\.(?:section(?!\s+\.AMDGPU\.csdata)|text|protected|globl)\b)", text, re.S | re.M)
        assert m, k
        body, tail = m.group(1), m.group(2)
        body = body[:body.rindex("s_endpgm") + len("s_endpgm")]
        lines = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line:
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            line = re.sub(r"\s+", " ", line)
            lines.append(line)
        r = {}
        for key in RES_KEYS:
            mm = re.search(r";\s*" + key + r":\s*(\d+)", tail)
            r[key] = int(mm.group(1)) if mm else None
        res.setdefault(dm[k].replace("(anonymous namespace)::", ""), []).append((os.path.basename(asm_path), r, lines))
    return res


def headers(root):
    hs = {}
    for d in ("puflow_amd/csrc", "include"):
        for f in sorted(os.listdir(os.path.join(root, d))):
            if f.endswith(".h"):
                hs[d + "/" + f] = open(os.path.join(root, d, f), "rb").read()
    return hs


def histogram(lines):
    """multiset of (mnemonic, operand count); labels count as themselves"""
    c = collections.Counter()
    for line in lines:
        op, _, rest = line.partition(" ")
        c[(op, len(rest.split(",")) if rest else 0)] += 1
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--dump")
    ap.add_argument("--removed")
    ap.add_argument("--renamed", nargs=2, metavar=("REGEX", "REPL"))
    args = ap.parse_args()
    parent, branch, dump = args.parent, args.branch, args.dump
    trees = {"parent": parent, "branch": branch}
    Bs = {k: load_build(v) for k, v in trees.items()}
    hp, hb = headers(parent), headers(branch)
    hdr_diff = sorted(h for h in set(hp) | set(hb) if hp.get(h) != hb.get(h))
    print("headers that differ:", hdr_diff or "none")
    files = {}
    for k, root in trees.items():
        other = trees["branch" if k == "parent" else "parent"]
        fs = []
        for s in Bs[k].SOURCES:
            a, b = os.path.join(root, "puflow_amd/csrc", s), os.path.join(other, "puflow_amd/csrc", s)
            if hdr_diff or not os.path.exists(b) or not filecmp.cmp(a, b, shallow=False):
                fs.append(s)
        files[k] = fs
    print("sources that differ:", files)
    tmp = tempfile.mkdtemp(prefix="cmpisa_")
    jobs = {}

    def vfiles(k, v):
        only = VARIANTS[v][1]
        only = getattr(Bs[k], only) if isinstance(only, str) else only
        return [s for s in files[k] if only is None or s in only]

    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        for k, root in trees.items():
            for v, (defs, _) in VARIANTS.items():
                for s in vfiles(k, v):
                    out = os.path.join(tmp, f"{k}_{v}_{s}.s")
                    jobs[(k, v, s)] = ex.submit(compile_s, Bs[k], os.path.join(root, "puflow_amd/csrc", s), defs, out)
        for j in jobs.values():
            j.result()
    ok, totals = True, [0, 0, 0]
    for v in VARIANTS:
        side = {}
        for k in trees:
            allk = {}
            for s in vfiles(k, v):
                for name, lst in parse(jobs[(k, v, s)].result()).items():
                    allk.setdefault(name, []).extend([(s,) + x[1:] for x in lst])
            if k == "parent" and args.renamed:
                allk = {re.sub(args.renamed[0], args.renamed[1], name): lst for name, lst in allk.items()}
            side[k] = allk
        P, Bk = side["parent"], side["branch"]
        print(f"\n== {v}: parent {sum(map(len, P.values()))} kernels ({len(P)} names), branch {sum(map(len, Bk.values()))} kernels ({len(Bk)} names)")
        only_p, only_b = sorted(set(P) - set(Bk)), sorted(set(Bk) - set(P))
        print("   only in parent:", only_p or "none")
        print("   only in branch:", only_b or "none")
        if only_b or [n for n in only_p if not (args.removed and re.search(args.removed, n))]:
            ok = False
        nsame, reordered, differs = 0, [], []
        for name in sorted(set(P) & set(Bk)):
            ps, pr, pl = P[name][0]
            for bs, br, bl in Bk[name]:
                if br["ScratchSize"] and not pr["ScratchSize"]:
                    print("   NEW SCRATCH", name, br); ok = False
                if pr != br:
                    print(f"   RESOURCES DIFFER {name}\n      parent {ps}: {pr}\n      branch {bs}: {br}")
                if pr == br and pl == bl:
                    nsame += 1
                    continue
                nline = sum(x != y for x, y in zip(pl, bl)) + abs(len(pl) - len(bl))
                what = f"{name} ({ps}: {len(pl)} instr, {bs}: {len(bl)} instr, {nline} lines differ)"
                if pr == br and len(pl) == len(bl) and histogram(pl) == histogram(bl):
                    reordered.append(what)
                else:
                    differs.append(what); ok = False
                if dump:
                    os.makedirs(dump, exist_ok=True)
                    h = hashlib.md5(name.encode()).hexdigest()[:8]
                    open(os.path.join(dump, f"{v}_{h}_parent.s"), "w").write(name + "\n" + "\n".join(pl) + "\n")
                    open(os.path.join(dump, f"{v}_{h}_branch.s"), "w").write(name + "\n" + "\n".join(bl) + "\n")
        print(f"   identical (registers, scratch, LDS, occupancy, instruction stream): {nsame} kernel copies; "
              f"total instructions compared {sum(len(x[2]) for l in Bk.values() for x in l)}")
        print(f"   reordered (same resources, instruction count and (mnemonic, operand count) multiset): {len(reordered)} kernel copies")
        for w in reordered:
            print("      REORDERED", w)
        print(f"   ISA DIFFERS: {len(differs)} kernel copies")
        for w in differs:
            print("      ISA DIFFERS", w)
        totals[0] += nsame; totals[1] += len(reordered); totals[2] += len(differs)
    print(f"\nTOTAL: identical {totals[0]}, reordered {totals[1]}, ISA differs {totals[2]}")
    print("RESULT:", "DIFFERENCES" if not ok else "ALL IDENTICAL" if not totals[1] else "IDENTICAL OR REORDERED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
