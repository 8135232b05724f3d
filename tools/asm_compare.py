#!/usr/bin/env python3
"""Compare the device code of two builds, kernel by kernel (CPU only; nothing is run).

    python tools/asm_compare.py PARENT_BUILD NEW_BUILD [--show N]

Each argument is the build/ directory that `make -C gpu-wah_amd asm` leaves: the resource figures of
-Rpass-analysis=kernel-resource-usage (resource_usage_<source>.txt) and the device assembly (wah_<source>-hip-amdgcn-*.s).
The usual use: the parent commit built in a scratch copy against the tree, before a refactor is believed to have left the
kernels alone.

Per kernel: VGPR / AGPR / SGPR / scratch / LDS / occupancy and the instruction count, parent -> new, and where the
mnemonic sequences differ -- the instruction lines between the kernel's label and the end of its function, operands and
register numbers left out, compared with difflib -- with the net change of every mnemonic's count.  --show N lists the
first N differing stretches of a kernel.

A kernel that is missing from its own source in the new build is paired by name with the one other source that gained it: a move
between files is compared like any other kernel, under its new source.

Exit status 1 if a kernel appears or disappears, gains scratch, changes its LDS or loses occupancy, or if a kernel's resource
record is missing from either build."""
import argparse
import collections
import difflib
import glob
import os
import re
import subprocess
import sys

FIELDS = (("VGPR", "VGPRs"), ("AGPR", "AGPRs"), ("SGPR", "TotalSGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
          ("LDS", "LDS Size [bytes/block]"), ("occupancy", "Occupancy [waves/SIMD]"))
REMARK = re.compile(r"remark: [^ ]+ +(Function Name|[A-Za-z][A-Za-z \[\]/]*?): (\S+) \[-Rpass-analysis")


def read_resources(path):
    """{mangled name: {remark field: int}} of one resource_usage_<source>.txt"""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = REMARK.search(line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None and m.group(2).lstrip("-").isdigit():
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def read_kernels(path):
    """{mangled name: [mnemonic, ...]} of the kernels (.amdhsa_kernel) of one assembly file"""
    text = open(path, errors="replace").read().split("\n")
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(text), re.M))
    out, name = {}, None
    for line in text:
        s = line.strip()
        if name is None:
            if s.endswith(":") or ": " in s:
                label = s.split(":", 1)[0]
                if label in kernels and label not in out:
                    name = label
                    out[name] = []
            continue
        if s.startswith(".Lfunc_end"):
            name = None
            continue
        s = s.split(";", 1)[0].strip()
        if not s or s[0] in ".#" or s.endswith(":"):
            continue
        out[name].append(s.split()[0])
    return out


def read_build(directory):
    """{source: {mangled name: (resources, mnemonics)}}"""
    build = {}
    for asm in sorted(glob.glob(os.path.join(directory, "*-hip-amdgcn-*.s"))):
        source = os.path.basename(asm).split("-hip-")[0]
        res_path = os.path.join(directory, "resource_usage_%s.txt" % source.replace("wah_", "", 1))
        res = read_resources(res_path) if os.path.exists(res_path) else {}
        build[source] = {k: (res.get(k, {}), seq) for k, seq in read_kernels(asm).items()}
    return build


def pair_moved(old, new):
    """A kernel that the new build lacks in its parent's source and has, under the same name, in exactly one other source that the
    parent lacks it in has moved: the parent's record goes under the new source, so that the two are compared.  {name: old source}"""
    moved = {}
    for source, ko in list(old.items()):
        for k in [k for k in ko if k not in new.get(source, {})]:
            homes = [s for s, kn in new.items() if k in kn and k not in old.get(s, {})]
            if len(homes) == 1:
                moved[k] = source
                old.setdefault(homes[0], {})[k] = ko.pop(k)
    return moved


def demangle(names):
    for tool in ("llvm-cxxfilt", "c++filt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        try:
            got = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        except (OSError, subprocess.CalledProcessError):
            continue
        if len(got) >= len(names):
            short = [re.sub(r"\(.*$", "", g.replace("wah::(anonymous namespace)::", "").replace("void ", "")) for g in got]
            return dict(zip(names, short))
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="list the first N differing stretches of every kernel that differs")
    args = ap.parse_args()
    old, new = read_build(args.parent), read_build(args.new)
    if not old or not new:
        sys.exit("no device assembly in %s" % (args.parent if not old else args.new))
    moved = pair_moved(old, new)
    failures = []
    for source in sorted(set(old) | set(new)):
        ko, kn = old.get(source, {}), new.get(source, {})
        names = demangle(sorted(set(ko) | set(kn)))
        same = differ = 0
        print("%s" % source)
        for k in sorted(names, key=names.get):
            if k not in ko or k not in kn:
                failures.append("%s: only in the %s build" % (names[k], "new" if k in kn else "parent's"))
                print("  %s\n    ONLY IN THE %s BUILD" % (names[k], "NEW" if k in kn else "PARENT'S"))
                continue
            (ro, so), (rn, sn) = ko[k], kn[k]
            for which, r in (("parent's", ro), ("new", rn)):
                lost = [short for short, field in FIELDS if field not in r]
                if lost:
                    failures.append("%s: no %s in the %s build's resource record" % (names[k], " / ".join(lost), which))
            figures = "  ".join("%s %s->%s" % (short, ro.get(field, "?"), rn.get(field, "?")) for short, field in FIELDS)
            print("  %s%s\n    %s  instructions %d->%d" % (names[k], " (the parent's: %s)" % moved[k] if k in moved else "", figures, len(so), len(sn)))
            get = lambda r, field: r.get(dict(FIELDS)[field], 0)
            if get(rn, "scratch") > get(ro, "scratch"):
                failures.append("%s: scratch %d -> %d" % (names[k], get(ro, "scratch"), get(rn, "scratch")))
            if get(rn, "LDS") != get(ro, "LDS"):
                failures.append("%s: LDS %d -> %d" % (names[k], get(ro, "LDS"), get(rn, "LDS")))
            if get(rn, "occupancy") < get(ro, "occupancy"):
                failures.append("%s: occupancy %d -> %d" % (names[k], get(ro, "occupancy"), get(rn, "occupancy")))
            if so == sn:
                same += 1
                print("    identical mnemonic sequence")
                continue
            differ += 1
            ops = [o for o in difflib.SequenceMatcher(None, so, sn, autojunk=False).get_opcodes() if o[0] != "equal"]
            gone, come = sum(o[2] - o[1] for o in ops), sum(o[4] - o[3] for o in ops)
            print("    differs in %d places, instructions %d..%d: %d instructions became %d" % (len(ops), ops[0][1], ops[-1][2], gone, come))
            net = collections.Counter(sn)
            net.subtract(collections.Counter(so))
            print("    net change by mnemonic: %s" % (" ".join("%+d %s" % (n, m) for m, n in sorted(net.items()) if n) or "none (the same instructions in another order)"))
            for tag, i1, i2, j1, j2 in ops[: args.show]:
                print("      at %d: [%s] -> [%s]" % (i1, " ".join(so[i1:i2]), " ".join(sn[j1:j2])))
        print("  %d kernels identical, %d differ" % (same, differ))
    for f in failures:
        print("FAIL " + f)
    print("%d conditions broken (a kernel appears or disappears, gains scratch, changes its LDS, loses occupancy, has no resource record)" % len(failures))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
