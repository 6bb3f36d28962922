#!/usr/bin/env python3
"""Do two source trees compile to the same kernels?  Host only: cross-compiles, needs no device.

    python tools/code_object_compare.py PARENT_TREE NEW_TREE --parent-units bvh_build \\
        --units bvh_build,bvh_fold,bvh_partition,bvh_subtrees,bvh_finish \\
        --config product= --config "lab=-DNBODY_LAB" [--only nbody::] [--jobs 4]

Every unit (csrc/<unit>.hip) of both trees is compiled for the device alone with the flags of its tree's Makefile, the
configuration's flags, -Rpass-analysis=kernel-resource-usage and -S.  Per kernel, by demangled name, two things are compared
for equality: the resource remarks (registers, scratch, LDS, occupancy: every field the compiler reports), and the
instruction sequence between the kernel's label and the end of the function, with comments and directives dropped and
local labels renumbered in order of appearance.  Whole sequences are compared; nothing is searched for.

    python tools/code_object_compare.py --objects A.o B.o [A2.o B2.o ...]

compares built objects pairwise instead: the device code object inside each is disassembled and the kernels' sequences
compared in the same way (no resource remarks there).

Prints one line per kernel and configuration; exit status 0 iff the name sets are equal and no kernel differs.
"""
import argparse
import concurrent.futures
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

CSRC = os.path.join("nbody-simulation_amd", "csrc")


def hipcc(tree):
    """the compiler the tree's Makefile names (or $HIPCC)"""
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)


def tool(tree, *names):
    """an LLVM / binutils tool: beside the clang behind the tree's hipcc, else on PATH"""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc(tree))))
    for name in names:
        for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin")):
            if os.path.exists(os.path.join(d, name)):
                return os.path.join(d, name)
        if shutil.which(name):
            return shutil.which(name)
    sys.exit("none of %s found" % (names,))


HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # the tree this script is in
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]*[0-9]+(?:_[0-9]+)?")


def makefile_flags(tree):
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return ["--offload-arch=" + arch] + shlex.split(flags)


def demangle(tree, names):
    if not names:
        return {}
    out = subprocess.run([tool(tree, "llvm-cxxfilt", "c++filt")], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return dict(zip(names, out.stdout.split("\n")))


def renumber(lines):
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), "L%d" % len(seen))

    return [LOCAL_LABEL.sub(sub, ln) for ln in lines]


def kernels_of_asm(asm):
    """{mangled name: [instruction lines]} of every kernel in a device assembly listing"""
    lines = asm.split("\n")
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", lines[i])
        if not (m and m.group(1) in names):
            i += 1
            continue
        body = []
        i += 1
        while i < len(lines) and not re.match(r"^\.Lfunc_end[0-9]+:", lines[i]):
            ln = lines[i].split(";", 1)[0].split("//", 1)[0].strip()
            i += 1
            if not ln:
                continue
            if ln.startswith(".") and not LOCAL_LABEL.match(ln.rstrip(":")):  # a directive
                continue
            body.append(" ".join(ln.split()))
        out[m.group(1)] = renumber(body)
    return out


def resources_of_remarks(err):
    """{mangled name: {field: value}} from -Rpass-analysis=kernel-resource-usage"""
    out, cur = {}, None
    for ln in err.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([^:]+):\s*(\S+)\s*\[-Rpass-analysis", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def compile_unit(tree, unit, extra):
    src = os.path.join(tree, CSRC, unit + ".hip")
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, unit + ".s")
        cmd = [hipcc(tree)] + makefile_flags(tree) + extra + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", src, "-o", s]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.join(tree, CSRC))
        if r.returncode != 0:
            sys.exit("compiling %s failed:\n%s" % (src, r.stderr[-4000:]))
        asm = open(s).read()
    return unit, kernels_of_asm(asm), resources_of_remarks(r.stderr)


def tree_kernels(pool, tree, units, extra):
    """{demangled name: (unit, instructions, resources)}"""
    out = {}
    for unit, insns, res in pool.map(lambda u: compile_unit(tree, u, extra), units):
        names = demangle(tree, sorted(insns))
        for mangled, body in insns.items():
            name = names[mangled]
            if name in out:
                sys.exit("kernel %s is in two units of %s" % (name, tree))
            out[name] = (unit, body, res.get(mangled, {}))
    return out


def short(name):  # for the table: without namespaces and parameters
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("nbody::", "")


def field(res, *keys):  # a remark by its name without the unit, e.g. "LDS Size [bytes/block]"
    for key in keys:
        for k, v in res.items():
            if k.split(" [")[0] == key:
                return v
    return "?"


def compare_sources(args):
    ok = True
    configs = [c.split("=", 1) for c in (args.config or ["product=", "lab=-DNBODY_LAB"])]
    units = args.units.split(",")
    parent_units = (args.parent_units or args.units).split(",")
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        for label, flags in configs:
            extra = shlex.split(flags)
            old = tree_kernels(pool, args.parent, parent_units, extra)
            new = tree_kernels(pool, args.new, units, extra)
            if args.only:
                old = {k: v for k, v in old.items() if k.startswith(args.only)}
                new = {k: v for k, v in new.items() if k.startswith(args.only)}
            same_names = set(old) == set(new)
            ok &= same_names
            print("== %s [%s]: %d kernels in the parent (%s), %d in the new units; name sets equal: %s"
                  % (label, flags, len(old), ",".join(parent_units), len(new), same_names))
            for name in sorted(set(old) ^ set(new)):
                print("   only in the %s: %s" % ("parent" if name in old else "new tree", name))
            for name in sorted(set(old) & set(new)):
                unit, body, res = new[name]
                _, pbody, pres = old[name]
                res_eq, ins_eq = bool(res) and res == pres, body == pbody
                ok &= res_eq and ins_eq
                print("%-28s %-14s sgpr %3s vgpr %3s agpr %3s scratch %2s lds %6s occ %s resources %s  insns %d %s"
                      % (short(name)[:28], unit, field(res, "TotalSGPRs", "SGPRs"), field(res, "VGPRs"), field(res, "AGPRs"),
                         field(res, "ScratchSize"), field(res, "LDS Size"), field(res, "Occupancy"),
                         "= parent" if res_eq else "DIFFER %r / parent %r" % (res, pres), len(body),
                         "= parent" if ins_eq else "DIFFER (parent %d)" % len(pbody)))
    return ok


def device_image(path, tmp):
    """the gfx code object bundled into a host object (section .hip_fatbin), as a file"""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([tool(HERE, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", path, fat], check=True, capture_output=True)
    bundler = tool(HERE, "clang-offload-bundler")
    listed = subprocess.run([bundler, "--list", "--type=o", "--input=" + fat], capture_output=True, text=True, check=True).stdout
    for target in listed.split():
        if target.startswith("hip") and "gfx" in target:
            dev = os.path.join(tmp, "device.co")
            subprocess.run([bundler, "--unbundle", "--type=o", "--input=" + fat, "--targets=" + target, "--output=" + dev],
                           check=True, capture_output=True)
            return dev
    sys.exit("no device code object in %s" % path)


def kernels_of_object(path):
    with tempfile.TemporaryDirectory() as tmp:
        dev = device_image(path, tmp)
        dis = subprocess.run([tool(HERE, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", "--demangle", dev],
                             capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for ln in dis.split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.strip():
            cur.append(" ".join(ln.split("//", 1)[0].split()))
    return out


def compare_objects(paths):
    ok = True
    for a, b in zip(paths[0::2], paths[1::2]):
        ka, kb = kernels_of_object(a), kernels_of_object(b)
        differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        same = set(ka) == set(kb) and not differ
        ok &= same
        print("%s / %s: %d / %d functions, name sets equal: %s, %s"
              % (a, b, len(ka), len(kb), set(ka) == set(kb), "instructions all equal" if not differ else "DIFFER: " + ", ".join(differ)))
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent", nargs="?")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--units", help="comma-separated unit names (csrc/<unit>.hip) of the new tree")
    ap.add_argument("--parent-units", help="... of the parent tree (default: the same)")
    ap.add_argument("--config", action="append", help="LABEL=FLAGS, repeatable (default: product= and lab=-DNBODY_LAB)")
    ap.add_argument("--only", default="", help="compare kernels whose demangled name starts with this")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--objects", nargs="+", metavar="OBJ", help="pairs of built objects to compare instead")
    args = ap.parse_args()
    if args.objects:
        if len(args.objects) % 2:
            ap.error("--objects takes pairs")
        ok = compare_objects(args.objects)
    else:
        if not (args.parent and args.new and args.units):
            ap.error("two trees and --units, or --objects")
        ok = compare_sources(args)
    print("RESULT: %s" % ("every kernel equal" if ok else "DIFFERENCES"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
