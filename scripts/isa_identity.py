"""Are the device instruction streams of a translation unit's kernels the same as at another commit?  (How "the device code is unchanged" is checked when an
experiment is added to a translation unit or its launch layer is rewritten: the kernels that were measured on the GPU must compile to exactly the code that was measured.)

    python scripts/isa_identity.py <git-rev> [file.hip ...]          # default files: y7t_conv.hip y7t_conv_patch.hip
        -D NAME            also define NAME on both sides (-D Y7T_ABLATE_BUILD: the measuring build)
        --names FILE       functions that were renamed since <git-rev>: lines "old name -> new name", names as c++filt prints them without the parameter list
                           (k_tracker_step1<256> -> k_tracker_step<0, 256>); '#' starts a comment
        --table FILE       write the comparison, one line per function, to FILE

Compiles each file at <git-rev> (its csrc/ and include/ extracted to a temporary directory) and in the working tree to gfx950 assembly (hipcc -S --cuda-device-only with
the file's flags of yolov7-tracker_amd/build.py) and compares function by function -- kernels and the device functions they call: label numbers (basic blocks, relaxed
long branches) and the names of the
file's own functions are normalised (a renamed function, or one whose template or argument list changed, has another mangled name), everything else must match.  For
kernels the resource numbers of the code object's metadata are compared as well (.vgpr_count .agpr_count .sgpr_count .private_segment_fixed_size .vgpr_spill_count
.sgpr_spill_count .group_segment_fixed_size .max_flat_workgroup_size); a device function has the first four of them (its "Function info" block).  A function whose
instructions differ only in the operands of scalar loads (s_load_*: the kernel-argument loads of a kernel whose argument list changed) and in .amdhsa_kernarg_size is
reported as such.  Functions that exist only
on one side are listed, not counted as differences.  Exit code 1 if a function that exists on both sides differs in more than its kernel-argument loads or in a number."""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
NUMBERS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
           ".max_flat_workgroup_size"]
FUNC_INFO = {"NumVgprs": ".vgpr_count", "NumAgprs": ".agpr_count", "TotalNumSgprs": ".sgpr_count", "ScratchSize": ".private_segment_fixed_size"}


def build_flags(f):
    """the flags build.py compiles `f` with, without its include directory (each side has its own)"""
    spec = importlib.util.spec_from_file_location("y7t_build", os.path.join(ROOT, "yolov7-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    flags, skip = [], False
    for x in b.FLAGS + b.FILE_FLAGS.get(f, []):
        if skip or x == "-I":
            skip = not skip
            continue
        if not x.startswith("-W"):
            flags.append(x)
    return flags


def asm(csrc, include, f, out, defines):
    cmd = [HIPCC] + build_flags(f) + ["-D" + d for d in defines] + ["-S", "--cuda-device-only", "-I", include, "-I", csrc, os.path.join(csrc, f), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def short_names(mangled):
    """mangled -> what c++filt prints, without return type and parameter list: k_tracker_step<0, 256>"""
    if not mangled:
        return {}
    out = subprocess.run([CXXFILT], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
    res = {}
    for m, d in zip(mangled, out):
        d = d.replace("(anonymous namespace)::", "")      # (its '(' is not the parameter list's)
        depth, start, end = 0, 0, len(d)
        for i, ch in enumerate(d):      # the name lies between the last blank and the first '(' outside template brackets
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == " " and depth == 0:
                start = i + 1
            elif ch == "(" and depth == 0:
                end = i
                break
        res[m] = d[start:end]
    return res


def functions(path):
    """-> {mangled name: (instruction lines, numbers)} of an assembly file"""
    t = open(path).read().splitlines()
    out, i = {}, 0
    while i < len(t):
        m = re.match(r"^(_Z\S+):", t[i])
        if m and "@" in t[i]:
            name, j = m.group(1), i + 1
            while j < len(t) and not t[j].startswith(".Lfunc_end"):
                j += 1
            # (label numbers count the file's functions / long branches in front of this one: .LBB<function>_<block>, .Lpost_getpc<n> of a relaxed branch)
            body = [re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip())) for l in t[i + 1:j]]
            body = [l for l in body if l.strip() and not l.strip().startswith((".loc", ".file", ".cfi", ".section", ".text"))]      # (.section / .text behind a kernel's descriptor: where the NEXT function goes)
            nums, k = {}, j
            while k < len(t) and not t[k].startswith("; Function info:") and ".amdhsa_kernel" not in t[k] and "@function" not in t[k]:
                k += 1
            if k < len(t) and t[k].startswith("; Function info:"):      # (a device function; a kernel's numbers come from the metadata below)
                for l in t[k + 1:k + 12]:
                    mm = re.match(r"^; (\w+): (\d+)", l)
                    if mm and mm.group(1) in FUNC_INFO:
                        nums[FUNC_INFO[mm.group(1)]] = mm.group(2)
            out[name] = (body, nums)
            i = j
        i += 1
    # kernels: the numbers of the code object's metadata
    cur, inside = None, False
    for l in t:
        if l.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and re.match(r"^\S", l):
            inside = False
        elif inside:
            mm = re.match(r"^  (- |  )(\.\w+):\s*(.*)$", l)
            if not mm:
                continue
            if mm.group(1) == "- ":
                cur = {}
            cur[mm.group(2)] = mm.group(3)
            if mm.group(2) == ".name" and mm.group(3) in out:
                out[mm.group(3)] = (out[mm.group(3)][0], cur)
    return out


def kernarg_line(x, y):
    """two lines that may differ where only the argument list of a kernel changed: a scalar load (of an argument, at another offset) or the size of the argument segment"""
    x, y = x.split()[0], y.split()[0]
    return x == y and (x.startswith("s_load_") or x == ".amdhsa_kernarg_size")


def compare(f, a, b, renamed, rows, what, rev):
    """a, b: functions() of the two sides; appends a row per paired function to `rows` -> how many differ"""
    sa, sb = short_names(list(a)), short_names(list(b))
    by_short = {}
    for m, s in sb.items():
        by_short.setdefault(s, []).append(m)
    # old mangled name -> new mangled name: the same mangled name, or the one function of the (renamed) short name
    pair = {}
    for m, s in sa.items():
        cand = by_short.get(renamed.get(s, s), [])
        if m in b and s not in renamed:
            pair[m] = m
        elif len(cand) == 1:
            pair[m] = cand[0]
    # the conv kernels' defaulted trailing int parameter added since (NW = 4)
    for m in a:
        if m not in pair:
            hit = next((c for c in (m.replace("EEv11Y7TConvArgs", "ELi%dEEv11Y7TConvArgs" % d) for d in (4, 0)) if c in b), None)
            if hit:
                pair[m] = hit
    # every own function's name, on either side, reads the same: longest first, so that no name is rewritten inside a longer one
    subst = sorted(((m, "FN<%s>" % sb[pair[m]]) for m in pair), key=lambda x: -len(x[0]))
    subst_new = sorted(((m, "FN<%s>" % s) for m, s in sb.items()), key=lambda x: -len(x[0]))

    def norm(body, table):
        res = []
        for l in body:
            if "_Z" in l:
                for m, s in table:
                    if m in l:
                        l = l.replace(m, s)
            res.append(l)
        return res

    same = diff = kernarg = 0
    gone = [m for m in a if m not in pair]
    for m in a:
        if m not in pair:
            continue
        (body_a, num_a), (body_b, num_b) = a[m], b[pair[m]]
        body_a, body_b = norm(body_a, subst), norm(body_b, subst_new)
        nums_same = all(num_a.get(k) == num_b.get(k) for k in NUMBERS)
        if body_a == body_b:
            verdict = "identical"
        elif len(body_a) == len(body_b) and all(x == y or kernarg_line(x, y) for x, y in zip(body_a, body_b)):
            verdict = "kernel-argument loads only (%d lines)" % sum(x != y for x, y in zip(body_a, body_b))
        else:
            verdict = "DIFFERENT"
        if not nums_same:
            verdict += ", NUMBERS DIFFER"
        if verdict == "identical":
            same += 1
        elif verdict.startswith("kernel-argument loads only") and nums_same:
            kernarg += 1
        else:
            diff += 1
            print("DIFFERENT", f, sa[m], "->", sb[pair[m]], ":", verdict)
        rows.append((f, sa[m], sb[pair[m]], [num_a.get(k, "-") for k in NUMBERS], [num_b.get(k, "-") for k in NUMBERS], len(body_a), len(body_b), verdict))
    new = [m for m in b if m not in pair.values()]
    print("%s: %d functions identical, %d differ in kernel-argument loads only, %d different, %d only at %s, %d only in the working tree" %
          (what, same, kernarg, diff, len(gone), rev, len(new)))
    for m in gone:
        print("  only at %s: %s" % (rev, sa[m]))
    for m in new:
        print("  only in the working tree: %s" % sb[m])
    return diff


def read_names(path):
    table = {}
    if path:
        for l in open(path):
            l = l.split("#")[0].strip()
            if l:
                a, b = l.split("->")
                table[a.strip()] = b.strip()
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev")
    ap.add_argument("files", nargs="*", default=["y7t_conv.hip", "y7t_conv_patch.hip"])
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--names")
    ap.add_argument("--table")
    args = ap.parse_args()
    renamed = read_names(args.names)
    bad, rows = 0, []
    with tempfile.TemporaryDirectory() as tmp:
        old_csrc, old_inc = os.path.join(tmp, "yolov7-tracker_amd", "csrc"), os.path.join(tmp, "include")      # (csrc includes "../../include/y7t.h")
        os.makedirs(old_csrc), os.makedirs(old_inc)
        for d, dst in (("yolov7-tracker_amd/csrc", old_csrc), ("include", old_inc)):
            names = subprocess.check_output(["git", "ls-tree", "--name-only", args.rev, d + "/"], cwd=ROOT, text=True).split()
            for n in names:
                open(os.path.join(dst, os.path.basename(n)), "wb").write(subprocess.check_output(["git", "show", "%s:%s" % (args.rev, n)], cwd=ROOT))
        for f in args.files:
            a = functions(asm(old_csrc, old_inc, f, os.path.join(tmp, "old.s"), args.defines))
            b = functions(asm(os.path.join(ROOT, "yolov7-tracker_amd", "csrc"), os.path.join(ROOT, "include"), f, os.path.join(tmp, "new.s"), args.defines))
            d = compare(f, a, b, renamed, rows, "%s vs %s%s" % (f, args.rev, "".join(" -D" + x for x in args.defines)), args.rev)
            bad += d
    if args.table:
        with open(args.table, "w") as o:
            o.write("# scripts/isa_identity.py %s %s%s\n" % (args.rev, " ".join(args.files), "".join(" -D " + d for d in args.defines)))
            o.write("# numbers: %s ('-': a device function has no such number)\n" % " ".join(NUMBERS))
            o.write("# file | old name | new name | numbers old | numbers new | instruction lines old / new | verdict\n")
            for f, s_old, s_new, na, nb, la, lb, verdict in rows:
                o.write("%s | %s | %s | %s | %s | %d / %d | %s\n" % (f, s_old, s_new, " ".join(na), " ".join(nb), la, lb, verdict))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
