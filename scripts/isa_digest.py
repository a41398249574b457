"""One line per kernel of the given HIP sources: a hash of its machine code and its resource numbers
(cross-compiles without a GPU).  Two trees emit the same code for a kernel iff its lines agree:

    python scripts/isa_digest.py vln-ce_amd/csrc/conv_u3.hip ... | sort > after.txt; diff before.txt after.txt

The hash (SHA-1) is over the kernel's instruction and label lines with directives and `;` comments
stripped and the local labels .LBB<n>_<m> renumbered in order of first appearance, so that moving a
kernel to another file (another function number n) does not change it.
Only symbols with a kernel descriptor are hashed (a device function that is not inlined is not seen),
and equal rows are printed once: a header's kernel that compiled differently in two files shows as
two rows under one name.
Line: demangled name | sha1 | instructions | next_free_vgpr | next_free_sgpr | LDS bytes | scratch bytes
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]
WANT = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(asm):
    """(mangled name, body lines, {amdhsa field: value}) of every kernel in an assembly listing"""
    lines = asm.split("\n")
    desc = {}   # mangled name -> descriptor fields
    name = None
    for l in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            name = m.group(1)
            desc[name] = {}
        elif name and l.strip() == ".end_amdhsa_kernel":
            name = None
        elif name:
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", l)
            if m:
                desc[name][m.group(1)] = m.group(2)
    out, name, body = [], None, []
    for l in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", l)
        if m and m.group(1) in desc:
            name, body = m.group(1), []
        elif name and (re.match(r"^\.Lfunc_end\d+:", l) or re.match(r"\s*\.section\b", l)):
            out.append((name, body, desc[name]))
            name = None
        elif name:
            body.append(l)
    return out


def digest(body):
    labels = {}

    def renumber(m):
        return labels.setdefault(m.group(0), f".LBB_{len(labels)}")

    kept, n_instr = [], 0
    for l in body:
        l = l.split(";", 1)[0].strip()
        if not l or (l.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", l)):
            continue   # comments, directives
        n_instr += not l.endswith(":")
        kept.append(re.sub(r"\s+", " ", re.sub(r"\.LBB\d+_\d+", renumber, l)))
    return hashlib.sha1("\n".join(kept).encode()).hexdigest(), n_instr


def main():
    rows = []
    extra = [a for a in sys.argv[1:] if a.startswith("-")]   # e.g. -DVLNCE_DBG_TIME
    for src in (a for a in sys.argv[1:] if not a.startswith("-")):
        if src.endswith(".s"):   # a listing kept from an earlier run (hipcc -S / -save-temps)
            asm = open(src).read()
        else:
            with tempfile.TemporaryDirectory() as tmp:
                s = os.path.join(tmp, "out.s")
                r = subprocess.run([HIPCC] + FLAGS + extra + [src, "-o", s], capture_output=True, text=True)
                if r.returncode != 0:
                    sys.exit(f"{src}: hipcc failed\n{r.stderr}")
                asm = open(s).read()
        ks = kernels(asm)
        dem = subprocess.run(["c++filt"], input="\n".join(k[0] for k in ks), capture_output=True,
                             text=True).stdout.split("\n")
        for (_, body, d), pretty in zip(ks, dem):
            sha, n = digest(body)
            pretty = re.sub(r"^void |vlnce_detail::\(anonymous namespace\)::|vlnce_detail::|\(anonymous namespace\)::", "", pretty)
            rows.append(" | ".join([re.sub(r"\(.*$", "", pretty), sha, str(n)] + [d.get(k, "?") for k in WANT]))
    print("\n".join(sorted(set(rows))))   # (a header's kernel, the same in every file that includes it: once)


if __name__ == "__main__":
    main()
