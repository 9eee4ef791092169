"""Compare the gfx950 code objects embedded in two builds of libsc_engine.so.

    python scripts/code_object_diff.py OLD.so NEW.so

Three comparisons, differences only: the set of kernel names; each kernel's metadata note (registers, spills, LDS,
scratch, kernarg size, workgroup size); each kernel's ``llvm-objdump -d`` text with the address column and the
address / encoding comments stripped, so that a kernel that merely moved inside the code object compares equal.
Exit status 0 when nothing differs, 1 otherwise.  For refactors of the host side: the device code must not change."""
import difflib
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_isa_scratch import READELF, gfx950_code_object  # noqa: E402

OBJDUMP = shutil.which("llvm-objdump") or os.path.join(os.path.dirname(READELF), "llvm-objdump")
NOTE_KEYS = ("sgpr_count", "vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size",
             "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")
SYMBOL = re.compile(r"^[0-9a-f]+ <(\S+)>:$")


def metadata(co):
    notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count", "\n" + notes)[1:]:
        blk = "      .agpr_count" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(m.group(1)) for k in NOTE_KEYS for m in [re.search(r"\." + k + r":\s+(\d+)", blk)] if m}
    return out


def instructions(co, only=None):
    """{symbol: [instruction text]} when `only` names symbols, else {symbol: (count, sha1 of the text)}."""
    cmd = [OBJDUMP, "-d", "--no-show-raw-insn", co]
    if only:
        cmd.insert(2, "--disassemble-symbols=" + ",".join(only))
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    out, name, lines = {}, None, None

    def close():
        if name is not None:
            out[name] = lines if only else (len(lines), hashlib.sha1("\n".join(lines).encode()).hexdigest())

    for raw in proc.stdout:
        m = SYMBOL.match(raw.strip())
        if m:
            close()
            name, lines = m.group(1), []
        elif name is not None and raw.startswith(("\t", " ")):
            text = raw.split("//")[0].strip()           # drops "// <address>: <encoding> <label>"
            if text:
                lines.append(text)
    close()
    if proc.wait():
        raise RuntimeError("llvm-objdump failed on " + co)
    return out


def main(old_so, new_so):
    tmp = tempfile.mkdtemp(prefix="code_object_diff_")
    try:
        cos = []
        for tag, so in (("old", old_so), ("new", new_so)):
            cos.append(os.path.join(tmp, tag + ".co"))
            open(cos[-1], "wb").write(gfx950_code_object(so))
        meta = [metadata(c) for c in cos]
        names = [set(m) for m in meta]
        print(f"kernels: old {len(names[0])}, new {len(names[1])}")
        n_diff = 0
        for tag, only in (("only in old", names[0] - names[1]), ("only in new", names[1] - names[0])):
            for n in sorted(only):
                print(f"{tag}: {n}")
                n_diff += 1
        common = sorted(names[0] & names[1])
        for n in common:
            if meta[0][n] != meta[1][n]:
                delta = {k: (meta[0][n].get(k), meta[1][n].get(k)) for k in NOTE_KEYS if meta[0][n].get(k) != meta[1][n].get(k)}
                print(f"metadata differs: {n}: {delta}")
                n_diff += 1
        text = [instructions(c) for c in cos]
        changed = [n for n in common if text[0].get(n) != text[1].get(n)]
        if changed:
            full = [instructions(c, only=changed) for c in cos]
            for n in changed:
                a, b = full[0].get(n, []), full[1].get(n, [])
                print(f"instructions differ: {n} (old {len(a)}, new {len(b)} instructions)")
                for line in list(difflib.unified_diff(a, b, "old", "new", n=0, lineterm=""))[2:22]:
                    print("    " + line)
                n_diff += 1
        n_ins = sum(text[1][n][0] for n in common if n in text[1])
        print(f"compared {len(common)} kernels, {n_ins} instructions: " +
              ("identical names, metadata and instruction text" if not n_diff else f"{n_diff} differences"))
        return 1 if n_diff else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
