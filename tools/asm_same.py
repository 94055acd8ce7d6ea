#!/usr/bin/env python
"""tools/asm_same.py A.s B.s: are two device-assembly listings the same code, function by function?

A listing is cut into functions at its `.type <sym>,@function` ... `.size <sym>` lines (the kernel descriptors and
everything else outside them are not compared); the `__hip_cuid_<hash>` object is ignored, since the hash changes with
any edit of the source text.  What is compared is the code: everything from `;` to the end of a line is a comment, and the
compiler's local labels (.LBB<f>_<n>, .LJTI<f>_<n>, .LCPI<f>_<n>, .Lfunc_begin<f>, .Lfunc_end<f>) carry the index <f> of the
function within its translation unit, which moves when a function is compiled next to other ones: the index is dropped, the
block number <n> stays.  .Ltmp<n> counts through the whole unit and is renumbered by first appearance within the function.
Everything else is compared as it stands.  A tree of several translation units is compared by concatenating its listings
(cat mrtx_kernels.s mrtx_terrain.s).  Prints the functions that were added, removed or differ, then one count line; the exit
status is 1 on any difference.
"""
import re
import sys

TYPE = re.compile(r"\s*\.type\s+([^,\s]+),@function")
SIZE = re.compile(r"\s*\.size\s+([^,\s]+),")
INDEXED = re.compile(r"\.L(BB|JTI|CPI)\d+_(\d+)\b")
FUNC = re.compile(r"\.Lfunc_(begin|end)\d+\b")
TMP = re.compile(r"\.Ltmp\d+\b")


def code(body):
    """The lines of a function body without comments and without the compiler's numbering of its local labels."""
    tmp, out = {}, []
    for line in body:
        line = line.split(";", 1)[0].rstrip()
        if not line or "__hip_cuid_" in line:
            continue
        line = FUNC.sub(r".Lfunc_\1", INDEXED.sub(r".L\1_\2", line))
        out.append(TMP.sub(lambda m: ".Ltmp_%d" % tmp.setdefault(m.group(0), len(tmp)), line))
    return "\n".join(out)


def functions(text):
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = TYPE.match(line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None:
            m = SIZE.match(line)
            if m and m.group(1) == name:
                out[name] = code(body)
                name = None
            else:
                body.append(line)
    return out


def compare(a_text, b_text, out=sys.stdout):
    a, b = functions(a_text), functions(b_text)
    removed, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    for tag, names in (("removed", removed), ("added", added), ("differs", differ)):
        for n in names:
            print(tag, n, file=out)
    print(f"{len(a)} / {len(b)} functions: {len(differ)} differ, {len(added)} added, {len(removed)} removed", file=out)
    return 1 if removed or added or differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(compare(open(sys.argv[1]).read(), open(sys.argv[2]).read()))
