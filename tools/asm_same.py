#!/usr/bin/env python
"""tools/asm_same.py A.s B.s: are two device-assembly listings the same code, function by function?

A listing is cut into functions at its `.type <sym>,@function` ... `.size <sym>` lines (the kernel descriptors and
everything else outside them are not compared); the `__hip_cuid_<hash>` object is ignored, since the hash changes with
any edit of the source text.  Text is compared as it stands.  Prints the functions that were added, removed or differ,
then one count line; the exit status is 1 on any difference.
"""
import re
import sys

TYPE = re.compile(r"\s*\.type\s+([^,\s]+),@function")
SIZE = re.compile(r"\s*\.size\s+([^,\s]+),")


def functions(text):
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = TYPE.match(line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None:
            m = SIZE.match(line)
            if m and m.group(1) == name:
                out[name] = "\n".join(l for l in body if "__hip_cuid_" not in l)
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
