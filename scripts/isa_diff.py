#!/usr/bin/env python3
"""scripts/isa_diff.py <a.s> <b.s>: compare two outputs of scripts/disasm.sh kernel by kernel.

Per symbol, the instruction text with addresses and encodings removed; trailing s_nop / s_code_end padding (a kernel that
is the last of its code object carries some) and llvm-objdump's non-instruction lines are ignored.  Prints the symbols
present on one side only and the symbols whose streams differ, with both lengths.  Exits 0 either way: it reports.
"""
import re
import sys

SYMBOL = re.compile(r"^[0-9a-f]+ <(.+)>:$")
PADDING = ("s_nop", "s_code_end")


def streams(path):
    out, cur = {}, None
    for line in open(path):
        m = SYMBOL.match(line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line[:1] in " \t" and "//" in line:      # an instruction: "\t<text>  // <address>: <encoding>"
            cur.append(" ".join(line.split("//")[0].split()))
    for ins in out.values():
        while ins and ins[-1].split()[0] in PADDING:
            ins.pop()
    return out


def main(a_path, b_path):
    a, b = streams(a_path), streams(b_path)
    for title, names in ((f"only in {a_path}", sorted(set(a) - set(b))), (f"only in {b_path}", sorted(set(b) - set(a)))):
        print(f"{title}: {len(names)}")
        for n in names:
            print(f"  {n}")
    differ = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    print(f"in both: {len(set(a) & set(b))}, identical: {len(set(a) & set(b)) - len(differ)}, different: {len(differ)}")
    for n in differ:
        print(f"  {n}: {len(a[n])} -> {len(b[n])} instructions")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
