"""Compare two gfx950 device assembly files (hipcc --cuda-device-only -S) function by function.

    python tools/isa_same.py A.s B.s [SUBSTRING]

For every function present in both files (names holding SUBSTRING, when given) the instruction lines are
compared after the labels that number themselves per translation unit -- .LBB<n>_<m> and .Lpost_getpc<n> --
are normalised.  Prints the functions that differ and those present in only one file; exit status 1 when
there are any.  Text comparison only: a refactor that moves kernels between translation units can show that
the generated code did not change.
"""
import re
import sys


def functions(path):
    """{name: [instruction lines]} of the functions of a device assembly file."""
    out, name, funcs = {}, None, set()
    for line in open(path):
        m = re.match(r"^\s*\.type\s+([\w$.]+),@function", line)
        if m:
            funcs.add(m.group(1))
            continue
        m = re.match(r"^([\w$.]+):", line)
        if m and m.group(1) in funcs:
            name = m.group(1)
            out[name] = []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            name = None
            continue
        if name is None:
            continue
        s = line.split(";", 1)[0].strip()  # drop comments
        if not s or (s.startswith(".") and not s.startswith(".L")):
            continue  # directives
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        s = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", s)
        out[name].append(s)
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    sub = sys.argv[3] if len(sys.argv) > 3 else ""
    names = sorted(n for n in set(a) | set(b) if sub in n)
    both = [n for n in names if n in a and n in b]
    differ = [n for n in both if a[n] != b[n]]
    for n in differ:
        i = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
        print(f"DIFFERS  {n}: {len(a[n])} vs {len(b[n])} instruction lines, first difference at line {i}")
    only = [(n, "A" if n in a else "B") for n in names if (n in a) != (n in b)]
    for n, w in only:
        print(f"ONLY IN {w}  {n}")
    print(f"{len(both)} functions in both files: {len(both) - len(differ)} identical, {len(differ)} differ; "
          f"{sum(w == 'A' for _, w in only)} only in A, {sum(w == 'B' for _, w in only)} only in B")
    sys.exit(1 if differ or only else 0)


if __name__ == "__main__":
    main()
