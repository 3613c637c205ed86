"""Whole-kernel mnemonic counts that differ between two hipcc -S listings of the same source (before / after a change).
usage: python tools/isa_diff.py before.s after.s <mangled kernel-name substring>
Complements tools/isa_hist.py (one pair body): a change that splits the body into several blocks still shows as counts here."""
import collections, re, sys
def hist(path, want):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if want in l and re.match(r"^_Z\S+:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    c = collections.Counter()
    for l in lines[start + 1:end]:
        t = l.strip()
        if not t or t.startswith(";") or t.startswith(".") or re.match(r"^\S+:(\s|$)", t):
            continue
        c[t.split()[0]] += 1
    return c
want = sys.argv[3]
a, b = hist(sys.argv[1], want), hist(sys.argv[2], want)
print(want, "total", sum(a.values()), "->", sum(b.values()), " VALU", sum(v for k, v in a.items() if k.startswith("v_")), "->", sum(v for k, v in b.items() if k.startswith("v_")))
for k in sorted(set(a) | set(b)):
    if a[k] != b[k]:
        print(f"  {k:30s} {a[k]:6d} -> {b[k]:6d}  ({b[k]-a[k]:+d})")
