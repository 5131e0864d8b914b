"""Compare the instruction streams of the kernels in two `hipcc --cuda-device-only -S` outputs: python tools/isa_diff.py old.s new.s
Kernels are matched by their demangled base name and template arguments' order of appearance; labels and symbol names are normalised, so a
renamed parameter type does not count, while any changed instruction, operand or kernel-argument offset does."""
import re
import sys


def bodies(path):
    out, name, cur = [], None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, cur = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out.append((name, cur))
                name = None
                continue
            t = line.split(";")[0].strip()
            if not t or t.startswith("."):
                t = re.sub(r"^\.LBB\d+_(\d+):", r"L\1:", t) if t.startswith(".LBB") else ""
            t = re.sub(r"\.LBB\d+_(\d+)", r"L\1", t)
            t = re.sub(r"_Z\w+", "SYM", t)
            if t:
                cur.append(t)
    return out


def base(n):
    m = re.search(r"\d+(attn\w*kernel|rope_store_kernel|kvq\w*kernel)", n)
    return m.group(1) if m else n


old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
pool = list(new)
same = diff = 0
for n, b in old:
    cands = [i for i, (m, _) in enumerate(pool) if base(m) == base(n)]
    if not cands:
        continue
    hit = next((i for i in cands if pool[i][1] == b), None)
    if hit is None:
        diff += 1
        print(f"DIFFERENT  {base(n)}  ({n[:60]}...): {len(b)} instructions, candidates {[len(pool[i][1]) for i in cands]}")
    else:
        same += 1
        print(f"identical  {base(n)}: {len(b)} lines")
        pool.pop(hit)
print(f"{same} identical, {diff} different; only in new: {sorted(set(base(m) for m, _ in pool if 'kernel' in base(m)))[:8]}")
