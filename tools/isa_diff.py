"""Compare the instruction streams of the kernels in two sets of `hipcc --cuda-device-only -S` outputs:
    python tools/isa_diff.py old.s[,old2.s...] new.s[,new2.s...]
Kernels are matched by their demangled base name and template arguments' order of appearance; labels and symbol names are normalised, so a
renamed parameter type does not count, while any changed instruction, operand or kernel-argument offset does.  The rows GEMV's kernels are
matched by their template arguments, the weight format as a number (gemv_rows_kernel's bool F8 -> 0 / 1, a gemv_rows_mx_kernel -> 2), and so are
the streaming GEMV's (gemv_stream_kernel by its six arguments, a gemv_mx_kernel<M, DUAL, KSPLIT, KU> -> <M, DUAL, KSPLIT, KU, 4, 3>),
and the conv tokenizers' row-in kernels by theirs with the row count in front (a row_in_kernel<NT> -> row_in_rows_kernel<1, NT>, the earlier
row_in_rows_kernel<BT> -> <BT, 0>): a kernel
whose stream differs is listed with the registers, LDS, scratch and spill counts of its metadata on both sides, a kernel (or device function)
that only one set holds with the side it is on.  Exit status 1 when a kernel differs or is missing from the new set, else 0."""
import re
import sys

META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def bodies(paths):
    out = []
    for path in paths.split(","):
        name, cur = None, []
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


def meta(paths):
    """kernel symbol -> {field: value} of the amdhsa.kernels metadata"""
    out = {}
    for path in paths.split(","):
        text = open(path).read()
        for block in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            out[name] = {f: int(re.search(rf"\.{f}:\s+(\d+)", block).group(1)) for f in META}
    return out


def base(n):
    m = re.search(r"\d+gemv_rows(_mx)?_kernelI((?:L[bi]\d+E)+)E", n)
    if m:
        args = re.findall(r"L[bi](\d+)E", m.group(2)) + (["2"] if m.group(1) else [])
        return "gemv_rows_kernel<" + ",".join(args) + ">"
    m = re.search(r"\d+gemv_(stream|mx)_kernelI((?:L[bi]\d+E)+)E", n)
    if m:
        args = re.findall(r"L[bi](\d+)E", m.group(2)) + (["4", "3"] if m.group(1) == "mx" else [])
        return "gemv_stream_kernel<" + ",".join(args) + ">"
    m = re.search(r"\d+row_in(_rows)?_kernelI((?:L[bi]\d+E)+)E", n)
    if m:
        args = re.findall(r"L[bi](\d+)E", m.group(2))
        return "row_in_rows_kernel<" + ",".join((["1"] if not m.group(1) else []) + args + (["0"] if m.group(1) and len(args) == 1 else [])) + ">"
    m = re.search(r"\d+(attn\w*kernel|rope_store_kernel|kvq\w*kernel)", n)
    return m.group(1) if m else n


def count(body):
    return sum(not t.endswith(":") for t in body)


old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
mo, mn = meta(sys.argv[1]), meta(sys.argv[2])
pool = list(new)
same = diff = 0
only_old = []
for n, b in old:
    cands = [i for i, (m, _) in enumerate(pool) if base(m) == base(n)]
    if not cands:
        only_old.append(base(n))
        continue
    hit = next((i for i in cands if pool[i][1] == b), None)
    if hit is None:
        diff += 1
        print(f"DIFFERENT  {base(n)}  ({n[:60]}...): {count(b)} instructions, candidates {[count(pool[i][1]) for i in cands]}")
        for i in cands:
            print("           " + "  ".join(f"{f} {mo[n][f]} -> {mn[pool[i][0]][f]}" for f in META))
    else:
        same += 1
        print(f"identical  {base(n)}: {len(b)} lines")
        pool.pop(hit)
pool = [(m, b) for m, b in pool if base(m) not in {base(n) for n, _ in old}]     # what is left of a matched name is listed above as DIFFERENT
only_new = sorted(set(base(m) for m, _ in pool))
for side, names in (("old", sorted(set(only_old))), ("new", only_new)):
    for name in names:
        print(f"ONLY IN {side.upper()}  {name}")
print(f"{same} identical, {diff} different, {len(only_old)} only in old, {len(pool)} only in new")
sys.exit(1 if diff or only_old else 0)
