"""Per-kernel comparison of two device-assembly files of the same translation unit (no GPU needed): the method of
profiles/composed_prune.md and profiles/argument_prune.md.
    hipcc --offload-arch=gfx950 <the flags csrc/Makefile gives the file> --cuda-device-only -S X.hip -o X.s     (twice)
    python tools/asm_table.py parent.s new.s
Per `.amdhsa_kernel` entry: the text from the kernel's label to its .Lfunc_end, comments and blank lines dropped, every
mangled name replaced by one token and every .LBBn_m label by its order of appearance, hashed (SHA-256, 16 hex digits);
instructions = the lines of that text that are neither labels nor directives; VGPR / SGPR / scratch / LDS from
.amdhsa_next_free_vgpr, .amdhsa_next_free_sgpr, .amdhsa_private_segment_fixed_size, .amdhsa_group_segment_fixed_size.
Below the table, for every kernel whose hash changed: the mnemonics whose count differs (parent -> new).  A kernel that is not
listed there but changed its hash holds the same instructions in another order or with other registers."""
import collections, hashlib, re, subprocess, sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    out = {}
    for block in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        name = block.group(1)
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        lines = [l.split(";")[0].strip() for l in body.splitlines()]
        lines = [re.sub(r"_Z\w+", "SYM", l) for l in lines if l]
        labels = {}
        for l in lines:
            for lab in re.findall(r"\.LBB\d+_\d+", l):
                labels.setdefault(lab, "L%d" % len(labels))
        lines = [re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], l) for l in lines]
        insts = sum(1 for l in lines if not l.endswith(":") and not l.startswith("."))
        res = tuple(int(re.search(r"\.amdhsa_%s (\d+)" % f, block.group(2)).group(1)) for f in FIELDS)
        ops = collections.Counter(l.split()[0] for l in lines if not l.endswith(":") and not l.startswith("."))
        out[name] = (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], insts) + res + (ops,)
    return out


def main():
    sides = []
    for path in sys.argv[1:3]:  # keyed by the demangled name without its parameter list: a dropped argument changes the mangled one
        k = kernels(path)
        plain = subprocess.run(["c++filt"] + list(k), capture_output=True, text=True).stdout.splitlines()
        sides.append({re.sub(r"^void |\(.*$", "", p): v for p, v in zip(plain, k.values())})
    old, new = sides
    print("| kernel | parent hash | new hash | instructions | VGPR | SGPR | scratch B | LDS B |\n|---|---|---|---|---|---|---|---|")
    for n in sorted(set(old) | set(new)):
        o, w = old.get(n), new.get(n)
        cell = lambda i: str((o or w)[i]) if o is None or w is None or o[i] == w[i] else "%d -> %d" % (o[i], w[i])
        print("| `%s` | %s | %s | %s |" % (n, o[0] if o else "absent", w[0] if w else "gone", " | ".join(cell(i) for i in range(1, 6))))
    same = sum(1 for n in old if n in new and old[n][0] == new[n][0])
    print("\n%d kernels in parent, %d in new, %d with the same hash" % (len(old), len(new), same))
    for n in sorted(set(old) & set(new)):
        a, b = old[n][6], new[n][6]
        moved = ["%s %d -> %d" % (m, a[m], b[m]) for m in sorted(set(a) | set(b)) if a[m] != b[m]]
        if moved:
            print("\n`%s`: %s" % (n, ", ".join(moved)))


if __name__ == "__main__":
    main()
