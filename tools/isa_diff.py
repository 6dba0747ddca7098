"""Compare the kernels of device assembly files (hipcc --cuda-device-only -S) after a source move:
python tools/isa_diff.py parent.s new_a.s [new_b.s ...]. Kernels are matched by demangled name with
the namespaces given by --ns (default: the anonymous one, attn, f32, conv) dropped, and a parent's
kernel with the new one that dropped template arguments of one value (RENAMES); a body is its text
from the label to .Lfunc_end with comments stripped, local labels renumbered and other symbols' names
blanked; the resources are its .amdhsa_ lines. A kernel that several new files hold (a static
__global__ of a shared header) is compared once per copy. Several parent files: concatenate them."""
import argparse
import re
import subprocess

from isa_stats import kernels


def demangle(names):
    # binutils' c++filt does not know DF16b (__bf16): pass it as Dh (half; not a substitution
    # candidate either, so the rest of the name demangles alike) and rename it afterwards
    text = "\n".join(n.replace("DF16b", "Dh") for n in names)
    out = subprocess.run(["c++filt"], input=text, capture_output=True, text=True, check=True).stdout
    return dict(zip(names, re.sub(r"\b(half|__fp16)\b", "bf16", out).split("\n")))


def body(text):
    lines = []
    for raw in text.split("\n"):
        l = re.sub(r"\s+", " ", raw.split(";")[0]).strip()
        if l and not l.startswith((".section", ".text")):      # the next function's section: linkage only
            lines.append(re.sub(r"\b_Z\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", l)))
    return lines


def resources(text):
    res = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        res[m.group(1)] = dict(l.split()[:2] for l in m.group(2).split("\n") if l.strip().startswith(".amdhsa_"))
    return res


def load(paths, ns):
    out = {}
    for p in paths:
        text = open(p).read()
        res = resources(text)
        ks = dict(kernels(text))
        for name, pretty in demangle(list(ks)).items():
            key = re.sub(r"^void ", "", pretty)
            for n in ns:
                key = key.replace(n + "::", "")
            out.setdefault(key, []).append((body(ks[name]), res[name], p))
    return out


# a parent kernel that lost template arguments which had one value: (pattern, its new name)
RENAMES = [
    (r"^(\w+)<float>\(", r"\1("),                                 # K<float>(..) became a plain K(..)
    (r"^(stem_bwd_apply2_kernel<\w+), 1>", r"\1>"),                # <T, U = 1> -> <T>
]


def untemplated(old, new):
    """parent kernels whose name matches a RENAMES pattern and exists only in its new form: under the new name"""
    for key in [k for k in old if k not in new]:
        for pat, repl in RENAMES:
            short = re.sub(pat, repl, key)
            if short != key and short in new and short not in old:
                old[short] = old.pop(key)
                break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new", nargs="+")
    ap.add_argument("--ns", default="(anonymous namespace),attn,f32,conv")
    a = ap.parse_args()
    ns = a.ns.split(",")
    old, new = load([a.parent], ns), load(a.new, ns)
    untemplated(old, new)
    same = copies = 0
    none = [(None, None, None)]
    for key, (b1, r1, path) in sorted(((k, c) for k in set(old) | set(new) for c in new.get(k, none)), key=lambda kc: kc[0]):
        if key not in old or b1 is None:
            print("ONLY IN", "parent" if key in old else path, key)
            continue
        b0, r0, _ = old[key][0]
        copies += 1
        rdiff = {k: (r0.get(k), r1.get(k)) for k in set(r0) | set(r1) if r0.get(k) != r1.get(k)}
        r = r1
        tag = "identical" if b0 == b1 and not rdiff else "DIFFERS"
        same += tag == "identical"
        print(f"{tag} {len(b1)} lines vgpr {r['.amdhsa_next_free_vgpr']} sgpr {r['.amdhsa_next_free_sgpr']} lds "
              f"{r['.amdhsa_group_segment_fixed_size']} scratch {r['.amdhsa_private_segment_fixed_size']}  {path}  {key}")
        if b0 != b1:
            print(f"    body: {len(b0)} -> {len(b1)} lines, first difference at line "
                  f"{next((i for i, (x, y) in enumerate(zip(b0, b1)) if x != y), min(len(b0), len(b1)))}")
        for k, v in sorted(rdiff.items()):
            print(f"    {k}: {v[0]} -> {v[1]}")
    print(f"kernels: parent {len(old)}, new {len(new)} in {sum(map(len, new.values()))} copies, compared {copies}, "
          f"identical {same}")


if __name__ == "__main__":
    main()
