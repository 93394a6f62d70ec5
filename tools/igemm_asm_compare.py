"""Compares the gfx950 assembly of csrc/igemm.hip from two builds kernel by kernel, whatever order the kernels were emitted in.

    python tools/igemm_asm_compare.py PARENT.s BRANCH.s        (the files build.py's audit leaves under ctrl-adapter_amd/build/)

The compiler emits the template instantiations in the order the host code first names them, and numbers its local labels
(.LBB<n>_*, .Lfunc_end<n>, .Lpost_getpc<n>, the "BB<n>_*" of its loop comments) by that position.  A host-side change that names the
same kernels in another order therefore moves whole functions and renumbers those labels without touching an instruction.  This tool
cuts both files into per-kernel pieces (text, kernel descriptor, resource comments, metadata entry), drops the position numbers and
the comment-column padding, and requires every piece -- and the file's preamble and epilogue, up to the __hip_cuid_<hash> symbol the
compiler derives from the source PATH -- to be equal.  Exit status 0 = equal."""
import re
import sys


def pieces(path):
    txt = open(path).read()
    meta_at = txt.index("\t.amdgpu_metadata")
    body, meta = txt[:meta_at], txt[meta_at:]
    starts = [m.start() for m in re.finditer(r"^\t\.section\t\.text\.[^\n]*\n\t\.globl\t", body, re.M)]
    tail_at = body.index("\t.section\t.AMDGPU.gpr_maximums")
    out = {"<preamble>": body[:starts[0]], "<epilogue>": re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", body[tail_at:])}
    order = []
    for a, b in zip(starts, starts[1:] + [tail_at]):
        sym = re.match(r"\t\.section\t\.text\.([^,]+),", body[a:]).group(1)
        ch = re.sub(r"BB\d+_", "BB_", body[a:b])
        ch = re.sub(r"\.L(func_begin|func_end|tmp|post_getpc)\d+", r".L\1", ch)
        assert sym not in out, sym
        out[sym] = re.sub(r"[ \t]+;", " ;", ch)
        order.append(sym)
    entries = re.split(r"(?m)^  - \.agpr_count:", meta)          # one metadata entry per kernel, then the target / version tail
    last, _, tail = entries[-1].partition("amdhsa.target")
    out["<metadata head>"], out["<metadata tail>"] = entries[0], tail
    for e in entries[1:-1] + [last]:
        out["metadata of " + re.search(r"\.name:\s+(\S+)", e).group(1)] = e
    return out, order


def main(a, b):
    (pa, oa), (pb, ob) = pieces(a), pieces(b)
    bad = sorted(set(pa) ^ set(pb)) + [k for k in pa if k in pb and pa[k] != pb[k]]
    for k in bad:
        print("DIFFERS: %s" % k)
    print("%d kernels; emitted in the same order: %s; %s" % (len(oa), oa == ob, "DIFFERENT" if bad else "every kernel identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
