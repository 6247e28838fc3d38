"""Which kernels of two gfx950 assembly listings of one source file (hipcc --cuda-device-only -S) have the same text and the
same metadata: comments, label numbers and blank lines dropped, as profiles/r09_a_sweep_12x2_isa.txt compared them.
usage: python scratch/isa_same_kernels.py parent.s this.s [substring of the kernels expected to differ]"""
import re
import sys


def kernels(path):
    txt = open(path).read()
    body, meta = {}, {}
    for m in re.finditer(r"^(_Z\S+):\s*(?:;.*)?$", txt, re.M):
        end = txt.find(".Lfunc_end", m.end())
        lines = []
        for ln in txt[m.end():end].splitlines():
            s = ln.split(";")[0].strip()
            if s:
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
        body[m.group(1)] = "\n".join(lines)
    for blk in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = tuple(re.search(r"\." + k + r":\s+(\d+)", blk).group(1) for k in
                                        ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size", "kernarg_segment_size"))
    return body, meta


def main():
    pb, pm = kernels(sys.argv[1])
    tb, tm = kernels(sys.argv[2])
    expected = sys.argv[3] if len(sys.argv) > 3 else None
    names = [n for n in pb if n in pm]
    missing = [n for n in names if n not in tb]
    new = [n for n in tb if n in tm and n not in pb]
    differ = [n for n in names if n in tb and (pb[n] != tb[n] or pm[n] != tm.get(n))]
    print(f"kernels of the parent {len(names)}; missing here {len(missing)}; new here {len(new)}; text or metadata differs {len(differ)}")
    for n in differ:
        print(("  expected  " if expected and expected in n else "  UNEXPECTED ") + n)
    same = len(names) - len(missing) - len(differ)
    print(f"identical text and metadata: {same}")
    if expected is not None:
        bad = [n for n in differ if expected not in n] + missing
        print("every kernel outside the named family is unchanged" if not bad else f"{len(bad)} kernels outside the named family changed")


if __name__ == "__main__":
    main()
