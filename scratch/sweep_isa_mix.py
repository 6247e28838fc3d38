"""Static instruction mix of the march loops of a sweep kernel in a gfx950 assembly listing
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fopenmp --cuda-device-only -S mf_cheb_fused.hip).
A march loop is a backward branch that spans at least MIN_SPAN instructions (the loop over trips of K super-passes; a kernel
that carries the wide and the narrow body has two).  Counts are those of the loop's text divided by K: per wavefront and
super-pass, rarely taken blocks (Dirichlet rows, skipped stages) included.
usage: python scratch/sweep_isa_mix.py file.s kernel-name-substring [K]"""
import re
import sys

MIN_SPAN = 1500


def kernel_text(txt, pat):
    """(name, lines) of the first kernel whose mangled name contains pat"""
    for m in re.finditer(r"^(_Z\S+):\s*(?:;.*)?$", txt, re.M):
        if pat in m.group(1):
            end = txt.find(".Lfunc_end", m.end())
            return m.group(1), txt[m.end():end].splitlines()
    raise SystemExit(f"no kernel matching {pat!r}")


def classify(op, line):
    c = []
    if op.startswith("v_"):
        c.append("VALU")
        if re.match(r"v_(add|mul|fma)_f64", op):
            c.append("FP64 add/mul/fma")
        if op.startswith(("v_readlane", "v_writelane")):
            c.append("v_readlane/v_writelane")
        if op.startswith("v_readfirstlane"):
            c.append("v_readfirstlane")
        if op.startswith("v_cndmask"):
            c.append("v_cndmask")
        dpp = re.search(r"quad_perm|row_shr|row_shl|row_ror|wave_sh|row_bcast|row_mirror|row_newbcast", line)
        if dpp:
            c.append("DPP")
        elif op.startswith("v_mov") or op.startswith("v_accvgpr"):
            c.append("v_mov")
        if re.match(r"v_div_|v_rcp_f64", op):
            c.append("v_div_* / v_rcp_f64")
    elif op.startswith("s_load") or op.startswith("s_buffer_load"):
        c.append("scalar memory loads")
    elif op == "s_waitcnt":
        c.append("s_waitcnt")
        if "lgkmcnt(0)" in line:
            c.append("s_waitcnt lgkmcnt(0)")
    elif op == "s_barrier":
        c.append("s_barrier")
    elif op.startswith(("s_cbranch", "s_branch")):
        c.append("branches")
    elif op == "s_nop":
        c.append("s_nop")
    elif op.startswith("s_"):
        c.append("SALU")
    elif op.startswith("ds_"):
        c.append("LDS reads" if "read" in op or "load" in op else "LDS writes")
    elif op.startswith("buffer_load"):
        c.append("buffer loads")
    elif op.startswith("buffer_store"):
        c.append("buffer stores")
    elif op.startswith(("scratch_", "global_", "flat_")):
        c.append("scratch / global / flat")
    return c


def main():
    txt = open(sys.argv[1]).read()
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    name, lines = kernel_text(txt, sys.argv[2])
    insts, labels = [], {}
    for ln in lines:
        s = ln.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.L\w+):", s)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        if s.startswith("."):
            continue
        insts.append(s)
    loops = []
    for i, s in enumerate(insts):
        m = re.match(r"s_c?branch\w*\s+(\.L\w+)", s)
        if m and m.group(1) in labels and labels[m.group(1)] <= i and i - labels[m.group(1)] >= MIN_SPAN:
            loops.append((labels[m.group(1)], i))
    # nested backward branches to the same head: keep the widest span per head
    spans = {}
    for h, e in loops:
        spans[h] = max(spans.get(h, e), e)
    print(f"kernel {name}")
    print(f"instructions in the kernel {len(insts)}; march loops found {len(spans)} (in the order of the text)")
    order = ["instructions", "VALU", "FP64 add/mul/fma", "v_readlane/v_writelane", "v_readfirstlane", "v_cndmask", "v_mov", "DPP",
             "v_div_* / v_rcp_f64", "scalar memory loads", "s_waitcnt", "s_waitcnt lgkmcnt(0)", "s_barrier", "SALU", "s_nop", "branches",
             "LDS reads", "LDS writes", "buffer loads", "buffer stores", "scratch / global / flat"]
    for n, (h, e) in enumerate(sorted(spans.items())):
        cnt = {k: 0 for k in order}
        vaddr = set()
        for s in insts[h:e + 1]:
            op = s.split()[0]
            cnt["instructions"] += 1
            for c in classify(op, s):
                cnt[c] += 1
            if op.startswith("buffer_load"):
                vaddr.add(s.split(",")[1].strip())
        kind = "narrow body (a per-lane row in the address)" if len(vaddr) > 2 else "wide body"
        print(f"\nloop {n + 1}: instructions {h} .. {e} of the kernel, {kind}; per super-pass (loop text / {K}):")
        for k in order:
            print(f"  {k:28s} {cnt[k] / K:8.1f}   (loop {cnt[k]})")


if __name__ == "__main__":
    main()
