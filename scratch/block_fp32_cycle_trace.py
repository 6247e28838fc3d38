"""Thirteen FP32 block cycles on four float right-hand sides (`material linear`, V(0,1) coarse cycle), nothing else after the setup:
run under `rocprofv3 --kernel-trace` and feed the kernel trace back to this file for the kernel sequence of the last cycle and the
time per kernel over the last ten.  usage: block_fp32_cycle_trace.py [cells] | block_fp32_cycle_trace.py sum <kernel_trace.csv>"""
import collections, csv, os, re, sys

CYCLES, WARM = 10, 3
BLOCK = "mf_laplace_block_f32_kernel"

if len(sys.argv) > 2 and sys.argv[1] == "sum":
    rows = sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    name = lambda r: re.sub(r"\(.*", "", r["Kernel_Name"].replace("void ", "").replace("mfmg::(anonymous namespace)::", "").replace("mfmg::vec::(anonymous namespace)::", "vec::"))
    marks = [i for i, r in enumerate(rows) if BLOCK in r["Kernel_Name"]]
    per = len(marks) // (CYCLES + WARM)
    assert per * (CYCLES + WARM) == len(marks), "the block launches do not divide into the cycles"
    tail = rows[marks[WARM * per]:]                              # from the first block launch of the first timed cycle
    span = (int(tail[-1]["End_Timestamp"]) - int(tail[0]["Start_Timestamp"])) / 1e3
    busy = sum(us(r) for r in tail)
    print(f"block launches/cycle {per}  kernels/cycle {len(tail) / CYCLES:.1f}  span {span / CYCLES:.1f} us/cycle  busy {busy / CYCLES:.1f}  idle {(span - busy) / CYCLES:.1f}")
    acc = collections.OrderedDict()
    for r in tail:
        a = acc.setdefault(name(r), [0, 0.0])
        a[0] += 1
        a[1] += us(r)
    for k, (c, t) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        print(f"{t / CYCLES:9.1f} us/cycle {c / CYCLES:5.1f} x {t / c:8.1f} us  {k[:110]}")
    print("seq (the last cycle):")
    for r in rows[marks[(CYCLES + WARM - 1) * per]:]:
        print(f"  {us(r):8.1f} us  grid {r.get('Grid_Size', '?'):>10}  {name(r)[:110]}")
    sys.exit(0)

import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mfmg_amd as M
cells = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ctx = M.Context()
prob = M.LaplaceProblem((cells,) * 3, "linear", device="cuda")
n = prob.n_dofs
ld = n + (n & 1)
params = {"eigensolver": {"number of eigenvectors": 2}, "agglomeration": {"partitioner": "block", "nx": 2, "ny": 2, "nz": 2},
          "smoother": {"type": "Chebyshev", "degree": 3, "smoothing_range": 20.0, "n_smoothing_steps": 1},
          "solver": {"type": "amg", "amg": {"smoother_degree": 1, "smoothing_range": 4.0, "n_cycles": 1, "aggregate_block": 2,
                                            "pre_smoothing_levels": 0}},
          "is preconditioner": True, "max levels": 2, "fine level precision": "float"}
h = M.Hierarchy(ctx, "HipMatrixFreeMeshEvaluator", prob, params)
B = torch.zeros(4, ld, dtype=torch.float32, device="cuda")
B[:, :n] = torch.rand(4, n, dtype=torch.float32, device="cuda")
X = torch.zeros_like(B)
for _ in range(WARM + CYCLES):
    h.apply_f32_block(B, X)
torch.cuda.synchronize()
print(h.block_info_f32())
