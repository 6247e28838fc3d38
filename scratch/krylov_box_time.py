# usage: krylov_box_time.py [columns=30] [reps=5]
# The owned-box basis kernels at the shape of a rank of the 2 x 2 x 2 bench run against the contiguous kernels on as many
# entries, one session on one box: BoxPartition((512,)*3, r, (2,2,2), low_ghost_cells=4) gives rank 0 a local box of
# 259^3 nodes of which it owns 256^3 from node 0, and rank 7 one of 261^3 of which it owns 257^3 from node 4 (odd row starts on
# every second row either way).  CGS2 of w against `columns` columns through Context.krylov_orthogonalize (two dots and two update
# launches per call), HIP events per launch (Context.profile_enable), the variants alternating, ns per owned entry and column.
import json, os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import mfmg_amd as M

columns = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ctx = M.Context()
gen = torch.Generator(device='cuda').manual_seed(1)
VARIANTS = {'contiguous': None}
for r in (0, 7):
    p = M.BoxPartition((512,) * 3, r, (2, 2, 2), low_ghost_cells=4)
    VARIANTS[f'rank{r}'] = (p.local_nodes, p.own0, p.own_n, 1)


def entries(box):
    if box is None:
        return 256 ** 3, 256 ** 3
    local, _, own_n, _ = box
    return local[0] * local[1] * local[2], own_n[0] * own_n[1] * own_n[2]


def timed(name, box, kernel):
    n_local, n_owned = entries(box)
    ld = (n_local + 1) // 2 * 2
    V = torch.rand(columns, ld, dtype=torch.float64, device='cuda', generator=gen)
    w0 = torch.rand(n_local, dtype=torch.float64, device='cuda', generator=gen)
    ctx.krylov_orthogonalize(V, w0.clone(), columns, 2, box=box)          # warm-up
    ctx.profile_enable(True, only=kernel + ('_box' if box else ''))
    for _ in range(reps):
        ctx.krylov_orthogonalize(V, w0.clone(), columns, 2, box=box)
    launches, ms, _ = ctx.profile_query(kernel + ('_box' if box else ''))
    ctx.profile_enable(False)
    del V, w0
    torch.cuda.empty_cache()
    return 1e3 * ms / launches, n_owned


result = {}
for kernel in ('basis_dots', 'basis_update'):
    for trip in range(2):                                                 # the variants alternate
        for name, box in VARIANTS.items():
            us, n_owned = timed(name, box, kernel)
            result.setdefault((kernel, name), []).append((us, n_owned))
for (kernel, name), runs in result.items():
    us = min(u for u, _ in runs)
    ref = min(u for u, _ in result[(kernel, 'contiguous')])
    n_owned = runs[0][1]
    print(json.dumps({'kernel': kernel, 'variant': name, 'columns': columns, 'us_per_launch': us, 'runs': [u for u, _ in runs],
                      'owned_entries': n_owned, 'ps_per_entry_and_column': 1e6 * us / n_owned / columns,
                      'ratio_to_contiguous_per_entry': (us / n_owned) / (ref / 256 ** 3)}), flush=True)
