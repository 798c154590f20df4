#!/usr/bin/env python3
"""Native bf16 aggregation against the up-cast / down-cast a caller needed before
the half-precision entry points existed.

For the synthetic Reddit-sized (h=256, k=32) and products-sized (h=256, k=16)
graphs of bench.py (the same graphs.synthetic_* calls and seed), per direction:

    native    g.forward(data_bf16, sel)            -> bf16
    baseline  g.forward(data_bf16.float(), sel).to(bf16)
              (the casts included: they are the two extra passes the issue
              is about; the fp32 call takes whatever AUTO picks for it)

and likewise g.backward.  The two are timed in alternation, REPS repetitions
each, every repetition the mean of INNER back-to-back calls between two HIP
events; the table gives min, median and spread ((max - min) / median).

    python tools/half_time.py [--out profiles/half_time.txt]
    python tools/half_time.py --baseline-only    # runs on a commit without the *_t entry points
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("reddit", 32), ("products", 16)]
H = 256


def ms_per_call(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, reps, inner):
    """fns: {name: callable}; one repetition of each in turn, reps times."""
    for fn in fns.values():     # plans, workspaces, AUTO choices
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(ms_per_call(fn, inner))
    return times


def row(label, t):
    med = statistics.median(t)
    return (f"{label:<34s} min {min(t):8.3f}  median {med:8.3f}  max {max(t):8.3f} ms  "
            f"spread {100 * (max(t) - min(t)) / med:5.1f} %")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--auto", default="fixed", choices=["fixed", "measure"],
                   help="MAXK_AUTO for the fp32 calls of the baseline (bench.py's default: fixed)")
    p.add_argument("--baseline-only", action="store_true",
                   help="time the up-cast / fp32 / down-cast baseline alone")
    p.add_argument("--graphs", default=",".join(g for g, _ in SHAPES))
    p.add_argument("--out", default=None, help="also write the table to this file")
    args = p.parse_args(argv)
    os.environ["MAXK_AUTO"] = args.auto
    import spgemm_new_amd as S
    from spgemm_new_amd.graphs import (CONFIGS, synthetic_columns, synthetic_indptr,
                                       synthetic_values)
    from spgemm_new_amd.ops import topk_cbsr

    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    lines = [f"# tools/half_time.py --reps {args.reps} --inner {args.inner} --auto {args.auto}"
             f"{' --baseline-only' if args.baseline_only else ''}; "
             f"{torch.cuda.get_device_name(dev)}; ms per call"]
    for graph, k in SHAPES:
        if graph not in args.graphs.split(","):
            continue
        V, E = CONFIGS[graph]
        indptr = synthetic_indptr(V, E, seed=args.seed, device=dev)
        indices = synthetic_columns(indptr, seed=args.seed, self_loops=(graph == "flickr"))
        values = synthetic_values(args.seed, 0, int(indptr[V]), device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed + 1)
        X = torch.rand((V, H), generator=gen, device=dev)
        G = torch.rand((V, H), generator=gen, device=dev).to(bf16)
        data32, sel = topk_cbsr(X, k, order="column")
        data = data32.to(bf16)
        del X, data32
        g = S.MaxKGraph(indptr, indices, values)
        fwd = {"baseline fp32 + casts": lambda: g.forward(data.float(), sel, H).to(bf16)}
        bwd = {"baseline fp32 + casts": lambda: g.backward(G.float(), sel).to(bf16)}
        if not args.baseline_only:
            y, dx = torch.empty((V, H), dtype=bf16, device=dev), torch.empty((V, k), dtype=bf16,
                                                                              device=dev)
            fwd["native bf16"] = lambda: g.forward(data, sel, H, out=y)
            bwd["native bf16"] = lambda: g.backward(G, sel, out=dx)
        lines.append(f"\n{graph}: V={V} E={int(indptr[V])} h={H} k={k}")
        for what, fns in (("forward", fwd), ("backward", bwd)):
            times = alternate(fns, args.reps, args.inner)
            for name, t in times.items():
                lines.append(row(f"  {what:<9s}{name}", t))
            if what == "backward":
                algos = []
                for name, fn in fns.items():
                    fn()
                    algos.append(f"{name}: {g.last_bwd_algo}")
                lines.append(f"  (backward algorithm -- {'; '.join(algos)})")
        if not args.baseline_only:
            lines.append(f"  (forward column blocks, fp32 / bf16: "
                         f"{g._fwd_blocks.get((k, H))} / {g._fwd_blocks.get((k, H, bf16))})")
        del g, fwd, bwd
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
