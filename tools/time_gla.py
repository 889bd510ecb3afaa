"""Time one Griffin-Lim iteration on the device: the fused griffin_lim_dev (lws_gla.hip) against the same iteration composed
from the public pieces (istft_dev -> stft_dev -> torch abs / divide / multiply / momentum update), alternating the two in
one process.  HIP events around `--iters` iterations, after a warm-up; per-iteration medians and the spread over `--reps`.
    PYTHONPATH=. python tools/time_gla.py [--iters 20 --reps 9 --out profiles/gla_iteration.json]"""
import argparse, json
import numpy as np, torch
import lws_amd

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--alpha", type=float, default=0.99)
ap.add_argument("--out", default=None)
ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_gla.py needs a GPU")
SHAPES = [(1024, 256, 64, 500), (512, 128, 256, 628)] if not a.small else [(64, 16, 3, 9)]


def composed(p, c, A, n, alpha):
    """n iterations from the public calls; returns t_n."""
    t_prev = None
    for i in range(1, n + 1):
        X = p.stft_dev(p.istft_dev(c))
        t = X * (A / X.abs())                    # (no zero bins in these inputs: the leanest form the pieces allow)
        c = t if i == 1 else torch.add(t, t - t_prev, alpha=alpha)
        t_prev = t
    return t_prev


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.iters


results = []
for fsize, fshift, B, T in SHAPES:
    F = fsize // 2 + 1
    p = lws_amd.lws(fsize, fshift)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    x = torch.randn((B, lws_amd._capi.istft_length(T, fsize, fshift, True)), device="cuda", generator=g)
    A = p.stft_dev(x).abs()
    assert tuple(A.shape) == (B, T, F)
    c0 = torch.polar(A, 2 * np.pi * torch.rand(A.shape, device="cuda", generator=g))
    runs = {"fused": lambda: p.griffin_lim_dev(c0, a.iters, alpha=a.alpha, magnitudes=A),
            "composed": lambda: composed(p, c0, A, a.iters, a.alpha)}
    # same seeded input, same result up to fp32 rounding of two different transform schedules
    d = runs["fused"]() - runs["composed"]()
    rel = float(torch.linalg.vector_norm(d) / torch.linalg.vector_norm(c0))
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):                      # alternate the two
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    row = {"fsize": fsize, "fshift": fshift, "B": B, "T": T, "iters": a.iters, "alpha": a.alpha, "reps": a.reps,
           "rel_l2_fused_vs_composed": rel}
    for k, v in ms.items():
        row[k] = {"median_ms_per_iteration": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    row["speedup_of_medians"] = row["composed"]["median_ms_per_iteration"] / row["fused"]["median_ms_per_iteration"]
    results.append(row)
    print(json.dumps(row), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")
