"""Time one MISI iteration on the device: the fused misi_dev (lws_gla.hip) against the same iteration composed from the public
pieces (istft_dev -> torch sum / subtract / add -> stft_dev -> torch abs / divide / multiply), alternating the two in one process.
HIP events around `--iters` iterations, after a warm-up; per-iteration medians and the spread over `--reps`; the result goes to
`--out` (none: it is only printed).
    PYTHONPATH=. python tools/time_misi.py [--iters 20 --reps 9] --out profiles/misi_iteration.json"""
import argparse, json
import numpy as np, torch
import lws_amd

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_misi.py needs a GPU")
# (fsize, fshift, mixtures, sources, frames)
SHAPES = [(512, 128, 64, 2, 500), (512, 128, 64, 4, 500)] if not a.small else [(64, 16, 3, 2, 9)]


def composed(p, c, A, y, n):
    """n iterations from the public calls; returns c_n."""
    B, K, T, F = c.shape
    for i in range(n):
        x = p.istft_dev(c.view(B * K, T, F)).view(B, K, -1)
        e = y - x.sum(dim=1)
        X = p.stft_dev((x + (e / K)[:, None]).view(B * K, -1)).view(B, K, T, F)
        c = X * (A / X.abs())                    # (no zero bins in these inputs: the leanest form the pieces allow)
    return c


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.iters


results = []
for fsize, fshift, B, K, T in SHAPES:
    F = fsize // 2 + 1
    p = lws_amd.lws(fsize, fshift)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    src = torch.randn((B, K, lws_amd._capi.istft_length(T, fsize, fshift, True)), device="cuda", generator=g)
    y = src.sum(dim=1)
    A = p.stft_dev(src.view(B * K, -1)).abs().view(B, K, T, F)
    c0 = torch.polar(A, 2 * np.pi * torch.rand(A.shape, device="cuda", generator=g))
    runs = {"fused": lambda: p.misi_dev(c0, y, a.iters, magnitudes=A),
            "composed": lambda: composed(p, c0, A, y, a.iters)}
    out = {k: fn() for k, fn in runs.items()}
    # same seeded input, same result up to fp32 rounding of two different transform schedules
    rel = float(torch.linalg.vector_norm(out["fused"] - out["composed"]) / torch.linalg.vector_norm(c0))
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):                      # alternate the two
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    row = {"fsize": fsize, "fshift": fshift, "B": B, "K": K, "T": T, "iters": a.iters, "reps": a.reps,
           "rel_l2_fused_vs_composed": rel}
    for k, v in ms.items():
        row[k] = {"median_ms_per_iteration": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    row["composed_over_fused"] = row["composed"]["median_ms_per_iteration"] / row["fused"]["median_ms_per_iteration"]
    results.append(row)
    print(json.dumps(row), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")
