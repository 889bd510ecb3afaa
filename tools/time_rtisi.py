"""Time RTISI-LA on the device: rtisi_la_dev (k_rtisi of lws_gla.hip; look-ahead 3, 5 iterations, no signal) alternating with
griffin_lim_dev (alpha = 0) at 5 * (3 + 1) iterations on the same stack -- the same number of frame transforms, done by the
throughput-bound batch kernels: the yardstick, not a competitor (it lets every frame see the whole future).  On a short clip the
look-ahead iteration is also composed from the public pieces (istft_dev -> stft_dev -> torch), which is what a caller had before.
HIP events around each call, after a warm-up; medians and the spread over `--reps`.
    PYTHONPATH=. python tools/time_rtisi.py [--reps 9 --out profiles/rtisi_iteration.json]"""
import argparse, json
import numpy as np, torch
import lws_amd

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--look-ahead", type=int, default=3)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--clip", type=int, default=24, help="frames of the short clip the composition is timed on (0: skip it)")
ap.add_argument("--out", default=None)
ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_rtisi.py needs a GPU")
SHAPES = [(512, 128, 256, 628), (1024, 256, 64, 500)] if not a.small else [(64, 16, 3, 12)]
LA, n = a.look_ahead, a.iters


def composed(p, c0, A):
    """rtisi_la from the public calls, on the uncut timeline (the cuts of perfectrec as a mask); returns c."""
    N, hop = p.fsize, p.fshift
    B, T, F = c0.shape
    c = c0.clone()
    total = hop * (T - 1) + N
    keep = torch.ones(total, device=c.device)
    if p.perfectrec:
        keep[:N - hop if N % hop == 0 else N - N % hop] = 0
        keep[total - (N - hop):] = 0
    done = torch.zeros((B, total), device=c.device)
    for m in range(T):
        last = min(m + LA, T - 1)
        lo, hi = hop * m, hop * last + N
        for it in range(n):
            y = (done[:, lo:hi] + lws_amd.istft_dev(c[:, m:last + 1], hop, p.swin, perfectrec=False)) * keep[lo:hi]
            X = lws_amd.stft_dev(y, N, hop, p.awin, perfectrec=False)
            c[:, m:last + 1] = X * (A[:, m:last + 1] / X.abs())      # (no zero bins in these inputs)
        done[:, lo:lo + N] += lws_amd.istft_dev(c[:, m:m + 1], hop, p.swin, perfectrec=False)
    return c


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v, transforms):
    return {"median_ms": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
            "median_ns_per_frame_transform": float(np.median(v)) * 1e6 / transforms}


results = []
for fsize, fshift, B, T in SHAPES:
    F = fsize // 2 + 1
    p = lws_amd.lws(fsize, fshift)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    x = torch.randn((B, lws_amd._capi.istft_length(T, fsize, fshift, True)), device="cuda", generator=g)
    X = p.stft_dev(x)
    assert tuple(X.shape) == (B, T, F)
    c0 = X * torch.polar(torch.ones_like(X.real), 0.3 * torch.randn(X.shape, device="cuda", generator=g))
    A = X.abs()
    runs = {"rtisi_la": lambda: p.rtisi_la_dev(c0, n, look_ahead=LA, magnitudes=A),
            "griffin_lim": lambda: p.griffin_lim_dev(c0, n * (LA + 1), alpha=0.0, magnitudes=A)}
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):                      # alternate the two
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    # forward and inverse transforms of one frame: n (LA + 1) of each per frame, less the look-aheads the end cuts short
    transforms = 2 * B * n * sum(min(m + LA, T - 1) - m + 1 for m in range(T))
    row = {"fsize": fsize, "fshift": fshift, "B": B, "T": T, "iterations": n, "look_ahead": LA, "reps": a.reps,
           "rtisi_la": stats(ms["rtisi_la"], transforms), "griffin_lim": stats(ms["griffin_lim"], 2 * B * T * n * (LA + 1))}
    row["rtisi_over_griffin_lim_of_medians"] = row["rtisi_la"]["median_ms"] / row["griffin_lim"]["median_ms"]
    if a.clip:
        Tc = min(a.clip, T)
        cc, Ac = c0[:, :Tc].contiguous(), A[:, :Tc].contiguous()
        short = {"rtisi_la": lambda: p.rtisi_la_dev(cc, n, look_ahead=LA, magnitudes=Ac), "composed": lambda: composed(p, cc, Ac)}
        d = short["rtisi_la"]() - short["composed"]()
        row["clip"] = {"T": Tc, "rel_l2_kernel_vs_composed": float(torch.linalg.vector_norm(d) / torch.linalg.vector_norm(cc))}
        torch.cuda.synchronize()
        cms = {k: [] for k in short}
        for _ in range(a.reps):
            for k, fn in short.items():
                cms[k].append(timed(fn))
        tc = 2 * B * n * sum(min(m + LA, Tc - 1) - m + 1 for m in range(Tc))
        for k, v in cms.items():
            row["clip"][k] = stats(v, tc)
        row["clip"]["speedup_of_medians"] = row["clip"]["composed"]["median_ms"] / row["clip"]["rtisi_la"]["median_ms"]
    results.append(row)
    print(json.dumps(row), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")
